"""GPU tests of dfm_news_batch (include/dfm_hip.h; csrc/news.hip) against the expectation model of tests/news_expect.py (the
forecast's expectation model for the three conditional means, the oracle's pass over the covariance panels for the weights) at
1e-9: the fused balanced pass, the time-chunked recursion with odd N, the tile route at r = 20, the companion routes, singular Q;
then the output invariants, the device entry, a call across the 8192-replicate slice boundary, api.news on the Stock-Watson panel
with groups and bootstrap bands, and the status codes.  tests/test_gpu_post_geometry.py covers the cell and gamma kernels'
launch classes (column-pair blocks, LDS cap, every bucket, targets at chunk edges and far beyond T)."""
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.news_expect import expect

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _batch(B, N, T, r, missing, first=0):
    reps = [ko.synth_replicate(first + b, N, T, r, missing=missing) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    st = {k: np.stack([p[k] for _, p in reps]) for k in reps[0][1]}
    st["mu0"] = st["mu0"] + 0.3
    return panel, st


def _varp_batch(B, N, T, r, p, missing):
    xs, qs = [], []
    for b in range(B):
        x = vo.synth_varp(b, N, T, r, p, missing=missing)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        xs.append(x); qs.append(dict(q, A=q["Avar"]))
    return np.stack(xs), {k: np.stack([q[k] for q in qs]) for k in KEYS}


def _old_of(new, seed, last=2):
    """The old vintage: the last `last` rows not yet released, one cell revised afterwards, one gap filled."""
    rng = np.random.default_rng(seed)
    B, T, N = new.shape
    old = new.copy()
    old[:, T - last:, :] = np.nan
    new = new.copy()
    for b in range(B):
        obs = np.argwhere(~np.isnan(old[b]))
        t, i = obs[rng.integers(len(obs))]
        new[b, t, i] += 0.5                                   # a revision
        t, i = obs[rng.integers(len(obs))]
        old[b, t, i] = np.nan                                 # a gap the new vintage fills
    return old, new


def _run(ctx, old, new, st, targets, p=1, mean=None, sd=None, what="", **kw):
    got = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], targets, mean=mean, sd=sd, **kw)
    B, T, N = new.shape
    for b in range(B):
        e = expect(old[b], new[b], *[st[k][b] for k in KEYS], targets, p=p, mean=None if mean is None else mean[b],
                   sd=None if sd is None else sd[b])
        for key in ("yhat", "impact", "news", "weight"):
            _close(got[key][b], e[key], f"{what} b={b} {key}")
    # invariants: the impacts sum to y_new - y_rev; weight is 0 off the new vintage's cells
    y = got["yhat"]
    d = y[:, 2] - y[:, 1]
    s = got["impact"].sum(axis=2)
    assert np.all(np.abs(s - d) <= 1e-9 * np.maximum(1.0, np.abs(y[:, 2]))), f"{what}: sum of impacts"
    off = np.broadcast_to(np.isnan(new)[:, None], got["weight"].shape)
    assert np.all(got["weight"][off] == 0.0), f"{what}: weight off Omega_new"
    return got


@pytest.mark.parametrize("scaled", [False, True])
def test_fused_balanced(ctx, scaled):
    B, N, T, r = 2, 60, 90, 8
    new, st = _batch(B, N, T, r, 0.0)
    old, new = _old_of(new, 1)
    assert not np.isnan(new).any()                            # Omega_new complete: the fused balanced pass
    rng = np.random.default_rng(2)
    mean = rng.standard_normal((B, N)) if scaled else None
    sd = rng.uniform(0.5, 3.0, (B, N)) if scaled else None
    targets = [(T - 1, 3), (T + 2, 0), (T - 2, 59), (10, 7)]
    _run(ctx, old, new, st, targets, mean=mean, sd=sd, what=f"fused scaled={scaled}")


def test_chunked_missing_odd_n(ctx):
    B, N, T, r = 2, 139, 222, 8
    new, st = _batch(B, N, T, r, 0.1, first=20)
    new[:, -1, :70] = np.nan                                  # a ragged edge
    old, new = _old_of(new, 3)
    _run(ctx, old, new, st, [(T - 1, 100), (T + 3, 5)], what="chunked odd N")
    nf, nt = ctx.chunk_fallbacks()
    assert nt == B * 2, "the weight passes did not run on the time-chunked recursion"


def test_tile_route_r20(ctx):
    new, st = _batch(1, 120, 150, 20, 0.1, first=40)
    old, new = _old_of(new, 4)
    _run(ctx, old, new, st, [(149, 2), (152, 119)], what="r=20")


@pytest.mark.parametrize("r,p", [(3, 2), (4, 4)])
def test_varp(ctx, r, p):
    new, st = _varp_batch(2, 40, 100, r, p, 0.1)
    old, new = _old_of(new, p)
    rng = np.random.default_rng(p)
    mean, sd = rng.standard_normal((2, 40)), rng.uniform(0.5, 2.0, (2, 40))
    _run(ctx, old, new, st, [(99, 1), (104, 39), (50, 20)], p=p, mean=mean, sd=sd, what=f"VAR({p}) r={r}")


def test_singular_q(ctx):
    new, st = _batch(2, 50, 80, 4, 0.1, first=60)
    for b in range(2):
        v = np.linalg.cholesky(st["Q"][b])[:, :3]
        st["Q"][b] = v @ v.T                                  # rank 3
    old, new = _old_of(new, 5)
    _run(ctx, old, new, st, [(79, 0), (82, 49)], what="singular Q", singular_q=True)


def test_no_news_and_device_entry(ctx):
    import torch
    new, st = _batch(2, 64, 70, 4, 0.15, first=80)
    old, new = _old_of(new, 6)
    tg = [(69, 3), (72, 0)]
    full = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], tg)
    lean = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], tg, want_news=False, want_weight=False)
    assert lean["news"] is None and lean["weight"] is None
    assert np.array_equal(lean["impact"], full["impact"]) and np.array_equal(lean["yhat"], full["yhat"])
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.news_batch(t(old), t(new), *[t(st[k]) for k in KEYS], tg)
    ctx.synchronize()
    for key in full:
        assert np.array_equal(got[key].cpu().numpy(), full[key]), key
    rev = np.where(np.isnan(old), np.nan, new)                # no news: impacts exactly 0, y_new = y_rev
    o = ctx.news_batch_host(old, rev, *[st[k] for k in KEYS], tg)
    assert np.all(o["impact"] == 0.0) and np.all(o["news"] == 0.0)
    assert np.array_equal(o["yhat"][:, 1], o["yhat"][:, 2])


def test_slices_of_8192(ctx):
    B, N, T, r = 2, 6, 12, 2
    new, st = _batch(B, N, T, r, 0.1, first=95)
    old, new = _old_of(new, 7)
    G = 4200                                                  # 8400 weight passes: the second slice starts at b = 1, g = 3992
    targets = [(t, i) for t in range(T + 2) for i in range(N)] * 60
    targets = targets[:G]
    got = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], targets)
    for b, gs in ((0, [0, 4199]), (1, [0, 3991, 3992, 3993, 4199])):
        sub = [targets[g] for g in gs]
        e = expect(old[b], new[b], *[st[k][b] for k in KEYS], sub)
        for q, g in enumerate(gs):
            _close(got["weight"][b, g], e["weight"][q], f"slices b={b} g={g} weight")
            _close(got["impact"][b, g], e["impact"][q], f"slices b={b} g={g} impact")
            _close(got["yhat"][b, :, g], e["yhat"][:, q], f"slices b={b} g={g} yhat")


def _sw_model(lags):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, lags)


def test_stock_watson_news(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=8, seed=11)
    params = {k: v.copy() for k, v in m.em_params.items()}
    cols = api._forecast_inputs(m, 224)[0]
    tg = [(int(cols[0]), 224), (int(cols[5]), 226)]
    groups = {"first": cols[:50], "rest": cols[50:]}
    o = api.news(m, 222, 224, tg, groups=groups, quantiles=[0.1, 0.5, 0.9], ctx=ctx)
    assert all(np.array_equal(params[k], m.em_params[k]) for k in params), "news changed m.em_params"
    assert np.array_equal(o["rows"], np.arange(3, 225)) and np.array_equal(o["cols"], cols)
    f_old = api.forecast(m, 4, through=222, ctx=ctx)              # y_old / y_new are the forecasts of the two vintages
    f_new = api.forecast(m, 2, through=224, ctx=ctx)
    j0, j5 = 0, 5
    _close(o["y_old"], np.array([f_old["x"][224 - 3, j0], f_old["x"][226 - 3, j5]]), "y_old vs forecast")
    _close(o["y_new"], np.array([f_new["x"][224 - 3, j0], f_new["x"][226 - 3, j5]]), "y_new vs forecast")
    assert np.array_equal(o["y_rev"], o["y_old"]), "pseudo real-time vintages have no revisions"
    _close(o["impact"].sum(axis=1), o["news_effect"], "sum of impacts")
    _close(o["groups"]["first"] + o["groups"]["rest"], o["news_effect"], "groups")
    assert o["impact_bands"].shape == (3, 2, cols.size) and o["revision_bands"].shape == (3, 2)
    assert np.all(o["impact_bands"][0] <= o["impact_bands"][2]) and np.all(o["revision_bands"][0] <= o["revision_bands"][2])
    nw = o["news"]
    assert np.all(nw[:220] == 0.0) and np.any(nw[-2:] != 0.0), "news outside the released rows"
    cells, z, mu, sd = api._forecast_inputs(m, 224)
    rp = m.replicates["params"]
    zo = np.where(np.arange(z.shape[0])[:, None] < 222 - 2, z, np.nan)
    e = expect(zo, z, *[rp[k][3] for k in KEYS], [(221, 0), (223, 5)], mean=mu, sd=sd)
    got = ctx.news_batch_host(zo[None], z[None], *[rp[k][3:4] for k in KEYS], [(221, 0), (223, 5)], mean=mu[None],
                              sd=sd[None])
    for key in ("yhat", "impact", "weight"):
        _close(got[key][0], e[key], f"SW replicate 3 {key}")


def test_status_codes(ctx):
    import ctypes
    from dynamic_factor_models_amd import _lib
    new, st = _batch(1, 20, 30, 2, 0.0)
    old, new = _old_of(new, 8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    y, imp = np.empty((1, 3, 1)), np.empty((1, 1, 20))
    args = [ptr(np.ascontiguousarray(st[k])) for k in KEYS]

    def call(G, t, i, o=old, yo=y, mean=None, sd=None):
        tt, ti = np.array([t], np.int32), np.array([i], np.int32)
        return ctx._lib.dfm_news_batch(ctx._h, 1, 30, 20, 2, 1, ptr(o), ptr(new), *args, mean, sd, G, ptr(tt), ptr(ti),
                                       None if yo is None else ptr(yo), ptr(imp), None, None, 1)
    assert call(0, 29, 0) == -1                               # G < 1: DFM_E_DIMS
    assert call(1, -1, 0) == -1                               # target before row 0
    assert call(1, 29, 20) == -1                              # target column outside [0, N)
    assert call(1, 29, 0, yo=None) == -3                      # yhat NULL: DFM_E_NULL
    assert call(1, 29, 0, mean=ptr(st["R"])) == -3            # mean without sd
    assert call(1, 29, 0, sd=ptr(st["R"])) == -3              # sd without mean
    assert call(1, 33, 0) == 0
    bad = old.copy()
    nan_in_new = np.argwhere(np.isnan(old[0]) == False)[0]    # a cell observed in old ...
    nw = new.copy()
    nw[0, nan_in_new[0], nan_in_new[1]] = np.nan              # ... missing in new
    with pytest.raises(_lib.DfmError) as ei:
        ctx.news_batch_host(bad, nw, *[st[k] for k in KEYS], [(29, 0)])
    assert ei.value.code == -8
    ok = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], [(29, 0)])   # the bit was reported once
    assert np.all(np.isfinite(ok["impact"]))
