"""GPU tests of dfm_forecast_batch (include/dfm_hip.h; csrc/forecast.hip) against the expectation model of
tests/forecast_expect.py (the oracle's smoother pass over the panel with H all-missing rows appended, and the header's cell
formulas) at 1e-9: the p = 1 routes (fused balanced pass, time-chunked recursion with the odd-N pad, the tile route at r = 20,
covariance form), the companion routes at p > 1, the invariants of the outputs, api.forecast on the Stock-Watson panel and its
bootstrap bands, and the status codes.  tests/test_gpu_post_geometry.py covers the fill kernel's launch classes (series blocks,
LDS cap, buckets r = 1 .. 32, long horizons)."""
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.forecast_expect import expect

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
    return panel, st


def _varp_batch(B, N, T, r, p, missing):
    xs, qs = [], []
    for b in range(B):
        x = vo.synth_varp(b, N, T, r, p, missing=missing)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        xs.append(x); qs.append(dict(q, A=q["Avar"]))
    return np.stack(xs), {k: np.stack([q[k] for q in qs]) for k in KEYS}


def _check(got, panel, st, H, p=1, mean=None, sd=None, what=""):
    for b in range(panel.shape[0]):
        e = expect(panel[b], *[st[k][b] for k in KEYS], H, p=p, mean=None if mean is None else mean[b],
                   sd=None if sd is None else sd[b])
        tag = f"{what} b={b}"
        _close(got["xhat"][b], e["xhat"], tag + " xhat")
        _close(got["f"][b], e["f"], tag + " f")
        if got["xvar"] is not None:
            _close(got["xvar"][b], e["xvar"], tag + " xvar")
        if got["common"] is not None:
            _close(got["common"][b], e["common"], tag + " common")
        if got["P"] is not None:
            _close(got["P"][b], e["P"], tag + " P")
        assert abs(got["loglik"][b] - e["loglik"]) <= TOL * abs(e["loglik"]), (tag, got["loglik"][b], e["loglik"])


def _fc(ctx, panel, st, H, **kw):
    return ctx.forecast_batch_host(panel, *[st[k] for k in KEYS], H, **kw)


@pytest.mark.parametrize("r", [1, 4, 8])
@pytest.mark.parametrize("H", [0, 1, 12])
def test_p1_balanced(ctx, r, H):
    panel, st = _batch(3, 60, 90, r, 0.0)
    got = _fc(ctx, panel, st, H)
    _check(got, panel, st, H, what=f"r={r} H={H}")
    _, _, ll = ctx.ks_pass_batch_host(panel, *[st[k] for k in KEYS])
    assert np.array_equal(got["loglik"], ll), "loglik differs from the plain pass on the unpadded panel"


@pytest.mark.parametrize("r", [4, 8])
def test_p1_missing_odd_n_chunked(ctx, r):
    B, N, T, H = 3, 139, 222, 8
    panel, st = _batch(B, N, T, r, 0.1, first=20)
    panel[:, -1, :70] = np.nan                               # a ragged edge
    got = _fc(ctx, panel, st, H)
    nf, nt = ctx.chunk_fallbacks()
    assert nt == B, "the pass did not run on the time-chunked recursion"
    _check(got, panel, st, H, what=f"r={r} missing odd N")
    _, _, ll = ctx.ks_pass_batch_host(panel, *[st[k] for k in KEYS])
    np.testing.assert_allclose(got["loglik"], ll, rtol=TOL)


def test_p1_r20_missing_tile_route(ctx):
    panel, st = _batch(2, 120, 150, 20, 0.1, first=40)
    got = _fc(ctx, panel, st, 6)
    _check(got, panel, st, 6, what="r=20")


def test_p1_singular_q(ctx):
    panel, st = _batch(2, 50, 80, 4, 0.1, first=60)
    got = _fc(ctx, panel, st, 5, singular_q=True)
    _check(got, panel, st, 5, what="singular Q")


@pytest.mark.parametrize("r,p", [(3, 2), (4, 4), (2, 3)])
@pytest.mark.parametrize("missing", [0.0, 0.1])
def test_varp(ctx, r, p, missing):
    panel, st = _varp_batch(2, 40, 100, r, p, missing)
    H = 7
    got = _fc(ctx, panel, st, H)
    _check(got, panel, st, H, p=p, what=f"r={r} p={p}")
    _, _, ll = ctx.ks_pass_varp_batch_host(panel, *[st[k] for k in ("Lam", "R", "A", "Q", "mu0", "P0")])
    np.testing.assert_allclose(got["loglik"], ll, rtol=TOL)
    nf, nt = ctx.chunk_fallbacks()
    print(f"VAR({p}) r={r} missing={missing}: chunk fallbacks {nf} of {nt}")


@pytest.mark.parametrize("r,p", [(4, 1), (3, 2)])
def test_invariants(ctx, r, p):
    import torch
    if p == 1:
        panel, st = _batch(3, 64, 70, r, 0.15, first=80)
    else:
        panel, st = _varp_batch(3, 64, 70, r, p, 0.15)
    H = 5
    full = _fc(ctx, panel, st, H)
    obs = ~np.isnan(panel)
    T = panel.shape[1]
    assert np.array_equal(full["xhat"][:, :T][obs], panel[obs]), "observed cells of xhat are not bit-exact"
    assert np.all(full["xvar"][:, :T][obs] == 0.0)
    lean = _fc(ctx, panel, st, H, want_var=False, want_common=False, want_P=False)
    assert np.array_equal(lean["xhat"], full["xhat"]) and np.array_equal(lean["f"], full["f"])
    again = _fc(ctx, panel, st, H)
    for k in ("xhat", "xvar", "common", "f", "P", "loglik"):
        assert np.array_equal(again[k], full[k]), k
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.forecast_batch(t(panel), *[t(st[k]) for k in KEYS], H)
    ctx.synchronize()
    for k in ("xhat", "xvar", "common", "f", "P", "loglik"):
        assert np.array_equal(got[k].cpu().numpy(), full[k]), f"_dev vs host: {k}"


def test_mean_sd_unstandardise(ctx):
    panel, st = _batch(2, 30, 60, 3, 0.1, first=90)
    rng = np.random.default_rng(3)
    mean = rng.standard_normal((2, 30)); sd = rng.uniform(0.5, 3.0, (2, 30))
    H = 4
    got = _fc(ctx, panel, st, H, mean=mean, sd=sd)
    _check(got, panel, st, H, mean=mean, sd=sd, what="mean/sd")
    plain = _fc(ctx, panel, st, H)
    obs = np.concatenate([~np.isnan(panel), np.zeros((2, H, 30), bool)], axis=1)
    _close(got["common"], mean[:, None, :] + sd[:, None, :] * plain["common"], "common in data units")
    _close(got["xhat"], np.where(obs, mean[:, None, :] + sd[:, None, :] * plain["xhat"], got["common"]), "xhat in data units")
    _close(got["xvar"], sd[:, None, :] ** 2 * plain["xvar"], "xvar in data units")


def _sw_model(lags):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, lags)


@pytest.mark.parametrize("lags", [1, 4])
def test_stock_watson_nowcast(ctx, lags):
    from dynamic_factor_models_amd import api
    m = _sw_model(lags)
    api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=lags, ctx=ctx)
    params = {k: v.copy() for k, v in m.em_params.items()}
    H = 8
    o = api.forecast(m, H, through=224, ctx=ctx)
    assert all(np.array_equal(params[k], m.em_params[k]) for k in params), "forecast changed m.em_params"
    incl = m.inclcode == 1
    xw = m.data[2:216][:, incl]
    z, sd = api.standardize_data(xw)
    enough = (~np.isnan(z)).sum(axis=0) >= 20
    cols = np.nonzero(incl)[0][enough]
    assert np.array_equal(o["cols"], cols) and np.array_equal(o["rows"], np.arange(3, 224 + H + 1))
    mu = (np.nansum(xw, axis=0) / (~np.isnan(xw)).sum(axis=0))[enough]
    sd = sd[0][enough]
    x = (m.data[2:224][:, cols] - mu) / sd
    A = params["Avar"] if lags > 1 else params["A"]
    e = expect(x, params["Lam"], params["R"], A, params["Q"], params["mu0"], params["P0"], H, p=lags, mean=mu, sd=sd)
    _close(o["x"], e["xhat"], "x")
    _close(o["x_sd"], np.sqrt(e["xvar"]), "x_sd")
    _close(o["common"], e["common"], "common")
    _close(o["factor"], e["f"], "factor")
    _close(o["factor_cov"], e["Pfull"], "factor_cov")
    assert abs(o["loglik"] - e["loglik"]) <= TOL * abs(e["loglik"])
    assert np.isnan(x[-1]).any() and np.all(np.isfinite(o["x"]))


def test_bootstrap_bands(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=32, seed=11)
    H, q = 6, np.array([0.05, 0.5, 0.95])
    o = api.forecast(m, H, through=224, quantiles=q, ctx=ctx)
    assert o["bands"].shape == (3, H, o["cols"].size)
    cols = o["cols"]
    incl = m.inclcode == 1
    xw = m.data[2:216][:, incl]
    n = (~np.isnan(xw)).sum(axis=0)
    _, sd = api.standardize_data(xw)
    enough = n >= 20
    mu, sd = (np.nansum(xw, axis=0) / n)[enough], sd[0][enough]
    z = (m.data[2:224][:, cols] - mu) / sd
    rp = m.replicates["params"]
    per = []
    for b in range(32):
        one = ctx.forecast_batch_host(z[None], *[rp[k][b:b + 1] for k in KEYS], H, mean=mu[None], sd=sd[None])
        per.append(one["xhat"][0, -H:])
    per = np.stack(per)
    srt = np.sort(per, axis=0)
    for j, qq in enumerate(q):
        k = int(np.ceil(qq * 32)) - 1
        _close(o["bands"][j], srt[k], f"band q={qq}")
    assert np.all(np.diff(o["bands"], axis=0) >= 0.0)


def test_status_codes(ctx):
    import ctypes
    from dynamic_factor_models_amd import _lib
    panel, st = _batch(1, 20, 30, 2, 0.0)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    xh, f = np.empty((1, 40, 20)), np.empty((1, 40, 2))
    args = [ptr(panel)] + [ptr(np.ascontiguousarray(st[k])) for k in KEYS]
    rc = ctx._lib.dfm_forecast_batch(ctx._h, 1, 30, 20, 2, 1, -1, *args, None, None, ptr(xh), None, None, ptr(f), None, None, 0)
    assert rc == -1                                          # H < 0: DFM_E_DIMS
    # r p > 32: whatever dfm_ks_pass_varp_batch says for the same shape
    r, p = 9, 4
    x, stv = _varp_batch(1, 20, 30, 3, 2, 0.0)
    big = dict(Lam=np.ones((1, 20, r)), R=np.ones((1, 20)), A=np.zeros((1, r, r * p)), Q=np.tile(np.eye(r), (1, 1, 1)),
               mu0=np.zeros((1, r * p)), P0=np.tile(np.eye(r * p), (1, 1, 1)))
    with pytest.raises(_lib.DfmError) as want:
        ctx.ks_pass_varp_batch_host(x, *[big[k] for k in KEYS])
    with pytest.raises(_lib.DfmError) as got:
        ctx.forecast_batch_host(x, *[big[k] for k in KEYS], 3)
    assert got.value.code == want.value.code
    bad = panel.copy(); bad[0, 5, 3] = np.nan
    for lags in (1, 2):
        if lags == 1:
            with pytest.raises(_lib.DfmError) as ei:
                ctx.forecast_batch_host(bad, *[st[k] for k in KEYS], 3, may_have_missing=False)
        else:
            xb = x.copy(); xb[0, 5, 3] = np.nan
            with pytest.raises(_lib.DfmError) as ei:
                ctx.forecast_batch_host(xb, *[stv[k] for k in KEYS], 3, may_have_missing=False)
        assert ei.value.code == -4, lags                     # DFM_E_MISSING
