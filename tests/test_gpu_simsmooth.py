"""GPU tests of dfm_simsmooth_batch (include/dfm_hip.h; csrc/simsmooth.hip) against the expectation model of
tests/simsmooth_expect.py (the header's steps on the header's random stream, the oracle's pass for the smoothed mean) at 1e-9:
the fused balanced pass, the time-chunked recursion with odd N, the tile route at r = 20, singular Q, the companion routes, with
and without the horizon and mean / sd; then f_draw without x_draw, the first_draw split, a call across the 8192-replicate slice
boundary, the draws' moments against dfm_forecast_batch, api.draw_paths on the Stock-Watson panel, parameter draws, and the
status codes.  tests/test_gpu_post_geometry.py covers the cell kernels' launch classes (column-pair blocks, LDS cap, every
loadings bucket, long horizons)."""
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.simsmooth_expect import draw

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
SEED = 20261016


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
    st["mu0"] = st["mu0"] + 0.3                               # a non-zero prior mean
    return panel, st


def _varp_batch(B, N, T, r, p, missing):
    xs, qs = [], []
    for b in range(B):
        x = vo.synth_varp(b, N, T, r, p, missing=missing)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        xs.append(x); qs.append(dict(q, A=q["Avar"]))
    return np.stack(xs), {k: np.stack([q[k] for q in qs]) for k in KEYS}


def _ss(ctx, panel, st, D, H, **kw):
    return ctx.simsmooth_batch_host(panel, *[st[k] for k in KEYS], D, H, **kw)


def _check(got, panel, st, H, p=1, seed=SEED, first_draw=0, mean=None, sd=None, which=None, what=""):
    B, D = got["f"].shape[:2]
    for b in range(B):
        for d in (range(D) if which is None else which):
            f, xd = draw(panel[b], *[st[k][b] for k in KEYS], H, p, seed, first_draw, d, b,
                         mean=None if mean is None else mean[b], sd=None if sd is None else sd[b])
            _close(got["f"][b, d], f, f"{what} b={b} d={d} f")
            if got["x"] is not None:
                _close(got["x"][b, d], xd, f"{what} b={b} d={d} x")


@pytest.mark.parametrize("H", [0, 6])
@pytest.mark.parametrize("scaled", [False, True])
def test_fused_balanced(ctx, H, scaled):
    B, N, T, r, D = 2, 60, 90, 8, 3
    panel, st = _batch(B, N, T, r, 0.0)
    rng = np.random.default_rng(1)
    mean = rng.standard_normal((B, N)) if scaled else None
    sd = rng.uniform(0.5, 3.0, (B, N)) if scaled else None
    got = _ss(ctx, panel, st, D, H, seed=SEED, mean=mean, sd=sd)
    _check(got, panel, st, H, mean=mean, sd=sd, what=f"fused H={H} scaled={scaled}")
    if not scaled:
        obs = np.broadcast_to(panel[:, None], (B, D, T, N))
        assert np.array_equal(got["x"][:, :, :T], obs), "observed cells are not the data bit for bit"


@pytest.mark.parametrize("H", [0, 8])
def test_chunked_missing_odd_n(ctx, H):
    B, N, T, r, D = 2, 139, 222, 8, 2
    panel, st = _batch(B, N, T, r, 0.1, first=20)
    panel[:, -1, :70] = np.nan                               # a ragged edge
    got = _ss(ctx, panel, st, D, H, seed=SEED + 1)
    nf, nt = ctx.chunk_fallbacks()
    assert nt == B * D, "the pass did not run on the time-chunked recursion"
    _check(got, panel, st, H, seed=SEED + 1, what=f"chunked H={H}")


def test_tile_route_r20_missing(ctx):
    panel, st = _batch(1, 120, 150, 20, 0.1, first=40)
    got = _ss(ctx, panel, st, 2, 6, seed=SEED + 2)
    _check(got, panel, st, 6, seed=SEED + 2, what="r=20")


def test_singular_q(ctx):
    panel, st = _batch(2, 50, 80, 4, 0.1, first=60)
    for b in range(2):
        v = np.linalg.cholesky(st["Q"][b])[:, :3]
        st["Q"][b] = v @ v.T                                  # rank 3
    got = _ss(ctx, panel, st, 2, 5, seed=SEED + 3, singular_q=True)
    _check(got, panel, st, 5, seed=SEED + 3, what="singular Q")


@pytest.mark.parametrize("r,p", [(3, 2), (4, 4)])
@pytest.mark.parametrize("H", [0, 7])
def test_varp(ctx, r, p, H):
    panel, st = _varp_batch(2, 40, 100, r, p, 0.1)
    rng = np.random.default_rng(p)
    mean, sd = rng.standard_normal((2, 40)), rng.uniform(0.5, 2.0, (2, 40))
    got = _ss(ctx, panel, st, 2, H, seed=SEED + p, mean=mean, sd=sd)
    _check(got, panel, st, H, p=p, seed=SEED + p, mean=mean, sd=sd, what=f"VAR({p}) r={r}")


def test_f_draw_without_x_and_device_entry(ctx):
    import torch
    panel, st = _batch(2, 64, 70, 4, 0.15, first=80)
    full = _ss(ctx, panel, st, 4, 5, seed=SEED + 5)
    lean = _ss(ctx, panel, st, 4, 5, seed=SEED + 5, want_x=False)
    assert lean["x"] is None and np.array_equal(lean["f"], full["f"]), "f_draw depends on whether x_draw is taken"
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.simsmooth_batch(t(panel), *[t(st[k]) for k in KEYS], 4, 5, seed=SEED + 5)
    ctx.synchronize()
    assert np.array_equal(got["f"].cpu().numpy(), full["f"]) and np.array_equal(got["x"].cpu().numpy(), full["x"])


def test_first_draw_split_is_bit_exact(ctx):
    panel, st = _batch(2, 40, 60, 3, 0.1, first=90)
    whole = _ss(ctx, panel, st, 6, 4, seed=SEED + 6, first_draw=10)
    part = _ss(ctx, panel, st, 3, 4, seed=SEED + 6, first_draw=13)
    assert np.array_equal(whole["f"][:, 3:], part["f"]) and np.array_equal(whole["x"][:, 3:], part["x"])
    _check(part, panel, st, 4, seed=SEED + 6, first_draw=13, which=[0, 2], what="first_draw = 13")


def test_slices_of_8192(ctx):
    B, D, H = 2, 4200, 2                                      # 8400 pass replicates: the second slice starts at b = 1, d = 3992
    panel, st = _batch(B, 6, 12, 2, 0.1, first=95)
    got = _ss(ctx, panel, st, D, H, seed=SEED + 7)
    for b, ds in ((0, [0, 4199]), (1, [0, 3991, 3992, 3993, 4199])):
        sub = dict(f=got["f"][b:b + 1], x=got["x"][b:b + 1])
        for d in ds:
            f, xd = draw(panel[b], *[st[k][b] for k in KEYS], H, 1, SEED + 7, 0, d, b)
            _close(sub["f"][0, d], f, f"slices b={b} d={d} f")
            _close(sub["x"][0, d], xd, f"slices b={b} d={d} x")


def test_moments_match_the_forecast(ctx):
    T, N, r, H, D = 60, 30, 3, 4, 8192
    panel, st = _batch(1, N, T, r, 0.1, first=99)
    got = _ss(ctx, panel, st, D, H, seed=SEED + 8)
    fc = ctx.forecast_batch_host(panel, *[st[k] for k in KEYS], H)
    il = np.tril_indices(r)
    diag = np.nonzero(il[0] == il[1])[0]
    Pd = fc["P"][0][:, diag]                                  # Var[f_t | X], t = 0 .. T+H-1
    f = got["f"][0]
    z_mean = (f.mean(0) - fc["f"][0]) / np.sqrt(Pd / D)
    z_var = (f.var(0, ddof=1) / Pd - 1.0) / np.sqrt(2.0 / D)
    assert np.abs(z_mean).max() < 5.0 and np.abs(z_var).max() < 5.0, (np.abs(z_mean).max(), np.abs(z_var).max())
    x = got["x"][0]
    xv = fc["xvar"][0]
    drawn = xv > 0.0
    obs = ~drawn
    assert np.all(x[:, obs] == fc["xhat"][0][obs])
    zx_mean = (x.mean(0)[drawn] - fc["xhat"][0][drawn]) / np.sqrt(xv[drawn] / D)
    zx_var = (x.var(0, ddof=1)[drawn] / xv[drawn] - 1.0) / np.sqrt(2.0 / D)
    assert np.abs(zx_mean).max() < 5.0 and np.abs(zx_var).max() < 5.0, (np.abs(zx_mean).max(), np.abs(zx_var).max())


def _sw_model(lags):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, lags)


@pytest.mark.parametrize("lags", [1, 4])
def test_stock_watson_draw_paths(ctx, lags):
    from dynamic_factor_models_amd import api
    m = _sw_model(lags)
    api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=lags, ctx=ctx)
    params = {k: v.copy() for k, v in m.em_params.items()}
    H, n = 8, 256
    o = api.draw_paths(m, n, H, through=224, seed=5, ctx=ctx)
    assert all(np.array_equal(params[k], m.em_params[k]) for k in params), "draw_paths changed m.em_params"
    fc = api.forecast(m, H, through=224, ctx=ctx)
    assert np.array_equal(o["rows"], fc["rows"]) and np.array_equal(o["cols"], fc["cols"])
    r = params["Lam"].shape[1]
    assert o["factor"].shape == (n, fc["rows"].size, r) and o["x"].shape == (n, fc["rows"].size, fc["cols"].size)
    data = m.data[2:224][:, o["cols"]]
    obs = ~np.isnan(data)
    assert np.array_equal(o["x"][:, :224 - 2][:, obs], np.broadcast_to(data[obs], (n, int(obs.sum())))), \
        "observed cells are not the data bit for bit"
    assert np.all(np.isfinite(o["x"])) and np.all(np.isfinite(o["factor"]))
    fsd = np.sqrt(np.diagonal(fc["factor_cov"], axis1=1, axis2=2))
    assert np.abs((o["factor"].mean(0) - fc["factor"]) / (fsd / np.sqrt(n))).max() < 5.0
    drawn = fc["x_sd"] > 0.0
    zx = (o["x"].mean(0)[drawn] - fc["x"][drawn]) / (fc["x_sd"][drawn] / np.sqrt(n))
    assert np.abs(zx).max() < 5.0
    again = api.draw_paths(m, 4, H, through=224, seed=5, first_draw=100, ctx=ctx)
    whole = api.draw_paths(m, 104, H, through=224, seed=5, ctx=ctx)
    assert np.array_equal(again["factor"], whole["factor"][100:]) and np.array_equal(again["x"], whole["x"][100:])


def test_parameter_draws(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=8, seed=11)
    H, n = 4, 16
    o = api.draw_paths(m, n, H, through=224, seed=3, parameter_draws=True, ctx=ctx)
    rows, ncol = o["rows"].size, o["cols"].size
    assert o["factor"].shape == (8, n, rows, 4) and o["x"].shape == (8, n, rows, ncol)
    cols, z, mu, sd = api._forecast_inputs(m, 224)
    rp = m.replicates["params"]
    for b, d in ((0, 0), (7, 15), (3, 5)):
        f, xd = draw(z, *[rp[k][b] for k in KEYS], H, 1, 3, 0, d, b, mean=mu, sd=sd)
        _close(o["factor"][b, d], f, f"replicate {b} draw {d} factor")
        _close(o["x"][b, d], xd, f"replicate {b} draw {d} x")
    data = m.data[2:224][:, cols]
    obs = ~np.isnan(data)
    assert np.all(o["x"][:, :, :222][:, :, obs] == data[obs])


def test_status_codes(ctx):
    import ctypes
    from dynamic_factor_models_amd import _lib
    panel, st = _batch(1, 20, 30, 2, 0.0)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    f, x = np.empty((1, 3, 40, 2)), np.empty((1, 3, 40, 20))
    args = [ptr(panel)] + [ptr(np.ascontiguousarray(st[k])) for k in KEYS]
    call = lambda B, D, T, p, H, fo, mean=None, sd=None: ctx._lib.dfm_simsmooth_batch(
        ctx._h, B, D, T, 20, 2, p, H, *args, mean, sd, 1, 0, fo, ptr(x), 0)
    assert call(1, 0, 30, 1, 3, ptr(f)) == -1                 # D < 1: DFM_E_DIMS
    assert call(1, 3, 30, 1, -1, ptr(f)) == -1                # H < 0
    assert call(1, 3, 1, 2, 3, ptr(f)) == -1                  # T < p
    assert call(1, 3, 30, 1, 3, None) == -3                   # f_draw NULL: DFM_E_NULL
    assert call(1, 3, 30, 1, 3, ptr(f), mean=ptr(st["R"])) == -3      # mean without sd
    assert call(1, 3, 30, 1, 3, ptr(f), sd=ptr(st["R"])) == -3        # sd without mean
    assert call(1, 3, 30, 1, 3, ptr(f)) == 0
    # r p > 32: whatever dfm_ks_pass_varp_batch says for the same shape
    r, p = 9, 4
    xv, _ = _varp_batch(1, 20, 30, 3, 2, 0.0)
    big = dict(Lam=np.ones((1, 20, r)), R=np.ones((1, 20)), A=np.zeros((1, r, r * p)), Q=np.tile(np.eye(r), (1, 1, 1)),
               mu0=np.zeros((1, r * p)), P0=np.tile(np.eye(r * p), (1, 1, 1)))
    with pytest.raises(_lib.DfmError) as want:
        ctx.ks_pass_varp_batch_host(xv, *[big[k] for k in KEYS])
    with pytest.raises(_lib.DfmError) as got:
        _ss(ctx, xv, big, 2, 3)
    assert got.value.code == want.value.code
    bad = panel.copy(); bad[0, 5, 3] = np.nan                 # NaN without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING
    with pytest.raises(_lib.DfmError) as ei:
        _ss(ctx, bad, st, 2, 3, may_have_missing=False)
    assert ei.value.code == -4
    sing = {k: v.copy() for k, v in st.items()}               # rank-deficient Q in information form: DFM_E_NUMERIC
    sing["Q"][0] = np.outer(np.ones(2), np.ones(2)) * 0.5
    with pytest.raises(_lib.DfmError) as ei:
        _ss(ctx, panel, sing, 2, 3)
    assert ei.value.code == -5
    ok = _ss(ctx, panel, sing, 2, 3, singular_q=True)
    assert np.all(np.isfinite(ok["f"]))
