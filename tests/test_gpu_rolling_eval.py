"""GPU tests of dfm_rolling_eval_batch (include/dfm_hip.h; csrc/rolling.hip) against the expectation model of
tests/rolling_expect.py: the three new kernels alone (max_iter = 0) over their launch geometry, the EM on the windows against the
oracle per window (plain, VAR(p), the balanced fast path, the per-window stop), a call of more than one slice, the status codes,
and api.evaluate_forecasts_rolling on the Stock-Watson panel.

Tolerances.  Windows, statistics, the rescaled start and the scores are fp64 sums of at most a few dozen terms of one sign pattern or
another: 1e-13 x scale (33 terms x 2^-53 is 4e-15).  Forecasts: the 1e-9 of tests/test_gpu_forecast.py, at the parameters and windows
the call returned.  EM: RTOL = 1e-8 of tests/test_gpu_em.py (the VAR(p) cases: the 1e-8 of tests/test_gpu_varp.py)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import rolling_expect as rx

pytestmark = pytest.mark.gpu
RTOL = 1e-8
FTOL = 1e-9
KEYS = rx.KEYS
ALL = ("fc", "fvar", "err", "err_std", "msfe", "msfe0", "cnt", "mean", "sd", "nobs", "win")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, tol, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern"
    if np.isnan(b).all():
        return
    scale = max(1.0, float(np.nanmax(np.abs(b))))
    err = float(np.nanmax(np.abs(a - b)))
    assert err <= tol * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _run(ctx, x, origins, W, H, start, **kw):
    return ctx.rolling_eval_batch_host(x, origins, W, H, *[start[k] for k in KEYS], want=ALL, **kw)


def _data_units(z, seed):
    rng = np.random.default_rng(seed)
    N = z.shape[1]
    return z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)


def _lead(q, akey="A"):
    return dict(Lam=q["Lam"][None], R=q["R"][None], Avar=q[akey][None], Q=q["Q"][None], mu0=q["mu0"][None], P0=q["P0"][None])


def _check_forecasts_and_scores(got, x, origins, lags, H, p, what):
    """fc / fvar at the RETURNED parameters and windows; the scores recomputed from the returned fc / fvar."""
    fc, fv = rx.forecasts(got["win"], got["params"], got["mean"], got["sd"], H, p)
    _close(got["fc"], fc, FTOL, what + " fc")
    _close(got["fvar"], fv, FTOL, what + " fvar")
    _check_scores(got, x, origins, lags, what)


def _check_scores(got, x, origins, lags, what):
    s = rx.score(x, origins, lags, got["fc"], got["fvar"], got["mean"])
    for k in ("err", "err_std", "msfe", "msfe0"):
        _close(got[k], s[k], 1e-13, f"{what} {k}")
    assert np.array_equal(got["cnt"], s["cnt"]), what + " cnt"


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------
def _geometry_case(N, W, variant):
    """A raw panel of T = W + 12 rows with 10 % missing cells, origins at the first full window, an uneven step and T - 1; one
    series at the largest lag (N >= 3: series 1) and one unobserved on every target row (N >= 3: the last)."""
    T, r = W + 12, min(2, N)
    min_obs = r + 1
    z, tr = ko.synth_replicate(11, N, T, r)
    x = _data_units(z, [N, W])
    origins = np.array([W - 1, W + 1, W + 4, T - 1])
    j_lag, j_dead = (1, N - 1) if N >= 3 else (0, None)
    lags = {"none": None, "mod3": np.arange(N) % 3, "max": np.zeros(N, dtype=int)}[variant]
    if variant == "max":
        lags[j_lag] = W - min_obs
    if lags is not None and j_dead is not None:
        lags[j_dead] = 0
    miss = np.random.default_rng([N, W, 1]).random((T, N)) < 0.1
    miss[:, j_lag] = False
    if j_dead is not None:
        miss[:, j_dead] = False
        miss[W:W + 9, j_dead] = True                          # every target row o + h, h = 1 .. 4, of the origins before T - 1
    xm = np.where(miss, np.nan, x)
    thin = ((~np.isnan(rx.windows(xm, origins, W, lags))).sum(axis=1) < min_obs).any(axis=0)
    if j_dead is not None:
        assert not thin[j_dead]
    xm[:, thin] = x[:, thin]                                  # (a series the draw left too thin for a window keeps all its cells)
    assert not rx.window_fails(rx.windows(xm, origins, W, lags), min_obs)
    sd_full = np.nanstd(xm, axis=0)
    return xm, origins, lags, _lead(tr), sd_full, j_dead


@pytest.mark.parametrize("H", [0, 1, 4])
@pytest.mark.parametrize("W", [8, 33])
@pytest.mark.parametrize("N", [1, 7, 64, 65, 130])
def test_kernels_alone_geometry(ctx, N, W, H):
    for variant in ("none", "mod3", "max"):
        x, origins, lags, start, sd_full, j_dead = _geometry_case(N, W, variant)
        what = f"N={N} W={W} H={H} lags={variant}"
        got = _run(ctx, x, origins, W, H, start, lags=lags, sd_start=sd_full, max_iter=0)
        raw = rx.windows(x, origins, W, lags)
        mu, sd, n, z = rx.standardise(raw)
        _close(got["win"], z, 1e-13, what + " windows")
        _close(got["mean"], mu, 1e-13, what + " mean")
        _close(got["sd"], sd, 1e-13, what + " sd")
        assert np.array_equal(got["nobs"], n), what + " nobs"
        st = rx.rescale_start(start, sd, sd_full)
        for k in KEYS:
            _close(got["params"][k], st[k], 1e-13, f"{what} start {k}")
        assert np.all(got["iters"] == 0) and got["loglik_path"] is None
        _check_forecasts_and_scores(got, x, origins, lags, H, 1, what)
        assert np.all(np.isfinite(got["fc"])) and np.all(np.isfinite(got["fvar"]))
        assert np.all(np.isnan(got["err"][-1, 1:]))            # the origin at T - 1: forecasts, nothing to score
        if lags is None:
            assert np.all(got["cnt"][0] == 0)                  # no nowcast without a publication lag
        if j_dead is not None:
            assert np.all(got["cnt"][:, j_dead] == 0) and np.all(np.isnan(got["msfe"][:, j_dead]))
            assert np.all(np.isnan(got["msfe0"][:, j_dead]))
        if H >= 1:
            assert got["cnt"][1:].max() == origins.size - 1


# ---- 2. EM parity, the per-window stop -----------------------------------------------------------------------------------------
def _check_em(got, e, tol_p, tol_path, what, windows=None):
    for b in (range(len(e["iters"])) if windows is None else windows):
        k = int(e["iters"][b])
        assert got["iters"][b] == k, (what, b, got["iters"][b], k)
        np.testing.assert_allclose(got["loglik_path"][b, :k], e["paths"][b], rtol=tol_path, err_msg=f"{what} path b={b}")
        assert np.all(np.isnan(got["loglik_path"][b, k:]))
        for key in KEYS:
            want = e["params"][key][b]
            err = np.abs(got["params"][key][b] - want).max()
            assert err <= tol_p * max(1.0, np.abs(want).max()), (what, key, b, err)


def test_em_parity_and_per_window_stop(ctx):
    x, origins, W, H, lags, start = rx.em_parity_case()
    got = _run(ctx, x, origins, W, H, start, lags=lags, max_iter=6, tol=0.0)
    e = rx.expect(x, origins, W, H, start, lags=lags, max_iter=6, tol=0.0)
    _close(got["win"], e["win"], 1e-13, "windows")
    _check_em(got, e, RTOL, RTOL, "tol=0")
    _check_forecasts_and_scores(got, x, origins, lags, H, 1, "tol=0")
    got = _run(ctx, x, origins, W, H, start, lags=lags, max_iter=30, tol=1e-4)
    e = rx.expect(x, origins, W, H, start, lags=lags, max_iter=30, tol=1e-4)
    assert e["iters"].max() < 30 and np.unique(e["iters"]).size > 1
    _check_em(got, e, RTOL, RTOL, "tol=1e-4")
    _check_forecasts_and_scores(got, x, origins, lags, H, 1, "tol=1e-4")


# ---- 3. VAR(p) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,p,missing", [(3, 2, 0.1), (4, 2, 0.0)])
def test_varp_windows(ctx, r, p, missing):
    N, T, W, H = 20, 90, 60, 2
    x = _data_units(vo.synth_varp(0, N, T, r, p, missing=missing), [r, p])
    origins = np.array([59, 65, 72, 80, 89])
    lags = np.arange(N) % 3 if missing else None
    _, _, _, z0 = rx.standardise(rx.windows(x, origins[:1], W, lags))
    q, _ = vo.varp_init(np.nan_to_num(z0[0]), r, p)
    start = _lead(q, "Avar")
    got = _run(ctx, x, origins, W, H, start, lags=lags, max_iter=4, tol=0.0)
    e = rx.expect(x, origins, W, H, start, lags=lags, p=p, max_iter=4, tol=0.0)
    _check_em(got, e, 1e-8, 1e-8, f"r={r} p={p}")
    _check_forecasts_and_scores(got, x, origins, lags, H, p, f"r={r} p={p}")


# ---- 4. balanced windows: the fast path ------------------------------------------------------------------------------------------
def test_balanced_windows_fast_path(ctx):
    N, T, W, H, r = 40, 120, 80, 3, 3
    z, _ = ko.synth_replicate(2, N, T, r)
    x = _data_units(z, 4)
    origins = np.array([79, 90, 101, 119])
    _, _, _, z0 = rx.standardise(rx.windows(x, origins[:1], W))
    q, _ = ko.pca_init(z0[0], r)
    start = _lead(q)
    got = _run(ctx, x, origins, W, H, start, max_iter=3, tol=0.0, may_have_missing=False)
    e = rx.expect(x, origins, W, H, start, max_iter=3, tol=0.0)
    _check_em(got, e, RTOL, RTOL, "balanced")
    _check_forecasts_and_scores(got, x, origins, None, H, 1, "balanced")


# ---- 5. more than one slice -------------------------------------------------------------------------------------------------------
def test_more_than_one_slice(ctx):
    T, N, W, r, H = 1100, 6, 16, 1, 2
    z, _ = ko.synth_replicate(5, N, T, r)
    x = _data_units(z, 6)
    origins = np.arange(W - 1, T)
    assert origins.size == 1085
    _, _, _, z0 = rx.standardise(rx.windows(x, origins[:1], W))
    q, _ = ko.pca_init(z0[0], r)
    start = _lead(q)
    got = _run(ctx, x, origins, W, H, start, max_iter=2, tol=0.0)
    e = rx.expect(x, origins, W, H, start, max_iter=2, tol=0.0, only=[0, 1023, 1024])
    _check_em(got, e, RTOL, RTOL, "slices", windows=[0, 1023, 1024])
    for b in (0, 1023, 1024):
        _close(got["fc"][b], e["fc"][b], FTOL, f"fc b={b}")
        _close(got["fvar"][b], e["fvar"][b], FTOL, f"fvar b={b}")
    _check_scores(got, x, origins, None, "slices")
    assert got["cnt"][1].min() == 1084 and got["cnt"][2].min() == 1083
    again = _run(ctx, x, origins, W, H, start, max_iter=2, tol=0.0)
    assert np.array_equal(again["msfe"], got["msfe"], equal_nan=True) and np.array_equal(again["msfe0"], got["msfe0"], equal_nan=True)
    assert np.all(np.isnan(got["msfe"][0])) and np.all(np.isfinite(got["msfe"][1:]))


# ---- 6. status codes --------------------------------------------------------------------------------------------------------------
def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    T, N, r, W, H = 30, 6, 2, 12, 2
    z, tr = ko.synth_replicate(8, N, T, r)
    x = _data_units(z, 9)
    start = _lead(tr)
    origins = np.array([11, 15, 29], dtype=np.int32)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def raw(T=T, N=N, r=r, p=1, W=W, H=H, origins=origins, min_obs=r + 1, n_start=1, lags=None, flags=1, max_iter=0):
        O = origins.size
        k = r * p
        out = [np.empty((O, N, r)), np.empty((O, N)), np.empty((O, r, k)), np.empty((O, r, r)), np.empty((O, k)), np.empty((O, k, k))]
        lg = None if lags is None else np.ascontiguousarray(lags, dtype=np.int32)
        return ctx._lib.dfm_rolling_eval_batch(
            ctx._h, T, N, r, p, W, H, O, min_obs, n_start, ptr(x), ptr(origins), ptr(lg), *[ptr(start[k_]) for k_ in KEYS], None,
            max_iter, 0.0, *map(ptr, out), None, None, None, None, None, None, None, None, None, None, None, None, None, flags)

    def good():
        o = _run(ctx, x, origins, W, H, start, max_iter=2)
        assert np.all(np.isfinite(o["fc"])) and np.all(o["iters"] == 2)

    i32 = lambda *v: np.array(v, dtype=np.int32)
    dims = [dict(W=T + 1), dict(W=1), dict(W=2, p=3, min_obs=3, origins=i32(5)), dict(H=-1), dict(origins=i32(10, 15)),
            dict(origins=i32(11, T)), dict(origins=i32(15, 15, 29)), dict(origins=i32(15, 11, 29)), dict(lags=[0, 0, -1, 0, 0, 0]),
            dict(lags=[0, 0, W - r, 0, 0, 0]), dict(min_obs=r), dict(n_start=2), dict(p=17, W=20, origins=i32(19, 29)),
            dict(max_iter=-1)]
    for kw in dims:
        assert raw(**kw) == -1, kw                             # DFM_E_DIMS
        good()
    assert raw(lags=[0, 1, 0, 0, 0, 0], flags=0) == -4         # DFM_E_MISSING: a lag without DFM_F_MAY_HAVE_MISSING
    good()
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, x, origins, W, H, start, lags=[0, 1, 0, 0, 0, 0], max_iter=0, may_have_missing=False)
    assert ei.value.code == -4
    bad = x.copy(); bad[20, 3] = np.nan
    with pytest.raises(_lib.DfmError) as ei:                    # a NaN in x without the flag: the pass's own DFM_E_MISSING
        _run(ctx, bad, origins, W, H, start, max_iter=0, may_have_missing=False)
    assert ei.value.code == -4
    good()
    thin = x.copy(); thin[6:16, 4] = np.nan                    # window 1 (rows 4 .. 15): 2 visible cells < min_obs = 3
    assert rx.window_fails(rx.windows(thin, origins, W), r + 1)
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, thin, origins, W, H, start, max_iter=2)
    assert ei.value.code == -9                                  # DFM_E_WINDOW
    good()
    const = x.copy(); const[18:30, 2] = 0.1                    # constant inside window 2 (rows 18 .. 29) only
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, const, origins, W, H, start, max_iter=2)
    assert ei.value.code == -9
    good()
    # the device-pointer entry raises it too, and leaves the handle usable
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with pytest.raises(_lib.DfmError) as ei:
        ctx.rolling_eval_batch(t(thin), origins, W, H, *[t(start[k]) for k in KEYS], max_iter=2)
    assert ei.value.code == -9
    o = ctx.rolling_eval_batch(t(x), origins, W, H, *[t(start[k]) for k in KEYS], max_iter=2)
    ctx.synchronize()
    h = _run(ctx, x, origins, W, H, start, max_iter=2)
    _close(o["fc"].cpu().numpy(), h["fc"], 1e-12, "_dev vs host fc")      # (the same kernels; the store width may differ with alignment)
    assert np.array_equal(o["cnt"].cpu().numpy(), h["cnt"])


# ---- 7. the API on the Stock-Watson panel ---------------------------------------------------------------------------------------
def test_api_stock_watson(ctx):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx)
    fit = {k: v.copy() for k, v in m.em_params.items()}
    H, W = 4, 120
    o = api.evaluate_forecasts_rolling(m, H, window=W, step=8, max_em_iter=5, ctx=ctx)
    assert all(np.array_equal(fit[k], m.em_params[k]) for k in fit), "the evaluation changed m.em_params"
    org = np.arange(122, 217, 8)
    O, n = org.size, o["cols"].size
    assert np.array_equal(o["origins"], org) and np.array_equal(o["horizons"], np.arange(H + 1))
    for k in ("forecast", "variance", "error", "error_std"):
        assert o[k].shape == (O, H + 1, n), k
    for k in ("msfe", "rmsfe", "relative", "count"):
        assert o[k].shape == (H + 1, n), k
    assert o["mean"].shape == (O, n) and o["iters"].shape == (O,) and o["loglik_path"].shape == (O, 5)
    x = m.data[2:216][:, o["cols"]]
    o0 = org - 3
    s = rx.score(x, o0, None, o["forecast"], o["variance"], o["mean"])
    assert np.array_equal(o["count"], s["cnt"]) and np.all(o["count"][0] == 0) and o["count"][1:].max() == O      # (the last origin, 210, has its targets inside the sample)
    have = o["count"] > 0
    assert np.all(np.isfinite(o["relative"][have])) and np.all(np.isnan(o["relative"][~have]))
    # three origins against the expectation model: the start is the full-sample fit in the full sample's units
    cols0, _, _, sd_full = api._forecast_inputs(m, m.lastperiod)
    keep = np.isin(cols0, o["cols"])
    start = dict(Lam=fit["Lam"][keep][None], R=fit["R"][keep][None], Avar=fit["A"][None], Q=fit["Q"][None], mu0=fit["mu0"][None],
                 P0=fit["P0"][None])
    some = [0, 5, O - 1]
    e = rx.expect(x, o0, W, H, start, sd_start=sd_full[keep], max_iter=5, tol=1e-6, only=some)
    got = dict(iters=o["iters"], loglik_path=o["loglik_path"], params=o["params"])
    _check_em(got, e, RTOL, RTOL, "Stock-Watson", windows=some)
    for b in some:
        _close(o["forecast"][b], e["fc"][b], FTOL, f"forecast b={b}")
        _close(o["variance"][b], e["fvar"][b], FTOL, f"variance b={b}")
    # one start per origin, no EM: the same forecasts (the same kernels on the same windows and parameters; only the order of
    # a sum could differ, so 1e-12)
    again = api.evaluate_forecasts_rolling(m, H, window=W, step=8, start=dict(o["params"], cols=o["cols"]), max_em_iter=0,
                                           ctx=ctx)
    assert np.all(again["iters"] == 0)
    _close(again["forecast"], o["forecast"], 1e-12, "n_start = O forecast")
    _close(again["variance"], o["variance"], 1e-12, "n_start = O variance")
    assert np.array_equal(again["count"], o["count"])
