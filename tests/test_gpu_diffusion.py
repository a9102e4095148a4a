"""GPU tests of dfm_diffusion_eval_batch (include/dfm_hip.h; csrc/diffusion.hip) against the expectation model of
tests/diffusion_expect.py: the new kernels alone (max_iter = 0, random finite start factors) over their launch geometry and every
lane-group width, the ALS in the loop against the oracle's sweeps, a call of more than one slice, a window with a non-finite factor
row, the status codes, and api.forecast_diffusion_index on the Stock-Watson panel.

Tolerances.  Windows and statistics: 1e-13 x scale, as tests/test_gpu_rolling_eval.py (the same kernel).  Regressions (beta, fc,
fc_ar, fvar, err*) at the factors the call returned: 1e-9 x scale, the bar tests/test_gpu_als.py sets for dfm_ols_batch;
tests/test_diffusion_cpu.py shows that lstsq and float64 normal equations agree to 1e-10 on every regression of every case here.
Scores from the returned errors: 1e-12.  ALS: the 1e-8 of tests/test_gpu_als.py on F and Lam; end to end against the oracle's own
factors 10 x the sensitivity figure tests/test_diffusion_cpu.py measures (diffusion_expect.SENSITIVITY), in units of win_sd."""
import ctypes
import os

import numpy as np
import pytest

from tests import diffusion_expect as dx
from tests import rolling_expect as rx

pytestmark = pytest.mark.gpu
FTOL = 1e-9
ALL = ("fc", "fc_ar", "fvar", "err", "err_ar", "err_std", "msfe", "msfe_ar", "msfe0", "cnt", "F", "Lam", "iters", "ssr", "mean", "sd",
       "nobs", "beta", "nobs_reg", "win")


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


def _run(ctx, x, origins, W, H, F_start, q, **kw):
    return ctx.diffusion_eval_batch_host(x, origins, W, H, F_start, q=q, want=ALL, **kw)


def _check_scores(got, x, origins, what):
    s = dx.score(x, origins, got["fc"], got["fc_ar"], got["fvar"], got["mean"])
    for k in ("err", "err_ar", "err_std", "msfe", "msfe_ar", "msfe0"):
        _close(got[k], s[k], 1e-12, f"{what} {k}")
    assert np.array_equal(got["cnt"], s["cnt"]), what + " cnt"


def _check_regressions(got, e, H, what):
    """The regressions against the expectation e computed at the returned factors, horizons 0 .. H of it."""
    for k in ("fc", "fc_ar", "fvar", "beta"):
        _close(got[k], e[k][:, :H + 1], FTOL, f"{what} {k}")
    assert np.array_equal(got["nobs_reg"], e["nobs_reg"][:, :H + 1]), what + " nobs_reg"


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", dx.NS)
@pytest.mark.parametrize("r,q", dx.RQ)
def test_kernels_alone_geometry(ctx, r, q, N):
    nt_min = dx.kernel_nt_min(r, q)
    ran = 0
    for W in dx.windows_of(r, q):
        Hs = [H for H in dx.HS if not dx.refused(r, q, W, H)]      # (what DFM_E_DIMS refuses of the grid is skipped)
        for vi, variant in enumerate(dx.VARIANTS if Hs else ()):
            x, origins, lags, Fp, min_obs = dx.kernel_case(N, W, r, q, variant)
            per_window = vi % 2 == 1                               # n_start = 1 and n_start = O in turn
            F_start = dx.start_windows(Fp, origins, W) if per_window else Fp
            e = None
            for H in sorted(Hs, reverse=True):
                what = f"N={N} W={W} r={r} q={q} H={H} lags={variant}"
                got = _run(ctx, x, origins, W, H, F_start, q, lags=lags, min_obs=min_obs, nt_min=nt_min, max_iter=0)
                if e is None:                                      # (the regressions of a smaller H are among those of the largest)
                    e = dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, F=got["F"])
                _close(got["win"], e["win"], 1e-13, what + " windows")
                _close(got["mean"], e["mean"], 1e-13, what + " mean")
                _close(got["sd"], e["sd"], 1e-13, what + " sd")
                assert np.array_equal(got["nobs"], e["nobs"]), what + " nobs"
                assert np.array_equal(got["F"], dx.start_windows(Fp, origins, W)), what + " F"
                assert np.all(got["iters"] == 0) and np.all(np.isnan(got["ssr"])) and np.all(np.isnan(got["Lam"]))
                _check_regressions(got, e, H, what)
                _check_scores(got, x, origins, what)
                assert np.all(np.isnan(got["err"][-1, 1:]))        # the origin at T - 1: nothing to score
                lg = np.zeros(N, dtype=int) if lags is None else lags
                assert np.all(np.isnan(got["fc"][:, 0, lg == 0])) and np.all(got["cnt"][0, lg == 0] == 0)      # h + l = 0: visible
                if N >= 3:
                    assert np.all(got["cnt"][:, N - 1] == 0) and np.all(np.isnan(got["msfe"][:, N - 1]))        # unobserved on every target row
                    assert np.all(np.isnan(got["msfe_ar"][:, N - 1])) and np.all(np.isnan(got["msfe0"][:, N - 1]))
                ran += 1
    assert ran > 0


# ---- 2. the ALS in the loop ----------------------------------------------------------------------------------------------------
def _check_als(got, e, what):
    assert np.array_equal(got["iters"], e["iters"]), (what, got["iters"], e["iters"])
    for k in ("F", "Lam"):
        _close(got[k], e[k], dx.ALS_PARITY, f"{what} {k}")
    np.testing.assert_allclose(got["ssr"], e["ssr"], rtol=dx.ALS_PARITY, err_msg=what + " ssr")


def _check_end_to_end(got, e, what):
    """fc and fc_ar against the expectation at the ORACLE's factors, in units of win_sd."""
    for k in ("fc", "fc_ar"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(e[k])), f"{what} {k}: NaN pattern"
        err = np.nanmax(np.abs(got[k] - e[k]) / e["sd"][:, None, :])
        assert err <= 10 * dx.SENSITIVITY, f"{what} {k}: {err:.3e} of win_sd"
    assert np.array_equal(got["nobs_reg"], e["nobs_reg"]) and np.array_equal(got["cnt"], e["cnt"])


def test_als_fixed_sweeps(ctx):
    x, origins, W, H, q, lags, nt_min, Fp = dx.als_case()
    got = _run(ctx, x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=6, tol=0.0)
    e = dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=6, tol=0.0)
    assert np.all(e["iters"] == 6)
    _close(got["win"], e["win"], 1e-13, "windows")
    _check_als(got, e, "tol=0")
    _check_regressions(got, dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, F=got["F"]), H, "tol=0")
    _check_scores(got, x, origins, "tol=0")
    _check_end_to_end(got, e, "tol=0")


def test_als_stop_rule(ctx):
    """The API's tol: every window stops by the rule, at its own sweep (tests/test_diffusion_cpu.py holds every stop decision of the
    oracle at least 100 x the factor parity away from the threshold)."""
    x, origins, W, H, q, lags, nt_min, Fp = dx.als_case()
    got = _run(ctx, x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=2000, tol=dx.ALS_TOL)
    e = dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=2000, tol=dx.ALS_TOL)
    assert e["iters"].max() < 2000 and np.unique(e["iters"]).size > 1
    _check_als(got, e, "tol=1e-8")
    _check_regressions(got, dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, F=got["F"]), H, "tol=1e-8")
    _check_end_to_end(got, e, "tol=1e-8")


# ---- 3. more than one slice ------------------------------------------------------------------------------------------------------
def _slice_case():
    from oracle import kalman_oracle as ko
    T, N, W, r, q, H = 1100, 6, 16, 1, 1, 2
    z, _ = ko.synth_replicate(5, N, T, r)
    rng = np.random.default_rng(6)
    x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
    Fp = np.random.default_rng(8).standard_normal((T, r))
    return x, np.arange(W - 1, T), W, H, q, Fp


def test_more_than_one_slice(ctx):
    x, origins, W, H, q, Fp = _slice_case()
    assert origins.size == 1085
    got = _run(ctx, x, origins, W, H, Fp, q, nt_min=5, max_iter=2, tol=0.0)
    some = [0, 1023, 1024, 1084]
    e = dx.expect(x, origins, W, H, Fp, q, nt_min=5, max_iter=2, tol=0.0, only=some)
    for b in some:
        _close(got["F"][b], e["F"][b], dx.ALS_PARITY, f"F b={b}")
        at = dx.expect(x, origins, W, H, Fp, q, nt_min=5, F=got["F"], only=[b])
        for k in ("fc", "fc_ar", "fvar", "beta"):
            _close(got[k][b], at[k][b], FTOL, f"{k} b={b}")
    _check_scores(got, x, origins, "slices")
    assert got["cnt"][1].min() == 1084 and got["cnt"][2].min() == 1083 and np.all(got["cnt"][0] == 0)
    again = _run(ctx, x, origins, W, H, Fp, q, nt_min=5, max_iter=2, tol=0.0)
    for k in ("msfe", "msfe_ar", "msfe0"):
        assert np.array_equal(again[k], got[k], equal_nan=True), k        # bit for bit, run to run


# ---- 4. a window whose factors are not finite ---------------------------------------------------------------------------------------
def test_degenerate_window(ctx):
    x, origins, W, H, q, lags, nt_min, Fp = dx.als_case()
    F0 = dx.start_windows(Fp, origins, W)
    good = _run(ctx, x, origins, W, H, F0, q, lags=lags, nt_min=nt_min, max_iter=0)
    bad0 = F0.copy()
    bad0[4, 7, 1] = np.inf
    bad = _run(ctx, x, origins, W, H, bad0, q, lags=lags, nt_min=nt_min, max_iter=0)
    for k in ("fc", "fc_ar", "fvar", "err", "err_ar", "err_std", "beta"):
        assert np.all(np.isnan(bad[k][4])), k
        rest = np.arange(origins.size) != 4
        assert np.array_equal(bad[k][rest], good[k][rest], equal_nan=True), k          # the neighbours: bit for bit
    assert np.all(bad["nobs_reg"][4] == 0)
    _check_scores(bad, x, origins, "degenerate")                    # (the window is not scored: its fc is NaN)
    assert (bad["cnt"] <= good["cnt"]).all() and bad["cnt"].sum() < good["cnt"].sum()


# ---- 5. status codes --------------------------------------------------------------------------------------------------------------
def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    from oracle import kalman_oracle as ko
    T, N, r, q, W, H = 40, 6, 2, 1, 16, 2
    z, _ = ko.synth_replicate(8, N, T, r)
    rng = np.random.default_rng(9)
    x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
    Fp = rng.standard_normal((T, r))
    origins = np.array([15, 21, 39], dtype=np.int32)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def raw(T=T, N=N, r=r, q=q, W=W, H=H, origins=origins, min_obs=r + 1, n_start=1, lags=None, flags=1, max_iter=0, x=x, F_start=Fp):
        lg = None if lags is None else np.ascontiguousarray(lags, dtype=np.int32)
        fc = np.empty((origins.size, H + 1 if H >= 0 else 1, N))
        return ctx._lib.dfm_diffusion_eval_batch(
            ctx._h, T, N, r, q, W, H, origins.size, min_obs, 5, n_start, ptr(x), ptr(origins), ptr(lg), ptr(F_start), max_iter, 0.0,
            *([None] * 8), ptr(fc), *([None] * 11), flags)

    def good():
        o = _run(ctx, x, origins, W, H, Fp, q, nt_min=5, max_iter=2, tol=0.0)
        assert np.all(np.isfinite(o["fc"][:, 1:])) and np.all(o["iters"] == 2)

    good()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    dims = [dict(r=8, q=24, W=40, min_obs=9, origins=i32(39)),      # K = 33 > 32
            dict(r=0), dict(q=-1), dict(H=-1), dict(W=T + 1), dict(W=1 + r + q + q + H + 1, origins=i32(20, 39)),
            dict(min_obs=r), dict(n_start=2), dict(origins=i32(14, 21)), dict(origins=i32(21, T)), dict(origins=i32(21, 21, 39)),
            dict(origins=i32(21, 15, 39)), dict(lags=[0, 0, -1, 0, 0, 0]), dict(lags=[0, 0, W - r, 0, 0, 0]),
            dict(lags=[1, 1, 2, 1, 1, 3]),                          # no series reaches the origin
            dict(max_iter=-1)]
    for kw in dims:
        assert raw(**kw) == -1, kw                                 # DFM_E_DIMS
        good()
    assert raw(x=None) == -3 and raw(F_start=None) == -3           # DFM_E_NULL
    good()
    assert raw(lags=[0, 1, 0, 0, 0, 0], flags=0) == -4             # DFM_E_MISSING: a lag without DFM_F_MAY_HAVE_MISSING
    good()
    hole = x.copy(); hole[20, 3] = np.nan
    with pytest.raises(_lib.DfmError) as ei:                        # a NaN of x inside a window without the flag
        _run(ctx, hole, origins, W, H, Fp, q, nt_min=5, max_iter=0, may_have_missing=False)
    assert ei.value.code == -4
    good()
    thin = x.copy(); thin[7:21, 4] = np.nan                        # window 1 (rows 6 .. 21): 2 visible cells < min_obs = 3
    assert rx.window_fails(rx.windows(thin, origins, W), r + 1)
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, thin, origins, W, H, Fp, q, nt_min=5, max_iter=2)
    assert ei.value.code == -9                                      # DFM_E_WINDOW
    good()
    # the ALS's LDS bound: (W + N) pad(r) doubles
    big = np.zeros((2600, 16))
    assert raw(T=2600, N=16, r=8, q=0, W=2600, H=0, min_obs=9, origins=i32(2599), x=big, F_start=np.zeros((2600, 8))) == -1
    good()
    # the device-pointer entry: the same numbers, DFM_E_WINDOW raised by the call itself
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with pytest.raises(_lib.DfmError) as ei:
        ctx.diffusion_eval_batch(t(thin), origins, W, H, t(Fp), q=q, nt_min=5, max_iter=2)
    assert ei.value.code == -9
    o = ctx.diffusion_eval_batch(t(x), origins, W, H, t(Fp), q=q, nt_min=5, max_iter=2, tol=0.0)
    ctx.synchronize()
    h = _run(ctx, x, origins, W, H, Fp, q, nt_min=5, max_iter=2, tol=0.0)
    _close(o["fc"].cpu().numpy(), h["fc"], 1e-12, "_dev vs host fc")
    assert np.array_equal(o["cnt"].cpu().numpy(), h["cnt"]) and o["beta"] is None


# ---- 6. the API on the Stock-Watson panel ---------------------------------------------------------------------------------------
def test_api_stock_watson(ctx):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 1)
    with pytest.raises(ValueError, match="estimate_factor"):
        api.forecast_diffusion_index(m, 4, window=120, ctx=ctx)
    api.estimate_factor(m, max_iter=200, ctx=ctx)
    factor = m.factor.copy()
    H, W = 4, 120
    o = api.forecast_diffusion_index(m, H, window=W, step=8, max_iter=30, ctx=ctx)
    assert np.array_equal(factor, m.factor, equal_nan=True), "the call changed m.factor"
    org = np.arange(122, 217, 8)
    O, n, r = org.size, o["cols"].size, 4
    assert np.array_equal(o["origins"], org) and np.array_equal(o["horizons"], np.arange(H + 1)) and n > 100
    for k in ("forecast", "forecast_ar", "variance", "error", "error_ar", "error_std"):
        assert o[k].shape == (O, H + 1, n), k
    for k in ("msfe", "msfe_ar", "msfe_mean", "relative_ar", "relative_mean", "count"):
        assert o[k].shape == (H + 1, n), k
    assert o["factor"].shape == (O, W, r) and o["loadings"].shape == (O, n, r) and o["iters"].shape == (O,) and o["ssr"].shape == (O,)
    assert o["mean"].shape == (O, n) and o["sd"].shape == (O, n)
    assert np.all(np.isfinite(o["factor"])) and np.all(np.isfinite(o["ssr"])) and np.all((o["iters"] >= 1) & (o["iters"] <= 30))
    x = m.data[2:216][:, o["cols"]]
    s = dx.score(x, org - 3, o["forecast"], o["forecast_ar"], o["variance"], o["mean"])
    assert np.array_equal(o["count"], s["cnt"]) and np.all(o["count"][0] == 0) and o["count"][1:].max() == O
    have = o["count"] > 0
    assert np.all(np.isfinite(o["relative_ar"][have])) and np.all(np.isnan(o["relative_ar"][~have]))
    last = api.forecast_diffusion_index(m, H, window=W, origins=[216], max_iter=30, ctx=ctx)      # an origin at lastperiod: real forecasts
    assert np.isfinite(last["forecast"][0, 1:]).mean() > 0.9 and np.all(last["count"] == 0) and np.all(np.isnan(last["msfe"]))
    # two windows against the expectation model at the returned factors
    for b in (0, O - 1):
        at = dx.expect(x, org - 3, W, H, factor[2:216], 4, nt_min=20, F=o["factor"], only=[b])
        _close(o["forecast"][b], at["fc"][b], FTOL, f"forecast b={b}")
        _close(o["forecast_ar"][b], at["fc_ar"][b], FTOL, f"forecast_ar b={b}")
        _close(o["variance"][b], at["fvar"][b], FTOL, f"variance b={b}")
