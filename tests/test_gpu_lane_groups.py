"""GPU parity of the lane-group kernels of the non-parametric estimator -- ols_kernel, als_kernel, standardize_kernel (als.hip),
var_boot_kernel, quantile_kernel (boot.hip), chow_kernel (breaks.hip) -- at every group width their launch_* switches can
pick: regressor counts that fill the width (no identity-padded row), three workgroups with a partial last one, and the edges
of each kernel's loops.  The cases, their inputs and their CPU references live in tests/lane_group_cases.py;
tests/test_lane_group_cases_cpu.py proves that the cases cover the widths and are conditioned far inside the tolerances used
here, which are those of tests/test_gpu_als.py, test_gpu_boot.py and test_gpu_breaks.py.  Every test prints its worst error."""
import numpy as np
import pytest

from oracle import als_oracle as ao
from oracle import boot_oracle as bo
from tests import lane_group_cases as lg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _report(what, **errs):
    print(f"\n[lane groups] {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


# ------------------------------------------------------------------------------------------------ OLS
def _check_ols(got, ref, K, T, nt_min, what):
    np.testing.assert_array_equal(got["nobs"], ref["nobs"])
    solved = ref["nobs"] >= max(K, nt_min)
    assert not solved[lg.OLS_SHORT] and solved.sum() >= len(solved) - 3
    e_beta = e_res = e_ssr = e_tss = 0.0
    for p in range(len(solved)):
        if not solved[p]:
            assert np.isnan(got["beta"][p]).all() and np.isnan(got["ssr"][p]) and np.isnan(got["tss"][p]), p
            assert np.isnan(got["resid"][:, p]).all(), p
            continue
        b, ok = ref["beta"][p], ~np.isnan(ref["resid"][:, p])
        e_beta = max(e_beta, np.abs(got["beta"][p] - b).max() / np.abs(b).max())
        e_res = max(e_res, np.abs(got["resid"][ok, p] - ref["resid"][ok, p]).max())
        e_ssr = max(e_ssr, abs(got["ssr"][p] / ref["ssr"][p] - 1.0))
        e_tss = max(e_tss, abs(got["tss"][p] / ref["tss"][p] - 1.0))
    _report(what, beta_rel=e_beta, resid_abs=e_res, ssr_rel=e_ssr, tss_rel=e_tss)
    for p in np.flatnonzero(solved):
        b, ok = ref["beta"][p], ~np.isnan(ref["resid"][:, p])
        np.testing.assert_allclose(got["beta"][p], b, rtol=0, atol=1e-9 * np.abs(b).max())
        np.testing.assert_allclose(got["resid"][ok, p], ref["resid"][ok, p], rtol=0, atol=1e-9)
        assert np.isnan(got["resid"][~ok, p]).all()
        np.testing.assert_allclose(got["ssr"][p], ref["ssr"][p], rtol=1e-9)
        np.testing.assert_allclose(got["tss"][p], ref["tss"][p], rtol=1e-9)


@pytest.mark.parametrize("shared", [True, False], ids=["sharedX", "ownX"])
@pytest.mark.parametrize("K,T", [c[:2] for c in lg.OLS_CASES])
def test_ols_at_every_width(ctx, K, T, shared):
    X, Y = lg.ols_data(K, T, shared)
    got = ctx.ols_batch_host(X, Y, nt_min=0)
    _check_ols(got, lg.ols_reference(K, T, shared), K, T, 0, f"ols K={K} R={lg.ols_width(K)} T={T} P={Y.shape[1]} shared={shared}")


def test_ols_nt_min_between_two_row_counts(ctx):
    K, T = lg.OLS_NT_MIN_CASE
    X, Y = lg.ols_data(K, T, True)
    ref = lg.ols_reference(K, T, True, lg.OLS_NT_MIN)
    assert K <= ref["nobs"][5] < lg.OLS_NT_MIN <= ref["nobs"][6]
    got = ctx.ols_batch_host(X, Y, nt_min=lg.OLS_NT_MIN)
    assert np.isnan(got["beta"][5]).all() and not np.isnan(got["beta"][6]).any()
    _check_ols(got, ref, K, T, lg.OLS_NT_MIN, f"ols K={K} nt_min={lg.OLS_NT_MIN}")


# ------------------------------------------------------------------------------------------------ bootstrap
@pytest.mark.parametrize("ns,p,T,H", [c[:4] for c in lg.BOOT_CASES])
def test_bootstrap_draws_at_every_width(ctx, ns, p, T, H):
    y, signs, ref = lg.var_data(ns, p, T), lg.boot_signs(ns, p, T), lg.boot_reference(ns, p, T, H)
    B = signs.shape[0]
    irf, beta = ctx.var_bootstrap_irf_host(y, ref["betahat"], ref["resid"], p, H, B, signs=signs, want_beta=True)
    _report(f"boot ns={ns} p={p} K={1 + ns * p} R={lg.boot_width(ns, p)} T={T} B={B}",
            beta_rel=np.abs(beta - ref["beta"]).max() / np.abs(ref["beta"]).max(),
            irf_rel=np.abs(irf - ref["irf"]).max() / np.abs(ref["irf"]).max(),
            point_rel=np.abs(irf[0] - ref["point"]).max() / np.abs(ref["point"]).max())
    np.testing.assert_allclose(beta, ref["beta"], rtol=0, atol=1e-9 * np.abs(ref["beta"]).max())
    np.testing.assert_allclose(irf, ref["irf"], rtol=0, atol=1e-9 * np.abs(ref["irf"]).max())
    np.testing.assert_allclose(irf[0], ref["point"], rtol=0, atol=1e-9 * np.abs(ref["point"]).max())   # all signs +1


@pytest.mark.parametrize("first_draw", lg.BOOT_FIRST_DRAWS)
@pytest.mark.parametrize("ns,p,T,H", lg.BOOT_SIGN_CASES)
def test_device_signs_are_the_restated_philox_stream(ctx, ns, p, T, H, first_draw):
    """Only the source of the signs differs between the two calls: drawn on the device, or handed in from
    boot_oracle.rademacher_signs.  The draws must be bit-equal."""
    y, ref = lg.var_data(ns, p, T), lg.boot_reference(ns, p, T, H)
    B = lg.three_workgroups(lg.boot_width(ns, p))
    signs = bo.rademacher_signs(lg.BOOT_SEED, first_draw, B, T)
    assert 0.3 < (signs > 0).mean() < 0.7 and (signs[:, p:].std(axis=0) > 0).all()
    drawn, beta_d = ctx.var_bootstrap_irf_host(y, ref["betahat"], ref["resid"], p, H, B, seed=lg.BOOT_SEED,
                                               first_draw=first_draw, want_beta=True)
    given, beta_g = ctx.var_bootstrap_irf_host(y, ref["betahat"], ref["resid"], p, H, B, signs=signs, want_beta=True)
    np.testing.assert_array_equal(beta_d, beta_g)
    np.testing.assert_array_equal(drawn, given)
    assert np.isfinite(drawn).all()


# ------------------------------------------------------------------------------------------------ quantiles
@pytest.mark.parametrize("B,S", lg.QUANTILE_CASES)
def test_quantiles_are_exact_order_statistics(ctx, B, S):
    x, ref = lg.quantile_data(B, S), lg.quantile_reference(B, S)
    q = np.array(lg.QUANTILE_Q)
    got = ctx.quantile_bands_host(x, q)
    np.testing.assert_array_equal(got, ref)                           # NaN draws count as +inf; an all-NaN column gives +inf
    cols = lg.quantile_finite_columns(S)
    np.testing.assert_array_equal(got[:, cols], np.quantile(x[:, cols], q, axis=0, method="inverted_cdf"))


# ------------------------------------------------------------------------------------------------ Chow
@pytest.mark.parametrize("k", lg.CHOW_K)
def test_chow_at_every_width(ctx, k):
    ys, Xs, series, breaks, qs = lg.chow_data(k)
    want = lg.chow_reference(k)
    got = ctx.chow_batch_host(list(ys), list(Xs), series, breaks, qs)
    _report(f"chow k={k} R={lg.chow_width(k)} P={len(want)}", rel=np.abs(got / want - 1.0).max())
    np.testing.assert_allclose(got, want, rtol=1e-8)


# ------------------------------------------------------------------------------------------------ standardize
@pytest.mark.parametrize("N", lg.STD_N)
def test_standardize_series_loop(ctx, N):
    import torch
    from dynamic_factor_models_amd import api
    x = lg.standardize_data(N)
    t = torch.from_numpy(x.copy()).cuda()
    mu, sd = ctx.standardize_batch(t)
    torch.cuda.synchronize()
    z_g, mu_g, sd_g = t.cpu().numpy(), mu.cpu().numpy(), sd.cpu().numpy()
    for b in range(lg.STD_B):
        z, s = api.standardize_data(x[b])
        n = (~np.isnan(x[b])).sum(axis=0)
        with np.errstate(invalid="ignore"):
            mean = np.nansum(x[b], axis=0) / n                       # NaN for the series without observations
        np.testing.assert_allclose(z_g[b], z, rtol=1e-12, atol=1e-13, equal_nan=True)
        np.testing.assert_allclose(sd_g[b], s[0], rtol=1e-13, equal_nan=True)
        np.testing.assert_allclose(mu_g[b], mean, rtol=1e-13, equal_nan=True)
        assert np.array_equal(np.isnan(z_g[b]), np.isnan(z)) and np.array_equal(np.isnan(sd_g[b]), n == 0)
    assert np.isnan(z_g[1, :, N // 2]).all() and np.isnan(mu_g[1, N // 2]) and np.isnan(sd_g[1, N // 2])
    assert not np.isnan(sd_g[0]).any() and not np.isnan(sd_g[2]).any()


# ------------------------------------------------------------------------------------------------ ALS
@pytest.mark.parametrize("r,T,N,miss,nt_min", [c[:5] for c in lg.ALS_CASES])
def test_als_at_every_width(ctx, r, T, N, miss, nt_min):
    refs = lg.als_reference(r, T, N, miss, nt_min)
    cap = lg.ALS_MAX_ITER
    got = ctx.als_batch_host(np.stack([o["z"] for o in refs]), np.stack([o["F0"] for o in refs]), nt_min=nt_min,
                             max_iter=cap, path_cap=cap, want_R2=True)
    errs = dict(ssr_path=0.0, F=0.0, Lam=0.0, R2=0.0)
    for b, o in enumerate(refs):
        k, m = o["iters"], ~np.isnan(o["lam"])
        if got["iters"][b] == k:
            errs["ssr_path"] = max(errs["ssr_path"], np.abs(got["ssr_path"][b, :k] / o["ssr_path"] - 1.0).max())
        errs["F"] = max(errs["F"], np.abs(got["F"][b] - o["f"]).max() / np.abs(o["f"]).max())
        errs["Lam"] = max(errs["Lam"], np.abs(got["Lam"][b][m] - o["lam"][m]).max() / np.abs(o["lam"][m]).max())
        errs["R2"] = max(errs["R2"], np.nanmax(np.abs(got["R2"][b] - o["R2"])))
    _report(f"als r={r} R={lg.als_width(r)} T={T} N={N}", **errs)
    for b, o in enumerate(refs):
        k = o["iters"]
        assert got["iters"][b] == k
        np.testing.assert_allclose(got["ssr_path"][b, :k], o["ssr_path"], rtol=1e-10)
        assert np.isnan(got["ssr_path"][b, k:]).all()
        np.testing.assert_allclose(got["ssr"][b], o["ssr"], rtol=1e-10)
        assert np.abs(got["F"][b] - o["f"]).max() <= 1e-8 * np.abs(o["f"]).max()
        assert np.array_equal(np.isnan(got["Lam"][b]), np.isnan(o["lam"]))          # the undefined rows
        assert np.isnan(got["Lam"][b, N - 1]).all()
        m = ~np.isnan(o["lam"])
        assert np.abs(got["Lam"][b][m] - o["lam"][m]).max() <= 1e-8 * np.abs(o["lam"][m]).max()
        np.testing.assert_allclose(got["R2"][b], o["R2"], rtol=0, atol=1e-9, equal_nan=True)


def test_als_factor_counts_differ_across_the_runs_of_a_batch(ctx):
    c = lg.ALS_MIXED
    z, F0, runs = lg.als_mixed_reference()
    re = np.array(c["r_each"])
    got = ctx.als_batch_host(z, np.repeat(F0[None], len(re), axis=0), r_each=re, nt_min=c["nt_min"], max_iter=c["max_iter"],
                             path_cap=c["max_iter"])
    for b, (r, o) in enumerate(zip(re, runs)):
        assert got["iters"][b] == o["iters"], r
        np.testing.assert_allclose(got["ssr"][b], o["ssr"], rtol=1e-9)
        assert np.isnan(got["F"][b][:, r:]).all() and np.isnan(got["Lam"][b][:, r:]).all()
        assert np.abs(got["F"][b][:, :r] - o["f"]).max() <= 1e-7 * np.abs(o["f"]).max()


# ------------------------------------------------------------------------------------------------ refusals
def _small_boot(ctx):
    ns, p, T, H = lg.BOOT_CASES[0][:4]
    ref = lg.boot_reference(ns, p, T, H)
    irf = ctx.var_bootstrap_irf_host(lg.var_data(ns, p, T), ref["betahat"], ref["resid"], p, H, 2, signs=np.ones((2, T)))
    np.testing.assert_allclose(irf[0], ref["point"], rtol=0, atol=1e-9 * np.abs(ref["point"]).max())


def _boot_inputs(ns, p, T):
    y = lg.var_data(ns, p, T)
    v = ao.estimate_var(y, p, 1, T)
    resid = np.zeros_like(y); resid[p:] = v["resid"][p:]
    return y, v["betahat"], resid


def test_bootstrap_lds_refusal_is_an_error_return(ctx):
    """NG = 32 groups of R = 8 lanes share the 160 KB: 640 doubles per draw.  A limitation, pinned here as it is."""
    from dynamic_factor_models_amd import DfmError
    for shape in (lg.BOOT_REFUSED, lg.BOOT_FIRST_REFUSED):
        ns, p, T = shape
        with pytest.raises(DfmError) as ei:
            ctx.var_bootstrap_irf_host(*_boot_inputs(ns, p, T), p, 3, 4, signs=np.ones((4, T)))
        assert ei.value.code == -1 and "LDS" in str(ei.value)         # DFM_E_DIMS
        _small_boot(ctx)                                              # the context is usable afterwards
    # the last shape that fits uses the whole 160 KB and runs: draw 0 with all signs +1 is the point estimate
    ns, p, T = lg.BOOT_LAST_FIT
    y, betahat, resid = _boot_inputs(ns, p, T)
    B = lg.groups(8) + 2
    irf = ctx.var_bootstrap_irf_host(y, betahat, resid, p, 3, B, signs=np.ones((B, T)))
    v = ao.estimate_var(y, p, 1, T)
    point = ao.impulse_response(v["M"], v["Q"], v["G"], range(ns), 3)
    np.testing.assert_allclose(irf[0], point, rtol=0, atol=1e-9 * np.abs(point).max())
    np.testing.assert_array_equal(irf[1:], np.repeat(irf[:1], B - 1, axis=0))


def test_quantile_refusal_above_the_cap(ctx):
    from dynamic_factor_models_amd import DfmError
    with pytest.raises(DfmError) as ei:
        ctx.quantile_bands_host(np.zeros((lg.QUANTILE_MAX_B + 1, 2)), np.array([0.5]))
    assert ei.value.code == -1                                        # DFM_E_DIMS
    np.testing.assert_array_equal(ctx.quantile_bands_host(np.array([[3.0], [1.0], [2.0]]), np.array([0.5])), [[2.0]])


def test_chow_refuses_a_bandwidth_above_15(ctx):
    from dynamic_factor_models_amd import DfmError
    ys, Xs, series, breaks, qs = lg.chow_data(2)
    bad = qs.copy(); bad[1] = 16
    with pytest.raises(DfmError) as ei:
        ctx.chow_batch_host(list(ys), list(Xs), series, breaks, bad)
    assert ei.value.code == -1                                        # DFM_E_DIMS
    got = ctx.chow_batch_host(list(ys), list(Xs), series[:5], breaks[:5], qs[:5])
    np.testing.assert_allclose(got, lg.chow_reference(2)[:5], rtol=1e-8)


def test_ols_refuses_65_regressors(ctx):
    from dynamic_factor_models_amd import DfmError
    assert lg.ols_width(65) is None
    with pytest.raises(DfmError) as ei:
        ctx.ols_batch_host(np.ones((70, 65)), np.ones((70, 2)))
    assert ei.value.code == -2                                        # DFM_E_R_UNSUPPORTED
    X, Y = lg.ols_data(1, 40, True)
    np.testing.assert_array_equal(ctx.ols_batch_host(X, Y)["nobs"], lg.ols_reference(1, 40, True)["nobs"])
