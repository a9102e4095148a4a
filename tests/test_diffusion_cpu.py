"""CPU checks of the diffusion-index evaluation (dfm_diffusion_eval_batch, csrc/diffusion.hip), no device needed: the expectation
model of tests/diffusion_expect.py against a second formulation (regressor matrices by lagmat, _ols, a triple loop for the scores);
the conditioning and the coverage of every case of tests/test_gpu_diffusion.py; the sensitivity figure that suite's end-to-end bar is
built on; the distance of every stop decision of its ALS case from the threshold; the argument checks of
api.forecast_diffusion_index and their order; the binding table and the constants the documents quote from the source."""
import os
import re

import numpy as np
import pytest

from oracle import als_oracle as ao
from tests import diffusion_expect as dx
from tests import rolling_expect as rx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_expectation_equals_a_second_formulation():
    x, origins, W, H, q, lags, nt_min, Fp = dx.als_case()
    origins = np.array([39, 45, 60, 69])                      # (one at the last row)
    T, N = x.shape
    r = Fp.shape[1]
    K = 1 + r + q
    e = dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=3, tol=0.0)
    assert np.all(e["iters"] == 3) and np.all(np.isfinite(e["F"]))
    seen = 0
    for b, o in enumerate(origins):
        win = x[o - W + 1:o + 1].copy()
        for i in range(N):
            win[W - lags[i]:, i] = np.nan
        z, _ = ao.standardize_data(win)
        mu, sd = np.nanmean(win, axis=0), np.nanstd(win, axis=0)
        F = e["F"][b]
        for i in range(N):
            l = int(lags[i])
            own = ao.lagmat(z[:, i], range(l, l + q))         # column m: z_{s-l-m,i}, NaN in front of the window
            X = np.column_stack([np.ones(W), F, own])
            for h in range(H + 1):
                if h + l == 0:
                    assert np.isnan(e["fc"][b, h, i]) and e["nobs_reg"][b, h, i] == 0
                    continue
                y = np.full(W, np.nan)
                y[:W - h] = z[h:, i]                          # the lead: y_s = z_{s+h,i}
                y[W - l - h:] = np.nan                        # s + h <= W - 1 - l
                ok = ~np.isnan(y) & ~np.isnan(X).any(axis=1)
                assert e["nobs_reg"][b, h, i] == ok.sum()
                if ok.sum() < max(nt_min, K):
                    assert np.isnan(e["fc"][b, h, i]) and np.all(np.isnan(e["beta"][b, h, i]))
                    continue
                bt, res = ao._ols(y[ok], X[ok])
                ba, _ = ao._ols(y[ok], X[ok][:, [0] + list(range(1 + r, K))])
                assert np.abs(bt - e["beta"][b, h, i]).max() <= 1e-10
                fz, fa = X[W - 1] @ bt, X[W - 1][[0] + list(range(1 + r, K))] @ ba
                for got, want in ((e["fc"][b, h, i], mu[i] + sd[i] * fz), (e["fc_ar"][b, h, i], mu[i] + sd[i] * fa)):
                    assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-10 * max(1.0, abs(want)), (b, h, i)
                v = sd[i] ** 2 * (res @ res) / (ok.sum() - K)
                assert abs(e["fvar"][b, h, i] - v) <= 1e-10 * max(1.0, v)
                seen += 1
    assert seen > 100
    # the scores by a triple loop
    sse = np.zeros((H + 1, N)); ssa = np.zeros((H + 1, N)); sse0 = np.zeros((H + 1, N)); cnt = np.zeros((H + 1, N), dtype=int)
    for b, o in enumerate(origins):
        for h in range(H + 1):
            for i in range(N):
                scored = o + h < T and np.isfinite(e["fc"][b, h, i]) and not np.isnan(x[min(o + h, T - 1), i])
                if not scored:
                    assert np.isnan(e["err"][b, h, i]) and np.isnan(e["err_ar"][b, h, i]) and np.isnan(e["err_std"][b, h, i])
                    continue
                er = x[o + h, i] - e["fc"][b, h, i]
                assert abs(e["err"][b, h, i] - er) <= 1e-10 and abs(e["err_ar"][b, h, i] - (x[o + h, i] - e["fc_ar"][b, h, i])) <= 1e-10
                assert abs(e["err_std"][b, h, i] - er / np.sqrt(e["fvar"][b, h, i])) <= 1e-10
                sse[h, i] += er ** 2; ssa[h, i] += e["err_ar"][b, h, i] ** 2; sse0[h, i] += (x[o + h, i] - e["mean"][b, i]) ** 2
                cnt[h, i] += 1
    assert np.array_equal(e["cnt"], cnt) and cnt[0, lags == 0].max() == 0 and cnt[0, lags > 0].max() > 1
    have = cnt > 0
    for k, s in (("msfe", sse), ("msfe_ar", ssa), ("msfe0", sse0)):
        assert np.all(np.isnan(e[k][~have])) and np.abs(e[k][have] - (s / np.maximum(cnt, 1))[have]).max() <= 1e-10, k
    assert np.all(np.isnan(e["err"][3, 1:])) and np.isfinite(e["fc"][3, 1:]).any()      # the origin at T - 1: forecasts, no scores


@pytest.mark.parametrize("r,q", dx.RQ)
def test_gpu_cases_are_conditioned_and_cover_the_refusals(r, q):
    """Every regression of every kernels-alone case of the GPU suite (those of H = 0 and 1 are among those of the largest H the
    grid allows): lstsq and float64 normal equations on the equilibrated Gram matrix agree to 1e-10, so the inputs are conditioned
    for the 1e-9 bar on the device's unpivoted elimination.  Over the cases of one (r, q) at least one regression is refused as thin
    and one is not, and (q > 0: there is an own lag) one forecast is NaN for a missing own lag at the origin."""
    K = 1 + r + q
    nt_min = dx.kernel_nt_min(r, q)
    thin = solved = lag_nan = 0
    worst = 0.0
    for N in dx.NS:
        for W in dx.windows_of(r, q):
            Hs = [H for H in dx.HS if not dx.refused(r, q, W, H)]
            if not Hs:
                continue
            H = max(Hs)
            for variant in dx.VARIANTS:
                x, origins, lags, Fp, _ = dx.kernel_case(N, W, r, q, variant)
                lg = np.zeros(N, dtype=int) if lags is None else lags
                _, _, _, z = rx.standardise(rx.windows(x, origins, W, lags))
                F = dx.start_windows(Fp, origins, W)
                for b in range(origins.size):
                    for i in range(N):
                        u0 = dx.origin_row(z[b], F[b], i, int(lg[i]), q)
                        for h in range(H + 1):
                            if h + lg[i] < 1:
                                continue
                            U, y, ok = dx.design(z[b], F[b], i, int(lg[i]), h, q)
                            if ok.sum() < max(nt_min, K):
                                thin += 1
                                continue
                            solved += 1
                            U, y = U[ok], y[ok]
                            bl = np.linalg.lstsq(U, y, rcond=None)[0]
                            G = U.T @ U
                            d = 1.0 / np.sqrt(np.diag(G))
                            bn = d * np.linalg.solve(G * d[:, None] * d[None, :], d * (U.T @ y))
                            worst = max(worst, np.abs(bl - bn).max() / max(1.0, np.abs(bl).max()))
                            lag_nan += bool(np.isnan(u0).any())
    print(f"r={r} q={q}: {solved} regressions solved, {thin} refused, {lag_nan} NaN at the origin, lstsq vs normal {worst:.2e}")
    assert worst <= 1e-10
    assert thin > 0 and solved > 0
    assert lag_nan > 0 or q == 0


def _converged():
    x, origins, W, H, q, lags, nt_min, Fp = dx.als_case()
    return dx.expect(x, origins, W, H, Fp, q, lags=lags, nt_min=nt_min, max_iter=2000, tol=dx.ALS_TOL), (x, origins, W, H, q, lags, nt_min)


def test_sensitivity_of_the_forecasts_to_the_factor_parity():
    """The oracle's converged factors of als_case() moved by 1e-8 max|F| (uniform in every entry, five seeds): the largest change of
    fc / win_sd and fc_ar / win_sd is 1.5e-7 -- the figure behind dx.SENSITIVITY (2e-7), DESIGN.md section 30 and the end-to-end bar
    of tests/test_gpu_diffusion.py."""
    e, (x, origins, W, H, q, lags, nt_min) = _converged()
    worst = 0.0
    for seed in range(5):
        rng = np.random.default_rng(seed)
        Fm = e["F"] + dx.ALS_PARITY * np.abs(e["F"]).max() * rng.uniform(-1.0, 1.0, e["F"].shape)
        p = dx.expect(x, origins, W, H, e["F"], q, lags=lags, nt_min=nt_min, F=Fm)
        assert np.array_equal(np.isnan(p["fc"]), np.isnan(e["fc"]))
        worst = max(worst, np.nanmax(np.abs(p["fc"] - e["fc"]) / e["sd"][:, None, :]))
    print("sensitivity of fc / win_sd:", worst)
    assert 0.0 < worst <= dx.SENSITIVITY and dx.SENSITIVITY <= 4.0 * worst


def test_stop_decisions_of_the_gpu_als_case_are_far_from_the_threshold():
    e, (x, origins, W, H, q, lags, nt_min) = _converged()
    thresh = dx.ALS_TOL * W * x.shape[1]
    closest = np.inf
    for b in range(origins.size):
        path = np.concatenate([[0.0], e["paths"][b]])
        d = np.abs(path[:-1] - path[1:])
        assert np.all(d[:-1] >= thresh) and d[-1] < thresh, b      # the stop is the rule's, not max_iter's
        closest = min(closest, np.abs(d - thresh).min() / thresh)
    print("closest stop decision (relative to the threshold):", closest, "sweeps:", e["iters"])
    assert closest >= 100 * dx.ALS_PARITY
    assert e["iters"].max() < 2000 and np.unique(e["iters"]).size > 1


def _model(T=60, ns=8, r=2):
    from dynamic_factor_models_amd import api
    x = np.random.default_rng(4).standard_normal((T, ns))
    x[5, 3] = np.nan
    return api, api.DFMModel(x, np.ones(ns), 5, 5, 3, 58, 0, r, 1e-8, 2, 1)


def test_api_argument_checks_and_their_order(monkeypatch):
    api, m = _model()

    def no_device(ctx):
        raise AssertionError("the device was touched before the argument checks were through")
    monkeypatch.setattr(api, "_own", no_device)
    fdi = api.forecast_diffusion_index
    rows = 56                                                  # periods 3 .. 58
    F = np.random.default_rng(1).standard_normal((rows, 2))
    cases = [("H must be", dict(H=-1, window=99)),             # (two rules broken: the earlier one answers)
             ("own_lags", dict(H=2, window=99, own_lags=-1)),
             ("own_lags", dict(H=2, window=20, own_lags=30)),
             ("window", dict(H=2, window=57, step=0)),
             ("window", dict(H=2, window=10)),                 # 1 + r + 2 own_lags + H + 2 = 11
             ("step", dict(H=2, window=20, step=0, origins=[21])),
             ("origins", dict(H=2, window=20, origins=[21, 30], start=F[:5])),      # the first full window ends at period 22
             ("origins", dict(H=2, window=20, origins=[30, 30])),
             ("start must be", dict(H=2, window=20, start=F[:5])),
             ("estimate_factor", dict(H=2, window=20, max_iter=-1)),                # m.factor is still NaN
             ("max_iter", dict(H=2, window=20, start=F, max_iter=-1, lags=[0])),
             ("lags", dict(H=2, window=20, start=F, lags=[0, 0, -1, 0, 0, 0, 0, 0])),
             ("publication lag", dict(H=2, window=20, start=F, lags=[0, 0, 16, 0, 0, 0, 0, 0])),
             ("reach the origin", dict(H=2, window=20, start=F, lags=[1] * 8))]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            fdi(m, kw.pop("H"), kw.pop("window"), **kw)
    m.nfac_o = 1
    with pytest.raises(ValueError, match="nfac_o"):
        fdi(m, 2, 20, start=F)
    m.nfac_o = 0
    before = m.factor.copy()
    with pytest.raises(AssertionError, match="device was touched"):   # every check passed: the next step is the device
        fdi(m, 2, 20, start=F)
    assert np.array_equal(before, m.factor, equal_nan=True)


def test_binding_table_header_and_build_list():
    from dynamic_factor_models_amd import _lib, build, kalman
    assert _lib.SYMBOLS["dfm_diffusion_eval_batch"] == _lib.SYMBOLS["dfm_diffusion_eval_batch_dev"]
    header = re.sub(r"/\*.*?\*/", "", _src("include", "dfm_hip.h"), flags=re.S)
    for name in ("dfm_diffusion_eval_batch", "dfm_diffusion_eval_batch_dev"):
        proto = re.search(name + r"\s*\(([^)]*)\)\s*;", header).group(1)
        assert len(proto.split(",")) == len(_lib.SYMBOLS[name][1]) == 38, name
    assert build.SOURCES.count("diffusion.hip") == 1 and os.path.exists(os.path.join(build.CSRC, "diffusion.hip"))
    assert callable(kalman.DfmContext.diffusion_eval_batch) and callable(kalman.DfmContext.diffusion_eval_batch_host)
    jl = _src("julia", "dfm_hip.jl")
    assert "function forecast_diffusion_index" in jl and "(:dfm_diffusion_eval_batch, LIB)" in jl


def test_constants_the_tests_and_documents_quote():
    capi, di = _src("dynamic_factor_models_amd", "csrc", "capi.hip"), _src("dynamic_factor_models_amd", "csrc", "diffusion.hip")
    design = _src("DESIGN.md")
    sec = design[design.index("## 30."):]
    assert "kRwSlice = 1024" in capi and "1024" in sec            # the slice the GPU suite's two-slice case is built around
    for name in ("di_start_kernel", "di_regress_kernel", "di_score_kernel"):
        assert f'"{name}"' in capi and f"void {name}(" in di and name in sec
    assert "constexpr int kDiSeries = 16;" in di and "16 series" in sec      # the block the cases straddle (N = 16, 17, 65)
    assert "constexpr int kDiThreads = 256;" in di
    assert "atomicAdd" not in di                                  # sums in a fixed order
    assert f"{dx.SENSITIVITY:g}" in sec and "1.5e-7" in sec       # the sensitivity figure and the constant built on it
    assert dx.kernel_nt_min(8, 23) == 36 and dx.refused(8, 7, 24, 0) and not dx.refused(8, 7, 33, 4) and not dx.refused(8, 23, 80, 4)
