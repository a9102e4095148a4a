"""CPU checks of the rolling-window evaluation (dfm_rolling_eval_batch, csrc/rolling.hip), no device needed: the expectation model
of tests/rolling_expect.py against brute-force Gaussian conditioning and a naive scoring loop, the distance of every stop decision
of the GPU suite's EM parity case from its tolerance, the argument checks of api.evaluate_forecasts_rolling, the binding table and
the constants the documents quote from the source."""
import os
import re

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from tests import rolling_expect as rx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8                                     # tests/test_gpu_em.py


def _src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_expectation_equals_brute_force_conditioning_and_a_naive_score():
    N, T, W, H, r = 5, 14, 8, 2, 2
    rng = np.random.default_rng(5)
    z, tr = ko.synth_replicate(3, N, T, r)
    x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
    x[rng.random((T, N)) < 0.1] = np.nan
    lags = np.array([0, 1, 2, 0, 1])
    origins = np.array([9])
    start = dict(Lam=tr["Lam"][None], R=tr["R"][None], Avar=tr["A"][None], Q=tr["Q"][None], mu0=tr["mu0"][None], P0=tr["P0"][None])
    e = rx.expect(x, origins, W, H, start, lags=lags, max_iter=2)
    # the vintage by hand
    o = origins[0]
    win = x[o - W + 1:o + 1].copy()
    for i in range(N):
        for t in range(W):
            if o - W + 1 + t > o - lags[i]:
                win[t, i] = np.nan
    mu = np.array([np.nanmean(win[:, i]) for i in range(N)]); sd = np.array([np.nanstd(win[:, i]) for i in range(N)])
    zw = (win - mu) / sd
    assert np.array_equal(np.isnan(e["win"][0]), np.isnan(zw))
    assert np.nanmax(np.abs(e["win"][0] - zw)) <= 1e-10 and np.abs(e["mean"][0] - mu).max() <= 1e-10 and np.abs(e["sd"][0] - sd).max() <= 1e-10
    assert np.array_equal(e["nobs"][0], (~np.isnan(win)).sum(axis=0))
    # forecasts: Gaussian conditioning on the window with H all-missing rows appended, at the parameters the EM returned
    q = {k: e["params"][k][0] for k in rx.KEYS}
    zp = np.vstack([zw, np.full((H, N), np.nan)])
    bf = ko.brute_force_gaussian(zp, q["Lam"], q["R"], q["Avar"], q["Q"], q["mu0"], q["P0"])
    for h in range(H + 1):
        t = W - 1 + h
        for i in range(N):
            lam = q["Lam"][i]
            if np.isnan(zp[t, i]):
                m, v = mu[i] + sd[i] * lam @ bf["f_smooth"][t], sd[i] ** 2 * (lam @ bf["P_smooth"][t] @ lam + q["R"][i])
            else:
                m, v = mu[i] + sd[i] * zp[t, i], 0.0
            assert abs(e["fc"][0, h, i] - m) <= 1e-10 * max(1.0, abs(m)), (h, i)
            assert abs(e["fvar"][0, h, i] - v) <= 1e-10 * max(1.0, abs(v)), (h, i)
    # scoring: several origins, one at the last row, by a triple loop
    origins = np.array([7, 9, 10, 13])
    e = rx.expect(x, origins, W, H, start, lags=lags, max_iter=0)
    sse = np.zeros((H + 1, N)); sse0 = np.zeros((H + 1, N)); cnt = np.zeros((H + 1, N), dtype=int)
    for b, o in enumerate(origins):
        for h in range(H + 1):
            for i in range(N):
                scored = o + h < T and (h >= 1 or lags[i] > 0) and not np.isnan(x[min(o + h, T - 1), i])
                if not scored:
                    assert np.isnan(e["err"][b, h, i]) and np.isnan(e["err_std"][b, h, i])
                    continue
                er = x[o + h, i] - e["fc"][b, h, i]
                assert abs(e["err"][b, h, i] - er) <= 1e-10 and abs(e["err_std"][b, h, i] - er / np.sqrt(e["fvar"][b, h, i])) <= 1e-10
                sse[h, i] += er ** 2; sse0[h, i] += (x[o + h, i] - e["mean"][b, i]) ** 2; cnt[h, i] += 1
    assert np.array_equal(e["cnt"], cnt) and cnt[0, lags == 0].max() == 0 and cnt.max() > 1
    have = cnt > 0
    assert np.all(np.isnan(e["msfe"][~have])) and np.all(np.isnan(e["msfe0"][~have]))
    assert np.abs(e["msfe"][have] - (sse / np.maximum(cnt, 1))[have]).max() <= 1e-10
    assert np.abs(e["msfe0"][have] - (sse0 / np.maximum(cnt, 1))[have]).max() <= 1e-10
    assert np.all(np.isfinite(e["fc"])) and np.all(np.isnan(e["err"][3, 1:]))      # the origin at T - 1: forecasts, no scores


def test_stop_decisions_of_the_gpu_parity_case_are_far_from_the_tolerance():
    x, origins, W, H, lags, start = rx.em_parity_case()
    tol, max_iter = 1e-4, 30
    e = rx.expect(x, origins, W, 0, start, lags=lags, max_iter=max_iter, tol=tol)
    closest = np.inf
    for b in range(origins.size):
        path = e["paths"][b]
        rel = (path[1:] - path[:-1]) / (0.5 * (np.abs(path[1:]) + np.abs(path[:-1])))
        closest = min(closest, np.abs(rel - tol).min())
        assert np.all(rel[:-1] >= tol) and rel[-1] < tol, b       # the stop is the rule's, not max_iter's
    print("closest stop decision:", closest, "iterations:", e["iters"])
    assert closest >= 100 * RTOL
    assert e["iters"].min() >= 3 and e["iters"].max() < max_iter and np.unique(e["iters"]).size > 1    # the per-window stop is exercised


def _fitted_model(T=60, ns=8, r=2):
    from dynamic_factor_models_amd import api
    x = np.random.default_rng(4).standard_normal((T, ns))
    x[5, 3] = np.nan
    m = api.DFMModel(x, np.ones(ns), 5, 5, 3, 58, 0, r, 1e-8, 4, 1)
    return api, m, dict(Lam=np.ones((ns, r)), R=np.ones(ns), A=0.5 * np.eye(r), Q=np.eye(r), mu0=np.zeros(r), P0=np.eye(r))


def test_api_argument_checks_run_before_any_device_work():
    api, m, fit = _fitted_model()
    with pytest.raises(ValueError, match="not been estimated"):
        api.evaluate_forecasts_rolling(m, 2, window=20)
    m.em_params = fit
    with pytest.raises(ValueError, match="window"):
        api.evaluate_forecasts_rolling(m, 2, window=57)            # rows 3..58: 56 of them
    with pytest.raises(ValueError, match="H must be"):
        api.evaluate_forecasts_rolling(m, -1, window=20)
    with pytest.raises(ValueError, match="origins"):
        api.evaluate_forecasts_rolling(m, 2, window=20, origins=[21, 30])     # the first full window ends at period 22
    with pytest.raises(ValueError, match="lags"):
        api.evaluate_forecasts_rolling(m, 2, window=20, lags=[0, 0, -1, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="publication lag"):
        api.evaluate_forecasts_rolling(m, 2, window=20, lags=[0, 0, 16, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="factor_lags"):
        api.evaluate_forecasts_rolling(m, 2, window=20, factor_lags=2)
    assert m.em_params is fit


def test_binding_table_header_and_build_list():
    from dynamic_factor_models_amd import _lib, build
    assert "dfm_rolling_eval_batch" in _lib.SYMBOLS and "dfm_rolling_eval_batch_dev" in _lib.SYMBOLS
    assert _lib.SYMBOLS["dfm_rolling_eval_batch"] == _lib.SYMBOLS["dfm_rolling_eval_batch_dev"]
    assert _lib.ERRORS[-9] == "DFM_E_WINDOW"
    assert re.search(r"DFM_E_WINDOW\s*=\s*-9\b", _src("include", "dfm_hip.h"))
    assert build.SOURCES.count("rolling.hip") == 1 and os.path.exists(os.path.join(build.CSRC, "rolling.hip"))
    from dynamic_factor_models_amd import kalman
    assert callable(kalman.DfmContext.rolling_eval_batch) and callable(kalman.DfmContext.rolling_eval_batch_host)


def test_constants_the_tests_and_documents_quote():
    capi, rw, kh = _src("dynamic_factor_models_amd", "csrc", "capi.hip"), _src("dynamic_factor_models_amd", "csrc", "rolling.hip"), \
        _src("dynamic_factor_models_amd", "csrc", "dfm_kernels.h")
    assert "kRwSlice = 1024" in capi                              # the slice the GPU suite's two-slice case is built around
    assert "DevBlock rw;" in capi and "&h->gb, &h->rw}) b->release();" in capi
    for name in ("rolling_window_kernel", "rolling_start_kernel", "rolling_score_kernel"):
        assert f'"{name}"' in capi and f"void {name}(" in rw
    assert "constexpr int kRwSeries = 64;" in rw                  # the series block the geometry table straddles (N = 64, 65, 130)
    assert "constexpr int kRwWindowBit = 128;" in kh
    assert "atomicAdd" not in rw                                  # sums in a fixed order
