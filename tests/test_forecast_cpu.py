"""CPU tests of the forecast entry points (include/dfm_hip.h dfm_forecast_batch, api.forecast): the C-ABI's argument check
without a handle, api.forecast's refusals before any device work, and the expectation model the GPU tests use
(tests/forecast_expect.py) against the closed-form forecast tail."""
import ctypes

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests.forecast_expect import closed_form_tail, expect


def test_forecast_without_a_handle_is_dfm_e_null():
    from dynamic_factor_models_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.dfm_forecast_batch, lib.dfm_forecast_batch_dev):
        rc = fn(None, 1, 4, 3, 1, 1, 2, *([ptr] * 7), None, None, ptr, None, None, ptr, None, None, 0)
        assert rc == -3


class _NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("api.forecast touched the device before refusing")


def _model(nfac_o=0):
    from dynamic_factor_models_amd import api
    rng = np.random.default_rng(5)
    data = rng.standard_normal((60, 12))
    data[55:, 3] = np.nan
    return api.DFMModel(data, np.ones(12, dtype=int), 20, 20, 1, 50, nfac_o, 2, 1e-8, 1, 1)


def _fake_fit(m):
    r = m.nfac_u
    m.em_params = dict(Lam=np.ones((12, r)), R=np.ones(12), A=0.5 * np.eye(r), Q=np.eye(r), mu0=np.zeros(r), P0=np.eye(r))


@pytest.fixture
def no_device(monkeypatch):
    from dynamic_factor_models_amd import kalman
    monkeypatch.setattr(kalman, "DfmContext", _NoDevice)


def test_api_forecast_refuses_before_device_work(no_device):
    from dynamic_factor_models_amd import api
    m = _model()
    with pytest.raises(ValueError, match="estimate"):
        api.forecast(m, 4)                                    # not estimated
    _fake_fit(m)
    with pytest.raises(ValueError, match="H"):
        api.forecast(m, -1)
    for bad in (49, 61):
        with pytest.raises(ValueError, match="through"):
            api.forecast(m, 4, through=bad)
    with pytest.raises(ValueError, match="replicates"):
        api.forecast(m, 4, quantiles=[0.1, 0.9])
    mo = _model(nfac_o=1)
    _fake_fit(mo)
    with pytest.raises(ValueError, match="nfac_o"):
        api.forecast(mo, 4)
    before = {k: v.copy() for k, v in m.em_params.items()}
    fac = m.factor.copy()
    with pytest.raises(AssertionError, match="touched the device"):
        api.forecast(m, 4, through=60)                        # every check passed: the next step is the device
    assert all(np.array_equal(before[k], m.em_params[k]) for k in before)
    assert np.array_equal(fac, m.factor, equal_nan=True)


def _close(a, b, tol, what):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f"{what}: {err:.3e}"


@pytest.mark.parametrize("r,H,missing", [(1, 5, 0.0), (3, 12, 0.1), (4, 1, 0.2)])
def test_expectation_model_matches_the_closed_form_var1_tail(r, H, missing):
    x, st = ko.synth_replicate(7, 30, 80, r, missing=missing)
    x[-1, :20] = np.nan                                       # a ragged last row
    e = expect(x, st["Lam"], st["R"], st["A"], st["Q"], st["mu0"], st["P0"], H)
    o = ko.kfs_pass(x, st["Lam"], st["R"], st["A"], st["Q"], st["mu0"], st["P0"], lag_one=False)
    T = x.shape[0]
    _close(e["f"][:T], o["f_smooth"], 1e-12, "smoothed rows")
    _close(e["Pfull"][:T], o["P_smooth"], 1e-12, "smoothed covariances")
    assert abs(e["loglik"] - o["loglik"]) <= 1e-12 * abs(o["loglik"])
    ft, Pt = closed_form_tail(o["f_smooth"][-1], o["P_smooth"][-1], st["A"], st["Q"], H)
    _close(e["f"][T:], ft, 1e-12, "forecast f")
    _close(e["Pfull"][T:], Pt, 1e-12, "forecast P")
    Lam, R = st["Lam"], st["R"]
    _close(e["xhat"][T:], ft @ Lam.T, 1e-12, "forecast x")
    _close(e["xvar"][T:], np.einsum("ij,hjk,ik->hi", Lam, Pt, Lam) + R, 1e-12, "forecast variance")
    obs = ~np.isnan(x)
    assert np.array_equal(e["xhat"][:T][obs], x[obs]) and np.all(e["xvar"][:T][obs] == 0.0)
    mean, sd = np.linspace(-1, 1, 30), np.linspace(0.5, 2, 30)
    es = expect(x, st["Lam"], st["R"], st["A"], st["Q"], st["mu0"], st["P0"], H, mean=mean, sd=sd)
    _close(es["xhat"], mean + sd * e["xhat"], 1e-12, "un-standardised x")
    _close(es["xvar"], sd ** 2 * e["xvar"], 1e-12, "un-standardised variance")


def test_expectation_model_matches_the_closed_form_companion_tail():
    r, p, H = 2, 3, 6
    x = vo.synth_varp(3, 25, 70, r, p, missing=0.1)
    q, _ = vo.varp_init(np.nan_to_num(x), r, p)
    e = expect(x, q["Lam"], q["R"], q["Avar"], q["Q"], q["mu0"], q["P0"], H, p=p)
    o = vo.kfs_pass_varp(x, q["Lam"], q["R"], q["Avar"], q["Q"], q["mu0"], q["P0"], p)
    M, Qk = vo.companion(q["Avar"], q["Q"], p)
    ft, Pt = closed_form_tail(o["f_smooth"][-1], o["P_smooth"][-1], M, Qk, H)
    T = x.shape[0]
    _close(e["f"][:T], o["f_smooth"][:, :r], 1e-12, "smoothed rows")
    _close(e["f"][T:], ft[:, :r], 1e-12, "forecast f")
    _close(e["Pfull"][T:], Pt[:, :r, :r], 1e-12, "forecast P")
    assert abs(e["loglik"] - o["loglik"]) <= 1e-12 * abs(o["loglik"])
