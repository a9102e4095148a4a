"""GPU tests of the parametric bootstrap on the device, through the public interface on the Stock-Watson panel
(tests/golden/sw_panel.npz; the small models the neighbouring api tests build):
  estimate(..., factor_lags = 2, nrep = 8) fills m.replicates from dfm_simulate_batch and dfm_em_varp_batch_dev -- the panels
  are the contract's (tests/simulate_expect.py), every log-likelihood path is finite and non-decreasing, the replicates are
  what dfm_em_varp_batch gives on the returned panels (the driver adds nothing to the two calls), and forecast / structural_irf
  take them for their bands; the same for estimate_ar_idio(nrep = 8) with forecast_ar_idio(params=, quantiles=) and
  evaluate_forecasts_ar_idio(params=); factor_lags = 1 with draws="device"; and the default at factor_lags = 1, whose panels
  stay those of the host loop."""
import os

import numpy as np
import pytest

from tests import simulate_expect as sx

pytestmark = pytest.mark.gpu
NREP, ITERS, SEED = 8, 3, 11
AR_KEYS = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _sw_model(lags, uarlag=4, last=216):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, last, 0, 4, 1e-8, uarlag, lags)


def _paths_ok(rep, nrep=NREP, iters=ITERS):
    path, it = rep["loglik_path"], rep["iters"]
    assert path.shape == (nrep, iters) and it.shape == (nrep,) and np.all(it >= 1) and np.all(it <= iters)
    for b in range(nrep):
        row = path[b, :it[b]]
        assert np.all(np.isfinite(row)), (b, row)
        # (non-decreasing up to the rounding of a sum of ~T N terms in fp64: 1e-10 of its size is a thousand times that)
        assert np.all(np.diff(row) >= -1e-10 * np.abs(row[:-1])), (b, row)


def _same(a, b, what, tol=1e-10):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= tol * max(1.0, float(np.abs(b).max())), f"{what}: {err:.3e}"


def _bands_ok(bands, shape):
    assert bands.shape == shape and np.all(np.isfinite(bands)) and np.all(np.diff(bands, axis=0) >= 0.0)


def test_varp_replicates(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(2)
    api.estimate(m, api.Parametric(), max_em_iter=ITERS, tol_em=0.0, factor_lags=2, ctx=ctx, nrep=NREP, seed=SEED)
    rep, ep = m.replicates, m.em_params
    assert {"params", "loglik_path", "iters", "iterations", "panels"} <= set(rep)
    _paths_ok(rep)
    cols, z, _, _ = api._forecast_inputs(m, m.lastperiod)
    T, N, r = z.shape[0], cols.size, 4
    assert rep["panels"].shape == (NREP, T, N) and np.array_equal(np.isnan(rep["panels"]), np.broadcast_to(np.isnan(z), (NREP, T, N)))
    for b in (0, NREP - 1):                                              # replicate b is draw b of the point estimate
        x, _ = sx.simulate(ep["Lam"], ep["R"], ep["Avar"], ep["Q"], ep["mu0"], ep["P0"], T, SEED, 0, b, 0, mask=z)
        keep = ~np.isnan(z)
        _same(rep["panels"][b][keep], x[keep], f"panel {b}", 1e-9)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (NREP,) + a.shape))
    new, path, iters, _, _ = ctx.em_varp_batch_host(rep["panels"], *[tile(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")],
                                                    max_iter=ITERS, tol=0.0)
    assert np.array_equal(iters, rep["iters"])
    _same(rep["loglik_path"], path, "loglik_path")
    for k in ("Lam", "R", "Avar", "Q", "mu0", "P0"):
        _same(rep["params"][k], new[k], k)
    assert np.array_equal(rep["params"]["A"], rep["params"]["Avar"]) and rep["params"]["A"].shape == (NREP, r, 2 * r)
    q = np.array([0.1, 0.5, 0.9])
    H = 6
    fc = api.forecast(m, H, quantiles=q, ctx=ctx)
    _bands_ok(fc["bands"], (3, H, N))
    from tests import structural_expect as se
    named = cols[se.greedy_named(ep["Lam"])]
    o = api.structural_irf(m, H, named=named, quantiles=q, ctx=ctx)
    _bands_ok(o["bands"], (3, N, H, r))


def test_lag_one_on_the_device_and_the_host_default(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(1)
    api.estimate(m, api.Parametric(), max_em_iter=ITERS, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=NREP, seed=SEED, draws="device")
    _paths_ok(m.replicates)
    ep = m.em_params
    cols, z, _, _ = api._forecast_inputs(m, m.lastperiod)
    T, N = z.shape
    x, _ = sx.simulate(ep["Lam"], ep["R"], ep["A"], ep["Q"], ep["mu0"], ep["P0"], T, SEED, 0, 3, 0, mask=z)
    _same(m.replicates["panels"][3][~np.isnan(z)], x[~np.isnan(z)], "panel 3", 1e-9)
    assert m.replicates["params"]["A"].shape == (NREP, 4, 4)
    _bands_ok(api.forecast(m, 4, quantiles=[0.1, 0.9], ctx=ctx)["bands"], (2, 4, N))
    # the default at factor_lags = 1: the host loop's panels for the same seed, restated
    m2 = _sw_model(1)
    api.estimate(m2, api.Parametric(), max_em_iter=ITERS, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=3, seed=SEED)
    e2 = m2.em_params
    rng = np.random.default_rng(SEED)
    LQ, LS, sq = api._psd_sqrt(e2["Q"]), api._psd_sqrt(e2["P0"]), np.sqrt(e2["R"])
    panels = np.empty((3, T, N))
    for b in range(3):
        f = e2["mu0"] + LS @ rng.standard_normal(4)
        for t in range(T):
            f = e2["A"] @ f + LQ @ rng.standard_normal(4)
            panels[b, t] = e2["Lam"] @ f + sq * rng.standard_normal(N)
    panels[:, np.isnan(z)] = np.nan
    assert np.array_equal(m2.replicates["panels"], panels, equal_nan=True)
    assert all(np.array_equal(e2[k], ep[k]) for k in ep), "draws= changed the point estimate"


def test_ar_idio_replicates(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(2, uarlag=2)
    api.estimate(m, api.NonParametric(), ctx=ctx)
    q = m.n_uarlag
    path = api.estimate_ar_idio(m, max_em_iter=ITERS, tol_em=0.0, nrep=NREP, seed=SEED, ctx=ctx)
    assert path.ndim == 1 and 1 <= path.size <= ITERS
    rep = m.replicates_ar
    assert {"params", "loglik_path", "iters"} <= set(rep) and set(rep["params"]) == set(AR_KEYS)
    _paths_ok(rep)
    fit, panels = rep["fit"], rep["panels"]
    inp = api._ar_model_inputs(m)[0]
    assert all(rep["params"][k].shape == (NREP,) + inp[k].shape for k in AR_KEYS)
    x0 = panels[0]
    T, N = x0.shape
    assert np.array_equal(panels[:, :q], np.broadcast_to(x0[:q], (NREP, q, N)), equal_nan=True)   # conditional on the first q rows
    assert all(np.array_equal(np.isnan(panels[b]), np.isnan(x0)) for b in range(NREP))
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a[0], (NREP,) + a.shape[1:]))
    new, lp, iters, _, _ = ctx.em_ar_batch_host(panels, *[tile(fit[k]) for k in AR_KEYS], max_iter=ITERS, tol=0.0)
    assert np.array_equal(iters, rep["iters"])
    _same(rep["loglik_path"], lp, "loglik_path")
    for k in AR_KEYS:
        _same(rep["params"][k], new[k], k)
    H = 4
    plain = api.forecast_ar_idio(m, H, ctx=ctx)
    fc = api.forecast_ar_idio(m, H, params=rep["params"], quantiles=[0.1, 0.5, 0.9], ctx=ctx)
    _bands_ok(fc["bands"], (3, H, N))
    assert np.array_equal(fc["x"], plain["x"], equal_nan=True) and "bands" not in plain
    ev = api.evaluate_forecasts_ar_idio(m, 2, params=rep["params"], quantiles=[0.25, 0.75], ctx=ctx)
    assert ev["bands"].shape == (2, 2, N) and np.all(np.diff(ev["bands"], axis=0)[0][np.isfinite(ev["bands"][0])] >= 0.0)
    sim = api.simulate_ar_idio(m, 2, seed=SEED, ctx=ctx)
    assert sim["x"].shape == (2, T, N) and sim["factor"].shape == (2, T - q, 4)
    free = api.simulate_ar_idio(m, 2, seed=SEED, masked=False, ctx=ctx)
    assert not np.isnan(free["x"]).any()


def test_api_simulate(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model(2)
    api.estimate(m, api.Parametric(), max_em_iter=ITERS, tol_em=0.0, factor_lags=2, ctx=ctx)
    cols, z, mu, sd = api._forecast_inputs(m, m.lastperiod)
    o = api.simulate(m, 3, seed=5, ctx=ctx)
    T, N = z.shape
    assert o["x"].shape == (3, T, N) and o["factor"].shape == (3, T, 4) and np.array_equal(o["cols"], cols)
    assert np.array_equal(np.isnan(o["x"]), np.broadcast_to(np.isnan(z), (3, T, N)))
    ep = m.em_params
    x, f = sx.simulate(ep["Lam"], ep["R"], ep["Avar"], ep["Q"], ep["mu0"], ep["P0"], T, 5, 0, 2, 0)
    _same(o["factor"][2], f, "factor", 1e-9)
    keep = ~np.isnan(z)
    _same(o["x"][2][keep], (mu + sd * x)[keep], "x in data units", 1e-9)
    assert not np.isnan(api.simulate(m, 1, seed=5, masked=False, ctx=ctx)["x"]).any()
