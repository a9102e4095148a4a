"""CPU checks of the simulated-panel entries (dfm_simulate_batch, dfm_simulate_ar_batch), none of which needs a device:
  (a) the contract of tests/simulate_expect.py really simulates the model: sample moments of its draws against the covariance
      the model implies, built from the companion form alone -- a wrong contract (a dropped sqrt, a transposed root, a lag block
      off by one) cannot pass;
  (b) the restated launch geometry of the two kernels against cell_geometry / series_geometry of csrc/dfm_cellgeom.h compiled
      for the host, and the constants and launch lines the restatement takes from csrc/simulate.hip, read from the source;
  (c) the argument checks of the public interface, which run before any device work."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import post_geometry as pg
from tests import simulate_expect as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, R_, P_, Q_ = 6, 5, 2, 2, 2
D = 4000
SEED = 20240607


def _model(q):
    rng = np.random.default_rng([11, q])
    Lam = rng.standard_normal((N, R_))
    R = rng.uniform(0.3, 1.2, N)
    A = np.hstack([0.5 * np.eye(R_) + 0.1 * rng.standard_normal((R_, R_)), -0.2 * np.eye(R_)])
    G = rng.standard_normal((R_, R_))
    Q = G @ G.T + 0.3 * np.eye(R_)
    k = R_ * max(P_, q + 1 if q else P_)
    H = rng.standard_normal((k, k))
    P0 = H @ H.T / k + 0.2 * np.eye(k)
    mu0 = rng.standard_normal(k)
    rho = np.stack([rng.uniform(-0.5, 0.6, N), rng.uniform(-0.3, 0.3, N)], axis=1)[:, :q] if q else None
    v0 = rng.uniform(0.5, 2.0, N)
    return Lam, R, rho, A, Q, mu0, P0, v0


def _moment_check(draws, S, mean):
    """Sample mean and covariance of `draws` [D, dim] against (mean, S): elementwise, 5 standard errors of the Gaussian sample
    moments -- sqrt(s_ii / D) for the mean, sqrt((s_ii s_jj + s_ij^2) / D) for the covariance about the known mean."""
    Dn = draws.shape[0]
    dev = draws - mean
    sd = np.sqrt(np.diag(S))
    assert np.all(np.abs(dev.mean(axis=0)) <= 5.0 * sd / np.sqrt(Dn))
    C = dev.T @ dev / Dn
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / Dn)
    worst = np.max(np.abs(C - S) / se)
    assert worst <= 5.0, worst
    return worst


def _companion_mean(A, mu0, steps, r):
    out, z = [], mu0.copy()
    for _ in range(steps):
        f = A @ z[:A.shape[1]]
        z = np.concatenate([f, z[:-r]])
        out.append(f)
    return np.array(out)


def test_plain_contract_has_the_models_moments():
    Lam, R, _, A, Q, mu0, P0, _ = _model(0)
    draws = np.stack([sx.simulate(Lam, R, A, Q, mu0, P0, T, SEED, 0, d, 0)[0].ravel() for d in range(D)])
    mean = (_companion_mean(A, mu0, T, R_) @ Lam.T).ravel()
    _moment_check(draws, sx.implied_cov(Lam, R, A, Q, P0, T), mean)


def test_ar_contract_has_the_models_moments():
    Lam, sig2, rho, A, Q, mu0, P0, v0 = _model(Q_)
    m = max(P_, Q_ + 1)
    draws = np.stack([sx.simulate_ar(Lam, sig2, rho, A, Q, mu0, P0, T, SEED, 0, d, 0, v0=v0)[0].ravel() for d in range(D)])
    lags = mu0.reshape(m, R_)                                            # f_{q-1} .. f_{q-m}
    fmean = np.vstack([lags[Q_ - 1 - t] for t in range(Q_)] + [_companion_mean(A, mu0, T - Q_, R_)])
    _moment_check(draws, sx.implied_cov_ar(Lam, sig2, rho, A, Q, P0, v0, T), (fmean @ Lam.T).ravel())


def test_a_wrong_contract_fails_the_moment_check():
    """The check has teeth: the same draws against a model whose idiosyncratic s.d. went in as a variance."""
    Lam, R, _, A, Q, mu0, P0, _ = _model(0)
    draws = np.stack([sx.simulate(Lam, R * R, A, Q, mu0, P0, T, SEED, 0, d, 0)[0].ravel() for d in range(D)])
    mean = (_companion_mean(A, mu0, T, R_) @ Lam.T).ravel()
    with pytest.raises(AssertionError):
        _moment_check(draws, sx.implied_cov(Lam, R, A, Q, P0, T), mean)


def test_contract_mask_rows_and_invariants():
    Lam, sig2, rho, A, Q, mu0, P0, v0 = _model(Q_)
    rng = np.random.default_rng(5)
    panel = rng.standard_normal((T, N))
    panel[3, 1] = panel[0, 2] = panel[1, 4] = np.nan
    free, _ = sx.simulate_ar(Lam, sig2, rho, A, Q, mu0, P0, T, 7, 0, 3, 1, v0=v0)
    x, f = sx.simulate_ar(Lam, sig2, rho, A, Q, mu0, P0, T, 7, 0, 3, 1, panel=panel, v0=v0)
    assert np.array_equal(x[:Q_], panel[:Q_], equal_nan=True)           # rows < q are the panel's, bit for bit
    assert np.array_equal(np.isnan(x), np.isnan(panel)) and f.shape == (T - Q_, R_)
    # the missing pre-sample cell of series 2 (row 0) and of series 4 (row 1) draws what the free run draws there
    x2, _ = sx.simulate_ar(Lam, sig2, rho, A, Q, mu0, P0, T, 7, 3, 0, 1, panel=panel, v0=v0)
    assert np.array_equal(x, x2, equal_nan=True)                        # draw d of first_draw k = draw 0 of first_draw k + d
    Lp, Rp, _, Ap, Qp, m0, P0p, _ = _model(0)
    mask = np.where(rng.uniform(size=(T, N)) < 0.3, np.nan, 0.0)
    a, fa = sx.simulate(Lp, Rp, Ap, Qp, m0, P0p, T, 7, 0, 2, 0, mask=mask)
    b, fb = sx.simulate(Lp, Rp, Ap, Qp, m0, P0p, T, 7, 0, 2, 0)
    assert np.array_equal(np.isnan(a), np.isnan(mask)) and np.array_equal(a[~np.isnan(mask)], b[~np.isnan(mask)])
    assert np.array_equal(fa, fb) and not np.isnan(free).any()


# ------------------------------------------------------------------------------------------------------------------ (b)
def _src(name):
    return open(os.path.join(ROOT, "dynamic_factor_models_amd", "csrc", name)).read()


def test_restated_constants_and_launch_lines_match_the_source():
    sim, capi, fcar = _src("simulate.hip"), _src("capi.hip"), _src("dfm_fcar.h")
    assert f"constexpr int kSimMaxThreads = {sx.SIM_MAX_THREADS};" in sim
    assert "constexpr size_t kSimLds = 32 * 1024;" in sim and sx.SIM_LDS == 32 * 1024
    assert "constexpr size_t kSimArLds = 48 * 1024;" in sim and sx.SIMAR_LDS == 48 * 1024
    assert f"constexpr int kSsArLdsTail = {sx.SSAR_TAIL};" in fcar
    assert f"static constexpr int kSsSlice = {sx.SLICE};" in capi
    assert "a.geo = cell_geometry((a.N + 1) / 2, a.r, a.T, kSimMaxThreads, kSimLds);" in sim
    assert "const dim3 grid((unsigned)a.S, (unsigned)a.geo.nchunk, (unsigned)a.geo.nsblk);" in sim
    assert "a.geo = series_geometry(a.N, a.r, a.n, kSimArLds - tail);" in sim
    assert "const size_t blocks = (size_t)a.S * a.geo.nsblk" in sim
    assert "const bool vec = cell_vec(a.N, a.panel, a.x_draw);" in sim


def test_plain_geometry_matches_the_host_function(tmp_path):
    exe = pg.build_cellgeom_host(tmp_path)
    geos = [sx.plain_launch(1, 1, n, r, rows) for n, r, rows in
            itertools.product((1, 2, 7, 8, 139, 200, 513, 514, 1025), pg.SWEEP_R, pg.SWEEP_ROWS + (222, 500))]
    calls = sorted({g["call"] for g in geos})
    host = dict(zip(calls, pg.ask_cellgeom_host(exe, [("cell",) + c for c in calls])))
    bad = [(g["call"], host[g["call"]]) for g in geos if tuple(g[f] for f in pg.GEOM_FIELDS) != host[g["call"]]]
    assert not bad, bad[:5]
    assert any(g["cap_binds"] for g in geos) and any(g["partial_last"] for g in geos) and {1, 2, 3} <= {g["nsblk"] for g in geos}
    g = sx.plain_launch(1, 3, 514, 8, 40)                               # 257 pairs in two blocks of 129: the last lane idles
    assert (g["nsblk"], g["NPB"], g["idle_last"], g["vec"], g["grid"][0]) == (2, 129, True, True, 3)
    g = sx.plain_launch(1, 1, 2, 32, 400)                               # one lane, 64 row groups: the LDS cap (128 rows) binds
    assert (g["NPB"], g["G"], g["cap"], g["RC"], g["cap_binds"]) == (1, 64, 128, 128, True)
    assert sx.plain_launch(3, 4000, 8, 4, 10)["grid"][0] == sx.SLICE


def test_ar_geometry_matches_the_host_function(tmp_path):
    exe = str(tmp_path / "seriesgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "seriesgeom_host.cpp")], check=True)
    geos = [sx.ar_launch(1, 1, n, r, q, rows + q) for n, r, q, rows in
            itertools.product((1, 2, 3, 256, 257, 514, 1000), (1, 4, 5, 8, 9, 16), (1, 2, 3, 4), (1, 31, 32, 33, 70))]
    text = "".join(" ".join(map(str, g["call"])) + "\n" for g in geos)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(geos)
    for g, line in zip(geos, out):
        assert tuple(map(int, line.split())) == tuple(g[f] for f in pg.GEOM_FIELDS), g["call"]
    assert sx.ar_launch(1, 1, 257, 4, 1, 40)["paired"] == (True, False)  # 2 blocks of 129: the second starts at an odd series
    assert sx.ar_launch(1, 1, 514, 4, 1, 40)["paired"] == (True, True, True)
    assert sx.ar_launch(2, 3, 257, 4, 2, 40)["grid"][0] == 12


# ------------------------------------------------------------------------------------------------------------------ (c)
class _NoDevice:
    """A context that fails the test if any device work is reached."""
    def __getattr__(self, name):
        raise AssertionError(f"device work reached: ctx.{name}")


def _api_model(nlag=2):
    from dynamic_factor_models_amd import api
    rng = np.random.default_rng(3)
    data = rng.standard_normal((40, 8))
    return api, api.DFMModel(data, np.ones(8, dtype=int), 10, 10, 1, 40, 0, 2, 1e-8, 2, nlag)


def test_estimate_argument_checks_need_no_device():
    api, m = _api_model()
    ctx = _NoDevice()
    with pytest.raises(ValueError, match="draws must be"):
        api.estimate(m, api.Parametric(), factor_lags=2, nrep=4, draws="gpu", ctx=ctx)
    with pytest.raises(ValueError, match="one GPU"):
        api.estimate(m, api.Parametric(), factor_lags=2, nrep=4, ngpu=2, ctx=ctx)
    with pytest.raises(ValueError, match="host generator"):
        api.estimate(m, api.Parametric(), factor_lags=2, nrep=4, draws="host", ctx=ctx)
    with pytest.raises(ValueError, match="one GPU"):
        api.estimate(m, api.Parametric(), factor_lags=1, nrep=4, draws="device", ngpu=2, ctx=ctx)


def test_simulate_and_band_argument_checks_need_no_device():
    api, m = _api_model()
    ctx = _NoDevice()
    with pytest.raises(ValueError, match="ndraws"):
        api.simulate(m, 0, ctx=ctx)
    with pytest.raises(ValueError, match="not been estimated"):
        api.simulate(m, 3, ctx=ctx)
    with pytest.raises(ValueError, match="ndraws"):
        api.simulate_ar_idio(m, 0, ctx=ctx)
    with pytest.raises(ValueError, match="nrep"):
        api.estimate_ar_idio(m, nrep=-1, ctx=ctx)
    with pytest.raises(ValueError, match="need parameter sets"):
        api.forecast_ar_idio(m, 2, quantiles=(0.1, 0.9), ctx=ctx)
    with pytest.raises(ValueError, match="quantiles= with them"):
        api.forecast_ar_idio(m, 2, params={}, ctx=ctx)
    with pytest.raises(ValueError, match="H >= 1"):
        api.forecast_ar_idio(m, 0, params={}, quantiles=(0.5,), ctx=ctx)
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        api.forecast_ar_idio(m, 2, params={}, quantiles=(0.0,), ctx=ctx)
    m.n_uarlag = 5
    with pytest.raises(ValueError, match="n_uarlag"):
        api.simulate_ar_idio(m, 3, ctx=ctx)
    with pytest.raises(ValueError, match="n_uarlag"):
        api.estimate_ar_idio(m, nrep=2, ctx=ctx)
