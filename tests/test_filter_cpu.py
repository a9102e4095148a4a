"""CPU tests of the filter family (include/dfm_hip.h dfm_filter_batch): the expectation model of tests/filter_expect.py against the
oracles, the collapsed update of csrc/dfm_filter.h restated in NumPy against the textbook update, the launch classes the GPU case
table reaches, and the argument checks, signatures and Julia names that need no device."""
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import filter_expect as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(r, p, N=12, T=30, missing=0.1):
    x, st = fe.params_for(1, N, T, r, p, missing=missing)
    return x[0], [st[k][0] for k in fe.KEYS]


def _smooth(x, P, p):
    if p == 1:
        return ko.kfs_pass_textbook(x, *P)
    return vo.kfs_pass_varp(x, *P, p)


@pytest.mark.parametrize("r,p", [(3, 1), (2, 3)])
def test_model_against_the_smoother_oracles(r, p):
    x, P = _one(r, p)
    zp, Pp, zf, Pf, ll = fe.textbook_filter(x, *P)
    o = _smooth(x, P, p)
    assert abs(ll.sum() - o["loglik"]) <= 1e-9 * max(1.0, abs(o["loglik"]))
    k = o["f_smooth"].shape[1]
    assert np.abs(zf[-1][:k] - o["f_smooth"][-1]).max() <= 1e-10
    assert np.abs(Pf[-1][:k, :k] - o["P_smooth"][-1]).max() <= 1e-10
    for t in (0, 7, 18):                                # filtered at t = smoothed terminal moments of the panel cut to t + 1 rows
        c = _smooth(x[:t + 1], P, p)
        assert np.abs(zf[t][:k] - c["f_smooth"][-1]).max() <= 1e-10
        assert np.abs(Pf[t][:k, :k] - c["P_smooth"][-1]).max() <= 1e-10


def test_model_against_the_joint_gaussian():
    g = np.random.default_rng(5)
    T, N, r, p = 4, 3, 1, 2
    Lam = g.standard_normal((N, r)); R = g.uniform(0.5, 1.5, N)
    A = np.array([[0.5, 0.3]]); Q = np.array([[0.7]])
    mu0 = g.standard_normal(2); L = g.standard_normal((2, 2)); P0 = L @ L.T + 0.5 * np.eye(2)
    x = g.standard_normal((T, N))
    x[1, 0] = np.nan; x[2, 2] = np.nan
    M, Qc = fe.companion(A, Q)
    Z = np.zeros((N, 2)); Z[:, :r] = Lam
    zp, Pp, zf, Pf, ll = fe.textbook_filter(x, Lam, R, A, Q, mu0, P0)
    for t in range(T):
        bf = ko.brute_force_gaussian(x[:t + 1], Z, R, M, Qc, mu0, P0)
        assert np.abs(zf[t] - bf["f_smooth"][-1]).max() <= 1e-12
        assert np.abs(Pf[t] - bf["P_smooth"][-1]).max() <= 1e-12
        if t == 0:
            ez, eP = M @ mu0, M @ P0 @ M.T + Qc
        else:                                           # an appended all-missing row: its smoothed moments are the predicted ones
            bp = ko.brute_force_gaussian(np.vstack([x[:t], np.full((1, N), np.nan)]), Z, R, M, Qc, mu0, P0)
            ez, eP = bp["f_smooth"][-1], bp["P_smooth"][-1]
        assert np.abs(zp[t] - ez).max() <= 1e-12 and np.abs(Pp[t] - eP).max() <= 1e-12
    assert abs(ll.sum() - ko.brute_force_gaussian(x, Z, R, M, Qc, mu0, P0)["loglik"]) <= 1e-11


@pytest.mark.parametrize("kind", ["full", "c_zero", "rank_deficient", "companion"])
def test_collapsed_update_equals_the_textbook_update(kind):
    g = np.random.default_rng(11)
    r, p, N = (3, 2, 9) if kind == "companion" else (4, 1, 9)
    k = r * p
    Lam = g.standard_normal((N, r)); R = g.uniform(0.5, 2.0, N); x = g.standard_normal(N)
    if kind == "c_zero":
        Lam[:] = 0.0
    L = g.standard_normal((k, k))
    if kind == "rank_deficient":
        L[:, 2:] = 0.0                                  # P_pred of rank 2: P11 has two zero pivots
    Pp = L @ L.T
    zp = g.standard_normal(k)
    b, s, n, ld, C = ko.collapse(x[None], Lam, R)
    z, P, ll = fe.collapsed_update(zp, Pp, r, b[0], C[0], float(s[0]), int(n[0]), float(ld[0]))
    Z = np.zeros((N, k)); Z[:, :r] = Lam
    F = Z @ Pp @ Z.T + np.diag(R)
    v = x - Z @ zp
    K = np.linalg.solve(F, Z @ Pp).T
    ez, eP = zp + K @ v, Pp - K @ Z @ Pp
    ell = -0.5 * (N * fe.LOG2PI + np.linalg.slogdet(F)[1] + v @ np.linalg.solve(F, v))
    assert np.abs(z - ez).max() <= 1e-12 * max(1.0, np.abs(ez).max())
    assert np.abs(P - eP).max() <= 1e-12 * max(1.0, np.abs(eP).max())
    assert abs(ll - ell) <= 1e-12 * max(1.0, abs(ell))


def test_fill_sp_rule_matches_cell_sp(tmp_path):
    """fill_launch's SP against cell_sp of csrc/dfm_cellgeom.h, compiled for the host, at the fill's register bucket."""
    exe = fe.pg.build_cellgeom_host(tmp_path)
    seen = fe.pg.check_sp_rule(exe, lambda N, r, al: fe.fill_launch(1, N, r, 20, aligned=al)["SP"], bucket=fe.pg.rb_bucket)
    assert seen == {1, 2}


def test_gpu_case_table_reaches_every_launch_class():
    assert fe.missing_classes() == set()
    names = [c[0] for c in fe.CASES]
    assert len(set(names)) == len(names)
    for row in fe.CASES:                                # the entry's limits: k <= 32, N within the collapse's register tiling
        c = fe.case_dict(row)
        assert c["r"] * c["p"] <= 32 and c["N"] <= (1024 if c["r"] <= 8 else 512 if c["r"] <= 16 else 256)
        assert 0 <= c["t0"] < c["T"]


def _model():
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 1)
    return api, m


def test_api_argument_errors_come_before_any_device(monkeypatch):
    api, m = _model()
    monkeypatch.setattr(api, "_own", lambda ctx: pytest.fail("a context was asked for"))
    with pytest.raises(ValueError, match="not been estimated"):
        api.filter_states(m)
    m.em_params = dict(Lam=np.zeros((3, 4)))
    for H in (0, -1):
        with pytest.raises(ValueError, match="H must be"):
            api.evaluate_forecasts(m, H)
    for fo in (2, 217, 0):
        with pytest.raises(ValueError, match="first_origin"):
            api.evaluate_forecasts(m, 4, first_origin=fo)
    for th in (215, m.T + 1):
        with pytest.raises(ValueError, match="through"):
            api.evaluate_forecasts(m, 4, through=th)
        with pytest.raises(ValueError, match="through"):
            api.filter_states(m, through=th)
    with pytest.raises(ValueError, match="replicates"):
        api.filter_states(m, quantiles=[0.5])
    from dynamic_factor_models_amd import filtering
    with pytest.raises(ValueError):
        filtering.check_args(10, -1, 0)
    with pytest.raises(ValueError):
        filtering.check_args(10, 2, 10)
    filtering.check_args(10, 0, 9)


def test_signatures_and_julia_names():
    from dynamic_factor_models_amd import _lib, filtering, kalman
    for name in ("dfm_filter_batch", "dfm_filter_batch_dev"):
        res, args = _lib.SYMBOLS[name]
        assert len(args) == 1 + 7 + 20 + 1 and args[-1] is _lib.c_uint
    assert kalman.DfmContext.filter_batch_host is filtering.filter_batch_host
    assert kalman.DfmContext.filter_batch_dev is filtering.filter_batch_dev
    jl = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    assert ":dfm_filter_batch" in jl and "function filter_states" in jl and "function evaluate_forecasts" in jl
    hdr = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    assert "dfm_filter_batch_dev(" in hdr and "dfm_filter_batch(" in hdr
