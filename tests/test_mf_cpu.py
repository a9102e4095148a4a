"""CPU: the mixed-frequency model itself (tests/mf_expect.py, what tests/test_gpu_mf.py compares the library with).  The reference has
no Kalman code to pin it to, so it is pinned here: the pass of the expanded model to brute-force Gaussian conditioning, the L = 1
case to the VAR(p) oracle, every block of the M-step as a stationary point of the expected complete-data log-likelihood, the
likelihood path, and the three statements of the C interface (header, ctypes table, Julia ccall) to each other."""
import ctypes
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import mf_expect as me
from tests.test_julia_shim_cpu import C2J, RET2J, header_prototypes, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
MF_SYMBOLS = ("dfm_ks_pass_mf_batch_dev", "dfm_ks_pass_mf_batch", "dfm_em_mf_batch_dev", "dfm_em_mf_batch")


@pytest.mark.parametrize("Nm,Nq,T,r,p,kind", [(4, 2, 12, 1, 1, "q_flow"), (3, 2, 12, 2, 1, "q_avg"), (4, 3, 9, 1, 2, "q_avg"),
                                              (3, 3, 12, 1, 3, "q_flow")])
def test_pass_of_the_expanded_model_is_gaussian_conditioning(Nm, Nq, T, r, p, kind):
    x, W, st = me.synth_mf(0, Nm, Nq, T, r, p, kind, missing=0.1, ragged=2)
    out = me.kfs_pass_mf(x, W=W, **st)
    LamK, M, Qk, m = me.expanded(st["Lam"], W, st["Avar"], st["Q"])
    bf = ko.brute_force_gaussian(x, LamK, st["R"], M, Qk, st["mu0"], st["P0"])
    for k in ("f_smooth", "P_smooth", "P_lag", "f0_smooth", "P0_smooth"):
        assert np.abs(out[k] - bf[k]).max() <= 1e-10 * max(1.0, np.abs(bf[k]).max()), k
    assert abs(out["loglik"] - bf["loglik"]) <= 1e-10 * max(1.0, abs(bf["loglik"]))
    # the loadings really are the aggregation: x_it loads on sum_l w_il f_{t-l}
    z = np.random.default_rng(0).standard_normal(r * m)
    g = sum(W[:, l:l + 1] * z[l * r:(l + 1) * r][None, :] for l in range(W.shape[1]))
    np.testing.assert_allclose(LamK @ z, np.einsum("ic,ic->i", st["Lam"], g), rtol=1e-13)


@pytest.mark.parametrize("p,missing", [(1, 0.0), (2, 0.07), (3, 0.05)])
def test_one_lag_and_unit_weights_is_the_varp_step(p, missing):
    N, T, r = 14, 50, 2
    x = vo.synth_varp(3, N, T, r, p, missing=missing)
    st, _ = vo.varp_init(np.where(np.isnan(x), 0.0, x), r, p)
    a, la, _ = vo.em_step_varp(x, p=p, **st)
    b, lb, _ = me.em_step_mf(x, W=np.ones((N, 1)), **st)
    assert abs(la - lb) <= 1e-12 * abs(la)
    for k in KEYS:
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * max(1.0, np.abs(a[k]).max()), k


def _expected_loglik(x, W, out, Lam, R, Avar, Q, pieces=False):
    """E[log p(X, Z) | X] up to constants, from the smoothed moments of the FULL companion state and the expanded loadings (no
    aggregated G_i / b_i: independent of em_step_mf's algebra).  pieces=True: also the sum of the terms' magnitudes, the
    per-series (n_i, quadratic form) and the transition's residual moment D."""
    T, N = x.shape
    r = Lam.shape[1]
    ka = Avar.shape[1]
    m = out["f_smooth"].shape[1] // r
    zs, Ps, Pl, z0, P0s = out["f_smooth"], out["P_smooth"], out["P_lag"], out["f0_smooth"], out["P0_smooth"]
    Ez = zs[:, :, None] * zs[:, None, :] + Ps
    C = me.mf_loadings(Lam, W, m)
    val, mag, ser = 0.0, 0.0, []
    for i in range(N):
        o = ~np.isnan(x[:, i])
        t1, t2, t3 = (x[o, i] ** 2).sum(), 2.0 * x[o, i] @ (zs[o] @ C[i]), np.einsum("k,tkl,l->", C[i], Ez[o], C[i])
        quad = t1 - t2 + t3
        val += -0.5 * (o.sum() * np.log(R[i]) + quad / R[i])
        mag += 0.5 * (o.sum() * abs(np.log(R[i])) + (abs(t1) + abs(t2) + abs(t3)) / R[i])
        ser.append((int(o.sum()), quad))
    S11 = Ez.sum(0)
    S00 = S11 - Ez[-1] + np.outer(z0, z0) + P0s
    zprev = np.vstack([z0[None], zs[:-1]])
    S10 = (zs[:, :, None] * zprev[:, None, :] + Pl).sum(0)
    parts = [S11[:r, :r], Avar @ S10[:r, :ka].T, S10[:r, :ka] @ Avar.T, Avar @ S00[:ka, :ka] @ Avar.T]
    D = parts[0] - parts[1] - parts[2] + parts[3]
    Qi = np.linalg.inv(Q)
    val += -0.5 * (T * np.linalg.slogdet(Q)[1] + np.trace(Qi @ D))
    mag += 0.5 * (T * abs(np.linalg.slogdet(Q)[1]) + sum(np.abs(Qi @ P).sum() for P in parts))
    return (val, mag, ser, D) if pieces else val


@pytest.mark.parametrize("kind,p", [("q_flow", 2), ("q_avg", 1), ("q_avg", 4)])
def test_every_m_step_block_is_a_stationary_point(kind, p):
    """Central differences with step h.  The tolerance is the error of the difference quotient itself: rounding, eps times the
    sum of the magnitudes of F's terms over h (8 eps: two evaluations, a factor 4 for the accumulated sums), plus truncation,
    h^2 / 6 times a bound on the third derivative F3.  F is quadratic in lam_i and A (no truncation).  In R_i it is
    -(n_i log R_i + q_i / R_i) / 2: |F3| <= (n_i + 3 q_i / R_i) / R_i^3.  In Q it is -(T log det Q + tr Q^-1 D) / 2: along a
    direction of norm <= 1, |F3| <= (T r + 3 tr(Q^-1 D)) ||Q^-1||^3.  The gradient must vanish to that at the update, and must be
    far from it at the parameters the iteration started from (else the check shows nothing)."""
    r = 2
    x, W, st = me.synth_mf(1, 12, 5, 60, r, p, kind, missing=0.05, ragged=2)
    T = x.shape[0]
    new, _, out = me.em_step_mf(x, W=W, **st)
    h = 1e-5
    _, mag, ser, D = _expected_loglik(x, W, out, new["Lam"], new["R"], new["Avar"], new["Q"], pieces=True)
    rounding = 8.0 * np.finfo(float).eps * mag / h
    Qi = np.linalg.inv(new["Q"])
    trunc = dict(Lam=lambda idx: 0.0, Avar=lambda idx: 0.0,
                 R=lambda idx: h * h / 6.0 * (ser[idx[0]][0] + 3.0 * ser[idx[0]][1] / new["R"][idx[0]]) / new["R"][idx[0]] ** 3,
                 Q=lambda idx: h * h / 6.0 * (T * r + 3.0 * np.trace(Qi @ D)) * np.linalg.norm(Qi, 2) ** 3)

    def grad(params, name, idx, sym=False):
        vals = []
        for s in (+1.0, -1.0):
            q = {k: params[k].copy() for k in ("Lam", "R", "Avar", "Q")}
            q[name][idx] += s * h
            if sym and idx[0] != idx[1]:
                q[name][idx[::-1]] += s * h
            vals.append(_expected_loglik(x, W, out, **q))
        return (vals[0] - vals[1]) / (2.0 * h)

    for name, idxs, sym in (("Lam", [(i, c) for i in (0, 5, 12, 16) for c in range(r)], False),
                            ("R", [(0,), (7,), (12,), (16,)], False),
                            ("Avar", [(a, b) for a in range(r) for b in range(r * p)], False),
                            ("Q", [(0, 0), (1, 0), (1, 1)], True)):
        g_new = [abs(grad(new, name, i, sym)) for i in idxs]
        tols = [rounding + trunc[name](i) for i in idxs]
        g_old = max(abs(grad(st, name, i, sym)) for i in idxs)
        print(f"{name}: |gradient| at the update {max(g_new):.2e} (tolerance {max(tols):.2e}), at the start {g_old:.2e}")
        for g, t, i in zip(g_new, tols, idxs):
            assert g <= t, (name, i, g, t)
        assert g_old > 100.0 * max(tols), name


@pytest.mark.parametrize("kind", ["q_flow", "q_avg"])
def test_likelihood_path_does_not_decrease(kind):
    x, W, st = me.synth_mf(0, 24, 8, 240, 2, 2, kind, missing=0.03, ragged=3)
    assert np.isnan(x[np.arange(240) % 3 != 2][:, 24:]).all() and not np.isnan(x[2::3, 24:]).any()
    _, path, _ = me.em_mf(x, st, W, max_iter=12)
    assert len(path) == 12 and np.all(np.diff(path) >= 0.0), np.diff(path)


def test_em_mf_tol_bookkeeping_and_thin_series():
    x, W, st = me.synth_mf(2, 10, 4, 90, 2, 1, "q_avg")
    x[4:, 3] = np.nan                                            # 4 cells left... and one with fewer than r + 1
    x[2:, 5] = np.nan
    new, _, _ = me.em_step_mf(x, W=W, **st)
    assert np.array_equal(new["Lam"][5], st["Lam"][5]) and new["R"][5] == st["R"][5]
    assert not np.array_equal(new["Lam"][3], st["Lam"][3])
    _, path, _ = me.em_mf(x, st, W, max_iter=60, tol=1e-4)
    assert 2 <= len(path) < 60


def test_a_series_whose_g_is_not_positive_definite_is_kept():
    """An all-zero weight row makes G_i = 0 exactly (the rule of include/dfm_hip.h: dfm_em_mf_batch): the series keeps lam_i and
    R_i, every other series and the transition step are what they are without the rule -- the zero row loads on nothing, so the
    pass is the pass of the panel without that series -- and tests/mf_blocks_expect.py states the same rule."""
    from tests import mf_blocks_expect as mb
    x, W, st = me.synth_mf(3, 10, 4, 60, 2, 1, "q_avg", missing=0.05)
    z = 4                                                        # a monthly series with every cell it had
    assert (~np.isnan(x[:, z])).sum() >= 3
    W0 = W.copy(); W0[z] = 0.0
    new, ll, _ = me.em_step_mf(x, W=W0, **st)
    assert np.array_equal(new["Lam"][z], st["Lam"][z]) and new["R"][z] == st["R"][z]
    rest = np.arange(W.shape[0]) != z
    sub = dict(st, Lam=st["Lam"][rest], R=st["R"][rest])
    ref, _, _ = me.em_step_mf(x[:, rest], W=W[rest], **sub)
    for k in KEYS:
        got = new[k][rest] if k in ("Lam", "R") else new[k]
        assert np.abs(got - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k
    assert np.all(new["Lam"][rest] != st["Lam"][rest]) and np.isfinite(ll)
    blk, _, _ = mb.em_step_mf_blocks(x, W=W0, free=np.ones_like(st["Lam"], bool), **st)
    for k in KEYS:
        assert np.abs(blk[k] - new[k]).max() <= 1e-12 * max(1.0, np.abs(new[k]).max()), k
    assert np.array_equal(blk["Lam"][z], st["Lam"][z]) and blk["R"][z] == st["R"][z]
    with pytest.raises(np.linalg.LinAlgError):                  # the model's test is the Cholesky attempt: a zero pivot fails it
        np.linalg.cholesky(np.zeros((2, 2)))
    _, path, _ = me.em_mf(x, st, W0, max_iter=4)
    assert np.all(np.diff(path) >= 0.0)


# ---- the C interface, stated three times -------------------------------------------------------------------------------------
def test_header_ctypes_table_and_julia_ccalls_agree():
    from dynamic_factor_models_amd import _lib
    protos = header_prototypes()
    c2ct = {"dfm_handle*": ctypes.c_void_p, "double*": ctypes.c_void_p, "int*": ctypes.c_void_p, "int": ctypes.c_int,
            "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for name in MF_SYMBOLS:
        assert name in protos, name
        cret, cargs = protos[name]
        assert cret == "int"
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == len(cargs), (name, len(args), len(cargs))
        for k, (a, ca) in enumerate(zip(args, cargs)):
            assert a is c2ct[ca], (name, k, ca)
    assert len(protos["dfm_ks_pass_mf_batch"][1]) == 19 and len(protos["dfm_em_mf_batch"][1]) == 22
    assert protos["dfm_em_mf_batch"][1] == protos["dfm_em_mf_batch_dev"][1]
    assert protos["dfm_ks_pass_mf_batch"][1] == protos["dfm_ks_pass_mf_batch_dev"][1]
    calls = {n: (ret, jargs) for n, ret, jargs in julia_ccalls()}
    for name in ("dfm_ks_pass_mf_batch", "dfm_em_mf_batch"):
        assert name in calls, f"julia/dfm_hip.jl does not bind {name}"
        ret, jargs = calls[name]
        cret, cargs = protos[name]
        assert RET2J[cret] == ret and len(jargs) == len(cargs)
        for k, (ja, ca) in enumerate(zip(jargs, cargs)):
            assert ja in C2J[ca], (name, k, ja, ca)
    src = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    body = src[src.index("function estimate_mixed("):]
    body = body[:body.index("\nend\n")]
    assert "mf_weights(" in body and "pca_init(" in body and "em_mf(" in body and "max_em_iter" in body and "tol_em" in body


def test_the_source_list_builds_the_new_kernels():
    from dynamic_factor_models_amd import build
    assert "mstep_mf.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mstep_mf.hip"))


def test_api_helpers_without_a_device():
    from dynamic_factor_models_amd import api
    W = api.mf_weights(["m", "q_flow", "q_avg"], 3)
    np.testing.assert_allclose(W, me.weight_rows(["m", "q_flow", "q_avg"]))
    np.testing.assert_allclose(W[1], np.array([1, 2, 3, 2, 1]) / 3)
    assert api.mf_weights(np.ones((4, 2)), 4).shape == (4, 2)
    with pytest.raises(ValueError):
        api.mf_weights(["m", "weekly"], 2)
    with pytest.raises(ValueError):
        api.mf_weights(["m"], 2)
    rng = np.random.default_rng(1)
    Lam, Avar, Q = rng.standard_normal((3, 2)), rng.standard_normal((2, 4)), np.eye(2)
    LamK, M, Qk = api._mf_expanded(Lam, W, Avar, Q)
    eL, eM, eQ, m = me.expanded(Lam, W, Avar, Q)
    assert m == 5 and np.array_equal(LamK, eL) and np.array_equal(M, eM) and np.array_equal(Qk, eQ)
    fit = dict(Lam=Lam, R=np.ones(3), Avar=Avar, Q=Q, mu0=np.zeros(10), P0=np.eye(10), W=W, mean=np.zeros(3), sd=np.ones(3))
    with pytest.raises(ValueError):
        api.forecast_mixed(fit, np.zeros((5, 3)), -1)
    with pytest.raises(ValueError):
        api.forecast_mixed(fit, np.zeros((5, 4)), 2)
    with pytest.raises(ValueError):
        api.forecast_mixed(fit, np.zeros((5, 3)), 2, quantiles=[0.5])
