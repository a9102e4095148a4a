"""CPU: the mixed-frequency EM with fixed loadings (tests/mf_blocks_expect.py, what tests/test_gpu_mf_blocks.py compares the library
with).  The model is pinned to tests/mf_expect.py where no loading is fixed, its series step is shown to be a stationary point of
the expected complete-data log-likelihood in the free coordinates, the keep rules are checked at their boundary, and the C
interface's three statements (header, ctypes table, Julia ccall) are held against each other."""
import ctypes
import os

import numpy as np
import pytest

from dynamic_factor_models_amd.api import mf_blocks
from tests import mf_blocks_expect as mb
from tests import mf_expect as me
from tests.test_julia_shim_cpu import C2J, RET2J, header_prototypes, julia_ccalls
from tests.test_mf_cpu import _expected_loglik

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = mb.KEYS
SHAPES = [(9, 4, 48, 3, 1), (12, 5, 60, 5, 2), (20, 6, 72, 8, 1), (7, 0, 36, 2, 4)]       # (Nm, Nq, T, r, p)


def _one(Nm, Nq, T, r, p, **kw):
    """Replicate 0 of a case: (x [T,N], W, free, start, marks)."""
    x, W, free, st, mark = mb.build_case(1, Nm, Nq, T, r, p, **kw)
    return x[0], W, free, {k: st[k][0] for k in KEYS}, mark


def test_all_free_mask_is_the_unrestricted_step():
    x, W, st = me.synth_mf(1, 12, 5, 60, 3, 2, "q_flow", missing=0.05, ragged=2)
    a, la, _ = me.em_step_mf(x, W=W, **st)
    b, lb, _ = mb.em_step_mf_blocks(x, W=W, free=np.ones((17, 3), np.uint8), **st)
    assert la == lb
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("Nm,Nq,T,r,p", SHAPES[:2])
def test_free_coordinates_are_a_stationary_point(Nm, Nq, T, r, p):
    """The bound of test_mf_cpu.test_every_m_step_block_is_a_stationary_point: central differences with step h of the expected
    log-likelihood, which is quadratic in lam_i (no truncation), so the tolerance is the rounding of the quotient, 8 eps times the
    sum of the magnitudes of its terms over h.  The gradient vanishes to that in every FREE coordinate of the update, is far from it
    at the start, and does not vanish in the fixed coordinates (the restriction binds)."""
    x, W, free, st, mark = _one(Nm, Nq, T, r, p, missing=0.05)
    new, _, out = mb.em_step_mf_blocks(x, W=W, free=free, **st)
    h = 1e-5
    _, mag, _, _ = _expected_loglik(x, W, out, new["Lam"], new["R"], new["Avar"], new["Q"], pieces=True)
    tol = 8.0 * np.finfo(float).eps * mag / h

    def grad(params, idx):
        vals = []
        for s in (+1.0, -1.0):
            q = {k: params[k].copy() for k in ("Lam", "R", "Avar", "Q")}
            q["Lam"][idx] += s * h
            vals.append(_expected_loglik(x, W, out, **q))
        return (vals[0] - vals[1]) / (2.0 * h)

    series = [i for i in range(x.shape[1]) if i not in (mark["at"], mark["fixed_row"])]
    g_free = [abs(grad(new, (i, c))) for i in series for c in range(r) if free[i, c]]
    g_old = max(abs(grad(st, (i, c))) for i in series for c in range(r) if free[i, c])
    g_fixed = max(abs(grad(new, (i, c))) for i in series for c in range(r) if not free[i, c])
    print(f"|gradient| free {max(g_free):.2e} (tolerance {tol:.2e}), at the start {g_old:.2e}, fixed coordinates {g_fixed:.2e}")
    assert max(g_free) <= tol
    assert g_old > 100.0 * tol and g_fixed > 100.0 * tol


@pytest.mark.parametrize("Nm,Nq,T,r,p", SHAPES)
def test_free_gradient_of_the_normal_equations_vanishes(Nm, Nq, T, r, p):
    """(b - G lam)_F at the update.  A backward-stable solve leaves a residual of a few eps per term of the sums times the size of
    the terms, |b| + |G||lam| (no condition number): 64 r eps of it."""
    x, W, free, st, mark = _one(Nm, Nq, T, r, p, missing=0.05 if Nq else 0.0)
    new, _, out = mb.em_step_mf_blocks(x, W=W, free=free, **st)
    for i, (n, G, b, _) in enumerate(mb.series_moments(x, W, out, r, W.shape[1])):
        if n < free[i].sum() + 1 or not free[i].any():
            continue
        lam = new["Lam"][i]
        resid = (b - G @ lam)[free[i]]
        scale = (np.abs(b) + np.abs(G) @ np.abs(lam))[free[i]]
        assert np.all(np.abs(resid) <= 64 * r * np.finfo(float).eps * scale), i


@pytest.mark.parametrize("Nm,Nq,T,r,p", SHAPES)
def test_fixed_entries_stay_and_the_path_does_not_decrease(Nm, Nq, T, r, p):
    x, W, free, st, mark = _one(Nm, Nq, T, r, p, missing=0.05 if Nq else 0.0)
    assert st["Lam"][mark["one"]] == 1.0 and not free[mark["one"]] and not free[mark["fixed_row"]].any()
    est, path, _ = mb.em_mf_blocks(x, st, W, free, max_iter=12)
    assert np.array_equal(est["Lam"][~free], st["Lam"][~free])
    assert est["Lam"][mark["one"]] == 1.0 and np.array_equal(est["Lam"][mark["fixed_row"]], np.zeros(r))
    assert not np.array_equal(est["Lam"][free], st["Lam"][free])
    print("relative steps", np.diff(path) / np.abs(path[:-1]))
    assert len(path) == 12 and np.all(np.diff(path) >= 0.0), np.diff(path)


@pytest.mark.parametrize("Nm,Nq,T,r,p", SHAPES)
def test_path_does_not_decrease_under_a_block_structure(Nm, Nq, T, r, p):
    """The mask api.mf_blocks builds: a global block and two halves of the series sharing the remaining factors."""
    x, W, st = me.synth_mf(0, Nm, Nq, T, r, p, "q_flow", missing=0.05 if Nq else 0.0)
    i = np.arange(Nm + Nq)
    h = max(1, r // 3)
    mem = np.stack([np.ones(Nm + Nq, bool), i % 2 == 0, i % 2 == 1], axis=1)
    free = mf_blocks(mem, [r - 2 * h, h, h]) if r >= 3 else mf_blocks(mem[:, :2], [1, 1])
    assert free.shape == (Nm + Nq, r)
    st = dict(st, Lam=np.where(free, st["Lam"], 0.0))
    est, path, _ = mb.em_mf_blocks(x, st, W, free, max_iter=12)
    assert np.all(est["Lam"][~free] == 0.0) and np.all(np.diff(path) >= 0.0), np.diff(path)


@pytest.mark.parametrize("Nm,Nq,T,r,p", SHAPES[:3])
def test_keep_rule_at_its_boundary(Nm, Nq, T, r, p):
    x, W, free, st, mark = _one(Nm, Nq, T, r, p)
    at, above = mark["at"], mark["above"]
    n = (~np.isnan(x)).sum(0)
    k = free.sum(1)
    assert n[at] == k[at] and n[above] == k[above] + 1 and k[above] < r and n[above] < r + 1
    new, _, _ = mb.em_step_mf_blocks(x, W=W, free=free, **st)
    assert np.array_equal(new["Lam"][at], st["Lam"][at]) and new["R"][at] == st["R"][at]
    assert not np.any(new["Lam"][above][free[above]] == st["Lam"][above][free[above]]) and new["R"][above] != st["R"][above]
    assert np.array_equal(new["Lam"][above][~free[above]], st["Lam"][above][~free[above]])
    old, _, _ = me.em_step_mf(x, W=W, **st)                     # the unrestricted rule, n_i < r + 1, keeps both
    assert np.array_equal(old["Lam"][above], st["Lam"][above]) and old["R"][above] == st["R"][above]


def test_series_without_a_free_loading_updates_its_variance_only():
    x, W, free, st, mark = _one(12, 5, 60, 3, 2)
    i = mark["fixed_row"]
    new, _, out = mb.em_step_mf_blocks(x, W=W, free=free, **st)
    assert np.array_equal(new["Lam"][i], st["Lam"][i]) and new["R"][i] != st["R"][i]
    n, G, b, sxx = mb.series_moments(x, W, out, 3, W.shape[1])[i]
    assert new["R"][i] == (sxx - 2.0 * st["Lam"][i] @ b + st["Lam"][i] @ G @ st["Lam"][i]) / n
    x2 = x.copy(); x2[:, i] = np.nan                             # n_i = 0: nothing to update it from
    new2, _, _ = mb.em_step_mf_blocks(x2, W=W, free=free, **st)
    assert new2["R"][i] == st["R"][i]


def test_a_loading_fixed_at_one_enters_the_right_hand_side():
    """lam_F = G_FF^-1 (b_F - G_FX lam_X): with lam_X = 1 the update differs from the one with lam_X = 0 by G_FF^-1 G_FX."""
    x, W, free, st, mark = _one(9, 4, 48, 3, 1)
    i = mark["one"][0]
    new1, _, out = mb.em_step_mf_blocks(x, W=W, free=free, **st)
    n, G, b, _ = mb.series_moments(x, W, out, 3, W.shape[1])[i]
    F, X = np.nonzero(free[i])[0], np.nonzero(~free[i])[0]
    want = np.linalg.solve(G[np.ix_(F, F)], b[F] - G[np.ix_(F, X)] @ st["Lam"][i, X])
    np.testing.assert_allclose(new1["Lam"][i, F], want, rtol=1e-12)
    assert np.abs(want - np.linalg.solve(G[np.ix_(F, F)], b[F])).max() > 1e-3


# ---- the C interface, stated three times -------------------------------------------------------------------------------------
BLOCK_SYMBOLS = ("dfm_em_mf_blocks_batch_dev", "dfm_em_mf_blocks_batch")


def test_header_ctypes_table_and_julia_ccalls_agree():
    from dynamic_factor_models_amd import _lib
    protos = header_prototypes()
    c2ct = {"dfm_handle*": ctypes.c_void_p, "double*": ctypes.c_void_p, "int*": ctypes.c_void_p, "void*": ctypes.c_void_p,
            "int": ctypes.c_int, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for name in BLOCK_SYMBOLS:
        assert name in protos, name
        cret, cargs = protos[name]
        assert cret == "int"
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == len(cargs), (name, len(args), len(cargs))
        for k, (a, ca) in enumerate(zip(args, cargs)):
            assert a is c2ct[ca], (name, k, ca)
    cargs = protos["dfm_em_mf_blocks_batch"][1]
    assert cargs == protos["dfm_em_mf_blocks_batch_dev"][1]
    plain = protos["dfm_em_mf_batch"][1]                        # the mask sits behind W; everything else is dfm_em_mf_batch
    assert len(cargs) == 23 and cargs[11] == "void*" and cargs[:11] + cargs[12:] == plain
    calls = {n: (ret, jargs) for n, ret, jargs in julia_ccalls()}
    for name in BLOCK_SYMBOLS:
        assert name in calls, f"julia/dfm_hip.jl does not bind {name}"
        ret, jargs = calls[name]
        cret, cargs = protos[name]
        assert RET2J[cret] == ret and len(jargs) == len(cargs)
        for k, (ja, ca) in enumerate(zip(jargs, cargs)):
            assert ja in C2J[ca], (name, k, ja, ca)
    src = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    doc = src[src.index("BLOCK-STRUCTURED"):src.index("int dfm_em_mf_blocks_batch_dev")]
    for words in ("G_FF^-1 (b_F - G_FX lam_X)", "n_i < k_i + 1", "k_i = 0", "free_mask == NULL is dfm_em_mf_batch"):
        assert words in doc, words


def test_the_source_list_builds_the_new_kernel():
    from dynamic_factor_models_amd import build
    assert "mstep_mf_blocks.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mstep_mf_blocks.hip"))


def test_python_binding_marshals_the_mask():
    """The host wrapper through a recorder in place of the library: the symbol, the mask as N x r bytes behind W, null for None."""
    from dynamic_factor_models_amd import _lib, kalman
    from tests.api_calls import Recorder

    x, W, free, st, _ = mb.build_case(2, 9, 4, 36, 2, 1)
    ctx = kalman.DfmContext.__new__(kalman.DfmContext)
    ctx._lib, ctx._h = Recorder(), ctypes.c_void_p(1)
    seen = {}
    for mask in (free.astype(float) * 3.0, None):
        est, path, iters, f, P = ctx.em_mf_blocks_batch_host(x, st["Lam"], st["R"], W, mask, st["Avar"], st["Q"], st["mu0"], st["P0"],
                                                             max_iter=3)
        name, args = ctx._lib.calls.pop()
        assert name == "dfm_em_mf_blocks_batch" and len(args) == len(_lib.SYMBOLS[name][1])
        assert args[1:7] == (2, 36, 13, 2, 1, W.shape[1])
        assert set(est) == set(KEYS) and path.shape == (2, 3) and est["Lam"] is not st["Lam"]
        seen[mask is None] = args[11]
    assert seen[True] is None
    got = np.ctypeslib.as_array(ctypes.cast(seen[False], ctypes.POINTER(ctypes.c_ubyte)), shape=free.shape)
    assert np.array_equal(got, free.astype(np.uint8))
    ctx._h = None


def test_api_blocks_without_a_device():
    from dynamic_factor_models_amd import api
    mem = np.zeros((6, 3), bool)
    mem[:, 0] = True; mem[:3, 1] = True; mem[3:, 2] = True
    free = api.mf_blocks(mem, [2, 1, 1])
    assert free.shape == (6, 4) and free.dtype == bool
    assert np.array_equal(free, mb.blocks_free(mem, [2, 1, 1]))
    assert np.array_equal(free[:, 0], free[:, 1]) and free[:, :2].all() and np.array_equal(free[:, 2], mem[:, 1])
    assert [(a, b) for a, b, _ in api._mf_block_runs(free)] == [(0, 2), (2, 3), (3, 4)]
    for bad in ((mem, [2, 1]), (mem[0], [1]), (mem, [1, 0, 1]), (mem, [1.5, 1, 1])):
        with pytest.raises(ValueError):
            api.mf_blocks(*bad)
    lonely = mem.copy(); lonely[2] = False
    with pytest.raises(ValueError, match="no block"):
        api.mf_blocks(lonely, [1, 1, 1])
    empty = mem.copy(); empty[:, 2] = False
    with pytest.raises(ValueError, match="no series"):
        api.mf_blocks(empty, [1, 1, 1])
    # blocks= is validated before a device is asked for
    x = np.random.default_rng(0).standard_normal((24, 6))
    assert np.array_equal(api._mf_free((mem, [2, 1, 1]), 6, 4), free) and np.array_equal(api._mf_free(free.astype(int), 6, 4), free)
    for blocks, r in (((mem, [2, 1, 1]), 3), (free[:5], 4), (free[0], 4)):
        with pytest.raises(ValueError):
            api.estimate_mixed_frequency(x, ["m"] * 6, r, 1, blocks=blocks, ctx=object())
    assert "blocks=None" in api.estimate_mixed_frequency.__doc__ or "blocks (None" in api.estimate_mixed_frequency.__doc__
    assert 'all weights "m"' in api.estimate_mixed_frequency.__doc__


def test_block_start_of_the_api_is_the_model_start():
    """api._mf_blocks_start with the oracle's PCA in place of the device's is mf_blocks_expect.mf_blocks_start; a block without a
    fully observed monthly series is refused."""
    from dynamic_factor_models_amd import api
    from oracle import kalman_oracle as ko

    class Pca:
        def pca_init_batch_host(self, panel, r):
            return None, ko.pca_init(panel[0], r)[1][None]

    x, W, _ = me.synth_mf(3, 18, 6, 72, 3, 2, "q_flow")
    mem = np.zeros((24, 3), bool)
    mem[:, 0] = True; mem[np.arange(24) % 2 == 0, 1] = True; mem[np.arange(24) % 2 == 1, 2] = True
    free = api.mf_blocks(mem, [1, 1, 1])
    a = api._mf_blocks_start(Pca(), x, W, free, 2)
    b = mb.mf_blocks_start(x, W, free, 2)
    for k in KEYS:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=1e-13, err_msg=k)
    assert np.all(a["Lam"][~free] == 0.0) and np.all(a["Lam"][free] != 0.0)
    x2 = x.copy(); x2[5, (np.arange(24) % 2 == 1) & (np.arange(24) < 18)] = np.nan      # block 2's monthly series all have a hole
    with pytest.raises(ValueError, match="no fully observed monthly series"):
        api._mf_blocks_start(Pca(), x2, W, free, 2)
