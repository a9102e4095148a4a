"""GPU: the mixed-frequency EM with fixed loadings (dfm_em_mf_blocks_batch*: mstep_mf_blocks.hip behind dfm_em_mf_batch's iteration)
against the NumPy model tests/mf_blocks_expect.py, which tests/test_mf_blocks_cpu.py pins.  Tolerances: those of tests/test_gpu_mf.py.

The cases are the smallest that reach every instance r = 1 .. 8 of the solve and its edges.  Every mask (mf_blocks_expect.case_mask)
has column 0 free everywhere, column c >= 1 free on the series with i mod (r - 1) == c - 1 (r = 1: free and fixed alternate), one
all-fixed row, one loading fixed at 1, one series thinned to n_i = k_i observed cells and one to n_i = k_i + 1.
Case i has L = 3 (q_avg), not L = 5: r max(p, L) must stay within DFM_MAX_R = 32, and 8 x 5 = 40 is refused by the pass itself."""
import ctypes
import functools

import numpy as np
import pytest

from tests import mf_blocks_expect as mb
from tests import mf_expect as me

pytestmark = pytest.mark.gpu

KEYS = mb.KEYS

# name: (B, Nm, Nq, T, r, p, kind of the quarterly series, missing, interleave)
CASES = {
    "a": (1, 5, 0, 24, 1, 1, "q_flow", 0.0, False),            # L = 1 (all "m"), r = 1; series 0 fixed at 1
    "b": (2, 9, 4, 36, 2, 1, "q_flow", 0.10, True),            # L = 5, interleaved: two weight classes
    "c": (2, 12, 5, 48, 3, 2, "q_avg", 0.0, False),            # L = 3
    "d": (1, 257, 0, 24, 2, 1, "q_flow", 0.05, False),         # L = 1; the second 256-thread block holds one series
    "e": (3, 17, 3, 36, 4, 4, "q_flow", 0.0, False),
    "f": (2, 20, 6, 48, 5, 1, "q_flow", 0.10, False),
    "g": (2, 20, 6, 48, 6, 2, "q_flow", 0.0, False),
    "h": (2, 20, 6, 60, 7, 1, "q_avg", 0.0, False),
    "i": (2, 20, 6, 72, 8, 1, "q_avg", 0.10, False),           # r = 8 (state 24)
}


@pytest.fixture(scope="module")
def ctx():
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    x, W, free, st, mark = mb.build_case(*CASES[name])
    for a in (x, W, free, *st.values()):
        a.setflags(write=False)
    return x, W, free, st, mark


@functools.lru_cache(maxsize=None)
def model(name, iters):
    """The NumPy model's (parameters, path, last pass) per replicate, computed once."""
    x, W, free, st, _ = case(name)
    return [mb.em_mf_blocks(x[b], {k: st[k][b] for k in KEYS}, W, free, max_iter=iters) for b in range(x.shape[0])]


def _packed(P, r):
    il = np.tril_indices(r)
    return P[:, :r, :r][:, il[0], il[1]]


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _args(x, st, W, free):
    return (x, st["Lam"], st["R"], W, free, st["Avar"], st["Q"], st["mu0"], st["P0"])


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_em_matches_model(ctx, name, iters):
    x, W, free, st, mark = case(name)
    B, r = x.shape[0], free.shape[1]
    est, path, its, f, P = ctx.em_mf_blocks_batch_host(*_args(x, st, W, free), max_iter=iters)
    for b in range(B):
        ref, opath, out = model(name, iters)[b]
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")
        for k in KEYS:
            tol = 1e-7 * max(1.0, np.abs(ref[k]).max())
            err = np.abs(est[k][b] - ref[k]).max()
            print(f"b={b} {k} {err:.2e}")
            assert err <= tol, (k, b, err)
        fo = out["f_smooth"][:, :r]
        assert np.abs(f[b] - fo).max() <= 1e-8 * max(1.0, np.abs(fo).max())
        assert _rel(P[b], _packed(out["P_smooth"], r)) <= 1e-8
    assert np.all(its == iters)
    # fixed entries bit for bit: zeros, the 1, the all-fixed row; the keep rule at its boundary
    assert np.array_equal(est["Lam"][:, ~free], st["Lam"][:, ~free])
    assert np.all(est["Lam"][(slice(None),) + mark["one"]] == 1.0) and not est["Lam"][:, mark["fixed_row"]].any()
    assert np.all(est["R"][:, mark["fixed_row"]] != st["R"][:, mark["fixed_row"]])          # k_i = 0: the variance alone
    at, above = mark["at"], mark["above"]
    assert np.array_equal(est["Lam"][:, at], st["Lam"][:, at]) and np.array_equal(est["R"][:, at], st["R"][:, at])
    assert np.all(est["Lam"][:, above][:, free[above]] != st["Lam"][:, above][:, free[above]])
    assert np.all(est["R"][:, above] != st["R"][:, above])


def test_null_mask_is_the_unrestricted_entry_bit_for_bit(ctx):
    x, W, free, st, _ = case("b")
    a, pa, ia, fa, Pa = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=3)
    b, pb, ib, fb, Pb = ctx.em_mf_blocks_batch_host(*_args(x, st, W, None), max_iter=3)
    assert np.array_equal(pa, pb) and np.array_equal(ia, ib) and np.array_equal(fa, fb) and np.array_equal(Pa, Pb)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_all_ones_mask_is_the_unrestricted_model(ctx):
    """One model by two kernels: the bound of test_gpu_mf.test_one_lag_is_the_varp_model."""
    x, W, free, st, _ = case("b")
    a, pa, _, fa, Pa = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=3)
    b, pb, _, fb, Pb = ctx.em_mf_blocks_batch_host(*_args(x, st, W, np.ones_like(free)), max_iter=3)
    assert _rel(pa, pb) <= 1e-10 and _rel(fa, fb) <= 1e-10 and _rel(Pa, Pb) <= 1e-10
    for k in KEYS:
        assert _rel(b[k], a[k]) <= 1e-10, (k, _rel(b[k], a[k]))
    prof_names = []
    ctx.profile_enable(True)
    ctx.em_mf_blocks_batch_host(*_args(x, st, W, free), max_iter=1)
    prof_names.append(set(ctx.profile_read()))
    ctx.profile_enable(True)
    ctx.em_mf_blocks_batch_host(*_args(x, st, W, None), max_iter=1)
    prof_names.append(set(ctx.profile_read()))
    ctx.profile_enable(False)
    assert "mf_solve_blocks_kernel" in prof_names[0] and "mf_solve_kernel" not in prof_names[0]
    assert "mf_solve_kernel" in prof_names[1] and "mf_solve_blocks_kernel" not in prof_names[1]


@pytest.mark.parametrize("tol", [1e-5, 5e-3])
def test_tol_stops_replicates_separately(ctx, tol):
    """Case e, max_iter = 40.  At tol = 1e-5 no replicate of the MODEL stops within 40 iterations (its relative steps are still
    ~1e-3 there), so that run checks the bookkeeping and the paths only; at 5e-3 the model stops after 14, 25 and 11 iterations,
    and the replicates that stopped first sit through the others' series steps untouched."""
    x, W, free, st, mark = case("e")
    st = dict(st, Lam=st["Lam"].copy())
    st["Lam"][2] = np.where(free, 0.3 * st["Lam"][2], st["Lam"][2])       # one replicate starts further away
    est, path, its, _, _ = ctx.em_mf_blocks_batch_host(*_args(x, st, W, free), max_iter=40, tol=tol)
    print("iters", its)
    for b in range(x.shape[0]):
        ref, opath, _ = mb.em_mf_blocks(x[b], {k: st[k][b] for k in KEYS}, W, free, max_iter=40, tol=tol)
        assert its[b] == len(opath), (b, its[b], len(opath))
        pb = path[b, :its[b]]
        np.testing.assert_allclose(pb, opath, rtol=1e-8)
        assert np.all(np.diff(pb) >= -1e-8 * np.abs(pb[:-1]))
        assert np.all(np.isnan(path[b, its[b]:]))
    assert np.array_equal(est["Lam"][:, ~free], st["Lam"][:, ~free])
    if tol == 5e-3:
        assert its.min() >= 2 and its.max() < 40 and len(set(its.tolist())) == 3


def test_device_entry_updates_in_place_and_leaves_the_mask(ctx):
    import torch
    x, W, free, st, _ = case("c")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)
    d = {k: t(st[k]) for k in KEYS}
    mask = t(free.astype(np.uint8) * 7)                         # any nonzero byte is "estimated"
    keep = mask.clone()
    path, its, f, P = ctx.em_mf_blocks_batch_dev(t(x), d["Lam"], d["R"], t(W), mask, d["Avar"], d["Q"], d["mu0"], d["P0"], max_iter=3)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(mask, keep)
    for b in range(x.shape[0]):
        ref, opath, _ = model("c", 3)[b]
        np.testing.assert_allclose(path[b].cpu().numpy(), opath, rtol=1e-8)
        for k in KEYS:
            assert np.abs(d[k][b].cpu().numpy() - ref[k]).max() <= 1e-7 * max(1.0, np.abs(ref[k]).max()), k
    assert np.array_equal(d["Lam"].cpu().numpy()[:, ~free], st["Lam"][:, ~free])
    assert P.shape == (2, 48, 6) and f.shape == (2, 48, 3)
    with pytest.raises(TypeError):
        ctx.em_mf_blocks_batch_dev(t(x), d["Lam"], d["R"], t(W), t(free.astype(np.float64)), d["Avar"], d["Q"], d["mu0"], d["P0"])


def test_status_codes_are_those_of_the_unrestricted_entry(ctx):
    from dynamic_factor_models_amd._lib import DfmError
    x, W, free, st, _ = case("c")
    x, st = x[:1], {k: v[:1] for k, v in st.items()}
    N = x.shape[2]

    def code(fn, *a, **kw):
        with pytest.raises(DfmError) as ei:
            fn(*a, **kw)
        return ei.value.code

    plain = lambda s, Wx: (x, s["Lam"], s["R"], Wx, s["Avar"], s["Q"], s["mu0"], s["P0"])
    r9 = dict(Lam=np.zeros((1, N, 9)), R=np.ones((1, N)), Avar=np.zeros((1, 9, 9)), Q=np.eye(9)[None], mu0=np.zeros((1, 27)),
              P0=np.eye(27)[None])
    c9 = code(ctx.em_mf_batch_host, *plain(r9, W), max_iter=2)
    assert code(ctx.em_mf_blocks_batch_host, *_args(x, r9, W, np.ones((N, 9), bool)), max_iter=2) == c9 == -2
    W9 = W.copy(); W9[:9, 2] = 0.01 * np.arange(9)               # nine distinct rows
    cw = code(ctx.em_mf_batch_host, *plain(st, W9), max_iter=2)
    assert code(ctx.em_mf_blocks_batch_host, *_args(x, st, W9, free), max_iter=2) == cw == -1
    # a NULL required pointer (R), through the library itself
    lib, p = ctx._lib, lambda a: ctypes.c_void_p(a.ctypes.data)
    B, T, _ = x.shape
    r, L = free.shape[1], W.shape[1]
    pp = st["Avar"].shape[2] // r
    cp = {k: np.array(v) for k, v in st.items()}
    xx, Wc, m8 = np.ascontiguousarray(x), np.ascontiguousarray(W), np.ascontiguousarray(free, dtype=np.uint8)
    path, its = np.empty((B, 2)), np.empty(B, np.int32)
    head = (ctx._h, B, T, N, r, pp, L, p(xx), p(cp["Lam"]), None, p(Wc))
    tail = (p(cp["Avar"]), p(cp["Q"]), p(cp["mu0"]), p(cp["P0"]), 2, 0.0, p(path), p(its), None, None, 1)
    null_plain = lib.dfm_em_mf_batch(*head, *tail)
    null_blocks = lib.dfm_em_mf_blocks_batch(*head, p(m8), *tail)
    assert null_blocks == null_plain and null_plain != 0
    est, path, _, _, _ = ctx.em_mf_blocks_batch_host(*_args(x, st, W, free), max_iter=2)   # the handle works on
    assert np.isfinite(path).all()


def test_api_with_blocks_on_a_synthetic_panel(ctx):
    """T 72, N 24 (six quarterly), three blocks of one factor each: a global one and two halves.  The library's fit from the API's
    block-wise start against the NumPy model run from the NumPy block start; bounds of test_gpu_mf.test_api_on_the_stock_watson_sheets."""
    from dynamic_factor_models_amd import api
    x, W, _ = me.synth_mf(3, 18, 6, 72, 3, 2, "q_flow", ragged=2)
    kinds = ["m"] * 18 + ["q_flow"] * 6
    i = np.arange(24)
    mem = np.stack([np.ones(24, bool), i % 2 == 0, i % 2 == 1], axis=1)
    full = ~np.isnan(x).any(axis=0)
    assert (full & mem[:, 1])[:18].any() and (full & mem[:, 2])[:18].any() and not full[:18].all()
    fit = api.estimate_mixed_frequency(x, kinds, 3, 2, max_em_iter=4, tol_em=0.0, blocks=(mem, [1, 1, 1]), ctx=ctx)
    free = fit["free"]
    assert np.array_equal(free, mb.blocks_free(mem, [1, 1, 1])) and np.array_equal(fit["W"], W)
    z = (x - fit["mean"]) / fit["sd"]
    start = mb.mf_blocks_start(z, W, free, 2)
    for k in KEYS:
        print(f"start {k} {_rel(fit['start'][k], start[k]):.2e}")
    ref, opath, _ = mb.em_mf_blocks(z, start, W, free, max_iter=4)
    np.testing.assert_allclose(fit["loglik_path"], opath, rtol=1e-7)
    assert np.all(np.diff(opath) > 0)
    assert np.abs(fit["Lam"] - ref["Lam"]).max() <= 1e-6 * np.abs(ref["Lam"]).max()
    assert np.all(fit["Lam"][~free] == 0.0) and np.all(fit["Lam"][free] != 0.0)
    fc = api.forecast_mixed(fit, x, 6, ctx=ctx)
    assert fc["x"].shape == (78, 24) and fc["factor"].shape == (78, 3)
    assert all(np.isfinite(fc[k]).all() for k in ("x", "x_sd", "common", "factor")) and np.isfinite(fc["loglik"])
    rep = api.estimate_mixed_frequency(x, kinds, 3, 2, max_em_iter=2, tol_em=0.0, nrep=3, blocks=free, ctx=ctx)
    assert np.array_equal(rep["replicates"]["params"]["Lam"][:, ~free], np.zeros((3, int((~free).sum()))))
    assert np.isfinite(rep["replicates"]["loglik_path"]).all()
