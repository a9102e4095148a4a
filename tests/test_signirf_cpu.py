"""CPU checks of the sign-restricted IRFs (dfm_signirf_batch): the expectation model of tests/signirf_expect.py against its own
invariants (the Haar factor, uniformity of the draws, the flip rule, rotation invariance with named series), the status codes the
library decides without a device, the binding of dynamic_factor_models_amd/structural.py against a call recorder and
_lib.SYMBOLS, and the api's refusals.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, structural
from tests import signirf_expect as sx
from tests import structural_expect as se
from tests.test_structural_cpu import HANDLE, _one, _rot, addr, arrays, both, make_ctx, shaped, val

SEED = 20160415


# ------------------------------------------------------------------------------------------------------------ the model
def test_the_batched_draw_is_normal2_of_the_oracle():
    for r, b, first in [(1, 0, 0), (3, 1, 3), (8, 2, 100), (16, 0, 7)]:
        Z = sx.draw(SEED, first, 5, b, r)
        for m in range(5):
            assert np.array_equal(Z[m], sx.draw_one(SEED, first + m, b, r)), (r, b, m)


@pytest.mark.parametrize("r", [1, 2, 3, 4, 8, 9, 16])
def test_rot_is_the_orthogonal_factor_with_a_positive_diagonal(r):
    for Z in sx.draw(SEED, 0, 50, 1, r):
        Rot, piv = sx.haar(Z)
        assert np.abs(Rot.T @ Rot - np.eye(r)).max() <= 1e-14
        U = Rot.T @ Z
        assert np.all(np.diag(U) > 0.0) and np.abs(np.tril(U, -1)).max() <= 1e-13 * np.abs(Z).max()
        np.testing.assert_allclose(np.diag(U), piv, rtol=1e-12)


def test_first_column_is_uniform_on_the_sphere():
    """G = 0, 20 000 candidates of the fixed stream: for x uniform on the sphere of R^r, E x_i = 0 (variance 1 / r),
    E x_i x_j = delta_ij / r, Var x_i^2 = 3 / (r (r + 2)) - 1 / r^2, Var x_i x_j = 1 / (r (r + 2)).  Every |z| <= 4."""
    r, M = 4, 20000
    x = np.stack([sx.haar(Z)[0][:, 0] for Z in sx.draw(SEED, 0, M, 0, r)])
    z = [x.mean(axis=0) * np.sqrt(M * r)]
    second = np.einsum("mi,mj->ij", x, x) / M
    sd_diag = np.sqrt((3.0 / (r * (r + 2)) - 1.0 / r ** 2) / M)
    sd_off = np.sqrt(1.0 / (r * (r + 2)) / M)
    z.append((np.diag(second) - 1.0 / r) / sd_diag)
    z.append(second[np.triu_indices(r, 1)] / sd_off)
    z = np.concatenate(z)
    print(f"uniformity: largest |z| {np.abs(z).max():.2f} over {z.size} moments")
    assert np.abs(z).max() <= 4.0, z


def _case(named=True, cum=False):
    _, q = _one(N=10, r=3, p=2)
    nm = se.greedy_named(q["Lam"]) if named else None
    c = (np.arange(10) % 3 == 0) if cum else None
    return q, nm, c


def test_the_flip_rule():
    q, nm, c = _case(cum=True)
    H, M = 5, 300
    restr = [(0, 0, 0, 2, 1), (4, 0, 1, 3, -1), (2, 2, 0, 0, 1)]              # shock 1 has no restriction
    sd = np.linspace(0.5, 2.0, 10)
    o = sx.run(q["Lam"], q["A"], q["Q"], q["R"], H, restr, M, M, SEED, 0, 0, sd=sd, named=nm, cum=c)
    _, _, out = sx.base_responses(q["Lam"], q["A"], q["Q"], H, sd, nm, c)
    seen = set()
    for m in range(M):
        x = out @ o["Rot"][m]                                                  # [H, N, r]: the unflipped candidate's responses
        state = []
        for k, rows in ((0, restr[:2]), (2, restr[2:])):
            v = np.concatenate([sg * x[h0:h1 + 1, i, k] for i, _, h0, h1, sg in rows])
            state.append("hold" if np.all(v > 0) else "reversed" if np.all(v < 0) else "mixed")
        seen.add(tuple(state))
        assert bool(o["mask"][m]) == ("mixed" not in state), (m, state)
        assert o["D"][m][1] == 1.0, "a column without restrictions was flipped"
        if o["mask"][m]:
            assert [o["D"][m][0], o["D"][m][2]] == [1.0 if s == "hold" else -1.0 for s in state]
    assert len(seen) >= 6, seen                                                # the stream reaches the branches of the rule
    assert o["n_accept"] == o["mask"].sum() > 0
    for s in range(o["n_accept"]):                                             # every kept slot carries the required signs
        for i, k, h0, h1, sg in restr:
            assert np.all(sg * o["irf"][s][k, h0:h1 + 1, i] > 0.0)
        np.testing.assert_allclose(o["S"][s] @ o["S"][s].T, o["S0"] @ o["S0"].T, rtol=0, atol=1e-13 * np.abs(o["S0"]).max() ** 2)
    assert np.all(np.isnan(o["irf"][o["n_accept"]:])) and np.all(o["cand"][o["n_accept"]:] == -1)


def test_kept_irf_is_the_plain_irf_of_the_rotated_set():
    q, nm, c = _case(cum=True)
    restr = [(0, 0, 0, 2, 1), (1, 1, 0, 1, -1)]
    o = sx.run(q["Lam"], q["A"], q["Q"], q["R"], 6, restr, 200, 3, SEED, 0, 0, named=nm, cum=c)
    assert o["n_accept"] >= 3
    for s in range(3):
        L2, A2, Q2 = sx.rotated_set(q["Lam"], q["A"], o["S"][s])
        e = se.irf_fevd(L2, A2, Q2, q["R"], 6, cum=c)
        np.testing.assert_allclose(o["irf"][s], e["irf"], rtol=0, atol=1e-11 * np.abs(e["irf"]).max())
        np.testing.assert_allclose(o["fevd"][s], e["fevd"], rtol=0, atol=1e-12)


def test_candidates_do_not_depend_on_the_split():
    q, nm, _ = _case()
    restr = [(0, 0, 0, 2, 1)]
    whole = sx.run(q["Lam"], q["A"], q["Q"], q["R"], 4, restr, 100, 100, SEED, 0, 1, named=nm)
    tail = sx.run(q["Lam"], q["A"], q["Q"], q["R"], 4, restr, 60, 2, SEED, 40, 1, named=nm)
    assert np.array_equal(whole["mask"][40:], tail["mask"]) and np.array_equal(whole["Rot"][40:], tail["Rot"])


def test_rotation_invariance_of_the_accepted_set_needs_named_series():
    """The construction of test_rotation_invariance_needs_named_series: Lam M^-1, M A_j M^-1, M Q M'.  With named series the base
    impact matrix moves with M, so every candidate gives the same responses; without, chol(Q) depends on the rotation."""
    _, q = _one()
    H, M = 8, _rot(3)
    named = se.greedy_named(q["Lam"])
    # restrictions that candidate 3 satisfies, read off its own responses at h 0-2, so that the accepted set is not empty
    _, _, out = sx.base_responses(q["Lam"], q["A"], q["Q"], 3, named=named)
    x = out @ sx.haar(sx.draw_one(SEED, 3, 0, 3))[0]
    steady = lambda k: [int(i) for i in np.nonzero(np.all(x[:, :, k] > 0, axis=0) | np.all(x[:, :, k] < 0, axis=0))[0]]
    restr = [(i, k, 0, 2, 1 if x[0, i, k] > 0 else -1) for k in (0, 1) for i in steady(k)[:2]]
    assert len(restr) == 4
    L2, A2, Q2 = se.rotate(q["Lam"], q["A"], q["Q"], M)
    a = sx.run(q["Lam"], q["A"], q["Q"], q["R"], H, restr, 400, 400, SEED, 0, 0, named=named)
    b = sx.run(L2, A2, Q2, q["R"], H, restr, 400, 400, SEED, 0, 0, named=named)
    safe = a["margin"] > 1e-9
    assert safe.mean() > 0.99 and np.array_equal(a["mask"][safe], b["mask"][safe]) and a["n_accept"] > 0
    if safe.all():
        n = a["n_accept"]
        np.testing.assert_allclose(b["irf"][:n], a["irf"][:n], rtol=0, atol=1e-10 * np.abs(a["irf"][:n]).max())
    a0 = sx.run(q["Lam"], q["A"], q["Q"], q["R"], H, restr, 400, 1, SEED, 0, 0)
    b0 = sx.run(L2, A2, Q2, q["R"], H, restr, 400, 1, SEED, 0, 0)
    assert not np.array_equal(a0["mask"], b0["mask"]), "without named series the accepted set should depend on the rotation"


def test_the_case_table_has_accepted_draws():
    for name, N, r, p, series in sx.CASES:
        _, st = se.synth(2, N, 8 if p == 1 else 100, r, p)
        for named in (None, se.greedy_named(st["Lam"][0])):
            n = [sx.run(st["Lam"][b], st["A"][b], st["Q"][b], st["R"][b], 4, sx.restrictions(series, r), 96, 1, sx.CASE_SEED, 0, b,
                        named=named)["n_accept"] for b in range(2)]
            assert min(n) > 0, (name, named is None, n)


# ------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes_without_a_device():
    lib = _lib.load()
    ip = lambda a: ctypes.cast(a, ctypes.c_void_p)
    good = (ctypes.c_int * 10)(0, 0, 0, 2, 1, 4, 1, 1, 1, -1)
    for fn in (lib.dfm_signirf_batch, lib.dfm_signirf_batch_dev):
        def call(B=1, N=5, r=2, p=1, H=3, named=None, G=0, restr=None, M=8, K=1, flags=0):
            return fn(None, B, N, r, p, H, None, None, None, None, None, named, None, G, restr, M, K, 7, 0, None, None, None, None,
                      None, None, flags)
        assert call() == -3                                                    # NULL handle, sizes in order
        assert call(G=2, restr=ip(good)) == -3
        assert call(H=0) == -1 and call(M=0) == -1 and call(K=0) == -1 and call(G=-1) == -1 and call(B=0) == -1 and call(p=0) == -1
        assert call(G=1, restr=None) == -3                                     # restrictions announced but not given
        for bad in [(5, 0, 0, 2, 1), (-1, 0, 0, 2, 1), (0, 2, 0, 2, 1), (0, -1, 0, 2, 1), (0, 0, -1, 2, 1), (0, 0, 2, 1, 1),
                    (0, 0, 0, 3, 1), (0, 0, 0, 2, 0), (0, 0, 0, 2, 2)]:
            assert call(G=1, restr=ip((ctypes.c_int * 5)(*bad))) == -1, bad    # decided before the handle
        assert call(r=9, p=4, N=40) == -2                                      # r p > 32
        rep = (ctypes.c_int * 2)(1, 1)
        assert call(named=ip(rep)) == -1
        # the table of restricted responses: 13 series x 30 horizons x 16 factors x 8 bytes = 49 920 > 49 152; 12 series fit
        rows = []
        for i in range(13):
            rows += [i, 0, 0, 29, 1]
        big = (ctypes.c_int * len(rows))(*rows)
        assert call(N=20, r=16, H=30, G=13, restr=ip(big)) == -1
        assert call(N=20, r=16, H=30, G=12, restr=ip(big)) == -3


def test_api_refuses_before_any_device_work():
    x = np.random.default_rng(0).standard_normal((40, 7))
    m = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    rs = [(0, 0, 0, 2, 1)]
    with pytest.raises(ValueError, match="not been estimated"):
        api.structural_irf_signs(m, 4, rs)
    with pytest.raises(ValueError, match="H must be"):
        api.structural_irf_signs(m, 0, rs)
    g = np.random.default_rng(1)
    m.em_params = dict(Lam=g.standard_normal((7, 2)), R=np.ones(7), A=0.5 * np.eye(2), Q=np.eye(2), mu0=np.zeros(2), P0=np.eye(2))
    ep = {k: v.copy() for k, v in m.em_params.items()}
    with pytest.raises(ValueError, match="candidates must be"):
        api.structural_irf_signs(m, 4, rs, candidates=0)
    with pytest.raises(ValueError, match="keep must be"):
        api.structural_irf_signs(m, 4, rs, keep=0)
    with pytest.raises(ValueError, match="quantile bands need named"):
        api.structural_irf_signs(m, 4, rs, quantiles=[0.5])
    with pytest.raises(ValueError, match="bootstrap replicates"):
        api.structural_irf_signs(m, 4, rs, named=[0, 1], quantiles=[0.5])
    with pytest.raises(ValueError, match="2 distinct"):
        api.structural_irf_signs(m, 4, rs, named=[1, 1])
    for bad, msg in [([(0, 2, 0, 2, 1)], "shock must lie"), ([(0, 0, 0, 4, 1)], "h0 <= h1 < H"), ([(0, 0, 2, 1, 1)], "h0 <= h1 < H"),
                     ([(0, 0, 0, 2, 0)], "sign must be"), ([(0, 0, 0, 2)], "rows"), ([(9, 0, 0, 2, 1)], "series 9 is not among")]:
        with pytest.raises(ValueError, match=msg):
            api.structural_irf_signs(m, 4, bad)
    m2 = api.DFMModel(x, [1, 1, 0, 1, 1, 1, 1], 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    m2.em_params = dict(m.em_params, Lam=m.em_params["Lam"][:6], R=np.ones(6))
    for call in (lambda: api.structural_irf_signs(m2, 4, [(2, 0, 0, 2, 1)]), lambda: api.structural_irf_signs(m2, 4, rs, cumulate=[2])):
        with pytest.raises(ValueError, match="series 2 is not among"):
            call()
    mo = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 1, 2, 1e-8, 4, 4)
    mo.em_params = m.em_params
    with pytest.raises(ValueError, match="nfac_o = 0"):
        api.structural_irf_signs(mo, 4, rs)
    if not torch.cuda.is_available():                             # and past the refusals there is no CPU fallback
        with pytest.raises(RuntimeError, match="HIP device"):
            api.structural_irf_signs(m, 4, rs)
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep)


# ------------------------------------------------------------------------------------------------------------ the binding
def one_call(lib, name):
    """The recorder's single call: plain ints where _lib.SYMBOLS has an integer type, pointers (or None) elsewhere."""
    assert [c[0] for c in lib.calls] == [name]
    args = lib.calls[0][1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds)
    for i, (x, kind) in enumerate(zip(args, kinds)):
        if kind in (ctypes.c_int, ctypes.c_uint, ctypes.c_uint64, ctypes.c_int64):
            assert type(x) is int, (name, i)
        else:
            assert x is None or isinstance(x, ctypes.c_void_p), (name, i)
    lib.calls.clear()
    return args


def test_signirf_binding():
    from tests.test_structural_cpu import B, H, N, p, r
    ctx, a = make_ctx(), arrays()
    assert ctx.signirf_batch_host.__func__ is structural.signirf_batch_host
    restr = [(3, 0, 0, 2, 1), (1, 1, 1, 3, -1), (3, 1, 0, 0, 1)]
    M, K = 70, 3
    for call, sym, s in both(ctx, "signirf_batch", a):
        for full in (True, False):
            named = [3, 1] if full else None
            cum = [0, 1, 0, 0, 1, 0] if full else None
            got = call(s["Lam"], s["Avar"], s["Q"], s["R"], H, restr if full else None, M, K, seed=2 ** 64 + 5, first_cand=2 ** 40,
                       sd=s["sd"] if full else None, named=named, cum=cum, want_mask=full, want_S=full, want_irf=full, want_fevd=full)
            args = one_call(ctx._lib, sym)
            assert val(args[0]) == HANDLE and args[1:6] == (B, N, r, p, H)
            assert [val(x) for x in args[6:11]] == [addr(s[k]) for k in ("Lam", "Avar", "Q", "R")] + [addr(s["sd"]) if full else None]
            if full:
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[11], ctypes.POINTER(ctypes.c_int)), (r,)), named)
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[12], ctypes.POINTER(ctypes.c_int)), (N,)), cum)
                assert args[13] == 3
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[14], ctypes.POINTER(ctypes.c_int)), (3, 5)), restr)
            else:
                assert args[11] is None and args[12] is None and args[13] == 0 and args[14] is None
            assert args[15:19] == (M, K, 5, 2 ** 40)
            assert list(got) == ["n_accept", "mask", "cand", "S", "irf", "fevd"]
            ints = torch.int32 if isinstance(s["Lam"], torch.Tensor) else np.int32
            assert tuple(got["n_accept"].shape) == (B,) and tuple(got["cand"].shape) == (B, K)
            assert got["n_accept"].dtype == ints and got["cand"].dtype == ints
            if full:
                assert tuple(got["mask"].shape) == (B, M) and got["mask"].dtype == ints
                shaped(got["S"], (B, K, r, r), s["Lam"]); shaped(got["irf"], (B, K, r, H, N), s["Lam"])
                shaped(got["fevd"], (B, K, r + 1, H, N), s["Lam"])
            else:
                assert got["mask"] is None and got["S"] is None and got["irf"] is None and got["fevd"] is None
            assert [val(x) for x in args[19:]] == [addr(got[k]) for k in got] + [0]
        with pytest.raises(ValueError, match="H must be"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], 0, restr, M)
        with pytest.raises(ValueError, match="candidates and keep"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, restr, 0)
        with pytest.raises(ValueError, match="rows"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, [(0, 0, 0, 1)], M)
        with pytest.raises(ValueError, match="sign"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, [(0, 0, 0, 1, 2)], M)
        with pytest.raises(ValueError, match="distinct"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, restr, M, named=[1, 1])
        assert not ctx._lib.calls


def test_the_symbols_are_in_the_table_and_kalman_names_none_of_them():
    from dynamic_factor_models_amd import kalman
    assert {"dfm_signirf_batch", "dfm_signirf_batch_dev"} <= set(_lib.SYMBOLS)
    assert "dfm_signirf_batch" not in open(kalman.__file__).read()
