"""CPU checks of the instrument-identified IRFs (dfm_proxyirf_batch): the expectation model of tests/proxy_expect.py against its own
invariants (the block starts, L = n, the normalisation, continuation, rotation invariance, recovery of a known impact column), the
condition under which tests/test_gpu_proxy.py compares every slot, the status codes the library decides without a device, the
binding of dynamic_factor_models_amd/structural.py against a call recorder and _lib.SYMBOLS, and the api's refusals.  No kernel is
launched here."""
import ctypes

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, structural
from tests import proxy_expect as px
from tests import structural_expect as se
from tests.test_signirf_cpu import one_call
from tests.test_structural_cpu import HANDLE, _rot, addr, arrays, both, make_ctx, shaped, val

SEED = px.SEED


# ------------------------------------------------------------------------------------------------------------ the model
def test_block_starts_cover_0_to_n_minus_L_and_nothing_else():
    for n, L in [(10, 7), (40, 40), (41, 1), (43, 8)]:
        seen = set()
        for g in range(400):
            s = px.starts(SEED, g, 1, n, L)
            assert len(s) == -(-n // L)
            seen.update(s)
        assert seen == set(range(n - L + 1)), (n, L, sorted(seen))
    # the formula at the ends of the word's range
    for n, L in [(10, 7), (107, 5)]:
        assert (0 * (n - L + 1)) >> 32 == 0 and ((2 ** 32 - 1) * (n - L + 1)) >> 32 == n - L


def test_positions_are_whole_blocks_with_the_last_one_cut():
    n, L = 43, 8
    pos = px.positions(SEED, 3, 0, n, L)
    assert pos.size == n and pos.min() >= 0 and pos.max() <= n - 1
    for k in range(n // L):
        assert np.array_equal(np.diff(pos[k * L:(k + 1) * L]), np.ones(L - 1, int))
    assert np.array_equal(np.diff(pos[(n // L) * L:]), np.ones(n % L - 1, int))


def test_block_length_n_makes_every_slot_the_sample():
    c = px.build("r4p4")
    for o in px.expect(c, 3, 6, L=c["n"]):
        for s in range(1, 7):
            assert np.array_equal(o["impact"][s], o["impact"][0]) and o["rel"][s] == o["rel"][0]
            assert np.array_equal(o["irf"][s], o["irf"][0])


@pytest.mark.parametrize("name", [c[0] for c in px.CASES])
def test_the_shock_has_unit_variance(name):
    c = px.build(name)
    for b, o in enumerate(px.expect(c, 2, 5, want_resp=False)):
        Q = c["params"]["Q"][b]
        for h in o["impact"]:
            assert abs(h @ np.linalg.solve(Q, h) - 1.0) <= 1e-13
        assert np.all(c["params"]["Lam"][b][c["norm"]] @ o["impact"].T >= 0.0)


def test_draws_continue_in_first_draw():
    c = px.build("r3p2")
    whole = px.expect(c, 4, 12)
    tail = px.expect(c, 4, 5, first=7)
    for b in range(2):
        assert np.array_equal(whole[b]["impact"][8:], tail[b]["impact"][1:]) and np.array_equal(whole[b]["irf"][8:], tail[b]["irf"][1:])
        assert np.array_equal(whole[b]["impact"][0], tail[b]["impact"][0])
    other = px.expect(c, 4, 3, want_resp=False)
    assert not np.array_equal(other[0]["impact"][1:], other[1]["impact"][1:])        # the stream word carries the replicate


@pytest.mark.parametrize("name", ["r3p2", "r4p4"])
def test_rotation_invariance(name):
    """Lam M^-1, M A_j M^-1, M Q M', M mu0, M P0 M': the smoother runs again on the rotated set.  impact -> M impact; rel, irf, fevd
    and shock do not move."""
    c = px.build(name)
    H, D, b = 6, 4, 0
    M = _rot(c["r"])
    q = {k: c["params"][k][b] for k in px.KEYS}
    q2 = px.rotate_all(q, M)
    f2, ll2 = se.smooth(c["panel"][b], *[q2[k] for k in px.KEYS], p=c["p"])
    assert abs(ll2 - c["loglik"][b]) <= 1e-9 * abs(ll2)
    kw = dict(sd=None if c["sd"] is None else c["sd"][b], cum=c["cum"], unit=c["unit"])
    a = px.run(c["f"][b], q["Lam"], q["R"], q["A"], q["Q"], H, c["z"], c["norm"], D, c["L"], SEED, 0, b, **kw)
    r2 = px.run(f2, q2["Lam"], q2["R"], q2["A"], q2["Q"], H, c["z"], c["norm"], D, c["L"], SEED, 0, b, **kw)
    for k in ("rel", "irf", "fevd", "shock"):
        assert np.abs(r2[k] - a[k]).max() <= 1e-9 * max(1.0, np.abs(a[k]).max()), k
    assert np.abs(r2["impact"] - a["impact"] @ M.T).max() <= 1e-9 * max(1.0, np.abs(a["impact"]).max())
    assert np.abs(r2["impact"] - a["impact"]).max() > 1e-3, "the impact vector should move with the rotation"


def test_a_known_impact_column_is_recovered():
    """T = 400, eta_t = S u_t, the instrument is u_1 plus noise: slot 0's impact vector points along S e_1 in the Q^-1 inner
    product (cosine >= 0.9: a loose bound on the method, not on arithmetic)."""
    g = np.random.default_rng(12)
    T, N, r = 400, 20, 3
    Lam = g.standard_normal((N, r))
    A = np.diag([0.6, 0.3, -0.2]) + 0.05 * g.standard_normal((r, r))
    S = np.tril(g.standard_normal((r, r))) + 1.5 * np.eye(r)
    Q = S @ S.T
    R = g.uniform(0.3, 0.8, N)
    u = g.standard_normal((T, r))
    f = np.zeros((T, r))
    for t in range(1, T):
        f[t] = A @ f[t - 1] + S @ u[t]
    x = f @ Lam.T + np.sqrt(R) * g.standard_normal((T, N))
    z = u[:, 0] + 0.5 * g.standard_normal(T)
    z[5:9] = np.nan
    fs, _ = se.smooth(x, Lam, R, A, Q, np.zeros(r), 4.0 * np.eye(r))
    o = px.run(fs, Lam, R, A, Q, 2, z, 0, 0, 1, SEED, 0, 0, want_resp=False)
    h, truth = o["impact"][0], S[:, 0]
    Qi = np.linalg.inv(Q)
    cos = abs(h @ Qi @ truth) / np.sqrt((h @ Qi @ h) * (truth @ Qi @ truth))
    print(f"cosine {cos:.4f}, rel {o['rel'][0]:.3f}")
    assert cos >= 0.9


def gpu_runs():
    """(case, D, L or None, missing) of every comparison tests/test_gpu_proxy.py makes against the model."""
    runs = [(c[0], px.D_CASE, None, 0.1, None) for c in px.CASES]
    runs += [("r3p2", max(px.D_EDGES), None, 0.1, None), ("r4p4", px.D_CASE, "n", 0.1, None), ("r3p2", px.D_CASE, None, 0.0, None),
             ("r8unit", px.D_CASE, None, 0.1, px.T_LONG)]
    return runs


@pytest.mark.parametrize("name,D,L,missing,T", gpu_runs())
def test_the_gpu_table_can_compare_every_slot(name, D, L, missing, T):
    """What lets the GPU test leave no slot out: over all slots of the case the instrument stays relevant (min rel >= 0.05, so
    kappa is far from 0) and the impact response of `norm` stays away from 0 (the sign and the unit effect are well determined)."""
    c = px.build(name, missing=missing, T=T)
    for b, o in enumerate(px.expect(c, 1, D, L=c["n"] if L == "n" else None, want_resp=False)):
        s = 1.0 if c["sd"] is None else c["sd"][b]
        resp = np.abs(s * (o["impact"] @ c["params"]["Lam"][b].T))              # [D+1, N]
        print(f"{name} b={b} D={D}: n {c['n']}, min rel {o['rel'].min():.3f}, min |norm response| / max {np.min(resp[:, c['norm']] / resp.max(axis=1)):.3e}")
        assert o["pd"] and np.all(np.isfinite(o["rel"])) and o["rel"].min() >= 0.05
        assert np.all(resp[:, c["norm"]] >= 1e-6 * resp.max(axis=1))


def test_the_long_case_is_past_the_lds_threshold():
    """csrc/dfm_kernels.h kPxTabLds: n rows of (r + 1) | 1 doubles; the table cases sit under it, the long case over it."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamic_factor_models_amd", "csrc", "dfm_kernels.h")).read()
    lds = eval(re.search(r"constexpr size_t kPxTabLds = ([0-9 *]+);", src).group(1))
    size = lambda c: c["n"] * ((c["r"] + 1) | 1) * 8
    assert all(size(px.build(row[0])) <= lds for row in px.CASES)
    assert size(px.build("r8unit", T=px.T_LONG)) > lds


def test_case_builder_places_the_gaps():
    for row in px.CASES:
        c = px.build(row[0])
        z, p, T = c["z"], c["p"], c["T"]
        assert np.isnan(z[p - 1]) and np.isnan(z[T - 1]) and np.isnan(z[20:23]).all() and np.isfinite(z[:p - 1]).all()
        assert c["n"] == px.used_rows(z, p).size >= c["r"] + 2 and (c["L"] == 1 or c["n"] % c["L"] != 0)
        assert np.isnan(c["panel"]).mean() > 0.05 and not np.array_equal(c["params"]["Q"][0], c["params"]["Q"][1])


# ------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes_without_a_device():
    lib = _lib.load()
    T = 12
    zbuf = (ctypes.c_double * T)(*([float("nan")] + [0.1 * t for t in range(1, T)]))
    znan = (ctypes.c_double * T)(*([0.5] * 4 + [float("nan")] * (T - 4)))
    zp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for fn in (lib.dfm_proxyirf_batch, lib.dfm_proxyirf_batch_dev):
        def call(B=1, T=T, N=5, r=2, p=1, H=3, z=zp(zbuf), norm=0, D=4, L=2, first=0):
            return fn(None, B, T, N, r, p, H, *[None] * 9, z, norm, D, L, 7, first, *[None] * 7, 0)
        assert call() == -3                                                    # NULL handle, sizes in order
        assert call(z=None) == -3
        assert call(H=0) == -1 and call(D=-1) == -1 and call(first=-1) == -1 and call(B=0) == -1 and call(p=0) == -1
        assert call(T=1) == -1 and call(T=2, p=2) == -1                        # T < p + 1
        assert call(norm=-1) == -1 and call(norm=5) == -1 and call(norm=4) == -3
        assert call(L=0) == -1 and call(L=12) == -1 and call(L=11) == -3       # n = 11 usable periods (t = 0 is NaN and t < p)
        assert call(p=2, L=11) == -1 and call(p=2, L=10) == -3                 # n = 10 with two lags
        assert call(z=zp(znan)) == -1 and call(z=zp(znan), r=1, L=1) == -3     # n = 3: r + 2 = 4 > 3; r = 1 fits
        assert call(r=9, p=4, N=40) == -2                                      # r p > 32
        assert call(B=2 ** 20, D=2 ** 11) == -1 and call(B=2 ** 20, D=2 ** 11 - 2) == -3      # B (D + 1) >= 2^31


def test_api_refuses_before_any_device_work():
    x = np.random.default_rng(0).standard_normal((40, 7))
    m = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    z = np.random.default_rng(2).standard_normal(40)
    with pytest.raises(ValueError, match="not been estimated"):
        api.structural_irf_proxy(m, 4, z, norm=0)
    with pytest.raises(ValueError, match="H must be"):
        api.structural_irf_proxy(m, 0, z, norm=0)
    g = np.random.default_rng(1)
    m.em_params = dict(Lam=g.standard_normal((7, 2)), R=np.ones(7), A=0.5 * np.eye(2), Q=np.eye(2), mu0=np.zeros(2), P0=np.eye(2))
    ep = {k: v.copy() for k, v in m.em_params.items()}
    with pytest.raises(ValueError, match="draws must be"):
        api.structural_irf_proxy(m, 4, z, norm=0, draws=-1)
    with pytest.raises(ValueError, match="quantile bands need draws"):
        api.structural_irf_proxy(m, 4, z, norm=0, quantiles=[0.5])
    with pytest.raises(ValueError, match="bootstrap replicates"):
        api.structural_irf_proxy(m, 4, z, norm=0, draws=5, quantiles=[0.5], parameter_draws=True)
    with pytest.raises(ValueError, match=r"1 x 16385 draws; at most 16384"):
        api.structural_irf_proxy(m, 4, z, norm=0, draws=16385, quantiles=[0.5])
    m.replicates = dict(params=dict(Lam=np.zeros((300, 7, 2))))
    with pytest.raises(ValueError, match=r"300 x 55 draws; at most 16384"):
        api.structural_irf_proxy(m, 4, z, norm=0, draws=55, quantiles=[0.5], parameter_draws=True)
    m.replicates = None
    with pytest.raises(ValueError, match="one entry per row"):
        api.structural_irf_proxy(m, 4, z[:39], norm=0)
    few = np.full(40, np.nan); few[10:13] = 1.0
    with pytest.raises(ValueError, match="3 usable periods"):
        api.structural_irf_proxy(m, 4, few, norm=0)
    for bad in (0, 40):                                            # n = 39: row 1 of the window precedes the first lag
        with pytest.raises(ValueError, match=r"block must lie in 1\.\.39"):
            api.structural_irf_proxy(m, 4, z, norm=0, block=bad)
    m2 = api.DFMModel(x, [1, 1, 0, 1, 1, 1, 1], 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    m2.em_params = dict(m.em_params, Lam=m.em_params["Lam"][:6], R=np.ones(6))
    for call in (lambda: api.structural_irf_proxy(m2, 4, z, norm=2), lambda: api.structural_irf_proxy(m2, 4, z, norm=0, cumulate=[2])):
        with pytest.raises(ValueError, match="series 2 is not among"):
            call()
    mo = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 1, 2, 1e-8, 4, 4)
    mo.em_params = m.em_params
    with pytest.raises(ValueError, match="nfac_o = 0"):
        api.structural_irf_proxy(mo, 4, z, norm=0)
    ma = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    ma.em_params = m.em_params
    ma.uar_coef = np.full((7, 4), 0.3)
    with pytest.raises(ValueError, match="AR idiosyncratic"):
        api.structural_irf_proxy(ma, 4, z, norm=0)
    if not torch.cuda.is_available():                             # and past the refusals there is no CPU fallback
        with pytest.raises(RuntimeError, match="HIP device"):
            api.structural_irf_proxy(m, 4, z, norm=0, draws=3, quantiles=[0.5])
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep)


# ------------------------------------------------------------------------------------------------------------ the binding
@pytest.mark.parametrize("mhm,bit", [(True, _lib.DFM_F_MAY_HAVE_MISSING), (False, 0)])
def test_proxyirf_binding(mhm, bit):
    from tests.test_structural_cpu import B, H, N, T, p, r
    ctx, a = make_ctx(), arrays()
    assert ctx.proxyirf_batch_host.__func__ is structural.proxyirf_batch_host
    z = np.linspace(-1.0, 1.0, T); z[5] = np.nan
    D, L = 6, 3
    for call, sym, s in both(ctx, "proxyirf_batch", a):
        P = [s[k] for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")]
        for full in (True, False):
            cum = [0, 1, 0, 0, 1, 0] if full else None
            got = call(s["panel"], *P, H, z, 4, draws=D, block=L, seed=2 ** 64 + 5, first_draw=2 ** 40, sd=s["sd"] if full else None,
                       cum=cum, unit_effect=full, want_irf=full, want_fevd=full, want_shock=full, may_have_missing=mhm, singular_q=full)
            args = one_call(ctx._lib, sym)
            assert val(args[0]) == HANDLE and args[1:7] == (B, T, N, r, p, H)
            assert [val(x) for x in args[7:14]] == [addr(s[k]) for k in ("panel", "Lam", "R", "Avar", "Q", "mu0", "P0")]
            assert val(args[14]) == (addr(s["sd"]) if full else None)
            if full:
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[15], ctypes.POINTER(ctypes.c_int)), (N,)), cum)
            else:
                assert args[15] is None
            zz = np.ctypeslib.as_array(ctypes.cast(args[16], ctypes.POINTER(ctypes.c_double)), (T,))
            assert np.array_equal(zz, z, equal_nan=True)
            assert args[17:22] == (4, D, L, 5, 2 ** 40)
            assert list(got) == ["impact", "rel", "irf", "fevd", "shock", "f", "loglik"]
            shaped(got["impact"], (B, D + 1, r), s["panel"]); shaped(got["rel"], (B, D + 1), s["panel"])
            shaped(got["f"], (B, T, r), s["panel"]); shaped(got["loglik"], (B,), s["panel"])
            if full:
                shaped(got["irf"], (B, D + 1, H, N), s["panel"]); shaped(got["fevd"], (B, D + 1, H, N), s["panel"])
                shaped(got["shock"], (B, T), s["panel"])
            else:
                assert got["irf"] is None and got["fevd"] is None and got["shock"] is None
            want = bit | ((_lib.DFM_F_SINGULAR_Q | _lib.DFM_SV_UNIT_EFFECT) if full else 0)
            assert [val(x) for x in args[22:]] == [addr(got[k]) for k in got] + [want]
        with pytest.raises(ValueError, match="H must be"):
            call(s["panel"], *P, 0, z, 0)
        with pytest.raises(ValueError, match="draws and first_draw"):
            call(s["panel"], *P, H, z, 0, draws=-1)
        with pytest.raises(ValueError, match="norm must be"):
            call(s["panel"], *P, H, z, N)
        with pytest.raises(ValueError, match="must have 12 entries"):
            call(s["panel"], *P, H, z[:-1], 0)
        with pytest.raises(ValueError, match="block must lie in 1..8"):          # rows 3 .. 11 without row 5
            call(s["panel"], *P, H, z, 0, block=9)
        with pytest.raises(ValueError, match="usable periods"):
            call(s["panel"], *P, H, np.where(np.arange(T) < 9, np.nan, z), 0)
        assert not ctx._lib.calls


def test_the_symbols_are_in_the_table_and_kalman_names_none_of_them():
    from dynamic_factor_models_amd import kalman
    assert {"dfm_proxyirf_batch", "dfm_proxyirf_batch_dev"} <= set(_lib.SYMBOLS)
    assert "dfm_proxyirf_batch" not in open(kalman.__file__).read()
    assert _lib.SYMBOLS["dfm_proxyirf_batch"] == _lib.SYMBOLS["dfm_proxyirf_batch_dev"]
