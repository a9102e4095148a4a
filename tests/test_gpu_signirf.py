"""GPU tests of dfm_signirf_batch (include/dfm_hip.h; csrc/signirf.hip) against the expectation model of tests/signirf_expect.py at
the project's 1e-9 x max(1, scale): the mask, the counts, the kept candidates, their impact matrices, responses and variance
shares over the case table; then what the device must satisfy on its own (orthogonality, the signs, the plain IRF of the rotated
set, continuation, independence of M and K, determinism, the two entries, empty slots, status codes) and the api."""
import ctypes
import functools

import numpy as np
import pytest

from tests import signirf_expect as sx
from tests import structural_expect as se

pytestmark = pytest.mark.gpu
TOL = 1e-9
SEED = sx.CASE_SEED
B, H, MMAX = 2, 6, 512
M_SWEEP = (1, 63, 64, 65, 257, 512)          # block edges of sv_sign_kernel (64 candidates per wave, 256 per workgroup)

# name of the shape in signirf_expect.CASES -> (named, cumulated series among the restricted ones, sd, K, fevd)
VARIANTS = {"r4": (True, True, True, 8, True), "r3p2": (False, False, False, 600, True), "r8": (True, False, True, 4, False),
            "r2": (False, True, False, 3, True), "r1": (True, False, False, 2, False), "r9": (True, False, True, 2, True),
            "r16p2": (False, True, False, 600, False)}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    scale = max(1.0, float(np.nanmax(np.abs(b)))) if np.isfinite(b).any() else 1.0
    err = float(np.nanmax(np.abs(a - b))) if np.isfinite(b).any() else 0.0
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def _setup(name):
    """The inputs of a case and the model's verdict on MMAX candidates of both replicates: computed once, shared, never changed."""
    _, N, r, p, series = next(c for c in sx.CASES if c[0] == name)
    named_on, cum_on, sd_on, K, fevd = VARIANTS[name]
    _, st = se.synth(B, N, 8 if p == 1 else 100, r, p)
    g = np.random.default_rng(7)
    named = se.greedy_named(st["Lam"][0]) if named_on else None
    cum = None
    if cum_on:
        cum = (g.random(N) < 0.3).astype(np.int32)
        cum[series[0]] = 1                                       # a cumulated restricted series
    sd = g.uniform(0.5, 3.0, (B, N)) if sd_on else None
    restr = sx.restrictions(series, r)
    model = [sx.run(st["Lam"][b], st["A"][b], st["Q"][b], st["R"][b], H, restr, MMAX, 1, SEED, 0, b, sd=None if sd is None else sd[b],
                    named=named, cum=cum) for b in range(B)]
    return dict(N=N, r=r, p=p, st=st, named=named, cum=cum, sd=sd, restr=restr, K=K, fevd=fevd, model=model)


def _call(ctx, c, M, K, first=0, restr="case", **kw):
    st = c["st"]
    kw = dict(dict(sd=c["sd"], named=c["named"], cum=c["cum"], want_mask=True), **kw)
    return ctx.signirf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], H, c["restr"] if restr == "case" else restr, M, K, seed=SEED,
                                  first_cand=first, **kw)


def _against_the_model(c, got, M, K, what, fevd):
    """mask, n_accept, cand and the slots against the model.  A candidate may be left out of the mask comparison only if the model's
    cond(Z) > 1e4 or its smallest restricted |response| is below 1e-7; the left-out share stays <= 1 %."""
    st = c["st"]
    for b in range(B):
        mo = c["model"][b]
        out = (mo["cond"][:M] > 1e4) | (mo["margin"][:M] < 1e-7)
        print(f"{what} b={b}: model accepts {mo['mask'][:M].sum()} of {M}, {out.sum()} left out")
        assert out.mean() <= 0.01, (what, b, out.mean())
        diff = np.nonzero((got["mask"][b] != mo["mask"][:M]) & ~out)[0]
        assert diff.size == 0, f"{what} b={b}: mask differs at candidates {diff[:8]}"
        force = {int(m): int(got["mask"][b][m]) for m in np.nonzero(out)[0]}
        e = sx.run(st["Lam"][b], st["A"][b], st["Q"][b], st["R"][b], H, c["restr"], M, K, SEED, 0, b,
                   sd=None if c["sd"] is None else c["sd"][b], named=c["named"], cum=c["cum"], force=force)
        assert got["n_accept"][b] == e["n_accept"] and np.array_equal(got["cand"][b], e["cand"]), (what, b)
        sure = np.array([m < 0 or not out[m] for m in e["cand"]])          # slots whose candidate was compared
        if got["S"] is not None:
            _close(got["S"][b][sure], e["S"][sure], f"{what} b={b} S_out")
        if got["irf"] is not None:
            _close(got["irf"][b][sure], e["irf"][sure], f"{what} b={b} irf")
        if fevd:
            _close(got["fevd"][b][sure], e["fevd"][sure], f"{what} b={b} fevd")
            full = e["cand"] >= 0
            assert np.abs(got["fevd"][b][full].sum(axis=1) - 1.0).max() <= 1e-12 if full.any() else True


# ------------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("name", [c[0] for c in sx.CASES])
def test_case_table_against_the_model(ctx, name):
    c = _setup(name)
    got = _call(ctx, c, MMAX, c["K"], want_fevd=c["fevd"])
    _against_the_model(c, got, MMAX, c["K"], name, c["fevd"])
    n = got["n_accept"]
    if c["K"] > n.max():                                         # K above n_accept: empty slots are NaN and -1
        for b in range(B):
            assert np.all(got["cand"][b][n[b]:] == -1) and np.all(np.isnan(got["S"][b][n[b]:])) and np.all(np.isnan(got["irf"][b][n[b]:]))
            assert np.all(np.isfinite(got["irf"][b][:n[b]]))
            if c["fevd"]:
                assert np.all(np.isnan(got["fevd"][b][n[b]:]))
    else:
        assert n.min() > c["K"], "K should lie below n_accept in this case"


@pytest.mark.parametrize("name", ["r3p2", "r9"])
@pytest.mark.parametrize("M", M_SWEEP)
def test_block_edges_against_the_model(ctx, name, M):
    c = _setup(name)
    got = _call(ctx, c, M, 3)
    _against_the_model(c, got, M, 3, f"{name} M={M}", False)


def test_no_restrictions_and_null_outputs(ctx):
    c = _setup("r4")
    got = _call(ctx, c, 130, 5, restr=None, want_S=False, want_irf=False)
    assert np.all(got["mask"] == 1) and np.all(got["n_accept"] == 130) and np.array_equal(got["cand"], np.tile(np.arange(5), (B, 1)))
    assert got["S"] is None and got["irf"] is None
    only_s = _call(ctx, c, 130, 5, want_irf=False)
    only_f = _call(ctx, c, 130, 5, want_S=False, want_irf=False, want_fevd=True)
    both = _call(ctx, c, 130, 5, want_fevd=True)
    assert np.array_equal(only_s["S"], both["S"], equal_nan=True) and np.array_equal(only_f["fevd"], both["fevd"], equal_nan=True)
    assert np.array_equal(only_s["mask"], both["mask"]) and only_f["irf"] is None


# ------------------------------------------------------------------------------------------------------------ on the device alone
@pytest.mark.parametrize("name", [c[0] for c in sx.CASES])
def test_kept_slots_are_rotations_with_the_required_signs(ctx, name):
    """S_out S_out' = S S' at 1e-12 x scale in every kept slot, no exclusions (the orthogonality bound); the restricted responses
    carry their signs; irf equals dfm_irf_batch with named = NULL on the rotated set (Lam S_m, S_m^-1 A S_m, I)."""
    c = _setup(name)
    st, r = c["st"], c["r"]
    K = 16
    got = _call(ctx, c, MMAX, K)
    assert got["n_accept"].max() > 0
    for b in range(B):
        n = min(K, int(got["n_accept"][b]))
        S0 = c["model"][b]["S0"]
        SS = S0 @ S0.T
        worst = 0.0
        for s in range(n):
            Sm = got["S"][b][s]
            err = np.abs(Sm @ Sm.T - SS).max()
            worst = max(worst, err)
            assert err <= 1e-12 * max(1.0, np.abs(SS).max()), (name, b, s, err)
            for i, k, h0, h1, sg in c["restr"]:
                assert np.all(sg * got["irf"][b][s][k, h0:h1 + 1, i] > 0.0), (name, b, s, i, k)
        print(f"{name} b={b}: {n} kept slots, worst |S_m S_m' - S S'| {worst:.3e}")
        if n == 0:
            continue
        sets = [sx.rotated_set(st["Lam"][b], st["A"][b], got["S"][b][s]) for s in range(n)]
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape))
        plain = ctx.irf_batch_host(np.stack([q[0] for q in sets]), np.stack([q[1] for q in sets]), np.stack([q[2] for q in sets]),
                                   rep(st["R"][b]), H, sd=None if c["sd"] is None else rep(c["sd"][b]), cum=c["cum"], want_fevd=False)
        _close(got["irf"][b][:n], plain["irf"], f"{name} b={b} irf against dfm_irf_batch on the rotated set")


@pytest.mark.parametrize("name", ["r4", "r9"])
def test_continuation_and_independence_of_m_and_k(ctx, name):
    c = _setup(name)
    whole = _call(ctx, c, 300, 300)
    again = _call(ctx, c, 300, 300)
    for k in ("n_accept", "mask", "cand"):                       # two identical calls agree bit for bit
        assert np.array_equal(whole[k], again[k]), k
    for k in ("S", "irf"):
        assert np.array_equal(whole[k], again[k], equal_nan=True), k
    head, tail = _call(ctx, c, 100, 100), _call(ctx, c, 200, 200, first=100)
    assert np.array_equal(np.concatenate([head["mask"], tail["mask"]], axis=1), whole["mask"])
    small = _call(ctx, c, 257, 2)                                # other M, other K: the same candidates, the same bits
    assert np.array_equal(small["mask"], whole["mask"][:, :257])
    for b in range(B):
        for part, shift in ((head, 0), (tail, 100), (small, 0)):
            for s, m in enumerate(part["cand"][b]):
                if m < 0:
                    continue
                at = int(np.nonzero(whole["cand"][b] == m + shift)[0][0])
                assert np.array_equal(part["S"][b][s], whole["S"][b][at]) and np.array_equal(part["irf"][b][s], whole["irf"][b][at])
        n = int(whole["n_accept"][b])
        assert n == whole["mask"][b].sum() and np.array_equal(whole["cand"][b][:n], np.nonzero(whole["mask"][b])[0])
        assert np.all(whole["cand"][b][n:] == -1) and np.all(np.isnan(whole["S"][b][n:])) and np.all(np.isnan(whole["irf"][b][n:]))


def test_dev_and_host_entries_agree(ctx):
    import torch
    c = _setup("r4")
    st = c["st"]
    host = _call(ctx, c, 200, 4, want_fevd=True)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.signirf_batch(t(st["Lam"]), t(st["A"]), t(st["Q"]), t(st["R"]), H, c["restr"], 200, 4, seed=SEED, sd=t(c["sd"]),
                            named=c["named"], cum=c["cum"], want_mask=True, want_fevd=True)
    ctx.synchronize()
    for k in host:
        assert np.array_equal(got[k].cpu().numpy(), host[k], equal_nan=host[k].dtype == np.float64), k


# ------------------------------------------------------------------------------------------------------------ status
def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    _, st = se.synth(1, 20, 8, 2)
    restr = [(0, 0, 0, 1, 1)]
    lam = st["Lam"].copy()
    lam[0, 5] = lam[0, 3]                                    # two equal named rows: Ln singular
    with pytest.raises(_lib.DfmError) as ei:
        ctx.signirf_batch_host(lam, st["A"], st["Q"], st["R"], 4, restr, 64, named=[3, 5])
    assert ei.value.code == -5
    ok = ctx.signirf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], 4, [(0, 0, 0, 0, 1)], 64, named=[3, 5])   # the status word was cleared
    assert ok["n_accept"][0] == 64                            # one response on one shock: it holds or it is reversed, never mixed
    v = np.array([1.0, 2.0])
    got = ctx.signirf_batch_host(st["Lam"], st["A"], np.outer(v, v)[None], st["R"], 4, restr, 64)         # rank-deficient Q
    assert got["n_accept"][0] > 0 and np.all(np.isfinite(got["irf"][0, 0]))
    ptr = lambda a: ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)
    lib = ctx._lib
    L, R, A, Q = (np.ascontiguousarray(st[k]) for k in ("Lam", "R", "A", "Q"))
    na, cd = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rs = np.array(restr, dtype=np.int32)
    base = [ptr(L), ptr(A), ptr(Q), ptr(R), None, None, None]

    def call(G=1, restr=ptr(rs), M=8, K=1, n_accept=ptr(na), cand=ptr(cd), flags=0, H=4):
        return lib.dfm_signirf_batch(ctx._h, 1, 20, 2, 1, H, *base, G, restr, M, K, 3, 0, n_accept, None, cand, None, None, None, flags)
    assert call() == 0
    assert call(M=0) == -1 and call(K=0) == -1 and call(G=-1) == -1 and call(H=1) == -1                 # h1 = 1 is not < H = 1
    assert call(restr=None) == -3 and call(n_accept=None) == -3 and call(cand=None) == -3
    assert call(flags=_lib.DFM_SV_UNIT_EFFECT) == -3
    assert call(G=0, restr=None) == 0 and na[0] == 8


# ------------------------------------------------------------------------------------------------------------ the api
def test_api_on_a_small_synthetic_model_with_bands(ctx):
    from dynamic_factor_models_amd import api
    x, _ = se.synth(1, 12, 120, 2)
    m = api.DFMModel(x[0], np.ones(12), 20, 40, 1, 120, 0, 2, 1e-8, 4, 1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=8, seed=11)
    ep = {k: v.copy() for k, v in m.em_params.items()}
    cols, _, _, sd = api._forecast_inputs(m, m.lastperiod)
    named = cols[se.greedy_named(ep["Lam"])]
    Hh, r, N, M = 5, 2, cols.size, 200
    restr = [(int(cols[0]), 0, 0, 1, 1), (int(cols[1]), 1, 0, 0, -1)]
    o = api.structural_irf_signs(m, Hh, restr, candidates=M, named=named, cumulate=cols[:3], fevd=True, seed=9, ctx=ctx)
    pos = np.array([int(np.nonzero(cols == i)[0][0]) for i in named])
    cum = np.zeros(N, int); cum[:3] = 1
    e = sx.run(ep["Lam"], ep["A"], ep["Q"], ep["R"], Hh, [(0, 0, 0, 1, 1), (1, 1, 0, 0, -1)], M, M, 9, 0, 0, sd=sd, named=pos, cum=cum)
    out = (e["cond"] > 1e4) | (e["margin"] < 1e-7)                          # the leave-out rule of _against_the_model
    assert out.mean() <= 0.01
    idx = o["candidate_index"]
    n = idx.size
    want = e["cand"][:e["n_accept"]]
    assert n > 0 and np.array_equal(idx[~out[idx]], want[~out[want]]), "the accepted sets differ on a candidate that was not left out"
    assert o["irf"].shape == (n, N, Hh, r) and o["fevd"].shape == (n, N, Hh, r + 1) and o["impact"].shape == (n, r, r)
    assert o["accepted_share"] == n / M and o["candidates_used"] == M
    ia, ie = np.nonzero(~out[idx])[0], np.nonzero(~out[want])[0]
    _close(o["irf"][ia], e["irf"][ie].transpose(0, 3, 2, 1), "api irf")
    _close(o["fevd"][ia], e["fevd"][ie].transpose(0, 3, 2, 1), "api fevd")
    _close(o["impact"][ia], e["S"][ie], "api impact")
    two = api.structural_irf_signs(m, Hh, restr, candidates=M, keep=2, named=named, cumulate=cols[:3], seed=9, ctx=ctx)
    assert np.array_equal(two["irf"], o["irf"][:2]) and two["fevd"] is None and two["accepted_share"] == o["accepted_share"]
    q = np.array([0.1, 0.5, 0.9])
    ob = api.structural_irf_signs(m, Hh, restr, candidates=M, named=named, cumulate=cols[:3], quantiles=q, seed=9, ctx=ctx)
    assert ob["bands"].shape == (3, N, Hh, r) and np.all(np.isfinite(ob["bands"])) and np.all(np.diff(ob["bands"], axis=0) >= 0.0)
    assert 0 <= ob["replicates_without_a_draw"] < 8 and np.array_equal(ob["irf"], o["irf"])
    for i, k, h0, h1, sg in [(0, 0, 0, 1, 1), (1, 1, 0, 0, -1)]:           # the bands of a restricted response carry its sign
        assert np.all(sg * ob["bands"][:, i, h0:h1 + 1, k] > 0.0)
    with pytest.raises(ValueError, match="accepted share 0 of 3 candidates"):
        api.structural_irf_signs(m, Hh, [(int(cols[0]), 0, 0, 4, 1), (int(cols[0]), 0, 0, 0, -1)], candidates=3, ctx=ctx)
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep), "the api changed m.em_params"
