"""GPU tests of dfm_irf_batch and dfm_histdecomp_batch (include/dfm_hip.h; csrc/structural.hip) against the expectation model of
tests/structural_expect.py at the project's 1e-9 x max(1, scale): the IRF / FEVD case table of tests/structural_geometry.py
(every launch class of sv_irf_fill_kernel), rotation invariance on the GPU itself, the historical decomposition over the pass
routes (fused, time-chunked, tile, covariance form, companion), the status codes, and the api on the Stock-Watson panel."""
import ctypes
import os

import numpy as np
import pytest

from tests import structural_expect as se
from tests import structural_geometry as sg

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = se.KEYS


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
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _named(st):
    """One set of named series for the batch: greedy pivoting on replicate 0 (shared by every replicate, as the entry takes it)."""
    return se.greedy_named(st["Lam"][0])


# ------------------------------------------------------------------------------------------------------------ IRF and FEVD
@pytest.mark.parametrize("row", sg.IRF_CASES, ids=[c[0] for c in sg.IRF_CASES])
def test_irf_fevd_against_the_model(ctx, row):
    import torch
    c = sg.irf_case(row)
    B, N, r, H = 2, c["N"], c["r"], c["H"]
    _, st = se.synth(B, N, 8 if c["p"] == 1 else 100, r, c["p"])
    g = np.random.default_rng(7)
    named = _named(st) if c["named"] else None
    cum = (g.random(N) < 0.4).astype(np.int32) if c["cum"] else None
    if cum is not None:
        cum[0] = 1
    sd = g.uniform(0.5, 3.0, (B, N)) if c["sd"] else None
    kw = dict(sd=sd, named=named, cum=cum, unit_effect=c["unit"], want_fevd=c["fevd"])
    if c["misaligned"]:
        dev = torch.device("cuda", ctx.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        lib = ctx._lib
        buf = torch.empty(B * r * H * N + 1, dtype=torch.float64, device=dev)
        fv = torch.empty((B, r + 1, H, N), dtype=torch.float64, device=dev)
        Ld, Ad, Qd, Rd = t(st["Lam"]), t(st["A"]), t(st["Q"]), t(st["R"])
        nm = np.ascontiguousarray(named, dtype=np.int32)
        ctx._sync_stream()
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        rc = lib.dfm_irf_batch_dev(ctx._h, B, N, r, c["p"], H, p(Ld), p(Ad), p(Qd), p(Rd), None, ctypes.c_void_p(nm.ctypes.data),
                                   None, ctypes.c_void_p(buf.data_ptr() + 8), p(fv), 0)
        assert rc == 0
        ctx.synchronize()
        got = dict(irf=buf[1:].reshape(B, r, H, N).cpu().numpy(), fevd=fv.cpu().numpy())
    else:
        got = ctx.irf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], H, **kw)
    for b in range(B):
        e = se.irf_fevd(st["Lam"][b], st["A"][b], st["Q"][b], st["R"][b], H, sd=None if sd is None else sd[b], named=named,
                        cum=cum, unit_effect=c["unit"])
        _close(got["irf"][b], e["irf"], f"{c['name']} b={b} irf")
        if c["fevd"]:
            _close(got["fevd"][b], e["fevd"], f"{c['name']} b={b} fevd")
            assert np.abs(got["fevd"][b].sum(axis=0) - 1.0).max() <= 1e-12
        else:
            assert got["fevd"] is None
        if c["unit"]:
            assert np.all(got["irf"][b][np.arange(r), 0, named] == 1.0), "unit effect: the impact response is not exactly 1"


def test_dev_and_host_entries_agree(ctx):
    import torch
    _, st = se.synth(2, 60, 8, 4)
    named = _named(st)
    host = ctx.irf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], 6, named=named)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.irf_batch(t(st["Lam"]), t(st["A"]), t(st["Q"]), t(st["R"]), 6, named=named)
    ctx.synchronize()
    for k in ("irf", "fevd"):
        assert np.array_equal(got[k].cpu().numpy(), host[k]), k


@pytest.mark.parametrize("r,p", [(4, 1), (3, 2)])
def test_rotation_invariance_on_the_gpu(ctx, r, p):
    N, H = 60, 12
    x, st = se.synth(2, N, 100, r, p)
    named = _named(st)
    g = np.random.default_rng(3)
    rot = {k: [] for k in ("Lam", "A", "Q")}
    Ms = []
    for b in range(2):
        M = g.standard_normal((r, r)) + 2.0 * np.eye(r)
        assert np.linalg.cond(M) < 50
        Ms.append(M)
        for k, v in zip(("Lam", "A", "Q"), se.rotate(st["Lam"][b], st["A"][b], st["Q"][b], M)):
            rot[k].append(v)
    rot = {k: np.stack(v) for k, v in rot.items()}
    cum = (np.arange(N) % 3 == 0).astype(np.int32)
    a = ctx.irf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], H, named=named, cum=cum)
    b = ctx.irf_batch_host(rot["Lam"], rot["A"], rot["Q"], st["R"], H, named=named, cum=cum)
    _close(b["irf"], a["irf"], "irf under rotation")
    _close(b["fevd"], a["fevd"], "fevd under rotation")
    # the decomposition too: the rotated model has the same likelihood, shocks and contributions (mu0, P0 rotated with it)
    k = r * p
    mu0 = np.stack([np.kron(np.eye(p), Ms[i]) @ st["mu0"][i] for i in range(2)])
    P0 = np.stack([np.kron(np.eye(p), Ms[i]) @ st["P0"][i] @ np.kron(np.eye(p), Ms[i]).T for i in range(2)])
    ha = ctx.histdecomp_batch_host(x, *[st[kk] for kk in KEYS], named=named)
    hb = ctx.histdecomp_batch_host(x, rot["Lam"], st["R"], rot["A"], rot["Q"], mu0, P0, named=named)
    _close(hb["hd"], ha["hd"], "hd under rotation")
    _close(hb["shocks"], ha["shocks"], "shocks under rotation")


# ------------------------------------------------------------------------------------------------------------ decomposition
def _check_hd(ctx, x, st, p=1, sd=None, what="", **kw):
    B = x.shape[0]
    named = _named(st)
    got = ctx.histdecomp_batch_host(x, *[st[k] for k in KEYS], sd=sd, named=named, **kw)
    for b in range(B):
        f, ll = se.smooth(x[b], *[st[k][b] for k in KEYS], p=p)
        _close(got["f"][b], f, f"{what} b={b} f_out against the oracle")
        assert abs(got["loglik"][b] - ll) <= TOL * abs(ll), (what, b, got["loglik"][b], ll)
        e = se.histdecomp(got["f"][b], st["Lam"][b], st["A"][b], st["Q"][b], sd=None if sd is None else sd[b], named=named)
        _close(got["hd"][b], e["hd"], f"{what} b={b} hd against the model fed with f_out")
        _close(got["shocks"][b], e["shocks"], f"{what} b={b} shocks")
        s = np.ones(x.shape[2]) if sd is None else sd[b]
        _close(got["hd"][b].sum(axis=0), s * (got["f"][b] @ st["Lam"][b].T), f"{what} b={b} sum identity")
    return got


def test_hd_balanced_r8_fused_pass(ctx):
    x, st = se.synth(3, 60, 90, 8)
    got = _check_hd(ctx, x, st, what="r=8 balanced")
    _, _, ll = ctx.ks_pass_batch_host(x, *[st[k] for k in KEYS], want_P=False)
    assert np.array_equal(got["loglik"], ll), "loglik differs from the plain pass"
    lean = ctx.histdecomp_batch_host(x, *[st[k] for k in KEYS], named=_named(st), want_shocks=False)
    assert lean["shocks"] is None and np.array_equal(lean["hd"], got["hd"])


@pytest.mark.parametrize("r", [4, 8])
def test_hd_missing_odd_n_chunked(ctx, r):
    B, N, T = 3, 139, 222
    x, st = se.synth(B, N, T, r, missing=0.1, first=20)
    sd = np.random.default_rng(2).uniform(0.5, 3.0, (B, N))
    _check_hd(ctx, x, st, sd=sd, what=f"r={r} missing odd N")
    ctx.histdecomp_batch_host(x, *[st[k] for k in KEYS], named=_named(st))
    nf, nt = ctx.chunk_fallbacks()
    assert nt == B, "the pass did not run on the time-chunked recursion"


def test_hd_r20_missing_tile_route(ctx):
    x, st = se.synth(2, 120, 150, 20, missing=0.1, first=40)
    _check_hd(ctx, x, st, what="r=20")


def test_hd_singular_q_flag_with_a_positive_definite_q(ctx):
    x, st = se.synth(2, 50, 80, 4, missing=0.1, first=60)
    _check_hd(ctx, x, st, what="covariance form", singular_q=True)


@pytest.mark.parametrize("r,p", [(3, 2), (4, 4), (2, 3), (1, 12)])
def test_hd_companion_routes(ctx, r, p):
    x, st = se.synth(2, 40, 100, r, p, missing=0.1)
    got = _check_hd(ctx, x, st, p=p, what=f"r={r} p={p}")
    _, _, ll = ctx.ks_pass_varp_batch_host(x, *[st[k] for k in KEYS])
    np.testing.assert_allclose(got["loglik"], ll, rtol=TOL)
    assert np.all(got["shocks"][:, :p] == 0.0)


def test_hd_r32_two_chain_groups(ctx):
    """r = 32: the 33 chains run in two workgroups per replicate (tests/structural_geometry.py path)."""
    assert sg.path(32, 1)["groups"] == 2
    x, st = se.synth(2, 64, 40, 32, first=70)
    _check_hd(ctx, x, st, what="r=32")


# ------------------------------------------------------------------------------------------------------------ status
def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    x, st = se.synth(1, 20, 30, 2)
    P = [st[k] for k in KEYS]
    lam = st["Lam"].copy()
    lam[0, 5] = lam[0, 3]                                    # two equal named rows: Ln singular
    with pytest.raises(_lib.DfmError) as ei:
        ctx.irf_batch_host(lam, st["A"], st["Q"], st["R"], 4, named=[3, 5])
    assert ei.value.code == -5
    ctx.irf_batch_host(st["Lam"], st["A"], st["Q"], st["R"], 4, named=[3, 5])      # the status word was cleared
    v = np.array([1.0, 2.0])
    Qs = np.outer(v, v)[None]                                 # rank 1: accepted by the IRF (zero column), refused by the decomposition
    got = ctx.irf_batch_host(st["Lam"], st["A"], Qs, st["R"], 4)
    e = se.irf_fevd(st["Lam"][0], st["A"][0], Qs[0], st["R"][0], 4)
    _close(got["irf"][0], e["irf"], "rank-deficient Q irf")
    assert np.all(got["irf"][0][1] == 0.0)
    with pytest.raises(_lib.DfmError) as ei:
        ctx.histdecomp_batch_host(x, st["Lam"], st["R"], st["A"], Qs, st["mu0"], st["P0"], singular_q=True)
    assert ei.value.code == -5
    ptr = lambda a: ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)
    out = np.empty((1, 3, 30, 20))
    lib = ctx._lib
    L, R, A, Q = (np.ascontiguousarray(st[k]) for k in ("Lam", "R", "A", "Q"))
    base = [ptr(L), ptr(A), ptr(Q), ptr(R), None]
    assert lib.dfm_irf_batch(ctx._h, 1, 20, 2, 1, 0, *base, None, None, ptr(out), None, 0) == -1          # H = 0
    rep = np.array([4, 4], dtype=np.int32)
    assert lib.dfm_irf_batch(ctx._h, 1, 20, 2, 1, 4, *base, ptr(rep), None, ptr(out), None, 0) == -1      # repeated named index
    assert lib.dfm_irf_batch(ctx._h, 1, 20, 2, 1, 4, *base, None, None, ptr(out), None, _lib.DFM_SV_UNIT_EFFECT) == -3
    assert lib.dfm_irf_batch(ctx._h, 1, 20, 2, 1, 4, *base, None, None, None, None, 0) == -3
    xs = np.ascontiguousarray(x[:, :1])
    hp = [ptr(xs), ptr(L), ptr(R), ptr(A), ptr(Q), ptr(st["mu0"]), ptr(st["P0"]), None, None, ptr(out), None, None, None]
    assert lib.dfm_histdecomp_batch(ctx._h, 1, 1, 20, 2, 1, *hp, 0) == -1                                  # T = p
    bad = x.copy(); bad[0, 5, 3] = np.nan
    with pytest.raises(_lib.DfmError) as ei:
        ctx.histdecomp_batch_host(bad, *P, may_have_missing=False)
    assert ei.value.code == -4                                # as the pass: DFM_E_MISSING
    ctx.histdecomp_batch_host(x, *P)                          # and the handle is fine afterwards


# ------------------------------------------------------------------------------------------------------------ the api
def _sw_model(lags):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, lags)


@pytest.mark.parametrize("lags", [1, 4])
def test_api_on_the_stock_watson_panel(ctx, lags):
    from dynamic_factor_models_amd import api
    m = _sw_model(lags)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=lags, ctx=ctx, nrep=8 if lags == 1 else 0, seed=11)
    ep = {k: v.copy() for k, v in m.em_params.items()}
    cols = api._forecast_inputs(m, m.lastperiod)[0]
    named = cols[se.greedy_named(ep["Lam"])]
    H, r, N = 10, 4, cols.size
    q = np.array([0.1, 0.5, 0.9])
    o = api.structural_irf(m, H, named=named, cumulate=cols[:20], unit_effect=True, quantiles=q if lags == 1 else None, ctx=ctx)
    assert np.array_equal(o["cols"], cols) and o["irf"].shape == (N, H, r) and o["fevd"].shape == (N, H, r + 1)
    assert np.abs(o["fevd"].sum(axis=2) - 1.0).max() <= 1e-12 and np.all(np.isfinite(o["irf"]))
    pos = np.array([int(np.nonzero(cols == i)[0][0]) for i in named])
    assert np.all(o["irf"][pos, 0, np.arange(r)] == 1.0)
    A = ep["Avar"] if lags > 1 else ep["A"]
    _, _, _, sd = api._forecast_inputs(m, m.lastperiod)
    cum = np.zeros(N, int); cum[:20] = 1
    e = se.irf_fevd(ep["Lam"], A, ep["Q"], ep["R"], H, sd=sd, named=pos, cum=cum, unit_effect=True)
    _close(o["irf"], e["irf"].transpose(2, 1, 0), "api irf")
    _close(o["fevd"], e["fevd"].transpose(2, 1, 0), "api fevd")
    if lags == 1:
        assert o["bands"].shape == (3, N, H, r) and np.all(np.isfinite(o["bands"]))
        assert np.all(np.diff(o["bands"], axis=0) >= 0.0)
        assert np.abs(o["bands"]).max() <= 100.0 * max(1.0, np.abs(o["irf"]).max())
    with pytest.raises(ValueError, match="named"):
        api.structural_irf(m, H, quantiles=q, ctx=ctx)
    hd = api.historical_decomposition(m, named=named, through=224, ctx=ctx)
    nrow = 224 - 3 + 1
    assert np.array_equal(hd["rows"], np.arange(3, 225)) and hd["contributions"].shape == (nrow, N, r + 1)
    assert hd["shocks"].shape == (nrow, r) and np.all(hd["shocks"][:lags] == 0.0)
    _close(hd["contributions"].sum(axis=2), sd * (hd["factor"] @ ep["Lam"].T), "api sum identity in data units")
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep), "the api changed m.em_params"
