"""The scan of the one-launch pass (pass_fused.hip, scan_reg) with its recurrences on the fp64 matrix pipe: one step of the
eight chunks of a wave is an 8 x 8 by 8 x 8 product (dfm_scan.h mm8), lane l of a wave holds component 4 (l / 8 % 2) + l / 16
of chunk l % 8.  Every result against the CPU oracle at the tolerances of test_gpu_ks_pass.py; under DFM_LIB=diag also against
the two-launch route (lane-group mat-vecs) at the tolerances of test_gpu_pass_fused.py.

What can go wrong is the arithmetic's geometry, so the shapes are the smallest that reach every case of it: chunk lengths
L = 1, 2, 4, 16 with the flips between them, fewer periods than transient steps plus chunks (idle columns), a partial top
chunk, the T = 512 limit; r < 8 (padded rows of a column); transients of 1-2 and of exactly 8 steps, and a replicate that
leaves for scan_seq between two that stay; one and three replicates; the E-step's E[f_0 | X]."""
import numpy as np
import pytest

from conftest import diag_only

from oracle import kalman_oracle as ko
from test_gpu_ks_pass import _batch, _compare, _ctx_with_env, _oracle, _run_dev, _slow_riccati
from test_gpu_pass_fused_onchip import ECAP, KEYS, _transient_len

pytestmark = pytest.mark.gpu

GEOM_T = [2, 3, 9, 32, 33, 64, 65, 257, 500, 512]
PAD_R = [5, 7, 8]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


_cache = {}


def _case(B, N, T, r):
    """Inputs and oracle results of one shape: generated once, shared, never modified."""
    key = (B, N, T, r)
    if key not in _cache:
        panel, st = _batch(B, N, T, r, 0.0)
        ref = _oracle(panel, st)
        assert all(np.all(np.isfinite(x)) for x in ref), key           # the oracle itself is finite for these seeds
        _cache[key] = (panel, st, ref)
    return _cache[key]


# ---- chunk geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", GEOM_T)
def test_chunk_geometry(ctx, T):
    panel, st, ref = _case(3, 16, T, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"T={T}")


# ---- rows i >= r of a column are not stored and do not reach the log-likelihood ------------------------------------------------
@pytest.mark.parametrize("r", PAD_R)
def test_state_padding(ctx, r):
    import torch
    B, N, T = 3, 40, 80
    panel, st, ref = _case(B, N, T, r)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # f_smooth as the middle of a larger buffer: a store of a padded row would land in the next period's row or past the end
    guard = torch.full((B * T * r + 64,), 7.25, dtype=torch.float64, device=dev)
    f = guard[32:32 + B * T * r].view(B, T, r)
    P = torch.empty((B, T, r * (r + 1) // 2), dtype=torch.float64, device=dev)
    ll = torch.empty((B,), dtype=torch.float64, device=dev)
    ctx.ks_pass_batch(t(panel), *[t(st[k]) for k in KEYS], may_have_missing=False, out=(f, P, ll))
    torch.cuda.synchronize()
    _compare((f.cpu().numpy(), P.cpu().numpy(), ll.cpu().numpy()), ref, f"r={r}")
    g = guard.cpu().numpy()
    assert np.all(g[:32] == 7.25) and np.all(g[32 + B * T * r:] == 7.25)


# ---- transient lengths ---------------------------------------------------------------------------------------------------------
def _steady_P0(Lam, R, A, Q):
    """P0 at the fixed point of the covariance recursion in the form the kernel iterates (dfm_cov8.h): it settles at once."""
    C = (Lam.T / R) @ Lam
    Om = np.eye(len(A))
    for _ in range(400):
        Om = np.linalg.inv(A @ np.linalg.inv(Om) @ A.T + Q) + C
        Om = 0.5 * (Om + Om.T)
    P = np.linalg.inv(Om)
    return 0.5 * (P + P.T)


_WG = 256                     # workgroups of the default grid: workgroup w scans replicates w, w + 256, w + 512 in this order


def _transient_batch():
    B, N, T, r = 516, 30, 50, 8
    fast = _slow_riccati(B, N, T, r, 0.3, 0.01, seed=21)
    for b in range(B):
        fast[1]["P0"][b] = _steady_P0(fast[1]["Lam"][b], fast[1]["R"][b], fast[1]["A"][b], fast[1]["Q"][b])
    seam = _slow_riccati(B, N, T, r, 0.4, 0.03, seed=22)          # E - 1 = 7 .. 10
    slow = _slow_riccati(B, N, T, r, 0.9, 1.0, seed=23)           # never settles within T: scan_seq
    kinds = [fast, seam, slow]
    which = np.arange(B) % 2
    which[0:4] = which[2 * _WG:2 * _WG + 4] = 0
    which[_WG:_WG + 4] = 2                                        # between replicates w and w + 512 of workgroups 0 .. 3
    panel = np.stack([kinds[which[b]][0][b] for b in range(B)])
    st = {k: np.stack([kinds[which[b]][1][k][b] for b in range(B)]) for k in KEYS}
    ts = np.array([_transient_len(st["Lam"][b], st["R"][b], st["A"][b], st["Q"][b], st["P0"][b], T) for b in range(B)])
    return panel, st, which, ts


def test_transient_lengths(ctx):
    panel, st, which, ts = _transient_batch()
    # (numpy rounds differently from the device, a replicate may land one step to either side: populations, not single replicates)
    assert (ts[which == 0] <= 2).sum() >= 200, np.bincount(ts[which == 0])
    assert (ts == ECAP).sum() >= 20 and (ts == ECAP - 1).sum() >= 20, np.bincount(ts[which == 1])
    for w in range(4):
        assert ts[w] <= ECAP - 1 and ts[w + _WG] >= ECAP + 2 and ts[w + 2 * _WG] <= ECAP - 1, (w, ts[w], ts[w + _WG], ts[w + 2 * _WG])
    ref = _oracle(panel, st)
    assert all(np.all(np.isfinite(x)) for x in ref)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, "transient lengths")
    _compare(_run_dev(ctx, panel, st, may_have_missing=False, want_P=False), ref, "transient lengths, no P")


# ---- batch edges; a stale register or LDS value shows on the second call only ------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_batch_edges_and_same_call_twice(ctx, B):
    panel, st, ref = _case(B, 16, 65, 8)
    first = _run_dev(ctx, panel, st, may_have_missing=False)
    second = _run_dev(ctx, panel, st, may_have_missing=False)
    _compare(first, ref, f"B={B}")
    for x, y in zip(first, second):
        np.testing.assert_array_equal(x, y)


# ---- EM: E[f_0 | X] comes out of the backward transient ------------------------------------------------------------------------
def test_two_em_iterations(ctx):
    import torch
    B, N, T, r = 4, 40, 80, 5
    panel, st = _batch(B, N, T, r, 0.0)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    par = {k: t(st[k]) for k in KEYS}
    path, its, f, P = ctx.em_batch(t(panel), *[par[k] for k in KEYS], max_iter=2, tol=0.0, may_have_missing=False)
    torch.cuda.synchronize()
    path = path.cpu().numpy(); f = f.cpu().numpy(); P = P.cpu().numpy()
    got = {k: par[k].cpu().numpy() for k in KEYS}
    assert np.all(its.cpu().numpy() == 2)
    for b in range(B):
        p, opath, out = ko.em(panel[b], {k: st[k][b] for k in KEYS}, max_iter=2, tol=0.0)
        assert np.all(np.isfinite(opath)) and all(np.all(np.isfinite(p[k])) for k in KEYS)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")     # (test_gpu_em.py's tolerance)
        for k in KEYS:                                                                          # mu0 is E[f_0 | X]
            assert np.abs(got[k][b] - p[k]).max() <= 1e-8 * max(1.0, np.abs(p[k]).max()), (k, b)
        assert np.abs(f[b] - out["f_smooth"]).max() <= 1e-8 * np.abs(out["f_smooth"]).max()
        assert np.abs(P[b] - ko.pack_sym(out["P_smooth"])).max() <= 1e-8 * np.abs(out["P_smooth"]).max()


# ---- diagnostics build: against the two-launch route (collapse launch + meanscan_kernel, lane-group mat-vecs) -----------------
def _against_two_launch(cases):
    one = _ctx_with_env(DFM_PASS_FUSED=1)
    two = _ctx_with_env(DFM_PASS_FUSED=0)
    try:
        for tag, panel, st in cases:
            f1, P1, l1 = _run_dev(one, panel, st, may_have_missing=False)
            f2, P2, l2 = _run_dev(two, panel, st, may_have_missing=False)
            np.testing.assert_allclose(l1, l2, rtol=1e-11, err_msg=tag)       # (test_gpu_pass_fused.py: cross-route tolerances)
            assert np.abs(f1 - f2).max() <= 1e-10 * np.abs(f2).max(), tag
            assert np.abs(P1 - P2).max() <= 1e-10 * np.abs(P2).max(), tag
    finally:
        one.close(); two.close()


@diag_only()
def test_chunk_geometry_against_two_launch():
    _against_two_launch([(f"T={T}",) + _case(3, 16, T, 8)[:2] for T in GEOM_T])


@diag_only()
def test_state_padding_against_two_launch():
    _against_two_launch([(f"r={r}",) + _case(3, 40, 80, r)[:2] for r in PAD_R])


@diag_only()
def test_transient_lengths_against_two_launch():
    panel, st, _, _ = _transient_batch()
    _against_two_launch([("transient lengths", panel, st)])
