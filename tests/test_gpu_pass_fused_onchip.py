"""The one-launch pass (pass_fused.hip) with the covariance tables handed to the scan on chip and the panel streamed in whole
row blocks: every result against the CPU oracle at the tolerances of test_gpu_ks_pass.py.

What can go wrong here is protocol, not arithmetic: two covariance waves take turns writing ONE LDS table set that the scan of
the previous replicate must have released, so the cases below vary the number of replicates per workgroup (1, 2, 3, >= 5; a
workgroup per CU, replicates b, b + CUs, ...), mix the scan routes that consume the set (scan_reg for a Riccati transient of
E - 1 <= 8 steps, scan_seq + the global overflow table beyond), and cut the T periods into stream segments at every shape
where the cut changes (row sizes whose 128-byte period is 2, 8 or 16 rows, T around the block and segment boundaries)."""
import numpy as np
import pytest

from conftest import diag_only

from oracle import kalman_oracle as ko
from test_gpu_ks_pass import _batch, _compare, _ctx_with_env, _oracle, _run_dev, _slow_riccati

pytestmark = pytest.mark.gpu

KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
STEADY_TOL = 4.5e-16          # kSteadyTol (csrc/dfm_smallmat.h)
ECAP = 8                      # transient steps staged on chip (kPfEcap)


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
        _cache[key] = (panel, st, _oracle(panel, st))
    return _cache[key]


def _transient_len(Lam, R, A, Q, P0, T):
    """E - 1 of one replicate: the forward covariance recursion of the balanced path in the information form the kernel uses
    (dfm_cov8.h), stopped where successive Om_f agree to STEADY_TOL.  numpy rounds differently from the device, so a replicate
    at the edge of the tolerance may land one step to either side; the tests below only count populations."""
    C = (Lam.T / R) @ Lam
    Qi = np.linalg.inv(Q)
    PsiT = Qi @ A
    Phi = A.T @ PsiT
    Om = np.linalg.inv(P0)
    for e in range(T):
        Z = np.linalg.inv(Om + Phi)
        new = (Qi - PsiT @ (Z @ PsiT.T)) + C
        same = bool(np.all(np.abs(new - Om) <= STEADY_TOL * np.abs(Om)))
        Om = new
        if same or e + 1 >= T:
            return e
    return T - 1


# ---- replicates per workgroup 1, 2, 3 and >= 5 (256 CUs: B = 3 / 257 / 600 / 1300), with and without P_smooth -----------------
@pytest.mark.parametrize("want_P", [True, False])
@pytest.mark.parametrize("r", [7, 8])
@pytest.mark.parametrize("B", [3, 257, 600, 1300])
def test_replicates_per_workgroup(ctx, B, r, want_P):
    panel, st, ref = _case(B, 24, 33, r)
    got = _run_dev(ctx, panel, st, may_have_missing=False, want_P=want_P)
    assert (got[1] is None) == (not want_P)
    _compare(got, ref, f"B={B} r={r} want_P={want_P}")


def test_two_em_iterations(ctx):
    """SP11 / SU / P0s and the global copy of P_T that the EM update reads, two replicates on some workgroups."""
    import torch
    B, N, T, r = 300, 30, 50, 8
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
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")     # (test_gpu_em.py's tolerance)
        for k in KEYS:
            assert np.abs(got[k][b] - p[k]).max() <= 1e-8 * max(1.0, np.abs(p[k]).max()), (k, b)
        assert np.abs(f[b] - out["f_smooth"]).max() <= 1e-8 * np.abs(out["f_smooth"]).max()
        assert np.abs(P[b] - ko.pack_sym(out["P_smooth"])).max() <= 1e-8 * np.abs(out["P_smooth"]).max()


# ---- transient lengths at the seam between scan_reg (tables on chip) and scan_seq (overflow table in global memory) --------
def _mixed_batch(B, N, T, r):
    """Replicates of three kinds -- a short transient, one around E - 1 = 8, a long one -- ordered so that every workgroup
    (replicates b, b + 256, b + 512) meets all three, in an order that differs between workgroups."""
    kinds = [_slow_riccati(B, N, T, r, 0.3, 0.01, seed=21),      # E - 1 = 5 .. 7
             _slow_riccati(B, N, T, r, 0.4, 0.03, seed=22),      # E - 1 = 7 .. 10: both sides of the seam, and the seam
             _slow_riccati(B, N, T, r, 0.9, 1.0, seed=23)]       # never settles within T: E = T
    which = (np.arange(B) // 256 + np.arange(B)) % 3
    panel = np.stack([kinds[which[b]][0][b] for b in range(B)])
    st = {k: np.stack([kinds[which[b]][1][k][b] for b in range(B)]) for k in KEYS}
    return panel, st, which


def test_transient_lengths_at_the_seam(ctx):
    B, N, T, r = 520, 24, 33, 8
    panel, st, which = _mixed_batch(B, N, T, r)
    ts = np.array([_transient_len(st["Lam"][b], st["R"][b], st["A"][b], st["Q"][b], st["P0"][b], T) for b in range(B)])
    # both sides of the seam and the seam itself occur, well beyond the one step numpy may differ from the device by
    assert (ts <= ECAP - 1).sum() >= 50 and (ts == ECAP).sum() >= 20 and (ts == ECAP + 1).sum() >= 20 and (ts >= ECAP + 2).sum() >= 50, \
        np.bincount(ts)
    # ... and inside one workgroup consecutive scans take different routes
    # (a workgroup per CU, 256 of them: workgroup w scans replicates w, w + 256, w + 512 in this order)
    clear = (ts <= ECAP - 1) | (ts >= ECAP + 2)
    assert sum(1 for w in range(256) if clear[w] and clear[w + 256] and (ts[w] > ECAP) != (ts[w + 256] > ECAP)) >= 64
    assert sum(1 for w in range(B - 512) if len({ts[w] > ECAP, ts[w + 256] > ECAP, ts[w + 512] > ECAP}) == 2) >= 4
    ref = _oracle(panel, st)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, "mixed transient lengths")
    _compare(_run_dev(ctx, panel, st, may_have_missing=False, want_P=False), ref, "mixed transient lengths, no P")


# ---- panels shorter than the transient -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 3, 7])
def test_short_panels(ctx, T):
    panel, st, ref = _case(515, 24, T, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"T={T}")


# ---- the segment cut -------------------------------------------------------------------------------------------------------
CUT_T = [500, 33, 37, 41, 42, 43, 5, 9]
CUT_N = [24, 38, 130, 200]


@pytest.mark.parametrize("N", CUT_N)
@pytest.mark.parametrize("T", CUT_T)
def test_segment_cut(ctx, T, N):
    B = 3 if T == 500 else 5
    panel, st, ref = _case(B, N, T, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"cut T={T} N={N}")


@pytest.mark.parametrize("nsw", [pytest.param(n, marks=diag_only()) for n in (1, 3, 5)])
def test_segment_cut_other_wave_counts(nsw):
    c = _ctx_with_env(DFM_PASS_NSW=nsw)
    try:
        for T in CUT_T:
            for N in CUT_N:
                panel, st, ref = _case(3 if T == 500 else 5, N, T, 8)
                _compare(_run_dev(c, panel, st, may_have_missing=False), ref, f"nsw={nsw} cut T={T} N={N}")
    finally:
        c.close()


# ---- no stale table: one handle, changing calls; the same call twice -------------------------------------------------------
def test_one_handle_changing_calls(ctx):
    big = _case(600, 24, 33, 8)
    small = _case(5, 24, 33, 7)
    first = _run_dev(ctx, big[0], big[1], may_have_missing=False)
    _compare(first, big[2], "B=600, first")
    _compare(_run_dev(ctx, small[0], small[1], may_have_missing=False), small[2], "B=5 in between")
    third = _run_dev(ctx, big[0], big[1], may_have_missing=False)
    for x, y in zip(first, third):
        np.testing.assert_array_equal(x, y)


def test_deterministic(ctx):
    panel, st, ref = _case(600, 24, 33, 8)
    a = _run_dev(ctx, panel, st, may_have_missing=False)
    b = _run_dev(ctx, panel, st, may_have_missing=False)
    _compare(a, ref, "B=600")
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
