"""The one-launch pass (pass_fused.hip) with the stream waves' weights handed over by the fill wave: W = lam / R and 1 / R of local
replicate j are parked in the highest rows of the b_t buffer that replicate j fills, the stream waves read them from LDS at the
replicate boundary (no drain of their DMA ring) and store b_t over the park once every wave has taken its values.  Every result
against the CPU oracle at the tolerances of test_gpu_ks_pass.py, and bitwise against the route without the hand-over
(DFM_PF_WPARK=0).

What can go wrong is protocol, not arithmetic: a park written before the scan has released the buffer, read before it is written,
or overwritten by a wave's b_t rows before another wave has read it.  At N = 24, T = 33 the park (3 x 64 + 24 doubles = 27 b_t
rows, rows 9 .. 35 of the buffer) overlaps the segments of all four stream waves (rows 0-11, 12-19, 20-27, 28-32), so the wait in
front of a wave's first store into the park runs in each of its forms: from the first block on, inside the segment, and -- wave 0
-- in its last block.  The route rule (pf_wpark_rule): two b_t buffers and 64 ceil(N / 8) + N <= 8 * 4 ceil(T / 4)."""
import numpy as np
import pytest

from conftest import diag_only

from oracle import kalman_oracle as ko
from test_gpu_ks_pass import RTOL, _batch, _compare, _ctx_with_env, _oracle, _run_dev

pytestmark = pytest.mark.gpu

KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")


def park_fits(T, N):
    """pf_wpark_rule of pass_fused.hip without its `two buffers` clause: the park fits below the b_t rows of one buffer."""
    return (N + 7) // 8 * 64 + N <= (T + 3) // 4 * 4 * 8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    """The route without the hand-over: every stream wave loads its own weights."""
    c = _ctx_with_env(DFM_PF_WPARK=0)
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


# ---- replicates per workgroup 1, 2, 3 and >= 5 (256 CUs: B = 3 / 257 / 600 / 1300), with and without P_smooth -----------------
@pytest.mark.parametrize("want_P", [True, False])
@pytest.mark.parametrize("r", [7, 8])
@pytest.mark.parametrize("B", [3, 257, 600, 1300])
def test_replicates_per_workgroup(ctx, B, r, want_P):
    assert park_fits(33, 24)
    panel, st, ref = _case(B, 24, 33, r)
    got = _run_dev(ctx, panel, st, may_have_missing=False, want_P=want_P)
    assert (got[1] is None) == (not want_P)
    _compare(got, ref, f"B={B} r={r} want_P={want_P}")


@pytest.mark.parametrize("want_P", [True, False])
@pytest.mark.parametrize("r", [7, 8])
def test_six_boundaries_per_workgroup(r, want_P):
    """Two workgroups (DFM_NUM_CU=2), B = 12: six replicates each, so every park is reused twice over."""
    panel, st, ref = _case(12, 24, 33, r)
    c = _ctx_with_env(DFM_NUM_CU=2)
    try:
        _compare(_run_dev(c, panel, st, may_have_missing=False, want_P=want_P), ref, f"2 CUs r={r} want_P={want_P}")
    finally:
        c.close()


# ---- weights that differ grossly between a workgroup's consecutive replicates ----------------------------------------------
def test_gross_weight_change_between_replicates(ctx):
    """Lam x 3 and R x 0.5 from replicate 256 on: workgroup w streams replicate w with one scale, w + 256 with the other and
    w + 512 with it again -- a stale or an early park is an O(1) error, not a rounding one."""
    B, N, T, r = 600, 24, 33, 8
    panel, st0, _ = _case(B, N, T, r)
    st = {k: v.copy() for k, v in st0.items()}
    st["Lam"][256:] *= 3.0
    st["R"][256:] *= 0.5
    ref = _oracle(panel, st)
    assert np.abs(ref[0][256:] - _case(B, N, T, r)[2][0][256:]).max() > 1e-3 * np.abs(ref[0]).max()   # the change matters
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, "gross weights")
    _compare(_run_dev(ctx, panel, st, may_have_missing=False, want_P=False), ref, "gross weights, no P")


# ---- both routes, bitwise --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,T", [(600, 24, 33), (515, 200, 228), (5, 130, 41)])
def test_routes_agree_bitwise(ctx, ctx_off, B, N, T):
    panel, st, ref = _case(B, N, T, 8)
    on = _run_dev(ctx, panel, st, may_have_missing=False)
    off = _run_dev(ctx_off, panel, st, may_have_missing=False)
    for x, y, name in zip(on, off, ("f_smooth", "P_smooth", "loglik")):
        np.testing.assert_array_equal(x, y, err_msg=f"{name} B={B} N={N} T={T}")
    _compare(on, ref, f"hand-over B={B} N={N} T={T}")
    _compare(off, ref, f"own loads B={B} N={N} T={T}")


# ---- the seam of the route rule --------------------------------------------------------------------------------------------
# the park fits from 8 * 4 ceil(T / 4) >= 64 ceil(N / 8) + N on: N = 200 -> 1800 doubles = 225 rows (T = 224 | 225), N = 256 ->
# 2304 doubles = 288 rows (T = 284 | 285)
SEAM = [(200, 224), (200, 225), (256, 284), (256, 285)]


def test_seam_shapes_sit_on_the_seam():
    for N, lo, hi in [(200, 224, 225), (256, 284, 285)]:
        assert not park_fits(lo, N) and park_fits(hi, N)


@pytest.mark.parametrize("N,T", SEAM)
def test_route_seam(ctx, N, T):
    panel, st, ref = _case(515, N, T, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"seam N={N} T={T} park={park_fits(T, N)}")


def test_three_stream_waves(ctx):
    """N = 256, T = 500: two b_t buffers fit the LDS with three rings only (pf_pick) -- the hand-over with three takers."""
    panel, st, ref = _case(515, 256, 500, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, "nsw = 3")


@pytest.mark.parametrize("T", [pytest.param(600, marks=diag_only("T > 512 takes the one-launch pass in the diagnostics build only"))])
def test_one_buffer(T):
    """N = 256, T = 600: one b_t buffer (pf_pick) -- no hand-over, whatever the switch says."""
    from dynamic_factor_models_amd import DfmContext
    panel, st, ref = _case(515, 256, T, 8)
    c = DfmContext()
    try:
        _compare(_run_dev(c, panel, st, may_have_missing=False), ref, "nbuf = 1")
    finally:
        c.close()


# ---- short and odd panels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 3, 7, 9])
def test_short_panels(ctx, T):
    panel, st, ref = _case(515, 24, T, 8)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"T={T} park={park_fits(T, 24)}")


@pytest.mark.parametrize("N", [10, 38, 202, 2])
def test_clamped_last_step(ctx, N):
    """N no multiple of 8: the last MFMA step is clamped for some lanes (weight 0), N = 2: for all but two."""
    panel, st, ref = _case(515, N, 33, 8 if N > 2 else 2)
    _compare(_run_dev(ctx, panel, st, may_have_missing=False), ref, f"N={N} park={park_fits(33, N)}")


# ---- EM ----------------------------------------------------------------------------------------------------------------------
def test_two_em_iterations(ctx):
    import torch
    B, N, T, r = 300, 30, 50, 8
    assert park_fits(T, N)
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


# ---- no stale park: one handle, changing calls; the same call twice --------------------------------------------------------
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
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
