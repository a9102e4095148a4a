"""The stream waves of the one-launch pass (pass_fused.hip) issue a ring block -- 4 panel rows x NDR pieces -- as ONE statement
(dfm_lds.h dma16_block_stream) off ONE running scalar pointer: advanced by four rows per block, formed anew only where the wave's
sequence of blocks moves to the next replicate, the clamp to a segment's last row only in the segment's last block.

What can go wrong is address code, not arithmetic: a row fetched from the wrong replicate, segment, block or slot, a piece at the
wrong offset or under the wrong lane mask, the repeated rows of a partial block.  The shapes are the small ones at which each of
these takes another form; every result goes against the CPU oracle at the tolerance of test_gpu_pass_fused.py (RTOL of
test_gpu_ks_pass.py) and bitwise against the route that shares the arithmetic (DFM_PF_WPARK=0: own weight loads), and the same
call twice on one handle compares bit for bit (a counted-wait slip shows on the first call only).

Layout per shape, from the library's own pass_fused_pick_* / pass_fused_supported (asserted below, so the table cannot go stale):
N = 258 and N = 512 lie past the one-launch pass (N <= 256: the 32 steps of the MFMA collapse) and take the two-launch pass --
their rows of three and four pieces never reach the block statement, which therefore exists for one and two pieces only.

The non-temporal and the plain DMA text: DFM_DMA_NT is read once per process and by the diagnostics build alone, so no test can
flip it between two calls.  The production rule (plain DMA for panels above 2 GiB) can: test_plain_dma_equals_nt_bitwise."""
import ctypes

import numpy as np
import pytest

from test_gpu_ks_pass import _batch, _compare, _ctx_with_env, _oracle, _run_dev

pytestmark = pytest.mark.gpu

# N: what it exercises (rowB = 8 N bytes per row, SB = the padded slot stride of pf_slot_bytes)
WIDTHS = {
    128: "one full piece; slot stride padded, SB != rowB",
    136: "second piece of 4 lanes",
    200: "SB = rowB, 36-lane second piece",
    258: "three pieces, clamped last MFMA step (two-launch pass: N > 256)",
    512: "four full pieces, padded stride (two-launch pass: N > 256)",
    10: "row of 80 B, unit of 8 rows",
}
# T: 9 = a single unit, 33 / 37 = a partial last block with 1 / 3 valid rows short of 4, 228 = many blocks, the park rows in play
LENGTHS = (9, 33, 37, 228)
# (N, T) -> (one-launch pass?, stream waves, b_t buffers, weight hand-over) as pass_fused_pick_* give them
LAYOUT = {
    (128, 9): (True, 1, 2, False), (128, 33): (True, 4, 2, False), (128, 37): (True, 4, 2, False), (128, 228): (True, 4, 2, True),
    (136, 9): (True, 1, 2, False), (136, 33): (True, 4, 2, False), (136, 37): (True, 4, 2, False), (136, 228): (True, 4, 2, True),
    (200, 9): (True, 1, 2, False), (200, 33): (True, 4, 2, False), (200, 37): (True, 4, 2, False), (200, 228): (True, 4, 2, True),
    (258, 9): (False, 1, 2, False), (258, 33): (False, 4, 2, False), (258, 37): (False, 4, 2, False), (258, 228): (False, 4, 2, False),
    (512, 9): (False, 1, 2, False), (512, 33): (False, 3, 2, False), (512, 37): (False, 3, 2, False), (512, 228): (False, 3, 1, False),
    (10, 9): (True, 1, 2, False), (10, 33): (True, 4, 2, True), (10, 37): (True, 4, 2, True), (10, 228): (True, 4, 2, True),
}
SHAPES = [pytest.param(N, T, id=f"N{N}-T{T}-" + ("fused-nsw%d-nbuf%d-wpark%d" % LAYOUT[N, T][1:] if LAYOUT[N, T][0] else "two-launch"))
          for N in WIDTHS for T in LENGTHS]


def _pick(T, N):
    from dynamic_factor_models_amd import _lib
    lib = _lib.load()
    sup, nsw = lib._ZN3dfm20pass_fused_supportedEiii, lib._ZN3dfm19pass_fused_pick_nswEiii
    nbuf, wpark = lib._ZN3dfm20pass_fused_pick_nbufEii, lib._ZN3dfm21pass_fused_pick_wparkEii
    sup.restype = wpark.restype = ctypes.c_bool
    return bool(sup(8, T, N)), int(nsw(T, N, 0)), int(nbuf(T, N)), bool(wpark(T, N))


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    """Two workgroups: B = 7 gives them 4 and 3 replicates, so the pointer is re-based three times and unevenly."""
    c = _ctx_with_env(DFM_NUM_CU=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2_off():
    c = _ctx_with_env(DFM_NUM_CU=2, DFM_PF_WPARK=0)
    yield c
    c.close()


_cache = {}


def _case(B, N, T):
    """Inputs and oracle results of one shape: generated once, shared, never modified.  Consecutive replicates OF A WORKGROUP
    (b, b + 2 on two CUs; every other pair on the default grid) differ grossly in scale -- Lam x 3, R x 0.5 -- so a row or a
    weight from the wrong replicate is an O(1) error."""
    key = (B, N, T)
    if key not in _cache:
        panel, st = _batch(B, N, T, 8, 0.0)
        st = {k: v.copy() for k, v in st.items()}
        odd = (np.arange(B) // 2) % 2 == 1
        st["Lam"][odd] *= 3.0
        st["R"][odd] *= 0.5
        _cache[key] = (panel, st, _oracle(panel, st))
    return _cache[key]


def _same(a, b, tag):
    for x, y, name in zip(a, b, ("f_smooth", "P_smooth", "loglik")):
        np.testing.assert_array_equal(x, y, err_msg=f"{name} {tag}")


def test_layout_table_is_the_librarys():
    for (N, T), want in LAYOUT.items():
        got = _pick(T, N)
        assert got[0] == want[0], (N, T)
        if want[0]:                      # (a shape the one-launch pass does not take has no layout; the diagnostics build's table
            assert got == want, (N, T)   #  set is larger and would pick other numbers for it)


@pytest.mark.parametrize("N,T", SHAPES)
def test_seven_replicates_on_two_workgroups(ctx2, ctx2_off, N, T):
    panel, st, ref = _case(7, N, T)
    first = _run_dev(ctx2, panel, st, may_have_missing=False)
    again = _run_dev(ctx2, panel, st, may_have_missing=False)
    off = _run_dev(ctx2_off, panel, st, may_have_missing=False)
    _compare(first, ref, f"first call N={N} T={T}")
    _same(first, again, f"the same call twice N={N} T={T}")
    _same(first, off, f"DFM_PF_WPARK=1 vs 0 N={N} T={T}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,T", SHAPES)
def test_default_grid(ctx, N, T, B):
    panel, st, ref = _case(B, N, T)
    first = _run_dev(ctx, panel, st, may_have_missing=False)
    _compare(first, ref, f"B={B} N={N} T={T}")
    _same(first, _run_dev(ctx, panel, st, may_have_missing=False), f"the same call twice B={B} N={N} T={T}")


def test_gross_scale_matters():
    """The scaling of _case changes the results far beyond the tolerance (else it would prove nothing)."""
    panel, st, ref = _case(7, 200, 33)
    _, plain = _batch(7, 200, 33, 8, 0.0)
    assert np.abs(ref[0][2:4] - _oracle(panel, plain)[0][2:4]).max() > 1e-3 * np.abs(ref[0]).max()


def test_plain_dma_equals_nt_bitwise(ctx):
    """The two straight-line texts of the block statement.  A batch whose panels exceed 2 GiB streams with the plain DMA, a smaller
    one with the non-temporal hint (stream_nt_hint); a replicate's results do not depend on the batch around it.  B = 2720 at the
    headline's N = 200, T = 500 is 2.18 GB; its first and last 64 replicates again as batches of their own must compare equal."""
    import torch
    B, T, N, r = 2720, 500, 200, 8
    assert B * T * N * 8 > 2 << 30
    panel, par = ctx.synth_panels(20160415, 0, B, T, N, r)
    big = ctx.ks_pass_batch(panel, *par, may_have_missing=False)
    torch.cuda.synchronize()
    for lo in (0, B - 64):
        sl = slice(lo, lo + 64)
        small = ctx.ks_pass_batch(panel[sl].contiguous(), *[p[sl].contiguous() for p in par], may_have_missing=False)
        torch.cuda.synchronize()
        for x, y, name in zip(big, small, ("f_smooth", "P_smooth", "loglik")):
            assert torch.equal(x[sl], y), f"{name} replicates {lo} .. {lo + 63}"
