"""Randomised shape sweep of the balanced fast path and of EM (seeded): every kernel choice the dispatcher can make
-- MFMA / VALU / wide collapse, fused and separate covariance launches, 1..8 period segments per replicate, padded r,
ragged T -- against the CPU oracle."""
import numpy as np
import pytest

from conftest import diag_only

from oracle import c_oracle as co
from oracle import kalman_oracle as ko

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _shapes(seed, n):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = int(g.integers(1, 13))
        N = int(g.integers(max(4, r + 2), 260))
        if g.random() < 0.7:
            N += N & 1                                   # mostly even (MFMA / DMA kernels), some odd (wide kernel)
        T = int(g.integers(3, 140))
        B = int(g.integers(1, 12))
        out.append((B, N, T, r))
    return out


@pytest.mark.parametrize("B,N,T,r", _shapes(20160415, 28))
def test_random_balanced_pass(ctx, B, N, T, r):
    import torch
    reps = [ko.synth_replicate(b, N, T, r, seed=ko.SEED0 + 31 * N + T) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    st = {k: np.stack([p[k] for _, p in reps]) for k in reps[0][1]}
    if not np.isfinite(panel).all():
        pytest.skip("degenerate standardisation")
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f, P, ll = ctx.ks_pass_batch(t(panel), t(st["Lam"]), t(st["R"]), t(st["A"]), t(st["Q"]), t(st["mu0"]), t(st["P0"]),
                                 may_have_missing=False)
    torch.cuda.synchronize()
    fo, Po, llo = co.ks_pass_batch(panel, st["Lam"], st["R"], st["A"], st["Q"], st["mu0"], st["P0"])
    np.testing.assert_allclose(ll.cpu().numpy(), llo, rtol=RTOL)
    assert np.abs(f.cpu().numpy() - fo).max() <= RTOL * np.abs(fo).max()
    assert np.abs(P.cpu().numpy() - Po).max() <= RTOL * np.abs(Po).max()


def _shapes32(seed, n):
    """r = 17 .. 32 (state padded to 32): the streaming collapse of config 4 (persistent workgroups, tiles of 128 periods,
    stages of 32 series, 1 .. 4 column groups past the first 16), the matrix-pipe scan (128 chunks), and -- with missing
    cells -- their variants for NaN panels plus the C_t kernel (N > 256) or collapse_kernel (N <= 256)."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        r = int(g.integers(17, 33))
        N = int(g.integers(r + 2, 700))
        if g.random() < 0.8:
            N += N & 1                                   # mostly even (LDS-DMA kernels), some odd (8-byte-load kernels)
        T = int(g.integers(3, 330))
        B = int(g.integers(1, 20))
        miss = float(g.choice([0.0, 0.0, 0.05, 0.3]))
        out.append((B, N, T, r, miss))
    return out


@pytest.mark.parametrize("B,N,T,r,miss", _shapes32(32, 16))
def test_random_wide_state_pass(ctx, B, N, T, r, miss):
    import torch
    reps = [ko.synth_replicate(b, N, T, r, seed=ko.SEED0 + 13 * N + T, missing=miss) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    st = {k: np.stack([p[k] for _, p in reps]) for k in reps[0][1]}
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f, P, ll = ctx.ks_pass_batch(t(panel), t(st["Lam"]), t(st["R"]), t(st["A"]), t(st["Q"]), t(st["mu0"]), t(st["P0"]),
                                 may_have_missing=miss > 0)
    torch.cuda.synchronize()
    fo, Po, llo = co.ks_pass_batch(panel, st["Lam"], st["R"], st["A"], st["Q"], st["mu0"], st["P0"])
    np.testing.assert_allclose(ll.cpu().numpy(), llo, rtol=RTOL)
    assert np.abs(f.cpu().numpy() - fo).max() <= RTOL * np.abs(fo).max()
    assert np.abs(P.cpu().numpy() - Po).max() <= RTOL * np.abs(Po).max()


@pytest.mark.parametrize("B,N,T,r", _shapes(7, 10))
def test_random_balanced_em(ctx, B, N, T, r):
    import torch
    if T < 3 * r + 4 or N < 2 * r + 2:
        # the PCA start fits a VAR(1) on T-1 pairs: with T-1 < 2r its residual covariance Q is singular, and the
        # information-form recursion needs Q^-1 (DESIGN.md "known limits"; test_singular_Q_is_reported below)
        pytest.skip("too few periods for a positive definite PCA start")
    reps = [ko.synth_replicate(b, N, T, r, seed=ko.SEED0 + 17 * N + T) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    if not np.isfinite(panel).all():
        pytest.skip("degenerate standardisation")
    starts = [ko.pca_init(panel[b], r)[0] for b in range(B)]
    keys = ("Lam", "R", "A", "Q", "mu0", "P0")
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: t(np.stack([s[k] for s in starts])) for k in keys}
    path, its, f, P = ctx.em_batch(t(panel), *[d[k] for k in keys], max_iter=3, tol=0.0)
    torch.cuda.synchronize()
    for b in range(B):
        p, opath, out = ko.em(panel[b], starts[b], max_iter=3, tol=0.0)
        np.testing.assert_allclose(path[b].cpu().numpy(), opath, rtol=1e-8)
        for k in keys:
            got = d[k][b].cpu().numpy()
            assert np.abs(got - p[k]).max() <= 1e-8 * max(1.0, np.abs(p[k]).max()), (k, b)


def test_singular_Q_is_reported(ctx):
    """T-1 < 2r: the PCA start's Q is rank deficient.  The covariance-form oracle still runs; the information-form
    HIP path cannot, and the synchronising host entry point must say so (DFM_E_NUMERIC), not hand back numbers."""
    from dynamic_factor_models_amd._lib import DfmError
    B, N, T, r = 1, 52, 18, 11
    x, _ = ko.synth_replicate(0, N, T, r, seed=ko.SEED0 + 17 * N + T)
    start = ko.pca_init(x, r)[0]
    assert np.linalg.matrix_rank(start["Q"], tol=1e-10) < r
    with pytest.raises(DfmError) as e:
        ctx.ks_pass_batch_host(x[None], *[start[k][None] for k in ("Lam", "R", "A", "Q", "mu0", "P0")])
    assert e.value.code == -5


@diag_only()
@pytest.mark.parametrize("r", [3, 8])
def test_lane_group_recursion_kernel_still_matches(r, monkeypatch):
    """DFM_NO_RECURSION_WAVE=1: the r-lanes-per-replicate recursion_kernel (what large batches and r > 8 use) on the
    shapes the default dispatch now gives to the wave-per-replicate kernel."""
    import torch
    from dynamic_factor_models_amd import DfmContext
    monkeypatch.setenv("DFM_NO_RECURSION_WAVE", "1")
    c = DfmContext()
    try:
        B, N, T = 3, 40, 60
        reps = [ko.synth_replicate(b, N, T, r, missing=0.1) for b in range(B)]
        x = np.stack([a for a, _ in reps])
        st = {k: np.stack([p[k] for _, p in reps]) for k in reps[0][1]}
        keys = ("Lam", "R", "A", "Q", "mu0", "P0")
        dev = torch.device("cuda", c.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        f, P, ll = c.ks_pass_batch(t(x), *[t(st[k]) for k in keys])
        d = {k: t(st[k]) for k in keys}
        path, its, f2, P2 = c.em_batch(t(x), *[d[k] for k in keys], max_iter=3, tol=0.0)
        torch.cuda.synchronize()
        for b in range(B):
            o = ko.kfs_pass(x[b], **reps[b][1])
            assert abs(ll[b].item() - o["loglik"]) <= RTOL * abs(o["loglik"])
            assert np.abs(f[b].cpu().numpy() - o["f_smooth"]).max() <= RTOL * np.abs(o["f_smooth"]).max()
            p, opath, _ = ko.em(x[b], reps[b][1], 3)
            np.testing.assert_allclose(path[b].cpu().numpy(), opath, rtol=1e-8)
            assert np.abs(d["Lam"][b].cpu().numpy() - p["Lam"]).max() <= 1e-8 * np.abs(p["Lam"]).max()
    finally:
        c.close()
        monkeypatch.delenv("DFM_NO_RECURSION_WAVE")
        DfmContext().close()              # resets the process-wide dispatch default


@pytest.mark.parametrize("B,N,T,r,why", [(2, 30, 1300, 6, "long panel on the wave kernel (LDS period index)"),
                                         (4100, 12, 20, 5, "B > 4096: lane-group kernel at Rp = 8"),
                                         (1600, 10, 15, 3, "B > 1536: no widening of r <= 4"),
                                         (2, 24, 40, 20, "Rp = 32 information form on Grid<32>")])
def test_dispatch_edges_of_the_sequential_path(ctx, B, N, T, r, why):
    import torch
    nchk = min(B, 3)
    reps = [ko.synth_replicate(b % nchk, N, T, r, missing=0.1) for b in range(nchk)]
    idx = np.arange(B) % nchk
    x = np.stack([reps[k][0] for k in idx])
    st = {k: np.stack([reps[q][1][k] for q in idx]) for k in reps[0][1]}
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f, P, ll = ctx.ks_pass_batch(t(x), *[t(st[k]) for k in ("Lam", "R", "A", "Q", "mu0", "P0")])
    torch.cuda.synchronize()
    for b in list(range(nchk)) + [B - 1]:
        o = ko.kfs_pass(x[b], **reps[idx[b]][1])
        assert abs(ll[b].item() - o["loglik"]) <= RTOL * abs(o["loglik"]), why
        assert np.abs(f[b].cpu().numpy() - o["f_smooth"]).max() <= 1e-8 * max(1.0, np.abs(o["f_smooth"]).max()), why


def test_companion_state_32_wide_with_large_lds(ctx):
    """r = 8, VAR(4), T = 760: Grid<32> with more than 64 KB of dynamic LDS (tiles + period index: 62 528 + 4 T bytes, the opt-in of
    launch_wave_cov_ch is first taken at T = 753; tests/test_gpu_varp_routes.py runs both sides of that edge)."""
    import torch
    from oracle import varp_oracle as vo
    B, N, T, r, p = 2, 40, 760, 8, 4
    keys = ("Lam", "R", "Avar", "Q", "mu0", "P0")
    xs = [vo.synth_varp(b, N, T, r, p, missing=0.05) for b in range(B)]
    qs = [vo.varp_init(np.nan_to_num(x), r, p)[0] for x in xs]
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f, P, ll = ctx.ks_pass_varp_batch(t(np.stack(xs)), *[t(np.stack([q[k] for q in qs])) for k in keys])
    torch.cuda.synchronize()
    for b in range(B):
        o = vo.kfs_pass_varp(xs[b], p=p, **qs[b])
        assert abs(ll[b].item() - o["loglik"]) <= 1e-8 * abs(o["loglik"])
        assert np.abs(f[b].cpu().numpy() - o["f_smooth"][:, :r]).max() <= 1e-7 * np.abs(o["f_smooth"]).max()
