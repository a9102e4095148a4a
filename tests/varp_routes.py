"""Case table of tests/test_gpu_varp_routes.py: the VAR(p) companion pass and EM (dfm_ks_pass_varp_batch / dfm_em_varp_batch) on
every route launch_recursion (csrc/recursion.hip) can take for them.  Test infrastructure only, no GPU code.

varp_run (csrc/capi.hip) plans a companion state of width k = r p <= 32 in covariance form: Rp = pad_r(k), loadings Rc = pad_r(r)
wide on the first block, rl = r.  launch_recursion then asks recursion_comp_supported, recursion_mbf16_supported and
recursion_wave_supported in that order and falls back to the lane-group recursion_kernel<Rp, true>.  `route` restates that
(the C++ stays the authority; tests/test_varp_routes_cpu.py pins the restatement to the strings and numbers the sources state) and
`classes` names what a row reaches:

  lane<2> lane<4> [lane<4> r=4]                 recursion_kernel<Rp, true>, k <= 4
  wave<8> Rc=2|4|8 [k=8 r<=2] [CH8=4]           recursion_wave_kernel<8, COV>, k = 5..8; CH8 = 4 beyond one wave per SIMD
  mbf16<2> mbf16<4> [mbf16<4> singular]         recursion_mbf16_kernel, k = 9..16 with r <= 4 that comp does not take
  comp Rp=16 | 32                               recursion_comp_kernel, r = 4 with k a multiple of 4, Q of full rank
  wave<16> Rc=8|16                              recursion_wave_kernel<16, COV>, k = 9..16 with r >= 5
  wave<32> Rc=2|4|8|16|32 [singular r=4]        recursion_wave_kernel<32, COV>, k = 17..32 except r = 4
  wave<32> lds<=64K | lds>64K                   the two sides of launch_wave_cov_ch's opt-in edge (T = 752 | 753 at Rp = 32)
  lane<16> lane<32>                             the fallback beyond the LDS cap (handles without the wave kernels: wave=False)

Shapes (B = 2 unless the row says otherwise): even N = max(2 r, 12) for the "balanced" variant (no NaN, may_have_missing=False: the
Cfull branch), odd N = max(2 r, 12) + 1 for the "missing" variant (15 % missing cells, periods 0, 5 and T - 1 without an
observation) -- at Rc = 8 the collapse is collapse_miss_kernel for even N <= 224 and collapse_kernel<8> otherwise, at Rc <= 4 odd N
goes through odd_pad.  T = k + p + 3 r + 12: shorter panels make the EM's Q singular at r >= 16 (the start needs T - p - k well
above r).  Panels from varp_oracle.synth_varp, starts from varp_oracle.varp_init.

Every reference is computed once per process (functools.lru_cache) and must not be modified by its users."""
import collections
import functools

import numpy as np

from oracle import varp_oracle as vo

KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
EM_ITERS = 3
MISS_SHARE = 0.15
VARIANTS = ("balanced", "missing")

# ------------------------------------------------------------------------------------------------ dispatch restated
K_LANE, K_WAVE, K_MBF16, K_COMP = "recursion_kernel", "recursion_wave_kernel", "recursion_mbf16_kernel", "recursion_comp_kernel"
DFM_MAX_R = 32
LDS_CAP = 150 * 1024                 # recursion_wave_supported: `cap = 150 * 1024`
LDS_OPT_IN = 64 * 1024               # launch_wave_cov_ch: `lds > 64 * 1024` asks for the larger dynamic LDS first
LDS_WAVE8 = 60 * 1024                # recursion_wave_supported at Rp = 8
MI355X_CU = 256


def pow2_ge(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def pad_r(n):
    """capi.hip pad_r: the power of two >= n, at least 2."""
    return max(2, pow2_ge(n))


def tile_stride(R):
    """dfm_grid.h kTileStride<R>."""
    return R + 2


def grid_prow(R):
    """dfm_grid.h kGridProw<R>."""
    return 2 * (4 * R + 4)


def wave_lds_bytes(R, T):
    """recursion_wave.hip wave_lds_bytes<R>(T): four tiles, the grid's exchange rows at R >= 16, one int per period."""
    RT = R * tile_stride(R)
    extra = grid_prow(R) + 2 * (R * R // 64) * R + 2 * RT if R >= 16 else 0
    return (4 * RT + extra) * 8 + 4 * T


Route = collections.namedtuple("Route", "kernel instance Rp Rc rl lds")


def route(r, p, singular_q=False, wave=True, T=100, B=2, num_cu=MI355X_CU):
    """The recursion kernel of a VAR(p) call: its name as note_kernel records it (recursion_kernel is the profile's default name of
    the launch), the template instance, the plan's widths, the dynamic LDS of the wave kernels (None elsewhere)."""
    k = r * p
    assert 1 <= r and 1 <= p and k <= DFM_MAX_R, (r, p)           # varp_run: DFM_E_R_UNSUPPORTED beyond
    Rp, Rc, rl = pad_r(k), pad_r(r), r                            # make_plan(k) + Companion{Rc = pad_r(r), rl = r, kdim = k, kb = 0}
    lane = Route(K_LANE, f"recursion_kernel<{Rp}, true>", Rp, Rc, rl, None)
    if not wave:                                                  # RouteOpts::no_rec_wave: RecursionArgs::wave = 0
        return lane
    # recursion_comp_supported: Rp = 16 | 32, 8 <= kdim <= Rp in blocks of 4, loadings exactly 4 wide, Q of full rank
    if Rp in (16, 32) and 8 <= k <= Rp and k % 4 == 0 and not (k <= Rp // 2 and Rp == 32) and Rc == 4 and rl == 4 and not singular_q:
        return Route(K_COMP, f"recursion_comp_kernel<{Rp // 16}, true>", Rp, Rc, rl, None)
    # recursion_mbf16_supported: Rp = 16, loadings 2 | 4 wide
    if Rp == 16 and Rc in (2, 4) and 1 <= rl <= Rc:
        return Route(K_MBF16, f"recursion_mbf16_kernel<{Rc}>", Rp, Rc, rl, None)
    # (recursion_chunk_supported, recursion_tile_supported, recursion_pair_supported: information form only)
    # recursion_wave_supported
    lds = wave_lds_bytes(Rp, T) if Rp >= 8 else None
    if Rp in (16, 32):
        ok = lds <= LDS_CAP
    else:
        ok = Rp == 8 and lds <= LDS_WAVE8                         # (the batch bound DFM_WAVE_BMAX applies to Rc = 0 only)
    if not ok:
        return lane
    ch8 = 4 if Rp == 8 and B > 4 * num_cu else 8                  # launch_wave_cov: B > multiProcessorCount * 4
    return Route(K_WAVE, f"recursion_wave_kernel<{Rp}, true, {ch8}>", Rp, Rc, rl, lds)


def classes(r, p, singular_q=False, wave=True, T=100, B=2, num_cu=MI355X_CU):
    """The route classes (module docstring) one call reaches."""
    rt = route(r, p, singular_q, wave, T, B, num_cu)
    k = r * p
    if rt.kernel == K_LANE:
        out = {f"lane<{rt.Rp}>"}
        if rt.Rp == 4 and r == 4:
            out.add("lane<4> r=4")
    elif rt.kernel == K_COMP:
        out = {f"comp Rp={rt.Rp}"}
    elif rt.kernel == K_MBF16:
        out = {f"mbf16<{rt.Rc}>"}
        if singular_q:
            out.add(f"mbf16<{rt.Rc}> singular")
    else:
        out = {f"wave<{rt.Rp}> Rc={rt.Rc}"}
        if rt.Rp == 8 and k == 8 and r <= 2:
            out.add("wave<8> k=8 r<=2")
        if rt.instance.endswith(", 4>"):
            out.add("wave<8> CH8=4")
        if singular_q and r == 4:
            out.add(f"wave<{rt.Rp}> singular r=4")
        if rt.Rp == 32 and LDS_OPT_IN - 4 < rt.lds <= LDS_OPT_IN:
            out.add("wave<32> lds<=64K")                            # the last T below the opt-in
        if rt.Rp == 32 and LDS_OPT_IN < rt.lds <= LDS_OPT_IN + 4:
            out.add("wave<32> lds>64K")                             # the first T that takes it
    return out


REQUIRED = {
    "lane<2>", "lane<4>", "lane<4> r=4",
    "wave<8> Rc=2", "wave<8> Rc=8", "wave<8> k=8 r<=2", "wave<8> CH8=4",
    "mbf16<2>", "mbf16<4>", "mbf16<4> singular",
    "comp Rp=16", "comp Rp=32",
    "wave<16> Rc=8", "wave<16> Rc=16",
    "wave<32> Rc=2", "wave<32> Rc=4", "wave<32> Rc=8", "wave<32> Rc=16", "wave<32> Rc=32", "wave<32> singular r=4",
    "wave<32> lds<=64K", "wave<32> lds>64K",
}
REQUIRED_DIAG = {"lane<16>", "lane<32>"}                            # handles created under DFM_NO_RECURSION_WAVE=1

# ------------------------------------------------------------------------------------------------ the rows
Row = collections.namedtuple("Row", "name r p singular N T B cls why")


def _row(r, p, cls, why, singular=False, N=None, T=None, B=2, tag=""):
    return Row(f"r{r}p{p}{tag}", r, p, singular, N, T, B, cls, why)


BATCH_EDGE = "r2p3-batch"
ROWS = [
    # lane groups, k <= 4
    _row(1, 1, "lane<2>", "Rp = 2, the narrowest state"),
    _row(1, 2, "lane<2>", "Rp = 2 filled by a companion state: one shift row"),
    _row(4, 1, "lane<4> r=4", "Rp = Rc = rl = 4: no padding anywhere"),
    # recursion_wave_kernel<8, COV>
    _row(1, 8, "wave<8> k=8 r<=2", "k = Rp = 8 at Rc = 2: seven shift rows, one padded loading"),
    _row(2, 4, "wave<8> k=8 r<=2", "k = Rp = 8 at Rc = 2, loadings fill Rc"),
    _row(5, 1, "wave<8> Rc=8", "Rc = 8 with rl = 5: narrow S11 at Rc = Rp"),
    _row(8, 1, "wave<8> Rc=8", "Rc = rl = k = 8"),
    # recursion_wave_kernel<16, COV>
    _row(5, 2, "wave<16> Rc=8", "the first r past mbf16's domain"),
    _row(8, 2, "wave<16> Rc=8", "k = Rp = 16, rl = Rc = 8"),
    _row(5, 3, "wave<16> Rc=8", "k = 15: one padding state"),
    _row(9, 1, "wave<16> Rc=16", "k = rl = 9, Rc = Rp = 16"),
    _row(12, 1, "wave<16> Rc=16", ""),
    _row(16, 1, "wave<16> Rc=16", "k = rl = Rc = Rp = 16"),
    # recursion_comp_kernel at Rp = 32
    _row(4, 5, "comp Rp=32", "k = 20: the first state of the two-tile instance"),
    _row(4, 6, "comp Rp=32", "k = 24"),
    _row(4, 8, "comp Rp=32", "k = Rp = 32"),
    # recursion_wave_kernel<32, COV>
    _row(1, 17, "wave<32> Rc=2", "k = 17, one factor"),
    _row(1, 32, "wave<32> Rc=2", "k = Rp = 32, 31 shift rows"),
    _row(2, 16, "wave<32> Rc=2", "k = Rp = 32, loadings fill Rc = 2"),
    _row(3, 6, "wave<32> Rc=4", "k = 18, rl = 3 < Rc"),
    _row(3, 10, "wave<32> Rc=4", "k = 30"),
    _row(5, 4, "wave<32> Rc=8", "k = 20, rl = 5"),
    _row(7, 4, "wave<32> Rc=8", "k = 28, rl = 7"),
    _row(9, 2, "wave<32> Rc=16", "k = 18, rl = 9"),
    _row(16, 2, "wave<32> Rc=16", "k = Rp = 32, rl = Rc = 16"),
    _row(10, 3, "wave<32> Rc=16", "k = 30, rl = 10"),
    _row(17, 1, "wave<32> Rc=32", "k = rl = 17"),
    _row(32, 1, "wave<32> Rc=32", "k = rl = Rc = Rp = 32 = DFM_MAX_R"),
    # singular Q at r = 4 (rank 3, as test_gpu_varp.py::test_rank_deficient_innovation_block_at_r4 makes it)
    _row(4, 4, "mbf16<4> singular", "comp refuses a singular Q", singular=True, tag="-sing"),
    _row(4, 5, "wave<32> singular r=4", "comp refuses a singular Q, mbf16 ends at k = 16", singular=True, tag="-sing"),
    # the routes tests/test_gpu_varp.py grew up with, one row each: the diagnostics handles below rerun them on the lane groups
    _row(4, 4, "comp Rp=16", "the reference's default lags at r = 4"),
    _row(2, 6, "mbf16<2>", "k = 12 at Rc = 2"),
    _row(3, 4, "mbf16<4>", "k = 12 at Rc = 4, rl = 3"),
    # the batch edge of recursion_wave_kernel<8, COV>: one replicate more than one wave per SIMD (B = None: 4 CUs + 1, known on the device)
    Row(BATCH_EDGE, 2, 3, False, 6, 24, None, "wave<8> CH8=4", "B = 4 (CU count) + 1: the CH8 = 4 instance"),
    # the 64 KB opt-in edge of launch_wave_cov_ch at Rp = 32: wave_lds_bytes<32>(752) = 65536
    _row(8, 4, "wave<32> lds<=64K", "the last T without the opt-in", N=16, T=752, tag="-T752"),
    _row(8, 4, "wave<32> lds>64K", "the first T with it", N=16, T=753, tag="-T753"),
]
BY_NAME = {row.name: row for row in ROWS}
assert len(BY_NAME) == len(ROWS)

# handles of the diagnostics build: (switch, row names).  DFM_NO_RECURSION_WAVE is read when the handle is created (RouteOpts);
# DFM_NO_COMP and DFM_NO_MBF16 are function-static in recursion_comp_supported / recursion_mbf16_supported -- read once per process,
# at the first launch_recursion of any handle -- so a test module cannot switch them and they have no rows here.
DIAG_ROWS = {"DFM_NO_RECURSION_WAVE": ("r5p2", "r4p4", "r2p6", "r8p4-diag", "r4p5")}
ROWS_DIAG_ONLY = [_row(8, 4, "wave<32> Rc=8", "the headline width with the default lags", tag="-diag")]
BY_NAME.update({row.name: row for row in ROWS_DIAG_ONLY})

# one row per route class for the want_P=False pass and the host entries
ONE_PER_CLASS = ("r1p2", "r4p1", "r2p4", "r8p1", "r5p3", "r16p1", "r4p6", "r2p16", "r3p6", "r7p4", "r10p3", "r32p1", "r4p4-sing", "r4p5-sing",
                 "r4p4", "r2p6", "r3p4")


def n_series(row, variant):
    if row.N is not None:
        return row.N
    n = max(2 * row.r, 12)
    return (n + 1) & ~1 if variant == "balanced" else n | 1


def n_periods(row):
    return row.T if row.T is not None else row.r * row.p + row.p + 3 * row.r + 12


def n_distinct(row):
    """Replicates the oracle computes: the batch-edge row tiles three over its batch."""
    return 3 if row.B is None else row.B


def batch(row, num_cu=MI355X_CU):
    return 4 * num_cu + 1 if row.B is None else row.B


def row_classes(row, num_cu=MI355X_CU, wave=True):
    return classes(row.r, row.p, row.singular, wave, n_periods(row), batch(row, num_cu), num_cu)


def missing_classes():
    seen = set()
    for row in ROWS:
        seen |= row_classes(row)
    return REQUIRED - seen


def missing_diag_classes():
    seen = set()
    for name in DIAG_ROWS["DFM_NO_RECURSION_WAVE"]:
        seen |= row_classes(BY_NAME[name], wave=False)
    return REQUIRED_DIAG - seen


# ------------------------------------------------------------------------------------------------ inputs and references
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def pack(P, r):
    """[T, k, k] -> the factor block's lower triangle, row-major packed: the layout of P_smooth."""
    tri = np.tril_indices(r)
    return np.ascontiguousarray(P[:, :r, :r][:, tri[0], tri[1]])


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    """x [D, T, N] and the start {key: [D, ...]} of the row's D distinct replicates."""
    row = BY_NAME[name]
    N, T, r, p = n_series(row, variant), n_periods(row), row.r, row.p
    xs, qs = [], []
    for b in range(n_distinct(row)):
        x = vo.synth_varp(b, N, T, r, p, missing=MISS_SHARE if variant == "missing" else 0.0)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        if variant == "missing":
            x[[0, 5, T - 1], :] = np.nan
        if row.singular:
            G = np.linalg.cholesky(q["Q"])[:, :r - 1]
            q["Q"] = G @ G.T                                       # rank r - 1
        xs.append(x); qs.append(q)
    x = np.stack(xs)
    q = {k: np.stack([s[k] for s in qs]) for k in KEYS}
    _frozen(x, *q.values())
    return x, q


def start(name, variant, b):
    _, q = inputs(name, variant)
    return {k: q[k][b] for k in KEYS}


@functools.lru_cache(maxsize=None)
def pass_reference(name, variant):
    """Per distinct replicate: loglik, f_smooth [T, r], P_smooth [T, r (r + 1) / 2] of varp_oracle.kfs_pass_varp at the start."""
    row = BY_NAME[name]
    x, _ = inputs(name, variant)
    out = []
    for b in range(x.shape[0]):
        o = vo.kfs_pass_varp(x[b], p=row.p, **start(name, variant, b))
        d = dict(loglik=float(o["loglik"]), f_smooth=np.ascontiguousarray(o["f_smooth"][:, :row.r]), P_smooth=pack(o["P_smooth"], row.r))
        _frozen(*d.values())
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def em_reference(name, variant):
    """Per distinct replicate: varp_oracle.em_varp, EM_ITERS iterations, tol 0: the parameters, the path, the last E-step's moments."""
    row = BY_NAME[name]
    x, _ = inputs(name, variant)
    out = []
    for b in range(x.shape[0]):
        q, path, o = vo.em_varp(x[b], start(name, variant, b), row.p, EM_ITERS, 0.0)
        d = dict(q, path=path, f_smooth=np.ascontiguousarray(o["f_smooth"][:, :row.r]), P_smooth=pack(o["P_smooth"], row.r))
        _frozen(*d.values())
        out.append(d)
    return tuple(out)
