"""Launch geometry of the loadings half of the M-step on a balanced panel (csrc/mstep_mfma.hip: mstep_mfma_kernel<R, STEPS, NDR>,
mstep_finish_kernel<R>; csrc/mstep_wide.hip: mstep_wide_kernel<R, NX>, mstep_finish_wide_kernel<R>; make_plan's waves per
replicate), restated in plain Python, the rule that says which loadings kernel a balanced EM takes, and the case tables of
tests/test_gpu_mstep_geometry.py.  Test infrastructure only: csrc/dfm_msgeom.h stays the authority, and
tests/test_mstep_geometry_cpu.py holds this restatement against that header, compiled for the host (tests/host/msgeom_host.cpp), for
every instance and over a sweep of N, T and B.

mstep_mfma: Rp = 4 | 8, a step is CS = 16 | 8 series, STEPS = ceil(N / CS) <= 32 accumulators per lane, NDR = ceil(8 N / 1024) 1-KB
pieces of a panel row per DMA row -- one NDR per (Rp, STEPS): 64 instances.  A replicate's T periods are dealt to wpr waves in
segments of tq periods, tq rounded up so that every segment starts on a 128-byte line; a segment runs in row blocks of 4 periods,
two in flight.  The first nfront workgroups of the launch are four transition-step waves each.
mstep_wide: an item is 128 series of a replicate, streamed in stages of 32 periods through three buffers; <32, NX> for Rp = 32 with
NX = 1 .. 4 groups of 4 factor columns past the first 16, <16, 0> for Rp <= 16 with rd = Rp columns in the caller's arrays.

Every reference is computed once per process (functools.lru_cache) and must not be modified by its users."""
import functools
import os
import subprocess

import numpy as np

from oracle import kalman_oracle as ko

KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
MS_MAX_STEPS = 32                    # dfm_msgeom.h kMsMaxSteps
MW_SER, MW_PER, MW_NBUF = 128, 32, 3  # dfm_msgeom.h kMwSer, kMwPer, kMwNBuf
NUM_CU = 256                         # an MI355X: the persistent grid of mstep_wide_kernel


def pad_r(n):
    """capi.hip pad_r: the power of two >= n, at least 2."""
    p = 2
    while p < n:
        p <<= 1
    return p


def collapse_max_n(Rp):
    """collapse.hip collapse_max_n."""
    return 1024 if Rp <= 8 else 512 if Rp <= 16 else 256


# ------------------------------------------------------------------------------------------------------------- the route
def fast_eligible(N, r, may_have_missing=False, singular_q=False):
    """capi.hip fast_eligible (no route switch set): collapse_dma_supported or collapse_wide_supported of the padded width."""
    if may_have_missing or singular_q:
        return False
    Rp = pad_r(r)
    dma = N % 2 == 0 and N <= collapse_max_n(Rp)
    wide = 2 <= Rp <= 32 and N >= 1
    return dma or wide


def mfma_supported(Rp, N):
    """mstep_mfma_supported."""
    if N % 2 or N * 8 > 4096 or N < 4 or Rp not in (4, 8):
        return False
    cs = 16 if Rp == 4 else 8
    return (N + cs - 1) // cs <= MS_MAX_STEPS


def wide_supported(Rp, N):
    """mstep_wide_supported."""
    if N % 2 or N < 2:
        return False
    return Rp in (16, 32) or (2 <= Rp <= 8 and N * 8 > 4096)


def route(N, r, may_have_missing=False):
    """The loadings kernel of an EM iteration (make_plan, em_iteration): mstep_mfma before mstep_wide, both on the fast path only."""
    Rp = pad_r(r)
    fast = fast_eligible(N, r, may_have_missing)
    if fast and mfma_supported(Rp, N):
        return "mstep_mfma"
    if fast and wide_supported(Rp, N):
        return "mstep_wide"
    return "mstep_lam"


PROFILE_NAME = {"mstep_mfma": "mstep_mfma_kernel", "mstep_wide": "mstep_wide_kernel", "mstep_lam": "mstep_lam_kernel"}


# ------------------------------------------------------------------------------------------------------------- mstep_mfma
def ms_cs(Rp):
    """MsGeo<Rp>::CS: 4 / min(4, factor groups of 4) series groups of 4 per instruction."""
    nfg = (Rp + 3) // 4
    return 4 * (4 // min(nfg, 4))


def ms_instance(Rp, N):
    """(Rp, STEPS, NDR) as launch_ms_pick chooses it."""
    cs = ms_cs(Rp)
    return Rp, (N + cs - 1) // cs, (8 * N + 1023) // 1024


def ms_instances():
    """The 64 instances: one NDR per (Rp, STEPS) over the even N of mstep_mfma_supported."""
    return sorted({ms_instance(Rp, N) for Rp in (4, 8) for N in range(4, 513, 2) if mfma_supported(Rp, N)})


def ms_range(Rp, steps):
    """The even N of instance (Rp, steps): lowest and highest."""
    cs = ms_cs(Rp)
    return max(4, cs * (steps - 1) + 2), cs * steps


def ms_wpr(B, T):
    """make_plan: waves (segments) per replicate."""
    w = max(1, min(8, 3072 // B))
    while w > 1 and T // w < 8:
        w -= 1
    return w


def tq_factor(N):
    """Rows a segment's length is rounded up to: 128 / lowbit(8 N mod 128), 1 where a row is a multiple of 128 bytes."""
    g = (8 * N) % 128
    g = 128 if g == 0 else g & -g
    return 128 // g


def ms_slot_bytes(N):
    sb = 8 * N
    while sb % 256 not in (64, 192):
        sb += 16
    return sb


def mfma(B, N, T, r):
    """One launch of mstep_mfma_kernel inside an EM iteration of a B x T x N batch with r factors."""
    Rp = pad_r(r)
    assert mfma_supported(Rp, N), (N, r)
    cs = ms_cs(Rp)
    _, steps, ndr = ms_instance(Rp, N)
    wpr = ms_wpr(B, T)
    m = tq_factor(N)
    tq = (((T + wpr - 1) // wpr + m - 1) // m) * m
    nrows = tuple(min(T, min(s * tq, T) + tq) - min(s * tq, T) for s in range(wpr))
    return dict(Rp=Rp, CS=cs, STEPS=steps, NDR=ndr, slot=ms_slot_bytes(N), tail_clamp=N % cs != 0, wpr=wpr, tq=tq, m=m, nrows=nrows,
                nfront=(B + 3) // 4, front_idle=(-B) % 4, stream_blocks=(B * wpr + 3) // 4, stream_idle=(-B * wpr) % 4,
                last_piece_lanes=(8 * N - 1024 * (ndr - 1)) // 16)


def mfma_host_tuple(g):
    """The fields of `mfma` in the order tests/host/msgeom_host.cpp prints an M line (lo = hi = NDR)."""
    return (1, g["CS"], g["STEPS"], g["NDR"], g["NDR"], g["NDR"], g["slot"], g["wpr"], g["tq"], g["nfront"], g["stream_blocks"]) + \
        g["nrows"] + (-1,) * (8 - g["wpr"])


def nrows_class(n):
    """How a segment of n rows runs: not at all; MODE 2 blocks only; MODE 1 then MODE 2; MODE 0 blocks in front of them."""
    if n == 0:
        return "0"
    if n < 8:
        return "1..7"
    if n == 8:
        return "8"
    if n < 12:
        return "9..11"
    return ">=12,partial" if n % 4 else ">=16,whole" if n >= 16 else ">=12,whole"


# ------------------------------------------------------------------------------------------------------------- mstep_wide
def wide(B, N, T, r, num_cu=NUM_CU):
    """One launch of mstep_wide_kernel + mstep_finish_wide_kernel."""
    Rp = pad_r(r)
    assert wide_supported(Rp, N), (N, r)
    R, nx = (16, 0) if Rp <= 16 else (32, 1 if r <= 16 else (r + 3 - 16) // 4)
    nsb = (N + MW_SER - 1) // MW_SER
    nst = (T + MW_PER - 1) // MW_PER
    xcd = int(B >= 16)
    g = max(8, (num_cu if num_cu > 0 else 256) // 8 * 8)
    if not xcd and B * nsb < g:
        g = B * nsb
    return dict(Rp=Rp, R=R, NX=nx, rd=Rp, nsb=nsb, last_series=N - (nsb - 1) * MW_SER, stages=nst, last_rows=T - (nst - 1) * MW_PER,
                xcd_map=xcd, grid=g, items=B * nsb, finish_blocks=(N + 255) // 256)


def wide_host_tuple(g):
    return (1, g["R"], g["NX"], g["rd"], g["nsb"], g["last_series"], g["stages"], g["last_rows"], g["xcd_map"], g["grid"],
            g["finish_blocks"], MW_NBUF)


def wide_instances():
    """(R, NX, rd): mstep_wide_kernel<32, 1..4> (with mstep_finish_wide_kernel<32>) and <16, 0> at rd = 2, 4, 8, 16 (with
    mstep_finish_wide_kernel<rd>): every instance of both kernels, and every rd the one <16, 0> instance is run with."""
    return [(32, nx, 32) for nx in (1, 2, 3, 4)] + [(16, 0, rd) for rd in (2, 4, 8, 16)]


# ------------------------------------------------------------------------------------------------------------- the case tables
# Every case starts from the parameters ko.synth_replicate returns beside the panel (the truth, rescaled), two EM iterations.
# MFMA_CASES (B, N, T, r): one case per instance in the order of ms_instances(), then the extra cases.
# r cycles 3, 4 (Rp = 4) and 5 .. 8 (Rp = 8); N walks the instance's range: its lowest even N (CS (STEPS - 1) + 2), its highest
# (CS STEPS; every multiple of 128, where the last 1-KB piece is whole), and N = 8 mod 16 / 4 mod 8 in between, so that a segment's
# length is rounded up to 8, 1, 2 and 4 rows; T = 9 .. 80 walks wpr = 1 .. 8 (B = 2: wpr = min(8, T / 8)) and the segments' rows.
MFMA_CASES = [
    (2, 4, 9, 3), (2, 32, 57, 4), (2, 40, 29, 3), (2, 60, 15, 4), (2, 66, 47, 3), (2, 96, 12, 4),
    (2, 104, 70, 3), (2, 128, 33, 4), (2, 130, 72, 3), (2, 160, 52, 4), (2, 168, 17, 3), (2, 188, 64, 4),
    (2, 194, 36, 3), (2, 224, 23, 4), (2, 232, 50, 3), (2, 256, 20, 4), (2, 258, 77, 3), (2, 288, 40, 4),
    (2, 296, 80, 3), (2, 316, 60, 4), (2, 322, 24, 3), (2, 352, 65, 4), (2, 360, 44, 3), (2, 384, 9, 4),
    (2, 386, 57, 3), (2, 416, 29, 4), (2, 424, 15, 3), (2, 444, 47, 4), (2, 450, 12, 3), (2, 480, 70, 4),
    (2, 488, 33, 3), (2, 512, 72, 4), (2, 4, 52, 5), (2, 16, 17, 6), (2, 24, 64, 7), (2, 28, 36, 8),
    (2, 34, 23, 5), (2, 48, 50, 6), (2, 56, 20, 7), (2, 60, 77, 8), (2, 66, 40, 5), (2, 80, 80, 6),
    (2, 88, 60, 7), (2, 92, 24, 8), (2, 98, 65, 5), (2, 112, 44, 6), (2, 120, 9, 7), (2, 128, 57, 8),
    (2, 130, 29, 5), (2, 144, 15, 6), (2, 152, 47, 7), (2, 156, 12, 8), (2, 162, 70, 5), (2, 176, 33, 6),
    (2, 184, 72, 7), (2, 188, 52, 8), (2, 194, 17, 5), (2, 208, 64, 6), (2, 216, 36, 7), (2, 220, 23, 8),
    (2, 226, 50, 5), (2, 240, 20, 6), (2, 248, 77, 7), (2, 256, 40, 8),
]
# B = 1, 5, 9: a front workgroup with one live wave (B = 5, 9: past a full one) and a streaming grid whose last workgroup is partial
# (3, 25 and 54 segments); T = 3 and T = 8: one segment of MODE 2 blocks only, one of exactly two row blocks.
MFMA_EXTRA = [(1, 40, 30, 3), (5, 50, 41, 6), (9, 36, 50, 4), (2, 22, 3, 3), (2, 44, 8, 5)]
# WIDE_CASES (B, N, T, r): NX = 1 .. 4 at both ends of its r; rd = 2 (r = 1, 2), 4, 8, 16 (r = 9, 16); N = 128 k, 128 k + 2, a last
# block of 2 .. 16 series, one block, more than 256 series (a second block of the finish kernel); T = 5 (one partial stage), 32,
# 33, 96 (the third buffer), 97 (the first buffer again); B = 17: a queue per XCD with B no multiple of 8 and fewer items than workgroups.
WIDE_CASES = [
    (2, 128, 32, 17), (2, 130, 33, 20), (2, 66, 97, 21), (2, 258, 40, 24), (2, 144, 96, 25), (2, 40, 33, 28), (2, 256, 32, 29),
    (2, 270, 40, 32), (2, 514, 33, 1), (2, 1024, 5, 2), (2, 600, 20, 3), (2, 770, 40, 7), (2, 130, 97, 9), (2, 64, 32, 16),
    (17, 48, 40, 22), (17, 258, 34, 10),
]
# STOP_CASES (B, N, T, r, tol, max_iter, route): replicates 2 and 3 start from STOP_SCALE x the loadings.  The oracle stops after
# (3, 4, 5, 5), (4, 4, 5, 5), (7, 7, 8, 9) and (6, 6, 8, 8) iterations.
STOP_CASES = [
    (4, 40, 60, 3, 1e-3, 40, "mstep_mfma"), (4, 50, 60, 6, 1e-3, 40, "mstep_mfma"),
    (4, 64, 48, 12, 1e-3, 40, "mstep_wide"), (4, 66, 90, 18, 1e-3, 40, "mstep_wide"),
]
MAX_ITER = 2
STOP_SCALE = 0.3


def case_id(row):
    return "b{}_n{}_t{}_r{}".format(*row[:4])


def mfma_classes(row):
    B, N, T, r = row[:4]
    g = mfma(B, N, T, r)
    s = {"instance={Rp},{STEPS},{NDR}".format(**g), f"wpr={g['wpr']}", f"tq_factor={g['m']}", "tail_clamp" if g["tail_clamp"] else "no_tail_clamp"}
    s |= {"nrows:" + nrows_class(n) for n in g["nrows"]}
    lo, hi = ms_range(g["Rp"], g["STEPS"])
    if N == lo:
        s.add("N=lowest")
    if N == hi:
        s.add("N=highest")
    if N == 4:
        s.add("N=4")
    s.add("last_piece:full" if g["last_piece_lanes"] == 64 else "last_piece:partial")
    if g["front_idle"]:
        s.add("front:clamped_wave")
    if B > 4 and g["front_idle"]:
        s.add("front:clamped_wave_past_a_full_group")
    if g["stream_idle"]:
        s.add("stream:partial_last_group")
    if T < 8:
        s.add("T<8")
    if T == 8:
        s.add("T==8")
    return s


MFMA_REQUIRED = (
    {"instance={},{},{}".format(*i) for i in ms_instances()}
    | {f"wpr={w}" for w in range(1, 9)} | {f"tq_factor={m}" for m in (1, 2, 4, 8)} | {"tail_clamp", "no_tail_clamp"}
    | {"nrows:" + c for c in ("0", "1..7", "8", "9..11", ">=12,partial", ">=16,whole")}
    | {"N=lowest", "N=highest", "N=4", "last_piece:full", "last_piece:partial"}
    | {"front:clamped_wave", "front:clamped_wave_past_a_full_group", "stream:partial_last_group", "T<8", "T==8"}
)


def wide_classes(row):
    B, N, T, r = row[:4]
    g = wide(B, N, T, r)
    s = {"instance={R},{NX},{rd}".format(**g), f"r={r}"}
    if N > 256:
        s.add("finish:second_block")
    if N % 128 == 0:
        s.add("N=128k")
    if N % 128 == 2:
        s.add("N=128k+2")
    if g["nsb"] > 1 and g["last_series"] <= 16:
        s.add("last_block<=16")
    if g["nsb"] == 1 and g["Rp"] >= 16:
        s.add("one_block")
    for t in (5, 32, 33, 96, 97):
        if T == t:
            s.add(f"T={t}")
    if g["xcd_map"] and B % 8:
        s.add("xcd_map,B%8!=0")
    if g["xcd_map"] and g["items"] < g["grid"]:
        s.add("xcd_map,items<grid")
    if not g["xcd_map"]:
        s.add("grid=items")
    return s


WIDE_REQUIRED = (
    {"instance={},{},{}".format(*i) for i in wide_instances()}
    | {f"r={r}" for r in (17, 20, 21, 24, 25, 28, 29, 32, 1, 2, 9, 16)}
    | {"finish:second_block", "N=128k", "N=128k+2", "last_block<=16", "one_block"}
    | {f"T={t}" for t in (5, 32, 33, 96, 97)} | {"xcd_map,B%8!=0", "xcd_map,items<grid", "grid=items"}
)


def missing_classes(required, classes, cases):
    hit = set()
    for row in cases:
        hit |= classes(row)
    return sorted(required - hit)


def watched_series(row):
    """Series whose update an un-updated or mis-addressed series could not imitate: the first, the last, the last of each 1-KB piece
    of a panel row, the first of the last block of 128."""
    N = row[1]
    return sorted({0, N - 1} | set(range(127, N, 128)) | {(N - 1) // MW_SER * MW_SER})


# ------------------------------------------------------------------------------------------------------------- panels, expectation
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def batch(B, N, T, r, scale_from=None):
    """Panel [B, T, N] and start {key: [B, ..]} of ko.synth_replicate(b, ..); the loadings of replicates scale_from .. are multiplied
    by STOP_SCALE (the stop cases)."""
    reps = [ko.synth_replicate(b, N, T, r) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    start = {k: np.stack([p[k] for _, p in reps]) for k in KEYS}
    if scale_from is not None:
        start["Lam"][scale_from:] *= STOP_SCALE
    _frozen(panel, *start.values())
    return panel, start


def _em(x, st, max_iter, tol):
    p, path, out = ko.em(x, st, max_iter=max_iter, tol=tol)
    e = dict(est=p, path=path, f=out["f_smooth"], P=ko.pack_sym(out["P_smooth"]), Pscale=float(np.abs(out["P_smooth"]).max()))
    _frozen(path, e["f"], e["P"], *p.values())
    return e


@functools.lru_cache(maxsize=None)
def expected(row):
    """A case of MFMA_CASES / MFMA_EXTRA / WIDE_CASES: the batch and, per replicate, two oracle EM iterations from its start."""
    B, N, T, r = row
    panel, start = batch(B, N, T, r)
    ems = tuple(_em(panel[b], {k: start[k][b] for k in KEYS}, MAX_ITER, 0.0) for b in range(B))
    return dict(panel=panel, start=start, ems=ems)


@functools.lru_cache(maxsize=None)
def expected_stop(row):
    """A case of STOP_CASES: the oracle's EM with the stop rule, replicate by replicate."""
    B, N, T, r, tol, max_iter, _ = row
    panel, start = batch(B, N, T, r, scale_from=2)
    ems = tuple(_em(panel[b], {k: start[k][b] for k in KEYS}, max_iter, tol) for b in range(B))
    return dict(panel=panel, start=start, ems=ems)


# ------------------------------------------------------------------------------------------------------------- the host check
SWEEP_N = range(2, 1101)
SWEEP_T = range(3, 141)
SWEEP_B = (1, 2, 5, 16, 17, 400, 3072, 4000)


def build_msgeom_host(directory):
    """tests/host/msgeom_host.cpp, which includes csrc/dfm_msgeom.h and nothing else of the library, compiled with g++."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "msgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "msgeom_host.cpp")], check=True)
    return exe


def ask_msgeom_host(exe, text, count):
    """One process for all the request lines of `text`: the printed fields of each, as int tuples."""
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == count, (len(out), count)
    return [tuple(map(int, line.split())) for line in out]
