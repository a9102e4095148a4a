"""Launch geometry of the parameter block of the Gibbs sampler -- gibbs_gram_kernel, gibbs_load_kernel<RB, MISS>, gibbs_var_kernel
(csrc/gibbs.hip) -- as launch_gibbs_gram / launch_gibbs_load / launch_gibbs_var launch them from dfm_gibbs_batch (csrc/capi.hip), the
eight instances of the load kernel, the cross-sections the sweep's pass admits, and the case table of tests/test_gpu_gibbs_geometry.py
with the coverage classes it must hit.  Test infrastructure only.

The series split is series_geometry's (csrc/dfm_cellgeom.h): forecast_ar_expect.geometry is its restatement, held against the header
by tests/host/seriesgeom_host.cpp; tests/test_gibbs_geometry_cpu.py puts every row through that program and reads the lines of
launch_gibbs_load that say the same from the source.  The missing-cell pattern is ar_post_geometry.edge_pattern at q = 0 and rc = 64:
the load kernel stages 64 rows of f per chunk and its panel prefetch restarts at each chunk.

What crosses a chunk edge: in gibbs_load_kernel the sums (G, s, xx, cnt) in registers, the prefetched cell `xn` does NOT (it is read
again at the chunk's first row); in gibbs_var_kernel the twelve accumulators, and the p lag rows are staged again ahead of each chunk
of 32 rows.

Every input is computed once per process (functools.lru_cache) and must not be modified by its users."""
import functools

import numpy as np

from oracle import kalman_oracle as ko
from oracle import synth_oracle as so
from oracle import varp_oracle as vo
from tests import ar_geometry as ag
from tests import ar_post_geometry as apg
from tests import forecast_ar_expect as fe
from tests import gibbs_ar_expect as gae
from tests import gibbs_cases as gc
from tests import gibbs_expect as ge

KEYS = gc.KEYS
B = 2
SWEEPS = 2
TC = 64                              # gibbs.hip kGbTC: rows of f per chunk of gibbs_load_kernel / gibbs_gram_kernel
VAR_TC = 32                          # gibbs.hip kGbVarTC: rows per chunk of gibbs_var_kernel, behind the p lag rows
THREADS = 256                        # gibbs.hip kGbThreads
BLOCK_LANES = 256                    # dfm_cellgeom.h kCellBlockLanes
VAR_ACC = 12                         # gibbs_var_kernel: acc[12], entries per thread at most
MAX_CELLS = 40000                    # N T of a row, at most
edge_pattern = apg.edge_pattern
N_EDGE_KINDS = apg.N_EDGE_KINDS


# ------------------------------------------------------------------------------------------------------------- admission, instances
def bucket(r):
    """dfm_cellgeom.h dispatch_r_bucket."""
    return 4 if r <= 4 else 8 if r <= 8 else 16 if r <= 16 else 32


def shape_admits(T, r, p):
    """capi.hip gibbs_check: r p <= 32 (DFM_MAX_R) and T > p."""
    return r >= 1 and p >= 1 and r * p <= 32 and T > p


def pass_admits(N, r, p, flag):
    """The cross-sections the sweep's pass (dfm_simsmooth_batch_dev -> slice_pass) takes.  p = 1 is dfm_ks_pass_batch_dev: without the
    may-have-missing flag fast_eligible holds at every N (collapse_wide_supported); with it check_general_n(N, r, plain): the plain
    model's exception at padded width 32 (collapse_wide2_supported of N or of N + 1: an even N, or an odd one padded to it), else
    N <= collapse_max_n(pad_r(r)).  p > 1 is varp_run: check_general_n(N, r) whatever the flag says (the companion's loadings are
    pad_r(r) wide)."""
    if N < 1:
        return False
    if p == 1:
        if not flag or ag.pad_r(r) == 32:
            return True
    return N <= ag.collapse_max_n(ag.pad_r(r))


def table_max_n(r, p):
    """What the table holds itself to under the flag, the rule at the padded width of the whole state r p: 1024 / 512 / 256 at
    <= 8 / <= 16 / 32.  Never wider than pass_admits at p > 1 (pad_r(r p) >= pad_r(r)); at p = 1 it forgoes the exception at width 32."""
    return ag.collapse_max_n(ag.pad_r(r * p))


LOAD_INSTANCES = [(rb, miss) for rb in (4, 8, 16, 32) for miss in (False, True)]


# ------------------------------------------------------------------------------------------------------------- launches
def launches(c):
    """dict(load, gram (None under the flag), var): the three launches of one sweep of the case."""
    N, T, r, p, miss = c["N"], c["T"], c["r"], c["p"], c["flag"]
    npb, _, _, _, nsblk, threads = fe.geometry(N, 1, T)
    rb = bucket(r)
    chunks = (T + TC - 1) // TC
    load = dict(kernel="gibbs_load_kernel", RB=rb, MISS=miss, nsblk=nsblk, npb=npb, threads=threads, chunks=chunks,
                last_chunk_rows=T - (chunks - 1) * TC, n=rb if rb <= 16 else r, call=(N, 1, T, 48 * 1024),
                idle_last=nsblk * npb > N,                                   # lanes behind series N - 1 in the last block
                ragged_wave=threads > npb)                                   # lanes behind the block's npb series in its last wave
    gram = None if miss else dict(kernel="gibbs_gram_kernel", rr=r * r, acc_used=(r * r + THREADS - 1) // THREADS, chunks=chunks,
                                  threads=THREADS)
    k = r * p
    ne = k * k + k * r + r * r
    var = dict(kernel="gibbs_var_kernel", k=k, n=T - p, chunks=(T - p + VAR_TC - 1) // VAR_TC, ne=ne, ept=(ne + THREADS - 1) // THREADS,
               nlow=r * (r - 1) // 2, threads=THREADS)
    return dict(load=load, gram=gram, var=var)


# ------------------------------------------------------------------------------------------------------------- the case table
# name, N, T, r, p, pattern, A0, empty.  pattern: None = balanced, flag off; "edge" = edge_pattern(x, 0, rc=64, first=b), flag on;
# a float = iid missing cells at that rate, flag on (a class that needs missing cells on a panel without 64 rows).  A0: the prior
# has a mean of A, non-symmetric and different per chain.  empty: a series without any observed cell (None: no such series).
# B = 2 chains, SWEEPS = 2.  N T <= 40 000.  The comment of a row names the classes it alone holds.
CASES = [
    # r = 1 under MISS (three identity-padded coordinates of bucket 4, hr = 1); k = 32 as (1, 32); p > 4; T - p = 33; nlow = 0 with
    # a prior mean of A at p > 1.  T = 65: a second chunk of one row, behind the edge kinds 1, 3, 4, 5, 6
    ("r1_p32_t65",   40,  65,  1,  32, "edge", True,  None),
    # r = 1 on the shared root: gram at rr = 1; three blocks of 201 with two idle lanes in the last; T = 64 exactly
    ("r1_n601_t64",  601, 64,  1,  1,  None,   False, None),
    # the top of bucket 4; T = 130: the kinds 0, 4, 5 at the edge 128; the prior mean of A at p = 1
    ("r4_t130",      24,  130, 4,  1,  "edge", True,  None),
    # k = 32 as (2, 16); nlow = 1; T - p = 32 exactly (shared with r32_miss: here behind sixteen staged lag rows)
    ("r2_p16_n32",   48,  48,  2,  16, None,   True,  None),
    # the bottom of bucket 8 under MISS; T - p = 65: a third var chunk of one row; every edge kind at 64; the series without a cell
    ("r5_t66",       40,  66,  5,  1,  "edge", False, 11),
    # the top of bucket 8 on the shared root; k = 32 as (8, 4); T - p = 64 behind four staged lag rows
    ("r8_p4_n64",    64,  68,  8,  4,  None,   False, None),
    # the bottom of bucket 16 under MISS, on two blocks of 129 with an idle lane in the last
    ("r9_n257",      257, 66,  9,  1,  "edge", False, None),
    # the top of bucket 16 on the shared root: gram at rr = 256, the first accumulator full; T = 128: two full chunks and no third
    ("r16_n256_t128", 256, 128, 16, 1, None,   False, None),
    # an odd r in the scratch bucket under MISS: the pair loop ends on a half-used pair; T = 129: a third chunk of one row
    ("r17_t129",     100, 129, 17, 1,  "edge", False, None),
    # the largest odd r on the shared root: gram over T = 65 with the accumulators two to four; twelve entries per thread at ne = 2883
    ("r31_t65",      70,  65,  31, 1,  None,   False, None),
    # r = 32 under MISS on its one block shape, N = 256 with no idle lane (iid missing cells: a 33-row panel has no chunk edge)
    ("r32_miss",     256, 33,  32, 1,  0.1,    False, None),
    # r = 32 on the shared root: gram at rr = 1024, every accumulator full
    ("r32_bal",      96,  40,  32, 1,  None,   False, None),
    # T - p = 1: one row behind four staged lag rows, every sum a single product
    ("n1_p4",        12,  5,   3,  4,  None,   True,  None),
]
CASE_KEYS = ("name", "N", "T", "r", "p", "pattern", "A0", "empty")
NAMES = [row[0] for row in CASES]
# one balanced row per bucket for the comparison of gibbs_load_kernel<RB, true> with <RB, false>; the bit-for-bit repeats
BUCKET_ROWS = ("r1_n601_t64", "r8_p4_n64", "r16_n256_t128", "r31_t65")
REPEAT_ROWS = ("r2_p16_n32", "r1_n601_t64")                   # k = 32 at p > 1; three series blocks


def case_dict(row):
    c = dict(zip(CASE_KEYS, row))
    c["flag"] = c["pattern"] is not None
    return c


def _row(name):
    return CASES[NAMES.index(name)]


# ------------------------------------------------------------------------------------------------------------- coverage classes
def _edge_kinds(c):
    """The (e, kind) the case's panel carries, from the pattern alone (no synthesis): edge_pattern on a dummy panel."""
    used = set()
    if c["pattern"] == "edge":
        for b in range(B):
            used |= edge_pattern(np.zeros((c["T"], c["N"])), 0, rc=TC, first=b)
    return used


def classes(c):
    """dict(load, gram, var) -> the set of coverage classes the case hits (the names of REQUIRED)."""
    g = launches(c)
    N, T, r, p = c["N"], c["T"], c["r"], c["p"]
    ld, s = g["load"], set()
    how = "MISS" if ld["MISS"] else "BAL"
    s.add(f"instance={ld['RB']},{how}")
    if r in (1, 4, 5, 8, 9, 16, 17, 32):
        s.add(f"r={r}")
    if r in (1, 32):
        s.add(f"r={r}:{how}")
    if r >= 17 and r % 2:
        s.add(f"odd_r>=17:{how}")
    s.add(f"T={T}" if T in (64, 65, 128, 129) else "T<64" if T < TC else "T:other")
    if ld["chunks"] >= 3:
        s.add("chunks>=3")
    s.add("nsblk=1" if ld["nsblk"] == 1 else "nsblk=2" if ld["nsblk"] == 2 else "nsblk>=3")
    if N == 256:
        s.add("N=256")
    if ld["idle_last"]:
        s.add("idle_last_block")
    if ld["ragged_wave"]:
        s.add("ragged_wave")
    if ld["RB"] == 16 and ld["MISS"] and ld["nsblk"] == 2:
        s.add("two_blocks:RB=16,MISS")
    s |= {f"edge@{e}:{kind}" for e, kind in _edge_kinds(c)}
    if c["empty"] is not None and ld["MISS"]:
        s.add("n_i=0")
    out = dict(load=s, gram=set(), var=set())
    if g["gram"] is not None:
        rr = g["gram"]["rr"]
        out["gram"] = {"rr<=256" if rr <= THREADS else "rr>256"} | ({"rr=1024"} if rr == 1024 else set()) | ({"T=65"} if T == 65 else set())
    v, s = g["var"], set()
    if v["n"] in (1, 32, 33, 64, 65):
        s.add(f"n={v['n']}")
    if v["chunks"] >= 3:
        s.add("var_chunks>=3")
    if v["k"] == 32:
        s.add(f"k=32:({r},{p})")
    s.add("ept=1" if v["ept"] == 1 else "ept=12" if v["ept"] == VAR_ACC else "ept=2..11")
    if v["nlow"] in (0, 1):
        s.add(f"nlow={v['nlow']}")
    if v["nlow"] % 2:
        s.add("nlow_odd")
    s.add("A0:none" if not c["A0"] else "A0:p=1" if p == 1 else "A0:p>1")
    if p > 4:
        s.add("p>4")
    out["var"] = s
    return out


REQUIRED = dict(
    load=({f"instance={rb},{'MISS' if miss else 'BAL'}" for rb, miss in LOAD_INSTANCES}
          | {f"r={r}" for r in (1, 4, 5, 8, 9, 16, 17, 32)}
          | {f"{what}:{how}" for what in ("r=1", "odd_r>=17", "r=32") for how in ("MISS", "BAL")}
          | {"T=64", "T=65", "T=128", "T=129", "T<64", "chunks>=3", "nsblk=1", "nsblk=2", "nsblk>=3", "N=256", "idle_last_block",
             "ragged_wave", "two_blocks:RB=16,MISS", "n_i=0"}
          | {f"edge@{TC}:{kind}" for kind in range(N_EDGE_KINDS)} | {f"edge@{2 * TC}:{kind}" for kind in (0, 4, 5)}),
    gram={"rr<=256", "rr>256", "rr=1024", "T=65"},
    var=({f"n={n}" for n in (1, 32, 33, 64, 65)} | {f"k=32:({r},{p})" for r, p in ((32, 1), (8, 4), (2, 16), (1, 32))}
         | {"var_chunks>=3", "ept=1", "ept=2..11", "ept=12", "nlow=0", "nlow=1", "nlow_odd", "A0:p=1", "A0:p>1", "A0:none", "p>4"}),
)


def missing_classes(cases=None):
    """{kernel: sorted classes of REQUIRED that no case of `cases` (default CASES) hits}; empty lists when all are covered."""
    hit = {kern: set() for kern in REQUIRED}
    for row in (CASES if cases is None else cases):
        for kern, s in classes(case_dict(row)).items():
            hit[kern] |= s
    return {kern: sorted(REQUIRED[kern] - hit[kern]) for kern in REQUIRED}


# ------------------------------------------------------------------------------------------------------------- inputs, the model's chains
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of a case: dict(case fields, x [B,T,N], st (KEYS -> [B,..]), prior, kinds (the (e, kind) of edge_pattern), seed).
    The start is gibbs_cases.build's: kalman_oracle.synth_replicate at p = 1, varp_oracle.synth_varp with gibbs_cases._varp_truth at
    p > 1.  Read only."""
    c = case_dict(_row(name))
    N, T, r, p = c["N"], c["T"], c["r"], c["p"]
    idx = NAMES.index(name)
    rate = c["pattern"] if isinstance(c["pattern"], float) else 0.0
    if p == 1:
        reps = [ko.synth_replicate(300 + 10 * idx + b, N, T, r, missing=rate) for b in range(B)]
        x = np.stack([xb for xb, _ in reps])
        st = {k: np.stack([q[k] for _, q in reps]) for k in KEYS}
        st["mu0"] = st["mu0"] + 0.3
    else:
        x = np.stack([vo.synth_varp(300 + 10 * idx + b, N, T, r, p, missing=rate) for b in range(B)])
        tr = [gc._varp_truth(b, N, r, p) for b in range(B)]
        st = {k: np.stack([q[k] for q in tr]) for k in KEYS}
    kinds = set()
    if c["pattern"] == "edge":
        for b in range(B):
            kinds |= edge_pattern(x[b], 0, rc=TC, first=b)
    if c["empty"] is not None:
        x[:, :, c["empty"]] = np.nan
    pr = ge.prior(r)
    if c["A0"]:
        rng = np.random.default_rng([11, idx])
        A0 = 0.1 * rng.standard_normal((B, r, r * p))
        A0[:, :, :r] += 0.5 * np.eye(r)
        pr = ge.prior(r, A0=A0, tau_A=3.0, s_Q=0.7, nu_Q=r + 4.5)
        _frozen(A0)
    st = {k: np.ascontiguousarray(v) for k, v in st.items()}
    out = dict(c, x=np.ascontiguousarray(x), st=st, prior=pr, kinds=kinds, seed=20261020 + 500 + idx)
    _frozen(out["x"], *st.values())
    return out


def chain_prior(c, b):
    """The prior of chain b as gibbs_expect takes it (A0 [r, r p] of the chain)."""
    pr = c["prior"]
    return pr if pr["A0"] is None else dict(pr, A0=pr["A0"][b])


def gamma_margins(c, b, j):
    """Sweep j of chain b on the header's stream: (rejected attempts of stream 6 [N], of stream 9 [r], the smallest distance of a
    taken attempt from its accept boundary).  The Gamma shapes depend on the observed-cell counts and on T - p only, so no sweep
    has to be run (gibbs_cases.attempt_counts; the margin is gibbs_ar_expect.gamma_margin)."""
    N, T, r, p, pr = c["N"], c["T"], c["r"], c["p"], c["prior"]
    key = so.replicate_key(c["seed"], j)
    aR = 0.5 * (pr["nu_R"] + (~np.isnan(c["x"][b])).sum(0))
    aQ = 0.5 * (pr["nu_Q"] + (T - p) - np.arange(r))
    gR, gQ = ge.gamma_attempts(key, 16 * b + 6, N), ge.gamma_attempts(key, 16 * b + 9, r)
    att_R, att_Q = ge.gamma_mt(aR, *gR)[1], ge.gamma_mt(aQ, *gQ)[1]
    return att_R, att_Q, min(gae.gamma_margin(aR, *gR, att_R), gae.gamma_margin(aQ, *gQ, att_Q))


@functools.lru_cache(maxsize=None)
def first_sweep(name, b=0):
    """gibbs_expect.sweep of sweep 0 of chain b from the case's start.  Read only."""
    c = make_case(name)
    o = ge.sweep(c["x"][b], *[c["st"][k][b] for k in KEYS], c["p"], chain_prior(c, b), c["seed"], 0, b)
    _frozen(*[v for v in o.values() if isinstance(v, np.ndarray)])
    return o


def edge_series(c):
    """[B, N] bool: the series with a missing cell (on an edge-pattern row: those the pattern touched)."""
    return apg.edge_series(c)
