"""Launch geometry of the series kernels of the model with AR(q) idiosyncratic terms -- forecast_ar_back_kernel / forecast_ar_fwd_kernel
(csrc/forecast_ar.hip), simsmooth_ar_diff_kernel / simsmooth_ar_fwd_kernel (csrc/simsmooth_ar.hip), gibbs_ar_series_kernel
(csrc/gibbs_ar.hip), filter_ar_kernel / filter_ar_fill_kernel / filter_ar_eval_kernel (csrc/filter_ar.hip) -- as the host entries launch
them, the template instances the admission rules of csrc/capi.hip can reach, a missing-cell pattern keyed to the staged-chunk edge, and
the case table of tests/test_gpu_ar_post_geometry.py with the coverage classes it must hit.  Test infrastructure only.

series_geometry and the fill's geometry are not restated here: forecast_ar_expect.geometry and filter_ar_expect.fill_launch are the
restatements, held against csrc/dfm_cellgeom.h by tests/host/seriesgeom_host.cpp and tests/host/filter_ar_geom_host.cpp;
tests/test_ar_post_geometry_cpu.py puts every launch of `launches` through those two programs.

A series kernel owns one replicate and a block of NPB series, a lane each, and walks the rows in chunks of RC = min(32, LDS cap, n)
staged rows.  The LDS cap never binds: the widest staged row is the forecast's forward row at r = 16, 16 + 136 = 152 doubles, 40 rows
of 48 KiB -- so there is no rc=cap class for the series kernels (the fill has one).  What crosses a chunk edge: the backward message
(Om, eta, seen, the prefetched cell) and the forward state (a, P) in registers, the Gibbs run-length counter in a register and the q lag
rows of gb_ar_stage in LDS.

Every reference is computed once per process (functools.lru_cache) and must not be modified by its users."""
import functools

import numpy as np

from tests import ar_geometry as ag
from tests import filter_ar_expect as fte
from tests import forecast_ar_expect as fe
from tests import gibbs_ar_expect as gae
from tests import simsmooth_ar_expect as sae

KEYS = fe.KEYS
B = 2
D = 2                                # draws per replicate of the path-draw product
SWEEPS = 3                           # sweeps of the Gibbs product
SEED = 20160415                      # the path draws' seed
EVAL_H_MAX = 3                       # the filter product evaluates min(H, 3) horizons: the evaluation walks origins, not horizons
SERIES_LDS = 48 * 1024               # kFcArLds, kSsArLds, kGbArLds
SSAR_TAIL = 64                       # dfm_fcar.h kSsArLdsTail, doubles behind the staged rows of the two draw kernels
EVAL_CHUNK = 64                      # dfm_filter.h kFtEvalChunk
RC = 32                              # dfm_cellgeom.h kSeriesChunkRows


# ------------------------------------------------------------------------------------------------------------- admission, instances
def ar_admits(r, p, q):
    """capi.hip ar_check with the entries' own q >= 1: 1 <= q <= 4 and r max(p, q + 1) <= 32 (DFM_MAX_R)."""
    return r >= 1 and p >= 1 and 1 <= q <= 4 and r * max(p, q + 1) <= 32


def gibbs_admits(r, p, q):
    """capi.hip gibbs_ar_check: ar_check's limits and r <= 8."""
    return ar_admits(r, p, q) and r <= 8


def max_n(r, p, q):
    """capi.hip check_general_n at the state width k = r max(p, q + 1): collapse_max_n of the padded k."""
    return ag.collapse_max_n(ag.pad_r(r * max(p, q + 1)))


def rb_series(r):
    """launch_fc_ar_r (forecast_ar.hip), launch_ssar_diff_q (simsmooth_ar.hip), launch_filter_ar_eval (filter_ar.hip): the loadings'
    register bucket."""
    return 4 if r <= 4 else 8 if r <= 8 else 16


_RB_FIRST_R = {4: 1, 8: 5, 16: 9}    # the smallest r of each bucket

# ar_check: r (q + 1) <= 32 at p = 1, so q admits r <= 32 // (q + 1) = 16, 10, 8, 6 -- the 16 bucket (r >= 9) at q = 1 and 2 only.
# (3, 16) and (4, 16) are compiled by launch_fc_ar and launch_simsmooth_ar_diff and can never be reached.
SERIES_INSTANCES = [(q, rb) for q in (1, 2, 3, 4) for rb in (4, 8, 16) if _RB_FIRST_R[rb] <= 32 // (q + 1)]
COMPILED_UNREACHABLE = [(3, 16), (4, 16)]
# gibbs_ar_check: r <= 8 on top of ar_check, so both buckets of launch_gibbs_ar_q at every q (r = 5 is admitted at q = 4: 25 <= 32).
GIBBS_INSTANCES = [(q, rb) for q in (1, 2, 3, 4) for rb in (4, 8) if _RB_FIRST_R[rb] <= min(8, 32 // (q + 1))]
# ar_check admits r <= 16 (at q = 1): all three buckets of launch_filter_ar_eval.
EVAL_INSTANCES = [rb for rb in (4, 8, 16) if _RB_FIRST_R[rb] <= 32 // 2]
# launch_filter_ar_fill: the bucket of w = r (q + 1) in 2 .. 32 (dispatch_r_bucket); cell_sp gives SP = 2 only in a bucket <= 16.
FILL_INSTANCES = [(wb, sp) for wb in (4, 8, 16, 32) for sp in (1, 2) if sp == 1 or wb <= 16]


# ------------------------------------------------------------------------------------------------------------- launches
def _series(kernel, Q, RB, N, row, n, lds=SERIES_LDS):
    """One series kernel as launch_fc_ar_q / launch_ssar_diff_q / launch_gibbs_ar_q launch it: `call` = series_geometry's arguments."""
    NPB, G, rc, nchunk, nsblk, threads = fe.geometry(N, row, n, lds_bytes=lds)
    return dict(kernel=kernel, Q=Q, RB=RB, NPB=NPB, G=G, RC=rc, nchunk=nchunk, nsblk=nsblk, threads=threads, n=n, call=(N, row, n, lds),
                idle_last=nsblk * NPB > N,                               # lanes behind series N - 1 in the last block
                ragged_wave=threads > NPB,                               # lanes behind the block's NPB series in its last wave
                paired=tuple((s * NPB) % 2 == 0 for s in range(nsblk)),  # SsArIdio: the block starts at an even series
                last_partner_idle=any((s * NPB) % 2 == 0 and (min(N, (s + 1) * NPB) - s * NPB) % 2 == 1 for s in range(nsblk)))


def _draw_kernels(N, r, q, n):
    """dfm_simsmooth_ar_batch on n output rows: the difference kernel, the backward messages, the forward filter that writes the draw."""
    rb, tail = rb_series(r), SERIES_LDS - 8 * SSAR_TAIL
    return [_series("simsmooth_ar_diff_kernel", q, rb, N, r, n, tail), _series("forecast_ar_back_kernel", q, rb, N, r, n),
            _series("simsmooth_ar_fwd_kernel", q, rb, N, 2 * r, n, tail)]


def products(c):
    """The products that admit the case's shape."""
    out = ["forecast", "simsmooth", "filter"]
    if gibbs_admits(c["r"], c["p"], c["q"]) and c["T"] - c["q"] > c["p"]:
        out.append("gibbs")
    return out


def launches(c):
    """{product: [kernel summaries]} of one case, as the host entries launch them (every optional output asked for)."""
    N, T, r, p, q, H = c["N"], c["T"], c["r"], c["p"], c["q"], c["H"]
    rb, n = rb_series(r), T + H - q
    k, w = r * max(p, q + 1), r * (q + 1)
    out = dict(
        forecast=[_series("forecast_ar_back_kernel", q, rb, N, r, n),
                  _series("forecast_ar_fwd_kernel", q, rb, N, r + r * (r + 1) // 2, n)],
        simsmooth=_draw_kernels(N, r, q, n),
        filter=[dict(kernel="filter_ar_kernel", k=k, w=w, Rp=ag.pad_r(k), n=T - q),
                dict(fte.fill_launch(B, N, r, q, T), w=w, n=T - q)])
    eh = eval_horizons(c)
    if eh > 0:
        origins = max(T - 1 - c["t0"], 0)
        out["filter"].append(dict(kernel="filter_ar_eval_kernel", RB=rb, nsblk=(N + 255) // 256, threads=256, origins=origins,
                                  chunks=(origins + EVAL_CHUNK - 1) // EVAL_CHUNK, H=eh))
    if "gibbs" in products(c):
        # a sweep draws the factor path by dfm_simsmooth_ar_batch_dev (D = 1, H = 0), then the series step on the T - q rows
        grb = 4 if r <= 4 else 8
        out["gibbs"] = _draw_kernels(N, r, q, T - q) + [_series("gibbs_ar_series_kernel", q, grb, N, grb, T - q, SERIES_LDS - 8 * q * grb)]
    return out


# ------------------------------------------------------------------------------------------------------------- the edge pattern
EDGE_KINDS = ("gap over the rows either side of the edge", "gap whose last cell is the row before the edge",
              "gap whose first cell is the row behind the edge", "gap of q + 1 cells from the row before the edge",
              "observed only in the row before the edge", "observed only in the row behind the edge", "observed only in the last panel row",
              "output row 0 and the row behind the edge missing")
N_EDGE_KINDS = len(EDGE_KINDS)


def edge_pattern(x, q, rc=RC, first=0):
    """Missing cells keyed to the staged-chunk edge, in place on x [T, N]: series i gets kind (i + first) % N_EDGE_KINDS at the edge
    e = rc (output rows e - 1 | e; output row t is panel row q + t), every second group of N_EDGE_KINDS series at e = 2 rc where the
    panel has the rows for the kind there.  A panel too short for a kind leaves that series balanced.  Returns the set of (e, kind)
    used.  Kinds 4 .. 6 leave one observed cell: the series' `last` is e - 1, e or the last row, and kind 6 puts a message on every
    row of every chunk."""
    T, N = x.shape
    nx = T - q
    need = (lambda e: e + 2, lambda e: e + 1, lambda e: e + 2, lambda e: e + q + 1, lambda e: e, lambda e: e + 1, lambda e: e + 1,
            lambda e: e + 2)
    used = set()
    for i in range(N):
        kind = (i + first) % N_EDGE_KINDS
        e = 2 * rc if (i // N_EDGE_KINDS) % 2 == 1 and nx >= need[kind](2 * rc) else rc
        if nx < need[kind](e):
            continue
        col = x[:, i]
        if kind == 0:
            col[q + e - 1:q + e + 1] = np.nan
        elif kind == 1:
            col[q + e - 3:q + e] = np.nan
        elif kind == 2:
            col[q + e:q + e + min(2, nx - e - 1)] = np.nan
        elif kind == 3:
            col[q + e - 1:q + e + q] = np.nan
        elif kind in (4, 5, 6):
            row = q + e - 1 if kind == 4 else q + e if kind == 5 else T - 1
            keep = col[row]
            col[:] = np.nan
            col[row] = keep
        else:
            col[q] = np.nan
            col[q + e] = np.nan
        used.add((e, kind))
    return used


# ------------------------------------------------------------------------------------------------------------- the case table
# name, N, T, r, p, q, H, t0 (None: q), pattern ("edge", a first kind of forecast_ar_expect.apply_pattern, None: balanced), scaled.
# B = 2 replicates.  Every row runs every product that admits its shape on one panel and one set of parameters: the forecast, the
# path draws with D = 2, the filter (min(H, 3) evaluation horizons from origin t0) and, at r <= 8 and T - q > p, three Gibbs sweeps.
# n = T + H - q output rows for the forecast and the draws, T - q for the filter and the Gibbs sweeps.  Every N respects
# collapse_max_n of the padded state width (forecasts and draws always run the pass with missing cells).
CASES = [
    # (1,16); k = w = 32; n = 72: three chunks, both edges; eval RB 16; fill WB 32 under its LDS cap.  Its classes are those of
    # r16_p1_n64 (the instance), r9_n33 (the evaluation bucket) and r10_q2 (the fill) together: it stays as the one row that walks the
    # full bucket r = 16 over three chunks, with the edge pattern on both edges, a horizon, and mean / sd
    ("r16_p2",      40,  70, 16, 2, 1, 3,  None, "edge", True),
    # (1,16) at n = 64 exactly; odd N below a wave; H = 0
    ("r16_p1_n64",  33,  65, 16, 1, 1, 0,  None, "edge", False),
    # the first r of the 16 bucket; k = 27 in Rp = 32, w = 18 < k; n = 33: a second chunk of one row
    ("r9_n33",      64,  33, 9,  3, 1, 1,  None, 3,      True),
    # (2,16); k = w = 30
    ("r10_q2",      41,  45, 10, 1, 2, 2,  None, "edge", False),
    # (1,8); two blocks of 129: the second starts at an odd series; n = 65; a horizon longer than a chunk; fill (16,2) on 129 lanes
    ("r8_n258_n65", 258, 36, 8,  2, 1, 30, None, "edge", True),
    # (2,8); w = 15; T - q = n = 33: the Gibbs walks' second chunk of one row, whose q lag rows are the first chunk's last
    ("r5_q2_n33",   139, 35, 5,  1, 2, 0,  None, 0,      False),
    # (4,8); k = w = 30
    ("r6_q4",       20,  40, 6,  1, 4, 2,  None, "edge", True),
    # (3,8) with p > q + 1; three chunks (see ar_geometry.CASES on starts with a singular Q: make_case fits the start on a longer panel)
    ("r6_q3_p5",    24,  80, 6,  5, 3, 1,  None, "edge", False),
    # (1,4); three blocks of 171: the second starts at an odd series, the third at an even one again, its last series beside an idle lane
    ("r4_n513",     513, 20, 4,  1, 1, 2,  None, 5,      True),
    # (3,4); three blocks of 172, all paired, two idle lanes in the last; w = 8; fill (8,2) in two blocks; n = 34
    ("r2_q3_n514",  514, 37, 2,  1, 3, 0,  None, "edge", False),
    # (3,8) at k = 32; n = 32 exactly: one full chunk and no second
    ("r8_q3_n32",   65,  35, 8,  1, 3, 0,  None, None,   True),
    # (2,4); T - q = 32: the horizon of the draws starts on the chunk edge; w = 9, the bottom of fill bucket 16
    ("drawedge",    24,  34, 3,  2, 2, 6,  None, "edge", False),
    # exactly 64 evaluation origins; fill (4,2)
    ("eval64",      24,  70, 2,  2, 1, 3,  5,    "edge", True),
    # 65 origins, a second evaluation chunk of one; odd N: fill (4,1)
    ("eval65",      25,  70, 2,  2, 1, 3,  4,    "edge", True),
    # (4,4); n = 2 <= q + 1: the recursions end before their state is full; fill rows below a chunk
    ("q4_n2",       12,  6,  2,  1, 4, 0,  None, 0,      False),
]
CASE_KEYS = ("name", "N", "T", "r", "p", "q", "H", "t0", "pattern", "scaled")
NAMES = [row[0] for row in CASES]


def case_dict(row):
    c = dict(zip(CASE_KEYS, row))
    if c["t0"] is None:
        c["t0"] = c["q"]
    return c


def eval_horizons(c):
    return min(c["H"], EVAL_H_MAX)


def _row(name):
    return CASES[NAMES.index(name)]


# ------------------------------------------------------------------------------------------------------------- coverage classes
def _edge_kinds(c):
    """The (e, kind) the case's panel carries, from the pattern alone (no synthesis): edge_pattern on a dummy panel."""
    if c["pattern"] != "edge":
        return set()
    used = set()
    for b in range(B):
        used |= edge_pattern(np.zeros((c["T"], c["N"])), c["q"], first=b)
    return used


def classes(c):
    """{product: set of coverage classes} one case hits (the names of REQUIRED)."""
    out = {}
    kinds = _edge_kinds(c)
    for prod, ks in launches(c).items():
        s = set()
        for g in (g for g in ks if "Q" in g):                            # the series kernels
            if g["kernel"] == "gibbs_ar_series_kernel" or prod != "gibbs":
                s.add(f"instance={g['Q']},{g['RB']}")
            if g["kernel"] != "gibbs_ar_series_kernel" and c["r"] in (4, 5, 8, 9, 16):
                s.add(f"RB={g['RB']}:r={c['r']}")                        # the first and the last r of a loadings bucket
            s.add("nsblk=1" if g["nsblk"] == 1 else "nsblk=2" if g["nsblk"] == 2 else "nsblk>=3")
            if g["idle_last"]:
                s.add("idle_last_block")
            if g["ragged_wave"]:
                s.add("ragged_wave")
            n = g["n"]
            if n in (32, 33, 64, 65):
                s.add(f"n={n}")
            if g["nchunk"] >= 3:
                s.add("chunks>=3")
            if n <= c["q"] + 1:
                s.add("n<=q+1")
            s.add("p<q+1" if c["p"] < c["q"] + 1 else "p=q+1" if c["p"] == c["q"] + 1 else "p>q+1")
            if prod in ("simsmooth", "gibbs"):
                s |= {"block_start=paired" if pr else "block_start=unpaired" for pr in g["paired"]}
                if len(g["paired"]) >= 3 and not g["paired"][1] and g["paired"][2]:
                    s.add("third_block=paired")
                if g["last_partner_idle"]:
                    s.add("paired:partner_idle")
            # an edge kind counts where the walk has rows behind the edge: n >= e + 2
            s |= {f"edge@{e}:{kind}" for e, kind in kinds if n >= e + 2}
        if prod == "simsmooth" and c["H"] > 0 and (c["T"] - c["q"]) % RC == 0:
            s.add("nx_on_chunk_edge")
        if prod == "filter":
            core, fill = ks[0], ks[1]
            k, w, Rp = core["k"], core["w"], core["Rp"]
            if k > 16 and k & (k - 1):
                s.add("k_not_pow2_above_16")
            if Rp == 32:
                s.add("Rp=32:w<k" if w < k else "Rp=32:w=k")
            if w in (8, 9, 16, 18, 32):
                s.add(f"w={w}")
            s.add(f"fill={fill['WB']},{fill['SP']}")
            s.add("fill:vec" if fill["vec"] else "fill:scalar")
            s.add("fill:rc=rows" if fill["RC"] == fill["rows"] else "fill:rc=cap" if fill["cap_binds"] else "fill:rc=8G")
            if fill["partial_last"]:
                s.add("fill:partial_chunk")
            s.add("fill:nsblk=1" if fill["nsblk"] == 1 else "fill:nsblk=2" if fill["nsblk"] == 2 else "fill:nsblk>=3")
            for g in ks[2:]:
                s.add(f"eval={g['RB']}")
                s.add("eval:nsblk=1" if g["nsblk"] == 1 else "eval:nsblk=2" if g["nsblk"] == 2 else "eval:nsblk>=3")
                if g["origins"] in (64, 65):
                    s.add(f"origins={g['origins']}")
        out[prod] = s
    return out


_SERIES = ({f"instance={q},{rb}" for q, rb in SERIES_INSTANCES}
           | {"nsblk=1", "nsblk=2", "nsblk>=3", "idle_last_block", "ragged_wave", "n=32", "n=33", "n=64", "n=65", "chunks>=3", "n<=q+1",
              "p<q+1", "p=q+1", "p>q+1"}
           | {f"edge@{RC}:{kind}" for kind in range(N_EDGE_KINDS)} | {f"edge@{2 * RC}:{kind}" for kind in (0, 4, 5)})
_BUCKET_EDGES = {"RB=4:r=4", "RB=8:r=5", "RB=8:r=8", "RB=16:r=9", "RB=16:r=16"}
_BLOCKS = {"block_start=paired", "block_start=unpaired", "third_block=paired", "paired:partner_idle"}
REQUIRED = dict(
    forecast=_SERIES | _BUCKET_EDGES,
    simsmooth=_SERIES | _BUCKET_EDGES | _BLOCKS | {"nx_on_chunk_edge"},
    # the sweeps walk the T - q panel rows, and r <= 8 keeps their cases apart from the r = 16 rows that hold n = 64 and n = 65: the
    # second edge is met in a three-chunk walk instead
    gibbs=({f"instance={q},{rb}" for q, rb in GIBBS_INSTANCES} | _BLOCKS | {"RB=4:r=4", "RB=8:r=5", "RB=8:r=8"}
           | {"nsblk=1", "nsblk=2", "nsblk>=3", "idle_last_block", "ragged_wave", "n=32", "n=33", "chunks>=3", "n<=q+1",
              "p<q+1", "p=q+1", "p>q+1"}
           | {f"edge@{RC}:{kind}" for kind in range(N_EDGE_KINDS)} | {f"edge@{2 * RC}:{kind}" for kind in (0, 4, 5)}),
    filter=({f"eval={rb}" for rb in EVAL_INSTANCES} | {f"fill={wb},{sp}" for wb, sp in FILL_INSTANCES}
            | {"k_not_pow2_above_16", "Rp=32:w<k", "Rp=32:w=k", "origins=64", "origins=65", "w=8", "w=9", "w=16", "w=18", "w=32"}
            | {"fill:vec", "fill:scalar", "fill:rc=8G", "fill:rc=cap", "fill:rc=rows", "fill:partial_chunk",
               "fill:nsblk=1", "fill:nsblk=2", "fill:nsblk>=3", "eval:nsblk=1", "eval:nsblk=2", "eval:nsblk>=3"}),
)


def missing_classes(cases=None):
    """{product: sorted classes of REQUIRED that no case of `cases` (default CASES) hits}; empty lists when all are covered."""
    hit = {prod: set() for prod in REQUIRED}
    for row in (CASES if cases is None else cases):
        for prod, s in classes(case_dict(row)).items():
            hit[prod] |= s
    return {prod: sorted(REQUIRED[prod] - hit[prod]) for prod in REQUIRED}


# ------------------------------------------------------------------------------------------------------------- inputs, expectations
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of a case: dict(case fields, x [B,T,N], st (KEYS -> [B,..]), v0 [B,N], mean, sd ([B,N] or None), kinds (the (e, kind)
    of edge_pattern or the kinds of apply_pattern), prior, seed).  The start is forecast_ar_expect.synth's, fitted on a panel long
    enough for its VAR(p) regression to leave a well-conditioned Q (2 r p + 2 r + 20 rows at least), then cut to T rows.  Read only."""
    c = case_dict(_row(name))
    N, T, r, p, q = c["N"], c["T"], c["r"], c["p"], c["q"]
    xs, sts, v0s, kinds = [], [], [], set()
    for b in range(B):
        x, st, v0 = fe.synth(b + 3, max(N, r + 2), max(T, 3 * r + 12, 2 * r * p + 2 * r + 20), r, p, q)
        x = np.ascontiguousarray(x[:T, :N])
        st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
        if c["pattern"] == "edge":
            kinds |= edge_pattern(x, q, first=b)
        elif c["pattern"] is not None:
            kinds |= fe.apply_pattern(x, q, c["pattern"] + b)
        xs.append(x); sts.append(st); v0s.append(v0[:N])
    rng = np.random.default_rng([5, N, T, q])
    mean, sd = rng.standard_normal((B, N)), rng.uniform(0.5, 2.0, (B, N))
    out = dict(c, x=np.stack(xs), st={k: np.ascontiguousarray(np.stack([s[k] for s in sts])) for k in KEYS}, v0=np.stack(v0s),
               mean=mean if c["scaled"] else None, sd=sd if c["scaled"] else None, kinds=kinds, prior=gae.prior(r),
               seed=20261020 + 300 + NAMES.index(name))
    _frozen(out["x"], out["v0"], out["mean"], out["sd"], *out["st"].values())
    return out


def _scales(c, b):
    return dict(mean=None if c["mean"] is None else c["mean"][b], sd=None if c["sd"] is None else c["sd"][b])


@functools.lru_cache(maxsize=None)
def forecast_expected(name, H=None):
    """Per replicate, forecast_ar_expect.expect of the case (at the case's H, or another one)."""
    c = make_case(name)
    out = [fe.expect(c["x"][b], *[c["st"][k][b] for k in KEYS], c["H"] if H is None else H, v0=c["v0"][b], **_scales(c, b))
           for b in range(B)]
    for e in out:
        _frozen(*[v for v in e.values() if isinstance(v, np.ndarray)])
    return out


@functools.lru_cache(maxsize=None)
def draws_expected(name):
    """(f [B, D, n, r], x [B, D, n, N]): simsmooth_ar_expect.draw of the case on the header's stream."""
    c = make_case(name)
    fs, xs = [], []
    for b in range(B):
        out = [sae.draw(c["x"][b], *[c["st"][k][b] for k in KEYS], c["H"], SEED, 0, d, b, v0=c["v0"][b], **_scales(c, b)) for d in range(D)]
        fs.append(np.stack([o[0] for o in out])); xs.append(np.stack([o[1] for o in out]))
    f, x = np.stack(fs), np.stack(xs)
    _frozen(f, x)
    return f, x


@functools.lru_cache(maxsize=None)
def filter_expected(name):
    """Per replicate, filter_ar_expect.expect of the case."""
    c = make_case(name)
    out = [fte.expect(c["x"][b], *[c["st"][k][b] for k in KEYS], H=eval_horizons(c), t0=c["t0"], **_scales(c, b)) for b in range(B)]
    for e in out:
        _frozen(*e.values())
    return out


@functools.lru_cache(maxsize=None)
def gibbs_chains(name):
    """The model's own chains of a Gibbs case: [b][j] -> the dict of gibbs_ar_expect.sweep, sweep j started from the model's state after
    sweep j - 1."""
    c = make_case(name)
    out = []
    for b in range(B):
        cur = {k: c["st"][k][b] for k in KEYS}
        sweeps = []
        for j in range(SWEEPS):
            o = gae.sweep(c["x"][b], *[cur[k] for k in KEYS], c["prior"], c["seed"], j, b)
            sweeps.append(o)
            cur = dict(cur, Lam=o["Lam"], sig2=o["sig2"], rho=o["rho"], Avar=o["A"], Q=o["Q"])
        out.append(sweeps)
    return out


def edge_series(c):
    """[B, N] bool: the series of an edge-pattern case whose cells the pattern touched."""
    x = c["x"]
    return np.isnan(x).any(axis=1)
