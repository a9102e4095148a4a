"""Launch geometry of the series step of the mixed-frequency EM (csrc/mstep_mf.hip: mf_loadings_kernel, mf_table_kernel,
mf_moments_kernel<2|3|4>, mf_solve_kernel<1..8>; csrc/mstep_mf_blocks.hip: mf_solve_blocks_kernel<1..8>) and the host-side dealing
of the series into weight classes and class-pure tiles (capi.hip: mf_classes), restated in plain Python, and the case tables of
tests/test_gpu_mf_geometry.py.  Test infrastructure only: csrc/dfm_mfgeom.h stays the authority, and
tests/test_mf_geometry_cpu.py holds this restatement against that header, compiled for the host (tests/host/mfgeom_host.cpp).

A class row of the table V (and a series row of OUT) is VW = 16 ceil(r (r + 1) / 32) + 16 columns: vech(E g g') packed lower, zeros
up to VW - 16, the r means, zeros; TT = VW / 16 tiles (2 for r <= 5, 3 for r = 6, 7, 4 for r = 8).  The distinct rows of W are the
classes, numbered by their first series; every class's series are dealt, in index order, into tiles of 16 with -1 padding, four
tiles (waves) to a workgroup of mf_moments_kernel, which walks the periods in groups of 16, one group loaded ahead, the rows past
T - 1 clamped and masked.  mf_table_kernel runs a thread per (period, column), mf_solve_kernel a thread per series, both in
workgroups of 256 with the replicate in blockIdx.y; mf_loadings_kernel a thread per entry of the expanded loadings of the batch.

The cases build their weights directly as custom rows (the model takes any W): a class is (weights, size, period), period 3 = observed
in the third month of a quarter only.  Every reference is computed once per process (functools.lru_cache) and must not be modified
by its users."""
import functools
import os
import subprocess

import numpy as np

from tests import mf_blocks_expect as mb
from tests import mf_expect as me

KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
MF_MAX_CLASSES, MF_MAX_LAGS = 8, 5    # dfm_mfgeom.h kMfMaxClasses, kMfMaxLags
TILE, WAVES, GROUP, BLOCK = 16, 4, 16, 256   # kMfTile, kMfWaves, kMfGroup, kMfBlock
MAX_ITER = 2
START_SCALE = 0.7                    # the start's loadings: that much of the loadings the panel was drawn from
STOP_SCALE = 0.3                     # ... of the replicates of a stop case that start further away


# ------------------------------------------------------------------------------------------------------------- the geometry
def row_width(r):
    """mf_row_width."""
    return 16 * ((r * (r + 1) // 2 + 15) // 16) + 16


def col_kinds(r):
    """mf_col_kind of every column of a row: 1 an entry of vech, 2 an entry of the mean, 0 a zero."""
    VW, npk = row_width(r), r * (r + 1) // 2
    return [1] * npk + [0] * (VW - 16 - npk) + [2] * r + [0] * (16 - r)


def vech_cols(r):
    """mf_vech_col(c, d), c >= d, in the order (0, 0), (1, 0), (1, 1), ..: packed lower, row after row."""
    return [c * (c + 1) // 2 + d for c in range(r) for d in range(c + 1)]


def mean_cols(r):
    return [row_width(r) - 16 + c for c in range(r)]


def pad_r(n):
    """capi.hip pad_r: the power of two >= n, at least 2 (the padded width of the companion state)."""
    p = 2
    while p < n:
        p <<= 1
    return p


def deal(W):
    """mf_deal: (status, C, class rows, class of every series, tile_class, tile_series [ntiles][16])."""
    W = np.asarray(W, float)
    N = W.shape[0]
    rows, cls = [], []
    for i in range(N):
        if not np.isfinite(W[i]).all():
            return dict(rc=1, C=0, ntiles=0, Wc=[], cls=[], tile_class=[], tile_series=[])
        w = tuple(W[i])
        if w not in rows:                                          # (-0.0 == 0.0 and 0.0 hashes like -0.0: exact comparison, as ==)
            if len(rows) == MF_MAX_CLASSES:
                return dict(rc=2, C=0, ntiles=0, Wc=[], cls=[], tile_class=[], tile_series=[])
            rows.append(w)
        cls.append(rows.index(w))
    tile_class, tile_series = [], []
    for c in range(len(rows)):
        members = [i for i in range(N) if cls[i] == c]
        for k in range(0, len(members), TILE):
            part = members[k:k + TILE]
            tile_class.append(c)
            tile_series.append(part + [-1] * (TILE - len(part)))
    return dict(rc=0, C=len(rows), ntiles=len(tile_class), Wc=rows, cls=cls, tile_class=tile_class, tile_series=tile_series)


def grids(N, L, r, T, B, Rk):
    """Workgroups (x) of mf_loadings_kernel, mf_table_kernel and mf_solve_kernel / mf_solve_blocks_kernel; the groups of 16 periods."""
    VW = row_width(r)
    return dict(VW=VW, TT=VW // 16, ngroups=(T + GROUP - 1) // GROUP, loadings=(B * N * Rk + BLOCK - 1) // BLOCK,
                table=(T * VW + BLOCK - 1) // BLOCK, solve=(N + BLOCK - 1) // BLOCK)


def host_tuple(N, L, r, T, B, Rk, W):
    """The fields of a request in the order tests/host/mfgeom_host.cpp prints them."""
    g, d = grids(N, L, r, T, B, Rk), deal(W)
    out = [g["VW"], g["TT"], g["ngroups"], g["loadings"], g["table"], (d["ntiles"] + WAVES - 1) // WAVES, g["solve"], d["rc"], d["C"],
           d["ntiles"]]
    out += col_kinds(r) + vech_cols(r) + mean_cols(r) + d["tile_class"] + [i for t in d["tile_series"] for i in t]
    out += [int(round(w * 1e6)) for row in d["Wc"] for w in row]
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------- the case tables
M2, M3, M4, M5 = (1.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 0.0)
AVG3 = (1 / 3, 1 / 3, 1 / 3)
FLOW = me.WEIGHTS["q_flow"]


def _case(name, B, r, p, T, classes, order, thin=(), first=None, seed=0):
    """classes: [(weights, size, period)]; order: "sorted" (class after class) | "interleaved" (a seeded permutation; first = the
    class of series 0; seed: of the panels); thin: [(class, member, cells)]: the member-th series of that class keeps its first `cells` observed cells."""
    return dict(name=name, B=B, r=r, p=p, T=T, classes=tuple(classes), order=order, thin=tuple(thin), first=first, seed=seed)


# One case per line of the issue's list, at the smallest shapes: see classes() for what each claims.
CASES = [
    # T = 7: one group, T VW = 224 <= 256 (one workgroup of the table kernel, partly idle); a class of 1 in a tile of its own,
    # quarterly with n_i = 2 = r + 1; the monthly class of 15
    _case("r1_t7", 1, 1, 1, 7, [(M2, 15, 1), ((0.5, 0.5), 1, 3)], "sorted"),
    # T = 13: one group; series 0 quarterly (NaN two months of three) while the monthly class's second tile has 15 padding lanes
    # that read it; a class with w_0 = 0; four tiles of three classes in one workgroup; p = L
    _case("r2_t13", 3, 2, 2, 13, [((0.5, 0.5), 1, 3), (M2, 17, 1), ((0.0, 1.0), 16, 1)], "interleaved", first=0),
    # T = 16: one whole group, T VW = 512 (two whole workgroups of the table kernel); r = 5 (15 of 16 vech columns); five tiles:
    # a second workgroup with three waves past ntiles; the all-zero class (G_i = 0: kept)
    _case("r5_t16", 1, 5, 1, 16, [((1.0,), 33, 1), ((2.0,), 15, 1), ((0.0,), 3, 1)], "sorted"),
    # T = 17: a last group of one live period; n_i = 0, and n_i = r and r + 1 side by side in a monthly and in a quarterly tile; p > L
    _case("r3_t17", 5, 3, 3, 17, [(M2, 20, 1), ((0.5, 0.5), 12, 3)], "interleaved",
          thin=[(0, 2, 3), (0, 3, 4), (0, 5, 0), (1, 2, 3), (1, 3, 4)]),
    # T = 18: a last group of two; no padding lane at all (16, 16, 32); w_0 = 0; p < L
    _case("r4_t18", 1, 4, 1, 18, [(M3, 16, 1), (AVG3, 16, 3), ((0.0, 1.0, 0.0), 32, 1)], "sorted"),
    # T = 31 (= 3 mod 4, a last group of 15); r = 6, TT = 3; L = 5 (state 30)
    _case("r6_t31", 1, 6, 1, 31, [(M5, 17, 1), (FLOW, 7, 3)], "interleaved"),
    # T = 32: two whole groups; r = 7, 28 of 32 vech columns; L = 4
    _case("r7_t32", 3, 7, 2, 32, [(M4, 15, 1), ((0.25, 0.25, 0.25, 0.25), 9, 3)], "sorted"),
    # T = 33: a third group of one period; r = 8, TT = 4; C = 8 at L = 4 = p (state 32); class sizes 1, 15, 16, 17; nine tiles;
    # the first workgroup holds four classes; an all-zero class
    _case("r8_t33_c8", 1, 8, 4, 33,
          [(M4, 1, 1), ((0.25, 0.25, 0.25, 0.25), 15, 1), ((0.0, 1.0, 0.0, 0.0), 16, 1), ((1.0, 1.0, 0.0, 0.0), 17, 1),
           ((1 / 3, 2 / 3, 2 / 3, 1 / 3), 5, 3), ((0.0, 0.0, 0.0, 0.0), 3, 1), ((0.5, 0.0, 0.5, 0.0), 4, 1), ((0.0, 0.0, 1.0, 1.0), 6, 1)],
          "sorted"),
    # N = 256: one whole workgroup of the solve; sixteen tiles
    _case("n256_t13", 1, 2, 1, 13, [(M3, 240, 1), (AVG3, 16, 3)], "interleaved"),
    # N = 257: the second workgroup of mf_solve_kernel holds one series; 32, 33 and 192 series; seventeen tiles; p > L = 1
    _case("n257_t7", 1, 1, 2, 7, [((1.0,), 32, 1), ((2.0,), 33, 1), ((0.5,), 192, 1)], "interleaved"),
    # one class
    _case("c1_t20", 1, 3, 1, 20, [((1.0,), 17, 1)], "sorted"),
]
BLOCKS_CASES = ("n257_t7", "r8_t33_c8", "r5_t16")                 # the same tile edges under mf_solve_blocks_kernel
PROFILE_CASE = "r2_t13"
# (case, tol, max_iter, replicates that start from STOP_SCALE x the loadings): B = 4.  The model stops after (4, 5, 5, 5),
# (5, 6, 6, 6) and (6, 7, 7, 5) iterations: the first stopper is replicate 0, replicate 0 and the last replicate.
STOP_CASES = [
    (_case("stop_r1", 4, 1, 1, 60, [(M3, 12, 1), (AVG3, 6, 3)], "sorted"), 3e-4, 40, (1, 2, 3)),
    (_case("stop_r5", 4, 5, 1, 70, [(M3, 20, 1), (AVG3, 8, 3)], "sorted"), 1e-3, 40, (1, 2, 3)),
    (_case("stop_r8", 4, 8, 1, 70, [(M3, 24, 1), (AVG3, 8, 3)], "sorted"), 1e-3, 40, (0, 1, 2)),
]
BY_NAME = {c["name"]: c for c in CASES}
BY_NAME.update({c["name"]: c for c, _, _, _ in STOP_CASES})


def layout(case):
    """The series order of a case: (labels [N] = the class of the table each series belongs to, W [N][L], period [N], thinned
    {series: cells})."""
    sizes = [s for _, s, _ in case["classes"]]
    lab = np.repeat(np.arange(len(sizes)), sizes)
    if case["order"] == "interleaved":
        lab = lab[np.random.default_rng([7, len(lab), case["T"]]).permutation(len(lab))]
        if case["first"] is not None:
            j = int(np.nonzero(lab == case["first"])[0][0])
            lab[0], lab[j] = lab[j], lab[0]
    W = np.array([case["classes"][c][0] for c in lab], float)
    period = np.array([case["classes"][c][2] for c in lab])
    thin = {int(np.nonzero(lab == c)[0][j]): n for c, j, n in case["thin"]}
    return lab, W, period, thin


def geometry(case):
    lab, W, period, thin = layout(case)
    N, L = W.shape
    d = deal(W)
    g = grids(N, L, case["r"], case["T"], case["B"], pad_r(case["r"] * max(case["p"], L)))
    return dict(g, N=N, L=L, deal=d, lab=lab, W=W, period=period, thin=thin)


def zero_class_series(case):
    lab = layout(case)[0]
    return [int(i) for i in range(len(lab)) if not any(case["classes"][lab[i]][0])]


def classes(case):
    """The coverage classes a case claims, from its geometry alone."""
    g = geometry(case)
    d, N, L, r, p, T, B = g["deal"], g["N"], g["L"], case["r"], case["p"], case["T"], case["B"]
    s = {f"r={r}", f"TT={g['TT']},r={r}", f"L={L}", "p<L" if p < L else "p=L" if p == L else "p>L", f"C={d['C']}", f"B={B}",
         f"ntiles%4={d['ntiles'] % 4}", f"T={T}"}
    assert r * max(p, L) <= 32
    for w in d["Wc"]:
        if not any(w):
            s.add("class:zero")
        elif w[0] == 0.0:
            s.add("class:w0=0")
    sizes = [d["cls"].count(c) for c in range(d["C"])]
    s |= {f"size={n}" for n in sizes}
    if d["ntiles"] >= 5:
        s.add("ntiles>=5")
    if d["ntiles"] > 4 and d["ntiles"] % 4:
        s.add("wg:second_with_waves_past_ntiles")
    if any(len(set(d["tile_class"][k:k + 4])) == 4 for k in range(0, d["ntiles"], 4)):
        s.add("wg:four_classes")
    contiguous = all(np.all(np.diff(np.nonzero(np.array(d["cls"]) == c)[0]) == 1) for c in range(d["C"]))
    if d["C"] > 1:
        s.add("order:sorted" if contiguous else "order:interleaved")
    padded = {d["tile_class"][k] for k in range(d["ntiles"]) if -1 in d["tile_series"][k]}
    if padded:
        s.add("pad:idx=-1")
    if any(t.count(-1) == 15 for t in d["tile_series"]):
        s.add("tile:one_live_lane")
    if g["period"][0] == 3 and padded - {d["cls"][0]}:
        s.add("s0:nan_under_padding_of_another_class")
    if T <= 16:
        s.add("T:one_group")
    if T % 2:
        s.add("T:odd")
    if T % 4 == 3:
        s.add("T%4=3")
    if 1 <= T % 16 <= 3:
        s.add("T:last_group_1..3")
    if T * g["VW"] <= 256:
        s.add("table:one_block")
    if T * g["VW"] % 256 == 0:
        s.add("table:whole_blocks")
    if N in (256, 257):
        s.add(f"N={N}")
    thin = g["thin"]
    if 0 in thin.values():
        s.add("n=0")
    for t in d["tile_series"]:
        ns = {thin[i] for i in t if i in thin}
        if {r, r + 1} <= ns:
            s.add("n=r,r+1:" + ("quarterly" if g["period"][t[0]] == 3 else "monthly") + "_tile")
    if T % 16:
        s.add("mutant:tail")
    if d["C"] > 1:
        s.add("mutant:tile0")
    if r in thin.values():
        s.add("mutant:n>=r")
    return s


REQUIRED = (
    {f"r={r}" for r in range(1, 9)} | {"TT=2,r=1", "TT=2,r=5", "TT=3,r=6", "TT=3,r=7", "TT=4,r=8"} | {f"L={L}" for L in range(1, 6)}
    | {"p<L", "p=L", "p>L"} | {f"C={c}" for c in (1, 2, 3, 8)} | {"class:zero", "class:w0=0"} | {f"size={n}" for n in (1, 15, 16, 17, 32, 33)}
    | {f"ntiles%4={k}" for k in range(4)} | {"ntiles>=5", "wg:second_with_waves_past_ntiles", "wg:four_classes", "order:sorted",
                                             "order:interleaved", "pad:idx=-1", "tile:one_live_lane", "s0:nan_under_padding_of_another_class"}
    | {f"T={t}" for t in (7, 13, 16, 17, 18, 31, 32, 33)} | {"T:one_group", "T:odd", "T%4=3", "T:last_group_1..3", "table:one_block",
                                                             "table:whole_blocks", "N=256", "N=257"}
    | {f"B={b}" for b in (1, 3, 5)} | {"n=0", "n=r,r+1:monthly_tile", "n=r,r+1:quarterly_tile"}
    | {"mutant:tail", "mutant:tile0", "mutant:n>=r"}
)


def missing_classes(required, cases):
    hit = set()
    for case in cases:
        hit |= classes(case)
    return sorted(required - hit)


def watched_series(case):
    """Series whose update an un-updated or mis-addressed series could not imitate: series 0 and N - 1, the first and the last live
    series of every tile (the series in a tile's only live lane among them), series 255 and 256, the series at n_i = r + 1."""
    g = geometry(case)
    w = {0, g["N"] - 1} | {i for i in (255, 256) if i < g["N"]} | {i for i, n in g["thin"].items() if n == case["r"] + 1}
    for t in g["deal"]["tile_series"]:
        live = [i for i in t if i >= 0]
        w |= {live[0], live[-1]}
    return sorted(w)


# ------------------------------------------------------------------------------------------------------------- panels, expectation
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _replicate(case, b, scale):
    """A seeded panel of replicate b on the case's weights and the start of its EM: the loadings the panel was drawn from times
    `scale`, unit variances, the transition it was drawn from, a unit P0."""
    lab, W, period, thin = layout(case)
    N, L = W.shape
    r, p, T = case["r"], case["p"], case["T"]
    m = max(p, L)
    rng = np.random.default_rng([20240, case["seed"], b, N, T, r, p])
    wl = 0.5 ** np.arange(1, p + 1); wl = 0.8 * wl / wl.sum()
    Avar = np.hstack([np.diag(np.linspace(0.6, 1.0, r)) * wl[l] * (1.0 if l % 2 == 0 else -1.0) for l in range(p)])
    qd = np.linspace(0.5, 1.0, r)
    f = np.zeros((T + 60, r))
    for t in range(p, T + 60):
        f[t] = Avar @ np.concatenate([f[t - 1 - l] for l in range(p)]) + np.sqrt(qd) * rng.standard_normal(r)
    Lam = rng.standard_normal((N, r))
    Lam += 0.5 * np.sign(Lam)                                      # no loading near zero: 0.3 of it is still a move
    g = np.stack([sum(W[i, l] * f[60 - l:T + 60 - l] for l in range(L)) @ Lam[i] for i in range(N)], axis=1)
    x = g + np.sqrt(rng.uniform(0.3, 1.0, N)) * rng.standard_normal((T, N))
    if T >= 16:                                                    # a few missing cells in the monthly series
        x[:, period == 1] = np.where(rng.random((T, int((period == 1).sum()))) < 0.05, np.nan, x[:, period == 1])
    x[np.ix_(np.arange(T) % 3 != 2, period == 3)] = np.nan
    for i, n in thin.items():
        keep = np.nonzero(~np.isnan(x[:, i]))[0][:n]
        assert len(keep) == n
        col = x[keep, i].copy()
        x[:, i] = np.nan
        x[keep, i] = col
    start = dict(Lam=scale * Lam, R=np.ones(N), Avar=Avar, Q=np.diag(qd), mu0=np.zeros(r * m), P0=np.eye(r * m))
    return x, start


@functools.lru_cache(maxsize=None)
def batch(name, slow=()):
    """(panel [B, T, N], W [N, L], start {key: [B, ..]}) of a case; the replicates in `slow` start from STOP_SCALE x the loadings."""
    case = BY_NAME[name]
    reps = [_replicate(case, b, STOP_SCALE if b in slow else START_SCALE) for b in range(case["B"])]
    panel = np.stack([x for x, _ in reps])
    start = {k: np.stack([s[k] for _, s in reps]) for k in KEYS}
    W = np.ascontiguousarray(layout(case)[1])
    _frozen(panel, W, *start.values())
    return panel, W, start


def kept_series(name):
    """The series the series step must leave as they are, in every replicate: n_i < r + 1, and the all-zero class (G_i = 0)."""
    case = BY_NAME[name]
    panel = batch(name)[0]
    n = (~np.isnan(panel)).sum(1)                                  # [B][N]
    few = np.nonzero((n < case["r"] + 1).all(0))[0]
    assert np.array_equal(few, np.nonzero((n < case["r"] + 1).any(0))[0])
    return sorted({int(i) for i in few} | set(zero_class_series(case)))


def _packed(P, r):
    il = np.tril_indices(r)
    return P[:, :r, :r][:, il[0], il[1]]


def _freeze_em(res, r):
    est, path, out = res
    e = dict(est=est, path=path, f=np.ascontiguousarray(out["f_smooth"][:, :r]), P=_packed(out["P_smooth"], r))
    _frozen(path, e["f"], e["P"], *est.values())
    return e


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per replicate, two iterations of the NumPy model (tests/mf_expect.py em_mf) from the case's start."""
    case = BY_NAME[name]
    panel, W, start = batch(name)
    ems = tuple(_freeze_em(me.em_mf(panel[b], {k: start[k][b] for k in KEYS}, W, max_iter=MAX_ITER), case["r"]) for b in range(case["B"]))
    return dict(panel=panel, W=W, start=start, ems=ems)


@functools.lru_cache(maxsize=None)
def expected_blocks(name):
    """The same case under the mask of mf_blocks_expect.case_mask (fixed entries of the start zero, a 1 at (0, 0)), against
    mf_blocks_expect.em_mf_blocks."""
    case = BY_NAME[name]
    panel, W, start = batch(name)
    free = mb.case_mask(W.shape[0], case["r"])
    start = dict(start, Lam=np.where(free[None], start["Lam"], 0.0))
    start["Lam"][:, 0, 0] = 1.0
    _frozen(free, start["Lam"])
    ems = tuple(_freeze_em(mb.em_mf_blocks(panel[b], {k: start[k][b] for k in KEYS}, W, free, max_iter=MAX_ITER), case["r"])
                for b in range(case["B"]))
    return dict(panel=panel, W=W, free=free, start=start, ems=ems)


@functools.lru_cache(maxsize=None)
def expected_stop(k):
    """Stop case k: the model's EM with the stop rule, replicate by replicate."""
    case, tol, max_iter, slow = STOP_CASES[k]
    panel, W, start = batch(case["name"], slow)
    ems = tuple(_freeze_em(me.em_mf(panel[b], {key: start[key][b] for key in KEYS}, W, max_iter=max_iter, tol=tol), case["r"])
                for b in range(case["B"]))
    return dict(panel=panel, W=W, start=start, ems=ems)


# ------------------------------------------------------------------------------------------------------------- wrong kernels, noise
MUTANTS = {"tail": "mutant:tail", "tile0": "mutant:tile0", "n>=r": "mutant:n>=r"}


def em_variant(x, params, W, max_iter=MAX_ITER, mutant=None, reverse=False):
    """em_mf with the series step restated beside the model's: reverse=True takes the time sums of G_i, b_i and sum x^2 from the
    last observed period to the first; mutant = "tail": the last T mod 16 periods are ignored (a last group never run);
    "tile0": every series takes the weights of tile 0's class; "n>=r": a series is updated from n_i = r on."""
    x = np.asarray(x, float)
    T, N = x.shape
    r, L = params["Lam"].shape[1], W.shape[1]
    cur = {k: np.array(v, float) for k, v in params.items()}
    live = T - T % 16 if mutant == "tail" else T
    need = r if mutant == "n>=r" else r + 1
    path, out = [], None
    for _ in range(max_iter):
        new, ll, out = me.em_step_mf(x, W=W, **cur)
        path.append(ll)
        zs, Ps = out["f_smooth"], out["P_smooth"]
        m = zs.shape[1] // r
        Ez = zs[:, :, None] * zs[:, None, :] + Ps
        zb = zs.reshape(T, m, r)[:, :L]
        Eb = Ez.reshape(T, m, r, m, r)[:, :L, :, :L, :]
        Lam, R = cur["Lam"].copy(), cur["R"].copy()
        for i in range(N):
            idx = np.nonzero(~np.isnan(x[:live, i]))[0]
            if reverse:
                idx = idx[::-1]
            n = len(idx)
            if n < need:
                continue
            w = W[0] if mutant == "tile0" else W[i]
            G = np.einsum("l,tlcmd,m->cd", w, Eb[idx], w)
            b = np.einsum("l,tlc->tc", w, zb[idx]).T @ x[idx, i]
            try:
                np.linalg.cholesky(G)
            except np.linalg.LinAlgError:
                continue
            lam = np.linalg.solve(G, b)
            Lam[i] = lam
            R[i] = ((x[idx, i] ** 2).sum() - 2.0 * lam @ b + lam @ G @ lam) / n
        cur = dict(new, Lam=Lam, R=R)
    return cur, np.array(path), out


# ------------------------------------------------------------------------------------------------------------- the host check
def build_mfgeom_host(directory):
    """tests/host/mfgeom_host.cpp, which includes csrc/dfm_mfgeom.h and nothing else of the library, compiled with g++."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "mfgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "mfgeom_host.cpp")], check=True)
    return exe


def ask_mfgeom_host(exe, requests):
    """One process for all the requests (N, L, r, T, B, Rk, W): the printed fields of each, as int tuples."""
    text = "".join(f"{N} {L} {r} {T} {B} {Rk} " + " ".join(repr(float(w)) for w in np.asarray(W).ravel()) + "\n"
                   for N, L, r, T, B, Rk, W in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests), (len(out), len(requests))
    return [tuple(map(int, line.split())) for line in out]
