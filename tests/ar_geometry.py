"""Launch geometry of the series step of the AR-idiosyncratic ECM (csrc/mstep_ar.hip: mmw_vec_kernel, ar_moments_kernel<R, Q1>,
ar_solve_kernel<R, Q1>), restated in plain Python, and the case table of tests/test_gpu_ar_geometry.py.  Test infrastructure
only: csrc/dfm_argeom.h stays the authority, and tests/test_ar_geometry_cpu.py holds this restatement against that header, compiled
for the host (tests/host/argeom_host.cpp), for every instance and over a sweep of N and T - q.

launch_mstep_ar switches over 38 template instances (r <= 8, q <= 4, r (q + 1) <= 32).  An instance has TT = NTM + (q + 1) NZF tiles
of 16 moment columns (NTM of W = sum E z z', NZF per lag of ZX = sum x z), dealt TPW to a wave over four waves, and takes SGW = 3, 2
or 1 groups of 16 series per workgroup.  The panel block is staged in chunks of 128 periods, in steps of 4 periods, three steps of
B operands in flight; ar_solve_kernel takes 64 series per workgroup; a row of V is VW doubles and mmw_vec_kernel fills it 256
columns per trip, 16 periods per workgroup.

Every reference is computed once per process (functools.lru_cache) and must not be modified by its users."""
import functools
import os
import subprocess

import numpy as np

from oracle import ar_oracle as ao

AR_TC = 128                          # dfm_argeom.h kArTC
AR_PF = 3                            # dfm_argeom.h kArPF
SOLVE_SERIES = 64                    # dfm_argeom.h kArSolveSeries
KEYS = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")

INSTANCES = [(r, q) for q in range(5) for r in range(1, 9) if r * (q + 1) <= 32]       # mstep_ar_supported


def pad_r(n):
    """capi.hip pad_r: the power of two >= n, at least 2."""
    p = 2
    while p < n:
        p <<= 1
    return p


def collapse_max_n(Rp):
    """collapse.hip collapse_max_n: the cross-section the pass with missing cells / EM takes at the padded state width."""
    return 1024 if Rp <= 8 else 512 if Rp <= 16 else 256


def geo(r, q):
    """ArGeo<r, q + 1> and the static deal of its tiles to the four waves (ar_wave_tiles)."""
    q1 = q + 1
    k1 = r * q1
    npr = k1 * (k1 + 1) // 2
    ntm, nzf = (npr + 15) // 16, (k1 + 15) // 16
    tt = ntm + q1 * nzf
    tpw = (tt + 3) // 4
    sgw = 3 if tpw <= 6 else 2 if tpw <= 9 else 1
    nt = tuple(max(0, min(tpw, tt - w * tpw)) for w in range(4))
    # a wave holds both kinds of tile: its first is a W tile, its last a ZX tile
    straddle = any(n > 0 and w * tpw < ntm < w * tpw + n for w, n in enumerate(nt))
    return dict(K1=k1, NTM=ntm, NZF=nzf, TT=tt, TPW=tpw, SGW=sgw, NT=nt, SW=16 * sgw, straddle=straddle)


def launch(r, q, p, N, T):
    """One call of launch_mstep_ar inside dfm_em_ar_batch: the instance's geometry, the workspace widths and the three grids."""
    g = geo(r, q)
    k = r * max(p, q + 1)
    Rk = pad_r(k)
    Tq = T - q
    chunks = (Tq + AR_TC - 1) // AR_TC
    last = Tq - (chunks - 1) * AR_TC
    return dict(g, k=k, Rk=Rk, Tq=Tq, chunks=chunks, last_steps=(last + 3) // 4, VW=16 * g["NTM"] + 16 * ((Rk + 15) // 16),
                ntm16=16 * g["NTM"], Ns=(N + 15) // 16 * 16, vec_blocks=(Tq + 15) // 16, moment_blocks=(N + g["SW"] - 1) // g["SW"],
                solve_blocks=(N + SOLVE_SERIES - 1) // SOLVE_SERIES)


HOST_FIELDS = ("K1", "NTM", "NZF", "TT", "TPW", "SGW", "NT0", "NT1", "NT2", "NT3", "VW", "ntm16", "Ns", "vec_blocks", "moment_blocks",
               "solve_blocks")


def host_tuple(L):
    """The fields of `launch` in the order tests/host/argeom_host.cpp prints them."""
    d = dict(L, NT0=L["NT"][0], NT1=L["NT"][1], NT2=L["NT"][2], NT3=L["NT"][3])
    return tuple(d[f] for f in HOST_FIELDS)


# ------------------------------------------------------------------------------------------------------------- the case table
# (r, q, p, N, T, missing, edge): B = 2 replicates each, two ECM iterations.  Every instance at least once; N and T - q walk the
# edges of the series blocks (48 k, 48 k + 1, 32 k + 1, 16 k + 1), of the solve block (64 / 65) and of the staged chunk (128 / 129,
# three chunks, T - q <= 12).  Every N respects collapse_max_n of the padded state width.
# (6, 0, 5) and (8, 0, 4) run at T = 75 / 70: synth_ar's start fits the VAR(p) of the r principal components by least squares, and at
# T = 35 / 30 its r p = 30 / 32 regressors fit the 30 / 26 usable rows exactly -- the start's Q is zero to rounding (eigenvalues
# 1e-30 .. 1e-26) and 1e-13 of relative noise on the start moves the ORACLE's own two-iteration result by up to 0.4 in Lam and 29 in
# P0, so no bound can be held against it.  tests/test_ar_geometry_cpu.py asks every case for a start the oracle is insensitive to.
CASES = [
    (1, 0, 1, 17, 12, 0.0, 0), (1, 1, 1, 47, 11, 0.0, 0), (1, 2, 4, 48, 131, 0.1, 1), (1, 3, 1, 49, 64, 0.1, 0), (1, 4, 5, 64, 133, 0.0, 1),
    (2, 0, 3, 65, 129, 0.1, 1), (2, 1, 2, 96, 62, 0.0, 0), (2, 2, 1, 97, 61, 0.1, 1), (2, 3, 4, 130, 44, 0.1, 0), (2, 4, 8, 145, 50, 0.0, 0),
    (3, 0, 1, 256, 41, 0.1, 0), (3, 1, 4, 17, 130, 0.1, 1), (3, 2, 3, 47, 261, 0.1, 1), (3, 3, 1, 48, 70, 0.0, 0), (3, 4, 2, 49, 132, 0.1, 1),
    (4, 0, 2, 64, 37, 0.1, 0), (4, 1, 1, 65, 129, 0.0, 0), (4, 2, 8, 96, 55, 0.1, 0), (4, 3, 4, 97, 90, 0.1, 1), (4, 4, 4, 256, 40, 0.05, 0),
    (5, 0, 1, 130, 39, 0.1, 0), (5, 1, 6, 145, 47, 0.1, 0), (5, 2, 3, 17, 131, 0.1, 1), (5, 3, 1, 47, 72, 0.1, 1), (5, 4, 2, 20, 137, 0.1, 1),
    (6, 0, 5, 48, 75, 0.1, 0), (6, 1, 2, 49, 130, 0.1, 1), (6, 2, 1, 65, 80, 0.0, 0), (6, 3, 4, 64, 133, 0.1, 1), (6, 4, 1, 16, 66, 0.1, 0),
    (7, 0, 1, 96, 33, 0.1, 0), (7, 1, 4, 97, 51, 0.1, 1), (7, 2, 3, 145, 135, 0.1, 1), (7, 3, 1, 97, 75, 0.1, 1),
    (8, 0, 4, 47, 70, 0.1, 0), (8, 1, 2, 130, 58, 0.1, 1), (8, 2, 1, 65, 263, 0.1, 1), (8, 3, 1, 49, 131, 0.1, 1),
    (6, 4, 5, 9, 134, 0.0, 0), (8, 3, 4, 40, 77, 0.1, 1), (6, 4, 2, 33, 60, 0.1, 1),
]
CASE_KEYS = ("r", "q", "p", "N", "T", "missing", "edge")
B = 2
MAX_ITER = 2

# the rewritten series of an edge case (panel_and_start)
EDGE_ENOUGH, EDGE_SHORT, EDGE_EMPTY = 3, 5, 7
EDGE_ENOUGH_START, EDGE_SHORT_START = 20, 25
EDGE_FILL = 0.25
EDGE_MASKED_CHUNK_TQ = 140           # beyond it the last series of an edge case has its whole first staged chunk masked


def case_dict(row):
    return dict(zip(CASE_KEYS, row))


def case_id(row):
    r, q, p, N, T, missing, edge = row
    return f"r{r}_q{q}_p{p}_n{N}_t{T}" + ("_edge" if edge else "_bal" if missing == 0.0 else "")


def classes(c):
    """The coverage classes one case hits (the names of REQUIRED)."""
    r, q, p, N, T = c["r"], c["q"], c["p"], c["N"], c["T"]
    L = launch(r, q, p, N, T)
    sgw, SW, Tq, nt = L["SGW"], L["SW"], L["Tq"], L["NT"]
    s = {f"instance={r},{q}", f"SGW={sgw}"}
    if N < SW:
        s.add(f"SGW={sgw}:N<SW")
    if N % SW == 0:
        s.add(f"SGW={sgw}:N%SW==0")
    if L["moment_blocks"] >= 3 and N % SW != 0:
        s.add(f"SGW={sgw}:blocks>=3,partial")
    if N % SW == 1:
        s.add(f"SGW={sgw}:N%SW==1")
    s.add("N%16==0" if N % 16 == 0 else "N%16!=0")
    for name, hit in (("N<64", N < 64), ("N==64", N == 64), ("N==65", N == 65), ("N>128", N > 128)):
        if hit:
            s.add("solve:" + name)
    for name, hit in (("Tq<=12", Tq <= 12), ("Tq==128", Tq == 128), ("Tq==129", Tq == 129), ("chunks=1", L["chunks"] == 1),
                      ("chunks=2", L["chunks"] == 2), ("chunks=3", L["chunks"] == 3)):
        if hit:
            s.add(name)
    s.add(f"Tq%4={Tq % 4}")
    s.add("Tq%16==0" if Tq % 16 == 0 else "Tq%16!=0")
    s.add("p<q+1" if p < q + 1 else "p==q+1" if p == q + 1 else "p>q+1")
    s.add("Rk>k" if L["Rk"] > L["k"] else "Rk==k")
    s.add("VW<=256" if L["VW"] <= 256 else "VW>256")
    if 0 in nt:
        s.add("deal:wave_without_tiles")
    if len(set(nt)) == 1:
        s.add("deal:all_equal")
    if nt[3] == 1:
        s.add("deal:last_wave_one_tile")
    if L["straddle"] and L["NZF"] == 2:
        s.add("deal:wave_with_both_kinds,NZF=2")
    if c["missing"] == 0.0:
        s.add("balanced")
    if c["missing"] == 0.1:
        s.add("missing=0.1")
    if c["edge"]:
        s.add("edge_series")
    return s


REQUIRED = (
    {f"instance={r},{q}" for r, q in INSTANCES}
    | {f"SGW={g}" for g in (1, 2, 3)}
    | {f"SGW={g}:{e}" for g in (1, 2, 3) for e in ("N<SW", "N%SW==0", "blocks>=3,partial", "N%SW==1")}
    | {"N%16==0", "N%16!=0", "solve:N<64", "solve:N==64", "solve:N==65", "solve:N>128"}
    | {"Tq<=12", "chunks=1", "Tq==128", "Tq==129", "chunks=2", "chunks=3", "Tq%4=0", "Tq%4=1", "Tq%4=2", "Tq%4=3", "Tq%16==0", "Tq%16!=0"}
    | {"p<q+1", "p==q+1", "p>q+1", "Rk>k", "Rk==k", "VW<=256", "VW>256"}
    | {"deal:wave_without_tiles", "deal:all_equal", "deal:last_wave_one_tile", "deal:wave_with_both_kinds,NZF=2"}
    | {"balanced", "missing=0.1", "edge_series"}
)


def missing_classes(cases=None):
    """Sorted classes of REQUIRED that no case of `cases` (default CASES) hits; empty when all are covered."""
    hit = set()
    for row in (CASES if cases is None else cases):
        hit |= classes(case_dict(row))
    return sorted(REQUIRED - hit)


# ------------------------------------------------------------------------------------------------------------- panels, expectation
def panel_and_start(c, b):
    """oracle.ar_oracle.synth_ar(b, ..) of the case.  An edge case has four series rewritten:
      series 3   all missing but a run of r + 2 q + 1 finite cells from period 20: exactly r + q + 1 usable quasi-differenced rows, just
                 enough for the series step (a missing cell inside the run becomes 0.25);
      series 5   the same with r + 2 q cells from period 25: one row short, the series is left as is;
      series 7   no observed cell;
      series N - 1 (T - q > 140)  its first 128 + q periods missing: the whole first staged chunk of the series is masked."""
    r, q, p, N, T = c["r"], c["q"], c["p"], c["N"], c["T"]
    x, st = ao.synth_ar(b, N, T, r, p, q, missing=c["missing"])
    if c["edge"]:
        assert N > EDGE_EMPTY + 1 and EDGE_SHORT_START + r + 2 * q <= T
        for i, t0, n in ((EDGE_ENOUGH, EDGE_ENOUGH_START, r + 2 * q + 1), (EDGE_SHORT, EDGE_SHORT_START, r + 2 * q)):
            run = np.where(np.isnan(x[t0:t0 + n, i]), EDGE_FILL, x[t0:t0 + n, i])
            x[:, i] = np.nan
            x[t0:t0 + n, i] = run
        x[:, EDGE_EMPTY] = np.nan
        if T - q > EDGE_MASKED_CHUNK_TQ:
            x[:AR_TC + q, N - 1] = np.nan
    return x, st


def usable_rows(x, q):
    """Per series, the number of periods where x_it and its q lags are observed."""
    T = x.shape[0]
    return (~np.isnan(np.stack([x[q - l:T - l] for l in range(q + 1)], axis=2)).any(axis=2)).sum(0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def expected(row):
    """The batch of a case and what the oracle makes of it: panel [B, T, N], start {key: [B, ..]}, and per replicate the pass at the
    start (kfs_pass_ar: loglik, f_smooth[:, :r], the packed leading r x r block of P_smooth) and two ECM iterations (em_ar: the
    parameters, the likelihood path, f_smooth[:, :r])."""
    c = case_dict(row)
    r = c["r"]
    xs, sts = zip(*[panel_and_start(c, b) for b in range(B)])
    panel = np.stack(xs)
    start = {k: np.stack([s[k] for s in sts]) for k in KEYS}
    tri = np.tril_indices(r)
    passes, ems = [], []
    for b in range(B):
        o = ao.kfs_pass_ar(panel[b], **{k: start[k][b] for k in KEYS})
        passes.append(dict(loglik=float(o["loglik"]), f=np.ascontiguousarray(o["f_smooth"][:, :r]),
                           P=np.ascontiguousarray(o["P_smooth"][:, :r, :r][:, tri[0], tri[1]])))
        est, path, out = ao.em_ar(panel[b], {k: start[k][b] for k in KEYS}, max_iter=MAX_ITER)
        ems.append(dict(est=est, path=path, f=np.ascontiguousarray(out["f_smooth"][:, :r])))
        _frozen(passes[-1]["f"], passes[-1]["P"], path, ems[-1]["f"], *est.values())
    _frozen(panel, *start.values())
    return dict(panel=panel, start=start, passes=tuple(passes), ems=tuple(ems))


def watched_series(c):
    """Series whose update an un-updated or mis-addressed series could not imitate: 0, the first of every moment block, the first of
    the second solve block, N - 1."""
    L = launch(c["r"], c["q"], c["p"], c["N"], c["T"])
    s = {0, c["N"] - 1} | {j * L["SW"] for j in range(L["moment_blocks"])}
    if c["N"] > SOLVE_SERIES:
        s.add(SOLVE_SERIES)
    return sorted(s)


# ------------------------------------------------------------------------------------------------------------- the host check
SWEEP_INSTANCES = ((4, 4), (8, 2), (8, 3))          # SGW = 3, 2, 1
SWEEP_N = range(1, 301)
SWEEP_TQ = range(2, 401)


def build_argeom_host(directory):
    """tests/host/argeom_host.cpp, which includes csrc/dfm_argeom.h and nothing else of the library, compiled with g++."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "argeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "argeom_host.cpp")], check=True)
    return exe


def ask_argeom_host(exe, requests):
    """One process for all `requests` (r, q, N, T, Rk): the printed fields of each (HOST_FIELDS), as int tuples."""
    text = "".join(" ".join(map(str, q)) + "\n" for q in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests)
    return [tuple(map(int, line.split())) for line in out]
