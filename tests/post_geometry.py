"""Launch geometry of the post-estimation cell kernels, restated in plain Python, and the case table of
tests/test_gpu_post_geometry.py.  Test infrastructure only: cell_geometry of csrc/dfm_cellgeom.h stays the authority, and
tests/test_post_geometry_cpu.py holds this restatement against that function, compiled for the host
(tests/host/cellgeom_host.cpp), over the case tables and a sweep of every call site's inputs.

The cell kernels (forecast_fill_kernel, simsmooth_diff_kernel / simsmooth_fill_kernel, news_cov_panel_kernel,
news_impact_kernel, sv_hd_fill_kernel) share one geometry: a workgroup owns one replicate (pass replicate), a chunk of RC rows
and a block of NPB lanes, each lane one series (SP = 1) or one pair of adjacent series; G row groups of NPB lanes are rounded up
to whole waves.  The host entry points stage every array 256-byte aligned, so the 16-byte path (SP = 2 / VEC) is taken exactly
when N is even (and, for the forecast, R <= 16)."""
import os
import subprocess

FC_MAX_THREADS = 512                 # forecast.hip kFcFillMaxThreads
FC_LDS = 48 * 1024                   # forecast.hip kFcFillLds
SS_MAX_THREADS = 512                 # simsmooth.hip kSsMaxThreads
SS_LDS = 32 * 1024                   # simsmooth.hip kSsLds
NW_MAX_THREADS = 512                 # news.hip kNwMaxThreads
NW_LDS = 32 * 1024                   # news.hip kNwLds

GEOM_FIELDS = ("NPB", "G", "RC", "nchunk", "nsblk", "threads")       # struct CellGeom


def cell_geometry(lanes, row_doubles, rows, max_threads, lds_bytes):
    """cell_geometry of dfm_cellgeom.h, the one restatement: blocks of at most 256 lanes, the row-group count G that idles the
    fewest lanes of the workgroup's whole waves, RC = max(1, min(8 G, LDS cap, rows)) rows per chunk."""
    nsblk = (lanes + 255) // 256
    npb = (lanes + nsblk - 1) // nsblk
    best, best_g = -1.0, 1
    g = 1
    while g * npb <= max_threads:
        th = (g * npb + 63) // 64 * 64
        if th > max_threads:
            break
        eff = g * npb / th
        if eff > best + 1e-9:
            best, best_g = eff, g
        g += 1
    rc = max(1, min(8 * best_g, lds_bytes // (8 * row_doubles), rows))
    return dict(NPB=npb, G=best_g, RC=rc, nchunk=(rows + rc - 1) // rc, nsblk=nsblk, threads=(best_g * npb + 63) // 64 * 64)


def _summary(kernel, call, grid, **extra):
    """One kernel's launch: `call` = the arguments of cell_geometry at its call site."""
    lanes, row_doubles, rows, _, lds_bytes = call
    g = cell_geometry(*call)
    return dict(g, kernel=kernel, rows=rows, grid=grid(g), cap=lds_bytes // (8 * row_doubles), call=call,
                idle_last=g["nsblk"] * g["NPB"] > lanes, cap_binds=g["RC"] < 8 * g["G"] and g["RC"] < rows,
                partial_last=g["nchunk"] > 1 and rows % g["RC"] != 0, **extra)


def forecast_fill(B, N, r, T, H, aligned=True):
    """forecast.hip launch_fill_r (SP: even N and R <= 16 with 16-byte aligned pointers) for forecast_fill_kernel<R, SP> over
    T + H rows of R + R (R + 1) / 2 staged doubles; the bucket is R = r itself.  The grid is one-dimensional: B * nchunk * nsblk
    workgroups."""
    sp = 2 if N % 2 == 0 and r <= 16 and aligned else 1
    call = ((N + sp - 1) // sp, r + r * (r + 1) // 2, T + H, FC_MAX_THREADS, FC_LDS)
    return _summary("forecast_fill_kernel", call, lambda g: (B * g["nchunk"] * g["nsblk"], 1, 1), SP=sp, R=r, vec=sp == 2)


def rb_bucket(r):
    """The loadings register bucket of launch_cells (simsmooth.hip), launch_news_cov_panel and launch_news_impact (news.hip):
    dispatch_r_bucket of dfm_cellgeom.h."""
    return 4 if r <= 4 else 8 if r <= 8 else 16 if r <= 16 else 32


def simsmooth_cells(B, D, N, r, T, H, fill):
    """simsmooth.hip launch_cells<FILL>: column pairs, r doubles per row, rows = T (difference kernel) or T + H (fill kernel);
    grid (B D, nchunk, nsblk) for a call of at most 8192 pass replicates."""
    call = ((N + 1) // 2, r, T + H if fill else T, SS_MAX_THREADS, SS_LDS)
    name = "simsmooth_fill_kernel" if fill else "simsmooth_diff_kernel"
    return _summary(name, call, lambda g: (B * D, g["nchunk"], g["nsblk"]), RB=rb_bucket(r), vec=N % 2 == 0)


def news_cells(B, G, N, r, T, impact):
    """news.hip launch_news_cov_panel (grid (B G, nchunk, nsblk)) or launch_news_impact (grid (B G, nsblk): one workgroup walks
    all T rows, RC at a time): column pairs, r doubles per row, T rows."""
    call = ((N + 1) // 2, r, T, NW_MAX_THREADS, NW_LDS)
    name = "news_impact_kernel" if impact else "news_cov_panel_kernel"
    grid = (lambda g: (B * G, g["nsblk"], 1)) if impact else (lambda g: (B * G, g["nchunk"], g["nsblk"]))
    return _summary(name, call, grid, RB=rb_bucket(r), vec=N % 2 == 0)


def news_gamma_kb(r, p):
    """launch_news_gamma (news.hip): news_gamma_kernel<KB, NT> with KB >= k = r p."""
    k = r * p
    return 8 if k <= 8 else 16 if k <= 16 else 32


def news_horizon(T, targets):
    """The horizon dfm_news_batch runs its forecasts over (capi.hip news_check)."""
    return max(0, max(t for t, _ in targets) + 1 - T)


# ------------------------------------------------------------------------------------------------------------- the case table
# One row per GPU case: every product (forecast, simsmooth with D = 2, news) runs on the same panel and parameters.
#   name, B, N, T, r, p, H, missing, scaled (mean / sd given), route (the pass route the panel is meant to take)
# Why some shapes are what they are:
#   * dfm_news_batch runs two of its three forecasts with DFM_F_MAY_HAVE_MISSING, and the pass with missing cells takes N <= 1024
#     at r <= 8 and N <= 512 at r <= 16 (capi.hip check_general_n).  Three column-pair blocks need N > 1024, so the nsblk >= 3 case
#     of the pair kernels runs at r > 16 (the plain model at Rp = 32 takes any N).
#   * The LDS cap of the pair kernels (32 KiB / 8 r rows) binds only with many row groups (small NPB) and more rows than the cap.
#   * The mixed batch is test_gpu_chunk's construction: replicate 0 has 12 series (padded to 200 with all-missing series), whose
#     filter forgets its start too slowly for the time-chunked recursion, replicate 1 has 200.
CASES = [
    # name          B  N     T    r   p   H   miss  scaled route
    ("n514_r8",     2, 514,  34,  8,  1,  12, 0.0,  False, "wide"),
    ("n1025_r17",   2, 1025, 24,  17, 1,  9,  0.0,  True,  "wide"),
    ("n514_r32",    2, 514,  12,  32, 1,  4,  0.0,  False, "wide"),
    ("n52_r32_cap", 2, 52,   130, 32, 1,  0,  0.1,  True,  "general_r32"),
    ("n200_r9",     2, 200,  40,  9,  1,  40, 0.0,  False, "wide"),
    ("n64_r16",     2, 64,   32,  16, 1,  1,  0.05, True,  "general_r16"),
    ("n139_r20",    2, 139,  30,  20, 1,  3,  0.1,  False, "tile"),
    ("n60_r8",      2, 60,   30,  8,  1,  0,  0.0,  True,  "fused"),
    ("n77_r3",      2, 77,   60,  3,  1,  6,  0.1,  False, "chunked"),
    ("n41_r5_seq",  2, 41,   20,  5,  1,  12, 0.1,  True,  "sequential"),
    ("n40_r1_p12",  2, 40,   40,  1,  12, 40, 0.05, False, "mbf16"),
    ("n40_r4_p4",   2, 40,   36,  4,  4,  41, 0.1,  True,  "comp"),
    ("n40_r6_p4",   2, 40,   36,  6,  4,  3,  0.05, False, "companion"),
    ("n41_r8_p4",   2, 41,   50,  8,  4,  2,  0.0,  True,  "companion"),
    ("mixed",       2, 200,  120, 8,  1,  5,  0.2,  False, "chunked_fallback"),
]
CASE_KEYS = ("name", "B", "N", "T", "r", "p", "H", "missing", "scaled", "route")

ROUTES = ("fused", "wide", "chunked", "tile", "comp", "mbf16", "sequential", "chunked_fallback")


def case_dict(row):
    return dict(zip(CASE_KEYS, row))


def targets(c):
    """The news targets of a case: t* = 0, 31, 32, T - 1, T, T + H - 1 and the columns 0, 1 (the second of a pair), N - 1 and the
    first column of the last column-pair block, paired up in turn until every time and every column has appeared."""
    T, N, H = c["T"], c["N"], c["H"]
    times = sorted({0, 31, 32, T - 1, T, T + H - 1})
    nw = news_cells(1, 1, N, c["r"], T, impact=True)
    cols = sorted({0, 1, N - 1, 2 * (nw["nsblk"] - 1) * nw["NPB"]})
    n = max(len(times), len(cols))
    return [(times[j % len(times)], cols[j % len(cols)]) for j in range(n)]


def geometries(c):
    """{family: [kernel summaries]} of one case, as the host entry points launch them."""
    B, N, T, r, p, H = c["B"], c["N"], c["T"], c["r"], c["p"], c["H"]
    tg = targets(c)
    return dict(
        forecast=[forecast_fill(B, N, r, T, H)],
        simsmooth=[simsmooth_cells(B, 2, N, r, T, H, fill=False), simsmooth_cells(B, 2, N, r, T, H, fill=True)],
        news=[news_cells(B, len(tg), N, r, T, impact=False), news_cells(B, len(tg), N, r, T, impact=True)],
    )


def classes(c):
    """{family: set of coverage classes} that one case hits (the class names of REQUIRED)."""
    T, r, p, H = c["T"], c["r"], c["p"], c["H"]
    out = {}
    for fam, geos in geometries(c).items():
        s = set()
        for g in geos:
            s.add("nsblk=1" if g["nsblk"] == 1 else "nsblk=2" if g["nsblk"] == 2 else "nsblk>=3")
            if g["idle_last"]:
                s.add("idle_last_block")
            s.add("vec" if g["vec"] else "scalar")
            if g["RC"] == g["rows"]:
                s.add("rc=rows")
            elif g["cap_binds"]:
                s.add("rc=cap")
            else:
                s.add("rc=8G")
            if g["partial_last"]:
                s.add("partial_chunk")
        if fam == "forecast":
            s.add("R=1-4" if r <= 4 else "R=5-8" if r <= 8 else "R=9-16" if r <= 16 else "R=17-32")
            s.add(f"r={r}")
        else:
            s.add(f"RB={rb_bucket(r)}")
        hz = news_horizon(T, targets(c)) if fam == "news" else H
        if hz == 0:
            s.add("H=0")
        if hz == 1:
            s.add("H=1")
        if hz >= 40:
            s.add("H>=40,p=1" if p == 1 else "H>=40,p>1")
        if T + hz in (32, 33):
            s.add(f"T+H={T + hz}")
        if fam == "news":
            s.add(f"KB={news_gamma_kb(r, p)},{'p=1' if p == 1 else 'p>1'}")
        s.add("route=" + c["route"])
        out[fam] = s
    return out


_ROUTES = {"route=" + x for x in ROUTES}
_GEOM = {"nsblk=1", "nsblk=2", "nsblk>=3", "idle_last_block", "vec", "scalar", "rc=8G", "rc=cap", "rc=rows", "partial_chunk"}
REQUIRED = dict(
    forecast=_GEOM | _ROUTES | {"R=1-4", "R=5-8", "R=9-16", "R=17-32", "r=9", "r=16", "r=17", "r=32",
                                "H=0", "H=1", "H>=40,p=1", "H>=40,p>1", "T+H=32", "T+H=33"},
    simsmooth=_GEOM | _ROUTES | {"RB=4", "RB=8", "RB=16", "RB=32",
                                 "H=0", "H=1", "H>=40,p=1", "H>=40,p>1", "T+H=32", "T+H=33"},
    # (news: targets at t* = T and t* = 32 are always asked for, so its horizon is >= 1 and T + H >= 33)
    news=_GEOM | _ROUTES | {"RB=4", "RB=8", "RB=16", "RB=32", "KB=8,p=1", "KB=16,p=1", "KB=16,p>1", "KB=32,p=1", "KB=32,p>1",
                            "H=1", "H>=40,p=1", "H>=40,p>1", "T+H=33"},
)


def missing_classes(cases=None):
    """{family: sorted classes of REQUIRED that no case of `cases` (default CASES) hits}; empty lists when all are covered."""
    hit = {fam: set() for fam in REQUIRED}
    for row in (CASES if cases is None else cases):
        for fam, s in classes(case_dict(row)).items():
            hit[fam] |= s
    return {fam: sorted(REQUIRED[fam] - hit[fam]) for fam in REQUIRED}


# ------------------------------------------------------------------------------------------------------------- the host check
SWEEP_N = range(1, 1101)
SWEEP_R = (1, 4, 5, 8, 9, 16, 17, 20, 32)
SWEEP_ROWS = (1, 7, 8, 39, 40, 41, 400)


def build_cellgeom_host(directory):
    """tests/host/cellgeom_host.cpp, which includes csrc/dfm_cellgeom.h and nothing else of the library, compiled with g++."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), "cellgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "cellgeom_host.cpp")], check=True)
    return exe


def ask_cellgeom_host(exe, requests):
    """One process for all `requests` ((kind, int, ..) with kind = cell | irf | path | sp): the printed fields of each, as int
    tuples."""
    text = "".join(" ".join(map(str, q)) + "\n" for q in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests)
    return [tuple(map(int, line.split())) for line in out]


def check_sp_rule(exe, restated, bucket=lambda r: r):
    """`restated(N, r, aligned)`, a launcher's SP as a test module restates it, against cell_sp of dfm_cellgeom.h at the launcher's
    register bucket: N in SWEEP_N, r in SWEEP_R, aligned and misaligned.  Returns the set of SP values seen."""
    q = [(N, r, al) for N in SWEEP_N for r in SWEEP_R for al in (1, 0)]
    got = ask_cellgeom_host(exe, [("sp", N, bucket(r), al) for N, r, al in q])
    bad = [(x, g[0], restated(x[0], x[1], bool(x[2]))) for x, g in zip(q, got) if g[0] != restated(x[0], x[1], bool(x[2]))]
    assert not bad, bad[:5]
    return {g[0] for g in got}
