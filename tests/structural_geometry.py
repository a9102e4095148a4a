"""Launch geometry of the structural kernels (csrc/structural.hip) restated in plain Python, and the case table of
tests/test_gpu_structural.py.  Test infrastructure only: the C++ stays the authority, and tests/test_structural_cpu.py pins this
restatement to the constants the source states and to the functions of csrc/dfm_cellgeom.h, compiled for the host."""
from tests.post_geometry import cell_geometry

IRF_LANES = 128                      # structural.hip kSvIrfLanes
FILL_MAX_THREADS = 512               # kSvFillMaxThreads
FILL_LDS = 48 * 1024                 # kSvFillLds
PATH_MAX_THREADS = 1024              # kSvPathMaxThreads
PATH_LDS = 48 * 1024                 # kSvPathLds


def irf_fill(B, N, r, H, cum, aligned=True):
    """launch_irf_r / irf_geometry (dfm_cellgeom.h): sv_irf_fill_kernel<R, SP>, one workgroup per (replicate, series block), RC
    Theta rows per LDS chunk (two tables with cum)."""
    sp = 2 if N % 2 == 0 and r <= 16 and aligned else 1
    lanes = (N + sp - 1) // sp
    nsblk = (lanes + IRF_LANES - 1) // IRF_LANES
    npb = (lanes + nsblk - 1) // nsblk
    rc = min((FILL_LDS - 32 * 8) // (r * r * (2 if cum else 1) * 8), H)
    return dict(SP=sp, nsblk=nsblk, NPB=npb, G=1, threads=(npb + 63) // 64 * 64, RC=rc, nchunk=(H + rc - 1) // rc, grid=B * nsblk)


def hd_fill(B, N, r, T, aligned=True):
    """launch_hd_r: sv_hd_fill_kernel<R, SP> with cell_geometry (r doubles per staged row) over B (r + 1) slabs of T rows."""
    sp = 2 if N % 2 == 0 and r <= 16 and aligned else 1
    g = cell_geometry((N + sp - 1) // sp, r, T, FILL_MAX_THREADS, FILL_LDS)
    return dict(g, SP=sp, grid=B * (r + 1) * g["nchunk"] * g["nsblk"])


def path(r, p):
    """path_geometry (dfm_cellgeom.h): CP chains of r p lanes per workgroup, TC rows staged between two write-outs."""
    k = r * p
    cp = min(PATH_MAX_THREADS // k, r + 1)
    tc = (PATH_LDS // 8 - 2 * cp * k) // (cp * r + r)
    tc = max(1, min(32, tc))
    return dict(CP=cp, groups=(r + 1 + cp - 1) // cp, TC=tc, threads=(cp * k + 63) // 64 * 64,
                lds=(2 * cp * k + tc * (cp * r + r)) * 8)


# ------------------------------------------------------------------------------------------------------------- the case tables
# IRF / FEVD: name, N, r, p, H, named, cum, sd, unit_effect, fevd, misaligned (irf pointer 8 bytes off on the _dev entry)
IRF_CASES = [
    ("r1_n7_h1", 7, 1, 1, 1, True, False, False, False, True, False),
    ("r2_n60_h2", 60, 2, 1, 2, True, True, True, True, True, False),
    ("r4_n139_h12", 139, 4, 1, 12, True, True, True, False, True, False),
    ("r8_n200_h41", 200, 8, 1, 41, True, True, True, True, True, False),
    ("r8_n200_misaligned", 200, 8, 1, 12, True, False, False, False, True, True),
    ("r9_n513_chol", 513, 9, 1, 12, False, True, False, False, True, False),
    ("r16_n200_nofevd", 200, 16, 1, 12, True, False, True, False, False, False),
    ("r17_n200_unit", 200, 17, 1, 2, True, False, False, True, True, False),
    ("r32_n1025_chunks", 1025, 32, 1, 12, True, True, True, False, True, False),
    ("r32_n60_h41", 60, 32, 1, 41, True, False, False, True, True, False),
    ("var2_r3", 60, 3, 2, 12, True, True, False, False, True, False),
    ("var4_r4", 139, 4, 4, 41, True, False, True, True, True, False),
    ("var3_r2_chol", 7, 2, 3, 12, False, False, False, False, True, False),
    ("var12_r1", 200, 1, 12, 41, True, True, False, False, True, False),
    ("var4_r8", 513, 8, 4, 12, True, False, True, False, True, False),
]
IRF_FIELDS = ("name", "N", "r", "p", "H", "named", "cum", "sd", "unit", "fevd", "misaligned")


def irf_case(row):
    return dict(zip(IRF_FIELDS, row))


def irf_classes(cases=IRF_CASES):
    """The launch classes the table reaches: (SP, series blocks: 1, 2 or 3 = three and more, more than one LDS chunk)."""
    out = set()
    for row in cases:
        c = irf_case(row)
        g = irf_fill(2, c["N"], c["r"], c["H"], c["cum"], not c["misaligned"])
        out.add((g["SP"], min(g["nsblk"], 3), g["nchunk"] > 1))
    return out
