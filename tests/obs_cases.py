"""Case table of tests/test_gpu_obs_geometry.py: the loadings step of the EM with observed factors (csrc/mstep_obs.hip) across its
launch geometry.  Test infrastructure only, no GPU code; tests/test_ar_geometry_cpu.py checks that the table covers every class.

RE = r_o + r_u <= 8 takes mstep_obs_kernel<RE>: an instance per RE in 2..8, one thread per series, 256 series per workgroup.  Wider
models take obs_augment_kernel and obs_moments_kernel<Re> on the moments of z = (g, f) padded to Re = 16 or 32; the padding carries
an identity block, which is absent when RE = Re.

Every reference is computed once per process (functools.lru_cache) and must not be modified by its users."""
import functools

import numpy as np

from oracle import kalman_oracle as ko
from oracle import obs_oracle as oo

KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
B = 2
MAX_ITER = 2
SEED0 = 100                          # replicate b is oo.synth_obs(SEED0 + b, ..)
NARROW_SERIES = 256                  # series per workgroup of mstep_obs_kernel
BLANKED = 5                          # in the cases with missing cells: the series left with r_o + r_u observed cells, one too few
BLANKED_START = 3

# (N, T, r_u, r_o, missing)
CASES = [
    (257, 40, 1, 1, 0.1),            # RE = 2, a second series block of one thread
    (256, 36, 4, 2, 0.0),            # RE = 6, exactly one block, balanced
    (513, 30, 5, 2, 0.1),            # RE = 7, three blocks
    (31, 50, 6, 1, 0.1),             # RE = 7, narrow
    (255, 33, 2, 6, 0.05),           # RE = 8, more observed than latent factors
    (300, 40, 7, 1, 0.1),            # RE = 8, narrow
    (64, 50, 1, 8, 0.1),             # RE = 9, the smallest wide model
    (40, 60, 8, 8, 0.1),             # RE = 16, no padding
    (48, 70, 9, 8, 0.0),             # RE = 17
    (80, 90, 16, 16, 0.1),           # RE = 32
    (60, 45, 2, 1, 0.1),             # RE = 3
    (70, 45, 2, 2, 0.0),             # RE = 4
    (50, 45, 2, 3, 0.1),             # RE = 5
]
CASE_KEYS = ("N", "T", "ru", "ro", "missing")


def case_dict(row):
    return dict(zip(CASE_KEYS, row))


def case_id(row):
    N, T, ru, ro, missing = row
    return f"n{N}_ru{ru}_ro{ro}"


def wide_width(re):
    """mstep_obs_wide_width: the padded width of z = (g, f) on the wide route."""
    return 16 if re <= 16 else 32


def classes(c):
    N, re = c["N"], c["ru"] + c["ro"]
    s = {"balanced" if c["missing"] == 0.0 else "missing"}
    if re <= 8:
        s.add(f"RE={re}")
        blocks = (N + NARROW_SERIES - 1) // NARROW_SERIES
        s.add("narrow:one_partial_block" if N < NARROW_SERIES else "narrow:exactly_one_block" if N == NARROW_SERIES else
              f"narrow:blocks={blocks}")
        if N % NARROW_SERIES == 1 and blocks > 1:
            s.add("narrow:last_block_of_one_thread")
    else:
        Re = wide_width(re)
        s.add(f"Re={Re},{'unpadded' if re == Re else 'padded'}")
        if re == 9:
            s.add("wide:RE=9")
    return s


REQUIRED = ({f"RE={re}" for re in range(2, 9)}
            | {"narrow:one_partial_block", "narrow:exactly_one_block", "narrow:blocks=2", "narrow:blocks=3", "narrow:last_block_of_one_thread"}
            | {"Re=16,padded", "Re=16,unpadded", "Re=32,padded", "Re=32,unpadded", "wide:RE=9", "balanced", "missing"})


def missing_classes(cases=None):
    hit = set()
    for row in (CASES if cases is None else cases):
        hit |= classes(case_dict(row))
    return sorted(REQUIRED - hit)


def replicate(c, b):
    """oo.synth_obs(SEED0 + b, ..).  With missing cells, series BLANKED keeps r_o + r_u observed cells only (a missing cell among
    them becomes 0.25): one fewer than the joint regression needs, so the series keeps its parameters."""
    x, G, p = oo.synth_obs(SEED0 + b, c["N"], c["T"], c["ru"], c["ro"], missing=c["missing"])
    if c["missing"] > 0.0:
        re = c["ru"] + c["ro"]
        keep = np.where(np.isnan(x[BLANKED_START:BLANKED_START + re, BLANKED]), 0.25, x[BLANKED_START:BLANKED_START + re, BLANKED])
        x[:, BLANKED] = np.nan
        x[BLANKED_START:BLANKED_START + re, BLANKED] = keep
    return x, G, p


@functools.lru_cache(maxsize=None)
def expected(row):
    """panel [B, T, N], G [B, T, r_o], start {key: [B, ..]} and, per replicate, oo.em_obs after MAX_ITER iterations: parameters,
    likelihood path, f_smooth and the packed P_smooth."""
    c = case_dict(row)
    reps = [replicate(c, b) for b in range(B)]
    panel = np.stack([x for x, _, _ in reps])
    G = np.stack([g for _, g, _ in reps])
    start = {k: np.stack([p[k] for _, _, p in reps]) for k in KEYS}
    est, path, f, P = [], [], [], []
    for b in range(B):
        p, opath, out = oo.em_obs(panel[b], G[b], {k: start[k][b] for k in KEYS}, max_iter=MAX_ITER, tol=0.0)
        est.append(p); path.append(opath); f.append(out["f_smooth"]); P.append(ko.pack_sym(out["P_smooth"]))
    for a in [panel, G, *start.values(), *path, *f, *P] + [v for p in est for v in p.values()]:
        a.setflags(write=False)
    return dict(panel=panel, G=G, start=start, est=tuple(est), path=tuple(path), f=tuple(f), P=tuple(P))
