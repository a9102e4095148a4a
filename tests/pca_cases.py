"""The case table of tests/test_gpu_pca_routes.py, shared with tests/test_pca_cpu.py (which asserts the table's two conditions from
the model, tests/pca_expect.py).  Every panel case is B replicates ko.synth_replicate(seed + b, N, T, true_r), b < B: distinct
replicates put the batch indexing under test.  The columns `gram` and `route` are what launch_gram_xx / launch_pca (csrc/pca.hip)
give for the shape; they are DATA for the reader and for the one kernel-name assertion of the GPU test, not a copy of the dispatch.

Conditions on the table (asserted by tests/test_pca_cpu.py; if a seed breaks one, change the seed, not the condition):
  gap        every case compared with the oracle has min gap among lambda_1 .. lambda_{r+1} >= GAP_MIN lambda_1: the reference's own
             vectors are then well posed one by one (eps lambda_1 / gap <= 5e-12)
  iterations every case meant to converge takes at most ITER_CAP model iterations under the present stopping rule -- half of
             max_iter, so that a GPU run which differs from the model in the last bits does not sit at the cap"""
import numpy as np

from oracle import kalman_oracle as ko
from tests import pca_expect as pe

B = 3
GAP_MIN = 5e-5
ITER_CAP = pe.MAX_ITER // 2
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")

# name: (N, T, true r, requested r, seed, gram kernel, what the shape reaches)
WEAK_GAP = {          # requested r beyond the strong factors: the cut lies in the noise bulk, lambda_{r+1} / lambda_r = 0.94 .. 0.98
    "weak_lds8": (40, 80, 3, 8, 3, "gram_xx_dma_kernel", "LDS-resident iteration R 8"),
    "weak_lds8_r6": (60, 200, 2, 6, 3, "gram_xx_dma_kernel", "LDS-resident R 8 with r < Rpad"),
    "weak_lds8_odd": (139, 222, 4, 8, 3, "gram_xx_mfma_kernel", "odd N, 8-tile bucket; LDS-resident R 8"),
    "weak_lds4": (50, 400, 1, 4, 3, "gram_xx_dma_kernel", "LDS-resident R 4"),
    "weak_gen16": (64, 50, 4, 12, 3, "gram_xx_dma_kernel", "generic R 16, jacobi_block<16>"),
    "weak_gen32": (300, 60, 5, 20, 0, "gram_xx_wide_kernel", "generic R 32"),
    "weak_gen32_r17": (258, 48, 3, 17, 0, "gram_xx_wide_kernel", "3 stages; smallest r of the 32 bucket"),
}
ROUTES = {            # r at the true count: a strong gap, a few dozen iterations (but for gen4_tiny and gen32_bulk)
    # (requested r beyond the one strong factor, yet no weak-gap row: at N = 12 the rate at the cut is 0.87 .. 0.97 and the first
    # stopping rule's early exit cost 4.3e-9 at the most over seeds 0 .. 39 -- inside 1e-8; replicate 2 of this seed is that panel)
    "gen4_tiny": (12, 40, 1, 3, 35, "gram_xx_dma_kernel", "generic R 4 (N 4 < 64)"),
    "gen8_partial_tile": (7, 30, 5, 5, 3, "gram_xx_mfma_kernel", "generic R 8 with N < 16: one partial tile, clamped rows in tall_gram_mfma / apply_S"),
    "gen2": (17, 30, 2, 2, 3, "gram_xx_mfma_kernel", "generic R 2"),
    "gen32_n_near_r": (40, 45, 20, 20, 3, "gram_xx_dma_kernel", "R 32 with N barely above r, 4-tile bucket, T between one and two 32-period blocks"),
    "gen32_full": (64, 40, 32, 32, 3, "gram_xx_dma_kernel", "the full 32-wide state (r = 32 <= T - 1)"),
    "gen32_bulk": (64, 40, 4, 32, 3, "gram_xx_dma_kernel", "R 32, most Ritz values in the bulk"),
    "wide_exact_gen16": (384, 48, 9, 9, 3, "gram_xx_wide_kernel", "N = 3 x 128, T = 3 x 16 exactly; R 16 at N > 256 with r = 9"),
    "wide_one_stage_gen4": (260, 12, 3, 3, 3, "gram_xx_wide_kernel", "ONE stage; generic R 4 through N > 256"),
    "wide_two_stages_gen2": (258, 20, 2, 2, 3, "gram_xx_wide_kernel", "TWO stages; generic R 2 through N > 256"),
    "valu_gen32": (257, 40, 20, 20, 3, "gram_xx_kernel", "the VALU kernel (odd N > 256) feeding R 32"),
    "valu_ragged_tile": (513, 24, 4, 4, 3, "gram_xx_kernel", "VALU gram, N not a multiple of 4 in the last tile"),
    "mfma_12_tiles": (199, 33, 6, 6, 3, "gram_xx_mfma_kernel", "12-tile bucket, T = 32 + 1"),
    "dma_8_tiles": (140, 32, 5, 5, 3, "gram_xx_dma_kernel", "8-tile bucket, T = exactly one block"),
    "gen16_full": (48, 70, 16, 16, 3, "gram_xx_dma_kernel", "Rpad 16 full"),
}
PANEL_CASES = {**WEAK_GAP, **ROUTES}

# spectrum-panel cases (pe.spectrum_panel): N 24, T 40, r 3, lambda proportional to (9, 6, 4, 4 rho, 2 .. 0.5); the rate at the cut is rho
SPEC_N, SPEC_T, SPEC_R = 24, 40, 3
RHO_STUCK = 0.9999        # the model does not converge: rel 5.7e-6 after max_iter steps under either rule
RHO_SLOW = 0.975          # converges under the present rule inside ITER_CAP (chosen on the CPU: tests/test_pca_cpu.py holds it to that)
SLOW_SEEDS = (0, 1)       # spectrum_case seeds of the slow case: two replicates


def good_small_panel():
    """[T, N]: an ordinary panel of the spectrum cases' shape, the well-behaved neighbour of the stuck one in a batch."""
    return ko.synth_replicate(11, SPEC_N, SPEC_T, SPEC_R)[0]


def panels(name):
    """[B, T, N] of a panel case."""
    N, T, true_r, _, seed = PANEL_CASES[name][:5]
    return np.stack([ko.synth_replicate(seed + b, N, T, true_r)[0] for b in range(B)])


def requested_r(name):
    return PANEL_CASES[name][3]


def spectrum(rho):
    lam = np.concatenate([[9.0, 6.0, 4.0, 4.0 * rho], np.linspace(2.0, 0.5, SPEC_N - 4)])
    return lam * (SPEC_T * SPEC_N / lam.sum())                 # trace of X'X as a standardised panel's


def spectrum_case(rho, seed=0):
    """[T, N] panel whose X'X has the eigenvalues spectrum(rho)."""
    return pe.spectrum_panel(seed, SPEC_T, SPEC_N, spectrum(rho))


def relative_gap(x, r):
    """min gap among lambda_1 .. lambda_{r+1} of x'x, relative to lambda_1 (lambda_{r+1} = 0 where r = min(T, N))."""
    sv = np.linalg.svd(x, compute_uv=False) ** 2
    lam = np.concatenate([sv, [0.0]])[:r + 1]
    return float(np.min(lam[:-1] - lam[1:]) / lam[0])


def worst_error(got, F, ref, Fo):
    """max over Lam, R, A, Q, P0, F of max|got - ref| / max|ref| (mu0 is zero on both sides: compared exactly by the callers)."""
    e = [np.abs(np.asarray(got[k]) - ref[k]).max() / np.abs(ref[k]).max() for k in KEYS if k != "mu0"]
    e.append(np.abs(np.asarray(F) - Fo).max() / np.abs(Fo).max())
    return float(max(e))
