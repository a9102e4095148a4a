"""CPU tests of the PCA start's model (tests/pca_expect.py) and of the case table the GPU test runs (tests/pca_cases.py):
  * the model with the present stopping rule equals the oracle (ko.pca_init: the reference's svd-based pca_score + OLS start) on
    every converging case within 1e-9 max|ref| per array (measured worst: 6.5e-11, gen32_full; 1e-9 leaves room for other BLAS builds);
  * the model with the FIRST rule (progress = halving the best residual) misses 1e-8 on every weak-gap row -- why the rule changed;
    this asserts nothing about the library;
  * the table's two conditions (pca_cases.py: gap, iterations);
  * the rho = 0.9999 spectrum panel ends unconverged with rel >= 1e-10 under either rule; the slow one converges inside ITER_CAP."""
import functools

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from tests import pca_cases as pc
from tests import pca_expect as pe


@functools.lru_cache(maxsize=None)
def _run(name, rule):
    """[(worst error vs the oracle, info, relative gap)] over the replicates of a panel case."""
    x, r = pc.panels(name), pc.requested_r(name)
    out = []
    for b in range(pc.B):
        ref, Fo = ko.pca_init(x[b], r)
        p, F, info = pe.pca_start(x[b], r, rule)
        assert np.array_equal(p["mu0"], ref["mu0"])
        out.append((pc.worst_error(p, F, ref, Fo), info, pc.relative_gap(x[b], r)))
    return out


def test_hash_start_is_the_kernels_32_bit_arithmetic():
    """Three entries worked by hand from pca_kernel's first loop (unsigned 32-bit wrap-around), the range and the shape."""
    def one(i, k):
        h = ((i * 73856093) & 0xFFFFFFFF) ^ (((k + 1) * 19349663) & 0xFFFFFFFF)
        h ^= h >> 13
        h = (h * 0x5BD1E995) & 0xFFFFFFFF
        h ^= h >> 15
        return (h & 0xFFFF) / 65536.0 - 0.5
    Y = pe.start(600, 32)
    assert Y.shape == (600, 32) and Y.min() >= -0.5 and Y.max() < 0.5
    for i, k in ((0, 0), (7, 3), (599, 31)):                    # 599 * 73856093 and 32 * 19349663 both wrap
        assert Y[i, k] == one(i, k)
    assert np.linalg.matrix_rank(Y) == 32


def test_spectrum_panel_has_the_prescribed_spectrum():
    lam = pc.spectrum(pc.RHO_SLOW)
    x = pe.spectrum_panel(0, pc.SPEC_T, pc.SPEC_N, lam)
    np.testing.assert_allclose(np.linalg.eigvalsh(x.T @ x)[::-1], lam, rtol=1e-12)
    assert not np.array_equal(x, pe.spectrum_panel(1, pc.SPEC_T, pc.SPEC_N, lam))


@pytest.mark.parametrize("name", list(pc.PANEL_CASES))
def test_model_with_the_present_rule_equals_the_oracle(name):
    for b, (err, info, _) in enumerate(_run(name, "new")):
        assert info["converged"], (name, b, info)
        assert err <= 1e-9, (name, b, err, info)


@pytest.mark.parametrize("name", list(pc.WEAK_GAP))
def test_model_with_the_first_rule_misses_on_the_weak_gap_rows(name):
    old, new = _run(name, "old"), _run(name, "new")
    worst = max(e for e, _, _ in old)
    assert worst > 1e-8, (name, [e for e, _, _ in old])
    b = int(np.argmax([e for e, _, _ in old]))                  # that replicate left early, by the second exit, still improving
    assert old[b][1]["converged"] and old[b][1]["rel"] > pe.REL_EXIT and old[b][1]["iterations"] < new[b][1]["iterations"]


@pytest.mark.parametrize("name", list(pc.ROUTES))
def test_the_rule_leaves_the_strong_gap_rows_alone(name):
    """Where the first rule left by rel <= 1e-14 the present one takes the same steps: same iteration count, same numbers."""
    x, r = pc.panels(name), pc.requested_r(name)
    p_old, F_old, i_old = pe.pca_start(x[0], r, "old")
    p_new, F_new, i_new = pe.pca_start(x[0], r, "new")
    if i_old["rel"] <= pe.REL_EXIT:
        assert i_new == i_old and np.array_equal(F_new, F_old) and all(np.array_equal(p_new[k], p_old[k]) for k in pc.KEYS)
    else:                                                       # (it left by the second exit: the present rule goes on)
        assert i_new["iterations"] > i_old["iterations"] and i_new["rel"] <= pe.REL_EXIT


@pytest.mark.parametrize("name", list(pc.PANEL_CASES))
def test_table_conditions(name):
    for b, (_, info, gap) in enumerate(_run(name, "new")):
        assert gap >= pc.GAP_MIN, (name, b, gap)
        assert info["iterations"] <= pc.ITER_CAP and info["rel"] <= pe.REL_EXIT, (name, b, info)


def test_route_columns_name_known_kernels():
    names = {"gram_xx_dma_kernel", "gram_xx_mfma_kernel", "gram_xx_wide_kernel", "gram_xx_kernel"}
    assert {c[5] for c in pc.PANEL_CASES.values()} == names      # every gram route is in the table


def test_spectrum_cases():
    stuck = pc.spectrum_case(pc.RHO_STUCK)
    for rule in ("old", "new"):
        _, _, info = pe.pca_start(stuck, pc.SPEC_R, rule)
        assert not info["converged"] and info["iterations"] == pe.MAX_ITER and info["rel"] >= 1e-10, info
    for x, lo in [(pc.spectrum_case(pc.RHO_SLOW, seed=s), 500) for s in pc.SLOW_SEEDS] + [(pc.good_small_panel(), 1)]:
        assert pc.relative_gap(x, pc.SPEC_R) >= pc.GAP_MIN
        ref, Fo = ko.pca_init(x, pc.SPEC_R)
        p, F, info = pe.pca_start(x, pc.SPEC_R, "new")
        assert info["converged"] and info["rel"] <= pe.REL_EXIT and lo <= info["iterations"] <= pc.ITER_CAP, info
        assert pc.worst_error(p, F, ref, Fo) <= 1e-9
