"""CPU proof that the case tables of tests/lane_group_cases.py are good: (a) every lane-group width each launch_* switch can
pick is hit, with a regressor count that fills the width where one exists and with problems for three workgroups; (b) every
regression case is conditioned so well that two CPU formulations of its reference agree far inside the tolerance of the GPU
test; (c) the restatement of the device-drawn Rademacher signs stands on the Random123 known-answer vectors."""
import numpy as np
import pytest

from oracle import boot_oracle as bo
from tests import lane_group_cases as lg
from tests.test_oracle_synth import KAT


# ------------------------------------------------------------------------------------------------ (a) coverage
def _coverage(kernel, widths, full, hits):
    """hits: (R, regressor count, problems) per case.  Returns the widths missing from each class and prints the table."""
    missing = dict(width=[], full=[], three_workgroups=[])
    print(f"\n{kernel}:")
    for R in widths:
        mine = [(n, P) for r, n, P in hits if r == R]
        filled = [n for n, _ in mine if n == full[R]]
        multi = [P for n, P in mine if P > 2 * lg.groups(R) and P % lg.groups(R) != 0]
        print(f"  R = {R:2d} (NG = {lg.groups(R):3d}): counts {sorted({n for n, _ in mine})}, "
              f"fills the width: {'yes' if filled else 'NO'}, three workgroups with a partial last: {'yes' if multi else 'NO'}")
        if not mine:
            missing["width"].append(R)
        if not filled:
            missing["full"].append(R)
        if not multi:
            missing["three_workgroups"].append(R)
    return missing


def _ols_hits(cases):
    return [(lg.ols_width(K), K, lg.three_workgroups(lg.ols_width(K))) for K, _, _ in cases]


def _boot_hits(cases):
    return [(lg.boot_width(ns, p), 1 + ns * p, lg.three_workgroups(lg.boot_width(ns, p))) for ns, p, _, _, _ in cases]


def _chow_hits(ks):
    return [(lg.chow_width(k), k, lg.three_workgroups(lg.chow_width(k))) for k in ks]


def test_every_group_width_is_covered(capsys):
    with capsys.disabled():
        assert not any(_coverage("ols_kernel", lg.OLS_WIDTHS, lg.OLS_FULL, _ols_hits(lg.OLS_CASES)).values())
        assert not any(_coverage("var_boot_kernel", lg.BOOT_WIDTHS, lg.BOOT_FULL, _boot_hits(lg.BOOT_CASES)).values())
        assert not any(_coverage("chow_kernel (count = k, 2 k regressors)", lg.CHOW_WIDTHS, lg.CHOW_FULL,
                                 _chow_hits(lg.CHOW_K)).values())
        # ALS: the batch axis is the run (one workgroup each); the lane groups walk the series and the periods in chunks of NG
        print("\nals_kernel (chunks of NG series / periods per sweep):")
        for R in lg.ALS_WIDTHS:
            mine = [(r, T, N) for r, T, N, *_ in lg.ALS_CASES if lg.als_width(r) == R]
            NG = lg.groups(R)
            print(f"  R = {R:2d} (NG = {NG:3d}): " + ", ".join(
                f"r = {r}: {-(-N // NG)} series and {-(-T // NG)} period chunks" for r, T, N in mine))
            assert any(r == R for r, _, _ in mine), R
            assert any(N > 2 * NG and N % NG for _, _, N in mine), R
        assert {r for r, *_ in lg.ALS_CASES} >= {2, 4, 8, 16, 17, 32}
        assert len(set(lg.ALS_MIXED["r_each"])) > 1 and max(lg.ALS_MIXED["r_each"]) == lg.ALS_MIXED["rmax"]
    # the Chow problems of one call: shuffled series of unequal length, every bandwidth within each four neighbours
    for k in lg.CHOW_K:
        ys, Xs, series, breaks, qs = lg.chow_data(k)
        assert sorted(len(y) for y in ys) == sorted(lg.CHOW_LENGTHS) and 40 <= min(lg.CHOW_LENGTHS) and max(lg.CHOW_LENGTHS) <= 130
        assert (np.diff(series) < 0).any() and set(series) == set(range(5))
        assert all(set(qs[i:i + 4]) == set(lg.CHOW_QS) for i in range(0, len(qs) - 3, 4))
        assert all(len({int(s) for s, qq in zip(series, qs) if qq == q}) >= 3 for q in lg.CHOW_QS)   # each over several lengths
        for s, tb in zip(series, breaks):
            T = len(ys[s])
            assert max(np.floor(lg.CHOW_TRIM * T), 2 * k + 2) <= tb <= T - max(np.floor(lg.CHOW_TRIM * T), 2 * k + 2)


@pytest.mark.parametrize("kernel,drop", [("ols", 2), ("ols", 16), ("ols", 64), ("boot", 16), ("boot", 64), ("chow", 8)])
def test_dropping_a_filling_case_is_noticed(kernel, drop):
    """The coverage check names the width whose only width-filling case leaves the table."""
    if kernel == "ols":
        m = _coverage("ols_kernel without K = %d" % drop, lg.OLS_WIDTHS, lg.OLS_FULL,
                      _ols_hits([c for c in lg.OLS_CASES if c[0] != drop]))
        assert m["full"] == [drop]
    elif kernel == "boot":
        m = _coverage("var_boot_kernel without K = %d" % drop, lg.BOOT_WIDTHS, lg.BOOT_FULL,
                      _boot_hits([c for c in lg.BOOT_CASES if 1 + c[0] * c[1] != drop]))
        assert m["full"] == [drop]
    else:
        m = _coverage("chow_kernel without k = %d" % drop, lg.CHOW_WIDTHS, lg.CHOW_FULL,
                      _chow_hits([k for k in lg.CHOW_K if k != drop]))
        assert m["full"] == [lg.chow_width(drop)]
    assert not m["width"] and not m["three_workgroups"]


def test_dispatch_restatement_matches_the_sources():
    # dfm_ols_batch_dev: pad_r up to 32, one wave above, K > 64 refused
    assert [lg.ols_width(K) for K in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == \
        [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, None]
    assert [lg.als_width(r) for r in (1, 2, 3, 8, 9, 16, 17, 32, 33)] == [2, 2, 4, 8, 16, 16, 32, 32, None]
    # launch_var_boot: the existing shapes (ns, p) = (3,2), (4,4), (2,1), (6,3), (8,4) never reach R = 16
    assert [lg.boot_width(*c) for c in ((3, 2), (4, 4), (2, 1), (6, 3), (8, 4))] == [8, 32, 8, 32, 64]
    assert lg.boot_width(9, 1) is None and lg.boot_width(8, 8) is None and lg.boot_width(7, 9) == 64
    assert [lg.chow_width(k) for k in range(1, 10)] == [2, 4, 8, 8, 16, 16, 16, 16, None]
    assert [lg.three_workgroups(R) for R in (2, 4, 8, 16, 32, 64)] == [259, 131, 67, 35, 19, 11]
    # the largest launch: 259 OLS problems of 40 periods
    assert max(lg.three_workgroups(lg.ols_width(K)) for K, _, _ in lg.OLS_CASES) == 259


def test_no_case_is_refused_and_the_refusals_are():
    for ns, p, T, H, _ in lg.BOOT_CASES:
        assert lg.boot_lds_bytes(ns, p, T) <= lg.LDS_LIMIT, (ns, p, T)
        assert T > p + 1 + ns * p                                   # dfm_var_bootstrap_irf_dev
    for ns, p, T, H in lg.BOOT_SIGN_CASES:
        assert (ns, p, T, H) in [c[:4] for c in lg.BOOT_CASES]
    # R = 8: 32 groups x (T ns + K ns + 16) doubles against 160 KB = 32 x 640 doubles
    assert lg.boot_lds_bytes(*lg.BOOT_REFUSED) == 32 * (222 * 4 + 5 * 4 + 16) * 8 > lg.LDS_LIMIT
    assert lg.boot_lds_bytes(*lg.BOOT_LAST_FIT) == lg.LDS_LIMIT < lg.boot_lds_bytes(*lg.BOOT_FIRST_REFUSED)
    for r, T, N, *_ in lg.ALS_CASES:
        assert lg.als_lds_bytes(r, T, N) <= lg.LDS_LIMIT
    assert lg.als_lds_bytes(4, 5000, 8) > lg.LDS_LIMIT              # the refusal tests/test_gpu_als.py pins
    for B, S in lg.QUANTILE_CASES:
        assert B <= lg.QUANTILE_MAX_B and lg.quantile_lds_bytes(B) <= lg.LDS_LIMIT
    assert {B for B, _ in lg.QUANTILE_CASES} == set(lg.QUANTILE_B) and {S for _, S in lg.QUANTILE_CASES} == set(lg.QUANTILE_S)
    assert lg.quantile_lds_bytes(lg.QUANTILE_MAX_B + 1) > lg.LDS_LIMIT


# ------------------------------------------------------------------------------------------------ (b) conditioning
def _rel(a, b):
    m = ~np.isnan(b)
    assert np.array_equal(np.isnan(a), ~m)
    return float(np.abs(a[m] - b[m]).max() / np.abs(b[m]).max())


def test_ols_cases_are_well_conditioned(capsys):
    worst = 0.0
    runs = [(K, T, sh, 0) for K, T, _ in lg.OLS_CASES for sh in (True, False)] + [lg.OLS_NT_MIN_CASE + (True, lg.OLS_NT_MIN)]
    for K, T, shared, nt_min in runs:
        a, b = lg.ols_reference(K, T, shared, nt_min), lg.ols_reference_other(K, T, shared, nt_min)
        solved = ~np.isnan(a["ssr"])
        assert solved.sum() >= len(solved) - 3 and not solved[lg.OLS_SHORT]      # the NaN problems are the planted ones
        err = max(_rel(b[key], a[key]) for key in ("beta", "resid", "ssr"))
        worst = max(worst, err)
        assert err <= 1e-11, (K, T, shared, err)
    # the nt_min case separates two problems that both have at least K complete rows
    K, T = lg.OLS_NT_MIN_CASE
    n = lg.ols_reference(K, T, True, lg.OLS_NT_MIN)["nobs"]
    assert K <= n[5] < lg.OLS_NT_MIN <= n[6]
    assert np.isnan(lg.ols_reference(K, T, True, lg.OLS_NT_MIN)["ssr"][5]) and not np.isnan(lg.ols_reference(K, T, True)["ssr"][5])
    with capsys.disabled():
        print(f"\nOLS: least squares against normal equations, worst disagreement {worst:.2e} of the largest entry")


def test_bootstrap_cases_are_well_conditioned(capsys):
    worst = 0.0
    for ns, p, T, H, _ in lg.BOOT_CASES:
        # the generator is stationary: companion matrix of the point estimate inside the unit circle
        a, b = lg.boot_reference(ns, p, T, H), lg.boot_reference_other(ns, p, T, H)
        err = max(_rel(b[key], a[key]) for key in ("beta", "irf"))
        worst = max(worst, err)
        assert err <= 1e-11, (ns, p, T, err)
        assert np.isfinite(a["irf"]).all() and np.abs(a["irf"][:, :, -1]).max() < 10 * np.abs(a["irf"][:, :, 0]).max()
    with capsys.disabled():
        print(f"\nbootstrap: least squares against normal equations, worst disagreement {worst:.2e} of the largest entry")


def test_chow_cases_are_well_conditioned(capsys):
    worst = 0.0
    for k in lg.CHOW_K:
        a, b = lg.chow_reference(k), lg.chow_reference_other(k)
        err = float(np.abs(b / a - 1.0).max())
        worst = max(worst, err)
        assert err <= 1e-10, (k, err)
    with capsys.disabled():
        print(f"\nChow: normal equations against least squares in the sandwich, worst relative disagreement {worst:.2e}")


def test_als_cases_are_well_conditioned(capsys):
    """Not a regression with a closed form: the sweeps by normal equations (what the kernel and the GPU test's reference do)
    against the sweeps by LAPACK least squares.  The GPU test allows 1e-10 on the SSR path and 1e-8 on the factors; the two
    CPU routes must agree a hundred times closer, sweep count included."""
    worst_ssr = worst_f = 0.0
    for r, T, N, miss, nt_min, _ in lg.ALS_CASES:
        for a, b in zip(lg.als_reference(r, T, N, miss, nt_min), lg.als_reference(r, T, N, miss, nt_min, solver="qr")):
            assert a["iters"] == b["iters"], (r, T, N)
            e_ssr = float(np.abs(b["ssr_path"] / a["ssr_path"] - 1.0).max())
            e_f = float(np.abs(b["f"] - a["f"]).max() / np.abs(a["f"]).max())
            worst_ssr, worst_f = max(worst_ssr, e_ssr), max(worst_f, e_f)
            assert e_ssr <= 1e-12 and e_f <= 1e-10, (r, T, N, e_ssr, e_f)
            assert np.isnan(a["lam"][N - 1]).all() and not np.isnan(a["lam"][:N - 1]).any()
    with capsys.disabled():
        print(f"\nALS: normal equations against least squares, worst disagreement SSR path {worst_ssr:.2e}, factors {worst_f:.2e}")


def test_quantile_definitions_agree_on_the_finite_columns():
    """The order-statistic definition of the GPU test equals numpy's inverted_cdf on every finite column of every case."""
    for B, S in lg.QUANTILE_CASES:
        x, ref = lg.quantile_data(B, S), lg.quantile_reference(B, S)
        cols = lg.quantile_finite_columns(S)
        np.testing.assert_array_equal(ref[:, cols], np.quantile(x[:, cols], lg.QUANTILE_Q, axis=0, method="inverted_cdf"))
        kinds = {lg.QUANTILE_KINDS[s % 7] for s in range(S)}
        assert S < 7 or kinds == set(lg.QUANTILE_KINDS)
    x = lg.quantile_data(257, 7)
    assert len(np.unique(x[:, 1])) < 20 and np.isinf(x[:, 2]).sum() == 3 and np.isnan(x[:, 3]).sum() == 1 and np.isnan(x[:, 4]).all()


def test_standardize_cases():
    for N in lg.STD_N:
        x = lg.standardize_data(N)
        assert x.shape == (lg.STD_B, lg.STD_T, N) and np.isnan(x[1, :, N // 2]).all()
        if N > 1:
            assert 0.05 < np.isnan(x).mean() < 0.15
            assert (~np.isnan(np.delete(x[1], N // 2, axis=1))).sum(axis=0).min() >= 2


# ------------------------------------------------------------------------------------------------ (c) Rademacher signs
def test_sign_block_is_philox_by_the_known_answers():
    for (c0, c1, c2, c3), (k0, k1), want in KAT:
        got = bo.sign_block(k0 | (k1 << 32), np.uint64(c0 | (c1 << 32)), np.uint64(c2 | (c3 << 32)))
        assert tuple(int(v) for v in got) == want


def test_rademacher_signs_read_word_0_of_the_block():
    seed, T, B = lg.BOOT_SEED, 9, 8
    for first in lg.BOOT_FIRST_DRAWS:
        s = bo.rademacher_signs(seed, first, B, T)
        assert s.shape == (B, T) and set(np.unique(s)) <= {-1.0, 1.0}
        for d in (0, 4, 5, B - 1):                                   # 2^32 - 5 + 5 = 2^32: the draw's high word becomes 1
            for t in (0, 1, T - 1):
                w = bo.sign_block(seed, np.uint64(t), np.uint64(first + d))
                assert s[d, t] == (1.0 if int(w[0]) & 1 else -1.0)
        # shards continue one stream: the draw index is global
        np.testing.assert_array_equal(bo.rademacher_signs(seed, first + 3, B - 3, T), s[3:])
    # a draw index that lost its high bits, or a swapped counter, is a different stream
    hi = bo.rademacher_signs(seed, 2 ** 40, 64, 64)
    assert not np.array_equal(hi, bo.rademacher_signs(seed, 0, 64, 64))
    assert not np.array_equal(bo.rademacher_signs(seed, 2 ** 32, 64, 64), bo.rademacher_signs(seed, 0, 64, 64))
    sq = bo.rademacher_signs(seed, 0, 64, 64)
    assert not np.array_equal(sq, sq.T) and abs(sq.mean()) < 0.1 and not np.array_equal(sq, bo.rademacher_signs(seed + 1, 0, 64, 64))
    # the first known-answer vector through the public function: seed 0, draw 0, period 0, word 0 = 0x6627e8d5 is odd
    assert bo.rademacher_signs(0, 0, 1, 1)[0, 0] == 1.0
