"""CPU checks of tests/mstep_geometry.py: the plain-Python restatement of the balanced loadings step's launch geometry against
csrc/dfm_msgeom.h itself, compiled for the host (tests/host/msgeom_host.cpp); the GPU case tables (tests/test_gpu_mstep_geometry.py)
against the coverage classes they must hit and the route they claim; and the preconditions the GPU tests lean on, checked on the
oracle alone: every case insensitive to its start, every watched series moving by far more than the GPU bound, and the stop cases
stopping at different iterations with room around the stop rule's threshold."""
import numpy as np
import pytest

from oracle import kalman_oracle as ko
from tests import mstep_geometry as mg

GPU_TOL = 1e-8                       # tests/test_gpu_mstep_geometry.py (tests/test_gpu_em.py RTOL)
MARGIN = 1000.0                      # a watched series moves by more than MARGIN x that bound
NOISE = 1e-13                        # relative noise on the start; what it moves stays below GPU_TOL / 100
TWO_ITER = mg.MFMA_CASES + mg.MFMA_EXTRA + mg.WIDE_CASES
IDS = [mg.case_id(row) for row in TWO_ITER]
STOP_IDS = [mg.case_id(row) for row in mg.STOP_CASES]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return mg.build_msgeom_host(tmp_path_factory.mktemp("msgeom"))


# ---- the restatement against the header ---------------------------------------------------------------------------------------
def test_the_64_instances():
    inst = mg.ms_instances()
    assert len(inst) == 64 and len({(Rp, s) for Rp, s, _ in inst}) == 64
    assert {(Rp, s) for Rp, s, _ in inst} == {(Rp, s) for Rp in (4, 8) for s in range(1, 33)}
    assert all(ndr == (s + 7) // 8 for Rp, s, ndr in inst if Rp == 4) and all(ndr == (s + 15) // 16 for Rp, s, ndr in inst if Rp == 8)
    assert (mg.ms_cs(4), mg.ms_cs(8)) == (16, 8)
    assert mg.ms_range(4, 1) == (4, 16) and mg.ms_range(8, 1) == (4, 8) and mg.ms_range(4, 32) == (498, 512) and mg.ms_range(8, 32) == (250, 256)


@pytest.mark.parametrize("Rp", [4, 8])
def test_mfma_sweep_matches_the_header(host_exe, Rp):
    """N = 2..1100 x T = 3..140 x B: every instance, every refusal, every wpr and segment length."""
    reqs = [(B, N, T) for N in mg.SWEEP_N for T in mg.SWEEP_T for B in mg.SWEEP_B]
    host = mg.ask_msgeom_host(host_exe, "".join(f"M {B} {N} {T} {Rp}\n" for B, N, T in reqs), len(reqs))
    seen, wprs, bad = set(), set(), []
    r = Rp                                                       # (pad_r(r) = Rp)
    for (B, N, T), h in zip(reqs, host):
        if not mg.mfma_supported(Rp, N):
            want = (0,)
        else:
            g = mg.mfma(B, N, T, r)
            want = mg.mfma_host_tuple(g)
            seen.add((g["Rp"], g["STEPS"], g["NDR"]))
            wprs.add(g["wpr"])
            assert sum(g["nrows"]) == T
        if want != h:
            bad.append(((B, N, T), want, h))
    assert not bad, bad[:5]
    assert seen == {i for i in mg.ms_instances() if i[0] == Rp} and wprs == set(range(1, 9))


@pytest.mark.parametrize("Rp", [2, 4, 8, 16, 32])
def test_wide_sweep_matches_the_header(host_exe, Rp):
    """The same sweep for mstep_wide at every padded width, r walking the width's range (Rp = 32: NX = 1 .. 4)."""
    rs = {2: (1, 2), 4: (3, 4), 8: (5, 6, 7, 8), 16: (9, 12, 16), 32: tuple(range(17, 33))}[Rp]
    reqs = [(B, N, T, rs[(N + T) % len(rs)]) for N in mg.SWEEP_N for T in mg.SWEEP_T for B in mg.SWEEP_B]
    host = mg.ask_msgeom_host(host_exe, "".join(f"W {B} {N} {T} {r} {Rp} {mg.NUM_CU}\n" for B, N, T, r in reqs), len(reqs))
    seen, bad = set(), []
    for (B, N, T, r), h in zip(reqs, host):
        if not mg.wide_supported(Rp, N):
            want = (0,)
        else:
            g = mg.wide(B, N, T, r)
            want = mg.wide_host_tuple(g)
            seen.add((g["R"], g["NX"], g["rd"]))
        if want != h:
            bad.append(((B, N, T, r), want, h))
    assert not bad, bad[:5]
    assert seen == {i for i in mg.wide_instances() if i[2] == Rp}


def test_wide_grid_follows_the_device(host_exe):
    """num_cu = 0 (unknown), 4, 100 and 304: the grid is a multiple of 8, at least 8, and never more than the items of an unmapped batch."""
    reqs = [(B, N, 40, 20, ncu) for B in (1, 2, 15, 16, 17) for N in (64, 130, 1000) for ncu in (0, 4, 100, 256, 304)]
    host = mg.ask_msgeom_host(host_exe, "".join(f"W {B} {N} {T} {r} 32 {ncu}\n" for B, N, T, r, ncu in reqs), len(reqs))
    for (B, N, T, r, ncu), h in zip(reqs, host):
        assert mg.wide_host_tuple(mg.wide(B, N, T, r, num_cu=ncu)) == h, (B, N, ncu)


def test_geometry_matches_the_sources():
    """The numbers the sources and DESIGN state about the two steps."""
    g = mg.mfma(4, 200, 500, 8)                                   # BASELINE config 2
    assert (g["CS"], g["STEPS"], g["NDR"], g["wpr"], g["tq"], g["nrows"][-1], g["slot"]) == (8, 25, 2, 8, 64, 52, 1600)
    g = mg.mfma(8192, 200, 500, 8)                                # ... its shard: one wave per replicate
    assert (g["wpr"], g["nrows"], g["nfront"]) == (1, (500,), 2048)
    g = mg.mfma(2, 66, 65, 3)                                     # rows of 528 bytes: segments of 16 periods, 16 16 16 16 1 0 0 0
    assert (g["m"], g["wpr"], g["tq"], g["nrows"]) == (8, 8, 16, (16, 16, 16, 16, 1, 0, 0, 0))
    w = mg.wide(2, 1000, 2000, 20)                                # BASELINE config 4
    assert (w["R"], w["NX"], w["nsb"], w["last_series"], w["stages"], w["last_rows"], w["grid"]) == (32, 1, 8, 104, 63, 16, 16)
    assert [mg.wide(2, 64, 40, r)["NX"] for r in (17, 20, 21, 24, 25, 28, 29, 32)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert mg.route(200, 8) == "mstep_mfma" and mg.route(40, 3) == "mstep_mfma" and mg.route(30, 2) == "mstep_lam"
    assert mg.route(31, 5) == "mstep_lam" and mg.route(600, 4) == "mstep_wide" and mg.route(64, 12) == "mstep_wide"
    assert mg.route(200, 8, may_have_missing=True) == "mstep_lam" and mg.route(2, 4) == "mstep_lam" and mg.route(514, 1) == "mstep_wide"


# ---- the tables ---------------------------------------------------------------------------------------------------------------
def test_mfma_table_covers_every_class():
    assert len(mg.MFMA_CASES) == 64
    assert [mg.ms_instance(mg.pad_r(r), N) for _, N, _, r in mg.MFMA_CASES] == mg.ms_instances()
    assert all(B == 2 and N % 2 == 0 and 9 <= T <= 80 for B, N, T, _ in mg.MFMA_CASES)
    assert [r for _, _, _, r in mg.MFMA_CASES] == [3, 4] * 16 + [5, 6, 7, 8] * 8
    assert sorted(B for B, _, _, _ in mg.MFMA_EXTRA if B != 2) == [1, 5, 9] and sorted(T for B, _, T, _ in mg.MFMA_EXTRA if B == 2) == [3, 8]
    missing = mg.missing_classes(mg.MFMA_REQUIRED, mg.mfma_classes, mg.MFMA_CASES + mg.MFMA_EXTRA)
    assert missing == [], f"coverage classes no case hits: {missing}"
    # the table alone walks the instances, wpr, the rounding factors and the segments' rows; the extra cases add B and T only
    alone = mg.missing_classes(mg.MFMA_REQUIRED, mg.mfma_classes, mg.MFMA_CASES)
    assert set(alone) <= {"front:clamped_wave_past_a_full_group", "T<8", "T==8"}, alone


def test_wide_table_covers_every_class():
    missing = mg.missing_classes(mg.WIDE_REQUIRED, mg.wide_classes, mg.WIDE_CASES)
    assert missing == [], f"coverage classes no case hits: {missing}"
    assert {mg.wide(*row)["rd"] if mg.wide(*row)["R"] == 16 else 32 for row in mg.WIDE_CASES} == {2, 4, 8, 16, 32}   # the finish kernel's instances
    assert all(B * T * N <= 2 * 80 * 1024 or B == 17 for B, N, T, _ in mg.WIDE_CASES)


@pytest.mark.parametrize("drop,lost", [((2, 144, 96, 25), "T=96"), ((2, 1024, 5, 2), "T=5"), ((2, 514, 33, 1), "r=1"),
                                       ((2, 600, 20, 3), "instance=16,0,4")])
def test_dropping_a_wide_case_is_noticed(drop, lost):
    assert drop in mg.WIDE_CASES
    rest = [row for row in mg.WIDE_CASES if row != drop]
    assert lost in mg.missing_classes(mg.WIDE_REQUIRED, mg.wide_classes, rest)


def test_every_case_takes_the_route_its_table_claims():
    for row in mg.MFMA_CASES + mg.MFMA_EXTRA:
        assert mg.route(row[1], row[3]) == "mstep_mfma", row
    for row in mg.WIDE_CASES:
        assert mg.route(row[1], row[3]) == "mstep_wide", row
    for row in mg.STOP_CASES:
        assert mg.route(row[1], row[3]) == row[6], row
    assert [mg.pad_r(row[3]) for row in mg.STOP_CASES] == [4, 8, 16, 32] and all(row[0] == 4 for row in mg.STOP_CASES)
    assert all(row[4] > 0.0 and row[5] <= 40 for row in mg.STOP_CASES)
    assert all(N <= 1024 for _, N, _, _ in TWO_ITER)                                     # check_em_n


# ---- the oracle alone ---------------------------------------------------------------------------------------------------------
def _rel(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _perturbed(st, rng):
    st2 = {k: v * (1.0 + NOISE * rng.standard_normal(v.shape)) for k, v in st.items()}
    st2["Q"], st2["P0"] = 0.5 * (st2["Q"] + st2["Q"].T), 0.5 * (st2["P0"] + st2["P0"].T)
    return st2


@pytest.mark.parametrize("row", TWO_ITER, ids=IDS)
def test_oracle_is_insensitive_to_its_start_and_moves_the_watched_series(row):
    """The reference's own error: 1e-13 of relative noise on every start parameter moves no quantity the GPU test compares by more
    than a hundredth of that quantity's bound; and two iterations move the loadings of every watched series by more than 1000
    times the bound, so that a series the kernel skipped or addressed wrongly cannot pass."""
    B, N, T, r = row
    e = mg.expected(row)
    rng = np.random.default_rng([B, N, T, r])
    for b in range(B if B <= 2 else 1):
        st = {k: e["start"][k][b] for k in mg.KEYS}
        ref = e["ems"][b]
        assert len(ref["path"]) == mg.MAX_ITER and np.isfinite(ref["path"]).all() and ref["est"]["R"].min() > 0.0
        p, path, out = ko.em(e["panel"][b], _perturbed(st, rng), max_iter=mg.MAX_ITER)
        assert np.abs(path / ref["path"] - 1.0).max() <= GPU_TOL / 100
        for k in mg.KEYS:
            assert _rel(p[k], ref["est"][k]) <= GPU_TOL / 100, (k, _rel(p[k], ref["est"][k]))
        assert _rel(out["f_smooth"], ref["f"]) <= GPU_TOL / 100
        assert float(np.abs(ko.pack_sym(out["P_smooth"]) - ref["P"]).max()) <= GPU_TOL / 100 * max(1.0, ref["Pscale"])
    for b in range(B):
        lam, lam0 = e["ems"][b]["est"]["Lam"], e["start"]["Lam"][b]
        need = MARGIN * GPU_TOL * max(1.0, float(np.abs(lam).max()))
        for i in mg.watched_series(row):
            assert np.abs(lam[i] - lam0[i]).max() > need, (b, i, np.abs(lam[i] - lam0[i]).max(), need)


@pytest.mark.parametrize("row", mg.STOP_CASES, ids=STOP_IDS)
def test_stop_cases_stop_at_different_iterations(row):
    """From the oracle alone: the replicates' iteration counts differ, are at least 2 and stay below max_iter; every decision of
    the stop rule along the way has 1e-6 of room around tol (fifty times what a path held to 1e-8 can move the criterion); and two
    iterations from the start are insensitive to it, as above."""
    B, N, T, r, tol, max_iter, _ = row
    e = mg.expected_stop(row)
    its = [len(em["path"]) for em in e["ems"]]
    assert min(its) >= 2 and max(its) < max_iter and min(its) != max(its), its
    assert min(its[:2]) < max(its[2:]), its                       # the replicates that start further away take longer
    for em in e["ems"]:
        path = em["path"]
        crit = np.diff(path) / (0.5 * (np.abs(path[1:]) + np.abs(path[:-1])))
        assert np.abs(crit - tol).min() >= 1e-6 and (crit[:-1] >= tol).all() and crit[-1] < tol
    rng = np.random.default_rng([B, N, T, r])
    for b in (0, B - 1):
        st = {k: e["start"][k][b] for k in mg.KEYS}
        p0, path0, _ = ko.em(e["panel"][b], st, max_iter=2)
        p1, path1, _ = ko.em(e["panel"][b], _perturbed(st, rng), max_iter=2)
        assert np.abs(path1 / path0 - 1.0).max() <= GPU_TOL / 100
        assert all(_rel(p1[k], p0[k]) <= GPU_TOL / 100 for k in mg.KEYS)
