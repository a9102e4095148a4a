"""CPU checks of tests/ar_geometry.py and tests/obs_cases.py: the plain-Python restatement of the AR series step's launch geometry
against csrc/dfm_argeom.h itself, compiled for the host (tests/host/argeom_host.cpp); the GPU case tables
(tests/test_gpu_ar_geometry.py, tests/test_gpu_obs_geometry.py) against the coverage classes they must hit; and the preconditions the
GPU tests lean on, checked on the oracle alone: every expectation finite, the edge series behaving as the table says, and every
watched series moving by far more than the GPU tolerance, so that an un-updated or mis-addressed series cannot pass."""
import itertools

import numpy as np
import pytest

from tests import ar_geometry as ag
from tests import obs_cases as oc

AR_IDS = [ag.case_id(row) for row in ag.CASES]
PARAM_TOL = 1e-7                     # tests/test_gpu_ar_geometry.py: parameters at 1e-7 max(1, |ref|)
MARGIN = 1000.0                      # a watched series moves by more than MARGIN x that tolerance


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return ag.build_argeom_host(tmp_path_factory.mktemp("argeom"))


def _check(host_exe, requests):
    """(r, q, p, N, T) requests: `launch` against the host program, field for field.  Returns the launches."""
    geos = [ag.launch(*req) for req in requests]
    host = ag.ask_argeom_host(host_exe, [(r, q, N, T, g["Rk"]) for (r, q, p, N, T), g in zip(requests, geos)])
    bad = [(req, h) for req, g, h in zip(requests, geos, host) if ag.host_tuple(g) != h]
    assert not bad, bad[:5]
    return geos


def test_instances_are_the_supported_ones():
    assert len(ag.INSTANCES) == 38 and len(set(ag.INSTANCES)) == 38
    assert all(1 <= r <= 8 and 0 <= q <= 4 and r * (q + 1) <= 32 for r, q in ag.INSTANCES)
    assert (7, 4) not in ag.INSTANCES and (8, 4) not in ag.INSTANCES and (6, 4) in ag.INSTANCES and (8, 3) in ag.INSTANCES


def test_every_instance_matches_the_header(host_exe):
    """Each (r, q) at p below, at and above q + 1 (Rk padded and not), and the case table itself."""
    reqs = [(r, q, p, N, T) for r, q in ag.INSTANCES for p in (1, q + 1, q + 2, 8) if r * max(p, q + 1) <= 32
            for N, T in ((1, q + 2), (49, 140))]
    reqs += [row[:5] for row in ag.CASES]
    assert len(_check(host_exe, reqs)) > 4 * 38


@pytest.mark.parametrize("r,q", ag.SWEEP_INSTANCES)
def test_geometry_sweep_matches_the_header(host_exe, r, q):
    """N = 1..300 x T - q = 2..400 at one instance per series-group width."""
    geos = _check(host_exe, [(r, q, 1, N, Tq + q) for N, Tq in itertools.product(ag.SWEEP_N, ag.SWEEP_TQ)])
    assert len(geos) == 300 * 399
    assert {1, 2, 3, 4} <= {g["chunks"] for g in geos} and {1, 32} <= {g["last_steps"] for g in geos}
    assert {1, 2, 5} <= {g["solve_blocks"] for g in geos} and {1, 2, 3} <= {g["moment_blocks"] for g in geos}


def test_series_group_widths_of_the_sweep():
    assert [ag.geo(r, q)["SGW"] for r, q in ag.SWEEP_INSTANCES] == [3, 2, 1]


def test_geometry_matches_the_sources():
    """The numbers mstep_ar.hip and DESIGN state about the instances."""
    g = ag.geo(4, 4)                                              # the Stock-Watson shape: 210 packed moments, 20 states
    assert (g["K1"], g["NTM"], g["NZF"], g["TT"], g["TPW"], g["SGW"], g["NT"]) == (20, 14, 2, 24, 6, 3, (6, 6, 6, 6))
    g = ag.geo(8, 3)                                              # K1 = 32: 528 = 33 x 16 packed moments, no padding column
    assert (g["K1"], g["NTM"], g["TT"], g["TPW"], g["SGW"], g["NT"]) == (32, 33, 41, 11, 1, (11, 11, 11, 8))
    g = ag.geo(6, 4)
    assert (g["TT"], g["TPW"], g["SGW"], g["NT"]) == (40, 10, 1, (10, 10, 10, 10))
    assert ag.geo(1, 0)["NT"] == (1, 1, 0, 0) and ag.geo(8, 0)["NT"] == (1, 1, 1, 1) and ag.geo(4, 2)["NT"] == (2, 2, 2, 2)
    straddle2 = {rq for rq in ag.INSTANCES if ag.geo(*rq)["straddle"] and ag.geo(*rq)["NZF"] == 2}
    assert {(5, 4), (6, 2), (6, 3), (7, 2), (7, 3)} <= straddle2
    L = ag.launch(4, 4, 4, 50, 150)                               # tests/test_gpu_ar_em.py: two series blocks, chunks of 128 + 18 periods
    assert (L["moment_blocks"], L["chunks"], L["last_steps"], L["Rk"], L["k"], L["VW"]) == (2, 2, 5, 32, 20, 256)
    L = ag.launch(2, 0, 3, 65, 129)                               # a second chunk of one period: fewer steps than the prefetch depth
    assert (L["Tq"], L["chunks"], L["last_steps"]) == (129, 2, 1) and L["last_steps"] < ag.AR_PF
    assert (L["k"], L["Rk"], L["solve_blocks"]) == (6, 8, 2)


def test_case_table_covers_every_class():
    assert {(row[0], row[1]) for row in ag.CASES} == set(ag.INSTANCES)
    assert ag.missing_classes() == [], f"coverage classes no case hits: {ag.missing_classes()}"


def test_case_table_respects_the_dimension_limits():
    for row in ag.CASES:
        c = ag.case_dict(row)
        L = ag.launch(c["r"], c["q"], c["p"], c["N"], c["T"])
        assert L["k"] <= 32 and c["N"] <= ag.collapse_max_n(L["Rk"]) and L["Tq"] >= 2, row
        assert c["N"] <= 256 and c["N"] * c["T"] <= 256 * 40 + 145 * 135, row        # one tiny batch per test id


@pytest.mark.parametrize("drop,lost", [("r6_q4_p1_n16_t66", "SGW=1:N%SW==0"), ("r6_q4_p5_n9_t134_bal", "SGW=1:N<SW"),
                                       ("r5_q4_p2_n20_t137_edge", "SGW=2:N<SW"), ("r6_q3_p4_n64_t133_edge", "SGW=2:N%SW==0")])
def test_dropping_a_case_is_noticed(drop, lost):
    """The coverage check fails, naming the class, when the only case of a class leaves the table."""
    assert drop in AR_IDS
    rest = [row for row in ag.CASES if ag.case_id(row) != drop]
    assert len(rest) == len(ag.CASES) - 1 and lost in ag.missing_classes(rest), drop


@pytest.mark.parametrize("row", ag.CASES, ids=AR_IDS)
def test_oracle_preconditions(row):
    c = ag.case_dict(row)
    r, q, N = c["r"], c["q"], c["N"]
    e = ag.expected(row)
    for b in range(ag.B):
        ps, em, st = e["passes"][b], e["ems"][b], {k: e["start"][k][b] for k in ag.KEYS}
        assert np.isfinite(ps["loglik"]) and np.isfinite(ps["f"]).all() and np.isfinite(ps["P"]).all()
        assert len(em["path"]) == ag.MAX_ITER and np.isfinite(em["path"]).all() and np.isfinite(em["f"]).all()
        assert all(np.isfinite(em["est"][k]).all() for k in ag.KEYS)
        assert em["est"]["sig2"].min() > 0.0
        n = ag.usable_rows(e["panel"][b], q)
        if c["edge"]:
            assert (n[ag.EDGE_ENOUGH], n[ag.EDGE_SHORT], n[ag.EDGE_EMPTY]) == (r + q + 1, r + q, 0)
            if c["T"] - q > ag.EDGE_MASKED_CHUNK_TQ:
                assert np.isnan(e["panel"][b][:ag.AR_TC + q, N - 1]).all() and n[N - 1] >= r + q + 1
            for i in (ag.EDGE_SHORT, ag.EDGE_EMPTY):
                assert all(np.array_equal(em["est"][k][i], st[k][i]) for k in ("Lam", "sig2", "rho")), i
            assert not np.array_equal(em["est"]["Lam"][ag.EDGE_ENOUGH], st["Lam"][ag.EDGE_ENOUGH])
            assert em["est"]["sig2"][ag.EDGE_ENOUGH] != st["sig2"][ag.EDGE_ENOUGH]
        # discrimination: the watched series move by more than MARGIN x the GPU tolerance of the quantity
        for k in ("Lam", "sig2", "rho"):
            if em["est"][k].size == 0:
                continue
            need = MARGIN * PARAM_TOL * max(1.0, np.abs(em["est"][k]).max())
            for i in ag.watched_series(c):
                moved = np.abs(em["est"][k][i] - st[k][i]).max()
                assert moved > need, (k, b, i, moved, need)


@pytest.mark.parametrize("row", ag.CASES, ids=AR_IDS)
def test_oracle_is_insensitive_to_its_start(row):
    """The reference's own error: Q and P0 of the start are well conditioned (cond <= 1e3), and 1e-13 of relative noise on every
    start parameter moves no quantity the GPU test compares by more than a thousandth of that quantity's bound."""
    from oracle import ar_oracle as ao
    c = ag.case_dict(row)
    e = ag.expected(row)
    rng = np.random.default_rng([c["r"], c["q"], c["p"], c["N"], c["T"]])
    for b in range(ag.B):
        st = {k: e["start"][k][b] for k in ag.KEYS}
        for k in ("Q", "P0"):
            ev = np.linalg.eigvalsh(st[k])
            assert ev[0] > 0.0 and ev[-1] <= 1e3 * ev[0], (k, b, ev[0], ev[-1])
    b = 0
    st = {k: e["start"][k][b] for k in ag.KEYS}
    st2 = {k: v * (1.0 + 1e-13 * rng.standard_normal(v.shape)) for k, v in st.items()}
    st2["Q"], st2["P0"] = 0.5 * (st2["Q"] + st2["Q"].T), 0.5 * (st2["P0"] + st2["P0"].T)
    est, path, out = ao.em_ar(e["panel"][b], st2, max_iter=ag.MAX_ITER)
    ref = e["ems"][b]
    rel = lambda got, want: np.abs(got - want).max() / max(1.0, np.abs(want).max())
    assert np.abs(path / ref["path"] - 1.0).max() <= 1e-8 / MARGIN
    assert rel(out["f_smooth"][:, :c["r"]], ref["f"]) <= 1e-8 / MARGIN
    for k in ag.KEYS:
        if ref["est"][k].size:
            assert rel(est[k], ref["est"][k]) <= PARAM_TOL / MARGIN, (k, rel(est[k], ref["est"][k]))


# ---- observed factors ---------------------------------------------------------------------------------------------------------
def test_obs_case_table_covers_every_class():
    assert oc.missing_classes() == [], f"coverage classes no case hits: {oc.missing_classes()}"
    assert [oc.wide_width(re) for re in (9, 16, 17, 32)] == [16, 16, 32, 32]


@pytest.mark.parametrize("drop", ["n257_ru1_ro1", "n256_ru4_ro2", "n40_ru8_ro8", "n80_ru16_ro16"])
def test_dropping_an_obs_case_is_noticed(drop):
    assert drop in [oc.case_id(row) for row in oc.CASES]
    assert oc.missing_classes([row for row in oc.CASES if oc.case_id(row) != drop]), drop


@pytest.mark.parametrize("row", oc.CASES, ids=[oc.case_id(row) for row in oc.CASES])
def test_obs_oracle_preconditions(row):
    c = oc.case_dict(row)
    e = oc.expected(row)
    re = c["ru"] + c["ro"]
    for b in range(oc.B):
        p, st = e["est"][b], {k: e["start"][k][b] for k in oc.KEYS}
        assert len(e["path"][b]) == oc.MAX_ITER and np.isfinite(e["path"][b]).all()
        assert all(np.isfinite(p[k]).all() for k in oc.KEYS) and np.isfinite(e["f"][b]).all() and np.isfinite(e["P"][b]).all()
        if c["missing"] > 0.0:
            assert (~np.isnan(e["panel"][b][:, oc.BLANKED])).sum() == re
            assert np.array_equal(p["Lam"][oc.BLANKED], st["Lam"][oc.BLANKED]) and p["R"][oc.BLANKED] == st["R"][oc.BLANKED]
        # the first and last series of every block of 256 move by far more than the 1e-8 of the GPU test
        for i in sorted({0, c["N"] - 1} | set(range(256, c["N"], 256)) | set(range(255, c["N"], 256))):
            assert np.abs(p["Lam"][i] - st["Lam"][i]).max() > MARGIN * 1e-8 * max(1.0, np.abs(p["Lam"]).max()), (b, i)
            assert abs(p["R"][i] - st["R"][i]) > MARGIN * 1e-8 * max(1.0, np.abs(p["R"]).max()), (b, i)
