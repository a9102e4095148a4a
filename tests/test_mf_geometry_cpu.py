"""CPU checks of tests/mf_geometry.py: the plain-Python restatement of the mixed-frequency series step's launch geometry and tile
dealing against csrc/dfm_mfgeom.h itself, compiled for the host (tests/host/mfgeom_host.cpp); the GPU case table
(tests/test_gpu_mf_geometry.py) against the coverage classes it must hit; and the preconditions the GPU tests lean on, checked on
the NumPy model alone: every watched series moving by far more than the GPU bound, three wrong kernels told from the right one,
the model's own noise a hundredth of every bound, and the stop cases stopping at different iterations."""
import numpy as np
import pytest

from tests import mf_expect as me
from tests import mf_geometry as mg

PATH_RTOL, PARAM_TOL, F_TOL, P_RTOL = 1e-8, 1e-7, 1e-8, 1e-8      # tests/test_gpu_mf_geometry.py (tests/test_gpu_mf.py)
MARGIN = 1000.0                      # a watched series, and a wrong kernel, move by more than MARGIN x the bound
IDS = [c["name"] for c in mg.CASES]
STOP_IDS = [row[0]["name"] for row in mg.STOP_CASES]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return mg.build_mfgeom_host(tmp_path_factory.mktemp("mfgeom"))


# ---- the restatement against the header ---------------------------------------------------------------------------------------
def _labels(rng, N, C, order):
    """A class of 0 .. C - 1 for every series (every class used where N allows): in runs, shuffled, or dealt round-robin."""
    lab = np.concatenate([np.arange(min(C, N)), rng.integers(0, C, max(0, N - C))])
    if order == 0:
        return np.sort(lab)
    if order == 1:
        return rng.permutation(lab)
    return np.arange(N) % C


def test_sweep_matches_the_header(host_exe):
    """N = 1 .. 300, C = 1 .. 8 in class-sorted, shuffled and round-robin orders, r = 1 .. 8, L = 1 .. 5, T = 1 .. 70: the widths, the
    column map, the grids, the classes in the order of their first series and every entry of the tile lists."""
    rng = np.random.default_rng(11)
    reqs = []
    for N in range(1, 301):
        for k in range(6):
            C, L, r = 1 + (N + k) % 8, 1 + (N + 2 * k) % 5, 1 + (N + 3 * k) % 8
            T, B = 1 + (11 * N + 17 * k) % 70, (1, 3, 5, 64)[(N + k) % 4]
            rows = np.unique(rng.integers(-2, 3, (64, L)), axis=0).astype(float)     # distinct rows, small integers (L = 1: five)
            rows = rows[rng.permutation(len(rows))][:C]
            lab = _labels(rng, N, len(rows), k % 3)
            reqs.append((N, L, r, T, B, mg.pad_r(r * L), rows[lab]))
    assert {q[2] for q in reqs} == set(range(1, 9)) and {q[1] for q in reqs} == set(range(1, 6)) and {q[3] for q in reqs} == set(range(1, 71))
    host = mg.ask_mfgeom_host(host_exe, reqs)
    seen_c, bad = set(), []
    for q, h in zip(reqs, host):
        want = mg.host_tuple(*q)
        seen_c.add(want[8])
        if want != h:
            bad.append((q[:6], want[:12], h[:12]))
    assert not bad, bad[:3]
    assert seen_c == set(range(1, 9))


def test_refusals_and_edges_match_the_header(host_exe):
    """Nine classes and a weight that is not finite are refused with the status capi.hip turns into DFM_E_DIMS, whichever comes
    first in the series order; -0.0 is the class of 0.0; the first series decides the class order."""
    W9 = np.arange(9.0)[:, None] * np.ones((1, 2))
    nan3 = W9[:8].copy(); nan3[3, 1] = np.nan
    inf = W9[:4].copy(); inf[2, 0] = np.inf
    both = W9.copy(); both[8, 0] = np.nan                            # the ninth row is not finite: that is met first
    late = np.vstack([W9, [[np.nan, 0.0]]])                          # ... and here the ninth class is
    zero = np.array([[0.0, 1.0], [-0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    order = np.array([[2.0], [1.0], [2.0], [0.0], [1.0]])
    reqs = [(len(W), W.shape[1], 2, 20, 1, 8, W) for W in (W9, W9[:8], nan3, inf, both, late, zero, order)]
    host = mg.ask_mfgeom_host(host_exe, reqs)
    for q, h in zip(reqs, host):
        assert mg.host_tuple(*q) == h
    assert [mg.deal(q[6])["rc"] for q in reqs] == [2, 0, 1, 1, 1, 2, 0, 0]
    assert mg.deal(zero)["cls"] == [0, 0, 1, 0] and mg.deal(order)["Wc"] == [(2.0,), (1.0,), (0.0,)]
    assert mg.deal(order)["tile_series"] == [[0, 2] + [-1] * 14, [1, 4] + [-1] * 14, [3] + [-1] * 15]


def test_geometry_matches_the_sources():
    """The numbers the sources and DESIGN state about the step."""
    assert [mg.row_width(r) for r in range(1, 9)] == [32, 32, 32, 32, 32, 48, 48, 64]
    assert sum(mg.col_kinds(5)[:16]) == 15 and sum(k == 1 for k in mg.col_kinds(7)) == 28 and mg.col_kinds(7)[28:32] == [0] * 4
    assert mg.mean_cols(8) == list(range(48, 56)) and mg.vech_cols(3) == [0, 1, 2, 3, 4, 5]
    g = mg.grids(139, 5, 4, 90, 2, 32)                             # the Stock-Watson window's width (tests/test_gpu_mf.py)
    assert (g["VW"], g["TT"], g["ngroups"], g["table"], g["solve"], g["loadings"]) == (32, 2, 6, 12, 1, 35)
    d = mg.deal(me.weight_rows(["m"] * 100 + ["q_flow"] * 39))
    assert (d["C"], d["ntiles"], d["tile_class"]) == (2, 10, [0] * 7 + [1] * 3) and d["tile_series"][6][4:] == [-1] * 12
    with open(mg.os.path.join(mg.os.path.dirname(mg.os.path.dirname(mg.os.path.abspath(__file__))), "dynamic_factor_models_amd", "csrc",
                              "dfm_mfgeom.h")) as fh:
        src = fh.read()
    for text in ("kMfMaxClasses = 8, kMfMaxLags = 5", "kMfTile = 16", "kMfWaves = 4", "kMfGroup = 16", "kMfBlock = 256"):
        assert text in src, text


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_class():
    missing = mg.missing_classes(mg.REQUIRED, mg.CASES)
    assert missing == [], f"coverage classes no case hits: {missing}"
    for c in mg.CASES:
        g = mg.geometry(c)
        assert g["N"] <= 300 and c["T"] <= 70 and c["r"] * max(c["p"], g["L"]) <= 32 and g["deal"]["rc"] == 0
        assert c["T"] > 16 or c["r"] <= 2 or all(per == 1 for _, _, per in c["classes"]), c["name"]   # short T: r <= 2 where a class is quarterly
    assert set(mg.BLOCKS_CASES) <= set(IDS)
    blk = [mg.classes(mg.BY_NAME[n]) for n in mg.BLOCKS_CASES]
    assert "N=257" in blk[0] and "C=8" in blk[1] and "ntiles>=5" in blk[2]
    assert [(c["B"], c["r"]) for c, _, _, _ in mg.STOP_CASES] == [(4, 1), (4, 5), (4, 8)]
    assert all(tol > 0.0 and it <= 40 for _, tol, it, _ in mg.STOP_CASES)


@pytest.mark.parametrize("drop,lost", [("r2_t13", "s0:nan_under_padding_of_another_class"), ("r3_t17", "n=r,r+1:quarterly_tile"),
                                       ("r5_t16", "T=16"), ("r8_t33_c8", "wg:four_classes"), ("c1_t20", "C=1")])
def test_dropping_a_case_is_noticed(drop, lost):
    rest = [c for c in mg.CASES if c["name"] != drop]
    assert len(rest) == len(mg.CASES) - 1 and lost in mg.missing_classes(mg.REQUIRED, rest)


def test_every_class_holds_an_updated_series_and_the_kept_ones_are_the_claimed():
    for c in mg.CASES:
        g, (panel, W, _) = mg.geometry(c), mg.batch(c["name"])
        n = (~np.isnan(panel)).sum(1)
        kept = set(mg.kept_series(c["name"]))
        for k, w in enumerate(g["deal"]["Wc"]):
            members = [i for i in range(g["N"]) if g["deal"]["cls"][i] == k]
            assert any(w) == any(i not in kept for i in members), (c["name"], k)
        for i, cells in g["thin"].items():
            assert (n[:, i] == cells).all() and (i in kept) == (cells < c["r"] + 1)
        if "s0:nan_under_padding_of_another_class" in mg.classes(c):
            assert np.isnan(panel[:, :, 0]).any(1).all()
    assert mg.kept_series("r3_t17") and len(mg.zero_class_series(mg.BY_NAME["r5_t16"])) == 3


# ---- the model alone ------------------------------------------------------------------------------------------------------------
def _scale(a):
    return max(1.0, float(np.abs(a).max()))


@pytest.mark.parametrize("name", IDS)
def test_one_iteration_moves_every_watched_series(name):
    """After ONE iteration from the start, lam_i and R_i of every watched series that is updated at all differ from the start by
    more than 1000 times the GPU bound: a series the kernel skipped or addressed wrongly cannot pass.  (The watched series that
    must be kept are compared with the start bit for bit instead.)"""
    c = mg.BY_NAME[name]
    panel, W, start = mg.batch(name)
    kept = set(mg.kept_series(name))
    watched = mg.watched_series(c)
    assert 0 in watched and panel.shape[2] - 1 in watched and len(set(watched) - kept) >= 2
    worst = [np.inf, np.inf]
    for b in range(c["B"]):
        new, _, _ = me.em_step_mf(panel[b], W=W, **{k: start[k][b] for k in mg.KEYS})
        for i in watched:
            dl, dr = np.abs(new["Lam"][i] - start["Lam"][b, i]).max(), abs(new["R"][i] - start["R"][b, i])
            if i in kept:
                assert dl == 0.0 and dr == 0.0
                continue
            worst = [min(worst[0], dl / _scale(new["Lam"])), min(worst[1], dr / _scale(new["R"]))]
            assert dl > MARGIN * PARAM_TOL * _scale(new["Lam"]) and dr > MARGIN * PARAM_TOL * _scale(new["R"]), (b, i, dl, dr)
    print(f"\n  {name}: smallest move of a watched series: Lam {worst[0]:.2e}  R {worst[1]:.2e}")


def _param_gap(a, b):
    return max(float(np.abs(a[k] - b[k]).max()) / _scale(b[k]) for k in ("Lam", "R"))


@pytest.mark.parametrize("mutant", list(mg.MUTANTS))
def test_the_table_tells_a_wrong_kernel_from_the_right_one(mutant):
    """Each wrong series step, put in the model's place, differs from the model by more than 1000 times the bound in Lam or R --
    on EVERY case that claims the class, which is more than the one the table needs."""
    claim = [c for c in mg.CASES if mg.MUTANTS[mutant] in mg.classes(c)]
    assert claim
    for c in claim:
        e = mg.expected(c["name"])
        gap = max(_param_gap(mg.em_variant(e["panel"][b], {k: e["start"][k][b] for k in mg.KEYS}, e["W"], mutant=mutant)[0],
                             e["ems"][b]["est"]) for b in range(c["B"]))
        print(f"\n  {mutant} on {c['name']}: {gap:.2e}")
        assert gap > MARGIN * PARAM_TOL, (c["name"], gap)


def test_the_variant_without_a_mutation_is_the_model():
    e = mg.expected("r3_t17")
    got, path, _ = mg.em_variant(e["panel"][1], {k: e["start"][k][1] for k in mg.KEYS}, e["W"])
    assert np.array_equal(path, e["ems"][1]["path"])
    assert _param_gap(got, e["ems"][1]["est"]) <= 1e-12


@pytest.mark.parametrize("name", IDS)
def test_reference_noise_is_a_hundredth_of_every_bound(name):
    """The model twice: as the GPU test uses it, and with the series in another order and the time sums of the series step taken
    from the last period to the first.  Every quantity the GPU test compares agrees to 1 % of its bound."""
    c = mg.BY_NAME[name]
    e = mg.expected(name)
    N = e["W"].shape[0]
    perm = np.random.default_rng([3, N]).permutation(N)
    worst = {}
    for b in range(c["B"]):
        ref = e["ems"][b]
        st = {k: e["start"][k][b] for k in mg.KEYS}
        st = dict(st, Lam=st["Lam"][perm], R=st["R"][perm])
        got, path, out = mg.em_variant(e["panel"][b][:, perm], st, e["W"][perm], reverse=True)
        got = dict(got, Lam=got["Lam"][np.argsort(perm)], R=got["R"][np.argsort(perm)])
        err = dict(path=float(np.abs(path / ref["path"] - 1.0).max()) / PATH_RTOL,
                   f=float(np.abs(out["f_smooth"][:, :c["r"]] - ref["f"]).max()) / _scale(ref["f"]) / F_TOL,
                   P=float(np.abs(mg._packed(out["P_smooth"], c["r"]) - ref["P"]).max() / np.abs(ref["P"]).max()) / P_RTOL)
        for k in mg.KEYS:
            err[k] = float(np.abs(got[k] - ref["est"][k]).max()) / _scale(ref["est"][k]) / PARAM_TOL
        for k, v in err.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n  {name}: noise / bound  " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.01, worst


@pytest.mark.parametrize("k", range(len(mg.STOP_CASES)), ids=STOP_IDS)
def test_stop_cases_stop_at_different_iterations(k):
    """From the model alone: the replicates' iteration counts differ, are at least 2 and stay below max_iter; the first stopper is
    replicate 0 (the first two cases) or the last replicate (the third), alone; every decision of the stop rule has 1e-6 of room
    around tol (fifty times what a path held to 1e-8 can move the criterion)."""
    case, tol, max_iter, slow = mg.STOP_CASES[k]
    e = mg.expected_stop(k)
    its = [len(em["path"]) for em in e["ems"]]
    print(f"\n  {case['name']}: iterations {its}")
    assert min(its) >= 2 and max(its) < max_iter
    first = 0 if k < 2 else case["B"] - 1
    assert first not in slow and all(its[first] < its[b] for b in range(case["B"]) if b != first), its
    for em in e["ems"]:
        path = em["path"]
        crit = np.diff(path) / (0.5 * (np.abs(path[1:]) + np.abs(path[:-1])))
        assert np.abs(crit - tol).min() >= 1e-6 and (crit[:-1] >= tol).all() and crit[-1] < tol
