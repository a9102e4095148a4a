"""CPU checks of tests/gibbs_geometry.py, no device needed: the case table of tests/test_gpu_gibbs_geometry.py against the coverage
classes it must hit and against the eight instances of gibbs_load_kernel a brute-force walk over (r, p) reaches; the series split of
every row against csrc/dfm_cellgeom.h itself through tests/host/seriesgeom_host.cpp; the constants and launch lines the restatement
takes from csrc/gibbs.hip, read from the source; and the conditions under which the reference alone holds the GPU tolerance --
conditions, not measurements: every edge kind meant for a row is in its panel, 1e-13 of relative noise on the start or on the factor
path moves no output of the reference by more than a hundredth of the tolerance, and no Gamma accept of streams 6 and 9 is decided
within 1e-6 of its boundary."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import ar_geometry as ag
from tests import gibbs_expect as ge
from tests import gibbs_geometry as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = gg.KEYS
TOL = 1e-9                           # the GPU tests' tolerance, of max(1, scale)
MARGIN = 100.0                       # 1e-13 of noise moves a reference by less than TOL / MARGIN
NOISE = 1e-13
DUPLICATES = set()                   # rows that hold no class alone (none: every row of gibbs_geometry.CASES names its own)
OUT = ("Lam", "R", "A", "Q", "f")


# ------------------------------------------------------------------------------------------------------------- coverage, instances
def test_case_table_covers_every_class():
    assert len(set(gg.NAMES)) == len(gg.NAMES)
    missing = gg.missing_classes()
    assert not any(missing.values()), f"coverage classes no case hits: {missing}"
    # the rows the GPU module runs under both values of the flag: balanced, one per bucket, admitted under the flag too
    rows = [gg.case_dict(gg._row(n)) for n in gg.BUCKET_ROWS]
    assert [gg.bucket(c["r"]) for c in rows] == [4, 8, 16, 32] and not any(c["flag"] for c in rows)
    assert all(gg.pass_admits(c["N"], c["r"], c["p"], True) and c["N"] <= gg.table_max_n(c["r"], c["p"]) for c in rows)
    # ... and twice for equal bytes: k = 32 at p > 1, three series blocks
    k32, blocks3 = (gg.case_dict(gg._row(n)) for n in gg.REPEAT_ROWS)
    assert k32["r"] * k32["p"] == 32 and k32["p"] > 1 and gg.launches(blocks3)["load"]["nsblk"] >= 3


@pytest.mark.parametrize("name", gg.NAMES)
def test_dropping_a_row_is_noticed(name):
    rest = [row for row in gg.CASES if row[0] != name]
    assert len(rest) == len(gg.CASES) - 1
    lost = gg.missing_classes(rest)
    assert any(lost.values()) != (name in DUPLICATES), (name, lost)


def test_reachable_instances_are_what_the_admission_rules_give():
    """A walk over every (r, p) gibbs_check admits, dispatch_r_bucket applied to it, under either value of the flag."""
    shapes = [(r, p) for r in range(1, 40) for p in range(1, 40) if gg.shape_admits(p + 1, r, p)]
    assert shapes and all(r * p <= 32 for r, p in shapes) and (32, 1) in shapes and (1, 32) in shapes and (33, 1) not in shapes
    assert not gg.shape_admits(4, 2, 4) and gg.shape_admits(5, 2, 4)
    assert {(gg.bucket(r), miss) for r, p in shapes for miss in (False, True)} == set(gg.LOAD_INSTANCES) and len(gg.LOAD_INSTANCES) == 8
    assert [gg.bucket(r) for r in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]
    seen = {(g["RB"], g["MISS"]) for g in (gg.launches(gg.case_dict(row))["load"] for row in gg.CASES)}
    assert seen == set(gg.LOAD_INSTANCES)
    # the var kernel's accumulators hold every admitted shape: k k + k r + r r <= 12 x 256 (3072 at (32, 1))
    assert max(r * p * r * p + r * p * r + r * r for r, p in shapes) == gg.VAR_ACC * gg.THREADS
    assert all(gg.launches(gg.case_dict(row))["var"]["ept"] <= gg.VAR_ACC for row in gg.CASES)
    # ... and the staged rows its LDS buffer st[2048]: (32 + p) r doubles
    assert max((gg.VAR_TC + p) * r for r, p in shapes) <= 2048


def test_case_table_respects_the_entries_limits():
    for row in gg.CASES:
        c = gg.case_dict(row)
        N, T, r, p = c["N"], c["T"], c["r"], c["p"]
        assert gg.shape_admits(T, r, p) and gg.pass_admits(N, r, p, c["flag"]), c["name"]
        assert not c["flag"] or N <= gg.table_max_n(r, p), c["name"]
        assert p == 1 or N <= gg.table_max_n(r, p), c["name"]                        # varp_run checks N whatever the flag says
        assert N * T <= gg.MAX_CELLS, c["name"]
        assert c["pattern"] in (None, "edge") or (isinstance(c["pattern"], float) and T < gg.TC), c["name"]
        assert c["pattern"] != "edge" or T > gg.TC, c["name"]
        assert c["empty"] is None or (c["flag"] and 0 <= c["empty"] < N), c["name"]
    assert [gg.table_max_n(r, p) for r, p in ((8, 1), (2, 4), (9, 1), (4, 4), (17, 1), (8, 4), (1, 32))] == [1024, 1024, 512, 512, 256, 256, 256]
    # the pass's own rule: the plain model at width 32 under the flag takes any N; p > 1 is held to pad_r(r), flag or not
    assert gg.pass_admits(1000, 20, 1, True) and gg.pass_admits(999, 32, 1, True) and not gg.pass_admits(513, 9, 1, True)
    assert gg.pass_admits(5000, 9, 1, False) and not gg.pass_admits(1025, 8, 4, False) and gg.pass_admits(1024, 8, 4, True)
    assert ag.pad_r(1) == 2 and ag.pad_r(17) == 32 and ag.pad_r(9) == 16


# ------------------------------------------------------------------------------------------------------------- the compiled header
def test_series_split_of_every_row_against_the_header(tmp_path):
    exe = str(tmp_path / "seriesgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "seriesgeom_host.cpp")], check=True)
    loads = [gg.launches(gg.case_dict(row))["load"] for row in gg.CASES]
    text = "".join(" ".join(map(str, g["call"])) + "\n" for g in loads)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(loads)
    for g, line in zip(loads, out):
        NPB, G, RC, nchunk, nsblk, threads = map(int, line.split())
        assert (NPB, nsblk, threads) == (g["npb"], g["nsblk"], g["threads"]), (g["call"], line)
        assert g["nsblk"] * g["npb"] >= g["call"][0] > (g["nsblk"] - 1) * g["npb"] and g["threads"] <= gg.THREADS


def test_the_launchers_say_what_the_restatement_says():
    """The constants and rules `launches` takes from the sources, read from the sources."""
    src = lambda f: open(os.path.join(ROOT, "dynamic_factor_models_amd", "csrc", f)).read()
    gb, cg, capi = src("gibbs.hip"), src("dfm_cellgeom.h"), src("capi.hip")
    assert f"constexpr int kGbTC = {gg.TC};" in gb and f"constexpr int kGbVarTC = {gg.VAR_TC};" in gb
    assert f"constexpr int kGbThreads = {gg.THREADS};" in gb and f"constexpr int kCellBlockLanes = {gg.BLOCK_LANES};" in cg
    assert "const int nsblk = (a.N + kCellBlockLanes - 1) / kCellBlockLanes, npb = (a.N + nsblk - 1) / nsblk;" in gb
    assert "block((unsigned)((npb + 63) / 64 * 64));" in gb
    assert "const int nsblk = gridDim.y, npb = (N + nsblk - 1) / nsblk;" in gb               # the kernel recomputes the launcher's npb
    assert "if (a.r * a.p > 32 || a.T <= a.p) return hipErrorInvalidValue;" in gb
    assert "for (int t0 = 0; t0 < T; t0 += kGbTC)" in gb and "for (int c0 = p; c0 < T; c0 += kGbVarTC)" in gb
    assert f"double acc[{gg.VAR_ACC}];" in gb and "sS[1024], sL[1024], sU[1024], sP[1024], sC[1024], st[2048];" in gb
    assert "constexpr bool REG = RB <= 16;" in gb and "const int n = REG ? RB : r;" in gb
    for line in ("if (r <= 4) return f(std::integral_constant<int, 4>{});", "if (r <= 8) return f(std::integral_constant<int, 8>{});",
                 "if (r <= 16) return f(std::integral_constant<int, 16>{});", "return f(std::integral_constant<int, 32>{});"):
        assert line in cg, line
    # the sweep: the gram kernel only without the flag; the pass's admission
    assert "if (!missing) HIP_LAUNCH(h, K_GB_GRAM, launch_gibbs_gram(a, h->stream));" in capi
    assert capi.count("launch_gibbs_gram(") == 1
    assert "int collapse_max_n(int Rpad) { return Rpad <= 8 ? 1024 : Rpad <= 16 ? 512 : 256; }" in src("collapse.hip")
    assert "if (plain && pad_r(r) == 32 && (collapse_wide2_supported(32, N) || collapse_wide2_supported(32, N + 1))) return 0;" in capi
    assert "if (N > collapse_max_n(pad_r(r)))" in capi
    assert "if (T <= p) return fail(h, DFM_E_DIMS, \"T must be > p" in capi


# ------------------------------------------------------------------------------------------------------------- the panels
def test_edge_pattern_at_the_load_kernels_chunk():
    """ar_post_geometry.edge_pattern at q = 0, rc = 64: each kind sits on the rows 63 | 64 (and 127 | 128)."""
    T, N = 131, 16
    x = np.arange(T * N, dtype=float).reshape(T, N)
    used = gg.edge_pattern(x, 0, rc=gg.TC)
    assert used == {(e, k) for e in (64, 128) for k in range(gg.N_EDGE_KINDS)}
    for i in range(N):
        kind, e = i % 8, 64 if i < 8 else 128
        gone = set(np.nonzero(np.isnan(x[:, i]))[0])
        want = [{e - 1, e}, {e - 3, e - 2, e - 1}, {e, e + 1}, {e - 1}, None, None, None, {0, e}][kind]
        if want is not None:
            assert gone == want, (i, gone)
        else:
            assert set(range(T)) - gone == {e - 1 if kind == 4 else e if kind == 5 else T - 1}, i


@pytest.mark.parametrize("name", gg.NAMES)
def test_every_kind_meant_for_a_case_is_in_its_panel(name):
    c = gg.make_case(name)
    x = c["x"]
    n_i = (~np.isnan(x)).sum(axis=1)                             # [B, N]
    if c["pattern"] == "edge":
        assert c["kinds"] == gg._edge_kinds(c) and c["kinds"]
        for e, kind in c["kinds"]:
            hit = False
            for b in range(gg.B):
                for i in (i for i in range(c["N"]) if (i + b) % 8 == kind and i != c["empty"]):
                    col = np.isnan(x[b, :, i])
                    if kind in (4, 5, 6):
                        row = e - 1 if kind == 4 else e if kind == 5 else c["T"] - 1
                        hit |= n_i[b, i] == 1 and not col[row]
                    else:
                        rows = [{e - 1, e}, {e - 3, e - 2, e - 1}, {e}, {e - 1}, None, None, None, {0, e}][kind]
                        hit |= rows <= set(np.nonzero(col)[0])
            assert hit, (name, e, kind)
        if any(kind in (4, 5, 6) for _, kind in c["kinds"]):
            assert (n_i == 1).any(), "no series with a single observed cell"
    elif c["pattern"] is None:
        assert not np.isnan(x).any() and not c["flag"]
    else:
        assert np.isnan(x).any() and (n_i > 0).all()
    if c["empty"] is not None:
        assert (n_i[:, c["empty"]] == 0).all()
    for cls in (k for k in gg.classes(c)["load"] if k.startswith("edge@")):
        e, kind = cls[5:].split(":")
        assert (int(e), int(kind)) in c["kinds"], cls
    assert ("n_i=0" in gg.classes(c)["load"]) == bool((n_i == 0).any())


# ------------------------------------------------------------------------------------------------------------- conditioning
def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def _moves(name):
    """({key: move of the whole sweep}, {key: move of the block alone}) of chain 0, sweep 0, relative to max(1, scale)."""
    c = gg.make_case(name)
    rng = np.random.default_rng([c["N"], c["T"], c["r"], c["p"]])
    b, p = 0, c["p"]
    pr = gg.chain_prior(c, b)
    ref = gg.first_sweep(name, b)
    assert all(np.isfinite(ref[k]).all() for k in OUT)
    st = {k: c["st"][k][b] * (1.0 + NOISE * rng.standard_normal(c["st"][k][b].shape)) for k in KEYS}
    st["Q"], st["P0"] = 0.5 * (st["Q"] + st["Q"].T), 0.5 * (st["P0"] + st["P0"].T)
    moved = ge.sweep(c["x"][b], *[st[k] for k in KEYS], p, pr, c["seed"], 0, b)
    assert np.array_equal(moved["att_R"], ref["att_R"]) and np.array_equal(moved["att_Q"], ref["att_Q"])
    whole = {k: _rel(moved[k], ref[k]) for k in OUT}
    rnd = ge.stream_randoms(c["seed"], 0, b, c["T"], c["N"], c["r"], p)
    f = ref["f"] * (1.0 + NOISE * rng.standard_normal(ref["f"].shape))
    Lam, R, _ = ge.draw_loadings(c["x"][b], f, pr, rnd["lam_n"], rnd["gam_R"])
    A, Q, _ = ge.draw_var(f, p, pr, rnd["E"], rnd["bart_n"], rnd["gam_Q"])
    cond = {k: _rel(v, ref[k]) for k, v in (("Lam", Lam), ("R", R), ("A", A), ("Q", Q))}
    return whole, cond


@pytest.mark.parametrize("name", gg.NAMES)
def test_reference_is_insensitive_to_the_start_and_to_the_path(name):
    """1e-13 of relative noise on every start parameter moves no output of gibbs_expect.sweep, and the same noise on f no output of
    draw_loadings / draw_var, by more than TOL / 100."""
    whole, cond = _moves(name)
    fmt = lambda d: ", ".join(f"{k} {v:.1e}" for k, v in d.items())
    print(f"{name}: reference moves, whole sweep {fmt(whole)}; block alone {fmt(cond)}")
    assert max(whole.values()) <= TOL / MARGIN, whole
    assert max(cond.values()) <= TOL / MARGIN, cond


def test_worst_reference_move_of_the_table():
    whole = max((max(_moves(n)[0].values()), n) for n in gg.NAMES)
    cond = max((max(_moves(n)[1].values()), n) for n in gg.NAMES)
    print(f"worst reference move of the table: whole sweep {whole[0]:.2e} ({whole[1]}), block alone {cond[0]:.2e} ({cond[1]}); "
          f"the GPU tolerance is {TOL:.0e}, the bound {TOL / MARGIN:.0e}")
    assert max(whole[0], cond[0]) <= TOL / MARGIN


def test_gamma_accepts_are_decided_away_from_their_boundary_and_rejections_are_met():
    """No accept of streams 6 and 9 within 1e-6 of its boundary, none at the cap; a rejected attempt of stream 6 on a series the edge
    pattern touched and one of stream 9, somewhere in the table."""
    rej6 = rej9 = edge6 = 0
    worst = np.inf
    for name in gg.NAMES:
        c = gg.make_case(name)
        touched = gg.edge_series(c) if c["pattern"] == "edge" else np.zeros((gg.B, c["N"]), bool)
        for b in range(gg.B):
            for j in range(gg.SWEEPS):
                att_R, att_Q, margin = gg.gamma_margins(c, b, j)
                assert margin >= 1e-6, f"{name} b={b} sweep={j}: a Gamma attempt within {margin:.2e} of its accept boundary"
                assert att_R.max() < ge.GAMMA_CAP and att_Q.max() < ge.GAMMA_CAP, f"{name} b={b} sweep={j}: the Gamma cap"
                worst = min(worst, margin)
                rej6 += int(att_R.sum()); rej9 += int(att_Q.sum()); edge6 += int(att_R[touched[b]].sum())
        o = gg.first_sweep(name)                                 # the counts above are the model's own
        a6, a9, _ = gg.gamma_margins(c, 0, 0)
        assert np.array_equal(o["att_R"], a6) and np.array_equal(o["att_Q"], a9), name
    print(f"smallest accept margin {worst:.2e}; rejected attempts: stream 6 {rej6} ({edge6} on series the edge pattern touched), "
          f"stream 9 {rej9}")
    assert rej6 > 0 and rej9 > 0 and edge6 > 0
