"""CPU checks of tests/ar_post_geometry.py, no device needed: the case table of tests/test_gpu_ar_post_geometry.py against the coverage
classes it must hit and against the template instances the admission rules of csrc/capi.hip can reach (a brute-force walk over
(r, p, q)); every launch of the table against csrc/dfm_cellgeom.h itself through the two host programs the forecast's and the filter's
CPU tests already build; and the conditions under which the references alone hold the GPU tolerances -- conditions, not
measurements: the kernels' two-filter recursion is dense conditioning on every series of every case, every edge kind meant for a
case is in its panel, the references do not move under 1e-13 of relative noise on the start, and the Gibbs rows decide no accept
within 1e-6 of its boundary."""
import os
import subprocess

import numpy as np
import pytest

from tests import ar_geometry as ag
from tests import ar_post_geometry as apg
from tests import filter_ar_expect as fte
from tests import forecast_ar_expect as fe
from tests import gibbs_ar_expect as gae
from tests import gibbs_expect as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = apg.KEYS
TOL = 1e-9                           # the GPU tests' tolerance, of max(1, scale)
MARGIN = 100.0                       # 1e-13 of noise on the start moves a reference by less than TOL / MARGIN
DUPLICATES = {"r16_p2"}              # rows whose comment in ar_post_geometry.CASES says what they repeat and why they stay
GIBBS_NAMES = [n for n in apg.NAMES if "gibbs" in apg.products(apg.case_dict(apg._row(n)))]


# ------------------------------------------------------------------------------------------------------------- coverage, instances
def test_case_table_covers_every_class():
    assert len(set(apg.NAMES)) == len(apg.NAMES)
    missing = apg.missing_classes()
    assert not any(missing.values()), f"coverage classes no case hits: {missing}"


@pytest.mark.parametrize("name", apg.NAMES)
def test_dropping_a_row_is_noticed(name):
    rest = [row for row in apg.CASES if row[0] != name]
    assert len(rest) == len(apg.CASES) - 1
    lost = apg.missing_classes(rest)
    assert any(lost.values()) != (name in DUPLICATES), (name, lost)


def test_reachable_instances_are_what_the_admission_rules_give():
    """A walk over every (r, p, q) the rules admit, each launcher's own bucket rule applied to it."""
    shapes = [(r, p, q) for r in range(1, 40) for p in range(1, 40) for q in range(0, 7) if apg.ar_admits(r, p, q)]
    assert shapes and all(1 <= q <= 4 and r * max(p, q + 1) <= 32 for r, p, q in shapes)
    assert {(q, apg.rb_series(r)) for r, p, q in shapes} == set(apg.SERIES_INSTANCES) and len(apg.SERIES_INSTANCES) == 10
    assert {(q, 4 if r <= 4 else 8) for r, p, q in shapes if apg.gibbs_admits(r, p, q)} == set(apg.GIBBS_INSTANCES)
    assert len(apg.GIBBS_INSTANCES) == 8 and max(r for r, p, q in shapes if apg.gibbs_admits(r, p, q)) == 8
    assert {apg.rb_series(r) for r, p, q in shapes} == set(apg.EVAL_INSTANCES) == {4, 8, 16}
    fills = {(fte.w_bucket(r * (q + 1)), sp) for r, p, q in shapes for sp in (1, 2) if sp == 1 or fte.w_bucket(r * (q + 1)) <= 16}
    assert fills == set(apg.FILL_INSTANCES) and len(apg.FILL_INSTANCES) == 7
    # what the launchers compile and no admitted shape reaches
    assert not set(apg.COMPILED_UNREACHABLE) & set(apg.SERIES_INSTANCES)
    assert set(apg.COMPILED_UNREACHABLE) | set(apg.SERIES_INSTANCES) == {(q, rb) for q in (1, 2, 3, 4) for rb in (4, 8, 16)}
    assert max(r for r, p, q in shapes if q == 3) == 8 and max(r for r, p, q in shapes if q == 4) == 6


def test_case_table_reaches_every_reachable_instance_of_every_launcher():
    seen = {}
    for row in apg.CASES:
        for prod, ks in apg.launches(apg.case_dict(row)).items():
            for g in ks:
                key = (g["WB"], g["SP"]) if "WB" in g else (g["Q"], g["RB"]) if "Q" in g else g.get("RB")
                seen.setdefault(g["kernel"], set()).add(key)
    for kernel in ("forecast_ar_back_kernel", "forecast_ar_fwd_kernel", "simsmooth_ar_diff_kernel", "simsmooth_ar_fwd_kernel"):
        assert seen[kernel] == set(apg.SERIES_INSTANCES), kernel
    assert seen["gibbs_ar_series_kernel"] == set(apg.GIBBS_INSTANCES)
    assert seen["filter_ar_eval_kernel"] == set(apg.EVAL_INSTANCES)
    assert seen["filter_ar_fill_kernel"] == set(apg.FILL_INSTANCES)


def test_case_table_respects_the_entries_limits():
    for row in apg.CASES:
        c = apg.case_dict(row)
        assert apg.ar_admits(c["r"], c["p"], c["q"]) and c["N"] <= apg.max_n(c["r"], c["p"], c["q"]), c["name"]
        assert c["q"] <= c["t0"] < c["T"] and c["T"] > c["q"] and c["H"] >= 0, c["name"]
        assert c["N"] * (c["T"] + c["H"]) <= 520 * 70, c["name"]                     # one tiny batch per test id
        assert ("gibbs" in apg.products(c)) == (c["r"] <= 8 and c["T"] - c["q"] > c["p"]), c["name"]
    scaled = sum(bool(row[9]) for row in apg.CASES)
    assert len(apg.CASES) // 2 - 1 <= scaled <= len(apg.CASES) // 2 + 2
    long_rows = [apg.case_dict(row) for row in apg.CASES if row[2] + row[6] - row[5] >= 34]
    assert sum(c["pattern"] == "edge" for c in long_rows) > len(long_rows) // 2
    assert any(c["pattern"] == "edge" and c["r"] <= 8 and c["T"] - c["q"] > c["p"] for c in long_rows)


# ------------------------------------------------------------------------------------------------------------- the compiled header
def test_every_launch_of_the_table_against_the_header(tmp_path):
    """series_geometry for the series kernels' calls and launch_filter_ar_fill's geometry for the fill, from the two host programs."""
    exes = {}
    for prog in ("seriesgeom_host", "filter_ar_geom_host"):
        exes[prog] = str(tmp_path / prog)
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", exes[prog], os.path.join(ROOT, "tests", "host", prog + ".cpp")], check=True)

    def ask(prog, reqs):
        text = "".join(" ".join(map(str, q)) + "\n" for q in reqs)
        out = subprocess.run([exes[prog]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(reqs)
        return [tuple(map(int, line.split())) for line in out]

    series, fills = [], []
    for row in apg.CASES:
        c = apg.case_dict(row)
        for ks in apg.launches(c).values():
            for g in ks:
                if "Q" in g:
                    series.append(g)
                elif "WB" in g:
                    fills.append((c, g))
    assert len(series) == 5 * len(apg.CASES) + 4 * len(GIBBS_NAMES) and len(fills) == len(apg.CASES)
    for g, got in zip(series, ask("seriesgeom_host", [g["call"] for g in series])):
        assert got == tuple(g[f] for f in ("NPB", "G", "RC", "nchunk", "nsblk", "threads")), (g["kernel"], g["call"], got)
        N, row_doubles, n, lds = g["call"]
        assert g["RC"] == min(apg.RC, n) and g["RC"] * row_doubles * 8 <= lds, "the LDS cap binds on a series kernel"
        assert g["RB"] >= row_doubles or g["kernel"] != "gibbs_ar_series_kernel"
    reqs = [(c["N"], g["w"], c["T"] - c["q"], 1) for c, g in fills]
    for (c, g), got in zip(fills, ask("filter_ar_geom_host", reqs)):
        SP, WB, row_doubles = got[:3]
        assert (SP, WB, row_doubles) == (g["SP"], g["WB"], fte.fill_row_doubles(c["r"], c["q"])), c["name"]
        assert got[3:] == tuple(g[f] for f in fte.pg.GEOM_FIELDS), c["name"]


def test_the_launchers_say_what_the_restatement_says():
    """The constants and bucket rules `launches` takes from the sources, read from the sources."""
    src = lambda f: open(os.path.join(ROOT, "dynamic_factor_models_amd", "csrc", f)).read()
    fc, ss, gb, cg = src("forecast_ar.hip"), src("simsmooth_ar.hip"), src("gibbs_ar.hip"), src("dfm_cellgeom.h")
    assert "constexpr size_t kFcArLds = 48 * 1024;" in fc and "constexpr size_t kSsArLds = 48 * 1024;" in ss
    assert "constexpr size_t kGbArLds = 48 * 1024;" in gb and "constexpr int kSsArLdsTail = 64;" in src("dfm_fcar.h")
    assert "constexpr int kFtEvalChunk = 64;" in src("dfm_filter.h")
    assert f"kSeriesChunkRows = {apg.RC};" in cg
    assert "kind == kFcArBack ? a.r : kind == kFcArDraw ? 2 * a.r : a.r + (a.xvar ? np : 0)" in fc
    assert "series_geometry(a.N, a.r, a.n, kSsArLds - tail)" in ss
    assert "const int RB = a.r <= 4 ? 4 : 8;" in gb and "series_geometry(a.N, RB, a.n, kGbArLds - lag)" in gb
    assert "if (a.r <= 4) return launch_fc_ar_q<Q, 4>(a, kind, s);" in fc and "if (a.r <= 8) return launch_fc_ar_q<Q, 8>(a, kind, s);" in fc


# ------------------------------------------------------------------------------------------------------------- the edge pattern
def test_edge_pattern_puts_each_kind_at_the_edge():
    q, T, N = 2, 80, 32
    x = np.arange(T * N, dtype=float).reshape(T, N)
    used = apg.edge_pattern(x, q)
    assert used == {(e, k) for e in (32, 64) for k in range(apg.N_EDGE_KINDS)}
    out = np.isnan(x[q:])                                       # output rows
    for i in range(N):
        kind, e = i % 8, 32 if (i // 8) % 2 == 0 else 64
        rows = set(np.nonzero(out[:, i])[0])
        seen = set(np.nonzero(~np.isnan(x[:, i]))[0])
        want = [{e - 1, e}, {e - 3, e - 2, e - 1}, {e, e + 1}, set(range(e - 1, e + q)), None, None, None, {0, e}][kind]
        if want is not None:
            assert rows == want and not np.isnan(x[:q, i]).any(), (i, rows)
        else:
            assert seen == {q + e - 1 if kind == 4 else q + e if kind == 5 else T - 1}, (i, seen)
    # a panel that ends on the edge: only the kind that needs no row behind it
    assert apg.edge_pattern(np.zeros((q + 32, 8)), q) == {(32, 4)}
    assert apg.edge_pattern(np.zeros((q + 31, 8)), q) == set()


@pytest.mark.parametrize("name", apg.NAMES)
def test_every_kind_meant_for_a_case_is_in_its_panel(name):
    c = apg.make_case(name)
    if c["pattern"] == "edge":
        assert c["kinds"] == apg._edge_kinds(c) and c["kinds"]
        for _, kind in c["kinds"]:                              # the three kinds that leave one observed cell did so
            assert kind not in (4, 5, 6) or ((~np.isnan(c["x"])).sum(axis=1) == 1).any()
    elif c["pattern"] is not None:
        assert c["kinds"], name
    else:
        assert not np.isnan(c["x"]).any()
    for prod, s in apg.classes(c).items():                      # the classes claimed from the pattern alone are in the panel
        for cls in (k for k in s if k.startswith("edge@")):
            e, kind = int(cls[5:7]), int(cls[-1])
            assert (e, kind) in c["kinds"], (prod, cls)


# ------------------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", apg.NAMES)
def test_two_filter_recursion_is_dense_conditioning_on_every_series(name):
    """The bound of tests/test_forecast_ar_cpu.py, on the panel's own cells of the output rows followed by the horizon."""
    c = apg.make_case(name)
    N, q, H = c["N"], c["q"], c["H"]
    worst = 0.0
    for b in range(apg.B):
        u = np.vstack([c["x"][b][q:], np.full((H, N), np.nan)])
        for i in range(N):
            rho, sig2, v0 = c["st"]["rho"][b, i], c["st"]["sig2"][b, i], c["v0"][b, i]
            assert np.abs(rho).sum() <= 0.85 + 1e-12
            e1, V1 = fe.dense_idio(u[:, i], rho, sig2, v0)
            e2, V2, stored = fe.two_filter(u[:, i], rho, sig2, v0)
            obs = ~np.isnan(u[:, i])
            assert stored == [t for t in range(len(obs)) if not obs[t] and obs[t + 1:].any()]
            worst = max(worst, np.abs(e1 - e2).max(), np.abs(V1 - V2).max())
    print(f"{name}: worst difference {worst:.2e}")
    assert worst <= 1e-12


def _rel(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float(np.abs(got[ok] - want[ok]).max() / max(1.0, np.abs(want[ok]).max())) if ok.any() else 0.0


@pytest.mark.parametrize("name", apg.NAMES)
def test_references_are_insensitive_to_the_start(name):
    """The references' own error: Q and P0 of the start are well conditioned (cond <= 1e4), every expectation is finite where it is
    defined, and 1e-13 of relative noise on every parameter moves no output of the forecast's and the filter's references by more
    than a hundredth of the GPU tolerance."""
    c = apg.make_case(name)
    rng = np.random.default_rng([c["N"], c["T"], c["r"], c["p"], c["q"]])
    for b in range(apg.B):
        for k in ("Q", "P0"):
            ev = np.linalg.eigvalsh(c["st"][k][b])
            assert ev[0] > 0.0 and ev[-1] <= 1e4 * ev[0], (k, b, ev[0], ev[-1])
        assert all(np.isfinite(v).all() for v in apg.forecast_expected(name)[b].values())
    b = 0
    st = {k: c["st"][k][b] * (1.0 + 1e-13 * rng.standard_normal(c["st"][k][b].shape)) for k in KEYS}
    st["Q"], st["P0"] = 0.5 * (st["Q"] + st["Q"].T), 0.5 * (st["P0"] + st["P0"].T)
    sc = apg._scales(c, b)
    moved = fe.expect(c["x"][b], *[st[k] for k in KEYS], c["H"], v0=c["v0"][b], **sc)
    ref = apg.forecast_expected(name)[b]
    worst = {k: _rel(np.asarray(moved[k], float), np.asarray(ref[k], float)) for k in ref}
    moved = fte.expect(c["x"][b], *[st[k] for k in KEYS], H=apg.eval_horizons(c), t0=c["t0"], **sc)
    ref = apg.filter_expected(name)[b]
    assert np.array_equal(moved.get("cnt"), ref.get("cnt"))
    worst.update({k: _rel(np.asarray(moved[k], float), np.asarray(ref[k], float)) for k in ref if k != "cnt"})
    print(f"{name}: largest relative moves {sorted(worst.items(), key=lambda kv: -kv[1])[:3]}")
    assert max(worst.values()) <= TOL / MARGIN, worst


@pytest.mark.parametrize("name", [n for n in apg.NAMES if apg.case_dict(apg._row(n))["H"] > 0])
def test_the_filter_rows_count_origins(name):
    """The evaluation's comparison must not pass on NaN alone."""
    c = apg.make_case(name)
    for b, e in enumerate(apg.filter_expected(name)):
        assert (e["cnt"] > 0).mean() >= 0.5, float((e["cnt"] > 0).mean())
        if c["T"] - 1 - c["t0"] > apg.EVAL_CHUNK:               # the first origin of the second chunk counts at horizon 1 for a
            t = c["t0"] + apg.EVAL_CHUNK                        # quarter of the series at least (the edge pattern sits around it)
            obs = ~np.isnan(c["x"][b])
            assert (obs[t - c["q"] + 1:t + 2].all(axis=0) & (e["cnt"][0] > 1)).sum() >= c["N"] // 4


# ------------------------------------------------------------------------------------------------------------- the Gibbs rows
def test_gibbs_rows_decide_nothing_at_a_boundary_and_reject_on_an_edge_series():
    """What tests/test_gibbs_ar_cpu.py asserts of its own table, on this one; and at least one rejected rho attempt on a series the
    edge pattern touched, in a walk that crosses a chunk edge."""
    assert len(GIBBS_NAMES) >= 8
    rej_rho = rej_gam = n0 = edge_rej = 0
    for name in GIBBS_NAMES:
        c = apg.make_case(name)
        touched = apg.edge_series(c) if c["pattern"] == "edge" and c["T"] - c["q"] > apg.RC else np.zeros((apg.B, c["N"]), bool)
        for b, sweeps in enumerate(apg.gibbs_chains(name)):
            for j, o in enumerate(sweeps):
                where = f"{name} b={b} sweep={j}"
                assert all(np.isfinite(o[k]).all() for k in ("Lam", "sig2", "rho", "A", "Q", "f")), where
                assert o["margin_rho"] >= 1e-6, f"{where}: a rho attempt within {o['margin_rho']:.2e} of |kappa| = 1"
                assert o["margin_gamma"] >= 1e-6, f"{where}: a Gamma attempt within {o['margin_gamma']:.2e} of its accept boundary"
                assert (o["att_R"] < ge.GAMMA_CAP).all() and (o["att_Q"] < ge.GAMMA_CAP).all(), f"{where}: the Gamma cap"
                assert not (o["att_rho"] == gae.RHO_CAP).any(), f"{where}: the rho cap"
                rej_rho += int(o["att_rho"].sum())
                rej_gam += int(o["att_R"].sum())
                n0 += int((o["n_i"] == 0).sum())
                edge_rej += int(o["att_rho"][touched[b]].sum())
                assert all(gae.stationary(o["rho"][i])[0] for i in range(c["N"])), where
    print(f"rejected rho attempts {rej_rho} ({edge_rej} on chunk-edge series), rejected Gamma attempts {rej_gam}, "
          f"series without a usable row {n0}")
    assert rej_rho > 0 and rej_gam > 0 and n0 > 0 and edge_rej > 0


def test_max_n_is_the_collapse_limit():
    shapes = ((4, 1, 1), (2, 1, 3), (8, 2, 1), (5, 1, 2), (16, 2, 1), (9, 3, 1))
    assert [apg.max_n(r, p, q) for r, p, q in shapes] == [1024, 1024, 512, 512, 256, 256]
    assert ag.pad_r(27) == 32 and ag.pad_r(30) == 32 and ag.pad_r(15) == 16
    assert [apg.rb_series(r) for r in (1, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16]
