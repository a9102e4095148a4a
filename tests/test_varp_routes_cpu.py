"""CPU proof that the table of tests/varp_routes.py is good: (a) the restated dispatch gives every row the route class the table
claims and the table reaches every class; (b) the kernel names and constants of the restatement are the ones csrc/*.hip state;
(c) every row is conditioned well enough for the oracle's EM, and a second formulation of the log-likelihood (the textbook
n_t x n_t innovation form of tests/filter_expect.py, which shares nothing with the oracle's recursion) agrees with the oracle to
1e-11: the 1e-9 of the GPU test cannot hide a wrong kernel behind the oracle's own rounding."""
import os

import numpy as np
import pytest

from tests import filter_expect as fe
from tests import varp_routes as vr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamic_factor_models_amd", "csrc")
ALL = [(row.name, v) for row in vr.ROWS + vr.ROWS_DIAG_ONLY for v in vr.VARIANTS]


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


# ------------------------------------------------------------------------------------------------ (a) classes reached
def test_every_row_reaches_the_class_it_claims(capsys):
    with capsys.disabled():
        print()
        for row in vr.ROWS:
            rt = vr.route(row.r, row.p, row.singular, True, vr.n_periods(row), vr.batch(row))
            got = vr.row_classes(row)
            print(f"  {row.name:12s} N = {vr.n_series(row, 'balanced'):2d} | {vr.n_series(row, 'missing'):2d}  T = {vr.n_periods(row):3d}  "
                  f"{rt.instance:38s} Rp {rt.Rp:2d} Rc {rt.Rc:2d} rl {rt.rl:2d}  {sorted(got)}")
            assert row.cls in got, (row.name, row.cls, got)
    assert not vr.missing_classes(), vr.missing_classes()
    assert not vr.missing_diag_classes(), vr.missing_diag_classes()
    for names in vr.DIAG_ROWS.values():
        assert all(n in vr.BY_NAME for n in names)
    # one row of every required class in the shorter lists (want_P=False, host entries); the batch and LDS edges have their own tests
    seen = set().union(*[vr.row_classes(vr.BY_NAME[n]) for n in vr.ONE_PER_CLASS])
    assert vr.REQUIRED - seen <= {"wave<8> CH8=4", "wave<32> lds<=64K", "wave<32> lds>64K"}


@pytest.mark.parametrize("name", ["r1p2", "r4p1", "r8p1", "r16p1", "r4p8", "r32p1", "r4p4-sing", "r4p5-sing", vr.BATCH_EDGE, "r8p4-T752",
                                  "r8p4-T753", "r4p4", "r2p6"])
def test_dropping_a_row_is_noticed(name, monkeypatch):
    """These rows are the only ones of their class, or share it with one other row: without the class's rows it is reported."""
    cls = vr.BY_NAME[name].cls
    monkeypatch.setattr(vr, "ROWS", [row for row in vr.ROWS if row.cls != cls])
    assert cls in vr.missing_classes()


def test_dispatch_restatement():
    kern = lambda *a, **k: vr.route(*a, **k).instance
    # the shapes tests/test_gpu_varp.py runs, as its comments name their kernels
    assert kern(2, 2) == "recursion_kernel<4, true>" and kern(1, 4) == "recursion_kernel<4, true>"
    assert kern(1, 5) == kern(4, 2) == "recursion_wave_kernel<8, true, 8>"
    assert kern(2, 6) == kern(1, 16) == "recursion_mbf16_kernel<2>" and kern(3, 4) == kern(4, 3, True) == "recursion_mbf16_kernel<4>"
    assert kern(4, 3) == kern(4, 4) == "recursion_comp_kernel<1, true>" and kern(4, 8) == "recursion_comp_kernel<2, true>"
    assert kern(8, 4) == "recursion_wave_kernel<32, true, 8>"
    assert kern(2, 3, B=1025) == "recursion_wave_kernel<8, true, 4>" and kern(2, 3, B=1024) == "recursion_wave_kernel<8, true, 8>"
    assert kern(2, 3, B=1025, num_cu=304) == "recursion_wave_kernel<8, true, 8>" and kern(3, 3, B=1100) == "recursion_mbf16_kernel<4>"
    # r = 4: the state must be whole blocks of 4 (always so) and Q regular; r = 3 shares Rc = 4 but not rl = 4
    assert kern(3, 8) == "recursion_wave_kernel<32, true, 8>" and kern(4, 5, True) == "recursion_wave_kernel<32, true, 8>"
    # the handles without the wave kernels
    assert [vr.route(r, p, wave=False).instance for r, p in ((5, 2), (4, 4), (2, 6), (8, 4), (4, 5))] == \
        ["recursion_kernel<16, true>"] * 3 + ["recursion_kernel<32, true>"] * 2
    # the LDS cap: passed at T > 22768 (Rp = 32) and T > 34416 (Rp = 16)
    assert vr.wave_lds_bytes(32, 0) == 62528 and vr.wave_lds_bytes(16, 0) == 15936 and vr.wave_lds_bytes(8, 0) == 2560
    assert vr.route(8, 4, T=22768).kernel == vr.K_WAVE and vr.route(8, 4, T=22769).instance == "recursion_kernel<32, true>"
    assert vr.route(5, 2, T=34416).kernel == vr.K_WAVE and vr.route(5, 2, T=34417).instance == "recursion_kernel<16, true>"
    assert vr.route(4, 8, T=10 ** 6).kernel == vr.K_COMP             # (comp and mbf16 have no dynamic LDS)
    with pytest.raises(AssertionError):
        vr.route(11, 3)


def test_lds_edge():
    assert vr.wave_lds_bytes(32, 752) == 65536 == vr.LDS_OPT_IN
    assert vr.wave_lds_bytes(32, 753) > 65536
    assert vr.n_periods(vr.BY_NAME["r8p4-T752"]) == 752 and vr.n_periods(vr.BY_NAME["r8p4-T753"]) == 753
    assert vr.n_series(vr.BY_NAME["r8p4-T752"], "missing") == 16


def test_shapes_stay_small():
    for row in vr.ROWS + vr.ROWS_DIAG_ONLY:
        for v in vr.VARIANTS:
            N, T = vr.n_series(row, v), vr.n_periods(row)
            assert N <= 65 and (N % 2 == (1 if v == "missing" else 0) or row.N is not None)
            assert T <= 141 or row.name.startswith("r8p4-T")
            assert N >= 2 * row.r or row.N is not None              # the PCA start has room for r factors
    assert vr.batch(vr.BY_NAME[vr.BATCH_EDGE]) == 1025 and vr.n_distinct(vr.BY_NAME[vr.BATCH_EDGE]) == 3


# ------------------------------------------------------------------------------------------------ (b) strings pinned
def test_strings_and_constants_are_the_sources():
    rec, wave, comp, mbf, grid, capi = (_src(f) for f in ("recursion.hip", "recursion_wave.hip", "recursion_comp.hip",
                                                           "recursion_mbf16.hip", "dfm_grid.h", "capi.hip"))
    assert f'note_kernel("{vr.K_WAVE}")' in wave and f'note_kernel("{vr.K_COMP}")' in comp and f'note_kernel("{vr.K_MBF16}")' in mbf
    assert f'"collapse_kernel", "{vr.K_LANE}"' in capi               # kKernelNames[K_RECURSION]: the launch's name when no launcher notes one
    assert "note_kernel" not in rec.split("static hipError_t launch_rec(")[1].split("hipError_t launch_recursion(")[0]
    # the order launch_recursion asks in
    order = [rec.index(s) for s in ("recursion_comp_supported(Rpad, a)", "recursion_mbf16_supported(Rpad, a)",
                                    "recursion_tile_supported(Rpad, a)", "recursion_wave_supported(Rpad, a)",
                                    "case 32: return launch_rec<32, true>(a, s);")]
    assert order == sorted(order)
    # the wave kernels' LDS
    assert "constexpr int kTileStride = R + 2;" in grid and "constexpr int kGridProw = 2 * (4 * R + 4);" in grid
    assert "constexpr size_t RT = (size_t)R * kTileStride<R>;" in wave
    assert "const size_t extra = R >= 16 ? (kGridProw<R> + 2 * (R * R / 64) * R + 2 * RT) : 0;" in wave
    assert "return (4 * RT + extra) * sizeof(double) + (size_t)T * sizeof(int);" in wave
    assert "constexpr size_t cap = 150 * 1024;" in wave and vr.LDS_CAP == 150 * 1024
    assert "if (Rpad == 16) return wave_lds_bytes<16>(a.T) <= cap;" in wave and "if (Rpad == 32) return wave_lds_bytes<32>(a.T) <= cap;" in wave
    assert "return Rpad == 8 && wave_lds_bytes<8>(a.T) <= 60 * 1024;" in wave and vr.LDS_WAVE8 == 60 * 1024
    assert "if (!attr_done && lds > 64 * 1024) {" in wave and vr.LDS_OPT_IN == 64 * 1024
    assert "if (a.B > simds) return launch_wave_cov_ch<R, COV, 4>(a, s);" in wave and "return pr.multiProcessorCount * 4;" in wave
    assert "if (a.Rc == 0 && a.B > bmax) return false;" in wave
    # comp and mbf16
    assert "if (off || (Rpad != 16 && Rpad != 32) || !a.cov || a.kdim < 8 || a.kdim > Rpad || (a.kdim & 3) != 0) return false;" in comp
    assert "const bool var = a.Rc == 4 && a.rl == 4 && a.kb == 0;" in comp and "if (a.qsing) return false;" in comp
    assert "if (off || Rpad != 16 || !a.cov || a.kb != 0) return false;" in mbf
    assert "if (a.Rc != 2 && a.Rc != 4) return false;" in mbf and "if (a.rl < 1 || a.rl > a.Rc) return false;" in mbf
    assert "if (a.Rc == 4) hipLaunchKernelGGL(recursion_mbf16_kernel<4>" in mbf
    # the plan of varp_run
    assert "comp.Rc = pad_r(r); comp.rl = r; comp.kdim = k;" in capi
    assert "make_plan(h->opt, B, T, N, k, flags | DFM_F_SINGULAR_Q, em, false, comp);" in capi
    assert "int pad_r(int r) { return pow2_ge(r) < 2 ? 2 : pow2_ge(r); }" in capi
    assert 'if (k > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");' in capi
    # the switches: one belongs to the handle, two to the process
    assert 'o.no_rec_wave = on(diag_env("DFM_NO_RECURSION_WAVE"));' in capi and "ra.wave = h->opt.no_rec_wave ? 0 : 1;" in capi
    assert 'static const bool off = [] { const char* v = diag_env("DFM_NO_COMP");' in comp
    assert 'static const bool off = [] { const char* v = diag_env("DFM_NO_MBF16");' in mbf


# ------------------------------------------------------------------------------------------------ (c) conditioning
def _min_eig_q(Q, singular):
    w = np.linalg.eigvalsh(Q)
    return w[1] if singular else w[0]                               # (rank r - 1 by construction, and the EM keeps the null direction)


@pytest.mark.parametrize("name,variant", ALL)
def test_rows_are_well_conditioned(name, variant):
    row = vr.BY_NAME[name]
    x, q = vr.inputs(name, variant)
    assert x.shape == (vr.n_distinct(row), vr.n_periods(row), vr.n_series(row, variant))
    if variant == "missing":
        assert np.isnan(x[:, [0, 5, -1], :]).all()
        assert 0.08 < np.isnan(np.delete(x, [0, 5, x.shape[1] - 1], axis=1)).mean() < 0.22
    else:
        assert not np.isnan(x).any()
    for b, (ref, em) in enumerate(zip(vr.pass_reference(name, variant), vr.em_reference(name, variant))):
        assert _min_eig_q(q["Q"][b], row.singular) >= 1e-4, ("Q at the start", np.linalg.eigvalsh(q["Q"][b]))
        assert _min_eig_q(em["Q"], row.singular) >= 1e-4, ("Q after the EM", np.linalg.eigvalsh(em["Q"]))
        if row.singular:
            assert abs(np.linalg.eigvalsh(q["Q"][b])[0]) <= 1e-12 * np.linalg.eigvalsh(q["Q"][b])[-1]
        assert em["R"].min() >= 1e-4 and q["R"][b].min() >= 1e-4
        path = em["path"]
        assert len(path) == vr.EM_ITERS and np.isfinite(path).all()
        assert (np.diff(path) >= -1e-7 * abs(path[0])).all(), path
        assert path[0] == ref["loglik"]
        assert em["Avar"].shape == (row.r, row.r * row.p) and em["Q"].shape == (row.r, row.r)
        assert em["P_smooth"].shape == (x.shape[1], row.r * (row.r + 1) // 2)


@pytest.mark.parametrize("name,variant", ALL)
def test_second_formulation_of_the_loglikelihood(name, variant):
    x, _ = vr.inputs(name, variant)
    for b, ref in enumerate(vr.pass_reference(name, variant)):
        s = vr.start(name, variant, b)
        ll = fe.textbook_filter(x[b], s["Lam"], s["R"], s["Avar"], s["Q"], s["mu0"], s["P0"])[4].sum()
        assert abs(ll - ref["loglik"]) <= 1e-11 * abs(ref["loglik"]), (ll, ref["loglik"])
