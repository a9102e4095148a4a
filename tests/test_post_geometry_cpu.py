"""CPU checks of tests/post_geometry.py: the plain-Python restatement of the post-estimation kernels' launch geometry against the
numbers the sources state and against cell_geometry of csrc/dfm_cellgeom.h itself, compiled for the host
(tests/host/cellgeom_host.cpp), and the GPU case table (tests/test_gpu_post_geometry.py) against the coverage classes it must
hit for each kernel family."""
import itertools

import pytest

from tests import post_geometry as pg


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return pg.build_cellgeom_host(tmp_path_factory.mktemp("cellgeom"))


def _check_cells(host_exe, geos):
    """Every summary of `geos` against the host function at the summary's own call-site arguments, field for field."""
    calls = sorted({g["call"] for g in geos})
    host = dict(zip(calls, pg.ask_cellgeom_host(host_exe, [("cell",) + c for c in calls])))
    bad = [(g["kernel"], g["call"], host[g["call"]]) for g in geos if tuple(g[f] for f in pg.GEOM_FIELDS) != host[g["call"]]]
    assert not bad, bad[:5]
    return len(calls)


def test_case_table_geometries_match_the_host_function(host_exe):
    geos = [g for row in pg.CASES for fam in pg.geometries(pg.case_dict(row)).values() for g in fam]
    assert len(geos) == 5 * len(pg.CASES) and _check_cells(host_exe, geos) > len(pg.CASES)


@pytest.mark.parametrize("family", ["forecast", "simsmooth", "news"])
def test_geometry_sweep_matches_the_host_function(host_exe, family):
    """N = 1..1100 x r x rows at each family's own call-site arguments (lanes, staged doubles per row, thread and LDS caps)."""
    one = dict(forecast=lambda N, r, rows: pg.forecast_fill(1, N, r, rows, 0),
               simsmooth=lambda N, r, rows: pg.simsmooth_cells(1, 1, N, r, rows, 0, fill=True),
               news=lambda N, r, rows: pg.news_cells(1, 1, N, r, rows, impact=False))[family]
    geos = [one(N, r, rows) for N, r, rows in itertools.product(pg.SWEEP_N, pg.SWEEP_R, pg.SWEEP_ROWS)]
    n = _check_cells(host_exe, geos)
    # the sweep reaches both sides of every branch of the function
    assert n > 10000 and {1, 2, 3} <= {g["nsblk"] for g in geos} and {1, 2, 5, 64} <= {g["G"] for g in geos}
    assert any(g["cap_binds"] for g in geos) and any(g["RC"] == 8 * g["G"] for g in geos) and any(g["RC"] == g["rows"] for g in geos)
    assert any(g["partial_last"] for g in geos) and any(g["threads"] > g["G"] * g["NPB"] for g in geos)


def test_sp_rule_matches_cell_sp(host_exe):
    """forecast_fill's SP (the bucket is R = r itself) against cell_sp, the one rule every SP launcher calls."""
    assert pg.check_sp_rule(host_exe, lambda N, r, al: pg.forecast_fill(1, N, r, 40, 0, aligned=al)["SP"]) == {1, 2}


def test_forecast_fill_launch_matches_the_sources():
    # cell_geometry / DESIGN.md section 10: N = 200, SP = 2 gives 5 x 100 of 512; N = 139 gives 3 x 139 of 448
    g = pg.forecast_fill(1, 200, 8, 500, 0)
    assert (g["SP"], g["nsblk"], g["G"], g["NPB"], g["threads"]) == (2, 1, 5, 100, 512)
    g = pg.forecast_fill(1, 139, 8, 500, 0)
    assert (g["SP"], g["nsblk"], g["G"], g["NPB"], g["threads"]) == (1, 1, 3, 139, 448)
    # r = 32: (32 + 528) doubles per staged row, 48 KiB of LDS: at most 10 rows per workgroup
    g = pg.forecast_fill(1, 600, 32, 60, 4)
    assert (g["SP"], g["nsblk"], g["NPB"], g["G"], g["RC"], g["nchunk"]) == (1, 3, 200, 2, 10, 7)
    assert g["cap_binds"] and g["partial_last"] and not g["idle_last"]
    # single-series lanes above r = 16 and for odd N
    assert pg.forecast_fill(1, 200, 17, 50, 0)["SP"] == 1 and pg.forecast_fill(1, 201, 16, 50, 0)["SP"] == 1
    assert pg.forecast_fill(1, 200, 16, 50, 0)["SP"] == 2


def test_pair_geometry_matches_the_sources():
    # column pairs: N = 200 gives 5 x 100 of 512 in simsmooth.hip and in news.hip
    for g in (pg.simsmooth_cells(1, 1, 200, 8, 500, 0, fill=False), pg.news_cells(1, 1, 200, 8, 500, impact=False)):
        assert (g["nsblk"], g["G"], g["NPB"], g["threads"], g["RC"]) == (1, 5, 100, 512, 40)
    # N = 514: 257 pairs in 2 blocks of 129, the last lane of block 1 idle
    g = pg.simsmooth_cells(1, 1, 514, 8, 40, 0, fill=False)
    assert (g["nsblk"], g["NPB"]) == (2, 129) and g["idle_last"]
    # N = 1025: 513 pairs (column 1024 unpaired) in 3 blocks of 171; forecast: 5 blocks of 205 single series
    g = pg.news_cells(1, 1, 1025, 20, 28, impact=True)
    assert (g["nsblk"], g["NPB"], g["vec"]) == (3, 171, False) and not g["idle_last"]
    g = pg.forecast_fill(1, 1025, 8, 28, 5)
    assert (g["SP"], g["nsblk"], g["NPB"]) == (1, 5, 205)
    # N = 1026, r = 4: forecast pairs on the 16-byte path, 3 blocks of 171
    g = pg.forecast_fill(1, 1026, 4, 40, 3)
    assert (g["SP"], g["nsblk"], g["NPB"]) == (2, 3, 171)
    # the LDS cap (32 KiB / 8 r) binds only with small NPB and many rows: N = 14, r = 12, T = 400 gives NPB = 7, G = 64, cap 341
    g = pg.simsmooth_cells(1, 1, 14, 12, 400, 0, fill=False)
    assert (g["NPB"], g["G"], g["cap"], g["RC"], g["nchunk"]) == (7, 64, 341, 341, 2) and g["cap_binds"] and g["partial_last"]


def test_buckets_match_the_sources():
    assert [pg.rb_bucket(r) for r in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]
    assert [pg.news_gamma_kb(r, p) for r, p in ((8, 1), (2, 4), (9, 1), (4, 4), (1, 12), (17, 1), (6, 4), (8, 4))] == \
        [8, 8, 16, 16, 16, 32, 32, 32]


def test_news_targets_cover_the_edges():
    for row in pg.CASES:
        c = pg.case_dict(row)
        T, N, H = c["T"], c["N"], c["H"]
        tg = pg.targets(c)
        times = {t for t, _ in tg}
        cols = {i for _, i in tg}
        assert {0, 31, 32, T - 1, T, T + H - 1} <= times, c["name"]
        last = pg.news_cells(1, 1, N, c["r"], T, impact=True)
        assert {0, 1, N - 1, 2 * (last["nsblk"] - 1) * last["NPB"]} <= cols, c["name"]
        assert all(0 <= i < N for i in cols)


def test_case_table_covers_every_class():
    missing = pg.missing_classes()
    assert all(not v for v in missing.values()), f"coverage classes no case hits: {missing}"


@pytest.mark.parametrize("drop", ["n1025_r17", "n514_r8", "n52_r32_cap", "mixed"])
def test_dropping_a_case_is_noticed(drop):
    """The coverage check fails, naming the class, when the only case of a class leaves the table."""
    rest = [row for row in pg.CASES if row[0] != drop]
    missing = pg.missing_classes(rest)
    assert any(missing.values()), drop
