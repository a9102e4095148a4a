"""GPU tests of the mixed-frequency EM's series step across its launch geometry (csrc/mstep_mf.hip: mf_loadings_kernel,
mf_table_kernel, mf_moments_kernel<2|3|4>, mf_solve_kernel<1..8>; csrc/mstep_mf_blocks.hip: mf_solve_blocks_kernel; the class and tile
dealing of capi.hip), against the NumPy model tests/mf_expect.py from the same start, two iterations, at the bounds of
tests/test_gpu_mf.py: the likelihood path at rtol 1e-8, every parameter at 1e-7 max(1, scale), f at 1e-8 max(1, scale), P at
relative 1e-8.  A series that must be kept (n_i < r + 1, or a G_i that is not positive definite: the all-zero class) is compared
with the start bit for bit.

The cases are the table of tests/mf_geometry.py: every instance r = 1 .. 8 of the solve and TT = 2, 3, 4 of the moments kernel,
L = 1 .. 5, C = 1, 2, 3 and 8 classes, class sizes 1, 15, 16, 17, 32 and 33, ntiles mod 4 = 1, 2, 3, 0, a workgroup of four classes, a
second workgroup with waves past ntiles, series 0 with NaN under another class's padding lanes, T = 7, 13, 16, 17, 18, 31, 32, 33,
N = 256 and 257, B = 1, 3, 5, n_i = 0, r and r + 1; three of them again under the fixed-loadings solve; three cases where replicates
stop at different iterations.  tests/test_mf_geometry_cpu.py checks that the table covers every class, that every watched series
moves by more than 1000 times the bound, that three wrong kernels would be noticed and that the model's own noise is a hundredth
of every bound."""
import numpy as np
import pytest

from tests import mf_geometry as mg

pytestmark = pytest.mark.gpu
KEYS = mg.KEYS
PATH_RTOL, PARAM_TOL, F_TOL, P_RTOL = 1e-8, 1e-7, 1e-8, 1e-8      # tests/test_gpu_mf.py
SOLO_RTOL = 1e-11                    # tests/test_gpu_mstep_geometry.py
IDS = [c["name"] for c in mg.CASES]
PROFILE = {"table": "mf_table_kernel", "moments": "mf_moments_kernel", "solve": "mf_solve_kernel", "blocks": "mf_solve_blocks_kernel"}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


def _run(ctx, e, max_iter, tol=0.0, free=None, rows=slice(None)):
    """The host-pointer entry on copies of the (read-only) expectation's arrays."""
    st = {k: np.array(e["start"][k][rows], order="C") for k in KEYS}
    x, W = np.array(e["panel"][rows], order="C"), np.array(e["W"], order="C")
    if free is None:
        return ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=max_iter, tol=tol)
    return ctx.em_mf_blocks_batch_host(x, st["Lam"], st["R"], W, np.array(free), st["Avar"], st["Q"], st["mu0"], st["P0"],
                                       max_iter=max_iter, tol=tol)


def _scaled(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "the result is not finite"
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _compare(label, e, est, path, its, f, P, B):
    """Every replicate against its expectation: prints the worst error per quantity, then asserts the bounds."""
    err = {}
    worst = lambda k, v: err.__setitem__(k, max(err.get(k, 0.0), v))
    for b in range(B):
        ref = e["ems"][b]
        worst("path", float(np.abs(path[b] / ref["path"] - 1.0).max()))
        for k in KEYS:
            worst(k, _scaled(est[k][b], ref["est"][k]))
        worst("f", _scaled(f[b], ref["f"]))
        assert np.isfinite(P[b]).all()
        worst("P", float(np.abs(P[b] - ref["P"]).max() / np.abs(ref["P"]).max()))
    print(f"\n  {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.all(its == mg.MAX_ITER)
    for b in range(B):
        np.testing.assert_allclose(path[b], e["ems"][b]["path"], rtol=PATH_RTOL, err_msg=f"loglik path b={b}")
    for k in KEYS:
        assert err[k] <= PARAM_TOL, (k, err[k])
    assert err["f"] <= F_TOL and err["P"] <= P_RTOL, err


@pytest.mark.parametrize("name", IDS)
def test_series_step_matches_the_model(ctx, name):
    case = mg.BY_NAME[name]
    e = mg.expected(name)
    est, path, its, f, P = _run(ctx, e, mg.MAX_ITER)
    _compare(name, e, est, path, its, f, P, case["B"])
    kept = mg.kept_series(name)
    assert np.array_equal(est["Lam"][:, kept], e["start"]["Lam"][:, kept]) and np.array_equal(est["R"][:, kept], e["start"]["R"][:, kept])
    moved = np.setdiff1d(np.arange(e["W"].shape[0]), kept)
    assert np.all(est["R"][:, moved] != e["start"]["R"][:, moved]) and np.all(np.any(est["Lam"][:, moved] != e["start"]["Lam"][:, moved], axis=2))


@pytest.mark.parametrize("name", mg.BLOCKS_CASES)
def test_blocks_solve_meets_the_same_tile_edges(ctx, name):
    """The N = 257, C = 8 and ntiles >= 5 cases through dfm_em_mf_blocks_batch under mf_blocks_expect.case_mask, against
    mf_blocks_expect.em_mf_blocks; the profile names the blocks solve and not the unrestricted one."""
    case = mg.BY_NAME[name]
    e = mg.expected_blocks(name)
    ctx.profile_enable(True)
    try:
        est, path, its, f, P = _run(ctx, e, mg.MAX_ITER, free=e["free"])
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    _compare(name + " (blocks)", e, est, path, its, f, P, case["B"])
    assert np.array_equal(est["Lam"][:, ~e["free"]], e["start"]["Lam"][:, ~e["free"]])
    for k in ("table", "moments", "blocks"):
        assert PROFILE[k] in prof and prof[PROFILE[k]][1] >= 1, sorted(prof)
    assert PROFILE["solve"] not in prof, sorted(prof)


def test_the_three_kernels_of_the_step_run(ctx):
    e = mg.expected(mg.PROFILE_CASE)
    ctx.profile_enable(True)
    try:
        _run(ctx, e, mg.MAX_ITER)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    for k in ("table", "moments", "solve"):
        assert PROFILE[k] in prof and prof[PROFILE[k]][1] >= 1, sorted(prof)
    assert PROFILE["blocks"] not in prof, sorted(prof)


@pytest.mark.parametrize("k", range(len(mg.STOP_CASES)), ids=[row[0]["name"] for row in mg.STOP_CASES])
def test_replicates_stop_separately(ctx, k):
    """A replicate that stops keeps the parameters of its own last iteration while its neighbours -- in the same grids of the
    table, moments and solve kernels -- go on; run alone, the first stopper takes the same path."""
    case, tol, max_iter, _ = mg.STOP_CASES[k]
    B = case["B"]
    e = mg.expected_stop(k)
    est, path, its, _, _ = _run(ctx, e, max_iter, tol=tol)
    want = [len(em["path"]) for em in e["ems"]]
    err = {}
    worst = lambda key, v: err.__setitem__(key, max(err.get(key, 0.0), v))
    for b in range(B):
        n = min(int(its[b]), want[b])
        worst("path", float(np.abs(path[b, :n] / e["ems"][b]["path"][:n] - 1.0).max()))
        for key in KEYS:
            worst(key, _scaled(est[key][b], e["ems"][b]["est"][key]))
    print(f"\n  {case['name']}: iters {its.tolist()} (model {want})  " + "  ".join(f"{key} {v:.2e}" for key, v in err.items()))
    assert its.tolist() == want
    for b in range(B):
        np.testing.assert_allclose(path[b, :its[b]], e["ems"][b]["path"], rtol=PATH_RTOL, err_msg=f"loglik path b={b}")
        assert np.all(np.isnan(path[b, its[b]:])), b
    for key in KEYS:
        assert err[key] <= PARAM_TOL, (key, err[key])
    b = int(np.argmin(its))                                         # the replicate that stopped first, alone
    assert b == (0 if k < 2 else B - 1)
    _, path1, its1, _, _ = _run(ctx, e, max_iter, tol=tol, rows=slice(b, b + 1))
    assert its1[0] == its[b]
    np.testing.assert_allclose(path1[0, :its[b]], path[b, :its[b]], rtol=SOLO_RTOL)
    assert np.all(np.isnan(path1[0, its[b]:]))
