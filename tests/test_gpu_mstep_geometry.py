"""GPU tests of the balanced EM's loadings step across its launch geometry (csrc/mstep_mfma.hip: the 64 instances of
mstep_mfma_kernel<R, STEPS, NDR> with the transition M-step in its front workgroups, mstep_finish_kernel; csrc/mstep_wide.hip: every
instance of mstep_wide_kernel and mstep_finish_wide_kernel), against oracle/kalman_oracle.py's EM from the same start, at the bounds
of tests/test_gpu_em.py: the likelihood path at rtol 1e-8, every parameter, f and P at 1e-8 max(1, scale), the path not decreasing.

The cases are the enumerated tables of tests/mstep_geometry.py: one case per mstep_mfma instance, walking the clamped last step, the
mask of the last 1-KB piece, 1 .. 8 segments per replicate with trailing segments of 0, 1 .. 7, 8, 9 .. 11 and more rows, front
workgroups with clamped waves; the wide step at every instance, block edge and stage count; and four cases where replicates stop at
different iterations on these routes.  tests/test_mstep_geometry_cpu.py checks that the tables cover every class, that every case
takes the route it claims, that the oracle is insensitive to the start and that every watched series moves by more than 1000 times
the bound."""
import numpy as np
import pytest

from tests import mstep_geometry as mg

pytestmark = pytest.mark.gpu
KEYS = mg.KEYS
RTOL = 1e-8                          # tests/test_gpu_em.py
STOP_PARAM_TOL = 1e-7                # tests/test_gpu_em.py::test_em_tolerance_stops_each_replicate_like_the_oracle
SOLO_RTOL = 1e-11
TWO_ITER = mg.MFMA_CASES + mg.MFMA_EXTRA + mg.WIDE_CASES


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


def _em(ctx, panel, start, max_iter, tol):
    """ctx.em_batch on copies of the (read-only) expectation's arrays: parameters, path, iters, f, P as numpy."""
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda v: torch.from_numpy(np.array(v, order="C")).to(dev)
    par = {k: t(start[k]) for k in KEYS}
    path, its, f, P = ctx.em_batch(t(panel), *[par[k] for k in KEYS], max_iter=max_iter, tol=tol, may_have_missing=False)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in par.items()}, path.cpu().numpy(), its.cpu().numpy(), f.cpu().numpy(), P.cpu().numpy()


def _err(got, ref, scale=None):
    """max |got - ref| / max(1, scale), scale = max |ref| unless given"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "the result is not finite"
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()) if scale is None else scale)


@pytest.mark.parametrize("row", TWO_ITER, ids=[mg.case_id(row) for row in TWO_ITER])
def test_loadings_step_matches_the_oracle(ctx, row):
    B = row[0]
    e = mg.expected(row)
    est, path, its, f, P = _em(ctx, e["panel"], e["start"], mg.MAX_ITER, 0.0)
    err = {}
    worst = lambda k, v: err.__setitem__(k, max(err.get(k, 0.0), v))
    for b in range(B):
        ref = e["ems"][b]
        worst("path", float(np.abs(path[b] / ref["path"] - 1.0).max()))
        for k in KEYS:
            worst(k, _err(est[k][b], ref["est"][k]))
        worst("f", _err(f[b], ref["f"]))
        worst("P", _err(P[b], ref["P"], ref["Pscale"]))
    print(f"\n  {mg.route(row[1], row[3])} {mg.case_id(row)}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.all(its == mg.MAX_ITER)
    for b in range(B):
        np.testing.assert_allclose(path[b], e["ems"][b]["path"], rtol=RTOL, err_msg=f"loglik path b={b}")
        assert np.all(np.diff(path[b]) > -1e-9 * np.abs(path[b][:-1])), "EM log-likelihood must not decrease"
    for k in KEYS + ("f", "P"):
        assert err[k] <= RTOL, (k, err[k])


@pytest.mark.parametrize("row", mg.STOP_CASES, ids=[mg.case_id(row) for row in mg.STOP_CASES])
def test_replicates_stop_separately_on_the_streaming_routes(ctx, row):
    """A replicate that stops keeps the parameters of its own last iteration while its neighbours (in the same front workgroup, the
    same streaming workgroups and finish grid) go on; run alone, it takes the same path."""
    B, N, T, r, tol, max_iter, _ = row
    e = mg.expected_stop(row)
    est, path, its, f, P = _em(ctx, e["panel"], e["start"], max_iter, tol)
    want = [len(em["path"]) for em in e["ems"]]
    err = {}
    worst = lambda k, v: err.__setitem__(k, max(err.get(k, 0.0), v))
    for b in range(B):
        n = min(int(its[b]), want[b])
        worst("path", float(np.abs(path[b, :n] / e["ems"][b]["path"][:n] - 1.0).max()))
        for k in KEYS:
            worst(k, _err(est[k][b], e["ems"][b]["est"][k]))
    print(f"\n  {mg.case_id(row)}: iters {its.tolist()} (oracle {want})  " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert its.tolist() == want
    for b in range(B):
        np.testing.assert_allclose(path[b, :its[b]], e["ems"][b]["path"], rtol=RTOL, err_msg=f"loglik path b={b}")
        assert np.all(np.isnan(path[b, its[b]:])), b
    for k in KEYS:
        assert err[k] <= STOP_PARAM_TOL, (k, err[k])
    b = int(np.argmin(its))                                         # the replicate that stopped first, alone
    est1, path1, its1, _, _ = _em(ctx, e["panel"][b:b + 1], {k: e["start"][k][b:b + 1] for k in KEYS}, max_iter, tol)
    assert its1[0] == its[b]
    np.testing.assert_allclose(path1[0, :its[b]], path[b, :its[b]], rtol=SOLO_RTOL)
    assert np.all(np.isnan(path1[0, its[b]:]))


@pytest.mark.parametrize("row", [mg.MFMA_CASES[0], mg.WIDE_CASES[0]], ids=["mstep_mfma", "mstep_wide"])
def test_the_dispatcher_takes_the_restated_route(ctx, row):
    """The profile names the loadings step of the route tests/mstep_geometry.py's rule gives, and not mstep_lam_kernel."""
    e = mg.expected(row)
    ctx.profile_enable(True)
    try:
        _em(ctx, e["panel"], e["start"], mg.MAX_ITER, 0.0)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    name = mg.PROFILE_NAME[mg.route(row[1], row[3])]
    assert name in prof and prof[name][1] >= 1, sorted(prof)
    assert mg.PROFILE_NAME["mstep_lam"] not in prof, sorted(prof)
