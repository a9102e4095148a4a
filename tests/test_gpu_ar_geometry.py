"""GPU tests of the AR-idiosyncratic smoother pass and ECM (dfm_ks_pass_ar_batch, dfm_em_ar_batch: csrc/mstep_ar.hip's mmw_vec_kernel,
ar_moments_kernel<R, Q1> and ar_solve_kernel<R, Q1>) across the launch geometry of the series step, against oracle/ar_oracle.py at the
bounds of tests/test_gpu_ar.py (pass: 1e-9) and tests/test_gpu_ar_em.py (ECM: path 1e-8, parameters 1e-7, factors 1e-8).

The cases are the enumerated table tests/ar_geometry.py CASES: each of the 38 template instances at least once, every series-group
width at the edges of its series block, the solve block at 64 / 65 series, the staged chunk at 128 / 129 periods and at three chunks,
every static deal of tiles to the four waves, a state wider than the moments' leading block, and the series the solve kernel must
leave as they are.  tests/test_ar_geometry_cpu.py checks that the table covers every class and that, on the oracle alone, every
watched series moves by more than 1000 times the bounds used here."""
import numpy as np
import pytest

from tests import ar_geometry as ag

pytestmark = pytest.mark.gpu
KEYS = ag.KEYS
PASS_TOL = 1e-9                      # tests/test_gpu_ar.py
PATH_RTOL = 1e-8                     # tests/test_gpu_ar_em.py
PARAM_TOL = 1e-7
F_TOL = 1e-8
DFM_E_DIMS = -1                      # include/dfm_hip.h


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


def _rel(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "the result is not finite"
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("row", ag.CASES, ids=[ag.case_id(row) for row in ag.CASES])
def test_ar_series_step_matches_the_oracle(ctx, row):
    import torch
    c = ag.case_dict(row)
    r = c["r"]
    e = ag.expected(row)
    panel, st = e["panel"], e["start"]
    dev = torch.device("cuda", ctx.device)
    t = lambda v: torch.from_numpy(np.array(v, order="C")).to(dev)    # (a copy: the expectation is read-only)
    f, P, ll = ctx.ks_pass_ar_batch(t(panel), *[t(st[k]) for k in KEYS])
    torch.cuda.synchronize()
    f, P, ll = f.cpu().numpy(), P.cpu().numpy(), ll.cpu().numpy()
    est, path, its, fe, _ = ctx.em_ar_batch_host(panel.copy(), *[st[k].copy() for k in KEYS], max_iter=ag.MAX_ITER)
    err = {}
    worst = lambda k, v: err.__setitem__(k, max(err.get(k, 0.0), v))
    for b in range(ag.B):
        ps, em = e["passes"][b], e["ems"][b]
        worst("pass loglik", abs(float(ll[b]) - ps["loglik"]) / max(1.0, abs(ps["loglik"])))
        worst("pass f", _rel(f[b], ps["f"]))
        worst("pass P", _rel(P[b], ps["P"]))
        worst("path", float(np.abs(path[b] / em["path"] - 1.0).max()))
        for k in KEYS:
            if em["est"][k].size:                                 # (rho at q = 0)
                worst(k, _rel(est[k][b], em["est"][k]))
        worst("em f", _rel(fe[b], em["f"]))
    print(f"\n  {ag.case_id(row)}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for b in range(ag.B):
        np.testing.assert_allclose(path[b], e["ems"][b]["path"], rtol=PATH_RTOL, err_msg=f"loglik path b={b}")
    for k in ("pass loglik", "pass f", "pass P"):
        assert err[k] <= PASS_TOL, (k, err[k])
    for k in KEYS:
        assert err.get(k, 0.0) <= PARAM_TOL, (k, err[k])
    assert err["em f"] <= F_TOL, err["em f"]
    assert np.all(its == ag.MAX_ITER)
    if c["edge"]:                                                 # fewer than r + q + 1 usable rows: the series is left as it is
        for i in (ag.EDGE_SHORT, ag.EDGE_EMPTY):
            for k in ("Lam", "rho", "sig2"):
                assert np.array_equal(est[k][:, i], st[k][:, i]), (k, i)
        assert not np.array_equal(est["Lam"][:, ag.EDGE_ENOUGH], st["Lam"][:, ag.EDGE_ENOUGH])


def test_refusals(ctx):
    """N beyond the collapse tiling of a state wider than 16, and T = q + 1 (one quasi-differenced row): DFM_E_DIMS, which
    include/dfm_hip.h numbers -1 (the -2 of tests/test_gpu_ar.py's dimension-limit test is DFM_E_R_UNSUPPORTED: r (q + 1) > 32)."""
    from dynamic_factor_models_amd._lib import DfmError
    from oracle import ar_oracle as ao
    for N, T, r, p, q in ((257, 40, 5, 1, 3), (20, 3, 2, 1, 2)):
        x, st = ao.synth_ar(0, N, max(T, 30), r, p, q)
        with pytest.raises(DfmError) as ei:
            ctx.em_ar_batch_host(x[None, :T], *[st[k][None] for k in KEYS], max_iter=2)
        assert ei.value.code == DFM_E_DIMS and "DFM_E_DIMS" in str(ei.value), (N, T, ei.value.code)
