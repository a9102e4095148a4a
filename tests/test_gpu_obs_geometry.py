"""GPU tests of the EM with observed factors (dfm_em_obs_batch) across the launch geometry of its loadings step (csrc/mstep_obs.hip):
every instance of mstep_obs_kernel<RE> (RE = r_o + r_u = 2..8), one, exactly one, two and three series blocks of 256 threads, and the
wide route (obs_augment_kernel + obs_moments_kernel<16 | 32>) at RE = 9, 16 (no padding), 17 and 32, against oracle/obs_oracle.py at
the bounds of tests/test_gpu_round3.py::test_em_with_observed_factors_matches_the_oracle (path 1e-9, parameters / f / P 1e-8).

The cases are tests/obs_cases.py CASES; tests/test_ar_geometry_cpu.py checks that they cover every class.  With missing cells, one
series keeps r_o + r_u observed cells, one fewer than the joint regression needs, and must come back bit-equal."""
import numpy as np
import pytest

from tests import obs_cases as oc

pytestmark = pytest.mark.gpu
KEYS = oc.KEYS
PATH_RTOL = 1e-9
TOL = 1e-8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("row", oc.CASES, ids=[oc.case_id(row) for row in oc.CASES])
def test_em_with_observed_factors_across_the_geometry(ctx, row):
    c = oc.case_dict(row)
    e = oc.expected(row)
    panel, G, st = e["panel"], e["G"], e["start"]
    new, path, its, f, P = ctx.em_obs_batch_host(panel.copy(), G.copy(), *[st[k].copy() for k in KEYS], max_iter=oc.MAX_ITER, tol=0.0)
    err = {}
    worst = lambda k, v: err.__setitem__(k, max(err.get(k, 0.0), v))
    for b in range(oc.B):
        assert np.isfinite(path[b]).all() and all(np.isfinite(new[k][b]).all() for k in KEYS)
        worst("path", float(np.abs(path[b] / e["path"][b] - 1.0).max()))
        for k in KEYS:
            worst(k, float(np.abs(new[k][b] - e["est"][b][k]).max()) / max(1.0, float(np.abs(e["est"][b][k]).max())))
        worst("f", float(np.abs(f[b] - e["f"][b]).max()) / float(np.abs(e["f"][b]).max()))
        worst("P", float(np.abs(P[b] - e["P"][b]).max()) / float(np.abs(e["P"][b]).max()))
    print(f"\n  {oc.case_id(row)}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for b in range(oc.B):
        np.testing.assert_allclose(path[b], e["path"][b], rtol=PATH_RTOL, err_msg=f"loglik path b={b}")
    for k in KEYS + ("f", "P"):
        assert err[k] <= TOL, (k, err[k])
    assert np.all(its == oc.MAX_ITER)
    if c["missing"] > 0.0:                                        # r_o + r_u observed cells: the series keeps its parameters
        assert np.array_equal(new["Lam"][:, oc.BLANKED], st["Lam"][:, oc.BLANKED])
        assert np.array_equal(new["R"][:, oc.BLANKED], st["R"][:, oc.BLANKED])
