"""GPU: the EM stop rule (csrc/dfm_em_epilogue.h: em_decide / em_record) at tol > 0 in every kernel that hosts it, each reached by
shape (tests/em_stop_cases.py names the route of every case).  The expectation needs no tol argument of any oracle: the family's oracle
runs once with tol = 0, and the iteration at which the relative improvement first falls below tol follows from its path."""
import numpy as np
import pytest

from tests import em_stop_cases as ec

pytestmark = pytest.mark.gpu
RTOL = 1e-8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


@pytest.mark.parametrize("name", list(ec.CASES))
def test_every_route_stops_each_replicate_where_the_oracle_path_says(ctx, name):
    c = ec.CASES[name]
    want = ec.expected(name)                                   # (asserts the case's preconditions on the oracle's path)
    orc = ec.oracle(name)
    got = ec.run(ctx, name, c["tol"])
    path, its = got["path"], got["iters"]
    # every replicate: a plausible count and a path that is NaN exactly past it
    assert np.all((its >= 2) & (its <= c["max_iter"])), (its.min(), its.max())
    col = np.arange(c["max_iter"])[None, :]
    assert np.array_equal(np.isnan(path), col >= its[:, None])
    for b in ec.compared(name):
        iters, msteps = want[b]
        opath, snaps = orc[b]
        print(name, "b", b, "iters", its[b], "expected", iters)
        assert its[b] == iters, (b, its[b], iters)
        np.testing.assert_allclose(path[b, :iters], opath[:iters], rtol=RTOL, err_msg=f"loglik path b={b}")
        assert np.all(np.isnan(path[b, iters:]))
        ref = snaps[msteps]
        for k in ec.keys(c):
            if ref[k].size == 0:                               # (rho at q = 0)
                continue
            err = np.abs(got[k][b] - ref[k]).max()
            assert err <= 1e-7 * max(1.0, np.abs(ref[k]).max()), (k, b, err)
