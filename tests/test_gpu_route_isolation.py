"""Route switches belong to the handle that was created under them: a handle's kernels depend on the environment at ITS
creation only, whatever handles the process creates (or destroys) afterwards.  Production switches only."""
import os

import numpy as np
import pytest

from oracle import kalman_oracle as ko

pytestmark = pytest.mark.gpu
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
SWITCHES = ("DFM_NO_CHUNK", "DFM_MSTEP_MISS")
B, N, T, R_ = 4, 200, 500, 8


def _ctx(**env):
    """A context created with exactly the switches of `env` set; the environment is put back before this returns."""
    import torch
    assert torch.cuda.is_available()
    from dynamic_factor_models_amd import DfmContext
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return DfmContext()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _problem():
    reps = [ko.synth_replicate(300 + b, N, T, R_, missing=0.10) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    return panel, {k: np.stack([p[k] for _, p in reps]) for k in KEYS}


def _pass(ctx, panel, st):
    import torch
    f, P, ll = ctx.ks_pass_batch(_dev(ctx, panel), *[_dev(ctx, st[k]) for k in KEYS])
    torch.cuda.synchronize()
    total = ctx.chunk_fallbacks()[1]
    return total, [t.cpu().numpy() for t in (f, P, ll)]


def test_chunk_switch_of_a_later_handle_leaves_an_earlier_handle_alone():
    panel, st = _problem()
    a = _ctx()
    try:
        total, first = _pass(a, panel, st)
        assert total == B                        # every replicate on the time-chunked recursion
        b = _ctx(DFM_NO_CHUNK=1)
        try:
            assert _pass(b, panel, st)[0] == 0   # ... and none under the switch
        finally:
            b.close()
        total, again = _pass(a, panel, st)
        assert total == B
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close()


def _em(ctx, panel, st):
    import torch
    dev = {k: _dev(ctx, st[k]) for k in KEYS}
    ctx.profile_enable(True)
    ctx.em_batch(_dev(ctx, panel), *[dev[k] for k in KEYS], max_iter=2, tol=0.0)
    torch.cuda.synchronize()
    kernels = [(name, launches) for name, (_, launches) in ctx.profile_read().items()]
    ctx.profile_enable(False)
    return kernels, {k: dev[k].cpu().numpy() for k in KEYS}


def test_loadings_switch_of_a_later_handle_leaves_an_earlier_handle_alone():
    panel, st = _problem()
    a = _ctx()
    try:
        kernels, first = _em(a, panel, st)
        b = _ctx(DFM_MSTEP_MISS=2)
        b.close()
        kernels_again, again = _em(a, panel, st)
        assert kernels_again == kernels
        for k in KEYS:
            assert first[k].tobytes() == again[k].tobytes(), k
    finally:
        a.close()
