"""The Python side of dfm_gibbs_batch[_dev] (dynamic_factor_models_amd/gibbs.py) without a GPU and without the library, in the
manner of tests/test_kalman_marshalling_cpu.py: both wrappers are driven against a recorder in place of the loaded library, and
the recorded call is held against _lib.SYMBOLS (argument count and kinds), the arrays passed and the documented return value.
Every dimension is distinct, so that a swapped argument shows."""
import ctypes

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, gibbs
from tests.test_kalman_marshalling_cpu import HANDLE, MISS, SING, addr, dev, make_ctx, val

B, T, N, r, p = 2, 12, 6, 3, 2
K_ = r * p
PRIOR = dict(tau_lam=1.5, nu_R=4, s_R=0.25, tau_A=2.5, nu_Q=r + 2, s_Q=0.75)       # (two integers: the wrapper makes them doubles)
STATE = ("Lam", "R", "Avar", "Q")
PER = dict(Lam=(N, r), R=(N,), A=(r, K_), Q=(r, r), f=(T, r))


def arrays(nan=True):
    g = np.random.default_rng(0)
    a = dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), R=g.random((B, N)) + 1,
             Avar=g.standard_normal((B, r, K_)), Q=g.standard_normal((B, r, r)), mu0=g.standard_normal((B, K_)),
             P0=g.standard_normal((B, K_, K_)), A0=g.standard_normal((B, r, K_)))
    if nan:
        a["panel"][1, 3, 2] = np.nan
    return a


def recorded(ctx, name):
    """The one recorded call, held against the prototype in _lib.SYMBOLS."""
    assert [c[0] for c in ctx._lib.calls] == [name]
    args = ctx._lib.calls.pop()[1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds) == 31
    for i, (x, kind) in enumerate(zip(args, kinds)):
        where = f"{name} argument {i}"
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int, where
        elif kind is ctypes.c_double:
            assert type(x) is float, where
        elif kind is ctypes.c_void_p:
            assert x is None or isinstance(x, ctypes.c_void_p), where
        else:
            assert kind in (ctypes.c_uint64, ctypes.c_int64) and type(x) is int, where
    return args


def call(ctx, host, a, prior, n_sweeps, **kw):
    conv = (lambda x: x) if host else dev
    t = {k: conv(v) for k, v in a.items()}
    pr = dict(prior)
    if pr.get("A0") is not None:
        pr["A0"] = t["A0"]
    fn = ctx.gibbs_batch_host if host else ctx.gibbs_batch
    state, draws = fn(t["panel"], t["Lam"], t["R"], t["Avar"], t["Q"], t["mu0"], t["P0"], pr, n_sweeps, **kw)
    return t, state, draws, recorded(ctx, "dfm_gibbs_batch" if host else "dfm_gibbs_batch_dev")


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("with_a0", [False, True])
def test_argument_order_types_and_state(host, with_a0):
    ctx, a = make_ctx(), arrays()
    prior = dict(PRIOR, A0=a["A0"] if with_a0 else None)
    keep = ("Lam", "R", "A", "Q", "f")
    t, state, draws, args = call(ctx, host, a, prior, 9, burn=2, thin=3, seed=(1 << 64) + 5, first_sweep=7, keep=keep)
    assert val(args[0]) == HANDLE and args[1:6] == (B, T, N, r, p)
    assert [val(x) for x in args[6:9]] == [addr(t["panel"]), addr(t["mu0"]), addr(t["P0"])]
    assert set(state) == set(STATE)
    for i, k in enumerate(STATE):                             # the state: in place on the device, copies on the host
        assert val(args[9 + i]) == addr(state[k])
        if host:
            assert state[k] is not a[k] and np.array_equal(state[k], a[k]) and addr(state[k]) != addr(a[k])
        else:
            assert state[k] is t[k]
    assert args[13:19] == (1.5, 4.0, 0.25, 2.5, float(r + 2), 0.75)
    assert val(args[19]) == (addr(t["A0"]) if with_a0 else None)
    assert args[20:25] == (9, 2, 3, 5, 7)                     # n_sweeps, burn, thin, seed mod 2^64, first_sweep
    K = 3                                                     # sweeps 2, 5, 8
    for i, k in enumerate(keep):
        assert type(draws[k]) is type(t["panel"]) and tuple(draws[k].shape) == (B, K) + PER[k] and str(draws[k].dtype).endswith("float64")
        assert val(args[25 + i]) == addr(draws[k])
    assert args[30] == MISS                                   # the panel was scanned: it has a NaN


@pytest.mark.parametrize("host", [False, True])
def test_keep_subsets_flags_and_no_kept_sweep(host):
    ctx, a = make_ctx(), arrays(nan=False)
    _, _, draws, args = call(ctx, host, a, PRIOR, 4, keep=("R", "f"), singular_q=True)
    assert [k for k in draws if draws[k] is not None] == ["R", "f"] and set(draws) == {"Lam", "R", "A", "Q", "f"}
    assert [val(x) for x in args[25:30]] == [None, addr(draws["R"]), None, None, addr(draws["f"])]
    assert args[30] == SING and args[20:25] == (4, 0, 1, 0, 0)
    _, _, draws, args = call(ctx, host, a, PRIOR, 4, may_have_missing=True)                  # the default keep: no f
    assert draws["f"] is None and all(tuple(draws[k].shape) == (B, 4) + PER[k] for k in ("Lam", "R", "A", "Q"))
    assert args[30] == MISS
    _, _, draws, args = call(ctx, host, a, PRIOR, 3, burn=3, keep=("Lam", "Q"))              # K = 0: nothing to point at
    assert tuple(draws["Lam"].shape) == (B, 0, N, r) and tuple(draws["Q"].shape) == (B, 0, r, r)
    assert [val(x) for x in args[25:30]] == [None] * 5
    _, _, draws, args = call(ctx, host, a, PRIOR, 5, keep=())
    assert all(v is None for v in draws.values()) and [val(x) for x in args[25:30]] == [None] * 5


def test_refusals_before_the_library_is_called():
    ctx, a = make_ctx(), arrays()
    for kw in (dict(n_sweeps=0), dict(n_sweeps=2, thin=0), dict(n_sweeps=2, burn=-1), dict(n_sweeps=2, keep=("Lam", "x"))):
        with pytest.raises(ValueError):
            ctx.gibbs_batch_host(*[a[k] for k in ("panel", "Lam", "R", "Avar", "Q", "mu0", "P0")], PRIOR, **kw)
    with pytest.raises(ValueError):                           # the device backend checks the shape of A0
        call(ctx, False, dict(a, A0=np.ascontiguousarray(a["A0"][:, :, :r])), dict(PRIOR, A0=a["A0"]), 2)
    assert ctx._lib.calls == []
    assert gibbs.kept(9, 2, 3) == 3 and gibbs.kept(3, 3, 1) == 0 and gibbs.kept(1, 0, 5) == 1
