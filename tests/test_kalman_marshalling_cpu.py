"""The Python side of the C boundary (dynamic_factor_models_amd/kalman.py) without a GPU and without the library: every
wrapper that binds a dfm_* symbol is driven against a recorder in place of the loaded library, and the recorded call is held
against _lib.SYMBOLS (argument count and kinds), the arrays passed (dimensions, pointers) and the documented return value.

The shapes are the smallest that keep every dimension distinct, so that a swapped argument shows."""
import contextlib
import ctypes
import types

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, kalman
from tests.api_calls import Recorder

B, T, N, r, p, q, L = 2, 12, 6, 2, 2, 1, 3
D, H, G = 2, 1, 1
MISS, SING = _lib.DFM_F_MAY_HAVE_MISSING, _lib.DFM_F_SINGULAR_Q
HANDLE = 0xD0F0


class _OnDevice(torch.Tensor):
    is_cuda = True          # the one answer of DfmContext._dev that a machine without a GPU cannot give


class _NoScan(torch.Tensor):
    """A panel that may not be searched for NaN."""
    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        assert func not in (torch.isnan, torch.Tensor.isnan), "the panel was scanned"
        return super().__torch_function__(func, types, args, kwargs or {})


def make_ctx(mod=kalman):
    """A DfmContext that never saw a device: the recorder for the library, and _dev = the real checks on CPU tensors."""
    ctx = mod.DfmContext.__new__(mod.DfmContext)
    ctx._lib, ctx._h, ctx._torch, ctx._use_torch_stream, ctx.device = Recorder(), ctypes.c_void_p(HANDLE), torch, False, 0
    ctx._dev = lambda t, name, shape=None: mod.DfmContext._dev(ctx, t.as_subclass(_OnDevice), name, shape)
    return ctx


def arrays(qq=q, pp=p, nan=True, seed=0):
    """NumPy inputs of every family, by name."""
    g = np.random.default_rng(seed)
    m_ar, m_mf = max(pp, qq + 1), max(pp, L)
    a = dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), R=g.random((B, N)) + 1,
             A=g.standard_normal((B, r, r)), Q=g.standard_normal((B, r, r)), mu0=g.standard_normal((B, r)),
             P0=g.standard_normal((B, r, r)), Avar=g.standard_normal((B, r, r * pp)), mu0p=g.standard_normal((B, r * pp)),
             P0p=g.standard_normal((B, r * pp, r * pp)), sig2=g.random((B, N)) + 1, rho=g.standard_normal((B, N, qq)),
             mu0ar=g.standard_normal((B, r * m_ar)), P0ar=g.standard_normal((B, r * m_ar, r * m_ar)),
             W=g.random((N, L)), mu0mf=g.standard_normal((B, r * m_mf)), P0mf=g.standard_normal((B, r * m_mf, r * m_mf)),
             mean=g.standard_normal((B, N)), sd=g.random((B, N)) + 1)
    if nan:
        a["panel"][1, 3, 2] = np.nan
    a["old"] = a["panel"].copy()
    a["old"][0, T - 1, 1] = np.nan
    return a


FAMILY = {"": ("panel", "Lam", "R", "A", "Q", "mu0", "P0"),
          "_varp": ("panel", "Lam", "R", "Avar", "Q", "mu0p", "P0p"),
          "_ar": ("panel", "Lam", "sig2", "rho", "Avar", "Q", "mu0ar", "P0ar"),
          "_mf": ("panel", "Lam", "R", "W", "Avar", "Q", "mu0mf", "P0mf")}
EXTRA = {"": (), "_varp": (p,), "_ar": (p, q), "_mf": (p, L)}
ROWS = {"": T, "_varp": T, "_ar": T - q, "_mf": T}
NPK = r * (r + 1) // 2


def dev(a):
    return None if a is None else torch.from_numpy(a)


def addr(a):
    """Where an array's data is (None: no array; a zero-size array has no data to point at)."""
    if a is None or (a.numel() if isinstance(a, torch.Tensor) else a.size) == 0:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def val(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


REACHED = set()


def one_call(lib, name, count=1):
    """The `count` recorded calls are all to `name`; each is held against the prototype in _lib.SYMBOLS.  Returns the last."""
    assert [c[0] for c in lib.calls] == [name] * count
    REACHED.add(name)
    for _, args in lib.calls:
        kinds = _lib.SYMBOLS[name][1]
        assert len(args) == len(kinds)
        for i, (x, kind) in enumerate(zip(args, kinds)):
            where = f"{name} argument {i}"
            if kind in (ctypes.c_int, ctypes.c_uint):
                assert type(x) is int, where
            elif kind is ctypes.c_double:
                assert type(x) is float, where
            elif kind is ctypes.c_void_p:
                assert x is None or isinstance(x, ctypes.c_void_p), where
            elif kind in (ctypes.c_uint64, ctypes.c_int64, ctypes.c_longlong, ctypes.c_size_t):
                assert type(x) is int or isinstance(x, kind), where
            else:                                       # typed pointers and string buffers: byref(...) / a ctypes array
                assert not isinstance(x, (int, float, np.ndarray, torch.Tensor)), where
    args = lib.calls[-1][1]
    lib.calls.clear()
    return args


def check_head(args, fam, a, extra=None, handle=HANDLE):
    """handle (None: some other leading argument), B, T, N, r, the family's extra integers, then the panel's and the
    parameters' pointers; returns the next index."""
    lead = 1
    if handle is not None:
        assert val(args[0]) == handle
    dims = (B, T, N, r) + (EXTRA[fam] if extra is None else extra)
    assert args[lead:lead + len(dims)] == dims
    i = lead + len(dims)
    for k, name in enumerate(FAMILY[fam]):
        assert val(args[i + k]) == addr(a[name]), name
    return i + len(FAMILY[fam])


def shaped(x, shape, like, dtype="float64"):
    """x is an array of the kind of `like` (tensor / ndarray) with that shape and dtype."""
    assert type(x) is type(like) and tuple(x.shape) == tuple(shape) and str(x.dtype).endswith(dtype)
    return x


MISSING = [(None, MISS), (False, 0), (True, MISS)]


# ------------------------------------------------------------------------------------------ _dev and the helpers
def test_dev_checks_type_contiguity_and_shape():
    ctx = make_ctx()
    good = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(TypeError, match="^Lam: expected a contiguous float64 tensor on the HIP device$"):
        ctx._dev(good.float(), "Lam")
    with pytest.raises(TypeError, match="^Lam: expected a contiguous float64 tensor on the HIP device$"):
        ctx._dev(good.t(), "Lam")
    with pytest.raises(ValueError, match=r"^Lam: shape \(2, 3\) != expected \(3, 2\)$"):
        ctx._dev(good, "Lam", (3, 2))
    with pytest.raises(TypeError):
        kalman.DfmContext._dev(ctx, good, "Lam")            # a CPU tensor is not on the device
    assert ctx._dev(good, "Lam", (2, 3)).value == good.data_ptr()


# ------------------------------------------------------------------------------------------ smoother pass
@pytest.mark.parametrize("fam", ["", "_varp", "_ar", "_mf"])
@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_pass_device(fam, mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    t = {k: dev(v) for k, v in a.items()}
    for want_P in (True, False):
        f, P, ll = getattr(ctx, f"ks_pass{fam}_batch")(*[t[k] for k in FAMILY[fam]], want_P=want_P, may_have_missing=mhm,
                                                       singular_q=sq)
        args = one_call(ctx._lib, f"dfm_ks_pass{fam}_batch_dev")
        i = check_head(args, fam, t)
        shaped(f, (B, ROWS[fam], r), t["panel"]), shaped(ll, (B,), t["panel"])
        assert P is None if not want_P else shaped(P, (B, ROWS[fam], NPK), t["panel"]) is P
        assert [val(x) for x in args[i:]] == [addr(f), addr(P), addr(ll), bit | (SING if sq else 0)]


@pytest.mark.parametrize("fam", ["", "_varp", "_ar", "_mf"])
@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_pass_host(fam, mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    f, P, ll = getattr(ctx, f"ks_pass{fam}_batch_host")(*[a[k] for k in FAMILY[fam]], may_have_missing=mhm, singular_q=sq)
    args = one_call(ctx._lib, f"dfm_ks_pass{fam}_batch")
    i = check_head(args, fam, a)                            # C-ordered float64 inputs are passed where they lie
    shaped(f, (B, ROWS[fam], r), a["panel"]), shaped(P, (B, ROWS[fam], NPK), a["panel"]), shaped(ll, (B,), a["panel"])
    assert [val(x) for x in args[i:]] == [addr(f), addr(P), addr(ll), bit | (SING if sq else 0)]


def test_plain_host_pass_alone_takes_want_P():
    ctx, a = make_ctx(), arrays()
    f, P, ll = ctx.ks_pass_batch_host(*[a[k] for k in FAMILY[""]], want_P=False)
    args = one_call(ctx._lib, "dfm_ks_pass_batch")
    assert P is None and args[13] is None and val(args[12]) == addr(f) and args[15] == MISS


def test_pass_out_is_written_and_returned():
    ctx, a = make_ctx(), arrays()
    t = {k: dev(v) for k, v in a.items()}
    out = (torch.empty(B, T, r, dtype=torch.float64), torch.empty(B, T, NPK, dtype=torch.float64),
           torch.empty(B, dtype=torch.float64))
    got = ctx.ks_pass_batch(*[t[k] for k in FAMILY[""]], may_have_missing=False, out=out)
    args = one_call(ctx._lib, "dfm_ks_pass_batch_dev")
    assert all(g is o for g, o in zip(got, out))
    assert [val(x) for x in args[12:]] == [addr(out[0]), addr(out[1]), addr(out[2]), 0]


def test_host_inputs_are_converted_not_trusted():
    ctx, a = make_ctx(), arrays()
    lam32 = a["Lam"].astype(np.float32)
    ctx.ks_pass_batch_host(a["panel"].tolist(), lam32, np.asfortranarray(a["R"]), a["A"], a["Q"], a["mu0"], a["P0"])
    args = one_call(ctx._lib, "dfm_ks_pass_batch")
    assert args[1:5] == (B, T, N, r) and val(args[6]) != addr(lam32) and args[15] == MISS


# ------------------------------------------------------------------------------------------ EM
@pytest.mark.parametrize("fam", ["", "_varp", "_ar", "_mf"])
@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_em_device(fam, mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    t = {k: dev(v) for k, v in a.items()}
    for want_smooth, want_P in ((True, True), (True, False), (False, True)):
        path, iters, f, P = getattr(ctx, f"em{fam}_batch")(*[t[k] for k in FAMILY[fam]], max_iter=5, tol=1, want_smooth=want_smooth,
                                                           want_P=want_P, may_have_missing=mhm, singular_q=sq)
        args = one_call(ctx._lib, f"dfm_em{fam}_batch_dev")
        i = check_head(args, fam, t)                        # the caller's tensors themselves: updated in place
        shaped(path, (B, 5), t["panel"]), shaped(iters, (B,), t["panel"], "int32")
        assert f is None if not want_smooth else shaped(f, (B, ROWS[fam], r), t["panel"]) is f
        assert P is None if not (want_smooth and want_P) else shaped(P, (B, ROWS[fam], NPK), t["panel"]) is P
        assert [val(x) for x in args[i:]] == [5, 1.0, addr(path), addr(iters), addr(f), addr(P), bit | (SING if sq else 0)]


@pytest.mark.parametrize("fam", ["", "_varp", "_ar", "_mf"])
@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_em_host(fam, mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    before = {k: v.copy() for k, v in a.items()}
    prm, path, iters, f, P = getattr(ctx, f"em{fam}_batch_host")(*[a[k] for k in FAMILY[fam]], max_iter=5, tol=1,
                                                                 may_have_missing=mhm, singular_q=sq)
    args = one_call(ctx._lib, f"dfm_em{fam}_batch")
    names = FAMILY[fam][1:]
    public = [n.rstrip("parmf") if n.startswith(("mu0", "P0")) else n for n in names]      # mu0p -> mu0, P0ar -> P0
    assert list(prm) == [n for n in public if n != "W"]
    passed = dict(a, **{n: prm[k] for n, k in zip(names, public) if k in prm})               # copies go, not the inputs
    i = check_head(args, fam, passed)
    for n, k in zip(names, public):
        assert np.array_equal(a[n], before[n], equal_nan=True)
        if k in prm:
            assert prm[k] is not a[n] and not np.shares_memory(prm[k], a[n]) and np.array_equal(prm[k], a[n])
    assert np.array_equal(a["panel"], before["panel"], equal_nan=True)
    shaped(path, (B, 5), a["panel"]), shaped(iters, (B,), a["panel"], "int32")
    shaped(f, (B, ROWS[fam], r), a["panel"]), shaped(P, (B, ROWS[fam], NPK), a["panel"])
    assert [val(x) for x in args[i:]] == [5, 1.0, addr(path), addr(iters), addr(f), addr(P), bit | (SING if sq else 0)]


def test_ar_without_lags_passes_null_rho():
    ctx, a = make_ctx(), arrays(qq=0)
    t = {k: dev(v) for k, v in a.items()}
    rho_at = 1 + 6 + 3                                       # handle, B T N r p q, panel Lam sig2
    for call, sym, src in ((ctx.ks_pass_ar_batch, "dfm_ks_pass_ar_batch_dev", t), (ctx.em_ar_batch, "dfm_em_ar_batch_dev", t),
                           (ctx.ks_pass_ar_batch_host, "dfm_ks_pass_ar_batch", a), (ctx.em_ar_batch_host, "dfm_em_ar_batch", a)):
        out = call(*[src[k] for k in FAMILY["_ar"]])
        args = one_call(ctx._lib, sym)
        assert args[1:7] == (B, T, N, r, p, 0) and args[rho_at] is None and args[rho_at - 1] is not None
        f = out[0] if "ks_pass" in sym else out[-2]
        assert tuple(f.shape) == (B, T, r)


def test_em_step_and_iterate():
    ctx, a = make_ctx(), arrays()
    t = {k: dev(v) for k, v in a.items()}
    prm = [t[k] for k in FAMILY[""]]
    for mhm, bit in MISSING:
        ll = ctx.em_step_batch(*prm, may_have_missing=mhm)
        args = one_call(ctx._lib, "dfm_em_step_batch_dev")
        i = check_head(args, "", t)
        assert [val(x) for x in args[i:]] == [addr(shaped(ll, (B,), t["panel"])), bit]
    path, iters, active = torch.empty(B, 5, dtype=torch.float64), torch.empty(B, dtype=torch.int32), torch.empty(B, dtype=torch.int32)
    f, P = torch.empty(B, T, r, dtype=torch.float64), torch.empty(B, T, NPK, dtype=torch.float64)
    with pytest.raises(AssertionError, match="the panel was scanned"):
        ctx.em_step_batch(prm[0].as_subclass(_NoScan), *prm[1:])
    assert ctx.em_iterate_batch(prm[0].as_subclass(_NoScan), *prm[1:], 3, 5, 1, path, iters, active) is None     # default False
    args = one_call(ctx._lib, "dfm_em_iterate_batch_dev")
    i = check_head(args, "", t)
    assert [val(x) for x in args[i:]] == [3, 5, 1.0, addr(path), addr(iters), addr(active), None, None, 0]
    ctx.em_iterate_batch(*prm, 0, 5, 0.5, path, iters, active, f=f, P=P, may_have_missing=None, singular_q=True)
    args = one_call(ctx._lib, "dfm_em_iterate_batch_dev")
    assert [val(x) for x in args[12:]] == [0, 5, 0.5, addr(path), addr(iters), addr(active), addr(f), addr(P), MISS | SING]
    with pytest.raises(ValueError, match=r"^loglik_path: shape \(2, 5\) != expected \(2, 4\)$"):
        ctx.em_iterate_batch(*prm, 0, 4, 0.5, path, iters, active)
    assert ctx._lib.calls == []


@pytest.mark.parametrize("mhm,bit", MISSING)
def test_em_obs_host_never_sets_singular_q(mhm, bit):
    ctx, a = make_ctx(), arrays()
    Gobs, Lam = np.ones((B, T, 3)), np.ones((B, N, 3 + r))
    prm, path, iters, f, P = ctx.em_obs_batch_host(a["panel"], Gobs, Lam, a["R"], a["A"], a["Q"], a["mu0"], a["P0"], max_iter=4,
                                                   may_have_missing=mhm)
    args = one_call(ctx._lib, "dfm_em_obs_batch")
    assert (val(args[0]),) + args[1:6] == (HANDLE, B, T, N, r, 3)
    assert [val(x) for x in args[6:]] == [addr(a["panel"]), addr(Gobs)] + [addr(prm[k]) for k in ("Lam", "R", "A", "Q", "mu0", "P0")] \
        + [4, 0.0, addr(path), addr(iters), addr(f), addr(P), bit]
    assert prm["Lam"] is not Lam and np.array_equal(prm["Lam"], Lam) and f.shape == (B, T, r) and P.shape == (B, T, NPK)
    assert path.shape == (B, 4) and iters.dtype == np.int32
    with pytest.raises(ValueError, match="^em_obs_batch_host: G must be"):
        ctx.em_obs_batch_host(a["panel"], Gobs[:, :-1], Lam, a["R"], a["A"], a["Q"], a["mu0"], a["P0"])
    assert ctx._lib.calls == []


# ------------------------------------------------------------------------------------------ several GPUs from one process
def test_multi_host_statics(monkeypatch):
    lib, a = Recorder(), arrays()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    prm = [a[k] for k in FAMILY[""]]
    for mhm, bit in MISSING:
        for sq in (False, True):
            got, path, iters, f, P, ran = kalman.DfmContext.em_batch_multi_host(2, *prm, max_iter=3, tol=2, may_have_missing=mhm,
                                                                                device_ids=[1, 0], singular_q=sq)
            args = one_call(lib, "dfm_em_batch_multi")
            assert args[0] == 2 and np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_int32)), (2,)), [1, 0])
            passed = dict(a, **got)
            i = check_head(args[1:], "", passed, handle=None) + 1
            assert [val(x) for x in args[i:i + 7]] == [3, 2.0, addr(path), addr(iters), addr(f), addr(P), bit | (SING if sq else 0)]
            assert args[-1] == 700 and ran == 0 and list(got) == list(FAMILY[""][1:])
            assert all(got[k] is not a[k] and np.array_equal(got[k], a[k]) for k in got)
            assert (path.shape, iters.dtype, f.shape, P.shape) == ((B, 3), np.int32, (B, T, r), (B, T, NPK))
        f, P, ll = kalman.DfmContext.ks_pass_batch_multi_host(1, *prm, may_have_missing=mhm)     # no singular_q to pass
        args = one_call(lib, "dfm_ks_pass_batch_multi")
        assert args[0] == 1 and args[1] is None
        i = check_head(args[1:], "", a, handle=None) + 1
        assert [val(x) for x in args[i:i + 4]] == [addr(f), addr(P), addr(ll), bit] and args[-1] == 700
        assert (f.shape, P.shape, ll.shape) == ((B, T, r), (B, T, NPK), (B,))


def test_multi_object(monkeypatch):
    lib, a = Recorder(), arrays()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    m = kalman.DfmMulti(2, device_ids=[1, 0], force_comm=True)
    args = one_call(lib, "dfm_multi_create")
    assert args[1] == 2 and args[3] == _lib.DFM_MULTI_F_FORCE_COMM and args[5] == 700
    m._m = ctypes.c_void_p(HANDLE)
    m.load(*[a[k] for k in FAMILY[""]])
    check_head(one_call(lib, "dfm_multi_load"), "", a)
    assert m.shape == (B, T, N, r)
    m.synth(7, 3, B, T, N, r, missing_prob=0.25, pca_start=True)
    assert one_call(lib, "dfm_multi_synth")[1:] == (7, 3, B, T, N, r, 0.25, 1)
    for mhm, sq in ((False, False), (True, False), (False, True), (True, True)):
        flags = (MISS if mhm else 0) | (SING if sq else 0)
        m.ks_pass(want_P=False, may_have_missing=mhm, singular_q=sq)
        assert one_call(lib, "dfm_multi_ks_pass")[1:] == (0, flags)
        assert m.em(max_iter=6, tol=1, want_P=False, may_have_missing=mhm, singular_q=sq) == 0
        assert one_call(lib, "dfm_multi_em")[1:6] == (6, 1.0, 1, 0, flags)
    for what, shape, dt in (("P_smooth", (B, T, NPK), np.float64), ("loglik_path", (B, 6), np.float64), ("iters", (B,), np.int32)):
        got = m.fetch(what)
        args = one_call(lib, "dfm_multi_fetch")
        assert (got.shape, got.dtype) == (shape, dt) and val(args[2]) == addr(got)
    assert m.ngpu == 0
    one_call(lib, "dfm_multi_ngpu")
    assert m.has_comm is False
    one_call(lib, "dfm_multi_has_comm")
    lib.dfm_multi_ks_pass = lambda *args: -7                # a failure reads the object's message
    lib.dfm_multi_last_error = lambda m: b"no peer"
    with pytest.raises(_lib.DfmError, match="DFM_E_COMM: no peer"):
        m.ks_pass()
    REACHED.add("dfm_multi_last_error")
    m.close()
    one_call(lib, "dfm_multi_destroy")
    assert m._m is None


# ------------------------------------------------------------------------------------------ forecast, path draws, news
POST = ("Lam", "R", "Avar", "Q", "mu0p", "P0p")


def both(ctx, name, a):
    """(method, symbol, inputs) of the device and of the host form of an entry."""
    t = {k: dev(v) for k, v in a.items()}
    return ((getattr(ctx, name), f"dfm_{name}_dev", t), (getattr(ctx, name + "_host"), f"dfm_{name}", a))


@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_forecast(mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    for call, sym, s in both(ctx, "forecast_batch", a):
        for scaled, want in ((True, True), (False, False)):
            got = call(s["panel"], *[s[k] for k in POST], H, mean=s["mean"] if scaled else None, sd=s["sd"] if scaled else None,
                       want_var=want, want_common=want, want_P=want, may_have_missing=mhm, singular_q=sq)
            args = one_call(ctx._lib, sym)
            i = check_head(args, "_varp", s, extra=(p, H))
            assert list(got) == ["xhat", "xvar", "common", "f", "P", "loglik"]
            for k, shape in (("xhat", (B, T + H, N)), ("f", (B, T + H, r)), ("loglik", (B,))):
                shaped(got[k], shape, s["panel"])
            for k, shape in (("xvar", (B, T + H, N)), ("common", (B, T + H, N)), ("P", (B, T + H, NPK))):
                assert got[k] is None if not want else shaped(got[k], shape, s["panel"]) is got[k]
            assert [val(x) for x in args[i:]] == [addr(s["mean"]) if scaled else None, addr(s["sd"]) if scaled else None] \
                + [addr(got[k]) for k in got] + [bit | (SING if sq else 0)]


@pytest.mark.parametrize("mhm,bit", MISSING)
@pytest.mark.parametrize("sq", [False, True])
def test_simsmooth(mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    for call, sym, s in both(ctx, "simsmooth_batch", a):
        for scaled, want_x in ((True, True), (False, False)):
            got = call(s["panel"], *[s[k] for k in POST], D, H=H, seed=-1, first_draw=5, mean=s["mean"] if scaled else None,
                       sd=s["sd"] if scaled else None, want_x=want_x, may_have_missing=mhm, singular_q=sq)
            args = one_call(ctx._lib, sym)
            assert val(args[0]) == HANDLE and args[1:8] == (B, D, T, N, r, p, H)
            for k, name in enumerate(("panel",) + POST):
                assert val(args[8 + k]) == addr(s[name])
            assert list(got) == ["f", "x"] and shaped(got["f"], (B, D, T + H, r), s["panel"]) is got["f"]
            assert got["x"] is None if not want_x else shaped(got["x"], (B, D, T + H, N), s["panel"]) is got["x"]
            assert [val(x) for x in args[15:]] == [addr(s["mean"]) if scaled else None, addr(s["sd"]) if scaled else None,
                                                   0xFFFFFFFFFFFFFFFF, 5, addr(got["f"]), addr(got["x"]), bit | (SING if sq else 0)]


@pytest.mark.parametrize("mhm", [None, False, True])
@pytest.mark.parametrize("sq", [False, True])
def test_news_scans_the_new_vintage(mhm, sq):
    for nan_in_new in (True, False):
        ctx, a = make_ctx(), arrays(nan=nan_in_new)                     # `old` always holds a NaN
        bit = MISS if (nan_in_new if mhm is None else mhm) else 0
        for call, sym, s in both(ctx, "news_batch", a):
            for scaled, want in ((True, True), (False, False)):
                got = call(s["old"], s["panel"], *[s[k] for k in POST], [(T, 4)], mean=s["mean"] if scaled else None,
                           sd=s["sd"] if scaled else None, want_news=want, want_weight=want, may_have_missing=mhm, singular_q=sq)
                args = one_call(ctx._lib, sym)
                assert val(args[0]) == HANDLE and args[1:6] == (B, T, N, r, p)
                for k, name in enumerate(("old", "panel") + POST):
                    assert val(args[6 + k]) == addr(s[name])
                assert list(got) == ["yhat", "impact", "news", "weight"]
                shaped(got["yhat"], (B, 3, G), s["panel"]), shaped(got["impact"], (B, G, N), s["panel"])
                assert got["news"] is None if not want else shaped(got["news"], (B, T, N), s["panel"]) is got["news"]
                assert got["weight"] is None if not want else shaped(got["weight"], (B, G, T, N), s["panel"]) is got["weight"]
                tgt = [ctypes.cast(x, ctypes.POINTER(ctypes.c_int32))[0] for x in args[17:19]]      # host arrays on both paths
                assert [val(x) for x in args[14:17]] == [addr(s["mean"]) if scaled else None, addr(s["sd"]) if scaled else None, G]
                assert tgt == [T, 4]
                assert [val(x) for x in args[19:]] == [addr(got[k]) for k in got] + [bit | (SING if sq else 0)]


def test_value_errors_come_before_any_call():
    ctx, a = make_ctx(), arrays()
    for dev_or_host in (0, 1):
        fc, ss, nw = (both(ctx, n, a)[dev_or_host] for n in ("forecast_batch", "simsmooth_batch", "news_batch"))
        s = fc[2]
        prm = [s[k] for k in POST]
        bad = [(lambda: fc[0](s["panel"], *prm, H, mean=s["mean"]), "^mean and sd go together$"),
               (lambda: fc[0](s["panel"], *prm, -1), "^H must be >= 0$"),
               (lambda: ss[0](s["panel"], *prm, D, sd=s["sd"]), "^mean and sd go together$"),
               (lambda: ss[0](s["panel"], *prm, D, H=-1), "^H must be >= 0$"),
               (lambda: ss[0](s["panel"], *prm, 0), "^D must be >= 1$"),
               (lambda: nw[0](s["old"], s["panel"], *prm, [(T, 4)], mean=s["mean"]), "^mean and sd go together$"),
               (lambda: nw[0](s["old"][:, 1:], s["panel"], *prm, [(T, 4)]), "^old and new must have the same shape$"),
               (lambda: nw[0](s["old"], s["panel"], *prm, []), "^at least one target is needed$"),
               (lambda: nw[0](s["old"], s["panel"], *prm, [(T, N)]), "^targets are "),
               (lambda: nw[0](s["old"], s["panel"], *prm, [(-1, 0)]), "^targets are ")]
        for call, text in bad:
            with pytest.raises(ValueError, match=text):
                call()
            assert ctx._lib.calls == []


def test_device_path_names_the_array_whose_shape_is_wrong():
    ctx, a = make_ctx(), arrays()
    t = {k: dev(v) for k, v in a.items()}
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    cases = [(ctx.ks_pass_batch, "", "mu0", t["mu0p"], f"mu0: shape {(B, r * p)} != expected {(B, r)}"),
             (ctx.em_varp_batch, "_varp", "P0p", t["P0"], f"P0: shape {(B, r, r)} != expected {(B, r * p, r * p)}"),
             (ctx.ks_pass_ar_batch, "_ar", "rho", z(B, N + 1, q), f"rho: shape {(B, N + 1, q)} != expected {(B, N, q)}"),
             (ctx.em_mf_batch, "_mf", "W", z(N + 1, L), f"W: shape {(N + 1, L)} != expected {(N, L)}"),
             (ctx.em_ar_batch, "_ar", "Avar", z(B, r + 1, r * p), f"Avar: shape {(B, r + 1, r * p)} != expected {(B, r, r * p)}"),
             (ctx.em_step_batch, "", "Lam", z(B, N + 1, r), f"Lam: shape {(B, N + 1, r)} != expected {(B, N, r)}")]
    for call, fam, slot, wrong, text in cases:
        with pytest.raises(ValueError) as e:
            call(*[wrong if k == slot else t[k] for k in FAMILY[fam]])
        assert str(e.value) == text and ctx._lib.calls == []
    with pytest.raises(ValueError) as e:
        ctx.forecast_batch(t["panel"], *[t[k] for k in POST], H, mean=t["mean"][:1], sd=t["sd"])
    assert str(e.value) == f"mean: shape {(1, N)} != expected {(B, N)}" and ctx._lib.calls == []
    with pytest.raises(TypeError, match="^sig2: expected a contiguous float64 tensor on the HIP device$"):
        ctx.ks_pass_ar_batch(*[t[k].float() if k == "sig2" else t[k] for k in FAMILY["_ar"]])
    assert ctx._lib.calls == []


# ------------------------------------------------------------------------------------------ the single-copy wrappers
def test_pca_and_standardize():
    ctx, a = make_ctx(), arrays()
    panel = dev(a["panel"])
    for want in (True, False):
        out = ctx.pca_init_batch(panel, r, want_factors=want)
        args = one_call(ctx._lib, "dfm_pca_init_batch_dev")
        assert (val(args[0]),) + args[1:5] == (HANDLE, B, T, N, r)
        assert [val(x) for x in args[5:]] == [addr(panel)] + [addr(x) for x in out]
        for x, shape in zip(out, ((B, N, r), (B, N), (B, r, r), (B, r, r), (B, r), (B, r, r))):
            shaped(x, shape, panel)
        assert out[6] is None if not want else shaped(out[6], (B, T, r), panel) is out[6]
        mu, sd = ctx.standardize_batch(panel, want_stats=want)
        args = one_call(ctx._lib, "dfm_standardize_batch_dev")
        assert args[1:4] == (B, T, N) and [val(x) for x in args[4:]] == [addr(panel), addr(mu), addr(sd)]
        assert (mu is None and sd is None) if not want else (shaped(mu, (B, N), panel) is mu and shaped(sd, (B, N), panel) is sd)
    prm, F = ctx.pca_init_batch_host(a["panel"], r)
    args = one_call(ctx._lib, "dfm_pca_init_batch")
    assert args[1:5] == (B, T, N, r) and list(prm) == ["Lam", "R", "A", "Q", "mu0", "P0"]
    assert [val(x) for x in args[5:]] == [addr(a["panel"])] + [addr(prm[k]) for k in prm] + [addr(F)] and F.shape == (B, T, r)


def test_als_and_ols_host():
    ctx, g = make_ctx(), np.random.default_rng(1)
    z, F0 = g.standard_normal((T, N)), g.standard_normal((B, T, r))
    got = ctx.als_batch_host(z, F0, r_each=[1, 2], nt_min=3, max_iter=10 ** 12, tol=1e-3, path_cap=4, want_R2=True)
    args = one_call(ctx._lib, "dfm_als_batch")
    assert args[1:5] == (B, T, N, r) and val(args[5]) == addr(z) and args[6] == 0 and args[10:13] == (3, 2 ** 31 - 1, 1e-3)
    assert got["F"] is not F0 and np.array_equal(got["F"], F0) and args[14] == 4
    assert [val(args[i]) for i in (8, 9, 13, 15, 16, 17)] == [addr(got[k]) for k in ("F", "Lam", "ssr_path", "iters", "ssr", "R2")]
    assert (got["Lam"].shape, got["ssr_path"].shape, got["R2"].shape, got["iters"].dtype) == ((B, N, r), (B, 4), (B, N), np.int32)
    got = ctx.als_batch_host(np.stack([z, z]), F0)
    args = one_call(ctx._lib, "dfm_als_batch")
    assert args[6] == T * N and args[7] is None and args[13] is None and args[17] is None and got["ssr_path"] is None and got["R2"] is None
    with pytest.raises(ValueError, match="^z and F0 disagree on B or T$"):
        ctx.als_batch_host(z[1:], F0)
    with pytest.raises(ValueError, match="^r_each must hold B values"):
        ctx.als_batch_host(z, F0, r_each=[1, 3])
    X, Y = g.standard_normal((T, 3)), g.standard_normal((T, N))
    got = ctx.ols_batch_host(X, Y, nt_min=2)
    args = one_call(ctx._lib, "dfm_ols_batch")
    assert args[1:4] == (N, T, 3) and val(args[4]) == addr(X) and args[5] == 0 and val(args[6]) == addr(Y) and args[7:10] == (1, N, 2)
    assert (got["beta"].shape, got["resid"].shape, got["nobs"].dtype) == ((N, 3), (T, N), np.int32) and args[11] is not None
    assert [val(args[i]) for i in (10, 12, 13, 14)] == [addr(got[k]) for k in ("beta", "ssr", "tss", "nobs")]
    got = ctx.ols_batch_host(np.stack([X] * N), Y, want_resid=False)
    args = one_call(ctx._lib, "dfm_ols_batch")
    assert args[5] == T * 3 and args[11] is None and got["resid"] is None
    with pytest.raises(ValueError, match="^X and Y disagree on T or P$"):
        ctx.ols_batch_host(X[1:], Y)
    assert ctx._lib.calls == []


def test_bootstrap_quantiles_chow():
    ctx, g = make_ctx(), np.random.default_rng(2)
    ns, pl, Hh, nd = 3, 2, 4, 5
    y, beta, resid = g.standard_normal((T, ns)), g.standard_normal((1 + ns * pl, ns)), g.standard_normal((T, ns))
    signs = np.ones((nd, T))
    irf, bo = ctx.var_bootstrap_irf_host(y, beta, resid, pl, Hh, nd, signs=signs, seed=9, want_beta=True, first_draw=2)
    args = one_call(ctx._lib, "dfm_var_bootstrap_irf")
    assert args[1:6] == (nd, T, ns, pl, Hh) and [val(args[i]) for i in (6, 7, 9)] == [addr(y), addr(beta), addr(signs)]
    assert (type(args[10]), args[10].value, type(args[11]), args[11].value) == (ctypes.c_uint64, 9, ctypes.c_int64, 2)
    assert [val(args[12]), val(args[13])] == [addr(bo), addr(irf)] and (irf.shape, bo.shape) == ((nd, ns, Hh, ns), (nd, 1 + ns * pl, ns))
    irf = ctx.var_bootstrap_irf_host(y, beta, resid, pl, Hh, nd)
    args = one_call(ctx._lib, "dfm_var_bootstrap_irf")
    assert args[9] is None and args[12] is None and val(args[13]) == addr(irf)
    with pytest.raises(ValueError, match="^signs must be"):
        ctx.var_bootstrap_irf_host(y, beta, resid, pl, Hh, nd, signs=signs[1:])
    x, qs = g.standard_normal((nd, 2, 3)), np.array([0.1, 0.9])
    bands = ctx.quantile_bands_host(x, qs)
    args = one_call(ctx._lib, "dfm_quantile_bands")
    assert args[1:4] == (nd, 6, 2) and [val(args[4]), val(args[5])] == [addr(x), addr(qs)] and bands.shape == (2, 2, 3)
    assert val(args[6]) == addr(bands.base if bands.base is not None else bands)
    out = ctx.chow_batch_host([np.ones(5), np.ones(7)], [np.ones((5, 2)), np.ones((7, 2))], [0, 1, 1], [2, 3, 4], [1, 1, 2])
    args = one_call(ctx._lib, "dfm_chow_batch")
    assert args[1:4] == (2, 7, 2) and args[7] == 3 and val(args[11]) == addr(out) and out.shape == (3,)
    assert ctx._lib.calls == []


def test_handle_services():
    ctx = make_ctx()
    ctx.synchronize()
    one_call(ctx._lib, "dfm_synchronize")
    assert ctx.chunk_fallbacks() == (0, 0)
    one_call(ctx._lib, "dfm_chunk_fallbacks")
    ctx.profile_enable(False)
    assert one_call(ctx._lib, "dfm_profile_enable")[1] == 0
    assert ctx.profile_read() == {}
    assert one_call(ctx._lib, "dfm_profile_read", count=2)[1:4:2] == (1, 64)
    ctx._torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda d: None, device=lambda d: contextlib.nullcontext()))
    assert ctx.hbm_probe(1 << 20, iters=2) == {"read_dma": 0.0, "copy": 0.0, "write": 0.0}
    assert one_call(ctx._lib, "dfm_hbm_probe", count=3)[1:4] == (1 << 20, 2, 2)
    ctx._torch = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda d: types.SimpleNamespace(cuda_stream=0xAB)))
    ctx._use_torch_stream = True
    ctx._sync_stream()
    assert val(one_call(ctx._lib, "dfm_set_stream")[1]) == 0xAB
    ctx._lib.dfm_synchronize = lambda h: -4                  # a failure reads the handle's message
    ctx._lib.dfm_last_error = lambda h: b"NaN in a balanced panel"
    with pytest.raises(_lib.DfmError, match="DFM_E_MISSING: NaN in a balanced panel"):
        lib, real = ctx._lib, _lib.load
        _lib.load = lambda: lib
        try:
            ctx.synchronize()
        finally:
            _lib.load = real
    REACHED.add("dfm_last_error")


# every symbol kalman.py names, but dfm_synth_panels_dev (asks torch for a cuda device), dfm_create and dfm_destroy
EXPECTED = {f"dfm_{kind}{fam}_batch{sfx}" for kind in ("ks_pass", "em") for fam in FAMILY for sfx in ("", "_dev")} | {
    "dfm_em_step_batch_dev", "dfm_em_iterate_batch_dev", "dfm_em_obs_batch", "dfm_em_batch_multi", "dfm_ks_pass_batch_multi",
    "dfm_forecast_batch", "dfm_forecast_batch_dev", "dfm_simsmooth_batch", "dfm_simsmooth_batch_dev", "dfm_news_batch",
    "dfm_news_batch_dev", "dfm_pca_init_batch", "dfm_pca_init_batch_dev", "dfm_standardize_batch_dev", "dfm_als_batch",
    "dfm_ols_batch", "dfm_var_bootstrap_irf", "dfm_quantile_bands", "dfm_chow_batch", "dfm_synchronize", "dfm_chunk_fallbacks",
    "dfm_profile_enable", "dfm_profile_read", "dfm_hbm_probe", "dfm_set_stream", "dfm_last_error", "dfm_multi_create",
    "dfm_multi_destroy", "dfm_multi_ngpu", "dfm_multi_has_comm", "dfm_multi_last_error", "dfm_multi_load", "dfm_multi_synth",
    "dfm_multi_ks_pass", "dfm_multi_em", "dfm_multi_fetch"}


def test_every_bound_symbol_was_reached():
    """Runs last in this file: the set of symbols the tests above reached is the list written here, and that list is what
    kalman.py names."""
    import re
    with open(kalman.__file__) as fh:
        src = fh.read()
    named = set(re.findall(r"\bdfm_[a-z0-9_]+\b", src)) & set(_lib.SYMBOLS)
    built = {f"dfm_{kind}{fam}_batch{sfx}" for kind in ("ks_pass", "em") for fam in FAMILY for sfx in ("", "_dev")}
    built |= {f"dfm_{n}_batch{sfx}" for n in ("forecast", "simsmooth", "news") for sfx in ("", "_dev")}
    assert (named | built) - {"dfm_synth_panels_dev", "dfm_create", "dfm_destroy"} == EXPECTED
    assert REACHED == EXPECTED
