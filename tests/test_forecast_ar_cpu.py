"""CPU checks of the forecasts with AR idiosyncratic terms (dfm_forecast_ar_batch, csrc/forecast_ar.hip), no device needed: the
expectation model of tests/forecast_ar_expect.py against brute-force conditioning of the joint Gaussian, the NumPy restatement of
the kernels' two-filter recursion against dense conditioning on the GPU case table's patterns, the reach of the initial variance
v0, the variance caveat's ratios, the geometry header against its restatement, the binding's marshalling against a recording
library, and api.forecast_ar_idio's argument errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, forecasting_ar, kalman
from tests import forecast_ar_expect as fe
from tests.api_calls import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCED = [(6, 14, 2, 1, 2, 4), (5, 12, 1, 2, 1, 3), (8, 16, 2, 2, 3, 5), (30, 20, 2, 1, 2, 4)]      # N, T, r, p, q, H
KEYS = fe.KEYS


@pytest.fixture(scope="module")
def balanced():
    """Per shape: the inputs, the expectation model's outputs and brute force's horizon mean and variance, computed once."""
    out = {}
    for shape in BALANCED:
        N, T, r, p, q, H = shape
        x, st, v0 = fe.synth(0, N, T, r, p, q)
        args = [st[k] for k in KEYS]
        out[shape] = dict(x=x, args=args, v0=v0, e=fe.expect(x, *args, H, v0=v0), brute=fe.brute_force(x, *args, H))
    return out


@pytest.mark.parametrize("shape", BALANCED)
def test_horizon_means_are_the_exact_conditional_means(balanced, shape):
    H = shape[5]
    c = balanced[shape]
    err = np.abs(c["e"]["xhat"][-H:] - c["brute"][0]).max()
    print(f"{shape}: horizon means against brute force: {err:.2e}")
    assert err <= 1e-10


def test_variance_ratios(balanced):
    """xvar adds the two variances and leaves out the cross-period covariance of the factor estimation error: not exact.  The
    ratios are printed for DESIGN.md section 20; nothing is asserted about them beyond their sign."""
    for shape in BALANCED:
        H = shape[5]
        ratio = balanced[shape]["e"]["xvar"][-H:] / balanced[shape]["brute"][1]
        print(f"{shape}: xvar / exact over the horizon in [{ratio.min():.3f}, {ratio.max():.3f}]")
        assert np.all(ratio > 0.0)


def _series_of_the_case_table():
    """(case, residual column with the case's missing pattern, rho_i, sig2_i, v0_i) for every series of every GPU case; the
    residuals are the panel's own cells of the output rows followed by the horizon."""
    for name in fe.CASES:
        c = fe.make_case(name)
        B, N, T, r, p, q, H = c["dims"]
        for b in range(B):
            u = np.vstack([c["x"][b][q:], np.full((H, N), np.nan)])
            for i in range(N):
                yield name, u[:, i], c["st"]["rho"][b, i], c["st"]["sig2"][b, i], c["v0"][b, i]


def test_two_filter_recursion_is_dense_conditioning_on_the_case_table():
    worst, count, stored = 0.0, 0, 0
    for name, u, rho, sig2, v0 in _series_of_the_case_table():
        assert np.abs(rho).sum() <= 0.85 + 1e-12, name
        e1, V1 = fe.dense_idio(u, rho, sig2, v0)
        e2, V2, st = fe.two_filter(u, rho, sig2, v0)
        obs = ~np.isnan(u)
        assert st == [t for t in range(len(u)) if not obs[t] and obs[t + 1:].any()], name
        worst = max(worst, np.abs(e1 - e2).max(), np.abs(V1 - V2).max())
        count += 1
        stored += len(st)
    print(f"{count} series, {stored} stored messages, worst difference {worst:.2e}")
    assert worst <= 1e-12


def test_case_table_reaches_every_class():
    dims = {name: v[:7] for name, v in fe.CASES.items()}
    kinds = set()
    for name in fe.CASES:
        kinds |= fe.make_case(name)["kinds"]
    assert kinds == set(range(1, fe.N_KINDS)), kinds
    assert {d[5] for d in dims.values()} == {1, 2, 3, 4}
    rel = {(d[4] > d[5] + 1) - (d[4] < d[5] + 1) for d in dims.values()}
    assert rel == {-1, 0, 1}, "p below, at and above q + 1"
    assert {1, 8} <= {d[3] for d in dims.values()} and any(d[3] == 8 and d[5] == 3 for d in dims.values())
    assert {1, 64, 65, 139, 256, 257, 513} <= {d[1] for d in dims.values()}
    assert {fe.geometry(d[1], d[3], d[2] + d[6] - d[5])[4] for d in dims.values()} == {1, 2, 3}
    assert any(d[2] == d[5] + 1 for d in dims.values()) and {0, 1, 41} <= {d[6] for d in dims.values()}
    assert any(d[6] > fe.geometry(d[1], d[3] + d[3] * (d[3] + 1) // 2, d[2] + d[6] - d[5])[2] for d in dims.values()), "a horizon longer than a chunk"
    assert {1, 3} <= {d[0] for d in dims.values()}
    assert any(v[7] is None and v[6] > 0 for v in fe.CASES.values()), "a balanced panel with H > 0"


def test_v0_reaches_no_further_than_the_first_q_observed_rows():
    """Once q CONSECUTIVE output rows of a series are observed its state a_t is known exactly, and by the Markov property nothing
    before them -- v0 included -- bears on the cells after them.  (Observed rows with gaps between them leave a lag of the state
    unknown, and v0's influence then only decays; such series are not part of the claim.)  Checked from three rows after the last
    of the first q observed rows onward, on the balanced shapes and on every series of the case table whose first q observed rows
    are consecutive."""
    worst, count = 0.0, 0

    def one(u, rho, sig2, v0):
        nonlocal worst, count
        q = len(rho)
        first = np.nonzero(~np.isnan(u))[0][:q]
        if len(first) < q or first[-1] - first[0] != q - 1 or first[-1] + 3 >= len(u):
            return
        for idio in (fe.dense_idio, fe.two_filter):
            a, b = idio(u, rho, sig2, v0)[:2], idio(u, rho, sig2, 50.0 * v0)[:2]
            s = slice(first[-1] + 3, None)
            worst = max(worst, np.abs(a[0][s] - b[0][s]).max(), np.abs(a[1][s] - b[1][s]).max())
        count += 1

    for N, T, r, p, q, H in BALANCED:
        x, st, v0 = fe.synth(1, N, T, r, p, q)
        u = np.vstack([x[q:], np.full((H, N), np.nan)])
        for i in range(N):
            one(u[:, i], st["rho"][i], st["sig2"][i], v0[i])
    for name, u, rho, sig2, v0 in _series_of_the_case_table():
        one(u, rho, sig2, v0)
    print(f"{count} series, worst move under v0 -> 50 v0: {worst:.2e}")
    assert count > 500 and worst <= 1e-12


def test_geometry_header_against_its_restatement(tmp_path):
    exe = str(tmp_path / "seriesgeom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "seriesgeom_host.cpp")], check=True)
    lds = 48 * 1024
    req = [(N, row, rows, lds) for N in range(1, 1101) for row, rows in ((1, 1), (2, 40), (5, 79), (44, 33), (152, 500))]
    req += [(139, 152, 226, 4096), (139, 600, 10, 4096)]
    text = "".join(" ".join(map(str, q)) + "\n" for q in req)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(req)
    for q, line in zip(req, out):
        got = tuple(map(int, line.split()))
        assert got == fe.geometry(q[0], q[1], q[2], lds_bytes=q[3]), (q, got)
        NPB, G, RC, nchunk, nsblk, threads = got
        assert G == 1 and NPB <= 256 and nsblk * NPB >= q[0] and (nsblk - 1) * NPB < q[0] and threads % 64 == 0 and NPB <= threads < NPB + 64
        assert 1 <= RC <= 32 and (nchunk - 1) * RC < q[2] <= nchunk * RC and (RC * q[1] * 8 <= q[3] or RC == 1)


# ---------------------------------------------------------------------------------------------------- marshalling
B, T, N, r, p, q, H = 2, 12, 6, 2, 2, 1, 3
HANDLE = 0xD0F0
NPK = r * (r + 1) // 2


class _OnDevice(torch.Tensor):
    is_cuda = True


def _make_ctx():
    ctx = kalman.DfmContext.__new__(kalman.DfmContext)
    ctx._lib, ctx._h, ctx._torch, ctx._use_torch_stream, ctx.device = Recorder(), ctypes.c_void_p(HANDLE), torch, False, 0
    ctx._dev = lambda t, name, shape=None: kalman.DfmContext._dev(ctx, t.as_subclass(_OnDevice), name, shape)
    return ctx


def _arrays():
    g = np.random.default_rng(0)
    k = r * max(p, q + 1)
    a = dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), sig2=g.random((B, N)) + 1,
             rho=0.3 * g.standard_normal((B, N, q)), Avar=g.standard_normal((B, r, r * p)), Q=g.standard_normal((B, r, r)),
             mu0=g.standard_normal((B, k)), P0=g.standard_normal((B, k, k)), v0=g.random((B, N)) + 1, mean=g.standard_normal((B, N)),
             sd=g.random((B, N)) + 1)
    a["panel"][1, 3, 2] = np.nan
    return a


def _addr(a):
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _val(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


INPUTS = ("panel", "Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
OUT_ORDER = ("xhat", "xvar", "common", "idio", "f", "P", "loglik")


@pytest.mark.parametrize("side", ["host", "dev"])
@pytest.mark.parametrize("opts", [dict(), dict(v0=False), dict(scaled=False), dict(want=("xvar",)), dict(want=()),
                                  dict(want=("common", "idio", "P", "loglik")), dict(missing=False), dict(missing=True)])
def test_marshalling(side, opts):
    ctx = _make_ctx()
    a = _arrays()
    if side == "dev":
        a = {k: torch.from_numpy(v) for k, v in a.items()}
    kw = {}
    if opts.get("v0", True):
        kw["v0"] = a["v0"]
    if opts.get("scaled", True):
        kw.update(mean=a["mean"], sd=a["sd"])
    if "want" in opts:
        kw["want"] = opts["want"]
    if "missing" in opts:
        kw["may_have_missing"] = opts["missing"]
    fn = ctx.forecast_ar_batch_host if side == "host" else ctx.forecast_ar_batch_dev
    out = fn(*[a[k] for k in INPUTS], H, **kw)
    name = "dfm_forecast_ar_batch" + ("" if side == "host" else "_dev")
    assert [c[0] for c in ctx._lib.calls] == [name]
    args = ctx._lib.calls[0][1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds)
    for x, kind in zip(args, kinds):
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int
        else:
            assert x is None or isinstance(x, ctypes.c_void_p)
    assert _val(args[0]) == HANDLE and args[1:8] == (B, T, N, r, p, q, H)
    for i, k in enumerate(INPUTS):
        assert _val(args[8 + i]) == _addr(a[k]), k
    assert _val(args[16]) == (_addr(a["v0"]) if "v0" in kw else None)
    assert _val(args[17]) == (_addr(a["mean"]) if "mean" in kw else None) and _val(args[18]) == (_addr(a["sd"]) if "sd" in kw else None)
    want = opts.get("want", forecasting_ar.OPTIONAL)
    n = T + H - q
    shapes = dict(xhat=(B, n, N), xvar=(B, n, N), common=(B, n, N), idio=(B, n, N), f=(B, n, r), P=(B, n, NPK), loglik=(B,))
    assert set(out) == set(OUT_ORDER)
    for i, k in enumerate(OUT_ORDER):
        if k in ("xhat", "f") or k in want:
            assert type(out[k]) is (np.ndarray if side == "host" else torch.Tensor) and tuple(out[k].shape) == shapes[k], k
            assert str(out[k].dtype).endswith("float64") and _val(args[19 + i]) == _addr(out[k]), k
        else:
            assert out[k] is None and args[19 + i] is None, k
    assert args[26] == (0 if opts.get("missing") is False else _lib.DFM_F_MAY_HAVE_MISSING)


def test_binding_argument_errors():
    ctx = _make_ctx()
    a = _arrays()
    args = [a[k] for k in INPUTS]
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, -1)
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, H, mean=a["mean"])
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, H, want=("xvar", "nonsense"))
    with pytest.raises(ValueError):                                                    # q = 0 is forecast_batch's model
        ctx.forecast_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 0)) for k in INPUTS], H)
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 5)) for k in INPUTS], H)
    with pytest.raises(ValueError):                                                    # T <= q
        ctx.forecast_ar_batch_host(a["panel"][:, :1], *args[1:], H)
    with pytest.raises(ValueError):                                                    # the device side checks shapes
        ctx.forecast_ar_batch_dev(*[torch.from_numpy(v) for v in args], H, v0=torch.from_numpy(a["v0"][:, :-1].copy()))
    assert ctx._lib.calls == []


def test_the_symbols_are_declared_once_everywhere():
    hdr = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    for name in ("dfm_forecast_ar_batch", "dfm_forecast_ar_batch_dev"):
        assert name in _lib.SYMBOLS and hdr.count(f"int {name}(") == 1
        assert len(_lib.SYMBOLS[name][1]) == 27
    assert jl.count(":dfm_forecast_ar_batch,") == 1 and "function forecast_ar(" in jl
    src = open(kalman.__file__).read()
    assert "dfm_forecast_ar" not in src and "forecasting_ar" in src


# ---------------------------------------------------------------------------------------------------- api.forecast_ar_idio
def _model(n_uarlag=2, nfac_o=0):
    g = np.random.default_rng(3)
    data = g.standard_normal((60, 8))
    m = api.DFMModel(data, np.ones(8, dtype=int), 20, 3, 1, 50, nfac_o, 2, 1e-8, n_uarlag, 1)
    return m


def test_api_argument_errors_come_before_any_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device was reached: " + name)

    m = _model()
    with pytest.raises(ValueError, match="H must be"):
        api.forecast_ar_idio(m, -1, ctx=NoDevice())
    with pytest.raises(ValueError, match="through"):
        api.forecast_ar_idio(m, 2, through=m.lastperiod - 1, ctx=NoDevice())
    with pytest.raises(ValueError, match="through"):
        api.forecast_ar_idio(m, 2, through=m.T + 1, ctx=NoDevice())
    with pytest.raises(ValueError, match="not estimated|first"):                       # nothing estimated yet
        api.forecast_ar_idio(m, 2, ctx=NoDevice())
    m5 = _model(n_uarlag=5)
    with pytest.raises(ValueError, match="n_uarlag"):
        api.forecast_ar_idio(m5, 2, ctx=NoDevice())


def test_ar_model_inputs_through_defaults_to_todays_rows():
    """`through` only lengthens the panel handed to the library; parameters, intercepts and P0 stay the estimation window's."""
    g = np.random.default_rng(4)
    m = _model()
    r, p, q, Nn = m.nfac_u, m.factor_var_model.nlag, m.n_uarlag, m.data.shape[1]
    m.factor[:] = g.standard_normal(m.factor.shape)
    m.lambda_[:] = g.standard_normal((Nn, r))
    m.uar_coef[:] = 0.2 * g.standard_normal((Nn, q))
    m.uar_ser[:] = g.random(Nn) + 0.5
    var = m.factor_var_model
    var.betahat = 0.1 * g.standard_normal((r * p + (1 if var.withconst else 0), r))
    var.seps = np.eye(r)
    base, cols, mu_f, c_i = api._ar_model_inputs(m)
    same, cols2, mu2, c2 = api._ar_model_inputs(m, m.lastperiod)
    for k in base:
        assert np.array_equal(base[k], same[k], equal_nan=True), k
    longer, cols3, mu3, c3 = api._ar_model_inputs(m, m.T)
    assert longer["x"].shape[0] == m.T - m.initperiod + 1 and np.array_equal(longer["x"][:base["x"].shape[0]], base["x"], equal_nan=True)
    for k in base:
        if k != "x":
            assert np.array_equal(base[k], longer[k]), k
    assert np.array_equal(c_i, c3) and np.array_equal(mu_f, mu3) and np.array_equal(cols, cols3)
