"""CPU checks of the filter with AR idiosyncratic terms (dfm_filter_ar_batch, csrc/filter_ar.hip), no device needed: the
expectation model of tests/filter_ar_expect.py against dense conditioning of the joint Gaussian (the h-step forecasts of every
origin of balanced panels) and against the oracle's pass (log-likelihood, last filtered moments), the binding's marshalling against
a recording library, the argument errors of the two api functions, the staged row size and geometry the fill's launcher takes from
csrc/dfm_cellgeom.h against their restatement, and the missing-cell cases of the GPU table, which must count origins."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, filtering_ar, kalman
from oracle import ar_oracle as ao
from tests import filter_ar_expect as fe
from tests import forecast_ar_expect as fae
from tests.api_calls import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCED = [(6, 14, 2, 1, 2, 4), (5, 12, 1, 2, 1, 3), (8, 16, 2, 2, 3, 5), (7, 15, 2, 3, 1, 4), (4, 14, 1, 1, 4, 3)]  # N, T, r, p, q, H
KEYS = fe.KEYS


# ---------------------------------------------------------------------------------------------------- the expectation model
@pytest.mark.parametrize("shape", BALANCED)
def test_forecasts_are_the_exact_conditional_means(shape):
    """Every origin t of a balanced panel: the expectation's h-step forecasts against E[x_{t+h} | x_0 .. x_t] from the joint Gaussian
    of every cell built by the model's own recursion (forecast_ar_expect.brute_force: no quasi-differencing, no filter)."""
    N, T, r, p, q, H = shape
    x, st, _ = fae.synth(0, N, T, r, p, q)
    args = [st[k] for k in KEYS]
    Z, M, Qc, _ = fe.state_space(st["Lam"], st["rho"], st["Avar"], st["Q"])
    zf = fe.textbook_filter(fe.quasi_difference(x, st["rho"]), Z, st["sig2"], M, Qc, st["mu0"], st["P0"])[2]
    worst = 0.0
    for t in range(q, T):
        full, common, ok = fe.forecasts(x, st["Lam"], st["rho"], M, zf[t - q], t, H)
        assert ok.all()
        exact = fae.brute_force(x[:t + 1], *args, H)[0]
        worst = max(worst, float(np.abs(full - exact).max()))
        assert np.abs(common - exact).max() > 1e-6          # the factor-only forecast is another number
    print(f"{shape}: forecasts of every origin against dense conditioning: {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("missing", [0.0, 0.15])
def test_model_against_the_oracles_pass(missing):
    N, T, r, p, q = 9, 30, 2, 3, 2
    x, st = fe.params_for(1, N, T, r, p, q, missing=missing)
    args = [st[k][0] for k in KEYS]
    e = fe.expect(x[0], *args)
    o = ao.kfs_pass_ar(x[0], *args)
    assert abs(e["loglik_t"].sum() - o["loglik"]) <= 1e-9 * max(1.0, abs(o["loglik"]))
    assert np.abs(e["z_filt"][-1] - o["f_smooth"][-1]).max() <= 1e-10
    assert np.abs(e["P_filt"][-1] - fe.pack(o["P_smooth"][-1])).max() <= 1e-10
    # x - xpred is verr wherever both are defined (sd = 1, mean = 0)
    both = ~np.isnan(e["verr"])
    assert np.abs((x[0][q:] - e["xpred"])[both] - e["verr"][both]).max() <= 1e-12
    assert np.array_equal(np.isnan(e["vstd"]), np.isnan(fe.quasi_difference(x[0], st["rho"][0])))


def test_evaluation_counts_follow_the_qualification_rule():
    N, T, r, p, q, H, t0 = 8, 40, 2, 1, 2, 3, 6
    x, st = fe.params_for(1, N, T, r, p, q)
    fe.missing_pattern(x, q)
    e = fe.expect(x[0], *[st[k][0] for k in KEYS], H=H, t0=t0)
    obs = ~np.isnan(x[0])
    for h in range(1, H + 1):
        for i in range(N):
            n = sum(1 for t in range(t0, T - h) if obs[t + h, i] and all(obs[t - l, i] for l in range(q)))
            assert e["cnt"][h - 1, i] == n
    assert np.all(e["cnt"][:, 4] == 0) and np.all(np.isnan(e["msfe"][:, 4]))
    assert np.array_equal(np.isnan(e["msfe"]), e["cnt"] == 0) and np.array_equal(np.isnan(e["msfe_common"]), e["cnt"] == 0)


def test_missing_cell_cases_of_the_gpu_table_count_origins():
    """The GPU comparison of a case with missing cells must not pass on NaN alone: cnt > 0 on at least half of its (h, i) pairs."""
    seen = 0
    for row in fe.CASES:
        c, x, st, mean, sd = fe.make_case(row)
        if c["missing"] == 0.0:
            continue
        assert c["H"] > 0 and np.isnan(x).any(), c["name"]
        seen += 1
        for b in range(c["B"]):
            cnt = fe.expect_case(x, st, b, c["H"], c["t0"], mean, sd)["cnt"]
            assert (cnt > 0).mean() >= 0.5, (c["name"], b, float((cnt > 0).mean()))
    assert seen >= 8


def test_gpu_case_table_covers_what_it_must():
    rows = [fe.case_dict(r) for r in fe.CASES]
    assert len({c["name"] for c in rows}) == len(rows)
    assert {c["q"] for c in rows} == {1, 2, 3, 4}
    assert any(c["p"] < c["q"] + 1 for c in rows) and any(c["p"] == c["q"] + 1 for c in rows) and any(c["p"] > c["q"] + 1 for c in rows)
    assert any(c["r"] == 1 for c in rows)
    kw = {(c["r"] * max(c["p"], c["q"] + 1), c["r"] * (c["q"] + 1)) for c in rows}
    assert (32, 16) in kw and (32, 32) in kw
    assert {1, 64, 65, 139, 256, 257, 513} <= {c["N"] for c in rows}
    assert any(c["T"] == c["q"] + 1 for c in rows) and any(c["T"] - c["t0"] > 64 and c["H"] > 0 for c in rows)
    assert any(c["H"] == 0 for c in rows) and any(c["H"] == 1 for c in rows) and any(c["H"] >= c["T"] - c["t0"] > 1 for c in rows)
    assert {1, 2, 3} <= {c["B"] for c in rows}
    assert any(c["scaled"] for c in rows) and any(not c["scaled"] for c in rows) and any(not c["aligned"] for c in rows)
    for c in rows:                                      # the entry's limits
        k = c["r"] * max(c["p"], c["q"] + 1)
        assert k <= 32 and c["N"] <= (1024 if k <= 8 else 512 if k <= 16 else 256) and c["q"] <= c["t0"] < c["T"]
    seen = set()
    for c in rows:
        g = fe.fill_launch(c["B"], c["N"], c["r"], c["q"], c["T"], c["aligned"])
        seen |= {f"wb={g['WB']}", "vec" if g["vec"] else "scalar", f"nsblk={min(g['nsblk'], 3)}"}
    assert {"wb=4", "wb=8", "wb=16", "wb=32", "vec", "scalar", "nsblk=1", "nsblk=2", "nsblk=3"} <= seen


# ---------------------------------------------------------------------------------------------------- the fill's launch geometry
def test_staged_row_and_geometry_against_the_header(tmp_path):
    exe = str(tmp_path / "filter_ar_geom_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "filter_ar_geom_host.cpp")], check=True)
    shapes = [(r, q) for r in (1, 2, 3, 4, 8, 16) for q in (1, 2, 3, 4) if r * (q + 1) <= 32]
    req = [(N, r, q, rows, al) for N in (1, 2, 64, 65, 139, 256, 257, 512, 513, 1024) for (r, q) in shapes for rows in (1, 7, 40, 218)
           for al in (1, 0)]
    text = "".join(f"{N} {r * (q + 1)} {rows} {al}\n" for N, r, q, rows, al in req)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(req)
    sps = set()
    for (N, r, q, rows, al), line in zip(req, out):
        SP, WB, row, NPB, G, RC, nchunk, nsblk, threads = map(int, line.split())
        w = r * (q + 1)
        assert row == fe.fill_row_doubles(r, q) == w + w * (w + 1) // 2
        g = fe.fill_launch(1, N, r, q, rows + q, aligned=bool(al))
        assert (SP, WB) == (g["SP"], g["WB"]) and WB >= w
        assert (NPB, G, RC, nchunk, nsblk, threads) == tuple(g[k] for k in fe.pg.GEOM_FIELDS)
        assert RC * row * 8 <= fe.FTAR_LDS and threads <= fe.FTAR_MAX_THREADS and nsblk * NPB * SP >= N
        sps.add(SP)
    assert sps == {1, 2}


# ---------------------------------------------------------------------------------------------------- marshalling
B, T, N, r, p, q, H, T0 = 2, 12, 6, 2, 2, 1, 3, 4
K = r * max(p, q + 1)
KK = K * (K + 1) // 2
HANDLE = 0xD0F0


class _OnDevice(torch.Tensor):
    is_cuda = True


def _make_ctx():
    ctx = kalman.DfmContext.__new__(kalman.DfmContext)
    ctx._lib, ctx._h, ctx._torch, ctx._use_torch_stream, ctx.device = Recorder(), ctypes.c_void_p(HANDLE), torch, False, 0
    ctx._dev = lambda t, name, shape=None: kalman.DfmContext._dev(ctx, t.as_subclass(_OnDevice), name, shape)
    return ctx


def _arrays():
    g = np.random.default_rng(0)
    a = dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), sig2=g.random((B, N)) + 1,
             rho=0.3 * g.standard_normal((B, N, q)), Avar=g.standard_normal((B, r, r * p)), Q=g.standard_normal((B, r, r)),
             mu0=g.standard_normal((B, K)), P0=g.standard_normal((B, K, K)), mean=g.standard_normal((B, N)), sd=g.random((B, N)) + 1)
    a["panel"][1, 3, 2] = np.nan
    return a


def _addr(a):
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _val(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


INPUTS = ("panel", "Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


@pytest.mark.parametrize("side", ["host", "dev"])
@pytest.mark.parametrize("opts", [dict(), dict(scaled=False), dict(want=("loglik_t",)), dict(want=()), dict(H=0), dict(t0=None),
                                  dict(want=("msfe_common", "cnt", "vstd")), dict(missing=False), dict(missing=True)])
def test_marshalling(side, opts):
    ctx = _make_ctx()
    a = _arrays()
    if side == "dev":
        a = {k: torch.from_numpy(v) for k, v in a.items()}
    h = opts.get("H", H)
    kw = dict(H=h)
    if "t0" not in opts:
        kw["t0"] = T0
    if opts.get("scaled", True):
        kw.update(mean=a["mean"], sd=a["sd"])
    if "want" in opts:
        kw["want"] = opts["want"]
    if "missing" in opts:
        kw["may_have_missing"] = opts["missing"]
    fn = ctx.filter_ar_batch_host if side == "host" else ctx.filter_ar_batch_dev
    out = fn(*[a[k] for k in INPUTS], **kw)
    name = "dfm_filter_ar_batch" + ("" if side == "host" else "_dev")
    assert [c[0] for c in ctx._lib.calls] == [name]
    args = ctx._lib.calls[0][1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds) == 32
    for x, kind in zip(args, kinds):
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int
        else:
            assert x is None or isinstance(x, ctypes.c_void_p)
    assert _val(args[0]) == HANDLE and args[1:9] == (B, T, N, r, p, q, h, T0 if "t0" not in opts else q)
    for i, k in enumerate(INPUTS):
        assert _val(args[9 + i]) == _addr(a[k]), k
    assert _val(args[17]) == (_addr(a["mean"]) if "mean" in kw else None) and _val(args[18]) == (_addr(a["sd"]) if "sd" in kw else None)
    want = opts.get("want", filtering_ar.OUTPUTS)
    n = T - q
    shapes = dict(z_pred=(B, n, K), P_pred=(B, n, KK), z_filt=(B, n, K), P_filt=(B, n, KK), loglik_t=(B, n), xpred=(B, n, N),
                  verr=(B, n, N), vstd=(B, n, N), msfe=(B, h, N), msfe_common=(B, h, N), msfe0=(B, h, N), cnt=(B, h, N))
    assert tuple(out) == filtering_ar.OUTPUTS == fe.OUTPUTS
    for i, k in enumerate(filtering_ar.OUTPUTS):
        if k in want and not (k in filtering_ar.EVAL and h == 0):
            assert type(out[k]) is (np.ndarray if side == "host" else torch.Tensor) and tuple(out[k].shape) == shapes[k], k
            assert str(out[k].dtype).endswith("int32" if k == "cnt" else "float64") and _val(args[19 + i]) == _addr(out[k]), k
        else:
            assert out[k] is None and args[19 + i] is None, k
    assert args[31] == (0 if opts.get("missing") is False else _lib.DFM_F_MAY_HAVE_MISSING)


def test_binding_argument_errors():
    ctx = _make_ctx()
    a = _arrays()
    args = [a[k] for k in INPUTS]
    with pytest.raises(ValueError):
        ctx.filter_ar_batch_host(*args, H=-1)
    with pytest.raises(ValueError):
        ctx.filter_ar_batch_host(*args, H=H, mean=a["mean"])
    with pytest.raises(ValueError):
        ctx.filter_ar_batch_host(*args, H=H, want=("vstd", "nonsense"))
    for t0 in (q - 1, T):
        with pytest.raises(ValueError):
            ctx.filter_ar_batch_host(*args, H=H, t0=t0)
    with pytest.raises(ValueError):                                                    # q = 0 is filter_batch's model
        ctx.filter_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 0)) for k in INPUTS], H=H)
    with pytest.raises(ValueError):
        ctx.filter_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 5)) for k in INPUTS], H=H)
    with pytest.raises(ValueError):                                                    # T <= q
        ctx.filter_ar_batch_host(a["panel"][:, :1], *args[1:], H=H)
    assert ctx._lib.calls == []


def test_the_symbols_are_declared_once_everywhere():
    hdr = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    for name in ("dfm_filter_ar_batch", "dfm_filter_ar_batch_dev"):
        assert name in _lib.SYMBOLS and hdr.count(f"int {name}(") == 1
        assert len(_lib.SYMBOLS[name][1]) == 1 + 8 + 22 + 1 and _lib.SYMBOLS[name][1][-1] is _lib.c_uint
    assert jl.count(":dfm_filter_ar_batch,") == 1 and "function filter_ar(" in jl and "function evaluate_forecasts_ar(" in jl
    src = open(kalman.__file__).read()
    assert "dfm_filter_ar" not in src and "filtering_ar" in src
    assert kalman.DfmContext.filter_ar_batch_host is filtering_ar.filter_ar_batch_host
    assert kalman.DfmContext.filter_ar_batch_dev is filtering_ar.filter_ar_batch_dev
    from dynamic_factor_models_amd import build
    assert "filter_ar.hip" in build.SOURCES


# ---------------------------------------------------------------------------------------------------- the api
def _model(n_uarlag=2):
    g = np.random.default_rng(3)
    data = g.standard_normal((60, 8))
    return api.DFMModel(data, np.ones(8, dtype=int), 20, 3, 1, 50, 0, 2, 1e-8, n_uarlag, 1)


def _filled(m):
    g = np.random.default_rng(4)
    rr, pp, qq, Nn = m.nfac_u, m.factor_var_model.nlag, m.n_uarlag, m.data.shape[1]
    m.factor[:] = g.standard_normal(m.factor.shape)
    m.lambda_[:] = g.standard_normal((Nn, rr))
    m.uar_coef[:] = 0.2 * g.standard_normal((Nn, qq))
    m.uar_ser[:] = g.random(Nn) + 0.5
    var = m.factor_var_model
    var.betahat = 0.1 * g.standard_normal((rr * pp + (1 if var.withconst else 0), rr))
    var.seps = np.eye(rr)
    return m


def test_api_argument_errors_come_before_any_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device was reached: " + name)

    m = _model()
    with pytest.raises(ValueError, match="H must be"):
        api.evaluate_forecasts_ar_idio(m, 0, ctx=NoDevice())
    for fn in (lambda **kw: api.filter_states_ar_idio(m, ctx=NoDevice(), **kw),
               lambda **kw: api.evaluate_forecasts_ar_idio(m, 2, ctx=NoDevice(), **kw)):
        with pytest.raises(ValueError, match="through"):
            fn(through=m.lastperiod - 1)
        with pytest.raises(ValueError, match="through"):
            fn(through=m.T + 1)
        with pytest.raises(ValueError, match="not estimated|first"):                   # nothing estimated yet
            fn()
    with pytest.raises(ValueError, match="parameter sets"):                            # estimate_ar_idio has no replicates
        api.evaluate_forecasts_ar_idio(m, 2, quantiles=[0.5], ctx=NoDevice())
    m5 = _model(n_uarlag=5)
    with pytest.raises(ValueError, match="n_uarlag"):
        api.filter_states_ar_idio(m5, ctx=NoDevice())
    with pytest.raises(ValueError, match="n_uarlag"):
        api.evaluate_forecasts_ar_idio(m5, 2, ctx=NoDevice())
    m = _filled(_model())
    qq = m.n_uarlag
    for fo in (m.initperiod + qq - 1, m.lastperiod + 1):
        with pytest.raises(ValueError, match="first_origin"):
            api.evaluate_forecasts_ar_idio(m, 2, first_origin=fo, ctx=NoDevice())
    inputs = api._ar_model_inputs(m)[0]
    own = {k: np.stack([inputs[k], inputs[k]]) for k in KEYS}
    with pytest.raises(ValueError, match="lacks"):
        api.evaluate_forecasts_ar_idio(m, 2, params={k: v for k, v in own.items() if k != "P0"}, ctx=NoDevice())
    with pytest.raises(ValueError, match="model's own shape"):
        api.evaluate_forecasts_ar_idio(m, 2, params=dict(own, rho=own["rho"][:, :, :1]), ctx=NoDevice())
    with pytest.raises(ValueError, match="quantiles"):
        api.evaluate_forecasts_ar_idio(m, 2, params=own, quantiles=[1.5], ctx=NoDevice())
    with pytest.raises(ValueError, match="one parameter set"):
        api.filter_states_ar_idio(m, params=own, ctx=NoDevice())
