"""CPU tests of the news decomposition with AR idiosyncratic terms (dfm_news_ar_batch), no device:
the expectation model of tests/news_ar_expect.py against dense conditioning of the model's own joint Gaussian, its weights against
the unit-step derivative of the forecast's expectation model, the structured covariance recursion against the quasi-difference of
the dense covariance, the exact invariants, the edge-shape rule with the measured reason for it, and the binding's plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, kalman, news_ar
from tests import forecast_ar_expect as fe
from tests import news_ar_expect as ne
from tests.api_calls import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ne.KEYS
SHAPES = [(6, 14, 2, 1, 2, 3), (5, 13, 1, 2, 1, 2), (7, 16, 2, 2, 3, 2), (4, 12, 2, 3, 1, 1)]      # N, T, r, p, q, H; the last: p > q + 1
TOL = 1e-10                                                                                        # the bound of tests/test_news_cpu.py


def _inputs(shape):
    """Edge-shaped vintages with a revised cell, a ragged edge shorter and one longer than q, a series at L = 2q - 1 and one without
    news; targets: a ragged-edge cell (news), horizon cells (the first and the last horizon row), a cell observed in old."""
    N, T, r, p, q, H = shape
    x, st, v0 = ne.synth(1, N, T, r, p, q)
    Lo, Ln = np.full(N, T - 1 - (q + 1)), np.full(N, T - 1)                     # the edge is q + 1 rows deep: longer than q
    Lo[0] = 2 * q - 1
    Lo[1], Ln[1] = T - 2, T - 1                                                # one row: not longer than q
    Lo[2] = Ln[2] = T - 2                                                      # no news, still missing in the last row
    Ln[N - 1] = T - 2
    old, new = ne.vintages(x, Lo, Ln, [(T - q - 3, 3 % N, 0.06), (0, 1, 0.05)])
    targets = [(T - 1, 0), (T + H - 1, 1), (q + 2, 3 % N), (T, N - 1), (T - 1, 2), (T - 1, 1)]
    return old, new, st, v0, targets


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in SHAPES:
        old, new, st, v0, tg = _inputs(shape)
        assert news_ar.edge_shape_error(old, new, shape[4]) is None
        out[shape] = dict(old=old, new=new, st=st, v0=v0, tg=tg, e=ne.expect(old, new, st, tg, v0=v0), b=ne.brute_force(old, new, st, tg))
    return out


# ---------------------------------------------------------------------------------------------------- (a) against brute force
@pytest.mark.parametrize("shape", SHAPES)
def test_expectation_against_dense_conditioning(cases, shape):
    c = cases[shape]
    e, b = c["e"], c["b"]
    assert np.abs(ne.model_matrices(c["st"])[0]).max() < 10 and np.abs(b["C"]).max() < 100      # a stable VAR: the brute force is sound
    for key in ("yhat", "news", "weight"):
        err = np.abs(e[key] - b[key]).max()
        assert err <= TOL, (key, err)
    on_news = np.where(e["cells"][None], e["weight"], 0.0)
    err = np.abs(on_news - b["news_weight"]).max()
    assert err <= TOL, ("Cov(y, I) Var(I)^-1", err)
    assert e["cells"].sum() > 0 and np.abs(e["yhat"][1] - e["yhat"][0]).max() > 1e-4              # news and a data revision exist
    assert np.abs(e["impact"].sum(axis=1) - (e["yhat"][2] - e["yhat"][1])).max() <= 1e-13


def test_scaled_outputs_are_the_standardised_ones_in_data_units(cases):
    shape = SHAPES[0]
    c = cases[shape]
    rng = np.random.default_rng(3)
    N = shape[0]
    mean, sd = rng.standard_normal(N), rng.uniform(0.5, 2.0, N)
    s = ne.expect(c["old"], c["new"], c["st"], c["tg"], v0=c["v0"], mean=mean, sd=sd)
    ti = [i for _, i in c["tg"]]
    assert np.abs(s["yhat"] - (mean[ti] + sd[ti] * c["e"]["yhat"])).max() <= 1e-13
    assert np.abs(s["news"] - sd * c["e"]["news"]).max() <= 1e-13
    assert np.abs(s["weight"] - c["e"]["weight"] * (sd[ti][:, None, None] / sd[None, None, :])).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------- (b) the derivative
def test_weights_are_the_unit_step_derivative_of_the_forecast(cases):
    shape = SHAPES[2]
    c = cases[shape]
    N, T, r, p, q, H = shape
    par = [c["st"][k] for k in KEYS]
    base = fe.expect(c["new"], *par, H, v0=c["v0"])["xhat"]
    fd = np.zeros_like(c["e"]["weight"])
    for t in range(q, T):
        for i in range(N):
            if np.isnan(c["new"][t, i]):
                continue
            xp = c["new"].copy()
            xp[t, i] += 1.0                                                    # the map is linear: a unit step is exact
            d = fe.expect(xp, *par, H, v0=c["v0"])["xhat"] - base
            fd[:, t - q, i] = [d[ts - q, i_s] for ts, i_s in c["tg"]]
    err = np.abs(fd - c["e"]["weight"]).max()
    assert err <= TOL, err


# ---------------------------------------------------------------------------------------------------- (c) the recursion
@pytest.mark.parametrize("shape", SHAPES)
def test_structured_covariance_panel_is_the_quasi_difference_of_the_dense_one(cases, shape):
    c = cases[shape]
    N, T, r, p, q, H = shape
    n = c["b"]["n"]
    for ts, i_s in c["tg"]:
        dense = ne.quasi_diff_of_cov(c["b"]["C"], c["st"], (ts - q) * N + i_s, n)
        got = ne.qc_panel(c["st"], ts - q, i_s, n)
        assert np.abs(got - dense).max() <= TOL * np.abs(dense).max(), (ts, i_s)


# ---------------------------------------------------------------------------------------------------- (d) invariants
def test_no_news_gives_exactly_zero_impacts(cases):
    c = cases[SHAPES[0]]
    rev = np.where(np.isnan(c["old"]), np.nan, c["new"])
    e = ne.expect(c["old"], rev, c["st"], c["tg"], v0=c["v0"])
    assert np.all(e["news"] == 0.0) and np.all(e["impact"] == 0.0) and np.array_equal(e["yhat"][1], e["yhat"][2])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_target_on_a_news_cell_weighs_itself_alone(cases, shape):
    c = cases[shape]
    N, T, r, p, q, H = shape
    for g, (ts, i_s) in enumerate(c["tg"]):
        if ts < T and c["e"]["cells"][ts - q, i_s]:
            w = c["e"]["weight"][g].copy()
            assert abs(w[ts - q, i_s] - 1.0) <= 1e-12
            w[ts - q, i_s] = 0.0
            assert np.abs(w).max() <= 1e-12
            break
    else:
        raise AssertionError("no target on a news cell")


# ---------------------------------------------------------------------------------------------------- (e) the edge-shape rule
def test_edge_shape_rule():
    N, T, r, p, q, H = SHAPES[0]
    old, new, st, v0, tg = _inputs(SHAPES[0])
    assert np.isnan(old[2 * q, 0]) and not np.isnan(old[2 * q - 1, 0])           # L = 2q - 1 is accepted
    assert news_ar.edge_shape_error(old, new, q) is None
    assert news_ar.edge_shape_error(old[None], new[None], q) is None

    def refused(o, n, column, condition, **kw):
        why = news_ar.edge_shape_error(o, n, q, **kw)
        assert why is not None and f"column {column} " in why and f"condition {condition}" in why, why
        return why
    o = old.copy(); o[2 * q - 1, 0] = np.nan                                   # L = 2q - 2
    refused(o, new, 0, 2)
    o, n = old.copy(), new.copy(); o[5, 4] = n[5, 4] = np.nan                  # an interior gap
    assert "interior gap" in refused(o, n, 4, 1)
    o, n = old.copy(), new.copy(); o[0, 3] = n[0, 3] = np.nan                  # a late start
    assert "starts late" in refused(o, n, 3, 1)
    o, n = old.copy(), new.copy(); o[:, 5] = n[:, 5] = np.nan                  # a never-observed series
    assert "never observed" in refused(o, n, 5, 2)
    n = new.copy(); n[T - 3:, 2] = np.nan                                      # old is not within new
    assert not np.isnan(old[T - 3, 2])
    refused(old, n, 2, 3)
    refused(old, n, 17, 3, cols=np.array([11, 13, 17, 19, 23, 29]))            # the caller's column names


def test_the_measured_gap_with_one_interior_gap(capsys):
    """Why interior gaps are refused: the AR pass quasi-differences one NaN into q + 1 NaN rows, so the conditional means no longer
    come from a projection on the observed cells and the decomposition stops adding up.  Prints the gap; asserts nothing about it."""
    for shape in SHAPES[:3]:
        N, T, r, p, q, H = shape
        old, new, st, v0, tg = _inputs(shape)
        e = ne.expect(old, new, st, tg, v0=v0)
        edge = np.abs(e["impact"].sum(axis=1) - (e["yhat"][2] - e["yhat"][1])).max()
        old[2 * q + 1, N - 2] = new[2 * q + 1, N - 2] = np.nan
        e = ne.expect(old, new, st, tg, v0=v0)
        gap = np.abs(e["impact"].sum(axis=1) - (e["yhat"][2] - e["yhat"][1])).max()
        with capsys.disabled():
            print(f"\n{shape}: |y_new - y_rev - sum w I| = {edge:.1e} edge-shaped, {gap:.1e} with one interior gap "
                  f"(largest |y_new - y_rev| {np.abs(e['yhat'][2] - e['yhat'][1]).max():.1e})")


# ---------------------------------------------------------------------------------------------------- (f) marshalling
B, T, N, r, p, q = 2, 12, 6, 2, 2, 1
HANDLE = 0xD0F1
TARGETS = [(11, 0), (13, 5), (4, 2)]
INPUTS = ("old", "new", "Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


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
    a = dict(old=g.standard_normal((B, T, N)), new=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)),
             sig2=g.random((B, N)) + 1, rho=0.3 * g.standard_normal((B, N, q)), Avar=g.standard_normal((B, r, r * p)),
             Q=g.standard_normal((B, r, r)), mu0=g.standard_normal((B, k)), P0=g.standard_normal((B, k, k)), v0=g.random((B, N)) + 1,
             mean=g.standard_normal((B, N)), sd=g.random((B, N)) + 1)
    a["old"][:, 10:, :3] = np.nan
    a["new"][1, 11, 2] = np.nan
    return a


def _addr(a):
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _val(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


@pytest.mark.parametrize("side", ["host", "dev"])
@pytest.mark.parametrize("opts", [dict(), dict(v0=False), dict(scaled=False), dict(want_news=False), dict(want_weight=False),
                                  dict(missing=False), dict(missing=True)])
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
    for k in ("want_news", "want_weight"):
        if k in opts:
            kw[k] = opts[k]
    if "missing" in opts:
        kw["may_have_missing"] = opts["missing"]
    fn = ctx.news_ar_batch_host if side == "host" else ctx.news_ar_batch_dev
    out = fn(*[a[k] for k in INPUTS], TARGETS, **kw)
    name = "dfm_news_ar_batch" + ("" if side == "host" else "_dev")
    assert [c[0] for c in ctx._lib.calls] == [name]
    args = ctx._lib.calls[0][1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds) == 27
    for x, kind in zip(args, kinds):
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int
        else:
            assert x is None or isinstance(x, ctypes.c_void_p)
    assert _val(args[0]) == HANDLE and args[1:7] == (B, T, N, r, p, q)
    for i, k in enumerate(INPUTS):
        assert _val(args[7 + i]) == _addr(a[k]), k
    assert _val(args[16]) == (_addr(a["v0"]) if "v0" in kw else None)
    assert _val(args[17]) == (_addr(a["mean"]) if "mean" in kw else None) and _val(args[18]) == (_addr(a["sd"]) if "sd" in kw else None)
    assert args[19] == len(TARGETS)
    tt = np.ctypeslib.as_array(ctypes.cast(args[20], ctypes.POINTER(ctypes.c_int32)), (len(TARGETS),))
    ti = np.ctypeslib.as_array(ctypes.cast(args[21], ctypes.POINTER(ctypes.c_int32)), (len(TARGETS),))
    assert list(zip(tt.tolist(), ti.tolist())) == TARGETS                                # panel rows, as given
    G = len(TARGETS)
    shapes = dict(yhat=(B, 3, G), impact=(B, G, N), news=(B, T - q, N), weight=(B, G, T - q, N))
    for i, k in enumerate(("yhat", "impact", "news", "weight")):
        if kw.get("want_" + k, True):
            assert type(out[k]) is (np.ndarray if side == "host" else torch.Tensor) and tuple(out[k].shape) == shapes[k], k
            assert str(out[k].dtype).endswith("float64") and _val(args[22 + i]) == _addr(out[k]), k
        else:
            assert out[k] is None and args[22 + i] is None, k
    assert args[26] == (0 if opts.get("missing") is False else _lib.DFM_F_MAY_HAVE_MISSING)


def test_binding_argument_errors():
    ctx = _make_ctx()
    a = _arrays()
    args = [a[k] for k in INPUTS]
    with pytest.raises(ValueError):
        ctx.news_ar_batch_host(*args, TARGETS, mean=a["mean"])
    with pytest.raises(ValueError):
        ctx.news_ar_batch_host(*args, [])
    with pytest.raises(ValueError):                                                    # a target in the conditioning rows
        ctx.news_ar_batch_host(*args, [(0, 1)])
    with pytest.raises(ValueError):
        ctx.news_ar_batch_host(*args, [(5, N)])
    with pytest.raises(ValueError):                                                    # q = 0 is news_batch's model
        ctx.news_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 0)) for k in INPUTS], TARGETS)
    with pytest.raises(ValueError):
        ctx.news_ar_batch_host(*[a[k] if k != "rho" else np.zeros((B, N, 5)) for k in INPUTS], TARGETS)
    with pytest.raises(ValueError):                                                    # T <= 2q
        ctx.news_ar_batch_host(a["old"][:, :2], a["new"][:, :2], *args[2:], [(1, 0)])
    with pytest.raises(ValueError):                                                    # old and new differ in shape
        ctx.news_ar_batch_host(a["old"][:, :-1], *args[1:], TARGETS)
    with pytest.raises(ValueError):                                                    # the device side checks shapes
        ctx.news_ar_batch_dev(*[torch.from_numpy(v) for v in args], TARGETS, v0=torch.from_numpy(a["v0"][:, :-1].copy()))
    assert ctx._lib.calls == []


def test_the_symbols_are_declared_once_everywhere():
    hdr = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    for name in ("dfm_news_ar_batch", "dfm_news_ar_batch_dev"):
        assert name in _lib.SYMBOLS and hdr.count(f"int {name}(") == 1
        assert len(_lib.SYMBOLS[name][1]) == 27
    assert jl.count(":dfm_news_ar_batch,") == 1 and "function news_ar(" in jl
    src = open(kalman.__file__).read()
    assert "dfm_news_ar" not in src and "news_ar" in src
    build = open(os.path.join(ROOT, "dynamic_factor_models_amd", "build.py")).read()
    assert build.count('"news_ar.hip"') == 1


# ---------------------------------------------------------------------------------------------------- api.news_ar_idio
def _model(n_uarlag=2):
    g = np.random.default_rng(3)
    m = api.DFMModel(g.standard_normal((60, 8)), np.ones(8, dtype=int), 20, 3, 1, 50, 0, 2, 1e-8, n_uarlag, 1)
    rr, pp, Nn = m.nfac_u, m.factor_var_model.nlag, m.data.shape[1]
    m.factor[:] = g.standard_normal(m.factor.shape)
    m.lambda_[:] = g.standard_normal((Nn, rr))
    m.uar_coef[:] = 0.2 * g.standard_normal((Nn, n_uarlag))
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
    before = {k: getattr(m, k).copy() for k in ("data", "lambda_", "uar_coef", "uar_ser", "factor")}
    old = m.data[:55].copy()
    old[53:, :4] = np.nan
    tg = [(0, 55), (5, 57)]
    with pytest.raises(ValueError, match="at least one target"):
        api.news_ar_idio(m, old, 55, [], ctx=NoDevice())
    with pytest.raises(ValueError, match="conditioning"):
        api.news_ar_idio(m, old, 55, [(0, m.initperiod + 1)], ctx=NoDevice())
    with pytest.raises(ValueError, match="target column"):
        api.news_ar_idio(m, old, 55, [(8, 55)], ctx=NoDevice())
    with pytest.raises(ValueError, match="groups"):
        api.news_ar_idio(m, old, 55, tg, groups={"g": [9]}, ctx=NoDevice())
    with pytest.raises(ValueError, match="through"):
        api.news_ar_idio(m, old, 61, tg, ctx=NoDevice())
    with pytest.raises(ValueError, match="params"):
        api.news_ar_idio(m, old, 55, tg, quantiles=[0.5], ctx=NoDevice())
    with pytest.raises(ValueError, match="params lacks"):
        api.news_ar_idio(m, old, 55, tg, params={"Lam": 0}, ctx=NoDevice())
    gap = old.copy()
    gap[30, 6] = np.nan
    new = m.data[:55].copy()
    new[30, 6] = np.nan
    with pytest.raises(ValueError, match=r"column 6 .*interior gap.*condition 1"):
        api.news_ar_idio(m, gap, new, tg, ctx=NoDevice())
    new = m.data[:55].copy()
    new[50:, 6] = np.nan                                                               # edge-shaped, but old has cells there
    with pytest.raises(ValueError, match=r"column 6 .*condition 3"):
        api.news_ar_idio(m, old, new, tg, ctx=NoDevice())
    short = old.copy()
    short[3:, 2] = np.nan
    with pytest.raises(ValueError, match=r"column 2 .*condition 2"):
        api.news_ar_idio(m, short, 55, tg, ctx=NoDevice())
    with pytest.raises(ValueError, match="n_uarlag"):
        api.news_ar_idio(_model(5), old, 55, tg, ctx=NoDevice())
    for k, v in before.items():
        assert np.array_equal(getattr(m, k), v, equal_nan=True), k
    m.uar_coef[:] = 0.3
    m.em_params = dict(Lam=np.zeros((8, 2)), R=np.ones(8), A=np.eye(2), Q=np.eye(2), mu0=np.zeros(2), P0=np.eye(2))
    with pytest.raises(ValueError, match="news_ar_idio"):                              # api.news points to the call for this model
        api.news(m, 50, 55, tg, ctx=NoDevice())
