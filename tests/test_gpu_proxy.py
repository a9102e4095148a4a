"""GPU tests of dfm_proxyirf_batch (include/dfm_hip.h; csrc/proxy.hip) against the expectation model of tests/proxy_expect.py at the
project's 1e-9 x max(1, scale), every slot compared (tests/test_proxy_cpu.py holds the condition that allows it): the case table,
the lane / wave / workgroup edges in D, L = n, a balanced panel, and on the device alone the normalisation, the sign, the unit
effect, the variance-share bound, continuation, determinism, both entries, the optional outputs, a replicate whose Q is not
positive definite, and the api on the Stock-Watson panel."""
import functools
import os

import numpy as np
import pytest

from tests import proxy_expect as px
from tests import structural_expect as se

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = px.KEYS
H = 6


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN in different places"
    scale = max(1.0, float(np.nanmax(np.abs(b))))
    err = float(np.nanmax(np.abs(a - b)))
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _call(ctx, c, D, L=None, first=0, host=True, **kw):
    P = [c["params"][k] for k in KEYS]
    args = dict(draws=D, block=c["L"] if L is None else L, seed=px.SEED, first_draw=first, sd=c["sd"], cum=c["cum"],
                unit_effect=c["unit"], want_fevd=True)
    args.update(kw)
    if host:
        return ctx.proxyirf_batch_host(c["panel"], *P, H, c["z"], c["norm"], **args)
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args["sd"] = t(args["sd"])
    got = ctx.proxyirf_batch(t(c["panel"]), *[t(a) for a in P], H, c["z"], c["norm"], **args)
    return got


def _np(got):
    return {k: None if v is None else (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()}


def _against_the_model(c, got, D, L=None, first=0, what=""):
    """Every output of every slot against the model fed with the call's own f_out, which is held to the oracle's smoother."""
    for b in range(2):
        _close(got["f"][b], c["f"][b], f"{what} b={b} f_out against the oracle")
        assert abs(got["loglik"][b] - c["loglik"][b]) <= TOL * abs(c["loglik"][b])
    e = px.expect(c, H, D, L=L, first=first, f=got["f"])
    for b in range(2):
        for k in ("impact", "rel", "irf", "fevd", "shock"):
            _close(got[k][b], e[b][k], f"{what} b={b} {k}")
    return e


def _on_the_device_alone(ctx, c, got):
    for b in range(2):
        q = {k: c["params"][k][b] for k in KEYS}
        h = got["impact"][b]
        one = np.einsum("sc,sc->s", h, np.linalg.solve(q["Q"], h.T).T)
        assert np.abs(one - 1.0).max() <= 1e-12, "hvec' Q^-1 hvec is not 1"
        first = got["irf"][b][:, 0, c["norm"]]
        assert np.all(first >= 0.0), "the impact response of norm is negative"
        if c["unit"]:
            assert np.all(first == 1.0), "unit effect: the impact response is not exactly 1"
    full = ctx.irf_batch_host(c["params"]["Lam"], c["params"]["A"], c["params"]["Q"], c["params"]["R"], H, cum=c["cum"])["fevd"]
    room = 1.0 - full[:, -1]                                                 # [B, H, N]: what the idiosyncratic slot leaves
    assert np.all(got["fevd"] >= 0.0) and np.all(got["fevd"] <= room[:, None] + 1e-12)


# ------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", [c[0] for c in px.CASES])
def test_case_table_against_the_model(ctx, name):
    c = px.build(name)
    got = _call(ctx, c, px.D_CASE)
    _against_the_model(c, got, px.D_CASE, what=name)
    _on_the_device_alone(ctx, c, got)
    assert np.all(got["shock"][:, :c["p"]] == 0.0)


@functools.lru_cache(maxsize=None)
def _edge_model(f_bytes):
    c = px.build("r3p2")
    f = np.frombuffer(f_bytes).reshape(2, c["T"], c["r"])
    return px.expect(c, H, max(px.D_EDGES), f=f)


@pytest.mark.parametrize("D", px.D_EDGES)
def test_lane_wave_and_workgroup_edges(ctx, D):
    """D + 1 slots with D at 0, 1 and around 64 and 256: the model runs once at the largest D (a draw does not depend on D)."""
    c = px.build("r3p2")
    got = _call(ctx, c, D)
    e = _edge_model(np.ascontiguousarray(got["f"]).tobytes())
    for b in range(2):
        assert got["irf"][b].shape == (D + 1, H, c["N"])
        for k in ("impact", "rel", "irf", "fevd"):
            _close(got[k][b], e[b][k][:D + 1], f"D={D} b={b} {k}")
        _close(got["shock"][b], e[b]["shock"], f"D={D} b={b} shock")


def test_block_length_n(ctx):
    c = px.build("r4p4")
    got = _call(ctx, c, px.D_CASE, L=c["n"])
    _against_the_model(c, got, px.D_CASE, L=c["n"], what="L=n")
    for k in ("impact", "rel", "irf", "fevd"):
        assert np.array_equal(got[k][:, 1:], np.broadcast_to(got[k][:, :1], got[k][:, 1:].shape)), k


def test_balanced_panel(ctx):
    c = px.build("r3p2", missing=0.0)
    assert not np.isnan(c["panel"]).any()
    got = _call(ctx, c, px.D_CASE)
    _against_the_model(c, got, px.D_CASE, what="balanced")


def test_row_table_beyond_lds(ctx):
    """T = 720 at r = 8: the row table (715 rows of 9 doubles) is over 48 KB, so the lanes read it from global memory."""
    c = px.build("r8unit", T=px.T_LONG)
    assert c["n"] * 9 * 8 > 48 * 1024
    got = _call(ctx, c, px.D_CASE)
    _against_the_model(c, got, px.D_CASE, what="long")
    _on_the_device_alone(ctx, c, got)


# ------------------------------------------------------------------------------------------------------------ the device alone
def test_continuation_and_determinism(ctx):
    c = px.build("r4p4")
    whole = _call(ctx, c, 70)
    again = _call(ctx, c, 70)
    for k in whole:
        assert np.array_equal(whole[k], again[k]), f"{k}: two identical calls differ"
    tail = _call(ctx, c, 30, first=40)
    for k in ("impact", "rel", "irf", "fevd"):
        assert np.array_equal(whole[k][:, 41:], tail[k][:, 1:]), f"{k}: draws 40.. of one call are not those of first_draw = 40"
        assert np.array_equal(whole[k][:, 0], tail[k][:, 0]), k


def test_dev_and_host_entries_agree(ctx):
    c = px.build("r3p2")
    host = _call(ctx, c, 65)
    dev = _call(ctx, c, 65, host=False)
    ctx.synchronize()
    dev = _np(dev)
    for k in host:
        assert np.array_equal(dev[k], host[k]), k


def test_optional_outputs_leave_the_others_unchanged(ctx):
    c = px.build("r8unit")
    full = _call(ctx, c, 5)
    no_irf = _call(ctx, c, 5, want_irf=False)
    no_fevd = _call(ctx, c, 5, want_fevd=False, want_shock=False)
    lean = _call(ctx, c, 5, want_irf=False, want_fevd=False)
    assert no_irf["irf"] is None and np.array_equal(no_irf["fevd"], full["fevd"])
    assert no_fevd["fevd"] is None and no_fevd["shock"] is None and np.array_equal(no_fevd["irf"], full["irf"])
    for k in ("impact", "rel"):
        assert np.array_equal(no_irf[k], full[k]) and np.array_equal(no_fevd[k], full[k]) and np.array_equal(lean[k], full[k])
    assert np.array_equal(lean["shock"], full["shock"])


def test_a_replicate_whose_q_is_not_positive_definite(ctx):
    """Replicate 1 gets a rank-deficient Q: status bit 16, DFM_E_NUMERIC from the host entry and from the check after the device
    entry, and replicate 0's outputs as the model has them."""
    from dynamic_factor_models_amd import _lib
    c = dict(px.build("r3p2"))
    params = {k: v.copy() for k, v in c["params"].items()}
    G = np.random.default_rng(4).standard_normal((c["r"], c["r"] - 1))
    params["Q"][1] = G @ G.T
    c["params"] = params
    with pytest.raises(_lib.DfmError) as ei:
        _call(ctx, c, 4, singular_q=True)
    assert ei.value.code == -5
    got = _call(ctx, c, 4, host=False, singular_q=True)
    with pytest.raises(_lib.DfmError) as ei:
        ctx.synchronize()
    assert ei.value.code == -5
    got = _np(got)
    good = px.build("r3p2")
    q = {k: good["params"][k][0] for k in KEYS}
    e = px.run(got["f"][0], q["Lam"], q["R"], q["A"], q["Q"], H, good["z"], good["norm"], 4, good["L"], px.SEED, 0, 0, sd=good["sd"][0],
               cum=good["cum"])
    for k in ("impact", "rel", "irf", "fevd", "shock"):
        _close(got[k][0], e[k], f"beside a non-PD replicate: {k}")
    clean = _call(ctx, good, 4)                                             # and the handle is fine afterwards
    assert np.all(np.isfinite(clean["irf"]))


# ------------------------------------------------------------------------------------------------------------ the api
def test_api_on_the_stock_watson_panel(ctx):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 1)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=1, ctx=ctx, nrep=8, seed=11)
    ep = {k: v.copy() for k, v in m.em_params.items()}
    cols, _, _, sd = api._forecast_inputs(m, m.lastperiod)
    r, N, Hh, D = 4, cols.size, 8, 40
    hd = api.historical_decomposition(m, ctx=ctx)
    g = np.random.default_rng(8)
    inst = np.full(m.data.shape[0], np.nan)
    inst[m.initperiod - 1:m.lastperiod] = hd["shocks"][:, 1] + 0.5 * g.standard_normal(hd["shocks"].shape[0])
    inst[30:36] = np.nan
    inst[m.lastperiod:] = 7.0                                               # outside the window: not used
    norm = int(cols[5])
    qs = np.array([0.1, 0.5, 0.9])
    o = api.structural_irf_proxy(m, Hh, inst, norm=norm, draws=D, cumulate=cols[:20], unit_effect=True, quantiles=qs, seed=9, ctx=ctx)
    assert np.array_equal(o["cols"], cols) and o["irf"].shape == (N, Hh) and o["fevd"].shape == (N, Hh) and o["impact"].shape == (r,)
    assert o["irf"][5, 0] == 1.0 and o["shock"].shape == (214,) and o["shock"][0] == 0.0
    zi = inst[m.initperiod - 1:m.lastperiod]
    n = int(np.isfinite(zi[1:]).sum())
    L = int(np.ceil(n ** (1.0 / 3.0) - 1e-12))
    assert n == 207 and L == 6
    cum = np.zeros(N, int); cum[:20] = 1
    e = px.run(hd["factor"], ep["Lam"], ep["R"], ep["A"], ep["Q"], Hh, zi, 5, D, L, 9, 0, 0, sd=sd, cum=cum, unit=True)
    _close(o["irf"], e["irf"][0].T, "api irf")
    _close(o["fevd"], e["fevd"][0].T, "api fevd")
    _close(o["impact"], e["impact"][0], "api impact")
    _close(o["shock"], e["shock"], "api shock")
    assert abs(o["relevance"] - e["rel"][0]) <= TOL and o["relevance"] > 0.3 and o["first_stage_F"] > 10.0
    assert o["bands"].shape == (3, N, Hh) and np.all(np.isfinite(o["bands"])) and np.all(np.diff(o["bands"], axis=0) >= 0.0)
    srt = np.sort(e["irf"][1:], axis=0)                                     # nearest rank over the D block draws
    _close(o["bands"][1], srt[int(np.ceil(0.5 * D)) - 1].T, "api median band")
    ob = api.structural_irf_proxy(m, Hh, inst, norm=norm, draws=16, cumulate=cols[:20], quantiles=qs, parameter_draws=True, seed=9,
                                  ctx=ctx)
    assert ob["bands"].shape == (3, N, Hh) and np.all(np.isfinite(ob["bands"])) and np.all(np.diff(ob["bands"], axis=0) >= 0.0)
    assert np.abs(ob["bands"]).max() <= 100.0 * max(1.0, np.abs(ob["irf"]).max())
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep), "the api changed m.em_params"
