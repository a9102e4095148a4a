"""GPU tests of dfm_news_ar_batch (include/dfm_hip.h; csrc/news_ar.hip) against the expectation model of tests/news_ar_expect.py (the
AR forecast's expectation model for the three conditional means, the oracle's pass over the structured covariance panels for the
weights) at 1e-9, at the smallest shapes that reach every class: q = 1 .. 4, p below / at / above q + 1, every width bucket of the
recursion kernel (k <= 8, 16, 32) and of the loadings (r <= 4, 8, 16), N = 1 / 64 / 65 / 257, T = 2q + 1, a sample that straddles
the 32-row chunk with targets at the chunk's edges and 41 rows into the horizon; then the output invariants, NULL outputs, the
device entry, a call across the 8192-replicate slice boundary, the status codes, and api.news_ar_idio on the Stock-Watson panel."""
import os

import numpy as np
import pytest

from tests import news_ar_expect as ne

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ne.KEYS


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
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _edges(N, T, q, b):
    """(L_old, L_new) of replicate b: series 0 has L = 2q - 1 in old, series 1 an edge deeper than q, series 2 an edge of one cell,
    series 3 no news; the others take these four in turn, shifted by b."""
    Lo, Ln = np.full(N, T - 1), np.full(N, T - 1)
    deep = max(2 * q - 1, T - q - 3)
    for i in range(N):
        kind = (i + (b if i >= 4 else 0)) % 4
        if kind == 0:
            Lo[i], Ln[i] = 2 * q - 1, T - 1 - (i % 2)
        elif kind == 1:
            Lo[i] = deep
        elif kind == 2:
            Lo[i] = T - 2
        else:
            Lo[i] = Ln[i] = T - 1 - (i % 3 == 0)
    return Lo, np.maximum(Ln, Lo)


def _case(B, N, T, r, p, q, seed=0):
    olds, news, sts, v0s = [], [], [], []
    for b in range(B):
        x, st, v0 = ne.synth(b + 1 + seed, N, T, r, p, q)
        Lo, Ln = _edges(N, T, q, b)
        old, new = ne.vintages(x, Lo, Ln, [(q + 1 if T > q + 1 else q, N // 2, 0.06), (0, 0, -0.1)])
        olds.append(old); news.append(new); sts.append(st); v0s.append(v0)
    rng = np.random.default_rng([9, N, T, q])
    return dict(old=np.stack(olds), new=np.stack(news), st={k: np.stack([s[k] for s in sts]) for k in KEYS}, v0=np.stack(v0s),
                mean=rng.standard_normal((B, N)), sd=rng.uniform(0.5, 2.0, (B, N)))


def _run(ctx, c, targets, scaled, v0, what):
    kw = dict(mean=c["mean"], sd=c["sd"]) if scaled else {}
    if v0:
        kw["v0"] = c["v0"]
    got = ctx.news_ar_batch_host(c["old"], c["new"], *[c["st"][k] for k in KEYS], targets, **kw)
    B, T, N = c["new"].shape
    q = c["st"]["rho"].shape[2]
    for b in range(B):
        e = ne.expect(c["old"][b], c["new"][b], {k: c["st"][k][b] for k in KEYS}, targets, v0=c["v0"][b] if v0 else None,
                      mean=c["mean"][b] if scaled else None, sd=c["sd"][b] if scaled else None)
        for key in ("yhat", "impact", "news", "weight"):
            _close(got[key][b], e[key], f"{what} b={b} {key}")
        assert np.all(got["news"][b][~e["cells"]] == 0.0), f"{what}: news off the news cells"
    y = got["yhat"]
    assert np.all(np.abs(got["impact"].sum(axis=2) - (y[:, 2] - y[:, 1])) <= 1e-9 * np.maximum(1.0, np.abs(y[:, 2]))), f"{what}: sum of impacts"
    off = np.broadcast_to(np.isnan(c["new"][:, q:])[:, None], got["weight"].shape)
    assert np.all(got["weight"][off] == 0.0), f"{what}: weight off Omega_new"
    return got


# name -> B, N, T, r, p, q, targets (panel rows), scaled, v0
CASES = {
    "q1_r1_n1_p_below": (1, 1, 40, 1, 1, 1, [(41, 0)], False, False),
    "q2_n64_p_at_b3_g5": (3, 64, 40, 2, 3, 2, [(39, 0), (41, 1), (5, 2), (40, 63), (38, 1)], True, True),
    "q3_r8_k32_n65_chunk_edges_h41": (1, 65, 43, 8, 1, 3, [(3, 5), (34, 0), (35, 64), (42, 2), (43, 1), (83, 3)], True, False),
    "q4_p_above_n257_two_blocks": (1, 257, 24, 1, 6, 4, [(24, 256)], False, True),
    "q4_t_min_k16_b3_g5": (3, 4, 9, 2, 1, 4, [(8, 0), (8, 1), (9, 2), (10, 3), (4, 1)], True, True),
    "q1_r10_k32_rb16": (1, 6, 20, 10, 1, 1, [(19, 0), (21, 4)], False, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_expectation_model(ctx, name):
    B, N, T, r, p, q, targets, scaled, v0 = CASES[name]
    _run(ctx, _case(B, N, T, r, p, q), targets, scaled, v0, name)


def test_null_outputs_device_entry_and_no_news(ctx):
    import torch
    c = _case(2, 64, 30, 2, 2, 2, seed=5)
    tg = [(29, 0), (31, 3)]
    par = [c["st"][k] for k in KEYS]
    full = ctx.news_ar_batch_host(c["old"], c["new"], *par, tg, v0=c["v0"], mean=c["mean"], sd=c["sd"])
    for kw in (dict(want_news=False), dict(want_weight=False), dict(want_news=False, want_weight=False)):
        lean = ctx.news_ar_batch_host(c["old"], c["new"], *par, tg, v0=c["v0"], mean=c["mean"], sd=c["sd"], **kw)
        for key in full:
            if (key == "news" and not kw.get("want_news", True)) or (key == "weight" and not kw.get("want_weight", True)):
                assert lean[key] is None
            else:
                assert np.array_equal(lean[key], full[key]), (kw, key)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.news_ar_batch_dev(t(c["old"]), t(c["new"]), *[t(a) for a in par], tg, v0=t(c["v0"]), mean=t(c["mean"]), sd=t(c["sd"]))
    ctx.synchronize()
    for key in full:
        assert np.array_equal(got[key].cpu().numpy(), full[key]), key
    rev = np.where(np.isnan(c["old"]), np.nan, c["new"])          # no news: impacts exactly 0, y_new = y_rev
    o = ctx.news_ar_batch_host(c["old"], rev, *par, tg)
    assert np.all(o["impact"] == 0.0) and np.all(o["news"] == 0.0)
    assert np.array_equal(o["yhat"][:, 1], o["yhat"][:, 2])


def test_slices_of_8192(ctx):
    """16384 pass replicates: the second slice starts at replicate 2.  The same replicates in two calls of one slice each."""
    B, N, T, r, p, q, G = 4, 4, 12, 2, 1, 1, 4096
    c = _case(B, N, T, r, p, q, seed=9)
    targets = ([(t, i) for t in range(q, T + 2) for i in range(N)] * 80)[:G]
    par = [c["st"][k] for k in KEYS]
    got = ctx.news_ar_batch_host(c["old"], c["new"], *par, targets, v0=c["v0"])
    for b0 in (0, 2):
        s = slice(b0, b0 + 2)
        part = ctx.news_ar_batch_host(c["old"][s], c["new"][s], *[a[s] for a in par], targets, v0=c["v0"][s])
        for key in got:
            assert np.array_equal(got[key][s], part[key]), (b0, key)
    gs = [0, 51, 4095]
    e = ne.expect(c["old"][3], c["new"][3], {k: c["st"][k][3] for k in KEYS}, [targets[g] for g in gs], v0=c["v0"][3])
    for j, g in enumerate(gs):
        _close(got["weight"][3, g], e["weight"][j], f"slices g={g} weight")
        _close(got["impact"][3, g], e["impact"][j], f"slices g={g} impact")
        _close(got["yhat"][3, :, g], e["yhat"][:, j], f"slices g={g} yhat")


def test_status_codes(ctx):
    import ctypes
    import torch
    from dynamic_factor_models_amd import _lib
    B, N, T, r, p, q = 1, 6, 16, 2, 1, 2
    c = _case(B, N, T, r, p, q, seed=3)
    old, new, st = c["old"], c["new"], c["st"]
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    y, imp = np.empty((1, 3, 1)), np.empty((1, 1, N))

    def call(G, t, i, q_=q, T_=T, rho=st["rho"], yo=y, mean=None, lam=st["Lam"]):
        tt, ti = np.array([t], np.int32), np.array([i], np.int32)
        args = [ptr(np.ascontiguousarray(a)) for a in (lam, st["sig2"], rho, st["Avar"], st["Q"], st["mu0"], st["P0"])]
        return ctx._lib.dfm_news_ar_batch(ctx._h, 1, T_, N, lam.shape[2], p, q_, ptr(old), ptr(new), *args, None, mean, None, G, ptr(tt),
                                          ptr(ti), None if yo is None else ptr(yo), ptr(imp), None, None, 1)
    assert call(1, T + 1, 0) == 0
    assert call(0, T - 1, 0) == -1                            # G < 1: DFM_E_DIMS
    assert call(1, q - 1, 0) == -1                            # a target in the conditioning rows
    assert call(1, T - 1, N) == -1                            # target column outside [0, N)
    assert call(1, T - 1, 0, q_=0) == -1                      # q < 1
    assert call(1, T - 1, 0, T_=2 * q) == -1                  # T <= 2q
    assert call(1, T - 1, 0, q_=5, rho=np.zeros((1, N, 5))) == -2          # q > 4: DFM_E_R_UNSUPPORTED
    wide = np.zeros((1, N, 12))
    assert call(1, T - 1, 0, lam=wide) == -2                  # r (q + 1) = 36 > 32: what ar_check refuses
    assert call(1, T - 1, 0, yo=None) == -3                   # yhat NULL: DFM_E_NULL
    assert call(1, T - 1, 0, mean=ptr(st["sig2"])) == -3      # mean without sd

    # DFM_E_VINTAGE from the device status word: the _dev entry, then dfm_check_status
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    par = [t(st[k]) for k in KEYS]

    def vintage_status(o, n):
        ctx.news_ar_batch_dev(t(o), t(n), *par, [(T - 1, 0)], may_have_missing=True)
        try:
            ctx.check_status()
        except _lib.DfmError as e:
            return e.code
        return 0
    assert vintage_status(old, new) == 0
    o2 = old.copy(); o2[0, 2 * q - 1:, 1] = np.nan            # L = 2q - 2 in old
    assert vintage_status(o2, new) == -8
    o2 = old.copy(); n2 = new.copy(); o2[0, 6, 1] = np.nan; n2[0, 6, 1] = np.nan   # an interior gap in both
    assert vintage_status(o2, n2) == -8
    n2 = new.copy(); n2[0, 6, 1] = np.nan; o2 = old.copy(); o2[0, 6:, 1] = np.nan   # an interior gap in new only
    assert vintage_status(o2, n2) == -8
    o2 = old.copy(); n2 = new.copy(); o2[0, 0, 2] = np.nan; n2[0, 0, 2] = np.nan   # a late start
    assert vintage_status(o2, n2) == -8
    o2 = old.copy(); n2 = new.copy(); o2[0, :, 3] = np.nan; n2[0, :, 3] = np.nan   # a never-observed series
    assert vintage_status(o2, n2) == -8
    n2 = new.copy(); n2[0, T - 3:, 3] = np.nan                # a cell of old (series 3 is complete there) missing in new
    assert not np.isnan(old[0, T - 3, 3])
    assert vintage_status(old, n2) == -8
    assert vintage_status(old, new) == 0                      # the bit was reported once


def _sw_model():
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    full = np.flatnonzero((d["inclcode"] == 1) & ~np.isnan(d["bpdata"][2:222]).any(axis=0))   # complete over rows 3 .. 222
    keep = np.zeros_like(d["inclcode"])
    keep[full[:40]] = 1
    return api.DFMModel(d["bpdata"], keep, 20, 40, 3, 216, 0, 4, 1e-8, 2, 1)


def test_stock_watson_news_ar(ctx):
    from dynamic_factor_models_amd import api
    m = _sw_model()
    api.estimate(m, api.NonParametric(), ctx=ctx)
    api.estimate_ar_idio(m, max_em_iter=3, ctx=ctx)
    draws = api.estimate_bayesian_ar_idio(m, 3, chains=2, burn=4, seed=5, ctx=ctx)
    before = {k: getattr(m, k).copy() for k in ("lambda_", "uar_coef", "uar_ser", "factor")}
    cols = api._ar_model_inputs(m)[1]
    old = m.data[:222].copy()
    old[220:, cols[::2]] = np.nan                              # a two-row ragged edge that the new vintage fills
    tg = [(int(cols[0]), 222), (int(cols[3]), 224)]
    groups = {"first": cols[:20], "rest": cols[20:]}
    o = api.news_ar_idio(m, old, 222, tg, groups=groups, params=draws["params"], quantiles=[0.1, 0.5, 0.9], ctx=ctx)
    assert all(np.array_equal(before[k], getattr(m, k), equal_nan=True) for k in before), "news_ar_idio changed m"
    q = m.n_uarlag
    assert np.array_equal(o["rows"], np.arange(m.initperiod + q, 223)) and np.array_equal(o["cols"], cols)
    _close(o["impact"].sum(axis=1), o["news_effect"], "sum of impacts")
    _close(o["groups"]["first"] + o["groups"]["rest"], o["news_effect"], "groups")
    assert o["impact_bands"].shape == (3, 2, cols.size) and o["revision_bands"].shape == (3, 2)
    assert np.all(o["impact_bands"][0] <= o["impact_bands"][2]) and np.all(o["revision_bands"][0] <= o["revision_bands"][2])
    assert np.all(o["news"][:-2] == 0.0) and np.any(o["news"][-2:] != 0.0), "news outside the released rows"
    i = o["inputs"]
    e = ne.expect(i["old"], i["new"], {k: i[k] for k in KEYS}, i["targets"], v0=i["v0"], mean=i["mean"], sd=i["sd"])
    _close(np.stack([o["y_old"], o["y_rev"], o["y_new"]]), e["yhat"], "SW yhat")
    for key in ("impact", "news", "weight"):
        _close(o[key], e[key], f"SW {key}")
