"""GPU tests of dfm_filter_ar_batch (include/dfm_hip.h; csrc/filter_ar.hip) against the expectation model of
tests/filter_ar_expect.py at the project's 1e-9 x max(1, scale), NaN positions and counts exactly: the case table of
filter_ar_expect.CASES, one panel of missing patterns, kernels this entry does not share (the AR pass, dfm_filter_batch at rho = 0,
dfm_forecast_ar_batch on a truncated panel), every optional output left out in turn, the two entries, repeated calls, the status
codes, a failed replicate, and the two api functions on the Stock-Watson panel.  The table of tests/ar_post_geometry.py
(tests/test_gpu_ar_post_geometry.py) adds r > 8, state widths that are no power of two, every reachable instance of the fill and of the
evaluation, and 64 and 65 evaluation origins."""
import ctypes
import os

import numpy as np
import pytest

from tests import filter_ar_expect as fe

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = fe.KEYS
B = 2


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN positions differ"
    ok = ~np.isnan(b)
    if not ok.any():
        return
    scale = max(1.0, float(np.abs(b[ok]).max()))
    err = float(np.abs(a[ok] - b[ok]).max())
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _compare(got, x, st, H, t0, mean, sd, what):
    for b in range(x.shape[0]):
        e = fe.expect_case(x, st, b, H, t0, mean, sd)
        for n, v in e.items():
            if n == "cnt":
                assert np.array_equal(got[n][b], v), f"{what} b={b} cnt"
            else:
                _close(got[n][b], v, f"{what} b={b} {n}")
    if H == 0:
        assert all(got[n] is None for n in ("msfe", "msfe_common", "msfe0", "cnt"))


def _run_dev_misaligned(ctx, x, st, H, t0, mean, sd, flags):
    """The _dev entry with every panel-sized output 8 bytes past a 16-byte boundary (the scalar path of the fill)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Bn, T, N = x.shape
    r, q = st["Lam"].shape[2], st["rho"].shape[2]
    k = st["mu0"].shape[1]
    kk = k * (k + 1) // 2
    n = T - q
    ins = [t(x)] + [t(st[name]) for name in KEYS] + [t(mean), t(sd)]
    cells = [torch.empty(Bn * n * N + 1, dtype=torch.float64, device=dev) for _ in range(3)]
    mom = dict(z_pred=(Bn, n, k), P_pred=(Bn, n, kk), z_filt=(Bn, n, k), P_filt=(Bn, n, kk), loglik_t=(Bn, n))
    mo = {name: torch.empty(s, dtype=torch.float64, device=dev) for name, s in mom.items()}
    ev = [torch.empty((Bn, H, N), dtype=torch.float64, device=dev) for _ in range(3)]
    cn = torch.empty((Bn, H, N), dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())
    ctx._sync_stream()
    rc = ctx._lib.dfm_filter_ar_batch_dev(ctx._h, Bn, T, N, r, st["Avar"].shape[2] // r, q, H, t0, *[p(a) for a in ins],
                                          *[p(mo[name]) for name in mom], *[ctypes.c_void_p(c.data_ptr() + 8) for c in cells],
                                          p(ev[0]), p(ev[1]), p(ev[2]), p(cn), flags)
    assert rc == 0
    ctx.synchronize()
    out = {name: v.cpu().numpy() for name, v in mo.items()}
    for name, c in zip(("xpred", "verr", "vstd"), cells):
        out[name] = c[1:].reshape(Bn, n, N).cpu().numpy()
    out.update(msfe=ev[0].cpu().numpy(), msfe_common=ev[1].cpu().numpy(), msfe0=ev[2].cpu().numpy(), cnt=cn.cpu().numpy())
    return out


def _host(ctx, x, st, **kw):
    return ctx.filter_ar_batch_host(x, *[st[k] for k in KEYS], **kw)


# ------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("row", fe.CASES, ids=[c[0] for c in fe.CASES])
def test_outputs_against_the_model(ctx, row):
    c, x, st, mean, sd = fe.make_case(row)
    miss = bool(np.isnan(x).any())
    if c["aligned"]:
        got = _host(ctx, x, st, H=c["H"], t0=c["t0"], mean=mean, sd=sd, may_have_missing=miss)
    else:
        got = _run_dev_misaligned(ctx, x, st, c["H"], c["t0"], mean, sd, 1 if miss else 0)
    _compare(got, x, st, c["H"], c["t0"], mean, sd, c["name"])
    if c["H"] > 0 and c["H"] >= c["T"] - c["t0"]:            # horizons without an origin: NaN, count 0
        h0 = max(c["T"] - 1 - c["t0"], 0)
        assert np.all(got["cnt"][:, h0:] == 0)
        for name in ("msfe", "msfe_common", "msfe0"):
            assert np.all(np.isnan(got[name][:, h0:]))
    if c["missing"] == 0.0 and c["H"] > 0 and c["T"] - 1 - c["t0"] >= 1:
        assert np.all(got["cnt"][:, 0] == c["T"] - 1 - c["t0"])


# ------------------------------------------------------------------------------------------------------------ missing patterns
def test_missing_patterns(ctx):
    N, T, r, p, q, H, t0 = 24, 40, 2, 2, 2, 4, 8
    x, st = fe.params_for(B, N, T, r, p, q)
    g = np.random.default_rng(23)
    x[:, :, 8:][g.random((B, T, N - 8)) < 0.08] = np.nan      # scattered cells beside the pattern's series 0 .. 5
    fe.missing_pattern(x, q)
    mean, sd = fe.scales(B, N, True)
    got = _host(ctx, x, st, H=H, t0=t0, mean=mean, sd=sd)
    _compare(got, x, st, H, t0, mean, sd, "missing patterns")
    row = 4 * q + 10                                          # the row with no observed cell empties q + 1 quasi-differenced rows
    for t in range(row - q, row + 1):
        assert np.array_equal(got["z_filt"][:, t], got["z_pred"][:, t]) and np.array_equal(got["P_filt"][:, t], got["P_pred"][:, t])
        assert np.all(got["loglik_t"][:, t] == 0.0) and np.all(np.isnan(got["verr"][:, t]))
    assert np.all(got["cnt"][:, :, 4] == 0) and np.all(np.isnan(got["msfe"][:, :, 4])) and np.all(np.isnan(got["xpred"][:, :, 4]))
    assert np.all(got["cnt"][:, :, [0, 1, 2, 3, 5]] > 0)
    assert np.all(np.isnan(got["xpred"][:, 0, 5])) and not np.isnan(got["xpred"][:, 1, 5]).any()      # the missing cell in panel row 0
    assert not np.isnan(got["xpred"][:, 4, 0]).any() and np.isnan(got["verr"][:, 4, 0]).all()         # x_ti missing, its lags observed


def test_two_calls_are_bit_identical(ctx):
    x, st = fe.params_for(B, 130, 150, 2, 2, 2, missing=0.1)
    want = ("msfe", "msfe_common", "msfe0", "cnt", "loglik_t", "vstd")
    a = _host(ctx, x, st, H=5, t0=10, want=want)
    b = _host(ctx, x, st, H=5, t0=10, want=want)
    for n in want:
        assert np.array_equal(a[n], b[n], equal_nan=True), n
    assert np.any(a["cnt"] > 64), "more than one origin chunk was meant to be summed"


# ------------------------------------------------------------------------------------------------------------ other kernels
@pytest.mark.parametrize("r,p,q,missing", [(2, 1, 1, 0.0), (2, 3, 2, 0.1), (4, 4, 4, 0.1), (8, 2, 3, 0.0)],
                         ids=["q1_balanced", "q2_missing", "q4_missing", "k32_balanced"])
def test_loglik_against_the_ar_pass_on_the_gpu(ctx, r, p, q, missing):
    N, T = 40, 60
    x, st = fe.params_for(B, N, T, r, p, q, missing=missing)
    got = _host(ctx, x, st, want=("z_filt", "P_filt", "loglik_t"))
    f, Ps, ll = ctx.ks_pass_ar_batch_host(x, *[st[k] for k in KEYS])
    _close(got["loglik_t"].sum(axis=1), ll, "sum of loglik_t against the AR pass")
    _close(got["z_filt"][:, -1, :r], f[:, -1], "last filtered mean against the last smoothed mean")
    _close(got["P_filt"][:, -1, :r * (r + 1) // 2], Ps[:, -1], "last filtered covariance against the last smoothed one")


def test_rho_zero_is_the_plain_filter(ctx):
    """Balanced, rho = 0, q = 1, p = 2: the same state width (k = 2 r), so everything equals dfm_filter_batch on panel rows 1 .. T-1
    with the same mu0 / P0, and the idiosyncratic term buys nothing: msfe_common = msfe."""
    N, T, r, p, q, H, t0 = 30, 40, 3, 2, 1, 4, 12
    x, st = fe.params_for(B, N, T, r, p, q)
    st = dict(st, rho=np.zeros_like(st["rho"]))
    mean, sd = fe.scales(B, N, True)
    got = _host(ctx, x, st, H=H, t0=t0, mean=mean, sd=sd)
    ref = ctx.filter_batch_host(np.ascontiguousarray(x[:, 1:]), st["Lam"], st["sig2"], st["Avar"], st["Q"], st["mu0"], st["P0"], H=H,
                                t0=t0 - 1, mean=mean, sd=sd)
    for n in ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t", "xpred", "verr", "vstd", "msfe", "msfe0"):
        _close(got[n], ref[n], f"rho = 0 against dfm_filter_batch: {n}")
    assert np.array_equal(got["cnt"], ref["cnt"]) and np.all(got["cnt"] > 0)
    _close(got["msfe_common"], got["msfe"], "rho = 0: msfe_common against msfe")


def test_single_origin_against_forecast_ar(ctx):
    """Balanced, t0 = T-1-H: horizon H has the single origin T-1-H, so msfe[H-1] = (x_{T-1,i} - xhat)^2 with xhat the last horizon
    row of dfm_forecast_ar_batch on the first T - H rows (v0 does not reach a balanced panel's horizon)."""
    N, T, r, p, q, H = 30, 40, 2, 2, 2, 3
    x, st = fe.params_for(B, N, T, r, p, q)
    got = _host(ctx, x, st, H=H, t0=T - 1 - H, want=("msfe", "cnt"))
    fc = ctx.forecast_ar_batch_host(np.ascontiguousarray(x[:, :T - H]), *[st[k] for k in KEYS], H, want=())
    assert np.all(got["cnt"][:, H - 1] == 1)
    _close(got["msfe"][:, H - 1], (x[:, T - 1] - fc["xhat"][:, -1]) ** 2, "single origin against dfm_forecast_ar_batch")


# ------------------------------------------------------------------------------------------------------------ outputs, entries
def test_every_optional_output_left_out_in_turn(ctx):
    N, T, r, p, q, H, t0 = 30, 24, 2, 1, 2, 3, 6
    x, st = fe.params_for(B, N, T, r, p, q, missing=0.1)
    mean, sd = fe.scales(B, N, True)
    full = _host(ctx, x, st, H=H, t0=t0, mean=mean, sd=sd)
    for drop in fe.OUTPUTS:
        want = tuple(n for n in fe.OUTPUTS if n != drop)
        got = _host(ctx, x, st, H=H, t0=t0, mean=mean, sd=sd, want=want)
        assert got[drop] is None
        for n in want:
            assert np.array_equal(got[n], full[n], equal_nan=True), (drop, n)
    for only in fe.OUTPUTS:
        got = _host(ctx, x, st, H=H, t0=t0, mean=mean, sd=sd, want=(only,))
        assert np.array_equal(got[only], full[only], equal_nan=True), only


def test_dev_and_host_entries_agree(ctx):
    import torch
    x, st = fe.params_for(B, 60, 40, 2, 3, 2, missing=0.1)
    mean, sd = fe.scales(B, 60, True)
    host = _host(ctx, x, st, H=4, t0=7, mean=mean, sd=sd)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.filter_ar_batch_dev(t(x), *[t(st[k]) for k in KEYS], H=4, t0=7, mean=t(mean), sd=t(sd))
    ctx.synchronize()
    for n in host:
        assert np.array_equal(got[n].cpu().numpy(), host[n], equal_nan=True), n


def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    Bn, T, N, r, p, q = 1, 30, 20, 2, 1, 2
    x, st = fe.params_for(Bn, N, T, r, p, q)
    P = [st[k] for k in KEYS]
    good = lambda: _host(ctx, x, st, H=2, t0=5)
    ptr = lambda a: ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)
    ll = np.full((1, T - q), np.nan)
    base = [ptr(x)] + [ptr(a) for a in P] + [None, None]
    outs = [None] * 4 + [ptr(ll)] + [None] * 7
    lib = ctx._lib
    call = lambda *dims, ins=base: lib.dfm_filter_ar_batch(ctx._h, *dims, *ins, *outs, 0)
    assert call(1, T, N, r, p, q, -1, q) == -1                                                    # H < 0
    good()
    assert call(1, T, N, r, p, 0, 2, 0) == -1                                                     # q < 1
    assert call(1, q, N, r, p, q, 0, q) == -1                                                     # T <= q
    assert call(1, T, N, r, p, q, 2, q - 1) == -1 and call(1, T, N, r, p, q, 2, T) == -1          # t0 outside [q, T)
    good()
    rho5 = np.zeros((1, N, 5))
    ins5 = [ptr(x)] + [ptr(a) if k != "rho" else ptr(rho5) for k, a in zip(KEYS, P)] + [None, None]
    assert call(1, T, N, r, p, 5, 2, 5, ins=ins5) == -2                                           # q > 4
    assert call(1, T, N, 8, 5, q, 2, q) == -2                                                     # r max(p, q + 1) > 32
    assert call(1, T, N, r, p, q, 2, q, ins=[ptr(x)] + [ptr(a) for a in P[:2]] + [None] + [ptr(a) for a in P[3:]] + [None, None]) == -3
    assert call(1, T, N, r, p, q, 2, q, ins=base[:-2] + [ptr(np.zeros((1, N))), None]) == -3      # mean without sd
    good()
    bad = x.copy(); bad[0, 5, 3] = np.nan
    with pytest.raises(_lib.DfmError) as ei:
        _host(ctx, bad, st, may_have_missing=False)
    assert ei.value.code == -4
    ok = good()
    assert np.all(np.isfinite(ok["loglik_t"]))
    assert lib.dfm_filter_ar_batch(ctx._h, 1, T, N, r, p, q, 0, q, *base, *outs, 0) == 0
    assert np.array_equal(ll, ok["loglik_t"])                                                     # H = 0 with every evaluation output NULL


def test_a_failed_replicate_leaves_the_other_untouched(ctx):
    import torch
    from dynamic_factor_models_amd import _lib
    N, T, r, p, q, H, t0 = 20, 30, 2, 1, 2, 2, 5
    x, st = fe.params_for(B, N, T, r, p, q)
    good = _host(ctx, x, st, H=H, t0=t0)
    P0 = st["P0"].copy()
    P0[0] = -100.0 * np.eye(P0.shape[1])                      # not positive semi-definite: the first update fails
    with pytest.raises(_lib.DfmError) as ei:
        _host(ctx, x, dict(st, P0=P0), H=H, t0=t0)
    assert ei.value.code == -5
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bad = dict(st, P0=P0)
    got = ctx.filter_ar_batch_dev(t(x), *[t(bad[k]) for k in KEYS], H=H, t0=t0)
    with pytest.raises(_lib.DfmError) as ei:
        ctx.synchronize()
    assert ei.value.code == -5
    got = {n: v.cpu().numpy() for n, v in got.items()}
    for n in ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t", "xpred", "verr", "vstd"):
        assert np.all(np.isnan(got[n][0])), n                 # NaN from the first period on
        assert np.array_equal(got[n][1], good[n][1], equal_nan=True), n
    for n in ("msfe", "msfe_common", "msfe0", "cnt"):
        assert np.array_equal(got[n][1], good[n][1], equal_nan=True), n
    again = _host(ctx, x, st, H=H, t0=t0)                     # the handle is usable afterwards
    assert np.array_equal(again["loglik_t"], good["loglik_t"])


# ------------------------------------------------------------------------------------------------------------ the api
def test_api_on_the_stock_watson_panel(ctx):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 4)
    api.estimate(m, api.NonParametric(), ctx=ctx)
    keep = (m.lambda_.copy(), m.uar_coef.copy(), m.uar_ser.copy(), m.factor.copy())
    q, r, H, fo = m.n_uarlag, m.nfac_u, 4, 150
    fs = api.filter_states_ar_idio(m, ctx=ctx)
    ev = api.evaluate_forecasts_ar_idio(m, H, first_origin=fo, ctx=ctx)
    inp = fs["inputs"]
    e = fe.expect(inp["x"], *[inp[k] for k in KEYS], H=H, t0=fo - m.initperiod, mean=inp["mean"], sd=np.ones(inp["mean"].size))
    n, N = e["xpred"].shape
    assert np.array_equal(fs["rows"], np.arange(m.initperiod + q, m.lastperiod + 1)) and fs["rows"].size == n
    assert np.array_equal(fs["cols"], ev["cols"]) and fs["cols"].size == N
    _close(fs["state_filt"], e["z_filt"], "api state_filt")
    _close(fs["factor_pred"], e["z_pred"][:, :r] + fs["mu_f"], "api factor_pred")
    _close(fe.pack(fs["factor_filt_cov"]), e["P_filt"][:, :r * (r + 1) // 2], "api factor_filt_cov")
    _close(fs["loglik_t"], e["loglik_t"], "api loglik_t")
    _close(fs["x_pred"], e["xpred"], "api x_pred")
    _close(fs["error"], e["verr"], "api error")
    _close(fs["error_std"], e["vstd"], "api error_std")
    fc = api.forecast_ar_idio(m, 0, ctx=ctx)
    assert abs(fs["loglik"] - fc["loglik"]) <= TOL * max(1.0, abs(fc["loglik"]))
    _close(ev["msfe"], e["msfe"], "api msfe")
    _close(ev["msfe_common"], e["msfe_common"], "api msfe_common")
    _close(ev["gain"], e["msfe"] / e["msfe_common"], "api gain")
    _close(ev["relative"], e["msfe"] / e["msfe0"], "api relative")
    assert np.array_equal(ev["count"], e["cnt"]) and np.all(ev["count"] > 0) and np.all(np.isfinite(ev["gain"]))
    assert np.array_equal(ev["horizons"], np.arange(1, H + 1))
    own = {k: np.stack([inp[k], inp[k]]) for k in KEYS}
    own["sig2"][1] *= 1.2
    own["rho"][1] *= 0.5
    two = api.evaluate_forecasts_ar_idio(m, H, first_origin=fo, params=own, quantiles=[0.25, 1.0], ctx=ctx)
    assert two["msfe"].shape == (H, N) and two["bands"].shape == (2, H, N) and two["gain_bands"].shape == (2, H, N)
    assert np.array_equal(two["msfe"], ev["msfe"]) and np.all(np.diff(two["bands"], axis=0) >= 0.0)
    assert np.array_equal(two["bands"][1], np.maximum(two["bands"][0], two["bands"][1]))
    first = api.evaluate_forecasts_ar_idio(m, 1, ctx=ctx)    # first_origin defaults to the middle of the output rows
    assert first["count"].max() <= n - 1 - n // 2 and first["count"].max() > 0
    for a, b in zip(keep, (m.lambda_, m.uar_coef, m.uar_ser, m.factor)):
        assert np.array_equal(a, b, equal_nan=True), "the api changed the model"
