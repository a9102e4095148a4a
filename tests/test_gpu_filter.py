"""GPU tests of dfm_filter_batch (include/dfm_hip.h; csrc/filter.hip) against the expectation model of tests/filter_expect.py at
the project's 1e-9 x max(1, scale), NaN positions and counts exactly: the case table of filter_expect.CASES (recursion shapes,
cross-sections over the collapse's lane tilings and every launch class of filter_fill_kernel, the evaluation's edges), the
missing patterns, the existing smoother kernels on the GPU itself, the status codes, the two entries and the api on the
Stock-Watson panel."""
import ctypes
import os

import numpy as np
import pytest

from tests import filter_expect as fe

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


def _compare(got, x, st, H, t0, mean, sd, what, names=None):
    for b in range(x.shape[0]):
        e = fe.expect(x[b], *[st[k][b] for k in KEYS], H=H, t0=t0, mean=None if mean is None else mean[b],
                      sd=None if sd is None else sd[b])
        for n, v in e.items():
            if names is not None and n not in names:
                continue
            if n == "cnt":
                assert np.array_equal(got[n][b], v), f"{what} b={b} cnt"
            else:
                _close(got[n][b], v, f"{what} b={b} {n}")
        if H == 0:
            assert got["msfe"] is None and got["msfe0"] is None and got["cnt"] is None


def _scales(N, scaled):
    if not scaled:
        return None, None
    g = np.random.default_rng(3)
    return g.standard_normal((B, N)), g.uniform(0.5, 3.0, (B, N))


def _run_dev_misaligned(ctx, x, st, H, t0, mean, sd, flags):
    """The _dev entry with every panel-sized output 8 bytes past a 16-byte boundary (the scalar path of the fill)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Bn, T, N = x.shape
    r = st["Lam"].shape[2]
    k = st["A"].shape[2]
    kk = k * (k + 1) // 2
    ins = [t(x)] + [t(st[n]) for n in KEYS] + [t(mean), t(sd)]
    cells = [torch.empty(Bn * T * N + 1, dtype=torch.float64, device=dev) for _ in range(3)]
    mom = dict(z_pred=(Bn, T, k), P_pred=(Bn, T, kk), z_filt=(Bn, T, k), P_filt=(Bn, T, kk), loglik_t=(Bn, T))
    mo = {n: torch.empty(s, dtype=torch.float64, device=dev) for n, s in mom.items()}
    ev = [torch.empty((Bn, H, N), dtype=torch.float64, device=dev) for _ in range(2)]
    cn = torch.empty((Bn, H, N), dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())
    ctx._sync_stream()
    rc = ctx._lib.dfm_filter_batch_dev(ctx._h, Bn, T, N, r, k // r, H, t0, *[p(a) for a in ins], *[p(mo[n]) for n in mom],
                                       *[ctypes.c_void_p(c.data_ptr() + 8) for c in cells], p(ev[0]), p(ev[1]), p(cn), flags)
    assert rc == 0
    ctx.synchronize()
    out = {n: v.cpu().numpy() for n, v in mo.items()}
    for n, c in zip(("xpred", "verr", "vstd"), cells):
        out[n] = c[1:].reshape(Bn, T, N).cpu().numpy()
    out.update(msfe=ev[0].cpu().numpy(), msfe0=ev[1].cpu().numpy(), cnt=cn.cpu().numpy())
    return out


# ------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("row", fe.CASES, ids=[c[0] for c in fe.CASES])
def test_outputs_against_the_model(ctx, row):
    c = fe.case_dict(row)
    x, st = fe.params_for(B, c["N"], c["T"], c["r"], c["p"], missing=c["missing"])
    mean, sd = _scales(c["N"], c["scaled"])
    miss = bool(np.isnan(x).any())
    if c["aligned"]:
        got = ctx.filter_batch_host(x, *[st[k] for k in KEYS], H=c["H"], t0=c["t0"], mean=mean, sd=sd, may_have_missing=miss)
    else:
        got = _run_dev_misaligned(ctx, x, st, c["H"], c["t0"], mean, sd, 1 if miss else 0)
    _compare(got, x, st, c["H"], c["t0"], mean, sd, c["name"])
    if c["H"] >= c["T"] - c["t0"] and c["H"] > 0:            # horizons without an origin: NaN, count 0
        h0 = max(c["T"] - 1 - c["t0"], 0)
        assert np.all(got["cnt"][:, h0:] == 0) and np.all(np.isnan(got["msfe"][:, h0:])) and np.all(np.isnan(got["msfe0"][:, h0:]))


def test_large_cross_section_is_refused(ctx):
    x, st = fe.params_for(1, 1025, 4, 8, 1)
    from dynamic_factor_models_amd import _lib
    with pytest.raises(_lib.DfmError) as ei:
        ctx.filter_batch_host(x, *[st[k] for k in KEYS], want=("loglik_t",))
    assert ei.value.code == -1 and "N too large" in str(ei.value)


# ------------------------------------------------------------------------------------------------------------ missing patterns
def test_missing_patterns(ctx):
    N, T, r, p, H, t0 = 24, 30, 3, 2, 4, 12
    x, st = fe.params_for(B, N, T, r, p, missing=0.1)
    x[:, 14, :] = np.nan                                      # an all-missing row in the middle
    x[:, :3, :] = np.nan                                      # three all-missing leading rows
    x[:, :, 5] = np.nan                                       # a series observed nowhere
    x[:, t0 + 1:, 7] = np.nan                                 # a series observed only up to the first origin: no target row
    mean, sd = _scales(N, True)
    got = ctx.filter_batch_host(x, *[st[k] for k in KEYS], H=H, t0=t0, mean=mean, sd=sd)
    _compare(got, x, st, H, t0, mean, sd, "missing patterns")
    for t in (0, 1, 2, 14):                                   # no observed cell: filtered = predicted exactly, log density 0
        assert np.array_equal(got["z_filt"][:, t], got["z_pred"][:, t]) and np.array_equal(got["P_filt"][:, t], got["P_pred"][:, t])
        assert np.all(got["loglik_t"][:, t] == 0.0)
    assert np.all(got["cnt"][:, :, [5, 7]] == 0) and np.all(np.isnan(got["msfe"][:, :, [5, 7]]))


def test_two_calls_are_bit_identical(ctx):
    x, st = fe.params_for(B, 130, 150, 4, 2, missing=0.1)
    a = ctx.filter_batch_host(x, *[st[k] for k in KEYS], H=5, t0=10, want=fe_eval())
    b = ctx.filter_batch_host(x, *[st[k] for k in KEYS], H=5, t0=10, want=fe_eval())
    for n in fe_eval():
        assert np.array_equal(a[n], b[n], equal_nan=True), n
    assert np.any(a["cnt"] > 64), "more than one origin chunk was meant to be summed"


def fe_eval():
    return ("msfe", "msfe0", "cnt")


# ------------------------------------------------------------------------------------------------------------ the smoother kernels
@pytest.mark.parametrize("r,p,missing", [(8, 1, 0.0), (8, 1, 0.1), (4, 4, 0.1)], ids=["fused", "chunked", "companion"])
def test_against_the_smoother_pass_on_the_gpu(ctx, r, p, missing):
    N, T = 40, 60
    x, st = fe.params_for(B, N, T, r, p, missing=missing)
    P = [st[k] for k in KEYS]
    npk = r * (r + 1) // 2
    pas = ctx.ks_pass_batch_host if p == 1 else ctx.ks_pass_varp_batch_host
    got = ctx.filter_batch_host(x, *P, want=("z_filt", "P_filt", "loglik_t"))
    f, Ps, ll = pas(x, *P)
    _close(got["loglik_t"].sum(axis=1), ll, "sum of loglik_t against the pass")
    _close(got["z_filt"][:, -1, :r], f[:, -1], "last filtered mean against the last smoothed mean")
    _close(got["P_filt"][:, -1, :npk], Ps[:, -1], "last filtered covariance against the last smoothed one")
    if p == 1:
        for t in (0, 17, 41):
            f, Ps, _ = pas(np.ascontiguousarray(x[:, :t + 1]), *P)
            _close(got["z_filt"][:, t, :r], f[:, -1], f"filtered mean at {t} against the pass on {t + 1} rows")
            _close(got["P_filt"][:, t, :npk], Ps[:, -1], f"filtered covariance at {t} against the pass on {t + 1} rows")


# ------------------------------------------------------------------------------------------------------------ status, entries
def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    x, st = fe.params_for(1, 20, 30, 2, 1)
    P = [st[k] for k in KEYS]
    good = lambda: ctx.filter_batch_host(x, *P, H=2, t0=5)
    ptr = lambda a: ctypes.c_void_p(np.ascontiguousarray(a).ctypes.data)
    ll = np.empty((1, 30))
    base = [ptr(x)] + [ptr(a) for a in P] + [None, None]
    outs = [None] * 4 + [ptr(ll)] + [None] * 6
    lib = ctx._lib
    assert lib.dfm_filter_batch(ctx._h, 1, 30, 20, 2, 1, -1, 0, *base, *outs, 0) == -1           # H < 0
    good()
    assert lib.dfm_filter_batch(ctx._h, 1, 30, 20, 2, 1, 2, 30, *base, *outs, 0) == -1           # t0 = T
    good()
    bad = x.copy(); bad[0, 5, 3] = np.nan
    with pytest.raises(_lib.DfmError) as ei:
        ctx.filter_batch_host(bad, *P, may_have_missing=False)
    assert ei.value.code == -4
    good()
    Qn = st["Q"].copy(); Qn[0, 0, 0] = -5.0                                                       # a negative eigenvalue
    with pytest.raises(_lib.DfmError) as ei:
        ctx.filter_batch_host(x, st["Lam"], st["R"], st["A"], Qn, st["mu0"], st["P0"])
    assert ei.value.code == -5
    ok = good()
    assert np.all(np.isfinite(ok["loglik_t"]))
    ok = ctx.filter_batch_host(x, *P, singular_q=True, want=("loglik_t",))                        # accepted, changes nothing
    assert np.array_equal(ok["loglik_t"], good()["loglik_t"])


def test_dev_and_host_entries_agree(ctx):
    import torch
    x, st = fe.params_for(B, 60, 40, 3, 2, missing=0.1)
    mean, sd = _scales(60, True)
    host = ctx.filter_batch_host(x, *[st[k] for k in KEYS], H=4, t0=7, mean=mean, sd=sd)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ctx.filter_batch_dev(t(x), *[t(st[k]) for k in KEYS], H=4, t0=7, mean=t(mean), sd=t(sd))
    ctx.synchronize()
    for n in host:
        assert np.array_equal(got[n].cpu().numpy(), host[n], equal_nan=True), n


# ------------------------------------------------------------------------------------------------------------ the api
def _sw_model(lags):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    return api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, lags)


@pytest.mark.parametrize("lags", [1, 4])
def test_api_on_the_stock_watson_panel(ctx, lags):
    from dynamic_factor_models_amd import api
    m = _sw_model(lags)
    api.estimate(m, api.Parametric(), max_em_iter=5, tol_em=0.0, factor_lags=lags, ctx=ctx, nrep=8 if lags == 1 else 0, seed=11)
    ep = {k: v.copy() for k, v in m.em_params.items()}
    cols, z, mu, sd = api._forecast_inputs(m, m.lastperiod)
    A = ep["Avar"] if lags > 1 else ep["A"]
    q = np.array([0.1, 0.5, 0.9]) if lags == 1 else None
    H, fo, r = 4, 150, 4
    fs = api.filter_states(m, quantiles=q, ctx=ctx)
    ev = api.evaluate_forecasts(m, H, first_origin=fo, quantiles=q, ctx=ctx)
    e = fe.expect(z, ep["Lam"], ep["R"], A, ep["Q"], ep["mu0"], ep["P0"], H=H, t0=fo - m.initperiod, mean=mu, sd=sd)
    T, N = z.shape
    assert np.array_equal(fs["cols"], cols) and np.array_equal(fs["rows"], np.arange(m.initperiod, m.lastperiod + 1))
    _close(fs["state_pred"], e["z_pred"], "api state_pred")
    _close(fs["state_filt"], e["z_filt"], "api state_filt")
    _close(fs["factor_filt"], e["z_filt"][:, :r], "api factor_filt")
    _close(fe.pack(fs["factor_pred_cov"]), e["P_pred"][:, :r * (r + 1) // 2], "api factor_pred_cov")
    _close(fe.pack(fs["factor_filt_cov"]), e["P_filt"][:, :r * (r + 1) // 2], "api factor_filt_cov")
    _close(fs["loglik_t"], e["loglik_t"], "api loglik_t")
    _close(fs["x_pred"], e["xpred"], "api x_pred")
    _close(fs["error"], e["verr"], "api error")
    _close(fs["error_std"], e["vstd"], "api error_std")
    _close(ev["msfe"], e["msfe"], "api msfe")
    _close(ev["relative"], e["msfe"] / e["msfe0"], "api relative")
    assert np.array_equal(ev["count"], e["cnt"]) and np.all(np.isfinite(ev["relative"][ev["count"] > 0]))
    _close(ev["rmsfe"], np.sqrt(e["msfe"]), "api rmsfe")
    if lags == 1:
        assert fs["bands"].shape == (3, T, N) and ev["bands"].shape == (3, H, N)
        assert np.all(np.diff(fs["bands"], axis=0) >= 0.0) and np.all(np.diff(ev["bands"][:, ev["count"] > 0], axis=0) >= 0.0)
    first = api.evaluate_forecasts(m, 1, ctx=ctx)              # first_origin defaults to the middle of the window
    assert first["count"].max() == T - 1 - T // 2
    assert all(np.array_equal(ep[k], m.em_params[k]) for k in ep), "the api changed m.em_params"
