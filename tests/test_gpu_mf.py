"""GPU: the mixed-frequency DFM (dfm_ks_pass_mf_batch*, dfm_em_mf_batch*: mstep_mf.hip + the companion pass routes and the restricted
transition step) against the NumPy model tests/mf_expect.py, which tests/test_mf_cpu.py pins to brute-force Gaussian conditioning.
PARITY UNPINNED by the reference (no Kalman / EM code there, and it averages the months away before estimating).
Tolerances: those of tests/test_gpu_ar_em.py for the sibling model."""
import os

import numpy as np
import pytest

from tests import mf_expect as me
from oracle import varp_oracle as vo

pytestmark = pytest.mark.gpu

KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


def _stack(B, Nm, Nq, T, r, p, kind, missing=0.0, ragged=0, thin=None):
    """B panels with ONE weight matrix (monthly series first)."""
    xs, Ws, sts = zip(*[me.synth_mf(b, Nm, Nq, T, r, p, kind, missing=missing, ragged=ragged) for b in range(B)])
    assert all(np.array_equal(W, Ws[0]) for W in Ws)
    x = np.stack(xs)
    if thin is not None:                                       # one series with fewer than r + 1 observed cells
        keep = np.nonzero(~np.isnan(x[0, :, thin]))[0][:r]
        col = x[:, :, thin].copy()
        x[:, :, thin] = np.nan
        x[:, keep, thin] = col[:, keep]
    return x, Ws[0], {k: np.stack([s[k] for s in sts]) for k in KEYS}


def _packed(P, r):
    il = np.tril_indices(r)
    return P[:, :r, :r][:, il[0], il[1]]


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# (B, Nm, Nq, T, r, p, kind, missing, ragged, thin series, singular_q, EM iterations): the companion routes by SHAPE
CASES = [
    (2, 10, 4, 60, 2, 1, "q_avg", 0.0, 0, None, False, 4),      # L = 3: state 6
    (2, 12, 5, 72, 2, 2, "q_flow", 0.05, 3, 1, False, 4),       # L = 5: state 10, odd N, missing cells, ragged edge, a thin series
    (2, 11, 4, 60, 3, 1, "q_flow", 0.04, 2, None, False, 3),    # state 15: blocks narrower than 4
    (2, 100, 39, 90, 4, 4, "q_flow", 0.05, 3, 5, False, 3),     # state 20, N = 139 (the Stock-Watson window's width), tiles of both classes
    (2, 100, 39, 90, 4, 4, "q_flow", 0.05, 3, 5, True, 3),      # the same in covariance form
    (2, 20, 12, 60, 4, 1, "q_avg", 0.0, 0, None, True, 3),      # state 12, even N, only the quarterly NaN pattern, covariance form
    (2, 14, 6, 66, 6, 2, "q_flow", 0.03, 2, None, False, 3),    # state 30
    (2, 12, 6, 60, 8, 1, "q_avg", 0.05, 0, 0, False, 3),        # r = 8, state 24: three G tiles per class row
]


@pytest.mark.parametrize("B,Nm,Nq,T,r,p,kind,missing,ragged,thin,sq,iters", CASES)
def test_pass_mf_matches_model(ctx, B, Nm, Nq, T, r, p, kind, missing, ragged, thin, sq, iters):
    x, W, st = _stack(B, Nm, Nq, T, r, p, kind, missing, ragged, thin=thin)
    f, P, ll = ctx.ks_pass_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], singular_q=sq)
    for b in range(B):
        out = me.kfs_pass_mf(x[b], W=W, **{k: st[k][b] for k in KEYS})
        fo, Po = out["f_smooth"][:, :r], _packed(out["P_smooth"], r)
        print(f"b={b} f {_rel(f[b], fo):.2e} P {_rel(P[b], Po):.2e} ll {abs(ll[b] - out['loglik']) / abs(out['loglik']):.2e}")
        assert _rel(f[b], fo) <= 1e-9
        assert _rel(P[b], Po) <= 1e-9
        assert abs(ll[b] - out["loglik"]) <= 1e-9 * abs(out["loglik"])


@pytest.mark.parametrize("B,Nm,Nq,T,r,p,kind,missing,ragged,thin,sq,iters", CASES)
def test_em_mf_matches_model(ctx, B, Nm, Nq, T, r, p, kind, missing, ragged, thin, sq, iters):
    x, W, st = _stack(B, Nm, Nq, T, r, p, kind, missing, ragged, thin=thin)
    est, path, its, f, P = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"],
                                                max_iter=iters, singular_q=sq)
    for b in range(B):
        ref, opath, out = me.em_mf(x[b], {k: st[k][b] for k in KEYS}, W, max_iter=iters)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")
        for k in KEYS:
            tol = 1e-7 * max(1.0, np.abs(ref[k]).max())
            err = np.abs(est[k][b] - ref[k]).max()
            print(f"b={b} {k} {err:.2e}")
            assert err <= tol, (k, b, err)
        fo = out["f_smooth"][:, :r]
        assert np.abs(f[b] - fo).max() <= 1e-8 * max(1.0, np.abs(fo).max())
        assert _rel(P[b], _packed(out["P_smooth"], r)) <= 1e-8
        if thin is not None:                                   # fewer than r + 1 observed cells: left as it was
            assert np.array_equal(est["Lam"][b, thin], st["Lam"][b, thin]) and est["R"][b, thin] == st["R"][b, thin]
    assert np.all(its == iters)


def test_series_order_does_not_matter(ctx):
    """Monthly and quarterly series interleaved (tiles gather their class's series by index) against the class-sorted panel."""
    x, W, st = _stack(2, 37, 20, 72, 3, 2, "q_flow", 0.05, 2)
    mix = np.random.default_rng(5).permutation(W.shape[0])
    x, W = np.ascontiguousarray(x[:, :, mix]), np.ascontiguousarray(W[mix])
    st = dict(st, Lam=st["Lam"][:, mix], R=st["R"][:, mix])
    order = np.argsort(W[:, 1] != 0.0, kind="stable")          # monthly first, quarterly after: class-contiguous
    assert np.any(np.diff(order) < 0)
    a, pa, _, fa, _ = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=3)
    b, pb, _, fb, _ = ctx.em_mf_batch_host(x[:, :, order], st["Lam"][:, order], st["R"][:, order], W[order], st["Avar"], st["Q"],
                                           st["mu0"], st["P0"], max_iter=3)
    assert _rel(pa, pb) <= 1e-10 and _rel(fa, fb) <= 1e-10
    assert _rel(a["Lam"][:, order], b["Lam"]) <= 1e-10 and _rel(a["R"][:, order], b["R"]) <= 1e-10
    for k in ("Avar", "Q", "mu0", "P0"):
        assert _rel(a[k], b[k]) <= 1e-10, k
    ref, opath, _ = me.em_mf(x[1], {k: st[k][1] for k in KEYS}, W, max_iter=3)
    np.testing.assert_allclose(pa[1], opath, rtol=1e-8)
    assert np.abs(a["Lam"][1] - ref["Lam"]).max() <= 1e-7 * max(1.0, np.abs(ref["Lam"]).max())


def test_three_weight_classes(ctx):
    kinds = ["q_flow", "q_avg"] * 9 + ["q_flow"]
    x, W, st = _stack(2, 21, 19, 72, 2, 2, kinds, 0.04, 2)
    assert len({tuple(w) for w in W}) == 3
    est, path, _, f, _ = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=3)
    for b in range(2):
        ref, opath, out = me.em_mf(x[b], {k: st[k][b] for k in KEYS}, W, max_iter=3)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8)
        for k in KEYS:
            assert np.abs(est[k][b] - ref[k]).max() <= 1e-7 * max(1.0, np.abs(ref[k]).max()), k


def test_one_lag_is_the_varp_model(ctx):
    B, N, T, r, p = 2, 24, 70, 3, 2
    xs = [vo.synth_varp(b, N, T, r, p, missing=0.06) for b in range(B)]
    sts = [vo.varp_init(np.where(np.isnan(x), 0.0, x), r, p)[0] for x in xs]
    x = np.stack(xs)
    st = {k: np.stack([s[k] for s in sts]) for k in KEYS}
    a, pa, _, fa, Pa = ctx.em_mf_batch_host(x, st["Lam"], st["R"], np.ones((N, 1)), st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=3)
    b, pb, _, fb, Pb = ctx.em_varp_batch_host(x, *[st[k] for k in KEYS], max_iter=3)
    assert _rel(pa, pb) <= 1e-10 and _rel(fa, fb) <= 1e-10 and _rel(Pa, Pb) <= 1e-10
    for k in KEYS:
        assert _rel(a[k], b[k]) <= 1e-10, (k, _rel(a[k], b[k]))


def test_tol_stops_replicates_separately(ctx):
    B = 4
    x, W, st = _stack(B, 14, 6, 90, 2, 1, "q_avg", 0.03, 2)
    st["Lam"][2:] *= 0.3                                       # two replicates start further away
    est, path, its, _, _ = ctx.em_mf_batch_host(x, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"], max_iter=40, tol=1e-5)
    print("iters", its)
    for b in range(B):
        _, opath, _ = me.em_mf(x[b], {k: st[k][b] for k in KEYS}, W, max_iter=40, tol=1e-5)
        assert its[b] == len(opath), (b, its[b], len(opath))
        pb = path[b, :its[b]]
        np.testing.assert_allclose(pb, opath, rtol=1e-8)
        assert np.all(np.diff(pb) >= -1e-8 * np.abs(pb[:-1]))
        assert np.all(np.isnan(path[b, its[b]:]))
    assert its.min() >= 2 and its.max() < 40 and its.min() != its.max()


def test_status_codes(ctx):
    from dynamic_factor_models_amd._lib import DfmError
    x, W, st = _stack(1, 10, 4, 36, 2, 1, "q_avg")
    args = lambda Wx, s=st: (x, s["Lam"], s["R"], Wx, s["Avar"], s["Q"], s["mu0"], s["P0"])

    def code(fn, *a, **kw):
        with pytest.raises(DfmError) as ei:
            fn(*a, **kw)
        return ei.value.code

    W6 = np.hstack([W, np.zeros((14, 3))])                      # L = 6
    s6 = dict(st, mu0=np.zeros((1, 12)), P0=np.eye(12)[None])
    assert code(ctx.em_mf_batch_host, *args(W6, s6), max_iter=2) == -1
    assert code(ctx.ks_pass_mf_batch_host, *args(W6, s6)) == -1
    r8 = dict(Lam=np.zeros((1, 14, 8)), R=np.ones((1, 14)), Avar=np.zeros((1, 8, 8)), Q=np.eye(8)[None], mu0=np.zeros((1, 40)),
              P0=np.eye(40)[None])
    W5 = np.hstack([W, np.zeros((14, 2))])                      # r L = 40 > 32
    assert code(ctx.em_mf_batch_host, *args(W5, r8), max_iter=2) == -2
    Wn = W.copy(); Wn[3, 1] = np.nan
    assert code(ctx.em_mf_batch_host, *args(Wn), max_iter=2) == -1
    assert code(ctx.ks_pass_mf_batch_host, *args(Wn)) == -1
    W9 = W.copy(); W9[:9, 2] = 0.01 * np.arange(9)              # nine distinct rows
    assert code(ctx.em_mf_batch_host, *args(W9), max_iter=2) == -1
    f, _, ll = ctx.ks_pass_mf_batch_host(*args(W9))             # (the pass has no class table: any finite W)
    assert np.isfinite(ll).all()
    assert code(ctx.em_mf_batch_host, *args(W), max_iter=2, may_have_missing=False) == -4
    est, path, _, _, _ = ctx.em_mf_batch_host(*args(W), max_iter=2)   # the handle works on
    assert np.isfinite(path).all()


def test_device_entry_updates_in_place(ctx):
    import torch
    x, W, st = _stack(2, 12, 5, 60, 2, 2, "q_flow", 0.03, 1)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: t(st[k]) for k in KEYS}
    path, its, f, P = ctx.em_mf_batch(t(x), d["Lam"], d["R"], t(W), d["Avar"], d["Q"], d["mu0"], d["P0"], max_iter=3)
    torch.cuda.synchronize()
    ref, opath, _ = me.em_mf(x[1], {k: st[k][1] for k in KEYS}, W, max_iter=3)
    np.testing.assert_allclose(path[1].cpu().numpy(), opath, rtol=1e-8)
    assert np.abs(d["Lam"][1].cpu().numpy() - ref["Lam"]).max() <= 1e-7 * max(1.0, np.abs(ref["Lam"]).max())
    assert P.shape == (2, 60, 3)
    f2, P2, ll = ctx.ks_pass_mf_batch(t(x), t(st["Lam"]), t(st["R"]), t(W), t(st["Avar"]), t(st["Q"]), t(st["mu0"]), t(st["P0"]))
    torch.cuda.synchronize()
    np.testing.assert_allclose(ll[1].item(), opath[0], rtol=1e-9)


def sw_mixed_panel(months=360, min_cells=24):
    """The monthly Stock-Watson panel from the two sheets of the fixture: the monthly sheet's include-code-1 series at MONTHLY
    frequency, the quarterly sheet's include-code-1 series in the third month of their quarter, each transformed by its own code at
    its own frequency and outlier-adjusted (oracle/sw_panel.py: transform, adjust_outlier), the last `months` months.  No biweight
    detrending and no deflators: the model needs neither, the test only needs a real ragged panel.  Series with fewer than
    `min_cells` observed cells in the window are dropped.  Returns (x [months, N], kinds, number dropped)."""
    from oracle import sw_panel as sp
    path = os.path.join(HERE, "golden", "hom_fac_1_sheets.xlsx")

    def sheet(name, ncodes, off, nmax=None):
        grid = sp.read_xlsx_sheet(path, name)
        top = 1 + 2 + ncodes
        ns = len(grid[0]) - 1
        row = lambda k: (grid[k][1:ns + 1] + [None] * ns)[:ns]
        tcode, ocode, incl = ([int(v) if isinstance(v, float) else 0 for v in row(k + off)] for k in (3, 5, 6))
        nobs = sum(1 for g in grid[top:] if g and isinstance(g[0], float))
        nobs = nobs if nmax is None else min(nobs, nmax)       # (the monthly sheet runs a few months past the last full quarter)
        dat = np.full((nobs, ns), np.nan)
        for t in range(nobs):
            for j, v in enumerate(row(top + t)):
                if isinstance(v, float):
                    dat[t, j] = v
        cols = [j for j in range(ns) if incl[j] == 1]
        out = np.full((nobs, len(cols)), np.nan)
        for c, j in enumerate(cols):
            out[:, c] = sp.transform(dat[:, j], tcode[j])
            sp.adjust_outlier(out[:, c], ocode[j])
        return out

    xq = sheet("Quarterly", 5, 0)
    xm = sheet("Monthly", 6, 1, 3 * xq.shape[0])
    assert xm.shape[0] == 3 * xq.shape[0]
    xm = xm[-months:]
    xq3 = np.full((months, xq.shape[1]), np.nan)
    xq3[2::3] = xq[-(months // 3):]
    x = np.hstack([xm, xq3])
    kinds = ["m"] * xm.shape[1] + ["q_flow"] * xq.shape[1]
    keep = (~np.isnan(x)).sum(0) >= min_cells
    return x[:, keep], [k for k, u in zip(kinds, keep) if u], int((~keep).sum())


def test_api_on_the_stock_watson_sheets(ctx):
    from dynamic_factor_models_amd import api
    x, kinds, dropped = sw_mixed_panel()
    N = x.shape[1]
    print(f"Stock-Watson mixed panel: {x.shape[0]} months x {N} series ({kinds.count('m')} monthly), dropped {dropped}")
    assert dropped <= 0.05 * (N + dropped)
    fit = api.estimate_mixed_frequency(x, kinds, 4, 4, max_em_iter=4, tol_em=0.0, ctx=ctx)
    W = fit["W"]
    z = (x - fit["mean"]) / fit["sd"]
    ref, opath, out = me.em_mf(z, fit["start"], W, max_iter=4)
    np.testing.assert_allclose(fit["loglik_path"], opath, rtol=1e-7)
    assert np.all(np.diff(opath) > 0)
    assert np.abs(fit["Lam"] - ref["Lam"]).max() <= 1e-6 * np.abs(ref["Lam"]).max()
    # nowcast / forecast: the conditional mean and variance of the expanded model at the fitted parameters (NumPy), H = 6
    H = 6
    fc = api.forecast_mixed(fit, x, H, ctx=ctx)
    T = x.shape[0]
    LamK, M, Qk, _ = me.expanded(fit["Lam"], W, fit["Avar"], fit["Q"])
    po = me.ko.kfs_pass(z, LamK, fit["R"], M, Qk, fit["mu0"], fit["P0"], lag_one=True)
    zs = [po["f_smooth"][-1]]; Ps = [po["P_smooth"][-1]]
    for _ in range(H):
        zs.append(M @ zs[-1]); Ps.append(M @ Ps[-1] @ M.T + Qk)
    Z = np.vstack([po["f_smooth"], np.array(zs[1:])])
    PP = np.concatenate([po["P_smooth"], np.array(Ps[1:])])
    mean = fit["mean"] + fit["sd"] * (Z @ LamK.T)
    var = fit["sd"] ** 2 * (np.einsum("ik,tkl,il->ti", LamK, PP, LamK) + fit["R"])
    obs = np.vstack([~np.isnan(x), np.zeros((H, N), bool)])
    xhat = np.where(obs, np.vstack([x, np.zeros((H, N))]), mean)
    xvar = np.where(obs, 0.0, var)
    jq = kinds.index("q_flow")                                  # a quarterly series: its unpublished months and the horizon
    edge = slice(T - 6, T + H)
    for name, got, want in (("x", fc["x"], xhat), ("x_sd", fc["x_sd"] ** 2, xvar), ("common", fc["common"], mean)):
        e_all, e_q = _rel(got[edge], want[edge]), _rel(got[edge, jq], want[edge, jq])
        print(f"{name}: ragged edge + horizon {e_all:.2e}, quarterly series {e_q:.2e}")
        assert e_all <= 1e-9 and e_q <= 1e-9
    assert np.isnan(x[T - 1, :kinds.count("m")]).any()          # the window does end in a ragged edge
    assert _rel(fc["factor"], Z[:, :4]) <= 1e-9
