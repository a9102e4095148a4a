"""GPU: the copy-back of the five EM drivers (csrc/capi.hip unpad_results / odd_unpad).  Each family's device entry runs three
times from the same start -- with f_smooth and P_smooth, with f_smooth only, with neither -- on a shape whose factor count is no
power of two, so that every un-padding copy runs; the plain family also at r = 8 (the caller's layout is the plan's: nothing to
copy back) and on an odd N with missing cells (the appended series is cut off again).  The three calls must agree at the 1e-8
the families' own files assert for EM paths and parameters, and the first is compared with the family's oracle as its own file
does (helpers and tolerances from tests/test_gpu_em.py, test_gpu_varp.py, test_gpu_ar_em.py, test_gpu_mf.py, test_gpu_round3.py)."""
import numpy as np
import pytest

from oracle import ar_oracle as ao
from oracle import kalman_oracle as ko
from oracle import obs_oracle as oo
from oracle import varp_oracle as vo
from tests import mf_expect as me
import test_gpu_ar_em as t_ar
import test_gpu_em as t_em
import test_gpu_mf as t_mf
import test_gpu_round3 as t_r3
import test_gpu_varp as t_varp

pytestmark = pytest.mark.gpu

B, T, ITERS, MISS = 2, 40, 3, 0.1
WANTS = ((True, True), (True, False), (False, False))          # (f_smooth, P_smooth) asked for


@pytest.fixture(scope="module")
def ctx():
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext(0)
    yield c
    c.close()


def _t(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _three(ctx, keys, st, call):
    """call(dev, want_smooth, want_P) -> (path, iters, f, P) with the tensors in `dev` updated in place.  Returns the three calls'
    (params, path, f, P) as NumPy after checking that they agree."""
    import torch
    runs = []
    for want_f, want_P in WANTS:
        dev = {k: _t(ctx, st[k]) for k in keys}
        path, its, f, P = call(dev, want_f, want_P)
        torch.cuda.synchronize()
        assert np.all(_np(its) == ITERS)
        assert (f is not None) == want_f and (P is not None) == want_P
        runs.append(({k: _np(dev[k]) for k in keys}, _np(path), _np(f), _np(P)))
    first = runs[0]
    for (want_f, want_P), run in zip(WANTS[1:], runs[1:]):
        for k in keys:
            if first[0][k].size:                                   # (rho at q = 0)
                err = np.abs(run[0][k] - first[0][k]).max()
                print(f"f={want_f} P={want_P} {k} {err:.2e}")
                assert err <= 1e-8 * max(1.0, np.abs(first[0][k]).max()), (k, want_f, want_P, err)
        np.testing.assert_allclose(run[1], first[1], rtol=1e-8, err_msg=f"loglik path f={want_f} P={want_P}")
        if want_f:
            assert np.abs(run[2] - first[2]).max() <= 1e-8 * max(1.0, np.abs(first[2]).max()), ("f_smooth", want_P)
    return first


# r = 3: widened to the 8-wide state, loadings 4 wide; r = 8: no padding; N = 25 with missing cells: one series appended
@pytest.mark.parametrize("N,r,missing", [(24, 3, MISS), (24, 8, MISS), (25, 3, MISS), (24, 3, 0.0), (24, 8, 0.0)])
def test_plain(ctx, N, r, missing):
    keys = t_em.KEYS
    panel, st = t_em._start(B, N, T, r, missing)
    x = _t(ctx, panel)
    par, path, f, P = _three(ctx, keys, st, lambda d, wf, wp: ctx.em_batch(
        x, *[d[k] for k in keys], max_iter=ITERS, tol=0.0, want_smooth=wf, want_P=wp))
    for b in range(B):
        p, opath, out = ko.em(panel[b], {k: st[k][b] for k in keys}, max_iter=ITERS, tol=0.0)
        np.testing.assert_allclose(path[b], opath, rtol=t_em.RTOL, err_msg=f"loglik path b={b}")
        for k in keys:
            assert np.abs(par[k][b] - p[k]).max() <= t_em.RTOL * max(1.0, np.abs(p[k]).max()), (k, b, np.abs(par[k][b] - p[k]).max())
        assert np.abs(f[b] - out["f_smooth"]).max() <= t_em.RTOL * np.abs(out["f_smooth"]).max()
        assert np.abs(P[b] - ko.pack_sym(out["P_smooth"])).max() <= t_em.RTOL * np.abs(out["P_smooth"]).max()


@pytest.mark.parametrize("N", [24, 25])                            # 25: loadings up to 4 wide, missing cells -> one series appended
def test_varp(ctx, N, r=3, p=2):
    keys = t_varp.KEYS
    panel, st = t_varp._batch(B, N, T, r, p, MISS)
    x = _t(ctx, panel)
    par, path, f, P = _three(ctx, keys, st, lambda d, wf, wp: ctx.em_varp_batch(
        x, *[d[k] for k in keys], max_iter=ITERS, tol=0.0, want_smooth=wf, want_P=wp))
    tri = np.tril_indices(r)
    for b in range(B):
        qo, opath, out = vo.em_varp(panel[b], {k: st[k][b] for k in keys}, p, ITERS)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8)
        for k in keys:
            t_varp._close(par[k][b], qo[k], 1e-8, k)
        t_varp._close(f[b], out["f_smooth"][:, :r], 1e-8, "f_smooth")
        t_varp._close(P[b], out["P_smooth"][:, :r, :r][:, tri[0], tri[1]], 1e-8, "P_smooth")


def test_ar(ctx, N=24, r=3, p=2, q=1):
    keys = t_ar.KEYS
    panel, st = t_ar._stack(B, N, T, r, p, q, MISS)
    x = _t(ctx, panel)
    par, path, f, P = _three(ctx, keys, st, lambda d, wf, wp: ctx.em_ar_batch(
        x, *[d[k] for k in keys], max_iter=ITERS, tol=0.0, want_smooth=wf, want_P=wp))
    assert f.shape == (B, T - q, r) and P.shape == (B, T - q, r * (r + 1) // 2)
    for b in range(B):
        ref, opath, out = ao.em_ar(panel[b], {k: st[k][b] for k in keys}, max_iter=ITERS)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")
        for k in keys:
            tol = 1e-7 * max(1.0, np.abs(ref[k]).max())
            assert np.abs(par[k][b] - ref[k]).max() <= tol, (k, b, np.abs(par[k][b] - ref[k]).max())
        fo = out["f_smooth"][:, :r]
        assert np.abs(f[b] - fo).max() <= 1e-8 * max(1.0, np.abs(fo).max())
        assert t_mf._rel(P[b], t_mf._packed(out["P_smooth"], r)) <= 1e-8


def test_mf(ctx, Nm=16, Nq=8, r=3, p=2):
    keys = t_mf.KEYS
    panel, W, st = t_mf._stack(B, Nm, Nq, T, r, p, "q_avg", MISS)
    assert W.shape == (Nm + Nq, 3)                                 # L = 3 aggregation lags
    x, w = _t(ctx, panel), _t(ctx, W)
    par, path, f, P = _three(ctx, keys, st, lambda d, wf, wp: ctx.em_mf_batch(
        x, d["Lam"], d["R"], w, d["Avar"], d["Q"], d["mu0"], d["P0"], max_iter=ITERS, tol=0.0, want_smooth=wf, want_P=wp))
    for b in range(B):
        ref, opath, out = me.em_mf(panel[b], {k: st[k][b] for k in keys}, W, max_iter=ITERS)
        np.testing.assert_allclose(path[b], opath, rtol=1e-8, err_msg=f"loglik path b={b}")
        for k in keys:
            tol = 1e-7 * max(1.0, np.abs(ref[k]).max())
            assert np.abs(par[k][b] - ref[k]).max() <= tol, (k, b, np.abs(par[k][b] - ref[k]).max())
        fo = out["f_smooth"][:, :r]
        assert np.abs(f[b] - fo).max() <= 1e-8 * max(1.0, np.abs(fo).max())
        assert t_mf._rel(P[b], t_mf._packed(out["P_smooth"], r)) <= 1e-8


def _em_obs_dev(ctx, x, G, d, want_f, want_P):
    """dfm_em_obs_batch_dev has no wrapper of its own in kalman.py (em_obs_batch_host stages through it)."""
    import torch
    Bn, Tn, N = x.shape
    ro, ru = G.shape[2], d["A"].shape[1]
    dev = x.device
    path = torch.empty((Bn, ITERS), dtype=torch.float64, device=dev)
    its = torch.empty((Bn,), dtype=torch.int32, device=dev)
    f = torch.empty((Bn, Tn, ru), dtype=torch.float64, device=dev) if want_f else None
    P = torch.empty((Bn, Tn, ru * (ru + 1) // 2), dtype=torch.float64, device=dev) if want_P else None
    ptr = lambda t: None if t is None else ctx._dev(t, "tensor")
    ctx._sync_stream()
    rc = ctx._lib.dfm_em_obs_batch_dev(ctx._h, Bn, Tn, N, ru, ro, ptr(x), ptr(G), *[ptr(d[k]) for k in t_r3.KEYS], ITERS, 0.0,
                                       ptr(path), its.data_ptr(), ptr(f), ptr(P), 1)   # DFM_F_MAY_HAVE_MISSING
    assert rc == 0, ctx._lib.dfm_last_error(ctx._h)
    return path, its, f, P


@pytest.mark.parametrize("ru,ro", [(3, 1), (8, 1)])                # (8, 1): r_o + r_u > 8, the unobserved block not padded
def test_observed_factors(ctx, ru, ro, N=24):
    keys = t_r3.KEYS
    reps = [oo.synth_obs(100 + b, N, T, ru, ro, missing=MISS) for b in range(B)]
    panel = np.stack([x for x, _, _ in reps]); G = np.stack([g for _, g, _ in reps])
    st = {k: np.stack([p[k] for _, _, p in reps]) for k in keys}
    x, g = _t(ctx, panel), _t(ctx, G)
    par, path, f, P = _three(ctx, keys, st, lambda d, wf, wp: _em_obs_dev(ctx, x, g, d, wf, wp))
    for b in range(B):
        p, opath, out = oo.em_obs(panel[b], G[b], {k: st[k][b] for k in keys}, max_iter=ITERS, tol=0.0)
        np.testing.assert_allclose(path[b], opath, rtol=t_r3.RTOL, err_msg=f"loglik path b={b}")
        for k in keys:
            assert np.abs(par[k][b] - p[k]).max() <= 1e-8 * max(1.0, np.abs(p[k]).max()), (k, b, np.abs(par[k][b] - p[k]).max())
        assert np.abs(f[b] - out["f_smooth"]).max() <= 1e-8 * np.abs(out["f_smooth"]).max()
        assert np.abs(P[b] - ko.pack_sym(out["P_smooth"])).max() <= 1e-8 * np.abs(out["P_smooth"]).max()
