#!/usr/bin/env python
"""Measurement lines of dfm_diffusion_eval_batch_dev (csrc/diffusion.hip; run on the GPU box).  Workloads:
  di_sw  -- the Stock-Watson panel, rows 3..224 in data units, r = 4, q = 4, W = 120, H = 4, the last 100 origins, 20 ALS sweeps
            from the full-sample factors
  di_c2  -- T = 500, N = 200, r = 8, q = 4, W = 250, H = 12, the last 250 origins, balanced (a dfm_synth_panels_dev replicate put
            into data units), 20 ALS sweeps from the full-sample PCA scores
Each line: ms per call (median of 20 timed calls after warm-up, HIP events); the same with max_iter = 0 (what is left is the ALS's
share); the per-kernel ms of one profiled call (dfm_profile_read); di_regress_kernel per regression (O N H of them: no publication
lags, so h = 0 is visible); and the route the kernel replaces -- the same regressions through dfm_ols_batch_dev on materialised
regressors, one [W][K] matrix per (origin, series, horizon), for 16 origins (the full set does not fit comfortably), per regression;
beside it the host loop's wall time (per origin one als_batch_host call, the regressors built in NumPy, one ols_batch_host call),
timed for those origins and scaled to O.  Prints one JSON line per workload."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, api  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, K_TIMED, SWEEPS, NSUB = 3, 20, 20, 16
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def timed(fn, k=K_TIMED):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ctx.synchronize()
    return float(np.median(ms))


def profiled(fn):
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: round(v[0], 4) for k, v in prof.items()}


def regressors(z, F, H, q):
    """One window's materialised problems, h = 1 .. H of every series: X [N H, W, K] and y [N H, W], NaN outside the rows in use."""
    W, N = z.shape
    r = F.shape[1]
    X = np.full((N, H, W, 1 + r + q), np.nan)
    y = np.full((N, H, W), np.nan)
    X[..., 0] = 1.0
    X[..., 1:1 + r] = F[None, None]
    for m in range(q):
        X[:, :, m:, 1 + r + m] = z[:W - m].T[:, None, :]
    for h in range(1, H + 1):
        y[:, h - 1, :W - h] = z[h:].T
    return X.reshape(N * H, W, -1), y.reshape(N * H, W)


def line(name, x, F_path, q, W, H, O, nt_min, min_obs):
    T, N = x.shape
    r = F_path.shape[1]
    Kreg = 1 + r + q
    origins = np.arange(T - O, T)
    miss = bool(np.isnan(x).any())
    xd, Fd = t(x), t(F_path)
    call = lambda it, want=("msfe", "msfe_ar", "msfe0", "cnt"): ctx.diffusion_eval_batch(
        xd, origins, W, H, Fd, q=q, min_obs=min_obs, nt_min=nt_min, max_iter=it, tol=0.0, want=want, may_have_missing=miss)
    ms, ms0, prof = timed(lambda: call(SWEEPS)), timed(lambda: call(0)), profiled(lambda: call(SWEEPS))
    nreg = O * N * H
    reg_ms = prof.get("di_regress_kernel", float("nan"))
    # the route the kernel replaces: materialised regressors of NSUB windows through dfm_ols_batch_dev
    o = call(SWEEPS, ("win", "F"))
    ctx.synchronize()
    some = np.linspace(0, O - 1, NSUB).astype(int)
    win, Fw = o["win"].cpu().numpy(), o["F"].cpu().numpy()
    Xs, ys = zip(*[regressors(win[b], Fw[b], H, q) for b in some])
    Xd, yd = t(np.concatenate(Xs)), t(np.concatenate(ys))
    P = Xd.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    beta, ssr, nobs = torch.empty((P, Kreg), **f64), torch.empty(P, **f64), torch.empty(P, dtype=torch.int32, device=dev)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())

    def ols():
        rc = ctx._lib.dfm_ols_batch_dev(ctx._h, P, W, Kreg, ptr(Xd), W * Kreg, ptr(yd), W, 1, max(nt_min, Kreg), ptr(beta), None, ptr(ssr), None,
                                        ptr(nobs))
        assert rc == 0, rc
    ctx._sync_stream()
    ols_ms = timed(ols)
    # ... and the host loop around it
    def loop():
        for b in some:
            ob = origins[b]
            z, _ = api.standardize_data(x[ob - W + 1:ob + 1])
            f = ctx.als_batch_host(z, F_path[ob - W + 1:ob + 1][None], nt_min=nt_min, max_iter=SWEEPS, tol=0.0)["F"][0]
            X, y = regressors(z, f, H, q)
            ctx.ols_batch_host(X, np.ascontiguousarray(y.T), nt_min=max(nt_min, Kreg), want_resid=False)

    loop()
    t0 = time.perf_counter(); loop(); loop_ms = (time.perf_counter() - t0) * 1e3 / NSUB * O
    print(json.dumps(dict(workload=name, T=T, N=N, r=r, q=q, K=Kreg, W=W, H=H, O=O, sweeps=SWEEPS, call_ms=round(ms, 3),
                          call_no_als_ms=round(ms0, 3), als_share=round(1.0 - ms0 / ms, 3), kernels_ms=prof, regressions=nreg,
                          regress_us_per_regression=round(reg_ms * 1e3 / nreg, 4), ols_problems=P, ols_ms=round(ols_ms, 4),
                          ols_us_per_regression=round(ols_ms * 1e3 / P, 4), fused_over_ols=round(reg_ms / nreg / (ols_ms / P), 3),
                          regressor_bytes_full=O * N * H * W * Kreg * 8, loop_ms=round(loop_ms, 1), loop_over_call=round(loop_ms / ms, 1))),
          flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 1)
api.estimate_factor(m, max_iter=200, computeR2=False, ctx=ctx)
cols = np.nonzero(m.inclcode == 1)[0]
x = m.data[2:224][:, cols]
W, O = 120, 100
T = x.shape[0]
obs = np.vstack([np.zeros((1, cols.size), dtype=int), np.cumsum(~np.isnan(x), axis=0)])
keep = np.all([obs[o + 1] - obs[o - W + 1] >= 20 for o in range(T - O, T)], axis=0)     # api.forecast_diffusion_index's rule
line("di_sw", np.ascontiguousarray(x[:, keep]), np.ascontiguousarray(m.factor[2:224]), 4, W, 4, O, 20, 20)

T, N, r = 500, 200, 8
panel, _ = ctx.synth_panels(7, 0, 1, T, N, r)
rng = np.random.default_rng(7)
z = panel[0].cpu().numpy()
x = z * rng.uniform(0.5, 3.0, N) + rng.uniform(-2.0, 2.0, N)
_, F0 = ctx.pca_init_batch_host(z[None], r)
line("di_c2", x, np.ascontiguousarray(F0[0]), 4, 250, 12, 250, 20, r + 1)
ctx.close()
