#!/usr/bin/env python
"""Measurement lines of dfm_rolling_eval_batch_dev (csrc/rolling.hip; run on the GPU box).  Workloads:
  rw_sw_p1, rw_sw_p4  -- the Stock-Watson panel, rows 3..224 in data units, r = 4, p = 1 and 4, W = 120, H = 4, the last 100
                         origins, 20 EM iterations from the full-sample fit
  rw_c2               -- T = 500, N = 200, r = 8, W = 250, H = 12, the last 250 origins, balanced (a dfm_synth_panels_dev
                         replicate put into data units), 20 EM iterations from the DGP's parameters
Each line: ms per call (median of 20 timed calls after warm-up, HIP events); the same with max_iter = 0 (windows, start, forecasts,
scores: what is left is the EM's share); the per-kernel ms of one profiled call (dfm_profile_read); rolling_window_kernel over
its write bound O W N 8 B at the probe's write rate; rolling_score_kernel beside the bytes it reads (xhat, xvar and x on the
target rows) at the probe's read rate; and the loop the call replaces -- per origin a window standardised on the host, one
single-window EM call and one forecast call through the host entries, timed for 8 origins (wall clock) and scaled to O.
Prints one JSON line per workload."""
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
WARM, K = 3, 20
KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def timed(fn, k=K):
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


probe = ctx.hbm_probe(1 << 30, 10)


def line(name, x, start, sd_start, p, W, H, O, iters, min_obs):
    """x [T, N] raw, start by KEYS [1, ..] in the units of sd_start: NumPy."""
    T, N = x.shape
    r = start["Lam"].shape[2]
    origins = np.arange(T - O, T)
    miss = bool(np.isnan(x).any())
    xd, sd_d = t(x), t(sd_start)
    sp = [t(start[k]) for k in KEYS]
    call = lambda it: ctx.rolling_eval_batch(xd, origins, W, H, *sp, sd_start=sd_d, min_obs=min_obs, max_iter=it, tol=0.0,
                                             may_have_missing=miss)
    ms, ms0, prof = timed(lambda: call(iters)), timed(lambda: call(0)), profiled(lambda: call(iters))
    wbound = O * W * N * 8 / (probe["write"] * 1e6)
    sbytes = 3 * O * (H + 1) * N * 8
    # the loop the call replaces, through the host entries
    some = np.linspace(0, O - 1, 8).astype(int)
    one = {k: start[k] for k in KEYS}

    def loop():
        for b in some:
            o = origins[b]
            w = x[o - W + 1:o + 1]
            n = (~np.isnan(w)).sum(axis=0)
            mu = np.nansum(w, axis=0) / n
            z, sd = api.standardize_data(w)
            sc = sd_start / sd[0]
            args = (z[None], one["Lam"] * sc[None, :, None], one["R"] * sc * sc, one["Avar"], one["Q"], one["mu0"], one["P0"])
            em = ctx.em_batch_host if p == 1 else ctx.em_varp_batch_host
            q = em(*args, max_iter=iters, tol=0.0, may_have_missing=miss)[0]
            ctx.forecast_batch_host(z[None], q["Lam"], q["R"], q["A" if p == 1 else "Avar"], q["Q"], q["mu0"], q["P0"], H,
                                    mean=mu[None], sd=sd, want_common=False, want_P=False, may_have_missing=miss)

    loop()
    t0 = time.perf_counter(); loop(); loop_ms = (time.perf_counter() - t0) * 1e3 / 8 * O
    win, sco = prof.get("rolling_window_kernel", float("nan")), prof.get("rolling_score_kernel", float("nan"))
    print(json.dumps(dict(workload=name, T=T, N=N, r=r, p=p, W=W, H=H, O=O, iters=iters, call_ms=round(ms, 3),
                          call_no_em_ms=round(ms0, 3), em_share=round(1.0 - ms0 / ms, 3), kernels_ms=prof,
                          write_gbs=round(probe["write"], 1), read_gbs=round(probe["read_dma"], 1),
                          window_ms=win, window_bound_ms=round(wbound, 5), window_over_bound=round(win / wbound, 2),
                          score_ms=sco, score_read_bytes=sbytes, score_read_ms_at_probe=round(sbytes / (probe["read_dma"] * 1e6), 5),
                          loop_ms=round(loop_ms, 1), loop_over_call=round(loop_ms / ms, 1))), flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
for p in (1, 4):
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, p)
    api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=p, ctx=ctx)
    cols, _, _, sd_full = api._forecast_inputs(m, 224)
    x = m.data[2:224][:, cols]
    W, O = 120, 100
    T = x.shape[0]
    obs = np.vstack([np.zeros((1, cols.size), dtype=int), np.cumsum(~np.isnan(x), axis=0)])
    keep = np.all([obs[o + 1] - obs[o - W + 1] >= 20 for o in range(T - O, T)], axis=0)     # api.evaluate_forecasts_rolling's rule
    ep = m.em_params
    start = dict(Lam=ep["Lam"][keep][None], R=ep["R"][keep][None], Avar=ep["Avar" if p > 1 else "A"][None], Q=ep["Q"][None],
                 mu0=ep["mu0"][None], P0=ep["P0"][None])
    line(f"rw_sw_p{p}", np.ascontiguousarray(x[:, keep]), start, sd_full[keep], p, W, 4, O, 20, 20)

T, N, r = 500, 200, 8
panel, params = ctx.synth_panels(7, 0, 1, T, N, r)
rng = np.random.default_rng(7)
scale, shift = rng.uniform(0.5, 3.0, N), rng.uniform(-2.0, 2.0, N)
x = panel[0].cpu().numpy() * scale + shift
start = {k: a.cpu().numpy() for k, a in zip(KEYS, params)}
line("rw_c2", x, start, scale, 1, 250, 12, 250, 20, r + 1)
ctx.close()
