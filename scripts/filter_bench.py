#!/usr/bin/env python
"""Measurement lines of dfm_filter_batch_dev (csrc/filter.hip; run on the GPU box).  Workloads:
  ft_c2       -- B = 1024, T = 500, N = 200, r = 8, H = 12, t0 = T / 2, balanced (dfm_synth_panels_dev replicates)
  ft_c2_miss  -- the same shape with 10 % missing cells
  ft_sw_var4  -- the Stock-Watson window, VAR(4), r = 4, the fitted parameters broadcast to B = 1024 replicates, H = 12
Each line: ms per call (median of 20 timed calls after warm-up, HIP events); the per-kernel ms of one profiled call
(dfm_profile_read); the fill's HBM bound (panel read at the probe's DMA read rate + three panel-sized writes at its write rate,
the bytes counted as in DESIGN section 10) and fill / bound, beside the forecast fill's figure from a dfm_forecast_batch_dev call
on the same panel; the smoother pass's kernels on the same panel; one panel read at the probe's rate beside the evaluation
kernel; and the loop the call replaces -- dfm_forecast_batch_dev on truncated panels, timed for 8 origins and scaled to T - t0.
Prints one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, api  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, K = 3, 20


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


def line(name, panel, params, p, H):
    Lam, R, A, Q, mu0, P0 = params
    B, T, N = panel.shape
    r = Lam.shape[2]
    t0 = T // 2
    miss = bool(panel.isnan().any().item())
    mean, sd = torch.zeros((B, N), dtype=torch.float64, device=dev), torch.ones((B, N), dtype=torch.float64, device=dev)
    fn = lambda: ctx.filter_batch_dev(panel, Lam, R, A, Q, mu0, P0, H=H, t0=t0, mean=mean, sd=sd, may_have_missing=miss)
    ms, prof = timed(fn), profiled(fn)
    cells = B * T * N * 8
    bound = cells / (probe["read_dma"] * 1e6) + 3 * cells / (probe["write"] * 1e6)
    fill = prof.get("filter_fill_kernel", float("nan"))
    fc = lambda: ctx.forecast_batch(panel, Lam, R, A, Q, mu0, P0, 0, mean=mean, sd=sd, may_have_missing=miss)
    fprof = profiled(fc)
    ps = (lambda: ctx.ks_pass_batch(panel, Lam, R, A, Q, mu0, P0, may_have_missing=miss)) if p == 1 else \
         (lambda: ctx.ks_pass_varp_batch(panel, Lam, R, A, Q, mu0, P0, may_have_missing=miss))
    pass_ms, pprof = timed(ps), profiled(ps)
    # the loop the call replaces: one forecast per origin on the panel cut behind it (8 origins spread over t0 .. T-1, scaled)
    origins = np.linspace(t0, T - 1, 8).astype(int)
    cuts = [panel[:, :t + 1].contiguous() for t in origins]
    loop = lambda: [ctx.forecast_batch(c, Lam, R, A, Q, mu0, P0, H, mean=mean, sd=sd, want_var=False, want_common=False,
                                       want_P=False, may_have_missing=miss) for c in cuts]
    loop_ms = timed(loop, 5) / 8 * (T - t0)
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, H=H, t0=t0, call_ms=round(ms, 4), kernels_ms=prof,
                          read_gbs=round(probe["read_dma"], 1), write_gbs=round(probe["write"], 1), fill_bound_ms=round(bound, 4),
                          fill_over_bound=round(fill / bound, 3),
                          forecast_fill_over_bound=round(fprof.get("forecast_fill_kernel", float("nan")) / bound, 3),
                          pass_ms=round(pass_ms, 4), pass_kernels_ms=pprof,
                          panel_read_ms=round(cells / (probe["read_dma"] * 1e6), 4), eval_ms=prof.get("filter_eval_kernel"),
                          forecast_loop_ms=round(loop_ms, 2), loop_over_call=round(loop_ms / ms, 1))), flush=True)


B, T, N, r = 1024, 500, 200, 8
for name, mp in (("ft_c2", 0.0), ("ft_c2_miss", 0.1)):
    panel, params = ctx.synth_panels(7, 0, B, T, N, r, missing_prob=mp)
    line(name, panel, params, 1, 12)
    del panel, params

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
ep = m.em_params
cols, z, mu, sd = api._forecast_inputs(m, 224)
rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)
line("ft_sw_var4", rep(z), tuple(rep(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")), 4, 12)
ctx.close()
