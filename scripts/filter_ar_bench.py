#!/usr/bin/env python
"""Measurement lines of dfm_filter_ar_batch_dev (csrc/filter_ar.hip; run on the GPU box).  Workloads, the shapes of DESIGN section
20's table, both at B = 1024 and H = 12, t0 = the middle of the output rows:
  ftar_q4  -- T = 222, N = 139, r = 4, p = 4, q = 4, 10 % missing cells
  ftar_q1  -- T = 500, N = 200, r = 4, p = 1, q = 1, balanced
Synthetic panels (dfm_synth_panels_dev) with AR coefficients and a VAR(p) written around their VAR(1) parameters, as
scripts/forecast_ar_bench.py.  Each line: ms per call (median of 20 timed calls after warm-up, HIP events); the per-kernel ms of
one profiled call (dfm_profile_read) and filter_ar_kernel's time per period; the fill's HBM bound at the same-box probe's rates
(q + 1 panel rows read per output row count once: the lags come from cache -- one panel read at the DMA read rate plus three
panel-sized writes at the write rate) and fill / bound; one panel read beside the evaluation kernel; and the loop the call
replaces -- dfm_forecast_ar_batch_dev on truncated panels, timed for 4 origins spread over t0 .. T-1 and scaled to T - t0.
Prints one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, K = 3, 20


def timed(fn, k=K, warm=WARM):
    for _ in range(warm):
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
read_gbs, write_gbs = probe["read_dma"], probe["write"]


def line(name, B, T, N, r, p, q, H, miss):
    panel, (Lam, R, A, Q, mu0, P0) = ctx.synth_panels(20261020, 0, B, T, N, r, miss)
    g = torch.Generator(device="cpu").manual_seed(7)
    rho = torch.zeros((B, N, q), dtype=torch.float64)
    rho[:, :, 0] = 0.1 + 0.5 * torch.rand((B, N), generator=g, dtype=torch.float64)
    for l in range(1, q):
        rho[:, :, l] = (0.2 * torch.rand((B, N), generator=g, dtype=torch.float64) - 0.1) / l
    rho = rho.to(dev)
    Avar = torch.zeros((B, r, r * p), dtype=torch.float64, device=dev)
    Avar[:, :, :r] = A
    k = r * max(p, q + 1)
    m_ar = torch.zeros((B, k), dtype=torch.float64, device=dev)
    P_ar = torch.eye(k, dtype=torch.float64, device=dev).expand(B, k, k).contiguous()
    has_nan = bool(torch.isnan(panel).any().item())
    n = T - q
    t0 = q + n // 2
    call = lambda: ctx.filter_ar_batch_dev(panel, Lam, R, rho, Avar, Q, m_ar, P_ar, H=H, t0=t0, may_have_missing=has_nan)
    ms, kern = timed(call), profiled(call)
    cells = B * n * N * 8
    bound = B * T * N * 8 / (read_gbs * 1e6) + 3 * cells / (write_gbs * 1e6)
    fill = kern.get("filter_ar_fill_kernel", float("nan"))
    rec = kern.get("filter_ar_kernel", float("nan"))
    origins = np.linspace(t0, T - 1, 4).astype(int)
    cuts = [panel[:, :t + 1].contiguous() for t in origins]
    loop = lambda: [ctx.forecast_ar_batch_dev(c, Lam, R, rho, Avar, Q, m_ar, P_ar, H, want=(), may_have_missing=has_nan) for c in cuts]
    loop_ms = timed(loop, 3, 1) / 4 * (T - t0)
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, q=q, H=H, t0=t0, missing=miss, call_ms=round(ms, 4), kernels_ms=kern,
                          recursion_us_per_period=round(1e3 * rec / n, 2), read_gbs=round(read_gbs, 1), write_gbs=round(write_gbs, 1),
                          fill_bound_ms=round(bound, 4), fill_over_bound=round(fill / bound, 3),
                          panel_read_ms=round(B * T * N * 8 / (read_gbs * 1e6), 4), eval_ms=kern.get("filter_ar_eval_kernel"),
                          forecast_ar_loop_ms=round(loop_ms, 2), loop_over_call=round(loop_ms / ms, 1))), flush=True)
    del panel, Lam, R, A, Q, mu0, P0, rho, Avar, cuts
    torch.cuda.empty_cache()


line("ftar_q4", 1024, 222, 139, 4, 4, 4, 12, 0.1)
line("ftar_q1", 1024, 500, 200, 4, 1, 1, 12, 0.0)
ctx.close()
