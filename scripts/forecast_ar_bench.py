#!/usr/bin/env python
"""Measurement lines of dfm_forecast_ar_batch_dev (csrc/forecast_ar.hip; run on the GPU box).  Workloads:
  fcar_q4  -- B = 1024, T = 222, N = 139, r = 4, p = 4, q = 4, H = 8, 10 % missing cells plus a ragged edge
  fcar_q1  -- B = 1024, T = 500, N = 200, r = 4, p = 1, q = 1, H = 12, balanced
Synthetic panels (dfm_synth_panels_dev) with AR coefficients and a VAR(p) written around their VAR(1) parameters.  All outputs
written.  Each line: ms per call (median of 20 timed calls after warm-up, HIP events), the per-kernel ms of the same calls
(dfm_profile_read; median of 20), each new kernel beside its byte bound at dfm_hbm_probe's read and write rates of the same box
(backward: panel and f read once, messages written; forward: panel, f, P and messages read, four cell outputs written), and
the yardstick on the same panel: dfm_forecast_batch at the same p (forecast.hip, untouched by this entry), call and kernels.
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


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ctx.synchronize()
    return float(np.median(ms))


def profiled(fn):
    """Per kernel name: the median over K calls of the summed ms of that kernel's launches in one call."""
    runs = []
    for _ in range(K):
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        fn()
        ctx.synchronize()
        runs.append({k: v[0] for k, v in ctx.profile_read().items()})
        ctx.profile_enable(False)
    return {k: round(float(np.median([r.get(k, 0.0) for r in runs])), 4) for k in runs[0]}


probe = ctx.hbm_probe(1 << 30, 10)
read_gbs, write_gbs = probe["read_dma"], probe["write"]


def line(name, B, T, N, r, p, q, H, miss, ragged):
    panel, (Lam, R, A, Q, mu0, P0) = ctx.synth_panels(20261020, 0, B, T, N, r, miss)
    if ragged:
        panel[:, T - 1, :N // 2] = float("nan")
        panel[:, T - 2, :N // 4] = float("nan")
    g = torch.Generator(device="cpu").manual_seed(7)
    rho = torch.zeros((B, N, q), dtype=torch.float64)
    rho[:, :, 0] = 0.1 + 0.5 * torch.rand((B, N), generator=g, dtype=torch.float64)
    for l in range(1, q):
        rho[:, :, l] = (0.2 * torch.rand((B, N), generator=g, dtype=torch.float64) - 0.1) / l
    rho = rho.to(dev)
    Avar = torch.zeros((B, r, r * p), dtype=torch.float64, device=dev)
    Avar[:, :, :r] = A
    eye = lambda k: torch.eye(k, dtype=torch.float64, device=dev).expand(B, k, k).contiguous()
    zeros = lambda k: torch.zeros((B, k), dtype=torch.float64, device=dev)
    k_ar, k_fc = r * max(p, q + 1), r * p
    has_nan = bool(torch.isnan(panel).any().item())
    m_ar, P_ar, m_fc, P_fc = zeros(k_ar), eye(k_ar), zeros(k_fc), eye(k_fc)
    call = lambda: ctx.forecast_ar_batch_dev(panel, Lam, R, rho, Avar, Q, m_ar, P_ar, H, may_have_missing=has_nan)
    yard = lambda: ctx.forecast_batch(panel, Lam, R, Avar, Q, m_fc, P_fc, H, may_have_missing=has_nan)
    ms, ms_yard = timed(call), timed(yard)
    kern, kern_yard = profiled(call), profiled(yard)
    n = T + H - q
    np_ = r * (r + 1) // 2
    nc = q + q * (q + 1) // 2
    nsblk = (N + 255) // 256
    obs = ~torch.isnan(torch.cat([panel[:, q:], torch.full((B, H, N), float("nan"), dtype=torch.float64, device=dev)], dim=1))
    later = torch.flip(torch.cummax(torch.flip(obs, [1]).to(torch.int8), dim=1)[0], [1]).bool()      # observed at t or later
    stored = int((~obs & later).sum().item())
    cells, par = B * n * N * 8, B * N * (r + q + 1) * 8
    back_rd, back_wr = cells + nsblk * B * n * r * 8 + par, stored * nc * 8 + B * N * 4
    fwd_rd, fwd_wr = cells + nsblk * B * n * (r + np_) * 8 + stored * nc * 8 + par + B * N * 4, 4 * cells
    bound = lambda rd, wr: rd / (read_gbs * 1e6) + wr / (write_gbs * 1e6)
    back, fwd = kern.get("forecast_ar_back_kernel", float("nan")), kern.get("forecast_ar_fwd_kernel", float("nan"))
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, q=q, H=H, missing=miss, ragged=ragged, ms_per_call=round(ms, 4),
                          kernels_ms=kern, stored_messages=stored, message_bytes=stored * nc * 8,
                          back_ms=back, back_bytes=[back_rd, back_wr], back_bound_ms=round(bound(back_rd, back_wr), 4),
                          back_over_bound=round(back / bound(back_rd, back_wr), 2),
                          fwd_ms=fwd, fwd_bytes=[fwd_rd, fwd_wr], fwd_bound_ms=round(bound(fwd_rd, fwd_wr), 4),
                          fwd_over_bound=round(fwd / bound(fwd_rd, fwd_wr), 2),
                          hbm_read_gbs=round(read_gbs, 1), hbm_write_gbs=round(write_gbs, 1),
                          yardstick_forecast_batch_ms=round(ms_yard, 4), yardstick_kernels_ms=kern_yard)), flush=True)
    del panel, Lam, R, A, Q, mu0, P0, rho, Avar, obs, later
    torch.cuda.empty_cache()


line("fcar_q4", 1024, 222, 139, 4, 4, 4, 8, 0.1, True)
line("fcar_q1", 1024, 500, 200, 4, 1, 1, 12, 0.0, False)
ctx.close()
