#!/usr/bin/env python
"""Measurement lines of dfm_simsmooth_ar_batch_dev (csrc/simsmooth_ar.hip; run on the GPU box).  Workloads, B = 1, D = 1024:
  ssar_q4  -- T = 222, N = 139, r = 4, p = 4, q = 4, H = 8, 10 % missing cells plus a ragged edge
  ssar_q1  -- T = 500, N = 200, r = 4, p = 1, q = 1, H = 12, balanced
Synthetic panels (dfm_synth_panels_dev) with the AR coefficients and VAR(p) of scripts/forecast_ar_bench.py.  Each line: ms per
call (median of 20 timed calls after warm-up, HIP events), the per-kernel ms of the same calls (dfm_profile_read; median of 20),
the two new series kernels beside their byte bounds at dfm_hbm_probe's read and write rates of the same box (generator: f+ read
once per series block, the difference panel written; forward: the panel's one replicate is cache-resident, so g, f+ and the stored
messages read, x_draw written), the generator beside simsmooth_diff_kernel of dfm_simsmooth_batch at the same D and cell count,
and the yardstick: dfm_forecast_ar_batch_dev at B = 1024 on the same panel replicated, all cell outputs written.  What the call
costs beyond yardstick + generator + finish is itemised from the kernel table (`other_ms`: expand, path, prep) and `gaps_ms`
(call minus the sum of its kernels: launch gaps, the pass's small kernels not under a profile id).  One JSON line per workload."""
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


def line(name, D, T, N, r, p, q, H, miss, ragged):
    panel, (Lam, R, A, Q, mu0, P0) = ctx.synth_panels(20261020, 0, 1, T, N, r, miss)
    if ragged:
        panel[:, T - 1, :N // 2] = float("nan")
        panel[:, T - 2, :N // 4] = float("nan")
    g = torch.Generator(device="cpu").manual_seed(7)
    rho = torch.zeros((1, N, q), dtype=torch.float64)
    rho[:, :, 0] = 0.1 + 0.5 * torch.rand((1, N), generator=g, dtype=torch.float64)
    for l in range(1, q):
        rho[:, :, l] = (0.2 * torch.rand((1, N), generator=g, dtype=torch.float64) - 0.1) / l
    rho = rho.to(dev)
    Avar = torch.zeros((1, r, r * p), dtype=torch.float64, device=dev)
    Avar[:, :, :r] = A
    eye = lambda b, k: torch.eye(k, dtype=torch.float64, device=dev).expand(b, k, k).contiguous()
    zeros = lambda b, k: torch.zeros((b, k), dtype=torch.float64, device=dev)
    k_ar, k_ss = r * max(p, q + 1), r * p
    has_nan = bool(torch.isnan(panel).any().item())
    m_ar, P_ar = zeros(1, k_ar), eye(1, k_ar)
    call = lambda: ctx.simsmooth_ar_batch_dev(panel, Lam, R, rho, Avar, Q, m_ar, P_ar, D, H, seed=1, may_have_missing=has_nan)
    rep = lambda a: a.expand((D,) + tuple(a.shape[1:])).contiguous()
    yp, yL, yR, yrho, yA, yQ, ym, yP = [rep(a) for a in (panel, Lam, R, rho, Avar, Q, m_ar, P_ar)]
    yard = lambda: ctx.forecast_ar_batch_dev(yp, yL, yR, yrho, yA, yQ, ym, yP, H, may_have_missing=has_nan)
    m_ss, P_ss = zeros(1, k_ss), eye(1, k_ss)
    plain = lambda: ctx.simsmooth_batch(panel, Lam, R, Avar, Q, m_ss, P_ss, D, H, seed=1, may_have_missing=has_nan)
    ms, ms_yard = timed(call), timed(yard)
    kern, kern_yard, kern_plain = profiled(call), profiled(yard), profiled(plain)
    n = T + H - q
    nc = q + q * (q + 1) // 2
    nsblk = (N + 255) // 256
    obs = ~torch.isnan(torch.cat([panel[:, q:], torch.full((1, H, N), float("nan"), dtype=torch.float64, device=dev)], dim=1))
    later = torch.flip(torch.cummax(torch.flip(obs, [1]).to(torch.int8), dim=1)[0], [1]).bool()      # observed at t or later
    stored = D * int((~obs & later).sum().item())
    gen_rd, gen_wr = nsblk * D * n * r * 8, D * (T + H) * N * 8
    fwd_rd, fwd_wr = nsblk * D * n * 2 * r * 8 + stored * nc * 8 + D * N * 4, D * n * N * 8
    bound = lambda rd, wr: rd / (read_gbs * 1e6) + wr / (write_gbs * 1e6)
    gen, fwd = kern.get("simsmooth_ar_diff_kernel", float("nan")), kern.get("simsmooth_ar_fwd_kernel", float("nan"))
    fin = kern.get("simsmooth_ar_finish_kernel", float("nan"))
    other = sum(kern.get(k, 0.0) for k in ("simsmooth_prep_kernel", "simsmooth_expand_kernel", "simsmooth_path_kernel",
                                           "simsmooth_ar_params_kernel", "simsmooth_ar_expand_kernel"))
    plain_diff = kern_plain.get("simsmooth_diff_kernel", float("nan"))
    plain_wr = D * T * N * 8
    print(json.dumps(dict(workload=name, D=D, T=T, N=N, r=r, p=p, q=q, H=H, missing=miss, ragged=ragged, ms_per_call=round(ms, 4),
                          kernels_ms=kern, stored_messages=stored,
                          gen_ms=gen, gen_bytes=[gen_rd, gen_wr], gen_bound_ms=round(bound(gen_rd, gen_wr), 4),
                          gen_over_bound=round(gen / bound(gen_rd, gen_wr), 2),
                          fwd_ms=fwd, fwd_bytes=[fwd_rd, fwd_wr], fwd_bound_ms=round(bound(fwd_rd, fwd_wr), 4),
                          fwd_over_bound=round(fwd / bound(fwd_rd, fwd_wr), 2),
                          finish_ms=fin, other_ms=round(other, 4), gaps_ms=round(ms - sum(kern.values()), 4),
                          simsmooth_diff_kernel_ms=plain_diff,
                          simsmooth_diff_over_write_bound=round(plain_diff / (plain_wr / (write_gbs * 1e6)), 2),
                          gen_over_write_bound=round(gen / (gen_wr / (write_gbs * 1e6)), 2),
                          hbm_read_gbs=round(read_gbs, 1), hbm_write_gbs=round(write_gbs, 1),
                          yardstick_forecast_ar_batch_ms=round(ms_yard, 4), yardstick_kernels_ms=kern_yard)), flush=True)
    del panel, Lam, R, A, Q, mu0, P0, rho, Avar, obs, later, yp, yL, yR, yrho, yA, yQ, ym, yP
    torch.cuda.empty_cache()


line("ssar_q4", 1024, 222, 139, 4, 4, 4, 8, 0.1, True)
line("ssar_q1", 1024, 500, 200, 4, 1, 1, 12, 0.0, False)
ctx.close()
