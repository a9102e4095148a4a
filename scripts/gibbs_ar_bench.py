#!/usr/bin/env python
"""Measurement lines of the Gibbs sampler of the model with AR idiosyncratic terms (csrc/gibbs_ar.hip, the driver loop in capi.hip;
run on the GPU box).  B = 1024 chains on the two shapes of scripts/simsmooth_ar_bench.py:
  gbar_q4  -- T = 222, N = 139, r = 4, p = 4, q = 4, 10 % missing cells plus a ragged edge
  gbar_q1  -- T = 500, N = 200, r = 4, p = 1, q = 1, balanced
Synthetic panels (dfm_synth_panels_dev) with that script's AR coefficients and VAR(p).  Each line: ms per sweep (median of timed
calls of SWEEPS sweeps after warm-up, HIP events; nothing is kept), the per-kernel ms of one profiled sweep (dfm_profile_read),
gibbs_ar_series_kernel beside its read bound (the n output rows of the panel and the factor path once per series block, over
dfm_hbm_probe's read rate of the same box: the second walk's reads are expected from cache -- the ratio says whether they are),
and two yardsticks measured in the same run: one path step (dfm_simsmooth_ar_batch_dev at D = 1, f only), which the series kernel
plus gibbs_var_kernel should not exceed, and gibbs_load_kernel<RB, true> of dfm_gibbs_batch at the same N, T, r (one walk, no
rejection loop).  Prints one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, bayes  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, K, SWEEPS = 2, 10, 5
B = 1024


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
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {k: round(v[0], 4) for k, v in prof.items()}


read_gbs = ctx.hbm_probe(1 << 30, 10)["read_dma"]


def line(name, T, N, r, p, q, miss, ragged):
    panel, (Lam, R, A, Q, _, _) = ctx.synth_panels(20261020, 0, B, T, N, r, miss)
    if ragged:
        panel[:, T - 1, :N // 2] = float("nan")
        panel[:, T - 2, :N // 4] = float("nan")
    g = torch.Generator(device="cpu").manual_seed(7)
    rho = torch.zeros((1, N, q), dtype=torch.float64)
    rho[:, :, 0] = 0.1 + 0.5 * torch.rand((1, N), generator=g, dtype=torch.float64)
    for l in range(1, q):
        rho[:, :, l] = (0.2 * torch.rand((1, N), generator=g, dtype=torch.float64) - 0.1) / l
    rho = rho.expand(B, N, q).contiguous().to(dev)
    Avar = torch.zeros((B, r, r * p), dtype=torch.float64, device=dev)
    Avar[:, :, :r] = A
    eye = lambda k: torch.eye(k, dtype=torch.float64, device=dev).expand(B, k, k).contiguous()
    zeros = lambda k: torch.zeros((B, k), dtype=torch.float64, device=dev)
    k_ar, k_ss = r * max(p, q + 1), r * p
    has_nan = bool(torch.isnan(panel).any().item())
    m_ar, P_ar, m_ss, P_ss = zeros(k_ar), eye(k_ar), zeros(k_ss), eye(k_ss)
    state = (Lam, R, rho, Avar, Q)
    start = [t.clone() for t in state]
    prior = bayes.default_prior_ar(r)

    def sweeps(n):
        for dst, src in zip(state, start):                          # every timed call runs the same sweeps from the same state
            dst.copy_(src)
        ctx.gibbs_ar_batch(panel, *state, m_ar, P_ar, prior, n, seed=7, keep=(), may_have_missing=has_nan)

    def plain(n):                                                   # dfm_gibbs_batch on the same panel: gibbs_load_kernel<RB, true>
        for dst, src in zip((Lam, R, Avar, Q), (start[0], start[1], start[3], start[4])):
            dst.copy_(src)
        ctx.gibbs_batch(panel, Lam, R, Avar, Q, m_ss, P_ss, bayes.default_prior(r), n, seed=7, keep=(), may_have_missing=True)

    draw = lambda: ctx.simsmooth_ar_batch_dev(panel, *start, m_ar, P_ar, 1, 0, seed=7, want_x=False, may_have_missing=has_nan)
    ms = timed(lambda: sweeps(SWEEPS)) / SWEEPS
    ms_draw = timed(draw)
    kern = profiled(lambda: sweeps(1))
    kern_plain = profiled(lambda: plain(1))
    pick = lambda d, stem: sum(v for k, v in d.items() if k.startswith(stem))
    series, var = pick(kern, "gibbs_ar_series_kernel"), pick(kern, "gibbs_var_kernel")
    load = pick(kern_plain, "gibbs_load_kernel")
    n = T - q
    nsblk = (N + 255) // 256
    series_bytes = B * (n * N + nsblk * n * r + 2 * N * (r + q + 1)) * 8
    bound = series_bytes / (read_gbs * 1e6)
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, q=q, missing=miss, ragged=ragged, ms_per_sweep=round(ms, 4),
                          kernels_ms=kern, series_ms=round(series, 4), var_ms=round(var, 4), path_step_ms=round(ms_draw, 4),
                          series_plus_var_over_path_step=round((series + var) / ms_draw, 3), hbm_read_gbs=round(read_gbs, 1),
                          series_bytes=series_bytes, series_bound_ms=round(bound, 4), series_over_bound=round(series / bound, 3),
                          gibbs_load_kernel_ms=round(load, 4), series_over_gibbs_load=round(series / load, 3))), flush=True)
    del panel, Lam, R, A, Q, rho, Avar, start
    torch.cuda.empty_cache()


line("gbar_q4", 222, 139, 4, 4, 4, 0.1, True)
line("gbar_q1", 500, 200, 4, 1, 1, 0.0, False)
ctx.close()
