#!/usr/bin/env python
"""Measurement lines of the Gibbs sampler (csrc/gibbs.hip, the driver loop in capi.hip; run on the GPU box).  B = 1024 chains:
  gb_p1_bal   -- T = 500, N = 200, r = 8, p = 1, balanced synthetic panels (dfm_synth_panels_dev), the shared-Gram route
  gb_p1_miss  -- the same with 10 % missing cells (a Gram matrix per series)
  gb_sw_var4  -- the Stock-Watson window (rows 3..216), VAR(4), r = 4, every chain on the same panel
Each line: ms per sweep (median of timed calls of SWEEPS sweeps after warm-up, HIP events; nothing is kept), the per-kernel ms of
one profiled sweep (dfm_profile_read), gibbs_load_kernel beside its read bound (the panel plus the factor path over
dfm_hbm_probe's read rate), and the two new kernels together beside one path draw of the same shape (the simulation smoother at
B = 1024, D = 1, H = 0, f only): the aim is new kernels <= one path draw, so that a sweep costs at most about two.
Prints one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, api, bayes  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, K, SWEEPS = 2, 10, 10
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


def line(name, panel, params, p):
    Lam, R, A, Q, mu0, P0 = params
    _, T, N = panel.shape
    r = Lam.shape[2]
    miss = bool(torch.isnan(panel).any().item())
    prior = bayes.default_prior(r)
    start = [t.clone() for t in (Lam, R, A, Q)]

    def sweeps(n):
        for dst, src in zip((Lam, R, A, Q), start):                 # every timed call runs the same sweeps from the same state
            dst.copy_(src)
        ctx.gibbs_batch(panel, Lam, R, A, Q, mu0, P0, prior, n, seed=7, keep=(), may_have_missing=miss)

    draw = lambda: ctx.simsmooth_batch(panel, *start, mu0, P0, 1, 0, seed=7, want_x=False, may_have_missing=miss)
    ms = timed(lambda: sweeps(SWEEPS)) / SWEEPS
    ms_draw = timed(draw)
    kern = profiled(lambda: sweeps(1))
    pick = lambda stem: sum(v for k, v in kern.items() if k.startswith(stem))
    load, var, gram = pick("gibbs_load_kernel"), pick("gibbs_var_kernel"), pick("gibbs_gram_kernel")
    load_bytes = B * (T * N + T * r) * 8
    bound = load_bytes / (read_gbs * 1e6)
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, missing=miss, ms_per_sweep=round(ms, 4), kernels_ms=kern,
                          gibbs_kernels_ms=round(load + var + gram, 4), path_draw_ms=round(ms_draw, 4),
                          gibbs_over_path_draw=round((load + var + gram) / ms_draw, 3), hbm_read_gbs=round(read_gbs, 1),
                          load_bytes_read=load_bytes, load_ms=round(load, 4), load_bound_ms=round(bound, 4),
                          load_over_bound=round(load / bound, 3))), flush=True)


for name, missing in (("gb_p1_bal", 0.0), ("gb_p1_miss", 0.1)):
    panel, params = ctx.synth_panels(20261018, 0, B, 500, 200, 8, missing)
    line(name, panel, params, 1)
    del panel, params
    torch.cuda.empty_cache()

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
cols, z, mu, sd = api._forecast_inputs(m, m.lastperiod)
t = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)
ep = m.em_params
line("gb_sw_var4", t(z), tuple(t(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")), 4)
ctx.close()
