#!/usr/bin/env python
"""Measurement lines of dfm_simsmooth_batch_dev (csrc/simsmooth.hip; run on the GPU box).  Workloads:
  ss_p1_bal   -- B = 1, D = 1024 draws, T = 500, N = 200, r = 8, p = 1, H = 12, a balanced synthetic panel (dfm_synth_panels_dev)
  ss_p1_miss  -- the same with 10 % missing cells
  ss_sw_var4  -- the Stock-Watson window (rows 3..216 fitted, state conditioned on rows 3..224), VAR(4), r = 4, H = 8, D = 1024
Both f_draw and x_draw are written.  Each line: ms per call (median of timed calls after warm-up, HIP events), the per-kernel ms of
one profiled call (dfm_profile_read), the difference and fill kernels' bytes / time beside dfm_hbm_probe's write rate (their
bound: the bytes they write over that rate -- the panel every draw re-reads comes from L2 / the Infinity Cache), the plain pass
(no P) on B D copies of the panel, and the call minus (difference + plain pass + fill).
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
D = 1024


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


probe = ctx.hbm_probe(1 << 30, 10)
read_gbs, write_gbs = probe["read_dma"], probe["write"]


def line(name, panel, params, p, H):
    Lam, R, A, Q, mu0, P0 = params
    B, T, N = panel.shape
    r = Lam.shape[2]
    miss = bool(torch.isnan(panel).any().item())
    call = lambda: ctx.simsmooth_batch(panel, Lam, R, A, Q, mu0, P0, D, H, seed=7, may_have_missing=miss)
    rep = lambda t: t.expand((B * D,) + tuple(t.shape[1:])).contiguous()
    pp = (rep(panel), rep(Lam), rep(R), rep(A), rep(Q), torch.zeros_like(rep(mu0)), rep(P0))
    if p == 1:
        plain = lambda: ctx.ks_pass_batch(*pp, want_P=False, may_have_missing=miss)
    else:
        plain = lambda: ctx.ks_pass_varp_batch(*pp, want_P=False, may_have_missing=miss)
    ms = timed(call)
    ms_plain = timed(plain)
    del pp
    kern = profiled(call)
    pick = lambda stem: sum(v for k, v in kern.items() if k.startswith(stem))
    diff, fill = pick("simsmooth_diff_kernel"), pick("simsmooth_fill_kernel")
    ours = sum(v for k, v in kern.items() if k.startswith("simsmooth_"))
    TH = T + H
    diff_wr = B * D * T * N * 8
    fill_wr = B * D * TH * N * 8
    diff_bound = diff_wr / (write_gbs * 1e6)
    fill_bound = fill_wr / (write_gbs * 1e6)
    print(json.dumps(dict(workload=name, B=B, D=D, T=T, N=N, r=r, p=p, H=H, missing=miss, ms_per_call=round(ms, 4),
                          kernels_ms=kern, pass_kernels_ms=round(sum(kern.values()) - ours, 4), plain_pass_ms=round(ms_plain, 4),
                          hbm_read_gbs=round(read_gbs, 1), hbm_write_gbs=round(write_gbs, 1),
                          diff_bytes_written=diff_wr, diff_ms=round(diff, 4), diff_bound_ms=round(diff_bound, 4),
                          diff_over_bound=round(diff / diff_bound, 3),
                          fill_bytes_written=fill_wr, fill_ms=round(fill, 4), fill_bound_ms=round(fill_bound, 4),
                          fill_over_bound=round(fill / fill_bound, 3),
                          call_minus_diff_plain_fill_ms=round(ms - diff - ms_plain - fill, 4))), flush=True)


for name, miss in (("ss_p1_bal", 0.0), ("ss_p1_miss", 0.1)):
    panel, params = ctx.synth_panels(20261016, 0, 1, 500, 200, 8, miss)
    line(name, panel, params, 1, 12)
    del panel, params
    torch.cuda.empty_cache()

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
cols, z, mu, sd = api._forecast_inputs(m, 224)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a[None])).to(dev)
ep = m.em_params
line("ss_sw_var4", t(z), tuple(t(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")), 4, 8)
ctx.close()
