#!/usr/bin/env python
"""Measurement lines of dfm_forecast_batch_dev (csrc/forecast.hip; run on the GPU box).  Workloads:
  fc_p1_bal   -- B = 1024, T = 500, N = 200, r = 8, p = 1, H = 12, balanced synthetic panels (dfm_synth_panels_dev)
  fc_p1_miss  -- the same with 10 % missing cells
  fc_sw_var4  -- the Stock-Watson window (rows 3..216 fitted, state conditioned on rows 3..224), VAR(4), r = 4, H = 8, the
                 fitted parameters broadcast to B = 1024 replicates
Outputs written: xhat, xvar, f, P (common off).  Each line: ms per call (median of timed calls after warm-up, HIP events), the
per-kernel ms of one profiled call (dfm_profile_read), the fill kernel's bytes / time beside dfm_hbm_probe's read and write
rates and the bound bytes_read / read_rate + bytes_written / write_rate, and the plain pass on the same panel.
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
    np_ = r * (r + 1) // 2
    miss = bool(torch.isnan(panel).any().item())
    call = lambda: ctx.forecast_batch(panel, Lam, R, A, Q, mu0, P0, H, want_common=False, may_have_missing=miss)
    if p == 1:
        plain = lambda: ctx.ks_pass_batch(panel, Lam, R, A, Q, mu0, P0, want_P=True, may_have_missing=miss)
    else:
        plain = lambda: ctx.ks_pass_varp_batch(panel, Lam, R, A, Q, mu0, P0, want_P=True, may_have_missing=miss)
    ms = timed(call)
    ms_plain = timed(plain)
    kern = profiled(call)
    fill = kern.get("forecast_fill_kernel", float("nan"))
    TH = T + H
    rows = B * TH * (r + np_) * 8                       # f / P rows staged (p = 1: also written to f_out / P_out)
    rd = B * T * N * 8 + rows + B * N * (r + 1) * 8
    wr = 2 * B * TH * N * 8 + (rows if p == 1 else 0)
    bound = rd / (read_gbs * 1e6) + wr / (write_gbs * 1e6)
    ok = fill == fill
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, H=H, missing=miss, ms_per_call=round(ms, 4),
                          kernels_ms=kern, plain_pass_ms=round(ms_plain, 4),
                          fill_bytes_read=rd, fill_bytes_written=wr, fill_ms=fill,
                          fill_gbs=round((rd + wr) / (fill * 1e6), 1) if ok else None,
                          hbm_read_gbs=round(read_gbs, 1), hbm_write_gbs=round(write_gbs, 1),
                          fill_bound_ms=round(bound, 4), fill_over_bound=round(fill / bound, 3) if ok else None,
                          call_minus_pass_plus_fill_ms=round(ms - ms_plain - fill, 4) if ok else None)), flush=True)


for name, miss in (("fc_p1_bal", 0.0), ("fc_p1_miss", 0.1)):
    panel, params = ctx.synth_panels(20261016, 0, 1024, 500, 200, 8, miss)
    line(name, panel, params, 1, 12)
    del panel, params
    torch.cuda.empty_cache()

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
cols, z, mu, sd = api._forecast_inputs(m, 224)
B = 1024
rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)
ep = m.em_params
line("fc_sw_var4", rep(z), tuple(rep(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")), 4, 8)
ctx.close()
