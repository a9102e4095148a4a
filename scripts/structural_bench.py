#!/usr/bin/env python
"""Measurement lines of dfm_irf_batch_dev and dfm_histdecomp_batch_dev (csrc/structural.hip; run on the GPU box).  Workloads:
  sv_irf      -- B = 1024, N = 200, r = 8, p = 1, H = 40, named series, fevd on (dfm_synth_panels_dev parameters)
  sv_hd       -- the same replicates, T = 500 balanced panels
  sv_sw_var4  -- the Stock-Watson window, VAR(4), r = 4, the fitted parameters broadcast to B = 1024 replicates: IRF (H = 40) and
                 the decomposition
Each line: ms per call (median of timed calls after warm-up, HIP events), the per-kernel ms of one profiled call
(dfm_profile_read), and for the two fill kernels the written bytes over dfm_hbm_probe's write rate as the bound and fill / bound;
sv_path_kernel's microseconds per dependent row.  Prints one JSON line per workload."""
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


write_gbs = ctx.hbm_probe(1 << 30, 10)["write"]


def greedy_named(Lam):
    res, out = Lam.astype(float).copy(), []
    for _ in range(Lam.shape[1]):
        nrm = np.linalg.norm(res, axis=1)
        nrm[out] = -1.0
        i = int(np.argmax(nrm))
        out.append(i)
        q = res[i] / np.linalg.norm(res[i])
        res = res - np.outer(res @ q, q)
    return out


def irf_line(name, Lam, A, Q, R, H, named):
    B, N, r = Lam.shape
    fn = lambda: ctx.irf_batch(Lam, A, Q, R, H, named=named)
    ms, prof = timed(fn), profiled(fn)
    bound = B * (2 * r + 1) * H * N * 8 / (write_gbs * 1e6)
    fill = prof.get("sv_irf_fill_kernel", float("nan"))
    print(json.dumps(dict(workload=name, B=B, N=N, r=r, H=H, call_ms=round(ms, 4), kernels_ms=prof, write_gbs=round(write_gbs, 1),
                          fill_bound_ms=round(bound, 4), fill_over_bound=round(fill / bound, 3))), flush=True)


def hd_line(name, panel, params, p, named):
    Lam, R, A, Q, mu0, P0 = params
    B, T, N = panel.shape
    r = Lam.shape[2]
    miss = bool(panel.isnan().any().item())
    fn = lambda: ctx.histdecomp_batch(panel, Lam, R, A, Q, mu0, P0, named=named, may_have_missing=miss)
    ms, prof = timed(fn), profiled(fn)
    bound = B * (r + 1) * T * N * 8 / (write_gbs * 1e6)
    fill = prof.get("sv_hd_fill_kernel", float("nan"))
    print(json.dumps(dict(workload=name, B=B, T=T, N=N, r=r, p=p, call_ms=round(ms, 4), kernels_ms=prof,
                          write_gbs=round(write_gbs, 1), fill_bound_ms=round(bound, 4), fill_over_bound=round(fill / bound, 3),
                          path_us_per_row=round(1e3 * prof.get("sv_path_kernel", float("nan")) / T, 3))), flush=True)


B, T, N, r = 1024, 500, 200, 8
panel, (Lam, R, A, Q, mu0, P0) = ctx.synth_panels(7, 0, B, T, N, r)
named = greedy_named(Lam[0].cpu().numpy())
irf_line("sv_irf", Lam, A, Q, R, 40, named)
hd_line("sv_hd", panel, (Lam, R, A, Q, mu0, P0), 1, named)

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
ep = m.em_params
cols, z, mu, sd = api._forecast_inputs(m, 224)
rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)
pr = tuple(rep(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0"))
named = greedy_named(ep["Lam"])
irf_line("sv_sw_var4_irf", pr[0], pr[2], pr[3], pr[1], 40, named)
hd_line("sv_sw_var4_hd", rep(z), pr, 4, named)
ctx.close()
