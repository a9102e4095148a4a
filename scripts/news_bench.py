#!/usr/bin/env python
"""Measurement lines of dfm_news_batch_dev (csrc/news.hip; run on the GPU box).  Workloads:
  nw1         -- B = 1024, T = 500, N = 200, r = 8, p = 1, G = 2, a balanced synthetic panel (dfm_synth_panels_dev); the new vintage
                 adds the last row, half observed; targets: a cell of that row and one at T + 2
  nw_sw_var4  -- the Stock-Watson window (rows 3..216 fitted), VAR(4), r = 4, N = 139, B = 1024 copies of the fit; old = rows
                 3..222, new = rows 3..224 (T = 222); G = 4 targets at periods 224 and 226
Each workload is run without and with `weight` (news is always written).  Each line: ms per call (median of timed calls after
warm-up, HIP events), the per-kernel ms of one profiled call (dfm_profile_read), the forecast and pass kernels the call launches,
the call minus those, and the cell kernels beside their bounds: news_cov_panel_kernel's written bytes over dfm_hbm_probe's write
rate; news_impact_kernel's bytes over the read rate (the covariance panels, plus the new, old and revised-old xhat panels once per
replicate -- its G targets run next to each other -- plus, with weight, the weights written in place over the write rate).
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


def line(name, old, new, params, p, targets):
    Lam, R, A, Q, mu0, P0 = params
    B, T, N = new.shape
    r = Lam.shape[2]
    G = len(targets)
    miss = bool(torch.isnan(new).any().item())
    for want_weight in (False, True):
        call = lambda: ctx.news_batch(old, new, Lam, R, A, Q, mu0, P0, targets, want_weight=want_weight, may_have_missing=miss)
        ms = timed(call)
        kern = profiled(call)
        pick = lambda stem: sum(v for k, v in kern.items() if k.startswith(stem))
        ours = pick("news_") + pick("simsmooth_expand_kernel")
        cov, imp, gam = pick("news_cov_panel_kernel"), pick("news_impact_kernel"), pick("news_gamma_kernel")
        cov_wr = B * G * T * N * 8
        imp_rd = (B * G * T * N + 3 * B * T * N) * 8
        imp_wr = (B * G * T * N * 8 if want_weight else 0) + B * T * N * 8
        cov_bound = cov_wr / (write_gbs * 1e6)
        imp_bound = imp_rd / (read_gbs * 1e6) + imp_wr / (write_gbs * 1e6)
        print(json.dumps(dict(workload=name, weight=want_weight, B=B, T=T, N=N, r=r, p=p, G=G, missing=miss,
                              ms_per_call=round(ms, 4), kernels_ms=kern, forecast_and_pass_ms=round(sum(kern.values()) - ours, 4),
                              call_minus_forecast_and_pass_ms=round(ms - (sum(kern.values()) - ours), 4),
                              hbm_read_gbs=round(read_gbs, 1), hbm_write_gbs=round(write_gbs, 1), gamma_ms=round(gam, 4),
                              cov_bytes_written=cov_wr, cov_ms=round(cov, 4), cov_bound_ms=round(cov_bound, 4),
                              cov_over_bound=round(cov / cov_bound, 3), impact_bytes_read=imp_rd, impact_bytes_written=imp_wr,
                              impact_ms=round(imp, 4), impact_bound_ms=round(imp_bound, 4),
                              impact_over_bound=round(imp / imp_bound, 3))), flush=True)
        torch.cuda.empty_cache()


B, T, N, r = 1024, 500, 200, 8
panel, params = ctx.synth_panels(20261016, 0, B, T, N, r, 0.0)
new = panel.clone()
new[:, T - 1, N // 2:] = float("nan")                         # the new vintage adds the last row, half observed
old = panel.clone()
old[:, T - 1, :] = float("nan")
line("nw1", old, new, params, 1, [(T - 1, 0), (T + 1, 3)])
del panel, params, new, old
torch.cuda.empty_cache()

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
cols, z, mu, sd = api._forecast_inputs(m, 224)
zo = z.copy()
zo[222 - 2:] = np.nan
t = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a[None], (1024,) + a.shape))).to(dev)
ep = m.em_params
line("nw_sw_var4", t(zo), t(z), tuple(t(ep[k]) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")), 4,
     [(221, 0), (221, 1), (223, 0), (223, 1)])
ctx.close()
