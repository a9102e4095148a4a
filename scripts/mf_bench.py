#!/usr/bin/env python
"""Measurement lines of the mixed-frequency EM (dfm_em_mf_batch_dev, csrc/mstep_mf.hip; run on the GPU box).
  iteration -- bench.py's `ar_em` shape (B = 1024, T = 222, N = 139, r = 4, p = 4, 10 % random missing; 16 distinct panels tiled):
               one ECM iteration of dfm_em_ar_batch with q = 4 (state 20) beside one EM iteration of dfm_em_mf_batch with L = 5
               (state 20, the same pass route) on the same panel and start, (a) all series in ONE weight class (1, 2, 3, 2, 1) / 3,
               (b) two classes: 96 monthly series and 43 quarterly flows, the quarterly series masked to every third month.
               9 blocks per variant, the variants alternating inside one process; median and min-max of the blocks.
  kernels   -- per iteration, from dfm_profile_read: mf_table_kernel, mf_moments_kernel, mf_solve_kernel beside their HBM byte
               bounds at dfm_hbm_probe's rates (table: the smoothed state's moments read, the class rows written; moments: the
               panel read once plus the class table once per series tile, the per-series sums written; solve: those sums read).
  forecast  -- api.forecast_mixed's one call at the real-data shape (T = 360, N = 139, r = 4, p = 4, L = 5: k = 20, B = 1024
               copies of a fit) beside the plain p = 1 forecast of a dense model of the same (B, T, N, k), same flags.
Prints one JSON line per item."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, api  # noqa: E402
from oracle import ar_oracle as aro  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
BLOCKS, NIT = 9, 5

B, N, T, r, p, q, miss = 1024, 139, 222, 4, 4, 4, 0.1
L = q + 1
xs, sts = zip(*[aro.synth_ar(b, N, T, r, p, q, missing=miss) for b in range(16)])
tile = lambda a: t(np.tile(a, (B // 16,) + (1,) * (a.ndim - 1)))
xa = tile(np.stack(xs))
KA = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
a0 = {k: tile(np.stack([s[k] for s in sts])) for k in KA}
KM = ("Lam", "sig2", "Avar", "Q", "mu0", "P0")
flow = np.array([1, 2, 3, 2, 1]) / 3.0
W1 = t(np.tile(flow, (N, 1)))
W2n = np.zeros((N, L)); W2n[:96, 0] = 1.0; W2n[96:] = flow
W2 = t(W2n)
xq = xa.clone()
xq[:, np.arange(T) % 3 != 2, 96:] = float("nan")


def block(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / NIT


def run_ar():
    aa = {k: v.clone() for k, v in a0.items()}
    return lambda: ctx.em_ar_batch(xa, *[aa[k] for k in KA], max_iter=NIT, want_smooth=False)


def run_mf(x, W):
    aa = {k: a0[k].clone() for k in KM}
    return lambda: ctx.em_mf_batch(x, aa["Lam"], aa["sig2"], W, aa["Avar"], aa["Q"], aa["mu0"], aa["P0"], max_iter=NIT, want_smooth=False,
                                   may_have_missing=True)


variants = dict(ar_em=run_ar, mf_one_class=lambda: run_mf(xa, W1), mf_two_classes_quarterly_mask=lambda: run_mf(xq, W2))
ms = {k: [] for k in variants}
for k, mk in variants.items():                                # warm-up: workspace, code objects
    block(mk())
for _ in range(BLOCKS):
    for k, mk in variants.items():
        fn = mk()                                             # (fresh parameters: every block runs the same NIT iterations)
        ms[k].append(block(fn))
for k, v in ms.items():
    print(json.dumps(dict(item="iteration", variant=k, B=B, T=T, N=N, r=r, p=p, state=r * L, blocks=BLOCKS, iterations_per_block=NIT,
                          ms_per_iteration_median=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))),
          flush=True)

probe = ctx.hbm_probe(1 << 30, 10)
rd, wr = probe["read_dma"], probe["write"]
Rk, VW = 32, 32                                               # state 20 padded to 32; class row: 16 (vech) + 16 (E g) columns at r = 4
for name, x, W, C in (("mf_one_class", xa, W1, 1), ("mf_two_classes_quarterly_mask", xq, W2, 2)):
    fn = run_mf(x, W)
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    prof = {k: v[0] / NIT for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    ntiles = (N + 15) // 16 if C == 1 else (96 + 15) // 16 + (43 + 15) // 16
    bound = dict(
        mf_table_kernel=(B * T * (Rk + Rk * (Rk + 1) // 2) * 8) / (rd * 1e6) + (B * T * C * VW * 8) / (wr * 1e6),
        mf_moments_kernel=(B * T * N * 8 + ntiles * B * T * VW * 8) / (rd * 1e6) + (B * N * (VW + 2) * 8) / (wr * 1e6),
        mf_solve_kernel=(B * N * (VW + 2) * 8) / (rd * 1e6) + (B * N * (r + 1) * 8) / (wr * 1e6))
    print(json.dumps(dict(item="kernels", variant=name, classes=C, series_tiles=ntiles, hbm_read_gbs=round(rd, 1), hbm_write_gbs=round(wr, 1),
                          ms_per_iteration={k: round(v, 4) for k, v in prof.items()},
                          bound_ms={k: round(v, 4) for k, v in bound.items()},
                          over_bound={k: round(prof[k] / v, 2) for k, v in bound.items() if k in prof})), flush=True)

# ---- forecast_mixed's call at the real-data shape beside the plain p = 1 forecast of the same (B, T, N, k)
Tm, H = 360, 6
rng = np.random.default_rng(7)
fac = np.zeros((Tm + 4, r))
for s in range(1, Tm + 4):
    fac[s] = 0.7 * fac[s - 1] + rng.standard_normal(r)
lam = rng.standard_normal((N, r))
g = np.stack([sum(W2n[i, l] * fac[4 - l:Tm + 4 - l] for l in range(L)) @ lam[i] for i in range(N)], axis=1)
xm = g + rng.standard_normal((Tm, N))
xm[np.arange(Tm) % 3 != 2, 96:] = np.nan
xm[-2:, :40] = np.nan                                         # a ragged edge
fit = api.estimate_mixed_frequency(xm, W2n, r, p, max_em_iter=5, tol_em=0.0, ctx=ctx)
LamK, M, Qk = api._mf_expanded(fit["Lam"], fit["W"], fit["Avar"], fit["Q"])
k = M.shape[0]
rep = lambda a: t(np.broadcast_to(a[None], (B,) + a.shape))
z = rep((xm - fit["mean"]) / fit["sd"])
mixed = (rep(LamK), rep(fit["R"]), rep(M), rep(Qk), rep(fit["mu0"]), rep(fit["P0"]))
Ad = 0.5 * np.linalg.qr(rng.standard_normal((k, k)))[0]
dense = (rep(rng.standard_normal((N, k)) / np.sqrt(k)), rep(fit["R"]), rep(Ad), rep(np.eye(k)), rep(np.zeros(k)), rep(np.eye(k)))
out = {}
for name, ps in (("forecast_mixed_expanded", mixed), ("plain_p1_dense", dense)):
    fn = lambda: ctx.forecast_batch(z, *ps, H, may_have_missing=True, singular_q=True)
    fn(); torch.cuda.synchronize()
    v = []
    for _ in range(BLOCKS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        v.append(1e3 * (time.perf_counter() - t0))
    ctx.profile_enable(True); fn(); ctx.synchronize()
    prof = {kk: round(vv[0], 4) for kk, vv in ctx.profile_read().items()}
    ctx.profile_enable(False)
    print(json.dumps(dict(item="forecast", variant=name, B=B, T=Tm, N=N, k=k, H=H, ms_per_call_median=round(float(np.median(v)), 4),
                          ms_min=round(min(v), 4), ms_max=round(max(v), 4), kernels_ms=prof)), flush=True)
ctx.close()
