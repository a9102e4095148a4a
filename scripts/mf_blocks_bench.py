#!/usr/bin/env python
"""Measurement lines of the mixed-frequency EM with fixed loadings (dfm_em_mf_blocks_batch_dev, csrc/mstep_mf_blocks.hip; run on the
GPU box), at scripts/mf_bench.py's shape: B = 1024, T = 222, N = 139, r = 4, p = 4, L = 5, 10 % random missing, 16 distinct panels
tiled, two weight classes (96 monthly series, 43 quarterly flows masked to every third month).
  iteration -- one EM iteration of dfm_em_mf_batch beside one of dfm_em_mf_blocks_batch with a global-plus-three-blocks mask (factor 0
               loads on every series, factors 1 .. 3 on a third of the series each; the start's fixed loadings set to 0).  9 blocks
               per variant, the variants alternating inside one process; median and min-max of the blocks.
  kernels   -- per iteration, from dfm_profile_read: mf_solve_kernel (unrestricted run) and mf_solve_blocks_kernel (masked run) with
               the table and moments kernels beside them.
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
KM = ("Lam", "sig2", "Avar", "Q", "mu0", "P0")
a0 = {k: tile(np.stack([s[k] for s in sts])) for k in KM}
flow = np.array([1, 2, 3, 2, 1]) / 3.0
Wn = np.zeros((N, L)); Wn[:96, 0] = 1.0; Wn[96:] = flow
W = t(Wn)
x = tile(np.stack(xs))
x[:, np.arange(T) % 3 != 2, 96:] = float("nan")
third = np.arange(N) % 3
free_n = api.mf_blocks(np.stack([np.ones(N, bool), third == 0, third == 1, third == 2], axis=1), [1, 1, 1, 1])
free = t(free_n.astype(np.uint8))
b0 = dict(a0, Lam=a0["Lam"] * t(free_n.astype(np.float64)))  # fixed loadings at 0


def block(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / NIT


def run_plain():
    aa = {k: a0[k].clone() for k in KM}
    return lambda: ctx.em_mf_batch(x, aa["Lam"], aa["sig2"], W, aa["Avar"], aa["Q"], aa["mu0"], aa["P0"], max_iter=NIT, want_smooth=False,
                                   may_have_missing=True)


def run_blocks():
    aa = {k: b0[k].clone() for k in KM}
    return lambda: ctx.em_mf_blocks_batch_dev(x, aa["Lam"], aa["sig2"], W, free, aa["Avar"], aa["Q"], aa["mu0"], aa["P0"], max_iter=NIT,
                                              want_smooth=False, may_have_missing=True)


variants = dict(mf_unrestricted=run_plain, mf_blocks_global_plus_three=run_blocks)
ms = {k: [] for k in variants}
for k, mk in variants.items():                                # warm-up: workspace, code objects
    block(mk())
for _ in range(BLOCKS):
    for k, mk in variants.items():
        fn = mk()                                             # (fresh parameters: every block runs the same NIT iterations)
        ms[k].append(block(fn))
for k, v in ms.items():
    print(json.dumps(dict(item="iteration", variant=k, B=B, T=T, N=N, r=r, p=p, state=r * L, blocks=BLOCKS, iterations_per_block=NIT,
                          free_loadings=int(free_n.sum()) if "blocks" in k else N * r,
                          ms_per_iteration_median=round(float(np.median(v)), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))),
          flush=True)

for name, mk in variants.items():
    fn = mk()
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    prof = {k: round(v[0] / NIT, 4) for k, v in ctx.profile_read().items() if k.startswith("mf_")}
    ctx.profile_enable(False)
    print(json.dumps(dict(item="kernels", variant=name, ms_per_iteration=prof)), flush=True)
ctx.close()
