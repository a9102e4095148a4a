#!/usr/bin/env python
"""Measurement lines of the simulated-panel entries (dfm_simulate_batch_dev, dfm_simulate_ar_batch_dev; csrc/simulate.hip; run on
the GPU box), taken as scripts/mf_bench.py takes its own: 9 blocks per variant, the variants alternating inside one process,
median and min-max of the blocks; kernel times from dfm_profile_read (an event pair around the launch).
  cells   -- simulate_cells_kernel at B = 1, D = 1024 and (T, N, r, p) = (222, 139, 4, 4) and (500, 200, 8, 1), beside
             simsmooth_fill_kernel of dfm_simsmooth_batch_dev on an ALL-NaN panel of the same shape (it then writes the same bytes
             with the same Philox work per cell) and beside the write bound D T N 8 bytes at dfm_hbm_probe's write rate.
  ar      -- simulate_ar_cells_kernel at the same shapes with q = 4 (q = 3 at r = 8: r (q + 1) <= 32) beside
             simsmooth_ar_diff_kernel of dfm_simsmooth_ar_batch_dev on the same panel.
  e2e     -- wall time of the replicate-panel generation at nrep = 1024, factor_lags = 1 (T = 222, N = 139, r = 4, 10 % missing):
             the host loop of api._bootstrap_replicates beside draws="device" (dfm_simulate_batch_dev; resident, and copied back).
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
from dynamic_factor_models_amd._lib import DfmError  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
BLOCKS, D = 9, 1024
probe = ctx.hbm_probe(1 << 30, 10)


def model(N, T, r, p, q):
    rng = np.random.default_rng([3, N, T, r, p, q])
    k = r * (max(p, q + 1) if q else p)
    A = np.hstack([(0.5 / p) * np.eye(r) + 0.1 / (p * np.sqrt(r)) * rng.standard_normal((r, r)) for _ in range(p)])
    G, H = rng.standard_normal((r, r)), rng.standard_normal((k, k))
    st = [rng.standard_normal((1, N, r)), rng.uniform(0.3, 1.5, (1, N))]
    if q:
        st.append(rng.uniform(-0.4, 0.5, (1, N, q)) / q)
    st += [A[None], (G @ G.T / r + 0.2 * np.eye(r))[None], np.zeros((1, k)), (H @ H.T / k + 0.1 * np.eye(k))[None]]
    return [t(a) for a in st], rng


def kernel_ms(fn, name):
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    ms = ctx.profile_read()[name][0]
    ctx.profile_enable(False)
    return ms


def compare(item, variants, nbytes, extra):
    try:
        for fn, name in variants.values():                   # warm-up: workspace, code objects
            kernel_ms(fn, name)
    except DfmError as err:                                  # (a status of the library, not a fault: say so and go on)
        ctx.profile_enable(False)
        print(json.dumps(dict(item=item, **extra, error=str(err))), flush=True)
        return
    ms = {k: [] for k in variants}
    for _ in range(BLOCKS):
        for k, (fn, name) in variants.items():
            ms[k].append(kernel_ms(fn, name))
    keys = list(variants)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    bound = nbytes / (probe["write"] * 1e6)
    print(json.dumps(dict(item=item, **extra, blocks=BLOCKS, bytes_written=nbytes, hbm_write_gbs=round(probe["write"], 1),
                          write_bound_ms=round(bound, 4),
                          kernels={k: dict(kernel=variants[k][1], ms_median=round(med[k], 4), ms_min=round(min(ms[k]), 4),
                                           ms_max=round(max(ms[k]), 4), gbs=round(nbytes / med[k] / 1e6, 1)) for k in keys},
                          new_over_old=round(med[keys[0]] / med[keys[1]], 3), new_over_write_bound=round(med[keys[0]] / bound, 3))),
          flush=True)


for T, N, r, p, q in ((222, 139, 4, 4, 4), (500, 200, 8, 1, 3)):
    P, rng = model(N, T, r, p, 0)
    nanp = torch.full((1, T, N), float("nan"), dtype=torch.float64, device=dev)
    compare("cells", dict(
        simulate=(lambda: ctx.simulate_batch(*P, D=D, T=T, seed=1), "simulate_cells_kernel"),
        simsmooth_fill=(lambda: ctx.simsmooth_batch(nanp, *P, D, 0, seed=1, may_have_missing=True), "simsmooth_fill_kernel")),
        D * T * N * 8, dict(D=D, T=T, N=N, r=r, p=p))
    Pa, rng = model(N, T, r, p, q)
    xa = t(rng.standard_normal((1, T, N)))
    compare("ar", dict(
        simulate_ar=(lambda: ctx.simulate_ar_batch(*Pa, D=D, panel=xa, seed=1), "simulate_ar_cells_kernel"),
        simsmooth_ar_diff=(lambda: ctx.simsmooth_ar_batch_dev(xa, *Pa, D, 0, seed=1, want_x=False, may_have_missing=True),
                           "simsmooth_ar_diff_kernel")),
        D * T * N * 8, dict(D=D, T=T, N=N, r=r, p=p, q=q))

# ---- end to end: the replicate panels of estimate(..., nrep = 1024, factor_lags = 1)
T, N, r, nrep = 222, 139, 4, 1024
P, rng = model(N, T, r, 1, 0)
z = rng.standard_normal((T, N))
z[rng.uniform(size=z.shape) < 0.1] = np.nan
Lam, R, A, Q, mu0, P0 = (a[0].cpu().numpy() for a in P)


def host_loop():
    g = np.random.default_rng(11)
    LQ, LS, sq = api._psd_sqrt(Q), api._psd_sqrt(P0), np.sqrt(R)
    panels = np.empty((nrep, T, N))
    for b in range(nrep):
        f = mu0 + LS @ g.standard_normal(r)
        for s in range(T):
            f = A @ f + LQ @ g.standard_normal(r)
            panels[b, s] = Lam @ f + sq * g.standard_normal(N)
    panels[:, np.isnan(z)] = np.nan
    return panels


def wall(fn, n):
    v = []
    for _ in range(n):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        v.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(float(np.median(v)), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3), runs=n)


zd = t(z[None])
resident = lambda: ctx.simulate_batch(*P, D=nrep, mask_panel=zd, seed=11, want_f=False)
resident()
print(json.dumps(dict(item="e2e", nrep=nrep, T=T, N=N, r=r, host_loop=wall(host_loop, 3), device_resident=wall(resident, BLOCKS),
                      device_copied_back=wall(lambda: resident()["x"].cpu(), BLOCKS))), flush=True)
ctx.close()
