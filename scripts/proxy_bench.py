#!/usr/bin/env python
"""Measurement lines of dfm_proxyirf_batch_dev (csrc/proxy.hip; run on the GPU box).  Shapes: (N 200, r 8, p 1, H 40, T 500) on
dfm_synth_panels_dev panels and parameters, and the Stock-Watson shape (N 139, r 4, p 4, H 40, T 222) on the fitted parameters, each
at B = 1024 replicates x D = 15 block draws and at B = 1, D = 16383.  The instrument is noise with a few gaps: the timing does not
depend on its values.
Each line: ms per call (median of timed calls after warm-up, HIP events; the call includes the smoother pass), the per-kernel ms of
one profiled call (dfm_profile_read), px_moment_kernel's nanoseconds per slot, and for the fill the written bytes (irf and fevd)
over dfm_hbm_probe's write rate as the bound.  The yardstick is what the parent commit offers: the same block resampling of the
instrument moment in NumPy on the host, from f_out of dfm_histdecomp_batch; its nanoseconds per draw are reported beside the
kernel's.  Prints one JSON line per workload."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext, api  # noqa: E402

ctx = DfmContext()
dev = torch.device("cuda", ctx.device)
WARM, REP = 2, 7


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REP):
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


def instrument(T, p):
    z = np.random.default_rng(3).standard_normal(T)
    z[p - 1] = np.nan; z[T - 1] = np.nan; z[T // 2:T // 2 + 3] = np.nan
    return z


def block_length(z, p):
    return int(np.ceil(int(np.isfinite(z[p:]).sum()) ** (1.0 / 3.0) - 1e-12))


def proxy_line(name, panel, P, H, D, p):
    B, T, N = panel.shape
    r = P[0].shape[2]
    z = instrument(T, p)
    L = block_length(z, p)
    fn = lambda: ctx.proxyirf_batch(panel, *P, H, z, 0, draws=D, block=L, seed=1, want_fevd=True, may_have_missing=False)
    ms, prof = timed(fn), profiled(fn)
    slots = B * (D + 1)
    bound = slots * 2 * H * N * 8 / (write_gbs * 1e6)
    fill, mom = prof["px_fill_kernel"], prof["px_moment_kernel"]       # (a missing kernel is an error, not a NaN in the table)
    print(json.dumps(dict(workload=name, B=B, D=D, T=T, N=N, r=r, p=p, H=H, L=L, call_ms=round(ms, 4), kernels_ms=prof,
                          moment_ns_per_slot=round(1e6 * mom / slots, 3), write_gbs=round(write_gbs, 1), fill_bound_ms=round(bound, 4),
                          fill_over_bound=round(fill / bound, 3))), flush=True)


def yardstick_line(name, panel, P, D, p):
    """One replicate: f_out of dfm_histdecomp_batch, then etahat, D moving block resamples of the n used rows and their centred
    moments, Q^-1 m and the normalisation in NumPy (vectorised over the draws)."""
    T = panel.shape[1]
    Lam, R, A, Q = (x[0].cpu().numpy() for x in P[:4])
    r = Lam.shape[1]
    z = instrument(T, p)
    L = block_length(z, p)
    f = ctx.histdecomp_batch(panel[:1], *[x[:1] for x in P])["f"][0].cpu().numpy()
    ctx.synchronize()
    g = np.random.default_rng(1)
    t0 = time.perf_counter()
    eta = f[p:].copy()
    for j in range(p):
        eta -= f[p - 1 - j:T - 1 - j] @ A[:, j * r:(j + 1) * r].T
    U = np.nonzero(np.isfinite(z[p:]))[0]
    n, nb = U.size, -(-U.size // L)
    e, zu = eta[U], z[p:][U]
    starts = g.integers(0, n - L + 1, size=(D, nb))
    idx = (starts[:, :, None] + np.arange(L)[None, None, :]).reshape(D, nb * L)[:, :n]
    zs = zu[idx]
    zc = zs - zs.mean(axis=1, keepdims=True)
    m = np.einsum("dnc,dn->dc", e[idx], zc) / n
    gq = np.linalg.solve(Q, m.T).T
    kappa = np.einsum("dc,dc->d", m, gq)
    hvec = m / np.sqrt(kappa)[:, None]
    hvec *= np.where(hvec @ Lam[0] < 0.0, -1.0, 1.0)[:, None]
    rel = kappa / (zc ** 2).mean(axis=1)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert np.all(np.isfinite(hvec)) and np.all(np.isfinite(rel))
    print(json.dumps(dict(workload=name, D=D, T=T, r=r, p=p, n=int(n), L=L, host_ms=round(host_ms, 3),
                          host_ns_per_draw=round(1e6 * host_ms / D, 1))), flush=True)


H = 40
B, T, N, r = 1024, 500, 200, 8
panel, P = ctx.synth_panels(7, 0, B, T, N, r)
proxy_line("proxy_r8_replicates", panel, P, H, 15, 1)
proxy_line("proxy_r8_point", panel[:1].contiguous(), [x[:1].contiguous() for x in P], H, 16383, 1)
yardstick_line("host_numpy_r8", panel, P, 16383, 1)
del panel, P

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
ep = m.em_params
x = np.nan_to_num(api._forecast_inputs(m, 224)[1])                  # 222 rows; balanced, as the synthetic shape is
rep = lambda a, n: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape))).to(dev)
par = lambda n: [rep(ep[k], n) for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")]
proxy_line("proxy_sw_var4_replicates", rep(x, B), par(B), H, 15, 4)
proxy_line("proxy_sw_var4_point", rep(x, 1), par(1), H, 16383, 4)
yardstick_line("host_numpy_sw_var4", rep(x, 1), par(1), 16383, 4)
ctx.close()
