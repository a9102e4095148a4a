#!/usr/bin/env python
"""Measurement lines of dfm_signirf_batch_dev (csrc/signirf.hip; run on the GPU box).  Shapes: B = 1024 replicates x M = 1024
candidates, K = 1 (one accepted rotation per posterior draw) and B = 1, M = 2^20, K = 1024 (the point estimate's accepted set), each at
(N 200, r 8, p 1, H 40) on dfm_synth_panels_dev parameters and at the Stock-Watson shape (N 139, r 4, p 4, H 40) on the fitted
parameters.  Restrictions: two series positive on shock 0 over h 0-2, one positive and one negative on shock 1.
Each line: ms per call (median of timed calls after warm-up, HIP events), the per-kernel ms of one profiled call
(dfm_profile_read), the call's microseconds per candidate, and for the kept-slot fill the written bytes over dfm_hbm_probe's write
rate as the bound.  The yardstick is what the parent commit offers: rotate every candidate's parameters on the host (NumPy) and call
dfm_irf_batch_dev on all of them, with the number of candidates cut so that its IRF output stays under 2 GB; its microseconds per
candidate are reported for the device call alone and with the host rotation.  Prints one JSON line per workload."""
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
RESTR = [(0, 0, 0, 2, 1), (1, 0, 0, 2, 1), (2, 1, 0, 2, 1), (3, 1, 0, 2, -1)]


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


def sign_line(name, Lam, A, Q, R, H, M, K):
    B, N, r = Lam.shape
    fn = lambda: ctx.signirf_batch(Lam, A, Q, R, H, RESTR, M, K, seed=1, want_fevd=True)
    ms, prof = timed(fn), profiled(fn)
    share = float(fn()["n_accept"].double().mean().item()) / M
    bound = B * K * (2 * r + 1) * H * N * 8 / (write_gbs * 1e6)
    fill = prof["sv_irf_fill_kernel"]                               # (a missing kernel is an error, not a NaN in the table)
    print(json.dumps(dict(workload=name, B=B, M=M, K=K, N=N, r=r, H=H, call_ms=round(ms, 4), us_per_candidate=round(1e3 * ms / (B * M), 5),
                          accepted_share=round(share, 4), kernels_ms=prof, write_gbs=round(write_gbs, 1),
                          fill_bound_ms=round(bound, 4), fill_over_bound=round(fill / bound, 3))), flush=True)


def yardstick_line(name, Lam, A, Q, R, H):
    """One replicate's parameters (NumPy), C candidates: Haar rotations by numpy.linalg.qr, the rotated sets (Lam S_m, S_m^-1 A S_m, I)
    on the host, then dfm_irf_batch_dev over the C sets."""
    N, r = Lam.shape
    p = A.shape[1] // r
    C = int(min(4096, (2 << 30) // (r * H * N * 8)))
    g = np.random.default_rng(1)
    t0 = time.perf_counter()
    S = np.linalg.cholesky(Q)
    Qm, U = np.linalg.qr(g.standard_normal((C, r, r)))
    Sm = S @ (Qm * np.sign(np.diagonal(U, axis1=1, axis2=2))[:, None, :])
    Si = np.linalg.inv(Sm)
    Lr = Lam @ Sm
    Ar = np.concatenate([Si @ A[:, j * r:(j + 1) * r] @ Sm for j in range(p)], axis=2)
    Qr = np.broadcast_to(np.eye(r), (C, r, r))
    host_ms = 1e3 * (time.perf_counter() - t0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ld, Ad, Qd, Rd = t(Lr), t(Ar), t(Qr), t(np.broadcast_to(R, (C, N)))
    ms = timed(lambda: ctx.irf_batch(Ld, Ad, Qd, Rd, H))
    print(json.dumps(dict(workload=name, candidates=C, N=N, r=r, H=H, irf_call_ms=round(ms, 4), host_rotation_ms=round(host_ms, 2),
                          us_per_candidate_device=round(1e3 * ms / C, 5), us_per_candidate_with_host=round(1e3 * (ms + host_ms) / C, 5))),
          flush=True)


H = 40
B, N, r = 1024, 200, 8
_, (Lam, R, A, Q, mu0, P0) = ctx.synth_panels(7, 0, B, 8, N, r)
sign_line("sign_r8_draws", Lam, A, Q, R, H, 1024, 1)
sign_line("sign_r8_point", Lam[:1].contiguous(), A[:1].contiguous(), Q[:1].contiguous(), R[:1].contiguous(), H, 1 << 20, 1024)
yardstick_line("host_rotate_irf_r8", *(x[0].cpu().numpy() for x in (Lam, A, Q, R)), H)
del Lam, R, A, Q, mu0, P0

d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 216, 0, 4, 1e-8, 4, 4)
api.estimate(m, api.Parametric(), max_em_iter=10, tol_em=0.0, factor_lags=4, ctx=ctx)
ep = m.em_params
rep = lambda a, n: torch.from_numpy(np.array(np.broadcast_to(a, (n,) + a.shape))).to(dev)
sign_line("sign_sw_var4_draws", rep(ep["Lam"], B), rep(ep["Avar"], B), rep(ep["Q"], B), rep(ep["R"], B), H, 1024, 1)
sign_line("sign_sw_var4_point", rep(ep["Lam"], 1), rep(ep["Avar"], 1), rep(ep["Q"], 1), rep(ep["R"], 1), H, 1 << 20, 1024)
yardstick_line("host_rotate_irf_sw_var4", ep["Lam"], ep["Avar"], ep["Q"], ep["R"], H)
ctx.close()
