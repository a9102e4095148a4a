#!/usr/bin/env python
"""Measurement lines of dfm_news_ar_batch_dev (csrc/news_ar.hip; run on the GPU box).  Workloads (edge-shaped synthetic vintages,
B = 1024 copies of one stable parameter set; the values of the cells do not move a time):
  na_sw   -- T = 222, N = 139, r = 4, p = 4, q = 4, G = 4; the new vintage adds two ragged rows (half, then a quarter of the series)
  na_long -- T = 500, N = 200, r = 4, p = 1, q = 1, G = 2; the new vintage adds the last row, half observed
Each workload is run without and with `weight` (news is always written).  Each line: ms per call (median of 20 timed calls after
warm-up, HIP events), the per-kernel ms of one profiled call (dfm_profile_read), one dfm_forecast_ar_batch_dev on the new panel at
the call's horizon (the call runs three), the recursion kernel, the covariance-panel kernel beside its written bytes over
dfm_hbm_probe's write rate, the weight passes (every other kernel of the call minus three forecasts), and the impact kernel beside
its bound: the covariance panels and the smoothed state read once per pass replicate, the new, old and revised-old xhat panels once
per replicate (its G targets run next to each other), the weights, news and impacts written once.  Two yardsticks on the same
panels: dfm_news_batch_dev at the same p (no AR terms) and the one forecast.  Prints one JSON line per workload."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_factor_models_amd import DfmContext  # noqa: E402

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


def model(N, r, p, q, seed):
    """One stable parameter set: diagonal VAR with halving lags, P0 its stationary covariance on m = max(p, q + 1) lags."""
    g = np.random.default_rng(seed)
    m = max(p, q + 1)
    k = r * m
    wl = 0.5 ** np.arange(p)
    Avar = np.hstack([np.diag(g.uniform(0.5, 0.85, r)) * wl[l] / wl.sum() for l in range(p)])   # the lags of a factor sum to < 0.85
    Q = 0.5 * np.eye(r)
    M = np.zeros((k, k)); M[:r, :r * p] = Avar; M[r:, :k - r] = np.eye(k - r)
    Qk = np.zeros((k, k)); Qk[:r, :r] = Q
    assert np.abs(np.linalg.eigvals(M)).max() < 0.95
    P0 = np.linalg.solve(np.eye(k * k) - np.kron(M, M), Qk.ravel()).reshape(k, k)
    rho = np.zeros((N, q)); rho[:, 0] = g.uniform(-0.3, 0.6, N)
    for l in range(1, q):
        rho[:, l] = g.uniform(-0.15, 0.15, N) / l
    return dict(Lam=g.standard_normal((N, r)), sig2=g.uniform(0.5, 1.5, N), rho=rho, Avar=Avar, Q=Q, mu0=np.zeros(k),
                P0=0.5 * (P0 + P0.T) + 1e-10 * np.eye(k))


def line(name, B, T, N, r, p, q, targets, edge_rows):
    st = model(N, r, p, q, 7)
    g = np.random.default_rng(11)
    new = g.standard_normal((T, N))
    for j in range(edge_rows):                                   # the last row is half observed (a quarter with two ragged rows,
        new[T - 1 - j, (N // 2 if edge_rows == 1 else (N // 4) * (j + 1)):] = np.nan   # the row before it half): edges, no gaps
    old = new.copy()
    old[T - edge_rows:] = np.nan
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a[None], (B,) + a.shape))).to(dev)
    xo, xn = t(old), t(new)
    par = [t(st[k]) for k in ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")]
    kp = r * p
    plain = [par[0], par[1], par[3], par[4], t(st["mu0"][:kp]), t(st["P0"][:kp, :kp])]
    G = len(targets)
    H = max(0, max(tt for tt, _ in targets) + 1 - T)
    ns, Rp = T - q, 1 << max(1, int(np.ceil(np.log2(r * max(p, q + 1)))))
    fc = lambda: ctx.forecast_ar_batch_dev(xn, *par, H, want=(), may_have_missing=True)
    fc_ms, fc_kern = timed(fc), profiled(fc)
    for want_weight in (False, True):
        call = lambda: ctx.news_ar_batch_dev(xo, xn, *par, targets, want_weight=want_weight, may_have_missing=True)
        ms = timed(call)
        kern = profiled(call)
        pick = lambda stem: sum(v for k, v in kern.items() if k.startswith(stem))
        rec, qc, imp = pick("news_ar_rec_kernel"), pick("news_ar_qc_kernel"), pick("news_ar_impact_kernel")
        ours = pick("news_") + pick("simsmooth_")
        passes = sum(kern.values()) - ours - 3 * sum(fc_kern.values())
        qc_wr = B * G * ns * N * 8
        imp_rd = (B * G * ns * (N + Rp) + 3 * B * ns * N) * 8
        imp_wr = ((B * G * ns * N if want_weight else 0) + B * ns * N + B * G * N) * 8
        qc_bound = qc_wr / (write_gbs * 1e6)
        imp_bound = imp_rd / (read_gbs * 1e6) + imp_wr / (write_gbs * 1e6)
        old_news = lambda: ctx.news_batch(xo, xn, *plain, targets, want_weight=want_weight, may_have_missing=True)
        print(json.dumps(dict(workload=name, weight=want_weight, B=B, T=T, N=N, r=r, p=p, q=q, G=G, H=H, ms_per_call=round(ms, 4),
                              kernels_ms=kern, one_forecast_ar_ms=round(fc_ms, 4), one_forecast_ar_kernels_ms=round(sum(fc_kern.values()), 4),
                              rec_ms=round(rec, 4), qc_ms=round(qc, 4), qc_bytes_written=qc_wr, qc_bound_ms=round(qc_bound, 4),
                              qc_over_bound=round(qc / qc_bound, 3), weight_passes_ms=round(passes, 4), impact_ms=round(imp, 4),
                              impact_bytes_read=imp_rd, impact_bytes_written=imp_wr, impact_bound_ms=round(imp_bound, 4),
                              impact_over_bound=round(imp / imp_bound, 3), hbm_read_gbs=round(read_gbs, 1),
                              hbm_write_gbs=round(write_gbs, 1), news_batch_same_p_ms=round(timed(old_news), 4))), flush=True)
        torch.cuda.empty_cache()


line("na_sw", 1024, 222, 139, 4, 4, 4, [(221, 0), (221, 100), (223, 0), (223, 100)], 2)
torch.cuda.empty_cache()
line("na_long", 1024, 500, 200, 4, 1, 1, [(499, 0), (501, 3)], 1)
ctx.close()
