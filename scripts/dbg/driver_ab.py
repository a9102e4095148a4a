#!/usr/bin/env python
"""The model drivers of csrc/capi.hip (em_run, varp_run, the AR, mixed-frequency and observed-factor drivers, forecast) under TWO
builds of libdfmhip in ONE process, from identical inputs: every entry that goes through a driver, at the small shapes of
tests/test_gpu_model_drivers.py.  Both libraries live in this process, one context each (as scripts/dbg/inproc_ab.py).
Usage: python scripts/dbg/driver_ab.py parent=<path of the other libdfmhip.so> [mode=ab|census|speed] [lib=parent|new] [first=new] [out=<file>]
  mode=ab (default): per output, the largest absolute difference parent-vs-parent (the same call twice) and new-vs-parent.  Where
      the parent reproduces itself bit for bit the new library must equal it bit for bit; elsewhere (EM sums through LDS atomics)
      new-vs-parent may be at most twice the parent's own run-to-run difference.  Exit status 1 when an output breaks that.
  mode=census lib=parent|new: the call list once on ONE library -- the run to put under `rocprofv3 --kernel-trace --stats --`.
  mode=speed: one EM iteration of the headline shape, the varp_em shape of scripts/bench_extra.py (N = 139, T = 222, r = 4, p = 4,
      10 % missing, B = 1024) and the same with q = 4 AR terms, two contexts per library created in mirrored order (parent, new, new, parent; first=new:
      the other way round), all four timed in turn for 8 rounds; per library the 16 figures are pooled."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dynamic_factor_models_amd import DfmContext
from dynamic_factor_models_amd import _lib as _L
from oracle import ar_oracle as ao, kalman_oracle as ko, obs_oracle as oo, varp_oracle as vo
from tests import mf_expect as me

ARGS = dict(a.split("=", 1) for a in sys.argv[1:])
MODE = ARGS.get("mode", "ab")
NEW_SO = _L.SO_PATH
PARENT_SO = ARGS["parent"] if os.path.isabs(ARGS.get("parent", "")) else os.path.join(ROOT, ARGS["parent"])
OUT = open(ARGS["out"], "w") if "out" in ARGS else None


def say(s=""):
    print(s, flush=True)
    if OUT: OUT.write(s + "\n"); OUT.flush()


def context(so):
    _L.SO_PATH = so; _L._lib = None
    return DfmContext(0)


B, T, IT, MISS = 2, 40, 3, 0.1
PLAIN = ("Lam", "R", "A", "Q", "mu0", "P0")
VARP = ("Lam", "R", "Avar", "Q", "mu0", "P0")
AR = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
dev = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
stack = lambda sts, keys: {k: np.stack([s[k] for s in sts]) for k in keys}


def plain_case(N, r, miss):
    xs = [ko.synth_replicate(b, N, T, r, missing=miss)[0] for b in range(B)]
    return np.stack(xs), stack([ko.pca_init(np.nan_to_num(x), r)[0] for x in xs], PLAIN)


def varp_case(N, r, p, miss=MISS):
    xs = [vo.synth_varp(b, N, T, r, p, missing=miss) for b in range(B)]
    return np.stack(xs), stack([vo.varp_init(np.nan_to_num(x), r, p)[0] for x in xs], VARP)


def obs_em(c, x, G, d, ru, ro):
    """dfm_em_obs_batch_dev (no wrapper of its own in kalman.py)"""
    N = x.shape[2]
    path = torch.empty((B, IT), dtype=torch.float64, device=dev); its = torch.empty((B,), dtype=torch.int32, device=dev)
    f = torch.empty((B, T, ru), dtype=torch.float64, device=dev); P = torch.empty((B, T, ru * (ru + 1) // 2), dtype=torch.float64, device=dev)
    c._sync_stream()
    rc = c._lib.dfm_em_obs_batch_dev(c._h, B, T, N, ru, ro, c._dev(x, "x"), c._dev(G, "G"), *[c._dev(d[k], k) for k in PLAIN], IT, 0.0,
                                     c._dev(path, "path"), its.data_ptr(), c._dev(f, "f"), c._dev(P, "P"), 1)
    assert rc == 0, c._lib.dfm_last_error(c._h)
    return path, its, f, P


def em_result(d, keys, res):
    path, its, f, P = res
    return dict({k: d[k] for k in keys if d[k].numel()}, path=path, f_smooth=f, P_smooth=P)


def call_list():
    """[(name, fn)], fn(ctx) -> {output name: device tensor}; every fn builds its device tensors afresh from the same host arrays."""
    L = []
    for N, r, miss, tag in [(24, 3, MISS, "padded"), (24, 8, MISS, "unpadded"), (25, 3, MISS, "odd N"), (24, 8, 0.0, "balanced")]:
        x, st = plain_case(N, r, miss)
        def em(c, x=x, st=st):
            d = {k: t(st[k]) for k in PLAIN}
            return em_result(d, PLAIN, c.em_batch(t(x), *[d[k] for k in PLAIN], max_iter=IT, tol=0.0))
        def ps(c, x=x, st=st):
            return dict(zip(("f_smooth", "P_smooth", "loglik"), c.ks_pass_batch(t(x), *[t(st[k]) for k in PLAIN])))
        if tag == "padded": L.append((f"plain pass N={N} r={r}", ps))
        L.append((f"plain EM {tag} N={N} r={r}", em))
    for N, r, p in [(24, 3, 2), (25, 2, 2)]:
        x, st = varp_case(N, r, p)
        def em(c, x=x, st=st):
            d = {k: t(st[k]) for k in VARP}
            return em_result(d, VARP, c.em_varp_batch(t(x), *[d[k] for k in VARP], max_iter=IT, tol=0.0))
        def ps(c, x=x, st=st):
            return dict(zip(("f_smooth", "P_smooth", "loglik"), c.ks_pass_varp_batch(t(x), *[t(st[k]) for k in VARP])))
        L += [(f"VAR({p}) pass N={N} r={r}", ps), (f"VAR({p}) EM N={N} r={r}", em)]
    xs, sts = zip(*[ao.synth_ar(b, 24, T, 3, 2, 1, missing=MISS) for b in range(B)])
    x, st = np.stack(xs), stack(sts, AR)
    def ar_em(c, x=x, st=st):
        d = {k: t(st[k]) for k in AR}
        return em_result(d, AR, c.em_ar_batch(t(x), *[d[k] for k in AR], max_iter=IT, tol=0.0))
    def ar_ps(c, x=x, st=st):
        return dict(zip(("f_smooth", "P_smooth", "loglik"), c.ks_pass_ar_batch(t(x), *[t(st[k]) for k in AR])))
    L += [("AR pass r=3 p=2 q=1", ar_ps), ("AR EM r=3 p=2 q=1", ar_em)]
    xs, Ws, sts = zip(*[me.synth_mf(b, 16, 8, T, 3, 2, "q_avg", missing=MISS) for b in range(B)])
    x, W, st = np.stack(xs), Ws[0], stack(sts, VARP)
    mf_args = lambda d: (d["Lam"], d["R"], t(W), d["Avar"], d["Q"], d["mu0"], d["P0"])
    def mf_em(c, x=x, st=st):
        d = {k: t(st[k]) for k in VARP}
        return em_result(d, VARP, c.em_mf_batch(t(x), *mf_args(d), max_iter=IT, tol=0.0))
    def mf_ps(c, x=x, st=st):
        return dict(zip(("f_smooth", "P_smooth", "loglik"), c.ks_pass_mf_batch(t(x), *mf_args({k: t(st[k]) for k in VARP}))))
    L += [("mixed-frequency pass r=3 p=2 L=3", mf_ps), ("mixed-frequency EM r=3 p=2 L=3", mf_em)]
    for ru, ro in [(3, 1), (8, 1)]:
        reps = [oo.synth_obs(100 + b, 24, T, ru, ro, missing=MISS) for b in range(B)]
        x, G, st = np.stack([a for a, _, _ in reps]), np.stack([g for _, g, _ in reps]), stack([p for _, _, p in reps], PLAIN)
        def ob(c, x=x, G=G, st=st, ru=ru, ro=ro):
            d = {k: t(st[k]) for k in PLAIN}
            return em_result(d, PLAIN, obs_em(c, t(x), t(G), d, ru, ro))
        L.append((f"observed factors EM r_u={ru} r_o={ro}", ob))
    for p in (1, 2):
        x, st = varp_case(24, 3, p)
        def fc(c, x=x, st=st):
            return {k: v for k, v in c.forecast_batch(t(x), *[t(st[k]) for k in VARP], H=4).items() if v is not None}
        L.append((f"forecast p={p} H=4", fc))
    return L


def run(c, fn):
    out = fn(c)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def diff(a, b):
    """(largest absolute difference, bit for bit equal)"""
    if not np.array_equal(np.isnan(a), np.isnan(b)): return float("inf"), False
    return (float(np.nanmax(np.abs(a - b))) if a.size else 0.0), a.tobytes() == b.tobytes()


def mode_ab():
    parent, new = context(PARENT_SO), context(NEW_SO)
    say(f"parent = {os.path.relpath(PARENT_SO, ROOT)}   new = {os.path.relpath(NEW_SO, ROOT)}   B={B} T={T} {IT} EM iterations, {MISS:.0%} missing")
    say(f"{'call':<40}{'output':<10}{'parent-parent':>15}{'new-parent':>15}  verdict")
    bad = 0
    for name, fn in call_list():
        p1, p2, n1 = run(parent, fn), run(parent, fn), run(new, fn)
        for k in p1:
            (dpp, same_pp), (dnp, same_np) = diff(p1[k], p2[k]), diff(n1[k], p1[k])
            ok = same_np if same_pp else dnp <= 2.0 * dpp
            verdict = ("bit for bit" if same_np else "within the parent's spread") if ok else "DIFFERS"
            bad += not ok
            say(f"{name:<40}{k:<10}{dpp:>15.3e}{dnp:>15.3e}  {verdict}")
    say(f"{bad} output(s) differ" if bad else "every output equals the parent's (bit for bit wherever the parent reproduces itself)")
    return 1 if bad else 0


def mode_census():
    c = context(PARENT_SO if ARGS.get("lib", "new") == "parent" else NEW_SO)
    for name, fn in call_list():
        run(c, fn)
        say(name)
    return 0


def mode_speed():
    # Two contexts per library, created parent, new, new, parent (first=new: new, parent, parent, new): a context's speed depends on
    # where its workspace landed (whichever library is created first reads up to 3 % slower at the headline shape), and the
    # mirrored order gives each library one early and one late placement.
    order = ("new", "parent", "parent", "new") if ARGS.get("first") == "new" else ("parent", "new", "new", "parent")
    ctxs = [(n, context(PARENT_SO if n == "parent" else NEW_SO)) for n in order]
    Bs = 1024
    panel, par = ctxs[0][1].synth_panels(20160415, 0, Bs, 500, 200, 8)
    tile = lambda a: torch.from_numpy(np.ascontiguousarray(np.tile(a, (Bs // 16,) + (1,) * (a.ndim - 1)))).to(dev)
    xs = [vo.synth_varp(b, 139, 222, 4, 4, missing=0.1) for b in range(16)]
    xv, v0 = tile(np.stack(xs)), {k: tile(v) for k, v in stack([vo.varp_init(np.nan_to_num(x), 4, 4)[0] for x in xs], VARP).items()}
    xa, sa = zip(*[ao.synth_ar(b, 139, 222, 4, 4, 4, missing=0.1) for b in range(16)])
    xa, a0 = tile(np.stack(xa)), {k: tile(v) for k, v in stack(sa, AR).items()}
    def headline(c, w):
        for s, p in zip(w, par): s.copy_(p)
        c.em_batch(panel, *w, max_iter=1, tol=0.0, want_smooth=False, may_have_missing=False)
    def varp_em(c, w):
        for k in VARP: w[k].copy_(v0[k])
        c.em_varp_batch(xv, *[w[k] for k in VARP], max_iter=1, tol=0.0, want_smooth=False, may_have_missing=True)
    def ar_em(c, w):
        for k in AR: w[k].copy_(a0[k])
        c.em_ar_batch(xa, *[w[k] for k in AR], max_iter=1, tol=0.0, want_smooth=False, may_have_missing=True)
    work = [("headline em B=1024 N=200 T=500 r=8", headline, [p.clone() for p in par], 50),
            ("varp_em B=1024 N=139 T=222 r=4 p=4 10% missing", varp_em, {k: v.clone() for k, v in v0.items()}, 20),
            ("ar_em the same with q=4", ar_em, {k: v.clone() for k, v in a0.items()}, 10)]
    bad = 0
    for name, fn, w, K in work:
        res = [[] for _ in ctxs]
        for n, c in ctxs:
            for _ in range(K): fn(c, w)
            torch.cuda.synchronize()
        for rnd in range(8):
            for i, (n, c) in enumerate(ctxs):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(K): fn(c, w)
                torch.cuda.synchronize()
                res[i].append((time.perf_counter() - t0) / K * 1e3)
        median = lambda v: sorted(v)[len(v) // 2]
        pool = {lib: sorted(x for (n, _), r in zip(ctxs, res) if n == lib for x in r) for lib in ("parent", "new")}
        inside = pool["parent"][0] <= median(pool["new"]) <= pool["parent"][-1]
        bad += median(pool["new"]) > pool["parent"][-1]
        say(name)
        for (n, _), r in zip(ctxs, res):
            say(f"  context {n:>6}: median {median(r):.4f} ms   all {[round(v, 4) for v in r]}")
        for lib in ("parent", "new"):
            say(f"  {lib:>6}, both contexts: median {median(pool[lib]):.4f} ms  min {pool[lib][0]:.4f}  max {pool[lib][-1]:.4f}")
        say(f"  new median {'inside' if inside else ('BELOW' if median(pool['new']) < pool['parent'][0] else 'ABOVE')} the parent's range")
    return 1 if bad else 0


sys.exit(dict(ab=mode_ab, census=mode_census, speed=mode_speed)[MODE]())
