#!/usr/bin/env python
"""The smoother pass and two EM iterations under TWO builds of libdfmhip in ONE process, from identical device inputs, under every
switch set that tests/test_gpu_ks_pass.py uses to reach a kernel choice or a schedule of the balanced pass (csrc/capi.hip fast_route,
the pass_* schedules, general_route): one context per library and switch set, created while the set is in the environment.  For a host
refactor of the enqueue path: every output must equal the parent's bit for bit, and so must the kernel names and launch counts the
library's own profile (profile_enable / profile_read) reports.  What no profile shows -- the stream of a launch, the event edges -- is
checked by reading.
Shapes: the five of test_balanced_kernel_choices_agree, the two of test_wide_sub_batches_agree, one r = 3 shape (with missing cells:
the narrow chunk table) and one VAR(3) shape with r = 2 (the companion table).  Per shape: the pass balanced and with 10 % of the
cells missing, then two EM iterations (tol = 0) of each.  Switches of the diagnostics build run on the two diagnostics libraries.
DFM_WIDE_SUB runs in a process of its own with the variable set for all of it: the parent read it at the first pass of the process.
Usage: python scripts/dbg/pass_route_ab.py parent=<the other libdfmhip.so> [parent_diag=<the other libdfmhip_diag.so>] [out=<file>]
       exit status 1 on any difference"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ARGS = dict(a.split("=", 1) for a in sys.argv[1:])
if "out" in ARGS and ARGS.get("mode") != "one": open(ARGS["out"], "w").close()
OUT = open(ARGS["out"], "a") if "out" in ARGS else None            # (appending: the process of DFM_WIDE_SUB writes to it as well)

PROD = [{}, dict(DFM_PASS_FUSED=0), dict(DFM_FORCE_GENERAL=1)]
DIAG = [{}, dict(DFM_COLLAPSE_VARIANT=199), dict(DFM_COLLAPSE_VARIANT=198), dict(DFM_NO_FUSE_COV=1), dict(DFM_COLLAPSE_WPR=1),
        dict(DFM_COLLAPSE_WPR=3), dict(DFM_COLLAPSE_WPR=7), dict(DFM_NO_SIDE=1), dict(DFM_SUBBATCH=2), dict(DFM_SUBBATCH=3),
        dict(DFM_NO_PFILL=1), dict(DFM_FUSED_GRAM=0), dict(DFM_FUSED_GRAM=0, DFM_PASS_FUSED=0), dict(DFM_FUSE_GRAM=1),
        dict(DFM_WIDE_OLD=1), dict(DFM_NO_SIDE=1, DFM_PASS_FUSED=0), dict(DFM_WIDE_SUB=2)]
SHAPES = [(5, 200, 500, 8), (3, 64, 48, 12), (4, 30, 41, 3), (3, 50, 7, 2), (2, 130, 37, 5), (64, 40, 20, 12), (65, 34, 130, 20),
          (6, 30, 222, 3)]
VARP = (4, 30, 60, 2, 3)                                   # B, N, T, r, p


def say(s=""):
    print(s, flush=True)
    if OUT: OUT.write(s + "\n"); OUT.flush()


def path(p):
    return p if os.path.isabs(p) else os.path.join(ROOT, p)


def run_set(env, diag):
    """Both libraries of one flavour under one switch set; returns the number of comparisons that differ."""
    import torch
    from dynamic_factor_models_amd import DfmContext
    from dynamic_factor_models_amd import _lib as _L
    new_so = os.path.join(os.path.dirname(_L.__file__), "lib", "libdfmhip_diag.so" if diag else "libdfmhip.so")
    old_so = path(ARGS["parent_diag" if diag else "parent"])

    def context(so, profile=True):
        _L.SO_PATH = so; _L._lib = None
        c = DfmContext(0)
        if profile: c.profile_enable(True)
        return c
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        libs = (context(old_so), context(new_so))
        gen = context(new_so, profile=False)                            # the inputs: a context of its own, outside both profiles
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    bits = lambda t: t.contiguous().view(torch.uint8)                  # (NaN-filled paths compare too)
    flat = lambda o: [x for x in (o.values() if isinstance(o, dict) else o) if x is not None]
    bad = 0

    def both(tag, call):
        nonlocal bad
        outs = [flat(call(c)) for c in libs]
        torch.cuda.synchronize()
        same = len(outs[0]) == len(outs[1]) and all(a.shape == b.shape and torch.equal(bits(a), bits(b)) for a, b in zip(*outs))
        prof = [{k: n for k, (_, n) in c.profile_read().items()} for c in libs]
        ok = same and prof[0] == prof[1]
        bad += not ok
        diff = {k: (prof[0].get(k, 0), prof[1].get(k, 0)) for k in sorted(set(prof[0]) | set(prof[1])) if prof[0].get(k) != prof[1].get(k)}
        say(f"  {tag:<46}{len(outs[1])} outputs {'bit for bit' if same else 'DIFFER'}; {len(prof[1])} kernel names and their launch counts "
            f"so far {'equal' if not diff else 'DIFFER (parent, new): ' + str(diff)}")

    def em(fn, c, panel, par, **kw):
        par = [p.clone() for p in par]                                  # (updated in place)
        return list(getattr(c, fn)(panel, *par, max_iter=2, tol=0.0, **kw)) + par
    say(f"{'diagnostics' if diag else 'production'} libraries, {env or 'no switch'}")
    for (B, N, T, r) in SHAPES:
        for miss in (0.0, 0.1):
            panel, par = gen.synth_panels(20160415, 0, B, T, N, r, missing_prob=miss)
            kw = dict(may_have_missing=miss > 0)
            both(f"B={B} N={N} T={T} r={r} missing={miss}: pass", lambda c: c.ks_pass_batch(panel, *par, **kw))
            both(f"B={B} N={N} T={T} r={r} missing={miss}: EM x 2", lambda c: em("em_batch", c, panel, par, **kw))
    B, N, T, r, p = VARP
    panel, (Lam, R, A, Q, mu0, P0) = gen.synth_panels(20160415, 0, B, T, N, r, missing_prob=0.1)
    par = (Lam, R, torch.cat([0.5 * A, 0.2 * A, 0.1 * A], dim=2).contiguous(), Q, torch.zeros((B, r * p), dtype=A.dtype, device=A.device),
           torch.eye(r * p, dtype=A.dtype, device=A.device).expand(B, r * p, r * p).contiguous())
    both(f"VAR({p}) B={B} N={N} T={T} r={r} missing=0.1: pass", lambda c: c.ks_pass_varp_batch(panel, *par, may_have_missing=True))
    both(f"VAR({p}) B={B} N={N} T={T} r={r} missing=0.1: EM x 2", lambda c: em("em_varp_batch", c, panel, par, may_have_missing=True))
    for c in libs + (gen,): c.close()
    return bad


def main():
    if ARGS.get("mode") == "one":                          # (a child of the run below: one set, already in the environment)
        env = dict(kv.split(":") for kv in ARGS["set"].split(",")) if ARGS.get("set") else {}
        return 1 if run_set(env, ARGS["flavour"] == "diag") else 0
    say("the enqueue path of the pass: this tree's libraries against the parent's, outputs bit for bit, kernel names and launch counts")
    bad = 0
    for diag, sets in ((False, PROD), (True, DIAG if "parent_diag" in ARGS else [])):
        for env in sets:
            if "DFM_WIDE_SUB" not in env:
                bad += run_set(env, diag)
                continue
            if OUT: OUT.flush()
            cmd = [sys.executable, os.path.abspath(__file__), "mode=one", "flavour=" + ("diag" if diag else "prod"),
                   "set=" + ",".join(f"{k}:{v}" for k, v in env.items())] + [f"{k}={ARGS[k]}" for k in ("parent", "parent_diag", "out") if k in ARGS]
            rc = subprocess.run(cmd, env=dict(os.environ, **{k: str(v) for k, v in env.items()})).returncode
            if rc not in (0, 1): say(f"  the process of {env} ended with status {rc}"); return rc
            bad += rc
    if "parent_diag" not in ARGS: say("no parent_diag=: the switches of the diagnostics build were not run")
    say(f"{bad} comparison(s) differ" if bad else "every output, kernel name and launch count equals the parent's")
    return 1 if bad else 0


sys.exit(main())
