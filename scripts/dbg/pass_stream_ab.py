#!/usr/bin/env python
"""The balanced smoother pass under TWO builds of libdfmhip in ONE process, from identical device inputs, at the shapes of
tests/test_gpu_pass_fused_stream.py (B = 7 on two workgroups, B = 1 and 3 on the default grid) and at two batches of the headline
shape -- B = 1024 (non-temporal panel stream) and B = 2720 (panels above 2 GiB: the plain DMA).  Every output must equal the
parent's bit for bit.  Both libraries live in this process, one context each (as scripts/dbg/driver_ab.py).
Usage: python scripts/dbg/pass_stream_ab.py parent=<path of the other libdfmhip.so> [out=<file>]      exit status 1 on a difference"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from dynamic_factor_models_amd import DfmContext
from dynamic_factor_models_amd import _lib as _L

ARGS = dict(a.split("=", 1) for a in sys.argv[1:])
NEW_SO = _L.SO_PATH
PARENT_SO = ARGS["parent"] if os.path.isabs(ARGS["parent"]) else os.path.join(ROOT, ARGS["parent"])
OUT = open(ARGS["out"], "w") if "out" in ARGS else None


def say(s=""):
    print(s, flush=True)
    if OUT: OUT.write(s + "\n"); OUT.flush()


def context(so, num_cu=None):
    _L.SO_PATH = so; _L._lib = None
    if num_cu: os.environ["DFM_NUM_CU"] = str(num_cu)
    try:
        return DfmContext(0)
    finally:
        os.environ.pop("DFM_NUM_CU", None)


pairs = {cu: (context(PARENT_SO, cu), context(NEW_SO, cu)) for cu in (None, 2)}
cases = [(7, N, T, 2) for N in (128, 136, 200, 258, 512, 10) for T in (9, 33, 37, 228)]
cases += [(B, N, T, None) for B in (1, 3) for N in (128, 136, 200, 258, 512, 10) for T in (9, 33, 37, 228)]
cases += [(1024, 200, 500, None), (2720, 200, 500, None)]
bad = 0
for B, N, T, cu in cases:
    parent, new = pairs[cu]
    panel, par = parent.synth_panels(20160415, 0, B, T, N, 8)
    if B > 1:                                   # replicates 2, 3, 6, 7, ... scaled: consecutive replicates of a workgroup differ
        odd = (torch.arange(B, device=panel.device) // 2) % 2 == 1          # grossly on two workgroups (b, b + 2), as in the test file
        par[0][odd] *= 3.0; par[1][odd] *= 0.5
    a = parent.ks_pass_batch(panel, *par, may_have_missing=False)
    b = new.ks_pass_batch(panel, *par, may_have_missing=False)
    torch.cuda.synchronize()
    same = [torch.equal(x, y) for x, y in zip(a, b)]
    finite = all(bool(torch.isfinite(x).all()) for x in b)
    bad += not (all(same) and finite)
    say(f"B={B:<5} N={N:<4} T={T:<4} workgroups={cu or 'all':<4} f_smooth, P_smooth, loglik: "
        f"{'bit for bit' if all(same) else 'DIFFER ' + str(same)}{'' if finite else '  NOT FINITE'}")
    del panel, par, a, b
say(f"{bad} case(s) differ" if bad else "every output equals the parent's bit for bit")
sys.exit(1 if bad else 0)
