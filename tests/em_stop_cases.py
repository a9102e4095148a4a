"""Cases of tests/test_gpu_em_stop.py: one EM run with tol > 0 per kernel that hosts the stop rule (csrc/dfm_em_epilogue.h), reached by
shape.  Each case names its family (plain factor model, VAR(p) factors, AR(q) idiosyncratic terms), its shape, and the tol / max_iter
chosen on the CPU from the family's oracle under the two preconditions `expected()` asserts.  No GPU code here."""
import numpy as np

from oracle import ar_oracle as ao
from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo

PLAIN_KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
VARP_KEYS = ("Lam", "R", "Avar", "Q", "mu0", "P0")
AR_KEYS = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")

# route (confirmed from launch_recursion / launch_em_update / recursion_*_supported, csrc): see the comment of every case
CASES = {
    # balanced, Rp = 2: fast-path E-step; the transition step is em_update_wave<2> -- deferred into the loadings step's streaming launch
    # (mstep_mfma.hip) or em_update_kernel<2>'s own launch, the same device function either way
    "em_update_wave": dict(kind="plain", B=6, N=30, T=60, r=2, missing=0.0, tol=9e-05, max_iter=10),
    # balanced, r = 12 -> Rp = 16: em_update_grid_supported -> em_update_grid_kernel<16>
    "em_update_grid": dict(kind="plain", B=3, N=64, T=48, r=12, missing=0.0, tol=0.0005, max_iter=12),
    # missing cells, r = 4 widened to Rp = 8 (B <= 1536), information form, T >= 2 (L + W): recursion_chunk_supported
    "recursion_chunk": dict(kind="plain", B=5, N=40, T=80, r=4, missing=0.15, tol=0.0002, max_iter=10),
    # Rp = 8, 12 series on 8 factors: the chunk boundaries do not agree (tests/test_gpu_chunk.py, slowly forgetting filter), the
    # replicates go to launch_recursion_wave8_fallback -> recursion_pair_kernel (B <= pair_bmax)
    "recursion_pair": dict(kind="plain", B=3, N=12, T=64, r=8, missing=0.1, tol=0.0015, max_iter=12),
    # missing cells, r = 12 -> Rp = 16, information form: recursion_wave_supported -> recursion_wave_kernel<16, false>
    "recursion_wave16": dict(kind="plain", B=2, N=60, T=50, r=12, missing=0.1, tol=0.001, max_iter=12),
    # missing cells, r = 20 -> Rp = 32, rstate in 17..31: recursion_tile_supported; B = 2 gives chunks -> tile_chunk_finish + tile_mstep
    "recursion_tile": dict(kind="plain", B=2, N=300, T=60, r=20, missing=0.1, tol=0.0003, max_iter=10),
    # r = 2, B > 1536: not widened to Rp = 8 (widens_small_r, capi.hip) -> the lane-group recursion_kernel<2, false>
    "recursion_rows": dict(kind="plain", B=1537, N=12, T=20, r=2, missing=0.1, tol=0.0005, max_iter=16,
                           idx=(0, 1, 31, 32, 767, 1024, 1535, 1536)),
    # VAR(4), r = 3: state 12 -> Rp = 16, Rc = 4, rl = 3: recursion_mbf16_supported -> recursion_mbf16_kernel + cov_epilogue_kernel<16>
    "recursion_mbf16": dict(kind="varp", B=3, N=40, T=60, r=3, p=4, missing=0.1, tol=0.00025, max_iter=10),
    # VAR(4), r = 4: kdim = 16, Rc = rl = 4: recursion_comp_supported (var) -> recursion_comp_kernel + cov_epilogue_kernel<16>
    "recursion_comp_var": dict(kind="varp", B=3, N=40, T=60, r=4, p=4, missing=0.1, tol=0.0003, max_iter=10),
    # AR(1) idiosyncratic terms, r = 2, p = 1: the smallest shape of tests/test_gpu_ar_em.py; state 4 -> Rp = 8, covariance form with
    # kb = 2: no chunk (cov), no comp (Rp = 8) -> recursion_wave_kernel<8, true> with the companion constraints
    "ar_wave8_cov": dict(kind="ar", B=3, N=12, T=60, r=2, p=1, q=1, missing=0.0, tol=0.0004, max_iter=10),
    # AR(4) idiosyncratic terms, r = 4, p = 4: state 20 -> Rp = 32, kb = 4, Rc = rl = 0: the smallest shape of tests/test_gpu_ar_em.py
    # that recursion_comp_supported (ar) accepts -> recursion_comp_kernel + cov_epilogue_kernel<32>
    "recursion_comp_ar": dict(kind="ar", B=2, N=20, T=90, r=4, p=4, q=4, missing=0.0, tol=0.0005, max_iter=14),
}


def keys(case):
    return {"plain": PLAIN_KEYS, "varp": VARP_KEYS, "ar": AR_KEYS}[case["kind"]]


_inputs = {}


def inputs(name):
    """(panel [B, T, N], start parameters {key: [B, ...]}) of a case; computed once, never modified."""
    if name in _inputs:
        return _inputs[name]
    c = CASES[name]
    xs, sts = [], []
    for b in range(c["B"]):
        if c["kind"] == "plain":
            x, _ = ko.synth_replicate(b, c["N"], c["T"], c["r"], missing=c["missing"])
            st, _ = ko.pca_init(np.nan_to_num(x), c["r"])      # (NaN -> 0 = column mean, as DGR do)
        elif c["kind"] == "varp":
            x = vo.synth_varp(b, c["N"], c["T"], c["r"], c["p"], missing=c["missing"])
            st, _ = vo.varp_init(np.nan_to_num(x), c["r"], c["p"])
        else:
            x, st = ao.synth_ar(b, c["N"], c["T"], c["r"], c["p"], c["q"], missing=c["missing"])
        xs.append(x); sts.append(st)
    panel = np.stack(xs)
    start = {k: np.stack([s[k] for s in sts]) for k in keys(c)}
    for a in (panel, *start.values()):
        a.setflags(write=False)
    _inputs[name] = (panel, start)
    return _inputs[name]


def compared(name):
    """Replicates compared with the oracle (all of them unless the case lists some)."""
    c = CASES[name]
    return tuple(c.get("idx", range(c["B"])))


def _step(c, x, par):
    if c["kind"] == "plain":
        return ko.em_step(x, **par)[:2]
    if c["kind"] == "varp":
        return vo.em_step_varp(x, p=c["p"], **par)[:2]
    return ao.em_step_ar(x, **par)[:2]


_oracle = {}


def oracle(name):
    """The family's oracle, once, with tol = 0 for max_iter iterations: {b: (path [max_iter], snaps)} with snaps[m] the parameters
    after m M-steps (snaps[0] = the start)."""
    if name in _oracle:
        return _oracle[name]
    c = CASES[name]
    panel, start = inputs(name)
    res = {}
    for b in compared(name):
        par = {k: np.array(start[k][b], float) for k in keys(c)}
        path, snaps = [], [par]
        for _ in range(c["max_iter"]):
            par, ll = _step(c, panel[b], par)
            path.append(ll); snaps.append(par)
        res[b] = (np.array(path), snaps)
    _oracle[name] = res
    return res


def rel_improvement(path):
    """(ll_k - ll_{k-1}) / (0.5 (|ll_k| + |ll_{k-1}|)), k = 1 ..: oracle/kalman_oracle.py em(), lines 254-256."""
    return (path[1:] - path[:-1]) / (0.5 * (np.abs(path[1:]) + np.abs(path[:-1])))


def expected(name):
    """{b: (iters, M-steps applied)} from the oracle's tol = 0 path: k* = first k >= 1 with relative improvement < tol, iters = k* + 1
    (k* M-steps applied), or max_iter (all applied).  Asserts the preconditions of the case on the oracle's path."""
    c = CASES[name]
    tol, mi = c["tol"], c["max_iter"]
    out = {}
    for b, (path, _) in oracle(name).items():
        ri = rel_improvement(path)
        assert np.all(np.abs(ri - tol) > 1e-3 * tol), (name, b, "a relative improvement lies within 1e-3 tol of tol")
        below = np.nonzero(ri < tol)[0]
        out[b] = (int(below[0]) + 2, int(below[0]) + 1) if below.size else (mi, mi)
    its = [v[0] for v in out.values()]
    assert min(its) < mi, (name, "no replicate stops before max_iter")
    assert max(its) > 2, (name, "no replicate goes on after iteration 2")
    return out


def run(ctx, name, tol):
    """The case on the library behind ctx (host-pointer entries).  Returns {params..., path, iters, f_smooth, P_smooth} as NumPy arrays."""
    c = CASES[name]
    panel, start = inputs(name)
    args = [start[k] for k in keys(c)]
    if c["kind"] == "plain":
        new, path, its, f, P = ctx.em_batch_host(panel, *args, max_iter=c["max_iter"], tol=tol)
    elif c["kind"] == "varp":
        new, path, its, f, P = ctx.em_varp_batch_host(panel, *args, max_iter=c["max_iter"], tol=tol)
    else:
        new, path, its, f, P = ctx.em_ar_batch_host(panel, *args, max_iter=c["max_iter"], tol=tol)
    out = {k: np.asarray(new[k]) for k in keys(c)}
    out.update(path=np.asarray(path), iters=np.asarray(its), f_smooth=np.asarray(f), P_smooth=np.asarray(P))
    return out
