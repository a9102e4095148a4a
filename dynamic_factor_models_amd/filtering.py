"""Binding of the filter entries of include/dfm_hip.h (csrc/filter.hip): dfm_filter_batch[_dev].  The functions take a DfmContext;
importing this module (kalman.py does) also attaches them to DfmContext as filter_batch_dev and filter_batch_host, with the
marshalling conventions of forecast_batch(_host): device tensors in and out on torch's current stream, or NumPy through the
host-pointer entry.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k

MOMENTS = ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t")
CELLS = ("xpred", "verr", "vstd")
EVAL = ("msfe", "msfe0", "cnt")
OUTPUTS = MOMENTS + CELLS + EVAL


def check_args(T: int, H: int, t0: int):
    """The argument rules of dfm_filter_batch that need no device."""
    if int(H) < 0:
        raise ValueError("H must be >= 0")
    if not (0 <= int(t0) < int(T)):
        raise ValueError(f"t0 (the first origin) must lie in 0..{int(T) - 1}")


def _filter(ctx, be, panel, params, H, t0, mean, sd, want, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._VARP, be, panel, params)
    B, T, N, r, p = dims
    H, t0 = int(H), int(t0)
    check_args(T, H, t0)
    want = OUTPUTS if want is None else tuple(want)
    unknown = [w for w in want if w not in OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose among {OUTPUTS}")
    mean, sd = _k._pair(be, mean, sd)
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    k = r * p
    kk = k * (k + 1) // 2
    shape = dict(z_pred=(B, T, k), P_pred=(B, T, kk), z_filt=(B, T, k), P_filt=(B, T, kk), loglik_t=(B, T), xpred=(B, T, N),
                 verr=(B, T, N), vstd=(B, T, N), msfe=(B, H, N), msfe0=(B, H, N), cnt=(B, H, N))
    out = {n: None for n in OUTPUTS}
    for n in want:
        if n in EVAL and H == 0:
            continue                                  # no evaluation: the entry leaves these untouched
        out[n] = be.out(*shape[n], int32=(n == "cnt"))
    be.sync()
    rc = getattr(ctx._lib, "dfm_filter_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, H, t0, be.ptr(panel, "panel"), *_k._ptrs(be, _k._VARP, params, shapes),
        be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), *[be.ptr(out[n], n) for n in OUTPUTS[:-1]],
        None if out["cnt"] is None else be.raw(out["cnt"]), flags)
    _k._check(ctx._h, rc)
    return out


def filter_batch_dev(ctx, panel, Lam, R, Avar, Q, mu0, P0, H: int = 0, t0: int = 0, mean=None, sd=None, want=None,
                     may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_filter_batch_dev (device tensors, torch's current stream): predicted and filtered states, per-period log-likelihoods,
    one-step prediction errors and the h-step out-of-sample record of B replicates, the parameters held fixed over all origins.
    Parameters as forecast_batch; `want` names the outputs to compute (default all of OUTPUTS; the evaluation's only for H >= 1).
    Returns a dict with every name of OUTPUTS, None where not computed.  A failed update is reported by synchronize()."""
    return _filter(ctx, _k._Torch(ctx, panel), panel, (Lam, R, Avar, Q, mu0, P0), H, t0, mean, sd, want, may_have_missing,
                   singular_q)


def filter_batch_host(ctx, panel, Lam, R, Avar, Q, mu0, P0, H: int = 0, t0: int = 0, mean=None, sd=None, want=None,
                      may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_filter_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as filter_batch_dev."""
    return _filter(ctx, _k._NP, panel, (Lam, R, Avar, Q, mu0, P0), H, t0, mean, sd, want, may_have_missing, singular_q)


for _f in (filter_batch_dev, filter_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
