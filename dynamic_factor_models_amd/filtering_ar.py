"""Binding of the filter entries of the model with AR idiosyncratic terms (include/dfm_hip.h, csrc/filter_ar.hip):
dfm_filter_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to
DfmContext as filter_ar_batch_dev and filter_ar_batch_host, on the marshalling of the `_ar` family (ks_pass_ar_batch) and with the
conventions of filter_batch(_host): device tensors in and out on torch's current stream, or NumPy through the host-pointer entry.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k

MOMENTS = ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t")
CELLS = ("xpred", "verr", "vstd")
EVAL = ("msfe", "msfe_common", "msfe0", "cnt")
OUTPUTS = MOMENTS + CELLS + EVAL


def check_args(T: int, q: int, H: int, t0: int):
    """The argument rules of dfm_filter_ar_batch that need no device."""
    if int(H) < 0:
        raise ValueError("H must be >= 0")
    if not (1 <= int(q) <= 4):
        raise ValueError("the filter needs 1 <= q <= 4 idiosyncratic lags (q = 0 is filter_batch)")
    if int(T) <= int(q):
        raise ValueError("T must exceed the number of idiosyncratic lags")
    if not (int(q) <= int(t0) < int(T)):
        raise ValueError(f"t0 (the first origin, a panel row) must lie in {int(q)}..{int(T) - 1}")


def _filter_ar(ctx, be, panel, params, H, t0, mean, sd, want, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._AR, be, panel, params)
    B, T, N, r, p, q = dims
    H = int(H)
    t0 = q if t0 is None else int(t0)
    check_args(T, q, H, t0)
    want = OUTPUTS if want is None else tuple(want)
    unknown = [w for w in want if w not in OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose among {OUTPUTS}")
    mean, sd = _k._pair(be, mean, sd)
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    k = r * max(p, q + 1)
    kk = k * (k + 1) // 2
    n = T - q
    shape = dict(z_pred=(B, n, k), P_pred=(B, n, kk), z_filt=(B, n, k), P_filt=(B, n, kk), loglik_t=(B, n), xpred=(B, n, N),
                 verr=(B, n, N), vstd=(B, n, N), msfe=(B, H, N), msfe_common=(B, H, N), msfe0=(B, H, N), cnt=(B, H, N))
    out = {name: None for name in OUTPUTS}
    for name in want:
        if name in EVAL and H == 0:
            continue                                  # no evaluation: the entry leaves these untouched
        out[name] = be.out(*shape[name], int32=(name == "cnt"))
    be.sync()
    rc = getattr(ctx._lib, "dfm_filter_ar_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, q, H, t0, be.ptr(panel, "panel"), *_k._ptrs(be, _k._AR, params, shapes),
        be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), *[be.ptr(out[name], name) for name in OUTPUTS[:-1]],
        None if out["cnt"] is None else be.raw(out["cnt"]), flags)
    _k._check(ctx._h, rc)
    return out


def filter_ar_batch_dev(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, H: int = 0, t0: Optional[int] = None, mean=None, sd=None,
                        want=None, may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_filter_ar_batch_dev (device tensors, torch's current stream): predicted and filtered states, per-period
    log-likelihoods, one-step prediction errors and the h-step out-of-sample record (with and without the idiosyncratic term) of B
    replicates of the model with AR(q) idiosyncratic terms, the parameters held fixed over all origins.  Parameters as
    ks_pass_ar_batch; the outputs have the T - q rows q .. T-1; t0 is a panel row (default q, the first); `want` names the outputs
    to compute (default all of OUTPUTS; the evaluation's only for H >= 1).  Returns a dict with every name of OUTPUTS, None where
    not computed.  A failed update is reported by synchronize()."""
    return _filter_ar(ctx, _k._Torch(ctx, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), H, t0, mean, sd, want,
                      may_have_missing, singular_q)


def filter_ar_batch_host(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, H: int = 0, t0: Optional[int] = None, mean=None, sd=None,
                         want=None, may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_filter_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as filter_ar_batch_dev."""
    return _filter_ar(ctx, _k._NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), H, t0, mean, sd, want, may_have_missing,
                      singular_q)


for _f in (filter_ar_batch_dev, filter_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
