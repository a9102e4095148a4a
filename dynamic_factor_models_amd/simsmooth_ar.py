"""Binding of the path-draw entries of the model with AR idiosyncratic terms (include/dfm_hip.h, csrc/simsmooth_ar.hip):
dfm_simsmooth_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to
DfmContext as simsmooth_ar_batch_dev and simsmooth_ar_batch_host, on the marshalling of the `_ar` family (ks_pass_ar_batch) and
with the conventions of simsmooth_batch(_host): device tensors in and out on torch's current stream, or NumPy through the
host-pointer entry.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k


def _simsmooth_ar(ctx, be, panel, params, D, H, v0, seed, first_draw, mean, sd, want_x, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._AR, be, panel, params)
    B, T, N, r, p, q = dims
    D, H = int(D), int(H)
    if D < 1:
        raise ValueError("D must be >= 1")
    from .forecasting_ar import check_args       # (kalman.py imports both modules: not at import time)
    check_args(T, q, H)
    mean, sd = _k._pair(be, mean, sd)
    v0 = None if v0 is None else be.inp(v0)
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    n = T + H - q
    f = be.out(B, D, n, r)
    x = be.out(B, D, n, N) if want_x else None
    be.sync()
    rc = getattr(ctx._lib, "dfm_simsmooth_ar_batch" + be.suffix)(
        ctx._h, B, D, T, N, r, p, q, H, be.ptr(panel, "panel"), *_k._ptrs(be, _k._AR, params, shapes),
        be.ptr(v0, "v0", (B, N)), be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(first_draw), be.ptr(f, "f_draw"), be.ptr(x, "x_draw"), flags)
    _k._check(ctx._h, rc)
    return dict(f=f, x=x)


def simsmooth_ar_batch_dev(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, D: int, H: int = 0, v0=None, seed: int = 0,
                           first_draw: int = 0, mean=None, sd=None, want_x: bool = True,
                           may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_simsmooth_ar_batch_dev (device tensors, torch's current stream): D joint posterior draws per replicate of the factor
    path and of the panel's missing and horizon cells from the model with AR(q) idiosyncratic terms, over the n = T + H - q rows
    q .. T + H - 1.  Parameters, v0 and mean / sd as forecast_ar_batch_dev; seed / first_draw as simsmooth_batch.  Returns
    dict(f [B,D,n,r], x [B,D,n,N] or None without want_x)."""
    return _simsmooth_ar(ctx, _k._Torch(ctx, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), D, H, v0, seed, first_draw, mean,
                         sd, want_x, may_have_missing, singular_q)


def simsmooth_ar_batch_host(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, D: int, H: int = 0, v0=None, seed: int = 0,
                            first_draw: int = 0, mean=None, sd=None, want_x: bool = True,
                            may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_simsmooth_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as simsmooth_ar_batch_dev."""
    return _simsmooth_ar(ctx, _k._NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), D, H, v0, seed, first_draw, mean, sd, want_x,
                         may_have_missing, singular_q)


for _f in (simsmooth_ar_batch_dev, simsmooth_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
