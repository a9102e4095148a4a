"""Binding of the forecast entries of the model with AR idiosyncratic terms (include/dfm_hip.h, csrc/forecast_ar.hip):
dfm_forecast_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to
DfmContext as forecast_ar_batch_dev and forecast_ar_batch_host, on the marshalling of the `_ar` family (ks_pass_ar_batch) and
with the conventions of forecast_batch(_host): device tensors in and out on torch's current stream, or NumPy through the
host-pointer entry.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k

CELLS = ("xhat", "xvar", "common", "idio")
OPTIONAL = ("xvar", "common", "idio", "P", "loglik")


def check_args(T: int, q: int, H: int):
    """The argument rules of dfm_forecast_ar_batch that need no device."""
    if int(H) < 0:
        raise ValueError("H must be >= 0")
    if not (1 <= int(q) <= 4):
        raise ValueError("the forecasts need 1 <= q <= 4 idiosyncratic lags (q = 0 is forecast_batch)")
    if int(T) <= int(q):
        raise ValueError("T must exceed the number of idiosyncratic lags")


def _forecast_ar(ctx, be, panel, params, H, v0, mean, sd, want, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._AR, be, panel, params)
    B, T, N, r, p, q = dims
    H = int(H)
    check_args(T, q, H)
    want = OPTIONAL if want is None else tuple(want)
    unknown = [w for w in want if w not in OPTIONAL]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}: choose among {OPTIONAL} (xhat and f are always returned)")
    mean, sd = _k._pair(be, mean, sd)
    v0 = None if v0 is None else be.inp(v0)
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    n = T + H - q
    out = dict(xhat=be.out(B, n, N), f=be.out(B, n, r))
    for name in CELLS[1:]:
        out[name] = be.out(B, n, N) if name in want else None
    out["P"] = be.out(B, n, r * (r + 1) // 2) if "P" in want else None
    out["loglik"] = be.out(B) if "loglik" in want else None
    be.sync()
    rc = getattr(ctx._lib, "dfm_forecast_ar_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, q, H, be.ptr(panel, "panel"), *_k._ptrs(be, _k._AR, params, shapes),
        be.ptr(v0, "v0", (B, N)), be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)),
        *[be.ptr(out[name], name) for name in CELLS], be.ptr(out["f"], "f_out"), be.ptr(out["P"], "P_out"),
        be.ptr(out["loglik"], "loglik"), flags)
    _k._check(ctx._h, rc)
    return out


def forecast_ar_batch_dev(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, H: int, v0=None, mean=None, sd=None, want=None,
                          may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_forecast_ar_batch_dev (device tensors, torch's current stream): nowcasts and forecasts of the panel from the model with
    AR(q) idiosyncratic terms over the n = T + H - q rows q .. T + H - 1.  Parameters as ks_pass_ar_batch; v0 [B,N] is the variance
    of the q idiosyncratic terms before output row 0 (None: sig2); mean / sd [B,N] (both or neither) put the cells into data
    units; `want` names the optional outputs to compute (default all of OPTIONAL).  Returns dict(xhat, xvar, common, idio [B,n,N],
    f [B,n,r], P [B,n,r(r+1)/2], loglik [B]); the outputs not asked for are None."""
    return _forecast_ar(ctx, _k._Torch(ctx, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), H, v0, mean, sd, want,
                        may_have_missing, singular_q)


def forecast_ar_batch_host(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, H: int, v0=None, mean=None, sd=None, want=None,
                           may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_forecast_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as forecast_ar_batch_dev."""
    return _forecast_ar(ctx, _k._NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), H, v0, mean, sd, want, may_have_missing,
                        singular_q)


for _f in (forecast_ar_batch_dev, forecast_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
