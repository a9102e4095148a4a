"""Binding of the diffusion-index evaluation entries (include/dfm_hip.h, csrc/diffusion.hip): dfm_diffusion_eval_batch[_dev].  The
functions take a DfmContext; importing this module (kalman.py does) also attaches them to DfmContext as diffusion_eval_batch and
diffusion_eval_batch_host, with the conventions of rolling.py: device tensors in and resident tensors out on torch's current stream,
or NumPy through the host-pointer entry; the origins and the publication lags are host integers on both sides.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import kalman as _k

OUTPUTS = ("fc", "fc_ar", "fvar", "err", "err_ar", "err_std", "msfe", "msfe_ar", "msfe0", "cnt", "F", "Lam", "iters", "ssr", "mean",
           "sd", "nobs")                                                                       # the default of `want`
ALL_OUTPUTS = OUTPUTS + ("beta", "nobs_reg", "win")


def _diffusion(ctx, be, x, origins, W, H, F_start, q, lags, min_obs, nt_min, max_iter, tol, want, may_have_missing):
    """dfm_diffusion_eval_batch[_dev] through backend `be`.  Every check here runs before the device is touched."""
    x = be.inp(x)
    if x.ndim != 2:
        raise ValueError("x must be one [T, N] panel")
    T, N = x.shape
    F_start = be.inp(F_start)
    org = np.ascontiguousarray(np.asarray(origins, dtype=np.int64).reshape(-1), dtype=np.int32)
    O, W, H, q, max_iter = org.size, int(W), int(H), int(q), int(max_iter)
    if O < 1:
        raise ValueError("at least one origin is needed")
    if F_start.ndim == 2 and tuple(F_start.shape)[0] == T:
        n_start, r = 1, F_start.shape[1]
    elif F_start.ndim == 3 and tuple(F_start.shape)[:2] == (O, W):
        n_start, r = O, F_start.shape[2]
    else:
        raise ValueError(f"F_start must be [T={T}, r] (one path) or [O={O}, W={W}, r] (one start per window)")
    lg = None if lags is None else np.ascontiguousarray(np.asarray(lags, dtype=np.int64).reshape(-1), dtype=np.int32)
    if lg is not None and lg.size != N:
        raise ValueError(f"lags must hold N = {N} integers")
    min_obs = r + 1 if min_obs is None else int(min_obs)
    unknown = set(want) - set(ALL_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}: choose from {ALL_OUTPUTS}")
    if max_iter < 0 or H < 0 or q < 0:
        raise ValueError("max_iter, H and q must be >= 0")
    if may_have_missing is None:
        may_have_missing = bool(lg is not None and (lg > 0).any()) or be.has_nan(x)
    flags = _k._flags(may_have_missing)
    K = 1 + r + q
    w = lambda name, *shape, **kw: be.out(*shape, **kw) if name in want else None
    out = dict(F=w("F", O, W, r), Lam=w("Lam", O, N, r), iters=w("iters", O, int32=True), ssr=w("ssr", O), mean=w("mean", O, N),
               sd=w("sd", O, N), nobs=w("nobs", O, N, int32=True), win=w("win", O, W, N), fc=w("fc", O, H + 1, N),
               fc_ar=w("fc_ar", O, H + 1, N), fvar=w("fvar", O, H + 1, N), err=w("err", O, H + 1, N), err_ar=w("err_ar", O, H + 1, N),
               err_std=w("err_std", O, H + 1, N), beta=w("beta", O, H + 1, N, K), nobs_reg=w("nobs_reg", O, H + 1, N, int32=True),
               msfe=w("msfe", H + 1, N), msfe_ar=w("msfe_ar", H + 1, N), msfe0=w("msfe0", H + 1, N), cnt=w("cnt", H + 1, N, int32=True))
    raw = lambda a: None if a is None else be.raw(a)
    p = lambda name: be.ptr(out[name], name)
    be.sync()
    rc = getattr(ctx._lib, "dfm_diffusion_eval_batch" + be.suffix)(
        ctx._h, T, N, r, q, W, H, O, min_obs, int(nt_min), n_start, be.ptr(x, "x"), _k._ptr(org), _k._ptr(lg), be.ptr(F_start, "F_start"),
        max_iter, float(tol), p("F"), p("Lam"), raw(out["iters"]), p("ssr"), p("mean"), p("sd"), raw(out["nobs"]), p("win"), p("fc"),
        p("fc_ar"), p("fvar"), p("err"), p("err_ar"), p("err_std"), p("beta"), raw(out["nobs_reg"]), p("msfe"), p("msfe_ar"), p("msfe0"),
        raw(out["cnt"]), flags)
    _k._check(ctx._h, rc)
    out.update(origins=org)
    return out


def diffusion_eval_batch(ctx, x, origins, W: int, H: int, F_start, q: int = 0, lags=None, min_obs: Optional[int] = None,
                         nt_min: int = 0, max_iter: int = 1000, tol: float = 1e-8, want=OUTPUTS,
                         may_have_missing: Optional[bool] = None):
    """dfm_diffusion_eval_batch_dev (device tensors, torch's current stream): the out-of-sample record of diffusion-index forecasts of
    the raw panel x [T,N], the factors re-estimated by ALS at every origin (include/dfm_hip.h).  origins: O increasing 0-based rows in
    W-1 .. T-1; F_start [T,r] (one path, cut per window) or [O,W,r] (not modified); q own lags; lags: N publication lags or None;
    min_obs: default r + 1; nt_min, max_iter, tol of the ALS (max_iter = 0: the factors are the start).  Returns a dict of resident
    tensors, of `want`: fc, fc_ar, fvar, err, err_ar, err_std [O,H+1,N], beta [O,H+1,N,1+r+q], nobs_reg [O,H+1,N], msfe, msfe_ar,
    msfe0, cnt [H+1,N], F [O,W,r], Lam [O,N,r], iters, ssr [O], mean, sd, nobs [O,N], win [O,W,N]; the others are None (beta, nobs_reg
    and win are not in the default).  The status word (DFM_E_MISSING) is read by synchronize(); DFM_E_WINDOW is raised by the call."""
    return _diffusion(ctx, _k._Torch(ctx, x), x, origins, W, H, F_start, q, lags, min_obs, nt_min, max_iter, tol, want, may_have_missing)


def diffusion_eval_batch_host(ctx, x, origins, W: int, H: int, F_start, q: int = 0, lags=None, min_obs: Optional[int] = None,
                              nt_min: int = 0, max_iter: int = 1000, tol: float = 1e-8, want=OUTPUTS,
                              may_have_missing: Optional[bool] = None):
    """dfm_diffusion_eval_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as diffusion_eval_batch."""
    return _diffusion(ctx, _k._NP, x, origins, W, H, F_start, q, lags, min_obs, nt_min, max_iter, tol, want, may_have_missing)


for _f in (diffusion_eval_batch, diffusion_eval_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
