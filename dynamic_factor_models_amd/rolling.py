"""Binding of the rolling-window evaluation entries (include/dfm_hip.h, csrc/rolling.hip): dfm_rolling_eval_batch[_dev].  The functions
take a DfmContext; importing this module (kalman.py does) also attaches them to DfmContext as rolling_eval_batch and
rolling_eval_batch_host, on the marshalling of the `_varp` family (em_varp_batch) and with the conventions of simulate.py: device
tensors in and resident tensors out on torch's current stream, or NumPy through the host-pointer entry.  The origins and the
publication lags are host integers on both sides, as the targets of news_batch are.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import kalman as _k

OUTPUTS = ("fc", "fvar", "err", "err_std", "msfe", "msfe0", "cnt", "mean", "sd", "nobs")      # the default of `want`
ALL_OUTPUTS = OUTPUTS + ("win",)


def _rolling(ctx, be, x, origins, W, H, start, lags, sd_start, min_obs, max_iter, tol, want, may_have_missing, singular_q):
    """dfm_rolling_eval_batch[_dev] through backend `be`.  Every check here runs before the device is touched."""
    x = be.inp(x)
    if x.ndim != 2:
        raise ValueError("x must be one [T, N] panel")
    T, N = x.shape
    start = [be.inp(a) for a in start]
    if start[0].ndim != 3 or start[0].shape[1] != N:
        raise ValueError(f"Lam of the start must be [n_start, N={N}, r]")
    n_start, _, r = start[0].shape
    (p,), _, shapes = _k._VARP.geom(n_start, int(W), N, r, *start)
    org = np.ascontiguousarray(np.asarray(origins, dtype=np.int64).reshape(-1), dtype=np.int32)
    O, W, H, max_iter = org.size, int(W), int(H), int(max_iter)
    lg = None if lags is None else np.ascontiguousarray(np.asarray(lags, dtype=np.int64).reshape(-1), dtype=np.int32)
    if lg is not None and lg.size != N:
        raise ValueError(f"lags must hold N = {N} integers")
    min_obs = r + 1 if min_obs is None else int(min_obs)
    unknown = set(want) - set(ALL_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}: choose from {ALL_OUTPUTS}")
    if O < 1:
        raise ValueError("at least one origin is needed")
    if max_iter < 0 or H < 0:
        raise ValueError("max_iter and H must be >= 0")
    sd_start = None if sd_start is None else be.inp(sd_start)
    if may_have_missing is None:
        may_have_missing = bool(lg is not None and (lg > 0).any()) or be.has_nan(x)
    flags = _k._flags(may_have_missing, singular_q)
    params = [be.out(O, *s[1:]) for s in shapes]
    path = be.out(O, max_iter) if max_iter else None
    iters = be.out(O, int32=True)
    w = lambda name, *shape, **kw: be.out(*shape, **kw) if name in want else None
    out = dict(fc=w("fc", O, H + 1, N), fvar=w("fvar", O, H + 1, N), err=w("err", O, H + 1, N), err_std=w("err_std", O, H + 1, N),
               msfe=w("msfe", H + 1, N), msfe0=w("msfe0", H + 1, N), cnt=w("cnt", H + 1, N, int32=True),
               mean=w("mean", O, N), sd=w("sd", O, N), nobs=w("nobs", O, N, int32=True), win=w("win", O, W, N))
    raw = lambda a: None if a is None else be.raw(a)
    be.sync()
    rc = getattr(ctx._lib, "dfm_rolling_eval_batch" + be.suffix)(
        ctx._h, T, N, r, p, W, H, O, min_obs, n_start, be.ptr(x, "x"), _k._ptr(org), _k._ptr(lg),
        *_k._ptrs(be, _k._VARP, start, shapes), be.ptr(sd_start, "sd_start", (N,)), max_iter, float(tol),
        *[be.ptr(a, n) for a, n in zip(params, _k._VARP.names)], be.ptr(path, "loglik_path"), be.raw(iters),
        be.ptr(out["mean"], "win_mean"), be.ptr(out["sd"], "win_sd"), raw(out["nobs"]), be.ptr(out["win"], "windows"), be.ptr(out["fc"], "fc"),
        be.ptr(out["fvar"], "fvar"), be.ptr(out["err"], "err"), be.ptr(out["err_std"], "err_std"), be.ptr(out["msfe"], "msfe"),
        be.ptr(out["msfe0"], "msfe0"), raw(out["cnt"]), flags)
    _k._check(ctx._h, rc)
    out.update(params=dict(zip(_k._VARP.names, params)), loglik_path=path, iters=iters, origins=org)
    return out


def rolling_eval_batch(ctx, x, origins, W: int, H: int, Lam, R, Avar, Q, mu0, P0, lags=None, sd_start=None,
                       min_obs: Optional[int] = None, max_iter: int = 10, tol: float = 0.0, want=OUTPUTS,
                       may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_rolling_eval_batch_dev (device tensors, torch's current stream): the rolling-window out-of-sample record of the raw
    panel x [T,N], re-estimated at every origin (include/dfm_hip.h).  origins: O increasing 0-based rows in W-1 .. T-1; lags: N
    publication lags or None; the start Lam [n,N,r], R [n,N], Avar [n,r,r p], Q [n,r,r], mu0 [n,r p], P0 [n,r p,r p] with n = 1 or O
    (not modified), in the units sd_start [N] says (None: the windows' own).  min_obs: default r + 1.  max_iter = 0: no EM.
    Returns a dict of resident tensors: params (the windows' parameters by name, [O,..]), loglik_path [O,max_iter] (None without EM),
    iters [O], and of `want`: fc, fvar, err, err_std [O,H+1,N], msfe, msfe0, cnt [H+1,N], mean, sd, nobs [O,N], win [O,W,N] (the standardised vintages; not in the default); the others are None.
    The status word (DFM_E_MISSING) is read by synchronize(); DFM_E_WINDOW is raised by the call itself."""
    return _rolling(ctx, _k._Torch(ctx, x), x, origins, W, H, (Lam, R, Avar, Q, mu0, P0), lags, sd_start, min_obs, max_iter, tol, want,
                    may_have_missing, singular_q)


def rolling_eval_batch_host(ctx, x, origins, W: int, H: int, Lam, R, Avar, Q, mu0, P0, lags=None, sd_start=None,
                            min_obs: Optional[int] = None, max_iter: int = 10, tol: float = 0.0, want=OUTPUTS,
                            may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_rolling_eval_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as rolling_eval_batch."""
    return _rolling(ctx, _k._NP, x, origins, W, H, (Lam, R, Avar, Q, mu0, P0), lags, sd_start, min_obs, max_iter, tol, want,
                    may_have_missing, singular_q)


for _f in (rolling_eval_batch, rolling_eval_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
