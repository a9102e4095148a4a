"""Binding of the news decomposition of the model with AR idiosyncratic terms (include/dfm_hip.h, csrc/news_ar.hip):
dfm_news_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to DfmContext
as news_ar_batch_dev and news_ar_batch_host, on the marshalling of the `_ar` family (ks_pass_ar_batch) and with the conventions of
news_batch(_host): device tensors in and out on torch's current stream, or NumPy through the host-pointer entry.

edge_shape_error is the vintage rule of the call as a host-side check: what the device raises as DFM_E_VINTAGE, said in words.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import kalman as _k


def check_args(T: int, q: int, targets):
    """The argument rules of dfm_news_ar_batch that need no device; returns the targets as an [G, 2] int64 array."""
    if not (1 <= int(q) <= 4):
        raise ValueError("the news decomposition needs 1 <= q <= 4 idiosyncratic lags (q = 0 is news_batch)")
    if int(T) <= 2 * int(q):
        raise ValueError("T must exceed 2 q: q conditioning rows and q rows that fix the idiosyncratic state")
    tg = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
    if tg.shape[0] and np.any(tg[:, 0] < int(q)):
        raise ValueError("a target row lies in the first q panel rows: those are conditioning values, not outputs")
    return tg


def edge_shape_error(old, new, q: int, cols=None) -> Optional[str]:
    """None when the vintages old / new [..., T, N] (NaN = missing) are what dfm_news_ar_batch accepts, else a sentence that names
    the first offending column and which condition it breaks:
      (1) in both vintages the observed rows of a column are exactly 0 .. L (no interior gap, no late start);
      (2) L >= 2 q - 1 in old (a never-observed column has L = -1);
      (3) every cell observed in old is observed in new.
    cols: the names of the columns (default: their positions)."""
    col = (lambda i: int(i)) if cols is None else (lambda i: cols[int(i)])
    oo, on = ~np.isnan(np.asarray(old, dtype=np.float64)), ~np.isnan(np.asarray(new, dtype=np.float64))
    T, N = oo.shape[-2:]
    oo, on = oo.reshape(-1, T, N), on.reshape(-1, T, N)
    rows = np.arange(T)[None, :, None]
    for name, m in (("old", oo), ("new", on)):
        cnt = m.sum(axis=1)                                         # [B, N]
        bad = (m & (rows >= cnt[:, None, :])).any(axis=1)           # an observed cell behind the first cnt rows
        if bad.any():
            b, i = np.argwhere(bad)[0]
            t = int(np.argmin(m[b, :, i]))
            kind = "starts late" if t == 0 else "has an interior gap"
            return (f"column {col(i)} (replicate {b}) of the {name} vintage {kind} (row {t} is missing before an observed row): "
                    "condition 1, the observed rows of a column must be exactly 0 .. L")
    cnt = oo.sum(axis=1)
    short = cnt < 2 * int(q)
    if short.any():
        b, i = np.argwhere(short)[0]
        what = "is never observed" if cnt[b, i] == 0 else f"has {cnt[b, i]} observed rows"
        return (f"column {col(i)} (replicate {b}) of the old vintage {what}: condition 2, it needs at least 2 q = {2 * int(q)} "
                "(q conditioning rows and q rows that fix its idiosyncratic state)")
    lost = (oo & ~on).any(axis=1)
    if lost.any():
        b, i = np.argwhere(lost)[0]
        return (f"column {col(i)} (replicate {b}) has a cell that is observed in the old vintage and missing in the new one: "
                "condition 3, the old vintage's cells must be a subset of the new one's")
    return None


def _news_ar(ctx, be, old, new, params, targets, v0, mean, sd, want_news, want_weight, may_have_missing, singular_q):
    new, params, dims, _, shapes = _k._model(_k._AR, be, new, params)
    B, T, N, r, p, q = dims
    check_args(T, q, targets)
    old = be.inp(old)
    if tuple(old.shape) != (B, T, N):
        raise ValueError("old and new must have the same shape")
    mean, sd = _k._pair(be, mean, sd)
    v0 = None if v0 is None else be.inp(v0)
    tt, ti = ctx._targets(targets, T, N)
    G = tt.size
    flags = _k._flags(may_have_missing, singular_q, be, new)         # the NEW vintage is the one scanned
    yhat, impact = be.out(B, 3, G), be.out(B, G, N)
    news = be.out(B, T - q, N) if want_news else None
    weight = be.out(B, G, T - q, N) if want_weight else None
    be.sync()
    rc = getattr(ctx._lib, "dfm_news_ar_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, q, be.ptr(old, "old"), be.ptr(new, "new"), *_k._ptrs(be, _k._AR, params, shapes),
        be.ptr(v0, "v0", (B, N)), be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), G, _k._ptr(tt), _k._ptr(ti),
        be.ptr(yhat, "yhat"), be.ptr(impact, "impact"), be.ptr(news, "news"), be.ptr(weight, "weight"), flags)
    _k._check(ctx._h, rc)
    return dict(yhat=yhat, impact=impact, news=news, weight=weight)


def news_ar_batch_dev(ctx, old, new, Lam, sig2, rho, Avar, Q, mu0, P0, targets, v0=None, mean=None, sd=None,
                      want_news: bool = True, want_weight: bool = True, may_have_missing: Optional[bool] = None,
                      singular_q: bool = False):
    """dfm_news_ar_batch_dev (device tensors, torch's current stream): the news decomposition of the revision of G target cells
    between two edge-shaped vintages old / new [B,T,N] under the model with AR(q) idiosyncratic terms.  Parameters as
    ks_pass_ar_batch, v0 / mean / sd as forecast_ar_batch; targets: G (panel row t* >= q, column i*) pairs, 0-based, host side.
    Returns dict(yhat [B,3,G] (old, revised, new), impact [B,G,N], news [B,T-q,N] or None, weight [B,G,T-q,N] or None) on the
    output rows (panel rows q ..); the status word (DFM_E_VINTAGE: a vintage that is not edge-shaped) is read by synchronize()."""
    return _news_ar(ctx, _k._Torch(ctx, new), old, new, (Lam, sig2, rho, Avar, Q, mu0, P0), targets, v0, mean, sd, want_news,
                    want_weight, may_have_missing, singular_q)


def news_ar_batch_host(ctx, old, new, Lam, sig2, rho, Avar, Q, mu0, P0, targets, v0=None, mean=None, sd=None,
                       want_news: bool = True, want_weight: bool = True, may_have_missing: Optional[bool] = None,
                       singular_q: bool = False):
    """dfm_news_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as news_ar_batch_dev."""
    return _news_ar(ctx, _k._NP, old, new, (Lam, sig2, rho, Avar, Q, mu0, P0), targets, v0, mean, sd, want_news, want_weight,
                    may_have_missing, singular_q)


for _f in (news_ar_batch_dev, news_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
