"""Binding of the structural entries of include/dfm_hip.h (csrc/structural.hip, csrc/signirf.hip, csrc/proxy.hip):
dfm_irf_batch[_dev], dfm_histdecomp_batch[_dev], dfm_signirf_batch[_dev] and dfm_proxyirf_batch[_dev].  The functions take a
DfmContext; importing this module (kalman.py does) also attaches them to DfmContext as irf_batch, irf_batch_host, histdecomp_batch,
histdecomp_batch_host, signirf_batch, signirf_batch_host, proxyirf_batch and proxyirf_batch_host, with the marshalling conventions of forecast_batch(_host): device tensors in and out on torch's current
stream, or NumPy through the host-pointer entries.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from . import kalman as _k


def _index(idx, n, what, distinct):
    """A host int32 array of series indices (None stays None)."""
    if idx is None:
        return None
    a = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    if a.size != n:
        raise ValueError(f"{what} must have {n} entries")
    if distinct and (np.any(a < 0) or np.unique(a).size != a.size):
        raise ValueError(f"{what} must be distinct, non-negative series indices")
    return np.ascontiguousarray(a, dtype=np.int32)


def _irf(ctx, be, Lam, Avar, Q, R, H, sd, named, cum, unit_effect, want_fevd):
    Lam, Avar, Q = be.inp(Lam), be.inp(Avar), be.inp(Q)
    B, N, r = Lam.shape
    p = Avar.shape[2] // r
    if int(H) < 1:
        raise ValueError("H must be >= 1")
    if unit_effect and named is None:
        raise ValueError("unit_effect needs named series")
    if want_fevd and R is None:
        raise ValueError("the variance decomposition needs R")
    R = None if R is None else be.inp(R)
    sd = None if sd is None else be.inp(sd)
    named = _index(named, r, "named", True)
    cum = _index(cum, N, "cum", False)
    irf = be.out(B, r, int(H), N)
    fevd = be.out(B, r + 1, int(H), N) if want_fevd else None
    be.sync()
    rc = getattr(ctx._lib, "dfm_irf_batch" + be.suffix)(
        ctx._h, B, N, r, p, int(H), be.ptr(Lam, "Lam", (B, N, r)), be.ptr(Avar, "Avar", (B, r, r * p)), be.ptr(Q, "Q", (B, r, r)),
        be.ptr(R, "R", (B, N)), be.ptr(sd, "sd", (B, N)), _k._ptr(named), _k._ptr(cum), be.ptr(irf, "irf"), be.ptr(fevd, "fevd"),
        _lib.DFM_SV_UNIT_EFFECT if unit_effect else 0)
    _k._check(ctx._h, rc)
    return dict(irf=irf, fevd=fevd)


def _histdecomp(ctx, be, panel, params, sd, named, want_shocks, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._VARP, be, panel, params)
    B, T, N, r, p = dims
    sd = None if sd is None else be.inp(sd)
    named = _index(named, r, "named", True)
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    hd = be.out(B, r + 1, T, N)
    shocks = be.out(B, T, r) if want_shocks else None
    f, ll = be.out(B, T, r), be.out(B)
    be.sync()
    rc = getattr(ctx._lib, "dfm_histdecomp_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, be.ptr(panel, "panel"), *_k._ptrs(be, _k._VARP, params, shapes), be.ptr(sd, "sd", (B, N)),
        _k._ptr(named), be.ptr(hd, "hd"), be.ptr(shocks, "shocks"), be.ptr(f, "f_out"), be.ptr(ll, "loglik"), flags)
    _k._check(ctx._h, rc)
    return dict(hd=hd, shocks=shocks, f=f, loglik=ll)


def _restrictions(restrictions):
    """The restrictions as a host int32 [G, 5] array of (series, shock, h0, h1, sign) rows; none: G = 0 and no array."""
    if restrictions is None:
        return 0, None
    a = np.asarray(restrictions, dtype=np.int64)
    if a.size == 0:
        return 0, None
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("restrictions must be (series, shock, h0, h1, sign) rows")
    if np.any(np.abs(a[:, 4]) != 1):
        raise ValueError("the sign of a restriction must be +1 or -1")
    return a.shape[0], np.ascontiguousarray(a, dtype=np.int32)


def _signirf(ctx, be, Lam, Avar, Q, R, H, restrictions, candidates, keep, seed, first_cand, sd, named, cum, want_mask, want_S,
             want_irf, want_fevd):
    Lam, Avar, Q = be.inp(Lam), be.inp(Avar), be.inp(Q)
    B, N, r = Lam.shape
    p = Avar.shape[2] // r
    H, M, K = int(H), int(candidates), int(keep)
    if H < 1:
        raise ValueError("H must be >= 1")
    if M < 1 or K < 1:
        raise ValueError("candidates and keep must be >= 1")
    if want_fevd and R is None:
        raise ValueError("the variance decomposition needs R")
    G, restr = _restrictions(restrictions)
    R = None if R is None else be.inp(R)
    sd = None if sd is None else be.inp(sd)
    named = _index(named, r, "named", True)
    cum = _index(cum, N, "cum", False)
    n_accept = be.out(B, int32=True)
    mask = be.out(B, M, int32=True) if want_mask else None
    cand = be.out(B, K, int32=True)
    S = be.out(B, K, r, r) if want_S else None
    irf = be.out(B, K, r, H, N) if want_irf else None
    fevd = be.out(B, K, r + 1, H, N) if want_fevd else None
    be.sync()
    rc = getattr(ctx._lib, "dfm_signirf_batch" + be.suffix)(
        ctx._h, B, N, r, p, H, be.ptr(Lam, "Lam", (B, N, r)), be.ptr(Avar, "Avar", (B, r, r * p)), be.ptr(Q, "Q", (B, r, r)),
        be.ptr(R, "R", (B, N)), be.ptr(sd, "sd", (B, N)), _k._ptr(named), _k._ptr(cum), G, _k._ptr(restr), M, K,
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_cand), be.raw(n_accept), None if mask is None else be.raw(mask), be.raw(cand),
        be.ptr(S, "S_out"), be.ptr(irf, "irf"), be.ptr(fevd, "fevd"), 0)
    _k._check(ctx._h, rc)
    return dict(n_accept=n_accept, mask=mask, cand=cand, S=S, irf=irf, fevd=fevd)


def _proxyirf(ctx, be, panel, params, H, instrument, norm, draws, block, seed, first_draw, sd, cum, unit_effect, want_irf, want_fevd,
              want_shock, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._VARP, be, panel, params)
    B, T, N, r, p = dims
    H, D, L, norm, first_draw = int(H), int(draws), int(block), int(norm), int(first_draw)
    if H < 1:
        raise ValueError("H must be >= 1")
    if D < 0 or first_draw < 0:
        raise ValueError("draws and first_draw must be >= 0")
    if not 0 <= norm < N:
        raise ValueError(f"norm must be a series index in 0..{N - 1}")
    z = np.ascontiguousarray(np.asarray(instrument, dtype=np.float64).reshape(-1))
    if z.size != T:
        raise ValueError(f"the instrument must have {T} entries, one per period")
    n = int(np.isfinite(z[p:]).sum())
    if n < r + 2:
        raise ValueError(f"the instrument has {n} usable periods; at least r + 2 = {r + 2} are needed")
    if not 1 <= L <= n:
        raise ValueError(f"block must lie in 1..{n} (the usable periods)")
    sd = None if sd is None else be.inp(sd)
    cum = _index(cum, N, "cum", False)
    flags = _k._flags(may_have_missing, singular_q, be, panel) | (_lib.DFM_SV_UNIT_EFFECT if unit_effect else 0)
    impact, rel = be.out(B, D + 1, r), be.out(B, D + 1)
    irf = be.out(B, D + 1, H, N) if want_irf else None
    fevd = be.out(B, D + 1, H, N) if want_fevd else None
    shock = be.out(B, T) if want_shock else None
    f, ll = be.out(B, T, r), be.out(B)
    be.sync()
    rc = getattr(ctx._lib, "dfm_proxyirf_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, H, be.ptr(panel, "panel"), *_k._ptrs(be, _k._VARP, params, shapes), be.ptr(sd, "sd", (B, N)),
        _k._ptr(cum), _k._ptr(z), norm, D, L, int(seed) & 0xFFFFFFFFFFFFFFFF, first_draw, be.ptr(impact, "impact"),
        be.ptr(rel, "rel"), be.ptr(irf, "irf"), be.ptr(fevd, "fevd"), be.ptr(shock, "shock"), be.ptr(f, "f_out"),
        be.ptr(ll, "loglik"), flags)
    _k._check(ctx._h, rc)
    return dict(impact=impact, rel=rel, irf=irf, fevd=fevd, shock=shock, f=f, loglik=ll)


def proxyirf_batch(ctx, panel, Lam, R, Avar, Q, mu0, P0, H: int, instrument, norm: int, draws: int = 0, block: int = 1,
                   seed: int = 0, first_draw: int = 0, sd=None, cum=None, unit_effect: bool = False, want_irf: bool = True,
                   want_fevd: bool = False, want_shock: bool = True, may_have_missing: Optional[bool] = None,
                   singular_q: bool = False):
    """dfm_proxyirf_batch_dev (device tensors, torch's current stream): the shock identified by the external `instrument` (host
    side, one entry per period, NaN = not available), signed by series `norm`; slot 0 is the sample, slots 1 .. draws are moving
    block draws (length `block`) of the instrument moment.  Parameters as histdecomp_batch, cum as irf_batch.  Returns dict(impact
    [B,draws+1,r], rel [B,draws+1], irf [B,draws+1,H,N], fevd [B,draws+1,H,N], shock [B,T], f [B,T,r], loglik [B]; None when not
    asked for).  Draws first_draw .. first_draw + draws - 1 of the stream of `seed`."""
    return _proxyirf(ctx, _k._Torch(ctx, panel), panel, (Lam, R, Avar, Q, mu0, P0), H, instrument, norm, draws, block, seed,
                     first_draw, sd, cum, unit_effect, want_irf, want_fevd, want_shock, may_have_missing, singular_q)


def proxyirf_batch_host(ctx, panel, Lam, R, Avar, Q, mu0, P0, H: int, instrument, norm: int, draws: int = 0, block: int = 1,
                        seed: int = 0, first_draw: int = 0, sd=None, cum=None, unit_effect: bool = False, want_irf: bool = True,
                        want_fevd: bool = False, want_shock: bool = True, may_have_missing: Optional[bool] = None,
                        singular_q: bool = False):
    """dfm_proxyirf_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as proxyirf_batch."""
    return _proxyirf(ctx, _k._NP, panel, (Lam, R, Avar, Q, mu0, P0), H, instrument, norm, draws, block, seed, first_draw, sd, cum,
                     unit_effect, want_irf, want_fevd, want_shock, may_have_missing, singular_q)


def signirf_batch(ctx, Lam, Avar, Q, R, H: int, restrictions, candidates: int, keep: int = 1, seed: int = 0, first_cand: int = 0,
                  sd=None, named=None, cum=None, want_mask: bool = False, want_S: bool = True, want_irf: bool = True,
                  want_fevd: bool = False):
    """dfm_signirf_batch_dev (device tensors, torch's current stream): `candidates` Haar rotations of the base impact matrix per
    replicate, those whose responses satisfy the sign `restrictions` ((series, shock, h0, h1, sign) rows, host side) accepted, the
    first `keep` accepted ones written out.  Inputs as irf_batch.  Returns dict(n_accept [B] int32, mask [B,candidates] int32 or
    None, cand [B,keep] int32 (-1: empty slot), S [B,keep,r,r], irf [B,keep,r,H,N], fevd [B,keep,r+1,H,N]; None when not asked
    for; NaN in empty slots).  Candidates first_cand .. first_cand + candidates - 1 of the stream of `seed`."""
    return _signirf(ctx, _k._Torch(ctx, Lam), Lam, Avar, Q, R, H, restrictions, candidates, keep, seed, first_cand, sd, named, cum,
                    want_mask, want_S, want_irf, want_fevd)


def signirf_batch_host(ctx, Lam, Avar, Q, R, H: int, restrictions, candidates: int, keep: int = 1, seed: int = 0,
                       first_cand: int = 0, sd=None, named=None, cum=None, want_mask: bool = False, want_S: bool = True,
                       want_irf: bool = True, want_fevd: bool = False):
    """dfm_signirf_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as signirf_batch."""
    return _signirf(ctx, _k._NP, Lam, Avar, Q, R, H, restrictions, candidates, keep, seed, first_cand, sd, named, cum, want_mask,
                    want_S, want_irf, want_fevd)


def irf_batch(ctx, Lam, Avar, Q, R, H: int, sd=None, named=None, cum=None, unit_effect: bool = False, want_fevd: bool = True):
    """dfm_irf_batch_dev (device tensors, torch's current stream): identified impulse responses irf [B,r,H,N] and forecast-error
    variance shares fevd [B,r+1,H,N] (None when not asked for) of every series.  Lam [B,N,r], Avar [B,r,r p], Q [B,r,r], R [B,N];
    sd [B,N] puts irf into data units; named (r distinct series, host side) identifies the shocks, cum (N flags, host side) marks
    the series whose outputs are cumulated.  The status word (a singular Lam[named]) is read by synchronize()."""
    return _irf(ctx, _k._Torch(ctx, Lam), Lam, Avar, Q, R, H, sd, named, cum, unit_effect, want_fevd)


def irf_batch_host(ctx, Lam, Avar, Q, R, H: int, sd=None, named=None, cum=None, unit_effect: bool = False,
                   want_fevd: bool = True):
    """dfm_irf_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as irf_batch."""
    return _irf(ctx, _k._NP, Lam, Avar, Q, R, H, sd, named, cum, unit_effect, want_fevd)


def histdecomp_batch(ctx, panel, Lam, R, Avar, Q, mu0, P0, sd=None, named=None, want_shocks: bool = True,
                     may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_histdecomp_batch_dev (device tensors, torch's current stream): the smoother pass, the structural shocks and the
    contribution of every shock and of the initial condition to every cell.  Parameters as forecast_batch; returns dict(hd
    [B,r+1,T,N], shocks [B,T,r] or None, f [B,T,r], loglik [B])."""
    return _histdecomp(ctx, _k._Torch(ctx, panel), panel, (Lam, R, Avar, Q, mu0, P0), sd, named, want_shocks, may_have_missing,
                       singular_q)


def histdecomp_batch_host(ctx, panel, Lam, R, Avar, Q, mu0, P0, sd=None, named=None, want_shocks: bool = True,
                          may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_histdecomp_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as histdecomp_batch."""
    return _histdecomp(ctx, _k._NP, panel, (Lam, R, Avar, Q, mu0, P0), sd, named, want_shocks, may_have_missing, singular_q)


for _f in (irf_batch, irf_batch_host, histdecomp_batch, histdecomp_batch_host, signirf_batch, signirf_batch_host, proxyirf_batch,
           proxyirf_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
