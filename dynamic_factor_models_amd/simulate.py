"""Binding of the simulated-panel entries (include/dfm_hip.h, csrc/simulate.hip): dfm_simulate_batch[_dev] and
dfm_simulate_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to
DfmContext as simulate_batch, simulate_batch_host, simulate_ar_batch and simulate_ar_batch_host, on the marshalling of the `_varp`
and `_ar` families (ks_pass_varp_batch, ks_pass_ar_batch) and with the conventions of simsmooth_batch(_host): device tensors in and
resident tensors out on torch's current stream, or NumPy through the host-pointer entry.  There is one difference: the panel is
optional here, so the shapes come from the loadings and T.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k


def _simulate(ctx, fam, be, params, D, T, panel, v0, seed, first_draw, want_f):
    """dfm_simulate<_ar>_batch[_dev] through backend `be` (fam: _VARP or _AR): dict(x [B,D,T,N], f [B,D,rows,r] or None).
    The panel (the mask panel of the plain model) may be None: T then says how many rows to draw."""
    params = [be.inp(a) for a in params]
    B, N, r = params[0].shape
    if int(D) < 1:
        raise ValueError("D must be >= 1")
    if panel is not None:
        panel = be.inp(panel)
        if panel.ndim != 3 or panel.shape[0] != B or panel.shape[2] != N or (T is not None and int(T) != panel.shape[1]):
            raise ValueError(f"panel: shape {tuple(panel.shape)} does not match [B={B}, T, N={N}] of the loadings")
        T = panel.shape[1]
    elif T is None:
        raise ValueError("T is needed when no panel is given")
    T = int(T)
    extra, rows, shapes = fam.geom(B, T, N, r, *params)
    if T < extra[0] or rows < 1:
        raise ValueError("T must be >= p and exceed the number of idiosyncratic lags")
    ar = fam is _k._AR
    v0 = None if v0 is None else be.inp(v0)
    x = be.out(B, int(D), T, N)
    f = be.out(B, int(D), rows, r) if want_f else None
    be.sync()
    rc = getattr(ctx._lib, f"dfm_simulate{'_ar' if ar else ''}_batch{be.suffix}")(
        ctx._h, B, int(D), T, N, r, *extra, be.ptr(panel, "panel", (B, T, N)), *_k._ptrs(be, fam, params, shapes),
        *((be.ptr(v0, "v0", (B, N)),) if ar else ()), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_draw),
        be.ptr(x, "x_sim"), be.ptr(f, "f_sim"), 0)
    _k._check(ctx._h, rc)
    return dict(x=x, f=f)


def simulate_batch(ctx, Lam, R, Avar, Q, mu0, P0, D: int, T: Optional[int] = None, mask_panel=None, seed: int = 0,
                   first_draw: int = 0, want_f: bool = True):
    """dfm_simulate_batch_dev (device tensors, torch's current stream): D panels per replicate simulated from the model --
    x+ of simsmooth_batch for the same (seed, first_draw), NaN where mask_panel [B,T,N] is NaN (None: balanced, T rows).
    Returns dict(x [B,D,T,N], f [B,D,T,r] or None without want_f), resident."""
    return _simulate(ctx, _k._VARP, _k._Torch(ctx, Lam), (Lam, R, Avar, Q, mu0, P0), D, T, mask_panel, None, seed, first_draw, want_f)


def simulate_batch_host(ctx, Lam, R, Avar, Q, mu0, P0, D: int, T: Optional[int] = None, mask_panel=None, seed: int = 0,
                        first_draw: int = 0, want_f: bool = True):
    """dfm_simulate_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as simulate_batch."""
    return _simulate(ctx, _k._VARP, _k._NP, (Lam, R, Avar, Q, mu0, P0), D, T, mask_panel, None, seed, first_draw, want_f)


def simulate_ar_batch(ctx, Lam, sig2, rho, Avar, Q, mu0, P0, D: int, T: Optional[int] = None, panel=None, v0=None,
                      seed: int = 0, first_draw: int = 0, want_f: bool = True):
    """dfm_simulate_ar_batch_dev (device tensors): D panels per replicate simulated from the model with AR(q) idiosyncratic
    terms -- rows q .. T-1 are x+ of simsmooth_ar_batch_dev, NaN where `panel` [B,T,N] is NaN; rows < q are the panel's own
    (None: simulated too, T rows).  v0 [B,N] as forecast_ar_batch_dev.  Returns dict(x [B,D,T,N], f [B,D,T-q,r] or None)."""
    return _simulate(ctx, _k._AR, _k._Torch(ctx, Lam), (Lam, sig2, rho, Avar, Q, mu0, P0), D, T, panel, v0, seed, first_draw, want_f)


def simulate_ar_batch_host(ctx, Lam, sig2, rho, Avar, Q, mu0, P0, D: int, T: Optional[int] = None, panel=None, v0=None,
                           seed: int = 0, first_draw: int = 0, want_f: bool = True):
    """dfm_simulate_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as simulate_ar_batch."""
    return _simulate(ctx, _k._AR, _k._NP, (Lam, sig2, rho, Avar, Q, mu0, P0), D, T, panel, v0, seed, first_draw, want_f)


for _f in (simulate_batch, simulate_batch_host, simulate_ar_batch, simulate_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
