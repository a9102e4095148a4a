"""Binding of the Gibbs sampler's entries of include/dfm_hip.h (csrc/gibbs.hip): dfm_gibbs_batch[_dev].  The functions take a
DfmContext; importing this module (kalman.py does) also attaches them to DfmContext as gibbs_batch and gibbs_batch_host, with the
marshalling conventions of simsmooth_batch(_host): device tensors on torch's current stream, the chain state updated in place,
or NumPy through the host-pointer entry, which updates copies.  tests/test_gibbs_marshalling_cpu.py drives both against a
recorder in place of the library.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k

STATE = ("Lam", "R", "Avar", "Q")
DRAWS = ("Lam", "R", "A", "Q", "f")
PRIOR = ("tau_lam", "nu_R", "s_R", "tau_A", "nu_Q", "s_Q")


def kept(n_sweeps: int, burn: int, thin: int) -> int:
    """K of the header: sweeps j = burn, burn + thin, .. below n_sweeps."""
    return (n_sweeps - burn + thin - 1) // thin if n_sweeps > burn else 0


def _gibbs(ctx, be, panel, params, prior, n_sweeps, burn, thin, seed, first_sweep, keep, may_have_missing, singular_q):
    panel, params, dims, _, shapes = _k._model(_k._VARP, be, panel, params)
    params = [be.upd(a) for a in params[:4]] + params[4:]       # the state is written; mu0 and P0 are read only
    B, T, N, r, p = dims
    n_sweeps, burn, thin = int(n_sweeps), int(burn), int(thin)
    if n_sweeps < 1 or thin < 1 or burn < 0:
        raise ValueError("n_sweeps >= 1, thin >= 1 and burn >= 0 are required")
    keep = tuple(keep)
    unknown = [n for n in keep if n not in DRAWS]
    if unknown:
        raise ValueError(f"unknown draws {unknown}: choose among {DRAWS}")
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    K = kept(n_sweeps, burn, thin)
    per = dict(Lam=(N, r), R=(N,), A=(r, r * p), Q=(r, r), f=(T, r))
    draws = {n: be.out(B, K, *per[n]) if n in keep else None for n in DRAWS}
    A0 = None if prior.get("A0") is None else be.inp(prior["A0"])
    Lam, R, Avar, Q, mu0, P0 = _k._ptrs(be, _k._VARP, params, shapes)
    be.sync()
    rc = getattr(ctx._lib, "dfm_gibbs_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, be.ptr(panel, "panel"), mu0, P0, Lam, R, Avar, Q, *[float(prior[n]) for n in PRIOR],
        be.ptr(A0, "A0", (B, r, r * p)), n_sweeps, burn, thin, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sweep),
        *[be.ptr(draws[n], n + "_draw") for n in DRAWS], flags)
    _k._check(ctx._h, rc)
    return dict(zip(STATE, params[:4])), draws


def gibbs_batch(ctx, panel, Lam, R, Avar, Q, mu0, P0, prior, n_sweeps: int, burn: int = 0, thin: int = 1, seed: int = 0,
                first_sweep: int = 0, keep=("Lam", "R", "A", "Q"), may_have_missing: Optional[bool] = None,
                singular_q: bool = False):
    """dfm_gibbs_batch_dev (device tensors, torch's current stream): B chains, n_sweeps sweeps each.  Lam [B,N,r], R [B,N],
    Avar [B,r,r p], Q [B,r,r] are the chains' state and are updated IN PLACE; mu0 [B,r p] and P0 [B,r p,r p] stay fixed.
    prior: dict(tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q[, A0 [B,r,r p]]).  keep: which of DRAWS are recorded for the K kept sweeps
    (j >= burn, (j - burn) % thin == 0).  Returns (state dict, dict(Lam [B,K,N,r], R [B,K,N], A [B,K,r,r p], Q [B,K,r,r],
    f [B,K,T,r]; None where not kept)); the status word is read by synchronize()."""
    return _gibbs(ctx, _k._Torch(ctx, panel), panel, (Lam, R, Avar, Q, mu0, P0), prior, n_sweeps, burn, thin, seed, first_sweep,
                  keep, may_have_missing, singular_q)


def gibbs_batch_host(ctx, panel, Lam, R, Avar, Q, mu0, P0, prior, n_sweeps: int, burn: int = 0, thin: int = 1, seed: int = 0,
                     first_sweep: int = 0, keep=("Lam", "R", "A", "Q"), may_have_missing: Optional[bool] = None,
                     singular_q: bool = False):
    """dfm_gibbs_batch (host pointers; what Julia's ccall binds): NumPy in / out, the inputs are not modified; the state after the
    last sweep is the first element of the result, as gibbs_batch."""
    return _gibbs(ctx, _k._NP, panel, (Lam, R, Avar, Q, mu0, P0), prior, n_sweeps, burn, thin, seed, first_sweep, keep,
                  may_have_missing, singular_q)


for _f in (gibbs_batch, gibbs_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
