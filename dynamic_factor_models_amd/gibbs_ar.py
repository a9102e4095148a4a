"""Binding of the Gibbs sampler of the model with AR idiosyncratic terms (include/dfm_hip.h, csrc/gibbs_ar.hip):
dfm_gibbs_ar_batch[_dev].  The functions take a DfmContext; importing this module (kalman.py does) also attaches them to
DfmContext as gibbs_ar_batch and gibbs_ar_batch_host, on the marshalling of the `_ar` family (ks_pass_ar_batch) and with the
conventions of gibbs_batch(_host): device tensors on torch's current stream, the chain state updated in place, or NumPy through
the host-pointer entry, which updates copies.  tests/test_gibbs_ar_cpu.py drives both against a recorder in place of the library.
"""
from __future__ import annotations

from typing import Optional

from . import kalman as _k
from .gibbs import kept

STATE = ("Lam", "sig2", "rho", "Avar", "Q")
DRAWS = ("Lam", "sig2", "rho", "A", "Q", "f")
PRIOR = ("tau_lam", "nu_R", "s_R", "tau_rho", "tau_A", "nu_Q", "s_Q")


def _gibbs_ar(ctx, be, panel, params, prior, n_sweeps, burn, thin, seed, first_sweep, keep, may_have_missing, singular_q):
    panel, params, dims, n, shapes = _k._model(_k._AR, be, panel, params)
    params = [be.upd(a) for a in params[:5]] + params[5:]       # the state is written; mu0 and P0 are read only
    B, T, N, r, p, q = dims
    n_sweeps, burn, thin = int(n_sweeps), int(burn), int(thin)
    if n_sweeps < 1 or thin < 1 or burn < 0:
        raise ValueError("n_sweeps >= 1, thin >= 1 and burn >= 0 are required")
    keep = tuple(keep)
    unknown = [k for k in keep if k not in DRAWS]
    if unknown:
        raise ValueError(f"unknown draws {unknown}: choose among {DRAWS}")
    missing = [k for k in PRIOR if prior.get(k) is None]
    if missing:
        raise ValueError(f"prior entries missing: {missing}")
    flags = _k._flags(may_have_missing, singular_q, be, panel)
    K = kept(n_sweeps, burn, thin)
    per = dict(Lam=(N, r), sig2=(N,), rho=(N, q), A=(r, r * p), Q=(r, r), f=(n, r))
    draws = {k: be.out(B, K, *per[k]) if k in keep else None for k in DRAWS}
    A0 = None if prior.get("A0") is None else be.inp(prior["A0"])
    Lam, sig2, rho, Avar, Q, mu0, P0 = _k._ptrs(be, _k._AR, params, shapes)
    be.sync()
    rc = getattr(ctx._lib, "dfm_gibbs_ar_batch" + be.suffix)(
        ctx._h, B, T, N, r, p, q, be.ptr(panel, "panel"), mu0, P0, Lam, sig2, rho, Avar, Q, *[float(prior[k]) for k in PRIOR],
        be.ptr(A0, "A0", (B, r, r * p)), n_sweeps, burn, thin, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sweep),
        *[be.ptr(draws[k], k + "_draw") for k in DRAWS], flags)
    _k._check(ctx._h, rc)
    return dict(zip(STATE, params[:5])), draws


def gibbs_ar_batch(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, prior, n_sweeps: int, burn: int = 0, thin: int = 1, seed: int = 0,
                   first_sweep: int = 0, keep=("Lam", "sig2", "rho", "A", "Q"), may_have_missing: Optional[bool] = None,
                   singular_q: bool = False):
    """dfm_gibbs_ar_batch_dev (device tensors, torch's current stream): B chains, n_sweeps sweeps each.  Lam [B,N,r], sig2 [B,N],
    rho [B,N,q], Avar [B,r,r p], Q [B,r,r] are the chains' state and are updated IN PLACE; mu0 [B,r m] and P0 [B,r m,r m]
    (m = max(p, q + 1)) stay fixed.  prior: dict(tau_lam, nu_R, s_R, tau_rho, tau_A, nu_Q, s_Q[, A0 [B,r,r p]]).  keep: which of
    DRAWS are recorded for the K kept sweeps (j >= burn, (j - burn) % thin == 0).  Returns (state dict, dict(Lam [B,K,N,r],
    sig2 [B,K,N], rho [B,K,N,q], A [B,K,r,r p], Q [B,K,r,r], f [B,K,T-q,r]; None where not kept)); the status word is read by
    synchronize()."""
    return _gibbs_ar(ctx, _k._Torch(ctx, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), prior, n_sweeps, burn, thin, seed,
                     first_sweep, keep, may_have_missing, singular_q)


def gibbs_ar_batch_host(ctx, panel, Lam, sig2, rho, Avar, Q, mu0, P0, prior, n_sweeps: int, burn: int = 0, thin: int = 1,
                        seed: int = 0, first_sweep: int = 0, keep=("Lam", "sig2", "rho", "A", "Q"),
                        may_have_missing: Optional[bool] = None, singular_q: bool = False):
    """dfm_gibbs_ar_batch (host pointers; what Julia's ccall binds): NumPy in / out, the inputs are not modified; the state after
    the last sweep is the first element of the result, as gibbs_ar_batch."""
    return _gibbs_ar(ctx, _k._NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), prior, n_sweeps, burn, thin, seed, first_sweep, keep,
                     may_have_missing, singular_q)


for _f in (gibbs_ar_batch, gibbs_ar_batch_host):
    setattr(_k.DfmContext, _f.__name__, _f)
