"""Host-side mirror of the reference's Julia interface for the parametric path.

The reference (QuantEcon/dynamic_factor_models, dfm_functions.ipynb) is Julia; Julia is not installed in
the build image, so the layer that a Julia user would call -- `DFMModel(...)`, `estimate!(m, Parametric())`
-- is mirrored here in Python with the same names, argument meaning and error behaviour, on top of the
same C-ABI (include/dfm_hip.h) the Julia shim (julia/dfm_hip.jl) binds with `ccall`.  Index arguments
(`initperiod`, `lastperiod`) are 1-based and inclusive exactly as in the reference.

What runs where: everything O(B T N) -- PCA initialisation, Kalman filter, RTS smoother, EM -- runs in the
hand-written HIP kernels of libdfmhip.so.  The host does what the reference's Julia host code does around
its numerical kernels: slicing the estimation window, `standardize_data`, the complete-case column filter,
and copying results into the model object.  There is no CPU implementation of the hot path in this
package: without a HIP device `estimate` raises.

Reference objects mirrored (file:line of dfm_functions.ipynb):
  EstimationMethod / NonParametric / Parametric   :21-23
  VARModel                                         :43-57, ctor :424-435
  FactorEstimateStats                              :66-73
  DFMModel                                         :89-111, ctor and its three `error(...)` checks :120-146
  standardize_data                                 :501-509
  drop_missing_col                                 :167-170
  estimate!(m, ::NonParametric)                    :530-543  (the only method the reference implements;
                                                              `Parametric` is the declared-but-empty slot)
"""
from __future__ import annotations

from contextlib import contextmanager as _contextmanager     # (underscore: api's public names stay what they were)
from dataclasses import dataclass, field
from typing import Optional

import numpy as np


# ----------------------------------------------------------------------------- dispatch tags (:21-23)
class EstimationMethod:
    pass


class NonParametric(EstimationMethod):
    pass


class Parametric(EstimationMethod):
    pass


# ----------------------------------------------------------------------------- containers
@dataclass
class FactorEstimateStats:          # dfm_functions.ipynb:66-73
    T: int
    ns: int
    nobs: Optional[int] = None
    tss: Optional[float] = None
    ssr: Optional[float] = None
    R2: np.ndarray = field(default_factory=lambda: np.empty(0))


@dataclass
class VARModel:                     # dfm_functions.ipynb:43-57 (y_t = Q z_t, z_t = M z_{t-1} + G u_t, :30-34)
    y: np.ndarray
    nlag: int
    withconst: bool
    initperiod: int
    lastperiod: int
    T: int
    ns: int
    resid: np.ndarray
    betahat: np.ndarray
    M: np.ndarray
    Q: np.ndarray
    G: np.ndarray
    seps: np.ndarray


def _var_model(y: np.ndarray, nlag: int = 1, withconst: bool = True, initperiod: int = 1,
               lastperiod: Optional[int] = None) -> VARModel:
    """VARModel(y, nlag; withconst, initperiod, lastperiod) -- dfm_functions.ipynb:424-435."""
    T, ns = y.shape
    lastperiod = T if lastperiod is None else lastperiod
    k = ns * nlag
    return VARModel(y=y, nlag=nlag, withconst=withconst, initperiod=initperiod, lastperiod=lastperiod, T=T, ns=ns,
                    resid=np.full((T, ns), np.nan), betahat=np.full((k + (1 if withconst else 0), ns), np.nan),
                    M=np.zeros((k, k)), Q=np.zeros((ns, k)), G=np.zeros((k, ns)), seps=np.full((ns, ns), np.nan))


class DFMModel:
    """DFMModel(data, inclcode, nt_min_factor_estimation, nt_min_factorloading_estimation, initperiod,
    lastperiod, nfac_o, nfac_u, tol, n_uarlag, n_factorlag) -- dfm_functions.ipynb:89-146.

    `data` is T x ns with NaN for the reference's `missing`.  `factor` and `factor_var_model.y` alias the
    same array, as in the reference (:80, :138).  The reference's field `lambda` is `lambda_` here."""

    def __init__(self, data, inclcode, nt_min_factor_estimation: int, nt_min_factorloading_estimation: int,
                 initperiod: int, lastperiod: int, nfac_o: int, nfac_u: int, tol: float, n_uarlag: int,
                 n_factorlag: int):
        data = np.asarray(data, dtype=np.float64)
        inclcode = np.asarray(inclcode).astype(int).ravel()
        if data.ndim != 2 or data.shape[1] != inclcode.shape[0]:
            raise ValueError("length of inclcode must equal to number of data series")          # :124
        if not (initperiod < lastperiod):
            raise ValueError("initperiod must be smaller than lastperiod")                      # :125
        if not (n_uarlag > 0 and n_factorlag > 0):
            raise ValueError("n_uarlag and n_factorlag must be positive")                       # :126
        T, ns = data.shape
        if not (1 <= initperiod and lastperiod <= T):
            raise ValueError("estimation window must lie inside the data (1 <= initperiod, lastperiod <= T)")
        self.data = data
        self.inclcode = inclcode
        self.T, self.ns = T, ns
        self.nt_min_factor_estimation = int(nt_min_factor_estimation)
        self.nt_min_factorloading_estimation = int(nt_min_factorloading_estimation)
        self.initperiod, self.lastperiod = int(initperiod), int(lastperiod)
        self.nfac_o, self.nfac_u = int(nfac_o), int(nfac_u)
        self.nfac_t = self.nfac_o + self.nfac_u
        self.tol = float(tol)
        n_incl = int(np.count_nonzero(inclcode == 1))
        self.fes = FactorEstimateStats(self.lastperiod - self.initperiod + 1, n_incl, None, None, None,
                                       np.full(n_incl, np.nan))
        self.factor = np.full((T, self.nfac_t), np.nan)
        self.lambda_ = np.full((ns, self.nfac_t), np.nan)
        self.uar_coef = np.full((ns, n_uarlag), np.nan)
        self.uar_ser = np.full(ns, np.nan)
        self.n_uarlag, self.n_factorlag = int(n_uarlag), int(n_factorlag)
        self.factor_var_model = _var_model(self.factor, self.n_factorlag, True, self.initperiod, self.lastperiod)
        self.r2 = np.full(ns, np.nan)
        # results of the parametric path that have no field in the reference struct
        self.loglik_path: Optional[np.ndarray] = None
        self.em_iters: Optional[int] = None
        self.em_params: Optional[dict] = None


# ----------------------------------------------------------------------------- host helpers
def standardize_data(x: np.ndarray):
    """dfm_functions.ipynb:501-509: per-series mean and *population* s.d. over the observed cells;
    returns ((x - mean) / sd, sd [1 x ns])."""
    x = np.asarray(x, dtype=np.float64)
    n = np.count_nonzero(~np.isnan(x), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):      # a column without observations stays all-NaN
        mu = np.nansum(x, axis=0) / n
        d = np.where(np.isnan(x), 0.0, x - mu)
        sd = np.sqrt((d * d).sum(axis=0) / n)
        return (x - mu) / sd, sd[None, :]


def drop_missing_col(A: np.ndarray):
    """dfm_functions.ipynb:167-170: keep the columns with no missing cell; returns (sub-matrix, mask)."""
    keep = ~np.isnan(A).any(axis=0)
    return A[:, keep], keep


# ----------------------------------------------------------------------------- estimate!(m, ::Parametric)
def estimate(m: DFMModel, method: EstimationMethod = None, *, max_em_iter: int = 50, tol_em: float = 1e-6,
             factor_lags: Optional[int] = None, ctx=None, lam_constr_f=None, lam_constr_fl=None,
             nrep: int = 0, seed: int = 20160415, ngpu: int = 1, draws: Optional[str] = None):
    """`estimate!(m::DFMModel, ::Parametric; max_em_iter, tol_em)`: PCA-initialised EM for the exact
    Gaussian state-space DFM  x_t = Lam f_t + e_t,  f_t = A f_{t-1} + eta_t  on the standardised
    estimation window (rows initperiod..lastperiod, series with inclcode == 1), fitted with the HIP
    library.  Mutates `m` in place like the reference's `estimate!` and returns the per-iteration
    log-likelihood vector (the reference's own methods return `nothing`).

      m.factor[initperiod:lastperiod, :]  <- smoothed factors E[f_t | X]
      m.lambda_[incl, :]                  <- loadings in data units (Lam_i * sd_i)
      m.uar_ser[incl]                     <- idiosyncratic s.d. in data units; m.uar_coef[incl, :] = 0
      m.factor_var_model.M / G / seps     <- A (companion block), chol(Q) lower, Q      (cf. :477-492)
      m.fes.tss / nobs / ssr / R2         <- as estimate_factor! defines them (:342-343, :366, :372-380),
                                             with the common component Lam f_t|T in place of the ALS fit
    `factor_lags` = p of the factor VAR, f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t; default: the model's own
    `n_factorlag` (dfm_functions.ipynb:120-146), run in the companion form `fill_matrices!` builds (:477-492)
    through dfm_em_varp_batch (r p <= 32); then M, G, seps, betahat hold [A_1 .. A_p], chol(Q), Q.
    `nrep` > 0 (`estimate!(m, ::Parametric; ..., nrep, seed, ngpu)`): after the point estimate, `nrep`
    parametric-bootstrap replicates of the standardised window are drawn from the fitted model (the window's own missing
    pattern; NumPy generator seeded with `seed`) and re-estimated by EM in ONE batched call on `ngpu` GPUs of this node
    (dfm_em_batch_multi: replicates sharded over the GPUs, one RCCL all-gather of {loglik, active} per EM iteration);
    the replicate estimates land in `m.replicates`.  That host generator serves factor_lags = 1 and is the default there.
    `draws="device"` (the default, and the only way, for factor_lags > 1): the panels are drawn on the device from the point
    estimate by dfm_simulate_batch (the random stream of dfm_simsmooth_batch, key `seed`, draw b = replicate b; the window's NaN
    pattern) and re-estimated from the point estimate where they lie, in one dfm_em_varp_batch_dev call (dfm_em_batch_dev at
    factor_lags = 1) on one GPU; a fit that needed the covariance-form recursion re-estimates in it too.  `m.replicates` has the
    same keys either way; with factor_lags > 1 params["A"] = params["Avar"] = [A_1 .. A_p], which is what every band-producing
    function reads.
    `NonParametric()` runs the reference's own estimator (ALS, loadings, VAR) on the HIP kernels of als.hip:
    see estimate_nonparametric below."""
    method = Parametric() if method is None else method
    if isinstance(method, NonParametric):
        return estimate_nonparametric(m, ctx=ctx, lam_constr_f=lam_constr_f, lam_constr_fl=lam_constr_fl)
    if not isinstance(method, Parametric):
        raise TypeError("method must be Parametric() or NonParametric()")
    if lam_constr_f is not None or lam_constr_fl is not None:
        raise NotImplementedError("loading constraints are not supported on the parametric path")
    if m.nfac_o != 0:
        if nrep:
            raise ValueError("bootstrap replicates (nrep > 0) are not available with observed factors")
        return _estimate_parametric_observed(m, max_em_iter, tol_em, ctx)
    r = m.nfac_u
    nlag = m.n_factorlag if factor_lags is None else int(factor_lags)
    if nlag < 1 or r * nlag > 32:
        raise ValueError("need 1 <= factor_lags and nfac_u * factor_lags <= 32 (DFM_MAX_R)")
    if draws not in (None, "host", "device"):
        raise ValueError('draws must be "host", "device" or None (host at factor_lags = 1, device beyond)')
    dev_draws = draws == "device" or (draws is None and nlag > 1)
    if nrep and nlag > 1 and not dev_draws:
        raise ValueError('the host generator of bootstrap panels serves factor_lags = 1 only: draws="device"')
    if nrep and nlag > 1 and int(ngpu) > 1:
        raise ValueError("bootstrap replicates with factor_lags > 1 run on one GPU (there is no multi-GPU VAR(p) EM): ngpu = 1")
    if nrep and dev_draws and int(ngpu) > 1:
        raise ValueError('draws="device" re-estimates the replicates on one GPU: ngpu = 1')
    incl = m.inclcode == 1
    xdata = m.data[m.initperiod - 1:m.lastperiod, :][:, incl]           # :335-336
    z, sd = standardize_data(xdata)                                     # :339
    obs = ~np.isnan(z)
    m.fes.tss = float(np.nansum(z * z))                                 # :342
    m.fes.nobs = int(obs.sum())                                         # :343
    enough = obs.sum(axis=0) >= m.nt_min_factor_estimation              # :357 (series too short are left out)
    if not enough.all():
        z = z[:, enough]
    xbal, balmask = drop_missing_col(z)                                 # :345
    T, N = z.shape
    if xbal.shape[1] < r:
        raise ValueError("fewer fully observed series than factors: cannot initialise by PCA")

    own_ctx = ctx is None
    with _device(ctx) as ctx:                                           # raises without a HIP device
        p0, F0 = ctx.pca_init_batch_host(xbal[None, :, :], r)          # pca_score (:179-183) + OLS start, on the GPU
        F0 = F0[0]
        Lam = np.empty((N, r)); R = np.empty(N)
        Lam[balmask] = p0["Lam"][0]; R[balmask] = p0["R"][0]
        gap = np.nonzero(~balmask)[0]
        if gap.size:                                                    # series with gaps: complete-case OLS on F0, no
            o = ctx.ols_batch_host(F0, z[:, gap], want_resid=False)     # intercept (`ols_skipmissing`, :242-252): dfm_ols_batch
            Lam[gap] = o["beta"]
            R[gap] = o["ssr"] / np.maximum(o["nobs"], 1)
        if nlag == 1:
            start = dict(Lam=Lam[None], R=R[None], A=p0["A"], Q=p0["Q"], mu0=p0["mu0"], P0=p0["P0"])
            args = (z[None], start["Lam"], start["R"], start["A"], start["Q"], start["mu0"], start["P0"])
            kw = dict(max_iter=max_em_iter, tol=tol_em, may_have_missing=bool((~obs).any()))
            # the information-form recursion inverts Q: a PCA start on fewer than 2r + 1 periods has a rank-deficient
            # VAR residual covariance.  Run the covariance-form recursion (DFM_F_SINGULAR_Q) instead of failing.
            (params, path, iters, f, P), used_singular_q = _numeric_retry(lambda **sq: (ctx.em_batch_host(*args, **sq, **kw), bool(sq)))
        else:
            # VAR(p) start (oracle/varp_oracle.py varp_init): OLS of the PCA factors on their p lags without constant
            # (dfm_ols_batch), Q = residual covariance / (T - p), z_0 ~ N(0, second moment of the stacked lags)
            if T - nlag <= r * nlag:
                raise ValueError("too few periods for a VAR(factor_lags) start")
            Z = np.hstack([F0[nlag - 1 - l:T - l] for l in range(nlag)])
            o = ctx.ols_batch_host(Z[:-1], F0[nlag:], want_resid=True)  # one regression per factor
            Avar = o["beta"].copy()                                     # [A_1 .. A_p]  (r, r p)
            e = o["resid"]
            Qv = e.T @ e / (T - nlag); Qv = 0.5 * (Qv + Qv.T)
            P0v = Z.T @ Z / Z.shape[0]; P0v = 0.5 * (P0v + P0v.T)
            vargs = (z[None], Lam[None], R[None], Avar[None], Qv[None], np.zeros((1, r * nlag)), P0v[None])
            vkw = dict(max_iter=max_em_iter, tol=tol_em, may_have_missing=bool((~obs).any()))
            # r = 4: recursion_comp.hip inverts the r x r block Q (as above)
            (params, path, iters, f, P), used_singular_q = _numeric_retry(lambda **sq: (ctx.em_varp_batch_host(*vargs, **sq, **vkw), bool(sq)))
            params = dict(params)
            params["A"] = params["Avar"]
    k = int(iters[0])
    f = f[0]
    Lam, R, A, Q = params["Lam"][0], params["R"][0], params["A"][0], params["Q"][0]
    m.loglik_path = path[0, :k].copy()
    m.em_iters = k
    m.em_params = {kk: v[0].copy() for kk, v in params.items()}
    m.factor[m.initperiod - 1:m.lastperiod, :] = f                      # in place: aliases factor_var_model.y (:371, :80)
    cols = np.nonzero(incl)[0][enough] if not enough.all() else np.nonzero(incl)[0]
    sdv = sd[0][enough] if not enough.all() else sd[0]
    m.lambda_[cols, :] = Lam * sdv[:, None]
    m.uar_ser[cols] = np.sqrt(R) * sdv
    m.uar_coef[cols, :] = 0.0
    common = f @ Lam.T
    e = np.where(np.isnan(z), 0.0, z - common)
    m.fes.ssr = float((e * e).sum())                                    # :366
    zc = z - np.nanmean(z, axis=0)
    R2 = 1.0 - (e * e).sum(axis=0) / np.nansum(zc * zc, axis=0)         # compute_r2 (:565-569)
    m.fes.R2 = np.full(m.fes.ns, np.nan)
    m.fes.R2[np.nonzero(enough)[0]] = R2
    m.r2[cols] = R2
    var = m.factor_var_model                                            # fill_matrices! (:477-492) for VAR(1)
    var.M[:] = 0.0; var.Q[:] = 0.0; var.G[:] = 0.0
    ka = min(A.shape[1], var.M.shape[1])                                # [A_1 .. A_p] into the model's companion (:484-486)
    var.M[:r, :ka] = A[:, :ka]
    if var.nlag > 1:
        var.M[r:, :-r] = np.eye(r * (var.nlag - 1))
    var.Q[:, :r] = np.eye(r)
    var.seps[:] = Q
    var.G[:r, :r] = _psd_sqrt(Q)            # lower Cholesky factor (:489); a rank-deficient Q has only a symmetric root
    var.betahat[:] = 0.0
    c0 = 1 if var.withconst else 0
    var.betahat[c0:c0 + ka, :] = A[:, :ka].T
    if nrep and dev_draws:
        with _device(None if own_ctx else ctx) as c:
            m.replicates = _bootstrap_replicates_device(c, z, params, nlag, int(nrep), int(seed), max_em_iter, tol_em, used_singular_q)
    elif nrep:
        m.replicates = _bootstrap_replicates(z, params, int(nrep), int(seed), int(ngpu), max_em_iter, tol_em,
                                             singular_q=used_singular_q)
    return m.loglik_path


def _estimate_parametric_observed(m: DFMModel, max_em_iter, tol_em, ctx):
    """`estimate(m, Parametric())` with OBSERVED factors (nfac_o > 0).  The reference's estimator is
    non-functional there (dfm_functions.ipynb:358-359, :371; App. D 7), so the semantics are those its data layout implies
    (include/dfm_hip.h, oracle/obs_oracle.py): the caller has put the observed factors g_t into the FIRST nfac_o columns of
    `m.factor` (rows initperiod..lastperiod, no gaps); they enter the measurement equation as known regressors,
        x_it = lam_o,i' g_t + lam_u,i' f_t + e_it,
    and only f_t (nfac_u columns, VAR(1)) is latent.  Start: per-series OLS on g (dfm_ols_batch), PCA + OLS start of the
    residual panel (dfm_pca_init_batch); EM: dfm_em_obs_batch.  Afterwards `m.factor[:, nfac_o:]` holds E[f_t | X],
    `m.lambda_` the nfac_t loadings in data units, and the factor VAR of ALL nfac_t factors -- the reference's own second
    stage -- is `estimate_var(m.factor_var_model)` (dfm_functions.ipynb:444-492), run here on the GPU as well."""
    ro, ru = m.nfac_o, m.nfac_u
    incl = m.inclcode == 1
    w0, w1 = m.initperiod - 1, m.lastperiod
    G = np.array(m.factor[w0:w1, :ro], float)
    if np.isnan(G).any():
        raise ValueError("observed factors: fill m.factor[initperiod:lastperiod, :nfac_o] (no gaps) before estimate()")
    z, sd = standardize_data(m.data[w0:w1, :][:, incl])                 # :335-339
    obs = ~np.isnan(z)
    m.fes.tss = float(np.nansum(z * z)); m.fes.nobs = int(obs.sum())    # :342-343
    enough = obs.sum(axis=0) >= m.nt_min_factor_estimation              # :357
    if not enough.all():
        z = z[:, enough]
    T, N = z.shape
    with _device(ctx) as ctx:
        og = ctx.ols_batch_host(G, z, want_resid=True)                  # series on the observed factors, complete cases
        Lam_o = og["beta"]
        res = og["resid"]                                               # [T, N], NaN where the cell is missing
        rbal, balmask = drop_missing_col(res)
        if rbal.shape[1] < ru:
            raise ValueError("fewer fully observed series than unobserved factors: cannot initialise by PCA")
        p0, F0 = ctx.pca_init_batch_host(rbal[None, :, :], ru)
        F0 = F0[0]
        Lam_u = np.empty((N, ru)); R = np.empty(N)
        Lam_u[balmask] = p0["Lam"][0]; R[balmask] = p0["R"][0]
        gap = np.nonzero(~balmask)[0]
        if gap.size:
            o = ctx.ols_batch_host(F0, res[:, gap], want_resid=False)
            Lam_u[gap] = o["beta"]; R[gap] = o["ssr"] / np.maximum(o["nobs"], 1)
        Lam = np.hstack([Lam_o, Lam_u])
        params, path, iters, f, P = ctx.em_obs_batch_host(z[None], G[None], Lam[None], R[None], p0["A"], p0["Q"], p0["mu0"], p0["P0"],
                                                          max_iter=max_em_iter, tol=tol_em, may_have_missing=bool((~obs).any()))
        k = int(iters[0]); f = f[0]
        Lam, R = params["Lam"][0], params["R"][0]
        m.loglik_path = path[0, :k].copy(); m.em_iters = k
        m.em_params = {kk: v[0].copy() for kk, v in params.items()}
        m.factor[w0:w1, ro:] = f                                        # in place (aliases factor_var_model.y, :80)
        cols = np.nonzero(incl)[0][enough] if not enough.all() else np.nonzero(incl)[0]
        sdv = sd[0][enough] if not enough.all() else sd[0]
        m.lambda_[cols, :] = Lam * sdv[:, None]
        m.uar_ser[cols] = np.sqrt(R) * sdv
        m.uar_coef[cols, :] = 0.0
        e = np.where(np.isnan(z), 0.0, z - np.hstack([G, f]) @ Lam.T)
        m.fes.ssr = float((e * e).sum())
        zc = z - np.nanmean(z, axis=0)
        R2 = 1.0 - (e * e).sum(axis=0) / np.nansum(zc * zc, axis=0)
        m.fes.R2 = np.full(m.fes.ns, np.nan); m.fes.R2[np.nonzero(enough)[0]] = R2
        m.r2[cols] = R2
        estimate_var(m.factor_var_model, ctx=ctx)                       # VAR of (g, f) jointly: the reference's second stage
    return m.loglik_path


def _psd_sqrt(S):
    """A square root L (L L' = S) of a symmetric positive SEMI-definite matrix: Cholesky when it exists, else the symmetric
    eigen square root (a fit that needed the covariance-form recursion has a rank-deficient Q)."""
    S = 0.5 * (S + S.T)
    try:
        return np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        w, V = np.linalg.eigh(S)
        return (V * np.sqrt(np.maximum(w, 0.0))) @ V.T


def _bootstrap_replicates(z, params, nrep, seed, ngpu, max_em_iter, tol_em, singular_q=False):
    """`nrep` parametric-bootstrap panels from the fitted model on the standardised window z (NaN where z is NaN),
    re-estimated from the point estimate in one dfm_em_batch_multi call (julia/dfm_hip.jl estimate!: same steps)."""
    from .kalman import DfmContext
    Lam, R, A, Q, mu0, P0 = (params[k][0] for k in ("Lam", "R", "A", "Q", "mu0", "P0"))
    T, N = z.shape
    r = Lam.shape[1]
    rng = np.random.default_rng(seed)
    LQ = _psd_sqrt(Q)                      # (never raises after the point estimate has been written into the model)
    LS = _psd_sqrt(P0)
    sq = np.sqrt(R)
    panels = np.empty((nrep, T, N))
    for b in range(nrep):
        f = mu0 + LS @ rng.standard_normal(r)
        for t in range(T):
            f = A @ f + LQ @ rng.standard_normal(r)
            panels[b, t] = Lam @ f + sq * rng.standard_normal(N)
    panels[:, np.isnan(z)] = np.nan
    rep = lambda a: np.repeat(a[None], nrep, axis=0)
    new, path, iters, _, _, ran = DfmContext.em_batch_multi_host(ngpu, panels, rep(Lam), rep(R), rep(A), rep(Q), rep(mu0),
                                                                 rep(P0), max_iter=max_em_iter, tol=tol_em,
                                                                 singular_q=singular_q)
    return dict(params=new, loglik_path=path, iters=iters, iterations=ran, panels=panels)


def _em_resident(em, panels, start, names, nrep, max_em_iter, tol_em, singular_q, sync, **kw):
    """One EM call on resident panels [nrep, T, N], every replicate started from `start` (name -> device tensor [1, ...]): the
    updated parameters, log-likelihood paths and iteration counts on the host.  The device entries only enqueue, so a replicate
    whose first log-likelihood is not finite is what the host entries report as DFM_E_NUMERIC: like the point estimate, the call
    is then run once more in covariance form."""
    for sq in ((True,) if singular_q else (False, True)):
        P = [start[k].expand(nrep, *start[k].shape[1:]).contiguous() for k in names]
        path, iters = em(panels, *P, max_iter=max_em_iter, tol=tol_em, singular_q=sq, **kw)[:2]
        sync()
        path, iters = path.cpu().numpy(), iters.cpu().numpy()
        if np.isfinite(path[:, 0]).all():
            break
    else:
        from ._lib import DfmError
        raise DfmError(-5, "bootstrap replicates: non-finite log-likelihood (Q or P0 not positive definite?)")
    return {k: a.cpu().numpy() for k, a in zip(names, P)}, path, iters


def _bootstrap_replicates_device(ctx, z, params, nlag, nrep, seed, max_em_iter, tol_em, singular_q=False):
    """`nrep` parametric-bootstrap panels drawn on the device from the fitted model on the standardised window z (NaN where z is
    NaN: dfm_simulate_batch, replicate b = draw b of seed `seed`), re-estimated from the point estimate where they lie
    (dfm_em_varp_batch_dev; dfm_em_batch_dev at factor_lags = 1).  The keys of _bootstrap_replicates."""
    torch = ctx._torch
    names = ("Lam", "R", "A" if nlag == 1 else "Avar", "Q", "mu0", "P0")
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=f"cuda:{ctx.device}")
    start = {k: dev(params[k][:1]) for k in names}
    miss = bool(np.isnan(z).any())
    sim = ctx.simulate_batch(*(start[k] for k in names), D=nrep, T=z.shape[0], mask_panel=dev(z[None]) if miss else None,
                             seed=seed, want_f=False)
    panels = sim["x"][0]
    em = ctx.em_batch if nlag == 1 else ctx.em_varp_batch
    new, path, iters = _em_resident(em, panels, start, names, nrep, max_em_iter, tol_em, singular_q, ctx.synchronize,
                                    may_have_missing=miss)
    if nlag > 1:
        new["A"] = new["Avar"]
    return dict(params=new, loglik_path=path, iters=iters, iterations=int(iters.max()), panels=panels.cpu().numpy())


# ----------------------------------------------------------------------------- nowcasts and forecasts of the panel
def _forecast_inputs(m: DFMModel, through: int):
    """The series `estimate` used (inclcode == 1 and the `enough` rule), the estimation window's mean and population s.d.
    (standardize_data, dfm_functions.ipynb:501-509), and rows initperiod..through standardised with them."""
    incl = m.inclcode == 1
    xwin = m.data[m.initperiod - 1:m.lastperiod, :][:, incl]
    n = np.count_nonzero(~np.isnan(xwin), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.nansum(xwin, axis=0) / n
    z, sd = standardize_data(xwin)
    enough = (~np.isnan(z)).sum(axis=0) >= m.nt_min_factor_estimation
    cols = np.nonzero(incl)[0][enough]
    mu, sd = mu[enough], sd[0][enough]
    x = m.data[m.initperiod - 1:through, :][:, cols]
    return cols, (x - mu) / sd, mu, sd


# ----------------------------------------------------------------------------- what the post-estimation calls share
# One text for what the functions of the parametric fit and their _ar_idio counterparts have in common (docs/HISTORY.md A.17,
# with the list of the differences between them that were kept as they were).
def _own(ctx):
    if ctx is not None:
        return ctx, False
    from .kalman import DfmContext
    return DfmContext(), True                                           # raises without a HIP device


@_contextmanager
def _device(ctx):
    """The context a function works on: `ctx` itself, which stays open, or with None a new one (_own), which is closed on the way
    out, also when the body raises."""
    ctx, own = _own(ctx)
    try:
        yield ctx
    finally:
        if own:
            ctx.close()


def _numeric_retry(call, unless=None):
    """The information form inverts Q, so a numeric failure (DfmError code -5) of call() is answered once with
    call(singular_q=True), the covariance form -- unless `unless(err)` says that this failure is not one that form can cure."""
    from ._lib import DfmError
    try:
        return call()
    except DfmError as err:
        if err.code != -5 or (unless is not None and unless(err)):
            raise
        return call(singular_q=True)


def _quantile_arg(quantiles, *needs, closed=False):
    """`quantiles` as a float64 vector (None stays None), each in (0, 1] -- `closed`: in [0, 1] -- or ValueError.  `needs`:
    (broken, message) pairs, the refusals a function has between reading the vector and checking its range (no replicates, no
    horizon); the first broken one is raised."""
    if quantiles is None:
        return None
    qs = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    for broken, message in needs:
        if broken:
            raise ValueError(message)
    if closed:
        if qs.size == 0 or np.any(~(qs >= 0.0)) or np.any(~(qs <= 1.0)):
            raise ValueError("quantiles must lie in [0, 1]")
    elif qs.size < 1 or not np.all((qs > 0.0) & (qs <= 1.0)):
        raise ValueError("quantiles must lie in (0, 1]")
    return qs


_NEED_REPLICATES = "quantile bands need bootstrap replicates: estimate(m, Parametric(), nrep=...) first"


def _need_fit(m: DFMModel):
    """Refuses a model without a parametric fit."""
    if m.em_params is None:
        raise ValueError("the model has not been estimated: run estimate(m, Parametric()) first")


def _through_arg(m: DFMModel, through):
    """`through` (None: lastperiod) as a 1-based period in lastperiod..T, or ValueError."""
    through = m.lastperiod if through is None else int(through)
    if not (m.lastperiod <= through <= m.T):
        raise ValueError(f"through must lie in lastperiod..T ({m.lastperiod}..{m.T})")
    return through


def _no_ar_terms(m: DFMModel, cols, who, hint):
    """Refuses, in the name of function `who`, a model whose series carry AR idiosyncratic coefficients; `hint`: where to go."""
    if np.any(np.nan_to_num(np.asarray(m.uar_coef, dtype=np.float64)[cols]) != 0.0):
        raise ValueError(f"{who} has no AR idiosyncratic terms: the model carries uar_coef {hint}")


def _plain_fit(m: DFMModel, through, who=None, hint=""):
    """What a function of the parametric fit starts from: the parameters in m.em_params as (Lam, R, A, Q, mu0, P0) -- A is
    [A_1 .. A_p], under whichever key estimate() left it -- and _forecast_inputs(m, through): cols, z, mu, sd.  Refuses a model
    whose series no longer match the fit and, with `who`, one with AR idiosyncratic terms (_no_ar_terms)."""
    ep = m.em_params
    prm = (ep["Lam"], ep["R"], ep["Avar"] if "Avar" in ep else ep["A"], ep["Q"], ep["mu0"], ep["P0"])
    cols, z, mu, sd = _forecast_inputs(m, through)
    if prm[0].shape[0] != cols.size:
        raise ValueError("m.em_params does not match the model's series (was the model changed after estimate?)")
    if who is not None:
        _no_ar_terms(m, cols, who, hint)
    return prm, cols, z, mu, sd


def _replicate_sets(m: DFMModel):
    """The bootstrap replicates' (or posterior draws') parameter sets in the order of _plain_fit, [B, ...] each."""
    rp = m.replicates["params"]
    return rp["Lam"], rp["R"], rp["A"], rp["Q"], rp["mu0"], rp["P0"]


def _rep(a, B):
    """`a` for each of B replicates: [B, ...], C-ordered."""
    return np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))


def _one(prm):
    """One parameter set as a batch of one."""
    return tuple(a[None] for a in prm)


def _unpack(Pp, k):
    """[rows, k (k + 1) / 2] packed lower triangles as full symmetric [rows, k, k]."""
    il = np.tril_indices(k)                                             # packed lower, row-major (include/dfm_hip.h)
    cov = np.empty((Pp.shape[0], k, k))
    cov[:, il[0], il[1]] = Pp
    cov[:, il[1], il[0]] = Pp
    return cov


def _horizon_bands(ctx, ob, H, qs):
    """Bands [nq, H, cols] over the horizon rows of the replicates' point forecasts (dfm_quantile_bands)."""
    return ctx.quantile_bands_host(ob["xhat"][:, -H:, :], qs)


def _with_bands(out, qs, **bands):
    """`out` with the quantiles and the band arrays behind them -- when bands were asked for."""
    if qs is not None:
        out["quantiles"] = qs
        out.update(bands)
    return out


def forecast(m: DFMModel, H: int, *, through: Optional[int] = None, quantiles=None, ctx=None) -> dict:
    """Nowcasts and H-step forecasts of the panel from the parametric fit (`estimate(m, Parametric())`, nfac_o = 0).

    Parameters come from the estimation window (m.em_params; its series and its mean / population s.d.); the state conditions
    on rows initperiod..`through` (1-based, lastperiod <= through <= m.T, default lastperiod), standardised with the window's
    mean and s.d. -- rows after lastperiod are the ragged edge a nowcast is for.  One dfm_forecast_batch call on the GPU.
    Returns a dict (data units unless noted):
      rows        1-based periods initperiod .. through + H (the last H are the forecast horizon)
      cols        column indices (0-based) of m.data: the series estimate() used
      x           [rows, cols] observed cells as they are, every other cell E[x_ti | X]
      x_sd        [rows, cols] s.d. of x given X: 0 on observed cells, sd_i sqrt(lam_i' P_t lam_i + R_i) elsewhere
      common      [rows, cols] mean_i + sd_i lam_i' E[f_t | X]
      factor      [rows, r] E[f_t | X] (the model's standardised factor units), factor_cov [rows, r, r] = Var[f_t | X]
      loglik      log-likelihood of the observed cells of rows initperiod..through at the fitted parameters
    `quantiles` (needs m.replicates from estimate(..., nrep=...)): every replicate's parameter set runs in ONE batched call on
    the same panel, and dfm_quantile_bands over the replicates' horizon rows gives bands [nq, H, len(cols)] (nearest rank).
    These bands are the PARAMETER uncertainty of the point forecast only; x_sd carries the shock part.  `m` is not modified."""
    H = int(H)
    if H < 0:
        raise ValueError("H must be >= 0")
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("forecast needs nfac_o = 0 (the future values of observed factors are unknown)")
    through = _through_arg(m, through)
    qs = _quantile_arg(quantiles, (getattr(m, "replicates", None) is None, _NEED_REPLICATES), (H < 1, "quantile bands need H >= 1"))
    prm, cols, z, mu, sd = _plain_fit(m, through)
    with _device(ctx) as ctx:
        def run(sets, **kw):                        # the information form inverts Q: as estimate(), retry in covariance form
            B = sets[0].shape[0]
            kw.update(mean=_rep(mu, B), sd=_rep(sd, B), may_have_missing=bool(np.isnan(z).any()))
            return _numeric_retry(lambda **sq: ctx.forecast_batch_host(_rep(z, B), *sets, H, **sq, **kw))
        o = run(_one(prm))
        bands = None
        if qs is not None:
            bands = _horizon_bands(ctx, run(_replicate_sets(m), want_var=False, want_common=False, want_P=False), H, qs)
    out = dict(rows=np.arange(m.initperiod, through + H + 1), cols=cols, x=o["xhat"][0], x_sd=np.sqrt(o["xvar"][0]),
               common=o["common"][0], factor=o["f"][0], factor_cov=_unpack(o["P"][0], prm[0].shape[1]),
               loglik=float(o["loglik"][0]))
    return _with_bands(out, qs, bands=bands)


# ----------------------------------------------------------------------------- filtered states and out-of-sample evaluation
def _filter_setup(m: DFMModel, through, quantiles):
    """The checks filter_states and evaluate_forecasts share (no device is touched): (through, quantiles or None)."""
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("the filter needs nfac_o = 0")
    through = _through_arg(m, through)
    return through, _quantile_arg(quantiles, (getattr(m, "replicates", None) is None, _NEED_REPLICATES))


def _flat_bands(ctx, x, qs):
    """Bands [nq, ...] of x [B, ...] over its first axis (dfm_quantile_bands takes the cells as one axis)."""
    return ctx.quantile_bands_host(np.ascontiguousarray(x.reshape(x.shape[0], -1)), qs).reshape((qs.size,) + x.shape[1:])


def _filter_run(m: DFMModel, through, H, t0, want, band_of, qs, ctx):
    """One dfm_filter_batch call at the fit and, for bands, one over the bootstrap replicates' parameter sets on the same panel
    followed by dfm_quantile_bands over band_of(outputs) [B, ...]."""
    prm, cols, z, mu, sd = _plain_fit(m, through)
    with _device(ctx) as ctx:
        def run(sets, w):
            B = sets[0].shape[0]
            return ctx.filter_batch_host(_rep(z, B), *sets, H=H, t0=t0, mean=_rep(mu, B), sd=_rep(sd, B), want=w,
                                         may_have_missing=bool(np.isnan(z).any()))
        o = run(_one(prm), want)
        bands = None if qs is None else _flat_bands(ctx, band_of(run(_replicate_sets(m), band_of.want)), qs)
    return cols, o, bands


def filter_states(m: DFMModel, *, through: Optional[int] = None, quantiles=None, ctx=None) -> dict:
    """What the parametric fit (`estimate(m, Parametric())`, nfac_o = 0) knew at every period: the Kalman filter's predicted and
    filtered factors and the one-step prediction errors of the panel.  The parameters (m.em_params) are held fixed over the sample.
    Window, series, standardisation and `through` as `forecast`.  One dfm_filter_batch call on the GPU.  Returns a dict:
      rows            1-based periods initperiod .. through
      cols            column indices (0-based) of m.data: the series estimate() used
      factor_pred     [rows, r] E[f_t | rows before t], factor_pred_cov [rows, r, r] its variance
      factor_filt     [rows, r] E[f_t | rows up to t],  factor_filt_cov [rows, r, r]
      state_pred, state_filt   [rows, r p] the whole companion state (equal to the factors for factor_lags = 1)
      loglik_t        [rows] log density of each row's observed cells given the rows before it; loglik their sum
      x_pred          [rows, cols] one-step prediction of every cell, data units
      error           [rows, cols] x - x_pred in data units, NaN on a missing cell
      error_std       [rows, cols] the standardised innovation (mean 0, variance 1 under the model), NaN on a missing cell
    `quantiles` (needs m.replicates): bands [nq, rows, cols] of x_pred over the bootstrap replicates' parameter sets
    (dfm_quantile_bands).  `m` is not modified."""
    through, qs = _filter_setup(m, through, quantiles)
    band_of = lambda o: o["xpred"]
    band_of.want = ("xpred",)
    want = ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t", "xpred", "verr", "vstd")
    cols, o, bands = _filter_run(m, through, 0, 0, want, band_of, qs, ctx)
    r = m.em_params["Lam"].shape[1]
    k = o["z_pred"].shape[2]
    Pp, Pf = _unpack(o["P_pred"][0], k), _unpack(o["P_filt"][0], k)
    out = dict(rows=np.arange(m.initperiod, through + 1), cols=cols, factor_pred=o["z_pred"][0][:, :r],
               factor_pred_cov=Pp[:, :r, :r], factor_filt=o["z_filt"][0][:, :r], factor_filt_cov=Pf[:, :r, :r],
               state_pred=o["z_pred"][0], state_filt=o["z_filt"][0], loglik_t=o["loglik_t"][0],
               loglik=float(o["loglik_t"][0].sum()), x_pred=o["xpred"][0], error=o["verr"][0], error_std=o["vstd"][0])
    return _with_bands(out, qs, bands=bands)


def evaluate_forecasts(m: DFMModel, H: int, *, first_origin: Optional[int] = None, through: Optional[int] = None, quantiles=None,
                       ctx=None) -> dict:
    """The pseudo-out-of-sample record of the parametric fit: the h-step forecast error of every series at every origin, h = 1..H,
    with the fit held fixed (the data flow is evaluated, not re-estimation), summarised per horizon and series.  Origins are the
    1-based periods first_origin .. through - h (default first_origin: the middle of the window initperiod..through); the
    forecast made at origin t uses rows initperiod..t only.  One dfm_filter_batch call on the GPU.  Returns a dict:
      horizons   1 .. H
      cols       column indices (0-based) of m.data: the series estimate() used
      msfe       [H, cols] mean squared forecast error in data units, NaN where no origin has its target observed
      rmsfe      its square root
      relative   [H, cols] msfe over the MSFE of the unconditional-mean forecast on the same cells (< 1: the model helps)
      count      [H, cols] origins averaged
    `quantiles` (needs m.replicates): bands [nq, H, cols] of msfe over the bootstrap replicates' parameter sets.  `m` is not
    modified."""
    H = int(H)
    if H < 1:
        raise ValueError("H must be >= 1")
    through, qs = _filter_setup(m, through, quantiles)
    rows = through - m.initperiod + 1
    first_origin = m.initperiod + rows // 2 if first_origin is None else int(first_origin)
    if not (m.initperiod <= first_origin <= through):
        raise ValueError(f"first_origin must lie in initperiod..through ({m.initperiod}..{through})")
    band_of = lambda o: o["msfe"]
    band_of.want = ("msfe",)
    cols, o, bands = _filter_run(m, through, H, first_origin - m.initperiod, ("msfe", "msfe0", "cnt"), band_of, qs, ctx)
    msfe, msfe0 = o["msfe"][0], o["msfe0"][0]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dict(horizons=np.arange(1, H + 1), cols=cols, msfe=msfe, rmsfe=np.sqrt(msfe), relative=msfe / msfe0, count=o["cnt"][0])
    return _with_bands(out, qs, bands=bands)


def evaluate_forecasts_rolling(m: DFMModel, H: int, window: int, *, origins=None, step: int = 1, lags=None, start=None,
                               max_em_iter: int = 50, tol_em: float = 1e-6, factor_lags: Optional[int] = None, ctx=None) -> dict:
    """The rolling-window out-of-sample record, RE-ESTIMATED at every origin: what the model forecast when it only knew what was
    known then.  Rows are initperiod..lastperiod of m.data in data units, the series those `estimate()` used.  At origin t (a 1-based
    period) the vintage is the `window` rows ending at t, with series i known through t - lags[i] only (`lags`: publication lags per
    column of m.data, default 0); it is standardised on its own visible cells, the EM runs on it from `start` for at most max_em_iter
    iterations (tol_em as `estimate`; 0 iterations: the start's parameters on per-window standardisation), and the panel is forecast
    h = 0..H rows past t (h = 0: the nowcast of the series not yet published).  One dfm_rolling_eval_batch call on the GPU: the
    windows are the batch of the EM.  origins: increasing periods in initperiod + window - 1 .. lastperiod (default every `step`-th).
    start: a dict with Lam, R, A or Avar, Q, mu0, P0 in standardised units, one set or one per origin (a leading axis), the loadings'
    rows the series estimate() used or those of its own "cols" (column indices of m.data; the `params` and `cols` this function
    returns make such a start), and optionally "sd": the s.d. of the sample those units belong to (absent: the windows' own units).
    The default is m.em_params with the estimation window's s.d. -- LOOK-AHEAD IN THE START VALUES ONLY (the data of every window
    are its own); pass the parameters of a fit on an earlier sample to avoid it.  factor_lags: p of the factor VAR, default the
    start's.  A series with fewer than max(m.nt_min_factor_estimation, r + 1) visible cells in any window is dropped beforehand.
    Returns a dict (data units):
      origins    the 1-based periods, horizons 0 .. H, cols the column indices (0-based) of m.data that were used
      forecast, variance   [origins, H+1, cols] mean and variance of the cell at origin + h given the vintage
      error, error_std     [origins, H+1, cols] x - forecast and the same over its s.d.; NaN unless the target lies in the sample, is
                           observed and was not visible in the vintage
      msfe, rmsfe, relative, count   [H+1, cols] over the scored origins; relative = msfe over that of the vintage's own mean
      params, iters, loglik_path     the windows' parameters (a dict, [origins, ..]), EM iterations and log-likelihood paths
      mean, sd   [origins, cols] of each vintage's visible cells
    `m` is not modified."""
    H, W, step = int(H), int(window), int(step)
    if H < 0:
        raise ValueError("H must be >= 0")
    if start is None and m.em_params is None:
        raise ValueError("the model has not been estimated: run estimate(m, Parametric()) first, or pass start")
    if m.nfac_o != 0:
        raise ValueError("the rolling evaluation needs nfac_o = 0")
    rows = m.lastperiod - m.initperiod + 1
    if not (2 <= W <= rows):
        raise ValueError(f"window must lie in 2..{rows} (the rows initperiod..lastperiod)")
    if step < 1:
        raise ValueError("step must be >= 1")
    first = m.initperiod + W - 1
    org = np.arange(first, m.lastperiod + 1, step) if origins is None else np.asarray(origins, dtype=np.int64).reshape(-1)
    if org.size < 1 or org.min() < first or org.max() > m.lastperiod or np.any(np.diff(org) <= 0):
        raise ValueError(f"origins must increase and lie in the first full window's end..lastperiod ({first}..{m.lastperiod})")
    cols, _, _, sd_full = _forecast_inputs(m, m.lastperiod)
    sp = dict(m.em_params, sd=sd_full) if start is None else dict(start)
    if sp.get("cols") is not None:                                      # the start's own series: a subset of those estimate() used
        scols = np.asarray(sp["cols"], dtype=np.int64).reshape(-1)
        if not np.all(np.isin(scols, cols)) or np.unique(scols).size != scols.size:
            raise ValueError("start['cols'] must be distinct series among those estimate() used")
        cols = scols
    Lam = np.asarray(sp["Lam"], dtype=np.float64)
    A = np.asarray(sp["Avar"] if "Avar" in sp else sp["A"], dtype=np.float64)
    one = Lam.ndim == 2                                                 # one start (no leading axis), or one per origin
    lead = (lambda a: np.asarray(a, dtype=np.float64)[None]) if one else (lambda a: np.asarray(a, dtype=np.float64))
    Lam, R, A, Q, mu0, P0 = (lead(a) for a in (Lam, sp["R"], A, sp["Q"], sp["mu0"], sp["P0"]))
    r = Lam.shape[2]
    p = A.shape[2] // r
    if factor_lags is not None and int(factor_lags) != p:
        raise ValueError(f"factor_lags = {int(factor_lags)} but the start has {p} lag(s)")
    if Lam.shape[1] != cols.size or Lam.shape[0] not in (1, org.size):
        raise ValueError("the start does not match the model's series, or has neither one set nor one per origin")
    if W < p:
        raise ValueError("window must be >= factor_lags")
    lg = np.zeros(m.ns, dtype=np.int64) if lags is None else np.asarray(lags, dtype=np.int64).reshape(-1)
    if lg.size != m.ns or np.any(lg < 0):
        raise ValueError(f"lags must hold one integer >= 0 per column of m.data ({m.ns})")
    lg = lg[cols]
    min_obs = max(int(m.nt_min_factor_estimation), r + 1)
    if np.any(lg > W - min_obs):
        raise ValueError(f"a publication lag beyond window - {min_obs} leaves a series too few rows")
    x = np.ascontiguousarray(m.data[m.initperiod - 1:m.lastperiod, :][:, cols], dtype=np.float64)
    o0 = org - m.initperiod                                             # 0-based rows of x
    cs = np.vstack([np.zeros((1, cols.size), dtype=np.int64), np.cumsum(~np.isnan(x), axis=0)])
    vis = cs[o0[:, None] - lg[None, :] + 1, np.arange(cols.size)[None, :]] - cs[o0 - W + 1]      # [origins, cols] visible cells
    keep = (vis >= min_obs).all(axis=0)
    if keep.sum() < r:
        raise ValueError("fewer series with enough visible cells in every window than factors")
    sd_start = None if sp.get("sd") is None else np.ascontiguousarray(np.asarray(sp["sd"], dtype=np.float64).reshape(-1)[keep])
    x, lg, cols = np.ascontiguousarray(x[:, keep]), lg[keep], cols[keep]
    args = (x, o0, W, H, np.ascontiguousarray(Lam[:, keep]), np.ascontiguousarray(R[:, keep]), A, Q, mu0, P0)
    kw = dict(lags=lg, sd_start=sd_start, min_obs=min_obs, max_iter=int(max_em_iter), tol=float(tol_em))
    with _device(ctx) as ctx:
        o = _numeric_retry(lambda singular_q=False: ctx.rolling_eval_batch_host(*args, singular_q=singular_q, **kw))
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(origins=org, horizons=np.arange(H + 1), cols=cols, forecast=o["fc"], variance=o["fvar"], error=o["err"],
                    error_std=o["err_std"], msfe=o["msfe"], rmsfe=np.sqrt(o["msfe"]), relative=o["msfe"] / o["msfe0"], count=o["cnt"],
                    params=o["params"], iters=o["iters"], loglik_path=o["loglik_path"], mean=o["mean"], sd=o["sd"])


def forecast_diffusion_index(m: DFMModel, H: int, window: int, *, origins=None, step: int = 1, lags=None, own_lags: Optional[int] = None,
                             start=None, max_iter: int = 1000, tol: Optional[float] = None, ctx=None) -> dict:
    """Diffusion-index forecasts (Stock and Watson 2002) from the NON-parametric fit (`estimate_factor`, nfac_o = 0), out of sample:
    do the estimated factors forecast?  Rows are initperiod..lastperiod of m.data in data units, the series with inclcode == 1.  At
    origin t (a 1-based period) the vintage is the `window` rows ending at t, with series i known through t - lags[i] only (`lags`:
    publication lags per column of m.data, default 0); it is standardised on its own visible cells, the factors are re-estimated on
    it by ALS (at most max_iter sweeps, tol as m.tol by default; 0 sweeps: the start's factors as they are), and every series is
    forecast h = 0..H rows past t by a direct regression of the series at s + h on a constant, the factors at s and its own last
    `own_lags` (default m.n_uarlag) visible values, on the complete cases of the window.  The competitors are the same regression
    without the factors (AR) and the vintage's mean.  One dfm_diffusion_eval_batch call on the GPU: the windows are the batch of
    the ALS, no regressor matrix is formed.  origins: increasing periods in initperiod + window - 1 .. lastperiod (default every
    `step`-th); an origin at lastperiod gives real forecasts.  start: the factors the ALS starts from, [rows, r] (one path over
    initperiod..lastperiod) or [origins, window, r]; the default is m.factor, so `estimate_factor` must have run -- LOOK-AHEAD IN THE
    START VALUES ONLY (the data of every window are its own); pass factors estimated on an earlier sample to avoid it.  A series with
    fewer than max(m.nt_min_factor_estimation, r + 1) visible cells in any window is dropped beforehand (see `cols`).
    Returns a dict (data units):
      origins    the 1-based periods, horizons 0 .. H, cols the column indices (0-based) of m.data that were used
      forecast, forecast_ar   [origins, H+1, cols]; NaN where the cell is visible in the vintage (h = 0, lag 0), the regression has too
                              few complete rows, or an own lag of the origin is missing
      variance   [origins, H+1, cols] the regression's residual variance (no parameter or factor uncertainty)
      error, error_ar, error_std   [origins, H+1, cols] x - forecast (..) and error over its s.d.; NaN unless the target lies in the
                              sample, is observed and has a forecast
      msfe, msfe_ar, msfe_mean, count   [H+1, cols] over the scored origins; relative_ar = msfe / msfe_ar, relative_mean = msfe / msfe_mean
      factor [origins, window, r], loadings [origins, cols, r], iters, ssr [origins]   the ALS of every window
      mean, sd   [origins, cols] of each vintage's visible cells
    `m` is not modified."""
    H, W, step = int(H), int(window), int(step)
    if H < 0:
        raise ValueError("H must be >= 0")
    if m.nfac_o != 0:
        raise ValueError("the diffusion-index forecasts need nfac_o = 0")
    r = int(m.nfac_u)
    q = int(m.n_uarlag) if own_lags is None else int(own_lags)
    if q < 0 or 1 + r + q > 32:
        raise ValueError("own_lags must be >= 0 and 1 + nfac_u + own_lags <= 32")
    rows = m.lastperiod - m.initperiod + 1
    if not (r + 2 * q + H + 3 <= W <= rows):
        raise ValueError(f"window must lie in {r + 2 * q + H + 3}..{rows} (1 + r + 2 own_lags + H + 2 .. the rows initperiod..lastperiod)")
    if step < 1:
        raise ValueError("step must be >= 1")
    first = m.initperiod + W - 1
    org = np.arange(first, m.lastperiod + 1, step) if origins is None else np.asarray(origins, dtype=np.int64).reshape(-1)
    if org.size < 1 or org.min() < first or org.max() > m.lastperiod or np.any(np.diff(org) <= 0):
        raise ValueError(f"origins must increase and lie in the first full window's end..lastperiod ({first}..{m.lastperiod})")
    F0 = np.asarray(m.factor[m.initperiod - 1:m.lastperiod, :] if start is None else start, dtype=np.float64)
    if F0.shape not in ((rows, r), (org.size, W, r)):
        raise ValueError(f"start must be [{rows}, {r}] (rows initperiod..lastperiod) or [{org.size}, {W}, {r}] (one per origin)")
    if not np.all(np.isfinite(F0)):
        raise ValueError("the start factors are not finite: run estimate_factor(m) first, or pass start")
    if int(max_iter) < 0:
        raise ValueError("max_iter must be >= 0")
    cols = np.nonzero(m.inclcode == 1)[0]
    lg = np.zeros(m.ns, dtype=np.int64) if lags is None else np.asarray(lags, dtype=np.int64).reshape(-1)
    if lg.size != m.ns or np.any(lg < 0):
        raise ValueError(f"lags must hold one integer >= 0 per column of m.data ({m.ns})")
    lg = lg[cols]
    min_obs = max(int(m.nt_min_factor_estimation), r + 1)
    if np.any(lg > W - min_obs):
        raise ValueError(f"a publication lag beyond window - {min_obs} leaves a series too few rows")
    x = np.ascontiguousarray(m.data[m.initperiod - 1:m.lastperiod, :][:, cols], dtype=np.float64)
    o0 = org - m.initperiod                                             # 0-based rows of x
    cs = np.vstack([np.zeros((1, cols.size), dtype=np.int64), np.cumsum(~np.isnan(x), axis=0)])
    vis = cs[o0[:, None] - lg[None, :] + 1, np.arange(cols.size)[None, :]] - cs[o0 - W + 1]      # [origins, cols] visible cells
    keep = (vis >= min_obs).all(axis=0)
    if keep.sum() < r:
        raise ValueError("fewer series with enough visible cells in every window than factors")
    if lg[keep].min() != 0:
        raise ValueError("every kept series has a publication lag: some series must reach the origin")
    x, lg, cols = np.ascontiguousarray(x[:, keep]), lg[keep], cols[keep]
    kw = dict(q=q, lags=lg, min_obs=min_obs, nt_min=int(m.nt_min_factor_estimation), max_iter=int(max_iter),
              tol=float(m.tol if tol is None else tol))
    with _device(ctx) as ctx:
        o = ctx.diffusion_eval_batch_host(x, o0, W, H, np.ascontiguousarray(F0), **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(origins=org, horizons=np.arange(H + 1), cols=cols, forecast=o["fc"], forecast_ar=o["fc_ar"], variance=o["fvar"],
                    error=o["err"], error_ar=o["err_ar"], error_std=o["err_std"], msfe=o["msfe"], msfe_ar=o["msfe_ar"],
                    msfe_mean=o["msfe0"], relative_ar=o["msfe"] / o["msfe_ar"], relative_mean=o["msfe"] / o["msfe0"], count=o["cnt"],
                    factor=o["F"], loadings=o["Lam"], iters=o["iters"], ssr=o["ssr"], mean=o["mean"], sd=o["sd"])


# ----------------------------------------------------------------------------- structural analysis of the parametric fit
def _structural_checks(m: DFMModel):
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("structural analysis needs nfac_o = 0")


def _to_cols(idx, cols, what):
    """Column indices of m.data as positions in `cols`; a series estimate() dropped is named in the error."""
    out = []
    for i in np.atleast_1d(np.asarray(idx, dtype=np.int64)):
        at = np.nonzero(cols == i)[0]
        if at.size != 1:
            raise ValueError(f"{what}: series {int(i)} is not among the series estimate() used")
        out.append(int(at[0]))
    return np.asarray(out, dtype=np.int32)


def _named_arg(named, cols, r):
    """`named` (None stays None) as r distinct positions in `cols`, or ValueError."""
    nm = None if named is None else _to_cols(named, cols, "named")
    if nm is not None and (nm.size != r or np.unique(nm).size != r):
        raise ValueError(f"named must be {r} distinct series")
    return nm


def _cumulate_arg(cumulate, cols):
    """`cumulate` (None stays None) as a 0 / 1 flag per series of `cols`."""
    if cumulate is None:
        return None
    cum = np.zeros(cols.size, dtype=np.int32)
    cum[_to_cols(cumulate, cols, "cumulate")] = 1
    return cum


def _structural_quantiles(m: DFMModel, quantiles, named):
    """`quantiles` of structural_irf and structural_irf_signs: bands need named series and replicates, in that order."""
    if quantiles is not None and named is None:
        raise ValueError("quantile bands need named series: the replicates are not in a common rotation otherwise")
    if quantiles is not None and getattr(m, "replicates", None) is None:
        raise ValueError(_NEED_REPLICATES)
    return _quantile_arg(quantiles)


def structural_irf(m: DFMModel, H: int, *, named=None, cumulate=None, unit_effect: bool = False, fevd: bool = True,
                   quantiles=None, ctx=None) -> dict:
    """Identified impulse responses and forecast-error variance decompositions of every series of the panel from the parametric
    fit (`estimate(m, Parametric())`, nfac_o = 0); definitions in include/dfm_hip.h (dfm_irf_batch).

    `named`: r distinct column indices of m.data: factor k is the common component of series named[k], and their order is the
    recursive (Cholesky) ordering; None: S = chol(Q) in the fit's own rotation.  `cumulate`: column indices of the series that
    entered in differences; their responses are cumulated.  `unit_effect` (needs named): shock k moves series named[k] by one
    data unit on impact.  Returns a dict:
      cols        column indices of m.data: the series estimate() used
      irf         [len(cols), H, r] in data units (series, horizon, shock: the reference's impulse_response order)
      fevd        [len(cols), H, r + 1] shares of the forecast-error variance, the last slot idiosyncratic (None if not asked for)
    `quantiles` (needs m.replicates and named: replicates are not in a common rotation otherwise): every replicate runs in ONE
    batched call, dfm_quantile_bands gives bands [nq, len(cols), H, r].  AR-idiosyncratic and mixed-frequency fits are out of
    scope.  `m` is not modified."""
    H = int(H)
    if H < 1:
        raise ValueError("H must be >= 1")
    _structural_checks(m)
    if unit_effect and named is None:
        raise ValueError("unit_effect needs named series")
    qs = _structural_quantiles(m, quantiles, named)
    (Lam, R, A, Q, _, _), cols, _, _, sd = _plain_fit(m, m.lastperiod)
    N, r = Lam.shape
    nm = _named_arg(named, cols, r)
    cum = _cumulate_arg(cumulate, cols)
    with _device(ctx) as ctx:
        def run(Lb, Rb, Ab, Qb, want_fevd):
            return ctx.irf_batch_host(Lb, Ab, Qb, Rb, H, sd=_rep(sd, Lb.shape[0]), named=nm, cum=cum, unit_effect=unit_effect,
                                      want_fevd=want_fevd)
        o = run(Lam[None], R[None], A[None], Q[None], fevd)
        bands = None
        if qs is not None:
            ob = run(*_replicate_sets(m)[:4], False)
            bands = ctx.quantile_bands_host(ob["irf"].reshape(ob["irf"].shape[0], -1), qs).reshape(qs.size, r, H, N)
    out = dict(cols=cols, irf=np.ascontiguousarray(o["irf"][0].transpose(2, 1, 0)),
               fevd=None if o["fevd"] is None else np.ascontiguousarray(o["fevd"][0].transpose(2, 1, 0)))
    return _with_bands(out, qs, bands=None if bands is None else np.ascontiguousarray(bands.transpose(0, 3, 2, 1)))


def structural_irf_signs(m: DFMModel, H: int, restrictions, *, candidates: int = 1000, keep: Optional[int] = None, named=None,
                         cumulate=None, fevd: bool = False, quantiles=None, seed: int = 20160415, ctx=None) -> dict:
    """Impulse responses identified by sign restrictions, from the parametric fit (`estimate(m, Parametric())`, nfac_o = 0);
    definitions in include/dfm_hip.h (dfm_signirf_batch).  `candidates` rotations of the base impact matrix (chol(Q), or the
    named-factor one with `named`) are drawn uniformly on the GPU; those whose responses carry the required signs are accepted.

    `restrictions`: rows (series, shock, h0, h1, sign): the response of column `series` of m.data to shock `shock` (0-based) is
    positive (sign = 1) or negative (sign = -1) at every horizon h0..h1 (0 = impact), cumulated responses for the series in
    `cumulate`.  A shock column all of whose rows hold with the signs reversed is flipped, so a shock is identified up to what the
    restrictions say and no further.  `keep`: how many accepted draws to return (default: all of them; the candidate stream is a
    pure function of `seed`, so a second call over the same candidates is exact).  Returns a dict:
      cols             column indices of m.data: the series estimate() used
      irf              [n_kept, len(cols), H, r] in data units (draw, series, horizon, shock)
      fevd             [n_kept, len(cols), H, r + 1] or None
      impact           [n_kept, r, r] the impact matrices S Rot D of the kept draws
      accepted_share   accepted candidates / candidates
      candidates_used  the number of candidates drawn; candidate_index [n_kept]: which of them the kept draws are
    `quantiles` (needs m.replicates -- bootstrap replicates or Gibbs draws -- and named, as structural_irf): one batched call runs
    `candidates` rotations on every replicate's parameters and keeps `keep or 1` draws of each; the pointwise bands
    [nq, len(cols), H, r] over the pooled kept draws come from dfm_quantile_bands; replicates_without_a_draw counts the replicates
    none of whose candidates was accepted.  No accepted draw at all raises ValueError.  Zero and narrative restrictions,
    AR-idiosyncratic and mixed-frequency fits are out of scope.  `m` is not modified."""
    H, M = int(H), int(candidates)
    if H < 1:
        raise ValueError("H must be >= 1")
    if M < 1:
        raise ValueError("candidates must be >= 1")
    if keep is not None and int(keep) < 1:
        raise ValueError("keep must be >= 1")
    _structural_checks(m)
    qs = _structural_quantiles(m, quantiles, named)
    (Lam, R, A, Q, _, _), cols, _, _, sd = _plain_fit(m, m.lastperiod)
    N, r = Lam.shape
    nm = _named_arg(named, cols, r)
    cum = _cumulate_arg(cumulate, cols)
    rs = np.asarray(restrictions, dtype=np.int64)
    if rs.size == 0:
        rs = rs.reshape(0, 5)
    if rs.ndim != 2 or rs.shape[1] != 5:
        raise ValueError("restrictions must be (series, shock, h0, h1, sign) rows")
    rs = rs.copy()
    if rs.shape[0]:
        rs[:, 0] = _to_cols(rs[:, 0], cols, "restrictions")
        if np.any(rs[:, 1] < 0) or np.any(rs[:, 1] >= r):
            raise ValueError(f"restrictions: the shock must lie in 0..{r - 1}")
        if np.any(rs[:, 2] < 0) or np.any(rs[:, 3] < rs[:, 2]) or np.any(rs[:, 3] >= H):
            raise ValueError(f"restrictions: need 0 <= h0 <= h1 < H = {H}")
        if np.any(np.abs(rs[:, 4]) != 1):
            raise ValueError("restrictions: the sign must be +1 or -1")
    with _device(ctx) as ctx:
        def run(sets, K, want_S, want_irf, want_fevd):
            Lb, Rb, Ab, Qb = sets[:4]
            return ctx.signirf_batch_host(Lb, Ab, Qb, Rb, H, rs, M, K, seed=seed, sd=_rep(sd, Lb.shape[0]), named=nm, cum=cum,
                                          want_S=want_S, want_irf=want_irf, want_fevd=want_fevd)
        none = "no candidate satisfied the restrictions: accepted share 0 of {} candidates{}"
        fit = (Lam[None], R[None], A[None], Q[None])
        if keep is None:                                  # count first, then keep them all: the same candidates, exactly
            n = int(run(fit, 1, False, False, False)["n_accept"][0])
            if n == 0:
                raise ValueError(none.format(M, ""))
            o = run(fit, n, True, True, fevd)
        else:
            o = run(fit, int(keep), True, True, fevd)
            n = int(o["n_accept"][0])
            if n == 0:
                raise ValueError(none.format(M, ""))
        nk = min(n, o["cand"].shape[1])
        bands = without = None
        if qs is not None:
            ob = run(_replicate_sets(m), int(keep) if keep is not None else 1, False, True, False)
            got = ob["cand"] >= 0
            if not got.any():
                raise ValueError(none.format(M, " in any replicate"))
            pooled = np.ascontiguousarray(ob["irf"][got])        # [draws, r, H, N]
            bands = ctx.quantile_bands_host(pooled.reshape(pooled.shape[0], -1), qs).reshape(qs.size, r, H, N)
            without = int((ob["n_accept"] == 0).sum())
    out = dict(cols=cols, irf=np.ascontiguousarray(o["irf"][0, :nk].transpose(0, 3, 2, 1)),
               fevd=None if o["fevd"] is None else np.ascontiguousarray(o["fevd"][0, :nk].transpose(0, 3, 2, 1)),
               impact=o["S"][0, :nk].copy(), accepted_share=n / M, candidates_used=M, candidate_index=o["cand"][0, :nk].copy())
    return _with_bands(out, qs, bands=None if bands is None else np.ascontiguousarray(bands.transpose(0, 3, 2, 1)),
                       replicates_without_a_draw=without)


_QUANTILE_MAX_DRAWS = 16384          # dfm_quantile_bands: draws per call, at most


def structural_irf_proxy(m: DFMModel, H: int, instrument, *, norm, draws: int = 0, block: Optional[int] = None, cumulate=None,
                         unit_effect: bool = False, fevd: bool = True, quantiles=None, parameter_draws: bool = False,
                         seed: int = 20160415, ctx=None) -> dict:
    """Impulse responses to ONE structural shock identified by an external instrument (proxy SVAR), from the parametric fit
    (`estimate(m, Parametric())`, nfac_o = 0); definitions in include/dfm_hip.h (dfm_proxyirf_batch).  The instrument is
    correlated with the shock of interest and with no other; the covariance of the factor-VAR innovations with it gives the
    shock's impact column.  No ordering, no named series: the answer does not depend on the rotation the fit sits in.

    `instrument`: one entry per row of m.data, NaN where it does not exist; the estimation window's rows are used.  `norm`: a
    column index of m.data; the shock is signed so that this series rises on impact, and with `unit_effect` it rises by one data
    unit.  `cumulate`: column indices of the series that entered in differences.  `draws`: moving block bootstrap draws of the
    instrument moment (blocks of `block` usable periods; the default block length is ceil(n ** (1/3)) for n usable periods), drawn
    on the GPU as a pure function of `seed`.  Returns a dict:
      cols           column indices of m.data: the series estimate() used
      irf            [len(cols), H] in data units
      fevd           [len(cols), H] share of the forecast-error variance due to the shock (None if not asked for)
      impact         [r] the impact column in the fit's own rotation
      relevance      the squared correlation of the instrument with the identified shock under the model's Q
      shock          [window rows] the identified unit-variance shock (zero in the first factor_lags rows)
      first_stage_F  the F statistic of the regression of the instrument on the factor innovations over the usable periods
    `quantiles` (needs draws >= 1): pointwise bands [nq, len(cols), H] by dfm_quantile_bands over the block draws of the point
    estimate, or with `parameter_draws=True` (needs m.replicates) over `draws` block draws of every replicate pooled; replicates x
    draws may not exceed 16384.  Q must be positive definite for the identification; a numeric failure of the pass is retried once
    in covariance form.  The historical decomposition under the identified shock, several instruments, weak-instrument-robust
    sets, AR-idiosyncratic and mixed-frequency fits are out of scope.  `m` is not modified."""
    H, D = int(H), int(draws)
    if H < 1:
        raise ValueError("H must be >= 1")
    if D < 0:
        raise ValueError("draws must be >= 0")
    _structural_checks(m)
    if quantiles is not None and D < 1:
        raise ValueError("quantile bands need draws >= 1")
    qs = _quantile_arg(quantiles)
    if parameter_draws and getattr(m, "replicates", None) is None:
        raise ValueError("parameter draws need bootstrap replicates: estimate(m, Parametric(), nrep=...) first")
    nrep = m.replicates["params"]["Lam"].shape[0] if parameter_draws else 1
    if qs is not None and nrep * D > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"quantile bands pool replicates x draws = {nrep} x {D} draws; at most {_QUANTILE_MAX_DRAWS} fit one call")
    prm, cols, z, _, sd = _plain_fit(m, m.lastperiod, "structural_irf_proxy", "(estimate_ar_idio?)")
    A = prm[2]
    N, r = prm[0].shape
    p = A.shape[1] // r
    inst = np.asarray(instrument, dtype=np.float64).reshape(-1)
    if inst.size != m.data.shape[0]:
        raise ValueError(f"the instrument must have one entry per row of m.data ({m.data.shape[0]}), NaN where it does not exist")
    zi = np.ascontiguousarray(inst[m.initperiod - 1:m.lastperiod])
    used = np.nonzero(np.isfinite(zi[p:]))[0] + p
    n = used.size
    if n < r + 2:
        raise ValueError(f"the instrument has {n} usable periods in the estimation window; at least r + 2 = {r + 2} are needed")
    L = int(np.ceil(n ** (1.0 / 3.0) - 1e-12)) if block is None else int(block)
    if not 1 <= L <= n:
        raise ValueError(f"block must lie in 1..{n} (the usable periods)")
    nrm = int(_to_cols(norm, cols, "norm")[0])
    cum = _cumulate_arg(cumulate, cols)
    from ._lib import DfmError
    with _device(ctx) as ctx:
        def run(sets, Dd, want_fevd, want_shock):
            B = sets[0].shape[0]
            call = lambda singular_q=False: ctx.proxyirf_batch_host(
                _rep(z, B), *sets, H, zi, nrm, draws=Dd, block=L, seed=seed, sd=_rep(sd, B), cum=cum,
                unit_effect=unit_effect, want_fevd=want_fevd, want_shock=want_shock, may_have_missing=bool(np.isnan(z).any()),
                singular_q=singular_q)
            try:
                return _numeric_retry(call)
            except DfmError as err:                 # the covariance form failed too: say what the identification needs
                if err.code != -5:
                    raise
                text = str(err).split(": ", 2)[-1]
                raise DfmError(err.code, f"{text}; identification by an instrument needs Q positive definite") from None
        o = run(_one(prm), 0 if parameter_draws else D, fevd, True)
        bands = None
        if qs is not None:
            if parameter_draws:
                pooled = run(_replicate_sets(m), D, False, False)["irf"][:, 1:]
            else:
                pooled = o["irf"][:, 1:]
            pooled = pooled.reshape(-1, H * N)
            pooled = np.ascontiguousarray(pooled[np.isfinite(pooled[:, 0])])
            if pooled.shape[0] == 0:
                raise ValueError("no block draw gave a finite response")
            bands = ctx.quantile_bands_host(pooled, qs).reshape(qs.size, H, N)
    f = o["f"][0]
    eta = f[p:].copy()
    for j in range(p):
        eta -= f[p - 1 - j:f.shape[0] - 1 - j] @ A[:, j * r:(j + 1) * r].T
    X = np.column_stack([np.ones(n), eta[used - p]])
    y = zi[used]
    res = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
    rss, tss = float(res @ res), float(((y - y.mean()) ** 2).sum())
    F = ((tss - rss) / r) / (rss / (n - r - 1)) if rss > 0.0 else np.inf
    out = dict(cols=cols, irf=np.ascontiguousarray(o["irf"][0, 0].T),
               fevd=None if o["fevd"] is None else np.ascontiguousarray(o["fevd"][0, 0].T), impact=o["impact"][0, 0].copy(),
               relevance=float(o["rel"][0, 0]), shock=o["shock"][0].copy(), first_stage_F=float(F))
    return _with_bands(out, qs, bands=None if bands is None else np.ascontiguousarray(bands.transpose(0, 2, 1)))


def historical_decomposition(m: DFMModel, *, named=None, through: Optional[int] = None, ctx=None) -> dict:
    """Which shocks drove every series through the sample: the contribution of each identified factor shock and of the initial
    condition to the common component of every cell, from the parametric fit (`estimate(m, Parametric())`, nfac_o = 0);
    definitions in include/dfm_hip.h (dfm_histdecomp_batch).  Window, series, standardisation and `through` as `forecast`;
    `named` as `structural_irf`.  Q must be positive definite: a numeric failure is retried once in covariance form and then
    reported.  Returns a dict:
      rows           1-based periods initperiod .. through
      cols           column indices of m.data: the series estimate() used
      contributions  [rows, cols, r + 1] in data units without the mean (the last slot is the initial condition); the slots sum
                     to sd_i lam_i' E[f_t | X]
      shocks         [rows, r] the unit-variance structural shocks (zero in the first factor_lags rows)
      factor         [rows, r] E[f_t | X]
      loglik         log-likelihood of the observed cells
    AR-idiosyncratic and mixed-frequency fits are out of scope.  `m` is not modified."""
    _structural_checks(m)
    through = _through_arg(m, through)
    prm, cols, z, _, sd = _plain_fit(m, through)
    nm = _named_arg(named, cols, prm[0].shape[1])
    with _device(ctx) as ctx:
        o = _numeric_retry(lambda singular_q=False: ctx.histdecomp_batch_host(
            z[None], *_one(prm), sd=sd[None], named=nm, may_have_missing=bool(np.isnan(z).any()), singular_q=singular_q))
    return dict(rows=np.arange(m.initperiod, through + 1), cols=cols,
                contributions=np.ascontiguousarray(o["hd"][0].transpose(1, 2, 0)), shocks=o["shocks"][0], factor=o["f"][0],
                loglik=float(o["loglik"][0]))


def draw_paths(m: DFMModel, ndraws: int, H: int = 0, *, through: Optional[int] = None, seed: int = 20160415,
               first_draw: int = 0, parameter_draws: bool = False, ctx=None) -> dict:
    """Joint posterior draws of the factor path and of the panel's missing and future cells from the parametric fit
    (`estimate(m, Parametric())`, nfac_o = 0): the counterpart of `forecast`, which gives the marginal moments only.

    Same window, series, standardisation and ragged-edge `through` as `forecast`.  Each draw is an exact, independent draw of
    (f_{initperiod..through+H}, the missing and future cells) given the observed cells, by the simulation smoother of Durbin and
    Koopman (2002): one dfm_simsmooth_batch call on the GPU (include/dfm_hip.h: the random stream is a pure function of `seed`
    and the draw's index first_draw + d, so draws [k, k + n) equal those of a call with first_draw = k).
    Returns a dict:
      rows        1-based periods initperiod .. through + H
      cols        column indices (0-based) of m.data: the series estimate() used
      factor      [ndraws, rows, r] factor paths (the model's standardised factor units)
      x           [ndraws, rows, cols] data units: observed cells as they are, every other cell drawn
    `parameter_draws=True` (needs m.replicates from estimate(..., nrep=...)): every bootstrap replicate's parameter set is one
    replicate of the same call, so the draws carry parameter and shock uncertainty together: factor [nrep, ndraws, rows, r],
    x [nrep, ndraws, rows, cols].  AR idiosyncratic terms and observed factors are refused.  `m` is not modified."""
    ndraws, H, first_draw = int(ndraws), int(H), int(first_draw)
    if ndraws < 1:
        raise ValueError("ndraws must be >= 1")
    if H < 0:
        raise ValueError("H must be >= 0")
    if first_draw < 0:
        raise ValueError("first_draw must be >= 0")
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("draw_paths needs nfac_o = 0 (observed factors have no draws here)")
    through = _through_arg(m, through)
    if parameter_draws and getattr(m, "replicates", None) is None:
        raise ValueError("parameter draws need bootstrap replicates: estimate(m, Parametric(), nrep=...) first")
    prm, cols, z, mu, sd = _plain_fit(m, through, "draw_paths", "-- draw_paths_ar_idio draws from it")
    if z.shape[0] < prm[2].shape[1] // prm[0].shape[1]:
        raise ValueError("the window is shorter than the number of factor lags")
    sets = _replicate_sets(m) if parameter_draws else _one(prm)
    B = sets[0].shape[0]
    kw = dict(seed=int(seed), first_draw=first_draw, mean=_rep(mu, B), sd=_rep(sd, B), may_have_missing=bool(np.isnan(z).any()))
    with _device(ctx) as ctx:                       # the information form inverts Q: as estimate(), retry in covariance form
        o = _numeric_retry(lambda **sq: ctx.simsmooth_batch_host(_rep(z, B), *sets, ndraws, H, **sq, **kw))
    factor, x = (o["f"], o["x"]) if parameter_draws else (o["f"][0], o["x"][0])
    xr = m.data[m.initperiod - 1:through, :][:, cols]                  # observed cells: the data itself, not mean + sd z
    obs = ~np.isnan(xr)
    x[..., :xr.shape[0], :][..., obs] = xr[obs]
    return dict(rows=np.arange(m.initperiod, through + H + 1), cols=cols, factor=factor, x=x)


def simulate(m: DFMModel, ndraws: int, *, seed: int = 20160415, masked: bool = True, ctx=None) -> dict:
    """`ndraws` panels simulated from the parametric fit (`estimate(m, Parametric())`, nfac_o = 0) over the estimation window, for
    Monte-Carlo work that is not a bootstrap: the size of a test under the fitted model, the sampling spread of a statistic.
    One dfm_simulate_batch call on the GPU (the random stream of `draw_paths`' unconditional step: draw d of `seed`).
    Returns a dict:
      rows        1-based periods initperiod .. lastperiod
      cols        column indices (0-based) of m.data: the series estimate() used
      x           [ndraws, rows, cols] data units (window mean + s.d. times the simulated standardised cell); `masked`: NaN where
                  the window's own cell is missing, else balanced
      factor      [ndraws, rows, r] the simulated factor paths (the model's standardised factor units)
    `m` is not modified."""
    ndraws = int(ndraws)
    if ndraws < 1:
        raise ValueError("ndraws must be >= 1")
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("simulate needs nfac_o = 0 (observed factors have no model to draw from)")
    prm, cols, z, mu, sd = _plain_fit(m, m.lastperiod)
    if z.shape[0] < prm[2].shape[1] // prm[0].shape[1]:
        raise ValueError("the window is shorter than the number of factor lags")
    with _device(ctx) as ctx:
        o = ctx.simulate_batch_host(*_one(prm), ndraws, T=z.shape[0], mask_panel=z[None] if masked and np.isnan(z).any() else None,
                                    seed=int(seed))
    return dict(rows=np.arange(m.initperiod, m.lastperiod + 1), cols=cols, x=mu + sd * o["x"][0], factor=o["f"][0])


def estimate_bayesian(m: DFMModel, ndraws: int, *, chains: int = 4, burn: int = 500, thin: int = 1, prior=None,
                      seed: int = 20160415, keep_factors: bool = False, quantiles=None, ctx=None) -> dict:
    """Bayesian estimation of the parametric model (`estimate(m, Parametric())` first, nfac_o = 0) by the Gibbs sampler of
    include/dfm_hip.h: `chains` independent chains, all started at m.em_params, run as one batch on the GPU on the standardised
    estimation window (rows initperiod..lastperiod, the series estimate() used).  Each chain runs `burn` sweeps and then keeps
    `ndraws` sweeps, one in `thin`.  `prior`: a dict that overrides entries of bayes.default_prior(r) (tau_lam, nu_R, s_R,
    tau_A, nu_Q, s_Q, A0).  mu0 and P0 stay at their EM values; the VAR block conditions on the first p drawn rows.
    No rotation or scale normalisation is applied: the common component, R, forecasts and named-factor IRFs are identified,
    Lam, A and Q one by one are not -- summarise those only through such functions.
    Returns a dict:
      params        dict(Lam, R, A, Q, mu0, P0), chains x ndraws flattened on the first axis (chain-major): the layout of
                    m.replicates["params"], so `m.replicates = dict(params=out["params"])` turns the bands of forecast, draw_paths,
                    structural_irf, historical_decomposition, news and evaluate_forecasts into posterior bands
      rows, cols    1-based periods of the window, column indices (0-based) of m.data
      R_mean [N], common_mean [rows, N]       posterior means in data units (sd_i^2 R_i; mean_i + sd_i lam_i' f_t)
      quantiles, R_bands [nq, N], common_bands [nq, rows, N]    with `quantiles`
      rhat_R [N], rhat_common [N]             split-R-hat across the chains of R_i and of the common component of the last period
      factor        [chains x ndraws, rows, r] with keep_factors
      prior, chains, ndraws
    AR idiosyncratic terms and observed factors are refused.  `m` is not modified."""
    from . import bayes
    ndraws, chains, burn, thin = int(ndraws), int(chains), int(burn), int(thin)
    if ndraws < 1 or chains < 1 or burn < 0 or thin < 1:
        raise ValueError("ndraws >= 1, chains >= 1, burn >= 0 and thin >= 1 are required")
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("estimate_bayesian needs nfac_o = 0 (observed factors have no draws here)")
    qs = _quantile_arg(quantiles)
    prm, cols, z, mu, sd = _plain_fit(m, m.lastperiod, "estimate_bayesian", "(estimate_bayesian_ar_idio?)")
    r = prm[0].shape[1]
    p = prm[2].shape[1] // r
    if z.shape[0] <= p:
        raise ValueError("the window is not longer than the number of factor lags")
    pr = bayes.check_prior(prior, r, p, chains)
    keep = ("Lam", "R", "A", "Q", "f")
    d = _gibbs_chains(ctx, "gibbs_batch_host", z, prm, pr, chains, ndraws, burn, thin, seed, keep)
    K = chains * ndraws
    params = dict(Lam=_pooled(d["Lam"]), R=_pooled(d["R"]), A=_pooled(d["A"]), Q=_pooled(d["Q"]), mu0=_rep(prm[4], K), P0=_rep(prm[5], K))
    return _bayes_summary(d, params, np.arange(m.initperiod, m.lastperiod + 1), cols, dict(R=d["R"] * sd ** 2), ("R",), mu, sd, pr,
                          qs, keep_factors)


def _gibbs_chains(ctx, entry, x, start, pr, chains, ndraws, burn, thin, seed, keep):
    """`chains` chains of the Gibbs sampler behind `entry` (a host entry of the context), all started at `start` on panel x: the
    kept draws, name -> [chains, ndraws, ...].  The information form inverts Q: as estimate(), a numeric failure is retried in
    covariance form -- not the sampler's own failures (a Cholesky of its regressions, the Gamma cap), which that form cannot cure."""
    n_sweeps = burn + (ndraws - 1) * thin + 1
    args = (_rep(x, chains), *[_rep(a, chains) for a in start], pr, n_sweeps)
    kw = dict(burn=burn, thin=thin, seed=int(seed), keep=keep, may_have_missing=bool(np.isnan(x).any()))
    with _device(ctx) as ctx:
        return _numeric_retry(lambda **sq: getattr(ctx, entry)(*args, **sq, **kw), unless=lambda err: "Gibbs sampler" in str(err))[1]


def _pooled(a):
    """Draws [chains, ndraws, ...] as [chains x ndraws, ...], chain-major."""
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def _bayes_summary(d, params, rows, cols, stats, checked, mean, sd, pr, qs, keep_factors, mu_f=None):
    """The returned dict of estimate_bayesian / estimate_bayesian_ar_idio from the chains' draws d (name -> [chains, ndraws, ...]).
    stats: name -> draws in data units, each summarised as <name>_mean; those named in `checked` also as rhat_<name> and, with qs,
    <name>_bands.  The common component is mean + sd lam_i' f_t (rhat_common: of the last period).  mu_f (the AR model): returned,
    and added to the factors."""
    from . import bayes
    chains, ndraws = d["f"].shape[:2]
    last = bayes.common_component(d["Lam"], d["f"], mean, sd, rows=[d["f"].shape[2] - 1])[:, :, 0, :]
    out = dict(params=params, rows=rows, cols=cols)
    out.update({k + "_mean": a.mean(axis=(0, 1)) for k, a in stats.items()})
    out.update({"rhat_" + k: bayes.split_rhat(stats[k]) for k in checked})
    out.update(rhat_common=bayes.split_rhat(last), prior=pr, chains=chains, ndraws=ndraws)
    if mu_f is not None:
        out["mu_f"] = mu_f
    if qs is None:
        out["common_mean"] = np.mean([bayes.common_component(d["Lam"][c], d["f"][c], mean, sd).mean(axis=0) for c in range(chains)],
                                     axis=0)
    else:
        cc = _pooled(bayes.common_component(d["Lam"], d["f"], mean, sd))
        out["common_mean"] = cc.mean(axis=0)
        out["quantiles"] = qs
        out.update({k + "_bands": np.quantile(_pooled(stats[k]), qs, axis=0) for k in checked})
        out["common_bands"] = np.quantile(cc, qs, axis=0)
    if keep_factors:
        out["factor"] = _pooled(d["f"]) if mu_f is None else _pooled(d["f"]) + mu_f
    return out


def news(m: DFMModel, old, new, targets, *, groups=None, quantiles=None, ctx=None) -> dict:
    """News decomposition of the revision of nowcasts / forecasts between two data vintages (Banbura and Modugno 2014) from the
    parametric fit (`estimate(m, Parametric())`, nfac_o = 0), with one parameter set for both vintages.

    `old` / `new`: arrays shaped like m.data (same columns; the one with fewer rows is padded with NaN rows), or ints meaning
    "m.data through that 1-based row" (pseudo real-time vintages).  Every cell observed in old must be observed in new.
    `targets`: (column of m.data, 1-based period) pairs, as `forecast`'s rows; a period past the data is a forecast.
    Series, window mean / s.d. and standardisation are those of `forecast`.  One dfm_news_batch call on the GPU.
    Returns a dict (data units):
      rows, cols        1-based periods initperiod .. the last row of the vintages; the series estimate() used
      y_old, y_rev, y_new   [G] the target conditioned on old, on the revised old data (new values on old's cells), on new
      revision          y_new - y_old = data_revision (y_rev - y_old) + news_effect (y_new - y_rev)
      impact            [G, cols] contribution of each series' new releases; sums to news_effect
      news              [rows, cols] the news I = x_new - E[x | revised old] on the new cells, 0 elsewhere
      weight            [G, rows, cols] d y_new / d x on new's observed cells (on the news cells: Cov(y, I) Var(I)^-1)
      groups            {name: [G]} impacts summed over the columns of each group (with `groups`: name -> columns of m.data)
    `quantiles` (needs m.replicates from estimate(..., nrep=...)): every bootstrap parameter set runs in the same batched call,
    and nearest-rank bands over the replicates give impact_bands [nq, G, cols] and revision_bands [nq, G].  `m` is not
    modified."""
    _need_fit(m)
    if m.nfac_o != 0:
        raise ValueError("news needs nfac_o = 0 (observed factors have no news here)")
    xo, xn, last = _vintages(m, old, new)
    if np.any(~np.isnan(xo) & np.isnan(xn)):
        raise ValueError("vintage: a cell observed in the old vintage is missing in the new one")
    tg = _target_list(targets)
    prm, cols, _, mu, sd = _plain_fit(m, m.lastperiod)
    pos = {int(c): j for j, c in enumerate(cols)}
    pairs = _news_targets(m, tg, pos, "estimate() used")
    gsum = _news_groups(groups, pos, "estimate() used")
    _no_ar_terms(m, cols, "news", "(news_ar_idio is the call for it)")
    qs = _quantile_arg(quantiles, (getattr(m, "replicates", None) is None, _NEED_REPLICATES))
    zo = (xo[m.initperiod - 1:, cols] - mu) / sd
    zn = (xn[m.initperiod - 1:, cols] - mu) / sd
    sets = _one(prm)
    if qs is not None:                              # replicate 0: the point estimate; 1 ..: the bootstrap parameter sets
        sets = [np.concatenate([a, b]) for a, b in zip(sets, _replicate_sets(m))]
    B = sets[0].shape[0]
    o, bands = _news_call(ctx, "news_batch_host", (_rep(zo, B), _rep(zn, B), *sets, pairs),
                          dict(mean=_rep(mu, B), sd=_rep(sd, B), may_have_missing=bool(np.isnan(zn).any())), qs)
    return _news_result(o, np.arange(m.initperiod, last + 1), cols, {}, gsum, qs, bands)


def _vintages(m: DFMModel, old, new):
    """The two vintages of news / news_ar_idio -- each an array shaped like m.data, or a 1-based row meaning "m.data through it" --
    as float64 arrays padded with NaN rows to the same number of rows: (old, new, that number)."""
    ncol = m.data.shape[1]

    def vintage(v, name):
        if np.isscalar(v) and float(v) == int(v):
            t = int(v)
            if not (m.initperiod <= t <= m.T):
                raise ValueError(f"{name} vintage: through must lie in initperiod..T ({m.initperiod}..{m.T})")
            return np.asarray(m.data[:t], dtype=np.float64)
        x = np.asarray(v, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != ncol or x.shape[0] < m.initperiod:
            raise ValueError(f"{name} vintage: an array shaped like m.data ([rows >= initperiod, {ncol}]) or a 1-based row")
        return x
    xo, xn = vintage(old, "old"), vintage(new, "new")
    last = max(xo.shape[0], xn.shape[0])
    padr = lambda x: np.vstack([x, np.full((last - x.shape[0], ncol), np.nan)])
    return padr(xo), padr(xn), last


def _target_list(targets):
    """`targets` as a list with at least one entry, or ValueError."""
    tg = list(targets) if targets is not None else []
    if len(tg) < 1:
        raise ValueError("at least one target (column, period) is needed")
    return tg


def _news_targets(m: DFMModel, tg, pos, used, q=0):
    """(column of m.data, 1-based period) targets as (window row, position) pairs; pos: column -> position among the series `used`
    (the message's words for them); q: the window's first q rows are conditioning values and no targets."""
    pairs = []
    for c, per in tg:
        if int(c) not in pos:
            raise ValueError(f"target column {c} is not one of the series {used}")
        if int(per) < m.initperiod + q:
            raise ValueError(f"target period {per} lies before initperiod ({m.initperiod})" if q == 0 else
                             f"target period {per} lies before initperiod + n_uarlag ({m.initperiod + q}): the first n_uarlag "
                             "window rows are conditioning values")
        pairs.append((int(per) - m.initperiod, pos[int(c)]))
    return pairs


def _news_groups(groups, pos, used):
    """`groups` (name -> columns of m.data; None stays None) as name -> positions among the series `used`."""
    if groups is None:
        return None
    gsum = {}
    for name, gc in dict(groups).items():
        idx = [pos.get(int(c), -1) for c in np.atleast_1d(gc)]
        if len(idx) < 1 or min(idx) < 0:
            raise ValueError(f"groups[{name!r}] must list columns {used}")
        gsum[name] = np.asarray(idx)
    return gsum


def _news_call(ctx, entry, args, kw, qs):
    """One call of the news entry `entry` (a host entry of the context) with replicate 0 the point estimate -- the information form
    inverts Q: as estimate(), retried in covariance form -- and, with qs, the nearest-rank bands of the impacts and of the revision
    over the replicates behind it: (outputs, (impact_bands, revision_bands) or None)."""
    with _device(ctx) as ctx:
        o = _numeric_retry(lambda **sq: getattr(ctx, entry)(*args, **sq, **kw))
        bands = None
        if qs is not None:
            bands = (ctx.quantile_bands_host(o["impact"][1:], qs),
                     ctx.quantile_bands_host(o["yhat"][1:, 2] - o["yhat"][1:, 0], qs))
    return o, bands


def _news_result(o, rows, cols, extra, gsum, qs, bands):
    """The returned dict of news / news_ar_idio from replicate 0 of the outputs; `extra`: the entries that follow `weight`."""
    y = o["yhat"][0]
    out = dict(rows=rows, cols=cols, y_old=y[0], y_rev=y[1], y_new=y[2], revision=y[2] - y[0],
               data_revision=y[1] - y[0], news_effect=y[2] - y[1], impact=o["impact"][0], news=o["news"][0],
               weight=o["weight"][0], **extra)
    if gsum is not None:
        out["groups"] = {name: out["impact"][:, idx].sum(axis=1) for name, idx in gsum.items()}
    if bands is not None:
        out["quantiles"] = qs
        out["impact_bands"], out["revision_bands"] = bands
    return out


# ============================================================================= the NON-parametric path
# `estimate!(m, ::NonParametric)` (dfm_functions.ipynb:530-543) = estimate_factor! -> estimate_factor_loading!
# -> estimate_var!, with every regression run by the batched HIP kernels of als.hip (dfm_als_batch /
# dfm_ols_batch) and the PCA start by pca.hip.  The host code below is what the reference's Julia host code is:
# slicing, standardising, building lag matrices, copying results into the model object.
# ----------------------------------------------------------------------------- mixed frequency: monthly factors, quarterly series
MF_WEIGHTS = {"m": (1.0,), "q_flow": (1 / 3, 2 / 3, 1.0, 2 / 3, 1 / 3), "q_avg": (1 / 3, 1 / 3, 1 / 3)}


def mf_weights(weights, N: int) -> np.ndarray:
    """[N][L] aggregation weights from the array itself or from a list of "m" (monthly), "q_flow" (quarterly growth rate,
    Mariano-Murasawa (1, 2, 3, 2, 1) / 3) and "q_avg" (quarterly mean of a monthly level, (1, 1, 1) / 3)."""
    if len(weights) and isinstance(weights[0], str):
        unknown = sorted(set(weights) - set(MF_WEIGHTS))
        if unknown:
            raise ValueError(f"unknown weight pattern {unknown}: use 'm', 'q_flow', 'q_avg' or an [N][L] array")
        W = np.zeros((len(weights), max(len(MF_WEIGHTS[k]) for k in weights)))
        for i, k in enumerate(weights):
            W[i, :len(MF_WEIGHTS[k])] = MF_WEIGHTS[k]
    else:
        W = np.array(weights, dtype=np.float64, ndmin=2)
    if W.shape[0] != N:
        raise ValueError(f"weights: {W.shape[0]} rows for {N} series")
    return np.ascontiguousarray(W)


def _mf_expanded(Lam, W, Avar, Q):
    """The mixed-frequency model as a plain p = 1 model on the companion state: (LamK [N, k], M [k, k], Qk [k, k]), k = r max(p, L)."""
    N, r = Lam.shape
    L = W.shape[1]
    p = Avar.shape[1] // r
    m = max(p, L)
    k = r * m
    LamK = np.zeros((N, m, r))
    LamK[:, :L] = W[:, :, None] * Lam[:, None, :]
    M = np.zeros((k, k))
    M[:r, :r * p] = Avar
    M[r:, :k - r] = np.eye(k - r)
    Qk = np.zeros((k, k))
    Qk[:r, :r] = Q
    return LamK.reshape(N, k), M, Qk


def _mf_start(ctx, z, W, r, p):
    """Start of the EM: PCA factors of the fully observed MONTHLY series (pca_start), every series' loadings by a regression on
    the aggregated PCA factors over its observed cells, VAR(p) by OLS, P0 = the stacked lags' second moment."""
    T, N = z.shape
    L = W.shape[1]
    m = max(p, L)
    monthly = (W[:, 0] == 1.0) & np.all(W[:, 1:] == 0.0, axis=1)
    if not monthly.any():
        raise ValueError("no monthly series (weights (1, 0, ..)): nothing to start the factors from")
    F = pca_start(ctx, z[:, monthly], r)
    Flag = np.stack([np.vstack([np.zeros((l, r)), F[:T - l]]) for l in range(L)])       # [L, T, r]: f_{t-l}
    Lam = np.zeros((N, r)); R = np.ones(N)
    for i in range(N):
        g = np.tensordot(W[i], Flag, axes=1)
        o = ~np.isnan(z[:, i]); o[:L - 1] = False
        if o.sum() < r + 1:
            continue
        Lam[i] = np.linalg.lstsq(g[o], z[o, i], rcond=None)[0]
        R[i] = max(np.mean((z[o, i] - g[o] @ Lam[i]) ** 2), 0.05)
    Z = np.hstack([F[p - 1 - l:T - l] for l in range(p)])
    Y, Xl = F[p:], Z[:-1]
    Avar = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y).T
    e = Y - Xl @ Avar.T
    Q = e.T @ e / (T - p)
    Zm = np.hstack([F[m - 1 - l:T - l] for l in range(m)])
    P0 = Zm.T @ Zm / Zm.shape[0] + 1e-3 * np.eye(r * m)
    return dict(Lam=Lam, R=R, Avar=Avar, Q=0.5 * (Q + Q.T), mu0=np.zeros(r * m), P0=0.5 * (P0 + P0.T))


def mf_blocks(membership, factors) -> np.ndarray:
    """The `free` matrix of a block structure (Banbura and Modugno 2014).  membership [N][G] (boolean): which series belong to
    which block -- a column of all True is a global block; factors [G]: the factor count of each block.  Returns free
    [N][sum(factors)] (boolean, True = the loading is estimated), the columns in block order: block g's factors load on its own
    series only, every other loading is fixed (at 0 in estimate_mixed_frequency's start)."""
    mem = np.asarray(membership)
    fac = np.asarray(factors)
    if mem.ndim != 2 or fac.ndim != 1 or fac.shape[0] != mem.shape[1] or mem.shape[1] < 1:
        raise ValueError("mf_blocks: membership must be [N][G] and factors [G]")
    if fac.dtype.kind not in "iu" or np.any(fac < 1):
        raise ValueError("mf_blocks: every block needs a whole number >= 1 of factors")
    mem = mem != 0
    if not mem.any(axis=1).all():
        raise ValueError(f"mf_blocks: series {np.nonzero(~mem.any(axis=1))[0].tolist()} belong to no block")
    if not mem.any(axis=0).all():
        raise ValueError(f"mf_blocks: blocks {np.nonzero(~mem.any(axis=0))[0].tolist()} have no series")
    return np.ascontiguousarray(np.repeat(mem, fac, axis=1))


def _mf_free(blocks, N: int, r: int) -> np.ndarray:
    """blocks= of estimate_mixed_frequency as a free [N][r] boolean matrix: the matrix itself, or (membership, factors)."""
    if isinstance(blocks, (tuple, list)) and len(blocks) == 2 and np.ndim(blocks[0]) == 2:
        free = mf_blocks(*blocks)
    else:
        free = np.asarray(blocks)
        if free.ndim != 2:
            raise ValueError("blocks: a free [N][r] matrix or (membership [N][G], factors [G])")
        free = np.ascontiguousarray(free != 0)
    if free.shape[0] != N:
        raise ValueError(f"blocks: {free.shape[0]} rows for {N} series")
    if free.shape[1] != r:
        raise ValueError(f"blocks: {free.shape[1]} factor columns, but r = {r}")
    return free


def _mf_block_runs(free):
    """Maximal runs of equal adjacent columns of free -- the blocks, as far as the start needs them: [(first, past the last, members)]."""
    runs, c0 = [], 0
    for c in range(1, free.shape[1] + 1):
        if c == free.shape[1] or not np.array_equal(free[:, c], free[:, c0]):
            runs.append((c0, c, free[:, c0]))
            c0 = c
    return runs


def _mf_blocks_start(ctx, z, W, free, p):
    """Block-wise start of the EM with fixed loadings: for each block in order (a run of equal columns of free), the first principal
    components (pca_start) of the block's fully observed MONTHLY series after the factors of the earlier blocks are projected
    out; every series regresses on its FREE aggregated factors only, its fixed loadings start at 0; VAR(p), P0 and the variance
    floor as _mf_start."""
    T, N = z.shape
    r = free.shape[1]
    L = W.shape[1]
    m = max(p, L)
    monthly = (W[:, 0] == 1.0) & np.all(W[:, 1:] == 0.0, axis=1)
    full = ~np.isnan(z).any(axis=0)
    F = np.zeros((T, 0))
    for c0, c1, member in _mf_block_runs(free):
        sel = monthly & full & member
        if not sel.any():
            raise ValueError(f"blocks: factor columns {c0}..{c1 - 1} have no fully observed monthly series to start from")
        zb = z[:, sel]
        if F.shape[1]:
            zb = zb - F @ np.linalg.lstsq(F, zb, rcond=None)[0]
        F = np.hstack([F, pca_start(ctx, zb, c1 - c0)])
    Flag = np.stack([np.vstack([np.zeros((l, r)), F[:T - l]]) for l in range(L)])       # [L, T, r]: f_{t-l}
    Lam = np.zeros((N, r)); R = np.ones(N)
    for i in range(N):
        fr = np.nonzero(free[i])[0]
        g = np.tensordot(W[i], Flag, axes=1)[:, fr]
        o = ~np.isnan(z[:, i]); o[:L - 1] = False
        if o.sum() < len(fr) + 1:
            continue
        lam = np.linalg.lstsq(g[o], z[o, i], rcond=None)[0] if len(fr) else np.zeros(0)
        Lam[i, fr] = lam
        R[i] = max(np.mean((z[o, i] - g[o] @ lam) ** 2), 0.05)
    Z = np.hstack([F[p - 1 - l:T - l] for l in range(p)])
    Y, Xl = F[p:], Z[:-1]
    Avar = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y).T
    e = Y - Xl @ Avar.T
    Q = e.T @ e / (T - p)
    Zm = np.hstack([F[m - 1 - l:T - l] for l in range(m)])
    P0 = Zm.T @ Zm / Zm.shape[0] + 1e-3 * np.eye(r * m)
    return dict(Lam=Lam, R=R, Avar=Avar, Q=0.5 * (Q + Q.T), mu0=np.zeros(r * m), P0=0.5 * (P0 + P0.T))


def estimate_mixed_frequency(x, weights, r: int, p: int, *, max_em_iter: int = 50, tol_em: float = 1e-6, nrep: int = 0,
                             seed: int = 20160415, blocks=None, ctx=None) -> dict:
    """Maximum likelihood of the mixed-frequency DFM by EM (include/dfm_hip.h: dfm_em_mf_batch): monthly factors f_t with
    VAR(p) dynamics, series i loading on sum_l w_il f_{t-l}.

    blocks (None: every loading is estimated, nothing below applies): a block structure of the loadings (dfm_em_mf_blocks_batch) --
    either a free [N][r] matrix (nonzero = estimated, zero = fixed at its starting value, which is 0) or (membership [N][G],
    factors [G]) as mf_blocks takes them; r must equal the number of factor columns.  The factor VAR stays unrestricted.  The start
    is block-wise (`_mf_blocks_start`; a block without a fully observed monthly series is a ValueError), the bootstrap replicates
    run under the same mask, and the returned dict gains `free`.  forecast_mixed takes such a fit as it is.  A SINGLE-frequency
    block model is this call with all weights "m".

    x [T, N] is the MONTHLY panel in data units: a quarterly series sits in the third month of each quarter and is NaN elsewhere.
    `weights`: the [N][L] array, or a list of "m" / "q_flow" / "q_avg" (mf_weights).  Every series is standardised with its own
    mean and population s.d. over its observed cells (standardize_data).  Start: `_mf_start`.  Returns a dict: Lam [N, r], R [N],
    Avar [r, r p], Q, mu0, P0 (standardised units), W, mean, sd, loglik_path (NaN past convergence), iters, f_smooth [T, r],
    start (the parameters the EM started from); with nrep > 0 also `replicates`: parametric-bootstrap panels drawn from the fit
    with the panel's missing pattern and re-estimated from the point estimate in ONE batched call (params, loglik_path, iters)."""
    x = np.asarray(x, dtype=np.float64)
    T, N = x.shape
    W = mf_weights(weights, N)
    n = np.count_nonzero(~np.isnan(x), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.nansum(x, axis=0) / n
    z, sd = standardize_data(x)
    sd = np.asarray(sd).reshape(N)
    free = None if blocks is None else _mf_free(blocks, N, int(r))
    with _device(ctx) as ctx:
        start = _mf_start(ctx, z, W, int(r), int(p)) if free is None else _mf_blocks_start(ctx, z, W, free, int(p))
        keys = ("Lam", "R", "Avar", "Q", "mu0", "P0")

        def run(panels, st, **kw):
            args = [panels, st["Lam"], st["R"], W, st["Avar"], st["Q"], st["mu0"], st["P0"]]
            em = ctx.em_mf_batch_host
            if free is not None:
                args.insert(4, free)
                em = ctx.em_mf_blocks_batch_host
            # the information form inverts Q: as estimate(), retry in covariance form
            return _numeric_retry(lambda **sq: em(*args, max_iter=max_em_iter, tol=tol_em, may_have_missing=True, **sq, **kw))
        est, path, iters, f, _ = run(z[None], {k: start[k][None] for k in keys})
        out = {k: est[k][0] for k in keys}
        out.update(W=W, mean=mu, sd=sd, loglik_path=path[0], iters=int(iters[0]), f_smooth=f[0], start=start)
        if free is not None:
            out["free"] = free
        if nrep > 0:
            LamK, M, Qk = _mf_expanded(out["Lam"], W, out["Avar"], out["Q"])
            k = M.shape[0]
            rng = np.random.default_rng(seed)
            LQ, LS, sq = _psd_sqrt(Qk), _psd_sqrt(out["P0"]), np.sqrt(out["R"])
            panels = np.empty((nrep, T, N))
            for b in range(nrep):
                s = out["mu0"] + LS @ rng.standard_normal(k)
                for t in range(T):
                    s = M @ s + LQ @ rng.standard_normal(k)
                    panels[b, t] = LamK @ s + sq * rng.standard_normal(N)
            panels[:, np.isnan(z)] = np.nan
            rest, rpath, riters, _, _ = run(panels, {k: np.repeat(out[k][None], nrep, axis=0) for k in keys})
            out["replicates"] = dict(params=rest, loglik_path=rpath, iters=riters)
    return out


def forecast_mixed(fit: dict, x, H: int, quantiles=None, *, ctx=None) -> dict:
    """Nowcasts and H-step forecasts of every cell of a mixed-frequency panel, quarterly series included, in data units.

    `fit` is what estimate_mixed_frequency returned; x [T, N] the monthly panel to condition on (the fit's own, or a later
    vintage with a longer ragged edge).  The expanded model -- loadings N x k, companion transition, [Q 0; 0 0] -- is a plain
    p = 1 model with k = r max(p, L) factors, so this is ONE dfm_forecast_batch call in covariance form; a shape that entry
    refuses raises its status unchanged.  Returns a dict: x [T + H, N] (observed cells as they are, every other cell -- the
    months a quarterly series is not published in, too -- E[x_ti | X]), x_sd (0 on observed cells), common, factor [T + H, r],
    loglik.  `quantiles` (needs fit["replicates"], H >= 1): bands [nq, H, N] over the replicates' point forecasts."""
    H = int(H)
    if H < 0:
        raise ValueError("H must be >= 0")
    x = np.asarray(x, dtype=np.float64)
    W, mu, sd = fit["W"], fit["mean"], fit["sd"]
    r = fit["Lam"].shape[1]
    if x.ndim != 2 or x.shape[1] != W.shape[0]:
        raise ValueError("x must be [T, N] with the fit's series")
    qs = _quantile_arg(quantiles, (fit.get("replicates") is None,
                                   "quantile bands need bootstrap replicates: estimate_mixed_frequency(..., nrep=...) first"),
                       (H < 1, "quantile bands need H >= 1"))
    z = (x - mu) / sd
    with _device(ctx) as ctx:
        def run(ps, **kw):
            B = ps["Lam"].shape[0]
            ex = [_mf_expanded(ps["Lam"][b], W, ps["Avar"][b], ps["Q"][b]) for b in range(B)]
            return ctx.forecast_batch_host(_rep(z, B), np.stack([e[0] for e in ex]), ps["R"], np.stack([e[1] for e in ex]),
                                           np.stack([e[2] for e in ex]), ps["mu0"], ps["P0"], H, mean=_rep(mu, B), sd=_rep(sd, B),
                                           may_have_missing=True, singular_q=True, **kw)
        o = run({k: fit[k][None] for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")}, want_P=False)
        bands = None
        if qs is not None:
            bands = _horizon_bands(ctx, run(fit["replicates"]["params"], want_var=False, want_common=False, want_P=False), H, qs)
    out = dict(x=o["xhat"][0], x_sd=np.sqrt(o["xvar"][0]), common=o["common"][0], factor=o["f"][0][:, :r],
               loglik=float(o["loglik"][0]))
    return _with_bands(out, qs, bands=bands)


def _lagmat(X: np.ndarray, lags) -> np.ndarray:
    """dfm_functions.ipynb:295-303."""
    X = X.reshape(X.shape[0], -1)
    T, nc = X.shape
    lags = list(lags)
    out = np.full((T, nc * len(lags)), np.nan)
    for k, lag in enumerate(lags):
        out[lag:, nc * k: nc * (k + 1)] = X[: T - lag]
    return out


def pca_start(ctx, z: np.ndarray, r: int) -> np.ndarray:
    """`pca_score` (dfm_functions.ipynb:179-183) of the columns of z without a missing cell (:345-348)."""
    xbal, _ = drop_missing_col(z)
    if xbal.shape[1] < r:
        raise ValueError("fewer fully observed series than factors: cannot initialise by PCA")
    _, F0 = ctx.pca_init_batch_host(xbal[None, :, :], r)
    return F0[0]


def estimate_factor(m: DFMModel, max_iter: int = 100000000, computeR2: bool = True, *, lam_constr=None, ctx=None):
    """`estimate_factor!(m, max_iter, computeR2)` -- dfm_functions.ipynb:328-382 (nfac_o = 0, no constraint)."""
    if lam_constr is not None:
        raise NotImplementedError("loading constraints are not supported on the HIP path")
    if m.nfac_o != 0:
        return _estimate_factor_observed(m, max_iter, computeR2, ctx)
    r = m.nfac_u
    xdata = m.data[m.initperiod - 1:m.lastperiod, :][:, m.inclcode == 1]   # :335-336
    z, _ = standardize_data(xdata)                                         # :339
    m.fes.tss = float(np.nansum(z * z))                                    # :342
    m.fes.nobs = int((~np.isnan(z)).sum())                                 # :343
    with _device(ctx) as ctx:
        F0 = pca_start(ctx, z, r)                                          # :345-348
        o = ctx.als_batch_host(z, F0[None], nt_min=m.nt_min_factor_estimation, max_iter=max_iter, tol=m.tol,
                               want_R2=computeR2)                          # :352-370 (+ :372-380)
    m.factor[m.initperiod - 1:m.lastperiod, :] = o["F"][0]                 # :371
    m.fes.ssr = float(o["ssr"][0])                                         # :366
    if computeR2:
        m.fes.R2 = o["R2"][0].copy()
    m.als_iters = int(o["iters"][0])
    return None


def _estimate_factor_observed(m: DFMModel, max_iter, computeR2, ctx):
    """`estimate_factor!` with OBSERVED factors, as the reference's loop is evidently meant (dfm_functions.ipynb:352-371: the
    factor step already regresses on `lambda[:, nfac_o+1:end]` only, :364; what is broken is that the loading step regresses
    on the nfac_u estimated columns alone, :358-359, and :371 writes nfac_u columns into nfac_t -- App. D 7).  g_t = the first
    nfac_o columns of `m.factor` (filled by the caller).  Per sweep TWO batched complete-case regressions on the GPU
    (dfm_ols_batch): every series on [g, f] (N problems), then every period's x_t - Lam_o g_t on Lam_u (T problems sharing
    the regressors) -- `ols_skipmissing(.., Unbalanced())` of :364; the stopping rule is the reference's (:366-368)."""
    ro, ru = m.nfac_o, m.nfac_u
    w0, w1 = m.initperiod - 1, m.lastperiod
    G = np.array(m.factor[w0:w1, :ro], float)
    if np.isnan(G).any():
        raise ValueError("observed factors: fill m.factor[initperiod:lastperiod, :nfac_o] (no gaps) before estimate_factor()")
    z, _ = standardize_data(m.data[w0:w1, :][:, m.inclcode == 1])          # :335-339
    T, N = z.shape
    m.fes.tss = float(np.nansum(z * z)); m.fes.nobs = int((~np.isnan(z)).sum())
    with _device(ctx) as ctx:
        res = ctx.ols_batch_host(G, z, want_resid=True)["resid"]           # start: PCA of what g does not explain
        F = pca_start(ctx, res, ru)
        ssr, it = 0.0, 0
        for it in range(1, int(min(max_iter, 10 ** 8)) + 1):
            ssr_old = ssr
            lam = ctx.ols_batch_host(np.hstack([G, F]), z, nt_min=m.nt_min_factor_estimation, want_resid=False)["beta"]   # :355-361
            y = z - G @ lam[:, :ro].T                                      # NaN rows of lam (short series) drop out below
            o = ctx.ols_batch_host(lam[:, ro:], y.T, want_resid=False)     # :364, one problem per period
            F = o["beta"]
            ssr = float(o["ssr"].sum())                                    # :366
            if not abs(ssr_old - ssr) >= m.tol * m.fes.T * m.fes.ns:       # :367-368
                break
        m.factor[w0:w1, ro:] = F                                           # :371 (the observed columns stay the caller's)
        m.fes.ssr = ssr
        m.als_iters = it
        if computeR2:                                                      # :372-380
            o = ctx.ols_batch_host(np.hstack([G, F]), z, nt_min=m.nt_min_factor_estimation, want_resid=False)
            m.fes.R2 = np.where(np.isnan(o["beta"][:, 0]), np.nan, 1.0 - o["ssr"] / o["tss"])
    return None


def estimate_factor_loading(m: DFMModel, *, lam_constr=None, ctx=None):
    """`estimate_factor_loading!(m)` -- dfm_functions.ipynb:391-415: every series (raw units) on [F 1] over the
    complete cases of the window, r2, then an AR(n_uarlag) of the residuals."""
    if lam_constr is not None:
        raise NotImplementedError("loading constraints are not supported on the HIP path")
    F = m.factor[m.initperiod - 1:m.lastperiod, :]
    Y = m.data[m.initperiod - 1:m.lastperiod, :]
    T, r = F.shape
    X = np.column_stack([F, np.ones(T)])
    with _device(ctx) as ctx:
        o = ctx.ols_batch_host(X, Y, nt_min=m.nt_min_factorloading_estimation)
        ok = ~np.isnan(o["beta"][:, 0])
        r2 = 1.0 - o["ssr"] / o["tss"]
        m.lambda_[ok, :] = o["beta"][ok, :r]
        m.r2[ok] = r2[ok]
        # AR(n) of the residuals with the gaps closed up (the reference hands `uar` the residual VECTOR of the
        # complete cases, :404-407); one regression problem per series, own lag matrix each
        nlag = m.n_uarlag
        idx = np.nonzero(ok & (r2 < 0.9999))[0]
        if idx.size:
            U = np.full((T, idx.size), np.nan)
            XL = np.full((idx.size, T, nlag), np.nan)
            nu = np.zeros(idx.size, dtype=int)
            for q, i in enumerate(idx):
                u = o["resid"][:, i]
                u = u[~np.isnan(u)]
                nu[q] = u.size
                U[:u.size, q] = u
                XL[q, :u.size] = _lagmat(u, range(1, nlag + 1))
            a = ctx.ols_batch_host(XL, U, nt_min=0, want_resid=False)
            m.uar_coef[idx, :] = a["beta"]
            m.uar_ser[idx] = np.sqrt(a["ssr"] / (nu - nlag))                # :310
        hi = np.nonzero(ok & ~(r2 < 0.9999))[0]
        m.uar_coef[hi, :] = 0.0
        m.uar_ser[hi] = 0.0
    return None


def estimate_var(varm: VARModel, compute_matrices: bool = True, *, ctx=None):
    """`estimate_var!(varm, compute_matrices)` + `fill_matrices!` -- dfm_functions.ipynb:444-492."""
    yr = varm.y[varm.initperiod - 1:varm.lastperiod, :]
    T, ns = yr.shape
    x = _lagmat(yr, range(1, varm.nlag + 1))
    if varm.withconst:
        x = np.column_stack([np.ones(T), x])
    rows_ok = ~np.isnan(x).any(axis=1) & ~np.isnan(yr).any(axis=1)         # the reference drops rows jointly (:455)
    Y = np.where(rows_ok[:, None], yr, np.nan)
    with _device(ctx) as ctx:
        o = ctx.ols_batch_host(x, Y, nt_min=0)
    K = x.shape[1]
    varm.betahat = o["beta"].T.copy()
    e = o["resid"][rows_ok]
    T_used = int(rows_ok.sum())
    varm.seps = e.T @ e / (T_used - K)
    varm.resid[:] = np.nan
    varm.resid[varm.initperiod - 1 + np.nonzero(rows_ok)[0]] = e
    if compute_matrices:
        _fill_matrices(varm)
    return None


def _fill_matrices(varm: VARModel):
    """`fill_matrices!` -- dfm_functions.ipynb:477-492: companion M, selection Q, G = lower Cholesky factor of seps."""
    ns = varm.seps.shape[0]
    b = varm.betahat[1:].T if varm.withconst else varm.betahat.T
    k = ns * varm.nlag
    varm.M = np.zeros((k, k)); varm.Q = np.zeros((ns, k)); varm.G = np.zeros((k, ns))
    varm.M[:ns] = b
    if k > ns:
        varm.M[ns:, :-ns] = np.eye(k - ns)
    varm.Q[:, :ns] = np.eye(ns)
    varm.G[:ns] = np.linalg.cholesky(varm.seps)


def estimate_nonparametric(m: DFMModel, *, ctx=None, lam_constr_f=None, lam_constr_fl=None):
    """`estimate!(m, NonParametric())` -- dfm_functions.ipynb:530-543."""
    if lam_constr_f is not None or lam_constr_fl is not None:
        raise NotImplementedError("loading constraints are not supported on the HIP path")
    with _device(ctx) as ctx:
        estimate_factor(m, lam_constr=lam_constr_f, ctx=ctx)
        estimate_factor_loading(m, lam_constr=lam_constr_fl, ctx=ctx)
        m.factor_var_model.y = m.factor
        estimate_var(m.factor_var_model, ctx=ctx)
    return None


def bai_ng_criterion(ssr: float, nobs: int, T: int, r: int) -> float:
    """dfm_functions.ipynb:648-654 (ICp2 with nbar = nobs / T)."""
    nbar = nobs / T
    g = np.log(min(nbar, T)) * (nbar + T) / nobs
    return float(np.log(ssr / nobs) + r * g)


def estimate_factor_numbers(m: DFMModel, nfacs, *, ctx=None, with_aw: bool = False):
    """`estimate_factor_numbers(m, nfacs)` -- dfm_functions.ipynb:698-725: the static-factor runs for every r in
    `nfacs` go through ONE dfm_als_batch call (shared panel, r_each); Bai-Ng ICp2 per r.  Returns
    dict(bn_icp, ssr_static, tss, nobs, T, iters, factors).

    with_aw: also the `amengual_watson_test` (:734-768) the reference runs inside every static run (:716-717): per static
    count i one dfm_ols_batch (every series on [1, lags of the i factors]) and one PCA start of the residual window,
    then ALL the dynamic runs (k = 1..i for every i) in ONE dfm_als_batch call, each run on its own residual window --
    adds aw_icp / ssr_dynamic [max r, n runs] (NaN above the diagonal, the reference's `missing`).  julia/dfm_hip.jl
    estimate_factor_numbers_hip is the same sequence of calls."""
    nfacs = [int(k) for k in nfacs]
    rmax = max(nfacs)
    xdata = m.data[m.initperiod - 1:m.lastperiod, :][:, m.inclcode == 1]
    z, _ = standardize_data(xdata)
    T = z.shape[0]
    tss = float(np.nansum(z * z)); nobs = int((~np.isnan(z)).sum())
    with _device(ctx) as ctx:
        F0 = pca_start(ctx, z, rmax)                       # scores are nested: run r starts from the first r columns
        o = ctx.als_batch_host(z, np.repeat(F0[None], len(nfacs), axis=0), r_each=nfacs,
                               nt_min=m.nt_min_factor_estimation, tol=m.tol)
        out = dict(bn_icp=np.array([bai_ng_criterion(s, nobs, T, k) for s, k in zip(o["ssr"], nfacs)]),
                   ssr_static=o["ssr"].copy(), tss=tss, nobs=nobs, T=T, iters=o["iters"].copy(), factors=o["F"])
        if with_aw:
            est = m.data[:, m.inclcode == 1]
            T_all = est.shape[0]
            nlag = m.factor_var_model.nlag
            init, last = m.initperiod + 4, m.lastperiod                       # :761 (the reference hard-codes the 4)
            Tw = last - init + 1
            zs, F0s, r_each, owner, meta = [], [], [], [], []
            for col, i in enumerate(nfacs):
                fac = np.full((T_all, i), np.nan)
                fac[m.initperiod - 1:m.lastperiod] = o["F"][col][:, :i]
                x = np.column_stack([np.ones(T_all), _lagmat(fac, range(1, nlag + 1))])
                res = ctx.ols_batch_host(x, est, nt_min=x.shape[1] + m.nt_min_factor_estimation)["resid"]
                zi, _ = standardize_data(res[init - 1:last])
                Fi = np.zeros((Tw, rmax)); Fi[:, :i] = pca_start(ctx, zi, i)
                meta.append((int((~np.isnan(zi)).sum()), zi.shape[0]))
                for k in range(1, i + 1):
                    zs.append(zi); F0s.append(Fi); r_each.append(k); owner.append((k, col))
            a = ctx.als_batch_host(np.stack(zs), np.stack(F0s), r_each=r_each, nt_min=m.nt_min_factor_estimation, tol=m.tol)
            aw = np.full((rmax, len(nfacs)), np.nan); ssr_dyn = np.full((rmax, len(nfacs)), np.nan)
            for b, (k, col) in enumerate(owner):
                aw[k - 1, col] = bai_ng_criterion(a["ssr"][b], meta[col][0], meta[col][1], k)
                ssr_dyn[k - 1, col] = a["ssr"][b]
            out.update(aw_icp=aw, ssr_dynamic=ssr_dyn)
    return out


def impulse_response(varm: VARModel, shock_ids, T: int) -> np.ndarray:
    """`impulse_response(varm, shock_ids, T)` -- dfm_functions.ipynb:793-816: irf[:, t, k] = Q M^t G[:, shock_k]
    (point estimate; host arithmetic on the 16 x 16 companion, as in the reference).  The reference's three methods:
      * a vector of shock ids  -> [ny, T, len(shock_ids)]                                   (:793-799)
      * ONE shock id (a number) -> the [ny, T] matrix of that shock                         (:817-821: the reference's method
        passes an undefined `x` and six arguments to the five-argument `compute_irf_single_shock!` and cannot run; this is
        what it evidently means -- the same recursion written into a matrix; julia/dfm_hip.jl repairs it the same way)
      * "all" (the reference's `:all`) -> every column of G                                 (:822-825)
    Shock ids are 0-based here (1-based in Julia)."""
    if isinstance(shock_ids, str):
        if shock_ids != "all":
            raise ValueError("shock_ids: a shock index, a sequence of them, or 'all'")
        shock_ids = range(varm.G.shape[1])
    scalar = np.isscalar(shock_ids)
    ids = [int(s) for s in np.atleast_1d(shock_ids)]
    out = np.empty((varm.Q.shape[0], T, len(ids)))
    for k, s in enumerate(ids):
        if not 0 <= s < varm.G.shape[1]:
            raise IndexError(f"shock id {s} out of range (G has {varm.G.shape[1]} columns)")
        x = varm.G[:, s].copy()
        for t in range(T):
            out[:, t, k] = varm.Q @ x
            x = varm.M @ x
    return out[:, :, 0] if scalar else out


def bootstrap_irf_bands(varm: VARModel, H: int, ndraws: int = 10000, quantiles=(0.05, 0.16, 0.5, 0.84, 0.95),
                        seed: int = 20160415, signs=None, ctx=None, rank: int = 0, world: int = 1, gather=None):
    """Wild-bootstrap bands of the impulse responses of an estimated VARModel (BASELINE config 5; no reference
    counterpart -- the reference stops at the point estimate).  Draws, re-estimation, Cholesky, IRF recursion and
    the quantiles all run in boot.hip.  Returns dict(point [ns,H,ns], bands [len(q),ns,H,ns], draws [B,ns,H,ns]).

    Multi-GPU (one process per GPU): rank k of `world` computes the draws shard.replicate_range(ndraws, world, k)
    -- the device-drawn signs depend on the global draw index only -- and `gather` (e.g. a function wrapping
    shard.allgather_replicates) assembles the [ndraws, ...] array before the bands are taken; that all-gather is
    the path's one collective."""
    rows = np.nonzero(~np.isnan(varm.resid).any(axis=1))[0]
    if rows.size == 0:
        raise ValueError("estimate_var(varm) first")
    first = rows[0] - varm.nlag
    if first < 0 or not np.array_equal(rows, np.arange(rows[0], rows[-1] + 1)):
        raise ValueError("the VAR's estimation rows must be one contiguous block (no missing factors inside the window)")
    y = varm.y[first:rows[-1] + 1]
    resid = np.zeros_like(y)
    resid[varm.nlag:] = varm.resid[rows]
    if not varm.withconst:
        raise NotImplementedError("bootstrap_irf_bands needs a VAR with constant (the reference's default)")
    with _device(ctx) as ctx:
        from .shard import replicate_range
        lo, hi = replicate_range(int(ndraws), world, rank)
        draws = ctx.var_bootstrap_irf_host(y, varm.betahat, resid, varm.nlag, H, hi - lo, seed=seed, first_draw=lo,
                                           signs=None if signs is None else np.asarray(signs)[lo:hi])
        if world > 1:
            if gather is None:
                raise ValueError("world > 1 needs a gather function")
            draws = np.asarray(gather(draws))
        bands = ctx.quantile_bands_host(draws, np.asarray(quantiles, float))
    return dict(point=impulse_response(varm, range(varm.ns), H), bands=bands, draws=draws)


def _ar_model_inputs(m: DFMModel, through: Optional[int] = None):
    """The parametric model with AR(n_uarlag) idiosyncratic terms assembled from what the reference's own estimator leaves
    in the model (`estimate!(m)`):

        x_it = c_i + lam_i' f_t + e_it,   e_it = sum_l uar_coef[i,l] e_i,t-l + eps_it,  sd(eps_it) = uar_ser[i]   (:391-415)
        f_t  = c_f + A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t,  Var(eta_t) = seps      (factor_var_model, :444-492)

    in deviations from the VAR's mean (the reference does not keep c_i: it is re-derived as the mean residual of the
    loading regression).  Series used: included (inclcode == 1) with loadings, AR coefficients and uar_ser > 0.  Runs
    dfm_ks_pass_ar_batch (quasi-differenced observation equation, state (f_t .. f_{t-m+1}), m = max(p, n_uarlag + 1),
    nfac_u * m <= 32; likelihood conditional on the first n_uarlag window rows).  z_q ~ N(0, stationary covariance of
    the companion VAR) -- or the sample second moment of the stacked factor estimates when the VAR is not stable.
    `through` (1-based, default lastperiod): the panel x holds rows initperiod..through; everything else -- c_i, mu_f, P0 -- comes
    from the estimation window initperiod..lastperiod whatever `through` is.
    Returns (inputs dict for the library, column indices used, factor mean mu_f, series intercepts c_i)."""
    if m.nfac_o != 0:
        raise NotImplementedError("observed factors (nfac_o > 0) are not supported (non-functional in the reference too)")
    var = m.factor_var_model
    r, p, q = m.nfac_u, var.nlag, m.n_uarlag
    mm = max(p, q + 1)
    k = r * mm
    if k > 32:
        raise ValueError("nfac_u * max(n_factorlag, n_uarlag + 1) must not exceed 32 (DFM_MAX_R)")
    if np.isnan(var.betahat).any() or np.isnan(var.seps).any():
        raise ValueError("factor_var_model is not estimated: run estimate(m, NonParametric()) first")
    rows = slice(m.initperiod - 1, m.lastperiod)
    F = m.factor[rows]
    use = (m.inclcode == 1) & ~np.isnan(m.lambda_).any(axis=1) & ~np.isnan(m.uar_coef).any(axis=1) & (m.uar_ser > 0)
    cols = np.nonzero(use)[0]
    if cols.size == 0:
        raise ValueError("no series with loadings and AR coefficients: run estimate(m, NonParametric()) first")
    Y = m.data[rows][:, cols]
    lam, rho, sig2 = m.lambda_[cols], m.uar_coef[cols], m.uar_ser[cols] ** 2
    c0 = 1 if var.withconst else 0
    Avar = np.ascontiguousarray(var.betahat[c0:c0 + r * p].T)            # [A_1 .. A_p]
    c_f = var.betahat[0] if var.withconst else np.zeros(r)
    Asum = sum(Avar[:, l * r:(l + 1) * r] for l in range(p))
    mu_f = np.linalg.solve(np.eye(r) - Asum, c_f)
    c_i = np.nanmean(Y - F @ lam.T, axis=0)                              # intercept of the loading regression (:396-400)
    Yx = Y if through is None else m.data[m.initperiod - 1:through][:, cols]
    x = Yx - c_i - lam @ mu_f
    M = np.zeros((k, k)); M[:r, :r * p] = Avar
    M[r:, :k - r] = np.eye(k - r)
    Qk = np.zeros((k, k)); Qk[:r, :r] = var.seps
    if np.abs(np.linalg.eigvals(M)).max() < 0.999:
        P0 = np.linalg.solve(np.eye(k * k) - np.kron(M, M), Qk.ravel()).reshape(k, k)
    else:
        Fd = F - mu_f
        Z = np.hstack([Fd[mm - 1 - l:Fd.shape[0] - l] for l in range(mm)])
        P0 = Z.T @ Z / Z.shape[0]
    P0 = 0.5 * (P0 + P0.T) + 1e-10 * np.eye(k)
    inputs = dict(x=x, Lam=lam, sig2=sig2, rho=rho, Avar=Avar, Q=np.array(var.seps), mu0=np.zeros(k), P0=P0)
    return inputs, cols, mu_f, c_i


def smooth_factors_ar_idio(m: DFMModel, *, ctx=None):
    """Kalman-smoothed factors and Gaussian log-likelihood of the parametric model with AR(n_uarlag)
    idiosyncratic terms at the parameters the reference's own estimator leaves in the model (`_ar_model_inputs`).
    Returns dict(loglik, factor [T_all, r] (NaN outside rows initperiod + n_uarlag .. lastperiod), P [T - q, r(r+1)/2],
    series (column indices used), inputs (the arrays handed to the library, for the parity test))."""
    inputs, cols, mu_f, _ = _ar_model_inputs(m)
    r, q = m.nfac_u, m.n_uarlag
    with _device(ctx) as ctx:
        f, P, ll = ctx.ks_pass_ar_batch_host(inputs["x"][None], inputs["Lam"][None], inputs["sig2"][None], inputs["rho"][None],
                                             inputs["Avar"][None], inputs["Q"][None], inputs["mu0"][None], inputs["P0"][None])
    factor = np.full((m.T_all if hasattr(m, "T_all") else m.data.shape[0], r), np.nan)
    factor[m.initperiod - 1 + q:m.lastperiod] = f[0] + mu_f
    return dict(loglik=float(ll[0]), factor=factor, P=P[0], series=cols, inputs=inputs, mu_f=mu_f)


def _ar_lags(m: DFMModel, who):
    """q = n_uarlag, which the post-estimation entries of the AR model take in 1..4; `who` is refused otherwise."""
    q = int(m.n_uarlag)
    if not (1 <= q <= 4):
        raise ValueError(f"{who} needs 1 <= n_uarlag <= 4")
    return q


def _ar_v0(m: DFMModel, cols, c_i, Lam):
    """The variance of the q idiosyncratic terms before the first output row: the window's sample variance of Y - c_i - F lam_i."""
    win = slice(m.initperiod - 1, m.lastperiod)
    return np.nanvar(m.data[win][:, cols] - c_i - m.factor[win] @ Lam.T, axis=0)


def _bootstrap_replicates_ar(ctx, m: DFMModel, x, cols, est, nrep, seed, max_em_iter, tol_em):
    """`nrep` parametric-bootstrap panels of the AR-idiosyncratic fit `est` (the parameters dfm_em_ar_batch returned, [1, ...]),
    drawn on the device conditional on the first n_uarlag rows of the window panel x (dfm_simulate_ar_batch: replicate b = draw b
    of seed `seed`, the panel's NaN pattern, the v0 of forecast_ar_idio at the fitted model) and re-estimated from the fit where
    they lie, in one dfm_em_ar_batch_dev call."""
    torch = ctx._torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=f"cuda:{ctx.device}")
    _, _, _, c_i = _ar_model_inputs(m)                       # the intercepts of the model as the fit left it
    v0 = _ar_v0(m, cols, c_i, est["Lam"][0])
    start = {k: dev(est[k][:1]) for k in _AR_PARAM_NAMES}
    sim = ctx.simulate_ar_batch(*(start[k] for k in _AR_PARAM_NAMES), D=nrep, panel=dev(x[None]), v0=dev(v0[None]), seed=seed,
                                want_f=False)
    panels = sim["x"][0]
    new, path, iters = _em_resident(ctx.em_ar_batch, panels, start, _AR_PARAM_NAMES, nrep, max_em_iter, tol_em, False,
                                    ctx.synchronize, may_have_missing=bool(np.isnan(x).any()))
    return dict(params=new, loglik_path=path, iters=iters, panels=panels.cpu().numpy(), v0=v0,
                fit={k: np.array(est[k][:1]) for k in _AR_PARAM_NAMES})


def estimate_ar_idio(m: DFMModel, *, max_em_iter: int = 20, tol_em: float = 1e-6, nrep: int = 0, seed: int = 20160415, ctx=None):
    """JOINT estimation of the parametric model with AR(n_uarlag) idiosyncratic terms -- the
    re-estimation of `lambda`, `uar_coef`, `uar_ser` and the factor VAR that the reference's two-step estimator
    (:391-415, :444-468) never does.  Started from `estimate(m, NonParametric())` (`_ar_model_inputs`: the reference's own
    loadings, AR coefficients, innovation s.d. and VAR), iterated by ECM on the device (dfm_em_ar_batch: smoother pass of
    the quasi-differenced model, transition step, loadings | rho, rho | loadings, sig2); the series intercepts and the
    factor mean stay at their two-step values.  Mutates m IN PLACE like the reference's estimators: `lambda`, `uar_coef`,
    `uar_ser` of the series used, `factor` (smoothed, rows initperiod + n_uarlag .. lastperiod), `factor_var_model`
    (`betahat` slope rows, `seps`, `M`, `Q`, `G` through `fill_matrices`).  Returns the log-likelihood path (conditional on
    the first n_uarlag window rows; non-decreasing).
    `nrep` > 0: after the fit, `nrep` parametric-bootstrap replicates of the window panel are drawn on the device from the fitted
    model, conditional on the panel's first n_uarlag rows -- what the likelihood conditions on -- with its NaN pattern and the
    pre-sample variance v0 of `forecast_ar_idio` (dfm_simulate_ar_batch: the random stream of dfm_simsmooth_ar_batch, key `seed`,
    draw b = replicate b), and re-estimated from the fit in ONE dfm_em_ar_batch_dev call.  They land in
    `m.replicates_ar = dict(params, loglik_path, iters, panels, v0, fit)`; `params` (name -> [nrep, ...], the layout of
    `estimate_bayesian_ar_idio`'s) is what `forecast_ar_idio`, `filter_states_ar_idio`, `evaluate_forecasts_ar_idio`,
    `news_ar_idio` and `draw_paths_ar_idio` take as `params=`.  Needs 1 <= n_uarlag <= 4."""
    nrep = int(nrep)
    if nrep < 0:
        raise ValueError("nrep must be >= 0")
    if nrep and not (1 <= int(m.n_uarlag) <= 4):
        raise ValueError("bootstrap replicates (nrep > 0) need 1 <= n_uarlag <= 4")
    inputs, cols, mu_f, _ = _ar_model_inputs(m)
    var = m.factor_var_model
    r, p, q = m.nfac_u, var.nlag, m.n_uarlag
    with _device(ctx) as ctx:
        est, path, iters, f, _ = ctx.em_ar_batch_host(inputs["x"][None], inputs["Lam"][None], inputs["sig2"][None],
                                                      inputs["rho"][None], inputs["Avar"][None], inputs["Q"][None],
                                                      inputs["mu0"][None], inputs["P0"][None], max_iter=max_em_iter, tol=tol_em)
        m.lambda_[cols] = est["Lam"][0]
        m.uar_coef[cols] = est["rho"][0]
        m.uar_ser[cols] = np.sqrt(est["sig2"][0])
        m.factor[m.initperiod - 1 + q:m.lastperiod] = f[0] + mu_f
        c0 = 1 if var.withconst else 0
        A = est["Avar"][0]
        var.betahat[c0:c0 + r * p] = A.T
        if var.withconst:                                        # the factor mean is held: c_f = (I - sum A_l) mu_f
            var.betahat[0] = (np.eye(r) - sum(A[:, l * r:(l + 1) * r] for l in range(p))) @ mu_f
        var.seps = est["Q"][0]
        _fill_matrices(var)
        if nrep:
            m.replicates_ar = _bootstrap_replicates_ar(ctx, m, inputs["x"], cols, est, nrep, int(seed), max_em_iter, tol_em)
    return path[0, :int(iters[0])].copy()


def forecast_ar_idio(m: DFMModel, H: int, *, through: Optional[int] = None, params=None, quantiles=None, ctx=None) -> dict:
    """Nowcasts and H-step forecasts of the panel from the model with AR(n_uarlag) idiosyncratic terms, after
    `estimate(m, NonParametric())`, optionally followed by `estimate_ar_idio(m)` (`_ar_model_inputs`: whatever loadings, `uar_coef`,
    `uar_ser` and factor VAR the model holds).  What `forecast` gives for the parametric fit, with the idiosyncratic persistence
    kept: one to four steps ahead rho_i e_iT is often the larger part of a series' forecast.

    Parameters, the series intercepts c_i and the factor mean mu_f come from the estimation window; the state conditions on rows
    initperiod..`through` (1-based, lastperiod <= through <= m.T, default lastperiod) -- rows after lastperiod are the ragged edge
    a nowcast is for.  The q = n_uarlag idiosyncratic terms before the first output row have the window's sample variance of
    Y - c_i - F lam_i.  One dfm_forecast_ar_batch call on the GPU.  Returns a dict (data units):
      rows        1-based periods initperiod + q .. through + H (the last H are the forecast horizon)
      cols        column indices (0-based) of m.data: the series `_ar_model_inputs` used
      x           [rows, cols] observed cells as they are, every other cell E[x_ti | X] = common + idio
      x_sd        [rows, cols] 0 on observed cells, sqrt(lam_i' P_t lam_i + V_ti) elsewhere -- the two variances added, without
                  the cross-period covariance of the factor estimation error (include/dfm_hip.h; within a few per cent of exact)
      common      [rows, cols] c_i + lam_i' (mu_f + E[f_t - mu_f | X])
      idio        [rows, cols] E[e_ti | X]: the residual on an observed cell, the AR(q) smoother's mean elsewhere
      factor      [rows, r] E[f_t | X] (with the factor mean mu_f, which is returned too), factor_cov [rows, r, r] = Var[f_t | X]
      loglik      log-likelihood of rows initperiod + q .. through, conditional on the first q rows
      inputs      the arrays handed to the library (those of `_ar_model_inputs`, v0 and mean), for the parity test
    `quantiles` (needs `params`: S parameter sets on the first axis, `m.replicates_ar["params"]` of `estimate_ar_idio(nrep=...)`
    or `estimate_bayesian_ar_idio`'s): every set runs in ONE batched call on the same panel, and dfm_quantile_bands over the sets'
    horizon rows gives bands [nq, H, len(cols)] (nearest rank) -- the PARAMETER uncertainty of the point forecast only, as in
    `forecast`; the point forecast stays that of the model's own parameters.  `m` is not modified."""
    H = int(H)
    if H < 0:
        raise ValueError("H must be >= 0")
    q = _ar_lags(m, "forecast_ar_idio")
    through = _through_arg(m, through)
    if quantiles is not None and params is None:
        raise ValueError("quantile bands need parameter sets: params=m.replicates_ar['params'] of estimate_ar_idio(nrep=...)")
    if quantiles is not None and H < 1:
        raise ValueError("quantile bands need H >= 1")
    qs = _quantile_arg(quantiles)
    if qs is None and params is not None:
        raise ValueError("params serve the quantile bands: give quantiles= with them")
    inputs, cols, mu_f, c_i = _ar_model_inputs(m, through)
    sets = None if params is None else _ar_param_sets(inputs, params)
    if sets is not None and sets[0].shape[0] > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"bands need at most {_QUANTILE_MAX_DRAWS} parameter sets")
    v0 = _ar_v0(m, cols, c_i, inputs["Lam"])
    mean = c_i + inputs["Lam"] @ mu_f
    x = inputs["x"]
    with _device(ctx) as ctx:
        def run(sets, **kw):
            S = sets[0].shape[0]
            return ctx.forecast_ar_batch_host(_rep(x, S), *sets, H, v0=_rep(v0, S), mean=_rep(mean, S), sd=np.ones((S, cols.size)),
                                              **kw, may_have_missing=bool(np.isnan(x).any()))
        o = run([inputs[k][None] for k in _AR_PARAM_NAMES])
        bands = None if qs is None else _horizon_bands(ctx, run(sets, want=()), H, qs)
    out = dict(rows=np.arange(m.initperiod + q, through + H + 1), cols=cols, x=o["xhat"][0], x_sd=np.sqrt(o["xvar"][0]),
               common=o["common"][0], idio=o["idio"][0], factor=o["f"][0] + mu_f, factor_cov=_unpack(o["P"][0], m.nfac_u),
               loglik=float(o["loglik"][0]), mu_f=mu_f, inputs=dict(inputs, v0=v0, mean=mean))
    return _with_bands(out, qs, bands=bands)


def simulate_ar_idio(m: DFMModel, ndraws: int, *, seed: int = 20160415, masked: bool = True, ctx=None) -> dict:
    """`ndraws` panels simulated from the model with AR(n_uarlag) idiosyncratic terms the model holds (`_ar_model_inputs`, as
    `forecast_ar_idio`), over the estimation window: what `simulate` is for the parametric fit.  One dfm_simulate_ar_batch call on
    the GPU.  `masked` (default): the draws are conditional on the window's first q = n_uarlag rows, which they repeat, and carry
    the window's NaN pattern -- the panels a bootstrap of `estimate_ar_idio` re-estimates; masked=False: every cell of every row is
    simulated, the q idiosyncratic terms before row initperiod + q with the variance v0 of `forecast_ar_idio`.  Returns a dict:
      rows        1-based periods initperiod .. lastperiod
      cols        column indices (0-based) of m.data: the series `_ar_model_inputs` used
      x           [ndraws, rows, cols] data units
      factor      [ndraws, rows from initperiod + q, r] the simulated factor paths, with the factor mean mu_f
    `m` is not modified."""
    ndraws = int(ndraws)
    if ndraws < 1:
        raise ValueError("ndraws must be >= 1")
    q = _ar_lags(m, "simulate_ar_idio")
    inputs, cols, mu_f, c_i = _ar_model_inputs(m)
    if inputs["x"].shape[0] <= q:
        raise ValueError("the window must be longer than n_uarlag")
    v0 = _ar_v0(m, cols, c_i, inputs["Lam"])
    mean = c_i + inputs["Lam"] @ mu_f
    with _device(ctx) as ctx:
        o = ctx.simulate_ar_batch_host(*(inputs[k][None] for k in _AR_PARAM_NAMES), ndraws, T=inputs["x"].shape[0],
                                       panel=inputs["x"][None] if masked else None, v0=v0[None], seed=int(seed))
    return dict(rows=np.arange(m.initperiod, m.lastperiod + 1), cols=cols, x=o["x"][0] + mean, factor=o["f"][0] + mu_f)


def draw_paths_ar_idio(m: DFMModel, ndraws: int, H: int = 0, *, through: Optional[int] = None, seed: int = 20160415,
                       first_draw: int = 0, quantiles=None, params=None, ctx=None) -> dict:
    """Joint draws of the factor path and of the panel's missing and future cells from the model with AR(n_uarlag) idiosyncratic
    terms: the counterpart of `forecast_ar_idio`, which gives the marginal moments only -- a fan chart of a series, the probability
    of an event over several cells.  The AR model's horizon errors are strongly correlated along time; the draws carry that.

    Model, window, `through`, v0 and the data units exactly as `forecast_ar_idio`.  One dfm_simsmooth_ar_batch call on the GPU
    (include/dfm_hip.h: a simulation smoother; the random stream is a pure function of `seed` and the draw's index first_draw + d,
    so draws [k, k + n) equal those of a call with first_draw = k).  The draws are independent, with mean `forecast_ar_idio`'s x
    and the joint covariance of its error: exact posterior draws when the only missing cells are the ragged edge and the horizon;
    with interior gaps they carry the pass's quasi-differencing convention.  Returns a dict (data units):
      rows        1-based periods initperiod + q .. through + H
      cols        column indices (0-based) of m.data: the series `_ar_model_inputs` used
      factor      [ndraws, rows, r] factor paths (with the factor mean mu_f)
      x           [ndraws, rows, cols] observed cells as they are, every other cell drawn
      x_sd        [rows, cols] sample standard deviation of the draws (ndraws >= 2, else 0): 0 on observed cells, elsewhere the
                  companion of `forecast_ar_idio`'s x_sd that includes the cross-period covariance of the factor estimation error
      bands       [nq, rows, cols] pointwise nearest-rank quantiles of x (dfm_quantile_bands), with `quantiles`
    `params` (default None: the model's own parameters): the `params` of `estimate_bayesian_ar_idio` -- dict(Lam, sig2, rho, Avar,
    Q, mu0, P0) with S parameter sets on the first axis.  Every set is one replicate of the same dfm_simsmooth_ar_batch call with
    `ndraws` draws each, and factor / x hold S x ndraws draws (set-major), so x_sd and bands carry the parameter uncertainty as
    well.  The data units (c_i, mu_f) and v0 stay those of the model.
    `m` is not modified."""
    ndraws, H, first_draw = int(ndraws), int(H), int(first_draw)
    if ndraws < 1:
        raise ValueError("ndraws must be >= 1")
    if H < 0:
        raise ValueError("H must be >= 0")
    if first_draw < 0:
        raise ValueError("first_draw must be >= 0")
    q = _ar_lags(m, "draw_paths_ar_idio")
    qs = _quantile_arg(quantiles, closed=True)
    if qs is not None and ndraws > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"bands need ndraws <= {_QUANTILE_MAX_DRAWS}")
    through = _through_arg(m, through)
    inputs, cols, mu_f, c_i = _ar_model_inputs(m, through)
    v0 = _ar_v0(m, cols, c_i, inputs["Lam"])
    mean = c_i + inputs["Lam"] @ mu_f
    x = inputs["x"]
    sets = [inputs[k][None] for k in _AR_PARAM_NAMES] if params is None else _ar_param_sets(inputs, params)
    S = sets[0].shape[0]
    if params is not None and qs is not None and S * ndraws > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"bands need S x ndraws <= {_QUANTILE_MAX_DRAWS}")
    total = S * ndraws
    kw = dict(v0=_rep(v0, S), seed=int(seed), first_draw=first_draw, mean=_rep(mean, S), sd=np.ones((S, cols.size)),
              may_have_missing=bool(np.isnan(x).any()))
    with _device(ctx) as ctx:                       # the information form inverts Q: as draw_paths, retry in covariance form
        o = _numeric_retry(lambda **sq: ctx.simsmooth_ar_batch_host(_rep(x, S), *sets, ndraws, H, **sq, **kw))
        xd, fd = _pooled(o["x"]), _pooled(o["f"])
        xr = m.data[m.initperiod - 1 + q:through][:, cols]              # observed cells: the data itself, not mean + z
        obs = ~np.isnan(xr)
        xd[:, :xr.shape[0], :][:, obs] = xr[obs]
        bands = None if qs is None else _flat_bands(ctx, xd, qs)
    x_sd = xd.std(axis=0, ddof=1) if total > 1 else np.zeros(xd.shape[1:])
    x_sd[:xr.shape[0]][obs] = 0.0
    out = dict(rows=np.arange(m.initperiod + q, through + H + 1), cols=cols, factor=fd + mu_f, x=xd, x_sd=x_sd,
               mu_f=mu_f, inputs=dict(inputs, v0=v0, mean=mean))
    return _with_bands(out, qs, bands=bands)


def estimate_bayesian_ar_idio(m: DFMModel, ndraws: int, *, chains: int = 4, burn: int = 500, thin: int = 1, prior=None,
                              seed: int = 20160415, keep_factors: bool = False, quantiles=None, ctx=None) -> dict:
    """Bayesian estimation of the model with AR(n_uarlag) idiosyncratic terms by the Gibbs sampler of include/dfm_hip.h
    (dfm_gibbs_ar_batch), after `estimate(m, NonParametric())`, optionally followed by `estimate_ar_idio(m)`: `chains` independent
    chains, all started at the parameters the model holds (`_ar_model_inputs`), run as one batch on the GPU on the window rows
    initperiod..lastperiod.  Each chain runs `burn` sweeps and then keeps `ndraws` sweeps, one in `thin`.  `prior`: a dict that
    overrides entries of bayes.default_prior_ar(r) (tau_lam, nu_R, s_R, tau_rho, tau_A, nu_Q, s_Q, A0).  mu0 and P0 stay at their
    start values, and so does the series mean  mean_i = c_i + lam_i' mu_f  (c_i the intercept of the loading regression, mu_f the
    factor VAR's mean): it is FIXED at the start values, the sampler draws deviations from it.  The series block conditions on the
    first q output rows, the VAR block on the first p drawn rows; A is not truncated to the stationary region, rho_i is.
    No rotation or scale normalisation is applied: rho, sig2, the common component and forecasts are identified, Lam, A and Q one
    by one are not.  Returns a dict:
      params        dict(Lam, sig2, rho, Avar, Q, mu0, P0), chains x ndraws flattened on the first axis (chain-major): hand it to
                    `draw_paths_ar_idio(m, ..., params=out["params"])` for fan charts with parameter uncertainty
      rows, cols    1-based periods initperiod + q .. lastperiod, column indices (0-based) of m.data
      sig2_mean [N], rho_mean [N, q], persistence_mean [N] (sum_l rho_il), common_mean [rows, N] (mean_i + lam_i' f_t)
      quantiles, sig2_bands [nq, N], persistence_bands [nq, N], common_bands [nq, rows, N]    with `quantiles`
      rhat_sig2 [N], rhat_persistence [N], rhat_common [N]    split-R-hat across the chains (common: of the last period)
      factor        [chains x ndraws, rows, r] (with the factor mean mu_f) with keep_factors
      prior, chains, ndraws, mu_f
    `m` is not modified."""
    from . import bayes
    ndraws, chains, burn, thin = int(ndraws), int(chains), int(burn), int(thin)
    if ndraws < 1 or chains < 1 or burn < 0 or thin < 1:
        raise ValueError("ndraws >= 1, chains >= 1, burn >= 0 and thin >= 1 are required")
    q = _ar_lags(m, "estimate_bayesian_ar_idio")
    if m.nfac_u > 8:
        raise ValueError("estimate_bayesian_ar_idio needs nfac_u <= 8")
    qs = _quantile_arg(quantiles)
    inputs, cols, mu_f, c_i = _ar_model_inputs(m)
    x = inputs["x"]
    r = inputs["Lam"].shape[1]
    p = inputs["Avar"].shape[1] // r
    if x.shape[0] - q <= p:
        raise ValueError("the window is not longer than n_uarlag plus the number of factor lags")
    pr = bayes.check_prior_ar(prior, r, p, chains)
    mean = c_i + inputs["Lam"] @ mu_f
    keep = ("Lam", "sig2", "rho", "A", "Q", "f")
    d = _gibbs_chains(ctx, "gibbs_ar_batch_host", x, [inputs[k] for k in _AR_PARAM_NAMES], pr, chains, ndraws, burn, thin, seed, keep)
    K = chains * ndraws
    params = dict(Lam=_pooled(d["Lam"]), sig2=_pooled(d["sig2"]), rho=_pooled(d["rho"]), Avar=_pooled(d["A"]), Q=_pooled(d["Q"]),
                  mu0=_rep(inputs["mu0"], K), P0=_rep(inputs["P0"], K))
    stats = dict(sig2=d["sig2"], rho=d["rho"], persistence=d["rho"].sum(axis=3))        # [chains, ndraws, N (, q)]
    return _bayes_summary(d, params, np.arange(m.initperiod + q, m.lastperiod + 1), cols, stats, ("sig2", "persistence"), mean, 1.0,
                          pr, qs, keep_factors, mu_f=mu_f)


_AR_PARAM_NAMES = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


def _ar_param_sets(inputs, params):
    """`params` (name -> [S, ...] in the layout of _AR_PARAM_NAMES) checked against the model's own shapes: the S sets as arrays."""
    lost = [k for k in _AR_PARAM_NAMES if k not in params]
    if lost:
        raise ValueError(f"params lacks {lost}")
    sets = [np.ascontiguousarray(params[k], dtype=np.float64) for k in _AR_PARAM_NAMES]
    S = sets[0].shape[0] if sets[0].ndim == 3 else 0
    for k, a in zip(_AR_PARAM_NAMES, sets):
        if S < 1 or a.shape != (S,) + inputs[k].shape:
            raise ValueError(f"params[{k!r}] must be [S, ...] with the model's own shape {inputs[k].shape} behind S >= 1")
    return sets


def _filter_ar_setup(m: DFMModel, through, params, who):
    """The checks and inputs filter_states_ar_idio and evaluate_forecasts_ar_idio share (no device is touched): q, through, the
    panel, the parameter sets [S, ...] (the model's own as one set without `params`), cols, mu_f and the data-unit mean."""
    q = _ar_lags(m, who)
    through = _through_arg(m, through)
    inputs, cols, mu_f, c_i = _ar_model_inputs(m, through)
    sets = [inputs[k][None] for k in _AR_PARAM_NAMES] if params is None else _ar_param_sets(inputs, params)
    mean = c_i + inputs["Lam"] @ mu_f
    return q, through, inputs, sets, cols, mu_f, mean


def filter_states_ar_idio(m: DFMModel, *, through: Optional[int] = None, params=None, ctx=None) -> dict:
    """What the model with AR(n_uarlag) idiosyncratic terms knew at every period: the Kalman filter's predicted and filtered
    factors, the per-period log-likelihood and the one-step prediction errors of the panel -- the diagnostics of the fit that
    `forecast_ar_idio` forecasts from.  Inputs, window, `through` and the data units (mean_i = c_i + lam_i' mu_f, sd = 1) exactly
    as `forecast_ar_idio`; the parameters are held fixed over the sample.  One dfm_filter_ar_batch call on the GPU.  Returns a dict:
      rows            1-based periods initperiod + q .. through
      cols            column indices (0-based) of m.data: the series `_ar_model_inputs` used
      factor_pred     [rows, r] E[f_t | rows before t] (with the factor mean mu_f), factor_pred_cov [rows, r, r] its variance
      factor_filt     [rows, r] E[f_t | rows up to t],  factor_filt_cov [rows, r, r]
      state_pred, state_filt   [rows, r m] the whole state (f_t, .., f_{t-m+1}), m = max(p, q + 1), in deviations from mu_f
      loglik_t        [rows] log density of each row's observed quasi-differences given the rows before it; loglik their sum, the
                      log-likelihood of `forecast_ar_idio` (conditional on the first q rows)
      x_pred          [rows, cols] one-step prediction of every cell whose q lags are observed (NaN elsewhere), data units
      error           [rows, cols] x - x_pred, NaN where the cell or one of its lags is missing
      error_std       [rows, cols] the standardised innovation (mean 0, variance 1 under the model), NaN likewise
    `params` (default None: the model's own parameters): ONE parameter set in the layout of `estimate_bayesian_ar_idio`'s `params`
    (S = 1 on the first axis).  `m` is not modified."""
    q, through, inputs, sets, cols, mu_f, mean = _filter_ar_setup(m, through, params, "filter_states_ar_idio")
    if sets[0].shape[0] != 1:
        raise ValueError("filter_states_ar_idio takes one parameter set (S = 1); evaluate_forecasts_ar_idio takes several")
    x = inputs["x"]
    want = ("z_pred", "P_pred", "z_filt", "P_filt", "loglik_t", "xpred", "verr", "vstd")
    with _device(ctx) as ctx:
        o = ctx.filter_ar_batch_host(x[None], *sets, H=0, mean=mean[None], sd=np.ones((1, cols.size)), want=want,
                                     may_have_missing=bool(np.isnan(x).any()))
    r = m.nfac_u
    k = o["z_pred"].shape[2]
    Pp, Pf = _unpack(o["P_pred"][0], k), _unpack(o["P_filt"][0], k)
    return dict(rows=np.arange(m.initperiod + q, through + 1), cols=cols, factor_pred=o["z_pred"][0][:, :r] + mu_f,
                factor_pred_cov=Pp[:, :r, :r], factor_filt=o["z_filt"][0][:, :r] + mu_f, factor_filt_cov=Pf[:, :r, :r],
                state_pred=o["z_pred"][0], state_filt=o["z_filt"][0], loglik_t=o["loglik_t"][0],
                loglik=float(o["loglik_t"][0].sum()), x_pred=o["xpred"][0], error=o["verr"][0], error_std=o["vstd"][0], mu_f=mu_f,
                inputs=dict(inputs, mean=mean))


def evaluate_forecasts_ar_idio(m: DFMModel, H: int, *, first_origin: Optional[int] = None, through: Optional[int] = None,
                               params=None, quantiles=None, ctx=None) -> dict:
    """The pseudo-out-of-sample record of the model with AR(n_uarlag) idiosyncratic terms: the h-step forecast error of every
    series at every origin, h = 1..H, with the fit held fixed, summarised per horizon and series -- and beside it the record of
    the factor-only forecast from the same filtered state on the same origins, so that `gain` says what the idiosyncratic
    persistence buys.  Inputs, window, `through` and the data units as `forecast_ar_idio`.  Origins are the 1-based periods
    first_origin .. through - h (default first_origin: the middle of the rows initperiod + q .. through) at which the series' last
    q cells and its target cell are observed; the forecast made at origin t uses rows initperiod..t only.  One dfm_filter_ar_batch
    call on the GPU.  Returns a dict:
      horizons     1 .. H
      cols         column indices (0-based) of m.data: the series `_ar_model_inputs` used
      msfe         [H, cols] mean squared forecast error, NaN where no origin qualifies;  rmsfe its square root
      msfe_common  [H, cols] the same of the factor-only forecast c_i + lam_i' f_{t+h|t}
      gain         [H, cols] msfe / msfe_common (< 1: the idiosyncratic term helps)
      relative     [H, cols] msfe over the MSFE of the unconditional-mean forecast on the same cells (< 1: the model helps)
      count        [H, cols] origins averaged
    `params`: the `params` of `estimate_bayesian_ar_idio` -- S parameter sets on the first axis, run as S replicates of the one
    call; the record above is then that of the first set, and with `quantiles` (needs `params`: `estimate_ar_idio` has no
    replicates) bands [nq, H, cols] of msfe and gain_bands of gain over the sets (dfm_quantile_bands).  `m` is not modified."""
    H = int(H)
    if H < 1:
        raise ValueError("H must be >= 1")
    if quantiles is not None and params is None:
        raise ValueError("quantile bands need parameter sets: params=estimate_bayesian_ar_idio(...)['params']")
    qs = _quantile_arg(quantiles)
    q, through, inputs, sets, cols, mu_f, mean = _filter_ar_setup(m, through, params, "evaluate_forecasts_ar_idio")
    first = m.initperiod + q
    rows = through - first + 1
    first_origin = first + rows // 2 if first_origin is None else int(first_origin)
    if not (first <= first_origin <= through):
        raise ValueError(f"first_origin must lie in initperiod + n_uarlag..through ({first}..{through})")
    S = sets[0].shape[0]
    if qs is not None and S > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"bands need at most {_QUANTILE_MAX_DRAWS} parameter sets")
    x = inputs["x"]
    with _device(ctx) as ctx:
        o = ctx.filter_ar_batch_host(_rep(x, S), *sets, H=H, t0=first_origin - m.initperiod, mean=_rep(mean, S),
                                     sd=np.ones((S, cols.size)), want=("msfe", "msfe_common", "msfe0", "cnt"),
                                     may_have_missing=bool(np.isnan(x).any()))
        bands = gbands = None
        if qs is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                g = o["msfe"] / o["msfe_common"]
            bands, gbands = _flat_bands(ctx, o["msfe"], qs), _flat_bands(ctx, g, qs)
    msfe, msfec, msfe0 = o["msfe"][0], o["msfe_common"][0], o["msfe0"][0]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dict(horizons=np.arange(1, H + 1), cols=cols, msfe=msfe, rmsfe=np.sqrt(msfe), msfe_common=msfec, gain=msfe / msfec,
                   relative=msfe / msfe0, count=o["cnt"][0])
    return _with_bands(out, qs, bands=bands, gain_bands=gbands)


def news_ar_idio(m: DFMModel, old, new, targets, *, groups=None, params=None, quantiles=None, ctx=None) -> dict:
    """News decomposition of the revision of nowcasts / forecasts between two data vintages from the model with AR(n_uarlag)
    idiosyncratic terms: what `news` gives for the parametric fit, with the effect of a release on its OWN series' nowcast through
    the idiosyncratic persistence kept.  After `estimate(m, NonParametric())`, optionally `estimate_ar_idio(m)`.

    `old` / `new` / `targets` / `groups` as in `news`; units, v0 and mean as in `forecast_ar_idio`; parameters, c_i and mu_f come from
    the estimation window, the vintages cover rows initperiod .. their last row.  The vintages must be EDGE-SHAPED on the series
    used: each series observed on window rows 0 .. L with no gap, L >= 2 n_uarlag - 1 in old, old's cells a subset of new's.  Any
    other pattern is a ValueError that names the first offending column and the condition it breaks (drop that series, or trim the
    rows): with an interior gap the decomposition would not add up.  The first n_uarlag window rows are
    conditioning values: a target there is refused, a revision there moves y_rev - y_old and has no weight.
    `params`: the dict of `estimate_bayesian_ar_idio` (S parameter sets); each runs as one replicate of the same
    dfm_news_ar_batch call, behind the point estimate, and with `quantiles` nearest-rank bands over them give impact_bands
    [nq, G, cols] and revision_bands [nq, G].  Returns the keys of `news` (data units) with rows = initperiod + n_uarlag .. the
    last row of the vintages, and inputs (the arrays handed to the library: old, new, the parameters, v0, mean, sd, targets).
    `m` is not modified."""
    from . import news_ar as _na
    q = _ar_lags(m, "news_ar_idio")
    xo, xn, last = _vintages(m, old, new)
    tg = _target_list(targets)
    inputs, cols, mu_f, c_i = _ar_model_inputs(m)
    pos = {int(c): j for j, c in enumerate(cols)}
    pairs = _news_targets(m, tg, pos, "the model uses", q)
    gsum = _news_groups(groups, pos, "the model uses")
    sets = [inputs[k][None] for k in _AR_PARAM_NAMES]
    if params is not None:                          # replicate 0: the point estimate
        sets = [np.concatenate([a, b]) for a, b in zip(sets, _ar_param_sets(inputs, params))]
    qs = _quantile_arg(quantiles, (params is None, "quantile bands need parameter sets: params=estimate_bayesian_ar_idio(m, ...)['params']"))
    if qs is not None and sets[0].shape[0] - 1 > _QUANTILE_MAX_DRAWS:
        raise ValueError(f"bands need at most {_QUANTILE_MAX_DRAWS} parameter sets")
    mean = c_i + inputs["Lam"] @ mu_f
    zo, zn = xo[m.initperiod - 1:, cols] - mean, xn[m.initperiod - 1:, cols] - mean
    _na.check_args(zn.shape[0], q, pairs)
    why = _na.edge_shape_error(zo, zn, q, cols=cols)
    if why is not None:
        raise ValueError("vintage: " + why)
    v0 = _ar_v0(m, cols, c_i, inputs["Lam"])
    B = sets[0].shape[0]
    sd = np.ones(cols.size)
    o, bands = _news_call(ctx, "news_ar_batch_host", (_rep(zo, B), _rep(zn, B), *sets, pairs),
                          dict(v0=_rep(v0, B), mean=_rep(mean, B), sd=_rep(sd, B), may_have_missing=bool(np.isnan(zn).any())), qs)
    extra = dict(inputs=dict({k: a[0] for k, a in zip(_AR_PARAM_NAMES, sets)}, old=zo, new=zn, v0=v0, mean=mean, sd=sd, targets=pairs))
    return _news_result(o, np.arange(m.initperiod + q, last + 1), cols, extra, gsum, qs, bands)


def amengual_watson_test(m: DFMModel, nper: int = 4, *, ctx=None):
    """`amengual_watson_test(m, nper)` -- dfm_functions.ipynb:734-768: the number of DYNAMIC factors.  Every
    included series is regressed on [1, lags 1..p of the r estimated static factors], p = the factor VAR's
    `nlag` (:737, :741), over all rows of the data (one dfm_ols_batch call, 1 + p r <= 64 regressors); the ALS
    estimator is then run on the residual panel for k = 1..r dynamic factors over rows initperiod + 4 .. lastperiod
    (:761 -- the reference hard-codes the 4 and never reads its `nper` argument; kept for signature
    parity and ignored here too), one dfm_als_batch call, r runs on a shared panel.  `m.factor` must hold the
    static factors (estimate_factor first).  Returns (aw_icp [r], ssr [r])."""
    r = m.nfac_t
    est = m.data[:, m.inclcode == 1]
    T_all, ns = est.shape
    nlag = m.factor_var_model.nlag
    x = np.column_stack([np.ones(T_all), _lagmat(m.factor, range(1, nlag + 1))])
    with _device(ctx) as ctx:
        # the reference keeps a series when it has at least nt_min rows MORE than regressors (:744)
        o = ctx.ols_batch_host(x, est, nt_min=x.shape[1] + m.nt_min_factor_estimation)
        res = o["resid"]                                                   # NaN where a row was not used
        init, last = m.initperiod + 4, m.lastperiod
        z, _ = standardize_data(res[init - 1:last])
        T = z.shape[0]
        nobs = int((~np.isnan(z)).sum())
        F0 = pca_start(ctx, z, r)
        a = ctx.als_batch_host(z, np.repeat(F0[None], r, axis=0), r_each=np.arange(1, r + 1),
                               nt_min=m.nt_min_factor_estimation, tol=m.tol)
    aw = np.array([bai_ng_criterion(s, nobs, T, k + 1) for k, s in enumerate(a["ssr"])])
    return aw, a["ssr"].copy()


# ============================================================================= structural breaks
def break_tests(m: DFMModel, T_break: int, ccut: float = 0.15, q: int = 6, min_obs: int = 80, *, ctx=None):
    """Chow statistic at `T_break` and HAC QLR statistic of every series of `m.data` regressed on the estimated
    factors -- the loop of the driver's Table 4 (Stock_Watson.ipynb:1085-1098) over `compute_chow` / `compute_qlr`
    (dfm_functions.ipynb:891-902, 1019-1047), all (series x break date x bandwidth) problems in ONE dfm_chow_batch
    call.  As in the driver, a series takes part when it has at least `min_obs` observations before and after
    row `T_break` (1-based, inclusive), regressions run on the complete cases of [y X], and the break dates index
    the complete-case rows.  Returns (chow [ns], qlr [ns]) with NaN for the series left out."""
    X = m.factor
    ns = m.data.shape[1]
    chow = np.full(ns, np.nan); qlr = np.full(ns, np.nan)
    ys, Xs, who = [], [], []
    for i in range(ns):
        y = m.data[:, i]
        if (~np.isnan(y[:T_break])).sum() >= min_obs and (~np.isnan(y[T_break:])).sum() >= min_obs:
            ok = ~np.isnan(y) & ~np.isnan(X).any(axis=1)
            ys.append(y[ok]); Xs.append(X[ok]); who.append(i)
    if not who:
        return chow, qlr
    ps, pb, pq, tag = [], [], [], []
    for s, yv in enumerate(ys):
        T = len(yv)
        ps.append(s); pb.append(T_break); pq.append(q); tag.append(0)                 # the Chow test of the driver
        n1 = int(np.floor(ccut * T))
        for tb in range(n1, T - n1 + 1):                                               # compute_qlr's HAC leg
            ps.append(s); pb.append(tb); pq.append(q); tag.append(1)
    with _device(ctx) as ctx:
        stat = ctx.chow_batch_host(ys, Xs, ps, pb, pq)
    ps = np.asarray(ps); tag = np.asarray(tag)
    for s, i in enumerate(who):
        sel = ps == s
        chow[i] = stat[sel & (tag == 0)][0]
        qlr[i] = stat[sel & (tag == 1)].max()
    return chow, qlr
