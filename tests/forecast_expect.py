"""Expectation model of dfm_forecast_batch (include/dfm_hip.h) on the CPU: the oracle's smoother pass over the panel with H
all-missing rows appended (the smoothed moments of those rows are the forecast moments), then the cell formulas of the header.
Shared by tests/test_forecast_cpu.py (checked against the closed-form tail) and tests/test_gpu_forecast.py."""
import numpy as np

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo


def expect(x, Lam, R, A, Q, mu0, P0, H, p=1, mean=None, sd=None):
    """One replicate: x [T, N] (NaN = missing), A = [A_1 .. A_p] (r, r p).  Returns dict(xhat, xvar, common [T+H, N],
    f [T+H, r], P [T+H, r(r+1)/2] packed lower, Pfull [T+H, r, r], loglik)."""
    T, N = x.shape
    r = Lam.shape[1]
    xp = np.vstack([x, np.full((H, N), np.nan)])
    if p == 1:
        out = ko.kfs_pass(xp, Lam, R, A, Q, mu0, P0, lag_one=False)
    else:
        out = vo.kfs_pass_varp(xp, Lam, R, A, Q, mu0, P0, p)
    f = out["f_smooth"][:, :r]
    P = out["P_smooth"][:, :r, :r]
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    m = f @ Lam.T
    quad = np.einsum("ij,tjk,ik->ti", Lam, P, Lam)
    obs = ~np.isnan(xp)
    common = m if mean is None else mu + s * m
    xobs = xp if mean is None else mu + s * xp
    xhat = np.where(obs, xobs, common)
    xvar = np.where(obs, 0.0, s * s * (quad + R))
    return dict(xhat=xhat, xvar=xvar, common=common, f=f, P=ko.pack_sym(P), Pfull=P, loglik=out["loglik"])


def closed_form_tail(fT, PT, A, Q, H):
    """f_{T+h|T} = A f_{T+h-1|T}, P_{T+h|T} = A P A' + Q for h = 1..H (VAR(1) or a companion matrix)."""
    fs, Ps = [], []
    f, P = fT, PT
    for _ in range(H):
        f = A @ f
        P = A @ P @ A.T + Q
        fs.append(f); Ps.append(P)
    return np.array(fs).reshape(H, -1), np.array(Ps).reshape(H, len(fT), len(fT))
