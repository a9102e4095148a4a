"""CPU tests of the news decomposition's contract (include/dfm_hip.h dfm_news_batch, api.news): the C-ABI's argument check
without a handle, api.news' refusals before any device work, and the expectation model the GPU tests use (tests/news_expect.py).
That model builds the weights from one smoother pass over a covariance panel; here every output is recomputed by plain Gaussian
conditioning on the joint vector of every cell -- the three conditional means, the news, and the news weights of Banbura and
Modugno as Cov(y, I) Var(I)^-1 -- with no use of the lemma that links the two."""
import ctypes

import numpy as np
import pytest

from oracle import varp_oracle as vo
from tests.news_expect import expect, horizon


def test_news_without_a_handle_is_dfm_e_null():
    from dynamic_factor_models_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    tg = (ctypes.c_int * 2)(0, 0)
    tp = ctypes.cast(tg, ctypes.c_void_p)
    for fn in (lib.dfm_news_batch, lib.dfm_news_batch_dev):
        rc = fn(None, 1, 4, 3, 1, 1, *([ptr] * 8), None, None, 1, tp, tp, ptr, ptr, None, None, 0)
        assert rc == -3


# ----------------------------------------------------------------------------- brute force
def _joint(Lam, R, A, Q, mu0, P0, p, rows):
    """Mean and covariance of every cell of rows 0 .. rows-1 (row t holds f_{t+1}), built from the innovations: the stacked
    companion states z_0 .. z_rows are a linear map of (z_0, eta_1 .. eta_rows)."""
    N, r = Lam.shape
    k = r * p
    M, Qk = vo.companion(A, Q, p)
    n = (rows + 1) * k
    L = np.zeros((n, n))                                          # z_t = M^t z_0 + sum_u M^(t-u) eta_u
    for t in range(rows + 1):
        for u in range(t + 1):
            L[t * k:(t + 1) * k, u * k:(u + 1) * k] = np.linalg.matrix_power(M, t - u)
    D = np.zeros((n, n))
    D[:k, :k] = P0
    for u in range(1, rows + 1):
        D[u * k:(u + 1) * k, u * k:(u + 1) * k] = Qk
    mz = L[:, :k] @ mu0
    Sz = L @ D @ L.T
    Sel = np.zeros((rows * N, n))                                 # x_ti = lam_i' f_{t+1} + e_ti
    for t in range(rows):
        Sel[t * N:(t + 1) * N, (t + 1) * k:(t + 1) * k + r] = Lam
    return Sel @ mz, Sel @ Sz @ Sel.T + np.diag(np.tile(R, rows))


def _cond_mean(m, C, obs, vals):
    """E[all cells | cells obs = vals]."""
    o = np.nonzero(obs)[0]
    if o.size == 0:
        return m.copy()
    return m + C[:, o] @ np.linalg.solve(C[np.ix_(o, o)], vals[o] - m[o])


def brute(old, new, Lam, R, A, Q, mu0, P0, targets, p, mean=None, sd=None):
    T, N = new.shape
    rows = T + horizon(targets, T)
    m, C = _joint(Lam, R, A, Q, mu0, P0, p, rows)
    mu = np.zeros(N) if mean is None else np.asarray(mean, float)
    s = np.ones(N) if sd is None else np.asarray(sd, float)
    pad = lambda x: np.vstack([x, np.full((rows - T, N), np.nan)]).ravel()
    xo, xn = pad(old), pad(new)
    Oo, On = ~np.isnan(xo), ~np.isnan(xn)
    xr = np.where(Oo, xn, np.nan)
    Eold, Erev, Enew = _cond_mean(m, C, Oo, xo), _cond_mean(m, C, Oo, xr), _cond_mean(m, C, On, xn)
    col = np.tile(np.arange(N), rows)
    unit = lambda v: mu[col] + s[col] * v
    tid = [int(t) * N + int(i) for t, i in targets]
    yhat = np.array([[unit(E)[j] for j in tid] for E in (Eold, Erev, Enew)])
    nw = On & ~Oo
    news = np.where(nw, s[col] * (np.nan_to_num(xn) - Erev), 0.0)
    o, n, a = np.nonzero(Oo)[0], np.nonzero(nw)[0], np.nonzero(On)[0]
    weight, bm = [], []
    for j in tid:
        w = np.zeros(rows * N)                                    # d E[y | Omega_new] / d x = C_ya C_aa^-1
        w[a] = np.linalg.solve(C[np.ix_(a, a)], C[a, j]) * s[col[j]] / s[col[a]]
        weight.append(w.reshape(rows, N)[:T])
        if n.size:                                                # Cov(y, I) Var(I)^-1 (standardised), to data units
            K = C[np.ix_(n, o)] @ np.linalg.inv(C[np.ix_(o, o)]) if o.size else np.zeros((n.size, 0))
            cov_yi = C[j, n] - (K @ C[o, j] if o.size else 0.0)
            var_i = C[np.ix_(n, n)] - (K @ C[np.ix_(o, n)] if o.size else 0.0)
            bm.append(np.linalg.solve(var_i, cov_yi) * s[col[j]] / s[col[n]])
        else:
            bm.append(np.zeros(0))
    return dict(yhat=yhat, news=news.reshape(rows, N)[:T], weight=np.array(weight), bm=bm, news_cells=n)


# ----------------------------------------------------------------------------- cases
def _params(N, r, p, seed, singular=False):
    rng = np.random.default_rng(seed)
    k = r * p
    Lam = rng.standard_normal((N, r))
    R = rng.uniform(0.3, 1.2, N)
    A = np.hstack([np.diag(rng.uniform(-0.5, 0.7, r)) * 0.6 ** l + 0.05 * rng.standard_normal((r, r)) for l in range(p)])
    B = rng.standard_normal((r, r))
    Q = B @ B.T / r + 0.2 * np.eye(r)
    if singular:
        v = rng.standard_normal((r, r - 1))
        Q = v @ v.T
    mu0 = rng.standard_normal(k)
    C = rng.standard_normal((k, k))
    P0 = C @ C.T / k + 0.5 * np.eye(k)
    return Lam, R, A, Q, mu0, P0


def _vintages(T, N, seed):
    """old: missing cells and the last two rows not yet released; new: the last two rows partly released, one old cell revised,
    one old gap filled."""
    rng = np.random.default_rng(seed)
    new = rng.standard_normal((T, N))
    new[rng.random((T, N)) < 0.15] = np.nan
    new[T - 1, : N // 2] = np.nan                                 # the ragged edge of the new vintage
    old = new.copy()
    old[T - 2:, :] = np.nan                                       # periods the old vintage did not have
    gap = np.argwhere(~np.isnan(new[: T - 2]))[0]
    old[gap[0], gap[1]] = np.nan                                  # a gap of the old vintage filled by the new one
    rv = np.argwhere(~np.isnan(old))[-1]
    new[rv[0], rv[1]] += 0.7                                      # a revised old cell
    return old, new


def _close(a, b, tol, what):
    scale = max(1.0, float(np.abs(b).max())) if np.size(b) else 1.0
    err = float(np.abs(a - b).max()) if np.size(b) else 0.0
    assert err <= tol * scale, f"{what}: {err:.3e}"


def _check(old, new, prm, targets, p, mean=None, sd=None):
    got = expect(old, new, *prm, targets, p=p, mean=mean, sd=sd)
    want = brute(old, new, *prm, targets, p, mean=mean, sd=sd)
    _close(got["yhat"], want["yhat"], 1e-10, "yhat")
    _close(got["news"], want["news"], 1e-10, "news")
    _close(got["weight"], want["weight"], 1e-10, "weight")
    n = want["news_cells"]
    T, N = new.shape
    for g in range(len(targets)):
        _close(got["weight"][g].ravel()[n], want["bm"][g], 1e-10, f"target {g}: news weights Cov(y, I) Var(I)^-1")
        _close(got["impact"][g].sum(), want["yhat"][2, g] - want["yhat"][1, g], 1e-10, f"target {g}: sum of impacts")
    assert np.all(got["weight"][:, np.isnan(new)] == 0.0)
    return got, want


@pytest.mark.parametrize("r,p,T,N", [(2, 1, 7, 4), (2, 2, 6, 3), (1, 3, 7, 3)])
@pytest.mark.parametrize("scaled", [False, True])
def test_expectation_model_matches_brute_force(r, p, T, N, scaled):
    prm = _params(N, r, p, seed=10 * r + p)
    old, new = _vintages(T, N, seed=T + N + p)
    news_cell = np.argwhere(~np.isnan(new) & np.isnan(old))[-1]
    targets = [(T - 1, N - 1), (T + 1, 0), (int(news_cell[0]), int(news_cell[1])), (1, 1)]
    rng = np.random.default_rng(3)
    mean = rng.standard_normal(N) if scaled else None
    sd = rng.uniform(0.5, 2.5, N) if scaled else None
    got, _ = _check(old, new, prm, targets, p, mean=mean, sd=sd)
    w = got["weight"][2]                                          # a target that is itself a news cell: weight 1 on itself
    e = np.zeros_like(w)
    e[news_cell[0], news_cell[1]] = 1.0
    _close(w, e, 1e-10, "news-cell target weight")


def test_no_news_gives_exactly_zero_impacts():
    T, N, r, p = 6, 4, 2, 1
    prm = _params(N, r, p, seed=4)
    old, new = _vintages(T, N, seed=5)
    new = np.where(np.isnan(old), np.nan, new)                    # only revisions: no news cell
    got, want = _check(old, new, prm, [(T - 1, 0), (T + 2, 3)], p)
    assert np.all(got["impact"] == 0.0) and np.all(got["news"] == 0.0)
    assert np.array_equal(got["yhat"][1], got["yhat"][2])


def test_singular_q():
    T, N, r, p = 6, 4, 3, 1
    prm = _params(N, r, p, seed=6, singular=True)
    assert np.linalg.matrix_rank(prm[3]) == r - 1
    old, new = _vintages(T, N, seed=7)
    _check(old, new, prm, [(T - 1, 1), (T, 2)], p)


# ----------------------------------------------------------------------------- api.news refusals
class _NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("api.news touched the device before refusing")


def _model(nfac_o=0):
    from dynamic_factor_models_amd import api
    rng = np.random.default_rng(5)
    data = rng.standard_normal((60, 12))
    data[55:, 3] = np.nan
    return api.DFMModel(data, np.ones(12, dtype=int), 20, 20, 1, 50, nfac_o, 2, 1e-8, 1, 1)


def _fake_fit(m):
    r = m.nfac_u
    m.em_params = dict(Lam=np.ones((12, r)), R=np.ones(12), A=0.5 * np.eye(r), Q=np.eye(r), mu0=np.zeros(r), P0=np.eye(r))
    m.uar_coef[:, :] = 0.0


@pytest.fixture
def no_device(monkeypatch):
    from dynamic_factor_models_amd import kalman
    monkeypatch.setattr(kalman, "DfmContext", _NoDevice)


def test_api_news_refuses_before_device_work(no_device):
    from dynamic_factor_models_amd import api
    m = _model()
    with pytest.raises(ValueError, match="estimate"):
        api.news(m, 52, 55, [(0, 55)])                           # not estimated
    _fake_fit(m)
    for bad in ((0, 55), (52, 61), (55, 52)):                      # before initperiod, after T, old later than new
        with pytest.raises(ValueError, match="vintage"):
            api.news(m, *bad, [(0, 55)])
    with pytest.raises(ValueError, match="vintage"):
        api.news(m, np.zeros((55, 13)), 55, [(0, 55)])            # not shaped like m.data
    late = m.data[:55].copy()
    late[10, 2] = 1.0 if np.isnan(late[10, 2]) else late[10, 2]
    early = m.data[:55].copy()
    early[10, 2] = np.nan
    with pytest.raises(ValueError, match="vintage"):
        api.news(m, late, early, [(0, 55)])                       # a cell of old missing in new
    with pytest.raises(ValueError, match="target"):
        api.news(m, 52, 55, [])
    with pytest.raises(ValueError, match="target"):
        api.news(m, 52, 55, [(12, 55)])                           # not a column of m.data
    with pytest.raises(ValueError, match="target"):
        api.news(m, 52, 55, [(0, 0)])                             # before the first period
    mo = _model(nfac_o=1)
    _fake_fit(mo)
    with pytest.raises(ValueError, match="nfac_o"):
        api.news(mo, 52, 55, [(0, 55)])
    ma = _model()
    _fake_fit(ma)
    ma.uar_coef[:, 0] = 0.3
    with pytest.raises(ValueError, match="AR idiosyncratic"):
        api.news(ma, 52, 55, [(0, 55)])
    with pytest.raises(ValueError, match="groups"):
        api.news(m, 52, 55, [(0, 55)], groups={"x": [99]})
    with pytest.raises(ValueError, match="replicates"):
        api.news(m, 52, 55, [(0, 55)], quantiles=[0.5])
    before = {k: v.copy() for k, v in m.em_params.items()}
    with pytest.raises(AssertionError, match="touched the device"):
        api.news(m, 52, 55, [(0, 55), (4, 58)], groups={"a": [0, 1], "b": [4]})   # every check passed
    assert all(np.array_equal(before[k], m.em_params[k]) for k in before)
