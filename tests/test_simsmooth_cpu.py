"""CPU tests of the simulation smoother's contract (include/dfm_hip.h dfm_simsmooth_batch, api.draw_paths), with no Monte Carlo:
the C-ABI's argument check without a handle, api.draw_paths' refusals before any device work, and the expectation model the GPU
tests use (tests/simsmooth_expect.py).  A draw is an affine function of its standard normals; on tiny shapes its map is built
column by column from unit vectors, and its intercept and G G' must be the brute-force posterior mean and JOINT covariance of
(f_1 .. f_{T+H}, x_draw) by plain Gaussian conditioning."""
import ctypes

import numpy as np
import pytest

from oracle import synth_oracle as so
from oracle import varp_oracle as vo
from tests.simsmooth_expect import draw, draw_from_normals, psd_root, sizes, stream_normals


def test_simsmooth_without_a_handle_is_dfm_e_null():
    from dynamic_factor_models_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.dfm_simsmooth_batch, lib.dfm_simsmooth_batch_dev):
        rc = fn(None, 1, 2, 4, 3, 1, 1, 2, *([ptr] * 7), None, None, 7, 0, ptr, None, 0)
        assert rc == -3


class _NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("api.draw_paths touched the device before refusing")


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


def test_api_draw_paths_refuses_before_device_work(no_device):
    from dynamic_factor_models_amd import api
    m = _model()
    with pytest.raises(ValueError, match="estimate"):
        api.draw_paths(m, 10)                                 # not estimated
    _fake_fit(m)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="ndraws"):
            api.draw_paths(m, bad)
    with pytest.raises(ValueError, match="H"):
        api.draw_paths(m, 10, -1)
    with pytest.raises(ValueError, match="first_draw"):
        api.draw_paths(m, 10, first_draw=-1)
    for bad in (49, 61):
        with pytest.raises(ValueError, match="through"):
            api.draw_paths(m, 10, through=bad)
    with pytest.raises(ValueError, match="replicates"):
        api.draw_paths(m, 10, parameter_draws=True)
    mo = _model(nfac_o=1)
    _fake_fit(mo)
    with pytest.raises(ValueError, match="nfac_o"):
        api.draw_paths(mo, 10)
    ma = _model()
    _fake_fit(ma)
    ma.uar_coef[:, 0] = 0.3
    with pytest.raises(ValueError, match="AR idiosyncratic"):
        api.draw_paths(ma, 10)
    before = {k: v.copy() for k, v in m.em_params.items()}
    with pytest.raises(AssertionError, match="touched the device"):
        api.draw_paths(m, 10, 4, through=60)                 # every check passed: the next step is the device
    assert all(np.array_equal(before[k], m.em_params[k]) for k in before)


# ----------------------------------------------------------------------------- the draw as an affine map of its normals
def _params(N, r, p, seed):
    rng = np.random.default_rng(seed)
    k = r * p
    Lam = rng.standard_normal((N, r))
    R = rng.uniform(0.3, 1.2, N)
    A = np.hstack([np.diag(rng.uniform(-0.5, 0.7, r)) * 0.6 ** l + 0.05 * rng.standard_normal((r, r)) for l in range(p)])
    B = rng.standard_normal((r, r))
    Q = B @ B.T / r + 0.2 * np.eye(r)
    mu0 = rng.standard_normal(k)                              # a non-zero prior mean: the pass of step 3 runs with mu0 = 0
    C = rng.standard_normal((k, k))
    P0 = C @ C.T / k + 0.5 * np.eye(k)
    return Lam, R, A, Q, mu0, P0


def _brute_joint(x, Lam, R, A, Q, mu0, P0, H, p):
    """kalman_oracle.brute_force_gaussian's conditioning, restated for the companion state and returning the FULL joint
    posterior of y = (f_1 .. f_{T+H} flat, every cell of rows 1 .. T+H flat): the panel padded with H all-missing rows."""
    T, N = x.shape
    r = Lam.shape[1]
    k = r * p
    TH = T + H
    M, Qk = vo.companion(A, Q, p)
    m = [np.asarray(mu0, float)]
    V = [np.asarray(P0, float)]
    for _ in range(TH):
        m.append(M @ m[-1])
        V.append(M @ V[-1] @ M.T + Qk)
    S = np.zeros(((TH + 1) * k, (TH + 1) * k))
    for a in range(TH + 1):
        for c in range(a, TH + 1):
            blk = np.linalg.matrix_power(M, c - a) @ V[a]        # Cov(z_c, z_a)
            S[c * k:(c + 1) * k, a * k:(a + 1) * k] = blk
            S[a * k:(a + 1) * k, c * k:(c + 1) * k] = blk.T
    mz = np.concatenate(m)
    Sel = np.zeros((TH * r, (TH + 1) * k))                       # f_t = z_t[:r], t = 1 .. T+H
    for t in range(TH):
        Sel[t * r:(t + 1) * r, (t + 1) * k:(t + 1) * k + r] = np.eye(r)
    mf, Sff = Sel @ mz, Sel @ S @ Sel.T
    Lb = np.kron(np.eye(TH), Lam)                                # every cell x_ti = lam_i' f_t + e_ti
    mx = Lb @ mf
    Sxf = Lb @ Sff
    Sxx = Lb @ Sff @ Lb.T + np.diag(np.tile(R, TH))
    mean = np.concatenate([mf, mx])
    C = np.block([[Sff, Sxf.T], [Sxf, Sxx]])
    xp = np.vstack([x, np.full((H, N), np.nan)]).ravel()
    o = TH * r + np.nonzero(~np.isnan(xp))[0]
    K = C[:, o] @ np.linalg.inv(C[np.ix_(o, o)])
    return mean + K @ (xp[o - TH * r] - mean[o]), C - K @ C[o, :]


def _affine_map(x, prm, H, p):
    T, N = x.shape
    r = prm[0].shape[1]
    shp = sizes(T, H, N, r, p)
    names = list(shp)
    n = [int(np.prod(shp[k])) for k in names]
    roots = (psd_root(prm[5]), psd_root(prm[3]))

    def y(u):
        nz, o = {}, 0
        for name, ni in zip(names, n):
            nz[name] = u[o:o + ni].reshape(shp[name])
            o += ni
        f, xd = draw_from_normals(x, *prm, H, p, nz, roots=roots)
        return np.concatenate([f.ravel(), xd.ravel()])

    nu = sum(n)
    c = y(np.zeros(nu))
    G = np.stack([y(np.eye(nu)[i]) - c for i in range(nu)], axis=1)
    return c, G, y


def _close(a, b, tol, what):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f"{what}: {err:.3e}"


@pytest.mark.parametrize("r,p,T,N,H", [(2, 1, 6, 4, 0), (2, 1, 6, 4, 3), (3, 1, 5, 3, 2), (2, 2, 6, 3, 3), (1, 3, 5, 3, 2)])
def test_draw_is_an_exact_draw_of_the_joint_posterior(r, p, T, N, H):
    prm = _params(N, r, p, seed=100 * r + 10 * p + H)
    rng = np.random.default_rng(T + N)
    x = rng.standard_normal((T, N))
    x[rng.random((T, N)) < 0.25] = np.nan                       # missing cells
    x[T // 2, :] = np.nan                                        # and an empty row
    c, G, y = _affine_map(x, prm, H, p)
    mean, cov = _brute_joint(x, *prm, H, p)
    _close(c, mean, 1e-10, "intercept vs posterior mean")
    _close(G @ G.T, cov, 1e-10, "G G' vs joint posterior covariance")
    u = rng.standard_normal(G.shape[1])
    _close(y(u), c + G @ u, 1e-10, "the draw is affine in its normals")
    obs = ~np.isnan(x)
    xd = y(u)[(T + H) * r:].reshape(T + H, N)
    assert np.array_equal(xd[:T][obs], x[obs]), "observed cells are not the data bit for bit"


def test_draw_with_a_singular_q():
    r, p, T, N, H = 3, 1, 5, 4, 2
    Lam, R, A, Q, mu0, P0 = _params(N, r, p, seed=7)
    v = np.random.default_rng(8).standard_normal((r, 2))
    Q = v @ v.T                                                  # rank 2
    L = psd_root(Q)
    assert np.allclose(L @ L.T, Q, atol=1e-14) and np.all(L[:, 2] == 0.0)
    x = np.random.default_rng(9).standard_normal((T, N))
    x[1, 2] = x[3, 0] = np.nan
    c, G, _ = _affine_map(x, (Lam, R, A, Q, mu0, P0), H, p)
    mean, cov = _brute_joint(x, Lam, R, A, Q, mu0, P0, H, p)
    _close(c, mean, 1e-10, "singular Q: mean")
    _close(G @ G.T, cov, 1e-10, "singular Q: covariance")


def test_stream_normals_follow_the_header_table():
    seed, fd, d, b, T, H, N, r, p = 12345, 7, 3, 2, 4, 2, 5, 3, 2
    nz = stream_normals(seed, fd, d, b, T, H, N, r, p)
    key = so.replicate_key(seed, fd + d)
    assert key == (seed ^ (0x9E3779B97F4A7C15 * (fd + d + 1))) & 0xFFFFFFFFFFFFFFFF
    for c in range(r * p):
        assert nz["n0"][c] == so.normal2(key, 16 * b + 1, np.array([c // 2]))[c % 2][0]
    hr, hN = (r + 1) // 2, (N + 1) // 2
    for t in range(T + H):
        for q in range(r):
            assert nz["eta"][t, q] == so.normal2(key, 16 * b + 2, np.array([t * hr + q // 2]))[q % 2][0]
        for i in range(N):
            assert nz["eps"][t, i] == so.normal2(key, 16 * b + 4, np.array([t * hN + i // 2]))[i % 2][0]
            if t < T:
                assert nz["eps_plus"][t, i] == so.normal2(key, 16 * b + 3, np.array([t * hN + i // 2]))[i % 2][0]
    assert {k: v.shape for k, v in nz.items()} == sizes(T, H, N, r, p)


def test_first_draw_split_property():
    r, p, T, N, H = 2, 1, 8, 5, 3
    prm = _params(N, r, p, seed=3)
    x = np.random.default_rng(4).standard_normal((T, N))
    x[2, 1] = np.nan
    for d in range(2, 5):                                        # draws [2, 5) of a call at first_draw = 0 ...
        f0, x0 = draw(x, *prm, H, p, 99, 0, d, 1)
        f1, x1 = draw(x, *prm, H, p, 99, 2, d - 2, 1)            # ... are the draws of a call at first_draw = 2
        assert np.array_equal(f0, f1) and np.array_equal(x0, x1)
    fa, _ = draw(x, *prm, H, p, 99, 0, 0, 1)
    fb, _ = draw(x, *prm, H, p, 99, 0, 0, 0)
    assert not np.allclose(fa, fb), "replicates b share a stream"
