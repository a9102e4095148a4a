"""Expectation model of dfm_simsmooth_ar_batch (include/dfm_hip.h; csrc/simsmooth_ar.hip) on the CPU, three texts:

  stream_normals     the normals of one draw from the header's stream table (oracle/synth_oracle.py's Philox4x32-10, Box-Muller);
  draw_from_normals  steps 1-7 of the header for given standard normals; step 6 is tests/forecast_ar_expect.expect on the
                     difference panel (the oracle's AR pass, then dense conditioning per series);
  brute_joint        the joint conditional mean and covariance of ALL non-observed output cells given whichever cells are observed,
                     from the model's own recursion (forecast_ar_expect.brute_force's model): no quasi-differencing, no two-step
                     argument.  Rows 0 .. q-1 are conditioned on, so they must be observed.

draw_from_normals is affine in its normals: affine_map returns its intercept and its matrix G by finite evaluation (exact, the map
has no curvature).  Shared by tests/test_simsmooth_ar_cpu.py and tests/test_gpu_simsmooth_ar.py."""
import numpy as np

from oracle import ar_oracle as ao
from oracle import synth_oracle as so
from tests import forecast_ar_expect as fe
from tests.simsmooth_expect import _pairs, psd_root


def sizes(T, H, N, r, p, q):
    """Shapes of the normals of one draw: n0 [k], eta [n, r], eps_plus [n, N], pre [q, N] (row l-1: pre-sample term l)."""
    n = T + H - q
    return dict(n0=(r * ao.state_lags(p, q),), eta=(n, r), eps_plus=(n, N), pre=(q, N))


def stream_normals(seed, first_draw, d, b, T, H, N, r, p, q):
    """Draw d of replicate b: key = replicate_key(seed, first_draw + d), stream word 16 b + s with s = 1, 2, 3, 5."""
    key = so.replicate_key(seed, first_draw + d)
    w = 16 * b
    n = T + H - q
    return dict(n0=_pairs(key, w + 1, 1, r * ao.state_lags(p, q))[0], eta=_pairs(key, w + 2, n, r),
                eps_plus=_pairs(key, w + 3, n, N), pre=_pairs(key, w + 5, q, N))


def draw_from_normals(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, nz, v0=None, mean=None, sd=None, roots=None):
    """One draw of one replicate: x [T, N] (NaN = missing), rho [N, q], Avar = [A_1 .. A_p].  Returns (f_draw [n, r], x_draw [n, N])."""
    x = np.asarray(x, float)
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    k = r * m
    n = T + H - q
    v0 = sig2 if v0 is None else np.asarray(v0, float)
    LP0, LQ = roots if roots is not None else (psd_root(P0), psd_root(Q))
    # 1. the state: lags f_{q-1} .. f_{q-m}
    z = mu0 + LP0 @ nz["n0"]
    hist = [z[l * r:(l + 1) * r] for l in range(m)]
    # 3. pre-sample terms e+_{q-l}, l = 1 .. q
    eh = [np.where(np.isnan(x[q - l]), np.sqrt(v0) * nz["pre"][l - 1], x[q - l] - Lam @ hist[l - 1]) for l in range(1, q + 1)]
    # 2. factor path and 4. series path
    fp, ep = np.empty((n, r)), np.empty((n, N))
    for t in range(n):
        f = sum(Avar[:, l * r:(l + 1) * r] @ hist[l] for l in range(p)) + LQ @ nz["eta"][t]
        e = sum(rho[:, l] * eh[l] for l in range(q)) + np.sqrt(sig2) * nz["eps_plus"][t]
        fp[t], ep[t] = f, e
        hist = [f] + hist[:-1]
        eh = [e] + eh[:-1]
    xplus = fp @ Lam.T + ep
    # 5. the difference panel on T + H rows
    Dp = np.full((T + H, N), np.nan)
    Dp[:q] = np.where(np.isnan(x[:q]), np.nan, 0.0)
    Dp[q:T] = x[q:] - xplus[:T - q]
    # 6. its smoothed mean with mu0 = 0 and the smoother's mean of its residuals
    o = fe.expect(Dp, Lam, sig2, rho, Avar, Q, np.zeros(k), P0, 0, v0=v0)
    g, ehs = o["f"], o["idio"]
    # 7. outputs
    fd = fp + g
    xo = np.vstack([x[q:], np.full((H, N), np.nan)])
    xd = np.where(np.isnan(xo), fd @ Lam.T + ep + ehs, xo)
    if mean is not None:
        xd = np.asarray(mean, float) + np.asarray(sd, float) * xd
    return fd, xd


def draw(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, seed, first_draw, d, b, v0=None, mean=None, sd=None, roots=None):
    """draw_from_normals on the header's stream: what dfm_simsmooth_ar_batch returns for (b, d)."""
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    nz = stream_normals(seed, first_draw, d, b, T, H, N, r, Avar.shape[1] // r, q)
    return draw_from_normals(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, nz, v0=v0, mean=mean, sd=sd, roots=roots)


def _pack(shapes, v):
    out, o = {}, 0
    for name, sh in shapes.items():
        c = int(np.prod(sh))
        out[name] = v[o:o + c].reshape(sh)
        o += c
    return out


def affine_map(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, v0=None):
    """x_draw = c + G nz over all normals stacked in the order of `sizes`: (c [n N], G [n N, dim])."""
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    shapes = sizes(T, H, N, r, Avar.shape[1] // r, q)
    dim = sum(int(np.prod(s)) for s in shapes.values())
    roots = (psd_root(P0), psd_root(Q))
    run = lambda v: draw_from_normals(x, Lam, sig2, rho, Avar, Q, mu0, P0, H, _pack(shapes, v), v0=v0, roots=roots)[1].ravel()
    c = run(np.zeros(dim))
    G = np.empty((c.size, dim))
    for j in range(dim):
        e = np.zeros(dim)
        e[j] = 1.0
        G[:, j] = run(e) - c
    return c, G


def brute_joint(x, Lam, sig2, rho, Avar, Q, mu0, P0, H):
    """x [T, N] with rows 0 .. q-1 observed.  Returns (mis [n, N] bool, mean [nmis], cov [nmis, nmis]): the non-observed output
    cells (row-major) and their joint conditional moments given the observed output cells and rows 0 .. q-1."""
    T, N = x.shape
    r, q = Lam.shape[1], rho.shape[1]
    p = Avar.shape[1] // r
    m = ao.state_lags(p, q)
    k = r * m
    n = T + H - q
    dim = k + n * r + n * N
    assert not np.isnan(x[:q]).any()

    def run(v):
        z = v[:k]
        eta = v[k:k + n * r].reshape(n, r)
        eps = v[k + n * r:].reshape(n, N)
        hist = [z[l * r:(l + 1) * r] for l in range(m)]
        eh = [x[q - 1 - l] - Lam @ hist[l] for l in range(q)]
        xs = np.empty((n, N))
        for t in range(n):
            f = sum(Avar[:, l * r:(l + 1) * r] @ hist[l] for l in range(p)) + eta[t]
            e = sum(rho[:, l] * eh[l] for l in range(q)) + eps[t]
            xs[t] = Lam @ f + e
            hist = [f] + hist[:-1]
            eh = [e] + eh[:-1]
        return xs.ravel()

    mean_v = np.zeros(dim)
    mean_v[:k] = mu0
    S = np.zeros((dim, dim))
    S[:k, :k] = P0
    for t in range(n):
        S[k + t * r:k + (t + 1) * r, k + t * r:k + (t + 1) * r] = Q
    S[k + n * r:, k + n * r:] = np.diag(np.tile(sig2, n))
    x0 = run(np.zeros(dim))
    J = np.empty((n * N, dim))
    for j in range(dim):
        e = np.zeros(dim)
        e[j] = 1.0
        J[:, j] = run(e) - x0
    mx = x0 + J @ mean_v
    C = J @ S @ J.T
    xo = np.vstack([x[q:], np.full((H, N), np.nan)])
    mis = np.isnan(xo)
    o, u = ~mis.ravel(), mis.ravel()
    if o.any():
        K = np.linalg.solve(C[np.ix_(o, o)], C[np.ix_(o, u)]).T
        mean = mx[u] + K @ (xo.ravel()[o] - mx[o])
        cov = C[np.ix_(u, u)] - K @ C[np.ix_(o, u)]
    else:
        mean, cov = mx[u], C[np.ix_(u, u)]
    return mis, mean, cov


# ---------------------------------------------------------------------------------------------------- the GPU case table
KEYS = fe.KEYS

# name -> B, D, N, T, r, p, q, H, first pattern kind (None: balanced).  B D <= 16.  Together: q = 1 .. 4; p below, at and above q + 1;
# r = 1, 4 and 8 with k = 32; N = 1, 64, 65 and 257 (two series blocks); T = q + 1; H = 0, 1 and 41 (longer than a 32-row chunk);
# B = 1 and 3; D = 1 and 5; every class of forecast_ar_expect.apply_pattern.
CASES = {
    "q1_n1_gap": (1, 5, 1, 40, 1, 1, 1, 1, 4),
    "q1_n1_none_observed": (1, 1, 1, 12, 1, 1, 1, 2, 7),
    "q2_p_eq_n64_h0": (3, 5, 64, 40, 2, 3, 2, 0, 0),
    "q3_r8_n65_long_h": (1, 5, 65, 41, 8, 1, 3, 41, 3),
    "q4_p_gt_n139": (3, 1, 139, 40, 1, 6, 4, 4, 1),
    "q1_r4_n257_two_blocks": (1, 5, 257, 40, 4, 2, 1, 2, 2),
    "q2_t_min_h0": (1, 5, 6, 3, 1, 1, 2, 0, 4),
    "q4_t_min_h1": (1, 1, 12, 5, 2, 1, 4, 1, 0),
    "q3_balanced_h5": (1, 5, 10, 24, 2, 2, 3, 5, None),
}


def make_case(name):
    """The inputs of a case, built as forecast_ar_expect.make_case builds its own: dict(dims (B, N, T, r, p, q, H), D, x [B,T,N],
    st (KEYS -> stacked arrays), v0, mean, sd [B,N], kinds)."""
    B, D, N, T, r, p, q, H, first = CASES[name]
    xs, sts, v0s = [], [], []
    kinds = set()
    for b in range(B):
        x, st, v0 = fe.synth(b + 3, max(N, r + 2), max(T, 3 * r + 12), r, p, q)
        x = np.ascontiguousarray(x[:T, :N])
        st = dict(st, Lam=st["Lam"][:N], sig2=st["sig2"][:N], rho=st["rho"][:N])
        if first is not None:
            kinds |= fe.apply_pattern(x, q, first + b)
        xs.append(x); sts.append(st); v0s.append(v0[:N])
    rng = np.random.default_rng([5, N, T, q])
    return dict(dims=(B, N, T, r, p, q, H), D=D, x=np.stack(xs), st={k: np.stack([s[k] for s in sts]) for k in KEYS},
                v0=np.stack(v0s), mean=rng.standard_normal((B, N)), sd=rng.uniform(0.5, 2.0, (B, N)), kinds=kinds)


def expect_draw(c, b, d, seed, first_draw=0, v0=True, scaled=False):
    H = c["dims"][6]
    return draw(c["x"][b], *[c["st"][k][b] for k in KEYS], H, seed, first_draw, d, b, v0=c["v0"][b] if v0 else None,
                mean=c["mean"][b] if scaled else None, sd=c["sd"][b] if scaled else None)
