"""Expectation model of the PCA start (csrc/pca.hip: gram_xx_* + pca_kernel) on the CPU, stage by stage as the kernel runs them:
  start           the deterministic hash start of the basis (the 32-bit arithmetic of pca_kernel's first loop)
  cholqr          Cholesky-QR orthonormalisation  V = Y L^-T,  Y'Y = L L'
  iterate         subspace iteration on S = X'X with the residual ||S V - V H||_F / ||S V||_F, H = V'S V, and both exits;
                  the stopping rule is a parameter, so that the rule the kernel had first can be shown beside the one it has now
  ritz            Rayleigh-Ritz on the symmetrised H of the final basis, descending order
  fix_signs       the oracle's sign rule (largest-|.| entry of a vector positive, first index on ties)
  tail            F = X V and the OLS / VAR(1) start exactly as the kernel forms it from F'F, F0'F0, F0'F1, F1'F1
  pca_start       all of it: the outputs of dfm_pca_init_batch for one panel, plus `iterations`, `converged`, `rel`
  spectrum_panel  a panel whose X'X has a prescribed spectrum: the convergence rate at the cut is a number the test chooses
Shared by tests/test_pca_cpu.py (checked against oracle/kalman_oracle.py pca_init = the reference's svd-based pca_score) and
tests/test_gpu_pca_routes.py (which compares the library with the ORACLE; the model is there to choose the cases)."""
import numpy as np

MAX_ITER = 4000          # capi.hip dfm_pca_init_batch_dev
REL_EXIT = 1e-14         # first exit: the residual is at the fp64 floor
STALL_EXIT = 8           # second exit: this many iterations in a row without progress ...
BEST_ACCEPT = 1e-10      # ... with the best residual under this level; also the level under which max_iter running out is no error


def start(N, r):
    """Y [N, r]: a fixed hash of (series i, column k) mapped to [-0.5, 0.5), the same for every replicate."""
    i = np.arange(N, dtype=np.uint64)[:, None]
    k = np.arange(r, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = ((i * np.uint64(73856093)) & m) ^ (((k + np.uint64(1)) * np.uint64(19349663)) & m)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0x5BD1E995)) & m
    h ^= h >> np.uint64(15)
    return (h & np.uint64(0xFFFF)).astype(float) / 65536.0 - 0.5


def cholqr(Y):
    """V = Y L^-T with Y'Y = L L': orthonormal columns spanning those of Y."""
    L = np.linalg.cholesky(Y.T @ Y)
    return np.linalg.solve(L, Y.T).T


def _stalled_old(rel, best):
    """The first rule: an iteration counts as progress only if it HALVES the best residual.  At a rate lambda_{r+1} / lambda_r
    near 1 almost none does, so the loop leaves as soon as `best` is under BEST_ACCEPT, still improving."""
    return not rel < 0.5 * best


def _stalled_new(rel, best):
    """The present rule: an iteration counts as progress if it sets a new minimum.  Eight in a row without one happen at the
    floating-point floor only."""
    return not rel < best


RULES = {"old": _stalled_old, "new": _stalled_new}


def iterate(S, V, rule="new", max_iter=MAX_ITER):
    """The loop of pca_kernel / pca_iterate_lds from the orthonormal start V.  Returns (V, iterations, converged, rel).
    `converged` is what keeps status bit 2 down: an exit fired (either rule), or -- present rule only -- max_iter ran out with the
    best residual under BEST_ACCEPT (the level the first rule accepted)."""
    stalled = RULES[rule]
    best, stall, fired, rel, it = 1e300, 0, False, np.inf, 0
    for it in range(1, max_iter + 1):
        Y = S @ V
        H = V.T @ Y
        rel = float(np.linalg.norm(Y - V @ H) / np.linalg.norm(Y))
        V = cholqr(Y)
        if rel <= REL_EXIT:
            fired = True
            break
        if stalled(rel, best):
            stall += 1
            if stall >= STALL_EXIT and best < BEST_ACCEPT:
                fired = True
                break
        else:
            best, stall = rel, 0
    converged = fired or (rule == "new" and best < BEST_ACCEPT)
    return V, it, converged, rel


def ritz(S, V):
    """V W with H = V'S V = W Theta W' (H symmetrised), Theta descending."""
    H = V.T @ (S @ V)
    H = 0.5 * (H + H.T)
    ev, W = np.linalg.eigh(H)
    return V @ W[:, np.argsort(-ev, kind="stable")]


def fix_signs(V):
    sg = np.where(V[np.abs(V).argmax(axis=0), np.arange(V.shape[1])] < 0.0, -1.0, 1.0)
    return V * sg


def tail(x, S, V):
    """Outputs of the kernel's tail from the sign-fixed Ritz vectors V [N, r]."""
    T = x.shape[0]
    r = V.shape[1]
    F = x @ V
    G = F.T @ F
    R = (np.diag(S) - np.einsum("ik,km,im->i", V, G, V)) / T
    F0, F1 = F[:-1], F[1:]
    W = F0.T @ F1                                              # [p][q] = sum_t F[t][p] F[t+1][q]
    At = np.linalg.solve(F0.T @ F0, W)                         # A'
    Q = (F1.T @ F1 - At.T @ W) / (T - 1)
    return dict(Lam=V.copy(), R=R, A=At.T, Q=0.5 * (Q + Q.T), mu0=np.zeros(r), P0=0.5 * (G + G.T) / T), F


def pca_start(x, r, rule="new", max_iter=MAX_ITER):
    """(params, F, info) of one balanced panel x [T, N]; info = dict(iterations, converged, rel)."""
    S = x.T @ x
    V, it, converged, rel = iterate(S, cholqr(start(x.shape[1], r)), rule, max_iter)
    params, F = tail(x, S, fix_signs(ritz(S, V)))
    return params, F, dict(iterations=it, converged=converged, rel=rel)


def spectrum_panel(seed, T, N, lam):
    """X = U diag(sqrt(lam)) W' [T, N] with seeded orthonormal U (T x N) and W (N x N): the eigenvalues of X'X are `lam`."""
    lam = np.asarray(lam, float)
    assert lam.shape == (N,) and T >= N
    rng = np.random.default_rng([20261018, seed])
    U, _ = np.linalg.qr(rng.standard_normal((T, N)))
    W, _ = np.linalg.qr(rng.standard_normal((N, N)))
    return (U * np.sqrt(lam)) @ W.T
