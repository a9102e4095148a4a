"""dfm_gibbs_ar_batch without a device: the expectation model of tests/gibbs_ar_expect.py against np.linalg, what the case table
of tests/gibbs_ar_cases.py reaches, the stream table, the Python marshalling against a recorder in place of the library
(tests/test_kalman_marshalling_cpu.py's), argument and prior errors, and the symbols of the header, _lib.py and the Julia shim."""
import ctypes
import os
import re

import numpy as np
import pytest

from dynamic_factor_models_amd import _lib, api, bayes, gibbs_ar
from tests import gibbs_ar_cases as gc
from tests import gibbs_ar_expect as gae
from tests import gibbs_expect as ge
from tests import simsmooth_ar_expect as sae
from tests.test_kalman_marshalling_cpu import HANDLE, MISS, SING, addr, dev, make_ctx, val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10


def _series(seed, n=60, r=3, q=2, gaps=True):
    g = np.random.default_rng(seed)
    f = g.standard_normal((n, r))
    lam = g.standard_normal(r)
    rho = np.array([0.5, -0.2, 0.1, 0.05])[:q]
    e = np.zeros(n)
    for t in range(n):
        e[t] = sum(rho[l] * e[t - 1 - l] for l in range(q) if t - 1 - l >= 0) + 0.7 * g.standard_normal()
    x = f @ lam + e
    if gaps:
        x[[7, 20, 21, 22, 40]] = np.nan
    return x, f, lam, rho


# ---------------------------------------------------------------------- the two series blocks against np.linalg
@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_rho_block_is_the_textbook_posterior(q):
    x, f, lam, _ = _series(q, q=q)
    sig2, tau = 0.6, 3.0
    use = gae.used_rows(x[:, None], q)[:, 0]
    assert 0 < use.sum() < len(x) - q and not use[:q].any()
    L, y = gae.rho_posterior(x, f, lam, sig2, use, q, tau)
    c = gae.rho_from(L, y, np.zeros(q))
    G = np.stack([gae.rho_from(L, y, np.eye(q)[j]) - c for j in range(q)], axis=1)
    e = x - f @ lam
    W = np.array([[e[t - 1 - l] for l in range(q)] for t in np.nonzero(use)[0]])
    ee = e[use]
    assert not np.isnan(W).any() and not np.isnan(ee).any(), "a used row touches a missing cell"
    Sinv = np.linalg.inv(tau * np.eye(q) + W.T @ W / sig2)
    assert np.abs(c - Sinv @ (W.T @ ee) / sig2).max() <= BOUND
    assert np.abs(G @ G.T - Sinv).max() <= BOUND
    # the candidate is affine in its normals
    n = np.random.default_rng(0).standard_normal(q)
    assert np.abs(gae.rho_from(L, y, n) - (c + G @ n)).max() <= BOUND


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_loading_block_is_the_textbook_posterior_on_quasi_differences(q):
    x, f, _, rho = _series(10 + q, q=q)
    tau, Ri = 2.0, 0.8
    r = f.shape[1]
    use = gae.used_rows(x[:, None], q)[:, 0]
    xt, ft = gae.quasi_difference(x, f, rho, use)
    tt = np.nonzero(use)[0]
    want_x = np.array([x[t] - sum(rho[l] * x[t - 1 - l] for l in range(q)) for t in tt])
    want_f = np.array([f[t] - sum(rho[l] * f[t - 1 - l] for l in range(q)) for t in tt])
    assert not np.isnan(want_x).any() and np.abs(xt - want_x).max() <= BOUND and np.abs(ft - want_f).max() <= BOUND
    L, y, xx = ge.load_posterior(ft, xt, tau)
    c = ge.lam_from(L, y, Ri, np.zeros(r))
    G = np.stack([ge.lam_from(L, y, Ri, np.eye(r)[j]) - c for j in range(r)], axis=1)
    S = tau * np.eye(r) + want_f.T @ want_f
    m = np.linalg.solve(S, want_f.T @ want_x)
    assert np.abs(c - m).max() <= BOUND and np.abs(G @ G.T - Ri * np.linalg.inv(S)).max() <= BOUND
    assert abs((xx - y @ y) - (want_x @ want_x - m @ S @ m)) <= BOUND * max(1.0, xx)


def test_a_series_without_a_usable_row_draws_from_the_priors():
    x, f, lam, rho = _series(3, q=2)
    x[::2] = np.nan                                              # never three observed cells in a row
    use = gae.used_rows(x[:, None], 2)[:, 0]
    assert use.sum() == 0
    L, y = gae.rho_posterior(x, f, lam, 0.5, use, 2, 4.0)
    assert np.array_equal(L, 2.0 * np.eye(2)) and np.array_equal(y, np.zeros(2))
    xt, ft = gae.quasi_difference(x, f, rho, use)
    L, y, xx = ge.load_posterior(ft, xt, 1.5)
    assert np.allclose(L, np.sqrt(1.5) * np.eye(3), atol=0, rtol=1e-15) and not y.any() and xx == 0.0


def test_step_down_agrees_with_the_companion_matrix():
    g = np.random.default_rng(2026)
    wrong = total = 0
    for q in (1, 2, 3, 4):
        for phi in g.normal(0.0, 0.6, (20000, q)):
            M = np.zeros((q, q))
            M[0] = phi
            M[1:, :-1] = np.eye(q - 1)
            radius = np.abs(np.linalg.eigvals(M)).max()
            if abs(radius - 1.0) < 1e-9:
                continue
            wrong += gae.stationary(phi)[0] != (radius < 1.0)
            total += 1
    assert total > 79000 and wrong == 0


# ---------------------------------------------------------------------- what the case table reaches
def test_the_table_reaches_rejections_priors_and_the_cap_and_decides_nothing_at_a_boundary():
    rej_rho = rej_gam = n0 = cap = 0
    kinds, few = set(), False
    for name in gc.CASES:
        c = gc.build(name)
        N, T, r, p, q = c["dims"]
        kinds |= c["kinds"]
        for b, sweeps in enumerate(gc.model_chains(name)):
            for j, o in enumerate(sweeps):
                where = f"{name} b={b} sweep={j}"
                assert all(np.isfinite(o[k]).all() for k in ("Lam", "sig2", "rho", "A", "Q", "f")), where
                assert o["margin_rho"] >= 1e-6, f"{where}: a rho attempt within {o['margin_rho']:.2e} of |kappa| = 1"
                assert o["margin_gamma"] >= 1e-6, f"{where}: a Gamma attempt within {o['margin_gamma']:.2e} of its accept boundary"
                assert (o["att_R"] < ge.GAMMA_CAP).all() and (o["att_Q"] < ge.GAMMA_CAP).all(), f"{where}: the Gamma cap"
                capped = o["att_rho"] == gae.RHO_CAP
                if name != "q4_tau1_cap":
                    assert not capped.any(), f"{where}: the rho cap at tau_rho = {c['prior']['tau_rho']}"
                cap += int(capped.sum())
                rej_rho += int(o["att_rho"][~capped].sum())
                rej_gam += int(o["att_R"].sum())
                n0 += int((o["n_i"] == 0).sum())
                few = few or bool(((o["n_i"] > 0) & (o["n_i"] < r)).any())
                for i in np.nonzero(~capped)[0]:
                    assert gae.stationary(o["rho"][i])[0], where
    assert rej_rho > 0 and rej_gam > 0 and n0 > 0 and cap > 0 and few
    assert kinds == set(range(1, 10)), f"pattern classes reached: {sorted(kinds)}"
    dims = np.array([gc.build(n)["dims"] for n in gc.CASES])
    assert set(dims[:, 4]) == {1, 2, 3, 4} and {1, 4, 8} <= set(dims[:, 2]) and {1, 64, 65, 139, 257} <= set(dims[:, 0])
    assert any(p < q + 1 for *_, p, q in dims) and any(p == q + 1 for *_, p, q in dims) and any(p > q + 1 for *_, p, q in dims)
    assert any(T - q == p + 1 for _, T, _, p, q in dims) and any(r * max(p, q + 1) == 32 for _, _, r, p, q in dims)
    assert any(not gc.build(n)["may_have_missing"] for n in gc.CASES) and any(gc.build(n)["singular_q"] for n in gc.CASES)


def test_the_capped_series_keep_their_rho():
    c = gc.build("q4_tau1_cap")
    hit = 0
    for b, sweeps in enumerate(gc.model_chains("q4_tau1_cap")):
        prev = c["st"]["rho"][b]
        for o in sweeps:
            capped = o["att_rho"] == gae.RHO_CAP
            assert np.array_equal(o["rho"][capped], prev[capped])
            hit += int(capped.sum())
            prev = o["rho"]
    assert hit > 0


def test_streams_10_and_11_are_not_the_path_step_s(monkeypatch):
    words = []
    real = sae._pairs
    monkeypatch.setattr(sae, "_pairs", lambda key, word, *a: (words.append(word), real(key, word, *a))[1])
    b = 3
    sae.stream_normals(5, 2, 0, b, 20, 0, 7, 2, 1, 2)
    assert words and {w - 16 * b for w in words} == {1, 2, 3, 5}
    words.clear()
    monkeypatch.setattr(gae, "_pairs", lambda key, word, *a: (words.append(word), real(key, word, *a))[1])
    gae.stream_randoms(5, 2, b, 20, 7, 2, 1, 2)
    own = {w - 16 * b for w in words} - {1, 2, 3, 5}
    assert {10, 11} <= own and 5 not in own and own <= {7, 8, 10, 11}


# ---------------------------------------------------------------------- marshalling
B, T, N, r, p, q = 2, 14, 6, 3, 2, 4
M_ = max(p, q + 1)
PRIOR = dict(tau_lam=1.5, nu_R=4, s_R=0.25, tau_rho=3.5, tau_A=2.5, nu_Q=r + 2, s_Q=0.75)
NAMES = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")
PER = dict(Lam=(N, r), sig2=(N,), rho=(N, q), A=(r, r * p), Q=(r, r), f=(T - q, r))


def arrays(nan=True):
    g = np.random.default_rng(0)
    a = dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), sig2=g.random((B, N)) + 1,
             rho=g.standard_normal((B, N, q)), Avar=g.standard_normal((B, r, r * p)), Q=g.standard_normal((B, r, r)),
             mu0=g.standard_normal((B, r * M_)), P0=g.standard_normal((B, r * M_, r * M_)), A0=g.standard_normal((B, r, r * p)))
    if nan:
        a["panel"][1, 3, 2] = np.nan
    return a


def recorded(ctx, name):
    assert [c[0] for c in ctx._lib.calls] == [name]
    args = ctx._lib.calls.pop()[1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds) == 35
    for i, (x, kind) in enumerate(zip(args, kinds)):
        where = f"{name} argument {i}"
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int, where
        elif kind is ctypes.c_double:
            assert type(x) is float, where
        elif kind is ctypes.c_void_p:
            assert x is None or isinstance(x, ctypes.c_void_p), where
        else:
            assert kind in (ctypes.c_uint64, ctypes.c_int64) and type(x) is int, where
    return args


def call(ctx, host, a, prior, n_sweeps, **kw):
    conv = (lambda x: x) if host else dev
    t = {k: conv(v) for k, v in a.items()}
    pr = dict(prior)
    if pr.get("A0") is not None:
        pr["A0"] = t["A0"]
    fn = ctx.gibbs_ar_batch_host if host else ctx.gibbs_ar_batch
    state, draws = fn(t["panel"], *[t[k] for k in NAMES], pr, n_sweeps, **kw)
    return t, state, draws, recorded(ctx, "dfm_gibbs_ar_batch" if host else "dfm_gibbs_ar_batch_dev")


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("with_a0", [False, True])
def test_argument_order_types_and_state(host, with_a0):
    ctx, a = make_ctx(), arrays()
    prior = dict(PRIOR, A0=a["A0"] if with_a0 else None)
    keep = gibbs_ar.DRAWS
    t, state, draws, args = call(ctx, host, a, prior, 9, burn=2, thin=3, seed=(1 << 64) + 5, first_sweep=7, keep=keep)
    assert val(args[0]) == HANDLE and args[1:7] == (B, T, N, r, p, q)
    assert [val(x) for x in args[7:10]] == [addr(t["panel"]), addr(t["mu0"]), addr(t["P0"])]
    assert tuple(state) == gibbs_ar.STATE == NAMES[:5]
    for i, k in enumerate(gibbs_ar.STATE):                    # the state: in place on the device, copies on the host
        assert val(args[10 + i]) == addr(state[k])
        if host:
            assert state[k] is not a[k] and np.array_equal(state[k], a[k]) and addr(state[k]) != addr(a[k])
        else:
            assert state[k] is t[k]
    assert args[15:22] == (1.5, 4.0, 0.25, 3.5, 2.5, float(r + 2), 0.75)
    assert val(args[22]) == (addr(t["A0"]) if with_a0 else None)
    assert args[23:28] == (9, 2, 3, 5, 7)                     # n_sweeps, burn, thin, seed mod 2^64, first_sweep
    for i, k in enumerate(keep):                              # K = 3: sweeps 2, 5, 8
        assert type(draws[k]) is type(t["panel"]) and tuple(draws[k].shape) == (B, 3) + PER[k] and str(draws[k].dtype).endswith("float64")
        assert val(args[28 + i]) == addr(draws[k])
    assert args[34] == MISS                                   # the panel was scanned: it has a NaN


@pytest.mark.parametrize("host", [False, True])
def test_keep_subsets_flags_and_refusals(host):
    ctx, a = make_ctx(), arrays(nan=False)
    _, _, draws, args = call(ctx, host, a, PRIOR, 4, keep=("rho", "f"), singular_q=True)
    assert [k for k in draws if draws[k] is not None] == ["rho", "f"] and tuple(draws) == gibbs_ar.DRAWS
    assert [val(x) for x in args[28:34]] == [None, None, addr(draws["rho"]), None, None, addr(draws["f"])]
    assert args[34] == SING and args[23:28] == (4, 0, 1, 0, 0)
    _, _, draws, args = call(ctx, host, a, PRIOR, 4, may_have_missing=True)                  # the default keep: no f
    assert draws["f"] is None and all(tuple(draws[k].shape) == (B, 4) + PER[k] for k in ("Lam", "sig2", "rho", "A", "Q"))
    assert args[34] == MISS
    _, _, draws, args = call(ctx, host, a, PRIOR, 3, burn=3, keep=("Lam", "rho"))            # K = 0: nothing to point at
    assert tuple(draws["rho"].shape) == (B, 0, N, q) and [val(x) for x in args[28:34]] == [None] * 6
    fn = ctx.gibbs_ar_batch_host if host else ctx.gibbs_ar_batch
    t = {k: (v if host else dev(v)) for k, v in a.items()}
    for kw in (dict(n_sweeps=0), dict(n_sweeps=2, thin=0), dict(n_sweeps=2, burn=-1), dict(n_sweeps=2, keep=("Lam", "R"))):
        with pytest.raises(ValueError):
            fn(t["panel"], *[t[k] for k in NAMES], PRIOR, **kw)
    with pytest.raises(ValueError):                           # the plain sampler's prior has no tau_rho
        fn(t["panel"], *[t[k] for k in NAMES], {k: v for k, v in PRIOR.items() if k != "tau_rho"}, 2)
    assert ctx._lib.calls == []


# ---------------------------------------------------------------------- priors, api arguments, symbols
def test_default_prior_ar_and_its_check():
    pr = bayes.default_prior_ar(3)
    assert pr == dict(bayes.default_prior(3), tau_rho=4.0)
    assert bayes.check_prior_ar(None, 3, 2, 4) == pr
    got = bayes.check_prior_ar(dict(tau_rho=2, s_Q=0.9, A0=np.ones((3, 6))), 3, 2, 4)
    assert got["tau_rho"] == 2.0 and type(got["tau_rho"]) is float and got["s_Q"] == 0.9 and got["A0"].shape == (4, 3, 6)
    for bad in (dict(tau_rho=0.0), dict(tau_rho=-1.0), dict(tau_rho=float("nan")), dict(tau_rh=1.0), dict(nu_R=1.0), dict(tau_lam=0.0)):
        with pytest.raises(ValueError):
            bayes.check_prior_ar(bad, 3, 2, 4)
    with pytest.raises(ValueError):                           # the plain model's check does not know tau_rho
        bayes.check_prior(dict(tau_rho=4.0), 3, 2, 4)


def test_api_argument_errors_come_before_any_work():
    x = np.random.default_rng(1).standard_normal((40, 8))
    m = api.DFMModel(x, np.ones(8, int), 20, 20, 1, 40, 0, 2, 1e-8, 2, 1)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device work before the argument checks: {name}")

    for kw in (dict(ndraws=0), dict(ndraws=5, chains=0), dict(ndraws=5, burn=-1), dict(ndraws=5, thin=0),
               dict(ndraws=5, quantiles=(0.0, 0.5)), dict(ndraws=5, quantiles=())):
        with pytest.raises(ValueError):
            api.estimate_bayesian_ar_idio(m, ctx=NoDevice(), **kw)
    with pytest.raises(ValueError, match="not estimated"):    # nothing fitted yet
        api.estimate_bayesian_ar_idio(m, 5, ctx=NoDevice())
    m5 = api.DFMModel(x, np.ones(8, int), 20, 20, 1, 40, 0, 2, 1e-8, 5, 1)
    with pytest.raises(ValueError, match="n_uarlag"):
        api.estimate_bayesian_ar_idio(m5, 5, ctx=NoDevice())
    import inspect
    sig = inspect.signature(api.estimate_bayesian_ar_idio)
    assert list(sig.parameters)[:2] == ["m", "ndraws"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        chains=4, burn=500, thin=1, prior=None, seed=20160415, keep_factors=False, quantiles=None, ctx=None)
    assert inspect.signature(api.draw_paths_ar_idio).parameters["params"].default is None


def test_header_lib_and_julia_name_the_entries():
    header = open(os.path.join(ROOT, "include", "dfm_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "dfm_hip.jl")).read()
    for name in ("dfm_gibbs_ar_batch_dev", "dfm_gibbs_ar_batch"):
        proto = re.search(r"\nint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
        kinds = _lib.SYMBOLS[name][1]
        assert len(args) == len(kinds) == 35
        for a, kind in zip(args, kinds):
            want = (ctypes.c_void_p if "*" in a else ctypes.c_double if a.startswith("double") else ctypes.c_uint64 if a.startswith("uint64_t")
                    else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_uint if a.startswith("unsigned") else ctypes.c_int)
            assert kind is want, (name, a)
        assert [a.split()[-1].lstrip("*") for a in args][1:7] == ["B", "T", "N", "r", "p", "q"]
        assert args[15:22] == ["double " + k for k in gibbs_ar.PRIOR]
    assert "function estimate_bayesian_ar(" in julia and "(:dfm_gibbs_ar_batch, LIB)" in julia
    for word in ("stream 11", "stream 10", "tau_rho", "step-down", "not identified", "first q output rows"):
        assert word in header, word
