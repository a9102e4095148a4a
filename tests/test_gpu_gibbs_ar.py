"""GPU tests of dfm_gibbs_ar_batch (include/dfm_hip.h; csrc/gibbs_ar.hip) against the expectation model of tests/gibbs_ar_expect.py
at 1e-9.  Every sweep is compared on its own: the model's sweep j starts from the device's state after sweep j - 1, so nothing
compounds.  The case table is tests/gibbs_ar_cases.py; tests/test_gibbs_ar_cpu.py asserts that no accept of it is decided within
1e-6 of its boundary, so no series is left out of a comparison.  Then: continuation, repeatability, burn / thin, NULL outputs, the
device entry, the rho cap, every status code, and api.estimate_bayesian_ar_idio with its draws handed to api.draw_paths_ar_idio.
That table reaches the sampler's branches; the table of tests/ar_post_geometry.py (tests/test_gpu_ar_post_geometry.py) runs every
(Q, RB) instance of gibbs_ar_series_kernel, three series blocks and the edges of its staged chunks.

The api test's figures are measured, not chosen: the expectation model, run on the CPU on the same stream
from the same start (scripts/gibbs_ar_api_bound.py: the Stock-Watson panel, 2 chains, 4 + 6 sweeps, about two minutes), gives
max |common_mean - mean| = 63.6619113791 (the largest posterior-mean common component in deviation from the fixed series mean, data
units) and 0.1568163285 for the mean over the series of persistence_mean.  A second model run whose start is moved by 1e-9 gives
63.6619113774 and 0.1568163285: a drift of 1.7e-9 (2.7e-11 of the figure) and 3.7e-12, so the ten sweeps do not amplify a
difference of the size of the per-sweep parity; no accept of either run is decided within 2.4e-5 of its boundary.  The margin is
therefore the per-sweep parity summed over the ten sweeps, 10 x 1e-9 of max(1, |figure|), on either side of the model's figure."""
import ctypes
import os

import numpy as np
import pytest

from tests import forecast_ar_expect as fe
from tests import gibbs_ar_cases as gc
from tests import gibbs_ar_expect as gae

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = gc.KEYS
STATE = ("Lam", "sig2", "rho", "Avar", "Q")
ALL = ("Lam", "sig2", "rho", "A", "Q", "f")
OF = dict(Lam="Lam", sig2="sig2", rho="rho", Avar="A", Q="Q")           # state name -> draw name
API_CHAINS, API_BURN, API_KEPT, API_SEED = 2, 4, 6, 77
API_MODEL_COMMON = 63.6619113791                                        # see the module docstring
API_MODEL_PERSISTENCE = 0.1568163285
API_MARGIN = 10 * TOL                                                   # of max(1, |figure|)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _run(ctx, c, n_sweeps, st=None, **kw):
    st = c["st"] if st is None else st
    kw.setdefault("keep", ALL)
    kw.setdefault("seed", c["seed"])
    return ctx.gibbs_ar_batch_host(c["panel"], *[st[k] for k in KEYS], c["prior"], n_sweeps, may_have_missing=c["may_have_missing"],
                                   singular_q=c["singular_q"], **kw)


def _compare_with_the_model(name, c, d):
    """Every sweep of every chain against the model started at the device's previous state; returns the capped series it met."""
    capped = 0
    for b in range(gc.B):
        cur = {k: c["st"][k][b] for k in KEYS}
        for j in range(gc.SWEEPS):
            want = gae.sweep(c["panel"][b], *[cur[k] for k in KEYS], gc.chain_prior(c, b), c["seed"], j, b)
            for k in ALL:
                _close(d[k][b, j], want[k], f"{name} b={b} sweep={j} {k}")
            cap = want["att_rho"] == gae.RHO_CAP
            assert np.array_equal(d["rho"][b, j][cap], cur["rho"][cap]), f"{name} b={b} sweep={j}: a capped series' rho moved"
            capped += int(cap.sum())
            cur.update(Lam=d["Lam"][b, j], sig2=d["sig2"][b, j], rho=d["rho"][b, j], Avar=d["A"][b, j], Q=d["Q"][b, j])
    return capped


@pytest.mark.parametrize("name", [n for n in gc.CASES if n != "q4_tau1_cap"])
def test_every_sweep_matches_the_model(ctx, name):
    c = gc.build(name)
    start = {k: v.copy() for k, v in c["st"].items()}
    state, d = _run(ctx, c, gc.SWEEPS)
    assert all(np.array_equal(start[k], c["st"][k]) for k in KEYS), "the host entry changed its inputs"
    for k in STATE:
        assert np.array_equal(state[k], d[OF[k]][:, -1]), f"the returned state is not the last sweep's {k}"
    assert _compare_with_the_model(name, c, d) == 0


def test_the_rho_cap_is_reported_and_leaves_rho(ctx):
    """tau_rho = 1 at q = 4: DFM_E_NUMERIC from the host entry; through the device entry the draws are all there -- the capped
    series' rho unchanged, everything else the model's."""
    import torch
    from dynamic_factor_models_amd import _lib
    c = gc.build("q4_tau1_cap")
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, c, gc.SWEEPS)
    assert ei.value.code == -5 and "Gibbs sampler" in str(ei.value)
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = {k: t(c["st"][k]) for k in KEYS}
    _, dd = ctx.gibbs_ar_batch(t(c["panel"]), *[st[k] for k in KEYS], c["prior"], gc.SWEEPS, seed=c["seed"], keep=ALL,
                               may_have_missing=c["may_have_missing"])
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in dd.items()}
    with pytest.raises(_lib.DfmError) as ei:
        ctx.synchronize()
    assert ei.value.code == -5
    assert _compare_with_the_model("q4_tau1_cap", c, d) > 0
    ok = gc.build("q3_balanced")                                        # the handle works on
    assert all(np.isfinite(v).all() for v in _run(ctx, ok, 1)[1].values())


@pytest.mark.parametrize("name", ["q3_r8_n65", "q3_balanced", "q1_r4_n257_two_blocks"])
def test_continuation_and_repeat_are_bit_exact(ctx, name):
    c = gc.build(name)
    whole_state, whole = _run(ctx, c, 4, first_sweep=5)
    again_state, again = _run(ctx, c, 4, first_sweep=5)
    for k in ALL:
        assert np.array_equal(whole[k], again[k]), f"two runs differ in {k}"
    s1, d1 = _run(ctx, c, 2, first_sweep=5)
    s2, d2 = _run(ctx, c, 2, st=dict(c["st"], **s1), first_sweep=7)
    for k in ALL:
        assert np.array_equal(whole[k][:, :2], d1[k]) and np.array_equal(whole[k][:, 2:], d2[k]), f"4 sweeps != 2 + 2 sweeps in {k}"
    for k in STATE:
        assert np.array_equal(whole_state[k], s2[k])


def test_burn_thin_null_outputs_and_device_entry(ctx):
    import torch
    c = gc.build("q2_a0_singular_q")
    full_state, full = _run(ctx, c, 7)
    _, kept = _run(ctx, c, 7, burn=2, thin=2)
    for k in ALL:
        assert kept[k].shape[1] == 3 and np.array_equal(kept[k], full[k][:, [2, 4, 6]]), f"burn / thin keep the wrong sweeps of {k}"
    _, none = _run(ctx, c, 3, burn=3)
    assert all(none[k].shape[1] == 0 for k in ALL)
    state, lean = _run(ctx, c, 7, keep=())
    assert all(v is None for v in lean.values())
    assert all(np.array_equal(state[k], full_state[k]) for k in state), "the state depends on which draws are taken"
    for k in ALL:                                                       # every draw output NULL in turn
        _, rest = _run(ctx, c, 7, keep=tuple(a for a in ALL if a != k))
        assert rest[k] is None and all(np.array_equal(rest[a], full[a]) for a in ALL if a != k), k
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = {k: t(c["st"][k]) for k in KEYS}
    pr = dict(c["prior"], A0=t(c["prior"]["A0"]))
    dstate, dd = ctx.gibbs_ar_batch(t(c["panel"]), *[st[k] for k in KEYS], pr, 7, seed=c["seed"], keep=ALL, may_have_missing=True,
                                    singular_q=True)
    ctx.synchronize()
    assert dstate["Lam"] is st["Lam"], "the device entry updates the state in place"
    for k in ALL:
        assert np.array_equal(dd[k].cpu().numpy(), full[k]), f"the device entry's {k} differs from the host entry's"
    for k in STATE:
        assert np.array_equal(st[k].cpu().numpy(), full_state[k]), f"device entry state {k}"


def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    N, T, r, p, q = 20, 30, 2, 1, 2
    reps = [fe.synth(40 + b, N, T, r, p, q) for b in range(gc.B)]
    c = dict(panel=np.stack([x for x, _, _ in reps]), st={k: np.stack([s[k] for _, s, _ in reps]) for k in KEYS}, prior=gae.prior(r),
             may_have_missing=False, singular_q=False, seed=3)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    st = {k: np.ascontiguousarray(c["st"][k]).copy() for k in KEYS}
    good_prior = dict(tau_lam=1.0, nu_R=2.0, s_R=0.5, tau_rho=0.5, tau_A=1.0, nu_Q=r + 1.0, s_Q=1.0)
    names = ("tau_lam", "nu_R", "s_R", "tau_rho", "tau_A", "nu_Q", "s_Q")

    def call(T_=T, p_=p, q_=q, r_=r, n_sweeps=2, burn=0, thin=1, null=(), **prior):
        pr = dict(good_prior, **prior)
        s = {k: v.copy() for k, v in st.items()}
        a = {k: None if k in null else ptr(v) for k, v in dict(s, panel=c["panel"]).items()}
        return ctx._lib.dfm_gibbs_ar_batch(
            ctx._h, gc.B, T_, N, r_, p_, q_, a["panel"], a["mu0"], a["P0"], *[a[k] for k in STATE], *[pr[k] for k in names], None,
            n_sweeps, burn, thin, 1, 0, None, None, None, None, None, None, 0)

    bad = [dict(n_sweeps=0), dict(thin=0), dict(burn=-1), dict(q_=0), dict(T_=q + p), dict(tau_lam=0.0), dict(nu_R=1.9), dict(s_R=0.0),
           dict(tau_rho=0.0), dict(tau_rho=float("nan")), dict(tau_A=-1.0), dict(nu_Q=r + 0.5), dict(s_Q=0.0)]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # DFM_E_DIMS
        assert call() == 0, f"no good call after {kw}"
    for kw in (dict(q_=5), dict(r_=9, nu_Q=10.0), dict(r_=8, p_=5, nu_Q=9.0)):      # the limits of dfm_em_ar_batch, under a prior valid for that r
        assert call(**kw) == -2, kw                                     # DFM_E_R_UNSUPPORTED
        assert call() == 0
    for k in ("panel", "mu0", "P0") + STATE:
        assert call(null=(k,)) == -3, k                                 # DFM_E_NULL
        assert call() == 0
    nanp = dict(c, panel=c["panel"].copy())
    nanp["panel"][0, 5, 3] = np.nan                                     # NaN without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, nanp, 2)
    assert ei.value.code == -4
    assert call() == 0
    # DFM_E_NUMERIC: test_the_rho_cap_is_reported_and_leaves_rho (a rank-deficient Q does not stop the AR pass)
    _, ok = _run(ctx, c, 2)
    assert all(np.all(np.isfinite(v)) for v in ok.values())


def test_estimate_bayesian_ar_idio_on_the_stock_watson_panel(ctx):
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 4)
    api.estimate(m, api.NonParametric(), ctx=ctx)
    before = {k: np.array(getattr(m, k), copy=True) for k in ("lambda_", "uar_coef", "uar_ser", "factor")}
    inputs, cols, mu_f, c_i = api._ar_model_inputs(m)
    N, r, q, p = cols.size, 4, 4, 4
    S = API_CHAINS * API_KEPT
    out = api.estimate_bayesian_ar_idio(m, API_KEPT, chains=API_CHAINS, burn=API_BURN, seed=API_SEED, quantiles=(0.05, 0.5, 0.95),
                                        keep_factors=True, ctx=ctx)
    for k, v in before.items():
        assert np.array_equal(getattr(m, k), v, equal_nan=True), k + " was modified"
    rp = out["params"]
    n = m.lastperiod - m.initperiod + 1 - q
    assert rp["Lam"].shape == (S, N, r) and rp["sig2"].shape == (S, N) and rp["rho"].shape == (S, N, q)
    assert rp["Avar"].shape == (S, r, r * p) and rp["Q"].shape == (S, r, r) and rp["mu0"].shape == (S, 20) and rp["P0"].shape == (S, 20, 20)
    assert out["factor"].shape == (S, n, r) and out["common_bands"].shape == (3, n, N) and out["rows"].shape == (n,)
    assert out["rho_mean"].shape == (N, q) and out["persistence_mean"].shape == (N,) and np.array_equal(out["cols"], cols)
    assert np.all(out["sig2_mean"] > 0.0) and np.all(out["common_bands"][0] <= out["common_bands"][2])
    assert np.allclose(out["persistence_mean"], out["rho_mean"].sum(1), rtol=0, atol=1e-12)
    for s in range(S):
        for i in range(N):
            assert gae.stationary(rp["rho"][s, i])[0]
    assert out["rhat_sig2"].shape == (N,) and out["rhat_persistence"].shape == (N,) and out["rhat_common"].shape == (N,)
    mean = c_i + inputs["Lam"] @ mu_f
    common = float(np.abs(out["common_mean"] - mean).max())
    pers = float(out["persistence_mean"].mean())
    print(f"max |common_mean - mean| {common:.10f} (model {API_MODEL_COMMON}); mean persistence {pers:.10f} "
          f"(model {API_MODEL_PERSISTENCE}); margin {API_MARGIN}")
    assert abs(common - API_MODEL_COMMON) <= API_MARGIN * max(1.0, API_MODEL_COMMON), common
    assert abs(pers - API_MODEL_PERSISTENCE) <= API_MARGIN * max(1.0, API_MODEL_PERSISTENCE), pers
    # the draws as parameter sets of the path draws: S replicates, 2 draws each
    H = 3
    fan = api.draw_paths_ar_idio(m, 2, H, quantiles=[0.1, 0.9], params=rp, ctx=ctx)
    one = api.draw_paths_ar_idio(m, 2, H, quantiles=[0.1, 0.9], ctx=ctx)
    assert fan["x"].shape == (2 * S, n + H, N) and fan["factor"].shape == (2 * S, n + H, r) and fan["bands"].shape == (2, n + H, N)
    assert one["x"].shape == (2, n + H, N)
    xr = m.data[m.initperiod - 1 + q:m.lastperiod][:, cols]
    obs = ~np.isnan(xr)
    assert np.array_equal(fan["x"][:, :n][:, obs], np.broadcast_to(xr[obs], (2 * S, int(obs.sum()))))
    assert np.all(np.isfinite(fan["x"])) and np.all(fan["x_sd"][n:] > 0.0) and np.all(fan["bands"][0] <= fan["bands"][1])
    # a parameter set equal to the model's own gives the model's own draws
    own = {k: inputs[k][None] for k in KEYS}
    same = api.draw_paths_ar_idio(m, 2, H, params=own, ctx=ctx)
    assert np.array_equal(same["x"], one["x"]) and np.array_equal(same["factor"], one["factor"])
    with pytest.raises(ValueError):
        api.draw_paths_ar_idio(m, 2, H, params=dict(own, rho=own["rho"][:, :, :2]), ctx=ctx)
    with pytest.raises(ValueError):
        api.draw_paths_ar_idio(m, 2, H, params={k: v for k, v in own.items() if k != "P0"}, ctx=ctx)
