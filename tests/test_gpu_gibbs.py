"""GPU tests of dfm_gibbs_batch (include/dfm_hip.h; csrc/gibbs.hip) against the expectation model of tests/gibbs_expect.py at 1e-9.
Every sweep is compared on its own: the model's sweep j starts from the device's state after sweep j - 1, so nothing compounds.
The case table is tests/gibbs_cases.py (tests/test_gibbs_cpu.py asserts that it meets rejected Gamma attempts in both streams).
Then: continuation, repeatability, burn / thin, NULL outputs, the device entry, every status code, and api.estimate_bayesian.

The api test's bound is measured, not chosen: the expectation model, run on the CPU on the same stream from the oracle's EM fit
of the same panel (4 chains, 300 + 300 sweeps; scripts/gibbs_api_bound.py, about a minute), puts the posterior-mean common component at 0.04451892 of the smoothed common
component at the EM estimate (max abs difference over the window; the panel is standardised).  Two model runs whose starts
differ by 1e-9 stay within 1.04e-8 of each other in every factor and 5.7e-10 in every loading over those 600 sweeps (a sweep
does not amplify along the path), so 1e-6, on either side of the model's figure, is a margin of two orders of magnitude for the 1e-9 per-sweep parity and the parity
of the two EM fits.  The same model run has split-R-hat 1.0205 (R) and 1.0004 (common component) at most; the test asks for the
conventional 1.1."""
import ctypes

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from tests import gibbs_cases as gc
from tests import gibbs_expect as ge

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = gc.KEYS
ALL = ("Lam", "R", "A", "Q", "f")
API_MODEL_DISTANCE = 0.04451892                                  # see the module docstring
API_MARGIN = 1e-6


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
    return ctx.gibbs_batch_host(c["panel"], *[st[k] for k in KEYS], c["prior"], n_sweeps, may_have_missing=c["may_have_missing"],
                                singular_q=c["singular_q"], **kw)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_every_sweep_matches_the_model(ctx, name):
    c = gc.build(name)
    start = {k: v.copy() for k, v in c["st"].items()}
    state, d = _run(ctx, c, gc.SWEEPS)
    assert all(np.array_equal(start[k], c["st"][k]) for k in KEYS), "the host entry changed its inputs"
    for k, dk in (("Lam", "Lam"), ("R", "R"), ("Avar", "A"), ("Q", "Q")):
        assert np.array_equal(state[k], d[dk][:, -1]), f"the returned state is not the last sweep's {k}"
    pr = c["prior"]
    for b in range(gc.B):
        prb = pr if pr["A0"] is None else dict(pr, A0=pr["A0"][b])
        cur = {k: c["st"][k][b] for k in KEYS}
        for j in range(gc.SWEEPS):
            want = ge.sweep(c["panel"][b], *[cur[k] for k in KEYS], c["p"], prb, c["seed"], j, b)
            for k in ALL:
                _close(d[k][b, j], want[k], f"{name} b={b} sweep={j} {k}")
            cur.update(Lam=d["Lam"][b, j], R=d["R"][b, j], A=d["A"][b, j], Q=d["Q"][b, j])


@pytest.mark.parametrize("name", ["missing_ragged", "balanced_fused", "companion"])
def test_continuation_and_repeat_are_bit_exact(ctx, name):
    c = gc.build(name)
    whole_state, whole = _run(ctx, c, 4, first_sweep=5)
    again_state, again = _run(ctx, c, 4, first_sweep=5)
    for k in ALL:
        assert np.array_equal(whole[k], again[k]), f"two runs differ in {k}"
    s1, d1 = _run(ctx, c, 2, first_sweep=5)
    st = dict(c["st"], Lam=s1["Lam"], R=s1["R"], A=s1["Avar"], Q=s1["Q"])
    s2, d2 = _run(ctx, c, 2, st=st, first_sweep=7)
    for k in ALL:
        assert np.array_equal(whole[k][:, :2], d1[k]) and np.array_equal(whole[k][:, 2:], d2[k]), f"4 sweeps != 2 + 2 sweeps in {k}"
    for k in ("Lam", "R", "Avar", "Q"):
        assert np.array_equal(whole_state[k], s2[k])


def test_burn_thin_null_outputs_and_device_entry(ctx):
    import torch
    c = gc.build("a0_singular_q")
    full_state, full = _run(ctx, c, 7)
    _, kept = _run(ctx, c, 7, burn=2, thin=2)
    for k in ALL:
        assert kept[k].shape[1] == 3 and np.array_equal(kept[k], full[k][:, [2, 4, 6]]), f"burn / thin keep the wrong sweeps of {k}"
    _, none = _run(ctx, c, 3, burn=3)
    assert all(none[k].shape[1] == 0 for k in ALL)
    state, lean = _run(ctx, c, 7, keep=())
    assert all(v is None for v in lean.values())
    assert all(np.array_equal(state[k], full_state[k]) for k in state), "the state depends on which draws are taken"
    _, only_r = _run(ctx, c, 7, keep=("R",))
    assert np.array_equal(only_r["R"], full["R"]) and only_r["Lam"] is None
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = {k: t(c["st"][k]) for k in KEYS}
    pr = dict(c["prior"], A0=t(c["prior"]["A0"]))
    dstate, dd = ctx.gibbs_batch(t(c["panel"]), *[st[k] for k in KEYS], pr, 7, seed=c["seed"], keep=ALL, may_have_missing=True,
                                 singular_q=True)
    ctx.synchronize()
    assert dstate["Lam"] is st["Lam"], "the device entry updates the state in place"
    for k in ALL:
        _close(dd[k].cpu().numpy(), full[k], f"device entry {k}")
    _close(st["R"].cpu().numpy(), full_state["R"], "device entry state R")


def test_status_codes(ctx):
    from dynamic_factor_models_amd import _lib
    N, T, r, p = 20, 30, 2, 1
    reps = [ko.synth_replicate(40 + b, N, T, r) for b in range(gc.B)]
    c = dict(panel=np.stack([x for x, _ in reps]), st={k: np.stack([q[k] for _, q in reps]) for k in KEYS}, p=p, prior=ge.prior(r),
             may_have_missing=False, singular_q=False, seed=3)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    st = {k: np.ascontiguousarray(c["st"][k]).copy() for k in KEYS}
    good_prior = dict(tau_lam=1.0, nu_R=2.0, s_R=0.5, tau_A=1.0, nu_Q=r + 1.0, s_Q=1.0)

    def call(T_=T, p_=p, n_sweeps=2, burn=0, thin=1, state=("Lam", "R", "A", "Q"), **prior):
        q = dict(good_prior, **prior)
        s = {k: v.copy() for k, v in st.items()}
        return ctx._lib.dfm_gibbs_batch(
            ctx._h, gc.B, T_, N, r, p_, ptr(c["panel"]), ptr(s["mu0"]), ptr(s["P0"]),
            *[ptr(s[k]) if k in state else None for k in ("Lam", "R", "A", "Q")],
            *[q[k] for k in ("tau_lam", "nu_R", "s_R", "tau_A", "nu_Q", "s_Q")], None, n_sweeps, burn, thin, 1, 0,
            None, None, None, None, None, 0)

    bad = [dict(n_sweeps=0), dict(thin=0), dict(burn=-1), dict(T_=p), dict(tau_lam=0.0), dict(nu_R=1.9), dict(s_R=0.0),
           dict(tau_A=-1.0), dict(nu_Q=r + 0.5), dict(s_Q=0.0), dict(tau_lam=float("nan"))]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # DFM_E_DIMS
        assert call() == 0, f"no good call after {kw}"
    for k in ("Lam", "R", "A", "Q"):
        assert call(state=tuple(s for s in ("Lam", "R", "A", "Q") if s != k)) == -3, k      # NULL state: DFM_E_NULL
        assert call() == 0
    # r p > 32: whatever the pass says for the same shape
    big = dict(Lam=np.ones((1, 20, 9)), R=np.ones((1, 20)), A=np.zeros((1, 9, 36)), Q=np.eye(9)[None].copy(), mu0=np.zeros((1, 36)),
               P0=np.eye(36)[None].copy())
    xv = np.random.default_rng(0).standard_normal((1, 30, 20))
    with pytest.raises(_lib.DfmError) as want:
        ctx.ks_pass_varp_batch_host(xv, *[big[k] for k in KEYS])
    with pytest.raises(_lib.DfmError) as got:
        ctx.gibbs_batch_host(xv, *[big[k] for k in KEYS], ge.prior(9), 2)
    assert got.value.code == want.value.code
    assert call() == 0
    nanp = dict(c, panel=c["panel"].copy())
    nanp["panel"][0, 5, 3] = np.nan                                     # NaN without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, nanp, 2)
    assert ei.value.code == -4
    assert call() == 0
    sing = dict(c, st={k: v.copy() for k, v in c["st"].items()})        # a rank-deficient Q in information form: the pass and with it
    sing["st"]["Q"][1] = 0.5 * np.ones((r, r))                          # the factor path are not finite, the Cholesky fails: DFM_E_NUMERIC
    with pytest.raises(_lib.DfmError) as ei:
        _run(ctx, sing, 2)
    assert ei.value.code == -5
    assert call() == 0
    ok_state, ok = _run(ctx, c, 2)
    assert all(np.all(np.isfinite(v)) for v in ok.values())


def test_estimate_bayesian_against_the_em_fit(ctx):
    from dynamic_factor_models_amd import api
    N, T, r, chains, burn, kept = 30, 120, 2, 4, 300, 300
    x, _ = ko.synth_replicate(7, N, T, r)
    m = api.DFMModel(x, np.ones(N, int), 20, 40, 1, T, 0, r, 1e-8, 1, 1)
    api.estimate(m, api.Parametric(), max_em_iter=20, tol_em=0.0, factor_lags=1, ctx=ctx)
    before = {k: v.copy() for k, v in m.em_params.items()}
    out = api.estimate_bayesian(m, kept, chains=chains, burn=burn, seed=77, quantiles=(0.05, 0.5, 0.95), keep_factors=True, ctx=ctx)
    assert all(np.array_equal(before[k], m.em_params[k]) for k in before) and getattr(m, "replicates", None) is None, \
        "estimate_bayesian changed the model"
    rp = out["params"]
    assert rp["Lam"].shape == (chains * kept, N, r) and rp["R"].shape == (chains * kept, N) and rp["A"].shape == (chains * kept, r, r)
    assert rp["Q"].shape == (chains * kept, r, r) and rp["mu0"].shape == (chains * kept, r) and rp["P0"].shape == (chains * kept, r, r)
    assert out["factor"].shape == (chains * kept, T, r) and out["common_bands"].shape == (3, T, N)
    cols, z, mu, sd = api._forecast_inputs(m, T)
    ep = m.em_params
    f_em = ctx.ks_pass_batch_host(z[None], *[ep[k][None] for k in KEYS], want_P=False)[0][0]       # smoothed at the EM estimate
    em_common = mu + sd * (f_em @ ep["Lam"].T)
    dist = float(np.abs(out["common_mean"] - em_common).max() / max(1.0, np.abs(em_common).max()))
    print(f"posterior-mean common component vs the EM fit: {dist:.6f} (model {API_MODEL_DISTANCE}); "
          f"max rhat R {out['rhat_R'].max():.4f}, common {out['rhat_common'].max():.4f}")
    assert abs(dist - API_MODEL_DISTANCE) <= API_MARGIN, dist
    assert np.all(out["common_bands"][0] <= out["common_bands"][2]) and np.all(out["R_mean"] > 0.0)
    assert np.all(np.isfinite(out["rhat_R"])) and out["rhat_R"].max() < 1.1 and out["rhat_common"].max() < 1.1
    m.replicates = dict(params=rp)                                      # the draws as parameter draws of a band-producing function
    fc = api.forecast(m, 4, quantiles=(0.1, 0.9), ctx=ctx)
    assert fc["bands"].shape == (2, 4, N) and np.all(fc["bands"][0] <= fc["bands"][1])
