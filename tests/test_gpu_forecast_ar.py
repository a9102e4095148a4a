"""GPU tests of dfm_forecast_ar_batch (include/dfm_hip.h; csrc/forecast_ar.hip) against the expectation model of
tests/forecast_ar_expect.py -- the oracle's AR pass over the panel with H all-missing rows appended, then per series DENSE Gaussian
conditioning of the idiosyncratic process on its residuals -- at 1e-9, section 10's tolerance for cell outputs.  Observed cells are
bit for bit, xvar on them is exactly 0.  The case table (forecast_ar_expect.CASES) holds the smallest shapes that reach every
branch: q = 1 .. 4, p below / at / above q + 1, r = 1 and 8 (k = 32), one / two / three series blocks with full and ragged last
waves, T = q + 1, a horizon longer than a staged chunk, every missing-cell pattern of apply_pattern in one panel;
tests/test_forecast_ar_cpu.py checks that table's coverage and conditioning without a device.  Branches, not kernel instances:
the table of tests/ar_post_geometry.py (tests/test_gpu_ar_post_geometry.py) runs every reachable (Q, RB) instance of the two kernels
and every edge of their staged chunks."""
import ctypes
import os

import numpy as np
import pytest

from tests import forecast_ar_expect as fe

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = fe.KEYS
CELLS = ("xhat", "xvar", "common", "idio")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


_cases = {}


def _case(name):
    """The case's inputs and, computed once and left unchanged, its expectations per replicate."""
    if name not in _cases:
        c = fe.make_case(name)
        c["expect"] = [fe.expect_case(c, b) for b in range(c["dims"][0])]
        _cases[name] = c
    return _cases[name]


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _run(ctx, c, **kw):
    H = c["dims"][6]
    kw.setdefault("v0", c["v0"])
    return ctx.forecast_ar_batch_host(c["x"], *[c["st"][k] for k in KEYS], H, **kw)


def _check(got, c, exp, what):
    B, N, T, r, p, q, H = c["dims"]
    obs = ~np.isnan(np.concatenate([c["x"], np.full((B, H, N), np.nan)], axis=1)[:, q:])
    for b in range(B):
        e = exp[b]
        tag = f"{what} b={b}"
        for k in CELLS + ("f", "P"):
            if got[k] is not None:
                _close(got[k][b], e[k], f"{tag} {k}")
        if got["loglik"] is not None:
            assert abs(got["loglik"][b] - e["loglik"]) <= TOL * abs(e["loglik"]), (tag, got["loglik"][b], e["loglik"])
        if got["xvar"] is not None:
            assert np.all(got["xvar"][b][obs[b]] == 0.0), tag + ": xvar on an observed cell is not exactly 0"
            assert np.all(got["xvar"][b][~obs[b]] > 0.0), tag + ": xvar on a missing cell is not positive"
    return obs


@pytest.mark.parametrize("name", list(fe.CASES))
def test_case_against_the_expectation_model(ctx, name):
    """mean / sd NULL: every output at 1e-9, observed cells of xhat bit for bit the panel's."""
    c = _case(name)
    B, N, T, r, p, q, H = c["dims"]
    got = _run(ctx, c)
    obs = _check(got, c, c["expect"], name)
    assert got["xhat"].shape == (B, T + H - q, N)
    assert np.array_equal(got["xhat"][:, :T - q][obs[:, :T - q]], c["x"][:, q:][obs[:, :T - q]]), "observed cells are not the panel's bits"
    assert not obs[:, T - q:].any()


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q4_p_gt_n139", "q1_n257_two_blocks"])
def test_mean_and_sd(ctx, name):
    c = _case(name)
    exp = [fe.expect_case(c, b, scaled=True) for b in range(c["dims"][0])]
    _check(_run(ctx, c, mean=c["mean"], sd=c["sd"]), c, exp, name + " scaled")


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q3_r8_n65_long_h"])
def test_v0_null_is_sig2(ctx, name):
    c = _case(name)
    exp = [fe.expect_case(c, b, v0=False) for b in range(c["dims"][0])]
    got = _run(ctx, c, v0=None)
    _check(got, c, exp, name + " v0 NULL")
    same = _run(ctx, c, v0=c["st"]["sig2"])
    for k in CELLS:
        assert np.array_equal(got[k], same[k], equal_nan=True), k


def test_every_optional_output_null_in_turn(ctx):
    from dynamic_factor_models_amd import forecasting_ar as fa
    c = _case("q4_p_gt_n139")
    full = _run(ctx, c)
    for drop in fa.OPTIONAL:
        got = _run(ctx, c, want=[w for w in fa.OPTIONAL if w != drop])
        assert got[drop] is None
        for k in CELLS + ("f", "P", "loglik"):
            if k != drop:
                assert np.array_equal(got[k], full[k]), f"without {drop}: {k} changed"
    got = _run(ctx, c, want=())
    assert np.array_equal(got["xhat"], full["xhat"]) and np.array_equal(got["f"], full["f"])


def _dev_call(ctx, c, shift, scaled):
    """The device entry by hand: every output starts `shift` doubles into its own allocation (shift = 1: 8 bytes off a 16-byte
    line)."""
    import torch
    B, N, T, r, p, q, H = c["dims"]
    n = T + H - q
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [t(c["x"])] + [t(c["st"][k]) for k in KEYS] + [t(c["v0"])] + ([t(c["mean"]), t(c["sd"])] if scaled else [None, None])
    sizes = dict(xhat=B * n * N, xvar=B * n * N, common=B * n * N, idio=B * n * N, f=B * n * r, P=B * n * (r * (r + 1) // 2), loglik=B)
    bufs = {k: torch.full((s + shift,), -7.0, dtype=torch.float64, device=dev) for k, s in sizes.items()}
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    optr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 8 * shift)
    ctx._sync_stream()
    rc = ctx._lib.dfm_forecast_ar_batch_dev(ctx._h, B, T, N, r, p, q, H, *[ptr(v) for v in ins],
                                            *[optr(k) for k in ("xhat", "xvar", "common", "idio", "f", "P", "loglik")], 1)
    assert rc == 0, rc
    ctx.synchronize()
    assert all(float(bufs[k][0]) == -7.0 for k in bufs) or shift == 0
    return {k: bufs[k][shift:].cpu().numpy() for k in bufs}


@pytest.mark.parametrize("name,scaled", [("q4_p_gt_n139", False), ("q2_p_eq_n64_h0", True), ("q1_n257_two_blocks", False)])
def test_host_and_device_entries_give_equal_bytes_at_any_alignment(ctx, name, scaled):
    c = _case(name)
    host = _run(ctx, c, may_have_missing=True, **(dict(mean=c["mean"], sd=c["sd"]) if scaled else {}))
    for shift in (0, 1):
        got = _dev_call(ctx, c, shift, scaled)
        for k in got:
            assert np.array_equal(got[k], host[k].ravel()), f"shift {shift}: {k} differs from the host entry"


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q3_r8_n65_long_h", "q4_t_min_h1"])
def test_moments_are_the_ar_pass_on_the_padded_panel(ctx, name):
    c = _case(name)
    B, N, T, r, p, q, H = c["dims"]
    got = _run(ctx, c)
    xp = np.concatenate([c["x"], np.full((B, H, N), np.nan)], axis=1)
    f, P, ll = ctx.ks_pass_ar_batch_host(xp, *[c["st"][k] for k in KEYS], may_have_missing=True)
    assert np.array_equal(got["f"], f) and np.array_equal(got["P"], P) and np.array_equal(got["loglik"], ll)


def test_slices_over_the_message_buffer(ctx):
    """B = 3 replicates at a cap that holds one replicate's messages, then two: the same bytes as the one-slice call."""
    from dynamic_factor_models_amd import DfmContext
    c = _case("q4_p_gt_n139")
    B, N, T, r, p, q, H = c["dims"]
    per = (q + q * (q + 1) // 2) * (T + H - q) * N * 8
    full = _run(ctx, c)
    for cap in (per, 2 * per + 8, 1):
        old = os.environ.get("DFM_FCAR_MSG_BYTES")
        os.environ["DFM_FCAR_MSG_BYTES"] = str(cap)
        try:
            small = DfmContext()
        finally:
            if old is None:
                os.environ.pop("DFM_FCAR_MSG_BYTES", None)
            else:
                os.environ["DFM_FCAR_MSG_BYTES"] = old
        try:
            got = _run(small, c)
        finally:
            small.close()
        for k in CELLS + ("f", "P", "loglik"):
            assert np.array_equal(got[k], full[k]), f"cap {cap}: {k} differs"


def _raw_host(ctx, dims, arrays, null=(), flags=1):
    """dfm_forecast_ar_batch itself, past the binding's own argument checks; arrays: name -> array or None."""
    B, N, T, r, p, q, H = dims
    n = max(T + H - q, 1)
    outs = dict(xhat=np.empty((B, n, N)), xvar=None, common=None, idio=None, f_out=np.empty((B, n, r)), P_out=None, loglik=np.empty(B))
    names = ("x",) + KEYS + ("v0", "mean", "sd")
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    keep = [None if k in null else (None if arrays.get(k) is None else np.ascontiguousarray(arrays[k], dtype=np.float64)) for k in names]
    return ctx._lib.dfm_forecast_ar_batch(ctx._h, B, T, N, r, p, q, H, *[ptr(a) for a in keep],
                                          *[ptr(None if k in null else outs[k]) for k in outs], flags)


def test_status_codes(ctx):
    c = _case("q3_balanced_h5")
    B, N, T, r, p, q, H = c["dims"]
    arrays = dict(c["st"], x=c["x"], v0=c["v0"], mean=c["mean"], sd=c["sd"])
    assert _raw_host(ctx, c["dims"], arrays) == 0
    assert _raw_host(ctx, (B, N, T, r, p, q, -1), arrays) == -1                         # H < 0
    assert _raw_host(ctx, (B, N, T, r, p, 0, H), arrays) == -1                          # q < 1
    assert _raw_host(ctx, (B, N, q, r, p, q, H), arrays) == -1                          # T <= q
    assert _raw_host(ctx, (B, N, T, r, p, 5, H), arrays) == -2                          # q > 4
    assert _raw_host(ctx, (B, N, T, 8, 1, 4, H), arrays) == -2                          # r (q + 1) = 40 > 32 (ar_check)
    assert _raw_host(ctx, c["dims"], arrays, null=("sd",)) == -3                        # mean without sd
    assert _raw_host(ctx, c["dims"], arrays, null=("xhat",)) == -3
    assert _raw_host(ctx, c["dims"], arrays, null=("f_out",)) == -3
    assert _raw_host(ctx, c["dims"], arrays, null=("rho",)) == -3
    assert _raw_host(ctx, c["dims"], arrays, null=("v0", "mean", "sd", "loglik")) == 0
    holed = dict(arrays, x=c["x"].copy())
    holed["x"][0, T // 2, 1] = np.nan
    assert _raw_host(ctx, c["dims"], holed, flags=0) == -4                              # a NaN panel without the flag
    assert _raw_host(ctx, c["dims"], holed, flags=1) == 0
    assert _raw_host(ctx, c["dims"], arrays, flags=0) == 0                              # balanced: the H empty rows are the entry's own


def test_binding_refuses_before_the_device(ctx):
    c = _case("q3_balanced_h5")
    args = [c["x"]] + [c["st"][k] for k in KEYS]
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, -1)
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, 2, mean=c["mean"])
    with pytest.raises(ValueError):
        ctx.forecast_ar_batch_host(*args, 2, want=("xvar", "nonsense"))


def test_forecast_ar_idio_on_the_stock_watson_panel():
    """estimate(m, NonParametric()) -> api.forecast_ar_idio with through = lastperiod and H = 4, against the expectation model on the
    arrays it handed to the library; the model object is left as it was."""
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 4)
    api.estimate(m, api.NonParametric())
    before = {k: np.array(getattr(m, k), copy=True) for k in ("lambda_", "uar_coef", "uar_ser", "factor")}
    H, q = 4, m.n_uarlag
    out = api.forecast_ar_idio(m, H, through=m.lastperiod)
    for k, v in before.items():
        assert np.array_equal(getattr(m, k), v, equal_nan=True), k + " was modified"
    a = out["inputs"]
    n = m.lastperiod - m.initperiod + 1 + H - q
    assert np.array_equal(out["rows"], np.arange(m.initperiod + q, m.lastperiod + H + 1)) and out["x"].shape == (n, out["cols"].size)
    e = fe.expect(a["x"], *[a[k] for k in KEYS], H, v0=a["v0"], mean=a["mean"], sd=np.ones_like(a["mean"]))
    _close(out["x"], e["xhat"], "x")
    _close(out["common"], e["common"], "common")
    _close(out["idio"], e["idio"], "idio")
    _close(out["x_sd"] ** 2, e["xvar"], "x_sd^2")
    _close(out["factor"] - out["mu_f"], e["f"], "factor")
    il = np.tril_indices(m.nfac_u)
    _close(out["factor_cov"][:, il[0], il[1]], e["P"], "factor_cov")
    assert abs(out["loglik"] - e["loglik"]) <= TOL * abs(e["loglik"]), (out["loglik"], e["loglik"])
    obs = ~np.isnan(a["x"][q:])
    data = m.data[m.initperiod - 1 + q:m.lastperiod][:, out["cols"]]
    assert np.abs(out["x"][:n - H][obs] - data[obs]).max() <= 1e-12 * np.abs(data[obs]).max()
    assert np.all(out["x_sd"][:n - H][obs] == 0.0) and np.all(out["x_sd"][n - H:] > 0.0)
    # the persistence is there: one step ahead the idiosyncratic part is not negligible beside the common part's deviation
    assert np.abs(out["idio"][n - H]).max() > 0.0
