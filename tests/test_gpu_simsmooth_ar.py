"""GPU tests of dfm_simsmooth_ar_batch (include/dfm_hip.h; csrc/simsmooth_ar.hip): every draw against the NumPy restatement of the
header's seven steps on the header's random stream (tests/simsmooth_ar_expect.py: the oracle's AR pass and dense conditioning per
series for step 6) at 1e-9 x scale, the bound of tests/test_gpu_simsmooth.py and tests/test_gpu_forecast_ar.py.  Observed cells
are bit for bit.  The case table (simsmooth_ar_expect.CASES; its coverage is checked in tests/test_simsmooth_ar_cpu.py, which
also shows that the restatement has the exact posterior mean and joint covariance) holds the smallest shapes that reach every
branch: q = 1 .. 4, p below / at / above q + 1, r = 1, 4 and 8 with k = 32, N = 1, 64, 65 and 257 (two series blocks), T = q + 1,
H = 0, 1 and 41 (longer than a staged chunk), B = 1 and 3, D = 1 and 5, every missing-cell class of apply_pattern.  Branches, not
kernel instances: the table of tests/ar_post_geometry.py (tests/test_gpu_ar_post_geometry.py) runs every reachable (Q, RB) instance of
the kernels, three series blocks and every edge of their staged chunks."""
import ctypes
import os

import numpy as np
import pytest

from tests import simsmooth_ar_expect as se

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = se.KEYS
SEED = 20160415


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


_cases, _expect = {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = se.make_case(name)
    return _cases[name]


def _expected(name, seed=SEED, v0=True, scaled=False):
    """(f [B,D,n,r], x [B,D,n,N]) of the case on the header's stream, computed once and left unchanged."""
    key = (name, seed, v0, scaled)
    if key not in _expect:
        c = _case(name)
        B, D = c["dims"][0], c["D"]
        fs, xs = [], []
        for b in range(B):
            out = [se.expect_draw(c, b, d, seed, v0=v0, scaled=scaled) for d in range(D)]
            fs.append(np.stack([o[0] for o in out])); xs.append(np.stack([o[1] for o in out]))
        f, x = np.stack(fs), np.stack(xs)
        f.setflags(write=False); x.setflags(write=False)
        _expect[key] = (f, x)
    return _expect[key]


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _run(ctx, c, D=None, st=None, **kw):
    H = c["dims"][6]
    kw.setdefault("v0", c["v0"])
    kw.setdefault("seed", SEED)
    st = c["st"] if st is None else st
    return ctx.simsmooth_ar_batch_host(c["x"], *[st[k] for k in KEYS], c["D"] if D is None else D, H, **kw)


def _observed(c):
    B, N, T, r, p, q, H = c["dims"]
    return ~np.isnan(np.concatenate([c["x"], np.full((B, H, N), np.nan)], axis=1)[:, q:])


@pytest.mark.parametrize("name", list(se.CASES))
def test_case_against_the_header_on_its_stream(ctx, name):
    """mean / sd NULL: every draw of f and x at 1e-9, observed cells of x bit for bit the panel's."""
    c = _case(name)
    B, N, T, r, p, q, H = c["dims"]
    D, n = c["D"], T + H - q
    got = _run(ctx, c)
    ef, ex = _expected(name)
    assert got["f"].shape == (B, D, n, r) and got["x"].shape == (B, D, n, N)
    _close(got["f"], ef, name + " f_draw")
    _close(got["x"], ex, name + " x_draw")
    obs = _observed(c)
    xo = np.concatenate([c["x"], np.full((B, H, N), np.nan)], axis=1)[:, q:]
    for d in range(D):
        assert np.array_equal(got["x"][:, d][obs], xo[obs]), "observed cells are not the panel's bits"
    assert np.all(np.isfinite(got["x"])) and not obs[:, T - q:].any()
    if D > 1 and (~obs).any():
        assert np.all(got["x"][:, 0][~obs] != got["x"][:, 1][~obs]), "two draws share a missing cell's value"


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q4_p_gt_n139", "q1_r4_n257_two_blocks"])
def test_mean_and_sd(ctx, name):
    c = _case(name)
    got = _run(ctx, c, mean=c["mean"], sd=c["sd"])
    ef, ex = _expected(name, scaled=True)
    _close(got["f"], ef, name + " scaled f_draw")
    _close(got["x"], ex, name + " scaled x_draw")
    obs = _observed(c)
    B, N, T, r, p, q, H = c["dims"]
    xo = np.concatenate([c["x"], np.full((B, H, N), np.nan)], axis=1)[:, q:]
    # mean + sd X with one rounding (a fused multiply-add) or two: within two ulps of the larger term either way
    prod = c["sd"][:, None, :] * xo
    want, ulp = c["mean"][:, None, :] + prod, 2.0 ** -52 * (np.abs(c["mean"][:, None, :]) + np.abs(prod))
    for d in range(c["D"]):
        assert np.all(np.abs(got["x"][:, d][obs] - want[obs]) <= 2.0 * ulp[obs]), "observed cells are not mean + sd X"
        assert np.array_equal(got["x"][:, d][obs], got["x"][:, 0][obs]), "observed cells differ between draws"


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q3_r8_n65_long_h"])
def test_v0_null_is_sig2(ctx, name):
    c = _case(name)
    got = _run(ctx, c, v0=None)
    ef, ex = _expected(name, v0=False)
    _close(got["f"], ef, name + " v0 NULL f_draw")
    _close(got["x"], ex, name + " v0 NULL x_draw")
    same = _run(ctx, c, v0=c["st"]["sig2"])
    assert np.array_equal(got["f"], same["f"]) and np.array_equal(got["x"], same["x"])


@pytest.mark.parametrize("name", ["q4_p_gt_n139", "q1_r4_n257_two_blocks"])
def test_f_draw_without_x_draw(ctx, name):
    c = _case(name)
    full = _run(ctx, c)
    got = _run(ctx, c, want_x=False)
    assert got["x"] is None and np.array_equal(got["f"], full["f"])


def _dev_call(ctx, c, shift, scaled):
    """The device entry by hand: both outputs start `shift` doubles into their own allocation."""
    import torch
    B, N, T, r, p, q, H = c["dims"]
    D, n = c["D"], T + H - q
    dev = torch.device("cuda", ctx.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [t(c["x"])] + [t(c["st"][k]) for k in KEYS] + [t(c["v0"])] + ([t(c["mean"]), t(c["sd"])] if scaled else [None, None])
    sizes = dict(f=B * D * n * r, x=B * D * n * N)
    bufs = {k: torch.full((s + shift,), -7.0, dtype=torch.float64, device=dev) for k, s in sizes.items()}
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    ctx._sync_stream()
    rc = ctx._lib.dfm_simsmooth_ar_batch_dev(ctx._h, B, D, T, N, r, p, q, H, *[ptr(v) for v in ins], SEED, 0,
                                             *[ctypes.c_void_p(bufs[k].data_ptr() + 8 * shift) for k in ("f", "x")], 1)
    assert rc == 0, rc
    ctx.synchronize()
    assert all(float(bufs[k][0]) == -7.0 for k in bufs) or shift == 0
    return {k: bufs[k][shift:].cpu().numpy() for k in bufs}


@pytest.mark.parametrize("name,scaled", [("q4_p_gt_n139", False), ("q2_p_eq_n64_h0", True)])
def test_host_and_device_entries_give_equal_bytes_at_any_alignment(ctx, name, scaled):
    c = _case(name)
    host = _run(ctx, c, may_have_missing=True, **(dict(mean=c["mean"], sd=c["sd"]) if scaled else {}))
    for shift in (0, 1):
        got = _dev_call(ctx, c, shift, scaled)
        for k in got:
            assert np.array_equal(got[k], host[k].ravel()), f"shift {shift}: {k} differs from the host entry"


@pytest.mark.parametrize("name", ["q2_p_eq_n64_h0", "q3_r8_n65_long_h"])
def test_first_draw_splits_a_call(ctx, name):
    """first_draw = 2, D = 3 equals draws 2 .. 4 of the D = 5 call, bit for bit."""
    c = _case(name)
    assert c["D"] == 5
    full = _run(ctx, c)
    part = _run(ctx, c, D=3, first_draw=2)
    assert np.array_equal(part["f"], full["f"][:, 2:5]) and np.array_equal(part["x"], full["x"][:, 2:5])


def test_slices_over_the_message_buffer(ctx):
    """B D = 15 pass replicates at caps that hold one, two and seven replicates' messages, and none: the one-slice call's bytes."""
    from dynamic_factor_models_amd import DfmContext
    c = _case("q2_p_eq_n64_h0")
    B, N, T, r, p, q, H = c["dims"]
    per = (q + q * (q + 1) // 2) * (T + H - q) * N * 8
    full = _run(ctx, c, mean=c["mean"], sd=c["sd"])
    for cap in (per, 2 * per + 8, 7 * per, 1):
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
            got = _run(small, c, mean=c["mean"], sd=c["sd"])
            nox = _run(small, c, want_x=False)
        finally:
            small.close()
        assert np.array_equal(got["f"], full["f"]) and np.array_equal(got["x"], full["x"]), f"cap {cap}"
        assert np.array_equal(nox["f"], full["f"]), f"cap {cap}, no x_draw"


def test_singular_q(ctx):
    """Q of rank 1 at r = 2, p = q + 1 (where the oracle's smoother still inverts its predicted covariance): DFM_F_SINGULAR_Q."""
    c = _case("q2_p_eq_n64_h0")
    B, D = c["dims"][0], c["D"]
    Q = c["st"]["Q"].copy()
    for b in range(B):
        v = np.linalg.cholesky(Q[b])[:, :1]
        Q[b] = v @ v.T
    st = dict(c["st"], Q=Q)
    got = _run(ctx, c, st=st, singular_q=True)
    H = c["dims"][6]
    for b in range(B):
        for d in (0, D - 1):
            f, x = se.draw(c["x"][b], *[st[k][b] for k in KEYS], H, SEED, 0, d, b, v0=c["v0"][b])
            _close(got["f"][b, d], f, f"singular Q b={b} d={d} f_draw")
            _close(got["x"][b, d], x, f"singular Q b={b} d={d} x_draw")


def _raw_host(ctx, dims, D, arrays, null=(), flags=1):
    """dfm_simsmooth_ar_batch itself, past the binding's own argument checks; arrays: name -> array or None."""
    B, N, T, r, p, q, H = dims
    n = max(T + H - q, 1)
    outs = dict(f_draw=np.empty((B, max(D, 1), n, r)), x_draw=np.empty((B, max(D, 1), n, N)))
    names = ("x",) + KEYS + ("v0", "mean", "sd")
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    keep = [None if k in null else (None if arrays.get(k) is None else np.ascontiguousarray(arrays[k], dtype=np.float64)) for k in names]
    return ctx._lib.dfm_simsmooth_ar_batch(ctx._h, B, D, T, N, r, p, q, H, *[ptr(a) for a in keep], SEED, 0,
                                           *[ptr(None if k in null else outs[k]) for k in outs], flags)


def test_status_codes(ctx):
    c = _case("q3_balanced_h5")
    B, N, T, r, p, q, H = c["dims"]
    D = 2
    arrays = dict(c["st"], x=c["x"], v0=c["v0"], mean=c["mean"], sd=c["sd"])
    assert _raw_host(ctx, c["dims"], D, arrays) == 0
    assert _raw_host(ctx, c["dims"], 0, arrays) == -1                                   # D < 1
    assert _raw_host(ctx, (B, N, T, r, p, q, -1), D, arrays) == -1                      # H < 0
    assert _raw_host(ctx, (B, N, T, r, p, 0, H), D, arrays) == -1                       # q < 1
    assert _raw_host(ctx, (B, N, q, r, p, q, H), D, arrays) == -1                       # T <= q
    assert _raw_host(ctx, (B, N, T, r, p, 5, H), D, arrays) == -2                       # q > 4
    assert _raw_host(ctx, (B, N, T, 8, 1, 4, H), D, arrays) == -2                       # r (q + 1) = 40 > 32
    assert _raw_host(ctx, c["dims"], D, arrays, null=("sd",)) == -3                     # mean without sd
    assert _raw_host(ctx, c["dims"], D, arrays, null=("f_draw",)) == -3
    assert _raw_host(ctx, c["dims"], D, arrays, null=("rho",)) == -3
    assert _raw_host(ctx, c["dims"], D, arrays, null=("v0", "mean", "sd", "x_draw")) == 0
    holed = dict(arrays, x=c["x"].copy())
    holed["x"][0, T // 2, 1] = np.nan
    assert _raw_host(ctx, c["dims"], D, holed, flags=0) == -4                           # a NaN panel without the flag
    assert _raw_host(ctx, c["dims"], D, holed, flags=1) == 0
    assert _raw_host(ctx, c["dims"], D, arrays, flags=0) == 0                           # balanced: the H empty rows are the entry's own


def test_draw_paths_ar_idio_on_the_stock_watson_panel():
    """estimate(m, NonParametric()) -> api.draw_paths_ar_idio with through = lastperiod, H = 4 and 8 draws: shapes as
    forecast_ar_idio, observed cells the data, the draws those of the header on the arrays handed to the library; the model object
    is left as it was."""
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 4)
    api.estimate(m, api.NonParametric())
    before = {k: np.array(getattr(m, k), copy=True) for k in ("lambda_", "uar_coef", "uar_ser", "factor")}
    H, q, nd = 4, m.n_uarlag, 8
    out = api.draw_paths_ar_idio(m, nd, H, through=m.lastperiod, quantiles=[0.1, 0.9])
    fc = api.forecast_ar_idio(m, H, through=m.lastperiod)
    for k, v in before.items():
        assert np.array_equal(getattr(m, k), v, equal_nan=True), k + " was modified"
    n, r = fc["x"].shape[0], m.nfac_u
    assert np.array_equal(out["rows"], fc["rows"]) and np.array_equal(out["cols"], fc["cols"])
    assert out["x"].shape == (nd,) + fc["x"].shape and out["factor"].shape == (nd, n, r)
    assert out["x_sd"].shape == fc["x_sd"].shape and out["bands"].shape == (2,) + fc["x"].shape
    a = out["inputs"]
    obs = ~np.isnan(a["x"][q:])
    data = m.data[m.initperiod - 1 + q:m.lastperiod][:, out["cols"]]
    for k in range(nd):
        assert np.array_equal(out["x"][k, :n - H][obs], data[obs]), "an observed cell is not the data"
    assert np.all(out["x_sd"][:n - H][obs] == 0.0) and np.all(out["x_sd"][n - H:] > 0.0)
    assert np.all(out["bands"][0] <= out["bands"][1])
    for k in (0, nd - 1):
        f, x = se.draw(a["x"], *[a[key] for key in KEYS], H, 20160415, 0, k, 0, v0=a["v0"], mean=a["mean"], sd=np.ones_like(a["mean"]))
        _close(out["factor"][k] - out["mu_f"], f, f"draw {k} factor")
        _close(np.where(np.isnan(a["x"][q:]), out["x"][k, :n - H], x[:n - H]), x[:n - H], f"draw {k} x, in sample")
        _close(out["x"][k, n - H:], x[n - H:], f"draw {k} x, horizon")
