"""GPU tests of the four products of the model with AR(q) idiosyncratic terms -- dfm_forecast_ar_batch, dfm_simsmooth_ar_batch,
dfm_filter_ar_batch, dfm_gibbs_ar_batch -- at every template instance their launchers can reach and at every edge of their staged
chunks: the case table of tests/ar_post_geometry.py, whose coverage, geometry and conditioning tests/test_ar_post_geometry_cpu.py
checks without a device.  Each row runs every product that admits its shape on one panel and one set of parameters, against the
expectation model each product's own GPU test uses and at that test's tolerance, 1e-9 x max(1, scale): forecast_ar_expect.expect,
simsmooth_ar_expect.draw on the header's stream, filter_ar_expect.expect, gibbs_ar_expect.sweep started from the device's previous
state.  The references are computed once per process (ar_post_geometry's caches)."""
import numpy as np
import pytest

from tests import ar_post_geometry as apg
from tests import filter_ar_expect as fte
from tests import gibbs_ar_expect as gae

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = apg.KEYS
B, D = apg.B, apg.D
GIBBS_ALL = ("Lam", "sig2", "rho", "A", "Q", "f")
GIBBS_NAMES = [n for n in apg.NAMES if "gibbs" in apg.products(apg.case_dict(apg._row(n)))]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _close(a, b, what):
    """The comparison of tests/test_gpu_filter_ar.py: NaN positions exactly, the rest at 1e-9 of max(1, scale)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN positions differ"
    ok = ~np.isnan(b)
    if not ok.any():
        return
    scale = max(1.0, float(np.abs(b[ok]).max()))
    err = float(np.abs(a[ok] - b[ok]).max())
    print(f"{what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _st(c):
    return [c["st"][k] for k in KEYS]


def _scale_kw(c):
    return dict(mean=c["mean"], sd=c["sd"]) if c["scaled"] else {}


def _output_rows(c):
    """(the panel's output rows followed by the horizon [B, n, N], observed [B, n, N])."""
    xo = np.concatenate([c["x"], np.full((B, c["H"], c["N"]), np.nan)], axis=1)[:, c["q"]:]
    return xo, ~np.isnan(xo)


# ------------------------------------------------------------------------------------------------------------ the forecast
@pytest.mark.parametrize("name", apg.NAMES)
def test_forecast(ctx, name):
    """Every output against forecast_ar_expect.expect; observed cells of xhat the panel's bits (mean + sd x within two ulps when
    scaled, as the path draws' test has it); xvar exactly 0 on observed cells and positive elsewhere."""
    c = apg.make_case(name)
    N, T, q, H = c["N"], c["T"], c["q"], c["H"]
    got = ctx.forecast_ar_batch_host(c["x"], *_st(c), H, v0=c["v0"], **_scale_kw(c))
    exp = apg.forecast_expected(name)
    xo, obs = _output_rows(c)
    assert got["xhat"].shape == (B, T + H - q, N) and not obs[:, T - q:].any()
    for b in range(B):
        for k in ("xhat", "xvar", "common", "idio", "f", "P"):
            _close(got[k][b], exp[b][k], f"{name} b={b} {k}")
        assert abs(got["loglik"][b] - exp[b]["loglik"]) <= TOL * abs(exp[b]["loglik"]), (name, b, got["loglik"][b], exp[b]["loglik"])
    assert np.all(got["xvar"][obs] == 0.0), "xvar on an observed cell is not exactly 0"
    assert np.all(got["xvar"][~obs] > 0.0), "xvar on a missing cell is not positive"
    if c["scaled"]:
        prod = c["sd"][:, None, :] * xo
        want, ulp = c["mean"][:, None, :] + prod, 2.0 ** -52 * (np.abs(c["mean"][:, None, :]) + np.abs(prod))
        assert np.all(np.abs(got["xhat"][obs] - want[obs]) <= 2.0 * ulp[obs]), "observed cells are not mean + sd X"
    else:
        assert np.array_equal(got["xhat"][obs], xo[obs]), "observed cells are not the panel's bits"


# ------------------------------------------------------------------------------------------------------------ the path draws
@pytest.mark.parametrize("name", apg.NAMES)
def test_path_draws(ctx, name):
    """f_draw and x_draw of both draws against simsmooth_ar_expect.draw on the header's stream; observed cells bit for bit."""
    c = apg.make_case(name)
    N, T, r, q, H = c["N"], c["T"], c["r"], c["q"], c["H"]
    n = T + H - q
    got = ctx.simsmooth_ar_batch_host(c["x"], *_st(c), D, H, v0=c["v0"], seed=apg.SEED, **_scale_kw(c))
    ef, ex = apg.draws_expected(name)
    assert got["f"].shape == (B, D, n, r) and got["x"].shape == (B, D, n, N)
    _close(got["f"], ef, name + " f_draw")
    _close(got["x"], ex, name + " x_draw")
    xo, obs = _output_rows(c)
    assert np.all(np.isfinite(got["x"]))
    for d in range(D):
        if c["scaled"]:
            assert np.array_equal(got["x"][:, d][obs], got["x"][:, 0][obs]), "observed cells differ between draws"
            prod = c["sd"][:, None, :] * xo
            want, ulp = c["mean"][:, None, :] + prod, 2.0 ** -52 * (np.abs(c["mean"][:, None, :]) + np.abs(prod))
            assert np.all(np.abs(got["x"][:, d][obs] - want[obs]) <= 2.0 * ulp[obs]), "observed cells are not mean + sd X"
        else:
            assert np.array_equal(got["x"][:, d][obs], xo[obs]), "observed cells are not the panel's bits"
    assert np.all(got["x"][:, 0][~obs] != got["x"][:, 1][~obs]), "two draws share a missing cell's value"


@pytest.mark.parametrize("name", ["r4_n513", "r2_q3_n514", "drawedge"])
def test_first_draw_splits_a_call(ctx, name):
    """first_draw = 1 with D = 1 is draw 1 of the D = 2 call, bit for bit: on the three-block rows and where the horizon starts on the
    chunk edge."""
    c = apg.make_case(name)
    kw = dict(v0=c["v0"], seed=apg.SEED, **_scale_kw(c))
    full = ctx.simsmooth_ar_batch_host(c["x"], *_st(c), D, c["H"], **kw)
    part = ctx.simsmooth_ar_batch_host(c["x"], *_st(c), 1, c["H"], first_draw=1, **kw)
    assert np.array_equal(part["f"][:, 0], full["f"][:, 1]) and np.array_equal(part["x"][:, 0], full["x"][:, 1])


# ------------------------------------------------------------------------------------------------------------ the filter
def _filter(ctx, c, x=None, **kw):
    x = c["x"] if x is None else x
    return ctx.filter_ar_batch_host(x, *_st(c), may_have_missing=bool(np.isnan(x).any()), **kw)


@pytest.mark.parametrize("name", apg.NAMES)
def test_filter(ctx, name):
    """Every output of filter_ar_expect.OUTPUTS against filter_ar_expect.expect, cnt exactly; and the sum of loglik_t against the
    forecast entry's loglik at H = 0 -- the AR pass on the same panel -- as tests/test_gpu_filter_ar.py compares the two."""
    c = apg.make_case(name)
    H = apg.eval_horizons(c)
    got = _filter(ctx, c, H=H, t0=c["t0"], **_scale_kw(c))
    exp = apg.filter_expected(name)
    assert tuple(got) == fte.OUTPUTS
    for b in range(B):
        assert set(exp[b]) == set(fte.OUTPUTS if H > 0 else fte.OUTPUTS[:8])
        for k, v in exp[b].items():
            if k == "cnt":
                assert np.array_equal(got[k][b], v), f"{name} b={b} cnt"
            else:
                _close(got[k][b], v, f"{name} b={b} {k}")
    if H == 0:
        assert all(got[k] is None for k in ("msfe", "msfe_common", "msfe0", "cnt"))
    fc = ctx.forecast_ar_batch_host(c["x"], *_st(c), 0, v0=c["v0"], want=("loglik",))
    _close(got["loglik_t"].sum(axis=1), fc["loglik"], name + " sum of loglik_t against the AR pass")


@pytest.mark.parametrize("name", ["eval64", "eval65"])
def test_evaluation_sums_across_the_origin_chunk(ctx, name):
    """The running sums of a walk over more than one chunk of 64 origins are those of the same call split at the chunk: horizon h
    of the whole call (origins t0 .. T-1-h) against the first chunk alone (the panel cut behind row t0 + 63 + h) plus the call
    that starts at origin t0 + 64.  And the two origins either side of the chunk edge, each alone, against dfm_forecast_ar_batch
    on the panel cut at the origin: tests/test_gpu_filter_ar.py's single-origin check."""
    c = apg.make_case(name)
    T, q, t0, H = c["T"], c["q"], c["t0"], apg.eval_horizons(c)
    edge = t0 + apg.EVAL_CHUNK
    want = ("msfe", "msfe_common", "msfe0", "cnt")
    whole = _filter(ctx, c, H=H, t0=t0, want=want)
    if edge <= T - 2:
        tail = _filter(ctx, c, H=H, t0=edge, want=want)
        for h in range(1, H + 1):
            head = _filter(ctx, c, x=np.ascontiguousarray(c["x"][:, :edge + h]), H=h, t0=t0, want=want)
            ch, ct = head["cnt"][:, h - 1], tail["cnt"][:, h - 1]
            assert np.array_equal(whole["cnt"][:, h - 1], ch + ct) and ch.max() <= apg.EVAL_CHUNK
            for k in want[:3]:
                parts = np.where(ch > 0, head[k][:, h - 1] * ch, 0.0) + np.where(ct > 0, tail[k][:, h - 1] * ct, 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    _close(whole[k][:, h - 1], np.where(ch + ct > 0, parts / (ch + ct), np.nan), f"{name} h={h} {k} split at the chunk")
        assert (tail["cnt"][:, 0] == 1).sum() >= B * c["N"] // 2
    for o in (edge - 1, edge):
        if o > T - 2:
            continue
        one = _filter(ctx, c, x=np.ascontiguousarray(c["x"][:, :o + 2]), H=1, t0=o, want=("msfe", "cnt"))
        fc = ctx.forecast_ar_batch_host(np.ascontiguousarray(c["x"][:, :o + 1]), *_st(c), 1, want=())
        ok = one["cnt"][:, 0] == 1
        assert ok.sum() >= B * c["N"] // 2 and np.all(one["cnt"][:, 0] <= 1)
        _close(one["msfe"][:, 0][ok], ((c["x"][:, o + 1] - fc["xhat"][:, -1]) ** 2)[ok], f"{name} origin {o} against dfm_forecast_ar_batch")


# ------------------------------------------------------------------------------------------------------------ the Gibbs sweeps
def _gibbs(ctx, c):
    return ctx.gibbs_ar_batch_host(c["x"], *_st(c), c["prior"], apg.SWEEPS, may_have_missing=bool(np.isnan(c["x"]).any()),
                                   keep=GIBBS_ALL, seed=c["seed"])


@pytest.mark.parametrize("name", GIBBS_NAMES)
def test_gibbs_sweeps(ctx, name):
    """Every sweep of every chain against gibbs_ar_expect.sweep started from the device's previous state, as
    tests/test_gpu_gibbs_ar.py compares them (tests/test_ar_post_geometry_cpu.py: no accept of the table is decided within 1e-6 of
    its boundary); a second call gives the same bytes."""
    c = apg.make_case(name)
    state, d = _gibbs(ctx, c)
    for b in range(B):
        cur = {k: c["st"][k][b] for k in KEYS}
        for j in range(apg.SWEEPS):
            want = gae.sweep(c["x"][b], *[cur[k] for k in KEYS], c["prior"], c["seed"], j, b)
            for k in GIBBS_ALL:
                _close(d[k][b, j], want[k], f"{name} b={b} sweep={j} {k}")
            assert not (want["att_rho"] == gae.RHO_CAP).any()
            cur.update(Lam=d["Lam"][b, j], sig2=d["sig2"][b, j], rho=d["rho"][b, j], Avar=d["A"][b, j], Q=d["Q"][b, j])
    for k, dk in dict(Lam="Lam", sig2="sig2", rho="rho", Avar="A", Q="Q").items():
        assert np.array_equal(state[k], d[dk][:, -1]), f"the returned state is not the last sweep's {k}"
    again_state, again = _gibbs(ctx, c)
    for k in GIBBS_ALL:
        assert np.array_equal(d[k], again[k]), f"two runs differ in {k}"
