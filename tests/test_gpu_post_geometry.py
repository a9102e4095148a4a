"""GPU tests of the post-estimation products across the launch geometry of their cell kernels: dfm_forecast_batch
(forecast_fill_kernel), dfm_simsmooth_batch (simsmooth_diff_kernel / simsmooth_fill_kernel) and dfm_news_batch
(news_cov_panel_kernel, news_impact_kernel, news_gamma_kernel) against the expectation models of tests/forecast_expect.py,
tests/simsmooth_expect.py and tests/news_expect.py at 1e-9.

The cases are the enumerated table tests/post_geometry.py CASES; its plain-Python restatement of the launch geometry says which
classes each case hits (one, two and three or more series blocks, a last block with idle lanes, the 16-byte and the scalar cell
path, RC set by 8 G, by the LDS cap or by the row count, a partial last chunk, every loadings bucket, horizons 0, 1 and >= 40,
T + H = 32 / 33, and the pass routes under the products), and tests/test_post_geometry_cpu.py checks that the table covers every
class for each kernel family.  Every product of a case runs on the same panel and parameters."""
import functools

import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import varp_oracle as vo
from tests import post_geometry as pg
from tests.forecast_expect import expect as forecast_expect
from tests.news_expect import expect as news_expect
from tests.simsmooth_expect import draw

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("Lam", "R", "A", "Q", "mu0", "P0")
SEED = 20261017
D = 2
IDS = [row[0] for row in pg.CASES]


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
    assert np.all(np.isfinite(b)), f"{what}: the reference is not finite"
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print(f"  {what}: max abs error {err:.3e} (scale {scale:.3e})")
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _batch(B, N, T, r, missing):
    reps = [ko.synth_replicate(b, N, T, r, missing=missing) for b in range(B)]
    panel = np.stack([x for x, _ in reps])
    st = {k: np.stack([p[k] for _, p in reps]) for k in KEYS}
    st["mu0"] = st["mu0"] + 0.3                               # a non-zero prior mean
    return panel, st


def _varp_batch(B, N, T, r, p, missing):
    xs, qs = [], []
    for b in range(B):
        x = vo.synth_varp(b, N, T, r, p, missing=missing)
        q, _ = vo.varp_init(np.nan_to_num(x), r, p)
        xs.append(x); qs.append(dict(q, A=q["Avar"]))
    return np.stack(xs), {k: np.stack([q[k] for q in qs]) for k in KEYS}


def _mixed_batch(B, N, T, r, missing):
    """tests/test_gpu_chunk.py's mixed batch: even replicates have 12 series (padded with all-missing series to N), whose
    filter needs far more than a chunk to forget its start; odd replicates have N."""
    panels, sts = [], []
    for b in range(B):
        n = 12 if b % 2 == 0 else N
        x, p = ko.synth_replicate(b, n, T, r, missing=missing)
        xx = np.full((T, N), np.nan); xx[:, :n] = x
        Lam = np.zeros((N, r)); Lam[:n] = p["Lam"]
        R = np.ones(N); R[:n] = p["R"]
        panels.append(xx); sts.append(dict(p, Lam=Lam, R=R))
    return np.stack(panels), {k: np.stack([s[k] for s in sts]) for k in KEYS}


def _old_of(new, seed, last=2):
    """The old vintage as in tests/test_gpu_news.py: the last `last` rows not yet released, one cell revised afterwards, one
    gap filled."""
    rng = np.random.default_rng(seed)
    B, T, N = new.shape
    old = new.copy()
    old[:, T - last:, :] = np.nan
    new = new.copy()
    for b in range(B):
        obs = np.argwhere(~np.isnan(old[b]))
        t, i = obs[rng.integers(len(obs))]
        new[b, t, i] += 0.5                                   # a revision
        t, i = obs[rng.integers(len(obs))]
        old[b, t, i] = np.nan                                 # a gap the new vintage fills
    return old, new


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(case, panel, st, mean, sd) of a case, built once for its three products."""
    c = pg.case_dict(next(row for row in pg.CASES if row[0] == name))
    B, N, T, r, p = c["B"], c["N"], c["T"], c["r"], c["p"]
    if c["route"] == "chunked_fallback":
        panel, st = _mixed_batch(B, N, T, r, c["missing"])
    elif p == 1:
        panel, st = _batch(B, N, T, r, c["missing"])
    else:
        panel, st = _varp_batch(B, N, T, r, p, c["missing"])
    mean = sd = None
    if c["scaled"]:
        rng = np.random.default_rng(T * 1000 + N)
        mean, sd = rng.standard_normal((B, N)), rng.uniform(0.5, 3.0, (B, N))
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(sd)) and np.all(sd > 0.0)
    # a non-degenerate standardisation: every series with observed cells has two or more of them and a finite, positive spread
    # (the mixed batch's padding series are empty by construction)
    for b in range(B):
        n_obs = (~np.isnan(panel[b])).sum(axis=0)
        seen = n_obs > 0
        assert seen.any() and np.all(n_obs[seen] >= 2), f"{name}: an empty panel or a series with a single observed cell"
        s = np.nanstd(panel[b][:, seen], axis=0)
        assert np.all(np.isfinite(s)) and np.all(s > 0.0), f"{name}: a constant series"
    return c, panel, st, mean, sd


def _pick(a, b):
    return None if a is None else a[b]


def _routes(ctx):
    prof = ctx.profile_read()
    return sorted(k for k in prof if "recursion" in k or "collapse" in k or "pass_fused" in k)


def _geometry_line(c, fam):
    return "; ".join(f"{g['kernel']} nsblk={g['nsblk']} NPB={g['NPB']} G={g['G']} RC={g['RC']} nchunk={g['nchunk']} "
                     f"threads={g['threads']}" for g in pg.geometries(c)[fam])


def _check_route(c, nf, nt, S):
    """dfm_chunk_fallbacks after the call (its last pass, S replicates): the time-chunked recursion ran where the case says so."""
    if c["route"] == "chunked":
        assert nt == S and nf < nt, ("no replicate's pass came from the time-chunked recursion", nf, nt)
    elif c["route"] == "chunked_fallback":
        assert nt > 0, ("the pass did not run on the time-chunked recursion", nf, nt)
    elif c["route"] == "sequential":
        assert nt == 0, ("T is below the time-chunked recursion's minimum, yet it ran", nf, nt)


@pytest.mark.parametrize("name", IDS)
def test_forecast(ctx, name):
    c, panel, st, mean, sd = _inputs(name)
    H, p = c["H"], c["p"]
    print(f"\n{name}: {_geometry_line(c, 'forecast')}")
    ctx.profile_enable(True)
    got = ctx.forecast_batch_host(panel, *[st[k] for k in KEYS], H, mean=mean, sd=sd)
    nf, nt = ctx.chunk_fallbacks()
    print(f"  pass kernels {_routes(ctx)}; chunk fallbacks {nf} of {nt}")
    ctx.profile_enable(False)
    _check_route(c, nf, nt, c["B"])
    if c["route"] == "chunked_fallback":
        assert 0 < nf < nt, ("the batch did not mix chunked and sequential replicates", nf, nt)
    for b in range(c["B"]):
        e = forecast_expect(panel[b], *[st[k][b] for k in KEYS], H, p=p, mean=_pick(mean, b), sd=_pick(sd, b))
        tag = f"{name} b={b}"
        for key in ("xhat", "xvar", "common", "f", "P"):
            _close(got[key][b], e[key], f"{tag} {key}")
        assert np.isfinite(e["loglik"])
        err = abs(got["loglik"][b] - e["loglik"])
        print(f"  {tag} loglik: abs error {err:.3e} ({e['loglik']:.6e})")
        assert err <= TOL * abs(e["loglik"]), (tag, got["loglik"][b], e["loglik"])


@pytest.mark.parametrize("name", IDS)
def test_simsmooth(ctx, name):
    c, panel, st, mean, sd = _inputs(name)
    H, p = c["H"], c["p"]
    print(f"\n{name}: {_geometry_line(c, 'simsmooth')}")
    ctx.profile_enable(True)
    got = ctx.simsmooth_batch_host(panel, *[st[k] for k in KEYS], D, H, seed=SEED, mean=mean, sd=sd)
    nf, nt = ctx.chunk_fallbacks()
    print(f"  pass kernels {_routes(ctx)}; chunk fallbacks {nf} of {nt}")
    ctx.profile_enable(False)
    _check_route(c, nf, nt, c["B"] * D)
    for b in range(c["B"]):
        for d in range(D):
            f, xd = draw(panel[b], *[st[k][b] for k in KEYS], H, p, SEED, 0, d, b, mean=_pick(mean, b), sd=_pick(sd, b))
            _close(got["f"][b, d], f, f"{name} b={b} d={d} f")
            _close(got["x"][b, d], xd, f"{name} b={b} d={d} x")


@pytest.mark.parametrize("name", IDS)
def test_news(ctx, name):
    c, panel, st, mean, sd = _inputs(name)
    p = c["p"]
    tg = pg.targets(c)
    print(f"\n{name}: targets {tg}; KB={pg.news_gamma_kb(c['r'], p)}; {_geometry_line(c, 'news')}")
    old, new = _old_of(panel, c["T"] + c["N"])
    ctx.profile_enable(True)
    got = ctx.news_batch_host(old, new, *[st[k] for k in KEYS], tg, mean=mean, sd=sd)
    nf, nt = ctx.chunk_fallbacks()
    print(f"  pass kernels {_routes(ctx)}; chunk fallbacks of the weight passes {nf} of {nt}")
    ctx.profile_enable(False)
    _check_route(c, nf, nt, c["B"] * len(tg))
    for b in range(c["B"]):
        e = news_expect(old[b], new[b], *[st[k][b] for k in KEYS], tg, p=p, mean=_pick(mean, b), sd=_pick(sd, b))
        for key in ("yhat", "impact", "news", "weight"):
            _close(got[key][b], e[key], f"{name} b={b} {key}")
    # invariants: the impacts sum to y_new - y_rev; weight is 0 off the new vintage's cells
    y = got["yhat"]
    s = got["impact"].sum(axis=2)
    assert np.all(np.abs(s - (y[:, 2] - y[:, 1])) <= 1e-9 * np.maximum(1.0, np.abs(y[:, 2]))), f"{name}: sum of impacts"
    off = np.broadcast_to(np.isnan(new)[:, None], got["weight"].shape)
    assert np.all(got["weight"][off] == 0.0), f"{name}: weight off Omega_new"
