"""GPU tests of dfm_simulate_batch and dfm_simulate_ar_batch (include/dfm_hip.h; csrc/simulate.hip) against the contract of
tests/simulate_expect.py at 1e-9 x scale, the tolerance tests/test_gpu_simsmooth.py holds on the same random stream.

The cases come from two tables.  Each row fixes (r, p[, q], N, B, D, mask / panel / v0) and runs every T of `_plain_rows` /
`_ar_rows`, which take the chunk edges from the restated launch geometry (simulate_expect.plain_launch / ar_launch, held against
csrc/dfm_cellgeom.h by tests/test_simulate_cpu.py): one row short of a full chunk, a full chunk, one row more, and a partial last
chunk behind two full ones.  Plain: r just inside and just past every edge of dispatch_r_bucket with r p <= 32 (the LDS cap binds
at r = 32 on the one-lane blocks); N = 1 (one lane), 2, 7 (odd tail, scalar path), 8 (16-byte path), 513 and 514 (257 column
pairs in two series blocks of 129 lanes: the last lane of the second idles, and at 513 the last live lane holds one column) and
516 (258 pairs: no idle lane).  AR: q = 1 .. 4, both register buckets each q admits, N = 1, 2, 3, 256, 257 (the
second block starts at an odd series: every lane evaluates its own Philox block) and 514 (even starts: the pair exchange),
T = q + 1 (T = p where p > q + 1: the entry wants T >= p) and the chunk edges, with and without a panel, with and without v0."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import simsmooth_expect as sse
from tests import simulate_expect as sx

pytestmark = pytest.mark.gpu
TOL = 1e-9
SEED = 20261021
PLAIN = ("Lam", "R", "Avar", "Q", "mu0", "P0")
AR = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


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
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern"
    scale = max(1.0, float(np.nanmax(np.abs(b), initial=0.0)))
    err = float(np.nanmax(np.abs(a - b), initial=0.0))
    assert err <= TOL * scale, f"{what}: max abs error {err:.3e} (scale {scale:.3e})"


def _model(B, N, r, p, q=0, tag=0):
    """A stable model of the given shape: dict of stacked arrays (PLAIN or AR names), plus v0 [B, N]."""
    rng = np.random.default_rng([SEED, N, r, p, q, tag])
    m = max(p, q + 1) if q else p
    k = r * m
    st = dict(Lam=rng.standard_normal((B, N, r)), Q=np.empty((B, r, r)), P0=np.empty((B, k, k)), mu0=0.3 * rng.standard_normal((B, k)))
    st["R" if q == 0 else "sig2"] = rng.uniform(0.3, 1.5, (B, N))
    st["Avar"] = np.stack([np.hstack([(0.5 / p) * np.eye(r) + 0.2 / (p * np.sqrt(r)) * rng.standard_normal((r, r)) for _ in range(p)])
                           for _ in range(B)])
    for b in range(B):
        G = rng.standard_normal((r, r)); st["Q"][b] = G @ G.T / r + 0.2 * np.eye(r)
        H = rng.standard_normal((k, k)); st["P0"][b] = H @ H.T / k + 0.1 * np.eye(k)
    if q:
        st["rho"] = rng.uniform(-0.4, 0.5, (B, N, q)) / q
    return st, rng.uniform(0.5, 2.0, (B, N))


def _mask(B, T, N, tag, values=False):
    """A whole-NaN row, a whole-NaN column, scattered cells (NaN; 0 elsewhere, or N(0, 1) values for the AR panel)."""
    rng = np.random.default_rng([SEED, B, T, N, tag])
    x = rng.standard_normal((B, T, N)) if values else np.zeros((B, T, N))
    x[rng.uniform(size=x.shape) < 0.15] = np.nan
    x[:, T // 2, :] = np.nan
    if N > 2:
        x[:, :, N - 2] = np.nan
    x[0, 0, 0] = np.nan
    return x


def _expect_plain(st, T, b, d, seed=SEED, first_draw=0, mask=None):
    return sx.simulate(*[st[k][b] for k in PLAIN], T, seed, first_draw, d, b, mask=None if mask is None else mask[b])


def _expect_ar(st, T, b, d, seed=SEED, first_draw=0, panel=None, v0=None):
    return sx.simulate_ar(*[st[k][b] for k in AR], T, seed, first_draw, d, b, panel=None if panel is None else panel[b],
                          v0=None if v0 is None else v0[b])


def _check(got, expect, B, D, what):
    for b, d in itertools.product(range(B), range(D)):
        x, f = expect(b, d)
        _close(got["x"][b, d], x, f"{what} b={b} d={d} x")
        if got["f"] is not None:
            _close(got["f"][b, d], f, f"{what} b={b} d={d} f")


# ------------------------------------------------------------------------------------------------------------------ the tables
_P_OF_R = {1: 3, 4: 2, 5: 1, 8: 4, 9: 3, 16: 2, 17: 1, 32: 1}         # r p = 3, 8, 5, 32, 27, 32, 17, 32
_PLAIN_N = (1, 2, 7, 8, 513, 514, 516)
PLAIN_CASES = [(r, _P_OF_R[r], N, 1 + (i + j) % 2, (1, 3)[(i + j // 2) % 2], (i + j) % 3 != 0)
               for i, r in enumerate(_P_OF_R) for j, N in enumerate(_PLAIN_N)]
_AR_RP = {1: ((16, 1), (4, 3)), 2: ((9, 1), (5, 2)), 3: ((8, 1), (2, 5)), 4: ((6, 1), (1, 1))}   # k = r max(p, q + 1) <= 32
_AR_N = (1, 2, 3, 256, 257, 514)
AR_CASES = [(q,) + _AR_RP[q][j % 2] + (N, 1 + (q + j) % 2, (1, 3)[(q + j // 2) % 2], (q + j) % 2 == 0, (q + j // 3) % 2 == 0)
            for q in (1, 2, 3, 4) for j, N in enumerate(_AR_N)]


def _plain_rows(N, r):
    rc = sx.plain_launch(1, 1, N, r, 1 << 20)["RC"]                      # the full chunk: min(8 G, LDS cap)
    return sorted({rc - 1, rc, rc + 1, 2 * rc + 3} - {0})


def _ar_rows(N, r, p, q):
    """The shortest panel the entry admits (T = q + 1; T = p where the factors have more lags than that) and the chunk edges."""
    rc = sx.ar_launch(1, 1, N, r, q, (1 << 20) + q)["RC"]
    return sorted({max(q + 1, p), q + rc - 1, q + rc, q + rc + 1, q + 2 * rc + 3})


def test_tables_cover_what_they_claim():
    assert {(c[0], c[2]) for c in PLAIN_CASES} == set(itertools.product(_P_OF_R, _PLAIN_N))
    assert all(r * p <= 32 for r, p in _P_OF_R.items()) and {sx.plain_launch(1, 1, 8, r, 9)["RB"] for r in _P_OF_R} == {4, 8, 16, 32}
    assert {c[4] for c in PLAIN_CASES} == {1, 3} and {c[3] for c in PLAIN_CASES} == {1, 2} and {c[5] for c in PLAIN_CASES} == {True, False}
    assert any(sx.plain_launch(1, 1, N, 32, max(_plain_rows(N, 32)))["cap_binds"] for N in (1, 2))
    assert {(c[0], c[3]) for c in AR_CASES} == set(itertools.product((1, 2, 3, 4), _AR_N))
    assert all(r * max(p, q + 1) <= 32 for q, v in _AR_RP.items() for r, p in v)
    assert {(c[6], c[7]) for c in AR_CASES} == set(itertools.product((True, False), repeat=2))
    assert sx.ar_launch(1, 1, 257, 4, 1, 40)["paired"] == (True, False) and all(sx.ar_launch(1, 1, 514, 4, 1, 40)["paired"])
    for N, r in ((513, 8), (514, 8), (516, 8)):
        g = sx.plain_launch(1, 1, N, r, 40)
        assert g["nsblk"] == 2 and g["idle_last"] == (N != 516)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: "r{}_p{}_n{}_b{}_d{}_{}".format(*c[:5], "mask" if c[5] else "bal"))
def test_plain_against_the_contract(ctx, case):
    r, p, N, B, D, masked = case
    st, _ = _model(B, N, r, p)
    for T in _plain_rows(N, r):
        if T < p:
            continue
        mask = _mask(B, T, N, r) if masked else None
        got = ctx.simulate_batch_host(*[st[k] for k in PLAIN], D, T=T, mask_panel=mask, seed=SEED)
        assert got["x"].shape == (B, D, T, N) and got["f"].shape == (B, D, T, r)
        _check(got, lambda b, d: _expect_plain(st, T, b, d, mask=mask), B, D, f"plain T={T}")


@pytest.mark.parametrize("case", AR_CASES, ids=lambda c: "q{}_r{}_p{}_n{}_b{}_d{}_{}_{}".format(
    *c[:6], "panel" if c[6] else "free", "v0" if c[7] else "sig2"))
def test_ar_against_the_contract(ctx, case):
    q, r, p, N, B, D, with_panel, with_v0 = case
    st, v0 = _model(B, N, r, p, q)
    for T in _ar_rows(N, r, p, q):
        panel = _mask(B, T, N, q, values=True) if with_panel else None
        got = ctx.simulate_ar_batch_host(*[st[k] for k in AR], D, T=T, panel=panel, v0=v0 if with_v0 else None, seed=SEED)
        assert got["x"].shape == (B, D, T, N) and got["f"].shape == (B, D, T - q, r)
        _check(got, lambda b, d: _expect_ar(st, T, b, d, panel=panel, v0=v0 if with_v0 else None), B, D, f"ar T={T}")
        if with_panel:
            rows = np.broadcast_to(panel[:, None, :q], (B, D, q, N))
            assert np.array_equal(got["x"][:, :, :q], rows, equal_nan=True), "rows < q are not the panel's bit for bit"


# ------------------------------------------------------------------------------------------------------------------ both entries
def _both(ctx):
    """(name, host call, device call, expectation, B, D) of a small masked case of each entry."""
    B, D, T, N, r, p, q = 2, 3, 37, 8, 4, 2, 2
    stp, _ = _model(B, N, r, p, tag=1)
    mask = _mask(B, T, N, 91)
    sta, v0 = _model(B, N, r, p, q, tag=1)
    panel = _mask(B, T, N, 92, values=True)
    import torch
    dev = lambda a: None if a is None else torch.as_tensor(a, device=f"cuda:{ctx.device}")
    plain = dict(
        host=lambda **kw: ctx.simulate_batch_host(*[stp[k] for k in PLAIN], **dict(dict(D=D, T=T, mask_panel=mask, seed=SEED), **kw)),
        dev=lambda **kw: ctx.simulate_batch(*[dev(stp[k]) for k in PLAIN], D=D, T=T, mask_panel=dev(mask), seed=SEED, **kw),
        expect=lambda b, d, **kw: _expect_plain(stp, T, b, d, mask=mask, **kw), st=stp)
    ar = dict(
        host=lambda **kw: ctx.simulate_ar_batch_host(*[sta[k] for k in AR], **dict(dict(D=D, T=T, panel=panel, v0=v0, seed=SEED), **kw)),
        dev=lambda **kw: ctx.simulate_ar_batch(*[dev(sta[k]) for k in AR], D=D, T=T, panel=dev(panel), v0=dev(v0), seed=SEED, **kw),
        expect=lambda b, d, **kw: _expect_ar(sta, T, b, d, panel=panel, v0=v0, **kw), st=sta)
    return dict(plain=plain, ar=ar), B, D


@pytest.mark.parametrize("which", ["plain", "ar"])
def test_split_repeat_device_and_no_f(ctx, which):
    e, B, D = _both(ctx)
    e = e[which]
    one = e["host"]()
    _check(one, e["expect"], B, D, which)
    again = e["host"]()                                                  # repeated calls on one handle agree
    assert np.array_equal(one["x"], again["x"], equal_nan=True) and np.array_equal(one["f"], again["f"])
    head, tail = e["host"](D=1), e["host"](D=D - 1, first_draw=1)        # a call split by first_draw equals one call
    assert np.array_equal(np.concatenate([head["x"], tail["x"]], axis=1), one["x"], equal_nan=True)
    assert np.array_equal(np.concatenate([head["f"], tail["f"]], axis=1), one["f"])
    nof = e["host"](want_f=False)                                        # f_sim NULL: the path lives in the handle, same x_sim
    assert nof["f"] is None and np.array_equal(nof["x"], one["x"], equal_nan=True)
    on = e["dev"]()                                                      # host bytes equal device bytes
    ctx.synchronize()
    assert np.array_equal(on["x"].cpu().numpy(), one["x"], equal_nan=True) and np.array_equal(on["f"].cpu().numpy(), one["f"])
    on = e["dev"](want_f=False)
    ctx.synchronize()
    assert on["f"] is None and np.array_equal(on["x"].cpu().numpy(), one["x"], equal_nan=True)


@pytest.mark.parametrize("which", ["plain", "ar"])
def test_rank_one_q_and_no_mask(ctx, which):
    B, D, T, N, r, p, q = 1, 2, 20, 7, 3, 2, (0 if which == "plain" else 2)
    st, v0 = _model(B, N, r, p, q, tag=2)
    v = np.array([[1.0, -0.5, 0.25]])
    st["Q"] = (v.T @ v)[None]                                            # rank 1: the root rule gives one column
    st["P0"][0, 0] = st["P0"][0, :, 0] = 0.0                             # and a rank-deficient P0
    if which == "plain":
        got = ctx.simulate_batch_host(*[st[k] for k in PLAIN], D, T=T, seed=SEED + 4)
        _check(got, lambda b, d: _expect_plain(st, T, b, d, seed=SEED + 4), B, D, "rank-1 Q")
    else:
        got = ctx.simulate_ar_batch_host(*[st[k] for k in AR], D, T=T, v0=v0, seed=SEED + 4)
        _check(got, lambda b, d: _expect_ar(st, T, b, d, seed=SEED + 4, v0=v0), B, D, "rank-1 Q (AR)")
    assert not np.isnan(got["x"]).any()


@pytest.mark.parametrize("which", ["plain", "ar"])
def test_across_the_slice_of_the_path_kernel(ctx, which):
    """B D = 8200 pass replicates: two launches of the path kernel; draws either side of the boundary against the contract."""
    D, T, N, r, q = sx.SLICE + 8, 4, 2, 1, (0 if which == "plain" else 1)
    st, _ = _model(1, N, r, 1, q, tag=3)
    if which == "plain":
        got = ctx.simulate_batch_host(*[st[k] for k in PLAIN], D, T=T, seed=SEED + 5, want_f=False)
        expect = lambda d: _expect_plain(st, T, 0, d, seed=SEED + 5)[0]
    else:
        got = ctx.simulate_ar_batch_host(*[st[k] for k in AR], D, T=T, seed=SEED + 5, want_f=False)
        expect = lambda d: _expect_ar(st, T, 0, d, seed=SEED + 5)[0]
    for d in (0, sx.SLICE - 1, sx.SLICE, D - 1):
        _close(got["x"][0, d], expect(d), f"{which} d={d}")


def test_plain_is_the_smoothers_x_plus(ctx):
    """x_sim = X - D with D the difference panel of dfm_simsmooth_batch's step 2, rebuilt from simsmooth_expect's own texts."""
    B, D, T, N, r, p = 1, 2, 30, 9, 3, 2
    st, _ = _model(B, N, r, p, tag=4)
    X = _mask(B, T, N, 93, values=True)
    got = ctx.simulate_batch_host(*[st[k] for k in PLAIN], D, T=T, mask_panel=X, seed=SEED + 6)
    Lam, R, A, Q, mu0, P0 = (st[k][0] for k in PLAIN)
    for d in range(D):
        nz = sse.stream_normals(SEED + 6, 0, d, 0, T, 0, N, r, p)
        fp = np.empty((T, r))
        sse._recursion(A, sse.psd_root(Q), nz["eta"], mu0 + sse.psd_root(P0) @ nz["n0"], range(T), fp)
        Dp = np.where(np.isnan(X[0]), np.nan, X[0] - (fp @ Lam.T + np.sqrt(R) * nz["eps_plus"]))
        _close(got["x"][0, d], X[0] - Dp, f"X - D, d={d}")


def test_status_codes(ctx):
    buf = np.ones(1 << 16)
    out = np.empty(1 << 16)
    P = ctypes.c_void_p(buf.ctypes.data)
    O = ctypes.c_void_p(out.ctypes.data)

    def plain(B, D, T, N, r, p, x=O, dev=False):
        fn = ctx._lib.dfm_simulate_batch_dev if dev else ctx._lib.dfm_simulate_batch
        return fn(ctx._h, B, D, T, N, r, p, None, P, P, P, P, P, P, 1, 0, x, None, 0)

    def ar(B, D, T, N, r, p, q, x=O, dev=False):
        fn = ctx._lib.dfm_simulate_ar_batch_dev if dev else ctx._lib.dfm_simulate_ar_batch
        return fn(ctx._h, B, D, T, N, r, p, q, None, P, P, P, P, P, P, P, None, 1, 0, x, None, 0)

    for dev in (False, True):
        assert plain(1, 0, 10, 4, 2, 1, dev=dev) == -1                   # D < 1: DFM_E_DIMS
        assert plain(1, 2, 2, 4, 2, 3, dev=dev) == -1                    # T < p
        assert plain(1, 2, 10, 4, 17, 2, dev=dev) == -1                  # r p > DFM_MAX_R
        assert plain(1, 2, 10, 4, 33, 1, dev=dev) == -1
        assert plain(0, 2, 10, 4, 2, 1, dev=dev) == -1 and plain(1, 2, 10, 0, 2, 1, dev=dev) == -1
        assert plain(1, 2, 10, 4, 2, 1, x=None, dev=dev) == -3           # x_sim NULL: DFM_E_NULL
        assert ar(1, 0, 10, 4, 2, 1, 2, dev=dev) == -1                   # D < 1
        assert ar(1, 2, 2, 4, 2, 1, 2, dev=dev) == -1                    # T <= q
        assert ar(1, 2, 3, 4, 2, 4, 2, dev=dev) == -1                    # T < p
        assert ar(1, 2, 10, 4, 2, 1, 0, dev=dev) == -1 and ar(1, 2, 10, 4, 2, 1, 5, dev=dev) == -1   # q outside 1 .. 4
        assert ar(1, 2, 10, 4, 11, 1, 2, dev=dev) == -1                  # r (q + 1) > DFM_MAX_R
        assert ar(1, 2, 10, 4, 2, 1, 2, x=None, dev=dev) == -3           # x_sim NULL
    assert plain(1, 2, 10, 4, 2, 1) == 0 and ar(1, 2, 10, 4, 2, 1, 2) == 0   # (the same calls, admitted)
    with pytest.raises(ValueError):
        ctx.simulate_batch_host(buf[:8].reshape(1, 4, 2), buf[:4].reshape(1, 4), buf[:4].reshape(1, 2, 2), buf[:4].reshape(1, 2, 2),
                                buf[:2].reshape(1, 2), buf[:4].reshape(1, 2, 2), 0, T=5)
