"""CPU checks of the structural feature (dfm_irf_batch / dfm_histdecomp_batch): the expectation model of
tests/structural_expect.py against the reference-style impulse_response and against its own invariants, the status codes the
library decides without a device, the api's refusals, the binding of dynamic_factor_models_amd/structural.py against a call
recorder and _lib.SYMBOLS, and tests/structural_geometry.py against csrc/structural.hip.  No kernel is launched here."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from dynamic_factor_models_amd import _lib, api, kalman, structural
from tests import post_geometry as pg
from tests import structural_expect as se
from tests import structural_geometry as sg
from tests.api_calls import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(N=24, r=3, p=2, T=100, first=0):
    x, st = se.synth(1, N, T, r, p, first=first)
    return x[0], {k: v[0] for k, v in st.items()}


def _rot(r, seed=5):
    g = np.random.default_rng(seed)
    while True:
        M = g.standard_normal((r, r)) + 2.0 * np.eye(r)
        if np.linalg.cond(M) < 20:
            return M


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("r,p", [(3, 1), (3, 2), (2, 3)])
def test_model_irf_equals_the_var_models_impulse_response(r, p):
    _, q = _one(r=r, p=p)
    H = 9
    named = se.greedy_named(q["Lam"])
    e = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], H, named=named)
    k = r * p
    v = api._var_model(np.zeros((30, r)), nlag=p)
    v.Q = np.hstack([q["Lam"], np.zeros((q["Lam"].shape[0], k - r))])
    v.M = se.companion(q["A"])
    v.G = np.vstack([se.impact(q["Lam"], q["Q"], named), np.zeros((k - r, r))])
    want = api.impulse_response(v, "all", H)                      # [N, H, r]
    np.testing.assert_allclose(e["irf"].transpose(2, 1, 0), want, rtol=1e-10, atol=1e-12)


def test_rotation_invariance_needs_named_series():
    _, q = _one()
    H, M = 8, _rot(3)
    named = se.greedy_named(q["Lam"])
    cum = np.arange(q["Lam"].shape[0]) % 3 == 0
    sd = np.linspace(0.5, 2.0, q["Lam"].shape[0])
    L2, A2, Q2 = se.rotate(q["Lam"], q["A"], q["Q"], M)
    a = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], H, sd=sd, named=named, cum=cum)
    b = se.irf_fevd(L2, A2, Q2, q["R"], H, sd=sd, named=named, cum=cum)
    np.testing.assert_allclose(b["irf"], a["irf"], rtol=0, atol=1e-10 * np.abs(a["irf"]).max())
    np.testing.assert_allclose(b["fevd"], a["fevd"], rtol=0, atol=1e-10)
    a0 = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], H)
    b0 = se.irf_fevd(L2, A2, Q2, q["R"], H)
    assert np.abs(b0["irf"] - a0["irf"]).max() > 1e-3 * np.abs(a0["irf"]).max(), "chol(Q) should depend on the rotation"


def test_impact_block_is_lower_triangular_with_a_unit_diagonal_under_unit_effect():
    _, q = _one(r=3, p=1)
    named = se.greedy_named(q["Lam"])
    sd = np.linspace(0.5, 2.0, q["Lam"].shape[0])
    e = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], 4, sd=sd, named=named)
    blk = e["irf"][:, 0, named].T                                 # [named series, shock]
    assert np.abs(np.triu(blk, 1)).max() <= 1e-12 * np.abs(blk).max()
    u = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], 4, sd=sd, named=named, unit_effect=True)
    blk = u["irf"][:, 0, named].T
    assert np.abs(np.triu(blk, 1)).max() <= 1e-12 and np.array_equal(np.diag(blk), np.ones(3))
    np.testing.assert_array_equal(u["fevd"], e["fevd"])           # the normalisation scales the IRF only


def test_fevd_slots():
    _, q = _one()
    N = q["Lam"].shape[0]
    cum = np.arange(N) % 2 == 1
    H = 10
    e = se.irf_fevd(q["Lam"], q["A"], q["Q"], q["R"], H, named=se.greedy_named(q["Lam"]), cum=cum)
    np.testing.assert_allclose(e["fevd"].sum(axis=0), 1.0, rtol=0, atol=1e-14)
    assert np.all(np.diff(e["num"], axis=1) >= 0.0)
    np.testing.assert_array_equal(e["idio"][:, cum], np.arange(1, H + 1)[:, None] * q["R"][cum])
    np.testing.assert_array_equal(e["idio"][:, ~cum], np.broadcast_to(q["R"][~cum], (H, (~cum).sum())))


@pytest.mark.parametrize("r,p", [(3, 1), (2, 3)])
def test_histdecomp_slots_sum_to_the_common_component(r, p):
    x, q = _one(r=r, p=p, T=60)
    f, _ = se.smooth(x, *[q[k] for k in se.KEYS], p=p)
    e = se.histdecomp(f, q["Lam"], q["A"], q["Q"], named=se.greedy_named(q["Lam"]))
    want = f @ q["Lam"].T
    assert np.abs(e["hd"].sum(axis=0) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.all(e["shocks"][:p] == 0.0) and np.all(e["paths"][:r, :p] == 0.0)
    # rotation invariance of the decomposition and of the shocks
    L2, A2, Q2 = se.rotate(q["Lam"], q["A"], q["Q"], _rot(r))
    e2 = se.histdecomp(f @ _rot(r).T, L2, A2, Q2, named=se.greedy_named(q["Lam"]))
    np.testing.assert_allclose(e2["hd"], e["hd"], rtol=0, atol=1e-9 * np.abs(e["hd"]).max())
    np.testing.assert_allclose(e2["shocks"], e["shocks"], rtol=0, atol=1e-9 * np.abs(e["shocks"]).max())


def test_case_table_is_well_conditioned_and_reaches_every_launch_class():
    for row in sg.IRF_CASES:
        c = sg.irf_case(row)
        _, st = se.synth(2, c["N"], 8 if c["p"] == 1 else 100, c["r"], c["p"])
        for b in range(2):
            assert np.linalg.cond(st["Lam"][b][se.greedy_named(st["Lam"][b])]) <= 100.0, c["name"]
    cl = sg.irf_classes()
    assert {sp for sp, _, _ in cl} == {1, 2} and {nb for _, nb, _ in cl} == {1, 2, 3} and {ch for _, _, ch in cl} == {False, True}
    assert {(c[2], c[3]) for c in sg.IRF_CASES} >= {(r, 1) for r in (1, 2, 4, 8, 9, 16, 17, 32)} | {(3, 2), (4, 4), (2, 3), (1, 12), (8, 4)}
    assert {c[1] for c in sg.IRF_CASES} == {7, 60, 139, 200, 513, 1025} and {c[4] for c in sg.IRF_CASES} == {1, 2, 12, 41}


# ------------------------------------------------------------------------------------------------------------ geometry
def test_geometry_restatement_matches_the_source():
    src = open(os.path.join(ROOT, "dynamic_factor_models_amd", "csrc", "structural.hip")).read()
    const = lambda n: re.search(rf"constexpr \w+ {n} = ([0-9 *]+);", src).group(1)
    assert eval(const("kSvIrfLanes")) == sg.IRF_LANES and eval(const("kSvFillMaxThreads")) == sg.FILL_MAX_THREADS
    assert eval(const("kSvFillLds")) == sg.FILL_LDS and eval(const("kSvPathMaxThreads")) == sg.PATH_MAX_THREADS
    assert eval(const("kSvPathLds")) == sg.PATH_LDS
    # irf_geometry: N = 200 pairs in one block of 100 lanes; misaligned: two blocks of 100 single series; r = 32: 5 Theta rows of
    # 8 KiB under the cap, 2 with the cumulated table beside them
    g = sg.irf_fill(1024, 200, 8, 40, False)
    assert (g["SP"], g["nsblk"], g["NPB"], g["threads"], g["RC"], g["grid"]) == (2, 1, 100, 128, 40, 1024)
    g = sg.irf_fill(2, 200, 8, 12, False, aligned=False)
    assert (g["SP"], g["nsblk"], g["NPB"]) == (1, 2, 100)
    assert sg.irf_fill(2, 60, 32, 41, False)["RC"] == 5 and sg.irf_fill(2, 1025, 32, 12, True)["RC"] == 2
    assert sg.irf_fill(2, 200, 17, 2, False)["SP"] == 1 and sg.irf_fill(2, 200, 16, 2, False)["SP"] == 2
    # launch_hd_r uses cell_geometry: N = 200 gives 5 x 100 of 512, N = 139 gives 3 x 139 of 448
    g = sg.hd_fill(1, 200, 8, 500)
    assert (g["SP"], g["G"], g["NPB"], g["threads"], g["RC"]) == (2, 5, 100, 512, 40)
    g = sg.hd_fill(1, 139, 8, 222)
    assert (g["SP"], g["G"], g["NPB"], g["threads"]) == (1, 3, 139, 448)
    # path_geometry: r = 8 runs its 9 chains in one workgroup of 72 lanes; r = 32 needs two groups of 32 and 1 chain
    assert (sg.path(8, 1)["CP"], sg.path(8, 1)["groups"], sg.path(8, 1)["threads"]) == (9, 1, 128)
    assert (sg.path(32, 1)["CP"], sg.path(32, 1)["groups"], sg.path(32, 1)["threads"]) == (32, 2, 1024)
    for r, p in [(1, 1), (1, 12), (1, 32), (8, 4), (20, 1), (32, 1), (16, 2), (3, 2)]:
        g = sg.path(r, p)
        assert g["lds"] <= sg.PATH_LDS and g["TC"] >= 1 and g["CP"] * r * p <= sg.PATH_MAX_THREADS


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return pg.build_cellgeom_host(tmp_path_factory.mktemp("cellgeom"))


def test_geometry_restatement_matches_the_host_functions(host_exe):
    """irf_fill, hd_fill and path against irf_geometry, cell_geometry and path_geometry of csrc/dfm_cellgeom.h compiled for the host,
    field for field: the rows of IRF_CASES, then N = 1..1100 x r x (H, with and without the cumulated table | T), and every (r, p)."""
    irf_q = [(c["N"], c["r"], c["H"], c["cum"], not c["misaligned"]) for c in map(sg.irf_case, sg.IRF_CASES)]
    irf_q += [(N, r, H, cum, True) for N, r, H, cum in itertools.product(pg.SWEEP_N, pg.SWEEP_R, (1, 2, 12, 41), (False, True))]
    hd_q = list(itertools.product(pg.SWEEP_N, pg.SWEEP_R, pg.SWEEP_ROWS))
    path_q = [(r, p) for r in range(1, 33) for p in range(1, 33) if r * p <= 32]
    want, req = [], []
    for N, r, H, cum, aligned in irf_q:
        g = sg.irf_fill(1, N, r, H, cum, aligned)
        want.append(tuple(g[f] for f in pg.GEOM_FIELDS))
        req.append(("irf", N, r, g["SP"], H, int(cum), sg.IRF_LANES, sg.FILL_LDS))
    for N, r, T in hd_q:
        g = sg.hd_fill(1, N, r, T)
        want.append(tuple(g[f] for f in pg.GEOM_FIELDS))
        req.append(("cell", (N + g["SP"] - 1) // g["SP"], r, T, sg.FILL_MAX_THREADS, sg.FILL_LDS))
    for r, p in path_q:
        g = sg.path(r, p)
        want.append((g["CP"], g["TC"], g["groups"], g["threads"], g["lds"]))
        req.append(("path", r, p, sg.PATH_MAX_THREADS, sg.PATH_LDS))
    got = pg.ask_cellgeom_host(host_exe, req)
    bad = [(q, w, g) for q, w, g in zip(req, want, got) if w != g]
    assert not bad, bad[:5]
    assert len(path_q) == sum(32 // r for r in range(1, 33)) and {q[3] for q in req if q[0] == "irf"} == {1, 2}


def test_sp_rule_matches_cell_sp(host_exe):
    """The SP of irf_fill and hd_fill (the bucket is R = r itself) against cell_sp of csrc/dfm_cellgeom.h."""
    assert pg.check_sp_rule(host_exe, lambda N, r, al: sg.irf_fill(1, N, r, 12, False, aligned=al)["SP"]) == {1, 2}
    assert pg.check_sp_rule(host_exe, lambda N, r, al: sg.hd_fill(1, N, r, 40, aligned=al)["SP"]) == {1, 2}


# ------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes_without_a_device():
    lib = _lib.load()
    named = (ctypes.c_int * 2)(0, 1)
    rep = (ctypes.c_int * 2)(1, 1)
    far = (ctypes.c_int * 2)(0, 5)
    none9, none13 = [None] * 9, [None] * 13
    assert lib.dfm_irf_batch(None, 1, 5, 2, 1, 3, *none9, 0) == -3                 # NULL handle
    assert lib.dfm_irf_batch_dev(None, 1, 5, 2, 1, 3, *none9, 0) == -3
    assert lib.dfm_histdecomp_batch(None, 1, 9, 5, 2, 1, *none13, 0) == -3
    assert lib.dfm_histdecomp_batch_dev(None, 1, 9, 5, 2, 1, *none13, 0) == -3
    for fn in (lib.dfm_irf_batch, lib.dfm_irf_batch_dev):                          # sizes are decided before the handle
        assert fn(None, 1, 5, 2, 1, 0, *none9, 0) == -1                            # H < 1
        assert fn(None, 0, 5, 2, 1, 3, *none9, 0) == -1
        assert fn(None, 1, 5, 2, 0, 3, *none9, 0) == -1                            # p < 1
        assert fn(None, 1, 40, 9, 4, 3, *none9, 0) == -2                           # r p > 32
        args = [None] * 5 + [ctypes.cast(rep, ctypes.c_void_p)] + [None] * 3
        assert fn(None, 1, 5, 2, 1, 3, *args, 0) == -1                             # a repeated named series
        args[5] = ctypes.cast(far, ctypes.c_void_p)
        assert fn(None, 1, 5, 2, 1, 3, *args, 0) == -1                             # a named series outside [0, N)
        args[5] = ctypes.cast(named, ctypes.c_void_p)
        assert fn(None, 1, 5, 2, 1, 3, *args, 0) == -3
    for fn in (lib.dfm_histdecomp_batch, lib.dfm_histdecomp_batch_dev):
        assert fn(None, 1, 2, 5, 2, 2, *none13, 0) == -1                           # T = p
        assert fn(None, 1, 1, 5, 2, 1, *none13, 0) == -1
        assert fn(None, 1, 9, 5, 9, 4, *none13, 0) == -2


def test_api_refuses_before_any_device_work():
    x = np.random.default_rng(0).standard_normal((40, 7))
    m = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    for call in (lambda: api.structural_irf(m, 4), lambda: api.historical_decomposition(m)):
        with pytest.raises(ValueError, match="not been estimated"):
            call()
    with pytest.raises(ValueError, match="H must be"):
        api.structural_irf(m, 0)
    g = np.random.default_rng(1)
    m.em_params = dict(Lam=g.standard_normal((7, 2)), R=np.ones(7), A=0.5 * np.eye(2), Q=np.eye(2), mu0=np.zeros(2), P0=np.eye(2))
    with pytest.raises(ValueError, match="unit_effect needs named"):
        api.structural_irf(m, 4, unit_effect=True)
    with pytest.raises(ValueError, match="quantile bands need named"):
        api.structural_irf(m, 4, quantiles=[0.5])
    with pytest.raises(ValueError, match="bootstrap replicates"):
        api.structural_irf(m, 4, named=[0, 1], quantiles=[0.5])
    with pytest.raises(ValueError, match="2 distinct"):
        api.structural_irf(m, 4, named=[1, 1])
    with pytest.raises(ValueError, match="through must lie"):
        api.historical_decomposition(m, through=3)
    m2 = api.DFMModel(x, [1, 1, 0, 1, 1, 1, 1], 5, 5, 1, 40, 0, 2, 1e-8, 4, 4)
    m2.em_params = dict(m.em_params, Lam=m.em_params["Lam"][:6], R=np.ones(6))
    for call in (lambda: api.structural_irf(m2, 4, named=[0, 2]), lambda: api.structural_irf(m2, 4, cumulate=[2]),
                 lambda: api.historical_decomposition(m2, named=[2, 0])):
        with pytest.raises(ValueError, match="series 2 is not among"):
            call()
    mo = api.DFMModel(x, np.ones(7), 5, 5, 1, 40, 1, 2, 1e-8, 4, 4)
    mo.em_params = m.em_params
    for call in (lambda: api.structural_irf(mo, 4), lambda: api.historical_decomposition(mo)):
        with pytest.raises(ValueError, match="nfac_o = 0"):
            call()
    if not torch.cuda.is_available():                             # and past the refusals there is no CPU fallback
        with pytest.raises(RuntimeError, match="HIP device"):
            api.structural_irf(m, 4, named=[0, 1])


# ------------------------------------------------------------------------------------------------------------ the binding
B, T, N, r, p, H = 2, 12, 6, 2, 3, 4
HANDLE = 0xD0F0


class _OnDevice(torch.Tensor):
    is_cuda = True


def make_ctx():
    ctx = kalman.DfmContext.__new__(kalman.DfmContext)
    ctx._lib, ctx._h, ctx._torch, ctx._use_torch_stream, ctx.device = Recorder(), ctypes.c_void_p(HANDLE), torch, False, 0
    ctx._dev = lambda t, name, shape=None: kalman.DfmContext._dev(ctx, t.as_subclass(_OnDevice), name, shape)
    return ctx


def arrays():
    g = np.random.default_rng(0)
    k = r * p
    return dict(panel=g.standard_normal((B, T, N)), Lam=g.standard_normal((B, N, r)), R=g.random((B, N)) + 1,
                Avar=g.standard_normal((B, r, k)), Q=g.standard_normal((B, r, r)), mu0=g.standard_normal((B, k)),
                P0=g.standard_normal((B, k, k)), sd=g.random((B, N)) + 1)


def addr(a):
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def val(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


def one_call(lib, name):
    assert [c[0] for c in lib.calls] == [name]
    args = lib.calls[0][1]
    kinds = _lib.SYMBOLS[name][1]
    assert len(args) == len(kinds)
    for i, (x, kind) in enumerate(zip(args, kinds)):
        if kind in (ctypes.c_int, ctypes.c_uint):
            assert type(x) is int, (name, i)
        else:
            assert x is None or isinstance(x, ctypes.c_void_p), (name, i)
    lib.calls.clear()
    return args


def both(ctx, name, a):
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    return ((getattr(ctx, name), f"dfm_{name}_dev", t), (getattr(ctx, name + "_host"), f"dfm_{name}", a))


def shaped(x, shape, like):
    assert tuple(x.shape) == shape and type(x) is (torch.Tensor if isinstance(like, torch.Tensor) else np.ndarray)
    return x


def test_irf_binding():
    ctx, a = make_ctx(), arrays()
    assert ctx.irf_batch_host.__func__ is structural.irf_batch_host
    for call, sym, s in both(ctx, "irf_batch", a):
        for full in (True, False):
            named = [3, 1] if full else None
            cum = [0, 1, 0, 0, 1, 0] if full else None
            got = call(s["Lam"], s["Avar"], s["Q"], s["R"], H, sd=s["sd"] if full else None, named=named, cum=cum,
                       unit_effect=full, want_fevd=full)
            args = one_call(ctx._lib, sym)
            assert val(args[0]) == HANDLE and args[1:6] == (B, N, r, p, H)
            assert [val(x) for x in args[6:11]] == [addr(s[k]) for k in ("Lam", "Avar", "Q", "R")] + [addr(s["sd"]) if full else None]
            if full:
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[11], ctypes.POINTER(ctypes.c_int)), (r,)), named)
                assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(args[12], ctypes.POINTER(ctypes.c_int)), (N,)), cum)
            else:
                assert args[11] is None and args[12] is None
            assert list(got) == ["irf", "fevd"] and shaped(got["irf"], (B, r, H, N), s["Lam"]) is got["irf"]
            assert got["fevd"] is None if not full else shaped(got["fevd"], (B, r + 1, H, N), s["Lam"]) is got["fevd"]
            assert [val(x) for x in args[13:]] == [addr(got["irf"]), addr(got["fevd"]), _lib.DFM_SV_UNIT_EFFECT if full else 0]
        with pytest.raises(ValueError, match="H must be"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], 0)
        with pytest.raises(ValueError, match="distinct"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, named=[1, 1])
        with pytest.raises(ValueError, match="unit_effect"):
            call(s["Lam"], s["Avar"], s["Q"], s["R"], H, unit_effect=True)
        assert not ctx._lib.calls


@pytest.mark.parametrize("mhm,bit", [(True, _lib.DFM_F_MAY_HAVE_MISSING), (False, 0), (None, 0)])
@pytest.mark.parametrize("sq", [False, True])
def test_histdecomp_binding(mhm, bit, sq):
    ctx, a = make_ctx(), arrays()
    for call, sym, s in both(ctx, "histdecomp_batch", a):
        for full in (True, False):
            got = call(s["panel"], *[s[k] for k in ("Lam", "R", "Avar", "Q", "mu0", "P0")], sd=s["sd"] if full else None,
                       named=[4, 0] if full else None, want_shocks=full, may_have_missing=mhm, singular_q=sq)
            args = one_call(ctx._lib, sym)
            assert val(args[0]) == HANDLE and args[1:6] == (B, T, N, r, p)
            assert [val(x) for x in args[6:13]] == [addr(s[k]) for k in ("panel", "Lam", "R", "Avar", "Q", "mu0", "P0")]
            assert val(args[13]) == (addr(s["sd"]) if full else None) and (args[14] is None) == (not full)
            assert list(got) == ["hd", "shocks", "f", "loglik"]
            shaped(got["hd"], (B, r + 1, T, N), s["panel"]); shaped(got["f"], (B, T, r), s["panel"]); shaped(got["loglik"], (B,), s["panel"])
            assert got["shocks"] is None if not full else shaped(got["shocks"], (B, T, r), s["panel"]) is got["shocks"]
            assert [val(x) for x in args[15:]] == [addr(got[k]) for k in got] + [bit | (_lib.DFM_F_SINGULAR_Q if sq else 0)]


def test_kalman_names_none_of_the_structural_symbols():
    src = open(kalman.__file__).read()
    assert "dfm_irf_batch" not in src and "dfm_histdecomp_batch" not in src
    assert {"dfm_irf_batch", "dfm_irf_batch_dev", "dfm_histdecomp_batch", "dfm_histdecomp_batch_dev"} <= set(_lib.SYMBOLS)
