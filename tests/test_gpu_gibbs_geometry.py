"""GPU tests of the parameter block of dfm_gibbs_batch -- gibbs_gram_kernel, gibbs_load_kernel<RB, MISS>, gibbs_var_kernel
(csrc/gibbs.hip) -- at every instance of the load kernel and at every edge of the staged chunks: the case table of
tests/gibbs_geometry.py, whose coverage, geometry and conditioning tests/test_gibbs_geometry_cpu.py checks without a device.  Each
row runs SWEEPS sweeps of B chains once per process and is held to the expectation model of tests/gibbs_expect.py at the tolerance
of tests/test_gpu_gibbs.py, 1e-9 x max(1, scale), twice: the whole sweep, started from the device's previous state, and the block
alone, from the device's own factor path of the sweep -- Lam, R, A and Q are functions of (panel, f, prior, stream) only, so the
second comparison speaks of gibbs.hip and not of the simulation smoother."""
import numpy as np
import pytest

from oracle import synth_oracle as so
from tests import gibbs_expect as ge
from tests import gibbs_geometry as gg

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = gg.KEYS
ALL = ("Lam", "R", "A", "Q", "f")
B = gg.B
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


def _gibbs(ctx, c, flag=None):
    return ctx.gibbs_batch_host(c["x"], *[c["st"][k] for k in KEYS], c["prior"], gg.SWEEPS, keep=ALL, seed=c["seed"],
                                may_have_missing=c["flag"] if flag is None else flag)


def _run(ctx, name):
    """The row's run under its own flag, once per process: (state, draws), read only."""
    if name not in _RUNS:
        state, d = _gibbs(ctx, gg.make_case(name))
        for v in list(state.values()) + list(d.values()):
            v.setflags(write=False)
        _RUNS[name] = (state, d)
    return _RUNS[name]


def _err(a, b):
    """(max abs error, scale) as tests/test_gpu_gibbs.py's _close has them."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), "the device's draw is not finite"
    return float(np.abs(a - b).max()) if a.size else 0.0, max(1.0, float(np.abs(b).max())) if b.size else 1.0


def _series_report(a, b, touched):
    """The largest error over the series the edge pattern touched and over the others, for a failure message."""
    e = np.abs(np.asarray(a) - np.asarray(b)).reshape(len(touched), -1).max(axis=1)
    worst = int(e.argmax())
    part = lambda m: f"{e[m].max():.3e}" if m.any() else "none"
    return (f"series with a missing cell: {part(touched)}, series without: {part(~touched)}, worst series {worst} "
            f"({'with' if touched[worst] else 'without'} a missing cell)")


def _compare(name, what, got, want, keys, touched, worst):
    for k in keys:
        err, scale = _err(got[k], want[k])
        worst[k] = max(worst.get(k, 0.0), err / scale)
        extra = "; " + _series_report(got[k], want[k], touched) if k in ("Lam", "R") else ""
        assert err <= TOL * scale, f"{name} {what} {k}: max abs error {err:.3e} (scale {scale:.3e}){extra}"


# ------------------------------------------------------------------------------------------------------------ the two comparisons
@pytest.mark.parametrize("name", gg.NAMES)
def test_every_sweep_matches_the_model(ctx, name):
    """Sweep j of the model starts from the device's state after sweep j - 1; every one of Lam, R, A, Q, f."""
    c = gg.make_case(name)
    state, d = _run(ctx, name)
    touched = gg.edge_series(c)
    for k, dk in (("Lam", "Lam"), ("R", "R"), ("Avar", "A"), ("Q", "Q")):
        assert np.array_equal(state[k], d[dk][:, -1]), f"the returned state is not the last sweep's {k}"
    worst = {}
    try:
        for b in range(B):
            pr = gg.chain_prior(c, b)
            cur = {k: c["st"][k][b] for k in KEYS}
            for j in range(gg.SWEEPS):
                want = ge.sweep(c["x"][b], *[cur[k] for k in KEYS], c["p"], pr, c["seed"], j, b)
                assert want["att_R"].max() < ge.GAMMA_CAP and want["att_Q"].max() < ge.GAMMA_CAP
                _compare(name, f"b={b} sweep={j}", {k: d[k][b, j] for k in ALL}, want, ALL, touched[b], worst)
                cur.update(Lam=d["Lam"][b, j], R=d["R"][b, j], A=d["A"][b, j], Q=d["Q"][b, j])
    finally:
        print(f"{name}: whole sweep, largest error / scale per key " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("name", gg.NAMES)
def test_the_block_alone_matches_the_model_on_the_devices_path(ctx, name):
    """gibbs_expect.draw_loadings and draw_var on the device's kept f of sweep j, on the header's streams, against the device's
    Lam, R, A and Q of that sweep."""
    c = gg.make_case(name)
    _, d = _run(ctx, name)
    touched = gg.edge_series(c)
    worst = {}
    try:
        for b in range(B):
            pr = gg.chain_prior(c, b)
            for j in range(gg.SWEEPS):
                rnd = ge.stream_randoms(c["seed"], j, b, c["T"], c["N"], c["r"], c["p"])
                f = d["f"][b, j]
                Lam, R, _ = ge.draw_loadings(c["x"][b], f, pr, rnd["lam_n"], rnd["gam_R"])
                A, Q, _ = ge.draw_var(f, c["p"], pr, rnd["E"], rnd["bart_n"], rnd["gam_Q"])
                _compare(name, f"b={b} sweep={j} given the device's f,", {k: d[k][b, j] for k in ALL[:4]}, dict(Lam=Lam, R=R, A=A, Q=Q),
                         ALL[:4], touched[b], worst)
    finally:
        print(f"{name}: block alone, largest error / scale per key " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------ per series
def test_a_series_without_a_cell_draws_from_the_priors_moments(ctx):
    """R_i = (nu_R s_R / 2) / Gamma(nu_R / 2) and lam_i = sqrt(R_i / tau_lam) z_i on the header's streams, sweep after sweep: a draw,
    not the start left alone."""
    names = [n for n in gg.NAMES if gg.case_dict(gg._row(n))["empty"] is not None]
    assert names
    for name in names:
        c = gg.make_case(name)
        i, pr, N, r = c["empty"], c["prior"], c["N"], c["r"]
        _, d = _run(ctx, name)
        for b in range(B):
            for j in range(gg.SWEEPS):
                key = so.replicate_key(c["seed"], j)
                z, u = ge.gamma_attempts(key, 16 * b + 6, N)
                g, _ = ge.gamma_mt(0.5 * pr["nu_R"], z[:, i:i + 1], u[:, i:i + 1])
                Ri = 0.5 * pr["nu_R"] * pr["s_R"] / g[0]
                lam = np.sqrt(Ri / pr["tau_lam"]) * ge.stream_randoms(c["seed"], j, b, c["T"], N, r, c["p"])["lam_n"][i]
                where = f"{name} b={b} sweep={j} series {i}"
                assert abs(d["R"][b, j, i] - Ri) <= TOL * max(1.0, Ri), (where, d["R"][b, j, i], Ri)
                assert np.abs(d["Lam"][b, j, i] - lam).max() <= TOL * max(1.0, np.abs(lam).max()), (where, d["Lam"][b, j, i], lam)
                assert d["R"][b, j, i] != c["st"]["R"][b, i] and np.all(d["Lam"][b, j, i] != c["st"]["Lam"][b, i]), where
            assert d["R"][b, 0, i] != d["R"][b, 1, i]


def test_series_with_one_cell_are_drawn(ctx):
    """The kinds 4 to 6 of the edge pattern: n_i = 1, the cell in the row before the edge, behind it, or in the last row.  Each such
    series against the model on the device's path, one by one (the rows' own comparison covers them; this one names them)."""
    met = 0
    for name in (n for n in gg.NAMES if gg.case_dict(gg._row(n))["pattern"] == "edge"):
        c = gg.make_case(name)
        _, d = _run(ctx, name)
        for b in range(B):
            one = np.nonzero((~np.isnan(c["x"][b])).sum(0) == 1)[0]
            rnd = ge.stream_randoms(c["seed"], 0, b, c["T"], c["N"], c["r"], c["p"])
            Lam, R, _ = ge.draw_loadings(c["x"][b], d["f"][b, 0], gg.chain_prior(c, b), rnd["lam_n"], rnd["gam_R"])
            for i in one:
                row = int(np.nonzero(~np.isnan(c["x"][b, :, i]))[0][0])
                assert abs(d["R"][b, 0, i] - R[i]) <= TOL * max(1.0, R[i]), (name, b, i, row)
                assert np.abs(d["Lam"][b, 0, i] - Lam[i]).max() <= TOL * max(1.0, np.abs(Lam[i]).max()), (name, b, i, row)
            met += len(one)
    assert met >= 3 * B


# ------------------------------------------------------------------------------------------------------------ the two routes of a bucket
@pytest.mark.parametrize("name", gg.BUCKET_ROWS)
def test_the_flag_changes_the_kernels_and_not_the_draws(ctx, name):
    """A balanced row under the may-have-missing flag runs gibbs_load_kernel<RB, true> and no gram kernel; its draws are those of the
    run without the flag at the tolerance (the factor paths of the two runs come from two routes of the pass)."""
    c = gg.make_case(name)
    assert not c["flag"] and not np.isnan(c["x"]).any()
    names = []
    for flag in (False, True):
        ctx.profile_enable(True)
        try:
            _, d = _gibbs(ctx, c, flag=flag)
            names.append((set(ctx.profile_read()), d))
        finally:
            ctx.profile_enable(False)
    (off, d_off), (on, d_on) = names
    assert "gibbs_gram_kernel" in off and "gibbs_gram_kernel" not in on, (sorted(off), sorted(on))
    assert "gibbs_load_kernel" in off and "gibbs_load_kernel" in on and "gibbs_var_kernel" in off and "gibbs_var_kernel" in on
    for k in ALL:
        assert np.array_equal(d_off[k], _run(ctx, name)[1][k]), f"profiling changed {k}"
        err, scale = _err(d_on[k], d_off[k])
        print(f"{name}: flag on against flag off, {k} {err / scale:.3e}")
        assert err <= TOL * scale, f"{name} {k}: flag on against flag off {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("name", gg.REPEAT_ROWS)
def test_two_runs_give_the_same_bytes(ctx, name):
    """No floating-point atomics: every sum runs in one fixed order."""
    c = gg.make_case(name)
    state, d = _run(ctx, name)
    again_state, again = _gibbs(ctx, c)
    for k in ALL:
        assert np.array_equal(d[k], again[k]), f"two runs differ in {k}"
    for k in state:
        assert np.array_equal(state[k], again_state[k]), f"two runs differ in the state's {k}"
