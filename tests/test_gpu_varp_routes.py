"""The VAR(p) companion pass and EM (dfm_ks_pass_varp_batch / dfm_em_varp_batch) on every recursion route of tests/varp_routes.py,
against oracle/varp_oracle.py.  Tolerances are those of tests/test_gpu_varp.py: 1e-9 on the pass (relative on the log-likelihood, of
max(1, largest entry) on the moments), 1e-8 on the EM (relative on the log-likelihood path, of max(1, largest entry) on the six
parameter arrays and the smoothed moments); the host entries repeat the device entries to 1e-12.  The kernel name in the handle's
profile guards the table: a later change of dispatch turns a row red instead of silently making it a copy of another.  The last
test prints the largest attained error of every route group next to its tolerance."""
import os

import numpy as np
import pytest

from conftest import diag_only

from tests import varp_routes as vr

pytestmark = pytest.mark.gpu
KEYS = vr.KEYS
PASS_TOL, EM_TOL, HOST_TOL = 1e-9, 1e-8, 1e-12
ALL = [(row.name, v) for row in vr.ROWS for v in vr.VARIANTS]
SHORT = [(name, v) for name in vr.ONE_PER_CLASS for v in vr.VARIANTS]
DIAG = [(name, v) for name in vr.DIAG_ROWS["DFM_NO_RECURSION_WAVE"] for v in vr.VARIANTS]
RECURSIONS = {vr.K_LANE, vr.K_WAVE, vr.K_MBF16, vr.K_COMP}
ATTAINED = {}                        # route group -> {figure: largest attained error in units of its tolerance's scale}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dynamic_factor_models_amd import DfmContext
    c = DfmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_lane():
    """A handle created under DFM_NO_RECURSION_WAVE=1 (diagnostics build): RouteOpts::no_rec_wave belongs to the handle, the
    environment is put back before the handle is used."""
    from dynamic_factor_models_amd import DfmContext
    old = os.environ.get("DFM_NO_RECURSION_WAVE")
    os.environ["DFM_NO_RECURSION_WAVE"] = "1"
    try:
        c = DfmContext()
    finally:
        if old is None:
            os.environ.pop("DFM_NO_RECURSION_WAVE", None)
        else:
            os.environ["DFM_NO_RECURSION_WAVE"] = old
    yield c
    c.close()


def _num_cu(c):
    import torch
    return torch.cuda.get_device_properties(c.device).multi_processor_count


def _group(rt):
    return rt.instance.rsplit(", ", 1)[0] + ">" if rt.kernel == vr.K_WAVE else rt.instance


def _note(group, figure, err):
    g = ATTAINED.setdefault(group, {})
    g[figure] = max(g.get(figure, 0.0), float(err))
    return float(err)


def _err(got, want):
    """Largest deviation in units of max(1, largest entry): what test_gpu_varp.py's _close bounds."""
    return np.abs(np.asarray(got) - want).max() / max(1.0, np.abs(want).max())


def _problem(c, name, variant):
    """The row's batch (its distinct replicates tiled over it), the replicates to check, the route the table expects."""
    row = vr.BY_NAME[name]
    x, q = vr.inputs(name, variant)
    B = vr.batch(row, _num_cu(c))
    idx = np.arange(B) % x.shape[0]
    check = sorted(set(range(min(B, x.shape[0]))) | {B - 1})
    kw = dict(singular_q=row.singular, may_have_missing=False if variant == "balanced" else None)
    return row, x[idx], {k: q[k][idx] for k in KEYS}, idx, check, kw


def _profiled(c, call):
    """call() under the handle's profile: its result and the names of the kernels it launched."""
    import torch
    c.profile_enable(True)
    try:
        out = call()
        torch.cuda.synchronize()
        prof = c.profile_read()
    finally:
        c.profile_enable(False)
    return out, {n for n, (_, launches) in prof.items() if launches >= 1}


def _guard(rt, launched, what):
    assert rt.kernel in launched and not (RECURSIONS - {rt.kernel}) & launched, (what, rt.instance, sorted(launched))


def _check_pass(c, name, variant, wave=True, want_P=True):
    import torch
    row, x, q, idx, check, kw = _problem(c, name, variant)
    rt = vr.route(row.r, row.p, row.singular, wave, x.shape[1], x.shape[0], _num_cu(c))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", c.device))
    (f, P, ll), launched = _profiled(c, lambda: c.ks_pass_varp_batch(t(x), *[t(q[k]) for k in KEYS], want_P=want_P, **kw))
    _guard(rt, launched, name)
    assert f.shape == (x.shape[0], x.shape[1], row.r) and (P is None) == (not want_P)
    ref = vr.pass_reference(name, variant)
    g, bad = _group(rt), []
    for b in check:
        o = ref[idx[b]]
        e = [_note(g, "pass loglik", abs(ll[b].item() - o["loglik"]) / abs(o["loglik"])),
             _note(g, "pass f_smooth", _err(f[b].cpu().numpy(), o["f_smooth"]))]
        if want_P:
            e.append(_note(g, "pass P_smooth", _err(P[b].cpu().numpy(), o["P_smooth"])))
        print(f"{name} {variant} {rt.instance} pass b={b}: " + " ".join(f"{v:.2e}" for v in e))
        bad += [(b, v) for v in e if not v <= PASS_TOL]
    assert not bad, (name, variant, rt.instance, bad)


def _check_em(c, name, variant, wave=True):
    import torch
    row, x, q, idx, check, kw = _problem(c, name, variant)
    rt = vr.route(row.r, row.p, row.singular, wave, x.shape[1], x.shape[0], _num_cu(c))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", c.device))
    d = {k: t(q[k]) for k in KEYS}
    (path, its, f, P), launched = _profiled(c, lambda: c.em_varp_batch(t(x), *[d[k] for k in KEYS], max_iter=vr.EM_ITERS, tol=0.0, **kw))
    _guard(rt, launched, name)
    B, T = x.shape[:2]
    assert d["Avar"].shape == (B, row.r, row.r * row.p) and d["Q"].shape == (B, row.r, row.r)
    assert f.shape == (B, T, row.r) and P.shape == (B, T, row.r * (row.r + 1) // 2) and path.shape == (B, vr.EM_ITERS)
    assert (its.cpu().numpy() == vr.EM_ITERS).all()
    ref = vr.em_reference(name, variant)
    g, bad = _group(rt), []
    for b in check:
        o = ref[idx[b]]
        e = [_note(g, "em path", np.abs(path[b].cpu().numpy() / o["path"] - 1.0).max())]
        e += [_note(g, "em " + k, _err(d[k][b].cpu().numpy(), o[k])) for k in KEYS]
        e += [_note(g, "em f_smooth", _err(f[b].cpu().numpy(), o["f_smooth"])), _note(g, "em P_smooth", _err(P[b].cpu().numpy(), o["P_smooth"]))]
        print(f"{name} {variant} {rt.instance} em b={b}: " + " ".join(f"{v:.2e}" for v in e))
        bad += [(b, v) for v in e if not v <= EM_TOL]
    assert not bad, (name, variant, rt.instance, bad)


@pytest.mark.parametrize("name,variant", ALL)
def test_pass(ctx, name, variant):
    _check_pass(ctx, name, variant)


@pytest.mark.parametrize("name,variant", SHORT)
def test_pass_without_P_smooth(ctx, name, variant):
    _check_pass(ctx, name, variant, want_P=False)


@pytest.mark.parametrize("name,variant", ALL)
def test_em(ctx, name, variant):
    _check_em(ctx, name, variant)


@pytest.mark.parametrize("name,variant", SHORT)
def test_host_entries_repeat_the_device_entries(ctx, name, variant):
    import torch
    row, x, q, idx, check, kw = _problem(ctx, name, variant)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    dev = [a.cpu().numpy() for a in ctx.ks_pass_varp_batch(t(x), *[t(q[k]) for k in KEYS], **kw)]
    for a, b_, what in zip(ctx.ks_pass_varp_batch_host(x, *[q[k] for k in KEYS], **kw), dev, ("f_smooth", "P_smooth", "loglik")):
        assert rel(a, b_) <= HOST_TOL, (name, variant, "pass", what, rel(a, b_))
    d = {k: t(q[k]) for k in KEYS}
    path, its, f, P = ctx.em_varp_batch(t(x), *[d[k] for k in KEYS], max_iter=vr.EM_ITERS, tol=0.0, **kw)
    new, hpath, hits, hf, hP = ctx.em_varp_batch_host(x, *[q[k] for k in KEYS], max_iter=vr.EM_ITERS, tol=0.0, **kw)
    assert new["Avar"].shape == (x.shape[0], row.r, row.r * row.p) and new["Q"].shape == (x.shape[0], row.r, row.r)
    assert np.array_equal(hits, its.cpu().numpy())
    for k in KEYS:
        assert rel(new[k], d[k].cpu().numpy()) <= HOST_TOL, (name, variant, "em", k, rel(new[k], d[k].cpu().numpy()))
    for a, b_, what in ((hpath, path, "path"), (hf, f, "f_smooth"), (hP, P, "P_smooth")):
        assert rel(a, b_.cpu().numpy()) <= HOST_TOL, (name, variant, "em", what, rel(a, b_.cpu().numpy()))
    x0, q0 = vr.inputs(name, variant)                               # the host entry leaves its inputs alone
    assert all(np.array_equal(q[k], q0[k][idx]) for k in KEYS) and np.array_equal(x, x0[idx], equal_nan=True)


@diag_only()
@pytest.mark.parametrize("name,variant", DIAG)
def test_pass_on_the_lane_groups_at_16_and_32(ctx_lane, name, variant):
    """recursion_kernel<16 | 32, true> on a companion state: what production takes beyond the wave kernels' 150 KB of LDS."""
    _check_pass(ctx_lane, name, variant, wave=False)


@diag_only()
@pytest.mark.parametrize("name,variant", DIAG)
def test_em_on_the_lane_groups_at_16_and_32(ctx_lane, name, variant):
    _check_em(ctx_lane, name, variant, wave=False)


def test_attained_errors_report(capsys):
    """Not a check of the library: the figures the tests above attained, per route group, next to their tolerances."""
    with capsys.disabled():
        print(f"\nVAR(p) routes, largest attained error (pass tolerance {PASS_TOL:.0e}, EM tolerance {EM_TOL:.0e}):")
        for g in sorted(ATTAINED):
            a = ATTAINED[g]
            em_par = max([v for k, v in a.items() if k[3:] in KEYS] or [float("nan")])
            print(f"  {g:32s} pass: loglik {a.get('pass loglik', float('nan')):.1e} f {a.get('pass f_smooth', float('nan')):.1e} "
                  f"P {a.get('pass P_smooth', float('nan')):.1e} | em: path {a.get('em path', float('nan')):.1e} parameters {em_par:.1e} "
                  f"f {a.get('em f_smooth', float('nan')):.1e} P {a.get('em P_smooth', float('nan')):.1e}")
