"""CPU checks of csrc/dfm_cell.h, the text the post-estimation cell kernels share: the loadings holder's dot product, the pair
kernels' dots (with a scaled load and an absent second series) and the packed quadratic form, compiled for the host
(tests/host/cell_host.cpp) in the register bucket of each r, against NumPy.

The bound: a dot product of r terms in any order of fused or plain operations carries at most r + 1 roundings of 1.1e-16 each
relative to the sum of the terms' magnitudes, the quadratic form r (r + 1) / 2 + 2 r of them -- 6e-14 at r = 32 in the worst case,
a few 1e-16 on drawn inputs; the inputs here are positive (a positive definite P with positive entries), so the sum of magnitudes
is the result itself and 1e-13 relative to the result holds at every r."""
import os
import subprocess

import numpy as np
import pytest

RS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("cell")), "cell_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "host", "cell_host.cpp")], check=True)
    return exe


def _ask(exe, requests):
    text = "".join(kind + " " + str(r) + " " + " ".join(float(x).hex() for x in vals) + "\n" for kind, r, vals in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests)
    return np.array([[float.fromhex(x) for x in line.split()] for line in out]).squeeze()


def test_dot_against_numpy(host_exe):
    g = np.random.default_rng(20)
    cases = [(r, g.uniform(0.1, 2.0, r), g.uniform(0.1, 2.0, r)) for r in RS for _ in range(8)]
    got = _ask(host_exe, [("dot", r, np.concatenate([lam, f])) for r, lam, f in cases])
    want = np.array([lam @ f for _, lam, f in cases])
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0.0)


def test_quadratic_form_against_numpy(host_exe):
    g = np.random.default_rng(21)
    cases = []
    for r in RS:
        for _ in range(8):
            L = g.uniform(0.0, 1.0, (r, r))
            P = L @ L.T + np.eye(r)                       # symmetric positive definite, every entry positive
            cases.append((r, g.uniform(0.1, 2.0, r), P))
    il = [np.tril_indices(r) for r, _, _ in cases]
    got = _ask(host_exe, [("quad", r, np.concatenate([lam, P[i]])) for (r, lam, P), i in zip(cases, il)])
    want = np.array([lam @ P @ lam for _, lam, P in cases])
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0.0)


def test_signed_inputs_stay_within_the_rounding_bound(host_exe):
    """Loadings and vectors of both signs: the error against the sum of the terms' magnitudes."""
    g = np.random.default_rng(22)
    cases = [(r, g.standard_normal(r), g.standard_normal(r)) for r in RS for _ in range(8)]
    got = _ask(host_exe, [("dot", r, np.concatenate([lam, f])) for r, lam, f in cases])
    for y, (r, lam, f) in zip(got, cases):
        assert abs(y - lam @ f) <= 1e-13 * np.abs(lam * f).sum()
    qc = []
    for r in RS:
        A = g.standard_normal((r, r))
        qc.append((r, g.standard_normal(r), A @ A.T))
    got = _ask(host_exe, [("quad", r, np.concatenate([lam, P[np.tril_indices(r)]])) for r, lam, P in qc])
    for y, (r, lam, P) in zip(got, qc):
        assert abs(y - lam @ P @ lam) <= 1e-13 * (np.abs(lam)[:, None] * np.abs(P) * np.abs(lam)[None, :]).sum()


def test_pair_dots_with_a_scaled_load_and_an_absent_series(host_exe):
    """CellLam<2, RB>::dots, what the pair kernels call: both series against NumPy with the loadings times sd at the load; with one
    series present the second result is exactly 0 and the first is unchanged to the bit."""
    g = np.random.default_rng(23)
    cases = [(r, g.uniform(0.1, 2.0, (2, r)), g.uniform(0.5, 3.0, 2), g.uniform(0.1, 2.0, r)) for r in RS for _ in range(4)]
    both = _ask_pair(host_exe, cases, 2)
    want = np.array([(sd[:, None] * lam) @ f for _, lam, sd, f in cases])
    np.testing.assert_allclose(both, want, rtol=1e-13, atol=0.0)
    one = _ask_pair(host_exe, cases, 1)
    assert np.array_equal(one[:, 0], both[:, 0]) and np.all(one[:, 1] == 0.0)


def _ask_pair(exe, cases, present):
    text = "".join(f"dots {r} {present} " + " ".join(float(x).hex() for x in np.concatenate([lam.ravel(), sd, f])) + "\n"
                   for r, lam, sd, f in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return np.array([[float.fromhex(x) for x in line.split()] for line in out])
