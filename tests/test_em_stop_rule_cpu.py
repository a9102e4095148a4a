"""CPU check of the EM stop rule's comparison: em_improved of csrc/dfm_em_epilogue.h, the one text every kernel calls, compiled for the
host (tests/host/em_stop_host.cpp) against the expression of oracle/kalman_oracle.py em().  The kernels around it are compared with
the oracle in tests/test_gpu_em_stop.py."""
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle import kalman_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emstop") / "em_stop_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "em_stop_host.cpp")], check=True)
    return exe


def _oracle_stops(ll, llp, tol):
    """oracle/kalman_oracle.py em(): `if (path[-1] - path[-2]) / (0.5 * (abs(path[-1]) + abs(path[-2]))) < tol: break`."""
    ll, llp = np.float64(ll), np.float64(llp)                  # (path entries are NumPy doubles: 0 / 0 is NaN, not an exception)
    with np.errstate(all="ignore"):
        return bool((ll - llp) / (0.5 * (abs(ll) + abs(llp))) < tol)


def _ask(exe, triples):
    blob = np.asarray(triples, dtype=np.float64).tobytes()
    out = subprocess.run([exe], input=blob, capture_output=True, check=True).stdout
    assert len(out) == len(triples)
    return np.frombuffer(out, dtype=np.uint8).astype(bool)


def test_the_oracle_still_has_the_expression_restated_here():
    src = inspect.getsource(ko.em)
    assert "(path[-1] - path[-2]) / (0.5 * (abs(path[-1]) + abs(path[-2]))) < tol" in src


def test_em_improved_agrees_with_the_oracle_expression(host_exe):
    lls = [-1234.5, -1.0, -1e-3, 1e-3, 2.5, 9876.0]
    steps = [0.0, 1e-12, 1e-7, 1e-4, 1e-2, -1e-7, -1e-2]        # ll == llp, increases, decreases (relative to |llp|)
    tols = [0.0, 1e-8, 1e-4, 1e-2]
    triples = [(llp + s * abs(llp), llp, tol) for llp, s, tol in itertools.product(lls, steps, tols)]
    triples += [(a, b, tol) for a, b in [(-5.0, 5.0), (5.0, -5.0), (-3.0, 2.0), (2.0, -3.0)] for tol in tols]   # across zero
    nan = float("nan")
    triples += [(nan, -10.0, 1e-4), (-10.0, nan, 1e-4), (nan, nan, 1e-4), (nan, -10.0, 0.0), (0.0, 0.0, 1e-4)]
    go = _ask(host_exe, triples)
    want = np.array([not _oracle_stops(*t) for t in triples])
    assert np.array_equal(go, want), [t for t, g, w in zip(triples, go, want) if g != w]
    # what the grid has to contain
    assert want.any() and not want.all()
    t = dict(zip(triples, go))
    assert t[(-1234.5, -1234.5, 1e-4)] == False and t[(-1234.5, -1234.5, 0.0)] == True     # ll == llp: 0 < tol stops, 0 < 0 does not
    assert t[(-1234.5 - 1e-2 * 1234.5, -1234.5, 0.0)] == False                              # a decrease stops even at tol = 0 ...
    assert all(go[-5:-1])                                                                   # ... a NaN on either side goes on
    assert go[-1]                                                                           # 0 / 0 = NaN as well
