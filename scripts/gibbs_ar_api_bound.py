"""The figures tests/test_gpu_gibbs_ar.py::test_estimate_bayesian_ar_idio_on_the_stock_watson_panel asks the device for, from the
expectation model (tests/gibbs_ar_expect.py) on the same stream: api.estimate_bayesian_ar_idio on the Stock-Watson panel with the
test's chains, burn, draws and seed, restated in NumPy from the same start (api._ar_model_inputs after estimate(m,
NonParametric())).  Prints
  max |common_mean - mean|     the largest posterior-mean common component, in deviation from the fixed series mean
  mean persistence_mean        the mean over the series of the posterior mean of sum_l rho_il
for the start itself and for a start moved by 1e-9 (relative in Lam, sig2, Q; absolute in rho, Avar), their difference (the drift
the test's margin is derived from) and the smallest distance of any accept decision from its boundary.

    python scripts/gibbs_ar_api_bound.py                  # the start from the device (estimate(m, NonParametric()))
    python scripts/gibbs_ar_api_bound.py --dump start.npz # only write that start
    python scripts/gibbs_ar_api_bound.py --inputs start.npz   # no device: the model alone (a few minutes of CPU)
"""
import argparse
import concurrent.futures as cf
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import gibbs_ar_expect as gae  # noqa: E402

CHAINS, BURN, KEPT, SEED = 2, 4, 6, 77
NAMES = ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0")


def start_from_the_device():
    from dynamic_factor_models_amd import api
    d = np.load(os.path.join(ROOT, "tests", "golden", "sw_panel.npz"))
    m = api.DFMModel(d["bpdata"], d["inclcode"], 20, 40, 3, 224, 0, 4, 1e-8, 4, 4)
    api.estimate(m, api.NonParametric())
    inputs, _, _, _ = api._ar_model_inputs(m)
    return {k: np.asarray(inputs[k]) for k in ("x",) + NAMES}


def chain(args):
    inp, b, eps = args
    from dynamic_factor_models_amd import bayes
    r = inp["Lam"].shape[1]
    pr = bayes.default_prior_ar(r)
    cur = dict(Lam=inp["Lam"] * (1 + eps), sig2=inp["sig2"] * (1 + eps), rho=inp["rho"] + eps, Avar=inp["Avar"] + eps,
               Q=inp["Q"] * (1 + eps), mu0=inp["mu0"], P0=inp["P0"])
    common, pers, margin = [], [], np.inf
    for j in range(BURN + KEPT):
        o = gae.sweep(inp["x"], *[cur[k] for k in NAMES], pr, SEED, j, b)
        margin = min(margin, o["margin_rho"], o["margin_gamma"])
        assert (o["att_rho"] < gae.RHO_CAP).all() and (o["att_R"] < 32).all(), "a cap: the device call would fail"
        cur.update(Lam=o["Lam"], sig2=o["sig2"], rho=o["rho"], Avar=o["A"], Q=o["Q"])
        if j >= BURN:
            common.append(o["f"] @ o["Lam"].T)
            pers.append(o["rho"].sum(1))
    return np.mean(common, axis=0), np.mean(pers, axis=0), margin


def figures(inp, eps, pool):
    res = list(pool.map(chain, [(inp, b, eps) for b in range(CHAINS)]))
    common = np.mean([c for c, _, _ in res], axis=0)
    pers = np.mean([p for _, p, _ in res], axis=0)
    return float(np.abs(common).max()), float(pers.mean()), min(m for _, _, m in res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs")
    ap.add_argument("--dump")
    a = ap.parse_args()
    inp = dict(np.load(a.inputs)) if a.inputs else start_from_the_device()
    if a.dump:
        np.savez(a.dump, **inp)
        print("wrote", a.dump)
        return
    with cf.ProcessPoolExecutor(max_workers=CHAINS) as pool:
        c0, p0, m0 = figures(inp, 0.0, pool)
        c1, p1, m1 = figures(inp, 1e-9, pool)
    print(f"max |common_mean - mean| = {c0:.10f}   mean persistence_mean = {p0:.10f}")
    print(f"start moved by 1e-9:       {c1:.10f}                           {p1:.10f}")
    print(f"drift: {abs(c1 - c0):.3e} and {abs(p1 - p0):.3e}; smallest accept margin {min(m0, m1):.3e}")


if __name__ == "__main__":
    main()
