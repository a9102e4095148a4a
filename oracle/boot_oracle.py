"""CPU fp64 oracle of the wild-bootstrap impulse-response draws (BASELINE config 5).

TEST INFRASTRUCTURE ONLY: nothing under dynamic_factor_models_amd/ may import it.

The reference has no bootstrap ("parity unpinned" for the draw loop); what it does have -- and what every
draw re-runs -- is pinned: `estimate_var!` + `fill_matrices!` (dfm_functions.ipynb:444-492) and
`impulse_response` (:793-816), restated in oracle/als_oracle.py and pinned by the notebook's Table 5.  The
draw itself is the textbook recursive-design wild bootstrap (Goncalves & Kilian 2004):
    e*_t = s_t e_t,  s_t = +-1;  y*_t = c + sum_l A_l y*_{t-l} + e*_t,  y*_t = y_t for t < p.
"""
from __future__ import annotations

import numpy as np

from . import als_oracle as ao
from . import synth_oracle as so


def sign_block(seed: int, period, draw) -> np.ndarray:
    """Philox::block(seed, period, draw) of dfm_philox.h as boot.hip calls it: the Philox4x32-10 block keyed by the
    64-bit `seed` with the 128-bit counter (period lo, period hi, draw lo, draw hi).  `period` and `draw` are uint64
    arrays of one shape; returns [..., 4] uint32."""
    t, d = np.broadcast_arrays(np.asarray(period, dtype=np.uint64), np.asarray(draw, dtype=np.uint64))
    ctr = np.stack([(t & so.MASK).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32),
                    (d & so.MASK).astype(np.uint32), (d >> np.uint64(32)).astype(np.uint32)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return so.philox4x32_10(ctr, key)


def rademacher_signs(seed: int, first_draw: int, B: int, T: int) -> np.ndarray:
    """The device-drawn signs of boot.hip's draw loop, [B, T] of +-1.0: sign (d, t) is +1 if word 0 of
    sign_block(seed, t, first_draw + d) is odd, else -1.  Periods t < p are listed too; the kernel never draws them."""
    d = np.array([(first_draw + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)], dtype=np.uint64)
    w0 = sign_block(seed, np.arange(T, dtype=np.uint64)[None, :], d[:, None])[..., 0]
    return np.where((w0 & np.uint32(1)) != 0, 1.0, -1.0)


def var_bootstrap_irf(y, p, H, signs):
    """y [T, ns] (no NaN); signs [B, T] of +-1.  Returns (irf [B, ns, H, ns], beta [B, 1 + ns p, ns],
    point estimate dict from als_oracle.estimate_var)."""
    y = np.asarray(y, float)
    T, ns = y.shape
    v = ao.estimate_var(y, p, 1, T)
    beta = v["betahat"]
    e = np.zeros((T, ns))
    e[p:] = v["resid"][p:]
    B = signs.shape[0]
    irf = np.empty((B, ns, H, ns))
    betas = np.empty((B,) + beta.shape)
    for d in range(B):
        ys = y.copy()
        for t in range(p, T):
            x = np.concatenate([[1.0]] + [ys[t - 1 - l] for l in range(p)])
            ys[t] = x @ beta + signs[d, t] * e[t]
        vd = ao.estimate_var(ys, p, 1, T)
        betas[d] = vd["betahat"]
        irf[d] = ao.impulse_response(vd["M"], vd["Q"], vd["G"], range(ns), H)
    return irf, betas, v
