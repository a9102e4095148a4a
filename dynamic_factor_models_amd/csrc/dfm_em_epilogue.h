// dfm_em_epilogue.h -- what every EM route does once a replicate's log-likelihood and sufficient statistics are known: the ONE text
// of the stop rule and of the transition M-step (Shumway-Stoffer 1982; oracle/kalman_oracle.py em() / em_step).
//
//   stop rule   record ll_k; a replicate that was active stops WITHOUT applying this M-step when k >= 1, tol > 0 and the relative
//               improvement over ll_{k-1} is below tol.  em_decide only reads, em_record does the three writes (one thread); the
//               barrier that keeps the writer behind every reader stays with the caller, in the kernel's own kind.
//   M-step      A = S10 S00^-1,  Q = sym(S11 - A S10') / T,  mu0 = f_0|T,  P0 = sym(P_0|T),  S11^-1 for the loadings step, with the
//               companion constraints and the narrow S11 layout of MstepCons (element per thread, Grid<R>), or row per lane.
//               recursion_kernel, recursion_wave_kernel and recursion_pair_kernel keep the M-step written out (wave: the bookkeeping
//               too, around em_improved): inlined from here their register allocation came out worse than before.
//
// How a kernel forms S11 / S10 / S00 is its own business.  em_improved is plain C++ so that the host can check it against the oracle's
// expression (tests/test_em_stop_rule_cpu.py through tests/host/em_stop_host.cpp).  Reference counterpart: none (the reference has no EM).
#pragma once

#if defined(__HIPCC__)
#include "dfm_grid.h"
#define DFM_EM_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define DFM_EM_HD inline
#endif

namespace dfm {

// false = stop.  Written as the negation of "<" so that a NaN on either side keeps iterating.
DFM_EM_HD bool em_improved(double ll, double llp, double tol) { return !((ll - llp) / (0.5 * (fabs(ll) + fabs(llp))) < tol); }

#if defined(__HIPCC__)

struct EmDecision {
    int was, go;      // (0 | 1) was still iterating; applies this M-step and goes on.  (ints: with bools recursion_kernel<16, false>
                      // spills two more SGPRs -- hipcc of ROCm 7.2.0, clang 22)
};
// Args: RecursionArgs | EmUpdArgs (active / iters / ll_path / k / max_iter / tol); a.active != nullptr is the caller's test
template <class Args>
__device__ __forceinline__ EmDecision em_decide(const Args& a, int b, double ll) {
    const bool was = a.k == 0 ? true : (a.active[b] != 0);
    bool go = was;
    if (was && a.k >= 1 && a.tol > 0.0) go = em_improved(ll, a.ll_path[(size_t)b * a.max_iter + a.k - 1], a.tol);
    return {was ? 1 : 0, go ? 1 : 0};
}
template <class Args>
__device__ __forceinline__ void em_record(const Args& a, int b, double ll, EmDecision d) {
    if (d.was) { a.ll_path[(size_t)b * a.max_iter + a.k] = ll; a.iters[b] = a.k + 1; }
    a.active[b] = d.go ? 1 : 0;
}

// The constraints of the models whose state is wider than their factors, as RecursionArgs carries them: kdim / ka / kb (companion
// state: only [A_1 .. A_p] and the innovation covariance of f_t are free) and rl / Rc (the loadings step sees the first rl components
// only: S11 / S11^-1 go out as [S11[:rl,:rl] 0; 0 T I] in its [Rc][Rc] layout).  All zero: a plain factor model; the grid form has
// an overload without the argument that compiles the branches out (a literal {} did not fold in time for em_update_grid_kernel<32>'s
// register allocation: 98 VGPRs for 64, hipcc of ROCm 7.2.0, clang 22).
struct MstepCons {
    int kdim, ka, kb, rl, Rc;
};

// Element per thread: thread G.l = R G.i + G.j holds element (i, j) of every matrix; L0, L1: LDS tiles of R x kTileStride<R>.
// Out: RecursionArgs | EmUpdArgs (A_out / Q_out / P0_out / mu0_out / S11 / S11inv).  The full-width S11 is the caller's to write.
template <int R, bool CONS, class Out>
__device__ __forceinline__ void transition_mstep_grid_impl(Grid<R>& G, double* L0, double* L1, const Out& out, int b, int T, double S11,
                                                           double S10, double S00, double Ps, double f0_row, bool em_apply, MstepCons cons) {
    constexpr int TS = kTileStride<R>;
    const int i = G.i, j = G.j;
    const size_t o = (size_t)b * R * R + G.l;
    const bool narrow = CONS && cons.rl > 0;
    const int rl = narrow ? cons.rl : R, Rc = cons.Rc > 0 ? cons.Rc : R;
    const bool inL = i < rl && j < rl, inC = i < Rc && j < Rc;
    double inv = S00;
    if (CONS && cons.kdim > 0 && cons.ka > 0) {   // VAR(p) inside a wider state: A = S10[:, :ka] S00[:ka, :ka]^-1, zero beyond
        if (i >= cons.ka || j >= cons.ka) inv = (i == j) ? 1.0 : 0.0;
        if (j >= cons.ka) S10 = 0.0;
    }
    (void)G.sweep_inverse(inv);
    G.sync();
    L0[TS * i + j] = S10;
    L1[TS * i + j] = inv;                                        // symmetric: rows = columns
    G.sync();
    const double An = dot_rows<R>(L0, L1, i, j);
    G.sync();
    L1[TS * i + j] = An;
    G.sync();
    double Qn = (S11 - dot_rows<R>(L1, L0, i, j)) / (double)T;   // (A S10')_ij = row i of A . row j of S10
    Qn = 0.5 * (Qn + G.transposed(Qn));
    double Aout = An;
    if (CONS && cons.kdim > 0) {
        const int rb = cons.kb > 0 ? cons.kb : rl;               // block size of the companion state
        if (i >= rb && i < cons.kdim) Aout = (j == i - rb) ? 1.0 : 0.0;
        if ((i >= rb && i < cons.kdim) || (j >= rb && j < cons.kdim)) Qn = 0.0;
    }
    const double P0n = 0.5 * (Ps + G.transposed(Ps));
    double inv2 = S11;
    if (narrow) {
        if (!inL) inv2 = (i == j) ? (double)T : 0.0;
        if (inC) out.S11[(size_t)b * Rc * Rc + i * Rc + j] = inv2;
    }
    (void)G.sweep_inverse(inv2);
    if (narrow) { if (inC) out.S11inv[(size_t)b * Rc * Rc + i * Rc + j] = inv2; }
    else out.S11inv[o] = inv2;
    if (em_apply) {
        out.A_out[o] = Aout;
        out.Q_out[o] = Qn;
        out.P0_out[o] = P0n;
        if (j == 0) out.mu0_out[(size_t)b * R + i] = f0_row;
    }
}
template <int R, class Out>
__device__ __forceinline__ void transition_mstep_grid(Grid<R>& G, double* L0, double* L1, const Out& out, int b, int T, double S11,
                                                      double S10, double S00, double Ps, double f0_row, bool em_apply) {
    transition_mstep_grid_impl<R, false>(G, L0, L1, out, b, T, S11, S10, S00, Ps, f0_row, em_apply, MstepCons{0, 0, 0, 0, 0});
}
template <int R, class Out>
__device__ __forceinline__ void transition_mstep_grid(Grid<R>& G, double* L0, double* L1, const Out& out, int b, int T, double S11,
                                                      double S10, double S00, double Ps, double f0_row, bool em_apply, MstepCons cons) {
    transition_mstep_grid_impl<R, true>(G, L0, L1, out, b, T, S11, S10, S00, Ps, f0_row, em_apply, cons);
}

// Row per lane, plain factor model: lane i of a group of R lanes holds ROW i of every matrix; X: the group's R x R LDS exchange slot.
// WAVE: the group lives in one wave that need not wait for the rest of its workgroup (group_sync, dfm_smallmat.h).  live: this group
// writes.  (recursion_kernel, the one row-per-lane kernel with constraints, keeps its own text: see recursion.hip.)
template <int R, bool WAVE, class Out>
__device__ __forceinline__ void transition_mstep_rows(double* X, int i, const Out& out, int b, int T, bool live, const double (&S11)[R],
                                                      const double (&S10)[R], const double (&S00)[R], const double (&Ps)[R], double f0_i,
                                                      bool em_apply) {
    const size_t o = (size_t)b * R * R + (size_t)i * R;
    double inv[R], An[R], tmp[R], Qn[R], P0n[R];
#pragma unroll
    for (int j = 0; j < R; ++j) inv[j] = S00[j];
    (void)gj_inverse<R, WAVE>(inv, X, i);
    group_sync<WAVE>();
    store_row<R>(X, i, inv);
    group_sync<WAVE>();
    mm_rows<R>(An, S10, X);                                // A row i
    group_sync<WAVE>();
    store_row<R>(X, i, S10);
    group_sync<WAVE>();
    mm_rowsT<R>(tmp, An, X);                               // (A S10')[i][:]
#pragma unroll
    for (int j = 0; j < R; ++j) Qn[j] = (S11[j] - tmp[j]) / (double)T;
    group_sync<WAVE>();
    store_row<R>(X, i, Qn);
    group_sync<WAVE>();
#pragma unroll
    for (int j = 0; j < R; ++j) Qn[j] = 0.5 * (Qn[j] + X[j * R + i]);
    group_sync<WAVE>();
    store_row<R>(X, i, Ps);
    group_sync<WAVE>();
#pragma unroll
    for (int j = 0; j < R; ++j) P0n[j] = 0.5 * (Ps[j] + X[j * R + i]);
#pragma unroll
    for (int j = 0; j < R; ++j) inv[j] = S11[j];
    (void)gj_inverse<R, WAVE>(inv, X, i);
    if (live) {
#pragma unroll
        for (int j = 0; j < R; ++j) out.S11inv[o + j] = inv[j];
        if (em_apply) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                out.A_out[o + j] = An[j];
                out.Q_out[o + j] = Qn[j];
                out.P0_out[o + j] = P0n[j];
            }
            out.mu0_out[(size_t)b * R + i] = f0_i;
        }
    }
}

#endif  // __HIPCC__

}  // namespace dfm
