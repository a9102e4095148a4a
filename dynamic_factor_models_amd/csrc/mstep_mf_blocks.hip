// mstep_mf_blocks.hip -- the series solve of the mixed-frequency EM with FIXED loadings (include/dfm_hip.h: dfm_em_mf_blocks_batch;
// tests/mf_blocks_expect.py em_step_mf_blocks).  free [N][r] (bytes, one matrix for the batch) says which loadings are
// estimated; the others keep the value they have in Lam: a zero for a block structure, a 1 for a normalisation.  With F the free
// and X the fixed coordinates of series i, k_i = |F|, and G_i, b_i, sum x^2, n_i as mf_table_kernel / mf_moments_kernel leave them:
//     lam_F = G_FF^-1 (b_F - G_FX lam_X),      R_i = (sum x^2 - 2 lam' b + lam' G lam) / n_i   (the whole lam).
// The free coordinates are NOT compacted into a k x k system: which coordinates are free differs from lane to lane, and an index
// that depends on the lane sends the register arrays to scratch.  The loops stay unrolled at R over a system of the SAME size in
// which every fixed coordinate is substituted out -- its row and column of G zero, its diagonal 1, its right-hand side 0 -- so that
// the factor of G_FF sits in the free rows and columns, the substituted pivots are exactly 1 and the solution's fixed entries
// exactly 0; lam_X is put back before the sums of R_i.  Only free entries of Lam are stored.
#include "dfm_kernels.h"
#include "dfm_mfgeom.h"

namespace dfm {

// Geometry and `active` skip of mf_solve_kernel (mstep_mf.hip): a thread per series, blockIdx.y = replicate.  A series with
// n_i < k_i + 1, or whose G_FF is not positive definite, keeps lam_i and R_i; k_i = 0 and n_i >= 1 updates R_i only.
template <int R>
__global__ __launch_bounds__(256) void mf_solve_blocks_kernel(MfMstepArgs a, const unsigned char* __restrict__ free_mask,
                                                              const double* __restrict__ OUT, const double* __restrict__ SM) {
    const int b = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (a.active && a.active[b] == 0) return;
    const int N = a.N, VW = a.VW;
    if (i >= N) return;
    unsigned fr = 0u;                                          // bit c: loading c of this series is estimated
#pragma unroll
    for (int c = 0; c < R; ++c) fr |= (free_mask[(size_t)i * R + c] != 0 ? 1u : 0u) << c;
    const int k = __popc(fr);
    const double* __restrict__ o = OUT + ((size_t)b * N + i) * VW;
    const int n = (int)(SM[((size_t)b * 2 + 1) * N + i] + 0.5);
    if (n < k + 1) return;
    const double sxx = SM[((size_t)b * 2 + 0) * N + i];
    double* __restrict__ lam = a.Lam + ((size_t)b * N + i) * R;
    double G[R][R], Lc[R][R], bv[R], y[R], lx[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        bv[c] = o[mf_mean_col(VW, c)];
        const double l = lam[c];                               // (read whole: a load under the lane's bit would split the row's loads)
        lx[c] = (fr >> c) & 1u ? 0.0 : l;                      // lam_X, zero on the free coordinates
#pragma unroll
        for (int d = 0; d <= c; ++d) { G[c][d] = o[mf_vech_col(c, d)]; G[d][c] = G[c][d]; }
    }
    // the substituted system: entry (q, j) is G[q][j] where both are free, the identity elsewhere
    auto free2 = [&](int q, int j) { return ((fr >> q) & (fr >> j) & 1u) != 0u; };
    bool pd = true;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        double d = free2(j, j) ? G[j][j] : 1.0;
#pragma unroll
        for (int q = 0; q < j; ++q) d -= Lc[j][q] * Lc[j][q];
        pd = pd && (d > 0.0);
        d = sqrt(d > 0.0 ? d : 1.0);
        Lc[j][j] = d;
#pragma unroll
        for (int q = j + 1; q < R; ++q) {
            double s = free2(q, j) ? G[q][j] : 0.0;
#pragma unroll
            for (int m = 0; m < j; ++m) s -= Lc[q][m] * Lc[j][m];
            Lc[q][j] = s / d;
        }
    }
    if (!pd) return;
#pragma unroll
    for (int c = 0; c < R; ++c) {
        double s = bv[c];                                      // b_F - G_FX lam_X (lx is zero where d is free)
#pragma unroll
        for (int d = 0; d < R; ++d) s = fma(-G[c][d], lx[d], s);
        s = (fr >> c) & 1u ? s : 0.0;
#pragma unroll
        for (int m = 0; m < c; ++m) s -= Lc[c][m] * y[m];
        y[c] = s / Lc[c][c];
    }
#pragma unroll
    for (int c = R - 1; c >= 0; --c) {
        double s = y[c];
#pragma unroll
        for (int m = c + 1; m < R; ++m) s -= Lc[m][c] * y[m];
        y[c] = s / Lc[c][c];
    }
#pragma unroll
    for (int c = 0; c < R; ++c) y[c] = (fr >> c) & 1u ? y[c] : lx[c];
    double lb = 0.0, lGl = 0.0;
#pragma unroll
    for (int c = 0; c < R; ++c) {
        lb = fma(y[c], bv[c], lb);
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < R; ++d) s = fma(G[c][d], y[d], s);
        lGl = fma(y[c], s, lGl);
    }
#pragma unroll
    for (int c = 0; c < R; ++c)
        if ((fr >> c) & 1u) lam[c] = y[c];
    a.R[(size_t)b * N + i] = (sxx - 2.0 * lb + lGl) / (double)n;
}

template <int R>
static hipError_t launch_mf_solve_blocks_r(const MfMstepArgs& a, const unsigned char* free_mask, const double* OUT, const double* SM,
                                           hipStream_t s) {
    hipLaunchKernelGGL(mf_solve_blocks_kernel<R>, dim3(mf_solve_blocks(a.N), a.B), dim3(kMfBlock), 0, s, a, free_mask, OUT, SM);
    return hipGetLastError();
}
hipError_t launch_mf_solve_blocks(const MfMstepArgs& a, const unsigned char* free_mask, double* ws, hipStream_t s) {
    note_kernel("mf_solve_blocks_kernel");
    if (!ws || !free_mask) return hipErrorInvalidValue;
    const double* OUT = ws + (size_t)a.B * a.T * a.C * a.VW;
    const double* SM = OUT + (size_t)a.B * a.N * a.VW;
    switch (a.r) {
        case 1: return launch_mf_solve_blocks_r<1>(a, free_mask, OUT, SM, s);
        case 2: return launch_mf_solve_blocks_r<2>(a, free_mask, OUT, SM, s);
        case 3: return launch_mf_solve_blocks_r<3>(a, free_mask, OUT, SM, s);
        case 4: return launch_mf_solve_blocks_r<4>(a, free_mask, OUT, SM, s);
        case 5: return launch_mf_solve_blocks_r<5>(a, free_mask, OUT, SM, s);
        case 6: return launch_mf_solve_blocks_r<6>(a, free_mask, OUT, SM, s);
        case 7: return launch_mf_solve_blocks_r<7>(a, free_mask, OUT, SM, s);
        case 8: return launch_mf_solve_blocks_r<8>(a, free_mask, OUT, SM, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dfm
