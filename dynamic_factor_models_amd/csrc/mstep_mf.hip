// mstep_mf.hip -- the series block of the EM iteration for the MIXED-FREQUENCY DFM (include/dfm_hip.h: dfm_em_mf_batch;
// tests/mf_expect.py em_step_mf, step 3):
//
//     x_it = lam_i' g_it + e_it,   g_it = sum_{l<L} w_il f_{t-l},   e_it ~ N(0, R_i)
//
// with KNOWN weights w_i (a monthly series (1, 0, ..), a quarterly flow (1, 2, 3, 2, 1) / 3, ..) on the companion state
// z_t = (f_t, .., f_{t-m+1}), m = max(p, L) (capi.hip: mf_run).  Over the observed periods of series i:
//     G_i = sum_t E[g_it g_it'],   b_i = sum_t x_it E[g_it],   lam_i = G_i^-1 b_i,
//     R_i = (sum_t x_it^2 - 2 lam_i' b_i + lam_i' G_i lam_i) / n_i.
// The weight vectors of a panel come in few distinct classes c (mf_run finds them on the host), so the aggregation over lags is
// done ONCE per replicate, period and class, not per series:
//   mf_table_kernel    V[b][t][c] = [vech(E g g') (packed lower), zeros to 16 NTG | E g (r columns), zeros to 16]  from the smoothed
//                      z_t and its packed covariance -- r(r+1)/2 + r columns whatever L is (the AR-style moment form would carry
//                      vech of an r L x r L block: 210 columns at r = 4, L = 5);
//   mf_moments_kernel  per replicate and 16 series of ONE class (mf_run deals the series into class-pure tiles by index, the panel
//                      and the outputs stay in the caller's order): G_i, b_i as products on v_mfma_f64_16x16x4, A operand = the
//                      observation mask (G tiles) or the masked panel column (b tile), B operand = the class's table rows;
//                      sum x^2 and n_i beside them on the vector pipe;
//   mf_solve_kernel    a thread per series: the r x r Cholesky solve and R_i, with the n_i < r + 1 rule.
// mf_loadings_kernel expands the loadings for the E-step: LamK[i] = [w_i0 lam_i, .., w_i,L-1 lam_i, 0..].
#include "dfm_kernels.h"
#include "dfm_mfgeom.h"

namespace dfm {

namespace {


constexpr int kMfU = 4;                                        // matrix steps (of 4 periods) loaded together, one group ahead

}  // namespace

__global__ void mf_loadings_kernel(int B, int N, int r, int L, int Rk, const double* __restrict__ Lam, const double* __restrict__ W,
                                   double* __restrict__ LamK) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (size_t)B * N * Rk) return;
    const int c = tid % Rk;
    const size_t bn = tid / Rk;
    const int i = (int)(bn % N);
    const int l = c / r, cc = c % r;
    LamK[tid] = l < L ? W[(size_t)i * L + l] * Lam[bn * r + cc] : 0.0;
}

// thread = (replicate, period, column of the class row); every class from one read of the state's moments
__global__ __launch_bounds__(256) void mf_table_kernel(MfMstepArgs a, double* __restrict__ V) {
    const int b = blockIdx.y;
    if (a.active && a.active[b] == 0) return;
    const int VW = a.VW, r = a.r, L = a.L, Rk = a.Rk, C = a.C;
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= a.T * VW) return;
    const int t = e / VW, col = e - t * VW;
    const int np = mf_vech_cols(r), ng16 = mf_mean_col0(VW);
    const size_t npk = (size_t)Rk * (Rk + 1) / 2;
    const double* __restrict__ zt = a.zsm + ((size_t)b * a.T + t) * Rk;
    const double* __restrict__ Pt = a.Psm + ((size_t)b * a.T + t) * npk;
    auto pk = [](int u, int v) { return u >= v ? u * (u + 1) / 2 + v : v * (v + 1) / 2 + u; };   // packed lower, symmetric
    double acc[kMfMaxClasses];
#pragma unroll
    for (int c = 0; c < kMfMaxClasses; ++c) acc[c] = 0.0;
    if (col < np) {
        int cc = 0;
        while ((cc + 1) * (cc + 2) / 2 <= col) ++cc;
        const int dd = col - cc * (cc + 1) / 2;
        for (int l = 0; l < L; ++l)
            for (int l2 = 0; l2 < L; ++l2) {
                const int u = l * r + cc, v = l2 * r + dd;
                const double m = fma(zt[u], zt[v], Pt[pk(u, v)]);
#pragma unroll
                for (int c = 0; c < kMfMaxClasses; ++c)
                    if (c < C) acc[c] = fma(a.Wc[c * L + l] * a.Wc[c * L + l2], m, acc[c]);
            }
    } else if (col >= ng16 && col < ng16 + r) {
        const int cc = col - ng16;
        for (int l = 0; l < L; ++l) {
            const double m = zt[l * r + cc];
#pragma unroll
            for (int c = 0; c < kMfMaxClasses; ++c)
                if (c < C) acc[c] = fma(a.Wc[c * L + l], m, acc[c]);
        }
    }
    double* __restrict__ Vr = V + (((size_t)b * a.T + t) * C) * VW + col;
#pragma unroll
    for (int c = 0; c < kMfMaxClasses; ++c)
        if (c < C) Vr[(size_t)c * VW] = acc[c];
}

// TT = VW / 16 tiles of a class row: NTG = TT - 1 of vech(E g g') against the mask, the last (E g) against the masked panel.
// One wave per 16 series of one class, four waves (tiles) per workgroup; no LDS: a step's A operand is 4 panel rows x 16 series.
// OUT[b][i][VW] and SM[b][2][N] in the caller's series order.
template <int TT>
__global__ __launch_bounds__(256) void mf_moments_kernel(MfMstepArgs a, const double* __restrict__ V, double* __restrict__ OUT,
                                                         double* __restrict__ SM) {
    const int b = blockIdx.y;
    if (a.active && a.active[b] == 0) return;
    const int tile = (int)blockIdx.x * kMfWaves + ((int)threadIdx.x >> 6);
    if (tile >= a.ntiles) return;
    const int lane = (int)threadIdx.x & 63, k4 = lane >> 4, c16 = lane & 15;
    const int T = a.T, N = a.N, VW = 16 * TT;
    const int cls = a.tile_class[tile];
    const int idx = a.tile_series[tile * 16 + c16];            // the series of this lane's A-operand row; -1: padding of the tile
    const int xcol = idx < 0 ? 0 : idx;
    const double* __restrict__ xb = a.panel + (size_t)b * T * N + xcol;
    const size_t vstride = (size_t)a.C * VW;
    const double* __restrict__ Vb = V + ((size_t)b * T * a.C + cls) * VW + c16;
    v4d acc[TT];
#pragma unroll
    for (int x = 0; x < TT; ++x) acc[x] = v4d{0.0, 0.0, 0.0, 0.0};
    double nn = 0.0, sxx = 0.0;
    double xq[kMfU], bq[kMfU][TT];
    auto load = [&](int g) {
#pragma unroll
        for (int u = 0; u < kMfU; ++u) {
            int t = 16 * g + 4 * u + k4;
            t = t < T ? t : T - 1;                             // (past the end: a clamped row, masked out below)
            xq[u] = xb[(size_t)t * N];
#pragma unroll
            for (int x = 0; x < TT; ++x) bq[u][x] = Vb[(size_t)t * vstride + 16 * x];
        }
    };
    const int ng = mf_groups(T);
    load(0);
    for (int g = 0; g < ng; ++g) {
        double xv[kMfU], bv[kMfU][TT];
#pragma unroll
        for (int u = 0; u < kMfU; ++u) {
            xv[u] = xq[u];
#pragma unroll
            for (int x = 0; x < TT; ++x) bv[u][x] = bq[u][x];
        }
        if (g + 1 < ng) load(g + 1);
#pragma unroll
        for (int u = 0; u < kMfU; ++u) {
            const bool ok = (16 * g + 4 * u + k4 < T) && idx >= 0 && (xv[u] == xv[u]);
            const double am = ok ? 1.0 : 0.0, xm = ok ? xv[u] : 0.0;
#pragma unroll
            for (int x = 0; x < TT; ++x)
                acc[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(x + 1 < TT ? am : xm, bv[u][x], acc[x], 0, 0, 0);
            nn += am;
            sxx = fma(xm, xm, sxx);
        }
    }
    // 16x16x4 D[(lane / 16) + 4 v][lane % 16]: series k4 + 4 v of the tile, column c16 of table tile x
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int i = a.tile_series[tile * 16 + k4 + 4 * v];
        if (i >= 0) {
#pragma unroll
            for (int x = 0; x < TT; ++x) OUT[((size_t)b * N + i) * VW + 16 * x + c16] = acc[x][v];
        }
    }
    nn += __shfl_xor(nn, 16, 64); nn += __shfl_xor(nn, 32, 64);
    sxx += __shfl_xor(sxx, 16, 64); sxx += __shfl_xor(sxx, 32, 64);
    if (k4 == 0 && idx >= 0) {
        SM[((size_t)b * 2 + 0) * N + idx] = sxx;
        SM[((size_t)b * 2 + 1) * N + idx] = nn;
    }
}

// A thread per series (the aggregation over lags is already in the table: r(r+1)/2 + r + 2 loads per series, no lag pairs to
// deal to more lanes as ar_solve_kernel does).  A series with fewer than r + 1 observed cells, or a G_i that is not positive
// definite, keeps its loadings and variance.
template <int R>
__global__ __launch_bounds__(256) void mf_solve_kernel(MfMstepArgs a, const double* __restrict__ OUT, const double* __restrict__ SM) {
    const int b = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (a.active && a.active[b] == 0) return;
    const int N = a.N, VW = a.VW;
    if (i >= N) return;
    const double* __restrict__ o = OUT + ((size_t)b * N + i) * VW;
    const int n = (int)(SM[((size_t)b * 2 + 1) * N + i] + 0.5);
    if (n < R + 1) return;
    const double sxx = SM[((size_t)b * 2 + 0) * N + i];
    double G[R][R], Lc[R][R], bv[R], y[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        bv[c] = o[mf_mean_col(VW, c)];
#pragma unroll
        for (int d = 0; d <= c; ++d) { G[c][d] = o[mf_vech_col(c, d)]; G[d][c] = G[c][d]; }
    }
    bool pd = true;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        double d = G[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= Lc[j][k] * Lc[j][k];
        pd = pd && (d > 0.0);
        d = sqrt(d > 0.0 ? d : 1.0);
        Lc[j][j] = d;
#pragma unroll
        for (int q = j + 1; q < R; ++q) {
            double s = G[q][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= Lc[q][k] * Lc[j][k];
            Lc[q][j] = s / d;
        }
    }
    if (!pd) return;
#pragma unroll
    for (int c = 0; c < R; ++c) {
        double s = bv[c];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= Lc[c][k] * y[k];
        y[c] = s / Lc[c][c];
    }
#pragma unroll
    for (int c = R - 1; c >= 0; --c) {
        double s = y[c];
#pragma unroll
        for (int k = c + 1; k < R; ++k) s -= Lc[k][c] * y[k];
        y[c] = s / Lc[c][c];
    }
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
    for (int c = 0; c < R; ++c) a.Lam[((size_t)b * N + i) * R + c] = y[c];
    a.R[(size_t)b * N + i] = (sxx - 2.0 * lb + lGl) / (double)n;
}

bool mstep_mf_supported(int r, int L) { return r >= 1 && r <= 8 && L >= 1 && L <= kMfMaxLags; }
int mstep_mf_row_width(int r) { return mf_row_width(r); }
// V [B][T][C][VW] | OUT [B][N][VW] | SM [B][2][N]
size_t mstep_mf_workspace(int B, int T, int N, int r, int C) {
    const size_t VW = (size_t)mstep_mf_row_width(r);
    return ((size_t)B * T * C * VW + (size_t)B * N * VW + (size_t)B * 2 * N) * sizeof(double);
}

hipError_t launch_mf_loadings(int B, int N, int r, int L, int Rk, const double* Lam, const double* W, double* LamK, hipStream_t s) {
    note_kernel("mf_loadings_kernel");
    hipLaunchKernelGGL(mf_loadings_kernel, dim3((unsigned)mf_loadings_blocks(B, N, Rk)), dim3(kMfBlock), 0, s, B, N, r, L, Rk, Lam, W, LamK);
    return hipGetLastError();
}

hipError_t launch_mf_table(const MfMstepArgs& a, double* ws, hipStream_t s) {
    note_kernel("mf_table_kernel");
    if (!ws || a.VW != mstep_mf_row_width(a.r) || a.C < 1 || a.C > kMfMaxClasses || a.r * a.L > a.Rk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mf_table_kernel, dim3(mf_table_blocks(a.T, a.VW), a.B), dim3(kMfBlock), 0, s, a, ws);
    return hipGetLastError();
}

hipError_t launch_mf_moments(const MfMstepArgs& a, double* ws, hipStream_t s) {
    note_kernel("mf_moments_kernel");
    if (!ws || a.VW != mstep_mf_row_width(a.r) || a.ntiles < 1) return hipErrorInvalidValue;
    const double* V = ws;
    double* OUT = ws + (size_t)a.B * a.T * a.C * a.VW;
    double* SM = OUT + (size_t)a.B * a.N * a.VW;
    const dim3 grid(mf_moment_blocks(a.ntiles), a.B), block(kMfBlock);
    switch (mf_row_tiles(a.VW)) {
        case 2: hipLaunchKernelGGL(mf_moments_kernel<2>, grid, block, 0, s, a, V, OUT, SM); break;
        case 3: hipLaunchKernelGGL(mf_moments_kernel<3>, grid, block, 0, s, a, V, OUT, SM); break;
        case 4: hipLaunchKernelGGL(mf_moments_kernel<4>, grid, block, 0, s, a, V, OUT, SM); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int R>
static hipError_t launch_mf_solve_r(const MfMstepArgs& a, const double* OUT, const double* SM, hipStream_t s) {
    hipLaunchKernelGGL(mf_solve_kernel<R>, dim3(mf_solve_blocks(a.N), a.B), dim3(kMfBlock), 0, s, a, OUT, SM);
    return hipGetLastError();
}
hipError_t launch_mf_solve(const MfMstepArgs& a, double* ws, hipStream_t s) {
    note_kernel("mf_solve_kernel");
    if (!ws) return hipErrorInvalidValue;
    const double* OUT = ws + (size_t)a.B * a.T * a.C * a.VW;
    const double* SM = OUT + (size_t)a.B * a.N * a.VW;
    switch (a.r) {
        case 1: return launch_mf_solve_r<1>(a, OUT, SM, s);
        case 2: return launch_mf_solve_r<2>(a, OUT, SM, s);
        case 3: return launch_mf_solve_r<3>(a, OUT, SM, s);
        case 4: return launch_mf_solve_r<4>(a, OUT, SM, s);
        case 5: return launch_mf_solve_r<5>(a, OUT, SM, s);
        case 6: return launch_mf_solve_r<6>(a, OUT, SM, s);
        case 7: return launch_mf_solve_r<7>(a, OUT, SM, s);
        case 8: return launch_mf_solve_r<8>(a, OUT, SM, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dfm
