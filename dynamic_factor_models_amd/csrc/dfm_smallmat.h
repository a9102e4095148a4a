// dfm_smallmat.h -- r x r dense helpers for the "lane i owns row i" layout of the recursion kernels:
// a group of R lanes holds one matrix, rows other lanes need are exchanged through a per-group LDS
// slot (one wave per workgroup, so __syncthreads() is a wave-level fence); and psd_root, the workgroup-wide
// Cholesky root in LDS of the prep kernels (simsmooth.hip, structural.hip).
#pragma once
#include "dfm_device.h"

namespace dfm {

constexpr double kSteadyTol = 4.5e-16;  // ~2 ulp: successive Om_f / P_s this close are "equal"
constexpr double kPsdTol = 1e-12;       // psd_root: a pivot <= this x trace zeroes its column

template <int R>
__device__ __forceinline__ void store_row(double* M, int i, const double (&row)[R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) M[i * R + j] = row[j];
}
// out[j] = sum_k own[k] * M[k][j]
template <int R>
__device__ __forceinline__ void mm_rows(double (&out)[R], const double (&own)[R], const double* M) {
#pragma unroll
    for (int j = 0; j < R; ++j) out[j] = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const double a = own[k];
#pragma unroll
        for (int j = 0; j < R; ++j) out[j] = fma(a, M[k * R + j], out[j]);
    }
}
// out[j] = sum_k own[k] * M[j][k]
template <int R>
__device__ __forceinline__ void mm_rowsT(double (&out)[R], const double (&own)[R], const double* M) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(own[k], M[j * R + k], s);
        out[j] = s;
    }
}
template <int R>
__device__ __forceinline__ double dot_vec(const double (&own)[R], const double* v) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < R; k += 2) {
        s0 = fma(own[k], v[k], s0);
        s1 = fma(own[k + 1], v[k + 1], s1);
    }
    return s0 + s1;
}

// In-place Gauss-Jordan inverse (no pivoting; SPD input).  Lane i holds row i in m; sweep k broadcasts
// row k through the two R-double LDS rows at X (double-buffered: one barrier per sweep).
// Returns det(input) = product of pivots.  Every lane of the group gets the same value.
// Exchange fence for LDS traffic between the lanes of ONE wave (no s_barrier): a wave's DS operations are
// processed in issue order, so only the compiler has to be kept from moving loads above stores.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool WAVE>
__device__ __forceinline__ void group_sync() {
    if constexpr (WAVE) wave_lds_sync(); else __syncthreads();
}

// WAVE = true: the lane groups exchanging through X all live in one wave of a multi-wave workgroup
template <int R, bool WAVE = false>
__device__ __forceinline__ double gj_inverse(double (&m)[R], double* X, int i) {
    double det = 1.0;
    group_sync<WAVE>();
#pragma unroll
    for (int k = 0; k < R; ++k) {
        double* buf = X + (k & 1) * R;
        if (i == k) {
#pragma unroll
            for (int j = 0; j < R; ++j) buf[j] = m[j];
        }
        group_sync<WAVE>();
        double q[R];
#pragma unroll
        for (int j = 0; j < R; ++j) q[j] = buf[j];
        const double piv = q[k];
        const double d = 1.0 / piv;
        det *= piv;
        const double c = m[k];
        const bool me = (i == k);
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (j == k) {
                m[j] = me ? d : -c * d;
            } else {
                const double qj = q[j] * d;
                m[j] = me ? qj : fma(-c, qj, m[j]);
            }
        }
    }
    return det;
}

// Symmetric diagonal scaling of a normal matrix held one row per lane: row <- d_k row d, d_k = G_kk^-1/2
// (G_kk > 0), exchanged through the group's R-double LDS row `dx`.  Returns d_k; the caller scales its
// right-hand side entry by d_k before, and its solution entry by d_k after, the solve.  Regressors on very
// different scales (a constant next to levels) otherwise cost the unpivoted elimination its accuracy.
template <int R, bool WAVE = false>
__device__ __forceinline__ double equilibrate_rows(double (&m)[R], double* dx, int i) {
    double dk = 1.0;
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (j == i) dk = m[j] > 0.0 ? 1.0 / sqrt(m[j]) : 1.0;
    group_sync<WAVE>();
    dx[i] = dk;
    group_sync<WAVE>();
#pragma unroll
    for (int j = 0; j < R; ++j) m[j] *= dk * dx[j];
    return dk;
}

__device__ __forceinline__ bool close_enough(double a, double b) {
    return fabs(a - b) <= kSteadyTol * fabs(b);
}

// Lower root L L' = M (n <= 32, lower triangle of M read) by Cholesky; a column whose pivot is <= tol_rel trace(M) is zero, so a
// positive semi-definite M has a root too.  Returns the number of zero columns.  L: LDS [n][n]; every thread of the workgroup
// takes part.
__device__ inline int psd_root(const double* M, int n, double* L, double tol_rel) {
    const int tid = threadIdx.x;
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += M[i * n + i];
    const double tol = tol_rel * tr;
    for (int e = tid; e < n * n; e += blockDim.x) L[e] = 0.0;
    __syncthreads();
    int dropped = 0;
    for (int j = 0; j < n; ++j) {
        double dj = M[j * n + j];
        for (int m = 0; m < j; ++m) dj -= L[j * n + m] * L[j * n + m];
        const bool keep = dj > tol;
        dropped += keep ? 0 : 1;
        const double ljj = keep ? sqrt(dj) : 0.0;
        for (int i = j + tid; i < n; i += blockDim.x) {
            if (i == j) {
                L[j * n + j] = ljj;
            } else {
                double v = M[i * n + j];
                for (int m = 0; m < j; ++m) v -= L[i * n + m] * L[j * n + m];
                L[i * n + j] = keep ? v / ljj : 0.0;
            }
        }
        __syncthreads();
    }
    return dropped;
}

// ---- 16 x 16 matrices on the fp64 matrix pipe (recursion_mbf16.hip, recursion_comp.hip): one v4d per lane in the D layout of
// v_mfma_f64_16x16x4_f64 -- lane l = 16 g + c holds rows 4 g .. 4 g + 3 of column c.
__device__ __forceinline__ v4d mm1(double a, double b, v4d acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ double row_sum16(double v) {          // sum over the 16 lanes of a row group, in every lane of it
    v += xor_lane<1>(v); v += xor_lane<2>(v); v += xor_lane<4>(v); v += xor_lane<8>(v);
    return v;
}
__device__ __forceinline__ double col_sum4(double v) {           // sum over the 4 row groups (lanes c, c + 16, c + 32, c + 48)
    v += xor_lane<16>(v); v += xor_lane<32>(v);
    return v;
}
// sqrt(x) and 1 / sqrt(x) of a positive, normal x: v_rsq_f64 refined by two Newton steps, the root by one correction (a pivot of an
// SPD matrix: no scaling, no fix-up -- the IEEE sqrt + division pair is ~35 instructions on a chain that is nothing but such pivots)
__device__ __forceinline__ void fast_sqrt_rsqrt(double x, double& s, double& r) {
    r = __builtin_amdgcn_rsq(x);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    s = x * r;
    s = fma(0.5 * r, fma(-s, s, x), s);
}
// x[q], q run-time: selects, no indexing.  The operands are PRVALUES -- unary plus: `q == 0 ? x[0] : x[1]` on lvalues is an lvalue, clang
// emits a select of ADDRESSES and one load, the array then stays in scratch memory behind a dynamic offset, and every pick is a scratch
// round trip behind an s_waitcnt vmcnt(0).
__device__ __forceinline__ double pick4(const double (&x)[4], int q) {
    const double a0 = +x[0], a1 = +x[1], a2 = +x[2], a3 = +x[3];
    return q == 0 ? +a0 : q == 1 ? +a1 : q == 2 ? +a2 : +a3;
}

}  // namespace dfm
