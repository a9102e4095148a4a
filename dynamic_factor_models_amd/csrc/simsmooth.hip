// simsmooth.hip -- posterior draws of factor and panel paths (dfm_simsmooth_batch, capi.hip): the simulation smoother of Durbin
// and Koopman (2002).  For pass replicate j = b D + d (replicate b of the call, draw d):
//   1. z+_0 = mu0 + L_P0 n,  f+_t = A_1 f+_{t-1} + .. + A_p f+_{t-p} + L_Q eta_t,  x+_ti = lam_i' f+_t + sqrt(R_i) eps+_ti
//      (simsmooth_path_kernel writes f+ into rows 0..T-1 of f_draw; the cells are never stored)
//   2. D_ti = X_ti - x+_ti on observed cells, NaN elsewhere                              (simsmooth_diff_kernel)
//   3. g = E[f | D] with mu0 = 0: the existing pass on the difference panels                        (capi.hip)
//   4. f_t = f+_t + g_t for t < T, then H steps of the companion recursion with fresh eta          (simsmooth_finish_kernel)
//   5. x_ti = mean_i + sd_i X_ti on observed cells, mean_i + sd_i (lam_i' f_t + sqrt(R_i) eps_ti) elsewhere (simsmooth_fill_kernel)
// Every normal is component c mod 2 of normal2(key, 16 b + s, idx) with key = seed ^ (0x9E3779B97F4A7C15 (first_draw + d + 1)):
//   s = 1 z+_0 (idx c/2), 2 eta of row t (t ceil(r/2) + k/2), 3 eps+ (t ceil(N/2) + i/2), 4 eps (t ceil(N/2) + i/2)
// (include/dfm_hip.h).  An index depends on neither the missing cells nor the launch geometry.
//
// The two cell kernels stream B D (T [+ H]) N cells: one workgroup owns a pass replicate's chunk of rows and a block of column
// pairs, stages the chunk's f rows in LDS, keeps its two rows of loadings in registers, draws one Philox counter per pair of
// cells and moves 16 bytes per lane where N is even.  blockIdx.x is the pass replicate: the D draws of a replicate run next to
// each other, so the panel chunk every one of them reads comes from L2 / the Infinity Cache and HBM sees the writes.
#include "dfm_cell.h"
#include "dfm_kernels.h"
#include "dfm_philox.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr int kSsTC = 32;                     // rows per chunk of the companion recursion (normals and L_Q eta staged in LDS)
constexpr int kSsMaxThreads = 512;            // cell kernels
constexpr size_t kSsLds = 32 * 1024;          // cell kernels: f rows staged per workgroup
enum : uint64_t { kSsZ0 = 1, kSsEta = 2, kSsEpsPlus = 3, kSsEps = 4 };

__device__ __forceinline__ uint64_t ss_key(uint64_t seed, int64_t first_draw, int d) {
    return seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(first_draw + d + 1));
}

// One workgroup per replicate b: the roots of P0 and Q, once for all D draws.
__global__ __launch_bounds__(64) void simsmooth_prep_kernel(SsArgs a) {
    __shared__ double L[32 * 32];
    const size_t b = blockIdx.x;
    const int r = a.r, k = a.r * a.p;
    psd_root(a.P0 + b * k * k, k, L, kPsdTol);
    for (int e = threadIdx.x; e < k * k; e += blockDim.x) a.LP0[b * k * k + e] = L[e];
    __syncthreads();
    psd_root(a.Q + b * r * r, r, L, kPsdTol);
    for (int e = threadIdx.x; e < r * r; e += blockDim.x) a.LQ[b * r * r + e] = L[e];
}

// The slice's pass parameters: replicate b's Lam, R, A, Q, P0 for each of its draws, mu0 = 0.  blockIdx.y = pass replicate.
__global__ __launch_bounds__(256) void simsmooth_expand_kernel(SsArgs a) {
    const int s = blockIdx.y;
    const size_t b = (size_t)((a.j0 + s) / a.D);
    const size_t N = a.N, r = a.r, k = (size_t)a.r * a.p;
    const size_t nL = N * r, nR = N, nA = r * k, nQ = r * r, nm = k, nP = k * k;
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nL) { a.eLam[s * nL + e] = a.Lam[b * nL + e]; return; }
    e -= nL;
    if (e < nR) { a.eR[s * nR + e] = a.R[b * nR + e]; return; }
    e -= nR;
    if (e < nA) { a.eA[s * nA + e] = a.A[b * nA + e]; return; }
    e -= nA;
    if (e < nQ) { a.eQ[s * nQ + e] = a.Q[b * nQ + e]; return; }
    e -= nQ;
    if (e < nm) { a.emu0[s * nm + e] = 0.0; return; }
    e -= nm;
    if (e < nP) a.eP0[s * nP + e] = a.P0[b * nP + e];
}

// The companion recursion f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + L_Q eta_t over output rows t0 .. t1-1 of one pass replicate, one
// wave.  zs[0][0 .. k) holds (row t0-1, .., row t0-p) on entry (zs: two LDS buffers of 32, used in turn: one barrier per row).
// arow: lane c < r holds row c of [A_1 .. A_p].  Rows go to f ([rows][r]), a chunk at a time: they are staged in seta (dead once
// L_Q eta is formed), because the barrier of every row would otherwise wait for that row's global store to complete.
__device__ __forceinline__ void ss_recursion(const SsArgs& a, uint64_t key, uint64_t stream, int t0, int t1, const double* sLQ,
                                             double* seta, double* sw, double (*zs)[32], const double (&arow)[32], double* f) {
    const int r = a.r, k = a.r * a.p, hr = (a.r + 1) / 2, tid = threadIdx.x;
    int cur = 0;
    for (int c0 = t0; c0 < t1; c0 += kSsTC) {
        const int nt = t1 - c0 < kSsTC ? t1 - c0 : kSsTC;
        for (int e = tid; e < nt * hr; e += blockDim.x) {
            const int tt = e / hr, q = e % hr;
            double z0, z1;
            normal2(key, stream, (uint64_t)(c0 + tt) * hr + q, z0, z1);
            seta[tt * 32 + 2 * q] = z0;
            if (2 * q + 1 < r) seta[tt * 32 + 2 * q + 1] = z1;
        }
        __syncthreads();
        for (int e = tid; e < nt * r; e += blockDim.x) {
            const int tt = e / r, c = e % r;
            double v = 0.0;
            for (int m = 0; m <= c; ++m) v = fma(sLQ[c * r + m], seta[tt * 32 + m], v);
            sw[tt * 32 + c] = v;
        }
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
            const double* zin = zs[cur];
            double v = 0.0;
            if (tid < r) {
                v = sw[tt * 32 + tid];
#pragma unroll
                for (int m = 0; m < 32; ++m)
                    if (m < k) v = fma(arow[m], zin[m], v);
                seta[tt * 32 + tid] = v;
            } else if (tid < k) {
                v = zin[tid - r];
            }
            if (tid < k) zs[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        for (int e = tid; e < nt * r; e += blockDim.x) f[(size_t)c0 * r + e] = seta[(e / r) * 32 + e % r];
        __syncthreads();
    }
    // (the caller reads nothing of zs afterwards)
}

__device__ __forceinline__ void ss_load_arow(const SsArgs& a, size_t b, double (&arow)[32]) {
    const int r = a.r, k = a.r * a.p, tid = threadIdx.x;
#pragma unroll
    for (int m = 0; m < 32; ++m) arow[m] = (tid < r && m < k) ? a.A[(b * r + tid) * k + m] : 0.0;
}

// Step 1 for rows 0..T-1: z+_0 from stream 1, then the recursion with eta from stream 2.  One wave per pass replicate of the slice.
__global__ __launch_bounds__(64) void simsmooth_path_kernel(SsArgs a) {
    __shared__ double sLQ[32 * 32], seta[kSsTC * 32], sw[kSsTC * 32], zs[2][32];
    const long long j = a.j0 + blockIdx.x;
    const size_t b = (size_t)(j / a.D);
    const int d = (int)(j % a.D), r = a.r, k = a.r * a.p, tid = threadIdx.x;
    const uint64_t key = ss_key(a.seed, a.first_draw, d);
    for (int e = tid; e < r * r; e += blockDim.x) sLQ[e] = a.LQ[b * r * r + e];
    if (tid < k) {
        double z0, z1;
        normal2(key, 16 * b + kSsZ0, (uint64_t)(tid / 2), z0, z1);
        seta[tid] = (tid & 1) ? z1 : z0;
    }
    __syncthreads();
    if (tid < k) {
        double v = a.mu0[b * k + tid];
        for (int m = 0; m <= tid; ++m) v = fma(a.LP0[(b * k + tid) * k + m], seta[m], v);
        zs[0][tid] = v;
    }
    double arow[32];
    ss_load_arow(a, b, arow);
    __syncthreads();
    ss_recursion(a, key, 16 * b + kSsEta, 0, a.T, sLQ, seta, sw, zs, arow, a.f_draw + (size_t)j * (a.T + a.H) * r);
}

// Step 4: f = f+ + g on rows 0..T-1, then rows T..T+H-1 by the recursion (eta of those rows from stream 2).
__global__ __launch_bounds__(64) void simsmooth_finish_kernel(SsArgs a) {
    __shared__ double sLQ[32 * 32], seta[kSsTC * 32], sw[kSsTC * 32], zs[2][32];
    const int s = blockIdx.x;
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.D);
    const int d = (int)(j % a.D), r = a.r, k = a.r * a.p, T = a.T, tid = threadIdx.x;
    double* F = a.f_draw + (size_t)j * (T + a.H) * r;
    const double* G = a.g + (size_t)s * T * r;
    double z = 0.0;
    if (tid < k && a.H > 0) {                                // companion state (row T-1, .., row T-p) of the draw (T >= p)
        const size_t e = (size_t)(T - 1 - tid / r) * r + tid % r;
        z = F[e] + G[e];
    }
    __syncthreads();
    for (int e = tid; e < T * r; e += blockDim.x) F[e] = F[e] + G[e];
    if (a.H == 0) return;
    for (int e = tid; e < r * r; e += blockDim.x) sLQ[e] = a.LQ[b * r * r + e];
    if (tid < k) zs[0][tid] = z;
    double arow[32];
    ss_load_arow(a, b, arow);
    __syncthreads();
    ss_recursion(a, ss_key(a.seed, a.first_draw, d), 16 * b + kSsEta, T, T + a.H, sLQ, seta, sw, zs, arow, F);
}

// The cell kernels.  FILL = false: D_ti of rows 0..T-1 into the slice's difference panels; FILL = true: x_draw rows 0..T+H-1.
// RB >= r: loadings in registers; VEC: N even and 16-byte aligned pointers (double2 loads / stores).
template <int RB, bool VEC, bool FILL>
__device__ __forceinline__ void ss_cells(const SsArgs& a) {
    extern __shared__ __attribute__((aligned(16))) double sfr[];
    const int r = a.r, N = a.N, T = a.T, TH = a.T + a.H, tid = threadIdx.x;
    const int rows = FILL ? TH : T;
    const int s = blockIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.z, blockIdx.y, s, rows);
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.D);
    const int d = (int)(j % a.D);
    const int t0 = ch.t0, t1 = ch.t1;
    cell_stage(sfr, a.f_draw + ((size_t)j * TH + t0) * r, (t1 - t0) * r);
    __syncthreads();
    const CellLane ln = cell_lane<2>(a.geo, tid, ch.s, N);
    if (!ln.live) return;
    const int i0 = ln.i0, gr = ln.g;
    const bool two = ln.n == 2;                              // (VEC: N even, always)
    CellLam<2, RB> lam;
    lam.load(a.Lam, b, N, i0, r, ln.n);
    const double sr0 = sqrt(a.R[b * N + i0]), sr1 = two ? sqrt(a.R[b * N + i0 + 1]) : 0.0;
    const bool scale = FILL && a.mean != nullptr;
    const double mu0 = scale ? a.mean[b * N + i0] : 0.0, mu1 = (scale && two) ? a.mean[b * N + i0 + 1] : 0.0;
    const double sd0 = scale ? a.sd[b * N + i0] : 1.0, sd1 = (scale && two) ? a.sd[b * N + i0 + 1] : 1.0;
    const uint64_t key = ss_key(a.seed, a.first_draw, d), stream = 16 * b + (FILL ? kSsEps : kSsEpsPlus);
    const uint64_t hN = (uint64_t)(N + 1) / 2;
    const double* px = a.panel + b * T * N + i0;
    double nx[2];                                             // the next row's cells, in flight while this row is computed
    cell_prefetch_pair<VEC>(px + (size_t)(t0 + gr) * N, t0 + gr < T && t0 + gr < t1, two, nx);
    for (int t = t0 + gr; t < t1; t += a.geo.G) {
        const double* f = sfr + (size_t)(t - t0) * r;
        const double x0 = nx[0], x1 = nx[1];
        const int tn = t + a.geo.G;
        cell_prefetch_pair<VEC>(px + (size_t)tn * N, tn < T && tn < t1, two, nx);
        double m[2];
        lam.dots(f, r, m);
        const double m0 = m[0], m1 = m[1];
        const bool o0 = x0 == x0, o1 = x1 == x1;
        double y[2];
        if constexpr (!FILL) {
            double e0 = 0.0, e1 = 0.0;
            if (o0 || o1) normal2(key, stream, (uint64_t)t * hN + (uint64_t)(i0 / 2), e0, e1);
            y[0] = o0 ? x0 - (m0 + sr0 * e0) : x0;
            y[1] = o1 ? x1 - (m1 + sr1 * e1) : x1;
        } else {
            double e0 = 0.0, e1 = 0.0;
            if (!o0 || (two && !o1)) normal2(key, stream, (uint64_t)t * hN + (uint64_t)(i0 / 2), e0, e1);
            const double v0 = o0 ? x0 : m0 + sr0 * e0, v1 = o1 ? x1 : m1 + sr1 * e1;
            y[0] = scale ? mu0 + sd0 * v0 : v0;
            y[1] = scale ? mu1 + sd1 * v1 : v1;
        }
        cell_st_pair<VEC>(FILL ? a.x_draw + ((size_t)j * TH + t) * N + i0 : a.diff + ((size_t)s * T + t) * N + i0, two, y);
    }
}

template <int RB, bool VEC>
__global__ __launch_bounds__(kSsMaxThreads) void simsmooth_diff_kernel(SsArgs a) { ss_cells<RB, VEC, false>(a); }
template <int RB, bool VEC>
__global__ __launch_bounds__(kSsMaxThreads) void simsmooth_fill_kernel(SsArgs a) { ss_cells<RB, VEC, true>(a); }

hipError_t launch_simsmooth_prep(const SsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(simsmooth_prep_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_simsmooth_expand(const SsArgs& a, hipStream_t s) {
    const size_t k = (size_t)a.r * a.p;
    const size_t per = (size_t)a.N * a.r + a.N + a.r * k + (size_t)a.r * a.r + k + k * k;
    hipLaunchKernelGGL(simsmooth_expand_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)a.S), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_simsmooth_path(const SsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(simsmooth_path_kernel, dim3((unsigned)a.S), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_simsmooth_finish(const SsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(simsmooth_finish_kernel, dim3((unsigned)a.S), dim3(64), 0, s, a);
    return hipGetLastError();
}

template <bool FILL, int RB>
static hipError_t launch_cells_rb(const SsArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)a.S, (unsigned)a.geo.nchunk, (unsigned)a.geo.nsblk);
    const size_t lds = (size_t)a.geo.RC * a.r * sizeof(double);
    if constexpr (FILL)
        return cell_launch_vec(simsmooth_fill_kernel<RB, false>, simsmooth_fill_kernel<RB, true>, vec, grid, a.geo.threads, lds, s, a);
    else
        return cell_launch_vec(simsmooth_diff_kernel<RB, false>, simsmooth_diff_kernel<RB, true>, vec, grid, a.geo.threads, lds, s, a);
}

// A lane per column pair; a staged row is f_t (cell_geometry, dfm_cellgeom.h); a 3-D grid: its y and z extents are checked.
template <bool FILL>
static hipError_t launch_cells(SsArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.S < 1) return hipErrorInvalidValue;
    a.geo = cell_geometry((a.N + 1) / 2, a.r, FILL ? a.T + a.H : a.T, kSsMaxThreads, kSsLds);
    if (a.geo.nchunk > 65535 || a.geo.nsblk > 65535) return hipErrorInvalidValue;
    const bool vec = cell_vec(a.N, a.panel, FILL ? a.x_draw : a.diff);
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_cells_rb<FILL, decltype(RB)::value>(a, vec, s); });
}

hipError_t launch_simsmooth_diff(SsArgs a, hipStream_t s) { return launch_cells<false>(a, s); }
hipError_t launch_simsmooth_fill(SsArgs a, hipStream_t s) { return launch_cells<true>(a, s); }

}  // namespace dfm
