// signirf.hip -- sign-restricted structural impulse responses (dfm_signirf_batch, capi.hip; semantics in include/dfm_hip.h).
// sv_prep_kernel (structural.hip) supplies the base impact matrix S and the tables Theta_h = Psi_h S of every replicate; then
//   sv_sign_table_kernel  one workgroup per replicate: a_{i,h} = sd_i lam_i' Theta_h (Theta^c_h where cum[i]) for the distinct
//                         restricted series i and h <= max h1.  The candidates never touch Lam.
//   sv_sign_kernel        the hot path: a workgroup owns a replicate and kSgLanes candidates, the replicate's table in LDS (every
//                         lane reads the same address: a broadcast).  A lane draws Z [r][r] from its candidate's key, factors it
//                         by Gram-Schmidt with a second orthogonalisation pass (Z = Rot U, diag U > 0: the Haar draw), evaluates the
//                         restrictions shock by shock (the shock index is a compile-time constant, so Rot stays in registers), and
//                         writes the mask, the accepted count of its wave and, if accepted, Rot D.  r <= 8: Rot in registers.
//                         r > 8: the same text on the candidate's slot of the scratch in global memory -- correct, not fast.
//   sv_sign_keep_kernel   a workgroup per (replicate, kSgKeepSlots kept slots): prefix sums of the wave counts in candidate order,
//                         cand_out, n_accept, S_out = S Rot D and the slots' tables Theta_h Rot D (NaN for an empty slot), which
//                         sv_irf_fill_kernel then streams into irf / fevd with SvArgs::slots = K.
// No floating-point atomics and no integer ones either: every count is a ballot or a sum in a fixed order.
#include "dfm_kernels.h"
#include "dfm_philox.h"

namespace dfm {

constexpr int kSgLanes = 256;                 // sv_sign_kernel: candidates per workgroup, 64 per wave
constexpr int kSgKeepSlots = 32;              // sv_sign_keep_kernel: kept slots per workgroup
constexpr uint64_t kSgStream = 10;            // stream word 16 b + 10 (1-9: simsmooth.hip, gibbs.hip)
constexpr double kSgPivTol = 1e-12;           // a pivot |U_jj| <= this x max|Z| rejects the candidate

// Z [n][n] in registers (n = R, every index a compile-time constant once the loops are unrolled) ...
template <int R>
struct SgRegMat {
    double z[R][R];
    __device__ __forceinline__ double get(int i, int j) const { return z[i][j]; }
    __device__ __forceinline__ void set(int i, int j, double v) { z[i][j] = v; }
};
// ... or in the candidate's slot of the scratch (row-major, the layout sv_sign_keep_kernel reads)
struct SgMemMat {
    double* z; int n;
    __device__ __forceinline__ double get(int i, int j) const { return z[i * n + j]; }
    __device__ __forceinline__ void set(int i, int j, double v) { z[i * n + j] = v; }
};

// One candidate: fills Z, leaves Rot in it, returns whether the candidate is accepted and the columns to flip (bit k).
// R > 0: n = R at compile time; R = 0: n = a.r.  tab: the replicate's table [nS][HT][n] in LDS.
template <int R, class Mat>
__device__ __forceinline__ bool sg_candidate(const SgArgs& a, size_t b, int m, const double* tab, Mat& Z, unsigned& flips) {
    const int n = R ? R : a.r, nn = n * n;
    const uint64_t key = a.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(a.first_cand + m + 1));
    double amax = 0.0;
#pragma unroll
    for (int q = 0; q < (nn + 1) / 2; ++q) {
        double z0, z1;
        normal2(key, 16 * (uint64_t)b + kSgStream, (uint64_t)q, z0, z1);
        Z.set((2 * q) / n, (2 * q) % n, z0);
        amax = fmax(amax, fabs(z0));
        if (2 * q + 1 < nn) {
            Z.set((2 * q + 1) / n, (2 * q + 1) % n, z1);
            amax = fmax(amax, fabs(z1));
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < n; ++j) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int i = 0; i < j; ++i) {
                double d = 0.0;
#pragma unroll
                for (int t = 0; t < n; ++t) d = fma(Z.get(t, i), Z.get(t, j), d);
#pragma unroll
                for (int t = 0; t < n; ++t) Z.set(t, j, fma(-d, Z.get(t, i), Z.get(t, j)));
            }
        }
        double ss = 0.0;
#pragma unroll
        for (int t = 0; t < n; ++t) ss = fma(Z.get(t, j), Z.get(t, j), ss);
        const double nrm = sqrt(ss);
        ok = ok && nrm > kSgPivTol * amax;
        const double inv = 1.0 / nrm;
#pragma unroll
        for (int t = 0; t < n; ++t) Z.set(t, j, Z.get(t, j) * inv);
    }
    flips = 0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
        const int g0 = a.gs[k], g1 = a.gs[k + 1];
        if (g0 == g1) continue;
        bool pos = true, neg = true;
        for (int g = g0; g < g1; ++g) {
            const int s = a.rows[4 * g], h0 = a.rows[4 * g + 1], h1 = a.rows[4 * g + 2], sg = a.rows[4 * g + 3];
            for (int h = h0; h <= h1; ++h) {
                const double* t = tab + ((size_t)s * a.HT + h) * n;
                double v = 0.0;
#pragma unroll
                for (int q = 0; q < n; ++q) v = fma(t[q], Z.get(q, k), v);
                v = sg > 0 ? v : -v;
                pos = pos && v > 0.0;
                neg = neg && v < 0.0;
            }
        }
        if (!pos) {
            if (neg) flips |= 1u << k;
            else ok = false;
        }
    }
    return ok;
}

__global__ __launch_bounds__(256) void sv_sign_table_kernel(SgArgs a) {
    const size_t b = blockIdx.x;
    const int r = a.r, rr = r * r, n = a.nS * a.HT * r;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int m = e % r, h = (e / r) % a.HT, s = e / (r * a.HT);
        const int i = a.ser[s];
        const bool c = a.cum != nullptr && a.cum[i] != 0;
        const double* T = (c ? a.Thc : a.Th) + (b * a.H + h) * rr + (size_t)m * r;      // shock-major: T[j] = (Theta_h)_jm
        const double* lam = a.Lam + (b * a.N + i) * r;
        double v = 0.0;
        for (int j = 0; j < r; ++j) v = fma(lam[j], T[j], v);
        a.tab[b * n + e] = a.sd ? a.sd[b * a.N + i] * v : v;
    }
}

// R in 1..8: Rot in registers.  R = 0: any r, Rot in the scratch.
template <int R>
__global__ __launch_bounds__(kSgLanes) void sv_sign_kernel(SgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, n = R ? R : a.r, nn = n * n;
    const unsigned nblk = (unsigned)((a.M + kSgLanes - 1) / kSgLanes);
    const size_t b = blockIdx.x / nblk;
    const int m = (int)(blockIdx.x % nblk) * kSgLanes + tid;
    const int ntab = a.nS * a.HT * n;
    for (int e = tid; e < ntab; e += blockDim.x) sm[e] = a.tab[b * ntab + e];
    __syncthreads();
    const bool live = m < a.M;
    bool ok = false;
    if (live) {
        double* slot = a.rot + (b * a.M + m) * nn;
        unsigned flips;
        if constexpr (R > 0) {
            SgRegMat<R> Z;
            ok = sg_candidate<R>(a, b, m, sm, Z, flips);
            if (ok) {
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int j = 0; j < R; ++j) slot[i * R + j] = (flips >> j & 1u) ? -Z.z[i][j] : Z.z[i][j];
            }
        } else {
            SgMemMat Z{slot, n};
            ok = sg_candidate<0>(a, b, m, sm, Z, flips);
            if (ok && flips)
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j)
                        if (flips >> j & 1u) slot[i * n + j] = -slot[i * n + j];
        }
        a.mask[b * a.M + m] = ok ? 1 : 0;
    }
    const unsigned long long acc = __ballot(ok);
    const int m0 = m - (tid & 63);                                   // the wave's first candidate
    if ((tid & 63) == 0 && m0 < a.M) a.wcnt[b * ((a.M + 63) / 64) + m0 / 64] = __popcll(acc);
}

__global__ __launch_bounds__(256) void sv_sign_keep_kernel(SgArgs a) {
    __shared__ int ssum[256], ssel[kSgKeepSlots];
    __shared__ double sRD[1024];
    const int tid = threadIdx.x, r = a.r, rr = r * r, K = a.K, M = a.M, H = a.H;
    const unsigned nkb = (unsigned)((K + kSgKeepSlots - 1) / kSgKeepSlots);
    const size_t b = blockIdx.x / nkb;
    const int kb = (int)(blockIdx.x % nkb);
    const int s0 = kb * kSgKeepSlots, s1 = s0 + kSgKeepSlots < K ? s0 + kSgKeepSlots : K;
    const int nW = (M + 63) / 64, seg = (nW + 255) / 256;
    const int w0 = tid * seg < nW ? tid * seg : nW, w1 = w0 + seg < nW ? w0 + seg : nW;
    const int* wc = a.wcnt + b * nW;
    const int* mask = a.mask + b * M;
    int cnt = 0;
    for (int w = w0; w < w1; ++w) cnt += wc[w];
    ssum[tid] = cnt;
    if (tid < kSgKeepSlots) ssel[tid] = -1;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                        // inclusive scan of the 256 segment counts
        const int v = tid >= off ? ssum[tid - off] : 0;
        __syncthreads();
        ssum[tid] += v;
        __syncthreads();
    }
    int base = ssum[tid] - cnt;                                      // accepted candidates in front of this thread's segment
    for (int w = w0; w < w1; ++w) {
        const int c = wc[w];
        if (c > 0 && base < s1 && base + c > s0) {                   // some of this wave's candidates land in this workgroup's slots
            int sl = base;
            for (int l = 0; l < 64 && w * 64 + l < M; ++l)
                if (mask[w * 64 + l]) {
                    if (sl >= s0 && sl < s1) ssel[sl - s0] = w * 64 + l;
                    ++sl;
                }
        }
        base += c;
    }
    __syncthreads();
    if (kb == 0 && tid == 0) a.n_accept[b] = ssum[255];
    if (tid < s1 - s0) a.cand_out[b * K + s0 + tid] = ssel[tid];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double* S = a.S + b * rr;
    for (int s = s0; s < s1; ++s) {
        const int cand = ssel[s - s0];
        const size_t bs = b * K + s;
        if (cand >= 0)
            for (int e = tid; e < rr; e += blockDim.x) sRD[e] = a.rot[(b * M + cand) * rr + e];
        __syncthreads();
        if (a.S_out)
            for (int e = tid; e < rr; e += blockDim.x) {
                const int i = e / r, k = e % r;
                double v = nan;
                if (cand >= 0) {
                    v = 0.0;
                    for (int j = 0; j < r; ++j) v = fma(S[i * r + j], sRD[j * r + k], v);
                }
                a.S_out[bs * rr + e] = v;
            }
        if (a.ThK)
            for (int e = tid; e < H * rr; e += blockDim.x) {         // ThK[h][k][i] = (Theta_h Rot D)_ik, shock-major as Th
                const int i = e % r, k = (e / r) % r, h = e / rr;
                double v = nan, vc = nan;
                if (cand >= 0) {
                    const double* T = a.Th + (b * H + h) * rr + i;   // T[j r] = (Theta_h)_ij
                    v = 0.0;
                    for (int j = 0; j < r; ++j) v = fma(T[j * r], sRD[j * r + k], v);
                    if (a.ThcK) {
                        const double* Tc = a.Thc + (b * H + h) * rr + i;
                        vc = 0.0;
                        for (int j = 0; j < r; ++j) vc = fma(Tc[j * r], sRD[j * r + k], vc);
                    }
                }
                a.ThK[bs * H * rr + e] = v;
                if (a.ThcK) a.ThcK[bs * H * rr + e] = vc;
            }
        __syncthreads();
    }
}

hipError_t launch_sv_sign_table(const SgArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sv_sign_table_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

size_t sign_table_bytes(int nS, int HT, int r) { return (size_t)nS * HT * r * sizeof(double); }

template <int R>
static hipError_t launch_sign_r(const SgArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((sv_sign_kernel<R>), dim3(blocks), dim3(kSgLanes), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_sv_sign(const SgArgs& a, hipStream_t s) {
    const size_t blocks = (size_t)a.B * ((a.M + kSgLanes - 1) / kSgLanes);
    const size_t lds = sign_table_bytes(a.nS, a.HT, a.r);
    if (a.r < 1 || a.r > 32 || blocks > 0x7fffffffu || lds > kSgTabLds) return hipErrorInvalidValue;
    switch (a.r) {
        case 1: return launch_sign_r<1>(a, (unsigned)blocks, lds, s);
        case 2: return launch_sign_r<2>(a, (unsigned)blocks, lds, s);
        case 3: return launch_sign_r<3>(a, (unsigned)blocks, lds, s);
        case 4: return launch_sign_r<4>(a, (unsigned)blocks, lds, s);
        case 5: return launch_sign_r<5>(a, (unsigned)blocks, lds, s);
        case 6: return launch_sign_r<6>(a, (unsigned)blocks, lds, s);
        case 7: return launch_sign_r<7>(a, (unsigned)blocks, lds, s);
        case 8: return launch_sign_r<8>(a, (unsigned)blocks, lds, s);
        default: return launch_sign_r<0>(a, (unsigned)blocks, lds, s);
    }
}

hipError_t launch_sv_sign_keep(const SgArgs& a, hipStream_t s) {
    const size_t blocks = (size_t)a.B * ((a.K + kSgKeepSlots - 1) / kSgKeepSlots);
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sv_sign_keep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
