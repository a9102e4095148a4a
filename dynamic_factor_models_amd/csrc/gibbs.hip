// gibbs.hip -- the block "parameters | factor path" of the Gibbs sampler (dfm_gibbs_batch, capi.hip; include/dfm_hip.h): for chain b
// and the factor path f the simulation smoother drew for this sweep,
//   gibbs_gram_kernel  (balanced panels only) the root of tau_lam I + F'F, once per chain
//   gibbs_load_kernel  lam_i, R_i | f: N conjugate regressions per chain, one series per lane -- the hot path
//   gibbs_var_kernel   A, Q | f: one matrix-normal / inverse-Wishart draw per chain, one workgroup per chain
// Every random number is a pure function of (key, stream word 16 b + s, index) with key = seed ^ (0x9E3779B97F4A7C15 (sweep + 1)),
// the key of dfm_simsmooth_batch with first_draw = sweep:
//   s = 5 normals of lam_i (idx i ceil(r/2) + k/2), 6 Gamma of R_i (item i of N), 7 normals E of A' (idx row ceil(r/2) + k/2),
//   8 normals of the Bartlett factor's strict lower part, 9 its Gammas (item j of r).
// Gamma(a, 1), a >= 1, is Marsaglia and Tsang (2000): attempt k of item i of n uses counter m = k n + i -- z = first normal of
// normal2(2 m), u = uniform1(2 m + 1); 32 rejected attempts raise the status bit.  No floating-point atomics: every sum runs over
// t in one fixed order, so two runs agree bit for bit.
#include "dfm_gibbs.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr int kGbTC = 64;                     // gibbs_load_kernel / gibbs_gram_kernel: f rows staged per chunk
constexpr int kGbVarTC = 32;                  // gibbs_var_kernel: rows per chunk (behind the p lag rows)
constexpr int kGbThreads = 256;

// One workgroup per chain: L L' = tau_lam I + F'F over all T rows (what every series of a balanced panel shares).
__global__ __launch_bounds__(kGbThreads) void gibbs_gram_kernel(GbArgs a) {
    __shared__ double sf[kGbTC * 32], S[32 * 32], L[32 * 32];
    const size_t b = blockIdx.x;
    const int r = a.r, T = a.T, tid = threadIdx.x, rr = a.r * a.r;
    const double* F = a.f + b * T * r;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < T; t0 += kGbTC) {
        const int nt = T - t0 < kGbTC ? T - t0 : kGbTC;
        __syncthreads();
        for (int e = tid; e < nt * r; e += kGbThreads) sf[e] = F[(size_t)t0 * r + e];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * kGbThreads;
            if (e < rr) {
                const int i = e / r, j = e % r;
                double v = acc[u];
                for (int tt = 0; tt < nt; ++tt) v = fma(sf[tt * r + i], sf[tt * r + j], v);
                acc[u] = v;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + u * kGbThreads;
        if (e < rr) S[e] = acc[u] + ((e / r == e % r) ? a.tau_lam : 0.0);
    }
    __syncthreads();
    const int dropped = psd_root(S, r, L, kPsdTol);
    if (dropped && tid == 0) atomicOr(a.status, kGbFailBit);
    for (int e = tid; e < rr; e += kGbThreads) a.Lsh[b * rr + e] = L[e];
}

// lam_i, R_i | f.  blockIdx.x = chain, blockIdx.y = block of series; one series per lane.  The chain's f rows go through LDS in
// chunks of kGbTC rows, the panel rows are read coalesced across the series.  RB <= 16: the loops run to RB at compile time and the
// packed Gram matrix, sum f x, sum x^2 and n_i live in registers (columns r .. RB-1 of f are zero: those coordinates decouple);
// RB = 32: the loops run to r and the arrays are indexed at run time (scratch).  MISS = false: sum f x and sum x^2 only, the root
// comes from gibbs_gram_kernel.
template <int RB, bool MISS>
__global__ __launch_bounds__(kGbThreads) void gibbs_load_kernel(GbArgs a) {
    constexpr bool REG = RB <= 16;
    constexpr int NP = MISS ? RB * (RB + 1) / 2 : 1;
    __shared__ double sf[kGbTC * RB];
    __shared__ double sL[MISS ? 1 : RB * RB];
    const int r = a.r, N = a.N, T = a.T, tid = threadIdx.x, nth = blockDim.x;   // (whole waves over the block's series: <= 256)
    const int n = REG ? RB : r;
    const size_t b = blockIdx.x;
    const int nsblk = gridDim.y, npb = (N + nsblk - 1) / nsblk;
    const int i = blockIdx.y * npb + tid;
    const bool active = tid < npb && i < N;
    const double* X = a.panel + b * T * N;
    const double* F = a.f + b * T * r;
    double G[NP], s[RB];
    double xx = 0.0, cnt = 0.0;
#pragma unroll
    for (int e = 0; e < NP; ++e) G[e] = 0.0;
#pragma unroll
    for (int q = 0; q < RB; ++q) s[q] = 0.0;
    if constexpr (!MISS) {
        for (int e = tid; e < n * n; e += nth) {
            const int ii = e / n, jj = e % n;
            sL[e] = (ii < r && jj < r) ? a.Lsh[(b * r + ii) * r + jj] : (ii == jj ? 1.0 : 0.0);
        }
    }
    for (int t0 = 0; t0 < T; t0 += kGbTC) {
        const int nt = T - t0 < kGbTC ? T - t0 : kGbTC;
        __syncthreads();
        for (int e = tid; e < nt * n; e += nth) {
            const int tt = e / n, q = e % n;
            sf[e] = q < r ? F[(size_t)(t0 + tt) * r + q] : 0.0;
        }
        __syncthreads();
        if (active) {
            double xn = X[(size_t)t0 * N + i];
            for (int tt = 0; tt < nt; ++tt) {
                const double x = xn;
                if (tt + 1 < nt) xn = X[(size_t)(t0 + tt + 1) * N + i];
                const double* fr = sf + tt * n;
                if (!MISS || x == x) {
                    xx = fma(x, x, xx);
                    cnt += 1.0;
#pragma unroll
                    for (int q = 0; q < n; ++q) {
                        const double fq = fr[q];
                        s[q] = fma(fq, x, s[q]);
                        if constexpr (MISS) {
#pragma unroll
                            for (int m = 0; m <= q; ++m) G[q * (q + 1) / 2 + m] = fma(fq, fr[m], G[q * (q + 1) / 2 + m]);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();                                          // (sL, staged before the first chunk, when T rows fit no chunk at all)
    if (!active) return;
    bool bad = false;
    if constexpr (MISS) {                                     // S = tau_lam I + G = L L', in place in the packed lower triangle
        double tr = 0.0;                                      // psd_root's rule: a pivot <= kPsdTol trace(S) fails (the r real coordinates)
#pragma unroll
        for (int j = 0; j < n; ++j)
            if (j < r) tr += G[j * (j + 1) / 2 + j] + a.tau_lam;
        const double tol = kPsdTol * tr;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            double dj = G[j * (j + 1) / 2 + j] + a.tau_lam;
#pragma unroll
            for (int m = 0; m < j; ++m) dj = fma(-G[j * (j + 1) / 2 + m], G[j * (j + 1) / 2 + m], dj);
            bad |= j < r && !(dj > tol);
            const double ljj = sqrt(dj), inv = 1.0 / ljj;
            G[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
            for (int i2 = j + 1; i2 < n; ++i2) {
                double v = G[i2 * (i2 + 1) / 2 + j];
#pragma unroll
                for (int m = 0; m < j; ++m) v = fma(-G[i2 * (i2 + 1) / 2 + m], G[j * (j + 1) / 2 + m], v);
                G[i2 * (i2 + 1) / 2 + j] = v * inv;
            }
        }
    }
    auto Lat = [&](int p, int q) -> double {
        if constexpr (MISS) return G[p * (p + 1) / 2 + q];
        else return sL[p * n + q];
    };
    // y = L^-1 sum f x (in s); m' S m = y'y
    double yy = 0.0;
#pragma unroll
    for (int p = 0; p < n; ++p) {
        double v = s[p];
#pragma unroll
        for (int q = 0; q < p; ++q) v = fma(-Lat(p, q), s[q], v);
        v = v / Lat(p, p);
        s[p] = v;
        yy = fma(v, v, yy);
    }
    const uint64_t key = gb_key(a.seed, a.sweep);
    bool capped = false;
    const double ga = 0.5 * (a.nu_R + cnt), gbb = 0.5 * (a.nu_R * a.s_R + xx - yy);
    const double g = gb_gamma(key, 16 * b + kGbRGam, i, N, ga, capped);
    const double Ri = gbb / g;
    bad |= !(Ri > 0.0);
    const double sr = sqrt(Ri);
    // lam = L^-T (y + sqrt(R_i) z)
    const int hr = (r + 1) / 2;
#pragma unroll
    for (int q2 = 0; q2 < (n + 1) / 2; ++q2) {
        double z0 = 0.0, z1 = 0.0;
        if (q2 < hr) normal2(key, 16 * b + kGbLamN, (uint64_t)i * hr + q2, z0, z1);
        s[2 * q2] = fma(sr, z0, s[2 * q2]);
        if (2 * q2 + 1 < n && 2 * q2 + 1 < r) s[2 * q2 + 1] = fma(sr, z1, s[2 * q2 + 1]);
    }
#pragma unroll
    for (int pp = 0; pp < n; ++pp) {
        const int p = n - 1 - pp;
        double v = s[p];
#pragma unroll
        for (int q = p + 1; q < n; ++q) v = fma(-Lat(q, p), s[q], v);
        s[p] = v / Lat(p, p);
    }
    if (bad || capped) atomicOr(a.status, kGbFailBit);
    if (bad) return;                                          // a failed draw leaves the series' lam_i, R_i as they were
#pragma unroll
    for (int q = 0; q < n; ++q)
        if (q < r) a.Lam[(b * N + i) * r + q] = s[q];
    a.R[b * N + i] = Ri;
}

// A, Q | f.  One workgroup per chain.  Rows t = p .. T-1: Y_t = f_t, Z_t = (f_t-1, .., f_t-p).  Every entry of Z'Z, Z'Y and Y'Y is
// one thread's sum over t in ascending order.
//   S = tau_A I + Z'Z = L L';  U = L^-1 (tau_A A0' + Z'Y);  M = L^-T U;  Psi = s_Q I + Y'Y + tau_A A0 A0' - U'U = C C'
//   Q = G G', G = C B_T^-T (B_T: the Bartlett factor of Wishart(nu_Q + n, I));  A' = M + L^-T E G'
__global__ __launch_bounds__(kGbThreads) void gibbs_var_kernel(GbArgs a) {
    __shared__ double sS[1024], sL[1024], sU[1024], sP[1024], sC[1024], st[2048];
    const size_t b = blockIdx.x;
    const int r = a.r, p = a.p, k = a.r * a.p, T = a.T, tid = threadIdx.x;
    const int nzz = k * k, nzy = k * r, ne = nzz + nzy + r * r, nrow = T - p;
    const double* F = a.f + b * T * r;
    const double* A0 = a.A0 ? a.A0 + b * r * k : nullptr;
    // an entry is the product of two staged columns: (row offset relative to the chunk's first row) * r + column
    int oa[12], ob[12];
    double acc[12];
    auto zoff = [&](int c) { return (p - 1 - c / r) * r + c % r; };
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int e = tid + u * kGbThreads;
        acc[u] = 0.0; oa[u] = 0; ob[u] = 0;
        if (e < nzz) { oa[u] = zoff(e / k); ob[u] = zoff(e % k); }
        else if (e < nzz + nzy) { oa[u] = zoff((e - nzz) / r); ob[u] = p * r + (e - nzz) % r; }
        else if (e < ne) { oa[u] = p * r + (e - nzz - nzy) / r; ob[u] = p * r + (e - nzz - nzy) % r; }
    }
    for (int c0 = p; c0 < T; c0 += kGbVarTC) {
        const int nt = T - c0 < kGbVarTC ? T - c0 : kGbVarTC;
        __syncthreads();
        for (int e = tid; e < (nt + p) * r; e += kGbThreads) st[e] = F[(size_t)(c0 - p) * r + e];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            if (tid + u * kGbThreads < ne) {
                double v = acc[u];
                for (int tt = 0; tt < nt; ++tt) v = fma(st[tt * r + oa[u]], st[tt * r + ob[u]], v);
                acc[u] = v;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int e = tid + u * kGbThreads;
        if (e < nzz) {
            sS[e] = acc[u] + ((e / k == e % k) ? a.tau_A : 0.0);
        } else if (e < nzz + nzy) {
            const int e2 = e - nzz, ar = e2 / r, c = e2 % r;
            sU[e2] = acc[u] + (A0 ? a.tau_A * A0[c * k + ar] : 0.0);
        } else if (e < ne) {
            sP[e - nzz - nzy] = acc[u];
        }
    }
    __syncthreads();
    int dropped = psd_root(sS, k, sL, kPsdTol);
    if (tid < r) {                                            // U = L^-1 rhs, column tid
        for (int ar = 0; ar < k; ++ar) {
            double v = sU[ar * r + tid];
            for (int m = 0; m < ar; ++m) v = fma(-sL[ar * k + m], sU[m * r + tid], v);
            sU[ar * r + tid] = v / sL[ar * k + ar];
        }
    }
    __syncthreads();
    for (int e = tid; e < r * r; e += kGbThreads) {
        const int i = e / r, j = e % r;
        double v = sP[e] + (i == j ? a.s_Q : 0.0);
        if (A0) {
            double w = 0.0;
            for (int m = 0; m < k; ++m) w = fma(A0[i * k + m], A0[j * k + m], w);
            v = fma(a.tau_A, w, v);
        }
        double w = 0.0;
        for (int m = 0; m < k; ++m) w = fma(sU[m * r + i], sU[m * r + j], w);
        sP[e] = v - w;
    }
    __syncthreads();
    dropped += psd_root(sP, r, sC, kPsdTol);
    if (dropped) {                                            // (the same in every thread) a failed draw leaves A, Q as they were
        if (tid == 0) atomicOr(a.status, kGbFailBit);
        return;
    }
    // (psd_root ends on a barrier: sP and sS are free)
    const uint64_t key = gb_key(a.seed, a.sweep);
    const int hr = (r + 1) / 2, nlow = r * (r - 1) / 2;
    bool capped = false;
    for (int e = tid; e < r * r; e += kGbThreads) sP[e] = 0.0;
    __syncthreads();
    if (tid < r) {
        const double nu = a.nu_Q + (double)nrow;
        sP[tid * r + tid] = sqrt(2.0 * gb_gamma(key, 16 * b + kGbBartG, tid, r, 0.5 * (nu - tid), capped));
        for (int ar = k - 1; ar >= 0; --ar) {                 // M = L^-T U, column tid
            double v = sU[ar * r + tid];
            for (int m = ar + 1; m < k; ++m) v = fma(-sL[m * k + ar], sU[m * r + tid], v);
            sU[ar * r + tid] = v / sL[ar * k + ar];
        }
    }
    for (int q = tid; q < (nlow + 1) / 2; q += kGbThreads) {
        double z0, z1;
        normal2(key, 16 * b + kGbBartN, (uint64_t)q, z0, z1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 2 * q + h;
            if (e < nlow) {
                int j = 1;
                while ((j + 1) * j / 2 <= e) ++j;             // e = j (j - 1) / 2 + c, c < j
                sP[j * r + (e - j * (j - 1) / 2)] = h ? z1 : z0;
            }
        }
    }
    for (int e = tid; e < k * hr; e += kGbThreads) {          // E [k][r] into st
        const int row = e / hr, q = e % hr;
        double z0, z1;
        normal2(key, 16 * b + kGbVarE, (uint64_t)row * hr + q, z0, z1);
        st[row * r + 2 * q] = z0;
        if (2 * q + 1 < r) st[row * r + 2 * q + 1] = z1;
    }
    __syncthreads();
    if (tid < r) {                                            // G B_T' = C, row tid, into sS
        for (int j = 0; j < r; ++j) {
            double v = sC[tid * r + j];
            for (int m = 0; m < j; ++m) v = fma(-sS[tid * r + m], sP[j * r + m], v);
            sS[tid * r + j] = v / sP[j * r + j];
        }
    }
    __syncthreads();
    for (int e = tid; e < r * r; e += kGbThreads) {
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int m = 0; m < r; ++m) v = fma(sS[i * r + m], sS[j * r + m], v);
        a.Q[b * r * r + e] = v;
    }
    double* W = st + 1024;
    for (int e = tid; e < k * r; e += kGbThreads) {           // W = E G'
        const int ar = e / r, c = e % r;
        double v = 0.0;
        for (int m = 0; m < r; ++m) v = fma(st[ar * r + m], sS[c * r + m], v);
        W[e] = v;
    }
    __syncthreads();
    if (tid < r) {                                            // A' = M + L^-T W, column tid
        for (int ar = k - 1; ar >= 0; --ar) {
            double v = W[ar * r + tid];
            for (int m = ar + 1; m < k; ++m) v = fma(-sL[m * k + ar], W[m * r + tid], v);
            v = v / sL[ar * k + ar];
            W[ar * r + tid] = v;
            a.A[(b * r + tid) * k + ar] = sU[ar * r + tid] + v;
        }
    }
    if (capped) atomicOr(a.status, kGbFailBit);
}

hipError_t launch_gibbs_gram(const GbArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gibbs_gram_kernel, dim3((unsigned)a.B), dim3(kGbThreads), 0, s, a);
    return hipGetLastError();
}

template <int RB>
static hipError_t launch_load_rb(const GbArgs& a, const dim3& grid, const dim3& block, hipStream_t s) {
    if (a.missing) hipLaunchKernelGGL((gibbs_load_kernel<RB, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gibbs_load_kernel<RB, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

// Series blocks of at most 256 lanes, as even as they come (cell_geometry's split); threads rounded up to whole waves.
hipError_t launch_gibbs_load(const GbArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 32) return hipErrorInvalidValue;
    const int nsblk = (a.N + kCellBlockLanes - 1) / kCellBlockLanes, npb = (a.N + nsblk - 1) / nsblk;
    if (nsblk > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.B, (unsigned)nsblk), block((unsigned)((npb + 63) / 64 * 64));
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_load_rb<decltype(RB)::value>(a, grid, block, s); });
}

hipError_t launch_gibbs_var(const GbArgs& a, hipStream_t s) {
    if (a.r * a.p > 32 || a.T <= a.p) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gibbs_var_kernel, dim3((unsigned)a.B), dim3(kGbThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
