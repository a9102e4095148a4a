// dfm_filter.h -- the one text of the forward recursion in covariance form and what else the two filter families share
// (filter.hip: the plain parametric fit; filter_ar.hip: the fit with AR idiosyncratic terms): the constants of the family, the
// positive semi-definite root of one wave's workgroup, the recursion itself (filter_recursion<WIDE>; filter_kernel and
// filter_ar_kernel are its two instances), its LDS size and launch, and the evaluation kernels' companion step.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "dfm_device.h"
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr int kFtFillMaxThreads = 512;
constexpr size_t kFtFillLds = 48 * 1024;
constexpr int kFtEvalChunk = 64;                  // origins whose states a workgroup of the evaluation advances together
constexpr int kFtFailBit = 32;

// Lower root L L' = M (leading n x n block of a matrix with rows ld apart, lower triangle read) of one wave's workgroup, as
// psd_root: a pivot <= tol_rel trace(M) gives a zero column.  Returns 1 when a pivot is below -tol_rel trace(M) or not finite
// (M is not positive semi-definite), else 0.  L: [n][n].
__device__ inline int filter_root(const double* M, int ld, int n, double* L, double tol_rel) {
    const int tid = threadIdx.x;
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += M[i * ld + i];
    const double tol = tol_rel * tr;
    for (int e = tid; e < n * n; e += blockDim.x) L[e] = 0.0;
    __syncthreads();
    int bad = (tr == tr && fabs(tr) <= 1.79e308) ? 0 : 1;
    for (int j = 0; j < n; ++j) {
        double dj = M[j * ld + j];
        for (int m = 0; m < j; ++m) dj -= L[j * n + m] * L[j * n + m];
        const bool keep = dj > tol;
        if (!(dj >= -tol)) bad = 1;
        const double ljj = keep ? sqrt(dj) : 0.0;
        for (int i = j + tid; i < n; i += blockDim.x) {
            if (i == j) {
                L[j * n + j] = ljj;
            } else {
                double v = M[i * ld + j];
                for (int m = 0; m < j; ++m) v -= L[i * n + m] * L[j * n + m];
                L[i * n + j] = keep ? v / ljj : 0.0;
            }
        }
        __syncthreads();
    }
    return bad;
}

// ---- the recursion: one wave per replicate, every matrix in LDS ---------------------------------------------------------------
// Three widths: k the state, ka = r p the columns of A that are not zero, w the leading entries of the state the observation
// loads on (b_t and C_t are nonzero in their leading w, w x w).
//   predict   z_p = M z,  P_p = M P M' + Qc          (the top r rows are products with A = [A_1 .. A_p], zero beyond ka; shifts below)
//   update    S = P_p[:, :w], P11 = S[:w] = U U' (zero columns for zero pivots), W = I + U' C_t U (w x w, SPD, eigenvalues >= 1),
//             G^-1 = I - C_t U W^-1 U',  a = b_t - C_t z_p[:w]
//             z = z_p + S G^-1 a,   P = P_p - S (G^-1 C_t) S'
//             loglik_t = -1/2 [n_t log 2 pi + ld_t + log det W + s_t - 2 b_t' z_p[:w] + z_p[:w]' C_t z_p[:w] - a' P11 G^-1 a]
// Nothing but W is factorised: Q, P_p and C_t may be singular.
// WIDE: the widths are the arguments' own (the AR fit: k = r max(p, q + 1), w = r (q + 1)).  !WIDE: the plain fit, k = ka = r p
// and w = r, written as expressions of r and p so that the compiler folds the three widths into one and the plain kernel keeps
// the index arithmetic it had with one width ("One text", has both instances' registers and times).
// LDS (doubles): A r k (zero beyond ka) | Q r r | P k k | Pp k k | X k w (A P, then C U, then S G^-1 C) | U w w |
// Y w (w+1) ([a | C_t]) | W w (w+1) (W, then W^-1 U' Y) | Lw w (w+1) (root of W, then G^-1 Y) | z k | zp k | bv w | tv w
__host__ __device__ inline size_t filter_ar_lds_doubles(int r, int k, int w) {
    return (size_t)r * k + (size_t)r * r + (size_t)2 * k * k + (size_t)k * w + (size_t)w * w + (size_t)3 * w * (w + 1) + (size_t)2 * k +
           (size_t)2 * w;
}

template <bool WIDE>
__device__ __forceinline__ void filter_recursion(const FtRec& a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, k = WIDE ? a.k : a.r * a.p, w = WIDE ? a.w : r, ka = WIDE ? a.r * a.p : k, n = a.n, N = a.N, Rp = a.Rp;
    const int tid = threadIdx.x, w1 = w + 1, kk = k * (k + 1) / 2, npR = Rp * (Rp + 1) / 2;
    const size_t b = blockIdx.x;
    double* sA = sm;
    double* sQ = sA + r * k;
    double* sP = sQ + r * r;
    double* sPp = sP + k * k;
    double* sX = sPp + k * k;
    double* sU = sX + k * w;
    double* sY = sU + w * w;
    double* sW = sY + w * w1;
    double* sL = sW + w * w1;
    double* sz = sL + w * w1;
    double* szp = sz + k;
    double* sbv = szp + k;
    double* stv = sbv + w;
    for (int e = tid; e < r * k; e += 64) {
        const int i = e / k, j = e % k;
        sA[e] = j < ka ? a.A[(b * r + i) * ka + j] : 0.0;
    }
    for (int e = tid; e < r * r; e += 64) sQ[e] = a.Q[b * r * r + e];
    for (int e = tid; e < k * k; e += 64) {       // (lower triangle read, as the packed outputs are)
        const int i = e / k, j = e % k;
        sP[e] = i >= j ? a.P0[b * k * k + e] : a.P0[b * k * k + j * k + i];
    }
    for (int e = tid; e < k; e += 64) sz[e] = a.mu0[b * k + e];
    __syncthreads();
    const double nan = __builtin_nan("");
    bool dead = false;
    for (int t = 0; t < n; ++t) {
        const size_t bt = b * n + t;
        double ll = 0.0;
        if (!dead) {
            // ---- predict
            for (int e = tid; e < k; e += 64) {
                double v;
                if (e < r) {
                    v = 0.0;
                    for (int l = 0; l < ka; ++l) v = fma(sA[e * k + l], sz[l], v);
                } else {
                    v = sz[e - r];
                }
                szp[e] = v;
            }
            for (int e = tid; e < r * k; e += 64) {
                const int i = e / k, j = e % k;
                double v = 0.0;
                for (int l = 0; l < ka; ++l) v = fma(sA[i * k + l], sP[l * k + j], v);
                sX[e] = v;
            }
            __syncthreads();
            for (int e = tid; e < k * k; e += 64) {
                const int i = e / k, j = e % k;
                if (j > i) continue;
                double v;
                if (i < r) {                      // (then j < r)
                    double vij = sQ[i * r + j], vji = sQ[j * r + i];
                    for (int l = 0; l < ka; ++l) {
                        vij = fma(sX[i * k + l], sA[j * k + l], vij);
                        vji = fma(sX[j * k + l], sA[i * k + l], vji);
                    }
                    v = 0.5 * (vij + vji);
                } else if (j < r) {
                    v = sX[j * k + (i - r)];
                } else {
                    v = sP[(i - r) * k + (j - r)];
                }
                sPp[i * k + j] = v;
                sPp[j * k + i] = v;
            }
            __syncthreads();
            // ---- update
            const int no = a.nobs[bt];
            if (no > 0) {
                const bool part = no < N;
                for (int e = tid; e < w * w; e += 64) {
                    const int i = e / w, j = e % w, hi = i > j ? i : j, lo = i > j ? j : i;
                    sY[i * w1 + 1 + j] = part ? a.Ct[bt * npR + hi * (hi + 1) / 2 + lo] : a.Cfull[b * Rp * Rp + hi * Rp + lo];
                }
                for (int e = tid; e < w; e += 64) sbv[e] = a.bcol[bt * Rp + e];
                int bad = filter_root(sPp, k, w, sU, kPsdTol);      // (its barriers also publish Y and bv)
                for (int e = tid; e < w; e += 64) {
                    double v = sbv[e];
                    for (int j = 0; j < w; ++j) v = fma(-sY[e * w1 + 1 + j], szp[j], v);
                    sY[e * w1] = v;                                 // a = b_t - C_t z_p[:w]
                }
                for (int e = tid; e < w * w; e += 64) {             // C U
                    const int i = e / w, j = e % w;
                    double v = 0.0;
                    for (int l = j; l < w; ++l) v = fma(sY[i * w1 + 1 + l], sU[l * w + j], v);
                    sX[e] = v;
                }
                __syncthreads();
                for (int e = tid; e < w * w; e += 64) {             // W = I + U' C U (lower triangle, mirrored)
                    const int i = e / w, j = e % w;
                    if (j > i) continue;
                    double v = i == j ? 1.0 : 0.0;
                    for (int l = i; l < w; ++l) v = fma(sU[l * w + i], sX[l * w + j], v);
                    sW[i * w + j] = v;
                    sW[j * w + i] = v;
                }
                __syncthreads();
                bad |= filter_root(sW, w, w, sL, 0.0);
                // the w + 1 columns of Y = [a | C]: Y2 = W^-1 U' Y, a lane per column
                for (int e = tid; e < w * w1; e += 64) {
                    const int i = e / w1, c = e % w1;
                    double v = 0.0;
                    for (int l = i; l < w; ++l) v = fma(sU[l * w + i], sY[l * w1 + c], v);
                    sW[i * w1 + c] = v;
                }
                __syncthreads();
                if (tid < w1) {
                    const int c = tid;
                    for (int i = 0; i < w; ++i) {
                        double v = sW[i * w1 + c];
                        for (int m = 0; m < i; ++m) v = fma(-sL[i * w + m], sW[m * w1 + c], v);
                        sW[i * w1 + c] = v / sL[i * w + i];
                    }
                    for (int i = w - 1; i >= 0; --i) {
                        double v = sW[i * w1 + c];
                        for (int m = i + 1; m < w; ++m) v = fma(-sL[m * w + i], sW[m * w1 + c], v);
                        sW[i * w1 + c] = v / sL[i * w + i];
                    }
                }
                if (tid < w) stv[tid] = 2.0 * log(sL[tid * w + tid]);   // log det W, term by term
                __syncthreads();
                // G^-1 Y = Y - (C U) Y2 into the root's place: column 0 = G^-1 a, columns 1 .. w = G^-1 C
                for (int e = tid; e < w * w1; e += 64) {
                    const int i = e / w1, c = e % w1;
                    double v = sY[e];
                    for (int l = 0; l < w; ++l) v = fma(-sX[i * w + l], sW[l * w1 + c], v);
                    sL[e] = v;
                }
                __syncthreads();
                // log-likelihood terms of row i, and z = z_p + S G^-1 a
                if (tid < w) {
                    const int i = tid;
                    double cf = 0.0, pg = 0.0;
                    for (int j = 0; j < w; ++j) {
                        cf = fma(sY[i * w1 + 1 + j], szp[j], cf);
                        pg = fma(sPp[i * k + j], sL[j * w1], pg);
                    }
                    stv[i] += szp[i] * (cf - 2.0 * sbv[i]) - sY[i * w1] * pg;
                }
                for (int e = tid; e < k; e += 64) {
                    double v = szp[e];
                    for (int j = 0; j < w; ++j) v = fma(sPp[e * k + j], sL[j * w1], v);
                    sz[e] = v;
                }
                __syncthreads();
                // S (G^-1 C) with G^-1 C symmetrised, then P = P_p - (S G^-1 C) S' on the lower triangle, mirrored
                for (int e = tid; e < k * w; e += 64) {
                    const int i = e / w, j = e % w;
                    double v = 0.0;
                    for (int l = 0; l < w; ++l) v = fma(sPp[i * k + l], 0.5 * (sL[l * w1 + 1 + j] + sL[j * w1 + 1 + l]), v);
                    sX[e] = v;
                }
                double qd = 0.0;
                for (int i = 0; i < w; ++i) qd += stv[i];
                ll = -0.5 * ((double)no * kLog2Pi + (part ? a.ldrow[bt] : a.ldfull[b]) + a.scol[bt] + qd);
                __syncthreads();
                for (int e = tid; e < k * k; e += 64) {
                    const int i = e / k, j = e % k;
                    if (j > i) continue;
                    double v = sPp[i * k + j];
                    for (int l = 0; l < w; ++l) v = fma(-sX[i * w + l], sPp[j * k + l], v);
                    sP[i * k + j] = v;
                    sP[j * k + i] = v;
                }
                bool fin = ll == ll && fabs(ll) <= 1.79e308;
                for (int e = tid; e < k; e += 64) fin = fin && sz[e] == sz[e] && fabs(sz[e]) <= 1.79e308;
                if (bad || __any(!fin)) dead = true;
            } else {
                for (int e = tid; e < k * k; e += 64) sP[e] = sPp[e];
                for (int e = tid; e < k; e += 64) sz[e] = szp[e];
                bool fin = true;
                for (int e = tid; e < k; e += 64) fin = fin && szp[e] == szp[e] && fabs(szp[e]) <= 1.79e308;
                if (__any(!fin)) dead = true;
            }
            __syncthreads();
            if (dead && tid == 0) atomicOr(a.status, kFtFailBit);
        }
        // ---- the period's outputs (NaN from the failed period on)
        for (int e = tid; e < k; e += 64) {
            if (a.z_pred) a.z_pred[bt * k + e] = dead ? nan : szp[e];
            if (a.z_filt) a.z_filt[bt * k + e] = dead ? nan : sz[e];
        }
        if (a.P_pred || a.P_filt)
            for (int e = tid; e < k * k; e += 64) {
                const int i = e / k, j = e % k;
                if (j > i) continue;
                const size_t o = bt * kk + i * (i + 1) / 2 + j;
                if (a.P_pred) a.P_pred[o] = dead ? nan : sPp[e];
                if (a.P_filt) a.P_filt[o] = dead ? nan : sP[e];
            }
        if (a.loglik_t && tid == 0) a.loglik_t[bt] = dead ? nan : ll;
        __syncthreads();
    }
}

// A recursion kernel's launch, a wave per replicate, with the kernel's own opt-in to more than 64 KB of LDS.
inline hipError_t launch_filter_recursion(void (*kern)(FtRec), LdsOptIn& attr_done, const FtRec& a, hipStream_t s) {
    const size_t lds = filter_ar_lds_doubles(a.r, a.k, a.w) * sizeof(double);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (!attr_done && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.B), dim3(64), lds, s, a);
    return hipGetLastError();
}

// ---- the evaluation kernels' companion step ----------------------------------------------------------------------------------
// nxt = M cur for the no origins of a chunk ([no][k] each), all threads of the workgroup, an (origin, component) pair each: the
// top r rows are products with A (sA: [r][ka], the columns of A that are not zero; ka = k in the plain fit), the rest are shifts.
__device__ __forceinline__ void filter_eval_step(const double* sA, int ka, const double* cur, double* nxt, int no, int r, int k) {
    for (int e = threadIdx.x; e < no * k; e += blockDim.x) {
        const int o = e / k, m = e % k;
        double v;
        if (m < r) {
            v = 0.0;
            for (int l = 0; l < ka; ++l) v = fma(sA[m * ka + l], cur[o * k + l], v);
        } else {
            v = cur[o * k + m - r];
        }
        nxt[e] = v;
    }
}

}  // namespace dfm
