// filter.hip -- filtered states, one-step prediction errors and the pseudo-out-of-sample record of a fitted parametric DFM
// (dfm_filter_batch, capi.hip).
//
// Model  x_t = Lam f_t + e_t, e_t ~ N(0, diag R),  f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t, eta_t ~ N(0, Q); state
// z_t = (f_t, .., f_{t-p+1}) of width k = r p, companion matrix M (top r rows [A_1 .. A_p], shifts below).  The collapse
// (collapse.hip) has reduced row t to  b_t = sum lam_i x_ti / R_i,  C_t = sum lam_i lam_i' / R_i,  s_t = sum x_ti^2 / R_i,
// n_t and ld_t = sum log R_i over its observed cells.  filter_kernel runs the forward recursion in covariance form:
//   predict   z_p = M z,  P_p = M P M' + Qc          (only the top r rows are products; the rest are shifts)
//   update    S = P_p[:, :r], P11 = S[:r] = U U' (zero columns for zero pivots), W = I + U' C_t U (SPD, eigenvalues >= 1),
//             G^-1 = I - C_t U W^-1 U',  a = b_t - C_t f_p
//             z = z_p + S G^-1 a,   P = P_p - S (G^-1 C_t) S'
//             loglik_t = -1/2 [n_t log 2 pi + ld_t + log det W + s_t - 2 b_t' f_p + f_p' C_t f_p - a' P11 G^-1 a]
// Nothing but W is factorised: Q, P_p and C_t may be singular.  filter_fill_kernel streams the prediction errors of every cell,
// filter_eval_kernel the h-step forecast errors of every origin and their means over origins.
#include "dfm_cell.h"
#include "dfm_filter.h"
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

// ---- the recursion: one wave per replicate, every matrix in LDS ---------------------------------------------------------------
// LDS (doubles): A r k | Q r r | P k k | Pp k k | X r k (A P, then C U, then S G^-1 C) | U r r | Y r (r+1) ([a | C_t]) |
// W r (r+1) (W, then W^-1 U' Y) | Lw r (r+1) (root of W, then G^-1 Y) | z k | zp k | bv r | tv r
__host__ __device__ inline size_t filter_lds_doubles(int r, int k) {
    return (size_t)2 * r * k + (size_t)2 * r * r + (size_t)2 * k * k + (size_t)3 * r * (r + 1) + (size_t)2 * k + (size_t)2 * r;
}
size_t filter_lds_bytes(int r, int k) { return filter_lds_doubles(r, k) * sizeof(double); }

__global__ __launch_bounds__(64) void filter_kernel(FtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, k = a.r * a.p, T = a.T, N = a.N, Rp = a.Rp, tid = threadIdx.x, r1 = r + 1;
    const int kk = k * (k + 1) / 2, npR = Rp * (Rp + 1) / 2;
    const size_t b = blockIdx.x;
    double* sA = sm;
    double* sQ = sA + r * k;
    double* sP = sQ + r * r;
    double* sPp = sP + k * k;
    double* sX = sPp + k * k;
    double* sU = sX + r * k;
    double* sY = sU + r * r;
    double* sW = sY + r * r1;
    double* sL = sW + r * r1;
    double* sz = sL + r * r1;
    double* szp = sz + k;
    double* sbv = szp + k;
    double* stv = sbv + r;
    for (int e = tid; e < r * k; e += 64) sA[e] = a.A[b * r * k + e];
    for (int e = tid; e < r * r; e += 64) sQ[e] = a.Q[b * r * r + e];
    for (int e = tid; e < k * k; e += 64) {       // (lower triangle read, as the packed outputs are)
        const int i = e / k, j = e % k;
        sP[e] = i >= j ? a.P0[b * k * k + e] : a.P0[b * k * k + j * k + i];
    }
    for (int e = tid; e < k; e += 64) sz[e] = a.mu0[b * k + e];
    __syncthreads();
    const double nan = __builtin_nan("");
    bool dead = false;
    for (int t = 0; t < T; ++t) {
        const size_t bt = b * T + t;
        double ll = 0.0;
        if (!dead) {
            // ---- predict
            for (int e = tid; e < k; e += 64) {
                double v;
                if (e < r) {
                    v = 0.0;
                    for (int l = 0; l < k; ++l) v = fma(sA[e * k + l], sz[l], v);
                } else {
                    v = sz[e - r];
                }
                szp[e] = v;
            }
            for (int e = tid; e < r * k; e += 64) {
                const int i = e / k, j = e % k;
                double v = 0.0;
                for (int l = 0; l < k; ++l) v = fma(sA[i * k + l], sP[l * k + j], v);
                sX[e] = v;
            }
            __syncthreads();
            for (int e = tid; e < k * k; e += 64) {
                const int i = e / k, j = e % k;
                if (j > i) continue;
                double v;
                if (i < r) {                      // (then j < r)
                    double vij = sQ[i * r + j], vji = sQ[j * r + i];
                    for (int l = 0; l < k; ++l) {
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
            const int n = a.nobs[bt];
            if (n > 0) {
                const bool part = n < N;
                for (int e = tid; e < r * r; e += 64) {
                    const int i = e / r, j = e % r, hi = i > j ? i : j, lo = i > j ? j : i;
                    sY[i * r1 + 1 + j] = part ? a.Ct[bt * npR + hi * (hi + 1) / 2 + lo] : a.Cfull[b * Rp * Rp + hi * Rp + lo];
                }
                for (int e = tid; e < r; e += 64) sbv[e] = a.bcol[bt * Rp + e];
                int bad = filter_root(sPp, k, r, sU, kPsdTol);      // (its barriers also publish Y and bv)
                for (int e = tid; e < r; e += 64) {
                    double v = sbv[e];
                    for (int j = 0; j < r; ++j) v = fma(-sY[e * r1 + 1 + j], szp[j], v);
                    sY[e * r1] = v;                                 // a = b_t - C_t f_p
                }
                for (int e = tid; e < r * r; e += 64) {             // C U
                    const int i = e / r, j = e % r;
                    double v = 0.0;
                    for (int l = j; l < r; ++l) v = fma(sY[i * r1 + 1 + l], sU[l * r + j], v);
                    sX[e] = v;
                }
                __syncthreads();
                for (int e = tid; e < r * r; e += 64) {             // W = I + U' C U (lower triangle, mirrored)
                    const int i = e / r, j = e % r;
                    if (j > i) continue;
                    double v = i == j ? 1.0 : 0.0;
                    for (int l = i; l < r; ++l) v = fma(sU[l * r + i], sX[l * r + j], v);
                    sW[i * r + j] = v;
                    sW[j * r + i] = v;
                }
                __syncthreads();
                bad |= filter_root(sW, r, r, sL, 0.0);
                // the r + 1 columns of Y = [a | C]: Y2 = W^-1 U' Y, a lane per column
                for (int e = tid; e < r * r1; e += 64) {
                    const int i = e / r1, c = e % r1;
                    double v = 0.0;
                    for (int l = i; l < r; ++l) v = fma(sU[l * r + i], sY[l * r1 + c], v);
                    sW[i * r1 + c] = v;
                }
                __syncthreads();
                if (tid < r1) {
                    const int c = tid;
                    for (int i = 0; i < r; ++i) {
                        double v = sW[i * r1 + c];
                        for (int m = 0; m < i; ++m) v = fma(-sL[i * r + m], sW[m * r1 + c], v);
                        sW[i * r1 + c] = v / sL[i * r + i];
                    }
                    for (int i = r - 1; i >= 0; --i) {
                        double v = sW[i * r1 + c];
                        for (int m = i + 1; m < r; ++m) v = fma(-sL[m * r + i], sW[m * r1 + c], v);
                        sW[i * r1 + c] = v / sL[i * r + i];
                    }
                }
                if (tid < r) stv[tid] = 2.0 * log(sL[tid * r + tid]);   // log det W, term by term
                __syncthreads();
                // G^-1 Y = Y - (C U) Y2 into the root's place: column 0 = G^-1 a, columns 1 .. r = G^-1 C
                for (int e = tid; e < r * r1; e += 64) {
                    const int i = e / r1, c = e % r1;
                    double v = sY[e];
                    for (int l = 0; l < r; ++l) v = fma(-sX[i * r + l], sW[l * r1 + c], v);
                    sL[e] = v;
                }
                __syncthreads();
                // log-likelihood terms of row i, and z = z_p + S G^-1 a
                if (tid < r) {
                    const int i = tid;
                    double cf = 0.0, pg = 0.0;
                    for (int j = 0; j < r; ++j) {
                        cf = fma(sY[i * r1 + 1 + j], szp[j], cf);
                        pg = fma(sPp[i * k + j], sL[j * r1], pg);
                    }
                    stv[i] += szp[i] * (cf - 2.0 * sbv[i]) - sY[i * r1] * pg;
                }
                for (int e = tid; e < k; e += 64) {
                    double v = szp[e];
                    for (int j = 0; j < r; ++j) v = fma(sPp[e * k + j], sL[j * r1], v);
                    sz[e] = v;
                }
                __syncthreads();
                // S (G^-1 C) with G^-1 C symmetrised, then P = P_p - (S G^-1 C) S' on the lower triangle, mirrored
                for (int e = tid; e < k * r; e += 64) {
                    const int i = e / r, j = e % r;
                    double v = 0.0;
                    for (int l = 0; l < r; ++l) v = fma(sPp[i * k + l], 0.5 * (sL[l * r1 + 1 + j] + sL[j * r1 + 1 + l]), v);
                    sX[e] = v;
                }
                double q = 0.0;
                for (int i = 0; i < r; ++i) q += stv[i];
                ll = -0.5 * ((double)n * kLog2Pi + (part ? a.ldrow[bt] : a.ldfull[b]) + a.scol[bt] + q);
                __syncthreads();
                for (int e = tid; e < k * k; e += 64) {
                    const int i = e / k, j = e % k;
                    if (j > i) continue;
                    double v = sPp[i * k + j];
                    for (int l = 0; l < r; ++l) v = fma(-sX[i * r + l], sPp[j * k + l], v);
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

hipError_t launch_filter(const FtArgs& a, hipStream_t s) {
    const size_t lds = filter_lds_bytes(a.r, a.r * a.p);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static LdsOptIn attr_done;
    if (!attr_done && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&filter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)a.B), dim3(64), lds, s, a);
    return hipGetLastError();
}

// ---- the panel-sized outputs ------------------------------------------------------------------------------------------------------
// As forecast_fill_kernel: a workgroup owns a replicate, a chunk of rows and a block of series; the chunk's f_{t|t-1} (the first r
// entries of the z_pred row) and packed P11 (the first r (r + 1) / 2 entries of the packed P_pred row) are staged in LDS and read as
// broadcasts; lam_i (zero beyond r in its register bucket RB), R_i, mean_i, sd_i sit in registers; 16 bytes per lane when N is even.
template <int RB, int SP>
__global__ __launch_bounds__(kFtFillMaxThreads) void filter_fill_kernel(FtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, k = a.r * a.p, T = a.T, tid = threadIdx.x, np = r * (r + 1) / 2, kk = k * (k + 1) / 2;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.x, T);
    const size_t b = ch.outer;
    const int t0 = ch.t0, t1 = ch.t1;
    double* sf = sm;
    double* sP = sm + (size_t)a.geo.RC * r;
    const bool wantStd = a.vstd != nullptr, needX = a.verr != nullptr || wantStd;
    cell_stage(sf, a.z_pred + (b * T + t0) * k, t1 - t0, r, k);
    if (wantStd) cell_stage(sP, a.P_pred + (b * T + t0) * kk, t1 - t0, np, kk);
    __syncthreads();
    const CellLane ln = cell_lane<SP>(a.geo, tid, ch.s, a.N);
    if (!ln.live) return;
    const int i0 = ln.i0;
    const bool scale = a.mean != nullptr;
    CellLam<SP, RB> lam;
    lam.load(a.Lam, b, a.N, i0, r);
    double Rv[SP], mu[SP], sd[SP];
#pragma unroll
    for (int q = 0; q < SP; ++q) {
        const size_t bi = b * a.N + i0 + q;
        Rv[q] = wantStd ? a.R[bi] : 0.0;
        mu[q] = scale ? a.mean[bi] : 0.0;
        sd[q] = scale ? a.sd[bi] : 1.0;
    }
    for (int t = t0 + ln.g; t < t1; t += a.geo.G) {
        const double* f = sf + (size_t)(t - t0) * r;
        const double* P = sP + (size_t)(t - t0) * np;
        const size_t o = (b * T + t) * a.N + i0;
        double x[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) x[q] = 0.0;
        if (needX) cell_ld<SP>(a.panel + o, x);
        double xp[SP], ve[SP], vs[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) {
            const double m = lam.dot(q, f, r);
            double qf = 0.0;
            if (wantStd) {
                DFM_CELL_QUAD(qf, lam.l[q], P, RB, r)
            }
            const double e = x[q] - m;                      // NaN on a missing cell
            xp[q] = scale ? mu[q] + sd[q] * m : m;
            ve[q] = scale ? sd[q] * e : e;
            vs[q] = e / sqrt(qf + Rv[q]);
        }
        if (a.xpred) cell_st<SP>(a.xpred + o, xp);
        if (a.verr) cell_st<SP>(a.verr + o, ve);
        if (wantStd) cell_st<SP>(a.vstd + o, vs);
    }
}

// A lane per SP series; a staged row is f_{t|t-1} and the packed P11 (cell_geometry, dfm_cellgeom.h).
hipError_t launch_filter_fill(FtArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32) return hipErrorInvalidValue;
    if (!a.xpred && !a.verr && !a.vstd) return hipSuccess;
    return dispatch_r_bucket(a.r, [&](auto RBc) -> hipError_t {
        constexpr int RB = decltype(RBc)::value;
        const int r = a.r;
        const int SP = cell_sp(a.N, RB, a.panel, a.xpred, a.verr, a.vstd);
        a.geo = cell_geometry((a.N + SP - 1) / SP, r + r * (r + 1) / 2, a.T, kFtFillMaxThreads, kFtFillLds);
        const size_t lds = (size_t)a.geo.RC * (r + r * (r + 1) / 2) * sizeof(double);
        return cell_launch_sp<RB>(filter_fill_kernel<RB, 1>, filter_fill_kernel<RB, cell_sp_max(RB)>, SP,
                                  (size_t)a.B * a.geo.nchunk * a.geo.nsblk, a.geo.threads, lds, s, a);
    });
}

// ---- the out-of-sample record --------------------------------------------------------------------------------------------------------
// A workgroup owns a replicate and a block of at most 256 series (a lane each, lam_i in registers) and walks the origins t0 .. T-2
// in chunks of kFtEvalChunk: the chunk's z_{t|t} are staged in LDS and advanced by one companion step per horizon (all threads, an
// (origin, component) pair each; two buffers), and after each step every lane adds its series' squared errors against row t + h
// over the chunk's origins, in the order of the origins, to the running sums of (h, i) -- its own cells of acc / acc0 / acn, which
// no other thread touches.  No atomics, one order of summation: bit-identical results.  The panel rows of a chunk (and the H rows
// behind it) are read once from HBM and H - 1 times from cache.
template <int RB>
__global__ __launch_bounds__(256) void filter_eval_kernel(FtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, k = a.r * a.p, T = a.T, N = a.N, H = a.H, tid = threadIdx.x;
    const int nsblk = (N + 255) / 256;
    const int s = blockIdx.x % nsblk;
    const size_t b = blockIdx.x / nsblk;
    double* sA = sm;                               // [r][k]
    double* buf0 = sA + r * k;                     // [kFtEvalChunk][k]
    double* buf1 = buf0 + kFtEvalChunk * k;
    for (int e = tid; e < r * k; e += blockDim.x) sA[e] = a.A[b * r * k + e];
    const int i = s * 256 + tid;
    const bool own = i < N;
    CellLam<1, RB> lam;
    lam.load(a.Lam, b, N, i, r, own ? 1 : 0);
    const int last = T - 2;                        // the last origin that has a row behind it
    bool first = true;
    for (int c0 = a.t0; c0 <= last; c0 += kFtEvalChunk) {
        const int no = (last - c0 + 1) < kFtEvalChunk ? (last - c0 + 1) : kFtEvalChunk;
        __syncthreads();
        for (int e = tid; e < no * k; e += blockDim.x) buf0[e] = a.z_filt[(b * T + c0) * k + e];
        double* cur = buf0;
        double* nxt = buf1;
        for (int h = 1; h <= H; ++h) {
            __syncthreads();
            for (int e = tid; e < no * k; e += blockDim.x) {
                const int o = e / k, m = e % k;
                double v;
                if (m < r) {
                    v = 0.0;
                    for (int l = 0; l < k; ++l) v = fma(sA[m * k + l], cur[o * k + l], v);
                } else {
                    v = cur[o * k + m - r];
                }
                nxt[e] = v;
            }
            __syncthreads();
            if (own) {
                const size_t ai = (b * H + (h - 1)) * N + i;
                double s1 = first ? 0.0 : a.acc[ai], s0 = first ? 0.0 : a.acc0[ai];
                int n = first ? 0 : a.acn[ai];
                for (int o = 0; o < no; ++o) {
                    const int th = c0 + o + h;
                    if (th >= T) break;
                    const double x = a.panel[(b * T + th) * N + i];
                    if (x == x) {
                        const double e = x - lam.dot(0, nxt + o * k, r);
                        s1 += e * e;
                        s0 += x * x;
                        ++n;
                    }
                }
                a.acc[ai] = s1; a.acc0[ai] = s0; a.acn[ai] = n;
            }
            double* sw = cur; cur = nxt; nxt = sw;
        }
        first = false;
    }
    if (!own) return;
    const double sc = a.sd ? a.sd[b * N + i] * a.sd[b * N + i] : 1.0;
    for (int h = 0; h < H; ++h) {
        const size_t ai = (b * H + h) * N + i;
        const int n = first ? 0 : a.acn[ai];
        const double nan = __builtin_nan("");
        if (a.msfe) a.msfe[ai] = n > 0 ? sc * a.acc[ai] / n : nan;
        if (a.msfe0) a.msfe0[ai] = n > 0 ? sc * a.acc0[ai] / n : nan;
        if (a.cnt) a.cnt[ai] = n;
    }
}

hipError_t launch_filter_eval(const FtArgs& a, hipStream_t s) {
    if (a.H < 1 || (!a.msfe && !a.msfe0 && !a.cnt)) return hipSuccess;
    const int k = a.r * a.p;
    const size_t lds = ((size_t)a.r * k + (size_t)2 * kFtEvalChunk * k) * sizeof(double);
    const size_t blocks = (size_t)a.B * ((a.N + 255) / 256);
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    return dispatch_r_bucket(a.r, [&](auto RBc) -> hipError_t {
        hipLaunchKernelGGL((filter_eval_kernel<decltype(RBc)::value>), dim3((unsigned)blocks), dim3(256), lds, s, a);
        return hipGetLastError();
    });
}

}  // namespace dfm
