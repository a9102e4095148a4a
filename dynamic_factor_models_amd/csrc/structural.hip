// structural.hip -- identified impulse responses, variance and historical decompositions of the panel (dfm_irf_batch,
// dfm_histdecomp_batch, capi.hip).  Model  x_t = Lam f_t + e_t,  f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t,  Var eta = Q,
// eta_t = S u_t with Var u = I.  Identification (include/dfm_hip.h): S = Ln^-1 chol(Ln Q Ln') with Ln = Lam[named, :], or chol(Q).
//   sv_prep_kernel      one workgroup per replicate: S, S^-1, the unit-effect scales and the tables Theta_h = Psi_h S, Theta^c_h
//   sv_irf_fill_kernel  streams irf [B][r][H][N] and fevd [B][r+1][H][N]: a workgroup owns a replicate (or one of its SvArgs::slots
//                       kept rotations, signirf.hip) and a block of series, a lane
//                       one series (or two adjacent ones, 16-byte stores), walks h in order with the Theta rows staged in LDS
//                       (every lane reads the same address: a broadcast) and the r running sums of squares in registers
//   sv_shock_kernel     etahat_t = f_t - sum_j A_j f_{t-j} and u_t = S^-1 etahat_t, all t at once
//   sv_path_kernel      the r + 1 contribution chains c^(k)_t = sum_j A_j c^(k)_{t-j} + S e_k u_kt, one lane per (chain, state
//                       component): (r + 1) r p busy lanes per dependent row instead of r
//   sv_hd_fill_kernel   streams hd [B][r+1][T][N] = sd_i lam_i' c^(k)_t, a chunk of rows and a block of series per workgroup
// The tables are stored shock-major, Th[h][k][m] = (Theta_h)_mk, so that a lane's dot product reads consecutive addresses.
#include "dfm_cell.h"
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr int kSvIrfLanes = 128;              // sv_irf_fill_kernel: lanes (series, or pairs of series) per workgroup
constexpr int kSvFillMaxThreads = 512;        // sv_hd_fill_kernel
constexpr size_t kSvFillLds = 48 * 1024;      // both fill kernels: Theta rows / contribution rows staged per workgroup
constexpr int kSvPathMaxThreads = 1024;       // sv_path_kernel
constexpr size_t kSvPathLds = 48 * 1024;
constexpr int kSvShockRows = 32;              // sv_shock_kernel: rows per workgroup
constexpr double kSvPivTol = 1e-12;           // Ln: a pivot <= this x max|Ln| raises the status bit
constexpr int kSvStatusBit = 16;

// One workgroup per replicate.  LDS: A [r][r p], a ring of p + 1 Theta matrices, Ln, M = Ln Q Ln' (or Q), its root L, and X
// (Ln Q, then S^-1, then the right-hand side L of Ln S = L).
__global__ __launch_bounds__(256) void sv_prep_kernel(SvArgs a) {
    __shared__ double sA[1024], sRing[2048], sLn[1024], sM[1024], sL[1024], sX[1024], sfac[32];
    const size_t b = blockIdx.x;
    const int r = a.r, p = a.p, k = a.r * a.p, rr = a.r * a.r, tid = threadIdx.x, nth = blockDim.x;
    const bool named = a.named != nullptr;
    const double* Q = a.Q + b * rr;
    for (int e = tid; e < r * k; e += nth) sA[e] = a.A[b * r * k + e];
    for (int e = tid; e < rr; e += nth) {
        const int i = e / r, j = e % r;
        sLn[e] = named ? a.Lam[(b * a.N + a.named[i]) * r + j] : (i == j ? 1.0 : 0.0);
        sM[e] = Q[e];
    }
    __syncthreads();
    if (named) {
        for (int e = tid; e < rr; e += nth) {                        // X = Ln Q
            const int i = e / r, j = e % r;
            double v = 0.0;
            for (int m = 0; m < r; ++m) v = fma(sLn[i * r + m], Q[m * r + j], v);
            sX[e] = v;
        }
        __syncthreads();
        for (int e = tid; e < rr; e += nth) {                        // M = X Ln'
            const int i = e / r, j = e % r;
            double v = 0.0;
            for (int m = 0; m < r; ++m) v = fma(sX[i * r + m], sLn[j * r + m], v);
            sM[e] = v;
        }
        __syncthreads();
    }
    const int dropped = psd_root(sM, r, sL, kPsdTol);
    if (a.need_pd && dropped && tid == 0) atomicOr(a.status, kSvStatusBit);
    // S^-1 = L^-1 Ln by forward substitution, a column per thread (a zero pivot leaves a zero row)
    if (a.Sinv) {
        for (int c = tid; c < r; c += nth)
            for (int i = 0; i < r; ++i) {
                double v = sLn[i * r + c];
                for (int m = 0; m < i; ++m) v -= sL[i * r + m] * sX[m * r + c];
                sX[i * r + c] = sL[i * r + i] > 0.0 ? v / sL[i * r + i] : 0.0;
            }
        __syncthreads();
        for (int e = tid; e < rr; e += nth) a.Sinv[b * rr + e] = sX[e];
        __syncthreads();
    }
    // S: Ln S = L by Gauss-Jordan elimination with partial pivoting on [Ln | X = L]
    double* S = sRing;                                               // slot 0 of the ring: Theta_0
    if (named) {
        double amax = 0.0;
        for (int e = 0; e < rr; ++e) amax = fmax(amax, fabs(sLn[e]));
        for (int e = tid; e < rr; e += nth) sX[e] = sL[e];
        __syncthreads();
        for (int j = 0; j < r; ++j) {
            int piv = j;
            double best = fabs(sLn[j * r + j]);
            for (int i = j + 1; i < r; ++i)
                if (fabs(sLn[i * r + j]) > best) { best = fabs(sLn[i * r + j]); piv = i; }
            __syncthreads();
            if (!(best > kSvPivTol * amax) && tid == 0) atomicOr(a.status, kSvStatusBit);
            if (piv != j)
                for (int c = tid; c < 2 * r; c += nth) {
                    double* row = c < r ? sLn : sX;
                    const int cc = c < r ? c : c - r;
                    const double t = row[j * r + cc];
                    row[j * r + cc] = row[piv * r + cc];
                    row[piv * r + cc] = t;
                }
            __syncthreads();
            const double pv = sLn[j * r + j];
            if (tid < r) sfac[tid] = tid == j ? 0.0 : sLn[tid * r + j] / pv;
            __syncthreads();
            for (int e = tid; e < 2 * rr; e += nth) {
                double* mat = e < rr ? sLn : sX;
                const int ee = e < rr ? e : e - rr, i = ee / r, c = ee % r;
                if (i != j) mat[i * r + c] = fma(-sfac[i], mat[j * r + c], mat[i * r + c]);
            }
            __syncthreads();
        }
        for (int e = tid; e < rr; e += nth) S[e] = sX[e] / sLn[(e / r) * r + e / r];
    } else {
        for (int e = tid; e < rr; e += nth) S[e] = sL[e];
    }
    __syncthreads();
    for (int e = tid; e < rr; e += nth) a.S[b * rr + e] = S[e];
    // the impact response of series named[k] to shock k in output units: the fill kernel's own arithmetic, so that its
    // quotient is exactly 1
    if (a.scale && named && tid < r) {
        const size_t n = b * a.N + a.named[tid];
        double v = 0.0;
        for (int m = 0; m < r; ++m) v = fma(a.Lam[n * r + m], S[m * r + tid], v);
        a.scale[b * r + tid] = a.sd ? a.sd[n] * v : v;
    }
    // Theta_h = sum_{j=1..min(h,p)} A_j Theta_{h-j}; each thread owns up to four elements and their running sums
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int h = 0; h < a.H; ++h) {
        double* cur = sRing + (size_t)(h % (p + 1)) * rr;
        for (int q = 0; q < 4; ++q) {
            const int e = tid + q * nth;
            if (e >= rr) break;
            const int i = e / r, c = e % r;
            double v = cur[e];
            if (h > 0) {
                v = 0.0;
                for (int j = 1; j <= p && j <= h; ++j) {
                    const double* prev = sRing + (size_t)((h - j) % (p + 1)) * rr;
                    for (int m = 0; m < r; ++m) v = fma(sA[i * k + (j - 1) * r + m], prev[m * r + c], v);
                }
                cur[e] = v;
            }
            acc[q] += v;
            const size_t o = (b * a.H + h) * rr + (size_t)c * r + i;
            a.Th[o] = v;
            if (a.Thc) a.Thc[o] = acc[q];
        }
        __syncthreads();
    }
}

template <int R, int SP>
__global__ __launch_bounds__(kSvIrfLanes) void sv_irf_fill_kernel(SvArgs a) {
    constexpr int RR = R * R;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, H = a.H, N = a.N;
    const int s = (int)(blockIdx.x % (unsigned)a.geo.nsblk);
    const size_t sl = blockIdx.x / (unsigned)a.geo.nsblk;             // tables and outputs: the slot; parameters: its replicate
    const size_t b = a.slots > 1 ? sl / (unsigned)a.slots : sl;
    const bool hasc = a.Thc != nullptr, wantV = a.fevd != nullptr, wantI = a.irf != nullptr, unit = a.scale != nullptr;
    double* sT = sm;
    double* sTc = sm + (size_t)a.geo.RC * RR;
    double* sSc = sm + (size_t)a.geo.RC * RR * (hasc ? 2 : 1);
    const CellLane ln = cell_lane<SP>(a.geo, tid, s, N);             // (G = 1: an idle lane stays for the barriers)
    const int i0 = ln.i0;
    const bool live = ln.live;
    CellLam<SP, R> lam;
    lam.load(a.Lam, b, N, i0, R, ln.n);
    double ssq[SP][R], sdv[SP], Rv[SP];
    bool cm[SP];
#pragma unroll
    for (int q = 0; q < SP; ++q) {
        const size_t bi = b * N + (live ? i0 + q : 0);
#pragma unroll
        for (int k = 0; k < R; ++k) ssq[q][k] = 0.0;
        sdv[q] = a.sd ? a.sd[bi] : 1.0;
        Rv[q] = wantV ? a.R[bi] : 0.0;
        cm[q] = a.cum != nullptr && a.cum[live ? i0 + q : 0] != 0;
    }
    if (tid < R) sSc[tid] = unit ? a.scale[b * R + tid] : 1.0;
    for (int h0 = 0; h0 < H; h0 += a.geo.RC) {
        const int nh = H - h0 < a.geo.RC ? H - h0 : a.geo.RC;
        __syncthreads();
        cell_stage(sT, a.Th + (sl * H + h0) * RR, nh * RR);
        if (hasc) cell_stage(sTc, a.Thc + (sl * H + h0) * RR, nh * RR);
        __syncthreads();
        if (!live) continue;
        for (int hh = 0; hh < nh; ++hh) {
            const int h = h0 + hh;
            const double* Tq[SP];
            double tot[SP];
#pragma unroll
            for (int q = 0; q < SP; ++q) { Tq[q] = (cm[q] ? sTc : sT) + (size_t)hh * RR; tot[q] = 0.0; }
#pragma unroll
            for (int k = 0; k < R; ++k) {
                double x[SP];
#pragma unroll
                for (int q = 0; q < SP; ++q) {
                    const double v = lam.dot(q, Tq[q] + k * R, R);
                    ssq[q][k] = fma(v, v, ssq[q][k]);
                    tot[q] += ssq[q][k];
                    x[q] = unit ? sdv[q] * v / sSc[k] : sdv[q] * v;
                }
                if (wantI) cell_st<SP>(a.irf + ((sl * R + k) * H + h) * N + i0, x);
            }
            if (!wantV) continue;
            double idio[SP], inv[SP];
#pragma unroll
            for (int q = 0; q < SP; ++q) {
                idio[q] = cm[q] ? (double)(h + 1) * Rv[q] : Rv[q];
                inv[q] = 1.0 / (tot[q] + idio[q]);
            }
#pragma unroll
            for (int k = 0; k <= R; ++k) {
                double x[SP];
#pragma unroll
                for (int q = 0; q < SP; ++q) x[q] = (k < R ? ssq[q][k < R ? k : 0] : idio[q]) * inv[q];
                cell_st<SP>(a.fevd + ((sl * (R + 1) + k) * H + h) * N + i0, x);
            }
        }
    }
}

// etahat and u for kSvShockRows rows of one replicate: a thread per (row, component).
__global__ __launch_bounds__(256) void sv_shock_kernel(SvArgs a) {
    __shared__ double sA[1024], sSi[1024], se[kSvShockRows * 32];
    const size_t b = blockIdx.x;
    const int r = a.r, p = a.p, k = a.r * a.p, T = a.T, tid = threadIdx.x, nth = blockDim.x;
    const int t0 = blockIdx.y * kSvShockRows, nt = T - t0 < kSvShockRows ? T - t0 : kSvShockRows;
    const double* f = a.f + b * T * r;
    for (int e = tid; e < r * k; e += nth) sA[e] = a.A[b * r * k + e];
    for (int e = tid; e < r * r; e += nth) sSi[e] = a.Sinv[b * r * r + e];
    __syncthreads();
    for (int e = tid; e < nt * r; e += nth) {
        const int t = t0 + e / r, c = e % r;
        double v = 0.0;
        if (t >= p) {
            v = f[(size_t)t * r + c];
            for (int j = 1; j <= p; ++j)
                for (int m = 0; m < r; ++m) v = fma(-sA[c * k + (j - 1) * r + m], f[(size_t)(t - j) * r + m], v);
        }
        se[(e / r) * 32 + c] = v;
    }
    __syncthreads();
    for (int e = tid; e < nt * r; e += nth) {
        const int tt = e / r, c = e % r;
        double v = 0.0;
        if (t0 + tt >= p)
            for (int m = 0; m < r; ++m) v = fma(sSi[c * r + m], se[tt * 32 + m], v);
        a.u[(b * T + t0 + tt) * r + c] = v;
    }
}

// The contribution chains of one replicate, CP of them per workgroup (blockIdx.y picks the group).  Lane (chain, c) with c < r
// computes component c of the chain's new row from its companion state (f_{t-1}, .., f_{t-p}) in LDS, lanes r <= c < r p shift
// the state; two state buffers used in turn: one barrier per row.  The rows of TC periods are staged in LDS and written out
// together (a global store in front of every barrier would make the barrier wait for it), as are the TC rows of shocks.
__global__ __launch_bounds__(kSvPathMaxThreads) void sv_path_kernel(SvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, p = a.p, k = a.r * a.p, T = a.T, CP = a.CP, TC = a.TC, tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int q0 = blockIdx.y * CP, nq = r + 1 - q0 < CP ? r + 1 - q0 : CP;
    double* st = sm;                                  // [2][CP][k]
    double* sout = sm + (size_t)2 * CP * k;           // [TC][CP][r]
    double* su = sout + (size_t)TC * CP * r;          // [TC][r]
    const int ql = tid / k, c = tid % k, q = q0 + ql;
    const bool live = ql < nq;
    const bool head = live && c < r;
    double arow[32];
#pragma unroll
    for (int m = 0; m < 32; ++m) arow[m] = (head && m < k) ? a.A[(b * r + c) * k + m] : 0.0;
    const double sq = (head && q < r) ? a.S[(b * r + c) * r + q] : 0.0;
    const double* f = a.f + b * T * r;
    for (int e = tid; e < 2 * CP * k; e += blockDim.x) st[e] = 0.0;
    int cur = 0;
    for (int c0 = 0; c0 < T; c0 += TC) {
        const int nt = T - c0 < TC ? T - c0 : TC;
        for (int e = tid; e < nt * r; e += blockDim.x) su[e] = a.u[(b * T + c0) * r + e];
        __syncthreads();
        for (int tt = 0; tt < nt; ++tt) {
            const int t = c0 + tt;
            if (live) {
                const double* zin = st + ((size_t)cur * CP + ql) * k;
                double v;
                if (c < r) {
                    if (t < p) {
                        v = q == r ? f[(size_t)t * r + c] : 0.0;
                    } else {
                        v = q < r ? sq * su[tt * r + q] : 0.0;
#pragma unroll
                        for (int m = 0; m < 32; ++m)
                            if (m < k) v = fma(arow[m], zin[m], v);
                    }
                    sout[((size_t)tt * CP + ql) * r + c] = v;
                } else {
                    v = zin[c - r];
                }
                st[((size_t)(cur ^ 1) * CP + ql) * k + c] = v;
            }
            cur ^= 1;
            __syncthreads();
        }
        for (int e = tid; e < nt * nq * r; e += blockDim.x) {
            const int cc = e % r, qq = (e / r) % nq, tt = e / (r * nq);
            a.C[((b * (r + 1) + q0 + qq) * T + c0 + tt) * r + cc] = sout[((size_t)tt * CP + qq) * r + cc];
        }
    }
}

template <int R, int SP>
__global__ __launch_bounds__(kSvFillMaxThreads) void sv_hd_fill_kernel(SvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int T = a.T, N = a.N, tid = threadIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.x, T);
    const size_t bk = ch.outer, b = bk / (R + 1);                           // bk = b (r + 1) + slot
    const int t0 = ch.t0, t1 = ch.t1;
    cell_stage(sm, a.C + (bk * T + t0) * R, (t1 - t0) * R);
    __syncthreads();
    const CellLane ln = cell_lane<SP>(a.geo, tid, ch.s, N);
    if (!ln.live) return;
    const int i0 = ln.i0;
    CellLam<SP, R> lam;                                                     // sd_i lam_i
    lam.load(a.Lam, b, N, i0, R, SP, a.sd);
    for (int t = t0 + ln.g; t < t1; t += a.geo.G) {
        const double* cr = sm + (size_t)(t - t0) * R;
        double x[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) x[q] = lam.dot(q, cr, R);
        cell_st<SP>(a.hd + (bk * T + t) * N + i0, x);
    }
}

hipError_t launch_sv_prep(const SvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sv_prep_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sv_shock(const SvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sv_shock_kernel, dim3((unsigned)a.B, (unsigned)((a.T + kSvShockRows - 1) / kSvShockRows)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sv_path(SvArgs a, hipStream_t s) {
    const PathGeom g = path_geometry(a.r, a.p, kSvPathMaxThreads, kSvPathLds);
    a.CP = g.CP;
    a.TC = g.TC;
    hipLaunchKernelGGL(sv_path_kernel, dim3((unsigned)a.B, (unsigned)g.groups), dim3(g.threads), g.lds, s, a);
    return hipGetLastError();
}

template <int R>
static hipError_t launch_irf_r(SvArgs a, hipStream_t s) {
    const int SP = cell_sp(a.N, R, a.irf, a.fevd);
    const bool hasc = a.Thc != nullptr;
    a.geo = irf_geometry(a.N, R, SP, a.H, hasc, kSvIrfLanes, kSvFillLds);
    const size_t lds = ((size_t)a.geo.RC * R * R * (hasc ? 2 : 1) + 32) * sizeof(double);
    return cell_launch_sp<R>(sv_irf_fill_kernel<R, 1>, sv_irf_fill_kernel<R, cell_sp_max(R)>, SP,
                             (size_t)a.B * (a.slots > 1 ? a.slots : 1) * a.geo.nsblk, a.geo.threads, lds, s, a);
}

// A lane per SP series; a staged row is one row of a contribution path (cell_geometry, dfm_cellgeom.h).
template <int R>
static hipError_t launch_hd_r(SvArgs a, hipStream_t s) {
    const int SP = cell_sp(a.N, R, a.hd);
    a.geo = cell_geometry((a.N + SP - 1) / SP, R, a.T, kSvFillMaxThreads, kSvFillLds);
    const size_t lds = (size_t)a.geo.RC * R * sizeof(double);
    return cell_launch_sp<R>(sv_hd_fill_kernel<R, 1>, sv_hd_fill_kernel<R, cell_sp_max(R)>, SP,
                             (size_t)a.B * (R + 1) * a.geo.nchunk * a.geo.nsblk, a.geo.threads, lds, s, a);
}

hipError_t launch_sv_irf_fill(SvArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.H < 1) return hipErrorInvalidValue;
    return dispatch_r_exact(a.r, hipErrorInvalidValue, [&](auto R) { return launch_irf_r<decltype(R)::value>(a, s); });
}

hipError_t launch_sv_hd_fill(SvArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.T < 1) return hipErrorInvalidValue;
    return dispatch_r_exact(a.r, hipErrorInvalidValue, [&](auto R) { return launch_hd_r<decltype(R)::value>(a, s); });
}

}  // namespace dfm
