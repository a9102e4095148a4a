// filter.hip -- filtered states, one-step prediction errors and the pseudo-out-of-sample record of a fitted parametric DFM
// (dfm_filter_batch, capi.hip).
//
// Model  x_t = Lam f_t + e_t, e_t ~ N(0, diag R),  f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t, eta_t ~ N(0, Q); state
// z_t = (f_t, .., f_{t-p+1}) of width k = r p, companion matrix M (top r rows [A_1 .. A_p], shifts below).  The collapse
// (collapse.hip) has reduced row t to  b_t = sum lam_i x_ti / R_i,  C_t = sum lam_i lam_i' / R_i,  s_t = sum x_ti^2 / R_i,
// n_t and ld_t = sum log R_i over its observed cells.  filter_kernel runs the forward recursion in covariance form, the text of
// dfm_filter.h (filter_recursion) with its three widths folded into one: the observation loads on f_t, the first w = r entries of
// the state, and A has no zero columns (ka = k).  filter_fill_kernel streams the prediction errors of every cell,
// filter_eval_kernel the h-step forecast errors of every origin and their means over origins.
#include "dfm_cell.h"
#include "dfm_filter.h"
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

// ---- the recursion: filter_recursion (dfm_filter.h) at k = ka = r p, w = r ----------------------------------------------------
size_t filter_lds_bytes(int r, int k) { return filter_ar_lds_doubles(r, k, r) * sizeof(double); }

__global__ __launch_bounds__(64) void filter_kernel(FtRec a) { filter_recursion<false>(a); }

hipError_t launch_filter(const FtRec& a, hipStream_t s) {
    if (a.k != a.r * a.p || a.w != a.r) return hipErrorInvalidValue;       // (the widths filter_recursion<false> takes as given)
    static LdsOptIn attr_done;
    return launch_filter_recursion(filter_kernel, attr_done, a, s);
}

// ---- the panel-sized outputs ------------------------------------------------------------------------------------------------------
// As forecast_fill_kernel: a workgroup owns a replicate, a chunk of rows and a block of series; the chunk's f_{t|t-1} (the first r
// entries of the z_pred row) and packed P11 (the first r (r + 1) / 2 entries of the packed P_pred row) are staged in LDS and read as
// broadcasts; lam_i (zero beyond r in its register bucket RB), R_i, mean_i, sd_i sit in registers; 16 bytes per lane when N is even.
template <int RB, int SP>
__global__ __launch_bounds__(kFtFillMaxThreads) void filter_fill_kernel(FtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, k = a.r * a.p, T = a.n, tid = threadIdx.x, np = r * (r + 1) / 2, kk = k * (k + 1) / 2;
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
        a.geo = cell_geometry((a.N + SP - 1) / SP, r + r * (r + 1) / 2, a.n, kFtFillMaxThreads, kFtFillLds);
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
    const int r = a.r, k = a.r * a.p, T = a.n, N = a.N, H = a.H, tid = threadIdx.x;
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
            filter_eval_step(sA, k, cur, nxt, no, r, k);
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
