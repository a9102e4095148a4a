// filter_ar.hip -- filtered states, one-step prediction errors and the pseudo-out-of-sample record of the model with AR(q)
// idiosyncratic terms (dfm_filter_ar_batch, capi.hip): what filter.hip is to the plain parametric fit.
//
// Model  x_it = lam_i' f_t + e_it,  e_it = sum_{l<=q} rho_il e_i,t-l + eps_it, eps_it ~ N(0, sig2_i),  f_t a VAR(p); state
// z_t = (f_t, .., f_{t-m+1}), m = max(p, q + 1), of width k = r m.  The quasi-differenced rows y_t = x_t - sum_l rho_l x_{t-l}
// = LamK z_t + eps_t (panel rows t = q .. T-1) load on the first w = r (q + 1) entries of the state: lamK_i = [lam_i, -rho_i1 lam_i,
// .., -rho_iq lam_i].  The collapse (collapse.hip, on the quasi-differenced panel with LamK) has reduced row t to b_t, C_t (nonzero
// in their leading w, w x w), s_t, n_t and ld_t.  filter_ar_kernel runs the forward recursion in covariance form, the text of
// dfm_filter.h (filter_recursion) with its three widths apart: the state k, the nonzero columns r p of A, and w.
// filter_ar_fill_kernel streams the prediction errors of every cell, filter_ar_eval_kernel the h-step forecast errors of every
// origin, with and without the idiosyncratic term, and their means.
#include "dfm_cell.h"
#include "dfm_filter.h"
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

// ---- the recursion: filter_recursion (dfm_filter.h) at the arguments' own k and w -----------------------------------------------
size_t filter_ar_lds_bytes(int r, int k, int w) { return filter_ar_lds_doubles(r, k, w) * sizeof(double); }

__global__ __launch_bounds__(64) void filter_ar_kernel(FtRec a) { filter_recursion<true>(a); }

hipError_t launch_filter_ar(const FtRec& a, hipStream_t s) {
    if (a.r < 1 || a.w < a.r || a.k < a.w || a.k > 32 || a.r * a.p > a.k || a.Rp < a.k) return hipErrorInvalidValue;
    static LdsOptIn attr_done;
    return launch_filter_recursion(filter_ar_kernel, attr_done, a, s);
}

// ---- the panel-sized outputs ------------------------------------------------------------------------------------------------------
// As filter_fill_kernel over the n = T - q output rows: a workgroup owns a replicate, a chunk of rows and a block of series; the
// chunk's z_{t|t-1}[:w] and the packed leading w x w block of P_{t|t-1} (the first w (w + 1) / 2 entries of the packed row) are
// staged in LDS and read as broadcasts; lamK_i (formed from lam_i and rho_i, zero beyond w in its register bucket WB), rho_i,
// sig2_i, mean_i, sd_i sit in registers; the row's cells and those of its q lags are read from the panel itself; 16 bytes per lane
// when N is even.
template <int WB, int SP>
__global__ __launch_bounds__(kFtArFillMaxThreads) void filter_ar_fill_kernel(FtArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, q = a.q, k = a.k, w = a.w, n = a.n, T = a.n + a.q, tid = threadIdx.x, np = w * (w + 1) / 2, kk = k * (k + 1) / 2;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.x, n);
    const size_t b = ch.outer;
    const int t0 = ch.t0, t1 = ch.t1;
    double* sf = sm;
    double* sP = sm + (size_t)a.geo.RC * w;
    const bool wantStd = a.vstd != nullptr, needX = a.verr != nullptr || wantStd;
    cell_stage(sf, a.z_pred + (b * n + t0) * k, t1 - t0, w, k);
    if (wantStd) cell_stage(sP, a.P_pred + (b * n + t0) * kk, t1 - t0, np, kk);
    __syncthreads();
    const CellLane ln = cell_lane<SP>(a.geo, tid, ch.s, a.N);
    if (!ln.live) return;
    const int i0 = ln.i0;
    const bool scale = a.mean != nullptr;
    CellLam<SP, WB> lam;
    double rh[SP][4], Rv[SP], mu[SP], sd[SP];
#pragma unroll
    for (int s = 0; s < SP; ++s) {
        const size_t bi = b * a.N + i0 + s;
#pragma unroll
        for (int l = 0; l < 4; ++l) rh[s][l] = l < q ? a.rho[bi * q + l] : 0.0;
#pragma unroll
        for (int m = 0; m < WB; ++m) {
            double v = 0.0;
            if (m < w) {
                const int l = m / r;
                const double c = l == 0 ? 1.0 : l == 1 ? -rh[s][0] : l == 2 ? -rh[s][1] : l == 3 ? -rh[s][2] : -rh[s][3];
                v = c * a.Lam[bi * r + (m - l * r)];
            }
            lam.l[s][m] = v;
        }
        Rv[s] = wantStd ? a.sig2[bi] : 0.0;
        mu[s] = scale ? a.mean[bi] : 0.0;
        sd[s] = scale ? a.sd[bi] : 1.0;
    }
    for (int t = t0 + ln.g; t < t1; t += a.geo.G) {
        const double* f = sf + (size_t)(t - t0) * w;
        const double* P = sP + (size_t)(t - t0) * np;
        const size_t o = (b * n + t) * a.N + i0;
        const size_t xo = (b * T + t + q) * a.N + i0;       // panel row t + q
        double x[SP], ls[SP];
#pragma unroll
        for (int s = 0; s < SP; ++s) { x[s] = 0.0; ls[s] = 0.0; }
        if (needX) cell_ld<SP>(a.panel + xo, x);
#pragma unroll
        for (int l = 1; l <= 4; ++l)
            if (l <= q) {
                double xl[SP];
                cell_ld<SP>(a.panel + xo - (size_t)l * a.N, xl);
#pragma unroll
                for (int s = 0; s < SP; ++s) ls[s] = fma(rh[s][l - 1], xl[s], ls[s]);
            }
        double xp[SP], ve[SP], vs[SP];
#pragma unroll
        for (int s = 0; s < SP; ++s) {
            const double m = lam.dot(s, f, w);
            double qf = 0.0;
            if (wantStd) {
                DFM_CELL_QUAD(qf, lam.l[s], P, WB, w)
            }
            const double e = (x[s] - ls[s]) - m;            // NaN when the cell or one of its lags is missing
            const double p1 = m + ls[s];                    // NaN when a lag is missing
            xp[s] = scale ? mu[s] + sd[s] * p1 : p1;
            ve[s] = scale ? sd[s] * e : e;
            vs[s] = e / sqrt(qf + Rv[s]);
        }
        if (a.xpred) cell_st<SP>(a.xpred + o, xp);
        if (a.verr) cell_st<SP>(a.verr + o, ve);
        if (wantStd) cell_st<SP>(a.vstd + o, vs);
    }
}

// A lane per SP series; a staged row is z_pred[:w] and the packed leading block of P_pred (filter_ar_fill_geometry, dfm_cellgeom.h).
hipError_t launch_filter_ar_fill(FtArArgs a, hipStream_t s) {
    if (a.w < 1 || a.w > 32 || a.q < 1 || a.q > 4) return hipErrorInvalidValue;
    if (!a.xpred && !a.verr && !a.vstd) return hipSuccess;
    return dispatch_r_bucket(a.w, [&](auto WBc) -> hipError_t {
        constexpr int WB = decltype(WBc)::value;
        const int SP = cell_sp(a.N, WB, a.panel, a.xpred, a.verr, a.vstd);
        a.geo = filter_ar_fill_geometry(a.N, SP, a.w, a.n);
        const size_t lds = (size_t)a.geo.RC * filter_ar_row_doubles(a.w) * sizeof(double);
        return cell_launch_sp<WB>(filter_ar_fill_kernel<WB, 1>, filter_ar_fill_kernel<WB, cell_sp_max(WB)>, SP,
                                  (size_t)a.B * a.geo.nchunk * a.geo.nsblk, a.geo.threads, lds, s, a);
    });
}

// ---- the out-of-sample record --------------------------------------------------------------------------------------------------------
// As filter_eval_kernel: a workgroup owns a replicate and a block of at most 256 series (a lane each; lam_i, rho_i in registers) and
// walks the origins t0 .. T-2 (panel rows) in chunks of kFtEvalChunk.  The chunk's z_{t|t} are staged in LDS once and kept (org):
// block l of it is f_{t-l|t}, so e_{t-l|t} = x_{t-l,i} - lam_i' org[block l], l < q.  A copy is advanced by one companion step per
// horizon (all threads, an (origin, component) pair each; two buffers) for the common part lam_i' f_{t+h|t}.  The idiosyncratic part
// needs no state per origin: e_{t+h|t} = sum_l psi_{h,l} e_{t-l|t} with psi_h the first row of the h-th power of the q x q AR
// companion of series i, kept in four registers and advanced per horizon (psi_{h+1,j} = psi_{h,0} rho_{j+1} + psi_{h,j+1}).  An origin
// counts when the cells t .. t-q+1 and t+h of the series are observed.  After each step every lane adds its series' squared errors
// over the chunk's origins, in the order of the origins, to the running sums of (h, i) -- its own cells of acc / accc / acc0 / acn,
// which no other thread touches.  No atomics, one order of summation: bit-identical results.
template <int RB>
__global__ __launch_bounds__(256) void filter_ar_eval_kernel(FtArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int r = a.r, q = a.q, k = a.k, ka = a.r * a.p, n = a.n, T = a.n + a.q, N = a.N, H = a.H, tid = threadIdx.x;
    const int nsblk = (N + 255) / 256;
    const int s = blockIdx.x % nsblk;
    const size_t b = blockIdx.x / nsblk;
    double* sA = sm;                               // [r][ka]
    double* org = sA + r * ka;                     // [kFtEvalChunk][k]: z_{t|t}, kept
    double* buf0 = org + kFtEvalChunk * k;         // [kFtEvalChunk][k]: M^h z_{t|t}, two buffers
    double* buf1 = buf0 + kFtEvalChunk * k;
    for (int e = tid; e < r * ka; e += blockDim.x) sA[e] = a.A[b * r * ka + e];
    const int i = s * 256 + tid;
    const bool own = i < N;
    CellLam<1, RB> lam;
    lam.load(a.Lam, b, N, i, r, own ? 1 : 0);
    double rh[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) rh[l] = (own && l < q) ? a.rho[(b * N + i) * q + l] : 0.0;
    const int last = T - 2;                        // the last origin that has a row behind it
    bool first = true;
    for (int c0 = a.t0; c0 <= last; c0 += kFtEvalChunk) {
        const int no = (last - c0 + 1) < kFtEvalChunk ? (last - c0 + 1) : kFtEvalChunk;
        __syncthreads();
        for (int e = tid; e < no * k; e += blockDim.x) org[e] = a.z_filt[(b * n + (c0 - q)) * k + e];
        const double* cur = org;
        double* nxt = buf0;
        double* oth = buf1;
        double psi[4] = {1.0, 0.0, 0.0, 0.0};
        for (int h = 1; h <= H; ++h) {
            __syncthreads();
            filter_eval_step(sA, ka, cur, nxt, no, r, k);
            {
                const double p0 = psi[0];
                psi[0] = fma(p0, rh[0], psi[1]);
                psi[1] = fma(p0, rh[1], psi[2]);
                psi[2] = fma(p0, rh[2], psi[3]);
                psi[3] = p0 * rh[3];
            }
            __syncthreads();
            if (own) {
                const size_t ai = (b * H + (h - 1)) * N + i;
                double s1 = first ? 0.0 : a.acc[ai], sc = first ? 0.0 : a.accc[ai], s0 = first ? 0.0 : a.acc0[ai];
                int cn = first ? 0 : a.acn[ai];
                for (int o = 0; o < no; ++o) {
                    const int t = c0 + o, th = t + h;
                    if (th >= T) break;
                    const double x = a.panel[(b * T + th) * N + i];
                    bool ok = x == x;
                    double ei = 0.0;
#pragma unroll
                    for (int l = 0; l < 4; ++l)
                        if (l < q) {
                            const double xl = a.panel[(b * T + (t - l)) * N + i];
                            ok = ok && xl == xl;
                            ei = fma(psi[l], xl - lam.dot(0, org + o * k + l * r, r), ei);
                        }
                    if (ok) {
                        const double fc = lam.dot(0, nxt + o * k, r);
                        const double ec = x - fc, e = x - (fc + ei);
                        s1 += e * e;
                        sc += ec * ec;
                        s0 += x * x;
                        ++cn;
                    }
                }
                a.acc[ai] = s1; a.accc[ai] = sc; a.acc0[ai] = s0; a.acn[ai] = cn;
            }
            cur = nxt;
            double* sw = nxt; nxt = oth; oth = sw;
        }
        first = false;
    }
    if (!own) return;
    const double scl = a.sd ? a.sd[b * N + i] * a.sd[b * N + i] : 1.0;
    for (int h = 0; h < H; ++h) {
        const size_t ai = (b * H + h) * N + i;
        const int cn = first ? 0 : a.acn[ai];
        const double nan = __builtin_nan("");
        if (a.msfe) a.msfe[ai] = cn > 0 ? scl * a.acc[ai] / cn : nan;
        if (a.msfe_common) a.msfe_common[ai] = cn > 0 ? scl * a.accc[ai] / cn : nan;
        if (a.msfe0) a.msfe0[ai] = cn > 0 ? scl * a.acc0[ai] / cn : nan;
        if (a.cnt) a.cnt[ai] = cn;
    }
}

hipError_t launch_filter_ar_eval(const FtArArgs& a, hipStream_t s) {
    if (a.H < 1 || (!a.msfe && !a.msfe_common && !a.msfe0 && !a.cnt)) return hipSuccess;
    if (a.r > 16 || a.q < 1 || a.q > 4 || a.t0 < a.q) return hipErrorInvalidValue;    // (k = r max(p, q + 1) <= 32 and q >= 1)
    const size_t lds = ((size_t)a.r * a.r * a.p + (size_t)3 * kFtEvalChunk * a.k) * sizeof(double);
    const size_t blocks = (size_t)a.B * ((a.N + 255) / 256);
    if (blocks > 0x7fffffffu || lds > 64 * 1024) return hipErrorInvalidValue;
    auto go = [&](auto RBc) -> hipError_t {
        hipLaunchKernelGGL((filter_ar_eval_kernel<decltype(RBc)::value>), dim3((unsigned)blocks), dim3(256), lds, s, a);
        return hipGetLastError();
    };
    if (a.r <= 4) return go(std::integral_constant<int, 4>{});
    if (a.r <= 8) return go(std::integral_constant<int, 8>{});
    return go(std::integral_constant<int, 16>{});
}

}  // namespace dfm
