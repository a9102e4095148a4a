// news.hip -- news decomposition of nowcast revisions (dfm_news_batch, capi.hip; Banbura and Modugno 2014).  For replicate b and
// target g = (t*, i*) the weights w = dy_new / dx on the observed cells of the new vintage are Sigma^-1 c with
// c = Cov(z_new, y_z); in the factor model x - Lam E_0[f | x] = R Sigma^-1 x, so one smoother pass with mu0 = 0 over the
// covariance panel c gives them all.  Pass replicate j = b G + g:
//   news_revise_kernel      the revised old panel (new values on the old vintage's cells) and the vintage check      [B][T][N]
//   news_gather_kernel      the target cells of a forecast's xhat into yhat                                          [B][3][G]
//   news_gamma_kernel       a_t = S Cov(z_{t+1}, z_{t*+1}) S' lam_i* for t < T from Gamma_t = Var(z_t)               [S][T][r]
//   news_cov_panel_kernel   c_ti = lam_i' a_t (+ R_i* on the target cell) on the new vintage's cells, NaN elsewhere  [S][T][N]
//   news_impact_kernel      w, the news I and the per-series impacts sum_t w I                                       [S][N]
// The two cell kernels: one workgroup owns a pass replicate's rows (a chunk of them for the covariance panel, all of them for the
// impacts, which are summed over t in registers and then across the workgroup's row groups in LDS in a fixed order: no atomics,
// results do not depend on scheduling), stages the r-vectors of its rows in LDS, keeps the loadings of its two columns in
// registers and moves 16 bytes per lane where N is even.  blockIdx.x is the pass replicate: the G targets of a replicate run next
// to each other, so the panels they share come from L2 / the Infinity Cache.
#include "dfm_cell.h"
#include "dfm_kernels.h"

namespace dfm {

constexpr int kNwMaxThreads = 512;            // cell kernels
constexpr size_t kNwLds = 32 * 1024;          // cell kernels: r-vectors of the rows staged per workgroup
constexpr int kNwTC = 32;                     // news_gamma_kernel: rows per LDS chunk of u_t / a_t (global traffic once per chunk)
constexpr int kNwVintageBit = 8;              // status word bit: Omega_old is not a subset of Omega_new

// rev = new where old is observed, NaN elsewhere; a cell observed in old but missing in new raises the vintage bit.
__global__ __launch_bounds__(256) void news_revise_kernel(NwArgs a) {
    const size_t n = (size_t)a.B * a.T * a.N;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    bool bad = false;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const double xo = a.oldp[e], xn = a.newp[e];
        const bool oo = xo == xo;
        bad = bad || (oo && xn != xn);
        a.rev[e] = oo ? xn : qnan;
    }
    if (bad) atomicOr(a.status, kNwVintageBit);
}

__global__ __launch_bounds__(256) void news_gather_kernel(NwArgs a, const double* xhat, int which) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.B * a.G) return;
    const int b = e / a.G, g = e % a.G;
    const int ts = a.tgt[2 * g], is = a.tgt[2 * g + 1];
    a.yhat[((size_t)b * 3 + which) * a.G + g] = xhat[((size_t)b * a.TH + ts) * a.N + is];
}

// One workgroup per pass replicate of the slice; KB >= k = r p.  With u_t = (A_c')^(t* - t) S' lam (u_t* = S' lam):
//   rows t < min(t*, T):     a_t = S Gamma_{t+1} u_t           (Cov(z_{t+1}, z_{t*+1}) = Gamma_{t+1} (A_c')^(t* - t))
//   row t = t* (if < T):     v = Gamma_{t*+1} S' lam,  a_t = S v
//   rows t* < t < T:         v <- A_c v,  a_t = S v          (Cov(z_{t+1}, z_{t*+1}) = A_c^(t - t*) Gamma_{t*+1})
// Gamma_0 = P0, Gamma_t = A_c Gamma_{t-1} A_c' + Q_c (symmetric: row m of Gamma is read for its column m).  Phase U runs the u
// chain backwards from t* into u (global, staged 32 rows at a time); phase Gamma runs the recursion forwards and reads u back in
// chunks.  a_t is staged the same way: a barrier waits for every outstanding global store, so no row stores on its own.
template <int KB, int NT>
__global__ __launch_bounds__(NT) void news_gamma_kernel(NwArgs a) {
    constexpr int NE = (KB * KB + NT - 1) / NT;               // elements of Gamma per thread
    __shared__ double sA[KB * KB], sG[KB * KB], sW[KB * KB];
    __shared__ double sU[2][kNwTC * KB], sAv[2][kNwTC * KB], sv[2][KB], sl[KB];
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G), r = a.r, k = a.r * a.p, T = a.T, N = a.N;
    const int ts = a.tgt[2 * gi], is = a.tgt[2 * gi + 1];
    double qe[NE];                                            // Q_c of this thread's elements
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        const int e = tid + q * NT, i = e / k, m = e % k;
        qe[q] = 0.0;
        if (e >= k * k) continue;
        sA[i * KB + m] = i < r ? a.A[(b * r + i) * k + m] : (m == i - r ? 1.0 : 0.0);
        sG[i * KB + m] = a.P0[(b * k + i) * k + m];
        qe[q] = (i < r && m < r) ? a.Q[(b * r + i) * r + m] : 0.0;
    }
    if (tid < k) {
        const double l = tid < r ? a.Lam[(b * N + is) * r + tid] : 0.0;
        sl[tid] = l;
        sv[0][tid] = l;
    }
    __syncthreads();
    double* U = a.u + (size_t)s * T * k;
    double* AV = a.av + (size_t)s * T * r;
    // phase U: u_t for t = t* - 1 .. 0 (stored for t < T), the chunk of rows [t, t + 32) flushed when t reaches its first row
    int cur = 0;
    for (int t = ts - 1; t >= 0; --t) {
        const int pb = (t / kNwTC) & 1;
        if (tid < k) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sA[m * KB + tid], sv[cur][m], v);
            sv[cur ^ 1][tid] = v;
            if (t < T) sU[pb][(t % kNwTC) * KB + tid] = v;
        }
        cur ^= 1;
        __syncthreads();
        if (t < T && t % kNwTC == 0) {
            const int nr = (t + kNwTC < T ? t + kNwTC : T) - t;
            for (int e = tid; e < nr * k; e += NT) U[(size_t)t * k + e] = sU[pb][(e / k) * KB + e % k];
        }
    }
    __syncthreads();                                          // (u is read back below by other threads)
    const int tend = ts < T ? ts : T - 1;                     // the recursion runs to Gamma_{tend + 1}
    auto flush_av = [&](int t) {                              // after a barrier: rows of t's chunk up to t
        const int pb = (t / kNwTC) & 1, c0 = t - t % kNwTC;
        for (int e = tid; e < (t - c0 + 1) * r; e += NT) AV[(size_t)c0 * r + e] = sAv[pb][(e / r) * KB + e % r];
    };
    for (int t = 0; t <= tend; ++t) {
        const int pb = (t / kNwTC) & 1;
        if (t < ts && t % kNwTC == 0) {                       // u rows of this chunk (read two barriers later)
            const int t1 = t + kNwTC < ts ? (t + kNwTC < T ? t + kNwTC : T) : (ts < T ? ts : T);
            for (int e = tid; e < (t1 - t) * k; e += NT) sU[pb][(e / k) * KB + e % k] = U[(size_t)t * k + e];
        }
#pragma unroll
        for (int q = 0; q < NE; ++q) {                        // W = A_c Gamma
            const int e = tid + q * NT, i = e / k, c = e % k;
            if (e >= k * k) continue;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sA[i * KB + m], sG[c * KB + m], v);
            sW[i * KB + c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NE; ++q) {                        // Gamma = W A_c' + Q_c
            const int e = tid + q * NT, i = e / k, c = e % k;
            if (e >= k * k) continue;
            double v = qe[q];
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sW[i * KB + m], sA[c * KB + m], v);
            sG[i * KB + c] = v;
        }
        __syncthreads();
        if (t < ts) {
            if (tid < r) {
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < KB; ++m)
                    if (m < k) v = fma(sG[tid * KB + m], sU[pb][(t % kNwTC) * KB + m], v);
                sAv[pb][(t % kNwTC) * KB + tid] = v;
            }
        } else if (tid < k) {                                 // t = t* < T
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < r) v = fma(sG[tid * KB + m], sl[m], v);
            sv[0][tid] = v;
            if (tid < r) sAv[pb][(t % kNwTC) * KB + tid] = v;
        }
        if (t % kNwTC == kNwTC - 1 || t == T - 1) {
            __syncthreads();
            flush_av(t);
        }
    }
    // rows t* < t < T: v <- A_c v
    cur = 0;
    __syncthreads();
    for (int t = tend + 1; t < T; ++t) {
        const int pb = (t / kNwTC) & 1;
        if (tid < k) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sA[tid * KB + m], sv[cur][m], v);
            sv[cur ^ 1][tid] = v;
            if (tid < r) sAv[pb][(t % kNwTC) * KB + tid] = v;
        }
        cur ^= 1;
        __syncthreads();
        if (t % kNwTC == kNwTC - 1 || t == T - 1) flush_av(t);
    }
}

// The covariance panels: chunk blockIdx.y of the rows of pass replicate blockIdx.x, column pairs of block blockIdx.z.
template <int RB, bool VEC>
__global__ __launch_bounds__(kNwMaxThreads) void news_cov_panel_kernel(NwArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sav[];
    const int r = a.r, N = a.N, T = a.T, tid = threadIdx.x;
    const int s = blockIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.z, blockIdx.y, s, T);
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G);
    const int t0 = ch.t0, t1 = ch.t1;
    cell_stage(sav, a.av + ((size_t)s * T + t0) * r, (t1 - t0) * r);
    __syncthreads();
    const CellLane ln = cell_lane<2>(a.geo, tid, ch.s, N);
    if (!ln.live) return;
    const int i0 = ln.i0, gr = ln.g;
    const bool two = ln.n == 2;
    CellLam<2, RB> lam;
    lam.load(a.Lam, b, N, i0, r, ln.n);
    const int ts = a.tgt[2 * gi], is = a.tgt[2 * gi + 1];
    const double radd = a.R[b * N + is];
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double* px = a.newp + b * T * N + i0;
    double nx[2];                                             // the next row's cells, in flight while this row is computed
    cell_prefetch_pair<VEC>(px + (size_t)(t0 + gr) * N, t0 + gr < t1, two, nx);
    for (int t = t0 + gr; t < t1; t += a.geo.G) {
        const double* av = sav + (size_t)(t - t0) * r;
        const double x0 = nx[0], x1 = nx[1];
        cell_prefetch_pair<VEC>(px + (size_t)(t + a.geo.G) * N, t + a.geo.G < t1, two, nx);
        double m[2];
        lam.dots(av, r, m);
        double m0 = m[0], m1 = m[1];
        if (t == ts) {
            if (i0 == is) m0 += radd;
            if (i0 + 1 == is) m1 += radd;
        }
        const double y[2] = {x0 == x0 ? m0 : qnan, x1 == x1 ? m1 : qnan};
        cell_st_pair<VEC>(a.cp + ((size_t)s * T + t) * N + i0, two, y);
    }
}

// w, I and the impacts of pass replicate blockIdx.x over all T rows, column pairs of block blockIdx.y.  The covariance panel may
// be the slice's part of weight: each cell is read before the same lane writes w there.
template <int RB, bool VEC>
__global__ __launch_bounds__(kNwMaxThreads) void news_impact_kernel(NwArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sgr[];
    double* sred = sgr + (size_t)a.geo.RC * a.r;             // [G][NPB][2] per-row-group sums
    const int r = a.r, N = a.N, T = a.T, tid = threadIdx.x;
    const int s = blockIdx.x, sb = blockIdx.y;
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G);
    const CellLane ln = cell_lane<2>(a.geo, tid, sb, N);     // (an idle lane stays for the barriers)
    const int jj = tid % a.geo.NPB, gr = ln.g, i0 = ln.i0;
    const bool act = ln.live;
    const bool two = i0 + 1 < N;
    CellLam<2, RB> lam;
    lam.load(a.Lam, b, N, i0, r, ln.n);
    double ir0 = 0.0, ir1 = 0.0, sc0 = 1.0, sc1 = 1.0, mu0 = 0.0, mu1 = 0.0, sd0 = 1.0, sd1 = 1.0;
    const bool scale = a.mean != nullptr;
    if (act) {
        ir0 = a.R[b * N + i0];
        ir1 = two ? a.R[b * N + i0 + 1] : 1.0;
        if (scale) {
            const double sdt = a.sd[b * N + a.tgt[2 * gi + 1]];
            mu0 = a.mean[b * N + i0]; sd0 = a.sd[b * N + i0]; sc0 = sdt / sd0;
            if (two) { mu1 = a.mean[b * N + i0 + 1]; sd1 = a.sd[b * N + i0 + 1]; sc1 = sdt / sd1; }
        }
    }
    const double* G = a.g + (size_t)s * T * r;
    const bool want_news = a.news != nullptr && gi == 0;
    double acc0 = 0.0, acc1 = 0.0;
    for (int t0 = 0; t0 < T; t0 += a.geo.RC) {
        const int t1 = t0 + a.geo.RC < T ? t0 + a.geo.RC : T;
        cell_stage(sgr, G + (size_t)t0 * r, (t1 - t0) * r);
        __syncthreads();
        if (act)
            for (int t = t0 + gr; t < t1; t += a.geo.G) {
                const double* gt = sgr + (size_t)(t - t0) * r;
                const size_t cb = (b * T + t) * N + i0, cs = ((size_t)s * T + t) * N + i0, cx = (b * a.TH + t) * N + i0;
                double xn[2] = {0.0, 0.0}, xo[2] = {0.0, 0.0}, cv[2] = {0.0, 0.0}, xr[2] = {0.0, 0.0};
                cell_ld_pair<VEC>(a.newp + cb, two, xn);
                cell_ld_pair<VEC>(a.oldp + cb, two, xo);
                cell_ld_pair<VEC>(a.cp + cs, two, cv);
                cell_ld_pair<VEC>(a.xrev + cx, two, xr);
                double m[2];
                lam.dots(gt, r, m);
                const double m0 = m[0], m1 = m[1];
                const bool on0 = xn[0] == xn[0], on1 = two && xn[1] == xn[1];
                const double w[2] = {on0 ? sc0 * ((cv[0] - m0) / ir0) : 0.0, on1 ? sc1 * ((cv[1] - m1) / ir1) : 0.0};
                const double n[2] = {(on0 && xo[0] != xo[0]) ? (scale ? mu0 + sd0 * xn[0] : xn[0]) - xr[0] : 0.0,
                                     (on1 && xo[1] != xo[1]) ? (scale ? mu1 + sd1 * xn[1] : xn[1]) - xr[1] : 0.0};
                acc0 = fma(w[0], n[0], acc0);
                acc1 = fma(w[1], n[1], acc1);
                if (a.weight) cell_st_pair<VEC>(a.weight + ((size_t)j * T + t) * N + i0, two, w);
                if (want_news) cell_st_pair<VEC>(a.news + cb, two, n);
            }
        __syncthreads();
    }
    if (act) {
        sred[((size_t)gr * a.geo.NPB + jj) * 2] = acc0;
        sred[((size_t)gr * a.geo.NPB + jj) * 2 + 1] = acc1;
    }
    __syncthreads();
    if (act && gr == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int q = 0; q < a.geo.G; ++q) {
            s0 += sred[((size_t)q * a.geo.NPB + jj) * 2];
            s1 += sred[((size_t)q * a.geo.NPB + jj) * 2 + 1];
        }
        a.impact[(size_t)j * N + i0] = s0;
        if (two) a.impact[(size_t)j * N + i0 + 1] = s1;
    }
}

hipError_t launch_news_revise(const NwArgs& a, hipStream_t s) {
    const size_t n = (size_t)a.B * a.T * a.N;
    size_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(news_revise_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_news_gather(const NwArgs& a, const double* xhat, int which, hipStream_t s) {
    const int n = a.B * a.G;
    hipLaunchKernelGGL(news_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, xhat, which);
    return hipGetLastError();
}

hipError_t launch_news_gamma(const NwArgs& a, hipStream_t s) {
    const int k = a.r * a.p;
    if (k < 1 || k > 32 || a.S < 1) return hipErrorInvalidValue;
    // k > 8: four waves, one element of Gamma per lane at k = 16 (one wave with four elements per lane measured slower: 5.1 against
    // 4.0 ms at k = 16, T = 222, 4096 pass replicates)
    if (k <= 8) hipLaunchKernelGGL((news_gamma_kernel<8, 64>), dim3((unsigned)a.S), dim3(64), 0, s, a);
    else if (k <= 16) hipLaunchKernelGGL((news_gamma_kernel<16, 256>), dim3((unsigned)a.S), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((news_gamma_kernel<32, 256>), dim3((unsigned)a.S), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Both cell kernels: column pairs in lanes, r doubles per staged row, T rows (a 3-D / 2-D grid: its y and z extents are checked).
static bool nw_cells(NwArgs& a) {
    if (a.r < 1 || a.r > 32 || a.S < 1) return false;
    a.geo = cell_geometry((a.N + 1) / 2, a.r, a.T, kNwMaxThreads, kNwLds);
    return a.geo.nchunk <= 65535 && a.geo.nsblk <= 65535;
}

template <int RB>
static hipError_t launch_cov_rb(const NwArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)a.S, (unsigned)a.geo.nchunk, (unsigned)a.geo.nsblk);
    const size_t lds = (size_t)a.geo.RC * a.r * sizeof(double);
    return cell_launch_vec(news_cov_panel_kernel<RB, false>, news_cov_panel_kernel<RB, true>, vec, grid, a.geo.threads, lds, s, a);
}

hipError_t launch_news_cov_panel(NwArgs a, hipStream_t s) {
    if (!nw_cells(a)) return hipErrorInvalidValue;
    const bool vec = cell_vec(a.N, a.newp, a.cp);
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_cov_rb<decltype(RB)::value>(a, vec, s); });
}

template <int RB>
static hipError_t launch_impact_rb(const NwArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)a.S, (unsigned)a.geo.nsblk);
    const size_t lds = ((size_t)a.geo.RC * a.r + (size_t)2 * a.geo.G * a.geo.NPB) * sizeof(double);
    return cell_launch_vec(news_impact_kernel<RB, false>, news_impact_kernel<RB, true>, vec, grid, a.geo.threads, lds, s, a);
}

hipError_t launch_news_impact(NwArgs a, hipStream_t s) {
    if (!nw_cells(a)) return hipErrorInvalidValue;
    const bool vec = cell_vec(a.N, a.newp, a.oldp, a.cp, a.xrev, a.weight, a.news);
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_impact_rb<decltype(RB)::value>(a, vec, s); });
}

}  // namespace dfm
