// news_ar.hip -- news decomposition of nowcast revisions for the model with AR(q) idiosyncratic terms (dfm_news_ar_batch, capi.hip;
// DESIGN.md section 27).  With edge-shaped vintages (every series observed on panel rows 0 .. L_i, L_i >= 2q - 1) the output cells
// x = D^-1 xq (+ terms of the first q panel rows, which are conditioning values) are a linear map of the quasi-differenced cells
// xq_ti = h_i' z_t + eps_ti, a plain state-space model on the state z_t of m = max(p, q + 1) lags with loadings
// h_i = [lam_i, -rho_i1 lam_i, .., -rho_iq lam_i, 0 ..].  The target is y = sum_{t <= t*} psi_{t* - t} xq_{t,i*} (psi: the AR impulse
// response of series i*), so Cov(xq_ti, y) = h_i' d_t + [i = i*, t <= t*] psi_{t* - t} sig2_i* with
//   u_t = M' u_{t+1} + [t <= t*] psi_{t* - t} h_i*    (backwards from u_{t*+1} = 0)
//   v_t = M v_{t-1} + [t <= t*] psi_{t* - t} Gamma_t h_i*,   d_t = M v_{t-1} + Gamma_t u_t     (Gamma_t = M Gamma_{t-1} M' + Q_c, Gamma_-1 = P0)
// (d_t = v_t + Gamma_t M' u_{t+1}: the rows s <= t reach t through M^(t-s) Gamma_s, the rows s > t through Gamma_t M'^(s-t)).  One smoother
// pass with mu0 = 0 over that covariance panel leaves g_t = E_0[z_t | qc], eps^_ti = qc_ti - h_i' g_t = sig2_i (Sigma^-1 c)_ti, and the
// weights on the cells of x are the adjoint of the quasi-difference applied to eps^ / sig2.  Pass replicate j = b G + g:
//   news_ar_revise_kernel   the revised old panel and the vintage check (edge shape, L_i >= 2q - 1, old within new)        [B][T][N]
//   news_ar_rec_kernel      u_t (staged through global memory), then Gamma_t, v_t and d_t[: (q + 1) r] with psi_{t* - t}   [S][T-q][(q+1) r + 1]
//   news_ar_qc_kernel       qc on the new vintage's cells, NaN elsewhere                                                  [S][T-q][N]
//   news_ar_impact_kernel   eps^, w, the news I and the per-series impacts sum_t w I                                       [S][N]
// Output rows t = 0 .. T - q - 1 are panel rows q .. T - 1, as in forecast_ar.hip; targets arrive in output rows.
#include "dfm_cell.h"
#include "dfm_kernels.h"

namespace dfm {

constexpr int kNaTC = 32;                     // news_ar_rec_kernel: rows per LDS chunk of u_t / d_t (global traffic once per chunk)
constexpr int kNaVintageBit = 8;              // status word bit (DFM_E_VINTAGE, as news_revise_kernel)
constexpr int kNaQcMaxThreads = 512;
constexpr size_t kNaLds = 32 * 1024;          // cell kernels: the rows staged per workgroup

// One lane per (replicate, series) walks the rows: adjacent lanes are adjacent series, a row of the panel is one coalesced read.
// rev = new where old is observed, NaN elsewhere.  The vintage bit: an observed cell behind a missing one in either vintage (an
// interior gap or a late start), fewer than 2q observed rows in old, or a cell of old that is missing in new.
__global__ __launch_bounds__(256) void news_ar_revise_kernel(NwArArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)a.B * a.N) return;
    const size_t b = e / a.N;
    const int i = (int)(e % a.N);
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const size_t c0 = b * a.T * a.N + i;
    bool gap_o = false, gap_n = false, bad = false;
    int no = 0;
    for (int t = 0; t < a.T; ++t) {
        const size_t c = c0 + (size_t)t * a.N;
        const double xo = a.oldp[c], xn = a.newp[c];
        const bool oo = xo == xo, on = xn == xn;
        bad = bad || (oo && gap_o) || (on && gap_n) || (oo && !on);
        gap_o = gap_o || !oo;
        gap_n = gap_n || !on;
        no += oo ? 1 : 0;
        a.rev[c] = oo ? xn : qnan;
    }
    if (bad || no < 2 * a.q) atomicOr(a.status, kNaVintageBit);
}

// One workgroup per pass replicate of the slice; KB >= k = r m.  Phase U runs the u chain backwards from t* (which may lie in the
// horizon: rows >= T - q are walked and not stored) into a.u with psi_{t* - t} behind each row; phase Gamma runs Gamma_t, v_t and d_t
// forwards and reads u back.  Both stage kNaTC rows in LDS and touch global memory once per chunk: a barrier waits for every
// outstanding global store, so no row stores on its own.  Rows behind t* have u_t = 0 and psi = 0: d_t = v_t = M v_{t-1}.
template <int KB, int NT>
__global__ __launch_bounds__(NT) void news_ar_rec_kernel(NwArArgs a) {
    constexpr int NE = (KB * KB + NT - 1) / NT;               // elements of Gamma per thread
    constexpr int KS = KB + 1;                                // a staged row: the vector and psi
    __shared__ double sA[KB * KB], sG[KB * KB], sW[KB * KB];
    __shared__ double sU[kNaTC * KS], sD[kNaTC * KS], sv[2][KB], sh[KB];
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G), r = a.r, q = a.q, k = a.k, ka = a.ka, ns = a.ns, N = a.N, w = (q + 1) * r;
    const int ts = a.tgt[2 * gi], is = a.tgt[2 * gi + 1];
    const size_t bis = b * N + is;
    double qe[NE];                                            // Q_c of this thread's elements
#pragma unroll
    for (int c = 0; c < NE; ++c) {
        const int e = tid + c * NT, i = e / k, m = e % k;
        qe[c] = 0.0;
        if (e >= k * k) continue;
        sA[i * KB + m] = i < r ? (m < ka ? a.A[(b * r + i) * ka + m] : 0.0) : (m == i - r ? 1.0 : 0.0);
        sG[i * KB + m] = a.P0[(b * k + i) * k + m];
        qe[c] = (i < r && m < r) ? a.Q[(b * r + i) * r + m] : 0.0;
    }
    if (tid < k) {
        const int l = tid / r;
        double v = 0.0;
        if (l <= q) v = (l == 0 ? 1.0 : -a.rho[bis * q + (l - 1)]) * a.Lam[bis * r + tid % r];
        sh[tid] = v;
        sv[0][tid] = 0.0;
    }
    double rh[4], ps[4] = {1.0, 0.0, 0.0, 0.0};               // rho of the target series (zero beyond q); psi_j, .., psi_{j-3}
#pragma unroll
    for (int l = 0; l < 4; ++l) rh[l] = l < q ? a.rho[bis * q + l] : 0.0;
    __syncthreads();
    double* U = a.u + (size_t)s * ns * (k + 1);
    double* DV = a.dv + (size_t)s * ns * (w + 1);
    const int tl = ts < ns ? ts : ns - 1;                     // the last stored row with a source
    // phase U: u_t for t = t* .. 0, the chunk of rows [t, t + 32) flushed when t reaches its first row
    int cur = 0;
    for (int t = ts; t >= 0; --t) {
        const int row = t % kNaTC;
        if (tid < k) {
            double v = ps[0] * sh[tid];
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sA[m * KB + tid], sv[cur][m], v);
            sv[cur ^ 1][tid] = v;
            if (t < ns) sU[row * KS + tid] = v;
        }
        if (tid == 0 && t < ns) sU[row * KS + KB] = ps[0];
        {
            const double pn = fma(rh[0], ps[0], fma(rh[1], ps[1], fma(rh[2], ps[2], rh[3] * ps[3])));
            ps[3] = ps[2]; ps[2] = ps[1]; ps[1] = ps[0]; ps[0] = pn;
        }
        cur ^= 1;
        __syncthreads();
        if (t < ns && row == 0) {
            const int nr = (t + kNaTC <= tl ? t + kNaTC : tl + 1) - t;
            for (int e = tid; e < nr * (k + 1); e += NT) {
                const int c = e % (k + 1);
                U[(size_t)t * (k + 1) + e] = sU[(e / (k + 1)) * KS + (c < k ? c : KB)];
            }
            __syncthreads();                                  // (the rows below reuse the buffer)
        }
    }
    if (tid < k) sv[0][tid] = 0.0;
    cur = 0;
    __syncthreads();                                          // (u is read back below by other threads)
    for (int t = 0; t < ns; ++t) {
        const int row = t % kNaTC;
        if (row == 0) {                                       // u rows of this chunk (read two barriers later), zero behind t*
            __syncthreads();
            const int nr = (t + kNaTC < ns ? t + kNaTC : ns) - t;
            for (int e = tid; e < nr * (k + 1); e += NT) {
                const int c = e % (k + 1), rr = e / (k + 1);
                sU[rr * KS + (c < k ? c : KB)] = t + rr <= tl ? U[(size_t)t * (k + 1) + e] : 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < NE; ++c) {                        // W = M Gamma
            const int e = tid + c * NT, i = e / k, cc = e % k;
            if (e >= k * k) continue;
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sA[i * KB + m], sG[cc * KB + m], v);
            sW[i * KB + cc] = v;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NE; ++c) {                        // Gamma = W M' + Q_c
            const int e = tid + c * NT, i = e / k, cc = e % k;
            if (e >= k * k) continue;
            double v = qe[c];
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) v = fma(sW[i * KB + m], sA[cc * KB + m], v);
            sG[i * KB + cc] = v;
        }
        __syncthreads();
        const double psi = sU[row * KS + KB];
        if (tid < k) {
            double mv = 0.0, gu = 0.0, gh = 0.0;
#pragma unroll
            for (int m = 0; m < KB; ++m)
                if (m < k) {
                    const double gm = sG[tid * KB + m];
                    mv = fma(sA[tid * KB + m], sv[cur][m], mv);
                    gu = fma(gm, sU[row * KS + m], gu);
                    gh = fma(gm, sh[m], gh);
                }
            sv[cur ^ 1][tid] = fma(psi, gh, mv);
            if (tid < w) sD[row * KS + tid] = mv + gu;
        }
        if (tid == 0) sD[row * KS + KB] = psi;
        cur ^= 1;
        if (row == kNaTC - 1 || t == ns - 1) {
            __syncthreads();
            const int c0 = t - row;
            for (int e = tid; e < (row + 1) * (w + 1); e += NT) {
                const int c = e % (w + 1);
                DV[(size_t)c0 * (w + 1) + e] = sD[(e / (w + 1)) * KS + (c < w ? c : KB)];
            }
        }
    }
}

// The lane's series: loadings, AR coefficients (an idle lane is not loaded: it has returned, or walks series N - 1 for the barriers).
template <int Q, int RB>
struct NaSeries {
    CellLam<1, RB> lam;
    double rho[Q];
    __device__ __forceinline__ void load(const NwArArgs& a, size_t b, int i) {
        lam.load(a.Lam, b, a.N, i, a.r);
#pragma unroll
        for (int l = 0; l < Q; ++l) rho[l] = a.rho[(b * a.N + i) * Q + l];
    }
    // h_i' row for a row of q + 1 lag blocks, r doubles each: lam' (row_0 - sum_l rho_l row_l)
    __device__ __forceinline__ double hdot(const double* row, int r) const {
        double v = lam.dot(0, row, r);
#pragma unroll
        for (int l = 0; l < Q; ++l) v = fma(-rho[l], lam.dot(0, row + (l + 1) * r, r), v);
        return v;
    }
};

// The covariance panels: chunk blockIdx.y of the rows of pass replicate blockIdx.x, series of block blockIdx.z, one series per lane.
template <int Q, int RB>
__global__ __launch_bounds__(kNaQcMaxThreads) void news_ar_qc_kernel(NwArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sdv[];
    const int r = a.r, N = a.N, ns = a.ns, tid = threadIdx.x, w1 = (Q + 1) * r + 1;
    const int s = blockIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.z, blockIdx.y, s, ns);
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G);
    const int t0 = ch.t0, t1 = ch.t1;
    cell_stage(sdv, a.dv + ((size_t)s * ns + t0) * w1, (t1 - t0) * w1);
    __syncthreads();
    const CellLane ln = cell_lane<1>(a.geo, tid, ch.s, N);
    if (!ln.live) return;
    const int i = ln.i0, is = a.tgt[2 * gi + 1];
    NaSeries<Q, RB> se;
    se.load(a, b, i);
    const double radd = i == is ? a.sig2[b * N + is] : 0.0;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double* px = a.newp + (b * a.T + Q) * N + i;        // output row t of the lane's series: px[t N]
    double xn = t0 + ln.g < t1 ? px[(size_t)(t0 + ln.g) * N] : qnan;
    for (int t = t0 + ln.g; t < t1; t += a.geo.G) {
        const double* dv = sdv + (size_t)(t - t0) * w1;
        const double x = xn;
        if (t + a.geo.G < t1) xn = px[(size_t)(t + a.geo.G) * N];   // the next row's cell, in flight while this row is computed
        const double m = fma(dv[w1 - 1], radd, se.hdot(dv, r));
        const double y[1] = {x == x ? m : qnan};
        cell_st<1>(a.qc + ((size_t)s * ns + t) * N + i, y);
    }
}

// eps^, w, I and the impacts of pass replicate blockIdx.x / nsblk, series of block blockIdx.x % nsblk: one series per lane, rows
// from the last to the first with eps^_{t+1 .. t+q} in registers (zero behind the sample: those quasi-differences are not
// observed), the impact summed by the lane in that fixed order.  The covariance panel may be the slice's part of weight: each cell is
// read before the same lane writes w there.
template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void news_ar_impact_kernel(NwArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sg[];
    const int r = a.r, N = a.N, ns = a.ns, tid = threadIdx.x, w = (Q + 1) * r;
    const int sb = (int)(blockIdx.x % (unsigned)a.geo.nsblk), s = (int)(blockIdx.x / (unsigned)a.geo.nsblk);
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.G);
    const int gi = (int)(j % a.G);
    const CellLane ln = cell_lane<1>(a.geo, tid, sb, N);     // (an idle lane stays for the barriers)
    const bool live = ln.live;
    const int i = live ? ln.i0 : N - 1;
    NaSeries<Q, RB> se;
    se.load(a, b, i);
    const size_t bi = b * N + i;
    const bool scale = a.mean != nullptr;
    const double isig = 1.0 / a.sig2[bi];
    const double mu = scale ? a.mean[bi] : 0.0, sd = scale ? a.sd[bi] : 1.0;
    const double sc = scale ? a.sd[b * N + a.tgt[2 * gi + 1]] / sd : 1.0;
    const bool want_news = a.news != nullptr && gi == 0;
    const double* pn = a.newp + (b * a.T + Q) * N + i;        // output row t of the lane's series: [t N]
    const double* po = a.oldp + (b * a.T + Q) * N + i;
    const double* pc = a.qc + (size_t)s * ns * N + i;
    const double* pr = a.xrev + b * a.n * N + i;
    double ea[Q];                                             // eps^_{t+1 .. t+q}
#pragma unroll
    for (int l = 0; l < Q; ++l) ea[l] = 0.0;
    double acc = 0.0;
    double nx[4] = {pn[(size_t)(ns - 1) * N], po[(size_t)(ns - 1) * N], pc[(size_t)(ns - 1) * N], pr[(size_t)(ns - 1) * N]};
    for (int ck = a.geo.nchunk - 1; ck >= 0; --ck) {
        const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < ns ? t0 + a.geo.RC : ns;
        __syncthreads();
        cell_stage(sg, a.g + ((size_t)s * ns + t0) * a.Rp, t1 - t0, w, a.Rp);
        __syncthreads();
        for (int t = t1 - 1; t >= t0; --t) {
            const double xn = nx[0], xo = nx[1], cv = nx[2], xr = nx[3];
            if (t > 0) {                                      // one row ahead, in flight during this row's algebra
                const size_t o = (size_t)(t - 1) * N;
                nx[0] = pn[o]; nx[1] = po[o]; nx[2] = pc[o]; nx[3] = pr[o];
            }
            const bool on = xn == xn;
            const double e = on ? cv - se.hdot(sg + (size_t)(t - t0) * w, r) : 0.0;
            double ad = e;
#pragma unroll
            for (int l = 0; l < Q; ++l) ad = fma(-se.rho[l], ea[l], ad);
#pragma unroll
            for (int l = Q - 1; l > 0; --l) ea[l] = ea[l - 1];
            ea[0] = e;
            const double wt[1] = {on ? sc * (ad * isig) : 0.0};
            const double nw[1] = {(on && xo != xo) ? (scale ? mu + sd * xn : xn) - xr : 0.0};
            acc = fma(wt[0], nw[0], acc);
            if (live) {
                if (a.weight) cell_st<1>(a.weight + ((size_t)j * ns + t) * N + i, wt);
                if (want_news) cell_st<1>(a.news + (b * ns + t) * N + i, nw);
            }
        }
    }
    if (live) a.impact[(size_t)j * N + i] = acc;
}

hipError_t launch_news_ar_revise(const NwArArgs& a, hipStream_t s) {
    const size_t n = (size_t)a.B * a.N, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(news_ar_revise_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_news_ar_rec(const NwArArgs& a, hipStream_t s) {
    if (a.k < 1 || a.k > 32 || a.ka > a.k || (a.q + 1) * a.r > a.k || a.q < 1 || a.q > 4 || a.ns < 1 || a.S < 1) return hipErrorInvalidValue;
    // as launch_news_gamma: four waves beyond k = 8, one element of Gamma per lane at k = 16
    if (a.k <= 8) hipLaunchKernelGGL((news_ar_rec_kernel<8, 64>), dim3((unsigned)a.S), dim3(64), 0, s, a);
    else if (a.k <= 16) hipLaunchKernelGGL((news_ar_rec_kernel<16, 256>), dim3((unsigned)a.S), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((news_ar_rec_kernel<32, 256>), dim3((unsigned)a.S), dim3(256), 0, s, a);
    return hipGetLastError();
}

enum NaKind { kNaQc, kNaImpact };

template <int Q, int RB>
static hipError_t launch_na_q(NwArArgs a, NaKind kind, hipStream_t s) {
    const int w = (Q + 1) * a.r;
    if (kind == kNaQc) {
        a.geo = cell_geometry(a.N, w + 1, a.ns, kNaQcMaxThreads, kNaLds);
        if (a.geo.nchunk > 65535 || a.geo.nsblk > 65535) return hipErrorInvalidValue;
        const dim3 grid((unsigned)a.S, (unsigned)a.geo.nchunk, (unsigned)a.geo.nsblk);
        hipLaunchKernelGGL((news_ar_qc_kernel<Q, RB>), grid, dim3(a.geo.threads), (size_t)a.geo.RC * (w + 1) * sizeof(double), s, a);
    } else {
        a.geo = series_geometry(a.N, w, a.ns, kNaLds);
        const size_t blocks = (size_t)a.S * a.geo.nsblk;
        if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
        hipLaunchKernelGGL((news_ar_impact_kernel<Q, RB>), dim3((unsigned)blocks), dim3(a.geo.threads), (size_t)a.geo.RC * w * sizeof(double), s, a);
    }
    return hipGetLastError();
}

template <int Q>
static hipError_t launch_na_r(const NwArArgs& a, NaKind kind, hipStream_t s) {
    if (a.r <= 4) return launch_na_q<Q, 4>(a, kind, s);
    if (a.r <= 8) return launch_na_q<Q, 8>(a, kind, s);
    return launch_na_q<Q, 16>(a, kind, s);
}

static hipError_t launch_na(const NwArArgs& a, NaKind kind, hipStream_t s) {
    if (a.r < 1 || a.r > 16 || (a.q + 1) * a.r > 32 || a.ns < 1 || a.S < 1) return hipErrorInvalidValue;
    switch (a.q) {
        case 1: return launch_na_r<1>(a, kind, s);
        case 2: return launch_na_r<2>(a, kind, s);
        case 3: return launch_na_r<3>(a, kind, s);
        case 4: return launch_na_r<4>(a, kind, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_news_ar_qc(const NwArArgs& a, hipStream_t s) { return launch_na(a, kNaQc, s); }
hipError_t launch_news_ar_impact(const NwArArgs& a, hipStream_t s) { return launch_na(a, kNaImpact, s); }

}  // namespace dfm
