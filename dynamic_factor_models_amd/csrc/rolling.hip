// rolling.hip -- rolling-window out-of-sample evaluation, re-estimated at every origin (dfm_rolling_eval_batch, capi.hip;
// DESIGN.md section 29).  Window b of the slice is rows o_b - W + 1 .. o_b of the raw panel; cell (t, i) of it is visible iff it is
// observed and t <= o_b - lag_i.  Around the EM and the forecast entries the driver reuses:
//   rolling_window_kernel   the vintage of every window, standardised on its own visible cells, and its mean / sd / count   [S][W][N]
//   rolling_start_kernel    the start parameters of every window, the loadings and variances in the window's units           [S][..]
//   rolling_score_kernel    fc, fvar, err, err_std of the target rows and the running sums of squared errors per (h, i)      [S][H+1][N]
// The window kernel is the panel-sized one: a workgroup owns one window and one block of kRwSeries series as kRwPairs column pairs
// in kRwGroups row groups; the raw panel is shared by all windows (L2), the bound is the store.  Its three sweeps (sum, centred sum of
// squares, store) reduce the row groups' partials in LDS in the order of the groups: no atomics, every lane of a pair adds the
// same numbers in the same order, so nothing is broadcast.  The score kernel has one lane per (horizon, series) and walks the
// slice's windows in order: its sums are the same from run to run.
#include "dfm_cell.h"
#include "dfm_kernels.h"

namespace dfm {

constexpr int kRwSeries = 64;                 // series per workgroup of rolling_window_kernel
constexpr int kRwPairs = kRwSeries / 2;       // column pairs (one lane each)
constexpr int kRwGroups = 8;                  // row groups
constexpr int kRwThreads = kRwPairs * kRwGroups;

// A lane's pair of partials reduced over the row groups in their order (op: +, fmin, fmax from `init`); every lane of the pair
// gets the totals.  Counts ride as doubles: they are integers below 2^31, so their sums are exact.
template <class Op>
__device__ __forceinline__ void rw_reduce(double (*sa)[kRwPairs][2], int g, int j, double (&a)[2], double init, Op op) {
    sa[g][j][0] = a[0]; sa[g][j][1] = a[1];
    __syncthreads();
    a[0] = a[1] = init;
#pragma unroll
    for (int q = 0; q < kRwGroups; ++q) {
        a[0] = op(a[0], sa[q][j][0]);
        a[1] = op(a[1], sa[q][j][1]);
    }
    __syncthreads();                                          // (the next reduction writes the same array)
}

template <bool VEC>
__global__ __launch_bounds__(kRwThreads) void rolling_window_kernel(RwArgs a) {
    __shared__ double sa[kRwGroups][kRwPairs][2];
    const int tid = threadIdx.x, j = tid % kRwPairs, g = tid / kRwPairs;
    const int s = blockIdx.x, i0 = (blockIdx.y * kRwPairs + j) * 2;
    const int N = a.N, W = a.W;
    const bool live = i0 < N, two = i0 + 1 < N;               // (an idle lane stays for the barriers)
    const int ob = a.origins[a.b0 + s];
    const double* xs = a.x + (size_t)(ob - W + 1) * N + i0;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    // rows t < vis[q] of the window are inside the vintage of series i0 + q
    int vis[2] = {live ? W : 0, two ? W : 0};
    if (a.lags) {
        if (live) vis[0] = W - a.lags[i0];
        if (two) vis[1] = W - a.lags[i0 + 1];
    }
    // sweep 1: the sum, the count and the range of the visible cells
    double sum[2] = {0.0, 0.0}, lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    double cnt[2] = {0.0, 0.0};
    if (live)
        for (int t = g; t < W; t += kRwGroups) {
            double x[2] = {qnan, qnan};
            cell_ld_pair<VEC>(xs + (size_t)t * N, two, x);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (t < vis[q] && x[q] == x[q]) {
                    sum[q] += x[q]; cnt[q] += 1.0;
                    lo[q] = fmin(lo[q], x[q]); hi[q] = fmax(hi[q], x[q]);
                }
        }
    const auto add = [](double u, double v) { return u + v; };
    rw_reduce(sa, g, j, sum, 0.0, add);
    rw_reduce(sa, g, j, cnt, 0.0, add);
    rw_reduce(sa, g, j, lo, INFINITY, [](double u, double v) { return fmin(u, v); });
    rw_reduce(sa, g, j, hi, -INFINITY, [](double u, double v) { return fmax(u, v); });
    const double mu[2] = {sum[0] / cnt[0], sum[1] / cnt[1]};
    // sweep 2: the centred sum of squares
    double ss[2] = {0.0, 0.0};
    if (live)
        for (int t = g; t < W; t += kRwGroups) {
            double x[2] = {qnan, qnan};
            cell_ld_pair<VEC>(xs + (size_t)t * N, two, x);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (t < vis[q] && x[q] == x[q]) {
                    const double d = x[q] - mu[q];
                    ss[q] += d * d;
                }
        }
    rw_reduce(sa, g, j, ss, 0.0, add);
    const double sd[2] = {sqrt(ss[0] / cnt[0]), sqrt(ss[1] / cnt[1])};
    if (g == 0) {
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (q == 0 ? live : two) {
                const size_t o = (size_t)s * N + i0 + q;
                a.mean[o] = mu[q]; a.sd[o] = sd[q]; a.nobs[o] = (int)cnt[q];
                // constant: the visible cells' range is empty (exact, whatever the rounding of the mean), or the sd says so
                bad = bad || cnt[q] < a.min_obs || !(sd[q] > 0.0) || lo[q] == hi[q];
            }
        if (bad) atomicOr(a.status, kRwWindowBit);
    }
    // sweep 3: the vintage, standardised
    if (live)
        for (int t = g; t < W; t += kRwGroups) {
            double x[2] = {qnan, qnan};
            cell_ld_pair<VEC>(xs + (size_t)t * N, two, x);
            const double y[2] = {t < vis[0] ? (x[0] - mu[0]) / sd[0] : qnan, t < vis[1] ? (x[1] - mu[1]) / sd[1] : qnan};
            cell_st_pair<VEC>(a.win + ((size_t)s * W + t) * N + i0, two, y);
        }
}

// Element e of the largest of the slice's parameter arrays; the start is window 0's (n_start = 1) or window b0 + s's own.
__global__ __launch_bounds__(256) void rolling_start_kernel(RwArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = a.N, r = a.r, k = a.k, S = a.S;
    const size_t nL = S * N * r, nR = S * N, nA = S * r * k, nQ = S * r * r, nm = S * k, nP = S * k * k;
    auto src = [&](size_t per) { return a.n_start == 1 ? e % per : (size_t)a.b0 * per + e; };
    if (e < nL) {
        const size_t si = e / r, i = si % N;
        const double sc = a.sd_start ? a.sd_start[i] / a.sd[si] : 1.0;
        a.Lam[e] = a.sLam[src(N * r)] * sc;
    }
    if (e < nR) {
        const double sc = a.sd_start ? a.sd_start[e % N] / a.sd[e] : 1.0;
        a.R[e] = a.sR[src(N)] * (sc * sc);
    }
    if (e < nA) a.A[e] = a.sA[src(r * k)];
    if (e < nQ) a.Q[e] = a.sQ[src(r * r)];
    if (e < nm) a.mu0[e] = a.smu0[src(k)];
    if (e < nP) a.P0[e] = a.sP0[src(k * k)];
}

// Lane = one (h, i): consecutive lanes are consecutive series of one horizon.  It walks the slice's windows in order, so the sum of
// (h, i) takes its terms in origin order whatever the slicing.  Target row o_b + h is scored iff it is inside the panel, outside the
// vintage (h >= 1, or h = 0 with lag_i > 0) and observed.  Nothing a lane stores is read again in the launch (__restrict__): the
// loads of four windows are in flight together, the adds stay in order.
__global__ __launch_bounds__(256) void rolling_score_kernel(RwArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.N, W = a.W, H1 = a.H + 1, T = a.T;
    if (e >= H1 * N) return;
    const int h = e / N, i = e % N;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const bool hidden = h > 0 || (a.lags && a.lags[i] > 0);
    const size_t per = ((size_t)W + a.H) * N, out = (size_t)H1 * N;
    const double* __restrict__ xh = a.xhat + (size_t)(W - 1 + h) * N + i;
    const double* __restrict__ xv = a.xvar + (size_t)(W - 1 + h) * N + i;
    const double* __restrict__ x = a.x + i;
    const double* __restrict__ mean = a.mean + i;
    const int* __restrict__ org = a.origins + a.b0;
    double* __restrict__ fc = a.fc ? a.fc + e : nullptr;
    double* __restrict__ fvar = a.fvar ? a.fvar + e : nullptr;
    double* __restrict__ err = a.err ? a.err + e : nullptr;
    double* __restrict__ err_std = a.err_std ? a.err_std + e : nullptr;
    double se = a.first ? 0.0 : a.sse[e], s0 = a.first ? 0.0 : a.sse0[e];
    int c = a.first ? 0 : a.cnt[e];
#pragma unroll 4
    for (int s = 0; s < a.S; ++s) {
        const int tt = org[s] + h;
        const double f = xh[s * per], v = xv[s * per], mu = mean[(size_t)s * N];
        double t = qnan;
        if (hidden && tt < T) t = x[(size_t)tt * N];
        const bool scored = t == t;
        const double d = scored ? t - f : qnan;
        if (fc) fc[s * out] = f;
        if (fvar) fvar[s * out] = v;
        if (err) err[s * out] = d;
        if (err_std) err_std[s * out] = scored ? d / sqrt(v) : qnan;
        if (scored) {
            const double d0 = t - mu;
            se += d * d; s0 += d0 * d0; ++c;
        }
    }
    a.sse[e] = se; a.sse0[e] = s0; a.cnt[e] = c;
    if (a.last) {
        if (a.msfe) a.msfe[e] = c ? se / c : qnan;
        if (a.msfe0) a.msfe0[e] = c ? s0 / c : qnan;
        if (a.cnt_out) a.cnt_out[e] = c;
    }
}

hipError_t launch_rolling_window(const RwArgs& a, hipStream_t s) {
    const int nblk = (a.N + kRwSeries - 1) / kRwSeries;
    if (a.S < 1 || nblk > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.S, (unsigned)nblk);
    return cell_launch_vec(rolling_window_kernel<false>, rolling_window_kernel<true>, cell_vec(a.N, a.x, a.win), grid, kRwThreads, 0, s, a);
}

hipError_t launch_rolling_start(const RwArgs& a, hipStream_t s) {
    const size_t S = a.S, N = a.N, r = a.r, k = a.k;
    const size_t nL = S * N * r, nP = S * k * k, n = nL > nP ? nL : nP;      // (the largest two: r <= k, so A, Q, mu0 <= P0)
    hipLaunchKernelGGL(rolling_start_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rolling_score(const RwArgs& a, hipStream_t s) {
    const size_t n = ((size_t)a.H + 1) * a.N;
    if (n > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rolling_score_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
