// diffusion.hip -- diffusion-index forecasts from the non-parametric fit, out of sample (dfm_diffusion_eval_batch, capi.hip;
// DESIGN.md section 30): Stock and Watson (2002).  Window b of the slice is the standardised vintage z [W][N] of rolling_window_kernel
// and its ALS factors F [W][r] (als_kernel, one workgroup per window).  For every series i (publication lag l) and horizon h with
// h + l >= 1 the direct regression, in window-local rows s (row W - 1 is the origin),
//     z_{s+h,i} = beta' u_s + e,   u_s = [1, F_s (r), z_{s-l,i}, .., z_{s-l-q+1,i}]   (K = 1 + r + q regressors)
// runs over the complete cases among s = max(0, l + q - 1) .. W - 1 - l - h; the AR benchmark is the same rows on the columns
// {1, own lags}; the forecasts are beta' u_{W-1}.
//   di_start_kernel     the start factors of every window, cut from one [T][r] path or copied from [O][W][r]; a NaN inside a window
//                       of a panel that was declared complete raises status bit 1                                       [S][W][r]
//   di_regress_kernel   the hot path: Gram matrix on the fly, two solves, forecast and residual variance              [S][H+1][N]
//   di_score_kernel     err, err_ar, err_std of the target rows and the running sums of squared errors per (h, i)      [S][H+1][N]
// di_regress_kernel<R>: a workgroup owns one window and one block of nb series; it stages F and the block's columns of z into LDS
// once (the only reads of either; the only place the finiteness of F is looked at).  A lane group of R = pad(K) lanes owns one
// (series, horizon): lane k holds row k of the Gram matrix and entry k of the right-hand side, as ols_kernel does; no regressor
// matrix exists anywhere.  A group never spans two waves and its exchange rows are its own, so every exchange is fenced at wave
// level (wave_lds_sync, gj_inverse<R, true>), as in breaks.hip: the groups of a wave run rows of different number.  No atomics.
// The score kernel has one lane per (horizon, series) and walks the slice's windows in order: its sums are the same from run to run
// and under any slicing.
#include "dfm_kernels.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr int kDiThreads = 256;
constexpr int kDiSeries = 16;                 // series per workgroup of di_regress_kernel where the LDS image allows it
constexpr int kDiExchange = 3 * kDiThreads;   // doubles: per lane group [2R] Gauss-Jordan rows and [R] vector exchange
constexpr size_t kDiLdsMax = 160 * 1024 - 64;   // (the 160 KB less the kernel's static word)

// (R = 32: one more [R][R] per lane group, where the Gram matrix waits while the benchmark is solved -- two copies of it beside the
// elimination's row do not fit the registers)
static __host__ __device__ size_t di_lds_doubles(int W, int r, int nb, int R) {
    return (size_t)W * (r + nb) + kDiExchange + (R == 32 ? (size_t)kDiThreads * R : 0);
}

int di_series_block(int W, int r, int Rpad) {
    for (int nb = kDiSeries; nb >= 1; nb >>= 1)
        if (di_lds_doubles(W, r, nb, Rpad) * sizeof(double) <= kDiLdsMax) return nb;
    return 0;
}

// sum over the R lanes of a group (aligned to R), in every lane of it
template <int R>
__device__ __forceinline__ double di_group_sum(double v) {
#pragma unroll
    for (int off = 1; off < R; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// x = D Ginv D h of the group's system G (row k in Grow, destroyed), D = diag(G)^-1/2
template <int R>
__device__ __forceinline__ double di_solve(double (&Grow)[R], double hk, double* Xg, double* hb, int k) {
    const double dk = equilibrate_rows<R, true>(Grow, Xg, k);
    gj_inverse<R, true>(Grow, Xg, k);
    wave_lds_sync();
    hb[k] = hk * dk;
    wave_lds_sync();
    double x = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) x = fma(Grow[j], hb[j], x);
    wave_lds_sync();                                          // (the caller writes hb again)
    return x * dk;
}

// regressor sm[base + t * stride] of window row t >= tmin (NaN in front of it), or the lane's fixed value
__device__ __forceinline__ double di_reg(const double* sm, int t, int base, int stride, int tmin, bool reads, double fixed) {
    const double v = sm[t >= tmin ? base + t * stride : 0];
    return reads ? (t >= tmin ? v : __longlong_as_double(0x7FF8000000000000ll)) : fixed;
}

template <int R>
__global__ __launch_bounds__(kDiThreads) void di_regress_kernel(DiArgs a) {
    constexpr int NG = kDiThreads / R;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ int sbad;
    const int W = a.W, N = a.N, r = a.r, q = a.q, K = a.K, H1 = a.H + 1, nb = a.nb;
    const int zoff = W * r;                                   // sm: [W][r] factors, [W][nb] the block's columns of z, the exchange rows
    double* zc = sm + zoff;
    const int tid = threadIdx.x, grp = tid / R, k = tid % R;
    double* Xg = zc + (size_t)W * nb + grp * 3 * R;
    double* hb = Xg + 2 * R;
    double* Gs = zc + (size_t)W * nb + kDiExchange + grp * R * R + k;   // (R = 32) entry j of the lane's row at Gs[j * R]
    const int s = blockIdx.x, i0 = blockIdx.y * nb;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double* __restrict__ Fg = a.F + (size_t)s * W * r;
    const double* __restrict__ z = a.win + (size_t)s * W * N;
    if (tid == 0) sbad = 0;
    __syncthreads();
    bool nonfinite = false;
    for (int e = tid; e < W * r; e += kDiThreads) {
        const double v = Fg[e];
        sm[e] = v;
        nonfinite = nonfinite || !(fabs(v) <= 1.7976931348623157e308);
    }
    for (int e = tid; e < W * nb; e += kDiThreads) {
        const int t = e / nb, i = i0 + e % nb;
        zc[e] = i < N ? z[(size_t)t * N + i] : qnan;
    }
    if (nonfinite) sbad = 1;
    __syncthreads();
    const bool bad = sbad != 0;                               // a window whose factors hold a non-finite value forecasts NaN

    // without publication lags every cell of h = 0 is visible: nothing is forecast there, and no lane group is spent on it
    const int hf = a.h_first, Hn = H1 - hf;
    const int nser = N - i0 < nb ? N - i0 : nb, ntask = nser * Hn;
    if (hf)
        for (int e = tid; e < nser; e += kDiThreads) {
            const size_t o = (size_t)s * H1 * N + i0 + e;
            a.fc[o] = qnan; a.fc_ar[o] = qnan; a.fvar[o] = qnan;
            if (a.nobs_reg) a.nobs_reg[o] = 0;
            if (a.beta)
                for (int j = 0; j < K; ++j) a.beta[o * K + j] = qnan;
        }
    for (int t0 = 0; t0 < ntask; t0 += NG) {                  // (the same number of rounds in every wave: the fences are wave-wide)
        const int task = t0 + grp;
        const bool act = task < ntask;
        const int c = act ? task / Hn : 0, h = act ? hf + task % Hn : 0, i = i0 + c;
        const int l = a.lags ? a.lags[i] : 0;
        // regressor k of window row t is sm[base + t * stride]: a factor, or an own lag (NaN in front of the window); the constant is
        // 1 and a lane past K holds 0
        const int m = k - r - 1;                              // own lag m = 0 .. q - 1 of lanes r + 1 .. K - 1
        const bool isf = k >= 1 && k <= r, isl = k > r && k < K;
        const int base = isf ? k - 1 : isl ? zoff + c - (l + m) * nb : 0, stride = isf ? r : isl ? nb : 0, tmin = isl ? l + m : 0;
        const double fixed = k == 0 ? 1.0 : 0.0;
        const bool reads = isf || isl;
#define DI_REG(t) di_reg(sm, (t), base, stride, tmin, reads, fixed)
        const bool run = act && !bad && h + l >= 1;           // (h + l = 0: the cell is visible, nothing is forecast)
        const int s_lo = l + q - 1 > 0 ? l + q - 1 : 0, s_hi = run ? W - 1 - l - h : -1;
        double G0[R];
#pragma unroll
        for (int j = 0; j < R; ++j) G0[j] = 0.0;
        double h0 = 0.0;
        int cnt = 0;
        for (int t = s_lo; t <= s_hi; ++t) {                  // the row's regressors go round the group through its exchange rows
            const double yv = zc[(t + h) * nb + c], uk = DI_REG(t);
            double* ub = Xg + (t & 1) * R;
            ub[k] = uk;
            wave_lds_sync();
            double u[R];
            bool ok = yv == yv;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                u[j] = ub[j];
                ok = ok && (u[j] == u[j]);
            }
            if (ok) {
                ++cnt;
                h0 = fma(yv, uk, h0);
#pragma unroll
                for (int j = 0; j < R; ++j) G0[j] = fma(uk, u[j], G0[j]);
            }
        }
        const bool solve = run && cnt >= a.nt_min && cnt >= K;          // dfm_ols_batch's rule
        // two solves of one text, the AR benchmark (the sub-system of the constant and the own lags) and the whole regression: a loop
        // that stays rolled, so that one elimination's registers are live at a time
        if constexpr (R == 32) {
#pragma unroll
            for (int j = 0; j < R; ++j) Gs[j * R] = G0[j];
        }
        double ak = 0.0, bk = 0.0;
#pragma nounroll
        for (int pass = 0; pass < 2; ++pass) {
            const bool whole = pass == 1;
            const bool mine = solve && (whole ? k < K : (k == 0 || isl));
            double G[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const bool col = whole ? j < K : (j == 0 || (j > r && j < K));
                double g = G0[j];
                if constexpr (R == 32) g = Gs[j * R];
                G[j] = mine ? (col ? g : 0.0) : (j == k ? 1.0 : 0.0);
            }
            const double x = di_solve<R>(G, mine ? h0 : 0.0, Xg, hb, k);
            ak = whole ? ak : x;
            bk = whole ? x : bk;
        }
        // its residual sum of squares: row after row, the fit summed over the group (a NaN regressor makes the fit NaN)
        double ss = 0.0;
        if (solve)
            for (int t = s_lo; t <= s_hi; ++t) {
                const double e = zc[(t + h) * nb + c] - di_group_sum<R>(bk * DI_REG(t));
                if (e == e) ss = fma(e, e, ss);
            }
        const double uo = DI_REG(W - 1);                      // the origin's regressors: NaN where an own lag is missing
#undef DI_REG
        const double fz = di_group_sum<R>(bk * uo), fa = di_group_sum<R>(ak * uo);
        if (act) {
            const size_t o = ((size_t)s * H1 + h) * N + i;
            if (k < K && a.beta) a.beta[o * K + k] = solve ? bk : qnan;
            if (k == 0) {
                const double mu = a.mean[(size_t)s * N + i], sd = a.sd[(size_t)s * N + i];
                a.fc[o] = solve ? fma(sd, fz, mu) : qnan;
                a.fc_ar[o] = solve ? fma(sd, fa, mu) : qnan;
                a.fvar[o] = (solve && cnt > K) ? sd * sd * ss / (double)(cnt - K) : qnan;
                if (a.nobs_reg) a.nobs_reg[o] = cnt;
            }
        }
    }
}

// Element e of the slice's start factors; n_start = 1: window b0 + s takes rows o - W + 1 .. o of the one path.  Its first S N threads
// also compare every series' visible cells with what its publication lag leaves of the window: fewer means a NaN of the panel itself.
__global__ __launch_bounds__(256) void di_start_kernel(DiArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)a.W * a.r;
    if (e < (size_t)a.S * per) {
        const size_t s = e / per, rem = e % per;
        const size_t row0 = (size_t)(a.origins[a.b0 + s] - a.W + 1) * a.r;
        a.F[e] = a.F_start[a.n_start == 1 ? row0 + rem : (size_t)(a.b0 + s) * per + rem];
    }
    if (!a.missing_ok && e < (size_t)a.S * a.N) {
        const int l = a.lags ? a.lags[e % a.N] : 0;
        if (a.nobs[e] != a.W - l) atomicOr(a.status, 1);
    }
}

// Lane = one (h, i), as rolling_score_kernel: it walks the slice's windows in order, so the sums of (h, i) take their terms in origin
// order whatever the slicing.  Target row o_b + h is scored iff its forecast is finite, it is inside the panel and observed.
__global__ __launch_bounds__(256) void di_score_kernel(DiArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.N, H1 = a.H + 1, T = a.T;
    if (e >= H1 * N) return;
    const int h = e / N, i = e % N;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const size_t out = (size_t)H1 * N;
    const double* __restrict__ fc = a.fc + e;
    const double* __restrict__ fc_ar = a.fc_ar + e;
    const double* __restrict__ fvar = a.fvar + e;
    const double* __restrict__ x = a.x + i;
    const double* __restrict__ mean = a.mean + i;
    const int* __restrict__ org = a.origins + a.b0;
    double* __restrict__ err = a.err ? a.err + e : nullptr;
    double* __restrict__ err_ar = a.err_ar ? a.err_ar + e : nullptr;
    double* __restrict__ err_std = a.err_std ? a.err_std + e : nullptr;
    double se = a.first ? 0.0 : a.sse[e], sa = a.first ? 0.0 : a.sse_ar[e], s0 = a.first ? 0.0 : a.sse0[e];
    int c = a.first ? 0 : a.cnt[e];
    for (int s = 0; s < a.S; ++s) {
        const int tt = org[s] + h;
        const double f = fc[s * out], fa = fc_ar[s * out], v = fvar[s * out], mu = mean[(size_t)s * N];
        double t = qnan;
        if (tt < T) t = x[(size_t)tt * N];
        const bool scored = t == t && fabs(f) <= 1.7976931348623157e308;
        const double d = scored ? t - f : qnan, da = scored ? t - fa : qnan;
        if (err) err[s * out] = d;
        if (err_ar) err_ar[s * out] = da;
        if (err_std) err_std[s * out] = scored ? d / sqrt(v) : qnan;
        if (scored) {
            const double d0 = t - mu;
            se += d * d; sa += da * da; s0 += d0 * d0; ++c;
        }
    }
    a.sse[e] = se; a.sse_ar[e] = sa; a.sse0[e] = s0; a.cnt[e] = c;
    if (a.last) {
        if (a.msfe) a.msfe[e] = c ? se / c : qnan;
        if (a.msfe_ar) a.msfe_ar[e] = c ? sa / c : qnan;
        if (a.msfe0) a.msfe0[e] = c ? s0 / c : qnan;
        if (a.cnt_out) a.cnt_out[e] = c;
    }
}

hipError_t launch_di_start(const DiArgs& a, hipStream_t s) {
    const size_t nF = (size_t)a.S * a.W * a.r, nN = (size_t)a.S * a.N, n = nF > nN ? nF : nN;
    if (a.S < 1 || (n + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(di_start_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int R>
static hipError_t launch_di_regress_r(const DiArgs& a, hipStream_t s) {
    const size_t lds = di_lds_doubles(a.W, a.r, a.nb, R) * sizeof(double);
    const int nblk = (a.N + a.nb - 1) / a.nb;
    if (a.nb < 1 || a.nb > kDiSeries || lds > kDiLdsMax || a.K > R || a.S < 1 || nblk > 65535) return hipErrorInvalidValue;
    static LdsOptIn attr_done;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&di_regress_kernel<R>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDiLdsMax);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipLaunchKernelGGL((di_regress_kernel<R>), dim3((unsigned)a.S, (unsigned)nblk), dim3(kDiThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_di_regress(int Rpad, const DiArgs& a, hipStream_t s) {
    switch (Rpad) {
        case 2: return launch_di_regress_r<2>(a, s);
        case 4: return launch_di_regress_r<4>(a, s);
        case 8: return launch_di_regress_r<8>(a, s);
        case 16: return launch_di_regress_r<16>(a, s);
        case 32: return launch_di_regress_r<32>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_di_score(const DiArgs& a, hipStream_t s) {
    const size_t n = ((size_t)a.H + 1) * a.N;
    if (n > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(di_score_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
