// forecast_ar.hip -- the series side of dfm_forecast_ar_batch (capi.hip): nowcasts and forecasts of the panel from the model with
// AR(q) idiosyncratic terms,  x_it = lam_i' f_t + e_it,  e_it = rho_i1 e_i,t-1 + .. + rho_iq e_i,t-q + eps_it,  eps ~ N(0, sig2_i).
//
// The AR pass (on the panel with H all-missing rows appended) has left the smoothed / forecast moments f_t, P_t of the n = T + H - q
// output rows (panel rows q .. T + H - 1).  Per series the residuals u_it = x_it - lam_i' f_t of the observed cells are exact
// observations of e_it, the q terms before output row 0 are N(0, v0_i I), and the two kernels here give E, Var[e_it | u_i.] on
// every missing and horizon cell, fused with the cell formulas of forecast_fill_kernel (forecast.hip).  B N independent recursions
// of a q-wide state a_t = (e_t, .., e_{t-q+1}): ONE LANE PER SERIES, a workgroup per (replicate, series block) that walks the rows in
// lockstep -- adjacent lanes are adjacent series, a row of the panel is one coalesced read; lam_i, rho_i, sig2_i and all q x q
// algebra in registers; the chunk's f_t / P_t rows staged in LDS and read as broadcasts.  "Observed" is a select, never a branch
// around the step; the only branch is wave-uniform (no lane of the wave has a message to join).
//
//   forecast_ar_back_kernel   rows n-1 .. 0: the message m_t(a_t) ~ exp(-a' Om_t a / 2 + eta_t' a) of the residuals AFTER t, zero
//     behind the last row.  t observed: a_t = (u_t, a_{t-1}[:q-1]) and the density of u_t given a_{t-1} joins, Om_{t-1} =
//     shift(Om_t[1:,1:]) + rho rho' / sig2, eta_{t-1} = shift(eta_t[1:] - Om_t[1:,0] u_t) + rho u_t / sig2.  t missing: e_t = rho' a_{t-1}
//     + eps is integrated out, M = Om_t - Om_t e0 e0' Om_t / (Om_00 + 1 / sig2) (the denominator is >= 1 / sig2 > 0), Om_{t-1} = F' M F,
//     eta_{t-1} = F' (eta_t - Om_t e0 eta_0 / (..)), F = [rho'; I 0].  (The same step as the Schur complement of c c' / sig2 +
//     pad(Om_t), c = (1, -rho), on its first coordinate, but as a downdate and products: that difference of O(1 / sig2) terms left
//     an absolute error of 1e-16 / sig2 in a message that has decayed to 1e-15.)  Om_t, eta_t are stored only where cell t
//     is missing AND a later cell of the series is observed (horizon and trailing-edge cells have zero messages and store nothing);
//     `last` gets the series' last observed row (-1: none), which tells the forward kernel where messages exist.
//   forecast_ar_fwd_kernel    rows 0 .. n-1: Kalman filter of a_t -- predict, then the exact-observation update k = P[:,0] / P_00
//     (P_00 >= sig2) -- and, on a missing cell, the message joined to the predicted moments: Om = L D L' (unit lower L, D >= 0; a
//     pivot below 2^-44 of its diagonal entry is rounding noise of a rank-deficient message and drops out), eta = L z, so the
//     message is q pseudo-observations w_j' a (w_j = column j of L) of precision d_j, joined one rank-one update at a time: gain
//     P w_j / (1 + d_j w_j' P w_j).  Every denominator is >= 1 whatever P is -- exact observations leave P singular -- and the result
//     is ((I + P Om)^-1 (a + P eta))_0, ((I + P Om)^-1 P)_00.  The same step writes xhat, xvar, common, idio.
//
// Messages: q + q (q + 1) / 2 doubles per cell, component-major -- msg[((b' NC + c) n + t) N + i], b' the replicate inside the
// slice -- so the lanes' stores of one component at one row are contiguous.  capi.hip slices the replicates over the buffer.
#include "dfm_fcar.h"

namespace dfm {

constexpr size_t kFcArLds = 48 * 1024;
constexpr double kFcArPivotTol = 0x1p-44;   // a pivot of the message's L D L' below this share of its diagonal entry is rounding noise

template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void forecast_ar_back_kernel(FcArArgs a) {
    constexpr int NC = Q + Q * (Q + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = a.n, N = a.N, r = a.r, tid = threadIdx.x;
    const int s = (int)(blockIdx.x % (unsigned)a.geo.nsblk);
    const size_t bl = blockIdx.x / (unsigned)a.geo.nsblk, b = (size_t)a.b0 + bl;
    FcArSeries<Q, RB> se;
    se.load(a, b, cell_lane<1>(a.geo, tid, s, N));
    const double inv = 1.0 / se.sig2;
    double Om[Q][Q], eta[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        eta[i] = 0.0;
#pragma unroll
        for (int j = 0; j < Q; ++j) Om[i][j] = 0.0;
    }
    bool seen = false;
    int last = -1;
    const double* xcol = a.panel + (b * (size_t)(n + Q) + Q) * N + se.i;   // output row t of the lane's series: xcol[t N]
    double* mcol = a.msg + bl * NC * (size_t)n * N + se.i;                  // component c at row t: mcol[(c n + t) N]
    double xn = xcol[(size_t)(n - 1) * N];
    for (int ck = a.geo.nchunk - 1; ck >= 0; --ck) {
        const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
        __syncthreads();
        cell_stage(sm, a.f + (b * n + t0) * r, (t1 - t0) * r);
        __syncthreads();
        for (int t = t1 - 1; t >= t0; --t) {
            const double x = xn;
            if (t > 0) xn = xcol[(size_t)(t - 1) * N];                       // one row ahead, in flight during this row's algebra
            const bool obs = x == x;
            const double u = obs ? x - se.lam.dot(0, sm + (size_t)(t - t0) * r, r) : 0.0;
            if (se.live && !obs && seen) {
#pragma unroll
                for (int i = 0; i < Q; ++i) mcol[((size_t)i * n + t) * N] = eta[i];
#pragma unroll
                for (int i = 0; i < Q; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) mcol[((size_t)(Q + i * (i + 1) / 2 + j) * n + t) * N] = Om[i][j];
            }
            last = (obs && last < 0) ? t : last;
            seen = seen || obs;
            // observed: a_t = (u_t, a_{t-1}[:q-1]) and the density of u_t given a_{t-1} joins.  missing: e_t = rho' a_{t-1} + eps is
            // integrated out -- M = Om - Om e0 e0' Om / (Om_00 + 1 / sig2), then F' M F with F = [rho'; I 0].
            const double sc = 1.0 / (Om[0][0] + inv), e0s = eta[0] * sc;
            double M[Q][Q], h[Q], MF[Q][Q], On[Q][Q], en[Q];
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                h[k] = eta[k] - Om[k][0] * e0s;
#pragma unroll
                for (int l = 0; l < Q; ++l) M[k][l] = Om[k][l] - Om[k][0] * Om[0][l] * sc;
            }
#pragma unroll
            for (int k = 0; k < Q; ++k)
#pragma unroll
                for (int j = 0; j < Q; ++j) MF[k][j] = M[k][0] * se.rho[j] + (j + 1 < Q ? M[k][j + 1] : 0.0);
            const double ui = u * inv;
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                const double eo = (i + 1 < Q ? eta[i + 1] - Om[i + 1][0] * u : 0.0) + se.rho[i] * ui;
                const double em = se.rho[i] * h[0] + (i + 1 < Q ? h[i + 1] : 0.0);
                en[i] = obs ? eo : em;
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const double oo = (i + 1 < Q ? Om[i + 1][j + 1] : 0.0) + se.rho[i] * se.rho[j] * inv;
                    const double om = se.rho[i] * MF[0][j] + (i + 1 < Q ? MF[i + 1][j] : 0.0);
                    On[i][j] = On[j][i] = obs ? oo : om;
                }
            }
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                eta[i] = seen ? en[i] : 0.0;
#pragma unroll
                for (int j = 0; j < Q; ++j) Om[i][j] = seen ? On[i][j] : 0.0;
            }
        }
    }
    if (se.live) a.last[bl * N + se.i] = last;
}

// DRAW (simsmooth_ar_fwd_kernel; dfm_simsmooth_ar_batch): the same filter on the difference panel D = X - x+ of pass replicate
// j = j0 + bl, which is not read but formed again -- the lane re-runs the e+ recursion of simsmooth_ar_diff_kernel from its counters
// (SsArIdio) on the staged f+ rows -- with a.f the smoothed mean g of D; the cell written is the draw, x_draw = mean + sd (lam' (f+ + g)
// + e+ + ehat*) off the observed cells.  Parameters are those of replicate j / D, f / msg / last the slice's.
template <int Q, int RB, bool DRAW>
__device__ __forceinline__ void fc_ar_fwd(const FcArArgs& a, const SsArDraw* dr) {
    constexpr int NC = Q + Q * (Q + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = a.n, N = a.N, r = a.r, np = r * (r + 1) / 2, tid = threadIdx.x;
    const int s = (int)(blockIdx.x % (unsigned)a.geo.nsblk);
    const size_t bl = blockIdx.x / (unsigned)a.geo.nsblk;
    const size_t j = DRAW ? (size_t)dr->j0 + bl : 0;                             // pass replicate (DRAW)
    const size_t b = DRAW ? j / (size_t)dr->D : (size_t)a.b0 + bl;               // the parameters' replicate
    const size_t bf = DRAW ? bl : b;                                              // the replicate of the f / P rows
    const bool wantVar = !DRAW && a.xvar != nullptr, scale = a.mean != nullptr;
    double* sf = sm;
    double* sP = sm + (size_t)a.geo.RC * r;                                       // (DRAW: the f+ rows)
    FcArSeries<Q, RB> se;
    se.load(a, b, cell_lane<1>(a.geo, tid, s, N));
    const size_t bi = b * N + se.i;
    const double mu = scale ? a.mean[bi] : 0.0, sd = scale ? a.sd[bi] : 1.0;
    const int last = a.last[bl * N + se.i];
    SsArIdio<Q, RB> gen;
    if constexpr (DRAW) {
        double* sz = sm + (size_t)a.geo.RC * 2 * r;
        const uint64_t key = ssar_key(dr->seed, dr->first_draw, (int)(j % (size_t)dr->D));
        ssar_stage_z(*dr, b, key, Q * r, sz, sz + 32);
        gen.start(a, *dr, se, b, key, sz, s * a.geo.NPB);
    }
    double av[Q], P[Q][Q];
    {
        const double v0 = a.v0 ? a.v0[bi] : se.sig2;
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            av[i] = 0.0;
#pragma unroll
            for (int j = 0; j < Q; ++j) P[i][j] = i == j ? v0 : 0.0;
        }
    }
    // output row t of the lane's series: xcol[t N] for t < nx (DRAW: the caller's T-row panel, NaN behind it)
    const double* xcol = DRAW ? dr->X + (b * (size_t)dr->T + Q) * N + se.i : a.panel + (b * (size_t)(n + Q) + Q) * N + se.i;
    const int nx = DRAW ? dr->T - Q : n;
    const double* mcol = a.msg + bl * NC * (size_t)n * N + se.i;
    double xn = xcol[0];
    for (int ck = 0; ck < a.geo.nchunk; ++ck) {
        const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
        __syncthreads();
        cell_stage(sf, a.f + (bf * n + t0) * r, (t1 - t0) * r);
        if (wantVar) cell_stage(sP, a.P + (bf * n + t0) * np, (t1 - t0) * np);
        if constexpr (DRAW) cell_stage(sP, dr->fplus + (j * n + t0) * r, (t1 - t0) * r);
        __syncthreads();
        for (int t = t0; t < t1; ++t) {
            const double x = xn;
            if (t + 1 < nx) xn = xcol[(size_t)(t + 1) * N];
            else if constexpr (DRAW) xn = __longlong_as_double(0x7FF8000000000000ll);
            const bool obs = x == x;
            const bool need = !obs && t < last;
            // the message of the rows behind t, where there is one
            double Om[Q][Q], eta[Q];
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                eta[i] = need ? mcol[((size_t)i * n + t) * N] : 0.0;
#pragma unroll
                for (int j = 0; j <= i; ++j) Om[i][j] = need ? mcol[((size_t)(Q + i * (i + 1) / 2 + j) * n + t) * N] : 0.0;
            }
            const double m = se.lam.dot(0, sf + (size_t)(t - t0) * r, r);
            double qf = 0.0;
            if (wantVar) {
                const double* Pt = sP + (size_t)(t - t0) * np;
                DFM_CELL_QUAD(qf, se.lam.l[0], Pt, RB, r)
            }
            double mp = 0.0, ep = 0.0;
            if constexpr (DRAW) {
                mp = se.lam.dot(0, sP + (size_t)(t - t0) * r, r);
                ep = gen.step(se, t);
            }
            const double u = obs ? (DRAW ? x - (mp + ep) : x) - m : 0.0;
            // predict
            double rP[Q], an[Q], Pn[Q][Q];
            an[0] = 0.0;
            Pn[0][0] = se.sig2;
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                rP[j] = 0.0;
#pragma unroll
                for (int l = 0; l < Q; ++l) rP[j] = fma(se.rho[l], P[l][j], rP[j]);
            }
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                an[0] = fma(se.rho[j], av[j], an[0]);
                Pn[0][0] = fma(rP[j], se.rho[j], Pn[0][0]);
            }
#pragma unroll
            for (int i = 1; i < Q; ++i) {
                an[i] = av[i - 1];
                Pn[0][i] = Pn[i][0] = rP[i - 1];
#pragma unroll
                for (int j = 1; j < Q; ++j) Pn[i][j] = P[i - 1][j - 1];
            }
            // missing cell: join the message (wave-uniform branch; without a message the answer is the predicted moment itself)
            double eh = an[0], V = Pn[0][0];
            if (__any(need)) {
                double L[Q][Q], d[Q], z[Q];
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    double piv = Om[j][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k] * d[k];
                    const bool ok = piv > kFcArPivotTol * Om[j][j];
                    d[j] = ok ? piv : 0.0;
                    const double ip = ok ? 1.0 / piv : 0.0;
                    L[j][j] = 1.0;
#pragma unroll
                    for (int i = j + 1; i < Q; ++i) {
                        double v = Om[i][j];
#pragma unroll
                        for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * d[k];
                        L[i][j] = v * ip;
                    }
                }
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    z[j] = eta[j];
#pragma unroll
                    for (int k = 0; k < j; ++k) z[j] -= L[j][k] * z[k];
                }
                double am[Q], Pm[Q][Q];
#pragma unroll
                for (int i = 0; i < Q; ++i) {
                    am[i] = an[i];
#pragma unroll
                    for (int j = 0; j < Q; ++j) Pm[i][j] = Pn[i][j];
                }
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    double Pw[Q], wPw = 0.0, wa = 0.0;                       // w = L[., j]: zero above row j
#pragma unroll
                    for (int i = 0; i < Q; ++i) {
                        Pw[i] = 0.0;
#pragma unroll
                        for (int k = j; k < Q; ++k) Pw[i] = fma(Pm[i][k], L[k][j], Pw[i]);
                    }
#pragma unroll
                    for (int k = j; k < Q; ++k) {
                        wPw = fma(L[k][j], Pw[k], wPw);
                        wa = fma(L[k][j], am[k], wa);
                    }
                    const double den = 1.0 / (1.0 + d[j] * wPw);
                    const double ga = (z[j] - d[j] * wa) * den, gp = d[j] * den;
#pragma unroll
                    for (int i = 0; i < Q; ++i) {
                        am[i] = fma(Pw[i], ga, am[i]);
#pragma unroll
                        for (int k = 0; k < Q; ++k) Pm[i][k] -= Pw[i] * Pw[k] * gp;
                    }
                }
                eh = am[0];
                V = Pm[0][0];
            }
            // observed cell: the exact-observation update (row and column 0 of P become exact zeros)
            {
                const double ip = 1.0 / Pn[0][0], e0 = u - an[0];
                double k[Q];
#pragma unroll
                for (int i = 0; i < Q; ++i) k[i] = Pn[i][0] * ip;
#pragma unroll
                for (int i = 0; i < Q; ++i) {
                    const double ao = i == 0 ? u : fma(k[i], e0, an[i]);
                    av[i] = obs ? ao : an[i];
#pragma unroll
                    for (int j = 0; j < Q; ++j) {
                        const double Po = (i == 0 || j == 0) ? 0.0 : Pn[i][j] - k[i] * Pn[0][j];
                        P[i][j] = obs ? Po : Pn[i][j];
                    }
                }
            }
            if constexpr (DRAW) {
                if (se.live) {
                    const double v = obs ? x : (mp + m) + (ep + eh);
                    const double xd[1] = {scale ? mu + sd * v : v};
                    cell_st<1>(dr->x_draw + (j * n + t) * N + se.i, xd);
                }
            } else if (se.live) {
                const double cm = scale ? mu + sd * m : m;
                const double e = obs ? u : eh;
                const double id[1] = {scale ? sd * e : e};
                const double xh[1] = {obs ? (scale ? mu + sd * x : x) : cm + id[0]};
                const size_t o = (b * n + t) * N + se.i;
                cell_st<1>(a.xhat + o, xh);
                if (wantVar) {
                    const double xv[1] = {obs ? 0.0 : (scale ? sd * sd * (qf + V) : qf + V)};
                    cell_st<1>(a.xvar + o, xv);
                }
                if (a.common) {
                    const double cv[1] = {cm};
                    cell_st<1>(a.common + o, cv);
                }
                if (a.idio) cell_st<1>(a.idio + o, id);
            }
        }
    }
}

template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void forecast_ar_fwd_kernel(FcArArgs a) { fc_ar_fwd<Q, RB, false>(a, nullptr); }
template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void simsmooth_ar_fwd_kernel(SsArArgs a) { fc_ar_fwd<Q, RB, true>(a, &a.dr); }

// The kernels on the geometry of series_geometry (dfm_cellgeom.h): a staged row is f_t (backward), f_t and the packed P_t
// (forward), g_t and f+_t with the z+ tail behind the chunk (draw).
enum FcArKind { kFcArBack, kFcArFwd, kFcArDraw };

template <int Q, int RB, class Args>
static hipError_t launch_fc_ar_q(Args a, FcArKind kind, hipStream_t s) {
    const int np = a.r * (a.r + 1) / 2;
    const int row = kind == kFcArBack ? a.r : kind == kFcArDraw ? 2 * a.r : a.r + (a.xvar ? np : 0);
    const size_t tail = kind == kFcArDraw ? kSsArLdsTail * sizeof(double) : 0;
    a.geo = series_geometry(a.N, row, a.n, kFcArLds - tail);
    const size_t blocks = (size_t)a.S * a.geo.nsblk, lds = (size_t)a.geo.RC * row * sizeof(double) + tail;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if constexpr (std::is_same_v<Args, SsArArgs>) {
        hipLaunchKernelGGL((simsmooth_ar_fwd_kernel<Q, RB>), dim3((unsigned)blocks), dim3(a.geo.threads), lds, s, a);
    } else {
        void (*k)(FcArArgs) = forecast_ar_fwd_kernel<Q, RB>;
        if (kind == kFcArBack) k = forecast_ar_back_kernel<Q, RB>;
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(a.geo.threads), lds, s, a);
    }
    return hipGetLastError();
}

template <int Q, class Args>
static hipError_t launch_fc_ar_r(const Args& a, FcArKind kind, hipStream_t s) {
    if (a.r <= 4) return launch_fc_ar_q<Q, 4>(a, kind, s);
    if (a.r <= 8) return launch_fc_ar_q<Q, 8>(a, kind, s);
    return launch_fc_ar_q<Q, 16>(a, kind, s);
}

template <class Args>
static hipError_t launch_fc_ar(const Args& a, FcArKind kind, hipStream_t s) {
    if (a.r < 1 || a.r > 16 || a.n < 1 || a.S < 1) return hipErrorInvalidValue;
    switch (a.q) {
        case 1: return launch_fc_ar_r<1>(a, kind, s);
        case 2: return launch_fc_ar_r<2>(a, kind, s);
        case 3: return launch_fc_ar_r<3>(a, kind, s);
        case 4: return launch_fc_ar_r<4>(a, kind, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_forecast_ar_back(const FcArArgs& a, hipStream_t s) { return launch_fc_ar(a, kFcArBack, s); }
hipError_t launch_forecast_ar_fwd(const FcArArgs& a, hipStream_t s) { return launch_fc_ar(a, kFcArFwd, s); }
hipError_t launch_simsmooth_ar_fwd(const SsArArgs& a, hipStream_t s) { return launch_fc_ar(a, kFcArDraw, s); }

size_t forecast_ar_msg_bytes(int n, int N, int q) {
    return (size_t)(q + q * (q + 1) / 2) * (size_t)n * N * sizeof(double);
}

}  // namespace dfm
