// forecast.hip -- nowcasts and h-step forecasts of the panel from a fitted parametric DFM (dfm_forecast_batch, capi.hip).
//
// Model  x_t = Lam f_t + e_t, e_t ~ N(0, diag R),  f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t.  The smoother pass gives the
// moments of f_t given the observed cells for t < T; past the sample the smoothed moments are the forecast moments:
//   f_{T+h|T} = A f_{T+h-1|T},   P_{T+h|T} = A P_{T+h-1|T} A' + Q          (p = 1: forecast_tail_kernel)
// (p > 1: the companion pass itself runs over H appended all-missing rows, whose smoothed moments are these.)
// forecast_fill_kernel then streams the panel-sized outputs, per cell (b, t, i):
//   common = mean_i + sd_i lam_i' f_t
//   xhat   = mean_i + sd_i x_ti on an observed cell (x_ti itself, bit for bit, without mean / sd), common otherwise
//   xvar   = 0 on an observed cell, sd_i^2 (lam_i' P_t lam_i + R_i) otherwise
// Both products are GEMMs with a small K per replicate (common = F Lam', K = r; lam' P lam against packed P, K = r(r+1)/2).
// At r <= 8 (K = 8 + 36) the VALU does them in the shadow of the stores: one workgroup owns a replicate's chunk of rows and a
// block of series, stages the chunk's f_t / P_t rows in LDS (every lane of a wave reads the same address: a broadcast), keeps its
// series' loadings in registers and writes 16 bytes per lane (two adjacent series) when N is even.
#include "dfm_cell.h"
#include "dfm_kernels.h"

namespace dfm {

constexpr int kFcFillMaxThreads = 512;
constexpr size_t kFcFillLds = 48 * 1024;

// p = 1: the H forecast rows behind the terminal smoothed moments.  One workgroup per replicate, r <= 32: A, P and A P in LDS.
__global__ __launch_bounds__(256) void forecast_tail_kernel(FcTailArgs a) {
    __shared__ double sA[32 * 32], sP[32 * 32], sM[32 * 32], sf[32], sf2[32];
    const int r = a.r, T = a.T, H = a.H, np = r * (r + 1) / 2, tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const bool wantP = a.Pt != nullptr;
    for (int e = tid; e < r * r; e += blockDim.x) {
        sA[e] = a.A[b * r * r + e];
        if (wantP) {
            const int i = e / r, j = e % r, hi = i > j ? i : j, lo = i > j ? j : i;
            sP[e] = a.Psm[(b * T + (T - 1)) * np + hi * (hi + 1) / 2 + lo];
        }
    }
    if (tid < r) sf[tid] = a.fsm[(b * T + (T - 1)) * r + tid];
    __syncthreads();
    for (int h = 0; h < H; ++h) {
        if (tid < r) {
            double v = 0.0;
            for (int k = 0; k < r; ++k) v += sA[tid * r + k] * sf[k];
            sf2[tid] = v;
        }
        if (wantP)
            for (int e = tid; e < r * r; e += blockDim.x) {
                const int i = e / r, j = e % r;
                double v = 0.0;
                for (int k = 0; k < r; ++k) v += sA[i * r + k] * sP[k * r + j];
                sM[e] = v;
            }
        __syncthreads();
        if (tid < r) {
            sf[tid] = sf2[tid];
            a.ft[(b * H + h) * r + tid] = sf2[tid];
        }
        if (wantP)
            for (int e = tid; e < np; e += blockDim.x) {
                int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
                while (i * (i + 1) / 2 > e) --i;
                while ((i + 1) * (i + 2) / 2 <= e) ++i;
                const int j = e - i * (i + 1) / 2;
                double vij = a.Q[b * r * r + i * r + j], vji = a.Q[b * r * r + j * r + i];
                for (int k = 0; k < r; ++k) {
                    vij += sM[i * r + k] * sA[j * r + k];
                    vji += sM[j * r + k] * sA[i * r + k];
                }
                const double v = 0.5 * (vij + vji);
                sP[i * r + j] = v;
                sP[j * r + i] = v;
                a.Pt[(b * H + h) * np + e] = v;
            }
        __syncthreads();
    }
}

// p > 1: the panel with H all-missing rows appended, written into the caller's xhat (the companion pass runs on it).  A NaN among
// the T observed rows of a panel declared balanced raises status bit 1, as the pass's own collapse would have.
__global__ __launch_bounds__(256) void forecast_pad_kernel(size_t B, int T, int H, int N, const double* panel, double* out,
                                                           int check_nan, int* status) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t row_n = (size_t)(T + H) * N;
    if (tid >= B * row_n) return;
    const size_t b = tid / row_n, rem = tid % row_n;
    const size_t t = rem / N;
    double v = __builtin_nan("");
    if (t < (size_t)T) {
        v = panel[b * (size_t)T * N + rem];
        if (check_nan && v != v) atomicOr(status, 1);
    }
    out[tid] = v;
}

template <int R, int SP>
__global__ __launch_bounds__(kFcFillMaxThreads) void forecast_fill_kernel(FcFillArgs a) {
    constexpr int NP = R * (R + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int TH = a.T + a.H, tid = threadIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.x, TH);
    const size_t b = ch.outer;
    const int t0 = ch.t0, t1 = ch.t1, nt = t1 - t0;
    double* sf = sm;
    double* sP = sm + (size_t)a.geo.RC * R;
    const bool loadP = a.Ph != nullptr, wantVar = a.xvar != nullptr;
    const bool copy = ch.s == 0 && a.f_out != nullptr;
    // the chunk's factor rows (contiguous in both sources); series block 0 also writes them to the caller's T + H row layout
    for (int e = tid; e < nt * R; e += blockDim.x) {
        const int t = t0 + e / R, k = e % R;
        const double v = t < a.Th ? a.fh[(b * a.Th + t) * R + k] : a.ft[(b * a.H + (t - a.Th)) * R + k];
        sf[e] = v;
        if (copy) a.f_out[(b * TH + t) * R + k] = v;
    }
    if (loadP)
        for (int e = tid; e < nt * NP; e += blockDim.x) {
            const int t = t0 + e / NP, k = e % NP;
            const double v = t < a.Th ? a.Ph[(b * a.Th + t) * NP + k] : a.Pt[(b * a.H + (t - a.Th)) * NP + k];
            sP[e] = v;
            if (copy && a.P_out) a.P_out[(b * TH + t) * NP + k] = v;
        }
    __syncthreads();
    const CellLane ln = cell_lane<SP>(a.geo, tid, ch.s, a.N);
    if (!ln.live) return;
    const int i0 = ln.i0;
    const bool scale = a.mean != nullptr;
    CellLam<SP, R> lam;
    lam.load(a.Lam, b, a.N, i0, R);
    double Rv[SP], mu[SP], sd[SP];
#pragma unroll
    for (int q = 0; q < SP; ++q) {
        const size_t bi = b * a.N + i0 + q;
        Rv[q] = wantVar ? a.R[bi] : 0.0;
        mu[q] = scale ? a.mean[bi] : 0.0;
        sd[q] = scale ? a.sd[bi] : 1.0;
    }
    for (int t = t0 + ln.g; t < t1; t += a.geo.G) {
        const double* f = sf + (size_t)(t - t0) * R;
        const double* P = sP + (size_t)(t - t0) * NP;
        double x[SP];
        if (t < a.T) {
            cell_ld<SP>(a.panel + (b * a.panel_rows + t) * a.N + i0, x);
        } else {
#pragma unroll
            for (int q = 0; q < SP; ++q) x[q] = __builtin_nan("");
        }
        double xh[SP], xv[SP], cm[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) {
            const double m = lam.dot(q, f, R);
            double qf = 0.0;
            if (wantVar) {
                DFM_CELL_QUAD(qf, lam.l[q], P, R, R)
            }
            const bool obs = x[q] == x[q];
            cm[q] = scale ? mu[q] + sd[q] * m : m;
            xh[q] = obs ? (scale ? mu[q] + sd[q] * x[q] : x[q]) : cm[q];
            xv[q] = obs ? 0.0 : (scale ? sd[q] * sd[q] * (qf + Rv[q]) : qf + Rv[q]);
        }
        const size_t o = (b * TH + t) * a.N + i0;
        cell_st<SP>(a.xhat + o, xh);
        if (wantVar) cell_st<SP>(a.xvar + o, xv);
        if (a.common) cell_st<SP>(a.common + o, cm);
    }
}

hipError_t launch_forecast_tail(const FcTailArgs& a, hipStream_t s) {
    if (a.H <= 0) return hipSuccess;
    hipLaunchKernelGGL(forecast_tail_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_forecast_pad(int B, int T, int H, int N, const double* panel, double* out, bool check_nan, int* status,
                               hipStream_t s) {
    const size_t n = (size_t)B * (T + H) * N;
    hipLaunchKernelGGL(forecast_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (size_t)B, T, H, N, panel, out,
                       check_nan ? 1 : 0, status);
    return hipGetLastError();
}

// A lane per SP series; a staged row is f_t and the packed P_t (cell_geometry, dfm_cellgeom.h).
template <int R>
static hipError_t launch_fill_r(FcFillArgs a, hipStream_t s) {
    const int SP = cell_sp(a.N, R, a.panel, a.xhat, a.xvar, a.common);
    a.geo = cell_geometry((a.N + SP - 1) / SP, R + R * (R + 1) / 2, a.T + a.H, kFcFillMaxThreads, kFcFillLds);
    const size_t lds = (size_t)a.geo.RC * (R + R * (R + 1) / 2) * sizeof(double);
    return cell_launch_sp<R>(forecast_fill_kernel<R, 1>, forecast_fill_kernel<R, cell_sp_max(R)>, SP,
                             (size_t)a.B * a.geo.nchunk * a.geo.nsblk, a.geo.threads, lds, s, a);
}

hipError_t launch_forecast_fill(const FcFillArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 32) return hipErrorInvalidValue;
    return dispatch_r_exact(a.r, hipErrorInvalidValue, [&](auto R) { return launch_fill_r<decltype(R)::value>(a, s); });
}

}  // namespace dfm
