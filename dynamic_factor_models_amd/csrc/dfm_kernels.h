// dfm_kernels.h -- host-visible launch interface of the gfx950 kernels (internal to libdfmhip.so).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dfm_cellgeom.h"
#include "dfm_device.h"

namespace dfm {

// The kernel a launcher actually dispatched to, for the per-kernel timing of dfm_profile_* (capi.hip): several launch_*
// functions choose among kernels (cov_kernel | cov_grid_kernel, recursion_kernel | recursion_wave_kernel |
// recursion_pair_kernel, ...), and bench.py's JSON must carry the names rocprofv3 prints.  thread_local: the multi-GPU
// object launches from one host thread per GPU.
extern thread_local const char* t_launched_kernel;
// Environment switches of the library, in two classes.
//   route_env: selects among PRODUCTION kernels that compute the same result to rounding (the one-launch pass or the two-launch
//              pass, one wave or a lane group per replicate, ...): what the test-suite uses to cover every fallback, and tuning
//              knobs (DFM_NUM_CU).  Twelve names: DFM_FORCE_GENERAL, DFM_PASS_FUSED, DFM_PF_WPARK, DFM_NO_CHUNK, DFM_NO_PAIR,
//              DFM_MSTEP_MISS, DFM_TILE_NC, DFM_NUM_CU, DFM_FCAR_MSG_BYTES -- which kernel runs or how a call is sliced, never what it
//              computes -- and DFM_CHUNK_W, DFM_TILE_W, DFM_CHUNK_TOL, which set the warm-up and the boundary tolerance of the
//              time-chunked recursions (a replicate that misses the tolerance is redone sequentially: accuracy knobs).
//   diag_env:  ablations (some produce WRONG results on purpose: stream-only, compute-only, skipped stages), phase stamps, the
//              *_OLD kernels kept for A/B.  Read only by a library built with -DDFM_DIAG (`python -m
//              dynamic_factor_models_amd.build --diag`); the default libdfmhip.so ignores them.
inline const char* route_env(const char* name) { return getenv(name); }
#ifdef DFM_DIAG
inline const char* diag_env(const char* name) { return getenv(name); }
#else
inline const char* diag_env(const char*) { return nullptr; }
#endif

// Non-temporal hint on a kernel's ONE-PASS panel stream (dfm_lds.h dma16_stream: pass_fused.hip, mstep_mfma.hip): on for batches whose panels are
// <= 2 GiB, where part of the pass's working set survives in the 256-MB Infinity Cache between launches (measured gains up to
// B = 4096 at the C2 shape, a loss at 8192).  DFM_DMA_NT=0 | 1 (diagnostics build) overrides.
inline bool stream_nt_hint(size_t panel_bytes) {
    static const int force = [] { const char* v = diag_env("DFM_DMA_NT"); return v ? (atoi(v) != 0 ? 1 : 0) : -1; }();
    if (force >= 0) return force != 0;
    return panel_bytes <= ((size_t)2 << 30);
}

inline void note_kernel(const char* name) { t_launched_kernel = name; }


// All device arrays below use the PADDED factor dimension Rp (2,4,8,16,32 >= r): parameters are
// embedded by pad_params_kernel (extra states: A = 0, Q = I, P0 = I, mu0 = 0, Lam = 0 -- independent
// unit-variance noise states that no series loads on; every determinant / quadratic form they add
// is exactly 0), so kernels are instantiated for a handful of sizes only.
constexpr int kSsumSlots = 16;

struct CollapseArgs {
    int B, T, N;
    int b0;               // collapse_dma only: first replicate of this launch (sub-batch pipelining)
    const double* panel;  // [B][T][N]
    const double* Lam;    // [B][N][Rp]
    const double* Rv;     // [B][N]
    double* bcol;         // [B][T][Rp]
    double* scol;         // [B][T]
    int* nobs;            // [B][T]
    double* ldrow;        // [B][T]      (written only where nobs < N)
    double* Ct;           // [B][T][Rp(Rp+1)/2] packed, or nullptr (written only where nobs < N)
    double* Cfull;        // [B][Rp][Rp]
    double* ldfull;       // [B]
    int* status;          // bit0: NaN met while Ct == nullptr
    double* ssum;         // [B][kSsumSlots]  balanced path only: sum_t s_t of each wave's periods (slots 0 .. nseg-1)
    const void* fuse_cov; // collapse_mfma only, HOST pointer read by the launcher (not by the kernel): FastArgs of the pass whose
                          // covariance workgroups + P_smooth fill ride at the front of this launch, or null
    int wpr;              // collapse_mfma only: waves (period segments) per replicate (0 = 4); nseg = wpr <= kSsumSlots
    int bst;              // collapse_wide2 (Rp = 32, balanced) only: > 0 = doubles between the rows of bcol (a multiple of 8, >= the state
                          // width: the padding components of b_t are exact zeros nobody needs); 0 = Rp
    int ct_r;             // ct_miss_wide2 only: > 0 = Ct rows are the packed LEADING ct_r x ct_r block (ct_r (ct_r + 1) / 2 doubles; the
                          // padding of the state carries no loadings, its entries equal Cfull's) -- what recursion_tile_kernel reads;
                          // 0 = the full Rp (Rp + 1) / 2 layout of the other recursion kernels
    double* obs_chunk;    // collapse_miss only (table mode): RecursionArgs::chunk_rows -- one 112-byte row per period: b_t (8), s_t,
                          // n_t log 2 pi + sum log R, the period's NaN bit mask (4 x 64 bits) -- written INSTEAD of bcol .. ldrow and C_t
    int kreal;            // collapse_kernel<32>: > 0 = the loadings' columns kreal .. 31 are zero padding (companion states narrower than their
                          // layout): their sums are written as zeros, not formed; 0 = all columns
    double* obs_table;    // ... and RecursionArgs::chunk_obs, the pass's observation table [B][obs_L][23][64] double2 (chunk-major, period
    int obs_L;            // t = obs_L lane + slot), which the workgroup fills from those rows when its stream is done (dfm_ctbuild.h)
    int lam_w;            // collapse_miss only: > 0 = Lam is [B][N][lam_w], lam_w < 8 (r <= 4 on the 8-wide state: columns lam_w .. 7 of the
                          // kernel's tables are zeros -- b_t, C_t come out 8 wide with a zero padding block); 0 = 8
};

struct RecursionArgs {
    int B, T, N, r;       // r = caller's factor count (<= Rp) for the outputs
    const double* A;      // [B][Rp][Rp]
    const double* Q;      // [B][Rp][Rp]
    const double* mu0;    // [B][Rp]
    const double* P0;     // [B][Rp][Rp]
    const double* bcol; const double* scol; const int* nobs; const double* ldrow;
    const double* Ct; const double* Cfull; const double* ldfull;
    // scratch
    double* ZJtab;        // [B][T+1][2][Rp][Rp]   Z_e, J_e of every distinct covariance step
    double* wtab;         // [B][T][Rp]
    int* eidx;            // [B][T]
    // outputs (caller's r): f_smooth [B][T][r], P_smooth [B][T][r(r+1)/2] or null, loglik [B]
    double* f_smooth; double* P_smooth; double* loglik;
    // EM sufficient statistics (null for a plain pass): S11,S10,S00 [B][Rp][Rp]; f0s [B][Rp]; P0s [B][Rp][Rp]
    double* S11; double* S10; double* S00; double* f0s; double* P0s;
    int* ncov;            // [B] number of distinct covariance steps (diagnostic), or null
    // EM epilogue (all null / 0 for a plain pass): new transition parameters written IN PLACE
    // (each replicate's A, Q, mu0, P0 are read only in the kernel prologue of the same group)
    double* A_out; double* Q_out; double* mu0_out; double* P0_out;   // padded [B][Rp][Rp] / [B][Rp]
    double* S11inv;       // [B][Rp][Rp]  (S11)^-1 for the loadings step
    int* active;          // [B] or null: replicate still iterating (read, then updated by the kernel)
    int* iters;           // [B] or null
    double* ll_path;      // [B][max_iter] or null
    int k, max_iter;      // current EM iteration
    double tol;
    // covariance-form recursion (Q may be singular) and companion states (recursion.hip, COV = true); all 0 otherwise
    int cov;              // 1: covariance-form forward sweep
    int Rc;               // padded width of bcol / Ct / Cfull when narrower than the state (0: same as the state)
    int rl;               // > 0: observation loads on the first rl state components only; outputs / S11 in the Rc layout
    int kdim;             // > 0: companion state of width kdim = rl * p: the M-step keeps the shift rows and Q's zero blocks
    int wave;             // 1: one wave per replicate where recursion_wave.hip supports the shape (Rp = 8, information form)
    int kb;               // > 0 with kdim: block size r of the companion state when the observation loads on MORE than the first
                          // block (AR idiosyncratic terms: rl = 0); 0: the block is rl
    int pair_bmax;        // Rp = 8, information form: batches up to this size run as a covariance wave + a mean wave per replicate
                          // (recursion_pair.hip); 0: never
    int ka;               // > 0 with kdim: only the first ka = r p columns of the transition rows are free (a VAR(p) inside a
                          // state that carries m > p lags); 0: all kdim columns
    int qsing;            // 1 with kdim: the caller passed DFM_F_SINGULAR_Q -- the r x r innovation block itself may be rank deficient:
                          // keep the kernels that never invert it (recursion_comp.hip inverts the block and is skipped)
    int ct_r;             // > 0: Ct holds the packed leading ct_r x ct_r block per period (see CollapseArgs::ct_r; recursion_tile only)
    int rstate;           // the model's state width before padding (0: unknown) -- recursion_tile.hip executes ceil(rstate / 4) of
                          // the 8 block pivots / k-steps of a 32-wide state and keeps the mean vectors in (padding) column 31
    // time-chunked recursion (recursion_chunk.hip; Rp = 8, information form): a replicate's T periods as 64 chunks of chunk_L, one per
    // lane of a wave, each lane warmed up over chunk_W periods; scratch owned by the handle's workspace
    double* chunk_scr;    // [B][chunk_L][22][64][2]  -Z_t (36 packed) and w_t (8) of every period, chunk-major (lane = chunk)
    double* chunk_cst;    // [B][320]  per-replicate constants (K, K', Q^-1 + Phi, Phi, Om_0 + Phi, xi_0, log-det and quadratic constants)
    double* chunk_term;   // [B][96]   P_T|T (36), f_T|T (8), P_0|T (36), f_0|T (8)
    double* chunk_obs;    // [B][chunk_L][23][64][2]  the observation table, chunk-major (period t = chunk_L lane + slot): C_t (36 packed), b_t (8),
                          // s_t, n_t log 2 pi + log det R_t of EVERY slot of all 64 lanes (benign rows beyond the sample)
    int chunk_obs_ready;  // 1: collapse_miss_kernel wrote the table itself (its table mode); 0: launch_recursion_chunk gathers the collapse
                          // kernels' per-period arrays
    int* chunk_fail;      // [B]       1: a chunk boundary did not agree to chunk_tol -- the replicate belongs to the sequential kernel
    int* chunk_skip;      // [B] or null: persists between the iterations of an EM run (k = 0 clears it) -- consecutive failures of the replicate's
                          // boundary check; from three on the chunked kernel leaves it to the sequential one at once (retried every 8th iteration)
    const int* only_if;   // [B] or null: the sequential kernels (recursion_wave / recursion_pair) run replicate b only if only_if[b] != 0
    int chunk_L, chunk_W;
    double chunk_tol;
    // time-chunked recursion_tile (Rp = 32, information form): tile_nc chunks of tile_lc periods per replicate, one workgroup each,
    // warmed up over tile_w periods; boundaries checked to chunk_tol, chunk_fail / only_if as above
    double* tile_scr;     // [B][tile_nc][...]  private tables of the warm-up periods, boundary states, parts of the sums (recursion_tile.hip)
    size_t tile_scr_bytes;
    int tile_nc;          // in: 0 = automatic, 1 = never, n = that many; the launcher fills in the count it uses
    int tile_lc, tile_w;
    int num_cu;
};

// Rp = 8, information form, plain factor model (no companion state): the time-chunked recursion
bool recursion_chunk_supported(int Rpad, const RecursionArgs& a);
size_t recursion_chunk_scratch_bytes(int B, int T);          // chunk_scr
size_t recursion_chunk_obs_bytes(int B, int T);              // chunk_obs
size_t recursion_chunk_rows_bytes(int B, int T);             // chunk_rows
int recursion_chunk_len(int T);                              // chunk_L for a sample of T periods
hipError_t launch_recursion_chunk(const RecursionArgs& a, hipStream_t s);
hipError_t launch_chunk_unbridge(const RecursionArgs& a, hipStream_t s);
bool recursion_wave8_fits(int T);
hipError_t launch_recursion_wave8_fallback(const RecursionArgs& a, hipStream_t s);

// Rp = 32, 17 <= rstate <= 31, information form, plain factor model: four waves per replicate, matrices as MFMA accumulator
// tiles, 4 x 4 block-pivot sweep inverse (recursion_tile.hip)
bool recursion_tile_supported(int Rpad, const RecursionArgs& a);
hipError_t launch_recursion_tile(const RecursionArgs& a, hipStream_t s);
int recursion_tile_chunks(const RecursionArgs& a, int* lc_out, int* w_out);   // chunks per replicate the launch will use (1: sequential)
bool recursion_tile_writes_fail(const RecursionArgs& a);      // the launch checks chunk boundaries / writes chunk_fail (recursion_tile1_kernel or chunks > 1)
size_t recursion_tile_scratch_bytes(int B, int T);            // tile_scr

struct MstepArgs {
    int B, T, N, r;
    const double* panel;  // [B][T][N]
    const double* fsm;    // [B][T][Rp]            smoothed means (padded layout)
    const double* Psm;    // [B][T][Rp(Rp+1)/2]    smoothed covariances, packed
    const double* S11;    // [B][Rp][Rp]
    const double* S11inv; // [B][Rp][Rp]
    double* Dmiss;        // [B][N][Rp(Rp+1)/2] zeroed scratch, or null (register accumulators)
    const int* active;    // [B] or null
    double* Lam_out;      // [B][N][lam_stride]
    double* R_out;        // [B][N]
    int lam_stride;
    int min_cells;        // mstep_lam: a series with fewer observed cells keeps its parameters (0 = 1)
};

// balanced panels at Rp = 16 | 32 (even N): the loadings step as a second streaming pass on the matrix pipe (mstep_wide.hip);
// ws = mstep_wide_workspace bytes; r = the caller's factor count
bool mstep_wide_supported(int Rpad, int N);
size_t mstep_wide_workspace(int B, int N, int Rpad);
hipError_t launch_mstep_wide(const MstepArgs& a, double* ws, int Rpad, int r, int num_cu, hipStream_t s);
// panels with missing cells, Rp = 8 | 16 | 32 (even N): D_i = sum over the series' missing periods of vec(E[f f']) and Sxf_i as one
// product per replicate on the matrix pipe, then a per-series Cholesky solve (mstep_miss.hip); r = the loadings' factor count
bool mstep_miss_supported(int Rpad, int r, int N);
size_t mstep_miss_workspace(int B, int T, int N, int Rpad, int r);
hipError_t launch_mstep_miss(const MstepArgs& a, double* ws, int Rpad, int r, int num_cu, hipStream_t s);
hipError_t launch_collapse(int Rpad, const CollapseArgs& a, hipStream_t s);
// the same contract on the LDS-DMA ring + matrix pipe (collapse_miss.hip): Rp = 8, the shapes of the MFMA collapse
bool collapse_miss_supported(int Rpad, int N);
hipError_t launch_collapse_miss(const CollapseArgs& a, int num_cu, hipStream_t s);
// Rp = 16, covariance form, observation on the first <= 4 state components (VAR(p) factor dynamics): one wave per replicate on the
// matrix pipe, rank-4 updates and the Bryson-Frazier smoother instead of 16 x 16 inversions (recursion_mbf16.hip)
bool recursion_mbf16_supported(int Rpad, const RecursionArgs& a);
hipError_t launch_recursion_mbf16(const RecursionArgs& a, hipStream_t s);
hipError_t launch_cov_epilogue(int Rpad, const RecursionArgs& a, hipStream_t s);
// companion states in blocks of 4 (VAR(p) factor dynamics at r = 4, AR idiosyncratic terms at r = 4): information form as a block
// elimination, one wave per replicate on matrix-pipe tiles, 4 x 4 pivots only (recursion_comp.hip)
bool recursion_comp_supported(int Rpad, const RecursionArgs& a);
hipError_t launch_recursion_comp(int Rpad, const RecursionArgs& a, hipStream_t s);
bool recursion_wave_supported(int Rpad, const RecursionArgs& a);
hipError_t launch_recursion_wave(const RecursionArgs& a, hipStream_t s, int Rpad);
// Rp = 8, information form, B <= ~1.5 x the SIMD count: the replicate split over a covariance wave and a mean wave (recursion_pair.hip)
bool recursion_pair_supported(const RecursionArgs& a);
hipError_t launch_recursion_pair(const RecursionArgs& a, hipStream_t s);
int collapse_max_n(int Rpad);
// balanced panels (no NaN), even N: LDS-DMA streaming collapse (writes bcol, scol only) + Gram kernel
bool collapse_dma_supported(int Rpad, int N);
hipError_t launch_collapse_dma(int Rpad, const CollapseArgs& a, hipStream_t s, int variant);
hipError_t launch_gram(int Rpad, const CollapseArgs& a, hipStream_t s);
// same contract as launch_collapse_dma, contraction on the fp64 matrix pipe (collapse_mfma.hip)
bool collapse_mfma_supported(int Rpad, int N);
bool collapse_mfma_fuses_cov(int Rpad, int N);   // launch_collapse_mfma honours CollapseArgs::fuse_cov for this shape
hipError_t launch_collapse_mfma(int Rpad, const CollapseArgs& a, hipStream_t s, int variant);
// cross-sections beyond the register tilings above (collapse_wide.hip): one wave per 16-period tile, weights
// re-read from L2 per tile; per-tile partial sums of s_t go to scol[b][tile]
bool collapse_wide_supported(int Rpad, int N);
int collapse_wide_tiles(int T);
hipError_t launch_collapse_wide(int Rpad, const CollapseArgs& a, hipStream_t s);
hipError_t launch_gram_wide(int Rpad, const CollapseArgs& a, hipStream_t s);
// Rp = 32 on the LDS-DMA path (collapse_wide2.hip): launch_wide_prep writes W = lam / R ([B][N][32] workspace), Cfull and
// ldfull (the Gram kernel's outputs); launch_collapse_wide2 then streams the panel (partials of sum_t s_t: scol[b][tile])
bool collapse_wide2_supported(int Rpad, int N);
int collapse_wide2_tiles(int T);
size_t collapse_wide2_ws_bytes(int B, int N, int Rpad);    // W [B][N][Rp] | 1 / R, log R [B][N padded to 32] | tile queue counters
// r > 0: the caller's factor count (skips the W table when launch_collapse_wide2 will not read it); V: [B][N][32] lam / sqrt(R) for
// launch_ct_miss_wide, or null
hipError_t launch_wide_prep(const CollapseArgs& a, double* ws, int Rpad, hipStream_t s, int r = 0, double* V = nullptr);
hipError_t launch_collapse_wide2(const CollapseArgs& a, double* ws, int Rpad, int r, int num_cu, hipStream_t s);
// a.nobs != nullptr selects the variant for panels with missing cells (per-period scol / nobs / ldrow); their C_t:
bool ct_miss_wide_compact_ok(int N, int ct_r);   // compact C_t rows (CollapseArgs::ct_r) are available for this cross-section
hipError_t launch_ct_miss_wide(const CollapseArgs& a, double* ws, int r, hipStream_t s, const double* V = nullptr);   // r: the caller's factor count; V: launch_wide_prep's
bool gram_supported(int Rpad, int N);       // launch_gram's register tilings
hipError_t launch_recursion(int Rpad, const RecursionArgs& a, hipStream_t s);
hipError_t launch_mstep_lam(int Rpad, const MstepArgs& a, hipStream_t s);
bool mstep_needs_dmiss(int Rpad, int N);
// balanced panels: the same M-step with the contraction on the matrix pipe (mstep_mfma.hip); workspace for the
// per-segment partial sums
bool mstep_mfma_supported(int Rpad, int N);
size_t mstep_mfma_workspace(int B, int N, int Rpad, int wpr);
struct EmUpdArgs;
// ua != nullptr (Rp <= 8): the transition M-step of every replicate runs as extra workgroups at the front of the streaming launch
// (dfm_em_update.h: em_update_wave) instead of as em_update_kernel's launch of the same function
hipError_t launch_mstep_mfma(int Rpad, const MstepArgs& a, int wpr, double* workspace, hipStream_t s, const EmUpdArgs* ua = nullptr);

// Series block of the ECM iteration with AR(q) idiosyncratic terms (mstep_ar.hip): loadings, AR coefficients and innovation
// variances from the smoothed moments of the companion state of the quasi-differenced model.
struct ArMstepArgs {
    int B, T, N, r, q, Rk;      // T: rows of the ORIGINAL panel (the moments cover its rows q .. T-1); Rk: padded state width
    const double* panel;        // [B][T][N], NaN = missing
    const double* zsm;          // [B][T-q][Rk]             smoothed means of z_t = (f_t, .., f_{t-m+1})
    const double* Psm;          // [B][T-q][Rk(Rk+1)/2]     smoothed covariances, packed lower
    const int* active;          // [B] or null
    double* Lam;                // [B][N][r]   in / out
    double* rho;                // [B][N][q]   in / out
    double* sig2;               // [B][N]      in / out
};
bool mstep_ar_supported(int r, int q);
size_t mstep_ar_workspace(int B, int T, int N, int r, int q, int Rk);
// ws: mstep_ar_workspace bytes (ar_moments_kernel + ar_solve_kernel)
hipError_t launch_mstep_ar(const ArMstepArgs& a, double* ws, hipStream_t s);
// Series block of the EM iteration of the mixed-frequency model (mstep_mf.hip): x_it = lam_i' sum_l w_il f_{t-l} + e_it with known
// weights in C <= kMfMaxClasses distinct classes; the series dealt by index into tiles of 16 of one class each.
// (kMfMaxClasses = 8, kMfMaxLags = 5, the row of the table and the grids: dfm_mfgeom.h)
struct MfMstepArgs {
    int B, T, N, r, L, Rk, C;   // Rk: padded state width (r max(p, L) <= Rk)
    int VW;                     // mstep_mf_row_width(r): columns of a class row of the table
    int ntiles;                 // series tiles
    const double* panel;        // [B][T][N], NaN = missing
    const double* zsm;          // [B][T][Rk]             smoothed means of z_t = (f_t, .., f_{t-m+1})
    const double* Psm;          // [B][T][Rk(Rk+1)/2]     smoothed covariances, packed lower
    const int* active;          // [B] or null
    const double* Wc;           // [C][L]      the classes' weights
    const int* tile_class;      // [ntiles]
    const int* tile_series;     // [ntiles][16] series index, -1 = padding
    double* Lam;                // [B][N][r]   in / out
    double* R;                  // [B][N]      in / out
};
bool mstep_mf_supported(int r, int L);
int mstep_mf_row_width(int r);
size_t mstep_mf_workspace(int B, int T, int N, int r, int C);
// LamK [B][N][Rk] = [w_i0 lam_i, .., w_i,L-1 lam_i, 0..] from Lam [B][N][r], W [N][L]
hipError_t launch_mf_loadings(int B, int N, int r, int L, int Rk, const double* Lam, const double* W, double* LamK, hipStream_t s);
// ws: mstep_mf_workspace bytes, the same block for the three launches of an iteration
hipError_t launch_mf_table(const MfMstepArgs& a, double* ws, hipStream_t s);
hipError_t launch_mf_moments(const MfMstepArgs& a, double* ws, hipStream_t s);
hipError_t launch_mf_solve(const MfMstepArgs& a, double* ws, hipStream_t s);
// The solve with fixed loadings (mstep_mf_blocks.hip): free_mask [N][r] bytes, nonzero = estimated; a fixed entry of Lam is not written
hipError_t launch_mf_solve_blocks(const MfMstepArgs& a, const unsigned char* free_mask, double* ws, hipStream_t s);
// V[b][t][tt16] = [vec(E f f' + P) of the leading r states (packed lower), zeros to ntm16 | f_t (Rp columns), zeros] (mstep_miss.hip)
hipError_t launch_mmw_vec(const double* fsm, const double* Psm, const int* active, int B, int T, int r, int Rp, int ntm16, int tt16,
                          double* V, hipStream_t s);

// Parametric model with OBSERVED factors (mstep_obs.hip): x_it = lam_o,i' g_t + lam_u,i' f_t + e_it with g_t
// known regressors.  E-step on the residual panel y = x - Lam_o g; loadings by one joint regression per series on z = (g, f).
struct ObsArgs {
    int B, T, N, ro, ru, Rl;    // Rl: width of the rows of fsm (padded loadings width); Psm rows: Rl (Rl + 1) / 2 packed
    const double* panel;        // [B][T][N], NaN = missing
    const double* G;            // [B][T][ro]  observed factors (no NaN)
    const double* fsm;          // [B][T][Rl]
    const double* Psm;          // [B][T][Rl(Rl+1)/2]
    const int* active;          // [B] or null
    double* Lam;                // [B][N][ro + ru]  observed-factor loadings first   in / out
    double* R;                  // [B][N]                                             in / out
};
bool mstep_obs_supported(int ro, int ru);
hipError_t launch_mstep_obs(const ObsArgs& a, hipStream_t s);
// r_o + r_u in 9 .. 32: the joint regression is the ORDINARY loadings step (launch_mstep_lam at Re = 16 | 32) on augmented
// moments z = (g, f), Var z = blockdiag(0, P) -- and the identity on the padding, as the padded state of an ordinary pass has it.
// launch_obs_augment builds z [B][T][Re], Var z packed [B][T][Re (Re + 1) / 2], the padded copy of the loadings [B][N][Re] and
// sum_t E z z' with its inverse [B][Re][Re] each.
bool mstep_obs_wide_supported(int ro, int ru);
int mstep_obs_wide_width(int ro, int ru);                      // Re
hipError_t launch_obs_augment(const ObsArgs& a, int Re, double* z, double* Vz, double* LamAug, double* S11, double* S11inv, hipStream_t s);
// y = x - Lam_o g (NaN stays NaN) and LamP [B][N][Rl] = unobserved-factor loadings, zero padded
hipError_t launch_obs_residual(const ObsArgs& a, double* y, double* LamP, hipStream_t s);

// Balanced-panel fast path (fastpath.hip): data-independent covariance steps (cov_kernel) and the
// time-parallel mean recursion (meanscan_kernel).  All matrices in the padded dimension Rp.
struct FastArgs {
    int B, T, N, r, L;          // r = caller's factor count for the outputs; L = chunk length (power of 2)
    const double* A; const double* Q; const double* mu0; const double* P0;   // [B][Rp][Rp] / [B][Rp]
    const double* Cfull; const double* ldfull;                               // gram_kernel outputs (Lam == nullptr)
    const double* Lam; const double* Rv;                                     // or: cov_kernel computes them itself
    // cov_kernel -> meanscan_kernel
    double* tab;                // [B][T][3][Rp][Rp]  Z_e, J_e, G_e of the distinct covariance steps
    int* E;                     // [B]  number of distinct steps; step t uses entry min(t, E-1)
    double* stead;              // [B][fast_stead_mats][Rp][Rp]  steady Z, J, G, G^(L 2^k), J^(L 2^k)
    double* xi0;                // [B][Rp]
    double* PT;                 // [B][Rp][Rp]   P_T|T
    double* llc;                // [B]  data-independent part of -2 loglik
    int* fill;                  // [B][2]  rows [lo, hi) of P_smooth equal to PsInf
    double* PsInf;              // [B][Rp][Rp]
    double* SP11; double* SU; double* P0s;   // EM covariance sums (or null)
    // collapse -> meanscan
    const double* bcol; const double* ssum;                                  // ssum [B][kSsumSlots]
    int nseg;                   // slots of ssum that were written
    const double* scol; int ntile;   // ntile > 0: sum_t s_t = sum of scol[b][0 .. ntile) instead (collapse_wide)
    double* wtab;               // [B][T][Rp] scratch
    size_t wrep;                // doubles per replicate of wtab (0: T Rp)
    int bst;                    // doubles between the rows of bcol (0: Rp) -- CollapseArgs::bst of the collapse that wrote them
    // outputs
    double* f_smooth; double* P_smooth; double* loglik;
    double* f0s;                // [B][Rp] E[f_0 | X] (EM) or null
    int b0;                     // meanscan: first replicate of this launch (sub-batch pipelining)
    int abl;                    // diagnostics (DFM_SCAN_ABL): bit0 skip the P_smooth fill, bit1 skip the scans
    int rstate;                 // the model's state width (<= Rp; 0 = unknown: Rp) -- cov_tile_kernel executes ceil(rstate / 4) block pivots
};
struct EmUpdArgs {               // transition M-step + EM bookkeeping after a fast-path E-step (all padded, Rp)
    int B, T;
    const double* fsm;           // [B][T][Rp] smoothed means
    const double* f0s;           // [B][Rp]    E[f_0 | X]
    const double* SP11; const double* SU; const double* P0s; const double* PT;   // cov_kernel: [B][Rp][Rp]
    const double* loglik;        // [B] log-likelihood of this E-step
    double* S11; double* S11inv; // [B][Rp][Rp] for the loadings step
    double* A_out; double* Q_out; double* mu0_out; double* P0_out;
    int* active; int* iters; double* ll_path; int k, max_iter; double tol;   // as RecursionArgs
};
hipError_t launch_em_update(int Rpad, const EmUpdArgs& a, hipStream_t s);
bool em_update_grid_supported(int Rpad);                                     // Rp = 16, 32: element-per-thread form (em_update_grid.hip)
hipError_t launch_em_update_grid(int Rpad, const EmUpdArgs& a, hipStream_t s);
hipError_t launch_cov(int Rpad, const FastArgs& a, hipStream_t s);
bool cov_fuses_gram(int Rpad, int N);   // launch_cov with a.Lam != nullptr is supported for this shape
hipError_t launch_meanscan(int Rpad, const FastArgs& a, hipStream_t s);
hipError_t launch_meanscan_mfma(int Rpad, const FastArgs& a, hipStream_t s);   // Rp = 16, 32: the steady scans on the matrix pipe (scan_mfma32.hip)
hipError_t launch_pfill(int Rpad, const FastArgs& a, hipStream_t s);   // the P_smooth fill of meanscan (then run it with abl bit 0)
// The whole balanced pass in one launch (pass_fused.hip: persistent workgroups, stream / covariance / scan waves) and the
// one-wave-per-replicate covariance recursion as a drop-in for launch_cov (Rp = 8, Cfull / ldfull from gram_kernel).
bool pass_fused_supported(int Rpad, int T, int N);
int pass_fused_pick_nsw(int T, int N, int want);            // stream waves per workgroup that fit the 160 KB of LDS (diagnostic)
int pass_fused_pick_nbuf(int T, int N);                     // b_t buffers of that layout (diagnostic)
bool pass_fused_pick_wpark(int T, int N);                   // the weight hand-over's route rule at that shape (diagnostic)
// nsw / ncov: stream / covariance waves per workgroup (0 = as many as fit)
hipError_t launch_pass_fused(const CollapseArgs& a, const FastArgs& fa, int nsw, int ncov, bool wpark, int num_cu, hipStream_t s);
hipError_t launch_cov_wave(const FastArgs& a, hipStream_t s);
// the element-per-thread covariance recursion for Rp = 16 / 32 (a workgroup of Rp x Rp threads per replicate; Cfull / ldfull
// from the Gram kernel): what launch_cov runs for those widths unless DFM_COV_ROWS=1
bool cov_grid_supported(int Rpad);
// Rp = 32: the same recursion with four waves per replicate on the matrix pipe (recursion_tile.hip); rstate = the model's state width
bool cov_tile_supported(int Rpad, const FastArgs& a, int rstate);
hipError_t launch_cov_tile(const FastArgs& a, int rstate, hipStream_t s);
hipError_t launch_cov_grid(int Rpad, const FastArgs& a, hipStream_t s);
int fast_chunk_len(int Rpad, int T);
int fast_stead_mats(int Rpad);
int fast_scan_groups(int Rpad);   // time chunks of the mean scan

// PCA initialisation (pca.hip).  Scratch arrays use the padded factor dimension Rp; outputs the caller's r.
struct PcaArgs {
    int B, T, N, r, max_iter;
    const double* panel;        // [B][T][N], no NaN
    double* S;                  // [B][N][N]   X'X
    double* V; double* Y;       // [B][N][Rp]  basis / S V
    double* F;                  // [B][T][Rp]  scores
    double* Lam; double* Rv; double* A; double* Q; double* mu0; double* P0;   // caller's layout (r)
    double* factors;            // [B][T][r] or null
    int* status;                // bit 1 (value 2): subspace iteration stopped at max_iter above its tolerance; or null
    int stop_after;             // diagnostics (DFM_PCA_STOP): > 0: pca_kernel returns after that phase (timing of the phases)
};
hipError_t launch_gram_xx(const PcaArgs& a, hipStream_t s, int variant = 0);   // 0: matrix pipe (N <= 256; even N beyond: gram_xx_wide.hip), 1: VALU
bool gram_xx_wide_supported(int N);
hipError_t launch_gram_xx_wide(const PcaArgs& a, hipStream_t s);
hipError_t launch_pca(int Rpad, const PcaArgs& a, hipStream_t s);

// Non-parametric estimator (als.hip): batched alternating least squares and batched complete-case OLS.
struct AlsArgs {
    int B, T, N, rmax;
    const double* z;            // standardised panels, [T][N] each, NaN = missing; problem b at z + b * z_stride
    long long z_stride;         // 0: every problem reads the same panel
    const int* r_each;          // [B] factors of each problem (<= rmax), or null (all rmax)
    double* F;                  // [B][T][rmax]  in: start (PCA scores); out: factors after the last sweep
    double* Lam;                // [B][N][rmax]  out: loadings of the last sweep (NaN: series without loadings)
    int nt_min, max_iter;
    double tol;
    double* ssr_path; int path_cap;   // [B][path_cap] SSR after every sweep (NaN past the last), or null
    int* iters; double* ssr;    // [B]
    double* R2;                 // [B][N] or null
};
hipError_t launch_als(int Rpad, const AlsArgs& a, hipStream_t s);
bool als_fits(int Rpad, int T, int N);      // factors + loadings fit the 160 KB of LDS

struct OlsArgs {
    int P, T, K;                // problems, rows, regressors (K <= 32)
    const double* X; long long x_stride;          // [T][K] per problem; x_stride 0: shared regressors
    const double* y; long long y_stride, y_inc;   // y_p[t] = y[p * y_stride + t * y_inc]
    int nt_min;                 // fewer complete rows: coefficients NaN
    double* beta;               // [P][K]
    double* resid;              // [P][T] (NaN on dropped rows) or null
    double* ssr; double* tss;   // [P]; tss = sum (y - ybar)^2 over the used rows, or null
    int* nobs;                  // [P] complete rows
};
hipError_t launch_ols(int Rpad, const OlsArgs& a, hipStream_t s);
hipError_t launch_standardize(int B, int T, int N, double* panel, double* mean_out, double* sd_out, hipStream_t s);

// Wild-bootstrap impulse responses of the factor VAR and quantile bands (boot.hip).
struct BootArgs {
    int B, T, ns, p, H;         // draws, periods of the window, variables, lags, horizons
    const double* y;            // [T][ns] the VAR's data over the window (no NaN)
    const double* betahat;      // [1 + ns p][ns] point estimate (constant first)
    const double* resid;        // [T][ns] residuals (rows < p unused)
    const double* signs;        // [B][T] +-1, or null: Rademacher signs from Philox(seed; draw, period)
    uint64_t seed; int64_t first_draw;   // device-drawn signs are a function of (seed, first_draw + d, period)
    double* beta_out;           // [B][1 + ns p][ns] re-estimated coefficients, or null
    double* irf;                // [B][ns][H][ns]  irf[d][i][h][k] = (Q M^h G[:, k])_i of draw d
};
hipError_t launch_var_boot(const BootArgs& a, hipStream_t s);
struct QuantArgs {
    int B, S, nq;               // draws, series per draw, quantiles
    const double* x;            // [B][S]
    const double* q;            // [nq] in (0, 1]
    double* out;                // [nq][S]
};
hipError_t launch_quantiles(const QuantArgs& a, hipStream_t s);

// Batched Chow / QLR statistics with HAC covariance (breaks.hip).
struct ChowArgs {
    int S, Tmax, k, P;          // series, row capacity per series, regressors (before interaction), problems
    const double* y;            // [S][Tmax] complete cases of each series
    const double* X;            // [S][Tmax][k]
    const int* Tlen;            // [S] rows in use
    const int* prob_series; const int* prob_break; const int* prob_q;   // [P]
    double* chow;               // [P]
};
hipError_t launch_chow(const ChowArgs& a, hipStream_t s);

// Nowcasts and forecasts of the panel from a fitted model (forecast.hip).
struct FcTailArgs {             // p = 1: f_{T+h|T}, P_{T+h|T} for h = 1..H from the terminal smoothed moments
    int B, T, H, r;
    const double* fsm;          // [B][T][r] smoothed factors
    const double* Psm;          // [B][T][r(r+1)/2] packed, or null (no covariances wanted)
    const double* A; const double* Q;   // [B][r][r]
    double* ft;                 // [B][H][r]
    double* Pt;                 // [B][H][r(r+1)/2] or null
};
hipError_t launch_forecast_tail(const FcTailArgs& a, hipStream_t s);
struct FcFillArgs {
    int B, T, H, N, r;
    const double* panel; int panel_rows;   // [B][panel_rows][N], rows t < T read (panel_rows = T, or T + H for xhat in place)
    const double* fh; const double* Ph; int Th;   // head rows t < Th: [B][Th][r], [B][Th][r(r+1)/2] (Ph null: no covariances)
    const double* ft; const double* Pt;           // rows Th <= t < T + H: [B][H][..] (p = 1 tail)
    const double* Lam; const double* R;           // [B][N][r], [B][N]
    const double* mean; const double* sd;         // [B][N] or both null
    double* xhat; double* xvar; double* common;   // [B][T+H][N]; xvar / common may be null
    double* f_out; double* P_out;                 // copy of the staged rows in the [B][T+H] layout, or null
    CellGeom geo;                                 // geometry (set by the launcher)
};
hipError_t launch_forecast_fill(const FcFillArgs& a, hipStream_t s);
hipError_t launch_forecast_pad(int B, int T, int H, int N, const double* panel, double* out, bool check_nan, int* status,
                               hipStream_t s);

// The path draws of the same model (simsmooth_ar.hip; dfm_simsmooth_ar_batch): what the two kernels that walk the simulated series
// read beside FcArArgs (SsArArgs, below).  There the launch covers the pass replicates j0 .. j0 + S - 1 (j = b D + d), Lam / sig2 /
// rho / v0 / mean / sd are the caller's [B] arrays, and f, msg, last are the slice's ([S]: the smoothed mean g of the difference
// panels).  A struct of its own: grown by these fields, FcArArgs cost two instances of forecast_ar_fwd_kernel a wave per SIMD.
struct SsArDraw {
    int D, T, k;                                  // draws per replicate, panel rows, k = r max(p, q + 1)
    long long j0;
    uint64_t seed; int64_t first_draw;
    const double* X;                              // [B][T][N] the caller's panel (NaN = missing)
    const double* fplus;                          // [B D][n][r] the simulated factor path (f_draw before g joins)
    const double* mu0; const double* LP0;         // [B][k], [B][k][k] (lower PSD root of P0)
    double* diff;                                 // [S][n + q][N] difference panels of the slice
    double* x_draw;                               // [B D][n][N]
    int check_nan; int* status;                   // a NaN in X raises bit 1 of *status (no DFM_F_MAY_HAVE_MISSING)
};

// The series side of the forecasts with AR(q) idiosyncratic terms (forecast_ar.hip): one launch covers the S replicates b0 ..
// b0 + S - 1 of the call, whose messages fill the slice buffer.
struct FcArArgs {
    int b0, S, n, N, r, q;                        // n = T + H - q output rows (panel rows q .. T + H - 1)
    const double* panel;                          // [B][n + q][N]: the panel with its H all-missing rows
    const double* f; const double* P;             // [B][n][r], [B][n][r(r+1)/2] (P is read only with xvar)
    const double* Lam; const double* sig2; const double* rho;   // [B][N][r], [B][N], [B][N][q]
    const double* v0;                             // [B][N] variance of the q terms before output row 0, or null (sig2)
    const double* mean; const double* sd;         // [B][N] or both null
    double* msg; int* last;                       // [S][q + q(q+1)/2][n][N] backward messages, [S][N] last observed row (-1: none)
    double* xhat; double* xvar; double* common; double* idio;   // [B][n][N]; all but xhat may be null
    CellGeom geo;                                 // geometry (set by the launcher)
};
hipError_t launch_forecast_ar_back(const FcArArgs& a, hipStream_t s);
hipError_t launch_forecast_ar_fwd(const FcArArgs& a, hipStream_t s);
size_t forecast_ar_msg_bytes(int n, int N, int q);   // the messages of ONE replicate
struct SsArArgs : FcArArgs { SsArDraw dr; };
hipError_t launch_simsmooth_ar_diff(const SsArArgs& a, hipStream_t s);      // simsmooth_ar.hip
hipError_t launch_simsmooth_ar_fwd(const SsArArgs& a, hipStream_t s);       // forecast_ar.hip: the forward kernel's text
// A_pad [B][r][r m] = [A_1 .. A_p 0 ..]; erho [S][N][q] = rho of replicate (j0 + s) / D
hipError_t launch_simsmooth_ar_params(int B, int r, int p, int m, const double* Avar, double* Apad, hipStream_t s);
hipError_t launch_simsmooth_ar_expand(int S, long long j0, int D, size_t per, const double* src, double* dst, hipStream_t s);
hipError_t launch_simsmooth_ar_finish(size_t n, const double* g, double* f_draw, hipStream_t s);   // f_draw += g

// Posterior draws of factor and panel paths, Durbin-Koopman simulation smoother (simsmooth.hip).  Pass replicate j = b D + d;
// a call runs its B D pass replicates in slices j0 .. j0 + S - 1.
struct SsArgs {
    int B, D, T, N, r, p, H;
    const double* panel;                          // [B][T][N] (NaN = missing)
    const double* Lam; const double* R;           // [B][N][r], [B][N]
    const double* A; const double* Q;             // [B][r][r p] = [A_1 .. A_p], [B][r][r]
    const double* mu0; const double* P0;          // [B][r p], [B][r p][r p]
    const double* mean; const double* sd;         // [B][N] or both null
    uint64_t seed; int64_t first_draw;
    double* f_draw;                               // [B][D][T+H][r]
    double* x_draw;                               // [B][D][T+H][N] or null
    double* LP0; double* LQ;                      // [B][r p][r p], [B][r][r]: lower PSD roots (simsmooth_prep_kernel)
    long long j0; int S;                          // the slice
    double* diff;                                 // [S][T][N] difference panels of the slice
    double *eLam, *eR, *eA, *eQ, *emu0, *eP0;     // [S][..] the pass's parameters (mu0 = 0)
    const double* g;                              // [S][T][r] smoothed mean of the difference panels
    CellGeom geo;                                 // geometry of the cell kernels (set by their launchers)
};
hipError_t launch_simsmooth_prep(const SsArgs& a, hipStream_t s);
hipError_t launch_simsmooth_expand(const SsArgs& a, hipStream_t s);
hipError_t launch_simsmooth_path(const SsArgs& a, hipStream_t s);
hipError_t launch_simsmooth_diff(SsArgs a, hipStream_t s);
hipError_t launch_simsmooth_finish(const SsArgs& a, hipStream_t s);
hipError_t launch_simsmooth_fill(SsArgs a, hipStream_t s);

// Panels simulated from a given model (simulate.hip; dfm_simulate_batch, dfm_simulate_ar_batch): x+ of the smoothers' step 1, written
// out.  Both read f+ of the slice from f_draw / dr.fplus, [B D][rows][r] with H = 0, as simsmooth_path_kernel leaves it.
//   plain: a.panel is the mask panel [B][T][N] or null (balanced), a.x_draw the output [B D][T][N]
//   AR:    a.dr.X is the panel [B][T][N] or null, a.dr.x_draw the output [B D][T][N] (rows < q included; a.n = T - q)
hipError_t launch_simulate_cells(SsArgs a, hipStream_t s);
hipError_t launch_simulate_ar_cells(const SsArArgs& a, hipStream_t s);

// News decomposition of nowcast revisions (news.hip).  Pass replicate j = b G + g (replicate b, target g); a call runs its B G
// weight passes in slices j0 .. j0 + S - 1.
struct NwArgs {
    int B, T, N, r, p, G, TH;                     // TH = T + H rows of the forecasts
    const double* oldp; const double* newp;       // [B][T][N] (NaN = missing)
    const double* Lam; const double* R;           // [B][N][r], [B][N]
    const double* A; const double* P0;            // [B][r][r p], [B][r p][r p]
    const double* Q;                              // [B][r][r]
    const double* mean; const double* sd;         // [B][N] or both null
    const int* tgt;                               // device [G][2] = (t*, i*)
    double* rev;                                  // [B][T][N] revised old panel
    const double* xrev;                           // [B][TH][N] xhat of the revised-old run
    double* yhat;                                 // [B][3][G]
    double* impact;                               // [B][G][N]
    double* news;                                 // [B][T][N] or null
    double* weight;                               // [B][G][T][N] or null
    int* status;                                  // bit 8: a cell of old is observed where new is NaN
    long long j0; int S;                          // the slice
    double* u;                                    // [S][T][r p] (A_c')^(t*-t) S' lam_i* of the rows t < min(t*, T)
    double* av;                                   // [S][T][r] S Cov(z_{t+1}, z_{t*+1}) S' lam_i*
    double* cp;                                   // [S][T][N] covariance panels (may alias the slice's part of weight)
    const double* g;                              // [S][T][r] E_0[f | c] of the covariance panels
    CellGeom geo;                                 // geometry of the cell kernels (set by their launchers)
};
hipError_t launch_news_revise(const NwArgs& a, hipStream_t s);
hipError_t launch_news_gather(const NwArgs& a, const double* xhat, int which, hipStream_t s);
hipError_t launch_news_gamma(const NwArgs& a, hipStream_t s);
hipError_t launch_news_cov_panel(NwArgs a, hipStream_t s);
hipError_t launch_news_impact(NwArgs a, hipStream_t s);

// The same for the model with AR(q) idiosyncratic terms (news_ar.hip).  Rows are output rows t = 0 .. (panel rows q ..), as in
// FcArArgs: ns = T - q of them in the sample, n = T + H - q in the forecasts; the state is k = r max(p, q + 1) wide.
struct NwArArgs {
    int B, T, N, r, q, k, ka, G, n, ns, Rp;       // ka = r p: columns of A; Rp: row stride of g (the pass's padded state)
    const double* oldp; const double* newp;       // [B][T][N] (NaN = missing)
    const double* Lam; const double* sig2; const double* rho;   // [B][N][r], [B][N], [B][N][q]
    const double* A; const double* Q; const double* P0;         // [B][r][ka], [B][r][r], [B][k][k]
    const double* mean; const double* sd;         // [B][N] or both null
    const int* tgt;                               // device [G][2] = (t* - q, i*): the target's OUTPUT row and series
    double* rev;                                  // [B][T][N] revised old panel
    const double* xrev;                           // [B][n][N] xhat of the revised-old run
    double* impact;                               // [B][G][N]
    double* news;                                 // [B][ns][N] or null
    double* weight;                               // [B][G][ns][N] or null
    int* status;                                  // bit 8: a vintage is not edge-shaped, or a cell of old is missing in new
    long long j0; int S;                          // the slice
    double* u;                                    // [S][ns][k + 1] u_t and psi_{t* - t} of the rows t <= min(t*, ns - 1)
    double* dv;                                   // [S][ns][(q + 1) r + 1] d_t on the observed lag blocks, psi_{t* - t} (0 behind t*)
    double* qc;                                   // [S][ns][N] covariance panels (may alias the slice's part of weight)
    const double* g;                              // [S][ns][Rp] E_0[z | qc] of the covariance panels
    CellGeom geo;                                 // geometry of the cell kernels (set by their launchers)
};
hipError_t launch_news_ar_revise(const NwArArgs& a, hipStream_t s);
hipError_t launch_news_ar_rec(const NwArArgs& a, hipStream_t s);
hipError_t launch_news_ar_qc(const NwArArgs& a, hipStream_t s);
hipError_t launch_news_ar_impact(const NwArArgs& a, hipStream_t s);

// Structural analysis of the factor VAR: identified impulse responses, variance and historical decompositions (structural.hip).
struct SvArgs {
    int B, N, r, p, H, T;
    const double* Lam; const double* R;           // [B][N][r], [B][N] (R null: no fevd)
    const double* A; const double* Q;             // [B][r][r p] = [A_1 .. A_p], [B][r][r]
    const double* sd;                             // [B][N] or null
    const int* named;                             // device [r] distinct series, or null (S = chol Q)
    const int* cum;                               // device [N], non-zero = cumulated outputs, or null
    int unit_effect, need_pd;                     // need_pd: a zero column of the root raises status bit 16 (S^-1 is wanted)
    int* status;                                  // bit 16: Ln singular, or (need_pd) the root has a zero pivot
    double* S; double* Sinv;                      // [B][r][r] eta = S u; Sinv = S^-1 (null: not wanted)
    double* scale;                                // [B][r] impact response of series named[k] to shock k in output units, or null
    double* Th; double* Thc;                      // [B][H][r][r] shock-major: Th[h][k][m] = (Theta_h)_mk; Thc cumulated (null: no cum)
    double* irf; double* fevd;                    // [B][r][H][N], [B][r+1][H][N] or null
    const double* f;                              // [B][T][r] smoothed factors
    double* u;                                    // [B][T][r] structural shocks, zero rows for t < p
    double* C;                                    // [B][r+1][T][r] contribution paths, slot r = the initial condition
    double* hd;                                   // [B][r+1][T][N]
    CellGeom geo; int CP, TC;                     // geometry (set by the launchers)
    int slots;                                    // sv_irf_fill_kernel: tables and outputs per replicate (signirf.hip: K kept slots;
                                                  // Th, Thc, irf, fevd are then [B slots][..]); 0 or 1: one, the plain entries
};
hipError_t launch_sv_prep(const SvArgs& a, hipStream_t s);
hipError_t launch_sv_irf_fill(SvArgs a, hipStream_t s);
hipError_t launch_sv_shock(const SvArgs& a, hipStream_t s);
hipError_t launch_sv_path(SvArgs a, hipStream_t s);
hipError_t launch_sv_hd_fill(SvArgs a, hipStream_t s);

// Sign-restricted impulse responses (signirf.hip): M candidate rotations per replicate, the first K accepted ones kept.
constexpr size_t kSgTabLds = 48 * 1024;           // sv_sign_kernel: the replicate's table of restricted responses, at most
struct SgArgs {
    int B, N, r, H, M, K;
    int nS, HT, G;                                // distinct restricted series, horizons in the table (max h1 + 1), restrictions
    const double* Lam; const double* sd;          // [B][N][r], [B][N] or null
    const int* cum;                               // device [N] or null
    const int* ser;                               // device [nS]: the distinct restricted series
    const int* gs;                                // device [r+1]: the restrictions of shock k are rows gs[k] .. gs[k+1] - 1
    const int* rows;                              // device [G][4]: (index into ser, h0, h1, sign), sorted by shock
    const double* S;                              // [B][r][r] base impact matrix (sv_prep_kernel)
    const double* Th; const double* Thc;          // [B][H][r][r] shock-major tables of sv_prep_kernel; Thc null: nothing cumulated
    double* tab;                                  // [B][nS][HT][r] a_{i,h} = sd_i lam_i' Theta_h (Theta^c_h where cum[i])
    uint64_t seed; int64_t first_cand;
    int* mask;                                    // [B][M] 1 = accepted
    int* wcnt;                                    // [B][ceil(M / 64)] accepted candidates of each group of 64
    double* rot;                                  // [B][M][r][r] Rot D of the accepted candidates (r > 8: of every candidate)
    int* n_accept; int* cand_out;                 // [B], [B][K]
    double* S_out;                                // [B][K][r][r] or null
    double* ThK; double* ThcK;                    // [B][K][H][r][r] tables of the kept slots, NaN where empty (null: not wanted)
};
size_t sign_table_bytes(int nS, int HT, int r);
hipError_t launch_sv_sign_table(const SgArgs& a, hipStream_t s);
hipError_t launch_sv_sign(const SgArgs& a, hipStream_t s);
hipError_t launch_sv_sign_keep(const SgArgs& a, hipStream_t s);

// Impulse responses identified by an external instrument (proxy.hip): slot 0 = the sample, slots 1 .. D = moving block draws of
// the n used rows.  S = chol(Q), S^-1 and the tables Theta_h = Psi_h S come from sv_prep_kernel with named = null.
constexpr int kPxLanes = 256;                     // px_moment_kernel: slots per workgroup, one per lane
constexpr size_t kPxTabLds = 48 * 1024;           // px_moment_kernel: a row table up to this size sits in LDS; a larger one is read
                                                  // from global memory (through L2)
struct PxArgs {
    int B, T, N, r, p, H, n, D, L, norm, unit;    // n used rows, D block draws of length L; unit: DFM_SV_UNIT_EFFECT
    const double* Lam; const double* sd;          // [B][N][r], [B][N] or null
    const double* A;                              // [B][r][r p]
    const int* cum;                               // device [N] or null
    const int* U;                                 // device [n]: the used rows, increasing
    const double* z;                              // device [T]: the instrument (NaN where not used)
    const double* f;                              // [B][T][r] smoothed factors
    const double* S; const double* Sinv;          // [B][r][r] (sv_prep_kernel)
    const double* Th; const double* Thc;          // [B][H][r][r] shock-major; Thc null: nothing cumulated
    uint64_t seed; int64_t first_draw;
    double* rows;                                 // [B][n][r+1]: etahat and z of the used rows
    double* impact; double* rel;                  // [B][D+1][r], [B][D+1]
    double* w;                                    // [B][D+1][r]: S^-1 hvec, a unit vector (NaN for a NaN slot)
    double* tk; double* tkc;                      // [B][D+1][H][r]: Theta_h w and the cumulated form (tkc null: nothing cumulated)
    double* scale;                                // [B][D+1]: the unit-effect divisor of the slot (null: no unit effect)
    const double* R;                              // [B][N] (the den table and fevd)
    double* den;                                  // [B][H][N]: sum_k num_k + idio of dfm_irf_batch (null: no fevd)
    double* irf; double* fevd;                    // [B][D+1][H][N] or null
    double* shock;                                // [B][T] or null
    CellGeom geo;                                 // geometry of the fill (set by its launcher)
};
size_t proxy_row_stride(int r);                   // doubles per row of the table in LDS: r + 1 rounded up to an odd number
hipError_t launch_px_rows(const PxArgs& a, hipStream_t s);
hipError_t launch_px_moment(const PxArgs& a, hipStream_t s);
hipError_t launch_px_slot_table(const PxArgs& a, hipStream_t s);
hipError_t launch_px_den(const PxArgs& a, hipStream_t s);
hipError_t launch_px_fill(PxArgs a, hipStream_t s);
hipError_t launch_px_shock(const PxArgs& a, hipStream_t s);

// Filtered states, prediction errors and out-of-sample evaluation: the plain parametric fit (filter.hip) and the fit with AR(q)
// idiosyncratic terms (filter_ar.hip).  Plain: the state has width k = r p, the observation loads on its first w = r entries and
// the n = T output rows are the panel's.  AR: m = max(p, q + 1), k = r m, w = r (q + 1) (the width the quasi-differenced
// observation loads on), n = T - q output rows (panel rows q .. T-1).  kk = k (k + 1) / 2.
// What the forward recursion reads and writes (filter_recursion, dfm_filter.h):
struct FtRec {
    int B, n, N, r, p, k, w, Rp;                  // Rp: width of the collapse's rows (pad_r(r); AR: pad_r(k))
    const double* A; const double* Q;             // [B][r][r p] = [A_1 .. A_p], [B][r][r]
    const double* mu0; const double* P0;          // [B][k], [B][k][k]
    // launch_collapse's per-period arrays (CollapseArgs) over the n rows: Ct / ldrow are read only where nobs < N
    const double* bcol; const double* scol; const int* nobs; const double* ldrow; const double* Ct; const double* Cfull;
    const double* ldfull;
    double* z_pred; double* P_pred;               // [B][n][k], [B][n][kk] (the fill reads them: never null when it runs)
    double* z_filt; double* P_filt;               // [B][n][k] (the evaluation reads it), [B][n][kk] or null
    double* loglik_t;                             // [B][n] or null
    int* status;                                  // bit 32: a replicate's update failed
};
// ... and what the fill and evaluation kernels of both fits take beyond that
struct FtCells : FtRec {
    int H, t0;                                    // t0: the first origin, a panel row (AR: >= q)
    const double* panel;                          // [B][T][N] (NaN = missing): the panel itself (AR: not its quasi-differences)
    const double* Lam;                            // [B][N][r]
    const double* mean; const double* sd;         // [B][N] or both null
    double* xpred; double* verr; double* vstd;    // [B][n][N] or null
    double* msfe; double* msfe0; int* cnt;        // [B][H][N] or null
    double* acc; double* acc0; int* acn;          // [B][H][N] each: the evaluation's running sums (scratch)
    CellGeom geo;                                 // geometry of the fill (set by its launcher)
};
struct FtArgs : FtCells {
    const double* R;                              // [B][N]
};
struct FtArArgs : FtCells {
    int q;
    const double* sig2; const double* rho;        // [B][N], [B][N][q]
    double* msfe_common;                          // [B][H][N] or null
    double* accc;                                 // [B][H][N]: its running sum (scratch)
};
size_t filter_lds_bytes(int r, int k);            // filter_kernel's LDS
size_t filter_ar_lds_bytes(int r, int k, int w);  // filter_ar_kernel's LDS
hipError_t launch_filter(const FtRec& a, hipStream_t s);
hipError_t launch_filter_fill(FtArgs a, hipStream_t s);
hipError_t launch_filter_eval(const FtArgs& a, hipStream_t s);
hipError_t launch_filter_ar(const FtRec& a, hipStream_t s);
hipError_t launch_filter_ar_fill(FtArArgs a, hipStream_t s);
hipError_t launch_filter_ar_eval(const FtArArgs& a, hipStream_t s);

// One Gibbs sweep's parameter block "parameters | factor path" (gibbs.hip); chain b of B, the key of sweep `sweep`.
struct GbArgs {
    int B, T, N, r, p;
    const double* panel;                          // [B][T][N] (NaN = missing)
    const double* f;                              // [B][T][r]: the sweep's factor path
    double* Lam; double* R;                       // [B][N][r], [B][N]: written by gibbs_load_kernel
    double* A; double* Q;                         // [B][r][r p], [B][r][r]: written by gibbs_var_kernel
    const double* A0;                             // [B][r][r p] prior mean of the VAR coefficients, or null (zero)
    double tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q;
    uint64_t seed; int64_t sweep;
    bool missing;                                 // DFM_F_MAY_HAVE_MISSING: a Gram matrix per series; else one per chain (Lsh)
    double* Lsh;                                  // [B][r][r]: root of tau_lam I + F'F (gibbs_gram_kernel; balanced panels)
    int* status;                                  // bit 64: a Cholesky failed or the gamma sampler ran into its cap
};
hipError_t launch_gibbs_gram(const GbArgs& a, hipStream_t s);
hipError_t launch_gibbs_load(const GbArgs& a, hipStream_t s);
hipError_t launch_gibbs_var(const GbArgs& a, hipStream_t s);

// The series block "rho_i, sig2_i, lam_i | factor path" of one sweep of dfm_gibbs_ar_batch (gibbs_ar.hip); chain b of B.  Output
// row t = 0 .. n-1 is panel row t + q; the first q panel rows are never read here.
struct GbArArgs {
    int B, n, N, r, q;
    const double* panel;                          // [B][n + q][N] (NaN = missing)
    const double* f;                              // [B][n][r]: the sweep's factor path
    double* Lam; double* sig2; double* rho;       // [B][N][r], [B][N], [B][N][q]: read on entry, written in place
    double tau_lam, nu_R, s_R, tau_rho;
    uint64_t seed; int64_t sweep;
    int* status;                                  // bit 64: a Cholesky failed, the gamma sampler or the rho sampler ran into its cap
    CellGeom geo;                                 // geometry (set by the launcher)
};
hipError_t launch_gibbs_ar_series(const GbArArgs& a, hipStream_t s);

// Rolling-window out-of-sample evaluation (rolling.hip; dfm_rolling_eval_batch).  A call runs its O windows in slices b0 ..
// b0 + S - 1; every array marked [S] is the slice's part (the driver offsets the caller's [O] arrays by b0).
constexpr int kRwWindowBit = 128;                 // status word bit: a series of a window is thin or constant
struct RwArgs {
    int T, N, W, H, r, k;                         // panel rows, series, window rows, horizons, factors, state width r p
    int b0, S, min_obs;
    const double* x;                              // [T][N] the raw panel, data units (NaN = missing)
    const int* origins; const int* lags;          // device [O], [N] (lags null: all 0)
    double* win;                                  // [S][W][N] the standardised vintages
    double* mean; double* sd; int* nobs;          // [S][N]
    int* status;                                  // bit kRwWindowBit
    int n_start;                                  // rolling_start_kernel: 1 = one start for every window, else one per window ([O])
    const double *sLam, *sR, *sA, *sQ, *smu0, *sP0;   // the start, layouts of dfm_em_varp_batch
    const double* sd_start;                       // [N] or null (no rescale)
    double *Lam, *R, *A, *Q, *mu0, *P0;           // [S][..] the windows' parameters
    const double* xhat; const double* xvar;       // rolling_score_kernel: [S][W + H][N] of the slice's forecasts
    double *fc, *fvar, *err, *err_std;            // [S][H + 1][N], each may be null
    double *sse, *sse0; int* cnt;                 // [H + 1][N] running sums over the origins scored so far
    double *msfe, *msfe0; int* cnt_out;           // [H + 1][N], each may be null: written when last
    int first, last;                              // the call's first / last slice: the sums start at zero / are divided
};
hipError_t launch_rolling_window(const RwArgs& a, hipStream_t s);
hipError_t launch_rolling_start(const RwArgs& a, hipStream_t s);
hipError_t launch_rolling_score(const RwArgs& a, hipStream_t s);

// Diffusion-index forecasts from the non-parametric fit, out of sample (diffusion.hip; dfm_diffusion_eval_batch).  The windows are
// those of RwArgs (launch_rolling_window) and run in the same slices; every array marked [S] is the slice's part.
struct DiArgs {
    int T, N, W, H, r, q, K;                      // panel rows, series, window rows, horizons, factors, own lags, K = 1 + r + q
    int b0, S, nt_min, n_start;
    int missing_ok;                               // di_start_kernel: DFM_F_MAY_HAVE_MISSING was given (else a NaN inside a window raises bit 1)
    const double* x;                              // [T][N] the raw panel, data units
    const int* origins; const int* lags;          // device [O], [N] (lags null: all 0)
    const double* F_start;                        // [T][r] (n_start = 1: window b takes rows o_b - W + 1 .. o_b) or [O][W][r]
    double* F;                                    // [S][W][r] di_start_kernel: the start; di_regress_kernel: the windows' factors
    const double* win;                            // [S][W][N] the standardised vintages
    const double* mean; const double* sd; const int* nobs;   // [S][N]
    int* status;
    double *fc, *fc_ar, *fvar;                    // [S][H + 1][N] data units; never null here (the driver's block where the caller takes none)
    double* beta; int* nobs_reg;                  // [S][H + 1][N][K], [S][H + 1][N], each may be null
    double *err, *err_ar, *err_std;               // [S][H + 1][N], each may be null
    double *sse, *sse_ar, *sse0; int* cnt;        // [H + 1][N] running sums over the origins scored so far
    double *msfe, *msfe_ar, *msfe0; int* cnt_out; // [H + 1][N], each may be null: written when last
    int first, last;
    int nb;                                       // series per workgroup of di_regress_kernel (set by di_series_block)
    int h_first;                                  // 1: no series has a publication lag, so h = 0 has no regression; else 0
};
int di_series_block(int W, int r, int Rpad);      // the largest block of series whose LDS image fits the 160 KB at R = Rpad; 0: none does
hipError_t launch_di_start(const DiArgs& a, hipStream_t s);
hipError_t launch_di_regress(int Rpad, const DiArgs& a, hipStream_t s);
hipError_t launch_di_score(const DiArgs& a, hipStream_t s);

// Device-side synthetic replicates (synth.hip); all arrays in the caller's layout (r).
struct SynthArgs {
    int B, T, N, r;
    uint64_t seed; int64_t first_replicate; double missing_prob;
    double* panel; double* Lam; double* R; double* A; double* Q; double* mu0; double* P0;
    double* fscratch;           // [B][T+1][r]
    double* colstats;           // [B][synth_tiles(T)][2][N]  per-tile column sums (sum x, sum x^2) of the raw cells
};
int synth_tiles(int T);
hipError_t launch_synth(const SynthArgs& a, hipStream_t s);

}  // namespace dfm
