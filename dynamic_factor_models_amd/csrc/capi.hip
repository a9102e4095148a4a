// capi.hip -- the C-ABI of libdfmhip.so (include/dfm_hip.h): handle, workspace, entry points.
#include "../../include/dfm_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "dfm_kernels.h"
#include "dfm_mfgeom.h"
#include "dfm_msgeom.h"

using namespace dfm;

thread_local const char* dfm::t_launched_kernel = nullptr;

// A grow-only device block of the handle.  Growing synchronises the device first: every stream the handle has launched on (the
// caller may have swapped streams with dfm_set_stream, and the side / post streams of the fast path) must be done with the old
// block before it goes back to the allocator.
namespace {
struct DevBlock {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t grow(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            if (hipError_t e = hipDeviceSynchronize()) return e;
            if (hipError_t e = hipFree(p)) return e;
            p = nullptr;
            bytes = 0;
        }
        if (hipError_t e = hipMalloc(&p, need)) return e;
        bytes = need;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct RouteOpts {
    int subbatch = 0;                      // DFM_SUBBATCH: sub-batches per fast pass (0 = automatic)
    bool force_general = false;            // DFM_FORCE_GENERAL=1: never take the balanced fast path
    int collapse_variant = 0;              // DFM_COLLAPSE_VARIANT: 0 = automatic; 1..199 VALU kernel tunings; 200 = MFMA kernel
    int collapse_wpr = 0;                  // DFM_COLLAPSE_WPR: period segments (waves) per replicate of the MFMA collapse; 0 = automatic
    int scan_abl = 0;                      // DFM_SCAN_ABL: ablation bits of the fast path's scan (diagnostics)
    bool no_side = false;                  // DFM_NO_SIDE=1: gram/cov on the main stream (diagnostics)
    bool no_pipe = false;                  // DFM_PIPE=0 (diagnostics build): large batches with missing cells as ONE batch on one stream (pipe_eligible)
    bool no_rec_wave = false;              // DFM_NO_RECURSION_WAVE=1: lane-group recursion_kernel also at Rp = 8 (A/B)
    int tile_nc = 0, tile_w = 0;   // DFM_TILE_NC (route): chunks per replicate on recursion_tile_kernel (0 = automatic, 1 = the sequential kernel), DFM_TILE_W: warm-up periods
    bool no_chunk = false; int chunk_w = 0; double chunk_tol = 0.0;   // DFM_NO_CHUNK=1 (route): panels with missing cells at Rp = 8 on the sequential kernels;
                                           // DFM_CHUNK_W=n, DFM_CHUNK_TOL=x (route): warm-up periods / boundary tolerance of recursion_chunk.hip (0 = its defaults: 8, 1e-10)
    int pair_bmax = -1;                    // Rp = 8: batch limit of the covariance-wave + mean-wave pair (recursion_pair.hip); -1 = one replicate per SIMD,
                                           // DFM_PAIR_BMAX=n; DFM_NO_PAIR=1 = 0 (never)
    bool no_pfill = false;                 // DFM_NO_PFILL=1: P_smooth fill inside meanscan (diagnostics)
    bool fused_gram = true;                // DFM_FUSED_GRAM=0: gram_kernel as its own launch in front of the fused collapse launch
    bool no_fuse_cov = false;              // DFM_NO_FUSE_COV=1: cov_kernel / pfill_kernel as their own launches on a forked stream
    bool no_defer_em = false;              // DFM_NO_DEFER_EM=1 (route): em_update_kernel as its own launch behind the E-step
    bool no_mstep_mfma = false;            // DFM_NO_MSTEP_MFMA=1: VALU M-step for balanced panels too (diagnostics)
    bool em_general = false;               // DFM_EM_GENERAL=1: EM of balanced panels on the general path too (diagnostics)
    bool fuse_gram = false;                // DFM_FUSE_GRAM=1: Gram matrices inside cov_kernel instead of gram_kernel (slower: its
                                           // per-series loads are dependent round trips, ~5 us each beside the collapse)
    int pass_fused = 1;                    // the balanced pass at Rp = 8 as ONE launch (pass_fused.hip); DFM_PASS_FUSED=0: two launches
    int pass_nsw = 0;                      // DFM_PASS_NSW: stream waves per workgroup of that launch (0 = automatic)
    bool pf_wpark = true;                  // DFM_PF_WPARK=0 (route): the stream waves of that launch load their own weights (no hand-over by the fill wave)
    bool wide_old = false;                 // DFM_WIDE_OLD=1: Rp = 32 balanced collapse by collapse_wide_kernel + gram_wide_kernel
    int wide_sub = 1;                      // DFM_WIDE_SUB=n (2..8): the wide2 balanced pass in n sub-batches (measured slower: fast_route)
    bool collapse_miss_old = false;        // DFM_COLLAPSE_MISS_OLD=1: register-streamed collapse_kernel for panels with missing cells
    bool narrow_tab_off = false;           // DFM_NARROW_TAB=0 (diagnostics build): r <= 4 on the 8-wide state through collapse_kernel<4> + chunk_bridge_kernel
    bool gram_xx_valu = false;             // DFM_GRAM_XX_VALU=1: X'X of the PCA start on the VALU kernel (diagnostics)
    int pass_ncov = 0;                     // DFM_PASS_NCOV: covariance waves per workgroup of that launch (0 = automatic)
    bool cov_wave = false;                 // DFM_COV_WAVE=1: one-wave-per-replicate covariance recursion on the separate-launch path
    int mstep_miss_mode = 1;               // DFM_MSTEP_MISS (route): loadings step with missing cells on the matrix pipe (mstep_miss.hip): 0 = never
                                           // (mstep_lam_kernel), 1 = where mstep_lam_kernel keeps its per-series accumulators in global memory
                                           // (Rp > 8 or N > 256), 2 = wherever supported
    size_t fcar_msg_cap = (size_t)4 << 30;     // DFM_FCAR_MSG_BYTES=n (route): cap of the message buffer of dfm_forecast_ar_batch and dfm_simsmooth_ar_batch, which slice their replicates over it (4 GiB)
    bool odd_pad8 = true;                  // DFM_ODD_PAD8=0 (diagnostics build): odd N at states up to 8 wide stays on collapse_kernel
};

// Every switch of the library, read from the environment ONCE: route_env names select among production kernels, diag_env names
// exist in the diagnostics build only (dfm_kernels.h).  A handle keeps the values of its own creation (dfm_handle::opt), so one
// process can hold handles on either kernel; dfm_workspace_bytes, which has no handle, reads them at the call.
RouteOpts route_opts_from_env() {
    auto num = [](const char* v, int dflt) { return v ? atoi(v) : dflt; };
    auto on = [](const char* v) { return v && atoi(v) != 0; };             // NAME=1 turns it on
    auto off = [](const char* v) { return v && atoi(v) == 0; };            // NAME=0 turns it off
    auto pos = [](const char* v) { return v && atoi(v) > 0 ? atoi(v) : 0; };
    RouteOpts o;
    o.force_general = on(route_env("DFM_FORCE_GENERAL"));
    o.collapse_variant = num(diag_env("DFM_COLLAPSE_VARIANT"), 0);
    o.collapse_wpr = num(diag_env("DFM_COLLAPSE_WPR"), 0);
    if (o.collapse_wpr < 0 || o.collapse_wpr > kSsumSlots) o.collapse_wpr = 0;
    o.no_side = on(diag_env("DFM_NO_SIDE"));
    o.no_pipe = off(diag_env("DFM_PIPE"));
    o.no_rec_wave = on(diag_env("DFM_NO_RECURSION_WAVE"));
    if (const char* v = diag_env("DFM_PAIR_BMAX")) o.pair_bmax = pos(v);
    if (on(route_env("DFM_NO_PAIR"))) o.pair_bmax = 0;
    o.no_pfill = on(diag_env("DFM_NO_PFILL"));
    o.fused_gram = !off(diag_env("DFM_FUSED_GRAM"));
    o.no_fuse_cov = on(diag_env("DFM_NO_FUSE_COV"));
    o.no_mstep_mfma = on(diag_env("DFM_NO_MSTEP_MFMA"));
    o.no_defer_em = on(diag_env("DFM_NO_DEFER_EM"));
    o.em_general = on(diag_env("DFM_EM_GENERAL"));
    o.fuse_gram = on(diag_env("DFM_FUSE_GRAM"));
    o.subbatch = num(diag_env("DFM_SUBBATCH"), 0);
    o.scan_abl = num(diag_env("DFM_SCAN_ABL"), 0);
    o.mstep_miss_mode = num(route_env("DFM_MSTEP_MISS"), 1);
    o.pass_fused = num(route_env("DFM_PASS_FUSED"), 1);
    o.pass_nsw = num(diag_env("DFM_PASS_NSW"), 0);
    o.pf_wpark = !off(route_env("DFM_PF_WPARK"));
    o.pass_ncov = num(diag_env("DFM_PASS_NCOV"), 0);
    o.gram_xx_valu = on(diag_env("DFM_GRAM_XX_VALU"));
    o.collapse_miss_old = on(diag_env("DFM_COLLAPSE_MISS_OLD"));
    o.narrow_tab_off = off(diag_env("DFM_NARROW_TAB"));
    o.odd_pad8 = !off(diag_env("DFM_ODD_PAD8"));
    o.no_chunk = on(route_env("DFM_NO_CHUNK"));
    o.chunk_w = pos(route_env("DFM_CHUNK_W"));
    if (const char* v = route_env("DFM_CHUNK_TOL")) o.chunk_tol = atof(v) > 0.0 ? atof(v) : 0.0;
    o.tile_nc = pos(route_env("DFM_TILE_NC"));
    o.tile_w = pos(route_env("DFM_TILE_W"));
    o.wide_old = on(diag_env("DFM_WIDE_OLD"));
    o.wide_sub = num(diag_env("DFM_WIDE_SUB"), 1);
    o.cov_wave = on(diag_env("DFM_COV_WAVE"));
    if (const char* v = route_env("DFM_FCAR_MSG_BYTES")) { if (atoll(v) > 0) o.fcar_msg_cap = (size_t)atoll(v); }
    return o;
}
}  // namespace

struct dfm_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side = nullptr;            // data-independent kernels (gram, cov) run beside the collapse
    hipStream_t post = nullptr;            // meanscan of sub-batch s runs here, beside the collapse of sub-batch s+1
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_post = nullptr;
    std::vector<hipEvent_t> ev_sub;        // collapse of sub-batch s done
    const RouteOpts opt = route_opts_from_env();   // every switch, as the environment stood when this handle was created
    int num_cu = 256;                      // the device's compute units; DFM_NUM_CU (route): persistent grids sized for fewer
    bool in_pipe = false;                  // inside a sub-batch of pipe_run: no nesting
    // The handle's status word: its own 256-byte allocation, zeroed at creation and again by whoever READS a non-zero value
    // (status_check).  It is sticky between checks -- no memset per call: that was a 5 us fill kernel in front of every pass,
    // 2 % of the headline's step.  Device-pointer callers that never check see nothing; dfm_synchronize / dfm_check_status and
    // every host-pointer entry report (and clear) whatever was raised since the last check.
    int* status_dev = nullptr;
    int discarded_status = 0;              // status bits of earlier, unchecked device-pointer calls that a host-pointer entry cleared (status_epoch)
    DevBlock ws;                           // the workspace every entry point plans (make_plan) and sizes (ensure_ws) before it uses it
    const int* ck_fail_dev = nullptr; int ck_fail_n = 0;   // chunk_fail of the last launch on recursion_chunk_kernel (dfm_chunk_fallbacks)
    // EM on the fast path at Rp <= 8: the transition M-step is not launched behind the E-step but handed to the loadings step's
    // streaming launch (mstep_mfma.hip runs it as extra workgroups): em_iteration sets defer_em, enqueue_pass_fast parks the
    // arguments here
    bool defer_em = false, have_deferred_em = false;
    dfm::EmUpdArgs deferred_em;
    DevBlock odd;                          // panel / loadings / R with one all-missing series appended (odd N beyond the tilings, odd_pad)
    DevBlock fc;                           // dfm_forecast_batch_dev: the pass's T-row moments, the forecast tail, P and loglik when the
                                           // caller does not take them (beside h->ws: the pass itself may reallocate that);
                                           // dfm_forecast_ar_batch_dev: the padded panel, P and loglik likewise, one slice's messages
    DevBlock ss;                           // dfm_simsmooth_batch_dev: roots, the slice's pass parameters, smoothed means, logliks and
                                           // (no x_draw) difference panels -- beside h->ws for the same reason;
                                           // dfm_simsmooth_ar_batch_dev: the same, the difference panels always, one slice's messages
    DevBlock nw;                           // dfm_news_batch_dev: targets, the revised old panel, one forecast's xhat, the slice's pass
                                           // parameters, u / a vectors, smoothed means and (no weight) covariance panels
                                           // dfm_news_ar_batch_dev: the same on the output rows of the AR forecasts, with rho,
                                           // the u / d vectors of news_ar_rec_kernel and the whole smoothed state of the slice
    DevBlock sv;                           // dfm_irf_batch_dev / dfm_histdecomp_batch_dev: named / cum, S, S^-1, the Theta tables, shocks and
                                           // contribution paths, and the pass outputs the caller does not take; dfm_signirf_batch_dev:
                                           // the restrictions, their table, mask, counts, rotations and the kept slots' tables;
                                           // dfm_proxyirf_batch_dev: cum, the used rows, the instrument, S, S^-1, the Theta tables, the row
                                           // table, the slots' w and tables, the den table and the pass outputs the caller does not take
    DevBlock ft;                           // the two filter drivers: each one's own arrays first (dfm_filter_batch_dev: the padded loadings;
                                           // dfm_filter_ar_batch_dev: the quasi-differenced panel, its loadings and the fourth running sum),
                                           // then what filter_carve lays out for both: the collapse's per-period arrays, the moments the
                                           // caller does not take and the evaluation's running sums
    DevBlock gb;                           // dfm_gibbs_batch_dev: the sweep's factor path and the shared Gram roots of balanced panels
                                           // dfm_gibbs_ar_batch_dev: the sweep's [B][T - q][r] factor path
    DevBlock rw;                           // dfm_rolling_eval_batch_dev: origins, lags, the running sums [H + 1][N], then one slice's windows,
                                           // xhat, xvar, factor rows and logliks, and the slice's part of every output the caller does not take
                                           // dfm_diffusion_eval_batch_dev: origins, lags, the running sums, then one slice's windows, factors,
                                           // loadings, statistics and forecasts where the caller does not take them
    std::vector<int> sv_idx;               // host copy of named / cum while their upload is in flight
    std::vector<double> sv_z;              // dfm_proxyirf_batch_dev: host copy of the instrument while its upload is in flight
    const double* odd_panel_src = nullptr; int odd_panel_dims[3] = {0, 0, 0};   // the panel whose padded copy h->odd holds (odd_pad keep_panel)
    std::string prof_file;                 // DFM_PF_PROF_FILE with DFM_SCAN_ABL=256: phase stamps of the fused pass
    char err[512] = {0};
    // optional per-kernel timing (bench.py roofline leg): event pairs on the launch stream
    bool profiling = false;
    struct Ev { const char* name; hipEvent_t a, b; };   // name: the kernel the launcher dispatched to (static string)
    std::vector<Ev> events;
    std::vector<const char*> prof_names;                // distinct names of `events`, in order of first launch
};

enum KernelId { K_COLLAPSE = 0, K_RECURSION, K_MSTEP_STATS, K_MSTEP_SOLVE, K_PCA, K_SYNTH, K_PAD,
                K_COLLAPSE_DMA, K_GRAM, K_COV, K_MEANSCAN, K_PFILL, K_COLLAPSE_MFMA, K_ALS, K_OLS, K_BOOT, K_QUANT, K_COLLAPSE_WIDE, K_EM_UPDATE, K_CHOW, K_MSTEP_MFMA, K_GRAM_XX, K_PASS_FUSED, K_FC_TAIL, K_FC_FILL, K_FC_PAD, K_SS_PREP, K_SS_EXPAND, K_SS_PATH, K_SS_DIFF, K_SS_FINISH, K_SS_FILL, K_NW_REVISE, K_NW_GATHER, K_NW_GAMMA, K_NW_COV, K_NW_IMPACT, K_MF_TABLE, K_MF_MOMENTS, K_MF_SOLVE, K_SV_PREP, K_SV_IRF_FILL, K_SV_SHOCK, K_SV_PATH, K_SV_HD_FILL, K_FT_FILTER, K_FT_FILL, K_FT_EVAL, K_GB_GRAM, K_GB_LOAD, K_GB_VAR, K_SV_SIGN_TABLE, K_SV_SIGN, K_SV_SIGN_KEEP, K_PX_ROWS, K_PX_MOMENT, K_PX_SLOT_TABLE, K_PX_DEN, K_PX_FILL, K_PX_SHOCK, K_MF_SOLVE_BLOCKS, K_FCAR_BACK, K_FCAR_FWD, K_SSAR_PARAMS, K_SSAR_EXPAND, K_SSAR_DIFF, K_SSAR_FWD, K_SSAR_FINISH, K_GB_AR_SERIES, K_FTAR_FILTER, K_FTAR_FILL, K_FTAR_EVAL, K_NWAR_REVISE, K_NWAR_REC, K_NWAR_QC, K_NWAR_IMPACT, K_SIM_CELLS, K_SIMAR_CELLS, K_RW_WINDOW, K_RW_START, K_RW_SCORE, K_DI_START, K_DI_REGRESS, K_DI_SCORE, K_COUNT };
static const char* const kKernelNames[K_COUNT] = {"collapse_kernel", "recursion_kernel", "mstep_lam_kernel",
                                                  "mstep_solve_kernel", "pca_kernel", "synth_kernel",
                                                  "pad_params_kernel", "collapse_dma_kernel", "gram_kernel",
                                                  "cov_kernel", "meanscan_kernel", "pfill_kernel", "collapse_mfma_kernel", "als_kernel", "ols_kernel", "var_boot_kernel", "quantile_kernel", "collapse_wide_kernel", "em_update_kernel", "chow_kernel", "mstep_mfma_kernel", "gram_xx_kernel", "pass_fused_kernel", "forecast_tail_kernel", "forecast_fill_kernel", "forecast_pad_kernel", "simsmooth_prep_kernel", "simsmooth_expand_kernel", "simsmooth_path_kernel", "simsmooth_diff_kernel", "simsmooth_finish_kernel", "simsmooth_fill_kernel", "news_revise_kernel", "news_gather_kernel", "news_gamma_kernel", "news_cov_panel_kernel", "news_impact_kernel", "mf_table_kernel", "mf_moments_kernel", "mf_solve_kernel", "sv_prep_kernel", "sv_irf_fill_kernel", "sv_shock_kernel", "sv_path_kernel", "sv_hd_fill_kernel", "filter_kernel", "filter_fill_kernel", "filter_eval_kernel", "gibbs_gram_kernel", "gibbs_load_kernel", "gibbs_var_kernel", "sv_sign_table_kernel", "sv_sign_kernel", "sv_sign_keep_kernel", "px_rows_kernel", "px_moment_kernel", "px_slot_table_kernel", "px_den_kernel", "px_fill_kernel", "px_shock_kernel", "mf_solve_blocks_kernel", "forecast_ar_back_kernel", "forecast_ar_fwd_kernel", "simsmooth_ar_params_kernel", "simsmooth_ar_expand_kernel", "simsmooth_ar_diff_kernel", "simsmooth_ar_fwd_kernel", "simsmooth_ar_finish_kernel", "gibbs_ar_series_kernel", "filter_ar_kernel", "filter_ar_fill_kernel", "filter_ar_eval_kernel", "news_ar_revise_kernel", "news_ar_rec_kernel", "news_ar_qc_kernel", "news_ar_impact_kernel", "simulate_cells_kernel", "simulate_ar_cells_kernel", "rolling_window_kernel", "rolling_start_kernel", "rolling_score_kernel", "di_start_kernel", "di_regress_kernel", "di_score_kernel"};

namespace dfm { int handle_device(const dfm_handle* h) { return h->device; } }   // (probe.hip)

namespace {

int fail(dfm_handle* h, int code, const char* fmt, const char* detail = "") {
    if (h) snprintf(h->err, sizeof(h->err), fmt, detail);
    return code;
}
int hip_fail(dfm_handle* h, hipError_t e, const char* where) {
    if (h) snprintf(h->err, sizeof(h->err), "%s: %s", where, hipGetErrorString(e));
    return (int)e;
}
#define HIP_TRY(h, expr)                                   \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(h, _e, #expr); \
    } while (0)

// The element-wise kernels of this file: one thread per element, 256 per block, on h->stream.  n = threads wanted (>= 1).
template <class... KArgs, class... Args>
int launch_1d(dfm_handle* h, void (*kernel)(KArgs...), size_t n, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, static_cast<KArgs>(args)...);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

struct ProfScope {  // records an event pair around one kernel launch when profiling is on
    dfm_handle* h; int idx = -1; hipStream_t st;
    ProfScope(dfm_handle* h_, int kid, hipStream_t st_ = nullptr) : h(h_), st(st_ ? st_ : h_->stream) {
        if (!h->profiling) return;
        dfm_handle::Ev ev; ev.name = kKernelNames[kid];
        if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return;
        dfm::t_launched_kernel = nullptr;
        (void)hipEventRecord(ev.a, st);
        h->events.push_back(ev);
        idx = (int)h->events.size() - 1;
    }
    ~ProfScope() {
        if (idx < 0) return;
        (void)hipEventRecord(h->events[idx].b, st);
        // the launcher says which kernel it dispatched to (rocprofv3's name); the scope's id is only the default
        if (dfm::t_launched_kernel) h->events[idx].name = dfm::t_launched_kernel;
    }
};
// One kernel launch on h->stream under its ProfScope: HIP_TRY(h, expr) with kernel kid's event pair around it (h->err quotes expr
// as HIP_TRY does).  A launch on another stream, or a scope that holds more than the launch, still writes its ProfScope out.
#define HIP_LAUNCH(h, kid, expr)                           \
    do {                                                   \
        ProfScope ps(h, kid);                              \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(h, _e, #expr); \
    } while (0)

int pad_r(int r) { return pow2_ge(r) < 2 ? 2 : pow2_ge(r); }

struct Plan {  // byte offsets into the workspace (all 256-byte aligned)
    int Rp;
    int r = 0;                                     // the caller's factor count (columns r .. Rp - 1 of the padded Lam are zero)
    size_t LamP, AP, QP, P0P, mu0P;                // padded parameters (only used when r != Rp)
    size_t bcol, scol, ldrow, nobs, Ct, Cfull, ldfull;
    size_t ZJ, wtab, status, ncov;
    size_t ck_skip = (size_t)-1;                  // recursion_chunk.hip: replicates that failed their boundary check earlier in this EM run
    size_t ck_rows = (size_t)-1;                  // collapse_miss_kernel's rows + NaN masks (ct_build_kernel's input)
    size_t ck_scr = (size_t)-1, ck_obs = (size_t)-1, ck_cst = (size_t)-1, ck_term = (size_t)-1, ck_fail = (size_t)-1;   // recursion_chunk.hip (Rp = 8, general path)
    size_t Vwide = (size_t)-1;
    size_t tk_scr = (size_t)-1, tk_bytes = 0;   // recursion_tile.hip (Rp = 32, general path): the chunks' scratch (ck_fail is shared)
    size_t S11, S10, S00, P0s, f0s, fsm, Psm, Sxf, Sxx, Dmiss, llbuf, active;
    // balanced fast path (fastpath.hip); (size_t)-1 when the plan is for the general path
    size_t f_tab, f_E, f_stead, f_xi0, f_PT, f_llc, f_fill, f_PsInf, f_ssum;
    size_t ms_ws = (size_t)-1; int ms_wpr = 0;   // mstep_mfma partial sums (EM on the fast path)
    size_t mw_ws = (size_t)-1;                     // mstep_wide: Sxf, Sxx of the Rp = 32 loadings step (EM on the fast path)
    size_t mm_ws = (size_t)-1;                     // mstep_miss: V, [D | Sxf], Sxx, counts of the loadings step with missing cells
    bool ms_mfma = false, ms_wide = false, ms_miss = false;   // which of the three the EM iteration launches (none: mstep_lam_kernel)
    size_t Wwide = (size_t)-1;                     // W = lam / R of the Rp = 32 collapse (collapse_wide2.hip)
    bool fast;
    // covariance-form recursion (DFM_F_SINGULAR_Q) and companion states (dfm_*_varp_*): see RecursionArgs
    bool cov = false; int Rc = 0, rl = 0, kdim = 0, kb = 0, ka = 0, qsing = 0;
    size_t total;
};

size_t take(size_t& off, size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
}

// Sequential path with r <= 4: the state is padded to 8 so that the one-wave-per-replicate recursion (recursion_wave.hip)
// applies; collapse, loadings and the loadings M-step stay pad_r(r) wide (Plan::Rc).  DFM_NO_RECURSION_WAVE=1 turns it off.
// (one wave per replicate pays while the batch leaves SIMDs idle under the lane-group kernel: measured crossover
// at r = 4 between B = 1024 (0.39 vs 0.60 ms) and B = 4096 (1.52 vs 0.65 ms))
bool widens_small_r(const RouteOpts& o, int B) { return !o.no_rec_wave && B <= 1536; }
// Loadings step with missing cells on the matrix pipe (mstep_miss.hip) for loadings Rw wide with rl factors: what
// DFM_MSTEP_MISS (RouteOpts::mstep_miss_mode) says about this shape
bool mstep_miss_wanted(const RouteOpts& o, int Rw, int rl, int N) {
    return o.mstep_miss_mode && mstep_miss_supported(Rw, rl, N) && (o.mstep_miss_mode == 2 || mstep_needs_dmiss(Rw, N));
}
// A companion state behind the factors (dfm_*_varp_*, the AR and mixed-frequency models): see RecursionArgs.  table: the
// chunk-major observation table of collapse_miss_kernel is wanted where the shape allows it (enqueue_pass comp_table).
struct Companion { int Rc = 0, rl = 0, kdim = 0, kb = 0, ka = 0, qsing = 0; bool table = false; };
// the AR and mixed-frequency models: a k-wide state of r-wide lag blocks, VAR(nlag) inside it (recursion_comp.hip's route), observed
// on several blocks (rl = 0: loadings as wide as the state)
Companion lag_blocks(int k, int r, int nlag, unsigned flags) {
    Companion c;
    c.kdim = k; c.kb = r; c.ka = r * nlag; c.qsing = (flags & DFM_F_SINGULAR_Q) ? 1 : 0;
    return c;
}

// rows of the w_t scratch per replicate: T, plus (fast path, Rp >= 16) the chunk-major region of meanscan_mfma_kernel
static size_t wtab_rows(bool fast, int Rp, int T) {
    return (size_t)T + ((fast && Rp >= 16) ? (size_t)fast_scan_groups(Rp) * fast_chunk_len(Rp, T) : 0);
}
// The whole plan of one call: r = width of the state (r p of a companion model, whose flags carry DFM_F_SINGULAR_Q).  Nobody
// writes to a Plan afterwards.
Plan make_plan(const RouteOpts& o, int B, int T, int N, int r, unsigned flags, bool em, bool fast = false,
               const Companion& comp = Companion()) {
    Plan p;
    int Rp = pad_r(r);
    p.r = r;
    p.fast = fast;
    p.cov = (flags & DFM_F_SINGULAR_Q) != 0;
    if (!fast && !p.cov && Rp < 8 && widens_small_r(o, B)) {
        p.Rc = Rp; p.rl = Rp;
        Rp = 8;
    }
    p.Rp = Rp;
    const size_t d = sizeof(double), rr = (size_t)Rp * Rp, np = (size_t)Rp * (Rp + 1) / 2;
    size_t off = 0;
    p.LamP = take(off, (size_t)B * N * Rp * d);
    p.AP = take(off, B * rr * d);
    p.QP = take(off, B * rr * d);
    p.P0P = take(off, B * rr * d);
    p.mu0P = take(off, (size_t)B * Rp * d);
    p.bcol = take(off, (size_t)B * T * Rp * d);
    p.scol = take(off, (size_t)B * T * d);
    p.ldrow = take(off, (size_t)B * T * d);
    p.nobs = take(off, (size_t)B * T * sizeof(int));
    p.Ct = (flags & DFM_F_MAY_HAVE_MISSING) ? take(off, (size_t)B * T * np * d) : (size_t)-1;
    p.Cfull = take(off, B * rr * d);
    p.ldfull = take(off, (size_t)B * d);
    p.f_tab = p.f_E = p.f_stead = p.f_xi0 = p.f_PT = p.f_llc = p.f_fill = p.f_PsInf = p.f_ssum = (size_t)-1;
    p.ZJ = (size_t)-1;
    if (fast) {
        p.f_tab = take(off, (size_t)B * T * 3 * rr * d);
        p.f_E = take(off, (size_t)B * sizeof(int));
        p.f_stead = take(off, (size_t)B * fast_stead_mats(Rp) * rr * d);
        p.f_xi0 = take(off, (size_t)B * Rp * d);
        p.f_PT = take(off, B * rr * d);
        p.f_llc = take(off, (size_t)B * d);
        p.f_fill = take(off, (size_t)B * 2 * sizeof(int));
        p.f_PsInf = take(off, B * rr * d);
        p.f_ssum = take(off, (size_t)B * kSsumSlots * d);
        // (+ room for up to 8 sub-batches laid out as batches of their own: enqueue_pass_fast)
        if (collapse_wide2_supported(Rp, N)) p.Wwide = take(off, collapse_wide2_ws_bytes(B, N, Rp) + 8 * collapse_wide2_ws_bytes(1, N, Rp));
    } else {
        p.ZJ = take(off, (size_t)B * (T + 1) * 2 * rr * d);
        if (p.Rc == 0 && Rp == 32 && N > collapse_max_n(32) && collapse_wide2_supported(32, N)) {
            p.Wwide = take(off, collapse_wide2_ws_bytes(B, N, 32));
            p.Vwide = take(off, (size_t)B * N * 32 * d);      // lam / sqrt(R): the C_t kernel's table
        }
    }
    // (fast path, Rp >= 16: the mean scan on the matrix pipe keeps the steady part of w_t in a second, chunk-major region behind the
    // T natural rows -- scan_mfma32.hip)
    p.wtab = take(off, (size_t)B * wtab_rows(fast, Rp, T) * Rp * d);
    if (!fast && !p.cov && Rp == 8 && !o.no_chunk) {   // (184 KB per replicate at T = 500 that the sequential kernels never touch)
        p.ck_scr = take(off, recursion_chunk_scratch_bytes(B, T));
        p.ck_obs = take(off, recursion_chunk_obs_bytes(B, T));
        if (collapse_miss_supported(8, N)) p.ck_rows = take(off, recursion_chunk_rows_bytes(B, T));   // (also r <= 4 on the 8-wide state: CollapseArgs::lam_w)
        p.ck_cst = take(off, (size_t)B * 320 * d);
        p.ck_term = take(off, (size_t)B * 96 * d);
        p.ck_fail = take(off, (size_t)B * sizeof(int));
        p.ck_skip = take(off, (size_t)B * sizeof(int));
    }
    if (!fast && !p.cov && Rp == 32 && p.Rc == 0) {
        p.tk_bytes = recursion_tile_scratch_bytes(B, T);
        p.tk_scr = take(off, p.tk_bytes);
        p.ck_fail = take(off, (size_t)B * sizeof(int));
    }
    p.status = take(off, 256);
    p.ncov = take(off, (size_t)B * sizeof(int));
    p.S11 = p.S10 = p.S00 = p.P0s = p.f0s = p.fsm = p.Psm = p.Sxf = p.Sxx = p.Dmiss = p.llbuf = p.active = (size_t)-1;
    if (em) {
        p.S11 = take(off, B * rr * d);
        p.S10 = take(off, B * rr * d);
        p.S00 = take(off, B * rr * d);
        p.P0s = take(off, B * rr * d);
        p.f0s = take(off, (size_t)B * Rp * d);
        p.fsm = take(off, (size_t)B * T * Rp * d);
        p.Psm = take(off, (size_t)B * T * np * d);
        p.Sxf = take(off, B * rr * d);                       // S11^-1
        p.llbuf = take(off, (size_t)B * d);
        p.active = take(off, (size_t)B * sizeof(int));
        if (mstep_needs_dmiss(Rp, N)) p.Dmiss = take(off, (size_t)B * N * np * d);
        if (fast && mstep_mfma_supported(Rp, N)) {
            p.ms_wpr = ms_wpr(B, T);
            p.ms_ws = take(off, mstep_mfma_workspace(B, N, Rp, p.ms_wpr));
        }
        if (fast && mstep_wide_supported(Rp, N)) p.mw_ws = take(off, mstep_wide_workspace(B, N, Rp));
        // (sized for loadings as wide as the state, whatever a companion model narrows them to)
        if (!fast && mstep_miss_wanted(o, Rp, r < Rp ? r : Rp, N)) p.mm_ws = take(off, mstep_miss_workspace(B, T, N, Rp, r < Rp ? r : Rp));
    }
    if (comp.kdim > 0) {                                      // (always with p.cov: nothing above has set these)
        p.Rc = comp.Rc; p.rl = comp.rl; p.kdim = comp.kdim; p.kb = comp.kb; p.ka = comp.ka; p.qsing = comp.qsing;
        if (comp.table && collapse_miss_supported(8, N) && (size_t)B * recursion_chunk_len(T) <= 0x7fffffffu) {
            p.ck_rows = take(off, recursion_chunk_rows_bytes(B, T));    // rows + masks, the chunk-major table
            p.ck_obs = take(off, recursion_chunk_obs_bytes(B, T));
        }
    }
    // the loadings step this plan's EM iterations launch (em_iteration)
    p.ms_mfma = p.ms_ws != (size_t)-1 && !o.no_mstep_mfma;
    p.ms_wide = p.mw_ws != (size_t)-1 && !o.no_mstep_mfma;
    const int Rl = p.Rc ? p.Rc : Rp;                          // width of the loadings, their factor count
    p.ms_miss = p.mm_ws != (size_t)-1 && mstep_miss_wanted(o, Rl, p.Rc ? (p.rl ? p.rl : Rl) : (r < Rl ? r : Rl), N);
    p.total = off;
    return p;
}

int ensure_ws(dfm_handle* h, size_t bytes) {
    // every entry point sizes the workspace before it uses it: whatever chunk_fail flags the last pass left in the block are about to
    // be overwritten or freed -- dfm_chunk_fallbacks must not read them (enqueue_pass sets the pointer again behind its launch)
    h->ck_fail_dev = nullptr; h->ck_fail_n = 0;
    HIP_TRY(h, h->ws.grow(bytes));
    return 0;
}

// byte offset `off` of a block as a typed pointer; (size_t)-1 = "not planned" = null
template <class T>
T* at(const DevBlock& b, size_t off) {
    return off == (size_t)-1 ? nullptr : reinterpret_cast<T*>(static_cast<char*>(b.p) + off);
}
template <class T>
T* at(dfm_handle* h, size_t off) {
    return at<T>(h->ws, off);
}

// The device side of ONE call of a host-pointer entry point: one block that holds every array of the call, allocated for the
// call and freed when it returns.  The entry declares its arrays in the order they lie in the block -- in (copied in), out (copied
// back by finish), inout (both; back = false: copied in only) -- each with its element count and the variable that receives its
// device pointer; begin() allocates the sum and enqueues the uploads.  A null host pointer keeps its n elements of space and gets a
// null device pointer, which is what the _dev twins take to mean "not wanted"; an array that is to take no space when it is not
// wanted is declared with n = 0.  Zero-length arrays enqueue no copy.
// align: bytes every array starts on, at least its element size.  1 = packed; 256 where a kernel moves its rows 16 bytes at a time
// (forecast_fill_kernel).  Several kernels pick their store width from the alignment of the pointer they are given, so an entry's
// order and rounding are part of its results bit for bit.
class HostStage {
  public:
    explicit HostStage(dfm_handle* h, size_t align = 1) : h_(h), align_(align) {}
    ~HostStage() { if (buf_) (void)hipFree(buf_); }
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    template <class T> void in(const T* host, size_t n, T*& dev) { add(host, nullptr, host != nullptr, n, sizeof(T), &dev); }
    template <class T> void out(T* host, size_t n, T*& dev) { add(nullptr, host, host != nullptr, n, sizeof(T), &dev); }
    template <class T> void inout(T* host, size_t n, T*& dev, bool back = true) { add(host, back ? host : nullptr, host != nullptr, n, sizeof(T), &dev); }
    int begin() {
        const size_t bytes = (total_ + align_ - 1) / align_ * align_;      // (the last array's rounding belongs to the block too)
        if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf_), bytes)) return hip_fail(h_, e, "hipMalloc (host-pointer entry)");
        for (const Arr& a : arrs_) {
            *a.dev = a.wanted ? buf_ + a.off : nullptr;
            if (a.up && a.bytes) note(hipMemcpyAsync(buf_ + a.off, a.up, a.bytes, hipMemcpyHostToDevice, h_->stream), "hipMemcpyAsync (host to device)");
        }
        return 0;
    }
    // rc: what the _dev twin returned.  rc == 0: copies the outputs back and waits for them.  Returns rc, else the first failed copy.
    int finish(int rc) {
        if (rc == 0 && err_ == hipSuccess) {
            for (const Arr& a : arrs_)
                if (a.down && a.bytes) note(hipMemcpyAsync(a.down, buf_ + a.off, a.bytes, hipMemcpyDeviceToHost, h_->stream), "hipMemcpyAsync (device to host)");
            note(hipStreamSynchronize(h_->stream), "hipStreamSynchronize");
        }
        if (rc == 0 && err_ != hipSuccess) return hip_fail(h_, err_, where_);
        return rc;
    }

  private:
    struct Arr { const void* up; void* down; size_t off, bytes; void** dev; bool wanted; };
    template <class T>
    void add(const void* up, void* down, bool wanted, size_t n, size_t elem, T** dev) {
        const size_t al = align_ > elem ? align_ : elem;
        total_ = (total_ + al - 1) / al * al;
        arrs_.push_back(Arr{up, down, total_, n * elem, reinterpret_cast<void**>(dev), wanted});
        total_ += n * elem;
    }
    void note(hipError_t e, const char* where) { if (e != hipSuccess && err_ == hipSuccess) { err_ = e; where_ = where; } }
    dfm_handle* h_;
    size_t align_, total_ = 0;
    char* buf_ = nullptr;
    std::vector<Arr> arrs_;
    hipError_t err_ = hipSuccess;
    const char* where_ = "";
};

int check_dims(dfm_handle* h, int B, int T, int N, int r) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 1 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, T, N, r must be >= 1%s");
    if (r > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r > DFM_MAX_R (32)%s");
    return 0;
}
// panels with missing cells (and EM) go through collapse_kernel's register tiling
// plain = the factor model itself (loadings as wide as the state): at Rp = 32 cross-sections beyond the register tiling take
// the streaming collapse of config 4 in its variant for missing cells (collapse_wide2.hip)
int check_general_n(dfm_handle* h, int N, int r, bool plain = false) {
    if (plain && pad_r(r) == 32 && (collapse_wide2_supported(32, N) || collapse_wide2_supported(32, N + 1))) return 0;   // odd N: odd_pad
    if (N > collapse_max_n(pad_r(r)))
        return fail(h, DFM_E_DIMS, "N too large for this r on the path with missing cells / EM (collapse kernel register "
                                   "tiling: N <= 1024 for r <= 8, 512 for r <= 16; r > 16: 256, or any even N for the plain model)%s");
    return 0;
}

// EM: balanced panels keep the fast-path E-step at any N (the wide collapse has no register tiling); what bounds them
// is the loadings M-step (mstep_lam_kernel: lane = series, N <= 1024; BASELINE config 4 is N = 1000, r = 20).
int check_em_n(dfm_handle* h, int N, int r, bool fast);

// Embed caller parameters (factor dimension r) into the padded dimension Rp.
__global__ void pad_params_kernel(int B, int N, int r, int Rp, int Rl, const double* Lam, const double* A,
                                  const double* Q, const double* mu0, const double* P0, double* LamP,
                                  double* AP, double* QP, double* mu0P, double* P0P) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nl = (size_t)B * N * Rl, nm = (size_t)B * Rp * Rp, nv = (size_t)B * Rp;
    if (tid < nl) {
        const int k = tid % Rl;
        const size_t bn = tid / Rl;
        LamP[tid] = k < r ? Lam[bn * r + k] : 0.0;
    }
    if (tid < nm) {
        const int j = tid % Rp, i = (tid / Rp) % Rp;
        const size_t b = tid / ((size_t)Rp * Rp);
        const bool in = i < r && j < r;
        const double eye = (i == j) ? 1.0 : 0.0;
        AP[tid] = in ? A[(b * r + i) * r + j] : 0.0;
        QP[tid] = in ? Q[(b * r + i) * r + j] : eye;
        P0P[tid] = in ? P0[(b * r + i) * r + j] : eye;
    }
    if (tid < nv) {
        const int i = tid % Rp;
        const size_t b = tid / Rp;
        mu0P[tid] = i < r ? mu0[b * r + i] : 0.0;
    }
}

struct PaddedParams {
    const double *Lam, *A, *Q, *mu0, *P0;
};
// The buffers of one planned call.  Lam .. P0: the parameters in the layout the kernels read (padded, or the companion form), which
// an EM run updates in place; fsm, Psm, llbuf, active: what the E-steps of an EM plan write (null for a plain pass).  model_bufs points
// all of them into the workspace; a driver whose layout is the caller's points them at the caller's arrays instead.
struct ModelBufs {
    double *Lam, *A, *Q, *mu0, *P0, *fsm, *Psm, *llbuf;
    int* active;
    PaddedParams pp() const { return PaddedParams{Lam, A, Q, mu0, P0}; }
};
ModelBufs model_bufs(dfm_handle* h, const Plan& p) {
    return ModelBufs{at<double>(h, p.LamP), at<double>(h, p.AP), at<double>(h, p.QP), at<double>(h, p.mu0P), at<double>(h, p.P0P),
                     at<double>(h, p.fsm), at<double>(h, p.Psm), at<double>(h, p.llbuf), at<int>(h, p.active)};
}

int pad_params(dfm_handle* h, const Plan& p, int B, int N, int r, const double* Lam, const double* A,
               const double* Q, const double* mu0, const double* P0, PaddedParams* out) {
    if (r == p.Rp) {
        *out = PaddedParams{Lam, A, Q, mu0, P0};
        return 0;
    }
    const size_t n = (size_t)B * N * p.Rp > (size_t)B * p.Rp * p.Rp ? (size_t)B * N * p.Rp : (size_t)B * p.Rp * p.Rp;
    const ModelBufs mb = model_bufs(h, p);
    *out = mb.pp();
    return launch_1d(h, pad_params_kernel, n, B, N, r, p.Rp, p.Rc ? p.Rc : p.Rp, Lam, A, Q, mu0, P0, mb.Lam, mb.A, mb.Q, mb.mu0, mb.P0);
}


// ---- odd N beyond the register tiling, panel with missing cells, r > 16 ------------------------------------------------
// The streaming collapse for missing cells (collapse_wide2.hip) and the matrix-pipe loadings step (mstep_miss.hip) move
// 16-byte series pairs.  The reference's estimator takes any cross-section (dfm_functions.ipynb:352-366 exists because panels
// are unbalanced), so an odd N gets ONE series appended: every cell missing, loadings 0, R = 1.  Its contribution to b_t, C_t,
// n_t, s_t and sum log R over the observed cells is exactly 0, so the pass equals the N-series pass; the loadings step skips
// a series without observed cells (mmw_finish_kernel), and its parameters are dropped on the way out.
__global__ void pad_last_col_kernel(size_t rows, int N, const double* src, double* dst) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= rows * (size_t)(N + 1)) return;
    const size_t row = tid / (size_t)(N + 1);
    const int i = (int)(tid % (size_t)(N + 1));
    dst[tid] = i < N ? src[row * N + i] : __builtin_nan("");
}
// dst[b][n][k] (n <= N) from src[b][n][k] (n < N), `fill` for the appended row; N1 = rows of dst per b (N + 1), or N to un-pad
__global__ void copy_series_rows_kernel(size_t nb, int Ns, int Nd, int w, double fill, const double* src, double* dst) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= nb * (size_t)Nd * w) return;
    const int k = (int)(tid % w);
    const int n = (int)((tid / w) % Nd);
    const size_t b = tid / ((size_t)w * Nd);
    dst[tid] = n < Ns ? src[(b * Ns + n) * w + k] : fill;
}
struct OddPad { double *panel, *Lam, *R; };
// keep_panel: the call continues an EM run on the same panel (dfm_em_iterate_batch_dev with k > 0: one call per iteration from the
// multi-GPU drivers) -- the padded copy made at k = 0 is still in h->odd, only the loadings and variances are copied again
int odd_pad(dfm_handle* h, int B, int T, int N, int r, const double* panel, const double* Lam, const double* R, OddPad* out,
            bool keep_panel = false) {
    const size_t n_panel = (size_t)B * T * (N + 1), n_lam = (size_t)B * (N + 1) * r, n_R = (size_t)B * (N + 1);
    const size_t bytes = (n_panel + n_lam + n_R) * sizeof(double) + 768;
    if (bytes > h->odd.bytes) h->odd_panel_src = nullptr;      // (the padded copy goes with the old block)
    HIP_TRY(h, h->odd.grow(bytes));
    auto al = [](size_t n) { return (n + 31) & ~(size_t)31; };
    out->panel = static_cast<double*>(h->odd.p);
    out->Lam = out->panel + al(n_panel);
    out->R = out->Lam + al(n_lam);
    const bool same = keep_panel && h->odd_panel_src == panel && h->odd_panel_dims[0] == B && h->odd_panel_dims[1] == T && h->odd_panel_dims[2] == N;
    if (!same)
        if (int rc = launch_1d(h, pad_last_col_kernel, n_panel, (size_t)B * T, N, panel, out->panel)) return rc;
    h->odd_panel_src = panel; h->odd_panel_dims[0] = B; h->odd_panel_dims[1] = T; h->odd_panel_dims[2] = N;
    if (int rc = launch_1d(h, copy_series_rows_kernel, n_lam, (size_t)B, N, N + 1, r, 0.0, Lam, out->Lam)) return rc;
    return launch_1d(h, copy_series_rows_kernel, n_R, (size_t)B, N, N + 1, 1, 1.0, R, out->R);
}
// ... and, after an EM run on the padded problem, the N series' loadings and variances back into the caller's arrays
int odd_unpad(dfm_handle* h, int B, int N, int r, const OddPad& o, double* Lam, double* R) {
    if (int rc = launch_1d(h, copy_series_rows_kernel, (size_t)B * N * r, (size_t)B, N + 1, N, r, 0.0, o.Lam, Lam)) return rc;
    return launch_1d(h, copy_series_rows_kernel, (size_t)B * N, (size_t)B, N + 1, N, 1, 0.0, o.R, R);
}

struct EmOpts {          // all-null for a plain pass
    double *A_out = nullptr, *Q_out = nullptr, *mu0_out = nullptr, *P0_out = nullptr;
    int* active = nullptr; int* iters = nullptr; double* ll_path = nullptr;
    int k = 0, max_iter = 1; double tol = 0.0;
};

// Balanced panel, even N, plain pass: may this call take the fast path (fastpath.hip)?
bool fast_eligible(const RouteOpts& o, int N, int r, unsigned flags) {
    if (o.force_general || (flags & (DFM_F_MAY_HAVE_MISSING | DFM_F_SINGULAR_Q))) return false;
    return collapse_dma_supported(pad_r(r), N) || collapse_wide_supported(pad_r(r), N);
}
// ... and the E-steps of an EM run on it?
bool em_fast_eligible(const dfm_handle* h, int N, int r, unsigned flags) { return fast_eligible(h->opt, N, r, flags) && !h->opt.em_general; }

bool needs_odd_pad(const RouteOpts& o, bool fast, int N, int r, unsigned flags, int B) {
    if (fast) return false;
    // states up to 8 wide, panels with missing cells: collapse_miss_kernel's rows are moved 16 bytes at a time (even N).  With the
    // appended series the pass takes its table mode (+ recursion_chunk_kernel) instead of collapse_kernel + chunk_bridge_kernel:
    // the Stock-Watson window (N = 139) is such a panel.  (r <= 4 beyond 1536 replicates stays on the 4-wide lane-group kernels.)
    if (o.odd_pad8 && pad_r(r) <= 8 && (N & 1) && (flags & DFM_F_MAY_HAVE_MISSING) && !(flags & DFM_F_SINGULAR_Q) && collapse_miss_supported(8, N + 1) &&
        (pad_r(r) == 8 || widens_small_r(o, B)))
        return true;
    return pad_r(r) == 32 && (N & 1) && N > collapse_max_n(32) && collapse_wide2_supported(32, N + 1);
}

int check_em_n(dfm_handle* h, int N, int r, bool fast) {   // fast: em_fast_eligible
    if (fast) {
        if (N > 1024 && !mstep_mfma_supported(pad_r(r), N))
            return fail(h, DFM_E_DIMS, "N > 1024: the loadings M-step (one lane per series, 4 series per lane) does not cover this cross-section%s");
        return 0;
    }
    return check_general_n(h, N, r, true);
}

// ---- large batches of panels with missing cells (states 8 wide): sub-batches on two streams, two workspace slots ------------------
// The general path's workspace is 0.9 MB per replicate (table entries of every period): 7.4 GB at B = 8192, 59 GB at B = 65536, beside
// 0.8 MB of panel per replicate.  From 16 replicates per CU on, the batch runs as sub-batches of 8 per CU that alternate between the
// caller's stream and h->post, each stream with its own workspace slot: the workspace stops growing (3.7 GB), and the kernels of
// neighbouring sub-batches overlap.  What the overlap is worth, measured (B = 8192, C2 shape, 10 % missing; profiles/r06/README.md):
// nothing for the pass (3.80 ms as one batch; 4.13 / 4.01 / 3.79 / 3.84 ms with sub-batches of 512 / 1024 / 2048 / 4096 -- the collapse
// beside the recursion takes 0.43-0.57 ms per 1024 replicates instead of 0.25, the recursion 0.37-0.45 instead of 0.24: one wave of each
// on a SIMD compete for its VALU issue slots), 3 % for the EM iteration (7.86 -> 7.56-7.64 ms).  Replicates are independent: the results
// are bit for bit those of the one-batch call (tests/test_gpu_pipe.py).
// body(b0, bn): enqueue everything for replicates [b0, b0 + bn) on h->stream with h->ws as its workspace.
int pipe_sub(const dfm_handle* h) { return 8 * h->num_cu; }
bool pipe_eligible(const dfm_handle* h, int B, int N, int r, unsigned flags) {
    if (h->opt.no_pipe || h->in_pipe || !h->post) return false;
    if (pad_r(r) != 8 || !(flags & DFM_F_MAY_HAVE_MISSING) || (flags & DFM_F_SINGULAR_Q)) return false;
    return B >= 2 * pipe_sub(h) && collapse_miss_supported(8, N) && !h->opt.collapse_miss_old && !h->opt.no_chunk;
}
template <class Body>
int pipe_run(dfm_handle* h, int B, size_t slot_bytes, Body body) {
    const int Bs = pipe_sub(h), S = (B + Bs - 1) / Bs;
    size_t off = 0;
    take(off, slot_bytes);
    const size_t slot = take(off, slot_bytes), o_agg = take(off, (size_t)B * sizeof(int));   // slots at 0 and `slot`, then the flags
    if (int rc = ensure_ws(h, off)) return rc;
    char* base = static_cast<char*>(h->ws.p);
    int* agg = reinterpret_cast<int*>(base + o_agg);          // chunk_fail of every replicate (dfm_chunk_fallbacks)
    hipStream_t main = h->stream;
    HIP_TRY(h, hipEventRecord(h->ev_fork, main));
    HIP_TRY(h, hipStreamWaitEvent(h->post, h->ev_fork, 0));
    int rc = 0;
    bool have_fail = true;
    h->in_pipe = true;
    for (int s_ = 0; s_ < S && rc == 0; ++s_) {
        const int b0 = s_ * Bs, bn = (B - b0 < Bs) ? B - b0 : Bs;
        h->ws.p = base + (size_t)(s_ & 1) * slot;
        h->stream = (s_ & 1) ? h->post : main;
        rc = body(b0, bn);
        if (rc == 0) {
            if (h->ck_fail_dev && h->ck_fail_n == bn) {
                const hipError_t e = hipMemcpyAsync(agg + b0, h->ck_fail_dev, (size_t)bn * sizeof(int), hipMemcpyDeviceToDevice, h->stream);
                if (e != hipSuccess) rc = hip_fail(h, e, "hipMemcpyAsync(chunk_fail)");
            } else have_fail = false;
        }
    }
    h->in_pipe = false;
    h->ws.p = base; h->stream = main;
    (void)hipEventRecord(h->ev_post, h->post);
    (void)hipStreamWaitEvent(main, h->ev_post, 0);              // join (also after a failure: the slots are in use until then)
    h->ck_fail_dev = (rc == 0 && have_fail) ? agg : nullptr;
    h->ck_fail_n = (rc == 0 && have_fail) ? B : 0;
    return rc;
}

// ---- one pass on an already-planned workspace: what the caller hands over, the argument structs, the route, the schedules ----------
// out_r = factor dimension of the f_smooth / P_smooth layout (caller's r for a plain pass, Rp for EM-internal buffers); em: null
// for a plain pass
struct PassIo {
    int B, T, N, out_r;
    const double* panel; PaddedParams pp; const double* Rv; double *f_smooth, *P_smooth, *loglik; const EmOpts* em;
};
// the CollapseArgs fields that the balanced and the general path share
CollapseArgs collapse_args(dfm_handle* h, const Plan& p, const PassIo& io) {
    CollapseArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.B = io.B; ca.T = io.T; ca.N = io.N; ca.panel = io.panel; ca.Lam = io.pp.Lam; ca.Rv = io.Rv;
    ca.bcol = at<double>(h, p.bcol); ca.scol = at<double>(h, p.scol);
    ca.Cfull = at<double>(h, p.Cfull); ca.ldfull = at<double>(h, p.ldfull); ca.status = h->status_dev;
    return ca;
}

// The route of the balanced pass (fastpath.hip) as a value: which collapse, with which geometry, on which of the six schedules.
enum FastCollapse { FC_DMA, FC_MFMA, FC_WIDE, FC_WIDE2 };   // collapse_dma.hip (VALU), collapse_mfma.hip, collapse_wide.hip, collapse_wide2.hip
enum FastSchedule {
    FS_IN_ORDER,     // DFM_NO_SIDE=1: gram, cov, collapse, scan in order on the caller's stream
    FS_ONE_LAUNCH,   // pass_fused.hip
    FS_TWO_LAUNCH,   // [covariance workgroups | MFMA collapse] -> scan, one stream
    FS_WIDE_SUB,     // DFM_WIDE_SUB=n: n sub-batches of the wide2 collapse on side, their scans on the caller's stream
    FS_FORKED,       // cov on the caller's stream, collapse on side, (wide2) the P_smooth fill on post
    FS_SUBBATCH      // DFM_SUBBATCH=n: gram + cov on side, n collapses on the caller's stream, their scans on post
};
struct FastRoute {
    FastCollapse collapse = FC_DMA; KernelId kid = K_COLLAPSE_DMA;   // the collapse kernel and its profiling label
    int cvariant = 0;                    // launch_collapse_dma's variant (>= 200: the MFMA kernel)
    int wpr = 4;                         // period segments per replicate: CollapseArgs::wpr and FastArgs::nseg
    int ntile = 0;                       // wide kernels: sum_t s_t arrives as partials per tile of the collapse (FastArgs::ntile, scol)
    int bst = 0;                         // > 0: narrowed rows of b_t (CollapseArgs::bst, FastArgs::bst)
    bool fuse_gram = false;              // DFM_FUSE_GRAM=1 where cov_kernel can: no Gram launch
    bool cov_gram = false;               // whoever runs the covariance recursion forms its Gram matrices itself (FastArgs::Lam, Rv)
    bool fill = false, fill_late = false;   // P_smooth's data-independent rows by pfill_kernel; ... on post, behind the collapse
    FastSchedule sched = FS_FORKED; int S = 1;   // S: sub-batches of FS_SUBBATCH / FS_WIDE_SUB
    bool wide2() const { return collapse == FC_WIDE2; }
};
// Pure host code: the switches of the handle, the plan and the shape in, the route out.  want_P: the caller takes P_smooth.
FastRoute fast_route(const RouteOpts& o, const Plan& p, int B, int T, int N, int num_cu, bool want_P) {
    FastRoute rt;
    const int cv = o.collapse_variant;
    // collapse kernel of the balanced path: contraction on the matrix pipe where the shape allows it (collapse_mfma.hip), else the VALU
    // kernel (collapse_dma.hip); DFM_COLLAPSE_VARIANT < 200 forces the latter; outside the register tilings (or = 198): the wide kernel
    // Rp = 16 | 32 with an even N: the streaming collapse of collapse_wide2.hip (Rp = 16 used to take the VALU kernel: 1.4-2.1 TB/s)
    const bool wide2_ok = !o.wide_old && p.Wwide != (size_t)-1;      // (planned where collapse_wide2_supported says so: make_plan)
    const bool use_wide = (wide2_ok && cv == 0) || !collapse_dma_supported(p.Rp, N) || cv == 198;
    const bool use_mfma = !use_wide && collapse_mfma_supported(p.Rp, N) && (cv == 0 || cv >= 200);
    const bool use_wide2 = use_wide && wide2_ok;
    rt.collapse = use_wide2 ? FC_WIDE2 : use_wide ? FC_WIDE : use_mfma ? FC_MFMA : FC_DMA;
    rt.kid = use_wide ? K_COLLAPSE_WIDE : use_mfma ? K_COLLAPSE_MFMA : K_COLLAPSE_DMA;
    rt.cvariant = use_mfma ? (cv >= 200 ? cv : 200) : (cv == 199 ? 0 : cv);   // 199: the VALU kernel's default
    if (use_wide) rt.ntile = !use_wide2 ? collapse_wide_tiles(T) : collapse_wide2_tiles(T);
    // Rp = 32 on the streaming collapse: b_t rows 8 ceil(r / 8) doubles apart instead of 32 -- the padding components are exact zeros
    // that the mean scan (its only reader here) substitutes; at BASELINE config 4 (r = 20) a quarter of the 0.39 GB of b_t traffic
    if (use_wide2 && p.Rp == 32) rt.bst = 8 * ((p.r + 7) / 8);
    // MFMA collapse: as many period segments per replicate as the chip has resident wave slots for this batch
    // (3 workgroups x 4 waves on each CU), so that the launch is one balanced round
    if (use_mfma) {
        rt.wpr = o.collapse_wpr > 0 ? o.collapse_wpr : (num_cu * 12) / B;
        if (rt.wpr < 1) rt.wpr = 1;
        if (rt.wpr > 8) rt.wpr = 8;
        while (rt.wpr > 1 && T / rt.wpr < 8) --rt.wpr;     // keep segments a few row blocks long
    }
    rt.fuse_gram = cov_fuses_gram(p.Rp, N) && o.fuse_gram;
    rt.fill = !o.no_pfill && want_P;
    // Rp = 32 (config 4): the fill is 0.86 GB of stores -- beside the collapse they cost it 0.4 ms of its 1.13; beside the latency-bound
    // scan they are free.  So: cov -> [event] ; collapse (side) -> [event] ; fill on the third stream after both, scan on the caller's
    // stream after the collapse, join at the end.  (A trickle of these stores from a few persistent workgroups UNDER the collapse was
    // tried: the collapse lost what the scan gained -- profiles/r04/ab_pfill_trickle_c4.txt.)
    rt.fill_late = rt.fill && use_wide2;
    // Measured on MI355X (profiles/r01): every cross-stream event edge costs 7-25 us, more than the
    // overlap buys at B = 1024, so the default is one sub-batch; DFM_SUBBATCH keeps the knob for big batches.
    int S = o.subbatch > 0 ? o.subbatch : 1;
    if (S > B) S = B;
    if (use_wide2) S = 1;                                     // (its workspace -- W, tile queues -- is laid out for the whole batch)
    // Wide states (collapse_wide2), DFM_WIDE_SUB = n > 1 (diagnostics; default off): the batch in n sub-batches, each a complete
    // small batch of its own (own W workspace slice, own tile queues), the mean scan of sub-batch s beside the collapse of sub-batch
    // s + 1.  MEASURED SLOWER at config 4 (B = 256): 1.39 ms -> 1.56 (n = 2) -> 1.81 (n = 4).  The scan is a latency chain per
    // replicate -- 0.41 ms for 256 replicates, 0.46 ms for 128 -- so a sub-batch's scan hides nothing and the last one still runs alone.
    const int Sw = (use_wide2 && o.wide_sub > 1 && o.wide_sub <= 8 && B >= 32 * o.wide_sub) ? o.wide_sub : 1;
    if (o.no_side) rt.sched = FS_IN_ORDER;   // diagnostics: everything in order on the main stream
    else if (S > 1) { rt.sched = FS_SUBBATCH; rt.S = S; }
    // ONE launch: persistent workgroups, b_t / w_t and the covariance tables never leave the chip (pass_fused.hip)
    else if (o.pass_fused && use_mfma && pass_fused_supported(p.Rp, T, N) && cv == 0) rt.sched = FS_ONE_LAUNCH;
    // ONE stream, two launches: [Gram + covariance workgroups + P_smooth fill | streaming collapse] -> scan.
    // The covariance waves sit at the front of the collapse grid (resident first, no cross-stream events).
    else if (use_mfma && !rt.fuse_gram && !o.no_fuse_cov && collapse_mfma_fuses_cov(p.Rp, N)) rt.sched = FS_TWO_LAUNCH;
    else if (Sw > 1) { rt.sched = FS_WIDE_SUB; rt.S = Sw; }
    else rt.sched = FS_FORKED;
    // (FS_TWO_LAUNCH, DFM_FUSED_GRAM=0: gram_kernel as its own launch in front)
    rt.cov_gram = rt.fuse_gram || rt.sched == FS_ONE_LAUNCH || (rt.sched == FS_TWO_LAUNCH && o.fused_gram);
    return rt;
}

FastArgs fast_args(dfm_handle* h, const Plan& p, const PassIo& io, const CollapseArgs& ca, const FastRoute& rt) {
    FastArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = io.B; fa.T = io.T; fa.N = io.N; fa.r = io.out_r; fa.L = fast_chunk_len(p.Rp, io.T);
    fa.rstate = p.r;
    fa.A = io.pp.A; fa.Q = io.pp.Q; fa.mu0 = io.pp.mu0; fa.P0 = io.pp.P0;
    fa.Cfull = ca.Cfull; fa.ldfull = ca.ldfull;
    fa.tab = at<double>(h, p.f_tab); fa.E = at<int>(h, p.f_E); fa.stead = at<double>(h, p.f_stead);
    fa.xi0 = at<double>(h, p.f_xi0); fa.PT = at<double>(h, p.f_PT); fa.llc = at<double>(h, p.f_llc);
    fa.fill = at<int>(h, p.f_fill); fa.PsInf = at<double>(h, p.f_PsInf);
    fa.bcol = ca.bcol; fa.ssum = ca.ssum; fa.wtab = at<double>(h, p.wtab); fa.wrep = wtab_rows(true, p.Rp, io.T) * (size_t)p.Rp;
    if (rt.ntile) { fa.scol = ca.scol; fa.ntile = rt.ntile; }
    fa.bst = rt.bst; fa.nseg = rt.wpr;
    if (rt.cov_gram) { fa.Lam = io.pp.Lam; fa.Rv = io.Rv; }
    fa.f_smooth = io.f_smooth; fa.P_smooth = io.P_smooth; fa.loglik = io.loglik;
    fa.abl = h->opt.scan_abl;
    if (io.em) {   // EM: covariance sums from cov_kernel, E[f_0 | X] from meanscan (workspace slots of S10 / S00 reused)
        fa.SP11 = at<double>(h, p.S10); fa.SU = at<double>(h, p.S00); fa.P0s = at<double>(h, p.P0s);
        fa.f0s = at<double>(h, p.f0s);
    }
    return fa;
}
// after the scan: transition M-step + bookkeeping from the sufficient statistics
int em_update(dfm_handle* h, const Plan& p, const PassIo& io, const FastArgs& fa) {
    const EmOpts* em = io.em;
    if (!em) return 0;
    EmUpdArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.B = io.B; ua.T = io.T; ua.fsm = io.f_smooth; ua.f0s = fa.f0s; ua.SP11 = fa.SP11; ua.SU = fa.SU; ua.P0s = fa.P0s;
    ua.PT = fa.PT; ua.loglik = io.loglik; ua.S11 = at<double>(h, p.S11); ua.S11inv = at<double>(h, p.Sxf);
    ua.A_out = em->A_out; ua.Q_out = em->Q_out; ua.mu0_out = em->mu0_out; ua.P0_out = em->P0_out;
    ua.active = em->active; ua.iters = em->iters; ua.ll_path = em->ll_path; ua.k = em->k; ua.max_iter = em->max_iter;
    ua.tol = em->tol;
    if (h->defer_em) { h->deferred_em = ua; h->have_deferred_em = true; return 0; }
    HIP_LAUNCH(h, K_EM_UPDATE, launch_em_update(p.Rp, ua, h->stream));
    return 0;
}

// Gram matrix (+ W for the wide2 collapse) and the streaming collapse of this route, on stream `st`
hipError_t fast_gram(dfm_handle* h, const Plan& p, const FastRoute& rt, const CollapseArgs& ca, hipStream_t st) {
    if (rt.wide2()) return launch_wide_prep(ca, at<double>(h, p.Wwide), p.Rp, st, p.r);
    return gram_supported(p.Rp, ca.N) ? launch_gram(p.Rp, ca, st) : launch_gram_wide(p.Rp, ca, st);
}
hipError_t fast_collapse(dfm_handle* h, const Plan& p, const FastRoute& rt, const CollapseArgs& c, hipStream_t st) {
    if (rt.wide2()) return launch_collapse_wide2(c, at<double>(h, p.Wwide), p.Rp, p.r, h->num_cu, st);
    return rt.collapse == FC_WIDE ? launch_collapse_wide(p.Rp, c, st) : launch_collapse_dma(p.Rp, c, st, rt.cvariant);
}
// the idioms of the schedules: h->ev_sub grown to n events; an edge (record ev on `from`, `to` waits for it); the late P_smooth
// fill on post, behind the two events that say its inputs are written and the collapse has left the memory system to it --
// whoever calls it waits for h->ev_post on the caller's stream behind its scans
int grow_ev_sub(dfm_handle* h, int n) {
    while ((int)h->ev_sub.size() < n) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ev_sub.push_back(e);
    }
    return 0;
}
int edge(dfm_handle* h, hipEvent_t ev, hipStream_t from, hipStream_t to) {
    HIP_TRY(h, hipEventRecord(ev, from)); HIP_TRY(h, hipStreamWaitEvent(to, ev, 0));
    return 0;
}
int late_pfill(dfm_handle* h, const Plan& p, const FastArgs& fa, hipEvent_t cov_done, hipEvent_t collapse_done) {
    HIP_TRY(h, hipStreamWaitEvent(h->post, cov_done, 0));
    HIP_TRY(h, hipStreamWaitEvent(h->post, collapse_done, 0));
    { ProfScope ps(h, K_PFILL, h->post); HIP_TRY(h, launch_pfill(p.Rp, fa, h->post)); }
    HIP_TRY(h, hipEventRecord(h->ev_post, h->post));
    return 0;
}

int pass_in_order(dfm_handle* h, const Plan& p, const CollapseArgs& ca, const FastArgs& fa, const FastRoute& rt) {
    if (!rt.fuse_gram) HIP_LAUNCH(h, K_GRAM, fast_gram(h, p, rt, ca, h->stream));
    HIP_LAUNCH(h, K_COV, launch_cov(p.Rp, fa, h->stream));
    HIP_LAUNCH(h, rt.kid, fast_collapse(h, p, rt, ca, h->stream));
    HIP_LAUNCH(h, K_MEANSCAN, launch_meanscan(p.Rp, fa, h->stream));
    return 0;
}
// DFM_SCAN_ABL & 256 (diagnostics): the one-launch pass leaves phase stamps of every replicate in scol; with DFM_PF_PROF_FILE
// they are dumped there after every pass (synchronises)
int dump_pass_stamps(dfm_handle* h, const CollapseArgs& ca) {
    if (const char* f = diag_env("DFM_PF_PROF_FILE")) h->prof_file = f;
    if (h->prof_file.empty()) return 0;
    std::vector<double> st((size_t)ca.B * ca.T);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(st.data(), ca.scol, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (FILE* fp = fopen(h->prof_file.c_str(), "w")) {
        for (int bb = 0; bb < ca.B; ++bb) {
            fprintf(fp, "%d", bb);
            for (int k = 0; k < 56; ++k) fprintf(fp, " %.0f", st[(size_t)bb * ca.T + k]);
            fprintf(fp, "\n");
        }
        fclose(fp);
    }
    return 0;
}
int pass_one_launch(dfm_handle* h, const CollapseArgs& ca, const FastArgs& fa) {
    HIP_LAUNCH(h, K_PASS_FUSED, launch_pass_fused(ca, fa, h->opt.pass_nsw, h->opt.pass_ncov, h->opt.pf_wpark, h->num_cu, h->stream));
    return (h->opt.scan_abl & 256) ? dump_pass_stamps(h, ca) : 0;
}
int pass_two_launch(dfm_handle* h, const Plan& p, CollapseArgs& ca, FastArgs& fa, const FastRoute& rt) {
    if (!rt.cov_gram) HIP_LAUNCH(h, K_GRAM, fast_gram(h, p, rt, ca, h->stream));   // else the covariance workgroups compute their Gram matrices themselves
    ca.fuse_cov = &fa;
    HIP_LAUNCH(h, rt.kid, fast_collapse(h, p, rt, ca, h->stream));
    ca.fuse_cov = nullptr;
    if (fa.P_smooth) fa.abl |= 1;
    HIP_LAUNCH(h, K_MEANSCAN, launch_meanscan(p.Rp, fa, h->stream));
    return 0;
}
int pass_wide_sub(dfm_handle* h, const Plan& p, const CollapseArgs& ca, FastArgs& fa, const FastRoute& rt) {
    const int B = ca.B, T = ca.T, N = ca.N, Sw = rt.S;
    if (int rc = grow_ev_sub(h, Sw + 1)) return rc;
    const int bmax = (B + Sw - 1) / Sw;
    const size_t slice = collapse_wide2_ws_bytes(bmax, N, p.Rp);
    auto sub_lo = [&](int s_) { return (int)((long long)B * s_ / Sw); };
    auto sub_args = [&](int s_) {
        const int b0 = sub_lo(s_), b1 = sub_lo(s_ + 1);
        CollapseArgs c = ca;
        c.B = b1 - b0;
        c.panel = ca.panel + (size_t)b0 * T * N; c.Lam = ca.Lam + (size_t)b0 * N * p.Rp; c.Rv = ca.Rv + (size_t)b0 * N;
        c.bcol = ca.bcol + (size_t)b0 * T * (ca.bst > 0 ? ca.bst : p.Rp); c.scol = ca.scol + (size_t)b0 * T; c.ssum = ca.ssum + (size_t)b0 * kSsumSlots;
        c.Cfull = ca.Cfull + (size_t)b0 * p.Rp * p.Rp; c.ldfull = ca.ldfull + b0;
        return c;
    };
    auto sub_ws = [&](int s_) { return reinterpret_cast<double*>(at<char>(h, p.Wwide) + (size_t)s_ * slice); };
    for (int s_ = 0; s_ < Sw; ++s_) HIP_LAUNCH(h, K_GRAM, launch_wide_prep(sub_args(s_), sub_ws(s_), p.Rp, h->stream, p.r));
    if (int rc = edge(h, h->ev_fork, h->stream, h->side)) return rc;
    HIP_LAUNCH(h, K_COV, launch_cov(p.Rp, fa, h->stream));      // resident before the collapse fills the CUs
    HIP_TRY(h, hipEventRecord(h->ev_sub[Sw], h->stream));                         // covariance tables done
    for (int s_ = 0; s_ < Sw; ++s_) {
        { ProfScope ps(h, rt.kid, h->side); HIP_TRY(h, launch_collapse_wide2(sub_args(s_), sub_ws(s_), p.Rp, p.r, h->num_cu, h->side)); }
        HIP_TRY(h, hipEventRecord(h->ev_sub[s_], h->side));
    }
    if (rt.fill_late) {               // 0.86 GB of stores at config 4: beside the scan of the last sub-batch, not beside the collapse
        if (int rc = late_pfill(h, p, fa, h->ev_sub[Sw], h->ev_sub[Sw - 1])) return rc;
        fa.abl |= 1;
    }
    for (int s_ = 0; s_ < Sw; ++s_) {
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_sub[s_], 0));
        FastArgs fs = fa;
        fs.b0 = sub_lo(s_); fs.B = sub_lo(s_ + 1) - sub_lo(s_);
        HIP_LAUNCH(h, K_MEANSCAN, launch_meanscan(p.Rp, fs, h->stream));
    }
    if (rt.fill_late) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_post, 0));
    return 0;
}
int pass_forked(dfm_handle* h, const Plan& p, const CollapseArgs& ca, FastArgs& fa, const FastRoute& rt) {
    // The covariance kernel (128 waves, 224 VGPRs each) must be resident BEFORE the streaming collapse fills
    // every CU, or it waits for the collapse to drain (measured: 285 us instead of 90).  It therefore goes
    // first on the caller's stream, and the collapse is the forked work: its queue starts ~6 us later.
    if (!rt.fuse_gram || rt.wide2()) HIP_LAUNCH(h, K_GRAM, fast_gram(h, p, rt, ca, h->stream));   // 12 us, alone
    if (int rc = edge(h, h->ev_fork, h->stream, h->side)) return rc;
    HIP_LAUNCH(h, K_COV, (h->opt.cov_wave && p.Rp == 8 && !rt.fuse_gram) ? launch_cov_wave(fa, h->stream) : launch_cov(p.Rp, fa, h->stream));
    { ProfScope ps(h, rt.kid, h->side); HIP_TRY(h, fast_collapse(h, p, rt, ca, h->side)); }
    HIP_TRY(h, hipEventRecord(h->ev_join, h->side));
    if (rt.fill && !rt.fill_late) {   // the data-independent rows of P_smooth, beside the collapse
        HIP_LAUNCH(h, K_PFILL, launch_pfill(p.Rp, fa, h->stream));
        fa.abl |= 1;
    }
    if (rt.fill_late) {               // (why late: fast_route)
        if (int rc = grow_ev_sub(h, 1)) return rc;
        HIP_TRY(h, hipEventRecord(h->ev_sub[0], h->stream));            // cov_kernel's outputs
        if (int rc = late_pfill(h, p, fa, h->ev_sub[0], h->ev_join)) return rc;   // ... and not before the collapse is done
        fa.abl |= 1;
    }
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    HIP_LAUNCH(h, K_MEANSCAN, launch_meanscan(p.Rp, fa, h->stream));
    if (rt.fill_late) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_post, 0));
    return 0;
}
// gram + cov on the side stream, beside the streaming collapse on the main stream; the batch is cut
// into sub-batches so that the (latency-bound) meanscan of sub-batch s runs on a third stream beside the
// (bandwidth-bound) collapse of sub-batch s+1.
int pass_subbatch(dfm_handle* h, const Plan& p, const CollapseArgs& ca, const FastArgs& fa, const FastRoute& rt) {
    const int B = ca.B, S = rt.S;
    if (int rc = grow_ev_sub(h, S)) return rc;
    // fork: side and post start after everything already enqueued on the main stream (parameters, memsets)
    if (int rc = edge(h, h->ev_fork, h->stream, h->side)) return rc;
    HIP_TRY(h, hipStreamWaitEvent(h->post, h->ev_fork, 0));
    if (!rt.fuse_gram) { ProfScope ps(h, K_GRAM, h->side); HIP_TRY(h, fast_gram(h, p, rt, ca, h->side)); }
    { ProfScope ps(h, K_COV, h->side); HIP_TRY(h, launch_cov(p.Rp, fa, h->side)); }
    if (int rc = edge(h, h->ev_join, h->side, h->post)) return rc;
    for (int s = 0; s < S; ++s) {
        const int b0 = (int)((long long)B * s / S), b1 = (int)((long long)B * (s + 1) / S);
        CollapseArgs cs = ca;
        cs.b0 = b0; cs.B = b1 - b0;
        HIP_LAUNCH(h, rt.kid, launch_collapse_dma(p.Rp, cs, h->stream, rt.cvariant));   // (the one collapse that takes b0)
        if (int rc = edge(h, h->ev_sub[s], h->stream, h->post)) return rc;
        FastArgs fs = fa;
        fs.b0 = b0; fs.B = b1 - b0;
        { ProfScope ps(h, K_MEANSCAN, h->post); HIP_TRY(h, launch_meanscan(p.Rp, fs, h->post)); }
    }
    return edge(h, h->ev_post, h->post, h->stream);   // join
}

int enqueue_pass_fast(dfm_handle* h, const Plan& p, const PassIo& io) {
    const FastRoute rt = fast_route(h->opt, p, io.B, io.T, io.N, h->num_cu, io.P_smooth != nullptr);
    CollapseArgs ca = collapse_args(h, p, io);
    ca.ssum = at<double>(h, p.f_ssum); ca.wpr = rt.wpr; ca.bst = rt.bst;
    FastArgs fa = fast_args(h, p, io, ca, rt);
    int rc = 0;
    switch (rt.sched) {
        case FS_IN_ORDER: rc = pass_in_order(h, p, ca, fa, rt); break;
        case FS_ONE_LAUNCH: rc = pass_one_launch(h, ca, fa); break;
        case FS_TWO_LAUNCH: rc = pass_two_launch(h, p, ca, fa, rt); break;
        case FS_WIDE_SUB: rc = pass_wide_sub(h, p, ca, fa, rt); break;
        case FS_FORKED: rc = pass_forked(h, p, ca, fa, rt); break;
        case FS_SUBBATCH: rc = pass_subbatch(h, p, ca, fa, rt); break;
    }
    return rc ? rc : em_update(h, p, io, fa);
}

// the general path: which recursion launch_recursion will pick, as far as enqueue_pass has to know, and which collapse feeds it
enum GeneralCollapse {
    GC_COMP_TABLE,   // companion state: collapse_miss_kernel's chunk table, then chunk_unbridge_kernel
    GC_CHUNK_TABLE,  // collapse_miss_kernel writes the table recursion_chunk_kernel reads
    GC_MISS,         // collapse_miss_kernel, rows in the sequential kernels' layout
    GC_WIDE2,        // Rp = 32 beyond the register tiling: wide prep, collapse_wide2, ct_miss_wide
    GC_PLAIN         // collapse_kernel
};
struct GeneralRoute { bool chunked, tiled; int ct_r, Rcol; GeneralCollapse collapse; };
GeneralRoute general_route(const RouteOpts& o, const Plan& p, int N, const RecursionArgs& ra) {
    GeneralRoute g;
    // (the kernel files' own predicates, asked once)
    g.chunked = ra.wave && recursion_chunk_supported(p.Rp, ra); g.tiled = ra.wave && recursion_tile_supported(p.Rp, ra);
    g.Rcol = p.Rc ? p.Rc : p.Rp;
    // C_t rows: the packed leading block when recursion_tile_kernel reads them (it executes ceil(r / 4) block pivots of the 32-wide
    // state: the rest is padding whose entries equal Cfull's), the full Rp (Rp + 1) / 2 layout for the other recursion kernels
    g.ct_r = 0;
    if (g.tiled && p.Wwide != (size_t)-1 && N > collapse_max_n(g.Rcol) && ct_miss_wide_compact_ok(N, 4 * ((p.r + 3) / 4))) g.ct_r = 4 * ((p.r + 3) / 4);
    // the time-chunked recursion reads one table row per period (C_t, b_t, s_t, n_t log 2 pi + log det R_t): at Rp = 8 with loadings as
    // wide as the state collapse_miss_kernel writes it directly
    // (r <= 4 widened to the 8-wide state, Plan::Rc = 2 / 4: the kernel pads the loadings with zero columns in its LDS tables --
    // CollapseArgs::lam_w -- and the table is the 8-wide one the chunks read anyway; collapse_kernel<4> + chunk_bridge_kernel took
    // 0.25 ms per 1024 replicates of the Stock-Watson window where this takes 0.1)
    const bool narrow_tab = p.Rc > 0 && p.Rc < 8 && p.kdim == 0 && p.rl == p.Rc && !o.narrow_tab_off;
    const bool table = g.chunked && !o.collapse_miss_old && (p.Rc == 0 || narrow_tab);
    // companion states (VAR(p) factor dynamics) with loadings up to 4 wide: the same table, then EVERY replicate's rows written
    // back in the layout the sequential kernels read (chunk_unbridge_kernel<Rc>: b_t, s_t, C_t of every period, nobs = 0) --
    // collapse_kernel<4> took 0.235 ms per 1024 replicates of the Stock-Watson window where these two take 0.12
    const bool comp_table = p.kdim > 0 && p.kb == 0 && p.Rc > 0 && p.Rc < 8 && p.ck_rows != (size_t)-1 && p.ck_obs != (size_t)-1 &&
                            collapse_miss_supported(8, N);
    if (comp_table) g.collapse = GC_COMP_TABLE;
    else if (table && p.ck_rows != (size_t)-1 && collapse_miss_supported(8, N) && (p.Rc == 0 ? g.Rcol == 8 : true)) g.collapse = GC_CHUNK_TABLE;
    else if (!o.collapse_miss_old && collapse_miss_supported(g.Rcol, N)) g.collapse = GC_MISS;
    else if (p.Wwide != (size_t)-1 && N > collapse_max_n(g.Rcol)) g.collapse = GC_WIDE2;   // (config 4 with missing cells)
    else g.collapse = GC_PLAIN;
    return g;
}
RecursionArgs recursion_args(dfm_handle* h, const Plan& p, const PassIo& io, const CollapseArgs& ca) {
    const EmOpts* em = io.em;
    RecursionArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.B = io.B; ra.T = io.T; ra.N = io.N; ra.r = io.out_r;
    ra.rstate = p.r; ra.cov = p.cov ? 1 : 0; ra.Rc = p.Rc; ra.rl = p.rl; ra.kdim = p.kdim; ra.kb = p.kb; ra.ka = p.ka; ra.qsing = p.qsing; ra.wave = h->opt.no_rec_wave ? 0 : 1;
    ra.pair_bmax = h->opt.pair_bmax >= 0 ? h->opt.pair_bmax : 4 * h->num_cu;
    ra.A = io.pp.A; ra.Q = io.pp.Q; ra.mu0 = io.pp.mu0; ra.P0 = io.pp.P0;
    ra.bcol = ca.bcol; ra.scol = ca.scol; ra.nobs = ca.nobs; ra.ldrow = ca.ldrow; ra.Ct = ca.Ct;
    ra.Cfull = ca.Cfull; ra.ldfull = ca.ldfull;
    ra.ZJtab = at<double>(h, p.ZJ); ra.wtab = at<double>(h, p.wtab);
    ra.chunk_scr = at<double>(h, p.ck_scr); ra.chunk_W = h->opt.chunk_w; ra.chunk_tol = h->opt.chunk_tol; ra.chunk_obs = at<double>(h, p.ck_obs); ra.chunk_cst = at<double>(h, p.ck_cst); ra.chunk_term = at<double>(h, p.ck_term); ra.chunk_fail = at<int>(h, p.ck_fail);
    ra.chunk_skip = at<int>(h, p.ck_skip);
    ra.tile_scr = at<double>(h, p.tk_scr); ra.tile_scr_bytes = p.tk_bytes; ra.tile_nc = h->opt.tile_nc; ra.tile_w = h->opt.tile_w; ra.num_cu = h->num_cu;
    ra.f_smooth = io.f_smooth; ra.P_smooth = io.P_smooth; ra.loglik = io.loglik;
    ra.ncov = at<int>(h, p.ncov);
    if (em) {
        ra.S11 = at<double>(h, p.S11); ra.S10 = at<double>(h, p.S10); ra.S00 = at<double>(h, p.S00);
        ra.f0s = at<double>(h, p.f0s); ra.P0s = at<double>(h, p.P0s); ra.S11inv = at<double>(h, p.Sxf);
        ra.A_out = em->A_out; ra.Q_out = em->Q_out; ra.mu0_out = em->mu0_out; ra.P0_out = em->P0_out;
        ra.active = em->active; ra.iters = em->iters; ra.ll_path = em->ll_path;
        ra.k = em->k; ra.max_iter = em->max_iter; ra.tol = em->tol;
    }
    return ra;
}

// Enqueue collapse + recursion for already-planned workspace.
int enqueue_pass(dfm_handle* h, const Plan& p, int B, int T, int N, int out_r, const double* panel,
                 const PaddedParams& pp, const double* Rv, double* f_smooth, double* P_smooth, double* loglik,
                 const EmOpts* em) {
    const PassIo io{B, T, N, out_r, panel, pp, Rv, f_smooth, P_smooth, loglik, em};
    if (p.fast) return enqueue_pass_fast(h, p, io);
    CollapseArgs ca = collapse_args(h, p, io);
    ca.nobs = at<int>(h, p.nobs); ca.ldrow = at<double>(h, p.ldrow); ca.Ct = at<double>(h, p.Ct);
    ca.kreal = (p.kdim > 0 && p.Rc == 0) ? p.kdim : 0;          // (companion state observed on every block: the AR idiosyncratic model)
    RecursionArgs ra = recursion_args(h, p, io, ca);
    const GeneralRoute g = general_route(h->opt, p, N, ra);
    ra.ct_r = ca.ct_r = g.ct_r;
    switch (g.collapse) {
        case GC_COMP_TABLE: {
            ca.lam_w = p.Rc;
            ca.obs_chunk = at<double>(h, p.ck_rows);
            ca.obs_table = at<double>(h, p.ck_obs); ca.obs_L = recursion_chunk_len(T);
            HIP_LAUNCH(h, K_COLLAPSE, launch_collapse_miss(ca, h->num_cu, h->stream));
            RecursionArgs ua = ra;                                // (ua.chunk_obs: that table)
            ua.chunk_fail = nullptr;                              // (no flags: every replicate)
            HIP_TRY(h, launch_chunk_unbridge(ua, h->stream));
            break;
        }
        case GC_CHUNK_TABLE:
            ca.lam_w = p.Rc;
            ca.obs_chunk = at<double>(h, p.ck_rows);
            ca.obs_table = ra.chunk_obs; ca.obs_L = recursion_chunk_len(T);
            ra.chunk_obs_ready = 1;
            HIP_LAUNCH(h, K_COLLAPSE, launch_collapse_miss(ca, h->num_cu, h->stream));
            break;
        case GC_MISS: HIP_LAUNCH(h, K_COLLAPSE, launch_collapse_miss(ca, h->num_cu, h->stream)); break;
        case GC_WIDE2: {
            double* W = at<double>(h, p.Wwide);
            double* V = at<double>(h, p.Vwide);
            HIP_LAUNCH(h, K_GRAM, launch_wide_prep(ca, W, 32, h->stream, 0, V));
            HIP_LAUNCH(h, K_COLLAPSE_WIDE, launch_collapse_wide2(ca, W, 32, p.r, h->num_cu, h->stream));
            HIP_LAUNCH(h, K_COLLAPSE, launch_ct_miss_wide(ca, W, p.r, h->stream, V));
            break;
        }
        case GC_PLAIN: HIP_LAUNCH(h, K_COLLAPSE, launch_collapse(g.Rcol, ca, h->stream)); break;
    }
    h->ck_fail_dev = nullptr; h->ck_fail_n = 0;
    if (g.chunked || (g.tiled && recursion_tile_writes_fail(ra))) { h->ck_fail_dev = ra.chunk_fail; h->ck_fail_n = B; }
    HIP_LAUNCH(h, K_RECURSION, launch_recursion(p.Rp, ra, h->stream));
    return 0;
}

// dst[b][i][j] = src[b][i][j], i < rd, j < cd (un-padding of parameters / smoother outputs)
__global__ void copy_block_kernel(size_t nb, int rs, int cs, int rd, int cd, const double* src, double* dst) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = nb * rd * cd;
    if (tid >= n) return;
    const int j = tid % cd;
    const int i = (tid / cd) % rd;
    const size_t b = tid / ((size_t)cd * rd);
    dst[tid] = src[(b * rs + i) * cs + j];
}
int copy_block(dfm_handle* h, size_t nb, int rs, int cs, int rd, int cd, const double* src, double* dst) {
    return launch_1d(h, copy_block_kernel, nb * rd * cd, nb, rs, cs, rd, cd, src, dst);
}

// One EM iteration on PADDED, writable device parameters (mb.Lam [B][N][Rp], A/Q/P0 [B][Rp][Rp], mu0 [B][Rp]).
int em_iteration(dfm_handle* h, const Plan& p, int B, int T, int N, const double* panel, const ModelBufs& mb, double* Rv,
                 const EmOpts& eo) {
    const int Rp = p.Rc ? p.Rc : p.Rp;          // width of the loadings (narrower than the state for a companion model)
    h->defer_em = p.ms_mfma && p.Rp <= 8 && !h->opt.no_defer_em;  // the transition M-step rides in the loadings step's launch
    h->have_deferred_em = false;
    const int rc_pass = enqueue_pass(h, p, B, T, N, Rp, panel, mb.pp(), Rv, mb.fsm, mb.Psm, mb.llbuf, &eo);
    h->defer_em = false;
    if (rc_pass) return rc_pass;
    MstepArgs ma;
    ma.B = B; ma.T = T; ma.N = N; ma.r = Rp;
    ma.panel = panel; ma.fsm = mb.fsm; ma.Psm = mb.Psm;
    ma.S11 = at<double>(h, p.S11); ma.S11inv = at<double>(h, p.Sxf);
    ma.Dmiss = mstep_needs_dmiss(Rp, N) ? at<double>(h, p.Dmiss) : nullptr;
    ma.active = eo.active; ma.Lam_out = mb.Lam; ma.R_out = Rv; ma.lam_stride = Rp; ma.min_cells = 1;
    if (p.ms_mfma) {   // balanced panel: second panel read on the matrix pipe
        ProfScope ps(h, K_MSTEP_MFMA);
        HIP_TRY(h, launch_mstep_mfma(Rp, ma, p.ms_wpr, at<double>(h, p.ms_ws), h->stream, h->have_deferred_em ? &h->deferred_em : nullptr));
        h->have_deferred_em = false;
        return 0;
    }
    if (p.ms_wide) {   // ... Rp = 32 (config 4): the same on the streaming machinery of its collapse
        HIP_LAUNCH(h, K_MSTEP_MFMA, launch_mstep_wide(ma, at<double>(h, p.mw_ws), Rp, p.r, h->num_cu, h->stream));
        return 0;
    }
    if (p.ms_miss) {   // panels with missing cells: both contractions of the loadings step as one product per replicate on the matrix pipe
        const int rl = p.Rc ? (p.rl ? p.rl : Rp) : (p.r < Rp ? p.r : Rp);     // the loadings' factor count
        HIP_LAUNCH(h, K_MSTEP_STATS, launch_mstep_miss(ma, at<double>(h, p.mm_ws), Rp, rl, h->num_cu, h->stream));
        return 0;
    }
    if (ma.Dmiss)
        HIP_TRY(h, hipMemsetAsync(ma.Dmiss, 0, (size_t)B * N * (Rp * (Rp + 1) / 2) * sizeof(double), h->stream));
    HIP_LAUNCH(h, K_MSTEP_STATS, launch_mstep_lam(Rp, ma, h->stream));
    return 0;
}

// The loop of every EM driver: iterations k_first .. k_end - 1 of a run of max_iter, one(eo) enqueues iteration eo.k; the transition
// M-step of every iteration writes mb's parameters, and mb.active are the device flags.  With bookkeeping (loglik_path; iters and the
// flags go with it) a run that starts at 0 gets its path NaN-filled and its counts zeroed, and with poll && tol > 0 the loop stops
// launching once no replicate of this batch is active.
template <class One>
int em_loop(dfm_handle* h, int B, int k_first, int k_end, int max_iter, double tol, double* loglik_path, int* iters,
            const ModelBufs& mb, bool poll, One one) {
    if (loglik_path && k_first == 0) {
        HIP_TRY(h, hipMemsetAsync(loglik_path, 0xFF, (size_t)B * max_iter * sizeof(double), h->stream));  // NaN
        HIP_TRY(h, hipMemsetAsync(iters, 0, (size_t)B * sizeof(int), h->stream));
    }
    const bool stop_early = poll && loglik_path && tol > 0.0;
    std::vector<int> act_host(stop_early ? (size_t)B : 0);
    for (int k = k_first; k < k_end; ++k) {
        EmOpts eo;
        eo.A_out = mb.A; eo.Q_out = mb.Q; eo.mu0_out = mb.mu0; eo.P0_out = mb.P0;
        eo.active = mb.active; eo.iters = iters; eo.ll_path = loglik_path; eo.k = k; eo.max_iter = max_iter; eo.tol = tol;
        if (int rc = one(eo)) return rc;
        if (stop_early && k + 1 < k_end) {
            HIP_TRY(h, hipMemcpyAsync(act_host.data(), mb.active, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            bool any = false;
            for (int b = 0; b < B; ++b) any = any || act_host[b] != 0;
            if (!any) break;
        }
    }
    return 0;
}

// The results of an EM run from the plan's layout into the caller's.  r = the caller's factor count, a_cols = columns of its A (r; r p
// of a VAR(p)), kw = width of its mu0 / P0 (r; the companion state's k), rows = periods of the smoother outputs.  What mb already
// points at the caller's array is not copied: the E-steps or the M-step wrote it in place.  Lam = null: the loadings are not mb's
// to give back (the driver's series step keeps them in the caller's array).
int unpad_results(dfm_handle* h, const Plan& p, int B, int N, int rows, int r, int a_cols, int kw, const ModelBufs& mb, double* Lam,
                  double* A, double* Q, double* mu0, double* P0, double* f_smooth, double* P_smooth) {
    const int Rk = p.Rp, Rl = p.Rc ? p.Rc : p.Rp;            // state width; loadings width, which the smoother outputs share
    const int np = r * (r + 1) / 2, npl = Rl * (Rl + 1) / 2;
    if (Lam && Lam != mb.Lam) if (int rc = copy_block(h, (size_t)B * N, 1, Rl, 1, r, mb.Lam, Lam)) return rc;
    if (A != mb.A) {
        if (int rc = copy_block(h, B, Rk, Rk, r, a_cols, mb.A, A)) return rc;
        if (int rc = copy_block(h, B, Rk, Rk, r, r, mb.Q, Q)) return rc;
        if (int rc = copy_block(h, B, Rk, Rk, kw, kw, mb.P0, P0)) return rc;
        if (int rc = copy_block(h, B, 1, Rk, 1, kw, mb.mu0, mu0)) return rc;
    }
    if (f_smooth && f_smooth != mb.fsm) if (int rc = copy_block(h, (size_t)B * rows, 1, Rl, 1, r, mb.fsm, f_smooth)) return rc;
    if (P_smooth && P_smooth != mb.Psm) if (int rc = copy_block(h, (size_t)B * rows, 1, npl, 1, np, mb.Psm, P_smooth)) return rc;
    return 0;
}

// ---- the model drivers ---------------------------------------------------------------------------------------------------------
// Every driver below (em_run, varp_run, the AR pair, the mixed-frequency pair, obs_em_run) is the same procedure around its own
// series step:
//   1. check the arguments                     check_dims / check_em_n / check_general_n, ar_check, mf_check
//   2. plan the call                           make_plan
//   3. size the workspace                      arrays behind the plan: off = p.total, then take(off, bytes); ensure_ws(h, off)
//   4. embed the caller's parameters           model_bufs, then pad_params (padded layout) or companion_pad (companion form)
//   5. run the pass, or the EM loop            enqueue_pass; em_loop around em_iteration or the family's own iteration
//   6. cut the results into the caller's layout   unpad_results (and odd_unpad after a run on a panel that odd_pad widened)
// The AR and the mixed-frequency model have a pass and an EM driver: ar_plan / mf_plan do steps 2 and 3 for both.

// Shared driver of dfm_em_step_batch_dev (max_iter = 1, no bookkeeping), dfm_em_batch_dev (iterations 0 .. max_iter-1,
// stops launching once no replicate of THIS batch is active) and dfm_em_iterate_batch_dev (iteration k_first only, the
// caller owns `active` and decides when to stop: the multi-GPU drivers).
int em_run(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R, double* A,
           double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
           double* loglik_single, double* f_smooth, double* P_smooth, unsigned flags, int k_first = 0, int k_count = -1,
           int* active_ext = nullptr) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    const bool fast = em_fast_eligible(h, N, r, flags);
    if (int rc = check_em_n(h, N, r, fast)) return rc;
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    HIP_TRY(h, hipSetDevice(h->device));
    if (needs_odd_pad(h->opt, fast, N, r, flags, B)) {   // odd N beyond the tilings: one all-missing series appended
        OddPad o;
        if (int rc = odd_pad(h, B, T, N, r, panel, Lam, R, &o, k_first > 0)) return rc;
        // (the appended series is missing in EVERY period: the padded problem has missing cells whatever the caller said about N)
        if (int rc = em_run(h, B, T, N + 1, r, o.panel, o.Lam, o.R, A, Q, mu0, P0, max_iter, tol, loglik_path, iters, loglik_single,
                            f_smooth, P_smooth, flags | DFM_F_MAY_HAVE_MISSING, k_first, k_count, active_ext)) return rc;
        return odd_unpad(h, B, N, r, o, Lam, R);
    }
    if (pipe_eligible(h, B, N, r, flags)) {     // sub-batches as EM runs of their own on two streams (pipe_run)
        const Plan ps = make_plan(h->opt, pipe_sub(h), T, N, r, flags, true, false);
        const size_t rr = (size_t)r * r, np = (size_t)r * (r + 1) / 2;
        return pipe_run(h, B, ps.total, [&](int b0, int bn) -> int {
            return em_run(h, bn, T, N, r, panel + (size_t)b0 * T * N, Lam + (size_t)b0 * N * r, R + (size_t)b0 * N, A + b0 * rr, Q + b0 * rr,
                          mu0 + (size_t)b0 * r, P0 + b0 * rr, max_iter, tol, loglik_path ? loglik_path + (size_t)b0 * max_iter : nullptr,
                          iters ? iters + b0 : nullptr, loglik_single ? loglik_single + b0 : nullptr,
                          f_smooth ? f_smooth + (size_t)b0 * T * r : nullptr, P_smooth ? P_smooth + (size_t)b0 * T * np : nullptr, flags,
                          k_first, k_count, active_ext ? active_ext + b0 : nullptr);
        });
    }
    // balanced panels: E-step on the fast path (collapse on the matrix pipe, time-parallel scan), transition
    // M-step by em_update_kernel; panels with missing cells: recursion_kernel does both
    const Plan p = make_plan(h->opt, B, T, N, r, flags, true, fast);
    if (int rc = ensure_ws(h, p.total)) return rc;
    ModelBufs mb = model_bufs(h, p);
    if (r != p.Rp) {
        PaddedParams pp;
        if (int rc = pad_params(h, p, B, N, r, Lam, A, Q, mu0, P0, &pp)) return rc;
    } else {   // the caller's layout is the plan's: the EM updates its arrays in place, and the E-steps write its smoother outputs
        mb.Lam = Lam; mb.A = A; mb.Q = Q; mb.mu0 = mu0; mb.P0 = P0;
        if (f_smooth) mb.fsm = f_smooth;
        if (P_smooth) mb.Psm = P_smooth;
    }
    // balanced panels with the loadings step on the matrix pipe: nothing in the EM reads the per-period smoothed covariances
    // (the M-step works from their sums, cov_kernel's SP11 / SU) -- unless the caller asked for them, the E-steps do not
    // write them (0.15 GB of stores per iteration at config 2, 0.86 GB at config 4)
    if (!P_smooth && (p.ms_mfma || p.ms_wide)) mb.Psm = nullptr;
    if (loglik_single) mb.llbuf = loglik_single;
    // no bookkeeping without a path (dfm_em_step_batch_dev); active_ext: the caller owns the flags and decides when to stop
    mb.active = loglik_path ? (active_ext ? active_ext : mb.active) : nullptr;
    const int k_end = k_count < 0 ? max_iter : (k_first + k_count < max_iter ? k_first + k_count : max_iter);
    if (int rc = em_loop(h, B, k_first, k_end, max_iter, tol, loglik_path, iters, mb, !active_ext, [&](const EmOpts& eo) {
            return em_iteration(h, p, B, T, N, panel, mb, R, eo);
        })) return rc;
    return unpad_results(h, p, B, N, T, r, r, r, mb, Lam, A, Q, mu0, P0, f_smooth, P_smooth);
}

// ---- VAR(p) factor dynamics in companion form ---------------------------------------------
// z_t = (f_t, .., f_{t-p+1}), k = r p <= 32;  M = [A_1 .. A_p; I 0],  Q_z = [Q 0; 0 0]  (dfm_functions.ipynb:477-492);
// padded to Rk x Rk with the usual identity / zero padding.  Loadings padded to Rc = pad_r(r).
__global__ void companion_pad_kernel(int B, int N, int r, int k, int ka, int Rc, int Rk, const double* Lam, const double* Avar,
                                     const double* Q, const double* mu0, const double* P0, double* LamP, double* AP,
                                     double* QP, double* mu0P, double* P0P) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nl = (size_t)B * N * Rc, nm = (size_t)B * Rk * Rk, nv = (size_t)B * Rk;
    if (Lam && tid < nl) {
        const int c = tid % Rc;
        const size_t bn = tid / Rc;
        LamP[tid] = c < r ? Lam[bn * r + c] : 0.0;
    }
    if (tid < nm) {
        const int j = tid % Rk, i = (tid / Rk) % Rk;
        const size_t b = tid / ((size_t)Rk * Rk);
        double a = 0.0, q = 0.0, p0 = 0.0;
        if (i < r && j < ka) a = Avar[(b * r + i) * ka + j];        // [A_1 .. A_p], ka = r p <= k
        else if (i >= r && i < k && j == i - r) a = 1.0;
        if (i < r && j < r) q = Q[(b * r + i) * r + j];
        else if (i >= k && i == j) q = 1.0;
        if (i < k && j < k) p0 = P0[(b * k + i) * k + j];
        else if (i >= k && i == j) p0 = 1.0;
        AP[tid] = a; QP[tid] = q; P0P[tid] = p0;
    }
    if (tid < nv) {
        const int i = tid % Rk;
        const size_t b = tid / Rk;
        mu0P[tid] = i < k ? mu0[b * k + i] : 0.0;
    }
}

// The caller's VAR parameters (Avar [B][r][ka], Q [B][r][r], mu0 [B][k], P0 [B][k][k]) into mb's companion form, and its loadings
// Lam [B][N][r] into mb.Lam at the plan's loadings width -- Lam = null: the family's own loadings kernel fills mb.Lam.
int companion_pad(dfm_handle* h, const Plan& p, int B, int N, int r, int k, int ka, const double* Lam, const double* Avar,
                  const double* Q, const double* mu0, const double* P0, const ModelBufs& mb) {
    const int Rk = p.Rp, Rc = p.Rc ? p.Rc : p.Rp;
    const size_t nl = Lam ? (size_t)B * N * Rc : 0, nm = (size_t)B * Rk * Rk;
    return launch_1d(h, companion_pad_kernel, nl > nm ? nl : nm, B, N, r, k, ka, Rc, Rk, Lam, Avar, Q, mu0, P0, mb.Lam, mb.A, mb.Q,
                     mb.mu0, mb.P0);
}

int varp_run(dfm_handle* h, int B, int T, int N, int r, int nlag, const double* panel, double* Lam, double* R,
             double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
             double* loglik_single, double* f_smooth, double* P_smooth, unsigned flags, bool em) {
    if (!h) return DFM_E_NULL;
    if (nlag < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    const int k = r * nlag;
    if (k > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (int rc = check_general_n(h, N, r)) return rc;
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    HIP_TRY(h, hipSetDevice(h->device));
    // panels with missing cells, loadings up to 4 wide: the collapse on collapse_miss_kernel's table mode (comp_table below); odd N
    // gets one all-missing series appended for it, as in em_run (the Stock-Watson window has 139 series)
    const bool comp_tab_ok = h->opt.odd_pad8 && !h->opt.narrow_tab_off && !h->opt.collapse_miss_old && pad_r(r) < 8 && (flags & DFM_F_MAY_HAVE_MISSING);
    if (comp_tab_ok && (N & 1) && collapse_miss_supported(8, N + 1)) {
        OddPad o;
        if (int rc = odd_pad(h, B, T, N, r, panel, Lam, R, &o)) return rc;
        if (int rc = varp_run(h, B, T, N + 1, r, nlag, o.panel, o.Lam, o.R, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, loglik_single,
                              f_smooth, P_smooth, flags, em)) return rc;
        return em ? odd_unpad(h, B, N, r, o, Lam, R) : 0;
    }
    Companion comp;                                           // loadings on the first block only, pad_r(r) wide
    comp.Rc = pad_r(r); comp.rl = r; comp.kdim = k; comp.qsing = (flags & DFM_F_SINGULAR_Q) ? 1 : 0; comp.table = comp_tab_ok;
    const Plan p = make_plan(h->opt, B, T, N, k, flags | DFM_F_SINGULAR_Q, em, false, comp);
    if (int rc = ensure_ws(h, p.total)) return rc;
    ModelBufs mb = model_bufs(h, p);
    if (int rc = companion_pad(h, p, B, N, r, k, k, Lam, Avar, Q, mu0, P0, mb)) return rc;
    if (!em)   // plain pass: smoothed moments of f_t = z_t[:r] straight into the caller's layout
        return enqueue_pass(h, p, B, T, N, r, panel, mb.pp(), R, f_smooth, P_smooth, loglik_single, nullptr);
    if (loglik_single) mb.llbuf = loglik_single;
    if (!loglik_path) mb.active = nullptr;
    if (int rc = em_loop(h, B, 0, max_iter, max_iter, tol, loglik_path, iters, mb, true, [&](const EmOpts& eo) {
            return em_iteration(h, p, B, T, N, panel, mb, R, eo);
        })) return rc;
    return unpad_results(h, p, B, N, T, r, k, k, mb, Lam, Avar, Q, mu0, P0, f_smooth, P_smooth);
}

// ---- AR idiosyncratic terms by quasi-differencing ----------------------------------------------
// x~_it = x_it - sum_l rho_il x_i,t-l (NaN when x_it or a lag is NaN);  loadings [lam_i, -rho_i1 lam_i, .., -rho_iq lam_i, 0..]
__global__ void quasi_diff_kernel(int B, int T, int N, int q, const double* x, const double* rho, double* out) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)B * (T - q) * N;
    if (tid >= n) return;
    const int i = tid % N;
    const int t = (tid / N) % (T - q);
    const size_t b = tid / ((size_t)N * (T - q));
    const double* xb = x + b * (size_t)T * N;
    double v = xb[(size_t)(t + q) * N + i];
    for (int l = 1; l <= q; ++l) v -= rho[(b * N + i) * q + (l - 1)] * xb[(size_t)(t + q - l) * N + i];
    out[tid] = v;
}
__global__ void ar_loadings_kernel(int B, int N, int r, int q, int Rk, const double* Lam, const double* rho, double* LamK) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (size_t)B * N * Rk) return;
    const int c = tid % Rk;
    const size_t bn = tid / Rk;
    const int l = c / r, cc = c % r;
    double v = 0.0;
    if (l <= q) v = (l == 0 ? 1.0 : -rho[bn * q + (l - 1)]) * Lam[bn * r + cc];
    LamK[tid] = v;
}

int ar_check(dfm_handle* h, int B, int T, int N, int r, int nlag, int q, bool em) {
    if (!h) return DFM_E_NULL;
    if (nlag < 1 || q < 0) return fail(h, DFM_E_DIMS, "need p >= 1 factor lags and q >= 0 idiosyncratic lags%s");
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (!em && T <= q) return fail(h, DFM_E_DIMS, "T must exceed the number of idiosyncratic lags%s");
    if (em && T <= q + 1) return fail(h, DFM_E_DIMS, "T must exceed the number of idiosyncratic lags by at least 2%s");
    const int m = nlag > q + 1 ? nlag : q + 1, k = r * m;
    if (k > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * max(p, q + 1) > DFM_MAX_R (32)%s");
    if (em && !mstep_ar_supported(r, q)) return fail(h, DFM_E_R_UNSUPPORTED, "joint AR estimation needs r <= 8 and q <= 4%s");
    return check_general_n(h, N, k);
}

// The plan of a pass on the T - q quasi-differenced periods (the observation loads on q + 1 blocks of the k-wide state) and, behind
// it, the quasi-differenced panel xq and (EM) the moments of the series CM-steps (mstep_ar.hip)
struct ArPlan { Plan p; ModelBufs mb; int k; double *xq, *mws; };
int ar_plan(dfm_handle* h, int B, int T, int N, int r, int nlag, int q, unsigned flags, bool em, ArPlan* s) {
    const int Tq = T - q;
    s->k = r * (nlag > q + 1 ? nlag : q + 1);
    s->p = make_plan(h->opt, B, Tq, N, s->k, flags | DFM_F_SINGULAR_Q, em, false, lag_blocks(s->k, r, nlag, flags));
    size_t off = s->p.total;
    const size_t xoff = take(off, (size_t)B * Tq * N * sizeof(double));
    const size_t moff = em ? take(off, mstep_ar_workspace(B, T, N, r, q, s->p.Rp)) : (size_t)-1;
    if (int rc = ensure_ws(h, off)) return rc;
    s->mb = model_bufs(h, s->p);
    s->xq = at<double>(h, xoff); s->mws = at<double>(h, moff);
    return 0;
}
// The series side of one pass at the current rho: the quasi-differenced panel (q > 0; *xin = what the pass reads) and the loadings
// on the lag blocks
int ar_prepare(dfm_handle* h, const ArPlan& s, int B, int T, int N, int r, int q, const double* panel, const double* Lam,
               const double* rho, const double** xin) {
    *xin = panel;
    if (q > 0) {
        if (int rc = launch_1d(h, quasi_diff_kernel, (size_t)B * (T - q) * N, B, T, N, q, panel, rho, s.xq)) return rc;
        *xin = s.xq;
    }
    return launch_1d(h, ar_loadings_kernel, (size_t)B * N * s.p.Rp, B, N, r, q, s.p.Rp, Lam, rho, s.mb.Lam);
}

int ar_pass_run(dfm_handle* h, int B, int T, int N, int r, int nlag, int q, const double* panel, const double* Lam,
                const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    if (int rc = ar_check(h, B, T, N, r, nlag, q, false)) return rc;
    if (!panel || !Lam || !sig2 || (q > 0 && !rho) || !Avar || !Q || !mu0 || !P0 || !f_smooth || !loglik)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    ArPlan s;
    if (int rc = ar_plan(h, B, T, N, r, nlag, q, flags, false, &s)) return rc;
    const double* xin;
    if (int rc = ar_prepare(h, s, B, T, N, r, q, panel, Lam, rho, &xin)) return rc;
    if (int rc = companion_pad(h, s.p, B, N, r, s.k, r * nlag, nullptr, Avar, Q, mu0, P0, s.mb)) return rc;
    return enqueue_pass(h, s.p, B, T - q, N, r, xin, s.mb.pp(), sig2, f_smooth, P_smooth, loglik, nullptr);
}

// Joint estimation with AR(q) idiosyncratic terms by ECM (oracle/ar_oracle.py em_ar).  Per iteration: quasi-difference the
// panel at the current rho, loadings [lam, -rho_1 lam, ..] on the companion state, smoother pass + transition CM-step (the
// recursion kernel's epilogue: VAR(p) inside the m-lag state, RecursionArgs::ka), then the series CM-steps (mstep_ar.hip).
int ar_em_run(dfm_handle* h, int B, int T, int N, int r, int nlag, int q, const double* panel, double* Lam, double* sig2,
              double* rho, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
              int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    if (int rc = ar_check(h, B, T, N, r, nlag, q, true)) return rc;
    if (!panel || !Lam || !sig2 || (q > 0 && !rho) || !Avar || !Q || !mu0 || !P0 || !loglik_path || !iters)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    HIP_TRY(h, hipSetDevice(h->device));
    ArPlan s;
    if (int rc = ar_plan(h, B, T, N, r, nlag, q, flags, true, &s)) return rc;
    const Plan& p = s.p;
    const ModelBufs& mb = s.mb;
    if (int rc = companion_pad(h, p, B, N, r, s.k, r * nlag, nullptr, Avar, Q, mu0, P0, mb)) return rc;
    ArMstepArgs ma;
    ma.B = B; ma.T = T; ma.N = N; ma.r = r; ma.q = q; ma.Rk = p.Rp;
    ma.panel = panel; ma.zsm = mb.fsm; ma.Psm = mb.Psm; ma.active = mb.active; ma.Lam = Lam; ma.rho = rho; ma.sig2 = sig2;
    if (int rc = em_loop(h, B, 0, max_iter, max_iter, tol, loglik_path, iters, mb, true, [&](const EmOpts& eo) -> int {
        const double* xin;
        if (int rc = ar_prepare(h, s, B, T, N, r, q, panel, Lam, rho, &xin)) return rc;
        if (int rc = enqueue_pass(h, p, B, T - q, N, p.Rp, xin, mb.pp(), sig2, mb.fsm, mb.Psm, mb.llbuf, &eo)) return rc;
        HIP_LAUNCH(h, K_MSTEP_STATS, launch_mstep_ar(ma, s.mws, h->stream));
        return 0;
    })) return rc;
    return unpad_results(h, p, B, N, T - q, r, r * nlag, s.k, mb, nullptr, Avar, Q, mu0, P0, f_smooth, P_smooth);
}

// ---- mixed frequency (mstep_mf.hip; tests/mf_expect.py) ---------------------------------------------------------------------
// x_it = lam_i' sum_{l<L} w_il f_{t-l} + e_it with known weights W [N][L] shared by the batch: a sibling of the AR model above without
// quasi-differencing and without a rho step.  Loadings [w_i0 lam_i, .., w_i,L-1 lam_i, 0..] on the companion state of
// m = max(p, L) lags, the pass and the restricted transition step as ar_em_run, then the series step from a per-class table.
using MfClasses = MfDeal;
// the distinct rows of W (exact comparison) and the series dealt into class-pure tiles of 16 (index lists, -1 = padding):
// dfm_mfgeom.h mf_deal
int mf_classes(dfm_handle* h, int N, int L, const std::vector<double>& W, MfClasses* mc) {
    switch (mf_deal(N, L, W.data(), mc)) {
        case kMfDealOk: return 0;
        case kMfDealNotFinite: return fail(h, DFM_E_DIMS, "mixed frequency: a weight is not finite%s");
        default: return fail(h, DFM_E_DIMS, "mixed frequency: more than 8 distinct weight vectors%s");
    }
}

int mf_check(dfm_handle* h, int B, int T, int N, int r, int nlag, int L) {
    if (!h) return DFM_E_NULL;
    if (nlag < 1 || L < 1) return fail(h, DFM_E_DIMS, "need p >= 1 factor lags and L >= 1 aggregation lags%s");
    if (L > kMfMaxLags) return fail(h, DFM_E_DIMS, "mixed frequency: L <= 5 aggregation lags%s");
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    const int m = nlag > L ? nlag : L, k = r * m;
    if (k > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * max(p, L) > DFM_MAX_R (32)%s");
    return check_general_n(h, N, k);
}

// The weights on the host (finite; EM: dealt into classes), the plan of a pass on the k-wide state (the observation loads on L
// blocks) and, for the EM, behind it: the series step's table and moments, then the class weights and the tile lists
struct MfPlan { Plan p; ModelBufs mb; int k; MfClasses mc; double *mws, *Wc; int *tile_class, *tile_series; };
int mf_plan(dfm_handle* h, int B, int T, int N, int r, int nlag, int L, const double* W, unsigned flags, bool em, MfPlan* s) {
    std::vector<double> Wh((size_t)N * L);
    HIP_TRY(h, hipMemcpyAsync(Wh.data(), W, Wh.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (em) {
        if (int rc = mf_classes(h, N, L, Wh, &s->mc)) return rc;
    } else {
        for (double w : Wh)
            if (!isfinite(w)) return fail(h, DFM_E_DIMS, "mixed frequency: a weight is not finite%s");
    }
    const MfClasses& mc = s->mc;
    s->k = r * (nlag > L ? nlag : L);
    s->p = make_plan(h->opt, B, T, N, s->k, flags | DFM_F_SINGULAR_Q, em, false, lag_blocks(s->k, r, nlag, flags));
    size_t off = s->p.total;
    const size_t none = (size_t)-1;
    const size_t moff = em ? take(off, mstep_mf_workspace(B, T, N, r, mc.C)) : none;
    const size_t woff = em ? take(off, mc.Wc.size() * sizeof(double)) : none;
    const size_t coff = em ? take(off, mc.tile_class.size() * sizeof(int)) : none;
    const size_t soff = em ? take(off, mc.tile_series.size() * sizeof(int)) : none;
    if (int rc = ensure_ws(h, off)) return rc;
    s->mb = model_bufs(h, s->p);
    s->mws = at<double>(h, moff); s->Wc = at<double>(h, woff); s->tile_class = at<int>(h, coff); s->tile_series = at<int>(h, soff);
    if (em) {
        HIP_TRY(h, hipMemcpyAsync(s->Wc, mc.Wc.data(), mc.Wc.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(s->tile_class, mc.tile_class.data(), mc.tile_class.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(s->tile_series, mc.tile_series.data(), mc.tile_series.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));         // (the host vectors need not outlive this call)
    }
    return 0;
}

int mf_pass_run(dfm_handle* h, int B, int T, int N, int r, int nlag, int L, const double* panel, const double* Lam, const double* R,
                const double* W, const double* Avar, const double* Q, const double* mu0, const double* P0, double* f_smooth,
                double* P_smooth, double* loglik, unsigned flags) {
    if (int rc = mf_check(h, B, T, N, r, nlag, L)) return rc;
    if (!panel || !Lam || !R || !W || !Avar || !Q || !mu0 || !P0 || !f_smooth || !loglik)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    MfPlan s;
    if (int rc = mf_plan(h, B, T, N, r, nlag, L, W, flags, false, &s)) return rc;
    HIP_TRY(h, launch_mf_loadings(B, N, r, L, s.p.Rp, Lam, W, s.mb.Lam, h->stream));
    if (int rc = companion_pad(h, s.p, B, N, r, s.k, r * nlag, nullptr, Avar, Q, mu0, P0, s.mb)) return rc;
    return enqueue_pass(h, s.p, B, T, N, r, panel, s.mb.pp(), R, f_smooth, P_smooth, loglik, nullptr);
}

// free_mask [N][r] (device bytes, or null = every loading estimated): the series solve with fixed loadings, mstep_mf_blocks.hip;
// nothing else of the iteration looks at it
int mf_run(dfm_handle* h, int B, int T, int N, int r, int nlag, int L, const double* panel, double* Lam, double* R, const double* W,
           double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
           double* f_smooth, double* P_smooth, unsigned flags, const unsigned char* free_mask = nullptr) {
    if (int rc = mf_check(h, B, T, N, r, nlag, L)) return rc;
    if (!mstep_mf_supported(r, L)) return fail(h, DFM_E_R_UNSUPPORTED, "mixed-frequency estimation needs r <= 8%s");
    if (!panel || !Lam || !R || !W || !Avar || !Q || !mu0 || !P0 || !loglik_path || !iters)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    HIP_TRY(h, hipSetDevice(h->device));
    MfPlan s;
    if (int rc = mf_plan(h, B, T, N, r, nlag, L, W, flags, true, &s)) return rc;
    const Plan& p = s.p;
    const ModelBufs& mb = s.mb;
    const int Rk = p.Rp;
    if (int rc = companion_pad(h, p, B, N, r, s.k, r * nlag, nullptr, Avar, Q, mu0, P0, mb)) return rc;
    MfMstepArgs ma;
    ma.B = B; ma.T = T; ma.N = N; ma.r = r; ma.L = L; ma.Rk = Rk; ma.C = s.mc.C; ma.VW = mstep_mf_row_width(r); ma.ntiles = s.mc.ntiles;
    ma.panel = panel; ma.zsm = mb.fsm; ma.Psm = mb.Psm; ma.active = mb.active; ma.Wc = s.Wc;
    ma.tile_class = s.tile_class; ma.tile_series = s.tile_series; ma.Lam = Lam; ma.R = R;
    if (int rc = em_loop(h, B, 0, max_iter, max_iter, tol, loglik_path, iters, mb, true, [&](const EmOpts& eo) -> int {
        HIP_LAUNCH(h, K_PAD, launch_mf_loadings(B, N, r, L, Rk, Lam, W, mb.Lam, h->stream));
        if (int rc = enqueue_pass(h, p, B, T, N, Rk, panel, mb.pp(), R, mb.fsm, mb.Psm, mb.llbuf, &eo)) return rc;
        HIP_LAUNCH(h, K_MF_TABLE, launch_mf_table(ma, s.mws, h->stream));
        HIP_LAUNCH(h, K_MF_MOMENTS, launch_mf_moments(ma, s.mws, h->stream));
        if (free_mask) HIP_LAUNCH(h, K_MF_SOLVE_BLOCKS, launch_mf_solve_blocks(ma, free_mask, s.mws, h->stream));
        else HIP_LAUNCH(h, K_MF_SOLVE, launch_mf_solve(ma, s.mws, h->stream));
        return 0;
    })) return rc;
    return unpad_results(h, p, B, N, T, r, r * nlag, s.k, mb, nullptr, Avar, Q, mu0, P0, f_smooth, P_smooth);
}

// ---- observed factors (mstep_obs.hip, oracle/obs_oracle.py em_obs) ------------------------------------
// Per iteration: y = x - Lam_o g and the padded Lam_u -> the ordinary smoother pass on y with the transition M-step (the
// pass's own EM epilogue: A, Q, mu0, P0 of the unobserved block) -> the joint loadings regression on z = (g, f).
int obs_em_run(dfm_handle* h, int B, int T, int N, int ru, int ro, const double* panel, const double* G, double* Lam, double* R,
               double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
               double* f_smooth, double* P_smooth, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (int rc = check_dims(h, B, T, N, ru)) return rc;
    const bool wide_obs = mstep_obs_wide_supported(ro, ru);   // r_o + r_u = 9 .. 32: the ordinary loadings step on augmented moments
    if (!mstep_obs_supported(ro, ru) && !wide_obs)
        return fail(h, DFM_E_R_UNSUPPORTED, "observed factors: need r_o >= 1, r_u >= 1 and r_o + r_u <= 32%s");
    const bool fast = em_fast_eligible(h, N, ru, flags);
    if (int rc = check_em_n(h, N, ru, fast)) return rc;
    if (wide_obs && N > 1024)   // (the joint regression at r_o + r_u > 8 runs on mstep_lam_kernel: lane = series, N <= 1024)
        return fail(h, DFM_E_DIMS, "observed factors with r_o + r_u > 8: N <= 1024%s");
    if (!panel || !G || !Lam || !R || !A || !Q || !mu0 || !P0 || !loglik_path || !iters)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const Plan p = make_plan(h->opt, B, T, N, ru, flags, true, fast);
    // behind the plan: the residual panel y, then for the wide joint regression
    // z [B][T][Re] | Var z [B][T][NPe] | LamAug [B][N][Re] | S11, S11inv [B][Re][Re] | Dmiss [B][N][NPe]
    const int Re = wide_obs ? mstep_obs_wide_width(ro, ru) : 0;
    const size_t NPe = (size_t)Re * (Re + 1) / 2;
    size_t off = p.total;
    const size_t yoff = take(off, (size_t)B * T * N * sizeof(double));
    const size_t o_z = wide_obs ? take(off, (size_t)B * T * Re * sizeof(double)) : 0;
    const size_t o_v = wide_obs ? take(off, (size_t)B * T * NPe * sizeof(double)) : 0;
    const size_t o_l = wide_obs ? take(off, (size_t)B * N * Re * sizeof(double)) : 0;
    const size_t o_s = wide_obs ? take(off, (size_t)B * Re * Re * sizeof(double)) : 0;
    const size_t o_i = wide_obs ? take(off, (size_t)B * Re * Re * sizeof(double)) : 0;
    const size_t o_d = wide_obs ? take(off, (size_t)B * N * NPe * sizeof(double)) : 0;
    if (int rc = ensure_ws(h, off)) return rc;
    const int Rp = p.Rp, Rl = p.Rc ? p.Rc : p.Rp;            // state width, loadings width
    double* y = at<double>(h, yoff);
    ModelBufs mb = model_bufs(h, p);                          // (mb.Lam: the padded Lam_u, embedded by launch_obs_residual)
    if (ru != Rp) {                                           // (N = 0: no loadings)
        if (int rc = launch_1d(h, pad_params_kernel, (size_t)B * Rp * Rp, B, 0, ru, Rp, Rl, nullptr, A, Q, mu0, P0, nullptr, mb.A, mb.Q,
                               mb.mu0, mb.P0)) return rc;
    } else {
        mb.A = A; mb.Q = Q; mb.mu0 = mu0; mb.P0 = P0;
    }
    ObsArgs oa;
    oa.B = B; oa.T = T; oa.N = N; oa.ro = ro; oa.ru = ru; oa.Rl = Rl;
    oa.panel = panel; oa.G = G; oa.fsm = mb.fsm; oa.Psm = mb.Psm; oa.active = mb.active; oa.Lam = Lam; oa.R = R;
    if (int rc = em_loop(h, B, 0, max_iter, max_iter, tol, loglik_path, iters, mb, true, [&](const EmOpts& eo) -> int {
        HIP_LAUNCH(h, K_PAD, launch_obs_residual(oa, y, mb.Lam, h->stream));
        if (int rc = enqueue_pass(h, p, B, T, N, Rl, y, mb.pp(), R, mb.fsm, mb.Psm, mb.llbuf, &eo)) return rc;
        if (!wide_obs) {
            HIP_LAUNCH(h, K_MSTEP_STATS, launch_mstep_obs(oa, h->stream));
        } else {
            double *z = at<double>(h, o_z), *Vz = at<double>(h, o_v), *LamAug = at<double>(h, o_l);
            HIP_LAUNCH(h, K_PAD, launch_obs_augment(oa, Re, z, Vz, LamAug, at<double>(h, o_s), at<double>(h, o_i), h->stream));
            MstepArgs ma;
            ma.B = B; ma.T = T; ma.N = N; ma.r = Re;
            ma.panel = panel; ma.fsm = z; ma.Psm = Vz; ma.S11 = at<double>(h, o_s); ma.S11inv = at<double>(h, o_i);
            ma.Dmiss = at<double>(h, o_d);
            ma.active = mb.active; ma.Lam_out = LamAug; ma.R_out = R; ma.lam_stride = Re;
            ma.min_cells = ro + ru + 1;                       // (as mstep_obs_kernel and the oracle: too few cells for the joint regression)
            HIP_TRY(h, hipMemsetAsync(ma.Dmiss, 0, (size_t)B * N * NPe * sizeof(double), h->stream));
            HIP_LAUNCH(h, K_MSTEP_STATS, launch_mstep_lam(Re, ma, h->stream));
            if (int rc = copy_block(h, (size_t)B * N, 1, Re, 1, ro + ru, LamAug, Lam)) return rc;   // (inactive replicates: their own values back)
        }
        return 0;
    })) return rc;
    return unpad_results(h, p, B, N, T, ru, ru, ru, mb, nullptr, A, Q, mu0, P0, f_smooth, P_smooth);
}

// ---- what the post-estimation drivers share, plain and AR-idiosyncratic (q = 0: the plain model) -----------------------------
// Lags of the state: the factors' p, and at least q + 1 where the series' AR terms read q lags of the factors.
int state_lags(int p, int q) { return p > q + 1 ? p : q + 1; }

// The model parameters of a host-pointer entry on the device.  stage_model declares them to the entry's HostStage in the order
// every _dev twin takes them -- Lam, R | sig2, [rho], Avar, Q, mu0, P0, [v0], mean, sd; rho and v0 with q > 0 only -- with the
// element counts of (B, N, r, p, q).  `md` receives the pointers at st.begin(): it lives where the entry's other pointers do.
struct ModelDev { double *Lam, *R, *rho, *A, *Q, *mu0, *P0, *v0, *mean, *sd; };
void stage_model(HostStage& st, ModelDev& md, int B, int N, int r, int p, int q, const double* Lam, const double* R, const double* rho,
                 const double* Avar, const double* Q, const double* mu0, const double* P0, const double* v0, const double* mean,
                 const double* sd) {
    const size_t n_R = (size_t)B * N, k = (size_t)r * state_lags(p, q);
    md = ModelDev{};
    st.in(Lam, n_R * r, md.Lam); st.in(R, n_R, md.R);
    if (q) st.in(rho, n_R * q, md.rho);
    st.in(Avar, (size_t)B * r * r * p, md.A); st.in(Q, (size_t)B * r * r, md.Q); st.in(mu0, (size_t)B * k, md.mu0);
    st.in(P0, (size_t)B * k * k, md.P0);
    if (q) st.in(v0, v0 ? n_R : 0, md.v0);
    st.in(mean, mean ? n_R : 0, md.mean); st.in(sd, sd ? n_R : 0, md.sd);
}

// The expanded parameters of one slice of at most Smax pass replicates (simsmooth_expand_kernel; rho by
// simsmooth_ar_expand_kernel) on a state of k: the constructor takes their room at `off` of a driver's block, in the order eLam,
// eR, [erho], eA, eQ, emu0, eP0; once the block has grown, point() writes them into the SsArgs and returns erho (q = 0: null).
struct SliceParams {
    size_t L, R, rho, A, Q, m, P;
    SliceParams(size_t& off, int Smax, int N, int r, size_t k, int q) {
        const size_t S = (size_t)Smax, d = sizeof(double);
        L = take(off, S * N * r * d); R = take(off, S * N * d);
        rho = q ? take(off, S * N * q * d) : (size_t)-1;
        A = take(off, S * r * k * d); Q = take(off, S * r * r * d); m = take(off, S * k * d); P = take(off, S * k * k * d);
    }
    double* point(const DevBlock& b, SsArgs& e) const {
        e.eLam = at<double>(b, L); e.eR = at<double>(b, R); e.eA = at<double>(b, A); e.eQ = at<double>(b, Q);
        e.emu0 = at<double>(b, m); e.eP0 = at<double>(b, P);
        return at<double>(b, rho);
    }
};

// The AR drivers run the plain model's kernels on m = state_lags(p, q) lags: *Am = Avar with zero blocks appended to m lags
// (simsmooth_ar_params_kernel into Apad, which the driver planned for p < m), or the caller's Avar where p = m.
int pad_avar(dfm_handle* h, int B, int r, int p, int m, const double* Avar, double* Apad, const double** Am) {
    *Am = Avar;
    if (p < m) {
        HIP_LAUNCH(h, K_SSAR_PARAMS, launch_simsmooth_ar_params(B, r, p, m, Avar, Apad, h->stream));
        *Am = Apad;
    }
    return 0;
}

// The target loop of both news checks: rows in [t_lo, 2^30), series in [0, N); *H = the horizon the targets need.
bool news_targets(int T, int N, int G, const int* target_t, const int* target_i, int t_lo, int* H) {
    int tmax = 0;
    for (int g = 0; g < G; ++g) {
        if (target_t[g] < t_lo || target_t[g] > 0x3fffffff || target_i[g] < 0 || target_i[g] >= N) return false;
        if (target_t[g] > tmax) tmax = target_t[g];
    }
    *H = tmax + 1 > T ? tmax + 1 - T : 0;
    return true;
}

// The targets as (row - shift, series) pairs at tgt [G][2] of the device (shift = q: output rows of the AR forecasts).
int news_stage_targets(dfm_handle* h, int G, const int* target_t, const int* target_i, int shift, int* tgt) {
    std::vector<int> tg((size_t)2 * G);                       // (a pageable source: staged before the call returns)
    for (int g = 0; g < G; ++g) { tg[2 * g] = target_t[g] - shift; tg[2 * g + 1] = target_i[g]; }
    HIP_TRY(h, hipMemcpyAsync(tgt, tg.data(), tg.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The three conditional means of both news drivers -- old, new, then the revised old panel `rev`, whose xhat stays behind for the
// impacts: forecast(panel, loglik, flags) runs one into xhat, news_gather_kernel (ga) picks the targets out of it.  The logliks go
// to ll_all [3][B] (old, revised, new), else all to ll_own.
template <class Forecast>
int news_forecasts(dfm_handle* h, int B, const NwArgs& ga, const double* oldp, const double* newp, const double* rev,
                   const double* xhat, double* ll_all, double* ll_own, unsigned flags, Forecast forecast) {
    const struct { const double* panel; unsigned fl; int which; } runs[3] = {
        {oldp, flags | DFM_F_MAY_HAVE_MISSING, 0}, {newp, flags, 2}, {rev, flags | DFM_F_MAY_HAVE_MISSING, 1}};
    for (const auto& run : runs) {
        if (int rc = forecast(run.panel, ll_all ? ll_all + (size_t)run.which * B : ll_own, run.fl)) return rc;
        HIP_LAUNCH(h, K_NW_GATHER, launch_news_gather(ga, xhat, run.which, h->stream));
    }
    return 0;
}

// The tail of a Gibbs sweep, for both samplers: sweep j is kept when it is past the burn-in and on the thinning grid, as slot
// (j - burn) / thin of K; gibbs_keep copies one parameter of it, dst [B][K][per] <- src [B][per], behind the sweep (dst null: not wanted).
bool gibbs_kept_slot(int j, int burn, int thin) { return j >= burn && (j - burn) % thin == 0; }
hipError_t gibbs_keep(dfm_handle* h, double* dst, const double* src, size_t per, size_t kk, size_t K, int B) {
    const size_t d = sizeof(double);
    return dst ? hipMemcpy2DAsync(dst + kk * per, K * per * d, src, per * d, per * d, (size_t)B, hipMemcpyDeviceToDevice, h->stream)
               : hipSuccess;
}

}  // namespace

extern "C" {

const char* dfm_version(void) { return "dfmhip 0.1 (gfx950, fp64)"; }

int dfm_create(dfm_handle** out, int device_id, void* stream) {
    if (!out) return DFM_E_NULL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return DFM_E_NO_DEVICE;
    if (device_id < 0 || device_id >= ndev) return DFM_E_DIMS;
    dfm_handle* h = new (std::nothrow) dfm_handle();
    if (!h) return DFM_E_NULL;
    h->device = device_id;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) {
        if (stream) {
            h->stream = static_cast<hipStream_t>(stream);
        } else {
            e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
            h->own_stream = true;
        }
    }
    if (e == hipSuccess) {   // the side stream carries the short latency-bound kernels (gram, cov) the scan waits for:
        int lo = 0, hi = 0;      // highest priority, so that their workgroups are placed ahead of the streaming collapse
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->post, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_post, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->status_dev), 256);
    if (e == hipSuccess) e = hipMemset(h->status_dev, 0, 256);
    if (e != hipSuccess) {
        delete h;
        return (int)e;
    }
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cu = prop.multiProcessorCount; }
    if (const char* v = route_env("DFM_NUM_CU")) { if (atoi(v) > 0) h->num_cu = atoi(v); }   // diagnostics: persistent grids sized for fewer CUs
    *out = h;
    return 0;
}

int dfm_destroy(dfm_handle* h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->side) { hipStreamSynchronize(h->side); hipStreamDestroy(h->side); }
    if (h->post) { hipStreamSynchronize(h->post); hipStreamDestroy(h->post); }
    if (h->ev_post) hipEventDestroy(h->ev_post);
    for (auto e : h->ev_sub) hipEventDestroy(e);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    for (DevBlock* b : {&h->ws, &h->odd, &h->fc, &h->ss, &h->nw, &h->sv, &h->ft, &h->gb, &h->rw}) b->release();
    if (h->status_dev) hipFree(h->status_dev);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int dfm_set_stream(dfm_handle* h, void* stream) {
    if (!h) return DFM_E_NULL;
    hipStream_t ns = static_cast<hipStream_t>(stream);
    if (ns == h->stream) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->own_stream && h->stream) {
        hipStreamSynchronize(h->stream);
        hipStreamDestroy(h->stream);
        h->own_stream = false;
    } else {
        // The handle has ONE workspace (bcol, wtab, tab, status, ...): work enqueued on the new stream must not start
        // before the work already enqueued on the old one has finished with it.
        HIP_TRY(h, hipEventRecord(h->ev_fork, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(ns, h->ev_fork, 0));
    }
    h->stream = ns;
    return 0;
}

// (forward: defined with the entry points that use it)
static int status_check(dfm_handle* h);
// A host-pointer entry point opens a new status epoch: whatever earlier, unchecked *_dev calls left in the sticky word is
// read and cleared here, so that the check at the END of the call reports this call's own kernels only (a stale NaN / PCA /
// time-out bit used to fail the next unrelated host call, and silently triggered api.estimate's singular-Q retry).  The
// discarded bits are kept in the handle (discarded_status) but NOT written to dfm_last_error -- a caller that reads the string after
// a successful call must not find an error text there; device-pointer callers that care call dfm_check_status after their own calls.  These entries copy whole panels across PCIe -- one 4-byte read more is free.
static int status_epoch(dfm_handle* h) {
    if (!h->status_dev) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int st = 0;
    HIP_TRY(h, hipMemcpy(&st, h->status_dev, sizeof(int), hipMemcpyDeviceToHost));
    if (st) {
        HIP_TRY(h, hipMemset(h->status_dev, 0, sizeof(int)));
        h->discarded_status |= st;                               // (not into h->err: this call has not failed)
    }
    return 0;
}

int dfm_synchronize(dfm_handle* h) {
    if (!h) return DFM_E_NULL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return status_check(h);
}

int dfm_check_status(dfm_handle* h) { return dfm_synchronize(h); }

int dfm_chunk_fallbacks(dfm_handle* h, int* n_failed, int* n_total) {
    if (!h) return DFM_E_NULL;
    if (!n_failed || !n_total) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    *n_failed = 0; *n_total = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!h->ck_fail_dev || h->ck_fail_n <= 0) return 0;
    std::vector<int> host((size_t)h->ck_fail_n);
    HIP_TRY(h, hipMemcpy(host.data(), h->ck_fail_dev, host.size() * sizeof(int), hipMemcpyDeviceToHost));
    int nf = 0;
    for (int v : host) nf += v != 0;
    *n_failed = nf; *n_total = h->ck_fail_n;
    return 0;
}

int dfm_profile_enable(dfm_handle* h, int on) {
    if (!h) return DFM_E_NULL;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (auto& ev : h->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    h->events.clear();
    h->profiling = on != 0;
    return 0;
}

int dfm_profile_read(dfm_handle* h, int kernel_index, char* name_out, int name_cap, double* total_ms,
                     int* launches) {
    if (!h) return DFM_E_NULL;
    if (kernel_index < 0) return DFM_E_DIMS;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->prof_names.clear();                                  // distinct kernel names, in order of first launch
    for (auto& ev : h->events) {
        bool seen = false;
        for (const char* n : h->prof_names) seen = seen || strcmp(n, ev.name) == 0;
        if (!seen) h->prof_names.push_back(ev.name);
    }
    if (kernel_index >= (int)h->prof_names.size()) return DFM_E_DIMS;
    const char* want = h->prof_names[kernel_index];
    double tot = 0.0; int n = 0;
    for (auto& ev : h->events)
        if (strcmp(ev.name, want) == 0) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) { tot += ms; ++n; }
        }
    if (name_out && name_cap > 0) { strncpy(name_out, want, name_cap - 1); name_out[name_cap - 1] = 0; }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return 0;
}

const char* dfm_last_error(const dfm_handle* h) { return h ? h->err : "null handle"; }

size_t dfm_workspace_bytes(int B, int T, int N, int r, unsigned flags) {
    if (B < 1 || T < 1 || N < 1 || r < 1 || r > DFM_MAX_R) return 0;
    // the larger of the two plans an entry point may take for this shape: sequential (general) path, or -- balanced
    // panels only -- the time-parallel fast path, whose `tab` ([B][T][3][Rp][Rp]) and M-step partial sums are larger.
    // No handle: the switches as the environment stands now, i.e. what a handle created at this moment would plan.
    const RouteOpts o = route_opts_from_env();
    size_t best = make_plan(o, B, T, N, r, flags, true, false).total;
    if (fast_eligible(o, N, r, flags)) {
        const size_t f = make_plan(o, B, T, N, r, flags, true, true).total;
        if (f > best) best = f;
    }
    return best;
}

int dfm_ks_pass_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, const double* Lam,
                          const double* R, const double* A, const double* Q, const double* mu0,
                          const double* P0, double* f_smooth, double* P_smooth, double* loglik,
                          unsigned flags) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0 || !f_smooth || !loglik)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    const bool fast = fast_eligible(h->opt, N, r, flags);
    if (!fast)
        if (int rc = check_general_n(h, N, r, true)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (needs_odd_pad(h->opt, fast, N, r, flags, B)) {  // odd N beyond the tilings: one all-missing series appended
        OddPad o;
        if (int rc = odd_pad(h, B, T, N, r, panel, Lam, R, &o)) return rc;
        // (the appended series is missing in EVERY period: the padded problem has missing cells whatever the caller said about N)
        return dfm_ks_pass_batch_dev(h, B, T, N + 1, r, o.panel, o.Lam, o.R, A, Q, mu0, P0, f_smooth, P_smooth, loglik,
                                     flags | DFM_F_MAY_HAVE_MISSING);
    }
    if (pipe_eligible(h, B, N, r, flags)) {
        const Plan ps = make_plan(h->opt, pipe_sub(h), T, N, r, flags, false, false);
        const size_t rr = (size_t)r * r, np = (size_t)r * (r + 1) / 2;
        return pipe_run(h, B, ps.total, [&](int b0, int bn) -> int {
            PaddedParams pp;
            if (int rc = pad_params(h, ps, bn, N, r, Lam + (size_t)b0 * N * r, A + b0 * rr, Q + b0 * rr, mu0 + (size_t)b0 * r, P0 + b0 * rr, &pp)) return rc;
            return enqueue_pass(h, ps, bn, T, N, r, panel + (size_t)b0 * T * N, pp, R + (size_t)b0 * N, f_smooth + (size_t)b0 * T * r,
                                P_smooth ? P_smooth + (size_t)b0 * T * np : nullptr, loglik + b0, nullptr);
        });
    }
    const Plan p = make_plan(h->opt, B, T, N, r, flags, false, fast);
    if (int rc = ensure_ws(h, p.total)) return rc;
    PaddedParams pp;
    if (int rc = pad_params(h, p, B, N, r, Lam, A, Q, mu0, P0, &pp)) return rc;
    return enqueue_pass(h, p, B, T, N, r, panel, pp, R, f_smooth, P_smooth, loglik, nullptr);
}

// The status word of the last call's plan, read after the stream has been synchronised.  Bits: 1 = NaN in a panel that was
// declared balanced, 2 = the PCA start's subspace iteration did not converge, 4 = a bounded wait between the waves of the
// one-launch pass ran out (its outputs are invalid even where the log-likelihood happens to be finite), 8 = dfm_news_batch: a cell
// of the old vintage is observed where the new one is missing, 16 = dfm_irf_batch / dfm_histdecomp_batch: a zero pivot in
// Lam[named, :] or (decomposition, dfm_proxyirf_batch) in the root of Q, 32 = dfm_filter_batch: a replicate's update failed, 128 (kRwWindowBit) =
// dfm_rolling_eval_batch: a thin or constant series in a window.  Every synchronising
// entry point goes through here; device-pointer callers get the same check from dfm_synchronize / dfm_check_status.
static int status_check(dfm_handle* h) {
    if (!h->status_dev) return 0;
    int st = 0;
    HIP_TRY(h, hipMemcpy(&st, h->status_dev, sizeof(int), hipMemcpyDeviceToHost));
    if (st) HIP_TRY(h, hipMemset(h->status_dev, 0, sizeof(int)));      // reported once
    if (st & 4) return fail(h, DFM_E_NUMERIC, "one-launch pass: a bounded wait between its waves ran out (results invalid)%s");
    if (st & kRwWindowBit) return fail(h, DFM_E_WINDOW, "rolling evaluation: a series of a window has fewer than min_obs visible cells, or they are all equal%s");
    if (st & 8) return fail(h, DFM_E_VINTAGE, "news: a cell observed in the old vintage is missing in the new one%s");
    if (st & 1) return fail(h, DFM_E_MISSING, "panel contains NaN but DFM_F_MAY_HAVE_MISSING was not set%s");
    if (st & 16) return fail(h, DFM_E_NUMERIC, "structural identification: Lam[named, :] is singular, or Q is not positive definite where S^-1 is needed%s");
    if (st & 32) return fail(h, DFM_E_NUMERIC, "filter: a replicate's update met a non-finite value or a matrix that is not positive semi-definite (NaN from that period on)%s");
    if (st & 64) return fail(h, DFM_E_NUMERIC, "Gibbs sampler: a Cholesky factorisation failed, or a Gamma draw or a stationary rho draw was rejected 32 times%s");
    if (st & 2) return fail(h, DFM_E_NUMERIC, "PCA subspace iteration did not converge (near-degenerate spectrum at the cut)%s");
    return 0;
}
// status word + log-likelihood sanity after a synchronising call (loglik_host: stride doubles apart)
static int post_check(dfm_handle* h, const double* loglik_host, int B, size_t stride = 1) {
    if (int rc = status_check(h)) return rc;
    for (int b = 0; b < B; ++b)
        if (!isfinite(loglik_host[(size_t)b * stride])) return fail(h, DFM_E_NUMERIC, "non-finite log-likelihood (Q or P0 not positive definite?)%s");
    return 0;
}

int dfm_ks_pass_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel, const double* Lam,
                      const double* R, const double* A, const double* Q, const double* mu0, const double* P0,
                      double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0 || !f_smooth || !loglik)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t np = (size_t)r * (r + 1) / 2, n_m = (size_t)B * r * r;
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(Lam, (size_t)B * N * r, lam_d); st.in(R, (size_t)B * N, R_d);
    st.in(A, n_m, A_d); st.in(Q, n_m, Q_d); st.in(mu0, (size_t)B * r, mu_d); st.in(P0, n_m, P0_d);
    st.out(f_smooth, (size_t)B * T * r, f_d); st.out(P_smooth, P_smooth ? (size_t)B * T * np : 0, P_d); st.out(loglik, (size_t)B, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_ks_pass_batch_dev(h, B, T, N, r, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, loglik, B);
    return rc;
}


// ---- EM --------------------------------------------------------------------------------------------
int dfm_em_step_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                          double* A, double* Q, double* mu0, double* P0, double* loglik, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (!loglik) return fail(h, DFM_E_NULL, "loglik is NULL%s");
    return em_run(h, B, T, N, r, panel, Lam, R, A, Q, mu0, P0, 1, 0.0, nullptr, nullptr, loglik, nullptr, nullptr, flags);
}

int dfm_em_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                     double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                     int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (!loglik_path || !iters) return fail(h, DFM_E_NULL, "loglik_path / iters is NULL%s");
    return em_run(h, B, T, N, r, panel, Lam, R, A, Q, mu0, P0, max_iter, tol, loglik_path, iters, nullptr, f_smooth,
                  P_smooth, flags);
}

int dfm_em_iterate_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                             double* A, double* Q, double* mu0, double* P0, int k, int max_iter, double tol,
                             double* loglik_path, int* iters, int* active, double* f_smooth, double* P_smooth,
                             unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (!loglik_path || !iters || !active) return fail(h, DFM_E_NULL, "loglik_path / iters / active is NULL%s");
    if (max_iter < 1 || k < 0 || k >= max_iter) return fail(h, DFM_E_DIMS, "need 0 <= k < max_iter%s");
    return em_run(h, B, T, N, r, panel, Lam, R, A, Q, mu0, P0, max_iter, tol, loglik_path, iters, nullptr, f_smooth, P_smooth,
                  flags, k, 1, active);
}

int dfm_em_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R, double* A,
                 double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
                 double* f_smooth, double* P_smooth, unsigned flags) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (int rc = check_em_n(h, N, r, em_fast_eligible(h, N, r, flags))) return rc;
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0 || !loglik_path || !iters)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t np = (size_t)r * (r + 1) / 2, n_m = (size_t)B * r * r;
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    int* it_d;
    st.in(panel, (size_t)B * T * N, x_d); st.inout(Lam, (size_t)B * N * r, lam_d); st.inout(R, (size_t)B * N, R_d);
    st.inout(A, n_m, A_d); st.inout(Q, n_m, Q_d); st.inout(mu0, (size_t)B * r, mu_d); st.inout(P0, n_m, P0_d);
    st.out(f_smooth, (size_t)B * T * r, f_d); st.out(P_smooth, (size_t)B * T * np, P_d);
    st.out(loglik_path, (size_t)B * max_iter, ll_d); st.out(iters, (size_t)B, it_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_em_batch_dev(h, B, T, N, r, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, max_iter, tol, ll_d, it_d, f_d, P_d, flags));
    if (rc == 0) rc = post_check(h, loglik_path, B, (size_t)max_iter);
    return rc;
}
// ---- VAR(p) factor dynamics -------------------------------------------------------------------------
int dfm_ks_pass_varp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                               const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                               double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (!f_smooth || !loglik) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return varp_run(h, B, T, N, r, p, panel, const_cast<double*>(Lam), const_cast<double*>(R), const_cast<double*>(Avar),
                    const_cast<double*>(Q), const_cast<double*>(mu0), const_cast<double*>(P0), 1, 0.0, nullptr, nullptr,
                    loglik, f_smooth, P_smooth, flags, false);
}

int dfm_em_varp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, double* Lam, double* R,
                          double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                          int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (!loglik_path || !iters) return fail(h, DFM_E_NULL, "loglik_path / iters is NULL%s");
    return varp_run(h, B, T, N, r, p, panel, Lam, R, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, nullptr,
                    f_smooth, P_smooth, flags, true);
}

// host-pointer variants: one device block for inputs and outputs, parameters copied in and (EM) out
static int varp_host(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, double* Lam, double* R,
                     double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                     int* iters, double* f_smooth, double* P_smooth, double* loglik, unsigned flags, bool em) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (p < 1 || r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "need 1 <= p and r * p <= DFM_MAX_R (32)%s");
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (em ? (!loglik_path || !iters) : (!f_smooth || !loglik)) return fail(h, DFM_E_NULL, "required output pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, np = (size_t)r * (r + 1) / 2;
    double* ll = em ? loglik_path : loglik;                      // [B max_iter] | [B]
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    int* it_d;
    st.in(panel, (size_t)B * T * N, x_d); st.inout(Lam, (size_t)B * N * r, lam_d, em); st.inout(R, (size_t)B * N, R_d, em);
    st.inout(Avar, (size_t)B * r * k, A_d, em); st.inout(Q, (size_t)B * r * r, Q_d, em); st.inout(mu0, (size_t)B * k, mu_d, em);
    st.inout(P0, (size_t)B * k * k, P0_d, em);
    st.out(f_smooth, (size_t)B * T * r, f_d); st.out(P_smooth, (size_t)B * T * np, P_d);
    st.out(ll, em ? (size_t)B * max_iter : (size_t)B, ll_d); st.out(iters, (size_t)B, it_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(em ? dfm_em_varp_batch_dev(h, B, T, N, r, p, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, max_iter, tol, ll_d, it_d, f_d, P_d, flags)
                          : dfm_ks_pass_varp_batch_dev(h, B, T, N, r, p, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll, B, em ? (size_t)max_iter : (size_t)1);
    return rc;
}

int dfm_ks_pass_varp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                           double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    return varp_host(h, B, T, N, r, p, panel, const_cast<double*>(Lam), const_cast<double*>(R), const_cast<double*>(Avar),
                     const_cast<double*>(Q), const_cast<double*>(mu0), const_cast<double*>(P0), 1, 0.0, nullptr, nullptr,
                     f_smooth, P_smooth, loglik, flags, false);
}

int dfm_em_varp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, double* Lam, double* R,
                      double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                      int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return varp_host(h, B, T, N, r, p, panel, Lam, R, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth,
                     P_smooth, nullptr, flags, true);
}

// ---- AR idiosyncratic terms -----------------------------------------------------------------------
int dfm_ks_pass_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                             const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                             const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    return ar_pass_run(h, B, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, f_smooth, P_smooth, loglik, flags);
}

// host entry points: em = false is the pass (loglik_path = loglik [B], iters unused)
static int ar_host(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, double* Lam, double* sig2, double* rho,
                   double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path, int* iters,
                   double* f_smooth, double* P_smooth, unsigned flags, bool em) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (p < 1 || q < 0 || T <= q + (em ? 1 : 0))
        return fail(h, DFM_E_DIMS, em ? "need p >= 1, 0 <= q < T - 1%s" : "need p >= 1, 0 <= q < T%s");
    const int m = state_lags(p, q);
    if (r * m > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * max(p, q + 1) > DFM_MAX_R (32)%s");
    if (!panel || !Lam || !sig2 || (q > 0 && !rho) || !Avar || !Q || !mu0 || !P0 || !loglik_path || (em ? !iters : !f_smooth))
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * m, np = (size_t)r * (r + 1) / 2, Tq = (size_t)(T - q);
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *rho_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    int* it_d;
    st.in(panel, (size_t)B * T * N, x_d); st.inout(Lam, (size_t)B * N * r, lam_d, em); st.inout(sig2, (size_t)B * N, R_d, em);
    st.inout(rho, (size_t)B * N * q, rho_d, em); st.inout(Avar, (size_t)B * r * r * p, A_d, em); st.inout(Q, (size_t)B * r * r, Q_d, em);
    st.inout(mu0, (size_t)B * k, mu_d, em); st.inout(P0, (size_t)B * k * k, P0_d, em);
    st.out(f_smooth, (size_t)B * Tq * r, f_d); st.out(P_smooth, (size_t)B * Tq * np, P_d);
    st.out(loglik_path, (size_t)B * (em ? max_iter : 1), ll_d); st.out(iters, (size_t)B, it_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(em ? ar_em_run(h, B, T, N, r, p, q, x_d, lam_d, R_d, rho_d, A_d, Q_d, mu_d, P0_d, max_iter, tol, ll_d, it_d, f_d, P_d, flags)
                          : ar_pass_run(h, B, T, N, r, p, q, x_d, lam_d, R_d, rho_d, A_d, Q_d, mu_d, P0_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, loglik_path, B, em ? (size_t)max_iter : 1);
    return rc;
}

int dfm_ks_pass_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                         const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    return ar_host(h, B, T, N, r, p, q, panel, const_cast<double*>(Lam), const_cast<double*>(sig2), const_cast<double*>(rho),
                   const_cast<double*>(Avar), const_cast<double*>(Q), const_cast<double*>(mu0), const_cast<double*>(P0), 1, 0.0, loglik,
                   nullptr, f_smooth, P_smooth, flags, false);
}

int dfm_em_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, double* Lam, double* sig2,
                        double* rho, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                        double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return ar_em_run(h, B, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth,
                     P_smooth, flags);
}

int dfm_em_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, double* Lam, double* sig2,
                    double* rho, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                    int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return ar_host(h, B, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                   flags, true);
}

// ---- mixed frequency ---------------------------------------------------------------------------------------------------
int dfm_ks_pass_mf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, const double* Lam,
                             const double* R, const double* W, const double* Avar, const double* Q, const double* mu0,
                             const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    return mf_pass_run(h, B, T, N, r, p, L, panel, Lam, R, W, Avar, Q, mu0, P0, f_smooth, P_smooth, loglik, flags);
}

int dfm_em_mf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                        const double* W, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                        double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return mf_run(h, B, T, N, r, p, L, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                  flags);
}

int dfm_em_mf_blocks_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                               const double* W, const void* free_mask, double* Avar, double* Q, double* mu0, double* P0,
                               int max_iter, double tol, double* loglik_path, int* iters, double* f_smooth, double* P_smooth,
                               unsigned flags) {
    return mf_run(h, B, T, N, r, p, L, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                  flags, static_cast<const unsigned char*>(free_mask));
}

// host entry points: em = false is the pass (loglik_path = loglik [B], iters unused).  free_mask (EM only, may be NULL) is staged
// LAST and takes no space when it is NULL: the block of a call without one is laid out as it always was
static int mf_host(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                   const double* W, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                   int* iters, double* f_smooth, double* P_smooth, unsigned flags, bool em, const unsigned char* free_mask = nullptr) {
    if (int rc = mf_check(h, B, T, N, r, p, L)) return rc;
    if (!panel || !Lam || !R || !W || !Avar || !Q || !mu0 || !P0 || !loglik_path || (em && !iters) || (!em && !f_smooth))
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * (p > L ? p : L), np = (size_t)r * (r + 1) / 2;
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *w_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    int* it_d;
    unsigned char* m_d;
    st.in(panel, (size_t)B * T * N, x_d); st.inout(Lam, (size_t)B * N * r, lam_d, em); st.inout(R, (size_t)B * N, R_d, em);
    st.in(W, (size_t)N * L, w_d); st.inout(Avar, (size_t)B * r * r * p, A_d, em); st.inout(Q, (size_t)B * r * r, Q_d, em);
    st.inout(mu0, (size_t)B * k, mu_d, em); st.inout(P0, (size_t)B * k * k, P0_d, em);
    st.out(f_smooth, (size_t)B * T * r, f_d); st.out(P_smooth, (size_t)B * T * np, P_d);
    st.out(loglik_path, (size_t)B * (em ? max_iter : 1), ll_d); st.out(iters, (size_t)B, it_d);
    st.in(free_mask, free_mask ? (size_t)N * r : 0, m_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(em ? mf_run(h, B, T, N, r, p, L, x_d, lam_d, R_d, w_d, A_d, Q_d, mu_d, P0_d, max_iter, tol, ll_d, it_d, f_d, P_d, flags, m_d)
                          : mf_pass_run(h, B, T, N, r, p, L, x_d, lam_d, R_d, w_d, A_d, Q_d, mu_d, P0_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, loglik_path, B, em ? (size_t)max_iter : 1);
    return rc;
}

int dfm_ks_pass_mf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, const double* Lam,
                         const double* R, const double* W, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags) {
    return mf_host(h, B, T, N, r, p, L, panel, const_cast<double*>(Lam), const_cast<double*>(R), W, const_cast<double*>(Avar),
                   const_cast<double*>(Q), const_cast<double*>(mu0), const_cast<double*>(P0), 1, 0.0, loglik, nullptr, f_smooth,
                   P_smooth, flags, false);
}

int dfm_em_mf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                    const double* W, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                    int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return mf_host(h, B, T, N, r, p, L, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                   flags, true);
}

int dfm_em_mf_blocks_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                           const double* W, const void* free_mask, double* Avar, double* Q, double* mu0, double* P0,
                           int max_iter, double tol, double* loglik_path, int* iters, double* f_smooth, double* P_smooth,
                           unsigned flags) {
    return mf_host(h, B, T, N, r, p, L, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                   flags, true, static_cast<const unsigned char*>(free_mask));
}

// ---- observed factors ------------------------------------------------------------------------------------------------
int dfm_em_obs_batch_dev(dfm_handle* h, int B, int T, int N, int r_u, int r_o, const double* panel, const double* G, double* Lam,
                         double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                         int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    return obs_em_run(h, B, T, N, r_u, r_o, panel, G, Lam, R, A, Q, mu0, P0, max_iter, tol, loglik_path, iters, f_smooth, P_smooth,
                      flags);
}

int dfm_em_obs_batch(dfm_handle* h, int B, int T, int N, int r_u, int r_o, const double* panel, const double* G, double* Lam,
                     double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                     int* iters, double* f_smooth, double* P_smooth, unsigned flags) {
    if (int rc = check_dims(h, B, T, N, r_u)) return rc;
    if (r_o < 1 || r_o + r_u > 32) return fail(h, DFM_E_R_UNSUPPORTED, "observed factors: need r_o >= 1 and r_o + r_u <= 32%s");
    if (!panel || !G || !Lam || !R || !A || !Q || !mu0 || !P0 || !loglik_path || !iters)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter < 1) return fail(h, DFM_E_DIMS, "max_iter must be >= 1%s");
    for (size_t k = 0; k < (size_t)B * T * r_o; ++k)
        if (G[k] != G[k]) return fail(h, DFM_E_MISSING, "observed factors must not contain NaN%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t re = (size_t)r_o + r_u, np = (size_t)r_u * (r_u + 1) / 2, n_m = (size_t)B * r_u * r_u;
    HostStage st(h);
    double *x_d, *g_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *f_d, *P_d, *ll_d;
    int* it_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(G, (size_t)B * T * r_o, g_d); st.inout(Lam, (size_t)B * N * re, lam_d);
    st.inout(R, (size_t)B * N, R_d); st.inout(A, n_m, A_d); st.inout(Q, n_m, Q_d); st.inout(mu0, (size_t)B * r_u, mu_d);
    st.inout(P0, n_m, P0_d);
    st.out(f_smooth, (size_t)B * T * r_u, f_d); st.out(P_smooth, (size_t)B * T * np, P_d);
    st.out(loglik_path, (size_t)B * max_iter, ll_d); st.out(iters, (size_t)B, it_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(obs_em_run(h, B, T, N, r_u, r_o, x_d, g_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, max_iter, tol, ll_d, it_d, f_d, P_d, flags));
    if (rc == 0) rc = post_check(h, loglik_path, B, (size_t)max_iter);
    return rc;
}

int dfm_pca_init_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                           double* A, double* Q, double* mu0, double* P0, double* factors) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 2 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, N, r must be >= 1 and T >= 2%s");
    if (r > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r > DFM_MAX_R (32)%s");
    if (r > N || r > T - 1) return fail(h, DFM_E_DIMS, "r must not exceed N or T - 1%s");
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const int Rp = pad_r(r);
    const size_t d = sizeof(double);
    size_t off = 0;
    const size_t oS = take(off, (size_t)B * N * N * d), oV = take(off, (size_t)B * N * Rp * d),
                 oY = take(off, (size_t)B * N * Rp * d), oF = take(off, (size_t)B * T * Rp * d), oSt = take(off, 256);
    if (int rc = ensure_ws(h, off)) return rc;
    PcaArgs pa;
    pa.B = B; pa.T = T; pa.N = N; pa.r = r; pa.max_iter = 4000;
    { static const int mi = [] { const char* v = diag_env("DFM_PCA_MAXIT"); return v ? atoi(v) : 0; }(); if (mi > 0) pa.max_iter = mi; }   // diagnostics
    { static const int stop = [] { const char* v = diag_env("DFM_PCA_STOP"); return v ? atoi(v) : 0; }(); pa.stop_after = stop; }
    pa.panel = panel;
    pa.S = at<double>(h, oS); pa.V = at<double>(h, oV); pa.Y = at<double>(h, oY); pa.F = at<double>(h, oF);
    pa.Lam = Lam; pa.Rv = R; pa.A = A; pa.Q = Q; pa.mu0 = mu0; pa.P0 = P0; pa.factors = factors;
    pa.status = h->status_dev;
    HIP_LAUNCH(h, K_GRAM_XX, launch_gram_xx(pa, h->stream, h->opt.gram_xx_valu ? 1 : 0));
    HIP_LAUNCH(h, K_PCA, launch_pca(Rp, pa, h->stream));
    return 0;
}

int dfm_pca_init_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                       double* A, double* Q, double* mu0, double* P0, double* factors) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 2 || N < 1 || r < 1 || r > DFM_MAX_R) return fail(h, DFM_E_DIMS, "bad dimensions%s");
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_panel = (size_t)B * T * N, n_m = (size_t)B * r * r;
    for (size_t k = 0; k < n_panel; ++k)
        if (panel[k] != panel[k]) return fail(h, DFM_E_MISSING, "PCA initialisation needs a balanced panel (NaN found)%s");
    HostStage st(h);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *P0_d, *mu_d, *f_d;
    st.in(panel, n_panel, x_d); st.out(Lam, (size_t)B * N * r, lam_d); st.out(R, (size_t)B * N, R_d); st.out(A, n_m, A_d);
    st.out(Q, n_m, Q_d); st.out(P0, n_m, P0_d); st.out(mu0, (size_t)B * r, mu_d); st.out(factors, (size_t)B * T * r, f_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_pca_init_batch_dev(h, B, T, N, r, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, f_d));
    if (rc == 0) rc = status_check(h);
    return rc;
}
int dfm_synth_panels_dev(dfm_handle* h, uint64_t seed, int64_t first_replicate, int B, int T, int N, int r,
                         double missing_prob, double* panel, double* Lam, double* R, double* A, double* Q,
                         double* mu0, double* P0) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 2 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, N, r must be >= 1 and T >= 2%s");
    if (r > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r > DFM_MAX_R (32)%s");
    if (!(missing_prob >= 0.0 && missing_prob < 1.0)) return fail(h, DFM_E_DIMS, "missing_prob must be in [0, 1)%s");
    if (!panel || !Lam || !R || !A || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    size_t off = 0;
    const size_t oF = take(off, (size_t)B * (T + 1) * r * sizeof(double));
    const size_t oC = take(off, (size_t)B * synth_tiles(T) * 2 * N * sizeof(double));
    if (int rc = ensure_ws(h, off)) return rc;
    SynthArgs sa;
    sa.B = B; sa.T = T; sa.N = N; sa.r = r; sa.seed = seed; sa.first_replicate = first_replicate;
    sa.missing_prob = missing_prob;
    sa.panel = panel; sa.Lam = Lam; sa.R = R; sa.A = A; sa.Q = Q; sa.mu0 = mu0; sa.P0 = P0;
    sa.fscratch = at<double>(h, oF);
    sa.colstats = at<double>(h, oC);
    HIP_LAUNCH(h, K_SYNTH, launch_synth(sa, h->stream));
    return 0;
}

}  // extern "C"


// ---- non-parametric estimator: batched ALS and batched complete-case OLS (als.hip) ---------------------
int dfm_als_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* z, long long z_stride,
                      const int* r_each, double* F, double* Lam, int nt_min, int max_iter, double tol,
                      double* ssr_path, int path_cap, int* iters, double* ssr, double* R2) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 1 || N < 1 || r < 1 || max_iter < 1 || z_stride < 0 || (ssr_path && path_cap < 1))
        return fail(h, DFM_E_DIMS, "B, T, N, r, max_iter must be >= 1, z_stride >= 0%s");
    if (r > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r > DFM_MAX_R (32)%s");
    if (!z || !F || !Lam || !iters || !ssr) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    const int Rp = pad_r(r);
    if (!als_fits(Rp, T, N)) return fail(h, DFM_E_DIMS, "(T + N) * pad(r) doubles exceed the 160 KB of LDS%s");
    HIP_TRY(h, hipSetDevice(h->device));
    AlsArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.N = N; a.rmax = r; a.z = z; a.z_stride = z_stride; a.r_each = r_each; a.F = F; a.Lam = Lam;
    a.nt_min = nt_min; a.max_iter = max_iter; a.tol = tol; a.ssr_path = ssr_path; a.path_cap = ssr_path ? path_cap : 0;
    a.iters = iters; a.ssr = ssr; a.R2 = R2;
    HIP_LAUNCH(h, K_ALS, launch_als(Rp, a, h->stream));
    return 0;
}

int dfm_als_batch(dfm_handle* h, int B, int T, int N, int r, const double* z, long long z_stride, const int* r_each,
                  double* F, double* Lam, int nt_min, int max_iter, double tol, double* ssr_path, int path_cap,
                  int* iters, double* ssr, double* R2) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 1 || N < 1 || r < 1 || z_stride < 0) return fail(h, DFM_E_DIMS, "B, T, N, r must be >= 1%s");
    if (!z || !F || !Lam || !iters || !ssr) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_z = z_stride == 0 ? (size_t)T * N : (size_t)(B - 1) * z_stride + (size_t)T * N;
    HostStage st(h);
    double *z_d, *F_d, *L_d, *p_d, *R2_d, *ssr_d;
    int *it_d, *re_d;
    st.in(z, n_z, z_d); st.inout(F, (size_t)B * T * r, F_d); st.out(Lam, (size_t)B * N * r, L_d);
    st.out(ssr_path, ssr_path ? (size_t)B * path_cap : 0, p_d); st.out(R2, R2 ? (size_t)B * N : 0, R2_d); st.out(ssr, (size_t)B, ssr_d);
    st.out(iters, (size_t)B, it_d); st.in(r_each, (size_t)B, re_d);
    if (int rc = st.begin()) return rc;
    return st.finish(dfm_als_batch_dev(h, B, T, N, r, z_d, z_stride, re_d, F_d, L_d, nt_min, max_iter, tol, p_d, path_cap, it_d, ssr_d, R2_d));
}

int dfm_ols_batch_dev(dfm_handle* h, int P, int T, int K, const double* X, long long x_stride, const double* y,
                      long long y_stride, long long y_inc, int nt_min, double* beta, double* resid, double* ssr,
                      double* tss, int* nobs) {
    if (!h) return DFM_E_NULL;
    if (P < 1 || T < 1 || K < 1 || x_stride < 0 || y_inc < 1 || y_stride < 0)
        return fail(h, DFM_E_DIMS, "P, T, K, y_inc must be >= 1, strides >= 0%s");
    if (K > 64) return fail(h, DFM_E_R_UNSUPPORTED, "K > 64 regressors%s");
    if (!X || !y || !beta || !ssr || !nobs) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    OlsArgs a;
    memset(&a, 0, sizeof(a));
    a.P = P; a.T = T; a.K = K; a.X = X; a.x_stride = x_stride; a.y = y; a.y_stride = y_stride; a.y_inc = y_inc;
    a.nt_min = nt_min; a.beta = beta; a.resid = resid; a.ssr = ssr; a.tss = tss; a.nobs = nobs;
    HIP_LAUNCH(h, K_OLS, launch_ols(K > 32 ? 64 : pad_r(K), a, h->stream));
    return 0;
}

int dfm_ols_batch(dfm_handle* h, int P, int T, int K, const double* X, long long x_stride, const double* y,
                  long long y_stride, long long y_inc, int nt_min, double* beta, double* resid, double* ssr,
                  double* tss, int* nobs) {
    if (!h) return DFM_E_NULL;
    if (P < 1 || T < 1 || K < 1 || x_stride < 0 || y_inc < 1 || y_stride < 0)
        return fail(h, DFM_E_DIMS, "P, T, K, y_inc must be >= 1, strides >= 0%s");
    if (!X || !y || !beta || !ssr || !nobs) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_X = (x_stride == 0 ? 0 : (size_t)(P - 1) * x_stride) + (size_t)T * K;
    const size_t n_y = (size_t)(P - 1) * y_stride + (size_t)(T - 1) * y_inc + 1;
    HostStage st(h);
    double *X_d, *y_d, *b_d, *e_d, *ssr_d, *tss_d;
    int* n_d;
    st.in(X, n_X, X_d); st.in(y, n_y, y_d); st.out(beta, (size_t)P * K, b_d); st.out(resid, resid ? (size_t)P * T : 0, e_d);
    st.out(ssr, (size_t)P, ssr_d); st.out(tss, (size_t)P, tss_d); st.out(nobs, (size_t)P, n_d);
    if (int rc = st.begin()) return rc;
    return st.finish(dfm_ols_batch_dev(h, P, T, K, X_d, x_stride, y_d, y_stride, y_inc, nt_min, b_d, e_d, ssr_d, tss_d, n_d));
}


// ---- wild-bootstrap IRF bands (boot.hip) -----------------------------------------------------------------
int dfm_var_bootstrap_irf_dev(dfm_handle* h, int B, int T, int ns, int p, int H, const double* y, const double* betahat,
                              const double* resid, const double* signs, uint64_t seed, int64_t first_draw, double* beta_out,
                              double* irf) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || ns < 1 || p < 1 || H < 1 || T <= p + 1 + ns * p)
        return fail(h, DFM_E_DIMS, "B, ns, p, H must be >= 1 and T > p + 1 + ns p%s");
    if (ns > 8 || 1 + ns * p > 64) return fail(h, DFM_E_R_UNSUPPORTED, "ns > 8 or 1 + ns p > 64%s");
    if (!y || !betahat || !resid || !irf) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    BootArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.T = T; a.ns = ns; a.p = p; a.H = H; a.y = y; a.betahat = betahat; a.resid = resid; a.signs = signs;
    a.seed = seed; a.first_draw = first_draw; a.beta_out = beta_out; a.irf = irf;
    hipError_t e;
    { ProfScope ps(h, K_BOOT); e = launch_var_boot(a, h->stream); }
    if (e == hipErrorInvalidValue) return fail(h, DFM_E_DIMS, "T x ns too large for the bootstrap kernel's LDS%s");
    HIP_TRY(h, e);
    return 0;
}

int dfm_var_bootstrap_irf(dfm_handle* h, int B, int T, int ns, int p, int H, const double* y, const double* betahat,
                          const double* resid, const double* signs, uint64_t seed, int64_t first_draw, double* beta_out,
                          double* irf) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || ns < 1 || p < 1 || H < 1 || T < 1) return fail(h, DFM_E_DIMS, "B, T, ns, p, H must be >= 1%s");
    if (!y || !betahat || !resid || !irf) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t K = 1 + (size_t)ns * p, n_y = (size_t)T * ns;
    HostStage st(h);
    double *y_d, *b_d, *e_d, *s_d, *bo_d, *irf_d;
    st.in(y, n_y, y_d); st.in(betahat, K * ns, b_d); st.in(resid, n_y, e_d); st.in(signs, signs ? (size_t)B * T : 0, s_d);
    st.out(beta_out, beta_out ? (size_t)B * K * ns : 0, bo_d); st.out(irf, (size_t)B * ns * H * ns, irf_d);
    if (int rc = st.begin()) return rc;
    return st.finish(dfm_var_bootstrap_irf_dev(h, B, T, ns, p, H, y_d, b_d, e_d, s_d, seed, first_draw, bo_d, irf_d));
}

int dfm_quantile_bands_dev(dfm_handle* h, int B, int S, int nq, const double* x, const double* q, double* out) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || S < 1 || nq < 1 || B > 16384) return fail(h, DFM_E_DIMS, "B in 1..16384, S, nq >= 1%s");
    if (!x || !q || !out) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    QuantArgs a;
    a.B = B; a.S = S; a.nq = nq; a.x = x; a.q = q; a.out = out;
    HIP_LAUNCH(h, K_QUANT, launch_quantiles(a, h->stream));
    return 0;
}

int dfm_quantile_bands(dfm_handle* h, int B, int S, int nq, const double* x, const double* q, double* out) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || S < 1 || nq < 1) return fail(h, DFM_E_DIMS, "B, S, nq must be >= 1%s");
    if (!x || !q || !out) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    HostStage st(h);
    double *x_d, *q_d, *o_d;
    st.in(x, (size_t)B * S, x_d); st.in(q, (size_t)nq, q_d); st.out(out, (size_t)nq * S, o_d);
    if (int rc = st.begin()) return rc;
    return st.finish(dfm_quantile_bands_dev(h, B, S, nq, x_d, q_d, o_d));
}


// ---- Chow / QLR statistics with HAC covariance (breaks.hip) ---------------------------------------------
int dfm_chow_batch_dev(dfm_handle* h, int S, int Tmax, int k, const double* y, const double* X, const int* Tlen, int P,
                       const int* prob_series, const int* prob_break, const int* prob_q, double* chow) {
    if (!h) return DFM_E_NULL;
    if (S < 1 || Tmax < 1 || k < 1 || P < 1) return fail(h, DFM_E_DIMS, "S, Tmax, k, P must be >= 1%s");
    if (k > 8) return fail(h, DFM_E_R_UNSUPPORTED, "k > 8 regressors%s");
    if (!y || !X || !Tlen || !prob_series || !prob_break || !prob_q || !chow)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    ChowArgs a;
    a.S = S; a.Tmax = Tmax; a.k = k; a.P = P; a.y = y; a.X = X; a.Tlen = Tlen; a.prob_series = prob_series;
    a.prob_break = prob_break; a.prob_q = prob_q; a.chow = chow;
    HIP_LAUNCH(h, K_CHOW, launch_chow(a, h->stream));
    return 0;
}

int dfm_chow_batch(dfm_handle* h, int S, int Tmax, int k, const double* y, const double* X, const int* Tlen, int P,
                   const int* prob_series, const int* prob_break, const int* prob_q, double* chow) {
    if (!h) return DFM_E_NULL;
    if (S < 1 || Tmax < 1 || k < 1 || P < 1) return fail(h, DFM_E_DIMS, "S, Tmax, k, P must be >= 1%s");
    if (!y || !X || !Tlen || !prob_series || !prob_break || !prob_q || !chow)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    for (int p = 0; p < P; ++p) {
        const int s = prob_series[p];
        if (s < 0 || s >= S || prob_q[p] < 0 || prob_q[p] > 15 || Tlen[s] < 1 || Tlen[s] > Tmax || prob_break[p] < 0 ||
            prob_break[p] > Tlen[s])
            return fail(h, DFM_E_DIMS, "problem list: series, break date or bandwidth out of range%s");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_y = (size_t)S * Tmax;
    HostStage st(h);
    double *y_d, *X_d, *c_d;
    int *T_d, *ps_d, *pb_d, *pq_d;
    st.in(y, n_y, y_d); st.in(X, n_y * k, X_d); st.out(chow, (size_t)P, c_d);
    st.in(Tlen, (size_t)S, T_d); st.in(prob_series, (size_t)P, ps_d); st.in(prob_break, (size_t)P, pb_d); st.in(prob_q, (size_t)P, pq_d);
    if (int rc = st.begin()) return rc;
    return st.finish(dfm_chow_batch_dev(h, S, Tmax, k, y_d, X_d, T_d, P, ps_d, pb_d, pq_d, c_d));
}


int dfm_standardize_batch_dev(dfm_handle* h, int B, int T, int N, double* panel, double* mean, double* sd) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 1 || N < 1) return fail(h, DFM_E_DIMS, "B, T, N must be >= 1%s");
    if (!panel) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_standardize(B, T, N, panel, mean, sd, h->stream));
    return 0;
}


// ---- nowcasts and forecasts of the panel (forecast.hip) ---------------------------------------------------------------
// p = 1: the plain pass on the caller's T-row panel (its own route: fused balanced pass, chunked recursion, pipe, odd-N pad) into
// h->fc, forecast_tail_kernel for the H rows behind it, forecast_fill_kernel for the panel-sized outputs (it also writes f_out /
// P_out in the T + H row layout).  p > 1: the panel with H all-missing rows appended goes into xhat, the companion pass runs on it
// as a (T + H)-row panel with missing cells straight into f_out / P_out (the smoothed moments of the empty rows are the forecast
// moments), forecast_fill_kernel rewrites xhat in place.
static int forecast_check(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                          const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                          const double* mean, const double* sd, const double* xhat, const double* f_out) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !xhat || !f_out)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    return 0;
}
int dfm_forecast_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                           const double* mean, const double* sd, double* xhat, double* xvar, double* common, double* f_out,
                           double* P_out, double* loglik, unsigned flags) {
    if (int rc = forecast_check(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, xhat, f_out)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), np = (size_t)r * (r + 1) / 2, TH = (size_t)T + H;
    const bool needP = xvar != nullptr || P_out != nullptr;
    FcFillArgs fa{};
    fa.B = B; fa.T = T; fa.H = H; fa.N = N; fa.r = r;
    fa.Lam = Lam; fa.R = R; fa.mean = mean; fa.sd = sd;
    fa.xhat = xhat; fa.xvar = xvar; fa.common = common;
    if (p == 1) {
        size_t off = 0;
        const size_t o_f = take(off, (size_t)B * T * r * d), o_P = needP ? take(off, (size_t)B * T * np * d) : (size_t)-1,
                     o_ft = H ? take(off, (size_t)B * H * r * d) : (size_t)-1,
                     o_Pt = (H && needP) ? take(off, (size_t)B * H * np * d) : (size_t)-1, o_ll = take(off, (size_t)B * d);
        HIP_TRY(h, h->fc.grow(off));
        double *fsm = at<double>(h->fc, o_f), *Psm = at<double>(h->fc, o_P), *ft = at<double>(h->fc, o_ft), *Pt = at<double>(h->fc, o_Pt);
        if (int rc = dfm_ks_pass_batch_dev(h, B, T, N, r, panel, Lam, R, Avar, Q, mu0, P0, fsm, Psm,
                                           loglik ? loglik : at<double>(h->fc, o_ll), flags)) return rc;
        if (H) {
            FcTailArgs ta{B, T, H, r, fsm, Psm, Avar, Q, ft, Pt};
            HIP_LAUNCH(h, K_FC_TAIL, launch_forecast_tail(ta, h->stream));
        }
        fa.panel = panel; fa.panel_rows = T;
        fa.fh = fsm; fa.Ph = needP ? Psm : nullptr; fa.Th = T; fa.ft = ft; fa.Pt = Pt;
        fa.f_out = f_out; fa.P_out = P_out;
    } else {
        double* Pbuf = P_out;
        size_t off = 0;
        const size_t o_P = (!P_out && xvar) ? take(off, (size_t)B * TH * np * d) : (size_t)-1, o_ll = take(off, (size_t)B * d);
        HIP_TRY(h, h->fc.grow(off));
        if (o_P != (size_t)-1) Pbuf = at<double>(h->fc, o_P);
        HIP_LAUNCH(h, K_FC_PAD, launch_forecast_pad(B, T, H, N, panel, xhat, !(flags & DFM_F_MAY_HAVE_MISSING), h->status_dev, h->stream));
        if (int rc = dfm_ks_pass_varp_batch_dev(h, B, (int)TH, N, r, p, xhat, Lam, R, Avar, Q, mu0, P0, f_out, Pbuf,
                                                loglik ? loglik : at<double>(h->fc, o_ll),
                                                flags | DFM_F_MAY_HAVE_MISSING)) return rc;
        fa.panel = xhat; fa.panel_rows = (int)TH;
        fa.fh = f_out; fa.Ph = xvar ? Pbuf : nullptr; fa.Th = (int)TH; fa.ft = nullptr; fa.Pt = nullptr;
        fa.f_out = nullptr; fa.P_out = nullptr;
    }
    HIP_LAUNCH(h, K_FC_FILL, launch_forecast_fill(fa, h->stream));
    return 0;
}

int dfm_forecast_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                       const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                       const double* mean, const double* sd, double* xhat, double* xvar, double* common, double* f_out,
                       double* P_out, double* loglik, unsigned flags) {
    if (int rc = forecast_check(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, xhat, f_out)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t np = (size_t)r * (r + 1) / 2, TH = (size_t)T + H, n_x = (size_t)B * TH * N;
    std::vector<double> ll_host((size_t)B);                     // (checked before the caller's loglik, which is optional, is written)
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *xh_d, *xv_d, *cm_d, *f_d, *P_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d);
    stage_model(st, md, B, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, mean, sd);
    st.out(xhat, n_x, xh_d); st.out(xvar, xvar ? n_x : 0, xv_d); st.out(common, common ? n_x : 0, cm_d);
    st.out(f_out, (size_t)B * TH * r, f_d); st.out(P_out, P_out ? (size_t)B * TH * np : 0, P_d); st.out(ll_host.data(), (size_t)B, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_forecast_batch_dev(h, B, T, N, r, p, H, x_d, md.Lam, md.R, md.A, md.Q, md.mu0, md.P0, md.mean, md.sd, xh_d, xv_d,
                                              cm_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), B);
    if (rc == 0 && loglik) memcpy(loglik, ll_host.data(), (size_t)B * sizeof(double));
    return rc;
}


// ---- nowcasts and forecasts with AR idiosyncratic terms (forecast_ar.hip) -----------------------------------------------------
// The panel with H all-missing rows appended goes into h->fc (xhat has q rows too few to hold it), the AR pass runs on its T + H
// rows straight into f_out / P_out (quasi-differencing a NaN row gives NaN rows: the smoothed moments of the empty rows are the
// forecast moments), then per slice of replicates the backward kernel leaves its messages in h->fc and the forward kernel writes
// the cells.  A slice is as many replicates as fit the cap of the message buffer (RouteOpts::fcar_msg_cap), at least one: the
// buffer does not grow with B.
static int forecast_ar_check(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* panel, const double* Lam,
                             const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                             const double* P0, const double* mean, const double* sd, const double* xhat, const double* f_out) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be >= 1 (q = 0 is dfm_forecast_batch)%s");
    if (T <= q) return fail(h, DFM_E_DIMS, "T must exceed the number of idiosyncratic lags%s");
    if (q > 4) return fail(h, DFM_E_R_UNSUPPORTED, "forecasts with AR idiosyncratic terms need q <= 4%s");
    if ((long long)T + H > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "T + H must be < 2^31%s");
    if (int rc = ar_check(h, B, T + H, N, r, p, q, false)) return rc;
    if (!panel || !Lam || !sig2 || !rho || !Avar || !Q || !mu0 || !P0 || !xhat || !f_out)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    return 0;
}

int dfm_forecast_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* panel, const double* Lam,
                              const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                              const double* P0, const double* v0, const double* mean, const double* sd, double* xhat, double* xvar,
                              double* common, double* idio, double* f_out, double* P_out, double* loglik, unsigned flags) {
    if (int rc = forecast_ar_check(h, B, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, xhat, f_out)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), np = (size_t)r * (r + 1) / 2, TH = (size_t)T + H, n = TH - q;
    const size_t per = forecast_ar_msg_bytes((int)n, N, q);
    size_t Sl = h->opt.fcar_msg_cap / per;
    if (Sl < 1) Sl = 1;
    if (Sl > (size_t)B) Sl = (size_t)B;
    size_t off = 0;
    const size_t o_x = take(off, (size_t)B * TH * N * d), o_P = (!P_out && xvar) ? take(off, (size_t)B * n * np * d) : (size_t)-1,
                 o_ll = loglik ? (size_t)-1 : take(off, (size_t)B * d), o_msg = take(off, Sl * per),
                 o_last = take(off, Sl * N * sizeof(int));
    HIP_TRY(h, h->fc.grow(off));
    double* xpad = at<double>(h->fc, o_x);
    double* Pbuf = P_out ? P_out : at<double>(h->fc, o_P);
    HIP_LAUNCH(h, K_FC_PAD, launch_forecast_pad(B, T, H, N, panel, xpad, !(flags & DFM_F_MAY_HAVE_MISSING), h->status_dev, h->stream));
    if (int rc = ar_pass_run(h, B, (int)TH, N, r, p, q, xpad, Lam, sig2, rho, Avar, Q, mu0, P0, f_out, Pbuf,
                             loglik ? loglik : at<double>(h->fc, o_ll), flags | DFM_F_MAY_HAVE_MISSING)) return rc;
    FcArArgs a{};
    a.n = (int)n; a.N = N; a.r = r; a.q = q;
    a.panel = xpad; a.f = f_out; a.P = xvar ? Pbuf : nullptr;
    a.Lam = Lam; a.sig2 = sig2; a.rho = rho; a.v0 = v0; a.mean = mean; a.sd = sd;
    a.msg = at<double>(h->fc, o_msg); a.last = at<int>(h->fc, o_last);
    a.xhat = xhat; a.xvar = xvar; a.common = common; a.idio = idio;
    for (size_t b0 = 0; b0 < (size_t)B; b0 += Sl) {
        a.b0 = (int)b0; a.S = (int)((size_t)B - b0 < Sl ? (size_t)B - b0 : Sl);
        HIP_LAUNCH(h, K_FCAR_BACK, launch_forecast_ar_back(a, h->stream));
        HIP_LAUNCH(h, K_FCAR_FWD, launch_forecast_ar_fwd(a, h->stream));
    }
    return 0;
}

int dfm_forecast_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* panel, const double* Lam,
                          const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                          const double* P0, const double* v0, const double* mean, const double* sd, double* xhat, double* xvar,
                          double* common, double* idio, double* f_out, double* P_out, double* loglik, unsigned flags) {
    if (int rc = forecast_ar_check(h, B, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, xhat, f_out)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t np = (size_t)r * (r + 1) / 2, n = (size_t)T + H - q, n_x = (size_t)B * n * N;
    std::vector<double> ll_host((size_t)B);                     // (checked before the caller's loglik, which is optional, is written)
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *xh_d, *xv_d, *cm_d, *id_d, *f_d, *P_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d);
    stage_model(st, md, B, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd);
    st.out(xhat, n_x, xh_d); st.out(xvar, xvar ? n_x : 0, xv_d); st.out(common, common ? n_x : 0, cm_d); st.out(idio, idio ? n_x : 0, id_d);
    st.out(f_out, (size_t)B * n * r, f_d); st.out(P_out, P_out ? (size_t)B * n * np : 0, P_d); st.out(ll_host.data(), (size_t)B, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_forecast_ar_batch_dev(h, B, T, N, r, p, q, H, x_d, md.Lam, md.R, md.rho, md.A, md.Q, md.mu0, md.P0, md.v0, md.mean,
                                                 md.sd, xh_d, xv_d, cm_d, id_d, f_d, P_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), B);
    if (rc == 0 && loglik) memcpy(loglik, ll_host.data(), (size_t)B * sizeof(double));
    return rc;
}

// ---- posterior draws of factor and panel paths: the simulation smoother (simsmooth.hip) --------------------------------------
// Per slice of at most kSsSlice pass replicates j = b D + d: expand the parameters (mu0 = 0), simulate f+ into f_draw, stream the
// difference panels, run the existing pass on them into h->ss, add its smoothed mean and draw the horizon, then (x_draw) the cells.
// The difference panels of a slice live at the start of that slice's part of x_draw when the caller takes x_draw (the fill reads
// only the panel and f_draw, and runs after the pass in stream order), else in h->ss.
static constexpr int kSsSlice = 8192;

// The pass over one slice of S expanded replicates (simsmooth_run's difference panels, news_run's covariance panels) with the
// parameters simsmooth_expand_kernel left in e: the plain pass at p = 1, the companion pass beyond; smoothed means only.
static int slice_pass(dfm_handle* h, int S, int T, int N, int r, int p, const double* panels, const SsArgs& e, double* g, double* ll,
                      unsigned flags) {
    if (p == 1) return dfm_ks_pass_batch_dev(h, S, T, N, r, panels, e.eLam, e.eR, e.eA, e.eQ, e.emu0, e.eP0, g, nullptr, ll, flags);
    return dfm_ks_pass_varp_batch_dev(h, S, T, N, r, p, panels, e.eLam, e.eR, e.eA, e.eQ, e.emu0, e.eP0, g, nullptr, ll, flags);
}

static int simsmooth_check(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                           const double* mean, const double* sd, const double* f_draw) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (D < 1) return fail(h, DFM_E_DIMS, "D (draws per replicate) must be >= 1%s");
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (T < p) return fail(h, DFM_E_DIMS, "T must be >= p (the horizon starts from the last p rows of the draw)%s");
    if ((long long)B * D > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * D must be < 2^31%s");
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !f_draw) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    return 0;
}

// ll_all: [B D] device log-likelihoods of the difference panels (the host entry checks them), or null (h->ss, per slice)
static int simsmooth_run(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                         const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                         const double* mean, const double* sd, uint64_t seed, int64_t first_draw, double* f_draw,
                         double* x_draw, double* ll_all, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), k = (size_t)r * p, TH = (size_t)T + H;
    const long long BD = (long long)B * D;
    const int Smax = (int)(BD < kSsSlice ? BD : kSsSlice);
    size_t off = 0;
    const size_t o_LP0 = take(off, (size_t)B * k * k * d), o_LQ = take(off, (size_t)B * r * r * d);
    const SliceParams sp(off, Smax, N, r, k, 0);
    const size_t o_g = take(off, (size_t)Smax * T * r * d), o_ll = ll_all ? (size_t)-1 : take(off, (size_t)Smax * d),
                 o_x = x_draw ? (size_t)-1 : take(off, (size_t)Smax * T * N * d);
    HIP_TRY(h, h->ss.grow(off));
    SsArgs a{};
    a.B = B; a.D = D; a.T = T; a.N = N; a.r = r; a.p = p; a.H = H;
    a.panel = panel; a.Lam = Lam; a.R = R; a.A = Avar; a.Q = Q; a.mu0 = mu0; a.P0 = P0; a.mean = mean; a.sd = sd;
    a.seed = seed; a.first_draw = first_draw; a.f_draw = f_draw; a.x_draw = x_draw;
    a.LP0 = at<double>(h->ss, o_LP0); a.LQ = at<double>(h->ss, o_LQ); a.g = at<double>(h->ss, o_g);
    sp.point(h->ss, a);
    HIP_LAUNCH(h, K_SS_PREP, launch_simsmooth_prep(a, h->stream));
    for (long long j0 = 0; j0 < BD; j0 += Smax) {
        const int S = (int)(BD - j0 < Smax ? BD - j0 : Smax);
        a.j0 = j0; a.S = S;
        a.diff = x_draw ? x_draw + (size_t)j0 * TH * N : at<double>(h->ss, o_x);
        double* ll = ll_all ? ll_all + j0 : at<double>(h->ss, o_ll);
        HIP_LAUNCH(h, K_SS_EXPAND, launch_simsmooth_expand(a, h->stream));
        HIP_LAUNCH(h, K_SS_PATH, launch_simsmooth_path(a, h->stream));
        HIP_LAUNCH(h, K_SS_DIFF, launch_simsmooth_diff(a, h->stream));
        if (int rc = slice_pass(h, S, T, N, r, p, a.diff, a, at<double>(h->ss, o_g), ll, flags)) return rc;
        HIP_LAUNCH(h, K_SS_FINISH, launch_simsmooth_finish(a, h->stream));
        if (x_draw) HIP_LAUNCH(h, K_SS_FILL, launch_simsmooth_fill(a, h->stream));
    }
    return 0;
}

int dfm_simsmooth_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel,
                            const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                            const double* P0, const double* mean, const double* sd, uint64_t seed, int64_t first_draw,
                            double* f_draw, double* x_draw, unsigned flags) {
    if (int rc = simsmooth_check(h, B, D, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, f_draw)) return rc;
    return simsmooth_run(h, B, D, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, seed, first_draw, f_draw, x_draw,
                         nullptr, flags);
}

int dfm_simsmooth_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                        const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                        const double* mean, const double* sd, uint64_t seed, int64_t first_draw, double* f_draw,
                        double* x_draw, unsigned flags) {
    if (int rc = simsmooth_check(h, B, D, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, f_draw)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t TH = (size_t)T + H, BD = (size_t)B * D;
    std::vector<double> ll_host(BD);
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *f_d, *xo_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d);
    stage_model(st, md, B, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, mean, sd);
    st.out(f_draw, BD * TH * r, f_d); st.out(x_draw, x_draw ? BD * TH * N : 0, xo_d); st.out(ll_host.data(), BD, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(simsmooth_run(h, B, D, T, N, r, p, H, x_d, md.Lam, md.R, md.A, md.Q, md.mu0, md.P0, md.mean, md.sd, seed, first_draw,
                                     f_d, xo_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), (int)BD);
    return rc;
}

// ---- posterior path draws with AR idiosyncratic terms (simsmooth_ar.hip) ------------------------------------------------------
// The factor side runs the kernels above on the state of m = max(p, q + 1) lags (Avar padded with zero blocks), with T = n output
// rows and no horizon of its own: the horizon rows are rows of the path.  Per slice of pass replicates j = b D + d: expand the
// parameters (mu0 = 0; rho by simsmooth_ar_expand_kernel), f+ into f_draw, the difference panels, the AR pass on them into g, then
// (x_draw) the backward messages of forecast_ar_back_kernel on (difference panel, g) and the assembling forward kernel, and
// f_draw += g behind it.  A slice is min(kSsSlice, fcar_msg_cap / one replicate's messages) pass replicates, at least one;
// everything of a slice lives in h->ss (the difference panels too: x_draw has q rows per replicate fewer, and a workgroup of the
// forward kernel would write cells of x_draw that another one's difference panel still holds).
static int simsmooth_ar_check(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                              const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                              const double* mu0, const double* P0, const double* mean, const double* sd, const double* f_draw) {
    if (!h) return DFM_E_NULL;
    if (D < 1) return fail(h, DFM_E_DIMS, "D (draws per replicate) must be >= 1%s");
    if (!f_draw) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (int rc = forecast_ar_check(h, B, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, f_draw, f_draw)) return rc;
    if ((long long)B * D > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * D must be < 2^31%s");
    return 0;
}

// ll_all: [B D] device log-likelihoods of the difference panels (the host entry checks them), or null (h->ss, per slice)
static int simsmooth_ar_run(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                            const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                            const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                            uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, double* ll_all, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int m = state_lags(p, q);
    const size_t d = sizeof(double), k = (size_t)r * m, TH = (size_t)T + H, n = TH - q;
    const long long BD = (long long)B * D;
    const size_t per = forecast_ar_msg_bytes((int)n, N, q);
    size_t Sl = h->opt.fcar_msg_cap / per;
    if (Sl > (size_t)kSsSlice) Sl = kSsSlice;
    if (Sl < 1) Sl = 1;
    const int Smax = (int)(BD < (long long)Sl ? BD : (long long)Sl);
    size_t off = 0;
    const size_t o_LP0 = take(off, (size_t)B * k * k * d), o_LQ = take(off, (size_t)B * r * r * d),
                 o_Ap = p < m ? take(off, (size_t)B * r * k * d) : (size_t)-1;
    const SliceParams sp(off, Smax, N, r, k, q);
    const size_t o_g = take(off, (size_t)Smax * n * r * d),
                 o_ll = ll_all ? (size_t)-1 : take(off, (size_t)Smax * d), o_x = take(off, (size_t)Smax * TH * N * d),
                 o_msg = x_draw ? take(off, (size_t)Smax * per) : (size_t)-1,
                 o_last = x_draw ? take(off, (size_t)Smax * N * sizeof(int)) : (size_t)-1;
    HIP_TRY(h, h->ss.grow(off));
    const double* Am;
    if (int rc = pad_avar(h, B, r, p, m, Avar, at<double>(h->ss, o_Ap), &Am)) return rc;
    // the factor side: the plain model's kernels on m lags and n rows
    SsArgs a{};
    a.B = B; a.D = D; a.T = (int)n; a.N = N; a.r = r; a.p = m; a.H = 0;
    a.Lam = Lam; a.R = sig2; a.A = Am; a.Q = Q; a.mu0 = mu0; a.P0 = P0;
    a.seed = seed; a.first_draw = first_draw; a.f_draw = f_draw;
    a.LP0 = at<double>(h->ss, o_LP0); a.LQ = at<double>(h->ss, o_LQ);
    double* erho = sp.point(h->ss, a);
    double* g = at<double>(h->ss, o_g);
    double* diff = at<double>(h->ss, o_x);
    // the series side: the generator and the assembling forward kernel read the caller's parameters, the backward kernel the slice's
    SsArArgs gen{};
    gen.n = (int)n; gen.N = N; gen.r = r; gen.q = q;
    gen.Lam = Lam; gen.sig2 = sig2; gen.rho = rho; gen.v0 = v0; gen.mean = mean; gen.sd = sd;
    gen.f = g; gen.msg = at<double>(h->ss, o_msg); gen.last = at<int>(h->ss, o_last);
    gen.dr.D = D; gen.dr.T = T; gen.dr.k = (int)k; gen.dr.seed = seed; gen.dr.first_draw = first_draw;
    gen.dr.X = panel; gen.dr.fplus = f_draw; gen.dr.mu0 = mu0; gen.dr.LP0 = a.LP0; gen.dr.diff = diff; gen.dr.x_draw = x_draw;
    gen.dr.check_nan = (flags & DFM_F_MAY_HAVE_MISSING) ? 0 : 1; gen.dr.status = h->status_dev;
    FcArArgs back{};
    back.n = (int)n; back.N = N; back.r = r; back.q = q;
    back.panel = diff; back.f = g; back.Lam = a.eLam; back.sig2 = a.eR; back.rho = erho;
    back.msg = gen.msg; back.last = gen.last;
    HIP_LAUNCH(h, K_SS_PREP, launch_simsmooth_prep(a, h->stream));
    for (long long j0 = 0; j0 < BD; j0 += Smax) {
        const int S = (int)(BD - j0 < Smax ? BD - j0 : Smax);
        a.j0 = j0; a.S = S;
        gen.dr.j0 = j0; gen.S = S; back.b0 = 0; back.S = S;
        double* ll = ll_all ? ll_all + j0 : at<double>(h->ss, o_ll);
        HIP_LAUNCH(h, K_SS_EXPAND, launch_simsmooth_expand(a, h->stream));
        HIP_LAUNCH(h, K_SSAR_EXPAND, launch_simsmooth_ar_expand(S, j0, D, (size_t)N * q, rho, erho, h->stream));
        HIP_LAUNCH(h, K_SS_PATH, launch_simsmooth_path(a, h->stream));
        HIP_LAUNCH(h, K_SSAR_DIFF, launch_simsmooth_ar_diff(gen, h->stream));
        if (int rc = ar_pass_run(h, S, (int)TH, N, r, m, q, diff, a.eLam, a.eR, erho, a.eA, a.eQ, a.emu0, a.eP0, g, nullptr, ll,
                                 flags | DFM_F_MAY_HAVE_MISSING)) return rc;
        if (x_draw) {
            HIP_LAUNCH(h, K_FCAR_BACK, launch_forecast_ar_back(back, h->stream));
            HIP_LAUNCH(h, K_SSAR_FWD, launch_simsmooth_ar_fwd(gen, h->stream));
        }
        HIP_LAUNCH(h, K_SSAR_FINISH, launch_simsmooth_ar_finish((size_t)S * n * r, g, f_draw + (size_t)j0 * n * r, h->stream));
    }
    return 0;
}

int dfm_simsmooth_ar_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                               const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                               const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                               uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags) {
    if (int rc = simsmooth_ar_check(h, B, D, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, f_draw)) return rc;
    return simsmooth_ar_run(h, B, D, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd, seed, first_draw, f_draw,
                            x_draw, nullptr, flags);
}

int dfm_simsmooth_ar_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                           const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                           const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                           uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags) {
    if (int rc = simsmooth_ar_check(h, B, D, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, f_draw)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)T + H - q, BD = (size_t)B * D;
    std::vector<double> ll_host(BD);
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *f_d, *xo_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d);
    stage_model(st, md, B, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd);
    st.out(f_draw, BD * n * r, f_d); st.out(x_draw, x_draw ? BD * n * N : 0, xo_d); st.out(ll_host.data(), BD, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(simsmooth_ar_run(h, B, D, T, N, r, p, q, H, x_d, md.Lam, md.R, md.rho, md.A, md.Q, md.mu0, md.P0, md.v0, md.mean, md.sd,
                                        seed, first_draw, f_d, xo_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), (int)BD);
    return rc;
}

// ---- panels simulated from a given model (simulate.hip) -----------------------------------------------------------------------
// x+ of the two smoothers above, written out: the roots once, then per slice of at most kSsSlice pass replicates j = b D + d the
// factor path f+ (simsmooth_path_kernel, into f_sim or h->ss) and the cells.  No pass runs: no N limit of the pass applies.
static int simulate_check(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* Lam, const double* R,
                          const double* rho, const double* Avar, const double* Q, const double* mu0, const double* P0,
                          const double* x_sim) {
    if (!h) return DFM_E_NULL;
    if (B < 1 || T < 1 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, T, N, r must be >= 1%s");
    if (D < 1) return fail(h, DFM_E_DIMS, "D (draws per replicate) must be >= 1%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (q < 0 || q > 4) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be 1 .. 4%s");
    if ((long long)r * (q ? state_lags(p, q) : p) > DFM_MAX_R)
        return fail(h, DFM_E_DIMS, "state wider than DFM_MAX_R (32): r p, or r max(p, q + 1) with AR idiosyncratic terms%s");
    if (T < p) return fail(h, DFM_E_DIMS, "T must be >= p%s");
    if (T <= q) return fail(h, DFM_E_DIMS, "T must exceed the number of idiosyncratic lags%s");
    if ((long long)B * D > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * D must be < 2^31%s");
    if (!Lam || !R || (q && !rho) || !Avar || !Q || !mu0 || !P0 || !x_sim) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return 0;
}

// q = 0: the plain model (R, mask = the mask panel); q > 0: AR idiosyncratic terms (R = sig2, mask = the panel).
static int simulate_run(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* mask, const double* Lam,
                        const double* R, const double* rho, const double* Avar, const double* Q, const double* mu0,
                        const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int m = q ? state_lags(p, q) : p;
    const size_t d = sizeof(double), k = (size_t)r * m, n = (size_t)T - q;
    const long long BD = (long long)B * D;
    const int Smax = (int)(BD < kSsSlice ? BD : kSsSlice);
    size_t off = 0;
    const size_t o_LP0 = take(off, (size_t)B * k * k * d), o_LQ = take(off, (size_t)B * r * r * d),
                 o_Ap = p < m ? take(off, (size_t)B * r * k * d) : (size_t)-1,
                 o_f = f_sim ? (size_t)-1 : take(off, (size_t)BD * n * r * d);
    HIP_TRY(h, h->ss.grow(off));
    const double* Am;
    if (int rc = pad_avar(h, B, r, p, m, Avar, at<double>(h->ss, o_Ap), &Am)) return rc;
    SsArgs a{};
    a.B = B; a.D = D; a.T = (int)n; a.N = N; a.r = r; a.p = m; a.H = 0;
    a.panel = mask; a.Lam = Lam; a.R = R; a.A = Am; a.Q = Q; a.mu0 = mu0; a.P0 = P0;
    a.seed = seed; a.first_draw = first_draw; a.f_draw = f_sim ? f_sim : at<double>(h->ss, o_f); a.x_draw = x_sim;
    a.LP0 = at<double>(h->ss, o_LP0); a.LQ = at<double>(h->ss, o_LQ);
    SsArArgs gen{};
    gen.n = (int)n; gen.N = N; gen.r = r; gen.q = q;
    gen.Lam = Lam; gen.sig2 = R; gen.rho = rho; gen.v0 = v0;
    gen.dr.D = D; gen.dr.T = T; gen.dr.k = (int)k; gen.dr.seed = seed; gen.dr.first_draw = first_draw;
    gen.dr.X = mask; gen.dr.fplus = a.f_draw; gen.dr.mu0 = mu0; gen.dr.LP0 = a.LP0; gen.dr.x_draw = x_sim;
    HIP_LAUNCH(h, K_SS_PREP, launch_simsmooth_prep(a, h->stream));
    for (long long j0 = 0; j0 < BD; j0 += Smax) {
        const int S = (int)(BD - j0 < Smax ? BD - j0 : Smax);
        a.j0 = j0; a.S = S; gen.dr.j0 = j0; gen.S = S;
        HIP_LAUNCH(h, K_SS_PATH, launch_simsmooth_path(a, h->stream));
        if (q) HIP_LAUNCH(h, K_SIMAR_CELLS, launch_simulate_ar_cells(gen, h->stream));
        else HIP_LAUNCH(h, K_SIM_CELLS, launch_simulate_cells(a, h->stream));
    }
    return 0;
}

static int simulate_host(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* mask, const double* Lam,
                         const double* R, const double* rho, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim) {
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t BD = (size_t)B * D;
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *xo_d, *f_d;
    st.in(mask, mask ? (size_t)B * T * N : 0, x_d);
    stage_model(st, md, B, N, r, p, q, Lam, R, rho, Avar, Q, mu0, P0, v0, nullptr, nullptr);
    st.out(x_sim, BD * T * N, xo_d); st.out(f_sim, f_sim ? BD * (size_t)(T - q) * r : 0, f_d);
    if (int rc = st.begin()) return rc;
    return st.finish(simulate_run(h, B, D, T, N, r, p, q, x_d, md.Lam, md.R, md.rho, md.A, md.Q, md.mu0, md.P0, md.v0, seed, first_draw,
                                  xo_d, f_d));
}

int dfm_simulate_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, const double* mask_panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, uint64_t seed,
                           int64_t first_draw, double* x_sim, double* f_sim, unsigned flags) {
    (void)flags;
    if (int rc = simulate_check(h, B, D, T, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, x_sim)) return rc;
    return simulate_run(h, B, D, T, N, r, p, 0, mask_panel, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, seed, first_draw, x_sim, f_sim);
}

int dfm_simulate_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, const double* mask_panel, const double* Lam,
                       const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, uint64_t seed,
                       int64_t first_draw, double* x_sim, double* f_sim, unsigned flags) {
    (void)flags;
    if (int rc = simulate_check(h, B, D, T, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, x_sim)) return rc;
    return simulate_host(h, B, D, T, N, r, p, 0, mask_panel, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, seed, first_draw, x_sim, f_sim);
}

int dfm_simulate_ar_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                              const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                              const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim,
                              unsigned flags) {
    (void)flags;
    if (h && q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be 1 .. 4%s");
    if (int rc = simulate_check(h, B, D, T, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, x_sim)) return rc;
    return simulate_run(h, B, D, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, seed, first_draw, x_sim, f_sim);
}

int dfm_simulate_ar_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                          const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                          const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim,
                          unsigned flags) {
    (void)flags;
    if (h && q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be 1 .. 4%s");
    if (int rc = simulate_check(h, B, D, T, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, x_sim)) return rc;
    return simulate_host(h, B, D, T, N, r, p, q, panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, seed, first_draw, x_sim, f_sim);
}

// ---- rolling-window out-of-sample evaluation, re-estimated at every origin (rolling.hip) ---------------------------------------
// Per slice of at most kRwSlice windows: rolling_window_kernel (the standardised vintages and their statistics), the status word's
// window bit (read here: no EM on a thin or constant series), rolling_start_kernel, the EM entry of the plain or the VAR(p) model in
// place in the windows' parameters, dfm_forecast_batch_dev on the windows, rolling_score_kernel.  The slice's arrays live in h->rw
// (beside h->ws and h->fc, which the entries it calls size for themselves); what the caller takes is written at its slice offset.
constexpr int kRwSlice = 1024;

static int rolling_check(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start, const double* x,
                         const int* origins, const int* lags, const double* Lam_start, const double* R_start, const double* Avar_start,
                         const double* Q_start, const double* mu0_start, const double* P0_start, int max_iter, const double* Lam,
                         const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (T < 1 || N < 1 || r < 1 || p < 1 || O < 1) return fail(h, DFM_E_DIMS, "T, N, r, p, O must be >= 1%s");
    if ((long long)r * p > DFM_MAX_R) return fail(h, DFM_E_DIMS, "r * p > DFM_MAX_R (32)%s");
    if (W > T || W < 2 || W < p) return fail(h, DFM_E_DIMS, "need max(2, p) <= W <= T%s");
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (max_iter < 0) return fail(h, DFM_E_DIMS, "max_iter must be >= 0%s");
    if (min_obs < r + 1) return fail(h, DFM_E_DIMS, "min_obs must be >= r + 1%s");
    if (n_start != 1 && n_start != O) return fail(h, DFM_E_DIMS, "n_start must be 1 or O%s");
    if (!x || !origins || !Lam_start || !R_start || !Avar_start || !Q_start || !mu0_start || !P0_start)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (max_iter > 0 && (!Lam || !R || !Avar || !Q || !mu0 || !P0))
        return fail(h, DFM_E_NULL, "the windows' parameter arrays are required when max_iter > 0%s");
    for (int b = 0; b < O; ++b)
        if (origins[b] < W - 1 || origins[b] > T - 1 || (b && origins[b] <= origins[b - 1]))
            return fail(h, DFM_E_DIMS, "origins must increase and lie in W - 1 .. T - 1%s");
    bool lagged = false;
    for (int i = 0; lags && i < N; ++i) {
        if (lags[i] < 0 || lags[i] > W - min_obs) return fail(h, DFM_E_DIMS, "publication lags must lie in 0 .. W - min_obs%s");
        lagged = lagged || lags[i] > 0;
    }
    if (lagged && !(flags & DFM_F_MAY_HAVE_MISSING))
        return fail(h, DFM_E_MISSING, "publication lags leave NaN in the windows: DFM_F_MAY_HAVE_MISSING is needed%s");
    return 0;
}

static int rolling_run(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start, const double* x,
                       const int* origins, const int* lags, const double* Lam_start, const double* R_start, const double* Avar_start,
                       const double* Q_start, const double* mu0_start, const double* P0_start, const double* sd_start, int max_iter,
                       double tol, double* Lam, double* R, double* Avar, double* Q, double* mu0, double* P0, double* loglik_path,
                       int* iters, double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                       double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), k = (size_t)r * p, H1 = (size_t)H + 1, TH = (size_t)W + H;
    const size_t Smax = O < kRwSlice ? O : kRwSlice, SN = Smax * N;
    size_t off = 0;
    // an output the caller does not take has the slice's part here; (size_t)-1: the caller's array, at its slice offset
    auto own = [&](const void* callers, size_t bytes) { return callers ? (size_t)-1 : take(off, bytes); };
    const size_t o_org = take(off, (size_t)O * sizeof(int)), o_lag = lags ? take(off, (size_t)N * sizeof(int)) : (size_t)-1,
                 o_sse = take(off, H1 * N * d), o_sse0 = take(off, H1 * N * d), o_cnt = take(off, H1 * N * sizeof(int)),
                 o_win = own(windows, Smax * W * N * d), o_xh = take(off, Smax * TH * N * d), o_xv = take(off, Smax * TH * N * d),
                 o_f = take(off, Smax * TH * r * d), o_ll = take(off, Smax * d),
                 o_L = own(Lam, SN * r * d), o_R = own(R, SN * d), o_A = own(Avar, Smax * r * k * d), o_Q = own(Q, Smax * r * r * d),
                 o_m = own(mu0, Smax * k * d), o_P = own(P0, Smax * k * k * d),
                 o_path = max_iter ? own(loglik_path, Smax * max_iter * d) : (size_t)-1, o_it = own(iters, Smax * sizeof(int)),
                 o_mean = own(win_mean, SN * d), o_sd = own(win_sd, SN * d), o_nobs = own(win_nobs, SN * sizeof(int));
    HIP_TRY(h, h->rw.grow(off));
    int* org_d = at<int>(h->rw, o_org);
    HIP_TRY(h, hipMemcpyAsync(org_d, origins, (size_t)O * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (lags) HIP_TRY(h, hipMemcpyAsync(at<int>(h->rw, o_lag), lags, (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    RwArgs a{};
    a.T = T; a.N = N; a.W = W; a.H = H; a.r = r; a.k = (int)k; a.min_obs = min_obs;
    a.x = x; a.origins = org_d; a.lags = at<int>(h->rw, o_lag); a.status = h->status_dev;
    a.n_start = n_start; a.sLam = Lam_start; a.sR = R_start; a.sA = Avar_start; a.sQ = Q_start; a.smu0 = mu0_start; a.sP0 = P0_start;
    a.sd_start = sd_start;
    a.xhat = at<double>(h->rw, o_xh); a.xvar = at<double>(h->rw, o_xv);
    a.sse = at<double>(h->rw, o_sse); a.sse0 = at<double>(h->rw, o_sse0); a.cnt = at<int>(h->rw, o_cnt);
    a.msfe = msfe; a.msfe0 = msfe0; a.cnt_out = cnt;
    double *xhat = at<double>(h->rw, o_xh), *xvar = at<double>(h->rw, o_xv), *fbuf = at<double>(h->rw, o_f), *llbuf = at<double>(h->rw, o_ll);
    for (int b0 = 0; b0 < O; b0 += kRwSlice) {
        const int S = O - b0 < kRwSlice ? O - b0 : kRwSlice;
        // the slice's part of an [O][per] array: the caller's, or the block's
        auto part = [&](auto* callers, size_t o_own, size_t per) { return callers ? callers + (size_t)b0 * per : at<std::remove_pointer_t<decltype(callers)>>(h->rw, o_own); };
        a.b0 = b0; a.S = S; a.first = b0 == 0; a.last = b0 + S == O;
        a.win = part(windows, o_win, (size_t)W * N); a.mean = part(win_mean, o_mean, N); a.sd = part(win_sd, o_sd, N); a.nobs = part(win_nobs, o_nobs, N);
        a.Lam = part(Lam, o_L, (size_t)N * r); a.R = part(R, o_R, N); a.A = part(Avar, o_A, r * k); a.Q = part(Q, o_Q, (size_t)r * r);
        a.mu0 = part(mu0, o_m, k); a.P0 = part(P0, o_P, k * k);
        a.fc = fc ? fc + (size_t)b0 * H1 * N : nullptr; a.fvar = fvar ? fvar + (size_t)b0 * H1 * N : nullptr;
        a.err = err ? err + (size_t)b0 * H1 * N : nullptr; a.err_std = err_std ? err_std + (size_t)b0 * H1 * N : nullptr;
        int* it = part(iters, o_it, 1);
        HIP_LAUNCH(h, K_RW_WINDOW, launch_rolling_window(a, h->stream));
        int st = 0;                                            // a thin or constant series: stop before the EM meets its window
        HIP_TRY(h, hipMemcpyAsync(&st, h->status_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (st & kRwWindowBit) return status_check(h);
        HIP_LAUNCH(h, K_RW_START, launch_rolling_start(a, h->stream));
        if (max_iter > 0) {
            double* path = part(loglik_path, o_path, (size_t)max_iter);
            if (int rc = p == 1 ? dfm_em_batch_dev(h, S, W, N, r, a.win, a.Lam, a.R, a.A, a.Q, a.mu0, a.P0, max_iter, tol, path, it, nullptr,
                                                   nullptr, flags)
                                : dfm_em_varp_batch_dev(h, S, W, N, r, p, a.win, a.Lam, a.R, a.A, a.Q, a.mu0, a.P0, max_iter, tol, path, it,
                                                        nullptr, nullptr, flags)) return rc;
        } else {
            HIP_TRY(h, hipMemsetAsync(it, 0, (size_t)S * sizeof(int), h->stream));
        }
        if (int rc = dfm_forecast_batch_dev(h, S, W, N, r, p, H, a.win, a.Lam, a.R, a.A, a.Q, a.mu0, a.P0, a.mean, a.sd, xhat, xvar, nullptr,
                                            fbuf, nullptr, llbuf, flags)) return rc;
        HIP_LAUNCH(h, K_RW_SCORE, launch_rolling_score(a, h->stream));
    }
    return 0;
}

static int rolling_host(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start, const double* x,
                        const int* origins, const int* lags, const double* Lam_start, const double* R_start, const double* Avar_start,
                        const double* Q_start, const double* mu0_start, const double* P0_start, const double* sd_start, int max_iter,
                        double tol, double* Lam, double* R, double* Avar, double* Q, double* mu0, double* P0, double* loglik_path,
                        int* iters, double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                        double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, nO = (size_t)O, ON = nO * N, n_fc = nO * (H + 1) * N, n_ms = (size_t)(H + 1) * N;
    HostStage st(h, 256);
    ModelDev sm, wm;
    double *x_d, *sds_d, *path_d, *win_d, *fc_d, *fv_d, *er_d, *es_d, *ms_d, *m0_d;
    int *it_d, *nobs_d, *cnt_d;
    st.in(x, (size_t)T * N, x_d);
    stage_model(st, sm, n_start, N, r, p, 0, Lam_start, R_start, nullptr, Avar_start, Q_start, mu0_start, P0_start, nullptr, nullptr, nullptr);
    st.in(sd_start, sd_start ? (size_t)N : 0, sds_d);
    // the windows' parameters and statistics: outputs only, each taking room only where the caller takes it
    wm = ModelDev{};
    st.out(Lam, Lam ? ON * r : 0, wm.Lam); st.out(R, R ? ON : 0, wm.R); st.out(Avar, Avar ? nO * r * k : 0, wm.A);
    st.out(Q, Q ? nO * r * r : 0, wm.Q); st.out(mu0, mu0 ? nO * k : 0, wm.mu0); st.out(P0, P0 ? nO * k * k : 0, wm.P0);
    st.out(loglik_path, loglik_path ? nO * max_iter : 0, path_d); st.out(iters, iters ? nO : 0, it_d);
    st.out(win_mean, win_mean ? ON : 0, wm.mean); st.out(win_sd, win_sd ? ON : 0, wm.sd); st.out(win_nobs, win_nobs ? ON : 0, nobs_d);
    st.out(windows, windows ? ON * W : 0, win_d);
    st.out(fc, fc ? n_fc : 0, fc_d); st.out(fvar, fvar ? n_fc : 0, fv_d); st.out(err, err ? n_fc : 0, er_d);
    st.out(err_std, err_std ? n_fc : 0, es_d); st.out(msfe, msfe ? n_ms : 0, ms_d); st.out(msfe0, msfe0 ? n_ms : 0, m0_d);
    st.out(cnt, cnt ? n_ms : 0, cnt_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(rolling_run(h, T, N, r, p, W, H, O, min_obs, n_start, x_d, origins, lags, sm.Lam, sm.R, sm.A, sm.Q, sm.mu0, sm.P0, sds_d,
                                   max_iter, tol, wm.Lam, wm.R, wm.A, wm.Q, wm.mu0, wm.P0, path_d, it_d, wm.mean, wm.sd, nobs_d, win_d, fc_d, fv_d,
                                   er_d, es_d, ms_d, m0_d, cnt_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}

int dfm_rolling_eval_batch_dev(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start,
                               const double* x, const int* origins, const int* lags, const double* Lam_start,
                               const double* R_start, const double* Avar_start, const double* Q_start, const double* mu0_start,
                               const double* P0_start, const double* sd_start, int max_iter, double tol, double* Lam, double* R,
                               double* Avar, double* Q, double* mu0, double* P0, double* loglik_path, int* iters,
                               double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                               double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = rolling_check(h, T, N, r, p, W, H, O, min_obs, n_start, x, origins, lags, Lam_start, R_start, Avar_start, Q_start, mu0_start,
                               P0_start, max_iter, Lam, R, Avar, Q, mu0, P0, flags)) return rc;
    return rolling_run(h, T, N, r, p, W, H, O, min_obs, n_start, x, origins, lags, Lam_start, R_start, Avar_start, Q_start, mu0_start, P0_start,
                       sd_start, max_iter, tol, Lam, R, Avar, Q, mu0, P0, loglik_path, iters, win_mean, win_sd, win_nobs, windows, fc, fvar, err,
                       err_std, msfe, msfe0, cnt, flags);
}

int dfm_rolling_eval_batch(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start,
                           const double* x, const int* origins, const int* lags, const double* Lam_start,
                           const double* R_start, const double* Avar_start, const double* Q_start, const double* mu0_start,
                           const double* P0_start, const double* sd_start, int max_iter, double tol, double* Lam, double* R,
                           double* Avar, double* Q, double* mu0, double* P0, double* loglik_path, int* iters,
                           double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                           double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = rolling_check(h, T, N, r, p, W, H, O, min_obs, n_start, x, origins, lags, Lam_start, R_start, Avar_start, Q_start, mu0_start,
                               P0_start, max_iter, Lam, R, Avar, Q, mu0, P0, flags)) return rc;
    return rolling_host(h, T, N, r, p, W, H, O, min_obs, n_start, x, origins, lags, Lam_start, R_start, Avar_start, Q_start, mu0_start, P0_start,
                        sd_start, max_iter, tol, Lam, R, Avar, Q, mu0, P0, loglik_path, iters, win_mean, win_sd, win_nobs, windows, fc, fvar, err,
                        err_std, msfe, msfe0, cnt, flags);
}

// ---- diffusion-index forecasts from the non-parametric fit, out of sample (diffusion.hip) --------------------------------------
// Per slice of at most kRwSlice windows: rolling_window_kernel and the status word's window bit as above, di_start_kernel (the start
// factors), als_kernel on the slice's windows (one workgroup per window; none when max_iter = 0), di_regress_kernel, di_score_kernel.
// The slice's arrays live in h->rw, as the rolling driver's do.
static int diffusion_check(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int n_start, const double* x,
                           const int* origins, const int* lags, const double* F_start, int max_iter, unsigned flags) {
    if (!h) return DFM_E_NULL;
    if (T < 1 || N < 1 || r < 1 || q < 0 || O < 1) return fail(h, DFM_E_DIMS, "T, N, r, O must be >= 1 and q >= 0%s");
    const long long K = 1ll + r + q;
    if (K > 32) return fail(h, DFM_E_DIMS, "1 + r + q > 32 regressors%s");
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (W > T || W < K + q + H + 2) return fail(h, DFM_E_DIMS, "need 1 + r + 2 q + H + 2 <= W <= T%s");
    if (max_iter < 0) return fail(h, DFM_E_DIMS, "max_iter must be >= 0%s");
    if (min_obs < r + 1) return fail(h, DFM_E_DIMS, "min_obs must be >= r + 1%s");
    if (n_start != 1 && n_start != O) return fail(h, DFM_E_DIMS, "n_start must be 1 or O%s");
    if (!x || !origins || !F_start) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    for (int b = 0; b < O; ++b)
        if (origins[b] < W - 1 || origins[b] > T - 1 || (b && origins[b] <= origins[b - 1]))
            return fail(h, DFM_E_DIMS, "origins must increase and lie in W - 1 .. T - 1%s");
    bool lagged = false, reaches = !lags;
    for (int i = 0; lags && i < N; ++i) {
        if (lags[i] < 0 || lags[i] > W - min_obs) return fail(h, DFM_E_DIMS, "publication lags must lie in 0 .. W - min_obs%s");
        lagged = lagged || lags[i] > 0;
        reaches = reaches || lags[i] == 0;
    }
    if (!reaches) return fail(h, DFM_E_DIMS, "no series reaches the origin (every publication lag > 0): its factor row has no data%s");
    if (!als_fits(pad_r(r), W, N)) return fail(h, DFM_E_DIMS, "(W + N) * pad(r) doubles exceed the 160 KB of LDS%s");
    if (!di_series_block(W, r, pad_r((int)K))) return fail(h, DFM_E_DIMS, "W * (r + 1) doubles and the regressions' exchange rows exceed the 160 KB of LDS%s");
    if (lagged && !(flags & DFM_F_MAY_HAVE_MISSING))
        return fail(h, DFM_E_MISSING, "publication lags leave NaN in the windows: DFM_F_MAY_HAVE_MISSING is needed%s");
    return 0;
}

static int diffusion_run(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int nt_min, int n_start,
                         const double* x, const int* origins, const int* lags, const double* F_start, int max_iter, double tol, double* F,
                         double* Lam, int* als_iters, double* als_ssr, double* win_mean, double* win_sd, int* win_nobs, double* windows,
                         double* fc, double* fc_ar, double* fvar, double* err, double* err_ar, double* err_std, double* beta,
                         int* nobs_reg, double* msfe, double* msfe_ar, double* msfe0, int* cnt, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), H1 = (size_t)H + 1, K = (size_t)1 + r + q;
    const size_t Smax = O < kRwSlice ? O : kRwSlice, SN = Smax * N;
    size_t off = 0;
    auto own = [&](const void* callers, size_t bytes) { return callers ? (size_t)-1 : take(off, bytes); };
    const size_t o_org = take(off, (size_t)O * sizeof(int)), o_lag = lags ? take(off, (size_t)N * sizeof(int)) : (size_t)-1,
                 o_sse = take(off, H1 * N * d), o_ssa = take(off, H1 * N * d), o_sse0 = take(off, H1 * N * d),
                 o_cnt = take(off, H1 * N * sizeof(int)), o_win = own(windows, Smax * W * N * d), o_F = own(F, Smax * W * r * d),
                 o_L = own(Lam, SN * r * d), o_it = own(als_iters, Smax * sizeof(int)), o_ssr = own(als_ssr, Smax * d),
                 o_mean = own(win_mean, SN * d), o_sd = own(win_sd, SN * d), o_nobs = own(win_nobs, SN * sizeof(int)),
                 o_fc = own(fc, SN * H1 * d), o_fa = own(fc_ar, SN * H1 * d), o_fv = own(fvar, SN * H1 * d);
    HIP_TRY(h, h->rw.grow(off));
    int* org_d = at<int>(h->rw, o_org);
    HIP_TRY(h, hipMemcpyAsync(org_d, origins, (size_t)O * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (lags) HIP_TRY(h, hipMemcpyAsync(at<int>(h->rw, o_lag), lags, (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    RwArgs w{};
    w.T = T; w.N = N; w.W = W; w.H = H; w.r = r; w.k = r; w.min_obs = min_obs;
    w.x = x; w.origins = org_d; w.lags = at<int>(h->rw, o_lag); w.status = h->status_dev;
    DiArgs a{};
    a.T = T; a.N = N; a.W = W; a.H = H; a.r = r; a.q = q; a.K = (int)K; a.nt_min = nt_min; a.n_start = n_start;
    a.missing_ok = (flags & DFM_F_MAY_HAVE_MISSING) != 0;
    a.x = x; a.origins = org_d; a.lags = w.lags; a.F_start = F_start; a.status = h->status_dev;
    a.sse = at<double>(h->rw, o_sse); a.sse_ar = at<double>(h->rw, o_ssa); a.sse0 = at<double>(h->rw, o_sse0); a.cnt = at<int>(h->rw, o_cnt);
    a.msfe = msfe; a.msfe_ar = msfe_ar; a.msfe0 = msfe0; a.cnt_out = cnt;
    const int Rp = pad_r(r), Rk = pad_r((int)K);
    a.nb = di_series_block(W, r, Rk);
    a.h_first = 1;
    for (int i = 0; lags && i < N; ++i) a.h_first = a.h_first && lags[i] == 0;
    for (int b0 = 0; b0 < O; b0 += kRwSlice) {
        const int S = O - b0 < kRwSlice ? O - b0 : kRwSlice;
        auto part = [&](auto* callers, size_t o_own, size_t per) { return callers ? callers + (size_t)b0 * per : at<std::remove_pointer_t<decltype(callers)>>(h->rw, o_own); };
        auto opt = [&](auto* callers, size_t per) { return callers ? callers + (size_t)b0 * per : nullptr; };
        w.b0 = b0; w.S = S;
        w.win = part(windows, o_win, (size_t)W * N); w.mean = part(win_mean, o_mean, N); w.sd = part(win_sd, o_sd, N); w.nobs = part(win_nobs, o_nobs, N);
        a.b0 = b0; a.S = S; a.first = b0 == 0; a.last = b0 + S == O;
        a.win = w.win; a.mean = w.mean; a.sd = w.sd; a.nobs = w.nobs;
        a.F = part(F, o_F, (size_t)W * r);
        a.fc = part(fc, o_fc, H1 * N); a.fc_ar = part(fc_ar, o_fa, H1 * N); a.fvar = part(fvar, o_fv, H1 * N);
        a.err = opt(err, H1 * N); a.err_ar = opt(err_ar, H1 * N); a.err_std = opt(err_std, H1 * N);
        a.beta = opt(beta, H1 * N * K); a.nobs_reg = opt(nobs_reg, H1 * N);
        double *lam = part(Lam, o_L, (size_t)N * r), *ssr = part(als_ssr, o_ssr, 1);
        int* it = part(als_iters, o_it, 1);
        HIP_LAUNCH(h, K_RW_WINDOW, launch_rolling_window(w, h->stream));
        int st = 0;                                            // a thin or constant series: stop before the ALS meets its window
        HIP_TRY(h, hipMemcpyAsync(&st, h->status_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (st & kRwWindowBit) return status_check(h);
        HIP_LAUNCH(h, K_DI_START, launch_di_start(a, h->stream));
        if (max_iter > 0) {
            AlsArgs al;
            memset(&al, 0, sizeof(al));
            al.B = S; al.T = W; al.N = N; al.rmax = r; al.z = a.win; al.z_stride = (long long)W * N; al.F = a.F; al.Lam = lam;
            al.nt_min = nt_min; al.max_iter = max_iter; al.tol = tol; al.iters = it; al.ssr = ssr;
            HIP_LAUNCH(h, K_ALS, launch_als(Rp, al, h->stream));
        } else {                                               // the factors are the start: no loadings, no sweeps (all-ones bytes: NaN)
            HIP_TRY(h, hipMemsetAsync(lam, 0xFF, (size_t)S * N * r * d, h->stream));
            HIP_TRY(h, hipMemsetAsync(ssr, 0xFF, (size_t)S * d, h->stream));
            HIP_TRY(h, hipMemsetAsync(it, 0, (size_t)S * sizeof(int), h->stream));
        }
        HIP_LAUNCH(h, K_DI_REGRESS, launch_di_regress(Rk, a, h->stream));
        HIP_LAUNCH(h, K_DI_SCORE, launch_di_score(a, h->stream));
    }
    return 0;
}

int dfm_diffusion_eval_batch_dev(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int nt_min, int n_start,
                                 const double* x, const int* origins, const int* lags, const double* F_start, int max_iter,
                                 double tol, double* F, double* Lam, int* als_iters, double* als_ssr, double* win_mean,
                                 double* win_sd, int* win_nobs, double* windows, double* fc, double* fc_ar, double* fvar, double* err,
                                 double* err_ar, double* err_std, double* beta, int* nobs_reg, double* msfe, double* msfe_ar,
                                 double* msfe0, int* cnt, unsigned flags) {
    if (int rc = diffusion_check(h, T, N, r, q, W, H, O, min_obs, n_start, x, origins, lags, F_start, max_iter, flags)) return rc;
    return diffusion_run(h, T, N, r, q, W, H, O, min_obs, nt_min, n_start, x, origins, lags, F_start, max_iter, tol, F, Lam, als_iters,
                         als_ssr, win_mean, win_sd, win_nobs, windows, fc, fc_ar, fvar, err, err_ar, err_std, beta, nobs_reg, msfe, msfe_ar,
                         msfe0, cnt, flags);
}

int dfm_diffusion_eval_batch(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int nt_min, int n_start,
                             const double* x, const int* origins, const int* lags, const double* F_start, int max_iter, double tol,
                             double* F, double* Lam, int* als_iters, double* als_ssr, double* win_mean, double* win_sd,
                             int* win_nobs, double* windows, double* fc, double* fc_ar, double* fvar, double* err, double* err_ar,
                             double* err_std, double* beta, int* nobs_reg, double* msfe, double* msfe_ar, double* msfe0, int* cnt,
                             unsigned flags) {
    if (int rc = diffusion_check(h, T, N, r, q, W, H, O, min_obs, n_start, x, origins, lags, F_start, max_iter, flags)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nO = (size_t)O, ON = nO * N, n_fc = nO * (H + 1) * N, n_ms = (size_t)(H + 1) * N, K = (size_t)1 + r + q;
    HostStage st(h, 256);
    double *x_d, *fs_d, *F_d, *L_d, *ssr_d, *mean_d, *sd_d, *win_d, *fc_d, *fa_d, *fv_d, *er_d, *ea_d, *es_d, *b_d, *ms_d, *ma_d, *m0_d;
    int *it_d, *nobs_d, *nr_d, *cnt_d;
    st.in(x, (size_t)T * N, x_d);
    st.in(F_start, n_start == 1 ? (size_t)T * r : nO * W * r, fs_d);
    // outputs only, each taking room only where the caller takes it
    st.out(F, F ? nO * W * r : 0, F_d); st.out(Lam, Lam ? ON * r : 0, L_d); st.out(als_iters, als_iters ? nO : 0, it_d);
    st.out(als_ssr, als_ssr ? nO : 0, ssr_d); st.out(win_mean, win_mean ? ON : 0, mean_d); st.out(win_sd, win_sd ? ON : 0, sd_d);
    st.out(win_nobs, win_nobs ? ON : 0, nobs_d); st.out(windows, windows ? ON * W : 0, win_d);
    st.out(fc, fc ? n_fc : 0, fc_d); st.out(fc_ar, fc_ar ? n_fc : 0, fa_d); st.out(fvar, fvar ? n_fc : 0, fv_d);
    st.out(err, err ? n_fc : 0, er_d); st.out(err_ar, err_ar ? n_fc : 0, ea_d); st.out(err_std, err_std ? n_fc : 0, es_d);
    st.out(beta, beta ? n_fc * K : 0, b_d); st.out(nobs_reg, nobs_reg ? n_fc : 0, nr_d);
    st.out(msfe, msfe ? n_ms : 0, ms_d); st.out(msfe_ar, msfe_ar ? n_ms : 0, ma_d); st.out(msfe0, msfe0 ? n_ms : 0, m0_d);
    st.out(cnt, cnt ? n_ms : 0, cnt_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(diffusion_run(h, T, N, r, q, W, H, O, min_obs, nt_min, n_start, x_d, origins, lags, fs_d, max_iter, tol, F_d, L_d, it_d,
                                     ssr_d, mean_d, sd_d, nobs_d, win_d, fc_d, fa_d, fv_d, er_d, ea_d, es_d, b_d, nr_d, ms_d, ma_d, m0_d,
                                     cnt_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}

// ---- Bayesian estimation: the Gibbs sampler (gibbs.hip)------------------------------------------------------------------------
// Sweep j: the factor path of every chain by dfm_simsmooth_batch_dev (D = 1, H = 0, first_draw = first_sweep + j) into h->gb, then
// lam_i, R_i | f and A, Q | f in place in the caller's state.  Nothing waits between the sweeps; kept sweeps are copied behind the
// sweep in stream order.
static int gibbs_kept(int n_sweeps, int burn, int thin) { return n_sweeps > burn ? (n_sweeps - burn + thin - 1) / thin : 0; }

static int gibbs_check(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* mu0, const double* P0,
                       const double* Lam, const double* R, const double* Avar, const double* Q, double tau_lam, double nu_R,
                       double s_R, double tau_A, double nu_Q, double s_Q, int n_sweeps, int burn, int thin) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (T <= p) return fail(h, DFM_E_DIMS, "T must be > p (the VAR block conditions on the first p drawn rows)%s");
    if (n_sweeps < 1 || thin < 1 || burn < 0) return fail(h, DFM_E_DIMS, "n_sweeps >= 1, thin >= 1 and burn >= 0 are required%s");
    if (!(tau_lam > 0.0) || !(nu_R >= 2.0) || !(s_R > 0.0) || !(tau_A > 0.0) || !(nu_Q >= (double)r + 1.0) || !(s_Q > 0.0))
        return fail(h, DFM_E_DIMS, "prior: tau_lam, s_R, tau_A, s_Q > 0, nu_R >= 2 and nu_Q >= r + 1 are required%s");
    if (!panel || !mu0 || !P0 || !Lam || !R || !Avar || !Q) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return 0;
}

int dfm_gibbs_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* mu0, const double* P0,
                        double* Lam, double* R, double* Avar, double* Q, double tau_lam, double nu_R, double s_R, double tau_A,
                        double nu_Q, double s_Q, const double* A0, int n_sweeps, int burn, int thin, uint64_t seed,
                        int64_t first_sweep, double* Lam_draw, double* R_draw, double* A_draw, double* Q_draw, double* f_draw,
                        unsigned flags) {
    if (int rc = gibbs_check(h, B, T, N, r, p, panel, mu0, P0, Lam, R, Avar, Q, tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q, n_sweeps, burn,
                             thin)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), k = (size_t)r * p;
    const bool missing = (flags & DFM_F_MAY_HAVE_MISSING) != 0;
    size_t off = 0;
    const size_t o_f = take(off, (size_t)B * T * r * d), o_L = missing ? (size_t)-1 : take(off, (size_t)B * r * r * d);
    HIP_TRY(h, h->gb.grow(off));
    GbArgs a{};
    a.B = B; a.T = T; a.N = N; a.r = r; a.p = p;
    a.panel = panel; a.f = at<double>(h->gb, o_f); a.Lam = Lam; a.R = R; a.A = Avar; a.Q = Q; a.A0 = A0;
    a.tau_lam = tau_lam; a.nu_R = nu_R; a.s_R = s_R; a.tau_A = tau_A; a.nu_Q = nu_Q; a.s_Q = s_Q;
    a.seed = seed; a.missing = missing; a.Lsh = at<double>(h->gb, o_L); a.status = h->status_dev;
    double* f = at<double>(h->gb, o_f);
    const size_t K = (size_t)gibbs_kept(n_sweeps, burn, thin);
    for (int j = 0; j < n_sweeps; ++j) {
        a.sweep = first_sweep + j;
        if (int rc = dfm_simsmooth_batch_dev(h, B, 1, T, N, r, p, 0, panel, Lam, R, Avar, Q, mu0, P0, nullptr, nullptr, seed, a.sweep, f,
                                             nullptr, flags)) return rc;
        if (!missing) HIP_LAUNCH(h, K_GB_GRAM, launch_gibbs_gram(a, h->stream));
        HIP_LAUNCH(h, K_GB_LOAD, launch_gibbs_load(a, h->stream));
        HIP_LAUNCH(h, K_GB_VAR, launch_gibbs_var(a, h->stream));
        if (gibbs_kept_slot(j, burn, thin)) {
            const size_t kk = (size_t)(j - burn) / thin;
            HIP_TRY(h, gibbs_keep(h, Lam_draw, Lam, (size_t)N * r, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, R_draw, R, (size_t)N, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, A_draw, Avar, (size_t)r * k, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, Q_draw, Q, (size_t)r * r, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, f_draw, f, (size_t)T * r, kk, K, B));
        }
    }
    return 0;
}

int dfm_gibbs_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* mu0, const double* P0,
                    double* Lam, double* R, double* Avar, double* Q, double tau_lam, double nu_R, double s_R, double tau_A,
                    double nu_Q, double s_Q, const double* A0, int n_sweeps, int burn, int thin, uint64_t seed, int64_t first_sweep,
                    double* Lam_draw, double* R_draw, double* A_draw, double* Q_draw, double* f_draw, unsigned flags) {
    if (int rc = gibbs_check(h, B, T, N, r, p, panel, mu0, P0, Lam, R, Avar, Q, tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q, n_sweeps, burn,
                             thin)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, BK = (size_t)B * gibbs_kept(n_sweeps, burn, thin);
    HostStage st(h, 256);
    double *x_d, *mu_d, *P0_d, *lam_d, *R_d, *A_d, *Q_d, *A0_d, *ld_d, *rd_d, *ad_d, *qd_d, *fd_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(mu0, (size_t)B * k, mu_d); st.in(P0, (size_t)B * k * k, P0_d);
    st.inout(Lam, (size_t)B * N * r, lam_d); st.inout(R, (size_t)B * N, R_d); st.inout(Avar, (size_t)B * r * k, A_d);
    st.inout(Q, (size_t)B * r * r, Q_d); st.in(A0, A0 ? (size_t)B * r * k : 0, A0_d);
    st.out(Lam_draw, Lam_draw ? BK * N * r : 0, ld_d); st.out(R_draw, R_draw ? BK * N : 0, rd_d);
    st.out(A_draw, A_draw ? BK * r * k : 0, ad_d); st.out(Q_draw, Q_draw ? BK * r * r : 0, qd_d);
    st.out(f_draw, f_draw ? BK * T * r : 0, fd_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_gibbs_batch_dev(h, B, T, N, r, p, x_d, mu_d, P0_d, lam_d, R_d, A_d, Q_d, tau_lam, nu_R, s_R, tau_A, nu_Q, s_Q,
                                           A0_d, n_sweeps, burn, thin, seed, first_sweep, ld_d, rd_d, ad_d, qd_d, fd_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}


// ---- Bayesian estimation with AR idiosyncratic terms (gibbs_ar.hip) -----------------------------------------------------------
// Sweep j: the factor path of every chain by dfm_simsmooth_ar_batch_dev (D = 1, H = 0, v0 / mean / sd / x_draw NULL, first_draw =
// first_sweep + j) into h->gb, then rho_i, sig2_i, lam_i | f (gibbs_ar_series_kernel) and A, Q | f (gibbs_var_kernel on the n = T - q
// rows of the path) in place in the caller's state.  Nothing waits between the sweeps; kept sweeps are copied behind the sweep.
static int gibbs_ar_check(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* mu0,
                          const double* P0, const double* Lam, const double* sig2, const double* rho, const double* Avar,
                          const double* Q, double tau_lam, double nu_R, double s_R, double tau_rho, double tau_A, double nu_Q,
                          double s_Q, int n_sweeps, int burn, int thin) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be >= 1 (q = 0 is dfm_gibbs_batch)%s");
    if (n_sweeps < 1 || thin < 1 || burn < 0) return fail(h, DFM_E_DIMS, "n_sweeps >= 1, thin >= 1 and burn >= 0 are required%s");
    if (!(tau_lam > 0.0) || !(nu_R >= 2.0) || !(s_R > 0.0) || !(tau_rho > 0.0) || !(tau_A > 0.0) || !(nu_Q >= (double)r + 1.0) ||
        !(s_Q > 0.0))
        return fail(h, DFM_E_DIMS, "prior: tau_lam, s_R, tau_rho, tau_A, s_Q > 0, nu_R >= 2 and nu_Q >= r + 1 are required%s");
    const int m = state_lags(p, q);
    if (q > 4 || r > 8 || (long long)r * m > DFM_MAX_R)
        return fail(h, DFM_E_R_UNSUPPORTED, "the Gibbs sampler with AR idiosyncratic terms needs q <= 4, r <= 8 and r max(p, q + 1) <= 32%s");
    if ((long long)T - q <= p) return fail(h, DFM_E_DIMS, "T - q must be > p (the VAR block conditions on the first p drawn rows)%s");
    if (!panel || !mu0 || !P0 || !Lam || !sig2 || !rho || !Avar || !Q) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return 0;
}

int dfm_gibbs_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* mu0,
                           const double* P0, double* Lam, double* sig2, double* rho, double* Avar, double* Q, double tau_lam,
                           double nu_R, double s_R, double tau_rho, double tau_A, double nu_Q, double s_Q, const double* A0,
                           int n_sweeps, int burn, int thin, uint64_t seed, int64_t first_sweep, double* Lam_draw,
                           double* sig2_draw, double* rho_draw, double* A_draw, double* Q_draw, double* f_draw, unsigned flags) {
    if (int rc = gibbs_ar_check(h, B, T, N, r, p, q, panel, mu0, P0, Lam, sig2, rho, Avar, Q, tau_lam, nu_R, s_R, tau_rho, tau_A, nu_Q,
                                s_Q, n_sweeps, burn, thin)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), k = (size_t)r * p, n = (size_t)T - q;
    HIP_TRY(h, h->gb.grow((size_t)B * n * r * d));
    double* f = at<double>(h->gb, 0);
    GbArArgs sa{};
    sa.B = B; sa.n = (int)n; sa.N = N; sa.r = r; sa.q = q;
    sa.panel = panel; sa.f = f; sa.Lam = Lam; sa.sig2 = sig2; sa.rho = rho;
    sa.tau_lam = tau_lam; sa.nu_R = nu_R; sa.s_R = s_R; sa.tau_rho = tau_rho; sa.seed = seed; sa.status = h->status_dev;
    GbArgs a{};                                             // gibbs_var_kernel on the path's n rows
    a.B = B; a.T = (int)n; a.N = N; a.r = r; a.p = p;
    a.f = f; a.A = Avar; a.Q = Q; a.A0 = A0; a.tau_A = tau_A; a.nu_Q = nu_Q; a.s_Q = s_Q; a.seed = seed; a.status = h->status_dev;
    const size_t K = (size_t)gibbs_kept(n_sweeps, burn, thin);
    for (int j = 0; j < n_sweeps; ++j) {
        a.sweep = sa.sweep = first_sweep + j;
        if (int rc = dfm_simsmooth_ar_batch_dev(h, B, 1, T, N, r, p, q, 0, panel, Lam, sig2, rho, Avar, Q, mu0, P0, nullptr, nullptr,
                                                nullptr, seed, a.sweep, f, nullptr, flags)) return rc;
        HIP_LAUNCH(h, K_GB_AR_SERIES, launch_gibbs_ar_series(sa, h->stream));
        HIP_LAUNCH(h, K_GB_VAR, launch_gibbs_var(a, h->stream));
        if (gibbs_kept_slot(j, burn, thin)) {
            const size_t kk = (size_t)(j - burn) / thin;
            HIP_TRY(h, gibbs_keep(h, Lam_draw, Lam, (size_t)N * r, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, sig2_draw, sig2, (size_t)N, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, rho_draw, rho, (size_t)N * q, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, A_draw, Avar, (size_t)r * k, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, Q_draw, Q, (size_t)r * r, kk, K, B));
            HIP_TRY(h, gibbs_keep(h, f_draw, f, n * r, kk, K, B));
        }
    }
    return 0;
}

int dfm_gibbs_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* mu0,
                       const double* P0, double* Lam, double* sig2, double* rho, double* Avar, double* Q, double tau_lam, double nu_R,
                       double s_R, double tau_rho, double tau_A, double nu_Q, double s_Q, const double* A0, int n_sweeps, int burn,
                       int thin, uint64_t seed, int64_t first_sweep, double* Lam_draw, double* sig2_draw, double* rho_draw,
                       double* A_draw, double* Q_draw, double* f_draw, unsigned flags) {
    if (int rc = gibbs_ar_check(h, B, T, N, r, p, q, panel, mu0, P0, Lam, sig2, rho, Avar, Q, tau_lam, nu_R, s_R, tau_rho, tau_A, nu_Q,
                                s_Q, n_sweeps, burn, thin)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t m = (size_t)state_lags(p, q), km = (size_t)r * m, k = (size_t)r * p, n = (size_t)T - q,
                 BK = (size_t)B * gibbs_kept(n_sweeps, burn, thin);
    HostStage st(h, 256);
    double *x_d, *mu_d, *P0_d, *lam_d, *s2_d, *rho_d, *A_d, *Q_d, *A0_d, *ld_d, *sd_d, *rd_d, *ad_d, *qd_d, *fd_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(mu0, (size_t)B * km, mu_d); st.in(P0, (size_t)B * km * km, P0_d);
    st.inout(Lam, (size_t)B * N * r, lam_d); st.inout(sig2, (size_t)B * N, s2_d); st.inout(rho, (size_t)B * N * q, rho_d);
    st.inout(Avar, (size_t)B * r * k, A_d); st.inout(Q, (size_t)B * r * r, Q_d); st.in(A0, A0 ? (size_t)B * r * k : 0, A0_d);
    st.out(Lam_draw, Lam_draw ? BK * N * r : 0, ld_d); st.out(sig2_draw, sig2_draw ? BK * N : 0, sd_d);
    st.out(rho_draw, rho_draw ? BK * N * q : 0, rd_d); st.out(A_draw, A_draw ? BK * r * k : 0, ad_d);
    st.out(Q_draw, Q_draw ? BK * r * r : 0, qd_d); st.out(f_draw, f_draw ? BK * n * r : 0, fd_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_gibbs_ar_batch_dev(h, B, T, N, r, p, q, x_d, mu_d, P0_d, lam_d, s2_d, rho_d, A_d, Q_d, tau_lam, nu_R, s_R, tau_rho,
                                              tau_A, nu_Q, s_Q, A0_d, n_sweeps, burn, thin, seed, first_sweep, ld_d, sd_d, rd_d, ad_d, qd_d,
                                              fd_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}


// ---- structural IRFs, variance and historical decompositions (structural.hip) ------------------------------------------------
// Sizes first (they are decided before the handle is looked at), then the handle and the required pointers.
static int sv_check(dfm_handle* h, int B, int T, int N, int r, int p, const int* named, unsigned flags) {
    if (B < 1 || T < 1 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, T, N, r must be >= 1%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r > DFM_MAX_R || (long long)r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (named)
        for (int a = 0; a < r; ++a) {
            if (named[a] < 0 || named[a] >= N) return fail(h, DFM_E_DIMS, "a named series lies outside [0, N)%s");
            for (int c = 0; c < a; ++c)
                if (named[c] == named[a]) return fail(h, DFM_E_DIMS, "a named series is repeated%s");
        }
    if (!h) return DFM_E_NULL;
    if ((flags & DFM_SV_UNIT_EFFECT) && !named) return fail(h, DFM_E_NULL, "DFM_SV_UNIT_EFFECT needs named series%s");
    return 0;
}

// named [r] and cum [N] as device ints at the start of h->sv (offsets o_named, o_cum; (size_t)-1: not given)
static int sv_upload_idx(dfm_handle* h, int r, int N, const int* named, const int* cum, size_t o_named, size_t o_cum) {
    h->sv_idx.clear();
    if (named) h->sv_idx.insert(h->sv_idx.end(), named, named + r);
    if (cum) h->sv_idx.insert(h->sv_idx.end(), cum, cum + N);
    const int* src = h->sv_idx.data();
    if (named) HIP_TRY(h, hipMemcpyAsync(at<int>(h->sv, o_named), src, (size_t)r * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (cum) HIP_TRY(h, hipMemcpyAsync(at<int>(h->sv, o_cum), src + (named ? r : 0), (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

int dfm_irf_batch_dev(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                      const double* R, const double* sd, const int* named, const int* cum, double* irf, double* fevd,
                      unsigned flags) {
    if (H < 1) return fail(h, DFM_E_DIMS, "H must be >= 1%s");
    if (int rc = sv_check(h, B, 1, N, r, p, named, flags)) return rc;
    if (!Lam || !Avar || !Q || !irf || (fevd && !R)) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), rr = (size_t)r * r;
    bool any_cum = false;
    if (cum)
        for (int i = 0; i < N; ++i) any_cum = any_cum || cum[i] != 0;
    if (!any_cum) cum = nullptr;
    size_t off = 0;
    const size_t o_named = named ? take(off, (size_t)r * sizeof(int)) : (size_t)-1, o_cum = cum ? take(off, (size_t)N * sizeof(int)) : (size_t)-1,
                 o_S = take(off, B * rr * d), o_sc = (flags & DFM_SV_UNIT_EFFECT) ? take(off, (size_t)B * r * d) : (size_t)-1,
                 o_Th = take(off, (size_t)B * H * rr * d), o_Thc = cum ? take(off, (size_t)B * H * rr * d) : (size_t)-1;
    HIP_TRY(h, h->sv.grow(off));
    if (int rc = sv_upload_idx(h, r, N, named, cum, o_named, o_cum)) return rc;
    SvArgs a{};
    a.B = B; a.N = N; a.r = r; a.p = p; a.H = H; a.T = 0;
    a.Lam = Lam; a.R = fevd ? R : nullptr; a.A = Avar; a.Q = Q; a.sd = sd;
    a.named = at<int>(h->sv, o_named); a.cum = at<int>(h->sv, o_cum);
    a.status = h->status_dev;
    a.S = at<double>(h->sv, o_S); a.scale = at<double>(h->sv, o_sc); a.Th = at<double>(h->sv, o_Th); a.Thc = at<double>(h->sv, o_Thc);
    a.irf = irf; a.fevd = fevd;
    HIP_LAUNCH(h, K_SV_PREP, launch_sv_prep(a, h->stream));
    HIP_LAUNCH(h, K_SV_IRF_FILL, launch_sv_irf_fill(a, h->stream));
    return 0;
}

int dfm_irf_batch(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                  const double* R, const double* sd, const int* named, const int* cum, double* irf, double* fevd,
                  unsigned flags) {
    if (H < 1) return fail(h, DFM_E_DIMS, "H must be >= 1%s");
    if (int rc = sv_check(h, B, 1, N, r, p, named, flags)) return rc;
    if (!Lam || !Avar || !Q || !irf || (fevd && !R)) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_R = (size_t)B * N, n_o = (size_t)B * H * N;
    HostStage st(h, 256);
    double *lam_d, *A_d, *Q_d, *R_d, *sd_d, *irf_d, *fv_d;
    st.in(Lam, n_R * r, lam_d); st.in(Avar, (size_t)B * r * r * p, A_d); st.in(Q, (size_t)B * r * r, Q_d);
    st.in(R, R ? n_R : 0, R_d); st.in(sd, sd ? n_R : 0, sd_d);
    st.out(irf, n_o * r, irf_d); st.out(fevd, fevd ? n_o * (r + 1) : 0, fv_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_irf_batch_dev(h, B, N, r, p, H, lam_d, A_d, Q_d, R_d, sd_d, named, cum, irf_d, fv_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}

// ---- sign-restricted impulse responses (signirf.hip) ----------------------------------------------------------------------------
// The restrictions as the kernels read them: the distinct restricted series, and the rows (index into that list, h0, h1, sign)
// sorted by shock with the first row of every shock.
struct SignPlan {
    std::vector<int> ser, gs, rows;
    int HT = 1;
};
static SignPlan sign_plan(int r, int G, const int* restr) {
    SignPlan sp;
    sp.gs.assign((size_t)r + 1, 0);
    for (int k = 0; k < r; ++k) {
        for (int g = 0; g < G; ++g) {
            const int* q = restr + 5 * g;
            if (q[1] != k) continue;
            size_t s = 0;
            while (s < sp.ser.size() && sp.ser[s] != q[0]) ++s;
            if (s == sp.ser.size()) sp.ser.push_back(q[0]);
            const int row[4] = {(int)s, q[2], q[3], q[4]};
            sp.rows.insert(sp.rows.end(), row, row + 4);
            if (q[3] + 1 > sp.HT) sp.HT = q[3] + 1;
        }
        sp.gs[k + 1] = (int)sp.rows.size() / 4;
    }
    return sp;
}

// Sizes and restrictions first (they are decided before the handle is looked at), then the handle and the required pointers.
// *sp: the plan of the restrictions, built once per call.
static int signirf_check(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                         const double* R, const int* named, int G, const int* restr, int M, int K, const int* n_accept,
                         const int* cand_out, const double* fevd, unsigned flags, SignPlan* sp) {
    if (H < 1) return fail(h, DFM_E_DIMS, "H must be >= 1%s");
    if (M < 1 || K < 1 || G < 0) return fail(h, DFM_E_DIMS, "need M >= 1, K >= 1 and G >= 0%s");
    if (G > 0 && !restr) return fail(h, DFM_E_NULL, "G > 0 restrictions but restr is NULL%s");
    for (int g = 0; g < G; ++g) {
        const int* q = restr + 5 * g;
        if (q[0] < 0 || q[0] >= N || q[1] < 0 || q[1] >= r || q[2] < 0 || q[3] < q[2] || q[3] >= H || (q[4] != 1 && q[4] != -1))
            return fail(h, DFM_E_DIMS, "a restriction (series, shock, h0, h1, sign) is out of range%s");
    }
    if (r >= 1 && r <= DFM_MAX_R) {
        *sp = sign_plan(r, G, restr);
        if (dfm::sign_table_bytes((int)sp->ser.size(), sp->HT, r) > dfm::kSgTabLds)
            return fail(h, DFM_E_DIMS, "the table of restricted responses (distinct series x (max h1 + 1) x r doubles) exceeds 48 KB%s");
    }
    if (int rc = sv_check(h, B, 1, N, r, p, named, 0)) return rc;
    if ((long long)B * M > 0x7fffffffLL || (long long)B * K > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * M and B * K must be < 2^31%s");
    if (flags & DFM_SV_UNIT_EFFECT) return fail(h, DFM_E_NULL, "DFM_SV_UNIT_EFFECT: a rotated shock has no named series to normalise on%s");
    if (!Lam || !Avar || !Q || !n_accept || !cand_out || (fevd && !R)) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return 0;
}

// The checked call on device pointers: what both entries run.
static int signirf_run(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                       const double* R, const double* sd, const int* named, const int* cum, int G, const SignPlan& sp, int M, int K,
                       uint64_t seed, int64_t first_cand, int* n_accept, int* mask_out, int* cand_out, double* S_out, double* irf,
                       double* fevd) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), rr = (size_t)r * r, BK = (size_t)B * K;
    bool any_cum = false;
    if (cum)
        for (int i = 0; i < N; ++i) any_cum = any_cum || cum[i] != 0;
    if (!any_cum) cum = nullptr;
    const int nS = (int)sp.ser.size();
    const bool fill = irf || fevd;
    // the host integers, in the order they lie at the start of h->sv: named | cum | ser | gs | rows
    std::vector<int>& ix = h->sv_idx;
    ix.clear();
    const size_t i_named = ix.size(); if (named) ix.insert(ix.end(), named, named + r);
    const size_t i_cum = ix.size();   if (cum) ix.insert(ix.end(), cum, cum + N);
    const size_t i_ser = ix.size();   ix.insert(ix.end(), sp.ser.begin(), sp.ser.end());
    const size_t i_gs = ix.size();    ix.insert(ix.end(), sp.gs.begin(), sp.gs.end());
    const size_t i_rows = ix.size();  ix.insert(ix.end(), sp.rows.begin(), sp.rows.end());
    size_t off = 0;
    const size_t o_ix = take(off, ix.size() * sizeof(int)), o_S = take(off, B * rr * d), o_Th = take(off, (size_t)B * H * rr * d),
                 o_Thc = cum ? take(off, (size_t)B * H * rr * d) : (size_t)-1, o_tab = take(off, (size_t)B * nS * sp.HT * r * d + 8),
                 o_mask = mask_out ? (size_t)-1 : take(off, (size_t)B * M * sizeof(int)),
                 o_wcnt = take(off, (size_t)B * ((M + 63) / 64) * sizeof(int)), o_rot = take(off, (size_t)B * M * rr * d),
                 o_ThK = fill ? take(off, BK * H * rr * d) : (size_t)-1, o_ThcK = (fill && cum) ? take(off, BK * H * rr * d) : (size_t)-1;
    HIP_TRY(h, h->sv.grow(off));
    int* ixd = at<int>(h->sv, o_ix);
    HIP_TRY(h, hipMemcpyAsync(ixd, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    SvArgs a{};
    a.B = B; a.N = N; a.r = r; a.p = p; a.H = H; a.T = 0;
    a.Lam = Lam; a.R = fevd ? R : nullptr; a.A = Avar; a.Q = Q; a.sd = sd;
    a.named = named ? ixd + i_named : nullptr; a.cum = cum ? ixd + i_cum : nullptr;
    a.status = h->status_dev;
    a.S = at<double>(h->sv, o_S); a.Th = at<double>(h->sv, o_Th); a.Thc = at<double>(h->sv, o_Thc);
    HIP_LAUNCH(h, K_SV_PREP, launch_sv_prep(a, h->stream));
    SgArgs g{};
    g.B = B; g.N = N; g.r = r; g.H = H; g.M = M; g.K = K; g.nS = nS; g.HT = sp.HT; g.G = G;
    g.Lam = Lam; g.sd = sd; g.cum = a.cum; g.ser = ixd + i_ser; g.gs = ixd + i_gs; g.rows = ixd + i_rows;
    g.S = a.S; g.Th = a.Th; g.Thc = a.Thc; g.tab = at<double>(h->sv, o_tab);
    g.seed = seed; g.first_cand = first_cand;
    g.mask = mask_out ? mask_out : at<int>(h->sv, o_mask); g.wcnt = at<int>(h->sv, o_wcnt); g.rot = at<double>(h->sv, o_rot);
    g.n_accept = n_accept; g.cand_out = cand_out; g.S_out = S_out;
    g.ThK = at<double>(h->sv, o_ThK); g.ThcK = at<double>(h->sv, o_ThcK);
    if (nS > 0) HIP_LAUNCH(h, K_SV_SIGN_TABLE, launch_sv_sign_table(g, h->stream));
    HIP_LAUNCH(h, K_SV_SIGN, launch_sv_sign(g, h->stream));
    HIP_LAUNCH(h, K_SV_SIGN_KEEP, launch_sv_sign_keep(g, h->stream));
    if (!fill) return 0;
    a.B = B; a.slots = K; a.Th = g.ThK; a.Thc = g.ThcK; a.irf = irf; a.fevd = fevd;
    HIP_LAUNCH(h, K_SV_IRF_FILL, launch_sv_irf_fill(a, h->stream));
    return 0;
}

int dfm_signirf_batch_dev(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                          const double* R, const double* sd, const int* named, const int* cum, int G, const int* restr, int M, int K,
                          uint64_t seed, int64_t first_cand, int* n_accept, int* mask_out, int* cand_out, double* S_out, double* irf,
                          double* fevd, unsigned flags) {
    SignPlan sp;
    if (int rc = signirf_check(h, B, N, r, p, H, Lam, Avar, Q, R, named, G, restr, M, K, n_accept, cand_out, fevd, flags, &sp)) return rc;
    return signirf_run(h, B, N, r, p, H, Lam, Avar, Q, R, sd, named, cum, G, sp, M, K, seed, first_cand, n_accept, mask_out, cand_out,
                       S_out, irf, fevd);
}

int dfm_signirf_batch(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                      const double* R, const double* sd, const int* named, const int* cum, int G, const int* restr, int M, int K,
                      uint64_t seed, int64_t first_cand, int* n_accept, int* mask_out, int* cand_out, double* S_out, double* irf,
                      double* fevd, unsigned flags) {
    SignPlan sp;
    if (int rc = signirf_check(h, B, N, r, p, H, Lam, Avar, Q, R, named, G, restr, M, K, n_accept, cand_out, fevd, flags, &sp)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_R = (size_t)B * N, BK = (size_t)B * K, n_o = BK * H * N;
    HostStage st(h, 256);
    double *lam_d, *A_d, *Q_d, *R_d, *sd_d, *S_d, *irf_d, *fv_d;
    int *na_d, *mk_d, *cd_d;
    st.in(Lam, n_R * r, lam_d); st.in(Avar, (size_t)B * r * r * p, A_d); st.in(Q, (size_t)B * r * r, Q_d);
    st.in(R, R ? n_R : 0, R_d); st.in(sd, sd ? n_R : 0, sd_d);
    st.out(n_accept, (size_t)B, na_d); st.out(mask_out, mask_out ? (size_t)B * M : 0, mk_d); st.out(cand_out, BK, cd_d);
    st.out(S_out, S_out ? BK * r * r : 0, S_d); st.out(irf, irf ? n_o * r : 0, irf_d); st.out(fevd, fevd ? n_o * (r + 1) : 0, fv_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(signirf_run(h, B, N, r, p, H, lam_d, A_d, Q_d, R_d, sd_d, named, cum, G, sp, M, K, seed, first_cand, na_d, mk_d,
                                   cd_d, S_d, irf_d, fv_d));
    if (rc == 0) rc = status_check(h);
    return rc;
}

int dfm_histdecomp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                             const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                             const double* sd, const int* named, double* hd, double* shocks, double* f_out, double* loglik,
                             unsigned flags) {
    if (T < p + 1) return fail(h, DFM_E_DIMS, "T must be >= p + 1%s");
    if (int rc = sv_check(h, B, T, N, r, p, named, 0)) return rc;
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !hd) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), rr = (size_t)r * r, n_f = (size_t)B * T * r;
    size_t off = 0;
    const size_t o_named = named ? take(off, (size_t)r * sizeof(int)) : (size_t)-1, o_S = take(off, B * rr * d), o_Si = take(off, B * rr * d),
                 o_f = f_out ? (size_t)-1 : take(off, n_f * d), o_ll = loglik ? (size_t)-1 : take(off, (size_t)B * d),
                 o_u = shocks ? (size_t)-1 : take(off, n_f * d), o_C = take(off, n_f * (r + 1) * d);
    HIP_TRY(h, h->sv.grow(off));
    if (int rc = sv_upload_idx(h, r, N, named, nullptr, o_named, (size_t)-1)) return rc;
    double* f = f_out ? f_out : at<double>(h->sv, o_f);
    double* ll = loglik ? loglik : at<double>(h->sv, o_ll);
    const unsigned pass_flags = flags & (DFM_F_MAY_HAVE_MISSING | DFM_F_SINGULAR_Q);
    if (p == 1) {
        if (int rc = dfm_ks_pass_batch_dev(h, B, T, N, r, panel, Lam, R, Avar, Q, mu0, P0, f, nullptr, ll, pass_flags)) return rc;
    } else {
        if (int rc = dfm_ks_pass_varp_batch_dev(h, B, T, N, r, p, panel, Lam, R, Avar, Q, mu0, P0, f, nullptr, ll, pass_flags)) return rc;
    }
    SvArgs a{};
    a.B = B; a.N = N; a.r = r; a.p = p; a.H = 0; a.T = T;
    a.Lam = Lam; a.A = Avar; a.Q = Q; a.sd = sd;
    a.named = at<int>(h->sv, o_named);
    a.need_pd = 1; a.status = h->status_dev;
    a.S = at<double>(h->sv, o_S); a.Sinv = at<double>(h->sv, o_Si);
    a.f = f; a.u = shocks ? shocks : at<double>(h->sv, o_u); a.C = at<double>(h->sv, o_C); a.hd = hd;
    HIP_LAUNCH(h, K_SV_PREP, launch_sv_prep(a, h->stream));
    HIP_LAUNCH(h, K_SV_SHOCK, launch_sv_shock(a, h->stream));
    HIP_LAUNCH(h, K_SV_PATH, launch_sv_path(a, h->stream));
    HIP_LAUNCH(h, K_SV_HD_FILL, launch_sv_hd_fill(a, h->stream));
    return 0;
}

int dfm_histdecomp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                         const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                         const double* sd, const int* named, double* hd, double* shocks, double* f_out, double* loglik,
                         unsigned flags) {
    if (T < p + 1) return fail(h, DFM_E_DIMS, "T must be >= p + 1%s");
    if (int rc = sv_check(h, B, T, N, r, p, named, 0)) return rc;
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !hd) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, n_R = (size_t)B * N, n_f = (size_t)B * T * r;
    std::vector<double> ll_host((size_t)B);                     // (checked before the caller's loglik, which is optional, is written)
    HostStage st(h, 256);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *sd_d, *hd_d, *u_d, *f_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(Lam, n_R * r, lam_d); st.in(R, n_R, R_d); st.in(Avar, (size_t)B * r * k, A_d);
    st.in(Q, (size_t)B * r * r, Q_d); st.in(mu0, (size_t)B * k, mu_d); st.in(P0, (size_t)B * k * k, P0_d); st.in(sd, sd ? n_R : 0, sd_d);
    st.out(hd, (size_t)B * (r + 1) * T * N, hd_d); st.out(shocks, shocks ? n_f : 0, u_d); st.out(f_out, f_out ? n_f : 0, f_d);
    st.out(ll_host.data(), (size_t)B, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_histdecomp_batch_dev(h, B, T, N, r, p, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, sd_d, named, hd_d, u_d, f_d, ll_d,
                                                flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), B);
    if (rc == 0 && loglik) memcpy(loglik, ll_host.data(), (size_t)B * sizeof(double));
    return rc;
}

// ---- impulse responses identified by an external instrument (proxy.hip) ----------------------------------------------------------
// Sizes, norm and the instrument first (they are decided before the handle is looked at), then the handle and the required
// pointers.  *U: the used rows {t : p <= t < T, z_t finite}, built once per call.
static int proxyirf_check(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                          const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, const double* z,
                          int norm, int D, int L, int64_t first_draw, const double* impact, const double* rel, std::vector<int>* U) {
    if (H < 1) return fail(h, DFM_E_DIMS, "H must be >= 1%s");
    if (D < 0 || first_draw < 0) return fail(h, DFM_E_DIMS, "need D >= 0 and first_draw >= 0%s");
    if (B < 1 || T < 1 || N < 1 || r < 1) return fail(h, DFM_E_DIMS, "B, T, N, r must be >= 1%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r > DFM_MAX_R || (long long)r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (T < p + 1) return fail(h, DFM_E_DIMS, "T must be >= p + 1%s");
    if (norm < 0 || norm >= N) return fail(h, DFM_E_DIMS, "norm lies outside [0, N)%s");
    if ((long long)B * ((long long)D + 1) > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * (D + 1) must be < 2^31%s");
    if (L < 1) return fail(h, DFM_E_DIMS, "the block length L must be >= 1%s");
    if (z) {
        U->clear();
        for (int t = p; t < T; ++t)
            if (isfinite(z[t])) U->push_back(t);
        const int n = (int)U->size();
        if (n < r + 2) return fail(h, DFM_E_DIMS, "the instrument has fewer than r + 2 usable periods%s");
        if (L > n) return fail(h, DFM_E_DIMS, "the block length L exceeds the number of usable periods%s");
    }
    if (!h) return DFM_E_NULL;
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !z || !impact || !rel) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    return 0;
}

// The checked call on device pointers (z and cum on the host): what both entries run.
static int proxyirf_run(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                        const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, const double* sd,
                        const int* cum, const std::vector<int>& U, const double* z, int norm, int D, int L, uint64_t seed,
                        int64_t first_draw, double* impact, double* rel, double* irf, double* fevd, double* shock, double* f_out,
                        double* loglik, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), rr = (size_t)r * r, n_f = (size_t)B * T * r, BS = (size_t)B * ((size_t)D + 1);
    const int n = (int)U.size();
    bool any_cum = false;
    if (cum)
        for (int i = 0; i < N; ++i) any_cum = any_cum || cum[i] != 0;
    if (!any_cum) cum = nullptr;
    const bool fill = irf || fevd, unit = (flags & DFM_SV_UNIT_EFFECT) != 0;
    // the host integers, in the order they lie at the start of h->sv: cum | U
    std::vector<int>& ix = h->sv_idx;
    ix.clear();
    if (cum) ix.insert(ix.end(), cum, cum + N);
    const size_t i_U = ix.size();
    ix.insert(ix.end(), U.begin(), U.end());
    h->sv_z.assign(z, z + T);
    size_t off = 0;
    const size_t o_ix = take(off, ix.size() * sizeof(int)), o_z = take(off, (size_t)T * d), o_S = take(off, B * rr * d),
                 o_Si = take(off, B * rr * d), o_Th = take(off, (size_t)B * H * rr * d),
                 o_Thc = cum ? take(off, (size_t)B * H * rr * d) : (size_t)-1, o_f = f_out ? (size_t)-1 : take(off, n_f * d),
                 o_ll = loglik ? (size_t)-1 : take(off, (size_t)B * d), o_rows = take(off, (size_t)B * n * (r + 1) * d),
                 o_w = take(off, BS * r * d), o_tk = fill ? take(off, BS * H * r * d) : (size_t)-1,
                 o_tkc = (fill && cum) ? take(off, BS * H * r * d) : (size_t)-1,
                 o_sc = (fill && unit) ? take(off, BS * d) : (size_t)-1, o_den = fevd ? take(off, (size_t)B * H * N * d) : (size_t)-1;
    HIP_TRY(h, h->sv.grow(off));
    int* ixd = at<int>(h->sv, o_ix);
    HIP_TRY(h, hipMemcpyAsync(ixd, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(at<double>(h->sv, o_z), h->sv_z.data(), (size_t)T * d, hipMemcpyHostToDevice, h->stream));
    double* f = f_out ? f_out : at<double>(h->sv, o_f);
    double* ll = loglik ? loglik : at<double>(h->sv, o_ll);
    const unsigned pass_flags = flags & (DFM_F_MAY_HAVE_MISSING | DFM_F_SINGULAR_Q);
    if (p == 1) {
        if (int rc = dfm_ks_pass_batch_dev(h, B, T, N, r, panel, Lam, R, Avar, Q, mu0, P0, f, nullptr, ll, pass_flags)) return rc;
    } else {
        if (int rc = dfm_ks_pass_varp_batch_dev(h, B, T, N, r, p, panel, Lam, R, Avar, Q, mu0, P0, f, nullptr, ll, pass_flags)) return rc;
    }
    SvArgs a{};
    a.B = B; a.N = N; a.r = r; a.p = p; a.H = H; a.T = T;
    a.Lam = Lam; a.A = Avar; a.Q = Q; a.sd = sd;
    a.need_pd = 1; a.status = h->status_dev;
    a.S = at<double>(h->sv, o_S); a.Sinv = at<double>(h->sv, o_Si); a.Th = at<double>(h->sv, o_Th); a.Thc = at<double>(h->sv, o_Thc);
    HIP_LAUNCH(h, K_SV_PREP, launch_sv_prep(a, h->stream));
    PxArgs g{};
    g.B = B; g.T = T; g.N = N; g.r = r; g.p = p; g.H = H; g.n = n; g.D = D; g.L = L; g.norm = norm; g.unit = unit ? 1 : 0;
    g.Lam = Lam; g.sd = sd; g.A = Avar; g.cum = cum ? ixd : nullptr; g.U = ixd + i_U; g.z = at<double>(h->sv, o_z); g.f = f;
    g.S = a.S; g.Sinv = a.Sinv; g.Th = a.Th; g.Thc = a.Thc;
    g.seed = seed; g.first_draw = first_draw;
    g.rows = at<double>(h->sv, o_rows); g.impact = impact; g.rel = rel; g.w = at<double>(h->sv, o_w);
    g.tk = at<double>(h->sv, o_tk); g.tkc = at<double>(h->sv, o_tkc); g.scale = at<double>(h->sv, o_sc);
    g.R = R; g.den = at<double>(h->sv, o_den); g.irf = irf; g.fevd = fevd; g.shock = shock;
    HIP_LAUNCH(h, K_PX_ROWS, launch_px_rows(g, h->stream));
    HIP_LAUNCH(h, K_PX_MOMENT, launch_px_moment(g, h->stream));
    if (shock) HIP_LAUNCH(h, K_PX_SHOCK, launch_px_shock(g, h->stream));
    if (!fill) return 0;
    HIP_LAUNCH(h, K_PX_SLOT_TABLE, launch_px_slot_table(g, h->stream));
    if (fevd) HIP_LAUNCH(h, K_PX_DEN, launch_px_den(g, h->stream));
    HIP_LAUNCH(h, K_PX_FILL, launch_px_fill(g, h->stream));
    return 0;
}

int dfm_proxyirf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                           const double* sd, const int* cum, const double* z, int norm, int D, int L, uint64_t seed,
                           int64_t first_draw, double* impact, double* rel, double* irf, double* fevd, double* shock,
                           double* f_out, double* loglik, unsigned flags) {
    std::vector<int> U;
    if (int rc = proxyirf_check(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, z, norm, D, L, first_draw, impact, rel, &U)) return rc;
    return proxyirf_run(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, sd, cum, U, z, norm, D, L, seed, first_draw, impact, rel,
                        irf, fevd, shock, f_out, loglik, flags);
}

int dfm_proxyirf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                       const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, const double* sd,
                       const int* cum, const double* z, int norm, int D, int L, uint64_t seed, int64_t first_draw, double* impact,
                       double* rel, double* irf, double* fevd, double* shock, double* f_out, double* loglik, unsigned flags) {
    std::vector<int> U;
    if (int rc = proxyirf_check(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, z, norm, D, L, first_draw, impact, rel, &U)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, n_R = (size_t)B * N, n_f = (size_t)B * T * r, BS = (size_t)B * ((size_t)D + 1), n_o = BS * H * N;
    std::vector<double> ll_host((size_t)B);                     // (checked before the caller's loglik, which is optional, is written)
    HostStage st(h, 256);
    double *x_d, *lam_d, *R_d, *A_d, *Q_d, *mu_d, *P0_d, *sd_d, *im_d, *rel_d, *irf_d, *fv_d, *u_d, *f_d, *ll_d;
    st.in(panel, (size_t)B * T * N, x_d); st.in(Lam, n_R * r, lam_d); st.in(R, n_R, R_d); st.in(Avar, (size_t)B * r * k, A_d);
    st.in(Q, (size_t)B * r * r, Q_d); st.in(mu0, (size_t)B * k, mu_d); st.in(P0, (size_t)B * k * k, P0_d); st.in(sd, sd ? n_R : 0, sd_d);
    st.out(impact, BS * r, im_d); st.out(rel, BS, rel_d); st.out(irf, irf ? n_o : 0, irf_d); st.out(fevd, fevd ? n_o : 0, fv_d);
    st.out(shock, shock ? (size_t)B * T : 0, u_d); st.out(f_out, f_out ? n_f : 0, f_d); st.out(ll_host.data(), (size_t)B, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(proxyirf_run(h, B, T, N, r, p, H, x_d, lam_d, R_d, A_d, Q_d, mu_d, P0_d, sd_d, cum, U, z, norm, D, L, seed,
                                    first_draw, im_d, rel_d, irf_d, fv_d, u_d, f_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), B);
    if (rc == 0 && loglik) memcpy(loglik, ll_host.data(), (size_t)B * sizeof(double));
    return rc;
}

// ---- news decomposition of nowcast revisions (news.hip) --------------------------------------------------------------------
// The three conditional means run through dfm_forecast_batch_dev unchanged (old, new, then the revised old panel, whose xhat stays
// in h->nw for the impacts).  The B G weight passes run in slices of at most kNwSlice pass replicates j = b G + g, as
// simsmooth_run runs its difference panels: expand the parameters (mu0 = 0; simsmooth_expand_kernel with D = G), the a_t
// vectors, the covariance panels, the existing pass over them, the impacts.  With weight the covariance panels of a slice live
// in that slice's part of weight, which news_impact_kernel overwrites cell by cell.
static constexpr int kNwSlice = 8192;

// Argument check of both entries; *H = the horizon the targets need.
static int news_check(dfm_handle* h, int B, int T, int N, int r, int p, const double* oldp, const double* newp, const double* Lam,
                      const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                      const double* mean, const double* sd, int G, const int* target_t, const int* target_i, const double* yhat,
                      const double* impact, int* H) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (G < 1) return fail(h, DFM_E_DIMS, "G (targets) must be >= 1%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if ((long long)B * G > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * G must be < 2^31%s");
    if (!oldp || !newp || !Lam || !R || !Avar || !Q || !mu0 || !P0 || !target_t || !target_i || !yhat || !impact)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    if (!news_targets(T, N, G, target_t, target_i, 0, H)) return fail(h, DFM_E_DIMS, "a target lies outside [0, T + H) x [0, N)%s");
    return 0;
}

// ll_all: [3 B + B G] device log-likelihoods (the three forecasts, then the weight passes; the host entry checks them), or null
static int news_run(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* oldp, const double* newp,
                    const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                    const double* mean, const double* sd, int G, const int* target_t, const int* target_i, double* yhat,
                    double* impact, double* news, double* weight, double* ll_all, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t d = sizeof(double), k = (size_t)r * p, TH = (size_t)T + H;
    const long long BG = (long long)B * G;
    const int Smax = (int)(BG < kNwSlice ? BG : kNwSlice);
    size_t off = 0;
    const size_t o_t = take(off, (size_t)2 * G * sizeof(int)), o_rev = take(off, (size_t)B * T * N * d),
                 o_x = take(off, (size_t)B * TH * N * d), o_f = take(off, (size_t)B * TH * r * d);
    const SliceParams sp(off, Smax, N, r, k, 0);
    const size_t o_u = take(off, (size_t)Smax * T * k * d), o_av = take(off, (size_t)Smax * T * r * d),
                 o_g = take(off, (size_t)Smax * T * r * d),
                 o_ll = ll_all ? (size_t)-1 : take(off, (size_t)(B > Smax ? B : Smax) * d),
                 o_c = weight ? (size_t)-1 : take(off, (size_t)Smax * T * N * d);
    HIP_TRY(h, h->nw.grow(off));
    int* tgt = at<int>(h->nw, o_t);
    double *xhat = at<double>(h->nw, o_x), *fbuf = at<double>(h->nw, o_f);
    if (int rc = news_stage_targets(h, G, target_t, target_i, 0, tgt)) return rc;
    NwArgs a{};
    a.B = B; a.T = T; a.N = N; a.r = r; a.p = p; a.G = G; a.TH = (int)TH;
    a.oldp = oldp; a.newp = newp; a.Lam = Lam; a.R = R; a.A = Avar; a.P0 = P0; a.Q = Q; a.mean = mean; a.sd = sd;
    a.tgt = tgt; a.rev = at<double>(h->nw, o_rev); a.xrev = xhat; a.yhat = yhat; a.impact = impact; a.news = news; a.weight = weight;
    a.status = h->status_dev; a.u = at<double>(h->nw, o_u); a.av = at<double>(h->nw, o_av); a.g = at<double>(h->nw, o_g);
    HIP_LAUNCH(h, K_NW_REVISE, launch_news_revise(a, h->stream));
    if (int rc = news_forecasts(h, B, a, oldp, newp, a.rev, xhat, ll_all, at<double>(h->nw, o_ll), flags,
                                [&](const double* panel, double* ll, unsigned fl) {
        return dfm_forecast_batch_dev(h, B, T, N, r, p, H, panel, Lam, R, Avar, Q, mu0, P0, mean, sd, xhat, nullptr, nullptr, fbuf,
                                      nullptr, ll, fl);
    })) return rc;
    SsArgs e{};
    e.B = B; e.D = G; e.T = T; e.N = N; e.r = r; e.p = p;
    e.Lam = Lam; e.R = R; e.A = Avar; e.Q = Q; e.mu0 = mu0; e.P0 = P0;
    sp.point(h->nw, e);
    for (long long j0 = 0; j0 < BG; j0 += Smax) {
        const int S = (int)(BG - j0 < Smax ? BG - j0 : Smax);
        a.j0 = j0; a.S = S; e.j0 = j0; e.S = S;
        a.cp = weight ? weight + (size_t)j0 * T * N : at<double>(h->nw, o_c);
        double* ll = ll_all ? ll_all + (size_t)3 * B + j0 : at<double>(h->nw, o_ll);
        HIP_LAUNCH(h, K_SS_EXPAND, launch_simsmooth_expand(e, h->stream));
        HIP_LAUNCH(h, K_NW_GAMMA, launch_news_gamma(a, h->stream));
        HIP_LAUNCH(h, K_NW_COV, launch_news_cov_panel(a, h->stream));
        if (int rc = slice_pass(h, S, T, N, r, p, a.cp, e, at<double>(h->nw, o_g), ll, flags)) return rc;
        HIP_LAUNCH(h, K_NW_IMPACT, launch_news_impact(a, h->stream));
    }
    return 0;
}

int dfm_news_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* old_panel, const double* new_panel,
                       const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                       const double* P0, const double* mean, const double* sd, int G, const int* target_t, const int* target_i,
                       double* yhat, double* impact, double* news, double* weight, unsigned flags) {
    int H = 0;
    if (int rc = news_check(h, B, T, N, r, p, old_panel, new_panel, Lam, R, Avar, Q, mu0, P0, mean, sd, G, target_t, target_i, yhat,
                            impact, &H)) return rc;
    return news_run(h, B, T, N, r, p, H, old_panel, new_panel, Lam, R, Avar, Q, mu0, P0, mean, sd, G, target_t, target_i, yhat,
                    impact, news, weight, nullptr, flags);
}

int dfm_news_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* old_panel, const double* new_panel,
                   const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                   const double* mean, const double* sd, int G, const int* target_t, const int* target_i, double* yhat,
                   double* impact, double* news, double* weight, unsigned flags) {
    int H = 0;
    if (int rc = news_check(h, B, T, N, r, p, old_panel, new_panel, Lam, R, Avar, Q, mu0, P0, mean, sd, G, target_t, target_i, yhat,
                            impact, &H)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t BG = (size_t)B * G, n_panel = (size_t)B * T * N, n_ll = (size_t)3 * B + BG;
    std::vector<double> ll_host(n_ll);
    HostStage st(h, 256);
    ModelDev md;
    double *xo_d, *xn_d, *y_d, *imp_d, *news_d, *w_d, *ll_d;
    st.in(old_panel, n_panel, xo_d); st.in(new_panel, n_panel, xn_d);
    stage_model(st, md, B, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, mean, sd);
    st.out(yhat, (size_t)B * 3 * G, y_d); st.out(impact, BG * N, imp_d); st.out(news, news ? n_panel : 0, news_d);
    st.out(weight, weight ? BG * T * N : 0, w_d); st.out(ll_host.data(), n_ll, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(news_run(h, B, T, N, r, p, H, xo_d, xn_d, md.Lam, md.R, md.A, md.Q, md.mu0, md.P0, md.mean, md.sd, G, target_t,
                                target_i, y_d, imp_d, news_d, w_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), (int)n_ll);
    return rc;
}

// ---- news decomposition with AR idiosyncratic terms (news_ar.hip) ------------------------------------------------------------------
// As news_run, on the output rows of dfm_forecast_ar_batch_dev: the vintage check and the revised old panel, the three forecasts
// (old, new, then the revised old panel, whose xhat stays in h->nw for the news), then the B G weight passes in slices of at most
// kNwSlice pass replicates j = b G + g.  A slice: expand the parameters (mu0 = 0; the state has m = max(p, q + 1) lags, Avar padded
// with zero blocks), the u / Gamma recursion, the covariance panels -- which ARE quasi-differenced cells -- the inner part of the AR
// pass over them (no quasi_diff_kernel) with the whole smoothed state kept (the rows t < q need E[f_{t-l}] before output row 0),
// the impacts.  With weight the covariance panels of a slice live in that slice's part of weight.
static int news_ar_check(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* oldp, const double* newp,
                         const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                         const double* mu0, const double* P0, const double* mean, const double* sd, int G, const int* target_t,
                         const int* target_i, const double* yhat, const double* impact, int* H) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (G < 1) return fail(h, DFM_E_DIMS, "G (targets) must be >= 1%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be >= 1 (q = 0 is dfm_news_batch)%s");
    if (q > 4) return fail(h, DFM_E_R_UNSUPPORTED, "news with AR idiosyncratic terms needs q <= 4%s");
    if (T <= 2 * q) return fail(h, DFM_E_DIMS, "T must exceed 2 q (q conditioning rows, q rows that fix the idiosyncratic state)%s");
    if ((long long)B * G > 0x7fffffffLL) return fail(h, DFM_E_DIMS, "B * G must be < 2^31%s");
    if (!oldp || !newp || !Lam || !sig2 || !rho || !Avar || !Q || !mu0 || !P0 || !target_t || !target_i || !yhat || !impact)
        return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    if (!news_targets(T, N, G, target_t, target_i, q, H)) return fail(h, DFM_E_DIMS, "a target lies outside [q, T + H) x [0, N)%s");
    return ar_check(h, B, T + *H, N, r, p, q, false);
}

// The AR pass's inner part over S panels of ns rows that are quasi-differenced already; g [S][ns][Rp] takes the whole smoothed
// state (out_r = Rp, as ar_em_run takes it).  ar_plan's room for a quasi-differenced panel stays unused.
static int news_ar_pass(dfm_handle* h, int S, int ns, int N, int r, int m, int q, const double* qc, const double* Lam,
                        const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                        const double* P0, double* g, double* ll, unsigned flags) {
    ArPlan s;
    if (int rc = ar_plan(h, S, ns + q, N, r, m, q, flags, false, &s)) return rc;
    if (int rc = launch_1d(h, ar_loadings_kernel, (size_t)S * N * s.p.Rp, S, N, r, q, s.p.Rp, Lam, rho, s.mb.Lam)) return rc;
    if (int rc = companion_pad(h, s.p, S, N, r, s.k, r * m, nullptr, Avar, Q, mu0, P0, s.mb)) return rc;
    return enqueue_pass(h, s.p, S, ns, N, s.p.Rp, qc, s.mb.pp(), sig2, g, nullptr, ll, nullptr);
}

// ll_all: [3 B + B G] device log-likelihoods (the three forecasts, then the weight passes; the host entry checks them), or null
static int news_ar_run(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* oldp, const double* newp,
                       const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                       const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd, int G,
                       const int* target_t, const int* target_i, double* yhat, double* impact, double* news, double* weight,
                       double* ll_all, unsigned flags) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int m = state_lags(p, q), Rp = pad_r(r * m), w = (q + 1) * r;
    const size_t d = sizeof(double), k = (size_t)r * m, TH = (size_t)T + H, n = TH - q, ns = (size_t)T - q;
    const long long BG = (long long)B * G;
    const int Smax = (int)(BG < kNwSlice ? BG : kNwSlice);
    size_t off = 0;
    const size_t o_t = take(off, (size_t)2 * G * sizeof(int)), o_rev = take(off, (size_t)B * T * N * d),
                 o_x = take(off, (size_t)B * n * N * d), o_f = take(off, (size_t)B * n * r * d),
                 o_Ap = p < m ? take(off, (size_t)B * r * k * d) : (size_t)-1;
    const SliceParams sp(off, Smax, N, r, k, q);
    const size_t o_u = take(off, (size_t)Smax * ns * (k + 1) * d),
                 o_dv = take(off, (size_t)Smax * ns * (w + 1) * d), o_g = take(off, (size_t)Smax * ns * Rp * d),
                 o_ll = ll_all ? (size_t)-1 : take(off, (size_t)(B > Smax ? B : Smax) * d),
                 o_c = weight ? (size_t)-1 : take(off, (size_t)Smax * ns * N * d);
    HIP_TRY(h, h->nw.grow(off));
    int* tgt = at<int>(h->nw, o_t);
    double *xhat = at<double>(h->nw, o_x), *fbuf = at<double>(h->nw, o_f);
    if (int rc = news_stage_targets(h, G, target_t, target_i, q, tgt)) return rc;       // (output rows)
    NwArArgs a{};
    a.B = B; a.T = T; a.N = N; a.r = r; a.q = q; a.k = (int)k; a.ka = r * p; a.G = G; a.n = (int)n; a.ns = (int)ns; a.Rp = Rp;
    a.oldp = oldp; a.newp = newp; a.Lam = Lam; a.sig2 = sig2; a.rho = rho; a.A = Avar; a.Q = Q; a.P0 = P0; a.mean = mean; a.sd = sd;
    a.tgt = tgt; a.rev = at<double>(h->nw, o_rev); a.xrev = xhat; a.impact = impact; a.news = news; a.weight = weight;
    a.status = h->status_dev; a.u = at<double>(h->nw, o_u); a.dv = at<double>(h->nw, o_dv); a.g = at<double>(h->nw, o_g);
    HIP_LAUNCH(h, K_NWAR_REVISE, launch_news_ar_revise(a, h->stream));
    NwArgs ga{};                                              // news_gather_kernel on the forecasts' n output rows
    ga.B = B; ga.G = G; ga.N = N; ga.TH = (int)n; ga.tgt = tgt; ga.yhat = yhat;
    if (int rc = news_forecasts(h, B, ga, oldp, newp, a.rev, xhat, ll_all, at<double>(h->nw, o_ll), flags,
                                [&](const double* panel, double* ll, unsigned fl) {
        return dfm_forecast_ar_batch_dev(h, B, T, N, r, p, q, H, panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd, xhat, nullptr,
                                         nullptr, nullptr, fbuf, nullptr, ll, fl);
    })) return rc;
    const double* Am;
    if (int rc = pad_avar(h, B, r, p, m, Avar, at<double>(h->nw, o_Ap), &Am)) return rc;
    SsArgs e{};
    e.B = B; e.D = G; e.T = (int)ns; e.N = N; e.r = r; e.p = m;
    e.Lam = Lam; e.R = sig2; e.A = Am; e.Q = Q; e.mu0 = mu0; e.P0 = P0;
    double* erho = sp.point(h->nw, e);
    for (long long j0 = 0; j0 < BG; j0 += Smax) {
        const int S = (int)(BG - j0 < Smax ? BG - j0 : Smax);
        a.j0 = j0; a.S = S; e.j0 = j0; e.S = S;
        a.qc = weight ? weight + (size_t)j0 * ns * N : at<double>(h->nw, o_c);
        double* ll = ll_all ? ll_all + (size_t)3 * B + j0 : at<double>(h->nw, o_ll);
        HIP_LAUNCH(h, K_SS_EXPAND, launch_simsmooth_expand(e, h->stream));
        HIP_LAUNCH(h, K_SSAR_EXPAND, launch_simsmooth_ar_expand(S, j0, G, (size_t)N * q, rho, erho, h->stream));
        HIP_LAUNCH(h, K_NWAR_REC, launch_news_ar_rec(a, h->stream));
        HIP_LAUNCH(h, K_NWAR_QC, launch_news_ar_qc(a, h->stream));
        if (int rc = news_ar_pass(h, S, (int)ns, N, r, m, q, a.qc, e.eLam, e.eR, erho, e.eA, e.eQ, e.emu0, e.eP0, at<double>(h->nw, o_g), ll,
                                  flags)) return rc;
        HIP_LAUNCH(h, K_NWAR_IMPACT, launch_news_ar_impact(a, h->stream));
    }
    return 0;
}

int dfm_news_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* old_panel, const double* new_panel,
                          const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                          const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd, int G,
                          const int* target_t, const int* target_i, double* yhat, double* impact, double* news, double* weight,
                          unsigned flags) {
    int H = 0;
    if (int rc = news_ar_check(h, B, T, N, r, p, q, old_panel, new_panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, G, target_t,
                               target_i, yhat, impact, &H)) return rc;
    return news_ar_run(h, B, T, N, r, p, q, H, old_panel, new_panel, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd, G, target_t,
                       target_i, yhat, impact, news, weight, nullptr, flags);
}

int dfm_news_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* old_panel, const double* new_panel,
                      const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                      const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd, int G,
                      const int* target_t, const int* target_i, double* yhat, double* impact, double* news, double* weight,
                      unsigned flags) {
    int H = 0;
    if (int rc = news_ar_check(h, B, T, N, r, p, q, old_panel, new_panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd, G, target_t,
                               target_i, yhat, impact, &H)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t BG = (size_t)B * G, n_panel = (size_t)B * T * N, n_s = (size_t)B * (T - q) * N, n_ll = (size_t)3 * B + BG;
    std::vector<double> ll_host(n_ll);
    HostStage st(h, 256);
    ModelDev md;
    double *xo_d, *xn_d, *y_d, *imp_d, *news_d, *w_d, *ll_d;
    st.in(old_panel, n_panel, xo_d); st.in(new_panel, n_panel, xn_d);
    stage_model(st, md, B, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, v0, mean, sd);
    st.out(yhat, (size_t)B * 3 * G, y_d); st.out(impact, BG * N, imp_d); st.out(news, news ? n_s : 0, news_d);
    st.out(weight, weight ? (size_t)G * n_s : 0, w_d); st.out(ll_host.data(), n_ll, ll_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(news_ar_run(h, B, T, N, r, p, q, H, xo_d, xn_d, md.Lam, md.R, md.rho, md.A, md.Q, md.mu0, md.P0, md.v0, md.mean, md.sd,
                                   G, target_t, target_i, y_d, imp_d, news_d, w_d, ll_d, flags));
    if (rc == 0) rc = post_check(h, ll_host.data(), (int)n_ll);
    return rc;
}


// ---- filtered states, prediction errors and out-of-sample evaluation (filter.hip) -------------------------------------------------
// One forward pass, outside enqueue_pass: the loadings padded to pad_r(r) columns (pad_params_kernel), collapse_kernel into arrays
// of h->ft (this one collapse route only), filter_kernel, then filter_fill_kernel and filter_eval_kernel for the outputs the caller
// takes.  The moments the later kernels read (z_pred / P_pred for the fill, z_filt for the evaluation) live in h->ft when the
// caller does not take them.  The parameters are the same at every origin.
static int filter_check(dfm_handle* h, int B, int T, int N, int r, int p, int H, int t0, const double* panel, const double* Lam,
                        const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                        const double* mean, const double* sd) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (t0 < 0 || t0 >= T) return fail(h, DFM_E_DIMS, "t0 (the first origin) must lie in [0, T)%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (r * p > DFM_MAX_R) return fail(h, DFM_E_R_UNSUPPORTED, "r * p > DFM_MAX_R (32)%s");
    if (!panel || !Lam || !R || !Avar || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    return check_general_n(h, N, r);
}

// What both filter drivers carve from h->ft behind their own arrays (`off`: the bytes those take), from the dimensions, inputs and
// caller's outputs already in `fa`: the collapse's per-period arrays over the n rows (into `ca` and `fa`), the moments the later
// kernels read and the caller does not take, and the evaluation's running sums.  Grows h->ft to the total.
static int filter_carve(dfm_handle* h, size_t off, bool miss, bool fill, bool eval, CollapseArgs& ca, FtCells& fa) {
    const size_t d = sizeof(double), B = (size_t)fa.B, Bn = B * fa.n, k = (size_t)fa.k, kk = k * (k + 1) / 2, Rp = (size_t)fa.Rp,
                 n_e = B * fa.H * fa.N;
    const size_t o_b = take(off, Bn * Rp * d), o_s = take(off, Bn * d), o_ld = take(off, Bn * d), o_n = take(off, Bn * sizeof(int)),
                 o_ct = miss ? take(off, Bn * (Rp * (Rp + 1) / 2) * d) : (size_t)-1, o_cf = take(off, B * Rp * Rp * d),
                 o_lf = take(off, B * d),
                 o_zp = (!fa.z_pred && fill) ? take(off, Bn * k * d) : (size_t)-1,
                 o_pp = (!fa.P_pred && fa.vstd) ? take(off, Bn * kk * d) : (size_t)-1,
                 o_zf = (!fa.z_filt && eval) ? take(off, Bn * k * d) : (size_t)-1,
                 o_acc = eval ? take(off, n_e * d) : (size_t)-1, o_acc0 = eval ? take(off, n_e * d) : (size_t)-1,
                 o_acn = eval ? take(off, n_e * sizeof(int)) : (size_t)-1;
    HIP_TRY(h, h->ft.grow(off));
    ca.B = fa.B; ca.T = fa.n; ca.N = fa.N;
    ca.bcol = at<double>(h->ft, o_b); ca.scol = at<double>(h->ft, o_s); ca.nobs = at<int>(h->ft, o_n); ca.ldrow = at<double>(h->ft, o_ld);
    ca.Ct = at<double>(h->ft, o_ct); ca.Cfull = at<double>(h->ft, o_cf); ca.ldfull = at<double>(h->ft, o_lf);
    ca.status = h->status_dev;
    fa.bcol = ca.bcol; fa.scol = ca.scol; fa.nobs = ca.nobs; fa.ldrow = ca.ldrow; fa.Ct = ca.Ct; fa.Cfull = ca.Cfull; fa.ldfull = ca.ldfull;
    if (!fa.z_pred) fa.z_pred = at<double>(h->ft, o_zp);
    if (!fa.P_pred) fa.P_pred = at<double>(h->ft, o_pp);
    if (!fa.z_filt) fa.z_filt = at<double>(h->ft, o_zf);
    fa.acc = at<double>(h->ft, o_acc); fa.acc0 = at<double>(h->ft, o_acc0); fa.acn = at<int>(h->ft, o_acn);
    fa.status = h->status_dev;
    return 0;
}

int dfm_filter_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, int t0, const double* panel,
                         const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, const double* mean, const double* sd, double* z_pred, double* P_pred,
                         double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr, double* vstd,
                         double* msfe, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = filter_check(h, B, T, N, r, p, H, t0, panel, Lam, R, Avar, Q, mu0, P0, mean, sd)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int Rp = pad_r(r);
    const size_t d = sizeof(double), rr = (size_t)Rp * Rp;
    const bool miss = (flags & DFM_F_MAY_HAVE_MISSING) != 0;
    const bool fill = xpred || verr || vstd, eval = H > 0 && (msfe || msfe0 || cnt);
    FtArgs fa{};
    fa.B = B; fa.n = T; fa.N = N; fa.r = r; fa.p = p; fa.k = r * p; fa.w = r; fa.Rp = Rp; fa.H = H; fa.t0 = t0;
    fa.panel = panel; fa.Lam = Lam; fa.R = R; fa.A = Avar; fa.Q = Q; fa.mu0 = mu0; fa.P0 = P0; fa.mean = mean; fa.sd = sd;
    fa.z_pred = z_pred; fa.P_pred = P_pred; fa.z_filt = z_filt; fa.P_filt = P_filt; fa.loglik_t = loglik_t;
    fa.xpred = xpred; fa.verr = verr; fa.vstd = vstd;
    fa.msfe = eval ? msfe : nullptr; fa.msfe0 = eval ? msfe0 : nullptr; fa.cnt = eval ? cnt : nullptr;
    size_t off = 0;
    const size_t o_lam = r != Rp ? take(off, (size_t)B * N * Rp * d) : (size_t)-1,
                 o_pad = r != Rp ? take(off, (3 * B * rr + (size_t)B * Rp) * d) : (size_t)-1;      // pad_params_kernel's other outputs (unused)
    CollapseArgs ca{};
    if (int rc = filter_carve(h, off, miss, fill, eval, ca, fa)) return rc;
    const double* LamP = Lam;
    if (r != Rp) {
        double* pad = at<double>(h->ft, o_pad);
        const size_t n = (size_t)B * N * Rp > B * rr ? (size_t)B * N * Rp : B * rr;
        ProfScope ps(h, K_PAD);
        // (A, Q, P0 and mu0 are read as if r wide -- in bounds of the caller's arrays, which are at least that large -- into `pad`)
        if (int rc = launch_1d(h, pad_params_kernel, n, B, N, r, Rp, Rp, Lam, Avar, Q, mu0, P0, at<double>(h->ft, o_lam), pad,
                               pad + B * rr, pad + 3 * B * rr, pad + 2 * B * rr)) return rc;
        LamP = at<double>(h->ft, o_lam);
    }
    ca.panel = panel; ca.Lam = LamP; ca.Rv = R;
    HIP_LAUNCH(h, K_COLLAPSE, launch_collapse(Rp, ca, h->stream));
    HIP_LAUNCH(h, K_FT_FILTER, launch_filter(fa, h->stream));
    if (fill) HIP_LAUNCH(h, K_FT_FILL, launch_filter_fill(fa, h->stream));
    if (eval) HIP_LAUNCH(h, K_FT_EVAL, launch_filter_eval(fa, h->stream));
    return 0;
}

int dfm_filter_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, int t0, const double* panel,
                     const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                     const double* P0, const double* mean, const double* sd, double* z_pred, double* P_pred,
                     double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr, double* vstd,
                     double* msfe, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = filter_check(h, B, T, N, r, p, H, t0, panel, Lam, R, Avar, Q, mu0, P0, mean, sd)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * p, kk = k * (k + 1) / 2, BT = (size_t)B * T, n_x = BT * N, n_e = (size_t)B * H * N;
    if (H == 0) { msfe = nullptr; msfe0 = nullptr; cnt = nullptr; }          // (left untouched)
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *zp_d, *pp_d, *zf_d, *pf_d, *ll_d, *xp_d, *ve_d, *vs_d, *m_d, *m0_d;
    int* cnt_d;
    st.in(panel, n_x, x_d);
    stage_model(st, md, B, N, r, p, 0, Lam, R, nullptr, Avar, Q, mu0, P0, nullptr, mean, sd);
    st.out(z_pred, z_pred ? BT * k : 0, zp_d); st.out(P_pred, P_pred ? BT * kk : 0, pp_d);
    st.out(z_filt, z_filt ? BT * k : 0, zf_d); st.out(P_filt, P_filt ? BT * kk : 0, pf_d);
    st.out(loglik_t, loglik_t ? BT : 0, ll_d);
    st.out(xpred, xpred ? n_x : 0, xp_d); st.out(verr, verr ? n_x : 0, ve_d); st.out(vstd, vstd ? n_x : 0, vs_d);
    st.out(msfe, msfe ? n_e : 0, m_d); st.out(msfe0, msfe0 ? n_e : 0, m0_d); st.out(cnt, cnt ? n_e : 0, cnt_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_filter_batch_dev(h, B, T, N, r, p, H, t0, x_d, md.Lam, md.R, md.A, md.Q, md.mu0, md.P0, md.mean, md.sd, zp_d, pp_d,
                                            zf_d, pf_d, ll_d, xp_d, ve_d, vs_d, m_d, m0_d, cnt_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}

// ---- the same for the model with AR idiosyncratic terms (filter_ar.hip) -----------------------------------------------------------
// As ar_pass_run prepares its pass: quasi_diff_kernel and ar_loadings_kernel (loadings on q + 1 lag blocks, pad_r(k) wide: the width
// of the AR pass's plan) into h->ft, collapse_kernel at that width on the quasi-differenced panel, then filter_ar_kernel and, for the
// outputs the caller takes, filter_ar_fill_kernel and filter_ar_eval_kernel -- both read the panel itself.
static int filter_ar_check(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, int t0, const double* panel,
                           const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                           const double* mu0, const double* P0, const double* mean, const double* sd) {
    if (int rc = check_dims(h, B, T, N, r)) return rc;
    if (H < 0) return fail(h, DFM_E_DIMS, "H must be >= 0%s");
    if (p < 1) return fail(h, DFM_E_DIMS, "number of factor lags must be >= 1%s");
    if (q < 1) return fail(h, DFM_E_DIMS, "number of idiosyncratic lags must be >= 1 (q = 0 is dfm_filter_batch)%s");
    if (T <= q) return fail(h, DFM_E_DIMS, "T must exceed the number of idiosyncratic lags%s");
    if (t0 < q || t0 >= T) return fail(h, DFM_E_DIMS, "t0 (the first origin) must lie in [q, T)%s");
    if (q > 4) return fail(h, DFM_E_R_UNSUPPORTED, "the filter with AR idiosyncratic terms needs q <= 4%s");
    if (int rc = ar_check(h, B, T, N, r, p, q, false)) return rc;
    if (!panel || !Lam || !sig2 || !rho || !Avar || !Q || !mu0 || !P0) return fail(h, DFM_E_NULL, "required pointer is NULL%s");
    if ((mean == nullptr) != (sd == nullptr)) return fail(h, DFM_E_NULL, "mean and sd must both be given or both be NULL%s");
    return 0;
}

int dfm_filter_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, int t0, const double* panel,
                            const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                            const double* mu0, const double* P0, const double* mean, const double* sd, double* z_pred,
                            double* P_pred, double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr,
                            double* vstd, double* msfe, double* msfe_common, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = filter_ar_check(h, B, T, N, r, p, q, H, t0, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int m = state_lags(p, q), k = r * m, w = r * (q + 1), Rp = pad_r(k), n = T - q;
    const size_t d = sizeof(double), Bn = (size_t)B * n;
    const bool miss = (flags & DFM_F_MAY_HAVE_MISSING) != 0;
    const bool fill = xpred || verr || vstd, eval = H > 0 && (msfe || msfe_common || msfe0 || cnt);
    FtArArgs fa{};
    fa.B = B; fa.n = n; fa.N = N; fa.r = r; fa.p = p; fa.q = q; fa.k = k; fa.w = w; fa.Rp = Rp; fa.H = H; fa.t0 = t0;
    fa.panel = panel; fa.Lam = Lam; fa.sig2 = sig2; fa.rho = rho; fa.A = Avar; fa.Q = Q; fa.mu0 = mu0; fa.P0 = P0; fa.mean = mean; fa.sd = sd;
    fa.z_pred = z_pred; fa.P_pred = P_pred; fa.z_filt = z_filt; fa.P_filt = P_filt; fa.loglik_t = loglik_t;
    fa.xpred = xpred; fa.verr = verr; fa.vstd = vstd;
    fa.msfe = eval ? msfe : nullptr; fa.msfe_common = eval ? msfe_common : nullptr; fa.msfe0 = eval ? msfe0 : nullptr;
    fa.cnt = eval ? cnt : nullptr;
    size_t off = 0;
    const size_t o_xq = take(off, Bn * N * d), o_lam = take(off, (size_t)B * N * Rp * d),
                 o_accc = eval ? take(off, (size_t)B * H * N * d) : (size_t)-1;
    CollapseArgs ca{};
    if (int rc = filter_carve(h, off, miss, fill, eval, ca, fa)) return rc;
    fa.accc = at<double>(h->ft, o_accc);
    double* xq = at<double>(h->ft, o_xq);
    double* LamK = at<double>(h->ft, o_lam);
    if (int rc = launch_1d(h, quasi_diff_kernel, Bn * N, B, T, N, q, panel, rho, xq)) return rc;
    if (int rc = launch_1d(h, ar_loadings_kernel, (size_t)B * N * Rp, B, N, r, q, Rp, Lam, rho, LamK)) return rc;
    ca.panel = xq; ca.Lam = LamK; ca.Rv = sig2;
    ca.kreal = w;                                               // (the loadings' columns w .. Rp - 1 are zero: as enqueue_pass at kdim)
    HIP_LAUNCH(h, K_COLLAPSE, launch_collapse(Rp, ca, h->stream));
    HIP_LAUNCH(h, K_FTAR_FILTER, launch_filter_ar(fa, h->stream));
    if (fill) HIP_LAUNCH(h, K_FTAR_FILL, launch_filter_ar_fill(fa, h->stream));
    if (eval) HIP_LAUNCH(h, K_FTAR_EVAL, launch_filter_ar_eval(fa, h->stream));
    return 0;
}

int dfm_filter_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, int t0, const double* panel,
                        const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                        const double* mu0, const double* P0, const double* mean, const double* sd, double* z_pred,
                        double* P_pred, double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr,
                        double* vstd, double* msfe, double* msfe_common, double* msfe0, int* cnt, unsigned flags) {
    if (int rc = filter_ar_check(h, B, T, N, r, p, q, H, t0, panel, Lam, sig2, rho, Avar, Q, mu0, P0, mean, sd)) return rc;
    if (int rc = status_epoch(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t k = (size_t)r * state_lags(p, q), kk = k * (k + 1) / 2, Bn = (size_t)B * (T - q), n_x = Bn * N, n_e = (size_t)B * H * N;
    if (H == 0) { msfe = nullptr; msfe_common = nullptr; msfe0 = nullptr; cnt = nullptr; }          // (left untouched)
    HostStage st(h, 256);
    ModelDev md;
    double *x_d, *zp_d, *pp_d, *zf_d, *pf_d, *ll_d, *xp_d, *ve_d, *vs_d, *m_d, *mc_d, *m0_d;
    int* cnt_d;
    st.in(panel, (size_t)B * T * N, x_d);
    stage_model(st, md, B, N, r, p, q, Lam, sig2, rho, Avar, Q, mu0, P0, nullptr, mean, sd);   // (this entry takes no v0)
    st.out(z_pred, z_pred ? Bn * k : 0, zp_d); st.out(P_pred, P_pred ? Bn * kk : 0, pp_d);
    st.out(z_filt, z_filt ? Bn * k : 0, zf_d); st.out(P_filt, P_filt ? Bn * kk : 0, pf_d);
    st.out(loglik_t, loglik_t ? Bn : 0, ll_d);
    st.out(xpred, xpred ? n_x : 0, xp_d); st.out(verr, verr ? n_x : 0, ve_d); st.out(vstd, vstd ? n_x : 0, vs_d);
    st.out(msfe, msfe ? n_e : 0, m_d); st.out(msfe_common, msfe_common ? n_e : 0, mc_d); st.out(msfe0, msfe0 ? n_e : 0, m0_d);
    st.out(cnt, cnt ? n_e : 0, cnt_d);
    if (int rc = st.begin()) return rc;
    int rc = st.finish(dfm_filter_ar_batch_dev(h, B, T, N, r, p, q, H, t0, x_d, md.Lam, md.R, md.rho, md.A, md.Q, md.mu0, md.P0, md.mean, md.sd,
                                               zp_d, pp_d, zf_d, pf_d, ll_d, xp_d, ve_d, vs_d, m_d, mc_d, m0_d, cnt_d, flags));
    if (rc == 0) rc = status_check(h);
    return rc;
}
