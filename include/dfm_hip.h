/* include/dfm_hip.h -- C-ABI of libdfmhip.so: MI355X (gfx950) batched Kalman filter / RTS smoother /
 * EM for the dynamic factor model of QuantEcon/dynamic_factor_models.
 *
 * What it replaces in the reference.  The reference has NO FFI and NO parametric estimator: it
 * declares the dispatch tag `struct Parametric <: EstimationMethod end` (dfm_functions.ipynb:21-23),
 * writes the state-space form y_t = Q z_t, z_t = M z_{t-1} + G u_t (dfm_functions.ipynb:30-34,
 * matrices filled at :477-492) and implements only `estimate!(m, ::NonParametric)` (:530-543).
 * The entry points below are what a new method `estimate!(m::DFMModel, ::Parametric; ...)` binds
 * with `ccall` (binding shown in INTEGRATION.md / julia/dfm_hip.jl).  Each entry point cites the
 * reference object whose role it fills.
 *
 * Conventions
 *   - all arithmetic and storage: IEEE fp64; integers only for sizes / indices
 *   - panel[b][t][i]  (i fastest; the reference stores T x ns column-major per model,
 *                      dfm_functions.ipynb:89-111 `data`; the Julia shim permutes once)
 *     NaN = missing cell (the reference's `missing`, dfm_functions.ipynb:155-158)
 *   - Lam[b][i][k] (= `lambda`, ns x r, dfm_functions.ipynb:104), R[b][i] (idiosyncratic variance;
 *     the reference keeps `uar_ser`, :106), A[b][r][r] row-major (= VAR(1) block of `M`, :477-492),
 *     Q[b][r][r] (= `seps`, :57 / G G'), mu0[b][r], P0[b][r][r]
 *   - packed symmetric outputs: lower triangle, row-major: idx(i,j) = i(i+1)/2 + j, j <= i
 *   - every function returns an int status: 0 ok; <0 argument error (DFM_E_*); >0 = hipError_t.
 *     No C++ exception or exit() crosses the boundary; dfm_last_error() gives the text.
 *   - "_dev" entry points take DEVICE pointers and only enqueue work on the handle's stream
 *     (asynchronous; inputs must stay valid until the stream is synchronised).  The plain entry
 *     points take HOST pointers, copy in, run, copy out and synchronise (what Julia's ccall binds).
 *   - the caller owns every buffer passed in; the library owns its workspace inside the handle.
 *   - requires Q and P0 positive definite (information-form recursion), 1 <= r <= DFM_MAX_R.
 */
#ifndef DFM_HIP_H
#define DFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFM_MAX_R 32

enum {
    DFM_OK = 0,
    DFM_E_DIMS = -1,          /* B,T,N,r out of range */
    DFM_E_R_UNSUPPORTED = -2, /* r > DFM_MAX_R */
    DFM_E_NULL = -3,          /* required pointer is NULL */
    DFM_E_MISSING = -4,       /* NaN found in the panel but DFM_F_MAY_HAVE_MISSING not set */
    DFM_E_NUMERIC = -5,       /* non-finite log-likelihood in some replicate (non-PD Q/P0/...) */
    DFM_E_NO_DEVICE = -6,     /* no HIP device / extension not usable */
    DFM_E_COMM = -7,          /* multi-GPU entry points: RCCL could not be loaded or a collective failed */
    DFM_E_VINTAGE = -8,       /* dfm_news_batch: a cell observed in the old vintage is missing in the new one */
    DFM_E_WINDOW = -9         /* dfm_rolling_eval_batch: a series of a window has too few visible cells, or they are all equal */
};

/* flags */
#define DFM_F_MAY_HAVE_MISSING 1u /* panel may contain NaN: allocate the per-period C_t workspace */
#define DFM_F_SINGULAR_Q 2u       /* Q (state innovation covariance) may be singular or ill-conditioned: run the
                                   * recursion in covariance form (never inverts Q; P0 must still be positive
                                   * definite).  Slower than the default information form; balanced panels lose the
                                   * time-parallel fast path. */
#define DFM_SV_UNIT_EFFECT 4u     /* dfm_irf_batch: unit-effect normalisation of the impulse responses (needs `named`) */

typedef struct dfm_handle dfm_handle;

/* Create a context bound to HIP device `device_id`.  `stream` is a hipStream_t the caller owns
 * (e.g. torch's current stream) or NULL for a stream created and owned by the handle. */
int dfm_create(dfm_handle** h, int device_id, void* stream);
int dfm_destroy(dfm_handle* h);
int dfm_set_stream(dfm_handle* h, void* stream);
/* dfm_synchronize: wait for the handle's stream, THEN read the handle's status word -- DFM_E_MISSING (NaN in a panel that
 * was declared balanced), DFM_E_NUMERIC (a bounded wait inside the one-launch pass ran out: outputs invalid; PCA start not
 * converged).  The word is STICKY: kernels only ever set bits, and the call that reads a non-zero value reports it once and
 * clears it -- so it covers every call enqueued since the previous check (no per-call reset: that was a fill kernel in front
 * of every pass).  The "_dev" entry points only enqueue, so this is where a device-pointer caller learns that a call went
 * wrong; the host-pointer entry points make the same check themselves -- and open a new EPOCH when they start: they read and
 * clear the word at entry, so what they report at the end is their own kernels' (a bit left by an earlier unchecked "_dev" call
 * is discarded there; dfm_last_error is left alone -- the call has not failed).  dfm_check_status is the same call under the name a reader looks for. */
int dfm_synchronize(dfm_handle* h);
int dfm_check_status(dfm_handle* h);
const char* dfm_last_error(const dfm_handle* h);
const char* dfm_version(void);

/* Per-kernel timing with HIP events recorded on the handle's stream around every kernel launch
 * (bench.py's roofline leg; no reference counterpart).  dfm_profile_enable(h, 1) clears and starts,
 * dfm_profile_read synchronises and returns the summed duration and launch count of kernel
 * `kernel_index` (0 .. until it returns DFM_E_DIMS) together with its name. */
int dfm_profile_enable(dfm_handle* h, int on);
int dfm_profile_read(dfm_handle* h, int kernel_index, char* name_out, int name_cap, double* total_ms,
                     int* launches);

/* dfm_hbm_probe: the streaming ceilings of the handle's device measured on the spot with the pass's own access patterns
 * (bench.py reports them beside the 8 TB/s spec peak; no reference counterpart).  mode 0: read-only LDS-DMA ring
 * (global_load_lds_dwordx4 -- the collapse's pattern); 1: 16-byte copy (read + write bytes both counted); 2: write-only.
 * `bytes` >= 16 MB of device memory are allocated for the call and freed; `iters` back-to-back launches are timed with HIP
 * events.  *gbs = GB/s, *ms_per_launch may be NULL. */
int dfm_hbm_probe(dfm_handle* h, size_t bytes, int mode, int iters, double* gbs, double* ms_per_launch);

/* dfm_chunk_fallbacks: diagnostics of the last pass / EM iteration with missing cells that ran on a time-chunked recursion
 * (r <= 8: csrc/recursion_chunk.hip, one chunk per lane; 17 <= r <= 31: the chunks of recursion_tile_kernel, one workgroup each,
 * csrc/recursion_tile.hip; no reference counterpart).  *n_total = replicates of that launch (0: the last call did not use one),
 * *n_failed = replicates whose chunk boundaries did not agree to the tolerance and were redone by the sequential kernel.
 * Synchronises the handle's stream. */
int dfm_chunk_fallbacks(dfm_handle* h, int* n_failed, int* n_total);

/* Bytes of device workspace the handle will hold for a pass / EM call on a (B,T,N,r) problem with these flags (for
 * capacity planning; the larger of the sequential and -- for balanced panels -- the time-parallel plan).  The VAR(p),
 * AR-idiosyncratic, PCA and synthetic-panel entry points add their own scratch on top (a quasi-differenced panel copy,
 * [B][N][N] Gram matrices, ...).  Environment switches are read at this call: the figure is that of a handle created now
 * (a handle keeps the switches of its own creation). */
size_t dfm_workspace_bytes(int B, int T, int N, int r, unsigned flags);

/* --- one full Kalman-smoother pass per replicate (SURVEY.md §8(d) "pass") ---------------------
 * Fills the slot of the reference's unused `Parametric` estimator: E-step at fixed parameters.
 * Outputs: f_smooth[b][t][k] = E[f_t | X] (what the reference stores in `factor`,
 * dfm_functions.ipynb:103), P_smooth[b][t][r(r+1)/2] = Var[f_t | X] packed (may be NULL),
 * loglik[b] = Gaussian log-likelihood of the replicate's observed cells. */
int dfm_ks_pass_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel,
                          const double* Lam, const double* R, const double* A, const double* Q,
                          const double* mu0, const double* P0, double* f_smooth, double* P_smooth,
                          double* loglik, unsigned flags);
int dfm_ks_pass_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel,
                      const double* Lam, const double* R, const double* A, const double* Q,
                      const double* mu0, const double* P0, double* f_smooth, double* P_smooth,
                      double* loglik, unsigned flags);

/* --- EM (Shumway-Stoffer / Banbura-Modugno) ------------------------------------------------------
 * One EM iteration per replicate, parameters updated IN PLACE (device pointers); loglik[b] is the
 * log-likelihood at the parameters passed in.  The role of the reference's per-series OLS
 * (dfm_functions.ipynb:391-415) and factor VAR OLS (:444-468) in the non-parametric path. */
int dfm_em_step_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel,
                          double* Lam, double* R, double* A, double* Q, double* mu0, double* P0,
                          double* loglik, unsigned flags);
/* max_iter EM iterations; loglik_path[b][k] = log-likelihood at the parameters entering iteration
 * k (NaN for k >= iters[b]); a replicate stops after iteration k >= 1 when
 * (ll_k - ll_{k-1}) / (0.5 (|ll_k| + |ll_{k-1}|)) < tol (tol <= 0: run all iterations); iters[b] =
 * iterations run.  A replicate that stops this way keeps the parameters that ENTERED its last
 * iteration (that M-step is discarded), exactly as oracle/kalman_oracle.py em().  Afterwards
 * f_smooth/P_smooth (may be NULL) hold the smoother output of the last E-step that was run.
 * Host-pointer variant copies parameters in and out. */
int dfm_em_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam,
                     double* R, double* A, double* Q, double* mu0, double* P0, int max_iter,
                     double tol, double* loglik_path, int* iters, double* f_smooth,
                     double* P_smooth, unsigned flags);
int dfm_em_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam,
                 double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol,
                 double* loglik_path, int* iters, double* f_smooth, double* P_smooth,
                 unsigned flags);

/* EM iteration number k (0-based) of max_iter with the bookkeeping of dfm_em_batch_dev kept in CALLER-owned device
 * arrays that persist between calls: loglik_path [B][max_iter] and iters [B] (both initialised by the k = 0 call) and
 * active [B] (written by every call: 1 while the replicate keeps iterating).  dfm_em_batch_dev is this call for k = 0,
 * 1, ... until no replicate of its batch is active; a multi-GPU driver (replicates sharded over the
 * GPUs, no data-path collective) calls it on every shard, all-gathers {loglik_path[:, k], active} -- north_star's
 * "single allgather at the end of each EM iteration" -- and stops when no replicate ANYWHERE is active:
 * dynamic_factor_models_amd/shard.py em_batch_sharded (one process per GPU, torch.distributed over RCCL) and
 * dfm_em_batch_multi below (one process, one host thread per GPU).  f_smooth / P_smooth (may be NULL) receive the
 * smoother output of this iteration's E-step. */
int dfm_em_iterate_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam, double* R,
                             double* A, double* Q, double* mu0, double* P0, int k, int max_iter, double tol,
                             double* loglik_path, int* iters, int* active, double* f_smooth, double* P_smooth,
                             unsigned flags);

/* --- the same operations on SEVERAL GPUs of one node from ONE process (a library-owned object with
 * `ngpu`, `device_ids`, per-GPU handles / streams / workspaces and ONE RCCL communicator; what
 * `estimate!(m, ::Parametric; nrep, ngpu)` of julia/dfm_hip.jl binds -- Julia has no torch.distributed).
 * GPU g of ngpu owns replicates [g B / ngpu, (g+1) B / ngpu) of a job (the partition of shard.py replicate_range); no
 * data-path collective.  One host thread per GPU inside a call; after every EM iteration ONE ncclAllGather of {loglik,
 * active} ([ceil(B/ngpu)][2] doubles per GPU) over xGMI gives every thread the global convergence state, and all GPUs stop
 * at the same iteration.
 *
 * dfm_multi_create: device_ids[ngpu] (NULL: 0 .. ngpu-1) must be distinct.  The communicator (ncclCommInitAll) is created
 * here, once, when ngpu > 1 or DFM_MULTI_F_FORCE_COMM is set (a 1-rank communicator: the exchange path of the EM loop then
 * runs -- and is tested -- on a single GPU); RCCL is bound with dlopen at that moment (DFM_E_COMM if it cannot be).
 * The replicates of a job live ON THE DEVICES between calls ("resident" job):
 *   dfm_multi_load   uploads host arrays (layouts of dfm_em_batch) to their owners;
 *   dfm_multi_synth  generates them where they live -- GPU g calls dfm_synth_panels_dev with first_replicate + lo_g, so
 *                    BASELINE configs[2] (65 536 replicates, 52 GB of panels) never crosses PCIe; pca_start != 0 replaces
 *                    the DGP parameters by the PCA + OLS start (dfm_pca_init_batch_dev; balanced panels only);
 *   dfm_multi_ks_pass / dfm_multi_em  run on the resident job (EM updates the resident parameters in place);
 *   dfm_multi_fetch  copies one resident array of the whole job back to the host, in global replicate order. */
typedef struct dfm_multi dfm_multi;
#define DFM_MULTI_F_FORCE_COMM 1u
enum {  /* dfm_multi_fetch `what`; element type double unless noted */
    DFM_MULTI_LAM = 0, DFM_MULTI_R, DFM_MULTI_A, DFM_MULTI_Q, DFM_MULTI_MU0, DFM_MULTI_P0,
    DFM_MULTI_F_SMOOTH,    /* [B][T][r]         of the last pass / last E-step */
    DFM_MULTI_P_SMOOTH,    /* [B][T][r(r+1)/2]  (only when the last call asked for it) */
    DFM_MULTI_LOGLIK,      /* [B]               of the last dfm_multi_ks_pass */
    DFM_MULTI_LOGLIK_PATH, /* [B][max_iter]     of the last dfm_multi_em */
    DFM_MULTI_ITERS,       /* int [B]           of the last dfm_multi_em */
    DFM_MULTI_PANEL        /* [B][T][N] */
};
int dfm_multi_create(dfm_multi** m, int ngpu, const int* device_ids, unsigned mflags, char* err, int err_cap);
int dfm_multi_destroy(dfm_multi* m);
int dfm_multi_ngpu(const dfm_multi* m);
int dfm_multi_has_comm(const dfm_multi* m);          /* 1 when the object owns an RCCL communicator */
const char* dfm_multi_last_error(const dfm_multi* m);
int dfm_multi_load(dfm_multi* m, int B, int T, int N, int r, const double* panel, const double* Lam, const double* R,
                   const double* A, const double* Q, const double* mu0, const double* P0);
int dfm_multi_synth(dfm_multi* m, uint64_t seed, int64_t first_replicate, int B, int T, int N, int r,
                    double missing_prob, int pca_start);
/* One smoother pass of every resident replicate (want_P: also P_smooth).  Synchronises every GPU. */
int dfm_multi_ks_pass(dfm_multi* m, int want_P, unsigned flags);
/* The EM loop of dfm_em_batch on the resident job: per iteration dfm_em_iterate_batch_dev on every shard, then the
 * all-gather; *iterations_run (may be NULL) = iterations every GPU ran.  want_smooth: keep f_smooth (and, with want_P,
 * P_smooth) of the last E-step resident for dfm_multi_fetch. */
int dfm_multi_em(dfm_multi* m, int max_iter, double tol, int want_smooth, int want_P, unsigned flags,
                 int* iterations_run);
int dfm_multi_fetch(dfm_multi* m, int what, void* dst);

/* Handle-less forms (round-2 ABI, kept): create + load + run + fetch + destroy in one call.  HOST pointers, layouts as
 * dfm_em_batch / dfm_ks_pass_batch; err[err_cap] (may be NULL) receives the message of the first failing GPU. */
int dfm_em_batch_multi(int ngpu, const int* device_ids, int B, int T, int N, int r, const double* panel, double* Lam,
                       double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol,
                       double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags,
                       int* iterations_run, char* err, int err_cap);
int dfm_ks_pass_batch_multi(int ngpu, const int* device_ids, int B, int T, int N, int r, const double* panel,
                            const double* Lam, const double* R, const double* A, const double* Q, const double* mu0,
                            const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags,
                            char* err, int err_cap);

/* --- VAR(p) factor dynamics ------------------------------------------------------
 *   x_t = Lam f_t + e_t,   f_t = A_1 f_{t-1} + ... + A_p f_{t-p} + eta_t,  eta_t ~ N(0, Q)
 * the parametric model with the reference's `n_factorlag` lags (DFMModel, dfm_functions.ipynb:120-146), run in the
 * companion form its `fill_matrices!` builds for the factor VAR (dfm_functions.ipynb:477-492): state
 * z_t = (f_t, .., f_{t-p+1}), k = r p <= DFM_MAX_R, transition [A_1 .. A_p; I 0], innovation covariance [Q 0; 0 0]
 * (singular: covariance-form recursion, as with DFM_F_SINGULAR_Q).
 *   Avar [B][r][r p] = [A_1 .. A_p],  Q [B][r][r],  mu0 [B][r p], P0 [B][r p][r p] = moments of z_0 (P0 positive definite)
 * Q itself (the r x r block) positive definite, or pass DFM_F_SINGULAR_Q: at r = 4 the companion recursion eliminates the state
 * in 4 x 4 blocks and inverts that block (recursion_comp.hip; a block that is not positive definite gives a NaN log-likelihood =
 * DFM_E_NUMERIC); with the flag the kernels that never invert it run instead (slower at r = 4).  Same for dfm_*_ar_*.
 * Outputs as dfm_ks_pass_batch / dfm_em_batch, for f_t = z_t[:r].  The M-step re-estimates Lam, R, [A_1..A_p], Q,
 * mu0, P0 and keeps the companion structure (oracle/varp_oracle.py).  p = 1 is dfm_em_batch's model. */
int dfm_ks_pass_varp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel,
                               const double* Lam, const double* R, const double* Avar, const double* Q,
                               const double* mu0, const double* P0, double* f_smooth, double* P_smooth,
                               double* loglik, unsigned flags);
int dfm_ks_pass_varp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel,
                           const double* Lam, const double* R, const double* Avar, const double* Q,
                           const double* mu0, const double* P0, double* f_smooth, double* P_smooth,
                           double* loglik, unsigned flags);
int dfm_em_varp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, double* Lam,
                          double* R, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                          double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);
int dfm_em_varp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, double* Lam,
                      double* R, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                      double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);

/* --- nowcasts and forecasts of the panel from a fitted model ------------------------------------------------------------
 * The model of dfm_ks_pass_batch (p = 1) / dfm_ks_pass_varp_batch (p >= 1); every moment conditions on the replicate's observed
 * cells X (T rows), output rows t = 0 .. T+H-1, rows T .. the forecast horizon (H >= 0; H = 0 is a pure nowcast):
 *   f_out[b][t]  = E[f_t | X]   (t < T: the smoothed factors; t >= T: the forecast f_{t|T})               [B][T+H][r]
 *   P_out[b][t]  = Var[f_t | X] packed lower (may be NULL)                                               [B][T+H][r(r+1)/2]
 *   common[b][t][i] = mean_i + sd_i lam_i' f_out[t]                                   (may be NULL)      [B][T+H][N]
 *   xhat[b][t][i]   = mean_i + sd_i x_ti on an observed cell (bit for bit x_ti when mean / sd are NULL); on a missing cell
 *                     and for t >= T: mean_i + sd_i lam_i' f_out[t]                                      [B][T+H][N]
 *   xvar[b][t][i]   = exactly 0 on an observed cell, else sd_i^2 (lam_i' P_out[t] lam_i + R_i)   (may be NULL)  [B][T+H][N]
 *   loglik[b]       = log-likelihood of the observed cells, as the plain pass on the T-row panel    (may be NULL)
 * Inputs: panel [B][T][N] (NaN = missing), Lam [B][N][r], R [B][N], Avar [B][r][r p] = [A_1 .. A_p], Q [B][r][r],
 * mu0 [B][r p], P0 [B][r p][r p]; mean / sd [B][N] (both or neither; what dfm_standardize_batch_dev returns) put the outputs
 * back into data units.  Flags as the pass (DFM_F_MAY_HAVE_MISSING, DFM_F_SINGULAR_Q: a NaN panel without the first gives
 * DFM_E_MISSING); a shape the underlying pass refuses gives that pass's status; H < 0: DFM_E_DIMS.  Outputs must not overlap the
 * inputs.  p = 1 runs the plain pass on the T-row panel and extends its terminal moments (f <- A f, P <- A P A' + Q); p > 1 writes
 * the panel with H all-missing rows into xhat and runs the companion pass on it as a (T+H)-row panel with missing cells. */
int dfm_forecast_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel,
                           const double* Lam, const double* R, const double* Avar, const double* Q,
                           const double* mu0, const double* P0, const double* mean, const double* sd,
                           double* xhat, double* xvar, double* common, double* f_out, double* P_out,
                           double* loglik, unsigned flags);
int dfm_forecast_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel,
                       const double* Lam, const double* R, const double* Avar, const double* Q,
                       const double* mu0, const double* P0, const double* mean, const double* sd,
                       double* xhat, double* xvar, double* common, double* f_out, double* P_out,
                       double* loglik, unsigned flags);

/* --- posterior draws of factor and panel paths: simulation smoother (Durbin and Koopman 2002) ---------------------------
 * The model of dfm_forecast_batch: x_t = Lam f_t + e_t, e_t ~ N(0, diag R), f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t,
 * eta_t ~ N(0, Q), z_0 = (f_0, .., f_{1-p}) ~ N(mu0, P0).  For replicate b, each draw d = 0 .. D-1 is an exact, independent draw of
 * (f_1 .. f_{T+H}, the missing and future cells of x) given the observed cells of X (T rows; H >= 0 horizon rows):
 *   1. z+_0 ~ N(mu0, P0); f+_t = sum_j A_j f+_{t-j} + eta+_t (t = 1..T); x+_ti = lam_i' f+_t + sqrt(R_i) eps+_ti
 *   2. D_ti = X_ti - x+_ti on observed cells, NaN where X is NaN
 *   3. g = E[f_{1:T} | D] by the pass of dfm_ks_pass_batch (p = 1) / dfm_ks_pass_varp_batch with the caller's parameters and mu0 = 0
 *   4. f_draw[b][d][t] = f+_t + g_t for rows t < T                                                                 [B][D][T+H][r]
 *   5. rows t >= T: f_t = sum_j A_j f_{t-j} + eta_t with fresh eta (needs T >= p)
 *   6. x_draw[b][d][t][i] = mean_i + sd_i X_ti on an observed cell (bit for bit X_ti when mean / sd are NULL); on a missing cell
 *      and for t >= T: mean_i + sd_i (lam_i' f_t + sqrt(R_i) eps_ti)                              (may be NULL)   [B][D][T+H][N]
 * Inputs as dfm_forecast_batch.  The random stream is part of the contract: Philox4x32-10 (counter lo = idx, hi = stream word),
 * Box-Muller on two 53-bit uniforms (as dfm_synth_panels_dev), key = seed ^ (0x9E3779B97F4A7C15 * (first_draw + d + 1)),
 * stream word 16 b + s, element c = component c mod 2 of the pair at idx; t = 0-based output row:
 *   s = 1: z+_0 = mu0 + L_P0 n,         idx = c / 2,                            c = 0 .. r p - 1
 *   s = 2: eta of row t = L_Q n,        idx = t ceil(r / 2) + k / 2,   c = k,   t = 0 .. T+H-1 (eta+ for t < T)
 *   s = 3: eps+ of the difference,      idx = t ceil(N / 2) + i / 2,   c = i,   t < T
 *   s = 4: eps of the drawn cells,      idx = t ceil(N / 2) + i / 2,   c = i
 * L_P0, L_Q: lower Cholesky roots, a column whose pivot is <= 1e-12 trace is zero (so Q may be singular with DFM_F_SINGULAR_Q).
 * Draws [k, k + D) of a call equal the draws of a call with first_draw = k.  Flags as the pass (a NaN panel needs
 * DFM_F_MAY_HAVE_MISSING, else DFM_E_MISSING).  Status: D < 1, H < 0, T < p: DFM_E_DIMS; f_draw NULL: DFM_E_NULL; mean without sd
 * or sd without mean: DFM_E_NULL; a shape the pass refuses: its status; a non-finite pass: DFM_E_NUMERIC (host entry).  Outputs
 * must not overlap the inputs.  Allocates in the handle (kept for the next call): the roots [B], the pass parameters and
 * smoothed means of one slice of at most 8192 pass replicates, and (x_draw NULL) that slice's [S][T][N] difference panels; with
 * x_draw they live at the start of the slice's part of x_draw, which the fill then overwrites. */
int dfm_simsmooth_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel,
                            const double* Lam, const double* R, const double* Avar, const double* Q,
                            const double* mu0, const double* P0, const double* mean, const double* sd,
                            uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags);
int dfm_simsmooth_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int H, const double* panel,
                        const double* Lam, const double* R, const double* Avar, const double* Q,
                        const double* mu0, const double* P0, const double* mean, const double* sd,
                        uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags);

/* --- Bayesian estimation: a batched Gibbs sampler ---------------------------------------------------------------------------
 * The model, shapes and flags of dfm_simsmooth_batch (x_t = Lam f_t + e_t, e ~ N(0, diag R); VAR(p) factors with innovation
 * covariance Q; NaN = missing; r p <= DFM_MAX_R); B independent chains.  mu0 [B][r p] and P0 [B][r p][r p] are inputs and stay
 * fixed; the VAR block conditions on the first p drawn rows.  No stationarity truncation and no rotation or scale normalisation
 * is applied: the posterior is proper through the priors, and the common component Lam f, R, forecasts and named-factor IRFs
 * are well defined without one; Lam, A and Q individually are not identified.
 * Priors (scalars per call, except A0 [B][r][r p], NULL = 0): lam_i | R_i ~ N(0, R_i / tau_lam I); R_i ~ IG(nu_R / 2, nu_R s_R / 2);
 * vec(A') | Q ~ N(vec(A0'), Q (x) I / tau_A); Q ~ IW(s_Q I, nu_Q).  tau_lam, s_R, tau_A, s_Q > 0, nu_R >= 2, nu_Q >= r + 1.
 * Lam [B][N][r], R [B][N], Avar [B][r][r p], Q [B][r][r] are the chain state: the start on entry, the state after the last sweep
 * on return.  Sweep j = 0 .. n_sweeps-1 of chain b, key = seed ^ (0x9E3779B97F4A7C15 * (first_sweep + j + 1)), stream word 16 b + s:
 *   1. f_1 .. f_T | X, state: dfm_simsmooth_batch_dev with D = 1, H = 0, first_draw = first_sweep + j (streams 1-4)
 *   2. for series i over its observed rows O_i (n_i of them): S = tau_lam I + sum f f' = L L', m = S^-1 sum f x,
 *      R_i = (nu_R s_R + sum x^2 - m' S m) / 2 / g, g ~ Gamma((nu_R + n_i) / 2, 1) from stream 6 (item i of N);
 *      lam_i = m + sqrt(R_i) L^-T n, n = r normals of stream 5: idx = i ceil(r / 2) + k / 2, component k mod 2.  n_i = 0: the prior.
 *   3. Y = rows p .. T-1 of f, Z their p lags (n = T - p rows): S = tau_A I + Z'Z = L L', M = S^-1 (tau_A A0' + Z'Y),
 *      Psi = s_Q I + Y'Y + tau_A A0 A0' - M' S M = C C'; B_T lower triangular with B_T[j][j] = sqrt(2 Gamma((nu_Q + n - j) / 2))
 *      from stream 9 (item j of r) and, below the diagonal, normals of stream 8: entry (j, c), c < j, is component e mod 2 of idx e / 2,
 *      e = j (j - 1) / 2 + c;  G = C B_T^-T, Q = G G';  A' = M + L^-T E G', E [r p][r] normals of stream 7: idx = row ceil(r / 2) + k / 2.
 * Gamma(a, 1), a >= 1, by Marsaglia and Tsang (2000): attempt k = 0, 1, .. of item i of n_items uses m = k n_items + i:
 * z = first normal of the pair at idx 2 m, u = the 53-bit uniform at idx 2 m + 1 (as dfm_synth_panels_dev's R), d = a - 1/3,
 * c = 1 / sqrt(9 d), v = (1 + c z)^3; accepted when v > 0 and log u < z^2 / 2 + d - d v + d log v; the draw is d v.  32 rejected
 * attempts raise a status bit (DFM_E_NUMERIC), as does a failed Cholesky (every Cholesky of the sampler fails on a pivot
 * <= 1e-12 trace, the rule of dfm_simsmooth_batch's roots, with or without DFM_F_MAY_HAVE_MISSING); a draw whose Cholesky failed leaves that part of the
 * chain's state (lam_i and R_i of the series; A and Q) as it was, so a failure does not turn into NaN cells of later sweeps.
 * Sweep j is kept when j >= burn and (j - burn) % thin == 0; K kept sweeps go to Lam_draw [B][K][N][r], R_draw [B][K][N],
 * A_draw [B][K][r][r p], Q_draw [B][K][r][r], f_draw [B][K][T][r] (each may be NULL).  A call of n sweeps with first_sweep = k from
 * the state k sweeps left equals the tail of one call of k + n sweeps bit for bit, and two runs agree bit for bit (no atomics
 * on floating point).  Status: n_sweeps < 1, thin < 1, burn < 0, T <= p or a prior outside its condition: DFM_E_DIMS; a NULL
 * panel, mu0, P0 or state: DFM_E_NULL; a shape the pass refuses: its status; a NaN panel without DFM_F_MAY_HAVE_MISSING:
 * DFM_E_MISSING, a failed Cholesky or the gamma cap: DFM_E_NUMERIC (status-word bits: the host entry reports them,
 * dfm_check_status after the "_dev" entry).  The sweeps are enqueued on the handle's stream without a wait between them.
 * Allocates in the handle (kept for the next call): one [B][T][r] factor path and [B][r][r] roots, beside what
 * dfm_simsmooth_batch_dev keeps. */
int dfm_gibbs_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* mu0,
                        const double* P0, double* Lam, double* R, double* Avar, double* Q, double tau_lam, double nu_R,
                        double s_R, double tau_A, double nu_Q, double s_Q, const double* A0, int n_sweeps, int burn, int thin,
                        uint64_t seed, int64_t first_sweep, double* Lam_draw, double* R_draw, double* A_draw, double* Q_draw,
                        double* f_draw, unsigned flags);
int dfm_gibbs_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* mu0,
                    const double* P0, double* Lam, double* R, double* Avar, double* Q, double tau_lam, double nu_R,
                    double s_R, double tau_A, double nu_Q, double s_Q, const double* A0, int n_sweeps, int burn, int thin,
                    uint64_t seed, int64_t first_sweep, double* Lam_draw, double* R_draw, double* A_draw, double* Q_draw,
                    double* f_draw, unsigned flags);

/* --- news decomposition of nowcast revisions (Banbura and Modugno 2014) -------------------------------------------------------
 * The model and conventions of dfm_forecast_batch; two vintages old / new [B][T][N] of the same standardised panel (a period the
 * old vintage did not have is all-NaN there).  Omega_old, Omega_new = their observed cells; Omega_old must be a subset of
 * Omega_new.  Targets g = 0 .. G-1: cells (target_t[g], target_i[g]), 0 <= t* < T + H, 0 <= i* < N, shared by every replicate; H
 * = max(0, max t* + 1 - T) is derived from them.  A target is y = E[x_t*i* | Omega] in data units (xhat of dfm_forecast_batch):
 *   yhat[b][0][g] = y conditioned on old, yhat[b][1][g] on the REVISED old panel (new values on Omega_old, NaN elsewhere),
 *   yhat[b][2][g] on new; yhat[1] - yhat[0] is the data-revision effect                                         [B][3][G]
 *   news[b][t][i]  = I_ti = x_new_ti - E[x_ti | revised old] (data units) on the news cells Omega_new \ Omega_old, 0 elsewhere
 *                                                                                                    (may be NULL) [B][T][N]
 *   weight[b][g][t][i] = w = d y_new / d x_ti on Omega_new (data units: sd_i* / sd_i times the standardised weight), 0 on its
 *                    missing cells; restricted to the news cells these are the news weights Cov(y, I) Var(I)^-1  (may be NULL)
 *                                                                                                                [B][G][T][N]
 *   impact[b][g][i] = sum over the news cells of series i of w I; sum_i impact = yhat[2] - yhat[1] exactly    [B][G][N]
 * The weights come from one smoother pass per (b, g) instead of one per news cell: with Sigma = Var(z on Omega_new) and
 * c = Cov(z_Omega_new, y_z), w = Sigma^-1 c, and x - Lam E_0[f | x] = R Sigma^-1 x (E_0: prior mean 0).  So c is written as a
 * panel on the Omega_new mask (c_ti = lam_i' Cov(f_t+1, f_t*+1) lam_i*, plus R_i* on the target cell when it is observed), the
 * pass of dfm_ks_pass_batch (p = 1) / dfm_ks_pass_varp_batch runs on it with mu0 = 0 and the caller's flags, and
 * w_ti = (sd_i* / sd_i) (c_ti - lam_i' g_t) / R_i.  Inputs as dfm_forecast_batch; target_t / target_i [G] are HOST arrays in
 * both entries (the horizon and the scratch depend on them).  Flags as the pass: the new panel and the covariance panels run
 * with the caller's flags (a NaN in new without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING), the old and revised old panels always
 * with DFM_F_MAY_HAVE_MISSING.  Status: G < 1 or a target outside [0, T + H) x [0, N): DFM_E_DIMS; a NULL required pointer,
 * mean without sd or sd without mean: DFM_E_NULL; Omega_old not a subset of Omega_new: DFM_E_VINTAGE (a status-word bit: the
 * host entry reports it, dfm_check_status after the "_dev" entry); a shape the pass refuses: its status; a non-finite pass:
 * DFM_E_NUMERIC (host entry).  Outputs must not overlap the inputs.  Allocates in the handle (kept for the next call): the
 * revised old panel and one forecast's [B][T+H][N] xhat, and per slice of at most 8192 pass replicates the pass parameters,
 * [S][T][r p] + 2 [S][T][r] vectors and (weight NULL) the [S][T][N] covariance panels; with weight they live in the slice's
 * part of weight, which the impacts overwrite.  Out of scope: re-estimation between vintages (one parameter set), a per-cell
 * split of the data-revision effect. */
int dfm_news_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* old_panel, const double* new_panel,
                       const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                       const double* P0, const double* mean, const double* sd, int G, const int* target_t,
                       const int* target_i, double* yhat, double* impact, double* news, double* weight, unsigned flags);
int dfm_news_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* old_panel, const double* new_panel,
                   const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                   const double* P0, const double* mean, const double* sd, int G, const int* target_t,
                   const int* target_i, double* yhat, double* impact, double* news, double* weight, unsigned flags);

/* --- news decomposition with AR(q) idiosyncratic terms -------------------------------------------------------------------------
 * The same question for the model, symbols and output-row convention of dfm_forecast_ar_batch (below): 1 <= q <= 4, the output
 * rows are panel rows q .. T + H - 1, n_s = T - q of them in the sample; v0, mean, sd as in that call.  Vintages and targets as in
 * dfm_news_batch: old / new [B][T][N], targets (target_t[g], target_i[g]) in PANEL rows with q <= t* < T + H, H derived from them.
 *   yhat[b][w][g]   = xhat of dfm_forecast_ar_batch at the target, conditioned on old (w = 0), revised old (1), new (2)  [B][3][G]
 *   news[b][t][i]   = I = x_new - E[x | revised old] on the news cells of output row t, 0 elsewhere      (may be NULL) [B][T-q][N]
 *   weight[b][g][t][i] = d y_new / d x on the cells of new in output row t (data units), 0 elsewhere     (may be NULL) [B][G][T-q][N]
 *   impact[b][g][i] = sum_t w I of series i; sum_i impact = yhat[2] - yhat[1]                                          [B][G][N]
 * The first q panel rows are conditioning values: the model is that of the cells behind them given them.  A revision there moves
 * yhat[1] - yhat[0] and carries no weight.
 * Both vintages must be EDGE-SHAPED: in every replicate and series the observed panel rows are exactly 0 .. L_i, with
 * L_i >= 2 q - 1 in old (hence in new, since every cell of old must be observed in new).  Anything else -- an interior gap, a late
 * start, a series with fewer than 2 q observed rows or none -- is DFM_E_VINTAGE (the status-word bit of dfm_news_batch: the host
 * entry reports it, dfm_check_status after the "_dev" entry), because the decomposition would not add up: the AR pass
 * quasi-differences one interior NaN into q + 1 NaN rows, so its factor estimate is no projection on the observed cells, and
 * y_new - y_rev - sum w I was measured at up to 4.5e-2 on revisions of 6e-2 with a single interior gap; a series with fewer than
 * q observed output rows brings v0 in and leaves 1e-8 .. 1e-6.  On edge-shaped vintages the identity holds to rounding.
 * The weights come from one pass per (b, g): the covariance of every quasi-differenced cell with the target is written as a panel
 * (NaN where the quasi-differenced new vintage is NaN), the inner part of the AR pass runs on it with mu0 = 0 and the caller's
 * flags, and the adjoint of the quasi-difference turns its residuals into weights.
 * Status: q < 1, T <= 2 q, G < 1, a target outside [q, T + H) x [0, N): DFM_E_DIMS; q > 4 and what dfm_ks_pass_ar_batch refuses
 * at T + H rows: DFM_E_R_UNSUPPORTED / its status; a NULL required pointer, mean without sd: DFM_E_NULL; a NaN in new without
 * DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING; a non-finite pass: DFM_E_NUMERIC (host entry).  target_t / target_i are HOST arrays in
 * both entries.  Outputs must not overlap the inputs.  Allocates in the handle as dfm_news_batch does, per slice of at most 8192
 * pass replicates.  Out of scope: vintages that are not edge-shaped, re-estimation between vintages, exact xvar, q > 4. */
int dfm_news_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* old_panel,
                          const double* new_panel, const double* Lam, const double* sig2, const double* rho, const double* Avar,
                          const double* Q, const double* mu0, const double* P0, const double* v0, const double* mean,
                          const double* sd, int G, const int* target_t, const int* target_i, double* yhat, double* impact,
                          double* news, double* weight, unsigned flags);
int dfm_news_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* old_panel, const double* new_panel,
                      const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                      const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd, int G,
                      const int* target_t, const int* target_i, double* yhat, double* impact, double* news, double* weight,
                      unsigned flags);

/* --- structural IRFs, variance and historical decompositions of the panel ---------------------------------------------------
 * The model of dfm_forecast_batch: x_t = Lam f_t + e_t, f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t, Var eta = Q, with
 * 1 <= r p <= DFM_MAX_R.  The structural shocks are eta_t = S u_t with Var u = I.
 * Identification: named-factor normalisation plus Cholesky ordering.  `named` is a HOST int[r] of distinct series indices shared
 * by every replicate, as the news targets are; it may be NULL.  With Ln = Lam[named, :] (r x r): S = Ln^-1 chol(Ln Q Ln').
 * Factor k then *is* the common component of series named[k]; the order of `named` is the recursive ordering.  With named = NULL:
 * S = chol(Q).  chol is the lower root with the zero-column rule of dfm_simsmooth_batch: a pivot <= 1e-12 trace gives a zero
 * column.  Ln is factored with partial pivoting; a pivot <= 1e-12 max|Ln| in any replicate raises a status bit, which the host
 * entry reports as DFM_E_NUMERIC (dfm_check_status after the "_dev" entry).  With `named` the outputs do not change under
 * Lam -> Lam M^-1, A_j -> M A_j M^-1, Q -> M Q M': that invariance is the point.
 * Responses: Theta_h = Psi_h S for h = 0 .. H-1, from the companion recursion; Theta^c_h = sum_{j<=h} Theta_j.  `cum` is a HOST
 * int[N] that may be NULL; cum[i] != 0 means series i entered in differences and its outputs are cumulated.  sd [B][N] may be
 * NULL; it puts the IRF and the historical decomposition into data units (no mean is involved).
 *
 * dfm_irf_batch: inputs Lam [B][N][r], Avar [B][r][r p], Q [B][r][r], R [B][N] (needed with fevd), sd, named, cum; no panel, no
 * pass.
 *   irf[b][k][h][i]  = sd_i lam_i' Theta_h e_k, with Theta^c_h where cum[i]                                       [B][r][H][N]
 *     flag DFM_SV_UNIT_EFFECT (needs named, else DFM_E_NULL) divides column k by the impact response of series named[k] in
 *     output units; that response is then exactly 1 at h = 0.  It scales the IRF only.
 *   fevd[b][k][h][i] (may be NULL), always from the unit-variance shocks:                                         [B][r+1][H][N]
 *     num_k = sum_{j<=h} (lam_i' Theta_j e_k)^2, cumulated responses where cum[i]; idio = R_i, or (h+1) R_i where cum[i];
 *     fevd[k] = num_k / (sum_k num_k + idio); slot k = r is the idiosyncratic share; the r+1 slots sum to 1.
 *   Status: H < 1 or a named entry out of range or repeated: DFM_E_DIMS; a NULL required pointer: DFM_E_NULL;
 *   r p > DFM_MAX_R: DFM_E_R_UNSUPPORTED.  Sizes are checked before the handle.  A rank-deficient Q is accepted (zero column).
 *
 * dfm_histdecomp_batch: inputs as dfm_forecast_batch without H and mean, plus named.
 *   1. the smoother pass of dfm_ks_pass_batch_dev (p = 1) / dfm_ks_pass_varp_batch_dev with the caller's flags and without
 *      P_smooth, exactly as dfm_forecast_batch_dev calls it
 *   2. for t >= p: etahat_t = f_t|T - sum_j A_j f_{t-j|T} and u_t = S^-1 etahat_t; with named that is L*^-1 Ln etahat_t by forward
 *      substitution (L* = chol(Ln Q Ln')).  A zero pivot gives the status bit and DFM_E_NUMERIC, so this entry needs Q positive
 *      definite.  Rows t < p carry no shock.
 *   3. contribution paths c^(k)_t = sum_j A_j c^(k)_{t-j} + S e_k u_{k,t} from zero, for k < r; slot k = r is the initial
 *      condition: c^(r)_t = f_t|T for t < p, then the shock-free recursion
 *   4. hd[b][k][t][i] = sd_i lam_i' c^(k)_t, every cell whether observed or not; the r+1 slots sum to sd_i lam_i' f_t|T
 *                                                                                                                 [B][r+1][T][N]
 *   5. optional outputs (may be NULL): shocks [B][T][r] (u_t, zero rows for t < p), f_out [B][T][r], loglik [B]
 *   6. Status: T < p + 1: DFM_E_DIMS; the rest as the pass.
 * Both allocate in the handle (kept for the next call): S, S^-1, the Theta tables [B][H][r][r], the contribution paths
 * [B][r+1][T][r] and whatever optional output the caller does not take.  Outputs must not overlap the inputs. */
int dfm_irf_batch_dev(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar,
                      const double* Q, const double* R, const double* sd, const int* named, const int* cum, double* irf,
                      double* fevd, unsigned flags);
int dfm_irf_batch(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                  const double* R, const double* sd, const int* named, const int* cum, double* irf, double* fevd,
                  unsigned flags);
int dfm_histdecomp_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                             const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                             const double* sd, const int* named, double* hd, double* shocks, double* f_out, double* loglik,
                             unsigned flags);
int dfm_histdecomp_batch(dfm_handle* h, int B, int T, int N, int r, int p, const double* panel, const double* Lam,
                         const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                         const double* sd, const int* named, double* hd, double* shocks, double* f_out, double* loglik,
                         unsigned flags);

/* --- sign-restricted structural IRFs: batched rotation draws -------------------------------------------------------------------
 * The model, `named`, `cum`, `sd`, the base impact matrix S and the tables Theta_h = Psi_h S are those of dfm_irf_batch, with
 * 1 <= r p <= DFM_MAX_R: S = chol(Q), or Ln^-1 chol(Ln Q Ln') with `named`.  Every S Rot with Rot orthogonal has S Rot (S Rot)' =
 * S S' and is an impact matrix too; M candidate rotations per replicate are drawn uniformly (Haar), those whose responses carry
 * the required signs are accepted, and the first K accepted ones of every replicate are kept and written out.
 *
 * Restrictions: `restr` is a HOST int[G][5] shared by every replicate, row g = (series i, shock k, h0, h1, sign) with
 * 0 <= i < N, 0 <= k < r, 0 <= h0 <= h1 < H, sign = +1 or -1.  Row g asks that sign * resp_i,k(h) > 0 for every h0 <= h <= h1,
 * resp being the response as it is output (cumulated where cum[i]).  G = 0 is allowed: every candidate is then accepted (but
 * for the pivot rule of step 4).
 *
 * Candidate m of replicate b, m = 0 .. M-1:
 *   1. key = seed ^ (0x9E3779B97F4A7C15 * (first_cand + m + 1)), the key of dfm_simsmooth_batch, with stream word 16 b + 10
 *      (streams 1-9 are taken).
 *   2. Z [r][r] of standard normals: entry e = row r + col is component e mod 2 of the pair at index e / 2 (normal2, as the
 *      other streams use it).
 *   3. Rot = the orthogonal factor of Z = Rot U with U upper triangular and a POSITIVE diagonal.  That factor is unique and is
 *      the Haar draw.  (The library: Gram-Schmidt by columns, every column orthogonalised twice.)
 *   4. A pivot |U_jj| <= 1e-12 max|Z| rejects the candidate.
 *   5. For every shock column k that has restrictions: if all its rows hold the column stays; if all its rows hold with every
 *      sign reversed the column is flipped (Rot e_k -> -Rot e_k); otherwise the candidate is rejected.  Columns without
 *      restrictions are never flipped.
 *   6. The impact matrix of an accepted candidate is S_m = S Rot D, D the diagonal of flips.
 * A candidate's result is a pure function of (seed, first_cand + m, b) and the inputs: it depends on neither M, K nor the launch
 * geometry, and candidates [k, k + M) of one call equal those of a call with first_cand = k.
 *
 * Outputs ("slot" s = 0 .. K-1 of replicate b holds its s-th accepted candidate, in candidate order):
 *   n_accept [B] int32            accepted among the M candidates
 *   mask_out [B][M] int32         1 accepted, 0 not (may be NULL)
 *   cand_out [B][K] int32         candidate index m (into mask_out) of the first min(K, n_accept[b]) accepted candidates; -1 behind
 *   S_out [B][K][r][r]            S_m of the kept slots (may be NULL)
 *   irf [B][K][r][H][N]           sd_i lam_i' Psi_h S_m e_k, cumulated where cum[i] (may be NULL): what dfm_irf_batch with
 *                                 named = NULL gives for the rotated set (Lam S_m, S_m^-1 A_j S_m, I)
 *   fevd [B][K][r+1][H][N]        dfm_irf_batch's definition with Theta_h Rot D in place of Theta_h (may be NULL; needs R)
 * Empty slots hold NaN in every double output.
 * Status: sizes and `restr` are checked before the handle.  H < 1, M < 1, K < 1, G < 0, a restr entry out of range, a named entry
 * out of range or repeated: DFM_E_DIMS; G > 0 with restr NULL, n_accept or cand_out NULL, a NULL input: DFM_E_NULL; r p >
 * DFM_MAX_R: DFM_E_R_UNSUPPORTED.  DFM_SV_UNIT_EFFECT is refused with DFM_E_NULL, the code that flag gets without named series:
 * a rotated shock has no named series to normalise on.  A singular Ln gives status bit 16 and DFM_E_NUMERIC, as dfm_irf_batch.
 * A rank-deficient Q is accepted.  The per-replicate table of restricted responses (the r-vectors sd_i lam_i' Theta_h of the
 * distinct restricted series i and h <= max h1) lives in LDS: (distinct restricted series) x (max h1 + 1) x r x 8 bytes must not
 * exceed 48 KB (49152), else DFM_E_DIMS.  B M and B K must be < 2^31 (DFM_E_DIMS).
 * Allocates in the handle (kept for the next call): S, the Theta tables, the mask when mask_out is NULL, one r x r rotation per
 * candidate ([B][M][r][r]) and the kept slots' tables [B][K][H][r][r].  Outputs must not overlap the inputs. */
int dfm_signirf_batch_dev(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar,
                          const double* Q, const double* R, const double* sd, const int* named, const int* cum, int G,
                          const int* restr, int M, int K, uint64_t seed, int64_t first_cand, int* n_accept, int* mask_out,
                          int* cand_out, double* S_out, double* irf, double* fevd, unsigned flags);
int dfm_signirf_batch(dfm_handle* h, int B, int N, int r, int p, int H, const double* Lam, const double* Avar, const double* Q,
                      const double* R, const double* sd, const int* named, const int* cum, int G, const int* restr, int M,
                      int K, uint64_t seed, int64_t first_cand, int* n_accept, int* mask_out, int* cand_out, double* S_out,
                      double* irf, double* fevd, unsigned flags);

/* --- structural IRFs identified by an external instrument (proxy SVAR): batched block draws ---------------------------------------
 * The model, sd, cum and the smoother pass are those of dfm_histdecomp_batch, with 1 <= r p <= DFM_MAX_R and Q positive definite.
 * An instrument z_t is correlated with ONE structural shock and with none of the others; the covariance of the factor-VAR
 * innovations with z_t then is that shock's impact column up to scale.  No ordering, no named series, no rotation search.  The
 * sampling error of the instrument moment is judged by a moving block bootstrap of the used rows (D draws of block length L per
 * replicate); parameter uncertainty is the replicate axis.
 *
 * Inputs: panel [B][T][N], Lam, R, Avar, Q, mu0, P0, sd (may be NULL) and cum (HOST int[N], may be NULL) as dfm_histdecomp_batch /
 * dfm_irf_batch.  z: HOST double[T] in both entries, shared by every replicate as cum is; NaN = not available in that period.
 * norm: series index, 0 <= norm < N; the identified shock is signed so that the impact response of series norm is non-negative.
 * D >= 0 block draws per replicate, L the block length, seed, first_draw >= 0.
 *
 * Replicate b:
 *   1. the smoother pass exactly as dfm_histdecomp_batch_dev calls it (caller's flags, no P_smooth)
 *   2. for t >= p: etahat_t = f_t|T - sum_j A_j f_{t-j|T}
 *   3. used rows U = {t : p <= t < T, z_t finite} in increasing order, n = |U| (the same for every replicate)
 *   4. slots s = 0 .. D.  Slot 0 is the sample itself: src(j) = U[j], j = 0 .. n-1.  Slot 1 + d is block draw g = first_draw + d:
 *      key = seed ^ (0x9E3779B97F4A7C15 * (g + 1)), the key of dfm_simsmooth_batch, stream word 16 b + 11 (streams 1-10 are
 *      taken); nb = ceil(n / L) blocks; block k takes component k mod 4 of Philox::block(key, k / 4, stream) as a 32-bit word w;
 *      its start is s_k = (uint64(w) * (n - L + 1)) >> 32 (integer arithmetic); src(j) = U[s_{j / L} + j mod L], the last block cut
 *      at n.  A draw is a pure function of (seed, g, b), the inputs and L: it depends on neither D nor the launch geometry, and
 *      draws [k, k + D) of one call equal those of a call with first_draw = k.
 *   5. moments of a slot: zbar = (1/n) sum_j z_src(j); m = (1/n) sum_j etahat_src(j) (z_src(j) - zbar), an r-vector;
 *      v = (1/n) sum_j (z_src(j) - zbar)^2
 *   6. impact vector: gq = Q^-1 m through the Cholesky root of Q (a pivot <= 1e-12 trace raises status bit 16, which the host
 *      entry reports as DFM_E_NUMERIC, as dfm_histdecomp_batch does); kappa = m' gq.  If kappa > 0 is false every output of the
 *      slot is NaN.  Otherwise hvec = m / sqrt(kappa), so that hvec' Q^-1 hvec = 1: the one-standard-deviation shock.  hvec is
 *      replaced by -hvec where lam_norm' hvec < 0.
 *        impact [B][D+1][r] = hvec;  rel [B][D+1] = kappa / v (under the model's Q the squared correlation of the instrument with
 *        the identified shock)
 *   7. responses, h = 0 .. H-1:
 *        irf [B][D+1][H][N] = sd_i lam_i' Psi_h hvec, with Psi^c_h = sum_{j<=h} Psi_j where cum[i].  Flag DFM_SV_UNIT_EFFECT divides
 *          the slot by the impact response of series norm in output units (a true division: that response is exactly 1 at
 *          h = 0); a zero impact response gives a NaN slot of irf.
 *        fevd [B][D+1][H][N] = num / (den + idio), always from the unit-variance shock: num = sum_{j<=h} (lam_i' Psi_j hvec)^2,
 *          den = sum_{j<=h} lam_i' Psi_j Q Psi_j' lam_i (dfm_irf_batch's sum_k num_k, since S S' = Q), idio as in dfm_irf_batch;
 *          cumulated forms where cum[i]
 *      Each of irf and fevd may be NULL.
 *   8. shock [B][T] (may be NULL): slot 0's series u_t = hvec' Q^-1 etahat_t for t >= p, zero before
 *   9. f_out [B][T][r] and loglik [B] are optional, as in dfm_histdecomp_batch
 * Invariance: under Lam -> Lam M^-1, A_j -> M A_j M^-1, Q -> M Q M', mu0 -> M mu0, P0 -> M P0 M' (blockwise for the companion
 * state) impact -> M impact, f_out -> f_out M', and rel, irf, fevd, shock do not change: the answer does not depend on the
 * rotation the fit sits in.
 * Status: sizes, norm and z are checked before the handle.  H < 1, T < p + 1, D < 0, first_draw < 0, norm out of range, n < r + 2,
 * L < 1, L > n, B (D + 1) >= 2^31: DFM_E_DIMS; a NULL required pointer (impact and rel are required): DFM_E_NULL; r p > DFM_MAX_R:
 * DFM_E_R_UNSUPPORTED; the rest as the pass.
 * Allocates in the handle (kept for the next call): S, S^-1, the Theta tables, the row table [B][n][r+1], one r-vector and (with irf
 * or fevd) one [H][r] table per slot, with fevd a [B][H][N] table, and the pass outputs the caller does not take.
 * dfm_workspace_bytes does not count them.  Outputs must not overlap the inputs. */
int dfm_proxyirf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0,
                           const double* sd, const int* cum, const double* z, int norm, int D, int L, uint64_t seed,
                           int64_t first_draw, double* impact, double* rel, double* irf, double* fevd, double* shock,
                           double* f_out, double* loglik, unsigned flags);
int dfm_proxyirf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, const double* panel, const double* Lam,
                       const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, const double* sd,
                       const int* cum, const double* z, int norm, int D, int L, uint64_t seed, int64_t first_draw, double* impact,
                       double* rel, double* irf, double* fevd, double* shock, double* f_out, double* loglik, unsigned flags);

/* --- AR idiosyncratic terms --------------------------------------------------------
 *   x_it = lam_i' f_t + e_it,   e_it = rho_i1 e_i,t-1 + .. + rho_iq e_i,t-q + eps_it,  eps_it ~ N(0, sig2_i)
 * with rho [B][N][q] / sig2 [B][N] in the role of the reference's uar_coef / uar_ser^2 (AR(n_uarlag) of the loading
 * regression residuals, dfm_functions.ipynb:305-311, 405-412) and VAR(p) factor dynamics as above.  The panel is
 * quasi-differenced on the device (x~_it = x_it - sum_l rho_il x_i,t-l, missing when x_it or one of its q lags is), the
 * state is z_t = (f_t, .., f_{t-m+1}), m = max(p, q + 1), r m <= DFM_MAX_R, loadings [lam_i, -rho_i1 lam_i, ..]; the
 * likelihood is conditional on the first q rows.  mu0 [B][r m], P0 [B][r m][r m]: moments of z_q (P0 positive definite).
 * Outputs for the T - q rows q+1..T: f_smooth [B][T-q][r], P_smooth [B][T-q][r(r+1)/2] or NULL, loglik [B].
 * q = 0 is dfm_ks_pass_varp_batch.  (Smoother pass only: rho / sig2 come from the reference's own estimator.) */
int dfm_ks_pass_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel,
                             const double* Lam, const double* sig2, const double* rho, const double* Avar,
                             const double* Q, const double* mu0, const double* P0, double* f_smooth,
                             double* P_smooth, double* loglik, unsigned flags);
int dfm_ks_pass_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel,
                         const double* Lam, const double* sig2, const double* rho, const double* Avar,
                         const double* Q, const double* mu0, const double* P0, double* f_smooth,
                         double* P_smooth, double* loglik, unsigned flags);

/* Joint estimation of the same model: loadings, AR coefficients (the reference's `uar_coef`, dfm_functions.ipynb:305-311,
 * 405-412), innovation variances (`uar_ser`^2), [A_1 .. A_p] and Q by ECM -- per iteration one smoother pass of the
 * quasi-differenced model at the current rho, the transition step (a VAR(p) inside the state of max(p, q + 1) lags), then
 * per series the loadings given rho, rho given the new loadings, and sig2 (all from the smoothed moments of the companion
 * state).  Every conditional step maximises its block of the expected complete-data likelihood, so loglik_path
 * [B][max_iter] (the likelihood conditional on the first q rows, at the parameters ENTERING each iteration) is
 * non-decreasing; bookkeeping (tol, iters) as dfm_em_batch.  Parameters are updated in place; rho [B][N][q]; mu0 / P0:
 * moments of the state at period q.  r <= 8, q <= 4, r * max(p, q + 1) <= 32; f_smooth / P_smooth (may be NULL): the
 * T - q smoothed rows of the last E-step.  Series with fewer than r + q + 1 usable quasi-differenced cells keep their
 * loadings / rho / sig2. */
int dfm_em_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, double* Lam,
                        double* sig2, double* rho, double* Avar, double* Q, double* mu0, double* P0, int max_iter,
                        double tol, double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);
int dfm_em_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, double* Lam,
                    double* sig2, double* rho, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                    double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);

/* Nowcasts and forecasts of the panel from the same model (csrc/forecast_ar.hip): dfm_forecast_batch with the idiosyncratic
 * persistence kept -- one to four steps ahead rho_i e_iT is often the larger part of a series' forecast.  Model, inputs and
 * conventions as dfm_ks_pass_ar_batch (1 <= q <= 4), mean / sd as dfm_forecast_batch.  Outputs have n = T + H - q rows, the panel
 * rows q .. T+H-1 (the AR pass's convention); the last H are the horizon (H >= 0).
 *   f_out [B][n][r], P_out [B][n][r(r+1)/2] (may be NULL), loglik [B] (may be NULL): what dfm_ks_pass_ar_batch gives on the panel
 *     with H all-missing rows appended, bit for bit (the smoothed moments of the empty rows are the forecast moments; the
 *     log-likelihood is conditional on the first q rows).
 *   On an observed cell of an output row u_it = x_it - lam_i' f_out[t] is an exact observation of e_it.  Per series the process e_i
 *   runs over the output rows, the q terms before row 0 are N(0, v0_i I_q) (v0 [B][N]; NULL: sig2_i), and ehat_it, V_it are the
 *   mean and variance of e_it given ALL residuals of series i (a scalar AR(q) smoother, missing cells and horizon included).  Panel
 *   rows < q inform the factors through the quasi-differences; they are not observations of this smoother.
 *   common[b][t][i] = mean_i + sd_i lam_i' f_out[t]                                                  (may be NULL)  [B][n][N]
 *   idio[b][t][i]   = sd_i ehat_it on a missing or horizon cell, sd_i u_it on an observed one            (may be NULL)  [B][n][N]
 *   xhat[b][t][i]   = mean_i + sd_i x_ti on an observed cell (bit for bit x_ti when mean / sd are NULL), else common + idio
 *   xvar[b][t][i]   = exactly 0 on an observed cell, else sd_i^2 (lam_i' P_out[t] lam_i + V_it)          (may be NULL)  [B][n][N]
 * xhat is the exact conditional mean E[x_ti | X]: the smoother is linear in the residuals, so E[e | X] is the smoother applied to
 * x - Lam E[f | X].  xvar IS NOT EXACT: it adds the two variances and leaves out the cross-period covariance of the factor
 * estimation error that enters through the residuals.  Against brute-force conditioning of the joint Gaussian, xvar / exact lay
 * between 0.967 and 1.018 over the horizon cells of four small balanced panels; the exact form needs lag-j
 * smoothed covariances.
 * Status: H < 0, q < 1, T <= q: DFM_E_DIMS; q > 4, or r max(p, q + 1) > DFM_MAX_R: DFM_E_R_UNSUPPORTED; a NULL required pointer
 * (xhat and f_out are required), mean without sd: DFM_E_NULL; a NaN in the panel without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING;
 * the rest as dfm_ks_pass_ar_batch on T + H rows.
 * Allocates in the handle (kept for the next call): the padded panel [B][T+H][N], P and loglik when the caller does not take them,
 * and the backward messages of one slice of replicates, q + q (q + 1) / 2 doubles per cell under a cap of 4 GiB
 * (DFM_FCAR_MSG_BYTES; one replicate's messages when they alone exceed it).  dfm_workspace_bytes does not count them.  Outputs must
 * not overlap the inputs. */
int dfm_forecast_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* panel,
                              const double* Lam, const double* sig2, const double* rho, const double* Avar,
                              const double* Q, const double* mu0, const double* P0, const double* v0, const double* mean,
                              const double* sd, double* xhat, double* xvar, double* common, double* idio, double* f_out,
                              double* P_out, double* loglik, unsigned flags);
int dfm_forecast_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, const double* panel,
                          const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                          const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                          double* xhat, double* xvar, double* common, double* idio, double* f_out, double* P_out,
                          double* loglik, unsigned flags);

/* Joint posterior draws of the factor path and of the panel's missing and horizon cells from the same model
 * (csrc/simsmooth_ar.hip): what dfm_simsmooth_batch is to dfm_forecast_batch, for dfm_forecast_ar_batch.  Inputs and conventions as
 * dfm_forecast_ar_batch, D draws per replicate; outputs have its n = T + H - q rows (panel rows q .. T+H-1).  m = max(p, q + 1),
 * k = r m.  Draw d of replicate b (simulation smoother of Durbin and Koopman 2002; every n below is a fresh N(0, 1)):
 *   1. State.  z+ = mu0 + L_P0 n: the state mu0 / P0 describe, lags f_{q-1} .. f_{q-m} in 0-based panel rows.
 *   2. Factor path.  f+_t = sum_j A_j f+_{t-j} + L_Q n_t for the n output rows, horizon included.
 *   3. Pre-sample terms, l = 1 .. q: e+_{q-l,i} = X_{q-l,i} - lam_i' f+_{q-l} where that panel cell is observed, sqrt(v0_i) n where it
 *      is missing (v0 NULL: sig2_i).
 *   4. Series path.  e+_ti = sum_l rho_il e+_{t-l,i} + sqrt(sig2_i) n_ti and x+_ti = lam_i' f+_t + e+_ti over the n output rows.
 *   5. Difference panel, T + H rows: rows < q are 0 where X is observed and NaN where it is not; rows q .. T-1 are X - x+ (NaN where
 *      X is NaN); the H horizon rows are NaN.
 *   6. Smoothed difference.  g, ehat* are what dfm_forecast_ar_batch computes on that panel with H = 0 extra rows, mu0 = 0 and the
 *      caller's other parameters and v0: the AR pass's f_smooth, and the per-series smoother's mean of the residuals D - lam' g.
 *   7. Outputs.  f_draw_t = f+_t + g_t                                                                              [B][D][n][r]
 *      x_draw (may be NULL) = mean_i + sd_i X_ti on an observed cell (bit for bit X_ti when mean / sd are NULL), and
 *      mean_i + sd_i (lam_i' f_draw_t + e+_ti + ehat*_ti) on every other cell                                       [B][D][n][N]
 * Exactness.  xhat of dfm_forecast_ar_batch is an affine map of the observed cells, so the draws are independent with mean xhat
 * and the joint covariance of xhat's error.  They are exact posterior draws on panels whose only missing cells are ragged-edge and
 * horizon cells, given rows 0 .. q-1 -- there the draws' variance is the exact form xvar of dfm_forecast_ar_batch leaves out.
 * With interior gaps they carry the pass's quasi-differencing convention (a quasi-difference is missing when any of its q + 1
 * cells is): mean and covariance are then those of xhat's error, not of the exact posterior.  Cells before a
 * series' first q consecutive observed output rows carry the v0 prior.
 * Random stream (part of the contract, as in dfm_simsmooth_batch): Philox4x32-10, Box-Muller on two 53-bit uniforms; key =
 * seed ^ (0x9E3779B97F4A7C15 (first_draw + d + 1)), stream word 16 b + s, element c of a pair is component c mod 2 at idx:
 *   s = 1  z+, idx = c / 2, c < k                     s = 2  eta of output row t, idx = t ceil(r/2) + c / 2
 *   s = 3  eps+ of output row t, idx = t ceil(N/2) + i / 2, c = i
 *   s = 5  pre-sample term l of series i, idx = (l - 1) ceil(N/2) + i / 2, c = i
 * Roots by the rule of dfm_simsmooth_batch (DFM_F_SINGULAR_Q works).  Draws [k, k + D) of a call equal those of a call with
 * first_draw = k.  An index depends on neither the missing cells nor the launch geometry nor the slicing.
 * Status: as dfm_forecast_ar_batch (f_draw in the place of xhat and f_out), plus D < 1: DFM_E_DIMS; B D >= 2^31: DFM_E_DIMS.
 * Allocates in the handle (kept for the next call): the roots and, for one slice of min(8192, DFM_FCAR_MSG_BYTES / one replicate's
 * messages) pass replicates (at least one), the pass parameters, g, the difference panels [T+H][N] and (x_draw) the backward
 * messages.  Results do not depend on the slicing.  Outputs must not overlap the inputs. */
int dfm_simsmooth_ar_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                               const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                               const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                               uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags);
int dfm_simsmooth_ar_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, int H, const double* panel,
                           const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                           const double* mu0, const double* P0, const double* v0, const double* mean, const double* sd,
                           uint64_t seed, int64_t first_draw, double* f_draw, double* x_draw, unsigned flags);

/* Panels simulated from a given model (csrc/simulate.hip): the parametric bootstrap's replicate panels, and Monte-Carlo panels in
 * general.  D draws per replicate b; the model, its parameters and their shapes are those of dfm_simsmooth_batch (plain) and
 * dfm_simsmooth_ar_batch (AR idiosyncratic terms; m = max(p, q + 1), mu0 [B][r m], P0 [B][r m][r m]).  No pass runs, so no N limit
 * of a pass applies: any N >= 1, and a state (r p, or r m) of at most DFM_MAX_R.
 * The random stream is part of the contract and is the smoothers': no new stream.
 *   dfm_simulate_batch.  x_sim[b][d] [T][N] is x+ of step 1 of dfm_simsmooth_batch for the same (seed, first_draw, b, d): z+_0 from
 *     stream 1, eta from stream 2, eps+ from stream 3, same key and same roots (a rank-deficient Q or P0 is fine).  A cell is NaN
 *     wherever mask_panel [B][T][N] is NaN; mask_panel is read for its NaN pattern only, and NULL means a balanced panel.
 *     f_sim [B][D][T][r] (may be NULL) is f+.
 *   dfm_simulate_ar_batch.  Rows q .. T-1 of x_sim[b][d] [T][N] are x+ of steps 1-4 of dfm_simsmooth_ar_batch with H = 0 (streams 1,
 *     2, 3 and 5; the pre-sample terms are X - lam' f+ where the panel cell is observed and sqrt(v0) n where it is not; v0 NULL:
 *     sig2), NaN where `panel` [B][T][N] is NaN.  Rows < q: with a panel, its own cells bit for bit (NaN stays NaN) -- a bootstrap
 *     conditional on the first q rows, which is what the likelihood of dfm_em_ar_batch conditions on; with panel NULL every cell is
 *     simulated: row q - l is lam_i' f+_{q-l} + e+_{q-l,i}, f+_{q-l} being lag block l - 1 of z+ and e+_{q-l,i} = sqrt(v0_i) n the
 *     pre-sample term l of stream 5.  f_sim [B][D][T-q][r] (may be NULL) is f+ of the output rows.
 * Draws [k, k + D) of a call equal the draws of a call with first_draw = k; an index depends on neither the mask nor the launch
 * geometry nor the slicing (at most 8192 pass replicates b D + d per launch of the path kernel).
 * Status: D < 1, T < p, T <= q, q outside 1..4, a state wider than DFM_MAX_R, B D >= 2^31: DFM_E_DIMS; x_sim or a parameter NULL:
 * DFM_E_NULL.  flags: none defined, pass 0.
 * Allocates in the handle (kept for the next call): the roots, Avar padded to m lags, and f+ [B D][rows][r] when f_sim is NULL.
 * Outputs must not overlap the inputs. */
int dfm_simulate_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, const double* mask_panel, const double* Lam,
                           const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, uint64_t seed,
                           int64_t first_draw, double* x_sim, double* f_sim, unsigned flags);
int dfm_simulate_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, const double* mask_panel, const double* Lam,
                       const double* R, const double* Avar, const double* Q, const double* mu0, const double* P0, uint64_t seed,
                       int64_t first_draw, double* x_sim, double* f_sim, unsigned flags);
int dfm_simulate_ar_batch_dev(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                              const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                              const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim,
                              unsigned flags);
int dfm_simulate_ar_batch(dfm_handle* h, int B, int D, int T, int N, int r, int p, int q, const double* panel, const double* Lam,
                          const double* sig2, const double* rho, const double* Avar, const double* Q, const double* mu0,
                          const double* P0, const double* v0, uint64_t seed, int64_t first_draw, double* x_sim, double* f_sim,
                          unsigned flags);

/* Bayesian estimation of the same model: a batched Gibbs sampler (csrc/gibbs_ar.hip), what dfm_gibbs_batch is to dfm_simsmooth_batch,
 * for dfm_simsmooth_ar_batch.  B independent chains; shapes, flags and m = max(p, q + 1) as dfm_ks_pass_ar_batch.  mu0 [B][r m] and
 * P0 [B][r m][r m] are inputs and stay fixed.  The chain state is Lam [B][N][r], sig2 [B][N], rho [B][N][q], Avar [B][r][r p],
 * Q [B][r][r]: the start on entry, the state after the last sweep on return.
 * Priors (scalars per call, except A0 [B][r][r p], NULL = 0): lam_i | sig2_i ~ N(0, sig2_i / tau_lam I); sig2_i ~ IG(nu_R / 2,
 * nu_R s_R / 2); rho_i ~ N(0, I / tau_rho) truncated to the stationary region (NOT scaled by sig2_i); vec(A') | Q ~ N(vec(A0'),
 * Q (x) I / tau_A); Q ~ IW(s_Q I, nu_Q).  tau_lam, s_R, tau_rho, tau_A, s_Q > 0, nu_R >= 2, nu_Q >= r + 1.
 * Sweep j = 0 .. n_sweeps-1 of chain b, key = seed ^ (0x9E3779B97F4A7C15 * (first_sweep + j + 1)), stream word 16 b + s.  Rows are
 * the n = T - q output rows (panel rows q .. T-1): X_t, F_t.  U_i = { t : q <= t < n, cells t, t-1, .. t-q of series i all observed }
 * (the AR pass's convention applied to the output rows), n_i = |U_i|.
 *   1. F = f_draw of dfm_simsmooth_ar_batch_dev with D = 1, H = 0, v0 / mean / sd / x_draw NULL, first_draw = first_sweep + j
 *      (streams 1, 2, 3, 5).
 *   2. rho_i | lam_i, sig2_i, F:  e_t = X_ti - lam_i' F_t, w_t = (e_t-1, .., e_t-q);  S = tau_rho I + sum_{U_i} w w' / sig2_i = L L',
 *      y = L^-1 sum_{U_i} w e_t / sig2_i.  A candidate is L^-T (y + n), n = q normals of stream 11: attempt k = 0, 1, .. of series i
 *      uses idx = (k N + i) ceil(q / 2) + l / 2, component l mod 2.  The first stationary candidate is the draw.  Stationarity is
 *      the step-down (Levinson) recursion: for k = q .. 1, kappa = phi_k; not stationary unless |kappa| < 1; then phi_j <-
 *      (phi_j + kappa phi_{k-j}) / (1 - kappa^2) for j < k.  32 rejected attempts raise a status bit (DFM_E_NUMERIC) and leave
 *      rho_i as it was.
 *   3. (sig2_i, lam_i) | rho_i, F with the new rho_i:  x~_t = X_t - sum_l rho_il X_t-l, f~_t = F_t - sum_l rho_il F_t-l over U_i;
 *      S = tau_lam I + sum f~ f~' = L L', y = L^-1 sum f~ x~;  sig2_i = (nu_R s_R + sum x~^2 - y'y) / 2 / g, g ~ Gamma((nu_R + n_i) / 2, 1)
 *      from stream 6 (item i of N);  lam_i = L^-T (y + sqrt(sig2_i) n), n = r normals of stream 10: idx = i ceil(r / 2) + k / 2,
 *      component k mod 2.  n_i = 0 gives the priors, in step 2 as well.
 *   4. A, Q | F: step 3 of dfm_gibbs_batch on the n rows of F (streams 7, 8, 9); it conditions on the first p drawn rows.
 * Stream 5 is NOT reused for the loadings: dfm_simsmooth_ar_batch spends it on the pre-sample terms with overlapping indices.
 * Gamma draws, their cap and the Cholesky rule (a pivot <= 1e-12 trace fails) as dfm_gibbs_batch: a failed block leaves its own
 * part of the series' state unchanged (rho_i; or lam_i and sig2_i; or A and Q) and raises the bit.
 * Approximations.  Steps 2-3 condition on the first q output rows of each series, as step 4 and dfm_gibbs_batch's VAR block
 * condition on the first p: the path step uses those q quasi-differences, the series step does not.  No stationarity truncation is
 * applied to A.  Lam, A and Q are not identified (no rotation or scale normalisation); rho, sig2, the common component and
 * forecasts are.  Interior gaps carry the pass's quasi-differencing convention (see dfm_simsmooth_ar_batch).
 * Sweep j is kept when j >= burn and (j - burn) % thin == 0; K kept sweeps go to Lam_draw [B][K][N][r], sig2_draw [B][K][N],
 * rho_draw [B][K][N][q], A_draw [B][K][r][r p], Q_draw [B][K][r][r], f_draw [B][K][n][r] (each may be NULL).  A call of n sweeps
 * with first_sweep = k from the state k sweeps left equals the tail of one call of k + n sweeps bit for bit, and two runs agree
 * bit for bit (no atomics on floating point; every sum runs over t in ascending order).
 * Status: n_sweeps < 1, thin < 1, burn < 0, q < 1, T - q <= p or a prior outside its condition: DFM_E_DIMS; q > 4, r > 8 or
 * r m > 32: DFM_E_R_UNSUPPORTED (the limits of dfm_em_ar_batch); a NULL panel, mu0, P0 or state: DFM_E_NULL; a NaN panel without
 * DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING; a failed Cholesky, the Gamma cap or the rho cap: DFM_E_NUMERIC (status-word bits: the host
 * entry reports them, dfm_check_status after the "_dev" entry).  The sweeps are enqueued on the handle's stream without a wait
 * between them.  Allocates in the handle (kept for the next call): one [B][n][r] factor path, beside what
 * dfm_simsmooth_ar_batch_dev keeps. */
int dfm_gibbs_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* mu0,
                           const double* P0, double* Lam, double* sig2, double* rho, double* Avar, double* Q, double tau_lam,
                           double nu_R, double s_R, double tau_rho, double tau_A, double nu_Q, double s_Q, const double* A0,
                           int n_sweeps, int burn, int thin, uint64_t seed, int64_t first_sweep, double* Lam_draw,
                           double* sig2_draw, double* rho_draw, double* A_draw, double* Q_draw, double* f_draw, unsigned flags);
int dfm_gibbs_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, const double* panel, const double* mu0,
                       const double* P0, double* Lam, double* sig2, double* rho, double* Avar, double* Q, double tau_lam,
                       double nu_R, double s_R, double tau_rho, double tau_A, double nu_Q, double s_Q, const double* A0,
                       int n_sweeps, int burn, int thin, uint64_t seed, int64_t first_sweep, double* Lam_draw,
                       double* sig2_draw, double* rho_draw, double* A_draw, double* Q_draw, double* f_draw, unsigned flags);

/* --- MIXED FREQUENCY: monthly factors, quarterly series (Mariano and Murasawa 2003; Banbura and Modugno 2014) ---------------
 *   x_it = lam_i' g_it + e_it,   g_it = sum_{l<L} w_il f_{t-l},   e_it ~ N(0, R_i),
 *   f_t  = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t,   eta_t ~ N(0, Q)
 * on a MONTHLY time index.  W [N][L] (one matrix for the whole batch) holds KNOWN aggregation weights: a monthly series has
 * (1, 0, ..), a quarterly growth rate (flow) (1, 2, 3, 2, 1) / 3, a quarterly average of a monthly level (1, 1, 1) / 3; any finite
 * W is legal, the library does not interpret it.  A quarterly series is NaN outside the third month of each quarter: ordinary
 * missing data.  The state is z_t = (f_t, .., f_{t-m+1}), m = max(p, L), loadings [w_i0 lam_i, .., w_i,L-1 lam_i, 0..], transition
 * of [A_1..A_p, 0], innovation covariance [Q 0; 0 0] -- the AR model above without quasi-differencing and without rho.
 * Lam [B][N][r], R [B][N], Avar [B][r][r p], Q [B][r][r], mu0 [B][r m], P0 [B][r m][r m] (moments of z_0, P0 positive definite);
 * f_smooth [B][T][r], P_smooth [B][T][r(r+1)/2] (or NULL): those of f_t = z_t[:r]; loglik [B].  L = 1, W = 1 is
 * dfm_ks_pass_varp_batch.  DFM_F_MAY_HAVE_MISSING / DFM_F_SINGULAR_Q as for dfm_*_varp_*.
 * Limits: 1 <= L <= 5 and finite weights (else DFM_E_DIMS), r max(p, L) <= DFM_MAX_R (else DFM_E_R_UNSUPPORTED), N as
 * dfm_*_ar_* for a state r max(p, L) wide (N <= 1024 up to 8, 512 up to 16, 256 beyond). */
int dfm_ks_pass_mf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, const double* Lam,
                             const double* R, const double* W, const double* Avar, const double* Q, const double* mu0,
                             const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags);
int dfm_ks_pass_mf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, const double* Lam,
                         const double* R, const double* W, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, double* f_smooth, double* P_smooth, double* loglik, unsigned flags);

/* Maximum likelihood of the same model by EM.  Per iteration: (1) the smoother pass of the expanded model; (2) the transition
 * step, a VAR(p) inside the state of m lags: [A_1..A_p] = S10[:r, :rp] S00[:rp, :rp]^-1, Q = (S11[:r,:r] - A S10[:r,:rp]') / T
 * symmetrised, mu0 / P0 = smoothed moments of z_0; (3) per series, over its n_i observed periods,
 *   G_i = sum_t E[g_it g_it'],  b_i = sum_t x_it E[g_it],  lam_i = G_i^-1 b_i,  R_i = (sum_t x_it^2 - 2 lam_i' b_i + lam_i' G_i lam_i) / n_i
 * with E[g_it] and E[g_it g_it'] read from the smoothed mean and covariance of z_t (L <= m: every lag is inside the state).  A
 * series with fewer than r + 1 observed cells keeps lam_i and R_i.  So does a series whose G_i is not positive definite (its
 * Cholesky factorisation meets a pivot <= 0: an all-zero weight row gives G_i = 0 exactly).  Parameters are updated in place;
 * loglik_path [B][max_iter]
 * (the likelihood at the parameters ENTERING each iteration, NaN past convergence, non-decreasing), iters and tol as
 * dfm_em_batch; f_smooth / P_smooth (may be NULL): the last E-step.  The distinct rows of W (compared exactly) are the weight
 * CLASSES; the aggregated moments are tabulated once per period and class, so a panel may hold at most 8 classes (else
 * DFM_E_DIMS; every use above has two or three).  Limits as the pass, and r <= 8 (else DFM_E_R_UNSUPPORTED).  W is read back
 * to the host once per call (the call synchronises the stream before its first launch). */
int dfm_em_mf_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                        const double* W, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                        double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);
int dfm_em_mf_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                    const double* W, double* Avar, double* Q, double* mu0, double* P0, int max_iter, double tol,
                    double* loglik_path, int* iters, double* f_smooth, double* P_smooth, unsigned flags);

/* The same EM with BLOCK-STRUCTURED loadings: some loadings are FIXED, the rest estimated (Banbura and Modugno 2014: a global
 * factor loads on every series, a "real" or "survey" factor on its own block only).  free_mask [N][r] (unsigned char, one matrix for
 * the whole batch; void* here so that every binding passes its byte array as it is): nonzero = estimated, zero = fixed.  A fixed loading keeps, bit for bit, the value it has in Lam on entry -- 0 for
 * a block structure, 1 for a normalisation -- in every replicate and iteration.  Steps (1) and (2) are those of dfm_em_mf_batch
 * (the factor VAR stays unrestricted over all r factors); in step (3), with F the free and X the fixed coordinates of series i,
 * k_i = |F|, and G_i, b_i as above,
 *   lam_F = G_FF^-1 (b_F - G_FX lam_X)  (Cholesky of G_FF),   R_i = (sum_t x_it^2 - 2 lam_i' b_i + lam_i' G_i lam_i) / n_i  (whole lam_i).
 * A series with n_i < k_i + 1 observed cells, or whose G_FF is not positive definite, keeps lam_i and R_i; a series with k_i = 0
 * and n_i >= 1 updates R_i only.  free_mask == NULL is dfm_em_mf_batch itself.  The _dev entry reads the mask on the device and
 * never copies it back.  Limits, flags and status codes are those of dfm_em_mf_batch. */
int dfm_em_mf_blocks_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                               const double* W, const void* free_mask, double* Avar, double* Q, double* mu0, double* P0,
                               int max_iter, double tol, double* loglik_path, int* iters, double* f_smooth, double* P_smooth,
                               unsigned flags);
int dfm_em_mf_blocks_batch(dfm_handle* h, int B, int T, int N, int r, int p, int L, const double* panel, double* Lam, double* R,
                           const double* W, const void* free_mask, double* Avar, double* Q, double* mu0, double* P0,
                           int max_iter, double tol, double* loglik_path, int* iters, double* f_smooth, double* P_smooth,
                           unsigned flags);

/* --- OBSERVED factors ------------------------------------------------------------------------------
 *   x_it = lam_o,i' g_t + lam_u,i' f_t + e_it,   e_it ~ N(0, R_i),     f_t = A f_{t-1} + eta_t,  eta_t ~ N(0, Q)
 * The reference's DFMModel has `nfac_o` observed factors in front of the `nfac_u` estimated ones (`factor` is T x nfac_t,
 * dfm_functions.ipynb:89-146; `lambda[:, nfac_o+1:end]` are the unobserved loadings, :364) but its estimator does not work for
 * nfac_o > 0 (:358-359, :371) -- the semantics here are those its data layout implies: g_t = the observed columns of `factor`
 * are KNOWN REGRESSORS of the measurement equation (FAVAR); their joint dynamics with f_t are the reference's own second
 * stage (`estimate_var!` on the whole `factor` matrix, :444-468).  EM: E-step = the ordinary pass on x - Lam_o g; loadings =
 * one joint regression per series on (g_t, f_t) over its observed periods; A, Q, mu0, P0 as dfm_em_batch (oracle/obs_oracle.py).
 * G [B][T][r_o] (no NaN), Lam [B][N][r_o + r_u] with the OBSERVED-factor loadings first, A / Q / P0 [B][r_u][r_u], mu0 [B][r_u];
 * f_smooth [B][T][r_u], P_smooth [B][T][r_u(r_u+1)/2] (may be NULL); bookkeeping (loglik_path, iters, tol) as dfm_em_batch.
 * r_o >= 1, r_u >= 1, r_o + r_u <= 32 (up to 8: a per-series Cholesky in registers; 9 .. 32: the ordinary loadings step on the
 * moments of z = (g, f), N <= 1024).  A series with fewer than r_o + r_u + 1 observed cells keeps its loadings and variance. */
int dfm_em_obs_batch_dev(dfm_handle* h, int B, int T, int N, int r_u, int r_o, const double* panel, const double* G, double* Lam,
                         double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                         int* iters, double* f_smooth, double* P_smooth, unsigned flags);
int dfm_em_obs_batch(dfm_handle* h, int B, int T, int N, int r_u, int r_o, const double* panel, const double* G, double* Lam,
                     double* R, double* A, double* Q, double* mu0, double* P0, int max_iter, double tol, double* loglik_path,
                     int* iters, double* f_smooth, double* P_smooth, unsigned flags);

/* --- PCA initialisation (reference: pca_score, dfm_functions.ipynb:179-183, on the standardised
 * balanced panel, :339-348) followed by the OLS start of EM: Lam = OLS(x on F), R = residual
 * variance, A/Q = VAR(1) OLS of F, mu0 = 0, P0 = F'F/T.  Balanced panels only (no NaN). */
int dfm_pca_init_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* panel,
                           double* Lam, double* R, double* A, double* Q, double* mu0, double* P0,
                           double* factors /* [B][T][r] PCA scores, may be NULL */);
int dfm_pca_init_batch(dfm_handle* h, int B, int T, int N, int r, const double* panel, double* Lam,
                       double* R, double* A, double* Q, double* mu0, double* P0, double* factors);

/* --- the reference's NON-parametric estimator, batched ---------------------------------------------
 * dfm_als_batch: `estimate_factor!` (dfm_functions.ipynb:328-382) for B independent runs -- the runs of
 * `estimate_factor_numbers` / `amengual_watson_test` (:698-768), bootstrap draws, Monte-Carlo replicates.
 * z: the standardised estimation window ([T][N] per run, NaN = missing, `standardize_data` :501-509 applied by
 * the caller); run b reads z + b * z_stride (0: all runs share one panel).  F [B][T][r]: in = starting factors
 * (`pca_score`, :179-183, columns >= r_each[b] ignored), out = factors after the last sweep.  Lam [B][N][r]:
 * loadings of the last sweep, NaN for the series the reference leaves undefined (fewer than nt_min observed
 * periods, :357).  A run stops after the sweep at which |SSR_old - SSR| < tol T N (SSR_old = 0 before the
 * first sweep: at least one sweep always runs, :349-353, :367-368) or after max_iter sweeps.
 * ssr_path [B][path_cap] (may be NULL): SSR after every sweep (`m.fes.ssr`, :366), NaN past iters[b].
 * R2 [B][N] (may be NULL): :372-380.  r_each may be NULL (every run has r factors).  r <= DFM_MAX_R and
 * (T + N) * pad(r) * 8 bytes must fit the 160 KB of LDS (DFM_E_DIMS otherwise). */
int dfm_als_batch_dev(dfm_handle* h, int B, int T, int N, int r, const double* z, long long z_stride,
                      const int* r_each, double* F, double* Lam, int nt_min, int max_iter, double tol,
                      double* ssr_path, int path_cap, int* iters, double* ssr, double* R2);
int dfm_als_batch(dfm_handle* h, int B, int T, int N, int r, const double* z, long long z_stride,
                  const int* r_each, double* F, double* Lam, int nt_min, int max_iter, double tol,
                  double* ssr_path, int path_cap, int* iters, double* ssr, double* R2);

/* dfm_standardize_batch_dev: `standardize_data` (dfm_functions.ipynb:501-509) of B panels IN PLACE (device
 * pointers): per series the mean and the POPULATION standard deviation over the observed cells; NaN stays NaN.
 * mean [B][N], sd [B][N] may be NULL. */
int dfm_standardize_batch_dev(dfm_handle* h, int B, int T, int N, double* panel, double* mean, double* sd);

/* dfm_ols_batch: P complete-case least-squares problems (`ols_skipmissing(..., Balanced())`,
 * dfm_functions.ipynb:242-252; the engine of `estimate_factor_loading!` :391-415, `uar` :305-311 and
 * `estimate_var!` :444-468).  Problem p regresses y_p[t] = y[p * y_stride + t * y_inc] on the rows of X_p =
 * X + p * x_stride ([T][K], x_stride 0 = shared regressors), dropping every row in which y or a regressor is
 * NaN.  Outputs: beta [P][K]; resid [P][T] (NaN on dropped rows; may be NULL); ssr [P]; tss [P] = sum (y -
 * ybar)^2 over the used rows (may be NULL; r2 = 1 - ssr / tss, `compute_r2` :565-569); nobs [P] = rows used.
 * Problems with fewer than max(nt_min, K) complete rows get NaN.  K <= 64. */
int dfm_ols_batch_dev(dfm_handle* h, int P, int T, int K, const double* X, long long x_stride, const double* y,
                      long long y_stride, long long y_inc, int nt_min, double* beta, double* resid, double* ssr,
                      double* tss, int* nobs);
int dfm_ols_batch(dfm_handle* h, int P, int T, int K, const double* X, long long x_stride, const double* y,
                  long long y_stride, long long y_inc, int nt_min, double* beta, double* resid, double* ssr,
                  double* tss, int* nobs);

/* --- wild-bootstrap impulse-response bands of the factor VAR (BASELINE config 5) --------------------
 * The reference stops at the point estimate: `estimate_var!` (dfm_functions.ipynb:444-468), `fill_matrices!`
 * (:477-492: companion M, selector Q, G = lower Cholesky of the residual covariance) and `impulse_response`
 * (:793-816: irf[:, t, k] = Q M^t G[:, k]).  dfm_var_bootstrap_irf runs B recursive-design wild-bootstrap
 * draws of that chain: e*_t = s_t e_t with one Rademacher sign per period, y*_t = c + sum_l A_l y*_{t-l} +
 * e*_t (y*_t = y_t for the first p periods), VAR(p) with constant re-estimated on y*, irf* from its M*, G*.
 * y [T][ns]: the VAR's data over the estimation window (no NaN); betahat [1 + ns p][ns] (constant first) and
 * resid [T][ns] (rows < p ignored): the point estimate, e.g. from dfm_ols_batch.  signs [B][T] (+1 / -1) or
 * NULL: signs drawn on the device (Philox4x32-10 keyed by seed, counter (period, first_draw + d); bit 0 of
 * word 0), a pure function of the GLOBAL draw index: a rank that owns draws [lo, hi) passes first_draw = lo.
 * Outputs: irf [B][ns][H][ns] (variable, horizon, shock); beta_out [B][1 + ns p][ns] or NULL.
 * ns <= 8, 1 + ns p <= 64.  A draw with all signs +1 reproduces the point estimate. */
int dfm_var_bootstrap_irf_dev(dfm_handle* h, int B, int T, int ns, int p, int H, const double* y,
                              const double* betahat, const double* resid, const double* signs, uint64_t seed,
                              int64_t first_draw, double* beta_out, double* irf);
int dfm_var_bootstrap_irf(dfm_handle* h, int B, int T, int ns, int p, int H, const double* y,
                          const double* betahat, const double* resid, const double* signs, uint64_t seed,
                          int64_t first_draw, double* beta_out, double* irf);
/* Nearest-rank quantiles over draws: x [B][S] -> out [nq][S], out[j][s] = the ceil(q[j] B)-th smallest of
 * x[0..B)[s] (NaN draws sort last).  B <= 16384 (the draws of one series are sorted in LDS). */
int dfm_quantile_bands_dev(dfm_handle* h, int B, int S, int nq, const double* x, const double* q, double* out);
int dfm_quantile_bands(dfm_handle* h, int B, int S, int nq, const double* x, const double* q, double* out);

/* --- structural-break statistics ------------------------------------------------------
 * dfm_chow_batch: P Chow statistics with HAC covariance -- `compute_chow` / `regress_hac` / `hac` /
 * `form_hscrc` / `form_kernel` (dfm_functions.ipynb:832-977); a `compute_qlr` (:1019-1047) is the maximum over
 * the problems of one series and bandwidth.  Series s: its complete cases y [S][Tmax], X [S][Tmax][k] (rows
 * 0 .. Tlen[s]-1 in use; k <= 8).  Problem p: series prob_series[p], break date prob_break[p] (the first
 * prob_break[p] rows are "before": D_t = 1 for t >= break, 0-based), Bartlett bandwidth prob_q[p] <= 15 (0 =
 * heteroskedasticity-robust only).  chow[p] = gamma' V22^-1 gamma of y = X beta + (X D) gamma. */
int dfm_chow_batch_dev(dfm_handle* h, int S, int Tmax, int k, const double* y, const double* X, const int* Tlen,
                       int P, const int* prob_series, const int* prob_break, const int* prob_q, double* chow);
int dfm_chow_batch(dfm_handle* h, int S, int Tmax, int k, const double* y, const double* X, const int* Tlen,
                   int P, const int* prob_series, const int* prob_break, const int* prob_q, double* chow);

/* --- filtered states, prediction errors and out-of-sample evaluation (csrc/filter.hip) -----------------
 * dfm_filter_batch: what the model knew at time t.  Model, layouts and conventions are those of dfm_forecast_batch:
 * x_t = Lam f_t + e_t, f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t, state z_t = (f_t, .., f_{t-p+1}) of width k = r p <=
 * DFM_MAX_R, mu0 / P0 the moments of z_0 (the period before panel row 0), NaN = missing cell, mean / sd [B][N] both given or
 * both NULL.  ONE forward recursion in covariance form (no matrix but the r x r W_t = I + U' C_t U, eigenvalues >= 1, is
 * factorised: Q, P_pred and C_t may be singular, so DFM_F_SINGULAR_Q is accepted and changes nothing) gives every origin.
 * THE PARAMETERS ARE HELD FIXED OVER ALL ORIGINS: the evaluation measures the data flow through a given fit, not
 * re-estimation (a caller who wants that batches expanding windows through dfm_em_batch and passes per-replicate parameters).
 * Outputs, every one may be NULL (then it is not written, and not computed where nothing else needs it); kk = k (k + 1) / 2:
 *   z_pred [B][T][k], P_pred [B][T][kk] packed lower   E, Var[z_t | x_0 .. x_{t-1}]
 *   z_filt [B][T][k], P_filt [B][T][kk]                E, Var[z_t | x_0 .. x_t]
 *   loglik_t [B][T]   log density of row t's observed cells given the rows before it; 0 for a row without observed cells
 *   xpred [B][T][N]   mean_i + sd_i lam_i' f_{t|t-1}, on every cell
 *   verr  [B][T][N]   x_ti - xpred in data units; NaN on a missing cell
 *   vstd  [B][T][N]   (x_ti - lam_i' f_{t|t-1}) / sqrt(lam_i' P11_{t|t-1} lam_i + R_i) in model units; NaN on a missing cell
 *   msfe  [B][H][N]   h = 1 .. H: the mean over the origins t = t0 .. T-1-h with x_{t+h,i} observed of
 *                     sd_i^2 (x_{t+h,i} - lam_i' (M^h z_{t|t})[:r])^2, M the companion matrix; NaN where there is no such origin
 *   msfe0 [B][H][N]   the same mean of sd_i^2 x_{t+h,i}^2: the unconditional-mean forecast, the benchmark
 *   cnt   [B][H][N]   int32, the number of origins averaged
 * H = 0: no evaluation -- msfe, msfe0 and cnt are left untouched whether NULL or not.  H < 0, t0 outside [0, T): DFM_E_DIMS.
 * N beyond the register tiling of the collapse with missing cells (1024 for r <= 8, 512 for r <= 16, 256 beyond): DFM_E_DIMS.
 * A NaN in the panel without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING.  A replicate whose update meets a non-finite value or a
 * P_pred / W_t that is not positive semi-definite writes NaN from that period on; the outputs are written and the call (the
 * host-pointer entry; dfm_check_status after the _dev entry) returns DFM_E_NUMERIC.  Sums over origins are taken in a fixed
 * order: results are bit-identical from run to run. */
int dfm_filter_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int H, int t0, const double* panel,
                         const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                         const double* P0, const double* mean, const double* sd, double* z_pred, double* P_pred,
                         double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr, double* vstd,
                         double* msfe, double* msfe0, int* cnt, unsigned flags);
int dfm_filter_batch(dfm_handle* h, int B, int T, int N, int r, int p, int H, int t0, const double* panel,
                     const double* Lam, const double* R, const double* Avar, const double* Q, const double* mu0,
                     const double* P0, const double* mean, const double* sd, double* z_pred, double* P_pred,
                     double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr, double* vstd,
                     double* msfe, double* msfe0, int* cnt, unsigned flags);

/* dfm_filter_ar_batch (csrc/filter_ar.hip): the same for the model with AR(q) idiosyncratic terms -- what dfm_filter_batch is to
 * dfm_forecast_batch, for dfm_forecast_ar_batch.  Model, inputs and conventions are those of dfm_ks_pass_ar_batch (1 <= q <= 4):
 * m = max(p, q + 1), state z_t = (f_t, .., f_{t-m+1}) of width k = r m <= DFM_MAX_R, the quasi-differenced rows
 * y_t = x_t - sum_l rho_l x_{t-l} = LamK z_t + eps_t for the panel rows t = q .. T-1 (a cell of y is missing when x_ti or one of its
 * q lags is), mu0 / P0 used exactly as the pass uses them (loglik_t summed over the rows is the pass's loglik), mean / sd as
 * dfm_filter_batch.  ONE forward recursion in covariance form, with the observation loading on the first w = r (q + 1) entries of
 * the state (only the w x w W_t = I + U' C_t U is factorised), gives every origin; THE PARAMETERS ARE HELD FIXED OVER ALL ORIGINS.
 * All outputs have n = T - q rows, the panel rows q .. T-1 (the pass's convention).  Every output may be NULL; kk = k (k + 1) / 2:
 *   z_pred [B][n][k], P_pred [B][n][kk] packed lower   E, Var[z_t | y rows before t]
 *   z_filt [B][n][k], P_filt [B][n][kk]                E, Var[z_t | y rows through t]
 *   loglik_t [B][n]   log density of row t's observed y cells given the rows before it; 0 for a row without observed cells
 *   xpred [B][n][N]   mean_i + sd_i (lamK_i' z_pred[t] + sum_l rho_il x_{t-l,i}): the one-step prediction of x, defined where x_ti
 *                     itself is missing; NaN where a lag is missing
 *   verr  [B][n][N]   sd_i (y_ti - lamK_i' z_pred[t]) = x - xpred in data units; NaN where y_ti is missing
 *   vstd  [B][n][N]   (y_ti - lamK_i' z_pred[t]) / sqrt(lamK_i' P_pred[:w,:w] lamK_i + sig2_i); NaN where y_ti is missing
 *   msfe, msfe_common, msfe0 [B][H][N]   h = 1 .. H: the mean over the qualifying origins of sd_i^2 (x_{t+h,i} - full)^2,
 *                     sd_i^2 (x_{t+h,i} - common)^2 and sd_i^2 x_{t+h,i}^2 (x in model units); NaN without such an origin
 *   cnt   [B][H][N]   int32, the origins averaged -- the same for all three
 * The forecast at origin t (a panel row) of a series whose cells t, t-1, .., t-q+1 are all observed:
 *   e_{t-l|t} = x_{t-l,i} - lam_i' z_{t|t}[block l], l = 0 .. q-1;  f_{t+h|t} = (M^h z_{t|t})[:r], M the companion matrix;
 *   e_{t+h|t} = sum_l rho_il e_{t+h-l|t} (the AR(q) recursion run forward);
 *   full = lam_i' f_{t+h|t} + e_{t+h|t},  common = lam_i' f_{t+h|t} (the factor-only forecast from the same state).
 * On a balanced panel `full` is the exact E[x_{t+h,i} | x_0 .. x_t] of the likelihood, which is conditional on the first q rows.
 * With missing cells the information set is the pass's own: a missing cell removes q + 1 quasi-differenced cells -- the convention
 * of the pass's likelihood.  Qualifying origins are t = t0 .. T-1-h with the cells t .. t-q+1 and t+h of series i observed; an
 * origin whose last q cells are not all observed needs lags the state does not hold, and is not evaluated and not counted.
 * msfe / msfe_common says what the idiosyncratic persistence buys, per series and horizon.
 * H = 0: no evaluation -- msfe, msfe_common, msfe0 and cnt are left untouched whether NULL or not.
 * Status: H < 0, q < 1, T <= q, t0 outside [q, T): DFM_E_DIMS (q = 0 is dfm_filter_batch); q > 4, or r max(p, q + 1) > DFM_MAX_R:
 * DFM_E_R_UNSUPPORTED; a NULL required input, mean without sd: DFM_E_NULL; a NaN in the panel without DFM_F_MAY_HAVE_MISSING:
 * DFM_E_MISSING; N beyond the collapse's register tiling at the state's width, as the pass: DFM_E_DIMS.  A replicate whose update
 * meets a non-finite value or a P_pred / W_t that is not positive semi-definite writes NaN from that period on; the outputs are
 * written and the call (the host-pointer entry; dfm_check_status after the _dev entry) returns DFM_E_NUMERIC.  Sums over origins
 * are taken in a fixed order: results are bit-identical from run to run.
 * Allocates in the handle (kept for the next call): the quasi-differenced panel [B][n][N], the loadings on the lag blocks, the
 * collapse's per-period arrays, the moments the caller does not take and the evaluation's running sums.  dfm_workspace_bytes does
 * not count them.  Outputs must not overlap the inputs. */
int dfm_filter_ar_batch_dev(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, int t0, const double* panel,
                            const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                            const double* mu0, const double* P0, const double* mean, const double* sd, double* z_pred,
                            double* P_pred, double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr,
                            double* vstd, double* msfe, double* msfe_common, double* msfe0, int* cnt, unsigned flags);
int dfm_filter_ar_batch(dfm_handle* h, int B, int T, int N, int r, int p, int q, int H, int t0, const double* panel,
                        const double* Lam, const double* sig2, const double* rho, const double* Avar, const double* Q,
                        const double* mu0, const double* P0, const double* mean, const double* sd, double* z_pred,
                        double* P_pred, double* z_filt, double* P_filt, double* loglik_t, double* xpred, double* verr,
                        double* vstd, double* msfe, double* msfe_common, double* msfe0, int* cnt, unsigned flags);

/* --- rolling-window out-of-sample evaluation, re-estimated at every origin (rolling.hip) ---------------
 * x [T][N] is ONE raw panel in data units (NaN = missing).  origins [O]: 0-based rows o_0 < o_1 < .. < o_{O-1} with
 * W - 1 <= o_b <= T - 1; lags [N]: publication lags lag_i >= 0 (NULL: all 0).  Both are HOST arrays in both entries.  Vintage b is
 * rows o_b - W + 1 .. o_b of x; cell (t, i) is visible iff x_ti is observed and t <= o_b - lag_i, every other cell of the window is
 * NaN.  Each window is standardised on its own visible cells (mean and population s.d., the reference's standardize_data):
 * win_mean, win_sd [O][N], win_nobs [O][N] (int); windows [O][W][N] takes the standardised vintages themselves.  A series with fewer than min_obs visible cells in a window, or whose visible
 * cells are all equal (s.d. 0), gives DFM_E_WINDOW: a status-word bit raised by rolling_window_kernel; the driver reads the word
 * behind that kernel of every slice and stops there, so no EM runs on such a window (both entries return the code).
 * Start: n_start = 1 or O parameter sets in standardised units, Lam_start [n_start][N][r], R_start [n_start][N], Avar_start
 * [n_start][r][r p], Q_start [n_start][r][r], mu0_start [n_start][r p], P0_start [n_start][r p][r p] (the layouts of
 * dfm_em_varp_batch; p = 1: those of dfm_em_batch).  sd_start [N] (may be NULL: no rescale) says which units the start's loadings are
 * in: window b starts from Lam_i sd_start_i / win_sd_bi and R_i (sd_start_i / win_sd_bi)^2; Avar, Q, mu0, P0 are copied.
 * EM: the windows are the batch of dfm_em_batch_dev (p = 1) or dfm_em_varp_batch_dev (p > 1) with T = W; max_iter, tol and flags
 * mean what they mean there.  max_iter = 0: no EM, the forecasts are those of the start parameters and iters = 0 (the record of
 * fixed parameters on per-window standardisation).  The windows' parameters Lam [O][N][r] .. P0 [O][r p][r p] are outputs (the EM runs
 * in place in them), as are loglik_path [O][max_iter] (NaN past iters[b]) and iters [O].
 * Forecasts: dfm_forecast_batch_dev on the windows with T = W, H, win_mean, win_sd.  For h = 0 .. H the target row is o_b + h:
 * fc [O][H+1][N] = xhat_b[W-1+h], fvar [O][H+1][N] = xvar_b[W-1+h], data units, written for every target (an origin at T - 1 has
 * real forecasts).  A target is SCORED iff its cell was not visible in vintage b (h >= 1; h = 0 where lag_i > 0: the nowcast),
 * o_b + h < T and x is observed there: err = x - fc, err_std = err / sqrt(fvar) [O][H+1][N], NaN on every other target; err0 = x -
 * win_mean[b][i] is the error of the unconditional-mean forecast of the same vintage.  msfe, msfe0 [H+1][N] are the means of err^2,
 * err0^2 over the scored origins, cnt [H+1][N] (int) their number; NaN where cnt = 0.  The sums are taken in origin order by one
 * lane per (h, i), no atomics: bit-identical from run to run.
 * Every output may be NULL, except the six parameter arrays when max_iter > 0 (DFM_E_NULL).
 * Status: W > T, W < max(2, p), H < 0, O < 1, origins out of range or not increasing, lag_i < 0 or lag_i > W - min_obs, min_obs <
 * r + 1, n_start not 1 or O, r p > DFM_MAX_R, max_iter < 0: DFM_E_DIMS.  A lag > 0 without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING (its
 * windows have NaN); a NaN in x without the flag: the pass's own DFM_E_MISSING (status word).  What the EM or the forecast entry
 * refuses at (O, W, N, r, p): its status.
 * The windows run in slices of at most 1024: one slice's windows, xhat, xvar and the EM's workspace are resident, so device memory
 * does not grow with O (beyond the origins and what the caller takes); the running sums are continued slice after slice.
 * Allocates in the handle (kept for the next call).  Outputs must not overlap the inputs. */
int dfm_rolling_eval_batch_dev(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start,
                               const double* x, const int* origins, const int* lags, const double* Lam_start,
                               const double* R_start, const double* Avar_start, const double* Q_start, const double* mu0_start,
                               const double* P0_start, const double* sd_start, int max_iter, double tol, double* Lam, double* R,
                               double* Avar, double* Q, double* mu0, double* P0, double* loglik_path, int* iters,
                               double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                               double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags);
int dfm_rolling_eval_batch(dfm_handle* h, int T, int N, int r, int p, int W, int H, int O, int min_obs, int n_start,
                           const double* x, const int* origins, const int* lags, const double* Lam_start,
                           const double* R_start, const double* Avar_start, const double* Q_start, const double* mu0_start,
                           const double* P0_start, const double* sd_start, int max_iter, double tol, double* Lam, double* R,
                           double* Avar, double* Q, double* mu0, double* P0, double* loglik_path, int* iters,
                           double* win_mean, double* win_sd, int* win_nobs, double* windows, double* fc, double* fvar, double* err,
                           double* err_std, double* msfe, double* msfe0, int* cnt, unsigned flags);

/* --- diffusion-index forecasts from the non-parametric fit, out of sample (diffusion.hip) ---------------
 * Stock and Watson (2002): at every origin the factors are re-estimated by ALS on the window, and every series is forecast h steps
 * ahead by a DIRECT regression on the factors and its own lags; the competitors are the same regression without the factors (AR) and
 * the window's mean.
 * x [T][N], origins [O], lags [N] (HOST arrays in both entries), W, min_obs, the vintages, their standardisation (win_mean, win_sd,
 * win_nobs [O][N], windows [O][W][N]) and DFM_E_WINDOW are exactly those of dfm_rolling_eval_batch (rolling_window_kernel).
 * Factors: F_start is [T][r] for n_start = 1 (window b starts from its rows o_b - W + 1 .. o_b) or [O][W][r] for n_start = O.  The
 * windows are the batch of dfm_als_batch_dev with T = W, nt_min, max_iter and tol (stop: |SSR_old - SSR| < tol W N); F [O][W][r], Lam
 * [O][N][r] (NaN: a series without loadings), als_iters [O] (int) and als_ssr [O] are its outputs.  max_iter = 0: no ALS, F is the start,
 * Lam and als_ssr are NaN and als_iters 0 (the record for given factors).
 * Regressions, on the standardised window z in window-local rows s = 0 .. W-1 (row W-1 is the origin): for every series i with l =
 * lag_i and every horizon h = 0 .. H with h + l >= 1, the target z_{s+h,i} on u_s = [1, F_s (r), z_{s-l,i}, .., z_{s-l-q+1,i}], K = 1 + r +
 * q regressors, over every row s with s - l - q + 1 >= 0, s + h <= W - 1 - l and all terms observed (complete cases); nobs_reg [O][H+1][N]
 * (int) is their number.  Fewer than max(nt_min, K) of them: every output of that regression is NaN (dfm_ols_batch's rule).  beta
 * [O][H+1][N][K] are the coefficients in the window's standardised units, in the order of u.  The AR benchmark is the same rows on the
 * columns {1, own lags}.  Forecasts, data units: fc = win_mean + win_sd beta' u_{W-1}, fc_ar likewise [O][H+1][N]; NaN where an own-lag
 * term of the origin is missing.  fvar [O][H+1][N] = win_sd^2 SSR / (nobs_reg - K) is the RESIDUAL variance of the regression only: it
 * carries no parameter uncertainty (none of beta, none of the estimated factors); NaN where nobs_reg = K.  h + l = 0 (the cell is
 * visible in the vintage): NaN and nobs_reg = 0.  A window whose factors hold a non-finite value (a row of the window with fewer usable
 * cells than factors makes the ALS's unpivoted elimination return inf or NaN; als_ssr shows it) gives NaN and nobs_reg = 0 for the
 * whole window and no error code.
 * Scores: the target o_b + h of (b, h, i) is SCORED iff fc is finite, o_b + h < T and x is observed there: err = x - fc, err_ar = x -
 * fc_ar, err_std = err / sqrt(fvar) [O][H+1][N], NaN on every other target.  msfe, msfe_ar, msfe0 [H+1][N] are the means of err^2,
 * err_ar^2 and (x - win_mean[b][i])^2 over the scored origins, cnt [H+1][N] (int) their number; NaN where cnt = 0.  The sums are taken
 * in origin order by one lane per (h, i), no atomics, continued slice after slice: bit-identical from run to run and under any slicing.
 * Every output may be NULL.
 * Status: 1 + r + q > 32, r < 1, q < 0, H < 0, O < 1, W > T, W < K + q + H + 2, min_obs < r + 1, n_start not 1 or O, origins out of range
 * or not increasing, lag_i < 0 or lag_i > W - min_obs, no lag_i = 0 (some series must reach the origin, or its factor row has no
 * data), (W + N) pad(r) doubles beyond the ALS's 160 KB of LDS, W (r + 1) doubles beyond the regressions', max_iter < 0: DFM_E_DIMS.  A lag
 * > 0 without DFM_F_MAY_HAVE_MISSING: DFM_E_MISSING; a NaN of x inside a window without the flag: DFM_E_MISSING through the status word.
 * The windows run in slices of at most 1024: device memory does not grow with O (beyond the origins and what the caller takes).
 * Allocates in the handle (kept for the next call).  Outputs must not overlap the inputs. */
int dfm_diffusion_eval_batch_dev(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int nt_min, int n_start,
                                 const double* x, const int* origins, const int* lags, const double* F_start, int max_iter,
                                 double tol, double* F, double* Lam, int* als_iters, double* als_ssr, double* win_mean,
                                 double* win_sd, int* win_nobs, double* windows, double* fc, double* fc_ar, double* fvar, double* err,
                                 double* err_ar, double* err_std, double* beta, int* nobs_reg, double* msfe, double* msfe_ar,
                                 double* msfe0, int* cnt, unsigned flags);
int dfm_diffusion_eval_batch(dfm_handle* h, int T, int N, int r, int q, int W, int H, int O, int min_obs, int nt_min, int n_start,
                             const double* x, const int* origins, const int* lags, const double* F_start, int max_iter, double tol,
                             double* F, double* Lam, int* als_iters, double* als_ssr, double* win_mean, double* win_sd,
                             int* win_nobs, double* windows, double* fc, double* fc_ar, double* fvar, double* err, double* err_ar,
                             double* err_std, double* beta, int* nobs_reg, double* msfe, double* msfe_ar, double* msfe0, int* cnt,
                             unsigned flags);

/* --- synthetic replicates generated on the device (SURVEY.md §8(d) DGP; no reference
 * counterpart -- the reference has no RNG).  Writes the standardised panel and the DGP parameters
 * rescaled to it.  Counter-based generator keyed by (seed, first_replicate + b). */
int dfm_synth_panels_dev(dfm_handle* h, uint64_t seed, int64_t first_replicate, int B, int T, int N,
                         int r, double missing_prob, double* panel, double* Lam, double* R,
                         double* A, double* Q, double* mu0, double* P0);

#ifdef __cplusplus
}
#endif
#endif /* DFM_HIP_H */
