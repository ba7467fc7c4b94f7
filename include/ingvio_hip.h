/*
 * ingvio_hip.h — C ABI of libingvio_hip.so: the MI355X (gfx950) covariance engine that replaces
 * the Eigen + SuiteSparse path behind InGVIO's StateManager / UpdateBase seam.
 *
 * The reference has no FFI today; its seam is the static API of `StateManager`
 * (ingvio_estimator/src/StateManager.h:38-127, sole friend of State::_cov, State.h:129-135) plus
 * the per-feature helpers of the Update classes.  Each export below names the reference
 * function(s) it replaces.  INTEGRATION.md shows the C++ shim a maintainer adds on the reference
 * side (ingvio_amd/csrc/host/ is that shim, ROS-free).
 *
 * Data model
 *   - A context owns `batch` independent filters on one GPU.  Filter b's covariance lives in HBM
 *     as an FP64 column-major n_b x n_b matrix inside an ldp x ldp buffer (ldp = n_max rounded up
 *     to 16), i.e. exactly Eigen::MatrixXd's layout (State.h:133) so `Eigen::Map` + `cov_set/get`
 *     is a plain strided copy.  The host keeps the typed nominal values and the Type::idx()/size()
 *     table (VecState.h:32-54); only integers and small parameter blocks cross the boundary - unless
 *     the context holds them itself (ingvio_nominal_create, opt-in).
 *   - All pointer arguments are HOST pointers unless the name ends in `_dev`.  Inputs are read
 *     during the call only; outputs are written before the call returns (calls that return
 *     results synchronise the context's stream; pure state mutations are asynchronous).
 *   - Every call returns 0 on success, <0 for the reference's fatal conditions / API misuse
 *     (the host shim turns these back into the reference's std::exit(EXIT_FAILURE) paths),
 *     >0 for soft conditions (e.g. INGVIO_NO_ROWS: nothing accepted, state untouched).
 *   - Thread-compatible per context, no globals (the reference is single-threaded,
 *     IngvioNode.cpp:36).
 *   - 3x3 rotations and T_cl2cr are row-major double[9] (+ double[3]); Phi (15x15), G (15x12),
 *     H and covariance blocks are column-major with explicit leading dimensions.
 */
#ifndef INGVIO_HIP_H
#define INGVIO_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INGVIO_OK 0
#define INGVIO_NO_ROWS 1             /* soft: no measurement rows survived gating              */
#define INGVIO_NEG_DIAG 2            /* soft: negative diagonal after update (StateManager.cpp:413-421, assert only) */
#define INGVIO_REJECTED 3            /* soft (per-filter status): the block chi^2 gate refused the update, state untouched (GnssUpdate.cpp:286) */
#define INGVIO_E_ARG (-1)            /* bad argument / out of range                            */
#define INGVIO_E_CAPACITY (-2)       /* n_max / c_max / f_max / m_max exceeded                 */
#define INGVIO_E_HIP (-3)            /* HIP runtime error, see ingvio_last_error               */
#define INGVIO_E_NOT_IN_STATE (-4)   /* StateManager.cpp:157-161 "Marg is not in the current state" */
#define INGVIO_E_UNSUPPORTED (-5)
#define INGVIO_E_NOT_PD (-6)         /* the innovation covariance S = H P H^T + R of a generic / landmark update is not positive definite:
                                        the filter's state is left untouched and its dx is zero */

typedef struct ingvio_ctx ingvio_ctx;

typedef struct {
    int batch;      /* independent filters held by this context (>= 1)                          */
    int n_max;      /* max state dimension N (21 + gnss + 6C + 3L)                               */
    int c_max;      /* max clones in the sliding window: <= 36; windows above 16 take the large-window kernels (factored path
                     * only: no dense MSCKF method), see DESIGN.md                */
    int f_max;      /* max features per MSCKF update                                             */
    int m_max;      /* max rows of a generic ekf_update (<= 128 in this build)                   */
    int device;     /* HIP device ordinal                                                        */
    void* stream;   /* hipStream_t to run on, or NULL to create a private non-blocking stream    */
} ingvio_ctx_desc;

/* State ctor (State.cpp:60-91): allocates P (batch x ldp^2 FP64, two ping-pong buffers) + workspaces. */
int ingvio_ctx_create(const ingvio_ctx_desc* desc, ingvio_ctx** out);
int ingvio_ctx_destroy(ingvio_ctx* ctx);
int ingvio_sync(ingvio_ctx* ctx);                     /* waits for the context's stream.  ingvio_propagate(_fused), ingvio_augment_clone,
                                                       * ingvio_marginalize and ingvio_append_independent only ENQUEUE (their inputs are
                                                       * copied into pinned staging before they return; argument / capacity errors are
                                                       * reported at once, a device fault by the next call that synchronises: this one,
                                                       * every cov_get / fetch / update call) */
void* ingvio_ctx_stream(ingvio_ctx* ctx);             /* the hipStream_t all kernels are launched on */
const char* ingvio_last_error(ingvio_ctx* ctx);
int ingvio_ldp(ingvio_ctx* ctx);                      /* leading dimension of the device P buffers  */
int ingvio_f_max(ingvio_ctx* ctx);                    /* feature capacity: length of the accepted[] arrays */
int ingvio_c_max(ingvio_ctx* ctx);                    /* window capacity: the most clones a staged frame may name */
/* Identity of the device code this library was built from (no reference counterpart): a JSON string
 * {"tu": {translation unit: hash of its text + headers + flags}, "kernels": {kernel: translation unit}} written by
 * ingvio_amd/build.py.  Profile counters are stored with it; bench.py prices a kernel only with counters of the same build. */
const char* ingvio_build_id(void);

/* initStateAndCov / getFullCov (State.cpp:126-167, StateManager.cpp:121-126). cov_get synchronises. */
int ingvio_cov_set(ingvio_ctx* ctx, int b, const double* P, int ld, int n);
int ingvio_cov_get(ingvio_ctx* ctx, int b, double* P, int ld);
int ingvio_get_n(ingvio_ctx* ctx, int b, int* n);
/* getMarginalCov (StateManager.cpp:128-153): out is ns x ns column-major, ns = sum(vsize). */
int ingvio_cov_get_marginal(ingvio_ctx* ctx, int b, const int* vidx, const int* vsize, int k, double* out);
/* getMarginalCov for filters [b0, b0 + nb) in one call: filter b0 + i takes the list vidx / vsize [i][k] (entries with vsize 0 pad a
 * shorter list) and gets its block - column-major ns x ns, ns = the sum of its vsize, exactly as ingvio_cov_get_marginal lays it out -
 * at out + i * ns_max * ns_max; the doubles of a filter's slot behind its ns * ns are not written.  The blocks are gathered on the
 * device from the live covariances (the entries are copies, bit for bit); one copy of the blocks alone and one synchronisation serve
 * the whole range, no full P travels.  Works with or without a nominal table.  1 <= ns_max <= INGVIO_MARGINAL_NS_MAX (the columns
 * one workgroup of the gather kernel lists).  INGVIO_E_ARG: range, NULL, k < 1, ns_max out of bounds, a filter's ns > ns_max, a
 * negative vsize; INGVIO_E_NOT_IN_STATE: an entry with vidx < 0 or vidx + vsize > the filter's n - nothing is written for any filter. */
#define INGVIO_MARGINAL_NS_MAX 64
int ingvio_cov_get_marginal_batch(ingvio_ctx* ctx, int b0, int nb, const int* vidx /* [nb][k] */, const int* vsize /* [nb][k] */,
                                  int k, int ns_max, double* out /* [nb][ns_max * ns_max] */);
/* device-to-device snapshot / restore of all filters' covariances and dims (benchmark hygiene). */
int ingvio_cov_snapshot(ingvio_ctx* ctx);
int ingvio_cov_restore(ingvio_ctx* ctx);

/* propagateStateCov (StateManager.cpp:42-119) for filters [b0, b0+nb).  Phi [nb][225], G [nb][180]
 * (column-major 15x15 / 15x12), dt [nb]; sigma = {noise_g, noise_a, noise_bg, noise_ba};
 * gnss_idx [nb][5] = state idx of {GPS, GLO, GAL, BDS, FS} or -1 (NULL: none);
 * sigma_cb / sigma_rw = StateParams::_noise_clockbias / _noise_cb_rw after quirk Q1. */
int ingvio_propagate(ingvio_ctx* ctx, int b0, int nb, const double* Phi, const double* G, const double* dt,
                     const double sigma[4], int enable_gnss, const int* gnss_idx,
                     double sigma_cb, double sigma_rw);
/* The k-step loop of ImuPropagator::propagateUntil (ImuPropagator.cpp:246-289) in ONE launch:
 * Phi [nb][k][225], G [nb][k][180], dt [nb][k].  The kernel composes the k transitions in LDS and
 * touches the covariance strip once (same result up to FP64 rounding). */
int ingvio_propagate_fused(ingvio_ctx* ctx, int b0, int nb, int k, const double* Phi, const double* G,
                           const double* dt, const double sigma[4], int enable_gnss, const int* gnss_idx,
                           double sigma_cb, double sigma_rw);

/* augmentSlidingWindowPose, covariance part (StateManager.cpp:279-293). R_i2w [nb][9] row-major.
 * new_idx [nb] receives the clone's idx == old N (bit-exact, StateManager.cpp:274). */
int ingvio_augment_clone(ingvio_ctx* ctx, int b0, int nb, const double* R_i2w, int* new_idx);
/* marginalize, covariance part (StateManager.cpp:163-177). idx [nb]. */
int ingvio_marginalize(ingvio_ctx* ctx, int b0, int nb, const int* idx, int size);
/* addVariableIndependent (StateManager.cpp:194-214). blk [nb][size*size] column-major. */
int ingvio_append_independent(ingvio_ctx* ctx, int b0, int nb, int size, const double* blk, int* new_idx);

/* noise kinds for the generic update */
#define INGVIO_R_SCALAR 0   /* R = (*R) * I                                                     */
#define INGVIO_R_DIAG 1     /* R = diag(R[0..m))     (GNSS, GnssUpdate.cpp:195,264)             */
#define INGVIO_R_FULL 2     /* R m x m column-major                                             */

/* ekfUpdate minus boxPlus (StateManager.cpp:359-423) on filter b: var_order as (vidx, vsize)[k],
 * H m x sum(vsize) column-major (ldh), res [m].  dx_out [N] = K res; the host applies boxPlus. */
int ingvio_ekf_update(ingvio_ctx* ctx, int b, const int* vidx, const int* vsize, int k,
                      const double* H, int ldh, int m, const double* res,
                      const double* R, int r_kind, double* dx_out);
/* ekfUpdate for filters [b0, b0+nb) in ONE launch and one synchronisation (e.g. the GNSS update of a whole batch): block i
 * belongs to filter b0+i.  R per block: one double (INGVIO_R_SCALAR) or m doubles (INGVIO_R_DIAG).  dx_out [nb][ldp]
 * (ingvio_ldp), status_out [nb] = INGVIO_OK / INGVIO_NEG_DIAG / INGVIO_E_NOT_PD per filter (may be NULL); the call returns the last
 * filter status that is not INGVIO_OK. */
typedef struct {
    const int* vidx;          /* var_order as (idx, size)[k]                                        */
    const int* vsize;
    int k;
    const double* H;          /* m x sum(vsize), column-major, leading dimension ldh                   */
    int ldh, m;
    const double* res;        /* [m]                                                                */
    const double* R;          /* noise, see r_kind                                                  */
} ingvio_update_block;
int ingvio_ekf_update_batch(ingvio_ctx* ctx, int b0, int nb, const ingvio_update_block* blocks, int r_kind,
                            double* dx_out, int* status_out);
/* ---- GnssUpdate::updateTrackedSys, covariance part, for filters [b0, b0+nb) (GnssUpdate.cpp:148-290) --------------------
 * Block i carries ALL candidate rows of filter b0+i as the host assembled them (pseudo-range rows, then Doppler rows; R = the m
 * row variances) over var_order = [SE23, YOF, clock biases..., FS] (<= 32 columns, <= 256 rows; m = 0: no measurement).  On the
 * device, in one launch sequence and without host round trips:
 *   gate_rows     (_is_gnss_chi2_test, :190,:259)  every row is tested alone on the PRIOR: r^2 / (h Pvv h^T + R_i) < chi2_table[1];
 *                 a row only touches the columns of its own sub_order, so the stacked row gives the reference's 11-column product;
 *                 rejected rows are removed, the rest move up (order kept).  A clock column whose rows were all rejected stays
 *                 in var_order as a zero column: the same posterior as the reference's shorter var_order.
 *   strong_reject (_is_gnss_strong_reject, :286)   if <= 14 rows survive, the block is gated as a whole against chi2_table[rows];
 *                 on failure the state is untouched and the filter's status is INGVIO_REJECTED.
 *   ekfUpdate     (:290) with the diagonal R; dx_out [nb][ldp] = K res (zero when nothing was applied).
 * rows_out [nb]: rows handed to ekfUpdate; keep_out [nb][ingvio_mld()]: 1/0 per candidate row; status_out [nb].
 * stage / run / fetch are the same operation split for device-resident throughput runs (run only enqueues kernels and may be
 * repeated: the staged rows are read-only, each run compacts them into working buffers). */
typedef struct {
    int gate_rows;
    int strong_reject;
    const double* chi2_table;      /* UpdateBase::_chi_squared_table, chi2_table[dof] */
    int chi2_len;
    int in_frame;                  /* ingvio_gnss_stage only: != 0 - the staged update belongs to the frame staged with ingvio_frame_stage
                                    * and is applied BY ingvio_frame_run right after the frame's MSCKF update (IngvioFilter.cpp:329-362
                                    * follows :276-327 in the same callback), in the same sweep over P: the update only reads the <= 16
                                    * columns var_order of the posterior, which are formed first; its rank-<=16 downdate then rides on
                                    * the MSCKF write-back (one read + one write of P for both).  Windows up to 16 clones, at most 16
                                    * candidate rows and 16 columns, no in-frame landmark stage - otherwise ingvio_frame_run applies
                                    * it as a separate pass.  Results: ingvio_gnss_fetch (dx in the state's index space AFTER the
                                    * frame's marginalisation).  ingvio_gnss_run must not be called for an in-frame stage. */
} ingvio_gnss_opts;
int ingvio_gnss_update_batch(ingvio_ctx* ctx, int b0, int nb, const ingvio_update_block* blocks, const ingvio_gnss_opts* opts,
                             double* dx_out, int* rows_out, int* keep_out, int* status_out);
int ingvio_gnss_stage(ingvio_ctx* ctx, int b0, int nb, const ingvio_update_block* blocks, const ingvio_gnss_opts* opts);
int ingvio_gnss_run(ingvio_ctx* ctx, int b0, int nb);
int ingvio_gnss_fetch(ingvio_ctx* ctx, int b0, int nb, double* dx_out, int* rows_out, int* keep_out, double* gamma_out,
                      int* status_out);
int ingvio_mld(ingvio_ctx* ctx);                      /* row stride of keep_out / gamma_out */

/* ---- the gnss_comm front of the GNSS update on the device ----------------------------------------
 * What GnssUpdate::updateTrackedSys obtains from gnss_comm before it builds its rows (GnssUpdate.cpp:98-122): satellite states
 * from the broadcast ephemerides at transmit time (gnss_comm/src/gnss_spp.cpp:50-98, gnss_utility.cpp:390-640), elevation,
 * Saastamoinen/Niell and Klobuchar delays (:762-899), pseudo-range and Doppler residuals (gnss_spp.cpp:100-146, :256-282).
 * ingvio_gnss_front_stage evaluates all of it for every filter of the range (one lane per satellite) and writes the candidate
 * rows where ingvio_gnss_stage would have put them: follow with ingvio_gnss_run / ingvio_gnss_fetch.  GLONASS satellites take
 * geph2svdt / geph2pos / geph2vel (gnss_utility.cpp:642-731: Runge-Kutta integration of the broadcast PZ-90 state vector).
 * Times are seconds of the GPS week.
 * The rows are GnssUpdate.cpp:148-272 with _is_adjust_yof = 0, the YOF column (column 9 of every row) zero, unless
 * ingvio_set_gnss_adjust_yof is on: then a pseudo-range row carries -u^T R_enu2ecef dRz(yaw) p_w there and a Doppler row the same with
 * v_w (:164-167, :239-242; dRz = GnssManager::dotRw2enu).  Column count, var_order and the row gates are the same either way.
 * Flat records of doubles:
 *   ephemeris [INGVIO_EPH_N]: sys (gnss_comm::sys2idx: GPS 0, GLO 1, GAL 2, BDS 3), prn, toe, toe in the constellation's own
 *     week (BDS: BDT of toe - 14 s, gnss_utility.cpp:489; else = toe), toc, A, e, i0, omg, OMG0, M0, delta_n, OMG_dot, i_dot,
 *     cuc, cus, crc, crs, cic, cis, af0, af1, af2, tgd[0], ura
 *     GLONASS (sys == 1, GloEphem): sys, prn, toe (GPS week seconds), 0, 0, pos[3], vel[3], acc[3] (m, m/s, m/s^2, PZ-90 ECEF),
 *     tau_n, gamma, zeros up to ura at [24]; the observation's frequency is the satellite's FDMA channel
 *   observation [INGVIO_OBS_N]: receive time, L1 pseudo-range (m), L1 Doppler (Hz), psr_std, dopp_std, L1 frequency (Hz, < 0: no L1;
 *     a frequency of exactly 0 is not a defined input: the Doppler residual and its noise divide by it)
 * An entry whose sys is none of 0 .. 3 is skipped like one without L1: unusable, no rows. */
#define INGVIO_EPH_N 25
#define INGVIO_OBS_N 6
#define INGVIO_GNSS_MAX_SAT 64
typedef struct {
    int n_sat;                                /* <= INGVIO_GNSS_MAX_SAT                                                */
    const double* eph;                        /* [n_sat][INGVIO_EPH_N]                                                 */
    const double* obs;                        /* [n_sat][INGVIO_OBS_N]                                                 */
    const double* ion;                        /* [8] Klobuchar parameters (latest_gnss_iono_params) or NULL            */
    double doy;                               /* gnss_comm::time2doy of the epoch                                      */
    double p_w[3], v_w[3];                    /* State::_extended_pose valueTrans1() / valueTrans2()                   */
    double cb[4], fs;                         /* GnssManager::getClockbiasVec (m), FS value (m/s)                      */
    double yaw_offset;                        /* YOF value                                                             */
    double R_enu2ecef[9], anchor_ecef[3];     /* GvioAligner::getRenu2ecef (row-major), translation of getTenu2ecef    */
    int idx_se23, idx_yof, idx_fs, idx_cb[4]; /* Type::idx() of the variables (idx_cb[s] = -1: clock s not in the state) */
    double psr_noise_amp, dopp_noise_amp;     /* GnssUpdate::_psr_noise_amp / _dopp_noise_amp                          */
} ingvio_gnss_epoch;
int ingvio_gnss_front_stage(ingvio_ctx* ctx, int b0, int nb, const ingvio_gnss_epoch* epochs, const ingvio_gnss_opts* opts);
/* per-satellite results of the last front_stage: out [nb][INGVIO_GNSS_MAX_SAT][INGVIO_GNSS_SAT_REC] = res_pos, res_vel, unit
 * receiver->satellite (3), azimuth, elevation, ionosphere delay, troposphere delay, usable (1/0), then the gnss_comm::SatState
 * (gnss_constant.hpp:506-516): pos (3), vel (3), dt, ddt, tgd, transmit time */
#define INGVIO_GNSS_SAT_REC 20
int ingvio_gnss_front_fetch(ingvio_ctx* ctx, int b0, int nb, double* out);
/* The same evaluation for any list of epochs, detached from the filters and from the staged rows (the idx_* / noise fields of
 * the epochs are ignored): the residual evaluator of gnss_comm::psr_pos (gnss_spp.cpp:148-254) and GvioAligner::batchAlign
 * (GvioAligner.cpp:88-383), whose iterations live in the host shim (host/GvioAligner.cpp).  To evaluate at a receiver given in
 * ECEF set R_enu2ecef = I, yaw_offset = 0, p_w = 0, anchor_ecef = position, v_w = ECEF velocity.
 * out [n_epochs][INGVIO_GNSS_MAX_SAT][INGVIO_GNSS_SAT_REC]. */
int ingvio_gnss_sat_eval(ingvio_ctx* ctx, int n_epochs, const ingvio_gnss_epoch* epochs, double* out);
/* test hook: the candidate rows of filter b as the last GNSS stage of any form left them, before any gate (a run only reads them):
 * H [ingvio_mld() x 32] column-major with leading dimension ingvio_mld() (rows 0 .. *m_out - 1: pseudo-range rows, then Doppler rows),
 * res / noise [ingvio_mld()] (noise: the row variances), colmap [32]: state column of H's column c for c < *nc_out - the var_order
 * [SE23 (9), YOF, clock biases in order of first appearance, FS] of GnssUpdate.cpp:148-272. */
int ingvio_debug_gnss_staged_rows(ingvio_ctx* ctx, int b, double* H, double* res, double* noise, int* colmap, int* m_out, int* nc_out);

/* ---- feature-sharded single filter (optional mode): the per-feature work (K3-K5 gate, K6/K7 in information form)
 * is independent given the prior, so G replicas of ONE filter can each take F/G of the frame's features:
 *   ingvio_frame_run_phase(ctx, restore, 1)   propagate + clone + gate + Gram of the staged (local) features
 *   ingvio_debug_msckf_info(ctx, b, A, &ncol) the local [A | b] = [sum H_j^T H_j | sum H_j^T r_j]  (35 KB at 11 clones, 260 KB at 30)
 *   -- the ONE exchange step: sum over the replicas (all-reduce; ingvio_amd/parallel.py::sharded_frame_update) --
 *   ingvio_info_set(ctx, b, A_sum, ncol, n_accepted_total)
 *   ingvio_frame_run_phase(ctx, 0, 2)         solve + apply + marginalise: identical posterior on every replica
 * phase 0 = ingvio_frame_run.  Factored method only; the accepted-feature cap (max_accept) is a global order and is not
 * supported across shards (INGVIO_E_ARG when the staged options carry max_accept > 0 and phase != 0).
 * Protocol: phase 1 leaves the filters half-stepped (cloned, n + 6, not yet updated); until phase 2 has run, every entry point
 * that changes or snapshots the covariance — ingvio_frame_run, a second phase 1, ingvio_frame_stage, ingvio_ekf_update, ... —
 * returns INGVIO_E_ARG; reading (ingvio_cov_get, ingvio_debug_msckf_info, ingvio_frame_fetch) and ingvio_info_set are allowed.
 * Phase 2 without a pending phase 1 (or twice) is INGVIO_E_ARG.  ingvio_cov_restore abandons a pending split step. */
int ingvio_frame_run_phase(ingvio_ctx* ctx, int restore_prior, int phase);
int ingvio_info_set(ingvio_ctx* ctx, int b, const double* A, int ncol, int n_accepted);
/* The same exchange WITHOUT a host hop: ingvio_info_reduce sums filter b's chunk partials on the device into one contiguous buffer
 * [A | b | n_accepted] (row-major ncol x (ncol + 1), then the local accepted count as a double; *count = ncol (ncol + 1) + 1) and
 * returns its DEVICE pointer (valid until the context is destroyed; complete when the call returns).  The caller all-reduces (sum)
 * the buffer in place over the replicas - ncclAllReduce on the pointer, or torch.distributed on a zero-copy view
 * (__cuda_array_interface__, ingvio_amd/parallel.py::sharded_frame_update) - and must have that collective finished (stream
 * synchronised) before ingvio_info_commit, which installs the buffer as the filter's information for phase 2. */
int ingvio_info_reduce(ingvio_ctx* ctx, int b, double** dev_ptr, int* count, int* ncol_out);
int ingvio_info_commit(ingvio_ctx* ctx, int b);

/* ---- batched SLAM-landmark update (LandmarkUpdate::updateLandmark{Mono,Stereo}, LandmarkUpdate.cpp:32-149) ----------------
 * For every in-state landmark observed in the current frame: rows against [extended pose | extrinsics | anchor clone | landmark]
 * (calcResJacobianSingleLandmark*, :521-572 / :619-686, as written), the per-landmark chi^2 gate on the prior (:98-99), the
 * accepted rows stacked, one ekfUpdate (:146) - rows, gates, stacking and the update on the device for a range of filters, with
 * S = H P H^T + s^2 I factorised outside LDS (up to INGVIO_LM_MAX landmarks = 256 stereo rows per filter).
 * The nominal values are the host's: it hands over the CURRENT pose / extrinsics / landmark positions and applies dx itself -
 * or, with the device-resident nominal state, the table's (ingvio_landmark_stage_nominal below: only the observations travel). */
#define INGVIO_LM_MAX 64
typedef struct {
    double R_i2w[9], p_i2w[3];    /* extended pose (row-major rotation, position)                          */
    double R_cl2i[9], p_c2i[3];   /* left camera -> IMU extrinsics                                          */
    int idx_epose, idx_ext;       /* state indices (9 and 6 columns)                                        */
    int n_lm;                     /* <= INGVIO_LM_MAX                                                       */
    const int* lm_idx;            /* [n_lm] state index of each landmark (3 columns)                        */
    const int* anchor_idx;        /* [n_lm] state index of its anchor clone (6 columns)                     */
    const double* pf;             /* [n_lm][3] world position (AnchoredLandmark::valuePosXyz)               */
    const double* uv;             /* [n_lm][4] current observation u0 v0 u1 v1 (mono: first two)            */
    const unsigned char* tracked; /* [n_lm] 1 = observed in this frame (0: the landmark is skipped)         */
} ingvio_landmark_frame;
typedef struct {
    int stereo;
    double noise;                 /* visual noise (sigma)                                                   */
    double chi2_thr;              /* quantile(chi_squared(rows per landmark), 0.95) (Update.cpp:98-100)     */
    double R_cl2cr[9], t_cl2cr[3];
    int in_frame;                 /* 1: ingvio_frame_run performs the update between the MSCKF update and the marginalisation
                                     (IngvioFilter.cpp:296-322 order) for every staged filter               */
} ingvio_landmark_opts;
int ingvio_landmark_stage(ingvio_ctx* ctx, int b0, int nb, const ingvio_landmark_frame* frames, const ingvio_landmark_opts* opts);
int ingvio_landmark_run(ingvio_ctx* ctx, int b0, int nb);
/* dx [nb][ldp] (may be NULL), rows [nb] accepted rows, accept [nb][INGVIO_LM_MAX] 1/0, gamma [nb][INGVIO_LM_MAX] (-1: not
 * tracked), status [nb] (INGVIO_NEG_DIAG etc. as ingvio_ekf_update); any pointer may be NULL */
int ingvio_landmark_fetch(ingvio_ctx* ctx, int b0, int nb, double* dx, int* rows, int* accept, double* gamma, int* status);

/* whitenResidual (Update.cpp:36-79): gamma = res^T (H Pcc H^T + R)^-1 res. */
int ingvio_chi2_gamma(ingvio_ctx* ctx, int b, const int* vidx, const int* vsize, int k,
                      const double* H, int ldh, int m, const double* res,
                      const double* R, int r_kind, double* gamma);

/* Many independent whitenResidual gates against the same prior in one launch and one synchronisation (all SLAM landmarks of
 * a frame, LandmarkUpdate.cpp:98-99; the per-row GNSS gates, GnssUpdate.cpp:190,259).  R = noise_var * I. */
typedef struct {
    const int* vidx;          /* var_order of this block as (idx, size)[k]                           */
    const int* vsize;
    int k;
    const double* H;          /* m x sum(vsize), column-major, leading dimension ldh                   */
    int ldh, m;
    const double* res;        /* [m]                                                                */
} ingvio_gate_block;
int ingvio_chi2_gamma_multi(ingvio_ctx* ctx, int b, int nblk, const ingvio_gate_block* blocks, double noise_var,
                            double* gamma_out);

/* ---- SLAM-landmark covariance operations -----------------------------
 * addVariableDelayedInvertible (StateManager.cpp:461-543): H_old s x sum(vsize) (ldh), H_new s x s (ldn),
 * s <= 6; appends s rows/columns, new_idx receives the new variable's idx (== old N). */
int ingvio_add_variable_delayed_invertible(ingvio_ctx* ctx, int b, const int* vidx, const int* vsize, int k,
                                           const double* H_old, int ldh, const double* H_new, int ldn, int s,
                                           double noise, int* new_idx);
/* addVariableDelayed (StateManager.cpp:549-637): H_old m x sum(vsize), H_new m x s, res [m] (inputs are not
 * modified; the Givens rotations run on the device copy).  chi2_check = quantile(chi_squared(m), 0.95)
 * (boost in the reference, :610-612; the caller supplies it).  *added = 0 when m <= s (:571-575) or when the
 * chi2 test fails (:614-618; state untouched).  On success the variable is appended (new_idx), the EKF update
 * with the remaining m-s rows is applied to the covariance and dx_out [N+s] = K res; the host applies boxPlus.
 * INGVIO_E_CAPACITY: n + s > n_max, m > ingvio_mld, the trailing update's S beyond LDS, or the gate's bound
 * 8 (nc (m-s) + (m-s+1)^2) <= 150 KB (stereo: 22 clones).  Under ingvio_set_delayed_form(ctx, 1) a candidate beyond the gate's
 * bound is not refused: it runs as a one-filter call of ingvio_add_variable_delayed_batch, with the same outputs. */
int ingvio_add_variable_delayed(ingvio_ctx* ctx, int b, const int* vidx, const int* vsize, int k,
                                const double* H_old, int ldh, const double* H_new, int ldn, int m, int s,
                                const double* res, double noise, double chi2_mult, int do_chi2, double chi2_check,
                                double* dx_out, int* added, int* new_idx, double* chi2_out);
/* addVariableDelayed for filters [b0, b0 + nb) with several candidate variables per filter, in one call and ONE stream
 * synchronisation (kernels_delayed.hip).  Per filter the candidates are tried in order, each against the covariance the
 * previous one left (the appended variable included), exactly as the reference's loops over new landmarks do
 * (LandmarkUpdate.cpp:399-421, :892-956): Givens rotations, chi2 of the lower m - s rows on the prior marginal, refusal
 * when chi2 > chi2_mult * chi2_check && do_chi2, otherwise addVariableDelayedInvertible and the ekfUpdate with the lower
 * rows.  The verdicts are taken on the device; the host sees nothing between the candidates.
 *   added / new_idx / chi2 [nb][cand_cap]: candidate j of filter b0 + i at [i * cand_cap + j].  A candidate with m <= s is
 *     skipped (added = 0, chi2 = 0); a refused or skipped candidate leaves that filter's P and n untouched bit for bit.
 *     new_idx = the filter's live N at the append (-1 when not added).  var_old_order must lie inside the state the
 *     filter has when the call starts (new variables go to the end, so the indices hold over the rounds).
 *   dx [nb][cand_cap][ldp] (may be NULL): K res of candidate j in the index space after its own append, zero when it was
 *     not added; boxPlus is the caller's (ingvio_nominal_box_plus or the host).
 *   status [nb] (may be NULL): INGVIO_OK / INGVIO_NEG_DIAG / INGVIO_E_NOT_PD per filter, as ingvio_ekf_update_batch;
 *     after a trailing update whose S was not positive definite the filter's remaining candidates are not tried.
 *     The worst of these codes is also the call's return value; the outputs and every filter's n are valid with it.
 * One noise (sigma, R = noise^2 I) for the call.  The call never touches the device nominal table: entering the new
 * variable there stays ingvio_nominal_get / _set (ingvio_landmark_init_nominal below forms the rows of new landmarks on the
 * device and enters them itself).
 * Refused before anything changes: INGVIO_E_ARG (range, NULL where data is needed, s outside 1..6, ldh / ldn < m,
 * n_cand > cand_cap, a split frame step pending, or a frame / GNSS epoch / landmark stage from the nominal table that
 * has not run - as ingvio_nominal_box_plus); INGVIO_E_NOT_IN_STATE (an (idx, size) beyond the filter's n);
 * INGVIO_E_CAPACITY (n + sum of the filter's s > n_max, m > ingvio_mld, more columns than the context holds, the
 * trailing update's S beyond LDS, the single-filter gate's bound 8 (nc (m-s) + (m-s+1)^2) <= 150 KB, or the front's own:
 * it keeps the rows AND T = Pcc H^T in LDS, 8 ((2 nc + 1)(m | 1) + 3 s m + (m-s+1)^2) + 4 nc + 1.3 KB <= 160 KB - tighter
 * than the single-filter call for wide windows, e.g. m = 64 rows on 16 clones fit, m = 84 on 21 clones do not).  The last two hold
 * under ingvio_set_delayed_form(ctx, 0) only: under mode 1 or 2 such a candidate takes the large form of the front (a round whose
 * filters mix the forms is two launches, one per form) and only the other bounds refuse. */
typedef struct {
    const int* vidx; const int* vsize; int k;   /* var_old_order as (idx, size)[k]                       */
    const double* H_old; int ldh;               /* m x sum(vsize), column-major                          */
    const double* H_new; int ldn;               /* m x s                                                 */
    const double* res;                          /* [m]                                                   */
    int m, s;                                   /* s <= 6                                                */
    double chi2_check;                          /* quantile(chi_squared(m), 0.95), supplied by the caller */
} ingvio_delayed_cand;
typedef struct {
    int n_cand;                                 /* 0: nothing for this filter                            */
    const ingvio_delayed_cand* cand;            /* [n_cand], tried in this order                         */
} ingvio_delayed_block;
int ingvio_add_variable_delayed_batch(ingvio_ctx* ctx, int b0, int nb, const ingvio_delayed_block* blocks,
                                      double noise, double chi2_mult, int do_chi2, int cand_cap,
                                      int* added, int* new_idx, double* chi2, double* dx, int* status);
/* replaceVarLinear (StateManager.cpp:639-693): the target variable (tidx, tsize <= 6) becomes H * [dependence
 * variables]: its rows/columns <- P H^T, its diagonal block <- H Pcc H^T.  H tsize x sum(vsize) (ldh). */
int ingvio_replace_var_linear(ingvio_ctx* ctx, int b, int tidx, int tsize, const int* vidx, const int* vsize, int k,
                              const double* H, int ldh);

/* ---- MSCKF visual update: K3-K11 ----------------------------------------------------------
 * One frame of flattened MapServer data for one filter (FeatureInfo/_stereo_obs/_landmark,
 * MapServer.h:69-134, flattened by the host shim).  Clones in ascending timestamp. */
typedef struct {
    int n_clones;                        /* C: clones in the window (State::_sw_camleft_poses)    */
    const int* clone_idx;                /* [C] Type::idx() of each clone                         */
    const double* clone_R;               /* [C][9] valueLinearAsMat(), row-major                  */
    const double* clone_p;               /* [C][3] valueTrans()                                   */
    int n_feat;                          /* F                                                     */
    const double* pf;                    /* [F][3] _landmark->valuePosXyz()                       */
    const int* anchor;                   /* [F] window slot of getAnchoredPose()                  */
    const unsigned long long* obs_mask;  /* [F] bit s: observation at slot s takes part           */
    const double* uv;                    /* [F][C][4] StereoMeas::asVec() (mono: [0..1])          */
    const int* dof;                      /* [F] dof passed to testChiSquared (Q4)                 */
} ingvio_msckf_frame;

typedef struct {
    int stereo;               /* 1: calcResJacobian...StereoObs, 0: ...MonoObs                      */
    double R_cl2cr[9];        /* StateParams::_T_cl2cr linear part, row-major                       */
    double t_cl2cr[3];
    double noise;             /* _visual_noise (sigma)                                              */
    const double* chi2_table; /* chi2_table[d], d = 0..chi2_len-1 (UpdateBase::_chi_squared_table)  */
    int chi2_len;
    int max_accept;           /* RemoveLostUpdate::_max_valid_ids (20); <= 0: no cap                */
    int compress_rule;        /* 0 as_written (RemoveLost keeps all rows, Q2), 1 top_n.  The GPU    */
                              /* always compresses to n rows: the two are the same posterior.       */
    int selected_variant;     /* 0 RemoveLost form, 1 SwMarg/Keyframe form (anchor block assigned,  */
                              /* quirk Q10, SwMargUpdate.cpp:302)                                   */
} ingvio_msckf_opts;

/* RemoveLostUpdate::updateState{Mono,Stereo} (RemoveLostUpdate.cpp:40-167,276-405),
 * SwMargUpdate::updateState* (SwMargUpdate.cpp:42-189,216-365), KeyframeUpdate::updateState*
 * (KeyframeUpdate.cpp:438-735) after triangulation, for filters [b0, b0+nb):
 * Jacobians + nullspace (K3,K4), chi2 gate on the prior (K5), accepted-feature cap, TSQR
 * compression (K6,K7) and the Kalman update (K8-K11).
 * dx_out [nb][ldp]; accepted [nb][f_max] (1/0); gamma [nb][f_max] (may be NULL);
 * rows_out [nb] = rows handed to the Kalman update (0: none accepted, state untouched). */
int ingvio_msckf_update(ingvio_ctx* ctx, int b0, int nb, const ingvio_msckf_frame* frames,
                        const ingvio_msckf_opts* opts, double* dx_out, int* accepted, double* gamma,
                        int* rows_out);

/* Selects how ingvio_msckf_update / ingvio_frame_run evaluate K4-K11 (same posterior to FP64 rounding):
 *   0 dense    — literal: projected blocks H_j, dense S_j, Householder TSQR of the stacked H,
 *                Cholesky Kalman update (kernels_msckf.hip, kernels_ekf.hip)
 *   1 factored — default: exploits H_x = Gblk*D (per-observation 4x3 factors times a sparse
 *                selection), the projector identity for gamma, R^T R accumulated as 6x6 clone-pair
 *                blocks and the information-form update (kernels_factored.hip); see DESIGN.md.
 * Also settable at context creation through the environment: INGVIO_MSCKF_METHOD=dense|factored. */
int ingvio_set_msckf_method(ingvio_ctx* ctx, int method);

/* Stacked-QR compression on its own (the SPQR call sites RemoveLostUpdate.cpp:376-397,
 * SwMargUpdate.cpp:336-357, KeyframeUpdate.cpp:707-728): H m x n (ldh) column-major, res [m] ->
 * H_thin n x n upper triangular (ldt) and r_thin [n] with H_thin^T H_thin = H^T H,
 * H_thin^T r_thin = H^T res.  Any m, n <= 4096.  Two methods (ingvio_set_qr_method): blocked Householder QR (kernels_qr.hip; the
 * oracle's reflector convention, rows above 6144 in chunks) and, by default for tall stacks (n >= 128, m >= 6 n: the 35100 x 180
 * stack of 300 features x 30 clones, the 6000 x 800 stress shape), Cholesky-QR: H_thin = chol([H|res]^T [H|res]) on the matrix
 * cores (kernels_chol.hip), diagonal positive, identical H_thin^T H_thin / H_thin^T r_thin - which is all ekfUpdate reads.
 * Touches no filter state; device buffers and the launch graph are cached per shape. */
/* method: 0 automatic (default), 1 Householder always, 2 Cholesky-QR always */
int ingvio_set_qr_method(ingvio_ctx* ctx, int method);
int ingvio_qr_compress(ingvio_ctx* ctx, const double* H, int ldh, int m, int n, const double* res,
                       double* H_thin, int ldt, double* r_thin);

/* ---- feature triangulation ----------------------------------------------
 * Triangulator::triangulateMonoObs / triangulateStereoObs (Triangulator.cpp:173-318, 320-359) for every feature of
 * frames[0..nb): Levenberg-Marquardt on (x/z, y/z, 1/z) in the frame of the last observation, Huber weights, depth /
 * parallax / convergence gates.  Of a frame only n_clones, clone_R, clone_p, n_feat, obs_mask and uv are used
 * (pf, anchor, dof may be NULL; clone_idx must be valid state indices or 0).  Outputs per filter stride f_max:
 * pf_out [nb][f_max][3] world points (0 where it failed), ok_out [nb][f_max].
 * frames == NULL: triangulate the frames already staged by ingvio_frame_stage / ingvio_msckf_update; the results stay
 * in the staged device frame (with mask_failed != 0 failed features lose their observation mask and drop out), so a
 * following ingvio_frame_run uses them without a host round trip. */
typedef struct {
    int stereo;
    double R_cl2cr[9];          /* row-major */
    double t_cl2cr[3];
    double trans_thres, huber_epsilon, conv_precision, init_damping;   /* Triangulator.h:67-70: 0.1, 0.01, 5e-7, 1e-3 */
    int outer_loop_max_iter, inner_loop_max_iter;                      /* :71-72: 10, 10 */
    double max_depth, min_depth;                                       /* :74-75: 60, 0.2 */
    int mask_failed;
} ingvio_tri_opts;
int ingvio_triangulate(ingvio_ctx* ctx, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_tri_opts* opts,
                       double* pf_out, int* ok_out);
/* RemoveLostUpdate::updateStateStereo / Mono in ONE device round trip (RemoveLostUpdate.cpp:276-405, :41-170): the reference
 * triangulates every lost feature (MapServerManager.cpp:274-341), drops the ones that fail and updates with the rest.  Here the
 * staged features' points are triangulated on the device from the frame's own observations (frames[].pf is ignored), a feature whose
 * triangulation fails - including a point behind its anchor camera, MapServerManager.cpp:290,325 - drops out of the update on the
 * device (accepted[i] = 0), and the rest is ingvio_msckf_update.  tri_ok[i]: 1 triangulated, 0 failed, 2 triangulated but behind its
 * anchor camera (the reference counts that attempt, MapServerManager.cpp:287 / :322).  pf_out [nb][f_max][3], tri_ok [nb][f_max]
 * (may be NULL).  One upload, one download, one synchronisation: ingvio_triangulate + ingvio_msckf_update cost a single real-time
 * filter two of each and the host a second packing of the same observations (round 5).
 * tri_masks (NULL, or nb pointers of which any may be NULL): the observations the TRIANGULATION of filter i's features uses, one
 * mask per feature over the window slots, when they differ from the update's obs_mask - the selected-stamp updates
 * (SwMargUpdate.cpp:236-257, KeyframeUpdate.cpp:607-628) triangulate from every observation and update with the selected stamps
 * only; frames[i].uv must then carry the measurements of every slot of the triangulation mask. */
int ingvio_msckf_update_tri(ingvio_ctx* ctx, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts,
                            const ingvio_tri_opts* tri, const unsigned long long* const* tri_masks, double* dx_out, int* accepted,
                            double* gamma, int* rows_out, double* pf_out, int* tri_ok);

/* ---- one benchmark "update" for the whole batch ------------------------------
 * k-step propagation + clone + MSCKF update + marginalise one clone, all filters, no host
 * synchronisation between the stages.  stage() uploads inputs (outside any timed region),
 * run() only enqueues kernels, fetch() synchronises and downloads. */
typedef struct {
    int k;                    /* IMU steps, 1 <= k <= 64, per filter (see below)                    */
    const double* Phi;        /* [k][225]                                                           */
    const double* G;          /* [k][180]                                                           */
    const double* dt;         /* [k]                                                                */
    int gnss_idx[5];
    double R_i2w[9];          /* IMU rotation at clone time                                         */
    int marg_idx;             /* idx of the clone to marginalise afterwards, -1: none               */
} ingvio_frame_step;

/* k, sigma, sigma_cb and sigma_rw are held per filter: ingvio_frame_run propagates filter b with the k of its own step and the noise
 * of the stage that staged it.  steps[i].k may differ between the filters of one call (each in 1..64; one out of range: INGVIO_E_ARG,
 * nothing changed).  sigma, sigma_cb and sigma_rw become the settings of the filters [b0, b0+nb) the call stages; the other filters
 * keep those of the frame last staged for them.  The first stage after ingvio_ctx_create or after a failed stage gives every filter
 * its settings.  ingvio_frame_set_imu_noise sets them per filter.  The same holds for ingvio_frame_stage_tracks. */
int ingvio_frame_stage(ingvio_ctx* ctx, int b0, int nb, const ingvio_frame_step* steps,
                       const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts,
                       const double sigma[4], int enable_gnss, double sigma_cb, double sigma_rw);
/* Same as ingvio_frame_stage for the WHOLE batch (b0 = 0, nb = batch), but the inputs travel on a separate copy
 * stream into a second set of device input buffers, so the call may be issued while the previous ingvio_frame_run is
 * still executing: PCIe and host packing of frame i+1 overlap the kernels of frame i.  Pattern per frame:
 * run(i); stage_async(i+1); fetch(i).  The next ingvio_frame_run / ingvio_triangulate(staged) waits for the copy. */
int ingvio_frame_stage_async(ingvio_ctx* ctx, int b0, int nb, const ingvio_frame_step* steps,
                             const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts,
                             const double sigma[4], int enable_gnss, double sigma_cb, double sigma_rw);
/* noise [nb][6] = {noise_g, noise_a, noise_bg, noise_ba, sigma_cb, sigma_rw} of filters [b0, b0+nb) for the frame currently
 * staged (sync or async); INGVIO_E_ARG if nothing is staged, the range or pointer is bad, a value is not finite, or a split
 * step (ingvio_frame_run_phase 1 -> 2) is pending.  A frame already running is not affected.  After ingvio_frame_stage_async the
 * values travel on the copy stream into the pending input set: run(i); stage_async(i+1); set_imu_noise(i+1); fetch(i). */
int ingvio_frame_set_imu_noise(ingvio_ctx* ctx, int b0, int nb, const double* noise);
/* ---- device-resident track store: the frame hand-over as a DELTA (round 6) -------------------------------------------------
 * The reference's MapServer gains ONE observation per live feature per camera frame (MapServerManager::collectStereoMeas,
 * MapServerManager.cpp:146-217) and forgets the observations of the clones that leave the window (KeyframeUpdate::
 * cleanStereoObsAtMargTime, KeyframeUpdate.cpp:737-761; SwMargUpdate.cpp:425-446); ingvio_frame_stage re-sends every filter's whole
 * [F][C][4] measurement array and its k transition matrices with every frame (61 KB per update at 150 features x 11 clones, k = 10).
 * With a track store the observations of every live track stay on the device (uv [t_max][c_max][4], a 64-bit observation mask and
 * the triangulated point per track and filter), and a frame travels as
 *   - the delta on the store, applied in this order: window slots that leave (the tracks' rows close up), tracks that were erased,
 *     the new clone's column (one measurement per observed track), points that changed;
 *   - the frame the update uses: the clone table and, per feature, its track, anchor slot, dof and - for the Selected-timestamp
 *     updates (SwMargUpdate.cpp:236-257) - a mask ANDed onto the stored one;
 *   - the raw IMU samples of the frame and the nominal state at its start: ImuPropagator::stateAndCovTransition
 *     (ImuPropagator.cpp:98-162, analytic branch) runs on the device (Phi, G, dt and the clone rotation never cross the bus);
 * about 7.6 KB per update for the same frame.  ingvio_frame_stage_tracks leaves the context exactly as ingvio_frame_stage(_async) does:
 * ingvio_frame_run / ingvio_frame_fetch follow.  Slot and track numbers are the CALLER's bookkeeping (the shim's MapServer); tracks
 * are numbered 0 .. t_max - 1 (t_max <= 65536), anchor slots and dof fit a byte.  A track may appear once per delta in obs_track
 * (one observation per track and frame): repeats are not checked, and two threads would then write one mask word. */
typedef struct {
    int n_drop; const int* drop_slots;            /* window slots leaving the window, ascending (before the append)              */
    int n_free; const int* free_tracks;           /* erased features: the track's observations are forgotten                     */
    int append_slot;                              /* window slot of the frame's new clone, -1: no new column                     */
    int n_obs; const int* obs_track; const double* obs_uv;      /* [n_obs], [n_obs][4] (mono: first two)                            */
    int n_pf; const int* pf_track; const double* pf;            /* [n_pf], [n_pf][3] points that changed                            */
    int n_clones; const int* clone_idx; const double* clone_R; const double* clone_p;      /* as ingvio_msckf_frame                */
    int n_feat; const int* feat_track; const int* feat_anchor; const int* feat_dof;
    const unsigned long long* feat_sel;           /* [n_feat] or NULL: every stored observation of the track takes part          */
} ingvio_track_frame;
typedef struct {
    int k;                        /* IMU steps, 1 <= k <= 64, per filter (as ingvio_frame_stage)                                  */
    const double* imu;            /* [k][7] gyro (3), accel (3), dt of each step, as ImuPropagator::propagateUntil forms them     */
    double R[9], p[3], v[3], bg[3], ba[3], gravity[3];      /* State::_extended_pose (row-major R), biases, gravity at the frame's start */
    int gnss_idx[5];
    int marg_idx;                 /* idx of the clone to marginalise afterwards, -1: none                                        */
} ingvio_frame_step_raw;
int ingvio_tracks_create(ingvio_ctx* ctx, int t_max);             /* allocates (or clears) the store: every track empty            */
int ingvio_frame_stage_tracks(ingvio_ctx* ctx, int b0, int nb, const ingvio_frame_step_raw* steps, const ingvio_track_frame* frames,
                              const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double sigma_cb, double sigma_rw,
                              int async /* != 0: whole batch, on the copy stream into the second input set, as ingvio_frame_stage_async */);
/* ---- device-resident nominal state (opt-in) ------------------------------------------------------------------
 * The typed values behind the Type::idx() table - StateManager's _err_var list with its nominal values (State.h:95-127) - held per
 * filter on the device, so that a closed-loop filter hands over only raw IMU samples and the track delta per frame: the device applies
 * boxPlus with the frame's dx, drops the marginalised clone, shifts the indices behind it, integrates the IMU nominal state and forms
 * the new clone's pose.  A context that never calls ingvio_nominal_create behaves exactly as without it.
 * Variable kinds (values: R row-major, p, v; a Vec3 in p, a Scalar in p[0], a landmark's world position valuePosXyz in p): */
#define INGVIO_NOM_NONE (-1)      /* free slot (a marginalised clone leaves one; the next clone takes the lowest free slot)       */
#define INGVIO_NOM_SE23 0         /* PoseState SE23, 9 columns: the extended pose (PoseState.cpp:174-186)                         */
#define INGVIO_NOM_SE3 1          /* PoseState SE3, 6 columns: clones, extrinsics (PoseState.cpp:79-88)                            */
#define INGVIO_NOM_VEC3 2         /* VecState Vec3, 3 columns: biases (VecState.cpp:25-29)                                         */
#define INGVIO_NOM_SCALAR 3       /* Scalar, 1 column: clock biases, FS, YOF (VecState.cpp:40-44)                                  */
#define INGVIO_NOM_LANDMARK 4     /* AnchoredLandmark, 3 columns; anchor = slot of its anchor clone (AnchoredLandmark.cpp:227-243) */
#define INGVIO_NOM_VAL 15         /* doubles per variable value                                                                    */
typedef struct {
    int n_var;                    /* slots in use (<= v_max); get: written                                                         */
    int* kind; int* idx; int* anchor;     /* [n_var] kind, Type::idx(), anchor slot (landmarks) or -1                              */
    double* val;                  /* [n_var][INGVIO_NOM_VAL] R (9), p (3), v (3)                                                   */
    int n_clones; int* clone_var; /* slots of the window's clones (State::_sw_camleft_poses), ascending time; get: [c_max]        */
    int v_ext, v_pose, v_bg, v_ba;        /* slots of _camleft_imu_extrinsics (SE3), _extended_pose (SE23), _bg, _ba (Vec3)        */
    double gravity[3];
} ingvio_nominal;
/* allocates (or clears: every slot free) a table of up to v_max variables per filter */
int ingvio_nominal_create(ingvio_ctx* ctx, int v_max);
int ingvio_nominal_set(ingvio_ctx* ctx, int b0, int nb, const ingvio_nominal* nom);
/* synchronises (the host's keyframe / marginalisation policy reads the clone poses here); the caller's arrays hold v_max / c_max entries */
int ingvio_nominal_get(ingvio_ctx* ctx, int b0, int nb, ingvio_nominal* out);
/* StateManager::boxPlus (StateManager.cpp:244-251) on the device with dx [nb][ldp] in the live index space (the dx of ingvio_gnss_fetch,
 * ingvio_landmark_fetch, ingvio_ekf_update_batch).  Every variable reads dx only: the order of the variables does not matter. */
int ingvio_nominal_box_plus(ingvio_ctx* ctx, int b0, int nb, const double* dx);
/* ingvio_frame_stage_tracks with the nominal values taken from the device table: per filter only k, the IMU samples, gnss_idx and marg_idx
 * (the idx of a window clone, -1: none).  frames[].n_clones / clone_idx / clone_R / clone_p are ignored: the window is the table's
 * plus the new clone (appended at idx = the live N, at the end of the window, with pose T_i2w * T_cl2i of the propagated state,
 * StateManager.cpp:263-272).  The following ingvio_frame_run ends, on the device and in this order, with boxPlus of the frame's dx
 * (the index space of the update: new clone included, before the marginalisation), the drop of the marginalised clone and the shift of
 * every later idx by 6 (StateManager.cpp:155-192).  async: as ingvio_frame_stage_tracks; the copy stream waits for the table of the
 * frame enqueued last, so run(i); stage(i+1, async); fetch_begin(i); run(i+1); fetch_end(i) is a closed loop.
 * Refused before anything changes: no table (INGVIO_E_ARG), a range other than the whole batch (b0 != 0 or nb != batch: the post-frame
 * step covers every filter, INGVIO_E_ARG), a frame staged from the table that has not run yet (INGVIO_E_ARG), an
 * in-frame GNSS or host-fed landmark stage or frame_parts > 1 (INGVIO_E_UNSUPPORTED), marg_idx not a window clone (INGVIO_E_NOT_IN_STATE), a
 * landmark anchored to the clone that leaves (INGVIO_E_ARG: stage with marg_idx = -1 and let ingvio_nominal_tail drop the clone), no free slot or a full window (INGVIO_E_CAPACITY).  While such a frame is
 * staged and has not run, ingvio_frame_stage(_async), ingvio_frame_stage_tracks, ingvio_nominal_set / _box_plus, ingvio_cov_snapshot
 * and ingvio_frame_run(restore_prior != 0) return INGVIO_E_ARG and ingvio_frame_run_phase INGVIO_E_UNSUPPORTED.  The ONE stage accepted
 * while such a frame is pending is ingvio_landmark_stage_nominal with opts->in_frame != 0: the frame's own landmark update.  ingvio_cov_snapshot /
 * ingvio_cov_restore copy the table with the covariance (restore abandons such a staged frame); a restore whose snapshot was taken
 * before ingvio_nominal_create holds no table and is refused (INGVIO_E_ARG). */
typedef struct {
    int k;                        /* IMU steps, 1 <= k <= 64                                                                       */
    const double* imu;            /* [k][7] gyro (3), accel (3), dt                                                                 */
    int gnss_idx[5];
    int marg_idx;
} ingvio_frame_step_nominal;
int ingvio_frame_stage_tracks_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_frame_step_nominal* steps, const ingvio_track_frame* frames,
                                      const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double sigma_cb, double sigma_rw,
                                      int async);
/* The FIRST MSCKF update of a camera frame (RemoveLostUpdate::updateStateStereo / Mono) with its features' points found on the device.
 * tri == NULL: ingvio_frame_stage_tracks_nominal exactly (that export is this call with NULL).
 * tri != NULL: the following ingvio_frame_run triangulates every listed feature of every filter from the window's clone poses as they
 * stand behind the IMU integration and the new clone (FeatureInfoManager::triangulateFeatureInfo*, MapServerManager.cpp:275-341) and in
 * front of the gate: from EVERY observation the store holds over the window, the new clone's column included (the full stored mask, not
 * stored & feat_sel), with the settings of ingvio_msckf_update_tri (check_anchor and mask_failed on).  A feature whose triangulation
 * fails or whose point lies behind its anchor camera loses its mask and drops out of the gate (accepted = 0); a point that succeeded
 * goes into the staged frame and into the store's point of its track (setValuePosXyz).  No host synchronisation; ingvio_frame_fetch_tri
 * returns flags and points.  Everything else is ingvio_frame_stage_tracks_nominal's: ingvio_landmark_stage_nominal(in_frame) and
 * ingvio_gnss_frame_stage_nominal on it, snapshot / restore, ingvio_nominal_tail behind it, the post-frame boxPlus / drop / shift.
 * Refused before anything is enqueued or changed: everything ingvio_frame_stage_tracks_nominal refuses, with its codes; tri without a
 * track store (INGVIO_E_ARG); tri->outer_loop_max_iter < 0 or tri->inner_loop_max_iter < 0 (INGVIO_E_ARG).  One thing precedes the
 * checks of the delta itself (capacity, slots, tracks out of range): a context's first stage with tri allocates its mask / track (and,
 * at placement 1, result) buffers and synchronises the compute stream once; a stage refused after that leaves table, store, covariance
 * and n as they were.  A HIP runtime error while enqueueing (INGVIO_E_HIP) invalidates the staged frame as for every stage. */
int ingvio_frame_stage_tracks_nominal_tri(ingvio_ctx* ctx, int b0, int nb, const ingvio_frame_step_nominal* steps, const ingvio_track_frame* frames,
                                          const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double sigma_cb, double sigma_rw,
                                          const ingvio_tri_opts* tri /* NULL: the store's points */, int async);
/* Where the triangulation of ingvio_frame_stage_tracks_nominal_tri is issued: 0 (default) on the compute stream in front of the gate, as
 * the update-only frame's; 1 at the stage, behind the gather (the copy stream of an asynchronous stage: off the step's chain).  Results
 * are bit-identical.  INGVIO_E_ARG for another mode or while a frame staged from the table has not run. */
int ingvio_set_first_tri_placement(ingvio_ctx* ctx, int mode);
/* The SECOND MSCKF update of a camera frame (SwMargUpdate / KeyframeUpdate::updateState*, IngvioFilter.cpp:271-324: behind RemoveLostUpdate,
 * linearised at the state that update left) as an update-only frame from the table and the track store: no IMU steps, no new clone, the
 * window is the table's as it stands (frames[].n_clones / clone_* are ignored).  frames[i].append_slot must be -1 and n_obs 0; n_drop,
 * n_free and n_pf are applied to the store as usual; feat_sel selects the stamps the update uses.  marg_idx [nb]: the idx of the window
 * clone the frame marginalises, -1: none (key-frame mode: ingvio_nominal_tail drops its two clones afterwards).
 * tri != NULL: ingvio_frame_run first triangulates every listed feature on the device from EVERY observation the store holds over the
 * window (SwMargUpdate.cpp:236-257, KeyframeUpdate.cpp:607-628, MapServerManager.cpp:309-341), with the settings of ingvio_msckf_update_tri
 * and without a host synchronisation; a feature whose triangulation fails or whose point lies behind its anchor drops out of the update,
 * a point that succeeded is also written to the store's point of its track (setValuePosXyz, MapServerManager.cpp:335), so a later frame
 * that lists the track without triangulating uses it.  tri == NULL: the store's points.
 * The context is left exactly as by ingvio_frame_stage_tracks_nominal: ingvio_frame_run / ingvio_frame_fetch(_begin / _end) follow, the run
 * ends with boxPlus of its dx, the drop and the shift on the table; async, snapshot / restore and ingvio_nominal_tail behind it as there.
 * ingvio_landmark_stage_nominal(in_frame) is accepted while it is pending (the reference runs the landmark update behind the second
 * MSCKF update, IngvioFilter.cpp:281-289).
 * Refused before anything changes: no table or no track store, a range other than the whole batch, another frame staged from the table
 * that has not run, append_slot >= 0 or n_obs > 0 (INGVIO_E_ARG); marg_idx not a window clone (INGVIO_E_NOT_IN_STATE); a landmark
 * anchored to the clone that leaves (INGVIO_E_ARG); frame_parts > 1 or an in-frame GNSS / host-fed landmark stage (INGVIO_E_UNSUPPORTED).
 * While it is pending: ingvio_gnss_frame_stage_nominal returns INGVIO_E_UNSUPPORTED (ingvio_gnss_front_stage_nominal + ingvio_gnss_run
 * behind the frame is the reference's order), ingvio_frame_run_phase INGVIO_E_UNSUPPORTED, ingvio_frame_run(restore_prior != 0)
 * INGVIO_E_ARG. */
int ingvio_update_stage_tracks_nominal(ingvio_ctx* ctx, int b0, int nb, const int* marg_idx /* [nb], -1: none */,
                                       const ingvio_track_frame* frames, const ingvio_msckf_opts* opts,
                                       const ingvio_tri_opts* tri /* NULL: the store's points */, int async);
/* flags and points of the triangulation of a frame from the table staged with tri (ingvio_frame_stage_tracks_nominal_tri or
 * ingvio_update_stage_tracks_nominal), after its run (and, pipelined, after the ingvio_frame_fetch_begin that follows it, for both kinds
 * of frame): pf_out [nb][f_max][3], tri_ok [nb][f_max] as ingvio_msckf_update_tri; INGVIO_E_ARG without a run that triangulated */
int ingvio_frame_fetch_tri(ingvio_ctx* ctx, int b0, int nb, double* pf_out, int* tri_ok);
/* ---- GNSS epochs in the device-resident closed loop ------------------------------------------------------------
 * Names the GNSS scalars of filters [b0, b0 + nb)'s tables: slots [nb][6] = the table slots of the clock biases GPS, GLO, GAL, BDS, then
 * FS, then YOF (State::GNSSType order, State.h:75); -1: not in the state.  From then on
 *   - ingvio_frame_stage_tracks_nominal with enable_gnss != 0 advances every registered clock with the frequency shift at each IMU sample,
 *     cb_s += dt_q * fs in the samples' order (ImuPropagator.cpp:139-148: _enable_gnss, the clock and FS in the state), on the device;
 *   - ingvio_gnss_front_stage_nominal reads the receiver state from the table.
 * The slots are part of the table's integer record: cleared by ingvio_nominal_create and by an ingvio_nominal_set of the filter, copied by
 * ingvio_cov_snapshot / _restore.  INGVIO_E_ARG, nothing changed: no table, a slot out of range, named twice or not an INGVIO_NOM_SCALAR,
 * a frame or a GNSS epoch staged from the table that has not run.  A filter that never registers runs exactly as before. */
int ingvio_nominal_set_gnss(ingvio_ctx* ctx, int b0, int nb, const int* slots /* [nb][6] */);
int ingvio_nominal_get_gnss(ingvio_ctx* ctx, int b0, int nb, int* slots /* [nb][6] */);
/* GnssUpdate::_is_adjust_yof for every GNSS launch of the context that forms rows: ingvio_gnss_front_stage, ingvio_gnss_front_stage_nominal
 * + ingvio_gnss_run, both orders of ingvio_gnss_frame_stage_nominal, ingvio_gnss_init_nominal and ingvio_debug_gnss_init_rows (the
 * columns are given with those calls).  ingvio_gnss_sat_eval has no rows and is unaffected.  on: 0 (the default; every launch produces
 * the bits it produces without this call) / != 0.  INGVIO_E_ARG: a GNSS epoch of any form staged and not yet run, or a split frame step
 * pending. */
int ingvio_set_gnss_adjust_yof(ingvio_ctx* ctx, int on);
/* StateManager::addGNSSVariable (StateManager.cpp:194-231; checkYofStatus adds YOF with it) on the table, for filters [b0, b0 + nb):
 * gtype[i] is the position of ingvio_nominal_set_gnss (0..3 the clock biases, 4 FS, 5 YOF), -1: nothing for this filter.  P gains an
 * independent 1 x 1 block at the live n (row and column n zero over [0, n), the diagonal var[i] - what ingvio_append_independent does),
 * the lowest free table slot becomes an INGVIO_NOM_SCALAR with idx = n and value[i], registered at that position.  All of it on the
 * device, on the context's stream, with no synchronisation; the host mirror (live sizes, table, slots) follows deterministically and
 * slot_out / idx_out [nb] (-1 where gtype is -1) come from it.  ingvio_cov_snapshot / _restore cover the scalar as they cover the table.
 * Refused before anything changes: INGVIO_E_ARG (no table, range, NULL, gtype outside -1..5, a scalar already registered at that
 * position, and the pending work ingvio_nominal_set_gnss refuses); INGVIO_E_CAPACITY (no free slot, or n + 1 > n_max). */
int ingvio_nominal_add_gnss(ingvio_ctx* ctx, int b0, int nb, const int* gtype /* [nb] */, const double* value /* [nb] */,
                            const double* var /* [nb] */, int* slot_out /* [nb] */, int* idx_out /* [nb] */);
/* StateManager::margGNSSVariable (StateManager.cpp:233-242 with marginalize :155-192) on the table, for filters [b0, b0 + nb): bit s of
 * mask[i] names the scalar registered at position s of ingvio_nominal_set_gnss.  Their rows and columns leave P in ONE read of P and one
 * write into the other ping-pong half, however many leave (the compaction of ingvio_nominal_tail); their slots become INGVIO_NOM_NONE,
 * their registrations -1, every surviving idx moves down by the number of removed columns below it, no surviving value changes.  No
 * synchronisation; the host mirror follows deterministically.  A filter with mask 0 is untouched; a call in which every mask is 0
 * launches nothing.  The clock indices of the next frame's ingvio_frame_step_nominal::gnss_idx are the host's to shrink.
 * Refused before anything changes: INGVIO_E_NOT_IN_STATE (a named position that is not registered, a table variable beyond the
 * filter's n); INGVIO_E_ARG (no table, range, NULL, bits above 5, and the pending work ingvio_nominal_tail refuses);
 * INGVIO_E_CAPACITY (a state too wide for the compaction's index maps). */
int ingvio_nominal_marg_gnss(ingvio_ctx* ctx, int b0, int nb, const unsigned* mask /* [nb] */);
/* ---- the landmark tail of a frame on the device -----------------------------------------------------------------
 * What callbackStereoFrame / callbackMonoFrame do behind the updates for the in-state landmarks, for filters [b0, b0 + nb) from what the
 * device holds, per filter in the reference's order:
 *   1. LandmarkUpdate::changeLandmarkAnchor (LandmarkUpdate.cpp:273-361): for every landmark of lm_slot, in that order, body = R_new^T
 *      (p_f - p_new) from the table's current values.  body.z <= 0: verdict 0, the landmark is marginalised instead (:298-302).  Otherwise
 *      verdict 1: FeatureInfoManager::changeAnchoredPose (MapServerManager.cpp:343-379), i.e. StateManager::replaceVarLinear
 *      (StateManager.cpp:639-693) with H = [-[p_f]x 0 | [p_f]x 0 | I] over [old anchor, new anchor, landmark]; the table's anchor slot
 *      becomes new_anchor, the world position stays (resetAnchoredPose(.., true)).
 *   2. the verdict-0 landmarks, the erase_slot landmarks (margAnchoredLandmarkInState, StateManager.cpp:340-353) and the marg_slot
 *      clones (margSwPose) are marginalised: P is compacted out of place into the other ping-pong half, n shrinks.
 *   3. the table: freed slots take INGVIO_NOM_NONE, the window list closes up, every surviving idx (the GNSS scalars' included) moves down
 *      by the size of what left below it; no value of a surviving variable changes.
 * All landmarks of a filter are one congruence P' = T P T^T (replacing L_i writes row and column L_i only and no H_j reads another
 * landmark), so P is read once and written once; the result equals the sequential reference up to rounding.  The diagonal blocks are
 * symmetrised as ingvio_replace_var_linear does, P stays exactly symmetric.
 * verdict [nb][lm_cap] (entry [i][e] for lm_slot[e] of filter b0 + i; the rest 0), status [nb] (may be NULL; INGVIO_OK).  The call
 * synchronises once at the end - only the device knows the verdicts - and the host mirror of the table follows them.  A filter whose
 * three lists are empty is untouched; a call in which every filter is empty launches nothing.  new_anchor is read only with
 * n_reanchor > 0.
 * Refused from the host mirror before anything changes: INGVIO_E_ARG (no table, range, NULL where data is needed, n_reanchor > lm_cap
 * or > 64, a split frame step pending, a frame / GNSS epoch / landmark stage from the table that has not run, a slot named twice or in
 * both landmark lists, new_anchor listed in marg_slot, a landmark already anchored to new_anchor, n_reanchor > 0 with fewer than two
 * window clones, a landmark in neither list that would stay anchored to a marg_slot clone); INGVIO_E_NOT_IN_STATE (a listed slot that
 * is free or holds no landmark, a marg_slot or new_anchor that is no window clone, a table variable beyond the filter's n);
 * INGVIO_E_CAPACITY (a state too wide for the kernels' index maps).  Stage the frame with marg_idx = -1 when the tail drops its clone. */
typedef struct {
    int n_reanchor; const int* lm_slot;   /* table slots of landmarks whose anchor leaves, in the reference's visiting order */
    int new_anchor;                       /* table slot of the target clone (the reference: the window's newest)            */
    int n_erase;    const int* erase_slot;/* landmarks marginalised unconditionally (lost track)                             */
    int n_marg;     const int* marg_slot; /* window clones that leave AFTER the anchor change (margSwPose; key-frame mode: two) */
} ingvio_nominal_tail_block;
int ingvio_nominal_tail(ingvio_ctx* ctx, int b0, int nb, const ingvio_nominal_tail_block* blocks, int lm_cap,
                        int* verdict /* [nb][lm_cap] */, int* status /* [nb], may be NULL */);
/* ---- odometry output of the device-resident loop ----------------------------------------------------------------
 * What the reference publishes at the end of every callback (IngvioFilter.cpp:409-454: _extended_pose rotation, position, velocity and
 * their covariance) and prints after ekfUpdate (a negative diagonal of P, StateManager.cpp:413-421), taken from the table and the live
 * covariance WITHOUT a host synchronisation.  ingvio_odom_begin only enqueues on the context's stream, behind everything already there:
 * one kernel over filters [b0, b0 + nb), one device-to-host copy of the records into a pinned buffer of their own, an event; the table
 * event is recorded behind the kernel, so a later asynchronous stage from the table cannot advance the pose before the record is taken.
 * ingvio_odom_end waits for that event and copies the nb records out: they are those of the state at the moment of _begin, whatever has
 * been staged or launched since.  One slot is pending at a time; the call changes no state, so a partial range is allowed.
 *   run(i); odom_begin(i); stage_tracks_nominal(i + 1, async); fetch_begin(i); run(i + 1); fetch_end(i); odom_end(i)
 * (with a late GNSS epoch or tail: odom_begin(i) behind its run) is a closed loop without a host synchronisation.  (The first call of a
 * context allocates the record buffers.)
 * what: INGVIO_ODOM_COV requests cov_err, INGVIO_ODOM_EUCL cov_pose and cov_vel (it implies COV), INGVIO_ODOM_DIAG the diagonal scan; the
 * values are always written, fields that were not requested are zero.
 * status: INGVIO_ODOM_NONFINITE a non-finite number among the values or cov_err; INGVIO_ODOM_NEG_DIAG diag_min < 0 (with DIAG);
 * INGVIO_ODOM_ABSENT one of the extended pose, bg, ba, extrinsics has no slot (-1) or idx + size > n: its values and its rows and columns
 * of the covariances are zero, the rest of the record is valid.
 * Refused with INGVIO_E_ARG before anything is enqueued, the context unchanged: no nominal table, a bad range, an unknown bit in what, a
 * split frame step pending, any stage from the table that has not run (a frame, an update-only frame, a GNSS epoch, a landmark stage:
 * the table has then already advanced or is about to be read by that run's own order), an ingvio_odom_begin that has not been ended.
 * ingvio_odom_end without a pending _begin: INGVIO_E_ARG.  ingvio_cov_snapshot / _restore are not involved: the record is of the live state. */
#define INGVIO_ODOM_COV 1
#define INGVIO_ODOM_EUCL 2
#define INGVIO_ODOM_DIAG 4
#define INGVIO_ODOM_NONFINITE 1
#define INGVIO_ODOM_NEG_DIAG 2
#define INGVIO_ODOM_ABSENT 4
typedef struct {
    int n;                        /* the filter's state dimension, read on the device                                              */
    int status;                   /* INGVIO_ODOM_NONFINITE | _NEG_DIAG | _ABSENT                                                    */
    int gnss_mask;                /* bit s: gnss[s] is registered (ingvio_nominal_set_gnss)                                        */
    int reserved;
    double R_i2w[9], p[3], v[3];  /* State::_extended_pose, R row-major                                                            */
    double bg[3], ba[3];
    double R_c2i[9], p_c2i[3];    /* _camleft_imu_extrinsics                                                                       */
    double gnss[6];               /* clock bias GPS, GLO, GAL, BDS, then FS, then YOF (State::GNSSType order)                      */
    double diag_min, diag_max;    /* over P[i][i], i < n                                                                           */
    double cov_err[15 * 15];      /* P over (extended pose 9: d_theta, d_p, d_v; bg 3; ba 3) gathered through each variable's idx, in
                                     the filter's own error coordinates; column-major as ingvio_cov_get_marginal, copies bit for bit */
    double cov_pose[6 * 6];       /* (position, orientation) in the world frame and Euclidean error: J_p S J_p^T on the 9 x 9 pose
                                     block S with J_p = [-[p]x I 0; I 0 0] (the retraction p' = Gamma0(dth) p + Gamma1(dth) dp gives
                                     delta p = dp - [p]x dth to first order; dth is a world-axis rotation already); exactly symmetric */
    double cov_vel[3 * 3];        /* J_v S J_v^T, J_v = [-[v]x 0 I]; exactly symmetric                                              */
} ingvio_odom;
int ingvio_odom_begin(ingvio_ctx* ctx, int b0, int nb, int what);
int ingvio_odom_end(ingvio_ctx* ctx, ingvio_odom* out /* [nb] */);
/* ---- MSCKF anchor change and invalid-feature erase on the track store --------------------------------------------
 * changeMSCKFAnchor (KeyframeUpdate.cpp:280-328, SwMargUpdate.cpp:367-413) and eraseInvalidFeatures (MapServerManager.cpp:456-491) for
 * the tracks the host lists from its integer bookkeeping; the depth tests read the store's points and the table's clone poses, which
 * exist only on the device.  Per filter one list of entries  track | anchor_pos << 16 | move << 24:
 *   anchor_pos  a position in the table's window list as it stands at the call's place in the stream (after a run that dropped a clone
 *               the list has closed up; the store's slot numbering plays no part)
 *   move = 1    the track's anchor leaves the window: anchor_pos names the NEW anchor (the reference takes the window's newest clone);
 *   move = 0    anchor_pos names the track's current anchor.
 * has_point is the reference's sticky _isTri (MapServerManager.cpp:292-296, 326-330): set when a point enters the store (pf_track of a
 * delta, a successful device triangulation), cleared by free_tracks, by ingvio_tracks_create and by an erasure of this call.  Per entry:
 *   no point:            move ? INGVIO_MAINTAIN_ERASED_UNTRIANGULATED : INGVIO_MAINTAIN_KEEP
 *   d = (R_a^T (p_f - p_a)).z with the store's point and the pose of the table's clone at anchor_pos
 *   move && d <= move_min_depth (0.3 key-frame mode, 0.0 sliding-window mode):  INGVIO_MAINTAIN_ERASED_MOVE
 *   d <= min_depth (0.2):  INGVIO_MAINTAIN_ERASED_INVALID   (a moved track is tested at its new anchor: no pose changes between the
 *                                                            reference's two steps)
 *   otherwise INGVIO_MAINTAIN_MOVED / INGVIO_MAINTAIN_KEEP.
 * The comparisons are C++'s: a NaN depth is not <= anything and KEEPS the track, as body.z() <= 0.2 does in the reference and in the
 * host shim; -inf erases, +inf keeps.  An erased track loses its mask and has_point exactly as one named in free_tracks; nothing else
 * changes in the store, the table, P or n.  depth is 0 for an entry without a point.
 * lm_slot (optional): table slots of in-state landmarks; each reports INGVIO_MAINTAIN_ERASED_INVALID when the depth of the table's value
 * at its table anchor is <= min_depth, else INGVIO_MAINTAIN_KEEP.  Report only: the caller marginalises them with ingvio_nominal_tail
 * (its erase_slot list).
 * _begin enqueues on the context's stream, behind everything already there: the lists (a small upload kernel reading pinned memory, or a copy), ONE kernel over the filters, the table event (an asynchronous
 * stage on the copy stream - from the table or host-fed - is ordered behind the erasures), one device-to-host copy into a pinned buffer of its own, an event.  _end
 * waits for that event only and copies the verdicts out: row i of verdict / depth has list_cap entries, of lm_verdict lm_cap entries;
 * depth may be NULL.  ingvio_tracks_maintain is _begin + _end.  A partial range is allowed (only the listed filters' store is touched);
 * one call is pending per context; a filter whose lists are empty is untouched, a call whose lists are all empty launches nothing.
 * (A call with longer lists than any before allocates; the context's first call does.)
 * The free-running form  run(i); maintain_begin(i); stage_tracks_nominal(i + 1, async); run(i + 1); maintain_end(i):  the stage of entry
 * i + 1 is built WITHOUT entry i's verdicts.  An erased track to which that stage appends is a restarted track holding that one
 * observation and no point; an erased track that the stage lists as a feature has an empty mask under its selection and drops out of the
 * update as accepted = 0, by the mechanism of a failed triangulation.  At _end the host corrects its bookkeeping of an erased track:
 * mask = the observations since _begin, anchor = the first of them.
 * Refused before anything is enqueued or changed.  INGVIO_E_ARG: no table or no store, a bad range, NULL where data is needed, a list
 * longer than t_max or list_cap (lm_cap), a track outside the store, a track named twice in a filter's list, bits above move, any stage
 * from the table that has not run, a split frame step pending, _begin while one is pending, _end without _begin.
 * INGVIO_E_NOT_IN_STATE: an anchor_pos beyond the host mirror's window, a landmark slot that is free or holds no landmark. */
#define INGVIO_MAINTAIN_KEEP 0
#define INGVIO_MAINTAIN_MOVED 1
#define INGVIO_MAINTAIN_ERASED_UNTRIANGULATED 2
#define INGVIO_MAINTAIN_ERASED_MOVE 3
#define INGVIO_MAINTAIN_ERASED_INVALID 4
typedef struct {
    int n_tracks; const int* tracks;      /* track | anchor_pos << 16 | move << 24                                                  */
    int n_lm; const int* lm_slot;         /* in-state landmarks (table slots), report only                                          */
} ingvio_maintain_block;
typedef struct {
    double move_min_depth, min_depth;
    int list_cap, lm_cap;                 /* entries per filter in the result arrays                                                */
} ingvio_maintain_opts;
int ingvio_tracks_maintain_begin(ingvio_ctx* ctx, int b0, int nb, const ingvio_maintain_block* blocks /* [nb] */, const ingvio_maintain_opts* opts);
int ingvio_tracks_maintain_end(ingvio_ctx* ctx, unsigned char* verdict /* [nb][list_cap] */, double* depth /* [nb][list_cap], may be NULL */,
                               unsigned char* lm_verdict /* [nb][lm_cap] */);
int ingvio_tracks_maintain(ingvio_ctx* ctx, int b0, int nb, const ingvio_maintain_block* blocks, const ingvio_maintain_opts* opts,
                           unsigned char* verdict, double* depth, unsigned char* lm_verdict);
/* ingvio_gnss_front_stage with the receiver taken from the device table: the epoch carries only what the host owns.  p_w, v_w
 * (State::_extended_pose), the clock biases, FS and YOF (GnssUpdate.cpp:98-122 reads them from the state) and every Type::idx() come
 * from the filter's table as the frame that has just run left it - IngvioFilter.cpp:329-362 runs after :276-327 and after margSwPose,
 * so the idx are the shifted ones, and with ingvio_set_gnss_adjust_yof on the YOF column is formed from the table's yaw, p_w and v_w -
 * on the context's stream, without a host round trip; the host-side checks of ingvio_gnss_front_stage
 * (INGVIO_E_NOT_IN_STATE, the capacity checks) are made on the host mirror of the table.  n_sat = 0: no epoch for that filter.
 * The following ingvio_gnss_run (same range, once: a second one is INGVIO_E_ARG) ends with StateManager::boxPlus of the update's dx on
 * the table, on the device (StateManager.cpp:244-251 after GnssUpdate.cpp:290), and keeps its dx / row count / status apart from the
 * frame's, so that ingvio_frame_fetch(_begin / _end) of the same frame is valid before or after it.  ingvio_gnss_fetch is optional.
 *   run(i); fetch_begin(i); gnss_front_stage_nominal(i); gnss_run(i); stage_tracks_nominal(i + 1, async); run(i + 1); fetch_end(i)
 * is a closed loop without a host synchronisation.
 * The stage replaces whatever GNSS rows the context holds staged and not yet run, of any range (one GNSS stage at a time).  If the run
 * itself is refused (INGVIO_E_NOT_IN_STATE, INGVIO_E_CAPACITY of the row gate: both before its first launch) the epoch stays staged.
 * Refused before anything changes: no table (whatever the epochs hold, also when none has a satellite), no registered scalars for a
 * filter with n_sat > 0, a frame staged from the table that has not run (INGVIO_E_ARG); opts->in_frame (INGVIO_E_UNSUPPORTED); the extended pose, YOF or FS not in the table with n_sat > 0
 * (INGVIO_E_NOT_IN_STATE).  While such an epoch is staged and has not run, ingvio_frame_stage_tracks_nominal, ingvio_nominal_set /
 * _box_plus / _set_gnss and ingvio_cov_snapshot return INGVIO_E_ARG; ingvio_cov_restore abandons it. */
typedef struct {
    int n_sat;                                /* <= INGVIO_GNSS_MAX_SAT; 0: no epoch                                   */
    const double* eph;                        /* [n_sat][INGVIO_EPH_N]                                                 */
    const double* obs;                        /* [n_sat][INGVIO_OBS_N]                                                 */
    const double* ion;                        /* [8] Klobuchar parameters or NULL                                      */
    double doy;
    double R_enu2ecef[9], anchor_ecef[3];     /* GvioAligner::getRenu2ecef (row-major), translation of getTenu2ecef    */
    double psr_noise_amp, dopp_noise_amp;     /* GnssUpdate::_psr_noise_amp / _dopp_noise_amp                          */
} ingvio_gnss_epoch_nominal;
int ingvio_gnss_front_stage_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_gnss_epoch_nominal* epochs, const ingvio_gnss_opts* opts);
/* The raw GNSS epoch that belongs to the frame staged from the table: called AFTER ingvio_frame_stage_tracks_nominal of that frame and
 * before its ingvio_frame_run, for the whole batch (the protocol of ingvio_landmark_stage_nominal with in_frame != 0).  The stage only
 * uploads - ephemerides, observations, the host-owned receiver record, the gate table, on the compute stream behind the kernels of the
 * frame enqueued last - and launches nothing: the rows are formed inside ingvio_frame_run, at the state after the MSCKF update of the
 * same frame (IngvioFilter.cpp:277-362), from the table.  It leaves the GNSS results of the frame before alone: ingvio_gnss_fetch of
 * frame i stays valid after the stages of frame i + 1 and is overwritten by ingvio_frame_run of frame i + 1, so
 *   run(i); stage_tracks_nominal(i + 1, async); gnss_frame_stage_nominal(i + 1); fetch_begin(i); gnss_fetch(i); run(i + 1); fetch_end(i)
 * is a closed loop in which the epoch of frame i does not hold back the stage of frame i + 1 (ingvio_gnss_fetch itself is optional).
 * The run applies the epoch in one of two orders and consumes it (it runs once; ingvio_gnss_run on it is INGVIO_E_ARG):
 *   folded      windows of at most 16 clones, at most 8 satellites (16 rows) per filter, every filter marginalises, every GNSS column
 *               below the clone that leaves, no in-frame landmark stage: solve -> MSCKF dx -> boxPlus on the table (no drop, no shift)
 *               -> rows from the table -> posterior columns -> row gates -> gain -> ONE write-back with the GNSS gain and the
 *               marginalisation fused -> one retraction of the GNSS dx with drop and shift.  ingvio_gnss_fetch returns dx in the index
 *               space AFTER the marginalisation, as for ingvio_gnss_stage with in_frame.
 *   otherwise   the frame completes as without the epoch; then the kernels of ingvio_gnss_front_stage_nominal + ingvio_gnss_run run
 *               behind it inside the same call, on the same inputs in the same order: results bit-identical to those two calls.
 * A filter with n_sat = 0 or a rejected block: dx = 0, zero rows, its table moves by the frame alone.  dx, rows, keep, gamma and status
 * of the epoch: ingvio_gnss_fetch; the frame's own dx, row counts and accept masks stay valid for ingvio_frame_fetch(_begin / _end).
 * Refused before anything is launched or changed, on the host mirror of the table: no table, no frame staged from the table waiting to
 * run, a range other than the whole batch, a second such stage for the same frame, no registered scalars for a filter with n_sat > 0,
 * n_sat < 0 or > INGVIO_GNSS_MAX_SAT, a missing array (INGVIO_E_ARG); 2 n_sat rows beyond the row buffers or the update's LDS
 * (INGVIO_E_CAPACITY); the extended pose, YOF or FS not in the table, or a GNSS column that - before or after the frame's marginalisation
 * shift - lies outside the state the update sees or on the clone that leaves (INGVIO_E_NOT_IN_STATE).  ingvio_cov_restore abandons the
 * stage with its frame.  Still refused: opts->in_frame on ingvio_gnss_front_stage(_nominal), a frame staged from the table while a host-fed
 * ingvio_gnss_stage(in_frame) is pending, frame_parts > 1 and the split step with a table (INGVIO_E_UNSUPPORTED). */
int ingvio_gnss_frame_stage_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_gnss_epoch_nominal* epochs, const ingvio_gnss_opts* opts);
/* test hook: how the GNSS update that ran last was applied - 0: no results / ingvio_gnss_run on the frame's slots, 1: a pass of its own
 * with its own result slots, 2: folded into the MSCKF write-back */
int ingvio_debug_gnss_fused_last(ingvio_ctx* ctx);
/* test hook: the retraction kernel of the folded order alone, on the TABLE of filters [b0, b0 + nb) only (the covariance is not touched) -
 * boxPlus of dx [nb][ldp] given in the index space behind the marginalisation of marg_idx[i] (a window clone), then drop and shift.
 * INGVIO_E_NOT_IN_STATE: marg_idx names no window clone or a variable would read beyond its row of dx. */
int ingvio_debug_nominal_update_post(ingvio_ctx* ctx, int b0, int nb, const double* dx, const int* marg_idx);
/* ---- in-state landmarks in the device-resident closed loop -------------------------------------------------------
 * ingvio_landmark_stage with the nominal values taken from the device table: per filter only the observations and the table slots of the
 * landmarks they belong to.  R_i2w, p_i2w (the table's extended pose), R_cl2i, p_c2i (its extrinsics), idx_epose, idx_ext and per
 * landmark lm_idx, anchor_idx (the idx of the slot and of its anchor's slot) and pf (its value) are read on the device at the moment the
 * rows are formed; the checks ingvio_landmark_stage makes on them are made on the host mirror of the table.
 *   opts->in_frame == 0: ingvio_landmark_run of the same range (once: a second one is INGVIO_E_ARG) forms the rows from the table as it
 *     stands, updates the covariance and ends with StateManager::boxPlus of its dx on the table (LandmarkUpdate.cpp:146-147).  While it is
 *     staged and has not run, ingvio_frame_stage_tracks_nominal, ingvio_nominal_set / _box_plus / _set_gnss, ingvio_cov_snapshot and
 *     ingvio_gnss_front_stage_nominal return INGVIO_E_ARG; ingvio_cov_restore abandons it.
 *   opts->in_frame != 0: called AFTER ingvio_frame_stage_tracks_nominal of the frame it belongs to and before its ingvio_frame_run, for
 *     the whole batch.  That run then follows IngvioFilter.cpp:277-324 on the device: MSCKF update -> boxPlus of the frame's dx on the
 *     table -> landmark rows at the UPDATED values -> per-landmark gates -> one stacked update -> boxPlus of the landmark dx (index space
 *     of the update, new clone included) -> drop of the marginalised clone and index shift.  The stage is consumed by the run;
 *     ingvio_cov_restore abandons it with the frame.  The upload is ordered behind the frame enqueued last, so
 *       run(i); stage_tracks_nominal(i + 1, async); landmark_stage_nominal(i + 1); fetch_begin(i); run(i + 1); fetch_end(i)
 *     is a closed loop without a host synchronisation.
 * ingvio_landmark_fetch returns dx / rows / accept / gamma / status as for the host-fed stage; the frame's own dx, row counts and accept
 * masks stay valid for ingvio_frame_fetch(_begin / _end) of the same frame.
 * Refused before anything changes: no table, a table without extended pose or extrinsics, a slot that is free, out of range, named twice
 * or not an INGVIO_NOM_LANDMARK, in_frame != 0 without a pending frame from the table or for a range other than the whole batch,
 * in_frame == 0 with such a frame pending, a GNSS epoch staged from the table that has not run (INGVIO_E_ARG); n_lm > INGVIO_LM_MAX
 * (INGVIO_E_CAPACITY); a variable beyond the live state (INGVIO_E_NOT_IN_STATE).  Still refused with a frame from the table: the host-fed
 * ingvio_landmark_stage with in_frame != 0 and any in-frame GNSS stage (INGVIO_E_UNSUPPORTED). */
typedef struct {
    int n_lm;                       /* <= INGVIO_LM_MAX; 0: no landmark update for this filter                 */
    const int* lm_var;              /* [n_lm] table slots, each of kind INGVIO_NOM_LANDMARK, no duplicates      */
    const double* uv;               /* [n_lm][4] current observation u0 v0 u1 v1 (mono: first two)              */
    const unsigned char* tracked;   /* [n_lm] 1 = observed in this frame (0: the landmark is skipped)           */
} ingvio_landmark_frame_nominal;
int ingvio_landmark_stage_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_landmark_frame_nominal* frames,
                                  const ingvio_landmark_opts* opts);
/* ---- landmark initialisation in the device-resident closed loop ------------------------------------------------
 * LandmarkUpdate::initNewLandmark{Mono,Stereo} (LandmarkUpdate.cpp:399-421, :928-955) for filters [b0, b0 + nb) from what the device
 * already holds: the observations and the 64-bit mask of the track store, the clone poses of the nominal table.  Per filter the
 * candidates are tried in order; for each one
 *   - the rows of calcResJacobianSingleFeatAll{Mono,Stereo}Obs (:426-500, :803-890) are formed on the device at the table's CURRENT clone
 *     poses, for every stored observation of `track` whose store column is not in drop_cols (the reference's
 *     sw_poses.find(time) == end() -> continue).  A store column maps to a window position by the count of dropped columns below it.
 *     var_old_order = the window's clones in ascending time, six columns each; s = 3; two rows per observation (mono) or four
 *     (opts->stereo, R_cl2cr, t_cl2cr), in ascending window position; the anchor's theta block is minus the observer's and both are
 *     absent when the observer is the anchor.  m = rows per observation x observations used;
 *   - addVariableDelayed as one round of ingvio_add_variable_delayed_batch with noise = opts->noise and the threshold
 *     chi2_mult * opts->chi2_table[m] (the quantile at dof m, StateManager.cpp:610-612);
 *   - on acceptance the landmark is entered into the table ON THE DEVICE: kind INGVIO_NOM_LANDMARK, idx = the live n, anchor = the
 *     table slot of window clone `anchor`, p = pf, in the slot the host reserved - candidate j of a filter gets the j-th lowest free
 *     slot of the table at the call's start, a refused candidate leaves its slot free - and then StateManager::boxPlus of the
 *     candidate's trailing dx runs on the table, the new landmark included.  The next candidate's rows are formed after that, as the
 *     reference forms them (ingvio_add_variable_delayed_batch takes every candidate's rows up front).
 * The host takes no decision between the candidates and synchronises once, at the end; then the live sizes and its mirror of the table
 * follow the verdicts.  40 bytes per candidate travel.
 *   added / new_idx / chi2 [nb][cand_cap], dx [nb][cand_cap][ldp] (may be NULL), status [nb] (may be NULL) and the soft
 *     INGVIO_NEG_DIAG / INGVIO_E_NOT_PD return with the stop of that filter's sequence: as ingvio_add_variable_delayed_batch.
 *   slot [nb][cand_cap]: the table slot of the new landmark, -1 when not added.
 *   A candidate whose used observations give m <= 3 is skipped on the device (added = 0, chi2 = 0, state untouched): only the device
 *     knows the mask.  A refused or skipped candidate leaves P, n and the table untouched.
 * Refused before anything changes, from the host mirror only: INGVIO_E_ARG (no table, no track store, range, NULL where data is
 * needed, n_cand > cand_cap, a track outside the store, an anchor outside the window, drop_cols not ascending or outside c_max, window
 * size + n_drop > c_max, chi2_table shorter than rows per observation x window size + 1, a split frame step pending, or a frame / GNSS
 * epoch / landmark stage from the table that has not run); INGVIO_E_NOT_IN_STATE (a window clone beyond the filter's n);
 * INGVIO_E_CAPACITY (fewer free table slots than candidates, n + 3 n_cand > n_max, the worst-case m - every window clone observing -
 * beyond ingvio_mld, more columns than the context holds, and the three LDS bounds of ingvio_add_variable_delayed_batch taken at that
 * worst-case m: the trailing update's S, the single-filter gate's 150 KB, the front's 160 KB - e.g. a stereo candidate on 20 clones;
 * under ingvio_set_delayed_form(ctx, 1) the last two do not refuse: the call's fronts then take the large form, up to 36 clones).
 * Not reproduced: the reference's hasNaN skip of an observation (:479, :866) - a point on a camera's z = 0 plane gives a non-finite
 * chi2 and is refused (with do_chi2 != 0).  The call runs where ingvio_add_variable_delayed_batch runs: between frames, on the window the
 * table holds then; it is not part of ingvio_frame_run.  Which tracks to try, triangulation, the max_landmarks cap and the MapServer's
 * _ftype flag stay the host's. */
typedef struct {
    int track;        /* track-store track of the feature                                                      */
    int anchor;       /* window position (ascending time, AFTER the pending drops) of getAnchoredPose()        */
    double pf[3];     /* _landmark->valuePosXyz() after triangulation                                          */
} ingvio_lm_init_cand;
typedef struct {
    int n_cand; const ingvio_lm_init_cand* cand;      /* tried in this order                                    */
    int n_drop; const int* drop_cols;                 /* store columns whose clone has left the table's window but whose drop has not
                                                         reached the store yet (what the next frame's drop_slots will be), ascending */
} ingvio_lm_init_block;
int ingvio_landmark_init_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_lm_init_block* blocks, const ingvio_msckf_opts* opts,
                                 double chi2_mult, int do_chi2, int cand_cap,
                                 int* added, int* new_idx, int* slot, double* chi2, double* dx, int* status);
/* parity hook (tests): the row formation of ingvio_landmark_init_nominal alone for filter b and one candidate; nothing changes, so
 * neither a free table slot nor room for three more columns is asked for (every other refusal as above).
 * H_old [m x 6 C] and H_new [m x 3] column-major with leading dimension *m_out, res [m]; the caller provides room for
 * m = rows per observation x window size. */
int ingvio_debug_landmark_init_rows(ingvio_ctx* ctx, int b, const ingvio_lm_init_cand* cand, const ingvio_msckf_opts* opts,
                                    int n_drop, const int* drop_cols, double* H_old, double* H_new, double* res, int* m_out);
/* ---- GNSS clock states initialised in the device-resident closed loop ----------------------------------------------
 * GnssUpdate::addNewTrackedSys (GnssUpdate.cpp:295-470, oracle/stream_filter.py::add_new_tracked_sys) for filters [b0, b0 + nb): the
 * frequency shift and the clock bias of every constellation the SPP fix reports and the table lacks are initialised by
 * addVariableDelayed, on the device, from the table.  The sibling of ingvio_landmark_init_nominal on the same front kernel.
 *   Which scalars to try is decided on the host, from its mirror of the table and the SPP fix: candidate 0 (FS) when |vel_spp[3]| > 1e-3
 *     and no FS is registered, candidate 1 + s (clock bias of GPS, GLO, GAL, BDS) when |pos_spp[3 + s]| > 1e-3 and clock s is not
 *     registered.  A filter with n_sat = 0 or without a registered YOF has no candidates (the reference returns silently there, :300;
 *     it is not an error).  Nothing else about the candidates is decided on the host.
 *   Residuals, once per call: the satellite front at the table's receiver state, with the clock biases to add taken from pos_spp[3 + s],
 *     FS from vel_spp[3] when it is to be added (0 when it is neither in the state nor to be added, :362-370), everything else from the
 *     table.  R_w2ecef = R_enu2ecef Rz(YOF) is formed once, from YOF at the call's start (:332), and kept for all rounds.
 *   One round per candidate, in the order above, each against the state the previous round left:
 *     - rows (getResJacobianOfSys, :472-521), one per usable satellite (FS) or per usable satellite of the constellation (a clock), in
 *       ascending satellite order: Hx [m x 10] over [SE23 (9), YOF (1)] with u^T R_w2ecef [x]x in columns 0-2 and -u^T R_w2ecef in columns
 *       6-8 (FS, x = v_w) or 3-5 (a clock, x = p_w); x is read from the table in this round (:397 / :458).  Column 9 is zero, as in
 *       every golden stream, unless ingvio_set_gnss_adjust_yof is on: then it is -u^T R_enu2ecef^T dRz(YOF) x, the reference AS WRITTEN
 *       (:401-404, :462-465: getRecef2enu(), the transpose of what the update rows take), with YOF read from the table in this round
 *       like x (dotRw2enu(state) is evaluated inside the reference's loop) while R_w2ecef of the other columns stays the call's.
 *       H_new is all ones, s = 1; res = -res_vel (FS) or -res_pos (a clock).
 *     - noise = amp * sqrt(mean(ura * std / sin^2 el)) over the rows, computed on the device: std = psr_std, amp = psr_noise_amp for a
 *       clock; std = dopp_std * c / freq, amp = dopp_noise_amp for FS; |sin el| floored at 1e-6.  It is the R of the Givens rounds, of
 *       the gate and of the trailing update, and is returned per candidate.
 *     - the gate: chi2 > chi2_mult * chi2_table[m] refuses (do_chi2 != 0), with the device's m.  m <= 1 is skipped: added = 0, chi2 = 0,
 *       noise = 0, state untouched.
 *     - on acceptance the scalar enters the table ON THE DEVICE: kind INGVIO_NOM_SCALAR, idx = the live n, value vel_spp[3] /
 *       pos_spp[3 + s], in the slot the host reserved - the k-th candidate of a filter gets the k-th lowest free slot at the call's start,
 *       a refused candidate leaves its slot free - and is registered as that GNSS scalar (what ingvio_nominal_set_gnss would do): the IMU
 *       steps of the next frame advance it and later epochs read it.  Then the trailing update on the m - 1 lower rows and
 *       StateManager::boxPlus of its dx on the table, the new scalar included.
 * The host synchronises once, at the end; then the live sizes, its mirror of the table and the GNSS slots follow the verdicts.
 *   added / new_idx / slot / chi2 / noise [nb][INGVIO_GNSS_INIT_CAND], dx [nb][INGVIO_GNSS_INIT_CAND][ldp] (may be NULL), status [nb] (may
 *   be NULL) and the soft INGVIO_NEG_DIAG / INGVIO_E_NOT_PD return with the stop of that filter's sequence: as
 *   ingvio_add_variable_delayed_batch.  A refused or skipped candidate leaves P, n and the table untouched.
 * Refused before anything changes, from the host mirror only: INGVIO_E_ARG (no table, range, NULL where data is needed, n_sat outside
 * 0..64, a missing array, chi2_len <= n_sat, a split frame step pending, a frame / GNSS epoch / landmark stage from the table that has
 * not run); INGVIO_E_NOT_IN_STATE (extended pose or YOF beyond the live state, for a filter with candidates); INGVIO_E_CAPACITY (fewer
 * free table slots than candidates, n + candidates > n_max, n_sat > ingvio_mld).
 * The call runs where ingvio_landmark_init_nominal runs: between frames, after the epoch's ingvio_gnss_run or after an ingvio_frame_run
 * that carried the epoch in-frame.  It is not part of ingvio_frame_run.  The clock indices the next frame's propagation takes
 * (ingvio_frame_step_nominal::gnss_idx) are the host's to extend with new_idx.  checkYofStatus' addGNSSVariable is
 * ingvio_nominal_add_gnss; batchAlign and the SPP fix stay host policy. */
#define INGVIO_GNSS_INIT_CAND 5          /* candidate j: 0 = FS, 1..4 = clock bias GPS, GLO, GAL, BDS: the order of
                                            stream_filter.py:908-911 and host/GnssUpdate.cpp:206-207 */
typedef struct {
    ingvio_gnss_epoch_nominal epoch;     /* n_sat = 0: nothing for this filter */
    double pos_spp[7], vel_spp[4];       /* SppMeas::posSpp / velSpp */
} ingvio_gnss_init_block;
int ingvio_gnss_init_nominal(ingvio_ctx* ctx, int b0, int nb, const ingvio_gnss_init_block* blocks,
                             const double* chi2_table, int chi2_len, double chi2_mult, int do_chi2,
                             int* added, int* new_idx, int* slot, double* chi2, double* noise,   /* [nb][5] */
                             double* dx /* [nb][5][ldp] or NULL */, int* status /* [nb] or NULL */);
/* parity hook (tests): the row formation of ingvio_gnss_init_nominal alone for filter b, its block and candidate g (any of 0..4, tried
 * by the call or not; the receiver is the call's: every scalar the call would add is overridden); nothing changes, so neither a free
 * table slot nor room in the state is asked for.  H_old [m x 10] column-major with leading dimension *m_out, res [m], *noise; the caller
 * provides room for 64 rows.  *m_out = 0: no usable satellite (or no YOF / n_sat = 0). */
int ingvio_debug_gnss_init_rows(ingvio_ctx* ctx, int b, const ingvio_gnss_init_block* block, int g,
                                double* H_old, double* res, double* noise, int* m_out);
int ingvio_frame_run(ingvio_ctx* ctx, int restore_prior);
/* Throughput batches (round 6, an experiment kept selectable): ingvio_frame_run deals the batch to `parts` slices of filters, each
 * on its own HIP stream; the slices' throughput-bound segments (gate + Gram, apply) are chained by events so that only ONE runs at a
 * time while the other slices' latency-bound kernels (restore, propagate, solve) execute beside it.  Consecutive ingvio_frame_run
 * calls pipeline (the slices are not joined at the end of the call); every other entry point, ingvio_sync and ingvio_ctx_stream
 * included, first makes the context's stream wait for them.  Per filter the same kernels with the same arguments: results are
 * bit-identical to parts = 1 (tests/test_gpu_alternatives.py).  parts: -1 / 0 / 1 off (the default: on MI355X the kernels are each
 * sized to fill a CU's LDS and registers alone, co-resident kernels halve each other's occupancy and the split loses),
 * 2..4 slices.  Windows up to 16 clones, factored method, no in-frame landmark stage.  The reference has no counterpart (one filter,
 * one thread: IngvioNode.cpp:36).  Environment override at context creation: INGVIO_FRAME_PARTS. */
int ingvio_set_frame_parts(ingvio_ctx* ctx, int parts);
/* The Gram kernel of the unsplit ingvio_frame_run in its reduced form: windows up to 12 clones solve gauge-reduced, with
 * the newest clone (slot n_clones - 1) as the reference whose block row and column of A the solve deletes, so the kernel does not form
 * them.  Every entry the solve reads is the same sum in the same order: results are bit-identical to the full form
 * (tests/test_gpu_gram_reduced.py).  on: 1 (the default) / 0 the full form everywhere, for comparison.  ingvio_msckf_update*,
 * ingvio_frame_run_phase, the split step, the Selected-timestamp variant, the dense method and windows of more than 12 clones always
 * take the full form.  After a step whose Gram kernel ran reduced ingvio_debug_msckf_info returns INGVIO_E_UNSUPPORTED.
 * Environment override at context creation: INGVIO_GRAM_REDUCED (0 / 1). */
int ingvio_set_gram_reduced(ingvio_ctx* ctx, int on);
/* The reduced form of the Gram kernel as k_feat_gram3 (window classes of up to 6 and up to 11 clones): operand panel and
 * sparse scratch double-buffered, the wave pairs of a workgroup decoupled, one barrier per batch.  The same sums in the same order:
 * results are bit-identical to the reduced k_feat_gram2 (tests/test_gpu_gram_decoupled.py).  on: 1 (the default) / 0 the reduced
 * k_feat_gram2, for comparison.  Has no effect where ingvio_set_gram_reduced has none, nor on 12-clone windows.
 * Environment override at context creation: INGVIO_GRAM_DECOUPLED (0 / 1). */
int ingvio_set_gram_decoupled(ingvio_ctx* ctx, int on);
/* The form the Gram stage of the context's last MSCKF update took: 0 the full form, 1 the reduced k_feat_gram2, 2 the reduced
 * k_feat_gram3.  A negative error code for a null context. */
int ingvio_last_gram_form(ingvio_ctx* ctx);
/* The write-back of ingvio_frame_run's fused step as k_info_apply_res: one workgroup per filter keeps the filter's whole
 * P[:, window columns] in the 160 KB LDS of a CU and sweeps the tiles without workgroup barriers.  Taken for more than 64 filters of the
 * window classes of up to 6 and up to 11 clones, ldp <= 256, with the marginalisation riding on the write-back and no in-frame GNSS
 * fold; everything else keeps k_info_apply whatever the switch says.  The same products in the same order: results are bit-identical
 * (tests/test_gpu_apply_resident.py).  on: 1 (the default) / 0 k_info_apply, for comparison.
 * Environment override at context creation: INGVIO_APPLY_RESIDENT (0 / 1). */
int ingvio_set_apply_resident(ingvio_ctx* ctx, int on);
/* The form the write-back of the context's last MSCKF update took: 1 k_info_apply_res, 0 any other kernel.  A negative error code for
 * a null context. */
int ingvio_last_apply_form(ingvio_ctx* ctx);
/* The route the context's last generic update took (ingvio_ekf_update, ingvio_ekf_update_batch; the dense-H landmark stack records
 * its solve here too, with no product bits).  Read-only, no synchronisation; 0 before the first such update, a negative error code for
 * a null context.  A call refused before its first launch leaves the value of the update before it.
 *   bits 0-1  INGVIO_UPDATE_ROUTE_MASK: INGVIO_UPDATE_LDS k_ekf_core + k_downdate (S in LDS); INGVIO_UPDATE_DENSE_REG the dense-H route
 *             with the register-resident solve k_lm_factor / k_lm_carry (dense workspace of up to 256 rows); INGVIO_UPDATE_DENSE_SWEEP
 *             the dense-H route with the Cholesky sweep out of L2 (k_chol_first / k_chol_step, k_lm_finish).  The workspace only
 *             grows: a context that has solved more than 256 rows keeps the sweep for every later dense-route update.
 *   bits 4-8  (form >> INGVIO_UPDATE_NTM_SHIFT) & INGVIO_UPDATE_NTM_MASK: with INGVIO_UPDATE_DENSE_REG the tile class of the solve
 *             (4, 8, 12, 14 or 16 tiles of 16 rows, chosen from the workspace's row capacity), else 0.
 *   INGVIO_UPDATE_GEMM64_PHT / _S: the product P H^T / S = H (P H^T) ran on k_gemm64 (64 x 64 blocks) instead of k_gemm.
 *   INGVIO_UPDATE_SPLIT_SWEEP: with INGVIO_UPDATE_DENSE_SWEEP, the carried rows were done by one k_chol_carried launch after the
 *             factorisation instead of riding through the panel launches. */
#define INGVIO_UPDATE_ROUTE_MASK 3
#define INGVIO_UPDATE_LDS 1
#define INGVIO_UPDATE_DENSE_REG 2
#define INGVIO_UPDATE_DENSE_SWEEP 3
#define INGVIO_UPDATE_NTM_SHIFT 4
#define INGVIO_UPDATE_NTM_MASK 31
#define INGVIO_UPDATE_GEMM64_PHT 0x200
#define INGVIO_UPDATE_GEMM64_S 0x400
#define INGVIO_UPDATE_SPLIT_SWEEP 0x800
int ingvio_last_update_form(ingvio_ctx* ctx);
/* Which form of the delayed-initialisation front ingvio_add_variable_delayed, ingvio_add_variable_delayed_batch and
 * ingvio_landmark_init_nominal take.  The LDS form keeps [H_old | res], T = Pcc H_old^T and S in LDS at once, which bounds
 * the window (stereo: 17 clones, mono: 21 - 26).  The large form keeps [H_old | res | T^T] in a per-filter workspace in device memory
 * (grown on demand, 8 (2 nc + 1) m bytes per filter, no part of ingvio_cov_snapshot), sweeps it through LDS in panels of 64 columns and
 * holds S as a packed triangle: every window the context accepts (36 clones, m <= 144, nc <= 216) runs.  Same outputs and side effects.
 *   0 (the default): the LDS form only, with its refusals.
 *   1: a candidate that fits the LDS form takes it (bit-identical to mode 0), any other takes the large form.  The front's 160 KB bound
 *      and the single-filter gate's 150 KB bound no longer refuse; m > ingvio_mld, more columns than the context holds, the trailing
 *      update's S beyond LDS (m - s > 141) and n + sum s > n_max still do.  ingvio_landmark_init_nominal chooses once per call, at the
 *      worst-case m of its widest window; ingvio_add_variable_delayed runs a candidate beyond its gate bound as a one-filter call of
 *      the batch path; ingvio_debug_landmark_init_rows forms rows that do not fit LDS in device memory.
 *   2: a test setting - every candidate takes the large form, so that the two forms can be compared on the same inputs.
 * INGVIO_E_ARG: any other value, a split frame step pending, or a frame staged from the nominal table that has not run. */
int ingvio_set_delayed_form(ingvio_ctx* ctx, int mode);
int ingvio_frame_fetch(ingvio_ctx* ctx, int b0, int nb, double* dx_out, int* accepted, int* rows_out);
/* The fetch in two halves (round 6): _begin enqueues the result copies (into pinned memory) behind the frame's kernels and returns;
 * _end waits for them and fills the caller's arrays.  In between the host may stage and LAUNCH the next frame - its kernels queue up
 * behind the copies, the device does not idle while the host unpacks:   run(i); fetch_begin(i); stage_async(i+1); run(i+1); fetch_end(i). */
int ingvio_frame_fetch_begin(ingvio_ctx* ctx, int b0, int nb);
int ingvio_frame_fetch_end(ingvio_ctx* ctx, double* dx_out, int* accepted, int* rows_out);

/* parity hook (tests): the stacked measurement information of filter b's LAST MSCKF update, A_out [ncol][ncol+1] row-major =
 * [sum_j H_j^T H_j | sum_j H_j^T r_j] over the used features in window-slot column order, ncol = 6 * n_clones (caller provides
 * (6 c_max) * (6 c_max + 1) doubles).  Factored method: the gram kernel's partial sums; dense method: R^T R from the TSQR factor.
 * INGVIO_E_UNSUPPORTED after an ingvio_frame_run whose Gram kernel ran in reduced form (ingvio_set_gram_reduced): the partials then
 * lack the reference clone's block row and column. */
int ingvio_debug_msckf_info(ingvio_ctx* ctx, int b, double* A_out, int* ncol_out);

/* parity hook (tests): [M | t] of filter b's last factored update as the solve kernel left it (MP x MP row-major + MP, MP = 6 * window class
 * rounded up to 4); count doubles are copied. */
int ingvio_debug_info_solution(ingvio_ctx* ctx, int b, double* out, int count);

/* parity hook (tests): filter b's slice of the track store, mask [t_max], uv [t_max][c_max][4], pf [t_max][3].  Waits for the context's
 * stream and the copy stream (an asynchronous stage applies its delta there), copies, changes nothing; a NULL array is skipped.
 * INGVIO_E_ARG for a b outside the batch or without a store.  Measurements are meaningful where the mask bit is set: closing a
 * track's row up leaves the old values in the columns it vacates. */
int ingvio_debug_tracks_read(ingvio_ctx* ctx, int b, unsigned long long* mask, double* uv, double* pf);
/* parity hook (tests): filter b's point flags has_point [t_max] of the track store (0 / 1); synchronises as ingvio_debug_tracks_read. */
int ingvio_debug_tracks_flags(ingvio_ctx* ctx, int b, unsigned char* has_point);

/* parity hook (tests): filter b's arrays of the input set the NEXT ingvio_frame_run reads (after an asynchronous stage: the set just
 * staged into), whichever of ingvio_frame_stage(_async) / ingvio_frame_stage_tracks(_nominal) filled it: n_clones [1], n_feat [1],
 * clone_idx [c_max], clone_R [c_max][9], clone_p [c_max][3], anchor [f_max], dof [f_max], obs_mask [f_max], pf [f_max][3],
 * uv [f_max][c_max][4].  Synchronises as ingvio_debug_tracks_read, changes nothing; a NULL array is skipped; INGVIO_E_ARG for a b
 * outside the batch. */
int ingvio_debug_staged_frame(ingvio_ctx* ctx, int b, int* n_clones, int* n_feat, int* clone_idx, double* clone_R, double* clone_p,
                              int* anchor, int* dof, unsigned long long* obs_mask, double* pf, double* uv);

/* debug: shader-clock stamps written by block (0,0) of the instrumented kernels (see dev_common.h) */
int ingvio_debug_read(ingvio_ctx* ctx, long long* out, int n);

/* per-kernel device time, measured with hipEvents on the context's stream.  enable=1 brackets
 * every kernel launch with events (adds launch-side overhead, off by default). */
int ingvio_profile_enable(ingvio_ctx* ctx, int enable);
/* restrict the event pairs to one kernel (name as returned by ingvio_profile_get; NULL or "" = every kernel): the
 * timed region of bench.py brackets only the dominant kernel, an event pair around every launch costs ~6 % */
int ingvio_profile_select(ingvio_ctx* ctx, const char* kernel_name);
int ingvio_profile_reset(ingvio_ctx* ctx);
/* names: array of `cap` char* receiving static strings; ms/calls: [cap]; returns number of entries */
int ingvio_profile_get(ingvio_ctx* ctx, const char** names, double* ms, int* calls, int cap);

#ifdef __cplusplus
}
#endif
#endif
