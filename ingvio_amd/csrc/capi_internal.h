// capi_internal.h — what the host translation units behind the C ABI share (capi.hip, capi_delayed.hip, capi_nominal.hip): the
// context struct and the helpers every entry point is written with.  Host code only.  Functions a few lines long that sit on the
// single-filter latency path are inline here; the rest are declared here and defined in capi.hip.
#pragma once
#include "../../include/ingvio_hip.h"
#include "dev_common.h"
#include "launch_ekf.h"
#include "launch_msckf.h"
#include "launch_factored.h"
#include "launch_tri.h"
#include "launch_tracks.h"
#include "launch_lm.h"
#include "launch_delayed.h"
#include "launch_qr.h"
#include "launch_chol.h"
#include "launch_gnss.h"
#include "launch_lmbatch.h"
#include "launch_nominal.h"
#include "launch_tail.h"
#include "launch_odom.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <atomic>
#include <cmath>
#include <functional>
#include <thread>
#include <utility>
#include <vector>

#ifndef UPLOAD_KERNEL_MAX      // host-to-device uploads up to this size travel as a kernel reading the pinned slab (Uploader::copy)
#define UPLOAD_KERNEL_MAX (256u << 10)
#endif

#pragma GCC visibility push(hidden)      // nothing here belongs to the library's dynamic symbol table

namespace capi {

enum ProfId { PF_RESTORE, PF_PROPAGATE, PF_AUGMENT, PF_GATE, PF_FOLD, PF_MERGE, PF_EKF_CORE, PF_DOWNDATE, PF_MARG,
              PF_GATE2, PF_GRAM, PF_INFO, PF_APPLY, PF_ROWGATE, PF_LM_BUILD, PF_LM_GEMM, PF_LM_CHOL, PF_POSTCOLS, PF_COUNT };
inline constexpr const char* kProfNames[PF_COUNT] = { "restore", "k_propagate", "k_augment", "k_msckf_gate", "k_msckf_fold",
                                                      "k_msckf_merge", "k_ekf_core", "k_downdate", "k_marginalize",
                                                      "gate", "gram", "solve", "apply", "k_rows_gate",      // stage slots: bench.py names the kernel that ran
                                                      "k_lm_build", "k_lm_gemm", "k_lm_chol", "k_post_cols" };
struct ProfRec { int id; hipEvent_t a, b; };

}  // namespace capi

struct ingvio_ctx {
    ingvio_ctx_desc d;
    int ldp, mld, nc_cap, G, rstride, hstride, cstride, ystride;
    int cls;                       // CMAX class of the MSCKF kernels
    hipStream_t st;
    bool own_stream;
    std::string err;
    // covariances
    double *Pbase, *Psnap;
    size_t pp = 0;                 // doubles between consecutive filters' covariances (ldp * ldp + pad)
    int *d_cur, *d_n, *d_n_snap;
    std::vector<int> h_n, h_cur, h_n_snap;
    bool has_snap;
    // partial restore: valid while half 0 still equals the snapshot outside the propagation strips, i.e. right after a
    // fused frame step that began with a restore; any other use of the covariance (view()) invalidates it
    int prof_only = -1;          // >= 0: only this kernel id is bracketed by events (ingvio_profile_select)
    bool strip_ok = false;
    std::vector<int> h_nclones;      // per filter: n_clones of the staged frame (picks the window class of the MSCKF kernels)
    // ingvio_gnss_sat_eval's device buffers, grown on demand and kept (psr_pos / dopp_vel call it once per Gauss-Newton iteration,
    // the aligner once per buffered epoch: per-call hipMalloc / hipFree were hundreds of implicit device syncs)
    struct { double *e = nullptr, *o = nullptr, *r = nullptr, *f = nullptr; int cap = 0; } se;
    bool phase_restore = false;      // the pending split step was started with restore_prior
    unsigned long long mut_seq = 0, strip_seq = 0;
    // propagation / structure staging
    double *d_Phi, *d_G, *d_dt, *d_R, *d_blk;      // d_Phi / d_G / d_dt of the frame path: filter b's steps at b * KMAX (fixed slots)
    double* d_prm = nullptr;                        // [B][8] per-filter IMU parameters of the staged frame: sigma[4], sigma_cb, sigma_rw, k, 0
    int *d_gnss, *d_idx;
    int* d_zero_idx = nullptr;      // [B] zeros: "marginalise nothing at 0" = an out-of-place write-back without compaction (frame with landmarks)
    // frame staging
    char* d_result_slab = nullptr;                     // d_dx | d_gamma | d_used | d_m | d_status are views into it; h_result: pinned mirror
    char* h_result = nullptr;
    size_t result_bytes = 0, ro_gam = 0, ro_used = 0, ro_m = 0, ro_st = 0, ro_tok = 0, ro_tpf = 0;      // ro_tok / ro_tpf: triangulation flags and points (ingvio_msckf_update_tri)
    char* d_frame_slab[2] = { nullptr, nullptr };      // the frame arrays below are views into these (frame_slab_carve); [1]: the async set
    int *d_clone_idx, *d_nclones, *d_nfeat, *d_anchor, *d_dof;
    double *d_clone_R, *d_clone_p, *d_pf, *d_uv, *d_chi2;
    unsigned long long* d_mask;
    // msckf / ekf workspaces
    double *d_gamma, *d_Rpart, *d_H, *d_res, *d_noise, *d_noise1, *d_Y, *d_Yc, *d_dx, *d_rec, *d_hnew;
    int method;                    // 0 dense TSQR path, 1 factored (information-form) path
    int *d_accept, *d_used, *d_chunk_used, *d_colmap, *d_m, *d_nc, *d_status, *d_pcbase;
    double *d_big_sg, *d_big_wk;        // large-window workspaces (c_max > 16)
    double* d_Asum = nullptr;           // [B][rstride]: the chunk partials of a filter summed (k_chunk_sum), windows up to 16 clones with G > 1
    int* d_used_sum = nullptr;          // [B]
    // what d_chi2 and d_noise hold (single-filter latency: an update re-sent the same gate table and the same noise variance with every
    // call, two host-to-device copies of ~7 us each in front of the kernels); invalidated by every other writer of those buffers
    struct { std::vector<double> chi2; bool chi2_ok = false; double var = 0.0; int b0 = -1, nb = 0; bool noise_ok = false; } upc;
    int apply_flipped = 0;              // set by run_msckf_factored: the fused marginalisation's flip (cur, n) was done by the write-back kernel itself (k_info_apply)
    bool fork_recorded = false;         // large windows: ev_fork already recorded on the main stream by the caller of run_msckf_factored
    unsigned long long* d_tri_mask = nullptr;      // [B][f_max], allocated on first use: triangulation masks of ingvio_msckf_update_tri
    char* d_imu = nullptr;              // [IMU_SLAB_NB filters] Phi | G | dt | gnss_idx of ingvio_propagate(_fused) in one piece (few filters per call)
    double* d_Tflat = nullptr;          // [min(B, APPLY_FLAT_NB)][ldp * 100]: T of the few-filter apply (k_apply_T_flat), windows up to 16 clones

    int* d_tri_ok;                      // [B][f_max] triangulation flags
    // ingvio_qr_compress, general path: device buffers and the captured launch sequence (~300 kernels) of the last shape
    struct QrCache { int m = 0, n = 0, ldh = 0, chol = 0; double *dA = nullptr, *db = nullptr, *ws = nullptr, *dT = nullptr; hipGraphExec_t exec = nullptr; } qr;
    int qr_method = 0;                  // ingvio_set_qr_method: 0 auto, 1 Householder, 2 Cholesky-QR
    double* d_noiseB = nullptr;         // ingvio_ekf_update_batch: [B][mld] scalar / diagonal noise per filter
    // ingvio_gnss_stage / _run / _fetch: the staged candidate rows of the batch (pristine: every run gates and compacts them
    // into the generic update's working buffers d_H / d_res / d_noiseB)
    struct GnssStage {
        double *H = nullptr, *res = nullptr, *noise = nullptr, *gamma = nullptr, *chi2 = nullptr;
        int *m = nullptr, *nc = nullptr, *colmap = nullptr, *keep = nullptr;
        double *feph = nullptr, *fobs = nullptr, *frcv = nullptr, *front = nullptr;      // ingvio_gnss_front_stage inputs / per-satellite results
        int ncw = 0, m_cap = 0, n_vars_hi = 0, chi2_len = 0, gate_rows = 0, strong = 0;
        double thr1 = 0.0;
        std::vector<int> hi;            // per filter: highest state index named by the staged var_order (+1)
        bool staged = false;
        // in-frame stage (ingvio_gnss_opts::in_frame): applied by ingvio_frame_run.  W [B][ldp * 16]: the var_order columns of the MSCKF
        // posterior (k_post_cols); Yf [B][ldp * 16]: the update's Cholesky-form gain, folded into k_info_apply; its own working rows
        // count / column count / dx (the frame's m, nc and dx slots belong to the MSCKF update)
        bool in_frame = false, fused_last = false;
        bool folded_last = false;      // the update that ran last rode on the MSCKF write-back (ingvio_debug_gnss_fused_last)
        bool results = false;           // an update has run on the current stage: ingvio_gnss_fetch has something to return.  A non-restoring
                                        // ingvio_frame_run CONSUMES an in-frame stage (staged = false, as it does a landmark stage: the rows
                                        // belong to one frame); its results stay fetchable until the next stage
        int nc_max = 0;
        double *W = nullptr, *Yf = nullptr, *dxf = nullptr;
        int *mf = nullptr, *ncf = nullptr;
        // stage from the device nominal state (ingvio_gnss_front_stage_nominal): its run keeps row count, column count, dx
        // AND status apart from the frame's (stf [B]), ends with the retraction of the table and therefore runs once
        // own_status: the status words of the update that ran last are in stf, not in the frame's d_status.  Set by the nominal
        // ingvio_gnss_run and kept after it, so that ingvio_gnss_fetch reads the right words for as long as those results are the
        // current ones; cleared by the next stage of any form (ingvio_gnss_stage, both front stages).
        bool nominal = false, nom_pending = false, own_status = false;
        // frame_nom: the raw epoch of the frame staged from the table (ingvio_gnss_frame_stage_nominal): in_frame and nominal, its front
        // runs inside ingvio_frame_run (the rows exist only there); hi holds the column range BEFORE the frame's marginalisation
        bool frame_nom = false;
        int nom_b0 = 0, nom_nb = 0;
        int* stf = nullptr;
    } gn;
    // dense-H update workspace (kernels_lmbatch.hip + kernels_chol.hip): the batched landmark update and generic updates whose S
    // does not fit in LDS.  Rows live in Hd [m_cap][n_ld] per filter, the sweep in X / Y [ldx][m_cap].
    struct DenseWs {
        double *Hd = nullptr, *X = nullptr, *Y = nullptr, *Tb = nullptr, *U = nullptr, *noise = nullptr, *noiseB = nullptr;      // U: factor tiles of the register-resident solve (m_cap <= 256); noise: one filter's R (ingvio_ekf_update); noiseB [B][m_cap]: scalar / diagonal R per filter (batch)
        int *m = nullptr, *cidx = nullptr, *rowmap = nullptr;      // rowmap [B][m_cap]: the landmark front's accepted rows (k_lm_front)
        int m_cap = 0, n_ld = 0, n32 = 0, ldx = 0;
        size_t hstride = 0, xstride = 0, tstride = 0, ustride = 0;
    } dw;
    struct LmStage {
        double *pose = nullptr, *pf = nullptr, *uv = nullptr, *gamma = nullptr, *dx = nullptr;      // dx: its own [B][ldp] (the frame's MSCKF dx stays in d_dx)
        int *idx = nullptr, *n_lm = nullptr, *lm_idx = nullptr, *anchor_idx = nullptr, *tracked = nullptr, *accept = nullptr;
        LmOpts op;
        int l_hi = 0, in_frame = 0;
        bool alloc = false, staged = false;
        // stage from the device nominal state (ingvio_landmark_stage_nominal): only uv / tracked / n_lm and the landmarks'
        // table slots are uploaded; pose, idx, lm_idx, anchor_idx and pf are filled from the table when the rows are formed
        // (launch_nominal_gather).  nom_pending: the stand-alone form, staged and not yet run (it runs once: its run moves the table)
        int* slot = nullptr;            // [B][LM_MAX]
        bool nominal = false, nom_pending = false;
        int nom_b0 = 0, nom_nb = 0;
        std::vector<int> hi;            // per filter: one past the highest state index the staged rows name (re-checked against the live n at run time)
    } lm;
    char* d_multi = nullptr;            // ingvio_chi2_gamma_multi: packed blocks (grown on demand)
    // ingvio_add_variable_delayed_batch (kernels_delayed.hip), grown on demand: the packed candidates of a call, the rows / row
    // counts its fronts hand to the update kernels, and the results of every round with their pinned mirror
    struct DelayedWs {
        char *in = nullptr, *wk = nullptr, *out = nullptr, *h_out = nullptr; size_t in_cap = 0, wk_cap = 0, out_cap = 0;
        char* ws = nullptr; size_t ws_cap = 0;      // the large form's [H_old | res | T^T] per filter (ingvio_set_delayed_form); no part of a snapshot
        void release();                 // capi_delayed.hip
    } dl;
    size_t multi_cap = 0;
    // staged frame state
    int st_stereo, st_enable_gnss, st_fmax_used;
    std::vector<double> st_prm;    // [B][8] host copy of d_prm (the input set the d_* pointers name)
    MsckfOpts st_op;
    std::vector<int> st_gnss;      // [B][5] clock-state indices of the staged steps (a stage with the same ones keeps the strip restore valid)
    std::vector<int> st_marg;      // per filter marg idx
    std::vector<int> st_cidx_hi;   // per filter: highest staged clone idx (checked against the live state by frame_run)
    bool staged;
    double* d_xchg = nullptr;      // [B][rstride + 8]: [A | b | n_accepted] of the split step's exchange (ingvio_info_reduce / _commit)
    bool phase_pending = false;    // ingvio_frame_run_phase(.., 1) ran and (.., 2) has not yet: the filters are half-stepped (n + 6, no update)
    // second set of device input buffers + copy stream (ingvio_frame_stage_async): the inputs of frame i+1 travel over
    // PCIe while frame i computes; the sets swap roles at every asynchronous stage
    struct InputSet {
        double *Phi = nullptr, *G = nullptr, *dt = nullptr, *R = nullptr, *clone_R = nullptr, *clone_p = nullptr, *pf = nullptr, *uv = nullptr,
               *chi2 = nullptr, *noise = nullptr, *prm = nullptr;
        int *gnss = nullptr, *idx = nullptr, *clone_idx = nullptr, *nclones = nullptr, *nfeat = nullptr, *anchor = nullptr, *dof = nullptr;
        unsigned long long* mask = nullptr;
    } alt;
    bool alt_ready = false;
    // large windows: the measurement-independent front of the Kalman solve runs here, under the gate and the Gram kernel (run_msckf_factored)
    hipStream_t st2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_ref = nullptr;
    hipEvent_t ev_fetch = nullptr;      // ingvio_frame_fetch_begin / _end
    int fetch_b0 = 0, fetch_nb = 0;
    hipStream_t st_copy = nullptr;
    hipEvent_t ev_copy = nullptr, ev_free[2] = { nullptr, nullptr };      // inputs landed / set no longer read by the compute stream
    bool copy_pending = false, free_valid[2] = { false, false };
    int set_id = 0;                                                        // which physical set the d_* pointers name
    // pinned host staging ring: inputs are packed straight into page-locked memory and copied asynchronously; a slab is
    // reused only after the copies issued from it have completed (its event), so no call has to synchronise the stream
    struct PinSlab { char* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool busy = false; };
    PinSlab pin[4];
    int pin_next = 0;
    // Split frame step (round 6): ingvio_frame_run deals the batch to `parts` slices, each with its own stream and
    // its own chain restore -> propagate -> gate -> Gram -> solve -> apply.  The gates are chained by events (slice p's gate starts
    // when slice p - 1's has ended; slice 0's when the LAST slice's of the previous step has), so the slices run half a step apart:
    // the HBM-bound kernels of one slice (apply, propagate, restore) sit under the FP64-bound ones of the other (gate, Gram).
    // The slices' streams are NOT joined at the end of the call - consecutive steps pipeline; every other entry point that touches
    // the context joins them first (join_parts, called through enter()).
    struct PartStream { hipStream_t st = nullptr; hipEvent_t ev_gate = nullptr, ev_apply = nullptr, ev_done = nullptr; };
    PartStream part[4];
    int parts_alloc = 0;
    int parts_req = -1;                 // ingvio_set_frame_parts: -1 automatic, 1 off, 2..4 forced
    int gram_reduced = 1;               // ingvio_set_gram_reduced: the fused frame step may run k_feat_gram2 in its reduced form
    int delayed_form = 0;               // ingvio_set_delayed_form: 0 LDS form only, 1 the large form where the LDS form does not fit, 2 the large form everywhere
    int gnss_adjust_yof = 0;            // ingvio_set_gnss_adjust_yof: GR_ADJ_YOF of every receiver record whose front forms rows
    int gram_decoupled = 1;             // ingvio_set_gram_decoupled: the reduced form runs as k_feat_gram3 in the window classes 6 and 11
    int gram_form_last = 0;             // ingvio_last_gram_form: 0 full, 1 reduced k_feat_gram2, 2 reduced k_feat_gram3
    int apply_resident = 1;             // ingvio_set_apply_resident: the fused frame step's write-back runs as k_info_apply_res where launch_factored can take it
    int apply_form_last = 0;            // ingvio_last_apply_form: 0 k_info_apply (or a few-filter / large-window kernel), 1 k_info_apply_res
    int update_form_last = 0;           // ingvio_last_update_form: route and variants of the last generic update (INGVIO_UPDATE_*)
    int gram_red_last = 0;              // the chunk partials in d_Rpart come from a reduced Gram launch (ingvio_debug_msckf_info refuses them)
    bool split_pending = false;         // slices of the last split step may still be running on their own streams
    hipEvent_t tok_last = nullptr;      // end of the throughput segment issued last (nullptr: none yet / chain broken)
    hipEvent_t ev_split_fork = nullptr;
    hipStream_t run_st = nullptr;       // the stream run_msckf_factored and ProfScope issue on (c->st except inside a split step)
    hipEvent_t tok_wait = nullptr, tok_rec = nullptr;      // run_msckf_factored: wait before / record after its throughput segment (phase 1: gate + Gram, phase 2: apply)
    // device-resident track store (ingvio_tracks_create / ingvio_frame_stage_tracks, kernels_tracks.hip)
    struct Tracks { double *uv = nullptr, *pf = nullptr; unsigned long long* mask = nullptr; int t_max = 0; char* stage[2] = { nullptr, nullptr }; size_t stage_cap = 0;
                    unsigned char* has = nullptr; } trk;      // has [B][t_max]: the track holds a point (TrackStore::has)
    // ingvio_tracks_maintain_begin / _end (k_tracks_maintain, capi_nominal.hip), grown on demand: the uploaded lists, the verdicts and
    // depths on the device and their pinned mirror - its own, as the odometry record's - with the event behind the copy; one call pending
    struct MaintainWs {
        char *in = nullptr, *out = nullptr, *h_out = nullptr; size_t in_cap = 0, out_cap = 0, h_cap = 0;
        hipEvent_t ev = nullptr; bool pending = false, launched = false, ev_recorded = false;      // ev_recorded: a call has launched on this context
        int nb = 0, tcap = 0, lcap = 0, list_cap = 0, lm_cap = 0;
        std::vector<int> cnt;           // [nb][2] the pending call's list lengths
        void release();                 // capi_nominal.hip
    } mt;
    // device-resident nominal state (ingvio_nominal_*, kernels_nominal.hip).  Every change of the integer records (slots,
    // idx, window list) is decided by the host, so it keeps a mirror of them and validates a stage without a device round trip.
    struct Nominal {
        int vmax = 0, ir = 0, dr = 0;
        int* ih = nullptr; double* dv = nullptr;              // the table (launch_nominal.h)
        int* ih_snap = nullptr; double* dv_snap = nullptr;    // ingvio_cov_snapshot's copy
        double* dx = nullptr;                                 // [B][ldp] dx of ingvio_nominal_box_plus
        std::vector<int> h_ih, h_ih_snap;                     // host mirror of the integer records
        bool has_snap = false;
        bool pending = false;                                 // a frame staged from the table has not run yet
        bool frame = false;                                   // the staged frame came from the table (it runs once)
        hipEvent_t ev = nullptr; bool ev_valid = false;       // behind the post-frame kernel of the frame enqueued last
        // update-only frame from the table (ingvio_update_stage_tracks_nominal): no propagation, no new clone; tri_on: its run
        // triangulates the listed features first (tri: the settings); tri_ran: the result slab holds that run's flags and points
        bool noprop = false, tri_on = false, tri_ran = false;
        int tri_fmx = 0;                                      // the largest feature count of the stage that set tri_on
        bool tri_fetched = false; int tri_b0 = 0, tri_nb = 0; // the pinned result mirror holds a triangulating run's flags and points of this range
        ingvio_tri_opts tri;
        int* d_tri_track = nullptr;                           // [B][f_max] track of each listed feature (k_tracks_gather_upd)
        // the triangulating ORDINARY frame from the table (ingvio_frame_stage_tracks_nominal_tri): tri_place 0 - k_triangulate on the compute
        // stream in front of the gate, 1 - at the stage behind the gather (the copy stream of an asynchronous stage), flags and points into
        // d_tri_ok_st / d_tri_pf_st [B][f_max] of its own (the result slab may still wait for the previous frame's fetch); tri_staged: the
        // staged frame's triangulation was issued that way, its run only copies the two into the result slab
        int tri_place = 0;
        bool tri_staged = false;
        int* d_tri_ok_st = nullptr; double* d_tri_pf_st = nullptr;
        void release();                                       // capi_nominal.hip
    } nom;
    // ingvio_nominal_tail (kernels_tail.hip), grown on demand: the uploaded lists, the panel kernel's workspace (transient: nothing in it
    // outlives the call, so a snapshot has nothing to copy) and the pinned mirror of the verdicts and the new dimensions
    struct TailWs {
        char *in = nullptr, *ws = nullptr, *h_out = nullptr; size_t in_cap = 0, ws_cap = 0, out_cap = 0;
        void release();                 // capi_nominal.hip
    } tl;
    // odometry output (ingvio_odom_begin / _end, kernels_odom.hip), allocated by the first _begin: the records [B][ODOM_REC] on the device
    // and their pinned mirror - its own, h_result is shared between the fetches - with the event behind the copy; one slot pending.
    // cols / ns / blk: ingvio_cov_get_marginal_batch's column lists and blocks, grown on demand
    struct OdomOut {
        double *d = nullptr, *h = nullptr; hipEvent_t ev = nullptr; bool pending = false; int b0 = 0, nb = 0;
        int *cols = nullptr, *ns = nullptr; double* blk = nullptr; size_t cols_cap = 0, blk_cap = 0;
        void release();                 // capi_nominal.hip
    } od;
    // profiling
    bool prof;
    std::vector<capi::ProfRec> recs;
    double prof_ms[capi::PF_COUNT];
    int prof_calls[capi::PF_COUNT];
};

namespace capi {

#define HIPCHK(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                    \
            return INGVIO_E_HIP;                                                                \
        }                                                                                       \
    } while (0)

template <class T>
int dalloc(ingvio_ctx* c, T** p, size_t count)
{
    HIPCHK(c, hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
    HIPCHK(c, hipMemsetAsync(*p, 0, sizeof(T) * (count ? count : 1), c->st));
    return 0;
}

// a device buffer grown on demand (never shrunk): frees *p behind a stream synchronisation and allocates the next whole MiB above
// `need`, zero-filled; *cap follows
int dev_grow(ingvio_ctx* c, char** p, size_t* cap, size_t need);

// The read-only view of the covariances; view() counts a use that may change P (it ends the validity of the propagation strips).
inline CovView view_ro(ingvio_ctx* c)
{
    CovView v;
    v.Pbase = c->Pbase; v.cur = c->d_cur; v.n = c->d_n; v.ldp = c->ldp; v.B = c->d.batch; v.pstride = c->pp;
    return v;
}
inline CovView view(ingvio_ctx* c) { ++c->mut_seq; return view_ro(c); }
FrameView fview(ingvio_ctx* c);

struct ProfScope {
    ingvio_ctx* c; int id; hipEvent_t a, b; bool on;
    ProfScope(ingvio_ctx* c_, int id_) : c(c_), id(id_), on(c_->prof && (c_->prof_only < 0 || c_->prof_only == id_))
    {
        if (on) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, c->run_st); }
    }
    ~ProfScope()
    {
        if (on) { hipEventRecord(b, c->run_st); c->recs.push_back({ id, a, b }); }
    }
};

inline int check_range(ingvio_ctx* c, int b0, int nb)
{
    if (!c || b0 < 0 || nb < 1 || b0 + nb > c->d.batch) return INGVIO_E_ARG;
    return 0;
}

// Entry points that change (or snapshot) the covariance refuse to run between the two halves of a split frame step
// (ingvio_frame_run_phase 1 -> 2): the filters are half-stepped there (cloned, not yet updated / marginalised).
int phase_busy(ingvio_ctx* c);

int up(ingvio_ctx* c, void* dst, const void* src, size_t bytes);
int down_sync(ingvio_ctx* c, void* dst, const void* src, size_t bytes);
int last_launch(ingvio_ctx* c);

// status word of the update kernels -> the soft return code of an entry point
inline int soft_status(int st) { return (st & 4) ? INGVIO_E_NOT_PD : ((st & 2) ? INGVIO_NEG_DIAG : INGVIO_OK); }

// The input set a frame step has read may be refilled (ingvio_frame_stage_async) once the kernels enqueued on the compute stream so
// far are done with it.
int release_input_set(ingvio_ctx* c);

// Split frame step: the compute stream waits for the slices' streams (a device-side wait, the host does not block).  Called by every
// entry point other than ingvio_frame_run itself before it touches the context.
int join_parts(ingvio_ctx* c);
#define ENTER(c) do { if ((c) && (c)->split_pending && capi::join_parts(c)) return INGVIO_E_HIP; } while (0)

// device-resident nominal state: the event an asynchronous stage from the table waits for, recorded behind every use of the table on
// the compute stream
int nom_mark(ingvio_ctx* c);
inline NomTable nom_table(ingvio_ctx* c) { return NomTable{ c->nom.ih, c->nom.dv, c->nom.vmax, c->nom.ir, c->nom.dr }; }
inline TrackStore track_store(ingvio_ctx* c) { return TrackStore{ c->trk.uv, c->trk.mask, c->trk.pf, c->trk.t_max, c->d.c_max, c->trk.has }; }
// a GNSS epoch staged from the table (ingvio_gnss_front_stage_nominal) whose update has not run: its rows are linearised at the table's
// present values, so nothing else may move the table or the covariance's bookkeeping in between
// (the same holds for a stand-alone landmark update staged from the table, ingvio_landmark_stage_nominal)
int gnss_nom_busy(ingvio_ctx* c, const char* who);
// the marginalisation on the host mirror of filter b's integer record, exactly as k_nominal_update<true> does it on the device
void nom_mirror_marg(ingvio_ctx* c, int b, int m);
// the host mirror of filter b's integer record: idx of the variable in slot `slot` (-1: none)
inline int nom_idx_of(const ingvio_ctx* c, int b, int slot)
{
    return slot >= 0 ? c->nom.h_ih[(size_t)b * c->nom.ir + NOM_IH + 4 * slot + 1] : -1;
}

// ---- pinned staging ------------------------------------------------------------------------------------------------
struct Uploader {
    ingvio_ctx* c;
    hipStream_t stream = nullptr;      // nullptr: the context's compute stream
    ingvio_ctx::PinSlab* slab = nullptr;
    size_t off = 0;
    int rc = 0;
    int begin(size_t bytes)
    {
        slab = &c->pin[c->pin_next];
        c->pin_next = (c->pin_next + 1) & 3;
        if (slab->busy) { HIPCHK(c, hipEventSynchronize(slab->ev)); slab->busy = false; }
        if (slab->cap < bytes) {
            if (slab->p) hipHostFree(slab->p);
            slab->p = nullptr; slab->cap = 0;
            const size_t cap = (bytes + (1u << 20)) & ~((size_t)(1u << 20) - 1);
            HIPCHK(c, hipHostMalloc((void**)&slab->p, cap, hipHostMallocDefault));
            memset(slab->p, 0, cap);
            slab->cap = cap;
        }
        if (!slab->ev) HIPCHK(c, hipEventCreateWithFlags(&slab->ev, hipEventDisableTiming));
        off = 0;
        return 0;
    }
    template <class T>
    T* take(size_t count)
    {
        off = (off + 63) & ~(size_t)63;
        T* p = reinterpret_cast<T*>(slab->p + off);
        off += sizeof(T) * count;
        return p;
    }
    template <class T>
    void copy(T* dst, const T* src, size_t count)
    {
        const size_t bytes = sizeof(T) * count;
        if (!count) return;
        // small uploads on the compute stream: a kernel that reads the pinned slab (k_upload_words) - no copy-engine hand-over
        if (!stream && bytes <= UPLOAD_KERNEL_MAX && (bytes & 3) == 0 && (((uintptr_t)dst | (uintptr_t)src) & 3) == 0) {
            launch_upload_words(dst, src, bytes, c->st);
            if (hipGetLastError() != hipSuccess) rc = INGVIO_E_HIP;
            return;
        }
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream ? stream : c->st) != hipSuccess) rc = INGVIO_E_HIP;
    }
    // rows of `width` elements at src + r * spitch into dst + r * dpitch: ONE copy (or upload kernel) for a batch of strided rows
    template <class T>
    void copy_rows(T* dst, size_t dpitch, const T* src, size_t spitch, size_t width, size_t rows)
    {
        if (rows == 1 || (width == spitch && width == dpitch)) { copy(dst, src, rows == 1 ? width : width * rows); return; }
        const size_t bytes = sizeof(T) * width * rows;
        if (!width || !rows) return;
        if (!stream && bytes <= UPLOAD_KERNEL_MAX && ((sizeof(T) * (width | spitch | dpitch)) & 3) == 0 && (((uintptr_t)dst | (uintptr_t)src) & 3) == 0) {
            launch_upload_rows(dst, sizeof(T) * dpitch, src, sizeof(T) * spitch, sizeof(T) * width, rows, c->st);
            if (hipGetLastError() != hipSuccess) rc = INGVIO_E_HIP;
            return;
        }
        if (hipMemcpy2DAsync(dst, sizeof(T) * dpitch, src, sizeof(T) * spitch, sizeof(T) * width, rows, hipMemcpyHostToDevice, stream ? stream : c->st) != hipSuccess)
            rc = INGVIO_E_HIP;
    }
    int end()
    {
        if (rc) { c->err = "upload from the pinned staging slab failed (hipMemcpyAsync / k_upload_words launch)"; return rc; }
        HIPCHK(c, hipEventRecord(slab->ev, stream ? stream : c->st));
        slab->busy = true;
        return 0;
    }
};
inline size_t pad64(size_t b) { return (b + 63) & ~(size_t)63; }

// Small host inputs of the covariance operations that return nothing from the device (propagate, clone, marginalise, append):
// copied into the pinned ring first, so the call neither reads caller memory after it returns nor has to wait for the stream -
// a stream synchronisation per call was 15-30 us, four of them made up most of a single filter's 0.09 ms frame (round 4).  A
// failed launch is reported by the call that made it (hipGetLastError), a device fault by the next synchronising call.
struct UpItem { void* dst; const void* src; size_t bytes; };
int stage_small(ingvio_ctx* c, const UpItem* it, int n);

// the generic update's inputs of filter b (rows, residual, column map, counts, noise) into the frame's working buffers; synchronises
int stage_generic(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H, int ldh, int m,
                  const double* res, const double* R, int r_kind, int* nc_out);

// fn(i) for i in [0, n): a few host threads when the batch is large enough to pay for them.  The workers are a process-wide POOL
// (round 6): spawning seven std::threads per call was ~0.2 ms of a 0.3 ms stage call once the hand-over itself had shrunk to 8 KB per
// update.  One user at a time; a second caller (another context staging from another host thread) runs its loop with freshly spawned
// threads as before instead of waiting.
// host_pool_run: job(t) for t = 1 .. T - 1 on the pool's workers and job(0) on the caller; false: the pool is busy (caller falls back)
bool host_pool_run(int T, const std::function<void(int)>& job);

template <class F>
void parallel_for(int n, F fn)
{
    unsigned hw = std::thread::hardware_concurrency();
    int T = (int)(hw ? hw : 1);
    if (T > 8) T = 8;
    if (T > n / 16) T = n / 16;
    if (T <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    const std::function<void(int)> stripe = [&](int t) { for (int i = t; i < n; i += T) fn(i); };
    if (host_pool_run(T, stripe)) return;
    std::vector<std::thread> th;
    int started = 1;                                                     // stripe 0 is this thread's
    try {
        for (int t = 1; t < T; ++t) { th.emplace_back([=]() { for (int i = t; i < n; i += T) fn(i); }); ++started; }
    } catch (...) {                                                      // thread limit reached: the stripes not started run here
    }
    for (int i = 0; i < n; i += T) fn(i);
    for (int t = started; t < T; ++t) for (int i = t; i < n; i += T) fn(i);
    for (auto& x : th) x.join();
}

// the compute stream must not read staged inputs before the copy stream has delivered them
int wait_inputs(ingvio_ctx* c);

}  // namespace capi

#pragma GCC visibility pop
