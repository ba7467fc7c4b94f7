// launch_tracks.h — host-side descriptors of kernels_tracks.hip (device-resident track store + per-frame delta hand-over).
#pragma once
#include "dev_common.h"
#include "launch_nominal.h"

// Per-filter header of a staged delta (ints).  Offsets TRK_OFF_* are positions of the filter's slice in the three upload pools
// (ints / doubles / 64-bit masks); TRK_I_* / TRK_D_* are positions INSIDE that slice.
enum {
    TRK_N_DROP, TRK_APPEND, TRK_N_OBS, TRK_N_FREE, TRK_N_PF, TRK_N_CLONES, TRK_N_FEAT, TRK_K, TRK_HAS_SEL, TRK_MARG,
    TRK_OFF_I, TRK_OFF_D, TRK_OFF_M,
    TRK_I_DROP, TRK_I_FREE, TRK_I_OBS, TRK_I_PF, TRK_I_CIDX, TRK_I_FEAT, TRK_I_GNSS,
    TRK_D_OBS, TRK_D_PF, TRK_D_CR, TRK_D_CP, TRK_D_IMU, TRK_D_STATE,
    TRK_NOM_SLOT, TRK_NOM_IDX, TRK_NOM_NVAR,      // device nominal stage: the new clone's variable slot and idx, the table's slots in use after it
    TRK_NOM_CLK,                                  // device nominal stage: != 0 - the frame is staged with enable_gnss (the registered clocks advance)
    TRK_HDR_USED, TRK_HDR = 32
};

struct TrackStage {                     // one staged delta of filters [b0, b0 + nb): views into the uploaded slab
    const int* hdr;                     // [nb][TRK_HDR]
    const int* ipool;
    const double* dpool;
    const unsigned long long* mpool;
};

struct TrackStore {                     // persistent, per context
    double* uv;                         // [B][tmax][cmax][4]
    unsigned long long* mask;           // [B][tmax]
    double* pf;                         // [B][tmax][3]
    int tmax, cmax;
    unsigned char* has;                 // [B][tmax] 1: the track holds a point (FeatureInfo::_isTri, sticky: MapServerManager.cpp:292-296, 326-330)
};

struct FrameOut {                       // FrameView with writable pointers (the gather kernel fills the staged frame)
    int* clone_idx; double* clone_R; double* clone_p; int* n_clones; int* n_feat; double* pf; int* anchor; unsigned long long* obs_mask;
    double* uv; int* dof; int cmax, fmax;
};

// nom != nullptr: the device-resident nominal state variants (k_imu_steps<true>, k_tracks_gather<true>)
void launch_imu_steps(const TrackStage& ts, int b0, int nb, int kst, double* Phi, double* G, double* dt, double* R, hipStream_t st,
                      const NomTable* nom = nullptr);
void launch_tracks_apply(const TrackStage& ts, const TrackStore& store, int b0, int nb, hipStream_t st);
void launch_tracks_gather(const TrackStage& ts, const TrackStore& store, const FrameOut& fv, int b0, int nb, int* idx_marg, int* gnss_idx, hipStream_t st,
                          const NomTable* nom = nullptr);
// the gather of a frame from the table that may triangulate - the update-only frame (ingvio_update_stage_tracks_nominal) and the ordinary
// one staged with tri (ingvio_frame_stage_tracks_nominal_tri): k_tracks_gather_upd (the kernel keeps the name it was introduced and
// profiled under); tri_mask / tri_track [B][fmax] or nullptr
void launch_tracks_gather_tri(const TrackStage& ts, const TrackStore& store, const FrameOut& fv, int b0, int nb, int* idx_marg, int* gnss_idx, hipStream_t st,
                              const NomTable& nom, unsigned long long* tri_mask, int* tri_track);
// triangulated points (ok == 1) of the listed features into the store's pf
void launch_tracks_store_points(const TrackStore& store, int b0, int nb, const int* n_feat, int fmax, const int* track, const int* ok, const double* pf, hipStream_t st);

// ---- k_tracks_maintain: changeMSCKFAnchor + eraseInvalidFeatures on the store ----
// Per filter of the call a row of `istride` ints in `in`: [TM_N_TRK] listed tracks, [TM_N_LM] listed landmark slots, then tcap entries
// track | window position << 16 | move << 24, then lcap table slots.  Results per filter at the same stride tcap + lcap: a verdict byte
// and the depth (0 where no depth was formed) per entry, the landmarks behind the tracks.
enum { TM_N_TRK, TM_N_LM, TM_HDR = 4 };
enum { TM_KEEP = 0, TM_MOVED = 1, TM_ERASED_UNTRIANGULATED = 2, TM_ERASED_MOVE = 3, TM_ERASED_INVALID = 4 };
struct TrackMaintain {
    const int* in; int istride, tcap, lcap;
    double move_min_depth, min_depth;
    unsigned char* verdict; double* depth;      // [nb][tcap + lcap]
};
void launch_tracks_maintain(const TrackStore& store, const NomTable& nom, const TrackMaintain& tm, int b0, int nb, hipStream_t st);
