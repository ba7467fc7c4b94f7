// launch_nominal.h — host-side descriptor of the device-resident nominal state (kernels_nominal.hip, ingvio_nominal_* in capi.hip).
#pragma once
#include "dev_common.h"

// Per filter b, two records:
//   ints    ih + b * ir:  [NOM_N_VAR] slots in use, [NOM_N_CLONES], [NOM_V_EXT], [NOM_V_POSE], [NOM_V_BG], [NOM_V_BA],
//                         [NOM_GNSS + s] variable slot of the GNSS scalars (ingvio_nominal_set_gnss): clock bias GPS, GLO, GAL, BDS, then FS,
//                         then YOF (State::GNSSType order, State.h:75); -1: not in the state / not registered,
//                         [NOM_CLONES + q] variable slot of window clone q (ascending time), then [v_max][4] = {kind, idx, anchor slot, 0}
//   doubles dv + b * dr:  gravity (3) + pad, then [v_max][16] = R (9, row-major), p (3), v (3), pad; a Vec3 in p, a Scalar in p[0],
//                         a landmark's world position (AnchoredLandmark::valuePosXyz) in p
enum { NOM_N_VAR, NOM_N_CLONES, NOM_V_EXT, NOM_V_POSE, NOM_V_BG, NOM_V_BA, NOM_GNSS, NOM_CLONES = NOM_GNSS + 6, NOM_IH = NOM_CLONES + 64 };
enum { NOM_G_FS = 4, NOM_G_YOF = 5 };      // positions behind NOM_GNSS (0..3: the clock biases)
enum { NOM_KIND_NONE = -1, NOM_KIND_SE23 = 0, NOM_KIND_SE3 = 1, NOM_KIND_VEC3 = 2, NOM_KIND_SCALAR = 3, NOM_KIND_LM = 4 };
#define NOM_DH 4           // doubles in front of the variables' values (gravity)
#define NOM_VD 16          // doubles per variable

struct NomTable {
    int* ih;
    double* dv;
    int vmax;
    int ir, dr;            // record lengths: NOM_IH + 4 vmax ints, NOM_DH + NOM_VD vmax doubles
};

// StateManager::boxPlus (StateManager.cpp:244-251) of filters [b0, b0 + nb) with dx [b][ldx] (row b of the batch); marg != nullptr: then
// drop the variable whose idx is marg[b] (a window clone, >= 0) and shift every later idx by 6 (StateManager.cpp:155-192)
void launch_nominal_update(const NomTable& t, const double* dx, int ldx, const int* marg, int b0, int nb, hipStream_t st);
// the same end state from a dx given in the index space BEHIND the marginalisation (marg[b] >= 0; a frame whose in-frame GNSS update rode on
// the write-back): each variable reads dx at its shifted idx, the clone that leaves reads nothing, then drop and shift (k_nominal_update_post)
void launch_nominal_update_post(const NomTable& t, const double* dx, int ldx, const int* marg, int b0, int nb, hipStream_t st);

// StateManager::addGNSSVariable (StateManager.cpp:194-231, ingvio_nominal_add_gnss) for filters [b0, b0 + nb): P gains an independent
// 1 x 1 block at the live n and the table a Scalar registered as GNSS scalar.  gs [nb][2] = {position behind NOM_GNSS (-1: nothing for
// this filter), table slot}, vv [nb][2] = {value, variance}, both in device memory
void launch_nominal_add_gnss(const CovView& cv, const NomTable& t, int b0, int nb, const int* gs, const double* vv, hipStream_t st);

// The landmark update's staged inputs (LmView, launch_lmbatch.h) filled from the table: per filter the extended pose and the extrinsics
// into pose [B][24] and their idx into idx [B][2], and for each of the n_lm[b] staged landmarks (slot [B][lmax]: its table slot)
// lm_idx = idx[slot], anchor_idx = idx[anchor[slot]] (-1: no live anchor), pf = p[slot].  Indexed by the ABSOLUTE filter b.
struct NomGather {
    const int* n_lm; const int* slot; int lmax;
    double* pose; int* idx; int* lm_idx; int* anchor_idx; double* pf;
};
// launch_nominal_update without drop and shift, then the gather above from the values it has just retracted, in ONE launch (the
// landmark rows of a frame are formed at the state after the MSCKF update's boxPlus, IngvioFilter.cpp:283-289).  dx == nullptr: gather only.
void launch_nominal_gather(const NomTable& t, const double* dx, int ldx, const NomGather& g, int b0, int nb, hipStream_t st);
