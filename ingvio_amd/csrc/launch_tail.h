// launch_tail.h — host-side descriptor of the landmark tail of a frame (kernels_tail.hip, ingvio_nominal_tail in capi.hip).
#pragma once
#include "dev_common.h"
#include "launch_nominal.h"

// Per filter i of the call (i = b - b0) the uploaded lists, ints at in + i * istride:
//   [TAIL_N_RE] landmarks to re-anchor, [TAIL_NEW] table slot of the target clone, [TAIL_N_ER] landmarks to erase, [TAIL_N_MG] clones that
//   leave, then lm_slot [kcap], erase_slot [ecap], marg_slot [mcap].  A filter whose three counts are zero is skipped by every kernel.
//   An erase_slot may also hold a registered GNSS scalar (ingvio_nominal_marg_gnss): one column leaves and its registration is cleared.
// and the workspace the panel kernel fills for the write-back:
//   nnew [nb]        the state dimension after the call
//   verdict [nb][kcap]   1: re-anchored, 0: behind the new anchor, marginalised (LandmarkUpdate.cpp:298-302)
//   map, tag [nb][ldp]   kept index i -> source index, and the panel column of a re-anchored landmark's row (-1: a plain row)
//   Z [nb][zstride]      n x 3 kcap, ld = ldp: column 3 a + c = column L_a + c of T P T^T in the SOURCE index space (the landmark rows included)
enum { TAIL_N_RE, TAIL_NEW, TAIL_N_ER, TAIL_N_MG, TAIL_HDR };
#define TAIL_LM_MAX 64

struct TailLaunch {
    CovView cv;
    NomTable t;
    int b0, nb;
    const int* in; int istride, kcap, ecap, mcap;
    int* nnew; int* verdict; int* map; int* tag;
    double* Z; size_t zstride;
};

// dynamic LDS of the panel kernel: two ints per column of P
inline size_t tail_panel_lds(int ldp) { return 2 * sizeof(int) * (size_t)ldp; }
#define TAIL_LDS_MAX (48u << 10)

// depth test, panel, index maps and the table (one workgroup per filter); then the compaction with substitution into the other half
// (grid = column tiles x filters) and the flip of cur / n.  Returns -1 without launching when a bound does not hold.
int launch_tail(const TailLaunch& L, int n_cap, hipStream_t st);
