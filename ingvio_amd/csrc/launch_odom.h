// launch_odom.h — host-side descriptors of the odometry record and the batched marginal getter (kernels_odom.hip; ingvio_odom_begin /
// _end and ingvio_cov_get_marginal_batch in capi.hip).
#pragma once
#include "dev_common.h"
#include "launch_nominal.h"

// The record of one filter as the kernel writes it: ODOM_REC doubles, the image of `ingvio_odom` (include/ingvio_hip.h; capi.hip
// asserts that the two agree).  The first two doubles hold four ints: n, status, gnss_mask, 0.
enum {
    ODOM_HDR = 2,                      // doubles taken by the four ints
    ODOM_O_VAL = 0,                    // behind the header: R_i2w 9, p 3, v 3, bg 3, ba 3, R_c2i 9, p_c2i 3, gnss 6
    ODOM_N_VAL = 39,
    ODOM_O_DIAG = ODOM_O_VAL + ODOM_N_VAL,      // diag_min, diag_max
    ODOM_O_ERR = ODOM_O_DIAG + 2,      // cov_err, 15 x 15 column-major
    ODOM_O_POSE = ODOM_O_ERR + 225,    // cov_pose 6 x 6
    ODOM_O_VEL = ODOM_O_POSE + 36,     // cov_vel 3 x 3
    ODOM_BODY = ODOM_O_VEL + 9,
    ODOM_REC = ODOM_HDR + ODOM_BODY
};
enum { ODOM_W_COV = 1, ODOM_W_EUCL = 2, ODOM_W_DIAG = 4 };                  // `what` (INGVIO_ODOM_*)
enum { ODOM_S_NONFINITE = 1, ODOM_S_NEG_DIAG = 2, ODOM_S_ABSENT = 4 };      // `status`
#define MARG_NS_MAX 64                 // columns of one filter's list in k_cov_marginal (INGVIO_MARGINAL_NS_MAX)

// the records of filters [b0, b0 + nb) into rec + b * ODOM_REC (indexed by the ABSOLUTE filter b), read from the table and the live P
void launch_odom_out(const NomTable& t, const CovView& cv, double* rec, int b0, int nb, int what, hipStream_t st);
// filter b0 + i: the ns[i] x ns[i] block of the live P over the columns cols [i][ns_max] (each in [0, n)), column-major and packed, to
// out + i * ns_max * ns_max
void launch_cov_marginal(const CovView& cv, const int* cols, const int* ns, int ns_max, double* out, int b0, int nb, hipStream_t st);
