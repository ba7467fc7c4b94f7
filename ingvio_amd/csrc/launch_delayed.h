// launch_delayed.h — host-side launcher of kernels_delayed.hip: StateManager::addVariableDelayed for a batch of filters, one
// candidate per filter and round (ingvio_add_variable_delayed_batch).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dev_common.h"

// One round: workgroup bl works on candidate `round` of filter b0 + bl.  The per-candidate arrays are this round's slices, [nb] each.
struct DelayedFront {
    CovView cv;
    int b0, nb;
    const double* dbuf;         // packed rows of every candidate of the call
    const size_t* doff;         // [nb] offset (doubles) of [H_old m x nc (ld m) | H_new m x s (ld m) | res m] in dbuf
    const int *m, *s, *nc;      // [nb]; m == 0: no candidate for this filter in this round (or one skipped for m <= s)
    const int* colmap;          // [nb][cs] state column of every column of H_old
    int cs;
    const double* thr;          // [nb] chi2_mult * chi2_check
    int do_chi2;
    double var;                 // noise^2
    double* Hu;                 // [nb][hsu] out: the lower m - s rotated rows, from row 0, ld = mldu (the update's H)
    double* resu;               // [nb][mldu] out: the lower m - s rotated residuals
    int mldu;
    size_t hsu;
    int* mu;                    // [nb] out: rows of the trailing update, m - s when the variable was added, else 0
    double* Y;                  // [nb][ystride] scratch, n x s (ld = ldp)
    size_t ystride;
    const int* status;          // [B] status words of the call's updates; bit 4 (S not positive definite) stops a filter's sequence
    int* added;                 // [nb] out
    int* new_idx;               // [nb] out: the live n at the append, -1 when not added
    double* chi2;               // [nb] out (0 where there was no candidate)
};

// dynamic LDS of one workgroup of k_delayed_front for a candidate (m, s, nc)
size_t delayed_front_lds(int m, int s, int nc);
// lds_bytes: the largest delayed_front_lds of the round's candidates.  -1: beyond the LDS of a CU
int launch_delayed_front(const DelayedFront& L, size_t lds_bytes, hipStream_t st);
