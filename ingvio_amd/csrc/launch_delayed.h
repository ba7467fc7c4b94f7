// launch_delayed.h — host-side launcher of kernels_delayed.hip: StateManager::addVariableDelayed for a batch of filters, one
// candidate per filter and round (ingvio_add_variable_delayed_batch).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dev_common.h"
#include "launch_gnss.h"
#include "launch_tracks.h"

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

// The rows of a round formed on the device (ingvio_landmark_init_nominal): LandmarkUpdate::calcResJacobianSingleFeatAll{Mono,Stereo}Obs
// (LandmarkUpdate.cpp:426-500, :803-890) of one track per filter, from the track store's observations and the nominal table's clone
// poses as they stand when the round starts.  With it the front ignores dbuf / doff / m / s / nc / colmap / thr of DelayedFront.
struct DelayedRows {
    NomTable nt;
    TrackStore ts;
    const int* track;                   // [nb] track of the round's candidate, -1: none for this filter
    const int* anchor;                  // [nb] window position of the anchor clone
    const int* slot;                    // [nb] table slot reserved for the landmark
    const double* pf;                   // [nb][3]
    const unsigned long long* dropm;    // [nb] store columns whose clone has left the window (pending drops)
    const double* chi2;                 // chi2_table[dof], at least rows per observation * window size + 1 entries
    double chi2_mult;
    int stereo;
    double R_lr[9], t_lr[3];
    int* nc_out;                        // [nb] out: 6 * window size (the trailing update's column count)
    int* colmap_out;                    // [nb][cs] out: state column of every column of H_old (cs of DelayedFront)
    int* slot_out;                      // [nb] out: the slot the landmark was entered at, -1 when not added
};

// The rows of a round formed on the device from GNSS satellites (ingvio_gnss_init_nominal): GnssUpdate::addNewTrackedSys
// (GnssUpdate.cpp:375-470, getResJacobianOfSys :472-521) for candidate scalar g of every filter - g = 0 the frequency shift (rows: every
// usable satellite, x = v_w, -u^T R_w2ecef in columns 6-8, res = -res_vel), g = 1..4 the clock bias of GPS, GLO, GAL, BDS (rows: the usable
// satellites of that constellation, x = p_w, columns 3-5, res = -res_pos).  Hx has 10 columns over [SE23 (9), YOF (1)]; u^T R_w2ecef [x]x
// in columns 0-2; column 9 stays zero unless the receiver record's GR_ADJ_YOF is set (ingvio_set_gnss_adjust_yof), then it is
// -u^T R_enu2ecef^T dRz(YOF) x as the reference writes it (:401-404, :462-465: getRecef2enu(), not the getRenu2ecef() of the update rows),
// YOF read from the table when the round runs like x; H_new is all ones, s = 1.  x is read from the table when the round runs;
// the residuals, lines of sight and elevations are those of k_gnss_front at the call's start, and so is R_w2ecef (Rw).  The noise of the
// round, amp * sqrt(mean(ura * std / sin^2 el)) over the rows, is computed by the front and is the R of its gate and of the trailing update.
// With it the front ignores dbuf / doff / m / s / nc / colmap / thr / var of DelayedFront.
struct DelayedGnssRows {
    NomTable nt;
    const double* front;                // [nb][64][GF_N] per-satellite records of k_gnss_front
    const double* eph;                  // [nb][smax][GE_N]
    const double* obs;                  // [nb][smax][GO_N]
    const double* rcv;                  // [nb][GR_N]
    int smax;
    const double* Rw;                   // [nb][9] R_w2ecef = R_enu2ecef Rz(YOF) at the call's start, row-major
    int g;                              // the round's candidate: 0 = FS, 1..4 = clock bias GPS, GLO, GAL, BDS
    const int* cand;                    // [nb] 1: the filter tries candidate g
    const int* slot;                    // [nb] table slot reserved for the scalar
    const double* value;                // [nb] its initial value (SppMeas::velSpp[3] / posSpp[3 + sys])
    const double* chi2;                 // chi2_table[dof], more than 64 satellites never arrive: 65 entries
    double chi2_mult;
    double* noise_out;                  // [nb] out: the round's noise (0 where nothing was tried)
    double* var_out;                    // [nb] out: noise^2, the trailing update's R (EkfLaunch::noise with nstride = 1)
    int* nc_out;                        // [nb] out: 10
    int* colmap_out;                    // [nb][cs] out
    int* slot_out;                      // [nb] out: the slot the scalar was entered at, -1 when not added
};

// The large form of the front (k_delayed_front_large, ingvio_set_delayed_form): [H_old | res | T^T] lives in a per-filter workspace
// in device memory and passes through LDS in column panels, so m and nc are bounded by the context, not by LDS.
struct DelayedLarge {
    double* ws;                 // [nb][ws_stride]: (2 nc + 1) columns of ldw doubles per filter
    size_t ws_stride;           // >= (2 nc + 1) * ldw for every candidate of the launch
    int ldw;                    // >= m of every candidate of the launch
    const int* sel;             // [nb] or null: 0 = the filter is not this launch's (left untouched), null = every filter is
};

// dynamic LDS of one workgroup of k_delayed_front for a candidate (m, s, nc)
size_t delayed_front_lds(int m, int s, int nc);
// lds_bytes: the largest delayed_front_lds of the round's candidates.  -1: beyond the LDS of a CU
int launch_delayed_front(const DelayedFront& L, size_t lds_bytes, hipStream_t st);
// the same with the rows formed in LDS from the track store and the nominal table (template instantiation <true>); an accepted
// candidate is also entered into the table.  lds_bytes: delayed_front_lds of the widest window with every clone observing
int launch_delayed_front_rows(const DelayedFront& L, const DelayedRows& R, size_t lds_bytes, hipStream_t st);
// test hook: the row formation alone for filter b (entry 0 of R's arrays) -> out = [H_old m x nc (ld m) | H_new m x 3 | res m], *m_out
int launch_delayed_rows_debug(const DelayedRows& R, int b, double* out, int* m_out, size_t lds_bytes, hipStream_t st);

// dynamic LDS of one workgroup of k_delayed_front_large for a candidate (m, s, nc)
size_t delayed_front_large_lds(int m, int s, int nc);
// the large form of launch_delayed_front / launch_delayed_front_rows: same inputs, outputs and side effects.  lds_bytes: the largest
// delayed_front_large_lds of the launch's candidates.  -1: beyond the LDS of a CU, or no workspace
int launch_delayed_front_large(const DelayedFront& L, const DelayedLarge& G, size_t lds_bytes, hipStream_t st);
int launch_delayed_front_rows_large(const DelayedFront& L, const DelayedRows& R, const DelayedLarge& G, size_t lds_bytes, hipStream_t st);
// test hook for windows whose rows do not fit LDS: out = [H_old m x nc | res m | H_new m x 3], column stride m, (nc + 4) m doubles
int launch_delayed_rows_debug_large(const DelayedRows& R, int b, double* out, int* m_out, hipStream_t st);

// ---- GNSS rows (ingvio_gnss_init_nominal): the LDS form only, m <= 64 rows on 10 columns ----
// R_w2ecef of filters [b0, b0 + nb) from the table's YOF and the receiver records' R_enu2ecef -> Rw [nb][9]
void launch_delayed_gnss_rw(const NomTable& nt, const double* rcv, int b0, int nb, double* Rw, hipStream_t st);
// the front with the rows formed from the satellite records (instantiation DL_GNSS); an accepted scalar is entered into the table and
// registered as GNSS scalar.  lds_bytes: delayed_front_lds(64, 1, 10)
int launch_delayed_front_gnss(const DelayedFront& L, const DelayedGnssRows& R, size_t lds_bytes, hipStream_t st);
// test hook: the row formation alone for filter b (entry 0 of R's arrays) -> out = [H_old m x 10 (ld m) | res m | noise], *m_out
int launch_delayed_gnss_rows_debug(const DelayedGnssRows& R, int b, double* out, int* m_out, hipStream_t st);
