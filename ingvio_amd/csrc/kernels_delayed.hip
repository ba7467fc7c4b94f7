// kernels_delayed.hip — StateManager::addVariableDelayed (StateManager.cpp:547-630) for a batch: k_delayed_front, one workgroup
// per filter, does for one candidate variable what the single-filter path does with k_delayed_qr + k_gamma + a host decision +
// k_delayed_add (kernels_lm.hip / kernels_ekf.hip):
//   1. [H_old | res] and H_new are staged in LDS (every load of the rows is in flight at once).
//   2. One lane derives the s (m - 1) Givens rotations from H_new (:580-592).  They depend on H_new only, so the other waves
//      form T = Pcc H_old^T (nc x m) from the filter's live covariance at the same time: the gate's loads of P run beside the
//      serial part, not behind it.  Rotating the rows of H_old rotates the columns of T by the same list (T Q = Pcc (Q^T H)^T).
//   3. Every column of [H_old | res | T^T] is swept by its own lane with the running carry of k_delayed_qr, in LDS.
//   4. S = Hup Pcc Hup^T + sigma^2 I of the lower m - s rows from the rotated H and T, bordered by the residual; the elimination
//      leaves chi2 = resup^T S^-1 resup (:604-611).
//   5. chi2 > chi2_mult chi2_check && do_chi2 (:614-618): refused, nothing written but the verdict.  Otherwise
//      addVariableDelayedInvertible with the upper s rows (:461-543, as k_delayed_add), n += s, and the lower rows go to the
//      update's buffers from row 0 with their count in mu[bl]: k_ekf_core / k_downdate of the same round do the ekfUpdate.
// k_delayed_front<true> (ingvio_landmark_init_nominal) replaces step 1: the rows are not loaded but FORMED in LDS, one lane per store
// column of the candidate's track, from the track store's observations and the nominal table's clone poses
// (calcResJacobianSingleFeatAll{Mono,Stereo}Obs, LandmarkUpdate.cpp:426-500 / :803-890); an accepted candidate is entered into the table.
// k_delayed_front<DL_GNSS> (ingvio_gnss_init_nominal) forms them one lane per satellite from the records of k_gnss_front and the table's
// extended pose (GnssUpdate::addNewTrackedSys, GnssUpdate.cpp:375-470), computes the round's noise itself and registers an accepted
// clock state in the table.  The template argument is the row source: DL_HOST (<false> before), DL_LM (<true>), DL_GNSS.
// No atomics, no global round trip inside the rotation loop.  FP64, gfx950 only.
#include <type_traits>

#include "dev_common.h"
#include "launch_delayed.h"
#include "lm_small.h"

#define DL_NT 256
#define DL_SMAX 6
#define DL_IB 8

namespace {

struct DelayedLds { size_t A, Hn, CS, S, sm, col, bytes; int ldA; };      // offsets in doubles (every one even: 16-byte aligned)

__host__ __device__ inline DelayedLds delayed_carve(int m, int s, int nc)
{
    auto even = [](size_t x) { return (x + 1) & ~(size_t)1; };
    DelayedLds L;
    const int mu = m - s;
    L.ldA = m | 1;                                           // odd: the lanes of the sweep (one column each) fall on different banks
    L.A = 0;                                                 // [2 nc + 1][ldA]: H_old columns, res, the rows of T
    L.Hn = even(L.A + (size_t)(2 * nc + 1) * L.ldA + DL_IB); // [s][m]      (+ DL_IB: the T product reads whole row groups)
    L.CS = even(L.Hn + (size_t)s * m);                       // [s][m][2]
    L.S = even(L.CS + 2 * (size_t)s * m);                    // [mu + 1][mu + 1]
    L.sm = even(L.S + (size_t)(mu + 1) * (mu + 1));          // 4 x [6][6]
    L.col = even(L.sm + 4 * DL_SMAX * DL_SMAX);              // nc ints
    L.bytes = 8 * L.col + 4 * (((size_t)nc + 3) & ~(size_t)3);
    return L;
}

struct NoRows {};

// The store columns of a track whose rows are formed: a stored observation, not a pending drop, its window position (the count of
// columns below it that are not dropped) inside the window of cw clones (and inside the store's cmax columns).  Uniform over the workgroup.
__device__ __forceinline__ unsigned long long rows_used(unsigned long long mask, unsigned long long dm, int cw, int cmax)
{
    unsigned long long um = 0ULL;
    int q = 0;
    for (int c = 0; c < cmax && c < 64 && q < cw; ++c) {
        if ((dm >> c) & 1ULL) continue;
        um |= mask & (1ULL << c);
        ++q;
    }
    return um;
}

// Lane c = store column c of filter b's candidate (entry bl of r's arrays): its two (mono) or four (stereo) rows of
// [H_old | res] into sA (column stride ldA, residual in column nc) and of H_new into sHn (column stride m).  Only the non-zero
// blocks are written: the observer's six columns, the anchor's theta block (minus the observer's; both absent when the observer is
// the anchor, LandmarkUpdate.cpp:470-474) and H_new.  Rows in ascending window position.
__device__ __forceinline__ void rows_form(const DelayedRows& r, int b, int bl, unsigned long long um, unsigned long long dm, int c, int m, int nc,
                                          double* sA, int ldA, double* sHn)
{
    if (!((um >> c) & 1ULL)) return;
    const unsigned long long below = (1ULL << c) - 1ULL;
    const int q = c - __popcll(dm & below), row = (r.stereo ? 4 : 2) * __popcll(um & below), anc = r.anchor[bl];
    const int* I = r.nt.ih + (size_t)b * r.nt.ir;
    const double* x = r.nt.dv + (size_t)b * r.nt.dr + NOM_DH + (size_t)I[NOM_CLONES + q] * NOM_VD;
    const double* pf = r.pf + 3 * (size_t)bl;
    const double4 uv4 = *reinterpret_cast<const double4*>(r.ts.uv + (((size_t)b * r.ts.tmax + r.track[bl]) * r.ts.cmax + c) * 4);
    const double uv[4] = { uv4.x, uv4.y, uv4.z, uv4.w };
    double RT[9], A[9], pc[3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) RT[3 * i + k] = x[3 * k + i];                          // R_cm2w^T
    const double d[3] = { pf[0] - x[9], pf[1] - x[10], pf[2] - x[11] };
    for (int i = 0; i < 3; ++i) {
        pc[i] = RT[3 * i] * d[0] + RT[3 * i + 1] * d[1] + RT[3 * i + 2] * d[2];            // pf_cm
        A[3 * i] = RT[3 * i + 1] * pf[2] - RT[3 * i + 2] * pf[1];                          // R_cm2w^T skew(pf_w)
        A[3 * i + 1] = RT[3 * i + 2] * pf[0] - RT[3 * i] * pf[2];
        A[3 * i + 2] = RT[3 * i] * pf[1] - RT[3 * i + 1] * pf[0];
    }
    for (int cam = 0; cam < (r.stereo ? 2 : 1); ++cam) {
        double p[3], J[6];                                                                 // H_proj, for the right camera H_proj_r R_cl2cr
        if (cam == 0) {
            for (int i = 0; i < 3; ++i) p[i] = pc[i];
            J[0] = 1.0 / p[2]; J[1] = 0.0; J[2] = -p[0] / (p[2] * p[2]);
            J[3] = 0.0; J[4] = 1.0 / p[2]; J[5] = -p[1] / (p[2] * p[2]);
        } else {
            for (int i = 0; i < 3; ++i) p[i] = r.R_lr[3 * i] * pc[0] + r.R_lr[3 * i + 1] * pc[1] + r.R_lr[3 * i + 2] * pc[2] + r.t_lr[i];
            const double h0 = 1.0 / p[2], h2 = -p[0] / (p[2] * p[2]), h5 = -p[1] / (p[2] * p[2]);
            for (int k = 0; k < 3; ++k) { J[k] = h0 * r.R_lr[k] + h2 * r.R_lr[6 + k]; J[3 + k] = h0 * r.R_lr[3 + k] + h5 * r.R_lr[6 + k]; }
        }
        for (int rr = 0; rr < 2; ++rr) {
            const int ro = row + 2 * cam + rr;
            for (int j = 0; j < 3; ++j) {
                const double ht = J[3 * rr] * A[j] + J[3 * rr + 1] * A[3 + j] + J[3 * rr + 2] * A[6 + j];
                const double hf = J[3 * rr] * RT[j] + J[3 * rr + 1] * RT[3 + j] + J[3 * rr + 2] * RT[6 + j];
                sHn[ro + j * m] = hf;
                sA[ro + (size_t)(6 * q + 3 + j) * ldA] = -hf;
                if (q != anc) { sA[ro + (size_t)(6 * q + j) * ldA] = ht; sA[ro + (size_t)(6 * anc + j) * ldA] = -ht; }
            }
            sA[ro + (size_t)nc * ldA] = uv[2 * cam + rr] - p[rr] / p[2];
        }
    }
}

// The satellites whose rows candidate r.g of filter entry bl takes (bit = satellite), ranked by ballot as k_gnss_front ranks its rows.
// lane = satellite; every lane of the wave must be active.
__device__ __forceinline__ unsigned long long gnss_rows_used(const DelayedGnssRows& r, int bl, int lane)
{
    bool sel = false;
    if (lane < r.smax && lane < (int)r.rcv[(size_t)bl * GR_N + GR_NSAT]) {
        const bool usable = r.front[((size_t)bl * 64 + lane) * GF_N + 9] != 0.0;
        const int sys = (int)r.eph[((size_t)bl * r.smax + lane) * GE_N + GE_SYS];
        sel = usable && (r.g == 0 || sys == r.g - 1);
    }
    return __ballot(sel);
}

// Lane = satellite of filter b (entry bl of r's arrays): its row of [H_old | res] into sA (column stride ldA, residual in column nc) and its
// noise term ura std / sin^2 el into sW, both at the satellite's rank.  Only the non-zero blocks are written.
__device__ __forceinline__ void gnss_rows_form(const DelayedGnssRows& r, int b, int bl, unsigned long long um, int lane, int nc,
                                               double* sA, int ldA, double* sW)
{
    if (!((um >> lane) & 1ULL)) return;
    const int row = __popcll(um & ((1ULL << lane) - 1ULL));
    const bool fs = r.g == 0;
    const int* I = r.nt.ih + (size_t)b * r.nt.ir;
    const double* x = r.nt.dv + (size_t)b * r.nt.dr + NOM_DH + (size_t)I[NOM_V_POSE] * NOM_VD + (fs ? 12 : 9);      // v_w or p_w, as the table holds it now
    const double* fr = r.front + ((size_t)bl * 64 + lane) * GF_N;
    const double* Rw = r.Rw + 9 * (size_t)bl;
    const double u[3] = { fr[2], fr[3], fr[4] };
    double uR[3];                                                      // u^T R_w2ecef
    for (int c = 0; c < 3; ++c) uR[c] = u[0] * Rw[c] + u[1] * Rw[3 + c] + u[2] * Rw[6 + c];
    const double h[3] = { uR[1] * x[2] - uR[2] * x[1], uR[2] * x[0] - uR[0] * x[2], uR[0] * x[1] - uR[1] * x[0] };      // u^T R [x]x
    for (int c = 0; c < 3; ++c) {
        sA[row + (size_t)c * ldA] = h[c];
        sA[row + (size_t)((fs ? 6 : 3) + c) * ldA] = -uR[c];
    }
    const double* rc = r.rcv + (size_t)bl * GR_N;
    if (rc[GR_ADJ_YOF] != 0.0) {
        // is_adjust_yof, as the reference writes it (GnssUpdate.cpp:401-404, :462-465): -u^T R_ecef2enu dRz(yaw) x with getRecef2enu(), the
        // TRANSPOSE of the R_enu2ecef the update rows take, and yaw read from the table in the round like x (dotRw2enu(state) sits inside
        // the reference's loop).  dRz x = (-s x0 - c x1, c x0 - s x1, 0): rows 0 and 1 of R_enu2ecef against u.
        const double yaw = r.nt.dv[(size_t)b * r.nt.dr + NOM_DH + (size_t)I[NOM_GNSS + NOM_G_YOF] * NOM_VD + 9];
        const double cy = cos(yaw), sy = sin(yaw);
        const double uE0 = u[0] * rc[GR_RENU] + u[1] * rc[GR_RENU + 1] + u[2] * rc[GR_RENU + 2];
        const double uE1 = u[0] * rc[GR_RENU + 3] + u[1] * rc[GR_RENU + 4] + u[2] * rc[GR_RENU + 5];
        sA[row + (size_t)9 * ldA] = -(uE0 * (-sy * x[0] - cy * x[1]) + uE1 * (cy * x[0] - sy * x[1]));
    }
    sA[row + (size_t)nc * ldA] = -(fs ? fr[1] : fr[0]);
    const double* ep = r.eph + ((size_t)bl * r.smax + lane) * GE_N;
    const double* ob = r.obs + ((size_t)bl * r.smax + lane) * GO_N;
    double se = sin(fr[6]);
    if (fabs(se) < 1e-6) se = 1e-6;
    const double sd = fs ? ob[GO_DOPP_STD] * 2.99792458e8 / ob[GO_FREQ] : ob[GO_PSR_STD];
    sW[row] = ep[GE_URA] * sd / (se * se);
}

// KIND: where the rows come from - DL_HOST the call's packed rows, DL_LM formed from the track store (ingvio_landmark_init_nominal),
// DL_GNSS formed from the satellite records of k_gnss_front (ingvio_gnss_init_nominal)
enum { DL_HOST = 0, DL_LM = 1, DL_GNSS = 2 };
template <int KIND> struct RowSource { using type = NoRows; };
template <> struct RowSource<DL_LM> { using type = DelayedRows; };
template <> struct RowSource<DL_GNSS> { using type = DelayedGnssRows; };

template <int KIND>
__global__ __launch_bounds__(DL_NT) void k_delayed_front(DelayedFront a, typename RowSource<KIND>::type r)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int bl = blockIdx.x, b = a.b0 + bl, tid = threadIdx.x;
    int m_ = 0, s_ = 3, nc_ = 0;
    unsigned long long um = 0ULL, dm = 0ULL;
    if constexpr (KIND == DL_GNSS) {
        // every wave evaluates the same 64-lane ballot (lane = satellite): m and the ranks are uniform over the workgroup before any barrier
        if (r.cand[bl] && !(a.status[b] & 4)) um = gnss_rows_used(r, bl, tid & (WAVE - 1));
        m_ = __popcll(um); s_ = 1; nc_ = 10;
        if (m_ <= s_) {                                      // not tried, a failed update before it, or m <= 1 (StateManager.cpp:571-575)
            if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; r.slot_out[bl] = -1; r.noise_out[bl] = 0.0; r.var_out[bl] = 1.0; }
            return;
        }
    } else if constexpr (KIND == DL_LM) {
        const int track = r.track[bl];
        if (track >= 0 && !(a.status[b] & 4)) {
            const int cw = r.nt.ih[(size_t)b * r.nt.ir + NOM_N_CLONES];
            dm = r.dropm[bl];
            um = rows_used(r.ts.mask[(size_t)b * r.ts.tmax + track], dm, cw, r.ts.cmax);
            m_ = (r.stereo ? 4 : 2) * __popcll(um);
            nc_ = 6 * cw;
        }
        if (m_ <= s_) {                                      // no candidate, a failed update before it, or m <= s (StateManager.cpp:571-575)
            if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; r.slot_out[bl] = -1; }
            return;
        }
    } else {
        m_ = a.m[bl];
        if (m_ == 0 || (a.status[b] & 4)) {                  // nothing to try (or an update of this call failed on this filter)
            if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; }
            return;
        }
        s_ = a.s[bl]; nc_ = a.nc[bl];
    }
    const int m = m_, s = s_, nc = nc_, mu = m - s;
    const DelayedLds L = delayed_carve(m, s, nc);
    double* base = reinterpret_cast<double*>(smem_raw);
    double *sA = base + L.A, *sHn = base + L.Hn, *sCS = base + L.CS, *sS = base + L.S;
    double *sHf = base + L.sm, *sHi = sHf + DL_SMAX * DL_SMAX, *sS3 = sHi + DL_SMAX * DL_SMAX, *sT3 = sS3 + DL_SMAX * DL_SMAX;
    int* sCol = reinterpret_cast<int*>(base + L.col);
    const int ldA = L.ldA, n = a.cv.n[b], ld = a.cv.ldp, LS = mu + 1;
    double* P = cov_ptr(a.cv, b);
    double* sT = sA + (size_t)(nc + 1) * ldA;               // row c of T = column nc + 1 + c of sA

    // ---- 1. stage the rows --------------------------------------------------------------------------------------------
    if constexpr (KIND == DL_GNSS) {                         // formed here: zero fill (columns 3-5 or 6-8 stay zero, and 9 unless is_adjust_yof), one lane per satellite
        for (int e = tid; e < (nc + 1) * ldA; e += DL_NT) sA[e] = 0.0;
        for (int e = tid; e < m; e += DL_NT) sHn[e] = 1.0;   // H_new: all ones
        const int* I = r.nt.ih + (size_t)b * r.nt.ir;
        if (tid < nc) {                                      // var_old_order: [SE23 (9), YOF (1)]
            const int col = tid < 9 ? I[NOM_IH + 4 * I[NOM_V_POSE] + 1] + tid : I[NOM_IH + 4 * I[NOM_GNSS + NOM_G_YOF] + 1];
            sCol[tid] = col; r.colmap_out[(size_t)bl * a.cs + tid] = col;
        }
        if (tid == 0) r.nc_out[bl] = nc;
        __syncthreads();
        if (tid < WAVE) gnss_rows_form(r, b, bl, um, tid, nc, sA, ldA, sS);      // sS: the rows' m noise terms until S is formed (S holds (mu + 1)^2 = m^2 >= m words and is first written two barriers on)
    } else if constexpr (KIND == DL_LM) {                    // formed here: zero fill, then one lane per store column writes its blocks
        for (int e = tid; e < (nc + 1) * ldA; e += DL_NT) sA[e] = 0.0;
        for (int e = tid; e < s * m; e += DL_NT) sHn[e] = 0.0;
        const int* I = r.nt.ih + (size_t)b * r.nt.ir;
        for (int c = tid; c < nc; c += DL_NT) {              // var_old_order: the window's clones in ascending time
            const int col = I[NOM_IH + 4 * I[NOM_CLONES + c / 6] + 1] + c % 6;
            sCol[c] = col; r.colmap_out[(size_t)bl * a.cs + c] = col;
        }
        if (tid == 0) r.nc_out[bl] = nc;
        __syncthreads();
        if (tid < WAVE) rows_form(r, b, bl, um, dm, tid, m, nc, sA, ldA, sHn);
    } else {
        const double* in = a.dbuf + a.doff[bl];
        const double *Hin = in, *Hnin = in + (size_t)m * nc, *rin = Hnin + (size_t)m * s;
        for (int e = tid; e < m * nc; e += DL_NT) sA[(e % m) + (size_t)(e / m) * ldA] = Hin[e];
        for (int e = tid; e < m; e += DL_NT) sA[e + (size_t)nc * ldA] = rin[e];
        for (int e = tid; e < s * m; e += DL_NT) sHn[e] = Hnin[e];
        for (int c = tid; c < nc; c += DL_NT) sCol[c] = a.colmap[(size_t)bl * a.cs + c];
    }
    __syncthreads();
    double var_ = a.var;
    if constexpr (KIND == DL_GNSS) {                         // noise = amp sqrt(mean(ura std / sin^2 el)), summed in row order by every thread alike
        double avg = 0.0;
        for (int i = 0; i < m; ++i) avg += sS[i];
        const double noise = r.rcv[(size_t)bl * GR_N + (r.g == 0 ? GR_DOPP_AMP : GR_PSR_AMP)] * sqrt(avg / m);
        var_ = noise * noise;
        if (tid == 0) { r.noise_out[bl] = noise; r.var_out[bl] = var_; }
    }
    const double var = var_;
    // ---- 2. the rotation list (one lane) beside T = Pcc H_old^T (the other waves) --------------------------------------
    if (tid < WAVE) {
        if (tid == 0)
            for (int col = 0; col < s; ++col)
                for (int r = m - 1; r > col; --r) {
                    double c, sn;
                    make_givens(sHn[(r - 1) + col * m], sHn[r + col * m], c, sn);
                    sCS[2 * (col * m + r)] = c; sCS[2 * (col * m + r) + 1] = sn;
                    for (int j = col; j < s; ++j) {              // applyOnTheLeft(G.adjoint()): x' = c x - s y, y' = s x + c y
                        const double x = sHn[(r - 1) + j * m], y = sHn[r + j * m];
                        sHn[(r - 1) + j * m] = c * x - sn * y;
                        sHn[r + j * m] = sn * x + c * y;
                    }
                }
    } else {
        const int items = nc * ((m + DL_IB - 1) / DL_IB);
        for (int it = tid - WAVE; it < items; it += DL_NT - WAVE) {
            const int c = it % nc, ib = (it / nc) * DL_IB;      // consecutive lanes: consecutive rows of Pcc (coalesced), one row group
            const double* prow = P + sCol[c];
            double acc[DL_IB];
#pragma unroll
            for (int ii = 0; ii < DL_IB; ++ii) acc[ii] = 0.0;
#pragma unroll 4
            for (int c2 = 0; c2 < nc; ++c2) {
                const double p = prow[(size_t)sCol[c2] * ld];
                // Whole row groups: for ib + ii >= m the read runs past the column into the pad word, the next column, for the last
                // column of H the residual column and, when m < DL_IB, on into the first rows of T that other lanes are writing
                // right now.  Whatever arrives there only enters acc[ii] of a row >= m, which is never stored; no product of a
                // stored row depends on it, and the read stays inside sA (its tail is padded by DL_IB words).
                const double* h = sA + ib + (size_t)c2 * ldA;
#pragma unroll
                for (int ii = 0; ii < DL_IB; ++ii) acc[ii] += p * h[ii];
            }
#pragma unroll
            for (int ii = 0; ii < DL_IB; ++ii) if (ib + ii < m) sT[(ib + ii) + (size_t)c * ldA] = acc[ii];
        }
    }
    __syncthreads();
    // ---- 3. the sweep: every column of [H_old | res | T^T], running carry (k_delayed_qr) --------------------------------
    for (int j = tid; j < 2 * nc + 1; j += DL_NT) {
        double* A = sA + (size_t)j * ldA;
        for (int col = 0; col < s; ++col) {
            double carry = A[m - 1];
            for (int r = m - 1; r > col; --r) {
                const double c = sCS[2 * (col * m + r)], sn = sCS[2 * (col * m + r) + 1];
                const double x = A[r - 1];
                A[r] = sn * x + c * carry;
                carry = c * x - sn * carry;
            }
            A[col] = carry;
        }
    }
    __syncthreads();
    // ---- 4. S of the lower rows (lower triangle), bordered by the residual; elimination as k_gamma -----------------------
    for (int e = tid; e < mu * mu; e += DL_NT) {
        const int i = e % mu, i2 = e / mu;
        if (i < i2) continue;
        double acc = 0.0;
        for (int c = 0; c < nc; ++c) acc += sA[(s + i) + (size_t)c * ldA] * sT[(s + i2) + (size_t)c * ldA];
        if (i == i2) acc += var;
        sS[i * LS + i2] = acc;
    }
    for (int e = tid; e <= mu; e += DL_NT) sS[mu * LS + e] = (e < mu) ? sA[(s + e) + (size_t)nc * ldA] : 0.0;
    __syncthreads();
    for (int j = 0; j < mu; ++j) {
        const double inv = 1.0 / sS[j * LS + j];
        const int w = mu - j;
        for (int e = tid; e < w * w; e += DL_NT) {
            const int i = j + 1 + e % w, k = j + 1 + e / w;
            if (k > i) continue;
            sS[i * LS + k] -= sS[i * LS + j] * sS[k * LS + j] * inv;
        }
        __syncthreads();
    }
    // ---- 5. the verdict (uniform: every thread reads the same LDS word) -------------------------------------------------
    const double chi2 = -sS[mu * LS + mu];
    bool refuse;
    if constexpr (KIND != DL_HOST) refuse = !(chi2 <= r.chi2_mult * r.chi2[m]);      // the quantile at dof m (StateManager.cpp:610-612); a non-finite chi2 is refused
    else refuse = chi2 > a.thr[bl];
    if (refuse && a.do_chi2) {
        if (tid == 0) {
            a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = chi2; a.mu[bl] = 0;
            if constexpr (KIND != DL_HOST) r.slot_out[bl] = -1;
        }
        return;
    }
    // the trailing update's rows, from row 0
    double* Hu = a.Hu + (size_t)bl * a.hsu;
    for (int e = tid; e < mu * nc; e += DL_NT) { const int i = e % mu, c = e / mu; Hu[i + (size_t)c * a.mldu] = sA[(s + i) + (size_t)c * ldA]; }
    for (int e = tid; e < mu; e += DL_NT) a.resu[(size_t)bl * a.mldu + e] = sA[(s + e) + (size_t)nc * ldA];
    // addVariableDelayedInvertible with the upper s rows: PH^T (:490-505) -> Y
    double* Y = a.Y + (size_t)bl * a.ystride;
    for (int r = tid; r < n; r += DL_NT) {
        double acc[DL_SMAX];
#pragma unroll
        for (int j = 0; j < DL_SMAX; ++j) acc[j] = 0.0;
#pragma unroll 4
        for (int c = 0; c < nc; ++c) {
            const double p = P[r + (size_t)sCol[c] * ld];
#pragma unroll
            for (int j = 0; j < DL_SMAX; ++j) if (j < s) acc[j] += p * sA[j + (size_t)c * ldA];
        }
#pragma unroll
        for (int j = 0; j < DL_SMAX; ++j) if (j < s) Y[r + (size_t)j * ld] = acc[j];
    }
    // S = Hx Pcc Hx^T + var I (:507-514) from the rotated T, H_new^-1 (:516)
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double acc = 0.0;
        for (int c = 0; c < nc; ++c) acc += sA[i + (size_t)c * ldA] * sT[j + (size_t)c * ldA];
        sS3[i + j * s] = acc + (i == j ? var : 0.0);
        sHf[i + j * s] = sHn[i + j * m];
    }
    __syncthreads();                                         // also: this thread's rows of Y are visible to the workgroup
    if (tid == 0) inv_small(sHf, sHi, s);
    __syncthreads();
    // T = Hi S ; corner = T Hi^T (:518), symmetrised as :534 does for the whole matrix
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double acc = 0.0;
        for (int l = 0; l < s; ++l) acc += sHi[i + l * s] * sS3[l + j * s];
        sT3[i + j * s] = acc;
    }
    __syncthreads();
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double x = 0.0, y = 0.0;
        for (int l = 0; l < s; ++l) { x += sT3[i + l * s] * sHi[j + l * s]; y += sT3[j + l * s] * sHi[i + l * s]; }
        P[(n + i) + (size_t)(n + j) * ld] = 0.5 * (x + y);
    }
    // cross = -PH^T Hi^T (:526-528)
    for (int r = tid; r < n; r += DL_NT) {
        double y[DL_SMAX];
#pragma unroll
        for (int l = 0; l < DL_SMAX; ++l) y[l] = l < s ? Y[r + (size_t)l * ld] : 0.0;
        for (int j = 0; j < s; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < DL_SMAX; ++l) if (l < s) acc += y[l] * sHi[j + l * s];
            P[r + (size_t)(n + j) * ld] = -acc;
            P[(n + j) + (size_t)r * ld] = -acc;
        }
    }
    if (tid == 0) { a.cv.n[b] = n + s; a.added[bl] = 1; a.new_idx[bl] = n; a.chi2[bl] = chi2; a.mu[bl] = mu; }
    if constexpr (KIND == DL_GNSS) {
        // the scalar's table record in the slot the host reserved, registered as GNSS scalar r.g: k_imu_steps advances it and later
        // epochs read it; the round's boxPlus retracts it with the rest
        if (tid == 0) {
            int* I = r.nt.ih + (size_t)b * r.nt.ir;
            const int slot = r.slot[bl];
            int* v = I + NOM_IH + 4 * slot;
            v[0] = NOM_KIND_SCALAR; v[1] = n; v[2] = -1; v[3] = 0;
            double* x = r.nt.dv + (size_t)b * r.nt.dr + NOM_DH + (size_t)slot * NOM_VD;
            for (int i = 0; i < NOM_VD; ++i) x[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
            x[9] = r.value[bl];
            I[NOM_GNSS + (r.g == 0 ? NOM_G_FS : r.g - 1)] = slot;
            if (slot >= I[NOM_N_VAR]) I[NOM_N_VAR] = slot + 1;
            r.slot_out[bl] = slot;
        }
    } else if constexpr (KIND == DL_LM) {
        // the landmark's table record, in the slot the host reserved: the round's boxPlus (k_nominal_update<false>, behind the
        // trailing update) retracts it with the rest (AnchoredLandmark.cpp:227-243)
        if (tid == 0) {
            int* I = r.nt.ih + (size_t)b * r.nt.ir;
            const int slot = r.slot[bl];
            int* v = I + NOM_IH + 4 * slot;
            v[0] = NOM_KIND_LM; v[1] = n; v[2] = I[NOM_CLONES + r.anchor[bl]]; v[3] = 0;
            double* x = r.nt.dv + (size_t)b * r.nt.dr + NOM_DH + (size_t)slot * NOM_VD;
            for (int i = 0; i < NOM_VD; ++i) x[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
            for (int i = 0; i < 3; ++i) x[9 + i] = r.pf[3 * (size_t)bl + i];
            if (slot >= I[NOM_N_VAR]) I[NOM_N_VAR] = slot + 1;
            r.slot_out[bl] = slot;
        }
    }
}

// test hook (ingvio_debug_landmark_init_rows): the row stage of k_delayed_front<true> alone, one wave, dense rows to global memory
__global__ __launch_bounds__(WAVE) void k_delayed_rows_debug(DelayedRows r, int b, double* __restrict__ out, int* __restrict__ m_out)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int cw = r.nt.ih[(size_t)b * r.nt.ir + NOM_N_CLONES], nc = 6 * cw, s = 3;
    const unsigned long long dm = r.dropm[0];
    const unsigned long long um = rows_used(r.ts.mask[(size_t)b * r.ts.tmax + r.track[0]], dm, cw, r.ts.cmax);
    const int m = (r.stereo ? 4 : 2) * __popcll(um);
    if (tid == 0) *m_out = m;
    if (m == 0) return;
    const DelayedLds L = delayed_carve(m, s, nc);
    double* base = reinterpret_cast<double*>(smem_raw);
    double *sA = base + L.A, *sHn = base + L.Hn;
    for (int e = tid; e < (nc + 1) * L.ldA; e += WAVE) sA[e] = 0.0;
    for (int e = tid; e < s * m; e += WAVE) sHn[e] = 0.0;
    __syncthreads();
    rows_form(r, b, 0, um, dm, tid, m, nc, sA, L.ldA, sHn);
    __syncthreads();
    for (int e = tid; e < m * nc; e += WAVE) out[e] = sA[(e % m) + (size_t)(e / m) * L.ldA];
    for (int e = tid; e < s * m; e += WAVE) out[(size_t)m * nc + e] = sHn[e];
    for (int e = tid; e < m; e += WAVE) out[(size_t)m * (nc + s) + e] = sA[e + (size_t)nc * L.ldA];
}

// test hook (ingvio_debug_gnss_init_rows): the row stage of k_delayed_front<DL_GNSS> alone, one wave, dense rows to global memory
__global__ __launch_bounds__(WAVE) void k_delayed_gnss_rows_debug(DelayedGnssRows r, int b, double* __restrict__ out, int* __restrict__ m_out)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, nc = 10;
    const unsigned long long um = gnss_rows_used(r, 0, tid);
    const int m = __popcll(um);
    if (tid == 0) *m_out = m;
    if (m == 0) return;
    const DelayedLds L = delayed_carve(m, 1, nc);
    double* base = reinterpret_cast<double*>(smem_raw);
    double *sA = base + L.A, *sW = base + L.Hn;
    for (int e = tid; e < (nc + 1) * L.ldA; e += WAVE) sA[e] = 0.0;
    __syncthreads();
    gnss_rows_form(r, b, 0, um, tid, nc, sA, L.ldA, sW);
    __syncthreads();
    for (int e = tid; e < m * (nc + 1); e += WAVE) out[e] = sA[(e % m) + (size_t)(e / m) * L.ldA];
    if (tid == 0) {
        double avg = 0.0;
        for (int i = 0; i < m; ++i) avg += sW[i];
        out[(size_t)m * (nc + 1)] = r.rcv[r.g == 0 ? GR_DOPP_AMP : GR_PSR_AMP] * sqrt(avg / m);
    }
}

// R_w2ecef = R_enu2ecef Rz(YOF), row-major, as k_gnss_front forms it (GnssUpdate.cpp:332): one thread per filter
__global__ __launch_bounds__(64) void k_delayed_gnss_rw(NomTable nt, const double* __restrict__ rcv, int b0, int nb, double* __restrict__ Rw)
{
    const int bl = blockIdx.x * 64 + threadIdx.x;
    if (bl >= nb) return;
    const int* I = nt.ih + (size_t)(b0 + bl) * nt.ir;
    const int sy_ = I[NOM_GNSS + NOM_G_YOF];
    const double yaw = sy_ >= 0 ? nt.dv[(size_t)(b0 + bl) * nt.dr + NOM_DH + (size_t)sy_ * NOM_VD + 9] : 0.0;
    const double cy = cos(yaw), sy = sin(yaw);
    const double* rc = rcv + (size_t)bl * GR_N;
    for (int r = 0; r < 3; ++r) {
        Rw[9 * bl + 3 * r] = rc[GR_RENU + 3 * r] * cy + rc[GR_RENU + 3 * r + 1] * sy;
        Rw[9 * bl + 3 * r + 1] = -rc[GR_RENU + 3 * r] * sy + rc[GR_RENU + 3 * r + 1] * cy;
        Rw[9 * bl + 3 * r + 2] = rc[GR_RENU + 3 * r + 2];
    }
}


// ---- the large form (ingvio_set_delayed_form): [H_old | res | T^T] in a per-filter HBM workspace, through LDS in column panels ----
// Same inputs, outputs and side effects as k_delayed_front.  What differs is where the (2 nc + 1) columns of m doubles live: in
// ws (column stride ldw) instead of LDS.  T is formed straight into the workspace beside the serial derivation of the rotations;
// the sweep takes DLL_W columns at a time through LDS (a column needs only itself and the rotation list); S is accumulated as a
// packed lower triangle in LDS from DLL_K-column chunks of the rotated lower rows, in ascending column order as the LDS form sums it.
#define DLL_W 64
#define DLL_K 8

struct DelayedLargeLds { size_t Hn, CS, sm, R, Sc, col, q, bytes; int ldA; };      // offsets in doubles (every one even)

__host__ __device__ inline DelayedLargeLds delayed_large_carve(int m, int s, int nc)
{
    auto even = [](size_t x) { return (x + 1) & ~(size_t)1; };
    DelayedLargeLds L;
    const size_t mu = m - s;
    L.ldA = m | 1;
    L.Hn = 0;                                                // [s][m]
    L.CS = even((size_t)s * m);                              // [s][m][2]
    L.sm = even(L.CS + 2 * (size_t)s * m);                   // 4 x [6][6]
    L.R = even(L.sm + 4 * DL_SMAX * DL_SMAX);                // one region, three tenants in turn:
    const size_t tri = even((mu + 1) * (mu + 2) / 2);        //   the sweep's panel [DLL_W][ldA];
    L.Sc = L.R + tri;                                        //   S packed [(mu + 1)(mu + 2) / 2] + the chunk [2][DLL_K][mu];
    size_t r = (size_t)DLL_W * L.ldA;                        //   the upper s rows of H and T [2][nc][DL_SMAX]
    if (tri + 2 * DLL_K * mu > r) r = tri + 2 * DLL_K * mu;
    if (2 * (size_t)nc * DL_SMAX > r) r = 2 * (size_t)nc * DL_SMAX;
    L.col = even(L.R + r);                                   // nc ints
    L.q = L.col + ((((size_t)nc + 3) & ~(size_t)3) >> 1);    // 64 ints: window position of the observer of every row group
    L.bytes = 8 * L.q + 4 * 64;
    return L;
}

template <bool ROWS>
__global__ __launch_bounds__(DL_NT) void k_delayed_front_large(DelayedFront a, std::conditional_t<ROWS, DelayedRows, NoRows> r, DelayedLarge g)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int bl = blockIdx.x, b = a.b0 + bl, tid = threadIdx.x;
    if (g.sel && !g.sel[bl]) return;                         // a filter of the other form (or none): that launch writes its outputs
    int m_ = 0, s_ = 3, nc_ = 0;
    unsigned long long um = 0ULL, dm = 0ULL;
    if constexpr (ROWS) {
        const int track = r.track[bl];
        if (track >= 0 && !(a.status[b] & 4)) {
            const int cw = r.nt.ih[(size_t)b * r.nt.ir + NOM_N_CLONES];
            dm = r.dropm[bl];
            um = rows_used(r.ts.mask[(size_t)b * r.ts.tmax + track], dm, cw, r.ts.cmax);
            m_ = (r.stereo ? 4 : 2) * __popcll(um);
            nc_ = 6 * cw;
        }
        if (m_ <= s_) {
            if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; r.slot_out[bl] = -1; }
            return;
        }
    } else {
        m_ = a.m[bl];
        if (m_ == 0 || (a.status[b] & 4)) {
            if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; }
            return;
        }
        s_ = a.s[bl]; nc_ = a.nc[bl];
    }
    const int m = m_, s = s_, nc = nc_, mu = m - s;
    const DelayedLargeLds L = delayed_large_carve(m, s, nc);
    double* base = reinterpret_cast<double*>(smem_raw);
    double *sHn = base + L.Hn, *sCS = base + L.CS, *sR = base + L.R, *sS = sR, *sC = base + L.Sc;
    double *sHf = base + L.sm, *sHi = sHf + DL_SMAX * DL_SMAX, *sS3 = sHi + DL_SMAX * DL_SMAX, *sT3 = sS3 + DL_SMAX * DL_SMAX;
    int *sCol = reinterpret_cast<int*>(base + L.col), *sQ = reinterpret_cast<int*>(base + L.q);
    const int ldA = L.ldA, n = a.cv.n[b], ld = a.cv.ldp, ldw = g.ldw;
    double* P = cov_ptr(a.cv, b);
    double* W = g.ws + (size_t)bl * g.ws_stride;             // [2 nc + 1][ldw]: H_old columns, res, the rows of T
    double* WT = W + (size_t)(nc + 1) * ldw;
    // where the unrotated H_old and res are read: the workspace (formed rows) or the call's packed rows (host-fed)
    const double *Hsrc = W, *rsrc = W + (size_t)nc * ldw;
    int ldh = ldw;

    // ---- 1. stage H_new, the column map; formed rows go to the workspace -------------------------------------------------
    if constexpr (ROWS) {
        for (size_t e = tid; e < (size_t)(nc + 1) * ldw; e += DL_NT) W[e] = 0.0;
        for (int e = tid; e < s * m; e += DL_NT) sHn[e] = 0.0;
        const int* I = r.nt.ih + (size_t)b * r.nt.ir;
        for (int c = tid; c < nc; c += DL_NT) {
            const int col = I[NOM_IH + 4 * I[NOM_CLONES + c / 6] + 1] + c % 6;
            sCol[c] = col; r.colmap_out[(size_t)bl * a.cs + c] = col;
        }
        if (tid < WAVE && ((um >> tid) & 1ULL)) {            // row group -> window position of its observer
            const unsigned long long below = (1ULL << tid) - 1ULL;
            sQ[__popcll(um & below)] = tid - __popcll(dm & below);
        }
        if (tid == 0) r.nc_out[bl] = nc;
        __syncthreads();
        if (tid < WAVE) rows_form(r, b, bl, um, dm, tid, m, nc, W, ldw, sHn);
    } else {
        const double* in = a.dbuf + a.doff[bl];
        Hsrc = in; ldh = m; rsrc = in + (size_t)m * (nc + s);
        const double* Hnin = in + (size_t)m * nc;
        for (int e = tid; e < s * m; e += DL_NT) sHn[e] = Hnin[e];
        for (int c = tid; c < nc; c += DL_NT) sCol[c] = a.colmap[(size_t)bl * a.cs + c];
    }
    __syncthreads();
    // ---- 2. the rotation list (one lane) beside T = Pcc H_old^T (the other waves), T into the workspace ------------------
    if (tid < WAVE) {
        if (tid == 0)
            for (int col = 0; col < s; ++col)
                for (int rr = m - 1; rr > col; --rr) {
                    double c, sn;
                    make_givens(sHn[(rr - 1) + col * m], sHn[rr + col * m], c, sn);
                    sCS[2 * (col * m + rr)] = c; sCS[2 * (col * m + rr) + 1] = sn;
                    for (int j = col; j < s; ++j) {
                        const double x = sHn[(rr - 1) + j * m], y = sHn[rr + j * m];
                        sHn[(rr - 1) + j * m] = c * x - sn * y;
                        sHn[rr + j * m] = sn * x + c * y;
                    }
                }
    } else if constexpr (ROWS) {
        // a formed row has nine non-zero entries: the anchor's theta block and the observer's six columns.  Taken in ascending
        // column order, the sum is the dense one with its zero terms left out.
        const int per = r.stereo ? 4 : 2, anc = r.anchor[bl];
        const int items = nc * m;
        for (int it = tid - WAVE; it < items; it += DL_NT - WAVE) {
            const int c = it % nc, i = it / nc, q = sQ[i / per];
            const double* prow = P + sCol[c];
            const double* h = W + i;
            double acc = 0.0;
            if (anc < q)
                for (int k = 0; k < 3; ++k) acc += prow[(size_t)sCol[6 * anc + k] * ld] * h[(size_t)(6 * anc + k) * ldw];
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += prow[(size_t)sCol[6 * q + k] * ld] * h[(size_t)(6 * q + k) * ldw];
            if (anc > q)
                for (int k = 0; k < 3; ++k) acc += prow[(size_t)sCol[6 * anc + k] * ld] * h[(size_t)(6 * anc + k) * ldw];
            WT[i + (size_t)c * ldw] = acc;
        }
    } else {
        const int items = nc * ((m + DL_IB - 1) / DL_IB);
        for (int it = tid - WAVE; it < items; it += DL_NT - WAVE) {
            const int c = it % nc, ib = (it / nc) * DL_IB;
            const int nr = m - ib < DL_IB ? m - ib : DL_IB;
            const double* prow = P + sCol[c];
            double acc[DL_IB];
#pragma unroll
            for (int ii = 0; ii < DL_IB; ++ii) acc[ii] = 0.0;
#pragma unroll 4
            for (int c2 = 0; c2 < nc; ++c2) {
                const double p = prow[(size_t)sCol[c2] * ld];
                const double* h = Hsrc + ib + (size_t)c2 * ldh;
#pragma unroll
                for (int ii = 0; ii < DL_IB; ++ii) acc[ii] += p * (ii < nr ? h[ii] : 0.0);      // no read past the column
            }
#pragma unroll
            for (int ii = 0; ii < DL_IB; ++ii) if (ii < nr) WT[(ib + ii) + (size_t)c * ldw] = acc[ii];
        }
    }
    __syncthreads();
    // ---- 3. the sweep, DLL_W columns at a time through LDS: every column by its own lane, running carry -------------------
    const int ncols = 2 * nc + 1;
    for (int p0 = 0; p0 < ncols; p0 += DLL_W) {
        const int pw = ncols - p0 < DLL_W ? ncols - p0 : DLL_W;
        for (int e = tid; e < pw * m; e += DL_NT) {
            const int jj = e / m, rr = e - jj * m, j = p0 + jj;
            const double* src = j < nc ? Hsrc + (size_t)j * ldh : (j == nc ? rsrc : W + (size_t)j * ldw);
            sR[rr + (size_t)jj * ldA] = src[rr];
        }
        __syncthreads();
        if (tid < pw) {
            double* A = sR + (size_t)tid * ldA;
            for (int col = 0; col < s; ++col) {
                double carry = A[m - 1];
                for (int rr = m - 1; rr > col; --rr) {
                    const double c = sCS[2 * (col * m + rr)], sn = sCS[2 * (col * m + rr) + 1];
                    const double x = A[rr - 1];
                    A[rr] = sn * x + c * carry;
                    carry = c * x - sn * carry;
                }
                A[col] = carry;
            }
        }
        __syncthreads();
        for (int e = tid; e < pw * m; e += DL_NT) {
            const int jj = e / m, rr = e - jj * m;
            W[rr + (size_t)(p0 + jj) * ldw] = sR[rr + (size_t)jj * ldA];
        }
        __syncthreads();
    }
    // ---- 4. S of the lower rows, packed lower triangle S(i, k) = sS[i (i + 1) / 2 + k], from chunks of DLL_K columns ------
    double *sHc = sC, *sTc = sC + (size_t)DLL_K * mu;
    for (int c0 = 0; c0 < nc; c0 += DLL_K) {
        const int kc = nc - c0 < DLL_K ? nc - c0 : DLL_K;
        for (int e = tid; e < kc * mu; e += DL_NT) {
            const int k = e / mu, i = e - k * mu;
            sHc[e] = W[(s + i) + (size_t)(c0 + k) * ldw];
            sTc[e] = WT[(s + i) + (size_t)(c0 + k) * ldw];
        }
        __syncthreads();
        for (int e = tid; e < mu * mu; e += DL_NT) {
            const int i = e % mu, i2 = e / mu;
            if (i < i2) continue;
            const int idx = i * (i + 1) / 2 + i2;
            double acc = c0 ? sS[idx] : 0.0;
            for (int k = 0; k < kc; ++k) acc += sHc[i + k * mu] * sTc[i2 + k * mu];
            if (i == i2 && c0 + kc == nc) acc += a.var;
            sS[idx] = acc;
        }
        __syncthreads();
    }
    const int bord = mu * (mu + 1) / 2;
    for (int e = tid; e <= mu; e += DL_NT) sS[bord + e] = (e < mu) ? W[(s + e) + (size_t)nc * ldw] : 0.0;
    __syncthreads();
    for (int j = 0; j < mu; ++j) {
        const int jj = j * (j + 1) / 2 + j;
        const double inv = 1.0 / sS[jj];
        const int w = mu - j;
        for (int e = tid; e < w * w; e += DL_NT) {
            const int i = j + 1 + e % w, k = j + 1 + e / w;
            if (k > i) continue;
            const int ri = i * (i + 1) / 2, rk = k * (k + 1) / 2;
            sS[ri + k] -= sS[ri + j] * sS[rk + j] * inv;
        }
        __syncthreads();
    }
    // ---- 5. the verdict ------------------------------------------------------------------------------------------------
    const double chi2 = -sS[bord + mu];
    bool refuse;
    if constexpr (ROWS) refuse = !(chi2 <= r.chi2_mult * r.chi2[m]);
    else refuse = chi2 > a.thr[bl];
    if (refuse && a.do_chi2) {
        if (tid == 0) {
            a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = chi2; a.mu[bl] = 0;
            if constexpr (ROWS) r.slot_out[bl] = -1;
        }
        return;
    }
    __syncthreads();                                         // every thread has read chi2: the region changes tenant
    // the upper s rows of the rotated H and T into LDS; the trailing update's rows, from row 0
    double *sHup = sR, *sTup = sR + (size_t)nc * DL_SMAX;
    for (int e = tid; e < s * nc; e += DL_NT) {
        const int j = e % s, c = e / s;
        sHup[j + c * DL_SMAX] = W[j + (size_t)c * ldw];
        sTup[j + c * DL_SMAX] = WT[j + (size_t)c * ldw];
    }
    double* Hu = a.Hu + (size_t)bl * a.hsu;
    for (int e = tid; e < mu * nc; e += DL_NT) { const int i = e % mu, c = e / mu; Hu[i + (size_t)c * a.mldu] = W[(s + i) + (size_t)c * ldw]; }
    for (int e = tid; e < mu; e += DL_NT) a.resu[(size_t)bl * a.mldu + e] = W[(s + e) + (size_t)nc * ldw];
    __syncthreads();
    // addVariableDelayedInvertible with the upper s rows, as k_delayed_front
    double* Y = a.Y + (size_t)bl * a.ystride;
    for (int rr = tid; rr < n; rr += DL_NT) {
        double acc[DL_SMAX];
#pragma unroll
        for (int j = 0; j < DL_SMAX; ++j) acc[j] = 0.0;
#pragma unroll 4
        for (int c = 0; c < nc; ++c) {
            const double p = P[rr + (size_t)sCol[c] * ld];
#pragma unroll
            for (int j = 0; j < DL_SMAX; ++j) if (j < s) acc[j] += p * sHup[j + c * DL_SMAX];
        }
#pragma unroll
        for (int j = 0; j < DL_SMAX; ++j) if (j < s) Y[rr + (size_t)j * ld] = acc[j];
    }
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double acc = 0.0;
        for (int c = 0; c < nc; ++c) acc += sHup[i + c * DL_SMAX] * sTup[j + c * DL_SMAX];
        sS3[i + j * s] = acc + (i == j ? a.var : 0.0);
        sHf[i + j * s] = sHn[i + j * m];
    }
    __syncthreads();
    if (tid == 0) inv_small(sHf, sHi, s);
    __syncthreads();
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double acc = 0.0;
        for (int l = 0; l < s; ++l) acc += sHi[i + l * s] * sS3[l + j * s];
        sT3[i + j * s] = acc;
    }
    __syncthreads();
    if (tid < s * s) {
        const int i = tid % s, j = tid / s;
        double x = 0.0, y = 0.0;
        for (int l = 0; l < s; ++l) { x += sT3[i + l * s] * sHi[j + l * s]; y += sT3[j + l * s] * sHi[i + l * s]; }
        P[(n + i) + (size_t)(n + j) * ld] = 0.5 * (x + y);
    }
    for (int rr = tid; rr < n; rr += DL_NT) {
        double y[DL_SMAX];
#pragma unroll
        for (int l = 0; l < DL_SMAX; ++l) y[l] = l < s ? Y[rr + (size_t)l * ld] : 0.0;
        for (int j = 0; j < s; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < DL_SMAX; ++l) if (l < s) acc += y[l] * sHi[j + l * s];
            P[rr + (size_t)(n + j) * ld] = -acc;
            P[(n + j) + (size_t)rr * ld] = -acc;
        }
    }
    if (tid == 0) { a.cv.n[b] = n + s; a.added[bl] = 1; a.new_idx[bl] = n; a.chi2[bl] = chi2; a.mu[bl] = mu; }
    if constexpr (ROWS) {
        if (tid == 0) {                                      // the landmark's table record, as k_delayed_front<true> enters it
            int* I = r.nt.ih + (size_t)b * r.nt.ir;
            const int slot = r.slot[bl];
            int* v = I + NOM_IH + 4 * slot;
            v[0] = NOM_KIND_LM; v[1] = n; v[2] = I[NOM_CLONES + r.anchor[bl]]; v[3] = 0;
            double* x = r.nt.dv + (size_t)b * r.nt.dr + NOM_DH + (size_t)slot * NOM_VD;
            for (int i = 0; i < NOM_VD; ++i) x[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
            for (int i = 0; i < 3; ++i) x[9 + i] = r.pf[3 * (size_t)bl + i];
            if (slot >= I[NOM_N_VAR]) I[NOM_N_VAR] = slot + 1;
            r.slot_out[bl] = slot;
        }
    }
}

// test hook: the row stage alone for a window whose rows do not fit LDS, formed straight into global memory
__global__ __launch_bounds__(WAVE) void k_delayed_rows_debug_large(DelayedRows r, int b, double* __restrict__ out, int* __restrict__ m_out)
{
    const int tid = threadIdx.x;
    const int cw = r.nt.ih[(size_t)b * r.nt.ir + NOM_N_CLONES], nc = 6 * cw, s = 3;
    const unsigned long long dm = r.dropm[0];
    const unsigned long long um = rows_used(r.ts.mask[(size_t)b * r.ts.tmax + r.track[0]], dm, cw, r.ts.cmax);
    const int m = (r.stereo ? 4 : 2) * __popcll(um);
    if (tid == 0) *m_out = m;
    if (m == 0) return;
    for (size_t e = tid; e < (size_t)m * (nc + s + 1); e += WAVE) out[e] = 0.0;
    __syncthreads();
    rows_form(r, b, 0, um, dm, tid, m, nc, out, m, out + (size_t)m * (nc + 1));      // [H_old | res | H_new], column stride m
}

}  // namespace

size_t delayed_front_lds(int m, int s, int nc) { return delayed_carve(m, s, nc).bytes; }

int launch_delayed_front(const DelayedFront& L, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front<DL_HOST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front<DL_HOST>, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L, NoRows{});
    return 0;
}

int launch_delayed_front_rows(const DelayedFront& L, const DelayedRows& R, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front<DL_LM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front<DL_LM>, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L, R);
    return 0;
}

int launch_delayed_rows_debug(const DelayedRows& R, int b, double* out, int* m_out, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024) return -1;
    hipFuncSetAttribute((const void*)k_delayed_rows_debug, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_rows_debug, dim3(1), dim3(WAVE), lds_bytes, st, R, b, out, m_out);
    return 0;
}

size_t delayed_front_large_lds(int m, int s, int nc) { return delayed_large_carve(m, s, nc).bytes; }

int launch_delayed_front_large(const DelayedFront& L, const DelayedLarge& G, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024 || !G.ws) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front_large<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front_large<false>, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L, NoRows{}, G);
    return 0;
}

int launch_delayed_front_rows_large(const DelayedFront& L, const DelayedRows& R, const DelayedLarge& G, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024 || !G.ws) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front_large<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front_large<true>, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L, R, G);
    return 0;
}

int launch_delayed_rows_debug_large(const DelayedRows& R, int b, double* out, int* m_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_delayed_rows_debug_large, dim3(1), dim3(WAVE), 0, st, R, b, out, m_out);
    return 0;
}

void launch_delayed_gnss_rw(const NomTable& nt, const double* rcv, int b0, int nb, double* Rw, hipStream_t st)
{
    hipLaunchKernelGGL(k_delayed_gnss_rw, dim3((nb + 63) / 64), dim3(64), 0, st, nt, rcv, b0, nb, Rw);
}

int launch_delayed_front_gnss(const DelayedFront& L, const DelayedGnssRows& R, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024 || R.smax > 64) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front<DL_GNSS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front<DL_GNSS>, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L, R);
    return 0;
}

int launch_delayed_gnss_rows_debug(const DelayedGnssRows& R, int b, double* out, int* m_out, hipStream_t st)
{
    if (R.smax > 64) return -1;
    const size_t lds_bytes = delayed_carve(64, 1, 10).bytes;
    hipFuncSetAttribute((const void*)k_delayed_gnss_rows_debug, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_gnss_rows_debug, dim3(1), dim3(WAVE), lds_bytes, st, R, b, out, m_out);
    return 0;
}
