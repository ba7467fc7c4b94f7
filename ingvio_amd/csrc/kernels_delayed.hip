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
// No atomics, no global round trip inside the rotation loop.  FP64, gfx950 only.
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

__global__ __launch_bounds__(DL_NT) void k_delayed_front(DelayedFront a)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int bl = blockIdx.x, b = a.b0 + bl, tid = threadIdx.x;
    const int m = a.m[bl];
    if (m == 0 || (a.status[b] & 4)) {                       // nothing to try (or an update of this call failed on this filter)
        if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = 0.0; a.mu[bl] = 0; }
        return;
    }
    const int s = a.s[bl], nc = a.nc[bl], mu = m - s;
    const DelayedLds L = delayed_carve(m, s, nc);
    double* base = reinterpret_cast<double*>(smem_raw);
    double *sA = base + L.A, *sHn = base + L.Hn, *sCS = base + L.CS, *sS = base + L.S;
    double *sHf = base + L.sm, *sHi = sHf + DL_SMAX * DL_SMAX, *sS3 = sHi + DL_SMAX * DL_SMAX, *sT3 = sS3 + DL_SMAX * DL_SMAX;
    int* sCol = reinterpret_cast<int*>(base + L.col);
    const int ldA = L.ldA, n = a.cv.n[b], ld = a.cv.ldp, LS = mu + 1;
    double* P = cov_ptr(a.cv, b);
    const double* in = a.dbuf + a.doff[bl];
    const double *Hin = in, *Hnin = in + (size_t)m * nc, *rin = Hnin + (size_t)m * s;
    double* sT = sA + (size_t)(nc + 1) * ldA;               // row c of T = column nc + 1 + c of sA

    // ---- 1. stage the rows --------------------------------------------------------------------------------------------
    for (int e = tid; e < m * nc; e += DL_NT) sA[(e % m) + (size_t)(e / m) * ldA] = Hin[e];
    for (int e = tid; e < m; e += DL_NT) sA[e + (size_t)nc * ldA] = rin[e];
    for (int e = tid; e < s * m; e += DL_NT) sHn[e] = Hnin[e];
    for (int c = tid; c < nc; c += DL_NT) sCol[c] = a.colmap[(size_t)bl * a.cs + c];
    __syncthreads();
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
        if (i == i2) acc += a.var;
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
    if (chi2 > a.thr[bl] && a.do_chi2) {
        if (tid == 0) { a.added[bl] = 0; a.new_idx[bl] = -1; a.chi2[bl] = chi2; a.mu[bl] = 0; }
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
        sS3[i + j * s] = acc + (i == j ? a.var : 0.0);
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
}

}  // namespace

size_t delayed_front_lds(int m, int s, int nc) { return delayed_carve(m, s, nc).bytes; }

int launch_delayed_front(const DelayedFront& L, size_t lds_bytes, hipStream_t st)
{
    if (lds_bytes > 160 * 1024) return -1;
    hipFuncSetAttribute((const void*)k_delayed_front, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(k_delayed_front, dim3(L.nb), dim3(DL_NT), lds_bytes, st, L);
    return 0;
}
