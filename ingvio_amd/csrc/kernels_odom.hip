// kernels_odom.hip — the output side of the device-resident loop: the odometry record of ingvio_odom_begin / _end and the
// batched marginal getter ingvio_cov_get_marginal_batch.  Both only READ the nominal table and the live half of P.
//
// k_odom_out: one workgroup of one wave per filter.  The wave resolves the record's variables through the table's slots, gathers the
// 15 x 15 block of P over (extended pose, bg, ba) through their idx into LDS, forms the two Euclidean congruences from there, scans the
// diagonal of P and copies the finished record from LDS to global memory in one coalesced sweep.  The whole record is staged in LDS, so
// every field that was not requested (or whose variable is absent) leaves as the zero it was initialised to.
// k_cov_marginal: the same gather with a per-filter list of columns, straight to global memory.
// gfx950 only.
#include <hip/hip_runtime.h>

#include "launch_odom.h"

namespace {

// dst[c * ns + r] = P(row cols[r], column cols[c]) for the ns x ns block, column-major; a negative column gives zeros (an absent variable)
template <class Dst>
__device__ __forceinline__ void gather_block(const double* __restrict__ P, int ldp, const int* cols, int ns, int tid, int nthreads, Dst dst)
{
    for (int e = tid; e < ns * ns; e += nthreads) {
        const int c = e / ns, r = e - c * ns;
        const int gc = cols[c], gr = cols[r];
        dst[e] = (gc >= 0 && gr >= 0) ? P[(size_t)gc * ldp + gr] : 0.0;
    }
}

__device__ __forceinline__ double wave_min(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off, WAVE));
    return x;
}
__device__ __forceinline__ double wave_max(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, WAVE));
    return x;
}

// -[a]x, entry (i, k)
__device__ __forceinline__ double neg_skew(const double* a, int i, int k)
{
    if (i == k) return 0.0;
    const int m = 3 - i - k;                                             // the third axis
    return ((k - i + 3) % 3 == 1) ? a[m] : -a[m];                        // [a]x(i, i + 1) = -a_m, so -[a]x(i, i + 1) = +a_m
}

}  // namespace

// grid = nb filters, block = one wave
__global__ __launch_bounds__(64) void k_odom_out(NomTable t, CovView cv, double* __restrict__ rec, int b0, int what)
{
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    __shared__ double s_rec[ODOM_BODY];                                  // the record behind its header
    __shared__ double s_J[9 * 9];                                        // rows 0-5: J_p (position, orientation), rows 6-8: J_v
    __shared__ int s_idx[4];                                             // idx of pose, bg, ba, extrinsics; -1: absent
    __shared__ int s_col[15];
    const int* I = t.ih + (size_t)b * t.ir;
    const int* var = I + NOM_IH;
    const double* D = t.dv + (size_t)b * t.dr + NOM_DH;
    const int n = cv.n[b], ldp = cv.ldp;
    const double* P = cov_ptr(cv, b);
    const int nv = min(I[NOM_N_VAR], t.vmax);
    for (int e = lane; e < ODOM_BODY; e += 64) s_rec[e] = 0.0;

    // ---- the values: lane l < 39 owns value l of the record, lanes 0 / 15 / 18 / 21 also publish their variable's idx ----
    int which = -1, off = 0, size = 0, need = -2;                        // need: the kind the slot must hold
    if (lane < 15) { which = NOM_V_POSE; off = lane; size = 9; need = NOM_KIND_SE23; }
    else if (lane < 18) { which = NOM_V_BG; off = 9 + lane - 15; size = 3; need = NOM_KIND_VEC3; }
    else if (lane < 21) { which = NOM_V_BA; off = 9 + lane - 18; size = 3; need = NOM_KIND_VEC3; }
    else if (lane < 33) { which = NOM_V_EXT; off = lane - 21; size = 6; need = NOM_KIND_SE3; }
    else if (lane < 39) { which = NOM_GNSS + lane - 33; off = 9; size = 1; need = NOM_KIND_SCALAR; }
    bool ok = false;
    int idx = -1;
    if (which >= 0) {
        const int slot = I[which];
        if (slot >= 0 && slot < nv && var[4 * slot] == need) {
            idx = var[4 * slot + 1];
            ok = lane >= 33 || (idx >= 0 && idx + size <= n);            // a registered GNSS scalar is present wherever its column lies
            if (ok) s_rec[ODOM_O_VAL + lane] = D[(size_t)slot * NOM_VD + off];
        }
    }
    const unsigned long long m_ok = __ballot(ok);
    const bool absent = (~m_ok & 0x1ffffffffull) != 0;                    // lanes 0 .. 32: pose, bg, ba, extrinsics
    const int gnss_mask = (int)((m_ok >> 33) & 0x3f);
    if (lane == 0) s_idx[0] = ok ? idx : -1;
    if (lane == 15) s_idx[1] = ok ? idx : -1;
    if (lane == 18) s_idx[2] = ok ? idx : -1;
    if (lane == 21) s_idx[3] = ok ? idx : -1;
    __syncthreads();
    if (lane < 15) {
        const int q = lane < 9 ? 0 : lane < 12 ? 1 : 2;
        s_col[lane] = s_idx[q] < 0 ? -1 : s_idx[q] + (lane < 9 ? lane : lane < 12 ? lane - 9 : lane - 12);
    }
    __syncthreads();

    // ---- cov_err, then the two congruences J S J^T on its 9 x 9 pose block ----
    double* S = s_rec + ODOM_O_ERR;                                      // column-major, ld 15
    if (what & ODOM_W_COV) gather_block(P, ldp, s_col, 15, lane, 64, S);
    if (what & ODOM_W_EUCL) {
        const double* p = s_rec + ODOM_O_VAL + 9;
        const double* v = s_rec + ODOM_O_VAL + 12;
        for (int e = lane; e < 81; e += 64) {                            // error order of the pose block: d_theta, d_p, d_v
            const int a = e / 9, k = e - 9 * a;
            double j = 0.0;
            if (a < 3) j = k < 3 ? neg_skew(p, a, k) : (k - 3 == a ? 1.0 : 0.0);
            else if (a < 6) j = k == a - 3 ? 1.0 : 0.0;
            else j = k < 3 ? neg_skew(v, a - 6, k) : (k - 6 == a - 6 ? 1.0 : 0.0);
            s_J[e] = j;
        }
    }
    __syncthreads();
    if ((what & ODOM_W_EUCL) && lane < 27) {                             // the upper triangles: 21 entries of cov_pose, 6 of cov_vel
        int a = 0, c = 0, r0 = 0, dim = 6, o = ODOM_O_POSE, q = lane;
        if (lane >= 21) { q = lane - 21; r0 = 6; dim = 3; o = ODOM_O_VEL; }
        while (q >= dim - a) { q -= dim - a; ++a; }
        c = a + q;
        const double* Ja = s_J + 9 * (r0 + a);
        const double* Jc = s_J + 9 * (r0 + c);
        double acc = 0.0;
        for (int k = 0; k < 9; ++k) {
            double tk = 0.0;
            for (int l = 0; l < 9; ++l) tk += S[15 * l + k] * Jc[l];
            acc += Ja[k] * tk;
        }
        s_rec[o + a * dim + c] = acc;
        s_rec[o + c * dim + a] = acc;
    }

    // ---- the diagonal of P ----
    int status = absent ? ODOM_S_ABSENT : 0;
    if (what & ODOM_W_DIAG) {
        double mn = INFINITY, mx = -INFINITY;
        for (int i = lane; i < n; i += 64) {
            const double d = P[(size_t)i * (ldp + 1)];
            mn = fmin(mn, d); mx = fmax(mx, d);
        }
        mn = wave_min(mn); mx = wave_max(mx);
        if (n > 0 && lane == 0) { s_rec[ODOM_O_DIAG] = mn; s_rec[ODOM_O_DIAG + 1] = mx; }
        if (n > 0 && mn < 0.0) status |= ODOM_S_NEG_DIAG;
    }
    __syncthreads();

    // ---- the record leaves LDS; the values and cov_err are checked on the way ----
    double* out = rec + (size_t)b * ODOM_REC;
    bool bad = false;
    for (int e = lane; e < ODOM_BODY; e += 64) {
        const double x = s_rec[e];
        out[ODOM_HDR + e] = x;
        if ((e < ODOM_O_DIAG || (e >= ODOM_O_ERR && e < ODOM_O_POSE)) && !isfinite(x)) bad = true;
    }
    if (__ballot(bad)) status |= ODOM_S_NONFINITE;
    if (lane < 4) reinterpret_cast<int*>(out)[lane] = lane == 0 ? n : lane == 1 ? status : lane == 2 ? gnss_mask : 0;
}

// grid = nb filters, block = 256
__global__ __launch_bounds__(256) void k_cov_marginal(CovView cv, const int* __restrict__ cols, const int* __restrict__ ns, int ns_max,
                                                      double* __restrict__ out, int b0)
{
    const int i = blockIdx.x, b = b0 + i, tid = threadIdx.x;
    __shared__ int s_col[MARG_NS_MAX];
    const int m = min(ns[i], min(ns_max, MARG_NS_MAX)), n = cv.n[b];
    if (tid < m) {
        const int g = cols[(size_t)i * ns_max + tid];
        s_col[tid] = (g >= 0 && g < n) ? g : -1;                         // (the host has checked the list against its n)
    }
    __syncthreads();
    gather_block(cov_ptr(cv, b), cv.ldp, s_col, m, tid, 256, out + (size_t)i * ns_max * ns_max);
}

void launch_odom_out(const NomTable& t, const CovView& cv, double* rec, int b0, int nb, int what, hipStream_t st)
{
    hipLaunchKernelGGL(k_odom_out, dim3(nb), dim3(64), 0, st, t, cv, rec, b0, what);
}

void launch_cov_marginal(const CovView& cv, const int* cols, const int* ns, int ns_max, double* out, int b0, int nb, hipStream_t st)
{
    hipLaunchKernelGGL(k_cov_marginal, dim3(nb), dim3(256), 0, st, cv, cols, ns, ns_max, out, b0);
}
