// kernels_nominal.hip — the device-resident nominal state (ingvio_nominal_*): the retractions of StateManager::boxPlus and
// the marginalisation's drop / index shift on the per-filter variable table of launch_nominal.h.
//
// One wave per filter, one lane per variable: every variable reads dx (and, for a landmark, its anchor's idx, which boxPlus does not
// change) and writes only its own value, so the lanes are independent and all loads are in flight together.  The formulas follow the
// C oracle (oracle/ingvio_oracle.c: orc_gamma, orc_se3_update, orc_se23_update) operation for operation, the small-angle branch
// (|theta| < 1e-6: Gamma_0 = Gamma_1 = I) included.
// gfx950 only.
#include <hip/hip_runtime.h>

#include "launch_nominal.h"

namespace {

// AuxGammaFunc.cpp:46-113 for m = 0, 1 (row-major out)
__device__ __forceinline__ void gamma01(const double* v, double G0[9], double G1[9])
{
    const double theta = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 9; ++i) { G0[i] = 0.0; G1[i] = 0.0; }
    if (fabs(theta) < 1e-06) {
        G0[0] = G0[4] = G0[8] = 1.0;
        G1[0] = G1[4] = G1[8] = 1.0;
        return;
    }
    const double n0 = v[0] / theta, n1 = v[1] / theta, n2 = v[2] / theta;
    const double nx[9] = { 0.0, -n2, n1, n2, 0.0, -n0, -n1, n0, 0.0 };
    double nx2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) nx2[3 * i + j] = nx[3 * i] * nx[j] + nx[3 * i + 1] * nx[3 + j] + nx[3 * i + 2] * nx[6 + j];
    double s, c;
    sincos(theta, &s, &c);
    const double a1 = s, a2 = 1.0 - c;                                   // Gamma_0
    const double b1 = (1.0 - c) / theta, b2 = (theta - s) / theta;       // Gamma_1
    for (int i = 0; i < 9; ++i) { G0[i] = a1 * nx[i] + a2 * nx2[i]; G1[i] = b1 * nx[i] + b2 * nx2[i]; }
    G0[0] += 1.0; G0[4] += 1.0; G0[8] += 1.0;
    G1[0] += 1.0; G1[4] += 1.0; G1[8] += 1.0;
}

__device__ __forceinline__ void mulv(const double A[9], const double* x, double y[3])
{
    for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}

}  // namespace

// grid = nb filters, block = one wave.  MARG: after the retraction, the variable of idx marg[b] (a window clone) leaves the table (its
// slot becomes free, the window list closes up) and every variable behind it moves 6 columns down.
// GATHER (never with MARG): after the retraction (skipped when dx is absent) the wave copies what the landmark update reads - pose,
// extrinsics, the staged landmarks' positions and every idx - from the table into the staged SoA (NomGather).  A lane is a staged
// landmark there, not a table slot: it reads back what the wave has just written, behind the barrier.
template <bool MARG, bool GATHER = false>
__global__ __launch_bounds__(64) void k_nominal_update(NomTable t, const double* __restrict__ dx, int ldx, const int* __restrict__ marg, int b0, NomGather g)
{
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    int* I = t.ih + (size_t)b * t.ir;
    int* var = I + NOM_IH;
    double* D = t.dv + (size_t)b * t.dr + NOM_DH;
    const double* d = dx + (size_t)b * ldx;
    const int nv = I[NOM_N_VAR];
    for (int v = lane; v < ((GATHER && !dx) ? 0 : nv); v += 64) {
        const int kind = var[4 * v], idx = var[4 * v + 1];
        double* x = D + (size_t)v * NOM_VD;
        if (kind == NOM_KIND_SE23 || kind == NOM_KIND_SE3) {             // PoseState.cpp:174-186 / :79-88
            double G0[9], G1[9], R[9], t1[3], t2[3];
            gamma01(d + idx, G0, G1);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) R[3 * i + j] = G0[3 * i] * x[j] + G0[3 * i + 1] * x[3 + j] + G0[3 * i + 2] * x[6 + j];
            mulv(G0, x + 9, t1); mulv(G1, d + idx + 3, t2);
            for (int i = 0; i < 9; ++i) x[i] = R[i];
            for (int i = 0; i < 3; ++i) x[9 + i] = t1[i] + t2[i];
            if (kind == NOM_KIND_SE23) {
                mulv(G0, x + 12, t1); mulv(G1, d + idx + 6, t2);
                for (int i = 0; i < 3; ++i) x[12 + i] = t1[i] + t2[i];
            }
        } else if (kind == NOM_KIND_VEC3) {                             // VecState.cpp:25-29
            for (int i = 0; i < 3; ++i) x[9 + i] = x[9 + i] + d[idx + i];
        } else if (kind == NOM_KIND_SCALAR) {                           // VecState.cpp:40-44
            x[9] = x[9] + d[idx];
        } else if (kind == NOM_KIND_LM) {                               // AnchoredLandmark.cpp:227-243: the anchor's d_theta
            const int as = var[4 * v + 2], a = as >= 0 ? var[4 * as + 1] : -1;
            if (a < 0) {                                                 // no live anchor: p + delta_p (AnchoredLandmark.cpp:238-242)
                for (int i = 0; i < 3; ++i) x[9 + i] = x[9 + i] + d[idx + i];
                continue;
            }
            double G0[9], G1[9], t1[3], t2[3];
            gamma01(d + a, G0, G1);
            mulv(G0, x + 9, t1); mulv(G1, d + idx, t2);
            for (int i = 0; i < 3; ++i) x[9 + i] = t1[i] + t2[i];
        }
    }
    if (GATHER) {
        __syncthreads();                                                 // the values the other lanes have just retracted
        const int vp = I[NOM_V_POSE], vx = I[NOM_V_EXT];
        if (lane < 24) g.pose[(size_t)b * 24 + lane] = D[(size_t)(lane < 12 ? vp : vx) * NOM_VD + (lane < 12 ? lane : lane - 12)];
        if (lane < 2) g.idx[2 * b + lane] = var[4 * (lane ? vx : vp) + 1];
        const int nl = min(g.n_lm[b], g.lmax);
        for (int l = lane; l < nl; l += 64) {
            const size_t o = (size_t)b * g.lmax + l;
            const int s = g.slot[o];
            const bool ok = s >= 0 && s < nv && var[4 * s] == NOM_KIND_LM;
            const int as = ok ? var[4 * s + 2] : -1;
            g.lm_idx[o] = ok ? var[4 * s + 1] : -1;
            g.anchor_idx[o] = (as >= 0 && as < nv) ? var[4 * as + 1] : -1;
            for (int i = 0; i < 3; ++i) g.pf[3 * o + i] = ok ? D[(size_t)s * NOM_VD + 9 + i] : 0.0;
        }
    }
    if (!MARG) return;
    const int m = marg[b];
    if (m < 0) return;
    __shared__ int s_drop;
    if (lane == 0) {                                                     // the window list closes up over the clone that leaves
        const int nc = I[NOM_N_CLONES];
        int w = 0, drop = -1;
        for (int q = 0; q < nc; ++q) {
            const int s = I[NOM_CLONES + q];
            if (drop < 0 && var[4 * s + 1] == m) { drop = s; continue; }
            I[NOM_CLONES + w++] = s;
        }
        I[NOM_N_CLONES] = w;
        s_drop = drop;
    }
    __syncthreads();
    const int drop = s_drop;
    for (int v = lane; v < nv; v += 64) {
        if (var[4 * v] == NOM_KIND_NONE) continue;
        if (v == drop) { var[4 * v] = NOM_KIND_NONE; var[4 * v + 1] = -1; var[4 * v + 2] = -1; }
        else if (var[4 * v + 1] > m) var[4 * v + 1] -= 6;
    }
}

// The trailing retraction of a frame whose in-frame GNSS update rode on the MSCKF write-back: boxPlus of a dx given
// in the index space AFTER the frame's marginalisation, then the drop and the shift of k_nominal_update<true>, in one launch.  The
// table's idx are still those before the marginalisation, so every lane maps its idx (a landmark lane also its anchor's) through the
// shift before it reads dx; the clone that leaves has no entry in dx and is not retracted.  A kernel of its own beside
// k_nominal_update - the same formulas, written out again - so that the instantiations above keep their code and registers.
__global__ __launch_bounds__(64) void k_nominal_update_post(NomTable t, const double* __restrict__ dx, int ldx, const int* __restrict__ marg, int b0)
{
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    int* I = t.ih + (size_t)b * t.ir;
    int* var = I + NOM_IH;
    double* D = t.dv + (size_t)b * t.dr + NOM_DH;
    const double* d = dx + (size_t)b * ldx;
    const int nv = I[NOM_N_VAR];
    const int m = marg[b];
    auto post = [m](int i) { return (m >= 0 && i > m) ? i - 6 : i; };    // idx before the marginalisation -> idx behind it
    for (int v = lane; v < nv; v += 64) {
        const int kind = var[4 * v], idx = var[4 * v + 1];
        if (kind == NOM_KIND_NONE || idx == m) continue;                 // (idx == m: the clone that leaves)
        const double* dv = d + post(idx);
        double* x = D + (size_t)v * NOM_VD;
        if (kind == NOM_KIND_SE23 || kind == NOM_KIND_SE3) {
            double G0[9], G1[9], R[9], t1[3], t2[3];
            gamma01(dv, G0, G1);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) R[3 * i + j] = G0[3 * i] * x[j] + G0[3 * i + 1] * x[3 + j] + G0[3 * i + 2] * x[6 + j];
            mulv(G0, x + 9, t1); mulv(G1, dv + 3, t2);
            for (int i = 0; i < 9; ++i) x[i] = R[i];
            for (int i = 0; i < 3; ++i) x[9 + i] = t1[i] + t2[i];
            if (kind == NOM_KIND_SE23) {
                mulv(G0, x + 12, t1); mulv(G1, dv + 6, t2);
                for (int i = 0; i < 3; ++i) x[12 + i] = t1[i] + t2[i];
            }
        } else if (kind == NOM_KIND_VEC3) {
            for (int i = 0; i < 3; ++i) x[9 + i] = x[9 + i] + dv[i];
        } else if (kind == NOM_KIND_SCALAR) {
            x[9] = x[9] + dv[0];
        } else if (kind == NOM_KIND_LM) {
            const int as = var[4 * v + 2], a = as >= 0 ? var[4 * as + 1] : -1;
            if (a < 0 || a == m) {                                       // no live anchor (a stage refuses a landmark on the leaving clone)
                for (int i = 0; i < 3; ++i) x[9 + i] = x[9 + i] + dv[i];
                continue;
            }
            double G0[9], G1[9], t1[3], t2[3];
            gamma01(d + post(a), G0, G1);
            mulv(G0, x + 9, t1); mulv(G1, dv, t2);
            for (int i = 0; i < 3; ++i) x[9 + i] = t1[i] + t2[i];
        }
    }
    if (m < 0) return;
    __shared__ int s_drop;
    if (lane == 0) {                                                     // the window list closes up over the clone that leaves
        const int nc = I[NOM_N_CLONES];
        int w = 0, drop = -1;
        for (int q = 0; q < nc; ++q) {
            const int s = I[NOM_CLONES + q];
            if (drop < 0 && var[4 * s + 1] == m) { drop = s; continue; }
            I[NOM_CLONES + w++] = s;
        }
        I[NOM_N_CLONES] = w;
        s_drop = drop;
    }
    __syncthreads();                                                     // every lane has read the idx it needed (its own, its anchor's)
    const int drop = s_drop;
    for (int v = lane; v < nv; v += 64) {
        if (var[4 * v] == NOM_KIND_NONE) continue;
        if (v == drop) { var[4 * v] = NOM_KIND_NONE; var[4 * v + 1] = -1; var[4 * v + 2] = -1; }
        else if (var[4 * v + 1] > m) var[4 * v + 1] -= 6;
    }
}

// StateManager::addGNSSVariable (StateManager.cpp:194-231) for filter b0 + blockIdx.x: an independent 1 x 1 block at the live n (row and
// column n zero over [0, n), the diagonal var - k_append's arithmetic), the scalar's record in the table slot the host chose, registered
// at NOM_GNSS + gtype.  gs [nb][2] = {gtype (-1: nothing for this filter), slot}, vv [nb][2] = {value, var}.  The host has checked on its
// mirror that the slot is free and inside the table and that n + 1 columns fit.
__global__ __launch_bounds__(256) void k_nominal_add_gnss(CovView cv, NomTable t, int b0, const int* __restrict__ gs, const double* __restrict__ vv)
{
    const int bl = blockIdx.x, b = b0 + bl, tid = threadIdx.x;
    const int gtype = gs[2 * bl], slot = gs[2 * bl + 1];
    if (gtype < 0) return;                                             // (uniform over the workgroup: ahead of the barrier)
    const int n = cv.n[b], ld = cv.ldp;
    double* P = cov_ptr(cv, b);
    for (int r = tid; r < n; r += 256) {
        P[r + (size_t)n * ld] = 0.0;
        P[n + (size_t)r * ld] = 0.0;
    }
    __syncthreads();                                                   // every wave has read n before thread 0 stores n + 1 (as k_append)
    if (tid != 0) return;
    P[n + (size_t)n * ld] = vv[2 * bl + 1];
    int* I = t.ih + (size_t)b * t.ir;
    int* v = I + NOM_IH + 4 * slot;
    v[0] = NOM_KIND_SCALAR; v[1] = n; v[2] = -1; v[3] = 0;
    double* x = t.dv + (size_t)b * t.dr + NOM_DH + (size_t)slot * NOM_VD;
    for (int i = 0; i < NOM_VD; ++i) x[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    x[9] = vv[2 * bl];
    I[NOM_GNSS + gtype] = slot;
    if (slot >= I[NOM_N_VAR]) I[NOM_N_VAR] = slot + 1;
    cv.n[b] = n + 1;
}

void launch_nominal_add_gnss(const CovView& cv, const NomTable& t, int b0, int nb, const int* gs, const double* vv, hipStream_t st)
{
    hipLaunchKernelGGL(k_nominal_add_gnss, dim3(nb), dim3(256), 0, st, cv, t, b0, gs, vv);
}

void launch_nominal_update(const NomTable& t, const double* dx, int ldx, const int* marg, int b0, int nb, hipStream_t st)
{
    if (marg) hipLaunchKernelGGL(k_nominal_update<true>, dim3(nb), dim3(64), 0, st, t, dx, ldx, marg, b0, NomGather{});
    else hipLaunchKernelGGL(k_nominal_update<false>, dim3(nb), dim3(64), 0, st, t, dx, ldx, marg, b0, NomGather{});
}

void launch_nominal_gather(const NomTable& t, const double* dx, int ldx, const NomGather& g, int b0, int nb, hipStream_t st)
{
    hipLaunchKernelGGL((k_nominal_update<false, true>), dim3(nb), dim3(64), 0, st, t, dx, ldx, (const int*)nullptr, b0, g);
}

void launch_nominal_update_post(const NomTable& t, const double* dx, int ldx, const int* marg, int b0, int nb, hipStream_t st)
{
    hipLaunchKernelGGL(k_nominal_update_post, dim3(nb), dim3(64), 0, st, t, dx, ldx, marg, b0);
}
