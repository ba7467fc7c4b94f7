// kernels_tail.hip — the landmark tail of a camera frame on the device-resident state (ingvio_nominal_tail):
//   LandmarkUpdate::changeLandmarkAnchor (LandmarkUpdate.cpp:273-361) -> FeatureInfoManager::changeAnchoredPose
//   (MapServerManager.cpp:343-379) -> StateManager::replaceVarLinear (StateManager.cpp:639-693), then margSwPose and
//   margAnchoredLandmarkInState (StateManager.cpp:340-353) for the landmarks that are behind the new anchor or lost.
// Replacing landmark L_a writes row and column L_a only and no H_b reads a landmark other than its own, so the sequence of replacements
// is ONE congruence P' = T P T^T (T = identity except rows L_a = H_a = [-[pf]x 0 | [pf]x 0 | I] over old anchor, new anchor, landmark)
// and the marginalisations are a selection S: the tail is S T P T^T S^T.
//   k_tail_panel  one workgroup per filter: depth test from the table, Z = (T P T^T)[:, landmark columns] (n x 3k, from nine columns of
//                 the ORIGINAL P per landmark), the kept-index -> source-index map, and the table (kinds, idx, anchors, window list)
//   k_tail_write  grid (column tiles, filters): P read once, the other ping-pong half written once, rows / columns of the re-anchored
//                 landmarks substituted from Z on the way; both triangles from the same values, so P stays exactly symmetric
//   k_tail_post   flips cur and sets n
#include "launch_tail.h"

namespace {

#define TAIL_NT 256
#define TAIL_COLS 8

__device__ __forceinline__ int tail_var_size(int kind)
{
    return kind == NOM_KIND_SE23 ? 9 : kind == NOM_KIND_SE3 ? 6 : kind == NOM_KIND_SCALAR ? 1 : 3;
}

__device__ __forceinline__ bool tail_idle(const int* in) { return in[TAIL_N_RE] + in[TAIL_N_ER] + in[TAIL_N_MG] == 0; }

// row c of [pf]x
__device__ __forceinline__ void skew_row(const double* pf, int c, double s[3])
{
    s[0] = c == 0 ? 0.0 : c == 1 ? pf[2] : -pf[1];
    s[1] = c == 0 ? -pf[2] : c == 1 ? 0.0 : pf[0];
    s[2] = c == 0 ? pf[1] : c == 1 ? -pf[0] : 0.0;
}

__global__ __launch_bounds__(TAIL_NT) void k_tail_panel(TailLaunch L)
{
    extern __shared__ int s_dyn[];
    __shared__ double s_pf[TAIL_LM_MAX][3];
    __shared__ int s_L[TAIL_LM_MAX], s_o[TAIL_LM_MAX], s_v[TAIL_LM_MAX];
    __shared__ int s_nw, s_wave[TAIL_NT / WAVE];
    const int bl = blockIdx.x, b = L.b0 + bl, tid = threadIdx.x;
    const int* in = L.in + (size_t)bl * L.istride;
    if (tail_idle(in)) return;
    const int k = in[TAIL_N_RE], nws = in[TAIL_NEW], ne = in[TAIL_N_ER], nm = in[TAIL_N_MG];
    const int* lm_slot = in + TAIL_HDR;
    const int* er_slot = lm_slot + L.kcap;
    const int* mg_slot = er_slot + L.ecap;
    int* I = L.t.ih + (size_t)b * L.t.ir;
    int* var = I + NOM_IH;
    const double* D = L.t.dv + (size_t)b * L.t.dr + NOM_DH;
    const int n = L.cv.n[b], ld = L.cv.ldp;
    const double* P = cov_ptr(L.cv, b);
    double* Z = L.Z + (size_t)bl * L.zstride;
    int* flag = s_dyn;            // per source index: -1 kept, -2 dropped, >= 0 panel column of a re-anchored landmark
    int* pre = s_dyn + ld;        // kept entries in front of a source index = its index after the call

    for (int r = tid; r < n; r += TAIL_NT) flag[r] = -1;
    if (tid < k) {
        // body = R_new^T (p_f - p_new); body.z <= 0: marginalised instead of re-anchored (LandmarkUpdate.cpp:295-302)
        const int sl = lm_slot[tid], an = var[4 * sl + 2];
        const double* pf = D + (size_t)sl * NOM_VD + 9;
        const double* Rn = D + (size_t)nws * NOM_VD;
        const double d0 = pf[0] - Rn[9], d1 = pf[1] - Rn[10], d2 = pf[2] - Rn[11];
        const double z = Rn[2] * d0 + Rn[5] * d1 + Rn[8] * d2;
        const int v = z <= 0.0 ? 0 : 1;
        s_pf[tid][0] = pf[0]; s_pf[tid][1] = pf[1]; s_pf[tid][2] = pf[2];
        s_L[tid] = var[4 * sl + 1]; s_o[tid] = var[4 * an + 1]; s_v[tid] = v;
        L.verdict[(size_t)bl * L.kcap + tid] = v;
    }
    if (tid == 0) s_nw = k ? var[4 * nws + 1] : 0;
    __syncthreads();
    if (tid < k) for (int c = 0; c < 3; ++c) flag[s_L[tid] + c] = s_v[tid] ? 3 * tid + c : -2;
    // (an erased slot holds a landmark, 3 columns, or a GNSS scalar, 1 column: ingvio_nominal_marg_gnss)
    for (int e = tid; e < ne; e += TAIL_NT) { const int ix = var[4 * er_slot[e] + 1], sz = tail_var_size(var[4 * er_slot[e]]); for (int c = 0; c < sz; ++c) flag[ix + c] = -2; }
    for (int e = tid; e < nm; e += TAIL_NT) { const int ix = var[4 * mg_slot[e] + 1]; for (int c = 0; c < 6; ++c) flag[ix + c] = -2; }
    // ---- Y_a = P H_a^T for every re-anchored landmark (StateManager.cpp:671-681), from the original P ----
    const int nw = s_nw;
    for (int e = tid; e < n * k; e += TAIL_NT) {
        const int r = e % n, a = e / n;
        if (!s_v[a]) continue;
        const int o = s_o[a], la = s_L[a];
        double po[3], pn[3], pl[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            po[l] = P[r + (size_t)(o + l) * ld]; pn[l] = P[r + (size_t)(nw + l) * ld]; pl[l] = P[r + (size_t)(la + l) * ld];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double s[3], acc = 0.0;
            skew_row(s_pf[a], c, s);
#pragma unroll
            for (int l = 0; l < 3; ++l) acc += po[l] * -s[l];
#pragma unroll
            for (int l = 0; l < 3; ++l) acc += pn[l] * s[l];
            acc += pl[c];
            Z[r + (size_t)(3 * a + c) * ld] = acc;
        }
    }
    __syncthreads();
    // ---- the landmark rows: P'[L_b, L_a] = H_b Y_a (:683-685; cross blocks a != b of the joint transform).  A thread reads clone rows,
    //      which nobody writes here, and the one element it overwrites ----
    const int k3 = 3 * k;
    for (int e = tid; e < k3 * k3; e += TAIL_NT) {
        const int col = e / k3, rr = e % k3, bb = rr / 3, cb = rr % 3;
        if (!s_v[bb] || !s_v[col / 3]) continue;
        const double* Zc = Z + (size_t)col * ld;
        const int row = s_L[bb] + cb, o = s_o[bb];
        double s[3], acc = 0.0;
        skew_row(s_pf[bb], cb, s);
#pragma unroll
        for (int l = 0; l < 3; ++l) acc += -s[l] * Zc[o + l];
#pragma unroll
        for (int l = 0; l < 3; ++l) acc += s[l] * Zc[nw + l];
        acc += Zc[row];
        Z[row + (size_t)col * ld] = acc;
    }
    // ---- kept index -> source index: an exclusive scan of the kept flags over the workgroup ----
    const int per = (n + TAIL_NT - 1) / TAIL_NT, r0 = tid * per, r1 = min(r0 + per, n);
    int cnt = 0;
    for (int r = r0; r < r1; ++r) cnt += flag[r] != -2;
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { const int t = __shfl_up(inc, off, WAVE); if ((tid & (WAVE - 1)) >= off) inc += t; }
    if ((tid & (WAVE - 1)) == WAVE - 1) s_wave[tid / WAVE] = inc;
    __syncthreads();
    int base = inc - cnt, total = 0;
    for (int w = 0; w < TAIL_NT / WAVE; ++w) { if (w < tid / WAVE) base += s_wave[w]; total += s_wave[w]; }
    int* map = L.map + (size_t)bl * ld;
    int* tag = L.tag + (size_t)bl * ld;
    for (int r = r0; r < r1; ++r) {
        pre[r] = base;
        if (flag[r] != -2) { map[base] = r; tag[base] = flag[r]; ++base; }
    }
    if (tid == 0) L.nnew[bl] = total;
    __syncthreads();
    // ---- the table: the window list closes up over the clones that left (StateManager.cpp:155-192), freed slots take kind NONE,
    //      every surviving idx moves down by the size of what left below it, a re-anchored landmark names its new anchor
    //      (resetAnchoredPose(.., true): its world position stays) ----
    if (tid == 0) {
        const int nc = I[NOM_N_CLONES];
        int w = 0;
        for (int q = 0; q < nc; ++q) {
            const int sl = I[NOM_CLONES + q];
            bool gone = false;
            for (int e = 0; e < nm; ++e) gone |= mg_slot[e] == sl;
            if (!gone) I[NOM_CLONES + w++] = sl;
        }
        I[NOM_N_CLONES] = w;
    }
    const int nv = I[NOM_N_VAR];
    for (int v = tid; v < nv; v += TAIL_NT) {
        if (var[4 * v] == NOM_KIND_NONE) continue;
        const int ix = var[4 * v + 1];
        if (flag[ix] == -2) {
            if (var[4 * v] == NOM_KIND_SCALAR)                         // a GNSS scalar that leaves is no longer registered (StateManager.cpp:233-242)
                for (int q = 0; q < 6; ++q) if (I[NOM_GNSS + q] == v) I[NOM_GNSS + q] = -1;
            var[4 * v] = NOM_KIND_NONE; var[4 * v + 1] = -1; var[4 * v + 2] = -1;
        } else var[4 * v + 1] = pre[ix];
    }
    if (tid < k && s_v[tid]) var[4 * lm_slot[tid] + 2] = nws;
}

__global__ __launch_bounds__(TAIL_NT) void k_tail_write(TailLaunch L)
{
    const int bl = blockIdx.y, b = L.b0 + bl, tid = threadIdx.x;
    if (tail_idle(L.in + (size_t)bl * L.istride)) return;
    const int nn = L.nnew[bl], ld = L.cv.ldp, j0 = blockIdx.x * TAIL_COLS;
    if (j0 >= nn) return;
    const double* src = cov_ptr(L.cv, b);
    double* dst = cov_alt_ptr(L.cv, b);
    const int* map = L.map + (size_t)bl * ld;
    const int* tag = L.tag + (size_t)bl * ld;
    const double* Z = L.Z + (size_t)bl * L.zstride;
    for (int i = tid; i < nn; i += TAIL_NT) {
        const int si = map[i], ti = tag[i];
        for (int jj = 0; jj < TAIL_COLS; ++jj) {
            const int j = j0 + jj;
            if (j >= nn) break;
            const int sj = map[j], tj = tag[j];
            double v;
            if (tj >= 0) {
                v = Z[si + (size_t)tj * ld];
                if (ti >= 0) v = 0.5 * (v + Z[sj + (size_t)ti * ld]);      // a landmark block: both roundings of the same entry, as k_replace_var's diagonal
            } else if (ti >= 0) v = Z[sj + (size_t)ti * ld];
            else v = NT_LOAD(&src[si + (size_t)sj * ld]);
            NT_STORE(&dst[i + (size_t)j * ld], v);
        }
    }
}

__global__ void k_tail_post(TailLaunch L)
{
    const int bl = blockIdx.x * blockDim.x + threadIdx.x;
    if (bl >= L.nb || tail_idle(L.in + (size_t)bl * L.istride)) return;
    const int b = L.b0 + bl;
    L.cv.cur[b] ^= 1;
    L.cv.n[b] = L.nnew[bl];
}

}  // namespace

int launch_tail(const TailLaunch& L, int n_cap, hipStream_t st)
{
    const size_t lds = tail_panel_lds(L.cv.ldp);
    if (L.nb < 1 || L.kcap < 0 || L.kcap > TAIL_LM_MAX || lds > TAIL_LDS_MAX || n_cap > L.cv.ldp ||
        L.zstride < (size_t)L.cv.ldp * 3 * (size_t)L.kcap) return -1;
    hipLaunchKernelGGL(k_tail_panel, dim3(L.nb), dim3(TAIL_NT), lds, st, L);
    hipLaunchKernelGGL(k_tail_write, dim3((n_cap + TAIL_COLS - 1) / TAIL_COLS, L.nb), dim3(TAIL_NT), 0, st, L);
    hipLaunchKernelGGL(k_tail_post, dim3((L.nb + 255) / 256), dim3(256), 0, st, L);
    return 0;
}
