// gram3_kernel.h — K4 + K6 + K7 in Gram form, third generation for the window classes of up to 11 clones: the wave pairs of a
// workgroup decoupled, ONE barrier per batch.  k_feat_gram3<CMAX, STEREO, RED>; RED = true is the product kernel of the fused frame
// step (launch_ft takes it where it took k_feat_gram2<.., true>, context switch ingvio_set_gram_decoupled), RED = false is the variant
// build's INGVIO_GRAM=3 (tests/test_gpu_alternatives.py).
//
// k_feat_gram2 walks a chunk in batches of 8 features in PHASES: all four waves run the rank-3 product Z^T Z of batch i (P3a), a
// barrier, then waves 0-1 build the operand rows of batch i + 1 (P2) beside the sparse sums of batch i on waves 2-3 (P3b), a second
// barrier.  Every wave waits through P3a, then waves 2-3 wait while waves 0-1 finish their rows.  Here the operand panel Z and the
// sparse scratch are double-buffered: per batch waves 0-1 (producers) run P2 of batch i + 1 into the other buffers, waves 2-3
// (consumers) run P3b of batch i, and the tiles of the rank-3 product of batch i are DEALT over all four waves by a compile-time table
// (Gram3Deal) - the matrix pipes are per SIMD, so tiles taken off a wave are issue cycles taken off its SIMD.  The two roles are separate
// loops with the same number of barriers each (one in front of the loop, one per batch - an empty chunk passes the first only), so
// that neither role carries the other's registers.
//
// History.  Round 6 measured the full-form kernel with (slot, anchor) sparse lanes at 114-117 us per 512 filters against gram2's
// 106-108 and rejected it: per batch and workgroup it issued P2 2 x 3.1 k cycles, 96 MFMAs 6.1 k, P3b 2 x 3.9 k - ~10 k on every SIMD
// with two workgroups per CU, out of a batch period of 11.7 k: issue-bound.  Since then the reduced panel (Gram2Cfg<CMAX, true>: no
// columns for the solve's reference clone, 10 upper tiles instead of 15 in class 11, 60 MFMAs per batch) and the by-lane sparse sums
// (lane = (slot, chunk of three values), one accumulator triple per anchor, 3 LDS values per feature and lane instead of 34) took about
// a third off that issue stream, while gram2's phases kept its period where it was.  This file is that kernel in the reduced, by-lane
// form, with the anchor's accumulator triple picked by index (GRAM3_P3B_INDEXED below).  Same sums in the same order as
// k_feat_gram2<.., RED>: a tile accumulates the batches in list order and the k-steps in order, the sparse additions run in feature
// order - the chunk partials are bit-identical (tests/test_gpu_gram_decoupled.py).
// Measured on MI355X, 512 filters of config 2: 77.4 us against k_feat_gram2<11, true, true>'s 83.5 (sigma 1.0).  Stamps of
// one batch, deal 1/1/4/4 (wall clock of a wave; the SIMD is shared with the same wave of the CU's other workgroup): producer rows
// 5.3 k + its tile 1.0 k + wait 0.4 k, consumer tiles 3.1 k + sparse sums 2.5 k + wait 1.2 k - a period of 6.8 k cycles.
// LDS, class 11 reduced: two Z panels 2 x 24 x 64 x 8 = 24.6 KB, two scratch buffers 47.9 KB (the epilogue view, 62.7 KB, overlays
// them), lists and poses ~3 KB: 76 KB of the 80 KB that two workgroups per CU leave each.
#pragma once

// Tiles of the rank-3 product per wave (waves 0-1 build rows, waves 2-3 run the sparse sums), upper tiles row-major over ti <= tj,
// consecutive runs.  Class 11 reduced has 10 tiles: 1/1/4/4 77.4 us, 2/2/3/3 81.2, 0/0/5/5 86.0, 0/1/4/5 81.8.  The full
// forms keep round 6's deals.  Exchanging the roles of the wave pairs in every second resident workgroup (by the hardware wave slot)
// was measured once and not kept: 77.8 against 77.5 us.
#ifndef GRAM3_DEAL_11R
#define GRAM3_DEAL_11R 1, 1, 4, 4
#endif
// The sparse sums' accumulators: 1 - the triple of the feature's anchor picked by index (77.4 us), 0 - k_feat_gram2's selector form,
// 33 multiply-adds per feature of which 30 add zero (80.9 us)
#ifndef GRAM3_P3B_INDEXED
#define GRAM3_P3B_INDEXED 1
#endif
#ifndef GRAM3_DEAL_6R
#define GRAM3_DEAL_6R 0, 0, 2, 1
#endif
template <int D0_, int D1_, int D2_, int D3_>
struct Gram3DealT { static constexpr int D0 = D0_, D1 = D1_, D2 = D2_, D3 = D3_; };
template <int CMAX, bool RED> struct Gram3Deal;
template <> struct Gram3Deal<11, true> : Gram3DealT<GRAM3_DEAL_11R> {};
template <> struct Gram3Deal<11, false> : Gram3DealT<5, 5, 3, 2> {};
template <> struct Gram3Deal<6, true> : Gram3DealT<GRAM3_DEAL_6R> {};
template <> struct Gram3Deal<6, false> : Gram3DealT<2, 2, 1, 1> {};

template <int CMAX, bool RED = false>
struct Gram3Batch {
    using Cfg = Gram2Cfg<CMAX, RED>;
    double Zm[2][Cfg::KR][Cfg::LDW];                              // the operand panel, double-buffered
    double sp[2][GRAM_NB][CMAX][Cfg::SPW];                        // per (feature, slot) sparse scratch, double-buffered
};
template <int CMAX, bool RED = false>
constexpr size_t gram3_lds_bytes()           // the batch view and the epilogue view share the LDS; the feature lists follow
{
    return ((std::max(sizeof(Gram3Batch<CMAX, RED>), sizeof(Gram2Out<CMAX, RED>)) + 15) / 16) * 16;
}

template <int CMAX, bool STEREO, bool RED = false>
__global__ __launch_bounds__(GRAM_NT, 2) void k_feat_gram3(
    FrameView fv, MsckfOpts op, int b0, const int* __restrict__ accept_in, int* __restrict__ used_out,
    double* __restrict__ Apart, int* __restrict__ chunk_used, int G, int rstride)
{
    using Cfg = Gram2Cfg<CMAX, RED>;
    using Deal = Gram3Deal<CMAX, RED>;
    constexpr int NC = Cfg::NC, TJ = Cfg::TJ, LDW = Cfg::LDW, KR = Cfg::KR;
    constexpr int NUP = Cfg::NUP, TI = Cfg::TI, RPO = STEREO ? 4 : 2;
    constexpr int D0 = Deal::D0, D1 = Deal::D1, D2 = Deal::D2, D3 = Deal::D3;
    static_assert(D0 + D1 + D2 + D3 == NUP && D0 >= 0 && D1 >= 0 && D2 >= 0 && D3 >= 0, "the deal covers every upper tile once");
    static_assert(CMAX * CMAX <= 128 && 11 * CMAX <= 128, "the sparse lanes and the epilogue's pair lanes sit on waves 2-3");
    constexpr int NPR = D0 > D1 ? D0 : D1, NCO = D2 > D3 ? D2 : D3;      // accumulator tiles of a producer / consumer wave
    constexpr int NMX = NPR > NCO ? NPR : NCO;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    Gram3Batch<CMAX, RED>& sb = *reinterpret_cast<Gram3Batch<CMAX, RED>*>(smem_raw);
    Gram2Out<CMAX, RED>& so = *reinterpret_cast<Gram2Out<CMAX, RED>*>(smem_raw);             // epilogue view of the same LDS
    int* sUse = reinterpret_cast<int*>(smem_raw + gram3_lds_bytes<CMAX, RED>());
    int* sList = sUse + fv.fmax;
    __shared__ int sNu;
    __shared__ double sPose[16][12];                              // the window's clone poses: R (9, row-major), p (3)
    // wave as a scalar: the tile coordinates of a wave's accumulators are wave-uniform (see k_feat_gram_big)
    const int bl = blockIdx.y, b = b0 + bl, g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = fv.n_feat[b], C = fv.n_clones[b], ncol = 6 * C;
    const int cref = RED ? C - 1 : -1;                            // the solve's reference clone: no panel columns, no block row / column
    for (int e = tid; e < 12 * C; e += GRAM_NT) {
        const int c = e / 12, q = e - 12 * c;
        sPose[c][q] = q < 9 ? fv.clone_R[((size_t)b * fv.cmax + c) * 9 + q] : fv.clone_p[((size_t)b * fv.cmax + c) * 3 + q - 9];
    }

    dbg_stamp(32);
    for (int j = tid; j < F; j += GRAM_NT) {                    // RemoveLostUpdate.cpp:357-359
        int use = accept_in[(size_t)b * fv.fmax + j];
        if (use && op.max_accept > 0) {
            int rank = 0;
            for (int q = 0; q < j; ++q) rank += accept_in[(size_t)b * fv.fmax + q];
            if (rank >= op.max_accept) use = 0;
        }
        sUse[j] = use;
        if (g == 0) used_out[(size_t)b * fv.fmax + j] = use;
    }
    // zero BOTH operand panels once: padding columns, the reference slot's columns (RED) and rows of a short last batch stay zero
    for (int e = tid; e < 2 * KR * LDW; e += GRAM_NT) (&sb.Zm[0][0][0])[e] = 0.0;
    __syncthreads();
    if (wave == 0) {                                            // ordered list of the used features
        int cnt = 0;
        for (int base = 0; base < F; base += WAVE) {
            const int j = base + lane;
            const bool u = j < F && sUse[j];
            const unsigned long long m = __ballot(u);
            if (u) sList[cnt + __popcll(m & ((1ULL << lane) - 1ULL))] = j;
            cnt += __popcll(m);
        }
        if (lane == 0) sNu = cnt;
    }
    __syncthreads();
    const int nu = sNu, per = (nu + G - 1) / G;
    const int q0 = g * per, q1 = min(nu, q0 + per);

    dbg_stamp(33);
    // waves 2-3: the sparse lanes (slot, chunk of three of the slot's 33 values) of the batch loop, the (slot, anchor) pair lanes of the epilogue
    const int ptid = tid - 128;
    const int pc = ptid >= 0 ? ptid / CMAX : 0, pa = ptid >= 0 ? ptid - pc * CMAX : 0;
    const bool pairlane = ptid >= 0 && ptid < CMAX * CMAX;
    const int uc = ptid >= 0 ? ptid / 11 : 0, uj = ptid >= 0 ? ptid - 11 * uc : 0;
    const bool ulane = ptid >= 0 && ptid < 11 * CMAX;
    const int kq = lane >> 4, l15 = lane & 15;

    // this wave's tiles: a run of the upper tiles t (row-major over ti <= tj) starting at tbeg
    const int tcnt = wave == 0 ? D0 : (wave == 1 ? D1 : (wave == 2 ? D2 : D3));
    const int tbeg = wave == 0 ? 0 : (wave == 1 ? D0 : (wave == 2 ? D0 + D1 : D0 + D1 + D2));
    int tiA[NMX], tjA[NMX];
#pragma unroll
    for (int u = 0; u < NMX; ++u) {
        int t = u < tcnt ? tbeg + u : NUP, ti = 0;
        while (ti < TI - 1 && t >= TJ - ti) { t -= TJ - ti; ++ti; }
        tiA[u] = ti; tjA[u] = ti + t;                          // t >= NUP gives tj >= TJ: never launched
    }
    // this wave's tiles of the rank-3 part of batch qb, Z^T Z over its stacked rows; NA: the accumulators its ROLE carries
    auto do_p3a = [&](auto& acc, auto na_c, int qb, int buf) {
        constexpr int NA = decltype(na_c)::value;
        const int nbf = min(GRAM_NB, q1 - qb);
        const int nst = (3 * nbf + 3) >> 2;
#pragma unroll
        for (int st = 0; st < KR / 4; ++st) {                // fully unrolled: the fragment reads of the later steps are
            if (st < nst) {                                  // issued while the earlier MFMAs run
#pragma unroll
                for (int u = 0; u < NA; ++u) {
                    if (u < tcnt) {
                        const int ti = tiA[u], tj = tjA[u];
                        const double af = sb.Zm[buf][4 * st + kq][16 * ti + l15];      // A[i][k] = Z[k][i]
                        const double bf = sb.Zm[buf][4 * st + kq][16 * tj + l15];      // B[k][j] = Z[k][j]
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc[u], 0, 0, 0);
                    }
                }
            }
        }
    };
    auto store_acc = [&](auto& acc, auto na_c) {             // epilogue, first half: the accumulator tiles into the epilogue view of the LDS
        constexpr int NA = decltype(na_c)::value;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            if (u < tcnt) {
                const int ti = tiA[u], tj = tjA[u];
                const int jc = 16 * tj + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + kq + 4 * r;      // C/D: col = lane&15, row = (lane>>4)+4r
                    if (i < NC && jc <= NC) so.A2[i][jc] = acc[u][r];
                }
            }
        }
    };
    // Pipeline: ONE barrier per batch.  Waves 0-1 build batch i + 1 (operand rows into the other panel, sparse scratch into the other
    // scratch buffer) while waves 2-3 run the sparse sums of batch i; every wave runs its tiles of batch i.  After the barrier that ends
    // batch i nobody reads buffer i & 1 any more: the producers refill it with batch i + 2.
    if (wave < 2) {
        // The per-observation quantities (N_o = G_o^T G_o, h_o = G_o^T r_o) are recomputed here from the frame inputs (one projection
        // per (feature, slot) lane), see k_feat_gram2.  Lane (f, c) = (tid >> 4, tid & 15); its raw inputs for the NEXT batch are
        // fetched into registers while this one is built.
        double in_uv[4], in_pf[3];
        unsigned long long in_mask = 0ULL;
        int in_anchor = 0;
        const int ft = tid;
        auto fetch = [&](int qb) {
            const int f = ft >> 4, c = ft & 15;
            in_mask = 0ULL; in_anchor = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) in_uv[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) in_pf[i] = 0.0;
            if (qb + f < q1) {
                const size_t oidx = (size_t)b * fv.fmax + sList[qb + f];
                in_mask = fv.obs_mask[oidx]; in_anchor = fv.anchor[oidx];
#pragma unroll
                for (int i = 0; i < 3; ++i) in_pf[i] = fv.pf[oidx * 3 + i];
                if (c < C && ((in_mask >> c) & 1ULL)) {
                    const double* z = fv.uv + (oidx * fv.cmax + c) * 4;
                    in_uv[0] = z[0]; in_uv[1] = z[1];
                    if (STEREO) { in_uv[2] = z[2]; in_uv[3] = z[3]; }
                }
            }
        };
        // sum over the 16 lanes of a feature, left in all of them (DPP row rotations, see k_feat_gram2)
        auto sum16 = [](double v) {
#ifdef GRAM_SHFL_SUM
            v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16);
#else
            v += row_ror_f64<8>(v); v += row_ror_f64<4>(v); v += row_ror_f64<2>(v); v += row_ror_f64<1>(v);
#endif
            return v;
        };
        // P2: operand rows into Zm[buf], sparse scratch into sp[buf]; the arithmetic of k_feat_gram2's P2, line for line
        auto do_p2 = [&](int qb, int buf) {
            const int nbf = min(GRAM_NB, q1 - qb);
            if (nbf < GRAM_NB) {                                   // short last batch: clear the unused stacked rows of this buffer
                for (int e = tid; e < (KR - 3 * nbf) * LDW; e += 128) (&sb.Zm[buf][3 * nbf][0])[e] = 0.0;
            }
            if (ft < nbf * 16) {
                const int f = ft >> 4, c = ft & 15;
                const int a = in_anchor;
                const double px = in_pf[0], py = in_pf[1], pz = in_pf[2];
                bool obs = c < C && ((in_mask >> c) & 1ULL);
                double N[9], h[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) N[i] = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) h[i] = 0.0;
                if (obs) {                                          // RemoveLostUpdate.cpp:435-506 for this (feature, clone)
                    double Gm[RPO][3], rs[RPO];
                    obs = feat_obs<STEREO>(sPose[c], sPose[c] + 9, in_uv, px, py, pz, op, Gm, rs);      // false: skipped by the NaN guard (:486)
                    if (obs) {
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
#pragma unroll
                            for (int m2 = 0; m2 < 3; ++m2) {
                                double sN = 0.0;
#pragma unroll
                                for (int q = 0; q < RPO; ++q) sN += Gm[q][m] * Gm[q][m2];
                                N[3 * m + m2] = sN;
                            }
                            double hh = 0.0;
#pragma unroll
                            for (int q = 0; q < RPO; ++q) hh += Gm[q][m] * rs[q];
                            h[m] = hh;
                        }
                    }
                }
                const double cn = (obs && c != a) ? 1.0 : 0.0, pl = (obs && !(op.selected_variant && c == a)) ? 1.0 : 0.0;
                // Ns = sum_o N_o (= Hf^T Hf), hs = sum_o h_o, Nsa = sum over the observations whose clone is not the anchor
                double Ns[9], hs[3], Nsa[9];
                const double n0 = sum16(N[0]), n1 = sum16(N[1]), n2 = sum16(N[2]), n4 = sum16(N[4]), n5 = sum16(N[5]), n8 = sum16(N[8]);
                Ns[0] = n0; Ns[1] = n1; Ns[2] = n2; Ns[3] = n1; Ns[4] = n4; Ns[5] = n5; Ns[6] = n2; Ns[7] = n5; Ns[8] = n8;
#ifdef GRAM_NSA_SUMS
                const double a0 = sum16(cn * N[0]), a1 = sum16(cn * N[1]), a2 = sum16(cn * N[2]), a4 = sum16(cn * N[4]), a5 = sum16(cn * N[5]),
                             a8 = sum16(cn * N[8]);
#else
                // the only observation with cn = 0 is the one AT the anchor slot: Nsa = Ns - N_anchor
                const int alane = (lane & 48) | (a & 15);
                const double a0 = n0 - __shfl(N[0], alane, WAVE), a1 = n1 - __shfl(N[1], alane, WAVE), a2 = n2 - __shfl(N[2], alane, WAVE),
                             a4 = n4 - __shfl(N[4], alane, WAVE), a5 = n5 - __shfl(N[5], alane, WAVE), a8 = n8 - __shfl(N[8], alane, WAVE);
#endif
                Nsa[0] = a0; Nsa[1] = a1; Nsa[2] = a2; Nsa[3] = a1; Nsa[4] = a4; Nsa[5] = a5; Nsa[6] = a2; Nsa[7] = a5; Nsa[8] = a8;
#pragma unroll
                for (int i = 0; i < 3; ++i) hs[i] = sum16(h[i]);
                if (c < C) {
                    double NX[9];
                    mulX(N, px, py, pz, NX);                            // N_o X
                    double Bt[9], Bp[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) { Bt[i] = cn * NX[i]; Bp[i] = -pl * N[i]; }
                    if (c == a) {                                       // theta_anchor block: -Nsa X   (the anchor's own cn is 0)
                        double T[9];
                        mulX(Nsa, px, py, pz, T);
#pragma unroll
                        for (int i = 0; i < 9; ++i) Bt[i] = -T[i];
                    }
                    // Z = D^-1/2 L^-1 B with Ns = L D L^T (3 x 3, SPD for a used feature): B^T Ns^-1 B = Z^T Z - ONE operand panel
                    const double s0 = Ns[0] > 0.0 ? gram_rsqrt(Ns[0]) : 0.0, r0 = s0 * s0;          // s_k = d_k^-1/2 (0: a pivot that is not positive)
                    const double l10 = Ns[1] * r0, l20 = Ns[2] * r0;
                    const double d1 = Ns[4] - l10 * Ns[1], s1 = d1 > 0.0 ? gram_rsqrt(d1) : 0.0, r1 = s1 * s1;
                    const double t21 = Ns[5] - l20 * Ns[1], l21 = t21 * r1;
                    const double d2 = (Ns[8] - l20 * Ns[2]) - l21 * t21, s2 = d2 > 0.0 ? gram_rsqrt(d2) : 0.0;
                    double (*Z)[LDW] = sb.Zm[buf];
                    if (!RED || c != cref) {                            // RED: the reference slot's six panel columns stay at their zeros
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            {
                                const double y0 = Bt[q], y1 = Bt[3 + q] - l10 * y0, y2 = (Bt[6 + q] - l20 * y0) - l21 * y1;
                                Z[3 * f + 0][6 * c + q] = s0 * y0; Z[3 * f + 1][6 * c + q] = s1 * y1; Z[3 * f + 2][6 * c + q] = s2 * y2;
                            }
                            {
                                const double y0 = Bp[q], y1 = Bp[3 + q] - l10 * y0, y2 = (Bp[6 + q] - l20 * y0) - l21 * y1;
                                Z[3 * f + 0][6 * c + 3 + q] = s0 * y0; Z[3 * f + 1][6 * c + 3 + q] = s1 * y1; Z[3 * f + 2][6 * c + 3 + q] = s2 * y2;
                            }
                        }
                    }
                    if (c == 0) {                                       // extra column: D^-1/2 L^-1 hs
                        const double y0 = hs[0], y1 = hs[1] - l10 * y0, y2 = (hs[2] - l20 * y0) - l21 * y1;
                        Z[3 * f + 0][NC] = s0 * y0; Z[3 * f + 1][NC] = s1 * y1; Z[3 * f + 2][NC] = s2 * y2;
                    }
                    // sparse scratch
                    double* sp = sb.sp[buf][f][c < CMAX ? c : 0];
                    double S1[9];
                    mulXt(NX, px, py, pz, S1);                          // X^T N X
#pragma unroll
                    for (int i = 0; i < 9; ++i) { sp[i] = cn * S1[i]; sp[9 + i] = cn * pl * NX[i]; }
                    sp[18] = cn * (pz * h[1] - py * h[2]);              // X^T h_o = h_o x p_f
                    sp[19] = cn * (px * h[2] - pz * h[0]);
                    sp[20] = cn * (py * h[0] - px * h[1]);
#pragma unroll
                    for (int i = 0; i < 9; ++i) sp[21 + i] = pl * N[i];                      // pl N_o
#pragma unroll
                    for (int i = 0; i < 3; ++i) sp[30 + i] = pl * h[i];                      // pl h_o
                    sp[33] = (obs || c == 0) ? (double)a : -1.0;          // key: the feature's anchor slot (slot 0 always carries it: the sparse lanes read it there)
                }
            }
        };
        double4_f acc[NPR > 0 ? NPR : 1];
#pragma unroll
        for (int u = 0; u < NPR; ++u) acc[u] = double4_f{ 0.0, 0.0, 0.0, 0.0 };
        fetch(q0);
        if (q0 < q1) { do_p2(q0, 0); fetch(q0 + GRAM_NB); }
        lds_barrier();
        int it = 0;
        for (int qb = q0; qb < q1; qb += GRAM_NB, ++it) {
            if (it == 3) dbg_stamp_at(36, 0);
            if (qb + GRAM_NB < q1) { do_p2(qb + GRAM_NB, (it + 1) & 1); fetch(qb + 2 * GRAM_NB); }
            if (it == 3) dbg_stamp_at(37, 0);
            do_p3a(acc, std::integral_constant<int, NPR>{}, qb, it & 1);
            if (it == 3) dbg_stamp_at(41, 0);
            lds_barrier();
            if (it == 3) dbg_stamp_at(42, 0);
        }
        store_acc(acc, std::integral_constant<int, NPR>{});
    } else {
        // The sparse sums by lane (slot uc, chunk uj of the slot's 33 values) with one accumulator triple per ANCHOR (k_feat_gram2's P3U):
        // a feature has one anchor - wave-uniform while the wave walks the batch - so a lane adds its three values into the triple of that
        // anchor behind a scalar selector.  Same additions in the same order as k_feat_gram2.
#if GRAM3_P3B_INDEXED
        // the triple of the feature's anchor addressed BY INDEX: the anchor is a scalar, so the three additions go to registers picked
        // through the index register - 3 additions per feature and lane instead of 33 multiply-adds of which 30 add zero.  The sum
        // x + s is what fma(1, x, s) gives and the skipped fma(0, x, s) leave s as it is: the same bits.
        // Anchors 0-7 sit in three 8-element vectors (indexable registers); anchors 8 and above (class 11 only) keep the selector form.
        typedef double dvec8 __attribute__((ext_vector_type(8)));
        constexpr int NHI = CMAX > 8 ? CMAX - 8 : 0;
        dvec8 sv0 = 0.0, sv1 = 0.0, sv2 = 0.0;
        double shi[NHI > 0 ? 3 * NHI : 1];
#pragma unroll
        for (int i = 0; i < 3 * NHI; ++i) shi[i] = 0.0;
#else
        double sacc[3 * CMAX];
#pragma unroll
        for (int i = 0; i < 3 * CMAX; ++i) sacc[i] = 0.0;
#endif
        auto do_p3b = [&](int qb, int buf) {
            const int nbf = min(GRAM_NB, q1 - qb);
            if (ulane) {
#if GRAM3_P3B_INDEXED
                // every LDS read of the batch first, then the additions (the key of a feature steers a scalar branch; measured: no
                // faster than reading feature by feature).  Features past a short batch's end are read (stale scratch, inside the
                // buffer) and not used.
                double xk[GRAM_NB], x0[GRAM_NB], x1[GRAM_NB], x2[GRAM_NB];
#pragma unroll
                for (int f = 0; f < GRAM_NB; ++f) {
                    const double* sp = sb.sp[buf][f][uc];
                    xk[f] = sb.sp[buf][f][0][33];                      // the feature's anchor slot (slot 0's key always carries it)
                    x0[f] = sp[3 * uj]; x1[f] = sp[3 * uj + 1]; x2[f] = sp[3 * uj + 2];      // zero for a slot that does not observe the feature
                }
#pragma unroll
                for (int f = 0; f < GRAM_NB; ++f) {
                    if (f < nbf) {
                        const int af = __builtin_amdgcn_readfirstlane((int)xk[f]);
                        if (NHI == 0 || af < 8) {                      // a scalar branch: af is wave-uniform
                            const int ai = af & 7;
                            sv0[ai] += x0[f]; sv1[ai] += x1[f]; sv2[ai] += x2[f];
                        } else {
#pragma unroll
                            for (int a2 = 0; a2 < NHI; ++a2) {
                                const double m = af == 8 + a2 ? 1.0 : 0.0;
                                shi[3 * a2] = fma(m, x0[f], shi[3 * a2]);
                                shi[3 * a2 + 1] = fma(m, x1[f], shi[3 * a2 + 1]);
                                shi[3 * a2 + 2] = fma(m, x2[f], shi[3 * a2 + 2]);
                            }
                        }
                    }
                }
#else
#pragma unroll
                for (int f = 0; f < GRAM_NB; ++f) {
                    if (f < nbf) {
                        const double* sp = sb.sp[buf][f][uc];
                        const int af = __builtin_amdgcn_readfirstlane((int)sb.sp[buf][f][0][33]);      // the feature's anchor slot (slot 0's key always carries it)
                        const double x0 = sp[3 * uj], x1 = sp[3 * uj + 1], x2 = sp[3 * uj + 2];       // zero for a slot that does not observe the feature
#pragma unroll
                        for (int a2 = 0; a2 < CMAX; ++a2) {             // wave-uniform selector per anchor (a scalar), three multiply-adds: no branch
                            const double m = af == a2 ? 1.0 : 0.0;
                            sacc[3 * a2] = fma(m, x0, sacc[3 * a2]);
                            sacc[3 * a2 + 1] = fma(m, x1, sacc[3 * a2 + 1]);
                            sacc[3 * a2 + 2] = fma(m, x2, sacc[3 * a2 + 2]);
                        }
                    }
                }
#endif
            }
        };
        double4_f acc[NCO > 0 ? NCO : 1];
#pragma unroll
        for (int u = 0; u < NCO; ++u) acc[u] = double4_f{ 0.0, 0.0, 0.0, 0.0 };
        lds_barrier();
        int it = 0;
        for (int qb = q0; qb < q1; qb += GRAM_NB, ++it) {
            if (it == 3) dbg_stamp_at(56, 128);
            do_p3a(acc, std::integral_constant<int, NCO>{}, qb, it & 1);
            if (it == 3) dbg_stamp_at(57, 128);
            do_p3b(qb, it & 1);
            if (it == 3) dbg_stamp_at(58, 128);
            lds_barrier();
            if (it == 3) dbg_stamp_at(59, 128);
        }
        store_acc(acc, std::integral_constant<int, NCO>{});
        if (ulane) {                                            // scratch order (S1, NX, X^T h, pl N, pl h) -> the epilogue's (S1, NX, pl N, X^T h, pl h)
#pragma unroll
            for (int a2 = 0; a2 < CMAX; ++a2)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int v = 3 * uj + i;
#if GRAM3_P3B_INDEXED
                    so.S[uc][a2][v < 18 ? v : (v < 21 ? v + 9 : (v < 30 ? v - 3 : v))] = a2 >= 8 ? shi[a2 >= 8 ? 3 * (a2 - 8) + i : 0] : (i == 0 ? sv0[a2 & 7] : (i == 1 ? sv1[a2 & 7] : sv2[a2 & 7]));
#else
                    so.S[uc][a2][v < 18 ? v : (v < 21 ? v + 9 : (v < 30 ? v - 3 : v))] = sacc[3 * a2 + i];
#endif
                }
        }
    }
    dbg_stamp(39);
    // ---- epilogue: assemble [A | b] of the chunk (k_feat_gram2's) ----------------------------------
    __syncthreads();
    double* out = Apart + ((size_t)bl * G + g) * rstride;      // [ncol][ncol+1] row-major, b in the last column
    // RED: blocks of the reference clone's row and column are neither assembled nor written (the diagonal blocks of the others still
    // sum over every anchor, the reference slot included); what is written goes to the same address as in the full form
    if (pairlane && pc < C && pa < C && pc != cref && pa != cref) {
        const int c = pc, c2 = pa;
        double blk[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) blk[i] = 0.0;
        double bb[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        if (c == c2) {
            for (int a = 0; a < C; ++a) {
                const double* S = so.S[c][a];          // obs at slot c, anchor a
                const double* Sa = so.S[a][c];         // obs at slot a, anchor c  -> (theta_c, theta_c) += S1
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int q2 = 0; q2 < 3; ++q2) {
                        blk[6 * q + q2] += S[3 * q + q2] + Sa[3 * q + q2];
                        blk[6 * q + 3 + q2] -= S[9 + 3 * q2 + q];            // (theta,p) = -NXs^T
                        blk[6 * (3 + q) + q2] -= S[9 + 3 * q + q2];          // (p,theta) = -NXs
                        blk[6 * (3 + q) + 3 + q2] += S[18 + 3 * q + q2];
                    }
#pragma unroll
                for (int q = 0; q < 3; ++q) { bb[q] += S[27 + q] - Sa[27 + q]; bb[3 + q] -= S[30 + q]; }
            }
        } else {
            const double* S = so.S[c][c2];             // obs at slot c, anchor c2
            const double* St = so.S[c2][c];            // obs at slot c2, anchor c
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int q2 = 0; q2 < 3; ++q2) {
                    blk[6 * q + q2] = -S[3 * q + q2] - St[3 * q + q2];       // S1 is symmetric
                    blk[6 * (3 + q) + q2] = S[9 + 3 * q + q2];               // (p_c, theta_a) = +NXs
                    blk[6 * q + 3 + q2] = St[9 + 3 * q2 + q];                // (theta_a, p_c') = +NXs^T
                }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2)
                {
                const int ri = 6 * c + q, rj = 6 * c2 + q2;
                // only tiles ti <= tj were accumulated: element (ri, rj) with ri/16 > rj/16 is read from its mirror
                const double a2 = (ri >> 4) <= (rj >> 4) ? so.A2[ri][rj] : so.A2[rj][ri];
                out[(size_t)ri * (ncol + 1) + rj] = blk[6 * q + q2] - a2;
            }
            if (c == c2) out[(size_t)(6 * c + q) * (ncol + 1) + ncol] = bb[q] - so.A2[6 * c + q][NC];
        }
    }
    if (tid == 0) chunk_used[bl * G + g] = max(0, q1 - q0);
    dbg_stamp(40);
}
