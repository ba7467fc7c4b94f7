// capi_delayed.hip — the C ABI's delayed initialisations: addVariableDelayed for one candidate, for a batch, and the landmark / GNSS forms from the nominal table.
// Host code only; the context and the shared helpers come from capi_internal.h.
#include "capi_internal.h"

using namespace capi;

namespace {

// ---- the round driver of the three batched forms below (kernels_delayed.hip) ----------------------------------------------------
// Round j = candidate j of every filter that has one: the form's front (rows, rotations, gate, verdict, append) + the batched
// k_ekf_core / k_downdate on the row counts the front wrote.  Nothing comes back to the host between the rounds.
//   work slab    Hu | resu | mu | the form's own (wk_own bytes from w_own)
//   result slab  added | new_idx | status [B] | chi2 | the form's own (out_own bytes from r_own) | the dx of every round (if asked for)
struct Rounds {
    int b0 = 0, nb = 0, R = 0, mu_cap = 0, nc_cap = 0, n_cap = 0, do_chi2 = 0;
    size_t in_bytes = 0, wk_own = 0, out_own = 0, ws_bytes = 0;         // ws_bytes: the large form's workspace (0: none)
    const bool* on = nullptr;                                           // [R] the rounds that are launched (null: every round)
    bool dx = false;                                                    // the caller wants every round's dx
    bool wait = false;                                                  // the fronts read the track store: behind the copy stream's last delta
    bool clear_all = false;                                             // every record in front of dx is cleared, not the status words alone
    bool table = false;                                                 // boxPlus of the round's dx on the nominal table behind the trailing update
    size_t RN = 0, cs = 0, hsu = 0, w_res = 0, w_mu = 0, w_own = 0, r_idx = 0, r_st = 0, r_chi = 0, r_own = 0, r_dx = 0, out_bytes = 0;      // rounds_begin's layout
    int mldu = 0;
};

// grows c->dl and its pinned mirror, sends the input slab pack(h) fills, clears the status words (or the records) and the frame's dx
template <class Pack>
int rounds_begin(ingvio_ctx* c, Rounds& rd, Pack pack)
{
    const size_t nb = rd.nb, B = c->d.batch;
    rd.RN = (size_t)rd.R * nb; rd.cs = rd.nc_cap; rd.mldu = (rd.mu_cap + 15) & ~15; rd.hsu = (size_t)rd.mldu * rd.nc_cap;
    rd.w_res = pad64(8 * nb * rd.hsu); rd.w_mu = rd.w_res + pad64(8 * nb * rd.mldu); rd.w_own = rd.w_mu + pad64(4 * nb);
    rd.r_idx = pad64(4 * rd.RN); rd.r_st = rd.r_idx + pad64(4 * rd.RN); rd.r_chi = rd.r_st + pad64(4 * B); rd.r_own = rd.r_chi + pad64(8 * rd.RN);
    rd.r_dx = rd.r_own + rd.out_own; rd.out_bytes = rd.r_dx + (rd.dx ? 8 * rd.RN * c->ldp : 0);
    auto& w = c->dl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, rd.in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.wk, &w.wk_cap, rd.w_own + rd.wk_own)) return rc;
    if (rd.ws_bytes) if (int rc = dev_grow(c, &w.ws, &w.ws_cap, rd.ws_bytes)) return rc;
    if (w.out_cap < rd.out_bytes && w.h_out) { hipHostFree(w.h_out); w.h_out = nullptr; }      // the pinned mirror grows with the device slab
    if (int rc = dev_grow(c, &w.out, &w.out_cap, rd.out_bytes)) return rc;
    if (!w.h_out) HIPCHK(c, hipHostMalloc((void**)&w.h_out, w.out_cap, hipHostMallocDefault));
    Uploader upl{ c };
    if (int rc = upl.begin(rd.in_bytes + 64)) return rc;
    char* h = upl.take<char>(rd.in_bytes);
    pack(h);
    upl.copy(w.in, h, rd.in_bytes);
    if (int rc = upl.end()) return rc;
    if (rd.wait && wait_inputs(c)) return INGVIO_E_HIP;
    if (rd.clear_all) HIPCHK(c, hipMemsetAsync(w.out, 0, rd.r_dx, c->st));                 // rounds nobody tries are never launched: their slots read "nothing"
    else HIPCHK(c, hipMemsetAsync((int*)(w.out + rd.r_st) + rd.b0, 0, sizeof(int) * nb, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_dx + (size_t)rd.b0 * c->ldp, 0, 8 * nb * c->ldp, c->st));      // entries past a filter's n stay zero
    return 0;
}

// the rounds, one fetch of the result slab into c->dl.h_out, one synchronisation; status [nb] (may be null) and *soft: the filters'
// decoded status words.  front(j, r0, F, E) launches round j's front(s) (r0 = j * nb: the round's records) and names E.colmap, E.nc, E.noise
template <class Front>
int rounds_run(ingvio_ctx* c, const Rounds& rd, int* status, int* soft, Front front)
{
    auto& w = c->dl;
    const int b0 = rd.b0, nb = rd.nb;
    int* d_st = (int*)(w.out + rd.r_st);
    const CovView cv = view(c);
    for (int j = 0; j < rd.R; ++j) {
        if (rd.on && !rd.on[j]) continue;
        const size_t r0 = (size_t)j * nb;
        DelayedFront F;
        memset(&F, 0, sizeof F);
        F.cv = cv; F.b0 = b0; F.nb = nb; F.cs = (int)rd.cs; F.do_chi2 = rd.do_chi2 ? 1 : 0;
        F.Hu = (double*)w.wk; F.resu = (double*)(w.wk + rd.w_res); F.mldu = rd.mldu; F.hsu = rd.hsu; F.mu = (int*)(w.wk + rd.w_mu);
        F.Y = c->d_Y + (size_t)b0 * c->ystride; F.ystride = (size_t)c->ystride; F.status = d_st;
        F.added = (int*)w.out + r0; F.new_idx = (int*)(w.out + rd.r_idx) + r0; F.chi2 = (double*)(w.out + rd.r_chi) + r0;
        EkfLaunch E;                                                                    // StateManager.cpp:623-624: ekfUpdate with the lower rows on the extended state
        memset(&E, 0, sizeof E);
        E.cv = cv; E.b0 = b0; E.nb = nb; E.H = F.Hu; E.res = F.resu; E.m = F.mu;
        E.r_kind = 0; E.mld = rd.mldu; E.hstride = (int)rd.hsu; E.cstride = (int)rd.cs; E.nstride = 0;
        E.Y = c->d_Y + (size_t)b0 * c->ystride; E.ystride = c->ystride; E.dx = c->d_dx; E.status = d_st; E.m_cap = rd.mu_cap; E.nc_cap = rd.nc_cap;
        if (int rc = front(j, r0, F, E)) return rc;
        { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->st); }
        { ProfScope p(c, PF_DOWNDATE); launch_downdate(E, rd.n_cap, c->st); }
        // boxPlus of the round's dx (zero where nothing was added) on the table, the new variable included (stream_filter.py:772-775)
        if (rd.table) launch_nominal_update(nom_table(c), c->d_dx, c->ldp, nullptr, b0, nb, c->st);
        if (rd.dx) HIPCHK(c, hipMemcpyAsync(w.out + rd.r_dx + 8 * r0 * c->ldp, c->d_dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToDevice, c->st));
    }
    HIPCHK(c, hipMemcpyAsync(w.h_out, w.out, rd.out_bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (int rc = last_launch(c)) return rc;
    const int* rs = (const int*)(w.h_out + rd.r_st) + b0;
    *soft = INGVIO_OK;
    for (int i = 0; i < nb; ++i) {
        const int st = soft_status(rs[i]);
        if (status) status[i] = st;
        if (st != INGVIO_OK) *soft = st;
    }
    return 0;
}

// the fetched common records of filter i's candidate in round j into entry o of the caller's arrays; true: the candidate was added
bool rounds_take(const ingvio_ctx* c, const Rounds& rd, int i, int j, size_t o, int* added, int* new_idx, double* chi2, double* dx)
{
    const char* h = c->dl.h_out;
    const size_t e = (size_t)j * rd.nb + i;
    added[o] = ((const int*)h)[e]; new_idx[o] = ((const int*)(h + rd.r_idx))[e];
    if (chi2) chi2[o] = ((const double*)(h + rd.r_chi))[e];
    if (dx && added[o]) memcpy(dx + o * c->ldp, (const double*)(h + rd.r_dx) + e * c->ldp, 8 * (size_t)c->ldp);
    return added[o] != 0;
}

}  // namespace

extern "C" {

static int stage_hnew(ingvio_ctx* c, const double* H_new, int ldn, int m, int s)
{
    if (!H_new || s < 1 || s > 6 || ldn < m || m > c->mld) return INGVIO_E_ARG;
    std::vector<double> Hn((size_t)c->mld * s, 0.0);
    for (int j = 0; j < s; ++j) memcpy(&Hn[(size_t)j * c->mld], H_new + (size_t)j * ldn, 8 * (size_t)m);
    if (up(c, c->d_hnew, Hn.data(), 8 * Hn.size())) return INGVIO_E_HIP;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return 0;
}

int ingvio_add_variable_delayed_invertible(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H_old, int ldh,
                                           const double* H_new, int ldn, int s, double noise, int* new_idx)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b, 1)) return INGVIO_E_ARG;
    if (c->h_n[b] + s > c->d.n_max) return INGVIO_E_CAPACITY;
    int nc = 0;
    const double var = noise * noise;
    std::vector<double> zero((size_t)(s > 0 ? s : 1), 0.0);
    int rc = stage_generic(c, b, vidx, vsize, k, H_old, ldh, s, zero.data(), &var, 0, &nc);
    if (rc) return rc;
    rc = stage_hnew(c, H_new, ldn, s, s);
    if (rc) return rc;
    if (launch_delayed_add(view(c), b, c->d_H + (size_t)b * c->hstride, c->d_hnew, c->d_colmap + (size_t)b * c->cstride, s, nc, c->mld,
                           var, c->d_Y + (size_t)b * c->ystride, c->st)) return INGVIO_E_CAPACITY;
    if (new_idx) *new_idx = c->h_n[b];
    c->h_n[b] += s;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return last_launch(c);
}

int ingvio_add_variable_delayed(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H_old, int ldh,
                                const double* H_new, int ldn, int m, int s, const double* res, double noise, double chi2_mult,
                                int do_chi2, double chi2_check, double* dx_out, int* added, int* new_idx, double* chi2_out)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b, 1) || !added) return INGVIO_E_ARG;
    *added = 0;
    if (m <= s) return INGVIO_OK;                                                  // StateManager.cpp:571-575
    if (c->h_n[b] + s > c->d.n_max) return INGVIO_E_CAPACITY;
    if (c->delayed_form && vidx && vsize && k >= 1) {
        // ingvio_set_delayed_form: a candidate beyond the gate's bound (mode 2: every candidate) runs as a one-filter call of the batch path
        size_t ncq = 0;
        for (int t = 0; t < k; ++t) ncq += vsize[t] > 0 ? vsize[t] : 0;
        const size_t muq = (size_t)(m - s);
        if (c->delayed_form == 2 || 8 * (ncq * muq + (muq + 1) * (muq + 1)) > 150 * 1024) {
            const ingvio_delayed_cand q{ vidx, vsize, k, H_old, ldh, H_new, ldn, res, m, s, chi2_check };
            const ingvio_delayed_block blk{ 1, &q };
            std::vector<double> dxb(dx_out ? (size_t)c->ldp : 0);
            int idx = -1, st = INGVIO_OK;
            double chi2 = 0.0;
            const int rc = ingvio_add_variable_delayed_batch(c, b, 1, &blk, noise, chi2_mult, do_chi2, 1, added, &idx, &chi2, dx_out ? dxb.data() : nullptr, &st);
            if (chi2_out && (rc == INGVIO_OK || rc == INGVIO_NEG_DIAG || rc == INGVIO_E_NOT_PD)) *chi2_out = chi2;
            if (*added) {
                if (new_idx) *new_idx = idx;
                if (dx_out) memcpy(dx_out, dxb.data(), 8 * (size_t)c->h_n[b]);
            }
            return rc;
        }
    }
    int nc = 0;
    const double var = noise * noise;
    int rc = stage_generic(c, b, vidx, vsize, k, H_old, ldh, m, res, &var, 0, &nc);
    if (rc) return rc;
    rc = stage_hnew(c, H_new, ldn, m, s);
    if (rc) return rc;
    if (!ekf_core_fits(m - s, nc)) return INGVIO_E_CAPACITY;     // the trailing EKF update must fit before the state is touched
    double* dH = c->d_H + (size_t)b * c->hstride;
    double* dres = c->d_res + (size_t)b * c->mld;
    const int* dcm = c->d_colmap + (size_t)b * c->cstride;
    if (launch_delayed_qr(dH, dres, c->d_hnew, m, s, nc, c->mld, c->st)) return INGVIO_E_CAPACITY;      // :577-589
    const int mu = m - s;
    if ((size_t)8 * ((size_t)nc * mu + (size_t)(mu + 1) * (mu + 1)) > 150 * 1024) return INGVIO_E_CAPACITY;
    launch_gamma(view(c), b, dH + s, dres + s, dcm, mu, nc, c->d_noise1, 0, c->mld, c->d_gamma + (size_t)b * c->d.f_max, c->st);   // :601-608
    double chi2 = 0.0;
    if (down_sync(c, &chi2, c->d_gamma + (size_t)b * c->d.f_max, 8)) return INGVIO_E_HIP;
    if (chi2_out) *chi2_out = chi2;
    if (chi2 > chi2_mult * chi2_check && do_chi2) return last_launch(c);           // :614-618
    if (launch_delayed_add(view(c), b, dH, c->d_hnew, dcm, s, nc, c->mld, var, c->d_Y + (size_t)b * c->ystride, c->st))
        return INGVIO_E_CAPACITY;
    if (new_idx) *new_idx = c->h_n[b];
    c->h_n[b] += s;
    *added = 1;
    // :623-624 ekfUpdate with the lower rows on the extended state
    int zero = 0;
    if (up(c, c->d_status + b, &zero, sizeof(int)) || up(c, c->d_m + b, &mu, sizeof(int))) return INGVIO_E_HIP;
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = view(c); E.b0 = b; E.nb = 1; E.H = dH + s; E.res = dres + s; E.colmap = dcm; E.m = c->d_m + b; E.nc = c->d_nc + b;
    E.noise = c->d_noise1; E.r_kind = 0; E.mld = c->mld; E.hstride = c->hstride; E.cstride = c->cstride;
    E.nstride = c->mld * c->mld; E.Y = c->d_Y + (size_t)b * c->ystride; E.ystride = c->ystride; E.dx = c->d_dx;
    E.status = c->d_status; E.m_cap = mu; E.nc_cap = nc;
    launch_ekf_core(E, c->st);
    launch_downdate(E, c->h_n[b], c->st);
    int status = 0;
    if (dx_out && down_sync(c, dx_out, c->d_dx + (size_t)b * c->ldp, 8 * (size_t)c->h_n[b])) return INGVIO_E_HIP;
    if (down_sync(c, &status, c->d_status + b, sizeof(int))) return INGVIO_E_HIP;
    rc = last_launch(c);
    if (rc) return rc;
    return soft_status(status);
}

// ---- addVariableDelayed for filters [b0, b0 + nb), several candidates per filter ----------------------------------------------------
int ingvio_add_variable_delayed_batch(ingvio_ctx* c, int b0, int nb, const ingvio_delayed_block* blocks, double noise, double chi2_mult,
                                      int do_chi2, int cand_cap, int* added, int* new_idx, double* chi2, double* dx, int* status)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !blocks || cand_cap < 1 || !added || !new_idx) return INGVIO_E_ARG;
    if (c->nom.pending) { c->err = "ingvio_add_variable_delayed_batch: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_add_variable_delayed_batch")) return INGVIO_E_ARG;
    // ---- everything that can be wrong, before anything changes ----
    int R = 0, mu_cap = 0, nc_cap = 0, n_cap = 0, ldw = 0, ncw = 0;
    size_t lds = 0, lds_large = 0, dtot = 0;
    const int form = c->delayed_form;             // ingvio_set_delayed_form
    for (int i = 0; i < nb; ++i) if (blocks[i].n_cand > R) R = blocks[i].n_cand;      // rounds (a wrong n_cand is refused below)
    if (R > cand_cap) return INGVIO_E_ARG;
    const size_t RN = (size_t)R * nb;
    std::vector<int> ncs(RN, 0);                  // [round][filter]: columns of the candidate, 0 = none / skipped
    std::vector<char> large(RN, 0);               // [round][filter]: the candidate takes the large form of the front
    std::vector<int> n_lds(R > 0 ? R : 1, 0), n_large(R > 0 ? R : 1, 0);      // per round: candidates of either form
    std::vector<size_t> offs(RN, 0);
    for (int i = 0; i < nb; ++i) {
        const ingvio_delayed_block& blk = blocks[i];
        const int b = b0 + i;
        if (blk.n_cand < 0 || (blk.n_cand > 0 && !blk.cand)) return INGVIO_E_ARG;
        int grow = 0;
        for (int j = 0; j < blk.n_cand; ++j) {
            const ingvio_delayed_cand& q = blk.cand[j];
            if (q.s < 1 || q.s > 6 || q.m < 0) return INGVIO_E_ARG;
            if (q.m <= q.s) continue;                                                   // StateManager.cpp:574-578: skipped
            if (!q.vidx || !q.vsize || !q.H_old || !q.H_new || !q.res || q.k < 1 || q.ldh < q.m || q.ldn < q.m) return INGVIO_E_ARG;
            int nc = 0;
            for (int t = 0; t < q.k; ++t) {
                if (q.vidx[t] < 0 || q.vsize[t] < 0 || q.vidx[t] + q.vsize[t] > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;      // checkSubOrder
                nc += q.vsize[t];
            }
            if (nc < 1) return INGVIO_E_ARG;
            const int mu = q.m - q.s;
            if (q.m > c->mld || nc > c->nc_cap || !ekf_core_fits(mu, nc)) return INGVIO_E_CAPACITY;
            if (!form && (size_t)8 * ((size_t)nc * mu + (size_t)(mu + 1) * (mu + 1)) > 150 * 1024) return INGVIO_E_CAPACITY;      // the single-filter gate's bound
            const size_t l = delayed_front_lds(q.m, q.s, nc);
            if (form == 2 || (form == 1 && l > 160 * 1024)) {                           // the large form: rows and T in the workspace
                const size_t ll = delayed_front_large_lds(q.m, q.s, nc);
                if (ll > 160 * 1024) return INGVIO_E_CAPACITY;
                if (ll > lds_large) lds_large = ll;
                if (q.m > ldw) ldw = q.m;
                if (nc > ncw) ncw = nc;
                large[(size_t)j * nb + i] = 1; ++n_large[j];
            } else {
                if (l > 160 * 1024) return INGVIO_E_CAPACITY;                           // the front's own: rows and T stay in LDS
                if (l > lds) lds = l;
                ++n_lds[j];
            }
            if (mu > mu_cap) mu_cap = mu;
            if (nc > nc_cap) nc_cap = nc;
            grow += q.s;
            ncs[(size_t)j * nb + i] = nc;
            offs[(size_t)j * nb + i] = dtot;
            dtot += (size_t)q.m * (nc + q.s + 1);
        }
        if (c->h_n[b] + grow > c->d.n_max) return INGVIO_E_CAPACITY;                    // every candidate of the filter may be added
        if (c->h_n[b] + grow > n_cap) n_cap = c->h_n[b] + grow;
    }
    const size_t CC = (size_t)nb * cand_cap;
    for (size_t e = 0; e < CC; ++e) { added[e] = 0; new_idx[e] = -1; if (chi2) chi2[e] = 0.0; }
    if (dx) memset(dx, 0, 8 * CC * c->ldp);
    if (status) for (int i = 0; i < nb; ++i) status[i] = INGVIO_OK;
    if (R == 0 || nc_cap == 0) return INGVIO_OK;                                        // nothing to try anywhere
    // ---- one slab up: [m | s | nc | colmap | offsets | thresholds | var | rows] ----
    const size_t cs = nc_cap;
    // (rounds that mix the two forms: the LDS launch's row counts with the large form's candidates struck, the large launch's selection)
    const size_t o_m = 0, o_s = o_m + pad64(4 * RN), o_nc = o_s + pad64(4 * RN), o_cm = o_nc + pad64(4 * RN), o_off = o_cm + pad64(4 * RN * cs),
                 o_thr = o_off + pad64(8 * RN), o_var = o_thr + pad64(8 * RN), o_ml = o_var + 64, o_sel = o_ml + (ldw ? pad64(4 * RN) : 0),
                 o_d = o_sel + (ldw ? pad64(4 * RN) : 0), in_bytes = o_d + pad64(8 * dtot);
    ldw = (ldw + 1) & ~1;
    const size_t ws_stride = (size_t)(2 * ncw + 1) * ldw;
    Rounds rd;
    rd.b0 = b0; rd.nb = nb; rd.R = R; rd.in_bytes = in_bytes; rd.ws_bytes = ldw ? 8 * (size_t)nb * ws_stride : 0;
    rd.mu_cap = mu_cap; rd.nc_cap = nc_cap; rd.n_cap = n_cap; rd.do_chi2 = do_chi2; rd.dx = dx != nullptr;
    if (int rc = rounds_begin(c, rd, [&](char* h) {
            memset(h, 0, o_d);
            int *hm = (int*)(h + o_m), *hs = (int*)(h + o_s), *hnc = (int*)(h + o_nc), *hcm = (int*)(h + o_cm);
            size_t* hoff = (size_t*)(h + o_off);
            double *hthr = (double*)(h + o_thr), *hd = (double*)(h + o_d);
            *(double*)(h + o_var) = noise * noise;
            int *hml = (int*)(h + o_ml), *hsel = (int*)(h + o_sel);
            parallel_for(nb, [=, &ncs, &offs, &large](int i) {
                const ingvio_delayed_block& blk = blocks[i];
                for (int j = 0; j < blk.n_cand; ++j) {
                    const size_t e = (size_t)j * nb + i;
                    const int nc = ncs[e];
                    if (!nc) continue;
                    const ingvio_delayed_cand& q = blk.cand[j];
                    hm[e] = q.m; hs[e] = q.s; hnc[e] = nc; hoff[e] = offs[e]; hthr[e] = chi2_mult * q.chi2_check;
                    if (ldw) { hml[e] = large[e] ? 0 : q.m; hsel[e] = large[e]; }
                    int* cm = hcm + e * cs;
                    int wr = 0;
                    for (int t = 0; t < q.k; ++t) for (int u = 0; u < q.vsize[t]; ++u) cm[wr++] = q.vidx[t] + u;
                    double* d = hd + offs[e];
                    for (int cc = 0; cc < nc; ++cc) memcpy(d + (size_t)cc * q.m, q.H_old + (size_t)cc * q.ldh, 8 * (size_t)q.m);
                    d += (size_t)nc * q.m;
                    for (int cc = 0; cc < q.s; ++cc) memcpy(d + (size_t)cc * q.m, q.H_new + (size_t)cc * q.ldn, 8 * (size_t)q.m);
                    memcpy(d + (size_t)q.s * q.m, q.res, 8 * (size_t)q.m);
                }
            });
        })) return rc;
    auto& w = c->dl;
    int soft = INGVIO_OK;
    if (int rc = rounds_run(c, rd, status, &soft, [&](int j, size_t r0, DelayedFront& F, EkfLaunch& E) {
            F.dbuf = (const double*)(w.in + o_d); F.doff = (const size_t*)(w.in + o_off) + r0;
            F.m = (const int*)(w.in + o_m) + r0; F.s = (const int*)(w.in + o_s) + r0; F.nc = (const int*)(w.in + o_nc) + r0;
            F.colmap = (const int*)(w.in + o_cm) + r0 * cs; F.thr = (const double*)(w.in + o_thr) + r0; F.var = noise * noise;
            // one launch per form: the LDS form first (it writes "nothing tried" for the filters it does not take), then the large
            // form, which skips every filter that is not its own
            if (!n_large[j]) { if (launch_delayed_front(F, lds, c->st)) return INGVIO_E_CAPACITY; }
            else {
                const int* m_all = F.m;
                if (n_lds[j]) { F.m = (const int*)(w.in + o_ml) + r0; if (launch_delayed_front(F, lds, c->st)) return INGVIO_E_CAPACITY; F.m = m_all; }
                DelayedLarge G{ (double*)w.ws, ws_stride, ldw, n_lds[j] ? (const int*)(w.in + o_sel) + r0 : nullptr };
                if (launch_delayed_front_large(F, G, lds_large, c->st)) return INGVIO_E_CAPACITY;
            }
            E.colmap = F.colmap; E.nc = F.nc; E.noise = (const double*)(w.in + o_var);
            return INGVIO_OK;
        })) return rc;
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < blocks[i].n_cand; ++j)
            if (rounds_take(c, rd, i, j, (size_t)i * cand_cap + j, added, new_idx, chi2, dx)) c->h_n[b0 + i] += blocks[i].cand[j].s;
    return soft;
}

// ---- LandmarkUpdate::initNewLandmark{Mono,Stereo} (LandmarkUpdate.cpp:363-424, :892-956) from the track store and the nominal table ----
// The rounds of ingvio_add_variable_delayed_batch with the rows formed by the front itself (k_delayed_front<true>) at the clone poses
// the table holds when the round starts, the accepted landmark entered into the table by the front, and boxPlus of the round's dx on
// the table behind the trailing update: candidate j + 1 is linearised where the reference linearises it.  Validation on the host
// mirror only, no decision between the rounds, one synchronisation.
struct LmInitPlan {
    int R = 0, mu_cap = 0, nc_cap = 0, n_cap = 0, per = 2;
    size_t lds = 0;
    bool large = false;                 // ingvio_set_delayed_form: the call's fronts take the large form (chosen at the worst-case m of the widest window)
    size_t lds_large = 0;
    int ldw = 0;
    std::vector<int> slots;             // [round][filter] reserved table slot (-1: no candidate)
    std::vector<unsigned long long> dropm;
};

// rows_only: the parity hook - it appends nothing, so neither a free table slot nor room in the state is asked for
static int lm_init_validate(ingvio_ctx* c, const char* who, int b0, int nb, const ingvio_lm_init_block* blocks, const ingvio_msckf_opts* o, int cand_cap,
                            LmInitPlan& pl, bool rows_only = false)
{
    auto& m = c->nom;
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !blocks || !o || cand_cap < 1) return INGVIO_E_ARG;
    if (!m.vmax) { c->err = std::string(who) + " without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (!c->trk.t_max) { c->err = std::string(who) + " without ingvio_tracks_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = std::string(who) + ": a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    if (!(o->noise > 0.0) || !o->chi2_table || o->chi2_len < 1) return INGVIO_E_ARG;
    const int cm = c->d.c_max, per = o->stereo ? 4 : 2;
    pl.per = per;
    for (int i = 0; i < nb; ++i) if (blocks[i].n_cand > pl.R) pl.R = blocks[i].n_cand;
    if (pl.R > cand_cap) return INGVIO_E_ARG;
    pl.slots.assign((size_t)pl.R * nb, -1);
    pl.dropm.assign((size_t)nb, 0ULL);
    int cap_err = 0;
    for (int i = 0; i < nb; ++i) {
        const ingvio_lm_init_block& blk = blocks[i];
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        const int cw = I[NOM_N_CLONES];
        if (blk.n_cand < 0 || (blk.n_cand > 0 && !blk.cand) || blk.n_drop < 0 || (blk.n_drop > 0 && !blk.drop_cols)) return INGVIO_E_ARG;
        for (int q = 0; q < blk.n_drop; ++q) {
            if (blk.drop_cols[q] < 0 || blk.drop_cols[q] >= cm || (q && blk.drop_cols[q] <= blk.drop_cols[q - 1])) {
                c->err = std::string(who) + ": drop_cols is not ascending or names a column outside c_max"; return INGVIO_E_ARG;
            }
            pl.dropm[i] |= 1ULL << blk.drop_cols[q];
        }
        if (cw + blk.n_drop > cm) { c->err = std::string(who) + ": the window and the pending drops exceed c_max"; return INGVIO_E_ARG; }
        if (blk.n_cand == 0) continue;
        for (int j = 0; j < blk.n_cand; ++j) {
            const ingvio_lm_init_cand& q = blk.cand[j];
            if (q.track < 0 || q.track >= c->trk.t_max) { c->err = std::string(who) + ": a track lies outside the store"; return INGVIO_E_ARG; }
            if (q.anchor < 0 || q.anchor >= cw) { c->err = std::string(who) + ": an anchor lies outside the window"; return INGVIO_E_ARG; }
        }
        if (o->chi2_len < per * cw + 1) { c->err = std::string(who) + ": chi2_table is shorter than the widest candidate needs"; return INGVIO_E_ARG; }
        for (int q = 0; q < cw; ++q) {
            const int ix = var[4 * I[NOM_CLONES + q] + 1];
            if (ix < 0 || ix + 6 > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;
        }
        // capacity (reported after every argument of the call has been looked at)
        int got = 0;
        for (int v = 0; v < m.vmax && got < blk.n_cand; ++v) if (var[4 * v] == NOM_KIND_NONE) pl.slots[(size_t)(got++) * nb + i] = v;
        const int mw = per * cw, nc = 6 * cw, mu = mw - 3;
        if (!rows_only && (got < blk.n_cand || c->h_n[b] + 3 * blk.n_cand > c->d.n_max)) { cap_err = 1; continue; }
        if (mw > c->mld || nc > c->nc_cap) { cap_err = 1; continue; }
        if (mu > 0) {
            const size_t l = delayed_front_lds(mw, 3, nc);
            const int form = c->delayed_form;
            if ((!form && l > 160 * 1024) || !ekf_core_fits(mu, nc)) { cap_err = 1; continue; }
            if (!form && (size_t)8 * ((size_t)nc * mu + (size_t)(mu + 1) * (mu + 1)) > 150 * 1024) { cap_err = 1; continue; }      // as ingvio_add_variable_delayed_batch
            if (form) {
                const size_t ll = delayed_front_large_lds(mw, 3, nc);
                if (ll > 160 * 1024) { cap_err = 1; continue; }
                if (ll > pl.lds_large) pl.lds_large = ll;
                if (mw > pl.ldw) pl.ldw = mw;
                if (form == 2 || l > 160 * 1024) pl.large = true;
            }
            if (l <= 160 * 1024 && l > pl.lds) pl.lds = l;
            if (mu > pl.mu_cap) pl.mu_cap = mu;
        }
        if (nc > pl.nc_cap) pl.nc_cap = nc;
        if (c->h_n[b] + 3 * blk.n_cand > pl.n_cap) pl.n_cap = c->h_n[b] + 3 * blk.n_cand;
    }
    return cap_err ? INGVIO_E_CAPACITY : INGVIO_OK;
}

static void lm_init_rows_common(ingvio_ctx* c, const ingvio_msckf_opts* o, double chi2_mult, DelayedRows& Rw)
{
    Rw.nt = nom_table(c);
    Rw.ts = track_store(c);
    Rw.chi2_mult = chi2_mult; Rw.stereo = o->stereo ? 1 : 0;
    memcpy(Rw.R_lr, o->R_cl2cr, 72); memcpy(Rw.t_lr, o->t_cl2cr, 24);
}

int ingvio_landmark_init_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_lm_init_block* blocks, const ingvio_msckf_opts* o, double chi2_mult,
                                 int do_chi2, int cand_cap, int* added, int* new_idx, int* slot, double* chi2, double* dx, int* status)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    if (!added || !new_idx || !slot) return INGVIO_E_ARG;
    LmInitPlan pl;
    if (int rc = lm_init_validate(c, "ingvio_landmark_init_nominal", b0, nb, blocks, o, cand_cap, pl)) return rc;
    const int R = pl.R;
    const size_t RN = (size_t)R * nb, CC = (size_t)nb * cand_cap;
    for (size_t e = 0; e < CC; ++e) { added[e] = 0; new_idx[e] = -1; slot[e] = -1; if (chi2) chi2[e] = 0.0; }
    if (dx) memset(dx, 0, 8 * CC * c->ldp);
    if (status) for (int i = 0; i < nb; ++i) status[i] = INGVIO_OK;
    if (R == 0 || pl.mu_cap == 0) return INGVIO_OK;                                    // nothing to try anywhere (or no window wider than m <= 3)
    // ---- one slab up: 40 bytes per candidate, the pending drops, the chi2 table ----
    const size_t ntab = (size_t)pl.mu_cap + 4;                                          // chi2_table[0 .. widest m]
    const size_t o_tr = 0, o_an = o_tr + pad64(4 * RN), o_sl = o_an + pad64(4 * RN), o_pf = o_sl + pad64(4 * RN), o_dm = o_pf + pad64(24 * RN),
                 o_tab = o_dm + pad64(8 * (size_t)nb), o_var = o_tab + pad64(8 * ntab), in_bytes = o_var + 64;
    const int ldw = (pl.ldw + 1) & ~1;
    const size_t ws_stride = (size_t)(2 * pl.nc_cap + 1) * ldw;
    const double var = o->noise * o->noise;
    Rounds rd;
    rd.b0 = b0; rd.nb = nb; rd.R = R; rd.in_bytes = in_bytes; rd.ws_bytes = pl.large ? 8 * (size_t)nb * ws_stride : 0;
    rd.wk_own = pad64(4 * (size_t)nb) + pad64(4 * (size_t)nb * pl.nc_cap);            // nc_out | colmap_out
    rd.out_own = pad64(4 * RN);                                                         // slot_out
    rd.mu_cap = pl.mu_cap; rd.nc_cap = pl.nc_cap; rd.n_cap = pl.n_cap; rd.do_chi2 = do_chi2; rd.dx = dx != nullptr;
    rd.wait = true;                                                                     // the store's last delta may have travelled on the copy stream
    rd.table = true;
    if (int rc = rounds_begin(c, rd, [&](char* h) {
            memset(h, 0, in_bytes);
            int *htr = (int*)(h + o_tr), *han = (int*)(h + o_an), *hsl = (int*)(h + o_sl);
            double* hpf = (double*)(h + o_pf);
            for (size_t e = 0; e < RN; ++e) htr[e] = -1;
            for (int i = 0; i < nb; ++i)
                for (int j = 0; j < blocks[i].n_cand; ++j) {
                    const size_t e = (size_t)j * nb + i;
                    const ingvio_lm_init_cand& q = blocks[i].cand[j];
                    htr[e] = q.track; han[e] = q.anchor; hsl[e] = pl.slots[e];
                    memcpy(hpf + 3 * e, q.pf, 24);
                }
            memcpy(h + o_dm, pl.dropm.data(), 8 * (size_t)nb);
            memcpy(h + o_tab, o->chi2_table, 8 * ntab);
            *(double*)(h + o_var) = var;
        })) return rc;
    auto& w = c->dl;
    DelayedRows Rw;
    memset(&Rw, 0, sizeof Rw);
    lm_init_rows_common(c, o, chi2_mult, Rw);
    Rw.dropm = (const unsigned long long*)(w.in + o_dm); Rw.chi2 = (const double*)(w.in + o_tab);
    Rw.nc_out = (int*)(w.wk + rd.w_own); Rw.colmap_out = (int*)(w.wk + rd.w_own + pad64(4 * (size_t)nb));
    int soft = INGVIO_OK;
    if (int rc = rounds_run(c, rd, status, &soft, [&](int, size_t r0, DelayedFront& F, EkfLaunch& E) {
            F.var = var;
            Rw.track = (const int*)(w.in + o_tr) + r0; Rw.anchor = (const int*)(w.in + o_an) + r0; Rw.slot = (const int*)(w.in + o_sl) + r0;
            Rw.pf = (const double*)(w.in + o_pf) + 3 * r0; Rw.slot_out = (int*)(w.out + rd.r_own) + r0;
            if (pl.large) {
                const DelayedLarge G{ (double*)w.ws, ws_stride, ldw, nullptr };
                if (launch_delayed_front_rows_large(F, Rw, G, pl.lds_large, c->st)) return INGVIO_E_CAPACITY;
            } else if (launch_delayed_front_rows(F, Rw, pl.lds, c->st)) return INGVIO_E_CAPACITY;
            E.colmap = Rw.colmap_out; E.nc = Rw.nc_out; E.noise = (const double*)(w.in + o_var);
            return INGVIO_OK;
        })) return rc;
    const int* rl = (const int*)(w.h_out + rd.r_own);
    for (int i = 0; i < nb; ++i) {
        int* I = &c->nom.h_ih[(size_t)(b0 + i) * c->nom.ir];
        for (int j = 0; j < blocks[i].n_cand; ++j) {
            const size_t e = (size_t)j * nb + i, oo = (size_t)i * cand_cap + j;
            if (!rounds_take(c, rd, i, j, oo, added, new_idx, chi2, dx)) continue;      // (slot stays -1)
            slot[oo] = rl[e];
            c->h_n[b0 + i] += 3;                                                        // the mirror follows the front's record
            int* v = I + NOM_IH + 4 * rl[e];
            v[0] = NOM_KIND_LM; v[1] = new_idx[oo]; v[2] = I[NOM_CLONES + blocks[i].cand[j].anchor]; v[3] = 0;
            if (rl[e] >= I[NOM_N_VAR]) I[NOM_N_VAR] = rl[e] + 1;
        }
    }
    if (nom_mark(c)) return INGVIO_E_HIP;
    return soft;
}

// parity hook (tests): the row stage of ingvio_landmark_init_nominal alone, for one filter and one candidate; changes nothing
int ingvio_debug_landmark_init_rows(ingvio_ctx* c, int b, const ingvio_lm_init_cand* cand, const ingvio_msckf_opts* o, int n_drop, const int* drop_cols,
                                    double* H_old, double* H_new, double* res, int* m_out)
{
    ENTER(c);
    if (!c || !cand || !H_old || !H_new || !res || !m_out) return INGVIO_E_ARG;
    ingvio_lm_init_block blk{ 1, cand, n_drop, drop_cols };
    LmInitPlan pl;
    if (int rc = lm_init_validate(c, "ingvio_debug_landmark_init_rows", b, 1, &blk, o, 1, pl, true)) return rc;
    const int cw = c->nom.h_ih[(size_t)b * c->nom.ir + NOM_N_CLONES], mw = pl.per * cw, nc = 6 * cw;
    const size_t rows = (size_t)mw * (nc + 4), o_pf = 64, o_dm = 128, in_bytes = 192, out_bytes = pad64(8 * rows) + 64;
    auto& w = c->dl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.wk, &w.wk_cap, out_bytes)) return rc;
    char h[192];
    memset(h, 0, sizeof h);
    ((int*)h)[0] = cand->track; ((int*)h)[1] = cand->anchor;
    memcpy(h + o_pf, cand->pf, 24); memcpy(h + o_dm, pl.dropm.data(), 8);
    if (up(c, w.in, h, in_bytes)) return INGVIO_E_HIP;
    if (wait_inputs(c)) return INGVIO_E_HIP;
    DelayedRows Rw;
    memset(&Rw, 0, sizeof Rw);
    lm_init_rows_common(c, o, 1.0, Rw);
    Rw.track = (const int*)w.in; Rw.anchor = (const int*)w.in + 1; Rw.pf = (const double*)(w.in + o_pf); Rw.dropm = (const unsigned long long*)(w.in + o_dm);
    int* d_m = (int*)(w.wk + pad64(8 * rows));
    const size_t lds = delayed_front_lds(mw > 0 ? mw : 1, 3, nc);
    const bool big = c->delayed_form && lds > 160 * 1024;      // rows formed in global memory: [H_old | res | H_new]
    if (big) launch_delayed_rows_debug_large(Rw, b, (double*)w.wk, d_m, c->st);
    else if (launch_delayed_rows_debug(Rw, b, (double*)w.wk, d_m, lds, c->st)) return INGVIO_E_CAPACITY;
    std::vector<double> out(rows);
    int m = 0;
    HIPCHK(c, hipMemcpyAsync(out.data(), w.wk, 8 * rows, hipMemcpyDeviceToHost, c->st));
    if (down_sync(c, &m, d_m, sizeof(int))) return INGVIO_E_HIP;
    if (int rc = last_launch(c)) return rc;
    *m_out = m;
    memcpy(H_old, out.data(), 8 * (size_t)m * nc);
    memcpy(H_new, out.data() + (size_t)m * (big ? nc + 1 : nc), 8 * (size_t)m * 3);
    memcpy(res, out.data() + (size_t)m * (big ? nc : nc + 3), 8 * (size_t)m);
    return INGVIO_OK;
}

// ---- GnssUpdate::addNewTrackedSys (GnssUpdate.cpp:295-470) from the nominal table: the twin of ingvio_landmark_init_nominal ----
// k_gnss_front<true> once at the receiver the SPP fix overrides, R_w2ecef once, then one round per candidate scalar (FS, clock GPS, GLO,
// GAL, BDS): k_delayed_front<DL_GNSS> (rows, noise, rotations, gate, verdict, append, table record), the trailing update, boxPlus on the
// table.  Validation on the host mirror only, no decision between the rounds, one synchronisation.
struct GnssInitPlan {
    int smax = 1, n_cap = 0;
    bool any = false;
    std::vector<int> cand, slots;       // [round][filter]: tried / reserved table slot
    bool round[INGVIO_GNSS_INIT_CAND] = { false, false, false, false, false };
};

// rows_only: the parity hook - it appends nothing, so neither a free table slot nor room in the state is asked for, and the candidate
// it names need not be one the call would try
static int gnss_init_validate(ingvio_ctx* c, const char* who, int b0, int nb, const ingvio_gnss_init_block* blocks, const double* chi2_table, int chi2_len,
                              GnssInitPlan& pl, bool rows_only = false)
{
    auto& m = c->nom;
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !blocks) return INGVIO_E_ARG;
    if (!m.vmax) { c->err = std::string(who) + " without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = std::string(who) + ": a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    if ((c->gn.frame_nom && c->gn.staged) || (c->lm.nominal && c->lm.staged)) {
        c->err = std::string(who) + ": an in-frame GNSS epoch or landmark update staged from the device nominal state has not run yet"; return INGVIO_E_ARG;
    }
    const int NC = INGVIO_GNSS_INIT_CAND;
    pl.cand.assign((size_t)NC * nb, 0);
    pl.slots.assign((size_t)NC * nb, -1);
    int cap_err = 0;
    for (int i = 0; i < nb; ++i) {
        const ingvio_gnss_epoch_nominal& e = blocks[i].epoch;
        if (e.n_sat < 0 || e.n_sat > INGVIO_GNSS_MAX_SAT || (e.n_sat && (!e.eph || !e.obs))) { c->err = std::string(who) + ": n_sat outside 0..64 or a missing array"; return INGVIO_E_ARG; }
        if (!rows_only && (!chi2_table || chi2_len <= e.n_sat)) { c->err = std::string(who) + ": chi2_table is shorter than n_sat + 1"; return INGVIO_E_ARG; }
        if (e.n_sat == 0) continue;
        if (e.n_sat > pl.smax) pl.smax = e.n_sat;
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        if (I[NOM_GNSS + NOM_G_YOF] < 0) continue;                    // GnssUpdate.cpp:300-301 returns silently: no candidates, not an error
        int nc = 0;
        if (rows_only) nc = 1;
        else {
            if (fabs(blocks[i].vel_spp[3]) > 1e-3 && I[NOM_GNSS + NOM_G_FS] < 0) { pl.cand[(size_t)0 * nb + i] = 1; ++nc; }
            for (int s4 = 0; s4 < 4; ++s4)
                if (fabs(blocks[i].pos_spp[3 + s4]) > 1e-3 && I[NOM_GNSS + s4] < 0) { pl.cand[(size_t)(1 + s4) * nb + i] = 1; ++nc; }
        }
        if (!nc) continue;
        const int ix_pose = nom_idx_of(c, b, I[NOM_V_POSE]), ix_yof = nom_idx_of(c, b, I[NOM_GNSS + NOM_G_YOF]);
        if (ix_pose < 0 || ix_pose + 9 > c->h_n[b] || ix_yof < 0 || ix_yof + 1 > c->h_n[b]) {
            c->err = std::string(who) + ": the extended pose or YOF lies beyond the live state"; return INGVIO_E_NOT_IN_STATE;
        }
        pl.any = true;
        if (rows_only) continue;
        // capacity (reported after every argument of the call has been looked at)
        int got = 0, v = 0;
        for (int g = 0; g < NC; ++g) {
            if (!pl.cand[(size_t)g * nb + i]) continue;
            while (v < m.vmax && var[4 * v] != NOM_KIND_NONE) ++v;
            if (v < m.vmax) { pl.slots[(size_t)g * nb + i] = v++; ++got; }
            pl.round[g] = true;
        }
        if (got < nc || c->h_n[b] + nc > c->d.n_max || e.n_sat > c->mld) { cap_err = 1; continue; }
        if (c->h_n[b] + nc > pl.n_cap) pl.n_cap = c->h_n[b] + nc;
    }
    if (!cap_err && pl.any && !rows_only && !ekf_core_fits(63, 10)) cap_err = 1;
    return cap_err ? INGVIO_E_CAPACITY : INGVIO_OK;
}

// the call's epochs, ephemerides and receiver records (the SPP fix in the scalars the table lacks) into the host slab h
static void gnss_init_fill(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_init_block* blocks, const GnssInitPlan& pl, double* he, double* ho, double* hr,
                           int only_g = -1)
{
    const size_t S = pl.smax;
    for (int i = 0; i < nb; ++i) {
        const ingvio_gnss_epoch_nominal& e = blocks[i].epoch;
        if (e.n_sat) {
            memcpy(he + (size_t)i * S * GE_N, e.eph, 8 * (size_t)e.n_sat * GE_N);
            memcpy(ho + (size_t)i * S * GO_N, e.obs, 8 * (size_t)e.n_sat * GO_N);
        }
        double* r = hr + (size_t)i * GR_N;
        r[GR_NSAT] = e.n_sat; r[GR_DOY] = e.doy; r[GR_HAVE_ION] = e.ion ? 1.0 : 0.0;
        if (e.ion) memcpy(r + GR_ION, e.ion, 64);
        memcpy(r + GR_RENU, e.R_enu2ecef, 72); memcpy(r + GR_ANCHOR, e.anchor_ecef, 24);
        r[GR_PSR_AMP] = e.psr_noise_amp; r[GR_DOPP_AMP] = e.dopp_noise_amp;
        r[GR_ADJ_YOF] = c->gnss_adjust_yof ? 1.0 : 0.0;
        // the scalars to add take the SPP fix (:343-372); k_gnss_front reads these fields only where the table has no such scalar
        const int* I = &c->nom.h_ih[(size_t)(b0 + i) * c->nom.ir];
        const bool fs_add = only_g >= 0 ? (fabs(blocks[i].vel_spp[3]) > 1e-3 && I[NOM_GNSS + NOM_G_FS] < 0) : pl.cand[(size_t)0 * nb + i] != 0;
        r[GR_FS] = fs_add ? blocks[i].vel_spp[3] : 0.0;
        for (int s4 = 0; s4 < 4; ++s4) {
            const bool add = only_g >= 0 ? (fabs(blocks[i].pos_spp[3 + s4]) > 1e-3 && I[NOM_GNSS + s4] < 0) : pl.cand[(size_t)(1 + s4) * nb + i] != 0;
            r[GR_CB + s4] = add ? blocks[i].pos_spp[3 + s4] : 0.0;
        }
    }
}

int ingvio_gnss_init_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_init_block* blocks, const double* chi2_table, int chi2_len, double chi2_mult,
                             int do_chi2, int* added, int* new_idx, int* slot, double* chi2, double* noise, double* dx, int* status)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    if (!added || !new_idx || !slot || !chi2 || !noise) return INGVIO_E_ARG;
    GnssInitPlan pl;
    if (int rc = gnss_init_validate(c, "ingvio_gnss_init_nominal", b0, nb, blocks, chi2_table, chi2_len, pl)) return rc;
    const int NC = INGVIO_GNSS_INIT_CAND;
    const size_t RN = (size_t)NC * nb, S = pl.smax;
    for (size_t e = 0; e < RN; ++e) { added[e] = 0; new_idx[e] = -1; slot[e] = -1; chi2[e] = 0.0; noise[e] = 0.0; }
    if (dx) memset(dx, 0, 8 * RN * c->ldp);
    if (status) for (int i = 0; i < nb; ++i) status[i] = INGVIO_OK;
    if (!pl.any) return INGVIO_OK;                                                      // nothing to try anywhere: nothing is launched
    // ---- one slab up: candidates, slots, values, the chi2 table, ephemerides, observations, receiver records ----
    const size_t ntab = 65;
    const size_t o_cd = 0, o_sl = o_cd + pad64(4 * RN), o_val = o_sl + pad64(4 * RN), o_tab = o_val + pad64(8 * RN), o_eph = o_tab + pad64(8 * ntab),
                 o_obs = o_eph + pad64(8 * (size_t)nb * S * GE_N), o_rcv = o_obs + pad64(8 * (size_t)nb * S * GO_N), in_bytes = o_rcv + pad64(8 * (size_t)nb * GR_N);
    Rounds rd;
    rd.b0 = b0; rd.nb = nb; rd.R = NC; rd.on = pl.round; rd.in_bytes = in_bytes;
    rd.mu_cap = 63; rd.nc_cap = 10; rd.n_cap = pl.n_cap; rd.do_chi2 = do_chi2; rd.dx = dx != nullptr;
    // its own part of the work slab: nc_out | colmap_out | var_out | R_w2ecef | the front's per-satellite records; of the results: slot_out | noise_out
    const size_t q_cm = pad64(4 * (size_t)nb), q_var = q_cm + pad64(4 * (size_t)nb * rd.nc_cap), q_rw = q_var + pad64(8 * (size_t)nb), q_fr = q_rw + pad64(72 * (size_t)nb);
    rd.wk_own = q_fr + pad64(8 * (size_t)nb * 64 * GF_N);
    rd.out_own = pad64(4 * RN) + pad64(8 * RN);
    rd.clear_all = true; rd.table = true;
    if (int rc = rounds_begin(c, rd, [&](char* h) {
            memset(h, 0, in_bytes);
            memcpy(h + o_cd, pl.cand.data(), 4 * RN); memcpy(h + o_sl, pl.slots.data(), 4 * RN);
            double* hval = (double*)(h + o_val);
            for (int i = 0; i < nb; ++i) {
                hval[i] = blocks[i].vel_spp[3];
                for (int s4 = 0; s4 < 4; ++s4) hval[(size_t)(1 + s4) * nb + i] = blocks[i].pos_spp[3 + s4];
            }
            memcpy(h + o_tab, chi2_table, 8 * std::min((size_t)chi2_len, ntab));
            gnss_init_fill(c, b0, nb, blocks, pl, (double*)(h + o_eph), (double*)(h + o_obs), (double*)(h + o_rcv));
        })) return rc;
    auto& w = c->dl;
    char* wk_own = w.wk + rd.w_own;
    const NomTable nt = nom_table(c);
    // ---- the residuals, once (:343-372), and R_w2ecef from YOF as it stands now (:332) ----
    GnssFrontLaunch G;
    memset(&G, 0, sizeof G);
    G.eph = (const double*)(w.in + o_eph); G.obs = (const double*)(w.in + o_obs); G.rcv = (const double*)(w.in + o_rcv); G.smax = (int)S;
    G.front = (double*)(wk_own + q_fr);                                                 // G.H == nullptr: no staged rows
    launch_gnss_front(G, nb, c->st, &nt, b0);
    launch_delayed_gnss_rw(nt, G.rcv, b0, nb, (double*)(wk_own + q_rw), c->st);
    const size_t lds = delayed_front_lds(64, 1, 10);
    DelayedGnssRows Rw;
    memset(&Rw, 0, sizeof Rw);
    Rw.nt = nt; Rw.front = G.front; Rw.eph = G.eph; Rw.obs = G.obs; Rw.rcv = G.rcv; Rw.smax = (int)S; Rw.Rw = (const double*)(wk_own + q_rw);
    Rw.chi2 = (const double*)(w.in + o_tab); Rw.chi2_mult = chi2_mult;
    Rw.var_out = (double*)(wk_own + q_var); Rw.nc_out = (int*)wk_own; Rw.colmap_out = (int*)(wk_own + q_cm);
    int soft = INGVIO_OK;
    if (int rc = rounds_run(c, rd, status, &soft, [&](int g, size_t r0, DelayedFront& F, EkfLaunch& E) {
            Rw.g = g; Rw.cand = (const int*)(w.in + o_cd) + r0; Rw.slot = (const int*)(w.in + o_sl) + r0; Rw.value = (const double*)(w.in + o_val) + r0;
            Rw.slot_out = (int*)(w.out + rd.r_own) + r0; Rw.noise_out = (double*)(w.out + rd.r_own + pad64(4 * RN)) + r0;
            if (launch_delayed_front_gnss(F, Rw, lds, c->st)) return INGVIO_E_CAPACITY;
            E.colmap = Rw.colmap_out; E.nc = Rw.nc_out; E.noise = Rw.var_out; E.nstride = 1;      // R = the round's noise^2, one per filter
            return INGVIO_OK;
        })) return rc;
    const int* rl = (const int*)(w.h_out + rd.r_own);
    const double* rnz = (const double*)(w.h_out + rd.r_own + pad64(4 * RN));
    for (int i = 0; i < nb; ++i) {
        int* I = &c->nom.h_ih[(size_t)(b0 + i) * c->nom.ir];
        for (int g = 0; g < NC; ++g) {
            const size_t e = (size_t)g * nb + i, oo = (size_t)i * NC + g;
            if (!pl.cand[e]) continue;
            noise[oo] = rnz[e];
            if (!rounds_take(c, rd, i, g, oo, added, new_idx, chi2, dx)) continue;      // (slot stays -1)
            slot[oo] = rl[e];
            c->h_n[b0 + i] += 1;                                                        // the mirror follows the front's record
            int* v = I + NOM_IH + 4 * rl[e];
            v[0] = NOM_KIND_SCALAR; v[1] = new_idx[oo]; v[2] = -1; v[3] = 0;
            I[NOM_GNSS + (g == 0 ? NOM_G_FS : g - 1)] = rl[e];
            if (rl[e] >= I[NOM_N_VAR]) I[NOM_N_VAR] = rl[e] + 1;
        }
    }
    if (nom_mark(c)) return INGVIO_E_HIP;
    return soft;
}

// parity hook (tests): the row stage of ingvio_gnss_init_nominal alone, for one filter and candidate g; changes nothing
int ingvio_debug_gnss_init_rows(ingvio_ctx* c, int b, const ingvio_gnss_init_block* block, int g, double* H_old, double* res, double* noise, int* m_out)
{
    ENTER(c);
    if (!c || !block || g < 0 || g >= INGVIO_GNSS_INIT_CAND || !H_old || !res || !noise || !m_out) return INGVIO_E_ARG;
    GnssInitPlan pl;
    if (int rc = gnss_init_validate(c, "ingvio_debug_gnss_init_rows", b, 1, block, nullptr, 0, pl, true)) return rc;
    *m_out = 0; *noise = 0.0;
    if (!pl.any) return INGVIO_OK;
    const size_t S = pl.smax, nrow = 64 * 11 + 1;
    const size_t o_eph = 0, o_obs = o_eph + pad64(8 * S * GE_N), o_rcv = o_obs + pad64(8 * S * GO_N), in_bytes = o_rcv + pad64(8 * GR_N);
    const size_t w_rw = pad64(8 * nrow), w_fr = w_rw + 128, w_m = w_fr + pad64(8 * 64 * GF_N), wk_bytes = w_m + 64;
    auto& w = c->dl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.wk, &w.wk_cap, wk_bytes)) return rc;
    std::vector<char> h(in_bytes, 0);
    gnss_init_fill(c, b, 1, block, pl, (double*)(h.data() + o_eph), (double*)(h.data() + o_obs), (double*)(h.data() + o_rcv), g);
    if (up(c, w.in, h.data(), in_bytes)) return INGVIO_E_HIP;
    const NomTable nt = nom_table(c);
    GnssFrontLaunch G;
    memset(&G, 0, sizeof G);
    G.eph = (const double*)(w.in + o_eph); G.obs = (const double*)(w.in + o_obs); G.rcv = (const double*)(w.in + o_rcv); G.smax = (int)S;
    G.front = (double*)(w.wk + w_fr);
    launch_gnss_front(G, 1, c->st, &nt, b);
    launch_delayed_gnss_rw(nt, G.rcv, b, 1, (double*)(w.wk + w_rw), c->st);
    DelayedGnssRows Rw;
    memset(&Rw, 0, sizeof Rw);
    Rw.nt = nt; Rw.front = G.front; Rw.eph = G.eph; Rw.obs = G.obs; Rw.rcv = G.rcv; Rw.smax = (int)S; Rw.Rw = (const double*)(w.wk + w_rw); Rw.g = g;
    int* d_m = (int*)(w.wk + w_m);
    if (launch_delayed_gnss_rows_debug(Rw, b, (double*)w.wk, d_m, c->st)) return INGVIO_E_CAPACITY;
    std::vector<double> out(nrow);
    int m = 0;
    HIPCHK(c, hipMemcpyAsync(out.data(), w.wk, 8 * nrow, hipMemcpyDeviceToHost, c->st));
    if (down_sync(c, &m, d_m, sizeof(int))) return INGVIO_E_HIP;                        // synchronises: the host vector above may go
    if (int rc = last_launch(c)) return rc;
    *m_out = m;
    if (m == 0) return INGVIO_OK;
    memcpy(H_old, out.data(), 8 * (size_t)m * 10);
    memcpy(res, out.data() + (size_t)m * 10, 8 * (size_t)m);
    *noise = out[(size_t)m * 11];
    return INGVIO_OK;
}

}  // extern "C"

void ingvio_ctx::DelayedWs::release()
{
    for (char* p : { in, wk, out, ws }) if (p) hipFree(p);
    if (h_out) hipHostFree(h_out);
}
