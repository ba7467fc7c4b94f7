// capi_nominal.hip — the C ABI's device-resident nominal table, odometry output and landmark tail (include/ingvio_hip.h).
// Host code only; the context and the shared helpers come from capi_internal.h.
#include "capi_internal.h"

using namespace capi;

extern "C" {

// ---- device-resident nominal state -----------------------------------------------------------------------------
static int nom_size(int kind) { return kind == NOM_KIND_SE23 ? 9 : kind == NOM_KIND_SE3 ? 6 : kind == NOM_KIND_SCALAR ? 1 : 3; }

int ingvio_nominal_create(ingvio_ctx* c, int v_max)
{
    ENTER(c);
    if (!c || phase_busy(c) || v_max < 1 || v_max > 4096) return INGVIO_E_ARG;
    if (c->d.c_max > NOM_IH - NOM_CLONES) return INGVIO_E_UNSUPPORTED;
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
    auto& m = c->nom;
    const size_t B = c->d.batch;
    if (m.vmax != v_max) {
        for (void* p : { (void*)m.ih, (void*)m.dv, (void*)m.ih_snap, (void*)m.dv_snap, (void*)m.dx }) if (p) hipFree(p);
        m.ih = nullptr; m.dv = nullptr; m.ih_snap = nullptr; m.dv_snap = nullptr; m.dx = nullptr; m.vmax = 0;
        const int ir = NOM_IH + 4 * v_max, dr = NOM_DH + NOM_VD * v_max;
        if (dalloc(c, &m.ih, B * ir) || dalloc(c, &m.dv, B * dr) || dalloc(c, &m.ih_snap, B * ir) || dalloc(c, &m.dv_snap, B * dr) ||
            dalloc(c, &m.dx, B * c->ldp)) return INGVIO_E_HIP;
        m.vmax = v_max; m.ir = ir; m.dr = dr;
    }
    m.h_ih.assign(B * m.ir, 0);
    for (size_t b = 0; b < B; ++b) {
        int* I = &m.h_ih[b * m.ir];
        I[NOM_V_EXT] = I[NOM_V_POSE] = I[NOM_V_BG] = I[NOM_V_BA] = -1;
        for (int s = 0; s < 6; ++s) I[NOM_GNSS + s] = -1;
        for (int v = 0; v < v_max; ++v) { I[NOM_IH + 4 * v] = NOM_KIND_NONE; I[NOM_IH + 4 * v + 1] = -1; I[NOM_IH + 4 * v + 2] = -1; }
    }
    HIPCHK(c, hipMemcpyAsync(m.ih, m.h_ih.data(), sizeof(int) * m.h_ih.size(), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemsetAsync(m.dv, 0, sizeof(double) * B * m.dr, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    m.has_snap = false;
    if (m.pending) { c->staged = false; m.pending = false; }
    m.frame = false;
    if (c->gn.nom_pending) { c->gn.nom_pending = false; c->gn.staged = false; }
    if (c->lm.nominal && c->lm.staged) { c->lm.nom_pending = false; c->lm.staged = false; }
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

int ingvio_nominal_set(ingvio_ctx* c, int b0, int nb, const ingvio_nominal* nom)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !nom) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_set without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_set: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_nominal_set")) return INGVIO_E_ARG;
    // ---- validation of every filter before anything is written ----
    for (int i = 0; i < nb; ++i) {
        const ingvio_nominal& q = nom[i];
        if (q.n_var < 0 || q.n_var > m.vmax || q.n_clones < 0 || q.n_clones > c->d.c_max) return INGVIO_E_CAPACITY;
        if (q.n_var && (!q.kind || !q.idx || !q.anchor || !q.val)) return INGVIO_E_ARG;
        if (q.n_clones && !q.clone_var) return INGVIO_E_ARG;
        auto kind_of = [&](int v) { return v >= 0 && v < q.n_var ? q.kind[v] : -2; };
        for (int v = 0; v < q.n_var; ++v) {
            const int k = q.kind[v];
            if (k < NOM_KIND_NONE || k > NOM_KIND_LM) return INGVIO_E_ARG;
            if (k == NOM_KIND_NONE) continue;
            if (q.idx[v] < 0 || q.idx[v] + nom_size(k) > c->d.n_max) return INGVIO_E_ARG;
            if (k == NOM_KIND_LM && kind_of(q.anchor[v]) != NOM_KIND_SE3) return INGVIO_E_ARG;
        }
        for (int a = 0; a < q.n_clones; ++a) {
            if (kind_of(q.clone_var[a]) != NOM_KIND_SE3) return INGVIO_E_ARG;
            for (int b = 0; b < a; ++b) if (q.clone_var[b] == q.clone_var[a]) return INGVIO_E_ARG;
        }
        if ((q.v_ext >= 0 && kind_of(q.v_ext) != NOM_KIND_SE3) || (q.v_pose >= 0 && kind_of(q.v_pose) != NOM_KIND_SE23) ||
            (q.v_bg >= 0 && kind_of(q.v_bg) != NOM_KIND_VEC3) || (q.v_ba >= 0 && kind_of(q.v_ba) != NOM_KIND_VEC3)) return INGVIO_E_ARG;
    }
    std::vector<int> ih((size_t)nb * m.ir, 0);
    std::vector<double> dv((size_t)nb * m.dr, 0.0);
    for (int i = 0; i < nb; ++i) {
        const ingvio_nominal& q = nom[i];
        int* I = &ih[(size_t)i * m.ir];
        double* D = &dv[(size_t)i * m.dr];
        I[NOM_N_VAR] = q.n_var; I[NOM_N_CLONES] = q.n_clones;
        I[NOM_V_EXT] = q.v_ext; I[NOM_V_POSE] = q.v_pose; I[NOM_V_BG] = q.v_bg; I[NOM_V_BA] = q.v_ba;
        for (int s = 0; s < 6; ++s) I[NOM_GNSS + s] = -1;                  // a new table: the GNSS scalars are registered again
        for (int a = 0; a < q.n_clones; ++a) I[NOM_CLONES + a] = q.clone_var[a];
        for (int v = 0; v < m.vmax; ++v) {
            const bool used = v < q.n_var && q.kind[v] != NOM_KIND_NONE;
            I[NOM_IH + 4 * v] = used ? q.kind[v] : NOM_KIND_NONE;
            I[NOM_IH + 4 * v + 1] = used ? q.idx[v] : -1;
            I[NOM_IH + 4 * v + 2] = used && q.kind[v] == NOM_KIND_LM ? q.anchor[v] : -1;
            if (used) memcpy(D + NOM_DH + (size_t)v * NOM_VD, q.val + (size_t)v * INGVIO_NOM_VAL, 8 * INGVIO_NOM_VAL);
        }
        memcpy(D, q.gravity, 24);
    }
    HIPCHK(c, hipMemcpyAsync(m.ih + (size_t)b0 * m.ir, ih.data(), sizeof(int) * ih.size(), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(m.dv + (size_t)b0 * m.dr, dv.data(), sizeof(double) * dv.size(), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    memcpy(&m.h_ih[(size_t)b0 * m.ir], ih.data(), sizeof(int) * ih.size());
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

int ingvio_nominal_get(ingvio_ctx* c, int b0, int nb, ingvio_nominal* out)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !out) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_get without ingvio_nominal_create"; return INGVIO_E_ARG; }
    for (int i = 0; i < nb; ++i) if (!out[i].kind || !out[i].idx || !out[i].anchor || !out[i].val || !out[i].clone_var) return INGVIO_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));      // an asynchronous stage from the table writes it there
    std::vector<int> ih((size_t)nb * m.ir);
    std::vector<double> dv((size_t)nb * m.dr);
    HIPCHK(c, hipMemcpyAsync(ih.data(), m.ih + (size_t)b0 * m.ir, sizeof(int) * ih.size(), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(dv.data(), m.dv + (size_t)b0 * m.dr, sizeof(double) * dv.size(), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (int i = 0; i < nb; ++i) {
        ingvio_nominal& q = out[i];
        const int* I = &ih[(size_t)i * m.ir];
        const double* D = &dv[(size_t)i * m.dr];
        q.n_var = I[NOM_N_VAR]; q.n_clones = I[NOM_N_CLONES];
        q.v_ext = I[NOM_V_EXT]; q.v_pose = I[NOM_V_POSE]; q.v_bg = I[NOM_V_BG]; q.v_ba = I[NOM_V_BA];
        for (int a = 0; a < q.n_clones; ++a) q.clone_var[a] = I[NOM_CLONES + a];
        for (int v = 0; v < q.n_var; ++v) {
            q.kind[v] = I[NOM_IH + 4 * v]; q.idx[v] = I[NOM_IH + 4 * v + 1]; q.anchor[v] = I[NOM_IH + 4 * v + 2];
            memcpy(q.val + (size_t)v * INGVIO_NOM_VAL, D + NOM_DH + (size_t)v * NOM_VD, 8 * INGVIO_NOM_VAL);
        }
        memcpy(q.gravity, D, 24);
    }
    return INGVIO_OK;
}

int ingvio_nominal_box_plus(ingvio_ctx* c, int b0, int nb, const double* dx)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !dx) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_box_plus without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_box_plus: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_nominal_box_plus")) return INGVIO_E_ARG;
    const size_t bytes = 8 * (size_t)nb * c->ldp;
    Uploader upl{ c };
    if (int rc = upl.begin(bytes + 64)) return rc;
    double* h = upl.take<double>((size_t)nb * c->ldp);
    memcpy(h, dx, bytes);
    upl.copy(m.dx + (size_t)b0 * c->ldp, h, (size_t)nb * c->ldp);
    if (int rc = upl.end()) return rc;
    launch_nominal_update(nom_table(c), m.dx, c->ldp, nullptr, b0, nb, c->st);
    if (int rc = last_launch(c)) return rc;
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// Test hook: k_nominal_update_post alone on the TABLE of filters [b0, b0 + nb) - boxPlus of dx [nb][ldp] given in the index space behind
// the marginalisation of marg_idx[i] (a window clone, >= 0), then the drop and the shift.  The covariance is not touched: the caller
// compares the table with its host model and discards the context.
int ingvio_debug_nominal_update_post(ingvio_ctx* c, int b0, int nb, const double* dx, const int* marg_idx)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !dx || !marg_idx) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax || m.pending || gnss_nom_busy(c, "ingvio_debug_nominal_update_post")) return INGVIO_E_ARG;
    static const int size_of[5] = { 9, 6, 3, 1, 3 };
    for (int i = 0; i < nb; ++i) {
        const int* I = &m.h_ih[(size_t)(b0 + i) * m.ir];
        const int* var = I + NOM_IH;
        const int mg = marg_idx[i];
        bool clone = false;
        for (int q = 0; q < I[NOM_N_CLONES]; ++q) if (mg >= 0 && var[4 * I[NOM_CLONES + q] + 1] == mg) clone = true;
        if (!clone) return INGVIO_E_NOT_IN_STATE;
        for (int v = 0; v < I[NOM_N_VAR]; ++v) {                       // every word of dx a lane will read lies inside the row
            const int kind = var[4 * v], idx = var[4 * v + 1];
            if (kind == NOM_KIND_NONE || idx == mg) continue;
            if (kind < 0 || kind > NOM_KIND_LM || idx < 0 || (idx > mg ? idx - 6 : idx) + size_of[kind] > c->ldp) return INGVIO_E_NOT_IN_STATE;
        }
    }
    int* d_marg = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_marg, sizeof(int) * (size_t)c->d.batch));
    int rc = up(c, d_marg + b0, marg_idx, sizeof(int) * (size_t)nb) | up(c, m.dx + (size_t)b0 * c->ldp, dx, 8 * (size_t)nb * c->ldp);
    if (!rc) launch_nominal_update_post(nom_table(c), m.dx, c->ldp, d_marg, b0, nb, c->st);
    hipStreamSynchronize(c->st);                                        // (pageable sources, the temporary)
    hipFree(d_marg);
    if (rc) return INGVIO_E_HIP;
    if (int rc2 = last_launch(c)) return rc2;
    for (int i = 0; i < nb; ++i) nom_mirror_marg(c, b0 + i, marg_idx[i]);
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// the table slots of the GNSS scalars (State::GNSSType order: clock GPS, GLO, GAL, BDS, FS, YOF); they live in the integer record
int ingvio_nominal_set_gnss(ingvio_ctx* c, int b0, int nb, const int* slots)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !slots) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_set_gnss without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_set_gnss: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_nominal_set_gnss")) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i) {
        const int* I = &m.h_ih[(size_t)(b0 + i) * m.ir];
        for (int s = 0; s < 6; ++s) {
            const int v = slots[6 * i + s];
            if (v == -1) continue;
            if (v < 0 || v >= I[NOM_N_VAR] || I[NOM_IH + 4 * v] != NOM_KIND_SCALAR) {
                c->err = "ingvio_nominal_set_gnss: a slot is out of range or holds no Scalar"; return INGVIO_E_ARG;
            }
            for (int t = 0; t < s; ++t) if (slots[6 * i + t] == v) { c->err = "ingvio_nominal_set_gnss: a slot is named twice"; return INGVIO_E_ARG; }
        }
    }
    // behind the kernels that read the record (the stream orders the copies); the six ints of a filter are contiguous
    Uploader upl{ c };
    if (int rc = upl.begin(pad64(sizeof(int) * 6 * (size_t)nb) + 64)) return rc;
    int* h = upl.take<int>(6 * (size_t)nb);
    memcpy(h, slots, sizeof(int) * 6 * (size_t)nb);
    // (no frame is staged from the table here - refused above - so nothing on the copy stream reads the record)
    upl.copy_rows(m.ih + (size_t)b0 * m.ir + NOM_GNSS, (size_t)m.ir, h, (size_t)6, (size_t)6, (size_t)nb);
    if (int rc = upl.end()) return rc;
    for (int i = 0; i < nb; ++i) memcpy(&m.h_ih[(size_t)(b0 + i) * m.ir + NOM_GNSS], slots + 6 * (size_t)i, sizeof(int) * 6);
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

int ingvio_nominal_get_gnss(ingvio_ctx* c, int b0, int nb, int* slots)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !slots) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_get_gnss without ingvio_nominal_create"; return INGVIO_E_ARG; }
    for (int i = 0; i < nb; ++i) memcpy(slots + 6 * (size_t)i, &m.h_ih[(size_t)(b0 + i) * m.ir + NOM_GNSS], sizeof(int) * 6);      // the mirror is the record
    return INGVIO_OK;
}

// ---- odometry output (kernels_odom.hip) -----------------------------------------------------------------------------
static_assert(sizeof(ingvio_odom) == 8 * ODOM_REC, "ingvio_odom and the kernel's record differ");
static_assert(offsetof(ingvio_odom, R_i2w) == 8 * (ODOM_HDR + ODOM_O_VAL) && offsetof(ingvio_odom, diag_min) == 8 * (ODOM_HDR + ODOM_O_DIAG) &&
              offsetof(ingvio_odom, cov_err) == 8 * (ODOM_HDR + ODOM_O_ERR) && offsetof(ingvio_odom, cov_pose) == 8 * (ODOM_HDR + ODOM_O_POSE) &&
              offsetof(ingvio_odom, cov_vel) == 8 * (ODOM_HDR + ODOM_O_VEL) && offsetof(ingvio_odom, gnss) == 8 * (ODOM_HDR + ODOM_O_VAL + 33),
              "ingvio_odom and the kernel's record differ");
static_assert(INGVIO_ODOM_COV == ODOM_W_COV && INGVIO_ODOM_EUCL == ODOM_W_EUCL && INGVIO_ODOM_DIAG == ODOM_W_DIAG &&
              INGVIO_ODOM_NONFINITE == ODOM_S_NONFINITE && INGVIO_ODOM_NEG_DIAG == ODOM_S_NEG_DIAG && INGVIO_ODOM_ABSENT == ODOM_S_ABSENT &&
              INGVIO_MARGINAL_NS_MAX == MARG_NS_MAX, "ingvio_hip.h and launch_odom.h differ");

// Only enqueues: the kernel, the table event behind it (an asynchronous stage from the table waits for that one before its IMU steps
// advance the pose), the copy of the records into their pinned mirror, the event ingvio_odom_end waits for.  Every refusal comes first.
int ingvio_odom_begin(ingvio_ctx* c, int b0, int nb, int what)
{
    if (!c || check_range(c, b0, nb)) return INGVIO_E_ARG;
    auto& m = c->nom;
    auto& o = c->od;
    if (what & ~(INGVIO_ODOM_COV | INGVIO_ODOM_EUCL | INGVIO_ODOM_DIAG)) { c->err = "ingvio_odom_begin: an unknown bit in what"; return INGVIO_E_ARG; }
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (!m.vmax) { c->err = "ingvio_odom_begin without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_odom_begin: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_odom_begin")) return INGVIO_E_ARG;
    if ((c->gn.frame_nom && c->gn.staged) || (c->lm.nominal && c->lm.staged)) {
        c->err = "ingvio_odom_begin: an in-frame GNSS epoch or landmark update staged from the device nominal state has not run yet";
        return INGVIO_E_ARG;
    }
    if (o.pending) { c->err = "ingvio_odom_begin: the previous ingvio_odom_begin has not been ended"; return INGVIO_E_ARG; }
    ENTER(c);
    if (!o.d) {                                                        // the first call of the context
        HIPCHK(c, hipMalloc((void**)&o.d, 8 * (size_t)c->d.batch * ODOM_REC));
        if (hipHostMalloc((void**)&o.h, 8 * (size_t)c->d.batch * ODOM_REC, hipHostMallocDefault) != hipSuccess) {
            hipFree(o.d); o.d = nullptr; o.h = nullptr;
            c->err = "ingvio_odom_begin: hipHostMalloc"; return INGVIO_E_HIP;
        }
    }
    if (!o.ev) HIPCHK(c, hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
    if (what & INGVIO_ODOM_EUCL) what |= INGVIO_ODOM_COV;
    launch_odom_out(nom_table(c), view_ro(c), o.d, b0, nb, what, c->st);
    if (int rc = last_launch(c)) return rc;
    if (nom_mark(c)) return INGVIO_E_HIP;
    HIPCHK(c, hipMemcpyAsync(o.h + (size_t)b0 * ODOM_REC, o.d + (size_t)b0 * ODOM_REC, 8 * (size_t)nb * ODOM_REC, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipEventRecord(o.ev, c->st));
    o.pending = true; o.b0 = b0; o.nb = nb;
    return INGVIO_OK;
}

int ingvio_odom_end(ingvio_ctx* c, ingvio_odom* out)
{
    if (!c || !out) return INGVIO_E_ARG;                                // (no ENTER: the records are already on their way)
    auto& o = c->od;
    if (!o.pending) { c->err = "ingvio_odom_end without a pending ingvio_odom_begin"; return INGVIO_E_ARG; }
    HIPCHK(c, hipEventSynchronize(o.ev));
    o.pending = false;
    memcpy(out, o.h + (size_t)o.b0 * ODOM_REC, 8 * (size_t)o.nb * ODOM_REC);
    return INGVIO_OK;
}

// ---- the landmark tail of a frame on the device (kernels_tail.hip) ------------------------------------------------
// changeLandmarkAnchor (LandmarkUpdate.cpp:273-361), margSwPose and margAnchoredLandmarkInState (StateManager.cpp:340-353) for filters
// [b0, b0 + nb) in one sweep over P.  Everything is validated on the host mirror before the first launch; the verdicts of the depth test
// come back with the one synchronisation at the end, and the mirror follows them.
int ingvio_nominal_tail(ingvio_ctx* c, int b0, int nb, const ingvio_nominal_tail_block* blocks, int lm_cap, int* verdict, int* status)
{
    ENTER(c);
    if (!c || phase_busy(c) || check_range(c, b0, nb) || !blocks || lm_cap < 0) return INGVIO_E_ARG;
    auto& m = c->nom;
    const char* who = "ingvio_nominal_tail";
    if (!m.vmax) { c->err = "ingvio_nominal_tail without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_tail: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    auto fail = [&](int code, const char* what) { c->err = std::string(who) + ": " + what; return code; };
    int kcap = 0, ecap = 0, mcap = 0, active = 0;
    std::vector<char> mark((size_t)m.vmax);
    for (int i = 0; i < nb; ++i) {
        const ingvio_nominal_tail_block& q = blocks[i];
        const int b = b0 + i;
        if (q.n_reanchor < 0 || q.n_erase < 0 || q.n_marg < 0) return fail(INGVIO_E_ARG, "a negative count");
        if (q.n_reanchor > lm_cap || q.n_reanchor > TAIL_LM_MAX) return fail(INGVIO_E_ARG, "n_reanchor exceeds lm_cap or 64");
        if ((q.n_reanchor && (!q.lm_slot || !verdict)) || (q.n_erase && !q.erase_slot) || (q.n_marg && !q.marg_slot)) return fail(INGVIO_E_ARG, "NULL where data is needed");
        if (q.n_erase > m.vmax || q.n_marg > NOM_IH - NOM_CLONES) return fail(INGVIO_E_ARG, "more slots listed than the table holds");
        if (q.n_reanchor + q.n_erase + q.n_marg == 0) continue;
        ++active;
        kcap = std::max(kcap, q.n_reanchor); ecap = std::max(ecap, q.n_erase); mcap = std::max(mcap, q.n_marg);
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        const int nv = I[NOM_N_VAR], nc = I[NOM_N_CLONES], n = c->h_n[b];
        auto in_window = [&](int sl) { for (int w = 0; w < nc; ++w) if (I[NOM_CLONES + w] == sl) return true; return false; };
        auto is_marg = [&](int sl) { for (int e = 0; e < q.n_marg; ++e) if (q.marg_slot[e] == sl) return true; return false; };
        // every column index the kernels form comes from the table: all of it has to lie inside the live state
        for (int v = 0; v < nv; ++v)
            if (var[4 * v] != NOM_KIND_NONE && (var[4 * v + 1] < 0 || var[4 * v + 1] + nom_size(var[4 * v]) > n)) return fail(INGVIO_E_NOT_IN_STATE, "a table variable lies beyond the filter's n");
        std::fill(mark.begin(), mark.end(), 0);
        for (int e = 0; e < q.n_reanchor + q.n_erase; ++e) {
            const int sl = e < q.n_reanchor ? q.lm_slot[e] : q.erase_slot[e - q.n_reanchor];
            if (sl < 0 || sl >= nv || var[4 * sl] != NOM_KIND_LM) return fail(INGVIO_E_NOT_IN_STATE, "a listed slot is free or holds no landmark");
            if (mark[sl]) return fail(INGVIO_E_ARG, "a landmark slot is named twice");
            mark[sl] = 1;
        }
        for (int e = 0; e < q.n_marg; ++e) {
            const int sl = q.marg_slot[e];
            if (sl < 0 || sl >= nv || var[4 * sl] != NOM_KIND_SE3 || !in_window(sl)) return fail(INGVIO_E_NOT_IN_STATE, "a marg_slot is no window clone");
            for (int t = 0; t < e; ++t) if (q.marg_slot[t] == sl) return fail(INGVIO_E_ARG, "a marg_slot is named twice");
        }
        if (q.n_reanchor) {
            const int na = q.new_anchor;
            if (na < 0 || na >= nv || var[4 * na] != NOM_KIND_SE3 || !in_window(na)) return fail(INGVIO_E_NOT_IN_STATE, "new_anchor is no window clone");
            if (is_marg(na)) return fail(INGVIO_E_ARG, "new_anchor is listed in marg_slot");
            if (nc < 2) return fail(INGVIO_E_ARG, "an anchor change needs two window clones (MapServerManager.cpp:347)");
            for (int e = 0; e < q.n_reanchor; ++e) {
                const int an = var[4 * q.lm_slot[e] + 2];
                if (an == na) return fail(INGVIO_E_ARG, "a landmark is already anchored to new_anchor");
                if (an < 0 || an >= nv || var[4 * an] != NOM_KIND_SE3) return fail(INGVIO_E_ARG, "a landmark without a live anchor");
            }
        }
        for (int v = 0; v < nv; ++v)
            if (var[4 * v] == NOM_KIND_LM && !mark[v] && is_marg(var[4 * v + 2])) return fail(INGVIO_E_ARG, "a surviving landmark would stay anchored to a clone that leaves");
    }
    if (tail_panel_lds(c->ldp) > TAIL_LDS_MAX) return fail(INGVIO_E_CAPACITY, "the state is too wide for the panel kernel's index maps");
    if (status) for (int i = 0; i < nb; ++i) status[i] = INGVIO_OK;
    if (verdict) for (size_t e = 0; e < (size_t)nb * lm_cap; ++e) verdict[e] = 0;
    if (!active) return INGVIO_OK;                                                      // nothing to do anywhere: nothing is launched
    // ---- lists up, workspace ----
    const int istride = TAIL_HDR + kcap + ecap + mcap, ld = c->ldp;
    const size_t in_bytes = pad64(sizeof(int) * (size_t)nb * istride);
    const size_t zstride = (size_t)ld * 3 * kcap;
    const size_t w_ver = pad64(sizeof(int) * (size_t)nb), w_map = w_ver + pad64(sizeof(int) * (size_t)nb * std::max(kcap, 1)),
                 w_tag = w_map + pad64(sizeof(int) * (size_t)nb * ld), w_Z = w_tag + pad64(sizeof(int) * (size_t)nb * ld),
                 ws_bytes = w_Z + 8 * (size_t)nb * zstride + 64, out_bytes = w_map;      // nnew | verdict come back
    auto& w = c->tl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.ws, &w.ws_cap, ws_bytes)) return rc;
    if (w.out_cap < out_bytes) {
        if (w.h_out) { hipHostFree(w.h_out); w.h_out = nullptr; w.out_cap = 0; }
        HIPCHK(c, hipHostMalloc((void**)&w.h_out, out_bytes + 4096, hipHostMallocDefault));
        w.out_cap = out_bytes + 4096;
    }
    Uploader upl{ c };
    if (int rc = upl.begin(in_bytes + 64)) return rc;
    int* h = upl.take<int>(in_bytes / sizeof(int));
    memset(h, 0, in_bytes);
    for (int i = 0; i < nb; ++i) {
        const ingvio_nominal_tail_block& q = blocks[i];
        int* r = h + (size_t)i * istride;
        r[TAIL_N_RE] = q.n_reanchor; r[TAIL_NEW] = q.n_reanchor ? q.new_anchor : 0; r[TAIL_N_ER] = q.n_erase; r[TAIL_N_MG] = q.n_marg;
        for (int e = 0; e < q.n_reanchor; ++e) r[TAIL_HDR + e] = q.lm_slot[e];
        for (int e = 0; e < q.n_erase; ++e) r[TAIL_HDR + kcap + e] = q.erase_slot[e];
        for (int e = 0; e < q.n_marg; ++e) r[TAIL_HDR + kcap + ecap + e] = q.marg_slot[e];
    }
    upl.copy((int*)w.in, h, in_bytes / sizeof(int));
    if (int rc = upl.end()) return rc;
    if (wait_inputs(c)) return INGVIO_E_HIP;                                            // nothing on the copy stream may still read the table
    TailLaunch L;
    L.cv = view(c); L.t = nom_table(c); L.b0 = b0; L.nb = nb;
    L.in = (const int*)w.in; L.istride = istride; L.kcap = kcap; L.ecap = ecap; L.mcap = mcap;
    L.nnew = (int*)w.ws; L.verdict = (int*)(w.ws + w_ver); L.map = (int*)(w.ws + w_map); L.tag = (int*)(w.ws + w_tag);
    L.Z = (double*)(w.ws + w_Z); L.zstride = zstride;
    if (launch_tail(L, c->d.n_max, c->st)) return fail(INGVIO_E_CAPACITY, "a workspace bound of the tail kernels does not hold");
    HIPCHK(c, hipMemcpyAsync(w.h_out, w.ws, out_bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                                             // only the device knows the verdicts
    if (int rc = last_launch(c)) return rc;
    // ---- the mirror follows the verdicts: the arithmetic of k_tail_panel's table pass on the host's copy ----
    const int* h_nnew = (const int*)w.h_out;
    const int* h_ver = (const int*)(w.h_out + w_ver);
    for (int i = 0; i < nb; ++i) {
        const ingvio_nominal_tail_block& q = blocks[i];
        if (q.n_reanchor + q.n_erase + q.n_marg == 0) continue;
        const int b = b0 + i;
        int* I = &m.h_ih[(size_t)b * m.ir];
        int* var = I + NOM_IH;
        const int nv = I[NOM_N_VAR];
        std::fill(mark.begin(), mark.end(), 0);                                         // 1: the slot leaves
        for (int e = 0; e < q.n_reanchor; ++e) {
            const int v = h_ver[(size_t)i * kcap + e];
            verdict[(size_t)i * lm_cap + e] = v;
            if (v) var[4 * q.lm_slot[e] + 2] = q.new_anchor; else mark[q.lm_slot[e]] = 1;
        }
        for (int e = 0; e < q.n_erase; ++e) mark[q.erase_slot[e]] = 1;
        for (int e = 0; e < q.n_marg; ++e) mark[q.marg_slot[e]] = 1;
        int wq = 0;
        for (int a = 0; a < I[NOM_N_CLONES]; ++a) if (!mark[I[NOM_CLONES + a]]) I[NOM_CLONES + wq++] = I[NOM_CLONES + a];
        I[NOM_N_CLONES] = wq;
        std::vector<int> nidx((size_t)nv, -1);
        int gone = 0;
        for (int v = 0; v < nv; ++v) {
            if (var[4 * v] == NOM_KIND_NONE) continue;
            if (mark[v]) { gone += nom_size(var[4 * v]); continue; }
            int sh = 0;
            for (int u = 0; u < nv; ++u) if (mark[u] && var[4 * u] != NOM_KIND_NONE && var[4 * u + 1] < var[4 * v + 1]) sh += nom_size(var[4 * u]);
            nidx[v] = var[4 * v + 1] - sh;
        }
        for (int v = 0; v < nv; ++v) {
            if (var[4 * v] == NOM_KIND_NONE) continue;
            if (mark[v]) { var[4 * v] = NOM_KIND_NONE; var[4 * v + 1] = -1; var[4 * v + 2] = -1; }
            else var[4 * v + 1] = nidx[v];
        }
        if (h_nnew[i] != c->h_n[b] - gone) return fail(INGVIO_E_HIP, "the device's dimension after the tail disagrees with the host mirror");
        c->h_n[b] = h_nnew[i];
        c->h_cur[b] ^= 1;
    }
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// ---- the GNSS scalars enter and leave the table on the device --------------------------------------------------------
// StateManager::addGNSSVariable (StateManager.cpp:194-231): one kernel appends the 1 x 1 block and writes the table record.  Only
// enqueues; slot and idx are decided on the host mirror, which then follows.
int ingvio_nominal_add_gnss(ingvio_ctx* c, int b0, int nb, const int* gtype, const double* value, const double* var, int* slot_out, int* idx_out)
{
    ENTER(c);
    if (!c || phase_busy(c) || check_range(c, b0, nb) || !gtype || !value || !var || !slot_out || !idx_out) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_nominal_add_gnss without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_add_gnss: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_nominal_add_gnss")) return INGVIO_E_ARG;
    int active = 0;
    for (int i = 0; i < nb; ++i) {
        if (gtype[i] < -1 || gtype[i] > 5) { c->err = "ingvio_nominal_add_gnss: gtype is -1 or a position 0..5"; return INGVIO_E_ARG; }
        if (gtype[i] < 0) continue;
        ++active;
        if (m.h_ih[(size_t)(b0 + i) * m.ir + NOM_GNSS + gtype[i]] >= 0) {
            c->err = "ingvio_nominal_add_gnss: a scalar is already registered at that position"; return INGVIO_E_ARG;
        }
    }
    std::vector<int> slots((size_t)nb, -1);
    for (int i = 0; i < nb; ++i) {
        if (gtype[i] < 0) continue;
        const int* I = &m.h_ih[(size_t)(b0 + i) * m.ir];
        int v = 0;
        while (v < m.vmax && I[NOM_IH + 4 * v] != NOM_KIND_NONE) ++v;
        if (v >= m.vmax) { c->err = "ingvio_nominal_add_gnss: no free table slot"; return INGVIO_E_CAPACITY; }
        if (c->h_n[b0 + i] + 1 > c->d.n_max) { c->err = "ingvio_nominal_add_gnss: n + 1 > n_max"; return INGVIO_E_CAPACITY; }
        slots[i] = v;
    }
    for (int i = 0; i < nb; ++i) { slot_out[i] = -1; idx_out[i] = -1; }
    if (!active) return INGVIO_OK;                                                      // nothing to do anywhere: nothing is launched
    const size_t o_vv = pad64(sizeof(int) * 2 * (size_t)nb), in_bytes = o_vv + pad64(8 * 2 * (size_t)nb);
    auto& w = c->tl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    Uploader upl{ c };
    if (int rc = upl.begin(in_bytes + 64)) return rc;
    char* h = upl.take<char>(in_bytes);
    memset(h, 0, in_bytes);
    int* hg = (int*)h;
    double* hv = (double*)(h + o_vv);
    for (int i = 0; i < nb; ++i) { hg[2 * i] = gtype[i]; hg[2 * i + 1] = slots[i]; hv[2 * i] = value[i]; hv[2 * i + 1] = var[i]; }
    upl.copy((int*)w.in, (const int*)h, in_bytes / sizeof(int));
    if (int rc = upl.end()) return rc;
    if (wait_inputs(c)) return INGVIO_E_HIP;                                            // nothing on the copy stream may still read the table
    launch_nominal_add_gnss(view(c), nom_table(c), b0, nb, (const int*)w.in, (const double*)(w.in + o_vv), c->st);
    if (int rc = last_launch(c)) return rc;
    for (int i = 0; i < nb; ++i) {
        if (gtype[i] < 0) continue;
        const int b = b0 + i, sl = slots[i];
        int* I = &m.h_ih[(size_t)b * m.ir];
        int* v = I + NOM_IH + 4 * sl;
        v[0] = NOM_KIND_SCALAR; v[1] = c->h_n[b]; v[2] = -1; v[3] = 0;
        I[NOM_GNSS + gtype[i]] = sl;
        if (sl >= I[NOM_N_VAR]) I[NOM_N_VAR] = sl + 1;
        slot_out[i] = sl; idx_out[i] = c->h_n[b];
        c->h_n[b] += 1;
    }
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// StateManager::margGNSSVariable (StateManager.cpp:233-242): the compaction of ingvio_nominal_tail with the named scalars as its erase
// list - one read of P, one write into the other half, the table pass of k_tail_panel.  Nothing comes back from the device, so the call
// only enqueues and the mirror follows on its own.
int ingvio_nominal_marg_gnss(ingvio_ctx* c, int b0, int nb, const unsigned* mask)
{
    ENTER(c);
    if (!c || phase_busy(c) || check_range(c, b0, nb) || !mask) return INGVIO_E_ARG;
    auto& m = c->nom;
    const char* who = "ingvio_nominal_marg_gnss";
    if (!m.vmax) { c->err = "ingvio_nominal_marg_gnss without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_nominal_marg_gnss: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    auto fail = [&](int code, const char* what) { c->err = std::string(who) + ": " + what; return code; };
    int ecap = 0, active = 0;
    for (int i = 0; i < nb; ++i) if (mask[i] & ~63u) return fail(INGVIO_E_ARG, "a mask names a position above 5");
    for (int i = 0; i < nb; ++i) {
        if (!mask[i]) continue;
        ++active;
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        const int nv = I[NOM_N_VAR], n = c->h_n[b];
        for (int v = 0; v < nv; ++v)
            if (var[4 * v] != NOM_KIND_NONE && (var[4 * v + 1] < 0 || var[4 * v + 1] + nom_size(var[4 * v]) > n)) return fail(INGVIO_E_NOT_IN_STATE, "a table variable lies beyond the filter's n");
        int cnt = 0;
        for (int s = 0; s < 6; ++s) {
            if (!((mask[i] >> s) & 1u)) continue;
            const int sl = I[NOM_GNSS + s];
            if (sl < 0 || sl >= nv || var[4 * sl] != NOM_KIND_SCALAR) return fail(INGVIO_E_NOT_IN_STATE, "a named position is not registered");
            ++cnt;
        }
        ecap = std::max(ecap, cnt);
    }
    if (!active) return INGVIO_OK;                                                      // nothing to do anywhere: nothing is launched
    if (tail_panel_lds(c->ldp) > TAIL_LDS_MAX) return fail(INGVIO_E_CAPACITY, "the state is too wide for the panel kernel's index maps");
    const int istride = TAIL_HDR + ecap, ld = c->ldp;
    const size_t in_bytes = pad64(sizeof(int) * (size_t)nb * istride);
    const size_t w_ver = pad64(sizeof(int) * (size_t)nb), w_map = w_ver + pad64(sizeof(int) * (size_t)nb),
                 w_tag = w_map + pad64(sizeof(int) * (size_t)nb * ld), w_Z = w_tag + pad64(sizeof(int) * (size_t)nb * ld), ws_bytes = w_Z + 64;
    auto& w = c->tl;
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.ws, &w.ws_cap, ws_bytes)) return rc;
    Uploader upl{ c };
    if (int rc = upl.begin(in_bytes + 64)) return rc;
    int* h = upl.take<int>(in_bytes / sizeof(int));
    memset(h, 0, in_bytes);
    for (int i = 0; i < nb; ++i) {
        const int* I = &m.h_ih[(size_t)(b0 + i) * m.ir];
        int* r = h + (size_t)i * istride;
        int cnt = 0;
        for (int s = 0; s < 6; ++s) if ((mask[i] >> s) & 1u) r[TAIL_HDR + cnt++] = I[NOM_GNSS + s];
        r[TAIL_N_ER] = cnt;
    }
    upl.copy((int*)w.in, h, in_bytes / sizeof(int));
    if (int rc = upl.end()) return rc;
    if (wait_inputs(c)) return INGVIO_E_HIP;                                            // nothing on the copy stream may still read the table
    TailLaunch L;
    L.cv = view(c); L.t = nom_table(c); L.b0 = b0; L.nb = nb;
    L.in = (const int*)w.in; L.istride = istride; L.kcap = 0; L.ecap = ecap; L.mcap = 0;
    L.nnew = (int*)w.ws; L.verdict = (int*)(w.ws + w_ver); L.map = (int*)(w.ws + w_map); L.tag = (int*)(w.ws + w_tag);
    L.Z = (double*)(w.ws + w_Z); L.zstride = 0;
    if (launch_tail(L, c->d.n_max, c->st)) return fail(INGVIO_E_CAPACITY, "a workspace bound of the tail kernels does not hold");
    if (int rc = last_launch(c)) return rc;
    // ---- the mirror: the table pass of k_tail_panel on the host's copy ----
    for (int i = 0; i < nb; ++i) {
        if (!mask[i]) continue;
        const int b = b0 + i;
        int* I = &m.h_ih[(size_t)b * m.ir];
        int* var = I + NOM_IH;
        const int nv = I[NOM_N_VAR];
        int gone[6], ng = 0;
        for (int s = 0; s < 6; ++s) {
            if (!((mask[i] >> s) & 1u)) continue;
            const int sl = I[NOM_GNSS + s];
            gone[ng++] = var[4 * sl + 1];
            var[4 * sl] = NOM_KIND_NONE; var[4 * sl + 1] = -1; var[4 * sl + 2] = -1;
            I[NOM_GNSS + s] = -1;
        }
        for (int v = 0; v < nv; ++v) {
            if (var[4 * v] == NOM_KIND_NONE) continue;
            int sh = 0;
            for (int e = 0; e < ng; ++e) if (gone[e] < var[4 * v + 1]) ++sh;
            var[4 * v + 1] -= sh;
        }
        c->h_n[b] -= ng;
        c->h_cur[b] ^= 1;
    }
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// ---- MSCKF anchor change and invalid-feature erase on the track store (k_tracks_maintain) ---------------------------
// changeMSCKFAnchor (KeyframeUpdate.cpp:280-328, SwMargUpdate.cpp:367-413) and eraseInvalidFeatures (MapServerManager.cpp:456-491) for the
// tracks the host lists.  _begin only enqueues, in the pattern of ingvio_odom_begin: the lists up, one kernel, the table event behind it (an
// asynchronous stage on the copy stream is then ordered behind the erasures), the copy of verdicts and depths into a pinned mirror of
// their own, the event _end waits for.  Every refusal is made on the host mirror before anything is enqueued or changed.
static_assert(INGVIO_MAINTAIN_KEEP == TM_KEEP && INGVIO_MAINTAIN_MOVED == TM_MOVED && INGVIO_MAINTAIN_ERASED_UNTRIANGULATED == TM_ERASED_UNTRIANGULATED &&
              INGVIO_MAINTAIN_ERASED_MOVE == TM_ERASED_MOVE && INGVIO_MAINTAIN_ERASED_INVALID == TM_ERASED_INVALID, "ingvio_hip.h and launch_tracks.h differ");

int ingvio_tracks_maintain_begin(ingvio_ctx* c, int b0, int nb, const ingvio_maintain_block* blocks, const ingvio_maintain_opts* opts)
{
    if (!c || check_range(c, b0, nb) || !blocks || !opts) return INGVIO_E_ARG;
    auto& m = c->nom;
    auto& w = c->mt;
    const char* who = "ingvio_tracks_maintain_begin";
    auto fail = [&](int code, const char* what) { c->err = std::string(who) + ": " + what; return code; };
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (!m.vmax) return fail(INGVIO_E_ARG, "no nominal table (ingvio_nominal_create)");
    if (!c->trk.t_max) return fail(INGVIO_E_ARG, "no track store (ingvio_tracks_create)");
    if (m.pending) return fail(INGVIO_E_ARG, "a frame staged from the device nominal state has not run yet");
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    if ((c->gn.frame_nom && c->gn.staged) || (c->lm.nominal && c->lm.staged))
        return fail(INGVIO_E_ARG, "an in-frame GNSS epoch or landmark update staged from the device nominal state has not run yet");
    if (w.pending) return fail(INGVIO_E_ARG, "the previous ingvio_tracks_maintain_begin has not been ended");
    if (opts->list_cap < 0 || opts->lm_cap < 0) return fail(INGVIO_E_ARG, "a negative capacity");
    const int T = c->trk.t_max;
    int tcap = 0, lcap = 0;
    std::vector<char> mark((size_t)T);
    for (int i = 0; i < nb; ++i) {
        const ingvio_maintain_block& q = blocks[i];
        const int* I = &m.h_ih[(size_t)(b0 + i) * m.ir];
        if (q.n_tracks < 0 || q.n_lm < 0) return fail(INGVIO_E_ARG, "a negative count");
        if (q.n_tracks > T || q.n_tracks > opts->list_cap) return fail(INGVIO_E_ARG, "a list is longer than t_max or list_cap");
        if (q.n_lm > m.vmax || q.n_lm > opts->lm_cap) return fail(INGVIO_E_ARG, "more landmark slots listed than the table holds or lm_cap");
        if ((q.n_tracks && !q.tracks) || (q.n_lm && !q.lm_slot)) return fail(INGVIO_E_ARG, "NULL where data is needed");
        tcap = std::max(tcap, q.n_tracks); lcap = std::max(lcap, q.n_lm);
        if (q.n_tracks) std::fill(mark.begin(), mark.end(), 0);
        for (int e = 0; e < q.n_tracks; ++e) {
            const unsigned wd = (unsigned)q.tracks[e];
            const int t = (int)(wd & 0xffffu), pos = (int)((wd >> 16) & 0xffu);
            if (wd >> 25) return fail(INGVIO_E_ARG, "an entry has bits above move set");
            if (t >= T) return fail(INGVIO_E_ARG, "a track lies outside the store");
            if (mark[t]) return fail(INGVIO_E_ARG, "a track is named twice");
            mark[t] = 1;
            if (pos >= I[NOM_N_CLONES]) return fail(INGVIO_E_NOT_IN_STATE, "an anchor_pos lies beyond the window");
        }
        for (int e = 0; e < q.n_lm; ++e) {
            const int sl = q.lm_slot[e];
            if (sl < 0 || sl >= I[NOM_N_VAR] || I[NOM_IH + 4 * sl] != NOM_KIND_LM) return fail(INGVIO_E_NOT_IN_STATE, "a landmark slot is free or holds no landmark");
            const int an = I[NOM_IH + 4 * sl + 2];
            if (an < 0 || an >= I[NOM_N_VAR] || I[NOM_IH + 4 * an] != NOM_KIND_SE3) return fail(INGVIO_E_NOT_IN_STATE, "a landmark without a live anchor");
        }
    }
    ENTER(c);
    w.cnt.resize((size_t)nb * 2);
    for (int i = 0; i < nb; ++i) { w.cnt[2 * i] = blocks[i].n_tracks; w.cnt[2 * i + 1] = blocks[i].n_lm; }
    w.nb = nb; w.tcap = tcap; w.lcap = lcap; w.list_cap = opts->list_cap; w.lm_cap = opts->lm_cap;
    w.launched = tcap + lcap > 0;
    if (!w.launched) { w.pending = true; return INGVIO_OK; }              // every list empty: nothing is launched
    const int istride = TM_HDR + tcap + lcap;
    const size_t ostride = (size_t)tcap + lcap;
    const size_t in_bytes = pad64(sizeof(int) * (size_t)nb * istride), o_ver = pad64(8 * (size_t)nb * ostride), out_bytes = o_ver + pad64((size_t)nb * ostride);
    if (int rc = dev_grow(c, &w.in, &w.in_cap, in_bytes)) return rc;
    if (int rc = dev_grow(c, &w.out, &w.out_cap, out_bytes)) return rc;
    if (w.h_cap < out_bytes) {
        if (w.h_out) { hipHostFree(w.h_out); w.h_out = nullptr; w.h_cap = 0; }
        HIPCHK(c, hipHostMalloc((void**)&w.h_out, out_bytes + 4096, hipHostMallocDefault));
        w.h_cap = out_bytes + 4096;
    }
    if (!w.ev) HIPCHK(c, hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
    Uploader upl{ c };
    if (int rc = upl.begin(in_bytes + 64)) return rc;
    int* h = upl.take<int>(in_bytes / sizeof(int));
    memset(h, 0, in_bytes);
    for (int i = 0; i < nb; ++i) {
        const ingvio_maintain_block& q = blocks[i];
        int* r = h + (size_t)i * istride;
        r[TM_N_TRK] = q.n_tracks; r[TM_N_LM] = q.n_lm;
        if (q.n_tracks) memcpy(r + TM_HDR, q.tracks, sizeof(int) * (size_t)q.n_tracks);
        if (q.n_lm) memcpy(r + TM_HDR + tcap, q.lm_slot, sizeof(int) * (size_t)q.n_lm);
    }
    upl.copy((int*)w.in, h, in_bytes / sizeof(int));
    if (int rc = upl.end()) return rc;
    if (wait_inputs(c)) return INGVIO_E_HIP;                              // nothing on the copy stream may still write the store
    TrackMaintain tm;
    tm.in = (const int*)w.in; tm.istride = istride; tm.tcap = tcap; tm.lcap = lcap;
    tm.move_min_depth = opts->move_min_depth; tm.min_depth = opts->min_depth;
    tm.depth = (double*)w.out; tm.verdict = (unsigned char*)(w.out + o_ver);
    launch_tracks_maintain(track_store(c), nom_table(c), tm, b0, nb, c->st);
    if (int rc = last_launch(c)) return rc;
    if (nom_mark(c)) return INGVIO_E_HIP;
    HIPCHK(c, hipMemcpyAsync(w.h_out, w.out, out_bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipEventRecord(w.ev, c->st));
    w.ev_recorded = true;
    w.pending = true;
    return INGVIO_OK;
}

int ingvio_tracks_maintain_end(ingvio_ctx* c, unsigned char* verdict, double* depth, unsigned char* lm_verdict)
{
    if (!c) return INGVIO_E_ARG;                                          // (no ENTER: the verdicts are already on their way)
    auto& w = c->mt;
    if (!w.pending) { c->err = "ingvio_tracks_maintain_end without a pending ingvio_tracks_maintain_begin"; return INGVIO_E_ARG; }
    if ((w.tcap && !verdict) || (w.lcap && !lm_verdict)) { c->err = "ingvio_tracks_maintain_end: NULL where data is needed"; return INGVIO_E_ARG; }
    if (w.launched) HIPCHK(c, hipEventSynchronize(w.ev));
    w.pending = false;
    if (!w.launched) return INGVIO_OK;
    const size_t ostride = (size_t)w.tcap + w.lcap, o_ver = pad64(8 * (size_t)w.nb * ostride);
    const double* hd = (const double*)w.h_out;
    const unsigned char* hv = (const unsigned char*)(w.h_out + o_ver);
    for (int i = 0; i < w.nb; ++i) {
        const int nt = w.cnt[2 * i], nl = w.cnt[2 * i + 1];
        if (nt) memcpy(verdict + (size_t)i * w.list_cap, hv + (size_t)i * ostride, (size_t)nt);
        if (nt && depth) memcpy(depth + (size_t)i * w.list_cap, hd + (size_t)i * ostride, 8 * (size_t)nt);
        if (nl) memcpy(lm_verdict + (size_t)i * w.lm_cap, hv + (size_t)i * ostride + w.tcap, (size_t)nl);
    }
    return INGVIO_OK;
}

int ingvio_tracks_maintain(ingvio_ctx* c, int b0, int nb, const ingvio_maintain_block* blocks, const ingvio_maintain_opts* opts,
                           unsigned char* verdict, double* depth, unsigned char* lm_verdict)
{
    if (!c || check_range(c, b0, nb) || !blocks || !opts) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i)
        if ((blocks[i].n_tracks > 0 && !verdict) || (blocks[i].n_lm > 0 && !lm_verdict)) { c->err = "ingvio_tracks_maintain: NULL where data is needed"; return INGVIO_E_ARG; }
    if (int rc = ingvio_tracks_maintain_begin(c, b0, nb, blocks, opts)) return rc;
    return ingvio_tracks_maintain_end(c, verdict, depth, lm_verdict);
}

}  // extern "C"

void ingvio_ctx::MaintainWs::release()
{
    for (char* p : { in, out }) if (p) hipFree(p);
    if (h_out) hipHostFree(h_out);
    if (ev) hipEventDestroy(ev);
}

// ---- what ingvio_ctx_destroy gives back for the three structs above (the table's triangulation buffers of the frame stage included) ----
void ingvio_ctx::Nominal::release()
{
    for (void* p : { (void*)ih, (void*)dv, (void*)ih_snap, (void*)dv_snap, (void*)dx, (void*)d_tri_track, (void*)d_tri_ok_st, (void*)d_tri_pf_st }) if (p) hipFree(p);
    if (ev) hipEventDestroy(ev);
}
void ingvio_ctx::OdomOut::release()
{
    for (void* p : { (void*)d, (void*)cols, (void*)ns, (void*)blk }) if (p) hipFree(p);
    if (h) hipHostFree(h);
    if (ev) hipEventDestroy(ev);
}
void ingvio_ctx::TailWs::release()
{
    for (char* p : { in, ws }) if (p) hipFree(p);
    if (h_out) hipHostFree(h_out);
}
