// capi.hip — the C ABI of libingvio_hip.so (include/ingvio_hip.h): context, staging, launches.
// (The delayed initialisations: capi_delayed.hip; nominal table, odometry, tail: capi_nominal.hip.)  gfx950 only, no CPU fallback:
// every entry point fails with INGVIO_E_HIP if the HIP runtime has no device.
#include "capi_internal.h"

#include <condition_variable>
#include <mutex>

#define KMAX 64            // IMU steps per fused propagation call
#define IMU_SLAB_NB 4      // ingvio_propagate(_fused) for up to this many filters: inputs travel as one copy (ingvio_ctx::d_imu)
#define CHI2_CAP 1024

// ---- the shared helpers capi_internal.h declares ---------------------------------------------------------------------------
namespace capi {

FrameView fview(ingvio_ctx* c)
{
    FrameView f;
    f.clone_idx = c->d_clone_idx; f.clone_R = c->d_clone_R; f.clone_p = c->d_clone_p;
    f.n_clones = c->d_nclones; f.n_feat = c->d_nfeat; f.pf = c->d_pf; f.anchor = c->d_anchor;
    f.obs_mask = c->d_mask; f.uv = c->d_uv; f.dof = c->d_dof; f.cmax = c->d.c_max; f.fmax = c->d.f_max;
    return f;
}

int phase_busy(ingvio_ctx* c)
{
    if (c && c->phase_pending) {
        c->err = "a split frame step is pending: finish it with ingvio_frame_run_phase(ctx, 0, 2) first";
        return 1;
    }
    return 0;
}

int up(ingvio_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return 0;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->st));
    return 0;
}

int down_sync(ingvio_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return 0;
}

int last_launch(ingvio_ctx* c)
{
    HIPCHK(c, hipGetLastError());
    return 0;
}

int release_input_set(ingvio_ctx* c)
{
    if (!c->alt_ready) return 0;
    HIPCHK(c, hipEventRecord(c->ev_free[c->set_id], c->st));
    c->free_valid[c->set_id] = true;
    return 0;
}

int join_parts(ingvio_ctx* c)
{
    if (!c->split_pending) return 0;
    for (int p = 0; p < c->parts_alloc; ++p) HIPCHK(c, hipStreamWaitEvent(c->st, c->part[p].ev_done, 0));
    c->split_pending = false;
    return release_input_set(c);                   // the slices' input set, once they are done with it
}

int nom_mark(ingvio_ctx* c)
{
    if (!c->nom.ev) HIPCHK(c, hipEventCreateWithFlags(&c->nom.ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->nom.ev, c->st));
    c->nom.ev_valid = true;
    return 0;
}

int gnss_nom_busy(ingvio_ctx* c, const char* who)
{
    if (!c || (!c->gn.nom_pending && !c->lm.nom_pending)) return 0;
    c->err = std::string(who) + (c->gn.nom_pending ? ": a GNSS epoch staged from the device nominal state has not run yet"
                                                   : ": a landmark update staged from the device nominal state has not run yet");
    return 1;
}

void nom_mirror_marg(ingvio_ctx* c, int b, int m)
{
    if (m < 0) return;
    int* I = &c->nom.h_ih[(size_t)b * c->nom.ir];
    int* var = I + NOM_IH;
    const int nc = I[NOM_N_CLONES];
    int w = 0, drop = -1;
    for (int q = 0; q < nc; ++q) {
        const int sl = I[NOM_CLONES + q];
        if (drop < 0 && var[4 * sl + 1] == m) { drop = sl; continue; }
        I[NOM_CLONES + w++] = sl;
    }
    I[NOM_N_CLONES] = w;
    for (int v = 0; v < I[NOM_N_VAR]; ++v) {
        if (var[4 * v] == NOM_KIND_NONE) continue;
        if (v == drop) { var[4 * v] = NOM_KIND_NONE; var[4 * v + 1] = -1; var[4 * v + 2] = -1; }
        else if (var[4 * v + 1] > m) var[4 * v + 1] -= 6;
    }
}

int stage_small(ingvio_ctx* c, const UpItem* it, int n)
{
    size_t tot = 0;
    for (int i = 0; i < n; ++i) tot += pad64(it[i].bytes);
    Uploader up{ c };
    int rc = up.begin(tot + 64);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        if (!it[i].bytes) continue;
        char* p = up.take<char>(it[i].bytes);
        memcpy(p, it[i].src, it[i].bytes);
        up.copy(reinterpret_cast<char*>(it[i].dst), p, it[i].bytes);
    }
    return up.end();
}

int dev_grow(ingvio_ctx* c, char** p, size_t* cap, size_t need)
{
    if (*cap >= need) return 0;
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    const size_t bytes = (need + (1u << 20)) & ~((size_t)(1u << 20) - 1);
    if (dalloc(c, p, bytes)) return INGVIO_E_HIP;
    *cap = bytes;
    return 0;
}

int stage_generic(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H, int ldh, int m,
                         const double* res, const double* R, int r_kind, int* nc_out)
{
    if (check_range(c, b, 1) || !vidx || !vsize || !H || !res || !R || k < 1 || m < 1 || ldh < m) return INGVIO_E_ARG;
    if (r_kind < 0 || r_kind > 2) return INGVIO_E_ARG;
    if ((m > c->d.m_max && m > 6 * c->d.c_max) || m > c->mld) return INGVIO_E_CAPACITY;
    int nc = 0;
    std::vector<int> cm;
    for (int i = 0; i < k; ++i) {
        if (vidx[i] < 0 || vidx[i] + vsize[i] > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;      // checkSubOrder
        for (int j = 0; j < vsize[i]; ++j) cm.push_back(vidx[i] + j);
        nc += vsize[i];
    }
    if (nc > c->nc_cap) return INGVIO_E_CAPACITY;
    std::vector<double> Hp((size_t)c->mld * nc, 0.0);
    for (int cc = 0; cc < nc; ++cc) memcpy(&Hp[(size_t)cc * c->mld], H + (size_t)cc * ldh, 8 * (size_t)m);
    int rc = up(c, c->d_H + (size_t)b * c->hstride, Hp.data(), 8 * Hp.size());
    rc |= up(c, c->d_res + (size_t)b * c->mld, res, 8 * (size_t)m);
    rc |= up(c, c->d_colmap + (size_t)b * c->cstride, cm.data(), sizeof(int) * (size_t)nc);
    rc |= up(c, c->d_m + b, &m, sizeof(int));
    rc |= up(c, c->d_nc + b, &nc, sizeof(int));
    rc |= up(c, c->d_noise1, R, 8 * (size_t)(r_kind == 0 ? 1 : (r_kind == 1 ? m : m * m)));
    if (rc) return INGVIO_E_HIP;
    HIPCHK(c, hipStreamSynchronize(c->st));
    *nc_out = nc;
    return 0;
}

// the process-wide worker pool behind parallel_for
namespace {
class HostPool {
public:
    static HostPool& get() { static HostPool p; return p; }
    // runs job(t) for t = 1 .. T - 1 on the workers and job(0) on the caller; false: the pool is busy (caller falls back)
    bool run(int T, const std::function<void(int)>& job)
    {
        if (getpid() != owner_) return false;                             // a fork()ed child has the object but not its threads
        std::unique_lock<std::mutex> user(user_m_, std::try_to_lock);
        if (!user.owns_lock()) return false;
        ensure(T - 1);
        if ((int)th_.size() < T - 1) return false;
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &job; want_ = T - 1; pending_ = T - 1; ++gen_;
        }
        cv_start_.notify_all();
        job(0);
        std::unique_lock<std::mutex> lk(m_);
        cv_done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
        return true;
    }
private:
    HostPool() : owner_(getpid()) {}
    ~HostPool()
    {
        if (getpid() != owner_) { for (auto& t : th_) t.detach(); return; }
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++gen_; }
        cv_start_.notify_all();
        for (auto& t : th_) t.join();
    }
    void ensure(int workers)
    {
        try {
            while ((int)th_.size() < workers) { const int id = (int)th_.size() + 1; th_.emplace_back([this, id] { loop(id); }); }
        } catch (...) {                                                   // thread limit: the caller falls back
        }
    }
    void loop(int id)
    {
        unsigned seen = 0;
        for (;;) {
            const std::function<void(int)>* job = nullptr;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_start_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                if (id <= want_) job = job_;
            }
            if (job) {
                (*job)(id);
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) cv_done_.notify_one();
            }
        }
    }
    const pid_t owner_;
    std::mutex user_m_, m_;
    std::condition_variable cv_start_, cv_done_;
    std::vector<std::thread> th_;
    const std::function<void(int)>* job_ = nullptr;
    int want_ = 0, pending_ = 0;
    unsigned gen_ = 0;
    bool stop_ = false;
};
}  // namespace
bool host_pool_run(int T, const std::function<void(int)>& job) { return HostPool::get().run(T, job); }

// the compute stream must not read staged inputs before the copy stream has delivered them
int wait_inputs(ingvio_ctx* c)
{
    if (c->copy_pending) {
        HIPCHK(c, hipStreamWaitEvent(c->st, c->ev_copy, 0));
        c->copy_pending = false;
    }
    return 0;
}

}  // namespace capi

using namespace capi;

namespace {

int parts_prepare(ingvio_ctx* c, int P)
{
    while (c->parts_alloc < P) {
        auto& q = c->part[c->parts_alloc];
        HIPCHK(c, hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&q.ev_gate, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&q.ev_apply, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
        ++c->parts_alloc;
    }
    if (!c->ev_split_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_split_fork, hipEventDisableTiming));
    return 0;
}

// INGVIO_RESTORE=pass: ingvio_frame_run(restore_prior) keeps the separate restore pass in front of the propagation (comparison runs)
static bool no_snap_propagate()
{
    static const bool v = [] { const char* e = getenv("INGVIO_RESTORE"); return e && !strcmp(e, "pass"); }();
    return v;
}

// INGVIO_FLIP=launch: the fused marginalisation's flip of the halves stays a launch of its own (k_post_marg; comparison runs)
static bool no_apply_flip()
{
    static const bool v = [] { const char* e = getenv("INGVIO_FLIP"); return e && !strcmp(e, "launch"); }();
    return v;
}

// The ten device arrays of a staged frame set live in ONE allocation, laid out exactly as pack_frames lays them out in the pinned
// slab (same order, every array 64-byte aligned): a stage of the WHOLE batch is then one host-to-device copy instead of ten (each
// costs ~3.5 us of API time and a ~4.7 us copy kernel on the stream - 80 us of a single filter's 0.3 ms update, round 4).
struct FrameSlabPtrs { int *clone_idx, *nclones, *nfeat, *anchor, *dof; double *clone_R, *clone_p, *pf, *uv; unsigned long long* mask; };
size_t frame_slab_carve(const ingvio_ctx* c, char* base, FrameSlabPtrs* out)
{
    const size_t B = c->d.batch, cm = c->d.c_max, fm = c->d.f_max;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = (off + 63) & ~(size_t)63; char* p = base ? base + off : nullptr; off += bytes; return p; };
    FrameSlabPtrs q;
    q.clone_idx = (int*)take(4 * B * cm); q.nclones = (int*)take(4 * B); q.nfeat = (int*)take(4 * B);
    q.anchor = (int*)take(4 * B * fm); q.dof = (int*)take(4 * B * fm);
    q.clone_R = (double*)take(8 * B * cm * 9); q.clone_p = (double*)take(8 * B * cm * 3);
    // uv last: a whole-batch upload then ends with the measurements of the last filter's LAST USED feature (pack_frames) - a single
    // filter that lost 6 tracks uploads 14 KB instead of the 360 KB its f_max x c_max measurement array takes
    q.pf = (double*)take(8 * B * fm * 3); q.mask = (unsigned long long*)take(8 * B * fm);
    q.uv = (double*)take(8 * B * fm * cm * 4);
    if (out) *out = q;
    return (off + 63) & ~(size_t)63;
}
int frame_slab_alloc(ingvio_ctx* c, char** slab, FrameSlabPtrs* out)
{
    const size_t bytes = frame_slab_carve(c, nullptr, nullptr);
    if (dalloc(c, slab, bytes)) return INGVIO_E_HIP;
    frame_slab_carve(c, *slab, out);
    return 0;
}

int prepare_async_set(ingvio_ctx* c)
{
    if (!c->alt_ready) {
        const int B = c->d.batch, cm = c->d.c_max, fm = c->d.f_max;
        auto& a = c->alt;
        int rc = 0;
        rc |= dalloc(c, &a.Phi, (size_t)B * KMAX * 225); rc |= dalloc(c, &a.G, (size_t)B * KMAX * 180); rc |= dalloc(c, &a.dt, (size_t)B * KMAX);
        rc |= dalloc(c, &a.R, (size_t)B * 9); rc |= dalloc(c, &a.gnss, (size_t)B * 5); rc |= dalloc(c, &a.idx, B);
        {
            FrameSlabPtrs q;
            if (frame_slab_alloc(c, &c->d_frame_slab[1], &q)) rc |= 1;
            else {
                a.clone_idx = q.clone_idx; a.nclones = q.nclones; a.nfeat = q.nfeat; a.anchor = q.anchor; a.dof = q.dof;
                a.clone_R = q.clone_R; a.clone_p = q.clone_p; a.pf = q.pf; a.uv = q.uv; a.mask = q.mask;
            }
        }
        rc |= dalloc(c, &a.chi2, CHI2_CAP); rc |= dalloc(c, &a.noise, B); rc |= dalloc(c, &a.prm, (size_t)B * 8);
        if (rc) return INGVIO_E_HIP;
        HIPCHK(c, hipStreamSynchronize(c->st));                        // the zero fills of dalloc
        HIPCHK(c, hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
        for (auto& e : c->ev_free) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->alt_ready = true;
    }
    return 0;
}

void swap_input_sets(ingvio_ctx* c)
{
    auto& a = c->alt;
    std::swap(c->d_Phi, a.Phi); std::swap(c->d_G, a.G); std::swap(c->d_dt, a.dt); std::swap(c->d_R, a.R);
    std::swap(c->d_gnss, a.gnss); std::swap(c->d_idx, a.idx); std::swap(c->d_clone_idx, a.clone_idx);
    std::swap(c->d_nclones, a.nclones); std::swap(c->d_nfeat, a.nfeat); std::swap(c->d_anchor, a.anchor); std::swap(c->d_dof, a.dof);
    std::swap(c->d_clone_R, a.clone_R); std::swap(c->d_clone_p, a.clone_p); std::swap(c->d_pf, a.pf); std::swap(c->d_uv, a.uv);
    std::swap(c->d_chi2, a.chi2); std::swap(c->d_mask, a.mask); std::swap(c->d_noise, a.noise); std::swap(c->d_prm, a.prm);
    c->upc.chi2_ok = false; c->upc.noise_ok = false;
    c->set_id ^= 1;
}

size_t frames_bytes(const ingvio_ctx* c, int nb)
{
    const size_t cm = c->d.c_max, fm = c->d.f_max, n = nb;
    return pad64(4 * n * cm) + 2 * pad64(4 * n) + 2 * pad64(4 * n * fm) + pad64(8 * n * cm * 9) + pad64(8 * n * cm * 3) + pad64(8 * n * fm * 3) +
           pad64(8 * n * fm * cm * 4) + pad64(8 * n * fm) + 1024;
}

// Everything that can be wrong with the caller's frames, checked BEFORE any context state is touched.  `grow` = rows/columns
// the state gains between now and the update (6: the clone ingvio_frame_run appends; 0: ingvio_msckf_update).
int validate_frames(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* fr, int grow, int* fmax_used)
{
    const int cm = c->d.c_max, fm = c->d.f_max;
    int fmx = 0;
    for (int i = 0; i < nb; ++i) {
        const ingvio_msckf_frame& f = fr[i];
        if (f.n_clones < 0 || f.n_clones > cm || f.n_feat < 0 || f.n_feat > fm) return INGVIO_E_CAPACITY;
        if (f.n_clones > 0 && (!f.clone_idx || !f.clone_R || !f.clone_p)) return INGVIO_E_ARG;
        if (f.n_feat > 0 && (!f.obs_mask || !f.uv)) return INGVIO_E_ARG;
        if (f.n_feat > fmx) fmx = f.n_feat;
        // a clone must lie inside the filter's LIVE state at update time (not merely inside the buffer): the gate and gram
        // kernels would otherwise read stale covariance (checkSubOrder, StateManager.cpp:340-357)
        const int n_live = grow >= 0 ? c->h_n[b0 + i] + grow : c->d.n_max;
        const int n_lim = n_live < c->d.n_max ? n_live : c->d.n_max;
        for (int s = 0; s < f.n_clones; ++s) {
            if (f.clone_idx[s] < 0) return INGVIO_E_ARG;
            if (f.clone_idx[s] + 6 > n_lim) return f.clone_idx[s] + 6 > c->d.n_max ? INGVIO_E_ARG : INGVIO_E_NOT_IN_STATE;
        }
        if (f.anchor)
            for (int j = 0; j < f.n_feat; ++j) if (f.anchor[j] < 0 || f.anchor[j] >= f.n_clones) return INGVIO_E_ARG;
    }
    if (fmax_used) *fmax_used = fmx;
    return 0;
}

// packs already VALIDATED frames [b0, b0+nb) into the slab of `up` and enqueues the copies into the SoA device staging; max F in
// *fmax_used.  Cannot fail.
int pack_frames(ingvio_ctx* c, Uploader& up, int b0, int nb, const ingvio_msckf_frame* fr, int* fmax_used)
{
    const int cm = c->d.c_max, fm = c->d.f_max;
    int fmx = 0;
    for (int i = 0; i < nb; ++i) if (fr[i].n_feat > fmx) fmx = fr[i].n_feat;
    const bool whole = b0 == 0 && nb == c->d.batch;          // the pinned image then IS the device slab's image
    up.off = (up.off + 63) & ~(size_t)63;
    const size_t slab0 = up.off;
    int* cidx = up.take<int>((size_t)nb * cm); int* ncl = up.take<int>(nb); int* nft = up.take<int>(nb);
    int* anc = up.take<int>((size_t)nb * fm); int* dof = up.take<int>((size_t)nb * fm);
    double* cR = up.take<double>((size_t)nb * cm * 9); double* cp = up.take<double>((size_t)nb * cm * 3);
    double* pf = up.take<double>((size_t)nb * fm * 3);
    unsigned long long* mk = up.take<unsigned long long>((size_t)nb * fm);
    double* uv = up.take<double>((size_t)nb * fm * cm * 4);      // same order as frame_slab_carve: uv last
    parallel_for(nb, [=](int i) {
        const ingvio_msckf_frame& f = fr[i];
        const int C = f.n_clones, F = f.n_feat;
        ncl[i] = C; nft[i] = F;
        memcpy(cidx + (size_t)i * cm, f.clone_idx, sizeof(int) * (size_t)C);
        memcpy(cR + (size_t)i * cm * 9, f.clone_R, 72 * (size_t)C);
        memcpy(cp + (size_t)i * cm * 3, f.clone_p, 24 * (size_t)C);
        if (f.pf) memcpy(pf + (size_t)i * fm * 3, f.pf, 24 * (size_t)F); else memset(pf + (size_t)i * fm * 3, 0, 24 * (size_t)F);
        if (f.anchor) memcpy(anc + (size_t)i * fm, f.anchor, sizeof(int) * (size_t)F); else memset(anc + (size_t)i * fm, 0, sizeof(int) * (size_t)F);
        if (f.dof) memcpy(dof + (size_t)i * fm, f.dof, sizeof(int) * (size_t)F); else memset(dof + (size_t)i * fm, 0, sizeof(int) * (size_t)F);
        const unsigned long long cmask = C >= 64 ? ~0ULL : ((1ULL << C) - 1ULL);
        unsigned long long* mki = mk + (size_t)i * fm;
        for (int j = 0; j < F; ++j) mki[j] = f.obs_mask[j] & cmask;
        for (int j = F; j < fm; ++j) mki[j] = 0ULL;
        double* uvi = uv + (size_t)i * fm * cm * 4;
        if (C == cm) memcpy(uvi, f.uv, 32 * (size_t)F * C);                           // same layout: one block
        else for (int j = 0; j < F; ++j) memcpy(uvi + (size_t)j * cm * 4, f.uv + (size_t)j * C * 4, 32 * (size_t)C);
    });
    for (int i = 0; i < nb; ++i) c->h_nclones[b0 + i] = fr[i].n_clones;
    if (whole) {
        // the image up to the measurements of the last filter's last feature (what lies behind is not read by any kernel)
        const size_t used = (size_t)(reinterpret_cast<char*>(uv) - (up.slab->p + slab0)) + 8 * ((size_t)(nb - 1) * fm + (size_t)fr[nb - 1].n_feat) * cm * 4;
        up.copy(reinterpret_cast<char*>(c->d_clone_idx), up.slab->p + slab0, std::max(used, (size_t)64));
        *fmax_used = fmx;
        return 0;
    }
    up.copy(c->d_clone_idx + (size_t)b0 * cm, cidx, (size_t)nb * cm);
    up.copy(c->d_nclones + b0, ncl, nb);
    up.copy(c->d_nfeat + b0, nft, nb);
    up.copy(c->d_anchor + (size_t)b0 * fm, anc, (size_t)nb * fm);
    up.copy(c->d_dof + (size_t)b0 * fm, dof, (size_t)nb * fm);
    up.copy(c->d_clone_R + (size_t)b0 * cm * 9, cR, (size_t)nb * cm * 9);
    up.copy(c->d_clone_p + (size_t)b0 * cm * 3, cp, (size_t)nb * cm * 3);
    up.copy(c->d_pf + (size_t)b0 * fm * 3, pf, (size_t)nb * fm * 3);
    up.copy(c->d_uv + (size_t)b0 * fm * cm * 4, uv, (size_t)nb * fm * cm * 4);
    up.copy(c->d_mask + (size_t)b0 * fm, mk, (size_t)nb * fm);
    *fmax_used = fmx;
    return 0;
}

// uploads frames [b0, b0+nb) into the SoA staging; returns max F in *fmax_used
int stage_frames(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* fr, int* fmax_used, int grow = 0)
{
    int rc = validate_frames(c, b0, nb, fr, grow, nullptr);
    if (rc) return rc;
    if (wait_inputs(c)) return INGVIO_E_HIP;
    Uploader up{ c };
    rc = up.begin(frames_bytes(c, nb));
    if (rc) return rc;
    pack_frames(c, up, b0, nb, fr, fmax_used);
    return up.end();
}

// the caller's options as the kernels take them; the chi-square table itself is uploaded by whoever calls this
void fill_opts(const ingvio_ctx* c, const ingvio_msckf_opts* o, MsckfOpts* op)
{
    memcpy(op->R_lr, o->R_cl2cr, 72);
    memcpy(op->t_lr, o->t_cl2cr, 24);
    op->var = o->noise * o->noise;
    op->max_accept = o->max_accept;
    op->selected_variant = o->selected_variant;
    op->chi2 = c->d_chi2;
    op->chi2_len = o->chi2_len;
}

int make_opts(ingvio_ctx* c, const ingvio_msckf_opts* o, MsckfOpts* op)
{
    if (!o || !o->chi2_table || o->chi2_len < 2 || o->chi2_len > CHI2_CAP) return INGVIO_E_ARG;
    fill_opts(c, o, op);
    if (wait_inputs(c)) return INGVIO_E_HIP;
    auto& u = c->upc;
    if (u.chi2_ok && (int)u.chi2.size() >= o->chi2_len && !memcmp(u.chi2.data(), o->chi2_table, 8 * (size_t)o->chi2_len)) return 0;      // already there
    const UpItem item = { c->d_chi2, o->chi2_table, 8 * (size_t)o->chi2_len };      // through the pinned ring: no stream synchronisation
    if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
    u.chi2.assign(o->chi2_table, o->chi2_table + o->chi2_len); u.chi2_ok = true;
    return 0;
}

// K3..K11 for filters [b0, b0+nb) using the staged frames; asynchronous.
// phase 0: the whole update; 1: gate + gram only (the chunk partials [A | b] stay in d_Rpart); 2: solve + apply from the partials
#define GNSS_NCW 32        // widest var_order of a staged GNSS update (the reference's is 9 + 1 + 4 + 1 = 15 columns)

// In-frame GNSS update, between the MSCKF solve (stage 2) and its write-back (stage 3): the var_order columns of the posterior
// (k_post_cols) -> per-row gates + compaction -> S, Cholesky, gain (k_ekf_core reading those columns instead of P) -> the gain
// rides on the write-back as a rank-16 downdate (L.gY).  Working rows / counts / dx live in the stage's own buffers.
void gnss_front_launch(ingvio_ctx* c, int b0, int nb, bool nominal, hipStream_t st);      // (defined with the GNSS front stages)
static int gnss_in_frame_launch(ingvio_ctx* c, int b0, int nb, FactoredLaunch& L)
{
    auto& g = c->gn;
    const size_t mld = c->mld, hs = mld * GNSS_NCW, ws = (size_t)c->ldp * 16;
    L.gcolmap = g.colmap + (size_t)b0 * GNSS_NCW; L.gnc = g.nc + b0; L.gcstride = GNSS_NCW;
    L.gW = g.W + (size_t)b0 * ws; L.gWstride = ws;
    if (g.frame_nom) {
        // the epoch of a frame staged from the table: its rows are formed here, at the state after the MSCKF update (IngvioFilter.cpp:277-362) -
        // the MSCKF dx ahead of the write-back, boxPlus on the table without drop and shift (the update's index space, new clone
        // included), then the front from the values and idx just written; the three launches are ordered by the stream
        L.stage = 10; launch_factored(L, c->run_st);
        launch_nominal_update(nom_table(c), c->d_dx, c->ldp, nullptr, b0, nb, c->run_st);
        gnss_front_launch(c, b0, nb, true, c->run_st);
    }
    { ProfScope p(c, PF_POSTCOLS); L.stage = 4; launch_factored(L, c->run_st); }
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = L.cv; E.b0 = b0; E.nb = nb; E.H = c->d_H + (size_t)b0 * hs; E.res = c->d_res + (size_t)b0 * mld;
    E.colmap = c->d_colmap + (size_t)b0 * GNSS_NCW; E.m = g.mf + b0; E.nc = g.ncf + b0;
    E.noise = c->d_noiseB + (size_t)b0 * mld; E.r_kind = INGVIO_R_DIAG; E.mld = c->mld; E.hstride = (int)hs; E.cstride = GNSS_NCW;
    E.nstride = c->mld; E.Y = g.Yf + (size_t)b0 * ws; E.ystride = (int)ws; E.dx = g.dxf;
    E.status = g.own_status ? g.stf : c->d_status; E.m_cap = g.m_cap; E.nc_cap = GNSS_NCW;
    E.W = L.gW; E.wstride = ws; E.ypad = 16; E.marg_idx = L.marg_idx; E.marg_size = L.marg_size;
    if (g.strong) { E.chi2 = g.chi2; E.chi2_len = g.chi2_len; E.gate_max_rows = 14; }      // GnssUpdate.cpp:286
    RowsGateIn in{ g.H + (size_t)b0 * hs, g.res + (size_t)b0 * mld, g.noise + (size_t)b0 * mld, g.m + b0, g.colmap + (size_t)b0 * GNSS_NCW,
                   g.nc + b0, (int)hs, GNSS_NCW };
    {
        ProfScope p(c, PF_ROWGATE);
        if (launch_rows_gate(E, in, g.thr1, g.gamma + (size_t)b0 * mld, g.keep + (size_t)b0 * mld, c->run_st)) return INGVIO_E_CAPACITY;
    }
    { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->run_st); }
    L.gY = E.Y; L.gYstride = ws; L.gm = g.mf + b0;
    g.fused_last = true; g.folded_last = true;
    g.results = true;
    return 0;
}

// frame_step: the call is the fused frame step (ingvio_frame_run, unsplit) - nothing reads the chunk partials but the solve below, so
// the Gram stage may take its reduced form (FactoredLaunch::gram_red); every other caller leaves the full [A | b] in d_Rpart
int run_msckf_factored(ingvio_ctx* c, int b0, int nb, const MsckfOpts& op, int stereo, int fmax_used,
                       const int* marg_idx = nullptr, int marg_size = 0, int phase = 0, bool gnss_fuse = false, bool frame_step = false)
{
    FactoredLaunch L;
    memset(&L, 0, sizeof L);
    L.stereo = stereo; L.cv = view(c); L.fv = fview(c); L.op = op; L.b0 = b0; L.nb = nb;
    L.fmax_used = fmax_used > 0 ? fmax_used : 1;
    L.ncol_cap = 6 * c->d.c_max;
    for (int i = 0; i < nb; ++i) if (c->h_nclones[b0 + i] > L.c_used) L.c_used = c->h_nclones[b0 + i];
    L.gamma = c->d_gamma; L.accept = c->d_accept; L.used = c->d_used; L.rec = c->d_rec;
    L.Apart = c->d_Rpart + (size_t)b0 * c->G * c->rstride; L.chunk_used = c->d_chunk_used + (size_t)b0 * c->G;
    L.G = c->G; L.rstride = c->rstride; L.noise = c->d_noise + b0;
    L.Tflat = c->d_Tflat; L.tfstride = (size_t)c->ldp * 100; L.flat_nb = std::min(c->d.batch, APPLY_FLAT_NB);
    L.Asum = c->d_Asum ? c->d_Asum + (size_t)b0 * c->rstride : nullptr; L.used_sum = c->d_used_sum ? c->d_used_sum + b0 : nullptr;
#ifdef INGVIO_ALT_KERNELS      // INGVIO_FEW=off: few filters take the same kernels as a full batch (chunk partials added inside the solve, k_info_apply)
    static const bool few_off = [] { const char* e = getenv("INGVIO_FEW"); return e && !strcmp(e, "off"); }();
    if (few_off) { L.Tflat = nullptr; L.Asum = nullptr; }
#endif
    L.T = c->d_Y + (size_t)b0 * c->ystride; L.Pc = c->d_Yc + (size_t)b0 * c->ystride; L.ystride = c->ystride;
    L.dx = c->d_dx; L.m_out = c->d_m + b0; L.nc_out = c->d_nc + b0; L.status = c->d_status;
    L.big_sg = c->d_big_sg ? c->d_big_sg + (size_t)b0 * bigwin_sg_doubles(c->G) : nullptr;
    L.big_wk = c->d_big_wk ? c->d_big_wk + (size_t)b0 * bigwin_wk_doubles() : nullptr;
    // Large windows (kernels_bigwin.hip): the part of the solve that needs the prior only - gauge reference, [Pdd; I], its Cholesky
    // sweep, the Pc copy: 8 of the chain's dependent launches, 0.12 ms alone - runs on a SECOND, higher-priority stream next to the
    // gate and the Gram kernel (round 5).  Measured per 32 filters at N = 807: in line 1.167 ms per step; forked before the gate
    // 1.134 (the sweep's launches crawl - 47 instead of 13 us each - and the gate loses 25 us, but the chain ends with the Gram
    // kernel); forked after the gate, under the Gram kernel only, 1.192.  Both hosts keep the register file full (the gate: 8 waves of
    // 231 VGPRs per CU, k_feat_gram_big: one workgroup of 8 waves at 256), so a sweep workgroup only gets a slot when a gate
    // workgroup retires - which the gate's 9600 short workgroups do all the time and the Gram kernel's 256 long ones never do.
    const bool big = c->d.c_max > 16;
    L.mstride = c->ystride; L.n_cap = c->d.n_max;
    L.marg_idx = marg_idx; L.marg_size = marg_size; L.pc_base = c->d_pcbase + b0;
    // the write-back flips the halves itself where its kernel can (k_info_apply); the caller asks c->apply_flipped before launch_post_marg
    c->apply_flipped = 0;
    L.flip_cnt = c->d_pcbase + c->d.batch + b0; L.did_flip = no_apply_flip() ? nullptr : &c->apply_flipped;
    // Order of ISSUE (round 5, single-filter latency): the fork point is recorded first (by the caller already when it has something to
    // run between the fork and the gate - the triangulation of ingvio_msckf_update_tri), then the main stream's gate and Gram launches,
    // and only then the eight launches of the side stream - issued first they kept the host busy for 24 us during which the gate could
    // not start (one filter, 27 clones: gate at +53 us after the frame's upload instead of +30).
    bool forked = false;
    if (big && phase == 0 && c->st2) {
        if (!c->fork_recorded) HIPCHK(c, hipEventRecord(c->ev_fork, c->run_st));      // after everything that wrote P on the main stream
        c->fork_recorded = false;
        forked = true;
    }
    if (phase != 2) {
        if (c->tok_wait) HIPCHK(c, hipStreamWaitEvent(c->run_st, c->tok_wait, 0));      // split frame step: one throughput segment at a time
        {
            // the gate's events ride on its dispatch packet (FactoredLaunch::prof_a / prof_b) instead of bracketing it
            const bool pon = c->prof && (c->prof_only < 0 || c->prof_only == PF_GATE2);
            int used = 0;
            if (pon) { hipEventCreate(&L.prof_a); hipEventCreate(&L.prof_b); L.prof_used = &used; }
            L.stage = 0;
            const int grc = launch_factored(L, c->run_st);
            if (pon) {
                if (used) c->recs.push_back({ PF_GATE2, L.prof_a, L.prof_b });
                else { hipEventDestroy(L.prof_a); hipEventDestroy(L.prof_b); }
                L.prof_a = nullptr; L.prof_b = nullptr; L.prof_used = nullptr;
            }
            if (grc) return INGVIO_E_UNSUPPORTED;
        }
        c->gram_red_last = 0; c->gram_form_last = 0;
        L.gram_red = frame_step && phase == 0 && c->gram_reduced; L.gram_was_red = &c->gram_red_last;
        L.gram_dec = c->gram_decoupled; L.gram_form = &c->gram_form_last;
        { ProfScope p(c, PF_GRAM); L.stage = 1; launch_factored(L, c->run_st); }
        L.gram_was_red = nullptr; L.gram_form = nullptr;
        if (c->tok_rec) HIPCHK(c, hipEventRecord(c->tok_rec, c->run_st));
    }
    if (forked) {
        // the side stream in two pieces: [A; b^T] of the main stream (stage 8) needs the gauge reference the set-up kernel picks, not the
        // sweep behind it - it runs while the sweep's last panels are still on their way (round 6)
        HIPCHK(c, hipStreamWaitEvent(c->st2, c->ev_fork, 0));
        L.stage = 6; launch_factored(L, c->st2);
        HIPCHK(c, hipEventRecord(c->ev_ref, c->st2));
        L.stage = 7; launch_factored(L, c->st2);
        HIPCHK(c, hipEventRecord(c->ev_join, c->st2));
    }
    if (phase == 1) return last_launch(c);
    if (forked) {
        ProfScope p(c, PF_INFO);
        HIPCHK(c, hipStreamWaitEvent(c->run_st, c->ev_ref, 0));
        L.stage = 8; launch_factored(L, c->run_st);
        HIPCHK(c, hipStreamWaitEvent(c->run_st, c->ev_join, 0));
        L.stage = 9; launch_factored(L, c->run_st);
    } else {
        if (big) { ProfScope p(c, PF_INFO); L.stage = 5; launch_factored(L, c->run_st); }      // split step / no side stream: in line
        { ProfScope p(c, PF_INFO); L.stage = 2; launch_factored(L, c->run_st); }
    }
    if (gnss_fuse) { if (int rc = gnss_in_frame_launch(c, b0, nb, L)) return rc; }
    if (phase == 2 && c->tok_wait) HIPCHK(c, hipStreamWaitEvent(c->run_st, c->tok_wait, 0));
    c->apply_form_last = 0;
    L.apply_res = frame_step && phase == 0 && c->apply_resident; L.apply_form = &c->apply_form_last;
    { ProfScope p(c, PF_APPLY); L.stage = 3; launch_factored(L, c->run_st); }
    if (phase == 2 && c->tok_rec) HIPCHK(c, hipEventRecord(c->tok_rec, c->run_st));
    return last_launch(c);
}

int run_msckf(ingvio_ctx* c, int b0, int nb, const MsckfOpts& op, int stereo, int fmax_used)
{
    if (c->method == 1) return run_msckf_factored(c, b0, nb, op, stereo, fmax_used);
    c->gram_red_last = 0; c->gram_form_last = 0;
    MsckfLaunch L;
    memset(&L, 0, sizeof L);
    L.stereo = stereo; L.cv = view(c); L.fv = fview(c); L.op = op; L.b0 = b0; L.nb = nb;
    L.fmax_used = fmax_used > 0 ? fmax_used : 1;
    L.gamma = c->d_gamma; L.accept = c->d_accept; L.used = c->d_used;
    L.Rpart = c->d_Rpart + (size_t)b0 * c->G * c->rstride; L.chunk_used = c->d_chunk_used + (size_t)b0 * c->G;
    L.G = c->G; L.rstride = c->rstride;
    L.Hout = c->d_H + (size_t)b0 * c->hstride; L.res_out = c->d_res + (size_t)b0 * c->mld;
    L.colmap = c->d_colmap + (size_t)b0 * c->cstride; L.m_out = c->d_m + b0; L.nc_out = c->d_nc + b0;
    L.mld = c->mld; L.hstride = c->hstride; L.cstride = c->cstride;
    { ProfScope p(c, PF_GATE); L.stage = 0; if (launch_msckf(L, c->st)) return INGVIO_E_UNSUPPORTED; }
    { ProfScope p(c, PF_FOLD); L.stage = 1; launch_msckf(L, c->st); }
    { ProfScope p(c, PF_MERGE); L.stage = 2; launch_msckf(L, c->st); }
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = view(c); E.b0 = b0; E.nb = nb; E.H = L.Hout; E.res = L.res_out; E.colmap = L.colmap; E.m = L.m_out; E.nc = L.nc_out;
    E.noise = c->d_noise + b0; E.r_kind = 0; E.mld = c->mld; E.hstride = c->hstride; E.cstride = c->cstride; E.nstride = 1;
    E.Y = c->d_Y + (size_t)b0 * c->ystride; E.ystride = c->ystride; E.dx = c->d_dx; E.status = c->d_status;
    E.m_cap = 6 * c->d.c_max; E.nc_cap = 6 * c->d.c_max;
    { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->st); }
    { ProfScope p(c, PF_DOWNDATE); launch_downdate(E, c->d.n_max, c->st); }
    return last_launch(c);
}

int fill_noise_scalar(ingvio_ctx* c, int b0, int nb, double var)
{
    auto& u = c->upc;
    if (u.noise_ok && u.b0 == b0 && u.nb == nb && u.var == var) return 0;                           // already there
    std::vector<double> v(nb, var);
    const UpItem item = { c->d_noise + b0, v.data(), 8 * (size_t)nb };
    if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
    u.noise_ok = true; u.b0 = b0; u.nb = nb; u.var = var;
    return 0;
}

// Per-filter IMU parameters of the staged frame.  Filter b propagates k_b steps from its own slot of d_Phi / d_G / d_dt (b * KMAX steps
// in: partial stages never touch another filter's steps) with its own sigma / sigma_cb / sigma_rw, held in d_prm [b][8] and mirrored on
// the host (st_prm).  A stage sets them for the filters it stages; the first stage after creation or after a failed stage sets them for
// every filter (k and noise of its first step for the filters it does not stage).  Packs the blocks to upload into `blk` and returns
// their first filter; *count = their number.
template <class Step>
int stage_imu_params(ingvio_ctx* c, int b0, int nb, const Step* steps, const double sigma[4], double scb, double srw, double* blk, int* count)
{
    const bool all = !c->staged;
    const int lo = all ? 0 : b0, hi = all ? c->d.batch : b0 + nb;
    for (int b = lo; b < hi; ++b) {
        double* h = &c->st_prm[(size_t)b * 8];
        h[0] = sigma[0]; h[1] = sigma[1]; h[2] = sigma[2]; h[3] = sigma[3]; h[4] = scb; h[5] = srw;
        h[6] = (double)steps[b >= b0 && b < b0 + nb ? b - b0 : 0].k; h[7] = 0.0;
        memcpy(blk + (size_t)(b - lo) * 8, h, 64);
    }
    *count = hi - lo;
    return lo;
}

// ---- staging a frame: the one sequence under ingvio_frame_stage(_async), ingvio_frame_stage_tracks and .._tracks_nominal ------------
//     refuse -> the form's validation -> begin -> the form's packing into the pinned slab -> commit -> the form's copies and launches,
//     upload_imu / upload_gate among them -> finish
// Nothing of the context changes before commit(): begin() only takes resources (the second input set, a pinned slab) and the slab is
// scratch, so the packing may still refuse.  From commit() on only HIP runtime errors can occur; they leave through fail(), which
// invalidates the staged frame.  Step: ingvio_frame_step or ingvio_frame_step_raw (k, gnss_idx, marg_idx).
struct FrameStage {
    ingvio_ctx* c; int b0, nb; const ingvio_msckf_opts* opts; const double* sigma; int enable_gnss; double scb, srw; bool async;
    Uploader upl{ c };
    // the refusals every form shares; inputs: the form's own pointers are there, tracks: the form needs the track store
    int refuse(bool inputs, bool tracks) const
    {
        if (phase_busy(c)) return INGVIO_E_ARG;
        if (c && c->nom.pending) { c->err = "a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
        if (check_range(c, b0, nb) || !inputs || !opts || !sigma) return INGVIO_E_ARG;
        if (tracks && !c->trk.t_max) { c->err = "ingvio_frame_stage_tracks without ingvio_tracks_create"; return INGVIO_E_ARG; }
        if (async && (b0 != 0 || nb != c->d.batch)) return INGVIO_E_ARG;      // a whole input set is replaced
        if (!opts->chi2_table || opts->chi2_len < 2 || opts->chi2_len > CHI2_CAP) return INGVIO_E_ARG;
        return 0;
    }
    // resources that may fail; bytes: the form's own share of the pinned slab
    int begin(size_t bytes)
    {
        if (async) if (int rc = prepare_async_set(c)) return rc;
        return upl.begin(bytes + pad64(8 * CHI2_CAP) + pad64(8 * (size_t)nb) + pad64(64 * (size_t)c->d.batch) + 1024);
    }
    int fail(int code)
    {
        hipStreamSynchronize(c->st);
        if (c->st_copy) hipStreamSynchronize(c->st_copy);
        c->staged = false; c->copy_pending = false;
        return code;
    }
    template <class Step>
    int commit(const Step* steps)
    {
        // new clock-state indices: the next restore is a full one (the strips the last step wrote are named by the OLD indices); a stage
        // with the same indices - every frame of a running filter between two GNSS initialisations - keeps the partial restore valid
        bool same = c->staged && enable_gnss == c->st_enable_gnss;
        for (int i = 0; i < nb; ++i)
            for (int g = 0; g < 5; ++g) {
                int& old = c->st_gnss[(size_t)(b0 + i) * 5 + g];
                if (old != steps[i].gnss_idx[g]) { same = false; old = steps[i].gnss_idx[g]; }
            }
        if (!same) c->strip_ok = false;
        // an earlier asynchronous stage into this set must land before it is overwritten in-stream
        if (!async) return wait_inputs(c) ? fail(INGVIO_E_HIP) : 0;
        // the set about to be overwritten was last read two frames ago; its "free" event is on the compute stream
        if (c->free_valid[c->set_id ^ 1] && hipStreamWaitEvent(c->st_copy, c->ev_free[c->set_id ^ 1], 0) != hipSuccess) return fail(INGVIO_E_HIP);
        swap_input_sets(c);
        upl.stream = c->st_copy;
        return 0;
    }
    // the filters' IMU parameter blocks (stage_imu_params)
    template <class Step>
    void upload_imu(const Step* steps)
    {
        double* prm = upl.take<double>(8 * (size_t)c->d.batch);
        int np = 0;
        const int p0 = stage_imu_params(c, b0, nb, steps, sigma, scb, srw, prm, &np);
        upl.copy(c->d_prm + (size_t)p0 * 8, prm, (size_t)np * 8);
    }
    // what the gate takes from the options: the chi-square table, the filters' measurement noise, st_op
    void upload_gate()
    {
        double* chi2 = upl.take<double>(CHI2_CAP); double* nz = upl.take<double>(nb);
        memcpy(chi2, opts->chi2_table, 8 * (size_t)opts->chi2_len);
        fill_opts(c, opts, &c->st_op);
        for (int i = 0; i < nb; ++i) nz[i] = c->st_op.var;
        upl.copy(c->d_chi2, chi2, (size_t)opts->chi2_len);
        upl.copy(c->d_noise + b0, nz, (size_t)nb);
        c->upc.chi2_ok = false; c->upc.noise_ok = false;
    }
    // Frame: ingvio_msckf_frame or ingvio_track_frame (n_clones, clone_idx); fmx: the call's largest feature count; plan: as
    // frame_stage_tracks_impl takes it; upd: the update-only frame from the table (no clone joins the mirror)
    template <class Step, class Frame>
    int finish(const Step* steps, const Frame* frames, int fmx, const int* plan = nullptr, bool upd = false)
    {
        if (int rc = upl.end()) return fail(rc);
        if (async) {
            if (hipEventRecord(c->ev_copy, c->st_copy) != hipSuccess) return fail(INGVIO_E_HIP);
            c->copy_pending = true;
        }
        for (int i = 0; i < nb; ++i) {
            c->st_marg[b0 + i] = steps[i].marg_idx;
            int hi = -1;
            if (plan) hi = plan[4 * i + 1];
            else for (int q = 0; q < frames[i].n_clones; ++q) if (frames[i].clone_idx[q] > hi) hi = frames[i].clone_idx[q];
            c->st_cidx_hi[b0 + i] = hi;
            c->h_nclones[b0 + i] = frames[i].n_clones;
        }
        if (plan) {                                   // the mirror follows what k_imu_steps<true> writes
            for (int i = 0; i < nb && !upd; ++i) {
                int* I = &c->nom.h_ih[(size_t)(b0 + i) * c->nom.ir];
                const int slot = plan[4 * i], ncl = plan[4 * i + 2];
                int* vc = I + NOM_IH + 4 * slot;
                vc[0] = NOM_KIND_SE3; vc[1] = plan[4 * i + 1]; vc[2] = -1; vc[3] = 0;
                I[NOM_CLONES + ncl - 1] = slot; I[NOM_N_CLONES] = ncl; I[NOM_N_VAR] = plan[4 * i + 3];
            }
            c->nom.pending = true;
        }
        c->nom.frame = plan != nullptr;                // a frame from the table is followed by the post-frame step
        c->nom.noprop = upd; c->nom.tri_on = false; c->nom.tri_staged = false;
        c->st_stereo = opts->stereo; c->st_enable_gnss = enable_gnss;
        if (!c->staged || fmx > c->st_fmax_used) c->st_fmax_used = fmx;
        c->staged = true;
        return INGVIO_OK;
    }
};

}  // namespace

extern "C" {

int ingvio_ctx_create(const ingvio_ctx_desc* desc, ingvio_ctx** out)
{
    if (!desc || !out || desc->batch < 1 || desc->n_max < 21 || desc->c_max < 1 || desc->f_max < 1) return INGVIO_E_ARG;
    if (desc->c_max > bigwin_cmax()) return INGVIO_E_CAPACITY;      // 17..36 clones: factored path only (kernels_bigwin.hip)
    if (desc->m_max > 128) return INGVIO_E_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= desc->device) return INGVIO_E_HIP;
    ingvio_ctx* c = new ingvio_ctx();
    c->d = *desc;
    if (c->d.m_max < 1) c->d.m_max = 32;
    c->err.clear();
    if (hipSetDevice(desc->device) != hipSuccess) { delete c; return INGVIO_E_HIP; }
    c->own_stream = desc->stream == nullptr;
    if (c->own_stream) {
        if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) { delete c; return INGVIO_E_HIP; }
    } else c->st = (hipStream_t)desc->stream;
    c->run_st = c->st;
    if (const char* e = getenv("INGVIO_FRAME_PARTS")) c->parts_req = atoi(e);
    if (const char* e = getenv("INGVIO_GRAM_REDUCED")) c->gram_reduced = atoi(e) != 0;      // A/B timing of an unchanged program
    if (const char* e = getenv("INGVIO_GRAM_DECOUPLED")) c->gram_decoupled = atoi(e) != 0;
    if (const char* e = getenv("INGVIO_APPLY_RESIDENT")) c->apply_resident = atoi(e) != 0;
    if (desc->c_max > 16) {
        // a higher priority than the compute stream's default: its short dependent launches take the slots the gate's workgroups free
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&c->st2, hipStreamNonBlocking, hi) != hipSuccess) c->st2 = nullptr;
        if (c->st2 && (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
                       hipEventCreateWithFlags(&c->ev_ref, hipEventDisableTiming) != hipSuccess ||
                       hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)) { hipStreamDestroy(c->st2); c->st2 = nullptr; }
    }
    const int B = desc->batch;
    c->ldp = (desc->n_max + 15) & ~15;
    // the factored kernels run at the padded width of their window class (6 / 11 / 16 clones): size the row/column
    // workspaces (M, the Pc copy) for the class, not for c_max itself
    const int cls0 = desc->c_max > 16 ? bigwin_cmax() : msckf_cmax_class(desc->c_max);
    const int cpad = cls0 > desc->c_max ? cls0 : desc->c_max;
    const int mcap = c->d.m_max > 6 * cpad ? c->d.m_max : 6 * cpad;
    c->mld = (mcap + 15) & ~15;
    // column capacity of a generic update (var_order may name any part of the state: 15 + 6 C + 3 L columns for the
    // landmark stack, LandmarkUpdate.cpp:32-149) is bounded by the state dimension, NOT by the row capacity m_max
    c->nc_cap = c->ldp > mcap ? c->ldp : mcap;
    c->G = (desc->c_max > 16 ? 256 : 512) / B;                              // ~2 resident gram workgroups per CU (large windows: 1,
    { const int gmax = desc->c_max > 16 ? 32 : 16; if (c->G > gmax) c->G = gmax; }   // and every chunk costs a 0.35 MB partial + sparse sums)
    if (c->G < 1) c->G = 1;
#ifdef INGVIO_ALT_KERNELS      // tuning knobs and forced code paths exist in variant builds only (tools/build_variant.sh alt -DINGVIO_ALT_KERNELS)
    if (const char* e = getenv("INGVIO_GRAM_CHUNKS")) { const int g = atoi(e); if (g >= 1 && g <= 64) c->G = g; }
#endif
    c->cls = msckf_cmax_class(desc->c_max);
    const int ncm = 6 * desc->c_max;
    c->rstride = ncm * (ncm + 1);
    c->hstride = c->mld * c->nc_cap;
    c->cstride = c->nc_cap;
    c->ystride = std::max(c->ldp * (c->mld + 4), c->mld * (c->mld + 1));      // Pc copy (ldp x MP) or M | t (MP x MP + MP)
    c->has_snap = false; c->staged = false; c->prof = false;
    c->method = 1;                                                          // information form; ingvio_set_msckf_method(0) selects the literal dense path
#ifdef INGVIO_ALT_KERNELS
    if (const char* e = getenv("INGVIO_MSCKF_METHOD")) c->method = (!strcmp(e, "dense") || !strcmp(e, "0")) ? 0 : 1;
#endif
    memset(c->prof_ms, 0, sizeof c->prof_ms); memset(c->prof_calls, 0, sizeof c->prof_calls);
    c->h_n.assign(B, 0); c->h_cur.assign(B, 0); c->h_n_snap.assign(B, 0); c->st_marg.assign(B, -1); c->st_cidx_hi.assign(B, -1); c->st_gnss.assign((size_t)B * 5, -2);
    c->st_prm.assign((size_t)B * 8, 0.0);
    c->h_nclones.assign(B, desc->c_max);
    // Consecutive filters' covariances must not sit a power of two apart: with ldp = 256 the stride would be 512 KB, and the SAME
    // element of every filter (the window block P_cc every gate wave of a filter reads, 64 filters per XCD) would fall into the same
    // L2 sets.  67 cache lines of pad walk the filters through the sets.  (Precaution: one default bench run showed the gate at
    // 1.30 ms instead of 0.28 in its config-3 pass; tools/gpu_alloc_sensitivity.py could not reproduce that with either layout -
    // six contexts per process, perturbed allocations, 0.289 - 0.294 ms for both -, so the pad is not the proven cure.)
#ifdef INGVIO_ALT_KERNELS
    static const bool no_pad = [] { const char* e = getenv("INGVIO_P_PAD"); return e && e[0] == '0'; }();
#else
    constexpr bool no_pad = false;
#endif
    c->pp = (size_t)c->ldp * c->ldp + (no_pad ? 0 : 67 * 16);
    const size_t pp = c->pp;
    const int cm = desc->c_max, fm = desc->f_max;
    int rc = 0;
    rc |= dalloc(c, &c->Pbase, 2 * (size_t)B * pp);
    rc |= dalloc(c, &c->Psnap, (size_t)B * pp);
    rc |= dalloc(c, &c->d_cur, B); rc |= dalloc(c, &c->d_n, B); rc |= dalloc(c, &c->d_n_snap, B);
    rc |= dalloc(c, &c->d_Phi, (size_t)B * KMAX * 225); rc |= dalloc(c, &c->d_G, (size_t)B * KMAX * 180);
    rc |= dalloc(c, &c->d_dt, (size_t)B * KMAX); rc |= dalloc(c, &c->d_R, (size_t)B * 9);
    rc |= dalloc(c, &c->d_blk, (size_t)B * 36); rc |= dalloc(c, &c->d_gnss, (size_t)B * 5); rc |= dalloc(c, &c->d_idx, B);
    rc |= dalloc(c, &c->d_prm, (size_t)B * 8);
    rc |= dalloc(c, &c->d_zero_idx, B);
    if (!rc && hipMemset(c->d_zero_idx, 0, sizeof(int) * (size_t)B) != hipSuccess) rc = 1;
    {
        FrameSlabPtrs q;
        if (frame_slab_alloc(c, &c->d_frame_slab[0], &q)) rc |= 1;
        else {
            c->d_clone_idx = q.clone_idx; c->d_nclones = q.nclones; c->d_nfeat = q.nfeat; c->d_anchor = q.anchor; c->d_dof = q.dof;
            c->d_clone_R = q.clone_R; c->d_clone_p = q.clone_p; c->d_pf = q.pf; c->d_uv = q.uv; c->d_mask = q.mask;
        }
    }
    rc |= dalloc(c, &c->d_chi2, CHI2_CAP);
    {
        // the results an update call hands back - dx, gamma, used flags, row count, status - sit in ONE device slab (and a pinned
        // mirror): a whole-batch fetch is one device-to-host copy instead of five (~18 us each for a single filter)
        const size_t o_dx = 0, o_gam = pad64(8 * (size_t)B * c->ldp), o_used = o_gam + pad64(8 * (size_t)B * fm), o_m = o_used + pad64(4 * (size_t)B * fm),
                     o_st = o_m + pad64(4 * (size_t)B), o_tok = o_st + pad64(4 * (size_t)B), o_tpf = o_tok + pad64(4 * (size_t)B * fm),
                     tot = o_tpf + pad64(8 * (size_t)B * fm * 3);
        if (dalloc(c, &c->d_result_slab, tot) || hipHostMalloc((void**)&c->h_result, tot, hipHostMallocDefault) != hipSuccess) rc |= 1;
        else {
            c->result_bytes = tot; c->ro_gam = o_gam; c->ro_used = o_used; c->ro_m = o_m; c->ro_st = o_st; c->ro_tok = o_tok; c->ro_tpf = o_tpf;
            c->d_dx = (double*)(c->d_result_slab + o_dx); c->d_gamma = (double*)(c->d_result_slab + o_gam);
            c->d_used = (int*)(c->d_result_slab + o_used); c->d_m = (int*)(c->d_result_slab + o_m); c->d_status = (int*)(c->d_result_slab + o_st);
        }
    }
    rc |= dalloc(c, &c->d_accept, (size_t)B * fm);
    rc |= dalloc(c, &c->d_Rpart, (size_t)B * c->G * c->rstride); rc |= dalloc(c, &c->d_chunk_used, (size_t)B * c->G);
    rc |= dalloc(c, &c->d_H, (size_t)B * c->hstride); rc |= dalloc(c, &c->d_res, (size_t)B * c->mld);
    rc |= dalloc(c, &c->d_colmap, (size_t)B * c->cstride); rc |= dalloc(c, &c->d_nc, B); rc |= dalloc(c, &c->d_pcbase, 2 * (size_t)B);      // [B] pc_base | [B] arrival counters of the fused flip (k_info_apply)
    rc |= dalloc(c, &c->d_tri_ok, (size_t)B * fm);
    rc |= dalloc(c, &c->d_imu, (size_t)IMU_SLAB_NB * (8 * (size_t)KMAX * (225 + 180 + 1) + 64) + 256);
    if (desc->c_max <= 16) rc |= dalloc(c, &c->d_Tflat, (size_t)std::min(B, APPLY_FLAT_NB) * c->ldp * 100);
    if (desc->c_max <= 16 && c->G > 1) { rc |= dalloc(c, &c->d_Asum, (size_t)B * c->rstride); rc |= dalloc(c, &c->d_used_sum, B); }
    c->d_big_sg = nullptr; c->d_big_wk = nullptr;
    if (desc->c_max > 16) {
        rc |= dalloc(c, &c->d_big_sg, (size_t)B * bigwin_sg_doubles(c->G)); rc |= dalloc(c, &c->d_big_wk, (size_t)B * bigwin_wk_doubles());
    }
    rc |= dalloc(c, &c->d_noise, B); rc |= dalloc(c, &c->d_noise1, (size_t)c->mld * c->mld);
    rc |= dalloc(c, &c->d_hnew, (size_t)c->mld * 6);
    rc |= dalloc(c, &c->d_Y, (size_t)B * c->ystride); rc |= dalloc(c, &c->d_Yc, (size_t)B * c->ystride);
    rc |= dalloc(c, &c->d_rec, (size_t)B * fm * factored_rec_size(desc->c_max));
    if (rc || hipStreamSynchronize(c->st) != hipSuccess) { *out = c; return INGVIO_E_HIP; }
    *out = c;
    return INGVIO_OK;
}

int ingvio_ctx_destroy(ingvio_ctx* c)
{
    if (!c) return INGVIO_E_ARG;
    for (int p = 0; p < c->parts_alloc; ++p) hipStreamSynchronize(c->part[p].st);
    hipStreamSynchronize(c->st);
    void* ptrs[] = { c->Pbase, c->Psnap, c->d_cur, c->d_n, c->d_n_snap, c->d_Phi, c->d_G, c->d_dt, c->d_R, c->d_blk, c->d_gnss,
                     c->d_idx, c->d_frame_slab[0], c->d_frame_slab[1],
                     c->d_chi2, c->d_result_slab, c->d_accept, c->d_Rpart, c->d_chunk_used,
                     c->d_H, c->d_res, c->d_colmap, c->d_nc, c->d_noise, c->d_noise1, c->d_Y, c->d_Yc, c->d_rec, c->d_pcbase, c->d_big_sg, c->d_big_wk, c->d_tri_ok, c->d_hnew, c->d_multi, c->d_noiseB,
                     c->gn.H, c->gn.res, c->gn.noise, c->gn.gamma, c->gn.chi2, c->gn.m, c->gn.nc, c->gn.colmap, c->gn.keep,
                     c->gn.feph, c->gn.fobs, c->gn.frcv, c->gn.front, c->gn.stf,
                     c->dw.Hd, c->dw.X, c->dw.Y, c->dw.Tb, c->dw.noise, c->dw.noiseB, c->dw.m, c->dw.cidx, c->lm.pose, c->lm.pf, c->lm.uv, c->lm.gamma, c->lm.idx, c->lm.n_lm,
                     c->lm.lm_idx, c->lm.anchor_idx, c->lm.tracked, c->lm.accept, c->lm.slot, c->lm.dx, c->d_xchg, c->dw.U, c->dw.rowmap, c->d_zero_idx,
                     c->d_Asum, c->d_used_sum, c->d_Tflat, c->d_imu, c->d_tri_mask, c->d_prm };
    for (void* p : ptrs) if (p) hipFree(p);
    c->dl.release(); c->tl.release(); c->od.release(); c->nom.release();
    for (auto& sl : c->pin) { if (sl.p) hipHostFree(sl.p); if (sl.ev) hipEventDestroy(sl.ev); }
    if (c->h_result) hipHostFree(c->h_result);
    if (c->qr.exec) hipGraphExecDestroy(c->qr.exec);
    for (double* p : { c->qr.dA, c->qr.db, c->qr.ws, c->qr.dT, c->se.e, c->se.o, c->se.r, c->se.f, c->gn.W, c->gn.Yf, c->gn.dxf }) if (p) hipFree(p);
    for (int* p : { c->gn.mf, c->gn.ncf }) if (p) hipFree(p);
    {
        auto& a = c->alt;
        void* ap[] = { a.Phi, a.G, a.dt, a.R, a.gnss, a.idx, a.chi2, a.noise, a.prm };      // its frame arrays: d_frame_slab (freed above)
        for (void* p : ap) if (p) hipFree(p);
        if (c->st_copy) hipStreamDestroy(c->st_copy);
        if (c->ev_copy) hipEventDestroy(c->ev_copy);
        for (auto e : c->ev_free) if (e) hipEventDestroy(e);
    }
    for (void* p : { (void*)c->trk.uv, (void*)c->trk.pf, (void*)c->trk.mask, (void*)c->trk.has, (void*)c->trk.stage[0], (void*)c->trk.stage[1] }) if (p) hipFree(p);
    c->mt.release();
    for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (int p = 0; p < c->parts_alloc; ++p) { hipStreamDestroy(c->part[p].st); hipEventDestroy(c->part[p].ev_gate); hipEventDestroy(c->part[p].ev_apply); hipEventDestroy(c->part[p].ev_done); }
    if (c->ev_split_fork) hipEventDestroy(c->ev_split_fork);
    if (c->ev_fetch) hipEventDestroy(c->ev_fetch);
    if (c->st2) hipStreamDestroy(c->st2);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->ev_ref) hipEventDestroy(c->ev_ref);
    if (c->own_stream) hipStreamDestroy(c->st);
    delete c;
    return INGVIO_OK;
}

int ingvio_sync(ingvio_ctx* c)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return INGVIO_OK;
}
void* ingvio_ctx_stream(ingvio_ctx* c)
{
    if (c && c->split_pending) join_parts(c);      // the caller orders its own work behind this stream
    return c ? (void*)c->st : nullptr;
}
const char* ingvio_last_error(ingvio_ctx* c) { return c ? c->err.c_str() : "null context"; }
int ingvio_ldp(ingvio_ctx* c) { return c ? c->ldp : 0; }
int ingvio_f_max(ingvio_ctx* c) { return c ? c->d.f_max : 0; }
int ingvio_c_max(ingvio_ctx* c) { return c ? c->d.c_max : 0; }

int ingvio_cov_set(ingvio_ctx* c, int b, const double* P, int ld, int n)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b, 1) || !P || n < 0 || n > c->d.n_max || ld < n) return INGVIO_E_ARG;
    double* dst = c->Pbase + ((size_t)c->h_cur[b] * c->d.batch + b) * c->pp;
    if (n) HIPCHK(c, hipMemcpy2DAsync(dst, 8 * (size_t)c->ldp, P, 8 * (size_t)ld, 8 * (size_t)n, n, hipMemcpyHostToDevice, c->st));
    c->h_n[b] = n;
    HIPCHK(c, hipMemcpyAsync(c->d_n + b, &c->h_n[b], sizeof(int), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return INGVIO_OK;
}

int ingvio_cov_get(ingvio_ctx* c, int b, double* P, int ld)
{
    ENTER(c);
    if (check_range(c, b, 1) || !P) return INGVIO_E_ARG;
    const int n = c->h_n[b];
    if (ld < n) return INGVIO_E_ARG;
    const double* src = c->Pbase + ((size_t)c->h_cur[b] * c->d.batch + b) * c->pp;
    if (n) HIPCHK(c, hipMemcpy2DAsync(P, 8 * (size_t)ld, src, 8 * (size_t)c->ldp, 8 * (size_t)n, n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipGetLastError());
    return INGVIO_OK;
}

int ingvio_get_n(ingvio_ctx* c, int b, int* n)
{
    ENTER(c);
    if (check_range(c, b, 1) || !n) return INGVIO_E_ARG;
    *n = c->h_n[b];
    return INGVIO_OK;
}

int ingvio_cov_get_marginal(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, double* out)
{
    ENTER(c);
    if (check_range(c, b, 1) || !vidx || !vsize || !out || k < 1) return INGVIO_E_ARG;
    const int n = c->h_n[b];
    std::vector<double> P((size_t)n * n);
    int rc = ingvio_cov_get(c, b, P.data(), n);
    if (rc) return rc;
    int ns = 0;
    for (int i = 0; i < k; ++i) { if (vidx[i] < 0 || vidx[i] + vsize[i] > n) return INGVIO_E_NOT_IN_STATE; ns += vsize[i]; }
    int r0 = 0;
    for (int a = 0; a < k; ++a) {
        int c0 = 0;
        for (int bb = 0; bb < k; ++bb) {
            for (int j = 0; j < vsize[bb]; ++j) for (int i = 0; i < vsize[a]; ++i)
                out[(size_t)(c0 + j) * ns + r0 + i] = P[(size_t)(vidx[bb] + j) * n + vidx[a] + i];
            c0 += vsize[bb];
        }
        r0 += vsize[a];
    }
    return INGVIO_OK;
}

int ingvio_cov_get_marginal_batch(ingvio_ctx* c, int b0, int nb, const int* vidx, const int* vsize, int k, int ns_max, double* out)
{
    if (check_range(c, b0, nb) || !vidx || !vsize || !out || k < 1 || ns_max < 1 || ns_max > INGVIO_MARGINAL_NS_MAX) return INGVIO_E_ARG;
    std::vector<int> cols((size_t)nb * ns_max, -1), ns((size_t)nb, 0);
    for (int i = 0; i < nb; ++i) {                                     // every filter is checked before anything is enqueued or written
        const int n = c->h_n[b0 + i];
        int w = 0;
        for (int a = 0; a < k; ++a) {
            const int v0 = vidx[(size_t)i * k + a], sz = vsize[(size_t)i * k + a];
            if (sz < 0) return INGVIO_E_ARG;
            if (sz == 0) continue;
            if (v0 < 0 || v0 + sz > n) return INGVIO_E_NOT_IN_STATE;
            if (w + sz > ns_max) return INGVIO_E_ARG;
            for (int j = 0; j < sz; ++j) cols[(size_t)i * ns_max + w++] = v0 + j;
        }
        ns[i] = w;
    }
    ENTER(c);
    auto& o = c->od;
    const size_t nblk = (size_t)nb * ns_max * ns_max;
    if (o.cols_cap < cols.size()) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (o.cols) hipFree(o.cols);
        if (o.ns) hipFree(o.ns);
        o.cols = nullptr; o.ns = nullptr; o.cols_cap = 0;
        HIPCHK(c, hipMalloc((void**)&o.cols, sizeof(int) * cols.size()));
        HIPCHK(c, hipMalloc((void**)&o.ns, sizeof(int) * cols.size()));
        o.cols_cap = cols.size();
    }
    if (o.blk_cap < nblk) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (o.blk) hipFree(o.blk);
        o.blk = nullptr; o.blk_cap = 0;
        HIPCHK(c, hipMalloc((void**)&o.blk, 8 * nblk));
        o.blk_cap = nblk;
    }
    if (up(c, o.cols, cols.data(), sizeof(int) * cols.size()) || up(c, o.ns, ns.data(), sizeof(int) * ns.size())) return INGVIO_E_HIP;
    launch_cov_marginal(view_ro(c), o.cols, o.ns, ns_max, o.blk, b0, nb, c->st);
    if (int rc = last_launch(c)) return rc;
    std::vector<double> blk(nblk);
    if (down_sync(c, blk.data(), o.blk, 8 * nblk)) return INGVIO_E_HIP;      // the blocks alone, one synchronisation
    for (int i = 0; i < nb; ++i)
        memcpy(out + (size_t)i * ns_max * ns_max, blk.data() + (size_t)i * ns_max * ns_max, 8 * (size_t)ns[i] * ns[i]);
    return INGVIO_OK;
}

int ingvio_cov_snapshot(ingvio_ctx* c)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (!c) return INGVIO_E_ARG;
    if (c->nom.pending) { c->err = "ingvio_cov_snapshot: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_cov_snapshot")) return INGVIO_E_ARG;
    launch_snapshot(view(c), c->d.n_max, c->Psnap, c->d_n_snap, c->st);
    c->h_n_snap = c->h_n;
    c->has_snap = true;
    if (c->nom.vmax) {                             // the nominal table travels with the covariance (device to device, same stream)
        auto& m = c->nom;
        HIPCHK(c, hipMemcpyAsync(m.ih_snap, m.ih, sizeof(int) * (size_t)c->d.batch * m.ir, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(m.dv_snap, m.dv, sizeof(double) * (size_t)c->d.batch * m.dr, hipMemcpyDeviceToDevice, c->st));
        m.h_ih_snap = m.h_ih;
        m.has_snap = true;
        if (nom_mark(c)) return INGVIO_E_HIP;
    }
    return last_launch(c);
}

int ingvio_cov_restore(ingvio_ctx* c)
{
    ENTER(c);
    if (!c || !c->has_snap) return INGVIO_E_ARG;
    if (c->nom.vmax && !c->nom.has_snap) {
        c->err = "ingvio_cov_restore: the snapshot was taken before ingvio_nominal_create and holds no nominal table";
        return INGVIO_E_ARG;
    }
    c->phase_pending = false;                      // the way out of an abandoned split step: every filter returns to the snapshot
    launch_restore(view(c), 0, c->d.batch, c->d.n_max, c->Psnap, c->d_n_snap, c->st);
    c->h_n = c->h_n_snap;
    std::fill(c->h_cur.begin(), c->h_cur.end(), 0);
    if (c->nom.vmax && c->nom.has_snap) {
        auto& m = c->nom;
        if (m.pending) { c->staged = false; m.pending = false; }      // the staged frame's clone is not in the restored table
        m.frame = false;
        if (c->gn.nom_pending) { c->gn.nom_pending = false; c->gn.staged = false; }      // rows linearised at the abandoned table
        if (c->gn.frame_nom) { c->gn.frame_nom = false; c->gn.in_frame = false; c->gn.staged = false; }      // the epoch of the abandoned frame
        if (c->lm.nominal && c->lm.staged) { c->lm.nom_pending = false; c->lm.staged = false; }      // either form: its slots name the abandoned table
        if (wait_inputs(c)) return INGVIO_E_HIP;                     // an asynchronous stage from the table must land before it is overwritten
        HIPCHK(c, hipMemcpyAsync(m.ih, m.ih_snap, sizeof(int) * (size_t)c->d.batch * m.ir, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(m.dv, m.dv_snap, sizeof(double) * (size_t)c->d.batch * m.dr, hipMemcpyDeviceToDevice, c->st));
        m.h_ih = m.h_ih_snap;
        if (nom_mark(c)) return INGVIO_E_HIP;
    }
    return last_launch(c);
}

int ingvio_propagate_fused(ingvio_ctx* c, int b0, int nb, int k, const double* Phi, const double* G, const double* dt,
                           const double sigma[4], int enable_gnss, const int* gnss_idx, double scb, double srw)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || k < 1 || k > KMAX || !Phi || !G || !dt || !sigma) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i) if (c->h_n[b0 + i] < 15) return INGVIO_E_ARG;
    if (wait_inputs(c)) return INGVIO_E_HIP;
    const bool with_gnss = enable_gnss && gnss_idx;
    if (c->d_imu && nb <= IMU_SLAB_NB) {
        // few filters: Phi | G | dt | gnss_idx packed into ONE pinned image and ONE copy into a device slab of the same layout (the four
        // arrays are four allocations, i.e. four copies of ~7 us each on the stream in front of the kernel - a third of what a single
        // filter's propagation costs its host)
        const size_t nPhi = (size_t)nb * k * 225, nG = (size_t)nb * k * 180, ndt = (size_t)nb * k;
        const size_t oG = 8 * nPhi, odt = oG + 8 * nG, ogn = pad64(odt + 8 * ndt), tot = ogn + (with_gnss ? sizeof(int) * (size_t)nb * 5 : 0);
        Uploader up{ c };
        if (up.begin(tot + 64)) return INGVIO_E_HIP;
        char* img = up.take<char>(tot);
        memcpy(img, Phi, 8 * nPhi); memcpy(img + oG, G, 8 * nG); memcpy(img + odt, dt, 8 * ndt);
        if (with_gnss) memcpy(img + ogn, gnss_idx, sizeof(int) * (size_t)nb * 5);
        up.copy(c->d_imu, img, tot);
        if (up.end()) return INGVIO_E_HIP;
        ProfScope p(c, PF_PROPAGATE);
        launch_propagate(view(c), b0, nb, c->d.n_max, (const double*)c->d_imu, (const double*)(c->d_imu + oG), (const double*)(c->d_imu + odt), k, k,
                         nullptr, with_gnss ? (const int*)(c->d_imu + ogn) : nullptr, sigma, enable_gnss, scb, srw, c->st);
        return last_launch(c);
    }
    const UpItem items[4] = { { c->d_Phi, Phi, 8 * (size_t)nb * k * 225 }, { c->d_G, G, 8 * (size_t)nb * k * 180 }, { c->d_dt, dt, 8 * (size_t)nb * k },
                              { c->d_gnss, gnss_idx, with_gnss ? sizeof(int) * (size_t)nb * 5 : 0 } };
    if (stage_small(c, items, 4)) return INGVIO_E_HIP;
    {
        ProfScope p(c, PF_PROPAGATE);
        launch_propagate(view(c), b0, nb, c->d.n_max, c->d_Phi, c->d_G, c->d_dt, k, k, nullptr, with_gnss ? c->d_gnss : nullptr,
                         sigma, enable_gnss, scb, srw, c->st);
    }
    return last_launch(c);                      // no stream synchronisation: the inputs were staged through the pinned ring (stage_small)
}

int ingvio_propagate(ingvio_ctx* c, int b0, int nb, const double* Phi, const double* G, const double* dt,
                     const double sigma[4], int enable_gnss, const int* gnss_idx, double scb, double srw)
{
    ENTER(c);
    return ingvio_propagate_fused(c, b0, nb, 1, Phi, G, dt, sigma, enable_gnss, gnss_idx, scb, srw);
}

int ingvio_augment_clone(ingvio_ctx* c, int b0, int nb, const double* R, int* new_idx)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !R) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i) {
        if (c->h_n[b0 + i] < 21) return INGVIO_E_ARG;
        if (c->h_n[b0 + i] + 6 > c->d.n_max) return INGVIO_E_CAPACITY;
    }
    if (wait_inputs(c)) return INGVIO_E_HIP;
    if (nb == 1) { ProfScope p(c, PF_AUGMENT); launch_augment_one(view(c), b0, R, c->st); }      // R as a kernel argument
    else {
        const UpItem item = { c->d_R, R, 8 * (size_t)nb * 9 };
        if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
        ProfScope p(c, PF_AUGMENT); launch_augment(view(c), b0, nb, c->d_R, c->st);
    }
    for (int i = 0; i < nb; ++i) { if (new_idx) new_idx[i] = c->h_n[b0 + i]; c->h_n[b0 + i] += 6; }
    return last_launch(c);
}

int ingvio_marginalize(ingvio_ctx* c, int b0, int nb, const int* idx, int size)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !idx || size < 1) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i)
        if (idx[i] >= 0 && idx[i] + size > c->h_n[b0 + i]) return INGVIO_E_NOT_IN_STATE;
    if (wait_inputs(c)) return INGVIO_E_HIP;
    if (nb == 1) { ProfScope p(c, PF_MARG); launch_marginalize(view(c), b0, 1, c->d.n_max, nullptr, size, c->st, idx[0]); }      // the index as a kernel argument
    else {
        const UpItem item = { c->d_idx, idx, sizeof(int) * (size_t)nb };
        if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
        ProfScope p(c, PF_MARG); launch_marginalize(view(c), b0, nb, c->d.n_max, c->d_idx, size, c->st);
    }
    for (int i = 0; i < nb; ++i) if (idx[i] >= 0) { c->h_n[b0 + i] -= size; c->h_cur[b0 + i] ^= 1; }
    return last_launch(c);
}

int ingvio_append_independent(ingvio_ctx* c, int b0, int nb, int size, const double* blk, int* new_idx)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !blk || size < 1 || size > 6) return INGVIO_E_ARG;
    for (int i = 0; i < nb; ++i) if (c->h_n[b0 + i] + size > c->d.n_max) return INGVIO_E_CAPACITY;
    if (wait_inputs(c)) return INGVIO_E_HIP;
    const UpItem item = { c->d_blk, blk, 8 * (size_t)nb * size * size };
    if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
    launch_append(view(c), b0, nb, size, c->d_blk, c->st);
    for (int i = 0; i < nb; ++i) { if (new_idx) new_idx[i] = c->h_n[b0 + i]; c->h_n[b0 + i] += size; }
    return last_launch(c);
}

static int dense_ws_alloc(ingvio_ctx* c, int m_need);
static int run_dense_update(ingvio_ctx* c, int b0, int nb, double var, int r_kind, const double* d_noise, int nstride, double* d_dx, bool products_done = false,
                            const int* rowmap = nullptr, const int* marg_idx = nullptr, int marg_size = 0, bool* marg_fused = nullptr);
#define DENSE_M_MAX 1024      // rows of one generic update through the dense-H route (S factorised out of HBM, kernels_chol.hip)

// ingvio_ekf_update for row counts whose S does not fit in LDS (or beyond the context's m_max): the host scatters the columns
// into the dense row layout of kernels_lmbatch.hip and the update runs as GEMM + Cholesky sweep + downdate.
static int ekf_update_dense_route(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H, int ldh, int m,
                                  const double* res, const double* R, int r_kind, double* dx_out)
{
    if (check_range(c, b, 1) || !vidx || !vsize || !H || !res || !R || k < 1 || m < 1 || ldh < m || r_kind < 0 || r_kind > 2) return INGVIO_E_ARG;
    if (m > DENSE_M_MAX) return INGVIO_E_CAPACITY;
    for (int i = 0; i < k; ++i) if (vidx[i] < 0 || vsize[i] < 0 || vidx[i] + vsize[i] > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;
    if (int rc = dense_ws_alloc(c, m)) return rc;
    auto& w = c->dw;
    std::vector<double> Hd((size_t)w.m_cap * w.n_ld, 0.0), rr((size_t)w.m_cap, 0.0);
    int col = 0;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < vsize[i]; ++j, ++col)
            for (int r = 0; r < m; ++r) Hd[(size_t)r * w.n_ld + vidx[i] + j] += H[(size_t)r + (size_t)col * ldh];
    memcpy(rr.data(), res, 8 * (size_t)m);
    int zero = 0, rc = up(c, w.Hd + (size_t)b * w.hstride, Hd.data(), 8 * Hd.size());
    if (hipMemcpy2DAsync(w.X + (size_t)b * w.xstride + w.m_cap + w.n32, 8 * (size_t)w.ldx, rr.data(), 8, 8, (size_t)w.m_cap, hipMemcpyHostToDevice, c->st) != hipSuccess) rc = INGVIO_E_HIP;
    rc |= up(c, w.m + b, &m, sizeof(int));
    rc |= up(c, w.noise, R, 8 * (size_t)(r_kind == 0 ? 1 : (r_kind == 1 ? m : (size_t)m * m)));
    rc |= up(c, c->d_status + b, &zero, sizeof(int));
    if (rc) return INGVIO_E_HIP;
    HIPCHK(c, hipStreamSynchronize(c->st));                                       // the host vectors go out of scope
    rc = run_dense_update(c, b, 1, 0.0, r_kind, w.noise, 0, c->d_dx);
    if (rc) return rc;
    int status = 0;
    if (dx_out && down_sync(c, dx_out, c->d_dx + (size_t)b * c->ldp, 8 * (size_t)c->h_n[b])) return INGVIO_E_HIP;
    if (down_sync(c, &status, c->d_status + b, sizeof(int))) return INGVIO_E_HIP;
    return soft_status(status);
}

int ingvio_ekf_update(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H, int ldh, int m,
                      const double* res, const double* R, int r_kind, double* dx_out)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    int nc = 0;
    if (c && vsize && k >= 1) {                                     // S beyond LDS / rows beyond m_max: the dense route
        int ncq = 0;
        for (int i = 0; i < k; ++i) ncq += vsize[i];
        if (m > c->mld || (m > c->d.m_max && m > 6 * c->d.c_max) || ncq > c->nc_cap || !ekf_core_fits(m, ncq))
            return ekf_update_dense_route(c, b, vidx, vsize, k, H, ldh, m, res, R, r_kind, dx_out);
    }
    int rc = stage_generic(c, b, vidx, vsize, k, H, ldh, m, res, R, r_kind, &nc);
    if (rc) return rc;
    if (!ekf_core_fits(m, nc)) return INGVIO_E_CAPACITY;          // before anything touches the covariance
    int zero = 0;
    if (up(c, c->d_status + b, &zero, sizeof(int))) return INGVIO_E_HIP;
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = view(c); E.b0 = b; E.nb = 1; E.H = c->d_H + (size_t)b * c->hstride; E.res = c->d_res + (size_t)b * c->mld;
    E.colmap = c->d_colmap + (size_t)b * c->cstride; E.m = c->d_m + b; E.nc = c->d_nc + b;
    E.noise = c->d_noise1; E.r_kind = r_kind; E.mld = c->mld; E.hstride = c->hstride; E.cstride = c->cstride;
    E.nstride = c->mld * c->mld; E.Y = c->d_Y + (size_t)b * c->ystride; E.ystride = c->ystride; E.dx = c->d_dx;
    E.status = c->d_status; E.m_cap = m; E.nc_cap = nc;
    { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->st); }
    { ProfScope p(c, PF_DOWNDATE); launch_downdate(E, c->h_n[b], c->st); }
    c->update_form_last = INGVIO_UPDATE_LDS;
    int status = 0;
    if (dx_out && down_sync(c, dx_out, c->d_dx + (size_t)b * c->ldp, 8 * (size_t)c->h_n[b])) return INGVIO_E_HIP;
    if (down_sync(c, &status, c->d_status + b, sizeof(int))) return INGVIO_E_HIP;
    rc = last_launch(c);
    if (rc) return rc;
    return soft_status(status);
}

// ekfUpdate for filters [b0, b0+nb) in one launch and one synchronisation (the GNSS update of a whole batch, config 3 x 4):
// block i = filter b0+i with its own var_order / H / res / noise (R scalar or diagonal).  dx_out [nb][ldp], status_out [nb]
// (INGVIO_OK / INGVIO_NEG_DIAG per filter, may be NULL).
int ingvio_ekf_update_batch(ingvio_ctx* c, int b0, int nb, const ingvio_update_block* blk, int r_kind, double* dx_out, int* status_out)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !blk) return INGVIO_E_ARG;
    if (r_kind != INGVIO_R_SCALAR && r_kind != INGVIO_R_DIAG) return INGVIO_E_UNSUPPORTED;
    int m_cap = 0, nc_cap = 0, n_cap = 0;
    bool dense = false;
    std::vector<int> ncs(nb);
    for (int i = 0; i < nb; ++i) {
        const ingvio_update_block& q = blk[i];
        const int b = b0 + i;
        if (!q.vidx || !q.vsize || !q.H || !q.res || !q.R || q.k < 1 || q.m < 1 || q.ldh < q.m) return INGVIO_E_ARG;
        if (q.m > DENSE_M_MAX) return INGVIO_E_CAPACITY;
        int nc = 0;
        for (int j = 0; j < q.k; ++j) {
            if (q.vidx[j] < 0 || q.vsize[j] < 0 || q.vidx[j] + q.vsize[j] > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;      // checkSubOrder
            nc += q.vsize[j];
        }
        if (q.m > c->mld || nc > c->nc_cap || !ekf_core_fits(q.m, nc)) dense = true;      // S beyond LDS: the whole call takes the dense-H route
        ncs[i] = nc;
        if (q.m > m_cap) m_cap = q.m;
        if (nc > nc_cap) nc_cap = nc;
        if (c->h_n[b] > n_cap) n_cap = c->h_n[b];
    }
    if (!ekf_core_fits(m_cap, nc_cap)) dense = true;      // one launch, its LDS sized by the most rows and the most columns of the call
    if (dense) {
        // GEMM + Cholesky sweep with carried rows + downdate on dense rows addressed by state column (kernels_lmbatch.hip /
        // kernels_chol.hip); the host scatters the columns, filter by filter
        if (int rc = dense_ws_alloc(c, m_cap)) return rc;
        auto& w = c->dw;
        std::vector<double> Hd((size_t)w.m_cap * w.n_ld), rr((size_t)w.m_cap), nz((size_t)w.m_cap);
        std::vector<int> zeros(nb, 0), ms(nb);
        int rc = 0;
        for (int i = 0; i < nb && !rc; ++i) {
            const ingvio_update_block& q = blk[i];
            std::fill(Hd.begin(), Hd.end(), 0.0); std::fill(rr.begin(), rr.end(), 0.0); std::fill(nz.begin(), nz.end(), 0.0);
            int col = 0;
            for (int j = 0; j < q.k; ++j)
                for (int t = 0; t < q.vsize[j]; ++t, ++col)
                    for (int r = 0; r < q.m; ++r) Hd[(size_t)r * w.n_ld + q.vidx[j] + t] += q.H[(size_t)r + (size_t)col * q.ldh];
            memcpy(rr.data(), q.res, 8 * (size_t)q.m);
            memcpy(nz.data(), q.R, 8 * (size_t)(r_kind == INGVIO_R_SCALAR ? 1 : q.m));
            ms[i] = q.m;
            rc |= up(c, w.Hd + (size_t)(b0 + i) * w.hstride, Hd.data(), 8 * Hd.size());
            if (hipMemcpy2DAsync(w.X + (size_t)(b0 + i) * w.xstride + w.m_cap + w.n32, 8 * (size_t)w.ldx, rr.data(), 8, 8, (size_t)w.m_cap,
                                 hipMemcpyHostToDevice, c->st) != hipSuccess) rc = INGVIO_E_HIP;
            rc |= up(c, w.noiseB + (size_t)(b0 + i) * w.m_cap, nz.data(), 8 * nz.size());
            if (!rc && hipStreamSynchronize(c->st) != hipSuccess) rc = INGVIO_E_HIP;      // the staging vectors are reused
        }
        rc |= up(c, w.m + b0, ms.data(), sizeof(int) * (size_t)nb);
        rc |= up(c, c->d_status + b0, zeros.data(), sizeof(int) * (size_t)nb);
        if (rc) return INGVIO_E_HIP;
        HIPCHK(c, hipStreamSynchronize(c->st));
        rc = run_dense_update(c, b0, nb, 0.0, r_kind, w.noiseB + (size_t)b0 * w.m_cap, w.m_cap, c->d_dx);
        if (rc) return rc;
        std::vector<int> status(nb, 0);
        if (dx_out) HIPCHK(c, hipMemcpyAsync(dx_out, c->d_dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
        if (down_sync(c, status.data(), c->d_status + b0, sizeof(int) * (size_t)nb)) return INGVIO_E_HIP;
        int soft = INGVIO_OK;
        for (int i = 0; i < nb; ++i) {
            const int st = soft_status(status[i]);
            if (status_out) status_out[i] = st;
            if (st != INGVIO_OK) soft = st;
        }
        return soft;
    }
    if (!c->d_noiseB) {
        if (dalloc(c, &c->d_noiseB, (size_t)c->d.batch * c->mld)) return INGVIO_E_HIP;
    }
    // compact strides for this call: only the widest var_order of the batch travels over PCIe (the d_H / d_colmap slots are
    // sized for nc_cap = ldp columns per filter, so the compact layout always fits)
    const size_t mld = c->mld, hs = (size_t)c->mld * nc_cap, cs = nc_cap;
    Uploader upl{ c };
    int rc = upl.begin(pad64(8 * (size_t)nb * hs) + pad64(8 * (size_t)nb * mld) * 2 + pad64(4 * (size_t)nb * cs) + pad64(4 * (size_t)nb) * 3 + 1024);
    if (rc) return rc;
    double* hH = upl.take<double>((size_t)nb * hs); double* hr = upl.take<double>((size_t)nb * mld); double* hn = upl.take<double>((size_t)nb * mld);
    int* hc = upl.take<int>((size_t)nb * cs); int* hm = upl.take<int>(nb); int* hnc = upl.take<int>(nb); int* hz = upl.take<int>(nb);
    parallel_for(nb, [=, &ncs](int i) {
        const ingvio_update_block& q = blk[i];
        const int nc = ncs[i];
        double* Hd = hH + (size_t)i * hs;
        for (int cc = 0; cc < nc; ++cc) {
            memcpy(Hd + (size_t)cc * mld, q.H + (size_t)cc * q.ldh, 8 * (size_t)q.m);
            memset(Hd + (size_t)cc * mld + q.m, 0, 8 * (mld - q.m));                              // k_ekf_core reads whole 16-row groups
        }
        memcpy(hr + (size_t)i * mld, q.res, 8 * (size_t)q.m);
        memcpy(hn + (size_t)i * mld, q.R, 8 * (size_t)(r_kind == INGVIO_R_SCALAR ? 1 : q.m));
        int* cm = hc + (size_t)i * cs;
        int w = 0;
        for (int j = 0; j < q.k; ++j) for (int t = 0; t < q.vsize[j]; ++t) cm[w++] = q.vidx[j] + t;
        hm[i] = q.m; hnc[i] = nc; hz[i] = 0;
    });
    upl.copy(c->d_H + (size_t)b0 * hs, hH, (size_t)nb * hs);
    upl.copy(c->d_res + (size_t)b0 * mld, hr, (size_t)nb * mld);
    upl.copy(c->d_noiseB + (size_t)b0 * mld, hn, (size_t)nb * mld);
    upl.copy(c->d_colmap + (size_t)b0 * cs, hc, (size_t)nb * cs);
    upl.copy(c->d_m + b0, hm, nb); upl.copy(c->d_nc + b0, hnc, nb); upl.copy(c->d_status + b0, hz, nb);
    rc = upl.end();
    if (rc) return rc;
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = view(c); E.b0 = b0; E.nb = nb; E.H = c->d_H + (size_t)b0 * hs; E.res = c->d_res + (size_t)b0 * mld;
    E.colmap = c->d_colmap + (size_t)b0 * cs; E.m = c->d_m + b0; E.nc = c->d_nc + b0;
    E.noise = c->d_noiseB + (size_t)b0 * mld; E.r_kind = r_kind; E.mld = c->mld; E.hstride = (int)hs; E.cstride = (int)cs;
    E.nstride = c->mld; E.Y = c->d_Y + (size_t)b0 * c->ystride; E.ystride = c->ystride; E.dx = c->d_dx;
    E.status = c->d_status; E.m_cap = m_cap; E.nc_cap = nc_cap;
    { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->st); }
    { ProfScope p(c, PF_DOWNDATE); launch_downdate(E, n_cap, c->st); }
    c->update_form_last = INGVIO_UPDATE_LDS;
    std::vector<int> status(nb, 0);
    if (dx_out) HIPCHK(c, hipMemcpyAsync(dx_out, c->d_dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
    if (down_sync(c, status.data(), c->d_status + b0, sizeof(int) * (size_t)nb)) return INGVIO_E_HIP;
    rc = last_launch(c);
    if (rc) return rc;
    int soft = INGVIO_OK;
    for (int i = 0; i < nb; ++i) {
        const int st = soft_status(status[i]);
        if (status_out) status_out[i] = st;
        if (st != INGVIO_OK) soft = st;
    }
    return soft;
}

// ---- GnssUpdate::updateTrackedSys for a batch (GnssUpdate.cpp:148-290): per-row gates, compaction, block gate, ekfUpdate ----

static int gnss_alloc(ingvio_ctx* c)
{
    auto& g = c->gn;
    if (g.H) return 0;
    const size_t B = c->d.batch, mld = c->mld, hs = mld * GNSS_NCW;
    int rc = 0;
    rc |= dalloc(c, &g.H, B * hs); rc |= dalloc(c, &g.res, B * mld); rc |= dalloc(c, &g.noise, B * mld); rc |= dalloc(c, &g.gamma, B * mld);
    rc |= dalloc(c, &g.chi2, CHI2_CAP); rc |= dalloc(c, &g.m, B); rc |= dalloc(c, &g.nc, B); rc |= dalloc(c, &g.colmap, B * GNSS_NCW);
    rc |= dalloc(c, &g.keep, B * mld);
    if (!c->d_noiseB) rc |= dalloc(c, &c->d_noiseB, B * mld);
    if (rc) return INGVIO_E_HIP;
    g.hi.assign(B, 0);
    return 0;
}

int ingvio_gnss_stage(ingvio_ctx* c, int b0, int nb, const ingvio_update_block* blk, const ingvio_gnss_opts* o)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !blk || !o) return INGVIO_E_ARG;
    if ((o->gate_rows || o->strong_reject) && (!o->chi2_table || o->chi2_len < 2 || o->chi2_len > CHI2_CAP)) return INGVIO_E_ARG;
    auto& g = c->gn;
    int m_cap = 0;
    std::vector<int> ncs(nb), his(nb);
    for (int i = 0; i < nb; ++i) {
        const ingvio_update_block& q = blk[i];
        if (q.m < 0 || q.k < 0) return INGVIO_E_ARG;
        if (q.m == 0) { ncs[i] = 0; his[i] = 0; continue; }                     // no measurement for this filter
        if (!q.vidx || !q.vsize || !q.H || !q.res || !q.R || q.k < 1 || q.ldh < q.m) return INGVIO_E_ARG;
        if (q.m > c->mld || q.m > 256) return INGVIO_E_CAPACITY;
        int nc = 0, hi = 0;
        for (int j = 0; j < q.k; ++j) {
            if (q.vidx[j] < 0 || q.vsize[j] < 1 || q.vidx[j] + q.vsize[j] > c->d.n_max) return INGVIO_E_NOT_IN_STATE;
            if (q.vidx[j] + q.vsize[j] > hi) hi = q.vidx[j] + q.vsize[j];
            nc += q.vsize[j];
        }
        if (nc > GNSS_NCW || !ekf_core_fits(q.m, nc)) return INGVIO_E_CAPACITY;
        ncs[i] = nc; his[i] = hi;
        if (q.m > m_cap) m_cap = q.m;
    }
    const size_t mld = c->mld, hs = mld * GNSS_NCW;
    if (gnss_alloc(c)) return INGVIO_E_HIP;
    Uploader upl{ c };
    int rc = upl.begin(pad64(8 * (size_t)nb * hs) + 2 * pad64(8 * (size_t)nb * mld) + pad64(4 * (size_t)nb * GNSS_NCW) + 2 * pad64(4 * (size_t)nb) +
                       pad64(8 * CHI2_CAP) + 1024);
    if (rc) return rc;
    double* hH = upl.take<double>((size_t)nb * hs); double* hr = upl.take<double>((size_t)nb * mld); double* hn = upl.take<double>((size_t)nb * mld);
    int* hc = upl.take<int>((size_t)nb * GNSS_NCW); int* hm = upl.take<int>(nb); int* hnc = upl.take<int>(nb);
    double* hchi = upl.take<double>(CHI2_CAP);
    parallel_for(nb, [=, &ncs](int i) {
        const ingvio_update_block& q = blk[i];
        const int nc = ncs[i];
        double* Hd = hH + (size_t)i * hs;
        for (int cc = 0; cc < nc; ++cc) {
            memcpy(Hd + (size_t)cc * mld, q.H + (size_t)cc * q.ldh, 8 * (size_t)q.m);
            memset(Hd + (size_t)cc * mld + q.m, 0, 8 * (mld - q.m));
        }
        if (q.m) { memcpy(hr + (size_t)i * mld, q.res, 8 * (size_t)q.m); memcpy(hn + (size_t)i * mld, q.R, 8 * (size_t)q.m); }
        int* cm = hc + (size_t)i * GNSS_NCW;
        int w = 0;
        if (q.m) for (int j = 0; j < q.k; ++j) for (int t = 0; t < q.vsize[j]; ++t) cm[w++] = q.vidx[j] + t;
        hm[i] = q.m; hnc[i] = nc;
    });
    for (int i = 0; i < nb; ++i) g.hi[b0 + i] = his[i];
    upl.copy(g.H + (size_t)b0 * hs, hH, (size_t)nb * hs);
    upl.copy(g.res + (size_t)b0 * mld, hr, (size_t)nb * mld);
    upl.copy(g.noise + (size_t)b0 * mld, hn, (size_t)nb * mld);
    upl.copy(g.colmap + (size_t)b0 * GNSS_NCW, hc, (size_t)nb * GNSS_NCW);
    upl.copy(g.m + b0, hm, nb); upl.copy(g.nc + b0, hnc, nb);
    g.chi2_len = 0;
    if (o->chi2_table) {
        memcpy(hchi, o->chi2_table, 8 * (size_t)o->chi2_len);
        upl.copy(g.chi2, hchi, (size_t)o->chi2_len);
        g.chi2_len = o->chi2_len;
    }
    rc = upl.end();
    if (rc) return rc;
    g.gate_rows = o->gate_rows ? 1 : 0; g.strong = o->strong_reject ? 1 : 0;
    g.thr1 = o->gate_rows ? o->chi2_table[1] : __builtin_inf();
    if (!g.staged || m_cap > g.m_cap) g.m_cap = m_cap;
    int ncm = 0;
    for (int i = 0; i < nb; ++i) if (ncs[i] > ncm) ncm = ncs[i];
    if (!g.staged || ncm > g.nc_max) g.nc_max = ncm;
    g.in_frame = o->in_frame != 0;
    g.fused_last = false;
    g.results = false;
    g.nominal = false; g.nom_pending = false; g.own_status = false; g.frame_nom = false;
    if (g.in_frame && !g.W) {
        const size_t B = c->d.batch, ws = (size_t)c->ldp * 16;
        if (dalloc(c, &g.W, B * ws) | dalloc(c, &g.Yf, B * ws) | dalloc(c, &g.dxf, B * (size_t)c->ldp) | dalloc(c, &g.mf, B) | dalloc(c, &g.ncf, B)) return INGVIO_E_HIP;
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    g.staged = true;
    return INGVIO_OK;
}

// The staged GNSS update as its own pass over the covariance (ingvio_gnss_run, and ingvio_frame_run for an in-frame stage that
// cannot ride on the MSCKF write-back)
static int gnss_run_separate(ingvio_ctx* c, int b0, int nb, bool own_slots = false);

// the buffers, then ephemerides, observations, receiver records and the gate table of epochs [b0, b0 + nb) onto the compute stream
// (behind whatever still reads them there); own_slots: also the result slots a stage from the device nominal state keeps apart
static int gnss_front_upload(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_epoch* ep, const ingvio_gnss_opts* o, bool own_slots)
{
    int rc = gnss_alloc(c);
    if (rc) return rc;
    auto& g = c->gn;
    const size_t B = c->d.batch;
    if (!g.front) {
        rc |= dalloc(c, &g.feph, B * INGVIO_GNSS_MAX_SAT * GE_N); rc |= dalloc(c, &g.fobs, B * INGVIO_GNSS_MAX_SAT * GO_N);
        rc |= dalloc(c, &g.frcv, B * GR_N); rc |= dalloc(c, &g.front, B * 64 * GF_N);
        if (rc) return INGVIO_E_HIP;
    }
    if (own_slots) {                                // the run's own result slots (shared with an in-frame stage) and status words
        if (!g.dxf) rc |= dalloc(c, &g.dxf, B * (size_t)c->ldp);
        if (!g.mf) rc |= dalloc(c, &g.mf, B);
        if (!g.ncf) rc |= dalloc(c, &g.ncf, B);
        if (!g.stf) rc |= dalloc(c, &g.stf, B);
        if (rc) return INGVIO_E_HIP;
    }
    const size_t S = INGVIO_GNSS_MAX_SAT;
    Uploader upl{ c };
    rc = upl.begin(pad64(8 * (size_t)nb * S * GE_N) + pad64(8 * (size_t)nb * S * GO_N) + pad64(8 * (size_t)nb * GR_N) + pad64(8 * CHI2_CAP) + 1024);
    if (rc) return rc;
    double* he = upl.take<double>((size_t)nb * S * GE_N); double* ho = upl.take<double>((size_t)nb * S * GO_N);
    double* hr = upl.take<double>((size_t)nb * GR_N); double* hchi = upl.take<double>(CHI2_CAP);
    const double adj_yof = c->gnss_adjust_yof ? 1.0 : 0.0;
    parallel_for(nb, [=](int i) {
        const ingvio_gnss_epoch& e = ep[i];
        memcpy(he + (size_t)i * S * GE_N, e.eph, 8 * (size_t)e.n_sat * GE_N);
        memcpy(ho + (size_t)i * S * GO_N, e.obs, 8 * (size_t)e.n_sat * GO_N);
        double* r = hr + (size_t)i * GR_N;
        memset(r, 0, 8 * GR_N);
        r[GR_NSAT] = e.n_sat; r[GR_DOY] = e.doy; r[GR_HAVE_ION] = e.ion ? 1.0 : 0.0;
        if (e.ion) memcpy(r + GR_ION, e.ion, 64);
        memcpy(r + GR_PW, e.p_w, 24); memcpy(r + GR_VW, e.v_w, 24); memcpy(r + GR_CB, e.cb, 32);
        r[GR_FS] = e.fs; r[GR_YAW] = e.yaw_offset;
        memcpy(r + GR_RENU, e.R_enu2ecef, 72); memcpy(r + GR_ANCHOR, e.anchor_ecef, 24);
        r[GR_IDX_SE23] = e.idx_se23; r[GR_IDX_YOF] = e.idx_yof; r[GR_IDX_FS] = e.idx_fs;
        for (int s = 0; s < 4; ++s) r[GR_IDX_CB + s] = e.idx_cb[s];
        r[GR_PSR_AMP] = e.psr_noise_amp; r[GR_DOPP_AMP] = e.dopp_noise_amp;
        r[GR_ADJ_YOF] = adj_yof;
    });
    upl.copy(g.feph + (size_t)b0 * S * GE_N, he, (size_t)nb * S * GE_N);
    upl.copy(g.fobs + (size_t)b0 * S * GO_N, ho, (size_t)nb * S * GO_N);
    upl.copy(g.frcv + (size_t)b0 * GR_N, hr, (size_t)nb * GR_N);
    g.chi2_len = 0;
    if (o->chi2_table) {
        memcpy(hchi, o->chi2_table, 8 * (size_t)o->chi2_len);
        upl.copy(g.chi2, hchi, (size_t)o->chi2_len);
        g.chi2_len = o->chi2_len;
    }
    rc = upl.end();
    if (rc) return rc;
    return rc;
}

// k_gnss_front over the uploaded epochs: candidate rows, column map and counts of the stage (nominal: receiver state and idx from the table)
namespace {      // (declared ahead of gnss_in_frame_launch)
void gnss_front_launch(ingvio_ctx* c, int b0, int nb, bool nominal, hipStream_t st)
{
    auto& g = c->gn;
    const size_t S = INGVIO_GNSS_MAX_SAT;
    const size_t mld = c->mld, hs = mld * GNSS_NCW;
    GnssFrontLaunch L;
    L.eph = g.feph + (size_t)b0 * S * GE_N; L.obs = g.fobs + (size_t)b0 * S * GO_N; L.rcv = g.frcv + (size_t)b0 * GR_N; L.smax = (int)S;
    L.front = g.front + (size_t)b0 * 64 * GF_N;
    L.H = g.H + (size_t)b0 * hs; L.res = g.res + (size_t)b0 * mld; L.noise = g.noise + (size_t)b0 * mld;
    L.m = g.m + b0; L.nc = g.nc + b0; L.colmap = g.colmap + (size_t)b0 * GNSS_NCW; L.mld = c->mld; L.hstride = (int)hs;
    const NomTable nt = nom_table(c);
    launch_gnss_front(L, nb, st, nominal ? &nt : nullptr, b0);
}
}  // namespace

// raw GNSS epochs -> candidate rows, on the device (kernels_gnss.hip)
// nominal: the receiver state and the idx_* the kernel uses come from the device nominal table (the epochs' idx_* are the host mirror's, for
// the checks below; p_w, v_w, cb, fs, yaw_offset are not read)
static int gnss_front_stage_impl(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_epoch* ep, const ingvio_gnss_opts* o, bool nominal)
{
    static_assert(GNSS_FRONT_NCW == GNSS_NCW, "column stride of the staged rows");
    if (check_range(c, b0, nb) || !ep || !o) return INGVIO_E_ARG;
    if ((o->gate_rows || o->strong_reject) && (!o->chi2_table || o->chi2_len < 2 || o->chi2_len > CHI2_CAP)) return INGVIO_E_ARG;
    int smax = 1;
    std::vector<int> his(nb, 0);
    for (int i = 0; i < nb; ++i) {
        const ingvio_gnss_epoch& e = ep[i];
        if (e.n_sat < 0 || e.n_sat > INGVIO_GNSS_MAX_SAT || (e.n_sat && (!e.eph || !e.obs))) return INGVIO_E_ARG;
        if (2 * e.n_sat > c->mld || 2 * e.n_sat > 256) return INGVIO_E_CAPACITY;
        if (e.n_sat > smax) smax = e.n_sat;
        int hi = 0;
        const int idx[7] = { e.idx_se23 + 9, e.idx_yof + 1, e.idx_fs + 1, e.idx_cb[0] + 1, e.idx_cb[1] + 1, e.idx_cb[2] + 1, e.idx_cb[3] + 1 };
        if (e.n_sat) { if (e.idx_se23 < 0 || e.idx_yof < 0 || e.idx_fs < 0) return INGVIO_E_NOT_IN_STATE; for (int v : idx) { if (v > c->d.n_max) return INGVIO_E_NOT_IN_STATE; if (v > hi) hi = v; } }
        his[i] = hi;
        if (!ekf_core_fits(2 * e.n_sat ? 2 * e.n_sat : 1, 15)) return INGVIO_E_CAPACITY;
    }
    if (int rc = gnss_front_upload(c, b0, nb, ep, o, nominal)) return rc;
    auto& g = c->gn;
    gnss_front_launch(c, b0, nb, nominal, c->st);
    for (int i = 0; i < nb; ++i) g.hi[b0 + i] = his[i];
    g.gate_rows = o->gate_rows ? 1 : 0; g.strong = o->strong_reject ? 1 : 0;
    g.thr1 = o->gate_rows ? o->chi2_table[1] : __builtin_inf();
    int m_cap = 2 * smax;
    // its own stage, never merged with an earlier one: GNSS rows of any range staged before and not yet run are dropped (documented in
    // the header); no satellite anywhere: no rows
    if (nominal) {
        g.staged = false;
        bool any = false;
        for (int i = 0; i < nb; ++i) if (ep[i].n_sat > 0) any = true;
        if (!any) m_cap = 0;
    }
    if (!g.staged || m_cap > g.m_cap) g.m_cap = m_cap;
    // the front builds the reference's var_order [SE23, YOF, <= 4 clocks, FS] = at most 15 columns; a front-staged update is applied
    // by ingvio_gnss_run (the flags of an earlier in-frame ingvio_gnss_stage must not leak into this stage)
    if (o->in_frame) { c->err = "ingvio_gnss_front_stage: in_frame is not supported (stage the rows with ingvio_gnss_stage)"; return INGVIO_E_UNSUPPORTED; }
    g.in_frame = false; g.nc_max = 15; g.fused_last = false; g.results = false;
    g.nominal = nominal; g.nom_pending = nominal; g.own_status = false; g.frame_nom = false; g.nom_b0 = b0; g.nom_nb = nb;
    g.staged = true;
    return last_launch(c);
}

int ingvio_gnss_front_stage(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_epoch* ep, const ingvio_gnss_opts* o)
{
    ENTER(c);
    return gnss_front_stage_impl(c, b0, nb, ep, o, false);
}

int ingvio_gnss_front_stage_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_epoch_nominal* ep, const ingvio_gnss_opts* o)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !ep || !o) return INGVIO_E_ARG;
    if (o->in_frame) { c->err = "ingvio_gnss_front_stage_nominal: in_frame is not supported"; return INGVIO_E_UNSUPPORTED; }
    auto& m = c->nom;
    // without a table there is nothing the kernel could read, whatever the epochs hold (also when none has a satellite)
    if (!m.vmax) { c->err = "ingvio_gnss_front_stage_nominal without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "ingvio_gnss_front_stage_nominal: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (c->lm.nom_pending) { c->err = "ingvio_gnss_front_stage_nominal: a landmark update staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    // the receiver's variables, from the host mirror of the table (no device round trip): what ingvio_gnss_front_stage checks on the
    // epoch's idx_* is checked on these
    std::vector<ingvio_gnss_epoch> full((size_t)nb);
    for (int i = 0; i < nb; ++i) {
        const ingvio_gnss_epoch_nominal& e = ep[i];
        ingvio_gnss_epoch& f = full[i];
        memset(&f, 0, sizeof f);
        f.n_sat = e.n_sat; f.eph = e.eph; f.obs = e.obs; f.ion = e.ion; f.doy = e.doy;
        memcpy(f.R_enu2ecef, e.R_enu2ecef, sizeof f.R_enu2ecef); memcpy(f.anchor_ecef, e.anchor_ecef, sizeof f.anchor_ecef);
        f.psr_noise_amp = e.psr_noise_amp; f.dopp_noise_amp = e.dopp_noise_amp;
        f.idx_se23 = f.idx_yof = f.idx_fs = -1;
        for (int s = 0; s < 4; ++s) f.idx_cb[s] = -1;
        if (e.n_sat <= 0) continue;                 // (n_sat < 0 is refused below; 0: no epoch for this filter)
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        bool reg = false;
        for (int s = 0; s < 6; ++s) if (I[NOM_GNSS + s] >= 0) reg = true;
        if (!reg) { c->err = "ingvio_gnss_front_stage_nominal: no GNSS scalars registered for the filter (ingvio_nominal_set_gnss)"; return INGVIO_E_ARG; }
        f.idx_se23 = nom_idx_of(c, b, I[NOM_V_POSE]);
        f.idx_yof = nom_idx_of(c, b, I[NOM_GNSS + NOM_G_YOF]);
        f.idx_fs = nom_idx_of(c, b, I[NOM_GNSS + NOM_G_FS]);
        for (int s = 0; s < 4; ++s) f.idx_cb[s] = nom_idx_of(c, b, I[NOM_GNSS + s]);
    }
    return gnss_front_stage_impl(c, b0, nb, full.data(), o, true);
}

// The raw epoch of the frame staged from the table: validated on the host mirror, uploaded, applied by that frame's
// ingvio_frame_run - on the MSCKF write-back where gnss_folds() allows it, else as the two-call sequence behind the frame.  Nothing is
// launched here (the front's inputs exist only after the MSCKF update) and the result slots of the frame before stay as they are.
int ingvio_gnss_frame_stage_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_gnss_epoch_nominal* ep, const ingvio_gnss_opts* o)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !ep || !o) return INGVIO_E_ARG;
    if ((o->gate_rows || o->strong_reject) && (!o->chi2_table || o->chi2_len < 2 || o->chi2_len > CHI2_CAP)) return INGVIO_E_ARG;
    auto& m = c->nom;
    auto& g = c->gn;
    if (!m.vmax) { c->err = "ingvio_gnss_frame_stage_nominal without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (!m.pending) { c->err = "ingvio_gnss_frame_stage_nominal: no frame staged from the device nominal state is waiting to run"; return INGVIO_E_ARG; }
    if (m.noprop) {
        c->err = "ingvio_gnss_frame_stage_nominal: an update-only frame takes no GNSS epoch (ingvio_gnss_front_stage_nominal + ingvio_gnss_run behind it)";
        return INGVIO_E_UNSUPPORTED;
    }
    if (b0 != 0 || nb != c->d.batch) { c->err = "ingvio_gnss_frame_stage_nominal stages the whole batch (b0 = 0, nb = batch)"; return INGVIO_E_ARG; }
    if (g.staged && g.frame_nom) { c->err = "ingvio_gnss_frame_stage_nominal: the frame has its GNSS epoch already"; return INGVIO_E_ARG; }
    std::vector<ingvio_gnss_epoch> full((size_t)nb);
    std::vector<int> his(nb, 0);
    int smax = 0;
    for (int i = 0; i < nb; ++i) {
        const ingvio_gnss_epoch_nominal& e = ep[i];
        ingvio_gnss_epoch& f = full[i];
        memset(&f, 0, sizeof f);
        if (e.n_sat < 0 || e.n_sat > INGVIO_GNSS_MAX_SAT || (e.n_sat && (!e.eph || !e.obs))) return INGVIO_E_ARG;
        if (2 * e.n_sat > c->mld || 2 * e.n_sat > 256) return INGVIO_E_CAPACITY;
        if (!ekf_core_fits(2 * e.n_sat ? 2 * e.n_sat : 1, 15)) return INGVIO_E_CAPACITY;
        f.n_sat = e.n_sat; f.eph = e.eph; f.obs = e.obs; f.ion = e.ion; f.doy = e.doy;
        memcpy(f.R_enu2ecef, e.R_enu2ecef, sizeof f.R_enu2ecef); memcpy(f.anchor_ecef, e.anchor_ecef, sizeof f.anchor_ecef);
        f.psr_noise_amp = e.psr_noise_amp; f.dopp_noise_amp = e.dopp_noise_amp;
        f.idx_se23 = f.idx_yof = f.idx_fs = -1;
        for (int s = 0; s < 4; ++s) f.idx_cb[s] = -1;
        if (e.n_sat == 0) continue;                 // no epoch for this filter
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        bool reg = false;
        for (int s = 0; s < 6; ++s) if (I[NOM_GNSS + s] >= 0) reg = true;
        if (!reg) { c->err = "ingvio_gnss_frame_stage_nominal: no GNSS scalars registered for the filter (ingvio_nominal_set_gnss)"; return INGVIO_E_ARG; }
        // every column the kernels will name, from the mirror (the frame's stage has put the new clone there; its 6 columns are appended
        // by the run): [idx, idx + size) inside the state at update time, clear of the clone that leaves, and inside the state behind
        // the marginalisation once shifted - whichever of the two orders the run takes
        const int var_idx[7] = { nom_idx_of(c, b, I[NOM_V_POSE]), nom_idx_of(c, b, I[NOM_GNSS + NOM_G_YOF]), nom_idx_of(c, b, I[NOM_GNSS + NOM_G_FS]),
                                 nom_idx_of(c, b, I[NOM_GNSS + 0]), nom_idx_of(c, b, I[NOM_GNSS + 1]), nom_idx_of(c, b, I[NOM_GNSS + 2]),
                                 nom_idx_of(c, b, I[NOM_GNSS + 3]) };
        if (var_idx[0] < 0 || var_idx[1] < 0 || var_idx[2] < 0) {
            c->err = "ingvio_gnss_frame_stage_nominal: the extended pose, YOF or FS is not in the table"; return INGVIO_E_NOT_IN_STATE;
        }
        const int n_upd = std::min(c->d.n_max, c->h_n[b] + 6), mg = c->st_marg[b];
        int hi = 0;
        for (int q = 0; q < 7; ++q) {
            const int lo = var_idx[q], sz = q == 0 ? 9 : 1;
            if (lo < 0) continue;                    // (a constellation without a clock in the state)
            bool ok = lo + sz <= n_upd;
            if (ok && mg >= 0) ok = (lo + sz <= mg || lo >= mg + 6) && (lo > mg ? lo - 6 : lo) + sz <= n_upd - 6;
            if (!ok) { c->err = "ingvio_gnss_frame_stage_nominal: a GNSS column lies outside the state the update will see"; return INGVIO_E_NOT_IN_STATE; }
            hi = std::max(hi, lo + sz);
        }
        f.idx_se23 = var_idx[0]; f.idx_yof = var_idx[1]; f.idx_fs = var_idx[2];
        for (int s = 0; s < 4; ++s) f.idx_cb[s] = var_idx[3 + s];
        his[i] = hi;
        smax = std::max(smax, e.n_sat);
    }
    // ---- from here on only HIP errors: buffers (first call), then the uploads on the compute stream, behind the kernels of the frame
    //      enqueued last that may still read them ----
    if (int rc = gnss_front_upload(c, b0, nb, full.data(), o, true)) return rc;
    if (!g.W) {
        const size_t B = c->d.batch, ws = (size_t)c->ldp * 16;
        if (dalloc(c, &g.W, B * ws) | dalloc(c, &g.Yf, B * ws)) return INGVIO_E_HIP;
    }
    for (int i = 0; i < nb; ++i) g.hi[b0 + i] = his[i];
    g.gate_rows = o->gate_rows ? 1 : 0; g.strong = o->strong_reject ? 1 : 0;
    g.thr1 = o->gate_rows ? o->chi2_table[1] : __builtin_inf();
    g.m_cap = 2 * smax; g.nc_max = 15;            // (no satellite anywhere: m_cap = 0, the frame runs alone)
    // (results / fused_last / own_status belong to the update that ran last: ingvio_gnss_fetch of the frame before stays valid)
    g.in_frame = true; g.nominal = true; g.nom_pending = false; g.frame_nom = true; g.nom_b0 = b0; g.nom_nb = nb;
    g.staged = true;
    return last_launch(c);
}

int ingvio_debug_gnss_fused_last(ingvio_ctx* c) { return c ? (c->gn.fused_last && c->gn.results ? (c->gn.folded_last ? 2 : 1) : 0) : INGVIO_E_ARG; }

// gnss_comm::sat_states + psr_res + dopp_res for an arbitrary list of epochs, detached from the filters of the context and from
// the staged update rows: what GvioAligner::batchAlign (GvioAligner.cpp:88-383) and gnss_comm::psr_pos (gnss_spp.cpp:148-254)
// iterate on.  One launch for all epochs, temporary device buffers, nothing of the context's state is touched.
int ingvio_gnss_sat_eval(ingvio_ctx* c, int n_epochs, const ingvio_gnss_epoch* ep, double* out)
{
    ENTER(c);
    if (!c || n_epochs < 1 || !ep || !out) return INGVIO_E_ARG;
    const size_t S = INGVIO_GNSS_MAX_SAT;
    for (int i = 0; i < n_epochs; ++i) {
        const ingvio_gnss_epoch& e = ep[i];
        if (e.n_sat < 0 || e.n_sat > INGVIO_GNSS_MAX_SAT) return INGVIO_E_CAPACITY;
        if (e.n_sat && (!e.eph || !e.obs)) return INGVIO_E_ARG;
    }
    std::vector<double> he((size_t)n_epochs * S * GE_N, 0.0), ho((size_t)n_epochs * S * GO_N, 0.0), hr((size_t)n_epochs * GR_N, 0.0);
    for (int i = 0; i < n_epochs; ++i) {
        const ingvio_gnss_epoch& e = ep[i];
        if (e.n_sat) {
            memcpy(he.data() + (size_t)i * S * GE_N, e.eph, 8 * (size_t)e.n_sat * GE_N);
            memcpy(ho.data() + (size_t)i * S * GO_N, e.obs, 8 * (size_t)e.n_sat * GO_N);
        }
        double* r = hr.data() + (size_t)i * GR_N;
        r[GR_NSAT] = e.n_sat; r[GR_DOY] = e.doy; r[GR_HAVE_ION] = e.ion ? 1.0 : 0.0;
        if (e.ion) memcpy(r + GR_ION, e.ion, 64);
        memcpy(r + GR_PW, e.p_w, 24); memcpy(r + GR_VW, e.v_w, 24); memcpy(r + GR_CB, e.cb, 32);
        r[GR_FS] = e.fs; r[GR_YAW] = e.yaw_offset;
        memcpy(r + GR_RENU, e.R_enu2ecef, 72); memcpy(r + GR_ANCHOR, e.anchor_ecef, 24);
        for (int s4 = 0; s4 < 4; ++s4) r[GR_IDX_CB + s4] = -1.0;
        r[GR_PSR_AMP] = e.psr_noise_amp; r[GR_DOPP_AMP] = e.dopp_noise_amp;
    }
    const size_t S64 = 64;
    if (n_epochs > c->se.cap) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        for (double** q : { &c->se.e, &c->se.o, &c->se.r, &c->se.f }) { if (*q) hipFree(*q); *q = nullptr; }
        c->se.cap = 0;
        const int cap = std::max(n_epochs, 32);
        if (hipMalloc((void**)&c->se.e, 8 * (size_t)cap * S * GE_N) != hipSuccess || hipMalloc((void**)&c->se.o, 8 * (size_t)cap * S * GO_N) != hipSuccess ||
            hipMalloc((void**)&c->se.r, 8 * (size_t)cap * GR_N) != hipSuccess || hipMalloc((void**)&c->se.f, 8 * (size_t)cap * S64 * GF_N) != hipSuccess) {
            for (double** q : { &c->se.e, &c->se.o, &c->se.r, &c->se.f }) { if (*q) hipFree(*q); *q = nullptr; }
            c->err = "hipMalloc failed (ingvio_gnss_sat_eval workspace)";
            return INGVIO_E_HIP;
        }
        c->se.cap = cap;
    }
    double *de = c->se.e, *dob = c->se.o, *dr = c->se.r, *df = c->se.f;
    int rc = up(c, de, he.data(), 8 * he.size()) | up(c, dob, ho.data(), 8 * ho.size()) | up(c, dr, hr.data(), 8 * hr.size());
    if (!rc) {
        GnssFrontLaunch L;
        memset(&L, 0, sizeof L);
        L.eph = de; L.obs = dob; L.rcv = dr; L.smax = (int)S; L.front = df;      // L.H == nullptr: no candidate rows
        launch_gnss_front(L, n_epochs, c->st);
        rc = down_sync(c, out, df, 8 * (size_t)n_epochs * 64 * GF_N);           // synchronises: the host vectors above may go
    }
    else hipStreamSynchronize(c->st);
    return rc ? INGVIO_E_HIP : last_launch(c);
}

int ingvio_gnss_front_fetch(ingvio_ctx* c, int b0, int nb, double* out)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !out || !c->gn.front) return INGVIO_E_ARG;
    if (down_sync(c, out, c->gn.front + (size_t)b0 * 64 * GF_N, 8 * (size_t)nb * 64 * GF_N)) return INGVIO_E_HIP;
    return last_launch(c);
}

// test hook: the candidate rows of filter b as the last stage left them (no gate has touched them; a run only reads them)
int ingvio_debug_gnss_staged_rows(ingvio_ctx* c, int b, double* H, double* res, double* noise, int* colmap, int* m_out, int* nc_out)
{
    ENTER(c);
    if (check_range(c, b, 1) || !H || !res || !noise || !colmap || !m_out || !nc_out) return INGVIO_E_ARG;
    auto& g = c->gn;
    if (!g.staged || !g.H) { c->err = "ingvio_debug_gnss_staged_rows: no GNSS rows are staged"; return INGVIO_E_ARG; }
    const size_t mld = c->mld, hs = mld * GNSS_NCW;
    HIPCHK(c, hipMemcpyAsync(H, g.H + (size_t)b * hs, 8 * hs, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(res, g.res + (size_t)b * mld, 8 * mld, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(noise, g.noise + (size_t)b * mld, 8 * mld, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(colmap, g.colmap + (size_t)b * GNSS_NCW, sizeof(int) * GNSS_NCW, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(m_out, g.m + b, sizeof(int), hipMemcpyDeviceToHost, c->st));
    if (down_sync(c, nc_out, g.nc + b, sizeof(int))) return INGVIO_E_HIP;
    return last_launch(c);
}

int ingvio_gnss_run(ingvio_ctx* c, int b0, int nb)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !c->gn.staged) return INGVIO_E_ARG;
    if (c->gn.in_frame) { c->err = "the staged GNSS update is in-frame: ingvio_frame_run applies it"; return INGVIO_E_ARG; }
    if (!c->gn.nominal) return gnss_run_separate(c, b0, nb);
    // ---- staged from the device nominal state: the update, then StateManager::boxPlus of its dx on the table, once ----
    auto& g = c->gn;
    if (b0 != g.nom_b0 || nb != g.nom_nb) { c->err = "ingvio_gnss_run: a stage from the device nominal state runs on the range it was staged for"; return INGVIO_E_ARG; }
    if (c->nom.pending) { c->err = "ingvio_gnss_run: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    for (int i = 0; i < nb; ++i) if (g.hi[b0 + i] > c->h_n[b0 + i]) return INGVIO_E_NOT_IN_STATE;      // before anything changes
    HIPCHK(c, hipMemsetAsync(g.dxf + (size_t)b0 * c->ldp, 0, 8 * (size_t)nb * c->ldp, c->st));       // dx = 0 beyond the live n and without rows
    HIPCHK(c, hipMemsetAsync(g.stf + b0, 0, sizeof(int) * (size_t)nb, c->st));
    HIPCHK(c, hipMemsetAsync(g.mf + b0, 0, sizeof(int) * (size_t)nb, c->st));
    // a refusal of the pass below (INGVIO_E_CAPACITY of the row gate's LDS check) comes before its first launch: the stage then stays
    // pending with its rows and the table is untouched (the stage's own result slots have been cleared: nothing to fetch)
    const bool own_before = g.own_status, fused_before = g.fused_last, results_before = g.results;
    g.own_status = true;
    if (int rc = gnss_run_separate(c, b0, nb, true)) {
        if (rc != INGVIO_E_HIP) { g.own_status = own_before; g.fused_last = fused_before; g.results = results_before; }
        return rc;
    }
    g.nom_pending = false; g.staged = false;       // consumed: the table moves with this run, a second one is refused
    if (g.m_cap > 0) {                              // rejected block / no epoch: dx = 0, the retraction's small-angle branch is the identity
        launch_nominal_update(nom_table(c), g.dxf, c->ldp, nullptr, b0, nb, c->st);
        if (int rc = last_launch(c)) return rc;
    }
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

// own_slots: called by ingvio_frame_run for an in-frame stage - row count, column count and dx go to the stage's own buffers (the
// frame's slots keep the MSCKF update's results for ingvio_frame_fetch) and the frame's status bits stay
static int gnss_run_separate(ingvio_ctx* c, int b0, int nb, bool own_slots)
{
    auto& g = c->gn;
    g.fused_last = own_slots; g.folded_last = false;
    g.results = true;
    int n_cap = 0;
    for (int i = 0; i < nb; ++i) {
        if (g.hi[b0 + i] > c->h_n[b0 + i]) return INGVIO_E_NOT_IN_STATE;          // checkSubOrder against the LIVE state
        if (c->h_n[b0 + i] > n_cap) n_cap = c->h_n[b0 + i];
    }
    if (g.m_cap == 0) return INGVIO_OK;
    const size_t mld = c->mld, hs = mld * GNSS_NCW;
    if (!own_slots) HIPCHK(c, hipMemsetAsync(c->d_status + b0, 0, sizeof(int) * (size_t)nb, c->st));
    // after a fused frame step every filter's live covariance sits in the SECOND ping-pong half and this update (k_downdate) is in
    // place there: the first half still holds the prior up to the propagation strips, so a following ingvio_frame_run(restore_prior)
    // may keep restoring the strips only (0.03 instead of 0.10 ms per 512 filters)
    bool keep_strips = c->strip_ok && c->mut_seq == c->strip_seq;
    for (int i = 0; i < nb && keep_strips; ++i) if (c->h_cur[b0 + i] != 1) keep_strips = false;      // ... which only holds for filters that sit in the second half
    EkfLaunch E;
    memset(&E, 0, sizeof E);
    E.cv = view(c);
    // k_downdate below is strictly in place in the live half (launch_downdate never writes the other one): the strips stay valid
    if (keep_strips) c->strip_seq = c->mut_seq;
    E.b0 = b0; E.nb = nb; E.H = c->d_H + (size_t)b0 * hs; E.res = c->d_res + (size_t)b0 * mld;
    E.colmap = c->d_colmap + (size_t)b0 * GNSS_NCW; E.m = (own_slots ? g.mf : c->d_m) + b0; E.nc = (own_slots ? g.ncf : c->d_nc) + b0;
    E.noise = c->d_noiseB + (size_t)b0 * mld; E.r_kind = INGVIO_R_DIAG; E.mld = c->mld; E.hstride = (int)hs; E.cstride = GNSS_NCW;
    E.nstride = c->mld; E.Y = c->d_Y + (size_t)b0 * c->ystride; E.ystride = c->ystride; E.dx = own_slots ? g.dxf : c->d_dx;
    E.status = g.own_status ? g.stf : c->d_status; E.m_cap = g.m_cap; E.nc_cap = GNSS_NCW;
    if (g.strong) { E.chi2 = g.chi2; E.chi2_len = g.chi2_len; E.gate_max_rows = 14; }      // GnssUpdate.cpp:286
    RowsGateIn in{ g.H + (size_t)b0 * hs, g.res + (size_t)b0 * mld, g.noise + (size_t)b0 * mld, g.m + b0, g.colmap + (size_t)b0 * GNSS_NCW,
                   g.nc + b0, (int)hs, GNSS_NCW };
    {
        ProfScope p(c, PF_ROWGATE);
        if (launch_rows_gate(E, in, g.thr1, g.gamma + (size_t)b0 * mld, g.keep + (size_t)b0 * mld, c->st)) return INGVIO_E_CAPACITY;
    }
    { ProfScope p(c, PF_EKF_CORE); launch_ekf_core(E, c->st); }
    { ProfScope p(c, PF_DOWNDATE); launch_downdate(E, n_cap, c->st); }
    return last_launch(c);
}

int ingvio_gnss_fetch(ingvio_ctx* c, int b0, int nb, double* dx_out, int* rows_out, int* keep_out, double* gamma_out, int* status_out)
{
    ENTER(c);
    if (check_range(c, b0, nb)) return INGVIO_E_ARG;
    if (!c->gn.results) { c->err = "ingvio_gnss_fetch: no GNSS update has run on the staged rows (an in-frame stage is applied by ingvio_frame_run)"; return INGVIO_E_ARG; }
    const size_t mld = c->mld;
    std::vector<int> status(nb, 0);
    const bool fz = c->gn.fused_last;             // the in-frame update kept its results apart from the frame's
    if (dx_out) HIPCHK(c, hipMemcpyAsync(dx_out, (fz ? c->gn.dxf : c->d_dx) + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
    if (rows_out) HIPCHK(c, hipMemcpyAsync(rows_out, (fz ? c->gn.mf : c->d_m) + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->gn.keep + (size_t)b0 * mld, sizeof(int) * (size_t)nb * mld, hipMemcpyDeviceToHost, c->st));
    if (gamma_out) HIPCHK(c, hipMemcpyAsync(gamma_out, c->gn.gamma + (size_t)b0 * mld, 8 * (size_t)nb * mld, hipMemcpyDeviceToHost, c->st));
    if (down_sync(c, status.data(), (c->gn.own_status ? c->gn.stf : c->d_status) + b0, sizeof(int) * (size_t)nb)) return INGVIO_E_HIP;
    int rc = last_launch(c);
    if (rc) return rc;
    int soft = INGVIO_OK;
    for (int i = 0; i < nb; ++i) {
        const int st = (status[i] & 8) ? INGVIO_REJECTED : soft_status(status[i]);
        if (status_out) status_out[i] = st;
        if (st == INGVIO_NEG_DIAG) soft = st;
    }
    return soft;
}

int ingvio_gnss_update_batch(ingvio_ctx* c, int b0, int nb, const ingvio_update_block* blk, const ingvio_gnss_opts* o, double* dx_out,
                             int* rows_out, int* keep_out, int* status_out)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    int rc = ingvio_gnss_stage(c, b0, nb, blk, o);
    if (rc) return rc;
    rc = ingvio_gnss_run(c, b0, nb);
    if (rc) return rc;
    return ingvio_gnss_fetch(c, b0, nb, dx_out, rows_out, keep_out, nullptr, status_out);
}

int ingvio_mld(ingvio_ctx* c) { return c ? c->mld : 0; }

int ingvio_chi2_gamma(ingvio_ctx* c, int b, const int* vidx, const int* vsize, int k, const double* H, int ldh, int m,
                      const double* res, const double* R, int r_kind, double* gamma)
{
    ENTER(c);
    if (!gamma) return INGVIO_E_ARG;
    int nc = 0;
    int rc = stage_generic(c, b, vidx, vsize, k, H, ldh, m, res, R, r_kind, &nc);
    if (rc) return rc;
    if ((size_t)8 * ((size_t)nc * m + (size_t)(m + 1) * (m + 1)) > 150 * 1024) return INGVIO_E_CAPACITY;
    launch_gamma(view(c), b, c->d_H + (size_t)b * c->hstride, c->d_res + (size_t)b * c->mld, c->d_colmap + (size_t)b * c->cstride,
                 m, nc, c->d_noise1, r_kind, c->mld, c->d_gamma + (size_t)b * c->d.f_max, c->st);
    if (down_sync(c, gamma, c->d_gamma + (size_t)b * c->d.f_max, 8)) return INGVIO_E_HIP;
    return last_launch(c);
}

// Many whitenResidual gates against the same prior in ONE launch and one synchronisation (all SLAM landmarks of a frame,
// LandmarkUpdate.cpp:98-99; the per-row GNSS gates, GnssUpdate.cpp:190,259): gamma_out[g] for block g, R = noise_var * I.
int ingvio_chi2_gamma_multi(ingvio_ctx* c, int b, int nblk, const ingvio_gate_block* blk, double noise_var, double* gamma_out)
{
    ENTER(c);
    if (check_range(c, b, 1) || nblk < 0 || (nblk && (!blk || !gamma_out))) return INGVIO_E_ARG;
    if (nblk == 0) return INGVIO_OK;
    size_t nd = 1, ni = 0, lds = 0;                         // doubles (slot 0 = noise), ints
    for (int g = 0; g < nblk; ++g) {
        const ingvio_gate_block& q = blk[g];
        if (!q.vidx || !q.vsize || !q.H || !q.res || q.k < 1 || q.m < 1 || q.ldh < q.m) return INGVIO_E_ARG;
        int nc = 0;
        for (int i = 0; i < q.k; ++i) {
            if (q.vidx[i] < 0 || q.vidx[i] + q.vsize[i] > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;
            nc += q.vsize[i];
        }
        nd += (size_t)q.m * nc + q.m; ni += nc;
        const size_t l = 8 * ((size_t)nc * q.m + (size_t)(q.m + 1) * (q.m + 1));
        if (l > lds) lds = l;
    }
    if (lds > 150 * 1024) return INGVIO_E_CAPACITY;
    const size_t bytes_d = pad64(8 * nd), bytes_i = pad64(4 * ni), bytes_desc = pad64(4 * 5 * (size_t)nblk), bytes_g = pad64(8 * (size_t)nblk);
    const size_t total = bytes_d + bytes_i + bytes_desc + bytes_g;
    if (c->multi_cap < total) if (int rc = dev_grow(c, &c->d_multi, &c->multi_cap, total * 2)) return rc;
    Uploader upl{ c };
    int rc = upl.begin(total + 1024);
    if (rc) return rc;
    double* hd = upl.take<double>(bytes_d / 8); int* hi = upl.take<int>(bytes_i / 4); int* hdesc = upl.take<int>(bytes_desc / 4);
    hd[0] = noise_var;
    size_t od = 1, oi = 0;
    for (int g = 0; g < nblk; ++g) {
        const ingvio_gate_block& q = blk[g];
        int nc = 0;
        int* cm = hi + oi;
        for (int i = 0; i < q.k; ++i) for (int j = 0; j < q.vsize[i]; ++j) cm[nc++] = q.vidx[i] + j;
        hdesc[5 * g] = (int)od;
        for (int cc = 0; cc < nc; ++cc) memcpy(hd + od + (size_t)cc * q.m, q.H + (size_t)cc * q.ldh, 8 * (size_t)q.m);
        od += (size_t)q.m * nc;
        hdesc[5 * g + 1] = (int)od;
        memcpy(hd + od, q.res, 8 * (size_t)q.m);
        od += q.m;
        hdesc[5 * g + 2] = (int)oi; hdesc[5 * g + 3] = q.m; hdesc[5 * g + 4] = nc;
        oi += nc;
    }
    double* dd = reinterpret_cast<double*>(c->d_multi);
    int* di = reinterpret_cast<int*>(c->d_multi + bytes_d);
    int* ddesc = reinterpret_cast<int*>(c->d_multi + bytes_d + bytes_i);
    double* dg = reinterpret_cast<double*>(c->d_multi + bytes_d + bytes_i + bytes_desc);
    upl.copy(dd, hd, nd); upl.copy(di, hi, ni); upl.copy(ddesc, hdesc, 5 * (size_t)nblk);
    rc = upl.end();
    if (rc) return rc;
    launch_gamma_multi(view(c), b, nblk, dd, di, ddesc, dd, dg, lds, c->st);
    if (down_sync(c, gamma_out, dg, 8 * (size_t)nblk)) return INGVIO_E_HIP;
    return last_launch(c);
}

// tri != nullptr: the points of the staged features are triangulated on the device first (ingvio_msckf_update_tri)
static int msckf_update_impl(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts, const ingvio_tri_opts* tri,
                             const unsigned long long* const* tri_masks, double* dx_out, int* accepted, double* gamma, int* rows_out, double* pf_out,
                             int* tri_ok)
{
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !frames || !opts) return INGVIO_E_ARG;
    if (tri && (tri->outer_loop_max_iter < 0 || tri->inner_loop_max_iter < 0)) return INGVIO_E_ARG;
    MsckfOpts op;
    c->fork_recorded = false;
    c->nom.tri_ran = false; c->nom.tri_fetched = false;      // (the result slab and its mirror are this call's from here on)
    HIPCHK(c, hipMemsetAsync(c->d_status + b0, 0, sizeof(int) * (size_t)nb, c->st));      // first: it runs while the host packs the frame
    int rc = make_opts(c, opts, &op);
    if (rc) return rc;
    int fmx = 0;
    rc = stage_frames(c, b0, nb, frames, &fmx);
    if (rc) return rc;
    rc = fill_noise_scalar(c, b0, nb, op.var);
    if (rc) return rc;
    const int fm = c->d.f_max;
    //  fork_recorded must not outlive this call: an early error return between here and run_msckf_factored - the only
    // place that consumes the flag - would make the NEXT large-window step skip recording ev_fork and start its side stream
    // against a stale event
    struct ForkGuard { ingvio_ctx* c; ~ForkGuard() { c->fork_recorded = false; } } fork_guard{ c };
    if (tri && c->d.c_max > 16 && c->st2 && c->method == 1) {      // the prior-only half of the large-window solve may start now, beside the triangulation
        HIPCHK(c, hipEventRecord(c->ev_fork, c->st));
        c->fork_recorded = true;
    }
    if (tri) {
        TriLaunch T;
        memset(&T, 0, sizeof T);
        T.fv = fview(c); T.b0 = b0;
        memcpy(T.R_lr, tri->R_cl2cr, 72); memcpy(T.t_lr, tri->t_cl2cr, 24);
        T.trans_thres = tri->trans_thres; T.huber_epsilon = tri->huber_epsilon; T.conv_precision = tri->conv_precision;
        T.init_damping = tri->init_damping; T.max_depth = tri->max_depth; T.min_depth = tri->min_depth;
        T.outer_loop_max_iter = tri->outer_loop_max_iter; T.inner_loop_max_iter = tri->inner_loop_max_iter;
        T.pf = c->d_pf; T.ok = c->d_tri_ok; T.mask_failed = 1; T.mask_rw = c->d_mask; T.check_anchor = 1;
        T.ok2 = (int*)(c->d_result_slab + c->ro_tok); T.pf2 = (double*)(c->d_result_slab + c->ro_tpf);
        if (tri_masks) {                                       // triangulation masks that differ from the update's: their own device array
            if (!c->d_tri_mask && dalloc(c, &c->d_tri_mask, (size_t)c->d.batch * fm)) return INGVIO_E_HIP;
            std::vector<unsigned long long> tm((size_t)nb * fm, 0ULL);
            for (int i = 0; i < nb; ++i) {
                const unsigned long long* src = tri_masks[i] ? tri_masks[i] : frames[i].obs_mask;
                const int C = frames[i].n_clones;
                const unsigned long long cmask = C >= 64 ? ~0ULL : ((1ULL << C) - 1ULL);
                for (int j = 0; j < frames[i].n_feat; ++j) tm[(size_t)i * fm + j] = src[j] & cmask;
            }
            const UpItem item = { c->d_tri_mask + (size_t)b0 * fm, tm.data(), 8 * tm.size() };
            if (stage_small(c, &item, 1)) return INGVIO_E_HIP;
            T.tri_mask = c->d_tri_mask;
        }
        if (launch_triangulate(T, nb, fmx > 0 ? fmx : 1, tri->stereo, c->st)) return INGVIO_E_UNSUPPORTED;
    }
    rc = run_msckf(c, b0, nb, op, opts->stereo, fmx);
    if (rc) return rc;
    std::vector<int> rows(nb), status(nb);
    if (b0 == 0 && nb == c->d.batch && (tri ? c->result_bytes : c->ro_tok) <= (1u << 20)) {      // the whole batch, small: one copy of the result slab (gated on the bytes this call copies)
        HIPCHK(c, hipMemcpyAsync(c->h_result, c->d_result_slab, tri ? c->result_bytes : c->ro_tok, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (dx_out) memcpy(dx_out, c->h_result, 8 * (size_t)nb * c->ldp);
        if (gamma) memcpy(gamma, c->h_result + c->ro_gam, 8 * (size_t)nb * fm);
        if (accepted) memcpy(accepted, c->h_result + c->ro_used, sizeof(int) * (size_t)nb * fm);
        memcpy(rows.data(), c->h_result + c->ro_m, sizeof(int) * (size_t)nb);
        memcpy(status.data(), c->h_result + c->ro_st, sizeof(int) * (size_t)nb);
        if (tri && tri_ok) memcpy(tri_ok, c->h_result + c->ro_tok, sizeof(int) * (size_t)nb * fm);
        if (tri && pf_out) memcpy(pf_out, c->h_result + c->ro_tpf, 8 * (size_t)nb * fm * 3);
    } else {
        if (tri && tri_ok) HIPCHK(c, hipMemcpyAsync(tri_ok, c->d_result_slab + c->ro_tok + sizeof(int) * (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
        if (tri && pf_out) HIPCHK(c, hipMemcpyAsync(pf_out, c->d_result_slab + c->ro_tpf + 8 * (size_t)b0 * fm * 3, 8 * (size_t)nb * fm * 3, hipMemcpyDeviceToHost, c->st));
        if (dx_out) HIPCHK(c, hipMemcpyAsync(dx_out, c->d_dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
        if (accepted) HIPCHK(c, hipMemcpyAsync(accepted, c->d_used + (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
        if (gamma) HIPCHK(c, hipMemcpyAsync(gamma, c->d_gamma + (size_t)b0 * fm, 8 * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(rows.data(), c->d_m + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(status.data(), c->d_status + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    rc = last_launch(c);
    if (rc) return rc;
    int soft = INGVIO_OK;
    for (int i = 0; i < nb; ++i) {
        if (rows_out) rows_out[i] = rows[i];
        if (rows[i] == 0 && soft == INGVIO_OK) soft = INGVIO_NO_ROWS;
        if (status[i] & 2) soft = INGVIO_NEG_DIAG;
    }
    return nb == 1 ? soft : (soft == INGVIO_NEG_DIAG ? soft : INGVIO_OK);
}

int ingvio_msckf_update(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts,
                        double* dx_out, int* accepted, double* gamma, int* rows_out)
{
    ENTER(c);
    return msckf_update_impl(c, b0, nb, frames, opts, nullptr, nullptr, dx_out, accepted, gamma, rows_out, nullptr, nullptr);
}

int ingvio_msckf_update_tri(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_msckf_opts* opts,
                            const ingvio_tri_opts* tri, const unsigned long long* const* tri_masks, double* dx_out, int* accepted,
                            double* gamma, int* rows_out, double* pf_out, int* tri_ok)
{
    ENTER(c);
    if (!tri) return INGVIO_E_ARG;
    return msckf_update_impl(c, b0, nb, frames, opts, tri, tri_masks, dx_out, accepted, gamma, rows_out, pf_out, tri_ok);
}

// ---- SLAM-landmark covariance operations -------------------------------------------------------
int ingvio_replace_var_linear(ingvio_ctx* c, int b, int tidx, int tsize, const int* vidx, const int* vsize, int k, const double* H, int ldh)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b, 1) || tsize < 1 || tsize > 6) return INGVIO_E_ARG;
    if (tidx < 0 || tidx + tsize > c->h_n[b]) return INGVIO_E_NOT_IN_STATE;       // "Target var not in state" (:653-657)
    int nc = 0;
    const double one = 1.0;
    std::vector<double> zero((size_t)tsize, 0.0);
    int rc = stage_generic(c, b, vidx, vsize, k, H, ldh, tsize, zero.data(), &one, 0, &nc);
    if (rc) return rc;
    if (launch_replace_var(view(c), b, c->d_H + (size_t)b * c->hstride, c->d_colmap + (size_t)b * c->cstride, tidx, tsize, nc, c->mld,
                           c->d_Y + (size_t)b * c->ystride, c->st)) return INGVIO_E_CAPACITY;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return last_launch(c);
}

// Triangulator::triangulate{Mono,Stereo}Obs for every feature of the given (or staged) frames
int ingvio_triangulate(ingvio_ctx* c, int b0, int nb, const ingvio_msckf_frame* frames, const ingvio_tri_opts* o,
                       double* pf_out, int* ok_out)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !o) return INGVIO_E_ARG;
    if (o->outer_loop_max_iter < 0 || o->inner_loop_max_iter < 0) return INGVIO_E_ARG;
    int fmx = c->d.f_max;
    if (frames) {
        const int rc = stage_frames(c, b0, nb, frames, &fmx, -1);      // poses and observations only: no state indices needed
        if (rc) return rc;
        c->strip_ok = false;
    } else if (!c->staged) return INGVIO_E_ARG;
    else if (wait_inputs(c)) return INGVIO_E_HIP;
    TriLaunch L;
    memset(&L, 0, sizeof L);
    L.fv = fview(c); L.b0 = b0;
    memcpy(L.R_lr, o->R_cl2cr, 72); memcpy(L.t_lr, o->t_cl2cr, 24);
    L.trans_thres = o->trans_thres; L.huber_epsilon = o->huber_epsilon; L.conv_precision = o->conv_precision;
    L.init_damping = o->init_damping; L.max_depth = o->max_depth; L.min_depth = o->min_depth;
    L.outer_loop_max_iter = o->outer_loop_max_iter; L.inner_loop_max_iter = o->inner_loop_max_iter;
    L.pf = c->d_pf; L.ok = c->d_tri_ok; L.mask_failed = o->mask_failed ? 1 : 0; L.mask_rw = c->d_mask;
    if (launch_triangulate(L, nb, fmx > 0 ? fmx : 1, o->stereo, c->st)) return INGVIO_E_UNSUPPORTED;
    const int fm = c->d.f_max;
    if (pf_out) HIPCHK(c, hipMemcpyAsync(pf_out, c->d_pf + (size_t)b0 * fm * 3, 8 * (size_t)nb * fm * 3, hipMemcpyDeviceToHost, c->st));
    if (ok_out) HIPCHK(c, hipMemcpyAsync(ok_out, c->d_tri_ok + (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return last_launch(c);
}

// ---------------------------------------------------------------------------------------------------------------------
// Dense-H update: rows already in dw.Hd (by state column), residual in the carried row of dw.X, row counts in dw.m.
//   S = H P H^T (+ noise), Y = P H^T L^-T, z = L^-1 res by one Cholesky sweep with carried rows; dx = Y z; P -= Y Y^T.
// ---------------------------------------------------------------------------------------------------------------------
static int dense_ws_alloc(ingvio_ctx* c, int m_need)
{
    auto& w = c->dw;
    const int m_cap = (m_need + 31) / 32 * 32;
    if (w.Hd && w.m_cap >= m_cap) return 0;
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (double** p : { &w.Hd, &w.X, &w.Y, &w.Tb, &w.U, &w.noise, &w.noiseB }) { if (*p) hipFree(*p); *p = nullptr; }
    if (w.m) { hipFree(w.m); w.m = nullptr; }
    if (w.cidx) { hipFree(w.cidx); w.cidx = nullptr; }
    if (w.rowmap) { hipFree(w.rowmap); w.rowmap = nullptr; }
    const int B = c->d.batch;
    w.m_cap = m_cap; w.n32 = (c->d.n_max + 31) / 32 * 32; w.n_ld = w.n32; w.ldx = m_cap + w.n32 + 32;
    w.hstride = std::max((size_t)m_cap * w.n_ld, (size_t)LM_MAX * 100);      // also holds the landmark path's compact blocks
    w.xstride = (size_t)w.ldx * m_cap;
    // launch_chol_sweep works with at least TWO T slots (kernels_chol.hip): a 32-row workspace used to be sized for one, and the last
    // filter's second slot lay past the allocation (found in round 4 when a change of the allocation order put unmapped memory there)
    w.tstride = (size_t)std::max(m_cap / 32, 2) * 1024 + (size_t)m_cap;
    w.ustride = m_cap <= 256 ? lm_chol_ws_doubles(m_cap) : 0;
    int rc = dalloc(c, &w.Hd, (size_t)B * w.hstride) | dalloc(c, &w.X, (size_t)B * w.xstride) | dalloc(c, &w.Y, (size_t)B * w.xstride)
           | dalloc(c, &w.Tb, (size_t)B * w.tstride) | (w.ustride ? dalloc(c, &w.U, (size_t)B * w.ustride) : 0) | dalloc(c, &w.m, (size_t)B) | dalloc(c, &w.noise, (size_t)m_cap * m_cap) | dalloc(c, &w.cidx, (size_t)B * LM_MAX * 4) | dalloc(c, &w.noiseB, (size_t)B * m_cap)
           | dalloc(c, &w.rowmap, (size_t)B * m_cap);
    return rc ? INGVIO_E_HIP : 0;
}

// noise: r_kind < 0 -> scalar variance `var` on the whole diagonal (the GEMM's epilogue); else d_noise (stride nstride) through k_add_noise
static int run_dense_update(ingvio_ctx* c, int b0, int nb, double var, int r_kind, const double* d_noise, int nstride, double* d_dx, bool products_done,
                            const int* rowmap, const int* marg_idx, int marg_size, bool* marg_fused)
{
    auto& w = c->dw;
    const int mc = w.m_cap, n_cap = c->d.n_max, B = c->d.batch;
    const size_t pp = c->pp;
    double *Hd = w.Hd + (size_t)b0 * w.hstride, *X = w.X + (size_t)b0 * w.xstride, *Y = w.Y + (size_t)b0 * w.xstride;
    const int* act = w.m + b0;
    int form = 0;
    if (!products_done) {
        ProfScope p(c, PF_LM_GEMM);
        GemmArgs g = {};
        // P H^T -> carried rows mc .. of X
        g.A = c->Pbase + (size_t)b0 * pp; g.sa = pp; g.lda = c->ldp; g.modeA = 0; g.a_sel = c->d_cur + b0; g.a_sel_stride = (size_t)B * pp;
        g.B = Hd; g.sb = w.hstride; g.ldb = w.n_ld; g.modeB = 1;
        g.C = X + mc; g.sc = w.xstride; g.rs = 1; g.cs = w.ldx;
        g.M = n_cap; g.N = mc; g.K = n_cap; g.m_lim = n_cap; g.n_lim = mc; g.ksplit = 1; g.active = act; g.batch = nb;
        if (launch_gemm(g, c->st)) form |= INGVIO_UPDATE_GEMM64_PHT;
        // S = H (P H^T), lower blocks
        g = GemmArgs{};
        g.A = Hd; g.sa = w.hstride; g.lda = w.n_ld; g.modeA = 1;
        g.B = X + mc; g.sb = w.xstride; g.ldb = w.ldx; g.modeB = 1;
        g.C = X; g.sc = w.xstride; g.rs = 1; g.cs = w.ldx;
        g.M = mc; g.N = mc; g.K = n_cap; g.m_lim = mc; g.n_lim = mc; g.ksplit = 1; g.lower = 1; g.diag_add = r_kind < 0 ? var : 0.0;
        g.active = act; g.batch = nb;
        if (launch_gemm(g, c->st)) form |= INGVIO_UPDATE_GEMM64_S;
        if (r_kind >= 0) launch_add_noise(X, w.xstride, w.ldx, d_noise, nstride, r_kind, act, mc, nb, c->st);
    }
    // S of up to 256 rows: one workgroup per filter, S in registers (kernels_lmchol.hip); larger: the sweep out of L2 (kernels_chol.hip)
#ifdef INGVIO_ALT_KERNELS
    static const bool sweep_only = getenv("INGVIO_LM_SOLVE") && !strcmp(getenv("INGVIO_LM_SOLVE"), "sweep");
#else
    constexpr bool sweep_only = false;
#endif
    if (w.U && !sweep_only) {
        ProfScope p(c, PF_LM_CHOL);
        LmCholArgs a = {};
        a.cv = view(c); a.b0 = b0; a.nb = nb; a.X = X; a.Y = Y; a.xs = w.xstride; a.ldx = w.ldx; a.mc = mc; a.res_row = mc + w.n32;
        a.U = w.U + (size_t)b0 * w.ustride; a.us = w.ustride; a.m = act; a.status = c->d_status + b0; a.fail_bit = 4; a.dx = d_dx;
        a.rowmap = rowmap; a.rm_stride = mc;
        form |= INGVIO_UPDATE_DENSE_REG | (launch_lm_chol(a, c->st) << INGVIO_UPDATE_NTM_SHIFT);
    } else {
        ProfScope p(c, PF_LM_CHOL);
        CholArgs a = {};
        a.W = X; a.Y = Y; a.xs = w.xstride; a.ld = w.ldx; a.Tb = w.Tb + (size_t)b0 * w.tstride; a.ts = w.tstride; a.t_slots = mc / 32;
        a.rows = w.ldx; a.ncols = mc; a.status = c->d_status + b0; a.fail_bit = 4; a.active = act; a.batch = nb;
        form |= INGVIO_UPDATE_DENSE_SWEEP | (launch_chol_sweep(a, c->st) ? INGVIO_UPDATE_SPLIT_SWEEP : 0);
        launch_lm_finish(view(c), b0, nb, Y, w.xstride, w.ldx, mc, mc + w.n32, act, d_dx, c->d_status, c->st);
    }
    {
        ProfScope p(c, PF_DOWNDATE);
        EkfLaunch E;
        memset(&E, 0, sizeof E);
        E.cv = view(c); E.b0 = b0; E.nb = nb; E.Y = Y + mc; E.m = w.m + b0; E.status = c->d_status; E.m_cap = mc;
        const bool fused = launch_downdate(E, n_cap, c->st, nullptr, w.ldx, w.xstride, marg_idx, marg_size);
        if (marg_fused) *marg_fused = fused;
    }
    c->mut_seq++;
    c->update_form_last = form;
    return last_launch(c);
}

// marg_idx / marg_size (optional): the marginalisation that follows the update in the frame, fused into the write-back where the
// downdate kernel supports it (*marg_fused; the caller then only flips the halves: launch_post_marg)
static int landmark_update_launch(ingvio_ctx* c, int b0, int nb, const int* marg_idx = nullptr, int marg_size = 0, bool* marg_fused = nullptr)
{
    if (marg_fused) *marg_fused = false;
    auto& w = c->dw;
    auto& s = c->lm;
    const int* rowmap = nullptr;
    {
        ProfScope p(c, PF_LM_BUILD);
        LmBuild L;
        memset(&L, 0, sizeof L);
        L.cv = view(c); L.op = s.op; L.b0 = b0; L.nb = nb;
        L.lv.pose = s.pose; L.lv.idx = s.idx; L.lv.n_lm = s.n_lm; L.lv.lm_idx = s.lm_idx; L.lv.anchor_idx = s.anchor_idx;
        L.lv.pf = s.pf; L.lv.uv = s.uv; L.lv.tracked = s.tracked; L.lv.lmax = LM_MAX;
        L.Hd = w.Hd + (size_t)b0 * w.hstride; L.hstride = w.hstride; L.n_ld = w.n_ld; L.m_cap = w.m_cap;
        L.X = w.X + (size_t)b0 * w.xstride; L.xstride = w.xstride; L.ldx = w.ldx; L.res_row = w.m_cap + w.n32;
        L.gamma = s.gamma + (size_t)b0 * LM_MAX; L.accept = s.accept + (size_t)b0 * LM_MAX; L.m_out = w.m + b0; L.dx = s.dx;
        L.cidx = w.cidx + (size_t)b0 * LM_MAX * 4; L.n_rows = w.n32;
        // states of up to 256 rows with the register-resident solve: rows, products and gate in one kernel (k_lm_front), the accepted
        // rows handed on as a row map; otherwise k_lm_build + k_lm_products write the compacted system
#ifdef INGVIO_ALT_KERNELS
        static const bool split_front = getenv("INGVIO_LM_FRONT") && !strcmp(getenv("INGVIO_LM_FRONT"), "split");
        static const bool sweep_only = getenv("INGVIO_LM_SOLVE") && !strcmp(getenv("INGVIO_LM_SOLVE"), "sweep");
#else
        constexpr bool split_front = false, sweep_only = false;
#endif
        if (w.U && !split_front && !sweep_only && launch_lm_front(L, s.l_hi, w.rowmap + (size_t)b0 * w.m_cap, c->st))
            rowmap = w.rowmap + (size_t)b0 * w.m_cap;
        else launch_lm_build(L, c->st);
    }
    return run_dense_update(c, b0, nb, s.op.var, -1, nullptr, 0, s.dx, true, rowmap, marg_idx, marg_size, marg_fused);
}

static int landmark_stage_alloc(ingvio_ctx* c, int l_hi)
{
    auto& s = c->lm;
    const int B = c->d.batch;
    if (!s.alloc) {
        int rc = dalloc(c, &s.pose, (size_t)B * 24) | dalloc(c, &s.pf, (size_t)B * LM_MAX * 3) | dalloc(c, &s.uv, (size_t)B * LM_MAX * 4)
               | dalloc(c, &s.gamma, (size_t)B * LM_MAX) | dalloc(c, &s.idx, (size_t)B * 2) | dalloc(c, &s.n_lm, (size_t)B)
               | dalloc(c, &s.lm_idx, (size_t)B * LM_MAX) | dalloc(c, &s.anchor_idx, (size_t)B * LM_MAX) | dalloc(c, &s.tracked, (size_t)B * LM_MAX)
               | dalloc(c, &s.accept, (size_t)B * LM_MAX) | dalloc(c, &s.dx, (size_t)B * c->ldp);
        if (rc) return INGVIO_E_HIP;
        s.alloc = true;
    }
    if (c->nom.vmax && !s.slot && dalloc(c, &s.slot, (size_t)B * LM_MAX)) return INGVIO_E_HIP;
    s.l_hi = std::max(s.l_hi, l_hi);
    return dense_ws_alloc(c, std::max(32, 4 * s.l_hi));
}

static void landmark_stage_commit(ingvio_ctx* c, int b0, int nb, const ingvio_landmark_opts* o, const std::vector<int>& hi_new)
{
    auto& s = c->lm;
    memcpy(s.op.R_lr, o->R_cl2cr, 72); memcpy(s.op.t_lr, o->t_cl2cr, 24);
    s.op.var = o->noise * o->noise; s.op.chi2_thr = o->chi2_thr; s.op.stereo = o->stereo ? 1 : 0;
    s.in_frame = o->in_frame ? 1 : 0;
    if ((int)s.hi.size() != c->d.batch) s.hi.assign(c->d.batch, 0);
    for (int i = 0; i < nb; ++i) s.hi[b0 + i] = hi_new[i];
    s.staged = true;
}

int ingvio_landmark_stage(ingvio_ctx* c, int b0, int nb, const ingvio_landmark_frame* fr, const ingvio_landmark_opts* o)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !fr || !o || !(o->noise > 0.0)) return INGVIO_E_ARG;
    auto& s = c->lm;
    int l_hi = 0;
    std::vector<int> hi_new(nb, 0);
    for (int i = 0; i < nb; ++i) {
        const auto& f = fr[i];
        if (f.n_lm < 0 || f.n_lm > LM_MAX) return INGVIO_E_CAPACITY;
        if (f.n_lm && (!f.lm_idx || !f.anchor_idx || !f.pf || !f.uv || !f.tracked)) return INGVIO_E_ARG;
        // every variable must lie inside the filter's LIVE state at update time (in_frame: the frame step appends the 6-column clone
        // first), not merely inside the buffer - rows beyond it would read stale covariance
        const int n_lim = std::min(c->d.n_max, c->h_n[b0 + i] + (o->in_frame ? 6 : 0));
        if (f.idx_epose < 0 || f.idx_epose + 9 > n_lim || f.idx_ext < 0 || f.idx_ext + 6 > n_lim) return INGVIO_E_NOT_IN_STATE;
        for (int l = 0; l < f.n_lm; ++l)
            if (f.lm_idx[l] < 0 || f.lm_idx[l] + 3 > n_lim || f.anchor_idx[l] < 0 || f.anchor_idx[l] + 6 > n_lim) return INGVIO_E_NOT_IN_STATE;
        int hi = f.n_lm ? std::max(f.idx_epose + 9, f.idx_ext + 6) : 0;
        for (int l = 0; l < f.n_lm; ++l) hi = std::max(hi, std::max(f.lm_idx[l] + 3, f.anchor_idx[l] + 6));
        hi_new[i] = hi;
        l_hi = std::max(l_hi, f.n_lm);
    }
    const int B = c->d.batch;
    if (int rc = landmark_stage_alloc(c, l_hi)) return rc;
    Uploader upl{ c };
    if (int rc = upl.begin(pad64(8 * (size_t)nb * (24 + 7 * LM_MAX)) + pad64(4 * (size_t)nb * (3 + 3 * LM_MAX)) + 1024)) return rc;
    double* hp = upl.take<double>((size_t)nb * 24);
    double* hpf = upl.take<double>((size_t)nb * LM_MAX * 3);
    double* huv = upl.take<double>((size_t)nb * LM_MAX * 4);
    int* hidx = upl.take<int>((size_t)nb * 2);
    int* hn = upl.take<int>((size_t)nb);
    int* hl = upl.take<int>((size_t)nb * LM_MAX);
    int* ha = upl.take<int>((size_t)nb * LM_MAX);
    int* ht = upl.take<int>((size_t)nb * LM_MAX);
    for (int i = 0; i < nb; ++i) {
        const auto& f = fr[i];
        memcpy(hp + 24 * i, f.R_i2w, 72); memcpy(hp + 24 * i + 9, f.p_i2w, 24); memcpy(hp + 24 * i + 12, f.R_cl2i, 72); memcpy(hp + 24 * i + 21, f.p_c2i, 24);
        hidx[2 * i] = f.idx_epose; hidx[2 * i + 1] = f.idx_ext; hn[i] = f.n_lm;
        for (int l = 0; l < LM_MAX; ++l) {
            const bool on = l < f.n_lm;
            hl[i * LM_MAX + l] = on ? f.lm_idx[l] : -1; ha[i * LM_MAX + l] = on ? f.anchor_idx[l] : -1; ht[i * LM_MAX + l] = on ? f.tracked[l] : 0;
            for (int k = 0; k < 3; ++k) hpf[((size_t)i * LM_MAX + l) * 3 + k] = on ? f.pf[3 * l + k] : 0.0;
            for (int k = 0; k < 4; ++k) huv[((size_t)i * LM_MAX + l) * 4 + k] = on ? ((o->stereo || k < 2) ? f.uv[4 * l + k] : 0.0) : 0.0;
        }
    }
    upl.copy(s.pose + (size_t)b0 * 24, hp, (size_t)nb * 24);
    upl.copy(s.pf + (size_t)b0 * LM_MAX * 3, hpf, (size_t)nb * LM_MAX * 3);
    upl.copy(s.uv + (size_t)b0 * LM_MAX * 4, huv, (size_t)nb * LM_MAX * 4);
    upl.copy(s.idx + (size_t)b0 * 2, hidx, (size_t)nb * 2);
    upl.copy(s.n_lm + b0, hn, (size_t)nb);
    upl.copy(s.lm_idx + (size_t)b0 * LM_MAX, hl, (size_t)nb * LM_MAX);
    upl.copy(s.anchor_idx + (size_t)b0 * LM_MAX, ha, (size_t)nb * LM_MAX);
    upl.copy(s.tracked + (size_t)b0 * LM_MAX, ht, (size_t)nb * LM_MAX);
    if (int rc = upl.end()) return rc;
    landmark_stage_commit(c, b0, nb, o, hi_new);
    s.nominal = false; s.nom_pending = false;      // (replaces a stage from the device nominal state that has not run)
    return INGVIO_OK;
}

// ingvio_landmark_stage with everything but the observations taken from the device nominal table.  Validated on the host
// mirror of the table's integer records, before anything changes; the upload (uv, tracked, n_lm, the table slots) goes to the compute
// stream, behind the kernels of the frame enqueued last that still read the staged arrays.
int ingvio_landmark_stage_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_landmark_frame_nominal* fr, const ingvio_landmark_opts* o)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !fr || !o || !(o->noise > 0.0)) return INGVIO_E_ARG;
    auto& s = c->lm;
    auto& m = c->nom;
    const int B = c->d.batch;
    if (!m.vmax) { c->err = "ingvio_landmark_stage_nominal without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (o->in_frame) {
        if (!m.pending) { c->err = "ingvio_landmark_stage_nominal(in_frame): no frame staged from the device nominal state is waiting to run"; return INGVIO_E_ARG; }
        if (b0 != 0 || nb != B) { c->err = "ingvio_landmark_stage_nominal(in_frame) stages the whole batch (b0 = 0, nb = batch)"; return INGVIO_E_ARG; }
    } else if (m.pending) {
        c->err = "ingvio_landmark_stage_nominal: a frame staged from the device nominal state has not run yet (in_frame = 0)"; return INGVIO_E_ARG;
    }
    if (c->gn.nom_pending) { c->err = "ingvio_landmark_stage_nominal: a GNSS epoch staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    int l_hi = 0;
    std::vector<int> hi_new(nb, 0);
    for (int i = 0; i < nb; ++i) {
        const auto& f = fr[i];
        const int b = b0 + i;
        if (f.n_lm < 0 || f.n_lm > LM_MAX) return INGVIO_E_CAPACITY;
        if (f.n_lm && (!f.lm_var || !f.uv || !f.tracked)) return INGVIO_E_ARG;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        if (I[NOM_V_POSE] < 0 || I[NOM_V_EXT] < 0) { c->err = "ingvio_landmark_stage_nominal: the table names no extended pose or extrinsics"; return INGVIO_E_ARG; }
        // (in_frame: the stage of the frame has already put the new clone into the mirror, its 6 columns are appended by the run -
        // unless the frame is an update-only one, which appends none)
        const int n_lim = std::min(c->d.n_max, c->h_n[b] + (o->in_frame && !m.noprop ? 6 : 0));
        const int ie = var[4 * I[NOM_V_POSE] + 1], ix = var[4 * I[NOM_V_EXT] + 1];
        if (ie < 0 || ie + 9 > n_lim || ix < 0 || ix + 6 > n_lim) return INGVIO_E_NOT_IN_STATE;
        int hi = f.n_lm ? std::max(ie + 9, ix + 6) : 0;
        for (int l = 0; l < f.n_lm; ++l) {
            const int v = f.lm_var[l];
            if (v < 0 || v >= I[NOM_N_VAR] || var[4 * v] != NOM_KIND_LM) { c->err = "ingvio_landmark_stage_nominal: a slot is free or holds no landmark"; return INGVIO_E_ARG; }
            for (int t = 0; t < l; ++t) if (f.lm_var[t] == v) { c->err = "ingvio_landmark_stage_nominal: a slot is named twice"; return INGVIO_E_ARG; }
            const int as = var[4 * v + 2], il = var[4 * v + 1], ia = as >= 0 && as < I[NOM_N_VAR] ? var[4 * as + 1] : -1;
            if (il < 0 || il + 3 > n_lim || ia < 0 || ia + 6 > n_lim) return INGVIO_E_NOT_IN_STATE;
            hi = std::max(hi, std::max(il + 3, ia + 6));
        }
        hi_new[i] = hi;
        l_hi = std::max(l_hi, f.n_lm);
    }
    if (int rc = landmark_stage_alloc(c, l_hi)) return rc;
    Uploader upl{ c };
    if (int rc = upl.begin(pad64(8 * (size_t)nb * 4 * LM_MAX) + pad64(4 * (size_t)nb * (1 + 2 * LM_MAX)) + 1024)) return rc;
    double* huv = upl.take<double>((size_t)nb * LM_MAX * 4);
    int* hn = upl.take<int>((size_t)nb);
    int* hs = upl.take<int>((size_t)nb * LM_MAX);
    int* ht = upl.take<int>((size_t)nb * LM_MAX);
    for (int i = 0; i < nb; ++i) {
        const auto& f = fr[i];
        hn[i] = f.n_lm;
        for (int l = 0; l < LM_MAX; ++l) {
            const bool on = l < f.n_lm;
            hs[i * LM_MAX + l] = on ? f.lm_var[l] : -1; ht[i * LM_MAX + l] = on ? f.tracked[l] : 0;
            for (int k = 0; k < 4; ++k) huv[((size_t)i * LM_MAX + l) * 4 + k] = on ? ((o->stereo || k < 2) ? f.uv[4 * l + k] : 0.0) : 0.0;
        }
    }
    upl.copy(s.uv + (size_t)b0 * LM_MAX * 4, huv, (size_t)nb * LM_MAX * 4);
    upl.copy(s.n_lm + b0, hn, (size_t)nb);
    upl.copy(s.slot + (size_t)b0 * LM_MAX, hs, (size_t)nb * LM_MAX);
    upl.copy(s.tracked + (size_t)b0 * LM_MAX, ht, (size_t)nb * LM_MAX);
    if (int rc = upl.end()) return rc;
    landmark_stage_commit(c, b0, nb, o, hi_new);
    s.nominal = true; s.nom_pending = !o->in_frame; s.nom_b0 = b0; s.nom_nb = nb;
    return INGVIO_OK;
}

// the staged arrays' pose / idx / lm_idx / anchor_idx / pf from the table (dx != nullptr: after boxPlus of dx, in the same launch)
static void landmark_gather_launch(ingvio_ctx* c, const double* dx, int b0, int nb)
{
    auto& s = c->lm;
    NomGather g;
    g.n_lm = s.n_lm; g.slot = s.slot; g.lmax = LM_MAX;
    g.pose = s.pose; g.idx = s.idx; g.lm_idx = s.lm_idx; g.anchor_idx = s.anchor_idx; g.pf = s.pf;
    launch_nominal_gather(nom_table(c), dx, c->ldp, g, b0, nb, c->st);
}

// The staged landmark rows name state columns: a marginalisation between stage and run may have shrunk or shifted the state,
// so every run re-validates them against the live dimension (as ingvio_gnss_run does with its staged var_order).
static int landmark_in_state(ingvio_ctx* c, int b0, int nb, const std::vector<int>& n_live, int extra)
{
    if ((int)c->lm.hi.size() != c->d.batch) return INGVIO_OK;
    for (int b = b0; b < b0 + nb; ++b)
        if (c->lm.hi[b] > n_live[b] + extra) { c->err = "a staged landmark row names a column beyond the live state"; return INGVIO_E_NOT_IN_STATE; }
    return INGVIO_OK;
}

int ingvio_landmark_run(ingvio_ctx* c, int b0, int nb)
{
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (check_range(c, b0, nb) || !c->lm.staged) return INGVIO_E_ARG;
    auto& s = c->lm;
    if (s.nominal) {                               // staged from the device nominal state: the range it was staged for, once
        if (s.in_frame) { c->err = "ingvio_landmark_run: the stage belongs to a frame staged from the device nominal state (ingvio_frame_run applies it)"; return INGVIO_E_ARG; }
        if (!s.nom_pending || b0 != s.nom_b0 || nb != s.nom_nb) { c->err = "ingvio_landmark_run: a stage from the device nominal state runs once, on the range it was staged for"; return INGVIO_E_ARG; }
        if (c->nom.pending) { c->err = "ingvio_landmark_run: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    }
    if (int rc = landmark_in_state(c, b0, nb, c->h_n, 0)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_status + b0, 0, sizeof(int) * (size_t)nb, c->st));
    if (!s.nominal) return landmark_update_launch(c, b0, nb);
    // rows at the table as it stands, the update, then StateManager::boxPlus of its dx on the table (LandmarkUpdate.cpp:146-147)
    s.nom_pending = false; s.staged = false;       // consumed: the table moves with this run, a second one is refused
    landmark_gather_launch(c, nullptr, b0, nb);
    if (int rc = landmark_update_launch(c, b0, nb)) return rc;
    launch_nominal_update(nom_table(c), s.dx, c->ldp, nullptr, b0, nb, c->st);
    if (int rc = last_launch(c)) return rc;
    return nom_mark(c) ? INGVIO_E_HIP : INGVIO_OK;
}

int ingvio_landmark_fetch(ingvio_ctx* c, int b0, int nb, double* dx, int* rows, int* accept, double* gamma, int* status)
{
    ENTER(c);
    if (check_range(c, b0, nb) || !c->lm.alloc) return INGVIO_E_ARG;
    if (dx) HIPCHK(c, hipMemcpyAsync(dx, c->lm.dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
    if (rows) HIPCHK(c, hipMemcpyAsync(rows, c->dw.m + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
    if (accept) HIPCHK(c, hipMemcpyAsync(accept, c->lm.accept + (size_t)b0 * LM_MAX, sizeof(int) * (size_t)nb * LM_MAX, hipMemcpyDeviceToHost, c->st));
    if (gamma) HIPCHK(c, hipMemcpyAsync(gamma, c->lm.gamma + (size_t)b0 * LM_MAX, 8 * (size_t)nb * LM_MAX, hipMemcpyDeviceToHost, c->st));
    if (status) HIPCHK(c, hipMemcpyAsync(status, c->d_status + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (status) for (int i = 0; i < nb; ++i) status[i] = soft_status(status[i]);   // bit 4: S not positive definite
    return last_launch(c);
}

int ingvio_set_qr_method(ingvio_ctx* c, int method)
{
    ENTER(c);
    if (!c || method < 0 || method > 2) return INGVIO_E_ARG;
    c->qr_method = method;
    return INGVIO_OK;
}

int ingvio_qr_compress(ingvio_ctx* c, const double* H, int ldh, int m, int n, const double* res, double* Ht, int ldt, double* rt)
{
    ENTER(c);
    if (!c || !H || !res || !Ht || !rt || m < 1 || n < 1 || ldh < m || ldt < n) return INGVIO_E_ARG;
    // Every shape takes the blocked Householder QR of kernels_qr.hip (device buffers and the launch graph cached per shape): no
    // per-call allocation and no use of any filter's staging buffers - a drop-in for six SPQR call sites must not touch batch state.
    // Matrices taller than 6144 rows are factorised in row chunks (launch_qr_dense).
    {
    if (n > 4096) return INGVIO_E_CAPACITY;
    auto& q = c->qr;
    // Every tall stack (m >= 6 n: the stacked MSCKF rows 6150 x 66 and 35100 x 180, the 6000 x 800 stress shape) takes Cholesky-QR,
    // measured 10 - 40 x faster than the blocked Householder QR on all three (profiles/r03_qr_shapes.json: 0.088 / 0.228 / 0.436 ms
    // against 0.85 / 9.0 / 7.2 ms); Householder keeps the shapes that are not tall, where forming the Gram matrix buys nothing.
    // ekfUpdate reads nothing but R^T R and R^T z (exact to eps |H|^2 either way); entry by entry R carries cond(H)^2 eps.
    const int chol = c->qr_method == 2 || (c->qr_method == 0 && (long long)m >= 6LL * n);
    if (q.m != m || q.n != n || q.ldh != ldh || q.chol != chol) {                      // new shape: buffers and the launch graph are rebuilt
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (q.exec) { hipGraphExecDestroy(q.exec); q.exec = nullptr; }
        for (double** p : { &q.dA, &q.db, &q.ws, &q.dT }) { if (*p) hipFree(*p); *p = nullptr; }
        q.m = q.n = q.ldh = 0;
        HIPCHK(c, hipMalloc((void**)&q.dA, 8 * (size_t)ldh * n));
        HIPCHK(c, hipMalloc((void**)&q.db, 8 * (size_t)m));
        const size_t wsd = chol ? qr_chol_workspace_doubles(m, n) : qr_dense_workspace_doubles(m, n);
        HIPCHK(c, hipMalloc((void**)&q.ws, 8 * wsd));
        HIPCHK(c, hipMemsetAsync(q.ws, 0, 8 * wsd, c->st));
        HIPCHK(c, hipMalloc((void**)&q.dT, 8 * ((size_t)n * n + n)));
        // the factorisation is a fixed sequence of 3 launches per 8-column panel: captured once, replayed as one graph
        hipGraph_t g = nullptr;
        HIPCHK(c, hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
        const int lrc = chol ? launch_qr_chol(q.dA, ldh, q.db, m, n, q.ws, q.dT, n, q.dT + (size_t)n * n, c->st)
                             : launch_qr_dense(q.dA, ldh, q.db, m, n, q.ws, q.dT, n, q.dT + (size_t)n * n, c->st);
        const hipError_t ce = hipStreamEndCapture(c->st, &g);
        if (lrc) { if (g) hipGraphDestroy(g); return INGVIO_E_CAPACITY; }
        if (ce != hipSuccess || !g) { c->err = "hipStreamEndCapture failed"; return INGVIO_E_HIP; }
        const hipError_t ie = hipGraphInstantiate(&q.exec, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (ie != hipSuccess) { q.exec = nullptr; c->err = "hipGraphInstantiate failed"; return INGVIO_E_HIP; }
        q.m = m; q.n = n; q.ldh = ldh; q.chol = chol;
    }
    int rc2 = up(c, q.dA, H, 8 * (size_t)ldh * n) | up(c, q.db, res, 8 * (size_t)m);
    if (!rc2) {
        ProfScope p(c, PF_FOLD);
        if (hipGraphLaunch(q.exec, c->st) != hipSuccess) rc2 = INGVIO_E_HIP;
    }
    if (!rc2) {
        double* dT = q.dT;
        if (ldt == n) rc2 = hipMemcpyAsync(Ht, dT, 8 * (size_t)n * n, hipMemcpyDeviceToHost, c->st) != hipSuccess;
        else rc2 = hipMemcpy2DAsync(Ht, 8 * (size_t)ldt, dT, 8 * (size_t)n, 8 * (size_t)n, n, hipMemcpyDeviceToHost, c->st) != hipSuccess;
        rc2 |= hipMemcpyAsync(rt, dT + (size_t)n * n, 8 * (size_t)n, hipMemcpyDeviceToHost, c->st) != hipSuccess;
        if (rc2) rc2 = INGVIO_E_HIP;
    }
    hipStreamSynchronize(c->st);
    if (rc2) return rc2 < 0 ? rc2 : INGVIO_E_HIP;
    return last_launch(c);
    }
}

// launch_propagate's IMU arguments for filters [b0, b0 + nb): k and the noise as scalar kernel arguments when every filter of the launch
// shares them (the headline case: k is then no memory round trip in front of the kernel), else prm = the filters' blocks (k_propagate<.., true>)
struct ImuLaunch { int k; double sigma[4], scb, srw; const double* prm; };
static ImuLaunch imu_launch(const ingvio_ctx* c, int b0, int nb)
{
    const double* h = &c->st_prm[(size_t)b0 * 8];
    ImuLaunch L{ (int)h[6], { h[0], h[1], h[2], h[3] }, h[4], h[5], nullptr };
    for (int i = 1; i < nb; ++i)
        if (memcmp(h, h + (size_t)i * 8, 7 * sizeof(double))) { L.prm = c->d_prm + (size_t)b0 * 8; break; }
    return L;
}

static int frame_stage_impl(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step* steps, const ingvio_msckf_frame* frames,
                            const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw, bool async)
{
    FrameStage stage{ c, b0, nb, opts, sigma, enable_gnss, scb, srw, async };
    if (int rc = stage.refuse(steps && frames, false)) return rc;
    int k = 0;                                                              // the call's largest step count: the slab's stride
    for (int i = 0; i < nb; ++i) {
        if (steps[i].k < 1 || steps[i].k > KMAX || !steps[i].Phi || !steps[i].G || !steps[i].dt) return INGVIO_E_ARG;
        if (steps[i].k > k) k = steps[i].k;
    }
    int fmx = 0;
    // clone indices are checked against the buffer only (grow < 0): the live size at run time depends on whether the run
    // restores the snapshot; ingvio_frame_run checks them against the live state before its first launch
    if (int rc = validate_frames(c, b0, nb, frames, -1, &fmx)) return rc;
    const size_t n = nb;
    if (int rc = stage.begin(pad64(8 * n * k * 225) + pad64(8 * n * k * 180) + pad64(8 * n * k) + pad64(8 * n * 9) + pad64(4 * n * 5) + pad64(4 * n) +
                             frames_bytes(c, nb))) return rc;
    if (int rc = stage.commit(steps)) return rc;
    // everything goes through ONE pinned slab: packed by a few host threads, copied asynchronously, no stream sync.  Filter i's steps
    // sit k (the call's largest count) apart in the slab and KMAX apart on the device: one strided copy each for Phi, G and dt
    Uploader& upl = stage.upl;
    double* Phi = upl.take<double>(n * k * 225); double* G = upl.take<double>(n * k * 180); double* dt = upl.take<double>(n * k);
    double* R = upl.take<double>(n * 9); int* gi = upl.take<int>(n * 5); int* mi = upl.take<int>(n);
    parallel_for(nb, [=](int i) {
        const size_t ki = steps[i].k;
        memcpy(Phi + (size_t)i * k * 225, steps[i].Phi, 8 * ki * 225);
        memcpy(G + (size_t)i * k * 180, steps[i].G, 8 * ki * 180);
        memcpy(dt + (size_t)i * k, steps[i].dt, 8 * ki);
        memcpy(R + (size_t)i * 9, steps[i].R_i2w, 72);
        for (int g = 0; g < 5; ++g) gi[(size_t)i * 5 + g] = steps[i].gnss_idx[g];
        mi[i] = steps[i].marg_idx;
    });
    upl.copy_rows(c->d_Phi + (size_t)b0 * KMAX * 225, (size_t)KMAX * 225, Phi, (size_t)k * 225, (size_t)k * 225, n);
    upl.copy_rows(c->d_G + (size_t)b0 * KMAX * 180, (size_t)KMAX * 180, G, (size_t)k * 180, (size_t)k * 180, n);
    upl.copy_rows(c->d_dt + (size_t)b0 * KMAX, (size_t)KMAX, dt, (size_t)k, (size_t)k, n);
    stage.upload_imu(steps);
    upl.copy(c->d_R + (size_t)b0 * 9, R, n * 9);
    upl.copy(c->d_gnss + (size_t)b0 * 5, gi, n * 5);
    upl.copy(c->d_idx + b0, mi, n);
    stage.upload_gate();
    pack_frames(c, upl, b0, nb, frames, &fmx);
    return stage.finish(steps, frames, fmx);
}

// ---- device-resident track store ---------------------------------------------------------------------------------------------
int ingvio_tracks_create(ingvio_ctx* c, int t_max)
{
    ENTER(c);
    if (!c || t_max < 1 || t_max > 65536) return INGVIO_E_ARG;
    if (c->d.c_max > 64) return INGVIO_E_UNSUPPORTED;
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
    auto& t = c->trk;
    const size_t B = c->d.batch, T = t_max, C = c->d.c_max, F = c->d.f_max;
    if (t.t_max != t_max) {
        for (void* p : { (void*)t.uv, (void*)t.pf, (void*)t.mask, (void*)t.has, (void*)t.stage[0], (void*)t.stage[1] }) if (p) hipFree(p);
        t = ingvio_ctx::Tracks();
        if (dalloc(c, &t.uv, B * T * C * 4) || dalloc(c, &t.pf, B * T * 3) || dalloc(c, &t.mask, B * T) || dalloc(c, &t.has, B * T)) return INGVIO_E_HIP;
        // worst case of one staged delta per filter: header + ints (drop C, free T, obs T, pf T, clone idx C, features F, gnss 5) +
        // masks F + doubles (obs 4 T, points 3 T, clone poses 12 C, IMU 7 KMAX, state 24)
        t.stage_cap = B * (4 * (TRK_HDR + 3 * T + 2 * C + F + 8) + 8 * F + 8 * (7 * T + 12 * C + 7 * KMAX + 24) + 256) + 4096;
        if (dalloc(c, &t.stage[0], t.stage_cap) || dalloc(c, &t.stage[1], t.stage_cap)) return INGVIO_E_HIP;
        t.t_max = t_max;
    } else {
        HIPCHK(c, hipMemsetAsync(t.mask, 0, 8 * B * T, c->st));
        HIPCHK(c, hipMemsetAsync(t.pf, 0, 8 * B * T * 3, c->st));
        HIPCHK(c, hipMemsetAsync(t.has, 0, B * T, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return INGVIO_OK;
}

// plan [nb][4] (device nominal stage, else nullptr): the new clone's variable slot, its idx, the window's clone count with it and the
// table's slots in use after it; frames[i].n_clones is that count, the frames' clone arrays are not read
// tg with noprop = true (upd; with a plan; the update-only frame from the table, ingvio_update_stage_tracks_nominal): steps[i].k = 0 and no IMU samples, nothing is
// propagated and no clone is appended - plan [nb][4] = -1, the window's highest clone idx, its clone count, the table's slots in use;
// tri_mask / tri_track: where the gather leaves the triangulation's masks and the features' tracks (nullptr: no triangulation)
// tg with noprop = false (with a plan, the ordinary frame from the table that triangulates, ingvio_frame_stage_tracks_nominal_tri): the
// gather leaves the same two arrays; tg->at_stage != nullptr: k_triangulate with these settings and k_tracks_store_points follow the
// gather on the stage's stream
// (both are one TableStage: noprop tells the update-only frame from the ordinary one that triangulates)
struct TableStage { bool noprop; unsigned long long* tri_mask; int* tri_track; const ingvio_tri_opts* at_stage; };

// The buffers a triangulating frame from the table leaves its masks, tracks and (at_stage) flags and points in, allocated by the first
// stage that needs them.  dalloc clears on the compute stream while the stage's kernels may write them on the copy stream, and no event
// orders the two at a context's first stage: a fresh allocation synchronises the compute stream, once.  Nothing else of the context changes.
static int tri_buffers(ingvio_ctx* c, bool at_stage)
{
    auto& m = c->nom;
    const size_t cnt = (size_t)c->d.batch * c->d.f_max;
    bool fresh = false;
    if (!c->d_tri_mask) { if (dalloc(c, &c->d_tri_mask, cnt)) return INGVIO_E_HIP; fresh = true; }
    if (!m.d_tri_track) { if (dalloc(c, &m.d_tri_track, cnt)) return INGVIO_E_HIP; fresh = true; }
    if (at_stage && !m.d_tri_ok_st) { if (dalloc(c, &m.d_tri_ok_st, cnt)) return INGVIO_E_HIP; fresh = true; }
    if (at_stage && !m.d_tri_pf_st) { if (dalloc(c, &m.d_tri_pf_st, cnt * 3)) return INGVIO_E_HIP; fresh = true; }
    if (fresh) HIPCHK(c, hipStreamSynchronize(c->st));
    return 0;
}

// The triangulation of a frame from the table on stream st: the listed features' points from every stored observation (the masks
// k_tracks_gather_upd left in d_tri_mask), with the settings of ingvio_msckf_update_tri - a feature that fails loses its mask and drops out
// of the gate - flags and points also into ok2 / pf2 [B][f_max], and the points that succeeded into the track store (setValuePosXyz,
// MapServerManager.cpp:335).  No host synchronisation.
static int nom_triangulate(ingvio_ctx* c, hipStream_t st, int* ok2, double* pf2)
{
    const int B = c->d.batch;
    const ingvio_tri_opts& o = c->nom.tri;
    TriLaunch T;
    memset(&T, 0, sizeof T);
    T.fv = fview(c); T.b0 = 0;
    memcpy(T.R_lr, o.R_cl2cr, 72); memcpy(T.t_lr, o.t_cl2cr, 24);
    T.trans_thres = o.trans_thres; T.huber_epsilon = o.huber_epsilon; T.conv_precision = o.conv_precision;
    T.init_damping = o.init_damping; T.max_depth = o.max_depth; T.min_depth = o.min_depth;
    T.outer_loop_max_iter = o.outer_loop_max_iter; T.inner_loop_max_iter = o.inner_loop_max_iter;
    T.pf = c->d_pf; T.ok = c->d_tri_ok; T.mask_failed = 1; T.mask_rw = c->d_mask; T.check_anchor = 1;
    T.ok2 = ok2; T.pf2 = pf2;
    T.tri_mask = c->d_tri_mask;
    if (launch_triangulate(T, B, c->nom.tri_fmx > 0 ? c->nom.tri_fmx : 1, o.stereo, st)) return INGVIO_E_UNSUPPORTED;
    const TrackStore store = track_store(c);
    launch_tracks_store_points(store, 0, B, c->d_nfeat, c->d.f_max, c->nom.d_tri_track, ok2, pf2, st);
    return 0;
}

static int frame_stage_tracks_impl(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step_raw* steps, const ingvio_track_frame* frames,
                                   const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw, int async,
                                   const int* plan, const TableStage* tg = nullptr)
{
    const bool upd = tg && tg->noprop;
    FrameStage stage{ c, b0, nb, opts, sigma, enable_gnss, scb, srw, async != 0 };
    if (int rc = stage.refuse(steps && frames, true)) return rc;
    const int T = c->trk.t_max, cm = c->d.c_max, fm = c->d.f_max;
    // ---- layout (counts only), then validation + packing per filter on a few host threads; nothing of the context is touched before
    //      every filter's delta has been found consistent (the pinned slab is scratch) ----
    std::vector<int> hdr((size_t)nb * TRK_HDR, 0);
    size_t ni = 0, nd = 0, nm = 0;
    int fmx = 0;
    for (int i = 0; i < nb; ++i) {
        const ingvio_track_frame& f = frames[i];
        const ingvio_frame_step_raw& s = steps[i];
        if (upd ? s.k != 0 : (s.k < 1 || s.k > KMAX || !s.imu)) return INGVIO_E_ARG;
        if (f.n_drop < 0 || f.n_drop > cm || f.n_free < 0 || f.n_free > T || f.n_obs < 0 || f.n_obs > T || f.n_pf < 0 || f.n_pf > T) return INGVIO_E_CAPACITY;
        if (f.n_clones < 0 || f.n_clones > cm || f.n_feat < 0 || f.n_feat > fm) return INGVIO_E_CAPACITY;
        if ((f.n_drop && !f.drop_slots) || (f.n_free && !f.free_tracks) || (f.n_obs && (!f.obs_track || !f.obs_uv)) || (f.n_pf && (!f.pf_track || !f.pf)) ||
            (f.n_clones && !plan && (!f.clone_idx || !f.clone_R || !f.clone_p)) || (f.n_feat && (!f.feat_track || !f.feat_anchor || !f.feat_dof))) return INGVIO_E_ARG;
        if (f.append_slot >= cm || (f.n_obs > 0 && f.append_slot < 0)) return INGVIO_E_ARG;
        if (f.n_feat > fmx) fmx = f.n_feat;
        int* h = &hdr[(size_t)i * TRK_HDR];
        h[TRK_N_DROP] = f.n_drop; h[TRK_APPEND] = f.append_slot; h[TRK_N_OBS] = f.n_obs; h[TRK_N_FREE] = f.n_free; h[TRK_N_PF] = f.n_pf;
        h[TRK_N_CLONES] = f.n_clones; h[TRK_N_FEAT] = f.n_feat; h[TRK_K] = s.k; h[TRK_HAS_SEL] = f.feat_sel ? 1 : 0; h[TRK_MARG] = s.marg_idx;
        h[TRK_OFF_I] = (int)ni; h[TRK_OFF_D] = (int)nd; h[TRK_OFF_M] = (int)nm;
        if (plan) { h[TRK_NOM_SLOT] = plan[4 * i]; h[TRK_NOM_IDX] = plan[4 * i + 1]; h[TRK_NOM_NVAR] = plan[4 * i + 3]; h[TRK_NOM_CLK] = enable_gnss ? 1 : 0; }
        int oi = 0, od = 0;
        h[TRK_I_DROP] = oi; oi += f.n_drop;
        h[TRK_I_FREE] = oi; oi += f.n_free;
        h[TRK_I_OBS] = oi; oi += f.n_obs;
        h[TRK_I_PF] = oi; oi += f.n_pf;
        const int nct = plan ? 0 : f.n_clones;          // from the device table: neither the clone table nor the start state travel
        h[TRK_I_CIDX] = oi; oi += nct;
        h[TRK_I_FEAT] = oi; oi += f.n_feat;
        h[TRK_I_GNSS] = oi; oi += 5;
        od = (od + 3) & ~3; h[TRK_D_OBS] = od; od += 4 * f.n_obs;                 // 32-byte aligned: read as double4
        h[TRK_D_PF] = od; od += 3 * f.n_pf;
        h[TRK_D_CR] = od; od += 9 * nct;
        h[TRK_D_CP] = od; od += 3 * nct;
        h[TRK_D_IMU] = od; od += 7 * s.k;
        h[TRK_D_STATE] = od; od += plan ? 0 : 24;
        ni += (size_t)oi; nd += ((size_t)od + 3) & ~(size_t)3;
        if (f.feat_sel) nm += (size_t)f.n_feat;
    }
    const size_t off_i = pad64(4 * (size_t)nb * TRK_HDR), off_m = off_i + pad64(4 * ni), off_d = off_m + pad64(8 * nm), total = off_d + pad64(8 * nd);
    if (total > c->trk.stage_cap) return INGVIO_E_CAPACITY;
    if (int rc = stage.begin(total)) return rc;
    Uploader& upl = stage.upl;
    char* slab = upl.take<char>(total);
    int* hp = reinterpret_cast<int*>(slab);
    int* ipool = reinterpret_cast<int*>(slab + off_i);
    unsigned long long* mpool = reinterpret_cast<unsigned long long*>(slab + off_m);
    double* dpool = reinterpret_cast<double*>(slab + off_d);
    memcpy(hp, hdr.data(), 4 * hdr.size());
    const int* hd = hdr.data();
    const int n_max = c->d.n_max;
    std::vector<int> bad((size_t)nb, 0);
    int* badp = bad.data();
    parallel_for(nb, [=](int i) {
        const ingvio_track_frame& f = frames[i];
        const ingvio_frame_step_raw& s = steps[i];
        const int* h = hd + (size_t)i * TRK_HDR;
        int* ip = ipool + h[TRK_OFF_I];
        double* dp = dpool + h[TRK_OFF_D];
        int err = 0;
        for (int q = 0; q < f.n_drop; ++q) if (f.drop_slots[q] < 0 || f.drop_slots[q] >= cm || (q && f.drop_slots[q] <= f.drop_slots[q - 1])) err = 1;
        for (int q = 0; q < f.n_free; ++q) if (f.free_tracks[q] < 0 || f.free_tracks[q] >= T) err = 1;
        for (int q = 0; q < f.n_obs; ++q) if (f.obs_track[q] < 0 || f.obs_track[q] >= T) err = 1;
        for (int q = 0; q < f.n_pf; ++q) if (f.pf_track[q] < 0 || f.pf_track[q] >= T) err = 1;
        if (!plan) for (int q = 0; q < f.n_clones; ++q) if (f.clone_idx[q] < 0 || f.clone_idx[q] + 6 > n_max) err = 1;
        int* fw = ip + h[TRK_I_FEAT];
        for (int j = 0; j < f.n_feat; ++j) {
            if (f.feat_track[j] < 0 || f.feat_track[j] >= T || f.feat_anchor[j] < 0 || f.feat_anchor[j] >= f.n_clones || f.feat_dof[j] < 0 || f.feat_dof[j] > 255) err = 1;
            fw[j] = (int)((unsigned)f.feat_track[j] | ((unsigned)f.feat_anchor[j] << 16) | ((unsigned)f.feat_dof[j] << 24));
        }
        badp[i] = err;
        if (f.n_drop) memcpy(ip + h[TRK_I_DROP], f.drop_slots, 4 * (size_t)f.n_drop);
        if (f.n_free) memcpy(ip + h[TRK_I_FREE], f.free_tracks, 4 * (size_t)f.n_free);
        if (f.n_obs) { memcpy(ip + h[TRK_I_OBS], f.obs_track, 4 * (size_t)f.n_obs); memcpy(dp + h[TRK_D_OBS], f.obs_uv, 32 * (size_t)f.n_obs); }
        if (f.n_pf) { memcpy(ip + h[TRK_I_PF], f.pf_track, 4 * (size_t)f.n_pf); memcpy(dp + h[TRK_D_PF], f.pf, 24 * (size_t)f.n_pf); }
        if (f.n_clones && !plan) {
            memcpy(ip + h[TRK_I_CIDX], f.clone_idx, 4 * (size_t)f.n_clones);
            memcpy(dp + h[TRK_D_CR], f.clone_R, 72 * (size_t)f.n_clones); memcpy(dp + h[TRK_D_CP], f.clone_p, 24 * (size_t)f.n_clones);
        }
        for (int g = 0; g < 5; ++g) ip[h[TRK_I_GNSS] + g] = s.gnss_idx[g];
        if (f.feat_sel) memcpy(mpool + h[TRK_OFF_M], f.feat_sel, 8 * (size_t)f.n_feat);
        if (s.k) memcpy(dp + h[TRK_D_IMU], s.imu, 56 * (size_t)s.k);
        if (!plan) {
            double* st0 = dp + h[TRK_D_STATE];
            memcpy(st0, s.R, 72); memcpy(st0 + 9, s.p, 24); memcpy(st0 + 12, s.v, 24); memcpy(st0 + 15, s.bg, 24); memcpy(st0 + 18, s.ba, 24); memcpy(st0 + 21, s.gravity, 24);
        }
    });
    for (int i = 0; i < nb; ++i) if (bad[i]) { c->err = "ingvio_frame_stage_tracks: a slot, track, clone index, anchor or dof is out of range"; return INGVIO_E_ARG; }
    if (int rc = stage.commit(steps)) return rc;
    const hipStream_t S = async ? c->st_copy : c->st;
    char* dstage = c->trk.stage[async ? 1 : 0];
    upl.copy(dstage, slab, total);
    stage.upload_gate();
    if (!upd) stage.upload_imu(steps);
    TrackStage ts{ reinterpret_cast<const int*>(dstage), reinterpret_cast<const int*>(dstage + off_i),
                   reinterpret_cast<const double*>(dstage + off_d), reinterpret_cast<const unsigned long long*>(dstage + off_m) };
    const TrackStore store = track_store(c);
    FrameOut fo{ c->d_clone_idx, c->d_clone_R, c->d_clone_p, c->d_nclones, c->d_nfeat, c->d_pf, c->d_anchor, c->d_mask, c->d_uv, c->d_dof, cm, fm };
    const NomTable nt = nom_table(c);
    // from the device table on the copy stream: the uploads above overlap the running frame, the kernels wait for its post-frame step
    if (plan && async && c->nom.ev_valid && hipStreamWaitEvent(S, c->nom.ev, 0) != hipSuccess) return stage.fail(INGVIO_E_HIP);
    // a host-fed asynchronous stage too lands behind the erasures of an ingvio_tracks_maintain_begin enqueued before it (both write masks and flags)
    if (!plan && async && c->mt.ev_recorded && hipStreamWaitEvent(S, c->mt.ev, 0) != hipSuccess) return stage.fail(INGVIO_E_HIP);
    if (!upd) launch_imu_steps(ts, b0, nb, KMAX, c->d_Phi, c->d_G, c->d_dt, c->d_R, S, plan ? &nt : nullptr);
    if (hipGetLastError() != hipSuccess) return stage.fail(INGVIO_E_HIP);       // before the store kernels change the track store
    launch_tracks_apply(ts, store, b0, nb, S);
    if (tg) launch_tracks_gather_tri(ts, store, fo, b0, nb, c->d_idx, c->d_gnss, S, nt, tg->tri_mask, tg->tri_track);
    else launch_tracks_gather(ts, store, fo, b0, nb, c->d_idx, c->d_gnss, S, plan ? &nt : nullptr);
    if (hipGetLastError() != hipSuccess) return stage.fail(INGVIO_E_HIP);
    if (tg && tg->at_stage) {                    // in front of finish(): the run's wait for the inputs covers it
        c->nom.tri = *tg->at_stage; c->nom.tri_fmx = fmx;
        if (nom_triangulate(c, S, c->nom.d_tri_ok_st, c->nom.d_tri_pf_st) || hipGetLastError() != hipSuccess) return stage.fail(INGVIO_E_HIP);
    }
    return stage.finish(steps, frames, fmx, plan, upd);
}

int ingvio_frame_stage_tracks(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step_raw* steps, const ingvio_track_frame* frames,
                              const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw, int async)
{
    ENTER(c);
    return frame_stage_tracks_impl(c, b0, nb, steps, frames, opts, sigma, enable_gnss, scb, srw, async, nullptr);
}

int ingvio_frame_stage_tracks_nominal(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step_nominal* steps, const ingvio_track_frame* frames,
                                      const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw, int async)
{
    return ingvio_frame_stage_tracks_nominal_tri(c, b0, nb, steps, frames, opts, sigma, enable_gnss, scb, srw, nullptr, async);
}

// where the triangulation of ingvio_frame_stage_tracks_nominal_tri is issued (Nominal::tri_place); results are bit-identical
int ingvio_set_first_tri_placement(ingvio_ctx* c, int mode)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    if (mode < 0 || mode > 1) { c->err = "ingvio_set_first_tri_placement: mode is 0 or 1"; return INGVIO_E_ARG; }
    if (c->nom.pending) { c->err = "ingvio_set_first_tri_placement: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    c->nom.tri_place = mode;
    return INGVIO_OK;
}

// The first MSCKF update of a camera frame (RemoveLostUpdate::updateStateStereo / Mono) from the table: tri != NULL, its features' points
// come from the window's clones as they stand behind the IMU integration and the new clone (MapServerManager.cpp:275-341)
int ingvio_frame_stage_tracks_nominal_tri(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step_nominal* steps, const ingvio_track_frame* frames,
                                          const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw,
                                          const ingvio_tri_opts* tri, int async)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !steps || !frames) return INGVIO_E_ARG;
    auto& m = c->nom;
    if (!m.vmax) { c->err = "ingvio_frame_stage_tracks_nominal without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (tri && !c->trk.t_max) { c->err = "ingvio_frame_stage_tracks_nominal_tri without ingvio_tracks_create"; return INGVIO_E_ARG; }
    if (tri && (tri->outer_loop_max_iter < 0 || tri->inner_loop_max_iter < 0)) return INGVIO_E_ARG;
    // the post-frame step retracts, drops and shifts EVERY filter of the batch, and a second stage before the run is refused: the frame
    // staged from the table is the whole batch's
    if (b0 != 0 || nb != c->d.batch) { c->err = "ingvio_frame_stage_tracks_nominal stages the whole batch (b0 = 0, nb = batch)"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, "ingvio_frame_stage_tracks_nominal")) return INGVIO_E_ARG;
    if ((c->gn.staged && c->gn.in_frame) || (c->lm.staged && c->lm.in_frame)) {
        c->err = "the device nominal state does not take an in-frame GNSS or landmark stage";
        return INGVIO_E_UNSUPPORTED;
    }
    if (c->parts_req > 1) { c->err = "the device nominal state runs with frame_parts = 1 only"; return INGVIO_E_UNSUPPORTED; }
    // ---- the new clone's slot and idx and the marginalisation, on the host mirror (nothing changes before every filter passed) ----
    std::vector<int> plan((size_t)nb * 4);
    std::vector<ingvio_frame_step_raw> raw((size_t)nb);
    std::vector<ingvio_track_frame> fr(frames, frames + nb);
    for (int i = 0; i < nb; ++i) {
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        if (I[NOM_V_EXT] < 0 || I[NOM_V_POSE] < 0 || I[NOM_V_BG] < 0 || I[NOM_V_BA] < 0) {
            c->err = "ingvio_frame_stage_tracks_nominal: the table names no extrinsics, pose or bias variable"; return INGVIO_E_ARG;
        }
        const int ncl = I[NOM_N_CLONES] + 1;
        int slot = -1;
        for (int v = 0; v < m.vmax && slot < 0; ++v) if (var[4 * v] == NOM_KIND_NONE) slot = v;
        if (ncl > c->d.c_max || slot < 0 || c->h_n[b] + 6 > c->d.n_max) return INGVIO_E_CAPACITY;
        const int idx = c->h_n[b], mg = steps[i].marg_idx;
        if (mg >= 0) {
            int ms = mg == idx ? slot : -1;
            for (int q = 0; q < ncl - 1 && ms < 0; ++q) if (var[4 * I[NOM_CLONES + q] + 1] == mg) ms = I[NOM_CLONES + q];
            if (ms < 0) { c->err = "ingvio_frame_stage_tracks_nominal: marg_idx names no clone of the window"; return INGVIO_E_NOT_IN_STATE; }
            for (int v = 0; v < I[NOM_N_VAR]; ++v)
                if (var[4 * v] == NOM_KIND_LM && var[4 * v + 2] == ms) {
                    c->err = "ingvio_frame_stage_tracks_nominal: a landmark is anchored to the clone that leaves the window"; return INGVIO_E_ARG;
                }
        }
        plan[4 * i] = slot; plan[4 * i + 1] = idx; plan[4 * i + 2] = ncl; plan[4 * i + 3] = std::max(I[NOM_N_VAR], slot + 1);
        ingvio_frame_step_raw& r = raw[i];
        memset(&r, 0, sizeof r);
        r.k = steps[i].k; r.imu = steps[i].imu; r.marg_idx = mg;
        memcpy(r.gnss_idx, steps[i].gnss_idx, sizeof r.gnss_idx);
        fr[i].n_clones = ncl; fr[i].clone_idx = nullptr; fr[i].clone_R = nullptr; fr[i].clone_p = nullptr;
    }
    if (!tri) return frame_stage_tracks_impl(c, b0, nb, raw.data(), fr.data(), opts, sigma, enable_gnss, scb, srw, async, plan.data());
    const bool at_stage = m.tri_place == 1;
    if (int rc = tri_buffers(c, at_stage)) return rc;
    const TableStage ft{ false, c->d_tri_mask, m.d_tri_track, at_stage ? tri : nullptr };
    const int rc = frame_stage_tracks_impl(c, b0, nb, raw.data(), fr.data(), opts, sigma, enable_gnss, scb, srw, async, plan.data(), &ft);
    if (rc == INGVIO_OK) {
        m.tri_on = true; m.tri_staged = at_stage; m.tri = *tri; m.tri_fmx = 0;
        for (int i = 0; i < nb; ++i) m.tri_fmx = std::max(m.tri_fmx, frames[i].n_feat);
    }
    return rc;
}

// The second MSCKF update of a camera frame (SwMargUpdate / KeyframeUpdate::updateState*, IngvioFilter.cpp:271-324) as a frame from the
// table of its own: no IMU steps, no new clone, the window as the table holds it
int ingvio_update_stage_tracks_nominal(ingvio_ctx* c, int b0, int nb, const int* marg_idx, const ingvio_track_frame* frames, const ingvio_msckf_opts* opts,
                                       const ingvio_tri_opts* tri, int async)
{
    ENTER(c);
    if (phase_busy(c) || check_range(c, b0, nb) || !marg_idx || !frames || !opts) return INGVIO_E_ARG;
    auto& m = c->nom;
    const char* who = "ingvio_update_stage_tracks_nominal";
    if (!m.vmax) { c->err = std::string(who) + " without ingvio_nominal_create"; return INGVIO_E_ARG; }
    if (!c->trk.t_max) { c->err = std::string(who) + " without ingvio_tracks_create"; return INGVIO_E_ARG; }
    if (b0 != 0 || nb != c->d.batch) { c->err = std::string(who) + " stages the whole batch (b0 = 0, nb = batch)"; return INGVIO_E_ARG; }
    if (m.pending) { c->err = "a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    if (gnss_nom_busy(c, who)) return INGVIO_E_ARG;
    if ((c->gn.staged && c->gn.in_frame) || (c->lm.staged && c->lm.in_frame)) {
        c->err = "the device nominal state does not take an in-frame GNSS or landmark stage";
        return INGVIO_E_UNSUPPORTED;
    }
    if (c->parts_req > 1) { c->err = "the device nominal state runs with frame_parts = 1 only"; return INGVIO_E_UNSUPPORTED; }
    if (tri && (tri->outer_loop_max_iter < 0 || tri->inner_loop_max_iter < 0)) return INGVIO_E_ARG;
    std::vector<int> plan((size_t)nb * 4);
    std::vector<ingvio_frame_step_raw> raw((size_t)nb);
    std::vector<ingvio_track_frame> fr(frames, frames + nb);
    for (int i = 0; i < nb; ++i) {
        const int b = b0 + i;
        const int* I = &m.h_ih[(size_t)b * m.ir];
        const int* var = I + NOM_IH;
        if (frames[i].append_slot >= 0 || frames[i].n_obs > 0) { c->err = std::string(who) + ": an update-only frame appends no observations"; return INGVIO_E_ARG; }
        const int ncl = I[NOM_N_CLONES], mg = marg_idx[i];
        int hi = -1, ms = -1;
        for (int q = 0; q < ncl; ++q) {
            const int idx = var[4 * I[NOM_CLONES + q] + 1];
            if (idx > hi) hi = idx;
            if (mg >= 0 && ms < 0 && idx == mg) ms = I[NOM_CLONES + q];
        }
        if (mg >= 0) {
            if (ms < 0) { c->err = std::string(who) + ": marg_idx names no clone of the window"; return INGVIO_E_NOT_IN_STATE; }
            for (int v = 0; v < I[NOM_N_VAR]; ++v)
                if (var[4 * v] == NOM_KIND_LM && var[4 * v + 2] == ms) {
                    c->err = std::string(who) + ": a landmark is anchored to the clone that leaves the window"; return INGVIO_E_ARG;
                }
        }
        plan[4 * i] = -1; plan[4 * i + 1] = hi; plan[4 * i + 2] = ncl; plan[4 * i + 3] = I[NOM_N_VAR];
        ingvio_frame_step_raw& r = raw[i];
        memset(&r, 0, sizeof r);
        r.marg_idx = mg < 0 ? -1 : mg;
        for (int g = 0; g < 5; ++g) r.gnss_idx[g] = c->st_gnss[(size_t)b * 5 + g];      // no propagation: the clock indices stay what they are
        fr[i].n_clones = ncl; fr[i].clone_idx = nullptr; fr[i].clone_R = nullptr; fr[i].clone_p = nullptr;
    }
    TableStage upd{ true, nullptr, nullptr, nullptr };
    if (tri) {
        if (int rc = tri_buffers(c, false)) return rc;
        upd.tri_mask = c->d_tri_mask; upd.tri_track = m.d_tri_track;
    }
    static const double no_sigma[4] = { 0.0, 0.0, 0.0, 0.0 };
    const int rc = frame_stage_tracks_impl(c, b0, nb, raw.data(), fr.data(), opts, no_sigma, c->staged ? c->st_enable_gnss : 0, 0.0, 0.0, async, plan.data(), &upd);
    if (rc == INGVIO_OK && tri) {
        m.tri_on = true; m.tri = *tri; m.tri_fmx = 0;
        for (int i = 0; i < nb; ++i) m.tri_fmx = std::max(m.tri_fmx, frames[i].n_feat);
    }
    return rc;
}

int ingvio_frame_stage(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step* steps, const ingvio_msckf_frame* frames,
                       const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw)
{
    ENTER(c);
    return frame_stage_impl(c, b0, nb, steps, frames, opts, sigma, enable_gnss, scb, srw, false);
}

int ingvio_frame_stage_async(ingvio_ctx* c, int b0, int nb, const ingvio_frame_step* steps, const ingvio_msckf_frame* frames,
                             const ingvio_msckf_opts* opts, const double sigma[4], int enable_gnss, double scb, double srw)
{
    ENTER(c);
    return frame_stage_impl(c, b0, nb, steps, frames, opts, sigma, enable_gnss, scb, srw, true);
}

int ingvio_frame_set_imu_noise(ingvio_ctx* c, int b0, int nb, const double* noise)
{
    ENTER(c);
    if (!c || phase_busy(c)) return INGVIO_E_ARG;
    if (!c->staged) { c->err = "ingvio_frame_set_imu_noise without a staged frame"; return INGVIO_E_ARG; }
    if (check_range(c, b0, nb) || !noise) return INGVIO_E_ARG;
    for (size_t i = 0; i < (size_t)nb * 6; ++i)
        if (!std::isfinite(noise[i])) { c->err = "ingvio_frame_set_imu_noise: a value is not finite"; return INGVIO_E_ARG; }
    // after ingvio_frame_stage_async the values belong to the input set still on its way: on the copy stream, behind that stage's
    // copies (the frame running on the compute stream reads the other set); otherwise on the compute stream, behind the frames
    // already enqueued there
    Uploader upl{ c };
    if (c->copy_pending) upl.stream = c->st_copy;
    if (int rc = upl.begin(pad64(64 * (size_t)nb) + 64)) return rc;
    double* blk = upl.take<double>(8 * (size_t)nb);
    for (int i = 0; i < nb; ++i) {
        double* h = &c->st_prm[(size_t)(b0 + i) * 8];
        memcpy(blk + (size_t)i * 8, noise + (size_t)i * 6, 48);
        blk[(size_t)i * 8 + 6] = h[6]; blk[(size_t)i * 8 + 7] = 0.0;
    }
    upl.copy(c->d_prm + (size_t)b0 * 8, blk, 8 * (size_t)nb);
    if (int rc = upl.end()) return rc;
    if (c->copy_pending) HIPCHK(c, hipEventRecord(c->ev_copy, c->st_copy));
    memcpy(&c->st_prm[(size_t)b0 * 8], blk, 64 * (size_t)nb);
    return INGVIO_OK;
}

// ---- running the staged frame: the pieces ingvio_frame_run / ingvio_frame_run_phase are made of ---------------------------------
static bool lm_in_frame(const ingvio_ctx* c) { return c->lm.staged && c->lm.in_frame; }
static bool gnss_in_frame(const ingvio_ctx* c) { return c->gn.staged && c->gn.in_frame && c->gn.m_cap > 0; }
// An in-frame GNSS stage rides on the MSCKF write-back when everything fits one sweep and the update's columns keep their indices
// through the frame's marginalisation (var_order entirely below the clone that goes); else it is a pass of its own
static bool gnss_folds(const ingvio_ctx* c)
{
    if (!gnss_in_frame(c) || c->d.c_max > 16 || c->gn.m_cap > 16 || c->gn.nc_max > 16) return false;
    for (int b = 0; b < c->d.batch; ++b) if (c->st_marg[b] < 0 || c->gn.hi[b] > c->st_marg[b]) return false;
    return true;
}

// restore_prior right after a fused frame step that itself began with a restore: half 0 still equals the snapshot outside the
// propagation's strips.  Asked before the step's first launch (view() counts the uses of the covariance).
static bool strips_valid(const ingvio_ctx* c, int restore_prior) { return restore_prior && c->strip_ok && c->mut_seq == c->strip_seq; }

// Restore (or not), then one launch: status reset + K1 (k composed IMU steps) + K2 (clone) when a workgroup owns a whole filter.  With
// valid strips the propagation READS the snapshot and writes half 0 where it can: no restore pass at all (round 6; before:
// k_restore_strips, 23 us and 94 MB per 512 filters)
static void launch_restore_propagate(ingvio_ctx* c, int restore_prior, bool strips, int b0, int nb, hipStream_t st)
{
    const bool from_snap = strips && propagate_can_restore(c->d.n_max) && !no_snap_propagate();
    if (restore_prior && !from_snap) {
        ProfScope p(c, PF_RESTORE);
        if (strips) launch_restore_strips(view(c), b0, nb, c->d.n_max, c->Psnap, c->d_n_snap, c->st_enable_gnss ? c->d_gnss : nullptr, st);
        else launch_restore(view(c), b0, nb, c->d.n_max, c->Psnap, c->d_n_snap, st);
    }
    ProfScope p(c, PF_PROPAGATE);
    const ImuLaunch im = imu_launch(c, b0, nb);
    launch_propagate(view(c), b0, nb, c->d.n_max, c->d_Phi + (size_t)b0 * KMAX * 225, c->d_G + (size_t)b0 * KMAX * 180, c->d_dt + (size_t)b0 * KMAX,
                     im.k, KMAX, im.prm, c->st_enable_gnss ? c->d_gnss + (size_t)b0 * 5 : nullptr, im.sigma, c->st_enable_gnss, im.scb, im.srw, st,
                     c->d_R + (size_t)b0 * 9, c->d_status, from_snap ? c->Psnap : nullptr, c->d_n_snap);
}

// the host mirrors of launch_restore_propagate over the whole batch and of the frame's marginalisation (true: of every filter)
static void mirror_restore_clone(ingvio_ctx* c, int restore_prior)
{
    if (restore_prior) { c->h_n = c->h_n_snap; std::fill(c->h_cur.begin(), c->h_cur.end(), 0); }
    for (int b = 0; b < c->d.batch; ++b) c->h_n[b] += 6;
}
static bool mirror_marg(ingvio_ctx* c)
{
    bool all = true;
    for (int b = 0; b < c->d.batch; ++b) { if (c->st_marg[b] >= 0) { c->h_n[b] -= 6; c->h_cur[b] ^= 1; } else all = false; }
    return all;
}

// An in-frame landmark or GNSS stage belongs to ONE frame: the step that applied it consumes it, so that a later frame cannot apply the
// old rows to a state that has moved on - unless the caller replays the same prior (the bench, the parity tests)
static void consume_in_frame(bool& staged, bool in_frame, bool replay) { if (staged && in_frame && !replay) staged = false; }
// the strip shortcut of the NEXT restore: valid after a step from the prior that wrote every filter's posterior into the other half
static void strips_after_step(ingvio_ctx* c, bool valid) { c->strip_ok = valid; c->strip_seq = c->mut_seq; }

// The fused frame step of windows up to 16 clones with the batch dealt to P slices.  Slice p = filters [p B / P, (p + 1) B / P) rounded
// to multiples of 8 (the kernels' XCD-aware block order works on groups of 8 filters), on stream part[p].st:
//     restore -> propagate + clone -> [wait: gate of slice p - 1] gate [record] -> Gram -> solve -> (GNSS in-frame) -> apply + marginalise
// Same kernels, same arguments per filter as the unsplit step: results are bit-identical (tests/test_gpu_parity.py runs both).
static int frame_run_split(ingvio_ctx* c, int restore_prior, int P, bool gnss_fuse)
{
    const int B = c->d.batch;
    if (parts_prepare(c, P)) return INGVIO_E_HIP;
    if (c->split_pending && c->copy_pending) ENTER(c);                     // fresh inputs on the copy stream: order them through c->st
    if (wait_inputs(c)) return INGVIO_E_HIP;
    if (!c->split_pending) {                                                // work on c->st since the last split step: the slices start behind it
        HIPCHK(c, hipEventRecord(c->ev_split_fork, c->st));
        for (int p = 0; p < P; ++p) HIPCHK(c, hipStreamWaitEvent(c->part[p].st, c->ev_split_fork, 0));
        c->tok_last = nullptr;
    }
    const bool strips = strips_valid(c, restore_prior);
    mirror_restore_clone(c, restore_prior);
    int rc = 0;
    auto range = [&](int p, int& b0, int& nb) {
        b0 = (int)((long long)B * p / P) & ~7;
        const int b1 = p + 1 == P ? B : ((int)((long long)B * (p + 1) / P) & ~7);
        nb = b1 - b0;
    };
    // Issue order = order of the throughput segments on the device: gate + Gram of every slice, then the apply of every slice; a
    // segment waits for the one issued before it (whatever stream that was on) - the slices' latency-bound kernels (restore, propagate,
    // solve, the flips) run freely in between, under the other slices' segments
    for (int p = 0; p < P && !rc; ++p) {
        int b0, nb; range(p, b0, nb);
        if (nb <= 0) continue;
        auto& q = c->part[p];
        c->run_st = q.st;
        launch_restore_propagate(c, restore_prior, strips, b0, nb, q.st);
        c->tok_wait = c->tok_last; c->tok_rec = q.ev_gate;
        rc = run_msckf_factored(c, b0, nb, c->st_op, c->st_stereo, c->st_fmax_used, c->d_idx + b0, 6, 1, gnss_fuse);
        c->tok_last = rc ? nullptr : q.ev_gate;
    }
    for (int p = 0; p < P && !rc; ++p) {
        int b0, nb; range(p, b0, nb);
        if (nb <= 0) continue;
        auto& q = c->part[p];
        c->run_st = q.st;
        c->tok_wait = c->tok_last; c->tok_rec = q.ev_apply;
        rc = run_msckf_factored(c, b0, nb, c->st_op, c->st_stereo, c->st_fmax_used, c->d_idx + b0, 6, 2, gnss_fuse);
        c->tok_last = rc ? nullptr : q.ev_apply;
        if (!rc && !c->apply_flipped) {
            ProfScope pr(c, PF_MARG);
            launch_post_marg(view(c), b0, nb, c->d_idx + b0, 6, q.st);
        }
    }
    for (int p = 0; p < P; ++p) hipEventRecord(c->part[p].ev_done, c->part[p].st);
    c->tok_wait = nullptr; c->tok_rec = nullptr;
    c->run_st = c->st;
    c->split_pending = true;
    if (rc) { c->tok_last = nullptr; ENTER(c); return rc; }
    const bool all_marg = mirror_marg(c);
    strips_after_step(c, all_marg && restore_prior);
    consume_in_frame(c->gn.staged, c->gn.in_frame, restore_prior != 0);
    return INGVIO_OK;                              // (the slices' input set is handed back by join_parts)
}

// front half of the split (feature-sharded) step: restore, propagate + clone, gate + Gram; the [A | b] partials stay on the device
static int frame_run_front(ingvio_ctx* c, int restore_prior)
{
    const int B = c->d.batch;
    ENTER(c);
    if (wait_inputs(c)) return INGVIO_E_HIP;
    launch_restore_propagate(c, restore_prior, strips_valid(c, restore_prior), 0, B, c->st);
    mirror_restore_clone(c, restore_prior);
    strips_after_step(c, false);
    const int rc = run_msckf_factored(c, 0, B, c->st_op, c->st_stereo, c->st_fmax_used, nullptr, 0, 1);
    // h_n is already + 6 (the clone exists on the device): only phase 2 may follow - and only after a front half that was
    // launched; after a refused one the step has to be abandoned with ingvio_cov_restore or replayed with
    // ingvio_frame_run(restore_prior)
    if (rc == 0) { c->phase_pending = true; c->phase_restore = restore_prior != 0; }
    return rc;
}

// back half: solve + apply + marginalise from the partials (a replay: the front half began with restore_prior)
static int frame_run_back(ingvio_ctx* c)
{
    c->phase_pending = false;
    const int B = c->d.batch;
    const bool with_lm = lm_in_frame(c), replay = c->phase_restore;
    int rc = run_msckf_factored(c, 0, B, c->st_op, c->st_stereo, c->st_fmax_used, with_lm ? nullptr : c->d_idx, with_lm ? 0 : 6, 2);
    if (rc) return rc;
    if (with_lm) { rc = landmark_update_launch(c, 0, B); if (rc) return rc; }
    {
        ProfScope p(c, PF_MARG);
        if (!with_lm) { if (!c->apply_flipped) launch_post_marg(view(c), 0, B, c->d_idx, 6, c->st); }
        else launch_marginalize(view(c), 0, B, c->d.n_max, c->d_idx, 6, c->st);
    }
    mirror_marg(c);
    consume_in_frame(c->lm.staged, c->lm.in_frame, replay);
    strips_after_step(c, false);
    // an in-frame GNSS stage: the split step never folds it into the write-back - its own pass, as the unsplit step does for the
    // shapes it cannot fold (it used to be dropped silently here)
    if (gnss_in_frame(c)) {
        rc = gnss_run_separate(c, 0, B, true);
        if (rc) return rc;
        consume_in_frame(c->gn.staged, c->gn.in_frame, replay);
    }
    return release_input_set(c);
}

// the whole step, unsplit, on the compute stream
static int frame_run_whole(ingvio_ctx* c, int restore_prior)
{
    const int B = c->d.batch;
    ENTER(c);
    if (wait_inputs(c)) return INGVIO_E_HIP;
    c->nom.tri_ran = false;
    if (c->nom.frame && c->nom.noprop) {
        // the update-only frame from the table: nothing is propagated and no clone joins, so the status reset that rides on the
        // propagation launch is issued here; then (tri_on) the listed features' points from every stored observation, with the settings
        // of ingvio_msckf_update_tri - a feature that fails loses its mask and drops out of the gate - and the points that succeeded
        // into the track store (setValuePosXyz, MapServerManager.cpp:335).  No host synchronisation.
        HIPCHK(c, hipMemsetAsync(c->d_status, 0, sizeof(int) * (size_t)B, c->st));
        if (c->nom.tri_on) {
            if (int rc = nom_triangulate(c, c->st, (int*)(c->d_result_slab + c->ro_tok), (double*)(c->d_result_slab + c->ro_tpf))) return rc;
            c->nom.tri_ran = true;
        }
    } else {
        launch_restore_propagate(c, restore_prior, strips_valid(c, restore_prior), 0, B, c->st);
        mirror_restore_clone(c, restore_prior);
        // the ordinary frame from the table that triangulates (ingvio_frame_stage_tracks_nominal_tri): the same two launches in front of the
        // gate, or - issued at the stage already (Nominal::tri_place) - only the flags and points on their way into the result slab
        if (c->nom.frame && c->nom.tri_on) {
            if (c->nom.tri_staged) {
                const size_t cnt = (size_t)B * c->d.f_max;
                HIPCHK(c, hipMemcpyAsync(c->d_result_slab + c->ro_tok, c->nom.d_tri_ok_st, sizeof(int) * cnt, hipMemcpyDeviceToDevice, c->st));
                HIPCHK(c, hipMemcpyAsync(c->d_result_slab + c->ro_tpf, c->nom.d_tri_pf_st, 8 * cnt * 3, hipMemcpyDeviceToDevice, c->st));
            } else if (int rc = nom_triangulate(c, c->st, (int*)(c->d_result_slab + c->ro_tok), (double*)(c->d_result_slab + c->ro_tpf))) return rc;
            c->nom.tri_ran = true;
        }
    }
    // factored path: the marginalisation of the oldest clone rides on the update's write-back (k_info_apply
    // stores the updated covariance compacted into the other ping-pong half); dense path: separate kernel
    // staged in-frame landmark update (IngvioFilter.cpp:296-322: MSCKF updates, landmark update, then the marginalisation):
    // the marginalisation cannot ride on the MSCKF write-back then
    const bool with_lm = lm_in_frame(c);
    const bool fuse = c->method == 1 && !with_lm;
    // with a landmark update to follow, the MSCKF update is still written OUT OF PLACE (a "marginalisation" of zero columns into the
    // other half, then the halves flip): the solve then reads P[:, clone columns] straight from the untouched prior instead of
    // copying them first (0.035 ms per 512 filters), and the landmark downdate writes back into the first half with the real
    // marginalisation fused
    const bool lm_oop = with_lm && c->method == 1;
    // in-frame GNSS stage (ingvio_gnss_opts::in_frame): on the MSCKF write-back when everything fits one sweep, else as its own pass below
    const bool gnss_here = gnss_in_frame(c), gnss_fuse = fuse && gnss_folds(c);
    // the raw epoch of a frame staged from the table (ingvio_gnss_frame_stage_nominal): its own result slots and status words, cleared here
    // (dx = 0 beyond the live n, for a filter without epoch and where no satellite was staged at all) - as the two-call form's run does
    const bool gnss_nomf = c->gn.staged && c->gn.frame_nom;
    if (gnss_nomf) {
        auto& g = c->gn;
        HIPCHK(c, hipMemsetAsync(g.dxf, 0, 8 * (size_t)B * c->ldp, c->st));
        HIPCHK(c, hipMemsetAsync(g.stf, 0, sizeof(int) * (size_t)B, c->st));
        HIPCHK(c, hipMemsetAsync(g.mf, 0, sizeof(int) * (size_t)B, c->st));
        g.own_status = true; g.results = true; g.fused_last = true; g.folded_last = false;
    }
    int rc = fuse     ? run_msckf_factored(c, 0, B, c->st_op, c->st_stereo, c->st_fmax_used, c->d_idx, 6, 0, gnss_fuse, true)
             : lm_oop ? run_msckf_factored(c, 0, B, c->st_op, c->st_stereo, c->st_fmax_used, c->d_zero_idx, 0, 0, false, true)
                      : run_msckf(c, 0, B, c->st_op, c->st_stereo, c->st_fmax_used);      // (method 0: the dense path)
    if (rc) return rc;
    if (lm_oop) {
        if (!c->apply_flipped) launch_post_marg(view(c), 0, B, c->d_zero_idx, 0, c->st);
        for (int b = 0; b < B; ++b) c->h_cur[b] ^= 1;
    }
    // landmarks staged from the device nominal state: boxPlus of the MSCKF dx on the table (no drop, no shift) and, in the same launch,
    // the landmark inputs from the values just retracted - the rows are formed at the state after the MSCKF update (IngvioFilter.cpp:283-289)
    const bool lm_nom = with_lm && c->lm.nominal;
    if (lm_nom) landmark_gather_launch(c, c->d_dx, 0, B);
    bool lm_fused = false;
    if (with_lm) { rc = landmark_update_launch(c, 0, B, c->d_idx, 6, &lm_fused); if (rc) return rc; }
    if (!(fuse && c->apply_flipped)) {             // (the write-back of the fused step has flipped the halves itself: no launch, no profile slot)
        ProfScope p(c, PF_MARG);
        if (fuse || lm_fused) launch_post_marg(view(c), 0, B, c->d_idx, 6, c->st);
        else launch_marginalize(view(c), 0, B, c->d.n_max, c->d_idx, 6, c->st);
    }
    consume_in_frame(c->lm.staged, c->lm.in_frame, restore_prior != 0);
    const bool all_marg = mirror_marg(c);
    if (c->nom.pending) {                          // device nominal state: boxPlus with the frame's dx, drop + shift, behind the marginalisation
        // (with landmarks from the table the frame's dx is on the table already: the LANDMARK update's dx, in the same index space)
        // (with the GNSS epoch folded into the write-back the MSCKF dx is on the table too, and the GNSS dx is given in the index space
        // behind the marginalisation: retraction through the shift, drop and shift in one launch)
        if (gnss_nomf && gnss_fuse) launch_nominal_update_post(nom_table(c), c->gn.dxf, c->ldp, c->d_idx, 0, B, c->st);
        else launch_nominal_update(nom_table(c), lm_nom ? c->lm.dx : c->d_dx, c->ldp, c->d_idx, 0, B, c->st);
        if (int rc2 = last_launch(c)) return rc2;
        for (int b = 0; b < B; ++b) nom_mirror_marg(c, b, c->st_marg[b]);
        c->nom.pending = false;
        if (nom_mark(c)) return INGVIO_E_HIP;
    }
    strips_after_step(c, fuse && all_marg && restore_prior);
    if (gnss_here && !gnss_fuse) {                 // not foldable (large window, landmarks in the frame, many rows): its own pass, now
        if (gnss_nomf) {
            // from the table: ingvio_gnss_front_stage_nominal + ingvio_gnss_run behind the frame, launch for launch - the front on the
            // table the frame has just left (idx behind the shift), the pass with its own slots, boxPlus of its dx
            for (int b = 0; b < B; ++b) { int& hi = c->gn.hi[b]; if (c->st_marg[b] >= 0 && hi > c->st_marg[b]) hi -= 6; }
            gnss_front_launch(c, 0, B, true, c->st);
        }
        rc = gnss_run_separate(c, 0, B, true);
        if (rc) return rc;
        if (gnss_nomf) {
            launch_nominal_update(nom_table(c), c->gn.dxf, c->ldp, nullptr, 0, B, c->st);
            if (int rc2 = last_launch(c)) return rc2;
            if (nom_mark(c)) return INGVIO_E_HIP;
        }
    }
    consume_in_frame(c->gn.staged, c->gn.in_frame, restore_prior != 0);
    if (!c->gn.staged) c->gn.frame_nom = false;
    return release_input_set(c);
}

// refusals -> checks against the live state -> one of {split, front half, back half, whole step}
static int frame_run_impl(ingvio_ctx* c, int restore_prior, int phase)
{
    if (!c || !c->staged) return INGVIO_E_ARG;
    if (c->nom.frame) {                                                     // a frame staged from the device nominal state
        if (!c->nom.pending) { c->err = "the frame staged from the device nominal state has already run"; return INGVIO_E_ARG; }
        if (phase) { c->err = "the split step does not take a frame staged from the device nominal state"; return INGVIO_E_UNSUPPORTED; }
        if (restore_prior) { c->err = "restore_prior with a frame staged from the device nominal state (restore with ingvio_cov_restore before the stage)"; return INGVIO_E_ARG; }
        // (the one in-frame stage it takes is the landmark stage from the table itself, ingvio_landmark_stage_nominal)
        if ((c->gn.staged && c->gn.in_frame && !c->gn.frame_nom) || (lm_in_frame(c) && !c->lm.nominal) || c->parts_req > 1) {
            c->err = "the device nominal state takes no in-frame GNSS / host-fed landmark stage and frame_parts = 1 only"; return INGVIO_E_UNSUPPORTED;
        }
    } else if (lm_in_frame(c) && c->lm.nominal) {
        c->err = "an in-frame landmark stage from the device nominal state needs a frame staged from it"; return INGVIO_E_ARG;
    } else if (c->gn.staged && c->gn.frame_nom) {
        c->err = "a GNSS epoch staged for a frame from the device nominal state needs that frame"; return INGVIO_E_ARG;
    }
    if (phase && c->method != 1) return INGVIO_E_UNSUPPORTED;             // the split needs the information form's [A | b]
    // protocol of the split step: 1 -> (ingvio_debug_msckf_info / ingvio_info_set) -> 2, exactly once each; the accepted-feature
    // cap is a global order over the features and is not defined across shards
    if (phase != 2 && phase_busy(c)) return INGVIO_E_ARG;
    if (phase == 2 && !c->phase_pending) { c->err = "ingvio_frame_run_phase(.., 2) without a preceding phase 1"; return INGVIO_E_ARG; }
    if (phase != 0 && c->st_op.max_accept > 0) { c->err = "max_accept is not supported by the split (feature-sharded) frame step"; return INGVIO_E_ARG; }
    if (phase == 2) return frame_run_back(c);
    const int B = c->d.batch;
    // ---- every check that can refuse the step comes before the first launch and before any host-side state changes ----
    if (restore_prior && !c->has_snap) return INGVIO_E_ARG;
    if (c->method == 0 && c->d.c_max > 16) return INGVIO_E_UNSUPPORTED;       // the dense MSCKF method stops at 16 clones
    {
        const std::vector<int>& n0 = restore_prior ? c->h_n_snap : c->h_n;
        const int grow = c->nom.frame && c->nom.noprop ? 0 : 6;             // (an update-only frame from the table takes no new clone)
        for (int b = 0; b < B; ++b) {
            if (n0[b] < 21) return INGVIO_E_ARG;
            if (n0[b] + grow > c->d.n_max) return INGVIO_E_CAPACITY;
            if (c->st_cidx_hi[b] + 6 > n0[b] + grow) return INGVIO_E_NOT_IN_STATE;      // a staged clone lies beyond the live state
            if (c->st_marg[b] >= 0 && c->st_marg[b] + 6 > n0[b] + grow) return INGVIO_E_NOT_IN_STATE;
        }
        if (lm_in_frame(c)) { if (int rc = landmark_in_state(c, 0, B, n0, grow)) return rc; }
    }
    if (phase == 1) return frame_run_front(c, restore_prior);
    // ---- split step (round 6): the batch as `parts` slices on their own streams, gates chained, nothing joined at the end ----
    // automatic = off: measured on MI355X at 512 filters x (150 features, 11 clones, N = 249) the split LOSES - 0.535 ms unsplit, 0.58
    // (gates chained) / 0.65 (throughput segments chained) with two slices, 0.73-0.97 with three and four
    const int P = std::min(c->parts_req > 0 ? c->parts_req : 1, 4);
    const bool gnss_fuse = gnss_folds(c);
    if (P > 1 && c->method == 1 && !lm_in_frame(c) && c->d.c_max <= 16 && (!gnss_in_frame(c) || gnss_fuse) && B >= 16 * P)
        return frame_run_split(c, restore_prior, P, gnss_fuse);
    return frame_run_whole(c, restore_prior);
}

int ingvio_frame_run(ingvio_ctx* c, int restore_prior) { return frame_run_impl(c, restore_prior, 0); }
int ingvio_set_frame_parts(ingvio_ctx* c, int parts)
{
    if (!c || parts < -1 || parts > 4) return INGVIO_E_ARG;
    ENTER(c);
    c->parts_req = parts == 0 ? 1 : parts;
    return INGVIO_OK;
}
// the fused frame step's Gram kernel in its reduced form, on by default; off: the full form everywhere, for comparison
int ingvio_set_gram_reduced(ingvio_ctx* c, int on)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    c->gram_reduced = on ? 1 : 0;
    return INGVIO_OK;
}
// the reduced form as k_feat_gram3 (wave pairs decoupled, one barrier per batch; window classes 6 and 11), on by default; off: k_feat_gram2
int ingvio_set_gram_decoupled(ingvio_ctx* c, int on)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    c->gram_decoupled = on ? 1 : 0;
    return INGVIO_OK;
}
// the form the last MSCKF update's Gram stage took: 0 full, 1 reduced k_feat_gram2, 2 reduced k_feat_gram3
int ingvio_last_gram_form(ingvio_ctx* c)
{
    if (!c) return INGVIO_E_ARG;
    return c->gram_form_last;
}
// the fused frame step's write-back with Pc resident in LDS (k_info_apply_res; full batches of the window classes 6 and 11,
// ldp <= 256, no in-frame GNSS fold); off: k_info_apply
int ingvio_set_apply_resident(ingvio_ctx* c, int on)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    c->apply_resident = on ? 1 : 0;
    return INGVIO_OK;
}
// the form the last MSCKF update's write-back took: 0 k_info_apply (or a few-filter / large-window kernel), 1 k_info_apply_res
int ingvio_last_apply_form(ingvio_ctx* c)
{
    if (!c) return INGVIO_E_ARG;
    return c->apply_form_last;
}
// route and variants of the last generic update (INGVIO_UPDATE_*); 0 before the first one
int ingvio_last_update_form(ingvio_ctx* c)
{
    if (!c) return INGVIO_E_ARG;
    return c->update_form_last;
}
// which form of the delayed-initialisation front the three entry points take (kernels_delayed.hip)
int ingvio_set_delayed_form(ingvio_ctx* c, int mode)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    if (mode < 0 || mode > 2) { c->err = "ingvio_set_delayed_form: mode is 0, 1 or 2"; return INGVIO_E_ARG; }
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (c->nom.pending) { c->err = "ingvio_set_delayed_form: a frame staged from the device nominal state has not run yet"; return INGVIO_E_ARG; }
    c->delayed_form = mode;
    return INGVIO_OK;
}
// A GNSS stage of any form whose update has not run.  Which flags each stage leaves:
//   ingvio_gnss_stage, ingvio_gnss_front_stage   staged = true, results = false; their run sets results and KEEPS staged (the pristine
//                                                rows may run again); an in-frame ingvio_gnss_stage is consumed by its frame's run
//   ingvio_gnss_front_stage_nominal              the same plus nom_pending, which its one run clears
//   ingvio_gnss_frame_stage_nominal              staged and frame_nom, results untouched (they are the frame before's); the frame's run
//                                                clears staged and frame_nom
static bool gnss_stage_waiting(const ingvio_ctx* c)
{
    const auto& g = c->gn;
    return g.staged && (g.frame_nom || g.nom_pending || !g.results);
}

// GnssUpdate::_is_adjust_yof: carried to the kernels in the receiver record (GR_ADJ_YOF), so it is fixed when an epoch is staged
int ingvio_set_gnss_adjust_yof(ingvio_ctx* c, int on)
{
    if (!c) return INGVIO_E_ARG;
    ENTER(c);
    if (phase_busy(c)) return INGVIO_E_ARG;
    if (gnss_stage_waiting(c)) {
        c->err = "ingvio_set_gnss_adjust_yof: a GNSS epoch is staged and has not run yet"; return INGVIO_E_ARG;
    }
    c->gnss_adjust_yof = on ? 1 : 0;
    return INGVIO_OK;
}
int ingvio_frame_run_phase(ingvio_ctx* c, int restore_prior, int phase)
{
    if (phase < 0 || phase > 2) return INGVIO_E_ARG;
    return frame_run_impl(c, restore_prior, phase);
}

// the stacked information [A | b] = [sum_j H_j^T H_j | sum_j H_j^T r_j] of filter b replaces the chunk partials (feature-sharded
// single filter: every rank sums the ranks' partials and continues with ingvio_frame_run_phase(.., 2))
int ingvio_info_set(ingvio_ctx* c, int b, const double* A, int ncol, int n_accepted)
{
    ENTER(c);
    if (check_range(c, b, 1) || !A || ncol < 6 || (size_t)ncol * (ncol + 1) > (size_t)c->rstride || n_accepted < 0) return INGVIO_E_ARG;
    std::vector<int> used(c->G, 0);
    used[0] = n_accepted;
    int rc = up(c, c->d_Rpart + (size_t)b * c->G * c->rstride, A, 8 * (size_t)ncol * (ncol + 1));
    rc |= up(c, c->d_chunk_used + (size_t)b * c->G, used.data(), sizeof(int) * (size_t)c->G);
    if (rc) return INGVIO_E_HIP;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return INGVIO_OK;
}

// ---- device-resident exchange of the feature-sharded filter (the ONE exchange step per frame) ---------------------
// ingvio_info_reduce sums filter b's chunk partials into one contiguous device buffer [A | b | n_accepted] (ncol (ncol + 1) + 1
// doubles; the accepted count rides along as a double so that ONE all-reduce carries everything) and hands out the DEVICE
// pointer: the caller all-reduces it in place (RCCL on the pointer itself, or torch.distributed on a zero-copy view,
// ingvio_amd/parallel.py) - nothing crosses PCIe.  ingvio_info_commit makes the reduced buffer the filter's information
// (chunk 0 = the sum, its count = the summed n_accepted) for ingvio_frame_run_phase(.., 2).
namespace {
__global__ __launch_bounds__(256) void k_info_reduce(const double* __restrict__ Apart, const int* __restrict__ chunk_used, int G, int rstride,
                                                     int cnt, double* __restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e > cnt) return;
    double s = 0.0;
    if (e < cnt) { for (int g = 0; g < G; ++g) if (chunk_used[g]) s += Apart[(size_t)g * rstride + e]; }
    else { for (int g = 0; g < G; ++g) s += (double)chunk_used[g]; }
    out[e] = s;
}
__global__ __launch_bounds__(256) void k_info_commit(const double* __restrict__ in, int cnt, double* __restrict__ Apart0, int* __restrict__ chunk_used, int G)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < cnt) Apart0[e] = in[e];
    if (e < G) chunk_used[e] = e == 0 ? (int)llrint(in[cnt]) : 0;
}
}  // namespace

int ingvio_info_reduce(ingvio_ctx* c, int b, double** dev_ptr, int* count, int* ncol_out)
{
    ENTER(c);
    if (check_range(c, b, 1) || !dev_ptr || !count || c->method != 1) return INGVIO_E_ARG;
    int C = 0;
    if (down_sync(c, &C, c->d_nclones + b, sizeof(int))) return INGVIO_E_HIP;
    const int ncol = 6 * C, cnt = ncol * (ncol + 1);
    if (cnt <= 0 || cnt > c->rstride) return INGVIO_E_ARG;
    if (!c->d_xchg && dalloc(c, &c->d_xchg, (size_t)c->d.batch * (c->rstride + 8))) return INGVIO_E_HIP;
    double* out = c->d_xchg + (size_t)b * (c->rstride + 8);
    hipLaunchKernelGGL(k_info_reduce, dim3((cnt + 256) / 256), dim3(256), 0, c->st, c->d_Rpart + (size_t)b * c->G * c->rstride,
                       c->d_chunk_used + (size_t)b * c->G, c->G, c->rstride, cnt, out);
    HIPCHK(c, hipStreamSynchronize(c->st));              // the caller's collective runs on ITS stream: the buffer must be complete
    *dev_ptr = out; *count = cnt + 1;
    if (ncol_out) *ncol_out = ncol;
    return last_launch(c);
}

int ingvio_info_commit(ingvio_ctx* c, int b)
{
    ENTER(c);
    if (check_range(c, b, 1) || !c->d_xchg || c->method != 1) return INGVIO_E_ARG;
    int C = 0;
    if (down_sync(c, &C, c->d_nclones + b, sizeof(int))) return INGVIO_E_HIP;
    const int ncol = 6 * C, cnt = ncol * (ncol + 1);
    if (cnt <= 0 || cnt > c->rstride) return INGVIO_E_ARG;
    hipLaunchKernelGGL(k_info_commit, dim3((std::max(cnt, c->G) + 255) / 256), dim3(256), 0, c->st, c->d_xchg + (size_t)b * (c->rstride + 8), cnt,
                       c->d_Rpart + (size_t)b * c->G * c->rstride, c->d_chunk_used + (size_t)b * c->G, c->G);
    return last_launch(c);
}

// The frame's results travel through the pinned mirror of the result slab (h_result): a device-to-host copy into pageable caller memory
// is staged by the runtime in small synchronous pieces (1.3 MB of dx + flags for 512 filters: 0.2 ms during which the device idles).
// _begin only ENQUEUES the copies behind the frame's kernels and records an event; _end waits for it and hands the data out - between
// the two the host may stage and launch the next frame (the copies sit in front of its kernels in the stream, so the slab is read
// before it is rewritten).
int ingvio_frame_fetch_begin(ingvio_ctx* c, int b0, int nb)
{
    ENTER(c);
    if (check_range(c, b0, nb)) return INGVIO_E_ARG;
    const int fm = c->d.f_max;
    if (!c->ev_fetch) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fetch, hipEventDisableTiming));
    HIPCHK(c, hipMemcpyAsync(c->h_result + 8 * (size_t)b0 * c->ldp, c->d_dx + (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->h_result + c->ro_used + sizeof(int) * (size_t)b0 * fm, c->d_used + (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->h_result + c->ro_m + sizeof(int) * (size_t)b0, c->d_m + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->st));
    // a run that triangulated (a frame from the table staged with tri, ordinary or update-only): its flags and points travel with the
    // frame's results
    c->nom.tri_fetched = false;
    if (c->nom.tri_ran) {
        HIPCHK(c, hipMemcpyAsync(c->h_result + c->ro_tok + sizeof(int) * (size_t)b0 * fm, c->d_result_slab + c->ro_tok + sizeof(int) * (size_t)b0 * fm,
                                 sizeof(int) * (size_t)nb * fm, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(c->h_result + c->ro_tpf + 8 * (size_t)b0 * fm * 3, c->d_result_slab + c->ro_tpf + 8 * (size_t)b0 * fm * 3,
                                 8 * (size_t)nb * fm * 3, hipMemcpyDeviceToHost, c->st));
        c->nom.tri_fetched = true; c->nom.tri_b0 = b0; c->nom.tri_nb = nb;
    }
    HIPCHK(c, hipEventRecord(c->ev_fetch, c->st));
    c->fetch_b0 = b0; c->fetch_nb = nb;
    return last_launch(c);
}

// the flags and points of the run that triangulated: those the last ingvio_frame_fetch(_begin) of that run brought along (they stay
// valid until the next fetch, whatever ran in between), else straight from the device
int ingvio_frame_fetch_tri(ingvio_ctx* c, int b0, int nb, double* pf_out, int* tri_ok)
{
    if (!c || check_range(c, b0, nb)) return INGVIO_E_ARG;
    const int fm = c->d.f_max;
    if (c->nom.tri_fetched && b0 >= c->nom.tri_b0 && b0 + nb <= c->nom.tri_b0 + c->nom.tri_nb) {
        HIPCHK(c, hipEventSynchronize(c->ev_fetch));
        if (tri_ok) memcpy(tri_ok, c->h_result + c->ro_tok + sizeof(int) * (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm);
        if (pf_out) memcpy(pf_out, c->h_result + c->ro_tpf + 8 * (size_t)b0 * fm * 3, 8 * (size_t)nb * fm * 3);
        return INGVIO_OK;
    }
    if (!c->nom.tri_ran) { c->err = "ingvio_frame_fetch_tri: the frame that ran last did not triangulate (neither stage from the table was given tri)"; return INGVIO_E_ARG; }
    ENTER(c);
    if (tri_ok && down_sync(c, tri_ok, c->d_result_slab + c->ro_tok + sizeof(int) * (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm)) return INGVIO_E_HIP;
    if (pf_out && down_sync(c, pf_out, c->d_result_slab + c->ro_tpf + 8 * (size_t)b0 * fm * 3, 8 * (size_t)nb * fm * 3)) return INGVIO_E_HIP;
    return INGVIO_OK;
}

int ingvio_frame_fetch_end(ingvio_ctx* c, double* dx_out, int* accepted, int* rows_out)
{
    if (!c || c->fetch_nb <= 0) return INGVIO_E_ARG;                       // (no ENTER: the results are already on their way)
    const int fm = c->d.f_max, b0 = c->fetch_b0, nb = c->fetch_nb;
    HIPCHK(c, hipEventSynchronize(c->ev_fetch));
    c->fetch_nb = 0;
    if (dx_out) memcpy(dx_out, c->h_result + 8 * (size_t)b0 * c->ldp, 8 * (size_t)nb * c->ldp);
    if (accepted) memcpy(accepted, c->h_result + c->ro_used + sizeof(int) * (size_t)b0 * fm, sizeof(int) * (size_t)nb * fm);
    if (rows_out) memcpy(rows_out, c->h_result + c->ro_m + sizeof(int) * (size_t)b0, sizeof(int) * (size_t)nb);
    return INGVIO_OK;
}

int ingvio_frame_fetch(ingvio_ctx* c, int b0, int nb, double* dx_out, int* accepted, int* rows_out)
{
    int rc = ingvio_frame_fetch_begin(c, b0, nb);
    if (rc) return rc;
    rc = ingvio_frame_fetch_end(c, dx_out, accepted, rows_out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));                              // as before: the call leaves the stream drained
    return last_launch(c);
}

int ingvio_set_msckf_method(ingvio_ctx* c, int method)
{
    ENTER(c);
    if (!c || method < 0 || method > 1) return INGVIO_E_ARG;
    c->method = method;
    return INGVIO_OK;
}

// parity hook: [A | b] = [sum_j H_j^T H_j | sum_j H_j^T r_j] of the last MSCKF update of filter b, ncol x (ncol + 1) row-major
int ingvio_debug_msckf_info(ingvio_ctx* c, int b, double* A_out, int* ncol_out)
{
    ENTER(c);
    if (check_range(c, b, 1) || !A_out || !ncol_out) return INGVIO_E_ARG;
    if (c->method == 1 && c->gram_red_last) {      // the reference clone's block row / column of the partials was not written
        c->err = "the last frame step formed [A | b] in reduced form; run it with ingvio_set_gram_reduced(ctx, 0) to read the full [A | b]";
        return INGVIO_E_UNSUPPORTED;
    }
    int C = 0;
    if (down_sync(c, &C, c->d_nclones + b, sizeof(int))) return INGVIO_E_HIP;
    const int ncol = 6 * C;
    *ncol_out = ncol;
    const size_t w = (size_t)ncol + 1;
    for (size_t e = 0; e < (size_t)ncol * w; ++e) A_out[e] = 0.0;
    if (c->method == 1) {
        std::vector<int> used(c->G);
        if (down_sync(c, used.data(), c->d_chunk_used + (size_t)b * c->G, sizeof(int) * (size_t)c->G)) return INGVIO_E_HIP;
        std::vector<double> part((size_t)ncol * w);
        for (int g = 0; g < c->G; ++g) {
            if (!used[g]) continue;
            if (down_sync(c, part.data(), c->d_Rpart + ((size_t)b * c->G + g) * c->rstride, 8 * part.size())) return INGVIO_E_HIP;
            for (size_t e = 0; e < part.size(); ++e) A_out[e] += part[e];
        }
        return INGVIO_OK;
    }
    // dense method: the merged factor R (upper triangular, column-major ld = mld) and Q^T r in d_H / d_res
    int m = 0;
    if (down_sync(c, &m, c->d_m + b, sizeof(int))) return INGVIO_E_HIP;
    if (m == 0) return INGVIO_OK;
    std::vector<double> R((size_t)c->mld * ncol), z(c->mld);
    if (down_sync(c, R.data(), c->d_H + (size_t)b * c->hstride, 8 * R.size()) || down_sync(c, z.data(), c->d_res + (size_t)b * c->mld, 8 * (size_t)ncol))
        return INGVIO_E_HIP;
    for (int i = 0; i < ncol; ++i) {
        for (int j = 0; j < ncol; ++j) {
            double a = 0.0;
            for (int k = 0; k <= (i < j ? i : j); ++k) a += R[k + (size_t)i * c->mld] * R[k + (size_t)j * c->mld];
            A_out[i * w + j] = a;
        }
        double bb = 0.0;
        for (int k = 0; k <= i; ++k) bb += R[k + (size_t)i * c->mld] * z[k];
        A_out[i * w + ncol] = bb;
    }
    return INGVIO_OK;
}

// parity hook: [M | t] handed from the information solve to the apply kernel (MP x MP row-major, then MP entries), filter b
int ingvio_debug_info_solution(ingvio_ctx* c, int b, double* out, int count)
{
    ENTER(c);
    if (check_range(c, b, 1) || !out || count < 1 || count > c->ystride) return INGVIO_E_ARG;
    if (down_sync(c, out, c->d_Y + (size_t)b * c->ystride, 8 * (size_t)count)) return INGVIO_E_HIP;
    return INGVIO_OK;
}

// both streams idle, then plain blocking copies: the hooks below read what the compute stream AND the copy stream (asynchronous
// stages) have written, and leave every flag and event of the context as it was
static int debug_quiesce(ingvio_ctx* c)
{
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->st_copy) HIPCHK(c, hipStreamSynchronize(c->st_copy));
    return 0;
}
static int debug_down(ingvio_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (dst && bytes) HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// parity hook: filter b's slice of the track store
int ingvio_debug_tracks_read(ingvio_ctx* c, int b, unsigned long long* mask, double* uv, double* pf)
{
    ENTER(c);
    if (check_range(c, b, 1)) return INGVIO_E_ARG;
    if (!c->trk.t_max) { c->err = "ingvio_debug_tracks_read without ingvio_tracks_create"; return INGVIO_E_ARG; }
    if (debug_quiesce(c)) return INGVIO_E_HIP;
    const size_t T = c->trk.t_max, C = c->d.c_max;
    if (debug_down(c, mask, c->trk.mask + (size_t)b * T, 8 * T) || debug_down(c, uv, c->trk.uv + (size_t)b * T * C * 4, 8 * T * C * 4) ||
        debug_down(c, pf, c->trk.pf + (size_t)b * T * 3, 8 * T * 3)) return INGVIO_E_HIP;
    return INGVIO_OK;
}

// parity hook: filter b's point flags of the track store
int ingvio_debug_tracks_flags(ingvio_ctx* c, int b, unsigned char* has_point)
{
    ENTER(c);
    if (check_range(c, b, 1)) return INGVIO_E_ARG;
    if (!c->trk.t_max) { c->err = "ingvio_debug_tracks_flags without ingvio_tracks_create"; return INGVIO_E_ARG; }
    if (debug_quiesce(c)) return INGVIO_E_HIP;
    const size_t T = c->trk.t_max;
    if (debug_down(c, has_point, c->trk.has + (size_t)b * T, T)) return INGVIO_E_HIP;
    return INGVIO_OK;
}

// parity hook: filter b's arrays of the input set the next ingvio_frame_run reads (the d_* pointers: after an asynchronous stage the
// set it staged into)
int ingvio_debug_staged_frame(ingvio_ctx* c, int b, int* n_clones, int* n_feat, int* clone_idx, double* clone_R, double* clone_p, int* anchor, int* dof,
                              unsigned long long* obs_mask, double* pf, double* uv)
{
    ENTER(c);
    if (check_range(c, b, 1)) return INGVIO_E_ARG;
    if (debug_quiesce(c)) return INGVIO_E_HIP;
    const size_t cm = c->d.c_max, fm = c->d.f_max, B = b;
    if (debug_down(c, n_clones, c->d_nclones + B, 4) || debug_down(c, n_feat, c->d_nfeat + B, 4) ||
        debug_down(c, clone_idx, c->d_clone_idx + B * cm, 4 * cm) || debug_down(c, clone_R, c->d_clone_R + B * cm * 9, 8 * cm * 9) ||
        debug_down(c, clone_p, c->d_clone_p + B * cm * 3, 8 * cm * 3) || debug_down(c, anchor, c->d_anchor + B * fm, 4 * fm) ||
        debug_down(c, dof, c->d_dof + B * fm, 4 * fm) || debug_down(c, obs_mask, c->d_mask + B * fm, 8 * fm) ||
        debug_down(c, pf, c->d_pf + B * fm * 3, 8 * fm * 3) || debug_down(c, uv, c->d_uv + B * fm * cm * 4, 8 * fm * cm * 4)) return INGVIO_E_HIP;
    return INGVIO_OK;
}

int ingvio_debug_read(ingvio_ctx* c, long long* out, int n)
{
    ENTER(c);
    if (!c || !out || n < 1 || n > 64) return INGVIO_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->st));
    long long a[64], bq[64], cq[64], sq[64];
    if (dbg_read_factored(a, 64) || dbg_read_cov(bq, 64) || dbg_read_bigwin(cq, 64) || dbg_read_solve(sq, 64)) return INGVIO_E_HIP;
    long long hq[64];
    if (dbg_read_chol(hq, 64)) return INGVIO_E_HIP;
    long long lq[64], mq[64];
    if (dbg_read_lmbatch(lq, 64) || dbg_read_lmchol(mq, 64)) return INGVIO_E_HIP;
    if (const char* e = getenv("INGVIO_DBG_TU")) {                     // debugging: all slots of one translation unit
        const long long* src = e[0] == 'b' ? cq : (e[0] == 'c' ? hq : (e[0] == 's' ? sq : (e[0] == 'l' ? lq : (e[0] == 'm' ? mq : a))));
        for (int i = 0; i < n; ++i) out[i] = src[i];
        return INGVIO_OK;
    }
    for (int i = 0; i < n; ++i)      // 16..23 cov, 24..31 the symmetric solve (its slots 0..7), 48..55 large-window TU, 56..63 kernels_chol (0..7)
        out[i] = i >= 56 ? hq[i - 56] : (i >= 48 ? cq[i] : ((i >= 24 && i < 32) ? sq[i - 24] : ((i < 16 || i >= 32) ? a[i] : bq[i])));
    return INGVIO_OK;
}

int ingvio_profile_select(ingvio_ctx* c, const char* kernel_name)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    c->prof_only = -1;
    if (!kernel_name || !*kernel_name) return INGVIO_OK;
    for (int i = 0; i < PF_COUNT; ++i) if (!strcmp(kernel_name, kProfNames[i])) { c->prof_only = i; return INGVIO_OK; }
    return INGVIO_E_ARG;
}

int ingvio_profile_enable(ingvio_ctx* c, int enable)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    c->prof = enable != 0;
    return INGVIO_OK;
}

static void prof_collect(ingvio_ctx* c)
{
    hipStreamSynchronize(c->st);
    for (auto& r : c->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->prof_ms[r.id] += ms; c->prof_calls[r.id] += 1; }
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    c->recs.clear();
}

int ingvio_profile_reset(ingvio_ctx* c)
{
    ENTER(c);
    if (!c) return INGVIO_E_ARG;
    prof_collect(c);
    memset(c->prof_ms, 0, sizeof c->prof_ms); memset(c->prof_calls, 0, sizeof c->prof_calls);
    return INGVIO_OK;
}

int ingvio_profile_get(ingvio_ctx* c, const char** names, double* ms, int* calls, int cap)
{
    ENTER(c);
    if (!c || !names || !ms || !calls) return INGVIO_E_ARG;
    prof_collect(c);
    int k = 0;
    for (int i = 0; i < PF_COUNT && k < cap; ++i) { names[k] = kProfNames[i]; ms[k] = c->prof_ms[i]; calls[k] = c->prof_calls[i]; ++k; }
    return k;
}

}  // extern "C"
