"""ctypes binding of the C ABI (include/ingvio_hip.h) — thin plumbing, no arithmetic.

There is no CPU fallback: importing works anywhere (so the symbol table can be checked without a
GPU), but creating a context raises if libingvio_hip.so is missing or no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("INGVIO_HIP_LIB") or os.path.join(_HERE, "lib", "libingvio_hip.so")     # override: build experiments only

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
c_up = C.POINTER(C.c_ulonglong)

OK, NO_ROWS, NEG_DIAG, REJECTED = 0, 1, 2, 3
E_ARG, E_CAPACITY, E_HIP, E_NOT_IN_STATE, E_UNSUPPORTED, E_NOT_PD = -1, -2, -3, -4, -5, -6
R_SCALAR, R_DIAG, R_FULL = 0, 1, 2
# ingvio_last_update_form (INGVIO_UPDATE_* of ingvio_hip.h)
UPDATE_LDS, UPDATE_DENSE_REG, UPDATE_DENSE_SWEEP = 1, 2, 3
UPDATE_GEMM64_PHT, UPDATE_GEMM64_S, UPDATE_SPLIT_SWEEP = 0x200, 0x400, 0x800


def update_form(route, ntm=0, gemm64=False, split=False):
    """the value ingvio_last_update_form reports for a route, the tile class of the register-resident solve, both products on
    k_gemm64 and the split sweep"""
    return route | (ntm << 4) | ((UPDATE_GEMM64_PHT | UPDATE_GEMM64_S) if gemm64 else 0) | (UPDATE_SPLIT_SWEEP if split else 0)


EXPORTS = [
    "ingvio_ctx_create", "ingvio_ctx_destroy", "ingvio_sync", "ingvio_ctx_stream", "ingvio_f_max", "ingvio_c_max", "ingvio_last_error", "ingvio_ldp",
    "ingvio_build_id",
    "ingvio_cov_set", "ingvio_cov_get", "ingvio_get_n", "ingvio_cov_get_marginal", "ingvio_cov_snapshot",
    "ingvio_cov_restore", "ingvio_propagate", "ingvio_propagate_fused", "ingvio_augment_clone", "ingvio_marginalize",
    "ingvio_append_independent", "ingvio_ekf_update", "ingvio_chi2_gamma", "ingvio_msckf_update", "ingvio_msckf_update_tri", "ingvio_qr_compress",
    "ingvio_frame_stage", "ingvio_frame_stage_async", "ingvio_frame_set_imu_noise", "ingvio_frame_fetch_begin", "ingvio_frame_fetch_end", "ingvio_tracks_create", "ingvio_frame_stage_tracks", "ingvio_frame_run", "ingvio_set_frame_parts", "ingvio_set_gram_reduced", "ingvio_set_gram_decoupled", "ingvio_last_gram_form", "ingvio_set_apply_resident", "ingvio_last_apply_form", "ingvio_last_update_form", "ingvio_frame_fetch", "ingvio_profile_enable", "ingvio_profile_select",
    "ingvio_profile_reset",
    "ingvio_profile_get", "ingvio_set_msckf_method", "ingvio_set_qr_method", "ingvio_landmark_stage", "ingvio_landmark_run",
    "ingvio_landmark_fetch", "ingvio_frame_run_phase", "ingvio_info_set", "ingvio_debug_read", "ingvio_triangulate",
    "ingvio_gnss_front_stage", "ingvio_gnss_front_fetch", "ingvio_gnss_update_batch", "ingvio_gnss_stage", "ingvio_gnss_run", "ingvio_gnss_fetch", "ingvio_mld", "ingvio_debug_msckf_info", "ingvio_debug_info_solution",
    "ingvio_info_reduce", "ingvio_info_commit", "ingvio_gnss_sat_eval", "ingvio_debug_gnss_staged_rows",
    "ingvio_chi2_gamma_multi", "ingvio_ekf_update_batch", "ingvio_add_variable_delayed_invertible", "ingvio_add_variable_delayed", "ingvio_add_variable_delayed_batch", "ingvio_replace_var_linear",
    "ingvio_nominal_create", "ingvio_nominal_set", "ingvio_nominal_get", "ingvio_nominal_box_plus", "ingvio_frame_stage_tracks_nominal",
    "ingvio_nominal_set_gnss", "ingvio_nominal_get_gnss", "ingvio_gnss_front_stage_nominal", "ingvio_landmark_stage_nominal",
    "ingvio_landmark_init_nominal", "ingvio_debug_landmark_init_rows", "ingvio_nominal_tail",
    "ingvio_debug_tracks_read", "ingvio_debug_staged_frame",
    "ingvio_gnss_frame_stage_nominal", "ingvio_debug_gnss_fused_last", "ingvio_debug_nominal_update_post",
    "ingvio_update_stage_tracks_nominal", "ingvio_frame_fetch_tri", "ingvio_set_delayed_form",
    "ingvio_odom_begin", "ingvio_odom_end", "ingvio_cov_get_marginal_batch",
    "ingvio_frame_stage_tracks_nominal_tri", "ingvio_set_first_tri_placement",
    "ingvio_gnss_init_nominal", "ingvio_debug_gnss_init_rows",
    "ingvio_tracks_maintain_begin", "ingvio_tracks_maintain_end", "ingvio_tracks_maintain", "ingvio_debug_tracks_flags",
    "ingvio_set_gnss_adjust_yof", "ingvio_nominal_add_gnss", "ingvio_nominal_marg_gnss",
]

# device-resident nominal state (ingvio_nominal_*): variable kinds, doubles per value
NOM_NONE, NOM_SE23, NOM_SE3, NOM_VEC3, NOM_SCALAR, NOM_LANDMARK = -1, 0, 1, 2, 3, 4
NOM_VAL = 15
# odometry record (ingvio_odom_begin / _end): the bits of `what` and of a record's status; the batch getter's column capacity
ODOM_COV, ODOM_EUCL, ODOM_DIAG = 1, 2, 4
ODOM_ALL = ODOM_COV | ODOM_EUCL | ODOM_DIAG
ODOM_NONFINITE, ODOM_NEG_DIAG, ODOM_ABSENT = 1, 2, 4
MARGINAL_NS_MAX = 64
# verdicts of ingvio_tracks_maintain (INGVIO_MAINTAIN_* of ingvio_hip.h)
MAINTAIN_KEEP, MAINTAIN_MOVED, MAINTAIN_ERASED_UNTRIANGULATED, MAINTAIN_ERASED_MOVE, MAINTAIN_ERASED_INVALID = 0, 1, 2, 3, 4


class GateBlock(C.Structure):
    _fields_ = [("vidx", C.POINTER(C.c_int)), ("vsize", C.POINTER(C.c_int)), ("k", C.c_int), ("H", C.POINTER(C.c_double)),
                ("ldh", C.c_int), ("m", C.c_int), ("res", C.POINTER(C.c_double))]


class UpdateBlock(C.Structure):
    _fields_ = [("vidx", C.POINTER(C.c_int)), ("vsize", C.POINTER(C.c_int)), ("k", C.c_int), ("H", C.POINTER(C.c_double)),
                ("ldh", C.c_int), ("m", C.c_int), ("res", C.POINTER(C.c_double)), ("R", C.POINTER(C.c_double))]


class DelayedCand(C.Structure):
    _fields_ = [("vidx", C.POINTER(C.c_int)), ("vsize", C.POINTER(C.c_int)), ("k", C.c_int), ("H_old", C.POINTER(C.c_double)),
                ("ldh", C.c_int), ("H_new", C.POINTER(C.c_double)), ("ldn", C.c_int), ("res", C.POINTER(C.c_double)),
                ("m", C.c_int), ("s", C.c_int), ("chi2_check", C.c_double)]


class DelayedBlock(C.Structure):
    _fields_ = [("n_cand", C.c_int), ("cand", C.POINTER(DelayedCand))]


def make_delayed_blocks(blocks):
    """blocks: per filter a list of candidates (vidx, vsize, H_old [m, nc], H_new [m, s], res [m][, chi2_check]); chi2_check defaults to
    quantile(chi2(m), 0.95) (scipy).  Returns (ingvio_delayed_block array, cand_cap, objects that own the memory the array points to)."""
    nb = len(blocks)
    arr = (DelayedBlock * max(nb, 1))(); keep = []
    cand_cap = max([len(cs) for cs in blocks] + [1])
    for g, cands in enumerate(blocks):
        arr[g].n_cand = len(cands)
        if not cands:
            continue
        ca = (DelayedCand * len(cands))()
        for j, cd in enumerate(cands):
            vidx, vsize, H_old, H_new, res = cd[:5]
            H_old = np.asfortranarray(np.atleast_2d(H_old), dtype=np.float64)
            H_new = np.asfortranarray(np.atleast_2d(H_new), dtype=np.float64)
            m, s = H_new.shape
            if len(cd) > 5 and cd[5] is not None:
                chk = float(cd[5])
            else:
                from scipy.stats import chi2 as _chi2
                chk = float(_chi2.ppf(0.95, m)) if m > 0 else 0.0
            vi, vs, r = i32(vidx), i32(vsize), f64(res)
            keep.append((H_old, H_new, vi, vs, r))
            ca[j].vidx = _i(vi); ca[j].vsize = _i(vs); ca[j].k = len(vi); ca[j].H_old = _d(H_old); ca[j].ldh = max(m, 1)
            ca[j].H_new = _d(H_new); ca[j].ldn = max(m, 1); ca[j].res = _d(r); ca[j].m = m; ca[j].s = s; ca[j].chi2_check = chk
        keep.append(ca)
        arr[g].cand = ca
    return arr, cand_cap, keep


class LmInitCand(C.Structure):
    _fields_ = [("track", C.c_int), ("anchor", C.c_int), ("pf", C.c_double * 3)]


class LmInitBlock(C.Structure):
    _fields_ = [("n_cand", C.c_int), ("cand", C.POINTER(LmInitCand)), ("n_drop", C.c_int), ("drop_cols", C.POINTER(C.c_int))]


def make_lm_init_blocks(blocks):
    """blocks: per filter a dict(cands=[(track, anchor window position, pf [3]), ...], drop=[pending drop columns of the store]).
    Returns (ingvio_lm_init_block array, cand_cap, objects that own the memory the array points to)."""
    nb = len(blocks)
    arr = (LmInitBlock * max(nb, 1))(); keep = []
    cand_cap = max([len(bk["cands"]) for bk in blocks] + [1])
    for g, bk in enumerate(blocks):
        cands, drop = bk["cands"], i32(bk.get("drop", []))
        arr[g].n_cand = len(cands); arr[g].n_drop = len(drop)
        if len(drop):
            arr[g].drop_cols = _i(drop); keep.append(drop)
        if not cands:
            continue
        ca = (LmInitCand * len(cands))()
        for j, (track, anchor, pf) in enumerate(cands):
            ca[j].track = int(track); ca[j].anchor = int(anchor); ca[j].pf = (C.c_double * 3)(*f64(pf).reshape(3))
        keep.append(ca)
        arr[g].cand = ca
    return arr, cand_cap, keep


class NominalTailBlock(C.Structure):
    _fields_ = [("n_reanchor", C.c_int), ("lm_slot", C.POINTER(C.c_int)), ("new_anchor", C.c_int), ("n_erase", C.c_int),
                ("erase_slot", C.POINTER(C.c_int)), ("n_marg", C.c_int), ("marg_slot", C.POINTER(C.c_int))]


class MaintainBlock(C.Structure):
    _fields_ = [("n_tracks", C.c_int), ("tracks", C.POINTER(C.c_int)), ("n_lm", C.c_int), ("lm_slot", C.POINTER(C.c_int))]


class MaintainOpts(C.Structure):
    _fields_ = [("move_min_depth", C.c_double), ("min_depth", C.c_double), ("list_cap", C.c_int), ("lm_cap", C.c_int)]


def maintain_word(track, anchor_pos, move):
    """one entry of a maintenance list: track | anchor_pos << 16 | move << 24"""
    return int(track) | (int(anchor_pos) << 16) | (int(move) << 24)


class GnssOpts(C.Structure):
    _fields_ = [("gate_rows", C.c_int), ("strong_reject", C.c_int), ("chi2_table", C.POINTER(C.c_double)), ("chi2_len", C.c_int),
                ("in_frame", C.c_int)]


class GnssEpoch(C.Structure):
    _fields_ = [("n_sat", C.c_int), ("eph", C.POINTER(C.c_double)), ("obs", C.POINTER(C.c_double)), ("ion", C.POINTER(C.c_double)),
                ("doy", C.c_double), ("p_w", C.c_double * 3), ("v_w", C.c_double * 3), ("cb", C.c_double * 4), ("fs", C.c_double),
                ("yaw_offset", C.c_double), ("R_enu2ecef", C.c_double * 9), ("anchor_ecef", C.c_double * 3), ("idx_se23", C.c_int),
                ("idx_yof", C.c_int), ("idx_fs", C.c_int), ("idx_cb", C.c_int * 4), ("psr_noise_amp", C.c_double),
                ("dopp_noise_amp", C.c_double)]


class GnssEpochNominal(C.Structure):
    _fields_ = [("n_sat", C.c_int), ("eph", C.POINTER(C.c_double)), ("obs", C.POINTER(C.c_double)), ("ion", C.POINTER(C.c_double)),
                ("doy", C.c_double), ("R_enu2ecef", C.c_double * 9), ("anchor_ecef", C.c_double * 3), ("psr_noise_amp", C.c_double),
                ("dopp_noise_amp", C.c_double)]


GNSS_INIT_CAND = 5       # ingvio_gnss_init_nominal: candidate 0 = FS, 1..4 = clock bias GPS, GLO, GAL, BDS


class GnssInitBlock(C.Structure):
    _fields_ = [("epoch", GnssEpochNominal), ("pos_spp", C.c_double * 7), ("vel_spp", C.c_double * 4)]


def make_gnss_init_blocks(blocks):
    """blocks: per filter None (nothing for this filter) or a dict(epoch=dict as for gnss_front_stage_nominal or None, pos_spp [7],
    vel_spp [4]).  Returns (ingvio_gnss_init_block array, objects that own the memory the array points to)."""
    arr = (GnssInitBlock * max(len(blocks), 1))(); keep = []
    for i, bk in enumerate(blocks):
        a = arr[i]
        a.epoch.n_sat = 0
        if bk is None:
            continue
        if bk.get("epoch") is not None:
            keep.append(_epoch_host_fields(a.epoch, bk["epoch"]))
        a.pos_spp = (C.c_double * 7)(*f64(bk["pos_spp"]).reshape(7)); a.vel_spp = (C.c_double * 4)(*f64(bk["vel_spp"]).reshape(4))
    return arr, keep


class LandmarkFrame(C.Structure):
    _fields_ = [("R_i2w", C.c_double * 9), ("p_i2w", C.c_double * 3), ("R_cl2i", C.c_double * 9), ("p_c2i", C.c_double * 3),
                ("idx_epose", C.c_int), ("idx_ext", C.c_int), ("n_lm", C.c_int), ("lm_idx", C.POINTER(C.c_int)),
                ("anchor_idx", C.POINTER(C.c_int)), ("pf", C.POINTER(C.c_double)), ("uv", C.POINTER(C.c_double)),
                ("tracked", C.POINTER(C.c_ubyte))]


class LandmarkFrameNominal(C.Structure):
    _fields_ = [("n_lm", C.c_int), ("lm_var", C.POINTER(C.c_int)), ("uv", C.POINTER(C.c_double)), ("tracked", C.POINTER(C.c_ubyte))]


class LandmarkOpts(C.Structure):
    _fields_ = [("stereo", C.c_int), ("noise", C.c_double), ("chi2_thr", C.c_double), ("R_cl2cr", C.c_double * 9),
                ("t_cl2cr", C.c_double * 3), ("in_frame", C.c_int)]


LM_MAX = 64


class CtxDesc(C.Structure):
    _fields_ = [("batch", C.c_int), ("n_max", C.c_int), ("c_max", C.c_int), ("f_max", C.c_int), ("m_max", C.c_int),
                ("device", C.c_int), ("stream", C.c_void_p)]


class MsckfFrame(C.Structure):
    _fields_ = [("n_clones", C.c_int), ("clone_idx", c_ip), ("clone_R", c_dp), ("clone_p", c_dp), ("n_feat", C.c_int),
                ("pf", c_dp), ("anchor", c_ip), ("obs_mask", c_up), ("uv", c_dp), ("dof", c_ip)]


class MsckfOpts(C.Structure):
    _fields_ = [("stereo", C.c_int), ("R_cl2cr", C.c_double * 9), ("t_cl2cr", C.c_double * 3), ("noise", C.c_double),
                ("chi2_table", c_dp), ("chi2_len", C.c_int), ("max_accept", C.c_int), ("compress_rule", C.c_int),
                ("selected_variant", C.c_int)]


class FrameStep(C.Structure):
    _fields_ = [("k", C.c_int), ("Phi", c_dp), ("G", c_dp), ("dt", c_dp), ("gnss_idx", C.c_int * 5),
                ("R_i2w", C.c_double * 9), ("marg_idx", C.c_int)]


class TrackFrame(C.Structure):
    _fields_ = [("n_drop", C.c_int), ("drop_slots", c_ip), ("n_free", C.c_int), ("free_tracks", c_ip), ("append_slot", C.c_int),
                ("n_obs", C.c_int), ("obs_track", c_ip), ("obs_uv", c_dp), ("n_pf", C.c_int), ("pf_track", c_ip), ("pf", c_dp),
                ("n_clones", C.c_int), ("clone_idx", c_ip), ("clone_R", c_dp), ("clone_p", c_dp),
                ("n_feat", C.c_int), ("feat_track", c_ip), ("feat_anchor", c_ip), ("feat_dof", c_ip), ("feat_sel", c_up)]


class FrameStepRaw(C.Structure):
    _fields_ = [("k", C.c_int), ("imu", c_dp), ("R", C.c_double * 9), ("p", C.c_double * 3), ("v", C.c_double * 3), ("bg", C.c_double * 3),
                ("ba", C.c_double * 3), ("gravity", C.c_double * 3), ("gnss_idx", C.c_int * 5), ("marg_idx", C.c_int)]


class Nominal(C.Structure):
    _fields_ = [("n_var", C.c_int), ("kind", c_ip), ("idx", c_ip), ("anchor", c_ip), ("val", c_dp), ("n_clones", C.c_int), ("clone_var", c_ip),
                ("v_ext", C.c_int), ("v_pose", C.c_int), ("v_bg", C.c_int), ("v_ba", C.c_int), ("gravity", C.c_double * 3)]


class Odom(C.Structure):
    _fields_ = [("n", C.c_int), ("status", C.c_int), ("gnss_mask", C.c_int), ("reserved", C.c_int),
                ("R_i2w", C.c_double * 9), ("p", C.c_double * 3), ("v", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3),
                ("R_c2i", C.c_double * 9), ("p_c2i", C.c_double * 3), ("gnss", C.c_double * 6), ("diag_min", C.c_double), ("diag_max", C.c_double),
                ("cov_err", C.c_double * 225), ("cov_pose", C.c_double * 36), ("cov_vel", C.c_double * 9)]


ODOM_DTYPE = np.dtype(Odom)


def odom_dicts(rec):
    """records (a numpy array of ODOM_DTYPE) as the dicts odom_end() and odom.odom_model() share: matrices as [row, column]"""
    def colmajor(x, m):
        return x.reshape(-1, m, m).transpose(0, 2, 1)
    mats = dict(R_i2w=rec["R_i2w"].reshape(-1, 3, 3), R_c2i=rec["R_c2i"].reshape(-1, 3, 3), cov_err=colmajor(rec["cov_err"], 15),
                cov_pose=colmajor(rec["cov_pose"], 6), cov_vel=colmajor(rec["cov_vel"], 3))
    out = []
    for i in range(len(rec)):
        d = dict(n=int(rec["n"][i]), status=int(rec["status"][i]), gnss_mask=int(rec["gnss_mask"][i]), diag_min=float(rec["diag_min"][i]),
                 diag_max=float(rec["diag_max"][i]))
        for k in ("p", "v", "bg", "ba", "p_c2i", "gnss"):
            d[k] = rec[k][i].copy()
        for k, m in mats.items():
            d[k] = m[i].copy()
        out.append(d)
    return out


class FrameStepNominal(C.Structure):
    _fields_ = [("k", C.c_int), ("imu", c_dp), ("gnss_idx", C.c_int * 5), ("marg_idx", C.c_int)]


def make_nominal(t):
    """t: dict(kind [n], idx [n], anchor [n], val [n][15], clone_var [c], v_ext, v_pose, v_bg, v_ba, gravity [3])"""
    keep = dict(kind=i32(t["kind"]), idx=i32(t["idx"]), anchor=i32(t["anchor"]), val=f64(np.asarray(t["val"], dtype=np.float64).reshape(-1, NOM_VAL)),
                clone_var=i32(t["clone_var"]))
    q = Nominal()
    q.n_var = len(keep["kind"]); q.kind = _i(keep["kind"]); q.idx = _i(keep["idx"]); q.anchor = _i(keep["anchor"]); q.val = _d(keep["val"])
    q.n_clones = len(keep["clone_var"]); q.clone_var = _i(keep["clone_var"])
    q.v_ext, q.v_pose, q.v_bg, q.v_ba = int(t["v_ext"]), int(t["v_pose"]), int(t["v_bg"]), int(t["v_ba"])
    q.gravity = (C.c_double * 3)(*np.asarray(t["gravity"], dtype=np.float64).reshape(3))
    return q, keep


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libingvio_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`"
                               % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.ingvio_last_error.restype = C.c_char_p
        _lib.ingvio_ctx_stream.restype = C.c_void_p
        _lib.ingvio_build_id.restype = C.c_char_p
    return _lib


def build_id():
    """{"tu": {...}, "kernels": {...}} of the LOADED library (ingvio_build_id, written by build.py at build time)."""
    import json
    return json.loads(lib().ingvio_build_id().decode())


def _d(a):
    return a.ctypes.data_as(c_dp)


def _i(a):
    return a.ctypes.data_as(c_ip)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class IngvioError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("ingvio_hip error %d %s" % (code, msg))
        self.code = code


def make_frame(fr):
    keep = dict(clone_idx=i32(fr["clone_idx"]), clone_R=f64(fr["clone_R"]), clone_p=f64(fr["clone_p"]), pf=f64(fr["pf"]),
                anchor=i32(fr["anchor"]), obs_mask=np.ascontiguousarray(fr["obs_mask"], dtype=np.uint64),
                uv=f64(fr["uv"]), dof=i32(fr["dof"]))
    f = MsckfFrame()
    f.n_clones = len(keep["clone_idx"]); f.clone_idx = _i(keep["clone_idx"]); f.clone_R = _d(keep["clone_R"])
    f.clone_p = _d(keep["clone_p"]); f.n_feat = keep["pf"].shape[0] if keep["pf"].size else 0; f.pf = _d(keep["pf"])
    f.anchor = _i(keep["anchor"]); f.obs_mask = keep["obs_mask"].ctypes.data_as(c_up); f.uv = _d(keep["uv"])
    f.dof = _i(keep["dof"])
    return f, keep


def make_opts(fr, max_accept=0, compress_rule=1, selected_variant=0):
    chi2 = f64(fr["chi2_table"])
    o = MsckfOpts()
    o.stereo = int(fr.get("stereo", 1))
    o.R_cl2cr = (C.c_double * 9)(*np.asarray(fr["R_cl2cr"], dtype=np.float64).reshape(9))
    o.t_cl2cr = (C.c_double * 3)(*np.asarray(fr["t_cl2cr"], dtype=np.float64).reshape(3))
    o.noise = float(fr["noise"]); o.chi2_table = _d(chi2); o.chi2_len = len(chi2)
    o.max_accept = int(max_accept); o.compress_rule = int(compress_rule); o.selected_variant = int(selected_variant)
    return o, chi2


def make_step(step):
    k = len(step["dt"])
    keep = dict(Phi=f64(np.stack([np.asarray(p).reshape(15, 15).T for p in step["Phi"]])),
                G=f64(np.stack([np.asarray(g).reshape(15, 12).T for g in step["G"]])), dt=f64(step["dt"]))
    s = FrameStep()
    s.k = k; s.Phi = _d(keep["Phi"]); s.G = _d(keep["G"]); s.dt = _d(keep["dt"])
    s.gnss_idx = (C.c_int * 5)(*[int(x) for x in step.get("gnss_idx", (-1,) * 5)])
    s.R_i2w = (C.c_double * 9)(*np.asarray(step["R_i2w"], dtype=np.float64).reshape(9))
    s.marg_idx = int(step.get("marg_idx", -1))
    return s, keep


def make_track_frame(d):
    """d: dict(drop=[...], free=[...], append=slot or -1, obs_track, obs_uv [n,4], pf_track, pf [n,3], clone_idx, clone_R, clone_p,
    feat_track, feat_anchor, feat_dof, feat_sel (optional))"""
    keep = dict(drop=i32(d.get("drop", [])), free=i32(d.get("free", [])), obs_track=i32(d.get("obs_track", [])), obs_uv=f64(d.get("obs_uv", np.zeros((0, 4)))),
                pf_track=i32(d.get("pf_track", [])), pf=f64(d.get("pf", np.zeros((0, 3)))), clone_idx=i32(d["clone_idx"]), clone_R=f64(d["clone_R"]),
                clone_p=f64(d["clone_p"]), feat_track=i32(d["feat_track"]), feat_anchor=i32(d["feat_anchor"]), feat_dof=i32(d["feat_dof"]))
    f = TrackFrame()
    f.n_drop = len(keep["drop"]); f.drop_slots = _i(keep["drop"]); f.n_free = len(keep["free"]); f.free_tracks = _i(keep["free"])
    f.append_slot = int(d.get("append", -1)); f.n_obs = len(keep["obs_track"]); f.obs_track = _i(keep["obs_track"]); f.obs_uv = _d(keep["obs_uv"])
    f.n_pf = len(keep["pf_track"]); f.pf_track = _i(keep["pf_track"]); f.pf = _d(keep["pf"])
    f.n_clones = len(keep["clone_idx"]); f.clone_idx = _i(keep["clone_idx"]); f.clone_R = _d(keep["clone_R"]); f.clone_p = _d(keep["clone_p"])
    f.n_feat = len(keep["feat_track"]); f.feat_track = _i(keep["feat_track"]); f.feat_anchor = _i(keep["feat_anchor"]); f.feat_dof = _i(keep["feat_dof"])
    if d.get("feat_sel") is not None:
        keep["feat_sel"] = np.ascontiguousarray(d["feat_sel"], dtype=np.uint64)
        f.feat_sel = keep["feat_sel"].ctypes.data_as(c_up)
    return f, keep


def make_step_raw(step):
    raw = step["raw"]
    keep = dict(imu=f64(raw["imu"]))
    s = FrameStepRaw()
    s.k = keep["imu"].shape[0]; s.imu = _d(keep["imu"])
    s.R = (C.c_double * 9)(*np.asarray(raw["R"], dtype=np.float64).reshape(9))
    for name in ("p", "v", "bg", "ba", "gravity"):
        setattr(s, name, (C.c_double * 3)(*np.asarray(raw[name], dtype=np.float64).reshape(3)))
    s.gnss_idx = (C.c_int * 5)(*[int(x) for x in step.get("gnss_idx", (-1,) * 5)])
    s.marg_idx = int(step.get("marg_idx", -1))
    return s, keep


def _gnss_opts(chi2_table, gate_rows, strong_reject, in_frame=False):
    """-> (GnssOpts, the table it points into)"""
    tab = f64(chi2_table)
    o = GnssOpts(); o.gate_rows = int(gate_rows); o.strong_reject = int(strong_reject); o.chi2_table = _d(tab); o.chi2_len = len(tab)
    o.in_frame = int(in_frame)
    return o, tab


def _landmark_opts(stereo, noise, chi2_thr, R_cl2cr, t_cl2cr, in_frame):
    o = LandmarkOpts(); o.stereo = int(bool(stereo)); o.noise = float(noise); o.chi2_thr = float(chi2_thr)
    o.R_cl2cr = (C.c_double * 9)(*f64(np.eye(3) if R_cl2cr is None else R_cl2cr).reshape(9))
    o.t_cl2cr = (C.c_double * 3)(*f64(np.zeros(3) if t_cl2cr is None else t_cl2cr).reshape(3))
    o.in_frame = int(bool(in_frame))
    return o


def _epoch_host_fields(a, e):
    """the host-owned part of a raw epoch into a GnssEpoch / GnssEpochNominal; -> the arrays it points into"""
    eph, obs = f64(e["eph"]), f64(e["obs"])
    ion = f64(e["ion"]) if e.get("ion") is not None else None
    a.n_sat = eph.shape[0]; a.eph = _d(eph); a.obs = _d(obs); a.ion = _d(ion) if ion is not None else None
    a.doy = float(e["doy"])
    a.R_enu2ecef = (C.c_double * 9)(*np.asarray(e["R_enu2ecef"], dtype=np.float64).reshape(9))
    a.anchor_ecef = (C.c_double * 3)(*e["anchor_ecef"])
    a.psr_noise_amp = float(e.get("psr_amp", 1.0)); a.dopp_noise_amp = float(e.get("dopp_amp", 1.0))
    return eph, obs, ion


class Context:
    """A batch of independent filters on one GPU (ingvio_ctx)."""

    def __init__(self, batch=1, n_max=256, c_max=11, f_max=160, m_max=64, device=0, stream=None):
        self.L = lib()
        d = CtxDesc(batch, n_max, c_max, f_max, m_max, device, stream)
        self.h = C.c_void_p()
        rc = self.L.ingvio_ctx_create(C.byref(d), C.byref(self.h))
        if rc != 0:
            msg = self.L.ingvio_last_error(self.h).decode() if self.h else "no HIP device / library"
            raise IngvioError(rc, msg)
        self.batch, self.n_max, self.c_max, self.f_max, self.device = batch, n_max, c_max, f_max, device
        self.ldp = self.L.ingvio_ldp(self.h)
        self.v_max = 0

    def close(self):
        if self.h:
            self.L.ingvio_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, soft_ok=True):
        if rc < 0 or (rc > 0 and not soft_ok):
            raise IngvioError(rc, self.L.ingvio_last_error(self.h).decode())
        return rc

    def sync(self):
        self._chk(self.L.ingvio_sync(self.h))

    def set_method(self, method):
        """'dense' (literal TSQR path) or 'factored' (default, structure-exploiting information form)."""
        self._chk(self.L.ingvio_set_msckf_method(self.h, {"dense": 0, "factored": 1}[method]))

    def set_qr_method(self, method):
        """qr_compress: "auto" (default), "householder", "cholesky" (ingvio_set_qr_method)"""
        self._chk(self.L.ingvio_set_qr_method(self.h, {"auto": 0, "householder": 1, "cholesky": 2}[method]))

    def debug_read(self, n=32):
        out = (C.c_longlong * n)()
        self._chk(self.L.ingvio_debug_read(self.h, out, n))
        return list(out)

    def stream(self):
        return self.L.ingvio_ctx_stream(self.h)

    # ---- covariance I/O -----------------------------------------------------------------
    def cov_set(self, b, P):
        P = np.asfortranarray(P, dtype=np.float64)
        n = P.shape[0]
        self._chk(self.L.ingvio_cov_set(self.h, b, _d(P), max(n, 1), n))

    def n(self, b=0):
        v = C.c_int(0)
        self._chk(self.L.ingvio_get_n(self.h, b, C.byref(v)))
        return v.value

    def cov_get(self, b=0):
        n = self.n(b)
        P = np.zeros((n, n), order="F")
        self._chk(self.L.ingvio_cov_get(self.h, b, _d(P), max(n, 1)))
        return P

    def marginal(self, b, vidx, vsize):
        ns = int(np.sum(vsize))
        out = np.zeros((ns, ns), order="F")
        self._chk(self.L.ingvio_cov_get_marginal(self.h, b, _i(i32(vidx)), _i(i32(vsize)), len(vidx), _d(out)))
        return out

    def snapshot(self):
        self._chk(self.L.ingvio_cov_snapshot(self.h))

    def restore(self):
        self._chk(self.L.ingvio_cov_restore(self.h))

    # ---- structure + propagation (batched over [b0, b0+nb)) ------------------------------
    def propagate(self, b0, Phi, G, dt, sigma, enable_gnss=0, gnss_idx=None, sigma_cb=0.0, sigma_rw=0.0, fused=False):
        """Phi [nb,k,15,15] (row-major numpy), G [nb,k,15,12], dt [nb,k]."""
        Phi = np.asarray(Phi, dtype=np.float64); G = np.asarray(G, dtype=np.float64); dt = np.asarray(dt, dtype=np.float64)
        if Phi.ndim == 2:
            Phi = Phi[None, None]; G = G[None, None]; dt = dt.reshape(1, 1)
        elif Phi.ndim == 3:
            Phi = Phi[None]; G = G[None]; dt = dt.reshape(1, -1)
        nb, k = Phi.shape[0], Phi.shape[1]
        PhiC = f64(np.swapaxes(Phi, -1, -2)); GC = f64(np.swapaxes(G, -1, -2)); dt = f64(dt)
        gi = None if gnss_idx is None else i32(np.asarray(gnss_idx).reshape(nb, 5))
        sig = f64(sigma)
        if fused or k > 1:
            rc = self.L.ingvio_propagate_fused(self.h, b0, nb, k, _d(PhiC), _d(GC), _d(dt), _d(sig), int(enable_gnss),
                                               _i(gi) if gi is not None else None, C.c_double(sigma_cb), C.c_double(sigma_rw))
        else:
            rc = self.L.ingvio_propagate(self.h, b0, nb, _d(PhiC), _d(GC), _d(dt), _d(sig), int(enable_gnss),
                                         _i(gi) if gi is not None else None, C.c_double(sigma_cb), C.c_double(sigma_rw))
        self._chk(rc)

    def augment(self, b0, R_i2w):
        R = f64(np.asarray(R_i2w).reshape(-1, 9))
        nb = R.shape[0]
        idx = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_augment_clone(self.h, b0, nb, _d(R), _i(idx)))
        return idx

    def marginalize(self, b0, idx, size):
        idx = i32(np.atleast_1d(idx))
        self._chk(self.L.ingvio_marginalize(self.h, b0, len(idx), _i(idx), int(size)))

    def append_independent(self, b0, blk):
        blk = np.asarray(blk, dtype=np.float64)
        if blk.ndim == 2:
            blk = blk[None]
        nb, s = blk.shape[0], blk.shape[1]
        b = f64(np.swapaxes(blk, -1, -2))
        idx = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_append_independent(self.h, b0, nb, s, _d(b), _i(idx)))
        return idx

    # ---- updates ----------------------------------------------------------------------------
    @staticmethod
    def _R(R, m):
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 0 or (R.size == 1 and m != 1):
            return f64(R.reshape(1)), R_SCALAR
        if R.ndim == 1:
            return f64(R), R_DIAG
        return np.asfortranarray(R), R_FULL

    def ekf_update(self, b, vidx, vsize, H, res, R):
        H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
        m = H.shape[0]
        Rb, kind = self._R(R, m)
        dx = np.zeros(self.n(b))
        rc = self.L.ingvio_ekf_update(self.h, b, _i(i32(vidx)), _i(i32(vsize)), len(vidx), _d(H), m, m, _d(f64(res)),
                                      _d(Rb), kind, _d(dx))
        return dx, self._chk(rc)

    def chi2_gamma(self, b, vidx, vsize, H, res, R):
        H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
        m = H.shape[0]
        Rb, kind = self._R(R, m)
        g = C.c_double(0.0)
        self._chk(self.L.ingvio_chi2_gamma(self.h, b, _i(i32(vidx)), _i(i32(vsize)), len(vidx), _d(H), m, m, _d(f64(res)),
                                           _d(Rb), kind, C.byref(g)))
        return g.value

    def ekf_update_batch(self, b0, blocks, diag=True):
        """blocks: list of (vidx, vsize, H, res, R) for filters b0, b0+1, ...; R scalar or 1-D per block (all of one kind).
        Returns (dx[nb, ldp], status[nb])."""
        nb = len(blocks)
        arr = (UpdateBlock * nb)(); keep = []
        for g, (vidx, vsize, H, res, R) in enumerate(blocks):
            H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
            vi, vs, r, Rv = i32(vidx), i32(vsize), f64(res), f64(np.atleast_1d(R))
            keep.append((H, vi, vs, r, Rv))
            arr[g].vidx = _i(vi); arr[g].vsize = _i(vs); arr[g].k = len(vi); arr[g].H = _d(H); arr[g].ldh = H.shape[0]
            arr[g].m = H.shape[0]; arr[g].res = _d(r); arr[g].R = _d(Rv)
        dx = np.zeros((nb, self.ldp)); st = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_ekf_update_batch(self.h, b0, nb, arr, 1 if diag else 0, _d(dx), _i(st)))
        return dx, st

    # ---- GnssUpdate::updateTrackedSys for a batch: per-row gates + compaction + block gate + ekfUpdate on the device ----
    @staticmethod
    def _update_blocks(blocks):
        nb = len(blocks)
        arr = (UpdateBlock * nb)(); keep = []
        for g, blk in enumerate(blocks):
            if blk is None:                               # no measurement for this filter
                arr[g].m = 0; arr[g].k = 0
                continue
            vidx, vsize, H, res, R = blk
            H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
            vi, vs, r, Rv = i32(vidx), i32(vsize), f64(res), f64(np.atleast_1d(R))
            keep.append((H, vi, vs, r, Rv))
            arr[g].vidx = _i(vi); arr[g].vsize = _i(vs); arr[g].k = len(vi); arr[g].H = _d(H); arr[g].ldh = H.shape[0]
            arr[g].m = H.shape[0]; arr[g].res = _d(r); arr[g].R = _d(Rv)
        return arr, keep

    def gnss_stage(self, b0, blocks, chi2_table, gate_rows=True, strong_reject=False, in_frame=False):
        """blocks: per filter (vidx, vsize, H [m, nc] candidate rows, res [m], Rdiag [m]) or None.  in_frame: applied by frame_run
        right after the frame's MSCKF update, in the same sweep over P (no gnss_run)."""
        arr, keep = self._update_blocks(blocks)
        o, tab = _gnss_opts(chi2_table, gate_rows, strong_reject, in_frame)
        self._chk(self.L.ingvio_gnss_stage(self.h, b0, len(blocks), arr, C.byref(o)))
        self._gnss_range = (b0, len(blocks))

    @staticmethod
    def _gnss_epochs(epochs):
        nb = len(epochs)
        arr = (GnssEpoch * nb)(); keep = []
        for i, e in enumerate(epochs):
            a = arr[i]
            keep.append(_epoch_host_fields(a, e))
            a.p_w = (C.c_double * 3)(*e["p_w"]); a.v_w = (C.c_double * 3)(*e["v_w"])
            a.cb = (C.c_double * 4)(*e["cb"]); a.fs = float(e["fs"]); a.yaw_offset = float(e["yaw_offset"])
            a.idx_se23 = int(e["idx_se23"]); a.idx_yof = int(e["idx_yof"]); a.idx_fs = int(e["idx_fs"])
            a.idx_cb = (C.c_int * 4)(*[int(x) for x in e["idx_cb"]])
        return arr, keep

    def gnss_sat_eval(self, epochs):
        """ingvio_gnss_sat_eval: the front's per-satellite records [n_epochs, 64, 20] for free-standing epochs (dicts as for
        gnss_front_stage; the idx_* entries may be omitted)."""
        eps = [dict(dict(idx_se23=0, idx_yof=0, idx_fs=0, idx_cb=[-1] * 4), **e) for e in epochs]
        arr, keep = self._gnss_epochs(eps)
        out = np.zeros((len(eps), 64, 20))
        self._chk(self.L.ingvio_gnss_sat_eval(self.h, len(eps), arr, _d(out)))
        return out

    def gnss_front_stage(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False):
        """epochs: per filter a dict(eph [ns,25], obs [ns,6], ion [8] or None, doy, p_w, v_w, cb [4], fs, yaw_offset, R_enu2ecef [3,3],
        anchor_ecef, idx_se23, idx_yof, idx_fs, idx_cb [4], psr_amp, dopp_amp): raw GNSS epochs -> candidate rows on the device."""
        self.gnss_front_stage_prepare(b0, epochs, chi2_table, gate_rows, strong_reject)()

    def gnss_front_stage_prepare(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False):
        """builds the C arguments of gnss_front_stage once and returns a callable that issues the stage"""
        nb = len(epochs)
        arr, keep = self._gnss_epochs(epochs)
        o, tab = _gnss_opts(chi2_table, gate_rows, strong_reject)

        def call(_keep=(keep, tab, arr, o)):
            self._chk(self.L.ingvio_gnss_front_stage(self.h, b0, nb, arr, C.byref(o)))
            self._gnss_range = (b0, nb)
        return call

    def gnss_front_stage_nominal_prepare(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False, in_frame=False):
        """ingvio_gnss_front_stage_nominal: epochs per filter a dict(eph, obs, ion, doy, R_enu2ecef, anchor_ecef, psr_amp, dopp_amp) or None
        (no epoch: n_sat = 0); the receiver state comes from the device nominal table.  Returns a callable that issues the stage."""
        nb = len(epochs)
        arr = (GnssEpochNominal * nb)(); keep = []
        for i, e in enumerate(epochs):
            a = arr[i]
            if e is None:
                a.n_sat = 0
                continue
            keep.append(_epoch_host_fields(a, e))
        o, tab = _gnss_opts(chi2_table, gate_rows, strong_reject, in_frame)

        def call(_keep=(keep, tab, arr, o)):
            self._chk(self.L.ingvio_gnss_front_stage_nominal(self.h, int(b0), nb, arr, C.byref(o)))
            self._gnss_range = (b0, nb)
        return call

    def gnss_front_stage_nominal(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False, in_frame=False):
        self.gnss_front_stage_nominal_prepare(b0, epochs, chi2_table, gate_rows, strong_reject, in_frame)()

    def gnss_frame_stage_nominal_prepare(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False):
        """ingvio_gnss_frame_stage_nominal: the raw epochs (as for gnss_front_stage_nominal) of the frame staged from the table, issued between
        frame_stage_tracks_nominal and frame_run, which applies them.  Returns a callable that issues the stage."""
        nb = len(epochs)
        arr = (GnssEpochNominal * nb)(); keep = []
        for i, e in enumerate(epochs):
            a = arr[i]
            if e is None:
                a.n_sat = 0
                continue
            keep.append(_epoch_host_fields(a, e))
        o, tab = _gnss_opts(chi2_table, gate_rows, strong_reject)

        def call(_keep=(keep, tab, arr, o)):
            self._chk(self.L.ingvio_gnss_frame_stage_nominal(self.h, int(b0), nb, arr, C.byref(o)))
            self._gnss_range = (b0, nb)
        return call

    def gnss_frame_stage_nominal(self, b0, epochs, chi2_table, gate_rows=True, strong_reject=False):
        self.gnss_frame_stage_nominal_prepare(b0, epochs, chi2_table, gate_rows, strong_reject)()

    def debug_gnss_fused_last(self):
        """0: no GNSS results of their own slots, 1: the update that ran last was a pass of its own, 2: it rode on the MSCKF write-back"""
        return int(self.L.ingvio_debug_gnss_fused_last(self.h))

    def debug_nominal_update_post(self, b0, dx, marg_idx):
        """the folded order's retraction kernel alone, on the table only: dx [nb, ldp] in the index space behind the marginalisation"""
        dx = f64(dx); mg = i32(marg_idx)
        self._chk(self.L.ingvio_debug_nominal_update_post(self.h, int(b0), len(mg), _d(dx), _i(mg)))

    def gnss_front_fetch(self, b0=None, nb=None):
        """-> [nb, 64, 20]: res_pos, res_vel, los (3), az, el, ion, tro, usable, then the SatState: pos (3), vel (3), dt, ddt, tgd, ttx"""
        b0, nb = (self._gnss_range if b0 is None else (b0, nb))
        out = np.zeros((nb, 64, 20))
        self._chk(self.L.ingvio_gnss_front_fetch(self.h, b0, nb, _d(out)))
        return out

    def debug_gnss_staged_rows(self, b):
        """ingvio_debug_gnss_staged_rows: -> (H [m, nc], res [m], noise [m], colmap [nc]) of filter b's candidate rows as staged"""
        mld = self.L.ingvio_mld(self.h)
        H = np.zeros((mld, 32), order="F"); res = np.zeros(mld); noise = np.zeros(mld); cm = np.zeros(32, dtype=np.int32)
        m = C.c_int(0); nc = C.c_int(0)
        self._chk(self.L.ingvio_debug_gnss_staged_rows(self.h, int(b), _d(H), _d(res), _d(noise), _i(cm), C.byref(m), C.byref(nc)))
        return H[:m.value, :nc.value].copy(), res[:m.value].copy(), noise[:m.value].copy(), cm[:nc.value].copy()

    def frame_run_phase(self, phase, restore_prior=False):
        """1: propagate + clone + gate + Gram of the staged features; 2: solve + apply + marginalise (ingvio_frame_run_phase)"""
        self._chk(self.L.ingvio_frame_run_phase(self.h, int(restore_prior), int(phase)))

    def info_reduce(self, b):
        """[A | b | n_accepted] of filter b summed over its chunk partials ON THE DEVICE: returns (device pointer, count of
        doubles, ncol) - the buffer the feature-sharded filter all-reduces in place (ingvio_info_reduce)."""
        ptr = C.POINTER(C.c_double)(); cnt = C.c_int(0); nc = C.c_int(0)
        self._chk(self.L.ingvio_info_reduce(self.h, b, C.byref(ptr), C.byref(cnt), C.byref(nc)))
        return C.cast(ptr, C.c_void_p).value, cnt.value, nc.value

    def info_commit(self, b):
        self._chk(self.L.ingvio_info_commit(self.h, b))

    def info_set(self, b, A, n_accepted):
        A = f64(A)
        self._chk(self.L.ingvio_info_set(self.h, b, _d(A), A.shape[0], int(n_accepted)))

    def landmark_stage(self, b0, frames, stereo, noise, chi2_thr, R_cl2cr=None, t_cl2cr=None, in_frame=False):
        """frames: per filter a dict(R_i2w, p_i2w, R_cl2i, p_c2i, idx_epose, idx_ext, lm_idx [L], anchor_idx [L], pf [L,3], uv [L,4],
        tracked [L]): the in-state landmarks seen in the current frame (ingvio_landmark_stage)."""
        nb = len(frames)
        arr = (LandmarkFrame * nb)(); keep = []
        for i, f in enumerate(frames):
            li = np.ascontiguousarray(f["lm_idx"], dtype=np.int32); ai = np.ascontiguousarray(f["anchor_idx"], dtype=np.int32)
            pf = f64(f["pf"]).reshape(-1, 3); uv = f64(f["uv"]).reshape(-1, 4)
            tr = np.ascontiguousarray(f.get("tracked", np.ones(len(li))), dtype=np.uint8)
            keep.append((li, ai, pf, uv, tr))
            a = arr[i]
            a.R_i2w = (C.c_double * 9)(*f64(f["R_i2w"]).reshape(9)); a.p_i2w = (C.c_double * 3)(*f64(f["p_i2w"]).reshape(3))
            a.R_cl2i = (C.c_double * 9)(*f64(f["R_cl2i"]).reshape(9)); a.p_c2i = (C.c_double * 3)(*f64(f["p_c2i"]).reshape(3))
            a.idx_epose = int(f["idx_epose"]); a.idx_ext = int(f["idx_ext"]); a.n_lm = len(li)
            a.lm_idx = _i(li); a.anchor_idx = _i(ai); a.pf = _d(pf); a.uv = _d(uv); a.tracked = tr.ctypes.data_as(C.POINTER(C.c_ubyte))
        o = _landmark_opts(stereo, noise, chi2_thr, R_cl2cr, t_cl2cr, in_frame)
        self._chk(self.L.ingvio_landmark_stage(self.h, b0, nb, arr, C.byref(o)))
        self._lm_range = (b0, nb)

    def landmark_stage_nominal_prepare(self, b0, frames, stereo, noise, chi2_thr, R_cl2cr=None, t_cl2cr=None, in_frame=False):
        """ingvio_landmark_stage_nominal: frames per filter a dict(lm_var [L] table slots, uv [L,4], tracked [L]) or None (n_lm = 0);
        everything else comes from the device nominal table.  Returns a callable that issues the stage."""
        nb = len(frames)
        arr = (LandmarkFrameNominal * nb)(); keep = []
        for i, f in enumerate(frames):
            a = arr[i]
            if f is None or len(f["lm_var"]) == 0:
                a.n_lm = 0
                continue
            lv = np.ascontiguousarray(f["lm_var"], dtype=np.int32); uv = f64(f["uv"]).reshape(-1, 4)
            tr = np.ascontiguousarray(f.get("tracked", np.ones(len(lv))), dtype=np.uint8)
            keep.append((lv, uv, tr))
            a.n_lm = len(lv); a.lm_var = _i(lv); a.uv = _d(uv); a.tracked = tr.ctypes.data_as(C.POINTER(C.c_ubyte))
        o = _landmark_opts(stereo, noise, chi2_thr, R_cl2cr, t_cl2cr, in_frame)

        def call(_keep=(keep, arr, o)):
            self._chk(self.L.ingvio_landmark_stage_nominal(self.h, int(b0), nb, arr, C.byref(o)))
            self._lm_range = (b0, nb)
        return call

    def landmark_stage_nominal(self, b0, frames, stereo, noise, chi2_thr, R_cl2cr=None, t_cl2cr=None, in_frame=False):
        self.landmark_stage_nominal_prepare(b0, frames, stereo, noise, chi2_thr, R_cl2cr, t_cl2cr, in_frame)()

    def landmark_run(self, b0=None, nb=None):
        b0, nb = (self._lm_range if b0 is None else (b0, nb))
        self._chk(self.L.ingvio_landmark_run(self.h, b0, nb))

    def landmark_fetch(self, b0=None, nb=None):
        """-> (dx [nb, ldp], rows [nb], accept [nb, 64], gamma [nb, 64], status [nb])"""
        b0, nb = (self._lm_range if b0 is None else (b0, nb))
        dx = np.zeros((nb, self.ldp)); rows = np.zeros(nb, dtype=np.int32); acc = np.zeros((nb, LM_MAX), dtype=np.int32)
        gam = np.zeros((nb, LM_MAX)); st = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_landmark_fetch(self.h, b0, nb, _d(dx), _i(rows), _i(acc), _d(gam), _i(st)))
        return dx, rows, acc, gam, st

    def gnss_run(self, b0=None, nb=None):
        b0, nb = (self._gnss_range if b0 is None else (b0, nb))
        self._chk(self.L.ingvio_gnss_run(self.h, b0, nb))

    def gnss_fetch(self, b0=None, nb=None):
        """-> (dx [nb, ldp], rows [nb], keep [nb, mld], gamma [nb, mld], status [nb])"""
        b0, nb = (self._gnss_range if b0 is None else (b0, nb))
        mld = self.L.ingvio_mld(self.h)
        dx = np.zeros((nb, self.ldp)); rows = np.zeros(nb, dtype=np.int32); keep = np.zeros((nb, mld), dtype=np.int32)
        gam = np.zeros((nb, mld)); st = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_gnss_fetch(self.h, b0, nb, _d(dx), _i(rows), _i(keep), _d(gam), _i(st)))
        return dx, rows, keep, gam, st

    def gnss_update_batch(self, b0, blocks, chi2_table, gate_rows=True, strong_reject=False):
        self.gnss_stage(b0, blocks, chi2_table, gate_rows, strong_reject)
        self.gnss_run()
        return self.gnss_fetch()

    def debug_msckf_info(self, b):
        """[A | b] of filter b's last MSCKF update: (A [ncol, ncol], b [ncol])."""
        cap = 6 * self.c_max
        out = np.zeros(cap * (cap + 1)); nc = C.c_int(0)
        self._chk(self.L.ingvio_debug_msckf_info(self.h, b, _d(out), C.byref(nc)))
        n = nc.value
        M = out[:n * (n + 1)].reshape(n, n + 1)
        return M[:, :n].copy(), M[:, n].copy()

    def debug_info_solution(self, b):
        """(M [nc, nc], t [nc]) of filter b's last factored update, nc = 6 * (window class of c_max)."""
        cls = 6 if self.c_max <= 6 else (11 if self.c_max <= 11 else 16)
        nc = 6 * cls; mp = (nc + 3) & ~3
        out = np.zeros(mp * mp + mp)
        self._chk(self.L.ingvio_debug_info_solution(self.h, b, _d(out), out.size))
        return out[:mp * mp].reshape(mp, mp)[:nc, :nc].copy(), out[mp * mp:mp * mp + nc].copy()

    def chi2_gamma_multi(self, b, blocks, noise_var):
        """blocks: list of (vidx, vsize, H, res); returns gamma[len(blocks)] (one launch, one sync)."""
        nb = len(blocks)
        arr = (GateBlock * nb)(); keep = []
        for g, (vidx, vsize, H, res) in enumerate(blocks):
            H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
            vi, vs, r = i32(vidx), i32(vsize), f64(res)
            keep.append((H, vi, vs, r))
            arr[g].vidx = _i(vi); arr[g].vsize = _i(vs); arr[g].k = len(vi); arr[g].H = _d(H); arr[g].ldh = H.shape[0]
            arr[g].m = H.shape[0]; arr[g].res = _d(r)
        out = np.zeros(max(nb, 1))
        self._chk(self.L.ingvio_chi2_gamma_multi(self.h, b, nb, arr, C.c_double(noise_var), _d(out)))
        return out[:nb]

    # ---- SLAM-landmark path (f-2) --------------------------------------------------------------
    def add_variable_delayed_invertible(self, b, vidx, vsize, H_old, H_new, noise):
        H_old = np.asfortranarray(np.atleast_2d(H_old), dtype=np.float64)
        H_new = np.asfortranarray(np.atleast_2d(H_new), dtype=np.float64)
        s = H_new.shape[0]
        idx = C.c_int(-1)
        self._chk(self.L.ingvio_add_variable_delayed_invertible(self.h, b, _i(i32(vidx)), _i(i32(vsize)), len(vidx), _d(H_old), s,
                                                                _d(H_new), s, s, C.c_double(noise), C.byref(idx)))
        return idx.value

    def add_variable_delayed(self, b, vidx, vsize, H_old, H_new, res, noise, chi2_mult=1.0, do_chi2=True, chi2_check=None):
        """Returns (added, dx[n+s] or None, chi2, new_idx)."""
        H_old = np.asfortranarray(np.atleast_2d(H_old), dtype=np.float64)
        H_new = np.asfortranarray(np.atleast_2d(H_new), dtype=np.float64)
        m, s = H_new.shape
        if chi2_check is None:
            from scipy.stats import chi2 as _chi2
            chi2_check = float(_chi2.ppf(0.95, m))
        dx = np.zeros(self.n(b) + s); added = C.c_int(0); idx = C.c_int(-1); chi2 = C.c_double(0.0)
        self._chk(self.L.ingvio_add_variable_delayed(self.h, b, _i(i32(vidx)), _i(i32(vsize)), len(vidx), _d(H_old), m, _d(H_new), m,
                                                     m, s, _d(f64(res)), C.c_double(noise), C.c_double(chi2_mult),
                                                     1 if do_chi2 else 0, C.c_double(chi2_check), _d(dx), C.byref(added),
                                                     C.byref(idx), C.byref(chi2)))
        return bool(added.value), (dx if added.value else None), chi2.value, idx.value

    def add_variable_delayed_batch(self, b0, blocks, noise, chi2_mult=1.0, do_chi2=True, want_dx=True):
        """addVariableDelayed for filters b0, b0+1, ..., several candidates each (make_delayed_blocks), one synchronisation.
        Returns per filter (added [bool], new_idx [int], chi2 [float], dx [array of the state after the append, or None]), one
        entry per candidate; self.delayed_status holds the per-filter status codes of the call (OK, NEG_DIAG or E_NOT_PD: after a trailing
        update whose S is not positive definite the variable stays appended, its dx is zero and the filter's later candidates are not tried)."""
        nb = len(blocks)
        arr, cap, keep = make_delayed_blocks(blocks)
        added = np.zeros((nb, cap), dtype=np.int32); idx = np.full((nb, cap), -1, dtype=np.int32); chi2 = np.zeros((nb, cap))
        dx = np.zeros((nb, cap, self.ldp)) if want_dx else None
        st = np.zeros(nb, dtype=np.int32)
        rc = self.L.ingvio_add_variable_delayed_batch(self.h, b0, nb, arr, C.c_double(noise), C.c_double(chi2_mult), 1 if do_chi2 else 0,
                                                      cap, _i(added), _i(idx), _d(chi2), _d(dx) if want_dx else None, _i(st))
        # NEG_DIAG / E_NOT_PD of a trailing update come back AFTER the state has grown: they are reported per filter in
        # delayed_status beside the results, never raised; everything else negative is a refusal that changed nothing
        if rc != E_NOT_PD:
            self._chk(rc)
        self.delayed_status = st
        out = []
        for g, cands in enumerate(blocks):
            k = len(cands)
            dxs = [(dx[g, j, :idx[g, j] + arr[g].cand[j].s].copy() if want_dx and added[g, j] else None) for j in range(k)]
            out.append(([bool(a) for a in added[g, :k]], [int(v) for v in idx[g, :k]], [float(v) for v in chi2[g, :k]], dxs))
        return out

    def landmark_init_nominal(self, b0, blocks, opts_frame, chi2_mult=1.0, do_chi2=True, want_dx=True):
        """ingvio_landmark_init_nominal for filters b0, b0+1, ...: blocks as make_lm_init_blocks takes them, opts_frame a dict with
        stereo / R_cl2cr / t_cl2cr / noise / chi2_table (make_opts).  Returns per filter (added [bool], new_idx [int], chi2 [float],
        dx [array of the state after the append, or None], slot [int]), one entry per candidate; self.delayed_status as
        add_variable_delayed_batch leaves it."""
        nb = len(blocks)
        arr, cap, keep = make_lm_init_blocks(blocks)
        o, tab = make_opts(opts_frame)
        added = np.zeros((nb, cap), dtype=np.int32); idx = np.full((nb, cap), -1, dtype=np.int32); slot = np.full((nb, cap), -1, dtype=np.int32)
        chi2 = np.zeros((nb, cap)); dx = np.zeros((nb, cap, self.ldp)) if want_dx else None
        st = np.zeros(nb, dtype=np.int32)
        rc = self.L.ingvio_landmark_init_nominal(self.h, int(b0), nb, arr, C.byref(o), C.c_double(chi2_mult), 1 if do_chi2 else 0, cap,
                                                 _i(added), _i(idx), _i(slot), _d(chi2), _d(dx) if want_dx else None, _i(st))
        if rc != E_NOT_PD:
            self._chk(rc)
        self.delayed_status = st
        out = []
        for g, bk in enumerate(blocks):
            k = len(bk["cands"])
            dxs = [(dx[g, j, :idx[g, j] + 3].copy() if want_dx and added[g, j] else None) for j in range(k)]
            out.append(([bool(a) for a in added[g, :k]], [int(v) for v in idx[g, :k]], [float(v) for v in chi2[g, :k]], dxs,
                        [int(v) for v in slot[g, :k]]))
        return out

    def debug_landmark_init_rows(self, b, cand, opts_frame, n_clones, drop=()):
        """the rows ingvio_landmark_init_nominal forms for filter b (its table's window holds n_clones clones) and the candidate
        (track, anchor, pf): (H_old [m, 6 n_clones], H_new [m, 3], res [m])"""
        o, tab = make_opts(opts_frame)
        ca = LmInitCand(); ca.track = int(cand[0]); ca.anchor = int(cand[1]); ca.pf = (C.c_double * 3)(*f64(cand[2]).reshape(3))
        drop = i32(list(drop))
        mw, nc = (4 if o.stereo else 2) * self.c_max, 6 * self.c_max
        H_old = np.zeros(mw * nc); H_new = np.zeros(mw * 3); res = np.zeros(mw); m = C.c_int(0)
        self._chk(self.L.ingvio_debug_landmark_init_rows(self.h, int(b), C.byref(ca), C.byref(o), len(drop), _i(drop) if len(drop) else None,
                                                         _d(H_old), _d(H_new), _d(res), C.byref(m)))
        m, nc = m.value, 6 * int(n_clones)
        return (H_old[:m * nc].reshape(nc, m).T.copy(), H_new[:3 * m].reshape(3, m).T.copy(), res[:m].copy())

    def gnss_init_nominal_prepare(self, b0, blocks, chi2_table, chi2_mult=0.95, do_chi2=True, want_dx=True):
        """builds the C arguments of ingvio_gnss_init_nominal once (blocks as make_gnss_init_blocks takes them) and returns a callable
        that issues the call and returns dict(added, new_idx, slot [nb, 5] int, chi2, noise [nb, 5], dx [nb, 5, ldp] or None, status [nb]);
        self.delayed_status as add_variable_delayed_batch leaves it."""
        nb = len(blocks)
        arr, keep = make_gnss_init_blocks(blocks)
        tab = f64(chi2_table)

        def call(_keep=(keep, arr, tab)):
            K = GNSS_INIT_CAND
            added = np.zeros((nb, K), dtype=np.int32); idx = np.full((nb, K), -1, dtype=np.int32); slot = np.full((nb, K), -1, dtype=np.int32)
            chi2 = np.zeros((nb, K)); noise = np.zeros((nb, K)); dx = np.zeros((nb, K, self.ldp)) if want_dx else None
            st = np.zeros(nb, dtype=np.int32)
            rc = self.L.ingvio_gnss_init_nominal(self.h, int(b0), nb, arr, _d(tab), len(tab), C.c_double(chi2_mult), 1 if do_chi2 else 0,
                                                 _i(added), _i(idx), _i(slot), _d(chi2), _d(noise), _d(dx) if want_dx else None, _i(st))
            if rc != E_NOT_PD:
                self._chk(rc)
            self.delayed_status = st
            return dict(added=added, new_idx=idx, slot=slot, chi2=chi2, noise=noise, dx=dx, status=st)
        return call

    def gnss_init_nominal(self, b0, blocks, chi2_table, chi2_mult=0.95, do_chi2=True, want_dx=True):
        """ingvio_gnss_init_nominal for filters b0, b0+1, ...: GnssUpdate::addNewTrackedSys from the device nominal table"""
        return self.gnss_init_nominal_prepare(b0, blocks, chi2_table, chi2_mult, do_chi2, want_dx)()

    def debug_gnss_init_rows(self, b, block, g):
        """the rows ingvio_gnss_init_nominal forms for filter b, its block and candidate g: (H_old [m, 10], res [m], noise)"""
        arr, keep = make_gnss_init_blocks([block])
        H = np.zeros(64 * 10); res = np.zeros(64); noise = C.c_double(0.0); m = C.c_int(0)
        self._chk(self.L.ingvio_debug_gnss_init_rows(self.h, int(b), arr, int(g), _d(H), _d(res), C.byref(noise), C.byref(m)))
        m = m.value
        return H[:10 * m].reshape(10, m).T.copy(), res[:m].copy(), noise.value

    def replace_var_linear(self, b, tidx, tsize, vidx, vsize, H):
        H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
        self._chk(self.L.ingvio_replace_var_linear(self.h, b, int(tidx), int(tsize), _i(i32(vidx)), _i(i32(vsize)), len(vidx),
                                                   _d(H), H.shape[0]))

    def msckf_update(self, b0, frames, max_accept=0, compress_rule=1, selected_variant=0):
        """frames: list of frame dicts (one per filter).  Returns (dx[nb,n], accepted[nb,F], gamma[nb,F], rows[nb])."""
        if isinstance(frames, dict):
            frames = [frames]
        nb = len(frames)
        arr = (MsckfFrame * nb)()
        keeps = []
        for i, fr in enumerate(frames):
            f, k = make_frame(fr)
            arr[i] = f; keeps.append(k)
        o, chi2 = make_opts(frames[0], max_accept, compress_rule, selected_variant)
        dx = np.zeros((nb, self.ldp)); acc = np.zeros((nb, self.f_max), dtype=np.int32)
        gam = np.zeros((nb, self.f_max)); rows = np.zeros(nb, dtype=np.int32)
        rc = self.L.ingvio_msckf_update(self.h, b0, nb, arr, C.byref(o), _d(dx), _i(acc), _d(gam), _i(rows))
        self._chk(rc)
        return dx, acc, gam, rows

    def msckf_update_tri(self, b0, frames, max_accept=0, compress_rule=1, selected_variant=0, stereo=True, tri_masks=None, **params):
        """ingvio_msckf_update_tri: the frames' points are triangulated on the device from their own observations (pf of the frame
        dicts is ignored), failed features drop out.  Returns (dx, accepted, gamma, rows, pf[nb, f_max, 3], tri_ok[nb, f_max])."""
        if isinstance(frames, dict):
            frames = [frames]
        nb = len(frames)
        arr = (MsckfFrame * nb)()
        keeps = []
        for i, fr in enumerate(frames):
            f, k = make_frame(fr)
            arr[i] = f; keeps.append(k)
        o, chi2 = make_opts(frames[0], max_accept, compress_rule, selected_variant)
        pr = dict(trans_thres=0.1, huber_epsilon=0.01, conv_precision=5e-7, init_damping=1e-3, outer_loop_max_iter=10,
                  inner_loop_max_iter=10, max_depth=60.0, min_depth=0.2)
        pr.update(params)
        t = TriOpts()
        t.stereo = 1 if stereo else 0
        Rl = f64(frames[0]["R_cl2cr"]).reshape(-1); tl = f64(frames[0]["t_cl2cr"])
        for i in range(9):
            t.R_cl2cr[i] = float(Rl[i])
        for i in range(3):
            t.t_cl2cr[i] = float(tl[i])
        for k, v in pr.items():
            setattr(t, k, v)
        dx = np.zeros((nb, self.ldp)); acc = np.zeros((nb, self.f_max), dtype=np.int32)
        gam = np.zeros((nb, self.f_max)); rows = np.zeros(nb, dtype=np.int32)
        pf = np.zeros((nb, self.f_max, 3)); ok = np.zeros((nb, self.f_max), dtype=np.int32)
        tm = None
        if tri_masks is not None:                              # one mask array per filter (None: the frame's obs_mask)
            tm_keep = [None if m is None else np.ascontiguousarray(m, dtype=np.uint64) for m in tri_masks]
            tm = (c_up * nb)(*[C.cast(None, c_up) if m is None else m.ctypes.data_as(c_up) for m in tm_keep])
        self._chk(self.L.ingvio_msckf_update_tri(self.h, b0, nb, arr, C.byref(o), C.byref(t), tm, _d(dx), _i(acc), _d(gam), _i(rows), _d(pf), _i(ok)))
        return dx, acc, gam, rows, pf, ok

    def qr_compress(self, H, res):
        H = np.asfortranarray(H, dtype=np.float64)
        m, n = H.shape
        Ht = np.zeros((n, n), order="F"); rt = np.zeros(n)
        self._chk(self.L.ingvio_qr_compress(self.h, _d(H), m, m, n, _d(f64(res)), _d(Ht), n, _d(rt)))
        return Ht, rt

    # ---- whole-batch frame (bench) ------------------------------------------------------------
    def frame_stage(self, b0, steps, frames, sigma, enable_gnss=0, sigma_cb=0.0, sigma_rw=0.0, max_accept=0,
                    compress_rule=1, selected_variant=0):
        self.frame_stage_prepare(b0, steps, frames, sigma, enable_gnss, sigma_cb, sigma_rw, max_accept, compress_rule, selected_variant)()

    def tracks_create(self, t_max):
        """allocates / clears the device-resident track store (ingvio_tracks_create)"""
        self._chk(self.L.ingvio_tracks_create(self.h, int(t_max)))
        self.t_max = int(t_max)

    def debug_tracks_read(self, b):
        """filter b's slice of the track store: (mask [t_max] uint64, uv [t_max, c_max, 4], pf [t_max, 3]) (ingvio_debug_tracks_read)"""
        T = getattr(self, "t_max", 0)
        mask = np.zeros(max(T, 1), dtype=np.uint64); uv = np.zeros((max(T, 1), self.c_max, 4)); pf = np.zeros((max(T, 1), 3))
        self._chk(self.L.ingvio_debug_tracks_read(self.h, int(b), mask.ctypes.data_as(c_up), _d(uv), _d(pf)))
        return mask, uv, pf

    def debug_tracks_flags(self, b):
        """filter b's point flags [t_max] uint8 of the track store (ingvio_debug_tracks_flags)"""
        has = np.zeros(max(getattr(self, "t_max", 0), 1), dtype=np.uint8)
        self._chk(self.L.ingvio_debug_tracks_flags(self.h, int(b), has.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return has

    # ---- MSCKF anchor change and invalid-feature erase on the store ------------------------------------------------
    def _maintain_args(self, blocks, move_min_depth, min_depth, list_cap, lm_cap):
        nb = len(blocks)
        arr = (MaintainBlock * max(nb, 1))(); keep = []
        for i, bk in enumerate(blocks):
            tr, lm = i32(bk.get("tracks", [])), i32(bk.get("lm_slot", []))
            keep.append((tr, lm))
            arr[i].n_tracks = len(tr); arr[i].n_lm = len(lm)
            if len(tr):
                arr[i].tracks = _i(tr)
            if len(lm):
                arr[i].lm_slot = _i(lm)
        o = MaintainOpts()
        o.move_min_depth = float(move_min_depth); o.min_depth = float(min_depth)
        o.list_cap = max([len(k[0]) for k in keep] + [1]) if list_cap is None else int(list_cap)
        o.lm_cap = max([len(k[1]) for k in keep] + [1]) if lm_cap is None else int(lm_cap)
        return nb, arr, o, keep

    def tracks_maintain_begin(self, b0, blocks, move_min_depth=0.0, min_depth=0.2, list_cap=None, lm_cap=None):
        """enqueues the anchor change / invalid-feature erase of filters b0, b0 + 1, ... (ingvio_tracks_maintain_begin); blocks are dicts
        with tracks (words as maintain_word makes them) and lm_slot, each optional.  No synchronisation."""
        nb, arr, o, keep = self._maintain_args(blocks, move_min_depth, min_depth, list_cap, lm_cap)
        self._chk(self.L.ingvio_tracks_maintain_begin(self.h, int(b0), nb, arr, C.byref(o)))
        self._maintain = (nb, o.list_cap, o.lm_cap, [(len(k[0]), len(k[1])) for k in keep])

    def tracks_maintain_end(self):
        """waits for the pending call; -> per filter a dict verdict [n_tracks] uint8, depth [n_tracks], lm_verdict [n_lm] uint8"""
        nb, lc, mc, cnt = getattr(self, "_maintain", (0, 1, 1, []))
        ver = np.zeros((max(nb, 1), max(lc, 1)), dtype=np.uint8); dep = np.zeros((max(nb, 1), max(lc, 1))); lmv = np.zeros((max(nb, 1), max(mc, 1)), dtype=np.uint8)
        ub = C.POINTER(C.c_ubyte)
        self._chk(self.L.ingvio_tracks_maintain_end(self.h, ver.ctypes.data_as(ub), _d(dep), lmv.ctypes.data_as(ub)))
        return [dict(verdict=ver[i, :nt].copy(), depth=dep[i, :nt].copy(), lm_verdict=lmv[i, :nl].copy()) for i, (nt, nl) in enumerate(cnt)]

    def tracks_maintain(self, b0, blocks, move_min_depth=0.0, min_depth=0.2, list_cap=None, lm_cap=None):
        """ingvio_tracks_maintain: begin + end in one call; returns as tracks_maintain_end"""
        nb, arr, o, keep = self._maintain_args(blocks, move_min_depth, min_depth, list_cap, lm_cap)
        ver = np.zeros((max(nb, 1), max(o.list_cap, 1)), dtype=np.uint8); dep = np.zeros((max(nb, 1), max(o.list_cap, 1)))
        lmv = np.zeros((max(nb, 1), max(o.lm_cap, 1)), dtype=np.uint8)
        ub = C.POINTER(C.c_ubyte)
        self._chk(self.L.ingvio_tracks_maintain(self.h, int(b0), nb, arr, C.byref(o), ver.ctypes.data_as(ub), _d(dep), lmv.ctypes.data_as(ub)))
        return [dict(verdict=ver[i, :len(k[0])].copy(), depth=dep[i, :len(k[0])].copy(), lm_verdict=lmv[i, :len(k[1])].copy()) for i, k in enumerate(keep)]

    def debug_staged_frame(self, b):
        """filter b's arrays of the input set the next frame_run reads (ingvio_debug_staged_frame): a dict n_clones, n_feat, clone_idx
        [c_max], clone_R [c_max, 9], clone_p [c_max, 3], anchor [f_max], dof [f_max], obs_mask [f_max], pf [f_max, 3], uv [f_max, c_max, 4]"""
        cm, fm = self.c_max, self.f_max
        nc = C.c_int(0); nf = C.c_int(0)
        o = dict(clone_idx=np.zeros(cm, dtype=np.int32), clone_R=np.zeros((cm, 9)), clone_p=np.zeros((cm, 3)), anchor=np.zeros(fm, dtype=np.int32),
                 dof=np.zeros(fm, dtype=np.int32), obs_mask=np.zeros(fm, dtype=np.uint64), pf=np.zeros((fm, 3)), uv=np.zeros((fm, cm, 4)))
        self._chk(self.L.ingvio_debug_staged_frame(self.h, int(b), C.byref(nc), C.byref(nf), _i(o["clone_idx"]), _d(o["clone_R"]), _d(o["clone_p"]),
                                                   _i(o["anchor"]), _i(o["dof"]), o["obs_mask"].ctypes.data_as(c_up), _d(o["pf"]), _d(o["uv"])))
        o["n_clones"] = nc.value; o["n_feat"] = nf.value
        return o

    def frame_stage_tracks_prepare(self, b0, steps, track_frames, opts_frame, sigma, enable_gnss=0, sigma_cb=0.0, sigma_rw=0.0, max_accept=0,
                                   compress_rule=1, selected_variant=0, use_async=False):
        """Builds the C argument arrays once and returns a callable that issues ingvio_frame_stage_tracks on them: the frame hand-over
        as a delta on the device-resident track store + raw IMU samples.  steps: step dicts with a "raw" entry (synth.Filter.step_dict);
        track_frames: dicts as make_track_frame takes them; opts_frame: a dict with stereo / R_cl2cr / t_cl2cr / noise / chi2_table."""
        nb = len(steps)
        sa = (FrameStepRaw * nb)(); fa = (TrackFrame * nb)()
        keeps = []
        for i in range(nb):
            s, k1 = make_step_raw(steps[i]); f, k2 = make_track_frame(track_frames[i])
            sa[i] = s; fa[i] = f; keeps.append((k1, k2))
        o, chi2 = make_opts(opts_frame, max_accept, compress_rule, selected_variant)
        sg = f64(sigma)

        def call():
            _keep = (keeps, chi2, sg)
            self._chk(self.L.ingvio_frame_stage_tracks(self.h, b0, nb, sa, fa, C.byref(o), _d(sg), int(enable_gnss), C.c_double(sigma_cb),
                                                       C.c_double(sigma_rw), 1 if use_async else 0))
        return call

    # ---- device-resident nominal state -------------------------------------------------------------------------
    def nominal_create(self, v_max):
        """allocates / clears the per-filter nominal table of up to v_max variables (ingvio_nominal_create)"""
        self._chk(self.L.ingvio_nominal_create(self.h, int(v_max)))
        self.v_max = int(v_max)

    def nominal_set(self, b0, tables):
        """tables: one dict per filter of [b0, b0 + len(tables)) as make_nominal takes it"""
        nb = len(tables)
        arr = (Nominal * nb)()
        keeps = []
        for i, t in enumerate(tables):
            q, k = make_nominal(t); arr[i] = q; keeps.append(k)
        self._chk(self.L.ingvio_nominal_set(self.h, int(b0), nb, arr))

    def nominal_get(self, b0=0, nb=None):
        """synchronises; a list of dicts (kind, idx, anchor, val [n_var][15], clone_var, v_ext, v_pose, v_bg, v_ba, gravity)"""
        nb = self.batch if nb is None else nb
        vm = self.v_max
        bufs = [dict(kind=np.zeros(vm, dtype=np.int32), idx=np.zeros(vm, dtype=np.int32), anchor=np.zeros(vm, dtype=np.int32),
                     val=np.zeros((vm, NOM_VAL)), clone_var=np.zeros(max(self.c_max, 1), dtype=np.int32)) for _ in range(nb)]
        arr = (Nominal * nb)()
        for i, bf in enumerate(bufs):
            arr[i].kind = _i(bf["kind"]); arr[i].idx = _i(bf["idx"]); arr[i].anchor = _i(bf["anchor"]); arr[i].val = _d(bf["val"])
            arr[i].clone_var = _i(bf["clone_var"])
        self._chk(self.L.ingvio_nominal_get(self.h, int(b0), nb, arr))
        out = []
        for i, bf in enumerate(bufs):
            q = arr[i]
            n, c = q.n_var, q.n_clones
            out.append(dict(kind=bf["kind"][:n].copy(), idx=bf["idx"][:n].copy(), anchor=bf["anchor"][:n].copy(), val=bf["val"][:n].copy(),
                            clone_var=bf["clone_var"][:c].copy(), v_ext=q.v_ext, v_pose=q.v_pose, v_bg=q.v_bg, v_ba=q.v_ba,
                            gravity=np.array(q.gravity[:])))
        return out

    def nominal_set_gnss(self, b0, slots):
        """slots [nb][6]: table slots of the clock biases GPS, GLO, GAL, BDS, then FS, then YOF; -1: not in the state (ingvio_nominal_set_gnss)"""
        sl = i32(np.asarray(slots, dtype=np.int32).reshape(-1, 6))
        self._chk(self.L.ingvio_nominal_set_gnss(self.h, int(b0), sl.shape[0], _i(sl)))

    def nominal_get_gnss(self, b0=0, nb=None):
        nb = self.batch if nb is None else nb
        sl = np.zeros((nb, 6), dtype=np.int32)
        self._chk(self.L.ingvio_nominal_get_gnss(self.h, int(b0), nb, _i(sl)))
        return sl

    def set_gnss_adjust_yof(self, on):
        """GnssUpdate::_is_adjust_yof for every GNSS launch of the context that forms rows: the YOF column (column 9) of the update rows
        and of the acquisition rows (ingvio_set_gnss_adjust_yof).  Default 0."""
        self._chk(self.L.ingvio_set_gnss_adjust_yof(self.h, int(bool(on))))

    def nominal_add_gnss(self, b0, gtype, value, var):
        """StateManager::addGNSSVariable on the device table and covariance (ingvio_nominal_add_gnss): gtype [nb] the position of
        nominal_set_gnss (0..3 clocks, 4 FS, 5 YOF; -1: nothing for this filter), value / var [nb].  No synchronisation.
        -> (slot [nb], idx [nb]); -1 where gtype is -1"""
        g = i32(np.asarray(gtype, dtype=np.int32).reshape(-1))
        nb = g.shape[0]
        val, vr = f64(np.broadcast_to(np.asarray(value, dtype=np.float64), (nb,))), f64(np.broadcast_to(np.asarray(var, dtype=np.float64), (nb,)))
        slot, idx = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int32)
        self._chk(self.L.ingvio_nominal_add_gnss(self.h, int(b0), nb, _i(g), _d(val), _d(vr), _i(slot), _i(idx)))
        return slot[:nb], idx[:nb]

    def nominal_marg_gnss(self, b0, mask):
        """StateManager::margGNSSVariable on the device (ingvio_nominal_marg_gnss): mask [nb], bit s = the scalar registered at position
        s of nominal_set_gnss; their rows and columns leave P in one sweep.  No synchronisation."""
        mk = np.ascontiguousarray(np.asarray(mask, dtype=np.uint32).reshape(-1))
        self._chk(self.L.ingvio_nominal_marg_gnss(self.h, int(b0), mk.shape[0], mk.ctypes.data_as(C.POINTER(C.c_uint))))

    # ---- odometry output -----------------------------------------------------------------------------------------
    def odom_begin(self, b0=0, nb=None, what=ODOM_ALL):
        """enqueues the odometry records of filters [b0, b0 + nb) behind everything on the stream; no synchronisation (ingvio_odom_begin)"""
        nb = self.batch - int(b0) if nb is None else nb
        self._chk(self.L.ingvio_odom_begin(self.h, int(b0), int(nb), int(what)))
        self._odom_nb = int(nb)

    def odom_end(self, raw=None, dicts=True):
        """waits for the pending records; -> a list of dicts (odom_dicts), or with dicts=False the records as one numpy array of
        ODOM_DTYPE (fields as in ingvio_odom: rec["p"] is [nb][3]).  raw: an (Odom * m) array to fill instead of a fresh one"""
        nb = getattr(self, "_odom_nb", 0)
        arr = (Odom * max(nb, 1))() if raw is None else raw
        self._chk(self.L.ingvio_odom_end(self.h, arr))
        rec = np.frombuffer(arr, dtype=ODOM_DTYPE, count=nb)
        return odom_dicts(rec) if dicts else rec

    def cov_get_marginal_batch(self, b0, lists, ns_max=None):
        """lists: per filter of [b0, b0 + len(lists)) a (vidx, vsize) pair; -> a list of ns x ns blocks (ingvio_cov_get_marginal_batch).
        ns_max: the stride's side (default: the largest ns of the call)"""
        nb = len(lists)
        k = max(1, max(len(v) for v, _ in lists))
        vidx, vsize = np.zeros((nb, k), dtype=np.int32), np.zeros((nb, k), dtype=np.int32)
        for i, (v, s) in enumerate(lists):
            vidx[i, :len(v)] = v; vsize[i, :len(s)] = s
        ns = [int(np.sum(s)) for _, s in lists]
        ns_max = max(1, max(ns)) if ns_max is None else int(ns_max)
        out = np.zeros((nb, ns_max * ns_max))
        self._chk(self.L.ingvio_cov_get_marginal_batch(self.h, int(b0), nb, _i(vidx), _i(vsize), k, ns_max, _d(out)))
        return [out[i, :m * m].reshape(m, m, order="F").copy() for i, m in enumerate(ns)]

    def nominal_box_plus(self, b0, dx):
        """StateManager::boxPlus on the device: dx [nb][ldp] in the live index space (ingvio_nominal_box_plus)"""
        d = f64(np.asarray(dx, dtype=np.float64).reshape(-1, self.ldp))
        self._chk(self.L.ingvio_nominal_box_plus(self.h, int(b0), d.shape[0], _d(d)))

    def nominal_tail(self, b0, blocks, lm_cap=None):
        """the landmark tail of a frame (ingvio_nominal_tail) for filters b0, b0+1, ...: blocks are dicts with lm_slot (landmarks to
        re-anchor, the reference's visiting order), new_anchor, erase_slot, marg_slot (each optional).  Synchronises.  Returns
        (verdict [nb][lm_cap]: 1 re-anchored, 0 behind the new anchor and marginalised; status [nb])."""
        nb = len(blocks)
        arr = (NominalTailBlock * max(nb, 1))(); keep = []
        for i, bk in enumerate(blocks):
            lm, er, mg = i32(bk.get("lm_slot", [])), i32(bk.get("erase_slot", [])), i32(bk.get("marg_slot", []))
            keep.append((lm, er, mg))
            arr[i].n_reanchor = len(lm); arr[i].n_erase = len(er); arr[i].n_marg = len(mg)
            arr[i].new_anchor = int(bk.get("new_anchor", -1))
            if len(lm):
                arr[i].lm_slot = _i(lm)
            if len(er):
                arr[i].erase_slot = _i(er)
            if len(mg):
                arr[i].marg_slot = _i(mg)
        cap = max([len(k[0]) for k in keep] + [1]) if lm_cap is None else int(lm_cap)
        verdict = np.zeros((nb, max(cap, 1)), dtype=np.int32); status = np.zeros(max(nb, 1), dtype=np.int32)
        self._chk(self.L.ingvio_nominal_tail(self.h, int(b0), nb, arr, cap, _i(verdict), _i(status)))
        return verdict[:, :cap], status[:nb]

    def frame_stage_tracks_nominal_prepare(self, b0, steps, track_frames, opts_frame, sigma, enable_gnss=0, sigma_cb=0.0, sigma_rw=0.0, max_accept=0,
                                           compress_rule=1, selected_variant=0, use_async=False):
        """as frame_stage_tracks_prepare, the nominal values from the device table (ingvio_frame_stage_tracks_nominal): steps are dicts
        imu [k][7], gnss_idx (optional), marg_idx; track_frames need no clone arrays"""
        return self._nominal_stage_prepare(False, None, b0, steps, track_frames, opts_frame, sigma, enable_gnss, sigma_cb, sigma_rw, max_accept,
                                           compress_rule, selected_variant, use_async)

    def frame_stage_tracks_nominal_tri_prepare(self, b0, steps, track_frames, opts_frame, sigma, enable_gnss=0, sigma_cb=0.0, sigma_rw=0.0, tri=None,
                                               max_accept=0, compress_rule=1, selected_variant=0, use_async=False):
        """ingvio_frame_stage_tracks_nominal_tri: as frame_stage_tracks_nominal_prepare; tri as update_stage_tracks_nominal_prepare takes it
        (None: NULL, the store's points; a dict: the run triangulates the listed features)"""
        return self._nominal_stage_prepare(True, tri, b0, steps, track_frames, opts_frame, sigma, enable_gnss, sigma_cb, sigma_rw, max_accept,
                                           compress_rule, selected_variant, use_async)

    def _nominal_stage_prepare(self, tri_export, tri, b0, steps, track_frames, opts_frame, sigma, enable_gnss, sigma_cb, sigma_rw, max_accept,
                               compress_rule, selected_variant, use_async):
        nb = len(steps)
        sa = (FrameStepNominal * nb)(); fa = (TrackFrame * nb)()
        keeps = []
        for i in range(nb):
            imu = f64(steps[i]["imu"])
            s = FrameStepNominal()
            s.k = imu.shape[0]; s.imu = _d(imu)
            s.gnss_idx = (C.c_int * 5)(*[int(x) for x in steps[i].get("gnss_idx", (-1,) * 5)])
            s.marg_idx = int(steps[i].get("marg_idx", -1))
            d = dict(track_frames[i])
            d.setdefault("clone_idx", []); d.setdefault("clone_R", np.zeros((0, 9))); d.setdefault("clone_p", np.zeros((0, 3)))
            f, k2 = make_track_frame(d)
            sa[i] = s; fa[i] = f; keeps.append((imu, k2))
        o, chi2 = make_opts(opts_frame, max_accept, compress_rule, selected_variant)
        sg = f64(sigma)
        t = None if tri is None else tri_opts(opts_frame, **tri)

        def call():
            _keep = (keeps, chi2, sg, t)
            if tri_export:
                return self._chk(self.L.ingvio_frame_stage_tracks_nominal_tri(self.h, b0, nb, sa, fa, C.byref(o), _d(sg), int(enable_gnss), C.c_double(sigma_cb),
                                                                              C.c_double(sigma_rw), None if t is None else C.byref(t), 1 if use_async else 0))
            return self._chk(self.L.ingvio_frame_stage_tracks_nominal(self.h, b0, nb, sa, fa, C.byref(o), _d(sg), int(enable_gnss),
                                                                      C.c_double(sigma_cb), C.c_double(sigma_rw), 1 if use_async else 0))
        return call

    def set_first_tri_placement(self, mode):
        """0 (default): the triangulation of a first update staged with tri runs on the compute stream in front of the gate; 1: at the
        stage, behind the gather (ingvio_set_first_tri_placement).  Bit-identical results."""
        self._chk(self.L.ingvio_set_first_tri_placement(self.h, int(mode)))

    def update_stage_tracks_nominal_prepare(self, b0, marg_idx, track_frames, opts_frame, tri=None, max_accept=0, compress_rule=1,
                                            selected_variant=0, use_async=False):
        """the update-only frame from the table and the track store (ingvio_update_stage_tracks_nominal): marg_idx [nb] (-1: none);
        track_frames as frame_stage_tracks_nominal_prepare takes them (no append, no observations); tri: None (the store's points) or
        a dict of ingvio_tri_opts fields that differ from tri_opts()'s defaults ({}: the defaults) - the run then triangulates"""
        nb = len(track_frames)
        fa = (TrackFrame * nb)()
        keeps = []
        for i in range(nb):
            d = dict(track_frames[i])
            d.setdefault("clone_idx", []); d.setdefault("clone_R", np.zeros((0, 9))); d.setdefault("clone_p", np.zeros((0, 3)))
            f, k2 = make_track_frame(d)
            fa[i] = f; keeps.append(k2)
        mg = i32(np.asarray(marg_idx, dtype=np.int32).reshape(-1))
        o, chi2 = make_opts(opts_frame, max_accept, compress_rule, selected_variant)
        t = None if tri is None else tri_opts(opts_frame, **tri)

        def call():
            _keep = (keeps, chi2, mg, t)
            return self._chk(self.L.ingvio_update_stage_tracks_nominal(self.h, int(b0), nb, _i(mg), fa, C.byref(o), None if t is None else C.byref(t),
                                                                       1 if use_async else 0))
        return call

    def frame_fetch_tri(self, b0=0, nb=None):
        """(pf [nb, f_max, 3], tri_ok [nb, f_max]) of the update-only frame's triangulation (ingvio_frame_fetch_tri)"""
        nb = self.batch if nb is None else nb
        pf = np.zeros((nb, self.f_max, 3)); ok = np.zeros((nb, self.f_max), dtype=np.int32)
        self._chk(self.L.ingvio_frame_fetch_tri(self.h, int(b0), nb, _d(pf), _i(ok)))
        return pf, ok

    def frame_stage_prepare(self, b0, steps, frames, sigma, enable_gnss=0, sigma_cb=0.0, sigma_rw=0.0, max_accept=0,
                            compress_rule=1, selected_variant=0, use_async=False):
        """Builds the C argument arrays once and returns a callable that re-issues ingvio_frame_stage on them (for timing
        the host hand-over without the Python marshalling)."""
        nb = len(steps)
        sa = (FrameStep * nb)(); fa = (MsckfFrame * nb)()
        keeps = []
        for i in range(nb):
            s, k1 = make_step(steps[i]); f, k2 = make_frame(frames[i])
            sa[i] = s; fa[i] = f; keeps.append((k1, k2))
        o, chi2 = make_opts(frames[0], max_accept, compress_rule, selected_variant)
        sg = f64(sigma)

        fn = self.L.ingvio_frame_stage_async if use_async else self.L.ingvio_frame_stage

        def call(_keep=(keeps, chi2, sa, fa, o, sg)):
            self._chk(fn(self.h, b0, nb, sa, fa, C.byref(o), _d(sg), int(enable_gnss), C.c_double(sigma_cb), C.c_double(sigma_rw)))
        return call

    def frame_set_imu_noise(self, b0, noise):
        """ingvio_frame_set_imu_noise: noise [nb][6] = (noise_g, noise_a, noise_bg, noise_ba, sigma_cb, sigma_rw) of filters
        [b0, b0 + nb) for the frame currently staged (after frame_stage_prepare(use_async=True): the pending one)"""
        nz = f64(np.asarray(noise, dtype=np.float64).reshape(-1, 6))
        self._chk(self.L.ingvio_frame_set_imu_noise(self.h, int(b0), nz.shape[0], _d(nz)))

    def frame_run(self, restore_prior=False):
        self._chk(self.L.ingvio_frame_run(self.h, 1 if restore_prior else 0))

    def set_frame_parts(self, parts):
        """-1 automatic, 1 off, 2..4: slices of the batch that ingvio_frame_run runs on their own streams (ingvio_set_frame_parts)"""
        self._chk(self.L.ingvio_set_frame_parts(self.h, int(parts)))

    def set_gram_reduced(self, on):
        """True (default): the unsplit frame_run forms [A | b] without the block row / column of the solve's reference clone; False: the
        full form everywhere (ingvio_set_gram_reduced).  Bit-identical results."""
        self._chk(self.L.ingvio_set_gram_reduced(self.h, 1 if on else 0))

    def set_gram_decoupled(self, on):
        """True (default): the reduced Gram stage of the window classes 6 and 11 runs as k_feat_gram3 (wave pairs decoupled, one barrier
        per batch); False: as k_feat_gram2 (ingvio_set_gram_decoupled).  Bit-identical results."""
        self._chk(self.L.ingvio_set_gram_decoupled(self.h, 1 if on else 0))

    def last_gram_form(self):
        """the form the last MSCKF update's Gram stage took: 0 full, 1 reduced k_feat_gram2, 2 reduced k_feat_gram3 (ingvio_last_gram_form)"""
        return int(self.L.ingvio_last_gram_form(self.h))

    def set_apply_resident(self, on):
        """True (default): the fused frame step's write-back runs as k_info_apply_res (P[:, window] resident in LDS, one workgroup per filter) for
        more than 64 filters of the window classes 6 and 11 at ldp <= 256; False: k_info_apply (ingvio_set_apply_resident).
        Bit-identical results."""
        self._chk(self.L.ingvio_set_apply_resident(self.h, 1 if on else 0))

    def last_apply_form(self):
        """the form the last MSCKF update's write-back took: 1 k_info_apply_res, 0 any other kernel (ingvio_last_apply_form)"""
        return int(self.L.ingvio_last_apply_form(self.h))

    def last_update_form(self):
        """route and variants of the last generic update as the bit-field of ingvio_last_update_form (UPDATE_* / update_form())"""
        return int(self.L.ingvio_last_update_form(self.h))

    def set_delayed_form(self, mode):
        """0 (default): delayed initialisation in its LDS form only; 1: the large form for candidates the LDS form cannot take (windows
        up to 36 clones); 2, a test setting: the large form for every candidate (ingvio_set_delayed_form)."""
        self._chk(self.L.ingvio_set_delayed_form(self.h, int(mode)))

    def frame_fetch(self, b0=0, nb=None):
        nb = self.batch if nb is None else nb
        dx = np.zeros((nb, self.ldp)); acc = np.zeros((nb, self.f_max), dtype=np.int32); rows = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.ingvio_frame_fetch(self.h, b0, nb, _d(dx), _i(acc), _i(rows)))
        return dx, acc, rows

    def frame_fetch_begin(self, b0=0, nb=None):
        """enqueues the result copies behind the frame's kernels (ingvio_frame_fetch_begin); frame_fetch_end() returns them"""
        nb = self.batch if nb is None else nb
        self._fetch_nb = nb
        self._chk(self.L.ingvio_frame_fetch_begin(self.h, b0, nb))

    def frame_fetch_end(self):
        nb = self._fetch_nb
        dx = np.empty((nb, self.ldp)); acc = np.empty((nb, self.f_max), dtype=np.int32); rows = np.empty(nb, dtype=np.int32)
        self._chk(self.L.ingvio_frame_fetch_end(self.h, _d(dx), _i(acc), _i(rows)))
        return dx, acc, rows

    # ---- triangulation (f-1) ------------------------------------------------------------------
    def triangulate(self, b0, frames, stereo=True, mask_failed=False, **params):
        """frames: list of frame dicts (clone_R, clone_p, obs_mask, uv, R_cl2cr, t_cl2cr; pf/anchor/dof unused), or None
        for the staged frames.  Returns (pf[nb, f_max, 3], ok[nb, f_max])."""
        pr = dict(trans_thres=0.1, huber_epsilon=0.01, conv_precision=5e-7, init_damping=1e-3, outer_loop_max_iter=10,
                  inner_loop_max_iter=10, max_depth=60.0, min_depth=0.2)
        pr.update(params)
        o = TriOpts()
        o.stereo = 1 if stereo else 0
        ref = frames[0] if frames else None
        Rl = f64(ref["R_cl2cr"]).reshape(-1) if ref is not None else np.eye(3).reshape(-1)
        tl = f64(ref["t_cl2cr"]) if ref is not None else np.zeros(3)
        if "R_cl2cr" in params:
            Rl = f64(pr.pop("R_cl2cr")).reshape(-1)
        if "t_cl2cr" in params:
            tl = f64(pr.pop("t_cl2cr"))
        for i in range(9):
            o.R_cl2cr[i] = float(Rl[i])
        for i in range(3):
            o.t_cl2cr[i] = float(tl[i])
        for k, v in pr.items():
            setattr(o, k, v)
        o.mask_failed = 1 if mask_failed else 0
        if frames is None:
            nb = self.batch - b0
            fa = None
            keeps = []
        else:
            nb = len(frames)
            fa = (MsckfFrame * nb)(); keeps = []
            for i in range(nb):
                f, k = make_frame(frames[i]); fa[i] = f; keeps.append(k)
        pf = np.zeros((nb, self.f_max, 3)); ok = np.zeros((nb, self.f_max), dtype=np.int32)
        self._chk(self.L.ingvio_triangulate(self.h, b0, nb, fa, C.byref(o), _d(pf), _i(ok)))
        return pf, ok

    # ---- profiling ---------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self.L.ingvio_profile_enable(self.h, 1 if on else 0))

    def profile_select(self, name=None):
        self._chk(self.L.ingvio_profile_select(self.h, name.encode() if name else None))

    def profile_reset(self):
        self._chk(self.L.ingvio_profile_reset(self.h))

    def profile_get(self):
        cap = 32
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); calls = (C.c_int * cap)()
        k = self.L.ingvio_profile_get(self.h, names, ms, calls, cap)
        return {names[i].decode(): (ms[i], calls[i]) for i in range(k)}


class TriOpts(C.Structure):
    _fields_ = [("stereo", C.c_int), ("R_cl2cr", C.c_double * 9), ("t_cl2cr", C.c_double * 3),
                ("trans_thres", C.c_double), ("huber_epsilon", C.c_double), ("conv_precision", C.c_double),
                ("init_damping", C.c_double), ("outer_loop_max_iter", C.c_int), ("inner_loop_max_iter", C.c_int),
                ("max_depth", C.c_double), ("min_depth", C.c_double), ("mask_failed", C.c_int)]


def tri_opts(opts_frame, stereo=None, **params):
    """ingvio_tri_opts with the reference's defaults (Triangulator.h:67-75), the outer calibration and (stereo=None) the camera
    model of opts_frame; params: the fields that differ"""
    pr = dict(trans_thres=0.1, huber_epsilon=0.01, conv_precision=5e-7, init_damping=1e-3, outer_loop_max_iter=10,
              inner_loop_max_iter=10, max_depth=60.0, min_depth=0.2)
    pr.update(params)
    t = TriOpts()
    t.stereo = int(opts_frame.get("stereo", 1)) if stereo is None else (1 if stereo else 0)
    t.R_cl2cr = (C.c_double * 9)(*np.asarray(opts_frame["R_cl2cr"], dtype=np.float64).reshape(9))
    t.t_cl2cr = (C.c_double * 3)(*np.asarray(opts_frame["t_cl2cr"], dtype=np.float64).reshape(3))
    for k, v in pr.items():
        setattr(t, k, v)
    return t


class DeviceCov:
    """Single-filter covariance engine with the same surface as oracle.Cov, backed by filter `b`
    of a Context (so ingvio_amd.synth can build scenarios on the GPU)."""

    def __init__(self, ctx, b, P):
        self.ctx, self.b = ctx, b
        ctx.cov_set(b, P)

    @property
    def n(self):
        return self.ctx.n(self.b)

    @property
    def P(self):
        return np.array(self.ctx.cov_get(self.b))

    def propagate(self, Phi, G, dt, sigma, enable_gnss=0, gnss_idx=(-1,) * 5, sigma_cb=0.0, sigma_rw=0.0):
        self.ctx.propagate(self.b, Phi, G, dt, sigma, enable_gnss, gnss_idx if enable_gnss else None, sigma_cb, sigma_rw)

    def augment(self, R_i2w):
        return int(self.ctx.augment(self.b, R_i2w)[0])

    def marginalize(self, idx, size):
        self.ctx.marginalize(self.b, [idx], size)

    def append_independent(self, blk):
        return int(self.ctx.append_independent(self.b, np.atleast_2d(blk))[0])
