#!/usr/bin/env python3
"""bench.py — EKF updates/s on synthetic stereo MSCKF frames (BASELINE.json metric).

One *step* = one pass of the hot path over one batch: every filter of the batch does
k=10-step covariance propagation (K1) + clone augmentation (K2) + F-feature MSCKF update
(Jacobians K3, nullspace K4, chi^2 gate K5, stacked compression K6/K7, Kalman update K8-K11) +
marginalisation of the oldest clone (K12) — SURVEY.md §8(d) "one update".  Inputs (IMU transitions,
clone poses, feature tracks, the prior covariances) are resident in HBM before the timed region;
each step restores the same prior device-to-device so the work per step is stationary.

Workloads (`--config`, BASELINE.json `configs`):
  2  (default, the one `metric` is quoted on)  150 feats x 11 clones, `--state nominal` N = 249 (6 GNSS scalars + 52 landmark
     blocks), `literal` N = 87, `gnss` N = 93; `--batch` independent filters per GPU (default 512 = configs[3]'s 4096 / 8 GPUs)
  3  config 2 + GnssUpdate::updateTrackedSys with 8 satellites (16 candidate rows), per-row chi^2 gates on, after the frame
  5  stress: 300 feats x 30 clones, N = 207 (`literal`/`gnss`) or 807 (`nominal`: + 200 landmark blocks), default batch 32
N > 1: weak scaling, each rank owns its own `--batch` filters, no data-path collective; RCCL only for the
timing barrier / max and one end-of-run gather of per-rank summaries.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run measures the headline alone: build the batch, warm up (+ the untimed conditioning steps), time `--steps` steps, print
the line.  `--full` adds everything else: the per-kernel table and roofline, the CPU baseline and the oracle cross-checks, the
as-written and host hand-over figures, configs 3 and 5 on the same clock (`aux_configs`), the single-filter latency streams and
the detail file.  `--dump-outputs DIR` writes what the last timed step computed (rank 0) as DIR/<name>.npy.

Roofline: `roofline.achieved` of the dominant kernel = EXECUTED FP64 operations per launch (rocprofv3 SQ counters committed
under profiles/, read from profiles/counters.json — bench.py cannot collect PMC itself) / the kernel's HIP-event time
measured live inside the timed region; <= peak by construction.  The ALGORITHMIC rate (SURVEY §8(d)'s dense formulation of
the reference / the same time) is reported next to it as `algorithmic`: the factored kernels execute about a quarter of
those operations, so that figure can exceed the peak and is not a fraction of anything.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6      # MI355X FP64 vector == FP64 MFMA peak (datasheet; issue rates: tools/micro/issue_rates.hip)
HBM_PEAK_GBS = 8000.0
COUNTERS_JSON = os.path.join(ROOT, "profiles", "counters.json")
DETAIL_JSON = os.path.join(ROOT, "bench_detail.json")


class LazyCov:
    """Index bookkeeping + deferred covariance ops so that `synth.Filter` can drive B filters in
    lockstep and the arithmetic is done by ONE batched C-ABI call per stage.  While `host_init`
    is set, append_independent assembles the block-diagonal prior on the host (data assembly only)."""

    def __init__(self, P):
        self.M = np.array(P, dtype=np.float64)
        self.n = self.M.shape[0]
        self.host_init = True
        self.pending_steps = None
        self.pending_R = None

    def append_independent(self, blk):
        assert self.host_init
        n, s = self.n, blk.shape[0]
        M = np.zeros((n + s, n + s)); M[:n, :n] = self.M; M[n:, n:] = blk
        self.M = M; self.n = n + s
        return n

    def propagate(self, Phi, G, dt, *a, **k):
        self.pending_steps.append((Phi, G, dt))

    def augment(self, R):
        self.pending_R = np.array(R)
        self.n += 6
        return self.n - 6


def build_batch(ctx, B, seed0, F, C, n_gnss, n_landmarks, lm_sigma=1.0, stereo=True):
    """Creates B config-2 style cases; priors are produced by the HIP path itself (batched propagate+clone)."""
    from ingvio_amd import host, synth
    pr = synth.PARAMS
    filters, rngs = [], []
    for b in range(B):
        rng = np.random.default_rng(0x1A6F10 + seed0 + b)
        flt = synth.Filter(LazyCov, host.imu_transition, t0=0.1 * ((seed0 + b) % 997), n_gnss=n_gnss, n_landmarks=n_landmarks,
                           lm_sigma=lm_sigma)
        flt.cov.host_init = False
        ctx.cov_set(b, flt.cov.M)
        filters.append(flt); rngs.append(rng)
    sigma = filters[0].sigma()
    for cyc in range(C - 1):
        Phi = np.zeros((B, synth.IMU_PER_FRAME, 15, 15)); G = np.zeros((B, synth.IMU_PER_FRAME, 15, 12))
        dt = np.zeros((B, synth.IMU_PER_FRAME)); R = np.zeros((B, 3, 3)); gi = np.zeros((B, 5), dtype=np.int32)
        for b, flt in enumerate(filters):
            flt.cov.pending_steps = []
            flt.propagate_cov(flt.imu_steps(rngs[b]))
            for s, (p, g, d) in enumerate(flt.cov.pending_steps):
                Phi[b, s], G[b, s], dt[b, s] = p, g, d
            flt.clone()
            R[b] = flt.cov.pending_R
            gi[b] = flt.gnss_idx
        ctx.propagate(0, Phi, G, dt, sigma, filters[0].enable_gnss, gi if filters[0].enable_gnss else None,
                      pr["sigma_cb"], pr["sigma_rw"], fused=True)
        idx = ctx.augment(0, R)
        assert all(int(idx[b]) == filters[b].cov.n - 6 for b in range(B))
    steps, frames, infos = [], [], []
    table = synth.chi2_table()
    Rlr, tlr = synth.t_cl2cr()
    for b, flt in enumerate(filters):
        rng = rngs[b]
        flt.cov.pending_steps = []
        st = flt.imu_steps(rng)
        t_new = flt.t
        clone_times = [c["t"] for c in flt.clones] + [t_new]
        step = flt.step_dict(st, marg_name=flt.clones[0]["name"])
        new_idx = flt.cov.n
        pf, uv, outlier = synth.make_features(rng, clone_times, F, stereo=stereo)
        clones = flt.clones + [dict(R=flt.R @ synth.R_CL2I, p=flt.p + flt.R @ synth.T_CL2I)]
        frames.append(dict(
            clone_idx=np.array([flt.idx_of(c["name"]) for c in flt.clones] + [new_idx], dtype=np.int32),
            clone_R=np.stack([c["R"] for c in clones]), clone_p=np.stack([c["p"] for c in clones]), pf=pf,
            anchor=np.zeros(F, dtype=np.int32), obs_mask=np.full(F, (1 << C) - 1, dtype=np.uint64), uv=uv,
            dof=np.full(F, C - 1, dtype=np.int32), stereo=1 if stereo else 0, R_cl2cr=Rlr, t_cl2cr=tlr, noise=pr["visual_noise"],
            chi2_table=table))
        steps.append(step)
        infos.append(dict(outlier=outlier, n_prior=flt.cov.n, rng=rng))
    return filters, steps, frames, infos


def algorithmic_flops(F_used, F, C, N, k):
    """SURVEY.md §8(d) formula block (the reference's dense formulation), per update, split by the kernel that carries the term."""
    n = 6 * C; rho = 4 * C - 3; m = F_used * rho
    k4 = 12.0 * (4 * C) * (n + 1)
    k5 = 2.0 * rho * n * n + 2.0 * rho * rho * n + rho ** 3 / 3.0 + 2.0 * rho * rho
    k7 = 2.0 * m * n * n - (2.0 / 3.0) * n ** 3 + 4.0 * m * n
    k8_9_11 = 2.0 * N * n * n + 2.0 * n ** 3 + n ** 3 / 3.0 + 2.0 * N * n * n + 2.0 * N * n
    k10 = 2.0 * N * N * n
    k1 = k * (2.0 * 15 * 15 * (N - 15) + 4.0 * 15 ** 3)
    k2 = 2.0 * 6 * 21 * N
    per_kernel = {
        "k_propagate": k1 + k2, "k_msckf_gate": F * (k4 + k5), "k_msckf_fold": F_used * k4 + k7,
        "k_ekf_core": k8_9_11, "k_downdate": k10,
        # factored path: same algorithmic work, carried by other kernels (K8/K9 -> k_info_update; K10/K11 and the
        # P H^T / K products -> k_info_apply)
        "gate": F * (k4 + k5), "gram": F_used * k4 + k7, "solve": 2.0 * n ** 3 + n ** 3 / 3.0,
        "apply": k10 + 4.0 * N * n * n + 2.0 * N * n}
    total = F * (k4 + k5) + k7 + k8_9_11 + k10 + k1 + k2
    return per_kernel, total


def algorithmic_bytes(N, k_imu, F, C):
    """bytes a kernel must move at least once per update (FP64).  Only kernels whose traffic has such a
    closed form are listed: the strip kernels and the update's read+write of P."""
    return {"k_propagate": 2.0 * 2 * (15 + 6) * N * 8 + 8.0 * k_imu * 405,      # 15-column strip + the 6 new clone rows, both ways
            "apply": 2.0 * N * N * 8,                                   # read + write P once
            "k_marginalize": 2.0 * N * N * 8, "restore_full": 2.0 * N * N * 8}


# ---- counters committed under profiles/ --------------------------------------------------------------------------------
def load_counters(path, key):
    """profiles/counters.json: {workloads: {key: {source, kernels: {name: {counter: per-launch average}}}}} written by
    tools/pmc_summary.py from rocprofv3 --pmc passes.  Returns (kernels dict or None, source note)."""
    try:
        with open(path) as f:
            J = json.load(f)
    except (OSError, ValueError):
        return None, "no %s" % os.path.relpath(path, ROOT), None
    w = J.get("workloads", {}).get(key)
    if w is None:
        return None, "%s holds no workload %r" % (os.path.relpath(path, ROOT), key), None
    return w.get("kernels", {}), "%s[%s]" % (os.path.relpath(path, ROOT), key), w.get("build")


def stale_kernels(kernel_names, recorded_tu, live_build):
    """Kernels of `kernel_names` whose committed counters do NOT belong to the running library: the workload's counters were
    folded (tools/pmc_summary.py) with the per-translation-unit hashes of the library that produced them; a kernel is current
    when the hash of ITS translation unit (text + included headers + flags, ingvio_build_id()) is the one recorded.  Counters
    without a record (collected before round 4) are stale by definition."""
    out = []
    for k in kernel_names:
        tu = (live_build or {}).get("kernels", {}).get(k)
        if recorded_tu is None or tu is None or recorded_tu.get(tu) != live_build["tu"].get(tu):
            out.append(k)
    return out


def executed_fp64_flops(c):
    """FP64 operations one launch EXECUTES, from the SQ counters (wave-level instruction counts x 64 lanes; an FMA is two
    operations; SQ_INSTS_VALU_MFMA_MOPS_F64 counts MFMA operations in units of 512 — rocprofiler-sdk counter_defs.yaml,
    TOTAL_64_OPS).  Lanes masked off by EXEC are included: this is what the FP64 pipe is occupied with, an upper bound of
    the useful arithmetic."""
    need = ("SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MFMA_MOPS_F64")
    if c is None or any(k not in c for k in need):
        return None
    valu = 64.0 * (c["SQ_INSTS_VALU_ADD_F64"] + c["SQ_INSTS_VALU_MUL_F64"] + c.get("SQ_INSTS_VALU_TRANS_F64", 0.0)
                   + 2.0 * c["SQ_INSTS_VALU_FMA_F64"])
    mfma = 512.0 * c["SQ_INSTS_VALU_MFMA_MOPS_F64"]
    out = dict(total=valu + mfma, valu=valu, mfma=mfma)
    # lane utilisation of the VALU stream (rocprofiler's derived metric VALUUtilization = SQ_THREAD_CYCLES_VALU /
    # (SQ_ACTIVE_INST_VALU x wave size)): the share of the 64 lanes that are enabled, averaged over the VALU instructions' cycles.
    # `useful` discounts the VALU part of the executed operations by it (the counter covers every VALU instruction, not the FP64
    # ones alone - an approximation, stated as such); matrix-core operations are not lane-masked.
    if c.get("SQ_THREAD_CYCLES_VALU") and c.get("SQ_ACTIVE_INST_VALU"):
        lu = c["SQ_THREAD_CYCLES_VALU"] / (64.0 * c["SQ_ACTIVE_INST_VALU"])
        out["lane_utilisation"] = lu
        out["useful"] = valu * min(lu, 1.0) + mfma
    return out


def hbm_traffic_bytes(c):
    """HBM bytes per launch from the PMC passes, corrected as MI355X_MICROARCH.md prescribes: FETCH_SIZE (KiB) reports half of
    the bytes of wide coalesced reads on gfx950 -> x2; WRITE_SIZE (KiB) as is (both calibrated on the pure-copy restore kernel,
    profiles/README.md)."""
    if c is None or "FETCH_SIZE" not in c or "WRITE_SIZE" not in c:
        return None
    return dict(read=2.0 * 1024.0 * c["FETCH_SIZE"], written=1024.0 * c["WRITE_SIZE"],
                total=2.0 * 1024.0 * c["FETCH_SIZE"] + 1024.0 * c["WRITE_SIZE"])


# The library's profile slots are named after the STAGE; rocprofv3 sees kernels.  Stage -> candidates, each candidate a tuple of
# kernels whose counters are added up (x their launches per step): the first candidate with counters for all its kernels wins.
STAGE_KERNELS = {
    "gate": (("k_feat_gate5",), ("k_feat_gate4",), ("k_feat_gate5m",), ("k_feat_gate3",)),      # stereo: four features per wave (round 4, windows <= 11 clones) / one per wave (round 3); mono: four per wave (round 6, 7..11 clones) / first generation
    "gram": (("k_feat_gram2",),),
    "solve": (("k_info_solve",), ("k_info_update",)),            # windows up to 12 clones / 13..16
    "apply": (("k_info_apply",),),
    "restore": (("k_restore_strips",), ("k_restore",)),
    "k_lm_build": (("k_lm_rows", "k_lm_front"), ("k_lm_build", "k_lm_products")),        # fused front (round 3) / compacting build + products
    "k_lm_gemm": (("k_gemm",),),
    "k_lm_chol": (("k_lm_factor", "k_lm_carry"), ("k_chol_first", "k_chol_step", "k_chol_carried", "k_lm_finish")),      # register-resident solve (round 3) / sweep out of L2
    "k_downdate": (("k_downdate64",), ("k_downdate",)),
}
STAGE_KERNELS_BIG = {                                                      # windows of 17..36 clones (kernels_bigwin.hip)
    "gate": (("k_feat_gate4_big",), ("k_feat_gate3_big",)), "gram": (("k_feat_gram_big",),),
    # round 5: the set-up is k_big_prep_P (prior only, on the side stream together with the first sweep) + k_big_prep_A
    "solve": (("k_big_prep_P", "k_big_prep_A", "k_chol_first", "k_chol_step", "k_chol_carried", "k_gemm64", "k_big_gauge_fix"),
                      ("k_big_prep_P", "k_big_prep_A", "k_chol_first", "k_chol_step", "k_chol_carried", "k_gemm64"), ("k_info_update_big",)),
    "apply": (("k_apply_T64b", "k_apply_sym64b"), ("k_apply_T", "k_apply_sym"), ("k_info_apply_big",)),
}


def mono_gate_kernel_of(C):
    """The mono gate kernel launch_factored / launch_bigwin pick: four features per wave for the 11-clone class (round 6, gate5m_kernel.h),
    the first-generation gate elsewhere (and with INGVIO_GATE=3)."""
    if C > 16:
        return "k_feat_gate3_big"
    return "k_feat_gate5m" if (6 < C <= 11 and os.environ.get("INGVIO_GATE", "")[:1] != "3") else "k_feat_gate3"


def gate_kernel_of(C):
    """The stereo gate kernel launch_factored / launch_bigwin pick for a window of C clones (INGVIO_GATE selects the older ones)."""
    g = os.environ.get("INGVIO_GATE", "")[:1]
    if C > 16:
        return "k_feat_gate3_big" if g == "3" else "k_feat_gate4_big"
    if g == "3":
        return "k_feat_gate3"
    return "k_feat_gate4" if (g == "4" or C > 11) else "k_feat_gate5"


def counters_for(counters, name, big, C=None, stereo=True):
    """-> (summed counters of the stage's kernels or None, the kernels they belong to)."""
    table = STAGE_KERNELS_BIG if big and name in STAGE_KERNELS_BIG else STAGE_KERNELS
    cands = table.get(name, ((name,),))
    if name == "gate" and C is not None:            # the gate that ran is known: counters of another generation do not apply
        cands = ((gate_kernel_of(C) if stereo else mono_gate_kernel_of(C),),)
    if counters is None:
        return None, cands[0]
    for cand in cands:
        if all(k in counters for k in cand):
            out = {}
            for k in cand:
                mult = counters[k].get("_launches_per_step", 1)
                for c, v in counters[k].items():
                    if not c.startswith("_"):
                        out[c] = out.get(c, 0.0) + v * mult
            return out, cand
    return None, cands[0]


def kernel_that_ran(stage, cand, C, stereo=True):
    """The kernel rocprofv3 sees for a profile slot (slots are named after the stage)."""
    name = "+".join(cand)
    if stage == "gate":
        if not stereo and cand[0] != "k_feat_gate5m":
            return "k_feat_gate3%s<%d>" % ("_big" if C > 16 else "", C)
        cls = 6 if C <= 6 else 11 if C <= 11 else 12 if C <= 12 else 16 if C <= 16 else 24 if C <= 24 else 28 if C <= 28 else 30 if C <= 30 else 32 if C <= 32 else 36      # launch_factored / launch_bigwin classes
        return "%s<%d>" % (cand[0], cls)
    return name


def price_kernels(prof, dom_name, counters, csrc, rec_build, live_build, C, B, per_kernel, bytes_k, stereo=True):
    """Per-kernel table (time from HIP events, executed operations / HBM bytes from the committed counters - only when they belong
    to the running build of the kernel's translation unit) and the roofline of the dominant kernel.  Pure function of its
    inputs: tests/test_bench_line.py flips a hash and sees frac = None."""
    kernels = {}
    for name, (ms, calls) in prof.items():
        if calls == 0:
            continue
        avg = ms / calls
        c, cand = counters_for(counters, name, C > 16, C, stereo)
        e = dict(avg_ms=avg, calls=calls, kernel=kernel_that_ran(name, cand, C, stereo))
        if c is not None:
            st = stale_kernels(cand, rec_build, live_build)
            if st:                                  # counters of another build of this kernel: no price, say so
                e["counters_stale"] = st
                c = None
        ex = executed_fp64_flops(c)
        if ex is not None:
            e["executed_fp64_flop_per_launch"] = ex["total"]
            e["executed_fp64_mfma_share"] = ex["mfma"] / ex["total"] if ex["total"] else 0.0
            e["executed_tflops"] = ex["total"] / (avg * 1e-3) / 1e12
            e["frac_fp64_peak"] = e["executed_tflops"] / FP64_PEAK_TFLOPS
            if "lane_utilisation" in ex:
                e["valu_lane_utilisation"] = ex["lane_utilisation"]
                e["useful_frac_fp64_peak"] = ex["useful"] / (avg * 1e-3) / 1e12 / FP64_PEAK_TFLOPS
        tr = hbm_traffic_bytes(c)
        if tr is not None:
            e["hbm_bytes_per_launch"] = tr
            e["hbm_gbs"] = tr["total"] / (avg * 1e-3) / 1e9
            e["frac_hbm_peak"] = e["hbm_gbs"] / HBM_PEAK_GBS
        if per_kernel.get(name, 0.0) > 0:
            e["algorithmic_flop_per_launch"] = per_kernel[name] * B
            e["algorithmic_tflops"] = per_kernel[name] * B / (avg * 1e-3) / 1e12
        if name in bytes_k:
            e["algorithmic_bytes_per_launch"] = bytes_k[name] * B
        kernels[name] = e
    roofline = None
    if dom_name is not None and dom_name in kernels:
        k = kernels[dom_name]
        if "executed_tflops" in k:
            mf = k["executed_fp64_mfma_share"]
            roofline = dict(kernel=k["kernel"], stage=dom_name, bound="mfma" if mf > 0.5 else "valu", achieved=k["executed_tflops"], peak=FP64_PEAK_TFLOPS,
                            unit="TFLOP/s", frac=k["frac_fp64_peak"],
                            traffic=k.get("hbm_bytes_per_launch", {}).get("total"), avg_launch_ms=k["avg_ms"],
                            launches_timed=k["calls"], executed_fp64_flop_per_launch=k["executed_fp64_flop_per_launch"],
                            mfma_share_of_executed=mf, lane_utilisation=k.get("valu_lane_utilisation"),
                            useful_frac=k.get("useful_frac_fp64_peak"),
                            algorithmic=dict(tflops=k.get("algorithmic_tflops"), flop_per_launch=k.get("algorithmic_flop_per_launch"),
                                             note="SURVEY 8(d) dense formulation of the reference / the same time; not a "
                                                  "fraction of the peak (the kernel executes fewer operations)"),
                            counters=csrc,
                            note="achieved = EXECUTED FP64 operations per launch (rocprofv3 SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64 x 64 "
                                 "lanes, FMA = 2, + SQ_INSTS_VALU_MFMA_MOPS_F64 x 512) / HIP-event time of the launches inside "
                                 "the timed region; peak: FP64 vector and FP64 MFMA peaks coincide on MI355X (78.6 TFLOP/s), "
                                 "`bound` names the pipe that carries most of the executed operations; traffic = HBM bytes per "
                                 "launch (FETCH_SIZE x 2 + WRITE_SIZE); lane_utilisation = SQ_THREAD_CYCLES_VALU / (64 "
                                 "SQ_ACTIVE_INST_VALU), useful_frac = (VALU operations x lane_utilisation + matrix-core "
                                 "operations) / time / peak: the executed figure counts masked-off lanes, this one does not")
        else:
            roofline = dict(kernel=k["kernel"], stage=dom_name, bound="valu", achieved=None, peak=FP64_PEAK_TFLOPS, unit="TFLOP/s", frac=None,
                            traffic=None, avg_launch_ms=k["avg_ms"], launches_timed=k["calls"],
                            counters_stale=bool(k.get("counters_stale")),
                            algorithmic=dict(tflops=k.get("algorithmic_tflops"), flop_per_launch=k.get("algorithmic_flop_per_launch")),
                            counters=csrc,
                            note=("the committed SQ counters of this kernel were collected on ANOTHER build of its translation "
                                  "unit (%s): not used" % ", ".join(k["counters_stale"])) if k.get("counters_stale") else
                                 "no committed SQ counters for this workload: the executed-operation count, and with it the "
                                 "achieved fraction, is unknown (collect with tools/gpu_counters.sh)")
    return kernels, roofline


def cpu_baseline(ctx, steps, frames, n_prior, ld, quick=False):
    """Times the oracle (C port of the reference algorithm) on a bounded sample of the same workload and cross-checks the GPU
    posterior on that sample.  Protocol: the reference is single-threaded (IngvioNode.cpp:36), so the primary
    figure is ONE thread: 10 warm-up updates, >= 100 timed updates (each on its own frame of the bench batch, cycled), median
    and p95 per update.  Beside it the all-cores figure (one filter per thread, OpenMP) for the batched configuration.
    Only the C call is inside a timed interval (structs are prepared once)."""
    from oracle import oracle as orc
    cores = os.cpu_count() or 1
    S = min(len(steps), cores)
    ctx.restore(); ctx.sync()
    P0 = np.zeros((S, ld, ld))
    for b in range(S):
        P0[b, :n_prior, :n_prior] = ctx.cov_get(b)
    n0 = np.full(S, n_prior, dtype=np.int32)
    # ---- one thread: warm-up 10, timed >= 100, median + p95 ---------------------------------------------------------
    n_warm, n_timed = (2, 10) if quick else (10, 100)
    nsingle = min(S, 16)
    singles = [orc.PreparedBatch(steps[i:i + 1], frames[i:i + 1], max_accept=0, compress_rule=1) for i in range(nsingle)]
    samples = []
    for it in range(n_warm + n_timed):
        i = it % nsingle
        Pw, nw = P0[i:i + 1].copy(), n0[i:i + 1].copy()
        t0 = time.perf_counter()
        singles[i].run(Pw, nw, ld, threads=1)
        dt = time.perf_counter() - t0
        if it >= n_warm:
            samples.append(dt)
        if len(samples) >= 10 and sum(samples) > (12.0 if not quick else 2.0):
            break                                                 # config 5 (0.5 s per update): bounded sample, reported as such
    samples = np.array(samples)
    one = dict(ms_median=float(np.median(samples) * 1e3), ms_p95=float(np.percentile(samples, 95) * 1e3),
               ms_mean=float(samples.mean() * 1e3), timed=int(len(samples)), warmup=n_warm,
               updates_per_s=float(1.0 / np.median(samples)))
    # ---- all cores, one filter per thread.  The container may be CPU-throttled (cgroup quota) well below os.cpu_count():
    #      more threads than the quota makes the baseline SLOWER, so probe a few counts and keep the best (reported as `cores`)
    prep = orc.PreparedBatch(steps[:S], frames[:S], max_accept=0, compress_rule=1)

    def rate(th, min_s, max_rounds=500):
        prep.run(P0.copy(), n0.copy(), ld, threads=th)
        times, last, Pw, nw = [], None, None, None
        while (sum(times) < min_s and len(times) < max_rounds) or len(times) < 2:
            Pw, nw = P0.copy(), n0.copy()
            t0 = time.perf_counter()
            last = prep.run(Pw, nw, ld, threads=th)
            times.append(time.perf_counter() - t0)
        return S / float(np.median(times)), times, (Pw, nw) + tuple(last)
    probes = {}
    for th in sorted({cores, min(cores, 64), min(cores, 32), min(cores, 16), min(cores, 8)}, reverse=True):
        probes[th] = rate(th, 0.8 if not quick else 0.2, 20)[0]
    best = max(probes, key=probes.get)
    val, times, (P1, n1, dx1, acc1) = rate(best, 6.0 if not quick else 0.5)
    # the reference AS WRITTEN (quirks Q2/Q3: accepted-feature cap 20, RemoveLost keeps all rows after SPQR, so S is
    # 820 x 820): one thread
    s2 = min(S, 2)
    prep2 = orc.PreparedBatch(steps[:s2], frames[:s2], max_accept=20, compress_rule=0)
    aw = []
    for it in range(1 + (3 if not quick else 1)):
        Pb, nb_ = P0[:s2].copy(), n0[:s2].copy()
        t2 = time.perf_counter()
        prep2.run(Pb, nb_, ld, threads=1)
        if it:
            aw.append((time.perf_counter() - t2) / s2)
    return dict(value=val, unit="updates/s", cores=best, kind="port",
                sample="oracle/ingvio_oracle.c on the bench's own frames (top_n compression, no accepted-feature cap): `value` = one "
                       "filter per thread on %d OpenMP threads, median of %d rounds x %d frames (best of the probed thread counts %s "
                       "on a host reporting %d CPUs); `one_thread` = the reference's execution model: %d warm-up + %d timed "
                       "single-filter updates" % (best, len(times), S, {k: round(v) for k, v in sorted(probes.items())}, cores,
                                                  n_warm, len(samples)),
                one_thread=one, as_written_cap20_ms_per_update_1thread=float(np.median(aw) * 1e3)), (P1, n1, dx1, acc1, S)



def oracle_parity_sample(ctx, one_step, steps, frames, gnss, n_prior, ld, N, F, S):
    """In-run cross-check of one step against the oracle on S filters spread over the batch (the first, the last, evenly in
    between): covariance, accept masks and dx after propagate + clone + MSCKF update + marginalise (+ the gated GNSS update of
    config 3, rows as the reference stacks them: oracle gnss_rows with chi2_test, then ekfUpdate)."""
    from oracle import oracle as orc
    B = len(steps)
    sample = sorted(set(int(round(x)) for x in np.linspace(0, B - 1, S)))
    ctx.restore(); ctx.sync()
    priors = {b: ctx.cov_get(b) for b in sample}
    one_step()
    dxg, accg, rowsg = ctx.frame_fetch()
    errs, dxe, mask_ok = [], [], True
    for b in sample:
        oc = orc.Cov(priors[b], ld=ld)
        dxo, acco, gamo, m = orc.frame_update(oc, steps[b], frames[b], max_accept=0, compress_rule=1)
        mask_ok = mask_ok and bool(np.array_equal(accg[b, :F], acco))
        if gnss is None:                                           # with GNSS the frame's dx slot is not the last update's
            dxe.append(float(np.linalg.norm(dxg[b, :N] - dxo) / max(np.linalg.norm(dxo), 1e-300)))
        else:
            go = dict(gnss[b]); go.update(chi2_test=1, chi2_table=frames[b]["chi2_table"])
            Ho, ro, Rdo, vio, vso = orc.gnss_rows(oc, go)
            if len(ro):
                oc.ekf_update(vio, vso, Ho, ro, Rdo)
        Pg = ctx.cov_get(b)
        errs.append(float(np.linalg.norm(Pg - oc.P) / np.linalg.norm(oc.P)))
    return dict(sample=len(sample), filters=sample, max_rel_cov_err=max(errs), accept_mask_equal=mask_ok,
                max_rel_dx_err=max(dxe) if dxe else None)


DUMP_LIMIT = 64 << 20                    # --dump-outputs: bytes in all
DUMP_COV_FILTERS = 64                    # posterior covariances dumped: at most this many filters, a fixed seeded sample of the batch
DUMP_SEED = 0x1A6F10


def dump_outputs(out_dir, ctx, B, arrays):
    """--dump-outputs: the results of the last timed step as float64 .npy files (integers are exact in float64).  The posterior
    covariances (B x n x n: 254 MB at the default workload) are a fixed sample of the batch, `cov_filters` names which."""
    os.makedirs(out_dir, exist_ok=True)
    out = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    n = ctx.n(0)
    room = DUMP_LIMIT - sum(a.nbytes for a in out.values()) - (1 << 20)
    S = max(1, min(B, DUMP_COV_FILTERS, room // (8 * n * n + 8)))
    sample = np.sort(np.random.default_rng(DUMP_SEED).choice(B, S, replace=False))
    covs = [ctx.cov_get(int(b)) for b in sample]
    assert all(P.shape == (n, n) for P in covs), "filters of one batch share their state size"
    out["cov_filters"] = sample.astype(np.float64)
    out["cov"] = np.ascontiguousarray(np.stack(covs), dtype=np.float64)
    total = sum(a.nbytes for a in out.values())
    assert total <= DUMP_LIMIT, "dump of %d bytes > %d" % (total, DUMP_LIMIT)
    for k, a in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 5], help="workload, numbered as in the docstring (= BASELINE.json configs[] position, 1-based)")
    ap.add_argument("--batch", type=int, default=None, help="independent filters per GPU (default 512; config 5: 32)")
    ap.add_argument("--feats", type=int, default=None)
    ap.add_argument("--clones", type=int, default=None)
    ap.add_argument("--state", default="nominal", choices=["nominal", "literal", "gnss"],
                    help="nominal: + 6 GNSS scalars + landmark padding (N = 249 / 807); literal: clones only (N = 87 / 201); gnss: + 6 GNSS scalars")
    ap.add_argument("--literal", action="store_true", help="same as --state literal")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--quick-cpu", action="store_true", help="short CPU baseline (smoke runs)")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket kernels with HIP events")
    ap.add_argument("--no-condition", action="store_true", help="no untimed device-conditioning steps in front of the timed region (see run_workload)")
    ap.add_argument("--method", default="factored", choices=["factored", "dense"])
    ap.add_argument("--counters", default=COUNTERS_JSON)
    ap.add_argument("--landmarks", default="padded", choices=["padded", "real"],
                    help="nominal state: the 3-column landmark blocks are padding (default) or REAL in-state SLAM landmarks that "
                         "receive rows every frame (LandmarkUpdate.cpp:32-149, batched on the device between the MSCKF update and "
                         "the marginalisation)")
    ap.add_argument("--gnss-separate", action="store_true", help="config 3: the GNSS update as its own pass over P after the frame (round 3) "
                    "instead of in-frame on the MSCKF write-back")
    ap.add_argument("--mono", action="store_true", help="the MONO form of the workload (BASELINE configs[0]: RemoveLostUpdate.cpp:169-273, two rows per "
                    "observation, rho = 2C - 3 rows per feature); auxiliary workload, never the default line")
    ap.add_argument("--no-aux", action="store_true", help="skip the auxiliary config-3 / config-5 passes of the default run")
    ap.add_argument("--no-latency", action="store_true", help="skip the single-filter latency figures (C++ shim stream) of the default run")
    ap.add_argument("--detail", default=DETAIL_JSON, help="where the full result (per-kernel tables, notes) is written (--full)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: per-kernel table and roofline, CPU baseline, oracle "
                    "cross-checks, as-written and host hand-over figures, aux configs 3 / 5, latency streams, the detail file")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0: dx, accept masks, row counts, a fixed "
                         "sample of posterior covariances, GNSS / landmark results where the workload has them) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.literal:
        args.state = "literal"
    return args


def run_workload(args, grp, aux=False):
    """One workload: build the batch, warm up, time `--steps` steps, assemble the result dict (rank 0; None elsewhere)."""

    from ingvio_amd import capi, host, synth
    rank, world, local_rank = grp.rank, grp.world, grp.local_rank
    big = args.config == 5
    B = args.batch if args.batch else (32 if big else 512)
    F = args.feats if args.feats else (300 if big else 150)
    C = args.clones if args.clones else (30 if big else 11)
    if args.config == 3 and args.state == "literal":
        args.state = "gnss"                                    # the GNSS update needs the clock / YOF scalars in the state
    n_gnss = 0 if args.state == "literal" else 6
    n_lm = 0 if args.state != "nominal" else (200 if big else 52)
    N = 21 + n_gnss + 3 * n_lm + 6 * C
    ctx = capi.Context(batch=B, n_max=((N + 15) // 16) * 16, c_max=C, f_max=F, m_max=64, device=grp.device_index)
    ctx.set_method(args.method)
    ld = ctx.ldp
    t_build = time.perf_counter()
    real_lm = args.landmarks == "real" and n_lm > 0
    n_lm_real = min(n_lm, capi.LM_MAX) if real_lm else 0
    stereo = not getattr(args, "mono", False)
    filters, steps, frames, infos = build_batch(ctx, B, rank * B, F, C, n_gnss, n_lm, lm_sigma=0.05 if real_lm else 1.0, stereo=stereo)
    ctx.snapshot()
    pr = synth.PARAMS
    ctx.frame_stage(0, steps, frames, filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"],
                    max_accept=0, compress_rule=1)
    if real_lm:
        lms = [synth.make_landmarks(infos[b]["rng"], filters[b], frames[b], n_lm_real) for b in range(B)]
        Rlr, tlr = synth.t_cl2cr()
        ctx.landmark_stage(0, lms, True, pr["visual_noise"], 9.487729036781154, Rlr, tlr, in_frame=True)
    gnss = None
    if args.config == 3:
        gnss = [synth.make_gnss(infos[b]["rng"], filters[b]) for b in range(B)]
        # in-frame: ingvio_frame_run applies the GNSS update on the MSCKF write-back (one sweep over P); --gnss-separate: its own pass
        ctx.gnss_stage(0, [host.gnss_rows(g) for g in gnss], frames[0]["chi2_table"], gate_rows=True, strong_reject=False,
                       in_frame=not args.gnss_separate)
    ctx.sync()
    t_build = time.perf_counter() - t_build

    def one_step():
        ctx.frame_run(restore_prior=True)
        if gnss is not None and args.gnss_separate:
            ctx.gnss_run()

    def barrier():
        ctx.sync()
        grp.barrier()

    for _ in range(args.warmup):
        one_step()
    # Device conditioning (round 6, disclosed on the line as `device_conditioning`): the driver's window - W = 5 warm-up steps, K = 20
    # timed ones - is 12 ms of work on a device that idled while the host built the inputs, and its clock / power management has not
    # converged by then: in a rocprofv3 timeline the steps of such a run shorten monotonically from 520 to 494 us across warm-up and
    # timed region, and ms_per_step falls with K (K = 20: 0.503, 50: 0.490, 200: 0.485, 1000: 0.483; tools/gpu_steps_sweep.sh).  The
    # workload's own steps therefore run UNTIMED for COND_SECONDS of wall time first (blocks of 20 between syncs; first and last block's
    # ms per step are reported) - the timed region below is unchanged: exactly K full steps between two barrier + sync pairs.
    cond = None
    if not args.no_condition:
        blocks = []
        t_c0 = time.perf_counter()
        while time.perf_counter() - t_c0 < COND_SECONDS and len(blocks) < 200:
            ctx.sync(); t_b = time.perf_counter()
            for _ in range(20):
                one_step()
            ctx.sync(); blocks.append((time.perf_counter() - t_b) / 20 * 1e3)
        cond = dict(steps=20 * len(blocks), seconds=time.perf_counter() - t_c0, first_block_ms_per_step=blocks[0], last_block_ms_per_step=blocks[-1])
    # Per-kernel table: a separate UNTIMED pass of 3 steps with a HIP-event pair around every launch (an event pair
    # per launch costs ~6 % of the step, so the timed region below only brackets the dominant kernel).  --full only.
    prof, dom_name = {}, None
    if args.full and not args.no_profile:
        ctx.profile_select(None); ctx.profile_reset(); ctx.profile_enable(True)
        for _ in range(3):
            one_step()
        ctx.sync(); ctx.profile_enable(False)
        prof = ctx.profile_get()
        cand = [(ms / calls, name) for name, (ms, calls) in prof.items() if calls and name != "restore"]
        dom_name = max(cand)[1] if cand else None
        ctx.profile_select(dom_name)

    def timed_region():
        barrier()
        ctx.profile_reset()
        ctx.profile_enable(dom_name is not None)
        t0 = time.perf_counter()
        for i in range(args.steps):
            # the dominant kernel carries its events on every PROF_EVERY-th launch of the timed region (`launches_timed` on the line): a
            # launch with events attached still costs the step ~5 us (0.4888 against 0.4830 ms per step with every launch instrumented)
            if dom_name is not None and PROF_EVERY > 1:
                ctx.profile_enable(i % PROF_EVERY == 0)
            one_step()
        ctx.sync()
        dt = time.perf_counter() - t0
        ctx.profile_enable(False)
        return dt

    elapsed_local = timed_region()
    # AUXILIARY passes only (aux_configs: configs 3 and 5 behind the headline workload in the same process; never the headline): a
    # timed region that comes out more than 1.5 x slower per step than the conditioning block right before it is an outlier of the
    # run, not of the kernels (seen once in a dozen default runs: config 5 at 1.98 ms per step between runs at 0.96-0.97) - it is
    # timed once more, and the first figure is reported beside the second (`retimed`)
    retimed = None
    if aux and cond and elapsed_local / args.steps * 1e3 > 1.5 * cond["last_block_ms_per_step"]:
        retimed = dict(first_ms_per_step=elapsed_local / args.steps * 1e3, conditioned_ms_per_step=cond["last_block_ms_per_step"])
        elapsed_local = timed_region()
    if dom_name is not None:
        prof[dom_name] = ctx.profile_get()[dom_name]      # the dominant kernel: measured live inside the timed region
    elapsed = grp.max_over_ranks(elapsed_local)
    per_rank_ms = [t / args.steps * 1e3 for t in grp.gather_scalars(elapsed_local)]
    # weak scaling with no data-path collective: every rank must take the same time; a spread above 5 % means a straggler (a
    # throttled GPU, host-side serialisation) and is flagged in the line and on stderr - the driver computes efficiency itself
    rank_spread = (max(per_rank_ms) - min(per_rank_ms)) / min(per_rank_ms) if per_rank_ms else 0.0
    if rank == 0 and rank_spread > 0.05:
        print("bench.py: per-rank ms/step spread %.1f %% > 5 %%: %s" % (100 * rank_spread, ["%.3f" % t for t in per_rank_ms]), file=sys.stderr)

    if gnss is not None and args.gnss_separate:    # the separate GNSS pass reuses the row-count slot: fetch the frame's results in between
        ctx.frame_run(restore_prior=True)
    dx, acc, rows = ctx.frame_fetch()
    if gnss is not None and args.gnss_separate:
        ctx.gnss_run()
    n_acc = acc[:, :F].sum(axis=1)
    ok = bool(np.isfinite(dx).all() and (rows == 6 * C).all())
    gn_used = None
    if gnss is not None:
        dxg, gn_used, keep, gam, st = ctx.gnss_fetch()
        ok = ok and bool(np.isfinite(dxg).all() and (st == 0).all())
    lm_rows = None
    if real_lm:
        dxl, lm_rows, lacc, lgam, lst = ctx.landmark_fetch()
        ok = ok and bool(np.isfinite(dxl).all() and (lst == 0).all() and (lm_rows > 0).all())
    if args.dump_outputs and rank == 0 and not aux:
        arrays = dict(dx=dx[:, :N], accepted=acc[:, :F], rows=rows)
        if gnss is not None:
            arrays.update(gnss_dx=dxg[:, :N], gnss_rows=gn_used, gnss_keep=keep, gnss_gamma=gam, gnss_status=st)
        if real_lm:
            arrays.update(lm_dx=dxl[:, :N], lm_rows=lm_rows, lm_accepted=lacc, lm_gamma=lgam, lm_status=lst)
        dump_outputs(args.dump_outputs, ctx, B, arrays)
    # N > 1: every rank cross-checks its FIRST filter against the oracle (covariance, accept mask) - a rank whose device or
    # library misbehaves shows up in the line, not only rank 0's (--full)
    rank_par = [0.0, 1.0]
    if args.full and world > 1 and not real_lm:
        rp = oracle_parity_sample(ctx, one_step, steps, frames, gnss, infos[0]["n_prior"], ld, N, F, 1)
        rank_par = [rp["max_rel_cov_err"], float(rp["accept_mask_equal"])]
    # one end-of-run gather of per-rank summaries
    summ = grp.gather_summaries([float(n_acc.sum()), float(np.abs(dx).sum()), float(ok)] + rank_par)
    ok = bool(summ[:, 2].all())

    out = None
    if rank == 0:
        F_used = float(n_acc.mean())
        per_kernel, total_flops = algorithmic_flops(F_used, F, C, N, synth.IMU_PER_FRAME)
        bytes_k = algorithmic_bytes(N, synth.IMU_PER_FRAME, F, C)
        wkey = "c%d_B%d_F%d_C%d_N%d" % (args.config, B, F, C, N) + ("_lmreal" if real_lm else "") + ("" if stereo else "_mono")
        counters, csrc, kernels, roofline = None, None, {}, None
        if args.full:
            counters, csrc, rec_build = load_counters(args.counters, wkey)
            live_build = capi.build_id()
            kernels, roofline = price_kernels(prof, dom_name, counters, csrc, rec_build, live_build, C, B, per_kernel, bytes_k, stereo=stereo)
        cpu, parity = None, None
        if args.full and world > 1 and not real_lm:
            parity = dict(sample=world, filters="filter 0 of every rank", max_rel_cov_err=float(summ[:, 3].max()),
                          per_rank_rel_cov_err=[float(x) for x in summ[:, 3]], accept_mask_equal=bool(summ[:, 4].all()))
        oracle_1t = None
        if aux and not real_lm:
            # auxiliary workload: no CPU timing, but the same in-run cross-check against the oracle on a strided sample
            t_or = time.perf_counter()
            parity = oracle_parity_sample(ctx, one_step, steps, frames, gnss, infos[0]["n_prior"], ld, N, F, 2 if big else 8)
            # (python-side structure packing included: an upper bound of the oracle's single-thread update time, for the latency line)
            oracle_1t = (time.perf_counter() - t_or) / parity["sample"] * 1e3
        if args.full and world == 1 and not args.no_cpu and not real_lm and not aux:      # the C oracle's frame has no landmark update: parity of that path is tests/test_landmark_batch.py
            cpu, (P1, n1, dx1, acc1, S) = cpu_baseline(ctx, steps, frames, infos[0]["n_prior"], ld, quick=args.quick_cpu)
            ctx.frame_run(restore_prior=True)
            dxg, accg, rowsg = ctx.frame_fetch(0, S)
            errs = []
            for b in range(S):
                Pg = ctx.cov_get(b); nb = Pg.shape[0]
                Po = P1[b, :nb, :nb]
                errs.append(float(np.linalg.norm(Pg - Po) / np.linalg.norm(Po)))
            dd = np.abs(dxg[:S, :9] - dx1[:S, :9])
            parity = dict(sample=S, max_rel_cov_err=max(errs), accept_mask_equal=bool(np.array_equal(accg[:, :F], acc1[:, :F])),
                          max_abs_dtheta=float(dd[:, 0:3].max()), max_abs_dp=float(dd[:, 3:6].max()),
                          max_abs_dv=float(dd[:, 6:9].max()),
                          max_rel_dx_err=float(max(np.linalg.norm(dxg[b, :N] - dx1[b, :N]) / max(np.linalg.norm(dx1[b, :N]), 1e-300)
                                                   for b in range(S))))
        aw = None
        if cpu is not None and not big:
            # the reference as written (Q2/Q3): only the first 20 accepted features are used
            ctx.frame_stage(0, steps, frames, filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"],
                            max_accept=20, compress_rule=0)
            for _ in range(2):
                ctx.frame_run(restore_prior=True)
            ctx.sync()
            t_aw = time.perf_counter()
            for _ in range(5):
                ctx.frame_run(restore_prior=True)
            ctx.sync()
            t_aw = time.perf_counter() - t_aw
            aw = dict(gpu_updates_per_s=B * 5 / t_aw, cpu_ms_per_update_1thread=cpu.pop("as_written_cap20_ms_per_update_1thread"),
                      note="accepted-feature cap 20, all rows kept (RemoveLostUpdate.cpp:359,390): auxiliary figure, not `value`")
        # Host hand-over (auxiliary, never `value`): the ABI takes host buffers; one frame of the batch is packed into pinned
        # memory, sent over PCIe and the results fetched back.  serial = stage; run; fetch.  pipelined = run(i);
        # stage_async(i+1) on the copy stream into the second input set; fetch(i).
        handover = None
        if cpu is not None and not big and args.config == 2:
            kw = dict(max_accept=0, compress_rule=1)
            sg = (filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"])
            st_sync = ctx.frame_stage_prepare(0, steps, frames, *sg, **kw)
            st_async = ctx.frame_stage_prepare(0, steps, frames, *sg, use_async=True, **kw)
            for _ in range(4):                                # allocates the pinned ring and the second input set
                st_sync(); ctx.frame_run(restore_prior=True); ctx.frame_fetch()
            t0 = time.perf_counter()
            for _ in range(5):
                st_sync(); ctx.frame_run(restore_prior=True); ctx.frame_fetch()
            t_serial = (time.perf_counter() - t0) / 5
            def pipelined(stage_call, n):
                """run(i); fetch_begin(i); stage_async(i + 1); run(i + 1); fetch_end(i): the result copies of frame i sit in front of frame
                i + 1's kernels, the host packs and unpacks while the device computes (round 6: fetch in two halves)"""
                stage_call(); ctx.frame_run(restore_prior=True)
                for _ in range(n):
                    ctx.frame_fetch_begin(); stage_call(); ctx.frame_run(restore_prior=True); res = ctx.frame_fetch_end()
                ctx.frame_fetch()
                return res
            pipelined(st_async, 3)
            t0 = time.perf_counter()
            pipelined(st_async, 10)
            t_pipe = (time.perf_counter() - t0) / 11
            ctx.sync()
            in_bytes = sum(np.asarray(v).nbytes for v in frames[0].values() if hasattr(v, "nbytes")) + \
                sum(np.asarray(v).nbytes for v in steps[0].values() if hasattr(v, "nbytes"))
            stg = None
            if not aux and world == 1:
                try:                                      # one PROCESS per stager, as ranks are (the threaded variant: tests/test_gpu_stagers.py)
                    stg = stagers_rate_processes(8, 64, reps=20)
                    stg["host_threads"] = os.cpu_count()
                    stg["tracks"] = stagers_rate_processes(8, 64, reps=20, mode="tracks")["aggregate_updates_per_s"]
                except Exception as e:                    # auxiliary figure: never takes the bench line down
                    stg = dict(error=str(e)[-200:])
            # the same hand-over as a DELTA on the device-resident track store (round 6): one new column per frame + the track list + raw IMU
            trk = None
            try:
                ref_dx, ref_acc, _ = (ctx.frame_run(restore_prior=True), ctx.frame_fetch())[1]
                tk_sync, tk_bytes = tracks_handover_prepare(ctx, steps, frames, sg, False, kw)
                for _ in range(3):
                    tk_sync(); ctx.frame_run(restore_prior=True); dxt, acct, _r = ctx.frame_fetch()
                same = bool(np.array_equal(acct, ref_acc) and np.linalg.norm(dxt - ref_dx) <= 1e-9 * np.linalg.norm(ref_dx))
                t0 = time.perf_counter()
                for _ in range(5):
                    tk_sync(); ctx.frame_run(restore_prior=True); ctx.frame_fetch()
                t_tser = (time.perf_counter() - t0) / 5
                tk_async, _ = tracks_handover_prepare(ctx, steps, frames, sg, True, kw)
                pipelined(tk_async, 3)
                t0 = time.perf_counter()
                dxp, accp, _r = pipelined(tk_async, 10)
                t_tpipe = (time.perf_counter() - t0) / 11
                same = same and bool(np.array_equal(accp, ref_acc) and np.linalg.norm(dxp - ref_dx) <= 1e-9 * np.linalg.norm(ref_dx))
                ctx.sync()
                trk = dict(serial_updates_per_s=B / t_tser, pipelined_updates_per_s=B / t_tpipe, input_bytes_per_update=tk_bytes,
                           same_result_as_staged_frame=same,
                           note="ingvio_frame_stage_tracks: observations stay on the device, a frame = the new clone's column + window / track "
                                "bookkeeping + the track list of the update + raw IMU samples (Phi / G formed on the device)")
            except Exception as e:
                trk = dict(error=str(e)[-300:])
            handover = dict(serial_updates_per_s=B / t_serial, pipelined_updates_per_s=B / t_pipe, input_bytes_per_update=in_bytes, stagers8=stg, tracks=trk,
                            note="host buffers -> pinned slab (8 host threads) -> PCIe -> run -> dx/accept back; pipelined = copy "
                                 "stream + second device input set (ingvio_frame_stage_async) + the fetch in two halves (ingvio_frame_fetch_begin / _end); auxiliary, `value` is device-resident")
        updates = B * world * args.steps
        step_desc = ("propagate(k=10)+clone+MSCKF update" + ("+landmark update (%d in-state landmarks, per-landmark chi2 gates)" % n_lm_real if real_lm else "")
                     + "+marginalise" + (("+GNSS update (8 sats, per-row chi2 gates, %s)" % ("separate pass" if args.gnss_separate else "in-frame: one sweep over P"))
                                         if gnss is not None else ""))
        # executed FP64 rate of the whole step, where counters exist for every kernel that ran
        step_exec = None
        if counters is not None:
            tot, missing = 0.0, []
            for name, e in kernels.items():
                if "executed_fp64_flop_per_launch" in e:
                    tot += e["executed_fp64_flop_per_launch"]
                elif name not in ("restore", "k_marginalize"):
                    missing.append(name)
            complete = not missing                       # a kernel without current counters makes the sum a lower bound only
            step_exec = dict(executed_fp64_flop_per_step=tot, tflops=tot / (elapsed / args.steps) / 1e12,
                             frac_fp64_peak=tot / (elapsed / args.steps) / 1e12 / FP64_PEAK_TFLOPS if complete else None,
                             kernels_without_current_counters=missing)
        out = dict(
            metric="ekf_updates_per_sec", value=updates / elapsed, unit="updates/s", n_gpus=world, steps=args.steps,
            warmup=args.warmup, ms_per_step=elapsed / args.steps * 1e3, higher_is_better=True, scaling="weak",
            vs_baseline=None, dtype="f64", data="synthetic",
            config=dict(workload="BASELINE configs[%d]: synthetic %s MSCKF, %d feats x %d clones, state dim N=%d (update at N), "
                                 "%d independent filters per GPU; step = %s" % (args.config - 1, "stereo" if stereo else "MONO", F, C, N, B, step_desc),
                        baseline_config=args.config, filters_per_gpu=B, feats=F, clones=C, state_dim=N, imu_steps=synth.IMU_PER_FRAME,
                        gnss_rows_used_per_filter=None if gn_used is None else float(np.mean(gn_used)),
                        landmarks=args.landmarks if n_lm else None, landmarks_in_state=n_lm_real if real_lm else 0,
                        landmark_rows_per_filter=None if lm_rows is None else float(np.mean(lm_rows)),
                        parallelism="independent filters, %d rank(s), no data-path collective" % world),
            ms_per_update=elapsed / args.steps * 1e3 / B, per_rank_ms_per_step=per_rank_ms, per_rank_spread=rank_spread, rank_balance_ok=bool(rank_spread <= 0.05), accepted_per_filter=F_used, results_finite=ok,
            algorithmic_flops_per_update=total_flops, whole_step_executed=step_exec,
            device_conditioning=cond, retimed=retimed, method=args.method, roofline=roofline, cpu_baseline=cpu, parity_vs_oracle=parity, as_written_cap20=aw, host_handover=handover,
            kernels=kernels, oracle_update_ms_upper_bound=oracle_1t,
            kernels_note="per-kernel avg_ms: separate untimed pass of 3 steps with an event pair around every launch; the "
                         "roofline kernel's avg_ms is from the timed region; executed_* and hbm_* come from the committed PMC passes "
                         "(%s)" % csrc, setup_s=t_build)
    ctx.close()
    return out


def stagers_rate(n_stagers=8, filters_each=64, F=150, C=11, n_gnss=6, n_lm=52, reps=12, device=0):
    """Host hand-over under concurrent stagers (SURVEY 8(d) config 4 "report both"): `n_stagers` contexts of
    `filters_each` filters on ONE GPU, each driven by its own host thread through the pipelined hand-over
        run(i); stage_async(i + 1); fetch(i)
    (pinned slab -> copy stream -> second device input set; ctypes releases the GIL inside the library calls, so the threads pack
    and copy concurrently) - what 8 ranks of one host would do to the PCIe root and the host cores.  Returns the aggregate staged
    updates/s, the same for one stager alone, and the device-resident rate of one context (run only) for scale.  Auxiliary: never
    `value`."""
    import threading
    from ingvio_amd import capi, synth
    N = 21 + n_gnss + 3 * n_lm + 6 * C
    pr = synth.PARAMS
    ctxs, calls, lock_free = [], [], []
    for s in range(n_stagers):
        ctx = capi.Context(batch=filters_each, n_max=((N + 15) // 16) * 16, c_max=C, f_max=F, m_max=64, device=device)
        filters, steps, frames, infos = build_batch(ctx, filters_each, 4000 + 97 * s, F, C, n_gnss, n_lm)
        ctx.snapshot()
        st = ctx.frame_stage_prepare(0, steps, frames, filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"],
                                     max_accept=0, compress_rule=1, use_async=True)
        st(); ctx.frame_run(restore_prior=True); st(); ctx.frame_fetch(); ctx.sync()      # allocates the pinned ring and the second input set
        ctxs.append(ctx); calls.append(st)
        lock_free.append((steps, frames))

    def loop(i, n, out):
        ctx, st = ctxs[i], calls[i]
        for _ in range(n):
            ctx.frame_run(restore_prior=True); st(); out[i] = ctx.frame_fetch()
        ctx.sync()

    def timed(active, n):
        res = [None] * n_stagers
        th = [threading.Thread(target=loop, args=(i, n, res)) for i in active]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        return time.perf_counter() - t0, res
    timed(range(n_stagers), 2)                                            # warm-up
    t_all, res_all = timed(range(n_stagers), reps)
    t_one, res_one = timed([0], reps)
    # one context device-resident (no staging, no fetch) for scale
    ctxs[0].sync(); t0 = time.perf_counter()
    for _ in range(reps):
        ctxs[0].frame_run(restore_prior=True)
    ctxs[0].sync(); t_dev = time.perf_counter() - t0
    same = bool(np.array_equal(res_all[0][0], res_one[0][0]) and np.array_equal(res_all[0][1], res_one[0][1]))
    finite = all(bool(np.isfinite(r[0]).all()) for r in res_all)
    for c in ctxs:
        c.close()
    return dict(stagers=n_stagers, filters_each=filters_each, aggregate_updates_per_s=n_stagers * filters_each * reps / t_all,
                one_stager_updates_per_s=filters_each * reps / t_one, device_resident_one_context_updates_per_s=filters_each * reps / t_dev,
                concurrent_equals_alone=same, results_finite=finite, host_threads=os.cpu_count())


def tracks_handover_prepare(ctx, steps, frames, sigma_args, use_async, kw):
    """Device-resident track store (ingvio_tracks_create / ingvio_frame_stage_tracks): fills the store with the batch's frames column by
    column (one delta per window slot, the points with the last one), then returns (steady-state call, input bytes per update).  The
    steady-state frame is what a running filter sends: the newest window slot leaves and arrives again with its column (one measurement
    per track), the clone table, the list of tracks the update uses, the raw IMU samples - the store and therefore the staged frame are
    the same after every call, so the step computes what the fully staged frame computes (checked by the caller).  The points are NOT
    re-sent: in a running filter they are the device's own triangulation results (ingvio_msckf_update_tri)."""
    B = len(steps)
    F, C = np.asarray(frames[0]["uv"]).shape[:2]
    ctx.tracks_create(F)
    base = [dict(clone_idx=fr["clone_idx"], clone_R=fr["clone_R"], clone_p=fr["clone_p"], feat_track=[], feat_anchor=[], feat_dof=[]) for fr in frames]
    tracks = np.arange(F, dtype=np.int32)

    def col(fr, s, **extra):
        return dict(append=s, obs_track=tracks, obs_uv=np.ascontiguousarray(np.asarray(fr["uv"])[:, s, :]), **extra)
    for s in range(C):
        last = s == C - 1
        tfs = [dict(base[b], **col(frames[b], s, **(dict(pf_track=tracks, pf=frames[b]["pf"]) if last else {}))) for b in range(B)]
        ctx.frame_stage_tracks_prepare(0, steps, tfs, frames[0], *sigma_args, **kw)()
    tfs = [dict(base[b], drop=[C - 1], feat_track=tracks, feat_anchor=frames[b]["anchor"], feat_dof=frames[b]["dof"], **col(frames[b], C - 1)) for b in range(B)]
    call = ctx.frame_stage_tracks_prepare(0, steps, tfs, frames[0], *sigma_args, use_async=use_async, **kw)
    k = len(steps[0]["dt"])
    nbytes = 4 * (32 + 1 + F + C + F + 5) + 8 * (4 * F + 12 * C + 7 * k + 24)      # header + ints + doubles of one filter's delta (capi.hip: ingvio_frame_stage_tracks)
    return call, nbytes


def _stager_child():
    """One stager PROCESS of stagers_rate_processes(): builds its own 64-filter context, reports READY, waits for the common start
    time on stdin, runs the pipelined hand-over loop and prints its own start / end wall-clock times."""
    from ingvio_amd import capi, synth
    i, n_f, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    F, C, n_gnss, n_lm = 150, 11, 6, 52
    N = 21 + n_gnss + 3 * n_lm + 6 * C
    pr = synth.PARAMS
    ctx = capi.Context(batch=n_f, n_max=((N + 15) // 16) * 16, c_max=C, f_max=F, m_max=64, device=int(os.environ.get("INGVIO_DEVICE", "0")))
    filters, steps, frames, infos = build_batch(ctx, n_f, 4000 + 97 * i, F, C, n_gnss, n_lm)
    ctx.snapshot()
    if len(sys.argv) > 5 and sys.argv[5] == "tracks":      # the hand-over as a delta on the device-resident track store
        st, _ = tracks_handover_prepare(ctx, steps, frames, (filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"]), True,
                                        dict(max_accept=0, compress_rule=1))
    else:
        st = ctx.frame_stage_prepare(0, steps, frames, filters[0].sigma(), filters[0].enable_gnss, pr["sigma_cb"], pr["sigma_rw"], max_accept=0,
                                     compress_rule=1, use_async=True)
    st()
    for _ in range(3):
        ctx.frame_run(restore_prior=True); st(); ctx.frame_fetch()
    ctx.sync()
    print("READY", flush=True)
    t_start = float(sys.stdin.readline())
    while time.time() < t_start:
        pass
    t0 = time.time()
    ctx.frame_run(restore_prior=True)
    for _ in range(reps - 1):
        ctx.frame_fetch_begin(); st(); ctx.frame_run(restore_prior=True); dx, acc, rows = ctx.frame_fetch_end()
    dx, acc, rows = ctx.frame_fetch()
    ctx.sync()
    t1 = time.time()
    print(json.dumps(dict(t0=t0, t1=t1, finite=bool(np.isfinite(dx).all()), accepted=float(acc.sum()) / n_f)), flush=True)
    ctx.close()


def stagers_rate_processes(n_stagers=8, filters_each=64, reps=20, mode="frames"):
    """The same hand-over loop as stagers_rate() with one PROCESS per stager - what `torchrun --nproc-per-node 8` ranks of one host
    are: own interpreter, own HIP runtime, own copy queues - all on GPU 0 here (a one-GPU box), started together.  Aggregate =
    all staged updates / (last end - first start)."""
    import subprocess
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--stager-child", str(i), str(filters_each), str(reps), mode], stdin=subprocess.PIPE,
                              stdout=subprocess.PIPE, text=True, cwd=ROOT) for i in range(n_stagers)]
    try:
        for p in procs:
            line = p.stdout.readline()
            if not line.startswith("READY"):
                raise RuntimeError("stager child failed: %r" % line)
        t_start = time.time() + 0.5
        for p in procs:
            p.stdin.write("%r\n" % t_start); p.stdin.flush()
        res = [json.loads(p.stdout.readline()) for p in procs]
    finally:
        for p in procs:
            try:
                p.wait(timeout=60)
            except Exception:
                p.kill()
    span = max(r["t1"] for r in res) - min(r["t0"] for r in res)
    return dict(stagers=n_stagers, filters_each=filters_each, reps=reps, aggregate_updates_per_s=n_stagers * filters_each * reps / span,
                per_stager_updates_per_s=[filters_each * reps / (r["t1"] - r["t0"]) for r in res], results_finite=all(r["finite"] for r in res))


REPLAY_TOOL = os.path.join(ROOT, "ingvio_amd", "lib", "ingvio_replay")
LATENCY_STREAMS = {      # SynthStream.h specs: every `life` frames a whole cohort of tracks is lost -> one RemoveLost update over all of them
    "config2": "feats=150,clones=11,life=10,cohort=1,birth_frame=3,frames=75,key=1",
    "config5": "feats=300,clones=30,life=28,cohort=1,birth_frame=2,frames=125,key=1",      # births on the frames whose clone survives the next key-frame marginalisation (SynthStream.h)
}


STAGGERED_STREAMS = {
    "kf11": "feats=150,clones=11,life=10,cohort=0,frames=90,key=1",
    "kf21": "feats=100,clones=21,life=19,cohort=0,frames=90,key=1",
    "kf27": "feats=150,clones=27,life=25,cohort=0,frames=110,key=1",
    # sliding-window mode (is_key_frame 0) at BASELINE's 11 poses: 12 clones at update time, the oldest marginalised every frame, three
    # selected stamps (frame_select_interval 5) - window class 72 of the solve since round 6
    "sw11": ("feats=150,clones=11,life=13,cohort=0,frames=90,key=0", ["--set", "frame_select_interval: 5"]),
    # the reference's shipped MONO configuration (config/sportsfield/ingvio_mono.yaml: 35 poses)
    "kf35_mono": "feats=150,clones=35,life=33,cohort=0,frames=120,key=1,stereo=0",
}


def latency_b1(args):
    """Single-filter latency: ONE filter driven through the C++ shim's callback surface
    (IngvioFilter::callbackIMU / callbackStereoFrame, IngvioFilter.cpp:252-379: propagate + clone, RemoveLost update, key-frame
    update, re-anchoring, marginalisation - as the reference sequences them) on a synthetic stream, wall time per camera
    callback measured inside tools/ingvio_replay.cpp.  `heavy` = the frames on which a whole cohort of tracks is lost (150 / 300
    features with up to window - 1 observations each in one RemoveLost update); `lifted` runs RemoveLost without the reference's
    accepted-feature cap of 20 and with top-n compression (quirks Q3 / Q2 off), `as_written` with both as in the reference."""
    import subprocess
    if not os.path.exists(REPLAY_TOOL):
        return dict(error="ingvio_replay not built")
    out = {}
    for name, spec in LATENCY_STREAMS.items():
        e = {}
        for label, sets in (("lifted", ["--set", "hip_max_valid_ids: 0", "--set", "hip_compress_rule: 1"]), ("as_written", [])):
            try:
                r = subprocess.run([REPLAY_TOOL, "--synth", spec, "--time"] + sets, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                e[label] = dict(error="timeout"); continue
            line = [l for l in r.stdout.splitlines() if l.startswith("LATENCY")]
            if r.returncode != 0 or not line:
                e[label] = dict(error=(r.stderr or r.stdout)[-200:]); continue
            kv = dict(x.split("=") for x in line[0].split()[1:])
            e[label] = dict(heavy_ms=float(kv["heavy_median_ms"]), heavy_min_ms=float(kv["heavy_min_ms"]), heavy_frames=int(kv["heavy_frames"]),
                            heavy_accepted=int(kv["heavy_accepted"]), heavy_rows=int(kv["heavy_rows"]), other_ms=float(kv["other_median_ms"]),
                            all_ms=float(kv["median_ms"]), frames=int(kv["timed"]), final_pos_err_m=float(kv["final_pos_err_m"]))
        e["stream"] = spec
        out[name] = e
    # every frame loses a few tracks (staggered deaths) - what a running tracker delivers: median over ALL camera callbacks, as written,
    # at the window sizes of the reference's shipped stereo configurations (config/fw_zed2i_f9p: 21 poses, config/sportsfield: 27)
    st = {}
    for name, spec in STAGGERED_STREAMS.items():
        sets = []
        if isinstance(spec, tuple):
            spec, sets = spec
        try:
            r = subprocess.run([REPLAY_TOOL, "--synth", spec, "--time"] + sets, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            st[name] = dict(error="timeout"); continue
        line = [l for l in r.stdout.splitlines() if l.startswith("LATENCY")]
        if r.returncode != 0 or not line:
            st[name] = dict(error=(r.stderr or r.stdout)[-200:]); continue
        kv = dict(x.split("=") for x in line[0].split()[1:])
        st[name] = dict(median_ms=float(kv["median_ms"]), frames=int(kv["timed"]), stream=spec)
    out["staggered"] = st
    return out


AUX_KEYS = ("value", "unit", "ms_per_step", "ms_per_update", "steps", "warmup", "config", "accepted_per_filter", "results_finite", "retimed",
            "roofline", "whole_step_executed", "parity_vs_oracle", "kernels", "setup_s", "oracle_update_ms_upper_bound")
PROF_EVERY = 4                           # timed region: the dominant kernel's events ride on every 4th of its launches
COND_SECONDS = 0.25                      # untimed steps of the workload in front of the timed region (run_workload: device conditioning)
LINE_LIMIT = 6000                        # the driver keeps the last ~8 KB of stdout: the final line must fit with room to spare


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def _rnd(x, sig=6):
    """Floats to `sig` significant digits (the line is for a parser and a reader, not for bit-exact replay)."""
    if isinstance(x, float):
        return float("%.*g" % (sig, x)) if np.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _rnd(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_rnd(v, sig) for v in x]
    return x


def compact_line(full, detail=True):
    """The ONE JSON line the driver parses, from the full result dict: the contract's keys, `roofline` and `cpu_baseline` reduced
    to their figures, a compact `aux_configs`; per-kernel tables, notes, the host hand-over and the as-written figures stay in
    bench_detail.json.  VERDICT r03 #1: the round-3 line (22 KB) no longer fitted the driver's stdout tail."""
    out = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data", "ms_per_update", "per_rank_ms_per_step", "rank_balance_ok",
                       "accepted_per_filter", "results_finite", "device_conditioning"))
    out["config"] = _pick(full.get("config"), ("workload", "baseline_config", "filters_per_gpu", "feats", "clones", "state_dim",
                                               "imu_steps", "parallelism"))
    rl = full.get("roofline")
    if rl is not None:
        r = _pick(rl, ("kernel", "bound", "achieved", "peak", "unit", "frac", "useful_frac", "traffic", "avg_launch_ms",
                       "launches_timed", "counters_stale", "counters"))
        r["executed_flop_per_launch"] = rl.get("executed_fp64_flop_per_launch")
        r["algorithmic_flop_per_launch"] = (rl.get("algorithmic") or {}).get("flop_per_launch")
        out["roofline"] = r
    ws = full.get("whole_step_executed")
    if ws is not None:
        out["whole_step_frac_fp64_peak"] = ws.get("frac_fp64_peak")
    cb = full.get("cpu_baseline")
    if cb is not None:
        c = _pick(cb, ("value", "unit", "cores", "kind"))
        c["sample"] = "oracle/ingvio_oracle.c on the bench's own frames; value: one filter per thread, one_thread: 1 filter, 1 thread"
        c["one_thread"] = _pick(cb.get("one_thread"), ("ms_median", "ms_p95", "timed"))
        out["cpu_baseline"] = c
    else:
        out["cpu_baseline"] = None
    out["parity_vs_oracle"] = _pick(full.get("parity_vs_oracle"), ("sample", "max_rel_cov_err", "accept_mask_equal", "max_rel_dx_err",
                                                                   "per_rank_rel_cov_err"))
    lat = full.get("latency_b1_ms")
    if lat is not None:
        # one filter, C++ shim callbacks, ms per camera callback: heavy = a RemoveLost update over a whole lost cohort (cap lifted /
        # as written: cap 20, all rows kept), other = the frames in between; the oracle's single-thread update time beside it
        cl = {}
        for k, e in lat.items():
            if not isinstance(e, dict) or k == "staggered":
                continue
            c = {}
            for label in ("lifted", "as_written"):
                v = e.get(label) or {}
                c[label] = _pick(v, ("heavy_ms", "heavy_accepted", "other_ms", "error"))
            c["oracle_1thread_update_ms"] = e.get("oracle_1thread_update_ms")
            cl[k] = c
        if isinstance(lat.get("staggered"), dict):      # a few lost tracks per frame, median over all callbacks, key-frame mode at 11 / 21 / 27 poses
            cl["staggered_median_ms"] = {k: (v.get("median_ms") if "median_ms" in v else v.get("error")) for k, v in lat["staggered"].items()}
        out["latency_b1_ms"] = cl
    if full.get("aux_configs"):
        out["aux_configs"] = {
            k: dict(value=v.get("value"), ms_per_step=v.get("ms_per_step"), workload=(v.get("config") or {}).get("workload"),
                    roofline_kernel=(v.get("roofline") or {}).get("kernel"), roofline_frac=(v.get("roofline") or {}).get("frac"),
                    max_rel_cov_err=(v.get("parity_vs_oracle") or {}).get("max_rel_cov_err"),
                    accept_mask_equal=(v.get("parity_vs_oracle") or {}).get("accept_mask_equal"))
            for k, v in full["aux_configs"].items()}
        for k, v in full["aux_configs"].items():
            if v.get("retimed"):                          # an outlier of the run was timed a second time (run_workload): both figures on the line
                out["aux_configs"][k]["retimed"] = v["retimed"]
    hh = full.get("host_handover")
    if hh is not None:
        # host buffers in, results out (never `value`): one context serial / pipelined, and 8 concurrent stagers x 64 filters on this GPU
        h = _pick(hh, ("serial_updates_per_s", "pipelined_updates_per_s"))
        s8 = hh.get("stagers8") or {}
        h["stagers8_aggregate_updates_per_s"] = s8.get("aggregate_updates_per_s")
        h["stagers8_host_threads"] = s8.get("host_threads")
        tk = hh.get("tracks") or {}      # the hand-over as a delta on the device-resident track store (round 6)
        h["tracks"] = dict(serial=tk.get("serial_updates_per_s"), pipelined=tk.get("pipelined_updates_per_s"), bytes_per_update=tk.get("input_bytes_per_update"),
                           same_result=tk.get("same_result_as_staged_frame"), stagers8_aggregate=s8.get("tracks"), error=tk.get("error"))
        h["bytes_per_update"] = hh.get("input_bytes_per_update")
        out["host_handover"] = h
    if detail:
        out["detail"] = "bench_detail.json (per-kernel table, notes, host hand-over, as-written cap-20 figures)"
    line = json.dumps(_rnd(out))
    assert len(line) < LINE_LIMIT, "bench line %d chars >= %d: move keys to bench_detail.json" % (len(line), LINE_LIMIT)
    return line


def main():
    args = parse_args()
    from ingvio_amd.parallel import Group
    grp = Group()                                  # RCCL ("nccl") when WORLD_SIZE > 1 (INGVIO_DIST_BACKEND=gloo: shared-device test)
    out = run_workload(args, grp, aux=False)
    # BASELINE configs 3 and 5 on the same clock: after the headline measurement the default single-GPU run
    # makes a short pass over each and reports it under `aux_configs` (same steps / warm-up, no CPU timing, an in-run oracle
    # parity sample each).  The headline keys above are config 2's alone.  --full only.
    if args.full and grp.world == 1 and args.config == 2 and not args.no_aux and args.method == "factored" and args.landmarks == "padded":
        aux = {}
        for cfg in (3, 5):
            a = argparse.Namespace(**vars(args))
            a.config, a.batch, a.feats, a.clones, a.state, a.no_cpu = cfg, None, None, None, "nominal", True
            r = run_workload(a, grp, aux=True)
            aux["config%d" % cfg] = {k: r[k] for k in AUX_KEYS if k in r}
        out["aux_configs"] = aux
        if not args.no_latency:
            lat = latency_b1(args)
            if isinstance(lat.get("config2"), dict) and out.get("cpu_baseline"):
                lat["config2"]["oracle_1thread_update_ms"] = out["cpu_baseline"]["one_thread"]["ms_median"]
            if isinstance(lat.get("config5"), dict):
                lat["config5"]["oracle_1thread_update_ms"] = aux["config5"].get("oracle_update_ms_upper_bound")
            out["latency_b1_ms"] = lat
    if grp.rank == 0:
        if args.full:
            try:
                with open(args.detail, "w") as f:
                    json.dump(out, f, indent=1)
            except OSError as e:                   # read-only checkout: the line still goes out
                print("bench.py: could not write %s: %s" % (args.detail, e), file=sys.stderr)
        print(compact_line(out, detail=args.full))
    grp.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--stager-child":
        _stager_child()
    else:
        main()
