"""Shader-clock phases of k_feat_gram3's two roles on config 2 (needs a kernels_factored build with -DINGVIO_DBG_STAMPS, e.g.
tools/build_tu_variant.sh s1144 kernels_factored -DINGVIO_DBG_STAMPS, selected with INGVIO_HIP_LIB).  Workgroup (0, 0), batch 3 of
its chunk: wave 0 stamps the producer role (P2 of the next batch, its tiles, the wait at the barrier), wave 2 the consumer role (its
tiles, the sparse sums, the wait)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from ingvio_amd import capi, synth
B = 512
ctx = capi.Context(batch=B, n_max=256, c_max=11, f_max=150, m_max=64)
filters, steps, frames, infos = bench.build_batch(ctx, B, 0, 150, 11, 6, 52)
ctx.snapshot(); pr = synth.PARAMS
ctx.frame_stage(0, steps, frames, filters[0].sigma(), 1, pr["sigma_cb"], pr["sigma_rw"])
for _ in range(3):
    ctx.frame_run(restore_prior=True)
print("gram form", ctx.last_gram_form())
d = ctx.debug_read(64)
print("producer (wave 0), batch 3: P2 %d  tiles %d  wait %d  period %d" % (d[37] - d[36], d[41] - d[37], d[42] - d[41], d[42] - d[36]))
print("consumer (wave 2), batch 3: tiles %d  sparse sums %d  wait %d  period %d" % (d[57] - d[56], d[58] - d[57], d[59] - d[58], d[59] - d[56]))
print("prologue %d  total %d  batches %d" % (d[33] - d[32], d[40] - d[32], -(-int(max(f["pf"].shape[0] for f in frames)) // 8)))
