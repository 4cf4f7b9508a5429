"""The resident training step of PostBiSelfAttentionRGCN (`--module BiSARGCN --post-aggregation`) with the split all-entity pass
on and off, and BiSelfAttentionRGCN on the same windows for scale.  Workload shapes of bench.py's synthetic table (bench.py
--encoder attention); the default S-gdelt has no inactive entities (500 entities, 500 nodes per snapshot: the all-entity attention
never runs there), so the probe defaults to the two ICEWS shapes, where B * N_inactive rows attend.

One prepared batch, fixed draws, own gates, eager launches.  Timing: device events around every step, warm-up, the three variants
interleaved step by step in one process, median and quartiles over --steps steps each.  Also prints the library kernels of one step
of the two routes (HIP-event trace).

    python tools/post_attention_probe.py [--workload S-icews14 S-icews0515] [--steps 30]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd.post_self_attention_rgcn import PostBiSelfAttentionRGCN  # noqa: E402
from temp_amd.sampling import CorruptTriples  # noqa: E402
from temp_amd.self_attention_rgcn import BiSelfAttentionRGCN  # noqa: E402


def build(cls, w, device, targets, **flags):
    args = bench.make_args(w, "BiSARGCN")
    args.EMA = False
    for k, v in flags.items():
        setattr(args, k, v)
    torch.manual_seed(1)
    m = cls(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(device)
    m.sample_rng = np.random.default_rng(2)
    m.corrupter = CorruptTriples(m.args, w["snapshots"], seed=5)
    wb = m.prepare(targets, w["L"], True)
    fixed = [tuple(x.to(device) for x in smp) for smp in m.draw_samples(wb)]
    return m, wb, fixed


def probe(name, steps, warm, lib, device):
    w = synthetic.workload(name, seed=0)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 3)
    post, wb, fixed = build(PostBiSelfAttentionRGCN, w, device, targets, post_aggregation=True)
    base, wb0, fixed0 = build(BiSelfAttentionRGCN, w, device, targets)

    def post_step(split):
        def run():
            post.split_all_entity = split
            return post.run_loss(wb, fixed)
        return bench.GraphStep(run, list(post.parameters()), graph=False)

    variants = [("PostBiSelfAttentionRGCN, split all-entity pass", post_step(True)),
                ("PostBiSelfAttentionRGCN, unsplit (materialised rows)", post_step(False)),
                ("BiSelfAttentionRGCN (no local stream, no gates)", bench.GraphStep(lambda: base.run_loss(wb0, fixed0), list(base.parameters()), graph=False))]
    for _ in range(warm):
        for _, st in variants:
            st.eager()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(steps):                                   # interleaved: drift of the shared machine hits all variants alike
        for k, (_, st) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.eager()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    D, N, B = w["D"], w["num_ents"], len(wb.graphs)
    T = wb.idx_all.shape[1] + 1
    print("\n%s: %d entities, D = %d, L = %d (T = %d positions), bsz %d; %d target rows, %d history-table rows, %d inactive (window, entity) rows"
          % (name, N, D, w["L"], T, B, int(sum(wb.target_sizes)), wb.n_hist_rows, wb.n_inactive))
    qkv_flop = lambda rows: 3 * 2.0 * rows * D * 3 * D       # forward + the two backward products
    print("  Q/K/V product of the all-entity pass (fwd + bwd): unsplit %d rows, %.2f GFLOP, %.1f MB (n, 3D) buffer + its gradient; "
          "split %d rows, %.2f GFLOP, %.1f MB gradient buffer"
          % (wb.n_inactive, qkv_flop(wb.n_inactive) / 1e9, 2 * wb.n_inactive * 3 * D * 4 / 1e6, N + B, qkv_flop(N + B) / 1e9,
             wb.n_inactive * 3 * D * 4 / 1e6))
    for (what, _), ts in zip(variants, times):
        q = np.percentile(ts, [25, 50, 75])
        print("  %-54s median %.3f ms/step  (quartiles %.3f - %.3f, %d steps)" % (what, q[1], q[0], q[2], len(ts)))
    med = [float(np.median(ts)) for ts in times]
    print("  split / unsplit = %.3f;  split / BiSelfAttentionRGCN = %.3f" % (med[0] / med[1], med[0] / med[2]))
    for what, st in variants[:2]:
        kernels = bench.traced_steps(st.eager, 3, lib)
        tot_ms = sum(v["ms_per_step"] for v in kernels.values())
        tot_n = sum(v["launches_per_step"] for v in kernels.values())
        print("  %s: library kernels of one step (median of 3 traced steps): %d launches, %.3f ms" % (what, round(tot_n), tot_ms))
        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])[:8]:
            print("    %-28s %4d launches  %8.4f ms" % (k, round(v["launches_per_step"]), v["ms_per_step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["S-icews14", "S-icews0515"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 (the median of fewer steps is not reported)")
    device = torch.device("cuda", 0)
    lib = _lib.load()
    print("device: %s; eager launches, device events per step, variants interleaved" % torch.cuda.get_device_name(0))
    for name in a.workload:
        probe(name, a.steps, a.warmup, lib, device)


if __name__ == "__main__":
    main()
