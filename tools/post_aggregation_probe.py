"""One training step of PostBiDynamicRGCN (`--post-aggregation`, embedding-level gate) against PostEnsembleBiDynamicRGCN
(`--post-ensemble`, score-level mix) at the config-3 shape: S-icews0515 workload, BiGRRGCN --rec-only-last-layer, L = 15, bsz 8,
fixed draws (the setup of bench.py's config-3 leg).  Both models use their OWN frequency-MLP gates inside the step, on feature
rows computed once per prepared batch.  Reports ms per step eagerly and under HIP-graph replay, and the library kernels of one
step (HIP-event trace: launches and ms per kernel).

    python tools/post_aggregation_probe.py [--steps 30]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN, PostEnsembleBiDynamicRGCN  # noqa: E402
from temp_amd.sampling import CorruptTriples  # noqa: E402


def build(cls, flag, w, device):
    args = bench.make_args(w, "BiGRRGCN")
    setattr(args, flag, True)
    torch.manual_seed(1)
    m = cls(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(device)
    m.sample_rng = np.random.default_rng(2)
    m.corrupter = CorruptTriples(m.args, w["snapshots"], seed=5)
    wb = m.prepare(synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 3), w["L"], True)
    fixed = [tuple(x.to(device) for x in smp) for smp in m.draw_samples(wb)]
    return m, wb, fixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    lib = _lib.load()
    w = synthetic.workload("S-icews0515", seed=0)

    m_e, wb_e, fx_e = build(PostEnsembleBiDynamicRGCN, "post_ensemble", w, device)
    feats = [m_e.ensemble_features(smp[0], wb_e.rows[i][-1], g) for i, (smp, g) in enumerate(zip(fx_e, wb_e.graphs))]

    def ens_step():
        wts = [(torch.sigmoid(m_e.subject_linear(sf)), torch.sigmoid(m_e.object_linear(of))) for sf, of in feats]
        return m_e.run_loss(wb_e, fx_e, wts)

    m_a, wb_a, fx_a = build(PostBiDynamicRGCN, "post_aggregation", w, device)

    def agg_step():
        return m_a.run_loss(wb_a, fx_a)                 # own gates: features cached on the prepared batch

    rows = []
    for name, fn, m in (("PostEnsembleBiDynamicRGCN", ens_step, m_e), ("PostBiDynamicRGCN", agg_step, m_a)):
        params = list(m.parameters())
        # captured FIRST, as in bench.py: the impute models keep the last step's local rows (and with them its autograd graph) on
        # the prepared batch, so eager steps on the default stream before the capture would leave parameter-gradient accumulators
        # bound to that stream for the capture to meet
        graph = bench.GraphStep(fn, params, graph=True)
        ms_graph = graph.time(a.steps, 3) if graph.graph is not None else float("nan")
        eager = bench.GraphStep(fn, params, graph=False)
        ms_eager = eager.time(a.steps, 3)
        kernels = bench.traced_steps(eager.eager, 3, lib)
        rows.append((name, ms_eager, ms_graph, kernels))
        del graph

    print("config-3 shape: S-icews0515 (%d entities, D = %d), BiGRRGCN --rec-only-last-layer, L = %d, bsz %d, fixed draws, own gates"
          % (w["num_ents"], w["D"], w["L"], w["bsz"]))
    print("device: %s" % torch.cuda.get_device_name(0))
    for name, ms_eager, ms_graph, _ in rows:
        print("%-28s eager %.3f ms/step   hip-graph replay %.3f ms/step" % (name, ms_eager, ms_graph))
    (_, e_e, g_e, _), (_, e_a, g_a, _) = rows
    print("post-aggregation / post-ensemble: eager %.3f, graph replay %.3f" % (e_a / e_e, g_a / g_e))
    for name, _, _, kernels in rows:
        tot_ms = sum(v["ms_per_step"] for v in kernels.values())
        tot_n = sum(v["launches_per_step"] for v in kernels.values())
        print("\n%s: library kernels of one eager step (median of 3 traced steps): %d launches, %.3f ms" % (name, round(tot_n), tot_ms))
        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"]):
            print("  %-28s %4d launches  %8.4f ms" % (k, round(v["launches_per_step"]), v["ms_per_step"]))


if __name__ == "__main__":
    main()
