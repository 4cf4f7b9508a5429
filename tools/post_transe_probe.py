#!/usr/bin/env python3
"""The S-gdelt training step of the post-aggregation model (PostBiDynamicRGCN, BiGRRGCN) with the TransE loss: the fused gated L1
node (temp_gated_query_* kind transE, temp_l1_mix_ce_fwd / _bwd_q / _bwd_table) against fused_loss = False (the tensor path:
per window and side two (P, 1 + neg, D) gathers, their mix and the broadcast difference), same model, same box, same run -- step
time over resident batches (eager: encoder + loss + backward + Adam), peak allocated memory of a step, and one evaluate() call
through temp_l1_mix_scores against PostEvaluationFilter's chunked route.  REPEATS timed passes each; a route is called slower only
when its best pass is slower than the other's worst.  The probe uses the public model API only, so it also runs on a tree
without the gated L1 kernels (both arms then take the tensor path).  A tensor-path arm that does not fit the card halves the
negative rate until it does and says so.

    python tools/post_transe_probe.py [steps] [num_pos_facts] [fused|both]      (fused: the fused arm alone, for a profiler run)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import backend as TB  # noqa: E402
from temp_amd import scores as SC  # noqa: E402
from temp_amd import synthetic  # noqa: E402
from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN  # noqa: E402
from temp_amd.sampling import CorruptTriples  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
num_pos = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
arms = sys.argv[3] if len(sys.argv) > 3 else "both"
REPEATS, WARM, RESIDENT = 3, 2, 4
w = synthetic.workload("S-gdelt", seed=0)
dev = torch.device("cuda:0")


class NoMixScores:
    """Backend view without temp_l1_mix_scores: PostEvaluationFilter's chunked literal route."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "l1_mix_scores":
            raise AttributeError(name)
        return getattr(self._be, name)


def build(negative_rate=None):
    args = bench.make_args(w, "BiGRRGCN")
    args.post_aggregation = True
    args.score_function = "transE"
    args.num_pos_facts = num_pos
    if negative_rate is not None:
        args.negative_rate = negative_rate
    torch.manual_seed(1)
    model = PostBiDynamicRGCN(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(dev)
    model.calc_score = SC.transE
    model.train()
    model.sample_rng = np.random.default_rng(2)
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)
    return model


def train_times(fused, negative_rate=None):
    model = build(negative_rate)
    model.fused_loss = fused
    opt = model.configure_optimizers()
    batches = [synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 1000 + r) for r in range(RESIDENT)]
    wbs = [model.prepare(b, w["L"], True) for b in batches]

    def one(i):
        loss = model.run_loss(wbs[i % RESIDENT])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    for i in range(WARM):
        one(i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    one(0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            one(i)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return out, peak, model.args.negative_rate


def tensor_path_times():
    """fused_loss = False at the workload's negative rate, or at the largest halving of it that fits the card."""
    rate = None
    while True:
        try:
            return train_times(False, rate)
        except torch.OutOfMemoryError:
            rate = (rate or bench.make_args(w, "BiGRRGCN").negative_rate) // 2
            torch.cuda.empty_cache()
            print("  (the tensor path does not fit the card; retrying with negative_rate %d)" % rate)
            if rate == 0:
                raise


def eval_times():
    model = build()
    model.eval()
    t_list = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 7)[:2]
    be = TB.get_backend()
    res = {}
    for name, backend in (("l1_mix_scores", be), ("chunked", NoMixScores(be))):
        TB.set_backend(backend)
        try:
            with torch.no_grad():
                ranks, _ = model.evaluate(t_list, val=True)          # (first call: filter lists, snapshot views)
                ts = []
                for _ in range(REPEATS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ranks, _ = model.evaluate(t_list, val=True)
                    torch.cuda.synchronize()
                    ts.append(1e3 * (time.perf_counter() - t0))
        finally:
            TB.set_backend(be)
        res[name] = (ts, ranks.cpu())
    return res


def verdict(a, b, what_a, what_b):
    if min(a) > max(b):
        return "%s is SLOWER than %s beyond the run-to-run spread" % (what_a, what_b)
    if max(a) < min(b):
        return "%s is faster than %s beyond the run-to-run spread" % (what_a, what_b)
    return "%s and %s are within the run-to-run spread" % (what_a, what_b)


fmt = lambda ts: "  ".join("%.2f" % t for t in ts)
has = hasattr(TB.get_backend(), "l1_mix_ce_fwd")
print("S-gdelt, PostBiDynamicRGCN (BiGRRGCN, --post-aggregation), transE, num_pos_facts %d, negative_rate %d, D %d, %d windows; "
      "%d steps per pass, %d passes; gated L1 kernels %s" %
      (num_pos, bench.make_args(w, "BiGRRGCN").negative_rate, w["D"], w["bsz"], steps, REPEATS, "present" if has else "ABSENT (both arms: tensor path)"))
f, fp, _ = train_times(True)
print("training step, fused gated L1 loss: %s ms/step   peak allocated above the resident state %.0f MB" % (fmt(f), fp / 2 ** 20))
if arms == "both":
    u, up, rate = tensor_path_times()
    print("training step, fused_loss = False : %s ms/step   peak allocated above the resident state %.0f MB   (negative_rate %d)"
          % (fmt(u), up / 2 ** 20, rate))
    print("  -> " + verdict(f, u, "the fused step", "the unfused step"))
    ev = eval_times()
    print("evaluate(), temp_l1_mix_scores route: %s ms" % fmt(ev["l1_mix_scores"][0]))
    print("evaluate(), chunked literal route   : %s ms" % fmt(ev["chunked"][0]))
    print("  -> " + verdict(ev["l1_mix_scores"][0], ev["chunked"][0], "the l1_mix_scores route", "the chunked route"))
    a, b = ev["l1_mix_scores"][1], ev["chunked"][1]
    print("  ranks: %d rows, %d equal between the routes, max difference %d"
          % (a.numel(), int((a == b).sum()), int((a - b).abs().max()) if a.numel() else 0))
