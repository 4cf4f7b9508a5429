#!/usr/bin/env python3
"""The S-gdelt training step with the TransE loss: the fused L1 nodes (temp_l1_ce_fwd / _bwd_q / _bwd_table) against
fused_loss = False (the tensor path: (P, 1 + neg, D) gathers per direction and target graph), same model, same box, same run --
step time over resident batches (eager: encoder + loss + backward + Adam), peak allocated memory of a step, and one evaluate()
call through temp_l1_scores against the chunked broadcast route.  REPEATS timed passes each; a route is called slower only when
its best pass is slower than the other's worst.  python tools/transe_probe.py [steps] [num_pos_facts]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import backend as TB  # noqa: E402
from temp_amd import link_loss as LL  # noqa: E402
from temp_amd import scores as SC  # noqa: E402
from temp_amd import synthetic  # noqa: E402
from temp_amd.evaluation import EvaluationFilter  # noqa: E402
from temp_amd.sampling import CorruptTriples  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
num_pos = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
REPEATS, WARM, RESIDENT = 3, 3, 4
w = synthetic.workload("S-gdelt", seed=0)
dev = torch.device("cuda:0")


class NoL1:
    """Backend view without the L1 kernels: the chunked evaluation route."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name in LL._L1_METHODS:
            raise AttributeError(name)
        return getattr(self._be, name)


def build():
    model = bench.build_model(w, dev)
    model.args.score_function, model.calc_score = "transE", SC.transE
    model.args.num_pos_facts = num_pos
    model.train()
    model.sample_rng = np.random.default_rng(2)
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)      # (fused_loss = False plans no loss: it draws per graph)
    return model


def train_times(fused):
    model = build()
    model.fused_loss = fused                               # False: the tensor path with its per-graph sampler, as before the L1 kernels
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
    return out, peak


def eval_times():
    model = build()
    model.eval()
    model.evaluater = EvaluationFilter(model.args, model.calc_score, w["snapshots"], w["snapshots"], w["snapshots"])
    t_list = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 7)
    be = TB.get_backend()
    res = {}
    for name, backend in (("l1_scores", be), ("chunked", NoL1(be))):
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
print("S-gdelt, transE, num_pos_facts %d, negative_rate %d, D %d, %d windows; %d steps per pass, %d passes" %
      (num_pos, bench.make_args(w, w["module"]).negative_rate, w["D"], w["bsz"], steps, REPEATS))
f, fp = train_times(True)
u, up = train_times(False)
print("training step, fused L1 loss     : %s ms/step   peak allocated above the resident state %.0f MB" % (fmt(f), fp / 2 ** 20))
print("training step, fused_loss = False: %s ms/step   peak allocated above the resident state %.0f MB" % (fmt(u), up / 2 ** 20))
print("  -> " + verdict(f, u, "the fused step", "the unfused step"))
ev = eval_times()
print("evaluate(), temp_l1_scores route : %s ms" % fmt(ev["l1_scores"][0]))
print("evaluate(), chunked broadcast    : %s ms" % fmt(ev["chunked"][0]))
print("  -> " + verdict(ev["l1_scores"][0], ev["chunked"][0], "the l1_scores route", "the chunked route"))
a, b = ev["l1_scores"][1], ev["chunked"][1]
print("  ranks: %d rows, %d equal between the routes, max difference %d" % (a.numel(), int((a == b).sum()), int((a - b).abs().max()) if a.numel() else 0))
