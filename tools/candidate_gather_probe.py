#!/usr/bin/env python
"""The two routes of a bilinear scorer's sampled loss next to each other, in one process: "gemm" (scores against ALL entities of a
window, temp_linear_multi + temp_gather_ce_* on the (rows, N) matrix) and "gather" (the candidates alone, temp_dot_ce_* /
temp_dot_mix_ce_* straight from the all-entity stack; link_loss.bilinear_route).

  node     forward + backward of one loss node on a synthetic loss plan with a fixed candidate matrix (the slot lists of the gather
           route are sorted once, as with injected samples), device time; "gather, fresh" hands the node a new candidate tensor
           every call, so the stable sort of the slot lists is inside the time (what a training step with fresh negatives pays).
  kernels  the scorer's candidate stage alone on a given query: gemm = linear_multi, gather_ce_fwd | gather_ce_bwd, linear_multi,
           linear_tn_multi; gather = dot_ce_fwd | dot_ce_bwd_q, dot_ce_bwd_table (slot lists given).
  Shape A  an ICEWS14 step: B = 8 windows of N = 7 128 entities, 400 rows each = 3 200 rows, C = 101, D = 128 and 200, ComplEx;
           the plain node at both widths, the gated node at D = 128.
  Shape B  N = 2^19 in one window, 3 072 rows, C = 101, D = 128: "gather" forward + backward; temp_gather_ce_bwd refuses N > 40 704,
           so the only arm "gemm" has there is its forward (a 6.4 GB score matrix).
  Protocol: warm-up, then rounds that alternate the arms, each round the device-event time of `reps` back-to-back calls; median
  and range (smallest - largest round) per arm.  No pass bar: the figures decide whether a later change makes "gather" the default
  below the ceiling.

    python tools/candidate_gather_probe.py [--out profiles/candidate_gather_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd import functional as TF  # noqa: E402
from temp_amd import link_loss as LL  # noqa: E402
from temp_amd.backend import get_backend  # noqa: E402
from tools.all_entity_loss_probe import N_REL, make_plan, rounds_of  # noqa: E402

C = 101


def inputs(B, N, rows_per_window, D, device):
    g = torch.Generator(device="cpu").manual_seed(N + D)
    plan = make_plan(B, N, rows_per_window, device, N + D)
    P = B * rows_per_window
    cand = torch.randint(0, N, (P, C), generator=g).int()
    cand[:, 0] = plan["truth"].cpu()
    plan["cand"] = cand.to(device)
    leaf = lambda n: (torch.randn(n, D, generator=g) * D ** -0.25).to(device).requires_grad_(True)
    return plan, P, leaf, g


def ratio(say, med, a, b):
    say("  %s / %s = %.3f of the medians" % (a, b, med[a] / med[b]))


def probe_plain(B, N, rows_per_window, D, rounds, reps, device, say, gemm_backward=True):
    be = get_backend()
    plan, P, leaf, g = inputs(B, N, rows_per_window, D, device)
    ent, rel, big = leaf(B * N), leaf(N_REL), leaf(B * N)
    say("\nplain node: B = %d, N = %d, %d rows, C = %d, D = %d, complex" % (B, N, P, C, D))

    def node(route, fresh=False):
        def run():
            inp = dict(plan, cand=plan["cand"].clone()) if fresh else plan
            TF.batched_link_prediction(ent, rel, big, "complex", inp, route=route).backward()
        return run

    def gemm_forward():
        with torch.no_grad():
            TF.batched_link_prediction(ent, rel, big, "complex", plan, route="gemm")
    if gemm_backward:
        med = rounds_of({"node gemm": node("gemm"), "node gather": node("gather"), "node gather, fresh": node("gather", True)}, rounds, reps, say)
        ratio(say, med, "node gather", "node gemm")
        ratio(say, med, "node gather, fresh", "node gemm")
    else:
        med = rounds_of({"node gemm FORWARD only": gemm_forward, "node gather": node("gather"), "node gather, fresh": node("gather", True)},
                        rounds, reps, say)
        say("  (no gemm backward: temp_gather_ce_bwd keeps N counters in LDS and refuses N > 40 704)")
        ratio(say, med, "node gather", "node gemm FORWARD only")

    # the candidate stage alone
    with torch.no_grad():
        q = be.bilinear_query_fwd("complex", ent, plan["known"], rel, plan["rel"], plan["is_tail"])
        one = torch.ones(1, device=device)
        bigd = big.detach()
        scorers = {r: LL._scorer("complex", plan, bigd, r) for r in ("gemm", "gather")}

        def stage(route, backward=True):
            sc = scorers[route]

            def run():
                _, saved = sc.ce_fwd(be, q, bigd)
                if backward:
                    sc.ce_bwd(be, q, bigd, saved, one)
            return run
        if gemm_backward:
            med = rounds_of({"kernels gemm": stage("gemm"), "kernels gather": stage("gather")}, rounds, reps, say)
            ratio(say, med, "kernels gather", "kernels gemm")
        else:
            med = rounds_of({"kernels gemm FORWARD only": stage("gemm", False), "kernels gather": stage("gather")}, rounds, reps, say)
            ratio(say, med, "kernels gather", "kernels gemm FORWARD only")
        moved = 4.0 * P * C * D * 3                                                    # the candidate rows: read by fwd and bwd_q; q rows per slot
        say("  the gather kernels read about %.0f MB of candidate and query rows -> %.2f TB/s over their median"
            % (moved / 1e6, moved / med["kernels gather"] / 1e12))


def probe_gated(B, N, rows_per_window, D, rounds, reps, device, say):
    plan, P, leaf, g = inputs(B, N, rows_per_window, D, device)
    plan = TF.gated_loss_inputs(plan, B * N, device)
    loc, rec, rel, big_loc, big_rec = leaf(B * N), leaf(B * N), leaf(N_REL), leaf(B * N), leaf(B * N)
    wk, wc = (torch.rand(P, 1, generator=g).to(device).requires_grad_(True) for _ in range(2))
    say("\ngated node: B = %d, N = %d, %d rows, C = %d, D = %d, complex" % (B, N, P, C, D))

    def node(route):
        def run():
            TF.batched_gated_link_prediction(loc, rec, rel, big_loc, big_rec, wk, wc, "complex", plan, route=route).backward()
        return run
    med = rounds_of({"node gemm": node("gemm"), "node gather": node("gather")}, rounds, reps, say)
    ratio(say, med, "node gather", "node gemm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("candidate_gather_probe needs the GPU: nothing here is measured without one")
    device = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events, arms alternating round by round" % torch.cuda.get_device_name(0))
    for D in (128, 200):
        probe_plain(8, 7128, 400, D, 7, 20, device, say)
    probe_gated(8, 7128, 400, 128, 7, 20, device, say)
    probe_plain(1, 1 << 19, 3072, 128, 5, 3, device, say, gemm_backward=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
