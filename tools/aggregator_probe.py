"""The frozen-ensemble loss kernel (temp_frozen_mix_ce: the candidate lists scored straight from two tables, loss rows and d_w in one
launch) against the composed route on the existing kernels, and the Aggregator training step on its two routes, in one process.

  kernel   (a) per shape, device time of
             fused     backend.frozen_mix_ce                                                    1 launch, nothing of size (P, N)
             composed  linear_multi x 2 (two (P, N) score matrices), gather_ce_mix_fwd, gather_ce_mix_bwd (two (P, N) gradient
                       matrices, which frozen streams throw away)
           at the S-icews14 step (B = 8 windows of N = 7 128 entities, 400 query rows each, C = 101, D = 128 and 200) and at
           N = 2^19 (one window, the largest P whose pair of (P, N) matrices fits in 60 % of the free device memory and stays
           under 2^31 elements per matrix, the size up to which the composed route is tested: P = 3 072).  temp_gather_ce_mix_bwd
           keeps N counters in LDS and refuses N > 40 704, so at 2^19 the composed arm is its forward alone -- the comparison then favours it.
           Protocol: warm-up, then rounds that alternate the arms (a disturbance of the shared machine hits both), each round the
           device-event time of `reps` back-to-back calls (200 at the small shape: windows of 10 - 60 ms), the host time to issue a
           call printed next to it; median and range (smallest - largest round) per arm.  Verdict per shape:
           the fused arm is "faster beyond the range" when median(composed) - median(fused) exceeds the composed arm's own range.
  step     (b) one Aggregator training step (frozen StaticRGCN + BiGRRGCN, fresh parameters, fixed samples, eager launches), the
           one-node route against the per-graph literal route, steps interleaved, median and range.

    python tools/aggregator_probe.py [--out profiles/aggregator_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import synthetic  # noqa: E402
from temp_amd.aggregator import Aggregator  # noqa: E402
from temp_amd.backend import get_backend  # noqa: E402
from tools.hyte_probe import timed  # noqa: E402


def probe_kernel(B, N, rows_per_window, C, D, rounds, reps, device, say):
    be = get_backend()
    g = torch.Generator(device="cpu").manual_seed(N + D)
    P = B * rows_per_window
    mk = lambda n, d: (torch.randn(n, d, generator=g) * d ** -0.25).to(device)
    q_a, q_b, T_a, T_b = mk(P, D), mk(P, D), mk(B * N, D), mk(B * N, D)
    w = torch.sigmoid(torch.randn(P, generator=g)).to(device)
    cand = torch.randint(0, N, (P, C), generator=g).int().to(device)
    window = torch.arange(B, dtype=torch.int32, device=device).repeat_interleave(rows_per_window)
    cand_abs = (cand + window.view(-1, 1) * N).contiguous()
    scale = torch.full((P,), 1.0 / rows_per_window, device=device)
    one = torch.ones(1, device=device)
    s_a, s_b = (torch.empty(P, N, device=device) for _ in range(2))
    # (the per-window operand views are made once, outside the timed calls)
    qs_a, qs_b = ([q[b * rows_per_window:(b + 1) * rows_per_window] for b in range(B)] for q in (q_a, q_b))
    Ts_a, Ts_b = ([T[b * N:(b + 1) * N] for b in range(B)] for T in (T_a, T_b))
    with_bwd = N * 4 <= 160 * 1024 - 1024

    def fused():
        return be.frozen_mix_ce(q_a, T_a, q_b, T_b, w, cand_abs, scale, None, "dot")

    def composed():
        be.linear_multi(qs_a, Ts_a, True, s_a)
        be.linear_multi(qs_b, Ts_b, True, s_b)
        loss, lse = be.gather_ce_mix_fwd(s_a, s_b, w, cand)
        if not with_bwd:
            return loss, None
        return loss, be.gather_ce_mix_bwd(s_a, s_b, w, cand, lse, one, 1.0, scale)[2]

    lf, df = fused()
    lc, dc = composed()
    err_l = float((lf - lc).abs().max())
    err_d = float((df - dc).abs().max()) if dc is not None else float("nan")
    for _ in range(2):
        timed(fused, reps)
        timed(composed, reps)
    t = {"fused": [], "composed": []}
    for _ in range(rounds):
        t["fused"].append(timed(fused, reps))
        t["composed"].append(timed(composed, reps))
    say("\nkernel: B = %d, N = %d, P = %d rows, C = %d, D = %d; composed arm %s; |loss rows fused - composed| <= %.3g, |d_w| <= %.3g"
        % (B, N, P, C, D, "forward + backward" if with_bwd else "FORWARD ONLY (temp_gather_ce_mix_bwd refuses this N)", err_l, err_d))
    # host time of issuing one call (no synchronisation inside): an arm whose device time is close to it is host-bound
    import time
    host = {}
    for k, fn in (("fused", fused), ("composed", composed)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        host[k] = (time.perf_counter() - t0) / reps
        torch.cuda.synchronize()
    say("  host time to issue one call: fused %.1f us, composed %.1f us" % (host["fused"] * 1e6, host["composed"] * 1e6))
    for k, v in t.items():
        say("  %-9s median %10.1f us   range %10.1f - %10.1f us   (%d rounds x %d calls)" % (k, np.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6, rounds, reps))
    gain = float(np.median(t["composed"]) - np.median(t["fused"]))
    spread = float(max(t["composed"]) - min(t["composed"]))
    faster = gain > spread
    gathered = 2.0 * P * C * D * 4
    say("  fused / composed = %.3f of the medians; difference %.1f us against the composed arm's range of %.1f us: fused is %s beyond the range"
        % (np.median(t["fused"]) / np.median(t["composed"]), gain * 1e6, spread * 1e6, "FASTER" if faster else "not faster"))
    say("  fused gathers %.1f MB of table rows -> %.2f TB/s" % (gathered / 1e6, gathered / float(np.median(t["fused"])) / 1e12))
    return faster


def probe_step(D, steps, warm, device, say):
    w = dict(synthetic.workload("S-icews14", seed=0), D=D, B=D)
    args = bench.make_args(w, "Aggregator")
    args.negative_rate, args.score_function = 100, "distmult"
    torch.manual_seed(1)
    snaps = w["snapshots"]
    model = Aggregator(args, w["num_ents"], w["num_rels"], snaps, snaps, snaps).to(device)          # (debug: fresh StaticRGCN + BiGRRGCN)
    ts = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 3)
    samples = [model.corrupter.single_graph_negative_sampling(t, snaps[t], w["num_ents"])[:3] for t in sorted(ts, reverse=True)]
    params = [p for p in model.parameters() if p.requires_grad]

    def step(fused):
        def run():
            model.fused_loss = fused
            return model(ts, samples=samples)
        return bench.GraphStep(run, params, graph=False)
    variants = [("one-node route (temp_frozen_mix_ce)", step(True)), ("per-graph literal route", step(False))]
    for _ in range(warm):
        for _, st in variants:
            st.eager()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(steps):
        for k, (_, st) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.eager()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    say("\nstep: Aggregator on S-icews14 at D = %d: N = %d, batch %d, %d negatives, %d query rows; loss %.6f / %.6f"
        % (D, w["num_ents"], len(ts), args.negative_rate, 2 * sum(s[0].shape[0] for s in samples), float(variants[0][1].out), float(variants[1][1].out)))
    for (what, _), tm in zip(variants, times):
        say("  %-38s median %8.3f ms/step   range %.3f - %.3f   (%d steps, both frozen encoders included)" % (what, np.median(tm), min(tm), max(tm), len(tm)))
    say("  one-node / literal = %.3f of the medians" % (np.median(times[0]) / np.median(times[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aggregator_probe needs the GPU: nothing here is measured without one")
    device = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events, arms alternating round by round" % torch.cuda.get_device_name(0))
    verdicts = {}
    for D in (128, 200):
        verdicts["S-icews14, D = %d" % D] = probe_kernel(8, 7128, 400, 101, D, 7, 200, device, say)
    # N = 2^19: the largest P (a multiple of 1 024) whose pair of (P, N) score matrices fits in 60 % of the memory that is free now
    # AND whose matrices stay under 2^31 elements: no test of the composed route's products and candidate passes goes past that
    # size, and a probe is not where an index overflow on a shared device should first show.  That bound is the binding one
    # (P = 3 072, 6.4 GB per matrix); the fused kernel has no (P, N) operand and no such bound.
    N_big = 1 << 19
    free = torch.cuda.mem_get_info()[0]
    P_big = max(1024, min(int(0.6 * free / (2 * N_big * 4)), ((1 << 31) - 1) // N_big) // 1024 * 1024)
    say("\nN = 2^19: %.1f GB free, two (P, N) matrices of %.1f GB each (under 2^31 elements) -> P = %d" % (free / 1e9, P_big * N_big * 4 / 1e9, P_big))
    verdicts["N = 2^19, P = %d, D = 128" % P_big] = probe_kernel(1, N_big, P_big, 101, 128, 5, 3, device, say)
    say("\nverdict: " + "; ".join("%s: %s" % (k, "fused faster beyond the range" if v else "fused NOT faster") for k, v in verdicts.items()))
    probe_step(128, a.steps, 3, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
