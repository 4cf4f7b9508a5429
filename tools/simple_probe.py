"""The pair table pass (functional.pair_rows: temp_pair_rows_fwd / _bwd) against torch's cat + expand and its autograd, in one process,
and the fused SimplE training step (`--module Simple`, batch 8) against the per-graph literal route.  The parent has no SimplE step,
so what is measured in the same run is the yardstick.

  pair     one (N, d) table pair for B = 8 windows, forward and backward, at the ICEWS14 entity shape (N = 7128, d = 128) and at
           N = 2^19: device time per pass (device events around back-to-back passes, the two variants interleaved round by round),
           median and the run-to-run range (smallest - largest round), device kernels per pass (torch.profiler), whether both sides
           give the same bits, and the HIP kernels' bytes/s against the 8.0 TB/s HBM3E peak and the 6.29 TB/s a float4 copy reaches.
           Bytes: the HIP forward reads 2 N d and writes 2 B N d floats, the backward reads 2 B N d and writes 2 N d; torch's cat
           writes 2 N d more and reads them back B times, its adjoint also copies both halves out of their narrow views.
           Three comparisons per direction: the full ranges (HIP's slowest round under torch's fastest), the quartiles (HIP's upper
           under torch's lower) and the rounds as pairs (the two sides of a round run back to back, so a disturbance of the shared
           machine that lasts a round slows both: in how many rounds HIP was the faster).  The verdict "faster beyond the run-to-run
           ranges" asks for disjoint quartile ranges AND every paired round; the full ranges are reported next to it.
  step     one prepared batch of bench.py's S-icews14 workload, fixed negatives, eager launches, device events per step, variants
           interleaved step by step, median and quartiles: the fused step (pair tables from the HIP pass, and from torch's
           composition) and the per-graph literal route (scores.simple_pair over gathered (P, 1 + negatives, 2 D) candidates) on
           the same samples.

    python tools/simple_probe.py [--widths 128] [--steps 30] [--out profiles/simple_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd import functional as TF  # noqa: E402
from temp_amd.non_recurrent import SimplE  # noqa: E402
from tools.hyte_probe import device_launches, timed  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def hip_rows(a, a_inv, B):
    return TF._PairRowsFn.apply(a, a_inv, B)


class TorchPairSimplE(SimplE):
    """Both pair tables from torch operators."""

    def table_stack(self, times):
        return TF.pair_rows_torch(self.ent_embeds, self.ent_embeds_inv, times.shape[0])

    def relation_stack(self, times):
        return TF.pair_rows_torch(self.rel_embeds, self.rel_embeds_inv, 1)


def probe_pair(B, N, d, rounds, reps, device, say):
    g = torch.Generator(device="cpu").manual_seed(N + d)
    mk = lambda *s: torch.randn(*s, generator=g).to(device)
    a, a_inv, g_out = mk(N, d), mk(N, d), mk(B * N, 2 * d)
    sides = {}
    for side, rows in (("HIP pass", hip_rows), ("torch cat + expand", TF.pair_rows_torch)):
        leaves = [x.clone().requires_grad_(True) for x in (a, a_inv)]
        out = rows(leaves[0], leaves[1], B)

        def bwd(leaves=leaves, out=out):
            for x in leaves:
                x.grad = None
            torch.autograd.backward((out,), (g_out,), retain_graph=True)

        def fwd_nograd(leaves=leaves, rows=rows):
            with torch.no_grad():
                return rows(leaves[0], leaves[1], B)

        bwd()
        sides[side] = dict(fwd=fwd_nograd, bwd=bwd, out=out.detach(), grads=[x.grad.clone() for x in leaves], t_fwd=[], t_bwd=[])
    for s in sides.values():
        for _ in range(3):
            s["fwd"]()
            s["bwd"]()
    torch.cuda.synchronize()
    for _ in range(rounds):                                      # interleaved: drift of the shared machine hits both sides alike
        for s in sides.values():
            s["t_fwd"].append(timed(s["fwd"], reps))
            s["t_bwd"].append(timed(s["bwd"], reps))
    h, t = sides["HIP pass"], sides["torch cat + expand"]
    same_out = bool(torch.equal(h["out"], t["out"]))
    diff_g = max(float((x - y).abs().max()) for x, y in zip(h["grads"], t["grads"]))
    say("\npair: B = %d, N = %d, d = %d (rows of %d floats); forward bit-equal: %s; largest gradient difference HIP - torch %.3g"
        % (B, N, d, 2 * d, "yes" if same_out else "NO", diff_g))
    for side, s in sides.items():
        nf, nb = device_launches(s["fwd"]), device_launches(s["bwd"])
        qf, qb = np.percentile(s["t_fwd"], [25, 75]) * 1e6, np.percentile(s["t_bwd"], [25, 75]) * 1e6
        say("  %-20s forward %9.2f us (quartiles %.2f - %.2f, range %.2f - %.2f, %s device kernels), backward %9.2f us (quartiles %.2f - %.2f, "
            "range %.2f - %.2f, %s device kernels); %d rounds x %d passes"
            % (side, np.median(s["t_fwd"]) * 1e6, qf[0], qf[1], min(s["t_fwd"]) * 1e6, max(s["t_fwd"]) * 1e6, nf,
               np.median(s["t_bwd"]) * 1e6, qb[0], qb[1], min(s["t_bwd"]) * 1e6, max(s["t_bwd"]) * 1e6, nb, rounds, reps))
    verdict = {}
    for what, key in (("forward", "t_fwd"), ("backward", "t_bwd")):
        full = max(h[key]) < min(t[key])
        quart = np.percentile(h[key], 75) < np.percentile(t[key], 25)
        paired = sum(1 for x, y in zip(h[key], t[key]) if x < y)
        verdict[what] = bool(quart and paired == rounds)
        say("  %s: HIP / torch = %.3f of the medians; full ranges %s, quartile ranges %s, HIP the faster in %d of %d paired rounds: %s beyond the ranges"
            % (what, np.median(h[key]) / np.median(t[key]), "disjoint" if full else "OVERLAP", "disjoint" if quart else "OVERLAP", paired, rounds,
               "faster" if verdict[what] else "not faster"))
    by = (2 * N * d + 2 * B * N * d) * 4
    for what, key in (("forward (k_pair_rows_fwd)", "t_fwd"), ("backward (k_pair_rows_bwd)", "t_bwd")):
        tm = float(np.median(h[key]))
        say("  HIP %s: %.1f MB -> %.2f TB/s = %.0f %% of the 8.0 TB/s peak, %.0f %% of the 6.29 TB/s copy rate"
            % (what, by / 1e6, by / tm / 1e12, 100 * by / tm / HBM_PEAK, 100 * by / tm / HBM_COPY))
    return verdict


def build(cls, w, D, device, targets):
    args = bench.make_args(w, "DE")
    args.module = "Simple"
    args.embed_size = args.hidden_size = D
    torch.manual_seed(1)
    m = cls(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(device)
    with torch.no_grad():                       # the init's ~0.04 entries give scores of 1e-4: a loss of log(1 + negatives) and no signal
        for p in m.parameters():
            p.mul_(8.0)
    m.sample_rng = np.random.default_rng(2)
    return m, m.prepare(targets)


def plan_samples(m):
    plan, cand = m._last_plan
    out = []
    for trip, (a0, _) in zip(plan["triples"], plan["splits"]):
        P = trip.shape[0]
        out.append((torch.from_numpy(trip).to(cand.device), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))
    return out


def probe_step(name, D, steps, warm, lib, device, say):
    w = synthetic.workload(name, seed=0)
    targets = synthetic.default_targets(w["num_times"], 1, w["bsz"], 3)
    hip, wb = build(SimplE, w, D, device, targets)
    ref, wb_t = build(TorchPairSimplE, w, D, device, targets)
    lit, _ = build(SimplE, w, D, device, targets)
    for m in (ref, lit):
        m.load_state_dict(hip.state_dict())
    lit.fused_loss = False                                      # every graph through scores.simple_pair
    with torch.no_grad():
        hip.run_loss(wb)
    cand = hip._last_plan[1]
    samples = plan_samples(hip)
    assert all(torch.equal(wb.fused["plan"][k], wb_t.fused["plan"][k]) for k in ("known", "rel", "truth")), "both models plan the same batch"
    variants = [("SimplE fused step, HIP pair pass", bench.GraphStep(lambda: hip.run_loss(wb, cand), list(hip.parameters()), graph=False)),
                ("SimplE fused step, pair tables from torch", bench.GraphStep(lambda: ref.run_loss(wb_t, cand), list(ref.parameters()), graph=False)),
                ("SimplE per-graph literal route", bench.GraphStep(lambda: lit(targets, samples=samples), list(lit.parameters()), graph=False))]
    for _ in range(warm):
        for _, st in variants:
            st.eager()
    torch.cuda.synchronize()
    diffs = [max(float((a.grad - b.grad).abs().max()) for a, b in zip(hip.parameters(), m.parameters())) for m in (ref, lit)]
    times = [[] for _ in variants]
    for _ in range(steps):
        for k, (_, st) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.eager()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    say("\nstep: %s at D = %d (pair rows of %d): N = %d, %d relations, batch %d, %d negatives; loss %.6f / %.6f / %.6f; largest gradient difference "
        "to the HIP fused step: torch pair tables %.3g, literal route %.3g"
        % (name, D, 2 * D, w["num_ents"], w["num_rels"], len(targets), hip.args.negative_rate, float(variants[0][1].out), float(variants[1][1].out),
           float(variants[2][1].out), diffs[0], diffs[1]))
    for (what, _), ts in zip(variants, times):
        q = np.percentile(ts, [25, 50, 75])
        say("  %-44s median %8.3f ms/step  (quartiles %.3f - %.3f, range %.3f - %.3f, %d steps)" % (what, q[1], q[0], q[2], min(ts), max(ts), len(ts)))
    med = [float(np.median(ts)) for ts in times]
    say("  fused HIP / fused torch tables = %.3f;  fused HIP / literal = %.3f" % (med[0] / med[1], med[0] / med[2]))
    what, st = variants[0]
    kernels = bench.traced_steps(st.eager, 3, lib)
    tot_ms = sum(v["ms_per_step"] for v in kernels.values())
    tot_n = sum(v["launches_per_step"] for v in kernels.values())
    say("  %s: %d library launches, %.3f ms in them (median of 3 traced steps); device kernels of one step by torch.profiler: %s"
        % (what, round(tot_n), tot_ms, device_launches(st.eager)))
    for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])[:10]:
        say("    %-28s %4d launches  %8.4f ms" % (k, round(v["launches_per_step"]), v["ms_per_step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", nargs="+", type=int, default=[128])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 (the median of fewer steps is not reported)")
    if not torch.cuda.is_available():
        raise SystemExit("simple_probe needs the GPU: nothing here is measured without one")
    device = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events, variants interleaved" % torch.cuda.get_device_name(0))
    v_small = probe_pair(8, 7128, 128, 15, 200, device, say)
    v_big = probe_pair(8, 1 << 19, 128, 9, 10, device, say)
    both = all(v_small.values()) and all(v_big.values())
    say("\nverdict: the HIP pass is %s than torch's composition beyond the run-to-run ranges at both shapes, both ways"
        % ("faster" if both else "NOT faster"))
    for D in a.widths:
        probe_step("S-icews14", D, a.steps, a.warmup, lib, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
