"""The DE training step (`--module DE`, ComplEx, batch 8) with the table stack from the HIP node (functional.diachronic_rows: one
launch forward, one backward) against the SAME step with the table built from torch operators the way the reference builds it
(per timestamp: mul, add, sin, cat, mul -- kept here, not in the package), on the entity counts of bench.py's two ICEWS shapes at
D = 128 and 200.  The parent has no DE step, so the torch composition measured in the same process is the yardstick.

One prepared batch, fixed negatives, eager launches.  Timing: device events around every step, warm-up, the two variants
interleaved step by step, median and quartiles over --steps steps each.  Launches per step: the library's own trace (HIP events
around its kernels) and, for the launches torch makes itself, torch.profiler's device-kernel count of one step.  The two kernels'
bytes/s: 2 N d floats read + B N d written (forward), the mirror image backward, over the time of back-to-back launches between
two device events, against the 8.0 TB/s HBM3E peak and the 6.29 TB/s a float4 copy reaches.

    python tools/diachronic_probe.py [--workload S-icews14 S-icews0515] [--widths 128 200] [--steps 30] [--out profiles/diachronic_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd.backend import get_backend  # noqa: E402
from temp_amd.non_recurrent import DiachronicEmbedding  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


class TorchTableDE(DiachronicEmbedding):
    """The table as baselines/DiachronicEmbedding.py:22-28 composes it, once per timestamp."""

    def table_stack(self, times):
        ent = self.ent_embeds
        ones = ent.new_ones(ent.shape[0], self.static_embed_size)
        return torch.cat([ent * torch.cat((ones, torch.sin(times[b] * self.w_temp_ent_embeds + self.b_temp_ent_embeds)), dim=-1)
                          for b in range(times.shape[0])], dim=0)


def build(cls, w, D, device, targets):
    args = bench.make_args(w, "DE")
    args.embed_size = args.hidden_size = D
    torch.manual_seed(1)
    m = cls(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(device)
    m.sample_rng = np.random.default_rng(2)
    return m, m.prepare(targets)


def device_launches(step):
    """Device kernels of one step as torch.profiler counts them (every launch, the library's and torch's own), or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:                                   # the count is then reported as not measured
        print("  (torch.profiler: %s)" % exc)
        return None


def kernel_rates(m, wb, reps, say):
    """Back-to-back launches of each kernel between two device events -> time per launch, bytes/s, share of the stream bound."""
    be = get_backend()
    ent, w, b, t = m.ent_embeds.detach(), m.w_temp_ent_embeds.detach(), m.b_temp_ent_embeds.detach(), wb.fused["times"]
    N, d = ent.shape
    B = t.shape[0]
    d_out = torch.randn(B * N, d, device=ent.device)
    nbytes = (2 * N * d + B * N * d) * 4
    for what, fn in (("k_diachronic_fwd", lambda: be.diachronic_rows_fwd(ent, w, b, t)), ("k_diachronic_bwd", lambda: be.diachronic_rows_bwd(ent, w, b, t, d_out))):
        for _ in range(5):
            fn()
        per = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e-3 / reps)
        s = float(np.median(per))
        say("  %s (B = %d, N = %d, d = %d): %.2f us per launch (median of 5 x %d back-to-back), %.1f MB -> %.2f TB/s = %.0f %% of the 8.0 TB/s peak, "
            "%.0f %% of the 6.29 TB/s copy rate" % (what, B, N, d, s * 1e6, reps, nbytes / 1e6, nbytes / s / 1e12, 100 * nbytes / s / HBM_PEAK,
                                                     100 * nbytes / s / HBM_COPY))


def probe(name, D, steps, warm, lib, device, say):
    w = synthetic.workload(name, seed=0)
    targets = synthetic.default_targets(w["num_times"], 1, w["bsz"], 3)
    hip, wb = build(DiachronicEmbedding, w, D, device, targets)
    ref, wb_t = build(TorchTableDE, w, D, device, targets)
    ref.load_state_dict(hip.state_dict())
    with torch.no_grad():
        hip.run_loss(wb)
    cand = hip._last_plan[1]
    assert all(torch.equal(wb.fused["plan"][k], wb_t.fused["plan"][k]) for k in ("known", "rel", "truth")), "both models plan the same batch"
    variants = [("DE step, HIP table node", bench.GraphStep(lambda: hip.run_loss(wb, cand), list(hip.parameters()), graph=False)),
                ("DE step, table from torch operators", bench.GraphStep(lambda: ref.run_loss(wb_t, cand), list(ref.parameters()), graph=False))]
    for _ in range(warm):
        for _, st in variants:
            st.eager()
    torch.cuda.synchronize()
    diff = max(float((a.grad - b.grad).abs().max()) for a, b in zip(hip.parameters(), ref.parameters()))
    times = [[] for _ in variants]
    for _ in range(steps):                                   # interleaved: drift of the shared machine hits both variants alike
        for k, (_, st) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.eager()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    say("\n%s entities at D = %d: N = %d, %d relations, batch %d (times %s), %d negatives, ComplEx; loss %.6f / %.6f, largest gradient difference %.3g"
        % (name, D, w["num_ents"], w["num_rels"], len(targets), [int(t) for t in targets], hip.args.negative_rate, float(variants[0][1].out),
           float(variants[1][1].out), diff))
    for (what, _), ts in zip(variants, times):
        q = np.percentile(ts, [25, 50, 75])
        say("  %-38s median %.3f ms/step  (quartiles %.3f - %.3f, %d steps)" % (what, q[1], q[0], q[2], len(ts)))
    med = [float(np.median(ts)) for ts in times]
    say("  HIP node / torch operators = %.3f" % (med[0] / med[1]))
    for what, st in variants:
        kernels = bench.traced_steps(st.eager, 3, lib)
        tot_ms = sum(v["ms_per_step"] for v in kernels.values())
        tot_n = sum(v["launches_per_step"] for v in kernels.values())
        n_dev = device_launches(st.eager)
        say("  %s: %d library launches, %.3f ms in them (median of 3 traced steps); device kernels of one step by torch.profiler: %s"
            % (what, round(tot_n), tot_ms, "not measured" if n_dev is None else str(n_dev)))
        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])[:6]:
            say("    %-28s %4d launches  %8.4f ms" % (k, round(v["launches_per_step"]), v["ms_per_step"]))
    kernel_rates(hip, wb, 50, say)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["S-icews14", "S-icews0515"])
    ap.add_argument("--widths", nargs="+", type=int, default=[128, 200])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 (the median of fewer steps is not reported)")
    device = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events per step, variants interleaved" % torch.cuda.get_device_name(0))
    for name in a.workload:
        for D in a.widths:
            probe(name, D, a.steps, a.warmup, lib, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
