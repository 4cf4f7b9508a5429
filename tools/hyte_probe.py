"""The hyperplane projection node (functional.hyperplane_rows: temp_hyperplane_rows_fwd / _bwd) against the torch composition of the
same projection, in one process, and the whole fused HyTE training step (`--module Hyte`, batch 8) with either.  The parent has no
HyTE step, so the torch composition measured in the same run is the yardstick; it is kept here, not in the package.

  tables   the two tables of a step (entities [N, D] and relations [2R, D], B = 8 time rows) forward and backward, at the ICEWS14
           shape (N = 7128, 2R = 460, D = 128 and 200) and at N = 2^19 (D = 128): device time per pass (device events around
           back-to-back passes, the two variants interleaved round by round, median over the rounds), device kernels per pass
           (torch.profiler), the largest difference between the two sides, whether d_w is bit-repeatable on each side, and the HIP
           kernels' bytes/s against the 8.0 TB/s HBM3E peak and the 6.29 TB/s a float4 copy reaches.  Bytes: forward N d read +
           B N d written; backward B N d + N d read, N d written, the tile partials (ceil(N / 32) B d) written and read once.
  step     one prepared batch of bench.py's S-icews14 workload, fixed negatives, eager launches, device events per step, variants
           interleaved step by step, median and quartiles; launches per step from the library's trace and torch.profiler.

    python tools/hyte_probe.py [--widths 128 200] [--steps 30] [--out profiles/hyte_probe.txt]
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
from temp_amd.non_recurrent import Hyte  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
TILE_ROWS = 32


def torch_rows(table, w):
    """baselines/Hyte.py:22-26 for B time rows at once: six element-wise and reduction operators over (B, N, D)."""
    n = w / torch.norm(w, p=2, dim=-1, keepdim=True)
    n = n.unsqueeze(1)
    t = table.unsqueeze(0)
    return (t - n * torch.sum(t * n, dim=-1, keepdim=True)).reshape(-1, table.shape[1])


class TorchTableHyte(Hyte):
    """Both stacks from torch operators."""

    def stacks(self, times):
        w = self.time_rows(times)
        return torch_rows(self.ent_embeds, w), torch_rows(self.rel_embeds, w)


def device_launches(step):
    """Device kernels of one call as torch.profiler counts them, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:
        print("  (torch.profiler: %s)" % exc)
        return None


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def probe_tables(N, R2, D, B, rounds, reps, device, say):
    g = torch.Generator(device="cpu").manual_seed(N + D)
    mk = lambda *s: torch.randn(*s, generator=g).to(device)
    ent, rel, w = mk(N, D), mk(R2, D), mk(B, D)
    g_ent, g_rel = mk(B * N, D), mk(B * R2, D)
    sides = {}
    for side, rows in (("HIP nodes", TF.hyperplane_rows), ("torch operators", torch_rows)):
        leaves = [x.clone().requires_grad_(True) for x in (ent, rel, w)]

        def fwd(leaves=leaves, rows=rows):
            return rows(leaves[0], leaves[2]), rows(leaves[1], leaves[2])

        outs = fwd()

        def bwd(leaves=leaves, outs=outs):
            for x in leaves:
                x.grad = None
            torch.autograd.backward(outs, (g_ent, g_rel), retain_graph=True)

        def fwd_nograd(leaves=leaves, rows=rows):
            with torch.no_grad():
                return rows(leaves[0], leaves[2]), rows(leaves[1], leaves[2])

        bwd()
        grads = [x.grad.clone() for x in leaves]
        bwd()
        sides[side] = dict(fwd=fwd_nograd, bwd=bwd, outs=[o.detach() for o in outs], grads=grads,
                           repeatable=bool(torch.equal(leaves[2].grad, grads[2])), t_fwd=[], t_bwd=[])
    for s in sides.values():
        for _ in range(3):
            s["fwd"]()
            s["bwd"]()
    torch.cuda.synchronize()
    for _ in range(rounds):                                      # interleaved: drift of the shared machine hits both sides alike
        for s in sides.values():
            s["t_fwd"].append(timed(s["fwd"], reps))
            s["t_bwd"].append(timed(s["bwd"], reps))
    a, b = sides["HIP nodes"], sides["torch operators"]
    diff_out = max(float((x - y).abs().max()) for x, y in zip(a["outs"], b["outs"]))
    diff_g = [float((x - y).abs().max()) for x, y in zip(a["grads"], b["grads"])]
    say("\ntables: entities N = %d, relation rows 2R = %d, D = %d, B = %d; largest difference HIP - torch: out %.3g, d_ent %.3g, d_rel %.3g, d_w %.3g "
        "(|d_w| up to %.3g)" % (N, R2, D, B, diff_out, diff_g[0], diff_g[1], diff_g[2], float(b["grads"][2].abs().max())))
    med = {}
    for side, s in sides.items():
        f, bw = float(np.median(s["t_fwd"])), float(np.median(s["t_bwd"]))
        med[side] = (f, bw)
        nf, nb = device_launches(s["fwd"]), device_launches(s["bwd"])
        say("  %-16s forward %8.2f us (%s device kernels), backward %8.2f us (%s device kernels); median of %d rounds x %d passes; "
            "d_w bit-repeatable: %s" % (side, f * 1e6, nf, bw * 1e6, nb, rounds, reps, "yes" if s["repeatable"] else "NO"))
    say("  HIP / torch: forward %.3f, backward %.3f" % (med["HIP nodes"][0] / med["torch operators"][0], med["HIP nodes"][1] / med["torch operators"][1]))
    rows_all = N + R2
    by_f = (rows_all * D + B * rows_all * D) * 4
    parts = (-(-N // TILE_ROWS) + -(-R2 // TILE_ROWS)) * B * D
    by_b = (B * rows_all * D + 2 * rows_all * D + 2 * parts) * 4
    for what, nbytes, t in (("forward (2 x k_hyperplane_fwd)", by_f, med["HIP nodes"][0]),
                            ("backward (2 x k_hyperplane_bwd + k_hyperplane_bwd_finish, autograd's sum of the two d_w)", by_b, med["HIP nodes"][1])):
        say("  HIP %s: %.1f MB -> %.2f TB/s = %.0f %% of the 8.0 TB/s peak, %.0f %% of the 6.29 TB/s copy rate"
            % (what, nbytes / 1e6, nbytes / t / 1e12, 100 * nbytes / t / HBM_PEAK, 100 * nbytes / t / HBM_COPY))


def build(cls, w, D, device, targets):
    args = bench.make_args(w, "DE")
    args.module = "Hyte"
    args.embed_size = args.hidden_size = D
    torch.manual_seed(1)
    m = cls(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(device)
    m.sample_rng = np.random.default_rng(2)
    return m, m.prepare(targets)


def probe_step(name, D, steps, warm, lib, device, say):
    w = synthetic.workload(name, seed=0)
    targets = synthetic.default_targets(w["num_times"], 1, w["bsz"], 3)
    hip, wb = build(Hyte, w, D, device, targets)
    ref, wb_t = build(TorchTableHyte, w, D, device, targets)
    ref.load_state_dict(hip.state_dict())
    with torch.no_grad():
        hip.run_loss(wb)
    cand = hip._last_plan[1]
    assert all(torch.equal(wb.fused["plan"][k], wb_t.fused["plan"][k]) for k in ("known", "rel", "truth")), "both models plan the same batch"
    variants = [("Hyte step, HIP projection nodes", bench.GraphStep(lambda: hip.run_loss(wb, cand), list(hip.parameters()), graph=False)),
                ("Hyte step, projections from torch operators", bench.GraphStep(lambda: ref.run_loss(wb_t, cand), list(ref.parameters()), graph=False))]
    for _ in range(warm):
        for _, st in variants:
            st.eager()
    torch.cuda.synchronize()
    diff = max(float((a.grad - b.grad).abs().max()) for a, b in zip(hip.parameters(), ref.parameters()))
    times = [[] for _ in variants]
    for _ in range(steps):
        for k, (_, st) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.eager()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    say("\nstep: %s at D = %d: N = %d, %d relations, batch %d, %d negatives, TransE; loss %.6f / %.6f, largest gradient difference %.3g"
        % (name, D, w["num_ents"], w["num_rels"], len(targets), hip.args.negative_rate, float(variants[0][1].out), float(variants[1][1].out), diff))
    for (what, _), ts in zip(variants, times):
        q = np.percentile(ts, [25, 50, 75])
        say("  %-46s median %.3f ms/step  (quartiles %.3f - %.3f, %d steps)" % (what, q[1], q[0], q[2], len(ts)))
    med = [float(np.median(ts)) for ts in times]
    say("  HIP nodes / torch operators = %.3f" % (med[0] / med[1]))
    for what, st in variants:
        kernels = bench.traced_steps(st.eager, 3, lib)
        tot_ms = sum(v["ms_per_step"] for v in kernels.values())
        tot_n = sum(v["launches_per_step"] for v in kernels.values())
        n_dev = device_launches(st.eager)
        say("  %s: %d library launches, %.3f ms in them (median of 3 traced steps); device kernels of one step by torch.profiler: %s"
            % (what, round(tot_n), tot_ms, "not measured" if n_dev is None else str(n_dev)))
        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])[:8]:
            say("    %-28s %4d launches  %8.4f ms" % (k, round(v["launches_per_step"]), v["ms_per_step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", nargs="+", type=int, default=[128, 200])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 (the median of fewer steps is not reported)")
    if not torch.cuda.is_available():
        raise SystemExit("hyte_probe needs the GPU: nothing here is measured without one")
    device = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events, variants interleaved" % torch.cuda.get_device_name(0))
    for D in a.widths:
        probe_tables(7128, 460, D, 8, 9, 50, device, say)
    probe_tables(1 << 19, 460, 128, 8, 7, 5, device, say)
    for D in a.widths:
        probe_step("S-icews14", D, a.steps, a.warmup, lib, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
