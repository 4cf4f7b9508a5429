#!/usr/bin/env python3
"""--module RRGCN / BiRRGCN (the linear recurrence) at window level: the training step on the one-launch linear chain against the
per-position loop of the batched path and against the reference-granular path.

    python tools/lin_chain_probe.py [--out profiles/lin_chain_probe.txt] [--rounds 7] [--reps 5] [--warmup 3]

The S-icews14 shape (temp_amd.synthetic) with bsz = 8, L = 15 and D = 128 and 200, --rec-only-last-layer.  One process; per module
and width one model, one prepared batch per arm, the negatives drawn once and fixed; the step is encoder + all-entity pass + loss +
backward, eager launches, timed with device events.  Three arms alternate round by round (a round = `reps` steps of one arm):
    chain          the linear_chain node (temp_lin_chain_fwd / _bwd)
    per-position   use_lin_chain = False: the batched path with one linear_nt + decay_rows per position
    granular       use_batched_path = False: one encoder call per window position (the only route before the chain existed; the
                   reference for time)
Reported per arm: the median and the smallest and largest round (ms per step) and the library launches of one step."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = (("chain", dict(use_batched_path=True, use_lin_chain=True)), ("per-position", dict(use_batched_path=True, use_lin_chain=False)),
        ("granular", dict(use_batched_path=False, use_lin_chain=False)))


def run_shape(module, D, a, lib):
    import numpy as np
    import torch
    import bench
    from temp_amd import synthetic
    from temp_amd.sampling import CorruptTriples
    dev = torch.device("cuda", 0)
    w = dict(synthetic.workload("S-icews14", seed=0), D=D, B=128 if D == 128 else D // 2, L=15, bsz=8, module=module)
    model = bench.build_model(w, dev)
    model.train()
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    arms = {}
    for name, flags in ARMS:
        for k, v in flags.items():
            setattr(model, k, v)
        model.sample_rng = np.random.default_rng(2)
        wb = model.prepare(targets, w["L"], True)
        assert wb.batched == flags["use_batched_path"] and (wb.program is not None) == (name == "chain")
        samples = model._samples_from_plan(wb) if getattr(wb, "loss_plan", None) is not None else model.draw_samples(wb)
        arms[name] = (dict(flags), wb, samples)
    params = [p for p in model.parameters()]

    def step(name):
        flags, wb, samples = arms[name]
        for k, v in flags.items():
            setattr(model, k, v)
        for p in params:
            p.grad = None
        loss = model.run_loss(wb, samples)
        loss.backward()
        return loss

    losses, launches = {}, {}
    for name, _ in ARMS:
        c0 = lib.temp_lin_chain_launches()
        for _ in range(a.warmup):
            losses[name] = float(step(name).detach())
        torch.cuda.synchronize()
        assert (lib.temp_lin_chain_launches() - c0 == 2 * a.warmup) == (name == "chain")
        launches[name] = bench.launches_of(lambda: step(name), lib)[0]
    times = {name: [] for name, _ in ARMS}
    for _ in range(a.rounds):
        for name, _ in ARMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.reps)
    lines = ["%s, S-icews14 shape, bsz = %d, L = %d, D = %d (%d bases): encoder + all-entity pass + loss + backward, fixed negatives"
             % (module, w["bsz"], w["L"], D, w["B"])]
    for name, _ in ARMS:
        t = times[name]
        lines.append("  %-13s median %8.3f ms   smallest round %8.3f   largest %8.3f   library launches per step %4d   loss %.6f"
                     % (name, float(np.median(t)), min(t), max(t), launches[name], losses[name]))
    ok = float(np.median(times["chain"])) < min(times["granular"])
    lines.append("  chain median below the granular arm's smallest round: %s   (granular / chain = %.2f, per-position / chain = %.2f)"
                 % ("yes" if ok else "NO", float(np.median(times["granular"]) / np.median(times["chain"])),
                    float(np.median(times["per-position"]) / np.median(times["chain"]))))
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lin_chain_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from temp_amd import _lib
    lib = _lib.load()
    lines = ["three arms alternating round by round in one process: %d rounds of %d steps after %d warm-up steps each, device events"
             % (a.rounds, a.reps, a.warmup)]
    accept = True
    for module in ("RRGCN", "BiRRGCN"):
        for D in (128, 200):
            part, ok = run_shape(module, D, a, lib)
            lines += part
            accept = accept and ok
            print("\n".join(part), flush=True)
    lines.append("accepted (the chain arm's median below the granular arm's smallest round at every shape): %s" % ("yes" if accept else "NO"))
    text = "\n".join(lines) + "\n"
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
