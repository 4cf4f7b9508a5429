#!/usr/bin/env python3
"""--module RRGCN with BOTH layers recurrent (the reference's grid flags: no --rec-only-last-layer) at window level: the training step on
the two-chain route (DynamicRGCN._run_lin_stack) against the reference-granular path, and the pair step of its all-entity pass
(temp_lin_rows_fwd / _bwd) against the composition of the row operators.

    python tools/lin_stack_probe.py [--out profiles/lin_stack_probe.txt] [--rounds 7] [--reps 5] [--warmup 3]

The S-icews14 shape (temp_amd.synthetic) with bsz = 8, L = 15, D = 128 and 200, self-loop dropout 0 and 0.1 (the reference's default).
One process; per width and dropout one model, one prepared batch per arm, the negatives drawn once and fixed; the step is encoder +
all-entity pass + loss + backward, eager launches, timed with device events.  Two arms alternate round by round (a round = `reps`
steps of one arm):
    stack      use_lin_stack = True: two linear_chain nodes over one program, the batched all-entity pass, the fused loss
    granular   use_lin_stack = False: one encoder call per window position and layer (what these flags ran before the route existed;
               the baseline)
Reported per arm: the median and the smallest and largest round (ms per step) and the library launches of one step.

Then functional.lin_step_rows forward + backward (layer 1's form: x rows gathered through x_rows) with the kernel and with
LIN_ROWS_KERNEL = False, alternating, at the step's own pair-row count and at 2^13, 2^15 and 2^17 rows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = (("stack", True), ("granular", False))


def timed_rounds(fns, rounds, reps):
    """fns: {name: callable}; the arms alternate round by round -> {name: [ms per call of every round]}."""
    import torch
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return times


def run_shape(D, dropout, a, lib):
    import numpy as np
    import torch
    import bench
    from temp_amd import synthetic
    from temp_amd.dynamic_rgcn import DynamicRGCN
    from temp_amd.sampling import CorruptTriples
    dev = torch.device("cuda", 0)
    w = dict(synthetic.workload("S-icews14", seed=0), D=D, B=128 if D == 128 else D // 2, L=15, bsz=8, module="RRGCN")
    args = bench.make_args(w, "RRGCN", dropout)
    args.rec_only_last_layer = False
    torch.manual_seed(1)
    model = DynamicRGCN(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(dev)
    model.train()
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    arms = {}
    for name, on in ARMS:
        model.use_lin_stack = on
        model.sample_rng = np.random.default_rng(2)
        wb = model.prepare(targets, w["L"], True)
        assert wb.batched == on and (wb.program is not None) == on and bool(model._fused_all_entity_ok(wb)) == on
        samples = model._samples_from_plan(wb) if getattr(wb, "loss_plan", None) is not None else model.draw_samples(wb)
        arms[name] = (on, wb, samples)
    params = [p for p in model.parameters()]

    def step(name):
        on, wb, samples = arms[name]
        model.use_lin_stack = on
        for p in params:
            p.grad = None
        loss = model.run_loss(wb, samples)
        loss.backward()
        return loss

    losses, launches = {}, {}
    for name, on in ARMS:
        c0 = lib.temp_lin_chain_launches()
        for _ in range(a.warmup):
            losses[name] = float(step(name).detach())
        torch.cuda.synchronize()
        assert lib.temp_lin_chain_launches() - c0 == (4 * a.warmup if on else 0)
        launches[name] = bench.launches_of(lambda: step(name), lib)[0]
    times = timed_rounds({name: (lambda name=name: step(name)) for name, _ in ARMS}, a.rounds, a.reps)
    wb = arms["stack"][1]
    n_pairs = int(model._all_maps(wb)[0]["n_prev"])
    lines = ["RRGCN, both layers recurrent, S-icews14 shape, bsz = %d, L = %d, D = %d (%d bases), dropout %.1f: encoder + all-entity pass + "
             "loss + backward, fixed negatives; %d node visits, %d pair rows in the all-entity pass"
             % (w["bsz"], w["L"], D, w["B"], dropout, wb.n_node_visits, n_pairs)]
    for name, _ in ARMS:
        t = times[name]
        lines.append("  %-9s median %8.3f ms   smallest round %8.3f   largest %8.3f   library launches per step %4d   loss %.6f%s"
                     % (name, float(np.median(t)), min(t), max(t), launches[name], losses[name], "  (its own masks)" if dropout else ""))
    ok = float(np.median(times["stack"])) < min(times["granular"])
    lines.append("  stack median below the granular arm's smallest round: %s   (granular / stack = %.2f)"
                 % ("yes" if ok else "NO", float(np.median(times["granular"]) / np.median(times["stack"]))))
    return lines, ok, n_pairs, w["num_ents"], int(wb.program.inst[wb.hist_inst].n)


def run_rows(n, d, n_x, n_h, a):
    """lin_step_rows forward + backward at n rows: the kernel against the composition, alternating."""
    import numpy as np
    import torch
    from temp_amd import functional as TF
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(n_x, d, generator=g) * 0.5).to(dev).requires_grad_(True)
    H = (torch.randn(n_h, d, generator=g) * 0.5).to(dev).requires_grad_(True)
    W = (torch.randn(d, d, generator=g) / d ** 0.5).to(dev).requires_grad_(True)
    xr, hr = rng.integers(0, n_x, n).astype(np.int32), rng.integers(0, n_h, n).astype(np.int32)
    x_rows, h_rows = torch.from_numpy(xr).to(dev), torch.from_numpy(hr).to(dev)
    x_inv, h_inv = TF.gather_inverse(xr, n_x, dev), TF.gather_inverse(hr, n_h, dev)
    dt = torch.from_numpy(rng.integers(1, 15, n).astype(np.float32)).to(dev).view(-1, 1)
    up = torch.randn(n, d, generator=g).to(dev)

    def call(kernel):
        old, TF.LIN_ROWS_KERNEL = TF.LIN_ROWS_KERNEL, kernel
        try:
            for t in (x, H, W):
                t.grad = None
            out = TF.lin_step_rows(x, x_rows, H, h_rows, dt, 0.1, W, 0, x_inv, h_inv)
            out.backward(up)
        finally:
            TF.LIN_ROWS_KERNEL = old
        return out

    assert TF.lin_rows_usable(d)
    outs = {}
    for name, kernel in (("kernel", True), ("composition", False)):
        for _ in range(a.warmup):
            outs[name] = call(kernel).detach()
    err = float((outs["kernel"] - outs["composition"]).abs().max())
    times = timed_rounds({"kernel": lambda: call(True), "composition": lambda: call(False)}, a.rounds, 4 * a.reps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return ("  n = %6d d = %3d (x %d rows, H %d rows): kernel median %7.3f ms [%7.3f .. %7.3f]   composition %7.3f ms [%7.3f .. %7.3f]   "
            "composition / kernel = %.2f   max |out difference| %.2e"
            % (n, d, n_x, n_h, med["kernel"], min(times["kernel"]), max(times["kernel"]), med["composition"], min(times["composition"]),
               max(times["composition"]), med["composition"] / med["kernel"], err)), med["kernel"] < med["composition"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lin_stack_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from temp_amd import _lib
    lib = _lib.load()
    lines = ["two arms alternating round by round in one process: %d rounds of %d steps after %d warm-up steps each, device events"
             % (a.rounds, a.reps, a.warmup)]
    accept, shapes = True, {}
    for D in (128, 200):
        for dropout in (0.0, 0.1):
            part, ok, n_pairs, n_ents, n_hist = run_shape(D, dropout, a, lib)
            lines += part
            accept = accept and ok
            shapes[D] = (n_pairs, n_ents, n_hist) if dropout == 0.0 else shapes[D]
            print("\n".join(part), flush=True)
    lines.append("accepted (the stack arm's median below the granular arm's smallest round at every shape): %s" % ("yes" if accept else "NO"))
    lines.append("lin_step_rows forward + backward (one autograd node; layer 1's form with x_rows), kernel against LIN_ROWS_KERNEL = False, "
                 "alternating: %d rounds of %d calls" % (a.rounds, 4 * a.reps))
    faster = True
    for D in (128, 200):
        n_pairs, n_ents, n_hist = shapes[D]
        for n in (n_pairs, 1 << 13, 1 << 15, 1 << 17):
            line, ok = run_rows(n, D, n_ents, n_hist, a)
            faster = faster and ok
            lines.append(line)
            print(line, flush=True)
    lines.append("kernel faster than the composition at every shape: %s" % ("yes" if faster else "NO"))
    text = "\n".join(lines) + "\n"
    print("\n".join(lines[-1:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
