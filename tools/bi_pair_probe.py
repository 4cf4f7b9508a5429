#!/usr/bin/env python3
"""--module BiRRGCN --rec-only-last-layer with the union pair pass (BiDynamicRGCN.bi_pair_pass): the row operator of its centre position
and pair rows (functional.lin_step_rows2; temp_lin_rows2_fwd / _bwd) against the composition of the row operators, and the training
step with the attribute on against off.

    python tools/bi_pair_probe.py [--out profiles/bi_pair_probe.txt] [--rounds 7] [--reps 5] [--warmup 3]

The S-icews14 shape (temp_amd.synthetic) with bsz = 8, L = 15, D = 128 and 200, self-loop dropout 0 and 0.1 (the reference's default).
One process; per width and dropout one model, one prepared batch per arm, the negatives drawn once and fixed; the step is encoder +
all-entity pass + loss + backward, eager launches, timed with device events.  Two arms alternate round by round (a round = `reps`
steps of one arm):
    on    bi_pair_pass = True: the centre and the union pair rows one lin_step_rows2 node each, the batched all-entity pass, the
          fused loss
    off   bi_pair_pass = False: the centre on the per-row operators, the all-entity pass per window, the loss per graph (the route of
          profiles/lin_chain_probe.txt's `chain` arm; the baseline)
Reported per arm: the median and the smallest and largest round (ms per step) and the library launches of one step.

Kernel part: lin_step_rows2 forward + backward with the kernel and with LIN_ROWS_KERNEL = False, alternating, at the step's own
pair-row count (x gathered through x_rows from one row per entity) and centre-row count (x_rows None)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lin_stack_probe import timed_rounds  # noqa: E402

ARMS = (("on", True), ("off", False))


def run_shape(D, dropout, a, lib):
    import numpy as np
    import torch
    import bench
    from temp_amd import synthetic
    from temp_amd.sampling import CorruptTriples
    dev = torch.device("cuda", 0)
    w = dict(synthetic.workload("S-icews14", seed=0), D=D, B=128 if D == 128 else D // 2, L=15, bsz=8, module="BiRRGCN")
    model = bench.build_model(w, dev, dropout=dropout)
    model.train()
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    arms = {}
    for name, on in ARMS:
        model.bi_pair_pass = on
        model.sample_rng = np.random.default_rng(2)
        wb = model.prepare(targets, w["L"], True)
        assert wb.batched and wb.program is not None and bool(model._fused_all_entity_ok(wb)) == on
        samples = model._samples_from_plan(wb) if getattr(wb, "loss_plan", None) is not None else model.draw_samples(wb)
        arms[name] = (on, wb, samples)
    params = [p for p in model.parameters()]

    def step(name):
        on, wb, samples = arms[name]
        model.bi_pair_pass = on
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
        assert lib.temp_lin_chain_launches() - c0 == 2 * a.warmup
        launches[name] = bench.launches_of(lambda: step(name), lib)[0]
    times = timed_rounds({name: (lambda name=name: step(name)) for name, _ in ARMS}, a.rounds, a.reps)
    wb = arms["on"][1]
    model.bi_pair_pass = True
    m = model._all_maps(wb)[0]
    f, b = m["idx_f_host"] >= 0, m["idx_b_host"] >= 0
    lines = ["BiRRGCN, S-icews14 shape, bsz = %d, L = %d, D = %d (%d bases), dropout %.1f: encoder + all-entity pass + loss + backward, fixed "
             "negatives; %d centre rows, %d union pair rows (%d forward only, %d backward only, %d both)"
             % (w["bsz"], w["L"], D, w["B"], dropout, wb.target.n_rows, m["n_prev"], int((f & ~b).sum()), int((~f & b).sum()), int((f & b).sum()))]
    for name, _ in ARMS:
        t = times[name]
        lines.append("  %-4s median %8.3f ms   smallest round %8.3f   largest %8.3f   library launches per step %4d   loss %.6f%s"
                     % (name, float(np.median(t)), min(t), max(t), launches[name], losses[name], "  (its own masks)" if dropout else ""))
    ok = float(np.median(times["on"])) < min(times["off"])
    lines.append("  on median below the off arm's smallest round: %s   (off / on = %.2f)"
                 % ("yes" if ok else "NO", float(np.median(times["off"]) / np.median(times["on"]))))
    n_hist = [int(wb.program.inst[i].n) for i in wb.hist_inst]
    return lines, ok, (int(m["n_prev"]), int(wb.target.n_rows), w["num_ents"], n_hist)


def run_rows(n, d, n_x, n_hist, gathered, a):
    """lin_step_rows2 forward + backward at n rows: the kernel against the composition, alternating.  gathered: x has n_x rows read
    through x_rows (the pair rows); else x has n rows and x_rows is None (the centre)."""
    import numpy as np
    import torch
    from temp_amd import functional as TF
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    g = torch.Generator().manual_seed(4)
    leaf = lambda r, c, s: (torch.randn(r, c, generator=g) * s).to(dev).requires_grad_(True)
    x = leaf(n_x if gathered else n, d, 0.5)
    Hf, Hb = leaf(n_hist[0], d, 0.5), leaf(n_hist[1], d, 0.5)
    Wf, Wb = leaf(d, d, d ** -0.5), leaf(d, d, d ** -0.5)
    rows, invs = [], []
    for r in n_hist:                                        # about a third of the rows without a state in that direction
        h = np.where(rng.random(n) < 0.35, -1, rng.integers(0, r, n)).astype(np.int32)
        rows.append(torch.from_numpy(h).to(dev))
        invs.append(TF.gather_inverse(h, r, dev))
    xr = rng.integers(0, n_x, n).astype(np.int32) if gathered else None
    x_rows = torch.from_numpy(xr).to(dev) if gathered else None
    x_inv = TF.gather_inverse(xr, n_x, dev) if gathered else None
    dts = [torch.from_numpy(rng.integers(1, 15, n).astype(np.float32)).to(dev).view(-1, 1) for _ in range(2)]
    up = torch.randn(n, d, generator=g).to(dev)

    def call(kernel):
        old, TF.LIN_ROWS_KERNEL = TF.LIN_ROWS_KERNEL, kernel
        try:
            for t in (x, Hf, Hb, Wf, Wb):
                t.grad = None
            out = TF.lin_step_rows2(x, x_rows, Hf, rows[0], dts[0], Hb, rows[1], dts[1], 0.1, Wf, Wb, 1, x_inv, invs[0], invs[1])
            out.backward(up)
        finally:
            TF.LIN_ROWS_KERNEL = old
        return out

    assert TF.lin_rows2_usable(d)
    outs = {}
    for name, kernel in (("kernel", True), ("composition", False)):
        for _ in range(a.warmup):
            outs[name] = call(kernel).detach()
    err = float((outs["kernel"] - outs["composition"]).abs().max())
    times = timed_rounds({"kernel": lambda: call(True), "composition": lambda: call(False)}, a.rounds, 4 * a.reps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return ("  %-6s n = %6d d = %3d (Hf %d rows, Hb %d rows): kernel median %7.3f ms [%7.3f .. %7.3f]   composition %7.3f ms [%7.3f .. %7.3f]   "
            "composition / kernel = %.2f   max |out difference| %.2e"
            % ("pairs" if gathered else "centre", n, d, n_hist[0], n_hist[1], med["kernel"], min(times["kernel"]), max(times["kernel"]),
               med["composition"], min(times["composition"]), max(times["composition"]), med["composition"] / med["kernel"], err)), \
        med["kernel"] < med["composition"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bi_pair_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from temp_amd import _lib
    lib = _lib.load()
    lines = ["two arms alternating round by round in one process: %d rounds of %d steps after %d warm-up steps each, device events"
             % (a.rounds, a.reps, a.warmup)]
    faster_step, shapes = True, {}
    for D in (128, 200):
        for dropout in (0.0, 0.1):
            part, ok, shape = run_shape(D, dropout, a, lib)
            lines += part
            faster_step = faster_step and ok
            shapes[D] = shape if dropout == 0.0 else shapes[D]
            print("\n".join(part), flush=True)
    lines.append("the on arm's median below the off arm's smallest round at every configuration: %s" % ("yes" if faster_step else "NO"))
    lines.append("lin_step_rows2 forward + backward (one autograd node, ReLU), kernel against LIN_ROWS_KERNEL = False, alternating: %d rounds of "
                 "%d calls" % (a.rounds, 4 * a.reps))
    faster = True
    for D in (128, 200):
        n_pairs, n_centre, n_ents, n_hist = shapes[D]
        for n, gathered in ((n_pairs, True), (n_centre, False)):
            line, ok = run_rows(n, D, n_ents, n_hist, gathered, a)
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
