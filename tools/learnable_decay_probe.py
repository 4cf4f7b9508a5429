"""--learnable-lambda on the headline shape: the encoder step through the one-launch GRU chain against the per-position loop.

    python tools/learnable_decay_probe.py [--out profiles/learnable_decay_probe.txt] [--steps 20] [--rounds 3]

bench.py's headline configuration (temp_amd.synthetic S-gdelt: BiGRRGCN, L = 15, bsz = 8, D = 200) with learnable_lambda = True;
eager encoder forward + backward.  One model, two prepared batches of the same windows: `use_gru_chain` True (the chain kernels
with the device {w, b} pair) and False (the position loop of single-step GRU launches, what the flag ran before the chain took
it).  After a warm-up of both, `rounds` alternations of `steps` device-synchronised steps each; the file gets both medians, their
spread and the library launches of one step of each."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(bench.REPO, "profiles", "learnable_decay_probe.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    w = synthetic.workload("S-gdelt", seed=0)
    real = bench.make_args
    bench.make_args = lambda *p, **k: argparse.Namespace(**dict(vars(real(*p, **k)), learnable_lambda=True))
    try:
        model = bench.build_model(w, dev)
    finally:
        bench.make_args = real
    l2 = model.ent_encoder.layer_2
    with torch.no_grad():                                  # exp(-max(0.1 dt, 0)): the fixed decay's values, through the learnable path
        l2.exponential_decay.weight.fill_(0.1)
        l2.exponential_decay.bias.fill_(0.0)
    model.sample_rng = np.random.default_rng(2)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    steps = {}
    for name, chain in (("chain", True), ("per-position", False)):
        model.use_gru_chain = chain
        assert model._can_chain() == chain
        wb = model.prepare(targets, w["L"], train=True)
        assert (wb.program is not None) == chain
        steps[name] = bench.GraphStep(lambda wb=wb: model.run(wb)[0], list(model.parameters()), graph=False)
    c0 = lib.temp_gru_chain_decay_launches()
    for st in steps.values():
        for _ in range(a.warmup):
            st.eager()
    torch.cuda.synchronize()
    assert lib.temp_gru_chain_decay_launches() - c0 == 2 * a.warmup      # one forward + one backward chain launch per chain step, none from the loop
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name, st in steps.items():
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                st.eager()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            times[name].append(ts)
    lines = ["learnable_lambda = True, S-gdelt (BiGRRGCN, L = %d, bsz = %d, D = %d), eager encoder forward + backward, %d x %d synchronised steps each, alternating"
             % (w["L"], w["bsz"], w["D"], a.rounds, a.steps)]
    med = {}
    for name, rounds in times.items():
        allt = np.concatenate(rounds)
        med[name] = float(np.median(allt))
        n, ms, top = bench.launches_of(steps[name].eager, lib)
        lines.append("%-13s median %.3f ms  (round medians %s; p10 %.3f  p90 %.3f)  library launches per step %d (%.3f ms of kernels)"
                     % (name, med[name], " ".join("%.3f" % np.median(r) for r in rounds), np.percentile(allt, 10), np.percentile(allt, 90), n, ms))
        lines.append("              " + "  ".join("%s x%d %.3f ms" % (k, v["launches"], v["ms"]) for k, v in top.items()))
    lines.append("per-position / chain = %.2f" % (med["per-position"] / med["chain"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
