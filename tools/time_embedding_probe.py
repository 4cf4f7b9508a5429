#!/usr/bin/env python3
"""--use-time-embedding on the headline shape: the training step through the one-launch GRU chain (the time embedding as the
chain's state offset, batched all-entity pass, fused loss) against `use_gru_chain = False` (the per-position loop with an eager
add per position).

    python tools/time_embedding_probe.py [--out profiles/time_embedding_probe.txt] [--steps 20] [--warmup 5] [--limit 240]

bench.py's headline configuration (temp_amd.synthetic S-gdelt: BiGRRGCN, L = 15, bsz = 8, D = 200) with use_time_embedding = True;
eager step on one resident batch: encoder + loss + backward + Adam, every step device-synchronised.  Each path runs in a child
process of its own under its own time limit (`--limit` seconds); a child that fails or runs out of time ends the probe."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_path(chain, steps, warmup):
    import numpy as np
    import torch
    import bench
    from temp_amd import _lib, synthetic
    from temp_amd.sampling import CorruptTriples
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    w = synthetic.workload("S-gdelt", seed=0)
    real = bench.make_args
    bench.make_args = lambda *p, **k: argparse.Namespace(**dict(vars(real(*p, **k)), use_time_embedding=True))
    try:
        model = bench.build_model(w, dev)
    finally:
        bench.make_args = real
    model.train()
    model.use_gru_chain = chain
    model.sample_rng = np.random.default_rng(2)
    model.corrupter = CorruptTriples(model.args, w["snapshots"], seed=5)
    opt = model.configure_optimizers()
    assert model._can_chain() == chain
    wb = model.prepare(synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0), w["L"], True)
    assert (wb.program is not None) == chain and model._fused_all_entity_ok(wb)

    def step():
        loss = model.run_loss(wb)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    c0 = lib.temp_gru_chain_offset_launches()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    assert (lib.temp_gru_chain_offset_launches() - c0 == 2 * warmup) if chain else (lib.temp_gru_chain_offset_launches() == c0)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    n, ms, top = bench.launches_of(lambda: (opt.zero_grad(set_to_none=True), model.run_loss(wb).backward()), lib)
    print(json.dumps(dict(path="chain" if chain else "per-position", median_ms=float(np.median(ts)), p10=float(np.percentile(ts, 10)),
                          p90=float(np.percentile(ts, 90)), loss=float(loss), launches=n, kernel_ms=ms,
                          top=["%s x%d %.3f ms" % (k, v["launches"], v["ms"]) for k, v in top.items()],
                          shape="L = %d, bsz = %d, D = %d" % (w["L"], w["bsz"], w["D"]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_embedding_probe.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each path's child process, seconds")
    ap.add_argument("--path", choices=("chain", "per-position"), help="(child) run this path and print its JSON line")
    a = ap.parse_args()
    if a.path:
        return run_path(a.path == "chain", a.steps, a.warmup)
    res = []
    for path in ("chain", "per-position"):
        cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)      # (a fresh child: nothing of a failed run is reused)
        if p.returncode != 0:
            sys.exit("time_embedding_probe: the %s run ended with status %d; nothing more is started" % (path, p.returncode))
        res.append(json.loads(p.stdout.strip().splitlines()[-1]))
    lines = ["use_time_embedding = True, S-gdelt (BiGRRGCN, %s), eager training step on one resident batch (encoder + loss + backward + Adam), "
             "%d synchronised steps after %d warm-up, each path in its own process" % (res[0]["shape"], a.steps, a.warmup)]
    for r in res:
        lines.append("%-13s median %.3f ms  (p10 %.3f  p90 %.3f)  loss %.6f  library launches per step %d (%.3f ms of kernels)"
                     % (r["path"], r["median_ms"], r["p10"], r["p90"], r["loss"], r["launches"], r["kernel_ms"]))
        lines.append("              " + "  ".join(r["top"]))
    lines.append("per-position / chain = %.2f" % (res[1]["median_ms"] / res[0]["median_ms"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
