#!/usr/bin/env python3
"""Development probe: per-position timeline of the two roles of k_gru_chain_fwd_x and k_gru_chain_bwd_hx (csrc/gru_chain_hx.hpp:
CHX_STAMP) on the S-gdelt batch of the bench.

    python tools/chain_phases.py [--block 0|1] [--positions N]

With a debug buffer set the chain launchers take the stamped (DEV = 1) instantiations of the headline kernels: lane 0 of the first
wave of each role writes the cycle counter at its barriers, at the end of its walks and around its gate passes, for the first panel
of block 0 and of the mid-grid block.  Printed per position, in cycles of the counter relative to the position's first stamp:
who reaches barriers A and B last and by how much, and what each role does in between.  One eager step is traced per kernel
(HIP events) with the stamps on, so the cycles convert to microseconds (the printed clock = panel cycles / kernel time; the
panel of a one-panel-per-CU launch spans the kernel)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from temp_amd import _lib, synthetic

EVENTS, MAX_STEPS = 8, 64
WORDS = 2 * 2 * 2 * MAX_STEPS * EVENTS            # CHX_STAMP_WORDS
HEAD = 8 * 4096                                   # DEBUG_EDGE_WORDS: the edge kernels' words in front (8 per block)
FWD = (("begin", "h walk done", "at A", "past A", "x walk done = at B", "past B"),
       ("begin", "x split done = at A", "past A", "x loads issued", "gates done = at B", "past B"))
BWD = (("at A", "past A", "walk done", "d_prev stored = at B", "past B"),
       ("gates begin", "gates done = at A", "past A", "prefetch issued = at B", "past B"))


def timeline(name, st, names, a_idx, b_idx, kernel_us, max_pos, reverse):
    """st: [role][position][event].  a_idx / b_idx: per role the event index of 'at A' / 'at B'."""
    used = np.nonzero(st[0, :, a_idx[0]])[0]
    if used.size == 0:
        print("%s: no stamps (the launch did not take the stamped instantiation)" % name)
        return
    order = used[::-1] if reverse else used
    t0 = min(int(st[r, order[0]][st[r, order[0]] != 0].min()) for r in (0, 1))
    t1 = max(int(st[r, order[-1]].max()) for r in (0, 1))
    span = t1 - t0
    ghz = span / (kernel_us * 1e3) if kernel_us else 0.0
    print("%s: %d positions, stamped span %d cycles; kernel %.1f us by HIP events -> %.2f cycles per ns" % (name, used.size, span, kernel_us, ghz))
    late_a, late_b = [], []
    for n, s in enumerate(order):
        mat, mem = st[0, s], st[1, s]
        base = min(int(mat[mat != 0].min()), int(mem[mem != 0].min()))
        la = int(mem[a_idx[1]]) - int(mat[a_idx[0]])          # > 0: the memory role reaches A after the matrix role
        lb = int(mem[b_idx[1]]) - int(mat[b_idx[0]])
        late_a.append(la)
        late_b.append(lb)
        if n < max_pos:
            print("  position %2d (+%7d)  A: memory role %+6d cycles behind the matrix role   B: %+6d" % (s, base - t0, la, lb))
            for r, role in enumerate(("matrix", "memory")):
                row = st[r, s]
                print("      %s  " % role + "  ".join("%s %d" % (nm, int(row[k]) - base) for k, nm in enumerate(names[r])))
    la, lb = np.array(late_a[1:-1] or late_a, dtype=np.float64), np.array(late_b[1:-1] or late_b, dtype=np.float64)
    per_pos = span / used.size
    print("  inner positions: the memory role is behind the matrix role at A by median %+.0f cycles (min %+.0f, max %+.0f), at B by median %+.0f (min %+.0f, max %+.0f); "
          "a position is %.0f cycles" % (np.median(la), la.min(), la.max(), np.median(lb), lb.min(), lb.max(), per_pos))
    exposed = np.clip(la, 0, None).sum() + np.clip(lb, 0, None).sum()
    print("  cycles the matrix role waits for the memory role at A and B, inner positions: %.0f of %d (%.1f %% of the span%s)"
          % (exposed, span, 100.0 * exposed / span, ", %.1f us" % (exposed / ghz / 1e3) if ghz else ""))
    # the intervals of each role, medians over the inner positions
    inner = order[1:-1] if order.size > 2 else order
    for r, role in enumerate(("matrix", "memory")):
        d = np.diff(st[r][inner][:, :len(names[r])].astype(np.int64), axis=1)
        print("      %s  medians: " % role + "  ".join("%s -> %s %d" % (names[r][k], names[r][k + 1], int(np.median(d[:, k]))) for k in range(d.shape[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=-1, help="0: block 0, 1: the mid-grid block, -1: both")
    ap.add_argument("--positions", type=int, default=4, help="positions printed stamp by stamp (the summary covers all)")
    opt = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    w = synthetic.workload("S-gdelt", seed=0)
    model = bench.build_model(w, dev)
    model.sample_rng = np.random.default_rng(2)
    wb = model.prepare(synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0), w["L"], train=True)
    step = bench.GraphStep(lambda: model.run(wb)[0], list(model.parameters()), graph=False)
    for _ in range(3):
        step.eager()
    torch.cuda.synchronize()
    buf = torch.zeros(HEAD + WORDS, dtype=torch.int64, device=dev)
    lib.temp_set_debug_buffer(buf.data_ptr(), HEAD + WORDS)
    try:
        step.eager()                                  # (the stamped instantiations' first launch: code-object load)
        torch.cuda.synchronize()
        buf.zero_()
        tr = bench.traced_steps(step.eager, 1, lib)
        torch.cuda.synchronize()
    finally:
        lib.temp_set_debug_buffer(None, 0)
    us = {k: 1e3 * v["avg_ms"] for k, v in tr.items() if "chain" in k.lower()}
    print("traced chain kernels (us per launch, stamps on):", ", ".join("%s %.1f" % kv for kv in sorted(us.items())))
    pick = lambda key: next((v for k, v in us.items() if key in k.lower()), 0.0)
    st = buf[HEAD:].cpu().numpy().reshape(2, 2, 2, MAX_STEPS, EVENTS)
    for blk in ((0, 1) if opt.block < 0 else (opt.block,)):
        where = "block 0" if blk == 0 else "mid-grid block"
        timeline("k_gru_chain_fwd_x, " + where, st[0, blk], FWD, (2, 1), (4, 4), pick("fwd"), opt.positions, False)
        timeline("k_gru_chain_bwd_hx, " + where, st[1, blk], BWD, (0, 1), (3, 3), pick("bwd"), opt.positions, True)


if __name__ == "__main__":
    main()
