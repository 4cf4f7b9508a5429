"""The selection pass of predict() (temp_filtered_topk, one launch over a [P, ld] score matrix) against the two routes a user has
without it: torch.topk on the ALREADY MASKED matrix (the yardstick: it leaves ties arbitrary and the masking is not counted) and
evaluation.topk_composite (mask + stable sort, the contract in torch operators).  Shapes: evaluation-sized (P = 512, N = 7128,
k = 10) and the large regime (P = 256, N = 2^19, k = 10 and 100), the latter also carried over column panels of 2^16.

Scores are seeded normal draws (ties negligible, so all three routes must name the same entities: checked before timing); every row
has a filter list of 8 random entities.  Timing: device events around `inner` back-to-back calls, warm-up, the routes interleaved
round by round, REPEATS rounds; per call: median and min - max over the rounds.  A route is called slower only when the medians
differ by more than the larger of the two routes' own min - max spread.  Bytes/s: P * ld * 4 (the one read of the matrix the
selection needs) over the time per call, against the 8.0 TB/s HBM3E peak and the 6.29 TB/s a float4 copy reaches.

    python tools/topk_probe.py [--out profiles/topk_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd.backend import get_backend  # noqa: E402
from temp_amd.evaluation import topk_composite  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
REPEATS = 7
# (P, N, k, panel columns or None, back-to-back calls per timed window)
SHAPES = [(512, 7128, 10, None, 50), (256, 1 << 19, 10, None, 5), (256, 1 << 19, 10, 1 << 16, 5), (256, 1 << 19, 100, None, 5),
          (256, 1 << 19, 100, 1 << 16, 5)]


_INPUTS = {}


def inputs(P, N, device, seed=0):
    if (P, N) not in _INPUTS:
        _INPUTS.clear()                                            # one shape's matrices at a time
        _INPUTS[(P, N)] = _make_inputs(P, N, device, seed)
    return _INPUTS[(P, N)]


def _make_inputs(P, N, device, seed):
    g = torch.Generator().manual_seed(seed + P + N)
    ld = (N + 3) // 4 * 4
    scores = torch.randn(P, ld, generator=g)
    scores[:, N:] = float("-inf")
    ids = torch.sort(torch.stack([torch.randperm(N, generator=g)[:8] for _ in range(P)]), dim=1).values
    ptr = (torch.arange(P + 1) * 8).int()
    masked = scores.clone()
    masked[torch.arange(P).view(-1, 1), ids] = float("-inf")
    return scores.to(device), masked.to(device), ptr.to(device), ids.reshape(-1).int().to(device)


def timed(routes, inner):
    """{name: [seconds per call] * REPEATS}, the routes interleaved round by round."""
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in routes}
    for _ in range(REPEATS):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e-3 / inner)
    return out


def probe(P, N, k, panel, inner, device, say):
    be = get_backend()
    scores, masked, ptr, ids = inputs(P, N, device)
    ld = scores.shape[1]

    def hip():
        if panel is None:
            return be.filtered_topk(scores, k, ptr, ids, n=N)
        carry = None
        for c0 in range(0, N, panel):
            carry = be.filtered_topk(scores[:, c0:], k, ptr, ids, col0=c0, n=min(N, c0 + panel) - c0, carry=carry)
        return carry

    routes = {"temp_filtered_topk": hip, "torch.topk (masked)": lambda: torch.topk(masked, k, dim=1),
              "topk_composite": lambda: topk_composite(scores, k, ptr, ids, n=N)}
    got, ref, lib = hip(), topk_composite(scores, k, ptr, ids, n=N), torch.topk(masked, k, dim=1)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0]), "kernel != composite"
    assert torch.equal(got[0], lib.values), "kernel != torch.topk"
    t = timed(routes, inner)
    nbytes = P * ld * 4
    say("\nP = %d, N = %d (ld %d), k = %d, %s: %.1f MB of scores; the three routes name the same answers"
        % (P, N, ld, k, "one launch" if panel is None else "%d carried panels of %d columns" % (-(-N // panel), panel), nbytes / 1e6))
    stat = {}
    for name, ts in t.items():
        med, lo, hi = float(np.median(ts)), min(ts), max(ts)
        stat[name] = (med, hi - lo)
        say("  %-22s median %9.1f us per call  (min - max %9.1f - %9.1f over %d x %d calls)  %6.2f TB/s = %4.1f %% of the 8.0 TB/s peak, %4.1f %% of the copy rate"
            % (name, med * 1e6, lo * 1e6, hi * 1e6, REPEATS, inner, nbytes / med / 1e12, 100 * nbytes / med / HBM_PEAK, 100 * nbytes / med / HBM_COPY))
    (a, sa), (b, sb) = stat["temp_filtered_topk"], stat["torch.topk (masked)"]
    spread = max(sa, sb)
    verdict = "slower than" if a - b > spread else ("faster than" if b - a > spread else "within the spread of")
    say("  -> the kernel is %s torch.topk: %.1f us against %.1f us, spread %.1f us (ratio %.2f)" % (verdict, a * 1e6, b * 1e6, spread * 1e6, a / b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; device events around back-to-back calls, routes interleaved, %d rounds" % (torch.cuda.get_device_name(0), REPEATS))
    for P, N, k, panel, inner in SHAPES:
        probe(P, N, k, panel, inner, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
