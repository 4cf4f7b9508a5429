"""The mixed selection of predict_gated() (temp_filtered_topk_mix: one launch over two [P, ld] score matrices and a weight per row)
against the route it replaces: the torch mix of the two matrices, w a + (1 - w) b as three elementwise operators (the leanest
eager form: no -inf masks, which the probe's operands do not need and evaluation.mixed_scores adds), the third matrix written and
read back, followed by temp_filtered_topk.  Shapes as in tools/topk_probe.py: evaluation-sized (P = 512,
N = 7128) and the large regime (P = 256, N = 2^19), both at k = 10.

Scores are seeded normal draws (ties negligible), the weights uniform in [0.05, 0.95), every row has a filter list of 8 random entities.
Both routes must name the same entities, and their values agree to the mix's rounding (the kernel's mix is one fmaf, torch's a
product more): checked before timing.  Timing: device events around `inner` back-to-back calls, warm-up, the routes interleaved
round by round, REPEATS rounds, the int64 conversion of the ids included; per call: median and min - max over the rounds.  The
fused route counts as faster only when the medians differ by more than the larger of the two routes' own min - max spread.
Bytes/s: 2 * P * ld * 4 (the one read of both matrices the selection needs) over the time per call, against the 8.0 TB/s HBM3E
peak and the 6.29 TB/s a float4 copy reaches.

    python tools/topk_mix_probe.py [--out profiles/topk_mix_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd.backend import get_backend  # noqa: E402
from tools.topk_probe import HBM_COPY, HBM_PEAK, REPEATS, timed  # noqa: E402

# (P, N, k, back-to-back calls per timed window)
SHAPES = [(512, 7128, 10, 50), (256, 1 << 19, 10, 5)]


def make_inputs(P, N, device, seed=0):
    g = torch.Generator().manual_seed(seed + P + N)
    ld = (N + 3) // 4 * 4
    mats = []
    for _ in range(2):
        s = torch.randn(P, ld, generator=g)
        s[:, N:] = float("-inf")
        mats.append(s.to(device))
    w = (0.05 + 0.9 * torch.rand(P, generator=g)).to(device)        # inside (0, 1): the pad columns' -inf stays -inf in the torch mix
    ids = torch.sort(torch.stack([torch.randperm(N, generator=g)[:8] for _ in range(P)]), dim=1).values
    ptr = (torch.arange(P + 1) * 8).int()
    return mats[0], mats[1], w, ptr.to(device), ids.reshape(-1).int().to(device)


def probe(P, N, k, inner, device, say):
    be = get_backend()
    a, b, w, ptr, ids = make_inputs(P, N, device)
    ld = a.shape[1]
    wc = w.view(-1, 1)
    routes = {"temp_filtered_topk_mix": lambda: be.filtered_topk_mix(a, b, w, k, ptr, ids, n=N),
              "torch mix + temp_filtered_topk": lambda: be.filtered_topk(wc * a + (1 - wc) * b, k, ptr, ids, n=N)}
    got, ref = routes["temp_filtered_topk_mix"](), routes["torch mix + temp_filtered_topk"]()
    assert torch.equal(got[1], ref[1]), "the two routes name different entities"
    assert torch.allclose(got[0], ref[0], rtol=0, atol=1e-5), "the two routes' values differ by more than the mix's rounding"
    t = timed(routes, inner)
    nbytes = 2 * P * ld * 4
    say("\nP = %d, N = %d (ld %d), k = %d: 2 x %.1f MB of scores; both routes name the same answers" % (P, N, ld, k, nbytes / 2e6))
    stat = {}
    for name, ts in t.items():
        med, lo, hi = float(np.median(ts)), min(ts), max(ts)
        stat[name] = (med, hi - lo)
        say("  %-31s median %9.1f us per call  (min - max %9.1f - %9.1f over %d x %d calls)  %6.2f TB/s = %4.1f %% of the 8.0 TB/s peak, %4.1f %% of the copy rate"
            % (name, med * 1e6, lo * 1e6, hi * 1e6, REPEATS, inner, nbytes / med / 1e12, 100 * nbytes / med / HBM_PEAK, 100 * nbytes / med / HBM_COPY))
    (f, sf), (c, sc) = stat["temp_filtered_topk_mix"], stat["torch mix + temp_filtered_topk"]
    spread = max(sf, sc)
    verdict = "faster than" if c - f > spread else ("slower than" if f - c > spread else "within the spread of")
    say("  -> the fused route is %s the torch mix + plain selection: %.1f us against %.1f us, spread %.1f us (ratio %.2f)"
        % (verdict, f * 1e6, c * 1e6, spread * 1e6, f / c))


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
    for P, N, k, inner in SHAPES:
        probe(P, N, k, inner, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
