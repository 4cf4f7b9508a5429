"""The streamed filtered rank (temp_filtered_rank_stream / temp_filtered_rank_stream_mix) against the routes it stands beside, at the
selection probes' shapes: evaluation-sized (P = 512, N = 7128) and the large regime (P = 256, N = 2^19).

  plain   temp_filtered_rank against one TEMP_RANK_WHOLE call on the same matrix: both read the matrix once, so the expectation is
          "within the run-to-run spread";
  mixed   the torch mix w a + (1 - w) b (three elementwise operators, the mixed matrix written and read back) followed by
          temp_filtered_rank, against one TEMP_RANK_WHOLE call of the _mix entry, which streams the two matrices once: the
          expectation is that the kernel wins;
  panels  (2^19 only) what a two-table filter does per corruption mode -- two products of the folded query (D = 32) against the
          tables, the mix, the rank -- once on whole [P, N] matrices (calc_metrics_single_graph's panel=None) and once under
          panel="auto" (TOPK_PANEL_BYTES: a COLLECT sweep and a counting sweep, every panel scored twice, the mix in registers),
          with the peak of torch.cuda.max_memory_allocated above the inputs for both.

Scores are seeded normal draws (ties negligible), the gates uniform in [0.05, 0.95), every row has a filter list of 8 random
entities.  The routes of a comparison must return the same ranks up to the mix's rounding (plain: exactly): checked before timing.
Timing as tools/topk_probe.py: device events around `inner` back-to-back calls, warm-up, the routes interleaved round by round,
REPEATS rounds; per call: median and min - max over the rounds.  A route counts as faster only when the medians differ by more than
the larger of the two routes' own min - max spread.  Bytes/s: the one read of the score matrices the rank needs, P * ld * 4 (plain)
or twice that (mixed), over the time per call, against the 8.0 TB/s HBM3E peak and the 6.29 TB/s a float4 copy reaches.

    python tools/rank_stream_probe.py [--out profiles/rank_stream_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd import evaluation  # noqa: E402
from temp_amd.backend import get_backend  # noqa: E402
from tools.topk_probe import HBM_COPY, HBM_PEAK, REPEATS, timed  # noqa: E402

# (P, N, back-to-back calls per timed window)
SHAPES = [(512, 7128, 50), (256, 1 << 19, 5)]
D_PANELS = 32


def make_inputs(P, N, device, seed=0):
    g = torch.Generator().manual_seed(seed + P + N)
    ld = (N + 3) // 4 * 4
    mats = []
    for _ in range(2):
        s = torch.randn(P, ld, generator=g)
        s[:, N:] = float("-inf")
        mats.append(s.to(device))
    w = (0.05 + 0.9 * torch.rand(P, generator=g)).to(device)
    ids = torch.sort(torch.stack([torch.randperm(N, generator=g)[:8] for _ in range(P)]), dim=1).values
    ptr = (torch.arange(P + 1) * 8).int()
    target = torch.randint(0, N, (P,), generator=g).int()
    return mats[0], mats[1], w, target.to(device), ptr.to(device), ids.reshape(-1).int().to(device)


def report(say, stat, new, old, what):
    (f, sf), (c, sc) = stat[new], stat[old]
    spread = max(sf, sc)
    verdict = "faster than" if c - f > spread else ("slower than" if f - c > spread else "within the spread of")
    say("  -> %s is %s %s: %.1f us against %.1f us, spread %.1f us (ratio %.2f)" % (new, verdict, what, f * 1e6, c * 1e6, spread * 1e6, f / c))


def show(say, t, nbytes, inner):
    stat = {}
    for name, ts in t.items():
        med, lo, hi = float(np.median(ts)), min(ts), max(ts)
        stat[name] = (med, hi - lo)
        rate = "" if nbytes is None else "  %6.2f TB/s = %4.1f %% of the 8.0 TB/s peak, %4.1f %% of the copy rate" % (
            nbytes / med / 1e12, 100 * nbytes / med / HBM_PEAK, 100 * nbytes / med / HBM_COPY)
        say("  %-38s median %9.1f us per call  (min - max %9.1f - %9.1f over %d x %d calls)%s" % (name, med * 1e6, lo * 1e6, hi * 1e6, REPEATS, inner, rate))
    return stat


def close_ranks(got, ref, what):
    """Integer ranks of scores that differ by the mix's rounding: a swapped pair of near-equal scores moves a rank by one (the
    count is reported); anything gross is a different computation."""
    off = (got - ref).abs()
    assert int(off.max()) <= 16, "%s: the routes' ranks differ by up to %d" % (what, int(off.max()))


def probe_kernels(P, N, inner, device, say):
    be = get_backend()
    a, b, w, target, ptr, ids = make_inputs(P, N, device)
    ld = a.shape[1]
    wc = w.view(-1, 1)
    say("\nP = %d, N = %d (ld %d): %.1f MB per score matrix" % (P, N, ld, P * ld * 4 / 1e6))
    plain = {"temp_filtered_rank_stream (WHOLE)": lambda: be.filtered_rank_stream(a, target, ptr, ids, n=N)[0],
             "temp_filtered_rank": lambda: be.filtered_rank(a, target, ptr, ids)}
    got, ref = (fn() for fn in plain.values())
    assert torch.equal(got, ref), "the plain routes' ranks differ"
    say(" plain: both routes return the same ranks")
    stat = show(say, timed(plain, inner), P * ld * 4, inner)
    report(say, stat, "temp_filtered_rank_stream (WHOLE)", "temp_filtered_rank", "temp_filtered_rank")
    mixed = {"temp_filtered_rank_stream_mix (WHOLE)": lambda: be.filtered_rank_stream_mix(a, b, w, target, ptr, ids, n=N)[0],
             "torch mix + temp_filtered_rank": lambda: be.filtered_rank(wc * a + (1 - wc) * b, target, ptr, ids)}
    got, ref = (fn() for fn in mixed.values())
    close_ranks(got, ref, "mixed")
    say(" mixed: %d of %d ranks differ between the routes (the mix's rounding), by at most %d" % (int((got != ref).sum()), P, int((got - ref).abs().max())))
    stat = show(say, timed(mixed, inner), 2 * P * ld * 4, inner)
    report(say, stat, "temp_filtered_rank_stream_mix (WHOLE)", "torch mix + temp_filtered_rank", "the torch mix + temp_filtered_rank")


def probe_panels(P, N, inner, device, say):
    be = get_backend()
    g = torch.Generator().manual_seed(P + N)
    loc, rec = (torch.randn(N, D_PANELS, generator=g).mul_(0.5).to(device) for _ in range(2))
    q = torch.randn(P, D_PANELS, generator=g).to(device)
    _, _, w, target, ptr, ids = make_inputs(P, 8, device)
    target = torch.randint(0, N, (P,), generator=g).int().to(device)
    ids = (torch.randint(0, N // 8, (P, 1), generator=g) + torch.arange(8).view(1, 8) * (N // 8)).reshape(-1).int().to(device)     # unique, ascending
    wc = w.view(-1, 1)
    panel = evaluation._rank_panel("auto", P, N, 2)
    rank = evaluation._rank_mixed(be)
    produce = lambda c0, c1: (be.linear(q, loc[c0:c1], True), be.linear(q, rec[c0:c1], True), w)

    def whole():
        s_loc, s_rec = be.linear(q, loc, True), be.linear(q, rec, True)
        return be.filtered_rank(evaluation._pad4(wc * s_loc + (1 - wc) * s_rec), target, ptr, ids)

    def panelled():
        return evaluation._streamed_rank(rank, produce, N, panel, target, ptr, ids)

    routes = {"panel=\"auto\" (%d panels, two sweeps)" % ((N + panel - 1) // panel): panelled, "whole [P, N] matrices": whole}
    peaks, out = {}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out[name] = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    got, ref = out.values()
    close_ranks(got, ref, "panels")
    say("\nP = %d, N = %d, D = %d, two tables: one corruption mode of a two-table filter; TOPK_PANEL_BYTES = %d MiB -> panels of %d columns"
        % (P, N, D_PANELS, evaluation.TOPK_PANEL_BYTES >> 20, panel))
    say(" %d of %d ranks differ between the routes (the mix's rounding), by at most %d" % (int((got != ref).sum()), P, int((got - ref).abs().max())))
    stat = show(say, timed(routes, inner), None, inner)
    for name in routes:
        say("  %-38s peak of max_memory_allocated above the inputs: %8.1f MB" % (name, peaks[name] / 1e6))
    names = list(routes)
    report(say, stat, names[0], names[1], "the whole-matrix route")


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
    for P, N, inner in SHAPES:
        probe_kernels(P, N, inner, device, say)
    P, N, inner = SHAPES[-1]
    torch.cuda.empty_cache()
    probe_panels(P, N, inner, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
