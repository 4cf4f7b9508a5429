"""The all-entity ("1-vs-all") loss node (functional.batched_all_entity_link_prediction: temp_filtered_ce_fwd / _bwd over the score
rows the GEMM scorer already computes) next to the sampled node and to the torch composite, in one process.

  node     forward + backward of one loss node on a synthetic loss plan, device time of
             all-entity   batched_all_entity_link_prediction (no sampler launch, no candidate matrix)
             sampled K    corrupt_sample (one launch, K negatives) + batched_link_prediction, K = 100 and 500
           at the S-icews14 step (B = 8 windows of N = 7 128 entities, 400 query rows each = 3 200 rows, D = 128 and 200, ComplEx) and
           at N = 2^19 (one window, 1 024 rows, D = 128: column panels of ALL_ENTITY_PANEL_BYTES, the scores recomputed in the
           backward; temp_gather_ce_bwd refuses N > 40 704, so the sampled node has no arm there).
  kernels  temp_filtered_ce_fwd + _bwd against the composite (link_loss.filtered_ce_rows_torch: mask to -inf, logsumexp, autograd)
           on the same (rows, N) score matrix, at both shapes.
  Known-true lists: 1 - 5 entries per row, every 100th row a hub of 300.
  Protocol: warm-up, then rounds that alternate the arms, each round the device-event time of `reps` back-to-back calls; median
  and range (smallest - largest round) per arm.

    python tools/all_entity_loss_probe.py [--out profiles/all_entity_loss_probe.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd import functional as TF  # noqa: E402
from temp_amd import link_loss as LL  # noqa: E402
from temp_amd.backend import get_backend  # noqa: E402
from tools.hyte_probe import timed  # noqa: E402

N_REL = 460


def make_plan(B, N, rows_per_window, device, seed):
    """A loss plan of the shape sampling.plan_batch_loss builds: per window [tail rows ; head rows], known rows among B * N."""
    rng = np.random.default_rng(seed)
    P = B * rows_per_window
    known = (np.repeat(np.arange(B), rows_per_window) * N + rng.integers(0, N, P)).astype(np.int64)
    rel = rng.integers(0, N_REL, P).astype(np.int64)
    is_tail = np.tile(np.repeat([1, 0], rows_per_window // 2), B)
    truth = rng.integers(0, N, P)
    lens = rng.integers(1, 6, P)
    lens[::100] = 300
    lists = []
    for p in range(P):
        others = rng.integers(0, N, int(lens[p]) - 1)                 # (a repeated draw only shortens the list)
        lists.append(np.unique(np.append(others, truth[p])))
    hi = np.cumsum([len(x) for x in lists])
    lo = hi - np.array([len(x) for x in lists])
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(device)
    return dict(known=i32(known), rel=i32(rel), is_tail=i32(is_tail), truth=i32(truth), lo=i32(lo), hi=i32(hi), ids=i32(np.concatenate(lists)),
                weights=torch.full((P,), 2.0 / rows_per_window, device=device), splits=[(b * rows_per_window, (b + 1) * rows_per_window) for b in range(B)],
                window=i32(np.repeat(np.arange(B), rows_per_window)), known_inv=TF.gather_inverse(known, B * N, device),
                rel_inv=TF.gather_inverse(rel, N_REL, device))


def rounds_of(arms, rounds, reps, say):
    for fn in arms.values():
        timed(fn, max(1, reps // 4))
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, reps))
    for k, v in t.items():
        say("  %-22s median %10.1f us   range %10.1f - %10.1f us   (%d rounds x %d calls)" % (k, np.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6, rounds, reps))
    return {k: float(np.median(v)) for k, v in t.items()}


def probe(B, N, rows_per_window, D, rounds, reps, device, say, sampled=True):
    be = get_backend()
    g = torch.Generator(device="cpu").manual_seed(N + D)
    plan = make_plan(B, N, rows_per_window, device, N + D)
    P = B * rows_per_window
    leaf = lambda n: (torch.randn(n, D, generator=g) * D ** -0.25).to(device).requires_grad_(True)
    ent, rel, big = leaf(B * N), leaf(N_REL), leaf(B * N)
    panel = LL.all_entity_panel(None, P, N)
    say("\nB = %d, N = %d, %d rows, D = %d, complex; %d column panel(s) of %d; %d list entries (longest %d)"
        % (B, N, P, D, -(-N // panel), panel, int(plan["ids"].shape[0]), int((plan["hi"] - plan["lo"]).max())))

    def all_entity():
        TF.batched_all_entity_link_prediction(ent, rel, big, "complex", plan).backward()

    def sampled_node(K):
        def run():
            cand = be.corrupt_sample(7, plan["truth"], plan["lo"], plan["hi"], plan["ids"], K, N)
            TF.batched_link_prediction(ent, rel, big, "complex", dict(plan, cand=cand)).backward()
        return run
    arms = {"node all-entity": all_entity}
    if sampled:
        arms.update({"node sampled K=100": sampled_node(100), "node sampled K=500": sampled_node(500)})
    med = rounds_of(arms, rounds, reps, say)
    for k in list(med)[1:]:
        say("  all-entity / %s = %.3f of the medians" % (k[5:], med["node all-entity"] / med[k]))
    if not sampled:
        say("  (no sampled arm: temp_gather_ce_bwd keeps N counters in LDS and refuses N > 40 704)")

    # the two kernels against the composite, on one (rows, N) score matrix
    scores = (torch.randn(P, N, generator=g) * 2.0).to(device)
    one = torch.ones(1, device=device)
    lists = (plan["truth"], plan["lo"], plan["hi"], plan["ids"])

    def kernels():
        _, lse, _ = be.filtered_ce_fwd(scores, *lists)
        return be.filtered_ce_bwd(scores, *lists, lse, one, 1.0, plan["weights"])

    def composite():
        s = scores.detach().requires_grad_(True)
        loss_rows, _ = LL.filtered_ce_rows_torch(s, *lists)
        (loss_rows * plan["weights"]).sum().backward()
        return s.grad
    err = float((kernels() - composite()).abs().max())
    med = rounds_of({"kernels fwd + bwd": kernels, "composite fwd + bwd": composite}, rounds, max(1, reps // 2), say)
    moved = 3.0 * P * N * 4
    say("  kernels / composite = %.3f of the medians (%s); max |d_scores kernels - composite| = %.3g; the kernels move %.0f MB -> %.2f TB/s"
        % (med["kernels fwd + bwd"] / med["composite fwd + bwd"],
           "the kernels are faster" if med["kernels fwd + bwd"] < med["composite fwd + bwd"] else "THE KERNELS LOSE to the composite's masked logsumexp",
           err, moved / 1e6, moved / med["kernels fwd + bwd"] / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("all_entity_loss_probe needs the GPU: nothing here is measured without one")
    device = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches, device events, arms alternating round by round" % torch.cuda.get_device_name(0))
    for D in (128, 200):
        probe(8, 7128, 400, D, 7, 20, device, say)
    probe(1, 1 << 19, 1024, 128, 5, 2, device, say, sampled=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
