"""The optimizer step of the reference trainer -- clip_grad_norm_(parameters, 1.0) + Adam(lr, weight_decay = 1e-4) -- two ways on the
same parameter set in one process: torch's route (clip_grad_norm_ + Adam(fused=True); the yardstick, not code under test) and
temp_amd.optim.ClippedAdam (table upload + k_adam_grad_norm, k_adam_norm_finish, k_adam_clip_step).

Parameter sets: the S-gdelt BiGRRGCN model's (bench.build_model), and the same set with the entity table at 2^19 x 200 (the
HBM-window size).  Gradients are fixed seeded tensors with a norm far above 1 (each route owns a copy: torch's clip scales its
gradients in place).  After warm-up the routes alternate, --rounds rounds of --steps steps each; per round and route:
  host issue time  = host clock from the first step's call to the last step's return, over the steps (nothing waits);
  device time      = device events around the same steps, read after a synchronise, over the steps (for a set this small the
                     device waits for the host, so this is the larger of the two costs, not kernel time).
Medians over the rounds.  Library launches and per-kernel times: the library's own trace (events around its launches) of 5 further
steps; the norm pass streams 4 bytes per element, the update 28 (p, g, m, v read; p, m, v written).  Device kernels of one step as
torch.profiler counts them, for both routes.

    python tools/clipped_adam_probe.py [--steps 50] [--rounds 7] [--out profiles/clipped_adam_probe.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd.optim import ClippedAdam  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
LR, WD, MAX_NORM = 1e-3, 1e-4, 1.0


def model_shapes(device):
    w = synthetic.workload("S-gdelt", seed=0)
    m = bench.build_model(w, device)
    return [(k, tuple(p.shape)) for k, p in m.named_parameters()]


def make_route(shapes, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=device, generator=g) * 0.1) for _, s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=device, generator=g)
    return params


def device_launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:
        print("  (torch.profiler: %s)" % exc)
        return None


def library_trace(step, steps, lib):
    cap = 16 * steps
    ids, ms, cnt = (ctypes.c_int32 * cap)(), (ctypes.c_float * cap)(), ctypes.c_int32()
    _lib.check(lib.temp_trace_begin(cap), "temp_trace_begin")
    try:
        for _ in range(steps):
            step()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, cap, ctypes.byref(cnt)), "temp_trace_end")
    per = {}
    for i in range(cnt.value):
        per.setdefault(lib.temp_trace_kernel_name(ids[i]).decode(), []).append(ms[i])
    return cnt.value / steps, {k: float(np.median(v)) for k, v in per.items()}


def probe(what, shapes, steps, rounds, lib, device, say):
    n_elem = sum(int(np.prod(s)) for _, s in shapes)
    tp, op = make_route(shapes, device, 1), make_route(shapes, device, 1)
    topt = torch.optim.Adam(tp, lr=LR, weight_decay=WD, fused=True)
    oopt = ClippedAdam(op, lr=LR, weight_decay=WD, max_norm=MAX_NORM)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
        topt.step()

    our_step = oopt.step
    routes = [("clip_grad_norm_ + Adam(fused=True)", torch_step), ("ClippedAdam", our_step)]
    for _ in range(5):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    norm = float(oopt.last_grad_norm)
    host, dev = [[] for _ in routes], [[] for _ in routes]
    for _ in range(rounds):
        for k, (_, fn) in enumerate(routes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            host[k].append(1e3 * (t1 - t0) / steps)
            dev[k].append(e0.elapsed_time(e1) / steps)
    say("\n%s: %d tensors, %d elements (%.1f MB per fp32 copy), gradient norm %.1f, max_norm %.1f; %d rounds x %d steps per route, alternating"
        % (what, len(shapes), n_elem, 4e-6 * n_elem, norm, MAX_NORM, rounds, steps))
    med = []
    for k, (name, fn) in enumerate(routes):
        h, d = np.percentile(host[k], [25, 50, 75]), np.percentile(dev[k], [25, 50, 75])
        med.append((h[1], d[1]))
        say("  %-36s host issue %.4f ms/step (quartiles %.4f - %.4f)   device events %.4f ms/step (quartiles %.4f - %.4f)"
            % (name, h[1], h[0], h[2], d[1], d[0], d[2]))
    say("  ClippedAdam / torch route: host %.3f, device %.3f" % (med[1][0] / med[0][0], med[1][1] / med[0][1]))
    for name, fn in routes:
        n_dev = device_launches(fn)
        say("  %-36s device kernels of one step by torch.profiler: %s" % (name, "not measured" if n_dev is None else str(n_dev)))
    n_launch, per = library_trace(our_step, 5, lib)
    say("  ClippedAdam: %.0f library launches per step" % n_launch)
    for kname, nbytes in (("k_adam_grad_norm", 4 * n_elem), ("k_adam_clip_step", 28 * n_elem)):
        s = per[kname] * 1e-3
        say("    %-20s %9.4f ms (median of 5 traced launches)  %8.1f MB  -> %.3f TB/s = %.0f %% of the 8.0 TB/s peak, %.0f %% of the 6.29 TB/s copy rate"
            % (kname, per[kname], nbytes / 1e6, nbytes / s / 1e12, 100 * nbytes / s / HBM_PEAK, 100 * nbytes / s / HBM_COPY))
    say("    %-20s %9.4f ms" % ("k_adam_norm_finish", per["k_adam_norm_finish"]))
    s = per["k_adam_grad_norm"] * 1e-3
    say("    norm pass: %.3g fp64 FMA/s (one per element: one per 4 bytes streamed)" % (n_elem / s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; eager launches; routes alternate in one process after 5 warm-up steps each" % torch.cuda.get_device_name(0))
    shapes = model_shapes(device)
    probe("S-gdelt BiGRRGCN parameters", shapes, a.steps, a.rounds, lib, device, say)
    big = [(k, (1 << 19, 200) if k == "ent_embeds" else s) for k, s in shapes]
    assert big != shapes
    probe("the same with the entity table at 2^19 x 200", big, a.big_steps, a.rounds, lib, device, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
