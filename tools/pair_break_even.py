#!/usr/bin/env python3
"""Break-even of the pair route: layer 1 forward + backward on unions of m GDELT-shaped snapshots, table route
(TEMP_OPT_RGCN_PAIR = 0) against pair route (2), each captured into a HIP graph, device-event times of 20 replays after 5; the ratio
n_edges / (n_rel_rows * n_table) of every union beside them.  TEMP_PAIR_MIN_RATIO must lie above the ratio where the two meet.
    python tools/pair_break_even.py [m ...]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temp_amd import _lib, synthetic  # noqa: E402
from temp_amd import functional as TF  # noqa: E402
from temp_amd import snapshot as S  # noqa: E402
from temp_amd.rgcn import RGCNLayer  # noqa: E402

ms = [int(x) for x in sys.argv[1:]] or [2, 4, 6, 9, 12, 16, 24, 40, 80, 163]
dev = torch.device("cuda:0")
lib = _lib.load()
w = synthetic.workload("S-gdelt", seed=0)
R2, N, D, B = 2 * w["num_rels"], w["num_ents"], w["D"], w["B"]
torch.manual_seed(1)
layer = RGCNLayer(argparse.Namespace(inv_temperature=0.1, learnable_lambda=False, impute=False), D, D, R2, B, [0], activation=None,
                  self_loop=True).to(dev)
table = torch.randn(N, D, device=dev, requires_grad=True)
print("snapshots  edges  edges/pair  table route us  pair route us  (forward + backward of layer 1, graph replay)")
for m in ms:
    g = S.batch([w["snapshots"][(7 * t) % w["num_times"]] for t in range(m)])
    ids = torch.from_numpy(g.gids.astype(np.int32)).to(dev)
    inv = TF.gather_inverse(g.gids, N, dev)
    gy = torch.randn(g.n, D, device=dev)
    res = []
    for opt in (0, 2):
        lib.temp_set_option(_lib.OPT_RGCN_PAIR, opt)
        layer.prepare_table(g, N, ids)
        def step():
            table.grad = None
            layer.conv_table(g, table, ids, inv).backward(gy)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        table.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(25):
            if it == 5:
                ev[0].record()
            graph.replay()
        ev[1].record()
        torch.cuda.synchronize()
        res.append(1e3 * ev[0].elapsed_time(ev[1]) / 20)
    print("%9d %6d %10.1f %15.1f %14.1f" % (m, g.number_of_edges(), g.number_of_edges() / (R2 * N), res[0], res[1]), flush=True)
lib.temp_set_option(_lib.OPT_RGCN_PAIR, 1)
