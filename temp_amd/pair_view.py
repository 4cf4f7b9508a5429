"""Pair view of a device graph: the edges of a table-fed RGCN layer grouped by (relation row, table row of the source).

The message of an edge (u, r, v) of layer 1 is table[ids[u]] . BD(W[r]): it depends on the pair (r, ids[u]) only (include/temp_amd.h:
TempPairView).  `build_pair_view` turns the by-destination view of a graph into

  fwd_row   per position of the by-dst edge arrays: the pair index  rel * n_table + ids[src]  (the row of M the forward gathers)
  by_pair   the same edges grouped by pair -- a stable sort of the by-dst positions by pair index, so the order inside a pair is the
            by-dst order: reproducible -- cut into chunks of at most PAIR_CHUNK edges with ordered partial slots

with torch tensor ops only, on whatever device the inputs live on, and WITHOUT a device -> host copy: every list is sized from an
upper bound that the host knows (array length, number of pairs) and padded with entries that land in the spare row P of the result
(see the header).  A prepare that waited for a count would wait for the training step in flight on the same stream.
"""
import ctypes

import torch

from . import _lib

PAIR_CHUNK = 128           # include/temp_amd.h: TEMP_CHUNK_PAIR
PAIR_MIN_RATIO = 4         # include/temp_amd.h: TEMP_PAIR_MIN_RATIO -- the specified floor, not a break-even: on GDELT's table the route won
                           # at every ratio tried, down to 0.7 (profiles/r08_pair_route_ab.txt); other tables were not measured


def expand_chunk_segments(chunk_seg, chunk_beg, chunk_end, n_pos):
    """seg_of [n_pos] int32: the segment of every edge-array position a chunk covers, -1 elsewhere (torch restatement of
    temp_expand_chunk_segments for tensors that are not on a GPU)."""
    seg_of = torch.full((n_pos,), -1, dtype=torch.int32, device=chunk_seg.device)
    cnt = (chunk_end - chunk_beg).long()
    if cnt.numel() == 0 or int(cnt.sum()) == 0:
        return seg_of
    start = torch.cumsum(cnt, 0) - cnt
    pos = torch.repeat_interleave(chunk_beg.long() - start, cnt) + torch.arange(int(cnt.sum()), device=cnt.device)
    seg_of[pos] = torch.repeat_interleave(chunk_seg, cnt)
    return seg_of


def build_pair_view(a, b, seg_of, ids, n_table, n_rel_rows, chunk=PAIR_CHUNK):
    """a, b, seg_of: int32 [L] -- source node, relation row and destination node of every by-dst edge-array position (seg_of < 0: the
    position holds no edge); ids int32 [n_nodes].  -> dict of int32 tensors (fwd_row, a, chunk_*, fix_*) and the host counts
    n_seg, n_chunks, n_partial, n_fix (upper bounds, see the module text)."""
    dev, L, P = a.device, int(a.shape[0]), int(n_rel_rows) * int(n_table)
    i32 = lambda t: t.to(torch.int32).contiguous()
    valid = seg_of >= 0
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    src = torch.where(valid, a.long(), zero)
    row = torch.where(valid, b.long(), zero) * n_table + ids.long()[src]
    key = torch.where(valid, row, torch.full((), P, dtype=torch.int64, device=dev))
    skey, order = torch.sort(key, stable=True)                      # positions without an edge sort behind every pair
    ptr = torch.searchsorted(skey, torch.arange(P + 1, device=dev))  # [P + 1] first sorted position of every pair
    cnt = ptr[1:] - ptr[:-1]
    nch = torch.clamp((cnt + chunk - 1) // chunk, min=1)            # every pair owns a chunk: its row of G is always written
    cum = torch.cumsum(nch, 0)
    n_chunks = L // chunk + P + 1                                   # >= sum(nch)
    cid = torch.arange(n_chunks, device=dev)
    cs = torch.searchsorted(cum, cid, right=True)                   # pair of chunk cid; P for the padding behind the last pair
    live = cs < P
    csc = torch.clamp(cs, max=P - 1)
    cbeg = ptr[csc] + (cid - (cum - nch)[csc]) * chunk
    cend = torch.minimum(cbeg + chunk, ptr[csc + 1])
    multi = nch > 1
    mc = live & multi[csc]
    slot = torch.where(mc, torch.cumsum(mc, 0) - 1, torch.full((), -1, dtype=torch.int64, device=dev))
    pad = torch.full((), P, dtype=torch.int64, device=dev)
    n_fix = min(P, L // chunk + 1)                                  # a multi-chunk pair has more than `chunk` edges
    fo = torch.sort(multi.logical_not().to(torch.int32), stable=True).indices[:n_fix]     # the multi-chunk pairs first, in pair order
    fv = multi[fo]
    fcnt = torch.where(fv, nch[fo], zero)
    return dict(fwd_row=i32(torch.where(valid, row, zero)), a=i32(seg_of[order]),
                chunk_seg=i32(torch.where(live, csc, pad)), chunk_beg=i32(torch.where(live, cbeg, zero)),
                chunk_end=i32(torch.where(live, cend, zero)), chunk_slot=i32(slot),
                fix_seg=i32(torch.where(fv, fo, pad)), fix_slot=i32(torch.cumsum(fcnt, 0) - fcnt), fix_cnt=i32(fcnt),
                n_seg=P + 1, n_edges=L, n_chunks=n_chunks, n_partial=n_chunks, n_fix=n_fix)


class DevicePairView:
    """build_pair_view of a device graph for one ids tensor + the TempPairView struct that points into its tensors."""

    def __init__(self, dg, ids, n_table, n_rel_rows, expand=None):
        self.ids = ids                                               # (kept alive: the cache is keyed by this tensor)
        vt = lambda name: dg.view_tensor("by_dst", name)
        a, b = vt("a"), vt("b")
        seg_of = (expand or expand_chunk_segments)(vt("chunk_seg"), vt("chunk_beg"), vt("chunk_end"), int(a.shape[0]))
        self.t = t = build_pair_view(a, b, seg_of, ids, n_table, n_rel_rows)
        self.n_table, self.n_rel_rows = int(n_table), int(n_rel_rows)
        c = _lib.TempPairView()
        c.n_table, c.n_rel_rows = self.n_table, self.n_rel_rows
        ptr = lambda x: x.data_ptr() if x.numel() else 0
        c.fwd_row = ptr(t["fwd_row"])
        v = c.by_pair
        for fld in ("n_seg", "n_edges", "n_chunks", "n_partial", "n_fix"):
            setattr(v, fld, t[fld])
        for an in ("a", "chunk_seg", "chunk_beg", "chunk_end", "chunk_slot", "fix_seg", "fix_slot", "fix_cnt"):
            setattr(v, an, ptr(t[an]))
        v.b = 0
        self.c = c

    def ref(self):
        return ctypes.byref(self.c)
