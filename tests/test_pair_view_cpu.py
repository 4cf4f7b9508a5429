"""Pair view builder (temp_amd/pair_view.py) without a GPU: the grouping of a by-destination view's edges by
(relation row, table row of the source) against a numpy restatement -- every edge exactly once, under its key, in a
reproducible order; the chunk / slot / fix-up tables consistent with that grouping; the padding harmless."""
import numpy as np
import pytest
import torch

from temp_amd import pair_view as PV
from temp_amd import snapshot as S
from temp_amd.snapshot import Snapshot


def np_grouping(a, b, seg_of, ids, n_table):
    """(positions of the edges in pair order, their keys): a stable sort of the occupied positions by rel * n_table + ids[src]."""
    pos = np.nonzero(seg_of >= 0)[0]
    key = b[pos].astype(np.int64) * n_table + ids[a[pos]]
    o = np.argsort(key, kind="stable")
    return pos[o], key[o]


def check_view(t, a, b, seg_of, ids, n_table, n_rel_rows, chunk):
    P = n_rel_rows * n_table
    v = {k: (x.numpy() if torch.is_tensor(x) else x) for k, x in t.items()}
    pos, key = np_grouping(a, b, seg_of, ids, n_table)
    E = pos.shape[0]
    # forward map: every occupied position names its pair
    assert np.array_equal(v["fwd_row"][pos], key)
    # the sorted destination list: pair order, by-dst order inside a pair
    assert np.array_equal(v["a"][:E], seg_of[pos])
    assert v["n_seg"] == P + 1 and v["n_chunks"] == v["chunk_seg"].shape[0] and v["n_fix"] == v["fix_seg"].shape[0]
    cseg, cbeg, cend, cslot = v["chunk_seg"], v["chunk_beg"], v["chunk_end"], v["chunk_slot"]
    live = cseg < P
    n_live = int(live.sum())
    assert live[:n_live].all(), "live chunks come first"
    assert (cseg[n_live:] == P).all() and (cbeg[n_live:] == cend[n_live:]).all() and (cslot[n_live:] == -1).all(), "padding chunks"
    assert (np.diff(cseg[:n_live]) >= 0).all() and np.array_equal(np.unique(cseg[:n_live]), np.arange(P)), "every pair owns a chunk"
    assert ((cend - cbeg) <= chunk).all() and ((cend - cbeg) >= 0).all()
    # the live chunks tile [0, E) in order: every edge exactly once, under its key
    covered = np.concatenate([np.arange(cbeg[c], cend[c]) for c in range(n_live)]) if n_live else np.zeros(0, np.int64)
    assert np.array_equal(covered, np.arange(E))
    per_edge_seg = np.repeat(cseg[:n_live], (cend - cbeg)[:n_live])
    assert np.array_equal(per_edge_seg, key)
    # slots and fix-up entries
    counts = np.bincount(cseg[:n_live], minlength=P)
    multi = np.nonzero(counts > 1)[0]
    nf = multi.shape[0]
    assert nf <= v["n_fix"] and int(counts[multi].sum()) <= v["n_partial"]
    assert np.array_equal(v["fix_seg"][:nf], multi) and np.array_equal(v["fix_cnt"][:nf], counts[multi])
    assert (v["fix_seg"][nf:] == P).all() and (v["fix_cnt"][nf:] == 0).all(), "padding fix-up entries"
    want_slot = np.full(n_live, -1, np.int64)
    first = np.concatenate([[0], np.cumsum(counts[multi])])[:-1] if nf else np.zeros(0, np.int64)
    assert np.array_equal(v["fix_slot"][:nf], first)
    for s, f0 in zip(multi, first):
        cs = np.nonzero(cseg[:n_live] == s)[0]
        want_slot[cs] = f0 + np.arange(cs.shape[0])
    assert np.array_equal(cslot[:n_live], want_slot)


@pytest.mark.parametrize("seed,L,n,n_table,R2,chunk,holes", [
    (0, 0, 5, 3, 2, 4, False),            # no edges at all
    (1, 37, 9, 4, 3, 4, False),
    (2, 400, 30, 5, 4, 8, True),          # positions that no chunk covers (a device-subsampled member)
    (3, 700, 40, 3, 2, 16, True),         # few pairs: every pair a multi-chunk one
    (4, 150, 20, 50, 6, 128, False),      # more pairs than edges: most pairs empty
])
def test_build_pair_view_matches_numpy_grouping(seed, L, n, n_table, R2, chunk, holes):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, L).astype(np.int32)
    b = rng.integers(0, R2, L).astype(np.int32)
    seg_of = np.sort(rng.integers(0, n, L)).astype(np.int32)
    if holes:
        dead = rng.random(L) < 0.3
        seg_of[dead] = -1
        a[dead] = 10 ** 6                  # what an unused position holds is never read
        b[dead] = -7
    ids = rng.integers(0, n_table, n).astype(np.int32)
    tt = lambda x: torch.from_numpy(x)
    t1 = PV.build_pair_view(tt(a), tt(b), tt(seg_of), tt(ids), n_table, R2, chunk=chunk)
    check_view(t1, a, b, seg_of, ids, n_table, R2, chunk)
    t2 = PV.build_pair_view(tt(a.copy()), tt(b.copy()), tt(seg_of.copy()), tt(ids.copy()), n_table, R2, chunk=chunk)
    for k, x in t1.items():
        assert torch.equal(x, t2[k]) if torch.is_tensor(x) else x == t2[k], k


def test_pair_view_of_a_union_device_graph():
    """Through the device-graph plumbing (CPU tensors): a union of snapshots with a hub pair and an unused relation row."""
    rng = np.random.default_rng(11)
    n_table, R2 = 12, 6
    parts = []
    for _ in range(3):
        n, E = 10, 300
        src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
        rel = rng.integers(0, R2 - 1, E)                  # relation row R2 - 1 never occurs: pairs without edges
        src[:200], rel[:200] = 0, 2                       # a hub pair
        parts.append(Snapshot(n, src, dst, rel, np.sort(rng.choice(n_table, n, replace=False))))
    g = S.batch(parts)
    dev = torch.device("cpu")
    dg = g.device_graph(dev, R2)
    ids = torch.from_numpy(g.gids.astype(np.int32))
    pv = PV.DevicePairView(dg, ids, n_table, R2)
    vt = lambda name: dg.view_tensor("by_dst", name).numpy()
    seg_of = PV.expand_chunk_segments(dg.view_tensor("by_dst", "chunk_seg"), dg.view_tensor("by_dst", "chunk_beg"),
                                      dg.view_tensor("by_dst", "chunk_end"), vt("a").shape[0]).numpy()
    assert (seg_of >= 0).sum() == g.number_of_edges()
    check_view(pv.t, vt("a"), vt("b"), seg_of, ids.numpy(), n_table, R2, PV.PAIR_CHUNK)
    # the edges of the view are the union's edges: (src, rel, dst) multisets agree
    got = np.stack([vt("a"), vt("b"), seg_of], 1)[seg_of >= 0]
    want = np.stack([g.src, g.rel, g.dst], 1)
    assert np.array_equal(got[np.lexsort(got.T)], want[np.lexsort(want.T)])
    assert pv.c.by_pair.n_seg == R2 * n_table + 1 and pv.c.n_table == n_table


def test_expand_chunk_segments_torch():
    cseg = torch.tensor([4, 4, 7, 9], dtype=torch.int32)
    cbeg = torch.tensor([0, 3, 6, 10], dtype=torch.int32)
    cend = torch.tensor([3, 5, 6, 12], dtype=torch.int32)       # position 5 and 6..9 unused, chunk 2 empty
    got = PV.expand_chunk_segments(cseg, cbeg, cend, 13).tolist()
    assert got == [4, 4, 4, 4, 4, -1, -1, -1, -1, -1, 9, 9, -1]
