"""The host-side facts the cases of tests/rgcn_layer_cases.py rest on, without a GPU: every claim of a case about its views -- the
by-destination view of the graph and the by-pair view temp_amd/pair_view.py builds from it -- is asserted from host data, so that a
GPU run is not spent on a case that cannot reach its path; the exact operands are exact (every sum of |terms| below 2^24
sixteenths); the fp64 reference agrees with an independent implementation (the fp32 test backend, bit for bit on the exact operands,
inside the GPU test's bar on the wide ones) and with its own gradient formulas written out; the comparison helper rejects what it
must."""
import functools

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import pair_view as PV
from temp_amd import snapshot as SN
from tests import rgcn_layer_cases as LC
from tests.cpu_backend import CpuTestBackend

CPU = torch.device("cpu")
PAIR_CASES = [c for c in LC.ALL if "pair" in c.routes and c.graph != "subsampled"]      # (a device-side subsample has no host views: test_subsampled_graph)


def _ids(cases):
    return [c.id for c in cases]


@functools.lru_cache(maxsize=4)
def _views(graph, seed, R2, n_table):
    """(Graph, Snapshot, device graph on the CPU, by-pair view) of a graph family"""
    case = LC.Case("", graph, seed, 0, 0, 1, R2, n_table, LC.FLAGS[0], (), (), {})
    G = LC.graph(case)
    snap = LC.snapshot(case, exact=True)
    dg = snap.device_graph(CPU, R2)
    ids = torch.from_numpy(G.ids.astype(np.int32))
    return G, snap, dg, PV.DevicePairView(dg, ids, n_table, R2)


def _fast_shape(d_in, d_out, B):
    return d_in == d_out and d_in % 4 == 0 and d_in <= 256 and d_in % B == 0 and (d_in // B) in (1, 2, 4)


def _pair_facts(case):
    G, snap, dg, pv = _views(case.graph, case.seed, case.R2, case.n_table)
    t = pv.t
    cnt = t["fix_cnt"].numpy()
    return dict(G=G, dg=dg, t=t, P=case.R2 * case.n_table, L=int(dg.view_tensor("by_dst", "a").shape[0]), real=int((cnt > 0).sum()),
                padded=int((cnt == 0).sum()), longest=int(cnt.max()) if cnt.size else 0, by_dst=dg.views["by_dst"])


@pytest.mark.parametrize("case", PAIR_CASES, ids=_ids(PAIR_CASES))
def test_pair_view_is_sized_from_upper_bounds_and_reaches_its_fixup(case):
    """n_chunks = n_partial = L // 128 + P + 1 and n_fix = min(P, L // 128 + 1) whatever the edges; padded fix entries have
    fix_cnt = 0 and land in the spare row P; launch_fixup on these counts makes exactly the launches the case pins."""
    f = _pair_facts(case)
    t, P, L = f["t"], f["P"], f["L"]
    assert t["n_chunks"] == t["n_partial"] == L // 128 + P + 1 and t["n_fix"] == min(P, L // 128 + 1) and t["n_seg"] == P + 1
    cnt, seg = t["fix_cnt"].numpy(), t["fix_seg"].numpy()
    assert cnt.shape[0] == t["n_fix"] and ((cnt == 0) == (seg == P)).all() and (cnt != 1).all()
    assert int(t["chunk_slot"].max()) < t["n_partial"]
    assert int((t["chunk_seg"] < P).sum()) >= P, "every pair owns a chunk"
    got = LC.predict_fix(t["n_fix"], t["n_partial"], case.d_out)
    print("%s: P %d, L %d, n_partial %d, n_fix %d (%d real, %d padded, longest %d of huge %d), items %d -> %s" % (
        case.id, P, L, t["n_partial"], t["n_fix"], f["real"], f["padded"], f["longest"], LC.fix_huge(t["n_partial"]),
        t["n_fix"] * -(-case.d_out // 256), sorted(got)))
    assert got == case.fix
    assert _fast_shape(case.d_in, case.d_out, case.B)


def test_small_graph_facts():
    c = LC.BY_ID["small_d8_b2_f0"]
    f = _pair_facts(c)
    G = f["G"]
    in_deg, out_deg = np.bincount(G.dst, minlength=G.n), np.bincount(G.src, minlength=G.n)
    assert G.n == 70 and G.src.shape[0] == 400 and c.R2 == 6 and c.n_table == 37
    assert (in_deg == 0).sum() >= 10 and (out_deg == 0).sum() >= 10
    assert G.rel.max() == 4 and set(range(34, 37)).isdisjoint(G.ids) and G.ids.max() < 34, "relation row 5 and the last three table rows are unused"
    assert np.unique(G.ids).shape[0] < G.n, "repeated ids"
    assert f["by_dst"]["n_fix"] == 0 and f["real"] == 0 and f["padded"] == 4
    assert LC.pair_tail_grid(37) == (5, 1) and LC.tail_waves(6) == (1, 6)
    shapes = [(x.d_in, x.B) for x in LC.ALL if x.graph == "small" and "pair" in x.routes and x.R2 == 6]
    assert sorted(set(shapes)) == [(8, 2), (32, 32), (200, 100), (256, 64)]
    assert [(D // B, D // 4) for D, B in sorted(set(shapes))] == [(4, 2), (1, 8), (2, 50), (4, 64)], "S and active lanes"
    for D, B in set(shapes):
        assert sorted(x.flags for x in LC.ALL if x.graph == "small" and x.R2 == 6 and (x.d_in, x.B) == (D, B) and "pair" in x.routes) == sorted(LC.FLAGS)


def test_generic_shapes_are_refused_by_the_pair_route():
    for cid, s in (("generic_24_24_b4", (6, 6)), ("generic_64_32_b16", (4, 2))):
        c = LC.BY_ID[cid]
        assert (c.d_in // c.B, c.d_out // c.B) == s and not _fast_shape(c.d_in, c.d_out, c.B) and c.routes == ("table",)
        assert max(c.d_in, c.d_out) <= 256, "temp_rgcn_table_bwd takes widths up to 256"


def test_one_pair_graph_facts():
    c = LC.BY_ID["one"]
    f = _pair_facts(c)
    t = f["t"]
    assert f["P"] == 1 and t["n_fix"] == 1 and t["fix_cnt"].tolist() == [3] and t["fix_seg"].tolist() == [0]
    assert t["n_chunks"] == 4 and int((t["chunk_seg"] == 0).sum()) == 3
    assert (t["chunk_end"] - t["chunk_beg"]).tolist() == [128, 128, 44, 0]
    assert LC.pair_tail_grid(1) == (1, 1) and LC.tail_waves(1) == (1, 1), "one block (no slice reduction), one active wave, a tile of one row"


def test_relation_shares_of_the_tail_waves():
    assert LC.tail_waves(9) == (2, 5) and LC.tail_waves(42) == (6, 7), "waves that own no relation row"
    for cid, R2 in (("rel9", 9), ("rel42", 42)):
        c = LC.BY_ID[cid]
        assert c.R2 == R2 and (c.d_in, c.B) == (64, 16) and LC.graph(c).rel.max() == R2 - 2


def test_tiles_graph_facts():
    c = LC.BY_ID["tiles"]
    f = _pair_facts(c)
    blocks, per = LC.pair_tail_grid(c.n_table)
    assert -(-c.n_table // 8) == 129 and (blocks, per) == (65, 2) and blocks <= 128 and blocks * per > 129 > (blocks - 1) * per, "a short last block"
    assert c.n_table % 8 != 0 and f["real"] == 0


def test_hubdst_graph_facts():
    c = LC.BY_ID["hubdst"]
    f = _pair_facts(c)
    v = f["by_dst"]
    assert v["n_fix"] == 1 and int(v["fix_seg"][0]) == 5 and int(v["fix_cnt"][0]) >= 11, "node 5: 700 in-edges in chunks of 64"
    assert LC.predict_fix(v["n_fix"], v["n_partial"], c.d_out) == {("fix_few", 0): 1}, "the table forward's own fix-up"


def test_fixmany_graph_facts():
    c = LC.BY_ID["fixmany"]
    f = _pair_facts(c)
    t = f["t"]
    assert f["P"] == 1600 and t["n_fix"] * -(-c.d_out // 256) > 1024 and t["n_partial"] < LC.FIX_SPLIT_MIN
    assert f["real"] > 0 and f["padded"] > 0 and f["longest"] <= 256


def test_split_graph_facts():
    c = LC.BY_ID["splitfew"]
    f = _pair_facts(c)
    t = f["t"]
    assert f["P"] == 33280 and t["n_partial"] >= LC.FIX_SPLIT_MIN and t["n_fix"] == 47 and (f["real"], f["padded"]) == (1, 46)
    assert f["longest"] == 3 <= LC.fix_huge(t["n_partial"]), "nothing is listed for the second level"
    c = LC.BY_ID["splitlisted"]
    f = _pair_facts(c)
    t = f["t"]
    huge = LC.fix_huge(t["n_partial"])
    assert t["n_partial"] >= LC.FIX_SPLIT_MIN and t["n_fix"] > 1024 and huge == 2048 == max(-(-t["n_partial"] // 4095), 2048)
    assert int((t["fix_cnt"] > huge).sum()) == 1 and f["longest"] == -(-270000 // 128) and f["padded"] > 0 and f["real"] == 2
    assert sorted(t["fix_cnt"][t["fix_cnt"] > 0].tolist()) == [3, 2110], "a short entry beside the listed one"
    assert int(t["fix_seg"][int(t["fix_cnt"].argmax())]) == 3 * c.n_table + 7
    assert f["by_dst"]["n_fix"] > 0


def test_members_graph_facts():
    c = LC.BY_ID["members"]
    G, snap, dg, pv = _views(c.graph, c.seed, c.R2, c.n_table)
    assert isinstance(snap, SN.BatchedSnapshot) and [(g.n, g.number_of_edges()) for g in snap.parts] == [(50, 150), (70, 300), (30, 0)]
    assert int(snap.edge_off[-1]) // (SN.REL_GROUP_EDGES * c.R2) > 1, "the union carries member tables"
    assert np.array_equal(snap.src, G.src) and np.array_equal(snap.dst, G.dst) and np.array_equal(snap.gids, G.ids)


def test_noedges_graph_facts():
    for cid in ("noedges_d16_b8", "noedges_d32_b32"):
        c = LC.BY_ID[cid]
        f = _pair_facts(c)
        assert f["by_dst"]["n_chunks"] == 0 and f["L"] == 0 and f["t"]["n_chunks"] == f["P"] + 1 and f["t"]["n_fix"] == 1 and f["real"] == 0
        assert int((f["t"]["chunk_end"] - f["t"]["chunk_beg"]).max()) == 0, "zero rows of G only"


def test_subsampled_graph():
    """Half the edges dropped by the subsample's own hash (the test backend's restatement of it): chunks left empty, nodes that keep
    their (empty) chunk and lose their last in-edge, in-degrees recomputed."""
    c = LC.BY_ID["subsampled"]
    parent = LC.snapshot(c, exact=False)
    assert parent.n == 300 and parent.number_of_edges() == 5000
    TB.set_backend(CpuTestBackend())
    try:
        sub = SN.device_subsample([parent], [LC.SUBSAMPLE_KEEP], [LC.SUBSAMPLE_SEED], CPU, c.R2, want_mask=True)[0]
    finally:
        TB.set_backend(None)
    dg = sub.device_graph(CPU, c.R2)
    beg, end, seg = (dg.view_tensor("by_dst", k).long() for k in ("chunk_beg", "chunk_end", "chunk_seg"))
    in_deg = dg.in_deg.long()
    assert sub.src.shape[0] == LC.SUBSAMPLE_KEEP and np.array_equal(np.bincount(sub.dst, minlength=300), in_deg.numpy())
    empty = end == beg
    both = int((in_deg[seg[empty]] == 0).sum())
    print("subsampled: %d of %d chunks emptied, %d nodes written by a chunk wave and by the in-degree loop" % (int(empty.sum()), empty.numel(), both))
    assert int(empty.sum()) >= 5 and both >= 5
    assert int((np.bincount(parent.dst, minlength=300) == 0).sum()) == 20 and int((in_deg == 0).sum()) >= 25
    t = PV.DevicePairView(dg, torch.from_numpy(sub.gids.astype(np.int32)), c.n_table, c.R2).t
    assert t["n_partial"] == 5000 // 128 + c.R2 * c.n_table + 1 and t["n_fix"] == 5000 // 128 + 1, "sized from the parent's array length"
    assert LC.predict_fix(t["n_fix"], t["n_partial"], c.d_out) == c.fix and int(t["a"].shape[0]) == 5000


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _reference(case, regime):
    G = LC.graph(case)
    snap = LC.snapshot(case, exact=regime == "exact")
    ops = LC.operands(case, G.n, regime, CPU)
    iso = case.routes == ("iso",)
    ref = LC.Reference(case, G.n, G.src, G.dst, G.rel, None if iso else G.ids, snap.nnorm, ops, CPU)
    return G, snap, ops, ref


EXACT_CASES = [c for c in LC.ALL + LC.ISO if "exact" in c.regimes]


@pytest.mark.parametrize("case", EXACT_CASES, ids=_ids(EXACT_CASES))
def test_exact_operands_are_exact(case):
    """every sum of |terms| -- a bound on every partial sum in any order -- stays below 2^24 of the smallest increment (a sixteenth:
    nnorm^2 >= 2^-4, integers otherwise)"""
    G, snap, ops, ref = _reference(case, "exact")
    worst = float(ref.pre_abs.max()) if ref.pre_abs.numel() else 0.0
    for k, v in ref.backward().items():
        if v is not None:
            worst = max(worst, float(v[1].max()))
            assert bool((v[0] * 16 == torch.round(v[0] * 16)).all())
    print("%s: largest sum |t| = %.0f sixteenths" % (case.id, worst * 16))
    assert worst * 16 < 2 ** 24
    assert bool((ref.pre * 16 == torch.round(ref.pre * 16)).all())
    assert set(np.unique(snap.nnorm)) <= {1.0, 0.5, 0.25}


CPU_CASES = LC.UP_TO_HUBDST + LC.ISO


def _buf(x, rows):
    b = LC.guarded(torch, rows, x.shape[-1], CPU)
    b[:rows] = x.reshape(rows, -1)
    return b


@pytest.mark.parametrize("case", CPU_CASES, ids=_ids(CPU_CASES))
def test_cpu_backend_meets_the_bars(case):
    """The fp32 test backend (the views, chunks and fix-up order of the kernels) against the fp64 reference over the plain edge list:
    bit for bit on the integer operands, inside the bar on the wide ones; few elements at the ReLU's edge; the gradient formulas
    written out give what autograd gives."""
    be = CpuTestBackend()
    iso = case.routes == ("iso",)
    for regime in case.regimes:
        G, snap, ops, ref = _reference(case, regime)
        drop, has_bias = LC.drop_arg(ops), ops.bias is not None
        if iso:
            out = be.rgcn_isolated_fwd(ops.table, ops.loop_w, ops.bias, ops.act, drop)
            grads = be.rgcn_isolated_bwd(ops.table, out, ops.gy, ops.loop_w, has_bias, ops.act, drop)
            grads = (grads[0], None, grads[1], grads[2])
        else:
            dg = snap.device_graph(CPU, case.R2)
            ids = torch.from_numpy(G.ids.astype(np.int32))
            inv = TF.gather_inverse(G.ids, case.n_table, CPU)
            out = be.rgcn_table_fwd(dg, ops.table, ids, ops.weight, ops.loop_w, ops.bias, case.B, ops.act, drop)
            grads = be.rgcn_table_bwd(dg, ops.table, ids, inv, out, ops.gy, ops.weight, ops.loop_w, has_bias, case.B, ops.act, drop)
        problems, ratios = [], {}
        p, ratios["out"] = LC.compare("out", _buf(out, G.n), G.n, ref.out, ref.pre_abs, regime)
        problems += p
        mask = out > 0 if ops.act == LC.RELU else None
        edge = ref.relu_edge()
        if mask is not None:
            assert bool((~(mask != ref.mask) | edge).all()), "the ReLU masks differ away from the edge"
        if regime == "wide":
            assert int(edge.sum()) <= LC.RELU_EDGE_CAP * edge.numel(), "%d of %d elements at the ReLU's edge" % (int(edge.sum()), edge.numel())
        want = ref.backward(mask)
        for name, got in zip(("d_table", "d_weight", "d_loop_w", "d_bias"), grads):
            if got is None or want[name] is None:
                assert name == "d_weight" and iso or name == "d_bias" and not has_bias
                continue
            val, sabs = want[name]
            p, ratios[name] = LC.compare(name, _buf(got, val.shape[0]), val.shape[0], val, sabs, regime)
            problems += p
        written = ref.explicit_backward(ref.mask if mask is None else mask, lambda v: v)
        for name, v in written.items():
            if want[name] is not None and not (iso and name == "d_weight"):
                assert bool(((v - want[name][0]).abs() <= 1e-12 * want[name][1]).all()), "%s: the written-out formula and autograd disagree" % name
        print("%s %s: max err/bar %s" % (case.id, regime, {k: "%.3f" % v for k, v in ratios.items()}))
        assert not problems, "; ".join(problems)


WIDE_RELU = [c for c in LC.ALL + LC.ISO if "wide" in c.regimes and c.flags[1] == LC.RELU and c not in CPU_CASES and c.graph != "subsampled"]


@pytest.mark.parametrize("case", WIDE_RELU, ids=_ids(WIDE_RELU))
def test_few_elements_at_the_relu_edge(case):
    """the cap of test_cpu_backend_meets_the_bars for the wide ReLU cases that do not run there (`subsampled`, whose edges the device
    picks, asserts it in the GPU test)"""
    edge = _reference(case, "wide")[3].relu_edge()
    assert int(edge.sum()) <= LC.RELU_EDGE_CAP * edge.numel(), "%d of %d elements at the ReLU's edge" % (int(edge.sum()), edge.numel())


def test_zero_rows_of_the_reference():
    """what the GPU test asserts as exact zeros is zero in the reference: table rows nobody gathers, relation rows without edges"""
    G, snap, ops, ref = _reference(LC.BY_ID["small_d32_b32_f2"], "wide")
    b = ref.backward()
    assert bool((b["d_table"][0][34:] == 0).all()) and bool((b["d_table"][1][34:] == 0).all()) and bool((b["d_table"][0][:34] != 0).any())
    assert bool((b["d_weight"][0][5] == 0).all()) and bool((b["d_weight"][1][5] == 0).all())
    assert ref.zero_row_epilogue().shape[0] == int((np.bincount(G.dst, minlength=G.n) == 0).sum()) >= 10


@pytest.mark.parametrize("regime", ["exact", "wide"])
def test_comparison_helper_rejects(regime):
    """one element off by three bars, two swapped rows, one NaN, one changed guard word"""
    G, snap, ops, ref = _reference(LC.BY_ID["small_d32_b32_f0"], regime)
    good = _buf(ref.out.float(), G.n)
    ok = lambda b: LC.compare("out", b, G.n, ref.out, ref.pre_abs, regime)[0]
    assert ok(good) == []
    i, j = [int(v) for v in torch.nonzero(ref.pre_abs > 0)[17]]
    b = good.clone()
    b[i, j] += float(3 * LC.BAR * ref.pre_abs[i, j])
    assert b[i, j] != good[i, j] and len(ok(b)) == 1
    b = good.clone()
    r0, r1 = [int(r) for r in torch.nonzero((good[:G.n] != good[0]).any(1))[:2, 0]]
    b[[r0, r1]] = good[[r1, r0]]
    assert not torch.equal(b, good) and len(ok(b)) == 1
    b = good.clone()
    b[G.n // 2, 3] = float("nan")
    assert len(ok(b)) >= 1
    b = good.clone()
    b.view(torch.int32)[G.n + 7, 5] += 1                      # (still a NaN: another bit pattern)
    assert ok(b) == ["out: guard rows were written"]
    assert ok(good[:G.n + LC.GUARD - 1]) == ["out: guard rows were written"]


def test_restatements_of_the_host_constants():
    assert LC.fix_huge(35624) == 2048 and LC.fix_huge(4095 * 2049) == 2049 and LC.FIX_SPLIT_MIN == 32768
    assert PV.PAIR_CHUNK == 128 and _lib.CHUNK == 64
    assert LC.pair_tail_grid(0) == (1, 1) and LC.pair_tail_grid(1024) == (128, 1) and LC.pair_tail_grid(1025) == (65, 2)
