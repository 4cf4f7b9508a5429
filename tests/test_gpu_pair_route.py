"""Pair route of the table-fed RGCN layer (temp_rgcn_pair_fwd / _bwd, include/temp_amd.h: TempPairView) on the GPU:
against the table route on the same graph (tolerances of test_rgcn_table_layer_equals_gather_then_layer), bit-repeatable,
selected where -- and only where -- the graph has many edges per (relation, table row) pair, and end to end in an encoder step."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import pair_view as PV
from temp_amd import snapshot as S
from temp_amd.snapshot import Snapshot
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    lib = _lib.load()
    prev = lib.temp_get_option(_lib.OPT_RGCN_PAIR)
    yield be
    lib.temp_set_option(_lib.OPT_RGCN_PAIR, prev)


def pair_view(be, dg, ids, n_table):
    return PV.DevicePairView(dg, ids, n_table, dg.n_rel_rows, expand=be.expand_chunk_segments)


def compare_routes(be, g, R2, n_table, ids_np, D, B, bias, act, drop, seed, what):
    """temp_rgcn_pair_fwd/bwd against temp_rgcn_table_fwd/bwd on graph g, twice (bitwise repeatable)."""
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    n, Sb = g.n, D // B
    table, w, lw = f(n_table, D), f(R2, B * Sb * Sb) * 0.5, f(D, D) * 0.2
    b = f(D) if bias else None
    gy = f(n, D)
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(DEV)
    inv = TF.gather_inverse(ids_np, n_table, DEV)
    dg = g.device_graph(DEV, R2)
    pv = pair_view(be, dg, ids, n_table)
    before = be.lib.temp_pair_launches()
    want = be.rgcn_table_fwd(dg, table, ids, w, lw, b, B, act, drop)
    got = be.rgcn_pair_fwd(dg, pv, table, ids, w, lw, b, B, act, drop)
    assert_close(got, want, 1e-5, 5e-6, what + " fwd")
    wd = be.rgcn_table_bwd(dg, table, ids, inv, want, gy, w, lw, bias, B, act, drop)
    gd = be.rgcn_pair_bwd(dg, pv, table, ids, inv, got, gy, w, lw, bias, B, act, drop)
    scale = max(1.0, float(n) ** 0.5)
    assert_close(gd[0], wd[0], 2e-5, 1e-5 * max(1.0, (n / n_table) ** 0.5), what + " d_table")
    assert_close(gd[1], wd[1], 2e-5, 1e-5 * scale, what + " d_weight")
    assert_close(gd[2], wd[2], 2e-5, 1e-5 * scale, what + " d_loop")
    if bias:
        assert_close(gd[3], wd[3], 2e-5, 1e-5 * scale, what + " d_bias")
    if n > 0:
        assert be.lib.temp_pair_launches() == before + 2
    # the same inputs again, through a view built again: the same bits
    pv2 = pair_view(be, dg, ids, n_table)
    for k, x in pv.t.items():
        assert torch.equal(x, pv2.t[k]) if torch.is_tensor(x) else x == pv2.t[k], "pair view not reproducible: " + k
    got2 = be.rgcn_pair_fwd(dg, pv2, table, ids, w, lw, b, B, act, drop)
    gd2 = be.rgcn_pair_bwd(dg, pv2, table, ids, inv, got2, gy, w, lw, bias, B, act, drop)
    assert torch.equal(got, got2), what + ": forward not bitwise repeatable"
    for x, y in zip(gd, gd2):
        assert (x is None and y is None) or torch.equal(x, y), what + ": backward not bitwise repeatable"
    return pv


def gdelt_union(n_members=5, keep_frac=0.5):
    """A multi-member union of GDELT-shaped snapshots whose last member is subsampled ON THE DEVICE (no host arrays)."""
    from temp_amd import synthetic
    w = synthetic.workload("S-gdelt", seed=0)
    R2 = 2 * w["num_rels"]
    parts = [w["snapshots"][t] for t in (3, 40, 7, 103, 12, 200, 61, 5, 90)[:n_members]]
    tgt = w["snapshots"][33]
    sub = S.device_subsample([tgt], [int(tgt.number_of_edges() * keep_frac)], [12345], DEV, R2)[0]
    return S.batch(parts + [sub]), R2, w["num_ents"]


@pytest.mark.parametrize("D,B", [(200, 100), (64, 16), (32, 32)])
@pytest.mark.parametrize("bias,act", [(True, 1), (False, 0), (False, 1), (True, 0)])
def test_pair_route_equals_table_route_gdelt_union(D, B, bias, act, hip_backend):
    g, R2, n_table = gdelt_union()
    assert isinstance(g.parts[-1], S.SubsampledSnapshot)
    compare_routes(hip_backend, g, R2, n_table, g.gids, D, B, bias, act, None, D + B + act, "gdelt union %d/%d" % (D, B))


@pytest.mark.parametrize("D,B,bias,act", [(200, 100, True, 1), (64, 16, False, 0), (32, 32, True, 0)])
def test_pair_route_with_self_loop_dropout(D, B, bias, act, hip_backend):
    g, R2, n_table = gdelt_union(n_members=2)
    compare_routes(hip_backend, g, R2, n_table, g.gids, D, B, bias, act, (0.3, 0x5EED1234), 7 + D, "dropout %d/%d" % (D, B))


@pytest.mark.parametrize("D,B", [(200, 100), (32, 32)])
def test_pair_route_hub_pair_empty_pairs_and_isolated_nodes(D, B, hip_backend):
    """One (relation, table row) pair with more than 10 000 edges (many chunks, the ordered fix-up), a relation row and table rows
    that no edge uses (zero rows of G), nodes without incoming edges (the epilogue-only rows of the forward)."""
    rng = np.random.default_rng(5)
    n, n_table, R2, E_hub, E_rest = 14000, 60, 8, 11000, 6000
    ids_np = rng.integers(0, n_table - 5, n)              # the last five table rows are never gathered
    hub_src = np.nonzero(ids_np == 9)[0]
    src = np.concatenate([rng.choice(hub_src, E_hub), rng.integers(0, n, E_rest)])
    rel = np.concatenate([np.full(E_hub, 3), rng.integers(0, R2 - 1, E_rest)])       # relation row R2 - 1 never occurs
    dst = np.concatenate([rng.permutation(12000)[:E_hub], rng.integers(0, 12000, E_rest)])   # nodes >= 12000: no incoming edge
    g = Snapshot(n, src, dst, rel, np.arange(n))
    pv = compare_routes(hip_backend, g, R2, n_table, ids_np, D, B, True, 1, None, 3, "hub pair %d/%d" % (D, B))
    seg = pv.t["chunk_seg"].cpu().numpy()
    assert (seg == 3 * n_table + 9).sum() > 10000 // PV.PAIR_CHUNK


def test_pair_route_equals_table_route_headline_union(hip_backend):
    """The headline's ratio (163 snapshots, 60 edges per pair, D/B = 200/100): forward and every gradient at the same bars."""
    from temp_amd import synthetic
    w = synthetic.workload("S-gdelt", seed=0)
    g = S.batch([w["snapshots"][t] for t in range(0, 326, 2)])
    compare_routes(hip_backend, g, 2 * w["num_rels"], w["num_ents"], g.gids, w["D"], w["B"], True, 1, None, 163, "headline union")


def test_pair_route_empty_graph(hip_backend):
    z = np.zeros(0, np.int64)
    g = Snapshot(50, z, z, z, np.arange(50))
    compare_routes(hip_backend, g, 6, 20, np.arange(50) % 20, 16, 8, True, 1, None, 1, "no edges")
    compare_routes(hip_backend, g, 6, 20, np.arange(50) % 20, 32, 32, False, 0, None, 2, "no edges, 1 x 1 blocks")


def test_pair_route_refuses_unsupported_shapes(hip_backend):
    lib = hip_backend.lib
    assert lib.temp_rgcn_pair_supported(200, 200, 100) == 1 and lib.temp_rgcn_pair_supported(128, 128, 128) == 1
    assert lib.temp_rgcn_pair_supported(24, 24, 4) == 0           # 6 x 6 blocks: the generic kernels only
    assert lib.temp_rgcn_pair_supported(260, 260, 130) == 0       # wider than the fast path
    assert lib.temp_rgcn_pair_supported(64, 32, 16) == 0


def _layer(D, B, R2):
    import argparse
    from temp_amd.rgcn import RGCNLayer
    torch.manual_seed(3)
    args = argparse.Namespace(inv_temperature=0.1, learnable_lambda=False, impute=False)
    return RGCNLayer(args, D, D, R2, B, [0], activation=torch.relu, self_loop=True).to(DEV)


def _conv_table(layer, g, table, ids_np):
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(DEV)
    inv = TF.gather_inverse(ids_np, table.shape[0], DEV)
    layer.prepare_table(g, table.shape[0], ids)
    t = table.clone().requires_grad_(True)
    out = layer.conv_table(g, t, ids, inv)
    (out * out).sum().backward()
    return out.detach(), t.grad


def test_route_selection(hip_backend):
    """Auto (the default) takes the pair route on a headline-shaped union and leaves a 9-member union (3.2 edges per pair) and an
    ICEWS-shaped one on the table route; with the option at 0 nothing takes it; the bits 4 / 8 switch off one half each."""
    from temp_amd import synthetic
    lib = hip_backend.lib
    assert lib.temp_get_option(_lib.OPT_RGCN_PAIR) == 1, "auto is the default"
    w = synthetic.workload("S-gdelt", seed=0)
    R2, N, D, B = 2 * w["num_rels"], w["num_ents"], w["D"], w["B"]
    layer = _layer(D, B, R2)
    table = torch.randn(N, D, device=DEV)
    count = lib.temp_pair_launches

    big = S.batch([w["snapshots"][t] for t in range(0, 326, 2)])           # 163 distinct snapshots: the headline's union
    assert big.number_of_edges() >= 50 * R2 * N
    c0 = count()
    out_pair, dt_pair = _conv_table(layer, big, table, big.gids)
    assert count() == c0 + 2, "the headline-shaped union did not take the pair route (forward + backward)"

    nine = S.batch([w["snapshots"][t] for t in range(9)])
    assert nine.number_of_edges() < PV.PAIR_MIN_RATIO * R2 * N
    c0 = count()
    _conv_table(layer, nine, table, nine.gids)
    assert count() == c0, "a 9-member union must keep the table route"

    wi = synthetic.workload("S-icews14", seed=0)
    Ri, Ni = 2 * wi["num_rels"], wi["num_ents"]
    li = _layer(wi["D"], wi["B"], Ri)
    icews = S.batch([wi["snapshots"][t] for t in range(60)])
    c0 = count()
    _conv_table(li, icews, torch.randn(Ni, wi["D"], device=DEV), icews.gids)
    assert count() == c0, "an ICEWS-shaped union must keep the table route"

    big2 = S.batch([w["snapshots"][t] for t in range(0, 326, 2)])          # a fresh union: nothing cached on it
    lib.temp_set_option(_lib.OPT_RGCN_PAIR, 0)
    c0 = count()
    out_off, dt_off = _conv_table(layer, big2, table, big2.gids)
    assert count() == c0, "option 0: nothing takes the pair route"
    assert_close(out_pair, out_off, 1e-5, 5e-6, "headline union: pair vs table route")

    for opt, moved in ((1 | 4, 1), (1 | 8, 1), (2 | 4 | 8, 0)):            # forward off / backward off / both off
        lib.temp_set_option(_lib.OPT_RGCN_PAIR, opt)
        c0 = count()
        _conv_table(layer, big, table, big.gids)
        assert count() == c0 + moved, "option %d" % opt

    lib.temp_set_option(_lib.OPT_RGCN_PAIR, 2)                             # forced: also where auto would not
    c0 = count()
    _conv_table(layer, nine, table, nine.gids)
    assert count() == c0 + 2


def test_encoder_step_forced_equals_off(hip_backend):
    """One BiDynamicRGCN encoder step (prepare + run + backward) with the pair route forced against the route off: outputs and
    every parameter gradient within the window tests' bars (tests/window_cases.py: batched vs generic)."""
    import bench
    from temp_amd import synthetic
    lib = hip_backend.lib
    w = synthetic.workload("S-tiny", seed=0)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    res = []
    for opt in (0, 2):
        lib.temp_set_option(_lib.OPT_RGCN_PAIR, opt)
        model = bench.build_model(w, DEV)
        model.sample_rng = np.random.default_rng(2)
        c0 = lib.temp_pair_launches()
        wb = model.prepare(targets, w["L"], train=True)
        out = model.run(wb)[0]
        (out * out).sum().backward()
        assert lib.temp_pair_launches() - c0 == (2 if opt else 0)
        res.append((out.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in model.named_parameters() if v.grad is not None}))
    (o0, g0), (o1, g1) = res
    assert_close(o1, o0, 1e-5, 2e-6, "encoder step: forced vs off")
    assert set(g0) == set(g1) and len(g0) >= 8
    for k in g0:
        assert_close(g1[k], g0[k], 1e-4, 3e-6 * max(1.0, float(g0[k].abs().max())), "encoder step forced vs off: d_" + k)
