"""The serial tail of the pair route (temp_rgcn_pair_fwd / _bwd): the one-pass P-row kernel of the backward (d_table and the
relation weights from one read of G), the self-loop branch beside the gather, and the forward epilogue without its own scan of
in_deg.  The table route on the same graph is the reference, at the bars of tests/test_gpu_pair_route.py (compare_routes, which
also runs every case twice and asks for the same bits)."""
import functools

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import pair_view as PV
from temp_amd.snapshot import Snapshot
from tests.test_gpu_pair_route import compare_routes, pair_view
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
DROP = (0.3, 0x5EED1234)


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    lib = _lib.load()
    prev = [(k, lib.temp_get_option(k)) for k in (_lib.OPT_RGCN_PAIR, _lib.OPT_OVERLAP)]
    yield be
    for k, v in prev:
        lib.temp_set_option(k, v)


@functools.lru_cache(maxsize=None)
def tiling_graph(n_table, R2):
    """3000 nodes, ~10^4 edges: the last relation row and (where the table has more than three rows) the last three table rows
    are used by no edge, one (relation 0, table row 0) pair has more than PAIR_CHUNK edges, 200 nodes have no incoming edge."""
    rng = np.random.default_rng(1000 * n_table + R2)
    n, E_hub, E_rest = 3000, 3 * PV.PAIR_CHUNK, 9000
    ids_np = rng.integers(0, max(1, n_table - 3), n)
    ids_np[:40] = 0
    hub_src = np.nonzero(ids_np == 0)[0]
    src = np.concatenate([rng.choice(hub_src, E_hub), rng.integers(0, n, E_rest)])
    rel = np.concatenate([np.zeros(E_hub, np.int64), rng.integers(0, R2 - 1, E_rest)])
    dst = rng.integers(0, n - 200, E_hub + E_rest)
    return Snapshot(n, src, dst, rel, np.arange(n)), ids_np


@pytest.mark.parametrize("D,B", [(200, 100), (64, 16), (32, 32), (256, 128)])
@pytest.mark.parametrize("R2", [2, 5, 42])
@pytest.mark.parametrize("n_table", [1, 37, 130])
def test_pair_tail_tiling_edges(n_table, R2, D, B, hip_backend):
    """Table sizes and relation counts that are no multiple of the pass's tile (8 table rows) or of its waves' shares of the
    relation rows; block sizes 2, 4 and 1; 50, 16, 8 and all 64 lanes of a row active."""
    g, ids_np = tiling_graph(n_table, R2)
    pv = compare_routes(hip_backend, g, R2, n_table, ids_np, D, B, True, 1, None, n_table + R2 + D, "tail %d x %d, %d/%d" % (n_table, R2, D, B))
    seg = pv.t["chunk_seg"].cpu().numpy()
    assert (seg == 0).sum() > 1, "the hub pair was meant to span several chunks"
    fwd_row = pv.t["fwd_row"].cpu().numpy()
    assert not (fwd_row // n_table == R2 - 1).any(), "the last relation row was meant to stay unused"


def test_pair_tail_table_of_several_tiles_per_block(hip_backend):
    """More table rows than 128 tiles of 8: a block of the pass walks several tiles and sums its relation-weight part over them."""
    rng = np.random.default_rng(11)
    n, n_table, R2, E = 4000, 1031, 3, 12000
    ids_np = rng.integers(0, n_table, n)
    g = Snapshot(n, rng.integers(0, n, E), rng.integers(0, n, E), rng.integers(0, R2, E), np.arange(n))
    compare_routes(hip_backend, g, R2, n_table, ids_np, 64, 16, False, 0, None, 5, "tail 1031 x 3")


def _bwd_inputs(be, g, R2, n_table, ids_np, D, B, bias, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    Sb = D // B
    table, w, lw = f(n_table, D), f(R2, B * Sb * Sb) * 0.5, f(D, D) * 0.2
    b = f(D) if bias else None
    gy = f(g.n, D)
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(DEV)
    inv = TF.gather_inverse(ids_np, n_table, DEV)
    dg = g.device_graph(DEV, R2)
    return dg, pair_view(be, dg, ids, n_table), table, ids, inv, w, lw, b, gy


@pytest.mark.parametrize("drop", [None, DROP])
@pytest.mark.parametrize("bias,act", [(True, 1), (False, 0)])
def test_pair_bwd_branch_on_equals_off(bias, act, drop, hip_backend):
    """The self-loop branch on the side stream (TEMP_OPT_OVERLAP 1) and in the caller's stream (0): the same launches, so every
    gradient has the same bits."""
    be, lib = hip_backend, hip_backend.lib
    g, ids_np = tiling_graph(130, 5)
    dg, pv, table, ids, inv, w, lw, b, gy = _bwd_inputs(be, g, 5, 130, ids_np, 200, 100, bias, 21)
    out = be.rgcn_pair_fwd(dg, pv, table, ids, w, lw, b, 100, act, drop)
    res = []
    for overlap in (0, 1, 0, 1):
        lib.temp_set_option(_lib.OPT_OVERLAP, overlap)
        res.append(be.rgcn_pair_bwd(dg, pv, table, ids, inv, out, gy, w, lw, bias, 100, act, drop))
    torch.cuda.synchronize()
    for other in res[1:]:
        for name, x, y in zip(("d_table", "d_weight", "d_loop", "d_bias"), res[0], other):
            assert (x is None and y is None) or torch.equal(x, y), "branch on / off: %s differs" % name
    assert all(bool(torch.isfinite(x).all()) for x in res[0] if x is not None)


def test_pair_fwd_bwd_captured_replays_equal_eager(hip_backend):
    """Pair forward + backward inside a captured graph (the side branch becomes a parallel branch of it): two replays give the
    eager bits."""
    be = hip_backend
    g, ids_np = tiling_graph(37, 5)
    dg, pv, table, ids, inv, w, lw, b, gy = _bwd_inputs(be, g, 5, 37, ids_np, 200, 100, True, 31)

    def step():
        out = be.rgcn_pair_fwd(dg, pv, table, ids, w, lw, b, 100, 1, None)
        return (out,) + tuple(be.rgcn_pair_bwd(dg, pv, table, ids, inv, out, gy, w, lw, True, 100, 1, None))

    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        for _ in range(2):
            eager = [x.clone() for x in step()]
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(("out", "d_table", "d_weight", "d_loop", "d_bias"), eager, held):
            assert torch.equal(x, y), "replay %d: %s differs from the eager run" % (rep, name)
        for y in held:
            y.fill_(float("nan"))                  # the second replay has to write everything again


def test_pair_fwd_epilogue_without_and_with_fix_entries(hip_backend):
    """Nodes without an incoming edge are finished by the gather itself.  First graph: no destination has more than one chunk, so
    the by-destination view lists no fix entry and the forward is the message product, the loop product and the gather alone;
    second graph: a hub destination as well."""
    rng = np.random.default_rng(8)
    n, n_table, R2, E = 5000, 90, 6, 9000
    ids_np = rng.integers(0, n_table, n)
    src, rel = rng.integers(0, n, E), rng.integers(0, R2, E)
    dst = rng.permutation(np.repeat(np.arange(1000, 4000), 3))[:E]          # in-degree <= 3; nodes < 1000 and >= 4000 isolated
    g = Snapshot(n, src, dst, rel, np.arange(n))
    assert g.device_graph(DEV, R2).c.by_dst.n_fix == 0
    compare_routes(hip_backend, g, R2, n_table, ids_np, 200, 100, True, 1, None, 1, "isolated nodes, no fix entry")
    compare_routes(hip_backend, g, R2, n_table, ids_np, 32, 32, False, 0, DROP, 2, "isolated nodes, no fix entry, dropout")
    dst2 = dst.copy()
    dst2[:700] = 2000                                                       # one destination with > 700 edges: many chunks
    g2 = Snapshot(n, src, dst2, rel, np.arange(n))
    assert g2.device_graph(DEV, R2).c.by_dst.n_fix == 1
    compare_routes(hip_backend, g2, R2, n_table, ids_np, 200, 100, True, 1, None, 3, "isolated nodes and a hub")

