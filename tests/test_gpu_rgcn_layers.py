"""The table-fed RGCN layer (temp_rgcn_table_fwd / _bwd), its pair route (temp_rgcn_pair_fwd / _bwd) and the isolated layer
(temp_rgcn_isolated_fwd / _bwd) on the MI355X, each against the fp64 layer over the plain edge list -- a reference that shares
nothing with another HIP route (tests/rgcn_layer_cases.py; tests/test_rgcn_layer_cases_cpu.py checks the host-side facts the cases
rest on and the reference itself).

A case calls the C ABI directly, with the library's default options.  Every output is NaN-filled with 64 guard rows and every
workspace, sized by its *_workspace query, holds NaN bit patterns before every call.  Checked per case, regime and entry point:
  * exact data: the forward and every gradient equal the fp64 value bit for bit;
  * wide data: every element is finite and within 2e-6 of sum |t| (the bar of the split-operand dense products, which the loop term
    goes through); an element whose terms are all zero is exactly zero;
  * under a ReLU the backward reference takes the mask of the kernel's own forward, which may differ from the fp64 mask only where
    the pre-activation lies within the bar of zero -- at most 0.1 % of the elements;
  * d_table rows nobody gathers and d_weight rows of unused relations are exactly 0; the out rows of nodes without in-edges carry the
    bits the same call gives on the graph without its edges (the epilogue of a zero row); guard rows keep their bits;
  * a second call on freshly poisoned buffers gives the same bits (the split fix-up's list order may vary, its sums may not);
  * pair route: temp_pair_launches moves by one per call; the fix-up launches counted over the backward are exactly the case's; the
    kernel trace has k_pair_fix_epi iff the by-destination view has multi-chunk segments and k_reduce_slices behind k_pair_tail iff
    the tail runs more than one block; generic shapes are refused with nothing launched and nothing written.
Pair and table route meet the fp64 bars independently: there is no pair-versus-table tolerance.

Measured on the MI355X, worst |got - ref| / (2e-6 sum |t|) over all cases of a kind (wide data; exact data: 0 everywhere):
  case        route  out    d_table  d_weight  d_loop_w  d_bias
  small       table  0.177  0.196    0.216     0.164     0.040
  small       pair   0.177  0.196    0.113     0.164     0.040
  generic     table  0.121  0.091    0.121     0.072     0.021
  one         table  0.058  0.016    0.025     0.032     0.029
  one         pair   0.058  0.016    0.169     0.032     0.029
  rel9        table  0.119  0.107    0.110     0.087     0.024
  rel9        pair   0.119  0.107    0.077     0.087     0.024
  rel42       table  0.109  0.102    0.083     0.094     -
  rel42       pair   0.109  0.102    0.115     0.094     -
  tiles       table  0.184  0.161    0.026     0.026     0.011
  tiles       pair   0.184  0.161    0.052     0.025     0.011
  hubdst      table  0.132  0.195    0.143     0.132     0.028
  hubdst      pair   0.132  0.195    0.092     0.132     0.028
  members     table  0.136  0.120    0.056     0.121     0.031
  members     pair   0.136  0.131    0.054     0.137     0.031
  subsampled  table  0.206  0.105    0.072     0.056     0.020
  subsampled  pair   0.206  0.105    0.114     0.049     0.020
  noedges     table  0.090  0.061    0         0.076     0.021
  noedges     pair   0.090  0.061    0         0.076     0.021
  isolated    -      0.197  0.235    -         0.141     0.031      (d_table: d_e)
fixmany, splitfew and splitlisted run on exact data only.  The whole module takes 3 s: the largest case (splitlisted, 300 000 edges) 0.4 s,
most of it the fp64 reference on the host.  With one summand dropped from the wave reduction of k_pair_tail, from k_pair_fix_epi's
walk and from k_fixup_split's final addition (a build made for this check, not kept), rel42, fixmany, splitfew, splitlisted and hubdst
fail -- hubdst on wide data at 34 bars -- and every other case passes."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import pair_view as PV
from temp_amd import snapshot as SN
from tests import rgcn_layer_cases as LC
from tests import rgcn_route_cases as RC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
from tests.test_gpu_row_loss_routes import _traced

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
E_UNSUPPORTED = 2                                            # include/temp_amd.h: TEMP_E_UNSUPPORTED
GRADS = ("d_table", "d_weight", "d_loop_w", "d_bias")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    lib = _lib.load()
    prev = lib.temp_get_option(_lib.OPT_RGCN_PAIR)
    yield be
    lib.temp_set_option(_lib.OPT_RGCN_PAIR, prev)
    TB.set_backend(None)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poisoned(nbytes):
    """a workspace of at least nbytes whose every word is a NaN bit pattern"""
    return torch.full((int(nbytes) // 4 + 64,), float("nan"), device=DEV)


def _nan(rows, cols):
    return LC.guarded(torch, rows, cols, DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _routes(lib):
    return [[lib.temp_rgcn_route_launches(r, s) for s in range(RC.S_CELLS)] for r in range(len(RC.ROUTES))]


def _delta(lib, before):
    after = _routes(lib)
    return {(RC.ROUTES[r], s): after[r][s] - before[r][s] for r in range(len(RC.ROUTES)) for s in range(RC.S_CELLS) if after[r][s] != before[r][s]}


def _drop(ops):
    if ops.p <= 0:
        return None, None
    d = _lib.TempDropout()
    d.p, d.seed = float(ops.p), LC.DROP_SEED
    return d, ctypes.byref(d)


class GraphSite:
    """a case's graph on the device: the edge list the reference reads, the device graph, ids, their inverse, the pair view, and the
    same nodes without any edge (for the epilogue-of-a-zero-row check)"""

    def __init__(self, be, case, exact):
        G = LC.graph(case)
        snap = LC.snapshot(case, exact)
        if case.graph == "subsampled":
            snap = SN.device_subsample([snap], [LC.SUBSAMPLE_KEEP], [LC.SUBSAMPLE_SEED], DEV, case.R2, want_mask=True)[0]
            G = LC.Graph(G.n, snap.src, snap.dst, snap.rel, G.ids, None)              # (the kept edges, from the device's keep mask)
        self.G, self.snap, self.n = G, snap, G.n
        self.nnorm = np.asarray(snap.nnorm, np.float32)
        self.dg = snap.device_graph(DEV, case.R2)
        self.ids = torch.from_numpy(G.ids.astype(np.int32)).to(DEV)
        self.inv = TF.gather_inverse(G.ids, case.n_table, DEV)
        mk = lambda dg: PV.DevicePairView(dg, self.ids, case.n_table, case.R2, expand=be.expand_chunk_segments)      # (generic shapes too: to be refused)
        self.pv = mk(self.dg)
        self.in_deg = torch.from_numpy(np.bincount(G.dst, minlength=G.n)).to(DEV)
        assert torch.equal(self.dg.in_deg.long(), self.in_deg), "the device graph's in-degrees are not the edge list's"
        z = np.zeros(0, np.int64)
        self.empty_snap = SN.Snapshot(G.n, z, z, z, G.ids, nnorm=self.nnorm)
        self.empty_dg = self.empty_snap.device_graph(DEV, case.R2)
        self.empty_pv = mk(self.empty_dg)


@functools.lru_cache(maxsize=2)
def _site(graph, seed, R2, n_table, exact):
    case = LC.Case("", graph, seed, 0, 0, 1, R2, n_table, LC.FLAGS[0], (), (), {})
    return GraphSite(TB.get_backend(), case, exact)


class Calls:
    """the raw entry points of one case on one device graph; every call allocates NaN-filled, guarded outputs and a poisoned workspace"""

    def __init__(self, lib, case, site, ops, dg=None, pv=None):
        self.lib, self.c, self.s, self.o = lib, case, site, ops
        self.dg, self.pv = (dg or site.dg, pv or site.pv) if site is not None else (None, None)
        self.drop_keep, self.drop = _drop(ops)
        self.act, self.has_bias = ops.act, int(ops.bias is not None)

    def _grads(self):
        c = self.c
        return (_nan(c.n_table, c.d_in), _nan(c.R2, LC.wrow(c)), _nan(c.d_in, c.d_out), _nan(1, c.d_out) if self.has_bias else None)

    def table_fwd(self):
        c, o, g = self.c, self.o, self.dg.ref()
        out = _nan(self.s.n, c.d_out)
        ws = _poisoned(self.lib.temp_rgcn_table_fwd_workspace(g, c.n_table, c.d_out))
        rc = self.lib.temp_rgcn_table_fwd(g, _p(o.table), _p(self.s.ids), c.n_table, c.d_in, c.d_out, c.B, c.R2, _p(o.weight), _p(o.loop_w), _p(o.bias), self.act,
                                          _p(out), _p(ws), ws.numel() * 4, self.drop, _stream())
        torch.cuda.synchronize()
        return rc, out

    def table_bwd(self, out):
        c, o, g = self.c, self.o, self.dg.ref()
        d_t, d_w, d_l, d_b = self._grads()
        ws = _poisoned(self.lib.temp_rgcn_table_bwd_workspace(g, c.n_table, c.d_in, c.d_out, c.B))
        rc = self.lib.temp_rgcn_table_bwd(g, _p(o.table), _p(self.s.ids), _p(self.s.inv[0]), _p(self.s.inv[1]), c.n_table, _p(out), _p(o.gy), c.d_in, c.d_out, c.B,
                                          c.R2, _p(o.weight), _p(o.loop_w), self.has_bias, self.act, _p(d_t), _p(d_w), _p(d_l), _p(d_b), _p(ws), ws.numel() * 4,
                                          self.drop, _stream())
        torch.cuda.synchronize()
        return rc, (d_t, d_w, d_l, d_b)

    def pair_fwd(self):
        c, o, g, pv = self.c, self.o, self.dg.ref(), self.pv.ref()
        out = _nan(self.s.n, c.d_out)
        ws = _poisoned(self.lib.temp_rgcn_pair_fwd_workspace(g, pv, c.d_out))
        rc = self.lib.temp_rgcn_pair_fwd(g, pv, _p(o.table), _p(self.s.ids), c.n_table, c.d_in, c.d_out, c.B, c.R2, _p(o.weight), _p(o.loop_w), _p(o.bias), self.act,
                                         _p(out), _p(ws), ws.numel() * 4, self.drop, _stream())
        torch.cuda.synchronize()
        return rc, out

    def pair_bwd(self, out):
        c, o, g, pv = self.c, self.o, self.dg.ref(), self.pv.ref()
        d_t, d_w, d_l, d_b = self._grads()
        ws = _poisoned(self.lib.temp_rgcn_pair_bwd_workspace(g, pv, c.d_in, c.d_out, c.B))
        rc = self.lib.temp_rgcn_pair_bwd(g, pv, _p(o.table), _p(self.s.ids), _p(self.s.inv[0]), _p(self.s.inv[1]), c.n_table, _p(out), _p(o.gy), c.d_in, c.d_out,
                                         c.B, c.R2, _p(o.weight), _p(o.loop_w), self.has_bias, self.act, _p(d_t), _p(d_w), _p(d_l), _p(d_b), _p(ws),
                                         ws.numel() * 4, self.drop, _stream())
        torch.cuda.synchronize()
        return rc, (d_t, d_w, d_l, d_b)

    def iso_fwd(self):
        c, o = self.c, self.o
        out = _nan(c.n_table, c.d_out)
        rc = self.lib.temp_rgcn_isolated_fwd(c.n_table, c.d_in, _p(o.table), _p(o.loop_w), _p(o.bias), self.act, _p(out), self.drop, _stream())
        torch.cuda.synchronize()
        return rc, out

    def iso_bwd(self, out):
        c, o = self.c, self.o
        d_e, _, d_l, d_b = self._grads()
        ws = _poisoned(self.lib.temp_rgcn_isolated_bwd_workspace(c.n_table, c.d_in))
        rc = self.lib.temp_rgcn_isolated_bwd(c.n_table, c.d_in, _p(o.table), _p(out), _p(o.gy), _p(o.loop_w), self.has_bias, self.act, _p(d_e), _p(d_l), _p(d_b),
                                             _p(ws), ws.numel() * 4, self.drop, _stream())
        torch.cuda.synchronize()
        return rc, (d_e, None, d_l, d_b)


def _same_bits(xs, ys):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def run_route(lib, case, regime, route, site, ops, ref):
    """one entry-point pair of a case in one regime -> (problems, {quantity: worst err / bar})"""
    problems, ratios = [], {}
    bad = problems.append
    calls = Calls(lib, case, site, ops)
    fwd, bwd = {"table": (calls.table_fwd, calls.table_bwd), "pair": (calls.pair_fwd, calls.pair_bwd), "iso": (calls.iso_fwd, calls.iso_bwd)}[route]
    n = site.n if site is not None else case.n_table
    tag = "%s %s %s" % (case.id, regime, route)
    # ---- forward
    pairs0, routes0 = lib.temp_pair_launches(), _routes(lib)
    rc, out = fwd()
    _lib.check(rc, tag + " forward")
    fwd_delta = _delta(lib, routes0)
    if route == "pair":
        if lib.temp_pair_launches() != pairs0 + 1:
            bad("temp_pair_launches did not move by one over the forward")
        if fwd_delta:
            bad("the pair forward counted edge-kernel routes: %s" % sorted(fwd_delta))
    p, ratios["out"] = LC.compare("out", out, n, ref.out, ref.pre_abs, regime)
    problems += p
    mask = None
    if ops.act == LC.RELU:
        mask = (out[:n] > 0).cpu()
        edge = ref.relu_edge()
        if not bool((~(mask != ref.mask) | edge).all()):
            bad("the ReLU mask differs from the fp64 mask away from the ReLU's edge")
        if regime == "wide" and int(edge.sum()) > LC.RELU_EDGE_CAP * edge.numel():
            bad("%d of %d elements at the ReLU's edge" % (int(edge.sum()), edge.numel()))
    if route != "iso":
        lone = site.in_deg == 0
        if bool(lone.any()):                                  # the same call on the graph without its edges: the epilogue of a zero row
            rc0, out0 = getattr(Calls(lib, case, site, ops, site.empty_dg, site.empty_pv), route + "_fwd")()
            _lib.check(rc0, tag + " forward without edges")
            if not torch.equal(_bits(out[:n][lone]), _bits(out0[:n][lone])):
                bad("rows of nodes without in-edges are not the epilogue of a zero row")
    # ---- backward, against the reference under the kernel's own ReLU mask
    out_rows = out[:n].contiguous()
    pairs0, routes0 = lib.temp_pair_launches(), _routes(lib)
    rc, grads = bwd(out_rows)
    _lib.check(rc, tag + " backward")
    bwd_delta = _delta(lib, routes0)
    want = ref.backward(mask)
    for name, got in zip(GRADS, grads):
        if got is None:
            continue
        val, sabs = want[name]
        p, ratios[name] = LC.compare(name, got, val.shape[0], val, sabs, regime)
        problems += p
    if route != "iso":
        unused_rows = torch.ones(case.n_table, dtype=torch.bool, device=DEV)
        unused_rows[site.ids.long()] = False
        unused_rels = torch.ones(case.R2, dtype=torch.bool, device=DEV)
        unused_rels[torch.from_numpy(site.G.rel).to(DEV)] = False
        if not bool((grads[0][:case.n_table][unused_rows] == 0).all()):
            bad("d_table rows that nobody gathers are not exactly zero")
        if not bool((grads[1][:case.R2][unused_rels] == 0).all()):
            bad("d_weight rows of unused relations are not exactly zero")
    # ---- the same calls again on freshly poisoned buffers (the pair route's under the kernel trace)
    if route == "pair":
        (rc, out2), names_f = _traced(fwd)
        (rc2, grads2), names_b = _traced(lambda: bwd(out_rows))
        if lib.temp_pair_launches() != pairs0 + 3:
            bad("temp_pair_launches did not move by one per call")
        if bwd_delta != case.fix:
            bad("the pair backward's fix-up launched %s, the case pins %s" % (sorted(bwd_delta.items()), sorted(case.fix.items())))
        if ("k_pair_fix_epi" in names_f) != (site.dg.views["by_dst"]["n_fix"] > 0):
            bad("forward trace %s with by_dst n_fix = %d" % (names_f, site.dg.views["by_dst"]["n_fix"]))
        if names_f.count("k_pair_msg") != 1 or names_f.count("k_pair_gather<fwd>") != 1:
            bad("forward trace %s" % names_f)
        tail = names_b.index("k_pair_tail") if "k_pair_tail" in names_b else -2
        sliced = names_b[tail + 1:tail + 2] == ["k_reduce_slices"]
        if tail < 0 or names_b.count("k_pair_tail") != 1 or sliced != (LC.pair_tail_grid(case.n_table)[0] > 1) or names_b.count("k_pair_gather<bwd>") != 1:
            bad("backward trace %s with a tail of %d blocks" % (names_b, LC.pair_tail_grid(case.n_table)[0]))
    else:
        rc, out2 = fwd()
        rc2, grads2 = bwd(out_rows)
    _lib.check(rc or rc2, tag + " second call")
    if not torch.equal(_bits(out), _bits(out2)):
        bad("forward: two calls gave different bits")
    if not _same_bits(grads, grads2):
        bad("backward: two calls gave different bits")
    if route == "table":
        if case.graph == "hubdst" and fwd_delta.get(("fix_few", 0)) != 1:
            bad("table forward without its fix-up launch: %s" % sorted(fwd_delta))
        if case.graph == "members" and ("fwd_tile8", 2) not in fwd_delta:
            bad("table forward of a union with member tables off the tiled kernels: %s" % sorted(fwd_delta))
        if "pair" not in case.routes and not ({("fwd_generic", 0)} <= set(fwd_delta) and {("dx_generic", 0), ("dw_generic", 0)} <= set(bwd_delta)):
            bad("generic shape off the generic kernels: %s / %s" % (sorted(fwd_delta), sorted(bwd_delta)))
    return problems, ratios


def refused(lib, case, site, ops):
    """both pair calls on a generic shape: TEMP_E_UNSUPPORTED, nothing launched, nothing written"""
    calls = Calls(lib, case, site, ops)
    assert lib.temp_rgcn_pair_supported(case.d_in, case.d_out, case.B) == 0
    before = lib.temp_pair_launches()
    (rc, out), names = _traced(calls.pair_fwd)
    assert rc == E_UNSUPPORTED and names == [] and bool((_bits(out) == LC.NAN_BITS).all())
    (rc, grads), names = _traced(lambda: calls.pair_bwd(torch.zeros(site.n, case.d_out, device=DEV)))
    assert rc == E_UNSUPPORTED and names == [] and all(g is None or bool((_bits(g) == LC.NAN_BITS).all()) for g in grads)
    assert lib.temp_pair_launches() == before


def measure(case):
    """-> ({(regime, route): ratios}, problems).  Nothing is asserted here (a script can print the figures of every case).
    The fp64 reference runs on the host, once per regime, and is shared by the case's routes: 270 000 double-precision additions into
    the one row of a hub pair serialise on the device."""
    lib = _lib.load()
    report, problems = {}, []
    iso = case.routes == ("iso",)
    for regime in case.regimes:
        t0 = time.perf_counter()
        if iso:
            site, n = None, case.n_table
            z = np.zeros(0, np.int64)
            G, nnorm = LC.Graph(n, z, z, z, None, None), None
        else:
            site = _site(case.graph, case.seed, case.R2, case.n_table, regime == "exact")
            G, n, nnorm = site.G, site.n, site.nnorm
        t1 = time.perf_counter()
        host_ops = LC.operands(case, n, regime, CPU)
        ref = LC.Reference(case, n, G.src, G.dst, G.rel, G.ids, nnorm, host_ops, CPU)
        ref.backward()
        ops = LC.Operands(*[v.to(DEV) if torch.is_tensor(v) else v for v in host_ops])
        t2 = time.perf_counter()
        for route in case.routes:
            p, ratios = run_route(lib, case, regime, route, site, ops, ref)
            report[(regime, route)] = ratios
            problems += ["%s %s: %s" % (regime, route, x) for x in p]
            print("rgcn-layer %s %s %s: max err/bar %s" % (case.id, regime, route, " ".join("%s %.3f" % kv for kv in ratios.items())))
        if not iso and "pair" not in case.routes:
            refused(lib, case, site, ops)
        print("rgcn-layer %s %s: graph %.2f s, reference %.2f s, calls and checks %.2f s" % (case.id, regime, t1 - t0, t2 - t1, time.perf_counter() - t2))
    return report, problems


CASES = LC.ALL + LC.ISO


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_rgcn_layer(case):
    assert _lib.load().temp_get_option(_lib.OPT_RGCN_PAIR) == 1 and _lib.load().temp_get_option(_lib.OPT_RGCN_TILE) == 1, "library defaults"
    report, problems = measure(case)
    assert not problems, "; ".join(problems)


def test_subsampled_graph_on_the_device():
    """the device's own subsample of the case: chunks emptied, nodes that keep an empty chunk (written by the chunk's wave and by the
    in-degree loop), in-degrees and norms recomputed from the kept edges"""
    c = LC.BY_ID["subsampled"]
    site = _site(c.graph, c.seed, c.R2, c.n_table, False)
    dg = site.dg
    beg, end, seg = (dg.view_tensor("by_dst", k).long() for k in ("chunk_beg", "chunk_end", "chunk_seg"))
    empty = end == beg
    assert site.G.src.shape[0] == LC.SUBSAMPLE_KEEP and int(dg.view_tensor("by_dst", "a").shape[0]) == 5000
    assert int(empty.sum()) >= 5 and int((dg.in_deg.long()[seg[empty]] == 0).sum()) >= 5
    assert torch.equal(dg.nnorm.cpu(), torch.from_numpy(site.nnorm)), "1 / in-degree of the kept edges"
