"""Cases and the fp64 reference for the RGCN LAYER entry points that sit on top of the edge kernels (temp_amd/csrc/rgcn_kernels.hip):
the table-fed layer (temp_rgcn_table_fwd / _bwd), its pair route (temp_rgcn_pair_fwd / _bwd) and the isolated layer
(temp_rgcn_isolated_fwd / _bwd).  Shared by tests/test_rgcn_layer_cases_cpu.py (the host-side facts every case rests on) and
tests/test_gpu_rgcn_layers.py (the kernels against fp64).  Graph recipes are plain numpy; no GPU here.

The reference works from the plain edge list (src, rel, dst), `ids` and nnorm -- no view, no chunk, no test backend.  With
x = table[ids] (isolated: x = e):

    agg[v]  = nnorm[v]^2 * sum_{(u,r,v)} x[u] . BD(W[r])                  (0 for in-degree 0)
    loop[v] = (x[v] . loop_w) * keep[v, :] / (1 - p)                      (isolated: + e[v])
    out     = act(agg + loop + bias)

The backward is fp64 autograd of that expression with the ReLU mask given (so that it can be the mask of a kernel's own forward).
Beside every value the reference returns sum |t|: the same expression on absolute values, dropout and ReLU masks held fixed (the
forward's magnitude is the pre-activation's: max(., 0) moves no two numbers apart).

Data regimes:
  exact   nnorm = 2^-(node % 3), patterned integers (table, bias in [-4, 4]; weights, loop_w, gy in [-2, 2]), p = 0.5 (scale 2):
          every partial sum stays below 2^24 sixteenths, so the fp32 result is the fp64 value bit for bit in any summation order
  wide    reals over three decades, the graph's own 1 / in-degree, p = 0.25

Graphs (what their views look like is asserted in tests/test_rgcn_layer_cases_cpu.py):
  small        70 nodes, 400 edges into nodes 0..57 from nodes 12..69, relation row R2 - 1 unused, 37 table rows of which the last
               three are never gathered, repeated ids
  one          40 nodes, 300 edges, one relation, one table row: ONE pair of three chunks
  tiles        4 000 nodes, 12 000 edges, 3 relations, 1 031 table rows: 129 tiles of 8 table rows
  hubdst       small + 700 edges into node 5
  fixmany      3 000 nodes, 140 000 uniform edges, 8 relations, 200 table rows
  splitfew     3 000 nodes, 6 000 edges (300 of them in one pair), 64 relations, 520 table rows
  splitlisted  3 000 nodes, 300 000 edges (270 000 of them in one pair, 300 in another), 64 relations, 520 table rows
  members      snapshot.batch of uniform members (50, 150), (70, 300), (30, 0); one relation
  subsampled   300 nodes, 5 000 edges (nodes 200..279 with one or two in-edges, 280..299 with none), half the edges kept on the device
  noedges      50 nodes, no edge"""
import collections

import numpy as np

from tests.rgcn_route_cases import _pattern, _wide, exact_nnorm, first_difference  # noqa: F401  (re-exported)

BAR = 2e-6                          # of sum |t|: the project's bar for its split-operand dense products (the loop term goes through them)
RELU_EDGE_CAP = 1e-3                # at most this share of the elements may lie within the bar of the ReLU's edge
GUARD = 64                          # guard rows behind every output
NAN_BITS = 0x7FC00000               # what torch.full(..., nan) writes
FIX_SPLIT_MIN, FIX_LIST_CAP, FIX_HUGE_MIN = 1 << 15, 4096, 2048          # csrc/rgcn_kernels.hip
PT_TE, PT_WAVES, PT_MAX_BLOCKS = 8, 8, 128                               # csrc/rgcn_kernels.hip: k_pair_tail
DROP_SEED = 0x5EED1234
RELU, NONE = 1, 0                   # include/temp_amd.h: TEMP_ACT_*
# (has_bias, act, dropout)
FLAGS = ((1, RELU, False), (0, NONE, False), (1, RELU, True), (0, RELU, True))

Case = collections.namedtuple("Case", "id graph seed d_in d_out B R2 n_table flags regimes routes fix")


def _case(id, graph, d_in, d_out, B, R2, n_table, flags, regimes=("exact", "wide"), routes=("table", "pair"), fix="few", seed=1):
    """fix: the fix-up launches of ONE temp_rgcn_pair_bwd on the by-pair view ('few', 'many', 'few_split', 'many_split')"""
    want = {("fix_" + fix, 0): 1}
    if fix.endswith("_split"):
        want[("fix_split2", 0)] = 1
    return Case(id, graph, seed, d_in, d_out, B, R2, n_table, FLAGS[flags], tuple(regimes), tuple(routes), want if "pair" in routes else {})


ALL = []
for _D, _B in ((8, 2), (32, 32), (200, 100), (256, 64)):
    for _f in range(4):
        ALL.append(_case("small_d%d_b%d_f%d" % (_D, _B, _f), "small", _D, _D, _B, 6, 37, _f))
ALL.append(_case("generic_24_24_b4", "small", 24, 24, 4, 6, 37, 0, routes=("table",)))
ALL.append(_case("generic_64_32_b16", "small", 64, 32, 16, 6, 37, 3, routes=("table",)))
ALL.append(_case("one", "one", 32, 32, 32, 1, 1, 2))
ALL.append(_case("rel9", "small", 64, 64, 16, 9, 37, 0))
ALL.append(_case("rel42", "small", 64, 64, 16, 42, 37, 3))
ALL.append(_case("tiles", "tiles", 64, 64, 16, 3, 1031, 2))
ALL.append(_case("hubdst", "hubdst", 200, 200, 100, 6, 37, 2))
ALL.append(_case("fixmany", "fixmany", 32, 32, 32, 8, 200, 2, regimes=("exact",), fix="many"))
ALL.append(_case("splitfew", "splitfew", 32, 32, 32, 64, 520, 0, regimes=("exact",), fix="few_split"))
ALL.append(_case("splitlisted", "splitlisted", 32, 32, 32, 64, 520, 3, regimes=("exact",), fix="many_split"))
ALL.append(_case("members", "members", 200, 200, 100, 1, 37, 2))
ALL.append(_case("subsampled", "subsampled", 64, 64, 16, 6, 100, 0, regimes=("wide",)))      # (the device recomputes 1 / in-degree: no exact norms)
ALL.append(_case("noedges_d16_b8", "noedges", 16, 16, 8, 6, 20, 0))
ALL.append(_case("noedges_d32_b32", "noedges", 32, 32, 32, 6, 20, 1))
ISO = []
for _i, (_n, _d) in enumerate((n, d) for n in (1, 33, 777) for d in (8, 200, 256)):
    ISO.append(_case("iso_n%d_d%d" % (_n, _d), "iso%d" % _n, _d, _d, 1, 1, _n, _i % 4, routes=("iso",)))

BY_ID = {c.id: c for c in ALL + ISO}
assert len(BY_ID) == len(ALL) + len(ISO)
UP_TO_HUBDST = [c for c in ALL if c.graph in ("small", "one", "tiles", "hubdst")]
SUBSAMPLE_KEEP, SUBSAMPLE_SEED = 2500, 12345


# ---- graph recipes ------------------------------------------------------------------------------------------------------------
Graph = collections.namedtuple("Graph", "n src dst rel ids members")


def graph(case):
    """-> Graph: the plain edge list (for `subsampled`: the parent's), ids into the table, members = ((n, E), ...) of a batch"""
    rng = np.random.default_rng(case.seed)
    R2, T = case.R2, case.n_table
    g = case.graph
    i64 = lambda *xs: [np.asarray(x, dtype=np.int64) for x in xs]
    rels = lambda E: rng.integers(0, max(R2 - 1, 1), E)                   # (relation row R2 - 1 stays unused where R2 > 1)
    members = None
    if g in ("small", "hubdst"):
        n = 70
        src, dst = rng.integers(12, 70, 400), rng.integers(0, 58, 400)
        rel = rels(400)
        if g == "hubdst":
            src, dst, rel = np.concatenate([src, rng.integers(12, 70, 700)]), np.concatenate([dst, np.full(700, 5)]), np.concatenate([rel, rels(700)])
        ids = rng.integers(0, T - 3, n)
    elif g == "one":
        n = 40
        src, dst, rel, ids = rng.integers(0, n, 300), rng.integers(0, n, 300), np.zeros(300), np.zeros(n)
    elif g == "tiles":
        n = 4000
        src, dst, rel, ids = rng.integers(0, n, 12000), rng.integers(0, n, 12000), rng.integers(0, R2, 12000), rng.integers(0, T, n)
    elif g == "fixmany":
        n = 3000
        src, dst, rel, ids = rng.integers(0, n, 140000), rng.integers(0, n, 140000), rng.integers(0, R2, 140000), rng.integers(0, T, n)
    elif g in ("splitfew", "splitlisted"):
        n = 3000
        E, hub = (6000, 300) if g == "splitfew" else (300000, 270000)
        ids = rng.integers(0, T, n)
        of_row = np.nonzero(ids == 7)[0]                                  # the pair (relation 3, table row 7)
        src = np.concatenate([rng.choice(of_row, hub), rng.integers(0, n, E - hub)])
        rel = np.concatenate([np.full(hub, 3), rng.integers(0, R2, E - hub)])
        if g == "splitlisted":                                            # a short entry beside the listed one: the pair (relation 5, table row 11)
            src[hub:hub + 300], rel[hub:hub + 300] = rng.choice(np.nonzero(ids == 11)[0], 300), 5
        dst = rng.integers(0, n, E)
    elif g == "members":
        members = ((50, 150), (70, 300), (30, 0))
        parts, off = [], 0
        for mn, mE in members:
            parts.append((rng.integers(0, mn, mE) + off, rng.integers(0, mn, mE) + off, np.zeros(mE)))
            off += mn
        n = off
        src, dst, rel = (np.concatenate([p[i] for p in parts]) for i in range(3))
        ids = rng.integers(0, T - 3, n)
    elif g == "subsampled":
        n = 300
        lone = np.concatenate([np.arange(200, 280), np.arange(200, 220)])              # one or two in-edges each
        src = rng.integers(0, n, 5000)
        dst = np.concatenate([rng.integers(0, 200, 5000 - lone.shape[0]), lone])
        rel, ids = rels(5000), rng.integers(0, T, n)
    elif g == "noedges":
        n = 50
        src = dst = rel = np.zeros(0)
        ids = np.arange(n) % T
    elif g.startswith("iso"):
        n = int(g[3:])
        src = dst = rel = np.zeros(0)
        ids = np.arange(n)
    else:
        raise KeyError(g)
    src, dst, rel, ids = i64(src, dst, rel, ids)
    return Graph(n, src, dst, rel, ids, members)


def snapshot(case, exact):
    """The case's graph as a Snapshot (BatchedSnapshot for `members`; the PARENT for `subsampled`)"""
    from temp_amd import snapshot as SN
    G = graph(case)
    if G.members is None:
        return SN.Snapshot(G.n, G.src, G.dst, G.rel, G.ids, nnorm=exact_nnorm(G.n) if exact else None)
    parts, off, e0 = [], 0, 0
    for mn, mE in G.members:
        sl = slice(e0, e0 + mE)
        parts.append(SN.Snapshot(mn, G.src[sl] - off, G.dst[sl] - off, G.rel[sl], G.ids[off:off + mn], nnorm=exact_nnorm(mn) if exact else None))
        off, e0 = off + mn, e0 + mE
    return SN.batch(parts)


# ---- host restatements of the dispatcher (asserted against the views on the CPU, against the counters on the GPU) ------------------
def fix_huge(n_partial):
    return max(-(-n_partial // (FIX_LIST_CAP - 1)), FIX_HUGE_MIN)


def pair_tail_grid(n_table):
    """-> (blocks, tiles per block): 128 blocks at most, 8 table rows per tile"""
    tiles = -(-max(n_table, 1) // PT_TE)
    per = -(-tiles // PT_MAX_BLOCKS)
    return -(-tiles // per), per


def tail_waves(R2):
    """-> (relation rows per wave, waves that own one) of k_pair_tail's eight waves"""
    per = -(-R2 // PT_WAVES)
    return per, -(-R2 // per)


def predict_fix(n_fix, n_partial, width):
    """the fix-up launches launch_fixup makes for a view"""
    if n_fix <= 0:
        return {}
    name = "fix_few" if n_fix * ((width + 255) // 256) <= 1024 else "fix_many"
    if n_partial >= FIX_SPLIT_MIN:
        return {(name + "_split", 0): 1, ("fix_split2", 0): 1}
    return {(name, 0): 1}


# ---- operands ---------------------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "table weight loop_w bias gy act p keep")


def wrow(case):
    return case.B * (case.d_in // case.B) * (case.d_out // case.B)


def operands(case, n, regime, device):
    """fp32 operands on `device`; keep: the dropout keep mask [n, d_out] as 0 / 1 (None without dropout)"""
    import torch
    from tests.cpu_backend import drop_mask
    has_bias, act, drop = case.flags
    T = case.n_table
    if regime == "exact":
        table, weight = _pattern(torch, T, case.d_in, 7, 11, 0, 9, device), _pattern(torch, case.R2, wrow(case), 5, 3, 1, 5, device)
        loop_w, bias = _pattern(torch, case.d_in, case.d_out, 3, 7, 2, 5, device), _pattern(torch, 1, case.d_out, 0, 1, 3, 9, device)[0]
        gy, p = _pattern(torch, n, case.d_out, 3, 5, 2, 5, device), 0.5
    else:
        mk = lambda shape, seed, scale: _wide(torch, shape, seed, scale).to(device)
        table, weight = mk((T, case.d_in), 31, 1.0), mk((case.R2, wrow(case)), 33, 0.3)
        loop_w, bias, gy, p = mk((case.d_in, case.d_out), 34, 0.1), mk((case.d_out,), 35, 0.5), mk((n, case.d_out), 32, 1.0), 0.25
    keep = (drop_mask((p, DROP_SEED), n, case.d_out) > 0).to(device) if drop and n else None
    return Operands(table, weight, loop_w, bias if has_bias else None, gy, act, p if drop else 0.0, keep)


def drop_arg(ops):
    """(p, seed) as the backends take it, None without dropout"""
    return (ops.p, DROP_SEED) if ops.p > 0 else None


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------
class Reference:
    """fp64 layer over the plain edge list.  src / dst / rel / ids: int64 numpy (ids None: the isolated layer, x = e = ops.table);
    nnorm: fp32 numpy.  forward() once; backward(mask) for any ReLU mask (None: the fp64 forward's own)."""

    def __init__(self, case, n, src, dst, rel, ids, nnorm, ops, device):
        import torch
        self.torch, self.case, self.n, self.ops, self.dev = torch, case, n, ops, device
        order = np.random.default_rng(0).permutation(src.shape[0])        # (a hub's edges are listed back to back: additions into one row serialise)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.src, self.dst, self.rel = t(src[order]), t(dst[order]), t(rel[order])
        self.ids = t(ids) if ids is not None else None
        self.nn2 = (t(np.asarray(nnorm, np.float32)).double() ** 2 if n and ids is not None else torch.zeros(n, dtype=torch.float64, device=device))
        self.scale = 1.0 / (1.0 - ops.p) if ops.p > 0 else 1.0
        self.keep = ops.keep.double() * self.scale if ops.keep is not None else None
        self.in_deg = torch.bincount(self.dst, minlength=n)
        self.out_deg = torch.bincount(self.src, minlength=n)
        self._bwd = None
        self.pre, self.pre_abs = self._forward(lambda v: v)[0], self._forward(lambda v: v.abs())[0]
        self.mask = self.pre > 0 if ops.act == RELU else torch.ones_like(self.pre, dtype=torch.bool)
        self.out = torch.where(self.mask, self.pre, torch.zeros_like(self.pre))

    def _forward(self, f, table=None, weight=None, loop_w=None, bias=None):
        """pre-activation from operands mapped through f (identity, abs) -- or from the given fp64 leaves (autograd)"""
        torch, c, o = self.torch, self.case, self.ops
        si, so = c.d_in // c.B, c.d_out // c.B
        T = f(o.table.double()) if table is None else table
        W = f(o.weight.double()) if weight is None else weight
        LW = f(o.loop_w.double()) if loop_w is None else loop_w
        b = (f(o.bias.double()) if o.bias is not None else None) if bias is None else bias
        x = T[self.ids] if self.ids is not None else T
        m = self.src.shape[0]
        pre = torch.zeros(self.n, c.d_out, dtype=torch.float64, device=self.dev)
        if m:
            msg = (x[self.src].view(m, c.B, si, 1) * W[self.rel].view(m, c.B, si, so)).sum(2).reshape(m, c.d_out)
            pre = pre.index_add(0, self.dst, msg) * self.nn2[:, None]
        loop = x @ LW
        if self.keep is not None:
            loop = loop * self.keep
        pre = pre + loop
        if self.ids is None:
            pre = pre + x
        if b is not None:
            pre = pre + b
        return pre, x

    def backward(self, mask=None):
        """-> {name: (value, sum |t|)} for d_table (isolated: d_e), d_weight, d_loop_w, d_bias (None without bias).  Values by autograd
        of the forward with the ReLU mask held at `mask`; magnitudes by the explicit gradient formulas on absolute values."""
        torch, o = self.torch, self.ops
        own = mask is None or torch.equal(mask, self.mask)
        if own and self._bwd is not None:
            return self._bwd
        mask = self.mask if mask is None else mask
        leaf = lambda v: v.double().clone().requires_grad_(True)
        T, W, LW = leaf(o.table), leaf(o.weight), leaf(o.loop_w)
        b = leaf(o.bias) if o.bias is not None else None
        pre, _ = self._forward(None, T, W, LW, b)
        (pre * mask.double() * o.gy.double()).sum().backward()
        mag = self.explicit_backward(mask, lambda v: v.abs())
        z = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
        res = {"d_table": (z(T), mag["d_table"]), "d_weight": (z(W), mag["d_weight"]), "d_loop_w": (z(LW), mag["d_loop_w"]),
               "d_bias": (z(b)[None, :], mag["d_bias"]) if b is not None else None}
        if own:
            self._bwd = res
        return res

    def explicit_backward(self, mask, f):
        """The gradient formulas written out, on operands mapped through f:
             dz = gy * mask, dzm = dz * keep / (1 - p), g[e] = nnorm[dst]^2 dz[dst]
             d_x[u] = sum_{(u,r,v)} BD(W[r]) . g  +  dzm[u] . loop_w^T (+ dz[u], isolated);  d_table = the index-add of d_x over ids
             d_W[r] = sum_{(u,r,v)} x[u]^T (x) g blockwise;  d_loop_w = x^T . dzm;  d_bias = the column sums of dz"""
        torch, c, o = self.torch, self.case, self.ops
        si, so = c.d_in // c.B, c.d_out // c.B
        T, W, LW = f(o.table.double()), f(o.weight.double()), f(o.loop_w.double())
        x = T[self.ids] if self.ids is not None else T
        dz = f(o.gy.double()) * mask.double()
        dzm = dz * self.keep if self.keep is not None else dz
        d_x = dzm @ LW.t()
        if self.ids is None:
            d_x = d_x + dz
        d_w = torch.zeros_like(W)
        m = self.src.shape[0]
        if m:
            g = (dz[self.dst] * self.nn2[self.dst][:, None]).view(m, c.B, 1, so)
            d_x = d_x.index_add(0, self.src, (W[self.rel].view(m, c.B, si, so) * g).sum(3).reshape(m, c.d_in))
            d_w = d_w.index_add(0, self.rel, (x[self.src].view(m, c.B, si, 1) * g).reshape(m, -1))
        d_table = torch.zeros_like(T).index_add(0, self.ids, d_x) if self.ids is not None else d_x
        return {"d_table": d_table, "d_weight": d_w, "d_loop_w": x.t() @ dzm, "d_bias": dz.sum(0, keepdim=True)}

    def zero_row_epilogue(self):
        """out rows of a node without in-edges: act(loop + bias) -- the epilogue of a zero aggregation row"""
        return self.out[self.in_deg == 0]

    def relu_edge(self):
        """elements whose fp64 pre-activation lies within the bar of zero (exact zeros of all-zero terms are not an edge)"""
        return (self.pre.abs() <= BAR * self.pre_abs) & (self.pre_abs > 0) if self.ops.act == RELU else self.torch.zeros_like(self.mask)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def guarded(torch, rows, cols, device):
    """a NaN-filled output of `rows` rows with GUARD guard rows behind"""
    return torch.full((rows + GUARD, cols), float("nan"), device=device)


def compare(name, buf, rows, ref, sabs, regime):
    """buf: fp32 [rows + GUARD, cols], NaN-filled before the call.  -> (problems, worst |got - ref| / (BAR sum |t|)).
    exact: buf[:rows] must equal the fp64 value bit for bit; wide: finite and within the bar everywhere (an element whose terms are
    all zero must be exactly zero); either: the guard rows keep their bits."""
    import torch
    problems = []
    if buf.shape[0] != rows + GUARD or not bool((buf[rows:].contiguous().view(torch.int32) == NAN_BITS).all()):
        problems.append("%s: guard rows were written" % name)
    got = buf[:rows].double()
    ref = ref.to(got.device)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        problems.append("%s: %d non-finite elements" % (name, int((~torch.isfinite(got)).sum())))
    err = (got - ref).abs()
    r = torch.where(err <= 0, torch.zeros_like(err), err / (BAR * sabs.to(got.device)))
    inf = float("inf")
    ratio = float(r.nan_to_num(nan=inf, posinf=inf).max()) if r.numel() else 0.0
    if regime == "exact":
        d = first_difference(got, ref)
        if d is not None:
            problems.append("%s, integer operands: %s" % (name, d))
    elif ratio > 1.0:
        bad = r.nan_to_num(nan=inf, posinf=inf)
        i, j = [int(v) for v in torch.nonzero(bad == bad.max())[0]]
        problems.append("%s: worst error %.3g of %.0e sum|t| at row %d column %d (got %r, want %r)" % (name, ratio, BAR, i, j, float(got[i, j]), float(ref[i, j])))
    return problems, ratio
