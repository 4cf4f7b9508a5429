"""One case per route of the RGCN edge-kernel dispatcher (temp_amd/csrc/rgcn_kernels.hip: run_agg, launch_agg, run_dw, launch_fixup;
rgcn_tile.hpp: tile_plan), shared by tests/test_rgcn_route_cases_cpu.py (the host-side facts every route rests on) and
tests/test_gpu_rgcn_routes.py (the kernels against fp64).  Graph recipes are plain numpy; no GPU here.

A case names its graph family and seed, d_in / d_out / num_bases / n_rel_rows, the options it sets and the launches the library must
then count (temp_rgcn_route_launches) for ONE call of the forward (temp_rgcn_fwd), of d/dh (temp_rgcn_bwd_dh) and of d/dweight
(temp_rgcn_bwd_weights): {(route, s): launches}.  A tiled aggregation that sums its multi-chunk segments in-block counts NO fix-up.

Families (nodes, edges; what the views look like is asserted in tests/test_rgcn_route_cases_cpu.py):
  small    200, 600 uniform                                          < 4 096 chunks, no fix-up
  hub      300, 900 uniform + one node of in-degree 150 + one of out-degree 150 + 300 edges of relation 2
                                                                     < 4 096 chunks, a few short fix-up entries in every view
  runs     200, 600 uniform + a hub with 640 in- and one with 640 out-edges in relations 0..3 + a node with 64 out- and one with
           64 in-edges of distinct relations                         chunks that take the run walk and chunks that take the per-edge walk
  many     6 000, 30 000 uniform (5 000 of them relation 0) + in / out hubs of degree 2 560 and 200
                                                                     >= 4 096 chunks; fix-up <16,1,32> with a long and a short entry
  fixmany  3 000, 6 000 uniform + one hub of degree 17 000 each way (relation 0) + 1 100 nodes of degree 70 each way
                                                                     > 1 024 fix-up items: <4,4,256> with a long entry (> 256 rows)
  batches  `members` = ((nodes, edges), ...) of uniform member snapshots joined by snapshot.batch"""
import collections

import numpy as np

ROUTES = ("fwd_tile8", "fwd_tile16", "fwd_lds_scalar", "fwd_lds_permute", "fwd_scalar", "fwd_permute", "fwd_generic",
          "dx_tile8", "dx_tile16", "dx_lds_scalar", "dx_lds_permute", "dx_scalar", "dx_permute", "dx_generic",
          "dw_hybrid", "dw_tile", "dw_scalar", "dw_permute", "dw_generic",
          "fix_few", "fix_many", "fix_few_split", "fix_many_split", "fix_split2")        # include/temp_amd.h: TEMP_RGCN_*, in order
S_CELLS = 5                                                                              # s = 0 .. 4
OPT = {"scalar": 2, "tile": 5, "debug": 6}                                               # include/temp_amd.h: TEMP_OPT_*

Case = collections.namedtuple("Case", "id family seed members d_in d_out B R2 opts fwd dx dw walks whole cpu")


def _case(id, family, d_in, d_out, B, R2, fwd, dx, dw, fix=(None, None, None), opts=None, seed=1, members=None, walks=(), whole=False, cpu=True):
    """fwd / dx / dw: route names without the phase prefix; fix: the fix-up launch behind each of the three (None: none).
    walks: views ('by_src', 'by_dst', 'by_rel') in which the case claims BOTH the run walk and the per-edge walk.
    whole: also the whole temp_rgcn_bwd with loop weights, bias and ReLU.  cpu: the CPU test also runs the fp32 test backend."""
    fast = d_in == d_out and d_in <= 256 and (d_in // B) in (1, 2, 4)
    s = d_in // B if fast else 0

    def ex(name, f):
        e = {(name, s if not name.endswith("generic") else 0): 1}
        if f:
            e[("fix_" + f, 0)] = 1
        if f and f.endswith("_split"):                       # (a view of 32 768 and more partial rows: the second level is always launched)
            e[("fix_split2", 0)] = 1
        return e
    return Case(id, family, seed, members, d_in, d_out, B, R2, dict(opts or {}), ex("fwd_" + fwd, fix[0]), ex("dx_" + dx, fix[1]),
                ex("dw_" + dw, fix[2]), tuple(walks), whole, cpu)


# ---- graph recipes ------------------------------------------------------------------------------------------------------------
def _uniform(rng, n, E, R2):
    return rng.integers(0, n, E), rng.integers(0, n, E), rng.integers(0, R2, E)


def _cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]).astype(np.int64) for i in range(3))


def edges(family, seed, R2):
    """-> (n, src, dst, rel) of a single-snapshot family"""
    rng = np.random.default_rng(seed)
    if family == "small":
        return (200,) + _cat([_uniform(rng, 200, 600, R2)])
    if family == "hub":
        n = 300
        u = _uniform(rng, n, 900, R2)
        into = (rng.integers(0, n, 150), np.zeros(150, np.int64), rng.integers(0, R2, 150))
        out = (np.ones(150, np.int64), rng.integers(0, n, 150), rng.integers(0, R2, 150))
        r2 = (rng.integers(0, n, 300), rng.integers(0, n, 300), np.full(300, 2))
        return (n,) + _cat([u, into, out, r2])
    if family == "runs":
        n = 200
        u = _uniform(rng, n, 600, R2)
        into = (rng.integers(0, n, 640), np.zeros(640, np.int64), rng.integers(0, 4, 640))
        out = (np.ones(640, np.int64), rng.integers(0, n, 640), rng.integers(0, 4, 640))
        d_out = (np.full(64, 5), rng.integers(0, n, 64), 10 + np.arange(64))
        d_in = (rng.integers(0, n, 64), np.full(64, 6), 100 + np.arange(64))
        return (n,) + _cat([u, into, out, d_out, d_in])
    if family == "many":
        n = 6000
        us, ud, ur = _uniform(rng, n, 30000, R2)
        ur[:5000] = 0
        parts = [(us, ud, ur)]
        for node, deg in ((0, 2560), (2, 200)):
            parts.append((rng.integers(0, n, deg), np.full(deg, node), rng.integers(0, R2, deg)))
        for node, deg in ((1, 2560), (3, 200)):
            parts.append((np.full(deg, node), rng.integers(0, n, deg), rng.integers(0, R2, deg)))
        return (n,) + _cat(parts)
    if family == "fixmany":
        n = 3000
        parts = [_uniform(rng, n, 6000, R2)]
        parts.append((rng.integers(0, n, 17000), np.zeros(17000, np.int64), np.zeros(17000, np.int64)))
        parts.append((np.ones(17000, np.int64), rng.integers(0, n, 17000), np.zeros(17000, np.int64)))
        mid = np.repeat(10 + np.arange(1100), 70)
        parts.append((rng.integers(0, n, mid.shape[0]), mid, rng.integers(0, R2, mid.shape[0])))
        parts.append((mid, rng.integers(0, n, mid.shape[0]), rng.integers(0, R2, mid.shape[0])))
        return (n,) + _cat(parts)
    raise KeyError(family)


def exact_nnorm(n):
    """2^-(node % 3): every product with nnorm^2 is exact"""
    return (2.0 ** -(np.arange(n) % 3)).astype(np.float32)


def build(case, exact):
    """The case's graph as a Snapshot (a BatchedSnapshot for `members`); exact: nnorm = 2^-(node % 3), else the graph's 1 / in-degree."""
    from temp_amd import snapshot as SN
    if case.members is None:
        n, src, dst, rel = edges(case.family, case.seed, case.R2)
        return SN.Snapshot(n, src, dst, rel, np.arange(n), nnorm=exact_nnorm(n) if exact else None)
    rng = np.random.default_rng(case.seed)
    parts = []
    for n, E in case.members:
        src, dst, rel = _uniform(rng, n, E, case.R2)
        parts.append(SN.Snapshot(n, src, dst, rel, np.arange(n), nnorm=exact_nnorm(n) if exact else None))
    return SN.batch(parts)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
FEW, MANY = "few", "many"
ALL = []
# permute kernels, relation table through L2 (small family: no fix-up): every lane grouping pick_lpr gives, ragged ones included
for D, s in ((4, 4), (8, 2), (12, 1), (16, 4), (20, 2), (32, 1), (36, 4), (64, 2), (68, 1), (128, 4)):
    ALL.append(_case("permute_d%d_s%d" % (D, s), "small", D, D, D // s, 8, "permute", "permute", "permute", whole=D in (12, 36, 128)))
# ... the same with fix-up entries in every view (<16,1,32>, short entries, width <= 256 and D * S)
for D, s in ((12, 4), (20, 1), (68, 2)):
    ALL.append(_case("permute_hub_d%d_s%d" % (D, s), "hub", D, D, D // s, 8, "permute", "permute", "permute", fix=(FEW, FEW, FEW)))
# scalar kernels, no LDS table: 33 of 64 lanes at D = 132, all lanes at 256; d/dh stays on the permute kernel at lpr = 64
for D, s in ((132, 4), (132, 1), (200, 2), (256, 1), (256, 4), (200, 4)):
    ALL.append(_case("scalar_d%d_s%d" % (D, s), "small", D, D, D // s, 8, "scalar", "permute", "scalar", whole=(D, s) in ((132, 4), (256, 1))))
ALL.append(_case("scalar_hub_d132_s2", "hub", 132, 132, 66, 8, "scalar", "permute", "scalar", fix=(FEW, FEW, FEW), whole=True))
# a table beyond 64 KB: d/dh on the scalar kernel, run walk and per-edge walk chosen per chunk; TEMP_OPT_DEBUG = 101 keeps d/dh on the permute kernel
ALL.append(_case("runs_d200_s2", "runs", 200, 200, 100, 460, "scalar", "scalar", "scalar", fix=(FEW, FEW, FEW), walks=("by_dst", "by_src", "by_rel"), whole=True))
ALL.append(_case("runs_d200_s2_debug101", "runs", 200, 200, 100, 460, "scalar", "permute", "scalar", fix=(FEW, FEW, FEW), opts={"debug": 101}))
# relation table in LDS (many family: >= 4 096 chunks); 65 536 bytes is the last size that goes there
ALL.append(_case("lds_scalar_d200_s2", "many", 200, 200, 100, 40, "lds_scalar", "lds_scalar", "scalar", fix=(FEW, FEW, FEW), whole=True))
ALL.append(_case("lds_scalar_d256_s1_64k", "many", 256, 256, 256, 64, "lds_scalar", "lds_scalar", "scalar", fix=(FEW, FEW, FEW)))
ALL.append(_case("lds_scalar_d256_s4_64k", "many", 256, 256, 64, 16, "lds_scalar", "lds_scalar", "scalar", fix=(FEW, FEW, FEW), cpu=False))
ALL.append(_case("l2_scalar_d256_s1_65rows", "many", 256, 256, 256, 65, "scalar", "scalar", "scalar", fix=(FEW, FEW, FEW), walks=("by_src",), cpu=False))
ALL.append(_case("l2_scalar_d256_s4_17rows", "many", 256, 256, 64, 17, "scalar", "scalar", "scalar", fix=(FEW, FEW, FEW), walks=("by_src",), cpu=False))
ALL.append(_case("lds_permute_d64_s4", "many", 64, 64, 16, 40, "lds_permute", "lds_permute", "permute", fix=(FEW, FEW, FEW), whole=True))
ALL.append(_case("lds_permute_d128_s2_64k", "many", 128, 128, 64, 64, "lds_permute", "lds_permute", "permute", fix=(FEW, FEW, FEW)))
ALL.append(_case("lds_permute_d32_s1", "many", 32, 32, 32, 40, "lds_permute", "lds_permute", "permute", fix=(FEW, FEW, FEW)))
ALL.append(_case("lds_permute_d200_scalar_off", "many", 200, 200, 100, 40, "lds_permute", "lds_permute", "permute", fix=(FEW, FEW, FEW), opts={"scalar": 0}, cpu=False))
# generic kernels: d_in != d_out, block sizes outside {1, 2, 4}, d > 256
for di, do, B in ((24, 24, 4), (8, 24, 4), (320, 64, 16)):
    ALL.append(_case("generic_%d_%d_b%d" % (di, do, B), "small", di, do, B, 8, "generic", "generic", "generic"))
for di, do, B in ((24, 24, 4), (8, 24, 4), (24, 8, 4), (12, 20, 4), (260, 260, 130), (320, 64, 16)):
    ALL.append(_case("generic_hub_%d_%d_b%d" % (di, do, B), "hub", di, do, B, 8, "generic", "generic", "generic", fix=(FEW, FEW, FEW),
                     whole=(di, do) in ((8, 24), (260, 260))))
ALL.append(_case("generic_many_24_8_b4", "many", 24, 8, 4, 40, "generic", "generic", "generic", fix=(FEW, FEW, FEW)))
# fix-up <4,4,256>: more than 1 024 items, a long entry in every view; weight-gradient rows of 2 and 4 column blocks
ALL.append(_case("fixmany_d200_s2", "fixmany", 200, 200, 100, 600, "scalar", "scalar", "scalar", fix=(MANY, MANY, MANY), walks=("by_dst", "by_src", "by_rel"), cpu=False))
ALL.append(_case("fixmany_d256_s4", "fixmany", 256, 256, 64, 600, "scalar", "scalar", "scalar", fix=(MANY, MANY, MANY), cpu=False))
ALL.append(_case("fixmany_d8_s2", "fixmany", 8, 8, 4, 600, "lds_permute", "lds_permute", "permute", fix=(MANY, MANY, FEW)))
ALL.append(_case("fixmany_generic_24_8_b4", "fixmany", 24, 8, 4, 600, "generic", "generic", "generic", fix=(MANY, MANY, FEW), cpu=False))
# tiled kernels on batches: 9 members (not a multiple of 8) of about 100 nodes, the fifth without edges; in-block fix-up in the node views
B9 = ((100, 400), (90, 380), (110, 420), (100, 400), (60, 0), (100, 410), (95, 400), (105, 400), (100, 390))
ALL.append(_case("tile8_d32_s1_dw_tile", "batch", 32, 32, 32, 8, "tile8", "tile8", "tile", fix=(None, None, FEW), opts={"tile": 2}, members=B9, whole=True))
ALL.append(_case("tile8_d200_s2_dw_hybrid", "batch", 200, 200, 100, 8, "tile8", "tile8", "hybrid", fix=(None, None, FEW), opts={"tile": 3}, members=B9))
ALL.append(_case("tile8_d64_s4_dw_tile", "batch", 64, 64, 16, 8, "tile8", "tile8", "tile", fix=(None, None, FEW), opts={"tile": 2}, members=B9))
ALL.append(_case("tile8_d200_s2_dw_gather", "batch", 200, 200, 100, 8, "tile8", "tile8", "scalar", fix=(None, None, FEW), members=B9, whole=True))
ALL.append(_case("tile_off_d200_s2", "batch", 200, 200, 100, 8, "scalar", "permute", "scalar", fix=(None, None, FEW), opts={"tile": 0}, members=B9))
# more than 256 relation rows: 16-bit relation ids in LDS (a batch needs 2 * 192 * n_rel_rows edges to carry member tables)
B16 = tuple((100, 12800) for _ in range(9))
ALL.append(_case("tile16_d16_s1_dw_hybrid", "batch", 16, 16, 16, 300, "tile16", "tile16", "hybrid", fix=(None, None, FEW), opts={"tile": 3}, members=B16, cpu=False))
ALL.append(_case("tile16_d40_s2_dw_tile", "batch", 40, 40, 20, 300, "tile16", "tile16", "tile", fix=(None, None, FEW), opts={"tile": 2}, members=B16, cpu=False))
ALL.append(_case("tile16_d64_s4_dw_hybrid", "batch", 64, 64, 16, 300, "tile16", "tile16", "hybrid", fix=(None, None, FEW), opts={"tile": 3}, members=B16, cpu=False))
# a member of 1 000 nodes at D = 200: narrow, ragged slices
ALL.append(_case("tile8_member1000_d200_s2", "batch", 200, 200, 100, 8, "tile8", "tile8", "tile", fix=(None, None, FEW), opts={"tile": 2},
                 members=((100, 400), (1000, 4000), (100, 400))))
# a member of 16 384 and more edge positions: the node views' fix-up is its own launch again
ALL.append(_case("tile8_member16400_d64_s2", "batch", 64, 64, 32, 8, "tile8", "tile8", "permute", fix=(FEW, FEW, FEW), members=((300, 16400), (100, 400), (100, 400))))
# a member of more than 8 190 nodes: its row offsets do not fit the 17 bits of the packed edge word; the plan is refused, the gather kernels run
ALL.append(_case("tile_refused_member8200_d8_s2", "batch", 8, 8, 4, 8, "lds_permute", "lds_permute", "permute", fix=(None, None, FEW), opts={"tile": 2},
                 members=((8200, 9000), (100, 400))))
# a member of more than 2 048 by-relation chunks: the chunk sort of the tiled weight gradient re-reads its chunk list.  Member tables
# need 2 * 192 * n_rel_rows edges and a member's edges must fit LDS, so the union has 39 members and 81 900 by-relation partial rows:
# its fix-up takes the split launches (no entry is long enough to be listed: the second level finds an empty list)
ALL.append(_case("tile16_member_2100_rel_chunks_d8_s1", "batch", 8, 8, 8, 2100, "tile16", "tile16", "tile", fix=(MANY, MANY, "many_split"), opts={"tile": 2},
                 members=tuple((100, 21000) for _ in range(39)), cpu=False))

BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)


# ---- operands, the fp64 reference and the bars (torch; any device) ------------------------------------------------------------
def shapes(case):
    si, so = case.d_in // case.B, case.d_out // case.B
    return si, so, case.B * si * so


def _pattern(torch, rows, cols, mr, mc, shift, mod, device):
    """x[r][c] = ((mr r + mc c + shift) % mod) - mod // 2: small integers, so that a wrong element names its row and column"""
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    c = torch.arange(cols, device=device, dtype=torch.int64)[None, :]
    return (((mr * r + mc * c + shift) % mod) - mod // 2).float()


def _wide(torch, shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp(3.0 * torch.rand(shape, generator=g) - 1.5) * scale


def operands(case, n, data, device):
    """-> (h [n, d_in], dz [n, d_out], weight [R2, wrow]) fp32.  exact: integers in [-4, 4] (rows) and [-2, 2] (weights);
    wide: reals spread over about three decades."""
    import torch
    wrow = shapes(case)[2]
    if data == "exact":
        return (_pattern(torch, n, case.d_in, 7, 11, 0, 9, device), _pattern(torch, n, case.d_out, 3, 5, 2, 9, device),
                _pattern(torch, case.R2, wrow, 5, 3, 1, 5, device))
    return (_wide(torch, (n, case.d_in), 31, 1.0).to(device), _wide(torch, (n, case.d_out), 32, 1.0).to(device),
            _wide(torch, (case.R2, wrow), 33, 0.3).to(device))


def reference(case, snap, h, dz, weight, device, slab=16384):
    """The three edge sums in fp64, term by term over the edge list (no views, no chunks):
         fwd[v] = nnorm[v]^2 sum_{(u,r,v)} h[u] . BD(W[r])      dx[u] = sum_{(u,r,v)} BD(W[r]) . nnorm[v]^2 dz[v]
         dw[r]  = sum_{(u,r,v)} h[u]^T (x) nnorm[v]^2 dz[v]  blockwise
    -> {phase: (value, sum of |terms|, edges of every output row's segment)}"""
    import torch
    si, so, wrow = shapes(case)
    B, n = case.B, snap.n
    # (the edges in a shuffled order: the recipes list a hub's edges back to back, and a slab of additions into ONE row serialises)
    order = np.random.default_rng(0).permutation(snap.src.shape[0])
    src = torch.from_numpy(np.ascontiguousarray(snap.src[order])).to(device)
    dst = torch.from_numpy(np.ascontiguousarray(snap.dst[order])).to(device)
    rel = torch.from_numpy(np.ascontiguousarray(snap.rel[order])).to(device)
    nn2 = torch.from_numpy(np.ascontiguousarray(snap.nnorm)).to(device).double() ** 2
    h64, dz64, w64 = h.double(), dz.double(), weight.double()
    z = lambda r, c: torch.zeros(r, c, dtype=torch.float64, device=device)
    fwd, fwd_a, dx, dx_a, dw, dw_a = z(n, case.d_out), z(n, case.d_out), z(n, case.d_in), z(n, case.d_in), z(case.R2, wrow), z(case.R2, wrow)
    for e0 in range(0, src.shape[0], slab):
        s_, d_, r_ = src[e0:e0 + slab], dst[e0:e0 + slab], rel[e0:e0 + slab]
        m = s_.shape[0]
        w = w64[r_].view(m, B, si, so)
        x = h64[s_].view(m, B, si, 1)
        g = (dz64[d_] * nn2[d_][:, None]).view(m, B, 1, so)
        fwd.index_add_(0, d_, (x * w).sum(2).reshape(m, -1))
        fwd_a.index_add_(0, d_, (x.abs() * w.abs()).sum(2).reshape(m, -1))
        dx.index_add_(0, s_, (w * g).sum(3).reshape(m, -1))
        dx_a.index_add_(0, s_, (w.abs() * g.abs()).sum(3).reshape(m, -1))
        dw.index_add_(0, r_, (x * g).reshape(m, -1))
        dw_a.index_add_(0, r_, (x.abs() * g.abs()).reshape(m, -1))
    fwd, fwd_a = fwd * nn2[:, None], fwd_a * nn2[:, None]
    cnt = lambda idx, k: torch.bincount(idx, minlength=k).double()
    return {"fwd": (fwd, fwd_a, cnt(dst, n)), "dx": (dx, dx_a, cnt(src, n)), "dw": (dw, dw_a, cnt(rel, case.R2))}


BAR1 = 1e-6                  # of sum |t|: the project's bar for dense products


def chain_k(case, phase, n_edges):
    """k of the second bar, |got - ref| <= k 2^-24 sum |t|: the longest chain of dependent roundings, to first order.  A chunk of
    min(n, C) edges adds S products each into one accumulator, the fix-up adds the ceil(n / C) chunk sums, and the norm, its square,
    the scaling and the block's own first product round once each (+ 4).  C = 64 for the node views, 128 by relation.  The generic
    kernels sum si (forward) or so (d/dh) products per edge; the weight gradient adds ONE product per edge and element, so outside
    the fast shapes (where the bar is stated with S) it takes the smaller of si and so."""
    import torch
    si, so, _ = shapes(case)
    fast = case.d_in == case.d_out and case.d_in <= 256 and si in (1, 2, 4)
    s = si if fast else {"fwd": si, "dx": so, "dw": min(si, so)}[phase]
    C = 128 if phase == "dw" else 64
    return s * torch.clamp(n_edges, max=C) + torch.ceil(n_edges / C) + 4


def compare(case, phase, got, ref, sabs, n_edges):
    """-> (finite, worst |got - ref| / (1e-6 sum|t|), worst |got - ref| / (k 2^-24 sum|t|)) over every element; an element whose
    terms are all zero must be exactly zero (ratio inf otherwise)"""
    import torch
    g = got.double()
    err = (g - ref).abs()
    k = chain_k(case, phase, n_edges)[:, None]
    inf = float("inf")

    def worst(bound):
        r = torch.where(err <= 0, torch.zeros_like(err), err / bound)
        return float(r.nan_to_num(nan=inf, posinf=inf).max()) if r.numel() else 0.0
    return bool(torch.isfinite(g).all()), worst(BAR1 * sabs), worst(k * 2.0 ** -24 * sabs)


def first_difference(got, ref):
    """None when got == ref everywhere, else a line naming the first wrong element"""
    import torch
    g = got.double()
    if torch.equal(g, ref):
        return None
    bad = ~(g == ref)
    r, c = [int(v) for v in torch.nonzero(bad)[0]]
    return "%d/%d elements differ, first at row %d column %d: got %r, want %r" % (int(bad.sum()), g.numel(), r, c, float(g[r, c]), float(ref[r, c]))
