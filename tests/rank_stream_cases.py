"""Cases of the streamed filtered rank (include/temp_amd.h: temp_filtered_rank_stream / temp_filtered_rank_stream_mix), of the three
evaluation filters' `panel=` route and of `eval_panel`, shared by the CPU suite (the torch contract, evaluation.rank_stream_torch,
through the test backends) and the GPU suite (the HIP kernel).  Integer ranks are compared with torch.equal throughout.

  * kernel cases: scores on a grid where every sigmoid implementation orders alike -- multiples of 1/8 in [-8, 8] (neighbours differ
    by far more than an ulp of their sigmoid), a plateau of scores >= 20 (fp32 sigmoid exactly 1) and one of scores <= -110 (exactly
    0), values repeated so that ties are broken by id.  The two operands of the mixed cases share the plateau COLUMNS and the gates
    are quarters, so the mix (exact: multiples of 1/32 below 256) stays on such a grid: multiples of 1/32 in [-8, 8], >= 20, <= -110.
    Seven rows: an empty list, a list naming the target, a hub list of 150, a list covering a whole 256-entity window, a target in
    the first and in the last column, a target that is the last entity of a panel;
  * filter cases: integer tables in {-2 .. 2}, D = 16, gates in quarters, on a graph of the ICEWS14 slice: every score is a multiple
    of 1/16 far below 2^24 / 16 on every route, so a table slice scores exactly as the whole table and `panel=p` == `panel=None`;
  * model cases: evaluate() of the golden G13 / G18 / G31 models with eval_panel set, under the comparison the goldens' own tests
    apply (window_cases.check_evaluate, check_post_ensemble_evaluate, aggregator_cases.check_golden_ranks), restated here."""
import types

import numpy as np
import torch

from temp_amd import _lib
from temp_amd import scores as SC
from temp_amd.evaluation import EvaluationFilter, PostEnsembleEvaluationFilter, PostEvaluationFilter, rank_stream_torch
from tests import topk_cases as KC

WHOLE, COLLECT, COUNT_FIRST, COUNT_ADD = _lib.RANK_WHOLE, _lib.RANK_COLLECT, _lib.RANK_COUNT_FIRST, _lib.RANK_COUNT_ADD
P_ROWS = 7                                   # a partly filled last workgroup on the wave route (four rows per workgroup)
SHAPES = (1000, 1028, 2500)                  # wave route with N % 256 != 0; the first size on the workgroup route; three panel widths
WIDTHS = (512, 1024, 2500)
GATES = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
SCORERS = {"distmult": SC.distmult, "complex": SC.complex, "transE": SC.transE}


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _draw(kind, g):
    """One matrix on the grid over the plateau layout `kind` (0 grid, 1 high plateau, 2 low plateau)."""
    grid = torch.randint(-64, 65, kind.shape, generator=g).float() / 8.0
    high = 20.0 + torch.randint(0, 41, kind.shape, generator=g).float() / 4.0
    low = -110.0 - torch.randint(0, 41, kind.shape, generator=g).float() / 4.0
    return torch.where(kind == 1, high, torch.where(kind == 2, low, grid))


def rows(N):
    """(a, b [7, N] float32, w [7], target [7] int32, filt_ptr [8] int32, filt_ids int32) on the CPU, made once per N and shared:
    callers must not modify them.  a alone is the operand of the plain cases."""
    if N not in _ROWS:
        g = torch.Generator().manual_seed(7919 * N + 1)
        u = torch.rand(P_ROWS, N, generator=g)
        kind = (u < 0.06).long() + 2 * ((u >= 0.06) & (u < 0.12)).long()
        a, b = _draw(kind, g), _draw(kind, g)
        last_of_panel = 1023 if N > 1024 else 511
        target = torch.tensor([N // 3, N // 2, 2 * N // 3, 300, 0, N - 1, last_of_panel], dtype=torch.int64)
        assert 1 in kind[2].tolist() and 2 in kind[0].tolist()
        # a target on each plateau: its ties with the plateau's other members are broken by id
        a[2, target[2]], b[2, target[2]] = 22.0, 21.0
        a[0, target[0]], b[0, target[0]] = -111.0, -112.5
        pick = lambda k: torch.sort(torch.randperm(N, generator=g)[:k]).values
        lists = [torch.zeros(0, dtype=torch.int64),
                 torch.unique(torch.cat([pick(9), target[1:2]])),
                 pick(150),
                 torch.unique(torch.cat([torch.arange(256, 512), pick(5)])),
                 torch.unique(torch.cat([pick(20), torch.tensor([1, 2, 3])])),
                 torch.unique(torch.cat([pick(20), torch.tensor([N - 2, N - 3])])),
                 torch.unique(torch.cat([pick(70), torch.tensor([last_of_panel - 1, last_of_panel + 1])]))]
        assert int(target[1]) in lists[1].tolist() and len(lists[2]) == 150 and set(range(256, 512)) <= set(lists[3].tolist())
        ptr = torch.zeros(P_ROWS + 1, dtype=torch.int32)
        ptr[1:] = torch.cumsum(torch.tensor([len(x) for x in lists]), 0).int()
        w = GATES[torch.tensor([2, 0, 4, 1, 3, 2, 1])]
        _ROWS[N] = (a, b, w, target.int(), ptr, torch.cat(lists).int())
    return _ROWS[N]


def mixed(a, b, w):
    """w a + (1 - w) b on the CPU: exact for the fixtures."""
    wc = w.view(-1, 1)
    m = wc * a + (1 - wc) * b
    assert torch.equal(m.double(), wc.double() * a.double() + (1 - wc.double()) * b.double())
    return m


def brute_ranks(s, target, ptr, ids):
    """The rank definition entity by entity in python: value 0 for a listed entity that is not the target, else the sigmoid class
    of the grid (>= 20: 1, <= -110: 0, else strictly increasing in the score); ahead iff larger, or equal with a smaller id."""
    def value(x):
        return 2e9 if x >= 20 else (-2e9 if x <= -110 else x)          # a monotone stand-in for the sigmoid on the grid
    out = []
    for p in range(s.shape[0]):
        t = int(target[p])
        listed = set() if ptr is None else set(int(e) for e in ids[int(ptr[p]):int(ptr[p + 1])])
        ts = value(float(s[p, t]))
        n = 0
        for e in range(s.shape[1]):
            v = -2e9 if (e in listed and e != t) else value(float(s[p, e]))
            n += (v > ts) or (v == ts and e < t)
        out.append(n + 1)
    return torch.tensor(out, dtype=torch.int64)


def sweep(rank, lead, target, ptr, ids, N, width, order, slicer=None):
    """A COLLECT sweep over ascending panels of `width` columns, then the counting sweep in `order`; the panels are pointer slices
    of the matrices in `lead` (vectors in `lead`, the gate, pass unsliced) unless `slicer(m, c0, c1)` makes them."""
    cut = slicer or (lambda m, c0, c1: m[:, c0:])
    part = lambda c0, c1: tuple(cut(m, c0, c1) if m.dim() == 2 else m for m in lead)
    carry = None
    for c0, c1 in KC.panels(N, width, "asc"):
        none, carry = rank(*part(c0, c1), target, ptr, ids, mode=COLLECT, col0=c0, n=c1 - c0, carry=carry)
        assert none is None
    ranks = None
    for i, (c0, c1) in enumerate(KC.panels(N, width, order)):
        ranks, carry = rank(*part(c0, c1), target, ptr, ids, mode=COUNT_ADD if i else COUNT_FIRST, col0=c0, n=c1 - c0, carry=carry)
    assert ranks.dtype == torch.int64 and carry[1].dtype == torch.int32 and torch.equal(ranks, carry[1].long() + 1)
    return ranks


def check_whole_equals_filtered_rank(rank, filtered_rank, to_dev, N):
    """Check 1: the plain WHOLE call == filtered_rank on the same matrix, on the grid and on a seeded normal matrix; both equal the
    definition applied entity by entity on the grid; raw ranks (no lists) likewise."""
    a, _, _, target, ptr, ids = rows(N)
    noise = 4.0 * torch.randn(P_ROWS, N, generator=torch.Generator().manual_seed(N))
    for what, s in (("grid", a), ("normal", noise)):
        for f in ((ptr, ids), (None, None)):
            got, carry = rank(to_dev(s), to_dev(target), to_dev(f[0]), to_dev(f[1]), mode=WHOLE)
            assert carry is None and got.dtype == torch.int64
            want = filtered_rank(to_dev(s), to_dev(target), to_dev(f[0]), to_dev(f[1]))
            assert torch.equal(got, want), (what, N, f[0] is None)
            if what == "grid":
                assert torch.equal(got.cpu(), brute_ranks(s, target, *f)), (N, f[0] is None)


def check_panels_equal_whole(rank, to_dev, N, width, order):
    """Check 2: COLLECT + COUNT_* == WHOLE, the counting sweep in any order; check 7: the same call twice gives the same bits."""
    a, _, _, target, ptr, ids = rows(N)
    dev = tuple(to_dev(x) for x in (a, target, ptr, ids))
    whole = rank(*dev, mode=WHOLE)[0]
    assert torch.equal(whole, rank(*dev, mode=WHOLE)[0])
    got = sweep(rank, dev[:1], *dev[1:], N, width, order)
    assert torch.equal(got, whole), (N, width, order)
    assert torch.equal(got, sweep(rank, dev[:1], *dev[1:], N, width, order))


def check_mixed(rank_mix, rank, to_dev, N, width):
    """Check 3: the mixed entry == the torch contract on the mixed matrix, whole and in panels; w = 1 is the plain entry on a,
    w = 0 on b."""
    a, b, w, target, ptr, ids = rows(N)
    m = mixed(a, b, w)
    want = rank_stream_torch(m, target, ptr, ids, mode=WHOLE)[0]
    assert torch.equal(want, brute_ranks(m, target, ptr, ids))
    f = tuple(to_dev(x) for x in (target, ptr, ids))
    a_d, b_d, w_d = to_dev(a), to_dev(b), to_dev(w)
    got = rank_mix(a_d, b_d, w_d, *f, mode=WHOLE)[0]
    assert torch.equal(got.cpu(), want), ("whole", N)
    assert torch.equal(got, rank_mix(a_d, b_d, w_d, *f, mode=WHOLE)[0])
    for order in ("asc", "shuffled"):
        assert torch.equal(sweep(rank_mix, (a_d, b_d, w_d), *f, N, width, order).cpu(), want), (N, width, order)
    for wv, src in ((1.0, a_d), (0.0, b_d)):
        wd = to_dev(torch.full((P_ROWS,), wv))
        assert torch.equal(rank_mix(a_d, b_d, wd, *f, mode=WHOLE)[0], rank(src, *f, mode=WHOLE)[0]), (N, wv)
        assert torch.equal(sweep(rank_mix, (a_d, b_d, wd), *f, N, width, "desc"), sweep(rank, (src,), *f, N, width, "desc")), (N, wv)


def check_pad_columns(rank, rank_mix, to_dev, N, width):
    """Check 4: ld = N + 4 with +100 in the pad columns changes nothing, in WHOLE and in every panel (the middle ones included) of a
    panelled run whose panels are matrices of their own, [P, width + 4], padded the same way."""
    a, b, w, target, ptr, ids = rows(N)
    f = tuple(to_dev(x) for x in (target, ptr, ids))
    pad = lambda m: torch.cat([m, torch.full((m.shape[0], 4), 100.0)], dim=1)
    own = lambda m, c0, c1: to_dev(pad(m[:, c0:c1].cpu()))
    assert len(KC.panels(N, width, "asc")) >= 3
    want = rank(to_dev(a), *f, mode=WHOLE)[0]
    assert torch.equal(rank(to_dev(pad(a)), *f, mode=WHOLE, n=N)[0], want), "whole"
    assert torch.equal(sweep(rank, (a,), *f, N, width, "asc", slicer=own), want), "panels"
    w_d = to_dev(w)
    want = rank_mix(to_dev(a), to_dev(b), w_d, *f, mode=WHOLE)[0]
    assert torch.equal(rank_mix(to_dev(pad(a)), to_dev(pad(b)), w_d, *f, mode=WHOLE, n=N)[0], want), "mixed whole"
    assert torch.equal(sweep(rank_mix, (a, b, w_d), *f, N, width, "asc", slicer=own), want), "mixed panels"


def check_listed_value_zero(rank, to_dev):
    """Check 5: a target whose own sigmoid is 0 (the -110 plateau).  Listed entities have value 0 and are NOT excluded: those with a
    smaller id are ahead, those with a larger id are not -- in the target's panel ([1024, 1536) of the 512-wide run) and in others.
    The listed entities hold high scores, so a kernel that ranks their score, or drops them, gives another rank."""
    N, t = 2500, 1300
    g = torch.Generator().manual_seed(5)
    s = torch.randint(-64, 65, (1, N), generator=g).float() / 8.0
    smaller, larger = [10, 700, 1100, 1200], [1400, 1500, 2000, 2400]
    low_smaller, low_larger = [5, 1290], [1301, 2499]                     # unlisted entities on the low plateau: value 0 as well
    s[0, smaller + larger] = 25.0
    s[0, low_smaller + low_larger] = -120.0
    s[0, t] = -110.0
    ids = torch.tensor(sorted(smaller + larger), dtype=torch.int32)
    ptr = torch.tensor([0, len(ids)], dtype=torch.int32)
    target = torch.tensor([t], dtype=torch.int32)
    zero_valued = len(smaller) + len(larger) + len(low_smaller) + len(low_larger)
    want = torch.tensor([(N - 1 - zero_valued) + len(smaller) + len(low_smaller) + 1])
    assert torch.equal(brute_ranks(s, target, ptr, ids), want)
    dev = tuple(to_dev(x) for x in (s, target, ptr, ids))
    assert torch.equal(rank(*dev, mode=WHOLE)[0].cpu(), want)
    for width in (512, 1024):
        for order in ("asc", "desc"):
            assert torch.equal(sweep(rank, dev[:1], *dev[1:], N, width, order).cpu(), want), (width, order)
    raw = rank(dev[0], dev[1], None, None, mode=WHOLE)[0].cpu()          # unlisted, the eight high scores are ahead whatever their id
    assert int(raw) == int(want) + len(larger)


def check_collect_touches_only_its_rows(rank, to_dev, N=2500, width=512):
    """COLLECT writes the target's raw score for the rows whose target is in the panel and leaves the others as they were."""
    a, _, _, target, ptr, ids = rows(N)
    a_d, f = to_dev(a), tuple(to_dev(x) for x in (target, ptr, ids))
    c0, c1 = 1024, 1536
    carry = (to_dev(torch.full((P_ROWS,), -7.0)), to_dev(torch.full((P_ROWS,), 3, dtype=torch.int32)))
    _, carry = rank(a_d[:, c0:], *f, mode=COLLECT, col0=c0, n=c1 - c0, carry=carry)
    inside = (target >= c0) & (target < c1)
    assert bool(inside.any()) and not bool(inside.all())
    want = torch.where(inside, a[torch.arange(P_ROWS), target.long()], torch.full((P_ROWS,), -7.0))
    assert torch.equal(carry[0].cpu(), want) and bool((carry[1].cpu() == 3).all())


# ---------------------------------------------------------------------------------------------------------------------
# filter level
# ---------------------------------------------------------------------------------------------------------------------
D_FILTER, T_FILTER = 16, 7
FILTER_CASES = [(f, n) for f in ("base", "ensemble", "gated") for n in ("distmult", "complex", "transE")] + [("ensemble_two_rel", "complex")]


def _ints(n, d, seed):
    return torch.randint(-2, 3, (n, d), generator=torch.Generator().manual_seed(seed)).float()


def _quarters(P, seed):
    return GATES[torch.randint(0, 5, (P,), generator=torch.Generator().manual_seed(seed))]


def filter_call(family, name, device):
    """-> (call(panel) -> ranks of the valid triples of timestamp T_FILTER on the slice under integer tables, P, N)."""
    from tests.window_cases import slice_snapshots
    s = slice_snapshots()
    g = s["va"][T_FILTER]
    N, R = s["num_e"], 2 * s["num_r"]
    samples = torch.from_numpy(np.stack([g.src, g.rel, g.dst], axis=1)).to(device)
    P = samples.shape[0]
    loc, rec, all_loc, all_rec = (_ints(n, D_FILTER, k).to(device) for k, n in enumerate((g.n, g.n, N, N)))
    rel, rel2 = _ints(R, D_FILTER, 11).to(device), _ints(R, D_FILTER, 12).to(device)
    w = [_quarters(P, 20 + k).to(device) for k in range(4)]
    assert all(0.0 in x.tolist() and 1.0 in x.tolist() for x in w[:2])
    cls = {"base": EvaluationFilter, "gated": PostEvaluationFilter}.get(family, PostEnsembleEvaluationFilter)
    ev = cls(types.SimpleNamespace(score_function=name), SCORERS[name], s["tr"], s["va"], s["te"])
    if family == "base":
        call = lambda panel: ev.calc_metrics_single_graph(loc, rel, all_loc, samples, g, T_FILTER, panel=panel)
    elif family == "gated":
        call = lambda panel: ev.calc_metrics_single_graph(loc, rec, rel, all_loc, all_rec, samples, *w, g, T_FILTER, panel=panel)
    else:
        kw = dict(rel_enc_temporal=rel2) if family == "ensemble_two_rel" else {}
        call = lambda panel: ev.calc_metrics_single_graph(loc, rec, rel, all_loc, all_rec, w[0], w[1], samples, g, T_FILTER, panel=panel, **kw)
    return call, P, N


def check_filter_panels(family, name, device, panels=None):
    """calc_metrics_single_graph(panel=p) == (panel=None) exactly, p in {8, 64, "auto", N rounded up to 4}."""
    call, P, N = filter_call(family, name, device)
    want = call(None)
    assert want.dtype == torch.int64 and tuple(want.shape) == (2 * P,) and int(want.min()) >= 1 and int(want.max()) <= N
    assert int(want.max()) > 1
    for panel in panels or (8, 64, "auto", (N + 3) // 4 * 4):
        got = call(panel)
        assert got.dtype == torch.int64 and torch.equal(got, want), (family, name, panel)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def band_check(ranks, z, split, min_safe, what):
    """The goldens' own comparison (window_cases.check_evaluate / check_post_ensemble_evaluate, aggregator_cases.check_golden_ranks):
    rows with no competitor inside the reference's fp32 tie band -- at least `min_safe` of them -- equal the reference's rank, every
    other row is within its band population."""
    from tests.golden_util import T
    want, nclose = T(z["ranks_" + split]).long(), T(z["nclose_" + split]).long()
    got = ranks.cpu()
    assert got.shape == want.shape, what
    safe = nclose == 0
    assert safe.float().mean().item() >= min_safe, what
    assert torch.equal(got[safe], want[safe]), (what, int((got[safe] != want[safe]).sum()))
    assert bool(((got - want).abs() <= nclose).all()), what


def golden_model(name, device):
    """-> (model, z, the share of safe rows the golden's own test asks for)."""
    from tests.golden_util import load
    from tests import window_cases as WC
    z = load(name)
    if name.startswith("G13"):
        return WC.build_window_model(z, device), z, 0.85 + 1e-9
    if name.startswith("G18"):
        from temp_amd.post_dynamic_rgcn import PostEnsembleBiDynamicRGCN, PostEnsembleDynamicRGCN
        bi = str(z["module"]).startswith("Bi")
        m = WC.build_post_model(z, device, PostEnsembleBiDynamicRGCN if bi else PostEnsembleDynamicRGCN, True, post_ensemble=True)
        with torch.no_grad():
            m.rel_embeds.mul_(float(z["rel_scale"]))
        m.calc_ensemble_ratio = WC.g18_ratio
        return m, z, 0.85 + 1e-9
    from tests import aggregator_cases as AC
    return AC.golden_model(z, device).eval(), z, 0.75


def check_model(name, device, panels=(64, "auto")):
    """eval_panel is None by default and evaluate() then is the present route (before and after the attribute was used); with
    eval_panel set evaluate() passes the golden's comparison."""
    m, z, min_safe = golden_model(name, device)
    t_list = [int(t) for t in z["t_list"]]
    assert m.eval_panel is None and type(m).eval_panel is None
    for split, val in (("val", True), ("test", False)):
        base, _ = m.evaluate(torch.tensor(t_list), val=val)
        band_check(base, z, split, min_safe, (name, split, None))
        for panel in panels:
            m.eval_panel = panel
            try:
                got, _ = m.evaluate(torch.tensor(t_list), val=val)
            finally:
                m.eval_panel = None
            assert got.dtype == torch.int64
            band_check(got, z, split, min_safe, (name, split, panel))
        again, _ = m.evaluate(torch.tensor(t_list), val=val)
        assert torch.equal(again, base)
