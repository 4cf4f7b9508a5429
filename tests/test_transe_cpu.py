"""TransE (L1) route without a GPU: the fp64 references of tests/transe_cases.py against the oracle's scorer and torch autograd,
the input conditions the GPU tests rely on, and the autograd nodes / the tkg_module and evaluation dispatch driven through a
test backend that implements the L1 methods in torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import temp_oracle as O
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import scores as SC
from tests import transe_cases as TC
from tests.cpu_backend import CpuTestBackend
from tests.golden_util import assert_close, load
from tests.window_cases import build_window_model, make_args, slice_snapshots


class L1CpuBackend(CpuTestBackend):
    """CpuTestBackend + the contract of the L1 entry points (include/temp_amd.h) in torch."""
    name = "cpu-test-l1"

    def __init__(self):
        self.calls = []

    def bilinear_query_fwd(self, kind, ent_rows, known_idx, rel, rel_idx, is_tail):
        if kind != "transE":
            return super().bilinear_query_fwd(kind, ent_rows, known_idx, rel, rel_idx, is_tail)
        k, r = ent_rows.detach()[known_idx.long()], rel.detach()[rel_idx.long()]
        return torch.where(is_tail.view(-1, 1) != 0, k + r, k - r)

    def bilinear_query_bwd(self, kind, ent_rows, known_idx, rel, rel_idx, is_tail, d_q):
        if kind != "transE":
            return super().bilinear_query_bwd(kind, ent_rows, known_idx, rel, rel_idx, is_tail, d_q)
        return d_q, torch.where(is_tail.view(-1, 1) != 0, d_q, -d_q)

    @staticmethod
    def _rows(base, cand):
        return cand.long() if base is None else cand.long() + base.long().view(-1, 1)

    def l1_ce_fwd(self, q, table, base, cand):
        self.calls.append("l1_ce_fwd")
        s = -(q.detach().unsqueeze(1) - table.detach()[self._rows(base, cand)]).abs().sum(dim=-1)
        lse = torch.logsumexp(s, dim=1)
        return s, lse - s[:, 0], lse

    def l1_ce_bwd_q(self, q, table, base, cand, s, lse, scale, inv_rows, row_scale=None):
        self.calls.append("l1_ce_bwd_q")
        g = torch.exp(s - lse.view(-1, 1))
        g[:, 0] -= 1.0
        g = g * (scale.reshape(-1)[0] * (row_scale.view(-1, 1) if row_scale is not None else inv_rows))
        sg = torch.sign(q.detach().unsqueeze(1) - table.detach()[self._rows(base, cand)])
        return g, -(g.unsqueeze(-1) * sg).sum(dim=1)

    def l1_ce_bwd_table(self, q, table, slot_ptr, slot, g):
        self.calls.append("l1_ce_bwd_table")
        C = g.shape[1]
        cnt = (slot_ptr[1:] - slot_ptr[:-1]).long()
        assert int(cnt.sum()) == slot.numel() == g.numel()
        n = torch.repeat_interleave(torch.arange(table.shape[0]), cnt)
        sl = slot.long()
        same = n[1:] == n[:-1]
        assert bool((sl[1:][same] > sl[:-1][same]).all()), "slots must ascend within a table row"
        terms = g.reshape(-1)[sl].view(-1, 1) * torch.sign(q.detach()[sl // C] - table.detach()[n])
        return torch.zeros_like(table).index_add_(0, n, terms)

    def l1_scores(self, q, table):
        self.calls.append("l1_scores")
        s = -torch.cdist(q.detach(), table.detach(), p=1)
        N = table.shape[0]
        pad = (-N) % 4
        return torch.cat([s, s.new_full((s.shape[0], pad), float("-inf"))], dim=1) if pad else s


@pytest.fixture
def l1_backend():
    be = L1CpuBackend()
    TB.set_backend(be)
    yield be
    TB.set_backend(None)


@pytest.fixture
def plain_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


SMALL = [c for c in TC.CANDIDATE_CASES if c[0] * c[1] * c[2] <= 200 * 101 * 67]


@pytest.mark.parametrize("d,C,P,rows,windows", SMALL)
def test_references_against_oracle_and_autograd(d, C, P, rows, windows):
    """candidate_reference == the oracle's transE + F.cross_entropy and torch autograd of it, in fp64; the L1 test backend
    and the host slot lists satisfy the same contract."""
    case = TC.candidate_case(d, C, P, rows, windows)
    idx = TC.table_rows(case)
    for use_rs in (True, False):
        ref = TC.candidate_reference(case, use_rs)
        q = case["q"].double().requires_grad_(True)
        table = case["table"].double().requires_grad_(True)
        score = O.transE(q, torch.zeros_like(q), table[idx], mode="tail")
        assert_close(score, ref["s"], 1e-13, 1e-13, "scores")
        loss_rows = F.cross_entropy(score, torch.zeros(P, dtype=torch.int64), reduction="none")
        assert_close(loss_rows, ref["loss"], 1e-12, 1e-12, "loss")
        w = case["row_scale"].double() if use_rs else torch.full((P,), case["inv_rows"], dtype=torch.float64)
        (float(case["scale"][0]) * (w * loss_rows).sum()).backward()
        assert_close(q.grad, ref["d_q"], 1e-11, 1e-13, "d_q")
        assert_close(table.grad, ref["d_table"], 1e-11, 1e-13, "d_table")
        be = L1CpuBackend()
        s, loss, lse = be.l1_ce_fwd(case["q"], case["table"], case["base"], case["cand"])
        g, d_q = be.l1_ce_bwd_q(case["q"], case["table"], case["base"], case["cand"], s, lse, case["scale"], case["inv_rows"],
                                case["row_scale"] if use_rs else None)
        ptr, slot = TC.slot_lists(case)
        ptr2, slot2 = TF.l1_slots(case["cand"], case["base"], case["n_rows"])
        assert torch.equal(ptr, ptr2) and torch.equal(slot, slot2)
        d_t = be.l1_ce_bwd_table(case["q"], case["table"], ptr, slot, g)
        assert float((s.double() - ref["s"]).abs().sub(4 * ref["tol_s"]).max()) <= 0
        assert bool((d_q.double() - ref["d_q"]).abs().le(4 * ref["eps"] * ref["a_q"]).all()), "backend d_q"
        assert bool((d_t.double() - ref["d_table"]).abs().le(4 * ref["eps"] * ref["a_table"]).all()), "backend d_table"
        if C == 1:
            assert float(ref["loss"].abs().max()) == 0.0 and float(ref["d_q"].abs().max()) == 0.0


@pytest.mark.parametrize("P,N,d,ld", TC.SCORE_CASES)
def test_score_reference_against_oracle(P, N, d, ld):
    c = TC.score_case(P, N, d)
    want = O.transE(c["q"].double(), torch.zeros(P, d, dtype=torch.float64), c["table"].double().unsqueeze(0), mode="tail")
    assert_close(c["s64"], want, 1e-13, 1e-13, "dense scores")
    assert float(c["s64"].min()) > -100.0                    # above the fp32 sigmoid's underflow: no ties by entity id
    # a strictly sequential fp32 sum (the dense kernel's order) and torch's stay inside the bound
    seq = torch.zeros(P, N)
    for k in range(d):
        seq = seq + (c["q"][:, k:k + 1] - c["table"][:, k].view(1, -1)).abs()
    assert bool(((-seq).double() - c["s64"]).abs().le(c["tol"]).all())


@pytest.mark.parametrize("P,N,d,ld", TC.SCORE_CASES[:2])
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_band_input_condition(P, N, d, ld, filtered):
    """At most 25 % of the rows have a band wider than one rank; the fp32 test backend's ranks lie inside it."""
    c = TC.score_case(P, N, d)
    target, ptr, ids = TC.rank_inputs(P, N)
    if not filtered:
        ptr = ids = None
    lo, hi = TC.rank_band(c["s64"], c["tol"], target, ptr, ids)
    assert bool((lo <= hi).all()) and float((lo != hi).float().mean()) <= 0.25
    be = L1CpuBackend()
    ranks = be.filtered_rank(be.l1_scores(c["q"], c["table"]), target, ptr, ids)
    assert bool(((ranks >= lo) & (ranks <= hi)).all())


def _transe_window_model():
    z = load("G10_bi_grrgcn_rol")
    m = build_window_model(z, torch.device("cpu"))
    m.args.score_function = "transE"
    m.calc_score = SC.transE
    return m, torch.tensor([int(t) for t in z["t_list"]]), int(z["L"])


def _grads(m, loss):
    for p in m.parameters():
        p.grad = None
    loss.backward()
    return m.ent_embeds.grad.clone(), m.rel_embeds.grad.clone(), m.ent_encoder.layer_1.loop_weight.grad.clone()


def test_window_model_nodes_equal_tensor_path(l1_backend):
    """The batched node (planned and injected samples) and the per-graph node against fused_loss = False: loss and gradients."""
    m, t_list, L = _transe_window_model()
    assert m.fused_loss_ok(m.embed_size) and not m.bilinear_loss_ok(m.embed_size)
    m.sample_rng = np.random.default_rng(3)
    wb = m.prepare(t_list, L, train=True)
    plan = wb.loss_plan
    assert plan is not None, "TransE gets the planned loss on a backend with the L1 methods"
    m.seed_rng = np.random.default_rng(7)
    planned = m.run_loss(wb)
    m.seed_rng = np.random.default_rng(7)
    cand = l1_backend.corrupt_sample(int(m.seed_rng.integers(1 << 62)), plan["truth"], plan["lo"], plan["hi"], plan["ids"],
                                     m.args.negative_rate, m.num_ents)
    samples = []
    for b, (a0, a1) in enumerate(plan["splits"]):
        P = plan["triples"][b].shape[0]
        samples.append((torch.from_numpy(plan["triples"][b]), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))
    l1_backend.calls.clear()
    fused = m.run_loss(wb, samples)
    assert abs(planned.item() - fused.item()) < 2e-5 * max(1.0, abs(fused.item()))
    gf = _grads(m, fused)
    assert l1_backend.calls == ["l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table"], l1_backend.calls
    inp = wb._loss_inputs[1]
    slots = inp["_l1_slots"]
    _grads(m, m.run_loss(wb, samples))
    assert inp["_l1_slots"] is slots, "the slot lists of a fixed sample set are built once"
    m.fused_loss = False
    l1_backend.calls.clear()
    ref = m.run_loss(wb, samples)
    gr = _grads(m, ref)
    assert l1_backend.calls == []
    assert abs(fused.item() - ref.item()) < 2e-5 * abs(ref.item())
    for x, y, what in zip(gf, gr, ("d ent_embeds", "d rel_embeds", "d encoder weight")):
        assert_close(x, y, 1e-4, 1e-5 * float(y.abs().max()), what)
    # the per-graph node (train_link_prediction / _both), one target graph
    m.fused_loss = True
    out, hist = m.run(wb)
    ent = out.split(wb.target.sizes)[0].detach().requires_grad_(True)
    all_e = torch.randn(m.num_ents, m.embed_size, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    trip, nt, nh = samples[0]
    labels = torch.zeros(trip.shape[0], dtype=torch.int64)
    res = []
    for fused_flag in (True, False):
        m.fused_loss = fused_flag
        for t in (ent, all_e):
            t.grad = None
        m.rel_embeds.grad = None
        both = m.train_link_prediction_both(ent, trip, nt, nh, labels, all_e)
        single = m.train_link_prediction(ent, trip, nh, labels, all_e, corrupt_tail=False)
        (both + single).backward()
        res.append((both.detach(), single.detach(), ent.grad.clone(), all_e.grad.clone(), m.rel_embeds.grad.clone()))
    m.fused_loss = True
    for x, y in zip(*res):
        assert_close(x, y, 1e-4, 1e-5 * float(y.abs().max()), "per-graph node")


def test_head_mode_input_condition_window_model(l1_backend):
    """No component of the head-mode difference of the window model's seeded samples lies within rounding of zero."""
    m, t_list, L = _transe_window_model()
    m.sample_rng = np.random.default_rng(3)
    wb = m.prepare(t_list, L, train=True)
    seen = {}
    fwd, ce = l1_backend.bilinear_query_fwd, l1_backend.l1_ce_fwd
    l1_backend.bilinear_query_fwd = lambda kind, e, k, r, ri, it: seen.setdefault("q", (e.detach(), k, r.detach(), ri, it)) and fwd(kind, e, k, r, ri, it)
    l1_backend.l1_ce_fwd = lambda q, t, b, c: seen.setdefault("ce", (t.detach(), b, c)) and ce(q, t, b, c)
    m.seed_rng = np.random.default_rng(7)
    m.run_loss(wb)
    e, k, r, ri, it = seen["q"]
    t, b, c = seen["ce"]
    head = torch.nonzero(it == 0).view(-1)
    assert head.numel() > 0
    cc, rr, oo = t[c[head].long() + b[head].long().view(-1, 1)], r[ri[head].long()], e[k[head].long()]
    assert TC.near_zero_components(cc, rr, oo) == 0
    # the mask finds what it is for: components at zero are exempt, components next to zero are counted
    o2, r2 = torch.randn(4, 8), torch.randn(4, 8)
    c2 = (o2 - r2).unsqueeze(1).repeat(1, 3, 1)
    c2[:, 1] += 1e-9
    c2[:, 2] += 0.5
    m = TC.near_zero_mask(c2, r2, o2)
    assert bool(m[:, 1].any()) and not bool(m[:, 2].any())


def _eval_inputs(D=16):
    s = slice_snapshots()
    t = s["times"][14]
    g = s["va"][t]
    N = s["num_e"]
    torch.manual_seed(5)
    all_e = torch.randn(N, D) * 0.5
    rel = torch.randn(2 * s["num_r"], D) * 0.5
    ent = all_e[torch.from_numpy(g.gids)]
    samples = torch.from_numpy(np.stack([g.src, g.rel, g.dst], axis=1))
    return s, t, g, N, all_e, rel, ent, samples


def test_evaluation_dispatch_equals_tensor_path(l1_backend):
    """calc_metrics_single_graph and the score-level ensemble filter take l1_scores for transE; ranks equal the chunked route on
    the rows the fp64 band marks unambiguous, inside the band elsewhere; at most 25 % of the rows ambiguous."""
    from temp_amd.evaluation import EvaluationFilter, PostEnsembleEvaluationFilter
    s, t, g, N, all_e, rel, ent, samples = _eval_inputs()
    args = make_args(score_function="transE")
    ev = EvaluationFilter(args, SC.transE, s["tr"], s["va"], s["te"])
    new = ev.calc_metrics_single_graph(ent, rel, all_e, samples, g, t)
    assert l1_backend.calls == ["l1_scores", "l1_scores"]
    TB.set_backend(CpuTestBackend())
    old = ev.calc_metrics_single_graph(ent, rel, all_e, samples, g, t)
    TB.set_backend(l1_backend)
    lo, hi = [], []
    for mode in ("head", "tail"):
        target, ptr, ids = ev._mode_inputs(mode, samples, g, int(t), N, all_e.device)
        known, r = ent[samples[:, 0] if mode == "tail" else samples[:, 2]], rel[samples[:, 1]]
        q = known + r if mode == "tail" else known - r
        s64 = -torch.cdist(q.double(), all_e.double(), p=1)
        a, b = TC.rank_band(s64, (all_e.shape[1] + 2) * TC.U * s64.abs(), target, ptr, ids)
        lo.append(a); hi.append(b)
    lo, hi = torch.cat(lo), torch.cat(hi)
    sure = lo == hi
    assert float((~sure).float().mean()) <= 0.25
    assert torch.equal(new[sure], old[sure]) and torch.equal(new[sure], lo[sure])
    assert bool(((new >= lo) & (new <= hi)).all()) and bool(((old >= lo) & (old <= hi)).all())
    # the score-level ensemble: the same score matrices through _score_matrix
    pe = PostEnsembleEvaluationFilter(args, SC.transE, s["tr"], s["va"], s["te"])
    ent2 = ent + 0.1
    w = torch.full((samples.shape[0], 1), 0.3)
    l1_backend.calls.clear()
    a = pe.calc_metrics_single_graph(ent, ent2, rel, all_e, all_e + 0.1, w, 1 - w, samples, g, t)
    assert l1_backend.calls == ["l1_scores"] * 4
    TB.set_backend(CpuTestBackend())
    b = pe.calc_metrics_single_graph(ent, ent2, rel, all_e, all_e + 0.1, w, 1 - w, samples, g, t)
    TB.set_backend(l1_backend)
    assert (a == b).float().mean() > 0.75 and int((a - b).abs().max()) <= 2


def test_plain_backend_keeps_the_tensor_path(plain_backend):
    """A backend without the L1 methods: no fused node, no planned loss, the chunked evaluation -- today's behaviour."""
    assert not TF.translation_supported()
    m, t_list, L = _transe_window_model()
    assert not m.fused_loss_ok(m.embed_size)
    m.sample_rng = np.random.default_rng(3)
    wb = m.prepare(t_list, L, train=True)
    assert wb.loss_plan is None
    loss = m.run_loss(wb)
    assert torch.isfinite(loss)
    loss.backward()
    assert torch.isfinite(m.ent_embeds.grad).all()


def test_static_model_takes_the_fused_node(l1_backend):
    """StaticRGCN with transE: the device sampler + the batched node on a backend with the L1 methods, equal to the per-graph
    tensor path on the same candidates; a width that is no multiple of 4 keeps the tensor path."""
    from temp_amd.static_rgcn import StaticRGCN
    s = slice_snapshots()
    args = make_args(module="SRGCN", embed_size=32, hidden_size=32, n_bases=16, score_function="transE")
    torch.manual_seed(5)
    m = StaticRGCN(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    assert m._fused_loss_ok()
    t_list = torch.tensor([20, 15, 9, 3])
    rng = np.random.default_rng(4)
    ids = [np.sort(rng.choice(s["tr"][int(t)].number_of_edges(), s["tr"][int(t)].number_of_edges() // 2, replace=False)) for t in t_list]
    m.sample_rng = np.random.default_rng(9)
    l1_backend.calls.clear()
    fused = m(t_list, target_edge_ids=ids)
    gf = (lambda: (fused.backward(), m.ent_embeds.grad.clone(), m.rel_embeds.grad.clone()))()[1:]
    assert l1_backend.calls == ["l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table"], l1_backend.calls
    plan, cand = m._last_plan
    samples = []
    for b, (a0, a1) in enumerate(plan["splits"]):
        P = plan["triples"][b].shape[0]
        samples.append((torch.from_numpy(plan["triples"][b]), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))
    m.ent_embeds.grad = m.rel_embeds.grad = None
    m.fused_loss = False
    ref = m(t_list, target_edge_ids=ids, samples=samples)
    ref.backward()
    assert abs(fused.item() - ref.item()) < 2e-5 * abs(ref.item())
    assert_close(gf[0], m.ent_embeds.grad, 1e-4, 1e-5 * float(m.ent_embeds.grad.abs().max()), "static d ent_embeds")
    assert_close(gf[1], m.rel_embeds.grad, 1e-4, 1e-5 * float(m.rel_embeds.grad.abs().max()), "static d rel_embeds")
    m.fused_loss = True
    m.hidden_size = 30                                       # (only the route decision reads it after construction)
    assert not m._fused_loss_ok()
