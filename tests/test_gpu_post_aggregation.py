"""Post-aggregation models on the MI355X: the C-ABI contracts of the gated kernels (temp_gated_query_*, temp_gather_ce_mix_*)
against fp64 torch, goldens G20 / G21 on the HIP path, the fused gated node against the fp64 restatement, and a config-3-shaped
training step of PostBiDynamicRGCN (HIP entry points called, bit-repeatable, HIP-graph replay == eager, evaluate())."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import post_aggregation_cases as PA
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


# ---------------------------------------------------------------------------------------------------------------------
# kernel contracts
# ---------------------------------------------------------------------------------------------------------------------
def _fold64(kind, k, r, is_tail):
    if kind == "distmult":
        return k * r
    h = k.shape[1] // 2
    rk, ik, rr, ir = k[:, :h], k[:, h:], r[:, :h], r[:, h:]
    sg = torch.where(is_tail.view(-1, 1) != 0, 1.0, -1.0).to(k.dtype)
    return torch.cat([rk * rr - sg * ik * ir, ik * rr + sg * rk * ir], dim=1)


@pytest.mark.parametrize("wmode", ["zero", "one", "random"])
@pytest.mark.parametrize("P", [1, 37, 3000])
@pytest.mark.parametrize("d", [32, 128, 200])
@pytest.mark.parametrize("kind", ["distmult", "complex"])
def test_gated_query_kernels_vs_fp64(kind, d, P, wmode):
    """temp_gated_query_fwd / _bwd: tail rows, head rows and temporal-only rows (a_idx < 0) against fp64 autograd."""
    g = torch.Generator().manual_seed(d * 7 + P)
    na, R2 = 300, 40
    A, B, rel = torch.randn(na, d, generator=g), torch.randn(na + 5, d, generator=g), torch.randn(R2, d, generator=g)
    ia = torch.randint(0, na, (P,), generator=g).int()
    ib = torch.randint(0, na + 5, (P,), generator=g).int()
    ia[torch.rand(P, generator=g) < 0.3] = -1                              # temporal-only rows
    ridx = torch.randint(0, R2, (P,), generator=g).int()
    tail = (torch.rand(P, generator=g) < 0.5).int()
    w = {"zero": torch.zeros(P), "one": torch.ones(P), "random": torch.rand(P, generator=g)}[wmode]
    dq = torch.randn(P, d, generator=g)
    A64, B64, r64, w64 = (x.double().requires_grad_(True) for x in (A, B, rel, w))
    gated = (ia >= 0).view(-1, 1)
    b_rows = B64[ib.long()]
    a_rows = A64[ia.long().clamp(min=0)]
    wc = w64.view(-1, 1)
    known = torch.where(gated, wc * a_rows + (1 - wc) * b_rows, b_rows)
    q64 = _fold64(kind, known, r64[ridx.long()], tail)
    q64.backward(dq.double())
    be = TB.get_backend()
    dev = lambda t: t.to(DEV)
    q = be.gated_query_fwd(kind, dev(A), dev(ia), dev(B), dev(ib), dev(w), dev(rel), dev(ridx), dev(tail))
    da, db, dr, dw = be.gated_query_bwd(kind, dev(A), dev(ia), dev(B), dev(ib), dev(w), dev(rel), dev(ridx), dev(tail), dev(dq))
    assert_close(q, q64, 1e-6, 1e-6, "gated query")
    # per-row gradients, summed over the index lists here the way the caller's segment sums do
    dA = torch.zeros(na, d, dtype=torch.float64).index_add_(0, ia.long().clamp(min=0), da.cpu().double() * gated)
    dB = torch.zeros(na + 5, d, dtype=torch.float64).index_add_(0, ib.long(), db.cpu().double())
    dR = torch.zeros(R2, d, dtype=torch.float64).index_add_(0, ridx.long(), dr.cpu().double())
    assert bool((da.cpu()[~gated.view(-1)] == 0).all()) and bool((dw.cpu()[~gated.view(-1)] == 0).all())
    assert_close(dA, A64.grad, 1e-5, 1e-5, "d A")
    assert_close(dB, B64.grad, 1e-5, 1e-5, "d B")
    assert_close(dR, r64.grad, 1e-5, 1e-5, "d rel")
    assert_close(dw, w64.grad, 1e-5, 1e-5, "d w")


def test_gated_kernels_reject_unaligned_width():
    """d % 4 != 0 (complex: d % 8 != 0) -> TEMP_E_UNSUPPORTED before anything is launched; the outputs stay untouched."""
    lib = _lib.load()
    P = 8
    for kind, d in ((_lib.SCORE_KINDS["distmult"], 30), (_lib.SCORE_KINDS["complex"], 36)):
        A = torch.randn(4, d, device=DEV)
        idx = torch.zeros(P, dtype=torch.int32, device=DEV)
        w = torch.rand(P, device=DEV)
        out = torch.full((P, d), 7.0, device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.temp_gated_query_fwd(P, d, kind, p(A), p(idx), p(A), p(idx), p(w), p(A), p(idx), p(idx), p(out), None)
        assert rc == 2
        rc = lib.temp_gated_query_bwd(P, d, kind, p(A), p(idx), p(A), p(idx), p(w), p(A), p(idx), p(idx), p(out), p(out), p(out), p(out),
                                      p(w), None)
        assert rc == 2
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())


@pytest.mark.parametrize("mag", [1.0, 1e3])
@pytest.mark.parametrize("row_scale", [False, True])
@pytest.mark.parametrize("N", [500, 2052])
@pytest.mark.parametrize("C", [2, 21, 101])
def test_gather_ce_mix_kernels_vs_fp64(C, N, row_scale, mag):
    """temp_gather_ce_mix_fwd / _bwd incl. d_w: duplicate candidates, row_scale set and null, both backward variants (N <= 1024:
    a wave per row; longer rows: a workgroup per row).  Unit scores at the bars of the gather_ce tests; scores of magnitude 1e3
    (lse stability) carry an fp32 rounding of ~1e-4 in the mixed score itself, so their softmax is known to ~1e-4 relative."""
    g = torch.Generator().manual_seed(C * 13 + N)
    P = 300
    s_a = torch.randn(P, N, generator=g) * mag
    s_b = torch.randn(P, N, generator=g) * mag
    w = torch.rand(P, generator=g)
    w[:5] = 0.0
    w[5:10] = 1.0
    cand = torch.randint(0, N, (P, C), generator=g).int()
    if C > 2:
        cand[:, 2] = cand[:, 1]
        cand[::3, 1] = cand[::3, 0]                                      # the truth listed twice
    rs = torch.rand(P, generator=g) if row_scale else None
    up = torch.tensor([0.7])
    a64, b64, w64 = (x.double().requires_grad_(True) for x in (s_a, s_b, w))
    m = w64.view(-1, 1) * a64.gather(1, cand.long()) + (1 - w64.view(-1, 1)) * b64.gather(1, cand.long())
    lse64 = torch.logsumexp(m, dim=1)
    loss_rows64 = lse64 - m[:, 0]
    scale64 = rs.double() if row_scale else torch.full((P,), 1.0 / P, dtype=torch.float64)
    (0.7 * (loss_rows64 * scale64).sum()).backward()
    be = TB.get_backend()
    dev = lambda t: t.to(DEV)
    loss_rows, lse = be.gather_ce_mix_fwd(dev(s_a), dev(s_b), dev(w), dev(cand))
    d_a, d_b, d_w = be.gather_ce_mix_bwd(dev(s_a), dev(s_b), dev(w), dev(cand), lse, dev(up), 1.0 / P, dev(rs) if row_scale else None)
    # at magnitude 1e3 the fp32 mixed score itself is only resolved to ~1e-4 (ulp of 2e3), so softmax terms carry ~1e-4 relative
    # error, and at a dominant truth column (softmax ~ 1, or ~ 1/2 when listed twice) G = cnt * softmax - 1 cancels to that absolute error
    rt, at = (2e-5, 2e-6) if mag == 1.0 else (3e-4, 1e-4)
    assert_close(loss_rows, loss_rows64, 2e-5, 2e-6 * mag, "loss rows")
    assert_close(lse, lse64, 2e-5, 2e-6 * mag, "lse")
    assert_close(d_a, a64.grad, rt, at, "d s_a")
    assert_close(d_b, b64.grad, rt, at, "d s_b")
    # d_w = sum_e G (s_a - s_b): the absolute error of G above, times |s_a - s_b|
    assert_close(d_w, w64.grad, rt, 2e-6 if mag == 1.0 else at * float((s_a - s_b).abs().max()), "d w")
    off = torch.ones(P, N, dtype=torch.bool).scatter_(1, cand.long(), False)
    assert bool((d_a.cpu()[off] == 0).all()) and bool((d_b.cpu()[off] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# goldens and the loss definition on the HIP path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("name", ["G20_post_agg_uni", "G20_post_agg_bi", "G20_post_agg_uni_full"])
def test_post_aggregation_own_gates_golden_gpu(name, batched):
    PA.check_g20(name, DEV, batched)


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("name", ["G21_eval_post_agg_uni", "G21_eval_post_agg_bi"])
def test_post_aggregation_evaluate_golden_gpu(name, batched):
    PA.check_g21(name, DEV, batched)


@pytest.mark.parametrize("kind,bi", [("complex", True), ("distmult", False)])
def test_gated_loss_definition_and_quirks_gpu(kind, bi):
    PA.check_gated_loss_definition(DEV, kind, bi)


@pytest.mark.parametrize("kind,bi", [("complex", True), ("distmult", False)])
def test_gated_loss_definition_wide_embeddings_gpu(kind, bi):
    """embed_size 320: the node's three segment sums run past 256 columns (more float4 columns than a wave has lanes)."""
    PA.check_gated_loss_definition(DEV, kind, bi, windows=3, P=37, C=21, D=320)


def test_gated_loss_definition_full_size_gpu():
    PA.check_gated_loss_definition(DEV, "complex", True, windows=3, P=1000, C=51, D=200, full_bar=True)


@pytest.mark.parametrize("kind", ["complex", "distmult"])
def test_gated_loss_per_window_equals_literal_gpu(kind):
    PA.check_per_window_equals_batched(DEV, kind)


# ---------------------------------------------------------------------------------------------------------------------
# config-3-shaped training step
# ---------------------------------------------------------------------------------------------------------------------
def _config3_model():
    import bench
    from temp_amd import synthetic
    from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN
    from temp_amd.sampling import CorruptTriples
    w = synthetic.workload("S-icews0515", seed=0)
    args = bench.make_args(w, "BiGRRGCN")
    args.post_aggregation = True
    torch.manual_seed(1)
    m = PostBiDynamicRGCN(args, w["num_ents"], w["num_rels"], w["snapshots"], w["snapshots"], w["snapshots"]).to(DEV)
    m.sample_rng = np.random.default_rng(2)
    m.corrupter = CorruptTriples(m.args, w["snapshots"], seed=5)
    wb = m.prepare(synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 3), w["L"], True)
    fixed = [tuple(x.to(DEV) for x in smp) for smp in m.draw_samples(wb)]
    return m, wb, fixed, w


def test_config3_post_aggregation_step_gpu():
    """Config-3-shaped step: captured as a HIP graph first (as bench.py does: the impute models keep the last step's local rows,
    and with them its autograd graph, on the prepared batch), replayed twice; then two eager steps that call the gated HIP entry
    points once each and equal each other and the replay bit for bit; then evaluate() end to end with the model's own gates."""
    m, wb, fixed, w = _config3_model()
    assert wb.batched
    params = [p for p in m.parameters()]

    def step():
        for p in params:
            p.grad = None
        loss = m.run_loss(wb, fixed)
        loss.backward()
        return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = m.run_loss(wb, fixed)
        loss.backward()
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]))
    be = TB.get_backend()
    calls = {}
    watched = ("gated_query_fwd", "gated_query_bwd", "gather_ce_mix_fwd", "gather_ce_mix_bwd", "bilinear_query_fwd", "gather_ce_fwd")
    for nm in watched:
        orig = getattr(be, nm)

        def wrap(*a, _nm=nm, _orig=orig, **k):
            calls[_nm] = calls.get(_nm, 0) + 1
            return _orig(*a, **k)
        setattr(be, nm, wrap)
    try:
        l1, g1 = step()
    finally:
        for nm in watched:
            be.__dict__.pop(nm, None)
    assert calls == {"gated_query_fwd": 1, "gated_query_bwd": 1, "gather_ce_mix_fwd": 1, "gather_ce_mix_bwd": 1}, calls
    assert torch.isfinite(l1) and float(l1) > 0
    for nm in ("subject_query_object_embed_linear", "object_query_object_embed_linear"):
        assert all(p.grad is None for p in getattr(m, nm).parameters()), nm
    l2, g2 = step()
    for lx, gx in [(l2, g2)] + replays:
        assert torch.equal(l1, lx)
        for a, b in zip(g1, gx):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    del graph
    from temp_amd import synthetic
    with torch.no_grad():
        ranks, _ = m.evaluate(synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 3)[:2], val=True)
    assert ranks.numel() > 0 and int(ranks.min()) >= 1 and int(ranks.max()) <= w["num_ents"]
