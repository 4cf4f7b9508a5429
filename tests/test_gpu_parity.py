"""GPU parity tests proper (-m gpu): the hand-written HIP kernels, called through the C ABI
(ctypes -> libtemp_amd.so), against (a) golden vectors recorded from the TeMP reference and
(b) the CPU oracle on seeded random inputs, including the edge cases the domain has: empty graph,
zero-in-degree nodes, hub nodes whose segment spans many chunks, duplicate edges, every block
shape (si=so=1,2,4 and a generic one), inactive previous rows (prev_idx = -1).
Tolerance: 1e-5 relative fp32 (+ absolute floor), as BASELINE.md states."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd.snapshot import Snapshot
from tests.cpu_backend import CpuTestBackend
from oracle import temp_oracle as O           # checker only (oracle/temp_oracle.py: the restatement pinned by the reference's goldens)
from tests.encoder_cases import check_G2, check_G4, check_G6, check_G7
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be


def test_library_loaded_is_in_tree():
    lib = _lib.load()
    assert lib.temp_abi_version() == 2
    assert _lib.LIB_PATH.endswith("temp_amd/libtemp_amd.so")


def test_G2_layer_golden():
    check_G2(DEV)


def test_G4_grrgcn_layer_golden():
    check_G4(DEV)


def test_G6_rrgcn_golden():
    check_G6(DEV)


def test_G7_birrgcn_golden():
    check_G7(DEV)


# ---------------------------------------------------------------------------------------------
def rand_graph(rng, n, E, R2, hub=False, dup=False):
    if E == 0:
        z = np.zeros(0, np.int64)
        return Snapshot(n, z, z, z, np.arange(n))
    src = rng.integers(0, n, E)
    dst = rng.integers(0, n, E)
    if hub:                               # a few destinations / sources with degree >> 64 (multi-chunk segments)
        dst[: E // 2] = rng.integers(0, 3, E // 2)
        src[E // 4: E // 2 + E // 4] = rng.integers(n - 2, n, E // 2)
    rel = rng.integers(0, R2, E)
    if dup:
        src[1::2], dst[1::2], rel[1::2] = src[0::2][: len(src[1::2])], dst[0::2][: len(src[1::2])], rel[0::2][: len(src[1::2])]
    # leave the upper part of the node range without in-edges sometimes: zero-in-degree rows
    return Snapshot(n, src, dst, rel, np.arange(n))


CASES = [
    # n, E, D, B, R2, hub, dup, bias, act
    (50, 0, 16, 8, 6, False, False, False, 0),          # empty graph
    (1, 1, 8, 2, 4, False, False, True, 1),             # single self edge, S=4
    (300, 900, 200, 100, 40, False, False, False, 0),   # BASELINE shape (2x2 blocks), LDS-resident table size
    (300, 5000, 200, 100, 460, True, False, True, 1),   # hubs -> multi-chunk + fix-up, big relation table
    (257, 2000, 128, 128, 24, True, True, False, 1),    # S=1 (shipped grid configs), duplicates
    (130, 700, 32, 8, 10, False, False, True, 0),       # S=4
    (90, 400, 24, 4, 10, True, False, True, 1),         # S=6 -> generic path
    (4000, 60000, 200, 100, 40, True, False, False, 0), # enough chunks for the persistent LDS-table variant
]


@pytest.mark.parametrize("case", CASES)
def test_rgcn_layer_vs_oracle(case, hip_backend):
    n, E, D, B, R2, hub, dup, bias, act = case
    rng = np.random.default_rng(hash(case) % (2 ** 31))
    g = rand_graph(rng, n, E, R2, hub, dup)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    S = D // B
    h, w, lw = f(n, D), f(R2, B * S * S) * 0.5, f(D, D) * 0.2
    b = f(D) if bias else None
    gy = f(n, D)
    cpu = CpuTestBackend()
    dg_c = g.device_graph(torch.device("cpu"), R2)
    want = cpu.rgcn_fwd(dg_c, h, None, w, lw, b, B, act)
    dg = g.device_graph(DEV, R2)
    cu = lambda t: t.to(DEV) if t is not None else None
    got = hip_backend.rgcn_fwd(dg, cu(h), None, cu(w), cu(lw), cu(b), B, act)
    assert_close(got, want, 1e-5, 5e-6, "rgcn_fwd %s" % (case,))
    wd = cpu.rgcn_bwd(dg_c, h, want, gy, w, lw, bias, B, act)
    gd = hip_backend.rgcn_bwd(dg, cu(h), got, cu(gy), cu(w), cu(lw), bias, B, act)
    scale = max(1.0, float(n) ** 0.5)
    assert_close(gd[0], wd[0], 1e-5, 5e-6, "d_h %s" % (case,))
    assert_close(gd[1], wd[1], 2e-5, 1e-5 * scale, "d_weight %s" % (case,))
    assert_close(gd[2], wd[2], 2e-5, 1e-5 * scale, "d_loop %s" % (case,))
    if bias:
        assert_close(gd[3], wd[3], 2e-5, 1e-5 * scale, "d_bias %s" % (case,))
    # the ORACLE itself (models/RGCN.py:53-104 restated, autograd for the gradients), not only the test backend
    # (run in fp64: a hub sums thousands of messages, and two fp32 summation orders differ by more than the 1e-5 bar)
    if E:
        og = O.SnapGraph(n, g.src, g.dst, g.rel, np.arange(n))
        og.nnorm, og.enorm = og.nnorm.double(), og.enorm.double()
        leaves = [t.double().requires_grad_(True) for t in (h, w, lw)] + ([b.double().requires_grad_(True)] if bias else [])
        oy = O.rgcn_layer(leaves[0], og, leaves[1], leaves[2], B, leaves[3] if bias else None, 'relu' if act else None)
        oy.backward(gy.double())
        f32 = lambda t: t.detach().float()
        assert_close(got, f32(oy), 1e-5, 5e-6, "rgcn_fwd vs oracle %s" % (case,))
        assert_close(gd[0], f32(leaves[0].grad), 1e-5, 5e-6, "d_h vs oracle %s" % (case,))
        assert_close(gd[1], f32(leaves[1].grad), 2e-5, 1e-5 * scale, "d_weight vs oracle %s" % (case,))
        assert_close(gd[2], f32(leaves[2].grad), 2e-5, 1e-5 * scale, "d_loop vs oracle %s" % (case,))


def test_rgcn_fused_gather_ids(hip_backend):
    rng = np.random.default_rng(5)
    n, E, D, B, R2, N = 200, 1500, 200, 100, 40, 1000
    g = rand_graph(rng, n, E, R2, hub=True)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    table, w, lw = f(N, D), f(R2, 2 * D) * 0.5, f(D, D) * 0.2
    ids = torch.from_numpy(rng.integers(0, N, n).astype(np.int32))
    dg = g.device_graph(DEV, R2)
    got = hip_backend.rgcn_fwd(dg, table.to(DEV), ids.to(DEV), w.to(DEV), lw.to(DEV), None, B, 0)
    want = hip_backend.rgcn_fwd(dg, table[ids.long()].to(DEV), None, w.to(DEV), lw.to(DEV), None, B, 0)
    assert torch.equal(got, want)            # same arithmetic, only the addressing differs


@pytest.mark.parametrize("n,D,act,bias", [(0, 16, 0, False), (1, 8, 1, True), (777, 200, 1, True), (5000, 128, 0, False)])
def test_rgcn_isolated_vs_oracle(n, D, act, bias, hip_backend):
    rng = np.random.default_rng(n + D)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    e, lw, gy = f(n, D), f(D, D) * 0.2, f(n, D)
    b = f(D) if bias else None
    cpu = CpuTestBackend()
    want = cpu.rgcn_isolated_fwd(e, lw, b, act)
    cu = lambda t: t.to(DEV) if t is not None else None
    got = hip_backend.rgcn_isolated_fwd(cu(e), cu(lw), cu(b), act)
    assert_close(got, want, 1e-5, 5e-6, "iso fwd")
    wd = cpu.rgcn_isolated_bwd(e, want, gy, lw, bias, act)
    gd = hip_backend.rgcn_isolated_bwd(cu(e), got, cu(gy), cu(lw), bias, act)
    scale = max(1.0, float(n) ** 0.5)
    assert_close(gd[0], wd[0], 1e-5, 5e-6, "iso d_e")
    assert_close(gd[1], wd[1], 2e-5, 1e-5 * scale, "iso d_loop")
    if bias:
        assert_close(gd[2], wd[2], 2e-5, 1e-5 * scale, "iso d_bias")
    if n:                                                    # the oracle (models/RGCN.py:78-89 restated)
        eo, lo = e.clone().requires_grad_(True), lw.clone().requires_grad_(True)
        oy = O.rgcn_layer_isolated(eo, lo, b, 'relu' if act else None)
        oy.backward(gy)
        assert_close(got, oy.detach(), 1e-5, 5e-6, "iso fwd vs oracle")
        assert_close(gd[0], eo.grad, 1e-5, 5e-6, "iso d_e vs oracle")
        assert_close(gd[1], lo.grad, 2e-5, 1e-5 * scale, "iso d_loop vs oracle")


@pytest.mark.parametrize("n,D,variant,learn,use_idx", [
    (0, 16, 0, False, False), (1, 8, 0, False, False), (333, 200, 0, False, True), (4000, 200, 0, False, True),
    (500, 128, 1, False, False), (260, 32, 0, True, True), (129, 24, 1, True, True)])
def test_gru_step_vs_oracle(n, D, variant, learn, use_idx, hip_backend):
    rng = np.random.default_rng(n * 7 + D + variant)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    k = 1.0 / np.sqrt(D)
    gi_w = D if variant == 1 else 3 * D
    x, w_ih, w_hh, b_ih, b_hh = f(n, D), f(gi_w, D) * k, f(3 * D, D) * k, f(gi_w) * k, f(3 * D) * k
    n_prev = max(n + 13, 1)
    prev = f(n_prev, D) if use_idx else f(n, D)
    idx = None
    if use_idx:
        perm = rng.permutation(n_prev)[:n].astype(np.int32)
        perm[rng.random(n) < 0.3] = -1                      # inactive at the previous window position (F8)
        idx = torch.from_numpy(perm)
    dt = torch.from_numpy(rng.integers(0, 9, n).astype(np.float32))
    wb = torch.tensor([0.3, -0.4]) if learn else None
    gy = f(n, D)
    cpu = CpuTestBackend()
    cu = lambda t: t.to(DEV) if t is not None else None
    want, saved_c = cpu.gru_fwd(x, prev, idx, dt, 0.1, wb, w_ih, w_hh, b_ih, b_hh, variant)
    got, saved = hip_backend.gru_fwd(cu(x), cu(prev), cu(idx), cu(dt), 0.1, cu(wb), cu(w_ih), cu(w_hh), cu(b_ih), cu(b_hh), variant)
    assert_close(got, want, 1e-5, 2e-6, "gru fwd")
    if n:                                                    # the oracle (models/RRGCN.py:77-89 / models/GRU_cell.py:18-30 restated)
        pv = prev if idx is None else prev[idx.long().clamp(min=0)] * (idx >= 0).float().view(-1, 1)
        hdec = O.decay_hidden(pv, dt, 0.1, (wb[0], wb[1]) if learn else None)
        oy = (O.gru_type1 if variant == 1 else O.gru_torch)(x, hdec, w_ih, w_hh, b_ih, b_hh)
        assert_close(got, oy, 1e-5, 2e-6, "gru fwd vs oracle")
    wd = cpu.gru_bwd(x, prev, idx, dt, 0.1, wb, w_ih, w_hh, saved_c, gy, variant)
    gd = hip_backend.gru_bwd(cu(x), cu(prev), cu(idx), cu(dt), 0.1, cu(wb), cu(w_ih), cu(w_hh), saved, cu(gy), variant)
    scale = max(1.0, float(n) ** 0.5)
    assert_close(gd[0], wd[0], 2e-5, 2e-6, "gru d_x")
    d_prev_got, d_prev_want = gd[1], wd[1]
    if idx is not None:                                      # rows with idx == -1 carry no gradient
        keep = (idx >= 0)
        d_prev_got, d_prev_want = gd[1][keep.to(DEV)], wd[1][keep]
    assert_close(d_prev_got, d_prev_want, 2e-5, 2e-6, "gru d_prev")
    for i, nm in ((2, "d_w_ih"), (3, "d_w_hh"), (4, "d_b_ih"), (5, "d_b_hh")):
        assert_close(gd[i], wd[i], 3e-5, 1e-5 * scale, "gru " + nm)
    if learn:
        assert_close(gd[6], wd[6], 1e-4, 1e-4 * scale, "gru d_decay")


def test_gather_scatter_rows(hip_backend):
    rng = np.random.default_rng(3)
    table = torch.from_numpy(rng.standard_normal((100, 200)).astype(np.float32)).to(DEV)
    idx = torch.from_numpy(rng.integers(-1, 100, 5000).astype(np.int32)).to(DEV)
    out = hip_backend.gather_rows(table, idx)
    i = idx.long()
    want = table[i.clamp(min=0)] * (i >= 0).float().view(-1, 1)
    assert torch.equal(out, want)
    src = torch.from_numpy(rng.integers(-8, 8, (5000, 200)).astype(np.float32)).to(DEV)   # integers: order-independent sum
    acc = torch.zeros(100, 200, device=DEV)
    hip_backend.scatter_add_rows(src, idx, acc)
    ref = torch.zeros(100, 200, device=DEV).index_add_(0, i[i >= 0], src[i >= 0])
    assert torch.equal(acc, ref)


def test_determinism_bitwise(hip_backend):
    """No atomics in the encoder kernels: two runs give identical bits."""
    rng = np.random.default_rng(9)
    g = rand_graph(rng, 500, 20000, 40, hub=True)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    h, w, lw, gy = f(500, 200), f(40, 400), f(200, 200), f(500, 200)
    dg = g.device_graph(DEV, 40)
    a = hip_backend.rgcn_fwd(dg, h, None, w, lw, None, 100, 1)
    b = hip_backend.rgcn_fwd(dg, h, None, w, lw, None, 100, 1)
    assert torch.equal(a, b)
    ga = hip_backend.rgcn_bwd(dg, h, a, gy, w, lw, False, 100, 1)
    gb = hip_backend.rgcn_bwd(dg, h, a, gy, w, lw, False, 100, 1)
    for u, v in zip(ga[:3], gb[:3]):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------
# window level: DynamicRGCN / BiDynamicRGCN / StaticRGCN .forward on the ICEWS14 slice (G10, G12)
# ---------------------------------------------------------------------------------------------
from tests.window_cases import check_batched_equals_generic, check_static, check_window  # noqa: E402


@pytest.mark.parametrize("name", ["G10_uni_grrgcn", "G10_uni_grrgcn_rol", "G10_bi_grrgcn_rol", "G10_bi_grrgcn",
                                  "G10_uni_grrgcn_d200", "G10_bi_grrgcn_rol_d200"])
def test_window_loss_and_grads_golden_gpu(name):
    check_window(name, DEV)


def test_default_flags_position_loop_golden_gpu():
    """The reference's default flags (both layers recurrent; G10_uni_grrgcn) through the reference-granular loop of
    RRGCN.forward calls; the test above takes the same golden through the one-node loop (temp_amd/rec_stack.py)."""
    m = check_window("G10_uni_grrgcn", DEV, stack=False)
    assert m._can_stack() is False


@pytest.mark.parametrize("type1,width", [(False, None), (True, None), (False, 200)])
def test_default_flags_stack_equals_generic_gpu(type1, width):
    """(width 200: the split-operand GEMMs and the 200-wide cell kernels; 100 bases of 2 x 2 blocks)"""
    from tests.window_cases import check_stack_equals_generic
    check_stack_equals_generic("G10_uni_grrgcn", DEV, type1, width)


@pytest.mark.parametrize("name", ["G10_uni_grrgcn_rol", "G10_bi_grrgcn_rol"])
def test_batched_equals_generic_gpu(name):
    check_batched_equals_generic(name, DEV)


def test_static_rgcn_golden_gpu():
    check_static(DEV)


@pytest.mark.parametrize("name", ["G13_eval_uni", "G13_eval_bi"])
def test_evaluate_ranks_golden_gpu(name):
    from tests.window_cases import check_evaluate
    check_evaluate(name, DEV)


@pytest.mark.parametrize("P,C,N,D", [(1, 3, 8, 8), (200, 51, 7128, 32), (3000, 501, 500, 200), (17, 501, 500, 200), (40, 1300, 4000, 32)])
def test_candidate_cross_entropy_vs_torch(P, C, N, D, hip_backend):
    """Fused link-prediction loss (one GEMM against all entities + candidate CE kernel) vs the
    reference formulation: gather (P, C, D) candidates, DistMult-style dot, F.cross_entropy(label 0)."""
    import torch.nn.functional as F
    from temp_amd import functional as TF
    rng = np.random.default_rng(P + C + N)
    q = torch.from_numpy(rng.standard_normal((P, D)).astype(np.float32) * 0.5).to(DEV).requires_grad_(True)
    E = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32) * 0.5).to(DEV).requires_grad_(True)
    cand = torch.from_numpy(rng.integers(0, N, (P, C)).astype(np.int32)).to(DEV)        # duplicates inside a row happen
    loss = TF.candidate_cross_entropy(q, E, cand)
    loss.backward()
    q2, E2 = q.detach().clone().requires_grad_(True), E.detach().clone().requires_grad_(True)
    score = (q2.unsqueeze(1) * E2[cand.long()]).sum(-1)
    want = F.cross_entropy(score, torch.zeros(P, dtype=torch.int64, device=DEV))
    want.backward()
    assert abs(loss.item() - want.item()) < 2e-5 * max(1.0, abs(want.item()))
    assert_close(q.grad, q2.grad, 2e-5, 2e-6, "d_query")
    assert_close(E.grad, E2.grad, 2e-5, 2e-6, "d_all_embeds")


# ---------------------------------------------------------------------------------------------
# self-attention encoder (SARGCN, config 5): sparse history-attention kernel + window models (G14)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R,T,D,decay", [(1, 1, 1, 8, False), (37, 50, 6, 32, True), (300, 2000, 15, 200, False),
                                           (1000, 700, 29, 200, True), (65, 10, 4, 64, True), (33, 9, 3, 512, False)])
def test_history_attention_kernel_vs_dense(n, R, T, D, decay, hip_backend):
    """temp_sa_attn_fwd / _bwd against the dense softmax formulation (test backend) on random rows:
    all-masked rows, repeated history rows, every per-lane column count (d_k = 1 .. 64)."""
    rng = np.random.default_rng(n * 7 + T)
    cpu = CpuTestBackend()
    qkv = torch.from_numpy(rng.standard_normal((n, 3 * D)).astype(np.float32))
    kvh = torch.from_numpy(rng.standard_normal((R, 2 * D)).astype(np.float32))
    idx = rng.integers(0, R, (n, T - 1)).astype(np.int32)
    idx[rng.random((n, T - 1)) < 0.6] = -1
    if n > 2 and T > 1:
        idx[0] = -1                                # only the current position is alive
        idx[1] = 0                                 # every position reads the same history row
    idx = torch.from_numpy(idx)
    dec = torch.from_numpy(-rng.random(T).astype(np.float32)) if decay else None
    d_out = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
    dev = lambda t: t.to(DEV) if t is not None else None
    out, score, lse = hip_backend.sa_attn_fwd(dev(qkv), dev(kvh), dev(idx), dev(dec))
    w_out, w_score, w_lse = cpu.sa_attn_fwd(qkv, kvh, idx, dec)
    assert_close(out, w_out, 1e-5, 2e-6, "attn out")
    assert_close(lse, w_lse, 1e-5, 2e-6, "attn lse")
    live = torch.isfinite(w_score)
    assert torch.equal(torch.isfinite(score).cpu(), live)
    assert_close(torch.where(live, score.cpu(), torch.zeros(())), torch.where(live, w_score, torch.zeros(())), 1e-5, 2e-6, "attn score")
    g = hip_backend.sa_attn_bwd(dev(qkv), dev(kvh), dev(idx), dev(dec), out, score, lse, dev(d_out))
    w = cpu.sa_attn_bwd(qkv, kvh, idx, dec, w_out, w_score, w_lse, d_out)
    assert_close(g[0], w[0], 2e-5, 3e-6, "d_qkv")
    assert_close(g[1], w[1], 2e-5, 3e-6, "d_kv_hist")
    if decay:
        assert_close(g[2], w[2], 5e-5, 2e-5, "d_decay")
    else:
        assert g[2] is None
    if T > 1:                                      # deterministic two-pass form: same values, bitwise repeatable
        from temp_amd import functional as TF
        inv = TF.attention_inverse(idx.numpy(), R, DEV)
        g1 = hip_backend.sa_attn_bwd(dev(qkv), dev(kvh), dev(idx), dev(dec), out, score, lse, dev(d_out), inv)
        g2 = hip_backend.sa_attn_bwd(dev(qkv), dev(kvh), dev(idx), dev(dec), out, score, lse, dev(d_out), inv)
        assert_close(g1[0], w[0], 2e-5, 3e-6, "d_qkv (table pass)")
        assert_close(g1[1], w[1], 2e-5, 3e-6, "d_kv_hist (table pass)")
        assert torch.equal(g1[1], g2[1]) and torch.equal(g1[0], g2[0])


@pytest.mark.parametrize("name", ["G14_sa_uni_rol", "G14_sa_uni", "G14_sa_bi_rol"])
def test_self_attention_window_golden_gpu(name):
    from tests.window_cases import check_sa_window
    check_sa_window(name, DEV)


def test_self_attention_dense_api_gpu():
    from tests.window_cases import check_sa_dense_api
    check_sa_dense_api(DEV)


@pytest.mark.parametrize("name", ["G14_sa_uni", "G14_sa_bi_rol"])
def test_self_attention_evaluate_gpu(name):
    from tests.window_cases import check_sa_evaluate
    check_sa_evaluate(name, DEV)


@pytest.mark.parametrize("kind", ["StaticRGCN", "SelfAttentionRGCN", "BiSelfAttentionRGCN"])
def test_evaluate_is_its_composition_gpu(kind):
    from tests.window_cases import check_evaluate_composition
    check_evaluate_composition(kind, DEV)


@pytest.mark.parametrize("rows,n,d", [(500, 100000, 200), (7128, 1800, 200), (64, 999, 32), (10, 0, 16), (3, 5000, 256),
                                       (40, 48000, 200), (1, 30000, 128)])      # the last two: split (two-stage) reduction
def test_segment_sum_matches_scatter_and_is_deterministic(rows, n, d, hip_backend):
    """temp_segment_sum_rows (deterministic adjoint of a static gather) against the atomic scatter-add."""
    from temp_amd import functional as TF
    rng = np.random.default_rng(rows + n)
    idx = rng.integers(-1, rows, n).astype(np.int32)                 # -1 rows contribute nothing
    src = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    seg_ptr, order = TF.gather_inverse(idx, rows, DEV)
    a = hip_backend.segment_sum_rows(src, seg_ptr, order, rows)
    b = hip_backend.segment_sum_rows(src, seg_ptr, order, rows)
    assert torch.equal(a, b)
    want = torch.zeros(rows, d, dtype=torch.float64)
    keep = idx >= 0
    want.index_add_(0, torch.from_numpy(idx[keep].astype(np.int64)), src.cpu().double()[torch.from_numpy(keep)])
    assert_close(a, want.float(), 1e-5, 1e-5 * max(1.0, (n / max(rows, 1)) ** 0.5), "segment sum")


@pytest.mark.parametrize("rows,n,d,a,relu", [(4000, 48000, 200, 1.2, False), (7691, 48013, 200, 1.1, True), (300, 5000, 64, 1.5, True),
                                             (1000, 2001, 256, 2.0, False)])
def test_segment_sum_skewed_segments_gpu(rows, n, d, a, relu, hip_backend):
    """Zipf-distributed gather indices (a hub segment of thousands of rows among short and EMPTY ones: the loss path's known-entity
    gather): the fixed-piece kernels (2-32 rows per segment on average) against an fp64 index_add, with and without the folded
    ReLU adjoint; bit-repeatable."""
    from temp_amd import functional as TF
    rng = np.random.default_rng(rows + n)
    p = 1.0 / np.arange(1, rows + 1) ** a
    idx = rng.permutation(rows)[rng.choice(rows, size=n, p=p / p.sum())].astype(np.int32)
    idx[rng.integers(0, n, n // 50)] = -1
    src = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(DEV)
    table = torch.from_numpy(rng.standard_normal((rows, d)).astype(np.float32)).to(DEV).relu() if relu else None
    seg_ptr, order = TF.gather_inverse(idx, rows, DEV)
    cnt = np.bincount(idx[idx >= 0], minlength=rows)
    assert cnt.max() > 40 * max(1.0, np.median(cnt)) and (cnt == 0).any()
    run = lambda: hip_backend.segment_sum_rows(src, seg_ptr, order, rows, relu_of=table)
    got = run()
    assert torch.equal(got, run())
    want = torch.zeros(rows, d, dtype=torch.float64)
    keep = torch.from_numpy(idx >= 0)
    want.index_add_(0, torch.from_numpy(idx.astype(np.int64))[keep], src.cpu().double()[keep])
    if relu:
        want = want * (table.cpu() > 0)
    assert_close(got, want.float(), 1e-5, 2e-6 * float(cnt.max()) ** 0.5 + 1e-5, "skewed segment sum")


@pytest.mark.parametrize("n_table,n,E,D,B,R2,bias,act", [(500, 3000, 40000, 200, 100, 40, False, 0), (7128, 900, 2500, 200, 100, 460, True, 1),
                                                          (64, 300, 900, 32, 8, 10, True, 1), (50, 20, 0, 16, 8, 6, False, 0)])
def test_rgcn_table_layer_equals_gather_then_layer(n_table, n, E, D, B, R2, bias, act, hip_backend):
    """temp_rgcn_table_fwd/bwd (input = table[ids], self-loop through the table, per-table-row sums) against the plain
    layer on the materialised gather followed by the gather's adjoint."""
    from temp_amd import functional as TF
    rng = np.random.default_rng(n_table + n + E)
    g = rand_graph(rng, n, E, R2, hub=E > 1000)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    S = D // B
    table, w, lw = f(n_table, D), f(R2, B * S * S) * 0.5, f(D, D) * 0.2
    b = f(D) if bias else None
    gy = f(n, D)
    ids_np = rng.integers(0, n_table, n)
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(DEV)
    inv = TF.gather_inverse(ids_np, n_table, DEV)
    dg = g.device_graph(DEV, R2)
    h = table[ids.long()].contiguous()
    want = hip_backend.rgcn_fwd(dg, h, None, w, lw, b, B, act)
    got = hip_backend.rgcn_table_fwd(dg, table, ids, w, lw, b, B, act)
    assert_close(got, want, 1e-5, 5e-6, "table fwd")
    wd = hip_backend.rgcn_bwd(dg, h, want, gy, w, lw, bias, B, act)
    gd = hip_backend.rgcn_table_bwd(dg, table, ids, inv, got, gy, w, lw, bias, B, act)
    d_table = torch.zeros_like(table).index_add_(0, ids.long(), wd[0])
    scale = max(1.0, float(n) ** 0.5)
    assert_close(gd[0], d_table, 2e-5, 1e-5 * max(1.0, (n / n_table) ** 0.5), "d_table")
    assert_close(gd[1], wd[1], 2e-5, 1e-5 * scale, "d_weight")
    assert_close(gd[2], wd[2], 2e-5, 1e-5 * scale, "d_loop")
    if bias:
        assert_close(gd[3], wd[3], 2e-5, 1e-5 * scale, "d_bias")


def test_forward_with_device_sampler_end_to_end_gpu():
    """DynamicRGCN.forward with its own (device-side) negative sampler and target subsampling: finite loss, gradients
    on every parameter; the sampler's candidates never hit a true triple."""
    from tests.window_cases import build_window_model
    from tests.golden_util import load
    z = load("G10_bi_grrgcn_rol")
    m = build_window_model(z, DEV)
    loss = m(torch.tensor([20, 15, 9]))
    loss.backward()
    assert torch.isfinite(loss)
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}     # time_embed etc. are unused in this config
    assert {"ent_embeds", "rel_embeds", "ent_encoder.layer_1.weight", "ent_encoder.layer_2.forward_rnn.weight_hh_l0"} <= set(grads)
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert m._true_store.device.type == "cuda" and m._true_store.size > 0          # planned loss + one sampler launch
    wb = m.prepare(torch.tensor([20, 15, 9]), m.train_seq_len, train=True)
    trip, neg_tail, neg_head = m.draw_samples(wb)[0]                                 # the per-graph sampler interface
    assert m._dev_corrupter.device.type == "cuda" and neg_tail.is_cuda and neg_tail.shape == (trip.shape[0], 1 + m.args.negative_rate)


def test_full_size_step_properties_gpu():
    """BASELINE's full headline size (S-gdelt: 8 windows x 29 positions x 7 475 edges, D = 200), where the oracle is far too
    slow: size-independent properties instead --
      * the restructured step (distinct snapshots once, table layer, one GRU program, segment-sum adjoints) equals the
        reference-granular path (one encoder call per window position through the drop-in BiRRGCN API) on the same draws,
      * with and without snapshot de-duplication,
      * bitwise repeatable."""
    import bench
    from temp_amd import synthetic
    w = synthetic.workload("S-gdelt", seed=0)
    model = bench.build_model(w, DEV)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)

    def run(batched, dedup):
        model.use_batched_path, model.dedup_snapshots = batched, dedup
        model.sample_rng = np.random.default_rng(2)
        for p in model.parameters():
            p.grad = None
        wb = model.prepare(targets, w["L"], train=True)
        out = model.run(wb)[0]
        (out * out).sum().backward()
        return out.detach().clone(), model.ent_embeds.grad.clone(), model.ent_encoder.layer_2.forward_rnn.weight_hh_l0.grad.clone()

    a = run(True, True)
    b = run(True, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "step is not bitwise repeatable"
    c = run(True, False)
    g = run(False, True)
    for other, name in ((c, "no dedup"), (g, "reference-granular")):
        assert_close(other[0], a[0], 2e-5, 2e-6, "target embeddings vs " + name)
        assert_close(other[1], a[1], 1e-4, 1e-4 * float(a[1].abs().max()), "d ent_embeds vs " + name)
        assert_close(other[2], a[2], 1e-4, 1e-4 * float(a[2].abs().max()), "d W_hh vs " + name)
    model.use_batched_path, model.dedup_snapshots = True, True


def test_device_union_views_equal_host_union_gpu():
    """Snapshot store: union views assembled on the GPU from per-snapshot resident views are identical, array by array,
    to the host-assembled union (and to what a CPU device graph holds)."""
    from temp_amd import snapshot as S
    from temp_amd import synthetic
    w = synthetic.workload("S-gdelt", seed=0)
    parts = [w["snapshots"][t] for t in (3, 40, 7, 3 + 100, 12)]
    parts.append(parts[1].edge_subgraph(np.arange(0, parts[1].number_of_edges(), 2)))        # a subsampled target graph
    R2 = 2 * w["num_rels"]
    g = S.batch(parts)
    host_views, in_deg, out_deg = S.union_views(g, R2)
    dg = g.device_graph(DEV, R2)
    assert dg.offs is None, "device store path was not taken"
    for vn, hv in host_views.items():
        for k in ("n_seg", "n_edges", "n_chunks", "n_partial", "n_fix"):
            assert dg.views[vn][k] == hv[k], (vn, k)
        for an in S._VIEW_ARRAYS:
            assert np.array_equal(dg.view_tensor(vn, an).cpu().numpy(), hv[an]), (vn, an)
    assert np.array_equal(dg.in_deg.cpu().numpy(), in_deg) and np.array_equal(dg.out_deg.cpu().numpy(), out_deg)
    assert np.array_equal(dg.nnorm.cpu().numpy(), g.nnorm)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_self_loop_dropout_kernels_vs_cpu_backend(p, hip_backend):
    """Dropout of the self-loop message: the HIP kernels and the test backend derive the same keep mask from (seed, row,
    col), so layer / table layer / isolated layer agree with dropout on, forward and backward."""
    from temp_amd import functional as TF
    rng = np.random.default_rng(17)
    n, E, R2, D, B, n_table = 700, 5000, 12, 64, 16, 90
    g = rand_graph(rng, n, E, R2, hub=True)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    h, w, lw, b, gy = f(n, D), f(R2, B * 4 * 4) * 0.5, f(D, D) * 0.2, f(D), f(n, D)
    drop = (p, 0x1234ABCD5678 + int(p * 100))
    cpu = CpuTestBackend()
    dg_c, dg = g.device_graph(torch.device("cpu"), R2), g.device_graph(DEV, R2)
    cu = lambda t: t.to(DEV)
    want = cpu.rgcn_fwd(dg_c, h, None, w, lw, b, B, 1, drop)
    got = hip_backend.rgcn_fwd(dg, cu(h), None, cu(w), cu(lw), cu(b), B, 1, drop)
    assert_close(got, want, 1e-5, 5e-6, "dropout fwd")
    nodrop = hip_backend.rgcn_fwd(dg, cu(h), None, cu(w), cu(lw), cu(b), B, 1, None)
    assert not torch.allclose(got, nodrop)
    wd = cpu.rgcn_bwd(dg_c, h, want, gy, w, lw, True, B, 1, drop)
    gd = hip_backend.rgcn_bwd(dg, cu(h), got, cu(gy), cu(w), cu(lw), True, B, 1, drop)
    for a_, b_, nm in zip(gd, wd, ("d_h", "d_weight", "d_loop", "d_bias")):
        assert_close(a_, b_, 2e-5, 3e-4, "dropout " + nm)
    # table layer
    table = f(n_table, D)
    ids_np = rng.integers(0, n_table, n)
    ids = torch.from_numpy(ids_np.astype(np.int32))
    inv_c, inv = TF.gather_inverse(ids_np, n_table, torch.device("cpu")), TF.gather_inverse(ids_np, n_table, DEV)
    want = cpu.rgcn_table_fwd(dg_c, table, ids, w, lw, b, B, 0, drop)
    got = hip_backend.rgcn_table_fwd(dg, cu(table), cu(ids), cu(w), cu(lw), cu(b), B, 0, drop)
    assert_close(got, want, 1e-5, 5e-6, "dropout table fwd")
    wd = cpu.rgcn_table_bwd(dg_c, table, ids, inv_c, want, gy, w, lw, True, B, 0, drop)
    gd = hip_backend.rgcn_table_bwd(dg, cu(table), cu(ids), inv, got, cu(gy), cu(w), cu(lw), True, B, 0, drop)
    for a_, b_, nm in zip(gd, wd, ("d_table", "d_weight", "d_loop", "d_bias")):
        assert_close(a_, b_, 2e-5, 3e-4, "dropout table " + nm)
    # isolated layer
    e = f(n, D)
    want = cpu.rgcn_isolated_fwd(e, lw, b, 1, drop)
    got = hip_backend.rgcn_isolated_fwd(cu(e), cu(lw), cu(b), 1, drop)
    assert_close(got, want, 1e-5, 5e-6, "dropout iso fwd")
    wd = cpu.rgcn_isolated_bwd(e, want, gy, lw, True, 1, drop)
    gd = hip_backend.rgcn_isolated_bwd(cu(e), got, cu(gy), cu(lw), True, 1, drop)
    for a_, b_, nm in zip(gd, wd, ("d_e", "d_loop", "d_bias")):
        assert_close(a_, b_, 2e-5, 3e-4, "dropout iso " + nm)


def test_window_model_with_reference_default_dropout_gpu():
    """The reference's default --dropout is 0.1 (utils/args.py:17): the window models must train with it (self-loop message
    dropout in every RGCN layer, fresh mask per call) and be deterministic in eval mode."""
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    args = make_args(module="BiGRRGCN", rec_only_last_layer=True, dropout=0.1, train_seq_len=5, test_seq_len=5)
    torch.manual_seed(0)
    m = BiDynamicRGCN(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(DEV)
    t_list = torch.tensor([s["times"][i] for i in (15, 9, 4)])
    wb = m.prepare(t_list, 5, train=True)
    m.train()
    a = m.run(wb)[0]
    b = m.run(wb)[0]
    assert torch.isfinite(a).all() and not torch.equal(a, b), "training mode must draw a fresh dropout mask per call"
    (a * a).sum().backward()
    assert m.ent_encoder.layer_1.loop_weight.grad is not None and torch.isfinite(m.ent_encoder.layer_1.loop_weight.grad).all()
    m.eval()
    c, d = m.run(wb)[0], m.run(wb)[0]
    assert torch.equal(c, d)


@pytest.mark.parametrize("module,rec_only", [("BiGRRGCN", True), ("GRRGCN", True), ("GRRGCN", False)])
def test_reference_default_sizes_paths_agree_gpu(module, rec_only):
    """The reference's default hyper-parameters (utils/args.py: embed = hidden = 128, n_bases = 128 -> 1x1 blocks, 15-step
    windows): the restructured step and the reference-granular path (different kernels: streaming GEMMs, per-call GRU) agree
    on outputs and gradients, and with the CPU test backend on the outputs."""
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    from temp_amd.dynamic_rgcn import DynamicRGCN
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    args = make_args(module=module, rec_only_last_layer=rec_only, embed_size=128, hidden_size=128, n_bases=128, train_seq_len=15,
                     test_seq_len=15)
    cls = BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN
    torch.manual_seed(3)
    m = cls(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(DEV)
    m.device_subsample = False          # host sampler: the CPU test backend below must draw the SAME target subsets from the same rng
    t_list = torch.tensor([s["times"][i] for i in (20, 16, 11, 2)])
    res = []
    for batched in (True, False):
        m.use_batched_path = batched
        m.sample_rng = np.random.default_rng(4)
        for p in m.parameters():
            p.grad = None
        wb = m.prepare(t_list, 15, train=True)
        assert wb.batched == (batched and rec_only)
        out = m.run(wb)[0]
        (out * out).sum().backward()
        res.append((out.detach().clone(), m.ent_embeds.grad.clone(), m.ent_encoder.layer_1.weight.grad.clone()))
    assert_close(res[1][0], res[0][0], 2e-5, 2e-6, "outputs")
    assert_close(res[1][1], res[0][1], 1e-4, 1e-5 * float(res[0][1].abs().max() + 1), "d ent_embeds")
    assert_close(res[1][2], res[0][2], 1e-4, 1e-5 * float(res[0][2].abs().max() + 1), "d weight")
    # same model on the CPU test backend (torch ops through the same views)
    TB.set_backend(CpuTestBackend())
    try:
        mc = cls(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
        mc.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
        mc.use_batched_path = False
        mc.sample_rng = np.random.default_rng(4)
        with torch.no_grad():
            want = mc.run(mc.prepare(t_list, 15, train=True))[0]
    finally:
        TB.set_backend(None)
    assert_close(res[0][0], want, 2e-5, 2e-6, "outputs vs CPU test backend")


@pytest.mark.parametrize("P,N", [(37, 500), (200, 7128), (7475, 500), (5, 10488), (0, 500)])
def test_filtered_rank_kernel_bit_exact(P, N):
    """temp_filtered_rank vs the test backend's masked-sigmoid counting on the same score matrix.  Scores are multiples of
    0.25 (distinct scores differ by far more than an ulp after the sigmoid, so only EXACT ties occur -- many of them) plus
    saturated rows (|score| >= 20: sigmoid is exactly 1 resp. < 1e-8) and filter lists that contain the target."""
    g = torch.Generator().manual_seed(P * 31 + N)
    sc = torch.randint(-32, 33, (P, N), generator=g).float() * 0.25
    if P:
        sc[::3] = torch.randint(-3, 4, (sc[::3].shape[0], N), generator=g).float() * 20.0
    tgt = torch.randint(0, N, (P,), generator=g).int()
    cnt = torch.randint(0, 40, (P,), generator=g)
    if P:
        cnt[0] = 0
    ptr = torch.zeros(P + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(cnt, 0).int()
    ids = torch.cat([torch.randperm(N, generator=g)[:c].sort().values for c in cnt.tolist()] + [torch.zeros(0, dtype=torch.int64)]).int()
    if P > 1:
        ids[ptr[1]] = tgt[1]                                    # the target itself is listed: must be ignored
    want = CpuTestBackend().filtered_rank(sc, tgt, ptr, ids)
    got = TB.get_backend().filtered_rank(sc.to(DEV), tgt.to(DEV), ptr.to(DEV), ids.to(DEV)).cpu()
    assert torch.equal(got, want)
    want_raw = CpuTestBackend().filtered_rank(sc, tgt)
    got_raw = TB.get_backend().filtered_rank(sc.to(DEV), tgt.to(DEV)).cpu()
    assert torch.equal(got_raw, want_raw)
    if P:
        assert int(got.min()) >= 1 and int(got.max()) <= N and bool((got <= got_raw).all())


@pytest.mark.parametrize("kind,D", [("complex", 200), ("distmult", 200), ("complex", 32), ("distmult", 36)])
def test_bilinear_query_kernels_vs_scores_module(kind, D):
    """temp_bilinear_query_fwd / _bwd (row gathers fused) vs temp_amd.scores.bilinear_query + autograd on the CPU."""
    g = torch.Generator().manual_seed(D)
    n_rows, R2, P = 700, 40, 1531
    ent = torch.randn(n_rows, D, generator=g)
    rel = torch.randn(R2, D, generator=g)
    known = torch.randint(0, n_rows, (P,), generator=g).int()
    ridx = torch.randint(0, R2, (P,), generator=g).int()
    tail = (torch.rand(P, generator=g) < 0.5).int()
    dq = torch.randn(P, D, generator=g)
    ref = CpuTestBackend()
    want = ref.bilinear_query_fwd(kind, ent, known, rel, ridx, tail)
    wdk, wdr = ref.bilinear_query_bwd(kind, ent, known, rel, ridx, tail, dq)
    be = TB.get_backend()
    dev = lambda t: t.to(DEV)
    got = be.bilinear_query_fwd(kind, dev(ent), dev(known), dev(rel), dev(ridx), dev(tail))
    gdk, gdr = be.bilinear_query_bwd(kind, dev(ent), dev(known), dev(rel), dev(ridx), dev(tail), dev(dq))
    assert_close(got, want, 1e-6, 1e-6, "query")
    assert_close(gdk, wdk, 1e-6, 1e-6, "d known rows")
    assert_close(gdr, wdr, 1e-6, 1e-6, "d rel rows")
    # the folded query reproduces the scorer on explicit candidates (utils/scores.py semantics)
    from temp_amd import scores as SC
    cand = torch.randn(P, 3, D, generator=g)
    fn = getattr(SC, kind)
    k, r = ent[known.long()], rel[ridx.long()]
    s_tail = fn(k, r, cand, mode="tail")
    s_head = fn(cand, r, k, mode="head")
    want_s = torch.where(tail.view(-1, 1) != 0, s_tail, s_head)
    assert_close((got.cpu().unsqueeze(1) * cand).sum(-1), want_s, 1e-5, 1e-5, "score through the folded query")


def test_linear_multi_matches_single_products():
    g = torch.Generator().manual_seed(9)
    N, K = 500, 200
    Ms = [6000, 0, 4100, 37, 5000, 6000]
    a = [torch.randn(m, K, generator=g).to(DEV) for m in Ms]
    b = [torch.randn(N, K, generator=g).to(DEV) for _ in Ms]
    be = TB.get_backend()
    out = torch.empty(sum(Ms), N, device=DEV)
    be.linear_multi(a, b, True, out)
    row = 0
    for ai, bi in zip(a, b):
        assert_close(out[row:row + ai.shape[0]], ai.double() @ bi.double().t(), 1e-5, 1e-4, "A . B^T")
        row += ai.shape[0]
    b2 = [torch.randn(K, N, generator=g).to(DEV) for _ in Ms]          # not transposed: d_query = d_scores . all_embeds
    a2 = [torch.randn(m, K, generator=g).to(DEV) for m in Ms]
    out2 = torch.empty(sum(Ms), N, device=DEV)
    be.linear_multi(a2, b2, False, out2)
    row = 0
    for ai, bi in zip(a2, b2):
        assert_close(out2[row:row + ai.shape[0]], ai.double() @ bi.double(), 1e-5, 1e-4, "A . B")
        row += ai.shape[0]


def test_corrupt_sample_kernel_contract():
    """temp_corrupt_sample: column 0 = truth, draws in range and never in the row's known-true slice (short slices: linear
    scan, long ones: binary search), a pure function of the seed, uniform over the entities that are allowed."""
    g = torch.Generator().manual_seed(4)
    R, K, N = 3000, 500, 500
    truth = torch.randint(0, N, (R,), generator=g).int()
    cnt = torch.randint(0, 6, (R,), generator=g)
    cnt[::7] = 200                                               # long known-true sets (40 % of all entities)
    cnt[5] = N - 1                                               # a single allowed entity
    lists = [torch.randperm(N, generator=g)[:c].sort().values for c in cnt.tolist()]
    ids = torch.cat(lists).int()
    hi = torch.cumsum(cnt, 0).int()
    lo = hi - cnt.int()
    be = TB.get_backend()
    d = lambda t: t.to(DEV)
    a = be.corrupt_sample(11, d(truth), d(lo), d(hi), d(ids), K, N).cpu()
    b = be.corrupt_sample(11, d(truth), d(lo), d(hi), d(ids), K, N).cpu()
    c = be.corrupt_sample(12, d(truth), d(lo), d(hi), d(ids), K, N).cpu()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.shape == (R, K + 1) and torch.equal(a[:, 0], truth) and int(a.min()) >= 0 and int(a.max()) < N
    an = a.numpy()
    for r in range(R):
        assert not np.isin(an[r, 1:], lists[r].numpy()).any(), r
    allowed5 = np.setdiff1d(np.arange(N), lists[5].numpy())
    assert (an[5, 1:] == allowed5[0]).all()
    free = an[cnt.numpy() == 0][:, 1:]                           # unfiltered rows: uniform over [0, N)
    hist = np.bincount(free.reshape(-1), minlength=N)
    exp = free.size / N
    assert abs(hist - exp).max() < 6 * np.sqrt(exp)
    raw = be.corrupt_sample(3, d(truth), None, None, None, K, N).cpu()
    assert torch.equal(raw[:, 0], truth) and int(raw.max()) < N
    assert be.corrupt_sample(3, d(truth[:0]), None, None, None, K, N).shape == (0, K + 1)


def test_training_step_with_planned_loss_gpu():
    """The default training path on the GPU: prepare() plans the loss, run_loss draws negatives with ONE kernel launch;
    equal to feeding the same candidates through the samples= interface."""
    from tests.window_cases import build_window_model
    from tests.golden_util import load
    z = load("G10_bi_grrgcn_rol")
    m = build_window_model(z, DEV)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    m.sample_rng = np.random.default_rng(3)
    wb = m.prepare(t_list, int(z["L"]), train=True)
    plan = wb.loss_plan
    assert plan is not None
    m.seed_rng = np.random.default_rng(7)
    loss1 = m.run_loss(wb)
    m.seed_rng = np.random.default_rng(7)
    cand = TB.get_backend().corrupt_sample(int(m.seed_rng.integers(1 << 62)), plan["truth"], plan["lo"], plan["hi"], plan["ids"],
                                           m.args.negative_rate, m.num_ents)
    samples = []
    for b, (a0, a1) in enumerate(plan["splits"]):
        P = plan["triples"][b].shape[0]                          # (a block may end in weight-0 padding rows)
        samples.append((torch.from_numpy(plan["triples"][b]), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))
    loss2 = m.run_loss(wb, samples)
    assert abs(loss1.item() - loss2.item()) < 2e-5 * max(1.0, abs(loss2.item()))
    loss1.backward()
    assert torch.isfinite(m.ent_embeds.grad).all()


def test_full_size_loss_properties_gpu():
    """BASELINE's headline size with the link-prediction loss (8 windows, 500 entities, negative_rate 500): the fused loss node
    (folded-query kernel, multi-problem score GEMMs, counting CE, segment-sum adjoints) equals the reference-shaped
    formulation -- gather (P, 1 + neg, D) candidates, utils/scores.py complex(), F.cross_entropy -- on the same candidates,
    loss and gradients; and it is bitwise repeatable."""
    import bench
    from temp_amd import synthetic
    w = synthetic.workload("S-gdelt", seed=0)
    model = bench.build_model(w, DEV)
    model.args.num_pos_facts = 400                      # the reference-shaped path materialises P x 501 x D floats per direction
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    model.sample_rng = np.random.default_rng(2)
    wb = model.prepare(targets, w["L"], train=True)
    plan = wb.loss_plan
    assert plan is not None and plan["truth"].shape[0] == 8 * 2 * 400
    cand = TB.get_backend().corrupt_sample(99, plan["truth"], plan["lo"], plan["hi"], plan["ids"], model.args.negative_rate, model.num_ents)
    samples = []
    for b, (a0, a1) in enumerate(plan["splits"]):
        P = plan["triples"][b].shape[0]                          # (a block may end in weight-0 padding rows)
        samples.append((torch.from_numpy(plan["triples"][b]), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))

    def run(fused):
        model.fused_loss = fused
        for p in model.parameters():
            p.grad = None
        loss = model.run_loss(wb, samples)
        loss.backward()
        return loss.detach().clone(), model.ent_embeds.grad.clone(), model.rel_embeds.grad.clone()

    a = run(True)
    b = run(True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "fused loss is not bitwise repeatable"
    r = run(False)
    model.fused_loss = True
    assert abs(a[0].item() - r[0].item()) < 2e-5 * abs(r[0].item())
    assert_close(a[1], r[1], 1e-4, 1e-5 * float(r[1].abs().max()), "d ent_embeds, fused vs reference-shaped loss")
    assert_close(a[2], r[2], 1e-4, 1e-5 * float(r[2].abs().max()), "d rel_embeds, fused vs reference-shaped loss")


@pytest.mark.parametrize("M,N,K", [(10488, 184, 200), (7128, 400, 200), (300, 8, 16), (5000, 36, 128)])
def test_linear_t_transposed_store(M, N, K):
    """temp_linear_t: (A . B^T)^T written through the transposed-store epilogue == the plain product, transposed."""
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g).to(DEV)
    b = torch.randn(N, K, generator=g).to(DEV)
    out_t = torch.empty(N, M, device=DEV)
    TB.get_backend().linear_t(a, b, True, out_t)
    assert_close(out_t, (a.double() @ b.double().t()).t(), 1e-5, 1e-4, "linear_t")


def test_fused_loss_entity_major_variant_matches(monkeypatch):
    """The opt-in entity-major formulation of the fused loss (TEMP_LOSS_TALL=1: scores through temp_linear_t, backward from
    d_scores^T) equals the default one on an ICEWS-shaped batch -- and really is another route: the switch is patched in the module
    that owns it, and only the tall arm calls linear_t."""
    from temp_amd import link_loss as LL
    from tests.post_attention_cases import recording
    from tests.window_cases import build_window_model
    from tests.golden_util import load
    z = load("G10_bi_grrgcn_rol")
    m = build_window_model(z, DEV)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    m.sample_rng = np.random.default_rng(3)
    wb = m.prepare(t_list, int(z["L"]), train=True)
    res = []
    for tall in (False, True):
        monkeypatch.setattr(LL, "_TALL_SCORES", tall)
        for p in m.parameters():
            p.grad = None
        m.seed_rng = np.random.default_rng(7)
        with recording() as rec:
            loss = m.run_loss(wb)
            loss.backward()
        assert (rec.count("linear_t") > 0) == tall and (rec.count("linear_multi") > 0) != tall
        res.append((loss.detach().clone(), m.ent_embeds.grad.clone(), m.rel_embeds.grad.clone()))
    assert abs(res[0][0].item() - res[1][0].item()) < 2e-5 * abs(res[0][0].item())
    assert_close(res[1][1], res[0][1], 1e-4, 1e-5 * float(res[0][1].abs().max()), "d ent_embeds")
    assert_close(res[1][2], res[0][2], 1e-4, 1e-5 * float(res[0][2].abs().max()), "d rel_embeds")
