"""The SimplE pair fold (temp_bilinear_query_fwd / _bwd with TEMP_SCORE_SIMPLE), the pair table pass (temp_pair_rows_fwd / _bwd) and
the SimplE baseline on the MI355X: the kernels through the C ABI, bit for bit against their torch fp32 expressions, with canaries,
NaN-prefilled outputs and the argument checks; then the node and model cases of tests/simple_cases.py (goldens G28 / G29, fused
against per-graph route, prepared batches, an empty graph, the literal width, predict(), the state_dict round trip) on the HIP
path.

Why bit equality: the halving is exact, so every element of the fold and of its adjoint is ONE rounded fp32 product of two inputs,
whatever the order of the two multiplications; the pair forward is a copy, and its backward adds B fp32 numbers in ascending b
starting from zero, which is what the torch loop does."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import simple_cases as SP
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG, E_UNSUPPORTED = 1, 2
KIND = 3                            # include/temp_amd.h: TEMP_SCORE_SIMPLE

# (P, W): one row of two float4s; several rows; 5 float4s per half (a thread's row changes inside a wave); the widest rows the
# models use (D = 128); more than one block with W / 8 = 25 float4s per half (rows straddle blocks)
FOLD_CASES = [(1, 8), (5, 8), (37, 40), (300, 256), (1030, 200)]
# (B, N, d): one element; float4 with one column; the scalar route; 9 float4 columns; more windows than the adjoint's unroll; more
# than one block; 32 columns over five blocks
PAIR_CASES = [(1, 1, 1), (1, 5, 4), (3, 37, 6), (3, 37, 36), (9, 33, 8), (8, 300, 100), (2, 1030, 128)]


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


_FOLD = {}


def _fold_inputs(P, W):
    """Host inputs and the torch fp32 expectations, computed once per shape: fewer table rows than query rows, so known_idx and
    rel_idx repeat; both modes in one batch."""
    key = (P, W)
    if key not in _FOLD:
        rng = np.random.default_rng(100 * P + W)
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        n_ent, n_rel = max(1, P // 3), max(1, P // 7)
        rows, rel, dq = f(n_ent, W), f(n_rel, W), f(P, W)
        ki = torch.from_numpy(rng.integers(0, n_ent, P).astype(np.int32))
        ri = torch.from_numpy(rng.integers(0, n_rel, P).astype(np.int32))
        tail = torch.from_numpy((np.arange(P) % 3 != 1).astype(np.int32) * (1 + np.arange(P, dtype=np.int32) % 2))     # 0 / 1 / 2: any non-zero is tail
        if P > 1:
            assert 0 < int((tail != 0).sum()) < P
        k, r = rows[ki.long()], rel[ri.long()]
        _FOLD[key] = (rows, ki, rel, ri, tail, dq, SP.fold_torch(k, r, tail), SP.fold_adjoint_torch(k, r, tail, dq))
    return _FOLD[key]


@pytest.mark.parametrize("P,W", FOLD_CASES)
def test_fold_forward_bit_equal(P, W, hip_backend):
    rows, ki, rel, ri, tail, _, want, _ = _fold_inputs(P, W)
    dev = [x.to(DEV) for x in (rows, ki, rel, ri, tail)]
    buf = torch.full((2 * P, W), float("nan"), dtype=torch.float32, device=DEV)
    buf[P:] = -77.0
    rc = hip_backend.lib.temp_bilinear_query_fwd(P, W, KIND, _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), _p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[P:] == -77.0).all()), "canary"
    out = buf[:P].cpu()
    assert not bool(torch.isnan(out).any()), "every element is written"
    assert torch.equal(out, want)
    assert torch.equal(hip_backend.bilinear_query_fwd("simple", *dev).cpu(), want), "the backend method is the same launch"


@pytest.mark.parametrize("P,W", FOLD_CASES)
def test_fold_backward_bit_equal(P, W, hip_backend):
    rows, ki, rel, ri, tail, dq, _, (want_k, want_r) = _fold_inputs(P, W)
    dev = [x.to(DEV) for x in (rows, ki, rel, ri, tail, dq)]
    bufs = []
    for _ in range(2):
        b = torch.full((2 * P, W), float("nan"), dtype=torch.float32, device=DEV)
        b[P:] = -77.0
        bufs.append(b)
    rc = hip_backend.lib.temp_bilinear_query_bwd(P, W, KIND, _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), _p(dev[5]),
                                                 _p(bufs[0]), _p(bufs[1]), None)
    torch.cuda.synchronize()
    assert rc == 0
    for b, want, what in zip(bufs, (want_k, want_r), ("d_known_rows", "d_rel_rows")):
        assert bool((b[P:] == -77.0).all()), what + ": canary"
        got = b[:P].cpu()
        assert not bool(torch.isnan(got).any()), what + ": every element is written"
        assert torch.equal(got, want), what
    for got, want in zip(hip_backend.bilinear_query_bwd("simple", *dev), (want_k, want_r)):
        assert torch.equal(got.cpu(), want)


def test_fold_argument_checks(hip_backend):
    """W = 12 (halves that are no whole float4s) -> TEMP_E_UNSUPPORTED; no is_tail -> TEMP_E_BADARG; the gated query refuses the
    kind; nothing is written."""
    lib = hip_backend.lib
    x = torch.ones(64, 24, device=DEV)
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    w = torch.full((8,), 0.5, device=DEV)
    out, out2 = torch.full((8, 24), 5.0, device=DEV), torch.full((8, 24), 5.0, device=DEV)
    assert lib.temp_bilinear_query_fwd(8, 12, KIND, _p(x), _p(idx), _p(x), _p(idx), _p(idx), _p(out), None) == E_UNSUPPORTED
    assert lib.temp_bilinear_query_bwd(8, 12, KIND, _p(x), _p(idx), _p(x), _p(idx), _p(idx), _p(x), _p(out), _p(out2), None) == E_UNSUPPORTED
    assert lib.temp_bilinear_query_fwd(8, 16, KIND, _p(x), _p(idx), _p(x), _p(idx), None, _p(out), None) == E_BADARG
    assert lib.temp_bilinear_query_bwd(8, 16, KIND, _p(x), _p(idx), _p(x), _p(idx), None, _p(x), _p(out), _p(out2), None) == E_BADARG
    assert lib.temp_bilinear_query_fwd(8, 16, KIND + 1, _p(x), _p(idx), _p(x), _p(idx), _p(idx), _p(out), None) == E_BADARG
    assert lib.temp_gated_query_fwd(8, 16, KIND, _p(x), _p(idx), _p(x), _p(idx), _p(w), _p(x), _p(idx), _p(idx), _p(out), None) == E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((out2 == 5.0).all())


_PAIR = {}


def _pair_inputs(B, N, d):
    key = (B, N, d)
    if key not in _PAIR:
        rng = np.random.default_rng(1000 * B + 10 * N + d)
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        a, a_inv, d_out = f(N, d), f(N, d), f(B * N, 2 * d)
        _PAIR[key] = (a, a_inv, d_out, SP.pair_torch(a, a_inv, B).contiguous(), SP.pair_adjoint_loop(d_out, B))
    return _PAIR[key]


@pytest.mark.parametrize("B,N,d", PAIR_CASES)
def test_pair_forward_bit_equal(B, N, d, hip_backend):
    a, a_inv, _, want, _ = _pair_inputs(B, N, d)
    ad, bd = a.to(DEV), a_inv.to(DEV)
    buf = torch.full((2 * B * N, 2 * d), float("nan"), dtype=torch.float32, device=DEV)
    buf[B * N:] = -77.0
    rc = hip_backend.lib.temp_pair_rows_fwd(B, N, d, _p(ad), _p(bd), _p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[B * N:] == -77.0).all()), "canary"
    assert torch.equal(buf[:B * N].cpu(), want)
    assert torch.equal(hip_backend.pair_rows_fwd(ad, bd, B).cpu(), want), "the backend method is the same launch"


@pytest.mark.parametrize("B,N,d", PAIR_CASES)
def test_pair_backward_bit_equal(B, N, d, hip_backend):
    """Both outputs bit-equal to the ascending-b fp32 loop; NaN-prefilled outputs are fully overwritten, the canary floats behind
    them stay; a second call gives the same bits."""
    _, _, d_out, _, want = _pair_inputs(B, N, d)
    gd = d_out.to(DEV)
    runs = []
    for _ in range(2):
        bufs = []
        for _ in range(2):
            b = torch.full((2 * N, d), float("nan"), dtype=torch.float32, device=DEV)
            b[N:] = -77.0
            bufs.append(b)
        rc = hip_backend.lib.temp_pair_rows_bwd(B, N, d, _p(gd), _p(bufs[0]), _p(bufs[1]), None)
        torch.cuda.synchronize()
        assert rc == 0
        assert all(bool((b[N:] == -77.0).all()) for b in bufs), "canary"
        runs.append([b[:N].cpu() for b in bufs])
    for first, again, w, what in zip(runs[0], runs[1], want, ("d_a", "d_a_inv")):
        assert not bool(torch.isnan(first).any()), what + ": every element is written"
        assert torch.equal(first, w), what
        assert torch.equal(first, again), what + ": repeatable"
    for got, w in zip(hip_backend.pair_rows_bwd(gd, B), want):
        assert torch.equal(got.cpu(), w)


def test_pair_bad_arguments_launch_nothing(hip_backend):
    lib = hip_backend.lib
    x = torch.zeros(256, device=DEV)
    out, out2 = torch.full((256,), 5.0, device=DEV), torch.full((256,), 5.0, device=DEV)
    for B, N, d in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4), (2, -3, 4), (2, 4, -4)):
        assert lib.temp_pair_rows_fwd(B, N, d, _p(x), _p(x), _p(out), None) == E_BADARG
        assert lib.temp_pair_rows_bwd(B, N, d, _p(x), _p(out), _p(out2), None) == E_BADARG
    assert lib.temp_pair_rows_fwd(2, 4, 4, None, _p(x), _p(out), None) == E_BADARG
    assert lib.temp_pair_rows_fwd(2, 4, 4, _p(x), None, _p(out), None) == E_BADARG
    assert lib.temp_pair_rows_fwd(2, 4, 4, _p(x), _p(x), None, None) == E_BADARG
    assert lib.temp_pair_rows_bwd(2, 4, 4, None, _p(out), _p(out2), None) == E_BADARG
    assert lib.temp_pair_rows_bwd(2, 4, 4, _p(x), None, _p(out2), None) == E_BADARG
    assert lib.temp_pair_rows_bwd(2, 4, 4, _p(x), _p(out), None, None) == E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((out2 == 5.0).all())
    with pytest.raises(_lib.TempAmdError):
        hip_backend.pair_rows_fwd(x[:64].view(16, 4), x[:80].view(16, 5), 2)
    with pytest.raises(_lib.TempAmdError):
        hip_backend.pair_rows_bwd(x[:120].view(15, 8), 2)


def test_pair_kernels_are_traced_by_name(hip_backend):
    lib = hip_backend.lib
    a, a_inv, d_out, _, _ = _pair_inputs(3, 37, 6)
    ad, bd, gd = a.to(DEV), a_inv.to(DEV), d_out.to(DEV)
    ids, ms, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)(), ctypes.c_int32()
    _lib.check(lib.temp_trace_begin(16), "temp_trace_begin")
    try:
        hip_backend.pair_rows_bwd(gd, 3)
        hip_backend.pair_rows_fwd(ad, bd, 3)
        hip_backend.pair_rows_fwd(ad, bd, 1)
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 16, ctypes.byref(cnt)), "temp_trace_end")
    assert [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)] == ["k_pair_rows_bwd", "k_pair_rows_fwd", "k_pair_rows_fwd"]


def test_node_equals_torch_composition():
    SP.check_node(DEV)


def test_scorers_agree():
    SP.check_scorer(DEV)


def test_state_dict_is_the_references():
    SP.check_state_dict(DEV)


def test_initial_parameters_are_the_references():
    SP.check_initial_parameters(DEV)


def test_g28_loss_gradients():
    SP.check_g28(DEV)


def test_g29_evaluate():
    SP.check_g29(DEV)


@pytest.mark.parametrize("n_times", [3, 1])
def test_fused_route_equals_per_graph(n_times):
    z = SP.load("G28_simple")
    t_list = torch.tensor([int(t) for t in z["t_list"]][:n_times])
    assert SP.check_fused_equals_per_graph(DEV, t_list), "one pair launch each way per table, whatever B is"


def test_prepared_batch_is_repeatable():
    SP.check_prepared_repeatable(DEV)


def test_batch_with_an_empty_graph():
    SP.check_empty_graph_batch(DEV)


def test_width_outside_the_alignment_takes_the_literal_route():
    SP.check_literal_width(DEV)


def test_predict():
    SP.check_predict(DEV)


def test_state_dict_round_trip():
    SP.check_state_dict_round_trip(DEV)
