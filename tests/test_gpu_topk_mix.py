"""temp_filtered_topk_mix on the GPU (tests/topk_mix_cases.py): the kernel against mixed_scores + topk_composite bit for bit on
tie-rich operands -- -inf in either operand under weights 0 and 1, every filter variant, keep, padding, carried panels in any
order and of mixed provenance, repeatability, the identity weights, refused arguments, the trace name; the two mixed filters'
topk_single_graph and predict_gated through the kernel."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import topk_mix_cases as MC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def dv(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("N", MC.N_VALUES)
@pytest.mark.parametrize("k", MC.K_VALUES)
def test_kernel_equals_composite_bit_exact(k, N):
    MC.check_selection(TB.get_backend().filtered_topk_mix, dv, k, N)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffled"])
@pytest.mark.parametrize("width", [64, 1000])
def test_carried_panels_equal_one_call(width, order):
    be = TB.get_backend()
    MC.check_panels(be.filtered_topk_mix, be.filtered_topk, dv, width, order)


def test_carried_panels_of_mixed_provenance():
    """Panels alternate between the mix entry point and the plain entry point fed the torch-mixed slice."""
    be = TB.get_backend()
    MC.check_panels(be.filtered_topk_mix, be.filtered_topk, dv, 1000, "shuffled", alternate=True)


def test_identity_weights_equal_the_plain_entry_point():
    be = TB.get_backend()
    MC.check_identity(be.filtered_topk_mix, be.filtered_topk, dv)


def test_arguments():
    """Mismatched shapes, a misaligned b, k = 0, k = 257 and a missing w are refused by the wrapper and by the C entry point;
    P = 0 succeeds."""
    be = TB.get_backend()
    a, b, w = torch.zeros(3, 8, device=DEV), torch.zeros(3, 8, device=DEV), torch.full((3,), 0.5, device=DEV)
    odd = torch.zeros(3 * 8 + 4, device=DEV)[1:25].view(3, 8)          # the shape and strides of a, four bytes off
    assert odd.data_ptr() % 16 == 4
    for k in (0, _lib.TOPK_MAX + 1):
        with pytest.raises(ValueError):
            be.filtered_topk_mix(a, b, w, k)
    for bad_b in (torch.zeros(3, 12, device=DEV), torch.zeros(2, 8, device=DEV), torch.zeros(3, 16, device=DEV)[:, :8], odd):
        with pytest.raises(ValueError):
            be.filtered_topk_mix(a, bad_b, w, 2)
    for bad_w in (None, w[:2]):
        with pytest.raises(ValueError):
            be.filtered_topk_mix(a, b, bad_w, 2)
    with pytest.raises(ValueError):
        be.filtered_topk_mix(torch.zeros(3, 6, device=DEV), torch.zeros(3, 6, device=DEV), w, 2)
    val, idx = be.filtered_topk_mix(torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV), torch.zeros(0, device=DEV), 4)
    assert tuple(val.shape) == tuple(idx.shape) == (0, 4)
    lib = _lib.load()
    tv, ti = torch.empty(3, 4, device=DEV), torch.empty(3, 4, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None

    def call(P, N, ld, k, col0=0, off_b=0, pa=a, pb=b, pw=w):
        return lib.temp_filtered_topk_mix(P, N, ld, k, col0, p(pa), p(pb, off_b) if pb is not None else None, p(pw), None, None, None, 0,
                                          p(tv), p(ti), TB._stream())

    assert call(3, 8, 8, 4) == 0
    # (a [P, 8] against b [P, 12] cannot be said through one ld: the C entry point refuses what it can see of a mismatch -- an ld
    # below N, an ld that is no multiple of 4, a b that is not aligned like a)
    for bad in (call(3, 8, 8, 0), call(3, 8, 8, _lib.TOPK_MAX + 1), call(3, 6, 6, 4), call(3, 4, 8, 4, off_b=4), call(3, 8, 4, 4),
                call(3, 8, 8, 4, col0=-1), call(-1, 8, 8, 4), call(3, 8, 8, 4, pw=None), call(3, 8, 8, 4, pb=None), call(3, 8, 8, 4, pa=None)):
        assert bad != 0
    assert lib.temp_filtered_topk_mix(0, 8, 8, 4, 0, None, None, None, None, None, None, 0, None, None, TB._stream()) == 0
    torch.cuda.synchronize()


def test_launch_is_traced_under_its_name():
    """One k_filtered_topk_mix record per call; the plain entry point keeps k_filtered_topk."""
    lib = _lib.load()
    be = TB.get_backend()
    a, b, w, _ = MC.mix_inputs(5, 1024)
    a, b, w = dv(a), dv(b), dv(w)
    be.filtered_topk_mix(a, b, w, 10, n=1024)
    torch.cuda.synchronize()
    ids, ms, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(16), "temp_trace_begin")
    try:
        be.filtered_topk_mix(a, b, w, 10, n=1024)
        be.filtered_topk(a, 10, n=1024)
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 16, ctypes.byref(cnt)), "temp_trace_end")
    assert [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)] == ["k_filtered_topk_mix", "k_filtered_topk"]


@pytest.mark.parametrize("panel", [None, 64])
@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("mode", ["tail", "head"])
@pytest.mark.parametrize("N", [204, 203])
@pytest.mark.parametrize("name", ["distmult", "complex", "transE"])
@pytest.mark.parametrize("family", ["ensemble", "aggregation"])
def test_evaluater_exact_on_integer_tables(family, name, N, mode, filtered, panel):
    MC.check_evaluater(DEV, family, name, N, 8, mode, filtered, panel)


@pytest.mark.parametrize("kind", MC.MODELS)
def test_predict_gated_against_fp64_tables(kind):
    MC.check_predict_gated(kind, DEV)


def test_predict_gated_distmult():
    MC.check_predict_gated("PostEnsembleGRRGCN", DEV, "distmult")


@pytest.mark.parametrize("kind", MC.MODELS)
def test_weight_extremes_are_the_single_tables(kind):
    MC.check_weight_extremes(kind, DEV)


@pytest.mark.parametrize("kind", MC.MODELS)
def test_own_gates_state_dict_and_predict_refusal(kind):
    MC.check_own_gates(kind, DEV)
