"""--module BiRRGCN's union pair pass on the MI355X: temp_lin_rows2_fwd / _bwd through functional.lin_step_rows2 against the float64
loop of tests/bi_pair_cases.py (d in 20, 32, 200, 256; n in 1, 31, 33, 97: partial tiles; row lists mixing forward-only, backward-only,
both and neither; x_rows None and an index with a -1 and a repeat; act 0 and 1, the reference taking the mask of the code under test;
one direction's H None), one kernel each way per node call in the library's trace, bit-repeatability, the composition with the
kernel switch off, the C entry points' return contract; BiDynamicRGCN.bi_pair_pass on against off -- loss, gradients, the float64
oracle's loss, all_embeds_batched against get_all_embeds_Gt, the dropout layout, windows of length 1 -- and the backend calls of a
training step.  Runs on poisoned allocations: an element of out, hdec_f, hdec_b, d_pre, d_hrows_f, d_hrows_b or a gradient that no
kernel writes is a NaN here.

Bars: tests/lin_chain_cases.py's -- STATE_BAR (rtol 1e-5 / atol 2e-6 . max(1, max |ref|)) for out, GRAD_BAR (1e-4 / 2e-5 . max(1,
max |ref|)) for d_x, d_Hf, d_Hb, d_Wf, d_Wb; the model's loss 1e-6 relative, its gradients tests/test_gpu_lin_stack.py's (1e-4 / 3e-6 .
max(1, max |ref|)).  Every case prints its figure before it asserts (pytest -s).
Measured on the MI355X (max err / bar, largest over n, act and x_rows):
  d = 20   out 0.054  d_x 0.00075  d_Hf 0.0045  d_Hb 0.0054  d_Wf 0.0037  d_Wb 0.0023
  d = 32   out 0.046  d_x 0.0012   d_Hf 0.0049  d_Hb 0.0062  d_Wf 0.0049  d_Wb 0.0039
  d = 200  out 0.15   d_x 0.0010   d_Hf 0.018   d_Hb 0.0094  d_Wf 0.0046  d_Wb 0.0045
  d = 256  out 0.22   d_x 0.0011   d_Hf 0.013   d_Hb 0.014   d_Wf 0.0048  d_Wb 0.0045
One direction's H None (d = 32, 200): out 0.085, gradients 0.0061.  Composition route at n = 97: out 0.15 (d = 200), gradients 0.013.
Model (D = 32, ICEWS14 slice): loss 24.35783005 with the attribute on, 24.35783386 off and in the float64 oracle (1.6e-7 relative);
gradients on against off at most 0.00097 of the bar; all_embeds_batched against get_all_embeds_Gt 0.016 of the state bar (0.036 on
(window, entity) rows); the union map holds 515 forward-only, 363 backward-only and 100 two-sided pairs; windows of length 1: the
bit-same loss, gradients 0.000075 of the bar; backend calls of a step 41 against 133.
lin_step_rows2 with Hb = None against lin_step_rows (d = 20, 200; n = 33): out, d_x, d_Hf, d_Wf equal to the bit (max |difference| 0)."""
import ctypes
from collections import Counter

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import bi_pair_cases as C
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
from tests.test_gpu_row_loss_routes import _traced

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
KERNELS = ("k_lin_rows2_fwd", "k_lin_rows2_bwd")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("n", C.ROW_NS)
@pytest.mark.parametrize("d", C.WIDTHS)
def test_node_vs_fp64(d, n, act):
    assert TF.lin_rows2_usable(d)
    (_, names) = _traced(lambda: C.check_rows2_node(n, d, act, DEV))
    assert [names.count(k) for k in KERNELS] == [2, 2], names               # (with and without x_rows: one launch each way per node call)


@pytest.mark.parametrize("d", [32, 200])
def test_absent_direction(d):
    (_, names) = _traced(lambda: C.check_absent_direction(d, DEV))
    assert [names.count(k) for k in KERNELS] == [2, 2], names


@pytest.mark.parametrize("d", C.ONE_SOURCE_WIDTHS)
def test_one_source_equals_lin_step_rows(d):
    """The two instantiations of the one row step agree to the bit where they compute the same thing: lin_step_rows2 with Hb = None
    against lin_step_rows (n = 33, x_rows given, ReLU, about a quarter of the history rows -1) -- out, d_x, d_Hf, d_Wf under
    torch.equal, one launch of each kernel."""
    assert TF.lin_rows_usable(d) and TF.lin_rows2_usable(d)
    (_, names) = _traced(lambda: C.check_one_source(d, DEV, exact=True))
    assert [names.count(k) for k in KERNELS + ("k_lin_rows_fwd", "k_lin_rows_bwd")] == [1, 1, 1, 1], names


def test_every_buffer_written(hip_backend):
    """Straight through the backend on poisoned buffers: all six outputs finite everywhere, hdec and d_hrows of a direction exactly 0
    on the rows without a previous state in it."""
    be = hip_backend
    for d in C.WIDTHS:
        for n in C.ROW_NS:
            c = {k: (v.to(DEV) if v is not None else None) for k, v in C.rows2_inputs(n, d, True).items()}
            pf, pb = be.lin_chain_pack_multi([c["Wf"], c["Wb"]])
            out, hf, hb, d_pre, dhf, dhb = (torch.empty(n, d, device=DEV) for _ in range(6))
            assert bool(torch.isnan(out).all())
            be.lin_rows2_fwd(c["x"], c["x_rows"], c["Hf"], c["rows_f"], c["dt_f"], c["Hb"], c["rows_b"], c["dt_b"], C.LAM, pf, pb, 1, out, hf, hb)
            be.lin_rows2_bwd(out, c["up"], c["rows_f"], c["dt_f"], c["rows_b"], c["dt_b"], C.LAM, pf, pb, 1, d_pre, dhf, dhb)
            for t in (out, hf, hb, d_pre, dhf, dhb):
                assert bool(torch.isfinite(t).all())
            for rows, h, dh in ((c["rows_f"], hf, dhf), (c["rows_b"], hb, dhb)):
                assert bool((h[rows < 0] == 0).all()) and bool((dh[rows < 0] == 0).all())
                assert float(h.abs().max()) > 0 and float(dh.abs().max()) > 0


def test_bit_repeatable():
    c = C.rows2_inputs(97, 200, True)
    a, b = (C.run_rows2_node(c, 1, DEV) for _ in range(2))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("d", [32, 200])
def test_composition_route(d, act):
    """The kernel switch off: no lin_rows2 launch, the same bars against the float64 loop."""
    assert TF.lin_rows2_usable(d)
    with C.rows_kernel(False):
        assert not TF.lin_rows2_usable(d)
    (_, names) = _traced(lambda: C.check_rows2_node(97, d, act, DEV, kernel=False))
    assert not any(k in names for k in KERNELS), names


def test_entry_point_contract(hip_backend):
    """The documented order: BADARG (n < 0, act outside {0, 1}) before UNSUPPORTED (d = 6, 260) before n == 0 (TEMP_OK, no launch)
    before the NULL pointers (BADARG); one kernel name per entry point in the trace."""
    be, lib = hip_backend, _lib.load()
    d, n = 32, 33
    c = {k: (v.to(DEV) if v is not None else None) for k, v in C.rows2_inputs(n, d, True).items()}
    pf, pb = be.lin_chain_pack_multi([c["Wf"], c["Wb"]])
    half = pf.numel() // 2
    out, hf, hb, d_pre, dhf, dhb = (torch.zeros(n, d, device=DEV) for _ in range(6))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = TB._stream()
    null = dict.fromkeys(("x", "Hf", "Hb", "rows_f", "rows_b", "dt_f", "dt_b", "up"))

    def fwd(n=n, d=d, act=1, t=c, o=out):
        return lib.temp_lin_rows2_fwd(n, d, p(t["x"]), p(c["x_rows"]), p(t["Hf"]), p(t["rows_f"]), p(t["dt_f"]), p(t["Hb"]), p(t["rows_b"]), p(t["dt_b"]),
                                      C.LAM, p(pf[:half]), p(pb[:half]), act, p(o), p(hf), p(hb), st)

    def bwd(n=n, d=d, act=1, t=c, o=d_pre):
        return lib.temp_lin_rows2_bwd(n, d, p(out), p(t["up"]), p(t["rows_f"]), p(t["dt_f"]), p(t["rows_b"]), p(t["dt_b"]), C.LAM, p(pf[half:]),
                                      p(pb[half:]), act, p(o), p(dhf), p(dhb), st)

    rc, names = _traced(lambda: (fwd(), bwd()))
    assert rc == (0, 0) and names == list(KERNELS), (rc, names)
    for bad in (dict(n=-1, d=6), dict(act=2, d=260), dict(d=0), dict(n=-1, t=null)):
        rc, names = _traced(lambda: (fwd(**bad), bwd(**bad)))
        assert rc == (1, 1) and names == [], (bad, rc)                      # TEMP_E_BADARG, before the width is looked at
    for bad in (6, 260):
        rc, names = _traced(lambda: (fwd(n=0, d=bad, t=null), bwd(n=0, d=bad, t=null)))
        assert rc == (2, 2) and names == [], (bad, rc)                      # TEMP_E_UNSUPPORTED, before n == 0
    rc, names = _traced(lambda: (fwd(n=0, t=null, o=None), bwd(n=0, t=null, o=None)))
    assert rc == (0, 0) and names == []                                     # n == 0 before the pointers
    for key in ("Hf", "rows_b", "dt_f"):
        rc, names = _traced(lambda: (fwd(t=dict(c, **{key: None})),))
        assert rc == (1,) and names == [], key
    for key in ("up", "rows_f", "dt_b"):
        rc, names = _traced(lambda: (bwd(t=dict(c, **{key: None})),))
        assert rc == (1,) and names == [], key
    rc, names = _traced(lambda: (fwd(o=None), bwd(o=None)))
    assert rc == (1, 1) and names == []
    assert not lib.temp_lin_rows2_supported(6) and not lib.temp_lin_rows2_supported(260) and lib.temp_lin_rows2_supported(256)


def test_on_vs_off_and_oracle_loss():
    C.check_on_vs_off(DEV)


@pytest.mark.parametrize("force_rep", [False, True])
def test_all_embeds_batched_vs_per_window(force_rep):
    C.check_all_embeds(DEV, force_rep)


def test_dropout_keeps_windows_apart():
    C.check_dropout(DEV)


def test_windows_of_length_one():
    C.check_on_vs_off(DEV, L=1, oracle=False)


def test_step_calls():
    """Attribute on: the centre and the pair rows one lin_rows2 launch each way, the history one chain launch each way, one fused
    loss node, no decay_rows.  Attribute off: the list of the model without the attribute."""
    calls, L, B = C.step_calls(DEV, True)
    n = Counter(calls)
    assert n["lin_rows2_fwd"] == 2 and n["lin_rows2_bwd"] == 2 and n["lin_chain_fwd"] == 1 and n["lin_chain_bwd"] == 1, n
    assert n["gather_ce_fwd"] == 1 and n["decay_rows"] == 0, n
    off, _, _ = C.step_calls(DEV, False)
    deleted, _, _ = C.step_calls(DEV, "deleted")
    assert off == deleted and Counter(off)["gather_ce_fwd"] == B and Counter(off)["lin_rows2_fwd"] == 0
    print("backend calls of the step: attribute on %d, off %d" % (len(calls), len(off)))
