"""One position of the linear recurrence on gathered rows on the MI355X: temp_lin_rows_fwd / _bwd through functional.lin_step_rows
against the float64 restatement of tests/lin_stack_cases.py (d in 20, 32, 200, 220; n in 1, 33, 70: partial panels; x_rows None and
an index with repeats; about a quarter of h_rows -1; act 0 and 1, the reference taking the mask of the code under test); straight
through the backend on poisoned buffers; identities (bit-repeatability, W = 0); the entry-point conditions; the node's composition
of the row operators against the kernel route.  Runs on poisoned allocations: an element of out, hdec, d_pre, d_hrows or a gradient
that no kernel writes is a NaN here.

Bars: tests/lin_chain_cases.py's, for this same product -- STATE_BAR (rtol 1e-5 / atol 2e-6 . max(1, max |ref|)) for out and hdec,
GRAD_BAR (1e-4 / 2e-5 . max(1, max |ref|)) for d_x, d_H and d_W.  Every case prints max err / bar before it asserts (pytest -s).
Measured on the MI355X (max err / bar, largest over n, act and x_rows):
  d = 20   out 0.031  hdec 0.0071  d_x 0.00076  d_H 0.0030  d_W 0.0047        d = 32   out 0.041  hdec 0.0074  d_x 0.00097  d_H 0.0047  d_W 0.0041
  d = 200  out 0.099  hdec 0.0080  d_x 0.0011   d_H 0.015   d_W 0.0042        d = 220  out 0.11   hdec 0.0071  d_x 0.0016   d_H 0.017   d_W 0.0053
Kernel against the composition at d = 200, n = 70: out 0.14, d_x 0 (the same segment sum of the same rows), d_H 0.011, d_W 0.0032."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import lin_stack_cases as C
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
from tests.test_gpu_row_loss_routes import _traced

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _backend_run(be, c, d, act):
    """Forward + backward straight through the backend -> (out, hdec, d_pre, d_hrows) on the device."""
    n = c["h_rows"].shape[0]
    t = {k: (v.to(DEV) if v is not None else None) for k, v in c.items()}
    pack = be.lin_chain_pack_multi([t["W"]])[0]
    out, hdec, d_pre, d_hrows = (torch.empty(n, d, device=DEV) for _ in range(4))
    assert bool(torch.isnan(out).all())
    be.lin_rows_fwd(t["x"], t["x_rows"], t["H"], t["h_rows"], t["dt"], C.LAM, pack, act, out, hdec)
    be.lin_rows_bwd(out, t["up"], t["h_rows"], t["dt"], C.LAM, pack, act, d_pre, d_hrows)
    return out, hdec, d_pre, d_hrows


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("n", C.ROW_NS)
@pytest.mark.parametrize("d", C.WIDTHS)
def test_node_vs_fp64(d, n, act):
    assert TF.lin_rows_usable(d)
    (_, names) = _traced(lambda: C.check_rows_node(n, d, act, DEV))
    assert names.count("k_lin_rows_fwd") == 2 and names.count("k_lin_rows_bwd") == 2, names        # (with and without x_rows)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("d", C.WIDTHS)
def test_every_buffer_written(hip_backend, d, act):
    """out, hdec, d_pre and d_hrows are finite everywhere on poisoned buffers; hdec against the restatement; the rows without a
    previous state have hdec and d_hrows exactly 0."""
    for n in C.ROW_NS:
        for with_x_rows in (False, True):
            c = C.rows_inputs(n, d, with_x_rows)
            out, hdec, d_pre, d_hrows = _backend_run(hip_backend, c, d, act)
            for t in (out, hdec, d_pre, d_hrows):
                assert bool(torch.isfinite(t).all())
            none = (c["h_rows"] < 0).to(DEV)
            assert bool((hdec[none] == 0).all()) and bool((d_hrows[none] == 0).all())
            assert float(hdec.abs().max()) > 0 and float(d_hrows.abs().max()) > 0
            ref = C.rows_reference(c, act, (out > 0).cpu() if act else None)
            C.check_quantities(dict(out=out.cpu(), hdec=hdec.cpu()), ref, "backend n = %d d = %d act = %d" % (n, d, act), names=("out", "hdec"))


def test_bit_repeatable():
    c = C.rows_inputs(70, 200, True)
    a, b = (C.run_rows_node(c, 1, DEV) for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("d", [32, 220])
def test_zero_weight_returns_x(d, act):
    c = C.rows_inputs(70, d, True)
    c["W"] = torch.zeros_like(c["W"])
    res = C.run_rows_node(c, act, DEV)
    want = c["x"][c["x_rows"].long()]
    assert torch.equal(res["out"], torch.relu(want) if act else want)


@pytest.mark.parametrize("act", [0, 1])
def test_composition_agrees(act):
    """The node's composition of the row operators (no lin_rows launch) against the kernel route, at the same bars."""
    c = C.rows_inputs(70, 200, True)
    ref, names = _traced(lambda: C.run_rows_node(c, act, DEV, kernel=False))
    assert "k_lin_rows_fwd" not in names and "k_lin_rows_bwd" not in names, names
    res = C.run_rows_node(c, act, DEV)
    C.check_quantities(res, {k: v.double() for k, v in ref.items()}, "kernel vs composition act = %d" % act)


def test_entry_point_conditions(hip_backend):
    """n = 0 succeeds without a launch; d = 6 and d = 260 are TEMP_E_UNSUPPORTED; a NULL H with n > 0 TEMP_E_BADARG; one kernel name
    per entry point in the trace."""
    be, lib = hip_backend, _lib.load()
    d, n = 32, 33
    c = {k: (v.to(DEV) if v is not None else None) for k, v in C.rows_inputs(n, d, True).items()}
    pack = be.lin_chain_pack_multi([c["W"]])[0]
    half = pack.numel() // 2
    out, hdec, d_pre, d_hrows = (torch.zeros(n, d, device=DEV) for _ in range(4))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = TB._stream()

    def fwd(n=n, d=d, H=c["H"]):
        return lib.temp_lin_rows_fwd(n, d, p(c["x"]), p(c["x_rows"]), p(H), p(c["h_rows"]), p(c["dt"]), C.LAM, p(pack[:half]), 1, p(out), p(hdec), st)

    def bwd(n=n, d=d, up=c["up"]):
        return lib.temp_lin_rows_bwd(n, d, p(out), p(up), p(c["h_rows"]), p(c["dt"]), C.LAM, p(pack[half:]), 1, p(d_pre), p(d_hrows), st)

    rc, names = _traced(lambda: (fwd(), bwd()))
    assert rc == (0, 0) and names == ["k_lin_rows_fwd", "k_lin_rows_bwd"], (rc, names)
    rc, names = _traced(lambda: (fwd(n=0), bwd(n=0)))
    assert rc == (0, 0) and names == []
    for bad in (6, 260):
        rc, names = _traced(lambda: (fwd(d=bad), bwd(d=bad)))
        assert rc == (2, 2) and names == [], (bad, rc)                      # TEMP_E_UNSUPPORTED
    rc, names = _traced(lambda: (fwd(H=None), bwd(up=None)))
    assert rc == (1, 1) and names == []                                     # TEMP_E_BADARG
    assert not lib.temp_lin_rows_supported(6) and not lib.temp_lin_rows_supported(260) and lib.temp_lin_rows_supported(256)
