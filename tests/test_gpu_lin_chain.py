"""The linear window chain on the MI355X: temp_lin_chain_fwd / _bwd (one launch each for ALL positions of --module RRGCN / BiRRGCN)
through lin_chain.linear_chain against the float64 autograd loop of tests/lin_chain_cases.py; identities (bit-repeatability, W = 0, the
torch route); the entry-point conditions; the window models against their other routes and the float64 oracle; the backend calls of
a training step.  Runs on poisoned allocations: an element of h, hdec, d_pre or a gradient that no kernel writes is a NaN here.

Bars: rtol 1e-5 / atol 2e-6 . max(1, max |ref|) for the states, rtol 1e-4 / atol 2e-5 . max(1, max |ref|) for d_x and d_W (the chain
suites' bars, tests/test_gpu_chain_time_embedding.py: the same accumulation lengths, fp32 accumulate).  Every case prints
max err / bar before it asserts (pytest -s).  Measured on the MI355X (max err / bar, largest over act and want):
  d = 20   states 0.054  d_x 0.0026  d_W 0.0053        d = 32   states 0.048  d_x 0.0048  d_W 0.0063
  d = 200  states 0.13   d_x 0.010   d_W 0.010         d = 220  states 0.15   d_x 0.010   d_W 0.014
  (max |ref|: states up to 3.4, d_x up to 58, d_W up to 173.)  Kernels against the torch route at d = 200: states equal to the bit,
  d_x 0.0036, d_W 0.0050.  Window models (D = 32, ICEWS14 slice): RRGCN loss 18.26619720 on the chain route and the per-position
  loop, 18.26619911 reference-granular, float64 oracle 18.26619898 (9.7e-8 relative); BiRRGCN 24.35783386 on all three routes,
  oracle within 2.9e-8.
"""
import ctypes
from collections import Counter

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import lin_chain as LC
from tests import lin_chain_cases as C
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
from tests.test_gpu_row_loss_routes import _traced

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _launches():
    return _lib.load().temp_lin_chain_launches()


@pytest.mark.parametrize("want_last", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("d", C.WIDTHS)
def test_kernels_vs_fp64_loop(d, act, want_last):
    c0 = _launches()
    C.check_node(d, act, want_last, DEV)
    assert _launches() - c0 == 2 + act              # forward + backward (+ the forward that reads the mask)


def test_bit_repeatable():
    prog, n_x = C.program()
    x, ws = C.inputs(n_x, 200, 2)
    a, b = (C.run_node(prog, x, ws, 1, None, DEV) for _ in range(2))
    for k in ("outs", "d_w"):
        assert all(torch.equal(p, q) for p, q in zip(a[k], b[k]))
    assert torch.equal(a["d_x"], b["d_x"])


@pytest.mark.parametrize("d", [32, 220])
def test_zero_weight_returns_x(d):
    prog, n_x = C.program()
    x, ws = C.inputs(n_x, d, 2)
    res = C.run_node(prog, x, [torch.zeros_like(w) for w in ws], 0, None, DEV)
    assert torch.equal(torch.cat(res["outs"]), x)


@pytest.mark.parametrize("act", [0, 1])
def test_torch_route_agrees(act):
    prog, n_x = C.program()
    x, ws = C.inputs(n_x, 200, 2)
    c0 = _launches()
    ref = C.run_node(prog, x, ws, act, None, DEV, kernels=False)
    assert _launches() == c0
    res = C.run_node(prog, x, ws, act, None, DEV)
    assert _launches() == c0 + 2
    C.check_against(res, {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in ref.items()}, "kernels vs torch route act = %d" % act)


def test_every_buffer_written(hip_backend):
    """h, hdec and d_pre straight from the backend calls, on poisoned buffers, `want` = the chains' last instances (the blocks
    without an upstream gradient included)."""
    be = hip_backend
    prog, n_x = C.program()
    d = 220
    x, ws = C.inputs(n_x, d, 2)
    want = C.last_instances(prog)
    tabs = prog.chain_tables(DEV, want)
    packs = be.lin_chain_pack_multi([w.to(DEV) for w in ws])
    h, hdec, d_pre = (torch.empty(prog.n_total, d, device=DEV) for _ in range(3))
    assert bool(torch.isnan(h).all())
    be.lin_chain_fwd(tabs, x.to(DEV), prog.x_index(DEV), C.LAM, packs, 1, h, hdec)
    ups = [torch.randn(prog.inst[i].n, d, device=DEV) for i in want]
    ups[0] = None
    be.lin_chain_bwd(tabs, h, ups, C.LAM, packs, 1, d_pre)
    for t in (h, hdec, d_pre):
        assert bool(torch.isfinite(t).all())
    assert float(hdec.abs().max()) > 0 and float(d_pre.abs().max()) > 0


def test_entry_point_conditions(hip_backend):
    """n_panels = 0 succeeds without a launch; d = 6 is TEMP_E_UNSUPPORTED; a NULL panel table TEMP_E_BADARG; one kernel name per entry
    point in the trace."""
    be, lib = hip_backend, _lib.load()
    prog, n_x = C.program()
    d = 32
    x, ws = C.inputs(n_x, d, 2)
    x = x.to(DEV)
    tabs = prog.chain_tables(DEV, None)
    h, hdec, d_pre = (torch.zeros(prog.n_total, d, device=DEV) for _ in range(3))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = TB._stream()
    up = (ctypes.c_void_p * 1)(h.data_ptr())

    def calls(c):
        return (lib.temp_lin_chain_fwd(ctypes.byref(c), p(x), None, p(h), p(hdec), st), lib.temp_lin_chain_bwd(ctypes.byref(c), p(h), 1, up, p(d_pre), st))

    def run():
        packs = be.lin_chain_pack_multi([w.to(DEV) for w in ws])
        c, keep = be._lin_desc(tabs, d, C.LAM, packs, 1)
        return packs, c, keep, calls(c)

    (packs, c, keep, rc), names = _traced(run)
    assert rc == (0, 0) and names == ["k_lin_chain_pack", "k_lin_chain_fwd", "k_lin_chain_bwd"], (rc, names)
    c.n_panels = 0
    rc, names = _traced(lambda: calls(c))
    assert rc == (0, 0) and names == []
    c.n_panels, c.d = tabs["n_panels"], 6
    rc, names = _traced(lambda: calls(c))
    assert rc == (2, 2) and names == []                                    # TEMP_E_UNSUPPORTED
    c.d, c.panel = d, None
    rc, names = _traced(lambda: calls(c))
    assert rc == (1, 1) and names == []                                    # TEMP_E_BADARG
    assert not lib.temp_lin_chain_supported(6, 8) and not lib.temp_lin_chain_supported(260, 8) and not lib.temp_lin_chain_supported(32, 65)
    assert lib.temp_lin_chain_supported(256, 64)


@pytest.mark.parametrize("module,golden", C.MODELS)
def test_window_models(module, golden):
    c0 = _launches()
    C.check_window_model(module, golden, DEV)
    assert _launches() > c0


def test_dropout_all_entity_pass_keeps_windows_apart_gpu():
    C.check_dropout_all_entity(DEV)


@pytest.mark.parametrize("module,golden", C.MODELS)
def test_step_calls(module, golden):
    """Chain route: exactly one lin_chain_fwd and one lin_chain_bwd; RRGCN then launches linear + decay_rows for the pairs of the
    batched all-entity pass alone (none per history position), BiRRGCN for the centre's two terms and its per-window all-entity pass
    (two per window).  use_lin_chain = False: the per-position list."""
    B = 4
    calls, L = C.step_calls(module, golden, DEV, True)
    n = Counter(calls)
    assert n["lin_chain_fwd"] == 1 and n["lin_chain_bwd"] == 1 and n["lin_chain_pack_multi"] == 1, n
    fwd = (2 + 2 * B) if module.startswith("Bi") else 1
    assert n["decay_rows"] == 2 * fwd, (n["decay_rows"], fwd)
    assert (n["gather_ce_fwd"] == 1) == (module == "RRGCN")
    calls, L = C.step_calls(module, golden, DEV, False)
    m = Counter(calls)
    assert m["lin_chain_fwd"] == 0 and m["lin_chain_bwd"] == 0 and m["lin_chain_pack_multi"] == 0
    per_position = 2 * (L - 2) if module.startswith("Bi") else L - 1          # history positions with a previous state (+ the uni target)
    assert m["decay_rows"] == 2 * (fwd + per_position), (m["decay_rows"], fwd, per_position)
    # (`linear` also serves the loss: the chain route saves exactly the per-position products, forward and d_x)
    assert m["linear"] - n["linear"] == 2 * per_position, (m["linear"], n["linear"])
    if module == "RRGCN":
        assert n["linear"] == 2 * fwd, n["linear"]
