"""The clipped-Adam kernels (temp_grad_norm_clip / temp_adam_clip_step) and temp_amd.optim.ClippedAdam on the MI355X: the HIP route
on the cases of tests/clipped_adam_cases.py against the fp64 contract, inside the band measured from clip_grad_norm_ +
Adam(fused=True) on the same device; repeatability; the launches a step makes; the argument checks; one slice model."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd.optim import ClippedAdam
from tests import clipped_adam_cases as AC
from tests.golden_util import load
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG, E_WORKSPACE = 1, 3


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


_STD = {}


def _standard():
    """The standard set: inputs, fp64 contract, the kernel run and the torch fused run, computed once."""
    if not _STD:
        inp = AC.standard_inputs()
        groups = AC.one_group(inp)
        _STD.update(inp=inp, groups=groups, want=AC.contract_fp64(inp, groups, AC.MAX_NORM))
        params, opt, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
        _STD.update(ours=AC.moments(params, opt), params=params, opt=opt, seen=[(n.cpu(), c.cpu()) for n, c in seen])
        rp, ro = AC.run_torch(inp, groups, AC.MAX_NORM, DEV, fused=True)
        _STD.update(ref=AC.moments(rp, ro))
    return _STD


def _traced(fn, cap=32):
    lib = TB.get_backend().lib
    ids, ms, cnt = (ctypes.c_int32 * cap)(), (ctypes.c_float * cap)(), ctypes.c_int32()
    _lib.check(lib.temp_trace_begin(cap), "temp_trace_begin")
    try:
        fn()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, cap, ctypes.byref(cnt)), "temp_trace_end")
    return [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)]


def test_a_step_is_at_most_three_launches_of_the_library():
    inp = AC.standard_inputs(steps=1)
    for max_norm, want in ((AC.MAX_NORM, ["k_adam_grad_norm", "k_adam_norm_finish", "k_adam_clip_step"]), (None, ["k_adam_clip_step"])):
        params = AC.build_params(inp, DEV)
        assert params[inp.view[0]].data_ptr() % 16 == 4, "the view parameter starts 4 bytes into its buffer"
        opt = ClippedAdam(params, lr=AC.LR, weight_decay=AC.WD, max_norm=max_norm)
        AC.set_grads(params, inp, 0, DEV)
        assert _traced(opt.step) == want
        opt.use_kernel = False
        AC.set_grads(params, inp, 0, DEV)
        assert _traced(opt.step) == []


def test_kernel_route_inside_the_band():
    s = _standard()
    assert min(s["want"][4]) > 100.0
    AC.check_band(s["ours"], s["ref"], s["want"][:3], "hip route")
    none = len(s["inp"]) - 1
    assert s["params"][none] not in s["opt"].state and torch.equal(s["params"][none].detach().cpu(), s["inp"].values[none])


def test_norm_and_coefficient_within_one_ulp():
    s = _standard()
    for (norm, coef), n64, c64 in zip(s["seen"], s["want"][4], s["want"][5]):
        print("norm %.9g (fp64 %.17g)  coef %.9g (fp64 %.17g)" % (float(norm), n64, float(coef), c64))
        assert AC.ulps_apart(norm, n64) <= 1 and AC.ulps_apart(coef, c64) <= 1


def _same(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert (u is None and v is None) or torch.equal(u, v)


def test_two_runs_are_bit_identical():
    s = _standard()
    params, opt, seen = AC.run_ours(s["inp"], s["groups"], AC.MAX_NORM, DEV)
    _same(AC.moments(params, opt), s["ours"])
    for (n0, c0), (n1, c1) in zip(s["seen"], seen):
        assert torch.equal(n0, n1.cpu()) and torch.equal(c0, c1.cpu())


def test_alignment_does_not_change_the_result():
    """The same values in 16-byte aligned tensors: the float4 route, bit-equal to the scalar route of the view."""
    s = _standard()
    aligned = AC.Inputs(s["inp"].values, s["inp"].grads, view=())
    params, opt, seen = AC.run_ours(aligned, s["groups"], AC.MAX_NORM, DEV)
    assert all(p.data_ptr() % 16 == 0 for p in params)
    _same(AC.moments(params, opt), s["ours"])
    assert all(torch.equal(a[0], b[0].cpu()) for a, b in zip(s["seen"], seen))


def test_under_the_threshold_the_coefficient_is_one_and_nothing_changes():
    inp = AC.standard_inputs(grad_scale=1e-3)
    groups = AC.one_group(inp)
    assert max(AC.contract_fp64(inp, groups, AC.MAX_NORM)[4]) < 1.0
    a, oa, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    b, ob, _ = AC.run_ours(inp, groups, None, DEV)
    assert all(float(c) == 1.0 for _, c in seen) and ob.last_clip_coef is None
    _same(AC.moments(a, oa), AC.moments(b, ob))


def test_many_rows_and_a_long_tensor():
    """Seventy tensors of 1 to 300 elements and one of 3 C + 1 in the middle: the chunk search across many table rows."""
    g = torch.Generator().manual_seed(11)
    counts = [int(x) for x in torch.randint(1, 301, (70,), generator=g)]
    counts[0], counts[1] = 1, 300
    counts.insert(35, 3 * _lib.ADAM_CHUNK + 1)
    inp = AC.make_inputs(counts, steps=3, seed=12)
    groups = AC.one_group(inp)
    ours, opt, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    ref, ropt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV, fused=True)
    want = AC.contract_fp64(inp, groups, AC.MAX_NORM)
    AC.check_band(AC.moments(ours, opt), AC.moments(ref, ropt), want[:3], "71 rows")
    for (norm, coef), n64, c64 in zip(seen, want[4], want[5]):
        assert AC.ulps_apart(norm.cpu(), n64) <= 1 and AC.ulps_apart(coef.cpu(), c64) <= 1


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_nonfinite_gradients_follow_the_arithmetic(kind):
    AC.check_nonfinite(kind, DEV, fused=True)


def test_two_groups_share_one_global_norm():
    inp = AC.standard_inputs(seed=4)
    n = len(inp)
    groups = [(list(range(0, n, 2)), 1e-3, 1e-4), (list(range(1, n, 2)), 3e-3, 0.0)]
    ours, opt, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    ref, ropt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV, fused=True)
    want = AC.contract_fp64(inp, groups, AC.MAX_NORM)
    AC.check_band(AC.moments(ours, opt), AC.moments(ref, ropt), want[:3], "two groups")
    assert all(AC.ulps_apart(norm.cpu(), n64) <= 1 for (norm, _), n64 in zip(seen, want[4]))


def test_composite_route_on_the_device_inside_the_band():
    s = _standard()
    params, opt, seen = AC.run_ours(s["inp"], s["groups"], AC.MAX_NORM, DEV, use_kernel=False)
    AC.check_band(AC.moments(params, opt), s["ref"], s["want"][:3], "composite on the device")
    for (n1, c1), n64, c64 in zip(seen, s["want"][4], s["want"][5]):
        assert AC.ulps_apart(n1.cpu(), n64) <= 1 and AC.ulps_apart(c1.cpu(), c64) <= 1


def test_strided_gradient_takes_the_composite():
    p = torch.nn.Parameter(torch.ones(6, 4, device=DEV))
    opt = ClippedAdam([p], max_norm=1.0)
    p.grad = torch.ones(4, 6, device=DEV).t()
    assert _traced(opt.step) == []
    p.grad = torch.ones(6, 4, device=DEV)
    assert _traced(opt.step) == ["k_adam_grad_norm", "k_adam_norm_finish", "k_adam_clip_step"]
    assert opt.state[p]["step"] == 2


def test_bigrrgcn_slice_model_on_both_routes():
    from tests.window_cases import build_window_model, window_inputs
    z = load("G10_bi_grrgcn_rol")
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    for use_kernel in (True, False):
        m = build_window_model(z, DEV)
        before = {k: (v.shape, v.dtype, v.data_ptr()) for k, v in m.state_dict().items()}
        worst, opt = AC.check_model_band(m, lambda: m(t_list, target_edge_ids=edge_ids, samples=samples), DEV, True, 2,
                                         "BiGRRGCN kernel=%s" % use_kernel, use_kernel=use_kernel)
        after = {k: (v.shape, v.dtype, v.data_ptr()) for k, v in m.state_dict().items()}
        assert after == before, "same keys, shapes and storage: the step only changes parameter values"
        assert all(bool(torch.isfinite(v).all()) for v in m.state_dict().values())
        assert 0.0 < float(opt.last_clip_coef) <= 1.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_refused_arguments_launch_nothing(hip_backend):
    lib = hip_backend.lib
    p, g = torch.full((8,), 5.0, device=DEV), torch.ones(8, device=DEV)
    m, v = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    row = _lib.TempAdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 8, 1e-3, 1.0, 0.1, 0.999, 0.001, 1e-8, 0.0, 0)
    table = torch.frombuffer(bytearray(bytes(row)), dtype=torch.uint8).to(DEV)
    out = torch.full((2,), -3.0, device=DEV)
    ws = torch.zeros(lib.temp_grad_norm_workspace(1), dtype=torch.uint8, device=DEV)
    assert lib.temp_grad_norm_workspace(1) >= 8 and lib.temp_grad_norm_workspace(-5) == lib.temp_grad_norm_workspace(0)
    names = _traced(lambda: [
        lib.temp_grad_norm_clip(-1, 1, _p(table), 1.0, _p(ws), ws.numel(), _p(out), None),
        lib.temp_grad_norm_clip(1, -1, _p(table), 1.0, _p(ws), ws.numel(), _p(out), None),
        lib.temp_grad_norm_clip(1, 1, None, 1.0, _p(ws), ws.numel(), _p(out), None),
        lib.temp_grad_norm_clip(0, 1, _p(table), 1.0, _p(ws), ws.numel(), _p(out), None),
        lib.temp_grad_norm_clip(1, 1, _p(table), 1.0, _p(ws), ws.numel(), None, None),
        lib.temp_adam_clip_step(-1, 1, _p(table), None, None),
        lib.temp_adam_clip_step(1, -1, _p(table), None, None),
        lib.temp_adam_clip_step(1, 1, None, None, None),
        lib.temp_adam_clip_step(0, 1, _p(table), None, None)])
    assert names == []
    assert lib.temp_grad_norm_clip(-1, 1, _p(table), 1.0, _p(ws), ws.numel(), _p(out), None) == E_BADARG
    assert lib.temp_grad_norm_clip(1, -1, _p(table), 1.0, _p(ws), ws.numel(), _p(out), None) == E_BADARG
    assert lib.temp_grad_norm_clip(1, 1, None, 1.0, _p(ws), ws.numel(), _p(out), None) == E_BADARG
    assert lib.temp_grad_norm_clip(1, 1, _p(table), 1.0, _p(ws), ws.numel(), None, None) == E_BADARG
    assert lib.temp_grad_norm_clip(1, 1, _p(table), 1.0, None, 0, _p(out), None) == E_WORKSPACE
    assert lib.temp_grad_norm_clip(1, 1, _p(table), 1.0, _p(ws), 4, _p(out), None) == E_WORKSPACE
    assert lib.temp_adam_clip_step(-1, 1, _p(table), None, None) == E_BADARG
    assert lib.temp_adam_clip_step(1, -1, _p(table), None, None) == E_BADARG
    assert lib.temp_adam_clip_step(1, 1, None, None, None) == E_BADARG
    assert lib.temp_adam_clip_step(0, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((p == 5.0).all()) and bool((out == -3.0).all()) and bool((m == 0).all())
    with pytest.raises(ValueError):
        hip_backend.adam_clip_step(table, 2, 1)                          # a table shorter than its row count
    with pytest.raises(_lib.TempAmdError):
        hip_backend.adam_clip_step(table.cpu(), 1, 1)
    with pytest.raises(ValueError):
        hip_backend.grad_norm_clip(table, 1, 1, 0.0, ws, out)
    with pytest.raises(ValueError):
        hip_backend.grad_norm_clip(table, 1, 1, 1.0, ws[:4], out)
    # and the accepted call does what the table says: one plain Adam step of 8 elements, norm sqrt(8)
    hip_backend.grad_norm_clip(table, 1, 1, 1.0, ws, out)
    hip_backend.adam_clip_step(table, 1, 1, out)
    torch.cuda.synchronize()
    assert AC.ulps_apart(out[0].cpu(), 8.0 ** 0.5) <= 1 and AC.ulps_apart(out[1].cpu(), 1.0 / (8.0 ** 0.5 + 1e-6)) <= 1
    assert bool((p < 4.999).all()) and bool((p > 4.99).all()) and bool((m > 0).all())
