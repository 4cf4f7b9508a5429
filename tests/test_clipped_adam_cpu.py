"""temp_amd.optim.ClippedAdam without a GPU: the composite route (plain torch, the contract of include/temp_amd.h with the norm in
fp64) against clip_grad_norm_ + torch.optim.Adam and the fp64 contract of tests/clipped_adam_cases.py; state dicts; the
configure_clipped_optimizer hook; two slice models."""
import argparse
import copy

import pytest
import torch

from temp_amd import backend as TB
from temp_amd.optim import ClippedAdam
from tests import clipped_adam_cases as AC
from tests.cpu_backend import CpuTestBackend
from tests.golden_util import load

DEV = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


_STD = {}


def _standard():
    """Inputs, fp64 contract, our run and the torch fp32 run of the standard set, computed once."""
    if not _STD:
        inp = AC.standard_inputs()
        groups = AC.one_group(inp)
        _STD.update(inp=inp, groups=groups, want=AC.contract_fp64(inp, groups, AC.MAX_NORM))
        params, opt, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
        _STD.update(ours=AC.moments(params, opt), opt=opt, params=params, seen=seen)
        rp, ro = AC.run_torch(inp, groups, AC.MAX_NORM, DEV)
        _STD.update(ref=AC.moments(rp, ro))
    return _STD


def test_the_cpu_backend_has_no_kernels_and_stays_untouched():
    assert not hasattr(CpuTestBackend(), "adam_clip_step") and not hasattr(CpuTestBackend(), "grad_norm_clip")


def test_fp64_composite_equals_torch():
    inp = AC.standard_inputs()
    groups = AC.one_group(inp)
    ours, opt, _ = AC.run_ours(inp, groups, AC.MAX_NORM, DEV, dtype=torch.float64)
    ref, ropt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV, dtype=torch.float64)
    for i, (a, b) in enumerate(zip(AC.moments(ours, opt), AC.moments(ref, ropt))):
        for x, y in zip(a, b):
            if y is None:
                assert x is None
                continue
            rel = float((x - y).abs().max()) / max(float(y.abs().max()), 1e-300)
            assert rel <= 1e-12, (i, rel)
    P = AC.contract_fp64(inp, groups, AC.MAX_NORM)[0]
    for a, w in zip(ours, P):
        assert float((a.detach() - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1.0)


def test_fp32_composite_inside_the_band():
    s = _standard()
    assert min(s["want"][4]) > 100.0, "the clip is active: the norm is far above max_norm"
    AC.check_band(s["ours"], s["ref"], s["want"][:3], "cpu composite")
    for (norm, coef), n64, c64 in zip(s["seen"], s["want"][4], s["want"][5]):
        assert AC.ulps_apart(norm, n64) <= 1 and AC.ulps_apart(coef, c64) <= 1


def test_under_the_threshold_the_coefficient_is_one_and_nothing_changes():
    inp = AC.standard_inputs(grad_scale=1e-3)
    groups = AC.one_group(inp)
    assert max(AC.contract_fp64(inp, groups, AC.MAX_NORM)[4]) < 1.0
    a, oa, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    b, ob, _ = AC.run_ours(inp, groups, None, DEV)
    assert all(float(c) == 1.0 for _, c in seen)
    assert ob.last_grad_norm is None and ob.last_clip_coef is None
    for x, y in zip(AC.moments(a, oa), AC.moments(b, ob)):
        for u, v in zip(x, y):
            assert (u is None and v is None) or torch.equal(u, v)


def test_parameter_without_gradient_is_skipped_entirely():
    s = _standard()
    none = len(s["inp"]) - 1
    assert torch.equal(s["params"][none].detach(), s["inp"].values[none])
    assert s["params"][none] not in s["opt"].state
    assert all(s["opt"].state[p]["step"] == AC.STEPS for p in s["params"][:none])


def test_late_gradient_starts_its_own_step_count():
    inp = AC.standard_inputs()
    none = len(inp) - 1
    g = torch.Generator().manual_seed(9)
    for k in (2, 3, 4):                                   # first gradient at the third step
        inp.grads[k][none] = torch.randn(17, generator=g)
    groups = AC.one_group(inp)
    ours, opt, _ = AC.run_ours(inp, groups, AC.MAX_NORM, DEV, steps=3)
    assert opt.state[ours[none]]["step"] == 1 and opt.state[ours[0]]["step"] == 3
    ours, opt, _ = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    assert opt.state[ours[none]]["step"] == 3 and opt.state[ours[0]]["step"] == 5
    ref, ropt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV)
    want = AC.contract_fp64(inp, groups, AC.MAX_NORM)
    assert want[3][none] == 3
    AC.check_band(AC.moments(ours, opt), AC.moments(ref, ropt), want[:3], "late gradient")


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_nonfinite_gradients_follow_the_arithmetic(kind):
    AC.check_nonfinite(kind, DEV, fused=False)


def test_two_groups_share_one_global_norm():
    inp = AC.standard_inputs(seed=4)
    n = len(inp)
    groups = [(list(range(0, n, 2)), 1e-3, 1e-4), (list(range(1, n, 2)), 3e-3, 0.0)]
    ours, opt, seen = AC.run_ours(inp, groups, AC.MAX_NORM, DEV)
    ref, ropt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV)
    want = AC.contract_fp64(inp, groups, AC.MAX_NORM)
    order = [i for idx, _, _ in groups for i in idx]
    assert order != sorted(order)
    AC.check_band(AC.moments(ours, opt), AC.moments(ref, ropt), want[:3], "two groups")
    for (norm, _), n64 in zip(seen, want[4]):
        assert AC.ulps_apart(norm, n64) <= 1


def _state_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].keys() == b[k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a[k]["step"]) == float(b[k]["step"])
        assert torch.equal(a[k]["exp_avg"], b[k]["exp_avg"]) and torch.equal(a[k]["exp_avg_sq"], b[k]["exp_avg_sq"])


def test_state_dict_round_trip_with_torch_adam():
    inp = AC.standard_inputs(steps=2)
    groups = AC.one_group(inp)
    tparams, topt = AC.run_torch(inp, groups, AC.MAX_NORM, DEV)
    sd = topt.state_dict()
    mine = ClippedAdam(AC.build_params(inp, DEV), max_norm=1.0)
    mine.load_state_dict(copy.deepcopy(sd))
    assert all(isinstance(st["step"], int) and st["step"] == 2 for st in mine.state.values())
    assert mine.param_groups[0]["lr"] == AC.LR and mine.param_groups[0]["weight_decay"] == AC.WD
    back = torch.optim.Adam(AC.build_params(inp, DEV))
    back.load_state_dict(copy.deepcopy(mine.state_dict()))
    _state_equal(back.state_dict()["state"], sd["state"])
    assert all(torch.is_tensor(st["step"]) for st in back.state.values())
    params = AC.build_params(inp, DEV)                       # and torch's Adam can go on stepping from it
    cont = torch.optim.Adam(params)
    cont.load_state_dict(copy.deepcopy(mine.state_dict()))
    AC.set_grads(params, inp, 0, DEV)
    cont.step()
    assert float(cont.state[params[0]]["step"]) == 3.0


def test_interrupted_run_is_bit_equal():
    s = _standard()

    def reload(k, params, opt):
        if k != 2:
            return opt
        sd = copy.deepcopy(opt.state_dict())
        new = ClippedAdam([dict(params=params, lr=AC.LR, weight_decay=AC.WD)], betas=AC.BETAS, eps=AC.EPS, max_norm=AC.MAX_NORM)
        new.load_state_dict(sd)
        return new

    params, opt, _ = AC.run_ours(s["inp"], s["groups"], AC.MAX_NORM, DEV, opt_hook=reload)
    assert opt is not s["opt"]
    for x, y in zip(AC.moments(params, opt), s["ours"]):
        for u, v in zip(x, y):
            assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_amsgrad_and_maximize_are_refused(flag):
    p = [torch.nn.Parameter(torch.ones(3))]
    sd = torch.optim.Adam(p, **{flag: True}).state_dict()
    with pytest.raises(ValueError, match=flag):
        ClippedAdam(p).load_state_dict(sd)


def test_sparse_gradients_are_refused():
    p = torch.nn.Parameter(torch.ones(4, 2))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2))
    with pytest.raises(RuntimeError, match="sparse"):
        ClippedAdam([p], max_norm=1.0).step()


def test_constructor_checks():
    p = [torch.nn.Parameter(torch.ones(3))]
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1), dict(max_norm=0.0), dict(max_norm=-2.0)):
        with pytest.raises(ValueError):
            ClippedAdam(p, **kw)


def _tiny_model(**ns):
    from temp_amd.tkg_module import TKG_Module

    class M(TKG_Module):
        def build_model(self):
            self.w = torch.nn.Parameter(torch.ones(5))

    args = argparse.Namespace(embed_size=4, hidden_size=4, num_pos_facts=1, negative_rate=1, score_function="distmult", lr=2e-3, debug=True,
                              **ns)
    return M(args, 3, 2, {0: None}, {}, {})


def test_hook_honours_gradient_clip_val():
    opt = _tiny_model(gradient_clip_val=0.25).configure_clipped_optimizer()
    assert isinstance(opt, ClippedAdam) and opt.max_norm == 0.25
    assert opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["weight_decay"] == 1e-4
    assert _tiny_model(gradient_clip_val=0).configure_clipped_optimizer().max_norm is None
    assert _tiny_model(gradient_clip_val=-1.0).configure_clipped_optimizer().max_norm is None
    assert _tiny_model().configure_clipped_optimizer().max_norm == 1.0
    assert _tiny_model(gradient_clip_val=0.25).configure_clipped_optimizer(max_norm=3.0).max_norm == 3.0
    assert _tiny_model(gradient_clip_val=0.25).configure_clipped_optimizer(max_norm=0).max_norm is None
    plain = _tiny_model(gradient_clip_val=0.25).configure_optimizers()
    assert type(plain) is torch.optim.Adam and plain.param_groups[0]["weight_decay"] == 1e-4


def test_diachronic_model_steps_inside_the_band():
    from tests import diachronic_cases as DC
    from tests.test_diachronic_cpu import DiachronicCpuBackend
    TB.set_backend(DiachronicCpuBackend())
    z = load("G24_de_complex")
    m = DC.build_model(z, DEV)
    t_list, samples = torch.tensor([int(t) for t in z["t_list"]]), DC.fixture_samples(z)
    AC.check_model_band(m, lambda: m(t_list, samples=samples), DEV, False, 3, "DiachronicEmbedding")


def test_grrgcn_model_steps_inside_the_band():
    from tests.window_cases import build_window_model, window_inputs
    z = load("G10_uni_grrgcn_rol")
    m = build_window_model(z, DEV)
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    worst, opt = AC.check_model_band(m, lambda: m(t_list, target_edge_ids=edge_ids, samples=samples), DEV, False, 3, "GRRGCN")
    assert float(opt.last_clip_coef) <= 1.0
