"""The all-entity ("1-vs-all") loss without a GPU: the torch composite against a row-by-row restatement, the carry contract of the
composite's panel form, the autograd node (one pass and panels) against the literal fp64 expression on the CPU test backend, and
the option through the models."""
import numpy as np
import pytest
import torch

from temp_amd import backend as TB
from temp_amd import evaluation
from temp_amd import link_loss as LL
from tests import all_entity_cases as AC
from tests.cpu_backend import CpuTestBackend


@pytest.fixture(autouse=True)
def cpu_backend():
    be = CpuTestBackend()
    TB.set_backend(be)
    yield be
    TB.set_backend(None)


def test_backend_has_no_filtered_ce_kernels(cpu_backend):
    """The CPU test backend stays without the kernels: everything below runs the composite route."""
    assert not hasattr(cpu_backend, "filtered_ce_fwd") and not hasattr(cpu_backend, "filtered_ce_bwd")


@pytest.mark.parametrize("P,N,ld", [(1, 8, 8), (5, 64, 64), (33, 1000, 1000), (7, 4001, 4004)])
def test_composite_against_row_loop(P, N, ld):
    """filtered_ce_rows_torch in fp64 against a loop over the rows that selects the admissible columns by hand."""
    c = AC.kernel_case(P, N, ld, 1.0)
    for p in range(P):
        t = int(c["truth"][p])
        keep = np.setdiff1d(np.arange(N), c["rows"][p][c["rows"][p] != t])
        x = c["s"][p, torch.from_numpy(keep)].double()
        lse = torch.logsumexp(x, 0)
        assert abs(float(lse) - float(c["lse64"][p])) <= 1e-12 * abs(float(lse))
        assert abs(float(lse - c["s"][p, t].double()) - float(c["loss64"][p])) <= 1e-12 * max(1.0, abs(float(lse)))
    assert bool((c["d64"][AC.filtered_mask(c)] == 0).all()) and bool((c["d64"][c["P"] // 2] == 0).all() or P == 1)
    # an all-but-truth row: the loss is 0, the gradient too
    if P >= len(AC.LIST_KINDS):
        p = AC.LIST_KINDS.index("all-but-truth")
        assert abs(float(c["loss64"][p])) < 1e-12 and float(c["d64"][p].abs().max()) < 1e-12


@pytest.mark.parametrize("panel", [4, 64, 44])
def test_composite_panels_carry(panel, cpu_backend):
    """The panel form of a backend without the kernels (link_loss._filtered_ce_fwd / _bwd) over panels equals one call and the fp64
    reference; a panel that is entirely filtered for a row leaves its state unchanged; no NaN."""
    c = AC.kernel_case(33, 1000, 1000, 1.0)
    N = c["N"]
    p_all = AC.LIST_KINDS.index("all-but-truth")
    c["truth"][p_all] = N - 1                                   # the truth in the last panel: every earlier one is entirely filtered
    c["rows"][p_all] = np.arange(N - 1)
    c["lo"], c["hi"], c["ids"] = AC.pack_lists(c["rows"])
    c.update(AC.reference(c, c["rs"]))
    state, states = None, []
    for c0 in range(0, N, panel):
        loss, lse, state = LL._filtered_ce_fwd(cpu_backend, c["s"][:, c0:min(N, c0 + panel)].contiguous(), c["truth"], c["lo"], c["hi"], c["ids"], c0, state)
        assert not bool(torch.isnan(state).any()) and not bool(torch.isnan(loss).any())
        states.append(state.clone())
    assert float(states[0][0, p_all]) == float("-inf") and float(states[0][1, p_all]) == 0.0
    one_loss, one_lse, _ = LL._filtered_ce_fwd(cpu_backend, c["s"], c["truth"], c["lo"], c["hi"], c["ids"], 0, None)
    for got, want in ((loss, c["loss64"]), (lse, c["lse64"]), (one_loss, c["loss64"]), (one_lse, c["lse64"])):
        assert bool(torch.isfinite(got).all())
        assert bool(((got.double() - want).abs() <= 2e-6 + 2e-5 * want.abs()).all())
    d = torch.cat([LL._filtered_ce_bwd(cpu_backend, c["s"][:, c0:min(N, c0 + panel)].contiguous(), c["truth"], c["lo"], c["hi"], c["ids"], c0, lse,
                                       torch.tensor([0.7]), c["rs"]) for c0 in range(0, N, panel)], dim=1)
    assert bool(((d.double() - c["d64"]).abs() <= 2e-6 + 2e-5 * c["d64"].abs()).all())
    assert bool((d[AC.filtered_mask(c)] == 0).all()) and bool((d[c["P"] // 2] == 0).all())


@pytest.mark.parametrize("panel", [None, 16])
@pytest.mark.parametrize("kind", AC.NODE_KINDS)
def test_node_against_literal_fp64(kind, panel):
    AC.check_node(kind, torch.device("cpu"), panel)


def test_node_refuses_other_scorers_and_odd_panels():
    plan, _ = AC.node_plan(torch.device("cpu"))
    ent, rel, big = AC.node_leaves(torch.device("cpu"))
    with pytest.raises(ValueError):
        LL.batched_all_entity_link_prediction(ent, rel, big, "transE", plan)
    with pytest.raises(ValueError):
        LL.batched_all_entity_link_prediction(ent, rel, big, "distmult", plan, panel=6)
    assert LL.ALL_ENTITY_PANEL_BYTES == evaluation.TOPK_PANEL_BYTES
    assert LL.all_entity_panel(None, 3200, 7128) == 7128 and LL.all_entity_panel(None, 3200, 1 << 19) == (LL.ALL_ENTITY_PANEL_BYTES // (4 * 3200)) // 4 * 4


def test_window_model_fused_equals_literal(cpu_backend):
    calls = []
    draw = cpu_backend.corrupt_sample
    cpu_backend.corrupt_sample = lambda *a, **k: calls.append("corrupt_sample") or draw(*a, **k)
    AC.check_window_model(torch.device("cpu"))
    assert calls == ["corrupt_sample"], "only the option-off step at the end draws"


def test_static_model_fused_equals_literal():
    AC.check_static_model(torch.device("cpu"))


def test_simple_model_fused_equals_literal():
    AC.check_simple_model(torch.device("cpu"))


def test_option_off_by_default_and_refusals():
    m, _, _ = AC.static_model(torch.device("cpu"), all_entity_loss=False)
    assert m.all_entity_loss is False
    from tests.window_cases import make_args
    args = make_args(module="SRGCN")
    assert not hasattr(args, "all_entity_loss")
    AC.check_refusals()
