"""Post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN) on the CPU test backend: goldens G20 / G21 on the batched and
generic paths, the fused gated loss and its gradients against an fp64 restatement, the reference's quirks."""
import pytest

from temp_amd import backend as TB
from tests import post_aggregation_cases as PA
from tests.cpu_backend import CpuTestBackend

CPU = "cpu"


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("name", ["G20_post_agg_uni", "G20_post_agg_bi", "G20_post_agg_uni_full"])
def test_post_aggregation_own_gates_golden(name, batched):
    PA.check_g20(name, CPU, batched)


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("name", ["G21_eval_post_agg_uni", "G21_eval_post_agg_bi"])
def test_post_aggregation_evaluate_golden(name, batched):
    PA.check_g21(name, CPU, batched)


@pytest.mark.parametrize("kind,bi", [("complex", True), ("distmult", False)])
def test_gated_loss_definition_and_quirks(kind, bi):
    PA.check_gated_loss_definition(CPU, kind, bi)


@pytest.mark.parametrize("kind", ["complex", "distmult"])
def test_gated_loss_per_window_equals_literal(kind):
    PA.check_per_window_equals_batched(CPU, kind)


def test_post_aggregation_classes_exported():
    from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN, PostDynamicRGCN, ImputeBiDynamicRGCN, ImputeDynamicRGCN
    assert issubclass(PostDynamicRGCN, ImputeDynamicRGCN) and issubclass(PostBiDynamicRGCN, ImputeBiDynamicRGCN)
    assert not PostBiDynamicRGCN.head_scored_as_tail
