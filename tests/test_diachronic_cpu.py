"""The embedding-only baselines (temp_amd.non_recurrent: Static / DiachronicEmbedding) and the diachronic table node without a GPU:
the cases of tests/diachronic_cases.py driven through test backends that add the contract of temp_diachronic_rows_fwd / _bwd
(include/temp_amd.h) in torch."""
import pytest
import torch

from temp_amd import backend as TB
from tests import diachronic_cases as DC
from tests.cpu_backend import CpuTestBackend
from tests.test_gated_transe_cpu import GatedL1CpuBackend


class _DiachronicRows:
    """diachronic_rows_fwd / _bwd: the argument is t * w rounded, then + b rounded (two fp32 operations, as the kernels form it);
    the backward recomputes sin / cos and adds the B terms in ascending b."""

    @staticmethod
    def _arg(w, b, t):
        prod = t.view(-1, 1, 1) * w.detach().unsqueeze(0)
        return prod + b.detach().unsqueeze(0)                                  # (B, N, d - ds)

    def diachronic_rows_fwd(self, ent, w, b, t):
        ent = ent.detach()
        N, d = ent.shape
        ds, B = d // 2, t.shape[0]
        assert tuple(w.shape) == tuple(b.shape) == (N, d - ds) and t.dtype == torch.float32 and t.dim() == 1 and B >= 1
        out = ent.unsqueeze(0).repeat(B, 1, 1)
        out[:, :, ds:] = ent[:, ds:].unsqueeze(0) * torch.sin(self._arg(w, b, t))
        return out.reshape(B * N, d)

    def diachronic_rows_bwd(self, ent, w, b, t, d_out):
        ent = ent.detach()
        N, d = ent.shape
        ds, B = d // 2, t.shape[0]
        g = d_out.detach().view(B, N, d)
        arg = self._arg(w, b, t)
        sn, cs = torch.sin(arg), torch.cos(arg)
        d_ent = torch.zeros_like(ent)
        d_w, d_b = torch.zeros(N, d - ds), torch.zeros(N, d - ds)
        for i in range(B):                                                      # ascending b, as the kernel's registers
            d_ent[:, :ds] += g[i, :, :ds]
            d_ent[:, ds:] += g[i, :, ds:] * sn[i]
            gc = g[i, :, ds:] * ent[:, ds:] * cs[i]
            d_b += gc
            d_w += gc * t[i]
        return d_ent, d_w, d_b


class DiachronicCpuBackend(_DiachronicRows, CpuTestBackend):
    name = "cpu-test-diachronic"


class DiachronicL1CpuBackend(_DiachronicRows, GatedL1CpuBackend):
    """... with the L1 methods, for TransE."""
    name = "cpu-test-diachronic-l1"


DEV = torch.device("cpu")


def _backend_for(name_or_kind):
    return DiachronicL1CpuBackend() if "transe" in name_or_kind.lower() else DiachronicCpuBackend()


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(DiachronicCpuBackend())
    yield
    TB.set_backend(None)


def test_node_equals_torch_composition():
    DC.check_node(DEV)


def test_node_wants_float32_times():
    ent, w = torch.zeros(3, 4), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="float32"):
        DC.TF.diachronic_rows(ent, w, w, torch.tensor([1, 2]))


@pytest.mark.parametrize("name", DC.G24)
def test_g24_tables_loss_gradients(name):
    TB.set_backend(_backend_for(name))
    DC.check_g24(name, DEV)


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_state_dict_is_the_references(name):
    DC.check_state_dict(name, DEV)


@pytest.mark.parametrize("name", DC.G25)
def test_g25_evaluate(name):
    DC.check_g25(name, DEV)


@pytest.mark.parametrize("name,kind", [("G24_de_complex", "complex"), ("G24_de_complex", "distmult"), ("G24_de_complex", "transE"),
                                       ("G24_static_complex", "complex")])
def test_fused_route_equals_per_graph(name, kind):
    TB.set_backend(_backend_for(kind))
    n_fwd, n_bwd = DC.check_fused_equals_per_graph(name, DEV, kind)
    assert (n_fwd, n_bwd) == ((1, 1) if "de" in name else (0, 0)), "one table launch each way for the whole batch"


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_prepared_batch_is_repeatable(name):
    DC.check_prepared_repeatable(name, DEV)


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_edge_batches(name):
    DC.check_edge_batches(name, DEV)


def test_width_without_a_fused_node_takes_the_per_graph_route():
    """D = 6 is outside the loss kernels' alignment: forward() falls to train_link_prediction_both, still on one table node, and
    run_loss on the prepared batch says so."""
    from temp_amd.non_recurrent import DiachronicEmbedding
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    torch.manual_seed(0)
    m = DiachronicEmbedding(make_args(module="DE", embed_size=6, hidden_size=6), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    assert m.static_embed_size == 3 and tuple(m.w_temp_ent_embeds.shape) == (s["num_e"], 3) and not m._fused_loss_ok()
    with DC.recording() as rec:
        loss = m([2, 5])
        loss.backward()
    assert torch.isfinite(loss) and rec.count("diachronic_rows_fwd") == 1 and rec.count("diachronic_rows_bwd") == 1
    with pytest.raises(NotImplementedError):
        m.run_loss(m.prepare([2, 5]))
