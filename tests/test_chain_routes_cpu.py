"""The backend calls of every route of gru_chain on the CPU test backend, pinned (tests/chain_route_cases.py).

EXPECTED was recorded with run_route on the commit before _GruChainFn was split into one function per route, on this backend, and
is never regenerated from the code under test: a change that makes a route launch something else has to say so here."""
import pytest
import torch

from temp_amd import backend as TB
from tests.chain_route_cases import CASES, run_route
from tests.cpu_backend import CpuTestBackend

EXPECTED = {
    "chain": [('gru_input_gates_multi', (), ()),
              ('gru_chain_pack', ((96, 32),), ()),
              ('gru_chain_pack', ((96, 32),), ()),
              ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ()),
              ('gru_chain_bwd_g4', ((5, 553, 32), (553, 128)), ()),
              ('gru_grads_g4', (), ())],
    "chain-d200": [('gru_input_gates_multi', (), ()),
                   ('gru_chain_pack', ((600, 200),), ()),
                   ('gru_chain_pack', ((600, 200),), ()),
                   ('gru_chain_fwd', ((553, 600), (553, 200), (5, 553, 200)), ()),
                   ('gru_chain_bwd_g4', ((5, 553, 200), (553, 800)), ()),
                   ('gru_grads_g4', (), ())],
    "want": [('gru_input_gates_multi', (), ()),
             ('gru_chain_pack', ((96, 32),), ()),
             ('gru_chain_pack', ((96, 32),), ()),
             ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ()),
             ('gru_chain_bwd_g4', ((5, 553, 32), (553, 128)), ()),
             ('gru_grads_g4', (), ())],
    "labels": [('gru_input_gates_multi', (), ('x_idx',)),
               ('gru_chain_pack', ((96, 32),), ()),
               ('gru_chain_pack', ((96, 32),), ()),
               ('gru_chain_fwd', ((280, 96), (553, 32), (5, 553, 32)), ('gi_index',)),
               ('gru_chain_bwd_g4', ((5, 553, 32), (553, 128)), ()),
               ('gru_grads_g4', (), ())],
    "type1": [('gru_input_gates_multi', (), ()),
              ('gru_chain_pack', ((120, 40),), ()),
              ('gru_chain_pack', ((120, 40),), ()),
              ('gru_chain_fwd', ((553, 40), (553, 40), (5, 553, 40)), ()),
              ('gru_chain_bwd', ((5, 553, 40), (553, 40), (553, 120)), ()),
              ('gru_weight_grads_multi', (), ()),
              ('gru_weight_grads', ((324, 40), (324, 40), (324, 40), (324, 120), (40, 40), (324, 40)), ()),
              ('gru_weight_grads', ((229, 40), (229, 40), (229, 40), (229, 120), (40, 40), (229, 40)), ())],
    "two-gate-matrices": [('gru_input_gates_multi', (), ()),
                          ('gru_chain_pack', ((96, 32),), ()),
                          ('gru_chain_pack', ((96, 32),), ()),
                          ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ()),
                          ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
                          ('gru_weight_grads_multi', (), ())],
    "per-gru-weight-grads": [('gru_input_gates_multi', (), ()),
                             ('gru_chain_pack', ((96, 32),), ()),
                             ('gru_chain_pack', ((96, 32),), ()),
                             ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ()),
                             ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
                             ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
                             ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "per-position": [('gru_input_gates_multi', (), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_fwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_cell_bwd_multi', ((5, 553, 32),), ()),
                     ('gru_weight_grads_multi', (), ())],
    "one-chain": [('gru_input_gates', ((324, 32), (96, 32), (96,), (324, 96)), ()),
                  ('gru_chain_pack', ((96, 32),), ()),
                  ('gru_chain_fwd', ((324, 96), (324, 32), (5, 324, 32)), ()),
                  ('gru_chain_bwd_g4', ((5, 324, 32), (324, 128)), ()),
                  ('gru_grads_g4', (), ())],
    "zero-state": [('gru_input_gates', ((17, 32), (96, 32), (96,), (17, 96)), ()),
                   ('gru_cell_fwd_multi', ((5, 17, 32),), ()),
                   ('gru_cell_bwd_multi', ((5, 17, 32),), ()),
                   ('gru_weight_grads', ((17, 32), (17, 96), (17, 96), (96, 32), (17, 32)), ())],
    "shared-centre": [('gru_input_gates_multi', (), ()),
                      ('gru_chain_pack', ((96, 32),), ()),
                      ('gru_chain_pack', ((96, 32),), ()),
                      ('gru_chain_fwd', ((72, 96), (72, 32), (5, 72, 32)), ()),
                      ('gru_chain_bwd', ((5, 72, 32), (72, 96), (72, 96)), ()),
                      ('gru_weight_grads', ((36, 32), (36, 32), (36, 96), (36, 96), (96, 32), (36, 32)), ()),
                      ('gru_weight_grads', ((24, 32), (24, 32), (24, 96), (24, 96), (96, 32), (24, 32)), ()),
                      ('gru_weight_grads', ((12, 32), (12, 32), (12, 96), (12, 96), (96, 32), (12, 32)), ())],
}


@pytest.fixture
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


def test_every_case_has_its_list():
    assert set(EXPECTED) == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_launches(cpu_backend, name):
    launches, _ = run_route(CASES[name], torch.device("cpu"))
    assert launches == EXPECTED[name]
