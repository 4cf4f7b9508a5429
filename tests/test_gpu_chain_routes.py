"""The backend calls of every route of gru_chain on the HIP backend, pinned (tests/chain_route_cases.py): the cases of the CPU suite
plus the routes only the library has -- the fused x route, the keyed g4, the one-launch weight gradients, decay and offset.

EXPECTED was recorded with run_route in one run on an MI355X with the gru_chain.py of the commit before _GruChainFn was split into
one function per route, and is never regenerated from the code under test.  Every case also runs twice: outputs, d_x and all
parameter gradients of the two runs are equal bit for bit."""
import pytest
import torch

from temp_amd import backend as TB
from tests.chain_route_cases import GPU_CASES, run_route
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]

EXPECTED = {
    "chain": [('gru_chain_pack_x_multi', (), ()),
              ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ()),
              ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
              ('gru_weight_grads_multi', (), ()),
              ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
              ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "chain-d200": [('gru_chain_pack_x_multi', (), ()),
                   ('gru_chain_fwd_x', ((553, 200), (553,), (553, 200), (5, 553, 200)), ()),
                   ('gru_chain_bwd', ((5, 553, 200), (553, 600), (553, 600)), ()),
                   ('gru_weight_grads_multi', (), ()),
                   ('gru_weight_grads', ((324, 200), (324, 200), (324, 600), (324, 600), (600, 200), (324, 200)), ()),
                   ('gru_weight_grads', ((229, 200), (229, 200), (229, 600), (229, 600), (600, 200), (229, 200)), ())],
    "want": [('gru_chain_pack_x_multi', (), ()),
             ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ()),
             ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
             ('gru_weight_grads_multi', (), ()),
             ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
             ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "labels": [('gru_chain_pack_x_multi', (), ()),
               ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ()),
               ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
               ('gru_weight_grads_multi', (), ()),
               ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
               ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "type1": [('gru_input_gates_multi', (), ()),
              ('gru_chain_pack_multi', (), ()),
              ('gru_chain_fwd', ((553, 40), (553, 40), (5, 553, 40)), ()),
              ('gru_chain_bwd', ((5, 553, 40), (553, 40), (553, 120)), ()),
              ('gru_weight_grads_multi', (), ()),
              ('gru_weight_grads', ((324, 40), (324, 40), (324, 40), (324, 120), (40, 40), (324, 40)), ()),
              ('gru_weight_grads', ((229, 40), (229, 40), (229, 40), (229, 120), (40, 40), (229, 40)), ())],
    "two-gate-matrices": [('gru_chain_pack_x_multi', (), ()),
                          ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ()),
                          ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ()),
                          ('gru_weight_grads_multi', (), ()),
                          ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
                          ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "per-gru-weight-grads": [('gru_chain_pack_x_multi', (), ()),
                             ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ()),
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
                     ('gru_weight_grads_multi', (), ()),
                     ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
                     ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ())],
    "one-chain": [('gru_chain_pack_x_multi', (), ()),
                  ('gru_chain_fwd_x', ((324, 32), (324,), (324, 32), (5, 324, 32)), ()),
                  ('gru_chain_bwd', ((5, 324, 32), (324, 96), (324, 96)), ()),
                  ('gru_weight_grads_multi', (), ()),
                  ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ())],
    "zero-state": [('gru_input_gates', ((17, 32), (96, 32), (96,), (17, 96)), ()),
                   ('gru_cell_fwd_multi', ((5, 17, 32),), ()),
                   ('gru_cell_bwd_multi', ((5, 17, 32),), ()),
                   ('gru_weight_grads', ((17, 32), (17, 96), (17, 96), (96, 32), (17, 32)), ())],
    "shared-centre": [('gru_chain_pack_x_multi', (), ()),
                      ('gru_chain_fwd_x', ((60, 32), (72,), (72, 32), (5, 72, 32)), ()),
                      ('gru_chain_bwd', ((5, 72, 32), (72, 96), (72, 96)), ()),
                      ('gru_weight_grads', ((36, 32), (36, 32), (36, 96), (36, 96), (96, 32), (36, 32)), ()),
                      ('gru_weight_grads', ((24, 32), (24, 32), (24, 96), (24, 96), (96, 32), (24, 32)), ()),
                      ('gru_weight_grads', ((12, 32), (12, 32), (12, 96), (12, 96), (96, 32), (12, 32)), ())],
    "decay": [('gru_chain_pack_x_multi', (), ()),
              ('gru_chain_fwd_x', ((553, 32), (553,), (553, 32), (5, 553, 32)), ('decay',)),
              ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ('d_arg', 'decay')),
              ('gru_weight_grads_multi', (), ()),
              ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
              ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ()),
              ('gru_chain_decay_reduce', ((553,),), ())],
    "offset": [('gru_input_gates_multi', (), ()),
               ('gru_chain_pack_multi', (), ('layout',)),
               ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ('offset',)),
               ('gru_chain_bwd', ((5, 553, 32), (553, 96), (553, 96)), ('d_state', 'offset')),
               ('gru_weight_grads_multi', (), ()),
               ('gru_weight_grads', ((324, 32), (324, 32), (324, 96), (324, 96), (96, 32), (324, 32)), ()),
               ('gru_weight_grads', ((229, 32), (229, 32), (229, 96), (229, 96), (96, 32), (229, 32)), ()),
               ('segment_sum_rows', ((553, 32), (8,), (491,)), ())],
    "long-panels-d200": [('gru_input_gates_multi', (), ()),
                         ('gru_chain_pack_multi', (), ()),
                         ('gru_chain_fwd', ((1749, 600), (1749, 200), (5, 1749, 200)), ()),
                         ('gru_chain_bwd', ((5, 1749, 200), (1749, 600), (1749, 600)), ()),
                         ('gru_weight_grads_multi', (), ()),
                         ('gru_weight_grads', ((889, 200), (889, 200), (889, 600), (889, 600), (600, 200), (889, 200)), ()),
                         ('gru_weight_grads', ((860, 200), (860, 200), (860, 600), (860, 600), (600, 200), (860, 200)), ())],
    "large-d200": [('gru_chain_pack_x_multi', (), ()),
                   ('gru_chain_fwd_x', ((18899, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                   ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                   ('gru_grads_g4', (), ('col_keys', 'row_keys'))],
    "large-want-d200": [('gru_chain_pack_x_multi', (), ()),
                        ('gru_chain_fwd_x', ((18899, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                        ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                        ('gru_grads_g4', (), ('col_keys', 'row_keys'))],
    "large-gi-route-d200": [('gru_input_gates_multi', (), ()),
                            ('gru_chain_pack_multi', (), ()),
                            ('gru_chain_fwd', ((18899, 600), (18899, 200), (5, 18899, 200)), ()),
                            ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                            ('gru_grads_g4', (), ('col_keys', 'row_keys'))],
    "large-gi-route-labels-d200": [('gru_input_gates_multi', (), ('x_idx',)),
                                   ('gru_chain_pack_multi', (), ()),
                                   ('gru_chain_fwd', ((9802, 600), (18899, 200), (5, 18899, 200)), ('gi_index',)),
                                   ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                                   ('gru_grads_g4', (), ('col_keys', 'row_keys'))],
    "large-unkeyed-d200": [('gru_chain_pack_x_multi', (), ()),
                           ('gru_chain_fwd_x', ((18899, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                           ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ()),
                           ('gru_grads_g4', (), ())],
    "large-two-gate-matrices-d200": [('gru_chain_pack_x_multi', (), ()),
                                     ('gru_chain_fwd_x', ((18899, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                                     ('gru_chain_bwd', ((5, 18899, 200), (18899, 600), (18899, 600)), ()),
                                     ('gru_weight_grads_multi', (), ())],
    "large-decay-d200": [('gru_chain_pack_x_multi', (), ()),
                         ('gru_chain_fwd_x', ((18899, 200), (18899,), (18899, 200), (5, 18899, 200)), ('decay',)),
                         ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('d_arg', 'decay', 'keys')),
                         ('gru_grads_g4', (), ('col_keys', 'row_keys')),
                         ('gru_chain_decay_reduce', ((18899,),), ())],
    "large-offset-d200": [('gru_input_gates_multi', (), ()),
                          ('gru_chain_pack_multi', (), ('layout',)),
                          ('gru_chain_fwd', ((18899, 600), (18899, 200), (5, 18899, 200)), ('offset',)),
                          ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('d_state', 'offset')),
                          ('gru_grads_g4', (), ()),
                          ('segment_sum_rows', ((18899, 200), (8,), (16446,)), ())],
}


@pytest.fixture
def hip_backend():
    TB.set_backend(None)
    assert TB.get_backend().name == "hip"
    yield
    TB.set_backend(None)


def test_every_case_has_its_list():
    assert set(EXPECTED) == set(GPU_CASES)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_route_launches_and_repeats_bitwise(hip_backend, name):
    dev = torch.device("cuda:0")
    launches, first = run_route(GPU_CASES[name], dev)
    assert launches == EXPECTED[name]
    again, second = run_route(GPU_CASES[name], dev)
    assert again == launches and len(first) == len(second)
    for k, (u, v) in enumerate(zip(first, second)):
        assert (u is None and v is None) or torch.equal(u, v), "tensor %d of the two runs differs" % k
