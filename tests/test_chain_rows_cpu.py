"""GruProgram.x_rows: the table row of every chain row when the x rows are a selection of a table's rows (gru_chain(table=...))."""
import numpy as np
import torch

from tests.chain_cases import random_program
from tests.chain_route_cases import shared_centre_program

CPU = torch.device("cpu")


def _x_index(prog):
    return np.concatenate([it.x0 + np.arange(it.n) for it in prog.inst]) if prog.inst else np.zeros(0, dtype=np.int64)


def test_x_rows_composes_chain_rows_with_x_index_shared_centre():
    """Two instances read the same x rows (the centre of a bi-directional window): both get those rows' table rows."""
    prog, n_x = shared_centre_program()
    assert prog.x_rows(CPU) is None                                  # never composed
    rng = np.random.default_rng(1)
    chain = rng.integers(0, 41, n_x)                                 # table rows repeat among the x rows
    tab = prog.x_rows(CPU, chain)
    assert tab.dtype == torch.int32 and tab.shape == (prog.n_total,)
    assert np.array_equal(tab.numpy(), chain[_x_index(prog)])
    a, b = prog.inst[2], prog.inst[5]                                # the two centre cells
    assert a.x0 == b.x0 and np.array_equal(tab.numpy()[a.h0:a.h0 + a.n], tab.numpy()[b.h0:b.h0 + b.n])
    assert prog.x_rows(CPU) is tab                                   # cached
    assert prog.x_rows_count == n_x and prog.x_rows_max == int(chain.max()) + 1


def test_x_rows_random_program_and_zero_rows():
    prog, n_x = random_program(33)
    chain = np.random.default_rng(2).permutation(n_x + 9)[:n_x]
    assert np.array_equal(prog.x_rows(CPU, chain).numpy(), chain[_x_index(prog)])
    chain[5] = -1                                                    # a zero row has no table row to read in place
    assert prog.x_rows(CPU, chain) is None and prog.x_rows(CPU) is None
