"""Poisoned allocations: while active, every buffer that `torch.empty`, `torch.empty_like` or `Tensor.new_empty`
hands out is filled with a value that no correct result contains, so that an output element a kernel never
writes, or a workspace word it reads before writing, shows up in the comparison instead of holding the previous
call's answer (the caching allocator returns the block the last call of the same shape released).

The library allocates nothing itself: every output and workspace is one of these three calls in temp_amd/*.py
(nothing there uses `torch.empty_strided`), so this reaches all of them.  `torch.zeros`, `torch.full` and the
random constructors are left alone.

Fill by dtype:
  floating / complex   NaN
  signed integers      -2   (not -1: the ABI uses -1 as "none" in prev_idx, top_idx and keep, so an unwritten
                             slot would read as a valid filler; a small negative index, if a kernel wrongly
                             uses one, reads just beside its buffer instead of far away)
  uint8                the `_ws` workspaces, which kernels reinterpret: the 4-byte-aligned prefix is the 32-bit
                       word 0xFFFFFFFE (NaN as fp32, as fp64 and as an fp16 pair; -2 as int32), tail bytes 0xFF
  bool                 True
  zero-size tensors    untouched

The poison is not chosen to make anything fault.  Use the context manager around single calls, or the fixture
of the same name for a whole module:

    from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
    pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
"""
import contextlib

import pytest
import torch

INT_POISON = -2
WORD_POISON = 0xFFFFFFFE                      # as int32: -2
_WORD_BYTES = (0xFE, 0xFF, 0xFF, 0xFF)        # the same word, little-endian
_SIGNED = (torch.int8, torch.int16, torch.int32, torch.int64)


def _fill_bytes(t):
    n = t.numel()
    if t.is_contiguous() and t.data_ptr() % 4 == 0:
        flat = t.view(-1)
        n4 = n - n % 4
        if n4:
            flat[:n4].view(torch.int32).fill_(INT_POISON)
        if n4 < n:
            flat[n4:].fill_(0xFF)
        return
    # any other layout: the same byte sequence in logical order
    pat = torch.tensor(_WORD_BYTES, dtype=torch.uint8).repeat(n // 4 + 1)[:n]
    pat[n - n % 4:] = 0xFF
    t.copy_(pat.view(t.shape))


def poison_(t):
    """Fill `t` in place with its dtype's poison; returns `t`."""
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or t.layout != torch.strided or t.is_meta:
        return t
    with torch.no_grad():
        if t.dtype.is_floating_point or t.dtype.is_complex:
            t.fill_(float("nan"))
        elif t.dtype in _SIGNED:
            t.fill_(INT_POISON)
        elif t.dtype == torch.uint8:
            _fill_bytes(t)
        elif t.dtype == torch.bool:
            t.fill_(True)
    return t


@contextlib.contextmanager
def poisoned_allocations():
    real_empty, real_empty_like = torch.empty, torch.empty_like
    own_new_empty = "new_empty" in torch.Tensor.__dict__          # else inherited from the C base class
    real_new_empty = torch.Tensor.new_empty

    def empty(*args, **kwargs):
        return poison_(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return poison_(real_empty_like(*args, **kwargs))

    def new_empty(self, *args, **kwargs):
        return poison_(real_new_empty(self, *args, **kwargs))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like
        if own_new_empty:
            torch.Tensor.new_empty = real_new_empty
        else:
            del torch.Tensor.new_empty


@pytest.fixture(name="poisoned_allocations")
def poisoned_allocations_fixture():
    with poisoned_allocations():
        yield
