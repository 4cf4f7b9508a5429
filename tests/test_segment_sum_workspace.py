"""temp_segment_sum_rows_workspace answers on the host, and its answer names the route temp_segment_sum_rows will take: the table of
tests/row_loss_route_cases.py (every route of the dispatch, and the widths past a wave of float4 columns) without a device."""
from temp_amd import _lib
from tests import row_loss_route_cases as RC


def test_segment_sum_workspace_table():
    lib = _lib.load()
    seen = set()
    for name, d in RC.NARROW + RC.WIDE:
        n_seg, n_rows = RC.check_shape(name)
        got = lib.temp_segment_sum_rows_workspace(n_seg, n_rows, d)
        assert got == RC.workspace_bytes(name, d), (name, d, got, RC.workspace_bytes(name, d))
        assert (got > 0) == (RC.launches(name, d) == 2), (name, d)
        seen.add(RC.route(name, d))
    assert seen == {"short", "pieces", "blk4", "blk16", "split", "wide"}
    assert lib.temp_segment_sum_rows_workspace(0, 100, 8) == 0 and lib.temp_segment_sum_rows_workspace(10, 0, 16) == 0
