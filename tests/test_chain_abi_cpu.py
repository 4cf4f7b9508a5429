"""The argument contract of temp_gru_chain_fwd / temp_gru_chain_bwd (include/temp_amd.h: "Return contract of the two calls").

Every case is an EMPTY chain (n_panels = 0): the call ends in an error code or in the empty chain's TEMP_OK before any HIP call, so
nothing here can launch and no GPU is needed (the library loads without one, as test_abi.py shows).  The pointers are dummy host
addresses that no check reads through.  The NULL checks of the buffers sit behind the empty-chain return and are not tested here.
"""
import ctypes

import pytest

from temp_amd import _lib

OK, BADARG, UNSUPPORTED = 0, 1, 2
F32, BX, HX, HX_X = _lib.CHAIN_PACK_F32, _lib.CHAIN_PACK_BX, _lib.CHAIN_PACK_HX, _lib.CHAIN_PACK_HX_X
TORCH, TYPE1 = _lib.GRU_TORCH, _lib.GRU_TYPE1

# (id, descriptor overrides, expected code) -- the same in both directions.  Defaults: d = 16, nn.GRU cell, one GRU, max_steps = 1,
# F32 packs, fixed lambda, no offset.  decay: "ok" | "null_wb"; offset: "ok" | "null_table" | "no_rows".
DESCRIPTOR = [
    ("plain", {}, OK),
    ("variant_7", {"variant": 7}, BADARG),
    ("n_rnn_5", {"n_rnn": 5}, BADARG),
    ("max_steps_65", {"max_steps": 65}, BADARG),
    ("bx_at_d12", {"d": 12, "layout": BX}, BADARG),
    ("d_248", {"d": 248}, UNSUPPORTED),
    ("decay", {"decay": "ok", "n_rnn": 4}, OK),
    ("decay_null_wb", {"decay": "null_wb", "n_rnn": 4}, BADARG),
    ("offset_null_table", {"offset": "null_table", "layout": BX}, BADARG),
    ("offset_no_rows", {"offset": "no_rows", "layout": BX}, BADARG),
    ("offset_on_bx", {"offset": "ok", "layout": BX}, OK),
    ("offset_on_f32_with_decay", {"offset": "ok", "decay": "ok"}, OK),
    ("offset_on_hx", {"offset": "ok", "layout": HX}, UNSUPPORTED),
]

# (id, descriptor overrides, the non-NULL members of TempChainFwd, expected code)
FWD_ROUTES = [
    ("gi_and_x", {"layout": HX_X}, ("gi", "x"), BADARG),                       # stricter than the split entries: inexpressible there
    ("x", {"layout": HX_X}, ("x",), OK),
    ("x_decay", {"layout": HX_X, "decay": "ok"}, ("x",), OK),
    ("x_on_f32_packs", {}, ("x",), BADARG),
    ("x_on_hx_packs", {"layout": HX}, ("x",), BADARG),
    ("x_type1", {"layout": HX_X, "variant": TYPE1}, ("x",), UNSUPPORTED),
    ("x_panel_too_long", {"layout": HX_X, "d": 200, "max_steps": 64}, ("x",), UNSUPPORTED),
    ("x_offset", {"layout": HX_X, "offset": "ok"}, ("x",), UNSUPPORTED),
    ("gi_offset_on_hx_x", {"layout": HX_X, "offset": "ok"}, ("gi",), UNSUPPORTED),
]

# (id, descriptor overrides, the non-NULL members of TempChainBwd (+ "n_up=<k>"; d_arg is added for a decay unless "no_d_arg"), expected)
BWD_ROUTES = [
    ("decay_without_d_arg", {"decay": "ok"}, ("dgi", "dgh", "no_d_arg"), BADARG),
    ("d_arg_without_decay", {}, ("dgi", "dgh", "d_arg"), BADARG),
    ("d_arg_without_decay_offset", {"offset": "ok", "layout": BX}, ("dgi", "dgh", "d_arg"), BADARG),
    ("d_state_without_offset", {}, ("dgi", "dgh", "d_state"), BADARG),
    ("d_state", {"offset": "ok", "layout": BX}, ("dgi", "dgh", "d_state"), OK),
    ("d_state_g4_decay", {"offset": "ok", "layout": BX, "decay": "ok"}, ("g4", "d_state"), OK),
    ("g4", {}, ("g4",), OK),
    ("g4_with_dgi", {}, ("g4", "dgi"), BADARG),
    ("g4_with_dgh", {}, ("g4", "dgh"), BADARG),
    ("g4_with_dgi_decay", {"decay": "ok"}, ("g4", "dgi"), BADARG),
    ("g4_with_dgh_offset", {"offset": "ok", "layout": BX}, ("g4", "dgh"), BADARG),
    ("n_up_negative", {}, ("dgi", "dgh", "n_up=-1", "up"), BADARG),
    ("n_up_9", {}, ("dgi", "dgh", "n_up=9", "up"), BADARG),
    ("n_up_without_up", {}, ("dgi", "dgh", "n_up=1"), BADARG),
    ("n_up_8", {}, ("dgi", "dgh", "n_up=8", "up"), OK),
    ("g4_type1", {"variant": TYPE1}, ("g4",), UNSUPPORTED),
    ("gates_type1", {"variant": TYPE1}, ("dgi", "dgh"), OK),
    ("keys_on_f32", {}, ("g4", "row_keys", "col_keys"), UNSUPPORTED),
    ("row_keys_on_bx", {"layout": BX}, ("g4", "row_keys"), UNSUPPORTED),
    ("col_keys_on_bx_decay", {"layout": BX, "decay": "ok"}, ("g4", "col_keys"), UNSUPPORTED),
    ("keys_on_hx", {"layout": HX}, ("g4", "row_keys", "col_keys"), OK),
    ("keys_on_hx_x_decay", {"layout": HX_X, "decay": "ok"}, ("g4", "row_keys", "col_keys"), OK),
    ("keys_type1", {"layout": HX, "variant": TYPE1}, ("g4", "row_keys", "col_keys"), UNSUPPORTED),
    ("keys_with_offset", {"offset": "ok", "layout": BX}, ("g4", "row_keys", "col_keys"), UNSUPPORTED),
    ("keys_without_g4", {"layout": HX}, ("dgi", "dgh", "row_keys", "col_keys"), BADARG),      # stricter: the split entry ignored them
    ("row_keys_without_g4_decay", {"layout": HX, "decay": "ok"}, ("dgi", "dgh", "row_keys"), BADARG),
]

_DUMMY = ctypes.create_string_buffer(256)
PTR = ctypes.addressof(_DUMMY)                  # a valid host address; an empty chain reads through none of its pointers
_UP = (_lib.c_vp * _lib.CHAIN_MAX_UP)(*[PTR] * _lib.CHAIN_MAX_UP)


def descriptor(d=16, variant=TORCH, n_rnn=1, max_steps=1, layout=F32, decay=None, offset=None):
    c = _lib.TempGruChain()
    c.d, c.variant, c.n_panels, c.n_steps, c.max_steps, c.n_rnn, c.pack_layout = d, variant, 0, 0, max_steps, n_rnn, layout
    for i in range(min(n_rnn, _lib.CHAIN_MAX_RNN)):
        c.packed[i], c.b_hh[i] = PTR, PTR
    keep = []
    if decay:
        cd = _lib.TempChainDecay()
        for i in range(min(n_rnn, _lib.CHAIN_MAX_RNN)):
            cd.wb[i] = None if decay == "null_wb" and i == n_rnn - 1 else PTR
        c.decay = ctypes.pointer(cd)
        keep.append(cd)
    if offset:
        co = _lib.TempChainOffset()
        co.table, co.index, co.n_rows = (None if offset == "null_table" else PTR), PTR, (0 if offset == "no_rows" else 3)
        c.offset = ctypes.pointer(co)
        keep.append(co)
    return c, keep


def run_fwd(desc, members):
    c, keep = descriptor(**desc)
    io = _lib.TempChainFwd()
    io.h_out, io.saved = PTR, PTR
    if "gi" in members:
        io.gi = PTR
    if "x" in members:
        io.x, io.x_index, io.b_ih = PTR, PTR, ctypes.cast(_UP, ctypes.c_void_p)
    return _lib.load().temp_gru_chain_fwd(ctypes.byref(c), ctypes.byref(io), None)


def run_bwd(desc, members):
    c, keep = descriptor(**desc)
    io = _lib.TempChainBwd()
    io.saved = PTR
    for m in members:
        if m.startswith("n_up="):
            io.n_up = int(m[5:])
        elif m == "up":
            io.up = ctypes.cast(_UP, ctypes.c_void_p)
        elif m != "no_d_arg":
            setattr(io, m, PTR)
    if desc.get("decay") and "no_d_arg" not in members:
        io.d_arg = PTR
    return _lib.load().temp_gru_chain_bwd(ctypes.byref(c), ctypes.byref(io), None)


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("name,desc,want", DESCRIPTOR, ids=_ids(DESCRIPTOR))
def test_descriptor_rules_fwd(name, desc, want):
    assert run_fwd(desc, ("gi",)) == want


@pytest.mark.parametrize("name,desc,want", DESCRIPTOR, ids=_ids(DESCRIPTOR))
def test_descriptor_rules_bwd(name, desc, want):
    assert run_bwd(desc, ("dgi", "dgh")) == want
    if desc.get("variant", TORCH) == TORCH:
        assert run_bwd(desc, ("g4",)) == want


@pytest.mark.parametrize("name,desc,members,want", FWD_ROUTES, ids=_ids(FWD_ROUTES))
def test_route_rules_fwd(name, desc, members, want):
    assert run_fwd(desc, members) == want


@pytest.mark.parametrize("name,desc,members,want", BWD_ROUTES, ids=_ids(BWD_ROUTES))
def test_route_rules_bwd(name, desc, members, want):
    assert run_bwd(desc, members) == want


def test_zero_initialised_descriptor_tail_means_fixed_lambda_and_no_offset():
    """decay / offset are the last members: a descriptor filled the way a caller of the earlier layout filled it leaves them NULL."""
    names = [f[0] for f in _lib.TempGruChain._fields_]
    assert names[-2:] == ["decay", "offset"]
    c, _ = descriptor()
    assert not c.decay and not c.offset
