"""The patch graph from a forward's neighbour lists (dagl_graph_from_lists*, csrc/graph_lists.hip) on fake pointers: every call below is
rejected before anything reaches the device, as in test_abi_graph_forward_host.py.  The entry came in without an ABI bump: it is found
by symbol."""
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE, WIDTH = (2, 24, 20), 8
ROWS = 2 * 6 * 5          # B L
_REQUIRED = ["nb_idx", "nb_wgt", "nb_cnt", "row_off", "key", "weight"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, ws=_WS, ws_bytes=1 << 40, null=("nb_s", "score"), shape=SHAPE, width=WIDTH, capacity=None):
    p = lambda n: None if n in null else _FAKE
    B, H, W = shape
    if capacity is None:
        capacity = B * (-(-H // 4)) * (-(-W // 4)) * max(width, 0)
    return lib.dagl_graph_from_lists(None, B, H, W, width, p("nb_idx"), p("nb_wgt"), p("nb_s"), p("nb_cnt"), p("row_off"), p("key"),
                                     p("weight"), p("score"), capacity, ws, ws_bytes)


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_graph_from_lists_workspace_bytes", "dagl_graph_from_lists"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert len(_lib.SIGNATURES["dagl_graph_from_lists"][1]) == 16 and len(_lib.SIGNATURES["dagl_graph_from_lists_workspace_bytes"][1]) == 3
    assert re.search(r"dagl_graph_from_lists\*[^.]*without a bump", header)


@pytest.mark.parametrize("name", _REQUIRED)
def test_null_pointers(lib, name):
    for with_scores in (False, True):
        null = (name,) + (() if with_scores else ("nb_s", "score"))
        assert _call(lib, null=null) == -1
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, null=null, ws_bytes=0) == -1               # ... before the workspace is looked at


def test_scores_in_and_out_go_together(lib):
    assert _call(lib, null=("nb_s",)) == -1
    assert b"nb_s and score_out" in lib.dagl_last_error()
    assert _call(lib, null=("score",)) == -1
    assert b"nb_s and score_out" in lib.dagl_last_error()
    assert _call(lib, null=(), ws_bytes=0) == -2                     # both given: as far as the workspace size
    assert _call(lib, ws_bytes=0) == -2                              # neither


@pytest.mark.parametrize("width", [0, 65, -1])
def test_width_outside_the_lists(lib, width):
    assert _call(lib, width=width, capacity=1 << 20) == -1
    assert b"width" in lib.dagl_last_error()


def test_widths_1_and_64_pass_the_check(lib):
    assert _call(lib, width=1, ws_bytes=0) == -2 and _call(lib, width=64, ws_bytes=0) == -2


def test_misaligned_workspace(lib):
    assert _call(lib, ws=_WS + 8) == -1
    assert b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, ws=None) == -1
    assert b"aligned" in lib.dagl_last_error()


def test_workspace_one_byte_short(lib):
    from dagl_amd import _lib
    need = lib.dagl_graph_from_lists_workspace_bytes(*SHAPE)
    assert need >= ROWS * 4
    assert _call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_graph_from_lists" in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err


def test_capacity_one_edge_short(lib):
    from dagl_amd import _lib
    assert _call(lib, capacity=ROWS * WIDTH - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(ROWS * WIDTH) in err, err
    assert _call(lib, capacity=ROWS * WIDTH, ws_bytes=0) == _lib.ERR_WORKSPACE       # enough: the next check is the workspace's
    assert "workspace" in lib.dagl_last_error().decode()


def test_too_many_slots_for_32_bit_edge_ids(lib):
    # B H W = 2^29 keys pass the row-id check; L = 2^24 per image, B L width = 2^31
    shape = (2, 16384, 16384)
    assert _call(lib, shape=shape, width=64, capacity=1 << 40) == -1
    assert b"2^31" in lib.dagl_last_error()
    assert _call(lib, shape=shape, width=63, capacity=1 << 40, ws_bytes=0) == -2     # one slot per row fewer: below 2^31


def test_bad_shapes(lib):
    assert _call(lib, shape=(0, 24, 20), capacity=1 << 20) == -1 and _call(lib, shape=(1, 24, 0), capacity=1 << 20) == -1
    assert b"bad shape" in lib.dagl_last_error()
    assert _call(lib, shape=(4, 16384, 16384), capacity=1 << 40) == -1
    assert b"row ids" in lib.dagl_last_error()


def test_planner(lib):
    planner = lib.dagl_graph_from_lists_workspace_bytes
    sizes = [planner(B, 24, 20) for B in (1, 2, 3, 64, 1024)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 1024 * 30 * 4                                # the [B L] int32 degrees
    assert planner(0, 24, 20) == 0 and planner(1, 0, 20) == 0 and planner(1, 24, -3) == 0
    assert b"bad shape" in lib.dagl_last_error()
