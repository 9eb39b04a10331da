"""The ABI 409 entry points (dagl_graph_apply*, csrc/graph_apply.hip) on fake pointers: every call below is rejected before anything
reaches the device, as in test_abi_symbols.py."""
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE, EDGES = (2, 24, 20), 777


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _forward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES):
    p = lambda n: None if n in null else _FAKE
    return lib.dagl_graph_apply(None, *SHAPE, p("b2p"), p("row_off"), p("key"), p("weight"), edges, p("out"), ws, ws_bytes)


def _backward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES):
    p = lambda n: None if n in null else _FAKE
    return lib.dagl_graph_apply_backward(None, *SHAPE, p("b2p"), p("row_off"), p("key"), p("weight"), edges, p("d_out"), p("col_off"),
                                         p("src_row"), p("perm"), p("d_b2p"), p("d_weight"), ws, ws_bytes)


def test_version_and_segment(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION >= 409
    assert lib.dagl_graph_apply_segment() > 0


@pytest.mark.parametrize("name", ["out", "b2p", "row_off", "key", "weight"])
def test_forward_null_pointers(lib, name):
    assert _forward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()


@pytest.mark.parametrize("name", ["b2p", "row_off", "d_out", "col_off", "perm"])
def test_backward_null_pointers(lib, name):
    assert _backward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()


def test_misaligned_workspace(lib):
    for call in (_forward, _backward):
        assert call(lib, ws=_WS + 8) == -1
        assert b"aligned" in lib.dagl_last_error()
        assert call(lib, ws=None) == -1
        assert b"aligned" in lib.dagl_last_error()


def test_workspace_one_byte_short(lib):
    from dagl_amd import _lib
    for call, planner in ((_forward, lib.dagl_graph_apply_workspace_bytes), (_backward, lib.dagl_graph_apply_backward_workspace_bytes)):
        need = planner(*SHAPE, EDGES)
        assert need > 0
        assert call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
        err = lib.dagl_last_error().decode()
        assert "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    # the planners: more edges need more partial rows, the backward also holds the d V rows; bad shapes and edge counts give 0
    seg = lib.dagl_graph_apply_segment()
    fwd = lib.dagl_graph_apply_workspace_bytes
    assert fwd(*SHAPE, EDGES + 64 * seg) > fwd(*SHAPE, EDGES) >= fwd(*SHAPE, 0) > 0
    assert lib.dagl_graph_apply_backward_workspace_bytes(*SHAPE, EDGES) >= fwd(*SHAPE, EDGES) + 2 * 480 * 784 * 4
    assert fwd(0, 24, 20, 5) == 0 and fwd(*SHAPE, -1) == 0 and fwd(*SHAPE, 1 << 31) == 0
    assert b"total_edges" in lib.dagl_last_error()


def test_bad_shape_and_edge_count(lib):
    assert lib.dagl_graph_apply(None, 0, 24, 20, _FAKE, _FAKE, _FAKE, _FAKE, 5, _FAKE, _WS, 1 << 40) == -1
    assert _forward(lib, edges=-1) == -1 and _backward(lib, edges=1 << 31) == -1
    # an empty graph needs neither keys nor weights; d_weight alone needs no transposed CSR
    assert _forward(lib, null=("key", "weight"), edges=0, ws_bytes=0) == -2
    assert _backward(lib, null=("d_b2p", "col_off", "src_row", "perm"), ws_bytes=0) == -2
