"""The ABI 412 entry points (dagl_graph_attend*, csrc/graph_attend.hip) on fake pointers: every call below is rejected before anything
reaches the device, as in test_abi_graph_apply_host.py."""
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


def _forward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES, shape=SHAPE, scale=10.0, flags=0, fake=_FAKE):
    p = lambda n: None if n in null else fake
    return lib.dagl_graph_attend(None, *shape, p("wq_rows"), p("x_rows"), p("row_off"), p("key"), edges, p("tau"), scale, flags,
                                 p("score"), p("weight"), ws, ws_bytes)


def _backward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES, shape=SHAPE, scale=10.0, flags=0, fake=_FAKE):
    p = lambda n: None if n in null else fake
    return lib.dagl_graph_attend_backward(None, *shape, p("wq_rows"), p("x_rows"), p("row_off"), p("key"), edges, p("tau"), scale, flags,
                                          p("score"), p("weight"), p("d_weight"), p("col_off"), p("src_row"), p("perm"), p("d_wq_rows"),
                                          p("d_x_rows"), p("d_tau"), ws, ws_bytes)


def test_version(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412


@pytest.mark.parametrize("name", ["wq_rows", "x_rows", "row_off", "key", "score", "weight"])
def test_forward_null_pointers(lib, name):
    assert _forward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()


@pytest.mark.parametrize("name", ["wq_rows", "x_rows", "row_off", "key", "score", "weight", "d_weight", "col_off", "src_row", "perm"])
def test_backward_null_pointers(lib, name):
    assert _backward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()


def test_misaligned_operands(lib):
    for call in (_forward, _backward):
        assert call(lib, ws=_WS + 8) == -1
        assert b"aligned" in lib.dagl_last_error()
        assert call(lib, ws=None) == -1
        assert b"aligned" in lib.dagl_last_error()
        assert call(lib, fake=_FAKE + 4) == -1             # the feature rows are read as float4
        assert b"16-byte aligned" in lib.dagl_last_error()


def test_workspace_one_byte_short(lib):
    from dagl_amd import _lib
    for call, planner in ((_forward, lib.dagl_graph_attend_workspace_bytes), (_backward, lib.dagl_graph_attend_backward_workspace_bytes)):
        need = planner(*SHAPE, EDGES)
        assert need > 0
        assert call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
        err = lib.dagl_last_error().decode()
        assert "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err


def test_planners_grow_with_the_graph(lib):
    seg = lib.dagl_graph_apply_segment()
    for planner in (lib.dagl_graph_attend_workspace_bytes, lib.dagl_graph_attend_backward_workspace_bytes):
        sizes = [planner(*SHAPE, e) for e in (0, 1, EDGES, EDGES + 64 * seg, 1 << 20, (1 << 31) - 1)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[3] > sizes[2] and sizes[5] > sizes[4]
        assert planner(4, 24, 20, EDGES) > planner(*SHAPE, EDGES)            # per-row slots
        assert planner(0, 24, 20, 5) == 0 and planner(*SHAPE, -1) == 0 and planner(*SHAPE, 1 << 31) == 0
        assert b"total_edges" in lib.dagl_last_error()
    # the backward holds d S and the products' partial rows (196 floats per segment) on top of the rows of the edges
    assert lib.dagl_graph_attend_backward_workspace_bytes(*SHAPE, 64 * seg) >= 64 * seg * 8 + 64 * 196 * 4


def test_bad_shape_edge_count_scale_and_flags(lib):
    for call in (_forward, _backward):
        assert call(lib, shape=(0, 24, 20)) == -1 and call(lib, shape=(1, 24, 0)) == -1
        assert b"bad shape" in lib.dagl_last_error()
        assert call(lib, edges=-1) == -1 and call(lib, edges=1 << 31) == -1
        assert b"total_edges" in lib.dagl_last_error()
        assert call(lib, scale=0.0) == -1 and call(lib, scale=float("nan")) == -1 and call(lib, scale=float("inf")) == -1
        assert b"scale" in lib.dagl_last_error()
        assert call(lib, flags=2) == -1
        assert b"flags" in lib.dagl_last_error()
        assert call(lib, flags=1, ws_bytes=0) == -2                          # bit 0 is the edges-only normalisation


def test_nullable_arguments(lib):
    """What may be null gets as far as the workspace check (-2), what may not is refused by name (-1)."""
    # no margin; an empty graph needs no edge arrays
    assert _forward(lib, null=("tau",), ws_bytes=0) == -2
    assert _forward(lib, null=("key", "score", "weight"), edges=0, ws_bytes=0) == -2
    assert _backward(lib, null=("key", "score", "weight", "d_weight", "src_row", "perm"), edges=0, ws_bytes=0) == -2
    # every d_* output is nullable; the transposed CSR is required only with d_x_rows
    for null in (("d_wq_rows",), ("d_x_rows", "col_off", "src_row", "perm"), ("d_tau",), ("d_tau", "tau"),
                 ("d_wq_rows", "d_x_rows", "d_tau", "col_off", "src_row", "perm")):
        assert _backward(lib, null=null, ws_bytes=0) == -2, null
    assert _backward(lib, null=("col_off",)) == -1
    assert b"transposed" in lib.dagl_last_error()
    assert _backward(lib, null=("tau",)) == -1                               # d tau of a call without a margin
    assert b"d_tau" in lib.dagl_last_error()
