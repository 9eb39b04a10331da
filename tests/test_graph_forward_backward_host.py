"""The training pair of the fused forward on a given patch graph (dagl_graph_forward_train, dagl_graph_forward_backward*,
csrc/graph_forward.hip) on fake pointers: every call below is rejected before anything reaches the device, as in
test_abi_graph_forward_host.py.  The entries came in without an ABI bump: they are found by symbol."""
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE, EDGES = (2, 24, 20), 777
_TRAIN_POINTERS = ["wq_rows", "x_rows", "b2p", "row_off", "key", "out", "row_max_out", "row_sum_out"]
_BACKWARD_POINTERS = ["wq_rows", "x_rows", "b2p", "row_off", "key", "row_max", "row_sum", "d_out"]
_GRADS = ("d_wq_rows", "d_x_rows", "d_tau", "d_b2p")


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _train(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES, shape=SHAPE, scale=10.0, flags=0, fake=_FAKE):
    p = lambda n: None if n in null else fake
    return lib.dagl_graph_forward_train(None, *shape, p("wq_rows"), p("x_rows"), p("b2p"), p("row_off"), p("key"), edges, p("tau"), scale,
                                        flags, p("out"), p("row_max_out"), p("row_sum_out"), ws, ws_bytes)


def _backward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES, shape=SHAPE, scale=10.0, flags=0, fake=_FAKE, at=None):
    """``null``: the arguments passed as NULL; ``at``: {argument: address} for single pointers."""
    p = lambda n: None if n in null else (at or {}).get(n, fake)
    return lib.dagl_graph_forward_backward(None, *shape, p("wq_rows"), p("x_rows"), p("b2p"), p("row_off"), p("key"), edges, p("tau"), scale,
                                           flags, p("row_max"), p("row_sum"), p("d_out"), p("col_off"), p("src_row"), p("perm"),
                                           p("d_wq_rows"), p("d_x_rows"), p("d_tau"), p("d_b2p"), ws, ws_bytes)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name, n_args in (("dagl_graph_forward_train", 18), ("dagl_graph_forward_backward_workspace_bytes", 4),
                         ("dagl_graph_forward_backward", 25)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert lib.dagl_version() == _lib.ABI_VERSION == 412               # no bump: found by symbol


@pytest.mark.parametrize("name", _TRAIN_POINTERS)
def test_train_null_pointers(lib, name):
    assert _train(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()
    assert _train(lib, null=(name,), ws_bytes=0) == -1                 # ... before the workspace is looked at


@pytest.mark.parametrize("name", _BACKWARD_POINTERS)
def test_backward_null_pointers(lib, name):
    assert _backward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()
    assert _backward(lib, null=(name,), ws_bytes=0) == -1


def test_misaligned_operands(lib):
    assert _train(lib, fake=_FAKE + 4) == -1 and b"16-byte aligned" in lib.dagl_last_error()
    assert _train(lib, ws=_WS + 8) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _backward(lib, ws=_WS + 8) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _backward(lib, ws=None) == -1 and b"aligned" in lib.dagl_last_error()
    for name in ("d_wq_rows", "d_x_rows"):
        assert _backward(lib, at={name: _FAKE + 4}, ws_bytes=0) == -1
        assert b"gradient rows must be 16-byte aligned" in lib.dagl_last_error()
    for name in ("b2p", "d_b2p"):
        assert _backward(lib, at={name: _FAKE + 8}, ws_bytes=0) == -1
        assert b"maps must be 16-byte aligned" in lib.dagl_last_error()
    for name in ("wq_rows", "x_rows"):
        assert _backward(lib, at={name: _FAKE + 4}, ws_bytes=0) == -1
        assert b"feature rows must be 16-byte aligned" in lib.dagl_last_error()


def test_d_tau_needs_tau(lib):
    assert _backward(lib, null=("tau",), ws_bytes=0) == -1
    assert b"d_tau asked for without tau" in lib.dagl_last_error()
    assert _backward(lib, null=("tau", "d_tau"), ws_bytes=0) == -2     # without d_tau: as far as the workspace size


@pytest.mark.parametrize("grad", ["d_x_rows", "d_b2p"])
@pytest.mark.parametrize("missing", ["col_off", "src_row", "perm"])
def test_transposed_csr_is_required_by_the_column_gradients(lib, grad, missing):
    other = "d_b2p" if grad == "d_x_rows" else "d_x_rows"
    assert _backward(lib, null=(missing, other), ws_bytes=0) == -1
    assert b"transposed CSR" in lib.dagl_last_error()
    # neither wanted: the transposed CSR may be missing altogether
    assert _backward(lib, null=("col_off", "src_row", "perm", "d_x_rows", "d_b2p"), ws_bytes=0) == -2


def test_workspace_one_byte_short(lib):
    from dagl_amd import _lib
    for call, planner, who in ((_train, lib.dagl_graph_forward_workspace_bytes, "dagl_graph_forward_train"),
                               (_backward, lib.dagl_graph_forward_backward_workspace_bytes, "dagl_graph_forward_backward")):
        need = planner(*SHAPE, EDGES)
        assert need > 0
        assert call(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
        err = lib.dagl_last_error().decode()
        assert who in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err


def test_planner(lib):
    seg = lib.dagl_graph_apply_segment()
    planner = lib.dagl_graph_forward_backward_workspace_bytes
    B, H, W = SHAPE
    rows, cols = B * (-(-H // 4)) * (-(-W // 4)), B * H * W
    sizes = [planner(*SHAPE, e) for e in (0, 1, EDGES, EDGES + 64 * seg, 1 << 20, (1 << 31) - 1)]
    # dAgg and the d V rows whatever the edge count; then it grows with E: a partial row and three sums per segment, three floats per edge
    assert sizes[0] >= (rows + cols) * 784 * 4 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] > sizes[2] and sizes[4] > sizes[3] and sizes[5] > sizes[4]
    assert planner(*SHAPE, 64 * seg) >= (rows + cols) * 784 * 4 + 64 * (784 * 4 + 24) + 64 * seg * 12
    assert planner(4, 24, 20, EDGES) > planner(*SHAPE, EDGES)
    assert planner(0, 24, 20, 5) == 0 and planner(*SHAPE, -1) == 0 and planner(*SHAPE, 1 << 31) == 0
    assert b"total_edges" in lib.dagl_last_error()


def test_bad_shape_edge_count_scale_and_flags(lib):
    for call in (_train, _backward):
        assert call(lib, shape=(0, 24, 20)) == -1 and call(lib, shape=(1, 24, 0)) == -1
        assert b"bad shape" in lib.dagl_last_error()
        assert call(lib, edges=-1) == -1 and call(lib, edges=1 << 31) == -1
        assert b"total_edges" in lib.dagl_last_error()
        assert call(lib, scale=0.0) == -1 and call(lib, scale=float("nan")) == -1
        assert b"scale" in lib.dagl_last_error()
        assert call(lib, flags=2) == -1
        assert b"flags" in lib.dagl_last_error()
        assert call(lib, flags=1, ws_bytes=0) == -2                    # bit 0 is the edges-only normalisation


def test_nullable_arguments(lib):
    """What may be null gets as far as the last check before the device, the workspace size (-2)."""
    assert _train(lib, null=("tau",), ws_bytes=0) == -2
    assert _train(lib, null=("key", "tau"), edges=0, ws_bytes=0) == -2
    assert _backward(lib, null=("tau", "d_tau"), ws_bytes=0) == -2
    assert _backward(lib, null=("key", "src_row", "perm"), edges=0, ws_bytes=0) == -2       # an empty graph: offsets alone
    for left in _GRADS:                                                # every gradient on its own
        gone = tuple(n for n in _GRADS if n != left)
        assert _backward(lib, null=gone, ws_bytes=0) == -2, left
    assert _backward(lib, null=_GRADS, ws_bytes=0) == -2
