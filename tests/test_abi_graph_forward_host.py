"""The fused forward on a given patch graph (dagl_graph_forward*, csrc/graph_forward.hip) on fake pointers: every call below is rejected
before anything reaches the device, as in test_abi_graph_attend_host.py.  The entry came in without an ABI bump: it is found by symbol."""
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE, EDGES = (2, 24, 20), 777
_POINTERS = ["wq_rows", "x_rows", "b2p", "row_off", "key", "out"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _forward(lib, ws=_WS, ws_bytes=1 << 40, null=(), edges=EDGES, shape=SHAPE, scale=10.0, flags=0, fake=_FAKE):
    p = lambda n: None if n in null else fake
    return lib.dagl_graph_forward(None, *shape, p("wq_rows"), p("x_rows"), p("b2p"), p("row_off"), p("key"), edges, p("tau"), scale, flags,
                                  p("out"), ws, ws_bytes)


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412


def test_symbols_in_the_header_and_the_table():
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_graph_forward_workspace_bytes", "dagl_graph_forward"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert len(_lib.SIGNATURES["dagl_graph_forward"][1]) == 16 and len(_lib.SIGNATURES["dagl_graph_forward_workspace_bytes"][1]) == 4
    assert "detected by symbol" in header or "detects them by symbol" in header


@pytest.mark.parametrize("name", _POINTERS)
def test_null_pointers(lib, name):
    assert _forward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error()
    assert _forward(lib, null=(name,), ws_bytes=0) == -1              # ... before the workspace is looked at


def test_misaligned_operands(lib):
    assert _forward(lib, ws=_WS + 8) == -1
    assert b"256-byte aligned" in lib.dagl_last_error()
    assert _forward(lib, ws=None) == -1
    assert b"aligned" in lib.dagl_last_error()
    assert _forward(lib, fake=_FAKE + 4) == -1                        # feature rows and value map are read as float4
    assert b"16-byte aligned" in lib.dagl_last_error()


def test_workspace_one_byte_short(lib):
    from dagl_amd import _lib
    need = lib.dagl_graph_forward_workspace_bytes(*SHAPE, EDGES)
    assert need > 0
    assert _forward(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_graph_forward" in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err


def test_planner(lib):
    seg = lib.dagl_graph_apply_segment()
    planner = lib.dagl_graph_forward_workspace_bytes
    B, H, W = SHAPE
    rows = B * (-(-H // 4)) * (-(-W // 4))
    sizes = [planner(*SHAPE, e) for e in (0, 1, EDGES, EDGES + 64 * seg, 1 << 20, (1 << 31) - 1)]
    assert sizes[0] >= rows * 784 * 4 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[3] > sizes[2] and sizes[5] > sizes[4]
    # a partial row and a (max, sum) slot per segment on top of the aggregated rows
    assert planner(*SHAPE, 64 * seg) >= rows * 784 * 4 + 64 * (784 * 4 + 12)
    assert planner(4, 24, 20, EDGES) > planner(*SHAPE, EDGES)
    assert planner(0, 24, 20, 5) == 0 and planner(*SHAPE, -1) == 0 and planner(*SHAPE, 1 << 31) == 0
    assert b"total_edges" in lib.dagl_last_error()


def test_bad_shape_edge_count_scale_and_flags(lib):
    assert _forward(lib, shape=(0, 24, 20)) == -1 and _forward(lib, shape=(1, 24, 0)) == -1
    assert b"bad shape" in lib.dagl_last_error()
    assert _forward(lib, edges=-1) == -1 and _forward(lib, edges=1 << 31) == -1
    assert b"total_edges" in lib.dagl_last_error()
    assert _forward(lib, scale=0.0) == -1 and _forward(lib, scale=float("nan")) == -1 and _forward(lib, scale=float("inf")) == -1
    assert b"scale" in lib.dagl_last_error()
    assert _forward(lib, flags=2) == -1
    assert b"flags" in lib.dagl_last_error()
    assert _forward(lib, flags=1, ws_bytes=0) == -2                   # bit 0 is the edges-only normalisation


def test_nullable_arguments(lib):
    """What may be null gets as far as the last check before the device, the workspace size (-2)."""
    assert _forward(lib, null=("tau",), ws_bytes=0) == -2              # no margin
    assert _forward(lib, null=("key",), edges=0, ws_bytes=0) == -2     # an empty graph needs no keys
    assert _forward(lib, null=("key", "tau"), edges=0, ws_bytes=0) == -2
