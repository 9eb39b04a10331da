"""The refresh of a patch graph (dagl_graph_refresh*, csrc/graph_refresh.hip) on fake pointers: every call below is rejected before
anything reaches the device, as in test_abi_graph_from_lists_host.py.  The entries came in without an ABI bump: found by symbol."""
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE = (2, 24, 20)
ROWS = 2 * 6 * 5          # B L
E, MAXDEG = 480, 8
_ALWAYS = ["wq_rows", "x_rows", "row_off", "row_off_out", "status_out"]
_WITH_EDGES = ["key", "key_out", "weight_out", "score_out"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, ws=_WS, ws_bytes=1 << 40, null=("tau",), shape=SHAPE, edges=E, max_row_edges=MAXDEG, radius=1, k=0, scale=10.0, flags=0,
          capacity=1 << 40):
    p = lambda n: None if n in null else _FAKE
    B, H, W = shape
    return lib.dagl_graph_refresh(None, B, H, W, p("wq_rows"), p("x_rows"), p("row_off"), p("key"), edges, max_row_edges, radius, p("tau"),
                                  k, scale, flags, p("row_off_out"), p("key_out"), p("weight_out"), p("score_out"), capacity,
                                  p("status_out"), ws, ws_bytes)


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_graph_refresh_max_candidates", "dagl_graph_refresh_workspace_bytes", "dagl_graph_refresh"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert len(_lib.SIGNATURES["dagl_graph_refresh"][1]) == 23 and len(_lib.SIGNATURES["dagl_graph_refresh_workspace_bytes"][1]) == 5
    assert re.search(r"dagl_graph_refresh\*[^.]*without a bump", header)
    assert lib.dagl_graph_refresh_max_candidates() >= 2048               # 64-key lists at radius 2


@pytest.mark.parametrize("name", _ALWAYS + _WITH_EDGES)
def test_null_pointers(lib, name):
    for tau in ((), ("tau",)):
        assert _call(lib, null=(name,) + tau) == -1
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, null=(name,) + tau, ws_bytes=0) == -1          # ... before the workspace is looked at


def test_arrays_may_be_null_without_edges(lib):
    assert _call(lib, null=tuple(_WITH_EDGES) + ("tau",), edges=0, max_row_edges=0, capacity=0, ws_bytes=0) == -2      # as far as the workspace
    for name in _ALWAYS:
        assert _call(lib, null=tuple(_WITH_EDGES) + (name,), edges=0, capacity=0) == -1


@pytest.mark.parametrize("radius", [-1, 9])
def test_radius_outside_0_8(lib, radius):
    assert _call(lib, radius=radius, max_row_edges=1) == -1
    assert b"radius" in lib.dagl_last_error()
    assert lib.dagl_graph_refresh_workspace_bytes(*SHAPE, E, radius) == 0


def test_radius_0_and_8_pass_the_check(lib):
    assert _call(lib, radius=0, ws_bytes=0) == -2 and _call(lib, radius=8, max_row_edges=4, ws_bytes=0) == -2


def test_k_scale_max_row_edges_flags(lib):
    assert _call(lib, k=-1) == -1 and b"k=-1" in lib.dagl_last_error()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(lib, scale=scale) == -1 and b"scale" in lib.dagl_last_error()
    assert _call(lib, max_row_edges=-1) == -1 and b"max_row_edges" in lib.dagl_last_error()
    assert _call(lib, flags=0x8) == -1 and b"flags" in lib.dagl_last_error()
    assert _call(lib, flags=0x7, ws_bytes=0) == -2                       # edges-only, keep-all, block rows: the three known bits


def test_candidate_cap(lib):
    from dagl_amd import _lib
    cap = lib.dagl_graph_refresh_max_candidates()
    for radius in (0, 1, 2):
        w2 = (2 * radius + 1) ** 2
        fits = cap // w2
        assert _call(lib, radius=radius, max_row_edges=fits, ws_bytes=0) == _lib.ERR_WORKSPACE       # at the cap (or the last below it)
        assert _call(lib, radius=radius, max_row_edges=fits + 1) == _lib.ERR_UNSUPPORTED
        err = lib.dagl_last_error().decode()
        assert str((fits + 1) * w2) in err and str(cap) in err, err
    assert _call(lib, radius=0, max_row_edges=cap, ws_bytes=0) == _lib.ERR_WORKSPACE                 # exactly at it
    assert _call(lib, radius=0, max_row_edges=cap + 1) == _lib.ERR_UNSUPPORTED                       # one above


def test_staged_candidates_must_fit_32_bits(lib):
    # 2^31 / 25 = 85 899 345.92: one edge fewer than the bound passes, at it the call is refused
    edge = -(-(1 << 31) // 25)
    assert _call(lib, edges=edge, radius=2) == -1 and b"2^31" in lib.dagl_last_error()
    assert _call(lib, edges=edge - 1, radius=2, ws_bytes=0) == -2
    assert _call(lib, edges=1 << 31, radius=0) == -1 and b"2^31" in lib.dagl_last_error()
    assert _call(lib, edges=(1 << 31) - 1, radius=0, ws_bytes=0) == -2
    assert _call(lib, edges=-1) == -1
    assert lib.dagl_graph_refresh_workspace_bytes(*SHAPE, edge, 2) == 0 and lib.dagl_graph_refresh_workspace_bytes(*SHAPE, edge - 1, 2) > 0


def test_misaligned_workspace(lib):
    assert _call(lib, ws=_WS + 8) == -1
    assert b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, ws=None) == -1
    assert b"aligned" in lib.dagl_last_error()


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_workspace_one_byte_short(lib, radius):
    from dagl_amd import _lib
    need = lib.dagl_graph_refresh_workspace_bytes(*SHAPE, E, radius)
    assert need >= ROWS * 4 + 3 * 4 * E * (2 * radius + 1) ** 2
    assert _call(lib, radius=radius, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_graph_refresh" in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err


def test_capacity_one_edge_short(lib):
    from dagl_amd import _lib
    # no rank cut: E (2 r + 1)^2
    assert _call(lib, capacity=E * 9 - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(E * 9) in err, err
    assert _call(lib, capacity=E * 9, ws_bytes=0) == _lib.ERR_WORKSPACE              # enough: the next check is the workspace's
    assert "workspace" in lib.dagl_last_error().decode()
    # a rank cut: B L k where that is smaller
    assert _call(lib, k=8, capacity=ROWS * 8 - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(ROWS * 8) in err, err
    assert _call(lib, k=8, capacity=ROWS * 8, ws_bytes=0) == _lib.ERR_WORKSPACE and "workspace" in lib.dagl_last_error().decode()
    # ... and E (2 r + 1)^2 where B L k is the larger one
    assert _call(lib, k=100, capacity=E * 9 - 1) == _lib.ERR_WORKSPACE and "capacity" in lib.dagl_last_error().decode()
    assert _call(lib, k=100, capacity=E * 9, ws_bytes=0) == _lib.ERR_WORKSPACE and "workspace" in lib.dagl_last_error().decode()
    # keep-all does not look at k
    assert _call(lib, k=8, flags=_lib.GRAPH_REFRESH_KEEP_ALL, capacity=E * 9 - 1) == _lib.ERR_WORKSPACE
    assert "capacity" in lib.dagl_last_error().decode()


def test_bad_shapes(lib):
    assert _call(lib, shape=(0, 24, 20)) == -1 and _call(lib, shape=(1, 24, 0)) == -1
    assert b"bad shape" in lib.dagl_last_error()
    assert _call(lib, shape=(4, 16384, 16384)) == -1
    assert b"row ids" in lib.dagl_last_error()


def test_planner(lib):
    planner = lib.dagl_graph_refresh_workspace_bytes
    by_edges = [planner(*SHAPE, e, 1) for e in (0, 1, 480, 4800, 1 << 20)]
    assert by_edges[0] > 0 and all(a <= b for a, b in zip(by_edges, by_edges[1:])) and by_edges[-1] > by_edges[0]
    by_radius = [planner(*SHAPE, 4800, r) for r in range(9)]
    assert all(a < b for a, b in zip(by_radius, by_radius[1:]))
    assert by_radius[2] >= 3 * 4 * 4800 * 25 + ROWS * 4                  # three staging arrays and the degrees
    by_batch = [planner(B, 24, 20, 480, 1) for B in (1, 2, 64, 1024)]
    assert all(a <= b for a, b in zip(by_batch, by_batch[1:])) and by_batch[-1] > by_batch[0]
    assert planner(0, 24, 20, 10, 1) == 0 and planner(1, 0, 20, 10, 1) == 0 and planner(1, 24, -3, 10, 1) == 0
    assert b"bad shape" in lib.dagl_last_error()
    assert planner(1, 24, 20, -1, 1) == 0
