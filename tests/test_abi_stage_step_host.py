"""The step of a whole CES stage (dagl_graph_stage_step*, dagl_ces_stage_fold_mix; csrc/graph_refresh.hip, csrc/aggregate.hip) on fake
pointers: every call below is rejected before anything reaches the device, as in test_abi_graph_refresh_host.py.  The entries came in
without an ABI bump: found by symbol."""
import ctypes as C
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE = (2, 24, 20)
ROWS = 4 * 2 * 6 * 5      # 4 B L
E, MAXDEG = 1920, 8
_TABLES = ["wq_rows4", "x_rows4", "b2p4"]
_ALWAYS = ["row_off", "x", "mix_w", "mix_b", "out", "status_out"]
_GRAPH = ["row_off_out", "key_out", "weight_out", "score_out"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _table(entries):
    return (C.c_void_p * 4)(*entries)


def _call(lib, ws=_WS, ws_bytes=1 << 40, null=("tau4",), entries=None, shape=SHAPE, edges=E, max_row_edges=MAXDEG, radius=1, k=0, scale=10.0,
          flags=0, capacity=1 << 40):
    """``null``: the arguments passed as NULL; ``entries``: {table: four values} in the place of four fake pointers."""
    entries = entries or {}
    p = lambda n: None if n in null else _FAKE
    t = lambda n: None if n in null else _table(entries.get(n, [_FAKE] * 4))
    B, H, W = shape
    return lib.dagl_graph_stage_step(None, B, H, W, t("wq_rows4"), t("x_rows4"), t("b2p4"), p("row_off"), p("key"), edges, max_row_edges,
                                     radius, t("tau4"), k, scale, flags, p("x"), p("mix_w"), p("mix_b"), p("out"), p("row_off_out"),
                                     p("key_out"), p("weight_out"), p("score_out"), capacity, p("status_out"), ws, ws_bytes)


def _fold_mix(lib, null=(), shape=SHAPE, agg=_FAKE):
    p = lambda n: None if n in null else _FAKE
    B, H, W = shape
    return lib.dagl_ces_stage_fold_mix(None, B, H, W, None if "agg" in null else agg, p("x"), p("mix_w"), p("mix_b"), p("out"))


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_ces_stage_fold_mix", "dagl_graph_stage_step_workspace_bytes", "dagl_graph_stage_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert len(_lib.SIGNATURES["dagl_graph_stage_step"][1]) == 28 and len(_lib.SIGNATURES["dagl_graph_stage_step_workspace_bytes"][1]) == 6
    assert len(_lib.SIGNATURES["dagl_ces_stage_fold_mix"][1]) == 9
    assert re.search(r"dagl_graph_stage_step\*[^.]*dagl_ces_stage_fold_mix[^.]*without a bump", header)


def test_the_call_passes_its_checks_as_far_as_the_workspace(lib):
    from dagl_amd import _lib
    assert _call(lib, ws_bytes=0) == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    assert _call(lib, null=(), ws_bytes=0) == _lib.ERR_WORKSPACE                                  # with tau
    assert _call(lib, null=tuple(_GRAPH) + ("tau4",), capacity=0, ws_bytes=0) == _lib.ERR_WORKSPACE      # the output alone


@pytest.mark.parametrize("name", _TABLES)
def test_pointer_tables(lib, name):
    assert _call(lib, null=(name, "tau4")) == -1 and b"null" in lib.dagl_last_error()
    for h in range(4):
        entries = [_FAKE] * 4
        entries[h] = None
        assert _call(lib, entries={name: entries}) == -1, (name, h)
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, entries={name: entries}, ws_bytes=0) == -1                              # ... before the workspace is looked at
        entries[h] = _FAKE + 8
        assert _call(lib, entries={name: entries}) == -1, (name, h)
        assert b"16-byte aligned" in lib.dagl_last_error()
    if name == "b2p4":
        assert b"b2p" in lib.dagl_last_error()


def test_tau_for_all_heads_or_none(lib):
    from dagl_amd import _lib
    assert _call(lib, entries={"tau4": [None] * 4}, null=(), ws_bytes=0) == _lib.ERR_WORKSPACE       # four null entries: no margin
    for given in ([_FAKE, None, None, None], [_FAKE, _FAKE, _FAKE, None], [None, _FAKE, _FAKE, _FAKE]):
        assert _call(lib, entries={"tau4": given}, null=()) == -1
        assert b"tau" in lib.dagl_last_error()


@pytest.mark.parametrize("name", _ALWAYS + ["key"])
def test_null_pointers(lib, name):
    for tau in ((), ("tau4",)):
        assert _call(lib, null=(name,) + tau) == -1
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, null=(name,) + tau, ws_bytes=0) == -1


def test_graph_outputs_all_or_none(lib):
    from dagl_amd import _lib
    for name in _GRAPH:
        assert _call(lib, null=(name, "tau4")) == -1 and b"null" in lib.dagl_last_error()
        only = tuple(n for n in _GRAPH if n != name) + ("tau4",)
        assert _call(lib, null=only) == -1 and b"null" in lib.dagl_last_error()
    # without edges the three edge arrays (and key) may be null, the offsets may not
    no_edges = dict(edges=0, max_row_edges=0, capacity=0, ws_bytes=0)
    assert _call(lib, null=("key", "key_out", "weight_out", "score_out", "tau4"), **no_edges) == _lib.ERR_WORKSPACE
    assert _call(lib, null=tuple(_GRAPH) + ("key", "tau4"), **no_edges) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("radius", [-1, 9])
def test_radius_outside_0_8(lib, radius):
    assert _call(lib, radius=radius, max_row_edges=1) == -1
    assert b"radius" in lib.dagl_last_error()
    assert lib.dagl_graph_stage_step_workspace_bytes(*SHAPE, E, radius, 1) == 0


def test_k_scale_max_row_edges_flags(lib):
    assert _call(lib, radius=0, ws_bytes=0) == -2 and _call(lib, radius=8, max_row_edges=4, ws_bytes=0) == -2
    assert _call(lib, k=-1) == -1 and b"k=-1" in lib.dagl_last_error()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(lib, scale=scale) == -1 and b"scale" in lib.dagl_last_error()
    assert _call(lib, max_row_edges=-1) == -1 and b"max_row_edges" in lib.dagl_last_error()
    assert _call(lib, flags=0x8) == -1 and b"flags" in lib.dagl_last_error()
    assert _call(lib, flags=0x7, ws_bytes=0) == -2


def test_candidate_cap(lib):
    from dagl_amd import _lib
    cap = lib.dagl_graph_refresh_max_candidates()
    for radius in (0, 1, 2):
        w2 = (2 * radius + 1) ** 2
        fits = cap // w2
        assert _call(lib, radius=radius, max_row_edges=fits, ws_bytes=0) == _lib.ERR_WORKSPACE
        assert _call(lib, radius=radius, max_row_edges=fits + 1) == _lib.ERR_UNSUPPORTED
        err = lib.dagl_last_error().decode()
        assert "dagl_graph_stage_step" in err and str((fits + 1) * w2) in err and str(cap) in err, err


def test_capacity_one_edge_short(lib):
    from dagl_amd import _lib
    assert _call(lib, capacity=E * 9 - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(E * 9) in err, err
    assert _call(lib, capacity=E * 9, ws_bytes=0) == _lib.ERR_WORKSPACE and "workspace" in lib.dagl_last_error().decode()
    # a rank cut: 4 B L k where that is smaller
    assert _call(lib, k=8, capacity=ROWS * 8 - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(ROWS * 8) in err, err
    assert _call(lib, k=8, capacity=ROWS * 8, ws_bytes=0) == _lib.ERR_WORKSPACE and "workspace" in lib.dagl_last_error().decode()
    assert _call(lib, k=8, flags=_lib.GRAPH_REFRESH_KEEP_ALL, capacity=E * 9 - 1) == _lib.ERR_WORKSPACE
    assert "capacity" in lib.dagl_last_error().decode()
    # the output alone does not look at it
    assert _call(lib, null=tuple(_GRAPH) + ("tau4",), capacity=0, ws_bytes=0) == _lib.ERR_WORKSPACE
    assert "workspace" in lib.dagl_last_error().decode()


@pytest.mark.parametrize("want_graph", [0, 1])
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_workspace_one_byte_short(lib, radius, want_graph):
    from dagl_amd import _lib
    need = lib.dagl_graph_stage_step_workspace_bytes(*SHAPE, E, radius, want_graph)
    assert need >= ROWS * 784 * 4 + want_graph * (ROWS * 4 + 3 * 4 * E * (2 * radius + 1) ** 2)
    null = ("tau4",) if want_graph else tuple(_GRAPH) + ("tau4",)
    assert _call(lib, null=null, radius=radius, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_graph_stage_step" in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    assert _call(lib, null=null, radius=radius, ws=_WS + 8) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, null=null, radius=radius, ws=None) == -1


def test_planner_and_shapes(lib):
    planner = lib.dagl_graph_stage_step_workspace_bytes
    # the rows of four heads: what the single-head planner says of 4 B images
    for want_graph in (0, 1):
        assert planner(*SHAPE, E, 1, want_graph) == lib.dagl_graph_step_workspace_bytes(4 * SHAPE[0], *SHAPE[1:], E, 1, want_graph)
    assert planner(*SHAPE, E, 1, 1) > planner(*SHAPE, E, 1, 0) > 0
    assert planner(0, 24, 20, 10, 1, 1) == 0 and planner(1, 0, 20, 10, 1, 1) == 0 and planner(1, 24, 20, -1, 1, 1) == 0
    assert _call(lib, shape=(0, 24, 20)) == -1 and b"bad shape" in lib.dagl_last_error()
    # 4 B H W must fit the row ids: a batch the single-head call would take
    assert lib.dagl_graph_step_workspace_bytes(1, 16384, 16384, 0, 1, 0) > 0
    assert _call(lib, shape=(1, 16384, 16384)) == -1 and b"row ids" in lib.dagl_last_error()
    assert planner(1, 16384, 16384, 0, 1, 0) == 0
    assert _call(lib, edges=1 << 31, radius=0) == -1 and b"2^31" in lib.dagl_last_error()


def test_stage_mix_refusals(lib):
    from dagl_amd import _lib
    assert "dagl_ces_stage_mix" in _lib.SIGNATURES
    call = lambda null=(), shape=SHAPE: lib.dagl_ces_stage_mix(None, *shape, *[None if n in null else _FAKE
                                                                                for n in ("cat", "x", "mix_w", "mix_b", "out")])
    for name in ("cat", "x", "mix_w", "mix_b", "out"):
        assert call(null=(name,)) == -1 and b"null" in lib.dagl_last_error() and b"dagl_ces_stage_mix" in lib.dagl_last_error()
    assert call(shape=(0, 24, 20)) == -1 and b"bad shape" in lib.dagl_last_error()
    assert call(shape=(65536, 4, 4)) == -1 and b"65535" in lib.dagl_last_error()


def test_fold_mix_refusals(lib):
    for name in ("agg", "x", "mix_w", "mix_b", "out"):
        assert _fold_mix(lib, null=(name,)) == -1
        assert b"null" in lib.dagl_last_error() and b"dagl_ces_stage_fold_mix" in lib.dagl_last_error()
    assert _fold_mix(lib, agg=_FAKE + 4) == -1 and b"16-byte aligned" in lib.dagl_last_error()
    assert _fold_mix(lib, shape=(0, 24, 20)) == -1 and b"bad shape" in lib.dagl_last_error()
    assert _fold_mix(lib, shape=(2, 24, -1)) == -1
    assert _fold_mix(lib, shape=(1, 16384, 16384)) == -1 and b"row ids" in lib.dagl_last_error()
