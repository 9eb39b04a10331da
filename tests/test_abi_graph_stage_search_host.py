"""The search step of a whole CES stage (dagl_graph_stage_search*; csrc/graph_refresh.hip) on fake pointers: every call below is rejected
before anything reaches the device, as in test_abi_stage_step_host.py.  The entries came in without an ABI bump: found by symbol."""
import ctypes as C
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE = (2, 24, 20)
ROWS = 4 * 2 * 6 * 5      # 4 B L
E, MAXDEG = 1920, 8
_GRAPH = ["row_off_out", "key_out", "weight_out", "score_out"]
_STEP_ONLY = ["x", "mix_w", "mix_b", "out"]
ENTRIES = ("dagl_graph_stage_search", "dagl_graph_stage_search_step")


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _table(entries):
    return (C.c_void_p * 4)(*entries)


def _call(lib, entry, ws=_WS, ws_bytes=1 << 40, null=("tau4",), entries=None, shape=SHAPE, edges=E, max_row_edges=MAXDEG, radius=1, k=0,
          scale=10.0, flags=0, capacity=1 << 40, propagate=1, explore=8, seed=0):
    """``null``: the arguments passed as NULL; ``entries``: {table: four values} in the place of four fake pointers."""
    entries = entries or {}
    p = lambda n: None if n in null else _FAKE
    t = lambda n: None if n in null else _table(entries.get(n, [_FAKE] * 4))
    B, H, W = shape
    step = entry.endswith("_step")
    front = (None, B, H, W, t("wq_rows4"), t("x_rows4")) + ((t("b2p4"),) if step else ())
    mid = (p("row_off"), p("key"), edges, max_row_edges, radius, t("tau4"), k, scale, flags)
    mix = (p("x"), p("mix_w"), p("mix_b"), p("out")) if step else ()
    back = (p("row_off_out"), p("key_out"), p("weight_out"), p("score_out"), capacity, p("status_out"), ws, ws_bytes, propagate, explore,
            seed)
    return getattr(lib, entry)(*front, *mid, *mix, *back)


def test_symbols_header_table_version(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    assert re.search(r"#define\s+DAGL_ABI_VERSION\s+412\b", header)
    for name in ("dagl_graph_stage_search_workspace_bytes",) + ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert len(_lib.SIGNATURES["dagl_graph_stage_search_workspace_bytes"][1]) == 10
    assert len(_lib.SIGNATURES["dagl_graph_stage_search"][1]) == 26 and len(_lib.SIGNATURES["dagl_graph_stage_search_step"][1]) == 31
    assert re.search(r"dagl_graph_stage_search\*[^.]*without a bump", header)
    # the two consequences of the contract are written down
    assert "HEAD-LOCAL" in header and "never crosses a head" in header


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_call_passes_its_checks_as_far_as_the_workspace(lib, entry):
    from dagl_amd import _lib
    assert _call(lib, entry, ws_bytes=0) == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    assert _call(lib, entry, null=(), ws_bytes=0) == _lib.ERR_WORKSPACE                                    # with tau
    for propagate, explore in ((0, 0), (1, 0), (0, 8), (1, 256)):                                           # both sources off is allowed
        assert _call(lib, entry, propagate=propagate, explore=explore, ws_bytes=0) == _lib.ERR_WORKSPACE
    if entry.endswith("_step"):
        assert _call(lib, entry, null=tuple(_GRAPH) + ("tau4",), capacity=0, ws_bytes=0) == _lib.ERR_WORKSPACE      # the output alone


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["wq_rows4", "x_rows4", "b2p4"])
def test_pointer_tables(lib, entry, name):
    if name == "b2p4" and not entry.endswith("_step"):
        return
    assert _call(lib, entry, null=(name, "tau4")) == -1 and b"null" in lib.dagl_last_error()
    for h in range(4):
        entries = [_FAKE] * 4
        entries[h] = None
        assert _call(lib, entry, entries={name: entries}) == -1, (name, h)
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, entry, entries={name: entries}, ws_bytes=0) == -1                                # ... before the workspace is looked at
        entries[h] = _FAKE + 8
        assert _call(lib, entry, entries={name: entries}) == -1, (name, h)
        assert b"16-byte aligned" in lib.dagl_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_tau_for_all_heads_or_none(lib, entry):
    from dagl_amd import _lib
    assert _call(lib, entry, entries={"tau4": [None] * 4}, null=(), ws_bytes=0) == _lib.ERR_WORKSPACE
    for given in ([_FAKE, None, None, None], [_FAKE, _FAKE, _FAKE, None], [None, _FAKE, _FAKE, _FAKE]):
        assert _call(lib, entry, entries={"tau4": given}, null=()) == -1
        assert b"tau" in lib.dagl_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(lib, entry):
    names = ["row_off", "status_out", "key"] + (_STEP_ONLY if entry.endswith("_step") else [])
    for name in names:
        assert _call(lib, entry, null=(name, "tau4")) == -1, name
        assert b"null" in lib.dagl_last_error()
        assert _call(lib, entry, null=(name, "tau4"), ws_bytes=0) == -1


@pytest.mark.parametrize("entry", ENTRIES)
def test_graph_outputs_all_or_none(lib, entry):
    from dagl_amd import _lib
    for name in _GRAPH:
        assert _call(lib, entry, null=(name, "tau4")) == -1 and b"null" in lib.dagl_last_error()
        only = tuple(n for n in _GRAPH if n != name) + ("tau4",)
        assert _call(lib, entry, null=only) == -1 and b"null" in lib.dagl_last_error()
    # the graph-only entry has nothing to give without them
    if not entry.endswith("_step"):
        assert _call(lib, entry, null=tuple(_GRAPH) + ("tau4",)) == -1 and b"null" in lib.dagl_last_error()
    # without edges and without random keys the three edge arrays (and key) may be null, the offsets may not
    no_edges = dict(edges=0, max_row_edges=0, capacity=0, ws_bytes=0, explore=0)
    assert _call(lib, entry, null=("key", "key_out", "weight_out", "score_out", "tau4"), **no_edges) == _lib.ERR_WORKSPACE
    assert _call(lib, entry, null=("key", "row_off_out", "tau4"), **no_edges) == -1
    # random keys populate an empty input: key may be null, the outputs may not
    populated = dict(edges=0, max_row_edges=0, explore=8, capacity=ROWS * 8, ws_bytes=0)
    assert _call(lib, entry, null=("key", "tau4"), **populated) == _lib.ERR_WORKSPACE
    assert _call(lib, entry, null=("key", "key_out", "weight_out", "score_out", "tau4"), **populated) == -1


@pytest.mark.parametrize("entry", ENTRIES)
def test_propagate_and_explore_ranges(lib, entry):
    for propagate in (-1, 2):
        assert _call(lib, entry, propagate=propagate) == -1 and b"propagate" in lib.dagl_last_error()
        assert lib.dagl_graph_stage_search_workspace_bytes(*SHAPE, E, 1, propagate, 8, 0, 1, 1) == 0
    for explore in (-1, 257):
        assert _call(lib, entry, explore=explore) == -1 and b"explore" in lib.dagl_last_error()
        assert lib.dagl_graph_stage_search_workspace_bytes(*SHAPE, E, 1, 1, explore, 0, 1, 1) == 0
    assert _call(lib, entry, explore=256, max_row_edges=4, ws_bytes=0) == -2


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("radius", [-1, 9])
def test_radius_outside_0_8(lib, entry, radius):
    assert _call(lib, entry, radius=radius, max_row_edges=1) == -1
    assert b"radius" in lib.dagl_last_error()
    assert lib.dagl_graph_stage_search_workspace_bytes(*SHAPE, E, radius, 1, 8, 0, 1, 1) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_scale_max_row_edges_flags(lib, entry):
    assert _call(lib, entry, radius=0, ws_bytes=0) == -2 and _call(lib, entry, radius=8, max_row_edges=1, ws_bytes=0) == -2
    assert _call(lib, entry, k=-1) == -1 and b"k=-1" in lib.dagl_last_error()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(lib, entry, scale=scale) == -1 and b"scale" in lib.dagl_last_error()
    assert _call(lib, entry, max_row_edges=-1) == -1 and b"max_row_edges" in lib.dagl_last_error()
    assert _call(lib, entry, flags=0x10) == -1 and b"flags" in lib.dagl_last_error()
    assert _call(lib, entry, flags=0xf, ws_bytes=0) == -2


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_bound_above_the_candidate_cap(lib, entry):
    from dagl_amd import _lib
    cap = lib.dagl_graph_refresh_max_candidates()
    for radius, propagate, explore in ((0, 1, 8), (1, 1, 8), (2, 1, 0), (1, 0, 8), (1, 0, 0), (2, 1, 256)):
        w2 = (2 * radius + 1) ** 2
        per = (1 + 4 * propagate) * w2
        fits = (cap - explore) // per
        assert _call(lib, entry, radius=radius, propagate=propagate, explore=explore, max_row_edges=fits, ws_bytes=0) == _lib.ERR_WORKSPACE
        assert _call(lib, entry, radius=radius, propagate=propagate, explore=explore, max_row_edges=fits + 1) == _lib.ERR_UNSUPPORTED
        err = lib.dagl_last_error().decode()
        assert entry in err and str((fits + 1) * per + explore) in err and str(cap) in err, err


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_one_edge_short(lib, entry):
    from dagl_amd import _lib
    # dagl_graph_search's rule with 4 B in the place of B: (1 + 4 propagate) E w2 + explore 4 B L, or 4 B L k where that is smaller
    for propagate, explore in ((1, 8), (0, 8), (1, 0), (0, 0)):
        may = (1 + 4 * propagate) * E * 9 + explore * ROWS
        assert _call(lib, entry, propagate=propagate, explore=explore, capacity=may - 1) == _lib.ERR_WORKSPACE
        err = lib.dagl_last_error().decode()
        assert "capacity" in err and str(may) in err, err
        assert _call(lib, entry, propagate=propagate, explore=explore, capacity=may, ws_bytes=0) == _lib.ERR_WORKSPACE
        assert "workspace" in lib.dagl_last_error().decode()
    assert _call(lib, entry, k=8, capacity=ROWS * 8 - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "capacity" in err and str(ROWS * 8) in err, err
    assert _call(lib, entry, k=8, capacity=ROWS * 8, ws_bytes=0) == _lib.ERR_WORKSPACE and "workspace" in lib.dagl_last_error().decode()
    assert _call(lib, entry, k=8, flags=_lib.GRAPH_REFRESH_KEEP_ALL, capacity=5 * E * 9 + 8 * ROWS - 1) == _lib.ERR_WORKSPACE
    assert "capacity" in lib.dagl_last_error().decode()
    if entry.endswith("_step"):                     # the output alone does not look at it
        assert _call(lib, entry, null=tuple(_GRAPH) + ("tau4",), capacity=0, ws_bytes=0) == _lib.ERR_WORKSPACE
        assert "workspace" in lib.dagl_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("want_graph", [0, 1])
@pytest.mark.parametrize("k", [0, 4])
def test_workspace_one_byte_short_or_misaligned(lib, entry, k, want_graph):
    from dagl_amd import _lib
    step = entry.endswith("_step")
    if not step and not want_graph:
        return
    need = lib.dagl_graph_stage_search_workspace_bytes(*SHAPE, E, 1, 1, 8, k, want_graph, 1 if step else 0)
    staged = ROWS * k if k else 5 * E * 9 + 8 * ROWS
    assert need >= (ROWS * 784 * 4 if step else 0) + want_graph * (ROWS * 4 + 3 * 4 * staged)
    null = ("tau4",) if want_graph else tuple(_GRAPH) + ("tau4",)
    assert _call(lib, entry, null=null, k=k, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert entry in err and "workspace" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    assert _call(lib, entry, null=null, k=k, ws=_WS + 8, ws_bytes=need) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, entry, null=null, k=k, ws=None, ws_bytes=need) == -1


def test_planner_grows_with_explore_and_propagate(lib):
    planner = lib.dagl_graph_stage_search_workspace_bytes
    for aggregate in (0, 1):
        sizes = [planner(*SHAPE, E, 1, 0, explore, 0, 1, aggregate) for explore in (0, 1, 8, 64, 256)]
        assert all(a > 0 for a in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        for explore in (0, 8):
            assert planner(*SHAPE, E, 1, 1, explore, 0, 1, aggregate) > planner(*SHAPE, E, 1, 0, explore, 0, 1, aggregate)
        # under a rank cut the staging holds 4 B L k entries whatever the sources are: never smaller with more of them
        assert planner(*SHAPE, E, 1, 1, 8, 4, 1, aggregate) >= planner(*SHAPE, E, 1, 0, 0, 4, 1, aggregate) > 0
    assert planner(*SHAPE, E, 1, 1, 8, 0, 1, 1) > planner(*SHAPE, E, 1, 1, 8, 0, 0, 1) >= ROWS * 784 * 4
    assert planner(*SHAPE, E, 1, 1, 8, -1, 1, 1) == 0
    assert planner(0, 24, 20, 10, 1, 1, 8, 0, 1, 1) == 0 and planner(1, 24, 20, -1, 1, 1, 8, 0, 1, 1) == 0
    # 4 B H W must fit the row ids
    assert planner(1, 16384, 16384, 0, 1, 1, 8, 0, 0, 1) == 0
    for entry in ENTRIES:
        assert _call(lib, entry, shape=(1, 16384, 16384)) == -1 and b"row ids" in lib.dagl_last_error()
        assert _call(lib, entry, shape=(0, 24, 20)) == -1 and b"bad shape" in lib.dagl_last_error()
        assert _call(lib, entry, edges=1 << 31, radius=0) == -1 and b"2^31" in lib.dagl_last_error()
