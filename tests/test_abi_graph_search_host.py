"""The search step on a patch graph (dagl_graph_search*, csrc/graph_refresh.hip) on fake pointers: every call below is rejected before
anything reaches the device, as in test_abi_graph_refresh_host.py.  The entries came in without an ABI bump: found by symbol.  Then what
the Python layer refuses on the host."""
import ctypes as C
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE = (2, 24, 20)
ROWS = 2 * 6 * 5          # B L
E, MAXDEG = 480, 8


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, step=False, ws=_WS, ws_bytes=1 << 40, null=("tau",), shape=SHAPE, edges=E, max_row_edges=MAXDEG, radius=1, k=0, scale=10.0,
          flags=0, capacity=1 << 40, propagate=1, explore=8, seed=3):
    p = lambda n: None if n in null else _FAKE
    B, H, W = shape
    head = (None, B, H, W, p("wq_rows"), p("x_rows")) + ((p("b2p"),) if step else ()) + (p("row_off"), p("key"), edges, max_row_edges,
                                                                                         radius, p("tau"), k, C.c_float(scale), flags)
    tail = (p("row_off_out"), p("key_out"), p("weight_out"), p("score_out"), capacity, p("status_out"), ws, ws_bytes, propagate, explore,
            seed)
    return lib.dagl_graph_search_step(*head, p("out"), *tail) if step else lib.dagl_graph_search(*head, *tail)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_graph_search_workspace_bytes", "dagl_graph_search", "dagl_graph_search_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    # the arguments of the plain entries plus propagate, explore, seed
    assert len(_lib.SIGNATURES["dagl_graph_search"][1]) == len(_lib.SIGNATURES["dagl_graph_refresh"][1]) + 3 == 26
    assert len(_lib.SIGNATURES["dagl_graph_search_step"][1]) == len(_lib.SIGNATURES["dagl_graph_step"][1]) + 3 == 28
    assert _lib.SIGNATURES["dagl_graph_search"][1][:23] == _lib.SIGNATURES["dagl_graph_refresh"][1]
    assert _lib.SIGNATURES["dagl_graph_search_step"][1][:25] == _lib.SIGNATURES["dagl_graph_step"][1]
    assert len(_lib.SIGNATURES["dagl_graph_search_workspace_bytes"][1]) == 10
    assert re.search(r"dagl_graph_search\*[^.]*without a bump", header)


def test_workspace_bytes(lib):
    planner = lib.dagl_graph_search_workspace_bytes
    B, H, W = SHAPE
    # both sources off: the plain entries' sizes
    for radius in (0, 1, 2):
        assert planner(B, H, W, E, radius, 0, 0, 0, 1, 0) == lib.dagl_graph_refresh_workspace_bytes(B, H, W, E, radius)
        assert planner(B, H, W, E, radius, 0, 0, 8, 1, 0) == lib.dagl_graph_refresh_workspace_bytes(B, H, W, E, radius)
        for want_graph in (0, 1):
            assert planner(B, H, W, E, radius, 0, 0, 0, want_graph, 1) == lib.dagl_graph_step_workspace_bytes(B, H, W, E, radius, want_graph)
    # the staging arrays: three of 4 bytes per entry; the entries by the layout (each array is carved at an aligned place: compare sizes
    # through the plain planner, which carves the same way at a chosen number of entries)
    def plain(entries):                           # the refresh's workspace with `entries` staged entries (radius 0: E = entries)
        return lib.dagl_graph_refresh_workspace_bytes(B, H, W, entries, 0)
    for radius in (0, 1, 2):
        w2 = (2 * radius + 1) ** 2
        for propagate, explore in ((1, 0), (0, 5), (1, 8), (1, 256)):
            assert planner(B, H, W, E, radius, propagate, explore, 0, 1, 0) == plain((1 + 4 * propagate) * E * w2 + explore * ROWS)
            assert planner(B, H, W, E, radius, propagate, explore, 4, 1, 0) == plain(ROWS * 4)          # a rank cut: k entries per row
            # the step: the aggregated rows in front; without graph outputs nothing else
            alone = planner(B, H, W, E, radius, propagate, explore, 0, 0, 1)
            assert alone == lib.dagl_graph_step_workspace_bytes(B, H, W, E, radius, 0) >= ROWS * 784 * 4
            assert planner(B, H, W, E, radius, propagate, explore, 0, 1, 1) - alone == plain((1 + 4 * propagate) * E * w2 + explore * ROWS)
    assert planner(B, H, W, 0, 1, 0, 8, 0, 1, 0) == plain(8 * ROWS)       # an empty graph can be populated
    assert planner(B, H, W, E, 1, 1, 8, 0, 1, 0) > planner(B, H, W, E, 1, 0, 8, 0, 1, 0) > planner(B, H, W, E, 1, 0, 0, 0, 1, 0)
    for bad, word in (((0, H, W, E, 1, 1, 8, 0, 1, 0), b"bad shape"), ((B, H, W, -1, 1, 1, 8, 0, 1, 0), b"total_edges"),
                      ((B, H, W, E, 9, 1, 8, 0, 1, 0), b"radius"), ((B, H, W, E, 1, 2, 8, 0, 1, 0), b"propagate"),
                      ((B, H, W, E, 1, -1, 8, 0, 1, 0), b"propagate"), ((B, H, W, E, 1, 1, 257, 0, 1, 0), b"explore"),
                      ((B, H, W, E, 1, 1, -1, 0, 1, 0), b"explore"), ((B, H, W, E, 1, 1, 8, -1, 1, 0), b"k=-1")):
        assert planner(*bad) == 0
        err = lib.dagl_last_error()
        assert word in err and b"dagl_graph_search_workspace_bytes" in err, err


@pytest.mark.parametrize("step", [False, True])
def test_search_arguments(lib, step):
    who = b"dagl_graph_search_step" if step else b"dagl_graph_search"
    for kw, word in ((dict(explore=257), b"explore=257"), (dict(explore=-1), b"explore=-1"), (dict(propagate=2), b"propagate=2"),
                     (dict(propagate=-1), b"propagate=-1")):
        assert _call(lib, step, **kw) == -1
        err = lib.dagl_last_error()
        assert word in err and who in err, err
        assert _call(lib, step, ws_bytes=0, **kw) == -1                   # ... before the workspace is looked at
    # the limits themselves pass as far as the workspace
    for kw in (dict(explore=256), dict(explore=0), dict(propagate=0), dict(propagate=0, explore=0), dict(seed=0xFFFFFFFF)):
        assert _call(lib, step, ws_bytes=0, **kw) == -2, kw


@pytest.mark.parametrize("step", [False, True])
def test_candidate_bound(lib, step):
    from dagl_amd import _lib
    cap = lib.dagl_graph_refresh_max_candidates()
    for radius, propagate, explore in ((0, 1, 0), (1, 1, 8), (1, 0, 8), (2, 1, 256), (0, 0, 256)):
        w2 = (2 * radius + 1) ** 2
        fits = (cap - explore) // ((1 + 4 * propagate) * w2)
        assert _call(lib, step, radius=radius, propagate=propagate, explore=explore, max_row_edges=fits, ws_bytes=0) == _lib.ERR_WORKSPACE
        assert _call(lib, step, radius=radius, propagate=propagate, explore=explore, max_row_edges=fits + 1) == _lib.ERR_UNSUPPORTED
        err = lib.dagl_last_error().decode()
        assert str((1 + 4 * propagate) * (fits + 1) * w2 + explore) in err and str(cap) in err and "explore" in err, err
    # the plain bound still comes first and keeps its message
    assert _call(lib, step, radius=1, max_row_edges=228) == _lib.ERR_UNSUPPORTED and b"2052 candidates" in lib.dagl_last_error()
    # both sources off: the plain bound alone
    assert _call(lib, step, radius=1, max_row_edges=227, propagate=0, explore=0, ws_bytes=0) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("step", [False, True])
def test_what_the_plain_entries_refuse(lib, step):
    from dagl_amd import _lib
    for kw, code, word in ((dict(null=("tau", "wq_rows")), -1, b"null"), (dict(null=("tau", "status_out")), -1, b"null"),
                           (dict(null=("tau", "key_out")), -1, b"null"), (dict(null=("tau", "key")), -1, b"null"),
                           (dict(radius=9), -1, b"radius"), (dict(radius=-1), -1, b"radius"), (dict(k=-1), -1, b"k=-1"),
                           (dict(scale=0.0), -1, b"scale"), (dict(max_row_edges=-1), -1, b"max_row_edges"), (dict(flags=0x8), -1, b"flags"),
                           (dict(ws=_WS + 8), -1, b"aligned"), (dict(shape=(0, 24, 20)), -1, b"bad shape"), (dict(edges=-1), -1, b"total_edges"),
                           (dict(edges=1 << 31, radius=0), -1, b"2^31")):
        assert _call(lib, step, **kw) == code, kw
        assert word in lib.dagl_last_error(), (kw, lib.dagl_last_error())
    if step:
        assert _call(lib, True, null=("tau", "b2p")) == -1 and _call(lib, True, null=("tau", "out")) == -1
    # with random keys an empty graph is populated: the output arrays may not be null then (they may with explore = 0)
    outs = ("key_out", "weight_out", "score_out")
    assert _call(lib, step, null=("tau", "key") + outs, edges=0, max_row_edges=0, explore=0, capacity=0, ws_bytes=0) == -2
    assert _call(lib, step, null=("tau", "key") + outs, edges=0, max_row_edges=0, explore=4) == -1 and b"null" in lib.dagl_last_error()
    assert _call(lib, step, null=("tau", "key"), edges=0, max_row_edges=0, explore=4, ws_bytes=0) == -2


def test_capacity_and_workspace_one_short(lib):
    from dagl_amd import _lib
    B, H, W = SHAPE
    for propagate, explore in ((1, 0), (0, 5), (1, 8)):
        may = (1 + 4 * propagate) * E * 9 + explore * ROWS
        for kw, bound in ((dict(), may), (dict(k=8), ROWS * 8), (dict(k=1000), may), (dict(k=8, flags=_lib.GRAPH_REFRESH_KEEP_ALL), may)):
            assert _call(lib, propagate=propagate, explore=explore, capacity=bound - 1, **kw) == _lib.ERR_WORKSPACE
            err = lib.dagl_last_error().decode()
            assert "capacity" in err and str(bound) in err, err
            assert _call(lib, propagate=propagate, explore=explore, capacity=bound, ws_bytes=0, **kw) == _lib.ERR_WORKSPACE
            assert "workspace" in lib.dagl_last_error().decode()
        for k, flags in ((0, 0), (8, 0), (8, _lib.GRAPH_REFRESH_KEEP_ALL)):
            need = lib.dagl_graph_search_workspace_bytes(B, H, W, E, 1, propagate, explore, 0 if flags else k, 1, 0)
            assert _call(lib, propagate=propagate, explore=explore, k=k, flags=flags, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
            err = lib.dagl_last_error().decode()
            assert "dagl_graph_search" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    # the step without graph outputs does not look at the capacity
    none = ("tau", "row_off_out", "key_out", "weight_out", "score_out")
    need = lib.dagl_graph_search_workspace_bytes(B, H, W, E, 1, 1, 8, 8, 0, 1)
    assert _call(lib, True, null=none, capacity=0, k=8, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert int(re.search(r"required (\d+) B", lib.dagl_last_error().decode()).group(1)) == need


# ---- the Python layer, on the host ------------------------------------------------------------------------------------------------------
def _cpu_graph(degree):
    import torch
    from dagl_amd.graph import PatchGraph
    B, H, W = 1, 24, 20
    n = B * 30
    row_off = torch.arange(n + 1, dtype=torch.int64) * degree
    g = PatchGraph(row_off, torch.zeros(n * degree, dtype=torch.int32), torch.zeros(n * degree), None, B, H, W, "topk", 4)
    g._valid, g._max_degree = True, degree
    return g


def test_row_bound_arithmetic():
    from dagl_amd import ops
    assert ops.graph_search_row_bound(8, 1, False, 0) == 72 and ops.graph_search_row_bound(8, 1, True, 8) == 368
    assert ops.graph_search_row_bound(16, 1, True, 8) == 728 and ops.graph_search_row_bound(45, 1, True, 24) == 2049
    assert ops.graph_search_row_bound(3, 0, 1, 256) == 271


def test_python_layer_refuses_on_the_host(lib, monkeypatch):
    """CPU tensors never reach the library; the search keywords are looked at before anything else."""
    import torch
    from dagl_amd import DaglError, ops
    from dagl_amd._lib import ERR_UNSUPPORTED
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    ce = CE(in_channels=64)
    ce.select_mode, ce.select_k = "topk", 4
    x = torch.zeros(1, 64, 24, 20)
    g = _cpu_graph(8)
    for call in (ce.refresh_graph, ce.step_graph):
        for kw, word in ((dict(explore=300), "explore=300"), (dict(explore=-1), "explore=-1"), (dict(explore=2.5), "explore"),
                         (dict(propagate=2), "propagate"), (dict(seed="a"), "seed")):
            with pytest.raises(DaglError, match=word):
                call(x, g, **kw)
    with pytest.raises(DaglError, match="explore=300"):
        ce.build_graph(x, explore=300)
    with pytest.raises(DaglError, match="iters"):
        ce.build_graph(x, iters=0)
    with pytest.raises(DaglError, match="GPU"):
        ce.build_graph(x)
    wq, xr = torch.zeros(1, 30, 196), torch.zeros(1, 480, 196)
    for kw in (dict(explore=300), dict(propagate=3), dict(seed=None)):
        with pytest.raises(DaglError, match=next(iter(kw))):
            ops.graph_search(wq, xr, g.row_off, g.key, hw=(24, 20), **kw)
        with pytest.raises(DaglError, match=next(iter(kw))):
            ops.graph_search_step(wq, xr, torch.zeros(1, 30, 26, 16), g.row_off, g.key, **kw)
    with pytest.raises(DaglError):                                         # a CPU tensor with the keywords in range
        ops.graph_search(wq, xr, g.row_off, g.key, hw=(24, 20), propagate=True, explore=8, max_row_edges=8)

    # the stage-fused step has no search flavour: refused before the state or the input is looked at
    ces = CES(64)
    for kw in (dict(propagate=True), dict(explore=8), dict(propagate=True, explore=8, seed=5)):
        with pytest.raises(DaglError, match="fused=True"):
            ces.step_graphs(torch.zeros(1, 64, 24, 20), None, fused=True, **kw)
    with pytest.raises(DaglError, match="explore=300"):
        ces.step_graphs(torch.zeros(1, 64, 24, 20), None, explore=300)
    with pytest.raises(DaglError, match="SequenceState"):                  # fused=None with the keywords: past the refusal
        ces.step_graphs(torch.zeros(1, 64, 24, 20), None, propagate=True)

    # the candidate bound (the refusal that follows the shape checks: those are stepped over here, the input is a CPU tensor)
    monkeypatch.setattr(CE, "_check_given_graph", lambda self, b, graph, what: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    cap = ops.graph_refresh_max_candidates()
    fits = (cap - 8) // 45
    for call in (ce.refresh_graph, ce.step_graph):
        with pytest.raises(DaglError, match="candidates") as e:
            call(x, _cpu_graph(fits + 1), propagate=True, explore=8)
        assert e.value.code == ERR_UNSUPPORTED and str(5 * (fits + 1) * 9 + 8) in str(e.value)
        with pytest.raises(DaglError, match="candidates") as e:            # the plain bound keeps its place and its message
            call(x, _cpu_graph(cap // 9 + 1), propagate=True, explore=8)
        assert e.value.code == ERR_UNSUPPORTED and "largest degree" in str(e.value)
    assert ce._refresh_arguments(x, _cpu_graph(fits), "refresh_graph", 1, None, "reference", "fp32", propagate=True, explore=8) \
        == (1, 4, False, fits)
    assert ce._refresh_arguments(x, _cpu_graph(fits + 1), "refresh_graph", 1, None, "reference", "fp32") == (1, 4, False, fits + 1)
