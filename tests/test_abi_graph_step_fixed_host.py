"""The step on a fixed-width patch graph (dagl_graph_step_fixed, csrc/graph_refresh.hip) on fake pointers: every call below is rejected
before anything reaches the device, as in test_abi_graph_search_host.py.  The entries came in without an ABI bump: found by symbol."""
import ctypes as C
import os
import re

import pytest

_WS = 0x100000            # a 256-byte aligned fake workspace
ERR_INVALID = -1          # DAGL_ERR_INVALID
SHAPE = (2, 24, 20)
ROWS = 2 * 6 * 5          # B L
N = 480
WIDTH = 8
# fake arrays 16 MiB apart: no two of them overlap at these sizes
_AT = {n: 0x10000000 + i * 0x1000000 for i, n in enumerate(("wq_rows", "x_rows", "b2p", "key_in", "deg_in", "tau", "out", "key_out",
                                                             "weight_out", "score_out", "deg_out", "status"))}


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, step=True, ws=_WS, ws_bytes=1 << 40, null=("tau",), at=None, shape=SHAPE, width_in=WIDTH, width_out=WIDTH, radius=1, k=0,
          scale=10.0, flags=0, propagate=0, explore=0, seed=3):
    null = tuple(null) + (() if step else ("b2p", "out"))
    where = dict(_AT, **(at or {}))
    p = lambda n: None if n in null else where[n]
    B, H, W = shape
    return lib.dagl_graph_step_fixed(None, B, H, W, p("wq_rows"), p("x_rows"), p("b2p"), p("key_in"), p("deg_in"), width_in, radius, p("tau"),
                                     k, C.c_float(scale), flags, propagate, explore, seed, p("out"), p("key_out"), p("weight_out"),
                                     p("score_out"), p("deg_out"), width_out, p("status"), ws, ws_bytes)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_graph_step_fixed_workspace_bytes", "dagl_graph_step_fixed"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    # the header's argument list, type by type, against the table's
    decl = re.search(r"int\s+dagl_graph_step_fixed\((.*?)\);", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(_lib._vp if "*" in arg else C.c_float if arg.startswith("float ") else C.c_uint32 if arg.startswith("uint32_t ")
                     else C.c_size_t if arg.startswith("size_t ") else C.c_int)
    assert kinds == _lib.SIGNATURES["dagl_graph_step_fixed"][1] and len(kinds) == 27
    assert _lib.SIGNATURES["dagl_graph_step_fixed_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert re.search(r"size_t\s+dagl_graph_step_fixed_workspace_bytes\(int B, int H, int W, int want_out\);", header)


def test_workspace_bytes(lib):
    planner = lib.dagl_graph_step_fixed_workspace_bytes
    B, H, W = SHAPE
    assert planner(B, H, W, 0) == 0
    assert planner(B, H, W, 1) == -(-ROWS * 784 * 4 // 256) * 256                 # the [B L, 784] rows, carved at 256 bytes
    assert planner(1, 33, 70, 1) == -(-(9 * 18) * 784 * 4 // 256) * 256
    # the same rows dagl_graph_step carves when it hands out no graph
    assert planner(B, H, W, 1) == lib.dagl_graph_step_workspace_bytes(B, H, W, 100, 1, 0)
    assert planner(0, H, W, 1) == 0
    err = lib.dagl_last_error()
    assert b"bad shape" in err and b"dagl_graph_step_fixed_workspace_bytes" in err, err


@pytest.mark.parametrize("step", [False, True])
def test_refusals(lib, step):
    from dagl_amd import _lib
    who = b"dagl_graph_step_fixed"
    cases = [(dict(shape=(0, 24, 20)), b"bad shape"), (dict(shape=(1 << 12, 1 << 10, 1 << 9)), b"32-bit"),
             (dict(radius=9), b"radius"), (dict(radius=-1), b"radius"),
             (dict(width_in=0), b"width_in=0"), (dict(width_out=0), b"width_out=0"), (dict(width_in=-4), b"width_in=-4"),
             (dict(propagate=2), b"propagate=2"), (dict(propagate=-1), b"propagate=-1"), (dict(explore=257), b"explore=257"),
             (dict(explore=-1), b"explore=-1"),
             (dict(null=("tau", "wq_rows")), b"null"), (dict(null=("tau", "x_rows")), b"null"), (dict(null=("tau", "key_in")), b"null"),
             (dict(null=("tau", "deg_in")), b"null"), (dict(null=("tau", "key_out")), b"null"), (dict(null=("tau", "weight_out")), b"null"),
             (dict(null=("tau", "score_out")), b"null"), (dict(null=("tau", "deg_out")), b"null"), (dict(null=("tau", "status")), b"null"),
             (dict(at=dict(wq_rows=_AT["wq_rows"] + 4)), b"16-byte"), (dict(flags=0x8), b"flags"), (dict(scale=0.0), b"scale"),
             (dict(scale=float("inf")), b"scale"), (dict(k=-1), b"k=-1"),
             # a rank cut needs room for min(k, N) entries
             (dict(k=9), b"width_out=8 < min(k, N) = 9"), (dict(k=3, width_out=2), b"width_out=2 < min(k, N) = 3"),
             (dict(k=1000, width_out=N - 1, width_in=4), b"min(k, N) = 480")]
    for kw, word in cases:
        assert _call(lib, step, **kw) == ERR_INVALID, kw
        err = lib.dagl_last_error()
        assert word in err and who in err, (kw, err)
        assert _call(lib, step, ws_bytes=0, ws=None, **kw) == ERR_INVALID   # ... before the workspace is looked at
    # exactly one of b2p and out
    for gone in ("b2p", "out"):
        assert _call(lib, True, null=("tau", gone)) == ERR_INVALID
        assert b"b2p and out" in lib.dagl_last_error()
    if step:
        assert _call(lib, True, at=dict(b2p=_AT["b2p"] + 8)) == ERR_INVALID and b"b2p must be 16-byte" in lib.dagl_last_error()
    # what passes goes as far as the workspace (the step) or the launch's own check would: with keep_all k does not bound the width,
    # k = N fits a row of N slots, the limits of the search arguments themselves pass
    for kw in (dict(k=9, flags=_lib.GRAPH_REFRESH_KEEP_ALL), dict(k=8), dict(k=1000, width_out=N, width_in=4), dict(explore=256, width_in=4),
               dict(propagate=1), dict(seed=0xFFFFFFFF, explore=1), dict(flags=_lib.GRAPH_REFRESH_BLOCK_ROWS | _lib.GRAPH_ATTEND_EDGES_ONLY)):
        assert _call(lib, True, ws_bytes=0, **kw) == _lib.ERR_WORKSPACE, kw


@pytest.mark.parametrize("step", [False, True])
def test_candidate_bound(lib, step):
    from dagl_amd import _lib
    cap = lib.dagl_graph_refresh_max_candidates()
    for radius, propagate, explore in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (1, 1, 8), (1, 0, 8), (2, 1, 256), (0, 0, 256)):
        w2 = (2 * radius + 1) ** 2
        fits = (cap - explore) // ((1 + 4 * propagate) * w2)
        kw = dict(radius=radius, propagate=propagate, explore=explore)
        assert _call(lib, True, width_in=fits, ws_bytes=0, **kw) == _lib.ERR_WORKSPACE
        assert _call(lib, step, width_in=fits + 1, **kw) == _lib.ERR_UNSUPPORTED
        err = lib.dagl_last_error().decode()
        assert str((1 + 4 * propagate) * (fits + 1) * w2 + explore) in err and str(cap) in err and "dagl_graph_step_fixed" in err, err


@pytest.mark.parametrize("step", [False, True])
def test_outputs_may_not_overlap_inputs(lib, step):
    from dagl_amd import _lib
    B, H, W = SHAPE
    sizes = dict(wq_rows=ROWS * 196 * 4, x_rows=B * N * 196 * 4, b2p=B * (H + 6) * (W + 6) * 16 * 4, key_in=ROWS * WIDTH * 4, deg_in=ROWS * 4,
                 tau=ROWS * 4, out=B * 16 * N * 4, key_out=ROWS * WIDTH * 4, weight_out=ROWS * WIDTH * 4, score_out=ROWS * WIDTH * 4,
                 deg_out=ROWS * 4)
    inputs = ("wq_rows", "x_rows", "key_in", "deg_in", "tau") + (("b2p",) if step else ())
    outputs = ("key_out", "weight_out", "score_out", "deg_out") + (("out",) if step else ())
    for o in outputs:
        for i in inputs:
            # the output on the input, on its last 16 bytes, and ending 16 bytes into it: refused;  touching it end to start: served
            for at in (_AT[i], _AT[i] + sizes[i] - 16, _AT[i] - sizes[o] + 16):
                assert _call(lib, step, null=(), at={o: at}) == ERR_INVALID, (o, i, at)
                err = lib.dagl_last_error()
                assert b"overlaps" in err and b"dagl_graph_step_fixed" in err, err
            # (the step form only: its empty workspace stops the call, the refresh alone needs none and would launch)
            for at in (_AT[i] + sizes[i], _AT[i] - sizes[o]):
                assert _call(lib, True, null=(), at={o: at}, ws_bytes=0) == _lib.ERR_WORKSPACE, (o, i, at)
    # the in-place update of a graph is such an overlap: key_out on key_in
    assert _call(lib, step, at=dict(key_out=_AT["key_in"])) == ERR_INVALID and b"overlaps" in lib.dagl_last_error()


def test_workspace_one_short(lib):
    from dagl_amd import _lib
    B, H, W = SHAPE
    need = lib.dagl_graph_step_fixed_workspace_bytes(B, H, W, 1)
    assert _call(lib, True, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_graph_step_fixed" in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    assert _call(lib, True, ws=_WS + 8) == ERR_INVALID and b"aligned" in lib.dagl_last_error()
    assert _call(lib, True, ws=None) == ERR_INVALID and b"workspace" in lib.dagl_last_error()
