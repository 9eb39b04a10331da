"""The fixed-width step of a whole CES stage (dagl_graph_stage_step_fixed, csrc/graph_refresh.hip) on fake pointers: every call below is
rejected before anything reaches the device, as in test_abi_graph_step_fixed_host.py and test_abi_graph_stage_search_host.py.  The
entries came in without an ABI bump: found by symbol."""
import ctypes as C
import os
import re

import pytest

_WS = 0x100000            # a 256-byte aligned fake workspace
ERR_INVALID = -1          # DAGL_ERR_INVALID
SHAPE = (2, 24, 20)
HEAD_ROWS = 2 * 6 * 5     # B L
ROWS = 4 * HEAD_ROWS      # 4 B L
N = 480
WIDTH = 8
_TABLES = ("wq_rows4", "x_rows4", "b2p4", "tau4")
_PLAIN = ("key_in", "deg_in", "x", "mix_w", "mix_b", "out", "key_out", "weight_out", "score_out", "deg_out", "status")
_STEP = ("b2p4", "x", "mix_w", "mix_b", "out")
# fake arrays 16 MiB apart: no two of them overlap at these sizes
_AT = {n: 0x10000000 + i * 0x1000000 for i, n in enumerate([f"{t}[{h}]" for t in _TABLES for h in range(4)] + list(_PLAIN))}
ENTRY = "dagl_graph_stage_step_fixed"


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, step=True, ws=_WS, ws_bytes=1 << 40, null=("tau4",), at=None, shape=SHAPE, width_in=WIDTH, width_out=WIDTH, radius=1, k=0,
          scale=10.0, flags=0, propagate=0, explore=0, seed=3):
    """``null``: arguments (a table by its name, an entry as ``name[h]``) passed as NULL; ``at``: other addresses.  ``step`` False: the
    graph alone -- b2p4, x, mix_w, mix_b and out all NULL."""
    null = tuple(null) + (() if step else _STEP)
    where = dict(_AT, **(at or {}))
    p = lambda n: None if n in null else where[n]
    t = lambda n: None if n in null else (C.c_void_p * 4)(*[p(f"{n}[{h}]") for h in range(4)])
    B, H, W = shape
    return lib.dagl_graph_stage_step_fixed(None, B, H, W, t("wq_rows4"), t("x_rows4"), t("b2p4"), p("key_in"), p("deg_in"), width_in, radius,
                                           t("tau4"), k, C.c_float(scale), flags, propagate, explore, seed, p("x"), p("mix_w"), p("mix_b"),
                                           p("out"), p("key_out"), p("weight_out"), p("score_out"), p("deg_out"), width_out, p("status"),
                                           ws, ws_bytes)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    assert re.search(r"#define\s+DAGL_ABI_VERSION\s+412\b", header)
    for name in ("dagl_graph_stage_step_fixed_workspace_bytes", ENTRY):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    # the header's argument list, type by type, against the table's
    decl = re.search(r"int\s+dagl_graph_stage_step_fixed\((.*?)\);", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.POINTER(_lib._vp) if "* const*" in arg else _lib._vp if "*" in arg else C.c_float if arg.startswith("float ")
                     else C.c_uint32 if arg.startswith("uint32_t ") else C.c_size_t if arg.startswith("size_t ") else C.c_int)
    assert kinds == _lib.SIGNATURES[ENTRY][1] and len(kinds) == 30
    assert kinds.count(C.POINTER(_lib._vp)) == 4
    assert _lib.SIGNATURES["dagl_graph_stage_step_fixed_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert re.search(r"size_t\s+dagl_graph_stage_step_fixed_workspace_bytes\(int B, int H, int W, int want_out\);", header)


def test_workspace_bytes(lib):
    planner = lib.dagl_graph_stage_step_fixed_workspace_bytes
    B, H, W = SHAPE
    assert planner(B, H, W, 0) == 0
    assert planner(B, H, W, 1) == -(-ROWS * 784 * 4 // 256) * 256                 # the [4 B L, 784] rows, carved at 256 bytes
    assert planner(1, 33, 70, 1) == -(-(4 * 9 * 18) * 784 * 4 // 256) * 256
    # the rows of four heads: what the single-head planner gives for 4 B images
    assert planner(B, H, W, 1) == lib.dagl_graph_step_fixed_workspace_bytes(4 * B, H, W, 1)
    # ... and what dagl_graph_stage_step carves when it hands out no graph
    assert planner(B, H, W, 1) == lib.dagl_graph_stage_step_workspace_bytes(B, H, W, 100, 1, 0)
    # monotone in B
    sizes = [planner(b, H, W, 1) for b in (1, 2, 3, 5, 8)]
    assert all(a > 0 for a in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(planner(b, H, W, 0) == 0 for b in (1, 2, 8))
    assert planner(0, H, W, 1) == 0
    err = lib.dagl_last_error()
    assert b"bad shape" in err and b"dagl_graph_stage_step_fixed_workspace_bytes" in err, err
    assert planner(1, 16384, 16384, 1) == 0 and b"row ids" in lib.dagl_last_error()    # 4 B H W must fit the row ids


@pytest.mark.parametrize("step", [False, True])
def test_the_call_passes_its_checks_as_far_as_the_workspace(lib, step):
    """What passes goes as far as the workspace (the step); the graph alone needs none, so only the step form is sent."""
    from dagl_amd import _lib
    if not step:
        return
    for kw in (dict(), dict(null=()), dict(k=9, flags=_lib.GRAPH_REFRESH_KEEP_ALL), dict(k=8), dict(k=1000, width_out=N, width_in=4),
               dict(explore=256, width_in=4), dict(propagate=1), dict(seed=0xFFFFFFFF, explore=1),
               dict(flags=_lib.GRAPH_REFRESH_BLOCK_ROWS | _lib.GRAPH_ATTEND_EDGES_ONLY), dict(radius=0), dict(radius=8, width_in=1)):
        assert _call(lib, True, ws_bytes=0, **kw) == _lib.ERR_WORKSPACE, kw
        assert b"workspace" in lib.dagl_last_error()


@pytest.mark.parametrize("step", [False, True])
def test_refusals(lib, step):
    who = ENTRY.encode()
    nulls = [(dict(null=("tau4", n)), b"null") for n in ("wq_rows4", "x_rows4", "key_in", "deg_in", "key_out", "weight_out", "score_out",
                                                           "deg_out", "status")]
    nulls += [(dict(null=("tau4", f"{t}[{h}]")), b"null") for t in ("wq_rows4", "x_rows4") + (("b2p4",) if step else ()) for h in range(4)]
    cases = [(dict(shape=(0, 24, 20)), b"bad shape"), (dict(shape=(1 << 12, 1 << 10, 1 << 9)), b"32-bit"),
             (dict(shape=(1, 16384, 16384)), b"row ids"),                        # B H W fits, 4 B H W does not
             (dict(radius=9), b"radius"), (dict(radius=-1), b"radius"),
             (dict(width_in=0), b"width_in=0"), (dict(width_out=0), b"width_out=0"), (dict(width_in=-4), b"width_in=-4"),
             (dict(shape=(64, 1024, 1024), width_in=128, width_out=4), b"slots, 2^31 or more"),      # 4 B L width_in = 2^31
             (dict(shape=(64, 1024, 1024), width_in=4, width_out=128), b"slots, 2^31 or more"),
             (dict(propagate=2), b"propagate=2"), (dict(propagate=-1), b"propagate=-1"), (dict(explore=257), b"explore=257"),
             (dict(explore=-1), b"explore=-1")] + nulls + \
            [(dict(at={"wq_rows4[2]": _AT["wq_rows4[2]"] + 4}), b"16-byte"), (dict(at={"x_rows4[3]": _AT["x_rows4[3]"] + 8}), b"16-byte"),
             (dict(flags=0x8), b"flags"), (dict(scale=0.0), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(k=-1), b"k=-1"),
             # a rank cut needs room for min(k, N) entries
             (dict(k=9), b"width_out=8 < min(k, N) = 9"), (dict(k=3, width_out=2), b"width_out=2 < min(k, N) = 3"),
             (dict(k=1000, width_out=N - 1, width_in=4), b"min(k, N) = 480")]
    for kw, word in cases:
        assert _call(lib, step, **kw) == ERR_INVALID, kw
        err = lib.dagl_last_error()
        assert word in err and who in err, (kw, err)
        assert _call(lib, step, ws_bytes=0, ws=None, **kw) == ERR_INVALID   # ... before the workspace is looked at
    # tau for all four heads or for none
    for given in ((0,), (0, 1, 2), (1, 2, 3)):
        assert _call(lib, step, null=tuple(f"tau4[{h}]" for h in range(4) if h not in given)) == ERR_INVALID
        err = lib.dagl_last_error()
        assert b"tau" in err and b"all or none" in err and who in err, err
    assert _call(lib, True, null=tuple(f"tau4[{h}]" for h in range(4)), ws_bytes=0) == -2        # four NULL entries: no margin


def test_value_operands_come_together(lib):
    """b2p4, x, mix_w, mix_b and out: all of them or none."""
    from dagl_amd import _lib
    for gone in _STEP:
        assert _call(lib, True, null=("tau4", gone)) == ERR_INVALID, gone
        err = lib.dagl_last_error()
        assert b"come together" in err and ENTRY.encode() in err, err
        only = tuple(n for n in _STEP if n != gone) + ("tau4",)
        assert _call(lib, True, null=only) == ERR_INVALID and b"come together" in lib.dagl_last_error(), gone
    assert _call(lib, True, ws_bytes=0) == _lib.ERR_WORKSPACE
    for h in range(4):
        assert _call(lib, True, at={f"b2p4[{h}]": _AT[f"b2p4[{h}]"] + 8}) == ERR_INVALID and b"b2p must be 16-byte" in lib.dagl_last_error()
        assert _call(lib, True, at={f"b2p4[{h}]": _AT[f"b2p4[{h}]"] + 8}, ws_bytes=0, ws=None) == ERR_INVALID


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
        assert str((1 + 4 * propagate) * (fits + 1) * w2 + explore) in err and str(cap) in err and ENTRY in err, err
        assert _call(lib, step, width_in=fits + 1, ws_bytes=0, ws=None, **kw) == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("step", [False, True])
def test_outputs_may_not_overlap_inputs(lib, step):
    from dagl_amd import _lib
    B, H, W = SHAPE
    sizes = {"key_in": ROWS * WIDTH * 4, "deg_in": ROWS * 4, "x": B * 64 * N * 4, "mix_w": 64 * 64 * 4, "mix_b": 64 * 4,
             "out": B * 64 * N * 4, "key_out": ROWS * WIDTH * 4, "weight_out": ROWS * WIDTH * 4, "score_out": ROWS * WIDTH * 4,
             "deg_out": ROWS * 4}
    for h in range(4):
        sizes.update({f"wq_rows4[{h}]": HEAD_ROWS * 196 * 4, f"x_rows4[{h}]": B * N * 196 * 4, f"b2p4[{h}]": B * (H + 6) * (W + 6) * 16 * 4,
                      f"tau4[{h}]": HEAD_ROWS * 4})
    inputs = ["key_in", "deg_in"] + [f"{t}[{h}]" for t in ("wq_rows4", "x_rows4", "tau4") + (("b2p4",) if step else ()) for h in range(4)] \
        + (["x", "mix_w", "mix_b"] if step else [])
    outputs = ("key_out", "weight_out", "score_out", "deg_out") + (("out",) if step else ())
    for o in outputs:
        for i in inputs:
            # the output on the input, on its last 16 bytes, and ending 16 bytes into it: refused;  touching it end to start: served
            for at in (_AT[i], _AT[i] + sizes[i] - 16, _AT[i] - sizes[o] + 16):
                assert _call(lib, step, null=(), at={o: at}) == ERR_INVALID, (o, i, at)
                err = lib.dagl_last_error()
                assert b"overlaps" in err and ENTRY.encode() in err, err
            # (the step form only: its empty workspace stops the call, the graph alone needs none and would launch)
            for at in (_AT[i] + sizes[i], _AT[i] - sizes[o]):
                assert _call(lib, True, null=(), at={o: at}, ws_bytes=0) == _lib.ERR_WORKSPACE, (o, i, at)
    # the in-place update of a stage's graph is such an overlap: key_out on key_in, deg_out on deg_in
    assert _call(lib, step, at=dict(key_out=_AT["key_in"])) == ERR_INVALID and b"overlaps" in lib.dagl_last_error()
    assert _call(lib, step, at=dict(deg_out=_AT["deg_in"])) == ERR_INVALID and b"overlaps" in lib.dagl_last_error()
    # an output inside ANOTHER head's rows of the slot array (head 2's quarter of key_in)
    assert _call(lib, step, at=dict(score_out=_AT["key_in"] + 2 * HEAD_ROWS * WIDTH * 4)) == ERR_INVALID
    assert b"overlaps" in lib.dagl_last_error()


def test_workspace_one_short(lib):
    from dagl_amd import _lib
    B, H, W = SHAPE
    need = lib.dagl_graph_stage_step_fixed_workspace_bytes(B, H, W, 1)
    assert _call(lib, True, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert ENTRY in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    assert _call(lib, True, ws=_WS + 8) == ERR_INVALID and b"aligned" in lib.dagl_last_error()
    assert _call(lib, True, ws=None) == ERR_INVALID and b"workspace" in lib.dagl_last_error()


def test_the_single_head_entry_keeps_its_refusals(lib):
    """dagl_graph_step_fixed shares the checks: a call of each kind still ends where it did."""
    from dagl_amd import _lib
    a = {n: 0x20000000 + i * 0x1000000 for i, n in enumerate(("wq", "x", "b2p", "key", "deg", "out", "ko", "wo", "so", "do", "st"))}
    call = lambda **kw: lib.dagl_graph_step_fixed(None, 2, 24, 20, a["wq"], a["x"], kw.get("b2p", a["b2p"]), a["key"], a["deg"],
                                                  kw.get("width_in", WIDTH), 1, None, 0, C.c_float(10.0), 0, 0, 0, 3, a["out"],
                                                  kw.get("ko", a["ko"]), a["wo"], a["so"], a["do"], WIDTH, a["st"], _WS,
                                                  kw.get("ws_bytes", 1 << 40))
    assert call(ws_bytes=0) == _lib.ERR_WORKSPACE
    assert call(b2p=None) == ERR_INVALID and b"b2p and out come together" in lib.dagl_last_error()
    assert call(ko=a["key"]) == ERR_INVALID and b"overlaps" in lib.dagl_last_error()
    assert call(width_in=228) == _lib.ERR_UNSUPPORTED and b"dagl_graph_step_fixed:" in lib.dagl_last_error()
