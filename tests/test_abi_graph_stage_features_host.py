"""The features of a whole CES stage (dagl_graph_stage_features16, csrc/stage_features.hip) on fake pointers: every call below is
rejected before anything reaches the device, as in test_abi_graph_stage_step_fixed_host.py.  The entries came in without an ABI bump:
found by symbol."""
import ctypes as C
import os
import re

import pytest

_WS = 0x100000            # a 256-byte aligned fake workspace
ERR_INVALID = -1          # DAGL_ERR_INVALID
ERR_WORKSPACE = -2
SHAPE = (2, 24, 20)
ENTRY = "dagl_graph_stage_features16"
SIZE = "dagl_graph_stage_features16_workspace_bytes"
_ARRAYS = ("x", "wq_rows", "x_rows", "b2p", "tau")
_WEIGHTS = ("g_w", "g_b", "theta_w", "theta_b", "thr_w", "thr_b", "bias_w", "bias_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
_MARGIN_ONLY = ("thr_w", "thr_b", "bias_w", "bias_b")
# fake arrays 16 MiB apart
_AT = {n: 0x10000000 + i * 0x1000000 for i, n in enumerate(list(_ARRAYS) + [f"{w}[{h}]" for h in range(4) for w in _WEIGHTS])}


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _call(lib, heads=4, shape=SHAPE, margin=1, null=(), at=None, ws=_WS, ws_bytes=1 << 40, table=True):
    """``null``: arguments (an array by its name, a weight of head h as ``name[h]``) passed as NULL; ``at``: other addresses; ``margin``
    0 drops ``tau`` unless ``at`` names it."""
    from dagl_amd import _lib
    where = dict(_AT, **(at or {}))
    null = tuple(null) + (("tau",) if not margin and "tau" not in (at or {}) else ())
    p = lambda n: None if n in null else where[n]
    arr = (_lib.CeWeights * 4)()
    for h in range(4):
        for w in _WEIGHTS:
            setattr(arr[h], w, p(f"{w}[{h}]"))
    B, H, W = shape
    return lib.dagl_graph_stage_features16(None, heads, B, H, W, p("x"), arr if table else None, margin, p("wq_rows"), p("x_rows"), p("b2p"),
                                           p("tau"), ws, ws_bytes)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    assert re.search(r"#define\s+DAGL_ABI_VERSION\s+412\b", header)
    for name in (SIZE, ENTRY):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    decl = re.search(r"int\s+dagl_graph_stage_features16\((.*?)\);", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.POINTER(_lib.CeWeights) if "dagl_ce_weights*" in arg else _lib._vp if "*" in arg
                     else C.c_size_t if arg.startswith("size_t ") else C.c_int)
    assert kinds == _lib.SIGNATURES[ENTRY][1] and len(kinds) == 14
    assert _lib.SIGNATURES[SIZE] == (C.c_size_t, [C.c_int] * 5)
    assert re.search(r"size_t\s+" + SIZE + r"\(int heads, int B, int H, int W, int margin\);", header)


def test_workspace_bytes(lib):
    planner = getattr(lib, SIZE)
    B, H, W = SHAPE
    for margin in (0, 1):
        sizes = [planner(4, b, H, W, margin) for b in (1, 2, 3, 5, 8)]
        assert all(a > 0 and a % 256 == 0 for a in sizes) and all(b > a for a, b in zip(sizes, sizes[1:])), sizes      # grows with B
        sizes = [planner(4, B, h, w, margin) for h, w in ((1, 1), (5, 9), (8, 33), (24, 20), (45, 38), (256, 256))]
        assert all(a > 0 for a in sizes) and all(b > a for a, b in zip(sizes, sizes[1:])), sizes                       # ... and with H W
        sizes = [planner(n, B, H, W, margin) for n in (1, 2, 3, 4)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes                                                     # ... and the heads
    for shape in ((1, 1, 1), SHAPE, (1, 45, 38)):
        assert planner(4, *shape, 1) > planner(4, *shape, 0) > 0, shape                                                # ... and with margin
    # at least the padded feature rows of both sides
    L, N = 6 * 5, H * W
    rows = lambda n: -(-n // 32) * 32 + 32
    assert planner(4, B, H, W, 0) > 4 * B * (rows(N) + rows(L)) * 204 * 4
    for bad in ((4, 0, H, W), (4, B, 0, W), (4, B, H, 0), (4, -1, H, W)):
        assert planner(*bad, 1) == 0
        err = lib.dagl_last_error()
        assert b"bad shape" in err and SIZE.encode() in err, err
    for heads in (0, 5, -1):
        assert planner(heads, B, H, W, 1) == 0
        err = lib.dagl_last_error()
        assert b"heads=" in err and SIZE.encode() in err, err
    assert planner(4, 1, 16384, 16384, 1) == 0 and b"row ids" in lib.dagl_last_error()      # heads B H W must fit the row ids
    assert planner(1, 1, 16384, 16384, 1) > 0


def test_the_call_passes_its_checks_as_far_as_the_workspace(lib):
    for kw in (dict(), dict(margin=0), dict(heads=1), dict(heads=3, margin=0), dict(shape=(1, 1, 1)), dict(shape=(1, 7, 31)),
               # heads the call does not use, thr / bias heads without the margin: not looked at
               dict(heads=2, null=("g_w[2]", "fc1_w[3]")), dict(margin=0, null=tuple(f"{w}[{h}]" for w in _MARGIN_ONLY for h in range(4)))):
        assert _call(lib, ws_bytes=0, **kw) == ERR_WORKSPACE, kw
        err = lib.dagl_last_error()
        assert b"workspace" in err and ENTRY.encode() in err, err


def test_refusals_in_their_order(lib):
    who = ENTRY.encode() + b":"
    B, H, W = SHAPE
    cases = [(dict(shape=(0, H, W)), b"bad shape"), (dict(shape=(B, 0, W)), b"bad shape"), (dict(shape=(B, H, -3)), b"bad shape"),
             (dict(heads=0), b"heads=0"), (dict(heads=5), b"heads=5"), (dict(heads=-2), b"heads=-2"),
             (dict(shape=(1, 16384, 16384)), b"row ids")]
    cases += [(dict(null=(n,)), b"null tensor pointer") for n in ("x", "wq_rows", "x_rows", "b2p")]
    cases += [(dict(table=False), b"null tensor pointer")]
    cases += [(dict(null=(f"{w}[{h}]",)), f"head {h} has a null".encode()) for h in range(4) for w in _WEIGHTS]
    cases += [(dict(margin=0, null=(f"{w}[{h}]",)), f"head {h} has a null".encode()) for h in (0, 3) for w in _WEIGHTS
              if w not in _MARGIN_ONLY]
    cases += [(dict(null=("tau",)), b"tau and margin come together"), (dict(margin=0, at={"tau": _AT["tau"]}), b"tau and margin come together")]
    cases += [(dict(at={n: _AT[n] + off}), b"16-byte aligned") for n in _ARRAYS for off in (4, 8)]
    for kw, word in cases:
        assert _call(lib, **kw) == ERR_INVALID, kw
        err = lib.dagl_last_error()
        assert word in err and who in err, (kw, err)
        assert _call(lib, ws_bytes=0, ws=None, **kw) == ERR_INVALID, kw       # ... before the workspace is looked at
        assert word in lib.dagl_last_error(), kw
    # the order: shape, heads, null arrays, null weights, tau / margin, alignment
    chain = [(dict(shape=(0, H, W)), b"bad shape"), (dict(heads=5), b"heads=5"), (dict(null=("x",)), b"null tensor pointer"),
             (dict(null=("g_b[1]",)), b"head 1 has a null"), (dict(null=("tau",)), b"come together"),
             (dict(at={"b2p": _AT["b2p"] + 4}), b"16-byte aligned")]
    for i, (_, word) in enumerate(chain):
        kw, null = {}, ()
        for later, _w in chain[i:]:                     # this fault and every later one in the same call: this one is named
            null += tuple(later.get("null", ()))
            kw.update({k: v for k, v in later.items() if k != "null"})
        assert _call(lib, null=null, **kw) == ERR_INVALID, kw
        assert word in lib.dagl_last_error(), (i, kw, lib.dagl_last_error())


def test_workspace_one_short(lib):
    B, H, W = SHAPE
    for heads, margin in ((4, 1), (4, 0), (1, 1)):
        need = getattr(lib, SIZE)(heads, B, H, W, margin)
        assert _call(lib, heads=heads, margin=margin, ws_bytes=need - 1) == ERR_WORKSPACE
        err = lib.dagl_last_error().decode()
        assert ENTRY in err and int(re.search(r"required (\d+) B", err).group(1)) == need, err
    assert _call(lib, ws=_WS + 8) == ERR_INVALID and b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, ws=_WS + 128) == ERR_INVALID and b"256-byte aligned" in lib.dagl_last_error()
    assert _call(lib, ws=None) == ERR_INVALID and b"workspace" in lib.dagl_last_error()
