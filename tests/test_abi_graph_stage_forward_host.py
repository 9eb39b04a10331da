"""A whole CES stage on its frozen graph, forward and backward (dagl_graph_stage_forward*, dagl_ces_stage_mix_backward*;
csrc/graph_forward.hip, csrc/stage_mix_grad.hip) on fake pointers: every call below is rejected before anything reaches the device, as in
test_abi_stage_step_host.py.  The entries came in without an ABI bump: found by symbol."""
import os
import re

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace
SHAPE = (2, 24, 20)
E = 1920
_OPERANDS = ["wq_rows4", "x_rows4", "b2p4", "row_off", "key", "x", "mix_w", "mix_b", "out"]
_TRAIN = ["row_max_out", "row_sum_out", "cat_out"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _forward(lib, ws=_WS, ws_bytes=1 << 40, null=("tau4",) + tuple(_TRAIN), ptr=None, shape=SHAPE, edges=E, scale=10.0, flags=0):
    """``null``: the arguments passed as NULL (default: no margin, no training outputs); ``ptr``: {name: value} in the place of a fake
    pointer."""
    ptr = ptr or {}
    p = lambda n: None if n in null else ptr.get(n, _FAKE)
    B, H, W = shape
    return lib.dagl_graph_stage_forward(None, B, H, W, p("wq_rows4"), p("x_rows4"), p("b2p4"), p("row_off"), p("key"), edges, p("tau4"),
                                        scale, flags, p("x"), p("mix_w"), p("mix_b"), p("out"), p("row_max_out"), p("row_sum_out"),
                                        p("cat_out"), ws, ws_bytes)


def _backward(lib, ws=_WS, ws_bytes=1 << 40, null=(), ptr=None, shape=SHAPE):
    ptr = ptr or {}
    p = lambda n: None if n in null else ptr.get(n, _FAKE)
    B, H, W = shape
    return lib.dagl_ces_stage_mix_backward(None, B, H, W, p("d_out"), p("cat4"), p("mix_w"), p("d_cat4"), p("d_mix_w"), p("d_mix_b"), ws,
                                           ws_bytes)


def test_symbols_in_the_header_and_the_table(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name, n_args in (("dagl_graph_stage_forward_workspace_bytes", 4), ("dagl_graph_stage_forward", 22),
                         ("dagl_ces_stage_mix_backward_workspace_bytes", 3), ("dagl_ces_stage_mix_backward", 12)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert re.search(r"dagl_graph_stage_forward\*[^.]*dagl_ces_stage_mix_backward\*[^.]*without a bump", header)


def test_the_calls_pass_their_checks_as_far_as_the_workspace(lib):
    from dagl_amd import _lib
    assert _forward(lib, ws_bytes=0) == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    assert b"dagl_graph_stage_forward" in lib.dagl_last_error()
    assert _forward(lib, null=tuple(_TRAIN), ws_bytes=0) == _lib.ERR_WORKSPACE                       # with tau
    assert _forward(lib, null=("tau4",), ws_bytes=0) == _lib.ERR_WORKSPACE                           # the training flavour
    assert _forward(lib, null=(), ws_bytes=0) == _lib.ERR_WORKSPACE
    assert _forward(lib, null=("key", "tau4") + tuple(_TRAIN), edges=0, ws_bytes=0) == _lib.ERR_WORKSPACE     # no edges: key may be null
    assert _backward(lib, ws_bytes=0) == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    assert b"dagl_ces_stage_mix_backward" in lib.dagl_last_error()
    for null in (("d_mix_w",), ("d_mix_b",), ("d_mix_w", "d_mix_b"), ("d_mix_w", "d_mix_b", "cat4")):
        assert _backward(lib, null=null, ws_bytes=0) == _lib.ERR_WORKSPACE, null


def test_short_and_misaligned_workspaces(lib):
    from dagl_amd import _lib
    need = lib.dagl_graph_stage_forward_workspace_bytes(*SHAPE, E)
    assert need > 0 and _forward(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.dagl_last_error()
    assert _forward(lib, ws=_WS + 8) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _forward(lib, ws=None) == -1 and b"workspace" in lib.dagl_last_error()
    need = lib.dagl_ces_stage_mix_backward_workspace_bytes(*SHAPE)
    assert need > 0 and _backward(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.dagl_last_error()
    assert _backward(lib, ws=_WS + 8) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _backward(lib, ws=None) == -1 and b"workspace" in lib.dagl_last_error()


@pytest.mark.parametrize("name", _OPERANDS)
def test_forward_null_pointers(lib, name):
    for tau in ((), ("tau4",)):
        assert _forward(lib, null=(name,) + tau + tuple(_TRAIN)) == -1
        assert b"null" in lib.dagl_last_error() and b"dagl_graph_stage_forward" in lib.dagl_last_error()
        assert _forward(lib, null=(name,) + tau + tuple(_TRAIN), ws_bytes=0) == -1              # ... before the workspace is looked at


@pytest.mark.parametrize("name", ["wq_rows4", "x_rows4", "b2p4"])
def test_forward_misaligned_pointers(lib, name):
    assert _forward(lib, ptr={name: _FAKE + 8}) == -1 and b"16-byte aligned" in lib.dagl_last_error()
    assert _forward(lib, ptr={name: _FAKE + 8}, ws_bytes=0) == -1
    if name == "b2p4":
        assert b"b2p" in lib.dagl_last_error()


def test_training_outputs_come_together(lib):
    for given in range(1, 7):                                      # every proper, non-empty subset of the three
        null = tuple(n for i, n in enumerate(_TRAIN) if not given >> i & 1) + ("tau4",)
        assert _forward(lib, null=null) == -1, null
        assert b"come together" in lib.dagl_last_error() and b"dagl_graph_stage_forward" in lib.dagl_last_error()
        assert _forward(lib, null=null, ws_bytes=0) == -1


def test_forward_shape_flags_scale(lib):
    for shape in ((0, 24, 20), (2, 0, 20), (2, 24, 0), (-1, 24, 20)):
        assert _forward(lib, shape=shape) == -1 and b"bad shape" in lib.dagl_last_error()
        assert lib.dagl_graph_stage_forward_workspace_bytes(*shape, E) == 0 and b"bad shape" in lib.dagl_last_error()
    # the rows of 4 B images are 32-bit: 2^28 pixels pass for one head, not for four
    big = (1, 1 << 14, 1 << 14)
    assert _forward(lib, shape=big) == -1 and b"too large" in lib.dagl_last_error()
    assert lib.dagl_graph_stage_forward_workspace_bytes(*big, E) == 0 and b"too large" in lib.dagl_last_error()
    for edges in (-1, 1 << 31):
        assert _forward(lib, edges=edges) == -1 and b"total_edges" in lib.dagl_last_error()
        assert lib.dagl_graph_stage_forward_workspace_bytes(*SHAPE, edges) == 0 and b"total_edges" in lib.dagl_last_error()
    for flags in (0x2, 0x8, -1):
        assert _forward(lib, flags=flags) == -1 and b"unknown flags" in lib.dagl_last_error()
    assert _forward(lib, flags=1, ws_bytes=0) == -2                                          # the edges-only normalisation is known
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _forward(lib, scale=scale) == -1 and b"scale" in lib.dagl_last_error()


def test_forward_sizes_grow(lib):
    size = lib.dagl_graph_stage_forward_workspace_bytes
    assert 0 < size(1, 24, 20, 0) < size(1, 24, 20, E) < size(1, 24, 20, 40 * E)
    assert size(1, 24, 20, E) < size(2, 24, 20, E) < size(3, 24, 20, E)
    # the rows of four heads: what the single-head forward asks for 4 B images
    assert size(2, 24, 20, E) == lib.dagl_graph_forward_workspace_bytes(8, 24, 20, E)


@pytest.mark.parametrize("name", ["d_out", "mix_w", "d_cat4", "cat4"])
def test_backward_null_pointers(lib, name):
    assert _backward(lib, null=(name,)) == -1
    assert b"null" in lib.dagl_last_error() and b"dagl_ces_stage_mix_backward" in lib.dagl_last_error()
    assert _backward(lib, null=(name,), ws_bytes=0) == -1
    if name == "cat4":                                             # needed by either parameter gradient
        assert _backward(lib, null=(name, "d_mix_w")) == -1 and _backward(lib, null=(name, "d_mix_b")) == -1


@pytest.mark.parametrize("name", ["d_out", "cat4", "d_cat4"])
def test_backward_misaligned_pointers(lib, name):
    assert _backward(lib, ptr={name: _FAKE + 4}) == -1 and b"16-byte aligned" in lib.dagl_last_error()
    assert _backward(lib, ptr={name: _FAKE + 4}, ws_bytes=0) == -1


def test_backward_shape_and_sizes(lib):
    size = lib.dagl_ces_stage_mix_backward_workspace_bytes
    for shape in ((0, 24, 20), (2, 0, 20), (2, 24, 0)):
        assert _backward(lib, shape=shape) == -1 and b"bad shape" in lib.dagl_last_error()
        assert size(*shape) == 0 and b"bad shape" in lib.dagl_last_error()
    big = (1, 1 << 14, 1 << 14)
    assert _backward(lib, shape=big) == -1 and b"too large" in lib.dagl_last_error() and size(*big) == 0
    # one slot of 64 x 64 + 64 floats per wave, four waves per block, a block per 4096 pixels, at most 128 blocks: B H W alone
    slot = 4 * (64 * 64 + 64) * 4
    blocks = lambda B, H, W: min(128, -(-B * H * W // 4096))
    for shape in ((1, 9, 6), (1, 24, 20), (2, 24, 20), (1, 64, 64), (1, 65, 64), (3, 100, 100), (1, 1024, 1024), (4, 1024, 1024)):
        assert size(*shape) == -(-blocks(*shape) * slot // 256) * 256, shape
    assert size(1, 64, 64) < size(1, 65, 64) < size(2, 65, 64) and size(1, 1024, 1024) == size(4, 1024, 1024)
    assert size(2, 32, 64) == size(1, 64, 64) == size(1, 32, 128)
