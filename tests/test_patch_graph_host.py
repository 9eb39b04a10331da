"""Host side of the graph export (no GPU): the ``PatchGraph`` container on hand-made CSR arrays, and what the three C entry points
(``dagl_ce_graph_workspace_bytes`` / ``_count`` / ``_fill``) reject before anything reaches the device."""
import ctypes as C

import pytest
import torch


# B = 2 images of 5 x 7 pixels: L = 2 x 2 = 4 queries, N = 35 keys; rows: [1, 5] [0] [] [34] | [] [2, 3, 4] [] []
_OFF = [0, 2, 3, 3, 4, 4, 7, 7, 7]
_KEY = [1, 5, 0, 34, 2, 3, 4]
_WGT = [0.5, 0.25, 1.0, 0.125, 0.1, 0.2, 0.3]


def _csr(with_score=False, **over):
    a = dict(row_off=torch.tensor(_OFF, dtype=torch.int64), key=torch.tensor(_KEY, dtype=torch.int32),
             weight=torch.tensor(_WGT, dtype=torch.float32), score=torch.arange(7, dtype=torch.float32) if with_score else None)
    a.update(over)
    return a


def _graph(with_score=False, **over):
    from dagl_amd import PatchGraph
    a = _csr(with_score, **over)
    return PatchGraph(a["row_off"], a["key"], a["weight"], a["score"], 2, 5, 7, "topk", 3)


def test_fields_degrees_rows():
    g = _graph(with_score=True)
    assert (g.B, g.L, g.N, g.H, g.W, g.mode, g.k, g.n_edges) == (2, 4, 35, 5, 7, "topk", 3, 7)
    assert g.degrees().dtype == torch.int64
    assert g.degrees().tolist() == [[2, 1, 0, 1], [0, 3, 0, 0]]
    key, wgt, sc = g.row(0, 0)
    assert key.tolist() == [1, 5] and wgt.tolist() == [0.5, 0.25] and sc.tolist() == [0.0, 1.0]
    key, wgt, sc = g.row(1, 1)
    assert key.tolist() == [2, 3, 4] and sc.tolist() == [4.0, 5.0, 6.0]
    assert key.data_ptr() == g.key.data_ptr() + 4 * 4                 # a view, not a copy
    assert g.row(0, 2)[0].numel() == 0
    assert _graph().row(0, 0)[2] is None
    for bad in ((2, 0), (0, 4), (-1, 0)):
        with pytest.raises(IndexError):
            g.row(*bad)


def test_to_dense_and_cpu():
    g = _graph()
    d0, d1 = g.to_dense(0), g.to_dense(1)
    assert d0.shape == (4, 35) and d0.dtype == torch.float32
    want0 = torch.zeros(4, 35); want0[0, 1], want0[0, 5], want0[1, 0], want0[3, 34] = 0.5, 0.25, 1.0, 0.125
    want1 = torch.zeros(4, 35); want1[1, 2], want1[1, 3], want1[1, 4] = 0.1, 0.2, 0.3
    assert torch.equal(d0, want0) and torch.equal(d1, want1)
    c = g.cpu()
    assert torch.equal(c.row_off, g.row_off) and torch.equal(c.key, g.key) and c.score is None and c.mode == "topk"


def test_to_dense_size_guard():
    from dagl_amd import DaglError, PatchGraph
    H = W = 256                                    # L x N = 4096 x 65536 = 2^28 entries
    g = PatchGraph(torch.zeros(4096 + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), None, 1, H, W)
    assert g.degrees().sum() == 0
    with pytest.raises(DaglError, match="to_dense"):
        g.to_dense(0)


@pytest.mark.parametrize("over, what", [
    (dict(row_off=torch.tensor(_OFF, dtype=torch.int32)), "dtype"),
    (dict(key=torch.tensor(_KEY, dtype=torch.int64)), "dtype"),
    (dict(weight=torch.tensor(_WGT, dtype=torch.float64)), "dtype"),
    (dict(score=torch.arange(7, dtype=torch.float64)), "dtype"),
    (dict(row_off=torch.tensor(_OFF[:-1], dtype=torch.int64)), "offsets"),
    (dict(row_off=torch.tensor([1] + _OFF[1:], dtype=torch.int64)), "start at 0"),
    (dict(row_off=torch.tensor([0, 2, 1, 3, 4, 4, 7, 7, 7], dtype=torch.int64)), "never decrease"),
    (dict(row_off=torch.tensor(_OFF[:-1] + [8], dtype=torch.int64)), "ends at 8"),
    (dict(weight=torch.tensor(_WGT[:-1], dtype=torch.float32)), "one entry per edge"),
    (dict(score=torch.arange(6, dtype=torch.float32)), "one entry per edge"),
    (dict(key=torch.tensor([_KEY], dtype=torch.int32)), "1-d"),
])
def test_constructor_rejects(over, what):
    from dagl_amd import DaglError
    with pytest.raises(DaglError, match=what):
        _graph(**over)


def test_constructor_rejects_shape_and_mode():
    from dagl_amd import DaglError, PatchGraph
    a = _csr()
    with pytest.raises(DaglError, match="bad shape"):
        PatchGraph(a["row_off"], a["key"], a["weight"], None, 0, 5, 7)
    with pytest.raises(DaglError, match="unknown mode"):
        PatchGraph(a["row_off"], a["key"], a["weight"], None, 2, 5, 7, "best")


# ---- the C entry points on fake pointers: rejected before anything reaches the device ----------------------------------------------------
_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake workspace


@pytest.fixture(scope="module")
def lib():
    from dagl_amd.build import build
    build()
    from dagl_amd import _lib
    return _lib.load()


def _count(lib, H, W, mode, k, ws, ws_bytes, info, null=(), rows=0):
    p = lambda name: None if name in null else _FAKE
    return lib.dagl_ce_graph_count(None, 1, H, W, p("b1"), p("thr"), p("bias"), p("fc1_w"), p("fc1_b"), p("fc2_w"), p("fc2_b"),
                                   mode, k, rows, p("row_off"), ws, ws_bytes, C.byref(info))


def _fill(lib, H, W, mode, k, ws, ws_bytes, null=(), total=100, capacity=100, rows=0):
    p = lambda name: None if name in null else _FAKE
    return lib.dagl_ce_graph_fill(None, 1, H, W, mode, k, rows, p("row_off"), p("key"), p("weight"), p("score"), total, capacity,
                                  ws, ws_bytes)


def test_graph_workspace_bytes(lib):
    small, large = lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 0, 0, 0), lib.dagl_ce_graph_workspace_bytes(1, 256, 256, 0, 0, 0)
    assert 0 < small < large
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 0, 0, 16) < small          # fewer score rows at a time
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 1, 5000, 0) == lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 1, 8, 0)
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 1, 0, 0) == 0 and b"k=0" in lib.dagl_last_error()
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 2, 0, 0) == 0 and b"k=0" in lib.dagl_last_error()
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 7, 0, 0) == 0 and b"unknown mode" in lib.dagl_last_error()
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 0x100, 0, 0) == 0 and b"unknown mode" in lib.dagl_last_error()   # (no flags here)
    assert lib.dagl_ce_graph_workspace_bytes(0, 64, 64, 0, 0, 0) == 0 and b"bad shape" in lib.dagl_last_error()
    assert lib.dagl_ce_graph_workspace_bytes(1, 64, 64, 0, 0, -1) == 0 and b"rows_per_chunk" in lib.dagl_last_error()


@pytest.mark.parametrize("H,W", [(64, 64), (45, 45)])
@pytest.mark.parametrize("mode,k", [(0, 0), (1, 8), (2, 8)])
def test_count_rejections(lib, H, W, mode, k):
    from dagl_amd import _lib
    need = lib.dagl_ce_graph_workspace_bytes(1, H, W, mode, k, 0)
    cases = [("null out", _WS, 1 << 40, ("row_off",)), ("null input", _WS, 1 << 40, ("b1",)), ("null weight", _WS, 1 << 40, ("fc2_b",)),
             ("misaligned workspace", _WS + 8, 1 << 40, ()), ("null workspace", None, 1 << 40, ()),
             ("no workspace", _WS, 0, ()), ("one byte short", _WS, need - 1, ())]
    if mode != 1:
        cases += [("null threshold input", _WS, 1 << 40, ("thr",)), ("null threshold input", _WS, 1 << 40, ("bias",))]
    for case, ws, ws_bytes, null in cases:
        info = _lib.CeInfo(*([77] * 7))
        rc = _count(lib, H, W, mode, k, ws, ws_bytes, info, null)
        err = lib.dagl_last_error()
        what = (case, H, W, mode, rc, err)
        assert info.required_bytes == need and info.total_edges == -1 and info.path == 8, what     # the size is reported either way
        if case in ("no workspace", "one byte short"):
            assert rc == _lib.ERR_WORKSPACE and b"workspace" in err and str(need).encode() in err, what
        else:
            assert rc == -1, what
            assert (b"aligned" in err) if "workspace" in case else (b"null" in err or b"required" in err), what
    info = _lib.CeInfo(*([77] * 7))
    if mode != 0:
        assert _count(lib, H, W, mode, 0, _WS, 1 << 40, info) == -1 and b"k=0" in lib.dagl_last_error()
    assert _count(lib, H, W, 5, k, _WS, 1 << 40, info) == -1 and b"unknown mode" in lib.dagl_last_error()
    if mode == 1:                                  # the fixed-k mode has no threshold heads: null thr / bias pass the pointer checks
        assert _count(lib, H, W, mode, k, _WS, need - 1, info, ("thr", "bias")) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("H,W", [(64, 64), (45, 45)])
@pytest.mark.parametrize("mode,k", [(0, 0), (1, 8)])
def test_fill_rejections(lib, H, W, mode, k):
    from dagl_amd import _lib
    need = lib.dagl_ce_graph_workspace_bytes(1, H, W, mode, k, 0)
    for case, ws, ws_bytes, null in [("null out", _WS, 1 << 40, ("key",)), ("null out", _WS, 1 << 40, ("weight",)),
                                     ("null input", _WS, 1 << 40, ("row_off",)), ("misaligned workspace", _WS + 8, 1 << 40, ()),
                                     ("null workspace", None, 1 << 40, ())]:
        rc = _fill(lib, H, W, mode, k, ws, ws_bytes, null)
        err = lib.dagl_last_error()
        assert rc == -1 and ((b"aligned" in err) if "workspace" in case else (b"null" in err)), (case, rc, err)
    for ws_bytes in (0, need - 1):
        rc = _fill(lib, H, W, mode, k, _WS, ws_bytes)
        err = lib.dagl_last_error()
        assert rc == _lib.ERR_WORKSPACE and b"workspace" in err and str(need).encode() in err, (ws_bytes, rc, err)
    # a capacity below the graph's edge count: an error that names both numbers, whatever else is wrong -- never a partial write
    rc = _fill(lib, H, W, mode, k, _WS, 1 << 40, total=1000, capacity=999)
    err = lib.dagl_last_error()
    assert rc == _lib.ERR_WORKSPACE and b"capacity 999" in err and b"1000 edges" in err, (rc, err)
    L, N = (-(-H // 4)) * (-(-W // 4)), H * W
    assert _fill(lib, H, W, mode, k, _WS, 1 << 40, total=L * N + 1, capacity=L * N + 1) == -1 and b"total_edges" in lib.dagl_last_error()
    assert _fill(lib, H, W, mode, k, _WS, 1 << 40, total=-1, capacity=10) == -1 and b"total_edges" in lib.dagl_last_error()
    if mode != 0:
        assert _fill(lib, H, W, mode, 0, _WS, 1 << 40) == -1 and b"k=0" in lib.dagl_last_error()
    assert _fill(lib, H, W, 9, k, _WS, 1 << 40) == -1 and b"unknown mode" in lib.dagl_last_error()
    assert _fill(lib, H, W, mode, k, _WS, 1 << 40, null=("score",), total=0, capacity=0) == 0        # an empty graph: nothing to write
