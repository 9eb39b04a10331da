"""``dagl_graph_step`` / ``dagl_graph_step_workspace_bytes`` on the host alone: sizes, and every rejection the entry makes on fake pointers
before anything reaches the device, with the codes ``dagl_graph_refresh`` uses for the same mistakes."""
import ctypes as C

import pytest

_FAKE = 0x10000           # a fake device pointer, 16-byte aligned
_WS = 0x100000            # a 256-byte aligned fake workspace
B, H, W, E, RADIUS, K = 2, 24, 20, 480, 1, 8
CAP = B * 30 * K          # B L k < E (2 radius + 1)^2


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _step(lib, **kw):
    a = dict(wq=_FAKE, x=_FAKE, b2p=_FAKE, row_off=_FAKE, key=_FAKE, E=E, longest=12, radius=RADIUS, tau=None, k=K, scale=10.0, flags=0,
             out=_FAKE, row_off_out=_FAKE, key_out=_FAKE, weight_out=_FAKE, score_out=_FAKE, cap=CAP, status=_FAKE, ws=_WS, ws_bytes=1 << 40)
    a.update(kw)
    rc = lib.dagl_graph_step(None, B, H, W, a["wq"], a["x"], a["b2p"], a["row_off"], a["key"], a["E"], a["longest"], a["radius"], a["tau"],
                             a["k"], C.c_float(a["scale"]), a["flags"], a["out"], a["row_off_out"], a["key_out"], a["weight_out"],
                             a["score_out"], a["cap"], a["status"], a["ws"], a["ws_bytes"])
    return rc, lib.dagl_last_error()


_NO_GRAPH = dict(row_off_out=None, key_out=None, weight_out=None, score_out=None)


def test_workspace_bytes(lib):
    with_graph = lib.dagl_graph_step_workspace_bytes(B, H, W, E, RADIUS, 1)
    alone = lib.dagl_graph_step_workspace_bytes(B, H, W, E, RADIUS, 0)
    assert alone > 0 and with_graph > alone
    assert alone >= B * 30 * 784 * 4                                   # the aggregated rows
    assert with_graph - alone == lib.dagl_graph_refresh_workspace_bytes(B, H, W, E, RADIUS)      # the refresh's regions behind them
    assert lib.dagl_graph_step_workspace_bytes(B, H, W, 0, RADIUS, 0) > 0
    for bad, word in (((0, H, W, E, RADIUS, 1), b"bad shape"), ((B, 0, W, E, RADIUS, 0), b"bad shape"), ((B, H, W, -1, RADIUS, 1), b"total_edges"),
                      ((B, H, W, E, 9, 1), b"radius"), ((B, H, W, E, -1, 0), b"radius")):
        assert lib.dagl_graph_step_workspace_bytes(*bad) == 0
        err = lib.dagl_last_error()
        assert word in err and b"dagl_graph_step_workspace_bytes" in err, err


def test_rejections_before_the_device(lib):
    from dagl_amd import _lib
    for kw, code, word in ((dict(out=None), -1, b"null"), (dict(b2p=None), -1, b"null"), (dict(wq=None), -1, b"null"),
                           (dict(status=None), -1, b"null"),
                           (dict(b2p=_FAKE + 8), -1, b"b2p must be 16-byte aligned"), (dict(ws=_WS + 8), -1, b"aligned"),
                           (dict(x=_FAKE + 4), -1, b"aligned"),
                           (dict(longest=228), _lib.ERR_UNSUPPORTED, b"2052 candidates"),             # 228 x 9 > 2048
                           (dict(radius=9), -1, b"radius"), (dict(k=-1), -1, b"k=-1"), (dict(scale=0.0), -1, b"scale"),
                           (dict(flags=0x8), -1, b"flags"),
                           (dict(cap=CAP - 1), _lib.ERR_WORKSPACE, b"capacity"),
                           # only some of the four graph outputs
                           (dict(row_off_out=None), -1, b"null"), (dict(key_out=None), -1, b"null"), (dict(weight_out=None), -1, b"null"),
                           (dict(score_out=None), -1, b"null"), (dict(_NO_GRAPH, key_out=_FAKE), -1, b"null"),
                           (dict(_NO_GRAPH, score_out=_FAKE), -1, b"null")):
        rc, err = _step(lib, **kw)
        assert rc == code and word in err and b"dagl_graph_step" in err, (kw, rc, err)
    # the refresh entry gives the same codes for the mistakes both can make
    rc = lib.dagl_graph_refresh(None, B, H, W, _FAKE, _FAKE, _FAKE, _FAKE, E, 228, RADIUS, None, K, C.c_float(10.0), 0, _FAKE, _FAKE, _FAKE,
                                _FAKE, CAP, _FAKE, _WS, 1 << 40)
    assert rc == _lib.ERR_UNSUPPORTED
    rc = lib.dagl_graph_refresh(None, B, H, W, _FAKE, _FAKE, _FAKE, _FAKE, E, 12, RADIUS, None, K, C.c_float(10.0), 0, _FAKE, _FAKE, _FAKE,
                                _FAKE, CAP - 1, _FAKE, _WS, 1 << 40)
    assert rc == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("want_graph", [1, 0])
def test_a_workspace_one_byte_short(lib, want_graph):
    from dagl_amd import _lib
    need = lib.dagl_graph_step_workspace_bytes(B, H, W, E, RADIUS, want_graph)
    outs = {} if want_graph else dict(_NO_GRAPH, cap=0)              # (without graph outputs the capacity is not looked at)
    for short in (need - 1, 0):
        rc, err = _step(lib, ws_bytes=short, **outs)
        assert rc == _lib.ERR_WORKSPACE and b"workspace" in err and str(need).encode() in err, (rc, err)


def test_python_layer_refuses_on_the_host():
    """What ``ops.graph_step`` refuses from shapes alone (CPU tensors never reach the library: the device check comes first)."""
    import torch
    from dagl_amd import DaglError, ops
    wq, x = torch.zeros(1, 4, 196), torch.zeros(1, 64, 196)
    with pytest.raises(DaglError):
        ops.graph_step(wq, x, torch.zeros(1, 14, 14, 16), torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                       max_row_edges=0, want_graph=False)
