"""The read-out entry of the split-fp16 g / theta kernel (dagl_ce_prologue16_debug, csrc/capi.hip) on fake pointers: every call below is
rejected before anything reaches the device, as in test_abi_graph_forward_host.py.  The entry came in without an ABI bump: it is found by
symbol."""
import ctypes as C

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake scratch
_TABLES = ["x", "g_w", "g_b", "theta_w", "theta_b"]
_REQUIRED = ["b2", "hi", "lo", "amax", "range"]


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _debug(lib, heads=2, imgs=3, H=7, W=65, null=(), null_head=None, null_table=(), tag=5, ws=_WS, ws_bytes=1 << 40, n=8, fake=_FAKE):
    """One call; ``null``: outputs passed as NULL, ``null_table``: pointer tables passed as NULL, ``null_head`` = (table, head): one entry."""
    def table(name):
        if name in null_table:
            return None
        vals = [fake] * max(heads, 1)
        if null_head is not None and null_head[0] == name:
            vals[null_head[1]] = None
        return (C.c_void_p * len(vals))(*vals)
    p = lambda name: None if name in null else fake
    return lib.dagl_ce_prologue16_debug(None, heads, imgs, H, W, *[table(t) for t in _TABLES], tag, ws, ws_bytes, p("b1"), p("b2"), p("hi"),
                                        p("lo"), p("hi2"), p("lo2"), p("amax"), p("range"), p("clear"), n)


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    assert len(_lib.SIGNATURES["dagl_ce_prologue16_debug"][1]) == 23


def test_scratch_size(lib):
    size = lib.dagl_ce_prologue16_debug_scratch_bytes
    assert size(1) == 20 * 16 * 128 + 256 and [size(h) for h in (2, 3, 4)] == [h * size(1) for h in (2, 3, 4)]
    assert size(0) == 0 and size(5) == 0


def test_bad_shapes(lib):
    for kw in (dict(heads=0), dict(heads=5), dict(imgs=0), dict(H=0), dict(W=0)):
        assert _debug(lib, **kw) == -1, kw
        assert b"bad shape" in lib.dagl_last_error()


@pytest.mark.parametrize("name", _TABLES)
def test_null_inputs(lib, name):
    assert _debug(lib, null_table=(name,)) == -1 and b"null pointer table" in lib.dagl_last_error()
    for head in (0, 1):
        assert _debug(lib, null_head=(name, head), ws_bytes=0) == -1          # ... before the scratch is looked at
        assert ("null input of head %d" % head).encode() in lib.dagl_last_error()


@pytest.mark.parametrize("name", _REQUIRED)
def test_null_outputs(lib, name):
    assert _debug(lib, null=(name,), ws_bytes=0) == -1
    assert b"null output" in lib.dagl_last_error()


def test_tier_pair_tag_and_clear_words(lib):
    assert _debug(lib, null=("hi2",)) == -1 and b"both planes or neither" in lib.dagl_last_error()
    assert _debug(lib, null=("lo2",)) == -1 and b"both planes or neither" in lib.dagl_last_error()
    assert _debug(lib, tag=0) == -1 and b"tag" in lib.dagl_last_error()
    assert _debug(lib, n=-1) == -1 and b"words to clear" in lib.dagl_last_error()
    assert _debug(lib, null=("clear",), n=1) == -1 and b"words to clear" in lib.dagl_last_error()


def test_misaligned_operands(lib):
    assert _debug(lib, fake=_FAKE + 8) == -1
    assert b"16-byte aligned" in lib.dagl_last_error()
    assert _debug(lib, ws=_WS + 16) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _debug(lib, ws=None) == -1 and b"aligned" in lib.dagl_last_error()


def test_scratch_one_byte_short(lib):
    from dagl_amd import _lib
    need = lib.dagl_ce_prologue16_debug_scratch_bytes(2)
    assert _debug(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_ce_prologue16_debug" in err and "required %d B" % need in err, err


def test_nullable_arguments(lib):
    """What may be null gets as far as the last check before the device, the scratch size (-2)."""
    assert _debug(lib, null=("b1",), ws_bytes=0) == -2
    assert _debug(lib, null=("hi2", "lo2"), ws_bytes=0) == -2
    assert _debug(lib, null=("clear",), n=0, ws_bytes=0) == -2
    assert _debug(lib, heads=4, imgs=1, H=1, W=1, ws_bytes=0) == -2
