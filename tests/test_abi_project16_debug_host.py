"""The read-out entry of the split-fp16 patch projection (dagl_ce_project16_debug, csrc/capi.hip) on fake pointers: every call below is
rejected before anything reaches the device, as in test_abi_prologue16_debug_host.py.  The entry came in without an ABI bump: it is found
by symbol."""
import ctypes as C

import pytest

_FAKE = 0x10000
_WS = 0x100000            # a 256-byte aligned fake scratch
_KEY_TABLES, _QUERY_TABLES, _THR_TABLES = ["fc2_w", "fc2_b"], ["fc1_w", "fc1_b"], ["thr_x", "thr_w", "bias_w"]
_KEY_OUT = ["x", "x_bf16", "x_hi", "x_lo", "colsum", "colpart", "rowsum"]
_QUERY_OUT = ["wq", "wq_bf16", "wq_hi", "wq_lo"]
_OPTIONAL = ["hi2", "lo2", "amax", "policy", "thr_part"] + _THR_TABLES


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def _debug(lib, heads=2, imgs=3, H=8, W=36, which=3, null=(), null_head=None, on=(), tag=5, ws=_WS, ws_bytes=1 << 40, slots=8, fake=_FAKE,
           odd=()):
    """One call.  Everything required and every output is passed unless named in ``null``; the optional inputs (coarse planes, slots,
    policy word, ride-along) only when named in ``on``; ``null_head`` = (table, head): one NULL entry; ``odd``: pointers passed + 8."""
    def present(name):
        if name in null:
            return False
        if name in _OPTIONAL:
            return name in on
        if name in _KEY_TABLES + _KEY_OUT:
            return bool(which & 1)
        if name in _QUERY_TABLES + _QUERY_OUT:
            return bool(which & 2)
        return True

    def table(name):
        if not present(name):
            return None
        vals = [fake] * max(heads, 1)
        if null_head is not None and null_head[0] == name:
            vals[null_head[1]] = None
        return (C.c_void_p * len(vals))(*vals)

    p = lambda name: (fake + (8 if name in odd else 0)) if present(name) else None
    return lib.dagl_ce_project16_debug(None, heads, imgs, H, W, which, p("hi"), p("lo"), p("hi2"), p("lo2"), p("amax"), slots,
                                       table("fc1_w"), table("fc1_b"), table("fc2_w"), table("fc2_b"), tag, p("range"), ws, ws_bytes,
                                       p("x"), p("wq"), p("x_bf16"), p("wq_bf16"), 1, p("x_hi"), p("x_lo"), p("wq_hi"), p("wq_lo"),
                                       p("colsum"), p("colpart"), p("rowsum"), p("policy"), table("thr_x"), table("thr_w"),
                                       table("bias_w"), p("thr_part"))


_TIERS = ("hi2", "lo2", "amax")
_RIDE = ("thr_x", "thr_w", "bias_w", "thr_part")


def test_version_is_unchanged(lib):
    from dagl_amd import _lib
    assert lib.dagl_version() == _lib.ABI_VERSION == 412
    assert len(_lib.SIGNATURES["dagl_ce_project16_debug"][1]) == 37


def test_scratch_size(lib):
    size = lib.dagl_ce_project16_debug_scratch_bytes
    assert size(1) == 2 * 2 * (49 * 7168 + 1024) and [size(h) for h in (2, 3, 4)] == [h * size(1) for h in (2, 3, 4)]
    assert size(1) % 256 == 0 and size(0) == 0 and size(5) == 0


def test_bad_shapes(lib):
    for kw in (dict(heads=0), dict(heads=5), dict(imgs=0), dict(H=0), dict(W=0), dict(which=0), dict(which=4)):
        assert _debug(lib, **kw) == -1, kw
        assert b"bad shape" in lib.dagl_last_error()


@pytest.mark.parametrize("name", _KEY_TABLES + _QUERY_TABLES)
def test_null_inputs(lib, name):
    assert _debug(lib, null=(name,)) == -1 and b"null pointer table" in lib.dagl_last_error()
    for head in (0, 1):
        assert _debug(lib, null_head=(name, head), ws_bytes=0) == -1          # ... before the scratch is looked at
        assert ("null input of head %d" % head).encode() in lib.dagl_last_error()
    # the tables of a side `which` leaves out are not looked at
    other = 2 if name in _KEY_TABLES else 1
    assert _debug(lib, which=other, ws_bytes=0) == -2


@pytest.mark.parametrize("name", ["hi", "lo"])
def test_null_planes(lib, name):
    assert _debug(lib, null=(name,), ws_bytes=0) == -1 and b"null plane" in lib.dagl_last_error()


@pytest.mark.parametrize("name", ["range", "x", "wq"])
def test_null_outputs(lib, name):
    assert _debug(lib, null=(name,), ws_bytes=0) == -1
    assert b"null output" in lib.dagl_last_error()


def test_outputs_of_a_side_left_out(lib):
    for which, names in ((2, _KEY_OUT), (1, _QUERY_OUT)):
        for name in names:
            assert _call_with_extra(lib, which, name) == -1 and b"leaves out" in lib.dagl_last_error(), (which, name)
        assert _call_with_extra(lib, which, None) == -2


def _call_with_extra(lib, which, extra):
    """A call of ``which`` that also passes the output ``extra`` of the other side."""
    keys, queries = bool(which & 1), bool(which & 2)
    p = lambda name, on: _FAKE if on or name == extra else None
    t = lambda on: (C.c_void_p * 2)(_FAKE, _FAKE) if on else None
    return lib.dagl_ce_project16_debug(None, 2, 3, 8, 36, which, _FAKE, _FAKE, None, None, None, 0, t(queries), t(queries), t(keys), t(keys),
                                       5, _FAKE, _WS, 0, p("x", keys), p("wq", queries), p("x_bf16", keys), p("wq_bf16", queries), 0,
                                       p("x_hi", keys), p("x_lo", keys), p("wq_hi", queries), p("wq_lo", queries), p("colsum", keys),
                                       p("colpart", keys), p("rowsum", keys), None, None, None, None, None)


def test_tiers_and_slots(lib):
    assert _debug(lib, on=("hi2", "amax")) == -1 and b"both planes or neither" in lib.dagl_last_error()
    assert _debug(lib, on=("lo2", "amax")) == -1 and b"both planes or neither" in lib.dagl_last_error()
    assert _debug(lib, on=("hi2", "lo2")) == -1 and b"slots come with the coarse tier" in lib.dagl_last_error()
    assert _debug(lib, on=("amax",)) == -1 and b"slots come with the coarse tier" in lib.dagl_last_error()
    for slots in (0, 3, 6, 1027, -4):
        assert _debug(lib, on=_TIERS, slots=slots) == -1 and b"a multiple of 4, at least 4" in lib.dagl_last_error(), slots
    for slots in (4, 8, 1028):
        assert _debug(lib, on=_TIERS, slots=slots, ws_bytes=0) == -2
    assert _debug(lib, slots=3, ws_bytes=0) == -2                          # without the tier the count is not looked at


def test_pairs_policy_and_tag(lib):
    for name in ("x_hi", "x_lo", "wq_hi", "wq_lo"):
        assert _debug(lib, null=(name,)) == -1 and b"both halves or neither" in lib.dagl_last_error(), name
    for name in ("colsum", "colpart"):
        assert _debug(lib, null=(name,)) == -1 and b"come together" in lib.dagl_last_error(), name
    assert _debug(lib, null=("rowsum",), on=("policy",)) == -1 and b"policy word without rowsum" in lib.dagl_last_error()
    assert _debug(lib, tag=0) == -1 and b"tag" in lib.dagl_last_error()


def test_ride_along(lib):
    for name in _RIDE:
        assert _debug(lib, on=tuple(n for n in _RIDE if n != name)) == -1 and b"ride-along is x, both weights" in lib.dagl_last_error(), name
    for name in _THR_TABLES:
        assert _debug(lib, on=_RIDE, null_head=(name, 1), ws_bytes=0) == -1 and b"null input of head 1" in lib.dagl_last_error()
    assert _debug(lib, on=_RIDE, ws_bytes=0) == -2                         # W = 36: served
    for W in (38, 33, 3):                                                  # thr_bias4_ok says no: W % 4 != 0
        assert _debug(lib, on=_RIDE, W=W, ws_bytes=0) == -1 and b"ride-along needs W % 4 == 0" in lib.dagl_last_error(), W
    x4 = (C.c_void_p * 2)(_FAKE, _FAKE + 4)                                # ... or a head's x off the 16-byte grid
    t = (C.c_void_p * 2)(_FAKE, _FAKE)
    rc = lib.dagl_ce_project16_debug(None, 2, 3, 8, 36, 3, _FAKE, _FAKE, None, None, None, 0, t, t, t, t, 5, _FAKE, _WS, 0, _FAKE, _FAKE,
                                     None, None, 0, None, None, None, None, None, None, None, None, x4, t, t, _FAKE)
    assert rc == -1 and b"ride-along needs" in lib.dagl_last_error()


def test_misaligned_operands(lib):
    for name in ("hi", "lo", "x", "wq", "x_bf16", "wq_bf16", "x_hi", "x_lo", "wq_hi", "wq_lo", "colsum", "colpart", "rowsum"):
        assert _debug(lib, odd=(name,)) == -1 and b"16-byte aligned" in lib.dagl_last_error(), name
    for name in _TIERS:
        assert _debug(lib, on=_TIERS, odd=(name,)) == -1 and b"16-byte aligned" in lib.dagl_last_error(), name
    assert _debug(lib, ws=_WS + 16) == -1 and b"256-byte aligned" in lib.dagl_last_error()
    assert _debug(lib, ws=None) == -1 and b"aligned" in lib.dagl_last_error()


def test_scratch_one_byte_short(lib):
    from dagl_amd import _lib
    need = lib.dagl_ce_project16_debug_scratch_bytes(2)
    assert _debug(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
    err = lib.dagl_last_error().decode()
    assert "dagl_ce_project16_debug" in err and "required %d B" % need in err, err


def test_nullable_arguments(lib):
    """What may be null gets as far as the last check before the device, the scratch size (-2)."""
    assert _debug(lib, null=("x_bf16", "wq_bf16"), ws_bytes=0) == -2
    assert _debug(lib, null=("x_hi", "x_lo"), ws_bytes=0) == -2
    assert _debug(lib, null=("wq_hi", "wq_lo", "colsum", "colpart", "rowsum"), ws_bytes=0) == -2
    assert _debug(lib, on=("policy",), ws_bytes=0) == -2
    assert _debug(lib, heads=4, imgs=1, H=1, W=1, which=1, ws_bytes=0) == -2
    assert _debug(lib, heads=1, imgs=1, H=1, W=1, which=2, ws_bytes=0) == -2
