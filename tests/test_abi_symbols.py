"""CPU-side checks of the C-ABI boundary: the shared library loads and exports every symbol the header declares."""
import ctypes
import os
import re

import pytest

from tests.helpers import REPO


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "dagl_ce.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dagl_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from dagl_amd.build import build
    return build()


def test_header_declares_the_path():
    syms = _declared_symbols()
    for must in ("dagl_ce_forward", "dagl_ce_workspace_bytes", "dagl_gather_aggregate", "dagl_last_error",
                 "dagl_project_patches", "dagl_fold_normalize", "dagl_ce_pivot_debug", "dagl_ce_wide_debug",
                 "dagl_ce_prologue16_plan", "dagl_ce_prologue16_debug", "dagl_conv_pair_backward_plan",
                 "dagl_project16_plan", "dagl_ce_project16_debug", "dagl_ce_project16_debug_scratch_bytes"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for s in _declared_symbols():
        assert hasattr(lib, s), f"{s} declared in include/dagl_ce.h but not exported"


def test_python_binding_covers_header(lib_path):
    from dagl_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared_symbols()
    lib = _lib.load()
    assert lib.dagl_version() >= 100


def test_host_side_argument_errors(lib_path):
    """No-GPU behaviour of the boundary: planning works, bad arguments give error codes + messages."""
    from dagl_amd import _lib
    lib = _lib.load()
    assert lib.dagl_ce_workspace_bytes(1, 64, 64, 0, 0) > 0
    assert lib.dagl_ce_workspace_bytes(1, 256, 256, 1, 8) > lib.dagl_ce_workspace_bytes(1, 64, 64, 1, 8)
    assert lib.dagl_ce_workspace_bytes(1, 64, 64, 1, 0) == 0          # k missing in top-k mode
    assert b"k=0" in lib.dagl_last_error()
    assert lib.dagl_ce_workspace_bytes(1, 64, 64, 7, 0) == 0          # unknown mode
    assert lib.dagl_ce_workspace_bytes(0, 64, 64, 0, 0) == 0
    assert lib.dagl_gather_aggregate(None, 4, 8, 783, None, None, None, None) == -1
    assert lib.dagl_feat_rows(100) == 160


_FAKE = 0x10000           # a fake device pointer: every call below is rejected before anything reaches the device
_WS = 0x100000            # a 256-byte aligned fake workspace
_FORWARD_ENTRIES = ("dagl_ce_forward", "dagl_ce_forward_debug", "dagl_ce_forward_profiled", "dagl_ce_forward_fused",
                    "dagl_ces_stage_forward", "dagl_ce_core_forward", "dagl_ce_core_dense_forward")
_FIRST_INPUT = {"dagl_ce_forward": "b1", "dagl_ce_forward_debug": "b1", "dagl_ce_forward_profiled": "b1",
                "dagl_ce_forward_fused": "x", "dagl_ces_stage_forward": "x", "dagl_ce_core_forward": "wq_rows",
                "dagl_ce_core_dense_forward": "wq_rows"}
_THRESHOLD_INPUT = {"dagl_ce_forward_fused": "thr_w", "dagl_ces_stage_forward": "thr_w", "dagl_ce_core_forward": "mu",
                    "dagl_ce_core_dense_forward": "mu"}


def _forward_call(lib, entry, H, W, mode, k, ws, ws_bytes, info, null=()):
    """One call of a forward entry point on fake pointers; the inputs named in ``null`` are null."""
    import ctypes as C
    from dagl_amd import _lib
    p = lambda name: None if name in null else _FAKE
    head = (None, 1, H, W)
    if entry in ("dagl_ce_forward", "dagl_ce_forward_debug", "dagl_ce_forward_profiled"):
        extra = {"dagl_ce_forward": (), "dagl_ce_forward_debug": (None, None, None), "dagl_ce_forward_profiled": (None,)}[entry]
        return getattr(lib, entry)(*head, p("b1"), p("b2"), p("thr"), p("bias"), p("fc1_w"), p("fc1_b"), p("fc2_w"), p("fc2_b"),
                                   mode, k, p("out"), ws, ws_bytes, C.byref(info), *extra)
    weights = [p(n) for n in ("g_w", "g_b", "theta_w", "theta_b", "thr_w", "thr_b", "bias_w", "bias_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]
    if entry == "dagl_ce_forward_fused":
        return lib.dagl_ce_forward_fused(*head, p("x"), *weights, mode, k, p("out"), ws, ws_bytes, C.byref(info), None)
    if entry == "dagl_ces_stage_forward":
        heads = (_lib.CeWeights * 4)(*[_lib.CeWeights(*weights) for _ in range(4)])
        return lib.dagl_ces_stage_forward(*head, p("x"), heads, p("mix_w"), p("mix_b"), mode, k, p("out"), ws, ws_bytes, C.byref(info), None)
    if entry == "dagl_ce_core_forward":
        return lib.dagl_ce_core_forward(*head, p("wq_rows"), p("x_rows"), p("b2"), p("thr"), p("bias"), mode, k, p("out"), p("nb_idx"),
                                        p("nb_wgt"), p("nb_s"), p("nb_cnt"), p("mu"), ws, ws_bytes, C.byref(info))
    return lib.dagl_ce_core_dense_forward(*head, 0, p("wq_rows"), p("x_rows"), p("b2"), p("thr"), p("bias"), p("out"), p("lse"),
                                          p("mu"), ws, ws_bytes, C.byref(info))


def forward_rejections(lib, entry):
    """Every rejection a forward entry point makes before it touches the device -- null pointers, a misaligned workspace, a
    workspace one byte short -- over screened / unscreened maps and the adaptive / top-k modes:
    [(case, rc, dagl_last_error, info fields)]."""
    from dagl_amd import _lib
    rows = []
    for H, W in ((64, 64), (45, 45)):
        for mode, k in ((0, 0), (1, 8)):
            cases = [("null out", _WS, 1 << 40, ("out",)), ("null input", _WS, 1 << 40, (_FIRST_INPUT[entry],)),
                     ("misaligned workspace", _WS + 8, 1 << 40, ()), ("no workspace", _WS, 0, ())]
            if mode == 0:
                cases.append(("null threshold input", _WS, 1 << 40, (_THRESHOLD_INPUT.get(entry, "thr"),)))
            for case, ws, ws_bytes, null in cases:
                info = _lib.CeInfo(*([77] * 7))
                rc = _forward_call(lib, entry, H, W, mode, k, ws, ws_bytes, info, null)
                rows.append(((case, H, W, mode), rc, lib.dagl_last_error(), tuple(getattr(info, n) for n, _ in _lib.CeInfo._fields_)))
                if case == "no workspace":        # the size it reported, one byte short
                    short = rows[-1][3][0] - 1
                    info = _lib.CeInfo(*([77] * 7))
                    rc = _forward_call(lib, entry, H, W, mode, k, _WS, short, info)
                    rows.append((("one byte short", H, W, mode), rc, lib.dagl_last_error(),
                                 tuple(getattr(info, n) for n, _ in _lib.CeInfo._fields_)))
    return rows


@pytest.mark.parametrize("entry", _FORWARD_ENTRIES)
def test_host_side_forward_rejections(lib_path, entry):
    """The forward entry points check their pointers and workspace before anything reaches the device: error codes, messages and
    the workspace size they report."""
    from dagl_amd import _lib
    rows = forward_rejections(_lib.load(), entry)
    for (case, H, W, mode), rc, err, info in rows:
        what = (entry, case, H, W, mode, err)
        if case in ("no workspace", "one byte short"):
            assert rc == _lib.ERR_WORKSPACE, what
            assert b"workspace" in err and info[0] > 0, what
        else:
            assert rc == -1, what
            assert (b"aligned" in err) if case == "misaligned workspace" else (b"null" in err or b"bad argument" in err
                                                                               or b"required" in err), what
    short = [r for r in rows if r[0][0] == "one byte short"]
    full = [r for r in rows if r[0][0] == "no workspace"]
    assert [r[3][0] for r in short] == [r[3][0] for r in full]       # one byte short of the size it asked for: the same answer


def test_wide_debug_rejections(lib_path):
    """dagl_ce_wide_debug refuses, before anything reaches the device, the calls that run no list kernel -- the adaptive mode, k up to
    the list width, min(k, N) > 1024 -- and checks its pointer and workspace like the forward entry points."""
    from dagl_amd import _lib
    lib = _lib.load()
    call = lambda mode, k, ws=_WS, ws_bytes=1 << 40, out=_FAKE, H=64, W=64: lib.dagl_ce_wide_debug(None, 1, H, W, mode, k, ws, ws_bytes, out)
    for mode, k in ((0, 0), (1, 8), (1, 64), (2, 64), (1, 1025), (2, 4096), (1, 1 << 20)):
        assert call(mode, k) == _lib.ERR_UNSUPPORTED, (mode, k)
        assert b"dagl_ce_wide_debug" in lib.dagl_last_error()
    assert call(1, 5000, H=40, W=44) == _lib.ERR_UNSUPPORTED            # min(k, N) = 1760 > 1024
    assert call(1, 100, out=None) == -1 and b"null" in lib.dagl_last_error()
    assert call(1, 100, ws=_WS + 8) == -1 and b"aligned" in lib.dagl_last_error()
    for mode, k in ((1, 100), (2, 1024)):
        need = lib.dagl_ce_workspace_bytes(1, 64, 64, mode, k)
        assert need > 0 and call(mode, k, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
        assert call(mode, k, ws_bytes=0) == _lib.ERR_WORKSPACE


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from dagl_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.DaglError, match="no fallback"):
        _lib.load()


def test_info_struct_layout_matches_header():
    """ctypes mirror of dagl_ce_info: same field order and size as the C struct (3 x int64 + 2 x int32)."""
    import ctypes as C
    from dagl_amd import _lib
    text = open(os.path.join(REPO, "include", "dagl_ce.h")).read()
    body = text[text.index("typedef struct dagl_ce_info {"):text.index("} dagl_ce_info;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in _lib.CeInfo._fields_]
    assert [t for t, _ in fields] == ["int64_t" if f is C.c_int64 else "int32_t" for _, f in _lib.CeInfo._fields_]
    assert C.sizeof(_lib.CeInfo) == 40
