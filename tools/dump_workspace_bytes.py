#!/usr/bin/env python
"""dump_workspace_bytes.py [LIB.so] [OUT.json]: what every workspace / scratch size entry point of the library answers over a
fixed table of shapes and arguments, as JSON rows {"entry", "args", "bytes"}.  ctypes only: the size entry points are host
arithmetic and need no device.  tests/golden/workspace_bytes.json is this script's output;
tests/test_workspace_bytes_host.py compares the built library against it row by row."""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 8, 8), (1, 20, 36), (2, 44, 48), (1, 64, 64), (3, 72, 72), (1, 128, 128), (1, 256, 256), (8, 128, 128), (1, 100, 300))
MODE_K = ((0, 0), (1, 8), (1, 50), (1, 100), (2, 16), (0x100, 0), (0x101, 16))       # k = 100 > DAGL_MAX_TOPK: the wide top-k layout
LIST_MODE_K = ((0, 0), (1, 8), (2, 64))
EDGES = (0, 1, 100000)
GENERIC = (5, 2, 1, 16)                                                              # ksize, stride_1, stride_2, inter_channels
GENERIC_CIN = 64


def table():
    """[(entry, args)]: args as the C prototype of include/dagl_ce.h takes them."""
    rows = []
    for B, H, W in SHAPES:
        rows += [("dagl_ce_workspace_bytes", (B, H, W, m, k)) for m, k in MODE_K]
        rows += [("dagl_ces_stage_workspace_bytes", (B, H, W, m, k)) for m, k in MODE_K]
        rows += [("dagl_ce_core_backward_workspace_bytes", (B, H, W, m, k)) for m, k in LIST_MODE_K]
        rows += [("dagl_ce_graph_workspace_bytes", (B, H, W, m, k, 0)) for m, k in LIST_MODE_K]
        rows += [("dagl_ce_core_dense_workspace_bytes", (B, H, W, bw)) for bw in (0, 1)]
        rows += [("dagl_ce_prologue16_scratch_bytes", (B, H, W))]
        rows += [("dagl_project_patches16_scratch_bytes", (B, H, W, q)) for q in (0, 1)]
        rows += [("dagl_graph_apply_workspace_bytes", (B, H, W, e)) for e in EDGES]
        rows += [("dagl_graph_apply_backward_workspace_bytes", (B, H, W, e)) for e in EDGES]
        rows += [("dagl_ce_generic_workspace_bytes", (B, GENERIC_CIN, H, W) + GENERIC)]
        rows += [("dagl_ce_generic_core_workspace_bytes", (B, H, W) + GENERIC + (bw,)) for bw in (0, 1)]
        rows += [("dagl_fc_grad16_scratch_bytes", (B, H, W))]
        rows += [("dagl_fc_grad16_dmap_scratch_bytes", (B, H, W))]
    return rows


def dump(lib_path):
    lib = C.CDLL(lib_path)
    out = []
    for entry, args in table():
        fn = getattr(lib, entry)
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_int] * len(args)
        if entry.startswith("dagl_graph_apply"):
            fn.argtypes = [C.c_int] * 3 + [C.c_int64]
        out.append({"entry": entry, "args": list(args), "bytes": int(fn(*args))})
    return out


if __name__ == "__main__":
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "dagl_amd", "csrc", "libdagl_ce.so")
    text = "[\n" + ",\n".join(json.dumps(r) for r in dump(lib_path)) + "\n]\n"
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
