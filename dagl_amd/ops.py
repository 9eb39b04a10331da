"""Stage-level host wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Every function takes contiguous fp32 CUDA(HIP) tensors, enqueues on torch's current stream and returns
freshly allocated outputs.  They mirror the stages of the reference method one to one
(DN_Gray/model/dagl.py:216-274); see include/dagl_ce.h for the exact contracts.

This module is the only caller of the library inside the package: ce.py, graph.py, trunk.py and train_ops.py keep modules,
autograd and layouts and hand every operand to a wrapper here, which checks it (``_need``) before its pointer is taken.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import D, DS, MODES, P, DaglError, check


# A/B switch (tests, bench.py --dense-backward fp32): the dense graph core's backward with its five matrix products on the fp32
# matrix cores.  An explicit attribute, not an environment variable: nothing outside the process can change gradient bits.
DENSE_BACKWARD_FP32 = False


def _stream() -> int:
    """torch's current stream ON THE CURRENT DEVICE -- every entry point below runs under ``_on_device`` which makes the
    tensors' device current first (the C ABI launches on the current HIP device)."""
    return torch.cuda.current_stream().cuda_stream


_SCALARS = frozenset((int, float, bool, str, type(None)))       # most arguments of a call: passed over before any isinstance


def _common_device(values, dev, who: str):
    """``dev`` or, when it is None, the device of the first GPU tensor among ``values`` (lists, tuples and dicts are looked
    into); a GPU tensor on another device is refused."""
    for a in values:
        if type(a) in _SCALARS:
            continue
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise DaglError(f"{who}: tensors on different devices ({dev} and {a.device})")
        elif isinstance(a, dict):
            dev = _common_device(a.values(), dev, who)
        elif isinstance(a, (list, tuple)):
            dev = _common_device(a, dev, who)
    return dev


def _on_device(fn):
    """Run ``fn`` with the device of its tensor arguments as the current device (a module living on cuda:1 must not
    launch on cuda:0's stream) and refuse tensors spread over several devices.  Every library call passes through here, a
    few hundred per training step: a plain loop over the arguments, and the device is switched only when it is not current."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = _common_device(args, None, fn.__name__)
        if kwargs:
            dev = _common_device(kwargs.values(), dev, fn.__name__)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)          # (no GPU tensor: the per-argument checks below report the CPU tensor)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def _need(t: torch.Tensor, name: str, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise DaglError(f"{name}: must live on the GPU (dagl_amd has no CPU path)")
    if t.dtype != dtype:
        raise DaglError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise DaglError(f"{name}: must be contiguous")
    return t


def _check_mode(mode: str):
    if mode not in MODES:
        raise DaglError(f"unknown mode {mode!r}")


def _ptr(t, used: bool = True):
    """Device pointer of an operand the call may go without: NULL when ``t`` is None or not ``used``."""
    return t.data_ptr() if used and t is not None else None


def _topk_flags(mode: str, exact_scan: bool, tight_topk: bool, sampled_topk: bool) -> int:
    """DAGL_FLAG_TIGHT_TOPK / DAGL_FLAG_SAMPLED_TOPK: only the top-k modes behind the screen have a candidate threshold."""
    if mode == "adaptive" or exact_scan:
        return 0
    return _lib.FLAG_TIGHT_TOPK if tight_topk else (_lib.FLAG_SAMPLED_TOPK if sampled_topk else 0)


def _info_dict(info, drop=(), **fixed) -> dict:
    """A call's ``CeInfo`` as a dict without the keys in ``drop``; ``fixed`` gives the values an entry point reports itself."""
    d = dict(required_bytes=info.required_bytes, total_edges=info.total_edges, max_degree=info.max_degree, path=info.path,
             redone_queries=info.redone_queries, range_fallback=info.range_fallback, dense_rerun_blocks=info.dense_rerun_blocks)
    for n in drop:
        del d[n]
    if fixed:
        d.update(fixed)
    return d


def query_grid(H: int, W: int):
    return -(-H // 4), -(-W // 4)


@_on_device
def pad_nhwc(x: torch.Tensor) -> torch.Tensor:
    """[B,16,H,W] -> zero-bordered channels-last [B,H+6,W+6,16]."""
    _need(x, "x")
    B, c, H, W = x.shape
    if c != 16:
        raise DaglError("pad_nhwc: 16 channels expected")
    out = torch.empty(B, H + 6, W + 6, 16, device=x.device, dtype=torch.float32)
    check(_lib.load().dagl_pad_nhwc(_stream(), B, H, W, x.data_ptr(), out.data_ptr()), "dagl_pad_nhwc")
    return out


@_on_device
def pack_fc_weight(w: torch.Tensor) -> torch.Tensor:
    _need(w, "w")
    if tuple(w.shape) != (196, 784):
        raise DaglError("pack_fc_weight: [196,784] expected")
    out = torch.empty(208 * 784, device=w.device, dtype=torch.float32)
    check(_lib.load().dagl_pack_fc_weight(_stream(), w.data_ptr(), out.data_ptr()), "dagl_pack_fc_weight")
    return out


@_on_device
def project_patches(map_nhwc: torch.Tensor, w_packed: torch.Tensor, fc_bias: torch.Tensor, H: int, W: int,
                    queries: bool, want_colsum: bool = False):
    """relu(Linear(patch)) for every patch -> ([B, rows_alloc, 204] features, optional [B,204] fp64 column sums)."""
    _need(map_nhwc, "map_nhwc"); _need(w_packed, "w_packed"); _need(fc_bias, "fc_bias")
    lib = _lib.load()
    B = map_nhwc.shape[0]
    Lh, Lw = query_grid(H, W)
    rows = Lh * Lw if queries else H * W
    ra = lib.dagl_feat_rows(rows)
    feat = torch.empty(B, ra, DS, device=map_nhwc.device, dtype=torch.float32)
    colsum = torch.empty(B, DS, device=map_nhwc.device, dtype=torch.float64) if (want_colsum and not queries) else None
    check(lib.dagl_project_patches(_stream(), B, H, W, int(queries), map_nhwc.data_ptr(), w_packed.data_ptr(),
                                   fc_bias.data_ptr(), feat.data_ptr(), _ptr(colsum)), "dagl_project_patches")
    return feat, colsum


@_on_device
def query_thresholds(wq: torch.Tensor, colsum: torch.Tensor, thr: torch.Tensor, L: int, N: int) -> torch.Tensor:
    _need(wq, "wq"); _need(colsum, "colsum", torch.float64); _need(thr, "thr")
    B = wq.shape[0]
    mt = torch.empty(B, L, device=wq.device, dtype=torch.float32)
    check(_lib.load().dagl_query_thresholds(_stream(), B, L, N, wq.data_ptr(), colsum.data_ptr(), thr.data_ptr(),
                                            mt.data_ptr()), "dagl_query_thresholds")
    return mt


@_on_device
def scores_dense(wq: torch.Tensor, x: torch.Tensor, L: int, N: int) -> torch.Tensor:
    _need(wq, "wq"); _need(x, "x")
    B = wq.shape[0]
    s = torch.empty(B, L, N, device=wq.device, dtype=torch.float32)
    check(_lib.load().dagl_scores_dense(_stream(), B, L, N, wq.data_ptr(), x.data_ptr(), s.data_ptr()),
          "dagl_scores_dense")
    return s


@_on_device
def gather_aggregate(idx: torch.Tensor, wgt: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """out[l,:] = sum_k wgt[l,k] * values[idx[l,k],:]   (idx < 0 = empty slot)."""
    _need(idx, "idx", torch.int32); _need(wgt, "wgt"); _need(values, "values")
    L, k = idx.shape
    if wgt.shape != idx.shape or values.dim() != 2:
        raise DaglError("gather_aggregate: shape mismatch")
    Pn = values.shape[1]
    out = torch.empty(L, Pn, device=values.device, dtype=torch.float32)
    check(_lib.load().dagl_gather_aggregate(_stream(), L, k, Pn, idx.data_ptr(), wgt.data_ptr(), values.data_ptr(),
                                            out.data_ptr()), "dagl_gather_aggregate")
    return out


@_on_device
def unfold_values(b2_nhwc: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _need(b2_nhwc, "b2_nhwc")
    B = b2_nhwc.shape[0]
    rows = torch.empty(B, H * W, P, device=b2_nhwc.device, dtype=torch.float32)
    check(_lib.load().dagl_unfold_values(_stream(), B, H, W, b2_nhwc.data_ptr(), rows.data_ptr()),
          "dagl_unfold_values")
    return rows


@_on_device
def fold_normalize(agg: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _need(agg, "agg")
    B = agg.shape[0]
    out = torch.empty(B, 16, H, W, device=agg.device, dtype=torch.float32)
    check(_lib.load().dagl_fold_normalize(_stream(), B, H, W, agg.data_ptr(), out.data_ptr()), "dagl_fold_normalize")
    return out


class StageProfile:
    """hipEvents at the stage boundaries of up to ``max_calls`` block forwards (include/dagl_ce.h, dagl_profile_*)."""

    def __init__(self, max_calls: int):
        self._h = C.c_void_p()
        check(_lib.load().dagl_profile_create(int(max_calls), C.byref(self._h)), "dagl_profile_create")
        self.max_calls = int(max_calls)

    def reset(self):
        check(_lib.load().dagl_profile_reset(self._h), "dagl_profile_reset")

    def select_stage(self, stage: "int | str"):
        """Record only the two events around one stage (index or name; -1 = every boundary again)."""
        if isinstance(stage, str):
            stage = list(_lib.STAGE_NAMES).index(stage)
        check(_lib.load().dagl_profile_select_stage(self._h, int(stage)), "dagl_profile_select_stage")

    def read(self):
        """-> list of per-call lists of N_STAGES milliseconds (waits for the recorded events)."""
        lib = _lib.load()
        n = C.c_int(0)
        buf = (C.c_float * (self.max_calls * _lib.N_STAGES))()
        check(lib.dagl_profile_read(self._h, C.byref(n), buf, self.max_calls), "dagl_profile_read")
        return [[buf[c * _lib.N_STAGES + s] for s in range(_lib.N_STAGES)] for c in range(n.value)]

    def __del__(self):
        try:
            if self._h:
                _lib.load().dagl_profile_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


class Workspace:
    """Grow-only device scratch buffers reused across calls, one per device (allocated through torch's caching allocator,
    so they are stream-ordered and visible to torch's memory accounting).  ``nn.DataParallel`` replicas share the
    object across per-device threads: the buffer is built in a local and looked up by device, never handed across."""

    def __init__(self):
        self._bufs = {}

    @property
    def buf(self):
        """The buffer of the current device (None before the first call there)."""
        if not self._bufs:
            return None
        if torch.cuda.is_available():
            b = self._bufs.get(torch.device("cuda", torch.cuda.current_device()))
            if b is not None:
                return b
        return next(iter(self._bufs.values())) if len(self._bufs) == 1 else None

    def peek(self, device):
        return self._bufs.get(torch.device(device))

    def get(self, nbytes: int, device) -> torch.Tensor:
        device = torch.device(device)
        if device.index is None and device.type == "cuda":
            device = torch.device("cuda", torch.cuda.current_device())
        b = self._bufs.get(device)
        if b is None or b.numel() < nbytes + 256:
            self._bufs.pop(device, None)
            b = None                                              # release before the larger allocation
            b = torch.empty(int(nbytes * 1.05) + 4096, device=device, dtype=torch.uint8)
            self._bufs[device] = b
        return b


def _aligned(buf: torch.Tensor):
    base = buf.data_ptr()
    a = (base + 255) // 256 * 256
    return a, buf.numel() - (a - base)


def _scratch(nbytes: int, device):
    """(buffer, 256-byte aligned pointer) of ``nbytes`` of throwaway device scratch; as with ``_region`` the caller keeps the
    buffer referenced until its launch is queued."""
    buf = torch.empty(nbytes + 256, device=device, dtype=torch.uint8)
    return buf, _aligned(buf)[0]


def _region(workspace: "Workspace | None", nbytes: int, device):
    """(buffer, 256-byte aligned pointer, bytes from there) of at least ``nbytes`` in ``workspace`` (a throwaway one when None).
    The caller keeps the buffer referenced until its launch is queued."""
    buf = (workspace if workspace is not None else Workspace()).get(nbytes, device)
    return (buf,) + _aligned(buf)


def _sized_region(workspace: "Workspace | None", device, entry: str, *args):
    """``_region`` of the bytes the library's ``entry`` (a ``*_workspace_bytes`` symbol) asks for ``args``.  0 bytes is its refusal of
    the shape: raised with the library's message."""
    need = getattr(_lib.load(), entry)(*args)
    if need == 0:
        check(-1, entry)
    return _region(workspace, need, device)


@_on_device
def ce_forward(b1, b2, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b, mode: str = "adaptive", k: int = 0,
               workspace: "Workspace | None" = None, return_info: bool = False, debug: bool = False,
               profile: "StageProfile | None" = None, exact_scan: bool = False, tight_topk: bool = False,
               sampled_topk: bool = False):
    """Everything of CE.forward after its prologue convolutions (dagl.py:216-274) -> [B,16,H,W].  ``tight_topk`` /
    ``sampled_topk``: DAGL_FLAG_TIGHT_TOPK / DAGL_FLAG_SAMPLED_TOPK (top-k modes behind the screen), as in ``ce_forward_fused``."""
    lib = _lib.load()
    _check_mode(mode)
    for n, t in (("b1", b1), ("b2", b2), ("fc1_w", fc1_w), ("fc1_b", fc1_b), ("fc2_w", fc2_w), ("fc2_b", fc2_b)):
        _need(t, n)
    B, c, H, W = b1.shape
    if c != 16 or b2.shape != b1.shape:
        raise DaglError("ce_forward: b1/b2 must both be [B,16,H,W]")
    if tuple(fc1_w.shape) != (196, 784) or tuple(fc2_w.shape) != (196, 784):
        raise DaglError("ce_forward: fc weights must be [196,784]")
    Lh, Lw = query_grid(H, W)
    if mode != "topk":
        _need(thr, "thr"); _need(bias, "bias")
        if thr.numel() != B * Lh * Lw or bias.numel() != B * Lh * Lw:
            raise DaglError("ce_forward: thr/bias must hold B*L values")
    mode_flags = MODES[mode] | (_lib.FLAG_EXACT_SCAN if exact_scan else 0)
    need = lib.dagl_ce_workspace_bytes(B, H, W, mode_flags, int(k))
    if need == 0:
        check(-1, "dagl_ce_workspace_bytes")
    mode_flags |= _topk_flags(mode, exact_scan, tight_topk, sampled_topk)
    out = torch.empty(B, 16, H, W, device=b1.device, dtype=torch.float32)
    info = _lib.CeInfo()
    rc = 0
    dbg = None
    if debug:
        L = Lh * Lw
        dbg = dict(deg=torch.empty(B, L, device=b1.device, dtype=torch.int32),
                   rowsum=torch.empty(B, L, device=b1.device, dtype=torch.float32),
                   agg=torch.empty(B, L, P, device=b1.device, dtype=torch.float32))
    for _attempt in range(2):
        buf, a, nbytes = _region(workspace, need, b1.device)
        args = (_stream(), B, H, W, b1.data_ptr(), b2.data_ptr(), _ptr(thr), _ptr(bias),
                fc1_w.data_ptr(), fc1_b.data_ptr(), fc2_w.data_ptr(), fc2_b.data_ptr(),
                mode_flags, int(k), out.data_ptr(), a, nbytes, C.byref(info))
        if profile is not None:
            rc = lib.dagl_ce_forward_profiled(*args, profile._h)
        elif dbg is None:
            rc = lib.dagl_ce_forward(*args)
        else:
            rc = lib.dagl_ce_forward_debug(*args, dbg["deg"].data_ptr(), dbg["rowsum"].data_ptr(),
                                           dbg["agg"].data_ptr())
        if rc == _lib.ERR_WORKSPACE and info.required_bytes > need:
            need = int(info.required_bytes)      # dense neighbourhoods: the CSR fallback asked for more
            continue
        break
    check(rc, "dagl_ce_forward")
    meta = _info_dict(info)
    if dbg is not None:
        meta.update(dbg)
    if return_info or debug:
        return out, meta
    return out


@_on_device
def ce_graph(b1, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b, mode: str = "adaptive", k: int = 0, scores: bool = False,
             max_edges: "int | None" = None, rows_per_chunk: int = 0, workspace: "Workspace | None" = None,
             degrees_only: bool = False):
    """The patch graph of dagl.py:250-261 as CSR (``dagl_ce_graph_count`` / ``_fill``, include/dagl_ce.h): inputs as ``ce_forward``'s
    without the value map -> dict(row_off [B*L+1] int64, key [E] int32, weight [E] fp32, score [E] fp32 | None).  The edge count is read
    on the host between the two phases (one synchronisation; not under stream capture); ``max_edges``: raise instead of allocating
    more; ``degrees_only``: the count phase alone -> row_off."""
    lib = _lib.load()
    _check_mode(mode)
    for n, t in (("b1", b1), ("fc1_w", fc1_w), ("fc1_b", fc1_b), ("fc2_w", fc2_w), ("fc2_b", fc2_b)):
        _need(t, n)
    if b1.dim() != 4 or b1.shape[1] != 16:
        raise DaglError("ce_graph: b1 must be [B,16,H,W]")
    B, _, H, W = b1.shape
    if tuple(fc1_w.shape) != (196, 784) or tuple(fc2_w.shape) != (196, 784):
        raise DaglError("ce_graph: fc weights must be [196,784]")
    Lh, Lw = query_grid(H, W)
    BL = B * Lh * Lw
    heads = mode != "topk"
    if heads:
        _need(thr, "thr"); _need(bias, "bias")
        if thr.numel() != BL or bias.numel() != BL:
            raise DaglError("ce_graph: thr/bias must hold B*L values")
    if torch.cuda.is_current_stream_capturing():
        raise DaglError("ce_graph: not available under stream capture (the edge count is read on the host between the two phases)")
    buf, a, nbytes = _sized_region(workspace, b1.device, "dagl_ce_graph_workspace_bytes", B, H, W, MODES[mode], int(k), int(rows_per_chunk))
    row_off = torch.empty(BL + 1, device=b1.device, dtype=torch.int64)
    info = _lib.CeInfo()
    check(lib.dagl_ce_graph_count(_stream(), B, H, W, b1.data_ptr(), _ptr(thr, heads), _ptr(bias, heads), fc1_w.data_ptr(),
                                  fc1_b.data_ptr(), fc2_w.data_ptr(), fc2_b.data_ptr(), MODES[mode], int(k), int(rows_per_chunk),
                                  row_off.data_ptr(), a, nbytes, C.byref(info)), "dagl_ce_graph_count")
    if degrees_only:
        return dict(row_off=row_off)
    total = int(row_off[-1])                          # the one synchronisation
    if max_edges is not None and total > int(max_edges):
        raise DaglError(f"ce_graph: the graph holds {total} edges, max_edges={int(max_edges)}")
    key = torch.empty(total, device=b1.device, dtype=torch.int32)
    weight = torch.empty(total, device=b1.device, dtype=torch.float32)
    score = torch.empty(total, device=b1.device, dtype=torch.float32) if scores else None
    check(lib.dagl_ce_graph_fill(_stream(), B, H, W, MODES[mode], int(k), int(rows_per_chunk), row_off.data_ptr(),
                                 _ptr(key, total > 0), _ptr(weight, total > 0), _ptr(score, total > 0), total, total, a, nbytes),
          "dagl_ce_graph_fill")
    del buf
    return dict(row_off=row_off, key=key, weight=weight, score=score)


def graph_apply_segment() -> int:
    """Edges a block of the graph-apply kernels takes (``dagl_graph_apply_segment``)."""
    return int(_lib.load().dagl_graph_apply_segment())


def _value_map(who: str, b2p):
    """Shape of a graph call's value map -> (B, H, W)."""
    if b2p.dim() != 4 or b2p.shape[3] != 16 or b2p.shape[1] < 7 or b2p.shape[2] < 7:
        raise DaglError(f"{who}: b2p must be the zero-bordered NHWC value map [B,H+6,W+6,16], got {tuple(b2p.shape)}")
    return b2p.shape[0], b2p.shape[1] - 6, b2p.shape[2] - 6


def _transposed_csr(who: str, what: str, transposed, n_cols: int, E: int):
    """The transposed CSR a gradient ``what`` needs -> (col_off [n_cols + 1], src_row [E], perm [E])."""
    if transposed is None:
        raise DaglError(f"{who}: {what} needs the transposed CSR (col_off, src_row, perm)")
    col_off, src_row, perm = transposed
    _need(col_off, "col_off", torch.int64); _need(src_row, "src_row", torch.int32); _need(perm, "perm", torch.int32)
    if col_off.numel() != n_cols + 1 or src_row.numel() != E or perm.numel() != E:
        raise DaglError(f"{who}: the transposed CSR must hold B*N+1 = {n_cols + 1} offsets and {E} edges")
    return col_off, src_row, perm


def _graph_apply_operands(who: str, b2p, row_off, key, weight):
    """Shapes of a graph-apply call's operands -> (B, H, W, E).  Array CONTENTS stay unread: the kernels bound every index themselves."""
    _need(b2p, "b2p"); _need(row_off, "row_off", torch.int64); _need(key, "key", torch.int32); _need(weight, "weight")
    B, H, W = _value_map(who, b2p)
    Lh, Lw = query_grid(H, W)
    E = key.numel()
    if row_off.dim() != 1 or row_off.numel() != B * Lh * Lw + 1:
        raise DaglError(f"{who}: row_off holds {row_off.numel()} offsets, expected B*L+1 = {B * Lh * Lw + 1}")
    if key.dim() != 1 or weight.dim() != 1 or weight.numel() != E:
        raise DaglError(f"{who}: key and weight must be 1-d with one entry per edge")
    return B, H, W, E


@_on_device
def graph_apply(b2p, row_off, key, weight, workspace: "Workspace | None" = None) -> torch.Tensor:
    """A block's output from a given patch graph (``dagl_graph_apply``, csrc/graph_apply.hip): ``fold(A_G . V(b2)) / cnt`` with b2p the
    zero-bordered NHWC value map [B,H+6,W+6,16] and (row_off [B*L+1] int64, key [E] int32, weight [E] fp32) the CSR of ``A_G`` ->
    [B,16,H,W].  Nothing is read on the host; keys outside [0, N) contribute nothing."""
    lib = _lib.load()
    B, H, W, E = _graph_apply_operands("graph_apply", b2p, row_off, key, weight)
    buf, a, nbytes = _sized_region(workspace, b2p.device, "dagl_graph_apply_workspace_bytes", B, H, W, E)
    out = torch.empty(B, 16, H, W, device=b2p.device, dtype=torch.float32)
    check(lib.dagl_graph_apply(_stream(), B, H, W, b2p.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), _ptr(weight, E > 0), E,
                               out.data_ptr(), a, nbytes), "dagl_graph_apply")
    del buf
    return out


@_on_device
def graph_apply_backward(d_out, b2p, row_off, key, weight, transposed=None, need_b2p: bool = True, need_weight: bool = True,
                         workspace: "Workspace | None" = None):
    """Gradients of ``graph_apply`` (``dagl_graph_apply_backward``) -> (d_b2p [B,H+6,W+6,16] | None, d_weight [E] | None).
    ``transposed`` = (col_off [B*N+1] int64, src_row [E] int32, perm [E] int32), the graph's transposed CSR
    (``PatchGraph.transpose``): required with ``need_b2p``."""
    lib = _lib.load()
    B, H, W, E = _graph_apply_operands("graph_apply_backward", b2p, row_off, key, weight)
    _need(d_out, "d_out")
    if tuple(d_out.shape) != (B, 16, H, W):
        raise DaglError(f"graph_apply_backward: d_out is {tuple(d_out.shape)}, expected {(B, 16, H, W)}")
    col_off = src_row = perm = None
    if need_b2p:
        col_off, src_row, perm = _transposed_csr("graph_apply_backward", "d_b2p", transposed, B * H * W, E)
    buf, a, nbytes = _sized_region(workspace, b2p.device, "dagl_graph_apply_backward_workspace_bytes", B, H, W, E)
    d_b2p = torch.empty_like(b2p) if need_b2p else None
    d_weight = torch.empty_like(weight) if need_weight else None
    check(lib.dagl_graph_apply_backward(_stream(), B, H, W, b2p.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), _ptr(weight, E > 0), E,
                                        d_out.data_ptr(), _ptr(col_off), _ptr(src_row, E > 0), _ptr(perm, E > 0), _ptr(d_b2p),
                                        _ptr(d_weight, E > 0), a, nbytes), "dagl_graph_apply_backward")
    del buf
    return d_b2p, d_weight


_GRAPH_NORMALIZE = {"reference": 0, "edges": _lib.GRAPH_ATTEND_EDGES_ONLY}


def _maps_of(L: int, N: int):
    """The maps (H, W) with H*W = N keys and a stride-4 query grid of L rows, by ascending H."""
    return ((h, N // h) for h in range(1, N + 1) if N % h == 0 and math.prod(query_grid(h, N // h)) == L)


def _map_of(L: int, N: int):
    """The first of ``_maps_of``: the graph-attend kernels use L and N alone, so any such map describes the call (``hw`` names the real
    one)."""
    hw = next(_maps_of(L, N), None)
    if hw is None:
        raise DaglError(f"graph_attend: no map of {N} keys has a stride-4 query grid of {L} rows")
    return hw


def _graph_attend_operands(who: str, wq_rows, x_rows, row_off, key, tau, normalize, hw):
    """Shapes of a graph-attend call's operands -> (B, H, W, E, flags): ``_graph_apply_operands``' checks with the feature rows in the place
    of the value map.  Array CONTENTS stay unread: the kernels bound every index themselves."""
    _need(wq_rows, "wq_rows"); _need(x_rows, "x_rows"); _need(row_off, "row_off", torch.int64); _need(key, "key", torch.int32)
    if wq_rows.dim() != 3 or x_rows.dim() != 3 or wq_rows.shape[2] != D or x_rows.shape[2] != D or wq_rows.shape[0] != x_rows.shape[0]:
        raise DaglError(f"{who}: expected wq_rows [B,L,{D}] and x_rows [B,N,{D}], got {tuple(wq_rows.shape)} and {tuple(x_rows.shape)}")
    B, L, N = wq_rows.shape[0], wq_rows.shape[1], x_rows.shape[1]
    H, W = (int(v) for v in hw) if hw is not None else _map_of(L, N)
    Lh, Lw = query_grid(H, W)
    if H * W != N or Lh * Lw != L:
        raise DaglError(f"{who}: a {H}x{W} map has {Lh * Lw} queries and {H * W} keys, the feature rows hold {L} and {N}")
    if row_off.dim() != 1 or row_off.numel() != B * L + 1:
        raise DaglError(f"{who}: row_off holds {row_off.numel()} offsets, expected B*L+1 = {B * L + 1}")
    if key.dim() != 1:
        raise DaglError(f"{who}: key must be 1-d with one entry per edge")
    if tau is not None:
        _need(tau, "tau")
        if tau.numel() != B * L:
            raise DaglError(f"{who}: tau holds {tau.numel()} values, expected B*L = {B * L}")
    if normalize not in _GRAPH_NORMALIZE:
        raise DaglError(f"{who}: normalize={normalize!r}, expected 'reference' or 'edges'")
    return B, H, W, key.numel(), _GRAPH_NORMALIZE[normalize]


@_on_device
def graph_attend(wq_rows, x_rows, row_off, key, tau=None, scale: float = 10.0, normalize: str = "reference",
                 workspace: "Workspace | None" = None, hw=None):
    """The block's edge weights on a given graph structure (``dagl_graph_attend``, csrc/graph_attend.hip) -> (weight [E], score [E]):
    wq_rows [B,L,196] / x_rows [B,N,196] the fc1 / fc2 features, (row_off [B*L+1] int64, key [E] int32) the CSR structure.
    ``score`` = S_e = <wq_rows[r], x_rows[b, key_e]>; with ``tau`` [B*L] the adaptive rule m = relu(S - tau_r), z = scale S m, edges with
    m = 0 weigh 0; without it z = scale S.  ``normalize="reference"``: the softmax of the reference over all N keys, every key off the
    graph counting as e^0 (rows with fewer than N edges); ``"edges"``: a plain softmax over the row's edges.  A row's degree counts
    EDGES: a repeated key is an entry of its own, not merged with its twin.  Keys outside [0, N) score 0 and weigh 0.  Nothing is read
    on the host; the same arrays give the same bits on every call.  ``hw``: the map (H, W) when the caller knows it."""
    lib = _lib.load()
    B, H, W, E, flags = _graph_attend_operands("graph_attend", wq_rows, x_rows, row_off, key, tau, normalize, hw)
    buf, a, nbytes = _sized_region(workspace, wq_rows.device, "dagl_graph_attend_workspace_bytes", B, H, W, E)
    score = torch.empty(E, device=wq_rows.device, dtype=torch.float32)
    weight = torch.empty_like(score)
    check(lib.dagl_graph_attend(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), E,
                                _ptr(tau), float(scale), flags, _ptr(score, E > 0), _ptr(weight, E > 0), a, nbytes), "dagl_graph_attend")
    del buf
    return weight, score


@_on_device
def graph_forward(wq_rows, x_rows, b2p, row_off, key, tau=None, scale: float = 10.0, normalize: str = "reference",
                  workspace: "Workspace | None" = None) -> torch.Tensor:
    """``graph_apply(b2p, row_off, key, graph_attend(...)[0])`` in one crossing of the edges (``dagl_graph_forward``,
    csrc/graph_forward.hip) -> [B,16,H,W]: the operands and the semantics of the two calls, ``score`` and ``weight`` never stored.  The
    result differs from the two-call one by fp32 roundings (weights are applied as e^(z - max) and scaled per row afterwards); the same
    arrays give the same bits on every call.  Nothing is read on the host."""
    lib = _lib.load()
    B, H, W, E, flags = _graph_forward_operands("graph_forward", wq_rows, x_rows, b2p, row_off, key, tau, normalize)
    buf, a, nbytes = _sized_region(workspace, wq_rows.device, "dagl_graph_forward_workspace_bytes", B, H, W, E)
    out = torch.empty(B, 16, H, W, device=wq_rows.device, dtype=torch.float32)
    check(lib.dagl_graph_forward(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), row_off.data_ptr(),
                                 _ptr(key, E > 0), E, _ptr(tau), float(scale), flags, out.data_ptr(), a, nbytes), "dagl_graph_forward")
    del buf
    return out


def _graph_forward_operands(who: str, wq_rows, x_rows, b2p, row_off, key, tau, normalize):
    """Shapes of a fused graph call's operands -> (B, H, W, E, flags): ``_graph_attend_operands`` on the map of ``b2p``."""
    _need(b2p, "b2p")
    hw = _value_map(who, b2p)[1:]
    B, H, W, E, flags = _graph_attend_operands(who, wq_rows, x_rows, row_off, key, tau, normalize, hw)
    if b2p.shape[0] != B:
        raise DaglError(f"{who}: b2p holds {b2p.shape[0]} images, the feature rows {B}")
    return B, H, W, E, flags


@_on_device
def graph_forward_train(wq_rows, x_rows, b2p, row_off, key, tau=None, scale: float = 10.0, normalize: str = "reference",
                        workspace: "Workspace | None" = None):
    """``graph_forward`` for training (``dagl_graph_forward_train``) -> (out [B,16,H,W], row_max [B*L] fp32, row_sum [B*L] fp64): ``out``
    carries ``graph_forward``'s bits, ``row_max`` / ``row_sum`` are the (M, D) each row was normalised with -- twelve bytes per row, all
    ``graph_forward_backward`` needs next to the operands.  An empty row's slots hold 0 and 1."""
    lib = _lib.load()
    B, H, W, E, flags = _graph_forward_operands("graph_forward_train", wq_rows, x_rows, b2p, row_off, key, tau, normalize)
    buf, a, nbytes = _sized_region(workspace, wq_rows.device, "dagl_graph_forward_workspace_bytes", B, H, W, E)
    out = torch.empty(B, 16, H, W, device=wq_rows.device, dtype=torch.float32)
    row_max = torch.empty(B * wq_rows.shape[1], device=wq_rows.device, dtype=torch.float32)
    row_sum = torch.empty(B * wq_rows.shape[1], device=wq_rows.device, dtype=torch.float64)
    check(lib.dagl_graph_forward_train(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), row_off.data_ptr(),
                                       _ptr(key, E > 0), E, _ptr(tau), float(scale), flags, out.data_ptr(), row_max.data_ptr(),
                                       row_sum.data_ptr(), a, nbytes), "dagl_graph_forward_train")
    del buf
    return out, row_max, row_sum


@_on_device
def graph_forward_backward(d_out, wq_rows, x_rows, b2p, row_off, key, row_max, row_sum, tau=None, scale: float = 10.0,
                           normalize: str = "reference", transposed=None, need_wq: bool = True, need_x: bool = True, need_tau: bool = True,
                           need_b2p: bool = True, workspace: "Workspace | None" = None):
    """Gradients of ``graph_forward_train`` (``dagl_graph_forward_backward``) -> (d_wq [B,L,196] | None, d_x [B,N,196] | None,
    d_tau [B*L] | None, d_b2p [B,H+6,W+6,16] | None) from ``d_out`` [B,16,H,W]; ``row_max`` / ``row_sum`` are the forward's.  One crossing
    of the edges recomputes scores and weights and forms ``<dAgg, V>`` per edge: what ``graph_apply_backward`` followed by
    ``graph_attend_backward`` computes from stored ``score`` / ``weight`` arrays.  ``transposed`` = (col_off, src_row, perm), the graph's
    transposed CSR (``PatchGraph.transpose``): required with ``need_x`` or ``need_b2p``.  ``d_tau`` is None without ``tau``.  Any subset
    of the outputs carries the bits of the full call."""
    lib = _lib.load()
    who = "graph_forward_backward"
    B, H, W, E, flags = _graph_forward_operands(who, wq_rows, x_rows, b2p, row_off, key, tau, normalize)
    n_rows = B * wq_rows.shape[1]
    _need(d_out, "d_out"); _need(row_max, "row_max"); _need(row_sum, "row_sum", torch.float64)
    if tuple(d_out.shape) != (B, 16, H, W):
        raise DaglError(f"{who}: d_out is {tuple(d_out.shape)}, expected {(B, 16, H, W)}")
    if row_max.numel() != n_rows or row_sum.numel() != n_rows:
        raise DaglError(f"{who}: row_max and row_sum must hold B*L = {n_rows} values")
    col_off = src_row = perm = None
    if need_x or need_b2p:
        col_off, src_row, perm = _transposed_csr(who, "d_x" if need_x else "d_b2p", transposed, B * H * W, E)
    buf, a, nbytes = _sized_region(workspace, wq_rows.device, "dagl_graph_forward_backward_workspace_bytes", B, H, W, E)
    d_wq = torch.empty_like(wq_rows) if need_wq else None
    d_x = torch.empty_like(x_rows) if need_x else None
    d_tau = torch.empty(n_rows, device=wq_rows.device, dtype=torch.float32) if need_tau and tau is not None else None
    d_b2p = torch.empty_like(b2p) if need_b2p else None
    check(lib.dagl_graph_forward_backward(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), row_off.data_ptr(),
                                          _ptr(key, E > 0), E, _ptr(tau), float(scale), flags, row_max.data_ptr(), row_sum.data_ptr(),
                                          d_out.data_ptr(), _ptr(col_off), _ptr(src_row, E > 0), _ptr(perm, E > 0), _ptr(d_wq), _ptr(d_x),
                                          _ptr(d_tau), _ptr(d_b2p), a, nbytes), "dagl_graph_forward_backward")
    del buf
    return d_wq, d_x, d_tau, d_b2p


@_on_device
def graph_from_lists(nb_idx, nb_wgt, nb_s, nb_cnt, hw, workspace: "Workspace | None" = None) -> dict:
    """The CSR patch graph of a list-form core forward's neighbour lists (``dagl_graph_from_lists``, csrc/graph_lists.hip): nb_idx /
    nb_wgt / nb_s [B,L,width] (``nb_s`` may be None) and nb_cnt [B,L] as ``ce_core_forward`` saves them, ``hw`` the map (H, W) ->
    dict(row_off [B*L+1] int64, key [E] int32, weight [E] fp32, score [E] fp32 | None), keys ascending inside a row.  Row r owns its
    first min(max(nb_cnt[r], 0), width) slots; a slot whose key is outside [0, H*W) is dropped; equal keys keep their slot order.  The
    arrays are allocated at capacity B*L*width and returned as views of their first E entries: E is read on the host (the one
    synchronisation; not under stream capture)."""
    lib = _lib.load()
    _need(nb_idx, "nb_idx", torch.int32); _need(nb_wgt, "nb_wgt"); _need(nb_cnt, "nb_cnt", torch.int32)
    if nb_s is not None:
        _need(nb_s, "nb_s")
    if nb_idx.dim() != 3 or nb_cnt.dim() != 2 or tuple(nb_cnt.shape) != tuple(nb_idx.shape[:2]):
        raise DaglError(f"graph_from_lists: expected nb_idx [B,L,width] and nb_cnt [B,L], got {tuple(nb_idx.shape)} and {tuple(nb_cnt.shape)}")
    for n, t in (("nb_wgt", nb_wgt), ("nb_s", nb_s)):
        if t is not None and t.shape != nb_idx.shape:
            raise DaglError(f"graph_from_lists: {n} is {tuple(t.shape)}, nb_idx {tuple(nb_idx.shape)}")
    B, L, width = nb_idx.shape
    H, W = (int(v) for v in hw)
    Lh, Lw = query_grid(H, W) if H >= 1 and W >= 1 else (0, 0)
    if B < 1 or Lh * Lw != L:
        raise DaglError(f"graph_from_lists: a {H}x{W} map has {Lh * Lw} queries, the lists hold {L} rows of {B} images")
    if torch.cuda.is_current_stream_capturing():
        raise DaglError("graph_from_lists: not available under stream capture (the edge count is read on the host)")
    buf, a, nbytes = _sized_region(workspace, nb_idx.device, "dagl_graph_from_lists_workspace_bytes", B, H, W)
    cap = B * L * width
    row_off = torch.empty(B * L + 1, device=nb_idx.device, dtype=torch.int64)
    key = torch.empty(cap, device=nb_idx.device, dtype=torch.int32)
    weight = torch.empty(cap, device=nb_idx.device, dtype=torch.float32)
    score = torch.empty(cap, device=nb_idx.device, dtype=torch.float32) if nb_s is not None else None
    check(lib.dagl_graph_from_lists(_stream(), B, H, W, width, nb_idx.data_ptr(), nb_wgt.data_ptr(), _ptr(nb_s), nb_cnt.data_ptr(),
                                    row_off.data_ptr(), key.data_ptr(), weight.data_ptr(), _ptr(score), cap, a, nbytes),
          "dagl_graph_from_lists")
    del buf
    total = int(row_off[-1])                          # the one synchronisation
    return dict(row_off=row_off, key=key[:total], weight=weight[:total], score=score[:total] if score is not None else None)


def graph_refresh_max_candidates() -> int:
    """Candidates (``max_row_edges * (2 radius + 1)^2``) a row of ``graph_refresh`` may expand into: a constant of the library."""
    return int(_lib.load().dagl_graph_refresh_max_candidates())


@_on_device
def graph_refresh(wq_rows, x_rows, row_off, key, *, radius: int = 1, tau=None, k: int = 0, scale: float = 10.0,
                  normalize: str = "reference", keep_all: bool = False, max_row_edges=None, workspace: "Workspace | None" = None,
                  hw=None, block_rows: bool = False) -> dict:
    """A graph structure moved onto new features (``dagl_graph_refresh``, csrc/graph_refresh.hip) -> dict(row_off [B*L+1] int64, key [E]
    int32, weight [E] fp32, score [E] fp32), keys strictly ascending inside a row.  Operands as ``graph_attend``.  Per row the candidates
    are the set of keys in the (2 radius + 1)^2 windows around its edges' keys (clipped at the map border; keys outside [0, N) contribute
    nothing, repeats count once), scored exactly (``score`` = the bits ``graph_attend`` gives the pair); with ``tau`` [B*L] a candidate
    passes when S - tau_r > 0; with ``k`` > 0 the min(k, passing) best stay, a tie at the last place going to the lower key;
    ``keep_all``: every candidate stays (the dilated graph; ``k`` is not looked at, edges with margin 0 weigh 0).  ``weight`` is
    ``graph_attend``'s on the output structure with the same ``tau``, ``scale``, ``normalize``.

    ``max_row_edges``: the largest degree of the input (None = one host read of it); ``max_row_edges * (2 radius + 1)^2`` must not
    exceed ``graph_refresh_max_candidates()``.  A row longer than declared is never truncated: the call raises ``DaglError`` with
    ``code == ERR_UNSUPPORTED`` naming the count.  The arrays are allocated at capacity and returned as views of their first E
    entries; E and the status words come from one host read (not under stream capture).  ``block_rows``: a block per row also where rows
    are short (for measurements; the same bits).  ``hw``: the map (H, W) -- the windows need it; it may be left out only where L and N
    fit one map alone.  The same arrays give the same bits on every call."""
    lib = _lib.load()
    B, H, W, E, flags, radius, k = _graph_refresh_operands("graph_refresh", wq_rows, x_rows, row_off, key, radius, tau, k, normalize,
                                                           keep_all, block_rows, hw)
    max_row_edges = _graph_refresh_longest("graph_refresh", row_off, E, max_row_edges)
    dev = wq_rows.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_refresh_workspace_bytes", B, H, W, E, radius)
    head, key_out, weight, score, cap = _graph_refresh_arrays(dev, B * wq_rows.shape[1], E, radius, k, keep_all)
    check(lib.dagl_graph_refresh(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), E,
                                 max_row_edges, radius, _ptr(tau), k, float(scale), flags, head.data_ptr(), _ptr(key_out, E > 0),
                                 _ptr(weight, E > 0), _ptr(score, E > 0), cap, head[-2:].data_ptr(), a, nbytes), "dagl_graph_refresh")
    del buf
    return _graph_refresh_result("graph_refresh", head, key_out, weight, score, max_row_edges)


def _graph_refresh_operands(who: str, wq_rows, x_rows, row_off, key, radius, tau, k, normalize, keep_all, block_rows, hw):
    """What ``graph_refresh`` and ``graph_step`` ask of their operands -> (B, H, W, E, flags, radius, k)."""
    if hw is None and isinstance(wq_rows, torch.Tensor) and isinstance(x_rows, torch.Tensor) and wq_rows.dim() == 3 and x_rows.dim() == 3:
        # (the windows need the map itself: L and N alone leave H x W and W x H apart only when one of them does not fit)
        L, N = wq_rows.shape[1], x_rows.shape[1]
        maps = list(_maps_of(L, N))
        if len(maps) > 1:
            raise DaglError(f"{who}: {len(maps)} maps have {N} keys and {L} queries ({maps[0][0]}x{maps[0][1]}, "
                            f"{maps[1][0]}x{maps[1][1]}, ...): pass hw=(H, W)")
        hw = maps[0] if maps else None
    B, H, W, E, flags = _graph_attend_operands(who, wq_rows, x_rows, row_off, key, tau, normalize, hw)
    if keep_all:
        flags |= _lib.GRAPH_REFRESH_KEEP_ALL
    if block_rows:
        flags |= _lib.GRAPH_REFRESH_BLOCK_ROWS
    return B, H, W, E, flags, int(radius), int(k)


def _graph_refresh_longest(who: str, row_off, E: int, max_row_edges) -> int:
    """The refusal under capture of a call that reads the edge count, then ``max_row_edges`` (None = one host read of it)."""
    if torch.cuda.is_current_stream_capturing():
        raise DaglError(f"{who}: not available under stream capture (the edge count is read on the host)")
    if max_row_edges is None:
        max_row_edges = int((row_off[1:] - row_off[:-1]).max()) if E > 0 else 0
    return int(max_row_edges)


def _graph_refresh_arrays(dev, n_rows: int, E: int, radius: int, k: int, keep_all: bool):
    """The output arrays at capacity -> (head [n_rows + 3] int64, key, weight, score, capacity): the offsets and the two status words
    share ``head``, so E and the status come from one host read."""
    cap = E * (2 * radius + 1) ** 2
    if k > 0 and not keep_all:
        cap = min(cap, n_rows * k)
    head = torch.empty(n_rows + 3, device=dev, dtype=torch.int64)
    key_out = torch.empty(cap, device=dev, dtype=torch.int32)
    weight = torch.empty(cap, device=dev, dtype=torch.float32)
    score = torch.empty(cap, device=dev, dtype=torch.float32)
    return head, key_out, weight, score, cap


def _graph_refresh_result(who: str, head, key_out, weight, score, max_row_edges: int, adjacent: bool = False) -> dict:
    """The one host read (E and the status words), the overlong-row refusal, the arrays as views of their first E entries.
    ``adjacent`` (a search call with ``propagate``): a row next to an overlong one is left empty and counted too."""
    total, overlong, _most = (int(v) for v in head[-3:].tolist())          # the one synchronisation
    if overlong:
        err = DaglError(f"{who}: {overlong} row(s) hold{' or lie next to a row that holds' if adjacent else ''} more than "
                        f"max_row_edges = {max_row_edges} edges; they were left empty, "
                        "not truncated: state the input's largest degree")
        err.code = _lib.ERR_UNSUPPORTED
        raise err
    return dict(row_off=head[:-2], key=key_out[:total], weight=weight[:total], score=score[:total])


@_on_device
def graph_step(wq_rows, x_rows, b2p, row_off, key, *, radius: int = 1, tau=None, k: int = 0, scale: float = 10.0,
               normalize: str = "reference", keep_all: bool = False, max_row_edges=None, want_graph: bool = True,
               workspace: "Workspace | None" = None, hw=None, block_rows: bool = False):
    """``graph_refresh`` and the block's output on its result in one call (``dagl_graph_step``, csrc/graph_refresh.hip) ->
    (out [B,16,H,W], dict | None, status): the operands and arguments of ``graph_refresh`` plus ``b2p``, the zero-bordered NHWC value map
    [B,H+6,W+6,16] (it names the map: ``hw`` is not needed).  The dict holds, bit for bit, what ``graph_refresh`` returns for the same
    arguments; ``out = fold(agg) / cnt`` with ``agg[r] = sum_c weight_c V[key_c]`` over the kept entries of row r in ascending key order,
    one fp32 fmaf chain per element -- the same bits with ``want_graph`` True or False, a wavefront or a block per row (``block_rows``),
    on every call.  A row with nothing kept gives zeros.  ``status``: the device int64[2] tensor (rows longer than ``max_row_edges``, the
    largest number of distinct candidates a row had).

    ``want_graph=True``: one host read (E and the status words; not under stream capture); a row longer than declared raises
    ``DaglError`` with ``code == ERR_UNSUPPORTED`` as in ``graph_refresh``.  ``want_graph=False``: the output alone -- nothing is read
    on the host and the call can be captured, so ``max_row_edges`` must be given; a row longer than declared contributes zeros and is
    counted in ``status[0]``, which is left for the caller to read; it is never truncated."""
    lib = _lib.load()
    who = "graph_step"
    _need(b2p, "b2p")
    map_hw = _value_map(who, b2p)[1:]
    if hw is not None and tuple(int(v) for v in hw) != tuple(map_hw):
        raise DaglError(f"{who}: hw={tuple(hw)} but b2p is the value map of a {map_hw[0]}x{map_hw[1]} image")
    B, H, W, E, flags, radius, k = _graph_refresh_operands(who, wq_rows, x_rows, row_off, key, radius, tau, k, normalize, keep_all,
                                                           block_rows, map_hw)
    if b2p.shape[0] != B:
        raise DaglError(f"{who}: b2p holds {b2p.shape[0]} images, the feature rows {B}")
    if want_graph:
        max_row_edges = _graph_refresh_longest(who, row_off, E, max_row_edges)
    elif max_row_edges is None:
        raise DaglError(f"{who}: want_graph=False needs max_row_edges, the input's largest degree"
                        + (" (reading it on the host is not available under stream capture)"
                           if torch.cuda.is_current_stream_capturing() else " (the call itself reads nothing on the host)"))
    max_row_edges = int(max_row_edges)
    dev = wq_rows.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_step_workspace_bytes", B, H, W, E, radius, 1 if want_graph else 0)
    out = torch.empty(B, 16, H, W, device=dev, dtype=torch.float32)
    if want_graph:
        head, key_out, weight, score, cap = _graph_refresh_arrays(dev, B * wq_rows.shape[1], E, radius, k, keep_all)
        status = head[-2:]
    else:
        head = key_out = weight = score = None
        cap, status = 0, torch.empty(2, device=dev, dtype=torch.int64)
    check(lib.dagl_graph_step(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), row_off.data_ptr(),
                              _ptr(key, E > 0), E, max_row_edges, radius, _ptr(tau), k, float(scale), flags, out.data_ptr(), _ptr(head),
                              _ptr(key_out, E > 0), _ptr(weight, E > 0), _ptr(score, E > 0), cap, status.data_ptr(), a, nbytes),
          "dagl_graph_step")
    del buf
    if not want_graph:
        return out, None, status
    return out, _graph_refresh_result(who, head, key_out, weight, score, max_row_edges), status


GRAPH_SEARCH_MAX_EXPLORE = 256      # random keys a row of ``graph_search`` may ask for (the library's limit)


def graph_search_row_bound(max_row_edges: int, radius: int, propagate, explore: int) -> int:
    """Candidates a row of ``graph_search`` may expand into, ``(1 + 4 propagate) max_row_edges (2 radius + 1)^2 + explore``: it must
    not exceed ``graph_refresh_max_candidates()``."""
    return (1 + 4 * int(bool(propagate))) * int(max_row_edges) * (2 * int(radius) + 1) ** 2 + int(explore)


def _graph_search_operands(who: str, propagate, explore, seed):
    """What the search calls ask of their three arguments, before any pointer is taken -> (propagate 0 / 1, explore, seed as uint32)."""
    if isinstance(propagate, torch.Tensor) or propagate not in (0, 1, False, True):
        raise DaglError(f"{who}: propagate={propagate!r}, expected False or True")
    if isinstance(explore, bool) or not isinstance(explore, int) or not 0 <= explore <= GRAPH_SEARCH_MAX_EXPLORE:
        raise DaglError(f"{who}: explore={explore!r} outside [0, {GRAPH_SEARCH_MAX_EXPLORE}]")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise DaglError(f"{who}: seed={seed!r}, an int expected")
    return int(bool(propagate)), explore, seed & 0xFFFFFFFF


def _graph_search_arrays(dev, n_rows: int, E: int, radius: int, k: int, keep_all: bool, propagate: int, explore: int):
    """``_graph_refresh_arrays`` at the capacity a search call may produce: ``(1 + 4 propagate) E (2 radius + 1)^2 + explore n_rows``, or
    ``n_rows k`` under a rank cut where that is smaller.  Both flags off: the plain refresh's arrays."""
    if not propagate and not explore:
        return _graph_refresh_arrays(dev, n_rows, E, radius, k, keep_all)
    cap = (1 + 4 * propagate) * E * (2 * radius + 1) ** 2 + explore * n_rows
    if k > 0 and not keep_all:
        cap = min(cap, n_rows * k)
    head = torch.empty(n_rows + 3, device=dev, dtype=torch.int64)
    key_out = torch.empty(cap, device=dev, dtype=torch.int32)
    weight = torch.empty(cap, device=dev, dtype=torch.float32)
    score = torch.empty(cap, device=dev, dtype=torch.float32)
    return head, key_out, weight, score, cap


@_on_device
def graph_search(wq_rows, x_rows, row_off, key, *, radius: int = 1, tau=None, k: int = 0, scale: float = 10.0,
                 normalize: str = "reference", keep_all: bool = False, max_row_edges=None, workspace: "Workspace | None" = None,
                 hw=None, block_rows: bool = False, propagate=False, explore: int = 0, seed: int = 0) -> dict:
    """``graph_refresh`` with two more candidate sources (``dagl_graph_search``, csrc/graph_refresh.hip) -> the same dict.  Per row the
    candidates are the set union of (a) ``graph_refresh``'s windows around the row's own edges; (b) ``propagate``: for each of the four
    queries adjacent to the row's in the stride-4 query grid of the same image (never across a grid-row end or an image boundary)
    the windows around its edges' keys shifted by the query offset, ``(y - 4 dqy, x - 4 dqx)``, clipped cell by cell -- the adjacent
    rows are read from the input graph, so the result does not depend on scheduling; (c) ``explore`` (0 .. 256) keys of the row's
    image from a stateless counter hash of (row, ``seed``, t), no window around them.  Everything after the expansion is
    ``graph_refresh``: a pair's score has the same bits, and with both sources off the call returns ``graph_refresh``'s arrays bit for
    bit.  A row with no edge of its own can be populated by (b) and (c) -- with ``explore`` > 0 also an empty input graph.

    ``max_row_edges`` as in ``graph_refresh``; ``graph_search_row_bound(max_row_edges, radius, propagate, explore)`` must not exceed
    ``graph_refresh_max_candidates()``.  A row whose own or (``propagate``) adjacent row is longer than declared comes out empty, never
    truncated, and the call raises ``DaglError`` with ``code == ERR_UNSUPPORTED`` naming the count.  One host read; not under stream
    capture.  The same arrays and seed give the same bits on every call."""
    lib = _lib.load()
    who = "graph_search"
    propagate, explore, seed = _graph_search_operands(who, propagate, explore, seed)
    B, H, W, E, flags, radius, k = _graph_refresh_operands(who, wq_rows, x_rows, row_off, key, radius, tau, k, normalize, keep_all,
                                                           block_rows, hw)
    max_row_edges = _graph_refresh_longest(who, row_off, E, max_row_edges)
    dev = wq_rows.device
    n_rows = B * wq_rows.shape[1]
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_search_workspace_bytes", B, H, W, E, radius, propagate, explore,
                                   0 if keep_all else k, 1, 0)
    head, key_out, weight, score, cap = _graph_search_arrays(dev, n_rows, E, radius, k, keep_all, propagate, explore)
    check(lib.dagl_graph_search(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), E,
                                max_row_edges, radius, _ptr(tau), k, float(scale), flags, head.data_ptr(), _ptr(key_out, cap > 0),
                                _ptr(weight, cap > 0), _ptr(score, cap > 0), cap, head[-2:].data_ptr(), a, nbytes, propagate, explore,
                                seed), "dagl_graph_search")
    del buf
    return _graph_refresh_result(who, head, key_out, weight, score, max_row_edges, adjacent=bool(propagate))


@_on_device
def graph_search_step(wq_rows, x_rows, b2p, row_off, key, *, radius: int = 1, tau=None, k: int = 0, scale: float = 10.0,
                      normalize: str = "reference", keep_all: bool = False, max_row_edges=None, want_graph: bool = True,
                      workspace: "Workspace | None" = None, hw=None, block_rows: bool = False, propagate=False, explore: int = 0,
                      seed: int = 0):
    """``graph_step`` with ``graph_search``'s candidate sources (``dagl_graph_search_step``, csrc/graph_refresh.hip) ->
    (out [B,16,H,W], dict | None, status): the dict holds, bit for bit, what ``graph_search`` returns for the same arguments, ``out``
    is ``graph_step``'s aggregation of the kept entries -- the same bits with ``want_graph`` True or False.  Host reads, capture,
    ``max_row_edges`` and the overlong-row rule as in ``graph_step``; ``seed`` is a launch argument: a captured call replays the seed
    it was captured with."""
    lib = _lib.load()
    who = "graph_search_step"
    propagate, explore, seed = _graph_search_operands(who, propagate, explore, seed)
    _need(b2p, "b2p")
    map_hw = _value_map(who, b2p)[1:]
    if hw is not None and tuple(int(v) for v in hw) != tuple(map_hw):
        raise DaglError(f"{who}: hw={tuple(hw)} but b2p is the value map of a {map_hw[0]}x{map_hw[1]} image")
    B, H, W, E, flags, radius, k = _graph_refresh_operands(who, wq_rows, x_rows, row_off, key, radius, tau, k, normalize, keep_all,
                                                           block_rows, map_hw)
    if b2p.shape[0] != B:
        raise DaglError(f"{who}: b2p holds {b2p.shape[0]} images, the feature rows {B}")
    if want_graph:
        max_row_edges = _graph_refresh_longest(who, row_off, E, max_row_edges)
    elif max_row_edges is None:
        raise DaglError(f"{who}: want_graph=False needs max_row_edges, the input's largest degree"
                        + (" (reading it on the host is not available under stream capture)"
                           if torch.cuda.is_current_stream_capturing() else " (the call itself reads nothing on the host)"))
    max_row_edges = int(max_row_edges)
    dev = wq_rows.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_search_workspace_bytes", B, H, W, E, radius, propagate, explore,
                                   0 if keep_all else k, 1 if want_graph else 0, 1)
    out = torch.empty(B, 16, H, W, device=dev, dtype=torch.float32)
    if want_graph:
        head, key_out, weight, score, cap = _graph_search_arrays(dev, B * wq_rows.shape[1], E, radius, k, keep_all, propagate, explore)
        status = head[-2:]
    else:
        head = key_out = weight = score = None
        cap, status = 0, torch.empty(2, device=dev, dtype=torch.int64)
    check(lib.dagl_graph_search_step(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), row_off.data_ptr(),
                                     _ptr(key, E > 0), E, max_row_edges, radius, _ptr(tau), k, float(scale), flags, out.data_ptr(),
                                     _ptr(head), _ptr(key_out, cap > 0), _ptr(weight, cap > 0), _ptr(score, cap > 0), cap,
                                     status.data_ptr(), a, nbytes, propagate, explore, seed), "dagl_graph_search_step")
    del buf
    if not want_graph:
        return out, None, status
    return out, _graph_refresh_result(who, head, key_out, weight, score, max_row_edges, adjacent=bool(propagate)), status


@_on_device
def graph_step_fixed(wq_rows, x_rows, b2p, key, deg, *, width_out: int, radius: int = 1, tau=None, k: int = 0, scale: float = 10.0,
                     normalize: str = "reference", keep_all: bool = False, propagate=False, explore: int = 0, seed: int = 0,
                     workspace: "Workspace | None" = None, hw=None, block_rows: bool = False):
    """``graph_step`` (``b2p`` given), ``graph_refresh`` (``b2p`` None) and -- ``propagate`` / ``explore`` -- their search forms on a
    FIXED-WIDTH graph (``dagl_graph_step_fixed``, csrc/graph_refresh.hip) -> (out [B,16,H,W] | None, dict(key, weight, score, deg),
    status).  ``key`` [B*L, width_in] int32 and ``deg`` [B*L] int32 hold row r's edges in slots ``0 .. deg[r] - 1`` (``deg`` is read
    clamped to [0, width_in]); the dict holds ``key`` / ``weight`` / ``score`` [B*L, width_out] and ``deg`` [B*L]: the kept entries in
    ascending key order, then ``(-1, 0, 0)`` -- every slot is written.  For the same rows the kept entries and ``out`` carry the bits
    the CSR calls give with ``max_row_edges = width_in``.  A row that keeps more than ``width_out`` entries (possible only without a
    rank cut) comes out EMPTY and is counted in ``status[0]`` (device int64[2], left for the caller to read); it is never truncated.
    With ``k`` > 0 and no ``keep_all``, ``width_out >= min(k, N)`` is required.

    One row launch and the fold: no staging, scan or copy.  NOTHING is read on the host in any form of the call, so it can be captured
    into a HIP graph with its graph output.  ``hw`` as in ``graph_refresh`` (``b2p`` names the map when given)."""
    lib = _lib.load()
    who = "graph_step_fixed"
    propagate, explore, seed = _graph_search_operands(who, propagate, explore, seed)
    n_rows, width_in, width_out = _graph_fixed_slots(who, key, deg, width_out)
    B, H, W, L = _graph_fixed_head(who, wq_rows, x_rows, b2p, tau, hw)
    if n_rows != B * L or deg.numel() != n_rows:
        raise DaglError(f"{who}: key holds {n_rows} rows and deg {deg.numel()} degrees, expected B*L = {B * L}")
    flags, radius, k = _graph_fixed_flags(who, normalize, keep_all, block_rows, radius, k, width_out, H * W)
    dev = wq_rows.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_step_fixed_workspace_bytes", B, H, W, 1) if b2p is not None \
        else (None, None, 0)
    out = torch.empty(B, 16, H, W, device=dev, dtype=torch.float32) if b2p is not None else None
    key_out, weight, score, deg_out, status = _graph_fixed_arrays(dev, n_rows, width_out)
    check(lib.dagl_graph_step_fixed(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), _ptr(b2p), key.data_ptr(), deg.data_ptr(),
                                    width_in, radius, _ptr(tau), k, float(scale), flags, propagate, explore, seed, _ptr(out),
                                    key_out.data_ptr(), weight.data_ptr(), score.data_ptr(), deg_out.data_ptr(), width_out,
                                    status.data_ptr(), a, nbytes), "dagl_graph_step_fixed")
    del buf
    return out, dict(key=key_out, weight=weight, score=score, deg=deg_out), status


def _graph_fixed_slots(who: str, key, deg, width_out):
    """The slot array and the degrees of a fixed-width call -> (rows, width_in, width_out)."""
    _need(key, "key", torch.int32); _need(deg, "deg", torch.int32)
    if key.dim() != 2 or key.shape[1] < 1 or deg.dim() != 1:
        raise DaglError(f"{who}: expected key [B*L, width >= 1] and deg [B*L], got {tuple(key.shape)} and {tuple(deg.shape)}")
    width_out = int(width_out)
    if width_out < 1:
        raise DaglError(f"{who}: width_out={width_out} < 1")
    return key.shape[0], key.shape[1], width_out


def _graph_fixed_head(who: str, wq_rows, x_rows, b2p, tau, hw):
    """What a fixed-width call asks of one head's operands (``_graph_refresh_operands``' checks without the offsets: this form has
    none) -> (B, H, W, L).  ``b2p`` None: no value map, ``hw`` names the map where L and N leave it open."""
    _need(wq_rows, "wq_rows"); _need(x_rows, "x_rows")
    if b2p is not None:
        _need(b2p, "b2p")
        map_hw = _value_map(who, b2p)[1:]
        if hw is not None and tuple(int(v) for v in hw) != tuple(map_hw):
            raise DaglError(f"{who}: hw={tuple(hw)} but b2p is the value map of a {map_hw[0]}x{map_hw[1]} image")
        hw = map_hw
    if wq_rows.dim() != 3 or x_rows.dim() != 3 or wq_rows.shape[2] != D or x_rows.shape[2] != D or wq_rows.shape[0] != x_rows.shape[0]:
        raise DaglError(f"{who}: expected wq_rows [B,L,{D}] and x_rows [B,N,{D}], got {tuple(wq_rows.shape)} and {tuple(x_rows.shape)}")
    B, L, N = wq_rows.shape[0], wq_rows.shape[1], x_rows.shape[1]
    if hw is None:
        maps = list(_maps_of(L, N))
        if len(maps) != 1:
            raise DaglError(f"{who}: {len(maps)} maps have {N} keys and {L} queries: pass hw=(H, W)")
        hw = maps[0]
    H, W = (int(v) for v in hw)
    if H * W != N or math.prod(query_grid(H, W)) != L:
        raise DaglError(f"{who}: a {H}x{W} map has {math.prod(query_grid(H, W))} queries and {H * W} keys, the feature rows hold {L} "
                        f"and {N}")
    if tau is not None:
        _need(tau, "tau")
        if tau.numel() != B * L:
            raise DaglError(f"{who}: tau holds {tau.numel()} values, expected B*L = {B * L}")
    if b2p is not None and b2p.shape[0] != B:
        raise DaglError(f"{who}: b2p holds {b2p.shape[0]} images, the feature rows {B}")
    return B, H, W, L


def _graph_fixed_flags(who: str, normalize, keep_all, block_rows, radius, k, width_out: int, N: int):
    """The flags of a fixed-width call and the room a rank cut needs -> (flags, radius, k)."""
    if normalize not in _GRAPH_NORMALIZE:
        raise DaglError(f"{who}: normalize={normalize!r}, expected 'reference' or 'edges'")
    flags = _GRAPH_NORMALIZE[normalize] | (_lib.GRAPH_REFRESH_KEEP_ALL if keep_all else 0) \
        | (_lib.GRAPH_REFRESH_BLOCK_ROWS if block_rows else 0)
    radius, k = int(radius), int(k)
    if k > 0 and not keep_all and width_out < min(k, N):
        raise DaglError(f"{who}: width_out={width_out} < min(k, N) = {min(k, N)} entries a row may keep")
    return flags, radius, k


def _graph_fixed_arrays(dev, n_rows: int, width_out: int):
    """The output arrays of a fixed-width call -> (key, weight, score, deg, status): sizes known before the launch."""
    return (torch.empty(n_rows, width_out, device=dev, dtype=torch.int32), torch.empty(n_rows, width_out, device=dev, dtype=torch.float32),
            torch.empty(n_rows, width_out, device=dev, dtype=torch.float32), torch.empty(n_rows, device=dev, dtype=torch.int32),
            torch.empty(2, device=dev, dtype=torch.int64))


def _stage_mix_operands(who: str, x, mix_w, mix_b, bias: bool = True):
    """x [B,64,H,W], the stage's 1x1 mix weights [64,64] or [64,64,1,1] and bias [64] -> (B, H, W).  ``bias`` False: a call that takes
    no bias (the mix's backward, x = d_out)."""
    _need(x, "x"); _need(mix_w, "mix_w")
    if bias:
        _need(mix_b, "mix_b")
    if x.dim() != 4 or x.shape[1] != 64:
        raise DaglError(f"{who}: expected x [B,64,H,W], got {tuple(x.shape)}")
    if tuple(mix_w.shape) not in ((64, 64), (64, 64, 1, 1)) or (bias and tuple(mix_b.shape) != (64,)):
        raise DaglError(f"{who}: expected mix_w [64,64] and mix_b [64], got {tuple(mix_w.shape)}"
                        + (f" and {tuple(mix_b.shape)}" if bias else ""))
    return x.shape[0], x.shape[2], x.shape[3]


@_on_device
def ces_stage_fold_mix(agg, x, mix_w, mix_b) -> torch.Tensor:
    """The end of a ``CES`` stage from its four heads' aggregated rows in one launch (``dagl_ces_stage_fold_mix``, csrc/aggregate.hip):
    ``conv1x1(cat_h(fold(agg_h) / cnt)) + mix_b + x`` -> [B,64,H,W].  agg [4,B,L,784] head-major, element order (kh, kw, c); x
    [B,64,H,W]; mix_w [64,64] (or [64,64,1,1]), mix_b [64].  The 64 concat values of a pixel are ``fold_normalize``'s bits and never go
    to memory; the product runs on the fp32 matrix cores.  The same arrays give the same bits on every call."""
    who = "ces_stage_fold_mix"
    B, H, W = _stage_mix_operands(who, x, mix_w, mix_b)
    _need(agg, "agg")
    Lh, Lw = query_grid(H, W)
    if tuple(agg.shape) != (4, B, Lh * Lw, P):
        raise DaglError(f"{who}: expected agg [4,{B},{Lh * Lw},{P}] for x {tuple(x.shape)}, got {tuple(agg.shape)}")
    out = torch.empty_like(x)
    check(_lib.load().dagl_ces_stage_fold_mix(_stream(), B, H, W, agg.data_ptr(), x.data_ptr(), mix_w.data_ptr(), mix_b.data_ptr(),
                                              out.data_ptr()), "dagl_ces_stage_fold_mix")
    return out


@_on_device
def ces_stage_mix(cat, x, mix_w, mix_b) -> torch.Tensor:
    """``conv1x1(cat) + mix_b + x`` on a stored concat map cat [B,64,H,W] (``dagl_ces_stage_mix``: the last launch of
    ``ces_stage_forward``, on its own) -- with ``fold_normalize`` in front, the two launches ``ces_stage_fold_mix`` replaces; for
    measurements."""
    B, H, W = _stage_mix_operands("ces_stage_mix", x, mix_w, mix_b)
    _need(cat, "cat")
    if cat.shape != x.shape:
        raise DaglError(f"ces_stage_mix: cat is {tuple(cat.shape)}, x {tuple(x.shape)}")
    out = torch.empty_like(x)
    check(_lib.load().dagl_ces_stage_mix(_stream(), B, H, W, cat.data_ptr(), x.data_ptr(), mix_w.data_ptr(), mix_b.data_ptr(),
                                         out.data_ptr()), "dagl_ces_stage_mix")
    return out


@_on_device
def graph_stage_forward(wq4, x4, b2p4, row_off, key, x, mix_w, mix_b, *, tau4=None, scale: float = 10.0, normalize: str = "reference",
                        train: bool = False, workspace: "Workspace | None" = None):
    """A whole ``CES`` stage on its FROZEN graph in one launch set (``dagl_graph_stage_forward``, csrc/graph_forward.hip) -> ``out``
    [B,64,H,W], or ``(out, row_max [4*B*L] fp32, row_sum [4*B*L] fp64, cat4 [4,B,16,H,W])`` with ``train=True``.  wq4 [4,B,L,196], x4
    [4,B,N,196], b2p4 [4,B,H+6,W+6,16], tau4 [4,B,L] | None: the four heads' ``graph_forward`` operands stacked head-major (what
    ``graph_stage_features16`` hands out); (row_off [4*B*L+1], key [E]) ONE CSR over the head-major rows, row ``(h * B + b) * L + i`` =
    query ``i`` of image ``b`` under head ``h`` (a ``SequenceState`` stage); x [B,64,H,W] the stage's input, mix_w / mix_b its 1x1 mix.

    ``graph_forward``'s segment and combine launches run once over the 4*B*L rows, then ``ces_stage_fold_mix`` on the aggregated rows:
    every row is ``graph_forward``'s for its head bit for bit, an empty graph gives ``mix_b + x``.  ``train=True`` adds the row
    statistics of ``graph_forward_train`` and ``cat4``, the pre-mix concat map head-major (``graph_forward``'s output of the stacked
    operands) -- what ``ces_stage_mix_backward`` and ``graph_forward_backward`` need next to the operands; ``out`` keeps its bits.
    Nothing is read on the host; the same arrays give the same bits on every call."""
    lib = _lib.load()
    who = "graph_stage_forward"
    B, H, W = _stage_mix_operands(who, x, mix_w, mix_b)
    for name, t in (("wq4", wq4), ("x4", x4), ("b2p4", b2p4)) + ((("tau4", tau4),) if tau4 is not None else ()):
        _need(t, name)
        if t.dim() < 2 or t.shape[0] != 4 or t.shape[1] != B:
            raise DaglError(f"{who}: {name} must be head-major [4,{B},...] for x {tuple(x.shape)}, got {tuple(t.shape)}")
    # the stacked operands are those of 4 B images: graph_forward's own checks on that view
    B4, H4, W4, E, flags = _graph_forward_operands(who, wq4.flatten(0, 1), x4.flatten(0, 1), b2p4.flatten(0, 1), row_off, key,
                                                   tau4.flatten(0, 1) if tau4 is not None else None, normalize)
    if (H4, W4) != (H, W):
        raise DaglError(f"{who}: b2p4 is the value map of {H4}x{W4} images, x holds {H}x{W}")
    dev = x.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_stage_forward_workspace_bytes", B, H, W, E)
    out = torch.empty_like(x)
    row_max = row_sum = cat4 = None
    if train:
        row_max = torch.empty(B4 * wq4.shape[2], device=dev, dtype=torch.float32)
        row_sum = torch.empty(B4 * wq4.shape[2], device=dev, dtype=torch.float64)
        cat4 = torch.empty(4, B, 16, H, W, device=dev, dtype=torch.float32)
    check(lib.dagl_graph_stage_forward(_stream(), B, H, W, wq4.data_ptr(), x4.data_ptr(), b2p4.data_ptr(), row_off.data_ptr(),
                                       _ptr(key, E > 0), E, _ptr(tau4), float(scale), flags, x.data_ptr(), mix_w.data_ptr(),
                                       mix_b.data_ptr(), out.data_ptr(), _ptr(row_max), _ptr(row_sum), _ptr(cat4), a, nbytes),
          "dagl_graph_stage_forward")
    del buf
    return (out, row_max, row_sum, cat4) if train else out


@_on_device
def ces_stage_mix_backward(d_out, cat4, mix_w, need_w: bool = True, need_b: bool = True, workspace: "Workspace | None" = None):
    """The backward of a stage's 1x1 mix + residual on the head-major concat map (``dagl_ces_stage_mix_backward``,
    csrc/stage_mix_grad.hip) -> ``(d_cat4 [4,B,16,H,W], d_mix_w [64,64] | None, d_mix_b [64] | None)`` from d_out [B,64,H,W], the
    ``cat4`` [4,B,16,H,W] that ``graph_stage_forward(train=True)`` left and mix_w [64,64] (or [64,64,1,1]).
    ``d_cat4[h,b,c] = sum_o mix_w[o][16 h + c] d_out[b,o]``: viewed as [4*B,16,H,W] it is ``graph_forward_backward``'s ``d_out`` on the
    stacked operands (which divides by the overlap count; nothing is divided here).  ``d_mix_w = sum_{b,p} d_out[b,o,p] cat[b,c,p]``,
    ``d_mix_b = sum_{b,p} d_out[b,o,p]``: per-wave partial tiles on the fp32 matrix cores, added in a fixed order in fp64.  The gradient
    of the residual input is ``d_out``.  The same operands give the same bits on every call, whatever ``need_w`` / ``need_b``."""
    lib = _lib.load()
    who = "ces_stage_mix_backward"
    B, H, W = _stage_mix_operands(who, d_out, mix_w, None, bias=False)
    _need(cat4, "cat4")
    if tuple(cat4.shape) != (4, B, 16, H, W):
        raise DaglError(f"{who}: expected cat4 [4,{B},16,{H},{W}] for d_out {tuple(d_out.shape)}, got {tuple(cat4.shape)}")
    dev = d_out.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_ces_stage_mix_backward_workspace_bytes", B, H, W)
    d_cat4 = torch.empty_like(cat4)
    d_w = torch.empty(64, 64, device=dev, dtype=torch.float32) if need_w else None
    d_b = torch.empty(64, device=dev, dtype=torch.float32) if need_b else None
    check(lib.dagl_ces_stage_mix_backward(_stream(), B, H, W, d_out.data_ptr(), cat4.data_ptr(), mix_w.data_ptr(), d_cat4.data_ptr(),
                                          _ptr(d_w), _ptr(d_b), a, nbytes), "dagl_ces_stage_mix_backward")
    del buf
    return d_cat4, d_w, d_b


@_on_device
def graph_stage_step(wq_rows4, x_rows4, b2p4, row_off, key, x, mix_w, mix_b, *, radius: int = 1, tau4=None, k: int = 0,
                     scale: float = 10.0, normalize: str = "reference", keep_all: bool = False, max_row_edges=None,
                     want_graph: bool = True, workspace: "Workspace | None" = None, block_rows: bool = False):
    """``graph_step`` for the four heads of a ``CES`` stage and the stage's mix on the result, in one call (``dagl_graph_stage_step``,
    csrc/graph_refresh.hip) -> (out [B,64,H,W], dict | None, status).  wq_rows4 / x_rows4 / b2p4 / tau4: sequences of four tensors, entry
    h what ``graph_step`` takes for head h (``tau4`` None: no margin); (row_off [4*B*L+1], key [E]) ONE CSR over the head-major rows,
    row ``(h * B + b) * L + i`` = query ``i`` of image ``b`` under head ``h``; x [B,64,H,W] the stage's input, mix_w / mix_b its 1x1 mix.
    The features stay where they are: the row kernel runs once per head on its slice of the offsets.

    The dict holds ONE CSR over the 4*B*L rows: rows ``h*B*L .. (h+1)*B*L`` are, bit for bit, what ``graph_step`` returns for head h's
    operands and its slice of the input graph (offsets continuing from head to head); ``out`` is ``ces_stage_fold_mix`` of the heads'
    aggregated rows, each ``graph_step``'s bits -- the same with ``want_graph`` True or False and on every call.  An empty graph gives
    ``mix_b + x``.  ``status``: device int64[2] (rows longer than ``max_row_edges`` summed over the heads, the largest candidate count).

    Host reads, ``max_row_edges``, the overlong-row refusal and capture: as ``graph_step`` -- one host read with ``want_graph=True``; none
    with ``want_graph=False``, which needs ``max_row_edges``."""
    lib = _lib.load()
    who = "graph_stage_step"
    for name, seq in (("wq_rows4", wq_rows4), ("x_rows4", x_rows4), ("b2p4", b2p4)) + ((("tau4", tau4),) if tau4 is not None else ()):
        if not isinstance(seq, (list, tuple)) or len(seq) != 4:
            raise DaglError(f"{who}: {name} must be a sequence of four tensors, one per head")
    B, H, W = _stage_mix_operands(who, x, mix_w, mix_b)
    _need(row_off, "row_off", torch.int64)
    L = math.prod(query_grid(H, W))
    if row_off.dim() != 1 or row_off.numel() != 4 * B * L + 1:
        raise DaglError(f"{who}: row_off holds {row_off.numel()} offsets, expected 4*B*L+1 = {4 * B * L + 1}")
    head_off = row_off[:B * L + 1]              # (a head's view: the shape checks of graph_step, head by head)
    for h in range(4):
        _need(b2p4[h], "b2p4[%d]" % h)
        map_hw = _value_map(who, b2p4[h])[1:]
        if tuple(map_hw) != (H, W) or b2p4[h].shape[0] != B:
            raise DaglError(f"{who}: b2p4[{h}] is the value map of {b2p4[h].shape[0]} {map_hw[0]}x{map_hw[1]} images, x holds {B} of {H}x{W}")
        Bh, _, _, E, flags, radius, k = _graph_refresh_operands(who, wq_rows4[h], x_rows4[h], head_off, key, radius,
                                                                tau4[h] if tau4 is not None else None, k, normalize, keep_all,
                                                                block_rows, (H, W))
        if Bh != B:
            raise DaglError(f"{who}: head {h}'s feature rows hold {Bh} images, x {B}")
    if want_graph:
        max_row_edges = _graph_refresh_longest(who, row_off, E, max_row_edges)
    elif max_row_edges is None:
        raise DaglError(f"{who}: want_graph=False needs max_row_edges, the input's largest degree"
                        + (" (reading it on the host is not available under stream capture)"
                           if torch.cuda.is_current_stream_capturing() else " (the call itself reads nothing on the host)"))
    max_row_edges = int(max_row_edges)
    dev = x.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_stage_step_workspace_bytes", B, H, W, E, radius, 1 if want_graph else 0)
    out = torch.empty_like(x)
    if want_graph:
        head, key_out, weight, score, cap = _graph_refresh_arrays(dev, 4 * B * L, E, radius, k, keep_all)
        status = head[-2:]
    else:
        head = key_out = weight = score = None
        cap, status = 0, torch.empty(2, device=dev, dtype=torch.int64)
    table = lambda seq: (C.c_void_p * 4)(*[t.data_ptr() for t in seq])
    check(lib.dagl_graph_stage_step(_stream(), B, H, W, table(wq_rows4), table(x_rows4), table(b2p4), row_off.data_ptr(), _ptr(key, E > 0),
                                    E, max_row_edges, radius, table(tau4) if tau4 is not None else None, k, float(scale), flags,
                                    x.data_ptr(), mix_w.data_ptr(), mix_b.data_ptr(), out.data_ptr(), _ptr(head), _ptr(key_out, E > 0),
                                    _ptr(weight, E > 0), _ptr(score, E > 0), cap, status.data_ptr(), a, nbytes), "dagl_graph_stage_step")
    del buf
    if not want_graph:
        return out, None, status
    return out, _graph_refresh_result(who, head, key_out, weight, score, max_row_edges), status


@_on_device
def graph_stage_step_fixed(wq_rows4, x_rows4, b2p4, key, deg, x=None, mix_w=None, mix_b=None, *, width_out: int, radius: int = 1,
                           tau4=None, k: int = 0, scale: float = 10.0, normalize: str = "reference", keep_all: bool = False,
                           propagate=False, explore: int = 0, seed: int = 0, workspace: "Workspace | None" = None, hw=None,
                           block_rows: bool = False):
    """``graph_step_fixed`` for the four heads of a ``CES`` stage in ONE row launch and the stage's mix on the result
    (``dagl_graph_stage_step_fixed``, csrc/graph_refresh.hip) -> (out [B,64,H,W] | None, dict(key, weight, score, deg), status).
    wq_rows4 / x_rows4 / b2p4 / tau4, x, mix_w, mix_b as ``graph_stage_step``; ``key`` [4*B*L, width_in] int32 and ``deg`` [4*B*L]
    int32 the stage's fixed-width graph over the head-major rows, row ``(h * B + b) * L + i`` = query ``i`` of image ``b`` under head
    ``h``.  The dict's arrays run over the same rows at ``width_out``: rows ``h*B*L .. (h+1)*B*L`` are, bit for bit and filler
    included, what ``graph_step_fixed`` returns for head h's operands and its rows of the input with the same arguments (the random
    keys are hashed from the head-local row, propagation never leaves an image); ``out`` is ``ces_stage_fold_mix`` of the heads'
    aggregated rows.  ``status``: device int64[2] -- the rows that came out empty for their length summed over the heads, the largest
    candidate count.

    ``b2p4``, ``x``, ``mix_w`` and ``mix_b`` all None: the graph alone (``out`` is None) -- the graph-only iterations of a search;
    ``hw`` then names the map where L and N leave it open.  The memset of the status words, one row launch, the fold + mix: no
    staging, scan or copy, and NOTHING is read on the host, so every form of the call can be captured with its graph output."""
    lib = _lib.load()
    who = "graph_stage_step_fixed"
    propagate, explore, seed = _graph_search_operands(who, propagate, explore, seed)
    step = b2p4 is not None
    if (x is not None, mix_w is not None, mix_b is not None) != (step,) * 3:
        raise DaglError(f"{who}: b2p4, x, mix_w and mix_b come together (all None: the graph alone)")
    tables = (("wq_rows4", wq_rows4), ("x_rows4", x_rows4)) + ((("b2p4", b2p4),) if step else ()) \
        + ((("tau4", tau4),) if tau4 is not None else ())
    for name, seq in tables:
        if not isinstance(seq, (list, tuple)) or len(seq) != 4:
            raise DaglError(f"{who}: {name} must be a sequence of four tensors, one per head")
    n_rows, width_in, width_out = _graph_fixed_slots(who, key, deg, width_out)
    if step:
        B, H, W = _stage_mix_operands(who, x, mix_w, mix_b)
        if hw is not None and tuple(int(v) for v in hw) != (H, W):
            raise DaglError(f"{who}: hw={tuple(hw)} but x is a {H}x{W} map")
        hw = (H, W)
    shapes = {_graph_fixed_head(who, wq_rows4[h], x_rows4[h], b2p4[h] if step else None, tau4[h] if tau4 is not None else None, hw)
              for h in range(4)}
    if len(shapes) != 1 or (step and next(iter(shapes))[:3] != (B, H, W)):
        raise DaglError(f"{who}: the four heads' operands must share B, H and W" + (f" with x {tuple(x.shape)}" if step else "")
                        + f", got {sorted(shapes)}")
    B, H, W, L = next(iter(shapes))
    if n_rows != 4 * B * L or deg.numel() != n_rows:
        raise DaglError(f"{who}: key holds {n_rows} rows and deg {deg.numel()} degrees, expected 4*B*L = {4 * B * L}")
    flags, radius, k = _graph_fixed_flags(who, normalize, keep_all, block_rows, radius, k, width_out, H * W)
    dev = key.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_stage_step_fixed_workspace_bytes", B, H, W, 1) if step else (None, None, 0)
    out = torch.empty_like(x) if step else None
    key_out, weight, score, deg_out, status = _graph_fixed_arrays(dev, n_rows, width_out)
    table = lambda seq: (C.c_void_p * 4)(*[t.data_ptr() for t in seq])
    check(lib.dagl_graph_stage_step_fixed(_stream(), B, H, W, table(wq_rows4), table(x_rows4), table(b2p4) if step else None,
                                          key.data_ptr(), deg.data_ptr(), width_in, radius, table(tau4) if tau4 is not None else None, k,
                                          float(scale), flags, propagate, explore, seed, _ptr(x), _ptr(mix_w), _ptr(mix_b), _ptr(out),
                                          key_out.data_ptr(), weight.data_ptr(), score.data_ptr(), deg_out.data_ptr(), width_out,
                                          status.data_ptr(), a, nbytes), "dagl_graph_stage_step_fixed")
    del buf
    return out, dict(key=key_out, weight=weight, score=score, deg=deg_out), status


_HEAD_SHAPES = {"g.weight": (16, 64, 3, 3), "g.bias": (16,), "theta.weight": (16, 64, 1, 1), "theta.bias": (16,),
                "thr_conv.weight": (1, 64, 7, 7), "thr_conv.bias": (1,), "bias_conv.weight": (1, 64, 7, 7), "bias_conv.bias": (1,),
                "fc1.0.weight": (D, P), "fc1.0.bias": (D,), "fc2.0.weight": (D, P), "fc2.0.bias": (D,)}


@_on_device
def graph_stage_features16(x, heads, margin: bool, workspace: "Workspace | None" = None):
    """The features of a whole ``CES`` stage for the stage-fused patch-graph calls in one launch set
    (``dagl_graph_stage_features16``, csrc/stage_features.hip) -> ``(wq4 [n,B,L,196], x4 [n,B,N,196], b2p4 [n,B,H+6,W+6,16],
    tau4 [n,B,L] | None)`` for the ``n`` = 1..4 (a stage: four) heads of ``heads``: dicts of state_dict names -> contiguous fp32 GPU
    tensors of the default head (ksize 7, 16 inner channels, 64 input channels; ``thr_conv.*`` / ``bias_conv.*`` are looked at with
    ``margin`` only), all on the shared input ``x`` [B,64,H,W].  ``t[h]`` is head h's operand as ``graph_stage_step`` /
    ``graph_stage_step_fixed`` / ``graph_stage_search*`` take it, already contiguous.

    The inference forward's heads-as-batch kernels: ONE g / theta launch, ONE split-fp16 projection launch for keys and queries of all
    heads, ONE copy-out launch that also forms ``tau`` (the mean over keys from the projection's fp64 column sums).  The map side has
    the forward's range (both tiers of g(x), the input's per-block scale); weights beyond the split's range or a non-finite ``x``
    NaN-fill EVERY element of all the arrays, of every head -- one range word per call -- never wrong numbers.  Nothing is read on
    the host: the call can be captured (the workspace must then have its size before the capture: one eager call)."""
    lib = _lib.load()
    who = "graph_stage_features16"
    _need(x, "x")
    if x.dim() != 4 or x.shape[1] != 64:
        raise DaglError(f"{who}: expected x [B,64,H,W], got {tuple(x.shape)}")
    if not isinstance(heads, (list, tuple)) or not 1 <= len(heads) <= 4:
        raise DaglError(f"{who}: heads must be a sequence of one to four parameter dicts, one per head")
    margin = bool(margin)
    n = len(heads)
    arr = (_lib.CeWeights * n)()
    for h, prm in enumerate(heads):
        for field, name in zip([f for f, _ in _lib.CeWeights._fields_], _lib.CeWeights.NAMES):
            if not margin and name.startswith(("thr_conv.", "bias_conv.")):
                continue
            if name not in prm:
                raise DaglError(f"{who}: head {h} has no {name}")
            t = prm[name]
            _need(t, name)
            if tuple(t.shape) != _HEAD_SHAPES[name]:
                raise DaglError(f"{who}: head {h} {name} is {tuple(t.shape)}, expected {_HEAD_SHAPES[name]}")
            setattr(arr[h], field, t.data_ptr())
    B, _, H, W = x.shape
    Lh, Lw = query_grid(H, W)
    L, N, dev = Lh * Lw, H * W, x.device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_stage_features16_workspace_bytes", n, B, H, W, int(margin))
    wq4 = torch.empty(n, B, L, D, device=dev, dtype=torch.float32)
    x4 = torch.empty(n, B, N, D, device=dev, dtype=torch.float32)
    b2p4 = torch.empty(n, B, H + 6, W + 6, 16, device=dev, dtype=torch.float32)
    tau4 = torch.empty(n, B, L, device=dev, dtype=torch.float32) if margin else None
    check(lib.dagl_graph_stage_features16(_stream(), n, B, H, W, x.data_ptr(), arr, int(margin), wq4.data_ptr(), x4.data_ptr(),
                                          b2p4.data_ptr(), _ptr(tau4), a, nbytes), "dagl_graph_stage_features16")
    del buf
    return wq4, x4, b2p4, tau4


def _graph_stage_search(who: str, entry: str, wq_rows4, x_rows4, b2p4, row_off, key, x, mix_w, mix_b, radius, tau4, k, scale, normalize,
                        keep_all, max_row_edges, want_graph, workspace, block_rows, propagate, explore, seed, head_launches):
    """The body of ``graph_stage_search`` (``b2p4`` None: x names the shape alone) and ``graph_stage_search_step``."""
    lib = _lib.load()
    step = b2p4 is not None
    propagate, explore, seed = _graph_search_operands(who, propagate, explore, seed)
    tables = (("wq_rows4", wq_rows4), ("x_rows4", x_rows4)) + ((("b2p4", b2p4),) if step else ()) \
        + ((("tau4", tau4),) if tau4 is not None else ())
    for name, seq in tables:
        if not isinstance(seq, (list, tuple)) or len(seq) != 4:
            raise DaglError(f"{who}: {name} must be a sequence of four tensors, one per head")
    if step:
        B, H, W = _stage_mix_operands(who, x, mix_w, mix_b)
    else:
        B, H, W = (int(v) for v in x)
    _need(row_off, "row_off", torch.int64)
    L = math.prod(query_grid(H, W))
    if row_off.dim() != 1 or row_off.numel() != 4 * B * L + 1:
        raise DaglError(f"{who}: row_off holds {row_off.numel()} offsets, expected 4*B*L+1 = {4 * B * L + 1}")
    head_off = row_off[:B * L + 1]              # (a head's view: the shape checks of graph_search, head by head)
    for h in range(4):
        if step:
            _need(b2p4[h], "b2p4[%d]" % h)
            map_hw = _value_map(who, b2p4[h])[1:]
            if tuple(map_hw) != (H, W) or b2p4[h].shape[0] != B:
                raise DaglError(f"{who}: b2p4[{h}] is the value map of {b2p4[h].shape[0]} {map_hw[0]}x{map_hw[1]} images, "
                                f"x holds {B} of {H}x{W}")
        Bh, _, _, E, flags, radius, k = _graph_refresh_operands(who, wq_rows4[h], x_rows4[h], head_off, key, radius,
                                                                tau4[h] if tau4 is not None else None, k, normalize, keep_all,
                                                                block_rows, (H, W))
        if Bh != B:
            raise DaglError(f"{who}: head {h}'s feature rows hold {Bh} images, expected {B}")
    if head_launches:
        flags |= _lib.GRAPH_STAGE_SEARCH_HEAD_LAUNCHES
    if want_graph:
        max_row_edges = _graph_refresh_longest(who, row_off, E, max_row_edges)
    elif max_row_edges is None:
        raise DaglError(f"{who}: want_graph=False needs max_row_edges, the input's largest degree"
                        + (" (reading it on the host is not available under stream capture)"
                           if torch.cuda.is_current_stream_capturing() else " (the call itself reads nothing on the host)"))
    max_row_edges = int(max_row_edges)
    dev = wq_rows4[0].device
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_graph_stage_search_workspace_bytes", B, H, W, E, radius, propagate, explore,
                                   0 if keep_all else k, 1 if want_graph else 0, 1 if step else 0)
    if want_graph:
        head, key_out, weight, score, cap = _graph_search_arrays(dev, 4 * B * L, E, radius, k, keep_all, propagate, explore)
        status = head[-2:]
    else:
        head = key_out = weight = score = None
        cap, status = 0, torch.empty(2, device=dev, dtype=torch.int64)
    table = lambda seq: (C.c_void_p * 4)(*[t.data_ptr() for t in seq])
    front = (_stream(), B, H, W, table(wq_rows4), table(x_rows4)) + ((table(b2p4),) if step else ())
    graph = (row_off.data_ptr(), _ptr(key, E > 0), E, max_row_edges, radius, table(tau4) if tau4 is not None else None, k, float(scale),
             flags)
    back = (_ptr(head), _ptr(key_out, cap > 0), _ptr(weight, cap > 0), _ptr(score, cap > 0), cap, status.data_ptr(), a, nbytes, propagate,
            explore, seed)
    out = None
    if step:
        out = torch.empty_like(x)
        check(lib.dagl_graph_stage_search_step(*front, *graph, x.data_ptr(), mix_w.data_ptr(), mix_b.data_ptr(), out.data_ptr(), *back), entry)
    else:
        check(lib.dagl_graph_stage_search(*front, *graph, *back), entry)
    del buf
    if not want_graph:
        return out, None, status
    return out, _graph_refresh_result(who, head, key_out, weight, score, max_row_edges, adjacent=bool(propagate)), status


@_on_device
def graph_stage_search(wq_rows4, x_rows4, row_off, key, hw, *, radius: int = 1, tau4=None, k: int = 0, scale: float = 10.0,
                       normalize: str = "reference", keep_all: bool = False, max_row_edges=None, workspace: "Workspace | None" = None,
                       block_rows: bool = False, propagate=False, explore: int = 0, seed: int = 0, head_launches: bool = False) -> dict:
    """``graph_search`` for the four heads of a ``CES`` stage in one row launch (``dagl_graph_stage_search``, csrc/graph_refresh.hip) ->
    dict: ONE CSR over the 4*B*L head-major rows.  wq_rows4 / x_rows4 / tau4, (row_off, key) as ``graph_stage_step``; ``hw`` the map
    (H, W).  Rows ``h*B*L .. (h+1)*B*L`` are, bit for bit, what ``graph_search`` returns for head h's operands, its slice of the input
    graph and the same ``propagate``, ``explore``, ``seed`` (offsets continuing from head to head): the random keys are hashed from the
    head-local row, so the four heads explore the same keys, and propagation never crosses an image, so never a head.  One host read;
    not under stream capture; the overlong-row refusal of ``graph_search``.  ``head_launches``: the row kernel once per head (for
    measurements; the same bits)."""
    wq0 = wq_rows4[0] if isinstance(wq_rows4, (list, tuple)) and len(wq_rows4) == 4 else None
    if not isinstance(wq0, torch.Tensor) or wq0.dim() != 3:
        raise DaglError("graph_stage_search: wq_rows4 must be a sequence of four [B,L,196] tensors, one per head")
    H, W = (int(v) for v in hw)
    return _graph_stage_search("graph_stage_search", "dagl_graph_stage_search", wq_rows4, x_rows4, None, row_off, key,
                               (wq0.shape[0], H, W), None, None, radius, tau4, k, scale, normalize, keep_all, max_row_edges, True, workspace,
                               block_rows, propagate, explore, seed, head_launches)[1]


@_on_device
def graph_stage_search_step(wq_rows4, x_rows4, b2p4, row_off, key, x, mix_w, mix_b, *, radius: int = 1, tau4=None, k: int = 0,
                            scale: float = 10.0, normalize: str = "reference", keep_all: bool = False, max_row_edges=None,
                            want_graph: bool = True, workspace: "Workspace | None" = None, block_rows: bool = False, propagate=False,
                            explore: int = 0, seed: int = 0, head_launches: bool = False):
    """``graph_search_step`` for the four heads of a ``CES`` stage and the stage's mix on the result (``dagl_graph_stage_search_step``,
    csrc/graph_refresh.hip) -> (out [B,64,H,W], dict | None, status): the arguments of ``graph_stage_step`` plus ``propagate``,
    ``explore`` and ``seed``.  ONE row launch covers the 4*B*L rows.  The dict is ``graph_stage_search``'s, bit for bit; ``out`` is
    ``ces_stage_fold_mix`` of the heads' aggregated rows, each ``graph_search_step``'s bits for its head -- the same with ``want_graph``
    True or False and on every call.  An empty graph with ``explore`` > 0 is populated; with ``explore`` = 0 it gives ``mix_b + x``.
    ``status``: device int64[2] (the overlong rows and their grid neighbours summed over the heads, the largest candidate count).

    Host reads, ``max_row_edges``, the overlong-row refusal and capture: as ``graph_search_step`` -- one host read with
    ``want_graph=True``; none with ``want_graph=False``, which needs ``max_row_edges`` and can be captured (``seed`` is a launch
    argument)."""
    if b2p4 is None:
        raise DaglError("graph_stage_search_step: b2p4 must be a sequence of four tensors, one per head")
    return _graph_stage_search("graph_stage_search_step", "dagl_graph_stage_search_step", wq_rows4, x_rows4, b2p4, row_off, key, x, mix_w,
                               mix_b, radius, tau4, k, scale, normalize, keep_all, max_row_edges, want_graph, workspace, block_rows,
                               propagate, explore, seed, head_launches)


@_on_device
def graph_attend_backward(d_weight, wq_rows, x_rows, row_off, key, score, weight, tau=None, scale: float = 10.0,
                          normalize: str = "reference", transposed=None, need_wq: bool = True, need_x: bool = True, need_tau: bool = True,
                          workspace: "Workspace | None" = None, hw=None):
    """Gradients of ``graph_attend`` (``dagl_graph_attend_backward``) -> (d_wq [B,L,196] | None, d_x [B,N,196] | None, d_tau [B*L] | None)
    from ``d_weight`` [E]; ``score`` / ``weight`` are the forward's outputs.  ``transposed`` = (col_off, src_row, perm), the graph's
    transposed CSR (``PatchGraph.transpose``): required with ``need_x``.  ``d_tau`` is None without ``tau``."""
    lib = _lib.load()
    B, H, W, E, flags = _graph_attend_operands("graph_attend_backward", wq_rows, x_rows, row_off, key, tau, normalize, hw)
    for n, t in (("d_weight", d_weight), ("score", score), ("weight", weight)):
        _need(t, n)
        if t.dim() != 1 or t.numel() != E:
            raise DaglError(f"graph_attend_backward: {n} must be 1-d with one entry per edge ({E})")
    col_off = src_row = perm = None
    if need_x:
        col_off, src_row, perm = _transposed_csr("graph_attend_backward", "d_x", transposed, B * H * W, E)
    buf, a, nbytes = _sized_region(workspace, wq_rows.device, "dagl_graph_attend_backward_workspace_bytes", B, H, W, E)
    d_wq = torch.empty_like(wq_rows) if need_wq else None
    d_x = torch.empty_like(x_rows) if need_x else None
    d_tau = torch.empty(B * wq_rows.shape[1], device=wq_rows.device, dtype=torch.float32) if need_tau and tau is not None else None
    check(lib.dagl_graph_attend_backward(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), row_off.data_ptr(), _ptr(key, E > 0), E,
                                         _ptr(tau), float(scale), flags, _ptr(score, E > 0), _ptr(weight, E > 0), _ptr(d_weight, E > 0),
                                         _ptr(col_off), _ptr(src_row, E > 0), _ptr(perm, E > 0), _ptr(d_wq), _ptr(d_x), _ptr(d_tau),
                                         a, nbytes), "dagl_graph_attend_backward")
    del buf
    return d_wq, d_x, d_tau


@_on_device
def ce_forward_generic(x, params: dict, ksize: int, stride_1: int, stride_2: int, inter_channels: int, mode: str = "adaptive",
                       k: int = 0, softmax_scale: float = 10.0, workspace: "Workspace | None" = None, want_degree: bool = False):
    """``CE.forward`` for ANY patch geometry (``dagl_ce_generic_forward``, csrc/generic.hip; dagl.py:175-176 makes ksize, stride_1,
    stride_2 and inter_channels constructor arguments): x [B,Cin,H,W] fp32 -> [B,inter_channels,H,W].  ``params`` = the block's
    state_dict tensors under their own names (fp32, on the device); Cin and inter_channels multiples of 4."""
    lib = _lib.load()
    _check_mode(mode)
    _need(x, "x")
    B, Cin, H, W = x.shape
    c, ks = int(inter_channels), int(ksize)
    P_, heads = ks * ks * c, mode != "topk"
    want = {"g.weight": (c, Cin, 3, 3), "g.bias": (c,), "theta.weight": (c, Cin, 1, 1), "theta.bias": (c,),
            "fc1.0.weight": (P_ // 4, P_), "fc1.0.bias": (P_ // 4,), "fc2.0.weight": (P_ // 4, P_), "fc2.0.bias": (P_ // 4,)}
    if heads:
        want.update({"thr_conv.weight": (1, Cin, ks, ks), "thr_conv.bias": (1,), "bias_conv.weight": (1, Cin, ks, ks), "bias_conv.bias": (1,)})
    for n, shp in want.items():
        _need(params[n], n)
        if tuple(params[n].shape) != shp:
            raise DaglError(f"ce_forward_generic: {n} is {tuple(params[n].shape)}, expected {shp}")
    need = lib.dagl_ce_generic_workspace_bytes(B, Cin, H, W, ks, int(stride_1), int(stride_2), c)
    if need == 0:
        raise DaglError(f"ce_forward_generic: unsupported shape / geometry B={B} Cin={Cin} H={H} W={W} ksize={ks} "
                        f"strides=({stride_1},{stride_2}) inter_channels={c}")
    buf, _, _ = _region(workspace, need, x.device)             # (the generic entry points take the buffer as it is)
    out = torch.empty(B, c, H, W, device=x.device, dtype=torch.float32)
    L = (-(-H // int(stride_1))) * (-(-W // int(stride_1)))
    deg = torch.empty(B, L, device=x.device, dtype=torch.int32) if want_degree else None
    check(lib.dagl_ce_generic_forward(_stream(), B, Cin, H, W, ks, int(stride_1), int(stride_2), c, float(softmax_scale), MODES[mode], int(k),
                                      x.data_ptr(), *(_ptr(params.get(n), n in want) for n in _lib.CeWeights.NAMES),
                                      out.data_ptr(), _ptr(deg), buf.data_ptr(), buf.numel()),
          "dagl_ce_generic_forward")
    return (out, deg) if want_degree else out


def generic_border(ksize: int) -> int:
    """Border of the zero-bordered NHWC maps of a generic patch geometry (``dagl_ce_generic_border``)."""
    return _lib.load().dagl_ce_generic_border(int(ksize))


def _generic_geom(H, W, ksize, stride_1, stride_2):
    pg = generic_border(ksize)
    L = (-(-H // int(stride_1))) * (-(-W // int(stride_1)))
    N = (-(-H // int(stride_2))) * (-(-W // int(stride_2)))
    return pg, L, N


@_on_device
def ce_generic_core_forward(wq_rows, x_rows, b2p, thr, bias, H: int, W: int, ksize: int, stride_1: int, stride_2: int, mode: str = "adaptive",
                            k: int = 0, softmax_scale: float = 10.0, workspace: "Workspace | None" = None, want_degree: bool = False):
    """dagl.py:250-272 from the feature rows for any patch geometry (``dagl_ce_generic_core_forward``): wq_rows [B,L,D], x_rows [B,N,D],
    b2p the zero-bordered NHWC value map [B,H+2pg,W+2pg,c] (pg = ``dagl_ce_generic_border(ksize)``), thr / bias [B,L] -> [B,c,H,W]."""
    lib = _lib.load()
    for n, t in (("wq_rows", wq_rows), ("x_rows", x_rows), ("b2p", b2p)):
        _need(t, n)
    B, c = b2p.shape[0], b2p.shape[3]
    pg, L, N = _generic_geom(H, W, ksize, stride_1, stride_2)
    D_ = ksize * ksize * c // 4
    if tuple(b2p.shape) != (B, H + 2 * pg, W + 2 * pg, c) or tuple(wq_rows.shape) != (B, L, D_) or tuple(x_rows.shape) != (B, N, D_):
        raise DaglError(f"ce_generic_core_forward: shapes {tuple(wq_rows.shape)}, {tuple(x_rows.shape)}, {tuple(b2p.shape)} do not fit "
                        f"L={L} N={N} D={D_} border={pg}")
    heads = mode != "topk"
    if heads:
        _need(thr, "thr"); _need(bias, "bias")
    need = lib.dagl_ce_generic_core_workspace_bytes(B, H, W, int(ksize), int(stride_1), int(stride_2), c, 0)
    buf, _, _ = _region(workspace, need, b2p.device)
    out = torch.empty(B, c, H, W, device=b2p.device, dtype=torch.float32)
    deg = torch.empty(B, L, device=b2p.device, dtype=torch.int32) if want_degree else None
    check(lib.dagl_ce_generic_core_forward(_stream(), B, H, W, int(ksize), int(stride_1), int(stride_2), c, float(softmax_scale), MODES[mode], int(k),
                                           wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), _ptr(thr, heads), _ptr(bias, heads),
                                           out.data_ptr(), _ptr(deg), buf.data_ptr(), buf.numel()), "dagl_ce_generic_core_forward")
    return (out, deg) if want_degree else out


@_on_device
def ce_generic_core_backward(d_out, wq_rows, x_rows, b2p, thr, bias, H: int, W: int, ksize: int, stride_1: int, stride_2: int,
                             mode: str = "adaptive", k: int = 0, softmax_scale: float = 10.0, workspace: "Workspace | None" = None):
    """Gradients of ``ce_generic_core_forward`` w.r.t. (wq_rows, x_rows, b2p, thr, bias) (``dagl_ce_generic_core_backward``)."""
    lib = _lib.load()
    _need(d_out, "d_out")
    B, c = b2p.shape[0], b2p.shape[3]
    heads = mode != "topk"
    need = lib.dagl_ce_generic_core_workspace_bytes(B, H, W, int(ksize), int(stride_1), int(stride_2), c, 1)
    buf, _, _ = _region(workspace, need, b2p.device)
    d_wq, d_x, d_b2p = torch.empty_like(wq_rows), torch.empty_like(x_rows), torch.empty_like(b2p)
    d_thr = torch.empty_like(thr) if heads else None
    d_bias = torch.empty_like(bias) if heads else None
    check(lib.dagl_ce_generic_core_backward(_stream(), B, H, W, int(ksize), int(stride_1), int(stride_2), c, float(softmax_scale), MODES[mode], int(k),
                                            wq_rows.data_ptr(), x_rows.data_ptr(), b2p.data_ptr(), _ptr(thr, heads), _ptr(bias, heads),
                                            d_out.data_ptr(), d_wq.data_ptr(), d_x.data_ptr(), d_b2p.data_ptr(), _ptr(d_thr), _ptr(d_bias),
                                            buf.data_ptr(), buf.numel()),
          "dagl_ce_generic_core_backward")
    return d_wq, d_x, d_b2p, d_thr, d_bias


@_on_device
def ce_prologue(x, g_w, g_b, theta_w, theta_b, thr_w=None, thr_b=None, bias_w=None, bias_b=None, fast=False):
    """The four prologue convolutions (dagl.py:208-215) -> (b1_nhwc, b2_nhwc, thr, bias); heads optional."""
    for n, t in (("x", x), ("g_w", g_w), ("g_b", g_b), ("theta_w", theta_w), ("theta_b", theta_b)):
        _need(t, n)
    B, c, H, W = x.shape
    if c != 64:
        raise DaglError("ce_prologue: 64 input channels expected")
    Lh, Lw = query_grid(H, W)
    b1p = torch.empty(B, H + 6, W + 6, 16, device=x.device, dtype=torch.float32)
    b2p = torch.empty_like(b1p)
    heads = thr_w is not None
    thr = torch.empty(B, Lh * Lw, device=x.device, dtype=torch.float32) if heads else None
    bias = torch.empty(B, Lh * Lw, device=x.device, dtype=torch.float32) if heads else None
    if heads:
        for n, t in (("thr_w", thr_w), ("thr_b", thr_b), ("bias_w", bias_w), ("bias_b", bias_b)):
            _need(t, n)
    if fast:
        # g / theta on the fp16 matrix cores with split operands (conv_pair16_kernel, the inference path's kernel, fp32 map out)
        lib = _lib.load()
        need = lib.dagl_ce_prologue16_scratch_bytes(B, H, W)
        scratch, base = _scratch(need, x.device)
        check(lib.dagl_ce_prologue16(_stream(), B, H, W, x.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), theta_w.data_ptr(), theta_b.data_ptr(),
                                     _ptr(thr_w), _ptr(thr_b), _ptr(bias_w), _ptr(bias_b), b1p.data_ptr(), b2p.data_ptr(), _ptr(thr),
                                     _ptr(bias), base, need),
              "dagl_ce_prologue16")
        return b1p, b2p, thr, bias
    scratch = torch.empty(8 * B * Lh * Lw, device=x.device, dtype=torch.float32) if heads else None
    check(_lib.load().dagl_ce_prologue(_stream(), B, H, W, x.data_ptr(), g_w.data_ptr(), g_b.data_ptr(),
                                       theta_w.data_ptr(), theta_b.data_ptr(), _ptr(thr_w), _ptr(thr_b), _ptr(bias_w), _ptr(bias_b),
                                       b1p.data_ptr(), b2p.data_ptr(), _ptr(thr), _ptr(bias), _ptr(scratch)), "dagl_ce_prologue")
    return b1p, b2p, thr, bias


def ce_prologue16_plan(heads: int, imgs: int, H: int, W: int) -> dict:
    """The launch plan of ``conv_pair16_kernel`` on ``heads`` x ``imgs`` images of [H, W] (``dagl_ce_prologue16_plan``, host only), by the
    function the launcher and the workspace carves plan with: ``strips`` of 64 columns, row ``chunks``, ``rows`` per block and ``slots``
    of |b1| maxima per head (4 waves x strips x chunks x imgs); the grid is (strips, chunks, heads * imgs)."""
    out = (C.c_int32 * 4)()
    check(_lib.load().dagl_ce_prologue16_plan(int(heads), int(imgs), int(H), int(W), out), "dagl_ce_prologue16_plan")
    return dict(zip(("strips", "chunks", "rows", "slots"), (int(v) for v in out)))


@_on_device
def ce_prologue16_debug(xs, g_w, g_b, theta_w, theta_b, tag: int = 1, range_init: int = 0, n_clear: int = 8, want_b1: bool = True,
                        coarse: bool = True) -> dict:
    """The inference flavour of the split-fp16 g / theta kernel with every output read out (``dagl_ce_prologue16_debug``, for tests).
    ``xs``, ``g_w`` ...: lists of one tensor per head (1..4), ``xs[h]`` [imgs,64,H,W].  Every buffer is poisoned before the call: NaN in
    the fp32 maps and the slots, 0x7e00 in the planes, 0xff in the scratch and the ``n_clear`` words, ``range_init`` in the range word.
    -> dict(b1, b2 [heads*imgs,H+6,W+6,16] fp32 (b1 None without ``want_b1``), hi, lo, hi2, lo2 (int16 bits; the coarse pair None without
    ``coarse``), amax [heads, slots], range (int32 [1]), clear (int32 [n_clear]))."""
    lib = _lib.load()
    heads = len(xs)
    if not (1 <= heads <= 4 and len(g_w) == len(g_b) == len(theta_w) == len(theta_b) == heads):
        raise DaglError("ce_prologue16_debug: 1..4 heads, one tensor of each kind per head")
    for h in range(heads):
        for n, t in (("x", xs[h]), ("g_w", g_w[h]), ("g_b", g_b[h]), ("theta_w", theta_w[h]), ("theta_b", theta_b[h])):
            _need(t, f"{n}[{h}]")
        if xs[h].shape != xs[0].shape or xs[h].dim() != 4 or xs[h].shape[1] != 64:
            raise DaglError("ce_prologue16_debug: every head's input is [imgs,64,H,W]")
    imgs, _, H, W = xs[0].shape
    dev = xs[0].device
    B = heads * imgs
    slots = ce_prologue16_plan(heads, imgs, H, W)["slots"]
    fmap = lambda: torch.full((B, H + 6, W + 6, 16), float("nan"), device=dev, dtype=torch.float32)
    plane = lambda: torch.full((B, H + 6, W + 6, 16), 0x7e00, device=dev, dtype=torch.int16)
    out = dict(b1=fmap() if want_b1 else None, b2=fmap(), hi=plane(), lo=plane(), hi2=plane() if coarse else None,
               lo2=plane() if coarse else None, amax=torch.full((heads, slots), float("nan"), device=dev, dtype=torch.float32),
               range=torch.full((1,), int(range_init), device=dev, dtype=torch.int32),
               clear=torch.full((max(int(n_clear), 1),), -1, device=dev, dtype=torch.int32)[:int(n_clear)])
    need = lib.dagl_ce_prologue16_debug_scratch_bytes(heads)
    scratch, base = _scratch(need, dev)
    scratch.fill_(0xff)
    table = lambda ts: (C.c_void_p * heads)(*[t.data_ptr() for t in ts])
    check(lib.dagl_ce_prologue16_debug(_stream(), heads, imgs, H, W, table(xs), table(g_w), table(g_b), table(theta_w), table(theta_b),
                                       int(tag), base, need, _ptr(out["b1"]), out["b2"].data_ptr(), out["hi"].data_ptr(),
                                       out["lo"].data_ptr(), _ptr(out["hi2"]), _ptr(out["lo2"]), out["amax"].data_ptr(),
                                       out["range"].data_ptr(), out["clear"].data_ptr() if n_clear else None, int(n_clear)),
          "dagl_ce_prologue16_debug")
    return out


PROJECT16_PLAN_FIELDS = ("key_items", "query_items", "lin", "units_q", "units_k", "n_full", "n_xcd", "n_split_groups", "n_proj", "cap",
                         "segs_k", "segs_q")
PROJECT16_FILL16 = 0x5A5A       # what ce_project16_debug leaves in the 16-bit halves the kernel does not store


def project16_plan(B: int, H: int, W: int, which: int = 3, cus: int = 0) -> dict:
    """The launch plan of ``project16_kernel`` on ``B`` images of [H, W] (``dagl_project16_plan``, host only), by the function the
    launcher plans with; ``which``: 1 keys, 2 queries, 3 both; ``cus`` <= 0: the current device's compute units (256 without one)."""
    out = (C.c_int32 * 12)()
    check(_lib.load().dagl_project16_plan(int(B), int(H), int(W), int(which), int(cus), out), "dagl_project16_plan")
    return dict(zip(PROJECT16_PLAN_FIELDS, (int(v) for v in out)))


@_on_device
def ce_project16_debug(map_hi, map_lo, H: int, W: int, heads: int = 1, which: int = 3, fc1_w=None, fc1_b=None, fc2_w=None, fc2_b=None,
                       map_hi2=None, map_lo2=None, amax=None, bf16: bool = False, q_tiled: bool = False, split: bool = False,
                       colsum: bool = False, rowsum: bool = False, policy=None, thr=None, tag: int = 1, range_init: int = 0,
                       scratch=None) -> dict:
    """The inference launch of the split-fp16 patch projection with every output read out (``dagl_ce_project16_debug``, for tests).
    ``map_hi`` / ``map_lo`` (and the optional coarse pair with ``amax`` [heads, slots]): int16 bits [heads*imgs, H+6, W+6, 16]; ``fc1_*``
    (queries) / ``fc2_*`` (keys): lists of one tensor per head, weights [196,784] in Linear order.  Switches: ``bf16`` copies (the query
    copy in fragment order with ``q_tiled``), ``split`` copies, ``colsum`` (with colpart), ``rowsum`` (``policy``: None = no policy word,
    else its value), ``thr`` = (xs, thr_w, bias_w) lists per head for the ride-along blocks.  Every buffer is poisoned before the call:
    NaN in the floats, ``PROJECT16_FILL16`` in the 16-bit copies, ``range_init`` in the range word.  ``scratch``: a uint8 buffer to reuse.
    -> dict of device tensors (None where not asked for): x, wq [B, rows, 204]; x_bf16, wq_bf16, x_hi, x_lo, wq_hi, wq_lo [B, rows_h, 216]
    int16 bits; colsum [B,204] fp64, colpart [B, 2 units_k, 224]; rowsum [B,N,8]; thr_part [heads,4,imgs,L,2]; range int32 [1]."""
    lib = _lib.load()
    _need(map_hi, "map_hi", torch.int16); _need(map_lo, "map_lo", torch.int16)
    B = map_hi.shape[0]
    if tuple(map_hi.shape) != (B, H + 6, W + 6, 16) or map_lo.shape != map_hi.shape or B % heads:
        raise DaglError("ce_project16_debug: planes are [heads*imgs, H+6, W+6, 16]")
    imgs, dev = B // heads, map_hi.device
    keys, queries = bool(which & 1), bool(which & 2)
    for side, w, b, on in (("fc2", fc2_w, fc2_b, keys), ("fc1", fc1_w, fc1_b, queries)):
        if on:
            if w is None or b is None or len(w) != heads or len(b) != heads:
                raise DaglError(f"ce_project16_debug: {side}: one weight and one bias per head")
            for h in range(heads):
                _need(w[h], f"{side}_w[{h}]"); _need(b[h], f"{side}_b[{h}]")
    for t, n in ((map_hi2, "map_hi2"), (map_lo2, "map_lo2")):
        if t is not None:
            _need(t, n, torch.int16)
    if amax is not None:
        _need(amax, "amax")
    N, (Lh, Lw) = H * W, query_grid(H, W)
    L = Lh * Lw
    rows = lambda n: lib.dagl_feat_rows(n)
    rows_h = lambda n: -(-n // 64) * 64 + 64
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=dev, dtype=dtype)
    half = lambda n, on: torch.full((B, rows_h(n), 216), PROJECT16_FILL16, device=dev, dtype=torch.int16) if on else None
    units_k = project16_plan(B, H, W, which)["units_k"]
    out = dict(x=nan(B, rows(N), DS) if keys else None, wq=nan(B, rows(L), DS) if queries else None,
               x_bf16=half(N, bf16 and keys), wq_bf16=half(L, bf16 and queries),
               x_hi=half(N, split and keys), x_lo=half(N, split and keys), wq_hi=half(L, split and queries), wq_lo=half(L, split and queries),
               colsum=nan(B, DS, dtype=torch.float64) if colsum else None, colpart=nan(B, 2 * units_k, 224) if colsum else None,
               rowsum=nan(B, N, 8) if rowsum else None, thr_part=None,
               range=torch.full((1,), int(range_init), device=dev, dtype=torch.int32))
    policy_word = torch.full((1,), int(policy), device=dev, dtype=torch.int32) if policy is not None else None
    table = lambda ts: (C.c_void_p * heads)(*[t.data_ptr() for t in ts]) if ts is not None else None
    thr_tables = (None, None, None)
    if thr is not None:
        for ts in thr:
            for h in range(heads):
                _need(ts[h], "thr operand")
        out["thr_part"] = nan(heads, 4, imgs, L, 2)
        thr_tables = tuple(table(ts) for ts in thr)
    need = lib.dagl_ce_project16_debug_scratch_bytes(heads)
    if scratch is None:
        scratch = torch.full((need + 256,), 0xFF, device=dev, dtype=torch.uint8)
    base = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    check(lib.dagl_ce_project16_debug(_stream(), heads, imgs, H, W, int(which), map_hi.data_ptr(), map_lo.data_ptr(), _ptr(map_hi2),
                                      _ptr(map_lo2), _ptr(amax), int(amax.shape[-1]) if amax is not None else 0,
                                      table(fc1_w if queries else None), table(fc1_b if queries else None),
                                      table(fc2_w if keys else None), table(fc2_b if keys else None), int(tag), out["range"].data_ptr(),
                                      base, scratch.numel() - (base - scratch.data_ptr()), _ptr(out["x"]), _ptr(out["wq"]),
                                      _ptr(out["x_bf16"]), _ptr(out["wq_bf16"]), int(q_tiled), _ptr(out["x_hi"]), _ptr(out["x_lo"]),
                                      _ptr(out["wq_hi"]), _ptr(out["wq_lo"]), _ptr(out["colsum"]), _ptr(out["colpart"]),
                                      _ptr(out["rowsum"]), _ptr(policy_word), *thr_tables, _ptr(out["thr_part"])),
          "dagl_ce_project16_debug")
    return out


@_on_device
def ce_forward_fused(x, params: dict, mode: str = "adaptive", k: int = 0, workspace: "Workspace | None" = None,
                     profile: "StageProfile | None" = None, exact_scan: bool = False, weights_packed: bool = False,
                     dense_hint: bool = False, want_info: bool = True, no_wait: bool = False, tight_topk: bool = False,
                     sampled_topk: bool = False, no_redo: bool = False):
    """Whole CE.forward (dagl.py:207-275) from the block input ``x`` [B,64,H,W]; ``params`` maps the block's
    state_dict names to contiguous fp32 GPU tensors.  Returns (out, info).  ``dense_hint``: go straight to the streamed
    dense formulation (adaptive mode; same result, see DAGL_FLAG_DENSE_HINT); with ``want_info=False`` that path does
    not read its edge statistics back (no host synchronisation) and info is None.  ``no_wait`` (adaptive mode behind the
    screen, DAGL_FLAG_NO_WAIT): the verdict stays on the device, an unserved call is NaN-filled and ``ce_range_check``
    reports it; info is None.  ``tight_topk`` (top-k modes, DAGL_FLAG_TIGHT_TOPK): candidate threshold from every second key tile and
    eight times the candidate slots -- for maps whose sampled threshold lets too many keys through (natural images); same result.
    ``sampled_topk`` (DAGL_FLAG_SAMPLED_TOPK) forces the sampled threshold; with neither the workspace's own policy word decides
    on the device (sticky switch to the tight threshold once a call overflowed; a cold workspace re-runs tight in the same call).
    ``no_redo`` (top-k modes, DAGL_FLAG_NO_REDO): the fp32 redo pass behind the refine kernel is not queued; a call that flagged a
    query group anyway is NaN-filled and ``ce_range_check`` reports it (bit 4, sticky)."""
    lib = _lib.load()
    _check_mode(mode)
    _need(x, "x")
    B, c, H, W = x.shape
    if c != 64:
        raise DaglError("ce_forward_fused: 64 input channels expected")
    ptrs = [_need(params[n], n).data_ptr() for n in _lib.CeWeights.NAMES]
    ws = workspace if workspace is not None else Workspace()
    mode_flags = MODES[mode] | (_lib.FLAG_EXACT_SCAN if exact_scan else 0)
    need = lib.dagl_ce_workspace_bytes(B, H, W, mode_flags, int(k))
    if need == 0:
        check(-1, "dagl_ce_workspace_bytes")
    held = ws.peek(x.device)
    if weights_packed and held is not None and held.numel() >= need + 256:
        mode_flags |= _lib.FLAG_WEIGHTS_PACKED           # same buffer as last time: the packed weights are still in it
    if dense_hint and mode == "adaptive" and not exact_scan:
        mode_flags |= _lib.FLAG_DENSE_HINT
        if held is not None:
            need = max(need, held.numel() - 4096)      # keep the (larger) buffer the dense path asked for earlier
    mode_flags |= _topk_flags(mode, exact_scan, tight_topk, sampled_topk)
    if no_redo and mode != "adaptive" and not exact_scan and (mode_flags & _lib.FLAG_WEIGHTS_PACKED):
        mode_flags |= _lib.FLAG_NO_REDO
    quiet = dense_hint and not want_info
    if no_wait and mode == "adaptive" and not exact_scan and not dense_hint and H * W >= 2048:
        mode_flags |= _lib.FLAG_NO_WAIT
        quiet = True
    out = torch.empty(B, 16, H, W, device=x.device, dtype=torch.float32)
    info = _lib.CeInfo()
    rc = 0
    for _attempt in range(3):
        buf, a, nbytes = _region(ws, need, x.device)
        rc = lib.dagl_ce_forward_fused(_stream(), B, H, W, x.data_ptr(), *ptrs, mode_flags, int(k), out.data_ptr(), a, nbytes,
                                       None if quiet else C.byref(info), profile._h if profile is not None else None)
        if rc == _lib.ERR_WORKSPACE and quiet:
            quiet = False                                # ask again, this time for the size
            continue
        if rc == _lib.ERR_WORKSPACE and info.required_bytes > need:
            need = int(info.required_bytes)
            mode_flags &= ~_lib.FLAG_WEIGHTS_PACKED      # the buffer is about to be replaced
            continue
        break
    check(rc, "dagl_ce_forward_fused")
    return out, None if quiet else _info_dict(info)


def ce_range_check(shape, mode: str, k: int, workspace: "Workspace", device) -> int:
    """True when a forward on ``workspace`` (input shape ``shape``) since the last check left the range of the split-fp16
    kernels and returned a NaN-filled output (``dagl_ce_range_check``; one host synchronisation; the word is sticky and
    cleared by the check that reports it).  ``shape[0]`` counts head x image pairs for a stage workspace."""
    lib = _lib.load()
    buf = workspace.peek(device)
    if buf is None:
        return False
    B, _, H, W = shape
    a, nbytes = _aligned(buf)
    out = C.c_int(0)
    with torch.cuda.device(device):
        check(lib.dagl_ce_range_check(_stream(), B, H, W, MODES[mode], int(k), a, nbytes, C.byref(out)), "dagl_ce_range_check")
    return int(out.value)            # bit 0: range, bit 1: an unserved no-wait adaptive call, bit 2: the last top-k call had a redo pass,
                                     # bit 3: the workspace's top-k threshold policy word says "tight", bit 4: a no-redo call went unserved


def ce_pivot_debug(shape, mode: str, k: int, workspace: "Workspace", device, sampled_topk: bool = True):
    """Test read-out (``dagl_ce_pivot_debug``): what the last top-k call on ``workspace`` (input shape ``shape``) that took its
    sampled threshold from pivot keys left there -> (pivot_idx [B, ceil(N/64), 2] int32, key_rowsum [B, N] fp32).  Raises
    ``DaglError`` (code ERR_UNSUPPORTED) for shapes / modes / k whose calls keep the tile sampling."""
    lib = _lib.load()
    buf = workspace.peek(device)
    if buf is None:
        raise DaglError("ce_pivot_debug: the workspace has served no call on this device")
    B, _, H, W = shape
    a, nbytes = _aligned(buf)
    idx = torch.empty(B, (H * W + 63) // 64, 2, device=device, dtype=torch.int32)
    rowsum = torch.empty(B, H * W, device=device, dtype=torch.float32)
    flags = MODES[mode] | (_lib.FLAG_SAMPLED_TOPK if sampled_topk and mode != "adaptive" else 0)
    with torch.cuda.device(device):
        check(lib.dagl_ce_pivot_debug(_stream(), B, H, W, flags, int(k), a, nbytes, idx.data_ptr(), rowsum.data_ptr()),
              "dagl_ce_pivot_debug")
    return idx, rowsum


def ce_wide_debug(shape, mode: str, k: int, workspace: "Workspace", device, exact_scan: bool = False):
    """Test read-out (``dagl_ce_wide_debug``): which query rows of the last row batch (L <= 2048: every row of the last image) the
    last wide top-k call on ``workspace`` (input shape ``shape``, same mode / k / ``exact_scan``) served from the one-block list kernel
    -> served [rows] int32, 1 = served, 0 = declined and left to the three-kernel form.  Raises ``DaglError`` (code ERR_UNSUPPORTED)
    for calls that run no list kernel (min(k, N) <= 64 or > 1024, the adaptive mode)."""
    lib = _lib.load()
    buf = workspace.peek(device)
    if buf is None:
        raise DaglError("ce_wide_debug: the workspace has served no call on this device")
    B, _, H, W = shape
    a, nbytes = _aligned(buf)
    Lh, Lw = query_grid(H, W)
    served = torch.full((Lh * Lw,), -1, device=device, dtype=torch.int32)       # (a batch holds at most L rows: the tail stays -1)
    flags = MODES[mode] | (_lib.FLAG_EXACT_SCAN if exact_scan else 0)
    with torch.cuda.device(device):
        check(lib.dagl_ce_wide_debug(_stream(), B, H, W, flags, int(k), a, nbytes, served.data_ptr()), "dagl_ce_wide_debug")
    return served[served >= 0]


@_on_device
def ces_stage_forward(x, head_params, mix_w, mix_b, mode: str = "adaptive", k: int = 0,
                      workspace: "Workspace | None" = None, profile: "StageProfile | None" = None,
                      weights_packed: bool = False, tight_topk: bool = False, sampled_topk: bool = False):
    """One CES stage in one launch set: ``conv1x1(cat(head_1(x)..head_4(x))) + x`` (dagl.py:114,116,118).
    ``head_params``: four dicts (state_dict names -> contiguous fp32 GPU tensors).  Returns (out [B,64,H,W], info), or
    (None, info) when a dense adaptive neighbourhood needs the per-head path.  The library reads the default head's weights
    (ksize 7, inter_channels 16) through raw pointers: every tensor's shape is checked here first."""
    _check_mode(mode)
    _need(x, "x"); _need(mix_w, "mix_w"); _need(mix_b, "mix_b")
    B, c, H, W = x.shape
    if c != 64 or len(head_params) != 4:
        raise DaglError("ces_stage_forward: x must be [B,64,H,W] and there must be four heads")
    if tuple(mix_w.shape) != (64, 64, 1, 1) or tuple(mix_b.shape) != (64,):
        raise DaglError(f"ces_stage_forward: mix_w is {tuple(mix_w.shape)}, mix_b {tuple(mix_b.shape)}; expected (64, 64, 1, 1) and (64,)")
    want = {"g.weight": (16, 64, 3, 3), "g.bias": (16,), "theta.weight": (16, 64, 1, 1), "theta.bias": (16,),
            "thr_conv.weight": (1, 64, 7, 7), "thr_conv.bias": (1,), "bias_conv.weight": (1, 64, 7, 7), "bias_conv.bias": (1,),
            "fc1.0.weight": (D, P), "fc1.0.bias": (D,), "fc2.0.weight": (D, P), "fc2.0.bias": (D,)}
    arr = (_lib.CeWeights * 4)()
    for h, prm in enumerate(head_params):
        for field, name in zip([f for f, _ in _lib.CeWeights._fields_], _lib.CeWeights.NAMES):
            if name not in prm:
                raise DaglError(f"ces_stage_forward: head {h} has no {name}")
            t = prm[name]
            _need(t, name)
            if tuple(t.shape) != want[name]:
                raise DaglError(f"ces_stage_forward: head {h} {name} is {tuple(t.shape)}, expected {want[name]}")
            setattr(arr[h], field, t.data_ptr())
    lib = _lib.load()
    out = torch.empty(B, 64, H, W, device=x.device, dtype=torch.float32)
    info = _lib.CeInfo()
    buf, a, nbytes = _sized_region(workspace, x.device, "dagl_ces_stage_workspace_bytes", B, H, W, MODES[mode], int(k))
    flags = MODES[mode] | (_lib.FLAG_WEIGHTS_PACKED if weights_packed else 0) | _topk_flags(mode, False, tight_topk, sampled_topk)
    rc = lib.dagl_ces_stage_forward(_stream(), B, H, W, x.data_ptr(), arr, mix_w.data_ptr(), mix_b.data_ptr(), flags, int(k),
                                    out.data_ptr(), a, nbytes, C.byref(info), profile._h if profile is not None else None)
    meta = _info_dict(info, drop=("range_fallback", "dense_rerun_blocks"))
    if rc == _lib.ERR_WORKSPACE and info.required_bytes == -1:
        return None, meta
    check(rc, "dagl_ces_stage_forward")
    return out, meta


@_on_device
def ce_core_forward(wq_rows, x_rows, b2, thr, bias, mode: str = "adaptive", k: int = 0,
                    workspace: "Workspace | None" = None, exact_scan: bool = False):
    """Graph core with the projections given (training path, include/dagl_ce.h ``dagl_ce_core_forward``):
    wq_rows [B,L,196], x_rows [B,N,196], b2 [B,16,H,W], thr/bias [B,L] -> (out [B,16,H,W], saved lists dict)."""
    lib = _lib.load()
    _check_mode(mode)
    for n, t in (("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2)):
        _need(t, n)
    B, c, H, W = b2.shape
    Lh, Lw = query_grid(H, W)
    L, N = Lh * Lw, H * W
    if c != 16 or tuple(wq_rows.shape) != (B, L, 196) or tuple(x_rows.shape) != (B, N, 196):
        raise DaglError("ce_core_forward: expected wq_rows [B,L,196], x_rows [B,H*W,196], b2 [B,16,H,W]")
    adaptive = mode != "topk"
    if adaptive:
        _need(thr, "thr"); _need(bias, "bias")
        if thr.numel() != B * L or bias.numel() != B * L:
            raise DaglError("ce_core_forward: thr/bias must hold B*L values")
    if mode != "adaptive":
        k = min(int(k), N)                 # top_k = min(num_edge, N): the lists are that wide
    mode_flags = MODES[mode] | (_lib.FLAG_EXACT_SCAN if exact_scan else 0)
    width = lib.dagl_ce_list_width(mode_flags, int(k))
    check(min(width, 0), "dagl_ce_list_width")
    dev = b2.device
    out = torch.empty(B, 16, H, W, device=dev, dtype=torch.float32)
    saved = dict(nb_idx=torch.zeros(B, L, width, device=dev, dtype=torch.int32),
                 nb_wgt=torch.zeros(B, L, width, device=dev, dtype=torch.float32),
                 nb_s=torch.zeros(B, L, width, device=dev, dtype=torch.float32),
                 nb_cnt=torch.zeros(B, L, device=dev, dtype=torch.int32),
                 mu=torch.zeros(B, L, device=dev, dtype=torch.float32) if adaptive else None)
    info = _lib.CeInfo()
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_ce_workspace_bytes", B, H, W, mode_flags, int(k))
    rc = lib.dagl_ce_core_forward(_stream(), B, H, W, wq_rows.data_ptr(), x_rows.data_ptr(), b2.data_ptr(),
                                  _ptr(thr, adaptive), _ptr(bias, adaptive), mode_flags, int(k), out.data_ptr(),
                                  saved["nb_idx"].data_ptr(), saved["nb_wgt"].data_ptr(), saved["nb_s"].data_ptr(),
                                  saved["nb_cnt"].data_ptr(), _ptr(saved["mu"]), a, nbytes, C.byref(info))
    check(rc, "dagl_ce_core_forward")
    saved["info"] = _info_dict(info, drop=("required_bytes",))
    return out, saved


@_on_device
def ce_core_backward(d_out, wq_rows, x_rows, b2, thr, bias, saved: dict, mode: str = "adaptive", k: int = 0,
                     workspace: "Workspace | None" = None):
    """Gradients of the graph core (``dagl_ce_core_backward``) -> (d_wq_rows, d_x_rows, d_b2, d_thr, d_bias)."""
    lib = _lib.load()
    for n, t in (("d_out", d_out), ("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2)):
        _need(t, n)
    B, _, H, W = b2.shape
    adaptive = mode != "topk"
    if mode != "adaptive":
        k = min(int(k), H * W)
    dev = b2.device
    d_wq = torch.empty_like(wq_rows)
    d_x = torch.empty_like(x_rows)
    d_b2 = torch.empty_like(b2)
    d_thr = torch.empty(B, wq_rows.shape[1], device=dev, dtype=torch.float32) if adaptive else None
    d_bias = torch.empty_like(d_thr) if adaptive else None
    buf, a, nbytes = _sized_region(workspace, dev, "dagl_ce_core_backward_workspace_bytes", B, H, W, MODES[mode], int(k))
    rc = lib.dagl_ce_core_backward(_stream(), B, H, W, MODES[mode], int(k), wq_rows.data_ptr(), x_rows.data_ptr(),
                                   b2.data_ptr(), _ptr(thr, adaptive), _ptr(bias, adaptive),
                                   saved["nb_idx"].data_ptr(), saved["nb_wgt"].data_ptr(), saved["nb_s"].data_ptr(),
                                   saved["nb_cnt"].data_ptr(), _ptr(saved["mu"]), d_out.data_ptr(), d_wq.data_ptr(),
                                   d_x.data_ptr(), d_b2.data_ptr(), _ptr(d_thr), _ptr(d_bias), a, nbytes)
    check(rc, "dagl_ce_core_backward")
    return d_wq, d_x, d_b2, d_thr, d_bias


@_on_device
def gemm_f32(A: torch.Tensor, B: torch.Tensor, a_k_contiguous: bool = True, b_k_contiguous: bool = False, out=None,
             alpha: float = 1.0, beta: float = 0.0, bias=None, relu: bool = False, chunk_tiles: int = 0,
             split_k: bool = True) -> torch.Tensor:
    """Batched fp32 matrix product on the matrix cores (``dagl_gemm_f32``).  A: [b,M,K] (a_k_contiguous) or [b,K,M];
    B: [b,N,K] (b_k_contiguous) or [b,K,N]; 2-D operands = batch of one.  Returns C [b,M,N] (= alpha A B + beta out)."""
    _need(A, "A"); _need(B, "B")
    squeeze = A.dim() == 2
    if squeeze:
        A, B = A[None], B[None]
    nb = A.shape[0]
    M, K = (A.shape[1], A.shape[2]) if a_k_contiguous else (A.shape[2], A.shape[1])
    N, K2 = (B.shape[1], B.shape[2]) if b_k_contiguous else (B.shape[2], B.shape[1])
    if K != K2 or B.shape[0] != nb:
        raise DaglError("gemm_f32: shape mismatch")
    if out is None:
        if beta != 0.0:
            raise DaglError("gemm_f32: beta needs an existing output")
        out = torch.empty(nb, M, N, device=A.device, dtype=torch.float32)
    else:
        _need(out, "out")
    if bias is not None:
        _need(bias, "bias")
    lib = _lib.load()
    scratch = None
    if split_k and nb == 1:
        nf = lib.dagl_gemm_f32_scratch_floats(nb, M, N, K)
        if nf:
            scratch = torch.empty(nf, device=A.device, dtype=torch.float32)
    check(lib.dagl_gemm_f32(_stream(), nb, M, N, K, A.data_ptr(), A.shape[2], A.shape[1] * A.shape[2],
                            int(a_k_contiguous), B.data_ptr(), B.shape[2], B.shape[1] * B.shape[2],
                            int(b_k_contiguous), out.data_ptr(), N, M * N, float(alpha), float(beta),
                            _ptr(bias), int(relu), int(chunk_tiles), _ptr(scratch)), "dagl_gemm_f32")
    return out[0] if squeeze and out.dim() == 3 else out


@_on_device
def ce_core_dense_forward(wq_rows, x_rows, b2, thr, bias, workspace: "Workspace | None" = None, want_info: bool = True,
                          exact: bool = False):
    """Graph core in the dense regime under autograd (``dagl_ce_core_dense_forward``): same operands as
    ``ce_core_forward`` (adaptive mode) -> (out [B,16,H,W], saved dict(lse [B,L,2], mu [B,L], info)).  ``exact``: the
    chunked fp32 GEMM form whatever the size (modules with ``scan="exact"``: no split-fp16 range limit)."""
    lib = _lib.load()
    for n, t in (("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2), ("thr", thr), ("bias", bias)):
        _need(t, n)
    B, c, H, W = b2.shape
    Lh, Lw = query_grid(H, W)
    L, N = Lh * Lw, H * W
    if c != 16 or tuple(wq_rows.shape) != (B, L, 196) or tuple(x_rows.shape) != (B, N, 196) or thr.numel() != B * L \
            or bias.numel() != B * L:
        raise DaglError("ce_core_dense_forward: expected wq_rows [B,L,196], x_rows [B,H*W,196], b2 [B,16,H,W], thr/bias [B,L]")
    need = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256
    dev = b2.device
    out = torch.empty(B, 16, H, W, device=dev, dtype=torch.float32)
    lse = torch.empty(B, L, 2, device=dev, dtype=torch.float32)
    mu = torch.empty(B, L, device=dev, dtype=torch.float32)
    info = _lib.CeInfo()
    buf, a, nbytes = _region(workspace, need, dev)
    check(lib.dagl_ce_core_dense_forward(_stream(), B, H, W, _lib.FLAG_EXACT_SCAN if exact else 0, wq_rows.data_ptr(),
                                         x_rows.data_ptr(), b2.data_ptr(), thr.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                         lse.data_ptr(), mu.data_ptr(), a, nbytes, C.byref(info) if want_info else None),
          "dagl_ce_core_dense_forward")
    meta = _info_dict(info, drop=("required_bytes",), path=5, redone_queries=-1) if want_info else None
    return out, dict(lse=lse, mu=mu, info=meta)


@_on_device
def ce_core_dense_backward(d_out, wq_rows, x_rows, b2, thr, bias, saved: dict, workspace: "Workspace | None" = None,
                           exact: bool = False):
    """Gradients of the dense graph core (``dagl_ce_core_dense_backward``) -> (d_wq_rows, d_x_rows, d_b2, d_thr, d_bias).
    ``exact``: the five matrix products on the fp32 matrix cores instead of the fp16 ones with split operands."""
    exact = exact or DENSE_BACKWARD_FP32
    lib = _lib.load()
    for n, t in (("d_out", d_out), ("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2), ("thr", thr), ("bias", bias)):
        _need(t, n)
    B, _, H, W = b2.shape
    need = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 1)
    dev = b2.device
    d_wq, d_x, d_b2 = torch.empty_like(wq_rows), torch.empty_like(x_rows), torch.empty_like(b2)
    d_thr = torch.empty(B, wq_rows.shape[1], device=dev, dtype=torch.float32)
    d_bias = torch.empty_like(d_thr)
    buf, a, nbytes = _region(workspace, need, dev)
    check(lib.dagl_ce_core_dense_backward(_stream(), B, H, W, _lib.FLAG_EXACT_SCAN if exact else 0, wq_rows.data_ptr(), x_rows.data_ptr(), b2.data_ptr(),
                                          thr.data_ptr(), bias.data_ptr(), saved["lse"].data_ptr(), saved["mu"].data_ptr(),
                                          d_out.data_ptr(), d_wq.data_ptr(), d_x.data_ptr(), d_b2.data_ptr(),
                                          d_thr.data_ptr(), d_bias.data_ptr(), a, nbytes), "dagl_ce_core_dense_backward")
    return d_wq, d_x, d_b2, d_thr, d_bias


DENSE_PLAN_FIELDS = ("Lc", "n_chunks", "Bc", "kslices", "nk", "h16")


def dense_plan(B: int, H: int, W: int, backward: bool = True) -> dict:
    """The launch plan of the dense / wide core ops at [B,H,W] under the chunk budget in force (``dagl_ce_core_dense_plan``, host
    only): queries per chunk ``Lc``, chunks per image ``n_chunks``, images per group ``Bc``, split-K factor of d Wq ``kslices``,
    K extent of the key-major operand copies ``nk``, ``h16`` = 1 where the backward's products may run on the fp16 matrix cores."""
    out = (C.c_int32 * 6)()
    check(_lib.load().dagl_ce_core_dense_plan(int(B), int(H), int(W), int(bool(backward)), out), "dagl_ce_core_dense_plan")
    return dict(zip(DENSE_PLAN_FIELDS, (int(v) for v in out)))


@contextlib.contextmanager
def dense_chunk_budget(floats: int):
    """Run the body with the dense core's chunk budget set to ``floats`` per [chunk, N] matrix (``dagl_ce_core_dense_chunk_floats``;
    0 = the built-in 128 Mi) and put the previous value back afterwards, also when the body raises.  A testing and tuning hook: the
    budget is process-wide, and a workspace sized under one budget is refused under a larger one (``ERR_WORKSPACE``)."""
    lib = _lib.load()
    before = lib.dagl_ce_core_dense_chunk_floats(int(floats))
    try:
        yield before
    finally:
        lib.dagl_ce_core_dense_chunk_floats(before)


@_on_device
def ce_core_wide_forward(wq_rows, x_rows, b2, thr, bias, mode: str, k: int, workspace: "Workspace | None" = None,
                         want_info: bool = False):
    """Graph core of the top-k modes whose neighbourhoods exceed the lists (min(k, N) > MAX_TOPK) under autograd
    (``dagl_ce_core_wide_forward``): the dense formulation with the row-wise selection of the k best scores as its mask
    (GReccR2b_3mh_1-checkpoint.py:242-250; CA_model-checkpoint.py:134-143 takes 500) -> (out [B,16,H,W], info | None).
    ``thr`` / ``bias`` are None in mode "topk"."""
    lib = _lib.load()
    if mode not in ("topk", "adaptive_topk"):
        raise DaglError(f"ce_core_wide_forward: mode {mode!r}: expected 'topk' or 'adaptive_topk'")
    for n, t in (("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2)) + ((("thr", thr), ("bias", bias)) if mode != "topk" else ()):
        _need(t, n)
    B, c, H, W = b2.shape
    Lh, Lw = query_grid(H, W)
    L, N = Lh * Lw, H * W
    if c != 16 or tuple(wq_rows.shape) != (B, L, 196) or tuple(x_rows.shape) != (B, N, 196):
        raise DaglError("ce_core_wide_forward: expected wq_rows [B,L,196], x_rows [B,H*W,196], b2 [B,16,H,W]")
    need = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256
    out = torch.empty(B, 16, H, W, device=b2.device, dtype=torch.float32)
    info = _lib.CeInfo()
    buf, a, nbytes = _region(workspace, need, b2.device)
    heads = mode != "topk"
    check(lib.dagl_ce_core_wide_forward(_stream(), B, H, W, MODES[mode], int(k), wq_rows.data_ptr(), x_rows.data_ptr(), b2.data_ptr(),
                                        _ptr(thr, heads), _ptr(bias, heads), out.data_ptr(),
                                        a, nbytes, C.byref(info) if want_info else None), "dagl_ce_core_wide_forward")
    return out, _info_dict(info, drop=("required_bytes", "dense_rerun_blocks"), path=5, redone_queries=-1,
                           range_fallback=0) if want_info else None


@_on_device
def ce_core_wide_backward(d_out, wq_rows, x_rows, b2, thr, bias, mode: str, k: int, workspace: "Workspace | None" = None):
    """Gradients of ``ce_core_wide_forward`` (``dagl_ce_core_wide_backward``) -> (d_wq_rows, d_x_rows, d_b2, d_thr, d_bias);
    the last two are None in mode "topk" (a 0/1 mask has no threshold heads)."""
    lib = _lib.load()
    heads = mode != "topk"
    for n, t in (("d_out", d_out), ("wq_rows", wq_rows), ("x_rows", x_rows), ("b2", b2)) + \
            ((("thr", thr), ("bias", bias)) if heads else ()):
        _need(t, n)
    B, _, H, W = b2.shape
    need = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 1)
    dev = b2.device
    d_wq, d_x, d_b2 = torch.empty_like(wq_rows), torch.empty_like(x_rows), torch.empty_like(b2)
    d_thr = torch.empty(B, wq_rows.shape[1], device=dev, dtype=torch.float32) if heads else None
    d_bias = torch.empty_like(d_thr) if heads else None
    buf, a, nbytes = _region(workspace, need, dev)
    check(lib.dagl_ce_core_wide_backward(_stream(), B, H, W, MODES[mode], int(k), wq_rows.data_ptr(), x_rows.data_ptr(), b2.data_ptr(),
                                         _ptr(thr, heads), _ptr(bias, heads), d_out.data_ptr(), d_wq.data_ptr(), d_x.data_ptr(),
                                         d_b2.data_ptr(), _ptr(d_thr), _ptr(d_bias), a, nbytes), "dagl_ce_core_wide_backward")
    return d_wq, d_x, d_b2, d_thr, d_bias


# ---- stages of the differentiable convolutions and projections (include/dagl_ce.h: train_ops.hip, gemm16s.hip, conv_grad.hip) ------
# The library checks the patch geometry against the map's extents; what it cannot see -- how much memory stands behind a pointer --
# is checked here.
def _map_geom(t: torch.Tensor, name: str, channels: "int | None" = None):
    _need(t, name)
    if t.dim() != 4 or channels not in (None, t.shape[3]):
        raise DaglError(f"{name}: a channels-last map [B,Hp,Wp,{channels or 'C'}] expected, got {tuple(t.shape)}")
    return tuple(t.shape)


@_on_device
def unfold_patches(pmap, k: int, stride: int, oy: int, ox: int, oh: int, ow: int) -> torch.Tensor:
    """rows[(b,py,px), (kh,kw,c)] = pmap[b, oy + py*stride + kh, ox + px*stride + kw, c] -> [B*oh*ow, k*k*C]."""
    B, Hp, Wp, c = _map_geom(pmap, "pmap")
    rows = torch.empty(B * oh * ow, k * k * c, device=pmap.device, dtype=torch.float32)
    check(_lib.load().dagl_unfold_patches(_stream(), B, Hp, Wp, c, k, stride, oy, ox, oh, ow, pmap.data_ptr(), rows.data_ptr()),
          "dagl_unfold_patches")
    return rows


@_on_device
def fold_patches(d_rows, map_shape, k: int, stride: int, oy: int, ox: int, oh: int, ow: int) -> torch.Tensor:
    """The adjoint of ``unfold_patches``: d_rows [B*oh*ow, k*k*C] -> d_map of ``map_shape`` = (B,Hp,Wp,C), every pixel written."""
    _need(d_rows, "d_rows")
    B, Hp, Wp, c = map_shape
    if d_rows.numel() != B * oh * ow * k * k * c:
        raise DaglError(f"fold_patches: d_rows {tuple(d_rows.shape)} does not hold {B * oh * ow} patches of {k}x{k}x{c}")
    d_map = torch.empty(B, Hp, Wp, c, device=d_rows.device, dtype=torch.float32)
    check(_lib.load().dagl_fold_patches(_stream(), B, Hp, Wp, c, k, stride, oy, ox, oh, ow, d_rows.data_ptr(), d_map.data_ptr()),
          "dagl_fold_patches")
    return d_map


@_on_device
def copy4(src, sizes, s_strides, dst, d_strides) -> None:
    """dst[i . d_strides] = src[i . s_strides] for every index i of the 4-D box ``sizes`` (strides in elements from each tensor's
    first element; the library takes them as they come, so the far corner of the box is checked here)."""
    for t, strides, name in ((src, s_strides, "src"), (dst, d_strides, "dst")):
        _need(t, name)
        if min(sizes) < 1 or min(strides) < 0 or sum((n - 1) * st for n, st in zip(sizes, strides)) >= t.numel():
            raise DaglError(f"copy4: box {tuple(sizes)} with strides {tuple(strides)} leaves {name} ({t.numel()} elements)")
    check(_lib.load().dagl_copy4(_stream(), *sizes, src.data_ptr(), *s_strides, dst.data_ptr(), *d_strides), "dagl_copy4")


@_on_device
def relu_backward(y, dz) -> torch.Tensor:
    """dz * (y > 0)."""
    _need(y, "y"); _need(dz, "dz")
    if y.numel() != dz.numel():
        raise DaglError("relu_backward: y and dz differ in size")
    out = torch.empty_like(dz)
    check(_lib.load().dagl_relu_backward(_stream(), dz.numel(), y.data_ptr(), dz.data_ptr(), out.data_ptr()), "dagl_relu_backward")
    return out


@_on_device
def col_sum(x) -> torch.Tensor:
    """Column sums of x [rows, cols] -> [cols] (fixed summation order)."""
    _need(x, "x")
    rows, cols = x.shape
    lib = _lib.load()
    out = torch.empty(cols, device=x.device, dtype=torch.float32)
    scratch = torch.empty(lib.dagl_col_sum_scratch_bytes(rows, cols), device=x.device, dtype=torch.uint8)
    check(lib.dagl_col_sum(_stream(), rows, cols, x.data_ptr(), out.data_ptr(), scratch.data_ptr()), "dagl_col_sum")
    return out


@_on_device
def project_patches16(pmap, weight, bias, H: int, W: int, queries: bool) -> torch.Tensor:
    """relu(Linear(patch)) of every 7x7x16 patch of the zero-bordered map [B,H+6,W+6,16] on the split-fp16 matrix cores (the forward
    of the differentiable path; weight [196,784] in (kh,kw,c) order) -> [B*rows, 196], rows = L (``queries``) or H*W."""
    B, Hp, Wp, _ = _map_geom(pmap, "pmap", 16)
    _need(weight, "weight"); _need(bias, "bias")
    if (Hp, Wp) != (H + 6, W + 6) or tuple(weight.shape) != (D, P) or bias.numel() != D:
        raise DaglError("project_patches16: expected pmap [B,H+6,W+6,16], weight [196,784], bias [196]")
    lib = _lib.load()
    Lh, Lw = query_grid(H, W)
    need = lib.dagl_project_patches16_scratch_bytes(B, H, W, int(queries))
    scratch, base = _scratch(need, pmap.device)
    y = torch.empty(B * (Lh * Lw if queries else H * W), D, device=pmap.device, dtype=torch.float32)
    check(lib.dagl_project_patches16(_stream(), B, H, W, int(queries), pmap.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                     base, need), "dagl_project_patches16")
    return y


def fc_grad16_fold_ok(stride: int, ow: int) -> bool:
    """Whether ``fc_grad16(fold=True)`` serves the grid (``dagl_fc_grad16_dmap_ok``)."""
    return bool(_lib.load().dagl_fc_grad16_dmap_ok(stride, ow))


FC_GRAD16_PLAN_FIELDS = ("n", "n_pad", "slices", "k_slice", "im_rps", "w_tile", "w_impl", "rows_tile", "n_loop", "fold_seg", "fold_rows",
                         "merged_split")


def fc_grad16_plan(B: int, Hp: int, Wp: int, geometry, want_w: bool = True, want_rows: bool = False, want_map: bool = False) -> dict:
    """The launch plan of one ``dagl_fc_grad16`` / ``dagl_fc_grad16_dmap`` call (``dagl_fc_grad16_plan``, host only), by the functions the
    call itself plans with.  ``geometry`` = (stride, oy, ox, oh, ow); ``want_*``: the outputs asked for (d_rows or d_map, not both).
    For d W: ``n`` patches, ``n_pad``, K ``slices`` of ``k_slice`` patches, ``im_rps`` image rows per slice where it reads shifted planes
    of the map (0: transposed patch rows), ``w_tile`` = 256 / 128 tile rows of its kernel (0: no d W), ``w_impl`` = 1 where that kernel
    is the instantiation that reads shifted planes.  For d rows / d map: ``rows_tile`` (0: neither), ``n_loop`` column tiles per block,
    ``fold_seg`` patches per folded row segment and ``fold_rows`` segments per 128-patch tile.  ``merged_split`` = 1 where one pass over
    d z writes both of its split copies."""
    stride, oy, ox, oh, ow = (int(v) for v in geometry)
    out = (C.c_int32 * 12)()
    check(_lib.load().dagl_fc_grad16_plan(int(B), int(Hp), int(Wp), stride, oy, ox, oh, ow, int(bool(want_w)), int(bool(want_rows)),
                                          int(bool(want_map)), out), "dagl_fc_grad16_plan")
    return dict(zip(FC_GRAD16_PLAN_FIELDS, (int(v) for v in out)))


@_on_device
def fc_grad16(pmap, weight, y, dz, geometry, need_w: bool = True, need_b: bool = True, need_map: bool = True, fold: bool = False):
    """The gradient products of a 7x7x16 -> 196 patch projection on the split-fp16 matrix cores (``dagl_fc_grad16``; ``fold``:
    ``dagl_fc_grad16_dmap``) -> (d_w [196,784], d_b [196], d_rows [n,784] or, with ``fold``, d_map like ``pmap``), None where not
    needed.  ``geometry`` = (stride, oy, ox, oh, ow); dz [n,196], n = B*oh*ow; ``y``: the layer's output (ReLU backward) or None."""
    B, Hp, Wp, _ = _map_geom(pmap, "pmap", 16)
    _need(weight, "weight"); _need(dz, "dz")
    if y is not None:
        _need(y, "y")
    stride, oy, ox, oh, ow = geometry
    n = B * oh * ow
    if tuple(weight.shape) != (D, P) or dz.numel() != n * D or (y is not None and y.numel() != n * D) or (fold and not need_map):
        raise DaglError(f"fc_grad16: expected weight [196,784], dz / y [{n},196]; fold=True computes the gradient of the map")
    lib = _lib.load()
    dev = pmap.device
    d_w = torch.empty(D, P, device=dev, dtype=torch.float32) if need_w else None
    d_b = torch.empty(D, device=dev, dtype=torch.float32) if need_b else None
    name = "dagl_fc_grad16_dmap" if fold else "dagl_fc_grad16"
    need = getattr(lib, name + "_scratch_bytes")(B, oh, ow)
    scratch, base = _scratch(need, dev)
    d_out = (torch.empty_like(pmap) if fold else torch.empty(n, P, device=dev, dtype=torch.float32)) if need_map else None
    check(getattr(lib, name)(_stream(), B, Hp, Wp, stride, oy, ox, oh, ow, pmap.data_ptr(), weight.data_ptr(), _ptr(y), dz.data_ptr(),
                             _ptr(d_w), _ptr(d_b), _ptr(d_out), base, need), name)
    return d_w, d_b, d_out


def conv_pair_backward_supported(B: int, H: int, W: int) -> bool:
    return bool(_lib.load().dagl_conv_pair_backward_supported(B, H, W))


def conv_pair_backward_plan(B: int, H: int, W: int) -> dict:
    """The strips of one ``dagl_conv_pair_backward`` call (``dagl_conv_pair_backward_plan``, host only), by the function the launcher
    and the scratch size plan with: ``rows_w`` rows per block and ``strips_w`` strips per image of the parameter gradients' launch,
    ``rows_x`` / ``strips_x`` of the input gradient's."""
    out = (C.c_int32 * 4)()
    check(_lib.load().dagl_conv_pair_backward_plan(int(B), int(H), int(W), out), "dagl_conv_pair_backward_plan")
    return dict(zip(("rows_w", "strips_w", "rows_x", "strips_x"), (int(v) for v in out)))


@_on_device
def conv_pair_backward(x, d_b1p, d_b2p, g_w, th_w, need_x: bool = True, need_params: bool = True):
    """Backward of g (3x3) and theta (1x1), 64 -> 16, on the maps themselves (``dagl_conv_pair_backward``): x [B,64,H,W] and the
    gradients of the two zero-bordered NHWC maps [B,H+6,W+6,16] -> (d_x, d_g_w, d_g_b, d_th_w, d_th_b), None where not needed."""
    for n, t in (("x", x), ("d_b1p", d_b1p), ("d_b2p", d_b2p), ("g_w", g_w), ("th_w", th_w)):
        _need(t, n)
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if tuple(x.shape) != (B, 64, H, W) or tuple(d_b1p.shape) != (B, H + 6, W + 6, 16) or d_b2p.shape != d_b1p.shape \
            or tuple(g_w.shape) != (16, 64, 3, 3) or th_w.numel() != 16 * 64:
        raise DaglError("conv_pair_backward: expected x [B,64,H,W], d_b1p / d_b2p [B,H+6,W+6,16], g_w [16,64,3,3], th_w [16,64,1,1]")
    lib = _lib.load()
    dev = x.device
    d_x = torch.empty_like(x) if need_x else None
    d_gw = d_gb = d_tw = d_tb = scratch = None
    if need_params:
        d_gw, d_gb = torch.empty_like(g_w), torch.empty(16, device=dev, dtype=torch.float32)
        d_tw, d_tb = torch.empty_like(th_w), torch.empty(16, device=dev, dtype=torch.float32)
        scratch = torch.empty(max(16, lib.dagl_conv_pair_backward_scratch_bytes(B, H, W)), device=dev, dtype=torch.uint8)
    check(lib.dagl_conv_pair_backward(_stream(), B, H, W, x.data_ptr(), d_b1p.data_ptr(), d_b2p.data_ptr(), g_w.data_ptr(), th_w.data_ptr(),
                                      _ptr(d_x), _ptr(d_gw), _ptr(d_gb), _ptr(d_tw), _ptr(d_tb), _ptr(scratch)), "dagl_conv_pair_backward")
    return d_x, d_gw, d_gb, d_tw, d_tb


@_on_device
def prelu_forward(x, weight) -> torch.Tensor:
    """Single-parameter PReLU, x > 0 ? x : weight * x (a multiple of 4 elements, 16-byte aligned: the kernels move float4s)."""
    _need(x, "x"); _need(weight, "weight")
    if weight.numel() != 1:
        raise DaglError("prelu_forward: one shared slope expected")
    y = torch.empty_like(x)
    check(_lib.load().dagl_prelu_forward(_stream(), x.numel(), x.data_ptr(), weight.data_ptr(), y.data_ptr()), "dagl_prelu_forward")
    return y


@_on_device
def prelu_backward(x, dy, weight):
    """(dx, d weight) of ``prelu_forward``; d weight by a fixed-order fp64 reduction."""
    _need(x, "x"); _need(dy, "dy"); _need(weight, "weight")
    if weight.numel() != 1 or dy.numel() != x.numel():
        raise DaglError("prelu_backward: one shared slope and a dy of x's size expected")
    lib = _lib.load()
    dx = torch.empty_like(x)
    da = torch.empty_like(weight)
    scratch = torch.empty(max(8, lib.dagl_prelu_scratch_bytes(x.numel())), device=x.device, dtype=torch.uint8)
    check(lib.dagl_prelu_backward(_stream(), x.numel(), x.data_ptr(), dy.data_ptr(), weight.data_ptr(), dx.data_ptr(), da.data_ptr(),
                                  scratch.data_ptr()), "dagl_prelu_backward")
    return dx, da


# ---- the residual trunk's convolutions (include/dagl_ce.h: dagl_trunk_*) -------------------------------------------------------
def _trunk_geom(t: torch.Tensor, name: str):
    _need(t, name)
    if t.dim() != 4:
        raise DaglError(f"{name}: [B,C,H,W] expected, got {tuple(t.shape)}")
    return tuple(t.shape)


@_on_device
def trunk_pack_weights(w: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """conv weight [Cout,Cin,k,k] -> the fragment layout of the trunk kernels (``transposed``: the input gradient's)."""
    Cout, Cin, kh, kw = _trunk_geom(w, "weight")
    if kh != kw:
        raise DaglError("trunk_pack_weights: square kernels only")
    lib = _lib.load()
    n = lib.dagl_trunk_packed_floats(Cin, Cout, kh, int(transposed))
    if n == 0:
        raise DaglError(f"trunk_pack_weights: unsupported layer {Cin}->{Cout} {kh}x{kw}")
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    check(lib.dagl_trunk_pack_weights(_stream(), Cin, Cout, kh, int(transposed), w.data_ptr(), out.data_ptr()), "dagl_trunk_pack_weights")
    return out


@_on_device
def trunk_conv_forward(x: torch.Tensor, packed: torch.Tensor, bias, Cout: int, ksize: int, slope=None, want_pre: bool = False,
                       res_scale: float = 1.0, residual=None):
    """conv(x) (+ bias) [-> PReLU(slope)] [-> * res_scale + residual] -> (out [B,Cout,H,W], pre-activation or None)."""
    B, Cin, H, W = _trunk_geom(x, "x")
    _need(packed, "packed")
    if bias is not None:
        _need(bias, "bias")
    if slope is not None:
        _need(slope, "slope")
    if residual is not None and _trunk_geom(residual, "residual") != (B, Cout, H, W):
        raise DaglError("trunk_conv_forward: residual shape mismatch")
    if want_pre and slope is None:
        raise DaglError("trunk_conv_forward: the pre-activation needs the PReLU slope")
    out = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
    pre = torch.empty_like(out) if want_pre else None
    check(_lib.load().dagl_trunk_conv_forward(_stream(), B, Cin, Cout, H, W, ksize, x.data_ptr(), packed.data_ptr(), _ptr(bias),
                                              _ptr(slope), _ptr(pre), float(res_scale), _ptr(residual), out.data_ptr()),
          "dagl_trunk_conv_forward")
    return out, pre


@_on_device
def trunk_conv_input_grad(d_out: torch.Tensor, packed_t: torch.Tensor, Cin: int, ksize: int, alpha: float = 1.0, slope=None,
                          pre=None, skip=None):
    """alpha * conv_transposed(d_out) [-> PReLU backward from ``pre``] [+ skip] -> (d_in [B,Cin,H,W], slope partials or None)."""
    B, Cout, H, W = _trunk_geom(d_out, "d_out")
    _need(packed_t, "packed_t")
    lib = _lib.load()
    part = None
    if slope is not None:
        _need(slope, "slope")
        if pre is None or _trunk_geom(pre, "pre") != (B, Cin, H, W):
            raise DaglError("trunk_conv_input_grad: the PReLU backward needs the pre-activation [B,Cin,H,W]")
        part = torch.empty(lib.dagl_trunk_input_grad_blocks(B, H, W), device=d_out.device, dtype=torch.float64)
    if skip is not None and _trunk_geom(skip, "skip") != (B, Cin, H, W):
        raise DaglError("trunk_conv_input_grad: skip gradient shape mismatch")
    d_in = torch.empty(B, Cin, H, W, device=d_out.device, dtype=torch.float32)
    check(lib.dagl_trunk_conv_input_grad(_stream(), B, Cin, Cout, H, W, ksize, d_out.data_ptr(), packed_t.data_ptr(), float(alpha),
                                         _ptr(slope), _ptr(pre), _ptr(part), _ptr(skip), d_in.data_ptr()), "dagl_trunk_conv_input_grad")
    return d_in, part


@_on_device
def trunk_conv_weight_grad(x: torch.Tensor, d_out: torch.Tensor, ksize: int, alpha: float = 1.0, want_bias: bool = True,
                           slope_part=None):
    """(d weight [Cout,Cin,k,k], d bias [Cout] or None, d slope [1] or None) of a trunk convolution; ``slope_part``: the partials
    of an earlier ``trunk_conv_input_grad`` to add up into the PReLU slope's gradient."""
    B, Cin, H, W = _trunk_geom(x, "x")
    Bo, Cout, Ho, Wo = _trunk_geom(d_out, "d_out")
    if (Bo, Ho, Wo) != (B, H, W):
        raise DaglError("trunk_conv_weight_grad: x and d_out do not match")
    lib = _lib.load()
    d_w = torch.empty(Cout, Cin, ksize, ksize, device=x.device, dtype=torch.float32)
    d_b = torch.empty(Cout, device=x.device, dtype=torch.float32) if want_bias else None
    d_s = None
    if slope_part is not None:
        _need(slope_part, "slope_part", torch.float64)
        d_s = torch.empty(1, device=x.device, dtype=torch.float32)
    need = lib.dagl_trunk_weight_grad_scratch_bytes(B, Cin, Cout, H, W, ksize)
    if need == 0:
        raise DaglError(f"trunk_conv_weight_grad: unsupported layer {Cin}->{Cout} {ksize}x{ksize}")
    scratch = torch.empty(need // 4, device=x.device, dtype=torch.float32)
    check(lib.dagl_trunk_conv_weight_grad(_stream(), B, Cin, Cout, H, W, ksize, x.data_ptr(), d_out.data_ptr(), float(alpha),
                                          d_w.data_ptr(), _ptr(d_b), _ptr(slope_part), slope_part.numel() if slope_part is not None else 0,
                                          _ptr(d_s), scratch.data_ptr(), need), "dagl_trunk_conv_weight_grad")
    return d_w, d_b, d_s
