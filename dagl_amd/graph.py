"""``PatchGraph`` -- the patch graph a ``CE`` block learns, as CSR over its query rows.

What ``CE.graph`` returns (``dagl_ce_graph_count`` / ``dagl_ce_graph_fill``, csrc/graph.hip): for every image and query patch the
keys with ``mask_b != 0`` and their weights ``A = softmax(10 S m) * mask_b`` -- the non-zeros of ``yi``, dagl.py:256-261.  The
container itself is plain tensor bookkeeping and works on CPU tensors.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import MODES, DaglError

DENSE_LIMIT = 1 << 26          # largest [L, N] ``to_dense`` builds (256 MiB of fp32)


class PatchGraph:
    """CSR over the ``B * L`` query rows (row ``b * L + i`` = query patch ``i`` of image ``b``):

    ``row_off`` [B*L+1] int64 row offsets; ``key`` [E] int32 key patch index, ``0 .. N-1`` row-major over ``H x W``, strictly
    ascending inside a row; ``weight`` [E] fp32 ``A[i, j]``; ``score`` [E] fp32 ``S[i, j]`` or None.  ``mode`` / ``k`` say how the
    keys were selected (``k`` = 0 in mode "adaptive")."""

    def __init__(self, row_off: torch.Tensor, key: torch.Tensor, weight: torch.Tensor, score: Optional[torch.Tensor],
                 B: int, H: int, W: int, mode: str = "adaptive", k: int = 0):
        B, H, W, k = int(B), int(H), int(W), int(k)
        if B < 1 or H < 1 or W < 1:
            raise DaglError(f"PatchGraph: bad shape B={B} H={H} W={W}")
        if mode not in MODES:
            raise DaglError(f"PatchGraph: unknown mode {mode!r}")
        L, N = (-(-H // 4)) * (-(-W // 4)), H * W
        arrays = [("row_off", row_off, torch.int64), ("key", key, torch.int32), ("weight", weight, torch.float32)]
        if score is not None:
            arrays.append(("score", score, torch.float32))
        for name, t, dtype in arrays:
            if not isinstance(t, torch.Tensor) or t.dim() != 1:
                raise DaglError(f"PatchGraph: {name} must be a 1-d tensor")
            if t.dtype != dtype:
                raise DaglError(f"PatchGraph: {name} has dtype {t.dtype}, expected {dtype}")
            if t.device != row_off.device:
                raise DaglError(f"PatchGraph: {name} lives on {t.device}, row_off on {row_off.device}")
        if row_off.numel() != B * L + 1:
            raise DaglError(f"PatchGraph: row_off holds {row_off.numel()} offsets, expected B*L+1 = {B * L + 1}")
        E = key.numel()
        if any(t.numel() != E for _, t, _ in arrays[2:]):
            raise DaglError("PatchGraph: key, weight and score must have one entry per edge")
        # (one host read of three words when the arrays live on the device)
        first, last, steps_ok = (int(v) for v in torch.stack([row_off[0], row_off[-1], (row_off[1:] >= row_off[:-1]).all().long()]).tolist())
        if first != 0 or not steps_ok:
            raise DaglError("PatchGraph: row_off must start at 0 and never decrease")
        if last != E:
            raise DaglError(f"PatchGraph: row_off ends at {last}, the arrays hold {E} edges")
        self.row_off, self.key, self.weight, self.score = row_off, key, weight, score
        self.B, self.L, self.N, self.H, self.W, self.mode, self.k = B, L, N, H, W, mode, k

    @property
    def n_edges(self) -> int:
        return self.key.numel()

    def degrees(self) -> torch.Tensor:
        """[B, L] int64: keys per query."""
        return (self.row_off[1:] - self.row_off[:-1]).view(self.B, self.L)

    def _row_index(self, b: int, i: int) -> int:
        if not (0 <= b < self.B and 0 <= i < self.L):
            raise IndexError(f"PatchGraph: row ({b}, {i}) outside [0, {self.B}) x [0, {self.L})")
        return b * self.L + i

    def row(self, b: int, i: int):
        """(key, weight, score | None) of query ``i`` of image ``b``: views into the arrays."""
        r = self._row_index(int(b), int(i))
        lo, hi = (int(v) for v in self.row_off[r:r + 2].tolist())
        return self.key[lo:hi], self.weight[lo:hi], (self.score[lo:hi] if self.score is not None else None)

    def to_dense(self, b: int) -> torch.Tensor:
        """[L, N] fp32: image ``b``'s ``A`` with zeros off the graph.  For tests and small maps: raises beyond 2^26 entries."""
        if self.L * self.N > DENSE_LIMIT:
            raise DaglError(f"PatchGraph.to_dense: [{self.L}, {self.N}] exceeds {DENSE_LIMIT} entries; walk the rows instead")
        r0 = self._row_index(int(b), 0)
        off = self.row_off[r0:r0 + self.L + 1]
        lo, hi = int(off[0]), int(off[-1])
        rows = torch.repeat_interleave(torch.arange(self.L, device=off.device), off[1:] - off[:-1])
        out = torch.zeros(self.L, self.N, dtype=torch.float32, device=off.device)
        out[rows, self.key[lo:hi].long()] = self.weight[lo:hi]
        return out

    def cpu(self) -> "PatchGraph":
        return PatchGraph(self.row_off.cpu(), self.key.cpu(), self.weight.cpu(), self.score.cpu() if self.score is not None else None,
                          self.B, self.H, self.W, self.mode, self.k)

    def __repr__(self):
        return (f"PatchGraph(B={self.B}, L={self.L}, N={self.N}, edges={self.n_edges}, mode={self.mode!r}, k={self.k}, "
                f"score={'yes' if self.score is not None else 'no'}, device={self.row_off.device})")
