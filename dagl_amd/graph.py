"""``PatchGraph`` -- the patch graph a ``CE`` block learns, as CSR over its query rows -- and ``FixedGraph``, the same graph as a fixed
number of slots per row: the form whose size is known before a step runs, so that a step can hand back its graph under stream capture.

What ``CE.graph`` returns (``dagl_ce_graph_count`` / ``dagl_ce_graph_fill``, csrc/graph.hip): for every image and query patch the
keys with ``mask_b != 0`` and their weights ``A = softmax(10 S m) * mask_b`` -- the non-zeros of ``yi``, dagl.py:256-261.  The
container itself is plain tensor bookkeeping and works on CPU tensors.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import MODES, DaglError

DENSE_LIMIT = 1 << 26          # largest [L, N] ``to_dense`` builds (256 MiB of fp32)


def trivial_graph(B: int, H: int, W: int, device, mode: str = "adaptive", ksize: int = 7, stride: int = 4) -> "PatchGraph":
    """The start of a graph search (``CE.build_graph``, ``SequenceState.start``): one edge per query, the key at the query patch's own
    position (the patch origin of ``synth.query_grid`` + 3, clamped to the map), weight 0, no score; valid, largest degree 1.  Works
    on the CPU."""
    from .synth import same_pad_amounts
    B, H, W = int(B), int(H), int(W)
    if B < 1 or H < 1 or W < 1:
        raise DaglError(f"trivial_graph: bad shape B={B} H={H} W={W}")
    Lh, Lw = -(-H // stride), -(-W // stride)
    pt, _bo = same_pad_amounts(H, ksize, stride)
    pl, _r = same_pad_amounts(W, ksize, stride)
    qy = (torch.arange(Lh, device=device) * 4 - pt + 3).clamp_(0, H - 1)
    qx = (torch.arange(Lw, device=device) * 4 - pl + 3).clamp_(0, W - 1)
    key = (qy.view(-1, 1) * W + qx.view(1, -1)).reshape(-1).repeat(B).to(torch.int32)
    g = PatchGraph(torch.arange(B * Lh * Lw + 1, device=device, dtype=torch.int64), key, torch.zeros(key.numel(), device=device),
                   None, B, H, W, mode if mode in MODES else "adaptive", 0)
    g._valid, g._max_degree = True, 1
    return g


class PatchGraph:
    """CSR over the ``B * L`` query rows (row ``b * L + i`` = query patch ``i`` of image ``b``):

    ``row_off`` [B*L+1] int64 row offsets; ``key`` [E] int32 key patch index, ``0 .. N-1`` row-major over ``H x W``, strictly
    ascending inside a row; ``weight`` [E] fp32 ``A[i, j]``; ``score`` [E] fp32 ``S[i, j]`` or None.  ``mode`` / ``k`` say how the
    keys were selected (``k`` = 0 in mode "adaptive").

    ``CE.apply_graph`` runs a block on such a graph, and the graph may be edited first (``select``, ``with_weight``) or built by hand:
    there keys may come in any order and repeat (repeats add up) and weights are any floats; ``validate`` checks the key range,
    ``transpose`` gives the column-major view the backward walks, ``to`` moves the arrays."""

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
        self._valid = False              # ``validate`` has found every key in [0, N)
        self._transposed = None          # ``transpose``'s (col_off, src_row, perm)
        self._max_degree = None          # ``max_degree``'s value

    @property
    def n_edges(self) -> int:
        return self.key.numel()

    def degrees(self) -> torch.Tensor:
        """[B, L] int64: keys per query."""
        return (self.row_off[1:] - self.row_off[:-1]).view(self.B, self.L)

    def max_degree(self) -> int:
        """The largest number of keys a query holds.  One reduction and one host read; the value is kept (``with_weight`` and ``to`` hand
        it on -- they keep the offsets --, ``select`` does not)."""
        if self._max_degree is None:
            self._max_degree = int((self.row_off[1:] - self.row_off[:-1]).max()) if self.n_edges else 0
        return self._max_degree

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

    # ---- editing (``CE.apply_graph`` takes the result): keys may then come in any order and repeat, weights are any floats ----------
    def _like(self, row_off, key, weight, score) -> "PatchGraph":
        """A graph of this one's shape over arrays that are already known to be consistent (no host read)."""
        g = object.__new__(PatchGraph)
        g.row_off, g.key, g.weight, g.score = row_off, key, weight, score
        g.B, g.L, g.N, g.H, g.W, g.mode, g.k = self.B, self.L, self.N, self.H, self.W, self.mode, self.k
        g._valid, g._transposed, g._max_degree = self._valid, None, None
        return g

    def rows(self) -> torch.Tensor:
        """[E] int64: the query row ``b * L + i`` of every edge."""
        n = self.B * self.L
        return torch.repeat_interleave(torch.arange(n, device=self.row_off.device), self.row_off[1:] - self.row_off[:-1],
                                       output_size=self.n_edges)

    def to(self, device) -> "PatchGraph":
        """The same graph with its arrays on ``device`` (what ``validate`` and ``transpose`` have found goes along)."""
        device = torch.device(device)
        g = self._like(self.row_off.to(device), self.key.to(device), self.weight.to(device),
                       self.score.to(device) if self.score is not None else None)
        if self._transposed is not None:
            g._transposed = tuple(t.to(device) for t in self._transposed)
        g._max_degree = self._max_degree
        return g

    @staticmethod
    def cat(graphs) -> "PatchGraph":
        """The graphs of ``graphs`` one after the other along the image axis (``B`` adds up, offsets rebased): what a ``CES`` stage keeps
        of its four heads -- head-major, row ``(h * B + b) * L + i`` = query ``i`` of image ``b`` under head ``h``.  They must share H, W,
        the device and whether ``score`` is present; ``mode`` / ``k`` come from the first; the result is valid when every input is, its
        largest degree is known when every input's is.  No host read."""
        graphs = list(graphs)
        if not graphs or not all(isinstance(g, PatchGraph) for g in graphs):
            raise DaglError("PatchGraph.cat: a non-empty sequence of PatchGraphs expected")
        first = graphs[0]
        for g in graphs[1:]:
            if (g.H, g.W) != (first.H, first.W):
                raise DaglError(f"PatchGraph.cat: maps of {first.H}x{first.W} and {g.H}x{g.W}")
            if g.row_off.device != first.row_off.device:
                raise DaglError(f"PatchGraph.cat: graphs on {first.row_off.device} and {g.row_off.device}")
            if (g.score is None) != (first.score is None):
                raise DaglError("PatchGraph.cat: score must be present in every graph or in none")
        parts, base = [first.row_off], first.row_off[-1:]
        for g in graphs[1:]:
            parts.append(g.row_off[1:] + base)
            base = base + g.row_off[-1:]
        out = first._like(torch.cat(parts), torch.cat([g.key for g in graphs]), torch.cat([g.weight for g in graphs]),
                          torch.cat([g.score for g in graphs]) if first.score is not None else None)
        out.B = sum(g.B for g in graphs)
        out._valid = all(g._valid for g in graphs)
        if all(g._max_degree is not None for g in graphs):
            out._max_degree = max(g._max_degree for g in graphs)
        return out

    def images(self, lo: int, hi: int) -> "PatchGraph":
        """The sub-graph of images ``lo .. hi - 1``: ``key`` / ``weight`` / ``score`` are views, the offsets are rebased on the device.
        Sizing the views takes the two bounding offsets: ONE host read of two words when the arrays live on the device (none on the CPU,
        and none for ``images(0, B)``).  Validity is handed on; the largest degree is not (it may be smaller)."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.B:
            raise DaglError(f"PatchGraph.images: [{lo}, {hi}) is not a non-empty range of the {self.B} images")
        r0, r1 = lo * self.L, hi * self.L
        if (lo, hi) == (0, self.B):
            e0, e1 = 0, self.n_edges
        else:
            e0, e1 = (int(v) for v in self.row_off[[r0, r1]].tolist())          # the one host read
        off = self.row_off[r0:r1 + 1]
        g = self._like(off - off[:1] if lo else off, self.key[e0:e1], self.weight[e0:e1],
                       self.score[e0:e1] if self.score is not None else None)
        g.B = hi - lo
        return g

    def with_weight(self, weight: torch.Tensor) -> "PatchGraph":
        """The same structure (the offsets and keys are shared, not copied) with ``weight`` [E] fp32 in the place of the weights.  A
        ``weight`` that requires grad is kept as it is: ``CE.apply_graph`` under autograd returns its gradient."""
        if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or weight.numel() != self.n_edges:
            raise DaglError(f"PatchGraph.with_weight: a 1-d tensor of {self.n_edges} weights expected")
        if weight.dtype != torch.float32:
            raise DaglError(f"PatchGraph.with_weight: weight has dtype {weight.dtype}, expected {torch.float32}")
        if weight.device != self.row_off.device:
            raise DaglError(f"PatchGraph.with_weight: weight lives on {weight.device}, the graph on {self.row_off.device}")
        g = self._like(self.row_off, self.key, weight, self.score)
        g._transposed, g._max_degree = self._transposed, self._max_degree
        return g

    def select(self, mask: torch.Tensor) -> "PatchGraph":
        """The edges with ``mask`` [E] bool set, in their order, as a new CSR with recomputed offsets."""
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 1 or mask.numel() != self.n_edges:
            raise DaglError(f"PatchGraph.select: a 1-d bool mask over the {self.n_edges} edges expected")
        if mask.device != self.row_off.device:
            raise DaglError(f"PatchGraph.select: mask lives on {mask.device}, the graph on {self.row_off.device}")
        deg = torch.zeros(self.B * self.L, dtype=torch.int64, device=mask.device).index_add_(0, self.rows(), mask.long())
        row_off = torch.cat([deg.new_zeros(1), deg.cumsum(0)])
        return self._like(row_off, self.key[mask], self.weight[mask], self.score[mask] if self.score is not None else None)

    def validate(self) -> "PatchGraph":
        """Every key must lie in [0, N): raises ``DaglError`` naming the first edge whose key does not.  One reduction and one host read;
        the verdict is kept (``with_weight`` / ``select`` / ``to`` hand it on: they add no keys)."""
        if self._valid:
            return self
        if self.n_edges:
            bad = (self.key < 0) | (self.key >= self.N)
            first = int(torch.where(bad.any(), bad.int().argmax(), bad.new_full((), -1, dtype=torch.int64)))      # the one host read
            if first >= 0:
                row = int(torch.searchsorted(self.row_off, torch.tensor(first, device=self.row_off.device), right=True)) - 1
                raise DaglError(f"PatchGraph.validate: edge {first} (query {row % self.L} of image {row // self.L}) has key "
                                f"{int(self.key[first])}, outside [0, {self.N})")
        self._valid = True
        return self

    def transpose(self):
        """The transposed CSR ``CE.apply_graph``'s backward walks: (col_off [B*N+1] int64, src_row [E] int32, perm [E] int32) -- the edges
        in a stable order of their column ``b * N + key``: transposed edge ``t`` is edge ``perm[t]`` of this graph and belongs to query
        row ``src_row[t]``; column ``c`` owns ``col_off[c] .. col_off[c+1]``.  Needs valid keys (``validate``); kept on the object."""
        if self._transposed is None:
            self.validate()
            if self.n_edges >= 1 << 31:
                raise DaglError(f"PatchGraph.transpose: {self.n_edges} edges do not fit 32-bit edge ids")
            rows = self.rows()
            col = torch.div(rows, self.L, rounding_mode="floor") * self.N + self.key.long()
            col, perm = torch.sort(col, stable=True)
            col_off = torch.searchsorted(col, torch.arange(self.B * self.N + 1, device=col.device))
            self._transposed = (col_off.contiguous(), rows[perm].int().contiguous(), perm.int().contiguous())
        return self._transposed

    def to_fixed(self, width: Optional[int] = None) -> "FixedGraph":
        """This graph as ``width`` slots per row (``FixedGraph``): row r's edges, verbatim and in their order (repeats, ``-1`` and ``N``
        included), in slots ``0 .. deg - 1``, then ``(-1, 0, 0)``.  ``width=None``: ``max_degree()``, at least 1.  A row longer than
        ``width`` is refused.  A gather, no boolean-mask indexing: no host read beyond ``max_degree()``.  A graph without scores gives
        zero scores."""
        longest = self.max_degree()
        width = max(longest, 1) if width is None else int(width)
        if width < 1:
            raise DaglError(f"PatchGraph.to_fixed: width={width} < 1")
        if longest > width:
            raise DaglError(f"PatchGraph.to_fixed: a row holds {longest} edges, more than width = {width} (rows are never truncated)")
        dev = self.row_off.device
        deg = self.row_off[1:] - self.row_off[:-1]
        slot = torch.arange(width, device=dev)
        live = slot[None, :] < deg[:, None]
        at = (self.row_off[:-1, None] + slot[None, :]).clamp_(0, max(self.n_edges - 1, 0))

        def rows_of(values, filler):
            if self.n_edges == 0:
                return torch.full((deg.numel(), width), filler, dtype=values.dtype, device=dev)
            return torch.where(live, values[at], torch.full((), filler, dtype=values.dtype, device=dev))

        score = self.score if self.score is not None else torch.zeros_like(self.weight)
        return FixedGraph(rows_of(self.key, -1), rows_of(self.weight, 0.0), rows_of(score, 0.0), deg.to(torch.int32), self.B, self.H,
                          self.W, self.mode, self.k)

    def __repr__(self):
        return (f"PatchGraph(B={self.B}, L={self.L}, N={self.N}, edges={self.n_edges}, mode={self.mode!r}, k={self.k}, "
                f"score={'yes' if self.score is not None else 'no'}, device={self.row_off.device})")


class FixedGraph:
    """A patch graph as ``width`` slots per query row (``rows = B * L``, row ``b * L + i`` = query ``i`` of image ``b``; ``B`` counts
    head-major images for a ``CES`` stage, as in ``PatchGraph.cat``):

    ``key`` [rows, width] int32, ``weight`` / ``score`` [rows, width] fp32, ``deg`` [rows] int32.  Row r holds its edges in slots
    ``0 .. deg[r] - 1`` -- in ascending key order when a step produced it -- and ``key = -1, weight = 0, score = 0`` from ``deg[r]`` on:
    every byte is defined, two graphs compare with ``torch.equal``.  ``mode`` / ``k`` as on ``PatchGraph``.

    Every array has a size known without looking at the graph, so ``CE.step_graph`` / ``refresh_graph`` on a ``FixedGraph`` read nothing
    on the host and run under stream capture WITH their graph output; ``copy_`` moves a new graph into a captured one's storage.
    ``PatchGraph.to_fixed`` / ``to_csr`` convert (plain torch, off the hot path); the routes that walk edges (``apply_graph``,
    ``attend_graph``, ``forward_on_graph``) take the CSR."""

    def __init__(self, key: torch.Tensor, weight: torch.Tensor, score: torch.Tensor, deg: torch.Tensor, B: int, H: int, W: int,
                 mode: str = "adaptive", k: int = 0):
        B, H, W, k = int(B), int(H), int(W), int(k)
        if B < 1 or H < 1 or W < 1:
            raise DaglError(f"FixedGraph: bad shape B={B} H={H} W={W}")
        if mode not in MODES:
            raise DaglError(f"FixedGraph: unknown mode {mode!r}")
        L, N = (-(-H // 4)) * (-(-W // 4)), H * W
        for name, t, dtype, dim in (("key", key, torch.int32, 2), ("weight", weight, torch.float32, 2), ("score", score, torch.float32, 2),
                                    ("deg", deg, torch.int32, 1)):
            if not isinstance(t, torch.Tensor) or t.dim() != dim:
                raise DaglError(f"FixedGraph: {name} must be a {dim}-d tensor")
            if t.dtype != dtype:
                raise DaglError(f"FixedGraph: {name} has dtype {t.dtype}, expected {dtype}")
            if t.device != key.device:
                raise DaglError(f"FixedGraph: {name} lives on {t.device}, key on {key.device}")
            if not t.is_contiguous():
                raise DaglError(f"FixedGraph: {name} must be contiguous")
        if key.shape[0] != B * L or key.shape[1] < 1:
            raise DaglError(f"FixedGraph: key is {tuple(key.shape)}, expected [B*L = {B * L}, width >= 1]")
        if weight.shape != key.shape or score.shape != key.shape or deg.numel() != B * L:
            raise DaglError("FixedGraph: weight and score must have key's shape, deg one entry per row")
        self.key, self.weight, self.score, self.deg = key, weight, score, deg
        self.B, self.L, self.N, self.H, self.W, self.mode, self.k = B, L, N, H, W, mode, k

    @property
    def width(self) -> int:
        return self.key.shape[1]

    @property
    def device(self):
        return self.key.device

    def _like(self, key, weight, score, deg, B=None) -> "FixedGraph":
        g = object.__new__(FixedGraph)
        g.key, g.weight, g.score, g.deg = key, weight, score, deg
        g.B, g.L, g.N, g.H, g.W, g.mode, g.k = (self.B if B is None else B), self.L, self.N, self.H, self.W, self.mode, self.k
        return g

    def n_edges(self) -> int:
        """The edges the graph holds (``deg`` clamped to [0, width]): one reduction and one host read."""
        return int(self.deg.clamp(0, self.width).sum())

    def degrees(self) -> torch.Tensor:
        """[B, L] int64: keys per query."""
        return self.deg.clamp(0, self.width).long().view(self.B, self.L)

    def row(self, b: int, i: int):
        """(key, weight, score) of query ``i`` of image ``b``: views of the row's first ``deg`` slots (one host read of the degree)."""
        b, i = int(b), int(i)
        if not (0 <= b < self.B and 0 <= i < self.L):
            raise IndexError(f"FixedGraph: row ({b}, {i}) outside [0, {self.B}) x [0, {self.L})")
        r = b * self.L + i
        d = min(max(int(self.deg[r]), 0), self.width)
        return self.key[r, :d], self.weight[r, :d], self.score[r, :d]

    def to(self, device) -> "FixedGraph":
        device = torch.device(device)
        return self._like(self.key.to(device), self.weight.to(device), self.score.to(device), self.deg.to(device))

    def cpu(self) -> "FixedGraph":
        return self.to("cpu")

    def images(self, lo: int, hi: int) -> "FixedGraph":
        """The sub-graph of images ``lo .. hi - 1``: row views of the four arrays.  Never reads on the host."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.B:
            raise DaglError(f"FixedGraph.images: [{lo}, {hi}) is not a non-empty range of the {self.B} images")
        r0, r1 = lo * self.L, hi * self.L
        return self._like(self.key[r0:r1], self.weight[r0:r1], self.score[r0:r1], self.deg[r0:r1], B=hi - lo)

    @staticmethod
    def cat(graphs) -> "FixedGraph":
        """The graphs one after the other along the image axis (``B`` adds up): what a ``CES`` stage keeps of its four heads,
        head-major.  They must share ``width``, H, W and the device; ``mode`` / ``k`` come from the first.  No host read."""
        graphs = list(graphs)
        if not graphs or not all(isinstance(g, FixedGraph) for g in graphs):
            raise DaglError("FixedGraph.cat: a non-empty sequence of FixedGraphs expected")
        first = graphs[0]
        for g in graphs[1:]:
            if (g.H, g.W) != (first.H, first.W):
                raise DaglError(f"FixedGraph.cat: maps of {first.H}x{first.W} and {g.H}x{g.W}")
            if g.width != first.width:
                raise DaglError(f"FixedGraph.cat: widths {first.width} and {g.width}")
            if g.device != first.device:
                raise DaglError(f"FixedGraph.cat: graphs on {first.device} and {g.device}")
        return first._like(torch.cat([g.key for g in graphs]), torch.cat([g.weight for g in graphs]),
                           torch.cat([g.score for g in graphs]), torch.cat([g.deg for g in graphs]), B=sum(g.B for g in graphs))

    def copy_(self, other: "FixedGraph") -> "FixedGraph":
        """``other``'s four arrays into this graph's storage, in place: four device copies, no host read (capturable).  ``B``, H, W and
        ``width`` must agree; ``mode`` / ``k`` are taken over."""
        if not isinstance(other, FixedGraph):
            raise DaglError(f"FixedGraph.copy_: a FixedGraph expected, got {type(other).__name__}")
        if (other.B, other.H, other.W) != (self.B, self.H, self.W):
            raise DaglError(f"FixedGraph.copy_: B={other.B} H={other.H} W={other.W} into B={self.B} H={self.H} W={self.W}")
        if other.width != self.width:
            raise DaglError(f"FixedGraph.copy_: width {other.width} into width {self.width}")
        self.key.copy_(other.key); self.weight.copy_(other.weight); self.score.copy_(other.score); self.deg.copy_(other.deg)
        self.mode, self.k = other.mode, other.k
        return self

    def to_csr(self) -> PatchGraph:
        """This graph as a ``PatchGraph`` with scores: row r's first ``deg[r]`` slots (``deg`` clamped to [0, width]) in their order.
        One host read, of the edge count.  ``g.to_fixed(w).to_csr()`` gives ``g``'s arrays back bit for bit."""
        dev = self.device
        deg = self.deg.clamp(0, self.width).long()
        row_off = torch.cat([deg.new_zeros(1), deg.cumsum(0)])
        E = int(row_off[-1])                                                     # the one host read
        rows = torch.repeat_interleave(torch.arange(deg.numel(), device=dev), deg, output_size=E)
        at = rows * self.width + (torch.arange(E, device=dev) - row_off[rows])
        g = object.__new__(PatchGraph)
        g.row_off, g.key, g.weight, g.score = row_off, self.key.reshape(-1)[at], self.weight.reshape(-1)[at], self.score.reshape(-1)[at]
        g.B, g.L, g.N, g.H, g.W, g.mode, g.k = self.B, self.L, self.N, self.H, self.W, self.mode, self.k
        g._valid, g._transposed, g._max_degree = False, None, None
        return g

    def __repr__(self):
        return (f"FixedGraph(B={self.B}, L={self.L}, N={self.N}, width={self.width}, mode={self.mode!r}, k={self.k}, "
                f"device={self.device})")
