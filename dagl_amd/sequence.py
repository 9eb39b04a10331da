"""``SequenceState`` -- the patch graphs a ``CES`` carries from frame to frame: one ``PatchGraph`` per stage over the stage's four heads.

``CES.forward_with_graphs`` / ``RR.forward_with_graphs`` return one for the key frame, ``step_graphs`` / ``search_graphs`` take it and
return the next; ``SequenceState.start`` is the trivial state ``build_graphs`` searches from.  Plain
bookkeeping over ``PatchGraph`` (graph.py): it works on CPU tensors.
"""
from __future__ import annotations

from ._lib import DaglError
from .graph import FixedGraph, PatchGraph

STAGES, HEADS = 3, 4


class SequenceState:
    """``stages[s]`` (s = 0, 1, 2): the graphs of stage ``s + 1``'s four heads as ONE ``PatchGraph`` over ``4 * B`` images, head-major --
    row ``(h * B + b) * L + i`` is query ``i`` of image ``b`` under head ``h`` (``PatchGraph.cat`` of the heads' graphs).

    The three stages may be ``FixedGraph``s instead (``to_fixed``; all three, never mixed): the state ``step_graphs`` moves without a host
    read and under stream capture, ``copy_`` taking the new state into the captured one's storage."""

    def __init__(self, stages):
        stages = list(stages)
        if len(stages) != STAGES or not (all(isinstance(g, PatchGraph) for g in stages) or all(isinstance(g, FixedGraph) for g in stages)):
            raise DaglError(f"SequenceState: {STAGES} PatchGraphs or {STAGES} FixedGraphs expected, one per stage (never mixed)")
        for g in stages:
            if g.B % HEADS:
                raise DaglError(f"SequenceState: a stage graph over {g.B} images does not hold {HEADS} heads of a batch")
            if (g.B, g.H, g.W) != (stages[0].B, stages[0].H, stages[0].W):
                raise DaglError("SequenceState: the stage graphs must share B, H and W")
        self.stages = stages
        self._heads = {}                 # (s, h) -> the head's sub-graph: ``images`` reads two offsets on the host, once per state

    @property
    def B(self) -> int:
        """Images per head."""
        return self.stages[0].B // HEADS

    @property
    def fixed(self) -> bool:
        """Whether the stages are ``FixedGraph``s."""
        return isinstance(self.stages[0], FixedGraph)

    def to_fixed(self, width=None) -> "SequenceState":
        """The state with every stage as a ``FixedGraph`` of ``width`` slots per row (None: each stage's own largest degree)."""
        if self.fixed:
            raise DaglError("SequenceState.to_fixed: the stages are FixedGraphs already")
        return SequenceState(g.to_fixed(width) for g in self.stages)

    def to_csr(self) -> "SequenceState":
        """The state with every stage as a ``PatchGraph`` (one host read per stage)."""
        if not self.fixed:
            raise DaglError("SequenceState.to_csr: the stages are PatchGraphs already")
        return SequenceState(g.to_csr() for g in self.stages)

    def copy_(self, other: "SequenceState") -> "SequenceState":
        """``other``'s arrays into this state's storage, stage by stage (``FixedGraph.copy_``: no host read, capturable)."""
        if not isinstance(other, SequenceState) or not (self.fixed and other.fixed):
            raise DaglError("SequenceState.copy_: two states of FixedGraphs expected (a CSR's size depends on its content)")
        for mine, theirs in zip(self.stages, other.stages):
            mine.copy_(theirs)
        return self

    @classmethod
    def from_heads(cls, graphs) -> "SequenceState":
        """From the 12 graphs of the heads in module order: c1_1 .. c1_4, c2_1 .. c2_4, c3_1 .. c3_4."""
        graphs = list(graphs)
        if len(graphs) != STAGES * HEADS:
            raise DaglError(f"SequenceState.from_heads: {STAGES * HEADS} graphs expected, got {len(graphs)}")
        if not all(isinstance(g, PatchGraph) for g in graphs) or len({g.B for g in graphs}) != 1:
            raise DaglError("SequenceState.from_heads: PatchGraphs that share B expected")
        state = cls(PatchGraph.cat(graphs[s * HEADS:(s + 1) * HEADS]) for s in range(STAGES))
        state._heads = {(s, h): graphs[s * HEADS + h] for s in range(STAGES) for h in range(HEADS)}
        return state

    @classmethod
    def start(cls, B: int, H: int, W: int, device=None, mode: str = "adaptive") -> "SequenceState":
        """The state a search starts from (``CES.build_graphs``): twelve trivial graphs over ``B`` images of ``H x W`` -- one edge per
        query at the query's own position, ``CE.build_graph``'s start (``graph.trivial_graph``).  The heads share the arrays."""
        from .graph import trivial_graph
        g = trivial_graph(B, H, W, device, mode)
        return cls.from_heads([g] * (STAGES * HEADS))

    def head(self, s: int, h: int):
        """The graph of head ``h`` (0..3) of stage ``s`` (0..2): ``stages[s].images(h * B, (h + 1) * B)``, kept on the object.  Of a
        fixed state: row views of the stage's arrays, no host read."""
        s, h = int(s), int(h)
        if not (0 <= s < STAGES and 0 <= h < HEADS):
            raise IndexError(f"SequenceState.head: ({s}, {h}) outside [0, {STAGES}) x [0, {HEADS})")
        if (s, h) not in self._heads:
            self._heads[(s, h)] = self.stages[s].images(h * self.B, (h + 1) * self.B)
        return self._heads[(s, h)]

    def has_head(self, s: int, h: int) -> bool:
        """Whether ``head(s, h)`` is at hand without a host read (a fixed state: always)."""
        return self.fixed or (int(s), int(h)) in self._heads

    def to(self, device) -> "SequenceState":
        return SequenceState(g.to(device) for g in self.stages)

    def __repr__(self):
        return f"SequenceState({', '.join(repr(g) for g in self.stages)})"
