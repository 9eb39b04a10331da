"""``PatchGraph.cat`` / ``PatchGraph.images`` and ``SequenceState`` (dagl_amd/graph.py, dagl_amd/sequence.py): plain bookkeeping on CPU tensors."""
import pytest
import torch

from dagl_amd import DaglError, PatchGraph
from dagl_amd.sequence import SequenceState

H, W = 9, 6                     # L = 3 * 2 = 6, N = 54
L, N = 6, 54
ARRAYS = ("row_off", "key", "weight", "score")


def _graph(B, seed, degrees=None, score=True, mode="topk", k=3):
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 5, (B * L,), generator=gen) if degrees is None else torch.tensor(degrees)
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    E = int(row_off[-1])
    key = torch.randint(0, N, (E,), generator=gen, dtype=torch.int32)
    weight = torch.rand(E, generator=gen)
    return PatchGraph(row_off, key, weight, torch.randn(E, generator=gen) if score else None, B, H, W, mode, k)


def _same(a, b):
    for n in ARRAYS:
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None and y is None) or torch.equal(x, y), n
    assert (a.B, a.H, a.W, a.L, a.N) == (b.B, b.H, b.W, b.L, b.N)


def test_cat_then_images_returns_the_inputs():
    # the seam rows are empty on both sides of the first seam, full on both sides of the second
    parts = [_graph(2, 1, degrees=[3, 0, 2, 1, 4, 0] + [1, 1, 0, 2, 0, 0]),
             _graph(1, 2, degrees=[0, 0, 3, 1, 2, 4]),
             _graph(3, 3, degrees=[2] * 18)]
    g = PatchGraph.cat(parts)
    assert g.B == 6 and g.row_off.numel() == 6 * L + 1 and g.n_edges == sum(p.n_edges for p in parts)
    assert int(g.row_off[0]) == 0 and int(g.row_off[-1]) == g.n_edges and bool((g.row_off[1:] >= g.row_off[:-1]).all())
    assert (g.mode, g.k) == (parts[0].mode, parts[0].k)
    lo = 0
    for p in parts:
        _same(g.images(lo, lo + p.B), p)
        lo += p.B
    _same(g.images(0, g.B), g)
    # rebasing: the rows of image 2 (the second part) through the whole graph and through the part
    for i in range(L):
        for a, b in zip(g.row(2, i), parts[1].row(0, i)):
            assert torch.equal(a, b)
    # the arrays of a sub-graph are views
    sub = g.images(2, 3)
    assert sub.key.data_ptr() == g.key[int(g.row_off[2 * L]):].data_ptr() and sub.weight._base is not None
    # a range over a seam
    both = g.images(1, 4)
    assert both.B == 3 and torch.equal(both.degrees().reshape(-1), g.degrees().reshape(-1)[L:4 * L])
    assert int(both.row_off[0]) == 0 and int(both.row_off[-1]) == both.n_edges


def test_cat_of_empty_graphs_and_without_scores():
    empty = [_graph(1, 0, degrees=[0] * L, score=False) for _ in range(4)]
    g = PatchGraph.cat(empty)
    assert g.B == 4 and g.n_edges == 0 and g.score is None and not bool(g.row_off.any())
    _same(g.images(1, 3), PatchGraph.cat(empty[:2]))
    mixed = PatchGraph.cat([empty[0], _graph(1, 5, score=False), empty[1]])
    _same(mixed.images(0, 1), empty[0])
    _same(mixed.images(2, 3), empty[1])
    assert mixed.images(1, 2).n_edges == mixed.n_edges
    _same(PatchGraph.cat([empty[0]]), empty[0])


def test_cat_hands_on_validity_and_the_largest_degree():
    a, b = _graph(1, 1), _graph(1, 2)
    assert not PatchGraph.cat([a, b])._valid and PatchGraph.cat([a, b])._max_degree is None
    a.validate()
    assert not PatchGraph.cat([a, b])._valid
    b.validate()
    assert PatchGraph.cat([a, b])._valid and PatchGraph.cat([a, b]).images(1, 2)._valid
    da = a.max_degree()
    assert PatchGraph.cat([a, b])._max_degree is None
    db = b.max_degree()
    g = PatchGraph.cat([a, b])
    assert g._max_degree == max(da, db) == g.max_degree() == int(g.degrees().max())
    assert g.images(0, 1)._max_degree is None


def test_mismatched_inputs_are_refused():
    a = _graph(1, 1)
    other_map = PatchGraph(torch.zeros(5, dtype=torch.int64), torch.empty(0, dtype=torch.int32), torch.empty(0), torch.empty(0), 1, 6, 6)
    for bad, word in (([a, other_map], "maps"), ([a, _graph(1, 2, score=False)], "score"), ([], "non-empty"), ([a, "graph"], "PatchGraph")):
        with pytest.raises(DaglError, match=word):
            PatchGraph.cat(bad)
    if torch.cuda.is_available():
        with pytest.raises(DaglError, match="graphs on"):
            PatchGraph.cat([a, _graph(1, 2).to("cuda:0")])
    for lo, hi in ((-1, 1), (0, 0), (1, 1), (0, 2), (1, 0)):
        with pytest.raises(DaglError, match="images"):
            a.images(lo, hi)


def test_sequence_state_bookkeeping():
    B = 2
    heads = [_graph(B, 10 + i) for i in range(12)]
    state = SequenceState.from_heads(heads)
    assert len(state.stages) == 3 and state.B == B and all(g.B == 4 * B for g in state.stages)
    for s in range(3):
        _same(state.stages[s], PatchGraph.cat(heads[4 * s:4 * s + 4]))
        for h in range(4):
            assert state.has_head(s, h) and state.head(s, h) is heads[4 * s + h]
            # row (h B + b) L + i of the stage graph is query i of image b under head h
            for a, b in zip(state.stages[s].row(h * B + 1, 3), heads[4 * s + h].row(1, 3)):
                assert torch.equal(a, b)
    rebuilt = SequenceState(state.stages)
    for s in range(3):
        for h in range(4):
            assert not rebuilt.has_head(s, h)
            _same(rebuilt.head(s, h), heads[4 * s + h])
            assert rebuilt.has_head(s, h) and rebuilt.head(s, h) is rebuilt.head(s, h)
    moved = state.to("cpu")
    assert isinstance(moved, SequenceState) and all(g.row_off.device.type == "cpu" for g in moved.stages)
    for s in range(3):
        _same(moved.stages[s], state.stages[s])
    with pytest.raises(IndexError):
        state.head(3, 0)
    with pytest.raises(IndexError):
        state.head(0, 4)
    for bad, word in ((heads[:11], "12"), (heads[:11] + [_graph(B + 1, 0)], "share B")):
        with pytest.raises(DaglError, match=word):
            SequenceState.from_heads(bad)
    with pytest.raises(DaglError, match="3 PatchGraphs"):
        SequenceState(state.stages[:2])
    with pytest.raises(DaglError, match="heads"):
        SequenceState([_graph(3, 0)] * 3)
    with pytest.raises(DaglError, match="share"):
        SequenceState([state.stages[0], state.stages[1], PatchGraph.cat([_graph(1, i) for i in range(4)])])
