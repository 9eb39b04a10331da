"""``FixedGraph`` (dagl_amd/graph.py): a patch graph as ``width`` slots per row, on CPU tensors -- the conversions from and to the CSR, the
views and the bookkeeping, ``SequenceState`` over fixed stages, and the refusals of the routes that walk CSR edges."""
import pytest
import torch

from tests.graph_step_reference import MAX_ROW, R_LONG, crafted

SHAPE = (2, 24, 20)
L, N = 30, 480
ARRAYS = ("row_off", "key", "weight", "score")


def _csr(shape=SHAPE, mode="topk", k=3):
    from dagl_amd import PatchGraph
    row_off, key = crafted(shape)
    gen = torch.Generator().manual_seed(3)
    E = key.numel()
    return PatchGraph(row_off.clone(), key.clone(), torch.randn(E, generator=gen), torch.randn(E, generator=gen), *shape, mode, k)


def test_round_trip_is_the_identity():
    """An empty row (0, and L: the first of image 1), repeats (4), unsorted keys (5), -1 / N (6) and the 12-key row (7) come back bit for
    bit, at the largest degree and at a wider width."""
    g = _csr()
    assert g.max_degree() == MAX_ROW
    for width in (None, MAX_ROW, MAX_ROW + 5):
        f = g.to_fixed(width)
        assert f.width == (width or MAX_ROW) and (f.B, f.H, f.W, f.L, f.N, f.mode, f.k) == (2, 24, 20, L, N, "topk", 3)
        assert f.key.shape == f.weight.shape == f.score.shape == (2 * L, f.width) and f.deg.shape == (2 * L,)
        assert f.key.dtype == f.deg.dtype == torch.int32 and f.weight.dtype == f.score.dtype == torch.float32
        back = f.to_csr()
        for n in ARRAYS:
            assert torch.equal(getattr(back, n), getattr(g, n)), (width, n)
        assert (back.B, back.H, back.W, back.mode, back.k) == (g.B, g.H, g.W, g.mode, g.k)
        assert f.n_edges() == g.n_edges and torch.equal(f.degrees(), g.degrees())
    f = g.to_fixed()
    assert f.key[6].tolist()[:3] == [-1, N, 3 * 20 + 3] and int(f.deg[6]) == 3              # carried verbatim
    assert f.key[4].tolist()[:3] == [7 * 20 + 7] * 3 and f.key[5].tolist()[:4] == [N - 3, 10, 9 * 20 + 4, 2 * 20 + 15]
    for b, i in ((0, 0), (0, R_LONG), (1, 0), (1, 3)):
        for got, want in zip(f.row(b, i), g.row(b, i)):
            assert torch.equal(got, want)
    assert "FixedGraph(" in repr(f) and "width=12" in repr(f)


def test_filler_content():
    g = _csr()
    f = g.to_fixed(MAX_ROW + 2)
    live = torch.arange(f.width)[None, :] < f.deg[:, None]
    assert torch.equal(f.deg.long(), g.row_off[1:] - g.row_off[:-1])
    assert bool((f.key[~live] == -1).all()) and not bool(f.weight[~live].any()) and not bool(f.score[~live].any())
    assert int(f.deg[0]) == 0 and int(f.deg[L]) == 0 and int(f.deg[R_LONG]) == MAX_ROW
    assert torch.equal(f.key, g.to_fixed(MAX_ROW + 2).key) and torch.equal(f.weight, g.to_fixed(MAX_ROW + 2).weight)     # every byte defined
    # a graph without scores: zero scores;  an empty graph: width 1, all filler
    from dagl_amd import PatchGraph
    ns = PatchGraph(g.row_off, g.key, g.weight, None, *SHAPE)
    assert not bool(ns.to_fixed().score.any()) and torch.equal(ns.to_fixed().to_csr().key, g.key)
    e = PatchGraph(torch.zeros(2 * L + 1, dtype=torch.int64), torch.empty(0, dtype=torch.int32), torch.empty(0), None, *SHAPE).to_fixed()
    assert e.width == 1 and bool((e.key == -1).all()) and not bool(e.deg.any()) and e.to_csr().n_edges == 0


def test_to_csr_clamps_the_degrees():
    f = _csr().to_fixed()
    f.deg[3], f.deg[8] = -3, f.width + 5
    back = f.to_csr()
    deg = back.row_off[1:] - back.row_off[:-1]
    assert int(deg[3]) == 0 and int(deg[8]) == f.width and f.n_edges() == back.n_edges
    assert torch.equal(back.row(0, 8)[0], f.key[8])


def test_too_small_a_width_is_refused():
    from dagl_amd import DaglError
    g = _csr()
    for width in (MAX_ROW - 1, 1, 0, -2):
        with pytest.raises(DaglError, match="width"):
            g.to_fixed(width)


def test_images_are_views():
    f = _csr().to_fixed()
    one = f.images(1, 2)
    assert (one.B, one.width) == (1, f.width)
    for n in ("key", "weight", "score", "deg"):
        assert getattr(one, n).data_ptr() == getattr(f, n)[L:].data_ptr(), n
    one.key[0, 0] = 77
    assert int(f.key[L, 0]) == 77
    assert f.images(0, 2).key.data_ptr() == f.key.data_ptr()
    from dagl_amd import DaglError
    for lo, hi in ((1, 1), (-1, 1), (0, 3)):
        with pytest.raises(DaglError, match="images"):
            f.images(lo, hi)


def test_cat_and_copy_refusals():
    from dagl_amd import DaglError, FixedGraph
    g = _csr()
    f = g.to_fixed()
    both = FixedGraph.cat([f, f.images(0, 1)])
    assert both.B == 3 and torch.equal(both.key[:2 * L], f.key) and torch.equal(both.deg[2 * L:], f.deg[:L])
    with pytest.raises(DaglError, match="widths"):
        FixedGraph.cat([f, g.to_fixed(MAX_ROW + 1)])
    with pytest.raises(DaglError, match="maps"):
        FixedGraph.cat([f, _csr((1, 33, 70)).to_fixed()])
    for bad in ([], [f, g]):
        with pytest.raises(DaglError, match="FixedGraphs expected"):
            FixedGraph.cat(bad)
    # copy_: all four arrays in place, mode / k taken over
    dst = FixedGraph(torch.zeros_like(f.key), torch.ones_like(f.weight), torch.ones_like(f.score), torch.zeros_like(f.deg), *SHAPE)
    ptr = dst.key.data_ptr()
    assert dst.copy_(f) is dst and dst.key.data_ptr() == ptr and (dst.mode, dst.k) == ("topk", 3)
    for n in ("key", "weight", "score", "deg"):
        assert torch.equal(getattr(dst, n), getattr(f, n))
    with pytest.raises(DaglError, match="width"):
        dst.copy_(g.to_fixed(MAX_ROW + 1))
    with pytest.raises(DaglError, match="B=1"):
        dst.copy_(f.images(0, 1))
    with pytest.raises(DaglError, match="FixedGraph expected"):
        dst.copy_(g)
    # the constructor's own checks
    for kw, word in ((dict(key=f.key.long()), "dtype"), (dict(deg=f.deg[:-1]), "deg"), (dict(weight=f.weight[:, :-1].contiguous()), "shape"),
                     (dict(key=f.key[:, ::2]), "contiguous")):
        a = dict(key=f.key, weight=f.weight, score=f.score, deg=f.deg)
        a.update(kw)
        with pytest.raises(DaglError, match=word):
            FixedGraph(a["key"], a["weight"], a["score"], a["deg"], *SHAPE)


def test_sequence_state_over_fixed_stages():
    from dagl_amd import DaglError, PatchGraph
    from dagl_amd.sequence import SequenceState
    g = _csr((1, 24, 20))
    stage = PatchGraph.cat([g, g, g, g])
    csr = SequenceState([stage, stage, stage])
    assert not csr.fixed and not csr.has_head(0, 1)
    fixed = csr.to_fixed()
    assert fixed.fixed and fixed.B == 1 and all(fixed.has_head(s, h) for s in range(3) for h in range(4))
    with pytest.raises(DaglError, match="never mixed"):
        SequenceState([stage, fixed.stages[1], stage])
    head = fixed.head(1, 2)
    assert head.B == 1 and head.key.data_ptr() == fixed.stages[1].key[2 * L:].data_ptr()
    back = fixed.to_csr()
    for s in range(3):
        for n in ARRAYS:
            assert torch.equal(getattr(back.stages[s], n), getattr(stage, n)), (s, n)
    other = csr.to_fixed(MAX_ROW)
    other.stages[2].key.fill_(5)
    assert fixed.copy_(other) is fixed and bool((fixed.stages[2].key == 5).all()) and bool((head.key == other.stages[1].key[2 * L:3 * L]).all())
    for bad in (csr, None):
        with pytest.raises(DaglError, match="copy_"):
            fixed.copy_(bad)
    with pytest.raises(DaglError, match="already"):
        fixed.to_fixed()
    with pytest.raises(DaglError, match="already"):
        csr.to_csr()
    with pytest.raises(DaglError, match="width"):
        fixed.copy_(csr.to_fixed(MAX_ROW + 1))


def test_csr_routes_refuse_a_fixed_graph(monkeypatch):
    """``apply_graph``, ``attend_graph`` and ``forward_on_graph`` name ``.to_csr()`` and never reach the library."""
    from dagl_amd import DaglError, _lib
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    from dagl_amd.sequence import SequenceState
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    ce = CE(in_channels=64)
    x = torch.zeros(2, 64, 24, 20)
    f = _csr().to_fixed()
    for call in (ce.apply_graph, ce.attend_graph, ce.forward_on_graph):
        with pytest.raises(DaglError, match=r"\.to_csr\(\)"):
            call(x, f)
    # a CES on a fixed state: forward_on_graphs and search_graphs refuse likewise, step_graphs refuses fused=True
    g1 = _csr((1, 24, 20)).to_fixed()
    from dagl_amd import FixedGraph
    stage = FixedGraph.cat([g1] * 4)
    state = SequenceState([stage] * 3)
    ces = CES(64)
    x1 = torch.zeros(1, 64, 24, 20)
    with pytest.raises(DaglError, match=r"\.to_csr\(\)"):
        ces.forward_on_graphs(x1, state)
    with pytest.raises(DaglError, match=r"\.to_csr\(\)"):
        ces.search_graphs(x1, state)
    with pytest.raises(DaglError, match="fused=True"):
        ces.step_graphs(x1, state, fused=True)
    with pytest.raises(DaglError, match="GPU"):                            # fused=None: head by head, as far as the CPU input
        ces.step_graphs(x1, state)
