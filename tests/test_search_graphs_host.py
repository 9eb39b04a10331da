"""``SequenceState.start`` and the refusals of ``CES.search_graphs`` / ``CES.build_graphs`` that need no device (net.py, sequence.py)."""
import pytest
import torch

SHAPES = [(2, 24, 20), (1, 23, 30), (1, 5, 9)]


@pytest.fixture(scope="module")
def ces():
    from dagl_amd.net import CES
    torch.manual_seed(0)
    return CES(64).eval()


@pytest.mark.parametrize("shape", SHAPES)
def test_start_is_twelve_of_build_graphs_starts(ces, shape):
    from dagl_amd.graph import PatchGraph
    from dagl_amd.sequence import SequenceState
    B, H, W = shape
    state = SequenceState.start(B, H, W, "cpu")
    assert state.B == B and len(state.stages) == 3
    L = -(-H // 4) * -(-W // 4)
    for s in (1, 2, 3):
        heads = ces._stage_modules(s)[0]
        starts = [hd._build_start(B, H, W, "cpu") for hd in heads]
        want = PatchGraph.cat(starts)
        got = state.stages[s - 1]
        assert (got.B, got.H, got.W, got.L) == (4 * B, H, W, L)
        assert torch.equal(got.row_off, want.row_off) and torch.equal(got.key, want.key) and torch.equal(got.weight, want.weight)
        assert got.score is None and got._valid and got.max_degree() == 1
        for h in range(4):
            g = state.head(s - 1, h)
            assert torch.equal(g.row_off, starts[h].row_off) and torch.equal(g.key, starts[h].key) and g.B == B
    # one edge per query, at the query's own position: the patch origin + 3, clamped to the map
    g = state.head(0, 0)
    assert torch.equal(g.row_off, torch.arange(B * L + 1))
    from dagl_amd.synth import same_pad_amounts
    pt, pl = same_pad_amounts(H, 7, 4)[0], same_pad_amounts(W, 7, 4)[0]
    Lw = -(-W // 4)
    for i in (0, L - 1, L // 2):
        qy, qx = divmod(i, Lw)
        y, x = min(max(4 * qy - pt + 3, 0), H - 1), min(max(4 * qx - pl + 3, 0), W - 1)
        assert int(g.key[(B - 1) * L + i]) == y * W + x


def test_start_refuses_bad_shapes():
    from dagl_amd._lib import DaglError
    from dagl_amd.sequence import SequenceState
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        with pytest.raises(DaglError):
            SequenceState.start(*shape, "cpu")


@pytest.mark.parametrize("iters", [0, -1, 1.5, True, None, "2"])
def test_bad_iters(ces, iters):
    from dagl_amd._lib import DaglError
    from dagl_amd.sequence import SequenceState
    x = torch.zeros(1, 64, 8, 8)
    with pytest.raises(DaglError, match="iters"):
        ces.search_graphs(x, SequenceState.start(1, 8, 8, "cpu"), iters=iters)
    with pytest.raises(DaglError, match="iters"):
        ces.build_graphs(x, iters=iters)


def test_want_graphs_false_needs_one_iteration(ces):
    from dagl_amd._lib import DaglError
    from dagl_amd.sequence import SequenceState
    x = torch.zeros(1, 64, 8, 8)
    for iters in (2, 3):
        with pytest.raises(DaglError, match="want_graphs=False"):
            ces.search_graphs(x, SequenceState.start(1, 8, 8, "cpu"), iters=iters, want_graphs=False)


def test_state_and_shape(ces):
    from dagl_amd._lib import DaglError
    from dagl_amd.sequence import SequenceState
    x = torch.zeros(1, 64, 8, 8)
    for state in (None, [], SequenceState.start(1, 8, 8, "cpu").stages[0]):
        with pytest.raises(DaglError, match="SequenceState expected"):
            ces.search_graphs(x, state)
    for shape in ((2, 8, 8), (1, 8, 12), (1, 12, 8)):
        with pytest.raises(DaglError, match="the state was built for"):
            ces.search_graphs(x, SequenceState.start(*shape, "cpu"))
    with pytest.raises(DaglError, match=r"\[B,C,H,W\]"):
        ces.search_graphs(torch.zeros(64, 8, 8), SequenceState.start(1, 8, 8, "cpu"))
    with pytest.raises(DaglError, match=r"\[B,C,H,W\]"):
        ces.build_graphs(torch.zeros(64, 8, 8))


def test_search_keywords(ces):
    from dagl_amd._lib import DaglError
    from dagl_amd.sequence import SequenceState
    x, state = torch.zeros(1, 64, 8, 8), SequenceState.start(1, 8, 8, "cpu")
    with pytest.raises(DaglError, match="explore"):
        ces.search_graphs(x, state, explore=257)
    with pytest.raises(DaglError, match="propagate"):
        ces.search_graphs(x, state, propagate=2)
    with pytest.raises(DaglError, match="seed"):
        ces.search_graphs(x, state, seed=1.5)
    with pytest.raises(DaglError, match="explore"):
        ces.build_graphs(x, explore=-1)


def test_rr_wraps_both():
    from dagl_amd._lib import DaglError
    from dagl_amd.net import RR
    from dagl_amd.sequence import SequenceState
    torch.manual_seed(0)
    rr = RR().eval()
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(DaglError, match="iters"):
        rr.search_graphs(x, SequenceState.start(1, 8, 8, "cpu"), iters=0)
    with pytest.raises(DaglError, match="iters"):
        rr.build_graphs(x, iters=0)
