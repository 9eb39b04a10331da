"""``PatchGraph``'s editing methods -- ``with_weight``, ``select``, ``transpose``, ``validate``, ``to`` -- on small hand-written CSRs, on
the CPU: empty rows, an empty graph, repeated keys, rows on either side of the image boundary of a batch of two."""
import pytest
import torch

from dagl_amd import DaglError
from dagl_amd.graph import PatchGraph

B, H, W = 2, 8, 4               # L = 2 x 1 query rows per image, N = 32 keys
L, N = 2, 32


def _graph(rows, weights=None):
    """rows: one list of keys per query row (B * L of them)."""
    deg = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    key = torch.tensor([k for r in rows for k in r], dtype=torch.int32)
    if weights is None:
        weights = torch.arange(1, key.numel() + 1, dtype=torch.float32) / 8
    return PatchGraph(row_off, key, weights, None, B, H, W)


def _dense(g, weight=None):
    """[B * L, N] with repeated keys added up."""
    a = torch.zeros(g.B * g.L, g.N, dtype=torch.float64)
    w = (g.weight if weight is None else weight).double()
    return a.index_put_((g.rows(), g.key.long()), w, accumulate=True)


# the last row of image 0 is long and unsorted with a repeated key, the first row of image 1 is empty
ROWS = [[5, 3, 5], [31, 0, 7, 7, 2], [], [0, 31]]
CASES = {"mixed": ROWS, "empty_rows_only_first": [[1], [], [], []], "empty_graph": [[], [], [], []],
         "all_in_last": [[], [], [], [4, 4, 4, 9]]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_transpose_round_trips(name):
    g = _graph(CASES[name])
    col_off, src_row, perm = g.transpose()
    assert col_off.dtype == torch.int64 and src_row.dtype == torch.int32 and perm.dtype == torch.int32
    assert col_off.numel() == B * N + 1 and int(col_off[0]) == 0 and int(col_off[-1]) == g.n_edges
    assert bool((col_off[1:] >= col_off[:-1]).all())
    assert sorted(perm.tolist()) == list(range(g.n_edges))
    # scattering weight[perm] by (col_off, src_row) rebuilds the dense matrix
    cols = torch.repeat_interleave(torch.arange(B * N), col_off[1:] - col_off[:-1])
    assert torch.equal(torch.div(cols, N, rounding_mode="floor"), torch.div(src_row.long(), L, rounding_mode="floor"))   # same image
    back = torch.zeros(B * L, N, dtype=torch.float64).index_put_((src_row.long(), cols % N), g.weight[perm.long()].double(), accumulate=True)
    assert torch.equal(back, _dense(g))
    # a stable sort: the edges of one column keep their order
    same = cols[1:] == cols[:-1]
    assert bool((perm[1:] > perm[:-1])[same].all())
    assert g.transpose() is g.transpose()                      # kept on the object


def test_with_weight_keeps_the_structure():
    g = _graph(ROWS)
    w = torch.randn(g.n_edges)
    h = g.with_weight(w)
    assert h.row_off is g.row_off and h.key is g.key and h.weight is w
    assert (h.B, h.H, h.W, h.L, h.N, h.mode, h.k) == (g.B, g.H, g.W, g.L, g.N, g.mode, g.k)
    assert torch.equal(_dense(h), _dense(g, w))
    wg = torch.randn(g.n_edges, requires_grad=True)
    assert g.with_weight(wg).weight is wg                      # a weight that requires grad is kept as it is
    for bad in (torch.randn(g.n_edges + 1), torch.randn(g.n_edges).double(), torch.randn(1, g.n_edges)):
        with pytest.raises(DaglError):
            g.with_weight(bad)
    e = _graph(CASES["empty_graph"])
    assert e.with_weight(torch.empty(0)).n_edges == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_select(name):
    g = _graph(CASES[name])
    same = g.select(torch.ones(g.n_edges, dtype=torch.bool))
    for a in ("row_off", "key", "weight"):
        assert torch.equal(getattr(same, a), getattr(g, a)), a
    gen = torch.Generator().manual_seed(3)
    mask = torch.rand(g.n_edges, generator=gen) < 0.5
    s = g.select(mask)
    assert s.row_off.dtype == torch.int64 and s.row_off.numel() == B * L + 1 and int(s.row_off[-1]) == int(mask.sum())
    assert torch.equal(s.key, g.key[mask]) and torch.equal(s.weight, g.weight[mask])
    assert torch.equal(_dense(s), _dense(g, torch.where(mask, g.weight, torch.zeros(()))))
    none = g.select(torch.zeros(g.n_edges, dtype=torch.bool))
    assert none.n_edges == 0 and torch.equal(none.row_off, torch.zeros(B * L + 1, dtype=torch.int64))
    with pytest.raises(DaglError):
        g.select(torch.ones(g.n_edges + 1, dtype=torch.bool))
    with pytest.raises(DaglError):
        g.select(torch.ones(g.n_edges))


def test_select_carries_scores_and_gradients():
    g0 = _graph(ROWS)
    g = PatchGraph(g0.row_off, g0.key, g0.weight, g0.weight * 3, B, H, W, "topk", 5)
    mask = torch.tensor([True, False] * 5)
    s = g.select(mask)
    assert torch.equal(s.score, g.score[mask]) and (s.mode, s.k) == ("topk", 5)
    w = torch.randn(g.n_edges, requires_grad=True)
    g.with_weight(w).select(mask).weight.sum().backward()
    assert torch.equal(w.grad, mask.float())


def test_validate():
    ok = _graph([[0, N - 1], [], [N - 1], [0]])
    assert ok.validate() is ok and ok._valid
    assert ok.with_weight(ok.weight * 2)._valid and ok.select(ok.weight > 0)._valid and ok.to("cpu")._valid
    for bad_key in (N, -1):
        g = _graph([[0, 1], [], [3, bad_key, N + 7], [2]])
        with pytest.raises(DaglError) as err:
            g.validate()
        msg = str(err.value)
        assert "edge 3" in msg and f"key {bad_key}" in msg and "query 0 of image 1" in msg, msg
        assert not g._valid
        with pytest.raises(DaglError):
            g.transpose()                                      # the transposed CSR is built over valid keys only
    assert _graph(CASES["empty_graph"]).validate()._valid


def test_to_moves_every_array():
    g0 = _graph(ROWS)
    g = PatchGraph(g0.row_off, g0.key, g0.weight, g0.weight + 1, B, H, W)
    g.transpose()
    h = g.to("cpu")
    assert h is not g and (h.B, h.H, h.W) == (B, H, W)
    for a in ("row_off", "key", "weight", "score"):
        assert torch.equal(getattr(h, a), getattr(g, a)) and getattr(h, a).device.type == "cpu"
    assert all(torch.equal(a, b) for a, b in zip(h.transpose(), g.transpose()))
    assert repr(h).startswith("PatchGraph(")
