"""``PatchGraph.max_degree`` on CPU tensors: the value, and who hands the kept value on."""
import torch

from dagl_amd.graph import PatchGraph


def _graph(deg):
    off = torch.tensor([0] + deg, dtype=torch.int64).cumsum(0)
    E = int(off[-1])
    return PatchGraph(off, torch.arange(E, dtype=torch.int32) % 16, torch.ones(E), None, 1, 4, 4)      # L = 1, N = 16


def test_value_and_cache():
    g = PatchGraph(torch.tensor([0, 3, 3, 10, 12]), torch.zeros(12, dtype=torch.int32), torch.ones(12), None, 1, 8, 8)      # L = 4
    assert g._max_degree is None and g.max_degree() == 7 and g._max_degree == 7
    g.row_off = None                                   # (the second call does not look at the offsets again)
    assert g.max_degree() == 7


def test_empty_graph():
    g = PatchGraph(torch.zeros(5, dtype=torch.int64), torch.empty(0, dtype=torch.int32), torch.empty(0), None, 1, 8, 8)
    assert g.max_degree() == 0


def test_who_hands_it_on():
    g = _graph([5])
    assert g.max_degree() == 5
    assert g.with_weight(torch.zeros(5))._max_degree == 5 and g.to("cpu")._max_degree == 5
    sel = g.select(torch.tensor([True, False, True, False, False]))
    assert sel._max_degree is None and sel.max_degree() == 2
    fresh = _graph([5])
    assert fresh.with_weight(torch.zeros(5))._max_degree is None and fresh.to("cpu")._max_degree is None
