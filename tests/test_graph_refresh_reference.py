"""The yardstick of the graph-refresh tests (tests/graph_refresh_reference.py) against brute force -- a Python loop over edges and windows,
a Python sort for the selection -- on a 5 x 6 map, before the GPU sees it."""
import pytest
import torch

from tests.graph_refresh_reference import candidate_mask, csr_of, mask_of, select_mask

H, W = 5, 6
N = H * W
# rows: a corner, the opposite corner with a border key, two adjacent keys (overlapping windows), a repeated key, keys outside [0, N) next
# to a valid one, an empty row, unsorted keys in the middle, only out-of-range keys
ROWS = [[0], [N - 1, W - 1], [14, 15], [8, 8, 8], [-1, N, 7, N + 3, -7], [], [22, 3, 16], [N, -1]]


def _csr(rows):
    off = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0)
    return off, torch.tensor([k for r in rows for k in r], dtype=torch.int32)


def _brute_candidates(rows, radius):
    out = []
    for r in rows:
        s = set()
        for key in r:
            if not 0 <= key < N:
                continue
            y, x = divmod(key, W)
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        s.add((y + dy) * W + x + dx)
        out.append(s)
    return out


@pytest.mark.parametrize("radius", [0, 1, 2, 8])
def test_candidates_against_brute_force(radius):
    mask = candidate_mask(*_csr(ROWS), H, W, radius)
    assert mask.shape == (len(ROWS), N)
    for r, want in enumerate(_brute_candidates(ROWS, radius)):
        assert set(mask[r].nonzero().view(-1).tolist()) == want, (r, radius)
    if radius == 0:
        assert [int(v) for v in mask.sum(dim=1)] == [1, 2, 2, 1, 1, 0, 3, 0]
    if radius == 1:
        # a corner keeps 4 of its 9, a border key 6; two adjacent keys share 6 of their windows: 12, not 18
        # (row 6: 9 + 6 + 9 less the 6 keys the windows of 22 and 16 share and the 2 those of 3 and 16 share)
        assert [int(v) for v in mask.sum(dim=1)] == [4, 4 + 4, 12, 9, 9, 0, 9 + 6 + 9 - 6 - 2, 0]
        assert not bool(mask[0, W - 1]) and not bool(mask[0, 2 * W])            # clipped, not wrapped
    if radius == 8:
        assert bool(mask[[0, 1, 2, 3, 4, 6]].all()) and not bool(mask[[5, 7]].any())


def _brute_select(cand, S, tau, k):
    keep = torch.zeros_like(cand)
    for r in range(cand.shape[0]):
        js = [j for j in range(cand.shape[1]) if cand[r, j] and (tau is None or float(S[r, j] - tau[r]) > 0)]
        js.sort(key=lambda j: (-float(S[r, j]), j))
        for j in (js[:k] if k > 0 else js):
            keep[r, j] = True
    return keep


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 40])
@pytest.mark.parametrize("with_tau", [False, True])
def test_selection_against_brute_force(with_tau, k):
    cand = candidate_mask(*_csr(ROWS), H, W, 1)
    gen = torch.Generator().manual_seed(3)
    S = torch.randint(0, 4, (len(ROWS), N), generator=gen).float() / 4           # few levels: ties at every place
    tau = torch.tensor([0.2, -1.0, 0.3, 5.0, 0.0, 0.1, 0.3, 0.2]) if with_tau else None
    got = select_mask(cand, S, tau, k)
    assert torch.equal(got, _brute_select(cand, S, tau, k))
    assert not bool((got & ~cand).any())
    if with_tau:
        assert int(got[3].sum()) == 0                                            # every candidate fails tau
    if k > 0:
        assert int(got.sum(dim=1).max()) <= k


def test_tie_rule_on_hand_written_scores():
    """One row, candidates 3 .. 8; scores 1 2 2 2 1 3: k = 2 keeps key 8 (the 3) and, of the three 2s, the LOWEST key 4; k = 3 adds key
    5; k = 4 key 6; with tau = 1 the 1s fail and k = 5 keeps the four that pass."""
    cand = torch.zeros(1, 12, dtype=torch.bool)
    cand[0, 3:9] = True
    S = torch.full((1, 12), 9.0)                                                 # off the candidates: larger than all, never looked at
    S[0, 3:9] = torch.tensor([1.0, 2.0, 2.0, 2.0, 1.0, 3.0])
    pick = lambda tau, k: select_mask(cand, S, tau, k)[0].nonzero().view(-1).tolist()
    assert pick(None, 1) == [8] and pick(None, 2) == [4, 8] and pick(None, 3) == [4, 5, 8] and pick(None, 4) == [4, 5, 6, 8]
    assert pick(None, 5) == [3, 4, 5, 6, 8]                                      # ... and of the two 1s the lower key
    assert pick(None, 0) == pick(None, 6) == pick(None, 50) == [3, 4, 5, 6, 7, 8]
    one = torch.tensor([1.0])
    assert pick(one, 5) == pick(one, 0) == [4, 5, 6, 8] and pick(one, 2) == [4, 8]
    assert pick(torch.tensor([3.0]), 0) == []


def test_csr_round_trip():
    mask = candidate_mask(*_csr(ROWS), H, W, 1)
    off, key = csr_of(mask)
    assert int(off[-1]) == key.numel() == int(mask.sum()) and key.dtype == torch.int32
    assert torch.equal(mask_of(off, key, N), mask)
    assert torch.equal(candidate_mask(off, key, H, W, 0), mask)                  # radius 0: the distinct valid keys
