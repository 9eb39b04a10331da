"""tests/graph_search_reference.py against brute force: a triple loop over rows, sources and window cells on a 9 x 10 map, the hash in
plain Python integers.  No GPU."""
import numpy as np
import torch

from tests import graph_refresh_reference as refresh_ref
from tests.graph_search_reference import ADJACENT, candidate_mask, emptied_rows, explore_keys, lowbias32

B, H, W = 2, 9, 10
LH, LW = 3, 3
L, N = LH * LW, H * W


def _lowbias32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _graph(seed=3):
    """Rows of 0 .. 4 keys, keys of -1 and N among them; row 4 (the grid's centre) of image 0 empty; corners of the map in the grid's
    corner rows, so that propagated centres fall off the map."""
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randint(-1, N + 1, (int(torch.randint(0, 5, (1,), generator=gen)),), generator=gen).tolist() for _ in range(B * L)]
    rows[0] = [0, 1]                              # propagated to row 1 with centre x - 4 < 0 ...
    rows[2] = [W - 1]                             # ... and to row 1 with centre x + 4 >= W
    rows[4] = []
    rows[L - 1] = [N - 1, -1, N]                  # the last row of image 0
    rows[L] = [5 * W + 5]                         # the first row of image 1
    row_off = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0)
    return rows, row_off, torch.tensor([k for r in rows for k in r], dtype=torch.int32)


def _brute(rows, radius, propagate, explore, seed):
    mask = torch.zeros(B * L, N, dtype=torch.bool)

    def window(r, cy, cx):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if 0 <= cy + dy < H and 0 <= cx + dx < W:
                    mask[r, (cy + dy) * W + cx + dx] = True

    for r in range(B * L):
        b, q = divmod(r, L)
        qy, qx = divmod(q, LW)
        for key in rows[r]:
            if 0 <= key < N:
                window(r, key // W, key % W)
        if propagate:
            for dqy, dqx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                if 0 <= qy + dqy < LH and 0 <= qx + dqx < LW:
                    for key in rows[b * L + (qy + dqy) * LW + qx + dqx]:
                        if 0 <= key < N:
                            window(r, key // W - 4 * dqy, key % W - 4 * dqx)
        for t in range(explore):
            h = _lowbias32_int(_lowbias32_int(r ^ (seed & 0xFFFFFFFF)) + t)
            mask[r, (h * N) >> 32] = True
    return mask


def test_hash_values_are_pinned():
    assert [int(v) for v in lowbias32(np.array([0, 1, 0xFFFFFFFF, 12345], dtype=np.uint32))] == [0x0, 0x688990c0, 0x6768824a, 0x912efcf7]
    assert int(lowbias32(np.uint32(1))) == 0x688990c0
    # h_t of row 7 with seed 3, and the keys they give on a 24 x 20 map
    assert [_lowbias32_int(_lowbias32_int(7 ^ 3) + t) for t in range(3)] == [0x8fd96704, 0x98d8b89c, 0xe683f479]
    assert explore_keys(8, 480, 3, 3)[7].tolist() == [269, 286, 432]
    rnd = np.random.default_rng(0).integers(0, 1 << 32, 1000, dtype=np.uint64)
    assert [int(v) for v in lowbias32(rnd.astype(np.uint32))] == [_lowbias32_int(int(v)) for v in rnd]


def test_explored_keys_stay_below_n():
    for n in (1, (1 << 31) - 1):
        for seed in (0, 1, 0xFFFFFFFF, -1, 1 << 40):
            k = explore_keys(4096, n, 16, seed)
            assert int(k.min()) >= 0 and int(k.max()) < n
    assert bool((explore_keys(64, 1, 8, 5) == 0).all())
    # the largest hash value still lands below N
    assert (0xFFFFFFFF * ((1 << 31) - 1)) >> 32 == (1 << 31) - 2
    # a seed is taken modulo 2^32
    assert torch.equal(explore_keys(32, 480, 4, -1), explore_keys(32, 480, 4, 0xFFFFFFFF))
    assert torch.equal(explore_keys(32, 480, 4, (1 << 32) + 9), explore_keys(32, 480, 4, 9))


def test_candidate_mask_against_brute_force():
    rows, row_off, key = _graph()
    assert ADJACENT == ((0, -1), (0, 1), (-1, 0), (1, 0))
    for radius in (0, 1, 2):
        for propagate in (False, True):
            for explore, seed in ((0, 0), (5, 0), (5, 11)):
                got = candidate_mask(row_off, key, B, H, W, radius, propagate, explore, seed)
                assert torch.equal(got, _brute(rows, radius, propagate, explore, seed)), (radius, propagate, explore, seed)
        # with both sources off: the refresh's reference
        assert torch.equal(candidate_mask(row_off, key, B, H, W, radius), refresh_ref.candidate_mask(row_off, key, H, W, radius))


def test_adjacency_stays_inside_a_grid_row_and_an_image():
    """A graph with a single edge: only the row itself and its grid neighbours of the same image see it."""
    for r_src, reached in ((2, {2, 1, 5}),                        # the end of grid row 0: row 3 (the next grid row's first) does not see it
                           (3, {3, 4, 0, 6}),                     # the start of grid row 1: row 2 does not
                           (L - 1, {L - 1, L - 2, L - 1 - LW}),   # the last row of image 0: row L (image 1) does not
                           (L, {L, L + 1, L + LW})):              # the first row of image 1: row L - 1 does not
        deg = torch.zeros(B * L, dtype=torch.int64)
        deg[r_src] = 1
        row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
        key = torch.tensor([4 * W + 5], dtype=torch.int32)
        got = candidate_mask(row_off, key, B, H, W, 0, True)
        assert set(got.any(dim=1).nonzero().view(-1).tolist()) == reached, r_src
        assert int(got.sum()) == len(reached)


def test_an_off_map_centre_keeps_its_on_map_cells():
    # row 1's left neighbour (row 0) holds key (0, 1): the centre as row 1 sees it is (0, 5); row 0 sees row 1's key (0, 2) at (0, -2)
    deg = torch.zeros(B * L, dtype=torch.int64)
    deg[1] = 1
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    key = torch.tensor([2], dtype=torch.int32)
    for radius, want in ((0, []), (1, []), (2, [0, W, 2 * W]), (3, [0, 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W, 3 * W + 1])):
        got = candidate_mask(row_off, key, B, H, W, radius, True)
        assert got[0].nonzero().view(-1).tolist() == want, radius
    # row 4 sees row 1's key (0, 2) at (0 + 4, 2): on the map; row 1 is (-1, 0) of row 4
    assert candidate_mask(row_off, key, B, H, W, 0, True)[4].nonzero().view(-1).tolist() == [4 * W + 2]


def test_emptied_rows():
    deg = torch.ones(B * L, dtype=torch.int64)
    deg[2], deg[L] = 5, 5
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    assert emptied_rows(row_off, B, H, W, 4, False).nonzero().view(-1).tolist() == [2, L]
    assert emptied_rows(row_off, B, H, W, 4, True).nonzero().view(-1).tolist() == [1, 2, 5, L, L + 1, L + LW]
    assert not bool(emptied_rows(row_off, B, H, W, 5, True).any())
