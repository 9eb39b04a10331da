"""The CPU reference of ``dagl_graph_search``'s candidates (checked against brute force by test_graph_search_reference.py before any GPU
test relies on it): ``graph_refresh_reference.candidate_mask`` with the two further sources, and the counter hash in numpy uint32.

Dense form, as graph_refresh_reference.py: a row's candidate set is a bool mask [rows, N] over the keys of the row's own image."""
import functools

import numpy as np
import torch

from tests.graph_reference import _LEVELS, _geom

ADJACENT = ((0, -1), (0, 1), (-1, 0), (1, 0))        # (dqy, dqx) of the four adjacent queries


def lowbias32(x):
    """lowbias32 of a uint32 array (or scalar), in uint32 arithmetic."""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def explore_keys(n_rows, N, m, seed):
    """[n_rows, m] int64: key_t = (uint64(h_t) N) >> 32 with h_t = lowbias32(lowbias32(uint32(r) ^ uint32(seed)) + uint32(t))."""
    r = np.arange(n_rows, dtype=np.uint64).astype(np.uint32)
    h0 = lowbias32(r ^ np.uint32(seed & 0xFFFFFFFF))
    with np.errstate(over="ignore"):
        h = lowbias32(h0[:, None] + np.arange(m, dtype=np.uint32)[None, :])
    key = (h.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)
    return torch.from_numpy(key.astype(np.int64)).reshape(n_rows, m)


def _windows(mask, rows, cy, cx, H, W, radius):
    """mask[r, cell] = True for every cell of the (2 radius + 1)^2 window around (cy, cx) that lies on the map -- clipped cell by cell,
    the centre itself may lie off it."""
    d = torch.arange(-radius, radius + 1)
    ny = (cy.view(-1, 1, 1) + d.view(1, -1, 1)).expand(-1, -1, d.numel())
    nx = (cx.view(-1, 1, 1) + d.view(1, 1, -1)).expand(-1, d.numel(), -1)
    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
    mask[rows.view(-1, 1, 1).expand_as(ny)[inside], (ny * W + nx)[inside]] = True


def candidate_mask(row_off, key, B, H, W, radius, propagate=False, explore=0, seed=0):
    """[B L, N] bool, the union of
    (a) the windows, clipped at the map border, around every edge of the row whose key is in [0, N);
    (b) ``propagate``: for (dqy, dqx) in ADJACENT with (qy + dqy, qx + dqx) inside the Lh x Lw query grid of the same image, the windows
        around (y - 4 dqy, x - 4 dqx) for every edge (y, x) of that adjacent row with key in [0, N);
    (c) ``explore`` keys of ``explore_keys`` (no window)."""
    N = H * W
    Lh, Lw = -(-H // 4), -(-W // 4)
    L = Lh * Lw
    n_rows = row_off.numel() - 1
    assert n_rows == B * L
    rows = torch.repeat_interleave(torch.arange(n_rows), row_off[1:] - row_off[:-1])
    key = key.long()
    valid = (key >= 0) & (key < N)
    rows, key = rows[valid], key[valid]
    y, x = torch.div(key, W, rounding_mode="floor"), key % W
    mask = torch.zeros(n_rows, N, dtype=torch.bool)
    _windows(mask, rows, y, x, H, W, radius)
    if propagate:
        q = rows % L
        qy, qx = torch.div(q, Lw, rounding_mode="floor"), q % Lw
        for dqy, dqx in ADJACENT:
            # the edges of the row at (qy, qx) reach the row at (qy - dqy, qx - dqx), whose adjacent row at (dqy, dqx) it is
            ty, tx = qy - dqy, qx - dqx
            ok = (ty >= 0) & (ty < Lh) & (tx >= 0) & (tx < Lw)
            target = rows - q + ty * Lw + tx
            _windows(mask, target[ok], (y - 4 * dqy)[ok], (x - 4 * dqx)[ok], H, W, radius)
    if explore:
        k = explore_keys(n_rows, N, explore, seed)
        mask[torch.arange(n_rows).view(-1, 1).expand_as(k), k] = True
    return mask


def emptied_rows(row_off, B, H, W, max_row_edges, propagate):
    """[B L] bool: the rows ``dagl_graph_search`` leaves empty and counts in status[0] -- the row's own degree, or with ``propagate`` the
    degree of an adjacent row, exceeds ``max_row_edges``."""
    Lh, Lw = -(-H // 4), -(-W // 4)
    over = ((row_off[1:] - row_off[:-1]) > max_row_edges).view(B, Lh, Lw)
    out = over.clone()
    if propagate:
        out[:, :, 1:] |= over[:, :, :-1]
        out[:, :, :-1] |= over[:, :, 1:]
        out[:, 1:, :] |= over[:, :-1, :]
        out[:, :-1, :] |= over[:, 1:, :]
    return out.reshape(-1)


# ---- the crafted graph and the banded features of test_gpu_graph_search.py (computed once per shape on the CPU, read-only) ---------------
SHAPES = [(2, 24, 20), (1, 33, 70)]
MAX_ROW = 12                                  # the declared max_row_edges
R_LONG = 7                                    # the row of exactly MAX_ROW distinct keys
R_FAIL = 9                                    # the row whose candidates all fail tau
FEATURE_SEARCH = dict(radius=1, propagate=True, explore=5, seed=21)      # the largest candidate sets the features are laid out for


@functools.lru_cache(maxsize=None)
def crafted(shape, seed=5):
    """(row_off, key) on the CPU, the graph of test_gpu_graph_refresh.py's ``_crafted``.  What the search sources meet on it: row 0 is
    empty and its right neighbour (row 1, the four corners of the map) has edges; rows Lw - 1 and Lw are the last query of a grid row
    and the first of the next, both with edges; row L - 1, the last row of image 0, holds five keys and -- in a batch of two --
    row L, the first of image 1, none; row 6 holds the keys -1 and N and is adjacent to rows 5 and 7; row 7 holds exactly MAX_ROW keys;
    rows 1 and 2 hold keys on the border, whose propagated centres fall off the map."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randint(0, N, (8,), generator=gen).tolist() for _ in range(B * L)]
    rows[0] = []
    rows[1] = [0, W - 1, (H - 1) * W, N - 1]
    rows[2] = [W // 2, (H - 1) * W + W // 2, (H // 2) * W, (H // 2) * W + W - 1]
    rows[3] = [5 * W + 5, 5 * W + 6]
    rows[4] = [7 * W + 7] * 3
    rows[5] = [N - 3, 10, 9 * W + 4, 2 * W + 15]
    rows[6] = [-1, N, 3 * W + 3]
    rows[R_LONG] = torch.randperm(N, generator=gen)[:MAX_ROW].tolist()
    rows[8] = [11 * W + 9]
    rows[R_FAIL] = [6 * W + 2, 15 * W + 11]
    rows[L - 1] = torch.randint(0, N, (5,), generator=gen).tolist()
    if B > 1:
        rows[L] = []
    row_off = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0)
    return row_off, torch.tensor([k for r in rows for k in r], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def features(shape, seed=7):
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU, banded as test_gpu_graph_refresh.py's: keys at five levels of a common
    random direction plus a tenth of noise, every third key row a BITWISE copy of its left neighbour (exact ties among the candidates
    of a window), each query row scaled so that its largest candidate score is 1.6; tau_r midway in the widest gap of the middle half
    of the row's sorted distinct candidate scores; row R_FAIL: above every score.  "Candidate" = FEATURE_SEARCH's sets, which hold
    those of every narrower call with the same seed."""
    row_off, key = crafted(shape)
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(196, generator=gen, dtype=torch.float64)
    level = _LEVELS[torch.randint(0, 5, (B, N), generator=gen)]
    x = level.unsqueeze(2) * (base + 0.1 * torch.rand(B, N, 196, generator=gen, dtype=torch.float64))
    twin = torch.arange(N)
    twin = twin[(twin % 3 == 1) & (twin % W != 0)]
    x[:, twin] = x[:, twin - 1]
    wq = torch.rand(B, L, 196, generator=gen, dtype=torch.float64)
    cand = candidate_mask(row_off, key, B, H, W, **FEATURE_SEARCH)
    S = torch.bmm(wq, x.transpose(1, 2)).reshape(B * L, N)
    smax = torch.where(cand, S, torch.zeros_like(S)).amax(dim=1)
    wq = wq * torch.where(smax > 0, 1.6 / smax.clamp(min=1e-30), torch.ones_like(smax)).view(B, L, 1)
    wq, x = wq.float(), x.float()
    S = torch.bmm(wq.double(), x.double().transpose(1, 2)).reshape(B * L, N)
    tau = torch.zeros(B * L, dtype=torch.float64)
    for r in range(B * L):
        s = torch.unique(S[r][cand[r]])
        if s.numel() == 1:
            tau[r] = s[0] / 2
        elif s.numel() >= 2:
            gaps = s[1:] - s[:-1]
            lo = gaps.numel() // 4
            hi = max(lo + 1, (3 * gaps.numel() + 3) // 4)
            j = lo + int(gaps[lo:hi].argmax())
            tau[r] = (s[j] + s[j + 1]) / 2
    tau[R_FAIL] = 100.0
    return wq, x, tau.float()


@functools.lru_cache(maxsize=None)
def dense_scores(shape, dtype):
    """[B L, N]: every pair's score on the CPU in ``dtype``."""
    wq, x, _ = features(shape)
    B, H, W, L, N = _geom(shape)
    torch.set_num_threads(16)
    return torch.bmm(wq.to(dtype), x.to(dtype).transpose(1, 2)).reshape(B * L, N)
