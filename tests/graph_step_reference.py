"""What the tests of ``ops.graph_step`` / ``CE.step_graph`` share (test_gpu_step_graph.py): the crafted graph and the banded features of
test_gpu_graph_refresh.py, restated here because no test module imports from another, a seeded value map, and the CPU references of the
step's output.  Everything is computed once per shape (``lru_cache``) on the CPU and read-only."""
import functools

import torch

from tests.graph_reference import _LEVELS, _dense_apply, _geom, _rows_of
from tests.graph_refresh_reference import candidate_mask
from tests.helpers import normwise

SHAPES = [(2, 24, 20), (1, 33, 70)]
MAX_ROW = 12                                  # the declared max_row_edges: 12 / 108 candidates at radius 0 / 1 (a wavefront per row), 300 at 2 (a block)
R_FAIL = 9                                    # the row whose candidates all fail tau
R_LONG = 7                                    # the row of exactly MAX_ROW distinct keys


@functools.lru_cache(maxsize=None)
def crafted(shape, seed=5):
    """(row_off, key) on the CPU.  Rows: 0 empty; 1 the four corners; 2 one key on each border; 3 two adjacent keys; 4 a key three times;
    5 unsorted keys; 6 a key of -1, one of N and a valid one; 7 exactly MAX_ROW distinct keys; 8 a single key; 9 a row whose candidates
    all fail tau; L - 1 (the last row of image 0) five keys, followed -- in a batch of two -- by an empty first row of image 1; every
    other row 8 keys drawn with replacement."""
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
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU: keys at five levels of a common random direction plus a tenth of noise,
    every third key row a BITWISE copy of its left neighbour (exact ties among the candidates of a window), each query row scaled so
    that its largest candidate score (radius 2) is 1.6; tau_r midway in the widest gap of the middle half of the row's sorted distinct
    candidate scores; row R_FAIL: above every score."""
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
    cand = candidate_mask(row_off, key, H, W, 2)
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
def value_map(shape, seed=9):
    """b2 [B,16,H,W] fp32 on the CPU: seeded randn."""
    B, H, W, L, N = _geom(shape)
    return torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(seed))


def apply_references(row_off, key, weight, shape):
    """(fp64, fp32) ``fold(A . V(b2)) / cnt`` of a CSR on the CPU over ``value_map(shape)``: the step's output written out densely."""
    b2 = value_map(shape)
    torch.set_num_threads(16)
    return _dense_apply(row_off, key, weight, b2.double(), shape), _dense_apply(row_off, key, weight, b2, shape)


def without_rows(row_off, key, weight, gone):
    """The CSR with the rows ``gone`` emptied."""
    rows = _rows_of(row_off)
    keep = ~torch.isin(rows, torch.tensor(sorted(gone)))
    deg = (row_off[1:] - row_off[:-1]).clone()
    deg[sorted(gone)] = 0
    return torch.cat([deg.new_zeros(1), deg.cumsum(0)]), key[keep], weight[keep]


def check_against(what, lib, other, ref64, ref32, slack=1e-6):
    """The project's bound with a second implementation in the place of the fp64 reference: ``|lib - other| <= 3 e_ref32 + slack``
    normwise, ``e_ref32`` the fp32 reference's own error against fp64."""
    e = normwise(lib.detach().double().cpu().numpy(), other.detach().double().cpu().numpy())
    e_32 = normwise(ref32.detach().double().numpy(), ref64.detach().numpy())
    print(f"[graph_step] {what}: e {e:.2e}, e_ref32 {e_32:.2e}, ratio {e / max(e_32, 1e-30):.2f}")
    assert e <= 3.0 * e_32 + slack, (what, e, e_32)
