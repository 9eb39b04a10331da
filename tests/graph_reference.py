"""What the tests of the patch-graph routes share (test_gpu_patch_graph.py, test_gpu_graph_apply.py, test_gpu_graph_attend.py,
test_gpu_graph_forward.py, test_gpu_forward_with_graph.py, test_gpu_refresh_graph.py, test_gpu_graph_refresh.py): the tables of shapes and
cases, the seeded inputs, modules and fp64 oracle stages (computed once per case, read-only), the rounding band of the edge set and the
``check_*`` functions of an exported graph, the crafted graphs, and the fp64 references of the apply and attend formulas.  No test
module imports from another: what two of them need lives here."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import normwise

DEV = "cuda:0"

TAU = 2e-5
SHAPES = [(2, 24, 20),      # N = 480, not a multiple of 256; L = 30; offsets cross an image boundary
          (1, 33, 70),      # odd sizes
          (2, 45, 45),      # unscreened size; degrees past 256 and 1024
          (1, 64, 64)]      # screened size; N = 4096, several block strides per row
# (variant, sparse_gain, mode, k)
CASES = [("default", 2.0, "adaptive", 0), ("sparse", 1.65, "adaptive", 0), ("sparse", 1.2, "adaptive", 0),
         ("allpass", 2.0, "adaptive", 0), ("nonepass", 2.0, "adaptive", 0),
         ("default", 2.0, "topk", 8), ("default", 2.0, "topk", 64), ("default", 2.0, "topk", 100), ("default", 2.0, "topk", 5000),
         ("sparse", 1.2, "adaptive_topk", 16), ("sparse", 1.2, "adaptive_topk", 100)]
SEEDS = (11, 12, 13)


def _seed(shape, case):
    return SEEDS[(SHAPES.index(shape) + CASES.index(case)) % 3]


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _inputs(seed, shape, variant, gain, in_channels=64):
    from dagl_amd.synth import make_ce_params, make_features
    B, H, W = shape
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(seed, in_channels=in_channels, variant=variant, sparse_gain=gain).items()}
    return torch.from_numpy(make_features(seed, B, in_channels, H, W)), prm


def _dense_a(st, mode, scale=10.0):
    """A = softmax(scale S m) mask_b of ``_graph_core`` from an oracle's stages, in their precision: [B, L, N]."""
    S, mb = st["S"], st["mask_b"]
    if mode == "topk":
        m = mb
    else:
        m = F.relu(S - S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2) + st["bias"].unsqueeze(2)) * mb
    return F.softmax(S * m * scale, dim=2) * mb


@functools.lru_cache(maxsize=None)
def _oracle(seed, shape, variant, gain, mode, k, dtype=torch.float64, in_channels=64, scale=10.0):
    """The oracle's stages + A, computed once per case and shared (read-only) by the tests."""
    from oracle.ce_oracle import ce_forward_oracle
    x, prm = _inputs(seed, shape, variant, gain, in_channels)
    torch.set_num_threads(16)
    with torch.no_grad():
        out, st = ce_forward_oracle(x, prm, mode=mode, k=k if mode != "adaptive" else None, dtype=dtype, stages=True,
                                    softmax_scale=scale)
        st = {n: st[n] for n in ("S", "thr", "bias", "mask_b", "b2", "cnt")}
        st["A"] = _dense_a(st, mode, scale)
    return st


def _module(seed, shape, variant, gain, mode, k, in_channels=64, half=False, scale=10):
    from dagl_amd.ce import CE
    x, prm = _inputs(seed, shape, variant, gain, in_channels)
    ce = CE(in_channels=in_channels, softmax_scale=scale)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode = mode
    if mode != "adaptive":
        ce.select_k = k
    ce = ce.to("cuda:0").eval()
    x = x.to("cuda:0")
    if half:
        ce, x = ce.half(), x.half()
    return ce, x


def ambiguity(st, mode, k):
    """(threshold-ambiguous, rank-ambiguous) [B, L, N] bool from the fp64 oracle's stages."""
    S = st["S"]
    N = S.shape[2]
    thr_amb = torch.zeros_like(S, dtype=torch.bool)
    if mode != "topk":
        mt = S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2)
        bs = st["bias"].unsqueeze(2).expand_as(S)
        thr_amb = (S - mt + bs).abs() < TAU * (S.abs() + mt.abs() + bs.abs())
    rank_amb = torch.zeros_like(S, dtype=torch.bool)
    if mode != "adaptive" and k < N:
        rankable = torch.ones_like(S, dtype=torch.bool)
        if mode == "adaptive_topk":
            rankable = F.relu(S - mt + bs) != 0
        top = torch.where(rankable, S, torch.full_like(S, -1.0)).topk(k + 1, dim=2).values
        sk, sk1 = top[..., k - 1:k], top[..., k:k + 1]                 # (-1: the row has fewer rankable keys -- nothing to rank)
        close = (sk1 >= 0) & ((sk - sk1) < TAU * sk)
        rank_amb = close & (S >= sk1 * (1 - TAU)) & (S <= sk * (1 + TAU)) & (rankable | thr_amb)
    return thr_amb, rank_amb


def membership(g):
    """[B, L, N] bool from a PatchGraph (on the CPU)."""
    deg = g.degrees().reshape(-1)
    rows = torch.repeat_interleave(torch.arange(g.B * g.L), deg)
    m = torch.zeros(g.B * g.L, g.N, dtype=torch.bool)
    m[rows, g.key.long()] = True
    return m.view(g.B, g.L, g.N), rows


def check_structure(g, mode, k, variant):
    off, key = g.row_off, g.key.long()
    assert off.dtype == torch.int64 and g.key.dtype == torch.int32 and g.weight.dtype == torch.float32
    assert off.numel() == g.B * g.L + 1 and int(off[0]) == 0 and bool((off[1:] >= off[:-1]).all()) and int(off[-1]) == key.numel()
    assert key.numel() == 0 or (int(key.min()) >= 0 and int(key.max()) < g.N)
    rows = torch.repeat_interleave(torch.arange(g.B * g.L), g.degrees().reshape(-1))
    same_row = rows[1:] == rows[:-1]
    assert bool((key[1:] > key[:-1])[same_row].all()), "keys must ascend strictly inside a row"
    if mode == "topk":
        assert bool((g.degrees() == min(k, g.N)).all())
    if variant == "nonepass":
        assert key.numel() == 0
    if (variant == "allpass" and mode == "adaptive") or (mode == "topk" and k >= g.N):
        assert bool((g.degrees() == g.N).all()) and torch.equal(key, torch.arange(g.N).repeat(g.B * g.L))


def check_edges(g, st, mode, k):
    """Membership against the oracle outside the band; returns (lib membership, rows of its edges, rows holding a rank-ambiguous pair)."""
    mem, rows = membership(g)
    thr_amb, rank_amb = ambiguity(st, mode, k)
    amb = thr_amb | rank_amb
    want = st["mask_b"] != 0
    wrong = (mem != want) & ~amb
    share, rank_rows = float(amb.double().mean()), rank_amb.any(dim=2)
    print(f"[graph] edges {g.n_edges}, degree mean {float(g.degrees().double().mean()):.1f} max {int(g.degrees().max())}; ambiguous pairs "
          f"{int(amb.sum())} ({share:.1e} of all), of them on the other side {int(((mem != want) & amb).sum())}; rows with a rank-ambiguous "
          f"pair {int(rank_rows.sum())} of {rank_rows.numel()}; wrong outside the band {int(wrong.sum())}")
    assert share <= 5e-4, "the band must not hide a failure: too many ambiguous pairs"
    assert float(rank_rows.double().mean()) <= 0.10, "the band must not hide a failure: too many rows with a rank-ambiguous pair"
    assert int(wrong.sum()) == 0
    return mem, rows, rank_rows


def check_values(g, mem, rows, rank_rows, st64, st32, mode, what):
    """Weights and scores over the edges both sides have, against the reference in its own precision (the bound of test_gpu_trunk)."""
    keep_row = ~rank_rows if mode != "adaptive" else torch.ones_like(rank_rows)
    want = st64["mask_b"] != 0
    common_lib = want.view(-1, g.N)[rows, g.key.long()] & keep_row.view(-1)[rows]            # per lib edge
    common_32 = (st32["mask_b"] != 0) & want & keep_row.unsqueeze(2)
    if int(common_lib.sum()) == 0 or int(common_32.sum()) == 0:          # (an empty graph: check_edges has compared the sets)
        print(f"[graph] {what}: no common edges to compare values on")
        return
    for name, lib, ref in (("weight", g.weight, "A"), ("score", g.score, "S")):
        r64 = st64[ref].view(-1, g.N)
        e_lib = normwise(lib[common_lib].numpy(), r64[rows, g.key.long()][common_lib].numpy())
        e_32 = normwise(st32[ref][common_32].numpy(), st64[ref][common_32].numpy())
        print(f"[graph] {what} {name}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, ratio {e_lib / max(e_32, 1e-30):.2f}")
        assert e_lib <= 3.0 * e_32 + 1e-6, (what, name, e_lib, e_32)


def _fold(agg, cnt, H, W):
    """[B, L, 784] aggregated rows (c, kh, kw) -> [B, 16, H, W], dagl.py:265-272."""
    z = F.fold(agg.transpose(1, 2), (H, W), (7, 7), padding=3, stride=4)
    return z / cnt


def _same_forward_after(ce, x, refused):
    from dagl_amd import DaglError
    with torch.no_grad():
        before = ce(x).clone()
    with pytest.raises(DaglError) as err:
        refused()
    with torch.no_grad():
        assert torch.equal(ce(x), before)
    return str(err.value)


def _seg():
    from dagl_amd import ops
    return ops.graph_apply_segment()


def _geom(shape):
    B, H, W = shape
    return B, H, W, (-(-H // 4)) * (-(-W // 4)), H * W


@functools.lru_cache(maxsize=None)
def _crafted(shape, seed=5):
    """(row_off, key, weight, b2) on the CPU: rows of degree 0, 1, SEG-1, SEG, SEG+1, 2 SEG+3, N (every key once), N+5 (more edges than
    keys), a row of 3 SEG+1 edges as the LAST row of image 0 -- followed, in a batch of two, by an empty first row of image 1 -- and 8
    everywhere else; keys drawn with replacement (unsorted, repeating), the four corners of the map in one row, signed weights."""
    B, H, W, L, N = _geom(shape)
    seg = _seg()
    gen = torch.Generator().manual_seed(seed)
    deg = [8] * (B * L)
    for r, d in enumerate((0, 1, seg - 1, seg, seg + 1, 2 * seg + 3, N, N + 5)):
        deg[r] = d
    deg[L - 1] = 3 * seg + 1
    if B > 1:
        deg[L] = 0
    keys = []
    for r, d in enumerate(deg):
        k = torch.randperm(N, generator=gen) if r == 6 else torch.randint(0, N, (d,), generator=gen)
        if r == 8:
            k[:4] = torch.tensor([0, W - 1, (H - 1) * W, N - 1])
        keys.append(k)
    key = torch.cat(keys).int()
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(deg, dtype=torch.int64).cumsum(0)])
    weight = torch.randn(key.numel(), generator=gen)
    b2 = torch.randn(B, 16, H, W, generator=gen)
    return row_off, key, weight, b2


KSHAPES = [(1, 8, 8),        # L = 4, N = 64: the long row holds more edges than there are keys
           (2, 20, 36),      # L = 45, N = 720, two images: empty rows on both sides of the image boundary
           (1, 45, 45)]      # odd sizes, L = 144, N = 2025


@functools.lru_cache(maxsize=None)
def _graph(shape, seed=5):
    """(row_off, key, b2) on the CPU.  Per image: an empty first row, a row of 3 SEG + 1 edges (it crosses at least three segments; at
    8x8 it is also the row with more edges than keys), short rows of 1 .. 5 edges that share a segment, a row of N + 5 edges (every key
    once and five repeats) where the image has rows to spare, 8 edges elsewhere, an empty last row -- so the first and the last row of
    the array are empty and, in a batch of two, two empty rows meet at the image boundary.  Keys are drawn with replacement: unsorted,
    repeating.  (An 8x8 map has four query rows: empty, long, one short row that shares the long row's last segment, empty.)"""
    B, H, W, L, N = _geom(shape)
    seg = _seg()
    gen = torch.Generator().manual_seed(seed)
    deg = []
    for b in range(B):
        d = [8] * L
        d[0] = d[L - 1] = 0
        d[1] = 3 * seg + 1
        for r, n in zip(range(2, L - 1), (3, 1, 5, 2, 3, 4)):
            d[r] = n
        if L > 12:
            d[9] = N + 5
        deg += d
    keys = []
    for r, d in enumerate(deg):
        if d == N + 5:
            k = torch.cat([torch.randperm(N, generator=gen), torch.randint(0, N, (5,), generator=gen)])
        else:
            k = torch.randint(0, N, (d,), generator=gen)
        keys.append(k)
    key = torch.cat(keys).int()
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(deg, dtype=torch.int64).cumsum(0)])
    b2 = torch.randn(B, 16, H, W, generator=gen)
    return row_off, key, b2


def _dense_apply(row_off, key, weight, b2, shape):
    """fold(A_G . V(b2)) / cnt in the dtype of ``b2`` (differentiable in ``weight`` and ``b2``)."""
    from oracle.ce_oracle import overlap_count, patch_rows
    B, H, W, L, N = _geom(shape)
    rows = torch.repeat_interleave(torch.arange(B * L), row_off[1:] - row_off[:-1])
    a = torch.zeros(B * L, N, dtype=b2.dtype).index_put((rows, key.long()), weight.to(b2.dtype), accumulate=True)
    agg = torch.bmm(a.view(B, L, N), patch_rows(b2, 7, 1))
    return _fold(agg, overlap_count(H, W, b2.dtype), H, W)


def _padded(b2):
    return F.pad(b2.permute(0, 2, 3, 1), (0, 0, 3, 3, 3, 3)).contiguous()


def _gap(st, mode, k, H, W):
    """The k-th / (k+1)-th relative gap rule of ``test_graph_reproduces_the_block`` (restated)."""
    if mode == "adaptive" or k >= H * W:
        return 1.0
    S = st["S"]
    if mode == "adaptive_topk":
        passing = F.relu(S - S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2) + st["bias"].unsqueeze(2)) != 0
        S = torch.where(passing, S, torch.full_like(S, -1.0))
    top = S.topk(k + 1, dim=2).values
    ok = top[..., k] > 0
    rel = (top[..., k - 1] - top[..., k]) / top[..., k - 1].clamp(min=1e-30)
    return float(torch.where(ok, rel, torch.ones_like(rel)).min())


def _state(ce):
    return {n: t.clone() for n, t in ce.state_dict().items()}, ce._pack_key, ce._pack_epoch


def _refused(ce, x, call, word):
    before = _state(ce)
    msg = _same_forward_after(ce, x, call)
    after = _state(ce)
    assert word in msg, msg
    assert all(torch.equal(before[0][n], after[0][n]) for n in before[0])
    return msg

SCALE = 10.0

_LEVELS = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5], dtype=torch.float64)


def _rows_of(row_off):
    return torch.repeat_interleave(torch.arange(row_off.numel() - 1), row_off[1:] - row_off[:-1])


def _edge_scores(wq, x, rows, key, L, N):
    """S_e out of the dense product [B L, N]."""
    B = wq.shape[0]
    S = torch.bmm(wq, x.transpose(1, 2)).reshape(B * L, N)
    return S[rows, key.long()]


def _edge_reference(wq, x, row_off, key, tau, normalize, shape, scale=SCALE):
    """(weight [E], score [E], logits [E]) in the dtype of ``wq``, differentiable in wq, x, tau."""
    B, H, W, L, N = _geom(shape)
    deg = row_off[1:] - row_off[:-1]
    rows = _rows_of(row_off)
    S = _edge_scores(wq, x, rows, key, L, N)
    if tau is not None:
        m = F.relu(S - tau.reshape(-1)[rows])
        z, on = S * m * scale, m != 0
    else:
        z, on = S * scale, torch.ones_like(S, dtype=torch.bool)
    pos = torch.arange(key.numel()) - row_off[rows]
    Z = torch.full((B * L, max(int(deg.max()), 1)), float("-inf"), dtype=wq.dtype).index_put((rows, pos), z)
    off = (N - deg).clamp(min=0) if normalize == "reference" else torch.zeros_like(deg)
    M = Z.detach().max(dim=1).values
    M = torch.where(off > 0, M.clamp(min=0.0), M)
    M = torch.where(deg > 0, M, torch.zeros_like(M))
    D = torch.exp(Z - M.unsqueeze(1)).sum(dim=1) + off.to(wq.dtype) * torch.exp(-M)
    return on.to(wq.dtype) * torch.exp(z - M[rows]) / D[rows], S, z


def _level_features(row_off, key, shape, seed=7):
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU for a graph of ``shape``: non-negative random rows -- the keys at
    five levels 0.5 .. 1.5 of a common random direction plus a tenth of noise, so that a row's scores come in separated bands --, each
    query row scaled so that its largest score is 1.6; tau_r midway between the two adjacent sorted (distinct) scores of the row with the
    widest gap in the middle half of the sorted list (a single score: half of it)."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(196, generator=gen, dtype=torch.float64)
    level = _LEVELS[torch.randint(0, 5, (B, N), generator=gen)]
    x = level.unsqueeze(2) * (base + 0.1 * torch.rand(B, N, 196, generator=gen, dtype=torch.float64))
    wq = torch.rand(B, L, 196, generator=gen, dtype=torch.float64)
    rows = _rows_of(row_off)
    smax = torch.zeros(B * L, dtype=torch.float64).scatter_reduce(0, rows, _edge_scores(wq, x, rows, key, L, N), "amax")
    wq = wq * torch.where(smax > 0, 1.6 / smax.clamp(min=1e-30), torch.ones_like(smax)).view(B, L, 1)
    wq, x = wq.float(), x.float()
    S = _edge_scores(wq.double(), x.double(), rows, key, L, N)
    tau = torch.zeros(B * L, dtype=torch.float64)
    for r in range(B * L):
        s = torch.unique(S[int(row_off[r]):int(row_off[r + 1])])          # sorted
        if s.numel() == 1:
            tau[r] = s[0] / 2
        elif s.numel() >= 2:
            gaps = s[1:] - s[:-1]
            lo = gaps.numel() // 4
            hi = max(lo + 1, (3 * gaps.numel() + 3) // 4)
            j = lo + int(gaps[lo:hi].argmax())
            tau[r] = (s[j] + s[j + 1]) / 2
    return wq, x, tau.float()


def _check(what, lib, ref64, ref32, slack=1e-6):
    e_lib = normwise(lib.detach().double().cpu().numpy(), ref64.detach().numpy())
    e_32 = normwise(ref32.detach().double().numpy(), ref64.detach().numpy())
    print(f"[graph_attend] {what}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, ratio {e_lib / max(e_32, 1e-30):.2f}")
    assert e_lib <= 3.0 * e_32 + slack, (what, e_lib, e_32)


def _band(st64, g, mode, k):
    """[E] bool: the edges of ``g`` (on the CPU) inside the threshold band of ``ambiguity``."""
    thr_amb, _ = ambiguity(st64, mode, k)
    return thr_amb.view(-1, g.N)[g.rows(), g.key.long()]


def _on_edges(st, name, g):
    return st[name].reshape(-1, g.N)[g.rows(), g.key.long()]


def _dense_on_structure(x, prm, member, margin, shape, scale=SCALE):
    """The block's output with its weights recomputed on a structure given as a [B, L, N] 0/1 mask: dagl.py:208-272 with the mask in the
    place of the selection, in the dtype of ``x`` (differentiable in ``x`` and ``prm``)."""
    from oracle.ce_oracle import overlap_count, patch_rows, same_pad
    B, H, W, L, N = _geom(shape)
    b1 = F.conv2d(x, prm["g.weight"], prm["g.bias"], padding=1)
    b2 = F.conv2d(x, prm["theta.weight"], prm["theta.bias"])
    wq = F.relu(F.linear(patch_rows(b1, 7, 4), prm["fc1.0.weight"], prm["fc1.0.bias"]))
    xk = F.relu(F.linear(patch_rows(b1, 7, 1), prm["fc2.0.weight"], prm["fc2.0.bias"]))
    S = torch.bmm(wq, xk.transpose(1, 2))
    m = member.to(x.dtype)
    if margin:
        xq, _ = same_pad(x, 7, 4)
        thr = F.conv2d(xq, prm["thr_conv.weight"], prm["thr_conv.bias"], stride=4).reshape(B, -1)
        bias = F.conv2d(xq, prm["bias_conv.weight"], prm["bias_conv.bias"], stride=4).reshape(B, -1)
        m = F.relu(S - (S.mean(dim=2) * thr - bias).unsqueeze(2)) * m
    A = F.softmax(S * m * scale, dim=2) * (m != 0).to(x.dtype)
    return _fold(torch.bmm(A, patch_rows(b2, 7, 1)), overlap_count(H, W, x.dtype), H, W)

_GRAD_NAMES = ("g.weight", "g.bias", "theta.weight", "theta.bias", "fc1.0.weight", "fc1.0.bias", "fc2.0.weight", "fc2.0.bias",
               "thr_conv.weight", "thr_conv.bias", "bias_conv.weight", "bias_conv.bias")

S0, S1, S2 = (2, 24, 20), (1, 33, 70), (1, 64, 64)
TOPK8, TOPK64, ATOPK16 = ("default", 2.0, "topk", 8), ("default", 2.0, "topk", 64), ("sparse", 1.2, "adaptive_topk", 16)
# (shape, (variant, sparse_gain, mode, k), seed)
COMBOS = [(s, c, _seed(s, c)) for c in (TOPK8, TOPK64, ATOPK16) for s in (S0, S1, S2)] + [
    (S0, ("sparse", 1.65, "adaptive", 0), 12),        # oracle: max degree 59, 21 empty rows of 60
    (S1, ("sparse", 2.0, "adaptive", 0), 11),         # max degree 31, 143 empty rows of 162
    (S2, ("sparse", 2.0, "adaptive", 0), 11),         # max degree 10
    (S0, ("nonepass", 2.0, "adaptive", 0), 11)]       # the empty graph


def _cid(combo):
    shape, case, seed = combo
    return "x".join(map(str, shape)) + "-" + "-".join(map(str, case)) + f"-s{seed}"


def _mod(combo, **kw):
    shape, (variant, gain, mode, k), seed = combo
    return _module(seed, shape, variant, gain, mode, k, **kw)
