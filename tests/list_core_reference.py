"""List-form reference of the graph core -- TEST INFRASTRUCTURE ONLY (plain torch on the CPU, any dtype).

``dagl_ce_core_backward`` is a pure function of (wq_rows, x_rows, b2, thr, bias, nb_idx, nb_wgt, nb_s, nb_cnt, mu, d_out): it never
selects a neighbour itself.  ``list_core_forward`` evaluates the same graph core from GIVEN neighbour lists, so a test can hand the
kernel any lists it likes (hubs, ragged counts, empty queries, image corners) with no selection discontinuity in the way, and
differentiate the evaluation with autograd in fp64.  ``tests/test_list_core_reference.py`` pins it to ``oracle.ce_oracle.ce_core_oracle``
on the oracle's own selection.

  S_t = <Wq_l, X_{j_t}>                       for the listed keys j_t, t < cnt_l (slots t >= cnt_l are ignored)
  adaptive modes:  mu_l = <Wq_l, mean_j X_j>,  m_t = S_t - mu_l thr_l + bias_l,  l_t = 10 S_t m_t   (no ReLU: a listed key IS active)
  top-k:           l_t = 10 S_t
  Z_l = sum_t exp(l_t) + (N - cnt_l)          (the keys that are not listed have logit 0 and stay in the denominator)
  A_t = exp(l_t) / Z_l,   agg_l = sum_t A_t V_{j_t},   out = fold(agg) / overlap count
"""
import torch
import torch.nn.functional as F

from oracle.ce_oracle import KSIZE, SOFTMAX_SCALE, STRIDE_Q, overlap_count
from tests.helpers import normwise

PATTERNS = ("random", "hub", "twin_hubs", "identical", "ragged", "empty", "corners")
GRAD_NAMES = ("d_wq_rows", "d_x_rows", "d_b2", "d_thr", "d_bias")


def query_count(H: int, W: int) -> int:
    return (-(-H // STRIDE_Q)) * (-(-W // STRIDE_Q))


def gather_value_rows(b2: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Rows ``key`` [B, ...] (int64, in [0, H*W)) of ``oracle.ce_oracle.patch_rows(b2, 7, 1)`` -- the 7x7 windows of the value map
    around the keys, element order (c, kh, kw), zeros outside the image -- read straight from the zero-padded map (the unfolded rows
    of a 256 x 256 map are 400 MB in fp64; the lists touch a few thousand of them)."""
    B, c, H, W = b2.shape
    pad = KSIZE // 2
    Hp, Wp = H + 2 * pad, W + 2 * pad
    flat = F.pad(b2, (pad, pad, pad, pad)).reshape(-1)
    ar = torch.arange(KSIZE)
    off = (torch.arange(c)[:, None, None] * (Hp * Wp) + ar[None, :, None] * Wp + ar[None, None, :]).reshape(-1)      # (c, kh, kw)
    jy, jx = key // W, key % W
    img = torch.arange(B).reshape([B] + [1] * (key.dim() - 1)) * (c * Hp * Wp)
    return flat[(img + jy * Wp + jx)[..., None] + off]


def list_core_forward(wq, x, b2, thr, bias, idx, cnt, mode: str, dtype=torch.float64):
    """wq [B,L,196], x [B,N,196], b2 [B,c,H,W], thr / bias [B,L] (unused by "topk"), idx [B,L,w] int64, cnt [B,L] ->
    (out [B,c,H,W], (S [B,L,w], A [B,L,w], mu [B,L] or None)); S and A are 0 in the ignored slots.  Everything in ``dtype``."""
    if mode not in ("topk", "adaptive", "adaptive_topk"):
        raise ValueError(mode)
    B, c, H, W = b2.shape
    N, L, w = H * W, wq.shape[1], idx.shape[2]
    assert tuple(idx.shape) == (B, L, w) and tuple(cnt.shape) == (B, L) and x.shape[1] == N and L == query_count(H, W)
    wq, x, b2 = wq.to(dtype), x.to(dtype), b2.to(dtype)
    valid = torch.arange(w)[None, None, :] < cnt[:, :, None]
    assert int(cnt.min()) >= 0 and int(cnt.max()) <= w and bool(((idx >= 0) & (idx < N))[valid].all())
    key = torch.where(valid, idx, torch.zeros_like(idx))
    vf = valid.to(dtype)
    xg = x.reshape(B * N, -1)[key + torch.arange(B)[:, None, None] * N]                       # [B,L,w,196]
    S = (wq[:, :, None, :] * xg).sum(dim=3) * vf
    mu = None
    if mode == "topk":
        logit = SOFTMAX_SCALE * S
    else:
        mu = (wq * x.mean(dim=1, keepdim=True)).sum(dim=2)
        m = S - (mu * thr.to(dtype))[:, :, None] + bias.to(dtype)[:, :, None]
        logit = SOFTMAX_SCALE * S * m
    e = torch.exp(logit) * vf
    Z = e.sum(dim=2) + (N - cnt).to(dtype)
    A = e / Z[:, :, None]
    agg = (A[..., None] * gather_value_rows(b2, key)).sum(dim=2)                              # [B,L,784]
    out = F.fold(agg.transpose(1, 2), (H, W), (KSIZE, KSIZE), padding=KSIZE // 2, stride=STRIDE_Q)
    ov = overlap_count(H, W, dtype)
    out = out / (ov + (ov == 0).to(dtype))
    return out, (S, A, mu)


def list_core_grads(inputs, idx, cnt, G, mode: str, dtype=torch.float64):
    """autograd of ``(out * G).sum()`` through ``list_core_forward`` -> dict(out, S, A, mu, d_wq_rows, d_x_rows, d_b2 and, in the
    adaptive modes, d_thr, d_bias), all detached, in ``dtype``."""
    n_in = 3 if mode == "topk" else 5
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in inputs[:n_in]]
    args = leaves + [None] * (5 - n_in)
    out, (S, A, mu) = list_core_forward(*args, idx, cnt, mode, dtype)
    grads = torch.autograd.grad((out * G.to(dtype)).sum(), leaves)
    res = dict(out=out.detach(), S=S.detach(), A=A.detach(), mu=None if mu is None else mu.detach())
    res.update(zip(GRAD_NAMES, grads))
    return res


def make_inputs(B: int, H: int, W: int, seed: int):
    """(wq_rows, x_rows, b2, thr, bias), G in fp32: feature rows rand * 0.1 as in the core tests of test_gpu_backward.py."""
    g = torch.Generator().manual_seed(seed)
    L, N = query_count(H, W), H * W
    wq = torch.rand(B, L, 196, generator=g) * 0.1
    x = torch.rand(B, N, 196, generator=g) * 0.1
    b2 = torch.randn(B, 16, H, W, generator=g)
    G = torch.randn(B, 16, H, W, generator=g)
    thr = 1.0 + 0.02 * torch.randn(B, L, generator=g)
    bias = 0.05 * torch.rand(B, L, generator=g)
    return (wq, x, b2, thr, bias), G


def _distinct_keys(g, B, L, n, N, reserved=()):
    """[B,L,n] keys, distinct inside a row, uniform over [0,N) without the ``reserved`` keys."""
    M = N - len(reserved)
    assert 0 <= n <= M
    if n == 0:
        return torch.zeros(B, L, 0, dtype=torch.int64)
    if M <= 4096:
        keys = torch.rand(B, L, M, generator=g).argsort(dim=2)[:, :, :n]
    else:                                           # few keys out of many: draw, and draw the rows with a repeat again
        keys = torch.randint(0, M, (B, L, n), generator=g)
        while True:
            s = keys.sort(dim=2).values
            bad = (s[:, :, 1:] == s[:, :, :-1]).any(dim=2)
            if not bool(bad.any()):
                break
            keys[bad] = torch.randint(0, M, (int(bad.sum()), n), generator=g)
    for r in sorted(reserved):                      # step over the reserved keys, lowest first
        keys = keys + (keys >= r).to(keys.dtype)
    return keys


def make_lists(pattern: str, B: int, H: int, W: int, width: int, seed: int):
    """Neighbour lists, deterministic in ``seed`` -> (idx [B,L,width] int64, cnt [B,L] int64).  The used slots of a row hold distinct
    keys in [0,N); a row uses at most n = min(width, N) slots.  Unused slots hold a VALID wrong key (the hub's): code that reads them
    adds to the hub's sums instead of leaving the arrays.
      random     n distinct random keys per query
      hub        slot 0 of every query is one key (in-degree L per image), the rest random
      twin_hubs  keys h and h+1 are in every list: two long runs adjacent in sorted order
      identical  every query lists the keys 0..n-1: every run has length L
      ragged     the hub lists cut to cnt uniform in 0..n, at least one query with 0 and one with n
      empty      cnt = 0 everywhere
      corners    the keys 0, W-1, N-W, N-1 in slots 0 and 1, two per list in turn (so with B > 1 the last key of image b and the
                 first of image b+1 are neighbours in sorted order), the rest random"""
    if pattern not in PATTERNS:
        raise ValueError(pattern)
    g = torch.Generator().manual_seed(seed)
    L, N = query_count(H, W), H * W
    n = min(width, N)
    hub = min((H // 2) * W + W // 2, max(N - 2, 0))
    idx = torch.full((B, L, width), hub, dtype=torch.int64)
    cnt = torch.full((B, L), n, dtype=torch.int64)
    if pattern == "random":
        idx[:, :, :n] = _distinct_keys(g, B, L, n, N)
    elif pattern in ("hub", "ragged"):
        idx[:, :, 1:n] = _distinct_keys(g, B, L, n - 1, N, (hub,))
        if pattern == "ragged":
            cnt = torch.randint(0, n + 1, (B, L), generator=g)
            cnt.reshape(-1)[0], cnt.reshape(-1)[-1] = 0, n
            idx[torch.arange(width)[None, None, :] >= cnt[:, :, None]] = hub
    elif pattern == "twin_hubs":
        assert n >= 2
        idx[:, :, 1] = hub + 1
        idx[:, :, 2:n] = _distinct_keys(g, B, L, n - 2, N, (hub, hub + 1))
    elif pattern == "identical":
        idx[:, :, :n] = torch.arange(n)
    elif pattern == "empty":
        cnt = torch.zeros(B, L, dtype=torch.int64)
    else:
        corners = (0, W - 1, N - W, N - 1)
        assert n >= 2 and len(set(corners)) == 4
        n = min(n, N - 2)                           # (a list holds two of the four corners and none of the other two)
        cnt = torch.full((B, L), n, dtype=torch.int64)
        turn = torch.arange(L) % 4
        idx[:, :, 0] = torch.tensor(corners)[turn]
        idx[:, :, 1] = torch.tensor(corners)[(turn + 2) % 4]
        idx[:, :, 2:n] = _distinct_keys(g, B, L, n - 2, N, corners)
    return idx, cnt


def bound(e_ref: float) -> float:
    """How far from fp64 a kernel's gradient may sit when the fp32 evaluation of the same reference sits ``e_ref`` away:
    4 e_ref + 2e-6, and never beyond 1e-5.  4: the kernel adds a hub's L terms one after the other through chunk partials where torch
    adds pairwise; 2e-6: what test_gpu_gemm.py grants an fp32 product chain; 1e-5: two orders under what one misplaced edge costs
    (tests/test_list_core_reference.py).  It needs well-conditioned lists: a weight A within 1e-5 of 1 leaves d l = A (d A - sum A d A)
    to a cancellation that fp32 carries to 1e-2 at best."""
    return min(4.0 * e_ref + 2e-6, 1e-5)


def check_against_fp64(tag: str, names, got, ref64: dict, ref32: dict, zero_below: float = 0.0):
    """The tolerance rule per tensor, normwise; prints one [parity] line each.  ``zero_below``: for the caller whose case makes a tensor
    exactly zero (one key, cnt = N = 1: A = 1 and the softmax has no derivative) while fp64 autograd returns rounding noise of 1e-15
    and less for it -- a reference below this magnitude IS zero, and normwise then measures the absolute error."""
    bad = []
    for name, g in zip(names, got):
        want = ref64[name].numpy()
        if abs(want).max() < zero_below:
            want = 0.0 * want
        e_hip = normwise(g.detach().cpu().numpy(), want)
        e_ref = normwise(ref32[name].numpy(), want)
        print(f"[parity] {tag} {name}: e_hip {e_hip:.2e}  e_ref {e_ref:.2e}  bound {bound(e_ref):.2e}")
        if not e_hip <= bound(e_ref):
            bad.append((name, e_hip, e_ref))
    assert not bad, (tag, bad)
