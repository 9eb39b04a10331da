"""Pins the checker of tests/test_gpu_list_backward.py (tests/list_core_reference.py): on the oracle's own selection the list form
IS the oracle, to fp64 rounding; one misplaced hub edge moves its gradients by orders more than the GPU tolerance; the list maker
keeps its promises (keys in range, no repeats, the advertised degenerate counts)."""
import pytest
import torch

from oracle.ce_oracle import ce_core_oracle, patch_rows
from tests.helpers import normwise
from tests.list_core_reference import (GRAD_NAMES, PATTERNS, gather_value_rows, list_core_grads, make_inputs, make_lists,
                                       query_count)


def _oracle_lists(wq, x, thr, bias, mode, k):
    """The oracle's own neighbour sets as lists: stable descending sort of the fp64 scores, the k best (top-k modes), cut at the
    adaptive mask's degree (adaptive modes)."""
    S = torch.einsum("bld,bnd->bln", wq.double(), x.double())
    order = S.sort(dim=2, descending=True, stable=True).indices
    B, L, N = S.shape
    if mode == "topk":
        cnt = torch.full((B, L), min(k, N), dtype=torch.int64)
    else:
        m = S - S.mean(dim=2, keepdim=True) * thr.double()[:, :, None] + bias.double()[:, :, None]
        cnt = (m > 0).sum(dim=2)
        if mode == "adaptive_topk":
            cnt = cnt.clamp(max=k)
    return order[:, :, :int(cnt.max())].contiguous(), cnt


@pytest.mark.parametrize("mode,k", [("topk", 5), ("adaptive", None), ("adaptive_topk", 6)])
def test_list_form_equals_the_oracle_on_the_oracles_own_selection(mode, k):
    B, H, W = 2, 24, 28
    (wq, x, b2, thr, _), G = make_inputs(B, H, W, seed=8)
    # every query's threshold in the middle of its widest score gap (degrees 3..30), as test_finite_difference_of_the_core_op
    # places them: T = mu thr - bias
    S = torch.einsum("bld,bnd->bln", wq.double(), x.double())
    v = S.sort(dim=2, descending=True).values
    d = (v[:, :, 2:30] - v[:, :, 3:31]).argmax(dim=2, keepdim=True) + 3
    T = 0.5 * (v.gather(2, d - 1) + v.gather(2, d)).squeeze(2)
    thr, bias = thr.double(), S.mean(dim=2) * thr.double() - T
    inputs = (wq.double(), x.double(), b2.double(), thr, bias)
    idx, cnt = _oracle_lists(wq, x, thr, bias, mode, k)
    if mode != "topk":
        assert torch.equal(cnt, d.squeeze(2).clamp(max=k) if k else d.squeeze(2))
    got = list_core_grads(inputs, idx, cnt, G, mode)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    ref = ce_core_oracle(*leaves, mode=mode, k=k)
    (ref * G.double()).sum().backward()
    assert normwise(got["out"].numpy(), ref.detach().numpy()) <= 1e-12
    for name, leaf in zip(GRAD_NAMES, leaves[:3 if mode == "topk" else 5]):
        e = normwise(got[name].numpy(), leaf.grad.numpy())
        print(f"[list-vs-oracle] {mode} {name}: {e:.2e}")
        assert e <= 1e-12, (mode, name, e)


def test_gathered_value_rows_are_the_unfolded_rows():
    g = torch.Generator().manual_seed(3)
    b2 = torch.randn(2, 16, 9, 11, generator=g, dtype=torch.float64)
    key = torch.arange(99).repeat(2, 1)
    assert torch.equal(gather_value_rows(b2, key), patch_rows(b2, 7, 1))


def test_one_misplaced_hub_edge_moves_the_gradients():
    """What the GPU tolerance (never above 1e-5) rests on: ONE of the hub's 256 edges moved to another key shifts d_x_rows and d_b2
    by more than 1e-3 normwise."""
    B, H, W, k = 1, 64, 64, 8
    inputs, G = make_inputs(B, H, W, seed=64)
    idx, cnt = make_lists("hub", B, H, W, k, seed=64)
    hub = int(idx[0, 0, 0])
    assert bool((idx[:, :, 0] == hub).all()) and int((idx == hub).sum()) == query_count(H, W)
    want = list_core_grads(inputs, idx, cnt, G, "topk")
    moved = idx.clone()
    other = next(j for j in range(H * W) if j not in set(idx[0, 100].tolist()))
    moved[0, 100, 0] = other
    got = list_core_grads(inputs, moved, cnt, G, "topk")
    for name in ("d_x_rows", "d_b2"):
        e = normwise(got[name].numpy(), want[name].numpy())
        print(f"[one-edge] {name}: {e:.2e}")
        assert e > 1e-3, (name, e)


@pytest.mark.parametrize("B,H,W,width", [(1, 10, 12, 5), (2, 24, 28, 64), (1, 255, 257, 1), (5, 6, 6, 64), (1, 1, 1, 64), (1, 2, 3, 4)])
def test_list_patterns_keep_their_promises(B, H, W, width):
    L, N = query_count(H, W), H * W
    n = min(width, N)
    for pattern in PATTERNS:
        if pattern in ("twin_hubs", "corners") and (n < 2 or min(H, W) < 2):
            continue
        idx, cnt = make_lists(pattern, B, H, W, width, seed=5)
        again = make_lists(pattern, B, H, W, width, seed=5)
        assert torch.equal(idx, again[0]) and torch.equal(cnt, again[1])
        assert tuple(idx.shape) == (B, L, width) and tuple(cnt.shape) == (B, L) and idx.dtype == torch.int64
        assert int(idx.min()) >= 0 and int(idx.max()) < N and int(cnt.min()) >= 0 and int(cnt.max()) <= n
        used = torch.arange(width)[None, None, :] < cnt[:, :, None]
        big = torch.where(used, idx, N + torch.arange(width).expand_as(idx)).sort(dim=2).values      # unused slots: distinct dummies
        assert not bool((big[:, :, 1:] == big[:, :, :-1]).any()), pattern
        if pattern == "empty":
            assert int(cnt.max()) == 0
        elif pattern == "ragged":
            assert int(cnt.max()) == n and (int(cnt.min()) == 0 or B * L < 2)
            assert bool((idx[~used] == idx[0, 0, 0]).all())
        else:
            assert bool((cnt == (min(n, N - 2) if pattern == "corners" else n)).all())
        if pattern == "hub":
            assert bool((idx[:, :, 0] == idx[0, 0, 0]).all())
        if pattern == "twin_hubs":
            assert bool((idx[:, :, 1] == idx[:, :, 0] + 1).all()) and bool((idx[:, :, 0] == idx[0, 0, 0]).all())
        if pattern == "identical":
            assert bool((idx[:, :, :n] == torch.arange(n)).all())
        if pattern == "corners":
            for c in (0, W - 1, N - W, N - 1):
                assert bool(((idx[:, :, :2] == c).sum(dim=(1, 2)) >= 2).all()) or L < 4
