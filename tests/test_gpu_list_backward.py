"""``dagl_ce_core_backward`` (csrc/backward.hip) on crafted neighbour lists against the fp64 list-form reference
(tests/list_core_reference.py, pinned to the oracle by tests/test_list_core_reference.py).

The backward is a pure function of (wq_rows, x_rows, b2, thr, bias, nb_idx, nb_wgt, nb_s, nb_cnt, mu, d_out), so every case builds its
lists on the CPU -- no forward, no selection --, takes S, A, mu from the fp64 forward, hands the kernel their fp32 roundings and compares
every gradient, per tensor and normwise, with fp64 autograd.  The shapes are the smallest that reach each launch plan:

  keys B*N -> radix passes (key_bits): < 256 one (the sorted pairs end in the "b" buffers), < 65 536 two, from there three; the
  marker of an unused slot, B*N, is 0xFF / 0xFFFF at 255 / 65 535 keys;  E = B*L*width against the 2048-edge radix tile and the
  16-edge chunk of the segmented reduction;  runs longer than a chunk (hubs) go through the chunk partials and row_fixup_kernel;
  7*B >= 48 switches the column sums of the adaptive modes to the wide kernel.

Every list is valid (keys in [0,N), cnt <= width); the unused slots hold NaN weights and scores and an in-range wrong key, so code
that read them would give wrong numbers, nothing else.

Tolerance (``check_against_fp64``): the same reference evaluated in fp32 on the CPU sits e_ref from fp64; the kernel must stay within
4 e_ref + 2e-6, and never beyond 1e-5.  One misplaced edge costs > 1e-3 (test_one_misplaced_hub_edge_moves_the_gradients)."""
import pytest
import torch

from tests.helpers import normwise
from tests.list_core_reference import GRAD_NAMES, check_against_fp64, list_core_grads, make_inputs, make_lists

pytestmark = pytest.mark.gpu


# (B, H, W, mode, k, patterns)                                                                    keys -> passes, E, what it reaches
PLAN_CASES = [
    (1, 10, 12, "topk", 5, ("random", "hub", "ragged")),                  # 120 -> 1, 45: result in the "b" buffers, one partial tile
    (1, 15, 17, "adaptive_topk", 6, ("ragged", "corners")),               # 255 -> 1, 120: marker = 0xFF
    (1, 16, 16, "topk", 8, ("identical", "twin_hubs")),                   # 256 -> 2, 128: runs exactly one chunk long
    (1, 64, 64, "topk", 8, ("hub", "twin_hubs", "identical", "corners")),  # 4096 -> 2, 2048: one full radix tile, runs over 16 chunks
    (1, 64, 64, "adaptive_topk", 9, ("hub", "ragged")),                   # 4096 -> 2, 2304: second tile partial
    (2, 24, 28, "adaptive", 0, ("ragged", "empty", "hub")),               # 1344 -> 2, 5376: width 64, narrow column sums
    (7, 20, 24, "adaptive", 0, ("ragged", "corners")),                    # 3360 -> 2, 13440: wide column sums, image-to-image adjacency
    (1, 255, 257, "topk", 1, ("ragged",)),                                # 65535 -> 2, 4160: marker = 0xFFFF
    (1, 256, 256, "topk", 2, ("hub", "random", "ragged")),                # 65536 -> 3, 8192: first three-pass size (only the unused
                                                                          # slots' marker has bit 16 set: just "ragged" needs pass three)
    (17, 64, 64, "topk", 4, ("hub", "ragged", "corners")),                # 69632 -> 3, 17408: nine tiles, 17 hubs of in-degree 256
    (17, 64, 64, "adaptive_topk", 4, ("hub", "ragged", "corners")),       #   ... + wide column sums + dxbar
]
TINY_SHAPES = [(1, 1, 1), (1, 1, 5), (1, 2, 3), (5, 6, 6), (1, 1, 64), (1, 64, 1), (1, 33, 2)]       # <= 180 keys -> 1 pass, L = 1 ..


def _cases():
    out = []
    for B, H, W, mode, k, patterns in PLAN_CASES:
        out += [(B, H, W, mode, k, p) for p in patterns]
    for B, H, W in TINY_SHAPES:
        N = H * W
        for mode, k in (("topk", min(4, N)), ("adaptive", 0), ("adaptive_topk", min(3, N))):
            out += [(B, H, W, mode, k, p) for p in ("random", "empty")]
    return out


def _seed(B, H, W, mode, k, pattern):
    return 1000 * B + 37 * H + W + 101 * k + 7 * len(mode) + 13 * len(pattern)


@pytest.mark.parametrize("B,H,W,mode,k,pattern", _cases(), ids=lambda v: str(v))
def test_list_backward_matches_fp64(B, H, W, mode, k, pattern):
    from dagl_amd import _lib, ops
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    width = _lib.load().dagl_ce_list_width(_lib.MODES[mode], k)
    assert width >= 1
    seed = _seed(B, H, W, mode, k, pattern)
    inputs, G = make_inputs(B, H, W, seed)
    idx, cnt = make_lists(pattern, B, H, W, width, seed)
    ref64 = list_core_grads(inputs, idx, cnt, G, mode, torch.float64)
    ref32 = list_core_grads(inputs, idx, cnt, G, mode, torch.float32)
    adaptive = mode != "topk"
    unused = torch.arange(width)[None, None, :] >= cnt[:, :, None]
    nb_s, nb_wgt = ref64["S"].float(), ref64["A"].float()
    nb_s[unused] = float("nan")
    nb_wgt[unused] = float("nan")
    saved = dict(nb_idx=idx.to(torch.int32).to(dev), nb_wgt=nb_wgt.to(dev), nb_s=nb_s.to(dev), nb_cnt=cnt.to(torch.int32).to(dev),
                 mu=ref64["mu"].float().to(dev) if adaptive else None)
    d = [t.to(dev) for t in inputs[:5 if adaptive else 3]] + [None] * (0 if adaptive else 2)
    Gd = G.to(dev)
    got = ops.ce_core_backward(Gd, *d, saved, mode=mode, k=k)
    again = ops.ce_core_backward(Gd, *d, saved, mode=mode, k=k)
    names = GRAD_NAMES[:5 if adaptive else 3]
    assert (got[3] is None and got[4] is None) or adaptive
    for name, a, b in zip(names, got, again):
        assert a.shape == ref64[name].shape, name
        assert torch.equal(a, b), name                                         # same bits (NaN anywhere would fail here too)
    check_against_fp64(f"[{B},{H},{W}] {mode} k={k} {pattern}", names, got, ref64, ref32, zero_below=1e-12 if H * W == 1 else 0.0)
    if pattern == "empty":
        for name, a in zip(names, got):
            assert int(torch.count_nonzero(a)) == 0, name                      # (d_x_rows in the adaptive modes: dxbar / N with d mu = 0)


@pytest.mark.parametrize("B,H,W", [s for s in TINY_SHAPES if s[1] * s[2] <= 64], ids=lambda v: str(v))
def test_tiny_maps_end_to_end_with_every_key_a_neighbour(B, H, W):
    """Forward + backward of the core op with k = N: every key is a neighbour of every query, so there is no tie and no selection to
    disagree on, and the fp64 oracle's autograd is the reference (e_ref: the oracle in fp32)."""
    from dagl_amd import ops
    from oracle.ce_oracle import ce_core_oracle
    dev = torch.device("cuda:0")
    N = H * W
    (wq, x, b2, _, _), G = make_inputs(B, H, W, seed=500 + N + B)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [t.to(dtype).requires_grad_(True) for t in (wq, x, b2)]
        out = ce_core_oracle(*leaves, None, None, mode="topk", k=N, dtype=dtype)
        grads = torch.autograd.grad((out * G.to(dtype)).sum(), leaves)
        refs[dtype] = dict(zip(GRAD_NAMES, grads), out=out.detach())
    d = [t.to(dev) for t in (wq, x, b2)]
    out, saved = ops.ce_core_forward(*d, None, None, mode="topk", k=N)
    assert bool((saved["nb_cnt"] == N).all())
    assert bool((saved["nb_idx"].long().sort(dim=2).values == torch.arange(N, device=dev)).all())
    assert normwise(out.cpu().numpy(), refs[torch.float64]["out"].numpy()) <= 1e-4          # TOL_OUT of test_gpu_backward.py
    got = ops.ce_core_backward(G.to(dev), *d, None, None, saved, mode="topk", k=N)
    assert got[3] is None and got[4] is None
    check_against_fp64(f"[{B},{H},{W}] end-to-end topk k=N", GRAD_NAMES[:3], got, refs[torch.float64], refs[torch.float32],
                       zero_below=1e-12 if N == 1 else 0.0)
