"""``ops.ces_stage_fold_mix`` (dagl_ces_stage_fold_mix, csrc/aggregate.hip): the fold of four heads' aggregated rows, the stage's 1x1 mix
and the residual in one launch, against ``conv2d(cat(fold / cnt)) + x`` on the CPU under the project's rule ``e <= 3 e_ref32 + 1e-6``, and
its pre-mix values pixel for pixel against ``ops.fold_normalize``."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import _check, _fold, _geom

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 480 and 2310 pixels: no multiple of the 64-pixel wave tile, several blocks; 33 and 70 no multiples of 4; 54 pixels: less than one tile
SHAPES = [(2, 24, 20), (1, 33, 70), (1, 9, 6)]


def _id(v):
    return "x".join(str(e) for e in v)


@functools.lru_cache(maxsize=None)
def _operands(shape, seed=3):
    """(agg [4,B,L,784] in the library's element order (kh, kw, c), x [B,64,H,W], mix_w [64,64] uniform +-1/8, mix_b [64]) on the CPU."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    agg = torch.randn(4, B, L, 784, generator=gen)
    x = torch.randn(B, 64, H, W, generator=gen)
    mix_w = (torch.rand(64, 64, generator=gen) - 0.5) / 4
    mix_b = (torch.rand(64, generator=gen) - 0.5) / 4
    return agg, x, mix_w, mix_b


def _reference(agg, x, mix_w, mix_b, shape, dtype):
    from oracle.ce_oracle import overlap_count
    B, H, W, L, N = _geom(shape)
    rows = agg.to(dtype).view(4, B, L, 7, 7, 16).permute(0, 1, 2, 5, 3, 4).reshape(4, B, L, 784)          # (c, kh, kw): F.fold's order
    cat = torch.cat([_fold(rows[h], overlap_count(H, W, dtype), H, W) for h in range(4)], dim=1)
    return F.conv2d(cat, mix_w.to(dtype).view(64, 64, 1, 1), mix_b.to(dtype)) + x.to(dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_against_the_cpu(shape):
    from dagl_amd import ops
    cpu = _operands(shape)
    dev = [t.to(DEV) for t in cpu]
    out = ops.ces_stage_fold_mix(*dev)
    assert out.shape == cpu[1].shape and out.dtype == torch.float32
    torch.set_num_threads(16)
    _check(f"fold_mix {shape}", out, _reference(*cpu, shape, torch.float64), _reference(*cpu, shape, torch.float32))
    assert torch.equal(ops.ces_stage_fold_mix(*dev), out)
    # the 1x1 convolution's own layout of the weights
    assert torch.equal(ops.ces_stage_fold_mix(dev[0], dev[1], dev[2].view(64, 64, 1, 1), dev[3]), out)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_concat_values_are_fold_normalize_s(shape):
    """Identity weights, no bias, no residual: every product but one of an output is an exact zero, so the output IS the pre-mix value."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    agg = _operands(shape)[0].to(DEV)
    out = ops.ces_stage_fold_mix(agg, torch.zeros(B, 64, H, W, device=DEV), torch.eye(64, device=DEV), torch.zeros(64, device=DEV))
    want = torch.cat([ops.fold_normalize(agg[h].contiguous(), H, W) for h in range(4)], dim=1)
    assert torch.equal(out, want)
    # ... and through a permutation of the channels: output o reads concat channel (o * 5 + 3) % 64
    perm = (torch.arange(64) * 5 + 3) % 64
    out = ops.ces_stage_fold_mix(agg, torch.zeros(B, 64, H, W, device=DEV), torch.eye(64)[perm].contiguous().to(DEV),
                                 torch.zeros(64, device=DEV))
    assert torch.equal(out, want[:, perm.to(DEV)])


def test_the_large_map_form():
    """From 2048 four-tile waves on (131072 pixels) a wave runs four tiles in the place of one: (1,366,362) has 132492 pixels, no
    multiple of 256, and sides that are no multiples of 4.  Against the CPU, and its pre-mix values against ``fold_normalize``."""
    from dagl_amd import ops
    shape = (1, 366, 362)
    B, H, W, L, N = _geom(shape)
    assert N >= 2048 * 64 and N % 256 != 0
    cpu = _operands(shape)
    dev = [t.to(DEV) for t in cpu]
    out = ops.ces_stage_fold_mix(*dev)
    torch.set_num_threads(16)
    _check(f"fold_mix {shape}", out, _reference(*cpu, shape, torch.float64), _reference(*cpu, shape, torch.float32))
    assert torch.equal(ops.ces_stage_fold_mix(*dev), out)
    zeros = torch.zeros(B, 64, H, W, device=DEV)
    out = ops.ces_stage_fold_mix(dev[0], zeros, torch.eye(64, device=DEV), torch.zeros(64, device=DEV))
    assert torch.equal(out, ops.fold_normalize(dev[0].view(4, L, 784), H, W).view(1, 64, H, W))


def test_the_two_launches_it_replaces():
    """``fold_normalize`` on the four heads as a batch (at B = 1 that IS the concat map) and ``ces_stage_mix``: the same reference, the
    same bound -- what tools/time_stage_step.py times the fused kernel against."""
    from dagl_amd import ops
    shape = SHAPES[1]
    B, H, W, L, N = _geom(shape)
    cpu = _operands(shape)
    agg, x, mix_w, mix_b = [t.to(DEV) for t in cpu]
    cat = ops.fold_normalize(agg.view(4, L, 784), H, W).view(1, 64, H, W)
    two = ops.ces_stage_mix(cat, x, mix_w, mix_b)
    torch.set_num_threads(16)
    _check(f"fold + stage_mix {shape}", two, _reference(*cpu, shape, torch.float64), _reference(*cpu, shape, torch.float32))
    with pytest.raises(ops.DaglError, match="cat"):
        ops.ces_stage_mix(cat[:, :32].contiguous(), x, mix_w, mix_b)


def test_operand_refusals():
    from dagl_amd import DaglError, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    agg, x, mix_w, mix_b = [t.to(DEV) for t in _operands(shape)]
    for bad, word in (((agg[:3].contiguous(), x, mix_w, mix_b), "agg"), ((agg[:, :1].contiguous(), x, mix_w, mix_b), "agg"),
                      ((agg, x[:, :32].contiguous(), mix_w, mix_b), "64"), ((agg, x, mix_w[:32].contiguous(), mix_b), "mix_w"),
                      ((agg, x, mix_w, mix_b[:32].contiguous()), "mix_b"), ((agg.cpu(), x, mix_w, mix_b), "GPU"),
                      ((agg, x.double(), mix_w, mix_b), "dtype"), ((agg, x, mix_w.t(), mix_b), "contiguous")):
        with pytest.raises(DaglError, match=word):
            ops.ces_stage_fold_mix(*bad)
