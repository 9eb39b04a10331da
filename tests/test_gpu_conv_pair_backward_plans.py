"""``dagl_conv_pair_backward`` (conv_grad.hip) over every class of its launch plan, bit for bit.  The f32-input MFMAs multiply exactly
and accumulate in fp32; with integer operands in [-3, 3] every partial sum of any strip, wave or reduce order is an exact integer
(tests/test_conv_pair_backward_plan_host.py proves ``sum |a||b| < 2^24`` over every term of every output of every case, and pins each
case's plan by hand), so all five outputs must equal the fp64 autograd of the two ``conv2d`` calls with ``torch.equal``.  A wrong
halo column, a strip boundary that reads the wrong ring slot or a partial the reduce drops fails.

Paths covered:
  * strips (W = 4): a single row, a last strip of one row in either launch, strips whose neighbours are outside the map, an odd strip
    height (3), 12 / 6 rows per block, both launches at the 32-row clamp with 258 partials in ``conv_pair_wgrad_reduce_kernel``;
  * widths (H = 5, B = 2): idle waves (4, 8), a pixel tile wider than the row (12), 8 and 9 K-steps over 8 waves (32, 36), both sides
    of the ``cg_xstride`` step-down (64, 124), the second float4 per thread (132), ``WT > W`` (252), the limit of the staging loops and
    of LDS (256);
  * for every case the three calls -- all outputs, input gradient only, parameter gradients only -- with bit-equal shared outputs;
  * the border of the padded gradient maps is poisoned, every output is pre-filled with NaN, a guard behind the scratch keeps its
    pattern.
The refusals (one parameter pointer missing, d_x without the weights) never reach the device: they are in the host file.  The GEMM
route these shapes fall back to for other widths is tests/test_gpu_gemm32_paths.py; its ``MLOOP`` instance is not reachable from either
entry and is covered by neither file."""
import pytest
import torch

from tests.test_conv_pair_backward_plan_host import DEVICE_SHAPES, NAMES, STRIP_CASES, WIDTHS, int_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN = -12345.5
GUARD = 256                                       # floats behind the scratch


def padded(d):
    """[B,H,W,16] -> the gradient of the zero-bordered map [B,H+6,W+6,16] with a poisoned border (a constant of the forward: never read)."""
    B, H, W, _ = d.shape
    p = torch.full((B, H + 6, W + 6, 16), 1e30)
    p[:, 3:3 + H, 3:3 + W] = d
    return p.to(DEV)


def run(lib, B, H, W, dev_in, want_x, want_params):
    """One call with NaN-filled outputs and a guarded scratch -> {name: tensor on the CPU} of the outputs asked for."""
    from dagl_amd import ops
    from dagl_amd._lib import check
    xd, gwd, twd, d1p, d2p = dev_in
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    outs = dict(d_x=nan(B, 64, H, W) if want_x else None)
    scr = None
    if want_params:
        outs.update(d_g_w=nan(16, 64, 3, 3), d_g_b=nan(16), d_th_w=nan(16, 64, 1, 1), d_th_b=nan(16))
        nf = lib.dagl_conv_pair_backward_scratch_bytes(B, H, W) // 4
        assert nf > 0
        scr = torch.full((nf + GUARD,), PATTERN, device=DEV)
    p = lambda t: t.data_ptr() if t is not None else None
    check(lib.dagl_conv_pair_backward(ops._stream(), B, H, W, xd.data_ptr(), d1p.data_ptr(), d2p.data_ptr(), gwd.data_ptr(), twd.data_ptr(),
                                      *(p(outs.get(n)) for n in NAMES), p(scr)), "dagl_conv_pair_backward")
    if scr is not None:
        assert bool((scr[nf:] == PATTERN).all()), "the guard behind the scratch was written"
        assert not bool((scr[:nf] == PATTERN).any()), "a partial sum of the scratch was left unwritten"
    return {n: t.cpu() for n, t in outs.items() if t is not None}


@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_plan_class_is_exact_on_integers(shape):
    from dagl_amd import _lib
    lib = _lib.load()
    B, H, W = shape
    what = STRIP_CASES[(B, H)][1] if (B, H) in STRIP_CASES else WIDTHS[W]
    (x, gw, tw, d1, d2), grads = int_case(B, H, W)
    dev_in = (x.to(DEV), gw.to(DEV), tw.to(DEV), padded(d1), padded(d2))
    both = run(lib, B, H, W, dev_in, True, True)
    for name, want in zip(NAMES, grads):
        assert torch.equal(both[name], want.float()), (shape, name, what)
    only_x = run(lib, B, H, W, dev_in, True, False)
    only_p = run(lib, B, H, W, dev_in, False, True)
    assert sorted(only_x) == ["d_x"] and sorted(only_p) == sorted(NAMES[1:])
    for name, t in {**only_x, **only_p}.items():
        assert torch.equal(t, both[name]), (shape, name, what)
