"""The strips of ``dagl_conv_pair_backward`` (csrc/conv_grad.hip: cg_rows_per_block, the one function the launcher, the scratch size and
``dagl_conv_pair_backward_plan`` read) -- no GPU.  Properties over a sweep, the plans of the shapes
tests/test_gpu_conv_pair_backward_plans.py runs pinned by hand, the integer operands of those cases with their fp64 reference (shared
with the device test) and the head room that makes the device test's tolerance zero: ``sum |a||b|`` over every term of every output
stays below 2^24, so every partial sum of any strip, wave or reduce order is an exact fp32 integer."""
import ctypes as C
import functools

import pytest
import torch

# [B, H] at W = 4 -> (rows_w, strips_w, rows_x, strips_x) and the strip class
STRIP_CASES = {
    (1, 1): ((2, 1, 4, 1), "a single row: both neighbours outside the map"),
    (1, 2): ((2, 1, 4, 1), "one strip of two rows"),
    (1, 3): ((2, 2, 4, 1), "parameter gradients: a last strip of one row"),
    (1, 4): ((2, 2, 4, 1), "input gradient: exactly one strip"),
    (1, 5): ((2, 3, 4, 2), "a last strip of one row in both launches"),
    (3, 100): ((3, 34, 4, 25), "an odd strip height (3) and a last strip of one row"),
    (1, 1500): ((12, 125, 6, 250), "rows_w = 12, rows_x = 6"),
    (2, 4100): ((32, 129, 32, 129), "both launches at the 32-row clamp; a last strip of 4 rows; 258 partials in the reduce"),
}
# W at H = 5, B = 2 (every one plans (2, 3, 4, 2)) and the width class
WIDTHS = {
    4: "one K-step: seven waves idle", 8: "two K-steps: six waves idle", 12: "a pixel tile wider than the row (WT = 16)",
    16: "exactly one pixel tile", 20: "a second pixel tile of four pixels", 32: "8 K-steps over 8 waves", 36: "9 K-steps over 8 waves",
    64: "cg_xstride steps down to 68", 124: "cg_xstride stays at 132 (no step-down), WT = 128", 128: "eight pixel tiles",
    132: "the second float4 per thread", 252: "WT = 256 > W", 256: "the limit of both staging loops and of LDS",
}
WIDTH_PLAN = (2, 3, 4, 2)
ROUNDING_SHAPES = {(2, 37, 64): (2, 19, 4, 10), (3, 100, 4): (3, 34, 4, 25)}
DEVICE_SHAPES = [(B, H, 4) for B, H in sorted(STRIP_CASES)] + [(2, 5, W) for W in sorted(WIDTHS)]


def rule(B, H):
    """The plan rule, written out: about 512 blocks (4 channel groups each) for the parameters, 256 for the input; 2..32 / 4..32 rows."""
    rw = min(32, max(2, -(-B * H * 4 // 512)))
    rx = min(32, max(4, -(-B * H // 256)))
    return rw, -(-H // rw), rx, -(-H // rx)


def xstride(W):
    s = (W + 2 + 63) // 64 * 64 + 4
    return s - 64 if s - 64 >= W + 2 else s


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def plan_of(lib, B, H, W):
    out = (C.c_int32 * 4)()
    assert lib.dagl_conv_pair_backward_plan(B, H, W, out) == 0, lib.dagl_last_error()
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("case", sorted(STRIP_CASES))
def test_plans_of_the_strip_cases(lib, case):
    assert plan_of(lib, *case, 4) == STRIP_CASES[case][0], STRIP_CASES[case][1]


def test_plans_of_the_width_and_rounding_cases(lib):
    for W in WIDTHS:
        assert plan_of(lib, 2, 5, W) == WIDTH_PLAN, W
    for shape, plan in ROUNDING_SHAPES.items():
        assert plan_of(lib, *shape) == plan, shape
    assert plan_of(lib, 8, 128, 128) == (8, 16, 4, 32)                  # the training size: 8 rows per block, 4 for the input


def test_the_width_classes_are_what_their_names_say():
    assert xstride(64) == 68 and xstride(124) == 132 and xstride(128) == 132 and xstride(256) == 260 and xstride(4) == 68
    assert [W for W in WIDTHS if 16 * (W // 4) > 1024] == [] and 16 * (256 // 4) == 1024 and 4 * 132 > 512 >= 4 * 128
    assert [W for W in WIDTHS if -(-W // 16) * 16 > W] == [4, 8, 12, 20, 36, 124, 132, 252]


def test_plan_properties_over_the_sweep(lib):
    for B in (1, 2, 3, 8, 64, 300):
        for H in list(range(1, 70)) + [100, 128, 255, 256, 257, 1500, 4100]:
            for W in (4, 64, 256):
                rw, sw, rx, sx = plan = plan_of(lib, B, H, W)
                what = (B, H, W, plan)
                assert plan == rule(B, H), what
                assert 2 <= rw <= 32 and 4 <= rx <= 32, what
                for r, s in ((rw, sw), (rx, sx)):                          # the strips cover [0, H) exactly once: none empty, none short
                    assert (s - 1) * r < H <= s * r, what
                assert lib.dagl_conv_pair_backward_scratch_bytes(B, H, W) == B * sw * (4 * 2560 + 32) * 4, what


def test_the_wrapper_reports_the_same_plan(lib):
    from dagl_amd import ops
    assert ops.conv_pair_backward_plan(3, 100, 4) == dict(rows_w=3, strips_w=34, rows_x=4, strips_x=25)


def test_plan_argument_checks(lib):
    out = (C.c_int32 * 4)()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, 30), (1, 8, 260)):
        assert lib.dagl_conv_pair_backward_plan(*bad, out) == -1 and b"dagl_conv_pair_backward_plan" in lib.dagl_last_error(), bad
    assert lib.dagl_conv_pair_backward_plan(1, 8, 8, None) == -1 and b"out" in lib.dagl_last_error()


_FAKE = 0x10000


def test_incomplete_outputs_are_refused_before_the_device(lib):
    """The four parameter gradients and the scratch go together; the input gradient needs the weights."""
    call = lambda g_w, th_w, d_x, outs: lib.dagl_conv_pair_backward(None, 1, 8, 8, _FAKE, _FAKE, _FAKE, g_w, th_w, d_x, *outs)
    full = [_FAKE] * 5                                                   # d_g_w, d_g_b, d_th_w, d_th_b, scratch
    for missing in range(1, 5):
        outs = list(full); outs[missing] = None
        assert call(_FAKE, _FAKE, None, outs) == -1 and b"go together" in lib.dagl_last_error(), missing
    for g_w, th_w in ((None, _FAKE), (_FAKE, None), (None, None)):
        assert call(g_w, th_w, _FAKE, [None] * 5) == -1 and b"needs the weights" in lib.dagl_last_error()
    assert lib.dagl_conv_pair_backward(None, 1, 8, 8, _FAKE + 4, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, *[None] * 5) == -1
    assert lib.dagl_conv_pair_backward(None, 1, 8, 30, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, *[None] * 5) == -1


# ---- the operands of the device cases and their fp64 reference --------------------------------------------------------------------
NAMES = ("d_x", "d_g_w", "d_g_b", "d_th_w", "d_th_b")


def autograd64(x, gw, tw, d1, d2):
    """fp64 autograd of the two conv2d calls: x [B,64,H,W], gw [16,64,3,3], tw [16,64,1,1], d1 / d2 [B,H,W,16] -> the five gradients."""
    import torch.nn.functional as F
    dt = x.dtype
    xr, gwr, twr = (t.clone().requires_grad_(True) for t in (x, gw, tw))
    gb = torch.zeros(16, dtype=dt, requires_grad=True); tb = torch.zeros(16, dtype=dt, requires_grad=True)
    b1 = F.conv2d(xr, gwr, gb, padding=1); b2 = F.conv2d(xr, twr, tb)
    ((b1 * d1.permute(0, 3, 1, 2)).sum() + (b2 * d2.permute(0, 3, 1, 2)).sum()).backward()
    return tuple(t.grad for t in (xr, gwr, gb, twr, tb))


@functools.lru_cache(maxsize=None)
def int_case(B, H, W):
    """Integer operands in [-3, 3] and the exact gradients (fp64): (x, gw, tw, d1, d2), the five gradients."""
    g = torch.Generator().manual_seed((B * 4099 + H) * 263 + W)
    r = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    ops5 = (r(B, 64, H, W), r(16, 64, 3, 3), r(16, 64, 1, 1), r(B, H, W, 16), r(B, H, W, 16))
    return ops5, autograd64(*(t.double() for t in ops5))


@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_of_the_device_cases_stay_below_2_24(shape):
    """The same autograd on the operands' magnitudes is sum |a||b| over every term of every output."""
    ops5, grads = int_case(*shape)
    units = autograd64(*(t.double().abs() for t in ops5))
    for name, u, g in zip(NAMES, units, grads):
        assert float(u.max()) < 2 ** 24, (shape, name)
        assert bool((g.abs() <= u).all()) and bool((g == g.round()).all()), (shape, name)
