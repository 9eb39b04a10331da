"""The launch plan of conv_pair16_kernel (csrc/prologue.hip: conv16_plan, the one function its launcher, the fused forward's workspace and
dagl_ce_prologue16's scratch plan with), read through ``dagl_ce_prologue16_plan`` -- no GPU.  Properties over a sweep of shapes, and the
plans of the shapes tests/test_gpu_prologue16.py runs on the device, pinned by hand: a later change of the plan rule shows here which of
its classes (one row per block, a last chunk of one row, the odd tail of the two-row loop, ...) have moved to other shapes."""
import ctypes as C
import os
import re

import pytest

# [B, H, W] -> (strips, chunks, rows per block, slots per head) and the class the GPU test runs the shape for
CASES = {
    (1, 1, 1): ((1, 1, 1, 4), "one row per block (H = 1); W < 4"),
    (1, 2, 3): ((1, 1, 2, 4), "one block of two rows; W < 4"),
    (1, 3, 5): ((1, 2, 2, 8), "a last chunk of one row"),
    (2, 5, 63): ((1, 3, 2, 24), "W = 63: the strip's last column and its right halo outside the map; a last chunk of one row"),
    (1, 4, 64): ((1, 2, 2, 8), "exactly one strip: the right halo outside the map"),
    (1, 6, 65): ((2, 3, 2, 24), "a second strip of one pixel"),
    (1, 9, 130): ((3, 5, 2, 60), "three strips; Lw = 33 through thr_bias_kernel (W % 4 = 2); a last chunk of one row"),
    (1, 8, 132): ((3, 4, 2, 48), "three strips; Lw = 33 through thr_bias4_kernel"),
    (43, 7, 65): ((2, 3, 3, 1032), "three rows per block: the loop's odd tail; chunks of 3, 3, 1 rows"),
    (64, 8, 70): ((2, 2, 4, 1024), "four rows per block"),
    (256, 5, 8): ((1, 1, 5, 1024), "one block per image, five rows = H"),
    (1, 8, 64): ((1, 4, 2, 16), "W % 4 == 0 with an unaligned x"),
    (1, 7, 65): ((2, 4, 2, 32), "an image of [43,7,65] alone: two rows per block"),
    (2, 12, 130): ((3, 6, 2, 144), "the scale cases: 6 chunks of 2 rows, 3 strips"),
}
MULTI_HEAD = ((4, 2, 7, 65), (2, 4, 2, 64))      # the 4-head debug call: (heads, imgs, H, W) -> plan


def rule(heads, imgs, H, W):
    """The plan rule, written out: one block per CU (256) over the launch, at least two rows per block, no empty block."""
    strips = -(-W // 64)
    chunks = max(1, min(-(-256 // (strips * heads * imgs)), (H + 1) // 2))
    rows = -(-H // chunks)
    chunks = -(-H // rows)
    return strips, chunks, rows, 4 * strips * chunks * imgs


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def plan_of(lib, heads, imgs, H, W):
    out = (C.c_int32 * 4)()
    assert lib.dagl_ce_prologue16_plan(heads, imgs, H, W, out) == 0, lib.dagl_last_error()
    return tuple(int(v) for v in out)


def test_symbols_in_the_header_and_the_table():
    from dagl_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_ce_prologue16_plan", "dagl_ce_prologue16_debug", "dagl_ce_prologue16_debug_scratch_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name


def test_plan_properties_over_the_sweep(lib):
    for heads in (1, 4):
        for imgs in (1, 2, 3, 43, 64, 256):
            for H in range(1, 41):
                for W in (1, 3, 63, 64, 65, 128, 129, 132, 200):
                    strips, chunks, rows, slots = plan = plan_of(lib, heads, imgs, H, W)
                    what = (heads, imgs, H, W, plan)
                    assert strips == -(-W // 64), what
                    assert chunks * rows >= H, what
                    assert (chunks - 1) * rows < H, what                  # no block is empty
                    assert rows >= 2 or H == 1, what
                    assert slots == 4 * strips * chunks * imgs, what
                    assert plan == rule(heads, imgs, H, W), what


def test_the_wrapper_reports_the_same_plan(lib):
    from dagl_amd import ops
    assert ops.ce_prologue16_plan(1, 43, 7, 65) == dict(strips=2, chunks=3, rows=3, slots=1032)


@pytest.mark.parametrize("shape", sorted(CASES))
def test_plans_of_the_device_cases(lib, shape):
    B, H, W = shape
    assert plan_of(lib, 1, B, H, W) == CASES[shape][0], CASES[shape][1]


def test_plan_of_the_four_head_call(lib):
    assert plan_of(lib, *MULTI_HEAD[0]) == MULTI_HEAD[1]
    # a stage's heads are one launch: the rows per block follow the whole batch, the slots are per head
    assert plan_of(lib, 4, 64, 8, 70) == (2, 1, 8, 4 * 2 * 1 * 64) and plan_of(lib, 1, 64, 8, 70)[1:3] == (2, 4)


def test_scratch_grows_by_exactly_the_slots(lib):
    """dagl_ce_prologue16_scratch_bytes carves the slots from the same plan: between two shapes that differ in nothing but their slots
    (H and H + 1 with the same query grid: the packed weights and the heads' partial sums stay) the size moves by exactly the slots' bytes
    after the carve's 256-byte rounding."""
    up = lambda n: -(-n // 256) * 256
    size = lib.dagl_ce_prologue16_scratch_bytes
    pairs = 0
    for B in (1, 2, 3, 43, 64, 256):
        for W in (1, 3, 63, 64, 65, 128, 129, 132, 200):
            for H in range(1, 40):
                # H and H + 1 with the same query grid (the heads' partial sums: 8 B L floats) differ only in their slots
                if -(-H // 4) != -(-(H + 1) // 4):
                    continue
                s0, s1 = plan_of(lib, 1, B, H, W)[3], plan_of(lib, 1, B, H + 1, W)[3]
                assert size(B, H + 1, W) - size(B, H, W) == up(4 * s1) - up(4 * s0), (B, H, W)
                pairs += up(4 * s1) != up(4 * s0)
    assert pairs > 50                                                     # ... and many of the pairs do differ
    assert size(0, 8, 8) == 0 and size(1, 0, 8) == 0


def test_argument_checks(lib):
    out = (C.c_int32 * 4)()
    for bad in ((0, 1, 8, 8), (5, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0)):
        assert lib.dagl_ce_prologue16_plan(*bad, out) == -1 and b"bad argument" in lib.dagl_last_error(), bad
    assert lib.dagl_ce_prologue16_plan(1, 1, 8, 8, None) == -1
