"""The launch plan of project16_kernel (csrc/project16.hip: project16_plan, the one function its launcher plans with), read through
``dagl_project16_plan`` at 256 compute units -- no GPU.  The plans of the shapes tests/test_gpu_project16.py runs on the device are pinned
by hand, one shape per class of the kernel's routes: a later change of the plan rule shows here which classes have moved to other shapes.
The block -> (unit, tile group) rule of the kernel is restated below and shown to be a bijection onto the two-group blocks of every case.

Plan fields (``ops.PROJECT16_PLAN_FIELDS``): key items, query items (32 patches each), lin (keys in row-major order across row ends,
W >= 32), units_q, units_k (8 items; two blocks per unit: tile groups 0-3 / 4-6), n_full (two-group blocks, project16_body2), n_xcd (the
ids among them mapped through the XCD permutation, n_full & ~15), n_split_groups (key units of the LAST image cut into 14 single-tile
blocks each, project16_body), n_proj (all blocks), cap (resident blocks), key items per row (row-wise keys), query items per row."""
import ctypes as C
import os
import re

import pytest

CUS = 256
FIELDS = ("key_items", "query_items", "lin", "units_q", "units_k", "n_full", "n_xcd", "n_split_groups", "n_proj", "cap", "segs_k", "segs_q")

# (B, H, W, which) -> (plan at 256 CUs, class)
CASES = {
    (1, 1, 1, 1): ((1, 1, 0, 0, 1, 0, 0, 1, 14, 512, 1, 1), "one patch: no two-group block at all, 7 single-tile blocks + 7 without an item"),
    (1, 1, 1, 2): ((1, 1, 0, 1, 0, 2, 0, 0, 2, 512, 1, 1), "one query: L < 32, both tile groups by the tail rule"),
    (1, 1, 1, 3): ((1, 1, 0, 1, 1, 2, 0, 1, 16, 512, 1, 1), "one patch and one query in one launch"),
    (1, 2, 3, 3): ((2, 1, 0, 1, 1, 2, 0, 1, 16, 512, 1, 1), "row-wise keys (lim = W), single-tile; SAME corner H, W = 2, 3 (mod 4)"),
    (1, 5, 9, 3): ((5, 1, 0, 1, 1, 2, 0, 1, 16, 512, 1, 1), "row-wise keys, single-tile, the second block with one item of four (wave_valid); H, W = 1 (mod 4)"),
    (1, 7, 31, 3): ((7, 1, 0, 1, 1, 2, 0, 1, 16, 512, 1, 1), "row-wise keys at the widest row (lim = 31); H, W = 3 (mod 4)"),
    (3, 16, 16, 3): ((16, 1, 0, 1, 2, 14, 0, 2, 42, 512, 1, 1),
                     "row-wise keys on two-group blocks (images 0, 1) beside single-tile (image 2); H, W = 0 (mod 4)"),
    (1, 9, 32, 3): ((9, 1, 1, 1, 2, 2, 0, 2, 30, 512, 1, 1), "linear keys, W = 32 exactly: every item is one row; a second unit of one item"),
    (1, 8, 33, 3): ((9, 1, 1, 1, 2, 2, 0, 2, 30, 512, 2, 1), "linear keys that wrap into the next row with nA < 32; last item of 8 patches"),
    (1, 3, 70, 3): ((7, 1, 1, 1, 1, 2, 0, 1, 16, 512, 3, 1), "linear keys, last item partial (18 patches) in the last map row: the Hp - 1 clamp"),
    (2, 9, 38, 3): ((11, 1, 1, 1, 2, 8, 0, 2, 36, 512, 2, 1), "linear + wrap on two-group blocks (image 0) and single-tile (image 1); L = 30"),
    (2, 45, 38, 1): ((54, 4, 1, 0, 7, 14, 0, 7, 112, 512, 2, 1), "a unit with missing items (54 of 56); tail ids only (n_full = 14)"),
    (2, 45, 38, 3): ((54, 4, 1, 1, 7, 18, 16, 7, 116, 512, 2, 1), "the same with queries: n_full = 18 = 16 XCD-mapped ids + a tail of 2; L = 120"),
    (2, 63, 50, 1): ((99, 7, 1, 0, 13, 26, 16, 13, 208, 512, 2, 1), "XCD-mapped ids + tail of 10 + 13 single-tile groups (n_full = 26)"),
    (144, 8, 32, 1): ((8, 1, 1, 0, 1, 288, 288, 0, 288, 512, 1, 1), "all blocks two-group, the group flip reached (ids >= 256), linear keys"),
    (144, 8, 1, 1): ((8, 1, 0, 0, 1, 288, 288, 0, 288, 512, 1, 1), "the same with row-wise keys of one patch per item (lim = 1)"),
    (144, 8, 32, 3): ((8, 1, 1, 1, 1, 574, 560, 1, 588, 512, 1, 1), "keys + queries, flip, a tail of 14, one split group (n_proj = 574 + 14)"),
}


def rule(B, H, W, which, cus=CUS):
    """The plan rule, written out."""
    N, Lw = H * W, -(-W // 4)
    L = -(-H // 4) * Lw
    lin = int(W >= 32)
    key_items = -(-N // 32) if lin else -(-W // 32) * H
    query_items = -(-L // 32)
    uq = -(-query_items // 8) if which & 2 else 0
    uk = -(-key_items // 8) if which & 1 else 0
    cap = 2 * cus
    total = 2 * B * (uq + uk)
    rem = total % cap
    groups = min((rem + 1) // 2 if 0 < rem <= cap // 2 else 0, uk)       # an overhang of at most half a round is cut up
    n_full = total - 2 * groups
    return (key_items, query_items, lin, uq, uk, n_full, n_full & ~15, groups, n_full + 14 * groups, cap, -(-W // 32), -(-Lw // 32))


def block_map(bid, n_full):
    """project16_kernel's block id -> (unit over all images, tile group), restated."""
    if bid < (n_full & ~15):
        xcd, q = bid & 7, bid >> 3
        return 8 * (q >> 1) + xcd, (q ^ (q >> 5)) & 1
    return bid >> 1, bid & 1


def single_tile_units(B, plan):
    """{(image, key unit)} served by the single-tile blocks: the last n_split_groups key units of the last image."""
    p = dict(zip(FIELDS, plan))
    return {(B - 1, p["units_k"] - p["n_split_groups"] + g) for g in range(p["n_split_groups"])}


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


def plan_of(lib, B, H, W, which, cus=CUS):
    out = (C.c_int32 * 12)()
    assert lib.dagl_project16_plan(B, H, W, which, cus, out) == 0, lib.dagl_last_error()
    return tuple(int(v) for v in out)


def test_symbols_in_the_header_and_the_table():
    from dagl_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dagl_ce.h")).read()
    for name in ("dagl_project16_plan", "dagl_ce_project16_debug", "dagl_ce_project16_debug_scratch_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b(size_t|int)\s+" + name + r"\(", header), name
    assert ops.PROJECT16_PLAN_FIELDS == FIELDS


@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "x".join(map(str, c)))
def test_plans_of_the_device_cases(lib, case):
    assert plan_of(lib, *case) == CASES[case][0], CASES[case][1]
    assert rule(*case) == CASES[case][0]


def test_every_class_of_the_routes_has_a_case():
    """What the table claims to reach, from the pinned figures themselves."""
    p = {c: dict(zip(FIELDS, v[0])) for c, v in CASES.items()}
    assert p[(1, 1, 1, 1)]["n_full"] == 0 and p[(1, 1, 1, 2)]["n_split_groups"] == 0
    for c in ((1, 2, 3, 3), (1, 5, 9, 3), (1, 7, 31, 3)):                # row-wise, every key unit single-tile; H, W = 1, 2, 3 (mod 4)
        assert not p[c]["lin"] and p[c]["n_split_groups"] == p[c]["units_k"] and c[0] == 1
    assert {(c[1] % 4, c[2] % 4) for c in CASES} >= {(0, 0), (1, 1), (2, 3), (3, 3)}
    c = (3, 16, 16, 3)                                                   # images 0, 1 two-group, image 2 single-tile
    assert not p[c]["lin"] and single_tile_units(3, CASES[c][0]) == {(2, 0), (2, 1)} and p[c]["n_full"] == 2 * (3 * 3 - 2)
    for c, last in (((1, 9, 32, 3), 32), ((1, 8, 33, 3), 8), ((1, 3, 70, 3), 18)):
        assert p[c]["lin"] and c[1] * c[2] - 32 * (p[c]["key_items"] - 1) == last
    c = (2, 9, 38, 3)
    assert p[c]["lin"] and single_tile_units(2, CASES[c][0]) == {(1, 0), (1, 1)} and -(-9 // 4) * -(-38 // 4) == 30
    assert p[(2, 45, 38, 1)]["key_items"] < 8 * p[(2, 45, 38, 1)]["units_k"] and p[(2, 45, 38, 1)]["n_xcd"] == 0
    assert (p[(2, 45, 38, 3)]["n_full"], p[(2, 45, 38, 3)]["n_xcd"]) == (18, 16)
    assert (p[(2, 63, 50, 1)]["n_full"], p[(2, 63, 50, 1)]["n_xcd"], p[(2, 63, 50, 1)]["n_split_groups"]) == (26, 16, 13)
    for c in ((144, 8, 32, 1), (144, 8, 1, 1)):
        assert p[c]["n_xcd"] == p[c]["n_full"] == 288 > 256 and p[c]["n_split_groups"] == 0
    c = (144, 8, 32, 3)
    assert p[c]["n_full"] - p[c]["n_xcd"] == 14 and p[c]["n_split_groups"] == 1 and p[c]["n_xcd"] > 256


@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "x".join(map(str, c)))
def test_block_map_is_a_bijection_onto_the_full_blocks(case):
    """Every (unit, tile group) that is not cut into single-tile blocks is served by exactly one block id < n_full."""
    B = case[0]
    p = dict(zip(FIELDS, CASES[case][0]))
    per = p["units_q"] + p["units_k"]
    served = [block_map(bid, p["n_full"]) for bid in range(p["n_full"])]
    want = {(v, g) for v in range(B * per - p["n_split_groups"]) for g in (0, 1)}
    assert len(served) == len(set(served)) and set(served) == want
    # ... and the units left out are exactly the last key units of the last image
    left = {(v // per, v % per - p["units_q"]) for v in range(B * per) if (v, 0) not in want}
    assert left == single_tile_units(B, CASES[case][0])


def test_block_map_over_a_sweep_of_block_counts():
    for n_full in range(0, 1200, 2):
        served = {block_map(bid, n_full) for bid in range(n_full)}
        assert served == {(v, g) for v in range(n_full // 2) for g in (0, 1)}, n_full
    assert {block_map(bid, 288)[1] for bid in range(256, 264)} == {1} and {block_map(bid, 288)[1] for bid in range(0, 8)} == {0}


def test_plan_follows_the_rule_over_a_sweep(lib):
    for cus in (256, 304, 64):
        for B in (1, 2, 3, 5, 64, 144):
            for H in (1, 2, 7, 8, 9, 45, 64):
                for W in (1, 3, 31, 32, 33, 38, 70, 128):
                    for which in (1, 2, 3):
                        plan = plan_of(lib, B, H, W, which, cus)
                        assert plan == rule(B, H, W, which, cus), (cus, B, H, W, which)
                        p = dict(zip(FIELDS, plan))
                        assert p["n_split_groups"] <= p["units_k"] and p["n_full"] % 2 == 0
                        assert 8 * p["units_k"] >= p["key_items"] * (which & 1) > 8 * (p["units_k"] - 1)


def test_the_wrapper_reports_the_same_plan(lib):
    from dagl_amd import ops
    assert tuple(ops.project16_plan(2, 63, 50, 1, cus=CUS).values()) == CASES[(2, 63, 50, 1)][0]
    assert tuple(ops.project16_plan(2, 63, 50, 1, cus=CUS)) == FIELDS


def test_argument_checks(lib):
    out = (C.c_int32 * 12)()
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 0), (1, 8, 8, 4)):
        assert lib.dagl_project16_plan(*bad, CUS, out) == -1 and b"bad argument" in lib.dagl_last_error(), bad
    assert lib.dagl_project16_plan(1, 8, 8, 3, CUS, None) == -1
    # cus <= 0: the device's count, 256 without a device -- a plan either way
    assert lib.dagl_project16_plan(1, 8, 8, 3, 0, out) == 0 and out[9] > 0
