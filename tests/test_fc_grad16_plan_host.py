"""The launch plan of the split-fp16 projection gradients (gemm16s.hip: fcg_implicit_rows, fcg_plan, gemm16s_tile), without a GPU: what
``dagl_fc_grad16_plan`` reports against plans derived by hand, for the shapes tests/test_gpu_fc_grad16_plans.py runs on the device (it
imports CASES from here), and the claim that those shapes reach every value of every planning axis."""
import ctypes as C

import pytest

from tests.test_abi_symbols import lib_path  # noqa: F401  (fixture)


def _case(name, B, oh, ow, stride=1, oy=0, ox=0, Hp=None, Wp=None):
    return dict(name=name, B=B, oh=oh, ow=ow, stride=stride, oy=oy, ox=ox, Hp=oh + 6 if Hp is None else Hp, Wp=ow + 6 if Wp is None else Wp)


# Every shape the device tests run.  k1 / k2: the stride-4 SAME 7x7 query grid of a 5 x 5 and of a 23 x 30 map on its 3-pixel border
# (5: 2 windows, padding 6 = 3 + 3 -> offset 3 - 3 = 0; 23: 6 windows, padding 4 = 2 + 2 -> oy = 1; 30: 8 windows, 5 = 2 + 3 -> ox = 1).
# j1 / j2: maps one pixel larger than the windows need (1 + 5 * 2 + 7 = 18 rows, 2 + 6 * 2 + 7 = 21 columns; 9 + 7 = 16, 12 + 7 = 19).
CASES = [
    _case("a", 1, 8, 32),
    _case("b", 1, 5, 128),
    _case("c", 1, 1, 256),
    _case("d", 1, 12, 32),
    _case("e", 2, 9, 64),
    _case("f", 1, 3, 5),
    _case("g", 3, 7, 16),
    _case("h", 2, 40, 36),
    _case("i", 1, 8, 32, Hp=15, Wp=39),
    _case("j1", 2, 6, 7, stride=2, oy=1, ox=2, Hp=19, Wp=22),
    _case("j2", 1, 4, 5, stride=3, Hp=17, Wp=20),
    _case("k1", 3, 2, 2, stride=4, Hp=11, Wp=11),
    _case("k2", 1, 6, 8, stride=4, oy=1, ox=1, Hp=29, Wp=36),
]
CASE = {c["name"]: c for c in CASES}

# By hand, for the call that asks for d_w and the input gradient (d_map where the product can fold: stride 1 and 16 | 32 | 64 | k 128
# patches per row; d_rows elsewhere).
#  fcg_implicit_rows: shifted planes need stride 1 from the map's corner, Hp = oh + 6, Wp = ow + 6, ow a power of two in 32 .. 512 and
#    n = B oh ow a multiple of 128; rows per slice = the first divisor r of oh with r ow >= 256, then any larger one up to 1.5 B oh / 36.
#  fcg_plan: otherwise 36 slices of ceil(n / 36) rounded up to 32, at least 256 patches, slices = ceil(n / k_slice); n_pad = slices x
#    k_slice rounded up to 128.
#  gemm16s_tile: d_w (M = 196) runs 256-row tiles when it has several slices or reads shifted planes, else 128; d rows (K = 224) 128-row
#    tiles, one column tile per block below 512 row tiles.
#   a (1,8,32):   n 256; divisors of 8 with r * 32 >= 256: 8 -> one slice of 256
#   b (1,5,128):  n 640; 1 * 128 < 256, 5 * 128 = 640 -> one slice of 640; rows 128 wide: one 128-patch segment per tile
#   c (1,1,256):  n 256; 1 * 256 -> one slice of one image row; two 128-segments
#   d (1,12,32):  n 384; r >= 8: 12 -> one slice of 384
#   e (2,9,64):   n 1152; 1, 3 (192) too short, 9 (576): one slice per image
#   f (1,3,5):    n 15, 5 patches per row: patch rows; ceil(15/36) -> 32 -> 256, one slice, n_pad 256; no fold below 16
#   g (3,7,16):   n 336, 16 < 32: patch rows; 10 -> 32 -> 256, ceil(336 / 256) = 2 slices, n_pad 512; fold: 8 segments of 16
#   h (2,40,36):  n 2880, 36 no power of two: patch rows; 80 -> 96 -> 256, ceil(11.25) = 12 slices, n_pad 3072; 36: no fold
#   i:            a's grid on a 15 x 39 map: Hp != oh + 6 -> patch rows, one slice of 256
#   j1 (2,6,7 stride 2): n 84 -> one slice, n_pad 256;  j2 (1,4,5 stride 3): n 20;  k1: n 12;  k2: n 48 -- all patch rows, no fold
_P = lambda n, n_pad, slices, k_slice, im_rps, w_tile, fold_seg=0, fold_rows=0: dict(  # noqa: E731
    n=n, n_pad=n_pad, slices=slices, k_slice=k_slice, im_rps=im_rps, w_tile=w_tile, w_impl=int(im_rps > 0), rows_tile=128, n_loop=1,
    fold_seg=fold_seg, fold_rows=fold_rows, merged_split=1)
WANT = {
    "a": _P(256, 256, 1, 256, 8, 256, 32, 4),
    "b": _P(640, 640, 1, 640, 5, 256, 128, 1),
    "c": _P(256, 256, 1, 256, 1, 256, 128, 1),
    "d": _P(384, 384, 1, 384, 12, 256, 32, 4),
    "e": _P(1152, 1152, 2, 576, 9, 256, 64, 2),
    "f": _P(15, 256, 1, 256, 0, 128),
    "g": _P(336, 512, 2, 256, 0, 256, 16, 8),
    "h": _P(2880, 3072, 12, 256, 0, 256),
    "i": _P(256, 256, 1, 256, 0, 128, 32, 4),
    "j1": _P(84, 256, 1, 256, 0, 128),
    "j2": _P(20, 256, 1, 256, 0, 128),
    "k1": _P(12, 256, 1, 256, 0, 128),
    "k2": _P(48, 256, 1, 256, 0, 128),
}
# the cases whose calls are repeated with every subset of the outputs (merged_split true and false)
SUBSET_CASES = ("e", "g", "h")


def folds(c):
    """Whether ``dagl_fc_grad16_dmap`` serves the case (fcg_fold_ok)."""
    return c["stride"] == 1 and c["ow"] >= 16 and (c["ow"] % 128 == 0 or 128 % c["ow"] == 0)


def plan_of(ops, c, want_w=True, want_rows=False, want_map=False):
    return ops.fc_grad16_plan(c["B"], c["Hp"], c["Wp"], (c["stride"], c["oy"], c["ox"], c["oh"], c["ow"]), want_w, want_rows, want_map)


@pytest.fixture()
def ops(lib_path):  # noqa: F811
    from dagl_amd import ops
    return ops


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_plans_match_the_hand_derived_ones(ops, name):
    c = CASE[name]
    plan = plan_of(ops, c, True, not folds(c), folds(c))
    assert sorted(plan) == sorted(ops.FC_GRAD16_PLAN_FIELDS)
    assert plan == WANT[name], plan
    # the same d_w plan whichever input gradient goes with it; the fold only where asked for
    rows = plan_of(ops, c, True, True, False)
    assert rows == dict(plan, fold_seg=0, fold_rows=0)
    alone = plan_of(ops, c, True, False, False)
    assert alone == dict(rows, rows_tile=0, n_loop=0, merged_split=0)


def test_shifted_planes_always_run_on_the_kernel_that_reads_them(ops):
    """One-image maps whose only admissible slice is the whole image (one K slice) as well as the many-slice plans: every plan that
    reads shifted planes names the IMPL instantiation of the 256-row kernel."""
    maps = [(1, 1, 256), (1, 1, 512), (1, 2, 128), (1, 3, 128), (1, 4, 64), (1, 6, 64), (1, 8, 32), (1, 12, 32)]
    maps += [(1, h, 128) for h in (5, 7, 11, 13, 17, 19, 23, 29, 31, 37)]
    for B, oh, ow in maps:
        p = plan_of(ops, _case("", B, oh, ow))
        assert (p["im_rps"], p["slices"], p["k_slice"]) == (oh, 1, oh * ow), (B, oh, ow, p)
        assert (p["w_tile"], p["w_impl"]) == (256, 1), (B, oh, ow, p)
    for B, oh, ow in [(2, 9, 64), (8, 128, 128), (1, 64, 64), (3, 40, 64), (2, 24, 32), (1, 16, 256), (4, 1, 512)]:
        p = plan_of(ops, _case("", B, oh, ow))
        assert p["im_rps"] > 0 and p["slices"] > 1 and (p["w_tile"], p["w_impl"]) == (256, 1), (B, oh, ow, p)
    # (8,128,128), the benchmark's size: the largest divisor of 128 up to 1.5 x 1024 / 36 = 42.7 image rows per slice is 32 -> 32 slices
    # of 4096 patches; 1024 row tiles of d rows: a block walks all 7 column tiles -- pinned so that no change to the one-slice plans moves it
    p = plan_of(ops, _case("", 8, 128, 128), True, False, True)
    assert (p["im_rps"], p["slices"], p["k_slice"], p["n_pad"], p["n_loop"], p["fold_seg"]) == (32, 32, 4096, 131072, 7, 128), p


def test_plans_without_the_weight_gradient(ops):
    """d_w not asked for: no shifted planes are planned (the slices are fcg_plan's own; only n_pad matters to the d rows product), no tile
    kernel for d_w is named, and the split of d z is the row-major copy alone."""
    p = plan_of(ops, CASE["e"], False, False, True)          # 1152 patches: 32 -> 256 per slice, ceil(4.5) = 5 slices, n_pad 1280
    assert p == dict(n=1152, n_pad=1280, slices=5, k_slice=256, im_rps=0, w_tile=0, w_impl=0, rows_tile=128, n_loop=1, fold_seg=64,
                     fold_rows=2, merged_split=0), p
    p = plan_of(ops, CASE["h"], False, True, False)
    assert (p["w_tile"], p["rows_tile"], p["merged_split"], p["fold_seg"]) == (0, 128, 0, 0), p
    p = plan_of(ops, CASE["h"], False, False, False)         # the bias-only call
    assert (p["w_tile"], p["rows_tile"], p["n_loop"], p["merged_split"]) == (0, 0, 0, 0), p


def test_the_case_list_reaches_every_value_of_every_axis(ops):
    plans = {c["name"]: plan_of(ops, c, True, not folds(c), folds(c)) for c in CASES}
    route = {(p["im_rps"] > 0, p["slices"] > 1) for p in plans.values()}
    assert route == {(True, False), (True, True), (False, False), (False, True)}        # shifted planes / patch rows x one / more slices
    assert {p["w_tile"] for p in plans.values()} == {128, 256}
    assert {p["fold_seg"] for p in plans.values()} >= {16, 32, 64, 128}
    assert any(p["n"] % 128 != 0 and p["n"] > 128 for p in plans.values()) and any(p["n"] < 128 for p in plans.values())
    assert any(p["n_pad"] > p["n"] for p in plans.values())
    # the output subsets run at these cases: both values of merged_split, a many-slice plan of either route, a fold
    sub = [CASE[n] for n in SUBSET_CASES]
    assert {plan_of(ops, c, w, r, False)["merged_split"] for c in sub for w in (0, 1) for r in (0, 1)} == {0, 1}
    assert {(plans[n]["im_rps"] > 0) for n in SUBSET_CASES} == {True, False} and all(plans[n]["slices"] > 1 for n in SUBSET_CASES)
    assert any(folds(c) for c in sub)
    # windows other than CE's two grids, and maps larger than their windows need
    assert any(c["stride"] not in (1, 4) for c in CASES) and any(c["stride"] == 1 and c["Hp"] > c["oh"] + 6 for c in CASES)


def test_plan_rejects_bad_arguments(ops):
    from dagl_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 12)()
    assert lib.dagl_fc_grad16_plan(1, 14, 38, 1, 0, 0, 8, 32, 1, 0, 1, out) == 0
    assert lib.dagl_fc_grad16_plan(0, 14, 38, 1, 0, 0, 8, 32, 1, 0, 1, out) == -1 and b"bad argument" in lib.dagl_last_error()
    assert lib.dagl_fc_grad16_plan(1, 13, 38, 1, 0, 0, 8, 32, 1, 0, 1, out) == -1          # the windows leave the map
    assert lib.dagl_fc_grad16_plan(1, 14, 38, 1, 0, 0, 8, 32, 1, 0, 1, None) == -1
    assert lib.dagl_fc_grad16_plan(1, 14, 38, 1, 0, 0, 8, 32, 1, 1, 1, out) == -1 and b"not both" in lib.dagl_last_error()
    assert lib.dagl_fc_grad16_plan(1, 9, 11, 1, 0, 0, 3, 5, 1, 0, 1, out) == -1 and b"fold" in lib.dagl_last_error()
    with pytest.raises(_lib.DaglError):
        plan_of(ops, _case("", 1, 3, 5), True, False, True)


def test_scratch_sizes_cover_the_plan_of_every_subset(ops):
    """The two scratch-size entries derive from the same planning functions as the call: a call that is handed one byte less than the
    entry reports is refused only if its own plan needs all of it -- and none needs more (fake pointers: nothing reaches the device)."""
    from dagl_amd import _lib
    lib = _lib.load()
    fake, ws = 0x10000, 0x100000
    for c in CASES:
        geo = (c["B"], c["Hp"], c["Wp"], c["stride"], c["oy"], c["ox"], c["oh"], c["ow"])
        need = lib.dagl_fc_grad16_scratch_bytes(c["B"], c["oh"], c["ow"])
        assert need > 0
        # a zero-byte scratch: every subset is refused by its size check, which names what it needs -- never more than `need`
        for d_w, d_b, d_rows in ((fake, fake, fake), (fake, None, None), (None, None, fake), (None, fake, None)):
            assert lib.dagl_fc_grad16(None, *geo, fake, fake, fake, fake, d_w, d_b, d_rows, ws, 0) == -1
            msg = lib.dagl_last_error().decode()
            assert "scratch 0 B, need " in msg, msg
            assert int(msg.split("need ")[1].split(" B")[0]) <= need, (c["name"], msg, need)
        if folds(c):
            need_m = lib.dagl_fc_grad16_dmap_scratch_bytes(c["B"], c["oh"], c["ow"])
            for d_w, d_map in ((fake, fake), (None, fake)):
                assert lib.dagl_fc_grad16_dmap(None, *geo, fake, fake, fake, fake, d_w, None, d_map, ws, 0) == -1
                msg = lib.dagl_last_error().decode()
                assert int(msg.split("need ")[1].split(" B")[0]) <= need_m, (c["name"], msg, need_m)
