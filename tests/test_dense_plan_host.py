"""The dense training core's launch plan (dense_train.hip, dt_plan) and its chunk budget, without a GPU: the plan
``dagl_ce_core_dense_plan`` reports against plans derived by hand from dt_plan, the budget setter
``dagl_ce_core_dense_chunk_floats`` and its context manager, and the refusal of a workspace sized under a smaller budget (fake
pointers, as in test_abi_symbols.py: every call is rejected before anything reaches the device)."""
import ctypes as C

import pytest

from tests.test_abi_symbols import lib_path  # noqa: F401  (fixture)

DEFAULT = 128 << 20          # floats per [chunk, N] matrix: the built-in budget
_FAKE = 0x10000
_WS = 0x100000


@pytest.fixture()
def ops(lib_path):  # noqa: F811
    from dagl_amd import _lib, ops
    lib = _lib.load()
    lib.dagl_ce_core_dense_chunk_floats(0)
    yield ops
    lib.dagl_ce_core_dense_chunk_floats(0)


# By hand from dt_plan at 128 Mi floats (L = ceil(H/4) ceil(W/4), N = H W, ldn = N rounded up to 32):
#  (1,216,216): ldn 46656, 2^27 / 46656 = 2876 -> 2816 queries per chunk (multiple of 128), L = 2916 -> 2 chunks, so Bc = 1 and fp32 products
#  (9,128,128): L 1024 in one chunk of 2^24 floats -> 8 images per group, last group of one; one chunk -> fp16 products
#  (8,128,128): 8 x 2 x 8 = 128 output tiles of d Wq -> split K by 2 (256), by 4 (512 tiles: stop)
#  (2,45,38):   N 1710, 4 tiles: split by 2 (N >= 512), by 4 (N >= 1024), not by 8 (N < 2048); nk = 1710 rounded up to 128 = 1792
#  (1,19,25):   N 475 < 512: no split
#  (1,47,45):   N 2115 >= 2048: split by 8; nk = 2115 rounded up to 256 = 2304
@pytest.mark.parametrize("shape,want", [
    ((1, 216, 216), dict(Lc=2816, n_chunks=2, Bc=1, h16=0)),
    ((9, 128, 128), dict(n_chunks=1, Bc=8, h16=1)),
    ((8, 128, 128), dict(kslices=4)),
    ((2, 45, 38), dict(kslices=4, nk=1792)),
    ((1, 19, 25), dict(kslices=1)),
    ((1, 47, 45), dict(kslices=8, nk=2304)),
])
def test_default_plans_match_the_hand_derived_ones(ops, shape, want):
    plan = ops.dense_plan(*shape, backward=True)
    assert sorted(plan) == sorted(ops.DENSE_PLAN_FIELDS)
    assert {k: plan[k] for k in want} == want, plan
    assert ops.dense_plan(*shape, backward=False)["h16"] == 0          # the forward has no fp16 products to plan


def test_plan_rejects_bad_arguments(ops):
    from dagl_amd import _lib
    lib = _lib.load()
    assert lib.dagl_ce_core_dense_plan(0, 8, 8, 1, (C.c_int32 * 6)()) == -1
    assert lib.dagl_ce_core_dense_plan(1, 8, 8, 1, None) == -1
    with pytest.raises(_lib.DaglError):
        ops.dense_plan(1, 0, 8)


def test_setter_returns_the_previous_value_and_zero_restores_the_default(ops):
    from dagl_amd import _lib
    lib = _lib.load()
    assert lib.dagl_ce_core_dense_chunk_floats(1000) == DEFAULT
    assert lib.dagl_ce_core_dense_chunk_floats(2000) == 1000
    assert lib.dagl_ce_core_dense_chunk_floats(0) == 2000
    assert lib.dagl_ce_core_dense_chunk_floats(0) == DEFAULT
    assert ops.dense_plan(1, 216, 216)["Lc"] == 2816


def test_small_budgets_give_the_chunked_and_grouped_plans(ops):
    with ops.dense_chunk_budget(128 * 4352):
        p = ops.dense_plan(1, 64, 68)
        assert (p["Lc"], p["n_chunks"], p["Bc"], p["h16"]) == (128, 3, 1, 0)          # 272 queries = 128 + 128 + 16
    with ops.dense_chunk_budget(2 * 128 * 1728):
        p = ops.dense_plan(5, 45, 38)
        assert (p["Lc"], p["n_chunks"], p["Bc"], p["h16"]) == (120, 1, 2, 1)          # groups of 2, 2, 1 images
    with ops.dense_chunk_budget(1):                                                    # a chunk never has fewer than 128 queries
        p = ops.dense_plan(2, 48, 50)
        assert (p["Lc"], p["n_chunks"], p["Bc"]) == (128, 2, 1)


@pytest.mark.parametrize("backward", [0, 1])
def test_workspace_bytes_follow_the_budget(ops, backward):
    from dagl_amd import _lib
    lib = _lib.load()
    full = lib.dagl_ce_core_dense_workspace_bytes(5, 45, 38, backward)
    with ops.dense_chunk_budget(2 * 128 * 1728):
        assert 0 < lib.dagl_ce_core_dense_workspace_bytes(5, 45, 38, backward) < full
    assert lib.dagl_ce_core_dense_workspace_bytes(5, 45, 38, backward) == full


def test_context_manager_restores_the_plan_also_when_the_body_raises(ops):
    default = ops.dense_plan(1, 216, 216)
    with ops.dense_chunk_budget(128 * 46656) as before:
        assert before == DEFAULT
        assert ops.dense_plan(1, 216, 216)["n_chunks"] == 23
        with ops.dense_chunk_budget(0):                                # nests: the inner one puts the outer budget back
            assert ops.dense_plan(1, 216, 216) == default
        assert ops.dense_plan(1, 216, 216)["n_chunks"] == 23
    assert ops.dense_plan(1, 216, 216) == default
    with pytest.raises(ZeroDivisionError):
        with ops.dense_chunk_budget(128 * 46656):
            assert ops.dense_plan(1, 216, 216)["Lc"] == 128
            1 / 0
    assert ops.dense_plan(1, 216, 216) == default


def test_workspace_sized_under_a_small_budget_is_refused_under_the_default(ops):
    """Nothing reaches the device: the pointers are fake, both calls return ERR_WORKSPACE from their size check."""
    from dagl_amd import _lib
    lib = _lib.load()
    B, H, W = 5, 45, 38
    with ops.dense_chunk_budget(2 * 128 * 1728):
        small_f = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256
        small_b = lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 1)
    assert small_f < lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256 and small_b < lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 1)
    p = [_FAKE] * 5
    info = _lib.CeInfo()
    rc = lib.dagl_ce_core_dense_forward(None, B, H, W, 0, *p, _FAKE, _FAKE, _FAKE, _WS, small_f, C.byref(info))
    assert rc == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    assert info.required_bytes == lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256
    rc = lib.dagl_ce_core_dense_backward(None, B, H, W, 0, *p, _FAKE, _FAKE, _FAKE, *([_FAKE] * 5), _WS, small_b)
    assert rc == _lib.ERR_WORKSPACE and b"workspace" in lib.dagl_last_error()
    for mode in (_lib.MODE_TOPK, _lib.MODE_ADAPTIVE_TOPK):             # the wide entry points plan with the same budget
        assert lib.dagl_ce_core_wide_forward(None, B, H, W, mode, 100, *p, _FAKE, _WS, small_f, None) == _lib.ERR_WORKSPACE
        assert lib.dagl_ce_core_wide_backward(None, B, H, W, mode, 100, *p, _FAKE, *([_FAKE] * 5), _WS, small_b) == _lib.ERR_WORKSPACE
