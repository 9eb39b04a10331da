"""Host half of tests/test_gpu_gemm32_paths.py -- no GPU.  The cases the device test runs (defined here, imported there), the K-slice
count of every split-K case pinned by hand through ``dagl_gemm_f32_scratch_floats / (M * N)``, the head room that makes the device
test's tolerance zero -- with integer operands ``sum |a||b|`` of every output element stays below 2^24, so every partial sum in any
order is an exact fp32 integer --, and the argument checks of ``dagl_gemm_f32`` that never reach the device."""
import functools

import pytest
import torch

# the instance sweep: every (M, N) of SIZES^2 at every K, batch 1 and 3, on all of a_kc x b_kc x chunk_tiles
KS = (1, 15, 16, 17, 31, 32, 33, 113)          # 1..8 K-tiles of 16: both buffer parities, K tails, a chunk boundary (7) inside
SIZES = (1, 3, 4, 127, 128, 129)               # rows < 4 and rows % 4 != 0: the K-major loader's scalar tail; 129: a second tile
BATCHES = (1, 3)
CHUNKS = (0, 1, 7)
LAYOUTS = ((True, True), (True, False), (False, True), (False, False))

# (M, N, K) -> K slices of the split (1: no split) -- by hand from gemm32_auto_slices: tiles < 256 and K >= 4096 -> min(ceil(512 /
# tiles), K / 1024, 256); the launcher then gives every slice whole K-tiles: kc = ceil(ceil(K / slices) / 16) * 16
SPLIT_CASES = {
    (8, 8, 4095): 1,
    (8, 8, 4096): 4,
    (5, 7, 4100): 4,                            # kc = 1040: the last slice covers 980 k, a K tail
    (300, 130, 8200): 8,                        # six output tiles
    (8, 8, 102500): 100,                        # kc = 1040: 99 slices are launched
}
HOST_ONLY_SLICES = {(2048, 2048, 4096): 1, (128, 128, 400000): 256}
# the loader cases (a 4-byte offset, a leading dimension that is no multiple of 4) and the addressing cases run on these
LOADER_SHAPES = ((129, 127, 33), (4, 128, 113), (3, 5, 16), (128, 4, 17))
EPILOGUE = dict(alpha=0.5, beta=2.0)


def int_range(K):
    return 8 if K <= 128 else 3


@functools.lru_cache(maxsize=None)
def int_operands(nb, M, N, K):
    """Integer-valued fp32 operands A [nb, M, K], B [nb, K, N] in [-8, 8] (K <= 128) or [-3, 3], an integer C0 and bias."""
    g = torch.Generator().manual_seed(((nb * 1009 + M) * 1013 + N) * 1019 + K)
    r = int_range(K)
    A = torch.randint(-r, r + 1, (nb, M, K), generator=g).float()
    B = torch.randint(-r, r + 1, (nb, K, N), generator=g).float()
    C0 = torch.randint(-9, 10, (nb, M, N), generator=g).float()
    bias = torch.randint(-9, 10, (N,), generator=g).float()
    return A, B, C0, bias


def exact_product(A, B):
    return A.double() @ B.double()


def epilogue_of(prod64, C0, bias):
    return torch.relu(EPILOGUE["alpha"] * prod64 + EPILOGUE["beta"] * C0.double() + bias.double())


def headroom(A, B, C0, bias):
    """max over the outputs of sum |a||b| + |bias| + 2 |c0|: below 2^23 the product, its halves and the epilogue are all exact."""
    u = A.double().abs() @ B.double().abs()
    return float((u + bias.double().abs() + 2.0 * C0.double().abs()).max())


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


@pytest.mark.parametrize("case", sorted(SPLIT_CASES) + sorted(HOST_ONLY_SLICES))
def test_slice_counts_pinned_by_hand(lib, case):
    M, N, K = case
    want = {**SPLIT_CASES, **HOST_ONLY_SLICES}[case]
    floats = lib.dagl_gemm_f32_scratch_floats(1, M, N, K)
    assert floats % (M * N) == 0
    assert (floats // (M * N) or 1) == want, (case, floats)
    assert lib.dagl_gemm_f32_scratch_floats(2, M, N, K) == 0                      # a batch is never split


def launched_slices(K, slices):
    kc = -(-(-(-K // slices)) // 16) * 16
    return -(-K // kc), kc


def test_launched_slices_of_the_split_cases():
    """What the launcher makes of the slice count (whole K-tiles per slice): the classes the device cases are there for."""
    assert launched_slices(4096, 4) == (4, 1024)
    assert launched_slices(4100, 4) == (4, 1040) and 4100 - 3 * 1040 == 980
    assert launched_slices(8200, 8) == (8, 1040)
    assert launched_slices(102500, 100) == (99, 1040)


def test_sums_of_the_instance_sweep_stay_below_2_24():
    top = max(SIZES)
    for K in KS:
        A, B, C0, bias = int_operands(max(BATCHES), top, top, K)                  # every case is a sub-block of this product
        assert headroom(A, B, C0, bias) < 2 ** 23, K


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_sums_of_the_split_cases_stay_below_2_24(case):
    A, B, C0, bias = int_operands(2, *case)
    assert headroom(A, B, C0, bias) < 2 ** 23, case


def test_sums_of_the_loader_cases_stay_below_2_24():
    for shape in LOADER_SHAPES:
        assert headroom(*int_operands(3, *shape)) < 2 ** 23, shape


_FAKE = 0x10000


def _call(lib, batch=1, M=8, N=8, K=8, A=_FAKE, lda=8, B=_FAKE, ldb=8, C=_FAKE, ldc=8, chunk=0):
    return lib.dagl_gemm_f32(None, batch, M, N, K, A, lda, M * K, 1, B, ldb, N * K, 0, C, ldc, M * ldc, 1.0, 0.0, None, 0, chunk, None)


def test_argument_checks_before_the_device(lib):
    for bad in (dict(batch=0), dict(M=-1), dict(N=-1), dict(K=0), dict(lda=0), dict(ldb=0), dict(ldc=7), dict(chunk=-1)):
        assert _call(lib, **bad) == -1 and b"dagl_gemm_f32" in lib.dagl_last_error(), bad
    for null in ("A", "B", "C"):
        assert _call(lib, **{null: None}) == -1 and b"gemm32" in lib.dagl_last_error(), null


def test_an_empty_product_is_ok_without_a_device(lib):
    assert _call(lib, M=0) == 0 and _call(lib, N=0, ldc=1) == 0
    assert _call(lib, M=0, A=None, B=None, C=None) == 0
    assert lib.dagl_gemm_f32_scratch_floats(1, 0, 8, 8192) == 0 and lib.dagl_gemm_f32_scratch_floats(1, 8, 0, 8192) == 0
