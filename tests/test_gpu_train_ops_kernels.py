"""The stages of the differentiable path that are not matrix products (train_ops.hip), each on its own against a plain CPU reference.
They move or select values, or add a handful of them, so every check but two is bit for bit.

Paths covered:
  * ``dagl_unfold_patches``: bit-equal to indexing the padded NHWC map; k of 1, 3, 7, stride 1 and 4, C of 4, 16, 64, B of 1 and 3,
    zero and non-zero offsets, windows that end exactly on the map's last row and column, float4 counts that leave idle threads;
  * ``dagl_fold_patches``: integer rows against a scatter-add in fp64 (exact), the same geometries (stride 4 with k of 1 and 3 leaves
    gaps: uncovered pixels are written as 0 over a NaN-filled map), and the adjoint identity <unfold(m), r> = <m, fold(r)> exactly;
  * ``dagl_copy4``: bit-equal to torch's strided copy over every axis permutation, a source stride of 0, n3 = 1, a destination with
    gaps (which keep their pattern);
  * ``dagl_relu_backward``: y with 0, -0, negatives and NaN; n of 0, 1, 255, 257;
  * ``dagl_col_sum``: cols of 1..256 x rows of 1..64*256+1 (more than 64 partials); integers exact; for randn the derived bound
    |got - ref| <= 2^-24 |ref| + rows 2^-52 sum|x| per column (fp64 accumulation, one cast); a repeated call bit-equal; rows = 0 gives
    zeros without touching the scratch (``dagl_col_sum_scratch_bytes(0, cols)`` is 0);
  * ``dagl_prelu_forward`` / ``_backward``: n around one block's 2048 float4, a negative slope, x with 0 and -0: forward and dx
    bit-equal to torch, d slope within 1e-6 of fp64.
The matrix products these stages sit between are tests/test_gpu_gemm32_paths.py (everything but the ``MLOOP`` instance of
``gemm32_kernel``, which no entry tested here or there reaches)."""
import itertools

import pytest
import torch

from tests.test_train_ops_kernels_host import (COL_SUM_COLS, COL_SUM_ROWS, GEOMETRIES, PRELU_SIZES, fold_ref, gid, int_map_and_rows,
                                               unfold_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN = -12345.5


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_unfold_is_the_indexed_map(g):
    from dagl_amd import ops
    B, C, k, stride, oy, ox, oh, ow, Hp, Wp = g
    pmap = torch.randn(B, Hp, Wp, C, generator=torch.Generator().manual_seed(Hp * 31 + Wp))
    pmap[0, 0, 0, 0] = -0.0
    got = ops.unfold_patches(pmap.to(DEV), k, stride, oy, ox, oh, ow).cpu()
    want = unfold_ref(pmap, k, stride, oy, ox, oh, ow)
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_fold_is_the_exact_adjoint(g):
    from dagl_amd import _lib, ops
    B, C, k, stride, oy, ox, oh, ow, Hp, Wp = g
    pmap, rows = int_map_and_rows(g)
    rd = rows.to(DEV)
    d_map = torch.full((B * Hp * Wp * C + 64,), float("nan"), device=DEV)
    d_map[B * Hp * Wp * C:] = PATTERN
    _lib.check(_lib.load().dagl_fold_patches(ops._stream(), B, Hp, Wp, C, k, stride, oy, ox, oh, ow, rd.data_ptr(), d_map.data_ptr()),
               "dagl_fold_patches")
    got = d_map[:B * Hp * Wp * C].view(B, Hp, Wp, C).cpu()
    assert bool((d_map[B * Hp * Wp * C:] == PATTERN).all())
    want = fold_ref(rows, (B, Hp, Wp, C), k, stride, oy, ox, oh, ow)
    assert torch.equal(got, want.float())
    covered = fold_ref(torch.ones_like(rows), (B, Hp, Wp, C), k, stride, oy, ox, oh, ow) > 0
    assert bool((bits(got)[~covered] == 0).all())                        # pixels no window covers: written, as +0
    assert torch.equal(ops.fold_patches(rd, (B, Hp, Wp, C), k, stride, oy, ox, oh, ow).cpu(), got)
    unf = ops.unfold_patches(pmap.to(DEV), k, stride, oy, ox, oh, ow).cpu()
    assert float((unf.double() * rows.double()).sum()) == float((pmap.double() * got.double()).sum())


def _copy4_case(src, sizes, s_strides, dst_numel, d_strides):
    """One copy into a pattern-filled destination against torch's strided copy -> nothing; asserts."""
    from dagl_amd import ops
    dst = torch.full((dst_numel,), PATTERN, device=DEV)
    ops.copy4(src, sizes, s_strides, dst, d_strides)
    want = torch.full((dst_numel,), PATTERN, device=DEV)
    want.as_strided(sizes, d_strides).copy_(src.as_strided(sizes, s_strides))
    assert torch.equal(bits(dst), bits(want)), (sizes, s_strides, d_strides)


@pytest.mark.parametrize("sizes", [(3, 5, 7, 2), (2, 3, 43, 1), (1, 1, 1, 257), (5, 1, 51, 1)])
def test_copy4_is_torchs_strided_copy(sizes):
    n = sizes[0] * sizes[1] * sizes[2] * sizes[3]
    assert n % 256 != 0
    src = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    contiguous = lambda shape: tuple(int(torch.tensor(shape[i + 1:]).prod()) if i < 3 else 1 for i in range(4))
    s_strides = contiguous(sizes)
    for perm in itertools.permutations(range(4)):                        # destination axes in the order perm: every transposition
        d_shape = [sizes[p] for p in perm]
        d_contig = contiguous(d_shape)
        d_strides = tuple(d_contig[perm.index(a)] for a in range(4))
        _copy4_case(src, sizes, s_strides, n, d_strides)
        _copy4_case(src, sizes, d_strides, n, s_strides)                 # ... and read through the permuted strides
    # a source stride of 0 on each axis (a broadcast), into a dense destination
    for axis in range(4):
        st = list(s_strides); st[axis] = 0
        _copy4_case(src, sizes, tuple(st), n, s_strides)
    # a destination with gaps: every second element, and padded rows; what the strides do not address keeps its pattern
    _copy4_case(src, sizes, s_strides, 2 * n, tuple(2 * s for s in s_strides))
    pad = (sizes[1] * sizes[2] * (sizes[3] + 3), sizes[2] * (sizes[3] + 3), sizes[3] + 3, 1)
    _copy4_case(src, sizes, s_strides, sizes[0] * pad[0], pad)


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_relu_backward_masks_bit_for_bit(n):
    from dagl_amd import _lib, ops
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([0.0, -0.0, -1.5, float("nan"), 2.0, float("inf"), float("-inf")])
    y = torch.randn(max(n, 1), generator=g)
    y[:min(n, 7)] = special[:min(n, 7)]
    if n > 7:
        y[-7:] = special
    dy = torch.randn(max(n, 1), generator=g)
    if n == 0:
        out = torch.full((4,), PATTERN, device=DEV)
        assert _lib.load().dagl_relu_backward(ops._stream(), 0, y.to(DEV).data_ptr(), dy.to(DEV).data_ptr(), out.data_ptr()) == 0
        assert bool((out == PATTERN).all())
        return
    got = ops.relu_backward(y.to(DEV), dy.to(DEV)).cpu()
    want = torch.where(y > 0, dy, torch.zeros(()))
    assert torch.equal(bits(got), bits(want))


def _col_sum(lib, xd, rows, cols, guard=32):
    from dagl_amd import ops
    nbytes = lib.dagl_col_sum_scratch_bytes(rows, cols)
    assert nbytes == -(-rows // 256) * cols * 8
    scr = torch.full((nbytes // 4 + guard,), PATTERN, device=DEV)
    out = torch.full((cols + guard,), float("nan"), device=DEV)
    out[cols:] = PATTERN
    rc = lib.dagl_col_sum(ops._stream(), rows, cols, xd.data_ptr() if rows else None, out.data_ptr(), scr.data_ptr() if nbytes else None)
    assert rc == 0, lib.dagl_last_error()
    assert bool((scr[nbytes // 4:] == PATTERN).all()) and bool((out[cols:] == PATTERN).all())
    return out[:cols].cpu()


@pytest.mark.parametrize("cols", COL_SUM_COLS)
def test_col_sum_exact_on_integers_and_within_the_fp64_bound(cols):
    from dagl_amd import _lib
    lib = _lib.load()
    top = max(COL_SUM_ROWS)
    g = torch.Generator().manual_seed(cols)
    xi = torch.randint(-8, 9, (top, cols), generator=g).float()
    xr = torch.randn(top, cols, generator=g)
    xid, xrd = xi.to(DEV), xr.to(DEV)
    for rows in COL_SUM_ROWS:                                            # the first `rows` rows of a contiguous matrix are one too
        got = _col_sum(lib, xid, rows, cols)
        assert torch.equal(got, xi[:rows].double().sum(0).float()), (rows, cols)
        got = _col_sum(lib, xrd, rows, cols)
        ref = xr[:rows].double().sum(0)
        bound = 2.0 ** -24 * ref.abs() + rows * 2.0 ** -52 * xr[:rows].double().abs().sum(0)
        assert bool(((got.double() - ref).abs() <= bound).all()), (rows, cols, float(((got.double() - ref).abs() / bound).max()))
        assert torch.equal(bits(_col_sum(lib, xrd, rows, cols)), bits(got)), (rows, cols)


@pytest.mark.parametrize("cols", [1, 20, 256])
def test_col_sum_of_no_rows_is_zero_and_leaves_the_scratch_alone(cols):
    """dagl_col_sum_scratch_bytes(0, cols) is 0: the call writes zeros into out and touches no scratch, given or not."""
    from dagl_amd import _lib, ops
    lib = _lib.load()
    assert lib.dagl_col_sum_scratch_bytes(0, cols) == 0
    assert torch.equal(bits(_col_sum(lib, None, 0, cols)), torch.zeros(cols, dtype=torch.int32))
    scr = torch.full((cols * 2 + 8,), PATTERN, device=DEV)             # a scratch handed in anyway stays as it is
    out = torch.full((cols,), float("nan"), device=DEV)
    src = torch.ones(cols, device=DEV)
    assert lib.dagl_col_sum(ops._stream(), 0, cols, src.data_ptr(), out.data_ptr(), scr.data_ptr()) == 0
    assert bool((out == 0).all()) and bool((scr == PATTERN).all())


@pytest.mark.parametrize("slope", [0.2, -0.25])
@pytest.mark.parametrize("n", PRELU_SIZES)
def test_prelu_around_one_block(n, slope):
    import torch.nn.functional as F
    from dagl_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g); dy = torch.randn(n, generator=g)
    x[0], x[1], x[-1], x[-2] = 0.0, -0.0, -0.0, 0.0
    a = torch.tensor([slope])
    xd, dyd, ad = x.to(DEV), dy.to(DEV), a.to(DEV)
    y = ops.prelu_forward(xd, ad).cpu()
    dx, da = (t.cpu() for t in ops.prelu_backward(xd, dyd, ad))
    assert torch.equal(bits(y), bits(torch.where(x > 0, x, a * x))) and torch.equal(y, F.prelu(x, a))
    xr, ar = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    F.prelu(xr, ar).backward(dy)
    assert torch.equal(bits(dx), bits(torch.where(x > 0, dy, a * dy))) and torch.equal(dx, xr.grad)
    ref64 = float((dy.double() * x.double() * (x <= 0)).sum())
    assert abs(float(da) - ref64) <= 1e-6 * abs(ref64) + 1e-6, (float(da), ref64)
    dx2, da2 = ops.prelu_backward(xd, dyd, ad)
    assert torch.equal(bits(da2.cpu()), bits(da)) and torch.equal(bits(dx2.cpu()), bits(dx))
