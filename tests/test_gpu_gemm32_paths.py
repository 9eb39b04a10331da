"""``dagl_gemm_f32`` (gemm32.hip) path by path, bit for bit.  The f32-input MFMA multiplies exactly and accumulates in fp32, so with
small integer operands (tests/test_gemm32_paths_host.py proves ``sum |a||b| < 2^24`` for every case) every partial sum in any order is
an exact integer and the kernel must reproduce ``A.double() @ B.double()`` with ``torch.equal`` -- whatever the split, the chunking or
the wave order.  One misplaced term, a dropped K tile or a wrong halo fails.

Paths covered:
  * the eight straight-line instances ``gemm32_kernel<AKC, BKC, CHUNK>`` (a_kc x b_kc x chunk_tiles 0 / 1 / 7) at K of 1..8 K-tiles with
    tails, M and N of 1, 3, 4 (the K-major loader's scalar tail), 127, 128, 129 (a second tile), batch 1 and 3;
  * the vector and the scalar loaders of both layouts: an operand 4 bytes into its buffer or with a leading dimension that is no
    multiple of 4 (``vecA`` / ``vecB`` = 0) gives the bits of the aligned call;
  * split-K (``gemm32_reduce_kernel`` and the epilogue that moves into it): 1, 4, 8 and 99 launched slices, a K tail in the last slice,
    six output tiles, with and without chunked accumulation, against the unsplit chain (``split_k=False``) and a batch (never split),
    with the epilogue alpha = 0.5, beta = 2, integer bias, relu (exact), and a guard region behind the scratch;
  * addressing through the C entry: ``ldc > N`` (padding columns untouched, plain and split), ``stride_a = 0``, ``stride_c > M ldc``;
  * ``M = 0`` / ``N = 0``: OK, nothing written.
Not covered: the ``MLOOP`` instance (``gemm32_kernel<true, true, true, true>``) -- it is reachable only from overflow.hip through a
device-side row limit, not from this entry."""
import pytest
import torch

from tests.test_gemm32_paths_host import (BATCHES, CHUNKS, EPILOGUE, KS, LAYOUTS, LOADER_SHAPES, SIZES, SPLIT_CASES, epilogue_of,
                                          exact_product, int_operands)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN = -12345.5


def stored(A, Bm, akc, bkc):
    """[nb,M,K], [nb,K,N] -> the operands as the layout flags store them."""
    return (A if akc else A.transpose(1, 2)).contiguous(), (Bm.transpose(1, 2) if bkc else Bm).contiguous()


def raw_gemm(nb, M, N, K, a, lda, sa, akc, b, ldb, sb, bkc, c, ldc, sc, alpha=1.0, beta=0.0, bias=None, relu=False, chunk=0,
             scratch=None):
    """The C entry with every argument the wrapper fixes; a, b, c, scratch: device addresses."""
    from dagl_amd import _lib, ops
    _lib.check(_lib.load().dagl_gemm_f32(ops._stream(), nb, M, N, K, a, lda, sa, int(akc), b, ldb, sb, int(bkc), c, ldc, sc, alpha, beta,
                                         bias.data_ptr() if bias is not None else None, int(relu), chunk, scratch), "dagl_gemm_f32")


def placed(mat, ld, offset=0, stride=None):
    """A copy of mat [nb, rows, cols] in a pattern-filled device buffer, ``offset`` floats in, rows ``ld`` apart: (buffer, view, address)."""
    nb, rows, cols = mat.shape
    stride = rows * ld if stride is None else stride
    buf = torch.full((offset + nb * stride + 8,), PATTERN, device=DEV)
    view = buf[offset:].as_strided((nb, rows, cols), (stride, ld, 1))
    view.copy_(mat)
    return buf, view, buf.data_ptr() + 4 * offset


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_every_instance_is_exact_on_integers(akc, bkc, chunk):
    """One full product per K on the CPU; every (batch, M, N) case is a sub-block of it."""
    from dagl_amd import ops
    top, nbt = max(SIZES), max(BATCHES)
    for K in KS:
        A, Bm, _, _ = int_operands(nbt, top, top, K)
        want = exact_product(A, Bm).float().to(DEV)
        Ad, Bd = A.to(DEV), Bm.to(DEV)
        for nb in BATCHES:
            for M in SIZES:
                for N in SIZES:
                    a_st, b_st = stored(Ad[:nb, :M], Bd[:nb, :, :N], akc, bkc)
                    out = torch.full((nb, M, N), float("nan"), device=DEV)
                    got = ops.gemm_f32(a_st, b_st, a_k_contiguous=akc, b_k_contiguous=bkc, out=out, chunk_tiles=chunk)
                    assert torch.equal(got, want[:nb, :M, :N]), (akc, bkc, chunk, K, nb, M, N)


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_scalar_loaders_give_the_bits_of_the_vector_loaders(akc, bkc):
    """A or B starting 4 bytes into its buffer, or with lda / ldb no multiple of 4: the scalar loads, the same integers."""
    nb = 3
    for M, N, K in LOADER_SHAPES:
        A, Bm, _, _ = int_operands(nb, M, N, K)
        want = exact_product(A, Bm).float().to(DEV)
        a_st, b_st = stored(A.to(DEV), Bm.to(DEV), akc, bkc)
        ra, ca = a_st.shape[1:]; rb, cb = b_st.shape[1:]
        up4 = lambda n: -(-n // 4) * 4
        for chunk in (0, 7):
            res = {}
            # (offset of A, lda, offset of B, ldb): aligned with a padded leading dimension first, then one thing off at a time
            for name, oa, lda, ob, ldb in (("aligned", 0, up4(ca) + 4, 0, up4(cb) + 4), ("A + 4 bytes", 1, up4(ca) + 4, 0, up4(cb) + 4),
                                           ("B + 4 bytes", 0, up4(ca) + 4, 1, up4(cb) + 4), ("lda odd", 0, up4(ca) + 1, 0, up4(cb) + 4),
                                           ("ldb odd", 0, up4(ca) + 4, 0, up4(cb) + 3), ("all off", 3, up4(ca) + 2, 1, up4(cb) + 1)):
                abuf, _, ap = placed(a_st, lda, oa)
                bbuf, _, bp = placed(b_st, ldb, ob)
                out = torch.full((nb, M, N), float("nan"), device=DEV)
                raw_gemm(nb, M, N, K, ap, lda, ra * lda, akc, bp, ldb, rb * ldb, bkc, out.data_ptr(), N, M * N, chunk=chunk)
                res[name] = out
                assert torch.equal(out, want), (name, akc, bkc, chunk, M, N, K)
            assert all(torch.equal(res["aligned"], r) for r in res.values())


def _split_call(lib, a_st, b_st, akc, bkc, M, N, K, chunk, epilogue, C0d, biasd, guard=64):
    """One batch-1 call with the scratch the library asks for and a pattern-filled guard behind it -> (C, launched the split)."""
    nf = lib.dagl_gemm_f32_scratch_floats(1, M, N, K)
    scr = torch.full((nf + guard,), PATTERN, device=DEV)
    out = C0d.clone() if epilogue else torch.full((1, M, N), float("nan"), device=DEV)
    kw = dict(alpha=EPILOGUE["alpha"], beta=EPILOGUE["beta"], bias=biasd, relu=True) if epilogue else {}
    raw_gemm(1, M, N, K, a_st.data_ptr(), a_st.shape[2], a_st.shape[1] * a_st.shape[2], akc, b_st.data_ptr(), b_st.shape[2],
             b_st.shape[1] * b_st.shape[2], bkc, out.data_ptr(), N, M * N, chunk=chunk, scratch=scr.data_ptr() if nf else None, **kw)
    assert bool((scr[nf:] == PATTERN).all()), "the guard behind the scratch was written"
    if nf:
        assert not bool((scr[:nf] == PATTERN).all())          # the slices did go through the scratch
    return out


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_split_k_is_exact_on_integers(case, akc, bkc):
    from dagl_amd import _lib, ops
    lib = _lib.load()
    M, N, K = case
    A, Bm, C0, bias = int_operands(2, M, N, K)
    prod = exact_product(A, Bm)
    want = prod.float().to(DEV)
    want_epi = epilogue_of(prod, C0, bias).float().to(DEV)
    a2, b2 = stored(A.to(DEV), Bm.to(DEV), akc, bkc)
    a1, b1 = a2[:1].contiguous(), b2[:1].contiguous()
    C0d, biasd = C0.to(DEV), bias.to(DEV)
    for chunk in (0, 7):
        what = (case, akc, bkc, chunk)
        assert torch.equal(_split_call(lib, a1, b1, akc, bkc, M, N, K, chunk, False, None, None), want[:1]), what
        assert torch.equal(_split_call(lib, a1, b1, akc, bkc, M, N, K, chunk, True, C0d[:1], biasd), want_epi[:1]), what
        # one chain, no split
        assert torch.equal(ops.gemm_f32(a1, b1, akc, bkc, chunk_tiles=chunk, split_k=False), want[:1]), what
        out = C0d[:1].clone()
        ops.gemm_f32(a1, b1, akc, bkc, out=out, bias=biasd, relu=True, chunk_tiles=chunk, split_k=False, **EPILOGUE)
        assert torch.equal(out, want_epi[:1]), what
        # a batch is not split
        assert torch.equal(ops.gemm_f32(a2, b2, akc, bkc, chunk_tiles=chunk), want), what
        out = C0d.clone()
        ops.gemm_f32(a2, b2, akc, bkc, out=out, bias=biasd, relu=True, chunk_tiles=chunk, **EPILOGUE)
        assert torch.equal(out, want_epi), what


@pytest.mark.parametrize("shape", [(129, 127, 33), (5, 7, 4100), (300, 130, 8200)])
def test_padding_columns_of_c_stay_untouched(shape):
    """ldc = N + 3, plain and split-K: the three padding columns of every row keep their pattern."""
    from dagl_amd import _lib
    lib = _lib.load()
    M, N, K = shape
    A, Bm, C0, bias = int_operands(2, M, N, K)
    A, Bm, C0 = A[:1], Bm[:1], C0[:1]
    prod = exact_product(A, Bm)
    a_st, b_st = stored(A.to(DEV), Bm.to(DEV), True, False)
    nf = lib.dagl_gemm_f32_scratch_floats(1, M, N, K)
    assert (nf > 0) == (K >= 4096)
    scr = torch.full((max(nf, 1) + 64,), PATTERN, device=DEV)
    ldc = N + 3
    for epilogue in (False, True):
        cbuf, cview, cp = placed(C0.to(DEV), ldc)
        kw = dict(bias=bias.to(DEV), relu=True, **EPILOGUE) if epilogue else {}
        raw_gemm(1, M, N, K, a_st.data_ptr(), K, M * K, True, b_st.data_ptr(), N, K * N, False, cp, ldc, M * ldc, chunk=7,
                 scratch=scr.data_ptr() if nf else None, **kw)
        want = (epilogue_of(prod, C0, bias) if epilogue else prod).float().to(DEV)
        assert torch.equal(cview, want), (shape, epilogue)
        pad = cbuf[:M * ldc].view(M, ldc)[:, N:]
        assert bool((pad == PATTERN).all()) and bool((cbuf[M * ldc:] == PATTERN).all()), (shape, epilogue)
        assert bool((scr[nf:] == PATTERN).all())


@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_batch_strides_that_are_not_dense(akc, bkc):
    """stride_a = 0 (one A shared by the batch), stride_b with a gap, stride_c larger than M ldc (the gaps keep their pattern)."""
    nb, (M, N, K) = 3, LOADER_SHAPES[0]
    A, Bm, _, _ = int_operands(nb, M, N, K)
    want = exact_product(A[:1].expand(nb, M, K), Bm).float().to(DEV)
    a_st, b_st = stored(A[:1].to(DEV), Bm.to(DEV), akc, bkc)
    rb, cb = b_st.shape[1:]
    sb, sc = rb * cb + 20, M * N + 37
    bbuf, _, bp = placed(b_st, cb, 0, stride=sb)
    cbuf, cview, cp = placed(torch.full((nb, M, N), float("nan"), device=DEV), N, 0, stride=sc)
    raw_gemm(nb, M, N, K, a_st.data_ptr(), a_st.shape[2], 0, akc, bp, cb, sb, bkc, cp, N, sc, chunk=1)
    assert torch.equal(cview, want)
    gaps = cbuf[:nb * sc].view(nb, sc)[:, M * N:]
    assert bool((gaps == PATTERN).all()) and bool((cbuf[nb * sc:] == PATTERN).all())


def test_an_empty_product_writes_nothing():
    from dagl_amd import _lib, ops
    lib = _lib.load()
    A = torch.ones(8, 16, device=DEV); Bm = torch.ones(16, 8, device=DEV)
    out = torch.full((64,), PATTERN, device=DEV)
    for M, N in ((0, 8), (8, 0), (0, 0)):
        rc = lib.dagl_gemm_f32(ops._stream(), 1, M, N, 16, A.data_ptr(), 16, 128, 1, Bm.data_ptr(), 8, 128, 0, out.data_ptr(), 8, 64, 1.0, 0.0,
                               None, 0, 0, None)
        assert rc == 0, (M, N)
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())
