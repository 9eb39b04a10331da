"""The trunk convolution kernels (csrc/trunk.hip) over their whole claimed scope, called through dagl_amd.ops so that every operand is
the test's: every channel-padding class, k-split of the weight gradient, column-tile seam, strip length and epilogue operand, against
torch.nn.functional.conv2d on the CPU in float64 (the epilogues written out as plain formulas), with the same computation on the
CPU in float32 as the yardstick: test_gpu_trunk._bound, e_lib <= 3 e_cpu32 + 1e-6 normwise, per output tensor.  Then guard bands
around every output, the unaligned-operand fall-back bit for bit, determinism and the footprint of a non-finite input.

The case table is module-level: tests/test_trunk_host.py checks, from the library's host-callable functions alone, that it keeps
reaching the tiling classes it was chosen for."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_trunk import _bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (Cin, Cout): every 4-channel k-step class (1, 2, 4, 8, 16) and 16-channel group count (1, 2, 3 padded to 4, 4) on both sides,
# every (n_pairs, ksplit, grid.y) of the weight gradient: (1, 8, 1) (2, 4, 1) (4, 2, 1) (8, 1, 1) (16, 1, 2)
PAIRS = ((1, 1), (2, 5), (4, 4), (5, 7), (8, 16), (12, 20), (16, 17), (17, 16), (20, 33), (24, 48), (31, 32), (32, 31), (33, 5),
         (40, 9), (48, 49), (49, 48), (63, 64), (64, 63))
# (B, H, W): 1, 2 and 3 column tiles in the forward (tile 128), 1, 2, 3 and 5 in the weight gradient (tile 64), the seams at
# 63..66 and 127..131, W % 4 of every kind, H <= 3 (halo rows outside the image on both sides), strips of 1, 2, 4, 6 and 12 rows
SHAPES = ((1, 1, 1), (1, 1, 17), (2, 2, 16), (1, 3, 15), (1, 5, 63), (2, 7, 64), (1, 4, 65), (1, 6, 66), (1, 9, 127), (2, 5, 128),
          (1, 4, 129), (1, 3, 130), (1, 70, 131), (1, 2, 257), (3, 33, 36), (1, 130, 20), (1, 300, 260))
# (B, Cin, Cout, H, W), ksize 3: the 64-row cap of a strip in both kernels, the three-level k-split tree at full strip length
LARGE = (2, 4, 4, 1100, 1030)
# ksize 1 runs all SHAPES over these: still every k-step class on both sides and every n_pairs value
K1_PAIRS = ((1, 1), (2, 5), (8, 16), (16, 17), (20, 33), (33, 5), (31, 32), (63, 64))
EPI_PAIRS = ((5, 7), (12, 20), (32, 32), (64, 33))
EPI_SHAPES = ((1, 5, 37), (2, 3, 130), (1, 9, 66), (1, 2, 257), (2, 8, 64))
# one channel pair per n_pairs value 1, 2, 4, 8, 16
DET_PAIRS = ((4, 4), (16, 17), (31, 32), (20, 33), (63, 64))

DTYPES = (("64", torch.float64), ("32", torch.float32))


def _np(t):
    return t.detach().cpu().double().numpy()


def _inputs(cin, cout, k, shape, seed):
    """Weight, bias, input and upstream gradient (or residual) of a case.  The input and the upstream gradient are N(0.5, 1), not
    zero-mean: with one output channel d_b is ONE sum over B H W terms (and d_w of a 1 -> 1 1x1 layer one sum of products), and a sum
    of zero-mean terms can come out a hundred times smaller than its partial sums.  A normwise bound on such a scalar measures the
    cancellation, not the kernel: 1 -> 1 3x3 at (1, 3, 15), zero-mean, had d_b = -0.297 from terms with sum |dy| = 32.5; the library
    was off by 4.6e-7 (one rounding of a partial sum above 4, e 1.56e-6) where torch's CPU order happened to round exactly
    (e_cpu32 5.0e-8).  With the mean the sums grow like their term counts and every order is judged by its rounding."""
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    x = 0.5 + torch.randn(B, cin, H, W, generator=g)
    up = 0.5 + torch.randn(B, cout, H, W, generator=g)
    return w, b, x, up


def _seed(pair, k, shape):
    return 1000003 * pair[0] + 10007 * pair[1] + 101 * k + 7 * shape[1] + shape[2]


def _stock(w, b, x, up, k):
    """{'64' / '32': (out, d_x, d_w, d_b)} of the stock layer on the CPU."""
    ref = {}
    for tag, dt in DTYPES:
        wi, bi, xi = (t.to(dt).requires_grad_(True) for t in (w, b, x))
        y = F.conv2d(xi, wi, bi, padding=k // 2)
        ref[tag] = (y.detach(),) + torch.autograd.grad(y, (xi, wi, bi), up.to(dt))
    return ref


def _plain_case(pair, k, shape):
    from dagl_amd import ops
    cin, cout = pair
    w, b, x, up = _inputs(cin, cout, k, shape, _seed(pair, k, shape))
    ref = _stock(w, b, x, up, k)
    wd, bd, xd, upd = (t.to(DEV) for t in (w, b, x, up))
    out, _ = ops.trunk_conv_forward(xd, ops.trunk_pack_weights(wd), bd, cout, k)
    d_x, _ = ops.trunk_conv_input_grad(upd, ops.trunk_pack_weights(wd, True), cin, k)
    d_w, d_b, _ = ops.trunk_conv_weight_grad(xd, upd, k)
    for name, a, r64, r32 in zip(("out", "d_x", "d_w", "d_b"), (out, d_x, d_w, d_b), ref["64"], ref["32"]):
        assert a.shape == r64.shape, (pair, k, shape, name)
        _bound(_np(a), r64.numpy(), _np(r32), (pair, k, shape, name))


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_conv3x3_table_vs_fp64(pair):
    for shape in SHAPES:
        _plain_case(pair, 3, shape)


@pytest.mark.parametrize("pair", K1_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_conv1x1_table_vs_fp64(pair):
    for shape in SHAPES:
        _plain_case(pair, 1, shape)


def test_large_map_reaches_the_row_cap():
    B, cin, cout, H, W = LARGE
    _plain_case((cin, cout), 3, (B, H, W))


def _prelu(z, a):
    return torch.where(z > 0, z, a * z)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("pair", EPI_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_forward_epilogues_vs_fp64(pair, k):
    """z = conv + b; u = where(z > 0, z, a z); out = u * res_scale + residual, every operand optional."""
    from dagl_amd import ops
    cin, cout = pair
    for shape in EPI_SHAPES:
        w, b, x, res = _inputs(cin, cout, k, shape, _seed(pair, k, shape) + 1)
        slope = torch.tensor([0.2])
        conv = {tag: F.conv2d(x.to(dt), w.to(dt), None, padding=k // 2) for tag, dt in DTYPES}
        wd, bd, xd, resd, sd = (t.to(DEV) for t in (w, b, x, res, slope))
        packed = ops.trunk_pack_weights(wd)
        for bias in (True, False):
            for act in ("none", "slope", "slope+pre"):
                for rs in (None, 1.0, 0.1):
                    want = {}
                    for tag, dt in DTYPES:
                        z = conv[tag] + b.to(dt).view(1, -1, 1, 1) if bias else conv[tag]
                        u = _prelu(z, slope.to(dt)) if act != "none" else z
                        want[tag] = (u * rs + res.to(dt) if rs is not None else u, z)
                    out, pre = ops.trunk_conv_forward(xd, packed, bd if bias else None, cout, k, slope=sd if act != "none" else None,
                                                      want_pre=act == "slope+pre", res_scale=1.0 if rs is None else rs,
                                                      residual=resd if rs is not None else None)
                    what = (pair, k, shape, "bias" if bias else "no bias", act, rs)
                    _bound(_np(out), want["64"][0].numpy(), _np(want["32"][0]), what + ("out",))
                    assert (pre is not None) == (act == "slope+pre"), what
                    if pre is not None:
                        _bound(_np(pre), want["64"][1].numpy(), _np(want["32"][1]), what + ("pre",))


def _pre_away_from_the_kink(shape, g):
    """A pre-activation INPUT no element of which sits near zero (fp32 and fp64 cannot disagree on a PReLU branch), both branches."""
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    pre = sign * (0.1 + torch.rand(shape, generator=g))
    share = float((pre > 0).float().mean())
    assert 0.3 <= share <= 0.7, share
    return pre


def _input_grad_operands(cin, cout, k, shape, seed):
    B, H, W = shape
    w, _, x, d_out = _inputs(cin, cout, k, shape, seed)
    g = torch.Generator().manual_seed(seed + 5)
    pre = _pre_away_from_the_kink((B, cin, H, W), g)
    skip = torch.randn(B, cin, H, W, generator=g)
    x_prev = torch.randn(B, 1, H, W, generator=g)          # the input of the weight-gradient call that adds the slope partials up
    return w, x, d_out, pre, skip, x_prev


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("pair", EPI_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_input_grad_epilogues_vs_fp64(pair, k):
    """g = alpha * conv_transposed(d_out); d_slope = sum over pre <= 0 of g pre; d_in = where(pre > 0, g, a g) + skip."""
    from dagl_amd import ops
    cin, cout = pair
    for shape in EPI_SHAPES:
        w, x, d_out, pre, skip, x_prev = _input_grad_operands(cin, cout, k, shape, _seed(pair, k, shape) + 2)
        slope = torch.tensor([0.2])
        g0 = {}
        for tag, dt in DTYPES:
            xi = x.to(dt).requires_grad_(True)
            g0[tag], = torch.autograd.grad(F.conv2d(xi, w.to(dt), None, padding=k // 2), xi, d_out.to(dt))
        wd, dd, pd, kd, xpd, sd = (t.to(DEV) for t in (w, d_out, pre, skip, x_prev, slope))
        packed_t = ops.trunk_pack_weights(wd, True)
        for alpha in (1.0, 0.1):
            for act in (False, True):
                for sk in (False, True):
                    want = {}
                    for tag, dt in DTYPES:
                        gg, p = alpha * g0[tag], pre.to(dt)
                        d_s = torch.where(p > 0, torch.zeros_like(gg), gg * p).sum() if act else None
                        if act:
                            gg = torch.where(p > 0, gg, slope.to(dt) * gg)
                        want[tag] = (gg + skip.to(dt) if sk else gg, d_s)
                    d_in, part = ops.trunk_conv_input_grad(dd, packed_t, cin, k, alpha=alpha, slope=sd if act else None,
                                                           pre=pd if act else None, skip=kd if sk else None)
                    what = (pair, k, shape, alpha, "slope" if act else "no slope", "skip" if sk else "no skip")
                    _bound(_np(d_in), want["64"][0].numpy(), _np(want["32"][0]), what + ("d_in",))
                    assert (part is not None) == act, what
                    if act:
                        _, _, d_s = ops.trunk_conv_weight_grad(xpd, d_in, k, slope_part=part)
                        _bound(_np(d_s), want["64"][1].reshape(1).numpy(), _np(want["32"][1].reshape(1)), what + ("d_slope",))


def _off16(t):
    """The same values in a contiguous view that starts 4 bytes into a larger buffer: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("pair", EPI_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_unaligned_operands_give_the_same_bits(pair, k):
    """W % 4 == 0 with an operand off the 16-byte grid: the element-wise path, the same bits as the 16-byte path."""
    from dagl_amd import ops
    cin, cout = pair
    shape = (2, 8, 64)
    w, b, x, res = _inputs(cin, cout, k, shape, _seed(pair, k, shape) + 3)
    wd, bd, xd, resd = (t.to(DEV) for t in (w, b, x, res))
    sd = torch.tensor([0.2], device=DEV)
    packed = ops.trunk_pack_weights(wd)
    for rs in (1.0, 0.1):
        out, pre = ops.trunk_conv_forward(xd, packed, bd, cout, k, slope=sd, want_pre=True, res_scale=rs, residual=resd)
        out_u, pre_u = ops.trunk_conv_forward(xd, packed, bd, cout, k, slope=sd, want_pre=True, res_scale=rs, residual=_off16(resd))
        assert torch.equal(out, out_u) and torch.equal(pre, pre_u), (pair, k, rs)
    w, x, d_out, pre, skip, x_prev = _input_grad_operands(cin, cout, k, shape, _seed(pair, k, shape) + 4)
    wd, dd, pd, kd, xpd = (t.to(DEV) for t in (w, d_out, pre, skip, x_prev))
    packed_t = ops.trunk_pack_weights(wd, True)
    for alpha in (1.0, 0.1):
        d_in, part = ops.trunk_conv_input_grad(dd, packed_t, cin, k, alpha=alpha, slope=sd, pre=pd, skip=kd)
        for pre_v, skip_v in ((_off16(pd), kd), (pd, _off16(kd)), (_off16(pd), _off16(kd))):
            d_in_u, part_u = ops.trunk_conv_input_grad(dd, packed_t, cin, k, alpha=alpha, slope=sd, pre=pre_v, skip=skip_v)
            assert torch.equal(d_in, d_in_u) and torch.equal(part, part_u), (pair, k, alpha)
        d_s = ops.trunk_conv_weight_grad(xpd, d_in, k, slope_part=part)[2]
        assert torch.equal(d_s, ops.trunk_conv_weight_grad(xpd, d_in_u, k, slope_part=part_u)[2]), (pair, k, alpha)


# ---- guard bands: the raw C ABI (the way ops.py calls it), every output inside a larger buffer of sentinels --------------------
SENTINEL32 = 0x7FA5A5A5                      # as a float: a NaN no kernel computes
SENTINEL64 = 0x7FF5A5A5A5A5A5A5
GUARD_BYTES = 256


class _Guarded:
    """``n`` elements of ``dtype`` (fp32 / fp64) between two bands of >= 256 sentinel bytes; ``skew``: start 4 bytes later."""

    def __init__(self, n, dtype=torch.float32, skew=False):
        wide = dtype == torch.float64
        self.sentinel = SENTINEL64 if wide else SENTINEL32
        self.pad = GUARD_BYTES // (8 if wide else 4) + (1 if skew else 0)
        self.n = n
        self.raw = torch.full((self.pad + n + GUARD_BYTES // 4,), self.sentinel, device=DEV, dtype=torch.int64 if wide else torch.int32)
        self.t = self.raw[self.pad:self.pad + n].view(dtype)
        assert self.t.data_ptr() % 16 == (4 if skew else 0)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, written=True):
        assert bool((self.raw[:self.pad] == self.sentinel).all()), (what, "written before the buffer")
        assert bool((self.raw[self.pad + self.n:] == self.sentinel).all()), (what, "written behind the buffer")
        if written:
            assert not bool((self.raw[self.pad:self.pad + self.n] == self.sentinel).any()), (what, "elements left unwritten")


def _guard_case(pair, k, shape, skew_out=False):
    from dagl_amd import _lib
    from dagl_amd._lib import check
    lib = _lib.load()
    cin, cout = pair
    B, H, W = shape
    w, b, x, up = _inputs(cin, cout, k, shape, _seed(pair, k, shape) + 6)
    g = torch.Generator().manual_seed(11)
    res = torch.randn(B, cout, H, W, generator=g)
    skip = torch.randn(B, cin, H, W, generator=g)
    pre_in = torch.where(torch.rand(B, cin, H, W, generator=g) < 0.5, -1.0, 1.0) * (0.1 + torch.rand(B, cin, H, W, generator=g))
    wd, bd, xd, upd, resd, skipd, pred = (t.to(DEV).contiguous() for t in (w, b, x, up, res, skip, pre_in))
    sd = torch.tensor([0.2], device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    tag = (pair, k, shape, "skewed out" if skew_out else "aligned")

    packed = _Guarded(lib.dagl_trunk_packed_floats(cin, cout, k, 0))
    packed_t = _Guarded(lib.dagl_trunk_packed_floats(cin, cout, k, 1))
    check(lib.dagl_trunk_pack_weights(st, cin, cout, k, 0, wd.data_ptr(), packed.ptr()), "pack")
    check(lib.dagl_trunk_pack_weights(st, cin, cout, k, 1, wd.data_ptr(), packed_t.ptr()), "pack transposed")
    packed.check(tag + ("packed",))
    packed_t.check(tag + ("packed_t",))

    out = _Guarded(B * cout * H * W, skew=skew_out)
    pre_out = _Guarded(B * cout * H * W)
    check(lib.dagl_trunk_conv_forward(st, B, cin, cout, H, W, k, xd.data_ptr(), packed.ptr(), bd.data_ptr(), sd.data_ptr(),
                                      pre_out.ptr(), 0.1, resd.data_ptr(), out.ptr()), "forward")
    out.check(tag + ("out",))
    pre_out.check(tag + ("pre_out",))
    if skew_out:
        return

    n_blocks = lib.dagl_trunk_input_grad_blocks(B, H, W)
    d_in = _Guarded(B * cin * H * W)
    part = _Guarded(n_blocks, torch.float64)
    check(lib.dagl_trunk_conv_input_grad(st, B, cin, cout, H, W, k, upd.data_ptr(), packed_t.ptr(), 0.1, sd.data_ptr(), pred.data_ptr(),
                                         part.ptr(), skipd.data_ptr(), d_in.ptr()), "input grad")
    d_in.check(tag + ("d_in",))
    part.check(tag + ("slope_part",))

    need = lib.dagl_trunk_weight_grad_scratch_bytes(B, cin, cout, H, W, k)
    assert need > 0 and need % 16 == 0
    d_w, d_b, d_s, scratch = _Guarded(cout * cin * k * k), _Guarded(cout), _Guarded(1), _Guarded(need // 4)
    check(lib.dagl_trunk_conv_weight_grad(st, B, cin, cout, H, W, k, xd.data_ptr(), upd.data_ptr(), 1.0, d_w.ptr(), d_b.ptr(),
                                          part.ptr(), n_blocks, d_s.ptr(), scratch.ptr(), need), "weight grad")
    d_w.check(tag + ("d_w",))
    d_b.check(tag + ("d_b",))
    d_s.check(tag + ("d_slope",))
    scratch.check(tag + ("scratch",))
    out.check(tag + ("out, after the backward",))
    # the guarded buffers took part as operands: the numbers are still the stock layer's
    ref = _stock(w, b, x, up, k)
    for name, a, i in (("d_w", d_w, 2), ("d_b", d_b, 3)):
        _bound(_np(a.t).reshape(ref["64"][i].shape), ref["64"][i].numpy(), _np(ref["32"][i]), tag + (name,))


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("pair", [(5, 7), (20, 33)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_no_write_outside_the_outputs(pair, k):
    for shape in ((2, 7, 64), (1, 4, 129), (1, 3, 15)):          # W % 4 = 0, 1, 3; two column tiles at 129
        _guard_case(pair, k, shape)
    _guard_case(pair, k, (2, 7, 64), skew_out=True)


@pytest.mark.parametrize("pair", DET_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_weight_grad_is_deterministic(pair):
    from dagl_amd import ops
    cin, cout = pair
    shape = (1, 70, 131)
    w, x, d_out, pre, _, _ = _input_grad_operands(cin, cout, 3, shape, _seed(pair, 3, shape) + 8)
    wd, xd, dd, pd = (t.to(DEV) for t in (w, x, d_out, pre))
    sd = torch.tensor([0.2], device=DEV)
    _, part = ops.trunk_conv_input_grad(dd, ops.trunk_pack_weights(wd, True), cin, 3, slope=sd, pre=pd)
    first = ops.trunk_conv_weight_grad(xd, dd, 3, slope_part=part)
    torch.empty(1 << 22, device=DEV).fill_(float("nan"))          # whatever the next scratch reuses holds other bits now
    second = ops.trunk_conv_weight_grad(xd, dd, 3, slope_part=part)
    for name, a, b in zip(("d_w", "d_b", "d_slope"), first, second):
        assert torch.equal(a, b), (pair, name)


@pytest.mark.parametrize("where", ["interior", "first", "last"])
@pytest.mark.parametrize("W", [66, 64])
def test_one_inf_reaches_what_it_reaches_in_the_stock_layer(W, where):
    """One +inf in x: the non-finite elements of out, d_w and d_b are the stock CPU fp32 layer's, every other element still meets the
    bound -- no padding zero (channels, columns, k-steps) is ever multiplied by a staged inf."""
    from dagl_amd import ops
    pair, k, shape = (12, 20), 3, (1, 9, W)
    cin, cout = pair
    H = shape[1]
    w, b, x, up = _inputs(cin, cout, k, shape, _seed(pair, k, shape) + 9)
    y, xx = {"interior": (4, W // 2), "first": (0, 0), "last": (H - 1, W - 1)}[where]
    x[0, 5, y, xx] = float("inf")
    ref = _stock(w, b, x, up, k)
    wd, bd, xd, upd = (t.to(DEV) for t in (w, b, x, up))
    out, _ = ops.trunk_conv_forward(xd, ops.trunk_pack_weights(wd), bd, cout, k)
    d_w, d_b, _ = ops.trunk_conv_weight_grad(xd, upd, k)
    for name, a, i in (("out", out, 0), ("d_w", d_w, 2), ("d_b", d_b, 3)):
        a, r64, r32 = a.cpu(), ref["64"][i], ref["32"][i]
        bad, bad32 = ~torch.isfinite(a), ~torch.isfinite(r32)
        assert torch.equal(bad, bad32), (W, where, name, "non-finite at", bad.nonzero().tolist()[:8], "stock", bad32.nonzero().tolist()[:8])
        assert torch.equal(bad32, ~torch.isfinite(r64)), (W, where, name)
        ok = ~bad
        _bound(_np(a[ok]), r64[ok].numpy(), _np(r32[ok]), (W, where, name))
    assert not torch.isfinite(out).all() and not torch.isfinite(d_w).all() and torch.isfinite(d_b).all()
