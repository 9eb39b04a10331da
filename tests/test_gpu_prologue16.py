"""The prologue convolutions (csrc/prologue.hip) element by element against fp64: conv_pair16_kernel (split fp16, through
``dagl_ce_prologue16`` and the read-out entry ``dagl_ce_prologue16_debug``), conv_pair_kernel (fp32, ``dagl_ce_prologue``) and the two
thr / bias kernels, at the smallest shapes of every class of the launch plan (tests/test_prologue16_plan_host.py pins each shape's plan
and names its class), over strip boundaries, odd and single rows per block, per-block input scales and the subnormal floor of the halves.

Reference: fp64 ``conv2d`` on the CPU (thr / bias over the SAME padding of make_grid).  With every output its error unit
    u = sum_window |w| |x| + |bias|                                         (fp64)
and every value check is per element against u -- a wrong halo column or last row touches few elements, no norm would see it.

Error model of the split kernel, per element:
    |got - ref| <= K 2^-22 u + 2^-25 (sum_window |w| / xs_block + sum_window |x| / 256)
  * xs_block: the input scale of the block that owns the pixel, by the kernel's rule: 16 while 16 max|x| < 60000 over the block's staged
    region (rows y0-1 .. y1, columns x0-1 .. x0+64), else 2^e, the largest power of two with 2^e max|x| < 32768, e in [-120, 4].
  * the second term is the subnormal floor of the fp16 halves (derived, not measured): a half below 2^-14 is a multiple of 2^-24, so
    16 x = hi + lo and 256 w = hi + lo each lose up to 2^-25 in absolute terms once |16 x| < 2^-14 2^11 (|x| <~ 8e-3) resp. |w| <~ 5e-4.
  * K = 3 + 2 r32: 3 for the split (rounding of x, of w, the dropped lo lo term), r32 = the largest per-element error of torch's fp32 CPU
    conv2d over the same cases in units of 2^-22 u (a reference, not the code under test), twice for another summation order.
The fp32 kernels: (2 r32 + 1) 2^-22 u, with r32 of the g / theta pair for conv_pair_kernel and of the 7x7 heads for the thr / bias kernels.
``test_floor_is_small_at_scale_one`` shows on the CPU that at O(1) inputs the floor is under 10 % of the bound at every element: it
cannot hide a failure there.

Measured: r32 = 1.27 (g / theta), 0.36 (7x7 heads) on the CPU, so K = 5.54 and the fp32 bounds are 3.54 / 1.71 units of 2^-22 u.  Worst
|got - ref| / (2^-22 u) of one run on the MI355X, split b1 / b2 . fp32 b1 / b2 . thr / bias (every line printed as "[prologue16] ..."):
  1,1,1    0.16 0.11 . 0.18 0.14 . 0.03 0.04      1,2,3    0.13 0.24 . 0.33 0.39 . 0.05 0.01      1,3,5   0.11 0.23 . 0.27 0.54 . 0.04 0.05
  2,5,63   0.16 0.40 . 0.61 0.85 . 0.07 0.09      1,4,64   0.19 0.42 . 0.36 0.80 . 0.04 0.03      1,6,65  0.18 0.36 . 0.57 0.86 . 0.06 0.08
  1,9,130  0.16 0.38 . 0.54 0.91 . 0.08 0.09      1,8,132  0.17 0.40 . 0.49 1.04 . 0.06 0.07      43,7,65 0.24 0.51 . 0.63 1.29 . 0.10 0.11
  64,8,70  0.22 0.56 . 0.63 1.51 . 0.11 0.09      256,5,8  0.24 0.56 . 0.63 1.01 . 0.11 0.11      1,8,64 (also unaligned) 0.19 0.40 . 0.35 1.01 . 0.05 0.05
  [2,12,130]: one 1e4 / 1e6 -- 0.77-1.85 / 1.32-1.89 inside the rescaled blocks; x 3e3 0.22 0.41; x 1e-4 14.9 42.4 and x 1e-6 1376 4294
  (0.35 / 0.39 of the bound: the floor term holds them); the 3e9 case 0.22 of K's term.  DESIGN.md section 5 has the table with classes.

Exact checks (same debug call's fp32 map, numpy float16 = round to nearest even, overflow to inf): hi == fp16(16 b1), lo == fp16(16 b1 -
hi), the coarse pair at 2^-8; slot (head, image, chunk, strip, wave) == max |b1| of that wave's rows and 16 columns, 0.0 without a column
inside the map, +inf for a non-finite value; the n clear words 0; the range word untouched while everything is in range."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_prologue16_plan_host import CASES, MULTI_HEAD, rule

gpu = pytest.mark.gpu

U22, U25 = 2.0 ** -22, 2.0 ** -25
TABLE = [s for s in sorted(CASES) if s not in ((1, 7, 65), (2, 12, 130))]        # the shapes every entry runs; the two others: below
ENTRIES = ("prologue16", "debug", "fp32")
SCALE_SHAPE = (2, 12, 130)
RANGE_INIT, TAG = 0x5A5A, 77


# ---- inputs and the fp64 reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """One head's parameters: randn x 0.1 (shared by every case: an image computed alone and inside a batch has the same weights)."""
    g = torch.Generator().manual_seed(900 + seed)
    r = lambda *s: torch.randn(*s, generator=g) * 0.1
    return dict(g_w=r(16, 64, 3, 3), g_b=r(16), th_w=r(16, 64, 1, 1), th_b=r(16), thr_w=r(1, 64, 7, 7), thr_b=r(1), bias_w=r(1, 64, 7, 7),
                bias_b=r(1))


@functools.lru_cache(maxsize=None)
def image_bank():
    """The images of [43,7,65]: the case itself, the image computed alone and the four-head call take theirs from here."""
    return torch.randn(43, 64, 7, 65, generator=torch.Generator().manual_seed(4307))


@functools.lru_cache(maxsize=None)
def case_input(shape):
    B, H, W = shape
    if shape == (43, 7, 65):
        return image_bank()
    return torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(B * 10007 + H * 131 + W))


def same_pad(H, W):
    """(left, right, top, bottom) of the stride-4 7x7 query grid (make_grid, csrc/dagl_common.h)."""
    Lh, Lw = -(-H // 4), -(-W // 4)
    ph, pw = max((Lh - 1) * 4 + 7 - H, 0), max((Lw - 1) * 4 + 7 - W, 0)
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def reference(x, w, zero_bias=False):
    """fp64 results and error units of the four convolutions: {name: (ref, u, sum_window |w|, sum_window |x|)}; g / theta as [B,16,H,W],
    thr / bias as [B,L]."""
    x64, a = x.double(), x.double().abs()
    B, _, H, W = x.shape
    ones = torch.ones_like(a)
    out = {}
    for name, wk, bk, pad in (("b1", "g_w", "g_b", 1), ("b2", "th_w", "th_b", 0)):
        wt = w[wk].double()
        b = w[bk].double() * (0.0 if zero_bias else 1.0)
        out[name] = (F.conv2d(x64, wt, b, padding=pad), F.conv2d(a, wt.abs(), b.abs(), padding=pad),
                     F.conv2d(ones, wt.abs(), padding=pad), F.conv2d(a, torch.ones(1, 64, *wt.shape[2:], dtype=torch.float64), padding=pad))
    pads = same_pad(H, W)
    xp, ap = F.pad(x64, pads), F.pad(a, pads)
    for name, wk, bk in (("thr", "thr_w", "thr_b"), ("bias", "bias_w", "bias_b")):
        wt, b = w[wk].double(), w[bk].double()
        out[name] = (F.conv2d(xp, wt, b, stride=4).reshape(B, -1), F.conv2d(ap, wt.abs(), b.abs(), stride=4).reshape(B, -1), None, None)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(shape):
    return reference(case_input(shape), weights())


def fp32_reference_error(x, w):
    """Largest per-element error of torch's fp32 CPU conv2d in units of 2^-22 u: (g / theta pair, thr / bias heads)."""
    ref = reference(x, w)
    B, _, H, W = x.shape
    got = {"b1": F.conv2d(x, w["g_w"], w["g_b"], padding=1), "b2": F.conv2d(x, w["th_w"], w["th_b"])}
    xp = F.pad(x, same_pad(H, W))
    got["thr"] = F.conv2d(xp, w["thr_w"], w["thr_b"], stride=4).reshape(B, -1)
    got["bias"] = F.conv2d(xp, w["bias_w"], w["bias_b"], stride=4).reshape(B, -1)
    r = {k: float(((got[k].double() - ref[k][0]).abs() / (U22 * ref[k][1])).max()) for k in got}
    return max(r["b1"], r["b2"]), max(r["thr"], r["bias"])


@functools.lru_cache(maxsize=None)
def r32():
    """(r32 of the pair, r32 of the heads) over the table's cases."""
    rs = [fp32_reference_error(case_input(s), weights()) for s in TABLE]
    return max(r[0] for r in rs), max(r[1] for r in rs)


def K():
    return 3.0 + 2.0 * r32()[0]


# ---- the kernel's per-block input scale, from the plan -------------------------------------------------------------------------------
def block_scales(x, plan):
    """-> (xs [B,H,W] float64: the scale of the block that owns the pixel, {(image, chunk, strip)} of the blocks that rescale)."""
    strips, chunks, rows, _ = plan
    B, _, H, W = x.shape
    amap = x.abs().amax(dim=1).double().numpy()
    xs = np.full((B, H, W), 16.0)
    rescaled = set()
    for b in range(B):
        for ch in range(chunks):
            y0, y1 = ch * rows, min(ch * rows + rows, H)
            for st in range(strips):
                x0 = 64 * st
                m = amap[b, max(y0 - 1, 0):min(y1, H - 1) + 1, max(x0 - 1, 0):min(x0 + 64, W - 1) + 1].max()
                with np.errstate(over="ignore"):
                    if np.float32(16.0) * np.float32(m) < 60000.0:
                        continue
                e = 15 - int(np.frexp(m)[1]) if np.float32(m) <= np.float32(3.0e38) else 0      # (beyond: as an inf, scale 1)
                xs[b, y0:y1, x0:x0 + 64] = 2.0 ** min(max(e, -120), 4)
                rescaled.add((b, ch, st))
    return xs, rescaled


def bound16(ref, name, xs):
    _, u, sw, sx = ref[name]
    return K() * U22 * u + U25 * (sw / torch.from_numpy(xs)[:, None] + sx / 256.0)


def interior(t):
    """[B,H+6,W+6,16] -> [B,16,H,W]"""
    return t[:, 3:-3, 3:-3, :].permute(0, 3, 1, 2)


def assert_border_zero(t, what):
    frame = torch.ones(t.shape[1:3], dtype=torch.bool)
    frame[3:-3, 3:-3] = False
    assert bool((t[:, frame] == 0).all()), f"{what}: the 3-pixel border is not zero"


def check(got, want, bound, what, sel=None):
    """Every (selected) element within its bound; prints the worst ratio first."""
    err = (got.double() - want).abs()
    ratio = err / bound
    if sel is not None:
        ratio = ratio[sel]
    bad = ~(ratio <= 1.0)                                    # a NaN fails
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
    print(f"[prologue16] {what}: worst |err| / bound {worst:.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond the bound, worst ratio {worst:.3f}"
    return worst


def units(got, want, u):
    """worst |got - ref| in units of 2^-22 u (the figure DESIGN.md section 5 lists)"""
    return float(((got.double() - want).abs() / (U22 * u)).max())


# ---- the three entries ---------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _params(w, dev, zero_bias=False):
    p = {k: v.to(dev).contiguous() for k, v in w.items()}
    if zero_bias:
        p["g_b"].zero_(); p["th_b"].zero_()
    return p


def run_prologue(xd, p, fast):
    """dagl_ce_prologue16 (``fast``) or dagl_ce_prologue on a device input: outputs pre-filled with NaN, scratch with 0xff bytes.
    -> dict of CPU tensors b1, b2 (padded NHWC), thr, bias."""
    from dagl_amd import _lib, ops
    lib = _lib.load()
    dev = xd.device
    B, _, H, W = xd.shape
    L = -(-H // 4) * -(-W // 4)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    b1, b2, thr, bias = nan(B, H + 6, W + 6, 16), nan(B, H + 6, W + 6, 16), nan(B, L), nan(B, L)
    args = [ops._stream(), B, H, W, xd.data_ptr(), p["g_w"].data_ptr(), p["g_b"].data_ptr(), p["th_w"].data_ptr(), p["th_b"].data_ptr(),
            p["thr_w"].data_ptr(), p["thr_b"].data_ptr(), p["bias_w"].data_ptr(), p["bias_b"].data_ptr(), b1.data_ptr(), b2.data_ptr(),
            thr.data_ptr(), bias.data_ptr()]
    if fast:
        need = lib.dagl_ce_prologue16_scratch_bytes(B, H, W)
        buf = torch.full((need + 256,), 0xFF, device=dev, dtype=torch.uint8)
        _lib.check(lib.dagl_ce_prologue16(*args, buf.data_ptr() + (-buf.data_ptr()) % 256, need), "dagl_ce_prologue16")
    else:
        buf = torch.full((8 * B * L * 4,), 0xFF, device=dev, dtype=torch.uint8)
        _lib.check(lib.dagl_ce_prologue(*args, buf.data_ptr()), "dagl_ce_prologue")
    torch.cuda.synchronize()
    return dict(b1=b1.cpu(), b2=b2.cpu(), thr=thr.cpu(), bias=bias.cpu())


def run_debug(xds, ps, **kw):
    from dagl_amd import ops
    out = ops.ce_prologue16_debug(xds, [p["g_w"] for p in ps], [p["g_b"] for p in ps], [p["th_w"] for p in ps], [p["th_b"] for p in ps],
                                  tag=TAG, range_init=RANGE_INIT, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def f16_pair(v32, scale):
    """numpy emulation of c16_split(v * scale): (hi bits, lo bits) as uint16"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = v32 * np.float32(scale)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def check_planes_and_slots(out, heads, imgs, H, W, coarse=True):
    """The exact checks on one debug call: planes, slots, clear words (the range word is the caller's)."""
    b1 = out["b1"][:, 3:-3, 3:-3, :].contiguous().numpy()
    pairs = [("hi", "lo", 16.0)] + ([("hi2", "lo2", 1.0 / 256.0)] if coarse else [])
    for hn, ln, scale in pairs:
        hi, lo = f16_pair(b1, scale)
        for name, want in ((hn, hi), (ln, lo)):
            got = out[name][:, 3:-3, 3:-3, :].contiguous().numpy().view(np.uint16)
            got, want = got[np.isfinite(b1)], want[np.isfinite(b1)]          # (a NaN's payload is nobody's contract)
            assert np.array_equal(got, want), f"plane {name}: {int((got != want).sum())} halves differ from fp16({scale} b1)"
            assert_border_zero(out[name], name)
    strips, chunks, rows, slots = rule(heads, imgs, H, W)
    a = np.abs(b1).max(axis=3)                                        # [B,H,W]
    a = np.where(np.isfinite(a), a, np.float32(np.inf))
    want = np.zeros((heads, imgs, chunks, strips, 4), dtype=np.float32)
    for ch in range(chunks):
        for st in range(strips):
            for wv in range(4):
                c0 = 64 * st + 16 * wv
                if c0 < W:
                    blk = a[:, ch * rows:min(ch * rows + rows, H), c0:min(c0 + 16, W)]
                    want[:, :, ch, st, wv] = blk.reshape(heads, imgs, -1).max(axis=2)
    got = out["amax"].numpy().reshape(heads, imgs, chunks, strips, 4)
    assert out["amax"].shape == (heads, slots)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} slots differ"
    assert bool((out["clear"] == 0).all()) and out["clear"].numel() == 8


# ---- CPU: the model's own consistency ------------------------------------------------------------------------------------------------
def test_floor_is_small_at_scale_one():
    """At O(1) inputs the floor term is under a tenth of the bound at every element of every table case (reference alone)."""
    print(f"[prologue16] r32 pair {r32()[0]:.3f}  heads {r32()[1]:.3f}  K {K():.3f}")
    assert 0.05 < r32()[0] < 8.0 and 0.05 < r32()[1] < 8.0               # a sane fp32 reference: a few units of 2^-22 u at most
    for shape in TABLE:
        ref = case_reference(shape)
        xs, rescaled = block_scales(case_input(shape), CASES[shape][0])
        assert not rescaled
        for name in ("b1", "b2"):
            _, u, sw, sx = ref[name]
            floor = U25 * (sw / 16.0 + sx / 256.0)
            assert float((floor / bound16(ref, name, xs)).max()) < 0.1, (shape, name)


def test_block_scales_follow_the_rule():
    x = torch.zeros(1, 64, 12, 130)
    x[0, 3, 5, 63] = 1.0e6
    xs, rescaled = block_scales(x, rule(1, 1, 12, 130))
    assert rescaled == {(0, 2, 0), (0, 3, 0), (0, 2, 1), (0, 3, 1)} and set(np.unique(xs)) == {16.0, 2.0 ** -5}
    x[0, 3, 5, 63] = 3749.0
    assert not block_scales(x, rule(1, 1, 12, 130))[1]
    x[0, 3, 5, 63] = 3750.0                                              # 16 x = 60000: not < 60000; 2^3 x 3750 < 32768
    assert set(np.unique(block_scales(x, rule(1, 1, 12, 130))[0])) == {16.0, 8.0}
    # the clamps of e are out of a finite input's reach: a block runs again from max|x| >= 3750 on (e <= 3), 3e38 -- the largest
    # value the kernel scales; beyond it counts as an inf -- gives e = -113
    x[0, 3, 5, 63] = 3.0e38
    assert set(np.unique(block_scales(x, rule(1, 1, 12, 130))[0])) == {16.0, 2.0 ** -113}
    x[0, 3, 5, 63] = float(np.finfo(np.float32).max)
    assert set(np.unique(block_scales(x, rule(1, 1, 12, 130))[0])) == {16.0, 1.0}


# ---- GPU: the table ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_input(shape, unaligned=False):
    x = case_input(shape)
    if not unaligned:
        return x.to(_dev())
    store = torch.empty(x.numel() + 1, device=_dev())
    view = store[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _run_entry(entry, xd, p):
    if entry == "debug":
        return run_debug([xd], [p])
    return run_prologue(xd, p, fast=entry == "prologue16")


def _check_case(shape, entry, unaligned=False):
    B, H, W = shape
    ref = case_reference(shape)
    xd, p = device_input(shape, unaligned), _params(weights(), _dev())
    out = _run_entry(entry, xd, p)
    xs = np.full((B, H, W), 16.0)
    figures = {}
    for name in ("b1", "b2"):
        got = interior(out[name])
        bound = bound16(ref, name, xs) if entry != "fp32" else (2.0 * r32()[0] + 1.0) * U22 * ref[name][1]
        check(got, ref[name][0], bound, f"{shape} {entry} {name}")
        figures[name] = units(got, ref[name][0], ref[name][1])
        assert_border_zero(out[name], f"{shape} {entry} {name}")
    if entry != "debug":
        for name in ("thr", "bias"):
            check(out[name], ref[name][0], (2.0 * r32()[1] + 1.0) * U22 * ref[name][1], f"{shape} {entry} {name}")
            figures[name] = units(out[name], ref[name][0], ref[name][1])
    else:
        check_planes_and_slots(out, 1, B, H, W)
        assert int(out["range"][0]) == RANGE_INIT                       # tiers on, everything in range: untouched
    print(f"[prologue16] {shape} {entry} units of 2^-22 u: " + "  ".join(f"{k} {v:.3f}" for k, v in figures.items()))
    again = _run_entry(entry, xd, p)
    for k, v in out.items():
        if v is not None and v.dtype == torch.float32:
            assert same_bits(v, again[k]), f"{shape} {entry} {k}: a second call gives other bits"
        elif v is not None:
            assert torch.equal(v, again[k]), f"{shape} {entry} {k}: a second call gives other bits"
    return out


@gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", TABLE, ids=lambda s: "x".join(map(str, s)))
def test_values_per_element(shape, entry):
    _check_case(shape, entry)


@gpu
def test_unaligned_input_at_w_multiple_of_four():
    """[1,8,64] with x one float into its storage: the float4 thr / bias kernel cannot take it; the generic kernel's result agrees with
    the aligned call's to the bit (both add the taps in the same order), and all three entries keep their bounds."""
    shape = (1, 8, 64)
    for entry in ENTRIES:
        un = _check_case(shape, entry, unaligned=True)
        al = _run_entry(entry, device_input(shape), _params(weights(), _dev()))
        for k in ("b1", "b2") + (("thr", "bias") if entry != "debug" else ()):
            assert same_bits(un[k], al[k]), (entry, k)


@gpu
def test_an_image_alone_inside_a_batch_and_inside_four_heads():
    """Per-pixel arithmetic does not depend on the plan (no block rescales here): image 17 of [43,7,65] (three rows per block) has the
    same bits computed alone (two rows per block) and as image 1 of head 2 of a four-head call, whose other heads have other weights and
    inputs -- the batch index b = head * imgs + image -- and every head keeps the bound."""
    H, W = 7, 65
    bank, p0 = image_bank(), _params(weights(), _dev())
    batch = run_prologue(bank.to(_dev()), p0, fast=True)
    alone = run_prologue(bank[17:18].to(_dev()), p0, fast=True)
    for k in ("b1", "b2", "thr", "bias"):
        assert same_bits(batch[k][17:18], alone[k]), k
    heads, imgs = MULTI_HEAD[0][:2]
    assert rule(heads, imgs, H, W) == MULTI_HEAD[1]
    ws = [weights(1), weights(2), weights(0), weights(3)]
    xs_cpu = [bank[0:2], bank[5:7], bank[16:18], bank[30:32]]
    out = run_debug([x.to(_dev()) for x in xs_cpu], [_params(w, _dev()) for w in ws])
    for k in ("b1", "b2"):
        assert same_bits(out[k][2 * imgs + 1], alone[k][0]), k
        assert_border_zero(out[k], k)
    for h in range(heads):
        ref = reference(xs_cpu[h], ws[h])
        for name in ("b1", "b2"):
            check(interior(out[name][h * imgs:(h + 1) * imgs]), ref[name][0], bound16(ref, name, np.full((imgs, H, W), 16.0)),
                  f"four heads, head {h} {name}")
    check_planes_and_slots(out, heads, imgs, H, W)
    assert int(out["range"][0]) == RANGE_INIT
    # the fine pair alone, no fp32 map, no words to clear: the same halves
    lean = run_debug([x.to(_dev()) for x in xs_cpu], [_params(w, _dev()) for w in ws], want_b1=False, coarse=False, n_clear=0)
    assert torch.equal(lean["hi"], out["hi"]) and torch.equal(lean["lo"], out["lo"]) and same_bits(lean["b2"], out["b2"])
    assert same_bits(lean["amax"], out["amax"])


# ---- GPU: scales ---------------------------------------------------------------------------------------------------------------------
PLACEMENTS = {          # (row, column) of the hot value in image 0 of [2,12,130] (6 chunks of 2 rows, 3 strips) -> (chunk, strip) that rescale
    "inside a strip": ((4, 20), {(1, 0), (2, 0)}),                       # row 4: chunk 2's own, chunk 1's row y1
    "column 64": ((4, 64), {(1, 0), (2, 0), (1, 1), (2, 1)}),           # strip 1's own pixel, strip 0's right halo
    "column 63": ((5, 63), {(2, 0), (3, 0), (2, 1), (3, 1)}),           # strip 0's own pixel, strip 1's left halo
    "row above a chunk": ((5, 100), {(2, 1), (3, 1)}),                  # chunk 3's row y0 - 1
}
HOT_CHANNEL = 5


@functools.lru_cache(maxsize=None)
def scale_base():
    """The hot-free run of the scale shape."""
    return run_prologue(case_input(SCALE_SHAPE).to(_dev()), _params(weights(), _dev()), fast=True)


def block_mask(shape, plan, blocks):
    """[B,H,W] bool: pixels owned by the given (image, chunk, strip) blocks"""
    B, H, W = shape
    m = torch.zeros(B, H, W, dtype=torch.bool)
    for b, ch, st in blocks:
        m[b, ch * plan[2]:ch * plan[2] + plan[2], 64 * st:64 * st + 64] = True
    return m


@gpu
@pytest.mark.parametrize("hot", (1.0e4, 1.0e6), ids=("1e4", "1e6"))
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_one_hot_value(place, hot):
    """One value of 1e4 (xs = 2) or 1e6 (xs = 2^-5: the floor term is what bounds the block's other pixels) in image 0: the blocks that
    stage it -- as their own pixel, their halo column or their halo row -- rescale, named here from the plan; the bound holds in them and
    around them; every other block and all of image 1 keep the bits of the hot-free run."""
    plan = CASES[SCALE_SHAPE][0]
    (y, xcol), want_blocks = PLACEMENTS[place]
    x = case_input(SCALE_SHAPE).clone()
    x[0, HOT_CHANNEL, y, xcol] = hot
    xs, rescaled = block_scales(x, plan)
    assert rescaled == {(0, ch, st) for ch, st in want_blocks}
    assert set(np.unique(xs)) == {16.0, 2.0 if hot == 1.0e4 else 2.0 ** -5}
    ref = reference(x, weights())
    out = run_prologue(x.to(_dev()), _params(weights(), _dev()), fast=True)
    base = scale_base()
    inside = block_mask(SCALE_SHAPE, plan, rescaled)
    for name in ("b1", "b2"):
        got = interior(out[name])
        check(got, ref[name][0], bound16(ref, name, xs), f"hot {hot:g} {place} {name}")
        sel = inside[:, None].expand_as(got)
        print(f"[prologue16] hot {hot:g} {place} {name}: rescaled blocks, units of 2^-22 u {units(got[sel], ref[name][0][sel], ref[name][1][sel]):.3f}")
        assert same_bits(got[~sel], interior(base[name])[~sel]), f"{name}: a block that does not rescale changed its bits"
        assert same_bits(out[name][1], base[name][1])
        assert_border_zero(out[name], name)
    for name in ("thr", "bias"):                                     # (the 7x7 heads have no scale of their own: image 1 is untouched)
        assert same_bits(out[name][1], base[name][1])


@gpu
def test_the_second_attempt_takes_the_scale_of_the_rule():
    """The bound cannot tell 2^e from 2^(e-1): a power of two moves nothing but the floor, by a factor the model's slack swallows.  Where
    the floor is ALL there is, the scale shows: a hot value of 3e9 gives its blocks xs = 2^-17 by the rule, every other input value then
    splits below 2^-14 -- hi is the value rounded to the subnormal grid 2^-24 (ties to even), lo rounds to zero -- so those blocks compute
    the convolution of x rounded to multiples of 2^-7, exactly that input.  Against the fp64 result on that rounded input the usual bound
    holds WITHOUT the input's floor term; one power of two off in either direction and the grid is another one (errors of ~1e-2 against
    a bound of ~5e-5)."""
    plan = CASES[SCALE_SHAPE][0]
    (y, xcol), want_blocks = PLACEMENTS["column 63"]
    x = case_input(SCALE_SHAPE).clone()
    x[0, HOT_CHANNEL, y, xcol] = 3.0e9
    xs, rescaled = block_scales(x, plan)
    assert rescaled == {(0, ch, st) for ch, st in want_blocks} and set(np.unique(xs)) == {16.0, 2.0 ** -17}
    assert float(case_input(SCALE_SHAPE).abs().max()) * 2.0 ** -17 < 2.0 ** -14
    xq = torch.round(x * 2.0 ** 7) / 2.0 ** 7                           # (torch.round: ties to even; the hot value is a multiple already)
    assert float(xq[0, HOT_CHANNEL, y, xcol]) == 3.0e9
    ref = reference(xq, weights())
    out = run_prologue(x.to(_dev()), _params(weights(), _dev()), fast=True)
    inside = block_mask(SCALE_SHAPE, plan, rescaled)
    for name in ("b1", "b2"):
        got = interior(out[name])
        _, u, _, sx = ref[name]
        check(got, ref[name][0], K() * U22 * u + U25 * sx / 256.0, f"hot 3e9 {name} against the input on the 2^-7 grid",
              sel=inside[:, None].expand_as(got))


@gpu
@pytest.mark.parametrize("factor", (1.0e-4, 1.0e-6, 3.0e3), ids=("1e-4", "1e-6", "3e3"))
def test_whole_input_scaled(factor):
    """x 1e-4 and x 1e-6 (zero conv biases, so that u scales with the input): every lo half, then every hi half, is an fp16 subnormal --
    K's term alone (a few 2^-22 u) is far below the halves' quantisation error here, the floor term is what is being tested.  x 3e3:
    every block rescales, each with the scale of its own maximum."""
    plan = CASES[SCALE_SHAPE][0]
    small = factor < 1.0
    x = case_input(SCALE_SHAPE) * factor
    xs, rescaled = block_scales(x, plan)
    assert len(rescaled) == (0 if small else 2 * plan[0] * plan[1])
    ref = reference(x, weights(), zero_bias=small)
    out = run_prologue(x.to(_dev()), _params(weights(), _dev(), zero_bias=small), fast=True)
    for name in ("b1", "b2"):
        got = interior(out[name])
        bound = bound16(ref, name, xs)
        if small:                                                    # the floor dominates the bound at every element
            assert float((K() * U22 * ref[name][1] / bound).max()) < 0.5
        check(got, ref[name][0], bound, f"x {factor:g} {name}")
        print(f"[prologue16] x {factor:g} {name}: units of 2^-22 u {units(got, ref[name][0], ref[name][1]):.3f}")
        assert_border_zero(out[name], name)


@gpu
def test_one_inf_through_the_debug_entry():
    """An inf in image 0: the waves whose pixels it reaches report +inf in their slots, the range word holds the call's tag; image 1 and
    every block of image 0 that does not stage the inf stay finite and within the bound."""
    plan = CASES[SCALE_SHAPE][0]
    B, H, W = SCALE_SHAPE
    clean = case_input(SCALE_SHAPE)
    x = clean.clone()
    x[0, HOT_CHANNEL, 4, 20] = float("inf")
    xs, rescaled = block_scales(x, plan)
    assert rescaled == {(0, 1, 0), (0, 2, 0)}
    ref = case_reference(SCALE_SHAPE)
    out = run_debug([x.to(_dev())], [_params(weights(), _dev())])
    assert int(out["range"][0]) == TAG
    keep = ~block_mask(SCALE_SHAPE, plan, rescaled)
    for name in ("b1", "b2"):
        got = interior(out[name])
        sel = keep[:, None].expand_as(got)
        assert bool(torch.isfinite(got[sel]).all())
        check(got, ref[name][0], bound16(ref, name, np.full((B, H, W), 16.0)), f"inf {name}", sel=sel)
    check_planes_and_slots(out, 1, B, H, W)
    slots = out["amax"].reshape(B, plan[1], plan[0], 4)
    assert bool(torch.isinf(slots[0, 2, 0, 1])) and bool(torch.isinf(slots[0, 1, 0, 1]))      # rows 3..5, columns 19..21: wave 1
    assert bool(torch.isfinite(slots[1]).all()) and bool(torch.isfinite(slots[0, 0]).all()) and bool(torch.isfinite(slots[0, :, 1:]).all())
