"""The split-fp16 patch projection (csrc/project16.hip, project16_kernel) element by element against fp64, through the read-out entry
``dagl_ce_project16_debug`` (the inference launch with every output in the caller's buffers) and the training entry
``dagl_project_patches16``, at the smallest shapes of every class of the launch plan: tests/test_project16_plan_host.py pins each case's
plan at 256 compute units and names its class, and the first test here asserts that the device plans the same.

Inputs: per-image distinct maps (randn), per-head distinct weights (randn x 0.05) and biases (randn x 0.1); the planes are built in numpy,
hi = fp16(16 a), lo = fp16(16 a - hi), so the activation split is no part of this test's error model (tests/test_gpu_prologue16.py proves
the planes bit-exact).  One variant has a non-zero 3-pixel border: the kernel is a patch Linear over the PADDED map.  Every output buffer
is poisoned before the call (NaN in the floats, 0x5A5A in the 16-bit copies): what the kernel does not store must still be there.

Reference: fp64 relu(unfold(a) W^T + bias) with a = (hi + lo) / 16 exactly (256 (hi2 + lo2) on the coarse tier), error unit
    u = unfold(|a|) |W|^T + |bias|                                          (fp64)
Value check, every element of the fp32 rows of X and Wq:
    |got - ref| <= K 2^-22 u + floor               (ReLU is 1-Lipschitz: the bound holds behind it)
  * K = 3 + 2 r32: 3 for the weight split (1024 w = hi + lo), the dropped lo lo term and the fp32 rounding of the scaled sum; r32 = the
    largest per-element error of torch's fp32 CPU product over the same cases in units of 2^-22 u (a reference, never the kernel), twice
    for another summation order.
  * floor = 2^-35 sum_window |a|: a half below 2^-14 is a multiple of 2^-24, so hi + lo misses 1024 w by up to 2^-25 once |1024 w| < 2^-3
    (|w| < 1.2e-4), i.e. up to 2^-35 per weight whatever its size; the activations are exact.  Derived, not measured.
``test_floor_is_small`` shows on the CPU that the floor stays under 10 % of the bound at every element; ``test_checker_flags_*`` feed the
checker a reference in which one patch lost the a_lo w_hi term of one tap, and one in which one halo column was read a pixel off: both
are flagged, so the bound can fail.

Measured: r32 = 0.79 on the CPU, K = 4.57.  Worst |got - ref| / bound of one run on the MI355X per case, keys / queries (printed
as "[project16] ..."):
  1,1,1.1 0.07 / -      1,1,1.2 - / 0.07      1,1,1.3 0.07 / 0.07    1,2,3.3 0.06 / 0.07    1,5,9.3 0.05 / 0.10     1,7,31.3 0.07 / 0.08
  3,16,16.3 0.16 / 0.09  1,9,32.3 0.09 / 0.10  1,8,33.3 0.08 / 0.08   1,3,70.3 0.07 / 0.09   2,9,38.3 0.11 / 0.11    2,45,38.1 0.15 / -
  2,45,38.3 0.15 / 0.12  2,63,50.1 0.16 / -    144,8,32.1 0.19 / -    144,8,1.1 0.13 / -     144,8,32.3 0.19 / 0.17
  (DESIGN.md section 5 has the table with classes and routes)

Exact checks against the same call's own fp32 rows: the bf16 copies == RNE bf16(v) in columns 0..195 with 196..207 zero, row-major and in
the screen's fragment order (a 32-row tile at halfs 32 T 216, half-tile p at + 3328 p, chunk t of 8 columns, row r at (16 t + r) 8);
row-major columns 208..215 are zero-filled by the two-group blocks and not written by the single-tile blocks -- the screen streams them
into the LDS with the row, but its fragment reads end at column 207, and nothing else reads the bf16 rows past it: they are unspecified
and not checked for single-tile rows.  The split copies: hi == fp16(64 v), lo == fp16(64 v - hi), columns 196..215 zero on both routes.
Every row >= N (keys) or >= L (queries) of every buffer, and the unused positions inside the last fragment-order tile, keep the fill.
rowsum: keys of two-group blocks have slots 1, 2, 3, 5, 6, 7 zero and the group sums in 0 and 4, keys of single-tile blocks a tile's sum
in each of slots 0..6 and the fill in slot 7 (pivot.hip does not read it); which key took which route comes from the plan.  Nothing is
written while the policy word is non-zero.  The range word is untouched while everything is in range.

Sums (the features are >= 0, so the bounds are relative, depth 2^-24 sum, depth = the longest fp32 addition chain read from the code):
  * pivot_rowsum's slot-order sum: depth 15 = 4 tile adds per lane + 5 exchange levels of the butterfly + 6 slot adds (two-group route;
    the single-tile route has 1 + 4 + 6);
  * colsum[b][c]: depth 37 = 32 rows per lane (2 items x 16 rows) + 1 across the row halves + 4 waves, then fp64 over the blocks.

Where the issue's list of routes was off (measured with the plan entry):
  * (2,45,38) . 3 has n_full = 18 = 16 XCD-mapped ids + a tail of 2, not tail ids only; . 1 (n_full = 14) is the tail-only case.
  * A head of a multi-head call equals the single-head call on the same images bit for bit only where both calls serve the image by the
    same route: the two routes add the three product terms in different orders (one accumulator / three).  The last image of a call
    runs single-tile, so the last image of every head but the last is on the other route in the two calls; the test compares those rows
    against fp64 with the bound and all others bit for bit (queries: always bit for bit).
  * A slot of +inf does not set the range word in this kernel: it selects the coarse tier.  The word is set by the kernel that wrote the
    slot (conv_pair16_kernel, tests/test_gpu_prologue16.py).  Here: a packed weight >= 60000 / 1024 and a split copy of 64 v >= 60000 do."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_project16_plan_host import CASES, CUS, FIELDS, single_tile_units

gpu = pytest.mark.gpu

U22, U24, U35 = 2.0 ** -22, 2.0 ** -24, 2.0 ** -35
D, DS, DSH, DPAD = 196, 204, 216, 208
FILL16 = 0x5A5A
RANGE_INIT, TAG = 0x5A5A, 77
DEPTH_ROW, DEPTH_COL = 15, 37
SHAPES = sorted({c[:3] for c in CASES})
TABLE = sorted(CASES)
BORDER_TABLE = [c for c in TABLE if c[0] <= 3 and c[3] == 3]
ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(head=0):
    """One head's parameters in Linear order [196][c][tap] (shared by every case)."""
    g = torch.Generator().manual_seed(1600 + head)
    r = lambda s, *shape: torch.randn(*shape, generator=g) * s
    return dict(fc1_w=r(0.05, D, 784), fc1_b=r(0.1, D), fc2_w=r(0.05, D, 784), fc2_b=r(0.1, D))


def split_planes(a32, scale):
    """numpy emulation of the split: (hi, lo) float16 with scale a = hi + lo up to the rounding of lo"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = a32.astype(np.float32) * np.float32(scale)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def exact_of(hi, lo, scale):
    return (hi.astype(np.float64) + lo.astype(np.float64)) / scale


@functools.lru_cache(maxsize=None)
def case_planes(shape, border=False, gain=1.0):
    """-> (hi, lo float16 [B,H+6,W+6,16], a = (hi + lo) / 16 float64): distinct images; a zero or a non-zero 3-pixel border."""
    B, H, W = shape
    a = torch.randn(B, H + 6, W + 6, 16, generator=torch.Generator().manual_seed(B * 10007 + H * 131 + W)).numpy() * np.float32(gain)
    if not border:
        inner = np.zeros_like(a)
        inner[:, 3:-3, 3:-3] = a[:, 3:-3, 3:-3]
        a = inner
    hi, lo = split_planes(a, 16.0)
    return hi, lo, exact_of(hi, lo, 16.0)


def same_pad_tl(H, W):
    """(top, left) of the SAME padding of the stride-4 query grid (make_grid, csrc/dagl_common.h)"""
    Lh, Lw = -(-H // 4), -(-W // 4)
    return max((Lh - 1) * 4 + 7 - H, 0) // 2, max((Lw - 1) * 4 + 7 - W, 0) // 2


def patch_rows(a, H, W, queries):
    """[B,H+6,W+6,16] -> [B, n, 784] patches in (c, kh, kw) order: every window of the padded map (keys), or the windows whose corner
    is 4 q - pad + 3 (queries)."""
    m = a.permute(0, 3, 1, 2)
    if not queries:
        return F.unfold(m, 7).transpose(1, 2)
    pt, pl = same_pad_tl(H, W)
    Lh, Lw = -(-H // 4), -(-W // 4)
    crop = m[:, :, 3 - pt:, 3 - pl:]
    nh, nw = (crop.shape[2] - 7) // 4 + 1, (crop.shape[3] - 7) // 4 + 1
    assert nh >= Lh and nw >= Lw
    u = F.unfold(crop, 7, stride=4).reshape(a.shape[0], 784, nh, nw)[:, :, :Lh, :Lw]
    return u.reshape(a.shape[0], 784, Lh * Lw).transpose(1, 2)


def reference(exact, H, W, heads=1, sides=("x", "wq"), wfun=weights):
    """fp64 features of every image of ``exact`` [heads*imgs, H+6, W+6, 16] with head h's weights: {side: (ref, u, sum_window |a|)} as
    [B, n, 196] / [B, n, 1] float64, and "r32": the largest error of torch's fp32 product in units of 2^-22 u."""
    a = torch.from_numpy(exact)
    imgs = a.shape[0] // heads
    out, r32 = {}, 0.0
    for side in sides:
        queries = side == "wq"
        refs, us, sas = [], [], []
        for h in range(heads):
            w, b = wfun(h)["fc1_w" if queries else "fc2_w"], wfun(h)["fc1_b" if queries else "fc2_b"]
            rows = patch_rows(a[h * imgs:(h + 1) * imgs], H, W, queries)
            ref = torch.relu(rows @ w.double().T + b.double())
            u = rows.abs() @ w.double().abs().T + b.double().abs()
            got32 = torch.relu(rows.float() @ w.T + b)
            r32 = max(r32, float(((got32.double() - ref).abs() / (U22 * u)).max()))
            refs.append(ref); us.append(u); sas.append(rows.abs().sum(dim=2, keepdim=True))
        out[side] = tuple(torch.cat(t).numpy() for t in (refs, us, sas))
    out["r32"] = r32
    return out


@functools.lru_cache(maxsize=None)
def case_reference(shape, border=False):
    return reference(case_planes(shape, border)[2], shape[1], shape[2])


@functools.lru_cache(maxsize=None)
def r32():
    return max(case_reference(s)["r32"] for s in SHAPES)


def K():
    return 3.0 + 2.0 * r32()


def bound_of(ref_side):
    _, u, sa = ref_side
    return K() * U22 * u + U35 * sa


def check(got, ref_side, what):
    """Every element within its bound (a NaN fails); prints and returns the worst ratio."""
    ratio = np.abs(got.astype(np.float64) - ref_side[0]) / bound_of(ref_side)
    bad = ~(ratio <= 1.0)
    worst = float(np.nan_to_num(ratio, nan=np.inf).max()) if ratio.size else 0.0
    print(f"[project16] {what}: worst |err| / bound {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the bound, worst ratio {worst:.3f}, first at {np.argwhere(bad)[0]}"
    return worst


# ---- CPU: the model's own consistency ------------------------------------------------------------------------------------------------
SMALL = (1, 5, 9)


def test_floor_is_small():
    """At these input scales the floor is under a tenth of the bound at every element of every case (reference alone)."""
    print(f"[project16] r32 {r32():.3f}  K {K():.3f}")
    assert 0.05 < r32() < 8.0                                            # a sane fp32 reference: a few units of 2^-22 u at most
    for shape in SHAPES:
        for side in ("x", "wq"):
            ref = case_reference(shape)[side]
            assert float((U35 * ref[2] / bound_of(ref)).max()) < 0.1, (shape, side)


def _small_rows():
    hi, lo, exact = case_planes(SMALL)
    rows = patch_rows(torch.from_numpy(exact), 5, 9, False)[0]                       # [45, 784]
    rows_lo = patch_rows(torch.from_numpy(lo.astype(np.float64) / 16.0), 5, 9, False)[0]
    return rows, rows_lo


def test_checker_flags_a_lost_cross_term():
    """One patch without the a_lo w_hi term of a single tap: beyond the bound."""
    w, b = weights()["fc2_w"].double(), weights()["fc2_b"].double()
    w_hi = torch.from_numpy(split_planes(w.float().numpy(), 1024.0)[0].astype(np.float64) / 1024.0)
    rows, rows_lo = _small_rows()
    patch, tap = 22, 24                                                  # the centre patch, the centre tap
    cols = torch.arange(16) * 49 + tap
    pre = rows @ w.T + b
    pre[patch] -= rows_lo[patch, cols] @ w_hi[:, cols].T
    wrong = torch.relu(pre).numpy()[None]
    ref = case_reference(SMALL)["x"]
    check(ref[0], ref, "the reference itself")
    with pytest.raises(AssertionError, match="beyond the bound"):
        check(wrong, ref, "lost a_lo w_hi of one tap")
    off = np.abs(wrong - ref[0]) > bound_of(ref)
    assert off[0, patch].any() and not np.delete(off[0], patch, axis=0).any()


def test_checker_flags_a_shifted_halo_column():
    """One patch whose first halo column (kw = 4 of the last patch of a row: the border) was read a pixel to the left: beyond the bound."""
    w, b = weights()["fc2_w"].double(), weights()["fc2_b"].double()
    rows, _ = _small_rows()
    patch = 8                                                            # (0, 8): the last patch of row 0
    r = rows.clone().reshape(45, 16, 7, 7)
    assert bool((r[patch, :, :, 4] == 0).all()) and bool((r[patch, :, 3:, 3] != 0).all())      # kw = 3: the map's last column
    r[patch, :, :, 4] = r[patch, :, :, 3]
    wrong = torch.relu(r.reshape(45, 784) @ w.T + b).numpy()[None]
    ref = case_reference(SMALL)["x"]
    with pytest.raises(AssertionError, match="beyond the bound"):
        check(wrong, ref, "halo column a pixel off")


def test_fp32_map_of_the_planes_is_exact():
    """(hi + lo) / 16 is an fp32 number and splits back into the same sum: the training entry sees the reference's activations."""
    for shape in ((1, 5, 9), (2, 9, 38)):
        for border in (False, True):
            hi, lo, exact = case_planes(shape, border)
            a32 = exact.astype(np.float32)
            assert np.array_equal(a32.astype(np.float64), exact)
            h2, l2 = split_planes(a32, 16.0)
            assert np.array_equal(exact_of(h2, l2, 16.0), exact)


# ---- GPU: one call --------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _bits(a16):
    return torch.from_numpy(np.ascontiguousarray(a16).view(np.int16)).to(_dev())


@functools.lru_cache(maxsize=None)
def _dev_weights(head):
    return {k: v.to(_dev()).contiguous() for k, v in weights(head).items()}


def call(hi, lo, H, W, which=3, heads=1, head_ids=None, wlist=None, full=True, **kw):
    """One ``ops.ce_project16_debug`` call on numpy float16 planes -> dict of numpy arrays (None where not asked for).  ``full``: every
    secondary output on (the query bf16 copy in fragment order unless ``q_tiled=False``)."""
    from dagl_amd import ops
    ws = wlist if wlist is not None else [_dev_weights(h) for h in (head_ids if head_ids is not None else range(heads))]
    args = dict(tag=TAG, range_init=RANGE_INIT)
    if full:
        args.update(bf16=True, q_tiled=True, split=True, colsum=bool(which & 1), rowsum=bool(which & 1), policy=0 if which & 1 else None)
    args.update(kw)
    for k in ("map_hi2", "map_lo2"):
        if args.get(k) is not None:
            args[k] = _bits(args[k])
    if args.get("amax") is not None:
        args["amax"] = torch.from_numpy(args["amax"]).to(_dev())
    out = ops.ce_project16_debug(_bits(hi), _bits(lo), H, W, heads=heads, which=which, fc1_w=[w["fc1_w"] for w in ws],
                                 fc1_b=[w["fc1_b"] for w in ws], fc2_w=[w["fc2_w"] for w in ws], fc2_b=[w["fc2_b"] for w in ws], **args)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@functools.lru_cache(maxsize=6)
def device_run(case, border=False, q_tiled=True):
    B, H, W, which = case
    hi, lo, _ = case_planes((B, H, W), border)
    return call(hi, lo, H, W, which, q_tiled=q_tiled)


def sides_of(which):
    return [s for s, bit in (("x", 1), ("wq", 2)) if which & bit]


def rows_of(side, H, W):
    return H * W if side == "x" else -(-H // 4) * -(-W // 4)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_values(out, ref, H, W, which, what):
    """The fp32 rows per element; -> {side: worst ratio}"""
    worst = {}
    for side in sides_of(which):
        n = rows_of(side, H, W)
        feat = out[side]
        assert feat.shape[2] == DS and feat.shape[1] >= n
        worst[side] = check(feat[:, :n, :D], ref[side], f"{what} {side}")
        assert (feat[:, :n, D:] == 0).all(), f"{what} {side}: columns 196..203 are not zero"
        assert np.isnan(feat[:, n:]).all(), f"{what} {side}: a row past the last patch was written"
    return worst


def bf16_bits(v32):
    u = np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def single_tile_rows(case):
    """bool [B, N]: the keys served by single-tile blocks, from the plan"""
    B, H, W, which = case
    p = dict(zip(FIELDS, CASES[case][0])) if case in CASES else _plan(case)
    n = np.arange(H * W)
    item = n // 32 if p["lin"] else (n // W) * p["segs_k"] + (n % W) // 32
    mask = np.zeros((B, H * W), dtype=bool)
    for b, unit in single_tile_units(B, tuple(p[f] for f in FIELDS)):
        mask[b] |= (item // 8) == unit
    return mask


def _plan(case):
    from dagl_amd import ops
    return ops.project16_plan(*case, cus=CUS)


def check_copies(out, case, q_tiled, what):
    """bf16 and split copies against the call's own fp32 rows, whole buffers: values, zero columns, fill everywhere else."""
    B, H, W, which = case
    for side in sides_of(which):
        n = rows_of(side, H, W)
        v = out[side][:, :n, :D]
        # ---- bf16 ------------------------------------------------------------------------------------------------------------------
        got = out[side + "_bf16"].view(np.uint16)
        bits = np.zeros((B, n, DPAD), dtype=np.uint16)
        bits[:, :, :D] = bf16_bits(v)
        want = np.full(got.shape, FILL16, dtype=np.uint16)
        care = np.ones(got.shape, dtype=bool)
        if side == "wq" and q_tiled:
            flat = want.reshape(B, -1)
            for row0 in range(0, n, 16):
                T, p = row0 // 32, (row0 // 16) & 1
                seg = flat[:, T * 32 * DSH + 3328 * p:T * 32 * DSH + 3328 * (p + 1)].reshape(B, 26, 16, 8)
                for r in range(min(16, n - row0)):
                    seg[:, :, r, :] = bits[:, row0 + r].reshape(B, 26, 8)
        else:
            want[:, :n, :DPAD] = bits
            want[:, :n, DPAD:] = 0
            if side == "x":
                care[:, :n, DPAD:] = ~single_tile_rows(case)[:, :, None]          # (single-tile blocks: columns 208..215 unspecified)
        diff = (got != want) & care
        assert not diff.any(), f"{what} {side}_bf16: {int(diff.sum())} halves differ, first at {np.argwhere(diff)[0]}"
        # ---- split -----------------------------------------------------------------------------------------------------------------
        hi, lo = split_planes(v, 64.0)
        for name, halves in ((side + "_hi", hi), (side + "_lo", lo)) if out[side + "_hi"] is not None else ():
            got = out[name].view(np.uint16)
            want = np.full(got.shape, FILL16, dtype=np.uint16)
            want[:, :n, :D] = halves.view(np.uint16)
            want[:, :n, D:] = 0
            diff = got != want
            assert not diff.any(), f"{what} {name}: {int(diff.sum())} halves differ, first at {np.argwhere(diff)[0]}"


def check_sums(out, case, what):
    """rowsum per slot and route, pivot_rowsum's slot-order sum, colsum -- against the fp64 sums of the call's own fp32 features."""
    B, H, W, which = case
    N = H * W
    X = out["x"][:, :N, :D].astype(np.float64)
    rs = out["rowsum"]
    assert rs.shape == (B, N, 8)
    single = single_tile_rows(case)
    two = rs[~single]                                                    # [keys, 8]
    assert (two[:, [1, 2, 3, 5, 6, 7]] == 0).all(), f"{what}: a two-group key has a non-zero spare slot"
    parts = {0: X[~single][:, :128].sum(axis=1), 4: X[~single][:, 128:].sum(axis=1)}
    for slot, want in parts.items():
        assert (np.abs(two[:, slot] - want) <= DEPTH_ROW * U24 * want).all(), f"{what}: slot {slot} of the two-group keys"
    one = rs[single]
    assert np.isnan(one[:, 7]).all(), f"{what}: slot 7 of a single-tile key was written"
    for t in range(7):
        want = X[single][:, 32 * t:32 * t + 32].sum(axis=1)
        assert (np.abs(one[:, t] - want) <= DEPTH_ROW * U24 * want).all(), f"{what}: slot {t} of the single-tile keys"
    s = rs[:, :, 0]
    for t in range(1, 7):
        s = (s + rs[:, :, t]).astype(np.float32)                         # pivot_rowsum's order, fp32
    want = X.sum(axis=2)
    err = np.abs(s - want)
    assert (err <= DEPTH_ROW * U24 * want).all(), f"{what}: slot-order row sum, worst {float((err / (U24 * want + 1e-300)).max()):.2f} x 2^-24"
    cs = out["colsum"]
    assert cs.shape == (B, DS) and np.isnan(cs[:, D:]).all(), f"{what}: colsum columns >= 196 were written"
    want = X.sum(axis=1)
    err = np.abs(cs[:, :D] - want)
    assert (err <= DEPTH_COL * U24 * want).all(), f"{what}: colsum, worst {float((err / (U24 * want + 1e-300)).max()):.2f} x 2^-24"
    print(f"[project16] {what}: single-tile keys {int(single.sum())} of {single.size}")


# ---- GPU: the table -------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_device_plans_the_pinned_cases():
    """cus = 0 (this device) gives the 256-CU plan of every case: the table means what it says on the machine that runs it."""
    from dagl_amd import ops
    for case in TABLE:
        assert tuple(ops.project16_plan(*case, cus=0).values()) == CASES[case][0], case


@gpu
@pytest.mark.parametrize("case", TABLE, ids=ids)
def test_values_per_element(case):
    B, H, W, which = case
    out = device_run(case)
    worst = check_values(out, case_reference((B, H, W)), H, W, which, f"{case}")
    assert int(out["range"][0]) == RANGE_INIT
    print(f"[project16] {case} worst/bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@gpu
@pytest.mark.parametrize("case", BORDER_TABLE, ids=ids)
def test_values_with_a_nonzero_border(case):
    B, H, W, which = case
    out = device_run(case, border=True)
    check_values(out, case_reference((B, H, W), True), H, W, which, f"{case} border")


@gpu
@pytest.mark.parametrize("case", TABLE, ids=ids)
def test_copies_fill_and_sums(case):
    B, H, W, which = case
    out = device_run(case)
    check_copies(out, case, True, f"{case}")
    if which & 1:
        check_sums(out, case, f"{case}")
    assert int(out["range"][0]) == RANGE_INIT


@gpu
@pytest.mark.parametrize("case", TABLE, ids=ids)
def test_row_major_query_copy_and_a_second_call(case):
    """The same call with the query copy row-major: that copy is checked, every other output has the first call's bits."""
    B, H, W, which = case
    first, out = device_run(case), device_run(case, q_tiled=False)
    check_copies(out, case, False, f"{case} row-major")
    for k, v in out.items():
        if k != "wq_bf16":                                               # (the unspecified columns of x_bf16 hold the same fill in both)
            assert same_bits(v, first[k]), f"{case} {k}: a second call gives other bits"


@gpu
def test_policy_word_stops_the_row_sums():
    for case in ((1, 5, 9, 3), (2, 9, 38, 3)):
        B, H, W, which = case
        hi, lo, _ = case_planes((B, H, W))
        ref = device_run(case)
        out = call(hi, lo, H, W, which, policy=3)
        assert np.isnan(out["rowsum"]).all(), f"{case}: row sums written under a non-zero policy word"
        no_word = call(hi, lo, H, W, which, policy=None)
        for k in ref:
            assert same_bits(no_word[k], ref[k]), f"{case} {k}: no policy word"
            if k != "rowsum":
                assert same_bits(out[k], ref[k]), f"{case} {k}: policy word set"


@gpu
def test_plain_call_without_secondary_outputs():
    """Only the fp32 rows asked for: the same bits as the call with every switch on."""
    for case in ((3, 16, 16, 3), (2, 9, 38, 1), (2, 9, 38, 2)):
        B, H, W, which = case
        hi, lo, _ = case_planes((B, H, W))
        out = call(hi, lo, H, W, which, full=False)
        check_values(out, case_reference((B, H, W)), H, W, which, f"{case} plain")
        assert all(out[k] is None for k in out if k not in sides_of(which) + ["range"])
        if case in CASES:
            for side in sides_of(which):
                assert same_bits(out[side], device_run(case)[side]), f"{case} {side}"


# ---- heads and tiers ------------------------------------------------------------------------------------------------------------------
HEAD_SHAPE = (8, 9, 38)               # two images per head: heads = 2 uses the first four, heads = 4 all eight


@gpu
@pytest.mark.parametrize("heads", (2, 4))
def test_heads(heads):
    imgs, (_, H, W) = 2, HEAD_SHAPE
    hi, lo, exact = case_planes(HEAD_SHAPE)
    B = heads * imgs
    out = call(hi[:B], lo[:B], H, W, 3, heads=heads)
    check_values(out, reference(exact[:B], H, W, heads=heads), H, W, 3, f"{heads} heads")
    check_copies(out, (B, H, W, 3), True, f"{heads} heads")
    check_sums(out, (B, H, W, 3), f"{heads} heads")
    N, L = H * W, rows_of("wq", H, W)
    for h in range(heads):
        sl = slice(h * imgs, (h + 1) * imgs)
        alone = call(hi[sl], lo[sl], H, W, 3, heads=1, head_ids=[h])
        assert same_bits(out["wq"][sl], alone["wq"]), f"head {h}: queries differ from the single-head call"
        assert same_bits(out["wq_bf16"][sl], alone["wq_bf16"]) and same_bits(out["wq_hi"][sl], alone["wq_hi"])
        # keys: the last image of the single-head call runs single-tile; in the multi-head call only the very last image does
        same_route = imgs if h == heads - 1 else imgs - 1
        assert same_bits(out["x"][sl][:same_route], alone["x"][:same_route]), f"head {h}: keys differ from the single-head call"
        assert same_bits(out["x_lo"][sl][:same_route], alone["x_lo"][:same_route])
        assert same_bits(out["colsum"][sl][:same_route], alone["colsum"][:same_route])


TIER_SHAPE = (2, 9, 38)               # heads = 2 x one image: image 0 on two-group blocks, image 1 (keys) single-tile
TIER_PLACES = ((4, 0), (4, 3), (8, 7), (1028, 0), (1028, 1023), (1028, 1024), (1028, 1027))


@functools.lru_cache(maxsize=None)
def tier_inputs(coarse_head):
    """Head ``coarse_head``: |a| ~ 1e5 in the coarse planes (2^-8 a = hi2 + lo2), fine planes fp16(16 a) = inf; the other head: an ordinary
    map in the fine planes and NaN in the coarse ones.  -> planes and the fp64 reference of both heads"""
    _, H, W = TIER_SHAPE
    hi, lo, exact = (t.copy() for t in case_planes(TIER_SHAPE))
    big = case_planes(TIER_SHAPE)[2][coarse_head].astype(np.float32) * np.float32(1.0e5)
    hi2 = np.full(hi.shape, np.nan, dtype=np.float16)
    lo2 = np.full(hi.shape, np.nan, dtype=np.float16)
    hi2[coarse_head], lo2[coarse_head] = split_planes(big, 1.0 / 256.0)
    hi[coarse_head], lo[coarse_head] = split_planes(big, 16.0)
    assert np.isinf(hi[coarse_head]).any()
    exact[coarse_head] = exact_of(hi2[coarse_head], lo2[coarse_head], 1.0 / 256.0)
    return hi, lo, hi2, lo2, reference(exact, H, W, heads=2)


@gpu
@pytest.mark.parametrize("coarse_head", (0, 1))
@pytest.mark.parametrize("place", TIER_PLACES, ids=ids)
def test_tier_choice_per_head(place, coarse_head):
    """The deciding slot (3750: the first value on the coarse tier) at the first, the last, a clamped and a tail-loop index; the other
    head's largest slot is 3749 at the same place (still fine) and its coarse planes are NaN."""
    slots, index = place
    _, H, W = TIER_SHAPE
    hi, lo, hi2, lo2, ref = tier_inputs(coarse_head)
    amax = np.zeros((2, slots), dtype=np.float32)
    amax[1 - coarse_head] = 1.0
    amax[coarse_head, index], amax[1 - coarse_head, index] = 3750.0, 3749.0
    out = call(hi, lo, H, W, 3, heads=2, map_hi2=hi2, map_lo2=lo2, amax=amax)
    check_values(out, ref, H, W, 3, f"tiers {place} coarse head {coarse_head}")
    check_copies(out, (2, H, W, 3), True, f"tiers {place}")
    # |a| ~ 1e5 gives features past the split copies' range (64 v >= 60000): the word says so, and only because of them
    assert not (out["x"][coarse_head, :H * W, :D] * np.float32(64.0) < 60000.0).all()
    assert int(out["range"][0]) == TAG
    plain = call(hi, lo, H, W, 3, heads=2, map_hi2=hi2, map_lo2=lo2, amax=amax, split=False)
    assert int(plain["range"][0]) == RANGE_INIT
    for side in ("x", "wq"):
        assert same_bits(plain[side], out[side]) and same_bits(plain[side + "_bf16"], out[side + "_bf16"])


@gpu
def test_all_fine_and_all_coarse_and_an_inf_slot():
    _, H, W = TIER_SHAPE
    hi, lo, _ = case_planes(TIER_SHAPE)
    nanp = np.full(hi.shape, np.nan, dtype=np.float16)
    base = device_run(TIER_SHAPE + (3,))
    fine = call(hi, lo, H, W, 3, heads=2, head_ids=[0, 0], map_hi2=nanp, map_lo2=nanp, amax=np.full((2, 8), 3749.0, dtype=np.float32))
    for side in ("x", "wq"):
        assert same_bits(fine[side], base[side]), f"{side}: fine heads beside NaN coarse planes differ from the call without tiers"
    # both heads coarse through a slot of +inf: the coarse planes are multiplied, the fine ones (NaN) are not; the word stays
    exact = case_planes(TIER_SHAPE)[2]
    hi2, lo2 = split_planes(exact.astype(np.float32), 1.0 / 256.0)
    amax = np.zeros((2, 4), dtype=np.float32)
    amax[:, 2] = np.inf
    out = call(nanp, nanp, H, W, 3, heads=2, head_ids=[0, 0], map_hi2=hi2, map_lo2=lo2, amax=amax)
    ref = reference(exact_of(hi2, lo2, 1.0 / 256.0), H, W, heads=2, wfun=lambda h: weights(0))
    check_values(out, ref, H, W, 3, "inf slot, coarse planes")
    assert int(out["range"][0]) == RANGE_INIT


# ---- range ----------------------------------------------------------------------------------------------------------------------------
def _hot_weights(side):
    w = {k: v.clone() for k, v in _dev_weights(0).items()}
    w[side][7, 300] = 60000.0 / 1024.0 + 0.01                            # |1024 w| >= 60000, still a finite fp16 number
    return w


@gpu
@pytest.mark.parametrize("case", ((1, 5, 9, 3), (144, 8, 1, 1)), ids=ids)
def test_range_word(case):
    """A packed weight >= 60000 / 1024 (either side) and a split copy of 64 v >= 60000 (either route) set the word to the tag."""
    B, H, W, which = case
    hi, lo, _ = case_planes((B, H, W))
    for side in ("fc2_w", "fc1_w")[:2 if which & 2 else 1]:
        out = call(hi, lo, H, W, which, wlist=[_hot_weights(side)], full=False)
        assert int(out["range"][0]) == TAG, side
    big = {k: v.clone() for k, v in _dev_weights(0).items()}
    big["fc2_b"][5] = 1000.0                                             # 64 v = 64000 in column 5 of every key
    out = call(hi, lo, H, W, which, wlist=[big])
    assert int(out["range"][0]) == TAG
    out = call(hi, lo, H, W, which, wlist=[big], full=False)             # ... which nobody looks at without the split copies
    assert int(out["range"][0]) == RANGE_INIT
    assert int(call(hi, lo, H, W, which, full=False)["range"][0]) == RANGE_INIT


def rows_order(w):
    """Linear order [196][c][tap] -> the differentiable path's [196][tap][c]"""
    return w.reshape(D, 16, 49).permute(0, 2, 1).reshape(D, 784).contiguous()


@gpu
def test_patches16_poisons_an_out_of_range_call_and_recovers():
    """dagl_project_patches16 with the same weight: all NaN (never numbers from halves past the range); an in-range call behind it on the
    same scratch is finite and has the bits of a call on a fresh scratch."""
    from dagl_amd import _lib, ops
    lib = _lib.load()
    B, H, W = 2, 9, 38
    pmap = torch.from_numpy(case_planes((B, H, W))[2].astype(np.float32)).to(_dev())
    good, hot = _dev_weights(0), _hot_weights("fc2_w")
    need = lib.dagl_project_patches16_scratch_bytes(B, H, W, 0)
    buf = torch.full((need + 256,), 0xFF, device=_dev(), dtype=torch.uint8)
    base = buf.data_ptr() + (-buf.data_ptr()) % 256

    def run(w):
        y = torch.full((B * H * W, D), 7.0, device=_dev())
        wr = rows_order(w["fc2_w"])
        _lib.check(lib.dagl_project_patches16(ops._stream(), B, H, W, 0, pmap.data_ptr(), wr.data_ptr(), w["fc2_b"].data_ptr(), y.data_ptr(),
                                              base, need), "dagl_project_patches16")
        torch.cuda.synchronize()
        return y.cpu()

    assert bool(torch.isnan(run(hot)).all())
    after = run(good)
    assert bool(torch.isfinite(after).all())
    fresh = ops.project_patches16(pmap, rows_order(good["fc2_w"]), good["fc2_b"], H, W, False).cpu()
    assert torch.equal(after.view(torch.int32), fresh.view(torch.int32))


# ---- the training entry ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("queries", (False, True), ids=("keys", "queries"))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_training_entry_per_element(shape, queries):
    """ops.project_patches16 (rows-order weights; the map split on the device: (hi + lo) / 16 is an fp32 number that splits back exactly)."""
    from dagl_amd import ops
    B, H, W = shape
    side = "wq" if queries else "x"
    w = _dev_weights(0)
    pmap = torch.from_numpy(case_planes(shape)[2].astype(np.float32)).to(_dev())
    y = ops.project_patches16(pmap, rows_order(w["fc1_w" if queries else "fc2_w"]), w["fc1_b" if queries else "fc2_b"], H, W, queries)
    torch.cuda.synchronize()
    n = rows_of(side, H, W)
    assert tuple(y.shape) == (B * n, D)
    check(y.cpu().numpy().reshape(B, n, D), case_reference(shape)[side], f"{shape} project_patches16 {side}")


# ---- the thr / bias blocks behind the projection's own ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("heads,shape", ((1, (3, 16, 16)), (2, (4, 8, 36)), (1, (144, 8, 32))), ids=ids)
def test_ride_along_blocks(heads, shape):
    """((p0 + p1) + (p2 + p3)) + bias of the partials against fp64 with the bound of the 7x7 heads in tests/test_gpu_prologue16.py,
    (2 r32 + 1) 2^-22 u; every feature output has the bits of the same call without the blocks."""
    from tests.test_gpu_prologue16 import r32 as prologue_r32, same_pad
    B, H, W = shape
    imgs = B // heads
    hi, lo, _ = case_planes(shape)
    g = torch.Generator().manual_seed(77)
    xs = [torch.randn(imgs, 64, H, W, generator=g) for _ in range(heads)]
    tw = [torch.randn(1, 64, 7, 7, generator=g) * 0.1 for _ in range(heads)]
    bw = [torch.randn(1, 64, 7, 7, generator=g) * 0.1 for _ in range(heads)]
    tb, bb = torch.randn(heads, generator=g) * 0.1, torch.randn(heads, generator=g) * 0.1
    dev = lambda ts: [t.to(_dev()).contiguous() for t in ts]
    out = call(hi, lo, H, W, 3, heads=heads, thr=(dev(xs), dev(tw), dev(bw)))
    plain = device_run(shape + (3,)) if shape + (3,) in CASES else call(hi, lo, H, W, 3, heads=heads)
    for k, v in plain.items():
        if k != "thr_part":
            assert same_bits(out[k], v), f"{k}: the ride-along blocks changed a feature output"
    L = rows_of("wq", H, W)
    part = out["thr_part"]
    assert part.shape == (heads, 4, imgs, L, 2) and not np.isnan(part).any()
    bound_k = (2.0 * prologue_r32()[1] + 1.0) * U22
    pads = same_pad(H, W)
    for h in range(heads):
        x64 = F.pad(xs[h].double(), pads)
        for j, (w, b) in enumerate(((tw[h], tb[h]), (bw[h], bb[h]))):
            ref = F.conv2d(x64, w.double(), b.double().reshape(1), stride=4).reshape(imgs, L).numpy()
            u = F.conv2d(x64.abs(), w.double().abs(), b.double().abs().reshape(1), stride=4).reshape(imgs, L).numpy()
            p = part[h, :, :, :, j]
            got = ((p[0] + p[1]) + (p[2] + p[3])) + np.float32(b)
            assert got.dtype == np.float32
            ratio = np.abs(got.astype(np.float64) - ref) / (bound_k * u)
            print(f"[project16] ride-along {shape} head {h} {'thr' if j == 0 else 'bias'}: worst |err| / bound {float(ratio.max()):.3f}")
            assert (ratio <= 1.0).all(), f"head {h} output {j}: worst ratio {float(ratio.max()):.3f}"
