"""Host half of tests/test_gpu_train_ops_kernels.py -- no GPU: the geometries the device test runs (defined here, imported there), the
CPU references of unfold and fold with their adjoint identity, the head room of the integer cases, and the argument checks of the
train_ops.hip entries that never reach the device."""
import itertools

import pytest
import torch

# (B, C, k, stride, oy, ox, oh, ow, Hp, Wp): every k x stride x C, B of 1 and 3 alternating; for each, a map the windows end exactly
# on (last row and column, oy = ox = 0) and one with offsets and slack.  stride 4 with k of 1 and 3 leaves gaps between the windows.
def geometries():
    out = []
    for n, (k, stride, C) in enumerate(itertools.product((1, 3, 7), (1, 4), (4, 16, 64))):
        B = (1, 3)[n % 2]
        oh, ow = 5, 6
        out.append((B, C, k, stride, 0, 0, oh, ow, (oh - 1) * stride + k, (ow - 1) * stride + k))
        Hp, Wp = 2 + (oh - 1) * stride + k + 2, 1 + (ow - 1) * stride + k + 2
        out.append((4 - B, C, k, stride, 2, 1, oh, ow, Hp, Wp + (Wp % 2 == 0)))       # odd x odd: never whole blocks of float4
    out.append((2, 16, 7, 1, 0, 0, 17, 24, 23, 30))                     # the key grid of a 17 x 24 map: 408 patches
    return out


GEOMETRIES = geometries()
COL_SUM_COLS = (1, 3, 16, 20, 100, 129, 196, 255, 256)
COL_SUM_ROWS = (1, 255, 256, 257, 513, 64 * 256 + 1)                    # the last: more than 64 partials (a second round of the final sum)
PRELU_SIZES = (4, 8188, 8192, 8196)                                     # around one block's 2048 float4


def gid(g):
    return "B{}C{}k{}s{}o{}{}_{}x{}".format(*g[:6], g[8], g[9])


def unfold_ref(pmap, k, stride, oy, ox, oh, ow):
    """rows[(b,py,px), (kh,kw,c)] = pmap[b, oy + py*stride + kh, ox + px*stride + kw, c] by indexing."""
    B, _, _, C = pmap.shape
    cols = [pmap[:, oy + kh: oy + kh + (oh - 1) * stride + 1: stride, ox + kw: ox + kw + (ow - 1) * stride + 1: stride, :]
            for kh in range(k) for kw in range(k)]
    return torch.stack(cols, dim=3).reshape(B * oh * ow, k * k * C)


def fold_ref(rows, shape, k, stride, oy, ox, oh, ow):
    """The scatter-add adjoint in fp64; pixels no window covers stay 0."""
    B, Hp, Wp, C = shape
    r = rows.double().view(B, oh, ow, k, k, C)
    out = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            out[:, oy + kh: oy + kh + (oh - 1) * stride + 1: stride, ox + kw: ox + kw + (ow - 1) * stride + 1: stride, :] += r[:, :, :, kh, kw, :]
    return out


def int_map_and_rows(g):
    B, C, k, stride, oy, ox, oh, ow, Hp, Wp = g
    gen = torch.Generator().manual_seed(hash(g) % (1 << 31))
    pmap = torch.randint(-8, 9, (B, Hp, Wp, C), generator=gen).float()
    rows = torch.randint(-8, 9, (B * oh * ow, k * k * C), generator=gen).float()
    return pmap, rows


@pytest.mark.parametrize("g", GEOMETRIES, ids=gid)
def test_references_are_adjoint_and_exact(g):
    B, C, k, stride, oy, ox, oh, ow, Hp, Wp = g
    assert oy + (oh - 1) * stride + k <= Hp and ox + (ow - 1) * stride + k <= Wp
    assert (oh * ow * k * k * (C // 4)) % 256 != 0 and (Hp * Wp * (C // 4)) % 256 != 0        # a last block with idle threads
    pmap, rows = int_map_and_rows(g)
    folded = fold_ref(rows, pmap.shape, k, stride, oy, ox, oh, ow)
    lhs = (unfold_ref(pmap.double(), k, stride, oy, ox, oh, ow) * rows.double()).sum()
    assert float(lhs) == float((pmap.double() * folded).sum())
    # at most k*k terms of magnitude <= 8 per pixel: far below 2^24, every fp32 partial sum is exact
    assert float(fold_ref(rows.abs(), pmap.shape, k, stride, oy, ox, oh, ow).max()) <= 8 * k * k < 2 ** 24


def test_the_geometries_hold_every_class():
    assert {(g[2], g[3], g[1]) for g in GEOMETRIES} >= set(itertools.product((1, 3, 7), (1, 4), (4, 16, 64)))
    assert {g[0] for g in GEOMETRIES} >= {1, 3}
    exact = [g for g in GEOMETRIES if g[4] + (g[6] - 1) * g[3] + g[2] == g[8] and g[5] + (g[7] - 1) * g[3] + g[2] == g[9]]
    assert len(exact) >= 18 and any(g[4] > 0 and g[5] > 0 for g in GEOMETRIES)
    assert any(g[3] > g[2] for g in GEOMETRIES)                          # gaps between the windows


def test_col_sum_integer_head_room():
    assert 8 * max(COL_SUM_ROWS) < 2 ** 24                              # integers in [-8, 8]: the fp64 sums and their fp32 cast are exact


@pytest.fixture(scope="module")
def lib():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    return _lib.load()


_FAKE = 0x10000


def test_col_sum_scratch_and_refusals(lib):
    size = lib.dagl_col_sum_scratch_bytes
    assert size(0, 16) == 0 and size(1, 16) == 128 and size(256, 3) == 24 and size(257, 3) == 48 and size(64 * 256 + 1, 256) == 65 * 256 * 8
    for cols in (0, 257, -1):
        assert lib.dagl_col_sum(None, 8, cols, _FAKE, _FAKE, _FAKE) == -1 and b"dagl_col_sum" in lib.dagl_last_error(), cols
    assert lib.dagl_col_sum(None, 8, 16, _FAKE, _FAKE, None) == -1       # rows > 0: the scratch is required
    assert lib.dagl_col_sum(None, 8, 16, None, _FAKE, _FAKE) == -1
    assert lib.dagl_col_sum(None, 0, 16, None, None, None) == -1         # ... and an output always


def test_patch_geometry_refusals(lib):
    for entry in (lib.dagl_unfold_patches, lib.dagl_fold_patches):
        ok = (1, 10, 10, 4, 3, 1, 0, 0, 8, 8)
        for i, v in ((3, 6), (3, 0), (8, 9), (9, 9), (6, 1), (4, 0), (5, 0), (0, 0)):
            bad = list(ok); bad[i] = v
            assert entry(None, *bad, _FAKE, _FAKE) == -1 and b"bad argument" in lib.dagl_last_error(), (i, v)
        assert entry(None, *ok, None, _FAKE) == -1 and entry(None, *ok, _FAKE, None) == -1
