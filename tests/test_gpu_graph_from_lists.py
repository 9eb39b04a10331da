"""``ops.graph_from_lists`` (dagl_graph_from_lists, csrc/graph_lists.hip): fixed-width neighbour lists -> CSR, on hand-made lists.

The check is EXACT (``torch.equal``) against a plain torch evaluation of the entry's semantics on the CPU: row r owns the slots
t < min(max(cnt[r], 0), width); a slot whose key is outside [0, N) is dropped; the survivors are written in ascending key order, equal
keys in slot order; weight and score follow their key; row_off is the exclusive scan of the surviving degrees.  The kernel moves data:
no tolerance applies.

Crafted rows.  The first row (cnt 0) and the last (cnt < 0) are empty; with two images the rows on both sides of the image boundary
are empty as well.  The rows in between take the recipes of ``RECIPES`` in turn, starting at recipe ``rot``.  Every slot past a row's
count holds garbage (out-of-range keys included).  What a case holds is read back from the ARRAYS (``_kinds``) and asserted before
the call.  A map of 8 x 8 has four query rows, two of them between the empty ends: no single set of lists can hold every kind there,
so a shape whose rows do not take all recipes at once is run once per rotation that is needed, and the kinds are asserted over the
rotations together."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 8, 8),        # L = 4
          (2, 20, 36),      # L = 45, two images: empty rows on both sides of the image boundary
          (1, 45, 45),      # odd sizes
          (2, 92, 92)]      # B L = 1058 > 1024: the scan's threads own more than one row
WIDTHS = [1, 5, 8, 63, 64]
BIG = 2 ** 31 - 1
SENTINEL = -7


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _geom(shape):
    B, H, W = shape
    return B, H, W, (-(-H // 4)) * (-(-W // 4)), H * W


# a recipe: (generator, width, N, row) -> (cnt, the keys of the owned slots)
def _one(g, w, N, r):
    return 1, torch.randint(0, N, (1,), generator=g)


def _ascending(g, w, N, r):
    return w, torch.randperm(N, generator=g)[:w].sort().values


def _descending_overlong(g, w, N, r):                 # cnt > width: clamped
    return w + 3, torch.randperm(N, generator=g)[:w].sort(descending=True).values


def _random(g, w, N, r):
    return w, torch.randperm(N, generator=g)[:w]


def _repeated(g, w, N, r):                            # two or three distinct keys over the whole row
    pool = torch.randperm(N, generator=g)[:3]
    return w, pool[torch.randint(0, 3, (w,), generator=g)] if w > 1 else pool[:1]


def _with_invalid(which):
    def recipe(g, w, N, r):
        keys = torch.randperm(N, generator=g)[:w]
        bad = [N, -1, BIG]
        bad = bad[which:] + bad[:which]               # `which` first: it is the one a narrow row has room for
        for j, v in enumerate(bad[:max(1, min(3, w - 1))]):
            keys[(r + 2 * j) % w if w >= 5 else j] = v
        return w, keys
    return recipe


def _empty(g, w, N, r):
    return 0, torch.empty(0, dtype=torch.int64)


def _negative(g, w, N, r):
    return -2, torch.empty(0, dtype=torch.int64)


def _partial(g, w, N, r):
    c = int(torch.randint(1, w + 1, (1,), generator=g))
    return c, torch.randint(0, N, (c,), generator=g)


RECIPES = [_one, _ascending, _descending_overlong, _random, _repeated, _with_invalid(0), _with_invalid(1), _with_invalid(2), _empty,
           _negative, _partial]


@functools.lru_cache(maxsize=None)
def _crafted(shape, width, rot):
    """(idx [B,L,w] int32, wgt, s fp32, cnt [B,L] int32) on the CPU."""
    B, H, W, L, N = _geom(shape)
    R = B * L
    g = torch.Generator().manual_seed(7919 * width + 31 * rot + H)
    idx = torch.randint(-5, N + 6, (R, width), generator=g)                       # garbage everywhere first
    idx[torch.rand(R, width, generator=g) < 0.1] = BIG
    idx[:, -1] = N + 1                                                            # (every unowned tail holds an out-of-range key)
    wgt = (torch.randperm(R * width, generator=g).float() + 1.0).view(R, width)   # all distinct: a swap of equal keys would show
    s = torch.randn(R, width, generator=g)
    cnt = torch.zeros(R, dtype=torch.int64)
    cnt[R - 1] = -3
    boundary = {L - 1: 0, L: -1} if B > 1 else {}
    j = rot
    for r in range(1, R - 1):
        if r in boundary:
            cnt[r] = boundary[r]
            continue
        c, keys = RECIPES[j % len(RECIPES)](g, width, N, r)
        j += 1
        cnt[r] = c
        idx[r, :keys.numel()] = keys
    return idx.int().view(B, L, width), wgt.view(B, L, width), s.view(B, L, width), cnt.int().view(B, L)


def _rotations(shape):
    """The rotations a shape needs for its middle rows to take every recipe."""
    B, H, W, L, N = _geom(shape)
    middle = B * L - 2 - (2 if B > 1 else 0)
    return tuple(range(0, len(RECIPES), middle)) if middle < len(RECIPES) else (0,)


def _kinds(idx, cnt, N):
    """Names of the kinds of row the arrays hold."""
    B, L, w = idx.shape
    idx, cnt = idx.view(B * L, w).long(), cnt.view(-1).long()
    found = set()
    for name, m in (("cnt0", cnt == 0), ("cnt1", cnt == 1), ("cnt_width", cnt == w), ("cnt_clamped", cnt > w), ("cnt_negative", cnt < 0)):
        if bool(m.any()):
            found.add(name)
    if int(cnt[0]) <= 0 and int(cnt[-1]) <= 0:
        found.add("empty_ends")
    own = cnt.clamp(0, w)
    for r in range(B * L):
        c = int(own[r])
        keys = idx[r, :c]
        ok = (keys >= 0) & (keys < N)
        for name, v in (("key_N", N), ("key_minus_1", -1), ("key_int_max", BIG)):
            if bool((keys == v).any()):
                found.add(name)
        if c < w and not bool(((idx[r, c:] >= 0) & (idx[r, c:] < N)).all()):
            found.add("garbage_past_cnt")
        if c == w and bool(ok.all()):
            d = keys[1:] - keys[:-1]
            if bool((d > 0).all()):
                found.add("ascending")
            if bool((d < 0).all()):
                found.add("descending")
            if bool((d > 0).any()) and bool((d < 0).any()):
                found.add("random")
            if keys.unique().numel() < c:
                found.add("repeated")
    return found


def _required(width):
    need = {"cnt0", "cnt1", "cnt_width", "cnt_clamped", "cnt_negative", "empty_ends", "key_N", "key_minus_1", "key_int_max",
            "ascending", "descending"}
    if width > 1:                                     # (one slot: the whole row is owned or empty, and has no order)
        need |= {"garbage_past_cnt", "repeated"}
    if width > 2:
        need.add("random")
    return need


def _reference(idx, wgt, s, cnt, N):
    """The semantics of include/dagl_ce.h in plain torch -> (row_off, key, weight, score)."""
    B, L, w = idx.shape
    idx, wgt, s, cnt = idx.view(B * L, w), wgt.view(B * L, w), s.view(B * L, w), cnt.view(-1).long()
    owned = torch.arange(w)[None, :] < cnt.clamp(0, w)[:, None]
    valid = owned & (idx >= 0) & (idx < N)
    order = torch.where(valid, idx.long(), torch.full_like(idx, 1, dtype=torch.int64) << 40).argsort(dim=1, stable=True)
    deg = valid.sum(dim=1)
    take = torch.arange(w)[None, :] < deg[:, None]                                # the valid slots come first in a sorted row
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    return row_off, idx.gather(1, order)[take], wgt.gather(1, order)[take], s.gather(1, order)[take]


def _direct(shape, width, idx, wgt, s, cnt, extra=16):
    """The C entry on arrays of the test's own, SENTINEL-filled, with ``extra`` entries beyond the capacity the call is told of."""
    from dagl_amd import _lib
    lib = _lib.load()
    B, H, W, L, N = _geom(shape)
    cap = B * L * width
    need = lib.dagl_graph_from_lists_workspace_bytes(B, H, W)
    ws = torch.empty(need + 256, device=DEV, dtype=torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    row_off = torch.full((B * L + 1,), SENTINEL, device=DEV, dtype=torch.int64)
    key = torch.full((cap + extra,), SENTINEL, device=DEV, dtype=torch.int32)
    weight = torch.full((cap + extra,), float(SENTINEL), device=DEV)
    score = torch.full((cap + extra,), float(SENTINEL), device=DEV) if s is not None else None
    rc = lib.dagl_graph_from_lists(torch.cuda.current_stream().cuda_stream, B, H, W, width, idx.data_ptr(), wgt.data_ptr(),
                                   s.data_ptr() if s is not None else None, cnt.data_ptr(), row_off.data_ptr(), key.data_ptr(),
                                   weight.data_ptr(), score.data_ptr() if s is not None else None, cap, base, need)
    assert rc == 0, lib.dagl_last_error()
    torch.cuda.synchronize()
    return row_off.cpu(), key.cpu(), weight.cpu(), score.cpu() if s is not None else None


@pytest.mark.parametrize("with_scores", [True, False], ids=["scores", "no_scores"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_crafted_lists(shape, width, with_scores):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    found = set()
    for rot in _rotations(shape):
        found |= _kinds(*(_crafted(shape, width, rot)[i] for i in (0, 3)), N)
    assert found >= _required(width), sorted(_required(width) - found)
    if B > 1:
        cnt = _crafted(shape, width, 0)[3]
        assert int(cnt[0, L - 1]) <= 0 and int(cnt[1, 0]) <= 0        # empty rows on both sides of the image boundary
    for rot in _rotations(shape):
        idx, wgt, s, cnt = _crafted(shape, width, rot)
        want = _reference(idx, wgt, s, cnt, N)
        E = int(want[0][-1])
        assert want[1].numel() == E <= B * L * width
        d_idx, d_wgt, d_s, d_cnt = (t.to(DEV) for t in (idx, wgt, s, cnt))
        d_s = d_s if with_scores else None
        got = ops.graph_from_lists(d_idx, d_wgt, d_s, d_cnt, (H, W))
        assert got["row_off"].dtype == torch.int64 and got["key"].dtype == torch.int32 and got["weight"].dtype == torch.float32
        assert torch.equal(got["row_off"].cpu(), want[0]), (rot, "row_off")
        assert torch.equal(got["key"].cpu(), want[1].int()), (rot, "key")
        assert torch.equal(got["weight"].cpu(), want[2]), (rot, "weight")
        if with_scores:
            assert torch.equal(got["score"].cpu(), want[3]), (rot, "score")
        else:
            assert got["score"] is None
        # the same bits on a second call and through a Workspace
        ws = ops.Workspace()
        for again in (ops.graph_from_lists(d_idx, d_wgt, d_s, d_cnt, (H, W)), ops.graph_from_lists(d_idx, d_wgt, d_s, d_cnt, (H, W), workspace=ws),
                      ops.graph_from_lists(d_idx, d_wgt, d_s, d_cnt, (H, W), workspace=ws)):
            for name in ("row_off", "key", "weight") + (("score",) if with_scores else ()):
                assert torch.equal(again[name], got[name]), (rot, name)
        # the C entry on sentinel-filled arrays: entries [0, E) as above, everything from E on untouched
        row_off, key, weight, score = _direct(shape, width, d_idx, d_wgt, d_s, d_cnt)
        assert torch.equal(row_off, want[0]) and torch.equal(key[:E], want[1].int()) and torch.equal(weight[:E], want[2])
        assert bool((key[E:] == SENTINEL).all()) and bool((weight[E:] == SENTINEL).all())
        if with_scores:
            assert torch.equal(score[:E], want[3]) and bool((score[E:] == SENTINEL).all())


@pytest.mark.parametrize("width", [1, 64])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_all_empty_lists(shape, width):
    """Counts of 0 and below everywhere, valid keys in every slot: row_off == 0, E = 0, nothing written."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, N, (B, L, width), generator=g).int().to(DEV)
    wgt = torch.rand(B, L, width, generator=g).to(DEV)
    cnt = (-torch.randint(0, 3, (B, L), generator=g)).int().to(DEV)
    got = ops.graph_from_lists(idx, wgt, wgt, cnt, (H, W))
    assert bool((got["row_off"] == 0).all()) and got["row_off"].numel() == B * L + 1
    assert got["key"].numel() == 0 and got["weight"].numel() == 0 and got["score"].numel() == 0
    row_off, key, weight, score = _direct(shape, width, idx, wgt, wgt, cnt)
    assert bool((row_off == 0).all()) and bool((key == SENTINEL).all()) and bool((weight == SENTINEL).all()) and bool((score == SENTINEL).all())


def test_argument_checks():
    from dagl_amd import DaglError, ops
    B, H, W, L, N = _geom(SHAPES[1])
    idx, wgt, s, cnt = (t.to(DEV) for t in _crafted(SHAPES[1], 8, 0))
    for bad, word in ((lambda: ops.graph_from_lists(idx.long(), wgt, s, cnt, (H, W)), "dtype"),
                      (lambda: ops.graph_from_lists(idx, wgt.double(), s, cnt, (H, W)), "dtype"),
                      (lambda: ops.graph_from_lists(idx, wgt, s, cnt.long(), (H, W)), "dtype"),
                      (lambda: ops.graph_from_lists(idx.cpu(), wgt, s, cnt, (H, W)), "GPU"),
                      (lambda: ops.graph_from_lists(idx, wgt[:, :, :4], s, cnt, (H, W)), "contiguous"),
                      (lambda: ops.graph_from_lists(idx, wgt[:, :, :4].contiguous(), s, cnt, (H, W)), "nb_wgt"),
                      (lambda: ops.graph_from_lists(idx, wgt, s, cnt[:, :-1].contiguous(), (H, W)), "nb_cnt"),
                      (lambda: ops.graph_from_lists(idx, wgt, s, cnt, (H + 4, W)), "queries"),
                      (lambda: ops.graph_from_lists(idx.repeat(1, 1, 9)[:, :, :65].contiguous(), wgt.repeat(1, 1, 9)[:, :, :65].contiguous(),
                                                    None, cnt, (H, W)), "width")):
        with pytest.raises(DaglError) as err:
            bad()
        assert word in str(err.value), (word, str(err.value))
