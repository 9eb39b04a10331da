"""``ops.graph_stage_step`` (dagl_graph_stage_step, csrc/graph_refresh.hip): ``ops.graph_step`` for the four heads of a CES stage -- one CSR
over the head-major rows, features and value maps that stay per head -- and the stage's fold + mix on the result.

The graph of every head is held EXACTLY against ``ops.graph_step`` on that head's operands and its slice of the input graph (whose own
tests hold it against the CPU selection and fp64); the output against the CPU mix of those calls' outputs under the project's rule
``e <= 3 e_ref32 + 1e-6``; and it must carry the same bits with and without the graph outputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import _check, _geom, _padded
from tests.graph_step_reference import MAX_ROW, R_LONG, SHAPES, crafted, features, value_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARRAYS = ("row_off", "key", "weight", "score")
HEAD_SEEDS = [(5, 7, 9), (6, 8, 10), (15, 17, 19), (25, 27, 29)]          # (graph, features, value map) of head h


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _stage(shape):
    """The four heads' operands on the device and the stage's CSR: head h's crafted graph (its rows 0 .. 9 are the crafted ones, so
    the first row of every head is empty and follows a non-empty last row), banded features and value map, each from a seed of its own."""
    B, H, W, L, N = _geom(shape)
    heads = []
    for gs, fs, vs in HEAD_SEEDS:
        row_off, key = crafted(shape, gs)
        wq, x, tau = features(shape, fs)
        heads.append(dict(row_off=row_off.to(DEV), key=key.to(DEV), wq=wq.to(DEV), x=x.to(DEV), tau=tau.to(DEV),
                          b2p=_padded(value_map(shape, vs)).to(DEV)))
    base, offs = 0, [torch.zeros(1, dtype=torch.int64)]
    for gs, _, _ in HEAD_SEEDS:
        row_off = crafted(shape, gs)[0]
        offs.append(row_off[1:] + base)
        base += int(row_off[-1])
    gen = torch.Generator().manual_seed(41)
    mix = dict(x=torch.randn(B, 64, H, W, generator=gen), mix_w=(torch.rand(64, 64, generator=gen) - 0.5) / 4,
               mix_b=(torch.rand(64, generator=gen) - 0.5) / 4)
    return heads, torch.cat(offs).to(DEV), torch.cat([h["key"] for h in heads]), mix


def _stage_call(shape, **kw):
    from dagl_amd import ops
    heads, row_off, key, mix = _stage(shape)
    with_tau = kw.pop("with_tau", False)
    return ops.graph_stage_step([h["wq"] for h in heads], [h["x"] for h in heads], [h["b2p"] for h in heads], row_off, key,
                                mix["x"].to(DEV), mix["mix_w"].to(DEV), mix["mix_b"].to(DEV),
                                tau4=[h["tau"] for h in heads] if with_tau else None, **kw)


def _head_calls(shape, with_tau=False, **kw):
    from dagl_amd import ops
    return [ops.graph_step(h["wq"], h["x"], h["b2p"], h["row_off"], h["key"], tau=h["tau"] if with_tau else None, **kw)
            for h in _stage(shape)[0]]


def _mix_references(outs, mix):
    """(fp64, fp32) ``conv1x1(cat(outs)) + mix_b + x`` on the CPU."""
    torch.set_num_threads(16)
    refs = []
    for dtype in (torch.float64, torch.float32):
        cat = torch.cat([o.cpu().to(dtype) for o in outs], dim=1)
        refs.append(F.conv2d(cat, mix["mix_w"].to(dtype).view(64, 64, 1, 1), mix["mix_b"].to(dtype)) + mix["x"].to(dtype))
    return refs


@pytest.mark.parametrize("k", [0, 8])
@pytest.mark.parametrize("with_tau", [False, True], ids=["no_tau", "tau"])
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_against_graph_step_head_by_head(shape, radius, with_tau, k):
    """Declared ``max_row_edges`` 12: radius 0 / 1 run a wavefront per row, radius 2 a block."""
    B, H, W, L, N = _geom(shape)
    heads, row_off, key, mix = _stage(shape)
    kw = dict(radius=radius, k=k, with_tau=with_tau, max_row_edges=MAX_ROW)
    what = f"{shape} radius {radius} tau {with_tau} k {k}"
    out, csr, status = _stage_call(shape, **kw)
    per_head = _head_calls(shape, **kw)
    assert out.shape == (B, 64, H, W) and out.dtype == torch.float32 and status.tolist()[0] == 0
    assert status.tolist()[1] == max(st.tolist()[1] for _, _, st in per_head)
    # 1. head h's rows: ops.graph_step's on its slice, bit for bit, the offsets continuing from head to head
    n = B * L
    off = csr["row_off"]
    assert off.numel() == 4 * n + 1 and int(off[0]) == 0 and int(off[-1]) == csr["key"].numel()
    bounds = off[::n].tolist()
    for h, (_, want, _) in enumerate(per_head):
        assert torch.equal(off[h * n:(h + 1) * n + 1] - off[h * n], want["row_off"]), (what, h)
        for name in ARRAYS[1:]:
            assert torch.equal(csr[name][bounds[h]:bounds[h + 1]], want[name]), (what, h, name)
    assert int(off[1]) == 0 and int(off[n + 1] - off[n]) == 0                           # the empty first rows, also at a seam
    # 2. the output: the CPU mix of the heads' graph_step outputs
    ref64, ref32 = _mix_references([o for o, _, _ in per_head], mix)
    _check(f"stage step out {what}", out, ref64, ref32)
    # 3. the same bits without the graph, a block per row, and again
    for again in (dict(want_graph=False), dict(block_rows=True), dict(want_graph=False, block_rows=True), dict()):
        o, g2, st = _stage_call(shape, **{**kw, **again})
        assert torch.equal(o, out), (what, sorted(again))
        assert st.tolist() == status.tolist()
        if again.get("want_graph", True):
            assert all(torch.equal(g2[name], csr[name]) for name in ARRAYS), (what, sorted(again))
        else:
            assert g2 is None


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_empty_graph_gives_bias_plus_input(shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    heads, _, _, mix = _stage(shape)
    x, mix_w, mix_b = (mix[n].to(DEV) for n in ("x", "mix_w", "mix_b"))
    row_off = torch.zeros(4 * B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    for kw in (dict(), dict(tau4=[h["tau"] for h in heads], k=8), dict(keep_all=True, radius=2)):
        for want_graph in (True, False):
            out, csr, status = ops.graph_stage_step([h["wq"] for h in heads], [h["x"] for h in heads], [h["b2p"] for h in heads], row_off,
                                                    key, x, mix_w, mix_b, max_row_edges=0, want_graph=want_graph, **kw)
            assert torch.equal(out, mix_b.view(1, 64, 1, 1) + x) and status.tolist() == [0, 0]
            if want_graph:
                assert csr["key"].shape == csr["weight"].shape == csr["score"].shape == (0,)
                assert csr["row_off"].shape == (4 * B * L + 1,) and not bool(csr["row_off"].any())
            else:
                assert csr is None


@pytest.mark.parametrize("radius", [1, 2])
def test_overlong_rows_are_counted_not_truncated(radius):
    """``max_row_edges`` declared one below the truth: every head holds one such row.  With the graph the call raises ``ERR_UNSUPPORTED``
    naming the count; without it the four rows contribute zeros and ``status[0]`` counts them, as ``ops.graph_step`` does per head."""
    from dagl_amd import _lib
    shape = SHAPES[0]
    heads = _stage(shape)[0]
    assert all(int(h["row_off"][R_LONG + 1] - h["row_off"][R_LONG]) == MAX_ROW for h in heads)
    with pytest.raises(_lib.DaglError, match="4 row") as e:
        _stage_call(shape, radius=radius, k=8, max_row_edges=MAX_ROW - 1)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "graph_stage_step" in str(e.value)
    out, csr, status = _stage_call(shape, radius=radius, k=8, max_row_edges=MAX_ROW - 1, want_graph=False)
    assert csr is None and status.tolist()[0] == 4
    per_head = _head_calls(shape, radius=radius, k=8, max_row_edges=MAX_ROW - 1, want_graph=False)
    assert all(st.tolist()[0] == 1 for _, _, st in per_head)
    _check(f"stage step out, overlong rows left out, radius {radius}", out, *_mix_references([o for o, _, _ in per_head], _stage(shape)[3]))
    full, _, status = _stage_call(shape, radius=radius, k=8, max_row_edges=MAX_ROW, want_graph=False)
    assert status.tolist()[0] == 0 and not torch.equal(full, out)


def test_operand_refusals():
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    heads, row_off, key, mix = _stage(shape)
    x, mix_w, mix_b = (mix[n].to(DEV) for n in ("x", "mix_w", "mix_b"))
    wq4, x4, b4, tau4 = ([h[n] for h in heads] for n in ("wq", "x", "b2p", "tau"))
    ok = dict(max_row_edges=MAX_ROW)

    def swap(seq, value, h=2):
        return seq[:h] + [value] + seq[h + 1:]
    for args, kw, word in (((wq4, x4, swap(b4, b4[2][:, :-1].contiguous()), row_off, key, x, mix_w, mix_b), ok, "value map"),
                           ((wq4, x4, swap(b4, b4[2][:1]), row_off, key, x, mix_w, mix_b), ok, "value map"),
                           ((wq4[:3], x4, b4, row_off, key, x, mix_w, mix_b), ok, "four"),
                           ((swap(wq4, wq4[2][:1]), x4, b4, row_off, key, x, mix_w, mix_b), ok, "wq_rows"),
                           ((wq4, x4, b4, row_off[:-1], key, x, mix_w, mix_b), ok, "row_off"),
                           ((wq4, x4, b4, row_off, key, x[:, :32].contiguous(), mix_w, mix_b), ok, "64"),
                           ((wq4, x4, b4, row_off, key, x, mix_w[:, :32].contiguous(), mix_b), ok, "mix_w"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, tau4=swap(tau4, tau4[2][:-1])), "tau"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, tau4=tau4[:2]), "four"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, scale=0.0), "scale"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, normalize="rows"), "normalize"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, radius=9), "radius"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(ok, k=-1), "k=-1"),
                           ((wq4, x4, b4, row_off, key, x, mix_w, mix_b), dict(want_graph=False), "max_row_edges")):
        with pytest.raises(_lib.DaglError, match=word):
            ops.graph_stage_step(*args, **kw)
    with pytest.raises(_lib.DaglError, match="candidates") as e:
        ops.graph_stage_step(wq4, x4, b4, row_off, key, x, mix_w, mix_b, radius=8, max_row_edges=MAX_ROW)        # 12 x 289
    assert e.value.code == _lib.ERR_UNSUPPORTED

    def captured(**kw):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ops.graph_stage_step(wq4, x4, b4, row_off, key, x, mix_w, mix_b, **kw)
    with pytest.raises(_lib.DaglError, match="captur"):
        captured(max_row_edges=MAX_ROW)
    with pytest.raises(_lib.DaglError, match="captur"):
        captured(want_graph=False)
    torch.cuda.synchronize()
