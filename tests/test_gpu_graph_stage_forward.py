"""``ops.graph_stage_forward`` (dagl_graph_stage_forward, csrc/graph_forward.hip), ``ops.ces_stage_mix_backward``
(dagl_ces_stage_mix_backward, csrc/stage_mix_grad.hip) and ``ce._GraphStageForward``: a whole CES stage on its frozen graph.

The rows and the folded values come from existing kernels, so they are compared bit for bit with ``ops.graph_forward`` on the stacked
operands as those of 4 B images (an identity mix makes the output the pre-mix value: every product but one is an exact zero).  The mix
and its backward are new arithmetic: fp64 on the CPU is the reference, the bound the project's ``e_lib <= 3 e_32 + 1e-6`` normwise with
``e_32`` the same evaluation in fp32.

Shapes: (1,24,20) has L = 30, N = 480 and, at top-k 8, head boundaries at 240 h edges: rows straddle 128-edge segments and head
boundaries; (2,20,36) has B = 2, where head-major differs from batch-major; (1,9,6) has 54 pixels, less than one tile, and planes that
are not 16-byte aligned; (1,33,70) has odd sizes and several blocks."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import CASES, SCALE, _check, _geom, _graph, _inputs, _level_features, _padded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 24, 20), (2, 20, 36), (1, 9, 6), (1, 33, 70)]
KINDS = ["module-topk8", "module-adaptive", "crafted", "second-head-empty", "no-edges"]
HEAD_SEEDS = (21, 22, 23, 24)


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _cat_csr(parts):
    """ONE CSR over the head-major rows from the heads' (row_off, key): the offsets continue from head to head."""
    offs, base = [torch.zeros(1, dtype=torch.int64)], 0
    for off, _ in parts:
        offs.append(off[1:] + base)
        base += int(off[-1])
    return torch.cat(offs), torch.cat([k for _, k in parts]).int()


@functools.lru_cache(maxsize=None)
def _stage(shape, kind):
    """dict(wq4 [4,B,L,196], x4 [4,B,N,196], b2p4 [4,B,H+6,W+6,16], tau4 [4,B,L] | None, row_off [4 B L + 1], key [E]) on the GPU,
    built once per case and left unchanged."""
    B, H, W, L, N = _geom(shape)
    if kind.startswith("module"):
        from dagl_amd.ce import CE
        variant, gain, mode, k = CASES[5] if kind == "module-topk8" else CASES[1]
        x = _inputs(11, shape, variant, gain)[0].to(DEV)
        feats, graphs = [], []
        with torch.no_grad():
            for seed in HEAD_SEEDS:
                ce = CE(in_channels=64)
                ce.load_state_dict(_inputs(seed, shape, variant, gain)[1], strict=True)
                ce.select_mode = mode
                if mode != "adaptive":
                    ce.select_k = k
                ce = ce.to(DEV).eval()
                g = ce.graph(x).cpu()
                graphs.append((g.row_off, g.key))
                feats.append(ce._graph_features(x, mode != "topk", False, False))
        tau4 = torch.stack([f[2] for f in feats]).contiguous() if mode != "topk" else None
        wq4, x4, b2p4 = (torch.stack([f[i] for f in feats]).contiguous() for i in (0, 1, 3))
    else:
        graphs, wq, xk, tau, b2p = [], [], [], [], []
        for h in range(4):
            row_off, key, b2 = _graph(shape, seed=5 + h)
            if kind == "no-edges" or (kind == "second-head-empty" and h == 1):
                row_off, key = torch.zeros_like(row_off), key[:0]
            graphs.append((row_off, key))
            f = _level_features(*_graph(shape, seed=5 + h)[:2], shape, seed=7 + h)
            wq.append(f[0]); xk.append(f[1]); tau.append(f[2].view(B, L)); b2p.append(_padded(b2))
        wq4, x4, tau4, b2p4 = (torch.stack(t).contiguous().to(DEV) for t in (wq, xk, tau, b2p))
    row_off, key = _cat_csr(graphs)
    assert row_off.numel() == 4 * B * L + 1 and int(row_off[-1]) == key.numel()
    return dict(wq4=wq4, x4=x4, b2p4=b2p4, tau4=tau4, row_off=row_off.to(DEV), key=key.to(DEV))


def _flat(t):
    return t.flatten(0, 1) if t is not None else None


def _head_major(t, B):
    """[B, 64, H, W] -> [4 B, 16, H, W] head-major."""
    return t.view(B, 4, 16, *t.shape[2:]).transpose(0, 1).reshape(4 * B, 16, *t.shape[2:]).contiguous()


def _variants(st):
    """(tau4 | None, normalize) a case is run with: with and without the margin where it has one, both normalisations."""
    return [(tau, nz) for tau in ([st["tau4"], None] if st["tau4"] is not None else [None]) for nz in ("reference", "edges")]


def _identity(shape):
    B, H, W, L, N = _geom(shape)
    return torch.zeros(B, 64, H, W, device=DEV), torch.eye(64, device=DEV), torch.zeros(64, device=DEV)


@functools.lru_cache(maxsize=None)
def _mix(shape, seed=3):
    """(x [B,64,H,W], mix_w [64,64] uniform +-1/8, mix_b [64], d_out [B,64,H,W], cat4 [4,B,16,H,W]) on the CPU."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 64, H, W, generator=gen), (torch.rand(64, 64, generator=gen) - 0.5) / 4, (torch.rand(64, generator=gen) - 0.5) / 4,
            torch.randn(B, 64, H, W, generator=gen), torch.randn(4, B, 16, H, W, generator=gen))


# ---- 1. rows and folded values come from existing kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_rows_and_folded_values_are_graph_forward_s(shape, kind):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    st = _stage(shape, kind)
    if kind == "module-topk8":
        assert st["key"].numel() == 4 * B * L * 8 and st["tau4"] is None
    if kind == "no-edges":
        assert st["key"].numel() == 0
    zeros, eye, no_bias = _identity(shape)
    for tau4, normalize in _variants(st):
        out = ops.graph_stage_forward(st["wq4"], st["x4"], st["b2p4"], st["row_off"], st["key"], zeros, eye, no_bias, tau4=tau4, scale=SCALE,
                                      normalize=normalize)
        want = ops.graph_forward(_flat(st["wq4"]), _flat(st["x4"]), _flat(st["b2p4"]), st["row_off"], st["key"], _flat(tau4), scale=SCALE,
                                 normalize=normalize)
        assert out.shape == (B, 64, H, W) and want.shape == (4 * B, 16, H, W)
        assert torch.equal(_head_major(out, B), want), (tau4 is not None, normalize)
        assert bool(torch.isfinite(out).all()) and (kind == "no-edges") == (not bool(out.any()))
    if kind == "second-head-empty":
        assert not bool(_head_major(out, B)[B:2 * B].any()) and bool(_head_major(out, B)[:B].any())


# ---- 2. the mix ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["module-topk8", "crafted", "no-edges"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_mix(shape, kind):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    st = _stage(shape, kind)
    x, mix_w, mix_b = _mix(shape)[:3]
    dev = [t.to(DEV) for t in (x, mix_w, mix_b)]
    torch.set_num_threads(16)
    for tau4, normalize in _variants(st)[:2]:
        call = lambda: ops.graph_stage_forward(st["wq4"], st["x4"], st["b2p4"], st["row_off"], st["key"], *dev, tau4=tau4, scale=SCALE,
                                               normalize=normalize)
        out = call()
        rows = ops.graph_forward(_flat(st["wq4"]), _flat(st["x4"]), _flat(st["b2p4"]), st["row_off"], st["key"], _flat(tau4), scale=SCALE,
                                 normalize=normalize)
        cat = rows.view(4, B, 16, H, W).transpose(0, 1).reshape(B, 64, H, W).cpu()
        ref = lambda dt: F.conv2d(cat.to(dt), mix_w.to(dt).view(64, 64, 1, 1), mix_b.to(dt)) + x.to(dt)
        _check(f"stage forward mix {shape} {kind} tau {tau4 is not None} {normalize}", out, ref(torch.float64), ref(torch.float32))
        assert torch.equal(call(), out)
        if kind == "no-edges":
            assert torch.equal(out, dev[0] + dev[2].view(1, 64, 1, 1))
    # the 1x1 convolution's own layout of the weights
    assert torch.equal(ops.graph_stage_forward(st["wq4"], st["x4"], st["b2p4"], st["row_off"], st["key"], dev[0], dev[1].view(64, 64, 1, 1),
                                               dev[2], tau4=tau4, scale=SCALE, normalize=normalize), out)


# ---- 3. the training flavour --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_training_flavour(shape, kind):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    st = _stage(shape, kind)
    dev = [t.to(DEV) for t in _mix(shape)[:3]]
    for tau4, normalize in _variants(st):
        args = (st["wq4"], st["x4"], st["b2p4"], st["row_off"], st["key"], *dev)
        plain = ops.graph_stage_forward(*args, tau4=tau4, scale=SCALE, normalize=normalize)
        out, row_max, row_sum, cat4 = ops.graph_stage_forward(*args, tau4=tau4, scale=SCALE, normalize=normalize, train=True)
        assert torch.equal(out, plain)
        want, want_max, want_sum = ops.graph_forward_train(_flat(st["wq4"]), _flat(st["x4"]), _flat(st["b2p4"]), st["row_off"], st["key"],
                                                           _flat(tau4), scale=SCALE, normalize=normalize)
        assert row_max.dtype == torch.float32 and row_sum.dtype == torch.float64 and row_max.shape == row_sum.shape == (4 * B * L,)
        assert torch.equal(row_max, want_max) and torch.equal(row_sum, want_sum)
        assert cat4.shape == (4, B, 16, H, W) and torch.equal(cat4.view(4 * B, 16, H, W), want)


# ---- 4. the backward of the mix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_mix_backward(shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    _, mix_w, _, d_out, cat4 = _mix(shape)
    g_out, g_cat, g_w = d_out.to(DEV), cat4.to(DEV), mix_w.to(DEV)
    # an identity mix hands d_out through, regrouped
    d_cat4, d_w, d_b = ops.ces_stage_mix_backward(g_out, g_cat, torch.eye(64, device=DEV))
    assert d_cat4.shape == (4, B, 16, H, W) and d_w.shape == (64, 64) and d_b.shape == (64,)
    assert torch.equal(d_cat4.view(4 * B, 16, H, W), _head_major(g_out, B))
    # random weights against fp64 on the CPU
    d_cat4, d_w, d_b = ops.ces_stage_mix_backward(g_out, g_cat, g_w)
    torch.set_num_threads(16)

    def ref(dt):
        do, w = d_out.to(dt).view(B, 64, N), mix_w.to(dt)
        cat = cat4.to(dt).transpose(0, 1).reshape(B, 64, N)
        dc = torch.einsum("oc,bop->bcp", w, do).view(B, 4, 16, H, W).transpose(0, 1).contiguous()
        return dc, torch.einsum("bop,bcp->oc", do, cat), do.sum(dim=(0, 2))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    for name, lib, a, b in zip(("d_cat4", "d_mix_w", "d_mix_b"), (d_cat4, d_w, d_b), r64, r32):
        _check(f"mix backward {name} {shape}", lib, a, b)
    # the same bits on every call, with any subset of the parameter gradients, and through the convolution's layout of the weights
    again = ops.ces_stage_mix_backward(g_out, g_cat, g_w)
    assert all(torch.equal(a, b) for a, b in zip(again, (d_cat4, d_w, d_b)))
    only_w = ops.ces_stage_mix_backward(g_out, g_cat, g_w, need_b=False)
    only_b = ops.ces_stage_mix_backward(g_out, g_cat, g_w, need_w=False)
    neither = ops.ces_stage_mix_backward(g_out, g_cat, g_w, need_w=False, need_b=False)
    assert only_w[2] is None and only_b[1] is None and neither[1] is None and neither[2] is None
    assert torch.equal(only_w[1], d_w) and torch.equal(only_b[2], d_b)
    assert all(torch.equal(t[0], d_cat4) for t in (only_w, only_b, neither))
    assert torch.equal(ops.ces_stage_mix_backward(g_out, g_cat, g_w.view(64, 64, 1, 1))[1], d_w)


def test_mix_backward_block_split():
    """(2,96,96): 18432 pixels, five blocks of the weight-gradient launch -- the ranges of the second to fourth cross the image boundary
    or start inside the second image, the last one is short."""
    from dagl_amd import ops
    shape = (2, 96, 96)
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(4)
    d_out, cat4, mix_w = torch.randn(B, 64, H, W, generator=gen), torch.randn(4, B, 16, H, W, generator=gen), torch.eye(64)
    _, d_w, d_b = ops.ces_stage_mix_backward(d_out.to(DEV), cat4.to(DEV), mix_w.to(DEV))
    torch.set_num_threads(16)
    ref = lambda dt: (torch.einsum("bop,bcp->oc", d_out.to(dt).view(B, 64, N), cat4.to(dt).transpose(0, 1).reshape(B, 64, N)),
                      d_out.to(dt).sum(dim=(0, 2, 3)))
    for name, lib, a, b in zip(("d_mix_w", "d_mix_b"), (d_w, d_b), ref(torch.float64), ref(torch.float32)):
        _check(f"mix backward {name} {shape}", lib, a, b)


def test_mix_backward_operand_refusals():
    from dagl_amd import DaglError, ops
    shape = SHAPES[0]
    _, mix_w, _, d_out, cat4 = [t.to(DEV) for t in _mix(shape)]
    for bad, word in (((d_out, cat4[:3].contiguous(), mix_w), "cat4"), ((d_out, cat4[:, :, :8].contiguous(), mix_w), "cat4"),
                      ((d_out[:, :32].contiguous(), cat4, mix_w), "64"), ((d_out, cat4, mix_w[:32].contiguous()), "mix_w"),
                      ((d_out.cpu(), cat4, mix_w), "GPU"), ((d_out, cat4.double(), mix_w), "dtype"), ((d_out, cat4, mix_w.t()), "contiguous")):
        with pytest.raises(DaglError, match=word):
            ops.ces_stage_mix_backward(*bad)


# ---- 5. the whole backward, library level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["module-adaptive", "crafted", "second-head-empty"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=_id)
def test_the_op_s_graph_gradients_are_graph_forward_backward_s(shape, kind):
    from dagl_amd import PatchGraph, ops
    from dagl_amd.ce import _GraphStageForward
    B, H, W, L, N = _geom(shape)
    st = _stage(shape, kind)
    graph = PatchGraph(st["row_off"], st["key"], torch.zeros(st["key"].numel(), device=DEV), None, 4 * B, H, W)
    zeros, eye, no_bias = _identity(shape)
    d_out = _mix(shape)[3].to(DEV)
    ws = [ops.Workspace() for _ in range(3)]
    for tau4, normalize in _variants(st)[:2]:
        leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (st["wq4"], st["x4"], tau4, st["b2p4"])]
        xg = zeros.clone().requires_grad_(True)
        out = _GraphStageForward.apply(*leaves, xg, eye, no_bias, graph, SCALE, normalize, *ws)
        plain = ops.graph_stage_forward(st["wq4"], st["x4"], st["b2p4"], st["row_off"], st["key"], zeros, eye, no_bias, tau4=tau4, scale=SCALE,
                                        normalize=normalize)
        assert out.requires_grad and torch.equal(out.detach(), plain)
        out.backward(d_out)
        _, row_max, row_sum = ops.graph_forward_train(_flat(st["wq4"]), _flat(st["x4"]), _flat(st["b2p4"]), st["row_off"], st["key"], _flat(tau4),
                                                      scale=SCALE, normalize=normalize)
        want = ops.graph_forward_backward(_head_major(d_out, B), _flat(st["wq4"]), _flat(st["x4"]), _flat(st["b2p4"]), st["row_off"], st["key"],
                                          row_max, row_sum, _flat(tau4), scale=SCALE, normalize=normalize, transposed=graph.transpose())
        for name, leaf, w in zip(("d_wq", "d_x", "d_tau", "d_b2p"), leaves, want):
            if leaf is None:
                assert w is None
                continue
            assert leaf.grad is not None and leaf.grad.shape == leaf.shape and torch.equal(leaf.grad.flatten(0, 1), w.view(leaf.grad.flatten(0, 1).shape)), name
        assert torch.equal(xg.grad, d_out)                                        # the residual input
    # needs_input_grad decides which products run: the value map alone
    b2p = st["b2p4"].clone().requires_grad_(True)
    out = _GraphStageForward.apply(st["wq4"], st["x4"], tau4, b2p, zeros, eye, no_bias, graph, SCALE, normalize, *ws)
    out.backward(d_out)
    assert torch.equal(b2p.grad.flatten(0, 1), want[3])


def test_operand_refusals():
    from dagl_amd import DaglError, ops
    shape = SHAPES[1]
    st = _stage(shape, "crafted")
    x, mix_w, mix_b = [t.to(DEV) for t in _mix(shape)[:3]]
    ok = dict(wq4=st["wq4"], x4=st["x4"], b2p4=st["b2p4"], row_off=st["row_off"], key=st["key"], x=x, mix_w=mix_w, mix_b=mix_b)
    for change, word in ((dict(wq4=st["wq4"][:3].contiguous()), "wq4"), (dict(x4=st["x4"][:, :1].contiguous()), "x4"),
                         (dict(b2p4=st["b2p4"][:, :1].contiguous()), "b2p"), (dict(row_off=st["row_off"][:-1].contiguous()), "row_off"),
                         (dict(x=x[:, :32].contiguous()), "64"), (dict(mix_w=mix_w[:32].contiguous()), "mix_w"), (dict(wq4=st["wq4"].cpu()), "GPU"),
                         (dict(key=st["key"].long()), "dtype")):
        with pytest.raises(DaglError, match=word):
            ops.graph_stage_forward(**{**ok, **change}, scale=SCALE)
    with pytest.raises(DaglError, match="tau"):
        ops.graph_stage_forward(**ok, tau4=st["tau4"][:, :, :-1].contiguous(), scale=SCALE)
    with pytest.raises(DaglError, match="normalize"):
        ops.graph_stage_forward(**ok, scale=SCALE, normalize="rows")
