"""``CE.apply_graph`` / ``ops.graph_apply`` / ``ops.graph_apply_backward`` (dagl_graph_apply*, csrc/graph_apply.hip): a block run on
a given patch graph, ``out = fold(A_G . V(theta(x))) / cnt``.

The reference everywhere is torch on the CPU in fp64: the dense ``A_G`` built with ``index_put_(accumulate=True)`` (repeated keys add
up), times ``oracle.ce_oracle.patch_rows(b2, 7, 1)``, folded as ``_fold`` of graph_reference.py does.  Kernel-level bound (the
project's pattern, graph_reference.py ``check_values``): ``e_lib <= 3 e_32 + 1e-6``, both normwise against fp64, ``e_32`` the same
formula evaluated by torch on the CPU in fp32."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import (CASES, SHAPES, _crafted, _dense_apply, _gap, _geom, _id, _inputs, _module, _oracle, _padded, _refused,
                                  _seed)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _crafted_reference(shape):
    row_off, key, weight, b2 = _crafted(shape)
    torch.set_num_threads(16)
    with torch.no_grad():
        return _dense_apply(row_off, key, weight, b2.double(), shape), _dense_apply(row_off, key, weight, b2, shape)


def _check(what, lib, ref64, ref32):
    e_lib = normwise(lib.double().cpu().numpy(), ref64.numpy())
    e_32 = normwise(ref32.double().numpy(), ref64.numpy())
    print(f"[graph_apply] {what}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, ratio {e_lib / max(e_32, 1e-30):.2f}")
    assert e_lib <= 3.0 * e_32 + 1e-6, (what, e_lib, e_32)


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]], ids=_id)
def test_kernel_against_fp64_on_crafted_graphs(shape):
    """Tests 1 and 2: ``ops.graph_apply`` on a random value map (no convolution in the way), and the same bits on a second call."""
    from dagl_amd import ops
    row_off, key, weight, b2 = _crafted(shape)
    ref64, ref32 = _crafted_reference(shape)
    args = [t.to(DEV) for t in (_padded(b2), row_off, key, weight)]
    out = ops.graph_apply(*args)
    assert out.shape == ref64.shape and out.dtype == torch.float32
    _check(f"crafted {shape}, {key.numel()} edges", out, ref64, ref32)
    ws = ops.Workspace()
    again = ops.graph_apply(*args, workspace=ws)
    assert torch.equal(out, again) and torch.equal(again, ops.graph_apply(*args, workspace=ws))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]], ids=_id)
def test_empty_graph(shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    b2p = torch.randn(B, H + 6, W + 6, 16, device=DEV)
    out = ops.graph_apply(b2p, torch.zeros(B * L + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                          torch.empty(0, device=DEV))
    assert out.shape == (B, 16, H, W) and bool((out == 0).all())
    d_b2p, d_w = ops.graph_apply_backward(torch.randn(B, 16, H, W, device=DEV), b2p, torch.zeros(B * L + 1, dtype=torch.int64, device=DEV),
                                          torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, device=DEV),
                                          transposed=(torch.zeros(B * N + 1, dtype=torch.int64, device=DEV),
                                                      torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)))
    assert d_w.numel() == 0 and d_b2p.shape == b2p.shape and bool((d_b2p == 0).all())


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5], CASES[7], CASES[9]], ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_round_trip(shape, case):
    """Test 3: ``apply_graph(x, graph(x))`` is ``forward(x)`` -- scan = "exact" and the default scan -- within the bound
    ``test_graph_reproduces_the_block`` applies to the same pair of quantities."""
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    B, H, W = shape
    ce, x = _module(seed, shape, variant, gain, mode, k)
    with torch.no_grad():
        got = ce.apply_graph(x, ce.graph(x))
    assert got.shape == (B, 16, H, W) and got.dtype == torch.float32
    gap = _gap(_oracle(seed, shape, variant, gain, mode, k), mode, k, H, W)
    bound = 1e-4 if gap >= 1e-6 else 1e-3
    for scan in ("screened", "exact"):
        ce.scan = scan
        ce.invalidate_packed()
        with torch.no_grad():
            out = ce(x)
        err = normwise(got.double().cpu().numpy(), out.double().cpu().numpy())
        print(f"[graph_apply] seed {seed} {shape} {case} scan={scan}: apply_graph(graph) vs forward {err:.2e} (bound {bound:.0e}, gap {gap:.1e})")
        assert err <= bound, (scan, err)


def test_editing():
    """Test 4: drop the lighter half of a top-k 100 graph's edges, double the rest: the fp64 dense evaluation of the EDITED graph on the
    oracle's value map (bound of the round trip: the value map is the module's own product); all-zero weights give exactly zero."""
    shape, case = SHAPES[3], CASES[7]
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    ce, x = _module(seed, shape, variant, gain, mode, k)
    g = ce.graph(x)
    t = g.weight.median()
    edited = g.select(g.weight >= t)
    edited = edited.with_weight(2 * edited.weight)
    assert 0 < edited.n_edges < g.n_edges
    with torch.no_grad():
        got = ce.apply_graph(x, edited)
        zero = ce.apply_graph(x, g.with_weight(0 * g.weight))
    st = _oracle(seed, shape, variant, gain, mode, k)
    want = _dense_apply(edited.row_off.cpu(), edited.key.cpu(), edited.weight.cpu().double(), st["b2"], shape)
    err = normwise(got.double().cpu().numpy(), want.numpy())
    print(f"[graph_apply] edited graph ({edited.n_edges} of {g.n_edges} edges): {err:.2e}")
    assert err <= 1e-4
    assert bool((zero == 0).all())


@functools.lru_cache(maxsize=None)
def _grad_reference(shape, dtype):
    row_off, key, weight, b2 = _crafted(shape)
    gen = torch.Generator().manual_seed(9)
    d_out = torch.randn(shape[0], 16, shape[1], shape[2], generator=gen)
    w = weight.to(dtype).clone().requires_grad_(True)
    v = b2.to(dtype).clone().requires_grad_(True)
    torch.set_num_threads(16)
    (_dense_apply(row_off, key, w, v, shape) * d_out.to(dtype)).sum().backward()
    return d_out, w.grad, v.grad


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=_id)
def test_kernel_gradients(shape):
    """Test 5, first half: ``ops.graph_apply_backward`` against fp64 autograd of the dense formula, on the crafted long-tailed graph."""
    from dagl_amd import ops
    from dagl_amd.graph import PatchGraph
    B, H, W, L, N = _geom(shape)
    row_off, key, weight, b2 = _crafted(shape)
    d_out, dw64, dv64 = _grad_reference(shape, torch.float64)
    _, dw32, dv32 = _grad_reference(shape, torch.float32)
    g = PatchGraph(row_off, key, weight, None, B, H, W).to(DEV)
    args = (d_out.to(DEV), _padded(b2).to(DEV), g.row_off, g.key, g.weight)
    d_b2p, d_w = ops.graph_apply_backward(*args, transposed=g.transpose())
    d_b2 = d_b2p[:, 3:3 + H, 3:3 + W, :].permute(0, 3, 1, 2)
    _check(f"d_weight {shape}", d_w, dw64, dw32)
    _check(f"d_b2 {shape}", d_b2, dv64, dv32)
    again = ops.graph_apply_backward(*args, transposed=g.transpose())
    assert torch.equal(again[0], d_b2p) and torch.equal(again[1], d_w)
    only_w = ops.graph_apply_backward(*args, need_b2p=False)
    assert only_w[0] is None and torch.equal(only_w[1], d_w)
    only_v = ops.graph_apply_backward(*args, transposed=g.transpose(), need_weight=False)
    assert only_v[1] is None and torch.equal(only_v[0], d_b2p)


def _through_theta(x, th_w, th_b, row_off, key, weight, shape):
    return _dense_apply(row_off, key, weight, F.conv2d(x, th_w, th_b), shape)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=_id)
def test_module_gradients(shape):
    """Test 5, second half: ``CE.apply_graph`` under autograd -- d x, d theta.weight, d theta.bias, d graph.weight against fp64 autograd
    of ``fold(A_G . V(conv1x1(x))) / cnt``; g, the fc layers and the heads get no gradient."""
    from dagl_amd.graph import PatchGraph
    B, H, W, L, N = _geom(shape)
    row_off, key, weight, _ = _crafted(shape)
    ce, x = _module(11, shape, "default", 2.0, "topk", 8)
    d_out = torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(9))
    refs = []
    for dt in (torch.float64, torch.float32):
        leaves = [t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (x, ce.theta.weight, ce.theta.bias, weight)]
        (_through_theta(*leaves[:3], row_off, key, leaves[3], shape) * d_out.to(dt)).sum().backward()
        refs.append([t.grad for t in leaves])
    g = PatchGraph(row_off, key, weight, None, B, H, W).to(DEV)
    w = g.weight.detach().clone().requires_grad_(True)
    xg = x.detach().clone().requires_grad_(True)
    out = ce.apply_graph(xg, g.with_weight(w))
    assert out.requires_grad
    (out * d_out.to(DEV)).sum().backward()
    for name, lib, r64, r32 in zip(("d x", "d theta.weight", "d theta.bias", "d graph.weight"),
                                   (xg.grad, ce.theta.weight.grad, ce.theta.bias.grad, w.grad), *refs):
        assert lib is not None, name
        _check(f"{name} {shape}", lib, r64, r32)
    for name, p in ce.named_parameters():
        if not name.startswith("theta."):
            assert p.grad is None, name
    # the weights alone: nothing flows into the module or the input
    ce.zero_grad(set_to_none=True)
    for p in ce.parameters():
        p.requires_grad_(False)
    w2 = g.weight.detach().clone().requires_grad_(True)
    (ce.apply_graph(x, g.with_weight(w2)) * d_out.to(DEV)).sum().backward()
    assert torch.equal(w2.grad, w.grad) and all(p.grad is None for p in ce.parameters())


@pytest.mark.parametrize("kind", ["in_channels_32", "half_module"])
def test_other_widths_and_precisions(kind):
    """Test 6: a 32-channel module, and a .half() module with a half input (computed on the fp32 copies, returned as half), against the
    fp64 dense evaluation of the exported graph on ``conv1x1`` of the values the module sees.  Bound: the kernel bound
    ``3 e_32 + 1e-6``; the half output adds its own rounding, at most 2^-11 of the largest element."""
    shape, (variant, gain, mode, k) = SHAPES[0], ("sparse", 1.2, "adaptive", 0)
    cin, half = (32, False) if kind == "in_channels_32" else (64, True)
    ce, x = _module(12, shape, variant, gain, mode, k, in_channels=cin, half=half)
    g = ce.graph(x)
    with torch.no_grad():
        got = ce.apply_graph(x, g)
    assert got.dtype == x.dtype and got.shape == (shape[0], 16, shape[1], shape[2])
    x0, prm = _inputs(12, shape, variant, gain, cin)
    th_w, th_b = prm["theta.weight"], prm["theta.bias"]
    if half:
        x0, th_w, th_b = x0.half().float(), th_w.half().float(), th_b.half().float()
    gc = g.cpu()
    with torch.no_grad():
        ref64 = _through_theta(x0.double(), th_w.double(), th_b.double(), gc.row_off, gc.key, gc.weight, shape)
        ref32 = _through_theta(x0, th_w, th_b, gc.row_off, gc.key, gc.weight, shape)
    e_lib = normwise(got.double().cpu().numpy(), ref64.numpy())
    e_32 = normwise(ref32.double().numpy(), ref64.numpy())
    bound = 3.0 * e_32 + 1e-6 + (2.0 ** -11 if half else 0.0)
    print(f"[graph_apply] {kind}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, bound {bound:.2e}")
    assert e_lib <= bound


def test_refusals_leave_the_module_alone():
    """Test 7: every refusal is a ``DaglError`` raised before anything is launched; the state dict and the forward's packed weights
    stay as they were (the forward returns the same bits before and after)."""
    from dagl_amd.graph import PatchGraph
    shape, (variant, gain, mode, k) = SHAPES[3], CASES[5]
    ce, x = _module(11, shape, variant, gain, mode, k)
    g = ce.graph(x)
    B, H, W, L, N = _geom(shape)

    def empty(b, h, w, dev=DEV):
        l = (-(-h // 4)) * (-(-w // 4))
        return PatchGraph(torch.zeros(b * l + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                          torch.empty(0, device=dev), None, b, h, w)
    for other in ((B, H, W + 4), (B, H - 4, W), (B + 1, H, W)):
        _refused(ce, x, lambda: ce.apply_graph(x, empty(*other)), "the graph was built for")
    _refused(ce, x, lambda: ce.apply_graph(x, g.cpu()), "lives on cpu")
    _refused(ce, x, lambda: ce.apply_graph(x, "graph"), "PatchGraph expected")
    # a key = N: refused by validate(), on every call
    key = g.key.clone()
    key[5] = N
    bad = PatchGraph(g.row_off, key, g.weight, None, B, H, W)
    for _ in range(2):
        assert "key 4096" in _refused(ce, x, lambda: ce.apply_graph(x, bad), "edge 5")
    # an unvalidated graph while the stream is being captured: validate() would read a word on the host
    fresh = PatchGraph(g.row_off, g.key, g.weight, None, B, H, W)

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ce.apply_graph(x, fresh)
    _refused(ce, x, captured, "captur")
    torch.cuda.synchronize()
    assert not fresh._valid
    with torch.no_grad():
        assert torch.equal(ce.apply_graph(x, fresh), ce.apply_graph(x, g))       # and it still works afterwards


def test_refusal_of_a_generic_geometry():
    from dagl_amd.ce import CE
    from dagl_amd.graph import PatchGraph
    torch.manual_seed(5)
    ce = CE(ksize=5, stride_1=2, stride_2=1, inter_channels=16, in_channels=64).to(DEV).eval()
    x = torch.randn(1, 64, 20, 24, device=DEV)
    g = PatchGraph(torch.zeros(5 * 6 + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                   torch.empty(0, device=DEV), None, 1, 20, 24)
    _refused(ce, x, lambda: ce.apply_graph(x, g), "scope")


def test_capture():
    """Test 8: a validated graph applied inside ``torch.cuda.graph`` (one stream, no parallel branches) replays to the eager result."""
    shape, (variant, gain, mode, k) = SHAPES[3], CASES[5]
    ce, x = _module(11, shape, variant, gain, mode, k)
    g = ce.graph(x).validate()
    with torch.no_grad():
        eager = ce.apply_graph(x, g).clone()          # (also brings the module's workspace to its size before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ce.apply_graph(x, g)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
