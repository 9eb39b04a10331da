"""Training on frozen patch graphs: ``CE.forward_on_graph(backward="fused")`` (``_GraphForward``: ``ops.graph_forward_train`` +
``ops.graph_forward_backward``), ``CES.forward_on_graphs`` and ``RR.forward_on_graphs``.

References are torch on the CPU in fp64: autograd of the dense formula with the structure as a mask (``_dense_on_structure``), for the
``CES`` the module's own wiring with that formula in the place of each head.  Bound (the module-level one of the two ops' tests):
``e_lib <= 3 e_32 + 1e-4`` normwise, ``e_32`` the same evaluation in fp32 against fp64."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import CASES, _GRAD_NAMES, _band, _check, _dense_on_structure, _geom, _id, _inputs, _module, _oracle, _refused
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MSHAPES = [(1, 48, 48), (2, 20, 36)]
MCASES = [CASES[5], CASES[1]]                                                                       # top-k 8, adaptive
SEED = 11
CES_SHAPE = (1, 24, 20)
_HEAD_NAMES = ("g.weight", "g.bias", "theta.weight", "theta.bias", "fc1.0.weight", "fc1.0.bias", "fc2.0.weight", "fc2.0.bias")


def _member(g):
    """[B, L, N] bool on the CPU from a PatchGraph on the CPU."""
    m = torch.zeros(g.B * g.L, g.N, dtype=torch.bool)
    m[g.rows(), g.key.long()] = True
    return m.view(g.B, g.L, g.N)


@functools.lru_cache(maxsize=None)
def _structure(shape, case):
    """The structure of the case on the CPU: the module's own export without the edges inside the threshold band of the fp64 oracle --
    an edge whose margin is zero to rounding is on in one evaluation and off in another, which is a property of the input, not of a
    backward.  (A given structure may be any structure.)"""
    variant, gain, mode, k = case
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x).cpu()
    band = _band(_oracle(SEED, shape, variant, gain, mode, k), g, mode, k)
    print(f"[train_on_graph] {shape} {case}: {g.n_edges} edges, {int(band.sum())} in the threshold band (left out)")
    g = g.select(~band)
    assert g.n_edges > 0
    return g


@functools.lru_cache(maxsize=None)
def _module_reference(shape, case):
    """(d_out, names, [fp64 gradients], [fp32 gradients]) of x and the parameters, computed once per case and shared (read-only)."""
    variant, gain, mode, k = case
    B, H, W, L, N = _geom(shape)
    member = _member(_structure(shape, case))
    margin = mode != "topk"
    d_out = torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(9))
    x0, prm = _inputs(SEED, shape, variant, gain)
    names = [n for n in _GRAD_NAMES if margin or not n.startswith(("thr_conv", "bias_conv"))]
    refs = []
    torch.set_num_threads(16)
    for dt in (torch.float64, torch.float32):
        xl = x0.to(dt).clone().requires_grad_(True)
        pl = {n: t.to(dt).clone().requires_grad_(True) for n, t in prm.items()}
        (_dense_on_structure(xl, pl, member, margin, shape) * d_out.to(dt)).sum().backward()
        refs.append([xl.grad] + [pl[n].grad for n in names])
    return d_out, names, refs[0], refs[1]


@pytest.mark.parametrize("features", ["fp32", "split16"])
@pytest.mark.parametrize("case", MCASES, ids=_id)
@pytest.mark.parametrize("shape", MSHAPES, ids=_id)
def test_module_gradients(shape, case, features):
    """Test E: ``forward_on_graph(backward="fused")`` under autograd -- the output carries the bits of the ``no_grad`` fused call, d x and
    the gradient of every parameter of g, theta, fc1, fc2 and (with the margin) thr_conv, bias_conv against fp64 autograd of the dense
    formula on the same structure."""
    variant, gain, mode, k = case
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = _structure(shape, case).to(DEV)
    d_out, names, ref64, ref32 = _module_reference(shape, case)
    with torch.no_grad():
        want = ce.forward_on_graph(x, g, features=features, fused=True)
    xg = x.detach().clone().requires_grad_(True)
    out = ce.forward_on_graph(xg, g, features=features, backward="fused")
    assert out.requires_grad and torch.equal(out.detach(), want)
    (out * d_out.to(DEV)).sum().backward()
    own = dict(ce.named_parameters())
    for name, lib, r64, r32 in zip(["x"] + names, [xg.grad] + [own[n].grad for n in names], ref64, ref32):
        assert lib is not None and r64 is not None, name
        _check(f"d {name} {shape} {case} {features}", lib, r64, r32, slack=1e-4)
    for n, p in own.items():
        if n not in names:
            assert p.grad is None, n                                  # W; in "topk" the two heads
    # fused=True is accepted with the fused backward, and gives the same bits
    ce.zero_grad(set_to_none=True)
    xh = x.detach().clone().requires_grad_(True)
    again = ce.forward_on_graph(xh, g, features=features, fused=True, backward="fused")
    (again * d_out.to(DEV)).sum().backward()
    assert torch.equal(again.detach(), want) and torch.equal(xh.grad, xg.grad)


def test_arguments():
    """Test F: the refusals of the new keyword, all before any launch and with the module left alone; without a gradient wanted the
    keyword changes nothing."""
    shape, (variant, gain, mode, k) = MSHAPES[1], CASES[1]
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x)
    grad_x = lambda: x.clone().requires_grad_(True)
    _refused(ce, x, lambda: ce.forward_on_graph(x, g, backward="both"), "backward=")
    _refused(ce, x, lambda: ce.forward_on_graph(grad_x(), g, backward="both"), "backward=")
    with torch.no_grad():
        _refused(ce, x, lambda: ce.forward_on_graph(x, g, backward=None), "backward=")
    _refused(ce, x, lambda: ce.forward_on_graph(grad_x(), g, fused=False, backward="fused"), "contradicts")
    _refused(ce, x, lambda: ce.forward_on_graph(grad_x(), g, fused=True), "fused=True")                 # the default route keeps its refusal
    _refused(ce, x, lambda: ce.forward_on_graph(grad_x(), g, fused=True, backward="two_ops"), "fused=True")
    half, xh = _module(SEED, shape, variant, gain, mode, k, half=True)
    _refused(half, xh, lambda: half.forward_on_graph(xh.clone().requires_grad_(True), g, backward="fused"), "fp32 parameters")
    with torch.no_grad():
        default = ce.forward_on_graph(x, g)
        assert torch.equal(ce.forward_on_graph(x, g, backward="fused"), default)
        assert torch.equal(ce.forward_on_graph(x, g, fused=False, backward="fused"), default)           # only validated here
        for features in ("fp32", "split16"):
            fused = ce.forward_on_graph(x, g, features=features, fused=True)
            assert torch.equal(ce.forward_on_graph(x, g, features=features, fused=True, backward="fused"), fused)
    # under autograd the default keeps the two ops: their bits, their saved arrays
    out = ce.forward_on_graph(grad_x(), g)
    assert out.requires_grad and torch.equal(out.detach(), default)


# ---- CES / RR -----------------------------------------------------------------------------------------------------------------------
def _build_ces():
    """A ``CES`` with seeded parameters (``net.seeded_state_dict``), every head on top-k 8 and the fp32 route, and a seeded input."""
    from dagl_amd.net import CES, seeded_state_dict
    torch.manual_seed(3)
    ces = CES(64)
    ces.load_state_dict(seeded_state_dict(ces.state_dict(), 21), strict=True)
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode, hd.select_k, hd.scan = "topk", 8, "exact"
    x = _inputs(SEED, CES_SHAPE, "default", 2.0)[0]
    return ces.to(DEV).eval(), x.to(DEV)


def _ces_reference(x, prm, members, shape):
    """``CES.forward``'s wiring on the CPU in the dtype of ``x`` with ``_dense_on_structure`` (no margin: top-k) in the place of each head."""
    out = x
    for s in (1, 2, 3):
        outs = [_dense_on_structure(out, {n: prm[f"c{s}_{h}.{n}"] for n in _HEAD_NAMES}, members[(s - 1) * 4 + h - 1], False, shape)
                for h in (1, 2, 3, 4)]
        out = F.conv2d(torch.cat(outs, dim=1), prm[f"c{s}_c.weight"], prm[f"c{s}_c.bias"]) + out
        if s < 3:
            for i in range(4):
                p = f"RBS{s}.{i}.body."
                t = F.conv2d(out, prm[p + "0.weight"], prm[p + "0.bias"], padding=1)
                t = F.conv2d(F.prelu(t, prm[p + "1.weight"]), prm[p + "2.weight"], prm[p + "2.bias"], padding=1)
                out = t + out
    return out


_CES_GRADS = ("c2_c.weight", "c1_3.fc1.0.weight")


def test_ces_forward_on_graphs():
    """Test G: on the state of ``forward_with_graphs(x)`` the frozen-graph forward reproduces that call's output (the structures are
    given, nothing is selected again, so the tight bound of test_gpu_graph_attend.test_round_trip's rule applies: 1e-4), and its
    gradients in x, a mix weight and a first-stage head's fc1 weight are the fp64 evaluation's, for both ``backward`` values."""
    from dagl_amd import DaglError
    ces, x = _build_ces()
    B, H, W, L, N = _geom(CES_SHAPE)
    with torch.no_grad():
        want, state = ces.forward_with_graphs(x)
        for backward in ("two_ops", "fused"):
            out = ces.forward_on_graphs(x, state, backward=backward)
            err = normwise(out.double().cpu().numpy(), want.double().cpu().numpy())
            print(f"[train_on_graph] CES.forward_on_graphs ({backward}, no grad) vs forward_with_graphs: {err:.2e}")
            assert out.shape == x.shape and not out.requires_grad and err <= 1e-4
    members = [_member(state.head(s, h).cpu()) for s in range(3) for h in range(4)]
    d_out = torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(9))
    refs = []
    torch.set_num_threads(16)
    for dt in (torch.float64, torch.float32):
        xl = x.detach().cpu().to(dt).requires_grad_(True)
        pl = {n: t.detach().cpu().to(dt).requires_grad_(True) for n, t in ces.state_dict().items()}
        (_ces_reference(xl, pl, members, CES_SHAPE) * d_out.to(dt)).sum().backward()
        refs.append([xl.grad] + [pl[n].grad for n in _CES_GRADS])
    own = dict(ces.named_parameters())
    for backward in ("two_ops", "fused"):
        ces.zero_grad(set_to_none=True)
        xg = x.detach().clone().requires_grad_(True)
        out = ces.forward_on_graphs(xg, state, backward=backward)
        assert out.requires_grad
        err = normwise(out.detach().double().cpu().numpy(), want.double().cpu().numpy())
        assert err <= 1e-4, (backward, err)
        (out * d_out.to(DEV)).sum().backward()
        for name, lib, r64, r32 in zip(("x",) + _CES_GRADS, [xg.grad] + [own[n].grad for n in _CES_GRADS], *refs):
            _check(f"CES d {name} backward={backward}", lib, r64, r32, slack=1e-4)
    # refusals, before the first launch
    with pytest.raises(DaglError, match="the state was built for B=1 H=24 W=20"):
        ces.forward_on_graphs(x[:, :, :20], state)
    with pytest.raises(DaglError, match="SequenceState"):
        ces.forward_on_graphs(x, state.stages[0])
    with pytest.raises(DaglError, match="backward="):
        ces.forward_on_graphs(x, state, backward="both")
    with pytest.raises(DaglError, match="features="):
        ces.forward_on_graphs(x, state, features="fp16")


def test_rr_forward_on_graphs():
    """``RR.forward_on_graphs``: the trunk around ``CES.forward_on_graphs``; on the key frame's own state it reproduces the key frame's
    output, and the result trains (it requires grad and every head receives a gradient)."""
    from dagl_amd.net import RR, seeded_state_dict
    torch.manual_seed(3)
    rr = RR(n_resblocks=2)
    rr.load_state_dict(seeded_state_dict(rr.state_dict(), 22))
    ces = rr.body[1]
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode, hd.select_k, hd.scan = "topk", 8, "exact"
    rr = rr.to(DEV).eval()
    x = torch.randn(1, 1, 24, 20, generator=torch.Generator().manual_seed(17)).to(DEV)
    with torch.no_grad():
        want, state = rr.forward_with_graphs(x)
    out = rr.forward_on_graphs(x, state, backward="fused")
    assert out.requires_grad and out.shape == x.shape
    err = normwise(out.detach().double().cpu().numpy(), want.double().cpu().numpy())
    print(f"[train_on_graph] RR.forward_on_graphs vs forward_with_graphs: {err:.2e}")
    assert err <= 1e-4
    out.square().sum().backward()
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            assert hd.fc1[0].weight.grad is not None and bool(torch.isfinite(hd.fc1[0].weight.grad).all())
    assert rr.head[0].weight.grad is not None
