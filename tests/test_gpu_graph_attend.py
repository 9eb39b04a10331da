"""``ops.graph_attend`` / ``ops.graph_attend_backward`` / ``CE.attend_graph`` / ``CE.forward_on_graph`` (dagl_graph_attend*,
csrc/graph_attend.hip): the block's own edge weights on a GIVEN structure -- scores on the edges, the adaptive margin, the reference's
softmax restricted to the graph -- and their gradients.

Every reference is torch on the CPU in fp64, autograd for the gradients.  Kernel level: the dense ``S = Wq X^T`` with the graph's edges
taken out of it, the softmax over a row's EDGES (a repeated key is an entry of its own) plus the reference's ``e^0`` for each of the
``N - deg`` keys off the graph (``_edge_reference``).  Module level, on exported structures (no repeats): the dense [B, L, N] formula with
the structure as a mask (``_dense_on_structure``).  Bound (the project's pattern): ``e_lib <= 3 e_32 + 1e-6`` normwise against fp64,
``e_32`` the same formula evaluated by torch on the CPU in fp32; ``3 e_32 + 1e-4`` for gradients through the convolutions."""
import functools

import pytest
import torch

from tests.graph_reference import (CASES, SCALE, SHAPES, _GRAD_NAMES, _band, _check, _crafted, _dense_a, _dense_on_structure,
                                  _edge_reference, _gap, _geom, _id, _inputs, _level_features, _module, _on_edges, _oracle, _refused,
                                  _rows_of, _seed)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = [(True, "reference"), (False, "reference"), (True, "edges"), (False, "edges")]          # (with tau, normalize)


def _vid(v):
    return ("tau" if v[0] else "notau") + "-" + v[1]


@functools.lru_cache(maxsize=None)
def _features(shape, seed=7):
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU for the crafted graph of ``shape`` (``_level_features``)."""
    row_off, key, _, _ = _crafted(shape)
    return _level_features(row_off, key, shape, seed)


@functools.lru_cache(maxsize=None)
def _kernel_reference(shape, with_tau, normalize, dtype):
    row_off, key, _, _ = _crafted(shape)
    wq, x, tau = _features(shape)
    torch.set_num_threads(16)
    with torch.no_grad():
        return _edge_reference(wq.to(dtype), x.to(dtype), row_off, key, tau.to(dtype) if with_tau else None, normalize, shape)


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_kernel_against_fp64_on_a_crafted_graph(shape, variant):
    """Test 1: weights and scores on the long-tailed graph (degrees 0, 1, SEG-1, SEG, SEG+1, 2 SEG+3, N, N+5, repeated and unsorted keys,
    the last row of image 0 followed by an empty row); the same bits on a second call and through a ``Workspace``."""
    from dagl_amd import ops
    with_tau, normalize = variant
    B, H, W, L, N = _geom(shape)
    row_off, key, _, _ = _crafted(shape)
    wq, x, tau = _features(shape)
    w64, s64, z64 = _kernel_reference(shape, with_tau, normalize, torch.float64)
    w32, s32, _ = _kernel_reference(shape, with_tau, normalize, torch.float32)
    # the case is what it claims to be, on the fp64 reference: logits neither flat nor one-hot, no margin in doubt
    rows, deg = _rows_of(row_off), row_off[1:] - row_off[:-1]
    for r in range(B * L):
        zr = z64[int(row_off[r]):int(row_off[r + 1])]
        if zr.numel() == 0 or (normalize == "edges" and zr.numel() == 1):          # (one edge alone is one-hot by definition)
            continue
        lo = min(float(zr.min()), 0.0) if normalize == "reference" and int(deg[r]) < N else float(zr.min())
        assert 2.0 <= float(zr.max()) - lo <= 30.0, (r, int(deg[r]), float(zr.max()) - lo)
    if with_tau:
        margin = ((s64 - tau.double()[rows]).abs() / s64.abs()).min()
        print(f"[graph_attend] {shape}: min |S - tau| / |S| = {float(margin):.2e}; edges on {int((w64 != 0).sum())} of {key.numel()}")
        assert float(margin) >= 1e-3
        assert 0 < int((w64 != 0).sum()) < key.numel()
    args = [t.to(DEV) for t in (wq, x, row_off, key)]
    kw = dict(tau=tau.to(DEV) if with_tau else None, scale=SCALE, normalize=normalize)
    weight, score = ops.graph_attend(*args, **kw)
    assert weight.shape == score.shape == (key.numel(),) and weight.dtype == score.dtype == torch.float32
    _check(f"score {shape} {_vid(variant)}", score, s64, s32)
    _check(f"weight {shape} {_vid(variant)}", weight, w64, w32)
    assert torch.equal((weight != 0).cpu(), w64 != 0)
    ws = ops.Workspace()
    for again in (ops.graph_attend(*args, **kw), ops.graph_attend(*args, workspace=ws, **kw), ops.graph_attend(*args, workspace=ws, **kw),
                  ops.graph_attend(*args, hw=(H, W), **kw)):
        assert torch.equal(again[0], weight) and torch.equal(again[1], score)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_empty_graph(shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    wq, x = torch.rand(B, L, 196, device=DEV), torch.rand(B, N, 196, device=DEV)
    row_off = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    tau = torch.rand(B * L, device=DEV)
    for t in (None, tau):
        weight, score = ops.graph_attend(wq, x, row_off, key, tau=t)
        assert weight.shape == score.shape == (0,) and weight.dtype == score.dtype == torch.float32
    none = torch.empty(0, device=DEV)
    transposed = (torch.zeros(B * N + 1, dtype=torch.int64, device=DEV), key, key)
    d_wq, d_x, d_tau = ops.graph_attend_backward(none, wq, x, row_off, key, none, none, tau=tau, transposed=transposed)
    assert d_wq.shape == wq.shape and d_x.shape == x.shape and d_tau.shape == (B * L,)
    assert bool((d_wq == 0).all()) and bool((d_x == 0).all()) and bool((d_tau == 0).all())


@functools.lru_cache(maxsize=None)
def _grad_reference(shape, with_tau, normalize, dtype):
    row_off, key, _, _ = _crafted(shape)
    wq, x, tau = _features(shape)
    g = torch.randn(key.numel(), generator=torch.Generator().manual_seed(9))
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (wq, x, tau)]
    torch.set_num_threads(16)
    w, _, _ = _edge_reference(leaves[0], leaves[1], row_off, key, leaves[2] if with_tau else None, normalize, shape)
    (w * g.to(dtype)).sum().backward()
    return g, [t.grad for t in leaves]


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=_id)
def test_kernel_gradients(shape, variant):
    """Test 2: ``ops.graph_attend_backward`` against fp64 autograd of the reference, the same bits on a second call, and a subset of the
    outputs (``need_*``) gives the bits of the full call."""
    from dagl_amd import ops
    from dagl_amd.graph import PatchGraph
    with_tau, normalize = variant
    B, H, W, L, N = _geom(shape)
    row_off, key, cw, _ = _crafted(shape)
    wq, x, tau = _features(shape)
    g, ref64 = _grad_reference(shape, with_tau, normalize, torch.float64)
    _, ref32 = _grad_reference(shape, with_tau, normalize, torch.float32)
    pg = PatchGraph(row_off, key, cw, None, B, H, W).to(DEV)
    fwd = (wq.to(DEV), x.to(DEV), pg.row_off, pg.key)
    kw = dict(tau=tau.to(DEV) if with_tau else None, scale=SCALE, normalize=normalize)
    weight, score = ops.graph_attend(*fwd, **kw)
    args = (g.to(DEV), *fwd, score, weight)
    d_wq, d_x, d_tau = ops.graph_attend_backward(*args, transposed=pg.transpose(), **kw)
    _check(f"d_wq {shape} {_vid(variant)}", d_wq, ref64[0], ref32[0])
    _check(f"d_x {shape} {_vid(variant)}", d_x, ref64[1], ref32[1])
    if with_tau:
        _check(f"d_tau {shape} {_vid(variant)}", d_tau, ref64[2], ref32[2])
    else:
        assert d_tau is None
    again = ops.graph_attend_backward(*args, transposed=pg.transpose(), **kw)
    ws = ops.Workspace()
    through_ws = ops.graph_attend_backward(*args, transposed=pg.transpose(), workspace=ws, **kw)
    for a, b, c in zip(again, through_ws, (d_wq, d_x, d_tau)):
        assert (c is None and a is None and b is None) or (torch.equal(a, c) and torch.equal(b, c))
    only_wq = ops.graph_attend_backward(*args, need_x=False, need_tau=False, **kw)
    assert only_wq[1] is None and only_wq[2] is None and torch.equal(only_wq[0], d_wq)
    only_x = ops.graph_attend_backward(*args, transposed=pg.transpose(), need_wq=False, need_tau=False, **kw)
    assert only_x[0] is None and only_x[2] is None and torch.equal(only_x[1], d_x)
    if with_tau:
        only_tau = ops.graph_attend_backward(*args, need_wq=False, need_x=False, **kw)
        assert only_tau[0] is None and only_tau[1] is None and torch.equal(only_tau[2], d_tau)


def test_edges_normalisation_sums_to_one():
    """Test 5: without a margin, ``normalize="edges"`` is a softmax over the row's edges."""
    from dagl_amd import ops
    for shape in (SHAPES[0], SHAPES[3]):
        row_off, key, _, _ = _crafted(shape)
        wq, x, _ = _features(shape)
        weight, _ = ops.graph_attend(wq.to(DEV), x.to(DEV), row_off.to(DEV), key.to(DEV), normalize="edges")
        deg = row_off[1:] - row_off[:-1]
        sums = torch.zeros(deg.numel(), dtype=torch.float64).index_add_(0, _rows_of(row_off), weight.double().cpu())
        err = (sums[deg > 0] - 1.0).abs().max()
        print(f"[graph_attend] {shape}: max |sum_e w_e - 1| over {int((deg > 0).sum())} rows = {float(err):.2e}")
        assert float(err) <= 1e-5 and bool((sums[deg == 0] == 0).all())


def _check_against_export(what, got, g, st64, st32, mode, k, over_pairs=False):
    """``attend_graph``'s arrays against the export's on the export's own structure: scores on every edge, weights outside the band.
    The band may hold at most 5e-4 of the edges (``over_pairs``: of all B L N pairs, the count graph_reference.check_edges caps)."""
    band = _band(st64, g, mode, k)
    share = float(band.sum()) / max(g.B * g.L * g.N if over_pairs else g.n_edges, 1)
    print(f"[graph_attend] {what}: {int(band.sum())} of {g.n_edges} edges in the threshold band")
    assert share <= 5e-4
    assert torch.equal(got.row_off.cpu(), g.row_off) and torch.equal(got.key.cpu(), g.key)
    for name, lib, exp, ref, keep in (("score", got.score, g.score, "S", torch.ones_like(band)), ("weight", got.weight, g.weight, "A", ~band)):
        if int(keep.sum()) == 0:
            continue
        r64, r32 = _on_edges(st64, ref, g)[keep], _on_edges(st32, ref, g)[keep]
        e_32 = normwise(r32.double().numpy(), r64.numpy())
        e_lib = normwise(lib.detach().cpu()[keep].double().numpy(), r64.numpy())
        e_exp = normwise(lib.detach().cpu()[keep].double().numpy(), exp[keep].double().numpy())
        print(f"[graph_attend] {what} {name}: against the export {e_exp:.2e}, against fp64 {e_lib:.2e}, e_ref32 {e_32:.2e}")
        assert e_exp <= 3.0 * e_32 + 1e-6, (what, name, e_exp, e_32)
        assert e_lib <= 3.0 * e_32 + 1e-6, (what, name, e_lib, e_32)
    return int(band.sum())


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5], CASES[9]], ids=_id)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_round_trip(shape, case):
    """Test 3: ``attend_graph(x, graph(x))`` returns the export's scores and (outside the threshold band) weights; ``forward_on_graph(x,
    graph(x))`` is ``forward(x)`` under the rule of test_gpu_graph_apply.test_round_trip."""
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    B, H, W = shape
    ce, x = _module(seed, shape, variant, gain, mode, k)
    g_dev = ce.graph(x, scores=True)
    with torch.no_grad():
        got = ce.attend_graph(x, g_dev)
        out = ce.forward_on_graph(x, g_dev)
    assert got.weight.dtype == got.score.dtype == torch.float32 and not got.weight.requires_grad
    st64 = _oracle(seed, shape, variant, gain, mode, k)
    st32 = _oracle(seed, shape, variant, gain, mode, k, torch.float32)
    _check_against_export(f"seed {seed} {shape} {case}", got, g_dev.cpu(), st64, st32, mode, k)
    assert out.shape == (B, 16, H, W) and out.dtype == torch.float32
    gap = _gap(st64, mode, k, H, W)
    bound = 1e-4 if gap >= 1e-6 else 1e-3
    for scan in ("screened", "exact"):
        ce.scan = scan
        ce.invalidate_packed()
        with torch.no_grad():
            ref = ce(x)
        err = normwise(out.double().cpu().numpy(), ref.double().cpu().numpy())
        print(f"[graph_attend] seed {seed} {shape} {case} scan={scan}: forward_on_graph(graph) vs forward {err:.2e} (bound {bound:.0e})")
        assert err <= bound, (scan, err)


@pytest.mark.parametrize("case", [CASES[1], CASES[5], CASES[9]], ids=_id)
def test_module_gradients(case):
    """Test 4: ``forward_on_graph`` under autograd -- d x and the gradient of every parameter of g, theta, fc1, fc2, thr_conv, bias_conv
    against fp64 autograd of the dense formula on the same structure.  No edge of the structure is threshold-ambiguous (asserted), so
    every margin has the reference's sign in all three evaluations.  In "topk" the heads get no gradient; ``W`` never does."""
    shape = SHAPES[0]
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    B, H, W, L, N = _geom(shape)
    ce, x = _module(seed, shape, variant, gain, mode, k)
    g = ce.graph(x)
    gc = g.cpu()
    st64 = _oracle(seed, shape, variant, gain, mode, k)
    assert gc.n_edges > 0 and int(_band(st64, gc, mode, k).sum()) == 0
    member = torch.zeros(B * L, N, dtype=torch.bool)
    member[gc.rows(), gc.key.long()] = True
    member = member.view(B, L, N)
    margin = mode != "topk"
    d_out = torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(9))
    x0, prm = _inputs(seed, shape, variant, gain)
    names = [n for n in _GRAD_NAMES if margin or not n.startswith(("thr_conv", "bias_conv"))]
    refs = []
    torch.set_num_threads(16)
    for dt in (torch.float64, torch.float32):
        xl = x0.to(dt).clone().requires_grad_(True)
        pl = {n: t.to(dt).clone().requires_grad_(True) for n, t in prm.items()}
        (_dense_on_structure(xl, pl, member, margin, shape) * d_out.to(dt)).sum().backward()
        refs.append([xl.grad] + [pl[n].grad for n in names])
    xg = x.detach().clone().requires_grad_(True)
    out = ce.forward_on_graph(xg, g)
    assert out.requires_grad
    (out * d_out.to(DEV)).sum().backward()
    own = dict(ce.named_parameters())
    for name, lib, r64, r32 in zip(["x"] + names, [xg.grad] + [own[n].grad for n in names], *refs):
        assert lib is not None and r64 is not None, name
        _check(f"d {name} {case}", lib, r64, r32, slack=1e-4)
    for n, p in own.items():
        if n not in names:
            assert p.grad is None, n                                  # W; in "topk" the two heads
    # attend_graph alone: its weight carries the graph of g, fc1, fc2 and the heads, not of theta
    ce.zero_grad(set_to_none=True)
    a = ce.attend_graph(x, g)
    assert a.weight.requires_grad and not a.score.requires_grad
    a.weight.sum().backward()
    assert bool((own["fc1.0.weight"].grad != 0).any()) and bool((own["g.weight"].grad != 0).any())
    assert own["theta.weight"].grad is None or bool((own["theta.weight"].grad == 0).all())


def test_margin_and_normalize_arguments():
    """``margin`` overrides the module's mode and ``normalize="edges"`` reaches the kernel (the kernel tests check the values): on a
    top-k module's structure the rows' sums and the weights tell the variants apart."""
    shape, (variant, gain, mode, k) = SHAPES[0], CASES[5]
    ce, x = _module(11, shape, variant, gain, mode, k)
    g = ce.graph(x)
    rows = g.rows()
    with torch.no_grad():
        plain = ce.attend_graph(x, g)
        edges = ce.attend_graph(x, g, normalize="edges")
        with_margin = ce.attend_graph(x, g, margin=True)
    sums = lambda w: torch.zeros(g.B * g.L, device=DEV, dtype=torch.float64).index_add_(0, rows, w.double())
    # (the edges-only denominator is the reference's without its (N - deg) e^(-M) >= 0: no weight can come out smaller)
    assert float((sums(edges.weight) - 1).abs().max()) <= 1e-5 and bool((edges.weight >= plain.weight * (1 - 1e-6)).all())
    assert torch.equal(with_margin.score, plain.score) and not torch.equal(with_margin.weight, plain.weight)
    assert torch.equal(with_margin.key, g.key) and with_margin.row_off is g.row_off


@functools.lru_cache(maxsize=None)
def _oracles_of(kind):
    """(st64, st32) of test 6's module: the half module sees half-rounded input and weights, the oracle gets the same values."""
    from oracle.ce_oracle import ce_forward_oracle
    shape, (variant, gain, mode, k) = SHAPES[0], ("sparse", 1.2, "adaptive", 0)
    cin, half = (32, False) if kind == "in_channels_32" else (64, True)
    x0, prm = _inputs(12, shape, variant, gain, cin)
    if half:
        x0, prm = x0.half().float(), {n: t.half().float() for n, t in prm.items()}
    sts = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            _, st = ce_forward_oracle(x0, prm, mode=mode, dtype=dt, stages=True)
        st["A"] = _dense_a(st, mode)
        sts.append(st)
    return sts


@pytest.mark.parametrize("kind", ["in_channels_32", "half_module"])
def test_other_widths_and_precisions(kind):
    """Test 6: a 32-channel module, and a .half() module with a half input under ``no_grad`` (computed on the fp32 copies): the
    export's scores and weights again, and ``forward_on_graph`` against ``apply_graph`` of the export -- the same product with weights
    that agree within the kernel bound, so 1e-4 (the round trip's bound) plus, for the half output, its two roundings 2^-10."""
    shape, (variant, gain, mode, k) = SHAPES[0], ("sparse", 1.2, "adaptive", 0)
    cin, half = (32, False) if kind == "in_channels_32" else (64, True)
    ce, x = _module(12, shape, variant, gain, mode, k, in_channels=cin, half=half)
    g = ce.graph(x, scores=True)
    with torch.no_grad():
        got = ce.attend_graph(x, g)
        out = ce.forward_on_graph(x, g)
        ref = ce.apply_graph(x, g)
    st64, st32 = _oracles_of(kind)
    # (the fp64 oracle finds 5 of the 32-channel module's 6 182 edges in the band, 8e-4 of the edges: this case keeps the cap of
    # test_gpu_patch_graph.test_other_widths_and_precisions, 5e-4 of all pairs, and still compares every edge outside the band)
    _check_against_export(kind, got, g.cpu(), st64, st32, mode, k, over_pairs=True)
    assert out.dtype == x.dtype and out.shape == (shape[0], 16, shape[1], shape[2])
    err = normwise(out.double().cpu().numpy(), ref.double().cpu().numpy())
    bound = 1e-4 + (2.0 ** -10 if half else 0.0)
    print(f"[graph_attend] {kind}: forward_on_graph vs apply_graph(graph) {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    if half:
        from dagl_amd import DaglError
        with pytest.raises(DaglError, match="fp32 parameters"):
            ce.forward_on_graph(x.clone().requires_grad_(True), g)


@pytest.mark.parametrize("method", ["attend_graph", "forward_on_graph"])
def test_refusals_leave_the_module_alone(method):
    """Test 7: ``apply_graph``'s refusals, for both methods: a ``DaglError`` before anything is launched, the state dict and the
    forward's packed weights as they were."""
    from dagl_amd.graph import PatchGraph
    shape, (variant, gain, mode, k) = SHAPES[3], CASES[5]
    ce, x = _module(11, shape, variant, gain, mode, k)
    call = getattr(ce, method)
    g = ce.graph(x)
    B, H, W, L, N = _geom(shape)

    def empty(b, h, w, dev=DEV):
        l = (-(-h // 4)) * (-(-w // 4))
        return PatchGraph(torch.zeros(b * l + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                          torch.empty(0, device=dev), None, b, h, w)
    for other in ((B, H, W + 4), (B, H - 4, W), (B + 1, H, W)):
        _refused(ce, x, lambda: call(x, empty(*other)), "the graph was built for")
    _refused(ce, x, lambda: call(x, g.cpu()), "lives on cpu")
    _refused(ce, x, lambda: call(x, "graph"), "PatchGraph expected")
    _refused(ce, x, lambda: call(x, g, normalize="rows"), "normalize")
    _refused(ce, x, lambda: call(x[:, :32], g), "expected [B,64,H,W]")
    key = g.key.clone()
    key[5] = N
    bad = PatchGraph(g.row_off, key, g.weight, None, B, H, W)
    for _ in range(2):
        assert "key 4096" in _refused(ce, x, lambda: call(x, bad), "edge 5")
    fresh = PatchGraph(g.row_off, g.key, g.weight, None, B, H, W)

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            call(x, fresh)
    _refused(ce, x, captured, "captur")
    torch.cuda.synchronize()
    assert not fresh._valid
    half = ce.half()
    _refused(half, x.half(), lambda: getattr(half, method)(x.half().requires_grad_(True), g), "fp32 parameters")


@pytest.mark.parametrize("method", ["attend_graph", "forward_on_graph"])
def test_refusal_of_a_generic_geometry(method):
    from dagl_amd.ce import CE
    from dagl_amd.graph import PatchGraph
    torch.manual_seed(5)
    ce = CE(ksize=5, stride_1=2, stride_2=1, inter_channels=16, in_channels=64).to(DEV).eval()
    x = torch.randn(1, 64, 20, 24, device=DEV)
    g = PatchGraph(torch.zeros(5 * 6 + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                   torch.empty(0, device=DEV), None, 1, 20, 24)
    _refused(ce, x, lambda: getattr(ce, method)(x, g), "scope")


def test_capture():
    """Test 8: a validated graph through ``forward_on_graph`` under ``no_grad`` inside ``torch.cuda.graph`` (one stream, no parallel
    branches) replays to the eager bits, twice."""
    shape, (variant, gain, mode, k) = SHAPES[3], CASES[9]
    ce, x = _module(_seed(shape, CASES[9]), shape, variant, gain, mode, k)
    g = ce.graph(x).validate()
    with torch.no_grad():
        eager = ce.forward_on_graph(x, g).clone()      # (also brings the module's workspaces to their size before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ce.forward_on_graph(x, g)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, eager)
