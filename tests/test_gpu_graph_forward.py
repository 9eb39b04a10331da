"""``ops.graph_forward`` (dagl_graph_forward, csrc/graph_forward.hip) and the ``features="split16"`` / ``fused`` arguments of
``CE.attend_graph`` / ``CE.forward_on_graph``.

Kernel level: crafted graphs on random features and a random value map against an fp64 evaluation of the formulas of include/dagl_ce.h
(``_forward_reference``: scores on the edges, margin, softmax over a row's EDGES plus the reference's e^0 per key off the graph, the
weighted patches, fold / overlap count).  Bound (the project's pattern): ``e_lib <= 3 e_32 + 1e-6`` normwise, ``e_32`` the same
evaluation by torch on the CPU in fp32.  Module level: the round trip under the rule of test_gpu_graph_attend.test_round_trip, gradients
against the fp32 route under ``3 e_32 + 1e-4`` (the bound of test_gpu_graph_attend.test_module_gradients, whose references these are)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import (CASES, KSHAPES, SHAPES, _GRAD_NAMES, _band, _dense_apply, _dense_on_structure, _edge_scores, _gap,
                                  _geom, _graph, _id, _inputs, _level_features, _module, _on_edges, _oracle, _padded, _refused, _rows_of,
                                  _seg)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
VARIANTS = [(True, "reference"), (False, "reference"), (True, "edges"), (False, "edges")]          # (with tau, normalize)
MSHAPES = [(1, 48, 48), (2, 20, 36)]
MCASES = [CASES[5], CASES[1]]                                                                       # top-k 8, adaptive
SEED = 11


def _vid(v):
    return ("tau" if v[0] else "notau") + "-" + v[1]


@functools.lru_cache(maxsize=None)
def _bad_key(shape):
    """The graph's keys with N, -1 and 2^31 - 1 in the long row (its first segment and its last) and in a short row."""
    row_off, key, _ = _graph(shape)
    B, H, W, L, N = _geom(shape)
    key = key.clone()
    key[int(row_off[1]) + 3] = N
    key[int(row_off[2]) - 2] = -1
    key[int(row_off[2])] = 2 ** 31 - 1
    return key


@functools.lru_cache(maxsize=None)
def _features(shape, seed=7):
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU for the graph of ``shape`` (``_level_features``)."""
    row_off, key, _ = _graph(shape)
    return _level_features(row_off, key, shape, seed)


def _forward_reference(wq, x, b2, row_off, key, tau, normalize, shape, scale=SCALE):
    """The formulas of include/dagl_ce.h for dagl_graph_attend + dagl_graph_apply in the dtype of ``wq``: a key outside [0, N) scores 0,
    takes part in D and carries no value row."""
    B, H, W, L, N = _geom(shape)
    deg = row_off[1:] - row_off[:-1]
    rows = _rows_of(row_off)
    valid = (key >= 0) & (key < N)
    kc = key.clamp(0, N - 1)
    S = _edge_scores(wq, x, rows, kc, L, N) * valid.to(wq.dtype)
    if tau is not None:
        m = F.relu(S - tau.reshape(-1)[rows])
        z, on = S * m * scale, m != 0
    else:
        z, on = S * scale, torch.ones_like(S, dtype=torch.bool)
    pos = torch.arange(key.numel()) - row_off[rows]
    Z = torch.full((B * L, max(int(deg.max()), 1)), float("-inf"), dtype=wq.dtype).index_put((rows, pos), z)
    off = (N - deg).clamp(min=0) if normalize == "reference" else torch.zeros_like(deg)
    M = Z.max(dim=1).values
    M = torch.where(off > 0, M.clamp(min=0.0), M)
    M = torch.where(deg > 0, M, torch.zeros_like(M))
    D = torch.exp(Z - M.unsqueeze(1)).sum(dim=1) + off.to(wq.dtype) * torch.exp(-M)
    w = (on & valid).to(wq.dtype) * torch.exp(z - M[rows]) / D[rows]
    return _dense_apply(row_off, kc, w, b2, shape)


@functools.lru_cache(maxsize=None)
def _kernel_reference(shape, with_tau, normalize, bad):
    """(fp64, fp32) outputs, computed once per case and shared."""
    row_off, key, b2 = _graph(shape)
    key = _bad_key(shape) if bad else key
    wq, x, tau = _features(shape)
    torch.set_num_threads(16)
    out = []
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            out.append(_forward_reference(wq.to(dt), x.to(dt), b2.to(dt), row_off, key, tau.to(dt) if with_tau else None, normalize, shape))
    return out


def _check(what, lib, ref64, ref32, slack=1e-6):
    e_lib = normwise(lib.detach().double().cpu().numpy(), ref64.detach().double().cpu().numpy())
    e_32 = normwise(ref32.detach().double().cpu().numpy(), ref64.detach().double().cpu().numpy())
    print(f"[graph_forward] {what}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, ratio {e_lib / max(e_32, 1e-30):.2f}")
    assert e_lib <= 3.0 * e_32 + slack, (what, e_lib, e_32)
    return e_32


def _device_args(shape, with_tau, bad):
    row_off, key, b2 = _graph(shape)
    key = _bad_key(shape) if bad else key
    wq, x, tau = _features(shape)
    return [t.to(DEV) for t in (wq, x, _padded(b2), row_off, key)], tau.to(DEV) if with_tau else None


def _graph_is_what_it_claims(shape):
    seg = _seg()
    row_off, key, _ = _graph(shape)
    B, H, W, L, N = _geom(shape)
    deg = row_off[1:] - row_off[:-1]
    assert int(deg[0]) == 0 and int(deg[-1]) == 0 and int(deg.max()) > N
    assert int(row_off[2] - 1) // seg - int(row_off[1]) // seg >= 2                        # the long row crosses three segments
    short = [(int(row_off[r]) // seg, int(row_off[r + 1] - 1) // seg) for r in range(B * L) if 0 < int(deg[r]) <= 8]
    assert all(a == b for a, b in short[:3]) and (L == 4 or len({a for a, _ in short[:6]}) < 6)
    bad = _bad_key(shape)
    assert int(((bad < 0) | (bad >= N)).sum()) == 3 and int(((key < 0) | (key >= N)).sum()) == 0


@pytest.mark.parametrize("bad", [False, True], ids=["keys_in_range", "keys_out_of_range"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", KSHAPES, ids=_id)
def test_kernel_against_fp64_on_a_crafted_graph(shape, variant, bad):
    """The fused call against the fp64 formulas and against the two existing calls on the same arrays; the same bits on a second call
    and through a ``Workspace``."""
    from dagl_amd import ops
    with_tau, normalize = variant
    B, H, W, L, N = _geom(shape)
    _graph_is_what_it_claims(shape)
    ref64, ref32 = _kernel_reference(shape, with_tau, normalize, bad)
    (wq, x, b2p, row_off, key), tau = _device_args(shape, with_tau, bad)
    kw = dict(tau=tau, scale=SCALE, normalize=normalize)
    out = ops.graph_forward(wq, x, b2p, row_off, key, **kw)
    assert out.shape == (B, 16, H, W) and out.dtype == torch.float32
    what = f"{shape} {_vid(variant)}{' bad keys' if bad else ''}, {key.numel()} edges"
    _check("fused vs fp64 " + what, out, ref64, ref32)
    weight, _ = ops.graph_attend(wq, x, row_off, key, hw=(H, W), **kw)
    two = ops.graph_apply(b2p, row_off, key, weight)
    e_32 = normwise(ref32.double().numpy(), ref64.numpy())
    e_two = normwise(out.double().cpu().numpy(), two.double().cpu().numpy())
    print(f"[graph_forward] fused vs attend + apply {what}: {e_two:.2e} (e_ref32 {e_32:.2e})")
    assert e_two <= 3.0 * e_32 + 1e-6
    ws = ops.Workspace()
    for again in (ops.graph_forward(wq, x, b2p, row_off, key, **kw), ops.graph_forward(wq, x, b2p, row_off, key, workspace=ws, **kw),
                  ops.graph_forward(wq, x, b2p, row_off, key, workspace=ws, **kw)):
        assert torch.equal(again, out)


@pytest.mark.parametrize("shape", [KSHAPES[0], KSHAPES[1]], ids=_id)
def test_empty_graph(shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    wq, x = torch.rand(B, L, 196, device=DEV), torch.rand(B, N, 196, device=DEV)
    b2p = torch.randn(B, H + 6, W + 6, 16, device=DEV)
    row_off = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    for tau in (None, torch.rand(B * L, device=DEV)):
        for normalize in ("reference", "edges"):
            out = ops.graph_forward(wq, x, b2p, row_off, key, tau=tau, normalize=normalize)
            assert out.shape == (B, 16, H, W) and bool((out == 0).all())


def test_operand_refusals():
    from dagl_amd import DaglError, ops
    shape = KSHAPES[0]
    (wq, x, b2p, row_off, key), tau = _device_args(shape, True, False)
    for call in (lambda: ops.graph_forward(wq, x, b2p[:, :-1].contiguous(), row_off, key),
                 lambda: ops.graph_forward(wq, x, b2p[..., :8].contiguous(), row_off, key),
                 lambda: ops.graph_forward(wq, x, b2p, row_off[:-1].contiguous(), key),
                 lambda: ops.graph_forward(wq, x, b2p, row_off, key, normalize="rows"),
                 lambda: ops.graph_forward(wq, x, b2p, row_off, key, tau=tau[:-1].contiguous()),
                 lambda: ops.graph_forward(wq, x, b2p, row_off, key, scale=0.0)):
        with pytest.raises(DaglError):
            call()


# ---- the module ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_out(shape, case, dtype):
    from oracle.ce_oracle import ce_forward_oracle
    variant, gain, mode, k = case
    x, prm = _inputs(SEED, shape, variant, gain)
    torch.set_num_threads(16)
    with torch.no_grad():
        return ce_forward_oracle(x, prm, mode=mode, k=k if mode != "adaptive" else None, dtype=dtype)


@pytest.mark.parametrize("case", MCASES, ids=_id)
@pytest.mark.parametrize("shape", MSHAPES, ids=_id)
def test_round_trip_with_split16_features(shape, case):
    """``forward_on_graph(x, graph(x), features="split16")`` is ``forward(x)`` under the rule test_gpu_graph_attend.test_round_trip applies
    to the fp32 route (1e-4 where the selection gap is >= 1e-6, 1e-3 otherwise); fused and two-op results agree within the kernel
    bound; ``attend_graph``'s weights are the fp32 route's outside the threshold band.  Measured on gfx950: see DESIGN.md section 4."""
    variant, gain, mode, k = case
    B, H, W = shape
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x, scores=True)
    weight0, score0 = g.weight.clone(), g.score.clone()
    with torch.no_grad():
        fused = ce.forward_on_graph(x, g, features="split16")
        assert torch.equal(fused, ce.forward_on_graph(x, g, features="split16", fused=True))           # None = fused here
        two = ce.forward_on_graph(x, g, features="split16", fused=False)
        a16 = ce.attend_graph(x, g, features="split16")
        a32 = ce.attend_graph(x, g)
    assert fused.shape == (B, 16, H, W) and fused.dtype == torch.float32
    assert torch.equal(g.weight, weight0) and torch.equal(g.score, score0)
    st64 = _oracle(SEED, shape, variant, gain, mode, k)
    gap = _gap(st64, mode, k, H, W)
    bound = 1e-4 if gap >= 1e-6 else 1e-3
    o64, o32 = _oracle_out(shape, case, torch.float64), _oracle_out(shape, case, torch.float32)
    e_32 = normwise(o32.double().numpy(), o64.numpy())
    e_f = normwise(fused.double().cpu().numpy(), two.double().cpu().numpy())
    print(f"[graph_forward] {shape} {case}: fused vs two ops {e_f:.2e} (e_ref32 {e_32:.2e})")
    assert e_f <= 3.0 * e_32 + 1e-6
    for scan in ("screened", "exact"):
        ce.scan = scan
        ce.invalidate_packed()
        with torch.no_grad():
            ref = ce(x)
        for name, out in (("fused", fused), ("two ops", two)):
            err = normwise(out.double().cpu().numpy(), ref.double().cpu().numpy())
            print(f"[graph_forward] {shape} {case} scan={scan}: split16 {name} vs forward {err:.2e} (bound {bound:.0e}, gap {gap:.1e})")
            assert err <= bound, (scan, name, err)
    # the weights: the fp32 route's, outside the threshold band of the fp64 oracle, under the kernel bound
    gc = g.cpu()
    keep = ~_band(st64, gc, mode, k)
    st32 = _oracle(SEED, shape, variant, gain, mode, k, torch.float32)
    r64, r32 = _on_edges(st64, "A", gc)[keep], _on_edges(st32, "A", gc)[keep]
    e_a32 = normwise(r32.double().numpy(), r64.numpy())
    e_w = normwise(a16.weight.cpu()[keep].double().numpy(), a32.weight.cpu()[keep].double().numpy())
    print(f"[graph_forward] {shape} {case}: split16 weights vs fp32 route {e_w:.2e} (e_ref32 {e_a32:.2e}), {int((~keep).sum())} edges in the band")
    assert e_w <= 3.0 * e_a32 + 1e-6
    assert torch.equal(a16.key, g.key) and a16.row_off is g.row_off


@pytest.mark.parametrize("case", MCASES, ids=_id)
def test_gradients_with_split16_features(case):
    """``forward_on_graph(features="split16")`` under autograd against the fp32 route's gradients, under the bound
    test_gpu_graph_attend.test_module_gradients applies to that route: ``3 e_32 + 1e-4``, e_32 the fp32 CPU autograd's error against
    fp64 on the dense formula with the structure as a mask."""
    shape = SHAPES[0]
    variant, gain, mode, k = case
    B, H, W, L, N = _geom(shape)
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x)
    gc = g.cpu()
    assert gc.n_edges > 0
    member = torch.zeros(B * L, N, dtype=torch.bool)
    member[gc.rows(), gc.key.long()] = True
    member = member.view(B, L, N)
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
    own = dict(ce.named_parameters())
    got = {}
    for features in ("fp32", "split16"):
        ce.zero_grad(set_to_none=True)
        xg = x.detach().clone().requires_grad_(True)
        out = ce.forward_on_graph(xg, g, features=features)
        assert out.requires_grad
        (out * d_out.to(DEV)).sum().backward()
        got[features] = [xg.grad.clone()] + [own[n].grad.clone() for n in names]
    for name, a, b, r64, r32 in zip(["x"] + names, got["split16"], got["fp32"], *refs):
        e_32 = normwise(r32.double().numpy(), r64.numpy())
        e = normwise(a.double().cpu().numpy(), b.double().cpu().numpy())
        print(f"[graph_forward] d {name} {case}: split16 vs fp32 route {e:.2e} (e_ref32 {e_32:.2e})")
        assert e <= 3.0 * e_32 + 1e-4, (name, e, e_32)


def test_arguments_and_refusals():
    from dagl_amd import DaglError, ops
    shape, (variant, gain, mode, k) = MSHAPES[1], CASES[1]
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x)
    for method in ("attend_graph", "forward_on_graph"):
        _refused(ce, x, lambda: getattr(ce, method)(x, g, features="fp16"), "features")
    _refused(ce, x, lambda: ce.forward_on_graph(x.clone().requires_grad_(True), g, fused=True), "fused=True")
    _refused(ce, x, lambda: ce.forward_on_graph(x.clone().requires_grad_(True), g, features="split16", fused=True), "fused=True")
    # default arguments: the two-op composition, bit for bit, called by hand on the route's own operands
    with torch.no_grad():
        default = ce.forward_on_graph(x, g)
        assert torch.equal(default, ce.forward_on_graph(x, g, features="fp32", fused=False))
        fused32 = ce.forward_on_graph(x, g, fused=True)
    e = normwise(fused32.double().cpu().numpy(), default.double().cpu().numpy())
    print(f"[graph_forward] fp32 features, fused vs default: {e:.2e}")
    assert e <= 1e-5                           # (another rounding order than the default's: why None does not pick it on this route)
    # under autograd None keeps the two differentiable ops, with either feature route
    for features in ("fp32", "split16"):
        out = ce.forward_on_graph(x.clone().requires_grad_(True), g, features=features)
        assert out.requires_grad


def test_half_module_under_no_grad():
    shape, (variant, gain, mode, k) = MSHAPES[1], CASES[1]
    ce, x = _module(SEED, shape, variant, gain, mode, k, half=True)
    g = ce.graph(x)
    with torch.no_grad():
        out = ce.forward_on_graph(x, g, features="split16")
        two = ce.forward_on_graph(x, g, features="split16", fused=False)
        ref = ce.forward_on_graph(x, g)
    assert out.dtype == two.dtype == torch.float16 and out.shape == (shape[0], 16, shape[1], shape[2])
    # the same fp32 copies through split-fp16 products (1e-4, the round trip's bound) + the two roundings to half of the outputs
    for name, o in (("fused", out), ("two ops", two)):
        err = normwise(o.double().cpu().numpy(), ref.double().cpu().numpy())
        print(f"[graph_forward] half module, split16 {name} vs fp32 route: {err:.2e}")
        assert err <= 1e-4 + 2.0 ** -10


@pytest.mark.parametrize("fused", [None, False], ids=["fused", "two_ops"])
@pytest.mark.parametrize("case", MCASES, ids=_id)
def test_out_of_range_input_is_nan_filled_and_the_module_stays(case, fused):
    """The input of test_gpu_round3.test_training_path_range_guard_moves_the_module_to_the_fp32_forward (features x 1e4: |b1| ~ 1e4 >
    4094): every element of the result is NaN -- with the margin too, where NaN scores alone would read as "no edge passes" -- and the
    module neither moves to scan = "exact" nor notes a violation; the fp32 route serves the same call."""
    shape = MSHAPES[0]
    variant, gain, mode, k = case
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x).validate()
    big = x * 1.0e4
    with torch.no_grad():
        out = ce.forward_on_graph(big, g, features="split16", fused=fused)
        a = ce.attend_graph(big, g, features="split16")
        ok = ce.forward_on_graph(big, g)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(a.weight).all())
    assert ce.scan == "screened" and bool(torch.isfinite(ok).all())
    with torch.no_grad():
        assert bool(torch.isfinite(ce.forward_on_graph(x, g, features="split16", fused=fused)).all())


def test_capture():
    """A validated graph through ``forward_on_graph(features="split16")`` under ``no_grad`` inside ``torch.cuda.graph`` (one stream, no
    parallel branches) replays to the eager bits, twice; an unvalidated graph under capture is refused."""
    from dagl_amd.graph import PatchGraph
    shape, (variant, gain, mode, k) = MSHAPES[0], CASES[1]
    ce, x = _module(SEED, shape, variant, gain, mode, k)
    g = ce.graph(x).validate()
    with torch.no_grad():
        eager = ce.forward_on_graph(x, g, features="split16").clone()      # (also brings the workspaces to their size before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ce.forward_on_graph(x, g, features="split16")
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, eager)
    fresh = PatchGraph(g.row_off, g.key, g.weight, None, *shape)

    def under_capture():
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            _ = x + 1.0
            ce.forward_on_graph(x, fresh, features="split16")
    _refused(ce, x, under_capture, "captur")
    torch.cuda.synchronize()
    assert not fresh._valid
