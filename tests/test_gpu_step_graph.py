"""``ops.graph_step`` (dagl_graph_step, csrc/graph_refresh.hip) and ``CE.step_graph``: the refresh of a patch graph and the block's output
on its result in one call.

The graph of a step is held EXACTLY against ``ops.graph_refresh`` / ``CE.refresh_graph`` with the same arguments (whose own tests hold it
against the CPU selection and fp64); the output against torch on the CPU in fp64 on that graph and against the library's other routes
under the project's rule ``e <= 3 e_ref32 + 1e-6``; and it must carry the same bits whichever form of the call produced it."""
import pytest
import torch

from tests.graph_reference import (ATOPK16, COMBOS, _check, _cid, _dense_on_structure, _gap, _geom, _inputs, _mod, _module, _oracle, _padded,
                                  _refused, _rows_of, membership)
from tests.graph_step_reference import (MAX_ROW, R_FAIL, R_LONG, SHAPES, apply_references, check_against, crafted, features, value_map,
                                        without_rows)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
ARRAYS = ("row_off", "key", "weight", "score")
# (name, with tau, k, keep_all, normalisations)
SELECTIONS = [("tau", True, 0, False, ("reference",)), ("k3", False, 3, False, ("reference",)),
              ("tau_k3", True, 3, False, ("reference", "edges")), ("keep_all", False, 0, True, ("reference",)),
              ("keep_all_tau", True, 0, True, ("edges",))]


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _device_args(shape):
    row_off, key = crafted(shape)
    wq, x, tau = features(shape)
    return [t.to(DEV) for t in (wq, x, _padded(value_map(shape)), row_off, key)], tau.to(DEV)


def _poisoned(shape, E, radius):
    """A ``Workspace`` whose buffer, large enough for every form of the call, holds a non-zero byte pattern (0x5b5b5b5b is 6.2e16 as a
    float): a row of the aggregated rows that no exit of the kernel writes shows in the output."""
    from dagl_amd import _lib, ops
    B, H, W, L, N = _geom(shape)
    need = _lib.load().dagl_graph_step_workspace_bytes(B, H, W, E, radius, 1)
    assert need > 0
    ws = ops.Workspace()
    ws.get(need, torch.device(DEV)).fill_(0x5B)
    return ws, ws.peek(DEV)


def _cpu(csr):
    return {n: csr[n].cpu() for n in ARRAYS}


# ---- the kernel, on a crafted graph -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_kernel_on_a_crafted_graph(shape, radius):
    """Declared ``max_row_edges`` 12: radius 0 / 1 run a wavefront per row (12 / 108 candidates), radius 2 a block (300)."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    row_off, key = crafted(shape)
    assert int((row_off[1:] - row_off[:-1]).max()) == int(row_off[R_LONG + 1] - row_off[R_LONG]) == MAX_ROW
    args, tau_dev = _device_args(shape)
    wq, x, b2p, off_dev, key_dev = args
    E = key.numel()
    for name, with_tau, k, keep_all, normalizations in SELECTIONS:
        for normalize in normalizations:
            what = f"{shape} radius {radius} {name} {normalize}"
            kw = dict(radius=radius, tau=tau_dev if with_tau else None, k=k, scale=SCALE, normalize=normalize, keep_all=keep_all,
                      max_row_edges=MAX_ROW)
            want = ops.graph_refresh(wq, x, off_dev, key_dev, hw=(H, W), **kw)
            ws, buf = _poisoned(shape, E, radius)
            out, csr, status = ops.graph_step(*args, workspace=ws, **kw)
            assert ws.peek(DEV) is buf, "the call must have run in the poisoned buffer"
            assert out.shape == (B, 16, H, W) and out.dtype == torch.float32 and status.tolist()[0] == 0
            # 1. the graph: ops.graph_refresh's, bit for bit
            for n in ARRAYS:
                assert torch.equal(csr[n], want[n]), (what, n)
            c = _cpu(csr)
            if with_tau and not keep_all:
                assert int(c["row_off"][R_FAIL + 1] - c["row_off"][R_FAIL]) == 0
            assert int(c["row_off"][1]) == 0 and (B == 1 or int(c["row_off"][L + 1] - c["row_off"][L]) == 0)
            # 2. the output against fold(A . V) / cnt on that graph, fp64 and fp32 on the CPU
            ref64, ref32 = apply_references(c["row_off"], c["key"], c["weight"], shape)
            _check(f"step out {what}", out, ref64, ref32)
            # 3. against ops.graph_apply on that graph
            check_against(f"step out vs graph_apply {what}", out, ops.graph_apply(b2p, csr["row_off"], csr["key"], csr["weight"]),
                          ref64, ref32)
            # 4. the same bits without the graph, a block per row, again, and through one Workspace twice -- each first call in a
            #    poisoned buffer of its own
            shared = _poisoned(shape, E, radius)[0]
            for again in (dict(want_graph=False), dict(block_rows=True), dict(want_graph=False, block_rows=True), dict(),
                          dict(workspace=shared), dict(workspace=shared), dict(workspace=shared, want_graph=False)):
                o, g2, st = ops.graph_step(*args, **{"workspace": _poisoned(shape, E, radius)[0], **kw, **again})
                assert torch.equal(o, out), (what, sorted(again))
                assert st.tolist()[0] == 0
                if again.get("want_graph", True):
                    assert all(torch.equal(g2[n], want[n]) for n in ARRAYS), (what, sorted(again))
                else:
                    assert g2 is None
            o, _, _ = ops.graph_step(*args, **kw)                            # and without a Workspace
            assert torch.equal(o, out), what


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_empty_graph(shape):
    """``E = 0``, and a graph whose only keys lie off the map: zeros of the right shape with and without the graph."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    wq, x = torch.rand(B, L, 196, device=DEV), torch.rand(B, N, 196, device=DEV)
    b2p = _padded(value_map(shape)).to(DEV)
    row_off = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    for kw in (dict(), dict(tau=torch.rand(B * L, device=DEV), k=8), dict(keep_all=True, radius=2)):
        for want_graph in (True, False):
            out, csr, status = ops.graph_step(wq, x, b2p, row_off, key, max_row_edges=0, want_graph=want_graph, **kw)
            assert out.shape == (B, 16, H, W) and out.dtype == torch.float32 and not bool(out.any())
            assert status.tolist() == [0, 0]
            if want_graph:
                assert csr["key"].shape == csr["weight"].shape == csr["score"].shape == (0,)
                assert csr["row_off"].shape == (B * L + 1,) and not bool(csr["row_off"].any())
            else:
                assert csr is None
    row_off[1:] = 2
    off_map = torch.tensor([-1, N], dtype=torch.int32, device=DEV)
    for want_graph in (True, False):
        ws, _ = _poisoned(shape, 2, 1)
        out, csr, status = ops.graph_step(wq, x, b2p, row_off, off_map, radius=1, max_row_edges=2, want_graph=want_graph, workspace=ws)
        assert not bool(out.any()) and status.tolist()[0] == 0
        assert csr is None or (csr["key"].numel() == 0 and not bool(csr["row_off"].any()))


@pytest.mark.parametrize("radius", [1, 2])
def test_overlong_rows_are_zero_rows_not_truncated(radius):
    """``max_row_edges`` declared one below the truth.  With the graph the call raises ``ERR_UNSUPPORTED`` naming the count; without it
    the row contributes zeros, ``status[0]`` counts it and every other row is what it was."""
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    args, tau_dev = _device_args(shape)
    with pytest.raises(_lib.DaglError, match="1 row") as e:
        ops.graph_step(*args, radius=radius, k=8, max_row_edges=MAX_ROW - 1)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "graph_step" in str(e.value)
    whole = _cpu(ops.graph_refresh(args[0], args[1], args[3], args[4], radius=radius, k=8, max_row_edges=MAX_ROW, hw=(H, W)))
    assert int(whole["row_off"][R_LONG + 1] - whole["row_off"][R_LONG]) == 8
    ws, _ = _poisoned(shape, args[4].numel(), radius)
    out, csr, status = ops.graph_step(*args, radius=radius, k=8, max_row_edges=MAX_ROW - 1, want_graph=False, workspace=ws)
    assert csr is None and status.tolist()[0] == 1
    ref64, ref32 = apply_references(*without_rows(whole["row_off"], whole["key"], whole["weight"], [R_LONG]), shape)
    _check(f"step out, overlong row left out, radius {radius}", out, ref64, ref32)
    full, _, status = ops.graph_step(*args, radius=radius, k=8, max_row_edges=MAX_ROW, want_graph=False)
    assert status.tolist()[0] == 0 and not torch.equal(full, out)


def test_operand_refusals():
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    args, tau_dev = _device_args(shape)
    wq, x, b2p, row_off, key = args
    ok = dict(max_row_edges=MAX_ROW)
    for bad, kw, word in (([wq, x, b2p[:, :-1].contiguous(), row_off, key], ok, "keys"),         # a border row short: another map
                          ([wq, x, b2p[..., :12].contiguous(), row_off, key], ok, "b2p"),
                          ([wq, x, b2p[:1], row_off, key], ok, "images"),
                          ([wq, x, b2p, row_off[:-1], key], ok, "row_off"),
                          (args, dict(ok, tau=tau_dev[:-1]), "tau"), (args, dict(ok, scale=0.0), "scale"),
                          (args, dict(ok, normalize="rows"), "normalize"), (args, dict(ok, radius=9), "radius"),
                          (args, dict(ok, k=-1), "k=-1"), (args, dict(ok, hw=(H, W + 1)), "hw"),
                          (args, dict(want_graph=False), "max_row_edges")):
        with pytest.raises(_lib.DaglError, match=word):
            ops.graph_step(*bad, **kw)
    with pytest.raises(_lib.DaglError, match="candidates") as e:
        ops.graph_step(*args, radius=8, max_row_edges=MAX_ROW)                                    # 12 x 289
    assert e.value.code == _lib.ERR_UNSUPPORTED

    def captured(**kw):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = wq + 1.0
            ops.graph_step(*args, **kw)
    with pytest.raises(_lib.DaglError, match="captur"):
        captured(max_row_edges=MAX_ROW)
    with pytest.raises(_lib.DaglError, match="captur"):
        captured(want_graph=False)
    torch.cuda.synchronize()


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
# top-k 8 at (2,24,20) and (1,64,64); adaptive AND top-16; top-k 64 at (1,33,70): 576 candidates at radius 1, a block per row; sparse
# adaptive: largest degree 59; the empty graph; radius 2 on the adaptive AND top-16 case (400 candidates)
STEP_CASES = [(COMBOS[0], 1), (COMBOS[2], 1), (COMBOS[6], 1), (COMBOS[4], 1), (COMBOS[9], 1), (COMBOS[12], 1), (COMBOS[6], 2)]
# the fixed point: the cases above whose fp64 oracle has a k-th / (k+1)-th gap of 1e-6 or more (3.6e-5, 1.3e-5, 2.6e-5, no rank cut -- on
# the CPU), so that the tight bound of the round-trip rule, 1e-4, is the one that applies; top-k 8 at (1,64,64) has 1.0e-6 and is left out
FIXED_POINT = [COMBOS[0], COMBOS[4], COMBOS[6], COMBOS[9]]


def _same_graph(a, b):
    for n in ARRAYS:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert (a.mode, a.k, a._valid, a.B, a.H, a.W) == (b.mode, b.k, b._valid, b.B, b.H, b.W)


def _structure_bound(combo, x_cpu, prm, g_cpu):
    """(fp64, fp32) of the block on the membership of ``g_cpu``, dense on the CPU: the fp32 reference's own error is the bound's e_ref32."""
    shape, (variant, gain, mode, k), seed = combo
    member = membership(g_cpu)[0]
    torch.set_num_threads(16)
    with torch.no_grad():
        d64 = _dense_on_structure(x_cpu.double(), {n: t.double() for n, t in prm.items()}, member, mode != "topk", shape)
        d32 = _dense_on_structure(x_cpu, prm, member, mode != "topk", shape)
    return d64, d32


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"{_cid(c[0])}-r{c[1]}")
def test_step_is_refresh_then_forward(case, feat):
    combo, radius = case
    shape, (variant, gain, mode, k), seed = combo
    ce, x = _mod(combo)
    x2 = torch.roll(x, (1, 1), (2, 3))
    g = ce.graph(x)
    want = ce.refresh_graph(x2, g, radius=radius, features=feat)
    out, g2 = ce.step_graph(x2, g, radius=radius, features=feat)
    _same_graph(g2, want)                                                                       # 8.
    assert out.shape == x2.shape[:1] + (16,) + x2.shape[2:] and out.dtype == x2.dtype and not out.requires_grad
    alone, none = ce.step_graph(x2, g, radius=radius, features=feat, want_graph=False)
    assert none is None and torch.equal(alone, out)
    assert torch.equal(ce.step_graph(x2, g, radius=radius, features=feat)[0], out)
    with torch.no_grad():
        two_calls = ce.forward_on_graph(x2, g2, features=feat, fused=False)                    # 9.
    x_cpu, prm = _inputs(seed, shape, variant, gain)
    d64, d32 = _structure_bound(combo, torch.roll(x_cpu, (1, 1), (2, 3)), prm, g2.cpu())
    check_against(f"step_graph vs forward_on_graph {_cid(combo)} radius {radius} {feat}: {g2.n_edges} edges", out, two_calls, d64, d32)
    if variant == "nonepass":
        assert g2.n_edges == 0 and not bool(out.any())


@pytest.mark.parametrize("combo", FIXED_POINT, ids=_cid)
def test_fixed_point_reproduces_the_forward(combo):
    shape, (variant, gain, mode, k), seed = combo
    B, H, W = shape
    ce, x = _mod(combo)
    gap = _gap(_oracle(seed, shape, variant, gain, mode, k), mode, k, H, W)
    assert gap >= 1e-6, "the case must be one the tight bound applies to"
    out, g = ce.step_graph(x, ce.graph(x), radius=1)
    with torch.no_grad():
        err = normwise(out.double().cpu().numpy(), ce(x).double().cpu().numpy())
    print(f"[step] {_cid(combo)} step_graph(x, graph(x)) vs forward(x): {err:.2e} (bound 1e-4, gap {gap:.1e})")
    assert err <= 1e-4


@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[6]], ids=_cid)
def test_three_frames_chained(combo):
    ce, x = _mod(combo)
    frames = [torch.roll(x, (s, s), (2, 3)) for s in (1, 2, 3)]
    a = b = ce.graph(x)
    for f in frames:
        out, a = ce.step_graph(f, a, features="split16")
        b = ce.refresh_graph(f, b, features="split16")
        _same_graph(a, b)
        assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("kind", ["in_channels_32", "half_module"])
def test_other_widths_and_precisions(kind):
    """A 32-channel module and a .half() module (on the fp32 copies of its weights, the half-rounded input), fp32 route.  ``out`` has the
    input's dtype.  The half output is the fp32 one rounded once: two fp32 values within d of each other round to halves within
    d + 2^-10 max|out| (half an ulp of 2^-10 relative on each side)."""
    shape, case = (2, 24, 20), ATOPK16
    variant, gain, mode, k = case
    cin, half = (32, False) if kind == "in_channels_32" else (64, True)
    ce, x = _module(12, shape, variant, gain, mode, k, in_channels=cin, half=half)
    g = ce.graph(x)
    out, g2 = ce.step_graph(x, g, radius=1)
    _same_graph(g2, ce.refresh_graph(x, g, radius=1))
    assert out.dtype == x.dtype == (torch.float16 if half else torch.float32) and out.shape == (2, 16, 24, 20)
    assert g2.weight.dtype == g2.score.dtype == torch.float32
    with torch.no_grad():
        two_calls = ce.forward_on_graph(x, g2, fused=False)
    x0, prm = _inputs(12, shape, variant, gain, cin)
    if half:
        x0, prm = x0.half().float(), {n: t.half().float() for n, t in prm.items()}
    d64, d32 = _structure_bound(((shape, case, 12)), x0, prm, g2.cpu())
    check_against(f"step_graph vs forward_on_graph {kind}", out, two_calls, d64, d32, slack=1e-6 + (2.0 ** -10 if half else 0.0))


def test_capture_of_the_output_alone():
    """On a validated graph whose largest degree has been read, ``want_graph=False`` under ``torch.cuda.graph`` (one stream, no parallel
    branches) replays to the eager bits, also on a new input; the forms that need a host read are refused before any launch and the
    capture stays usable."""
    from dagl_amd import DaglError
    from dagl_amd.graph import PatchGraph
    combo = COMBOS[0]
    ce, x = _mod(combo)
    x2 = torch.roll(x, (1, 1), (2, 3))
    g = ce.graph(x).validate()
    g.max_degree()
    eager2 = ce.step_graph(x2, g, want_graph=False, features="split16")[0].clone()     # (also brings the workspace to its size)
    eager1 = ce.step_graph(x, g, want_graph=False, features="split16")[0].clone()
    assert not torch.equal(eager1, eager2)
    frame = x2.clone()
    unvalidated = PatchGraph(g.row_off, g.key, g.weight, None, *combo[0])
    unvalidated._max_degree = g.max_degree()
    unknown = g.with_weight(g.weight)
    unknown._max_degree = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    refusals = []
    with torch.cuda.graph(graph):
        for bad, kw in ((g, dict(want_graph=True)), (unvalidated, dict(want_graph=False)), (unknown, dict(want_graph=False))):
            with pytest.raises(DaglError) as e:
                ce.step_graph(frame, bad, features="split16", **kw)
            refusals.append(str(e.value))
        captured = ce.step_graph(frame, g, want_graph=False, features="split16")[0]
    assert "captur" in refusals[0] and "validate()" in refusals[1] and "max_degree()" in refusals[2], refusals
    assert not unvalidated._valid and unknown._max_degree is None
    for src, eager in ((x2, eager2), (x, eager1), (x2, eager2)):
        frame.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def test_refusals_leave_the_module_alone():
    from dagl_amd import ops
    from dagl_amd._lib import ERR_UNSUPPORTED, DaglError
    from dagl_amd.graph import PatchGraph
    combo = COMBOS[0]
    shape, (variant, gain, mode, k), seed = combo
    B, H, W = shape
    ce, x = _mod(combo)
    g = ce.graph(x)

    def empty(b, h, w, dev=DEV):
        l = (-(-h // 4)) * (-(-w // 4))
        return PatchGraph(torch.zeros(b * l + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                          torch.empty(0, device=dev), None, b, h, w)
    for want_graph in (True, False):
        kw = dict(want_graph=want_graph)
        for other in ((B, H, W + 4), (B + 1, H, W)):
            _refused(ce, x, lambda: ce.step_graph(x, empty(*other), **kw), "the graph was built for")
        _refused(ce, x, lambda: ce.step_graph(x, g.cpu(), **kw), "lives on cpu")
        _refused(ce, x, lambda: ce.step_graph(x.cpu(), g, **kw), "GPU")
        _refused(ce, x, lambda: ce.step_graph(x[:, :32], g, **kw), "expected [B,64,H,W]")
        _refused(ce, x, lambda: ce.step_graph(x.double(), g, **kw), "dtype")
        _refused(ce, x, lambda: ce.step_graph(x, (g.row_off, g.key), **kw), "PatchGraph")
        _refused(ce, x, lambda: ce.step_graph(x, g, features="fp16", **kw), "features")
        _refused(ce, x, lambda: ce.step_graph(x, g, normalize="rows", **kw), "normalize")
        _refused(ce, x, lambda: ce.step_graph(x, g, radius=9, **kw), "radius")
        _refused(ce, x, lambda: ce.step_graph(x, g, radius=-1, **kw), "radius")

        def without_k():
            ce.select_k = 0
            try:
                ce.step_graph(x, g, **kw)
            finally:
                ce.select_k = k
        _refused(ce, x, without_k, "select_k")

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ce.step_graph(x, g)
    _refused(ce, x, captured, "captur")
    torch.cuda.synchronize()
    # the all-pass graph, 480 keys per query: more candidates than a row may expand into
    cap = ops.graph_refresh_max_candidates()
    wide = _module(11, shape, "allpass", 2.0, "adaptive", 0)[0].graph(x)
    radius = 1 if 480 * 9 > cap else 2
    assert wide.max_degree() == 480 and 480 * (2 * radius + 1) ** 2 > cap
    msg = _refused(ce, x, lambda: ce.step_graph(x, wide, radius=radius), "candidates")
    assert str(480 * (2 * radius + 1) ** 2) in msg and str(cap) in msg and "step_graph" in msg
    with pytest.raises(DaglError) as e:
        ce.step_graph(x, wide, radius=radius, want_graph=False)
    assert e.value.code == ERR_UNSUPPORTED
    assert ce.step_graph(x, g)[1].n_edges == B * 30 * 8                                  # and it still works afterwards


def test_refusal_of_a_generic_geometry():
    from dagl_amd.ce import CE
    from dagl_amd.graph import PatchGraph
    torch.manual_seed(5)
    ce = CE(ksize=5, stride_1=2, stride_2=1, inter_channels=16, in_channels=64).to(DEV).eval()
    x = torch.randn(1, 64, 20, 24, device=DEV)
    g = PatchGraph(torch.zeros(5 * 6 + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                   torch.empty(0, device=DEV), None, 1, 20, 24)
    _refused(ce, x, lambda: ce.step_graph(x, g), "scope")


@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[6], COMBOS[9]], ids=_cid)
def test_the_module_state_is_untouched(combo):
    """What ``forward`` keeps between calls and the ``state_dict`` are as they were after ``step_graph`` on either feature route, with and
    without the graph; the forward returns the same bits; with grad enabled and an input that requires grad the results are constants."""
    mode = combo[1][2]
    ce, x = _mod(combo)
    with torch.no_grad():
        before = ce(x).clone()
        g0 = ce.graph(x)
    tight = ce.topk_policy_is_tight() if mode != "adaptive" else None
    state = (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call)
    params = {n: t.clone() for n, t in ce.state_dict().items()}
    res = [ce.step_graph(x, g0, features=f, want_graph=w) for f in ("fp32", "split16") for w in (True, False)]
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out, g = ce.step_graph(xg, g0)
    assert not out.requires_grad and out.grad_fn is None
    assert not g.weight.requires_grad and not g.score.requires_grad and g.weight.grad_fn is None
    assert torch.equal(out, res[0][0]) and torch.equal(g.key, res[0][1].key) and torch.equal(g.weight, res[0][1].weight)
    assert (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call) == state
    assert all(torch.equal(t, params[n]) for n, t in ce.state_dict().items())
    with torch.no_grad():
        assert torch.equal(ce(x), before)
    if tight is not None:
        assert ce.topk_policy_is_tight() == tight
