"""``ops.graph_step_fixed`` (dagl_graph_step_fixed, csrc/graph_refresh.hip), ``CE.refresh_graph`` / ``CE.step_graph`` on a ``FixedGraph`` and
``CES.step_graphs`` on a fixed ``SequenceState``: the step that hands back its graph at a size known before the launch, so that it reads
nothing on the host and runs under stream capture.

The CSR route defines every result: the rows of the fixed-width output, read back through ``to_csr()``, and ``out`` are held against
``ops.graph_refresh`` / ``graph_step`` / ``graph_search`` / ``graph_search_step`` and the module calls on the CSR under ``torch.equal``."""
import pytest
import torch

from tests import graph_search_reference as SR
from tests.graph_reference import COMBOS, _cid, _geom, _inputs, _mod, _padded
from tests.graph_step_reference import MAX_ROW, SHAPES, apply_references, check_against, crafted, features, value_map, without_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
ARRAYS = ("row_off", "key", "weight", "score")
KEEP_ALL, BLOCK_ROWS, EDGES_ONLY = 0x2, 0x4, 0x1


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _fixed_of(row_off, key, shape, width):
    """The (row_off, key) of a crafted graph as a ``FixedGraph`` of ``width`` slots on the device."""
    from dagl_amd import PatchGraph
    return PatchGraph(row_off, key, torch.zeros(key.numel()), None, *shape).to_fixed(width).to(DEV)


def _raw(shape, wq, x, b2p, key, deg, tau, width_out, radius=1, k=0, flags=0, propagate=0, explore=0, seed=0):
    """The C entry on output arrays pre-filled with garbage and a workspace filled with 0x5B (6.2e16 as a float): a slot, a degree or an
    aggregated row that no exit of the kernel writes shows in the result -> (out | None, FixedGraph, status)."""
    from dagl_amd import FixedGraph, _lib
    lib = _lib.load()
    B, H, W, L, N = _geom(shape)
    rows = B * L
    key_out = torch.full((rows, width_out), 0x5B5B5B5B, dtype=torch.int32, device=DEV)
    weight = torch.full((rows, width_out), 6.2e16, device=DEV)
    score = torch.full((rows, width_out), -6.2e16, device=DEV)
    deg_out = torch.full((rows,), 12345, dtype=torch.int32, device=DEV)
    status = torch.full((2,), 99, dtype=torch.int64, device=DEV)
    out = torch.full((B, 16, H, W), 7e16, device=DEV) if b2p is not None else None
    need = lib.dagl_graph_step_fixed_workspace_bytes(B, H, W, 1 if b2p is not None else 0)
    assert (need > 0) == (b2p is not None)
    buf = torch.full((need + 256,), 0x5B, dtype=torch.uint8, device=DEV)
    ws = (buf.data_ptr() + 255) // 256 * 256
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = lib.dagl_graph_step_fixed(torch.cuda.current_stream().cuda_stream, B, H, W, wq.data_ptr(), x.data_ptr(), ptr(b2p), key.data_ptr(),
                                   deg.data_ptr(), key.shape[1], radius, ptr(tau), k, SCALE, flags, propagate, explore, seed, ptr(out),
                                   key_out.data_ptr(), weight.data_ptr(), score.data_ptr(), deg_out.data_ptr(), width_out,
                                   status.data_ptr(), ws if need else None, need)
    assert rc == 0, lib.dagl_last_error()
    torch.cuda.synchronize()
    del buf
    return out, FixedGraph(key_out, weight, score, deg_out, *shape), status


def _assert_filler(f):
    live = torch.arange(f.width, device=f.key.device)[None, :] < f.deg[:, None]
    assert bool(((f.deg >= 0) & (f.deg <= f.width)).all())
    assert bool((f.key[~live] == -1).all()) and not bool(f.weight[~live].any()) and not bool(f.score[~live].any())
    assert bool((f.key[live] >= 0).all())


def _assert_rows(f, want, what):
    """``f.to_csr()``'s arrays are the CSR dict's, bit for bit."""
    back = f.to_csr()
    for n in ARRAYS:
        assert torch.equal(getattr(back, n), want[n]), (what, n)


# ---- 1. the kernel against the CSR entries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_kernel_against_the_csr_entries(shape, radius):
    """12 slots per row: radius 0 / 1 run a wavefront per row (12 / 108 candidates), radius 2 a block (300); each once more with
    ``block_rows``.  ``width_out`` 3 (= k) and 5 (room to spare)."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    row_off, key = crafted(shape)
    wq, x, tau = (t.to(DEV) for t in features(shape))
    b2p = _padded(value_map(shape)).to(DEV)
    off_dev, key_dev = row_off.to(DEV), key.to(DEV)
    fixed = _fixed_of(row_off, key, shape, MAX_ROW)
    assert fixed.width == MAX_ROW
    for name, with_tau in (("k3", False), ("tau_k3", True)):
        t = tau if with_tau else None
        for block_rows in (False, True):
            kw = dict(radius=radius, tau=t, k=3, scale=SCALE, max_row_edges=MAX_ROW, block_rows=block_rows)
            want = ops.graph_refresh(wq, x, off_dev, key_dev, hw=(H, W), **kw)
            want_out = ops.graph_step(wq, x, b2p, off_dev, key_dev, **kw)[0]
            for width_out in (3, 5):
                what = f"{shape} radius {radius} {name} block_rows {block_rows} width_out {width_out}"
                flags = BLOCK_ROWS if block_rows else 0
                for value_map_given in (True, False):
                    out, f, status = _raw(shape, wq, x, b2p if value_map_given else None, fixed.key, fixed.deg, t, width_out, radius, 3, flags)
                    assert status.tolist()[0] == 0 and 0 < status.tolist()[1] <= MAX_ROW * (2 * radius + 1) ** 2, what
                    _assert_filler(f)
                    _assert_rows(f, want, what)
                    assert (out is None) == (not value_map_given)
                    if value_map_given:
                        assert torch.equal(out, want_out), what
                # the Python entry: the same arrays
                out, arrays, status = ops.graph_step_fixed(wq, x, b2p, fixed.key, fixed.deg, width_out=width_out, radius=radius, tau=t, k=3,
                                                           scale=SCALE, block_rows=block_rows)
                assert torch.equal(out, want_out) and status.tolist()[0] == 0
                for n in ("key", "weight", "score", "deg"):
                    assert torch.equal(arrays[n], getattr(f, n)), (what, n)
                none, arrays, _ = ops.graph_step_fixed(wq, x, None, fixed.key, fixed.deg, width_out=width_out, radius=radius, tau=t, k=3,
                                                       scale=SCALE, block_rows=block_rows, hw=(H, W))
                assert none is None and torch.equal(arrays["key"], f.key) and torch.equal(arrays["weight"], f.weight)


# ---- 2. the search flavour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 21])
@pytest.mark.parametrize("sources", [(True, 0), (False, 8), (True, 8)], ids=lambda s: f"p{int(s[0])}e{s[1]}")
def test_search_flavour_against_the_csr_entries(sources, seed):
    """(2,24,20) holds a grid-row end (rows Lw - 1, Lw) and the image boundary of a batch of two (rows L - 1, L)."""
    from dagl_amd import ops
    propagate, explore = sources
    shape = (2, 24, 20)
    B, H, W, L, N = _geom(shape)
    row_off, key = SR.crafted(shape)
    wq, x, tau = (t.to(DEV) for t in SR.features(shape))
    b2p = _padded(value_map(shape)).to(DEV)
    off_dev, key_dev = row_off.to(DEV), key.to(DEV)
    fixed = _fixed_of(row_off, key, shape, SR.MAX_ROW)
    for t in (None, tau):
        kw = dict(radius=1, tau=t, k=3, scale=SCALE, max_row_edges=SR.MAX_ROW, propagate=propagate, explore=explore, seed=seed)
        want = ops.graph_search(wq, x, off_dev, key_dev, hw=(H, W), **kw)
        want_out = ops.graph_search_step(wq, x, b2p, off_dev, key_dev, **kw)[0]
        for flags in (0, BLOCK_ROWS):
            what = f"propagate {propagate} explore {explore} seed {seed} tau {t is not None} flags {flags}"
            out, f, status = _raw(shape, wq, x, b2p, fixed.key, fixed.deg, t, 3, 1, 3, flags, int(propagate), explore, seed)
            assert status.tolist()[0] == 0, what
            _assert_filler(f)
            _assert_rows(f, want, what)
            assert torch.equal(out, want_out), what
            none, f2, _ = _raw(shape, wq, x, None, fixed.key, fixed.deg, t, 3, 1, 3, flags, int(propagate), explore, seed)
            assert none is None and all(torch.equal(getattr(f2, n), getattr(f, n)) for n in ("key", "weight", "score", "deg")), what
        out, arrays, _ = ops.graph_step_fixed(wq, x, b2p, fixed.key, fixed.deg, width_out=3, radius=1, tau=t, k=3, scale=SCALE,
                                              propagate=propagate, explore=explore, seed=seed)
        assert torch.equal(out, want_out) and torch.equal(arrays["key"], f.key) and torch.equal(arrays["deg"], f.deg)


# ---- 3. the overflow rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", ["tau", "keep_all"])
def test_a_row_that_overflows_comes_out_empty(selection):
    """No rank cut: a row may keep more than ``width_out``.  It leaves EMPTY and counted, never truncated; every other row is the CSR's."""
    from dagl_amd import PatchGraph, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    row_off, key = crafted(shape)
    wq, x, tau = (t.to(DEV) for t in features(shape))
    b2p = _padded(value_map(shape)).to(DEV)
    fixed = _fixed_of(row_off, key, shape, MAX_ROW)
    keep_all = selection == "keep_all"
    t = None if keep_all else tau
    want = ops.graph_refresh(wq, x, row_off.to(DEV), key.to(DEV), hw=(H, W), radius=1, tau=t, k=0, scale=SCALE, keep_all=keep_all,
                             max_row_edges=MAX_ROW)
    deg = (want["row_off"][1:] - want["row_off"][:-1]).cpu()
    width_out = max(int(deg[deg > 0].float().median()), 1)
    over = deg > width_out
    assert bool(over.any()) and bool(((deg > 0) & ~over).any()), (width_out, deg.tolist())
    out, f, status = _raw(shape, wq, x, b2p, fixed.key, fixed.deg, t, width_out, 1, 0, KEEP_ALL if keep_all else 0)
    assert status.tolist()[0] == int(over.sum())
    _assert_filler(f)
    assert not bool(f.deg.cpu()[over].any())
    wide = PatchGraph(*(want[n].cpu() for n in ARRAYS), *shape).to_fixed(int(deg.max()))
    wide.key[over], wide.weight[over], wide.score[over], wide.deg[over] = -1, 0.0, 0.0, 0
    for n in ("key", "weight", "score"):
        assert torch.equal(getattr(f, n).cpu(), getattr(wide, n)[:, :width_out].contiguous()), n
    assert torch.equal(f.deg.cpu(), wide.deg)
    gone = torch.nonzero(over).flatten().tolist()
    left = without_rows(want["row_off"].cpu(), want["key"].cpu(), want["weight"].cpu(), gone)
    ref64, ref32 = apply_references(*left, shape)
    check_against(f"fixed step out, {len(gone)} overflowing rows left out ({selection}, width_out {width_out})", out,
                  ops.graph_apply(b2p, *(a.to(DEV) for a in left)), ref64, ref32)
    # with room for the longest row nothing overflows and the CSR comes back whole
    out, f, status = _raw(shape, wq, x, b2p, fixed.key, fixed.deg, t, int(deg.max()), 1, 0, KEEP_ALL if keep_all else 0)
    assert status.tolist()[0] == 0
    _assert_rows(f, want, selection)


# ---- 4. degenerate inputs ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    from dagl_amd import ops
    from dagl_amd.graph import trivial_graph
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    row_off, key = crafted(shape)
    wq, x, tau = (t.to(DEV) for t in features(shape))
    b2p = _padded(value_map(shape)).to(DEV)
    fixed = _fixed_of(row_off, key, shape, MAX_ROW)
    # every degree 0: zeros out, degree 0, filler;  with explore = 8 the rows populate as the empty CSR's do
    none = torch.zeros_like(fixed.deg)
    for flags in (0, BLOCK_ROWS):
        out, f, status = _raw(shape, wq, x, b2p, fixed.key, none, tau, 3, 1, 3, flags)
        assert not bool(out.any()) and not bool(f.deg.any()) and status.tolist() == [0, 0]
        _assert_filler(f)
    empty_off, empty_key = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)
    want = ops.graph_search(wq, x, empty_off, empty_key, hw=(H, W), radius=1, k=3, scale=SCALE, max_row_edges=0, explore=8, seed=4)
    out, f, status = _raw(shape, wq, x, b2p, fixed.key, none, None, 3, 1, 3, 0, 0, 8, 4)
    assert bool((f.deg > 0).all()) and status.tolist()[0] == 0
    _assert_rows(f, want, "explore on an empty graph")
    assert torch.equal(out, ops.graph_search_step(wq, x, b2p, empty_off, empty_key, radius=1, k=3, scale=SCALE, max_row_edges=0, explore=8,
                                                  seed=4)[0])
    # degrees outside [0, width]: clamped, no slot outside the row read (row 9's keys follow row 8's slots)
    odd = _fixed_of(row_off, key, shape, MAX_ROW)
    odd.deg[3], odd.deg[8] = -3, MAX_ROW + 5
    clamped = odd.to_csr()
    assert int(clamped.row_off[4] - clamped.row_off[3]) == 0 and int(clamped.row_off[9] - clamped.row_off[8]) == MAX_ROW
    for radius in (1, 2):
        want = ops.graph_refresh(wq, x, clamped.row_off, clamped.key, hw=(H, W), radius=radius, tau=tau, k=3, scale=SCALE,
                                 max_row_edges=MAX_ROW)
        out, f, status = _raw(shape, wq, x, b2p, odd.key, odd.deg, tau, 3, radius, 3)
        assert status.tolist()[0] == 0 and int(f.deg[3]) == 0
        _assert_rows(f, want, f"clamped degrees, radius {radius}")
    # one slot in, one slot out
    one = trivial_graph(B, H, W, DEV).to_fixed()
    assert one.width == 1
    csr = one.to_csr()
    want = ops.graph_refresh(wq, x, csr.row_off, csr.key, hw=(H, W), radius=1, k=1, scale=SCALE, max_row_edges=1)
    out, f, status = _raw(shape, wq, x, b2p, one.key, one.deg, None, 1, 1, 1)
    assert f.width == 1 and bool((f.deg == 1).all()) and status.tolist()[0] == 0
    _assert_rows(f, want, "width 1")
    assert torch.equal(out, ops.graph_step(wq, x, b2p, csr.row_off, csr.key, radius=1, k=1, scale=SCALE, max_row_edges=1)[0])


# ---- 5. the module -------------------------------------------------------------------------------------------------------------------------
def _same_as_csr(f, g, ce):
    from dagl_amd import FixedGraph
    assert isinstance(f, FixedGraph) and (f.mode, f.k, f.B, f.H, f.W) == (g.mode, g.k, g.B, g.H, g.W) and f.mode == ce.select_mode
    back = f.to_csr()
    for n in ARRAYS:
        assert torch.equal(getattr(back, n), getattr(g, n)), n
    _assert_filler(f)


# top-k 8, adaptive AND top-16, adaptive (largest degree 10 in 16 slots)
MODULE_CASES = [(COMBOS[0], None), (COMBOS[6], None), (COMBOS[11], 16)]


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: _cid(c[0]))
def test_module_step_and_refresh(case, feat):
    combo, width = case
    mode, k = combo[1][2], combo[1][3]
    ce, x = _mod(combo)
    x2 = torch.roll(x, (1, 1), (2, 3))
    g = ce.graph(x)
    fixed = g.to_fixed(width)
    want_out, want = ce.step_graph(x2, g, features=feat)
    out, f = ce.step_graph(x2, fixed, features=feat)
    _same_as_csr(f, want, ce)
    assert f.width == (k if mode != "adaptive" else width)
    assert torch.equal(out, want_out) and out.dtype == x2.dtype and not out.requires_grad
    alone, none = ce.step_graph(x2, fixed, features=feat, want_graph=False)
    assert none is None and torch.equal(alone, want_out)
    _same_as_csr(ce.refresh_graph(x2, fixed, features=feat), ce.refresh_graph(x2, g, features=feat), ce)


def test_module_search_keywords():
    ce, x = _mod(COMBOS[0])
    x2 = torch.roll(x, (2, 1), (2, 3))
    g = ce.graph(x)
    kw = dict(propagate=True, explore=8, seed=5)
    want_out, want = ce.step_graph(x2, g, **kw)
    out, f = ce.step_graph(x2, g.to_fixed(), **kw)
    _same_as_csr(f, want, ce)
    assert torch.equal(out, want_out)
    _same_as_csr(ce.refresh_graph(x2, g.to_fixed(), **kw), ce.refresh_graph(x2, g, **kw), ce)


@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[6]], ids=_cid)
def test_three_frames_chained(combo):
    """Rank-cut modes: no row can overflow, so the fixed chain is the CSR chain frame after frame."""
    ce, x = _mod(combo)
    a = ce.graph(x)
    b = a.to_fixed()
    for s in (1, 2, 3):
        frame = torch.roll(x, (s, s), (2, 3))
        out_a, a = ce.step_graph(frame, a, features="split16")
        out_b, b = ce.step_graph(frame, b, features="split16")
        _same_as_csr(b, a, ce)
        assert torch.equal(out_a, out_b)


def test_adaptive_fixed_point():
    """``COMBOS[9]`` (adaptive, largest degree 59) on the input its graph came from, in 64 slots: the step reproduces ``CE.graph``'s
    structure, as it does on the CSR, and no row overflows."""
    from dagl_amd import ops
    combo = COMBOS[9]
    ce, x = _mod(combo)
    g = ce.graph(x)
    assert g.max_degree() <= 64
    fixed = g.to_fixed(64)
    out, f = ce.step_graph(x, fixed)
    want_out, want = ce.step_graph(x, g)
    _same_as_csr(f, want, ce)
    assert torch.equal(out, want_out)
    back = f.to_csr()
    assert torch.equal(back.row_off, g.row_off) and torch.equal(back.key, g.key)
    with torch.no_grad():
        wq_rows, x_rows, tau, b2p, _ = ce._graph_features(x, True, False, False)
        _, arrays, status = ops.graph_step_fixed(wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous(), fixed.key, fixed.deg, width_out=64,
                                                 radius=1, tau=tau.contiguous(), scale=float(ce.softmax_scale))
    assert status.tolist()[0] == 0 and torch.equal(arrays["key"], f.key) and torch.equal(arrays["weight"], f.weight)


def test_module_refusals_come_before_any_launch():
    from dagl_amd import DaglError, _lib
    ce, x = _mod(COMBOS[0])
    f = ce.graph(x).to_fixed()
    for call in (ce.apply_graph, ce.attend_graph, ce.forward_on_graph):
        with pytest.raises(DaglError, match=r"\.to_csr\(\)"):
            call(x, f)
    for bad, word in ((f.images(0, 1), "B=1"), (f.cpu(), "lives on")):
        for call in (ce.step_graph, ce.refresh_graph):
            with pytest.raises(DaglError, match=word):
                call(x, bad)
    with pytest.raises(DaglError, match="radius"):
        ce.step_graph(x, f, radius=9)
    with pytest.raises(DaglError, match="explore=300"):
        ce.step_graph(x, f, explore=300)
    with pytest.raises(DaglError, match="candidates") as e:                     # 8 slots at radius 8: 5 * 8 * 289 + 8 candidates
        ce.step_graph(x, f, radius=8, propagate=True, explore=8)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------------------
def test_capture_of_the_step_with_its_graph():
    """One stream, one eager warm-up.  ``out, g_new = ce.step_graph(x, g); g.copy_(g_new)`` captured once and replayed over three frames
    gives the eager chain's output and graph after every replay: the graph follows the frames inside the HIP graph."""
    ce, x0 = _mod(COMBOS[0])
    frames = [torch.roll(x0, (s, s), (2, 3)) for s in (1, 2, 3)]
    start = ce.graph(x0).to_fixed()
    chain, g = [], start
    for frame in frames:                                                        # the eager chain (and the warm-up)
        out, g = ce.step_graph(frame, g, features="split16")
        chain.append((out.clone(), g))
    x = frames[0].clone()
    g = start._like(start.key.clone(), start.weight.clone(), start.score.clone(), start.deg.clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert torch.cuda.is_current_stream_capturing()
        out, g_new = ce.step_graph(x, g, features="split16")                    # want_graph=True: no refusal, no host read
        g.copy_(g_new)
    assert not torch.cuda.is_current_stream_capturing()
    for frame, (want_out, want_g) in zip(frames, chain):
        x.copy_(frame)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out)
        for n in ("key", "weight", "score", "deg"):
            assert torch.equal(getattr(g, n), getattr(want_g, n)), n
    assert (g.mode, g.k) == (ce.select_mode, 8)


def _ces(case, shape):
    """A ``CES`` whose twelve heads carry seeded parameters of ``case``, and a seeded input."""
    from dagl_amd.net import CES
    variant, gain, mode, k = case
    torch.manual_seed(3)
    ces = CES(64)
    for i, (s, h) in enumerate((s, h) for s in (1, 2, 3) for h in (1, 2, 3, 4)):
        hd = getattr(ces, f"c{s}_{h}")
        hd.load_state_dict(_inputs(11 + i, shape, variant, gain)[1], strict=True)
        hd.select_mode, hd.select_k = mode, k
    return ces.to(DEV).eval(), _inputs(11, shape, variant, gain)[0].to(DEV)


def test_capture_of_a_whole_ces():
    """``CES.step_graphs`` on a fixed ``SequenceState`` under capture with ``state.copy_(new_state)``, against the eager head-by-head call
    on the CSR state: the same output, the same graphs."""
    from dagl_amd import DaglError
    from dagl_amd.sequence import SequenceState
    shape = (1, 24, 20)
    ces, x0 = _ces(COMBOS[0][1], shape)
    with torch.no_grad():
        _, key_state = ces.forward_with_graphs(x0)
    frames = [torch.roll(x0, (s, s), (2, 3)) for s in (1, 2)]
    chain, st = [], key_state
    for frame in frames:
        out, st = ces.step_graphs(frame, st, fused=False)
        chain.append((out.clone(), st))
    start = key_state.to_fixed(8)                                               # (top-k 8: the width every step gives back)
    with pytest.raises(DaglError, match="fused=True"):
        ces.step_graphs(frames[0], start, fused=True)
    warm, warm_state = ces.step_graphs(frames[0], start)                        # eager, and the warm-up
    assert torch.equal(warm, chain[0][0]) and warm_state.fixed
    state = SequenceState(g._like(g.key.clone(), g.weight.clone(), g.score.clone(), g.deg.clone()) for g in start.stages)
    x = frames[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, new_state = ces.step_graphs(x, state)
        state.copy_(new_state)
    for frame, (want_out, want_state) in zip(frames, chain):
        x.copy_(frame)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out)
        back = state.to_csr()
        for s in range(3):
            for n in ARRAYS:
                assert torch.equal(getattr(back.stages[s], n), getattr(want_state.stages[s], n)), (s, n)


# ---- 7. the module's state -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[6], COMBOS[9]], ids=_cid)
def test_the_module_state_is_untouched(combo):
    mode = combo[1][2]
    ce, x = _mod(combo)
    with torch.no_grad():
        before = ce(x).clone()
        f0 = ce.graph(x).to_fixed(64 if mode == "adaptive" else None)
    tight = ce.topk_policy_is_tight() if mode != "adaptive" else None
    state = (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call)
    params = {n: t.clone() for n, t in ce.state_dict().items()}
    res = [ce.step_graph(x, f0, features=f, want_graph=w) for f in ("fp32", "split16") for w in (True, False)]
    ce.refresh_graph(x, f0)
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out, g = ce.step_graph(xg, f0)
    assert not out.requires_grad and out.grad_fn is None
    assert not g.weight.requires_grad and not g.score.requires_grad and g.weight.grad_fn is None
    assert torch.equal(out, res[0][0]) and torch.equal(g.key, res[0][1].key) and torch.equal(g.weight, res[0][1].weight)
    assert (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call) == state
    assert all(torch.equal(t, params[n]) for n, t in ce.state_dict().items())
    with torch.no_grad():
        assert torch.equal(ce(x), before)
    if tight is not None:
        assert ce.topk_policy_is_tight() == tight
