"""``ops.graph_stage_step_fixed`` (dagl_graph_stage_step_fixed, csrc/graph_refresh.hip) and the module route on it:
``CES.step_graphs(x, fixed_state, fused="stage")`` and ``CES.search_graphs`` on a fixed ``SequenceState`` (dagl_amd/net.py).

The op is held EXACTLY against four single-head calls (``ops.graph_step_fixed`` on head h's operands and its rows of the stage's graph,
whose own tests hold it against the CSR entries): every output array is the concatenation of the heads' arrays bit for bit, filler
included, the status words their sum and maximum, and ``out`` is ``ops.ces_stage_fold_mix`` of the four calls' aggregated rows (read out
of those calls' workspaces, where they come first), also bit for bit.  The stage call runs on output arrays pre-filled with garbage and
a workspace filled with 0x5B, so a slot, a degree or an aggregated row that no exit of the kernel writes shows.

The module route is held against the head-by-head fixed call with the scheme of test_gpu_ces_step_graphs.py (exact graphs on one stage
input; that file's bounds on whole calls) and, bit for bit, against the stage-fused call on the CSR state: the same row body, the same
fold + mix kernel, no overflow in the rank-cut modes."""
import functools

import pytest
import torch

from tests.graph_reference import ATOPK16, TOPK8, _check, _geom
from tests.graph_search_reference import MAX_ROW, crafted
from tests.test_gpu_ces_step_graphs import _assert_state, _build, _cid, _key_state, _module_state, _nw
from tests.test_gpu_graph_stage_search import HEAD_SEEDS, _agg_rows, _mix_refs, _stage_of
from tests.test_gpu_graph_step_fixed import _assert_filler, _fixed_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
SHAPES = [(2, 24, 20), (1, 23, 30)]           # the first: a grid-row end and an image boundary inside each head
ARRAYS = ("key", "weight", "score", "deg")
CSR_ARRAYS = ("row_off", "key", "weight", "score")
KEEP_ALL, BLOCK_ROWS = 0x2, 0x4
MODULE_SHAPE = (1, 24, 20)


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _stage(shape):
    """Head h's crafted graph, banded features and value map, each from a seed of its own (``_stage_of``'s scheme) -> (heads, the
    stage's slot array [4 B L, MAX_ROW], its degrees [4 B L], the mix operands).  Shared by the tests and left unchanged."""
    from dagl_amd import FixedGraph
    heads, _, _, mix = _stage_of(shape, [crafted(shape, gs) for gs, _, _ in HEAD_SEEDS])
    fixed = FixedGraph.cat([_fixed_of(h["cpu_off"], h["cpu_key"], shape, MAX_ROW) for h in heads])
    return heads, fixed.key, fixed.deg, mix


def _raw(shape, heads, mix, key, deg, width_out, step=True, with_tau=False, radius=1, k=0, flags=0, propagate=0, explore=0, seed=0):
    """The C entry on output arrays pre-filled with garbage and a workspace filled with 0x5B -> (out | None, arrays, status, the
    aggregated rows [4 B L, 784] | None)."""
    import ctypes as C
    from dagl_amd import _lib
    lib = _lib.load()
    B, H, W, L, N = _geom(shape)
    rows = 4 * B * L
    res = dict(key=torch.full((rows, width_out), 0x5B5B5B5B, dtype=torch.int32, device=DEV), weight=torch.full((rows, width_out), 6.2e16, device=DEV),
               score=torch.full((rows, width_out), -6.2e16, device=DEV), deg=torch.full((rows,), 12345, dtype=torch.int32, device=DEV))
    status = torch.full((2,), 99, dtype=torch.int64, device=DEV)
    out = torch.full((B, 64, H, W), 7e16, device=DEV) if step else None
    need = lib.dagl_graph_stage_step_fixed_workspace_bytes(B, H, W, 1 if step else 0)
    assert (need > 0) == step
    buf = torch.full((need + 256,), 0x5B, dtype=torch.uint8, device=DEV)
    ws = (buf.data_ptr() + 255) // 256 * 256
    table = lambda name: (C.c_void_p * 4)(*[h[name].data_ptr() for h in heads])
    ptr = lambda t: t.data_ptr() if step else None
    rc = lib.dagl_graph_stage_step_fixed(torch.cuda.current_stream().cuda_stream, B, H, W, table("wq"), table("x"), table("b2p") if step else None,
                                         key.data_ptr(), deg.data_ptr(), key.shape[1], radius, table("tau") if with_tau else None, k, SCALE,
                                         flags, propagate, explore, seed, ptr(mix["x"]), ptr(mix["mix_w"]), ptr(mix["mix_b"]),
                                         out.data_ptr() if step else None, res["key"].data_ptr(), res["weight"].data_ptr(),
                                         res["score"].data_ptr(), res["deg"].data_ptr(), width_out, status.data_ptr(), ws if need else None,
                                         need)
    assert rc == 0, lib.dagl_last_error()
    torch.cuda.synchronize()
    agg = buf[ws - buf.data_ptr():ws - buf.data_ptr() + rows * 784 * 4].view(torch.float32).view(rows, 784).clone() if step else None
    del buf
    return out, res, status, agg


def _head_calls(shape, heads, key, deg, width_out, with_tau=False, radius=1, k=0, flags=0, propagate=0, explore=0, seed=0):
    """The four single-head calls on head h's operands and its rows of (key, deg) -> [(arrays, status, aggregated rows [B L, 784])]."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    n = B * L
    res = []
    for h, hd in enumerate(heads):
        ws = ops.Workspace()
        _, arrays, status = ops.graph_step_fixed(hd["wq"], hd["x"], hd["b2p"], key[h * n:(h + 1) * n], deg[h * n:(h + 1) * n], width_out=width_out,
                                                 radius=radius, tau=hd["tau"] if with_tau else None, k=k, scale=SCALE,
                                                 keep_all=bool(flags & KEEP_ALL), block_rows=bool(flags & BLOCK_ROWS),
                                                 propagate=bool(propagate), explore=explore, seed=seed, workspace=ws)
        res.append((arrays, status, _agg_rows(ws, n)))
    return res


def _against_heads(shape, heads, mix, key, deg, width_out, what, **kw):
    """The stage call, with and without the value operands, against the four single-head calls -> (arrays, status, out, per head)."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    per_head = _head_calls(shape, heads, key, deg, width_out, **kw)
    out, arrays, status, agg = _raw(shape, heads, mix, key, deg, width_out, True, **kw)
    for name in ARRAYS:
        assert torch.equal(arrays[name], torch.cat([a[name] for a, _, _ in per_head])), (what, name)
    assert status.tolist() == [sum(int(st[0]) for _, st, _ in per_head), max(int(st[1]) for _, st, _ in per_head)], what
    assert torch.equal(agg, torch.cat([rows for _, _, rows in per_head])), what
    want_out = ops.ces_stage_fold_mix(torch.stack([rows.view(B, L, 784) for _, _, rows in per_head]).contiguous(), mix["x"], mix["mix_w"],
                                      mix["mix_b"])
    assert out.shape == (B, 64, H, W) and torch.equal(out, want_out), what
    # the graph alone: all value operands null
    none, alone, status_alone, _ = _raw(shape, heads, mix, key, deg, width_out, False, **kw)
    assert none is None and status_alone.tolist() == status.tolist(), what
    for name in ARRAYS:
        assert torch.equal(alone[name], arrays[name]), (what, name, "graph alone")
    return arrays, status, out, per_head


def _as_graph(arrays, shape):
    from dagl_amd import FixedGraph
    return FixedGraph(arrays["key"], arrays["weight"], arrays["score"], arrays["deg"], 4 * shape[0], *shape[1:])


# ---- 1. the op against four single-head calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_against_four_single_head_calls(shape, radius):
    """12 slots per row: radius 0 / 1 run a wavefront per row (12 / 108 candidates), radius 2 a block (300); each once more with
    ``block_rows``.  k = 3 with and without ``tau``; ``width_out`` 3 (= k) and 5 (room to spare)."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    heads, key, deg, mix = _stage(shape)
    for with_tau in (False, True):
        for flags in (0, BLOCK_ROWS):
            for width_out in (3, 5):
                what = f"{shape} radius {radius} tau {with_tau} flags {flags} width_out {width_out}"
                arrays, status, out, _ = _against_heads(shape, heads, mix, key, deg, width_out, what, with_tau=with_tau, radius=radius, k=3,
                                                        flags=flags)
                assert status.tolist()[0] == 0 and 0 < status.tolist()[1] <= MAX_ROW * (2 * radius + 1) ** 2, what
                _assert_filler(_as_graph(arrays, shape))
                assert 0 < int(arrays["deg"].max()) <= 3
            # the Python entry: the same arrays, with and without the value operands
            kw = dict(width_out=3, radius=radius, tau4=[h["tau"] for h in heads] if with_tau else None, k=3, scale=SCALE,
                      block_rows=bool(flags))
            arrays3 = _raw(shape, heads, mix, key, deg, 3, True, with_tau=with_tau, radius=radius, k=3, flags=flags)
            got_out, got, got_status = ops.graph_stage_step_fixed([h["wq"] for h in heads], [h["x"] for h in heads], [h["b2p"] for h in heads],
                                                                  key, deg, mix["x"], mix["mix_w"], mix["mix_b"], **kw)
            assert torch.equal(got_out, arrays3[0]) and got_status.tolist() == arrays3[2].tolist()
            none, alone, _ = ops.graph_stage_step_fixed([h["wq"] for h in heads], [h["x"] for h in heads], None, key, deg, hw=(H, W), **kw)
            assert none is None
            for name in ARRAYS:
                assert torch.equal(got[name], arrays3[1][name]) and torch.equal(alone[name], arrays3[1][name]), name


# ---- 2. the search flavour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 21])
@pytest.mark.parametrize("sources", [(1, 0), (0, 8), (1, 8)], ids=lambda s: f"p{s[0]}e{s[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_search_flavour_against_four_single_head_calls(shape, sources, seed):
    """Propagation reads rows r +- 1 and r +- Lw of the STAGE's input inside the row's image: never across a grid-row end, an image or a
    head.  The random keys are hashed from the head-local row: a head's rows are the single-head call's."""
    propagate, explore = sources
    heads, key, deg, mix = _stage(shape)
    for with_tau in (False, True):
        for flags in (0, BLOCK_ROWS):
            what = f"{shape} propagate {propagate} explore {explore} seed {seed} tau {with_tau} flags {flags}"
            arrays, status, _, _ = _against_heads(shape, heads, mix, key, deg, 3, what, with_tau=with_tau, radius=1, k=3, flags=flags,
                                                  propagate=propagate, explore=explore, seed=seed)
            assert status.tolist()[0] == 0, what
            _assert_filler(_as_graph(arrays, shape))


# ---- 3. the overflow rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_rows_that_overflow_come_out_empty(shape):
    """No rank cut, ``width_out`` at the median degree: a row of any head that keeps more leaves EMPTY and counted, never truncated;
    every other row is the single-head result."""
    B, H, W, L, N = _geom(shape)
    heads, key, deg, mix = _stage(shape)
    kw = dict(with_tau=True, radius=1, k=0)
    wide = torch.cat([a["deg"] for a, _, _ in _head_calls(shape, heads, key, deg, MAX_ROW * 9, **kw)]).cpu()
    width_out = max(int(wide[wide > 0].float().median()), 1)
    over = wide > width_out
    assert bool(over.any()) and bool(((wide > 0) & ~over).any()), (width_out, wide.tolist())
    n = B * L
    assert sum(bool(over[h * n:(h + 1) * n].any()) for h in range(4)) >= 2, "rows of more than one head must overflow"
    arrays, status, out, per_head = _against_heads(shape, heads, mix, key, deg, width_out, f"overflow {shape}", **kw)
    assert status.tolist()[0] == int(over.sum()) == sum(int(st[0]) for _, st, _ in per_head)
    _assert_filler(_as_graph(arrays, shape))
    got = arrays["deg"].cpu()
    assert not bool(got[over].any()) and torch.equal(got[~over], wide[~over].to(torch.int32))
    assert bool((arrays["key"][over.to(DEV)] == -1).all())
    # with room for the longest row nothing overflows
    arrays, status, _, _ = _against_heads(shape, heads, mix, key, deg, int(wide.max()), f"no overflow {shape}", **kw)
    assert status.tolist()[0] == 0 and torch.equal(arrays["deg"].cpu(), wide.to(torch.int32))


# ---- 4. degenerate inputs ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    from dagl_amd import FixedGraph
    from dagl_amd.graph import trivial_graph
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    n = B * L
    heads, key, deg, mix = _stage(shape)
    # every degree 0: degree 0 and filler everywhere, zeros aggregated, out = mix_b + x
    none = torch.zeros_like(deg)
    for flags in (0, BLOCK_ROWS):
        arrays, status, out, _ = _against_heads(shape, heads, mix, key, none, 3, "all degrees 0", with_tau=True, radius=1, k=3, flags=flags)
        assert not bool(arrays["deg"].any()) and status.tolist() == [0, 0]
        _assert_filler(_as_graph(arrays, shape))
        assert torch.equal(out, mix["mix_b"].view(1, 64, 1, 1) + mix["x"])
    # explore = 8 on the empty stage: every row populates, the four heads from the same hashed keys
    for propagate in (0, 1):
        arrays, status, out, _ = _against_heads(shape, heads, mix, key, none, 3, "explore on an empty stage", radius=1, k=3,
                                                propagate=propagate, explore=8, seed=4)
        assert bool((arrays["deg"] == 3).all()) and status.tolist()[0] == 0
        assert not torch.equal(out, mix["mix_b"].view(1, 64, 1, 1) + mix["x"])
    # degrees outside [0, width] in the last row of head 1 and the first row of head 2: clamped, and -- the single-head calls see only
    # their own head's rows -- no slot of the neighbouring head is read, with propagation on either
    odd = deg.clone()
    odd[2 * n - 1], odd[2 * n] = MAX_ROW + 5, -3
    for propagate, radius in ((0, 1), (1, 1), (0, 2), (1, 0)):
        arrays, status, _, _ = _against_heads(shape, heads, mix, key, odd, 3, f"odd degrees propagate {propagate} radius {radius}",
                                              with_tau=True, radius=radius, k=3, propagate=propagate)
        assert status.tolist()[0] == 0
        _assert_filler(_as_graph(arrays, shape))
    full, empty = deg.clone(), deg.clone()
    full[2 * n - 1], empty[2 * n] = MAX_ROW, 0
    want = _raw(shape, heads, mix, key, torch.where(torch.arange(4 * n, device=DEV) == 2 * n, empty, full), 3, False, with_tau=True, k=3)[1]
    got = _raw(shape, heads, mix, key, odd, 3, False, with_tau=True, k=3)[1]
    assert all(torch.equal(got[name], want[name]) for name in ARRAYS)
    # one slot in, one slot out
    one = FixedGraph.cat([trivial_graph(B, H, W, DEV).to_fixed()] * 4)
    assert one.width == 1
    arrays, status, _, _ = _against_heads(shape, heads, mix, one.key, one.deg, 1, "width 1", radius=1, k=1)
    assert arrays["key"].shape == (4 * n, 1) and bool((arrays["deg"] == 1).all()) and status.tolist()[0] == 0


# ---- 5. the module -------------------------------------------------------------------------------------------------------------------------
def _fixed_start(ces, x, case):
    """The key frame's state as CSR and as ``FixedGraph``s of the width every step of ``case`` gives back (its k)."""
    state = _key_state(ces, x)
    return state, state.to_fixed(case[3])


def _same_fixed(a, b, arrays=ARRAYS):
    for n in arrays:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert (a.mode, a.k, a.B, a.H, a.W, a.width) == (b.mode, b.k, b.B, b.H, b.W, b.width)


def _same_as_csr(fixed_state, csr_state):
    back = fixed_state.to_csr()
    for s in range(3):
        for n in CSR_ARRAYS:
            assert torch.equal(getattr(back.stages[s], n), getattr(csr_state.stages[s], n)), (s, n)


def _held_to_the_bounds(out_f, a, out_u, b, what):
    """test_gpu_ces_step_graphs.py's bounds for fused against head by head on whole calls: the first stage's graph bit for bit, keys and
    degrees equal, scores within 1e-4, output within 1e-3."""
    assert bool(torch.isfinite(out_f).all()) and bool(torch.isfinite(out_u).all())
    _same_fixed(a.stages[0], b.stages[0])
    err = _nw(out_f, out_u)
    print(f"[ces fixed] {what}: fused='stage' vs head by head {err:.2e} (bound 1e-3)")
    assert err <= 1e-3
    for s in range(3):
        _same_fixed(a.stages[s], b.stages[s], arrays=("key", "deg"))
        assert _nw(a.stages[s].score, b.stages[s].score) <= 1e-4, s


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_module_one_stage_input(case, feat):
    """Stage by stage on the head-by-head chain's inputs, a rolled second frame: the graph of ``fused="stage"`` is the head-by-head
    fixed call's bit for bit -- made of the call's arrays, no ``cat`` --, the output within the project's rule of the CPU mix of the
    heads' outputs."""
    from dagl_amd import FixedGraph
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    _, fixed = _fixed_start(ces, x, case)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    search = dict(propagate=False, explore=0, seed=0)
    plan = ces._plan_fixed("CES.step_graphs", x2, fixed, 1, feat, "stage", search)
    inp = x2
    with torch.no_grad():
        for s in (1, 2, 3):
            heads, mix = ces._stage_modules(s)
            pairs = [hd.step_graph(inp, fixed.head(s - 1, h), features=feat) for h, hd in enumerate(heads)]
            o_f, g_f = ces._stage_fixed_fused(s, inp, fixed.stages[s - 1], plan[s], feat, search, 1)
            _same_fixed(g_f, FixedGraph.cat([g for _, g in pairs]))
            _assert_filler(g_f)
            assert g_f.width == case[3] and int(g_f.deg.max()) > 0
            refs = _mix_refs([o for o, _ in pairs], mix, inp)
            _check(f"fixed stage {s} fused out {_cid(case)} {feat}", o_f, *refs)
            inp = ces._between_stages(s, mix(torch.cat([o for o, _ in pairs], dim=1)) + inp)
    _assert_state(ces, before)


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_module_three_frames_chained(case, feat):
    """Whole calls over three rolled frames.  Against the stage-fused call on the CSR state: output and graphs bit for bit, frame after
    frame.  Against the head-by-head fixed call: the bounds for whole calls.  ``fused=None`` stays head by head."""
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    csr, a = _fixed_start(ces, x, case)
    b, key_state = a, csr
    before = _module_state(ces)
    for i, shift in enumerate((1, 2, 3)):
        frame = torch.roll(x, (shift, shift), (2, 3))
        out_c, csr = ces.step_graphs(frame, csr, features=feat, fused=True)
        out_f, a = ces.step_graphs(frame, a, features=feat, fused="stage")
        assert a.fixed and not out_f.requires_grad and out_f.shape == frame.shape
        assert torch.equal(out_f, out_c), (i, "output against the CSR stage-fused step")
        _same_as_csr(a, csr)
        out_u, b_next = ces.step_graphs(frame, b, features=feat, fused=False)
        if i == 0:
            out_d, d = ces.step_graphs(frame, b, features=feat)                 # fused=None: head by head, bit for bit
            assert torch.equal(out_d, out_u) and all(torch.equal(getattr(d.stages[s], n), getattr(b_next.stages[s], n))
                                                     for s in range(3) for n in ARRAYS)
        b = b_next
        _held_to_the_bounds(out_f, a, out_u, b, f"{_cid(case)} {feat} frame {i + 1}")
        alone, none = ces.step_graphs(frame, a, features=feat, fused="stage", want_graphs=False)
        assert none is None and bool(torch.isfinite(alone).all())
    # on a CSR state fused="stage" means True
    frame = torch.roll(x, (1, 1), (2, 3))
    out_s, st_s = ces.step_graphs(frame, key_state, features=feat, fused="stage")
    out_t, st_t = ces.step_graphs(frame, key_state, features=feat, fused=True)
    assert torch.equal(out_s, out_t) and all(torch.equal(getattr(st_s.stages[s], n), getattr(st_t.stages[s], n))
                                             for s in range(3) for n in CSR_ARRAYS)
    _assert_state(ces, before)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_module_search_graphs_on_a_fixed_state(case, feat, iters):
    """``search_graphs`` on a fixed state: ``fused="stage"`` against its definition ``fused=False`` by the whole-call scheme, and
    against the stage-fused search on the CSR state bit for bit; ``fused=None`` stays refused there and names the served forms."""
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    csr, fixed = _fixed_start(ces, x, case)
    frame = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    kw = dict(features=feat, seed=3, iters=iters)
    out_f, a = ces.search_graphs(frame, fixed, fused="stage", **kw)
    out_u, b = ces.search_graphs(frame, fixed, fused=False, **kw)
    assert a.fixed and b.fixed and not out_f.requires_grad
    _held_to_the_bounds(out_f, a, out_u, b, f"search {_cid(case)} {feat} iters {iters}")
    out_c, c = ces.search_graphs(frame, csr, fused=True, **kw)
    assert torch.equal(out_f, out_c)
    _same_as_csr(a, c)
    for g in a.stages:
        _assert_filler(g)
    from dagl_amd import DaglError
    with pytest.raises(DaglError, match=r"fused='stage'.*fused=False.*\.to_csr\(\)"):      # the default on a fixed state: refused as before
        ces.search_graphs(frame, fixed, **kw)
    if iters == 1:
        alone, none = ces.search_graphs(frame, fixed, fused="stage", want_graphs=False, **kw)
        assert none is None and torch.equal(alone, out_f)
    _assert_state(ces, before)


def test_a_key_frame_from_the_trivial_start():
    """``SequenceState.start(...).to_fixed(k)`` followed by ``search_graphs(iters=n)``: the stage-fused build of the CSR route, bit for
    bit."""
    from dagl_amd.sequence import SequenceState
    _, ces, x = _build(TOPK8, shape=MODULE_SHAPE)
    start = SequenceState.start(x.shape[0], x.shape[2], x.shape[3], x.device, "topk")
    out_c, c = ces.build_graphs(x, iters=3, seed=4, fused=True)
    out_f, a = ces.search_graphs(x, start.to_fixed(8), iters=3, seed=4, fused="stage")
    assert torch.equal(out_f, out_c)
    _same_as_csr(a, c)
    assert all(int(g.deg.min()) >= 1 for g in a.stages)


def test_rr_passes_the_value_through():
    rr, ces, x = _build(TOPK8, shape=MODULE_SHAPE, trunk=True)
    with torch.no_grad():
        out, state = rr.forward_with_graphs(x)
    fixed = state.to_fixed(8)
    frame = torch.roll(x, (1, 1), (2, 3))
    out_f, a = rr.step_graphs(frame, fixed, fused="stage")
    out_u, b = rr.step_graphs(frame, fixed)
    assert a.fixed and out_f.shape == x.shape and _nw(out_f, out_u) <= 1e-4
    _same_fixed(a.stages[0], b.stages[0])
    out_s, s = rr.search_graphs(frame, fixed, iters=2, fused="stage")
    out_h, h = rr.search_graphs(frame, fixed, iters=2, fused=False)
    assert bool(torch.isfinite(out_s).all()) and _nw(out_s, out_h) <= 1e-3
    _same_fixed(s.stages[0], h.stages[0])


def test_module_refusals_come_before_any_launch():
    from dagl_amd import DaglError, _lib
    _, ces, x = _build(TOPK8, shape=MODULE_SHAPE)
    _, fixed = _fixed_start(ces, x, TOPK8)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    launches = []
    from dagl_amd import ops
    real = ops.graph_stage_step_fixed
    ops.graph_stage_step_fixed = lambda *a, **k: launches.append(1) or real(*a, **k)
    try:
        for call in (ces.step_graphs, ces.search_graphs):
            # fused=True on a fixed state: still refused, and the message names the new value
            with pytest.raises(DaglError, match="fused=True") as e:
                call(x2, fixed, fused=True)
            assert "fused='stage'" in str(e.value)
            with pytest.raises(DaglError, match="fused="):
                call(x2, fixed, fused="heads")
            # the row bound: 8 slots at radius 8 with propagation
            with pytest.raises(DaglError, match="candidates") as e:
                call(x2, fixed, fused="stage", radius=8, propagate=True, explore=8)
            assert e.value.code == _lib.ERR_UNSUPPORTED
            # a state that does not fit the input
            with pytest.raises(DaglError, match="state was built"):
                call(torch.cat([x2, x2]), fixed, fused="stage")
        # a stage that does not qualify: another scale in one head of stage 2 (the widths agree)
        ces.c2_3.softmax_scale = 5.0
        for call in (ces.step_graphs, ces.search_graphs):
            with pytest.raises(DaglError, match="stage 2 does not qualify"):
                call(x2, fixed, fused="stage")
        out, new = ces.step_graphs(x2, fixed)                                   # head by head serves it
        assert bool(torch.isfinite(out).all()) and new.fixed
        ces.c2_3.softmax_scale = ces.c2_1.softmax_scale
        # mixed widths: another k in one head of stage 3
        ces.c3_2.select_k = 4
        for call in (ces.step_graphs, ces.search_graphs):
            with pytest.raises(DaglError, match="widths"):
                call(x2, fixed, fused="stage")
        ces.c3_2.select_k = 8
        assert not launches
        out, new = ces.step_graphs(x2, fixed, fused="stage")
        assert launches == [1, 1, 1] and new.fixed
    finally:
        ops.graph_stage_step_fixed = real
    _assert_state(ces, before)


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------------------
def _capture_and_replay(ces, frames, start, call):
    """One stream, one eager warm-up (the eager chain).  ``out, new = call(x, state); state.copy_(new)`` captured once and replayed over
    the frames gives the eager chain's output and graphs after every replay."""
    from dagl_amd.sequence import SequenceState
    chain, st = [], start
    for frame in frames:                                                        # the eager chain (and the warm-up)
        out, st = call(frame, st)
        chain.append((out.clone(), st))
    state = SequenceState(g._like(g.key.clone(), g.weight.clone(), g.score.clone(), g.deg.clone()) for g in start.stages)
    x = frames[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert torch.cuda.is_current_stream_capturing()
        out, new_state = call(x, state)                                         # want_graphs=True: no refusal, no host read
        state.copy_(new_state)
    assert not torch.cuda.is_current_stream_capturing()
    for frame, (want_out, want_state) in zip(frames, chain):
        x.copy_(frame)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out)
        for s in range(3):
            for n in ARRAYS:
                assert torch.equal(getattr(state.stages[s], n), getattr(want_state.stages[s], n)), (s, n)


def test_capture_of_the_stage_fused_step():
    _, ces, x0 = _build(TOPK8, shape=MODULE_SHAPE)
    _, start = _fixed_start(ces, x0, TOPK8)
    frames = [torch.roll(x0, (s, s), (2, 3)) for s in (1, 2)]
    _capture_and_replay(ces, frames, start, lambda x, st: ces.step_graphs(x, st, fused="stage", features="split16"))


def test_capture_of_the_stage_fused_search():
    _, ces, x0 = _build(TOPK8, shape=MODULE_SHAPE)
    _, start = _fixed_start(ces, x0, TOPK8)
    frames = [torch.roll(x0, (s, s), (2, 3)) for s in (1, 2)]
    _capture_and_replay(ces, frames, start, lambda x, st: ces.search_graphs(x, st, iters=2, fused="stage", features="split16"))
