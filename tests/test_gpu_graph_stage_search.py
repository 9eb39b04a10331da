"""``ops.graph_stage_search`` / ``ops.graph_stage_search_step`` (dagl_graph_stage_search*, csrc/graph_refresh.hip) and the module methods on
them, ``CES.search_graphs`` / ``CES.build_graphs`` / ``RR.search_graphs`` / ``RR.build_graphs`` (dagl_amd/net.py).

The ops are held EXACTLY against four single-head calls (``ops.graph_search`` / ``ops.graph_search_step`` on head h's operands and its
slice of the input graph, whose own tests hold them against the CPU selection): every array of the graph bit for bit, and ``out`` against
``ops.ces_stage_fold_mix`` of the four single-head calls' aggregated rows, also bit for bit (the rows are read out of those calls'
workspaces, where they come first).  The module methods are held against their head-by-head definition (``fused=False``) with the scheme
of test_gpu_ces_step_graphs.py: exact graphs stage by stage on the head-by-head chain's stage inputs, that file's bounds on whole calls."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import ATOPK16, TOPK8, _check, _geom
from tests.graph_search_reference import MAX_ROW, candidate_mask, crafted, emptied_rows, features
from tests.test_gpu_ces_step_graphs import _assert_state, _build, _cid, _key_state, _module_state, _nw, _same_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARRAYS = ("row_off", "key", "weight", "score")
SHAPES = [(2, 24, 20), (1, 23, 30)]
HEAD_SEEDS = [(5, 7, 9), (6, 8, 10), (15, 17, 19), (25, 27, 29)]          # (graph, features, value map) of head h
SOURCES = [dict(propagate=True, explore=0), dict(propagate=False, explore=8), dict(propagate=True, explore=8)]
# top-k 4: a region of k per row, a wavefront per row where the row bound is <= 128 (radius 0; radius 1 with explore alone);
# adaptive and keep_all: no rank cut, the prefix-sum staging; block_rows: the block form where the wavefront form would run
CONFIGS = {"topk4": dict(k=4), "adaptive": dict(k=0, with_tau=True), "keep_all": dict(keep_all=True, with_tau=True),
           "topk4_block_rows": dict(k=4, block_rows=True)}
SEARCH = dict(propagate=True, explore=8, seed=5)


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _padded(b2):
    return F.pad(b2.permute(0, 2, 3, 1), (0, 0, 3, 3, 3, 3)).contiguous()


def _csr(rows):
    row_off = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0)
    return row_off, torch.tensor([k for r in rows for k in r], dtype=torch.int32)


def _rows_of(row_off, key):
    off = row_off.tolist()
    return [key[off[r]:off[r + 1]].tolist() for r in range(len(off) - 1)]


def _stage_of(shape, graphs, feature_seeds=None, value_seeds=None):
    """The four heads' operands on the device and the stage's CSR over the head-major rows, from four (row_off, key) on the CPU."""
    B, H, W, L, N = _geom(shape)
    heads = []
    for h, (row_off, key) in enumerate(graphs):
        wq, x, tau = features(shape, (feature_seeds or [s[1] for s in HEAD_SEEDS])[h])
        b2 = torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed((value_seeds or [s[2] for s in HEAD_SEEDS])[h]))
        heads.append(dict(row_off=row_off.to(DEV), key=key.to(DEV), wq=wq.to(DEV), x=x.to(DEV), tau=tau.to(DEV), b2p=_padded(b2).to(DEV),
                          cpu_off=row_off, cpu_key=key))
    base, offs = 0, [torch.zeros(1, dtype=torch.int64)]
    for row_off, _ in graphs:
        offs.append(row_off[1:] + base)
        base += int(row_off[-1])
    gen = torch.Generator().manual_seed(41)
    mix = dict(x=torch.randn(B, 64, H, W, generator=gen).to(DEV), mix_w=((torch.rand(64, 64, generator=gen) - 0.5) / 4).to(DEV),
               mix_b=((torch.rand(64, generator=gen) - 0.5) / 4).to(DEV))
    return heads, torch.cat(offs).to(DEV), torch.cat([h["key"] for h in heads]), mix


@functools.lru_cache(maxsize=None)
def _stage(shape):
    """Head h's crafted graph (rows 0 .. 9 are the crafted ones: the first row of every head is empty and follows a non-empty last row),
    banded features and value map, each from a seed of its own."""
    return _stage_of(shape, [crafted(shape, gs) for gs, _, _ in HEAD_SEEDS])


def _kw(stage, with_tau=False, **kw):
    heads = stage[0]
    return dict(tau4=[h["tau"] for h in heads] if with_tau else None, **kw)


def _graph_call(stage, shape, **kw):
    from dagl_amd import ops
    heads, row_off, key, _ = stage
    return ops.graph_stage_search([h["wq"] for h in heads], [h["x"] for h in heads], row_off, key, shape[1:], **_kw(stage, **kw))


def _step_call(stage, workspace=None, **kw):
    from dagl_amd import ops
    heads, row_off, key, mix = stage
    return ops.graph_stage_search_step([h["wq"] for h in heads], [h["x"] for h in heads], [h["b2p"] for h in heads], row_off, key,
                                       mix["x"], mix["mix_w"], mix["mix_b"], workspace=workspace, **_kw(stage, **kw))


def _agg_rows(ws, n_rows):
    """The aggregated rows [n_rows, 784] a step call left at the front of its workspace."""
    from dagl_amd import ops
    buf = ws.peek(DEV)
    at = ops._aligned(buf)[0] - buf.data_ptr()
    return buf[at:at + n_rows * 784 * 4].view(torch.float32).view(n_rows, 784).clone()


def _head_calls(stage, shape, step, with_tau=False, **kw):
    """The four single-head calls -> [(csr, status | None, aggregated rows | None)]."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    res = []
    for h in stage[0]:
        tau = h["tau"] if with_tau else None
        if step:
            ws = ops.Workspace()
            _, csr, status = ops.graph_search_step(h["wq"], h["x"], h["b2p"], h["row_off"], h["key"], tau=tau, workspace=ws, **kw)
            res.append((csr, status, _agg_rows(ws, B * L)))
        else:
            res.append((ops.graph_search(h["wq"], h["x"], h["row_off"], h["key"], tau=tau, hw=(H, W), **kw), None, None))
    return res


def _same_as_heads(csr, per_head, n, what):
    """Head h's rows of ``csr``: the single-head call's arrays bit for bit, the offsets continuing from head to head."""
    off = csr["row_off"]
    assert off.numel() == 4 * n + 1 and int(off[0]) == 0 and int(off[-1]) == csr["key"].numel(), what
    bounds = off[::n].tolist()
    for h, (want, _, _) in enumerate(per_head):
        assert torch.equal(off[h * n:(h + 1) * n + 1] - off[h * n], want["row_off"]), (what, h)
        for name in ARRAYS[1:]:
            assert torch.equal(csr[name][bounds[h]:bounds[h + 1]], want[name]), (what, h, name)


def _fold_mix(per_head, stage, shape):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    mix = stage[3]
    return ops.ces_stage_fold_mix(torch.stack([agg.view(B, L, 784) for _, _, agg in per_head]).contiguous(), mix["x"], mix["mix_w"],
                                  mix["mix_b"])


# ---- 1. the ops against four single-head calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_against_four_single_head_calls(shape, radius, config):
    """Declared ``max_row_edges`` 12: the row bound is 5 * 12 * (2 radius + 1)^2 + 8 at most, 68 (a wavefront) ... 1508 (a block)."""
    B, H, W, L, N = _geom(shape)
    stage = _stage(shape)
    for src in SOURCES:
        kw = dict(radius=radius, max_row_edges=MAX_ROW, seed=21, **src, **CONFIGS[config])
        what = f"{shape} radius {radius} {config} {src}"
        # the graph alone
        csr = _graph_call(stage, shape, **kw)
        _same_as_heads(csr, _head_calls(stage, shape, False, **kw), B * L, what)
        assert csr["key"].numel() > 0
        # the step: the same graph, the output from the single-head calls' aggregated rows
        out, csr_s, status = _step_call(stage, **kw)
        per_head = _head_calls(stage, shape, True, **kw)
        _same_as_heads(csr_s, per_head, B * L, what)
        assert all(torch.equal(csr_s[n], csr[n]) for n in ARRAYS), what
        assert status.tolist() == [0, max(st.tolist()[1] for _, st, _ in per_head)], what
        assert out.shape == (B, 64, H, W) and torch.equal(out, _fold_mix(per_head, stage, shape)), what
        # the same bits without the graph outputs, in the other form, with the row kernel launched per head
        for again in (dict(want_graph=False), dict(block_rows=True), dict(head_launches=True), dict(want_graph=False, head_launches=True)):
            o, g2, st = _step_call(stage, **{**kw, **again})
            assert torch.equal(o, out) and st.tolist() == status.tolist(), (what, sorted(again))
            assert g2 is None or all(torch.equal(g2[n], csr[n]) for n in ARRAYS), (what, sorted(again))


def test_both_sources_off_gives_the_plain_entries_bits():
    from dagl_amd import ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    stage = _stage(shape)
    heads, row_off, key, mix = stage
    for cfg in (dict(k=4), dict(k=0, with_tau=True)):
        kw = dict(radius=1, max_row_edges=MAX_ROW, **cfg)
        out, csr, status = _step_call(stage, propagate=False, explore=0, **kw)
        want_out, want, want_status = ops.graph_stage_step([h["wq"] for h in heads], [h["x"] for h in heads], [h["b2p"] for h in heads],
                                                           row_off, key, mix["x"], mix["mix_w"], mix["mix_b"], **_kw(stage, **kw))
        assert torch.equal(out, want_out) and status.tolist() == want_status.tolist()
        assert all(torch.equal(csr[n], want[n]) for n in ARRAYS)
        assert all(torch.equal(_graph_call(stage, shape, propagate=False, explore=0, **kw)[n], want[n]) for n in ARRAYS)


# ---- 2. the unbalanced graph: what a per-slice staging placement corrupts ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unbalanced(shape):
    """Head 0: degree 12 in every row; heads 1 - 3: degree 1; a few rows empty in every head."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(3)
    graphs = []
    for h in range(4):
        rows = [torch.randperm(N, generator=gen)[:12 if h == 0 else 1].tolist() for _ in range(B * L)]
        for r in (0, 3 + h, L - 1, B * L - 2):
            rows[r] = []
        graphs.append(_csr(rows))
    return _stage_of(shape, graphs)


@pytest.mark.parametrize("config", ["adaptive", "keep_all"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_unbalanced_heads_without_a_rank_cut(shape, config):
    """No rank cut, ``propagate``, radius 1, row bound 5 * 12 * 9 + 8 = 548: head 0 may stage 5 E_0 9 entries, far past where head 1's
    rows would begin in a layout by slices; no row of the other three heads may be lost."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    n = B * L
    stage = _unbalanced(shape)
    kw = dict(radius=1, max_row_edges=12, propagate=True, explore=8, seed=9, **CONFIGS[config])
    assert ops.graph_search_row_bound(12, 1, True, 8) == 548
    csr = _graph_call(stage, shape, **kw)
    per_head = _head_calls(stage, shape, False, **kw)
    _same_as_heads(csr, per_head, n, config)
    deg = csr["row_off"][1:] - csr["row_off"][:-1]
    for h in (1, 2, 3):
        want = per_head[h][0]["row_off"]
        assert torch.equal(deg[h * n:(h + 1) * n], want[1:] - want[:-1]), h
        assert int(deg[h * n:(h + 1) * n].min()) >= (1 if config == "keep_all" else 0) and int(deg[h * n:(h + 1) * n].sum()) > 0
    out, csr_s, status = _step_call(stage, **kw)
    per_head = _head_calls(stage, shape, True, **kw)
    assert all(torch.equal(csr_s[name], csr[name]) for name in ARRAYS) and status.tolist()[0] == 0
    assert torch.equal(out, _fold_mix(per_head, stage, shape))


# ---- 3. the hash is head-local --------------------------------------------------------------------------------------------------------------
def test_four_identical_heads_explore_the_same_keys():
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    n = B * L
    graph = crafted(shape, 5)
    stage = _stage_of(shape, [graph] * 4, feature_seeds=[7] * 4, value_seeds=[9] * 4)
    slices = {}
    for seed in (1, 2):
        csr = _graph_call(stage, shape, radius=0, k=4, max_row_edges=MAX_ROW, propagate=False, explore=8, seed=seed)
        off = csr["row_off"]
        bounds = off[::n].tolist()
        slices[seed] = [(off[h * n:(h + 1) * n + 1] - off[h * n],) + tuple(csr[name][bounds[h]:bounds[h + 1]] for name in ARRAYS[1:])
                        for h in range(4)]
        for h in (1, 2, 3):
            assert all(torch.equal(a, b) for a, b in zip(slices[seed][h], slices[seed][0])), (seed, h)
    assert not (slices[1][0][1].numel() == slices[2][0][1].numel() and torch.equal(slices[1][0][1], slices[2][0][1]))
    # keep_all at radius 0 returns the candidate set itself: the row's own valid keys and the keys hashed from the HEAD-LOCAL row
    csr = _graph_call(stage, shape, radius=0, keep_all=True, max_row_edges=MAX_ROW, propagate=False, explore=8, seed=1)
    want = candidate_mask(graph[0], graph[1], B, H, W, 0, False, 8, 1)
    rows = torch.repeat_interleave(torch.arange(4 * n), (csr["row_off"][1:] - csr["row_off"][:-1]).cpu())
    got = torch.zeros(4 * n, N, dtype=torch.bool)
    got[rows, csr["key"].cpu().long()] = True
    assert torch.equal(got, want.repeat(4, 1))


# ---- 4. empty inputs and overlong rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_empty_inputs(shape):
    B, H, W, L, N = _geom(shape)
    n = 4 * B * L
    base = _stage(shape)
    empty = (base[0], torch.zeros(n + 1, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), base[3])
    mix = base[3]
    # explore = 0: an empty graph and out = mix_b + x
    for kw in (dict(propagate=True), dict(propagate=False), dict(propagate=True, k=4, with_tau=True)):
        for want_graph in (True, False):
            out, csr, status = _step_call(empty, max_row_edges=0, explore=0, want_graph=want_graph, **kw)
            assert torch.equal(out, mix["mix_b"].view(1, 64, 1, 1) + mix["x"]) and status.tolist() == [0, 0]
            if want_graph:
                assert csr["key"].shape == csr["weight"].shape == csr["score"].shape == (0,)
                assert csr["row_off"].shape == (n + 1,) and not bool(csr["row_off"].any())
        csr = _graph_call(empty, shape, max_row_edges=0, explore=0, **kw)
        assert csr["key"].numel() == 0 and not bool(csr["row_off"].any())
    # explore = 8 populates it: the hashed keys, the same for the four heads
    for propagate in (False, True):
        kw = dict(max_row_edges=0, propagate=propagate, explore=8, seed=4, keep_all=True, radius=1)
        csr = _graph_call(empty, shape, **kw)
        want = candidate_mask(torch.zeros(B * L + 1, dtype=torch.int64), torch.empty(0, dtype=torch.int32), B, H, W, 1, propagate, 8, 4)
        deg = (csr["row_off"][1:] - csr["row_off"][:-1]).cpu()
        assert torch.equal(deg, want.sum(dim=1).repeat(4)) and int(deg.min()) >= 1
        got = torch.zeros(n, N, dtype=torch.bool)
        got[torch.repeat_interleave(torch.arange(n), deg), csr["key"].cpu().long()] = True
        assert torch.equal(got, want.repeat(4, 1))
        out, csr_s, status = _step_call(empty, **kw)
        assert all(torch.equal(csr_s[name], csr[name]) for name in ARRAYS) and status.tolist()[0] == 0
        assert bool(torch.isfinite(out).all()) and not torch.equal(out, mix["mix_b"].view(1, 64, 1, 1) + mix["x"])


def test_an_overlong_row_in_head_2():
    """Row 20 of head 2 holds 13 keys, 12 are declared: it and its grid neighbours come out empty and are counted once each; with the
    graph wanted the wrapper raises ``ERR_UNSUPPORTED``."""
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    n = B * L
    graphs = [crafted(shape, gs) for gs, _, _ in HEAD_SEEDS]
    rows = _rows_of(*graphs[2])
    rows[20] = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:MAX_ROW + 1].tolist()
    graphs[2] = _csr(rows)
    stage = _stage_of(shape, graphs)
    emptied = emptied_rows(graphs[2][0], B, H, W, MAX_ROW, True)
    assert emptied.nonzero().view(-1).tolist() == [15, 20, 21, 25]
    assert not any(bool(emptied_rows(graphs[h][0], B, H, W, MAX_ROW, True).any()) for h in (0, 1, 3))
    kw = dict(radius=1, k=4, max_row_edges=MAX_ROW, propagate=True, explore=8, seed=2)
    ws = ops.Workspace()
    out, none, status = _step_call(stage, workspace=ws, want_graph=False, **kw)
    assert none is None and status.tolist()[0] == 4
    agg = _agg_rows(ws, 4 * n).view(4, n, 784)
    assert not bool(agg[2][emptied.to(DEV)].any()) and bool(agg[2][~emptied.to(DEV)].any(dim=1).all())
    per_head = []
    for h in stage[0]:
        hws = ops.Workspace()
        _, _, st = ops.graph_search_step(h["wq"], h["x"], h["b2p"], h["row_off"], h["key"], workspace=hws, want_graph=False, **kw)
        per_head.append((None, st, _agg_rows(hws, n)))
    assert [int(st[0]) for _, st, _ in per_head] == [0, 0, 4, 0]
    assert torch.equal(out, _fold_mix(per_head, stage, shape))
    for call in (lambda: _step_call(stage, **kw), lambda: _graph_call(stage, shape, **kw)):
        with pytest.raises(_lib.DaglError, match="4 row") as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED and "next to" in str(e.value)
    # without propagation the row alone
    out, none, status = _step_call(stage, want_graph=False, **{**kw, "propagate": False})
    assert status.tolist()[0] == 1


# ---- 5. determinism and capture -------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_captured_one_give_the_same_bits():
    from dagl_amd import ops
    shape = SHAPES[0]
    stage = _stage(shape)
    heads, row_off, key, mix = stage
    kw = dict(radius=1, k=4, max_row_edges=MAX_ROW, propagate=True, explore=8, seed=6)
    out, csr, status = _step_call(stage, **kw)
    out2, csr2, status2 = _step_call(stage, **kw)
    assert torch.equal(out, out2) and status.tolist() == status2.tolist() and all(torch.equal(csr[n], csr2[n]) for n in ARRAYS)
    ws = ops.Workspace()
    eager = _step_call(stage, workspace=ws, want_graph=False, **kw)[0].clone()          # (also brings the workspace to its size)
    assert torch.equal(eager, out)
    other = _step_call(stage, workspace=ws, want_graph=False, **{**kw, "seed": 7})[0]
    assert not torch.equal(other, eager)
    x_in = mix["x"].clone()
    captured_stage = (heads, row_off, key, dict(mix, x=x_in))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(ops.DaglError, match="captur"):
            _step_call(captured_stage, workspace=ws, **kw)                              # the graph is read on the host
        captured, none, _ = _step_call(captured_stage, workspace=ws, want_graph=False, **kw)
    assert none is None
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


# ---- 6. - 10. the module methods --------------------------------------------------------------------------------------------------------------
WHAT = "CES.search_graphs"


def _plans(ces, x, state, feat, search=SEARCH, want_graphs=True):
    plan_u = ces._plan_step(x, state, 1, feat, want_graphs, False, search, what=WHAT)
    plan_f = ces._plan_step(x, state, 1, feat, want_graphs, True, search, what=WHAT)
    assert all(plan_f[s][0] and not plan_u[s][0] for s in (1, 2, 3))
    return plan_u, plan_f


def _mix_refs(outs, mix, inp):
    torch.set_num_threads(16)
    return [F.conv2d(torch.cat([o.cpu().to(dt) for o in outs], dim=1), mix.weight.detach().cpu().to(dt), mix.bias.detach().cpu().to(dt))
            + inp.cpu().to(dt) for dt in (torch.float64, torch.float32)]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_search_stage_fused_against_head_by_head(case, feat, iters):
    """Stage by stage on the head-by-head chain's inputs, a rolled second frame: the graphs bit for bit, the output against the CPU mix
    of the heads' outputs (the chain of public calls), the same bits without the graphs."""
    _, ces, x = _build(case)
    state = _key_state(ces, x)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    plan_u, plan_f = _plans(ces, x2, state, feat)
    kw = dict(radius=1, features=feat, propagate=True, explore=8)
    inp = x2
    with torch.no_grad():
        for s in (1, 2, 3):
            o_u, g_u = ces._search_stage(s, inp, state, plan_u[s], iters, feat, True, SEARCH)
            o_f, g_f = ces._search_stage(s, inp, state, plan_f[s], iters, feat, True, SEARCH)
            _same_graph(g_f, g_u)
            assert g_f.B == 4 * x.shape[0] and g_f.n_edges > 0
            heads, mix = ces._stage_modules(s)
            outs = []
            for h, hd in enumerate(heads):                       # the chain of public calls: refresh_graph x (iters - 1), step_graph
                g = state.head(s - 1, h)
                for i in range(iters - 1):
                    g = hd.refresh_graph(inp, g, seed=SEARCH["seed"] + i, **kw)
                o, g = hd.step_graph(inp, g, seed=SEARCH["seed"] + iters - 1, **kw)
                outs.append(o)
                _same_graph(g_f.images(h * x.shape[0], (h + 1) * x.shape[0]), g)
            if iters == 1:
                alone, none = ces._search_stage(s, inp, state, plan_f[s], 1, feat, False, SEARCH)
                assert none is None and torch.equal(alone, o_f)
            refs = _mix_refs(outs, mix, inp)
            _check(f"search stage {s} fused out {_cid(case)} {feat} iters {iters}", o_f, *refs)
            _check(f"search stage {s} head-by-head out {_cid(case)} {feat} iters {iters}", o_u, *refs)
            inp = ces._between_stages(s, o_u)
    _assert_state(ces, before)


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_search_graphs_whole_call(case, feat):
    """Both forms from the key frame's state on a rolled frame: finite outputs, the first stage's graph bit for bit, every structure
    equal, the scores within 1e-4 and the outputs within 1e-3 of each other (test_gpu_ces_step_graphs.py's bounds for calls whose
    later stages see inputs that differ by the mix product's roundings); the default form is the fused one; the state is untouched."""
    _, ces, x = _build(case)
    state = _key_state(ces, x)
    frame = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    kw = dict(features=feat, seed=3, iters=2)
    out_f, a = ces.search_graphs(frame, state, fused=True, **kw)
    out_u, b = ces.search_graphs(frame, state, fused=False, **kw)
    assert out_f.shape == frame.shape and bool(torch.isfinite(out_f).all()) and bool(torch.isfinite(out_u).all())
    assert not out_f.requires_grad
    _same_graph(a.stages[0], b.stages[0])
    out_d, d = ces.search_graphs(frame, state, **kw)
    assert torch.equal(out_d, out_f) and all(torch.equal(getattr(d.stages[s], n), getattr(a.stages[s], n)) for s in range(3) for n in ARRAYS)
    err = _nw(out_f, out_u)
    print(f"[ces search] {_cid(case)} {feat}: fused vs head by head {err:.2e} (bound 1e-3); edges {[g.n_edges for g in a.stages]}")
    assert err <= 1e-3
    for s in range(3):
        _same_graph(a.stages[s], b.stages[s], arrays=("row_off", "key"))
        assert _nw(a.stages[s].score, b.stages[s].score) <= 1e-4, s
    alone, none = ces.search_graphs(frame, a, features=feat, want_graphs=False)
    assert none is None and bool(torch.isfinite(alone).all())
    _assert_state(ces, before)


def test_three_iterations_are_three_calls():
    """``iters=3`` on a stage: the same graph and output as three ``iters=1`` steps with seeds s, s + 1, s + 2 fed the same stage input
    and each other's graphs."""
    from dagl_amd.sequence import SequenceState
    _, ces, x = _build(TOPK8)
    state = _key_state(ces, x)
    x2 = torch.roll(x, (1, 1), (2, 3))
    feat = "split16"
    plan_u, plan_f = _plans(ces, x2, state, feat)
    inp = x2
    with torch.no_grad():
        for s in (1, 2, 3):
            for plan in (plan_f, plan_u):
                o3, g3 = ces._search_stage(s, inp, state, plan[s], 3, feat, True, SEARCH)
                cur = state
                for i in range(3):
                    o1, g1 = ces._search_stage(s, inp, cur, plan[s], 1, feat, True, dict(SEARCH, seed=SEARCH["seed"] + i))
                    cur = SequenceState([g1 if j == s - 1 else state.stages[j] for j in range(3)])
                _same_graph(g1, g3)
                assert torch.equal(o1, o3)
            inp = ces._between_stages(s, ces._search_stage(s, inp, state, plan_u[s], 3, feat, True, SEARCH)[0])
    # whole calls head by head run the very same launches either way: bit for bit
    out3, st3 = ces.search_graphs(x2, state, iters=3, seed=5, features=feat, fused=False)
    assert torch.equal(out3, ces._between_stages(3, o3)) and bool(torch.isfinite(out3).all())
    for s in range(3):
        assert st3.stages[s].n_edges > 0
    _same_graph(st3.stages[2], g3)


@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_build_graphs(case):
    """``CES.build_graphs(iters=3)``: every head's graph is ``hd.build_graph`` on the chain's stage input, bit for bit; in top-k mode no
    row is empty; the same seed gives the same state, another seed another."""
    from dagl_amd.sequence import SequenceState
    _, ces, x = _build(case)
    B = x.shape[0]
    before = _module_state(ces)
    feat = "fp32"
    search = dict(propagate=True, explore=8, seed=4)
    start = SequenceState.start(*x.shape[:1], *x.shape[2:], x.device)
    plan_u, plan_f = _plans(ces, x, start, feat, search)
    inp = x
    with torch.no_grad():
        for s in (1, 2, 3):
            o_u, g_u = ces._search_stage(s, inp, start, plan_u[s], 3, feat, True, search)
            o_f, g_f = ces._search_stage(s, inp, start, plan_f[s], 3, feat, True, search)
            _same_graph(g_f, g_u)
            for h, hd in enumerate(ces._stage_modules(s)[0]):
                want = hd.build_graph(inp, iters=3, radius=1, explore=8, seed=4, features=feat)
                _same_graph(g_f.images(h * B, (h + 1) * B), want)
            if case[2] == "topk":
                assert int(g_f.degrees().min()) >= 1
            inp = ces._between_stages(s, o_u)
    out, state = ces.build_graphs(x, iters=3, seed=4)
    g0 = ces.build_graphs(x, iters=3, seed=4, fused=False)[1].stages[0]
    _same_graph(state.stages[0], g0)
    for h, hd in enumerate(ces._stage_modules(1)[0]):            # the first stage's input is x itself
        _same_graph(state.head(0, h), hd.build_graph(x, iters=3, seed=4))
    assert out.shape == x.shape and bool(torch.isfinite(out).all()) and g0.n_edges > 0
    out2, again = ces.build_graphs(x, iters=3, seed=4)
    assert torch.equal(out2, out) and all(torch.equal(getattr(again.stages[s], n), getattr(state.stages[s], n))
                                          for s in range(3) for n in ARRAYS)
    _, other = ces.build_graphs(x, iters=3, seed=5)
    assert not all(other.stages[s].key.numel() == state.stages[s].key.numel() and torch.equal(other.stages[s].key, state.stages[s].key)
                   for s in range(3))
    # the built state steps
    stepped, nxt = ces.step_graphs(torch.roll(x, (1, 1), (2, 3)), state)
    assert bool(torch.isfinite(stepped).all()) and nxt.stages[0].n_edges > 0
    _assert_state(ces, before)


def test_rr_build_and_search_graphs():
    rr, ces, x = _build(TOPK8, shape=(1, 24, 20), trunk=True)
    out, state = rr.build_graphs(x, iters=2, seed=1)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())
    assert (state.B, state.stages[0].H, state.stages[0].W) == (1, 24, 20)
    frame = torch.roll(x, (1, 1), (2, 3))
    stepped, nxt = rr.step_graphs(frame, state)
    assert stepped.shape == x.shape and bool(torch.isfinite(stepped).all()) and nxt.stages[2].n_edges > 0
    searched, nxt2 = rr.search_graphs(frame, state, iters=2)
    assert searched.shape == x.shape and bool(torch.isfinite(searched).all())
    by_heads, nxt3 = rr.search_graphs(frame, state, iters=2, fused=False)
    _same_graph(nxt2.stages[0], nxt3.stages[0])
    assert _nw(searched, by_heads) <= 1e-3


def test_refusals():
    from dagl_amd import DaglError, _lib
    from dagl_amd.sequence import SequenceState
    _, ces, x = _build(TOPK8)
    ces.c2_3.select_k = 4
    start = SequenceState.start(*x.shape[:1], *x.shape[2:], x.device)
    before = _module_state(ces)
    with pytest.raises(DaglError, match="stage 2"):
        ces.search_graphs(x, start, fused=True)
    with pytest.raises(DaglError, match="stage 2"):
        ces.build_graphs(x, iters=2, fused=True)
    out, state = ces.build_graphs(x, iters=2)                    # fused=None: stage 2 head by head
    assert bool(torch.isfinite(out).all())
    assert [int(state.head(1, h).degrees().max()) for h in range(4)] == [8, 8, 4, 8]
    _assert_state(ces, before)
    # an adaptive mask that keeps nearly every candidate: from the trivial start a row holds up to 5 * 25 + 8 = 133 candidates at radius 2
    # after one iteration, and 17 kept ones already put the next row bound, 5 * 17 * 25 + 8, past the 2048 a row may expand into
    _, dense, xd = _build(("default", 2.0, "adaptive", 0))
    startd = SequenceState.start(*xd.shape[:1], *xd.shape[2:], xd.device)
    once, grown = dense.search_graphs(xd, startd, iters=1, radius=2)
    assert bool(torch.isfinite(once).all()) and grown.stages[0].max_degree() >= 17
    for fused in (True, False):
        with pytest.raises(DaglError, match="candidates") as e:
            dense.search_graphs(xd, startd, iters=2, radius=2, fused=fused)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(DaglError, match="after 1 iteration"):
        dense.search_graphs(xd, startd, iters=2, radius=2, fused=True)
    with pytest.raises(DaglError) as e:                          # ... and at the start of a call on the grown state
        dense.search_graphs(xd, grown, radius=2)
    assert e.value.code == _lib.ERR_UNSUPPORTED
