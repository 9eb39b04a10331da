"""``CES.forward_with_graphs`` / ``CES.step_graphs`` and the ``RR`` methods around them (dagl_amd/net.py): sequence steps of a whole
stage-and-head module on per-head patch graphs.

``fused=False`` -- ``CE.step_graph`` head by head, ``torch.cat``, the mix convolution -- is the definition; the fused form
(``ops.graph_stage_step``) must return the same graphs bit for bit and an output within the project's rule ``e <= 3 e_ref32 + 1e-6`` of the
CPU mix of the heads' step outputs.  Exact equality is a statement about ONE stage on ONE input: the two forms' stage outputs differ by the
roundings of the mix product, so the next stage of a whole call sees inputs that differ in the last bits and its weights do too.  The
stage-by-stage test therefore feeds both forms the head-by-head chain's stage inputs; the whole-call tests hold the first stage's graph
exactly, every later structure exactly (the cases' k-th / (k+1)-th gaps are orders above the perturbation) and the outputs under the
round-trip rule's bounds."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import ATOPK16, TOPK8, _check, _gap, _inputs
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 24, 20)
ARRAYS = ("row_off", "key", "weight", "score")
CASES = [TOPK8, ATOPK16]
HEAD_SEEDS = list(range(11, 23))


def _cid(case):
    return "-".join(map(str, case))


def _nw(a, b):
    return normwise(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


def _build(case, shape=SHAPE, scan=None, trunk=False):
    """A ``CES`` (or a two-ResBlock ``RR`` around one) whose twelve heads carry seeded parameters of ``case``, and a seeded input."""
    from dagl_amd.net import CES, RR
    variant, gain, mode, k = case
    torch.manual_seed(3)
    net = RR(n_resblocks=2) if trunk else CES(64)
    ces = net.body[1] if trunk else net
    for i, (s, h) in enumerate((s, h) for s in (1, 2, 3) for h in (1, 2, 3, 4)):
        hd = getattr(ces, f"c{s}_{h}")
        hd.load_state_dict(_inputs(HEAD_SEEDS[i], shape, variant, gain)[1], strict=True)
        hd.select_mode = mode
        if mode != "adaptive":
            hd.select_k = k
        if scan is not None:
            hd.scan = scan
    net = net.to(DEV).eval()
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(shape[0], 1, *shape[1:], generator=gen) if trunk else _inputs(11, shape, variant, gain)[0]
    return net, ces, x.to(DEV)


def _key_state(ces, x):
    """The key frame's state from every head's ``CE.graph`` of its stage input (the stage inputs are ``forward``'s)."""
    from dagl_amd.sequence import SequenceState
    graphs, out = [], x
    with torch.no_grad():
        for s in (1, 2, 3):
            heads, _ = ces._stage_modules(s)
            graphs += [hd.graph(out) for hd in heads]
            out = ces._between_stages(s, ces._stage(s, out))
    return SequenceState.from_heads(graphs)


def _same_graph(a, b, arrays=ARRAYS):
    for n in arrays:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert (a.mode, a.k, a._valid, a.B, a.H, a.W) == (b.mode, b.k, b._valid, b.B, b.H, b.W)


def _module_state(ces):
    heads = [getattr(ces, f"c{s}_{h}") for s in (1, 2, 3) for h in (1, 2, 3, 4)]
    return (dict(ces._pack_key), dict(ces._skip_fused), dict(ces._fused_calls),
            [(hd.last_info, hd.scan, hd.topk_threshold, hd._train_dense, hd._pack_key, hd._pack_epoch, hd._last_call) for hd in heads],
            {n: t.clone() for n, t in ces.state_dict().items()})


def _assert_state(ces, before):
    after = _module_state(ces)
    assert after[:4] == before[:4]
    assert all(torch.equal(t, before[4][n]) for n, t in after[4].items())


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_fused_stage_against_head_by_head(case, feat):
    """Stage by stage on the head-by-head chain's inputs, a rolled second frame: the graphs bit for bit, the output against the CPU mix
    of the heads' ``CE.step_graph`` outputs, the same bits without the graphs."""
    _, ces, x = _build(case)
    state = _key_state(ces, x)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    plan_u = ces._plan_step(x2, state, 1, feat, True, False)
    plan_f = ces._plan_step(x2, state, 1, feat, True, True)
    assert all(plan_f[s][0] and not plan_u[s][0] for s in (1, 2, 3))
    inp = x2
    torch.set_num_threads(16)
    with torch.no_grad():
        for s in (1, 2, 3):
            o_u, g_u = ces._step_stage(s, inp, state, plan_u[s], feat, True)
            o_f, g_f = ces._step_stage(s, inp, state, plan_f[s], feat, True)
            _same_graph(g_f, g_u)
            assert g_f.B == 4 * SHAPE[0] and g_f.n_edges > 0
            alone, none = ces._step_stage(s, inp, state, plan_f[s], feat, False)
            assert none is None and torch.equal(alone, o_f)
            heads, mix = ces._stage_modules(s)
            outs = [hd.step_graph(inp, state.head(s - 1, h), features=feat, want_graph=False)[0] for h, hd in enumerate(heads)]
            refs = [F.conv2d(torch.cat([o.cpu().to(dt) for o in outs], dim=1), mix.weight.detach().cpu().to(dt), mix.bias.detach().cpu().to(dt))
                    + inp.cpu().to(dt) for dt in (torch.float64, torch.float32)]
            _check(f"stage {s} fused out {_cid(case)} {feat}", o_f, *refs)
            _check(f"stage {s} head-by-head out {_cid(case)} {feat}", o_u, *refs)
            inp = ces._between_stages(s, o_u)
    _assert_state(ces, before)


@pytest.mark.parametrize("feat", ["fp32", "split16"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_three_frames_chained(case, feat):
    """Whole calls, both forms, three rolled frames: finite outputs, the first step's first-stage graph bit for bit, every structure
    equal, the outputs within 1e-3 of each other; the default form is the fused one here; the module state is untouched."""
    _, ces, x = _build(case)
    a = b = _key_state(ces, x)
    key_again = _key_state(ces, x)
    with torch.no_grad():
        want = ces(x).clone()
    before = _module_state(ces)
    for i, shift in enumerate((1, 2, 3)):
        frame = torch.roll(x, (shift, shift), (2, 3))
        out_f, a = ces.step_graphs(frame, a, features=feat, fused=True)
        out_u, b = ces.step_graphs(frame, b, features=feat, fused=False)
        assert out_f.shape == frame.shape and bool(torch.isfinite(out_f).all()) and bool(torch.isfinite(out_u).all())
        assert not out_f.requires_grad
        if i == 0:
            _same_graph(a.stages[0], b.stages[0])
            out_d, d = ces.step_graphs(frame, key_again, features=feat)
            assert torch.equal(out_d, out_f) and all(torch.equal(getattr(d.stages[s], n), getattr(a.stages[s], n))
                                                     for s in range(3) for n in ARRAYS)
        err = _nw(out_f, out_u)
        # the later stages' inputs differ by the mix product's roundings (1e-7); a logit z = 10 S m turns a relative change d of S into
        # 2 |z| d of its weight, and the sparse heads' logits reach ~1e2: the weights are printed, the scores (linear in the input) and
        # the outputs are held -- the outputs under the round-trip rule's bound for calls whose selection inputs may move, 1e-3
        w_err = [_nw(a.stages[s].weight, b.stages[s].weight) for s in range(3)]
        print(f"[ces step] {_cid(case)} {feat} frame {i + 1}: fused vs head by head {err:.2e} (bound 1e-3); edges "
              f"{[g.n_edges for g in a.stages]}; weights {['%.1e' % e for e in w_err]}")
        assert err <= 1e-3
        for s in range(3):
            _same_graph(a.stages[s], b.stages[s], arrays=("row_off", "key"))
            assert _nw(a.stages[s].score, b.stages[s].score) <= 1e-4, s
        alone, none = ces.step_graphs(frame, a, features=feat, want_graphs=False)
        assert none is None and bool(torch.isfinite(alone).all())
    _assert_state(ces, before)
    with torch.no_grad():
        assert torch.equal(ces(x), want)                     # (the stage's own launch set: the bits it had)


def test_key_frame_reproduces_the_forward():
    """``forward_with_graphs`` against ``forward`` on heads with ``scan = "exact"``: top-k 8 at (2,24,20), every head's k-th / (k+1)-th
    gap on its own stage input at least 1e-6 (the fp64 oracle, on the CPU), so the tight bound of the round-trip rule, 1e-4, applies."""
    from oracle.ce_oracle import ce_forward_oracle
    variant, gain, mode, k = TOPK8
    _, ces, x = _build(TOPK8, scan="exact")
    inputs = []
    hooks = [getattr(ces, f"c{s}_1").register_forward_pre_hook(lambda m, args: inputs.append(args[0].detach().cpu())) for s in (1, 2, 3)]
    with torch.no_grad():
        want = ces(x)
    for hk in hooks:
        hk.remove()
    before = _module_state(ces)
    torch.set_num_threads(16)
    gaps = []
    for s in range(3):
        for h in range(4):
            prm = _inputs(HEAD_SEEDS[4 * s + h], SHAPE, variant, gain)[1]
            with torch.no_grad():
                st = ce_forward_oracle(inputs[s], prm, mode=mode, k=k, dtype=torch.float64, stages=True)[1]
            gaps.append(_gap(st, mode, k, *SHAPE[1:]))
    print(f"[ces key frame] gaps {['%.1e' % g for g in gaps]}")
    assert min(gaps) >= 1e-6, "the case must be one the tight bound applies to"
    with torch.no_grad():
        out, state = ces.forward_with_graphs(x)
    err = _nw(out, want)
    print(f"[ces key frame] forward_with_graphs vs forward: {err:.2e} (bound 1e-4)")
    assert err <= 1e-4
    assert all(g.B == 4 * SHAPE[0] and g._valid and g.n_edges == 4 * SHAPE[0] * 30 * k for g in state.stages)
    _assert_state(ces, before)
    # the state steps: the same frame again, from the key frame's own graphs
    again, _ = ces.step_graphs(x, state)
    err = _nw(again, want)
    print(f"[ces key frame] step_graphs(x, key state) vs forward: {err:.2e} (bound 1e-4)")
    assert err <= 1e-4


def test_a_stage_with_mixed_select_k():
    from dagl_amd import DaglError
    _, ces, x = _build(TOPK8)
    ces.c2_3.select_k = 4
    state = _key_state(ces, x)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    plan = ces._plan_step(x2, state, 1, "fp32", True, None)
    assert [plan[s][0] for s in (1, 2, 3)] == [True, False, True]
    out, new = ces.step_graphs(x2, state)
    assert bool(torch.isfinite(out).all())
    assert [int(new.head(1, h).degrees().max()) for h in range(4)] == [8, 8, 4, 8]
    with pytest.raises(DaglError, match="stage 2"):
        ces.step_graphs(x2, state, fused=True)
    _assert_state(ces, before)
    # refusals that do not depend on a stage
    for bad, kw, word in ((x2[:1], {}, "state was built"), (x2, dict(radius=9), "radius"), (x2, dict(features="fp16"), "features"),
                          (x2.cpu(), {}, "GPU")):
        with pytest.raises(DaglError, match=word):
            ces.step_graphs(bad, state, **kw)
    with pytest.raises(DaglError, match="SequenceState"):
        ces.step_graphs(x2, state.stages)
    _assert_state(ces, before)


def test_capture_of_the_output_alone():
    """On a validated state whose largest degrees have been read, ``want_graphs=False`` under ``torch.cuda.graph`` (one stream, no parallel
    branches) replays to the eager bits, also on a new input; the forms that read the host are refused before any launch and the capture
    stays usable."""
    from dagl_amd import DaglError
    from dagl_amd.sequence import SequenceState
    _, ces, x = _build(TOPK8)
    x2 = torch.roll(x, (1, 1), (2, 3))
    state = _key_state(ces, x)
    for g in state.stages:
        g.validate().max_degree()
    kw = dict(want_graphs=False, features="split16")
    eager2 = ces.step_graphs(x2, state, **kw)[0].clone()              # (also brings the workspaces to their sizes)
    eager1 = ces.step_graphs(x, state, **kw)[0].clone()
    assert not torch.equal(eager1, eager2)
    frame = x2.clone()
    unknown = SequenceState([g._like(g.row_off, g.key, g.weight, g.score) for g in state.stages])       # largest degrees not read
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    refusals = []
    with torch.cuda.graph(graph):
        for bad, bad_kw in ((state, dict(features="split16")), (unknown, kw), (unknown, dict(kw, fused=False))):
            with pytest.raises(DaglError) as e:
                ces.step_graphs(frame, bad, **bad_kw)
            refusals.append(str(e.value))
        captured = ces.step_graphs(frame, state, **kw)[0]
    assert "captur" in refusals[0] and "max_degree()" in refusals[1] and "captur" in refusals[2], refusals
    assert all(g._max_degree is None for g in unknown.stages)
    for src, eager in ((x2, eager2), (x, eager1), (x2, eager2)):
        frame.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def test_rr_sequence_against_the_hand_written_one():
    """A two-ResBlock ``RR`` at (1,24,20): the key frame and two steps with ``fused=False`` are, bit for bit, the ``body`` modules run in
    order by hand with the ``CES`` methods where the ``CES`` sits; with the default ``fused`` the outputs stay within 1e-4."""
    from dagl_amd.net import CES
    rr, ces, x = _build(TOPK8, shape=(1, 24, 20), trunk=True)
    frames = [x, torch.roll(x, (1, 1), (2, 3)), torch.roll(x, (2, 2), (2, 3))]

    def by_hand(frame, ces_call):
        out, state = rr.head(frame), None
        for m in rr.body:
            if isinstance(m, CES):
                out, state = ces_call(m, out)
            else:
                out = m(out)
        return frame + rr.tail(out), state

    with torch.no_grad():
        out, state = rr.forward_with_graphs(frames[0])
        want, want_state = by_hand(frames[0], lambda m, t: m.forward_with_graphs(t))
        assert torch.equal(out, want) and out.shape == x.shape
        default_state = state
        for frame in frames[1:]:
            out, state = rr.step_graphs(frame, state, fused=False)
            want, want_state = by_hand(frame, lambda m, t: m.step_graphs(t, want_state, fused=False))
            assert torch.equal(out, want)
            for s in range(3):
                _same_graph(state.stages[s], want_state.stages[s])
            out_d, default_state = rr.step_graphs(frame, default_state)
            err = _nw(out_d, out)
            print(f"[rr step] default fused vs head by head: {err:.2e} (bound 1e-4)")
            assert err <= 1e-4 and bool(torch.isfinite(out_d).all())
        alone, none = rr.step_graphs(frames[2], state, want_graphs=False)
        assert none is None and alone.shape == x.shape
