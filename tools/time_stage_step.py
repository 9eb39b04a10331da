"""What a sequence step of one ``CES`` stage costs (``CES.step_graphs``, dagl_amd/net.py) next to the stage's own forward.

    python tools/time_stage_step.py            # a stage input of [1,64,256,256], top-k 8
    python tools/time_stage_step.py 1024 1024  # with a size: adaptive AND top-16 on the sparse variant (the benchmark's 1024^2 regime)

Per case, ms per call (median of event-timed windows after warm-up calls, lowest - highest window in brackets):
``CES._stage`` on the next frame; the stage's step head by head (``fused=False``: ``CE.step_graph`` x 4, ``torch.cat``, the mix
convolution); the fused step (``ops.graph_stage_step``) with and without the graphs; the four heads' features alone; and the fold + mix
kernel (``ops.ces_stage_fold_mix``) against ``fold`` + ``stage_mix`` -- the two launches it replaces: ``ops.fold_normalize`` on the four
heads as a batch, ``ops.ces_stage_mix`` on the stored concat map -- on the same aggregated rows.

    python tools/time_stage_step.py --search [1024 1024]    # the search step of a stage (``CES.search_graphs``), the same two cases

One stage, ``features="split16"``, radius 1, ``propagate``, ``explore=8``: the fused search step (``ops.graph_stage_search_step``) against
head by head (``step_graphs(..., fused=False, propagate=True, explore=8)``), with and without the graphs; its ONE row launch against the
same kernel launched once per head (``head_launches``), on stored features; ``iters=3`` against three ``iters=1`` calls; and, on the whole
module, ``CES.build_graphs`` (4 iterations from the trivial start) against ``CES.forward_with_graphs``.  Noise-like maps carry no spatial
coherence: the times say what a search step costs, not what it finds.

    python tools/time_stage_step.py --fixed [--search] [1024 1024]    # the same stage on a fixed-width state (``FixedGraph``)

``fused="stage"`` (``ops.graph_stage_step_fixed``: the four heads' rows in one row launch, fold + mix in one) against head by head
(``CE.step_graph`` x 4 on the heads' row views, ``FixedGraph.cat``, ``torch.cat``, the mix convolution), each eager and per replayed
frame of a captured HIP graph -- a frame is the stage's step and ``copy_`` of the new graph into the captured one's storage --, with the
stage-fused step on the CSR state (one host read, not capturable with its graph) next to them.  ``--search``: the same with
``propagate``, ``explore=8``.

    python tools/time_stage_step.py --frozen [1024 1024]    # frozen graphs (``CES.forward_on_graphs``), the same two cases

One stage and the whole ``CES`` on graphs that do not move, head by head against ``fused=True`` (``ops.graph_stage_forward``; under
autograd ``ce._GraphStageForward``), the two legs of every line interleaved window by window: without a gradient on ``"fp32"``,
``"split16"`` and ``"stage16"`` (the last against head by head on ``"split16"``: it has no head-by-head form), a training step
(forward + backward, ``backward="fused"``) on ``"fp32"`` and ``"split16"``, and what the ``torch.stack`` of the per-head operands costs.

Every table also has the ``features="stage16"`` column (``ops.graph_stage_features16``: the four heads' prologue and projections in one
launch each) next to ``"split16"``: the features alone, the fused step with and without the graphs, the fused search step, and
``--fixed [--search]`` eager and replayed.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, warmup=3, repeats=7, inner=10):
    """Median and spread (ms per call) of ``repeats`` event-timed windows of ``inner`` calls, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / inner)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _case(H, W, big):
    """The module and the two frames of a case -> (name, mode, ces, x, x2)."""
    from dagl_amd.net import CES
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    name, mode, k, variant, gain = ("adaptive AND top-16 (sparse, gain 1.7)", "adaptive_topk", 16, "sparse", 1.7) if big else \
        ("top-k 8", "topk", 8, "default", 1.65)
    torch.manual_seed(3)
    ces = CES(64)
    for i, (s, h) in enumerate((s, h) for s in (1, 2, 3) for h in (1, 2, 3, 4)):
        hd = getattr(ces, f"c{s}_{h}")
        hd.load_state_dict({n: torch.from_numpy(a) for n, a in make_ce_params(7 + i, variant=variant, sparse_gain=gain).items()}, strict=True)
        hd.select_mode, hd.select_k = mode, k
    ces = ces.to(dev).eval()
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    return name, mode, ces, x, torch.roll(x, (1, 1), (2, 3))


def _fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def search_leg(H, W, big):
    from dagl_amd import ops
    from dagl_amd.sequence import SequenceState
    name, mode, ces, x, x2 = _case(H, W, big)
    feat, fmt = "split16", _fmt
    search = dict(propagate=True, explore=8, seed=0)
    with torch.no_grad():
        heads, mix = ces._stage_modules(1)
        graphs = [hd.graph(x) for hd in heads]
        state = SequenceState.from_heads(graphs * 3)          # the state of stage 1 alone is timed
        for g in state.stages:
            g.validate().max_degree()
        for g in graphs:
            g.max_degree()
        plan_u = ces._plan_step(x2, state, 1, feat, True, False, search)[1]
        plan_f = ces._plan_step(x2, state, 1, feat, True, True, search, what="CES.search_graphs")[1]
        # 1. the fused search step against head by head (step_graphs(..., fused=False, propagate=True, explore=8))
        by_head = _events(lambda: ces._step_stage(1, x2, state, plan_u, feat, True, search))
        by_head_alone = _events(lambda: ces._step_stage(1, x2, state, plan_u, feat, False, search))
        fused = _events(lambda: ces._search_stage(1, x2, state, plan_f, 1, feat, True, search))
        alone = _events(lambda: ces._search_stage(1, x2, state, plan_f, 1, feat, False, search))
        # ... and with the stage's features in one pass (features="stage16")
        plan_s = ces._plan_step(x2, state, 1, "stage16", True, True, search, what="CES.search_graphs")[1]
        fused16 = _events(lambda: ces._search_stage(1, x2, state, plan_s, 1, "stage16", True, search))
        alone16 = _events(lambda: ces._search_stage(1, x2, state, plan_s, 1, "stage16", False, search))
        o_u, g_u = ces._step_stage(1, x2, state, plan_u, feat, True, search)
        o_f, g_f = ces._search_stage(1, x2, state, plan_f, 1, feat, True, search)
        same = all(torch.equal(getattr(g_u, n), getattr(g_f, n)) for n in ("row_off", "key", "weight", "score"))
        gap = float((o_u - o_f).abs().max() / o_u.abs().max())
        # 2. the ONE row launch against the same kernel once per head, on stored features, without the graphs (no host read)
        radius, k_eff, margin, longest = plan_f[1]
        feats = [hd._graph_features(x2, margin, True, False) for hd in heads]
        stage = state.stages[0]
        ws = ops.Workspace()
        args = ([f[0].contiguous() for f in feats], [f[1].contiguous() for f in feats], [f[3].contiguous() for f in feats], stage.row_off,
                stage.key, x2.contiguous(), mix.weight.detach().contiguous(), mix.bias.detach().contiguous())
        kw = dict(radius=radius, tau4=[f[2].contiguous() for f in feats] if margin else None, k=k_eff, max_row_edges=longest,
                  want_graph=False, workspace=ws, propagate=True, explore=8, seed=0)
        one = _events(lambda: ops.graph_stage_search_step(*args, **kw), inner=20)
        four = _events(lambda: ops.graph_stage_search_step(*args, head_launches=True, **kw), inner=20)
        # 3. three iterations on features computed once against three calls
        it3 = _events(lambda: ces._search_stage(1, x2, state, plan_f, 3, feat, True, search))

        def three_calls():
            cur = state
            for i in range(3):
                _, g = ces._search_stage(1, x2, cur, plan_f, 1, feat, True, dict(search, seed=i))
                cur = SequenceState([g, state.stages[1], state.stages[2]])

        calls3 = _events(three_calls)
        # 4. a key frame of the whole module: four search iterations from the trivial start against the L N scans
        built = _events(lambda: ces.build_graphs(x2, iters=4, features=feat), inner=3)
        keyframe = _events(lambda: ces.forward_with_graphs(x2), inner=3)
    bound = ops.graph_search_row_bound(longest, radius, True, 8)
    print(f"[1,64,{H},{W}] {name}, search step (radius 1, propagate, explore 8, split16): stage graphs {stage.n_edges} -> {g_f.n_edges} edges "
          f"over 4 heads, largest degree {longest}, row bound {bound} ({'a wavefront' if bound <= 128 else 'a block'} per row)\n"
          f"    search step head by head (step_graphs fused=False) {fmt(by_head)}; without the graphs {fmt(by_head_alone)}\n"
          f"    search step fused {fmt(fused)} = {fused[0] / by_head[0]:.2f} of head by head; without the graphs {fmt(alone)} = "
          f"{alone[0] / by_head_alone[0]:.2f} of head by head; fused graphs equal head by head: {same}; outputs differ by {gap:.1e} of "
          f"the largest\n"
          f"    search step fused, features='stage16' {fmt(fused16)} = {fused16[0] / fused[0]:.2f} of split16; without the graphs {fmt(alone16)} = "
          f"{alone16[0] / alone[0]:.2f} of split16\n"
          f"    ops.graph_stage_search_step on stored features, no graphs: one row launch {fmt(one)}, the same kernel once per head "
          f"{fmt(four)}: {one[0] / four[0]:.2f}\n"
          f"    iters=3 {fmt(it3)} against three iters=1 calls {fmt(calls3)}: {it3[0] / calls3[0]:.2f}\n"
          f"    whole CES: build_graphs(iters=4) {fmt(built)} against forward_with_graphs {fmt(keyframe)}: {built[0] / keyframe[0]:.2f}",
          flush=True)


def stage_leg(H, W, big):
    from dagl_amd import ops
    from dagl_amd.sequence import SequenceState
    name, mode, ces, x, x2 = _case(H, W, big)
    dev, fmt = x.device, _fmt
    feat = "split16"
    with torch.no_grad():
        heads, mix = ces._stage_modules(1)
        graphs = [hd.graph(x) for hd in heads]
        # the state of stage 1 alone is timed: the other two stages hold the same graphs
        state = SequenceState.from_heads(graphs * 3)
        for g in state.stages:
            g.validate().max_degree()
        for g in graphs:
            g.max_degree()
        plan_u = ces._plan_step(x2, state, 1, feat, True, False)[1]
        plan_f = ces._plan_step(x2, state, 1, feat, True, True)[1]
        fwd = _events(lambda: ces._stage(1, x2))
        by_head = _events(lambda: ces._step_stage(1, x2, state, plan_u, feat, True))
        fused = _events(lambda: ces._step_stage(1, x2, state, plan_f, feat, True))
        alone = _events(lambda: ces._step_stage(1, x2, state, plan_f, feat, False))
        by_head_alone = _events(lambda: ces._step_stage(1, x2, state, plan_u, feat, False))
        margin = mode != "topk"
        feats = _events(lambda: [hd._graph_features(x2, margin, True, False) for hd in heads])
        # the stage's features in one pass (features="stage16"): alone, and under the fused step
        plan_s = ces._plan_step(x2, state, 1, "stage16", True, True)[1]
        feats16 = _events(lambda: ces._stage_features(1, x2, margin, "stage16"))
        fused16 = _events(lambda: ces._step_stage(1, x2, state, plan_s, "stage16", True))
        alone16 = _events(lambda: ces._step_stage(1, x2, state, plan_s, "stage16", False))
        o_u, g_u = ces._step_stage(1, x2, state, plan_u, feat, True)
        o_f, g_f = ces._step_stage(1, x2, state, plan_f, feat, True)
        same = all(torch.equal(getattr(g_u, n), getattr(g_f, n)) for n in ("row_off", "key", "weight", "score"))
        gap = float((o_u - o_f).abs().max() / o_u.abs().max())
        # the last kernel against the two launches it replaces, on the aggregated rows of a step: seeded rows of the same shape
        L = g_f.L
        agg = torch.randn(4, 1, L, 784, device=dev)
        mw, mb = mix.weight.detach().reshape(64, 64).contiguous(), mix.bias.detach().contiguous()
        k_fm = _events(lambda: ops.ces_stage_fold_mix(agg, x2, mw, mb), inner=20)
        rows = agg.view(4, L, 784)                   # the four heads as a batch of four: at B = 1 its fold IS the [1,64,H,W] concat map
        cat = ops.fold_normalize(rows, H, W).view(1, 64, H, W)
        k_two = _events(lambda: ops.ces_stage_mix(ops.fold_normalize(rows, H, W).view(1, 64, H, W), x2, mw, mb), inner=20)
        k_fold = _events(lambda: ops.fold_normalize(rows, H, W), inner=20)
        k_mix = _events(lambda: ops.ces_stage_mix(cat, x2, mw, mb), inner=20)
    print(f"[1,64,{H},{W}] {name}: stage graphs {g_f.n_edges} edges over 4 heads, largest degree {state.stages[0].max_degree()}\n"
          f"    CES._stage(x2) {fmt(fwd)}\n"
          f"    step head by head (fused=False, radius 1, split16) {fmt(by_head)}; without the graphs {fmt(by_head_alone)}\n"
          f"    step fused {fmt(fused)} = {fused[0] / by_head[0]:.2f} of head by head, {fused[0] / fwd[0]:.2f} of _stage; without the graphs "
          f"{fmt(alone)} = {alone[0] / by_head_alone[0]:.2f} of head by head, {alone[0] / fwd[0]:.2f} of _stage\n"
          f"    the four heads' features alone {fmt(feats)}; fused graphs equal head by head: {same}; outputs differ by {gap:.1e} of the largest\n"
          f"    features='stage16': the features alone {fmt(feats16)} = {feats16[0] / feats[0]:.2f} of split16; step fused {fmt(fused16)} = "
          f"{fused16[0] / fused[0]:.2f} of split16; without the graphs {fmt(alone16)} = {alone16[0] / alone[0]:.2f} of split16\n"
          f"    ops.ces_stage_fold_mix {fmt(k_fm)} against fold + stage_mix {fmt(k_two)} (fold alone {fmt(k_fold)}, stage_mix alone "
          f"{fmt(k_mix)}): {k_fm[0] / k_two[0]:.2f} of the two launches", flush=True)


def fixed_leg(H, W, big, search_on):
    from dagl_amd.graph import FixedGraph
    from dagl_amd.sequence import SequenceState
    name, mode, ces, x, x2 = _case(H, W, big)
    feat, fmt = "split16", _fmt
    search = dict(propagate=True, explore=8, seed=0) if search_on else dict(propagate=False, explore=0, seed=0)
    with torch.no_grad():
        heads, mix = ces._stage_modules(1)
        graphs = [hd.graph(x) for hd in heads]
        state = SequenceState.from_heads(graphs * 3)          # the state of stage 1 alone is timed
        for g in state.stages:
            g.validate().max_degree()
        width = heads[0].select_k
        fixed = state.to_fixed(width)
        plan = ces._plan_fixed("CES.step_graphs", x2, fixed, 1, feat, "stage", search)[1]
        B = x.shape[0]

        def by_heads(x_in, stage):
            pairs = [hd.step_graph(x_in, stage.images(h * B, (h + 1) * B), radius=1, features=feat, **search) for h, hd in enumerate(heads)]
            return mix(torch.cat([o for o, _ in pairs], dim=1)) + x_in, FixedGraph.cat([g for _, g in pairs])

        def fused(x_in, stage):
            return ces._stage_fixed_fused(1, x_in, stage, plan, feat, search, 1)

        def frames(form):
            """(eager, replayed) ms per frame: the step and the copy of its graph into the stage's storage."""
            g0 = fixed.stages[0]
            stage = g0._like(g0.key.clone(), g0.weight.clone(), g0.score.clone(), g0.deg.clone())
            x_in = x2.clone()
            eager = _events(lambda: stage.copy_(form(x_in, stage)[1]))
            stage.copy_(g0)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out, g = form(x_in, stage)
                stage.copy_(g)
            return eager, _events(graph.replay)

        o_u, g_u = by_heads(x2, fixed.stages[0])
        o_f, g_f = fused(x2, fixed.stages[0])
        same = all(torch.equal(getattr(g_u, n), getattr(g_f, n)) for n in ("key", "weight", "score", "deg"))
        gap = float((o_u - o_f).abs().max() / o_u.abs().max())
        heads_eager, heads_replay = frames(by_heads)
        fused_eager, fused_replay = frames(fused)
        # ... and with the stage's features in one pass (features="stage16")
        plan16 = ces._plan_fixed("CES.step_graphs", x2, fixed, 1, "stage16", "stage", search)[1]
        fused16_eager, fused16_replay = frames(lambda x_in, stage: ces._stage_fixed_fused(1, x_in, stage, plan16, "stage16", search, 1))
        o_s, _g = ces._stage_fixed_fused(1, x2, fixed.stages[0], plan16, "stage16", search, 1)
        gap16 = float((o_s - o_f).abs().max() / o_f.abs().max())
        if search_on:
            plan_c = ces._plan_step(x2, state, 1, feat, True, True, search, what="CES.search_graphs")[1]
            csr = _events(lambda: ces._search_stage(1, x2, state, plan_c, 1, feat, True, search))
        else:
            plan_c = ces._plan_step(x2, state, 1, feat, True, True)[1]
            csr = _events(lambda: ces._step_stage(1, x2, state, plan_c, feat, True))
    what = "search step (propagate, explore 8)" if search_on else "step"
    print(f"[1,64,{H},{W}] {name}, {what} of one stage on a fixed-width state ({width} slots per row, radius 1, split16), per frame = the "
          f"step + copy_ of its graph\n"
          f"    head by head: eager {fmt(heads_eager)}, replayed {fmt(heads_replay)}\n"
          f"    fused='stage': eager {fmt(fused_eager)} = {fused_eager[0] / heads_eager[0]:.2f} of head by head, replayed {fmt(fused_replay)} = "
          f"{fused_replay[0] / heads_replay[0]:.2f} of head by head; graphs equal head by head: {same}; outputs differ by {gap:.1e} of the "
          f"largest\n"
          f"    fused='stage', features='stage16': eager {fmt(fused16_eager)} = {fused16_eager[0] / fused_eager[0]:.2f} of split16, replayed "
          f"{fmt(fused16_replay)} = {fused16_replay[0] / fused_replay[0]:.2f} of split16; outputs differ from split16 by {gap16:.1e} of the largest\n"
          f"    the stage-fused {what} on the CSR state, eager with its graph (one host read): {fmt(csr)}", flush=True)


def _interleaved(fns, warmup=2, rounds=7, inner=3):
    """``_events`` for legs that are compared with each other: every round times each leg once, in turn, so that a drift of the
    clocks or of the device's state meets all of them alike -> [(median, lowest, highest) ms per call] per leg."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for fn, ts in zip(fns, times):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1) / inner)
    return [(sorted(ts)[len(ts) // 2], min(ts), max(ts)) for ts in times]


def frozen_leg(H, W, big):
    """``CES.forward_on_graphs``: one stage and the whole module on frozen graphs, head by head against ``fused=True``."""
    from dagl_amd.sequence import SequenceState
    name, mode, ces, x, x2 = _case(H, W, big)
    fmt = _fmt
    margin = mode != "topk"
    with torch.no_grad():
        heads, mix = ces._stage_modules(1)
        graphs = [hd.graph(x) for hd in heads]
        state = SequenceState.from_heads(graphs * 3)          # every stage runs on the graphs of stage 1
        for g in state.stages:
            g.validate().transpose()
        for g in graphs:
            g.validate().transpose()
        stage = state.stages[0]

    def stage_by_head(feat, backward="two_ops"):
        outs = [hd.forward_on_graph(x2, state.head(0, h), features=feat, backward=backward) for h, hd in enumerate(heads)]
        return mix(torch.cat(outs, dim=1)) + x2

    def train(forward):
        def step():
            ces.zero_grad(set_to_none=True)
            forward().square().sum().backward()
        return step

    print(f"[1,64,{H},{W}] {name}, frozen graphs: stage graph {stage.n_edges} edges over 4 heads; ms per call, legs of a line interleaved",
          flush=True)
    with torch.no_grad():
        for feat in ("fp32", "split16"):
            by_head, fused = _interleaved([lambda: stage_by_head(feat), lambda: ces._stage_forward_fused(1, x2, stage, margin, feat)])
            gap = float((stage_by_head(feat) - ces._stage_forward_fused(1, x2, stage, margin, feat)).abs().max() / stage_by_head(feat).abs().max())
            print(f"    one stage, no grad, {feat}: head by head {fmt(by_head)}, fused=True {fmt(fused)} = {fused[0] / by_head[0]:.2f}; outputs "
                  f"differ by {gap:.1e} of the largest", flush=True)
        by_head, fused = _interleaved([lambda: stage_by_head("split16"), lambda: ces._stage_forward_fused(1, x2, stage, margin, "stage16")])
        print(f"    one stage, no grad, stage16: fused=True {fmt(fused)} = {fused[0] / by_head[0]:.2f} of head by head on split16 {fmt(by_head)}",
              flush=True)
        for feat in ("fp32", "split16"):
            by_head, fused = _interleaved([lambda: ces.forward_on_graphs(x2, state, features=feat),
                                           lambda: ces.forward_on_graphs(x2, state, features=feat, fused=True)])
            print(f"    whole CES, no grad, {feat}: head by head {fmt(by_head)}, fused=True {fmt(fused)} = {fused[0] / by_head[0]:.2f}", flush=True)
        by_head, fused = _interleaved([lambda: ces.forward_on_graphs(x2, state, features="split16"),
                                       lambda: ces.forward_on_graphs(x2, state, features="stage16", fused=True)])
        print(f"    whole CES, no grad, stage16: fused=True {fmt(fused)} = {fused[0] / by_head[0]:.2f} of head by head on split16 {fmt(by_head)}",
              flush=True)
        # what the stack of the per-head features costs (the stage-fused kernels take one head-major array per operand)
        feats = ces._stage_features(1, x2, margin, "split16")
        stack = _events(lambda: [torch.stack([f[i] for f in feats]) for i in ((0, 1, 2, 3) if margin else (0, 1, 3))])
        print(f"    torch.stack of the four heads' operands (wq, x, b2p" + (", tau" if margin else "") + f"): {fmt(stack)}", flush=True)
        del feats
    for feat in ("fp32", "split16"):
        by_head, fused = _interleaved([train(lambda: stage_by_head(feat, "fused")),
                                       train(lambda: ces._stage_forward_fused(1, x2, stage, margin, feat))])
        print(f"    one stage, training step (forward + backward, backward='fused'), {feat}: head by head {fmt(by_head)}, fused=True {fmt(fused)} "
              f"= {fused[0] / by_head[0]:.2f}", flush=True)
        by_head, fused = _interleaved([train(lambda: ces.forward_on_graphs(x2, state, features=feat, backward="fused")),
                                       train(lambda: ces.forward_on_graphs(x2, state, features=feat, backward="fused", fused=True))])
        print(f"    whole CES, training step, {feat}: head by head {fmt(by_head)}, fused=True {fmt(fused)} = {fused[0] / by_head[0]:.2f}", flush=True)


def main():
    search = "--search" in sys.argv[1:]
    argv = [a for a in sys.argv[1:] if a not in ("--search", "--fixed", "--frozen")]
    if "--frozen" in sys.argv[1:]:
        return frozen_leg(int(argv[0]), int(argv[1]), True) if len(argv) > 1 else frozen_leg(256, 256, False)
    if "--fixed" in sys.argv[1:]:
        return fixed_leg(int(argv[0]), int(argv[1]), True, search) if len(argv) > 1 else fixed_leg(256, 256, False, search)
    leg = search_leg if search else stage_leg
    if len(argv) > 1:
        return leg(int(argv[0]), int(argv[1]), True)
    return leg(256, 256, False)


if __name__ == "__main__":
    main()
