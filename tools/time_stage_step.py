"""What a sequence step of one ``CES`` stage costs (``CES.step_graphs``, dagl_amd/net.py) next to the stage's own forward.

    python tools/time_stage_step.py            # a stage input of [1,64,256,256], top-k 8
    python tools/time_stage_step.py 1024 1024  # with a size: adaptive AND top-16 on the sparse variant (the benchmark's 1024^2 regime)

Per case, ms per call (median of event-timed windows after warm-up calls, lowest - highest window in brackets):
``CES._stage`` on the next frame; the stage's step head by head (``fused=False``: ``CE.step_graph`` x 4, ``torch.cat``, the mix
convolution); the fused step (``ops.graph_stage_step``) with and without the graphs; the four heads' features alone; and the fold + mix
kernel (``ops.ces_stage_fold_mix``) against ``fold`` + ``stage_mix`` -- the two launches it replaces: ``ops.fold_normalize`` on the four
heads as a batch, ``ops.ces_stage_mix`` on the stored concat map -- on the same aggregated rows.
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


def stage_leg(H, W, big):
    from dagl_amd import ops
    from dagl_amd.net import CES
    from dagl_amd.sequence import SequenceState
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
    x2 = torch.roll(x, (1, 1), (2, 3))
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
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
          f"    ops.ces_stage_fold_mix {fmt(k_fm)} against fold + stage_mix {fmt(k_two)} (fold alone {fmt(k_fold)}, stage_mix alone "
          f"{fmt(k_mix)}): {k_fm[0] / k_two[0]:.2f} of the two launches", flush=True)


def main():
    if len(sys.argv) > 2:
        return stage_leg(int(sys.argv[1]), int(sys.argv[2]), True)
    return stage_leg(256, 256, False)


if __name__ == "__main__":
    main()
