"""What ``CE.graph`` costs next to the forward of the same call (a diagnostic path: the number is for users, not a target).

    python tools/time_patch_graph.py [H W]          # default 256 256: top-k 8 and the dense adaptive regime
    python tools/time_patch_graph.py --apply [H W]  # what ``CE.apply_graph`` costs: forward / graph / apply / apply + backward
    python tools/time_patch_graph.py --attend [H W] # what ``CE.attend_graph`` / ``forward_on_graph`` cost on the same three graphs
    python tools/time_patch_graph.py --lists [H W]  # what ``CE.forward_with_graph`` costs next to forward + graph, same three graphs
    python tools/time_patch_graph.py --refresh [H W]  # ``CE.refresh_graph`` + ``forward_on_graph`` on a next frame next to ``forward``:
                                                      # top-k 8 at 256 256; with a size (1024 1024) adaptive AND top-16
    python tools/time_patch_graph.py --step [H W]     # ``CE.step_graph`` (with and without the graph) next to that two-call sequence and
                                                      # to ``forward``, the same two cases
    python tools/time_patch_graph.py --train-graph [H W]  # training on a frozen graph: the fused forward / backward next to the two
                                                          # ops and their backwards, ops alone and through ``forward_on_graph``
    python tools/time_patch_graph.py --search [H W]   # the search step: ``refresh_graph`` alone, + propagate, + explore 8, both, on a
                                                      # shifted frame -- time and recall against ``graph``; ``build_graph`` per
                                                      # iteration next to the forward that selects; the two cases of --refresh
    python tools/time_patch_graph.py --fixed [H W]    # the step on a ``FixedGraph`` (eager, and replayed from a captured HIP graph with
                                                      # ``g.copy_(g_new)`` inside) next to the CSR step with and without its graph;
                                                      # interleaved repeats; the two cases of --refresh
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _events(fn, warmup=3, repeats=5, inner=10):
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


def _interleaved(legs, warmup=3, repeats=7, inner=10):
    """``_events`` for several legs measured in turn -- every repeat times each leg once, so that a drift of the clocks meets all of them
    alike -> {name: (median, min, max)} in ms per call."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / inner)
    out = {}
    for name, t in times.items():
        t.sort()
        out[name] = (t[len(t) // 2], t[0], t[-1])
    return out


def _long_tailed(g, n_rows=16):
    """``g`` with every key once (weight 1 / N) in the place of ``n_rows`` of its rows, spread over the row range."""
    from dagl_amd.graph import PatchGraph
    dev = g.key.device
    deg = g.degrees().reshape(-1).clone()
    picked = torch.linspace(0, deg.numel() - 1, n_rows, device=dev).long()
    keep = torch.ones(g.n_edges, dtype=torch.bool, device=dev)
    keep[torch.isin(g.rows(), picked)] = False
    rows = torch.cat([g.rows()[keep], picked.repeat_interleave(g.N)])
    key = torch.cat([g.key[keep], torch.arange(g.N, dtype=torch.int32, device=dev).repeat(n_rows)])
    weight = torch.cat([g.weight[keep], torch.full((n_rows * g.N,), 1.0 / g.N, device=dev)])
    order = torch.sort(rows, stable=True).indices
    deg[picked] = g.N
    row_off = torch.cat([deg.new_zeros(1), deg.cumsum(0)])
    return PatchGraph(row_off, key[order].contiguous(), weight[order].contiguous(), None, g.B, g.H, g.W, g.mode, g.k)


def apply_leg(H, W):
    """forward / graph / apply_graph(graph) / apply_graph forward + backward of one module and input, and the gather's algorithmic
    bytes per second: E * (3136 + 8) -- an edge's 784 value floats, its key and its weight -- over the time of ``ops.graph_apply``
    alone (the value map given: no theta convolution in the window)."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    for name, mode, k, variant, tail in _table_cases():
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            g = ce.graph(x)
            if tail:
                g = _long_tailed(g)
            g.validate()
            fwd = _events(lambda: ce(x))
            exp = _events(lambda: ce.graph(x), warmup=1, repeats=3, inner=2)
            app = _events(lambda: ce.apply_graph(x, g))
            b2p = ops.ce_prologue(x, *(ce._params_f32()[n] for n in ("g.weight", "g.bias", "theta.weight", "theta.bias")))[1]
            ws = ops.Workspace()
            ker = _events(lambda: ops.graph_apply(b2p, g.row_off, g.key, g.weight, workspace=ws))
        xg = x.clone().requires_grad_(True)
        gw = g.with_weight(g.weight.clone().requires_grad_(True))
        g.transpose()

        def both():
            ce.apply_graph(xg, gw).sum().backward()
            xg.grad = gw.weight.grad = None
            ce.zero_grad(set_to_none=True)
        fb = _events(both, repeats=3, inner=5)
        gbs = g.n_edges * (3136 + 8) / (ker[0] * 1e-3) / 1e12
        fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
        print(f"[1,64,{H},{W}] {name}: {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {int(g.degrees().max())}\n"
              f"    forward {fmt(fwd)}; graph {fmt(exp)}; apply_graph(graph) {fmt(app)}; apply_graph forward + backward {fmt(fb)}\n"
              f"    ops.graph_apply alone {fmt(ker)}: {gbs:.2f} TB/s of E * (3136 + 8) algorithmic bytes", flush=True)


def _table_cases():
    return (("top-k 8", "topk", 8, "default", False), ("sparse adaptive (gain 1.65)", "adaptive", 0, "sparse", False),
            ("top-k 8 + 16 rows of degree N", "topk", 8, "default", True))


def attend_leg(H, W):
    """forward / attend_graph / forward_on_graph (fp32 features; split-fp16 features with the two ops and fused; fp32 features fused) /
    forward_on_graph forward + backward on the three graphs of ``apply_leg``, the ops calls alone (features given), and the module's own training path (``_forward_train`` forward, forward + backward) to compare with."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    for name, mode, k, variant, tail in _table_cases():
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            g = ce.graph(x)
            if tail:
                g = _long_tailed(g)
            g.validate()
            g.transpose()
            fwd = _events(lambda: ce(x))
            att = _events(lambda: ce.attend_graph(x, g))
            fog = _events(lambda: ce.forward_on_graph(x, g))
            f16 = _events(lambda: ce.forward_on_graph(x, g, features="split16", fused=False))
            f16f = _events(lambda: ce.forward_on_graph(x, g, features="split16"))
            f32f = _events(lambda: ce.forward_on_graph(x, g, fused=True))
            # the two ops calls alone, on the module's own features
            from dagl_amd import train_ops as T
            p = ce._params_f32(scaled=False)
            b1p = ops.ce_prologue(x, p["g.weight"], p["g.bias"], p["theta.weight"], p["theta.bias"])[0]
            wq = T.patch_linear(b1p, T.fc_weight_rows(p["fc1.0.weight"], 16, 7), p["fc1.0.bias"], 7, 4, T._head_grid(H, W)[0],
                                T._head_grid(H, W)[1], -(-H // 4), -(-W // 4), relu=True, allow_fast=False).contiguous()
            xk = T.patch_linear(b1p, T.fc_weight_rows(p["fc2.0.weight"], 16, 7), p["fc2.0.bias"], 7, 1, 0, 0, H, W, relu=True,
                                allow_fast=False).contiguous()
            tau = None
            if mode != "topk":
                heads = ops.ce_prologue(x, *(p[n] for n in ("g.weight", "g.bias", "theta.weight", "theta.bias", "thr_conv.weight",
                                                             "thr_conv.bias", "bias_conv.weight", "bias_conv.bias")))
                tau = (torch.bmm(wq, xk.mean(dim=1).unsqueeze(2)).squeeze(2) * heads[2].reshape(1, -1) - heads[3].reshape(1, -1)).contiguous()
            ws, wsb = ops.Workspace(), ops.Workspace()
            call = dict(tau=tau, scale=float(ce.softmax_scale), hw=(H, W))
            k_f = _events(lambda: ops.graph_attend(wq, xk, g.row_off, g.key, workspace=ws, **call))
            weight, score = ops.graph_attend(wq, xk, g.row_off, g.key, workspace=ws, **call)
            b2p = ops.ce_prologue(x, p["g.weight"], p["g.bias"], p["theta.weight"], p["theta.bias"])[1]
            wsa, wsf = ops.Workspace(), ops.Workspace()
            k_a = _events(lambda: ops.graph_apply(b2p, g.row_off, g.key, weight, workspace=wsa))
            fcall = dict(tau=tau, scale=float(ce.softmax_scale))
            k_ff = _events(lambda: ops.graph_forward(wq, xk, b2p, g.row_off, g.key, workspace=wsf, **fcall))
            d_w = torch.randn_like(weight)
            k_b = _events(lambda: ops.graph_attend_backward(d_w, wq, xk, g.row_off, g.key, score, weight, transposed=g.transpose(),
                                                            workspace=wsb, **call))
        xg = x.clone().requires_grad_(True)

        def both():
            ce.forward_on_graph(xg, g).sum().backward()
            xg.grad = None
            ce.zero_grad(set_to_none=True)
        fb = _events(both, repeats=5, inner=5)
        ce.train()
        with torch.no_grad():
            trf = _events(lambda: ce._forward_train(x))

        def train_both():
            ce._forward_train(xg).sum().backward()
            xg.grad = None
            ce.zero_grad(set_to_none=True)
        trb = _events(train_both, repeats=5, inner=5)
        ce.eval()
        print(f"[1,64,{H},{W}] {name}: {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {int(g.degrees().max())}\n"
              f"    forward {fmt(fwd)}; attend_graph {fmt(att)}; forward_on_graph {fmt(fog)}; forward_on_graph forward + backward {fmt(fb)}\n"
              f"    forward_on_graph split16, two ops {fmt(f16)}; split16 fused {fmt(f16f)}; fp32 features fused {fmt(f32f)}\n"
              f"    ops.graph_attend alone {fmt(k_f)}; ops.graph_apply alone {fmt(k_a)}; ops.graph_forward alone {fmt(k_ff)}; "
              f"ops.graph_attend_backward alone {fmt(k_b)}\n"
              f"    the module's own training path (_forward_train, its own selection): forward {fmt(trf)}; forward + backward {fmt(trb)}",
              flush=True)


def lists_leg(H, W):
    """forward / graph / forward_with_graph (split-fp16 and fp32 features) / ops.graph_from_lists alone (the lists given) /
    forward_with_graph followed by forward_on_graph(features="split16") on its result, on the three graphs of ``apply_leg``.  The
    call serves what the neighbour lists hold (64 keys per query): a graph beyond that is refused, and the line says so."""
    from dagl_amd import DaglError, ops
    from dagl_amd import train_ops as T
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    for name, mode, k, variant, tail in _table_cases():
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            g = ce.graph(x)
            head = f"[1,64,{H},{W}] {name}: {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {int(g.degrees().max())}"
            if tail:
                print(f"{head} before the edit\n    refused: rows of degree N are written by hand, no forward produces them and no neighbour "
                      "list holds them; forward_with_graph on this module returns the top-k 8 graph of the first table", flush=True)
                continue
            try:
                ce.forward_with_graph(x)
            except DaglError as e:
                print(f"{head}\n    refused (code {e.code}): {e}", flush=True)
                continue
            fwd = _events(lambda: ce(x))
            exp = _events(lambda: ce.graph(x), warmup=1, repeats=3, inner=2)
            w16 = _events(lambda: ce.forward_with_graph(x, features="split16"))
            w32 = _events(lambda: ce.forward_with_graph(x, features="fp32"))
            chain = _events(lambda: ce.forward_on_graph(x, ce.forward_with_graph(x, features="split16")[1], features="split16"))
            # the conversion alone, on the lists of a core call on the module's own fp32 features
            p = ce._params_f32(scaled=False)
            heads = mode != "topk"
            maps = ops.ce_prologue(x, *(p[n] for n in ("g.weight", "g.bias", "theta.weight", "theta.bias")
                                        + (("thr_conv.weight", "thr_conv.bias", "bias_conv.weight", "bias_conv.bias") if heads else ())))
            wq = T.patch_linear(maps[0], T.fc_weight_rows(p["fc1.0.weight"], 16, 7), p["fc1.0.bias"], 7, 4, T._head_grid(H, W)[0],
                                T._head_grid(H, W)[1], -(-H // 4), -(-W // 4), relu=True, allow_fast=False).contiguous()
            xk = T.patch_linear(maps[0], T.fc_weight_rows(p["fc2.0.weight"], 16, 7), p["fc2.0.bias"], 7, 1, 0, 0, H, W, relu=True,
                                allow_fast=False).contiguous()
            b2 = maps[1][:, 3:3 + H, 3:3 + W, :].permute(0, 3, 1, 2).contiguous()
            _, s = ops.ce_core_forward(wq, xk, b2, maps[2] if heads else None, maps[3] if heads else None, mode=mode, k=k, exact_scan=True)
            ws = ops.Workspace()
            conv = _events(lambda: ops.graph_from_lists(s["nb_idx"], s["nb_wgt"], None, s["nb_cnt"], (H, W), workspace=ws))
        both = fwd[0] + exp[0]
        print(f"{head}\n    forward {fmt(fwd)}; graph {fmt(exp)}; forward + graph {both:.3f} ms\n"
              f"    forward_with_graph split16 {fmt(w16)} = {w16[0] / both:.2f} of forward + graph; fp32 {fmt(w32)} = {w32[0] / both:.2f}\n"
              f"    ops.graph_from_lists alone {fmt(conv)}; forward_with_graph + forward_on_graph(split16) on its graph {fmt(chain)}", flush=True)


def refresh_leg(H, W, big):
    """A sequence step: the graph of one frame moved to the next (``refresh_graph``, radius 1, split-fp16 features) and used
    (``forward_on_graph(features="split16")``), next to ``forward`` on the next frame -- top-k 8, or (``big``: a size was given)
    adaptive AND top-16 on the sparse variant of the benchmark's 1024^2 configuration.  The next frame is the input rolled by one
    pixel each way.  ``ops.graph_refresh`` alone (features given) at radius 0 / 1 / 2, a wavefront and a block per row, and the recall of
    the refreshed structure against ``graph`` of the next frame."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    x2 = torch.roll(x, (1, 1), (2, 3))
    name, mode, k, variant, gain = ("adaptive AND top-16 (sparse, gain 1.7)", "adaptive_topk", 16, "sparse", 1.7) if big else \
        ("top-k 8", "topk", 8, "default", 1.65)
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=gain).items()}
    ce = CE(in_channels=64)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode, ce.select_k = mode, k
    ce = ce.to(dev).eval()
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    with torch.no_grad():
        g = ce.graph(x)
        g.max_degree()
        full = ce.graph(x2)
        fwd = _events(lambda: ce(x2))
        ref = _events(lambda: ce.refresh_graph(x2, g, radius=1, features="split16"))
        g2 = ce.refresh_graph(x2, g, radius=1, features="split16")
        fog = _events(lambda: ce.forward_on_graph(x2, g2, features="split16"))
        chain = _events(lambda: ce.forward_on_graph(x2, ce.refresh_graph(x2, g, radius=1, features="split16"), features="split16"))
        wq, xk, tau, _, _ = ce._graph_features(x2, mode != "topk", True, False)
        wq, xk, tau = wq.contiguous(), xk.contiguous(), (tau.contiguous() if tau is not None else None)
        ws = ops.Workspace()
        call = dict(tau=tau, k=k, scale=float(ce.softmax_scale), max_row_edges=g.max_degree(), workspace=ws, hw=(H, W))
        alone, stats = {}, {}
        full_keys = full.rows() * full.N + full.key.long()
        for radius in (0, 1, 2):
            for block in (False, True):
                alone[(radius, block)] = _events(lambda: ops.graph_refresh(wq, xk, g.row_off, g.key, radius=radius, block_rows=block, **call))
            r = ce.refresh_graph(x2, g, radius=radius, features="split16")
            hit = torch.isin(r.rows() * r.N + r.key.long(), full_keys).sum()
            dil = ops.graph_refresh(wq, xk, g.row_off, g.key, radius=radius, keep_all=True, **call)
            stats[radius] = (r.n_edges, int(hit) / max(full.n_edges, 1), dil["key"].numel() / g.L)
    print(f"[1,64,{H},{W}] {name}: graph(x) {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {g.max_degree()}; graph(x2) {full.n_edges} edges\n"
          f"    forward(x2) {fmt(fwd)}; refresh_graph(x2, graph(x), radius 1, split16) {fmt(ref)}; forward_on_graph(x2, refreshed, split16) "
          f"{fmt(fog)}; refresh_graph + forward_on_graph {fmt(chain)} = {chain[0] / fwd[0]:.2f} of forward", flush=True)
    for radius in (0, 1, 2):
        edges, recall, cands = stats[radius]
        print(f"    radius {radius}: {cands:.1f} candidates per row, {edges} edges, recall against graph(x2) {recall:.3f}; ops.graph_refresh alone "
              f"{fmt(alone[(radius, False)])}, a block per row {fmt(alone[(radius, True)])}", flush=True)


def step_leg(H, W, big):
    """A sequence step in one call (``step_graph``, radius 1, split-fp16 features, with and without the graph) next to the two-call
    sequence ``refresh_graph`` + ``forward_on_graph`` and to ``forward`` on the next frame, in one process: the cases and the protocol
    of ``refresh_leg``.  ``ops.graph_step`` alone (features given), a wavefront and a block per row, next to ``ops.graph_refresh`` +
    ``ops.graph_forward`` on the same features."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    x2 = torch.roll(x, (1, 1), (2, 3))
    name, mode, k, variant, gain = ("adaptive AND top-16 (sparse, gain 1.7)", "adaptive_topk", 16, "sparse", 1.7) if big else \
        ("top-k 8", "topk", 8, "default", 1.65)
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=gain).items()}
    ce = CE(in_channels=64)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode, ce.select_k = mode, k
    ce = ce.to(dev).eval()
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    f16 = dict(radius=1, features="split16")
    with torch.no_grad():
        g = ce.graph(x)
        g.max_degree()
        fwd = _events(lambda: ce(x2))
        chain = _events(lambda: ce.forward_on_graph(x2, ce.refresh_graph(x2, g, **f16), features="split16"))
        both = _events(lambda: ce.step_graph(x2, g, **f16))
        alone = _events(lambda: ce.step_graph(x2, g, want_graph=False, **f16))
        out, g2 = ce.step_graph(x2, g, **f16)
        two = ce.forward_on_graph(x2, g2, features="split16")
        gap = float((out - two).abs().max() / two.abs().max())
        wq, xk, tau, b2p, _ = ce._graph_features(x2, mode != "topk", True, False)
        wq, xk, b2p, tau = wq.contiguous(), xk.contiguous(), b2p.contiguous(), (tau.contiguous() if tau is not None else None)
        feats = _events(lambda: ce._graph_features(x2, mode != "topk", True, False))
        ws, wsr, wsf = ops.Workspace(), ops.Workspace(), ops.Workspace()
        call = dict(radius=1, tau=tau, k=k, scale=float(ce.softmax_scale), max_row_edges=g.max_degree())
        k_step = {(w, blk): _events(lambda: ops.graph_step(wq, xk, b2p, g.row_off, g.key, want_graph=w, block_rows=blk, workspace=ws, **call))
                  for w in (True, False) for blk in (False, True)}
        k_ref = _events(lambda: ops.graph_refresh(wq, xk, g.row_off, g.key, workspace=wsr, hw=(H, W), **call))
        k_fwd = _events(lambda: ops.graph_forward(wq, xk, b2p, g2.row_off, g2.key, tau=tau, scale=float(ce.softmax_scale), workspace=wsf))
    print(f"[1,64,{H},{W}] {name}: graph(x) {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {g.max_degree()}; stepped to x2 "
          f"{g2.n_edges} edges\n"
          f"    forward(x2) {fmt(fwd)}; refresh_graph + forward_on_graph (radius 1, split16) {fmt(chain)}\n"
          f"    step_graph {fmt(both)} = {both[0] / chain[0]:.2f} of the two calls, {both[0] / fwd[0]:.2f} of forward; "
          f"step_graph(want_graph=False) {fmt(alone)} = {alone[0] / chain[0]:.2f} of the two calls, {alone[0] / fwd[0]:.2f} of forward\n"
          f"    step_graph out against forward_on_graph on its graph: {gap:.1e} normwise; the features alone (_graph_features) {fmt(feats)}\n"
          f"    ops.graph_step alone {fmt(k_step[(True, False)])}, a block per row {fmt(k_step[(True, True)])}; without the graph "
          f"{fmt(k_step[(False, False)])}, a block per row {fmt(k_step[(False, True)])}; ops.graph_refresh alone {fmt(k_ref)}; "
          f"ops.graph_forward alone on the result {fmt(k_fwd)}", flush=True)


def fixed_leg(H, W, big):
    """One head, a next frame, radius 1, split-fp16 features (the cases of ``step_leg``): ``step_graph`` on the CSR with and without its
    graph, on the ``FixedGraph`` eager, and the fixed step replayed from a captured HIP graph that holds ``out, g_new = step_graph(x, g);
    g.copy_(g_new)`` -- the form a sequence runs per frame.  Then the library calls alone on given features.  Interleaved repeats."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    x2 = torch.roll(x, (1, 1), (2, 3))
    name, mode, k, variant, gain = ("adaptive AND top-16 (sparse, gain 1.7)", "adaptive_topk", 16, "sparse", 1.7) if big else \
        ("top-k 8", "topk", 8, "default", 1.65)
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=gain).items()}
    ce = CE(in_channels=64)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode, ce.select_k = mode, k
    ce = ce.to(dev).eval()
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    f16 = dict(radius=1, features="split16")
    with torch.no_grad():
        g = ce.graph(x)
        g.max_degree()
        fg = g.to_fixed(k)
        out_csr, g_csr = ce.step_graph(x2, g, **f16)
        out_fix, g_fix = ce.step_graph(x2, fg, **f16)
        back = g_fix.to_csr()
        same = torch.equal(out_csr, out_fix) and all(torch.equal(getattr(back, n), getattr(g_csr, n)) for n in ("row_off", "key", "weight"))
        # the captured frame: static input, static graph, the new graph copied over the old one inside the HIP graph
        xs, gs = x2.clone(), fg._like(fg.key.clone(), fg.weight.clone(), fg.score.clone(), fg.deg.clone())
        torch.cuda.synchronize()
        hip_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hip_graph):
            out_s, g_new = ce.step_graph(xs, gs, **f16)
            gs.copy_(g_new)
        hip_graph.replay()
        torch.cuda.synchronize()
        replay_same = torch.equal(out_s, out_fix) and torch.equal(gs.key, g_fix.key)

        def eager_frame():
            o, n = ce.step_graph(xs, gs, **f16)
            gs.copy_(n)

        legs = _interleaved({"csr": lambda: ce.step_graph(x2, g, **f16), "csr_alone": lambda: ce.step_graph(x2, g, want_graph=False, **f16),
                             "fixed": lambda: ce.step_graph(x2, fg, **f16), "fixed_copy": eager_frame, "replay": hip_graph.replay,
                             "features": lambda: ce._graph_features(x2, mode != "topk", True, False)})
        wq, xk, tau, b2p, _ = ce._graph_features(x2, mode != "topk", True, False)
        wq, xk, b2p, tau = wq.contiguous(), xk.contiguous(), b2p.contiguous(), (tau.contiguous() if tau is not None else None)
        ws, wsf = ops.Workspace(), ops.Workspace()
        call = dict(radius=1, tau=tau, k=k, scale=float(ce.softmax_scale))
        lib = _interleaved({
            "csr": lambda: ops.graph_step(wq, xk, b2p, g.row_off, g.key, workspace=ws, max_row_edges=g.max_degree(), **call),
            "csr_alone": lambda: ops.graph_step(wq, xk, b2p, g.row_off, g.key, want_graph=False, workspace=ws, max_row_edges=g.max_degree(),
                                                **call),
            "fixed": lambda: ops.graph_step_fixed(wq, xk, b2p, fg.key, fg.deg, width_out=k, workspace=wsf, **call)})
    print(f"[1,64,{H},{W}] {name}: graph(x) {g.n_edges} edges, degree max {g.max_degree()}, {fg.width} slots per row; the fixed step gives the "
          f"CSR step's bits: {same}; the replayed one: {replay_same}\n"
          f"    step_graph on the CSR, with its graph {fmt(legs['csr'])}; without its graph {fmt(legs['csr_alone'])}\n"
          f"    step_graph on the FixedGraph, eager {fmt(legs['fixed'])} = {legs['fixed'][0] / legs['csr'][0]:.2f} of the CSR step with its "
          f"graph; eager with g.copy_(g_new) {fmt(legs['fixed_copy'])}\n"
          f"    the captured frame (step_graph + g.copy_(g_new)) replayed {fmt(legs['replay'])} = "
          f"{legs['replay'][0] / legs['fixed_copy'][0]:.2f} of the same frame eager, {legs['replay'][0] / legs['csr'][0]:.2f} of the CSR step "
          f"with its graph (the two frames with the copy run on the graph as it moves: {gs.n_edges()} edges after the first frame); "
          f"the features alone (_graph_features) {fmt(legs['features'])}\n"
          f"    the library calls on given features: ops.graph_step with its graph {fmt(lib['csr'])}, without {fmt(lib['csr_alone'])}; "
          f"ops.graph_step_fixed {fmt(lib['fixed'])}", flush=True)


def _recall(r, full):
    """Edges of ``full`` that ``r`` holds, over the edges of ``full`` (as ``refresh_leg`` counts it)."""
    hit = torch.isin(r.rows() * r.N + r.key.long(), full.rows() * full.N + full.key.long()).sum()
    return int(hit) / max(full.n_edges, 1)


def search_leg(H, W, big):
    """The search step (``refresh_graph`` with ``propagate`` / ``explore``, radius 1, split-fp16 features) on the cases of
    ``refresh_leg``.  The next frame is the input rolled by 1 pixel each way (inside the radius) and by 3 (outside it: the plain
    refresh cannot follow); per frame the plain refresh, + propagate, + explore 8 and both: time of the call, edges, recall against
    ``graph`` of that frame; a second and third search step on the same frame (the graph improves from step to step).  Then
    ``build_graph`` (no L N scan, explore 8) per number of iterations: time and recall against ``graph(x)``, next to ``forward`` and
    ``graph`` on the same input."""
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    name, mode, k, variant, gain = ("adaptive AND top-16 (sparse, gain 1.7)", "adaptive_topk", 16, "sparse", 1.7) if big else \
        ("top-k 8", "topk", 8, "default", 1.65)
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=gain).items()}
    ce = CE(in_channels=64)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode, ce.select_k = mode, k
    ce = ce.to(dev).eval()
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    f16 = dict(radius=1, features="split16")
    cases = (("refresh alone", dict()), ("+ propagate", dict(propagate=True)), ("+ explore 8", dict(explore=8, seed=1)),
             ("+ propagate + explore 8", dict(propagate=True, explore=8, seed=1)))
    with torch.no_grad():
        g = ce.graph(x)
        g.max_degree()
        fwd = _events(lambda: ce(x))
        exp = _events(lambda: ce.graph(x), warmup=1, repeats=3, inner=2)
        print(f"[1,64,{H},{W}] {name}: graph(x) {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {g.max_degree()}; forward(x) "
              f"{fmt(fwd)}; graph(x) {fmt(exp)}", flush=True)
        for shift in (1, 3):
            x2 = torch.roll(x, (shift, shift), (2, 3))
            full = ce.graph(x2)
            print(f"    next frame rolled by {shift}: graph(x2) {full.n_edges} edges", flush=True)
            for what, kw in cases:
                t = _events(lambda: ce.refresh_graph(x2, g, **f16, **kw))
                r = ce.refresh_graph(x2, g, **f16, **kw)
                line = f"        {what}: {fmt(t)}, {r.n_edges} edges, recall {_recall(r, full):.3f}"
                if kw:
                    for i in (2, 3):            # further steps on the same frame, a new seed each
                        r = ce.refresh_graph(x2, r, **f16, **dict(kw, seed=i) if "explore" in kw else kw)
                        line += f"; after step {i}: {_recall(r, full):.3f}"
                print(line, flush=True)
        for iters in (1, 2, 4, 8):
            t = _events(lambda: ce.build_graph(x, iters=iters, features="split16"), warmup=1, repeats=3, inner=3)
            b = ce.build_graph(x, iters=iters, features="split16")
            print(f"    build_graph(x, iters={iters}, explore 8): {fmt(t)} = {t[0] / fwd[0]:.2f} of forward, {t[0] / exp[0]:.2f} of graph; "
                  f"{b.n_edges} edges, recall against graph(x) {_recall(b, g):.3f}", flush=True)


def train_graph_leg(H, W):
    """Training on a frozen graph, the three graphs of ``apply_leg``, one process, the protocol of ``attend_leg``.  The ops alone (the
    module's own fp32 features given): ``graph_attend`` + ``graph_apply`` next to ``graph_forward_train``, ``graph_apply_backward`` +
    ``graph_attend_backward`` next to ``graph_forward_backward``.  The module: ``forward_on_graph`` forward + backward with
    ``backward="two_ops"`` and ``"fused"`` on both feature routes, and the module's own ``_forward_train`` forward + backward for
    orientation.  The yardstick of every fused figure is the two-op figure of the same run."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    fmt = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"
    for name, mode, k, variant, tail in _table_cases():
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            g = ce.graph(x)
            if tail:
                g = _long_tailed(g)
            g.validate()
            tr = g.transpose()
            wq, xk, tau, b2p, _ = ce._graph_features(x, mode != "topk", False, False)
            wq, xk, b2p, tau = wq.contiguous(), xk.contiguous(), b2p.contiguous(), (tau.contiguous() if tau is not None else None)
            call = dict(tau=tau, scale=float(ce.softmax_scale))
            ws = [ops.Workspace() for _ in range(6)]
            weight, score = ops.graph_attend(wq, xk, g.row_off, g.key, workspace=ws[0], hw=(H, W), **call)
            _, row_max, row_sum = ops.graph_forward_train(wq, xk, b2p, g.row_off, g.key, workspace=ws[2], **call)
            d_out = torch.randn(1, 16, H, W, device=dev)

            def two_forward():
                w, _ = ops.graph_attend(wq, xk, g.row_off, g.key, workspace=ws[0], hw=(H, W), **call)
                return ops.graph_apply(b2p, g.row_off, g.key, w, workspace=ws[1])

            def two_backward():
                _, d_w = ops.graph_apply_backward(d_out, b2p, g.row_off, g.key, weight, transposed=tr, workspace=ws[3])
                return ops.graph_attend_backward(d_w, wq, xk, g.row_off, g.key, score, weight, transposed=tr, workspace=ws[4], hw=(H, W), **call)
            k_f2 = _events(two_forward)
            k_f1 = _events(lambda: ops.graph_forward_train(wq, xk, b2p, g.row_off, g.key, workspace=ws[2], **call))
            k_b2 = _events(two_backward)
            k_b1 = _events(lambda: ops.graph_forward_backward(d_out, wq, xk, b2p, g.row_off, g.key, row_max, row_sum, transposed=tr,
                                                              workspace=ws[5], **call))
        xg = x.clone().requires_grad_(True)
        module = {}
        for features in ("fp32", "split16"):
            for backward in ("two_ops", "fused"):
                def both():
                    ce.forward_on_graph(xg, g, features=features, backward=backward).sum().backward()
                    xg.grad = None
                    ce.zero_grad(set_to_none=True)
                module[(features, backward)] = _events(both, repeats=5, inner=10)
        ce.train()

        def train_both():
            ce._forward_train(xg).sum().backward()
            xg.grad = None
            ce.zero_grad(set_to_none=True)
        trb = _events(train_both, repeats=5, inner=10)
        ce.eval()
        rows = g.B * g.L
        print(f"[1,64,{H},{W}] {name}: {g.n_edges} edges, degree mean {g.n_edges / g.L:.1f} max {int(g.degrees().max())}\n"
              f"    ops forward: graph_attend + graph_apply {fmt(k_f2)}; graph_forward_train {fmt(k_f1)}\n"
              f"    ops backward: graph_apply_backward + graph_attend_backward {fmt(k_b2)}; graph_forward_backward {fmt(k_b1)}\n"
              f"    forward_on_graph forward + backward, fp32 features: two_ops {fmt(module[('fp32', 'two_ops')])}; fused "
              f"{fmt(module[('fp32', 'fused')])}\n"
              f"    forward_on_graph forward + backward, split16 features: two_ops {fmt(module[('split16', 'two_ops')])}; fused "
              f"{fmt(module[('split16', 'fused')])}\n"
              f"    the module's own training path (_forward_train, its own selection) forward + backward {fmt(trb)}\n"
              f"    kept by autograd between forward and backward: two_ops score + weight = {8 * g.n_edges} B; fused row_max + row_sum = "
              f"{12 * rows} B", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--train-graph":
        return train_graph_leg(*((int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (256, 256)))
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        return search_leg(*((int(sys.argv[2]), int(sys.argv[3]), True) if len(sys.argv) > 3 else (256, 256, False)))
    if len(sys.argv) > 1 and sys.argv[1] == "--fixed":
        return fixed_leg(*((int(sys.argv[2]), int(sys.argv[3]), True) if len(sys.argv) > 3 else (256, 256, False)))
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step_leg(*((int(sys.argv[2]), int(sys.argv[3]), True) if len(sys.argv) > 3 else (256, 256, False)))
    if len(sys.argv) > 1 and sys.argv[1] == "--refresh":
        return refresh_leg(*((int(sys.argv[2]), int(sys.argv[3]), True) if len(sys.argv) > 3 else (256, 256, False)))
    if len(sys.argv) > 1 and sys.argv[1] == "--lists":
        return lists_leg(*((int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (256, 256)))
    if len(sys.argv) > 1 and sys.argv[1] == "--apply":
        return apply_leg(*((int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (256, 256)))
    if len(sys.argv) > 1 and sys.argv[1] == "--attend":
        return attend_leg(*((int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (256, 256)))
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 256)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    for mode, k, variant in (("topk", 8, "default"), ("adaptive", 0, "default"), ("adaptive", 0, "sparse")):
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            fwd = _timed(lambda: ce(x), 10)
            deg = _timed(lambda: ce.degrees(x), 3)
            holder = {}
            def export():
                holder["g"] = None                      # (release the previous arrays first)
                holder["g"] = ce.graph(x)
            tot = _timed(export, 3)
        g = holder["g"]
        print(f"[1,64,{H},{W}] {mode} k={k} ({variant}): {g.n_edges} edges (mean degree {g.n_edges / g.L:.1f}); "
              f"graph {tot:.2f} ms, degrees alone {deg:.2f} ms, forward {fwd:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
