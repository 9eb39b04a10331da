"""``ops.graph_stage_features16`` (dagl_graph_stage_features16, csrc/stage_features.hip) and ``features="stage16"`` of the stage-fused
``CES`` calls (dagl_amd/net.py).

Values: the reference is fp64 on the CPU from the module parameters (conv2d for g / theta / thr / bias, unfold + Linear + ReLU, the
mean over keys, tau), the error measure the project's ``max|d| / max|ref|`` per array, and the yardstick the per-head route
``CE._graph_features(x, margin, True, False)`` on the same input in the same test: the new route's error may be at most 2 x the per-head
route's.  Why 2: both routes run the same kernels on the same split operands; the multi-head projection only changes which images run
the single-tile route, whose three split products meet in another order (the docstring of test_gpu_project16.py);
``tau`` exchanges a torch fp32 mean for the fp64 column sums, which can only help.

Shapes: the smallest of each launch-plan class of tests/test_project16_plan_host.py that still carry four heads; (1,16,16) takes the
thr / bias ride-along, W % 4 != 0 the separate launch.  Every case runs four distinct heads, margin off and on."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import ATOPK16, TOPK8, _inputs
from tests.helpers import normwise
from tests.test_gpu_ces_step_graphs import _assert_state, _build, _cid, _module_state, _nw
from tests.test_gpu_graph_stage_step_fixed import (ARRAYS, CSR_ARRAYS, MODULE_SHAPE, _capture_and_replay, _fixed_start, _same_as_csr,
                                                   _same_fixed)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 5, 9), (1, 7, 31), (1, 8, 33), (2, 9, 38), (1, 16, 16), (1, 45, 38)]
HEAD_SEEDS = (21, 22, 23, 24)
NAMES = ("wq_rows", "x_rows", "b2p", "tau")


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _geom(shape):
    B, H, W = shape
    return B, H, W, -(-H // 4) * -(-W // 4), H * W


@functools.lru_cache(maxsize=None)
def _heads(shape):
    """Four distinct heads (seeded parameters, on the GPU, eval) and the input they share.  Left unchanged by the tests."""
    from dagl_amd.ce import CE
    heads = []
    for seed in HEAD_SEEDS:
        ce = CE(in_channels=64)
        ce.load_state_dict(_inputs(seed, shape, "default", 2.0)[1], strict=True)
        heads.append(ce.to(DEV).eval())
    return heads, _inputs(11, shape, "default", 2.0)[0].to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """fp64 on the CPU, per head -> dict(wq_rows [B,L,196], x_rows [B,N,196], b2p [B,H+6,W+6,16], tau [B,L]).  Computed once."""
    from oracle.ce_oracle import patch_rows, same_pad
    heads, x = _heads(shape)
    B, H, W, L, N = _geom(shape)
    x64 = x.double().cpu()
    refs = []
    torch.set_num_threads(16)
    with torch.no_grad():
        for hd in heads:
            p = {n: t.detach().double().cpu() for n, t in hd.named_parameters()}
            b1 = F.conv2d(x64, p["g.weight"], p["g.bias"], padding=1)
            b2 = F.conv2d(x64, p["theta.weight"], p["theta.bias"])
            wq = F.relu(F.linear(patch_rows(b1, 7, 4), p["fc1.0.weight"], p["fc1.0.bias"]))
            xk = F.relu(F.linear(patch_rows(b1, 7, 1), p["fc2.0.weight"], p["fc2.0.bias"]))
            xq, _ = same_pad(x64, 7, 4)
            thr = F.conv2d(xq, p["thr_conv.weight"], p["thr_conv.bias"], stride=4).reshape(B, -1)
            bias = F.conv2d(xq, p["bias_conv.weight"], p["bias_conv.bias"], stride=4).reshape(B, -1)
            mean = torch.bmm(wq, xk.mean(dim=1).unsqueeze(2)).squeeze(2)
            refs.append(dict(wq_rows=wq, x_rows=xk, b2p=F.pad(b2.permute(0, 2, 3, 1), (0, 0, 3, 3, 3, 3)).contiguous(),
                             tau=mean * thr - bias))
    assert refs[0]["wq_rows"].shape == (B, L, 196) and refs[0]["x_rows"].shape == (B, N, 196) and refs[0]["tau"].shape == (B, L)
    return refs


def _params(heads):
    return [hd._params_f32(scaled=False) for hd in heads]


def _raw(shape, params, x, margin, buf=None):
    """The C entry on outputs poisoned with NaN and (``buf`` None) a workspace of 0xFF bytes -> dict of the four arrays (tau None
    without the margin)."""
    from dagl_amd import _lib
    lib = _lib.load()
    B, H, W, L, N = _geom(shape)
    nan = float("nan")
    res = dict(wq_rows=torch.full((4, B, L, 196), nan, device=DEV), x_rows=torch.full((4, B, N, 196), nan, device=DEV),
               b2p=torch.full((4, B, H + 6, W + 6, 16), nan, device=DEV), tau=torch.full((4, B, L), nan, device=DEV) if margin else None)
    need = lib.dagl_graph_stage_features16_workspace_bytes(4, B, H, W, int(margin))
    assert need > 0
    if buf is None:
        buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    assert buf.numel() >= need + 256
    ws = (buf.data_ptr() + 255) // 256 * 256
    arr = (_lib.CeWeights * 4)()
    for h, prm in enumerate(params):
        for field, name in zip([f for f, _ in _lib.CeWeights._fields_], _lib.CeWeights.NAMES):
            setattr(arr[h], field, prm[name].data_ptr())
    rc = lib.dagl_graph_stage_features16(torch.cuda.current_stream().cuda_stream, 4, B, H, W, x.data_ptr(), arr, int(margin),
                                         res["wq_rows"].data_ptr(), res["x_rows"].data_ptr(), res["b2p"].data_ptr(),
                                         res["tau"].data_ptr() if margin else None, ws, need)
    assert rc == 0, lib.dagl_last_error()
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _routes(shape, margin):
    """(the new route's arrays from ``_raw``, the per-head route's arrays stacked the same way).  Computed once per case."""
    heads, x = _heads(shape)
    new = _raw(shape, _params(heads), x, margin)
    with torch.no_grad():
        feats = [hd._graph_features(x, margin, True, False) for hd in heads]
    old = dict(wq_rows=torch.stack([f[0] for f in feats]), x_rows=torch.stack([f[1] for f in feats]), b2p=torch.stack([f[3] for f in feats]),
               tau=torch.stack([f[2] for f in feats]) if margin else None)
    torch.cuda.synchronize()
    return new, old


# ---- 1. values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [False, True], ids=["nomargin", "margin"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_values_against_fp64_by_the_per_head_route(shape, margin):
    new, old = _routes(shape, margin)
    refs = _reference(shape)
    B, H, W, L, N = _geom(shape)
    assert new["wq_rows"].shape == old["wq_rows"].shape and new["x_rows"].shape == old["x_rows"].shape and new["b2p"].shape == old["b2p"].shape
    failures = []
    for name in NAMES if margin else NAMES[:3]:
        ref = torch.stack([r[name] for r in refs]).numpy()
        e_new = normwise(new[name].double().cpu().numpy(), ref)
        e_old = normwise(old[name].double().cpu().numpy(), ref)
        print(f"[stage16] {_id(shape)} margin {int(margin)} {name}: stage16 {e_new:.3e}  per head {e_old:.3e}  (bound 2 x)")
        if not e_new <= 2.0 * e_old:
            failures.append((name, e_new, e_old))
    for name, n in (("wq_rows", L), ("x_rows", N)):
        same = (new[name] == old[name]).all(dim=-1)
        print(f"[stage16] {_id(shape)} margin {int(margin)} {name}: {int(same.sum())} of {4 * B * n} rows equal the per-head route bit for bit"
              + f" (per head, image: {same.view(4, B, n).sum(dim=2).tolist()})")
    assert not failures, failures


# ---- 2. fill ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [False, True], ids=["nomargin", "margin"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_element_is_written(shape, margin):
    """Outputs poisoned with NaN, a workspace of 0xFF bytes: everything is finite afterwards, the value map's border zero."""
    new, _ = _routes(shape, margin)
    for name in NAMES if margin else NAMES[:3]:
        assert bool(torch.isfinite(new[name]).all()), name
    b2p = new["b2p"]
    inner = torch.zeros(b2p.shape[2:4], dtype=torch.bool, device=DEV)
    inner[3:-3, 3:-3] = True
    assert bool((b2p[:, :, ~inner] == 0).all())
    assert bool((b2p[:, :, inner] != 0).any())
    assert new["tau"] is None or margin


# ---- 3. repeat ----------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((a[n] is None and b[n] is None) or torch.equal(a[n], b[n]) for n in NAMES)


@pytest.mark.parametrize("margin", [False, True], ids=["nomargin", "margin"])
def test_nothing_stale_is_read(margin):
    """The same bits on a second call, and after a call at another shape on the same (larger) workspace."""
    from dagl_amd import _lib
    lib = _lib.load()
    small, big = (2, 9, 38), (1, 45, 38)
    need = max(lib.dagl_graph_stage_features16_workspace_bytes(4, *s, int(margin)) for s in (small, big))
    buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    hs, xs = _heads(small)
    hb, xb = _heads(big)
    first = _raw(small, _params(hs), xs, margin, buf)
    assert _same(first, _routes(small, margin)[0])                   # (a workspace of its exact size gave the same)
    assert _same(_raw(small, _params(hs), xs, margin, buf), first)
    other = _raw(big, _params(hb), xb, margin, buf)
    assert _same(other, _routes(big, margin)[0])
    assert _same(_raw(small, _params(hs), xs, margin, buf), first)
    # the Python entry: the same arrays
    from dagl_amd import ops
    ws = ops.Workspace()
    for shape, heads, x, want in ((small, hs, xs, first), (big, hb, xb, other), (small, hs, xs, first)):
        wq4, x4, b2p4, tau4 = ops.graph_stage_features16(x, _params(heads), margin, workspace=ws)
        assert _same(dict(wq_rows=wq4, x_rows=x4, b2p=b2p4, tau=tau4), want), shape
        assert all(t[h].is_contiguous() for t in (wq4, x4, b2p4) for h in range(4))


# ---- 4. range -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [False, True], ids=["nomargin", "margin"])
def test_range(margin):
    from dagl_amd import _lib
    lib = _lib.load()
    shape = (2, 9, 38)
    heads, x = _heads(shape)
    need = lib.dagl_graph_stage_features16_workspace_bytes(4, *shape, int(margin))
    buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    sane = _raw(shape, _params(heads), x, margin, buf)
    assert _same(sane, _routes(shape, margin)[0])
    # one head's fc2 weight past the split's range (|1024 w| >= 60000, still a finite fp16 number): the whole stage is NaN
    hot = [dict(p) for p in _params(heads)]
    hot[2]["fc2.0.weight"] = hot[2]["fc2.0.weight"].clone()
    hot[2]["fc2.0.weight"][7, 300] = 60000.0 / 1024.0 + 0.01
    got = _raw(shape, hot, x, margin, buf)
    for name in NAMES if margin else NAMES[:3]:
        assert bool(torch.isnan(got[name]).all()), name
    # the next call with sane weights on the same workspace: finite, the first bits
    assert _same(_raw(shape, _params(heads), x, margin, buf), sane)
    # a large input: the tiers and the per-block input scale serve it
    gen = torch.Generator().manual_seed(5)
    big = (1e4 * torch.randn(shape[0], 64, *shape[1:], generator=gen)).to(DEV)
    got = _raw(shape, _params(heads), big, margin, buf)
    with torch.no_grad():
        per_head = [hd._graph_features(big, margin, True, False) for hd in heads]
    print(f"[stage16] x = 1e4 randn, margin {int(margin)}: stage16 finite "
          f"{[bool(torch.isfinite(got[n]).all()) for n in (NAMES if margin else NAMES[:3])]}, per head (wq_rows, x_rows) finite "
          f"{[(bool(torch.isfinite(f[0]).all()), bool(torch.isfinite(f[1]).all())) for f in per_head]}")
    for name in NAMES if margin else NAMES[:3]:
        assert bool(torch.isfinite(got[name]).all()), name
    # a non-finite input trips the word
    bad = x.clone()
    bad[0, 3, 2, 5] = float("inf")
    got = _raw(shape, _params(heads), bad, margin, buf)
    for name in NAMES if margin else NAMES[:3]:
        assert bool(torch.isnan(got[name]).all()), name
    assert _same(_raw(shape, _params(heads), x, margin, buf), sane)


# ---- 5. wiring, bit for bit ---------------------------------------------------------------------------------------------------------------
def _by_hand(ces, s, x, margin):
    from dagl_amd import ops
    heads, mix = ces._stage_modules(s)
    wq4, x4, b2p4, tau4 = ops.graph_stage_features16(x, _params(heads), margin)
    return (list(wq4), list(x4), list(b2p4), list(tau4) if margin else None, mix.weight.detach().contiguous(), mix.bias.detach().contiguous())


@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_wiring_on_a_fixed_state(case):
    from dagl_amd import ops
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    _, fixed = _fixed_start(ces, x, case)
    x2 = torch.roll(x, (1, 1), (2, 3)).contiguous()
    before = _module_state(ces)
    search = dict(propagate=False, explore=0, seed=0)
    plan = ces._plan_fixed("CES.step_graphs", x2, fixed, 1, "stage16", "stage", search)
    with torch.no_grad():
        inp = x2
        for s in (1, 2, 3):
            radius, k_eff, margin, width_out = plan[s]
            stage = fixed.stages[s - 1]
            out, g = ces._stage_fixed_fused(s, inp, stage, plan[s], "stage16", search, 1)
            wq4, x4, b2p4, tau4, mw, mb = _by_hand(ces, s, inp, margin)
            want, arrays, _ = ops.graph_stage_step_fixed(wq4, x4, b2p4, stage.key, stage.deg, inp, mw, mb, width_out=width_out, radius=radius,
                                                         tau4=tau4, k=k_eff, scale=10.0, hw=inp.shape[2:])
            assert torch.equal(out, want), s
            for n in ARRAYS:
                assert torch.equal(getattr(g, n), arrays[n]), (s, n)
            inp = ces._between_stages(s, out).contiguous()
        # the search form, three iterations, on the first stage
        search = dict(propagate=True, explore=8, seed=3)
        plan = ces._plan_fixed("CES.search_graphs", x2, fixed, 1, "stage16", "stage", search, 3)
        radius, k_eff, margin, width_out = plan[1]
        stage = fixed.stages[0]
        out, g = ces._stage_fixed_fused(1, x2, stage, plan[1], "stage16", search, 3)
        wq4, x4, b2p4, tau4, mw, mb = _by_hand(ces, 1, x2, margin)
        kw = dict(width_out=width_out, radius=radius, tau4=tau4, k=k_eff, scale=10.0, hw=x2.shape[2:], propagate=True, explore=8)
        key, deg = stage.key, stage.deg
        for i in range(2):
            arrays = ops.graph_stage_step_fixed(wq4, x4, None, key, deg, seed=3 + i, **kw)[1]
            key, deg = arrays["key"], arrays["deg"]
        want, arrays, _ = ops.graph_stage_step_fixed(wq4, x4, b2p4, key, deg, x2, mw, mb, seed=5, **kw)
        assert torch.equal(out, want)
        for n in ARRAYS:
            assert torch.equal(getattr(g, n), arrays[n]), n
    # whole calls: the fixed and the CSR form of the search agree bit for bit, as they do on the other routes
    csr = fixed.to_csr()
    out_f, a = ces.search_graphs(x2, fixed, iters=3, seed=3, features="stage16", fused="stage")
    out_c, c = ces.search_graphs(x2, csr, iters=3, seed=3, features="stage16", fused=True)
    assert torch.equal(out_f, out_c) and bool(torch.isfinite(out_f).all())
    _same_as_csr(a, c)
    _assert_state(ces, before)


@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_wiring_on_a_csr_state(case):
    from dagl_amd import ops
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    state, _ = _fixed_start(ces, x, case)
    x2 = torch.roll(x, (1, 1), (2, 3)).contiguous()
    before = _module_state(ces)
    plan = ces._plan_step(x2, state, 1, "stage16", True, True)
    with torch.no_grad():
        inp = x2
        for s in (1, 2, 3):
            use, (radius, k_eff, margin, longest) = plan[s]
            assert use
            stage = state.stages[s - 1]
            out, g = ces._stage_step_fused(s, inp, stage, radius, k_eff, margin, longest, "stage16", True)
            wq4, x4, b2p4, tau4, mw, mb = _by_hand(ces, s, inp, margin)
            want, csr, _ = ops.graph_stage_step(wq4, x4, b2p4, stage.row_off, stage.key, inp, mw, mb, radius=radius, tau4=tau4, k=k_eff,
                                                scale=10.0, max_row_edges=longest, want_graph=True)
            assert torch.equal(out, want), s
            for n in CSR_ARRAYS:
                assert torch.equal(getattr(g, n), csr[n]), (s, n)
            inp = ces._between_stages(s, out).contiguous()
        # the search form, three iterations, on the first stage
        search = dict(propagate=True, explore=8, seed=3)
        plan = ces._plan_step(x2, state, 1, "stage16", True, True, search, what="CES.search_graphs")
        use, (radius, k_eff, margin, longest) = plan[1]
        stage = state.stages[0]
        out, g = ces._search_stage(1, x2, state, plan[1], 3, "stage16", True, search)
        wq4, x4, b2p4, tau4, mw, mb = _by_hand(ces, 1, x2, margin)
        kw = dict(radius=radius, tau4=tau4, k=k_eff, scale=10.0, propagate=True, explore=8)
        cur = stage
        for i in range(2):
            csr = ops.graph_stage_search(wq4, x4, cur.row_off, cur.key, tuple(x2.shape[2:]), max_row_edges=longest if i == 0 else cur.max_degree(),
                                         seed=3 + i, **kw)
            cur = stage._like(csr["row_off"], csr["key"], csr["weight"], csr["score"])
        want, csr, _ = ops.graph_stage_search_step(wq4, x4, b2p4, cur.row_off, cur.key, x2, mw, mb, max_row_edges=cur.max_degree(),
                                                   want_graph=True, seed=5, **kw)
        assert torch.equal(out, want)
        for n in CSR_ARRAYS:
            assert torch.equal(getattr(g, n), csr[n]), n
    _assert_state(ces, before)


# ---- 6. against features="split16" --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [TOPK8, ATOPK16], ids=_cid)
def test_against_split16(case):
    """Whole calls on the first stage's input: the output within 1e-3 of the "split16" call (``_held_to_the_bounds``' output bound for
    fused against head by head).  Rows whose key sets differ are counted, not asserted: a fixed-k cut may flip on last bits."""
    _, ces, x = _build(case, shape=MODULE_SHAPE)
    csr, fixed = _fixed_start(ces, x, case)
    x2 = torch.roll(x, (1, 1), (2, 3))
    before = _module_state(ces)
    for what, state, fused in (("csr", csr, True), ("fixed", fixed, "stage")):
        out_n, st_n = ces.step_graphs(x2, state, features="stage16", fused=fused)
        out_o, st_o = ces.step_graphs(x2, state, features="split16", fused=fused)
        assert bool(torch.isfinite(out_n).all()) and out_n.shape == x2.shape and not out_n.requires_grad
        err = _nw(out_n, out_o)
        a, b = (st_n.to_fixed(case[3]), st_o.to_fixed(case[3])) if what == "csr" else (st_n, st_o)
        differ = [int((a.stages[s].key.sort(dim=1).values != b.stages[s].key.sort(dim=1).values).any(dim=1).sum()) for s in range(3)]
        print(f"[stage16] {_cid(case)} {what}: output against split16 {err:.2e} (bound 1e-3); rows whose key sets differ per stage {differ} "
              f"of {a.stages[0].key.shape[0]}")
        assert err <= 1e-3
    # the default keeps its bits, and RR hands the value through
    out_d, _ = ces.step_graphs(x2, csr)
    out_e, _ = ces.step_graphs(x2, csr, features="fp32")
    assert torch.equal(out_d, out_e)
    _assert_state(ces, before)


def test_build_graphs_and_rr():
    rr, ces, x = _build(TOPK8, shape=MODULE_SHAPE, trunk=True)
    out_n, st_n = rr.build_graphs(x, iters=2, seed=4, features="stage16")
    out_o, st_o = rr.build_graphs(x, iters=2, seed=4, features="split16")
    print(f"[stage16] RR.build_graphs against split16: {_nw(out_n, out_o):.2e} (reported: the random candidates meet fixed-k cuts)")
    assert out_n.shape == x.shape and bool(torch.isfinite(out_n).all()) and not st_n.fixed
    out_s, st = rr.step_graphs(torch.roll(x, (1, 1), (2, 3)), st_n.to_fixed(8), features="stage16", fused="stage")
    assert st.fixed and bool(torch.isfinite(out_s).all())


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------------------
def test_capture_of_the_stage_fused_step_on_stage_features():
    _, ces, x0 = _build(TOPK8, shape=MODULE_SHAPE)
    _, start = _fixed_start(ces, x0, TOPK8)
    frames = [torch.roll(x0, (s, s), (2, 3)) for s in (1, 2, 3)]
    before = _module_state(ces)
    _capture_and_replay(ces, frames, start, lambda x, st: ces.step_graphs(x, st, fused="stage", features="stage16"))
    _assert_state(ces, before)
