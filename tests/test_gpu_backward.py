"""Backward of the graph core: gradients through the C ABI against (a) the reference's own autograd
gradients (tests/golden/grad_*.npz) and (b) the fp64 oracle's autograd, plus the training-path forward and the
error contract for dense neighbourhoods.  Tolerances are normwise (max|a-b| / max|b|), per tensor."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import normwise
from tests.list_core_reference import GRAD_NAMES, check_against_fp64, list_core_grads
from tests.test_oracle_grad import GRAD_CASES, compare_grads, grad_case_inputs, load_grad_case, oracle_grads

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4          # forward, as in test_gpu_block.py
TOL_GRAD = 1e-3         # vs the reference's fp32 gradients (whose own distance to fp64 reaches 3e-4)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _module(params, mode, k, scan="screened", train=True):
    from dagl_amd.ce import CE
    ce = CE(in_channels=params["g.weight"].shape[1])       # (goldens at 32 / 96 / 128 input channels: CE(in_channels=n_feats))
    ce.load_state_dict(params, strict=True)
    ce.select_mode, ce.select_k, ce.scan = mode, (k or 8), scan
    ce = ce.to(_dev())
    return ce.train() if train else ce.eval()


def _hip_grads(meta, scan="screened"):
    x, params, G = grad_case_inputs(meta)
    ce = _module(params, meta["mode"], meta["k"], scan)
    xg = x.to(_dev()).requires_grad_(True)
    out = ce(xg)
    (out * G.to(_dev())).sum().backward()
    grads = {"d_x": xg.grad}
    grads.update({"d_" + n: p.grad for n, p in ce.named_parameters() if p.grad is not None})
    return ce, out.detach(), grads


@pytest.mark.parametrize("scan", ["screened", "exact"])
@pytest.mark.parametrize("path", GRAD_CASES, ids=[os.path.basename(p)[5:-4] for p in GRAD_CASES])
def test_gradients_match_reference_autograd(path, scan):
    meta, want = load_grad_case(path)
    ce, out, grads = _hip_grads(meta, scan)
    assert normwise(out.cpu().numpy(), want["out"]) <= TOL_OUT
    assert "d_W.weight" not in grads                      # registered but never applied (dagl.py:192)
    dense = meta["mode"] != "topk" and "sparse" not in meta["name"]
    if dense:
        # the two scalar head biases are sums over all queries with heavy cancellation: the REFERENCE's own fp32 values
        # sit 3e-3 .. 5e-3 from an fp64 evaluation in this regime (measured: make_golden_grad's gray_default_64x64), so
        # they are held to 1e-2 here and to the fp64 oracle in test_gradients_are_as_close_to_fp64_as_the_reference
        scal = {k: v for k, v in want.items() if k in ("d_thr_conv.bias", "d_bias_conv.bias")}
        compare_grads(grads, scal, meta["fc_step"], 1e-2)
        want = {k: v for k, v in want.items() if k not in scal}
    compare_grads(grads, want, meta["fc_step"], TOL_GRAD)
    if meta["mode"] == "topk":
        assert "d_thr_conv.weight" not in grads           # the fixed-k variant has no threshold heads
    elif "sparse" in meta["name"]:
        assert ce.last_info["max_degree"] <= 64 and ce.last_info["path"] != 5
    else:                                                 # "default" / "longtail": dense formulation (forward: the streamed
        assert ce.last_info["max_degree"] > 64 and ce.last_info["path"] in (4, 5)   # kernel, path 4; small maps: GEMM form, 5)


@pytest.mark.parametrize("path", GRAD_CASES, ids=[os.path.basename(p)[5:-4] for p in GRAD_CASES])
def test_gradients_are_as_close_to_fp64_as_the_reference(path):
    meta, ref32 = load_grad_case(path)
    _, g64 = oracle_grads(meta, torch.float64)
    _, _, grads = _hip_grads(meta)
    for name, w in g64.items():
        w = w.numpy()
        g = grads[name].cpu().numpy()
        e_hip = normwise(g, w)
        if name in ("d_fc1.0.weight", "d_fc2.0.weight"):
            w = w.reshape(-1)[::meta["fc_step"]]
        e_ref = normwise(ref32[name], w)
        # the two scalar head biases of a dense mask are sums over all queries that cancel to ~1e-3 of their terms: the reference's
        # own fp32 value lands anywhere between 4e-7 (gray_default_c96_32x36) and 5e-3 (gray_default_64x64) from fp64 on them
        dense_scalar = name in ("d_thr_conv.bias", "d_bias_conv.bias") and meta["mode"] != "topk" and "sparse" not in meta["name"]
        assert e_hip <= 3 * e_ref + (1e-3 if dense_scalar else 1e-4), (name, e_hip, e_ref)


def test_training_forward_equals_inference_forward():
    meta, _ = load_grad_case([p for p in GRAD_CASES if "gray_sparse_b2_40x36" in p][0])
    x, params, _ = grad_case_inputs(meta)
    for mode, k in (("adaptive", 0), ("topk", 8), ("adaptive_topk", 6)):
        ce = _module(params, mode, k)
        xd = x.to(_dev())
        with torch.no_grad():
            ref = ce(xd)
        out = ce(xd.clone().requires_grad_(True))
        assert out.requires_grad
        # (two evaluations of the same maths: fused split-fp16 kernels vs unfold + fp32 GEMM chains)
        assert normwise(out.detach().cpu().numpy(), ref.cpu().numpy()) <= 5e-5
        with torch.no_grad():                               # and the inference path still works afterwards
            again = ce(xd)
        assert torch.equal(again, ref)


def test_adaptive_topk_gradients_match_oracle_autograd():
    meta, _ = load_grad_case([p for p in GRAD_CASES if "gray_sparse_b2_40x36" in p][0])
    meta = dict(meta, mode="adaptive_topk", k=6)
    _, g64 = oracle_grads(meta, torch.float64)
    _, _, grads = _hip_grads(meta)
    for name, w in g64.items():
        assert normwise(grads[name].cpu().numpy(), w.numpy()) <= 5e-4, name


def test_finite_difference_of_the_core_op():
    """Directional derivative of the HIP core op by central differences, independent of any autograd: checks
    d_wq_rows, d_x_rows, d_b2, d_thr, d_bias of dagl_ce_core_backward together.  The loss is only piecewise smooth
    (neighbour sets are discrete), so the inputs are built with a margin -- seed 8 has a 1.6e-4 gap between every
    query's 5th and 6th score, and the adaptive thresholds are put in the middle of each query's widest score gap
    -- and the test insists that both probe points select the same neighbours."""
    from dagl_amd import ops
    g = torch.Generator().manual_seed(8)
    B, H, W = 1, 24, 28
    L, N = 6 * 7, H * W
    dev = _dev()
    wq_c = torch.rand(B, L, 196, generator=g) * 0.1
    xr_c = torch.rand(B, N, 196, generator=g) * 0.1
    S = wq_c[0].double() @ xr_c[0].double().t()
    v = S.sort(dim=1, descending=True).values
    d = (v[:, 2:30] - v[:, 3:31]).argmax(dim=1) + 3                         # degree with the widest gap, 3..30
    T = 0.5 * (v[torch.arange(L), d - 1] + v[torch.arange(L), d])
    thr_c = torch.ones(B, L)
    bias_c = (S.mean(dim=1) - T).float()[None]                               # T = mu * thr - bias
    wq, xr, thr, bias = (t.to(dev).contiguous() for t in (wq_c, xr_c, thr_c, bias_c))
    b2 = torch.randn(B, 16, H, W, generator=g).to(dev)
    G = torch.randn(B, 16, H, W, generator=g).to(dev)
    base = (wq, xr, b2, thr, bias)
    dirs = [0.1 * torch.randn(t.shape, generator=g).to(dev) for t in (wq, xr)] + \
           [torch.randn(b2.shape, generator=g).to(dev)] + \
           [(2 * torch.rand(t.shape, generator=g) - 1).to(dev) for t in (thr, bias)]
    eps = 1e-4
    for mode, k in (("topk", 5), ("adaptive", 0)):
        out, saved = ops.ce_core_forward(*base, mode=mode, k=k)
        if mode == "adaptive":
            assert torch.equal(saved["nb_cnt"][0].cpu().long(), d)
        grads = ops.ce_core_backward(G, *base, saved, mode=mode, k=k)
        n_in = 3 if mode == "topk" else 5
        analytic = sum(float((gi.double() * di.double()).sum()) for gi, di in zip(grads[:n_in], dirs[:n_in]))

        def probe(sign):
            a = [(t + sign * eps * di).contiguous() if i < n_in else t for i, (t, di) in enumerate(zip(base, dirs))]
            o, s2 = ops.ce_core_forward(*a, mode=mode, k=k)
            return float((o.double() * G.double()).sum()), s2
        (fp, sp), (fm, sm) = probe(+1), probe(-1)
        for s2 in (sp, sm):
            assert torch.equal(s2["nb_cnt"], saved["nb_cnt"])
            assert torch.equal(s2["nb_idx"].sort(dim=2).values, saved["nb_idx"].sort(dim=2).values)
        numeric = (fp - fm) / (2 * eps)
        assert abs(numeric - analytic) <= 2e-2 * abs(analytic) + 1e-2, (mode, numeric, analytic)


def test_gradients_are_bit_reproducible():
    """No atomics in the core backward: the scatter-adds are segmented sums over the key-sorted edge list.  (The trunk's
    MIOpen weight-gradient kernels are not bit-reproducible, so the check is on the core op itself.)"""
    from dagl_amd import ops
    g = torch.Generator().manual_seed(21)
    B, H, W = 2, 40, 36
    L, N = 10 * 9, H * W
    dev = _dev()
    wq = (torch.rand(B, L, 196, generator=g) * 0.1).to(dev)
    xr = (torch.rand(B, N, 196, generator=g) * 0.1).to(dev)
    # a hub key: the best neighbour of every query (score 1.0 against 0.5), run spans many chunks.  (0.1, not more: at 0.2 the hub's
    # weight is within 1e-5 of 1 and d l = A (d A - sum A d A) cancels to what fp32 cannot carry -- the fp32 reference itself then sits
    # 7e-3 (top-k) and 0.6 (adaptive) from fp64 and the value check below could not bind.)
    xr[:, 7] = 0.1
    b2 = torch.randn(B, 16, H, W, generator=g).to(dev)
    thr = torch.full((B, L), 1.17, device=dev)
    bias = torch.full((B, L), 0.0, device=dev)
    G = torch.randn(B, 16, H, W, generator=g).to(dev)
    for mode, k in (("topk", 8), ("adaptive", 0)):
        out, saved = ops.ce_core_forward(wq, xr, b2, thr, bias, mode=mode, k=k)
        assert int((saved["nb_idx"][:, :, :max(k, 1)] == 7).sum()) >= B * L or mode == "adaptive"
        runs = [ops.ce_core_backward(G, wq, xr, b2, thr, bias, saved, mode=mode, k=k) for _ in range(3)]
        for i, t0 in enumerate(runs[0]):
            if t0 is not None:
                assert torch.equal(t0, runs[1][i]) and torch.equal(t0, runs[2][i]), (mode, i)
        assert torch.isfinite(runs[0][1]).all() and float(runs[0][1][:, 7].abs().max()) > 0
        # and against a plain autograd evaluation of the same lists (hub included): the forward's own nb_idx / nb_cnt through the
        # fp64 list-form reference, under the tolerance rule of test_gpu_list_backward.py (e_ref: the same reference in fp32)
        idx, cnt = saved["nb_idx"].cpu().long(), saved["nb_cnt"].cpu().long()
        inputs = [t.cpu() for t in (wq, xr, b2, thr, bias)]
        ref64 = list_core_grads(inputs, idx, cnt, G.cpu(), mode, torch.float64)
        ref32 = list_core_grads(inputs, idx, cnt, G.cpu(), mode, torch.float32)
        n_in = 3 if mode == "topk" else 5
        check_against_fp64(f"bit-reproducible [{B},{H},{W}] {mode}", GRAD_NAMES[:n_in], runs[0][:n_in], ref64, ref32)


def test_hub_keys_shared_by_every_query():
    """A constant image makes every score tie; ties go to the smallest key index, so the same k keys are the
    neighbours of ALL queries (in-degree L): the key-sorted gather must cope, and the gradients stay finite."""
    from dagl_amd.synth import make_ce_params
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(61, variant="default").items()}
    ce = _module(params, "topk", 4)
    x = torch.full((1, 64, 48, 48), 0.3, device=_dev(), requires_grad=True)
    out = ce(x)
    out.square().sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    for p in ce.parameters():
        assert p.grad is None or torch.isfinite(p.grad).all()


def test_dense_neighbourhoods_train_through_the_dense_formulation():
    """Default-initialised heads keep ~95 % of the keys: the list form refuses (DAGL_ERR_UNSUPPORTED) and the module goes
    to the dense formulation (dense_train.hip); forward equals the inference path, and the module remembers the regime."""
    from dagl_amd import ops
    from dagl_amd._lib import ERR_UNSUPPORTED, DaglError
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(16, variant="default").items()}
    ce = _module(params, "adaptive", 0)
    x = torch.from_numpy(make_features(16, 1, 64, 64, 64)).to(_dev())
    with torch.no_grad():
        ref = ce(x)
        b1, b2, thr, bias = ce._prologue(x)
        wq = torch.rand(1, 256, 196, device=_dev()); xr = torch.rand(1, 4096, 196, device=_dev())
        with pytest.raises(DaglError) as ei:                       # the C ABI contract of the list entry point
            ops.ce_core_forward(wq, xr, b2.contiguous(), torch.zeros(1, 256, device=_dev()),
                                torch.zeros(1, 256, device=_dev()), mode="adaptive")
        assert ei.value.code == ERR_UNSUPPORTED
    out = ce(x.clone().requires_grad_(True))
    assert out.requires_grad and ce._train_dense and ce.last_info["path"] == 5
    assert ce.last_info["max_degree"] > 64
    assert normwise(out.detach().cpu().numpy(), ref.cpu().numpy()) <= 1e-4
    out2 = ce(x.clone().requires_grad_(True))                       # second call: straight to the dense formulation
    assert torch.equal(out2.detach(), out.detach())
    out2.sum().backward()
    assert all(torch.isfinite(p.grad).all() for n, p in ce.named_parameters() if not n.startswith("W."))


def test_dense_backward_is_bit_reproducible_and_chunking_invariant():
    from dagl_amd import ops
    g = torch.Generator().manual_seed(4)
    B, H, W = 2, 24, 28
    L, N = 6 * 7, H * W
    dev = _dev()
    wq = (torch.rand(B, L, 196, generator=g) * 0.1).to(dev); xr = (torch.rand(B, N, 196, generator=g) * 0.1).to(dev)
    b2 = torch.randn(B, 16, H, W, generator=g).to(dev); G = torch.randn(B, 16, H, W, generator=g).to(dev)
    thr = torch.full((B, L), 0.9, device=dev); bias = torch.zeros(B, L, device=dev)
    out, saved = ops.ce_core_dense_forward(wq, xr, b2, thr, bias)
    g1 = ops.ce_core_dense_backward(G, wq, xr, b2, thr, bias, saved)
    g2 = ops.ce_core_dense_backward(G, wq, xr, b2, thr, bias, saved)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    # one image at a time = other batch grouping: same numbers
    o1, s1 = ops.ce_core_dense_forward(wq[1:], xr[1:], b2[1:], thr[1:], bias[1:])
    assert torch.equal(o1, out[1:])
    h1 = ops.ce_core_dense_backward(G[1:], wq[1:], xr[1:], b2[1:], thr[1:], bias[1:], s1)
    assert all(torch.equal(a, b[1:]) for a, b in zip(h1, g1))


def test_dense_core_matches_the_oracle_and_its_autograd():
    """dagl_ce_core_dense_forward / _backward against the fp64 oracle on the same feature rows (odd sizes, N not a multiple
    of 4, thresholds that keep about half of the keys)."""
    from dagl_amd import ops
    from oracle.ce_oracle import ce_core_oracle
    g = torch.Generator().manual_seed(12)
    B, H, W = 2, 45, 38
    L, N = 12 * 10, H * W
    wq = torch.rand(B, L, 196, generator=g) * 0.1; xr = torch.rand(B, N, 196, generator=g) * 0.1
    b2 = torch.randn(B, 16, H, W, generator=g); G = torch.randn(B, 16, H, W, generator=g)
    # every query's threshold sits in the middle of its widest score gap around the median (the mask is discontinuous: a
    # key within rounding of the threshold would flip between fp32 and fp64 scores and move the output by 1/deg)
    S = torch.einsum("bld,bnd->bln", wq.double(), xr.double())
    v = S.sort(dim=2).values
    lo = int(0.3 * N)
    gap = v[:, :, lo + 1:int(0.7 * N)] - v[:, :, lo:int(0.7 * N) - 1]
    at = gap.argmax(dim=2, keepdim=True) + lo
    T = 0.5 * (v.gather(2, at) + v.gather(2, at + 1)).squeeze(2)
    thr = 1.0 + 0.02 * torch.randn(B, L, generator=g)
    bias = (S.mean(dim=2) * thr.double() - T).float()                  # T = mu * thr - bias
    leaves = [t.double().requires_grad_(True) for t in (wq, xr, b2, thr, bias)]
    ref, st = ce_core_oracle(*leaves, mode="adaptive", stages=True)
    (ref * G.double()).sum().backward()
    assert 0.2 * N < float(st["deg"].mean()) < 0.8 * N
    dev = _dev()
    d = [t.to(dev) for t in (wq, xr, b2, thr, bias)]
    out, saved = ops.ce_core_dense_forward(*d)
    assert saved["info"]["total_edges"] == int(st["deg"].sum()) and saved["info"]["max_degree"] == int(st["deg"].max())
    assert normwise(out.cpu().numpy(), ref.detach().numpy()) <= TOL_OUT
    grads = ops.ce_core_dense_backward(G.to(dev), *d, saved)                  # matrix products on the fp16 matrix cores, split operands
    grads32 = ops.ce_core_dense_backward(G.to(dev), *d, saved, exact=True)    # ... on the fp32 matrix cores
    for name, got, got32, leaf in zip(("d_wq", "d_x", "d_b2", "d_thr", "d_bias"), grads, grads32, leaves):
        e16, e32 = normwise(got.cpu().numpy(), leaf.grad.numpy()), normwise(got32.cpu().numpy(), leaf.grad.numpy())
        print(f"dense backward {name}: split-fp16 products {e16:.2e}, fp32 products {e32:.2e} from the fp64 oracle's autograd")
        assert e16 <= 3e-4 and e32 <= 3e-4, name
        assert e16 <= 3.0 * e32 + 2e-6, name              # the split products are no further from fp64 than the fp32 ones


def test_one_sgd_step_reduces_the_loss():
    """DN_Gray/trainer.py:44-50 in miniature: L1 loss, backward, optimizer step on a CE head (top-k, sparse regime)."""
    meta, _ = load_grad_case([p for p in GRAD_CASES if "topk8_b2_45x38" in p][0])
    x, params, G = grad_case_inputs(meta)
    ce = _module(params, "topk", 8)
    opt = torch.optim.SGD(ce.parameters(), lr=1e-5)
    xd, target = x.to(_dev()), (0.1 * G).to(_dev())
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(ce(xd), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[2] < losses[0]


@pytest.mark.parametrize("B,H,W", [(1, 40, 36), (2, 63, 50), (8, 128, 128)])
def test_fast_projection_forward_equals_the_gemm_forward(B, H, W):
    """The training forward of fc1 / fc2 runs on the inference kernels (split-fp16 matrix cores, no unfolded rows); the
    fp32 unfold + GEMM path it replaces is kept (other layers, and the backward): both must give the same features."""
    from dagl_amd import train_ops as T
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + H + W)
    b1_rows = torch.randn(B, H * W, 16, generator=g).to(dev)
    w = (torch.randn(196, 784, generator=g) * 0.05).to(dev)
    bias = (torch.randn(196, generator=g) * 0.1).to(dev)
    b1p = T.to_padded_nhwc(b1_rows, H, W, from_rows=True)
    from dagl_amd.synth import same_pad_amounts
    t, l = same_pad_amounts(H, 7, 4)[0], same_pad_amounts(W, 7, 4)[0]
    Lh, Lw = -(-H // 4), -(-W // 4)
    outs = {}
    for fast in (True, False):
        T.FAST_FC_FORWARD = fast
        try:
            q = T.patch_linear(b1p, T.fc_weight_rows(w, 16, 7), bias, 7, 4, T.PAD - t, T.PAD - l, Lh, Lw, relu=True)
            k = T.patch_linear(b1p, T.fc_weight_rows(w, 16, 7), bias, 7, 1, 0, 0, H, W, relu=True)
        finally:
            T.FAST_FC_FORWARD = True
        outs[fast] = (q.clone(), k.clone())
    for a, b in zip(outs[True], outs[False]):
        assert a.shape == b.shape
        assert normwise(a.cpu().numpy(), b.cpu().numpy()) <= 2e-6
