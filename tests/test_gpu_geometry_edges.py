"""Where the generic-geometry route (``CE`` built with ``ksize / stride_1 / stride_2 / inter_channels`` other than (7, 4, 1, 16):
csrc/generic.hip) meets the rest of the project, against the fp64 oracle:

A  a ``CES`` stage whose heads are not the default head must go head by head -- the fused launch set ``dagl_ces_stage_forward`` has
   the default head's weight shapes compiled in -- and ``ops.ces_stage_forward`` refuses mis-shaped weights before the library;
B  the fixed-k modes with 64 < min(k, N): the dense row kernel's radix selection (ties to the lower key index), on both sides of the
   (key, weight) lists' cutoff k = 64, over more than one chunk of score rows, and under autograd;
C  a non-finite input pixel: the image comes back NaN where the oracle's is, the other images of the batch as if alone.

Part A never lets mis-shaped weights reach the device: the routing tests replace ``ops.ces_stage_forward`` with a sentinel, the
validation test the library loader with a stub."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import normwise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _params(seed, ksize=7, Cin=64, c=16, variant="default", gain=2.0):
    from dagl_amd.synth import make_ce_params
    return {n: torch.from_numpy(a) for n, a in make_ce_params(seed, in_channels=Cin, inter_channels=c, ksize=ksize, variant=variant,
                                                              sparse_gain=gain).items()}


def _features(seed, B, C, H, W):
    from dagl_amd.synth import make_features
    return torch.from_numpy(make_features(seed, B, C, H, W))


def _topk_gap(S, k):
    """Smallest relative gap between a query's k-th and (k+1)-th fp64 score (inf when every key is taken)."""
    kk = min(int(k), S.shape[-1])
    if kk >= S.shape[-1]:
        return float("inf")
    top = S.topk(kk + 1, dim=-1).values
    return float(((top[..., kk - 1] - top[..., kk]) / top[..., kk - 1].abs().clamp(min=1e-30)).min())


def _bound(S, mode, k):
    """1e-4, or 1e-3 where some query's k-th and (k+1)-th oracle scores lie within 1e-6 relative (either key is a legitimate k-th
    neighbour; the rule of tests/test_gpu_fuzz.py)."""
    return 1e-4 if mode == "adaptive" or _topk_gap(S, k) >= 1e-6 else 1e-3


# ---- A: CES stages with non-default heads -----------------------------------------------------------------------------------------

def _no_fused_launch(*args, **kwargs):
    raise AssertionError("the fused CES launch set was reached with heads it does not hold")


def _load_ces(ces, seed, variant, gain):
    """Seed every head from make_ce_params at its own ksize, the rest of the module from seeded_state_dict."""
    from dagl_amd.net import seeded_state_dict
    sd = seeded_state_dict(ces.state_dict(), seed)
    for s in (1, 2, 3):
        for h in (1, 2, 3, 4):
            name = f"c{s}_{h}"
            ks = getattr(ces, name).ksize
            for n, t in _params(seed + 10 * s + h, ksize=ks, variant=variant, gain=gain).items():
                sd[f"{name}.{n}"] = t
    ces.load_state_dict(sd, strict=True)
    return ces


def _stage_oracle(ces, s, x, mode, k):
    """fp64 ``mix(cat(head_1(x) .. head_4(x))) + x`` of stage ``s`` from the module's own parameters (CPU)."""
    from oracle.ce_oracle import ce_forward_oracle
    outs, S_all = [], []
    for h in (1, 2, 3, 4):
        hd = getattr(ces, f"c{s}_{h}")
        prm = {n: p.detach().cpu() for n, p in hd.named_parameters() if not n.startswith("W.")}
        o, st = ce_forward_oracle(x.cpu(), prm, mode=mode, k=k or None, dtype=torch.float64, stages=True, ksize=hd.ksize,
                                  stride_q=hd.stride_1, stride_kv=hd.stride_2)
        outs.append(o)
        S_all.append(st["S"])
    mix = getattr(ces, f"c{s}_c")
    out = F.conv2d(torch.cat(outs, dim=1), mix.weight.detach().cpu().double(), mix.bias.detach().cpu().double()) + x.cpu().double()
    bound = max(_bound(S, mode, k) for S in S_all)
    return out, bound


def _set_mode(ces, mode, k):
    for s in (1, 2, 3):
        for h in (1, 2, 3, 4):
            hd = getattr(ces, f"c{s}_{h}")
            hd.select_mode = mode
            if k:
                hd.select_k = k


@pytest.mark.parametrize("mode,k,variant", [("adaptive", 0, "sparse"), ("topk", 8, "default")])
def test_ces_with_generic_heads_goes_head_by_head(monkeypatch, mode, k, variant):
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    monkeypatch.setattr(ops, "ces_stage_forward", _no_fused_launch)
    ces = _load_ces(CES(64, ce_cls=partial(CE, ksize=5, stride_1=3)), 301, variant, 1.5).to(DEV).eval()
    _set_mode(ces, mode, k)
    x = _features(301, 1, 64, 30, 34)
    want, bound = _stage_oracle(ces, 1, x, mode, k)
    with torch.no_grad():
        got = ces._stage(1, x.to(DEV))
    assert ces.last_info is None                                             # (set by the fused path only)
    assert got.shape == (1, 64, 30, 34)
    assert normwise(got.cpu().numpy(), want.numpy()) <= bound


def test_ces_with_one_generic_head_among_default_heads_goes_head_by_head(monkeypatch):
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    monkeypatch.setattr(ops, "ces_stage_forward", _no_fused_launch)
    ces = CES(64)
    ces.c1_3 = CE(in_channels=64, ksize=5, stride_1=3)
    ces = _load_ces(ces, 302, "sparse", 1.6).to(DEV).eval()
    x = _features(302, 1, 64, 32, 36)
    want, bound = _stage_oracle(ces, 1, x, "adaptive", 0)
    with torch.no_grad():
        got = ces._stage(1, x.to(DEV))
    assert ces.last_info is None
    assert normwise(got.cpu().numpy(), want.numpy()) <= bound


def test_ces_with_default_heads_still_fuses(monkeypatch):
    from dagl_amd import ops
    from dagl_amd.net import CES
    real, calls = ops.ces_stage_forward, []

    def spy(*args, **kwargs):
        calls.append(kwargs.get("mode"))
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "ces_stage_forward", spy)
    ces = _load_ces(CES(64), 303, "sparse", 1.6).to(DEV).eval()
    x = _features(303, 1, 64, 32, 36)
    want, bound = _stage_oracle(ces, 1, x, "adaptive", 0)
    with torch.no_grad():
        got = ces._stage(1, x.to(DEV))
    assert calls == ["adaptive"] and ces.last_info is not None, (calls, ces.last_info)
    assert normwise(got.cpu().numpy(), want.numpy()) <= bound


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"ces_stage_forward reached the library ({name}) before refusing its arguments")


@pytest.mark.parametrize("case", ["ksize5_head", "inter_channels32_head", "mix_w", "missing_key"])
def test_ces_stage_forward_refuses_mis_shaped_weights(monkeypatch, case):
    from dagl_amd import _lib, ops
    from dagl_amd._lib import DaglError
    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())
    heads = [{n: t.to(DEV) for n, t in _params(310 + h).items() if not n.startswith("W.")} for h in range(4)]
    mix_w = torch.randn(64, 64, 1, 1, device=DEV)
    mix_b = torch.randn(64, device=DEV)
    match = {"ksize5_head": "thr_conv.weight", "inter_channels32_head": "g.weight", "mix_w": "mix_w", "missing_key": "fc2.0.bias"}[case]
    if case == "ksize5_head":
        heads[2] = {n: t.to(DEV) for n, t in _params(320, ksize=5).items() if not n.startswith("W.")}
    elif case == "inter_channels32_head":
        heads[1] = {n: t.to(DEV) for n, t in _params(321, c=32).items() if not n.startswith("W.")}
    elif case == "mix_w":
        mix_w = torch.randn(64, 32, 1, 1, device=DEV)
    else:
        del heads[3]["fc2.0.bias"]
    x = torch.randn(1, 64, 16, 16, device=DEV)
    with pytest.raises(DaglError, match=match):
        ops.ces_stage_forward(x, heads, mix_w, mix_b, mode="adaptive")


# ---- B: the fixed-k modes beyond the (key, weight) lists --------------------------------------------------------------------------

# (ksize, stride_1, stride_2, inter_channels, Cin, B, H, W)
K5S3 = (5, 3, 1, 16, 64, 1, 40, 44)               # L = 14 x 15, N = 1760
K7S4KV2 = (7, 4, 2, 16, 64, 1, 48, 56)            # L = 12 x 14, N = 24 x 28 = 672


def _geom_forward(geom, seed, mode, k, variant, gain=1.6, x=None):
    from dagl_amd import ops
    from oracle.ce_oracle import ce_forward_oracle
    ks, s1, s2, c, Cin, B, H, W = geom
    params = _params(seed, ksize=ks, Cin=Cin, c=c, variant=variant, gain=gain)
    if x is None:
        x = _features(seed, B, Cin, H, W)
    want, st = ce_forward_oracle(x, params, mode=mode, k=k, dtype=torch.float64, stages=True, ksize=ks, stride_q=s1, stride_kv=s2)
    out, deg = ops.ce_forward_generic(x.to(DEV), {n: t.to(DEV) for n, t in params.items()}, ks, s1, s2, c, mode=mode, k=k,
                                      want_degree=True)
    return out.cpu(), deg.cpu(), want, st


def _n_keys(geom):
    ks, s1, s2, c, Cin, B, H, W = geom
    return (-(-H // s2)) * (-(-W // s2))


@pytest.mark.parametrize("geom", [K5S3, K7S4KV2], ids=["k5s3_40x44", "k7s4kv2_48x56"])
@pytest.mark.parametrize("mode,variant", [("topk", "default"), ("adaptive_topk", "allpass"), ("adaptive_topk", "sparse")])
@pytest.mark.parametrize("kcase", ["64", "65", "100", "N-1"])
def test_generic_fixed_k_beyond_the_lists_against_the_fp64_oracle(geom, mode, variant, kcase):
    """k = 64 takes the (key, weight) lists, k = 65 and beyond the dense A chunk behind the radix selection: both sides of the
    cutoff are held to the same bound."""
    N = _n_keys(geom)
    k = N - 1 if kcase == "N-1" else int(kcase)
    out, deg, want, st = _geom_forward(geom, 400 + geom[0], mode, k, variant)
    kk = min(k, N)
    if variant != "sparse":                                                  # every query keeps exactly min(k, N) keys
        assert int(st["deg"].min()) == kk == int(st["deg"].max())
        assert int(deg.min()) == kk == int(deg.max())
    d = (deg.long() - st["deg"].long()).abs()
    if mode == "topk":
        assert int(d.max()) == 0
    else:
        assert int(d.max()) <= 2 and float((d != 0).float().mean()) <= 0.02, (int(d.max()), float((d != 0).float().mean()))
    assert normwise(out.numpy(), want.numpy()) <= _bound(st["S"], mode, k)


def test_generic_fixed_k_ties_at_the_kth_place():
    """A constant input map: the interior keys' scores are all equal; exactly k keys are taken on either side of the lists' cutoff
    and far beyond it, not every key that reaches the k-th score.  "adaptive_topk" with heads that let every key pass: the tie rule
    is shared by both modes."""
    from dagl_amd import ops
    x = torch.full((1, 64, 24, 28), 0.25, device=DEV)                           # N = 672
    for mode, variant in (("topk", "default"), ("adaptive_topk", "allpass")):
        params = {n: t.to(DEV) for n, t in _params(405, ksize=5, variant=variant).items()}
        for k in (64, 65, 300):
            out, deg = ops.ce_forward_generic(x, params, 5, 3, 1, 16, mode=mode, k=k, want_degree=True)
            assert int(deg.min()) == k == int(deg.max()), (mode, k)
            assert bool(torch.isfinite(out).all()), (mode, k)


def test_generic_fixed_k_over_two_chunks_of_score_rows():
    """96 x 96, (3, 1, 1, 4), two images: L = N = 9216 > the 7281 score rows of one chunk (the second chunk ragged), through the
    lists (k = 64) and the dense A chunk (k = 65)."""
    geom = (3, 1, 1, 4, 4, 2, 96, 96)
    for k in (64, 65):
        out, deg, want, st = _geom_forward(geom, 406, "topk", k, "default")
        assert int(deg.min()) == k == int(deg.max()) and int(st["deg"].min()) == k
        bound = _bound(st["S"], "topk", k)
        for b in range(2):
            assert normwise(out[b].numpy(), want[b].numpy()) <= bound, (k, b)


@pytest.mark.parametrize("mode", ["topk", "adaptive_topk"])
def test_generic_fixed_k_beyond_the_lists_gradients(mode):
    """k = 100 on a k5s3 module under autograd (dagl_ce_generic_core_forward / _backward: the backward redoes the selection) against
    the fp64 oracle's autograd."""
    from tests.test_geometry_oracle import GEOM_GRAD_CASES, geom_grad_inputs, geom_oracle_grads
    from tests.test_oracle_grad import load_grad_case
    from dagl_amd.ce import CE
    meta, _ = load_grad_case([p for p in GEOM_GRAD_CASES if "k5s3_topk6" in p][0])
    meta = dict(meta, mode=mode, k=100)
    x, params, G = geom_grad_inputs(meta)
    want, g64 = geom_oracle_grads(meta, torch.float64)
    ce = CE(ksize=5, stride_1=3, stride_2=1, in_channels=meta["C"], inter_channels=meta["inter_channels"])
    ce.load_state_dict(params, strict=True)
    ce.select_mode, ce.select_k = mode, 100
    ce = ce.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    out = ce(xg)
    (out * G.to(DEV)).sum().backward()
    got = {"d_x": xg.grad, **{"d_" + n: p.grad for n, p in ce.named_parameters() if p.grad is not None}}
    assert normwise(out.detach().cpu().numpy(), want.numpy()) <= 1e-4
    assert set(got) == set(g64)
    for name, w in g64.items():
        assert normwise(got[name].cpu().numpy(), w.numpy()) <= 5e-4, name


# ---- C: non-finite input ---------------------------------------------------------------------------------------------------------

K5S3_SMALL = (5, 3, 1, 16, 64, 2, 24, 27)
K7S4KV2_SMALL = (7, 4, 2, 16, 64, 2, 32, 36)


@pytest.mark.parametrize("geom", [K5S3_SMALL, K7S4KV2_SMALL], ids=["k5s3", "k7s4kv2"])
@pytest.mark.parametrize("mode,k", [("adaptive", 0), ("topk", 6), ("adaptive_topk", 9)])
@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("where", ["interior", "corner"])
@pytest.mark.parametrize("route", ["inference", "train"])
def test_generic_nonfinite_pixel_gives_nan_where_the_oracle_does(geom, mode, k, value, where, route):
    from dagl_amd.ce import CE
    from oracle.ce_oracle import ce_forward_oracle
    ks, s1, s2, c, Cin, B, H, W = geom
    params = _params(500 + ks, ksize=ks, Cin=Cin, c=c, variant="sparse" if mode == "adaptive" else "default", gain=1.5)
    x = _features(500 + ks, B, Cin, H, W)
    y, xx = (H // 2, W // 3) if where == "interior" else (H - 1, W - 1)
    x[1, 5, y, xx] = float(value)
    want, st = ce_forward_oracle(x, params, mode=mode, k=k or None, dtype=torch.float64, stages=True, ksize=ks, stride_q=s1,
                                 stride_kv=s2)
    assert bool(torch.isnan(want[1]).any()) and not bool(torch.isnan(want[0]).any())
    ce = CE(ksize=ks, stride_1=s1, stride_2=s2, in_channels=Cin, inter_channels=c)
    ce.load_state_dict(params, strict=True)
    ce.select_mode = mode
    if k:
        ce.select_k = k
    ce = ce.to(DEV)

    def run(inp):
        if route == "train":
            ce.train()
            return ce(inp.to(DEV).requires_grad_(True)).detach().cpu()
        ce.eval()
        with torch.no_grad():
            return ce(inp.to(DEV)).cpu()
    out = run(x)
    alone = run(x[:1].clone())
    assert torch.equal(torch.isnan(out[1]), torch.isnan(want[1])), \
        (int(torch.isnan(out[1]).sum()), int(torch.isnan(want[1]).sum()), want[1].numel())
    assert torch.equal(out[0], alone[0])
    assert normwise(out[0].numpy(), want[0].numpy()) <= _bound(st["S"][:1], mode, k)
