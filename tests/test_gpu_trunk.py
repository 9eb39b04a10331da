"""The trunk's convolutions on the library (dagl_amd.trunk, csrc/trunk.hip) against torch on the CPU in float64, with torch's own
CPU fp32 result as the yardstick: e_lib <= 3 e_cpu32 + 1e-6 (normwise, both against the fp64 result)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.helpers import GOLDEN_DIR, normwise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bound(got, ref64, ref32, what):
    e = normwise(got, ref64)
    e32 = normwise(ref32, ref64)
    assert e <= 3.0 * e32 + 1e-6, (what, e, e32)


def _layer_case(cin, cout, k, bias, shape, seed):
    from dagl_amd import trunk
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (cin * k * k) ** 0.5)
        if bias:
            conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    x = torch.randn((shape[0], cin) + shape[1:], generator=g)
    up = torch.randn((shape[0], cout) + shape[1:], generator=g)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        c = nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias).to(dt)
        c.load_state_dict(conv.state_dict())
        xi = x.to(dt).clone().requires_grad_(True)
        y = c(xi)
        (y * up.to(dt)).sum().backward()
        res[tag] = [y.detach(), xi.grad, c.weight.grad] + ([c.bias.grad] if bias else [])
    lib = trunk.convert(nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias))
    lib.load_state_dict(conv.state_dict())
    lib = lib.to(DEV)
    xi = x.to(DEV).clone().requires_grad_(True)
    y = lib(xi)
    (y * up.to(DEV)).sum().backward()
    got = [y.detach(), xi.grad, lib.weight.grad] + ([lib.bias.grad] if bias else [])
    for name, a, r64, r32 in zip(("out", "d_x", "d_w", "d_b"), got, res["64"], res["32"]):
        _bound(a.cpu().double().numpy(), r64.numpy(), r32.double().numpy(), (cin, cout, k, bias, shape, name))


@pytest.mark.parametrize("cin,cout,k", [(64, 64, 3), (1, 64, 3), (3, 64, 3), (64, 1, 3), (64, 3, 3), (64, 64, 1)])
@pytest.mark.parametrize("bias", [True, False])
def test_single_layer_vs_fp64(cin, cout, k, bias):
    for i, shape in enumerate(((2, 37, 53), (1, 1, 1), (3, 2, 5), (4, 72, 72))):
        _layer_case(cin, cout, k, bias, shape, 100 * cin + 10 * cout + k + i)


@pytest.mark.parametrize("res_scale", [1.0, 0.1])
def test_fused_resblock_vs_fp64(res_scale):
    from dagl_amd import trunk
    from dagl_amd.net import ResBlock
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    rb = ResBlock(64, res_scale)
    with torch.no_grad():
        rb.body[1].weight.fill_(0.2)
    x = torch.randn(2, 64, 33, 40, generator=g)
    up = torch.randn(2, 64, 33, 40, generator=g)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        m = ResBlock(64, res_scale).to(dt)
        m.load_state_dict(rb.state_dict())
        xi = x.to(dt).clone().requires_grad_(True)
        y = m(xi)
        (y * up.to(dt)).sum().backward()
        res[tag] = [y.detach(), xi.grad] + [p.grad for p in m.parameters()]
    lib = ResBlock(64, res_scale)
    lib.load_state_dict(rb.state_dict())
    lib = trunk.convert(lib).to(DEV)
    xi = x.to(DEV).clone().requires_grad_(True)
    y = lib(xi)
    assert type(y.grad_fn).__name__.startswith("_ResBlockFn")         # the fused path ran
    (y * up.to(DEV)).sum().backward()
    got = [y.detach(), xi.grad] + [p.grad for p in lib.parameters()]
    names = ["out", "d_x"] + [n for n, _ in lib.named_parameters()]
    for name, a, r64, r32 in zip(names, got, res["64"], res["32"]):
        _bound(a.cpu().double().numpy(), r64.numpy(), r32.double().numpy(), (res_scale, name))


def test_whole_network_gradients_match_oracle_autograd():
    """Converted RR(n_colors=3), adaptive mode (dense neighbourhoods), with the loss and yardstick of
    test_gpu_configs.test_config5_whole_network_gradients_match_oracle_autograd."""
    from dagl_amd import trunk
    from dagl_amd.ce import CE
    from dagl_amd.net import RR, seeded_state_dict
    from dagl_amd.train import freeze_unused, task_loss
    from tests.test_gpu_configs import _oracle_ce_cls
    B, C, H, W = 2, 3, 48, 48
    ref = RR(n_colors=C, ce_cls=_oracle_ce_cls())
    sd = seeded_state_dict(ref.state_dict(), 19)
    ref.load_state_dict(sd, strict=True)
    ref32 = RR(n_colors=C, ce_cls=_oracle_ce_cls())
    ref32.load_state_dict(sd, strict=True)
    net = trunk.convert(RR(n_colors=C))
    net.load_state_dict(sd, strict=True)
    for m in list(ref.modules()) + list(ref32.modules()) + list(net.modules()):
        if isinstance(m, CE):
            m.select_mode = "adaptive"
    freeze_unused(ref); freeze_unused(ref32); freeze_unused(net)
    g = torch.Generator().manual_seed(23)
    hr = torch.rand(B, C, H, W, generator=g)
    lr = hr + (50.0 / 255.0) * torch.randn(B, C, H, W, generator=g)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref32 = ref32.train()
    task_loss(ref32(lr), hr, "dn_real").backward()
    g32 = {n: p.grad for n, p in ref32.named_parameters()}
    ref = ref.double().train()
    loss_ref = task_loss(ref(lr.double()), hr.double(), "dn_real")
    loss_ref.backward()
    net = net.to(DEV).train()
    loss = task_loss(net(lr.to(DEV)), hr.to(DEV), "dn_real")
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-4 * abs(float(loss_ref.detach()))
    gref = dict(ref.named_parameters())
    e32 = {n: normwise(g32[n].numpy(), gref[n].grad.numpy()) for n, p in net.named_parameters()
           if p.requires_grad and gref[n].grad is not None and g32[n] is not None}
    floor32 = float(np.median(list(e32.values())))
    for n, p in net.named_parameters():
        if n not in e32:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        e = normwise(p.grad.cpu().numpy(), gref[n].grad.numpy())
        assert e <= 3.0 * (e32[n] + floor32), (n, e, e32[n], floor32)


def _set12(model, name, subs_file, ref_file, batched=False):
    from dagl_amd.net import chop_forward, chop_forward_batched, psnr, set12_protocol_noise
    ref = json.load(open(os.path.join(GOLDEN_DIR, ref_file)))
    imgs = np.load(os.path.join(GOLDEN_DIR, "set12.npz"))
    subs = np.load(os.path.join(GOLDEN_DIR, subs_file))
    clean = torch.from_numpy(imgs[f"img_{name}"].astype(np.float32) / 255.0)[None, None]
    noisy = set12_protocol_noise(clean, 50.0, 1.0)
    drive = chop_forward_batched if batched else chop_forward
    with torch.no_grad():
        out = torch.clamp(drive(model, noisy.to(DEV)), 0.0, 1.0).cpu()
    r = ref["images"][name]
    assert abs(psnr(out, clean) - r["psnr_out"]) <= 0.02, (name, psnr(out, clean), r["psnr_out"])
    assert normwise(out[0, 0, ::8, ::8].numpy(), subs[f"out_{name}"]) <= 2e-3


def test_set12_quality_converted():
    from dagl_amd import trunk
    from dagl_amd.net import RR, seeded_state_dict
    seed = json.load(open(os.path.join(GOLDEN_DIR, "set12_psnr_ref.json")))["seed"]
    m = RR().eval()
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    m = trunk.convert(m).to(DEV)
    for name in ("01", "07"):
        _set12(m, name, "set12_out_sub.npz", "set12_psnr_ref.json")
    z = np.load(os.path.join(GOLDEN_DIR, "quality_ckpt_fp16.npz"))
    t = RR().eval()
    t.load_state_dict({k: torch.from_numpy(z[k].astype(np.float32)) for k in z.files}, strict=True)
    t = trunk.convert(t).to(DEV)
    _set12(t, "05", "set12_out_sub_trained.npz", "set12_psnr_ref_trained.json", batched=True)


def _rr3(seed=3):
    from dagl_amd.net import RR, seeded_state_dict
    m = RR(n_colors=3)
    m.load_state_dict(seeded_state_dict(m.state_dict(), seed), strict=True)
    return m


def _set_mode(m, mode, k=8):
    from dagl_amd.ce import CE
    for mod in m.modules():
        if isinstance(mod, CE):
            mod.select_mode = mode
            if mode == "topk":
                mod.select_k = k


def test_converted_network_never_calls_the_stock_convolution(monkeypatch):
    import torch.nn.functional as F
    from dagl_amd import trunk
    from dagl_amd.train import TrainOptions, TrainStep, freeze_unused, make_optimizer
    calls = []

    def refuse(*a, **kw):
        calls.append(1)
        raise RuntimeError("stock conv2d called")
    g = torch.Generator(device=DEV).manual_seed(1)
    hr = torch.rand(2, 3, 48, 48, device=DEV, generator=g)
    monkeypatch.setattr(F, "conv2d", refuse)
    ctl = _rr3().to(DEV)                                    # control: the unconverted model reaches the patched function
    with pytest.raises(RuntimeError, match="stock conv2d"):
        ctl(hr)
    assert calls
    calls.clear()
    net = trunk.convert(_rr3()).to(DEV)
    _set_mode(net, "topk", 8)
    freeze_unused(net)
    opt = TrainOptions(task="dn_real")
    step = TrainStep(net, make_optimizer(net, opt), opt, torch.Generator(device=DEV).manual_seed(2))
    loss, _ = step(hr)
    assert torch.isfinite(loss)
    _set_mode(net, "adaptive")                              # dense masks at this initialisation: CES runs its per-head path + mix conv
    net.eval()
    with torch.no_grad():
        out = net(hr)
    assert torch.isfinite(out).all()
    assert not calls


def test_converted_network_gradients_are_deterministic():
    from dagl_amd import trunk
    from dagl_amd.train import freeze_unused, task_loss
    net = trunk.convert(_rr3()).to(DEV).train()
    _set_mode(net, "topk", 8)
    freeze_unused(net)
    g = torch.Generator(device=DEV).manual_seed(4)
    hr = torch.rand(2, 3, 64, 64, device=DEV, generator=g)
    lr = hr + 0.2 * torch.randn(2, 3, 64, 64, device=DEV, generator=g)
    runs = []
    for _ in range(3):
        for p in net.parameters():
            p.grad = None
        out = net(lr)
        task_loss(out, hr, "dn_real").backward()
        runs.append((out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    (o1, g1), (o2, g2) = runs[1], runs[2]
    assert torch.equal(o1, o2)
    assert g1.keys() == g2.keys() and len(g1) > 100
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


def test_half_precision_input_is_refused():
    from dagl_amd import DaglError, trunk
    conv = trunk.convert(nn.Conv2d(8, 8, 3, padding=1)).to(DEV)
    with pytest.raises(DaglError, match="fp32 GPU"):
        conv(torch.zeros(1, 8, 6, 6, device=DEV, dtype=torch.float16))
    conv.half()
    with pytest.raises(DaglError):
        conv(torch.zeros(1, 8, 6, 6, device=DEV))


# ---- the fused ResBlock away from 64 channels and W % 4 == 0 ------------------------------------------------------------------
RESBLOCK_SHAPES = ((1, 5, 37), (2, 3, 130), (1, 9, 66), (1, 2, 257))
_resblock_seeds = {}


def _resblock_inputs(n_feats, res_scale, shape, seed):
    from dagl_amd.net import ResBlock
    torch.manual_seed(seed)
    rb = ResBlock(n_feats, res_scale)
    with torch.no_grad():
        rb.body[1].weight.fill_(0.2)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((shape[0], n_feats) + shape[1:], generator=g)
    up = torch.randn((shape[0], n_feats) + shape[1:], generator=g)
    return rb, x, up


def _unambiguous_seed(n_feats, shape):
    """The first seed from 100 (of at most 40) at which no pre-activation of the stock block sits near the PReLU kink: min |pre64| >=
    32 max |pre32 - pre64|, both from the stock float64 / float32 block on the CPU.  There fp32 and fp64 take the same branch at
    every element, by about ten times the slack _bound grants, so a branch flip cannot be mistaken for (or excuse) an error."""
    from dagl_amd.net import ResBlock
    key = (n_feats, shape)
    if key not in _resblock_seeds:
        for seed in range(100, 140):
            rb, x, _ = _resblock_inputs(n_feats, 1.0, shape, seed)
            pre = {}
            for tag, dt in (("64", torch.float64), ("32", torch.float32)):
                m = ResBlock(n_feats, 1.0).to(dt)
                m.load_state_dict(rb.state_dict())
                with torch.no_grad():
                    pre[tag] = m.body[0](x.to(dt)).double()
            if float(pre["64"].abs().min()) >= 32.0 * float((pre["32"] - pre["64"]).abs().max()):
                _resblock_seeds[key] = seed
                break
        else:
            raise AssertionError(f"no unambiguous seed in 100..139 for {key}")
    return _resblock_seeds[key]


def _resblock_case(n_feats, res_scale, shape, seed, layout="contiguous"):
    from dagl_amd import trunk
    from dagl_amd.net import ResBlock
    rb, x, up = _resblock_inputs(n_feats, res_scale, shape, seed)
    if layout == "expanded grad":
        up = torch.ones_like(up)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        m = ResBlock(n_feats, res_scale).to(dt)
        m.load_state_dict(rb.state_dict())
        xi = x.to(dt).clone().requires_grad_(True)
        y = m(xi)
        (y * up.to(dt)).sum().backward()
        res[tag] = [y.detach(), xi.grad] + [p.grad for p in m.parameters()]
    lib = ResBlock(n_feats, res_scale)
    lib.load_state_dict(rb.state_dict())
    lib = trunk.convert(lib).to(DEV)
    y, d_x = _run_layouts(lib, x, up, layout)
    assert type(y.grad_fn).__name__.startswith("_ResBlockFn")         # the fused path ran
    got = [y.detach(), d_x] + [p.grad for p in lib.parameters()]
    names = ["out", "d_x"] + [n for n, _ in lib.named_parameters()]
    for name, a, r64, r32 in zip(names, got, res["64"], res["32"]):
        _bound(a.cpu().double().numpy(), r64.numpy(), r32.double().numpy(), (n_feats, res_scale, shape, seed, layout, name))


def _run_layouts(lib, x, up, layout):
    """Forward and backward of ``lib`` on the GPU with the input / upstream gradient in ``layout`` -> (y, d_x as [B,C,H,W])."""
    if layout == "channels_last":
        xi = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        assert not xi.is_contiguous() or 1 in xi.shape[1:]
        xin = xi
    elif layout == "sliced":
        wide = torch.full(x.shape[:3] + (x.shape[3] + 3,), 7.0)
        wide[..., 1:-2] = x
        xi = wide.to(DEV).requires_grad_(True)
        xin = xi[..., 1:-2]
        assert not xin.is_contiguous()
    else:
        xi = x.to(DEV).clone().requires_grad_(True)
        xin = xi
    y = lib(xin)
    if layout == "expanded grad":
        y.sum().backward()                                            # the upstream gradient is an expanded scalar (strides 0)
    else:
        (y * up.to(DEV)).sum().backward()
    d_x = xi.grad
    if layout == "sliced":
        assert bool((d_x[..., :1] == 0).all()) and bool((d_x[..., -2:] == 0).all())
        d_x = d_x[..., 1:-2]
    return y, d_x


@pytest.mark.parametrize("res_scale", [1.0, 0.1])
@pytest.mark.parametrize("n_feats", [64, 33, 20, 5])
def test_fused_resblock_channel_classes_vs_fp64(n_feats, res_scale):
    for shape in RESBLOCK_SHAPES:
        _resblock_case(n_feats, res_scale, shape, _unambiguous_seed(n_feats, shape))


@pytest.mark.parametrize("layout", ["channels_last", "sliced", "expanded grad"])
def test_fused_resblock_input_layouts(layout):
    shape = (2, 3, 130)
    _resblock_case(20, 0.1, shape, _unambiguous_seed(20, shape), layout)


@pytest.mark.parametrize("layout", ["channels_last", "sliced", "expanded grad"])
@pytest.mark.parametrize("cin,cout,k", [(20, 33, 3), (33, 20, 1)])
def test_single_layer_input_layouts(cin, cout, k, layout):
    from dagl_amd import trunk
    shape = (2, 9, 66)
    g = torch.Generator().manual_seed(31 * cin + k)
    conv = nn.Conv2d(cin, cout, k, padding=k // 2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (cin * k * k) ** 0.5)
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    x = torch.randn((shape[0], cin) + shape[1:], generator=g)
    up = torch.randn((shape[0], cout) + shape[1:], generator=g)
    if layout == "expanded grad":
        up = torch.ones_like(up)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        c = nn.Conv2d(cin, cout, k, padding=k // 2).to(dt)
        c.load_state_dict(conv.state_dict())
        xi = x.to(dt).clone().requires_grad_(True)
        y = c(xi)
        (y * up.to(dt)).sum().backward()
        res[tag] = [y.detach(), xi.grad, c.weight.grad, c.bias.grad]
    lib = trunk.convert(nn.Conv2d(cin, cout, k, padding=k // 2))
    lib.load_state_dict(conv.state_dict())
    lib = lib.to(DEV)
    y, d_x = _run_layouts(lib, x, up, layout)
    got = [y.detach(), d_x, lib.weight.grad, lib.bias.grad]
    for name, a, r64, r32 in zip(("out", "d_x", "d_w", "d_b"), got, res["64"], res["32"]):
        _bound(a.cpu().double().numpy(), r64.numpy(), r32.double().numpy(), (cin, cout, k, layout, name))


# ---- the packed-weight cache follows the weights ------------------------------------------------------------------------------
def _cache_model(kind):
    from dagl_amd.net import ResBlock
    return nn.Conv2d(20, 33, 3, padding=1) if kind == "conv" else ResBlock(20, 0.1)


def _cache_convs(m):
    return [c for c in m.modules() if isinstance(c, nn.Conv2d)]


def _new_weight(c, seed):
    return torch.randn(c.weight.shape, generator=torch.Generator().manual_seed(seed)) / (c.in_channels * 9) ** 0.5


def _mutate_optimizer_step(m):
    torch.optim.SGD(m.parameters(), lr=0.5).step()                    # the gradients of the first backward


def _mutate_no_grad_mul(m):
    with torch.no_grad():
        for c in _cache_convs(m):
            c.weight.mul_(2)


def _mutate_load_state_dict(m):
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for i, c in enumerate(_cache_convs(m)):
        name = next(n for n, p in m.named_parameters() if p is c.weight)
        sd[name] = _new_weight(c, 50 + i).to(DEV)
    m.load_state_dict(sd)


def _mutate_assign_data(m):
    for i, c in enumerate(_cache_convs(m)):
        c.weight.data = _new_weight(c, 60 + i).to(DEV)


def _mutate_cpu_round_trip(m):
    m.to("cpu")
    with torch.no_grad():
        for c in _cache_convs(m):
            c.weight.mul_(0.5)
    m.to(DEV)


def _mutate_data_write_then_invalidate(m):
    from dagl_amd import trunk
    for c in _cache_convs(m):
        c.weight.data.mul_(2)                                         # neither the version nor the storage changes: documented limit
    assert trunk.invalidate_packed(m) is m


_MUTATIONS = {"optimizer step": _mutate_optimizer_step, "no_grad mul_": _mutate_no_grad_mul, "load_state_dict": _mutate_load_state_dict,
              "weight.data = t": _mutate_assign_data, "to cpu and back": _mutate_cpu_round_trip,
              "data.mul_ + invalidate_packed": _mutate_data_write_then_invalidate}


@pytest.mark.parametrize("how", list(_MUTATIONS))
@pytest.mark.parametrize("kind", ["conv", "resblock"])
def test_packed_weight_cache_follows_the_weights(kind, how):
    """After one forward and backward (both packings cached) the weights change; the next forward and backward are those of a freshly
    built layer holding the new weights -- the same kernels on the same operands: the same bits."""
    from dagl_amd import trunk
    torch.manual_seed(3)
    m = trunk.convert(_cache_model(kind)).to(DEV)
    assert all(type(c) is trunk.Conv2d for c in _cache_convs(m))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 20, 9, 66, generator=g).to(DEV)

    def run(model):
        for p in model.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        y = model(xi)
        up = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        (y * up).sum().backward()
        return [y.detach(), xi.grad] + [p.grad for p in model.parameters()]

    before = run(m)
    assert all(len(c.__dict__["_trunk_packed"]) == 2 for c in _cache_convs(m))       # forward and transposed packings are cached
    old = [c.weight.detach().clone() for c in _cache_convs(m)]
    _MUTATIONS[how](m)
    assert all(not torch.equal(c.weight.detach(), o) for c, o in zip(_cache_convs(m), old))
    fresh = _cache_model(kind)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    fresh = trunk.convert(fresh).to(DEV)
    after, want = run(m), run(fresh)
    names = ["out", "d_x"] + [n for n, _ in m.named_parameters()]
    assert not torch.equal(after[0], before[0])
    for name, a, b in zip(names, after, want):
        assert torch.equal(a, b), (kind, how, name, float((a - b).abs().max()))
