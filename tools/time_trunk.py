#!/usr/bin/env python3
"""Run ON THE GPU BOX: the trunk's convolutions, stock (torch / MIOpen) against the library (dagl_amd.trunk), in one process with
device events, the two alternated, median and spread over repeats:
  * each conv kind of a 3x3 64 -> 64 convolution (forward, input gradient, weight gradient + bias) at [8,64,128,128] and at the
    batched leaf tiles [64,64,72,72]
  * the [8,3,128,128] top-k 8 TrainStep of RR(n_colors=3)
  * chop_forward_batched of a 256^2 image (RR(), top-k 8 and the shipped adaptive semantics at default-like init: dense masks)
     python tools/time_trunk.py [--repeats N] [--only train]      (--only train --steps K: just the converted training step, for a
                                                                   profiler run)"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagl_amd import ops, trunk  # noqa: E402
from dagl_amd.ce import CE  # noqa: E402
from dagl_amd.net import RR, chop_forward_batched, seeded_state_dict  # noqa: E402
from dagl_amd.train import TrainOptions, TrainStep, freeze_unused, make_optimizer  # noqa: E402

DEV = torch.device("cuda:0")


def per_call_ms(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def alternate(variants, n, repeats, warmup=2):
    """{name: [ms per call of each repeat]}, the variants alternated repeat by repeat."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            out[k].append(per_call_ms(fn, n))
    return out


def report(what, res, flop=None):
    parts = []
    for k, v in res.items():
        med = statistics.median(v)
        extra = f", {flop / med / 1e9:.0f} TF" if flop else ""
        parts.append(f"{k} {med:.4f} ms [{min(v):.4f} .. {max(v):.4f}]{extra}")
    ratio = statistics.median(res["library"]) / statistics.median(res["stock"])
    print(f"{what}: " + "; ".join(parts) + f"; library / stock {ratio:.3f}", flush=True)


def conv_kinds(shape, repeats):
    B, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(B, C, H, W, device=DEV, generator=g)
    dy = torch.randn(B, C, H, W, device=DEV, generator=g)
    w = torch.randn(C, C, 3, 3, device=DEV, generator=g) / 24.0
    b = torch.randn(C, device=DEV, generator=g) * 0.1
    packed, packed_t = ops.trunk_pack_weights(w), ops.trunk_pack_weights(w, True)
    flop = 2.0 * B * H * W * C * C * 9
    conv_bwd = torch.ops.aten.convolution_backward
    stock = {
        "forward": lambda: F.conv2d(x, w, b, padding=1),
        "input gradient": lambda: conv_bwd(dy, x, w, [C], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False]),
        "weight gradient": lambda: conv_bwd(dy, x, w, [C], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True]),
    }
    lib = {
        "forward": lambda: ops.trunk_conv_forward(x, packed, b, C, 3),
        "input gradient": lambda: ops.trunk_conv_input_grad(dy, packed_t, C, 3),
        "weight gradient": lambda: ops.trunk_conv_weight_grad(x, dy, 3),
    }
    # the same numbers first (normwise against the stock result)
    agree = {
        "forward": (lib["forward"]()[0], stock["forward"]()),
        "input gradient": (lib["input gradient"]()[0], stock["input gradient"]()[0]),
        "weight gradient": (lib["weight gradient"]()[0], stock["weight gradient"]()[1]),
    }
    for kind in stock:
        a, r = agree[kind]
        err = float((a - r).abs().max() / r.abs().max())
        res = alternate({"stock": stock[kind], "library": lib[kind]}, 20, repeats)
        report(f"conv 3x3 64->64 {kind} {list(shape)} (normwise vs stock {err:.1e})", res, flop)


def rr3_topk8(seed=7):
    net = RR(n_colors=3)
    net.load_state_dict(seeded_state_dict(net.state_dict(), seed), strict=True)
    for m in net.modules():
        if isinstance(m, CE):
            m.select_mode, m.select_k = "topk", 8
    return net


def train_steps(repeats, steps):
    hr = torch.rand(8, 3, 128, 128, generator=torch.Generator().manual_seed(200)).to(DEV)
    runs = {}
    base = rr3_topk8()
    for name, net in (("stock", copy.deepcopy(base)), ("library", trunk.convert(copy.deepcopy(base)))):
        net = net.to(DEV)
        freeze_unused(net)
        opt = TrainOptions(task="dn_real", lr=1e-4)
        step = TrainStep(net, make_optimizer(net, opt), opt, generator=torch.Generator(device=DEV).manual_seed(300))
        runs[name] = lambda step=step: step(hr)
    res = alternate(runs, steps, repeats, warmup=4)
    report("TrainStep RR(n_colors=3) [8,3,128,128] top-k 8", res)


def inference(repeats):
    img = torch.rand(1, 1, 256, 256, generator=torch.Generator().manual_seed(5)).to(DEV)
    base = RR().eval()
    base.load_state_dict(seeded_state_dict(base.state_dict(), 11), strict=True)
    for mode in ("topk", "adaptive"):
        variants = {}
        for name, net in (("stock", copy.deepcopy(base)), ("library", trunk.convert(copy.deepcopy(base)))):
            for m in net.modules():
                if isinstance(m, CE):
                    m.select_mode = mode
                    if mode == "topk":
                        m.select_k = 8
            net = net.to(DEV)

            def run(net=net):
                with torch.no_grad():
                    return chop_forward_batched(net, img)
            variants[name] = run
        with torch.no_grad():
            a, r = variants["library"](), variants["stock"]()
        err = float((a - r).abs().max() / r.abs().max())
        res = alternate(variants, 3, repeats)
        report(f"chop_forward_batched 256^2 RR() {'top-k 8' if mode == 'topk' else 'adaptive (dense masks)'} "
               f"(normwise vs stock {err:.1e})", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", choices=["train"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_trunk.py runs on the GPU"
    print(f"[time_trunk] {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    if a.only == "train":
        net = trunk.convert(rr3_topk8()).to(DEV)
        freeze_unused(net)
        opt = TrainOptions(task="dn_real", lr=1e-4)
        step = TrainStep(net, make_optimizer(net, opt), opt, generator=torch.Generator(device=DEV).manual_seed(300))
        hr = torch.rand(8, 3, 128, 128, generator=torch.Generator().manual_seed(200)).to(DEV)
        for _ in range(3):
            step(hr)
        torch.cuda.synchronize()
        print(f"converted TrainStep: {per_call_ms(lambda: step(hr), a.steps):.2f} ms per step", flush=True)
        return
    for shape in ((8, 64, 128, 128), (64, 64, 72, 72)):
        conv_kinds(shape, a.repeats)
    train_steps(a.repeats, a.steps)
    inference(a.repeats)


if __name__ == "__main__":
    main()
