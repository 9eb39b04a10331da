#!/usr/bin/env python3
"""Gradient golden vectors from the REFERENCE block's own autograd (CPU, build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad.py

For each case the reference ``CE`` (DN_Gray/model/dagl.py:174-277; fixed-k variant from
.ipynb_checkpoints/GReccR2b_3mh_1-checkpoint.py) is run WITH autograd on seeded inputs, the scalar
``loss = sum(out * G)`` (G seeded, numpy PCG64) is back-propagated the way DN_Gray/trainer.py:44-50 does, and only
DATA is stored in ``tests/golden/grad_<case>.npz``:

    out          [B,16,H,W]      forward output
    d_x          [B,64,H,W]      dL/d input feature map
    d_<param>    gradient of every parameter that takes part (fc weights: every ``fc_step``-th element, flattened)
    meta         json            case description

and, for every case, the gradients of the bias parameters from the reference run in float64 (module, input and G in double)
in ``tests/golden/grad_ref64_biases.json`` ({case name: {"d_<param>": [values]}}, exact float64 values): the fp32 values of
sums with heavy cancellation (the scalar head biases) depend on the CPU's summation order, these do not.

The fixed-k variant returns ``b + W(y)``; the loss is put on ``y`` (the 16-channel block output, captured at W's input).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from dagl_amd.synth import make_ce_params, make_features  # noqa: E402
from make_golden import _load_module  # noqa: E402

# (name, task, seed, variant, sparse_gain, mode, k, B, H, W)
CASES = [
    ("gray_sparse_b2_40x36", "DN_Gray", 31, "sparse", 1.8, "adaptive", 0, 2, 40, 36),
    ("gray_sparse_64x64", "DN_Gray", 32, "sparse", 2.2, "adaptive", 0, 1, 64, 64),
    ("topk8_b2_45x38", "TOPK", 33, "default", 2.0, "topk", 8, 2, 45, 38),
    ("topk4_64x64", "TOPK", 34, "default", 2.0, "topk", 4, 1, 64, 64),
    # dense neighbourhoods: default-initialised heads keep ~95 % of the keys; "longtail": a few queries beyond 64 keys
    ("gray_default_64x64", "DN_Gray", 35, "default", 2.0, "adaptive", 0, 1, 64, 64),
    ("gray_longtail_b2_40x36", "DN_Gray", 36, "sparse", 1.45, "adaptive", 0, 2, 40, 36),
    # CE(in_channels != 64): an 11th column = the input width (dagl.py:94-109 builds heads as CE(in_channels=n_feats))
    ("gray_sparse_c32_b2_36x40", "DN_Gray", 37, "sparse", 1.8, "adaptive", 0, 2, 36, 40, 32),
    ("gray_default_c96_32x36", "DN_Gray", 38, "default", 2.0, "adaptive", 0, 1, 32, 36, 96),
]
FC_STEP = 5


def loss_weights(seed: int, shape):
    return np.random.Generator(np.random.PCG64(seed + 1000)).standard_normal(shape).astype(np.float32)


def reference_grads(case, dtype):
    """One reference forward + backward of ``case`` in ``dtype`` -> (out, d_x, {param name: gradient})."""
    name, task, seed, variant, gain, mode, k, B, H, W = case[:10]
    Cin = case[10] if len(case) > 10 else 64
    mod = _load_module(task)
    np_params = make_ce_params(seed, in_channels=Cin, variant=variant, sparse_gain=gain)
    default_dtype = torch.get_default_dtype()
    torch.set_default_dtype(dtype)          # (tensors the reference makes on its own follow the run's precision)
    try:
        x = torch.from_numpy(make_features(seed, B, Cin, H, W)).to(dtype).requires_grad_(True)
        if task == "TOPK":
            ce = mod.CE(in_channels=Cin, num_edge=k)
            sd = {n: torch.from_numpy(a) for n, a in np_params.items() if not n.startswith(("thr_conv", "bias_conv"))}
            ce.load_state_dict(sd, strict=False)
        else:
            ce = mod.CE(in_channels=Cin)
            ce.load_state_dict({n: torch.from_numpy(a) for n, a in np_params.items()}, strict=True)
        ce = ce.to(dtype)
        ce.train()
        grabbed = {}
        if task == "TOPK":
            ce.W.register_forward_pre_hook(lambda m, inp: grabbed.__setitem__("y", inp[0]))
        y = ce(x)
        out = grabbed["y"] if task == "TOPK" else y
        G = torch.from_numpy(loss_weights(seed, tuple(out.shape))).to(dtype)
        (out * G).sum().backward()
    finally:
        torch.set_default_dtype(default_dtype)
    grads = {n: p.grad for n, p in ce.named_parameters() if not n.startswith(("W.", "conv33")) and p.grad is not None}
    return out.detach(), x.grad, grads


def run_case(case):
    """Write grad_<case>.npz (fp32 run); return the float64 run's bias gradients for REF64_JSON."""
    name, task, seed, variant, gain, mode, k, B, H, W = case[:10]
    Cin = case[10] if len(case) > 10 else 64
    out, d_x, grads = reference_grads(case, torch.float32)
    _, _, grads64 = reference_grads(case, torch.float64)
    arrays = dict(out=out.numpy().astype(np.float32), d_x=d_x.numpy().astype(np.float32))
    for n, g in grads.items():
        g = g.numpy().astype(np.float32)
        arrays["d_" + n] = g.reshape(-1)[::FC_STEP].copy() if n in ("fc1.0.weight", "fc2.0.weight") else g
    meta = dict(name=name, task=task, seed=seed, variant=variant, sparse_gain=gain, mode=mode, k=k, B=B, C=Cin, H=H, W=W,
                fc_step=FC_STEP, torch=torch.__version__)
    np.savez_compressed(os.path.join(HERE, "grad_" + name + ".npz"), meta=json.dumps(meta), **arrays)
    print(name, {n: (a.shape, float(np.abs(a).max())) for n, a in arrays.items()}, flush=True)
    return {"d_" + n: g.reshape(-1).tolist() for n, g in grads64.items() if n.endswith(".bias")}


REF64_JSON = os.path.join(HERE, "grad_ref64_biases.json")

if __name__ == "__main__":
    torch.manual_seed(0)
    only = set(sys.argv[1:])
    ref64 = json.load(open(REF64_JSON)) if os.path.exists(REF64_JSON) else {}
    for c in CASES:
        if not only or c[0] in only:
            ref64[c[0]] = run_case(c)
    with open(REF64_JSON, "w") as f:
        json.dump(ref64, f, indent=1)
        f.write("\n")
