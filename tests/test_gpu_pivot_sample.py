"""Top-k sampling stage: pivot_sample_kernel (csrc/screen.hip) picks its step's pivot keys, fetches their rows from Xh and scores
them in ONE launch, in place of pivot_keys_kernel + the streaming sampling launch with the pivot matrix between them.  Nothing the
call computes may change: DAGL_PIVOT_SAMPLE=0 in the environment keeps the two launches, and every case below runs in two fresh
child processes -- that setting and the default; the library reads it once per process -- whose block outputs, pivot indices, key
row sums and call infos must agree bit for bit.  One pair of children computes all cases (a child costs a process start and a
library load), each case is a test of its own over what they wrote.

Shapes: the smallest the pivot rule takes (maps of <= 16 384 keys start on the tight threshold, so the sampled one is forced):
136 x 136 (18 496 keys, N a multiple of 64; 8-wave blocks, 10 pivot steps behind 58 key chunks: 48 chunks sample nothing),
132 x 140 (the last key block and the last query tile partial), a batch of two (per-image strides), k = 1 / 8 / 16, and k = 17,
which keeps the tile sampling.  Crafted maps: a constant 64-key block (every row sum of the block equal: the tie goes to the lower
keys), a NaN pixel (NaN row sums count as -inf; NaN-filled output), an all-zero image (every row sum equal, theta = 0: the redo
pass serves the call).  A CES stage of four heads, a workspace that "auto" has moved to the tight threshold (Set12 features at
256 x 256: 16-wave blocks, the kernel leaves the pivots alone and samples key tiles as before), and a captured graph."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 240

# name -> (B, H, W, k, crafted input or None)
CASES = {
    "136x136_k1": (1, 136, 136, 1, None),
    "136x136_k8": (1, 136, 136, 8, None),
    "136x136_k16": (1, 136, 136, 16, None),
    "136x136_k17_tile_sampling": (1, 136, 136, 17, None),
    "132x140_partial_block_and_tile": (1, 132, 140, 8, None),
    "batch2_136x132": (2, 136, 132, 8, None),
    "constant_key_block": (1, 136, 136, 8, "const"),
    "nan_pixel": (1, 136, 136, 8, "nan"),
    "all_zero_image": (1, 136, 136, 8, "zero"),
}
CONST_BLOCK = 128                      # key block 128 of a 136-wide map = keys 8192 .. 8255 = row 60, columns 32 .. 95
W_SEED, F_SEED = 2024, 100


def _params(seed=W_SEED):
    from dagl_amd.synth import make_ce_params
    return {n: torch.from_numpy(a) for n, a in make_ce_params(seed, variant="default").items()}


def _input(name):
    from dagl_amd.synth import make_features
    B, H, W, k, craft = CASES[name]
    params = _params()
    x = torch.from_numpy(make_features(F_SEED, B, 64, H, W))
    if craft == "const":
        # every 7 x 7 patch of b1 = g(x) (3 x 3) around the block's 64 keys sees the same input: zero, so that these keys are light
        # (their features come from the biases alone) and stay away from every query's k-th place
        x[0, :, 60 - 4:60 + 5, 32 - 4:96 + 4] = 0.0
    elif craft == "nan":
        x[0, 3, 70, 41] = float("nan")
    elif craft == "zero":
        x.zero_()
        for n in params:
            if n.endswith("bias"):
                params[n].zero_()
    return x, params, k


def _module(params, k):
    from dagl_amd.ce import CE
    ce = CE(in_channels=64)
    ce.load_state_dict(params, strict=True)
    ce.select_mode, ce.select_k = "topk", k
    return ce.to(DEV).eval()


def _bits(t):
    return t.detach().float().cpu().contiguous().numpy().view(np.int32)


# ---- the child: every case under the process's DAGL_PIVOT_SAMPLE, results into one .npz ----------------------------------------

def _child_block_case(name, res):
    from dagl_amd import ops
    from dagl_amd._lib import DaglError
    x, params, k = _input(name)
    ce = _module(params, k)
    ws = ops.Workspace()

    def call(debug):
        with torch.no_grad():
            b1, b2, thr, bias = ce._prologue(x.to(DEV))
            return ops.ce_forward(b1.contiguous(), b2.contiguous(), thr.contiguous(), bias.contiguous(), ce.fc1[0].weight, ce.fc1[0].bias,
                                  ce.fc2[0].weight, ce.fc2[0].bias, mode="topk", k=k, workspace=ws, debug=debug, return_info=True,
                                  sampled_topk=True)
    out, info = call(True)                               # (the debug entry point reports the redone queries ...)
    res[name + "/out"] = _bits(out)
    res[name + "/info"] = np.array([info["path"], info["max_degree"], info["redone_queries"]], dtype=np.int64)
    out2, _ = call(False)                                # (... but its aggregated rows overwrite the row sums: read them after a plain call)
    res[name + "/out_plain"] = _bits(out2)
    try:
        idx, rowsum = ops.ce_pivot_debug(x.shape, "topk", k, ws, torch.device(DEV))
        res[name + "/pidx"] = idx.cpu().numpy()
        res[name + "/rowsum"] = _bits(rowsum)
    except DaglError:                                    # (k = 17: no pivots)
        pass


def _child_ces_stage(res):
    from dagl_amd import ops
    from dagl_amd.synth import make_ce_params, make_features
    x = torch.from_numpy(make_features(F_SEED, 1, 64, 136, 136)).to(DEV)
    prm = [{n: torch.from_numpy(a).to(DEV).contiguous() for n, a in make_ce_params(80 + h, variant="default").items() if not n.startswith("W.")}
           for h in range(4)]
    g = torch.Generator().manual_seed(9)
    mix_w = (torch.rand(64, 64, 1, 1, generator=g) - 0.5).mul(0.25).to(DEV)
    mix_b = (torch.rand(64, generator=g) - 0.5).mul(0.1).to(DEV)
    with torch.no_grad():
        got, info = ops.ces_stage_forward(x, prm, mix_w, mix_b, mode="topk", k=8, sampled_topk=True)
    res["ces_stage/out"] = _bits(got)
    res["ces_stage/info"] = np.array([info["path"], info["max_degree"]], dtype=np.int64)


def _child_tight_workspace(res):
    from tests.test_gpu_real_features import real_features
    x, ce = real_features("img_01")
    ce.topk_threshold = "auto"
    ce.reset_topk_policy()
    with torch.no_grad():
        for n in range(3):                               # the first call flips the policy word; the later ones find it tight
            y = ce(x)
            res[f"tight_workspace/out{n}"] = _bits(y)
    res["tight_workspace/is_tight"] = np.array([int(ce.topk_policy_is_tight())])


def _child_main(out_path):
    res = {}
    for name in CASES:
        _child_block_case(name, res)
    _child_ces_stage(res)
    _child_tight_workspace(res)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


# ---- the parent ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pivot_sample")
    out = {}
    for tag, setting in (("two_launches", "0"), ("one_launch", None)):
        env = dict(os.environ)
        env.pop("DAGL_PIVOT_SAMPLE", None)
        if setting is not None:
            env["DAGL_PIVOT_SAMPLE"] = setting
        path = str(d / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        assert r.returncode == 0, f"child ({tag}) exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        out[tag] = dict(np.load(path))
    return out


def _same(runs, key):
    a, b = runs["two_launches"][key], runs["one_launch"][key]
    assert a.shape == b.shape and np.array_equal(a, b), f"{key}: {int((a != b).sum())} of {a.size} words differ"
    return b


def _picks_follow_the_rule(pidx, rowsum_bits, N):
    """Every block's two pivots from the row sums the library formed: the largest sum, the lowest key among equals; then the same
    among the rest; NaN counts as -inf; keys past N do not exist."""
    rs = rowsum_bits.view(np.float32).astype(np.float64)
    rs = np.where(np.isnan(rs), -np.inf, rs)
    B, n_blk, _ = pidx.shape
    for b in range(B):
        for v in range(n_blk):
            lo, hi = 64 * v, min(64 * v + 64, N)
            s = rs[b, lo:hi]
            p0 = int(np.argmax(s))                       # (argmax: the first of equals, -inf among -inf included)
            want = [lo + p0, -1]
            if hi - lo >= 2:
                rest = np.arange(hi - lo) != p0
                want[1] = lo + int(np.flatnonzero(rest & (s == s[rest].max()))[0])
            assert list(pidx[b, v]) == want, (b, v, pidx[b, v], want)


@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_computes_what_the_two_launches_compute(runs, name):
    B, H, W, k, craft = CASES[name]
    out = _same(runs, name + "/out")
    _same(runs, name + "/out_plain")
    info = _same(runs, name + "/info")
    assert np.array_equal(runs["one_launch"][name + "/out"], runs["one_launch"][name + "/out_plain"])
    path, _, redone = (int(v) for v in info)
    if craft != "nan":
        assert path == 3
    if k == 17:
        assert name + "/pidx" not in runs["one_launch"] and name + "/pidx" not in runs["two_launches"]
        assert redone == 0
        return
    pidx = _same(runs, name + "/pidx")
    rowsum = _same(runs, name + "/rowsum")
    assert pidx.shape == (B, (H * W + 63) // 64, 2)
    _picks_follow_the_rule(pidx, rowsum, H * W)
    if craft == "nan":
        assert np.isnan(out.view(np.float32)).all()
    elif craft == "zero":
        assert redone > 0 and np.isfinite(out.view(np.float32)).all()      # theta = 0: every key a candidate, the redo pass serves the call
        assert (pidx.reshape(-1, 2) == np.arange(pidx.shape[1])[:, None] * 64 + np.array([0, 1])).all()
    else:
        assert np.isfinite(out.view(np.float32)).all()
        if craft is None:
            assert redone == 0
    if craft == "const":
        blk = rowsum[0, 64 * CONST_BLOCK:64 * CONST_BLOCK + 64]
        assert (blk == blk[0]).all(), "the crafted block's row sums are not all equal"
        assert list(pidx[0, CONST_BLOCK]) == [64 * CONST_BLOCK, 64 * CONST_BLOCK + 1]


def test_constant_key_block_is_resolved_by_the_reference_alone(runs):
    """The crafted map has no tie at any query's k-th place (the constant keys are light: none of them is near it), so the reference
    defines the answer, and both settings give it."""
    from oracle.ce_oracle import ce_forward_oracle
    from tests.helpers import normwise
    x, params, k = _input("constant_key_block")
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        want, st = ce_forward_oracle(x, params, mode="topk", k=k, dtype=torch.float64, stages=True)
    top = torch.topk(st["S"][0], k + 1, dim=1).values
    gap = (top[:, k - 1] - top[:, k]).min().item()
    print(f"[pivot sample] constant block: smallest gap between a k-th and a (k+1)-th score {gap:.3e}")
    assert gap > 1e-6
    got = runs["one_launch"]["constant_key_block/out"].view(np.float32)
    assert normwise(got, want.float().numpy()) <= 1e-4


def test_ces_stage_of_four_heads(runs):
    _same(runs, "ces_stage/out")
    info = _same(runs, "ces_stage/info")
    assert int(info[0]) == 3


def test_tight_workspace_leaves_the_pivots_alone(runs):
    assert int(runs["one_launch"]["tight_workspace/is_tight"][0]) == 1 and int(runs["two_launches"]["tight_workspace/is_tight"][0]) == 1
    for n in range(3):
        _same(runs, f"tight_workspace/out{n}")


def test_one_launch_replays_from_a_captured_graph():
    """This process has the default setting: the captured forward holds pivot_sample_kernel (16-wave blocks at 256 x 256 under the
    policy word, which stays on the sampled threshold for these features)."""
    from dagl_amd.synth import make_features
    assert os.environ.get("DAGL_PIVOT_SAMPLE") in (None, "1")
    ce = _module(_params(71), 8)
    x_static = torch.from_numpy(make_features(71, 1, 64, 256, 256)).to(DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm-up on the capture stream: workspace, packed weights, policy
            for _ in range(3):
                eager = ce(x_static).clone()
        torch.cuda.current_stream().wait_stream(side)
        assert not ce.topk_policy_is_tight()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_static = ce(x_static)
        for _ in range(3):
            out_static.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out_static, eager)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child_main(sys.argv[1])
