"""Top-k screen: the sampled candidate threshold taken from PIVOT keys -- the two keys with the largest feature row sum of every 64
consecutive keys (csrc/pivot.hip) -- instead of every 8th key tile.  Any set of distinct keys gives a valid threshold ("at least k
distinct keys score >= theta"), so the pivots may change how many candidates reach the exact rescoring and nothing else: same
bits as the tight threshold, right answers when the pivots are the worst possible choice, the parent's behaviour on non-finite and
degenerate maps, and no change outside the rule (k <= 16, N >= 1024 k, a sampled stride >= 2).

Small maps, sampled threshold forced (maps of <= 16 384 keys start on the tight one).  The issue's 64 x 24 case cannot take the
screen at all (1536 keys < 2048); 96 x 24 is the smallest map with W < 32 (the projection's non-linear key items) that does."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import normwise

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
DEV = "cuda:0"


def _params(seed):
    from dagl_amd.synth import make_ce_params
    return {n: torch.from_numpy(a) for n, a in make_ce_params(seed, variant="default").items()}


def _features(seed, B, H, W):
    from dagl_amd.synth import make_features
    return torch.from_numpy(make_features(seed, B, 64, H, W))


def _module(params, mode, k):
    from dagl_amd.ce import CE
    ce = CE(in_channels=64)
    ce.load_state_dict(params, strict=True)
    ce.select_mode = mode
    if k:
        ce.select_k = k
    return ce.to(DEV).eval()


def _forward(ce, x, workspace=None, debug=True, **flags):
    """Module prologue + the (debug) forward of the C ABI (the projection runs inside the call): out, info, b1.  ``debug=False``: the
    plain entry point -- the debug one materialises the aggregated rows, which share their workspace region with the row sums."""
    from dagl_amd import ops
    with torch.no_grad():
        b1, b2, thr, bias = ce._prologue(x.to(DEV))
        out, info = ops.ce_forward(b1.contiguous(), b2.contiguous(), thr.contiguous(), bias.contiguous(), ce.fc1[0].weight,
                                   ce.fc1[0].bias, ce.fc2[0].weight, ce.fc2[0].bias, mode=ce.select_mode, k=ce.select_k,
                                   workspace=workspace, debug=debug, return_info=True, **flags)
    return out.cpu(), info, b1


@functools.lru_cache(maxsize=None)
def _oracle(w_seed, f_seed, H, W, k):
    from oracle.ce_oracle import ce_forward_oracle
    return ce_forward_oracle(_features(f_seed, 1, H, W), _params(w_seed), mode="topk", k=k, dtype=torch.float64).float()


# ---- 1. same bits as the tight threshold ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 8, 16])
@pytest.mark.parametrize("w_seed,f_seed", [(2024, 100), (41, 41)])
def test_pivot_threshold_gives_the_tight_thresholds_bits(w_seed, f_seed, k):
    from dagl_amd import ops
    ce = _module(_params(w_seed), "topk", k)
    x = _features(f_seed, 1, 128, 128)
    ws = ops.Workspace()
    out_p, info_p, _ = _forward(ce, x, workspace=ws, sampled_topk=True)
    idx, _ = ops.ce_pivot_debug(x.shape, "topk", k, ws, torch.device(DEV))          # (the call did take the pivot path: two distinct keys
    idx = idx[0].cpu().numpy()                                                        # of its own 64 in every block)
    assert (idx // 64 == np.arange(128 * 128 // 64)[:, None]).all() and (idx[:, 0] != idx[:, 1]).all()
    out_t, info_t, _ = _forward(ce, x, tight_topk=True)
    want = _oracle(w_seed, f_seed, 128, 128, k)
    print(f"[pivot] seeds ({w_seed}, {f_seed}) k={k}: pivot {normwise(out_p.numpy(), want.numpy()):.2e} tight "
          f"{normwise(out_t.numpy(), want.numpy()):.2e} of the fp64 oracle; redone {info_p['redone_queries']} / {info_t['redone_queries']}")
    assert torch.equal(out_p, out_t)
    assert normwise(out_p.numpy(), want.numpy()) <= TOL_OUT
    assert normwise(out_t.numpy(), want.numpy()) <= TOL_OUT
    assert info_p["redone_queries"] == 0 and info_t["redone_queries"] == 0
    assert info_p["path"] == 3 and info_t["path"] == 3


# ---- 2. pivot properties ---------------------------------------------------------------------------------------------------------

def _true_rowsums(ce, b1):
    """Row sums of X = relu(fc2(key patches of b1)) in fp64 on the host: [B, N]."""
    b1 = b1.detach().double().cpu()
    w, b = ce.fc2[0].weight.detach().double().cpu(), ce.fc2[0].bias.detach().double().cpu()
    B, _, H, W = b1.shape
    rows = F.unfold(F.pad(b1, (3, 3, 3, 3)), 7).transpose(1, 2)                       # [B, N, 784] (c, kh, kw)
    return F.relu(rows @ w.t() + b).sum(dim=2)


@pytest.mark.parametrize("B,H,W,k", [(1, 128, 128, 8), (1, 100, 92, 8), (1, 96, 24, 2), (2, 100, 92, 4)],
                         ids=["128x128", "100x92_partial_block", "96x24_nonlinear_items", "batch2"])
def test_pivots_are_the_two_heaviest_keys_of_their_blocks(B, H, W, k):
    from dagl_amd import ops
    from oracle.ce_oracle import ce_forward_oracle
    params = _params(2024)
    ce = _module(params, "topk", k)
    x = _features(100, B, H, W)
    ws = ops.Workspace()
    out, info, b1 = _forward(ce, x, workspace=ws, debug=False, sampled_topk=True)
    idx, rowsum = ops.ce_pivot_debug(x.shape, "topk", k, ws, torch.device(DEV))
    idx, rowsum = idx.cpu().numpy(), rowsum.cpu().double().numpy()
    N = H * W
    n_blk = (N + 63) // 64
    assert idx.shape == (B, n_blk, 2)
    true = _true_rowsums(ce, b1).numpy()
    print(f"[pivot] {B}x{H}x{W}: row sums {normwise(rowsum, true):.2e} of fp64")
    assert normwise(rowsum, true) <= 1e-5
    for b in range(B):
        flat = idx[b].reshape(-1)
        picked = flat[flat >= 0]
        assert len(np.unique(picked)) == len(picked)                                  # no key twice
        for v in range(n_blk):
            lo, hi = 64 * v, min(64 * v + 64, N)
            have = [int(p) for p in idx[b, v] if p >= 0]
            assert len(have) == min(2, hi - lo), (b, v, idx[b, v])
            assert all(lo <= p < hi for p in have), (b, v, idx[b, v])
            if hi - lo >= 2:
                second = np.sort(true[b, lo:hi])[-2]
                assert all(true[b, p] >= (1 - 1e-5) * second for p in have), (b, v, idx[b, v])
    want = ce_forward_oracle(x, params, mode="topk", k=k, dtype=torch.float64).float()
    assert normwise(out.numpy(), want.numpy()) <= TOL_OUT


def test_policy_word_takes_the_pivots_from_the_second_call_on():
    """No threshold flag (the module's "auto"): the first call of a shape keeps the tile sampling -- its overflow under the uniform
    sample decides the workspace's policy as before --, calls on the prepared workspace take the pivots where the tile sampling's
    stride is >= 4.  192 x 192: stride 4, 384-query blocks in the sampling launch.  Same bits as the tight threshold, which
    tests/test_gpu_block.py and the cases above tie to the oracle."""
    from dagl_amd import ops
    params = _params(2024)
    x = _features(100, 1, 192, 192)
    outs = {}
    for pol in ("auto", "full"):
        ce = _module(params, "topk", 8)
        ce.topk_threshold = pol
        with torch.no_grad():
            for _ in range(3):
                y = ce(x.to(DEV))
        outs[pol] = y.cpu()
        if pol == "auto":
            assert not ce.topk_policy_is_tight()
            idx, rowsum = ops.ce_pivot_debug(x.shape, "topk", 8, ce._ws, torch.device(DEV), sampled_topk=False)
            idx, rowsum = idx[0].cpu().numpy(), rowsum[0].cpu().numpy()
            n_blk = 192 * 192 // 64
            assert idx.shape == (n_blk, 2) and (idx // 64 == np.arange(n_blk)[:, None]).all() and (idx[:, 0] != idx[:, 1]).all()
            second = np.sort(rowsum.reshape(n_blk, 64), axis=1)[:, -2]
            assert (rowsum[idx] >= second[:, None]).all()
    assert torch.equal(outs["auto"], outs["full"])


# ---- 3. a valid but useless threshold -------------------------------------------------------------------------------------------

def test_heaviest_keys_that_no_query_sees_still_give_the_right_answer():
    """Two keys of every 64 are made by far the heaviest -- in feature columns where every query is zero, and zero in all others: the
    pivots score 0 against every query, theta collapses to 0, every key is a candidate, the slots overflow and the flagged groups
    take the exact redo pass.  Input channel 63 is a marker map that g copies into channel 15 of the key / query map; fc1 ignores
    that channel and leaves feature columns 98.. zero; fc2 turns the marker at a patch's centre into columns 98.. and (weight -50)
    switches columns ..97 off."""
    from dagl_amd import ops
    from oracle.ce_oracle import ce_forward_oracle
    H = W = 128
    k = 8
    params = {n: t.clone() for n, t in _params(2024).items()}
    g_w, g_b = params["g.weight"], params["g.bias"]
    g_w[:, 63] = 0.0; g_w[15] = 0.0; g_w[15, 63, 1, 1] = 1.0; g_b[15] = 0.0
    ch15 = slice(15 * 49, 16 * 49)
    centre = 15 * 49 + 24
    f1_w, f1_b = params["fc1.0.weight"], params["fc1.0.bias"]
    f1_w[:, ch15] = 0.0; f1_w[98:] = 0.0; f1_b[98:] = -1.0
    f2_w, f2_b = params["fc2.0.weight"], params["fc2.0.bias"]
    f2_w[:, ch15] = 0.0; f2_w[:98, centre] = -50.0
    f2_w[98:] = 0.0; f2_w[98:, centre] = 1.0; f2_b[98:] = 0.0
    x = _features(100, 1, H, W)
    rng = np.random.default_rng(7)
    marker = np.zeros(H * W, dtype=np.float32)
    marked = np.stack([64 * v + rng.choice(64, 2, replace=False) for v in range(H * W // 64)])      # [n_blk, 2]
    marker[marked.reshape(-1)] = 100.0
    x[0, 63] = torch.from_numpy(marker.reshape(H, W))
    ce = _module(params, "topk", k)
    ws = ops.Workspace()
    out, info, b1 = _forward(ce, x, workspace=ws, sampled_topk=True)
    idx, _ = ops.ce_pivot_debug(x.shape, "topk", k, ws, torch.device(DEV))
    assert np.array_equal(np.sort(idx[0].cpu().numpy(), axis=1), np.sort(marked, axis=1))           # the crafted keys ARE the pivots
    want = ce_forward_oracle(x, params, mode="topk", k=k, dtype=torch.float64).float()
    print(f"[pivot] useless pivots: {normwise(out.numpy(), want.numpy()):.2e} of the fp64 oracle, redone {info['redone_queries']}")
    assert info["redone_queries"] > 0
    assert normwise(out.numpy(), want.numpy()) <= TOL_OUT


# ---- 4. non-finite and degenerate maps --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_key_patch_is_nan_filled_and_reported(bad):
    """As tests/test_gpu_range.py expects of every top-k call: NaN-filled output, the workspace's range word reports it."""
    ce = _module(_params(2024), "topk", 8)
    ce.topk_threshold = "sparse"
    x = _features(100, 1, 128, 128)
    x[0, 3, 70, 41] = bad
    with torch.no_grad():
        out = ce(x.to(DEV))
        assert torch.isnan(out).all()
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            assert not ce.range_ok()


def test_all_zero_map():
    """No bias anywhere, x = 0: every feature and every score is 0, theta = 0, all keys tie and the lower key index wins."""
    from oracle.ce_oracle import ce_forward_oracle
    params = {n: t.clone() for n, t in _params(2024).items()}
    for n in params:
        if n.endswith("bias"):
            params[n].zero_()
    x = torch.zeros(1, 64, 128, 128)
    ce = _module(params, "topk", 8)
    out, info, _ = _forward(ce, x, sampled_topk=True)
    want = ce_forward_oracle(x, params, mode="topk", k=8, dtype=torch.float64).float()
    assert torch.isfinite(out).all()
    assert normwise(out.numpy(), want.numpy()) <= TOL_OUT


# ---- 5. scope guard ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,k,variant", [("topk", 50, "default"), ("adaptive", 0, "sparse")])
def test_outside_the_rule_nothing_changes(mode, k, variant):
    from dagl_amd import ops
    from dagl_amd._lib import DaglError, ERR_UNSUPPORTED
    from dagl_amd.synth import make_ce_params
    from oracle.ce_oracle import ce_forward_oracle
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(51, variant=variant, sparse_gain=2.6).items()}
    ce = _module(params, mode, k)
    x = _features(51, 1, 128, 128)
    ws = ops.Workspace()
    flags = {"sampled_topk": True} if mode != "adaptive" else {}
    out, info, _ = _forward(ce, x, workspace=ws, **flags)
    assert info["path"] == 3
    with pytest.raises(DaglError) as e:
        ops.ce_pivot_debug(x.shape, mode, k, ws, torch.device(DEV))
    assert e.value.code == ERR_UNSUPPORTED
    want = ce_forward_oracle(x, params, mode=mode, k=k or None, dtype=torch.float64).float()
    assert normwise(out.numpy(), want.numpy()) <= TOL_OUT
