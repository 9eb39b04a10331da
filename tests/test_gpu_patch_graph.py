"""``CE.graph`` / ``CE.degrees`` (dagl_ce_graph_count / _fill, csrc/graph.hip) against the fp64 oracle's ``S``, ``thr``, ``bias`` and
``mask_b``: CSR structure, the edge set outside a rounding band, weights and scores against the reference in its own precision,
the block's output rebuilt from the exported graph, exact ties, refusals.

The band.  A pair (i, j) is THRESHOLD-AMBIGUOUS when |S - mu thr + bias| < tau (|S| + |mu thr| + |bias|) (mu = the fp64 row mean)
and RANK-AMBIGUOUS (fixed-k modes, k < N) when the k-th and (k+1)-th best rankable scores of its row differ by less than tau
relative and its score lies within tau relative of them.  tau = 2e-5: all products are of non-negative features, so an fp32 dot
product over 196 terms is within 196 * 2^-24 = 1.2e-5 relative in any order; the row mean gets the rest.  Outside both bands the
membership must be the oracle's; inside a pair may go either way -- but at most 5e-4 of all pairs and 10 % of the rows may be
ambiguous at all, so that the band cannot hide a failure."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import (CASES, SHAPES, _dense_a, _fold, _id, _inputs, _module, _oracle, _same_forward_after, _seed, ambiguity,
                                  check_edges, check_structure, check_values, membership)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_graph_against_the_fp64_oracle(shape, case):
    """Structure, edge set outside the rounding band, weights and scores (checks 1-3)."""
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    ce, x = _module(seed, shape, variant, gain, mode, k)
    g_dev = ce.graph(x, scores=True)
    again = ce.graph(x, scores=True)
    for a, b in ((g_dev.row_off, again.row_off), (g_dev.key, again.key), (g_dev.weight, again.weight), (g_dev.score, again.score)):
        assert torch.equal(a, b)
    assert torch.equal(g_dev.degrees(), ce.degrees(x))
    assert ce.graph(x).score is None
    g = g_dev.cpu()
    check_structure(g, mode, k, variant)
    st64 = _oracle(seed, shape, variant, gain, mode, k)
    mem, rows, rank_rows = check_edges(g, st64, mode, k)
    st32 = _oracle(seed, shape, variant, gain, mode, k, torch.float32)
    check_values(g, mem, rows, rank_rows, st64, st32, mode, f"seed {seed} {shape} {case}")


@pytest.mark.parametrize("kind", ["in_channels_32", "half_module"])
def test_other_widths_and_precisions(kind):
    """A 32-channel module (prologue as unfold + GEMM), and a .half() module on the fp32 copies of its weights."""
    shape, case = (2, 24, 20), ("sparse", 1.2, "adaptive", 0)
    variant, gain, mode, k = case
    cin, half = (32, False) if kind == "in_channels_32" else (64, True)
    ce, x = _module(12, shape, variant, gain, mode, k, in_channels=cin, half=half)
    g = ce.graph(x, scores=True).cpu()
    assert torch.equal(g.degrees(), ce.degrees(x).cpu())
    check_structure(g, mode, k, variant)
    # (the half module sees the half-rounded input too: the oracle gets the same values)
    if half:
        x0, prm = _inputs(12, shape, variant, gain, cin)
        from oracle.ce_oracle import ce_forward_oracle
        xs, ps = x0.half().float(), {n: t.half().float() for n, t in prm.items()}
        sts = []
        for dt in (torch.float64, torch.float32):
            with torch.no_grad():
                _, st = ce_forward_oracle(xs, ps, mode=mode, dtype=dt, stages=True)
            st["A"] = _dense_a(st, mode)
            sts.append(st)
        st64, st32 = sts
    else:
        st64 = _oracle(12, shape, variant, gain, mode, k, torch.float64, cin)
        st32 = _oracle(12, shape, variant, gain, mode, k, torch.float32, cin)
    mem, rows, rank_rows = check_edges(g, st64, mode, k)
    check_values(g, mem, rows, rank_rows, st64, st32, mode, kind)


@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=_id)
def test_softmax_scale_other_than_10(case):
    """``softmax_scale = 40`` (the module scales fc1 and the bias head, here by exact powers of two: 2 in the adaptive mode, 4 in the
    fixed-k mode): the same edges, weights of ``softmax(40 S m)``, and ``score`` is S itself again."""
    shape = (2, 24, 20)
    variant, gain, mode, k = case
    ce, x = _module(12, shape, variant, gain, mode, k, scale=40)
    g = ce.graph(x, scores=True).cpu()
    check_structure(g, mode, k, variant)
    st64 = _oracle(12, shape, variant, gain, mode, k, torch.float64, 64, 40.0)
    st32 = _oracle(12, shape, variant, gain, mode, k, torch.float32, 64, 40.0)
    mem, rows, rank_rows = check_edges(g, st64, mode, k)
    check_values(g, mem, rows, rank_rows, st64, st32, mode, f"softmax_scale 40 {case}")


@pytest.mark.parametrize("case", [CASES[2], CASES[7], CASES[9]], ids=_id)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=_id)
def test_chunk_height_does_not_change_the_graph(shape, case):
    """rows_per_chunk 0 (one chunk), 16 and 7 (chunks that cross image boundaries unevenly): the same arrays, bit for bit."""
    variant, gain, mode, k = case
    ce, x = _module(_seed(shape, case), shape, variant, gain, mode, k)
    ref = ce.graph(x, scores=True)
    for rpc in (16, 7):
        g = ce.graph(x, scores=True, rows_per_chunk=rpc)
        for name in ("row_off", "key", "weight", "score"):
            assert torch.equal(getattr(g, name), getattr(ref, name)), (rpc, name)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5], CASES[7], CASES[9]], ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_graph_reproduces_the_block(shape, case):
    """A_csr @ (the oracle's fp64 value rows), folded and divided by the overlap count, is what ``forward`` returns -- the default
    scan and scan = "exact" -- within the bound test_gpu_fuzz applies to that forward against the oracle."""
    from oracle.ce_oracle import patch_rows
    variant, gain, mode, k = case
    seed = _seed(shape, case)
    B, H, W = shape
    ce, x = _module(seed, shape, variant, gain, mode, k)
    g = ce.graph(x).cpu()
    st = _oracle(seed, shape, variant, gain, mode, k)
    v_rows = patch_rows(st["b2"], 7, 1)                               # [B, N, 784] fp64
    agg = torch.stack([g.to_dense(b).double() @ v_rows[b] for b in range(B)])
    want = _fold(agg, st["cnt"], H, W)
    gap = 1.0
    if mode != "adaptive" and k < H * W:
        S = st["S"]
        if mode == "adaptive_topk":                  # only keys that pass the adaptive test rank (rows with fewer than k + 1 of them: gap 1)
            passing = F.relu(S - S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2) + st["bias"].unsqueeze(2)) != 0
            S = torch.where(passing, S, torch.full_like(S, -1.0))
        top = S.topk(k + 1, dim=2).values
        ok = top[..., k] > 0
        rel = (top[..., k - 1] - top[..., k]) / top[..., k - 1].clamp(min=1e-30)
        gap = float(torch.where(ok, rel, torch.ones_like(rel)).min())
    bound = 1e-4 if gap >= 1e-6 else 1e-3
    for scan in ("screened", "exact"):
        ce.scan = scan
        ce.invalidate_packed()
        with torch.no_grad():
            out = ce(x).double().cpu()
        err = normwise(out.numpy(), want.numpy())
        print(f"[graph] seed {seed} {shape} {case} scan={scan}: forward vs the folded graph {err:.2e} (bound {bound:.0e}, gap {gap:.1e})")
        assert err <= bound, (scan, err)


def test_exact_ties_go_to_the_lower_key():
    """A map of identical pixels: interior patches are bitwise equal, whole runs of keys tie at the k-th place.  On every row whose
    rank-ambiguous pairs are all exact fp64 ties, the exported keys are the oracle's ``_k_best`` set (the lower key index wins)."""
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params
    from oracle.ce_oracle import ce_forward_oracle
    B, H, W, k = 1, 24, 20, 8
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(11, variant="default").items()}
    col = torch.from_numpy(np.random.default_rng(11).standard_normal((1, 64, 1, 1)).astype(np.float32))
    x = col.expand(B, 64, H, W).contiguous()
    ce = CE(in_channels=64)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode, ce.select_k = "topk", k
    ce = ce.to("cuda:0").eval()
    g = ce.graph(x.to("cuda:0")).cpu()
    check_structure(g, "topk", k, "default")
    with torch.no_grad():
        _, st = ce_forward_oracle(x, prm, mode="topk", k=k, dtype=torch.float64, stages=True)
    _, rank_amb = ambiguity(st, "topk", k)
    mem, _ = membership(g)
    want = st["mask_b"] != 0
    checked = tied = 0
    for i in range(g.L):
        band = st["S"][0, i][rank_amb[0, i]]
        if band.numel() and float(band.max()) != float(band.min()):
            # near ties that are not exact: either side of the band is legitimate, the rest of the row is not
            assert torch.equal(mem[0, i][~rank_amb[0, i]], want[0, i][~rank_amb[0, i]]), i
            continue
        assert torch.equal(mem[0, i], want[0, i]), (i, mem[0, i].nonzero().flatten().tolist(), want[0, i].nonzero().flatten().tolist())
        checked += 1
        tied += int(band.numel() > k)
    print(f"[graph] ties: {checked} of {g.L} rows compared key by key, {tied} of them with more than k keys tied at the k-th place")
    assert tied > 0, "the case must hold rows with an exact tie at the k-th place"


def test_refusals_leave_the_module_alone():
    shape, case = (1, 64, 64), CASES[5]
    variant, gain, mode, k = case
    ce, x = _module(11, shape, variant, gain, mode, k)
    # more edges than the caller allows: L * k = 256 * 8
    assert "2048 edges" in _same_forward_after(ce, x, lambda: ce.graph(x, max_edges=2047))
    assert ce.graph(x, max_edges=2048).n_edges == 2048
    # under stream capture the edge count cannot be read
    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ce.graph(x)
    assert "captur" in _same_forward_after(ce, x, captured)
    def captured_degrees():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ce.degrees(x)
    assert "captur" in _same_forward_after(ce, x, captured_degrees)
    torch.cuda.synchronize()
    assert ce.graph(x).n_edges == 2048                # and the export still works afterwards


def test_refusal_of_a_generic_geometry():
    from dagl_amd.ce import CE
    torch.manual_seed(5)
    ce = CE(ksize=5, stride_1=2, stride_2=1, inter_channels=16, in_channels=64).to("cuda:0").eval()
    x = torch.randn(1, 64, 20, 24, device="cuda:0")
    for call in (lambda: ce.graph(x), lambda: ce.degrees(x)):
        assert "scope" in _same_forward_after(ce, x, call)


def test_fill_never_writes_past_a_capacity_below_the_devices_total():
    """The C pair called by hand with a caller that understates the edge count: the host cannot see that, the kernels compare the
    capacity with the total the scan left on the device and write NOTHING -- not a partial graph, not a byte past the arrays."""
    import ctypes as C
    from dagl_amd import _lib, ops
    shape, (variant, gain, mode, k) = (2, 24, 20), CASES[2]
    ce, x = _module(13, shape, variant, gain, mode, k)
    want = ce.graph(x)
    B, H, W = shape
    lib = _lib.load()
    p = ce._params_f32()
    with torch.no_grad():
        b1p, _, thr, bias = ops.ce_prologue(x, p["g.weight"], p["g.bias"], p["theta.weight"], p["theta.bias"], p["thr_conv.weight"],
                                            p["thr_conv.bias"], p["bias_conv.weight"], p["bias_conv.bias"])
        b1 = b1p[:, 3:3 + H, 3:3 + W, :].permute(0, 3, 1, 2).contiguous()
    need = lib.dagl_ce_graph_workspace_bytes(B, H, W, 0, 0, 0)
    ws = torch.empty(need + 256, device=x.device, dtype=torch.uint8)
    base = (ws.data_ptr() + 255) // 256 * 256
    row_off = torch.empty(B * want.L + 1, device=x.device, dtype=torch.int64)
    info = _lib.CeInfo()
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.dagl_ce_graph_count(stream, B, H, W, b1.data_ptr(), thr.data_ptr(), bias.data_ptr(), p["fc1.0.weight"].data_ptr(),
                                 p["fc1.0.bias"].data_ptr(), p["fc2.0.weight"].data_ptr(), p["fc2.0.bias"].data_ptr(), 0, 0, 0,
                                 row_off.data_ptr(), base, need, C.byref(info))
    assert rc == 0 and info.required_bytes == need and info.path == 8
    assert torch.equal(row_off, want.row_off)
    E = want.n_edges

    def fill(claimed, key, weight):
        return lib.dagl_ce_graph_fill(stream, B, H, W, 0, 0, 0, row_off.data_ptr(), key.data_ptr(), weight.data_ptr(), None,
                                      claimed, claimed, base, need)
    key = torch.full((E,), -7, device=x.device, dtype=torch.int32)
    weight = torch.full((E,), -7.0, device=x.device)
    assert fill(E - 1, key, weight) == 0              # (the arrays hold E entries: nothing can go wrong even if it did write)
    torch.cuda.synchronize()
    assert bool((key == -7).all()) and bool((weight == -7.0).all())
    assert fill(E, key, weight) == 0
    assert torch.equal(key, want.key) and torch.equal(weight, want.weight)
