"""``CE.graph`` / ``CE.degrees`` (dagl_ce_graph_count / _fill, csrc/graph.hip) against the fp64 oracle's ``S``, ``thr``, ``bias`` and
``mask_b``: CSR structure, the edge set outside a rounding band, weights and scores against the reference in its own precision,
the block's output rebuilt from the exported graph, exact ties, refusals.

The band.  A pair (i, j) is THRESHOLD-AMBIGUOUS when |S - mu thr + bias| < tau (|S| + |mu thr| + |bias|) (mu = the fp64 row mean)
and RANK-AMBIGUOUS (fixed-k modes, k < N) when the k-th and (k+1)-th best rankable scores of its row differ by less than tau
relative and its score lies within tau relative of them.  tau = 2e-5: all products are of non-negative features, so an fp32 dot
product over 196 terms is within 196 * 2^-24 = 1.2e-5 relative in any order; the row mean gets the rest.  Outside both bands the
membership must be the oracle's; inside a pair may go either way -- but at most 5e-4 of all pairs and 10 % of the rows may be
ambiguous at all, so that the band cannot hide a failure."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import normwise

pytestmark = pytest.mark.gpu

TAU = 2e-5
SHAPES = [(2, 24, 20),      # N = 480, not a multiple of 256; L = 30; offsets cross an image boundary
          (1, 33, 70),      # odd sizes
          (2, 45, 45),      # unscreened size; degrees past 256 and 1024
          (1, 64, 64)]      # screened size; N = 4096, several block strides per row
# (variant, sparse_gain, mode, k)
CASES = [("default", 2.0, "adaptive", 0), ("sparse", 1.65, "adaptive", 0), ("sparse", 1.2, "adaptive", 0),
         ("allpass", 2.0, "adaptive", 0), ("nonepass", 2.0, "adaptive", 0),
         ("default", 2.0, "topk", 8), ("default", 2.0, "topk", 64), ("default", 2.0, "topk", 100), ("default", 2.0, "topk", 5000),
         ("sparse", 1.2, "adaptive_topk", 16), ("sparse", 1.2, "adaptive_topk", 100)]
SEEDS = (11, 12, 13)


def _seed(shape, case):
    return SEEDS[(SHAPES.index(shape) + CASES.index(case)) % 3]


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _inputs(seed, shape, variant, gain, in_channels=64):
    from dagl_amd.synth import make_ce_params, make_features
    B, H, W = shape
    prm = {n: torch.from_numpy(a) for n, a in make_ce_params(seed, in_channels=in_channels, variant=variant, sparse_gain=gain).items()}
    return torch.from_numpy(make_features(seed, B, in_channels, H, W)), prm


def _dense_a(st, mode, scale=10.0):
    """A = softmax(scale S m) mask_b of ``_graph_core`` from an oracle's stages, in their precision: [B, L, N]."""
    S, mb = st["S"], st["mask_b"]
    if mode == "topk":
        m = mb
    else:
        m = F.relu(S - S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2) + st["bias"].unsqueeze(2)) * mb
    return F.softmax(S * m * scale, dim=2) * mb


@functools.lru_cache(maxsize=None)
def _oracle(seed, shape, variant, gain, mode, k, dtype=torch.float64, in_channels=64, scale=10.0):
    """The oracle's stages + A, computed once per case and shared (read-only) by the tests."""
    from oracle.ce_oracle import ce_forward_oracle
    x, prm = _inputs(seed, shape, variant, gain, in_channels)
    torch.set_num_threads(16)
    with torch.no_grad():
        out, st = ce_forward_oracle(x, prm, mode=mode, k=k if mode != "adaptive" else None, dtype=dtype, stages=True,
                                    softmax_scale=scale)
        st = {n: st[n] for n in ("S", "thr", "bias", "mask_b", "b2", "cnt")}
        st["A"] = _dense_a(st, mode, scale)
    return st


def _module(seed, shape, variant, gain, mode, k, in_channels=64, half=False, scale=10):
    from dagl_amd.ce import CE
    x, prm = _inputs(seed, shape, variant, gain, in_channels)
    ce = CE(in_channels=in_channels, softmax_scale=scale)
    ce.load_state_dict(prm, strict=True)
    ce.select_mode = mode
    if mode != "adaptive":
        ce.select_k = k
    ce = ce.to("cuda:0").eval()
    x = x.to("cuda:0")
    if half:
        ce, x = ce.half(), x.half()
    return ce, x


def ambiguity(st, mode, k):
    """(threshold-ambiguous, rank-ambiguous) [B, L, N] bool from the fp64 oracle's stages."""
    S = st["S"]
    N = S.shape[2]
    thr_amb = torch.zeros_like(S, dtype=torch.bool)
    if mode != "topk":
        mt = S.mean(dim=2, keepdim=True) * st["thr"].unsqueeze(2)
        bs = st["bias"].unsqueeze(2).expand_as(S)
        thr_amb = (S - mt + bs).abs() < TAU * (S.abs() + mt.abs() + bs.abs())
    rank_amb = torch.zeros_like(S, dtype=torch.bool)
    if mode != "adaptive" and k < N:
        rankable = torch.ones_like(S, dtype=torch.bool)
        if mode == "adaptive_topk":
            rankable = F.relu(S - mt + bs) != 0
        top = torch.where(rankable, S, torch.full_like(S, -1.0)).topk(k + 1, dim=2).values
        sk, sk1 = top[..., k - 1:k], top[..., k:k + 1]                 # (-1: the row has fewer rankable keys -- nothing to rank)
        close = (sk1 >= 0) & ((sk - sk1) < TAU * sk)
        rank_amb = close & (S >= sk1 * (1 - TAU)) & (S <= sk * (1 + TAU)) & (rankable | thr_amb)
    return thr_amb, rank_amb


def membership(g):
    """[B, L, N] bool from a PatchGraph (on the CPU)."""
    deg = g.degrees().reshape(-1)
    rows = torch.repeat_interleave(torch.arange(g.B * g.L), deg)
    m = torch.zeros(g.B * g.L, g.N, dtype=torch.bool)
    m[rows, g.key.long()] = True
    return m.view(g.B, g.L, g.N), rows


def check_structure(g, mode, k, variant):
    off, key = g.row_off, g.key.long()
    assert off.dtype == torch.int64 and g.key.dtype == torch.int32 and g.weight.dtype == torch.float32
    assert off.numel() == g.B * g.L + 1 and int(off[0]) == 0 and bool((off[1:] >= off[:-1]).all()) and int(off[-1]) == key.numel()
    assert key.numel() == 0 or (int(key.min()) >= 0 and int(key.max()) < g.N)
    rows = torch.repeat_interleave(torch.arange(g.B * g.L), g.degrees().reshape(-1))
    same_row = rows[1:] == rows[:-1]
    assert bool((key[1:] > key[:-1])[same_row].all()), "keys must ascend strictly inside a row"
    if mode == "topk":
        assert bool((g.degrees() == min(k, g.N)).all())
    if variant == "nonepass":
        assert key.numel() == 0
    if (variant == "allpass" and mode == "adaptive") or (mode == "topk" and k >= g.N):
        assert bool((g.degrees() == g.N).all()) and torch.equal(key, torch.arange(g.N).repeat(g.B * g.L))


def check_edges(g, st, mode, k):
    """Membership against the oracle outside the band; returns (lib membership, rows of its edges, rows holding a rank-ambiguous pair)."""
    mem, rows = membership(g)
    thr_amb, rank_amb = ambiguity(st, mode, k)
    amb = thr_amb | rank_amb
    want = st["mask_b"] != 0
    wrong = (mem != want) & ~amb
    share, rank_rows = float(amb.double().mean()), rank_amb.any(dim=2)
    print(f"[graph] edges {g.n_edges}, degree mean {float(g.degrees().double().mean()):.1f} max {int(g.degrees().max())}; ambiguous pairs "
          f"{int(amb.sum())} ({share:.1e} of all), of them on the other side {int(((mem != want) & amb).sum())}; rows with a rank-ambiguous "
          f"pair {int(rank_rows.sum())} of {rank_rows.numel()}; wrong outside the band {int(wrong.sum())}")
    assert share <= 5e-4, "the band must not hide a failure: too many ambiguous pairs"
    assert float(rank_rows.double().mean()) <= 0.10, "the band must not hide a failure: too many rows with a rank-ambiguous pair"
    assert int(wrong.sum()) == 0
    return mem, rows, rank_rows


def check_values(g, mem, rows, rank_rows, st64, st32, mode, what):
    """Weights and scores over the edges both sides have, against the reference in its own precision (the bound of test_gpu_trunk)."""
    keep_row = ~rank_rows if mode != "adaptive" else torch.ones_like(rank_rows)
    want = st64["mask_b"] != 0
    common_lib = want.view(-1, g.N)[rows, g.key.long()] & keep_row.view(-1)[rows]            # per lib edge
    common_32 = (st32["mask_b"] != 0) & want & keep_row.unsqueeze(2)
    if int(common_lib.sum()) == 0 or int(common_32.sum()) == 0:          # (an empty graph: check_edges has compared the sets)
        print(f"[graph] {what}: no common edges to compare values on")
        return
    for name, lib, ref in (("weight", g.weight, "A"), ("score", g.score, "S")):
        r64 = st64[ref].view(-1, g.N)
        e_lib = normwise(lib[common_lib].numpy(), r64[rows, g.key.long()][common_lib].numpy())
        e_32 = normwise(st32[ref][common_32].numpy(), st64[ref][common_32].numpy())
        print(f"[graph] {what} {name}: e_lib {e_lib:.2e}, e_ref32 {e_32:.2e}, ratio {e_lib / max(e_32, 1e-30):.2f}")
        assert e_lib <= 3.0 * e_32 + 1e-6, (what, name, e_lib, e_32)


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


def _fold(agg, cnt, H, W):
    """[B, L, 784] aggregated rows (c, kh, kw) -> [B, 16, H, W], dagl.py:265-272."""
    z = F.fold(agg.transpose(1, 2), (H, W), (7, 7), padding=3, stride=4)
    return z / cnt


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


def _same_forward_after(ce, x, refused):
    from dagl_amd import DaglError
    with torch.no_grad():
        before = ce(x).clone()
    with pytest.raises(DaglError) as err:
        refused()
    with torch.no_grad():
        assert torch.equal(ce(x), before)
    return str(err.value)


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
