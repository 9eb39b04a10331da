"""``ops.graph_refresh`` (dagl_graph_refresh, csrc/graph_refresh.hip) on a crafted graph: candidates, scores, selection, weights.

The candidate sets and the selection rule come from tests/graph_refresh_reference.py (checked against brute force on the CPU); scores and
weights are held against torch on the CPU in fp64 under the project's rule ``e <= 3 e_ref32 + 1e-6`` (``_check`` of
test_gpu_graph_attend.py).  The selection itself is checked EXACTLY: it is the CPU rule applied, in fp32, to the scores the keep-all call
returned -- a score does not depend on k, tau, the flags or the rest of the row."""
import ctypes as C
import functools

import pytest
import torch

from tests.graph_reference import _LEVELS, _check, _edge_reference, _geom, _rows_of
from tests.graph_refresh_reference import candidate_mask, csr_of, mask_of, select_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
SHAPES = [(2, 24, 20), (1, 33, 70)]
MAX_ROW = 12                                  # the declared max_row_edges: 108 candidates at radius 1 (a wavefront per row), 300 at 2 (a block)
R_FAIL = 9                                    # the row whose candidates all fail tau


def _id(v):
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _crafted(shape, seed=5):
    """(row_off, key) on the CPU.  Rows: 0 empty; 1 the four corners; 2 one key on each border; 3 two adjacent keys; 4 a key three times;
    5 unsorted keys; 6 a key of -1, one of N and a valid one; 7 exactly MAX_ROW distinct keys; 8 a single key; 9 a row whose candidates
    all fail tau; L - 1 (the last row of image 0) five keys, followed -- in a batch of two -- by an empty first row of image 1; every
    other row 8 keys drawn with replacement."""
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randint(0, N, (8,), generator=gen).tolist() for _ in range(B * L)]
    rows[0] = []
    rows[1] = [0, W - 1, (H - 1) * W, N - 1]
    rows[2] = [W // 2, (H - 1) * W + W // 2, (H // 2) * W, (H // 2) * W + W - 1]
    rows[3] = [5 * W + 5, 5 * W + 6]
    rows[4] = [7 * W + 7] * 3
    rows[5] = [N - 3, 10, 9 * W + 4, 2 * W + 15]
    rows[6] = [-1, N, 3 * W + 3]
    rows[7] = torch.randperm(N, generator=gen)[:MAX_ROW].tolist()
    rows[8] = [11 * W + 9]
    rows[R_FAIL] = [6 * W + 2, 15 * W + 11]
    rows[L - 1] = torch.randint(0, N, (5,), generator=gen).tolist()
    if B > 1:
        rows[L] = []
    row_off = torch.tensor([0] + [len(r) for r in rows], dtype=torch.int64).cumsum(0)
    return row_off, torch.tensor([k for r in rows for k in r], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _features(shape, seed=7):
    """(wq [B,L,196], x [B,N,196], tau [B*L]) fp32 on the CPU, banded as graph_reference._level_features builds them: keys at five levels of
    a common random direction plus a tenth of noise, every third key row a BITWISE copy of its left neighbour (exact ties among the
    candidates of a window), each query row scaled so that its largest candidate score (radius 2) is 1.6; tau_r midway in the widest gap
    of the middle half of the row's sorted distinct candidate scores; row R_FAIL: above every score."""
    row_off, key = _crafted(shape)
    B, H, W, L, N = _geom(shape)
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(196, generator=gen, dtype=torch.float64)
    level = _LEVELS[torch.randint(0, 5, (B, N), generator=gen)]
    x = level.unsqueeze(2) * (base + 0.1 * torch.rand(B, N, 196, generator=gen, dtype=torch.float64))
    twin = torch.arange(N)
    twin = twin[(twin % 3 == 1) & (twin % W != 0)]
    x[:, twin] = x[:, twin - 1]
    wq = torch.rand(B, L, 196, generator=gen, dtype=torch.float64)
    cand = candidate_mask(row_off, key, H, W, 2)
    S = torch.bmm(wq, x.transpose(1, 2)).reshape(B * L, N)
    smax = torch.where(cand, S, torch.zeros_like(S)).amax(dim=1)
    wq = wq * torch.where(smax > 0, 1.6 / smax.clamp(min=1e-30), torch.ones_like(smax)).view(B, L, 1)
    wq, x = wq.float(), x.float()
    S = torch.bmm(wq.double(), x.double().transpose(1, 2)).reshape(B * L, N)
    tau = torch.zeros(B * L, dtype=torch.float64)
    for r in range(B * L):
        s = torch.unique(S[r][cand[r]])
        if s.numel() == 1:
            tau[r] = s[0] / 2
        elif s.numel() >= 2:
            gaps = s[1:] - s[:-1]
            lo = gaps.numel() // 4
            hi = max(lo + 1, (3 * gaps.numel() + 3) // 4)
            j = lo + int(gaps[lo:hi].argmax())
            tau[r] = (s[j] + s[j + 1]) / 2
    tau[R_FAIL] = 100.0
    return wq, x, tau.float()


@functools.lru_cache(maxsize=None)
def _dense_scores(shape, dtype):
    wq, x, _ = _features(shape)
    B, H, W, L, N = _geom(shape)
    torch.set_num_threads(16)
    return torch.bmm(wq.to(dtype), x.to(dtype).transpose(1, 2)).reshape(B * L, N)


def _device_args(shape):
    row_off, key = _crafted(shape)
    wq, x, tau = _features(shape)
    return [t.to(DEV) for t in (wq, x, row_off, key)], tau.to(DEV)


def _cpu(out):
    return {n: t.cpu() for n, t in out.items()}


def _same(a, b):
    return all(torch.equal(a[n], b[n]) for n in ("row_off", "key", "weight", "score"))


def _structure_ok(out, n_rows, N):
    off, key = out["row_off"], out["key"].long()
    assert off.dtype == torch.int64 and out["key"].dtype == torch.int32 and out["weight"].dtype == out["score"].dtype == torch.float32
    assert off.numel() == n_rows + 1 and int(off[0]) == 0 and bool((off[1:] >= off[:-1]).all())
    assert int(off[-1]) == key.numel() == out["weight"].numel() == out["score"].numel()
    assert key.numel() == 0 or (int(key.min()) >= 0 and int(key.max()) < N)
    rows = _rows_of(off)
    assert bool((key[1:] > key[:-1])[rows[1:] == rows[:-1]].all()), "keys must ascend strictly inside a row"


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_kernel_on_a_crafted_graph(shape, radius):
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    row_off, key = _crafted(shape)
    wq, x, tau = _features(shape)
    assert int((row_off[1:] - row_off[:-1]).max()) == int(row_off[8] - row_off[7]) == MAX_ROW
    args, tau_dev = _device_args(shape)
    S64, S32 = _dense_scores(shape, torch.float64), _dense_scores(shape, torch.float32)
    cand = candidate_mask(row_off, key, H, W, radius)
    # the case is what it claims to be: clipped windows, overlaps, no margin in doubt
    if radius == 1:
        assert int(cand[1].sum()) == 16 and int(cand[2].sum()) == 24 and int(cand[3].sum()) == 12 and int(cand[4].sum()) == 9
        assert int(cand[6].sum()) == 9 and int(cand[0].sum()) == 0
    if radius == 0:
        assert int(cand[4].sum()) == 1 and int(cand[6].sum()) == 1 and int(cand[7].sum()) == MAX_ROW
    margin = ((S64 - tau.double().view(-1, 1)).abs() / S64.abs())[candidate_mask(row_off, key, H, W, 2)].min()
    assert float(margin) >= 1e-3, float(margin)

    # (a) keep_all: the candidate sets, exactly; the scores against fp64
    kept = {}
    for with_tau in (False, True):
        t = tau_dev if with_tau else None
        dil = _cpu(ops.graph_refresh(*args, radius=radius, tau=t, keep_all=True, max_row_edges=MAX_ROW, scale=SCALE, hw=(H, W)))
        _structure_ok(dil, B * L, N)
        want_off, want_key = csr_of(cand)
        assert torch.equal(dil["row_off"], want_off) and torch.equal(dil["key"], want_key)
        kept[with_tau] = dil
    assert torch.equal(kept[False]["score"], kept[True]["score"])                # a score does not depend on tau
    dil = kept[False]
    rows = _rows_of(dil["row_off"])
    _check(f"refresh score {shape} radius {radius}", dil["score"], S64[rows, dil["key"].long()], S32[rows, dil["key"].long()])
    # keep_all with k set: k is not looked at
    assert _same(_cpu(ops.graph_refresh(*args, radius=radius, keep_all=True, k=1, max_row_edges=MAX_ROW, hw=(H, W))), dil)
    # the scores of the call, as a dense matrix for the CPU selection (off the candidates: never looked at)
    S_gpu = torch.zeros(B * L, N).index_put((rows, dil["key"].long()), dil["score"])

    # exact ties at the k-th place occur (bitwise copies among the key rows)
    tie_rows = 0
    for r in range(B * L):
        s = S_gpu[r][cand[r]].sort(descending=True).values
        tie_rows += int(any(kk < s.numel() and float(s[kk - 1]) == float(s[kk]) for kk in (1, 8, 64)))
    print(f"[graph_refresh] {shape} radius {radius}: rows with an exact tie at a k-th place: {tie_rows}")
    if radius > 0:
        assert tie_rows >= 1

    # (b) - (e)
    for with_tau in (False, True):
        t_cpu, t_dev = (tau, tau_dev) if with_tau else (None, None)
        for k in (0, 1, 8, 64):
            want = select_mask(cand, S_gpu, t_cpu, k)
            want_off, want_key = csr_of(want)
            for normalize in ("reference", "edges"):
                kw = dict(radius=radius, tau=t_dev, k=k, scale=SCALE, normalize=normalize, max_row_edges=MAX_ROW, hw=(H, W))
                dev = ops.graph_refresh(*args, **kw)
                out = _cpu(dev)
                what = f"{shape} radius {radius} {'tau' if with_tau else 'notau'} k {k} {normalize}"
                _structure_ok(out, B * L, N)
                # (b) the structure: exactly the CPU selection on the scores of (a); the kept scores are (a)'s bits
                assert torch.equal(out["row_off"], want_off) and torch.equal(out["key"], want_key), what
                orow = _rows_of(out["row_off"])
                assert torch.equal(out["score"], S_gpu[orow, out["key"].long()]), what
                if k > 0:
                    assert int((out["row_off"][1:] - out["row_off"][:-1]).max()) <= k
                if with_tau:
                    assert int(out["row_off"][R_FAIL + 1] - out["row_off"][R_FAIL]) == 0
                # (c) the weights: _edge_reference on the OUTPUT structure
                if out["key"].numel():
                    with torch.no_grad():
                        w64, _, _ = _edge_reference(wq.double(), x.double(), out["row_off"], out["key"], tau.double() if with_tau else None,
                                                    normalize, shape, SCALE)
                        w32, _, _ = _edge_reference(wq, x, out["row_off"], out["key"], t_cpu, normalize, shape, SCALE)
                    _check(f"refresh weight {what}", out["weight"], w64, w32)
                    assert torch.equal(out["weight"] != 0, w64 != 0), what
                # (d) the scores are ops.graph_attend's on the output structure, bit for bit
                _, s_att = ops.graph_attend(args[0], args[1], dev["row_off"], dev["key"], tau=t_dev, scale=SCALE, normalize=normalize,
                                            hw=(H, W))
                assert torch.equal(s_att, dev["score"]), what
            # (e) the same bits on a second call, through a Workspace, with the degree read by the call, a block per row
            ws = ops.Workspace()
            last = dict(kw)
            for again in (dict(last), dict(last, workspace=ws), dict(last, workspace=ws), dict(last, max_row_edges=None),
                          dict(last, block_rows=True)):
                assert _same(_cpu(ops.graph_refresh(*args, **again)), out), (what, sorted(again))
    # keep_all with tau: edges with margin 0 weigh 0 and take part in the sum
    dil_t = kept[True]
    with torch.no_grad():
        w64, _, _ = _edge_reference(wq.double(), x.double(), dil_t["row_off"], dil_t["key"], tau.double(), "reference", shape, SCALE)
        w32, _, _ = _edge_reference(wq, x, dil_t["row_off"], dil_t["key"], tau, "reference", shape, SCALE)
    _check(f"refresh weight {shape} radius {radius} keep_all tau", dil_t["weight"], w64, w32)
    assert torch.equal(dil_t["weight"] != 0, w64 != 0) and 0 < int((w64 != 0).sum()) < w64.numel()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_empty_graph(shape):
    """An empty input graph, and one whose only keys lie off the map, give an empty output."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    wq, x = torch.rand(B, L, 196, device=DEV), torch.rand(B, N, 196, device=DEV)
    row_off = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    for kw in (dict(), dict(tau=torch.rand(B * L, device=DEV), k=8), dict(keep_all=True, radius=2), dict(max_row_edges=0)):
        out = ops.graph_refresh(wq, x, row_off, key, hw=(H, W), **kw)
        assert out["key"].shape == out["weight"].shape == out["score"].shape == (0,)
        assert out["row_off"].shape == (B * L + 1,) and bool((out["row_off"] == 0).all())
    # only keys off the map: candidates of nothing
    row_off[1:] = 2
    out = ops.graph_refresh(wq, x, row_off, torch.tensor([-1, N], dtype=torch.int32, device=DEV), radius=1, hw=(H, W))
    assert out["key"].numel() == 0 and bool((out["row_off"] == 0).all())


def test_overlong_rows_are_refused_not_truncated():
    """A row one edge longer than the declared ``max_row_edges``: ``ops`` raises ``ERR_UNSUPPORTED``; at the C level the row comes out empty,
    ``status_out[0]`` counts it and every other row is what it was."""
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    B, H, W, L, N = _geom(shape)
    args, tau_dev = _device_args(shape)
    with pytest.raises(_lib.DaglError, match="1 row") as e:
        ops.graph_refresh(*args, radius=1, k=8, max_row_edges=MAX_ROW - 1, hw=(H, W))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    whole = _cpu(ops.graph_refresh(*args, radius=1, k=8, max_row_edges=MAX_ROW, hw=(H, W)))
    # at the C level: the row comes out empty, status[0] counts it, the other rows are what they were
    lib = _lib.load()
    E = args[3].numel()
    need = lib.dagl_graph_refresh_workspace_bytes(B, H, W, E, 1)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    a = (ws.data_ptr() + 255) // 256 * 256
    cap = B * L * 8
    off = torch.empty(B * L + 1, dtype=torch.int64, device=DEV)
    key, weight, score = (torch.empty(cap, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32, torch.float32))
    status = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    rc = lib.dagl_graph_refresh(torch.cuda.current_stream().cuda_stream, B, H, W, *(t.data_ptr() for t in args), E, MAX_ROW - 1, 1, None,
                                8, C.c_float(10.0), 0, off.data_ptr(), key.data_ptr(), weight.data_ptr(), score.data_ptr(), cap,
                                status.data_ptr(), a, need)
    assert rc == 0, lib.dagl_last_error()
    torch.cuda.synchronize()
    off, n = off.cpu(), int(off[-1])
    assert status.tolist()[0] == 1 and 0 < status.tolist()[1] <= (MAX_ROW - 1) * 9
    assert int(off[8] - off[7]) == 0
    got, want = mask_of(off, key[:n].cpu(), N), mask_of(whole["row_off"], whole["key"], N)
    keep = torch.arange(B * L) != 7
    assert torch.equal(got[keep], want[keep]) and int(want[7].sum()) == 8
    rows_w = _rows_of(whole["row_off"])
    assert torch.equal(weight[:n].cpu(), whole["weight"][rows_w != 7]) and torch.equal(score[:n].cpu(), whole["score"][rows_w != 7])


def test_operand_refusals():
    from dagl_amd import _lib, ops
    shape = SHAPES[0]
    args, tau_dev = _device_args(shape)
    cap = ops.graph_refresh_max_candidates()
    assert cap >= 2048
    hw = shape[1:]
    for kw, word in ((dict(radius=9), "radius"), (dict(radius=-1), "radius"), (dict(k=-1), "k=-1"), (dict(scale=0.0), "scale"),
                     (dict(normalize="rows"), "normalize"), (dict(tau=tau_dev[:-1]), "tau"), (dict(hw=(24, 24)), "map"),
                     (dict(hw=None), "pass hw")):
        with pytest.raises(_lib.DaglError, match=word):
            ops.graph_refresh(*args, **{"hw": hw, **kw})
    with pytest.raises(_lib.DaglError, match="candidates") as e:
        ops.graph_refresh(*args, radius=8, max_row_edges=MAX_ROW, hw=hw)                # 12 x 289
    assert e.value.code == _lib.ERR_UNSUPPORTED

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = args[0] + 1.0
            ops.graph_refresh(*args, max_row_edges=MAX_ROW, hw=hw)
    with pytest.raises(_lib.DaglError, match="captur"):
        captured()
    torch.cuda.synchronize()
