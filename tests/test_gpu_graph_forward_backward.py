"""``ops.graph_forward_train`` / ``ops.graph_forward_backward`` (dagl_graph_forward_train, dagl_graph_forward_backward,
csrc/graph_forward.hip): the fused forward on a given patch graph with the row statistics kept, and its backward in one crossing of the
edges.

Every reference is torch on the CPU: fp64 autograd of ``_forward_reference`` (test_gpu_graph_forward: the formulas of include/dagl_ce.h
for dagl_graph_attend + dagl_graph_apply, keys outside [0, N) included) for a seeded ``d_out``, on the crafted graphs of ``_graph`` --
empty first and last rows, a row across three segments, a row of N + 5 edges, short rows that share a segment, two empty rows at an image
boundary.  Bound (the two ops' own): ``e_lib <= 3 e_32 + 1e-6`` normwise, ``e_32`` the same evaluation in fp32 against fp64."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.graph_reference import KSHAPES, _check, _edge_scores, _geom, _graph, _id, _level_features, _padded, _rows_of
from tests.helpers import normwise
from tests.test_gpu_graph_forward import _bad_key, _forward_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 10.0
VARIANTS = [(True, "reference"), (False, "reference"), (True, "edges"), (False, "edges")]          # (with tau, normalize)
U32 = 2.0 ** -24


def _vid(v):
    return ("tau" if v[0] else "notau") + "-" + v[1]


@functools.lru_cache(maxsize=None)
def _features(shape, seed=7):
    row_off, key, _ = _graph(shape)
    return _level_features(row_off, key, shape, seed)


@functools.lru_cache(maxsize=None)
def _d_out(shape):
    B, H, W, _, _ = _geom(shape)
    return torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(9))


@functools.lru_cache(maxsize=None)
def _grad_reference(shape, with_tau, normalize, bad, dtype):
    """(d_wq, d_x, d_tau | None, d_b2) by autograd in ``dtype``, computed once per case and shared (read-only)."""
    row_off, key, b2 = _graph(shape)
    key = _bad_key(shape) if bad else key
    wq, x, tau = _features(shape)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (wq, x, tau, b2)]
    torch.set_num_threads(16)
    out = _forward_reference(leaves[0], leaves[1], leaves[3], row_off, key, leaves[2] if with_tau else None, normalize, shape)
    (out * _d_out(shape).to(dtype)).sum().backward()
    return leaves[0].grad, leaves[1].grad, leaves[2].grad if with_tau else None, leaves[3].grad


@functools.lru_cache(maxsize=None)
def _transposed(shape, bad):
    """(col_off [B N + 1], src_row [E], perm [E]) on the CPU: the edges with a key of the map in a stable order of their column, as
    ``PatchGraph.transpose`` orders them (which refuses keys outside the map); the edges without a column come behind the last column's
    and carry a source row or a ``perm`` entry outside its range (B L, -1; -1, E), so that nothing of them may be looked up."""
    row_off, key, _ = _graph(shape)
    key = _bad_key(shape) if bad else key
    B, H, W, L, N = _geom(shape)
    rows, E = _rows_of(row_off), key.numel()
    valid = (key >= 0) & (key < N)
    e_valid = torch.nonzero(valid).reshape(-1)
    col = (rows[e_valid] // L) * N + key[e_valid].long()
    col, order = torch.sort(col, stable=True)
    perm_valid = e_valid[order]
    col_off = torch.searchsorted(col, torch.arange(B * N + 1))
    e_bad = torch.nonzero(~valid).reshape(-1).tolist()
    assert len(e_bad) == (3 if bad else 0)
    # (source row, perm) of the three: a row past the last with a real edge, a real row with perm -1, row -1 with perm E
    junk = [(B * L, e_bad[0]), (int(rows[e_bad[1]]), -1), (-1, E)] if bad else []
    src_row = torch.cat([rows[perm_valid], torch.tensor([r for r, _ in junk], dtype=torch.int64)]).int()
    perm = torch.cat([perm_valid, torch.tensor([p for _, p in junk], dtype=torch.int64)]).int()
    assert src_row.numel() == perm.numel() == E and int(col_off[-1]) == int(valid.sum())
    return col_off.contiguous(), src_row.contiguous(), perm.contiguous()


def _device_args(shape, with_tau, bad):
    row_off, key, b2 = _graph(shape)
    key = _bad_key(shape) if bad else key
    wq, x, tau = _features(shape)
    return [t.to(DEV) for t in (wq, x, _padded(b2), row_off, key)], tau.to(DEV) if with_tau else None


def _interior(d_b2p, H, W):
    return d_b2p[:, 3:3 + H, 3:3 + W, :].permute(0, 3, 1, 2)


def _run(shape, with_tau, normalize, bad, **kw):
    """-> (forward outputs, backward outputs, the arguments of the backward) of the library on ``shape``."""
    from dagl_amd import ops
    (wq, x, b2p, row_off, key), tau = _device_args(shape, with_tau, bad)
    call = dict(tau=tau, scale=SCALE, normalize=normalize)
    fwd = ops.graph_forward_train(wq, x, b2p, row_off, key, **call)
    args = (_d_out(shape).to(DEV), wq, x, b2p, row_off, key, fwd[1], fwd[2])
    call["transposed"] = tuple(t.to(DEV) for t in _transposed(shape, bad))
    return fwd, ops.graph_forward_backward(*args, **call, **kw), args, call


@pytest.mark.parametrize("bad", [False, True], ids=["keys_in_range", "keys_out_of_range"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", KSHAPES, ids=_id)
def test_kernel_gradients(shape, variant, bad):
    """Test A: d_wq, d_x, d_tau and d_b2p against fp64 autograd of the reference.  Under "edges" a row of one edge is one-hot: its weight
    is exactly 1 when the backward sees the logit the forward took the maximum from, and its d_wq row is zero within the bound."""
    with_tau, normalize = variant
    B, H, W, L, N = _geom(shape)
    ref64 = _grad_reference(shape, with_tau, normalize, bad, torch.float64)
    ref32 = _grad_reference(shape, with_tau, normalize, bad, torch.float32)
    _, (d_wq, d_x, d_tau, d_b2p), _, _ = _run(shape, with_tau, normalize, bad)
    what = f"{shape} {_vid(variant)}{' bad keys' if bad else ''}"
    assert d_wq.shape == (B, L, 196) and d_x.shape == (B, N, 196) and d_b2p.shape == (B, H + 6, W + 6, 16)
    _check("d_wq " + what, d_wq, ref64[0], ref32[0])
    _check("d_x " + what, d_x, ref64[1], ref32[1])
    _check("d_b2 " + what, _interior(d_b2p, H, W), ref64[3], ref32[3])
    if with_tau:
        assert d_tau.shape == (B * L,)
        _check("d_tau " + what, d_tau, ref64[2], ref32[2])
    else:
        assert d_tau is None
    if normalize == "edges":
        row_off, _, _ = _graph(shape)
        one = torch.nonzero((row_off[1:] - row_off[:-1]) == 1).reshape(-1)
        assert L == 4 or one.numel() >= B                                       # (an 8x8 map has no row to spare for it)
        if one.numel():
            e_32 = normwise(ref32[0].double().numpy(), ref64[0].numpy())
            worst = float(d_wq.reshape(B * L, 196)[one.to(DEV)].abs().max()) / float(ref64[0].abs().max())
            print(f"[graph_forward_backward] {what}: largest |d_wq| of the {one.numel()} one-edge rows / max |d_wq| = {worst:.2e}")
            assert float(ref64[0].reshape(B * L, 196)[one].abs().max()) <= 1e-12 * float(ref64[0].abs().max())      # the truth is zero
            assert worst <= 3.0 * e_32 + 1e-6


def _reference_stats(shape, with_tau, normalize, bad):
    """(M [B L], D [B L]) in fp64, the statistics inside ``_forward_reference``, and the largest |S| and |m| of the case."""
    row_off, key, _ = _graph(shape)
    key = _bad_key(shape) if bad else key
    wq, x, tau = (t.double() for t in _features(shape))
    B, H, W, L, N = _geom(shape)
    deg, rows = row_off[1:] - row_off[:-1], _rows_of(row_off)
    valid = (key >= 0) & (key < N)
    S = _edge_scores(wq, x, rows, key.clamp(0, N - 1), L, N) * valid.double()
    m = F.relu(S - tau[rows]) if with_tau else torch.ones_like(S)
    z = S * m * SCALE
    pos = torch.arange(key.numel()) - row_off[rows]
    Z = torch.full((B * L, max(int(deg.max()), 1)), float("-inf"), dtype=torch.float64).index_put((rows, pos), z)
    off = (N - deg).clamp(min=0) if normalize == "reference" else torch.zeros_like(deg)
    M = Z.max(dim=1).values
    M = torch.where(off > 0, M.clamp(min=0.0), M)
    M = torch.where(deg > 0, M, torch.zeros_like(M))
    D = torch.exp(Z - M.unsqueeze(1)).sum(dim=1) + off.double() * torch.exp(-M)
    return M, D, float(S.abs().max()), float(m.abs().max())


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", [KSHAPES[0], KSHAPES[1]], ids=_id)
def test_bits(shape, variant):
    """Test B: the training forward returns the forward's bits and the rows' (M, D); the backward gives the same bits on a second call,
    through a ``Workspace`` and for every subset of its outputs.

    The statistics' tolerance is the rounding of their inputs: a score is a 196-term fp32 dot product (relative error at most
    gamma = 200 u, u = 2^-24), the logit ``scale S m`` with ``m = S - tau`` carries ``scale (|S| + |m|)`` times the score's absolute
    error, so ``|M - M_64| <= gamma scale S_max (S_max + m_max) + 4 u |M_64|``; D sums ``e^(z - M)``, each term off by at most twice that
    (z and M) relatively, plus expf and the fp32 value of each term: ``|D / D_64 - 1| <= 2 tol_M + 8 u``."""
    from dagl_amd import ops
    with_tau, normalize = variant
    (out, row_max, row_sum), grads, args, call = _run(shape, with_tau, normalize, True)
    (wq, x, b2p, row_off, key), tau = _device_args(shape, with_tau, True)
    assert torch.equal(out, ops.graph_forward(wq, x, b2p, row_off, key, tau=tau, scale=SCALE, normalize=normalize))
    assert row_max.dtype == torch.float32 and row_sum.dtype == torch.float64
    M, D, s_max, m_max = _reference_stats(shape, with_tau, normalize, True)
    deg = (row_off[1:] - row_off[:-1]).cpu()
    tol_m = 200 * U32 * SCALE * s_max * (s_max + m_max)
    err_m = (row_max.double().cpu() - M).abs()
    err_d = (row_sum.cpu() / D - 1).abs()
    print(f"[graph_forward_backward] {shape} {_vid(variant)}: max |M - M64| {float(err_m[deg > 0].max()):.2e} (tolerance {tol_m:.2e} + "
          f"4 u |M64|), max |D / D64 - 1| {float(err_d[deg > 0].max()):.2e} (tolerance {2 * tol_m + 8 * U32:.2e})")
    assert bool((err_m <= tol_m + 4 * U32 * M.abs())[deg > 0].all()) and float(err_d[deg > 0].max()) <= 2 * tol_m + 8 * U32
    assert bool((row_max.cpu()[deg == 0] == 0).all()) and bool((row_sum.cpu()[deg == 0] == 1).all())

    def same(got, keep):
        for i, (a, b) in enumerate(zip(got, grads)):
            assert (a is None) if (i not in keep or b is None) else torch.equal(a, b), i

    ws = ops.Workspace()
    same(ops.graph_forward_backward(*args, **call), (0, 1, 2, 3))
    same(ops.graph_forward_backward(*args, workspace=ws, **call), (0, 1, 2, 3))
    same(ops.graph_forward_backward(*args, workspace=ws, **call), (0, 1, 2, 3))
    names = ("need_wq", "need_x", "need_tau", "need_b2p")
    subsets = [(0,), (1,), (2,), (3,), (0, 2), (1, 3), (0, 1, 2)]
    for keep in subsets:
        kw = dict(call, **{n: i in keep for i, n in enumerate(names)})
        if 1 not in keep and 3 not in keep:
            kw["transposed"] = None                                              # the row gradients need no transposed CSR
        same(ops.graph_forward_backward(*args, **kw), keep)


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_against_the_two_ops(variant):
    """Test C: the fused backward next to ``graph_apply_backward`` (on ``graph_attend``'s weights) chained with ``graph_attend_backward`` on
    the same arrays: both errors against fp64 are printed and each is held to the bound on its own, neither to the other."""
    from dagl_amd import ops
    from dagl_amd.graph import PatchGraph
    shape = KSHAPES[1]
    with_tau, normalize = variant
    B, H, W, L, N = _geom(shape)
    ref64 = _grad_reference(shape, with_tau, normalize, False, torch.float64)
    ref32 = _grad_reference(shape, with_tau, normalize, False, torch.float32)
    _, fused, (d_out, wq, x, b2p, row_off, key, _, _), call = _run(shape, with_tau, normalize, False)
    pg = PatchGraph(row_off, key, torch.zeros(key.numel(), device=DEV), None, B, H, W)
    kw = dict(tau=call["tau"], scale=SCALE, normalize=normalize)
    weight, score = ops.graph_attend(wq, x, row_off, key, hw=(H, W), **kw)
    d_b2p, d_weight = ops.graph_apply_backward(d_out, b2p, row_off, key, weight, transposed=pg.transpose())
    d_wq, d_x, d_tau = ops.graph_attend_backward(d_weight, wq, x, row_off, key, score, weight, transposed=pg.transpose(), hw=(H, W), **kw)
    two = (d_wq, d_x, d_tau, d_b2p)
    for i, name in enumerate(("d_wq", "d_x", "d_tau", "d_b2")):
        if ref64[i] is None:                                                     # d_tau without tau
            assert fused[i] is None and two[i] is None
            continue
        r64, r32 = ref64[i], ref32[i]
        pick = (lambda t: _interior(t, H, W)) if i == 3 else (lambda t: t)
        _check(f"fused {name} {shape} {_vid(variant)}", pick(fused[i]), r64, r32)
        _check(f"two ops {name} {shape} {_vid(variant)}", pick(two[i]), r64, r32)


@pytest.mark.parametrize("shape", [KSHAPES[0], KSHAPES[1]], ids=_id)
def test_empty_graph(shape):
    """Test D: no edge at all -- every gradient is zeros, the statistics hold 0 and 1, no launch fails."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(shape)
    wq, x = torch.rand(B, L, 196, device=DEV), torch.rand(B, N, 196, device=DEV)
    b2p = torch.randn(B, H + 6, W + 6, 16, device=DEV)
    row_off = torch.zeros(B * L + 1, dtype=torch.int64, device=DEV)
    key = torch.empty(0, dtype=torch.int32, device=DEV)
    transposed = (torch.zeros(B * N + 1, dtype=torch.int64, device=DEV), key, key)
    d_out = torch.randn(B, 16, H, W, device=DEV)
    for tau in (None, torch.rand(B * L, device=DEV)):
        for normalize in ("reference", "edges"):
            out, row_max, row_sum = ops.graph_forward_train(wq, x, b2p, row_off, key, tau=tau, normalize=normalize)
            assert out.shape == (B, 16, H, W) and bool((out == 0).all())
            assert bool((row_max == 0).all()) and bool((row_sum == 1).all())
            d_wq, d_x, d_tau, d_b2p = ops.graph_forward_backward(d_out, wq, x, b2p, row_off, key, row_max, row_sum, tau=tau,
                                                                 normalize=normalize, transposed=transposed)
            assert d_wq.shape == wq.shape and d_x.shape == x.shape and d_b2p.shape == b2p.shape
            assert bool((d_wq == 0).all()) and bool((d_x == 0).all()) and bool((d_b2p == 0).all())
            assert (d_tau is None) if tau is None else (d_tau.shape == (B * L,) and bool((d_tau == 0).all()))
    torch.cuda.synchronize()


def test_operand_refusals():
    from dagl_amd import DaglError, ops
    shape = KSHAPES[0]
    (out, row_max, row_sum), _, args, call = _run(shape, True, "reference", False)
    d_out, wq, x, b2p, row_off, key = args[:6]
    for refused in (lambda: ops.graph_forward_backward(d_out[:, :8].contiguous(), *args[1:], **call),
                    lambda: ops.graph_forward_backward(*args[:6], row_max[:-1].contiguous(), row_sum, **call),
                    lambda: ops.graph_forward_backward(*args[:7], row_sum.float(), **call),
                    lambda: ops.graph_forward_backward(*args, **dict(call, transposed=None)),
                    lambda: ops.graph_forward_backward(*args, **dict(call, transposed=None), need_x=False),
                    lambda: ops.graph_forward_backward(*args, **dict(call, normalize="rows")),
                    lambda: ops.graph_forward_train(wq, x, b2p[:, :-1].contiguous(), row_off, key),
                    lambda: ops.graph_forward_train(wq, x, b2p, row_off, key, scale=0.0)):
        with pytest.raises(DaglError):
            refused()
