"""The dense training core (dense_train.hip: dagl_ce_core_dense_forward / _backward, dagl_ce_core_wide_forward / _backward) under
every branch of its launch plan, against the fp64 oracle and its autograd: several chunks per image with a ragged last one, image
groups with a remainder, every split-K factor of d Wq, maps smaller than the window, rows whose mask is empty or full, the wide
top-k modes across chunks.  The chunk budget is a run-time value (ops.dense_chunk_budget), so every case is small; each case first
asserts the plan ops.dense_plan reports, so none can silently run the one-chunk plan.

Tolerance, per tensor, normwise (tests.helpers.normwise): e_hip = kernel vs fp64, e_ref = the same oracle in fp32 on the CPU vs
fp64.  Forward: e_hip <= 1e-4.  Gradients: e_hip <= min(3 e_ref + 2e-6, 3e-4) -- three times what plain fp32 costs, the 2e-6 floor
test_dense_core_matches_the_oracle_and_its_autograd grants the split-fp16 products, and its cap.  Every case also asserts
e_ref <= 1e-4: a reference that loses its own digits to cancellation would loosen the bound instead of failing.
One run's [parity] lines: profiles/r12_dense_plan_parity.log."""
import functools
import os
import zlib

import pytest
import torch

from tests.helpers import normwise

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
GRADS = ("d_wq", "d_x", "d_b2", "d_thr", "d_bias")


def _budget(rows, H, W):
    """Floats of ``rows`` query rows of a [chunk, N] matrix (N rounded up to 32, as dt_plan does)."""
    return rows * ((H * W + 31) // 32 * 32)


# name -> shape, chunk budget in floats (0 = the built-in one), the plan asserted before anything runs, selection mode
CASES = {
    # N < 512: no split of d Wq; N % 32 != 0; L = 35 just over one 32-row pad of the transposed copies
    "k1": dict(shape=(1, 19, 25), budget=0, plan=dict(n_chunks=1, kslices=1, h16=1)),
    "k2": dict(shape=(2, 24, 28), budget=0, plan=dict(n_chunks=1, Bc=2, kslices=2, h16=1)),
    # two M tiles, the second ragged (L = 144); 189 zero-padded K columns of d Wq
    "k8": dict(shape=(1, 47, 45), budget=0, plan=dict(n_chunks=1, kslices=8, nk=2304, h16=1)),
    # chunks of 128, 128 and 16 queries: offsets into every per-query array, beta = 1 accumulation of d X and d V, fp32 products
    "chunks3": dict(shape=(1, 64, 68), budget=_budget(128, 64, 68), plan=dict(Lc=128, n_chunks=3, Bc=1, h16=0)),
    "chunks2x2": dict(shape=(2, 48, 50), budget=_budget(128, 48, 50), plan=dict(Lc=128, n_chunks=2, Bc=1, h16=0)),
    # image groups of 2, 2, 1 on the split-fp16 route: scale words and operand copies redone per group
    "groups221": dict(shape=(5, 45, 38), budget=_budget(2 * 128, 45, 38), plan=dict(Lc=120, n_chunks=1, Bc=2, h16=1)),
    # ... with the last image 16 times larger (b2 and G): a scale word kept from an earlier group would send its halves to infinity
    "groups221_scaled": dict(shape=(5, 45, 38), budget=_budget(2 * 128, 45, 38), plan=dict(Lc=120, n_chunks=1, Bc=2, h16=1),
                             image_scale=(1.0, 1.0, 1.0, 1.0, 16.0)),
    "groups111": dict(shape=(3, 19, 25), budget=_budget(35, 19, 25), plan=dict(Lc=35, n_chunks=1, Bc=1, h16=1)),
    # maps under the 7 x 7 window, L = 1 .. 18, N < 32
    "tiny_1x1": dict(shape=(1, 1, 1), budget=0, plan=dict(Lc=1, n_chunks=1)),
    "tiny_4x4": dict(shape=(1, 4, 4), budget=0, plan=dict(Lc=1, n_chunks=1)),
    "tiny_7x9": dict(shape=(2, 7, 9), budget=0, plan=dict(Lc=6, n_chunks=1, Bc=2)),
    "tiny_5x40": dict(shape=(1, 5, 40), budget=0, plan=dict(Lc=20, n_chunks=1)),
    "tiny_3x70": dict(shape=(1, 3, 70), budget=0, plan=dict(Lc=18, n_chunks=1)),
    # 8 rows of degree 0 and 8 of degree N in the last image, some of each in the last chunk
    "degenerate": dict(shape=(2, 45, 38), budget=0, plan=dict(n_chunks=1, Bc=2, kslices=4, nk=1792, h16=1), degenerate=True),
    "degenerate_chunks3": dict(shape=(1, 64, 68), budget=_budget(128, 64, 68), plan=dict(Lc=128, n_chunks=3, h16=0), degenerate=True),
    # the wide top-k modes: selection words, re-selection in the backward, per chunk and per group
    "wide_topk100_chunks3": dict(shape=(1, 64, 68), budget=_budget(128, 64, 68), plan=dict(Lc=128, n_chunks=3), mode="topk", k=100),
    "wide_adaptive_topk80_chunks3": dict(shape=(1, 64, 68), budget=_budget(128, 64, 68), plan=dict(Lc=128, n_chunks=3),
                                         mode="adaptive_topk", k=80),
    "wide_topk200_groups": dict(shape=(5, 30, 26), budget=_budget(2 * 56, 30, 26), plan=dict(Lc=56, n_chunks=1, Bc=2), mode="topk", k=200),
    # ([1,36,40] has L = 90 < 128 queries: a chunk never holds fewer than 128, so it stays one chunk under any budget)
    "wide_topk90_ties_chunks2": dict(shape=(1, 48, 50), budget=_budget(128, 48, 50), plan=dict(Lc=128, n_chunks=2), mode="topk", k=90,
                                     ties=True),
    # ... and with the adaptive test in force but passed by every key (thr = 0, bias = 1: m = S + 1 >= 1), so that the tie falls where
    # the topk case has it: the tie rule is shared by both modes
    "wide_adaptive_topk90_ties_chunks2": dict(shape=(1, 48, 50), budget=_budget(128, 48, 50), plan=dict(Lc=128, n_chunks=2),
                                              mode="adaptive_topk", k=90, ties=True),
}
_SEEDS = {name: zlib.crc32(name.encode()) for name in CASES}       # (a case added later leaves the others' inputs alone)


def _geom(name):
    B, H, W = CASES[name]["shape"]
    return B, H, W, -(-H // 4) * -(-W // 4), H * W


def _midgap_thresholds(S):
    """Per query the middle of the widest gap between consecutive sorted scores inside the 30 .. 70 % band (the mask is discontinuous: a key
    within rounding of the threshold would flip between fp32 and fp64 scores and move the output by 1 / degree)."""
    N = S.shape[2]
    v = S.sort(dim=2).values
    if N == 1:
        return v[:, :, 0] - 0.25 * v[:, :, 0].abs()
    lo = min(int(0.3 * N), N - 2)
    hi = max(lo + 1, min(int(0.7 * N), N - 1))
    gap = v[:, :, lo + 1:hi + 1] - v[:, :, lo:hi]
    at = gap.argmax(dim=2, keepdim=True) + lo
    return 0.5 * (v.gather(2, at) + v.gather(2, at + 1)).squeeze(2)


def degenerate_rows(L):
    """(rows of degree 0, rows of degree N): 8 each, spread over the queries, two of each among the last 16."""
    return ([0, 17, L // 2 - 1, L // 2, L - 16, L - 9, L - 2, L - 1], [1, 18, L // 2 - 2, L // 2 + 1, L - 15, L - 8, L - 3, L - 4])


def _kth_gap(wq, xr, k):
    """fp64 relative gap between every row's k-th and (k+1)-th best score -> [B,L]."""
    v = torch.einsum("bld,bnd->bln", wq.double(), xr.double()).sort(dim=2, descending=True).values
    return (v[:, :, k - 1] - v[:, :, k]) / v[:, :, k - 1].abs()


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(wq, xr, b2, thr, bias, G) of a case on the CPU in fp32 (thr / bias None in mode "topk") and a dict of what the builder knows."""
    case = CASES[name]
    B, H, W, L, N = _geom(name)
    mode, k = case.get("mode", "adaptive"), case.get("k")
    g = torch.Generator().manual_seed(_SEEDS[name])
    facts = {}
    if case.get("ties"):
        # Scores tied THROUGH IDENTICAL KEY ROWS: 40 distinct rows, key j holds row j % 40, so every query has 40 score values 60 keys
        # each and the k-th place falls inside the second group: the lowest key indices of it win.  Features are multiples of 2^-7
        # below 2^-3: every product and every partial sum is exact in fp32 and in fp64 in any order, a tie is a tie on both sides.
        wq = torch.randint(0, 16, (B, L, 196), generator=g).float() / 128.0
        xr = (torch.randint(0, 16, (B, 40, 196), generator=g).float() / 128.0).repeat(1, N // 40, 1)
        facts["kth_gap"] = _kth_gap(wq, xr, k)
    else:
        wq = torch.rand(B, L, 196, generator=g) * 0.1
        xr = torch.rand(B, N, 196, generator=g) * 0.1
    b2 = torch.randn(B, 16, H, W, generator=g)
    G = torch.randn(B, 16, H, W, generator=g)
    if case.get("image_scale"):
        f = torch.tensor(case["image_scale"]).view(B, 1, 1, 1)
        b2, G = b2 * f, G * f
    if mode != "adaptive" and not case.get("ties"):
        # a k-th and a (k+1)-th score within fp32 rounding of each other would be taken in either order: rows whose fp64 gap is
        # under 2e-5 of the score are drawn again (one row in seventeen at these sizes); the test asserts the gap it relies on
        for _ in range(50):
            close = _kth_gap(wq, xr, k) <= 2e-5
            if not bool(close.any()):
                break
            wq[close] = torch.rand(int(close.sum()), 196, generator=g) * 0.1
        facts["kth_gap"] = _kth_gap(wq, xr, k)
    thr = bias = None
    if mode != "topk" and case.get("ties"):
        thr, bias = torch.zeros(B, L), torch.ones(B, L)                    # scores are sums of non-negative products: every key passes
    elif mode != "topk":
        S = torch.einsum("bld,bnd->bln", wq.double(), xr.double())
        T = _midgap_thresholds(S)
        if case.get("degenerate"):
            zero, full = degenerate_rows(L)
            span = S.max(dim=2).values - S.min(dim=2).values
            T[B - 1, zero] = (S.max(dim=2).values + 0.1 * span + 1e-3)[B - 1, zero]
            T[B - 1, full] = (S.min(dim=2).values - 0.1 * span - 1e-3)[B - 1, full]
        thr = 1.0 + 0.02 * torch.randn(B, L, generator=g)
        bias = (S.mean(dim=2) * thr.double() - T).float()                  # T = mu * thr - bias
    return (wq, xr, b2, thr, bias, G), facts


def _oracle(name, dtype):
    from oracle.ce_oracle import ce_core_oracle
    case = CASES[name]
    (wq, xr, b2, thr, bias, G), _ = case_inputs(name)
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_(True) for t in (wq, xr, b2, thr, bias)]
    out, st = ce_core_oracle(*leaves, mode=case.get("mode", "adaptive"), k=case.get("k"), dtype=dtype, stages=True)
    (out * G.to(dtype)).sum().backward()
    return out.detach(), [None if t is None else t.grad for t in leaves], st["deg"].detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle with its autograd and the same in fp32, once per case: dict(out, grads, deg, e_ref per gradient, e_ref_out)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out64, g64, deg = _oracle(name, torch.float64)
    out32, g32, _ = _oracle(name, torch.float32)
    e_ref = {n: normwise(a.numpy(), b.numpy()) for n, a, b in zip(GRADS, g32, g64) if b is not None}
    return dict(out=out64, grads=dict(zip(GRADS, g64)), deg=deg, e_ref=e_ref, e_ref_out=normwise(out32.numpy(), out64.numpy()))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_case(name, exact=False):
    """The case's forward and backward through the core ops under its budget, the plan asserted first -> (out, grads dict, info).
    The chunked calls get a workspace filled with 0xFF bytes (NaN as floats and as halves): a pad row or column that a product
    reads and no kernel wrote shows up as NaN instead of depending on what the allocator handed out."""
    from dagl_amd import _lib, ops
    case = CASES[name]
    B, H, W, L, N = _geom(name)
    mode, k = case.get("mode", "adaptive"), case.get("k")
    (wq, xr, b2, thr, bias, G), _ = case_inputs(name)
    dev = _dev()
    d = [None if t is None else t.to(dev) for t in (wq, xr, b2, thr, bias)]
    with ops.dense_chunk_budget(case["budget"]):
        for backward in (False, True):
            plan = ops.dense_plan(B, H, W, backward=backward)
            want = {f: v for f, v in case["plan"].items() if backward or f != "h16"}
            assert {f: plan[f] for f in want} == want, (name, plan)
        lib, ws = _lib.load(), ops.Workspace()
        nbytes = max(lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 0) + 256, lib.dagl_ce_core_dense_workspace_bytes(B, H, W, 1))

        def poisoned():
            ws.get(nbytes, dev).fill_(0xFF)
            return ws

        if mode == "adaptive":
            streamed = not exact and N >= 2048             # (the streamed forward keeps words of its own in its workspace: a fresh one)
            out, saved = ops.ce_core_dense_forward(*d, workspace=None if streamed else poisoned(), exact=exact)
            info = saved["info"]
            grads = ops.ce_core_dense_backward(G.to(dev), *d, saved, workspace=poisoned(), exact=exact)
        else:
            out, info = ops.ce_core_wide_forward(*d, mode, k, workspace=poisoned(), want_info=True)
            grads = ops.ce_core_wide_backward(G.to(dev), *d, mode, k, workspace=poisoned())
        torch.cuda.synchronize()
    return out, dict(zip(GRADS, grads)), info


def check_values(name, out, grads, info, label):
    case = CASES[name]
    B, H, W, L, N = _geom(name)
    ref = reference(name)
    what = f"[{B},{H},{W}] {case.get('mode', 'adaptive')} {name} {label}"
    assert info["total_edges"] == int(ref["deg"].sum()) and info["max_degree"] == int(ref["deg"].max()), what
    e_out = normwise(out.cpu().numpy(), ref["out"].numpy())
    print(f"[parity] {what} out: e_hip {e_out:.2e}  e_ref {ref['e_ref_out']:.2e}  bound {TOL_OUT:.2e}")
    failed = [] if e_out <= TOL_OUT else ["out"]
    for n in GRADS:
        want = ref["grads"][n]
        if want is None:
            assert grads[n] is None, what
            continue
        e_ref = ref["e_ref"][n]
        e_hip = normwise(grads[n].cpu().numpy(), want.numpy())
        bound = min(3.0 * e_ref + 2e-6, 3e-4)
        print(f"[parity] {what} {n}: e_hip {e_hip:.2e}  e_ref {e_ref:.2e}  bound {bound:.2e}")
        assert e_ref <= 1e-4, (what, n, "the fp32 reference itself is too far from fp64: pick another seed")
        if not e_hip <= bound:
            failed.append(n)
        if case.get("degenerate") and n in ("d_thr", "d_bias"):
            # degree-0 rows: the fp64 gradient is identically zero there; absolute, against the tensor's largest magnitude elsewhere
            zero, _ = degenerate_rows(L)
            assert float(want[B - 1, zero].abs().max()) == 0.0, what
            assert float(grads[n][B - 1, zero].abs().max()) <= bound * float(want.abs().max()), (what, n)
    assert not failed, (what, failed)


_BOTH_FORMS = ("k1", "k2", "k8", "chunks3", "chunks2x2", "groups221", "groups221_scaled", "groups111")


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", _BOTH_FORMS)
def test_dense_core_under_every_plan_matches_fp64(name, exact):
    """``exact`` = the forward in its chunked fp32 GEMM form whatever the size (the default form of N >= 2048 keys is the streamed
    kernel, which does not chunk) and the backward's products on the fp32 matrix cores where the plan would take the fp16 ones."""
    out, grads, info = run_case(name, exact=exact)
    check_values(name, out, grads, info, "exact" if exact else "default")


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("tiny_")])
def test_maps_smaller_than_the_window_match_fp64(name):
    out, grads, info = run_case(name)
    check_values(name, out, grads, info, "default")


@pytest.mark.parametrize("name", ["degenerate", "degenerate_chunks3"])
def test_rows_with_an_empty_or_a_full_mask_match_fp64(name):
    B, H, W, L, N = _geom(name)
    deg = reference(name)["deg"]
    zero, full = degenerate_rows(L)
    assert len(set(zero + full)) == 16 and min(zero + full) >= 0
    assert bool((deg[B - 1, zero] == 0).all()) and bool((deg[B - 1, full] == N).all())
    assert sum(r >= L - 16 for r in zero) >= 1 and sum(r >= L - 16 for r in full) >= 1          # the last chunk holds some of each
    for exact in (False, True):
        out, grads, info = run_case(name, exact=exact)
        check_values(name, out, grads, info, "exact" if exact else "default")


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("wide_")])
def test_wide_modes_across_chunks_and_groups_match_fp64(name):
    case = CASES[name]
    _, facts = case_inputs(name)
    gap = facts["kth_gap"]
    if case.get("ties"):
        assert bool((gap == 0).all())                      # every row ties at the k-th place: the lower key index decides
        assert bool((reference(name)["deg"] == case["k"]).all())             # ... and exactly k keys are taken, not all that reach the k-th score
    else:
        assert float(gap.min()) > 1e-5, float(gap.min())   # no row leaves the choice of its k-th key to fp32 rounding
    out, grads, info = run_case(name)
    assert info["max_degree"] <= case["k"]
    check_values(name, out, grads, info, f"k={case['k']}")


@pytest.mark.parametrize("name", ["chunks3", "groups221"])
def test_chunking_and_grouping_do_not_change_a_bit_of_the_per_query_results(name):
    """fp32 products (``exact``), the built-in budget against the case's small one.  gemm32's products are fixed chains over K that
    do not depend on M or on the batch, and nothing per query crosses a chunk or a group: out, d Wq, d thr and d bias are the same
    bits.  d X and d V (d b2) are summed over the chunks in another order: the value tolerance."""
    from dagl_amd import ops
    B, H, W, L, N = _geom(name)
    (wq, xr, b2, thr, bias, G), _ = case_inputs(name)
    d = [t.to(_dev()) for t in (wq, xr, b2, thr, bias)]
    one = ops.dense_plan(B, H, W)
    assert one["n_chunks"] == 1 and one["Bc"] == B
    out1, saved = ops.ce_core_dense_forward(*d, exact=True)
    g1 = dict(zip(GRADS, ops.ce_core_dense_backward(G.to(_dev()), *d, saved, exact=True)))
    out2, g2, info = run_case(name, exact=True)
    assert torch.equal(out1, out2)
    for n in ("d_wq", "d_thr", "d_bias"):
        assert torch.equal(g1[n], g2[n]), n
    check_values(name, out1, g1, saved["info"], "exact, built-in budget")
    check_values(name, out2, g2, info, "exact, small budget")
    if CASES[name]["plan"]["n_chunks"] == 1:               # groups only: no sum changes its order
        assert torch.equal(g1["d_x"], g2["d_x"]) and torch.equal(g1["d_b2"], g2["d_b2"])


@pytest.mark.parametrize("name", ["chunks3", "groups221", "wide_topk100_chunks3", "wide_topk200_groups"])
def test_two_calls_under_the_same_budget_give_the_same_bits(name):
    out1, g1, _ = run_case(name)
    out2, g2, _ = run_case(name)
    assert torch.equal(out1, out2)
    for n in GRADS:
        assert (g1[n] is None and g2[n] is None) or torch.equal(g1[n], g2[n]), n
