"""``CE.forward_with_graph``: a block's output and the patch graph that produced it from one call -- the list-form route of the
differentiable forward, its neighbour lists turned into CSR by ``ops.graph_from_lists`` (csrc/graph_lists.hip).

The graph is held to the export's own checks (``check_structure`` / ``check_edges`` / ``check_values`` of graph_reference.py: the
band TAU = 2e-5, the caps on its share, the 3 e_32 + 1e-6 bound, all unchanged) on the fp32 route, the output to the bits of the
module's own differentiable forward and, under the project's gap rule, to the inference forward; the graph must reproduce the output
through ``apply_graph`` and ``forward_on_graph``.  The cases are those whose fp64 oracle degrees fit the lists (<= 64 keys per query)."""
import pytest
import torch

from tests.graph_reference import (COMBOS, S0, S1, TOPK8, _cid, _gap, _mod, _module, _oracle, _refused, ambiguity, check_edges,
                                  check_structure, check_values, membership)
from tests.helpers import normwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_COMBOS = [COMBOS[0], COMBOS[9]]                  # (2,24,20): top-k 8 and the adaptive case
FEATURES = ("split16", "fp32")
SCAN_OF = {"split16": "screened", "fp32": "exact"}


def _arrays(g):
    return (g.row_off, g.key, g.weight) + ((g.score,) if g.score is not None else ())


def _nw(a, b):
    return normwise(a.double().cpu().numpy(), b.double().cpu().numpy())


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_graph_against_the_fp64_oracle(combo):
    """Check 1: on the fp32 route the graph is the export's graph up to summation order -- the export's own checks, unchanged."""
    shape, (variant, gain, mode, k), seed = combo
    ce, x = _mod(combo)
    with torch.no_grad():
        out, g_dev = ce.forward_with_graph(x, scores=True, features="fp32")
    assert out.shape == (shape[0], 16, shape[1], shape[2]) and out.dtype == torch.float32
    assert (g_dev.B, g_dev.H, g_dev.W, g_dev.mode, g_dev.k) == (*shape, mode, min(k, shape[1] * shape[2]) if mode != "adaptive" else 0)
    assert g_dev._valid and not g_dev.weight.requires_grad
    g = g_dev.cpu()
    check_structure(g, mode, k, variant)
    if mode == "topk":
        assert bool((g.degrees() == min(k, g.N)).all())
    st64 = _oracle(seed, shape, variant, gain, mode, k)
    mem, rows, rank_rows = check_edges(g, st64, mode, k)
    st32 = _oracle(seed, shape, variant, gain, mode, k, torch.float32)
    check_values(g, mem, rows, rank_rows, st64, st32, mode, f"forward_with_graph fp32 seed {seed} {shape} {combo[1]}")


@pytest.mark.parametrize("features", FEATURES)
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_bits_of_the_differentiable_forward(combo, features):
    """Check 2: ``out`` is, bit for bit, what the module's own differentiable forward returns (a fresh module in train(), the input
    requiring grad, ``scan`` set to match); at (2,24,20) also the gradients of the input and of every parameter."""
    ref_ce, x = _mod(combo)
    ref_ce.train()
    ref_ce.scan = SCAN_OF[features]
    xr = x.clone().requires_grad_(True)
    want = ref_ce(xr)
    ce, _ = _mod(combo)
    xg = x.clone().requires_grad_(True)
    out, g = ce.forward_with_graph(xg, features=features)
    assert out.requires_grad and not g.weight.requires_grad and g.score is None
    assert torch.equal(out, want)
    if combo not in GRAD_COMBOS:
        return
    d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    names = [n for n, _ in ce.named_parameters()]
    got = torch.autograd.grad(out, [xg] + [p for _, p in ce.named_parameters()], d_out, allow_unused=True)
    ref = torch.autograd.grad(want, [xr] + [p for _, p in ref_ce.named_parameters()], d_out, allow_unused=True)
    used = 0
    for n, a, b in zip(["input"] + names, got, ref):
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(a, b), n
            used += 1
    mode = combo[1][2]
    assert used == (1 + 8 if mode == "topk" else 1 + 12) and got[0] is not None     # g, theta, fc1, fc2 (+ the two heads): weight and bias


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_output_graph_and_inference_forward(combo):
    """Checks 3 - 5: ``out`` against the inference forward under the gap rule; the graph reproduces ``out`` through ``apply_graph``
    (structure fixed: 1e-4) and ``forward_on_graph`` (gap rule); the two feature routes' graphs compared pair by pair (printed)."""
    shape, (variant, gain, mode, k), seed = combo
    B, H, W = shape
    ce, x = _mod(combo)
    st64 = _oracle(seed, shape, variant, gain, mode, k)
    gap = _gap(st64, mode, k, H, W)
    bound = 1e-4 if gap >= 1e-6 else 1e-3
    res = {}
    with torch.no_grad():
        for f in FEATURES:
            res[f] = ce.forward_with_graph(x, scores=True, features=f)
        for scan in ("screened", "exact"):
            ce.scan = scan
            ce.invalidate_packed()
            infer = ce(x)
            for f in FEATURES:
                err = _nw(res[f][0], infer)
                print(f"[fwg] {_cid(combo)} out[{f}] vs forward(scan={scan}): {err:.2e} (bound {bound:.0e}, gap {gap:.1e})")
                assert err <= bound, (f, scan, err)
        for f in FEATURES:
            out, g = res[f]
            e_apply = _nw(ce.apply_graph(x, g), out)
            e_on = _nw(ce.forward_on_graph(x, g, features=f), out)
            print(f"[fwg] {_cid(combo)} [{f}] edges {g.n_edges}: apply_graph vs out {e_apply:.2e} (bound 1e-04), forward_on_graph vs out "
                  f"{e_on:.2e} (bound {bound:.0e})")
            assert e_apply <= 1e-4, (f, e_apply)
            assert e_on <= bound, (f, e_on)
    # check 5 (nothing asserted: the band of the split-fp16 features has not been measured)
    m16, _ = membership(res["split16"][1].cpu())
    m32, _ = membership(res["fp32"][1].cpu())
    thr_amb, rank_amb = ambiguity(st64, mode, k)
    diff = m16 != m32
    print(f"[fwg] {_cid(combo)} split16 vs fp32 structure: {int(diff.sum())} pairs differ of {diff.numel()}, "
          f"{int((diff & (thr_amb | rank_amb)).sum())} of them inside the oracle's band")


@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[6], COMBOS[9]], ids=_cid)
def test_state_and_determinism(combo):
    """Check 6."""
    mode = combo[1][2]
    ce, x = _mod(combo)
    with torch.no_grad():
        before = ce(x).clone()
        tight = ce.topk_policy_is_tight() if mode != "adaptive" else None
        state = (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call)
        for f in (None,) + FEATURES:
            out, g = ce.forward_with_graph(x, scores=True, features=f)
            out2, g2 = ce.forward_with_graph(x, scores=True, features=f)
            assert torch.equal(out, out2)
            assert len(_arrays(g)) == 4 and all(torch.equal(a, b) for a, b in zip(_arrays(g), _arrays(g2)))
            assert ce.forward_with_graph(x, features=f)[1].score is None
            if f is None:                             # scan = "screened": the default route is split16
                o16, g16 = ce.forward_with_graph(x, scores=True, features="split16")
                assert torch.equal(out, o16) and all(torch.equal(a, b) for a, b in zip(_arrays(g), _arrays(g16)))
        assert (ce.last_info, ce.scan, ce.topk_threshold, ce._train_dense, ce._pack_key, ce._pack_epoch, ce._last_call) == state
        assert torch.equal(ce(x), before)
        if tight is not None:
            assert ce.topk_policy_is_tight() == tight
        ce.scan = "exact"                             # ... and "fp32" is the default route of an exact module
        ce.invalidate_packed()
        o_def, g_def = ce.forward_with_graph(x, scores=True)
        o32, g32 = ce.forward_with_graph(x, scores=True, features="fp32")
        assert torch.equal(o_def, o32) and all(torch.equal(a, b) for a, b in zip(_arrays(g_def), _arrays(g32)))


@pytest.mark.parametrize("case", [TOPK8, ("sparse", 1.65, "adaptive", 0)], ids=lambda c: "-".join(map(str, c)))
def test_softmax_scale_other_than_10(case):
    """``softmax_scale = 40`` (the factor of ``_scale_c`` is a power of two): the oracle's edges and weights at that scale, and ``score``
    is S itself again."""
    shape = (2, 24, 20)
    variant, gain, mode, k = case
    ce, x = _module(12, shape, variant, gain, mode, k, scale=40)
    with torch.no_grad():
        g = ce.forward_with_graph(x, scores=True, features="fp32")[1].cpu()
    check_structure(g, mode, k, variant)
    st64 = _oracle(12, shape, variant, gain, mode, k, torch.float64, 64, 40.0)
    st32 = _oracle(12, shape, variant, gain, mode, k, torch.float32, 64, 40.0)
    mem, rows, rank_rows = check_edges(g, st64, mode, k)
    check_values(g, mem, rows, rank_rows, st64, st32, mode, f"forward_with_graph softmax_scale 40 {case}")


def test_refusals_leave_the_module_alone():
    """Check 7."""
    ce, x = _mod(COMBOS[0])
    _refused(ce, x, lambda: ce.forward_with_graph(x.cpu()), "GPU")
    _refused(ce, x, lambda: ce.forward_with_graph(x[:, :32].contiguous()), "expected [B,64,H,W]")
    _refused(ce, x, lambda: ce.forward_with_graph(x, features="fp16"), "features")
    _refused(ce, x, lambda: ce.forward_with_graph(x.double()), "dtype")

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _ = x + 1.0
            ce.forward_with_graph(x)
    _refused(ce, x, captured, "captur")
    torch.cuda.synchronize()
    with torch.no_grad():
        assert ce.forward_with_graph(x)[1].n_edges == 2 * 30 * 8          # and it still works afterwards


def test_refusal_of_wide_and_dense_neighbourhoods():
    from dagl_amd import DaglError
    from dagl_amd._lib import ERR_UNSUPPORTED
    # k = 100: no neighbour lists of that width
    ce, x = _module(11, S0, "default", 2.0, "topk", 100)
    assert "CE.graph" in _refused(ce, x, lambda: ce.forward_with_graph(x), "CE.graph")
    # an adaptive mask that keeps 209 keys for some query (the fp64 oracle's largest degree): found by the core
    ce, x = _module(13, S1, "sparse", 1.65, "adaptive", 0)
    for f in FEATURES:
        with torch.no_grad(), pytest.raises(DaglError) as err:
            ce.forward_with_graph(x, features=f)
        assert err.value.code == ERR_UNSUPPORTED and "CE.graph" in str(err.value), str(err.value)
    _refused(ce, x, lambda: ce.forward_with_graph(x), "CE.graph")


def test_refusal_of_a_generic_geometry():
    from dagl_amd.ce import CE
    torch.manual_seed(5)
    ce = CE(ksize=5, stride_1=2, stride_2=1, inter_channels=16, in_channels=64).to(DEV).eval()
    x = torch.randn(1, 64, 20, 24, device=DEV)
    _refused(ce, x, lambda: ce.forward_with_graph(x), "scope")


def test_half_module():
    """Check 8 and the last refusal of check 7: a .half() module runs on the fp32 copies of its weights under ``torch.no_grad()`` and
    hands ``out`` back in the input's dtype; with a gradient wanted it is refused."""
    ce, x = _mod(COMBOS[0], half=True)
    assert x.dtype == torch.float16
    _refused(ce, x, lambda: ce.forward_with_graph(x), "fp32 parameters")
    with torch.no_grad():
        out, g = ce.forward_with_graph(x, scores=True)
        ref = ce(x)
    assert out.dtype == torch.float16 and g.weight.dtype == torch.float32 and g.score.dtype == torch.float32
    check_structure(g.cpu(), "topk", 8, "default")
    # both sides are fp32 results within 1e-4 of each other (the rule of check 3), each rounded to half: half an ulp, 2^-11, a side
    err = _nw(out, ref)
    print(f"[fwg] half module: out vs forward {err:.2e}")
    assert err <= 1e-4 + 2.0 ** -10
