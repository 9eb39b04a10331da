"""``CES.forward_on_graphs(fused=True)`` / ``RR.forward_on_graphs(fused=True)``: one ``ops.graph_stage_forward`` per stage, under
autograd ``ce._GraphStageForward`` (``ops.ces_stage_mix_backward`` + one ``ops.graph_forward_backward`` on the stacked operands).

Modelled on Test G of test_gpu_train_on_graph.py: the same module, input, fp64 reference (the module's wiring on the CPU with the dense
formula on the given structure in the place of each head) and bounds -- 1e-4 normwise against ``forward_with_graphs`` on its own state
(the structures are given, nothing is selected again), ``e_lib <= 3 e_32 + 1e-4`` for gradients.  ``features="stage16"`` is held, bit for
bit, to ``ops.graph_stage_forward`` on ``ops.graph_stage_features16``'s operands (the wiring) and, against fp64, to the 1e-3 normwise
that test_gpu_stage_features.py applies to that feature route's output."""
import copy
import functools

import pytest
import torch

from tests.graph_reference import CASES, _check, _geom
from tests.helpers import normwise
from tests.test_gpu_ces_step_graphs import _assert_state, _build, _key_state, _module_state
from tests.test_gpu_train_on_graph import CES_SHAPE, _CES_GRADS, _build_ces, _ces_reference, _member

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = _CES_GRADS + ("c2_c.bias",)


def _nw(a, b):
    return normwise(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _setup():
    """(ces, x, forward_with_graphs' output, its state): built once; the tests leave parameters and state as they are."""
    ces, x = _build_ces()
    with torch.no_grad():
        want, state = ces.forward_with_graphs(x)
    for g in state.stages:
        g.validate()
    return ces, x, want, state


@functools.lru_cache(maxsize=None)
def _reference():
    """(d_out, the output in fp64, [fp64 gradients], [fp32 gradients]) of x and GRADS on the CPU: computed once, read-only."""
    ces, x, _, state = _setup()
    B, H, W, L, N = _geom(CES_SHAPE)
    members = [_member(state.head(s, h).cpu()) for s in range(3) for h in range(4)]
    d_out = torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(9))
    refs, out64 = [], None
    torch.set_num_threads(16)
    for dt in (torch.float64, torch.float32):
        xl = x.detach().cpu().to(dt).requires_grad_(True)
        pl = {n: t.detach().cpu().to(dt).requires_grad_(True) for n, t in ces.state_dict().items()}
        out = _ces_reference(xl, pl, members, CES_SHAPE)
        (out * d_out.to(dt)).sum().backward()
        refs.append([xl.grad] + [pl[n].grad for n in GRADS])
        out64 = out.detach() if dt == torch.float64 else out64
    return d_out, out64, refs[0], refs[1]


@pytest.mark.parametrize("features", ["fp32", "split16"])
def test_no_grad_against_forward_with_graphs(features):
    ces, x, want, state = _setup()
    before = _module_state(ces)
    with torch.no_grad():
        out = ces.forward_on_graphs(x, state, fused=True, features=features)
        again = ces.forward_on_graphs(x, state, fused=True, features=features, backward="fused")
        by_head = ces.forward_on_graphs(x, state, features=features)
    err = _nw(out, want)
    print(f"[frozen fused] CES.forward_on_graphs(fused=True, {features}, no grad) vs forward_with_graphs: {err:.2e}; vs head by head "
          f"{_nw(out, by_head):.2e}")
    assert out.shape == x.shape and not out.requires_grad and err <= 1e-4
    assert torch.equal(again, out)
    _assert_state(ces, before)


def test_no_grad_two_images():
    """B = 2, where head-major differs from batch-major: the second image is the first one rolled."""
    ces, x, _, _ = _setup()
    x2 = torch.cat([x, torch.roll(x, (3, 5), (2, 3))]).contiguous()
    with torch.no_grad():
        want, state = ces.forward_with_graphs(x2)
        for features in ("fp32", "split16", "stage16"):
            out = ces.forward_on_graphs(x2, state, fused=True, features=features)
            err = _nw(out, want)
            print(f"[frozen fused] B=2 {features} vs forward_with_graphs: {err:.2e}")
            assert out.shape == x2.shape and err <= (1e-3 if features == "stage16" else 1e-4)


def test_stage16_wiring_and_values():
    from dagl_amd import ops
    ces, x, want, state = _setup()
    before = _module_state(ces)
    with torch.no_grad():
        whole = ces.forward_on_graphs(x, state, fused=True, features="stage16")
        inp = x
        for s in (1, 2, 3):
            heads, mix = ces._stage_modules(s)
            stage = state.stages[s - 1]
            got = ces._stage_forward_fused(s, inp, stage, False, "stage16")
            wq4, x4, b2p4, tau4 = ops.graph_stage_features16(inp, [hd._params_f32(scaled=False) for hd in heads], False)
            assert tau4 is None
            by_hand = ops.graph_stage_forward(wq4, x4, b2p4, stage.row_off, stage.key, inp, mix.weight.detach().contiguous(),
                                              mix.bias.detach().contiguous(), scale=10.0)
            assert torch.equal(got, by_hand), s
            inp = ces._between_stages(s, got).contiguous()
        assert torch.equal(whole, inp)
    out64 = _reference()[1]
    err = _nw(whole, out64)
    print(f"[frozen fused] stage16 vs fp64 reference: {err:.2e} (bound 1e-3); vs forward_with_graphs {_nw(whole, want):.2e}")
    assert bool(torch.isfinite(whole).all()) and err <= 1e-3
    _assert_state(ces, before)


@pytest.mark.parametrize("features", ["fp32", "split16"])
def test_under_autograd(features):
    ces, x, want, state = _setup()
    d_out, _, ref64, ref32 = _reference()
    own = dict(ces.named_parameters())
    with torch.no_grad():
        plain = ces.forward_on_graphs(x, state, fused=True, features=features)
    grads = []
    for _ in range(2):
        ces.zero_grad(set_to_none=True)
        xg = x.detach().clone().requires_grad_(True)
        out = ces.forward_on_graphs(xg, state, fused=True, features=features, backward="fused")
        assert out.requires_grad and torch.equal(out.detach(), plain)
        (out * d_out.to(DEV)).sum().backward()
        grads.append([xg.grad.clone()] + [own[n].grad.clone() for n in GRADS])
    for name, lib, r64, r32 in zip(("x",) + GRADS, grads[0], ref64, ref32):
        _check(f"CES fused=True d {name} {features}", lib, r64, r32, slack=1e-4)
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            assert hd.fc1[0].weight.grad is not None and bool(torch.isfinite(hd.fc1[0].weight.grad).all())
    assert all(torch.equal(a, b) for a, b in zip(*grads))                    # the same operands, the same bits
    ces.zero_grad(set_to_none=True)


def test_adaptive_heads():
    """``CASES[1]``: the adaptive rule, so the margin (``tau4``) and the two head convolutions take part.  Its masks keep up to 129
    keys per query here, more than the neighbour lists of ``forward_with_graphs`` hold (it refuses them), so the state comes from the
    heads' ``CE.graph`` (``_key_state``) and the yardstick of the 1e-4 bound is the frozen-graph call's own definition on that state:
    head by head on the same features, from which the fused form differs by the roundings of the mix product alone."""
    _, ces, x = _build(CASES[1], shape=CES_SHAPE)
    state = _key_state(ces, x)
    assert max(g.max_degree() for g in state.stages) > 8
    with torch.no_grad():
        for features in ("fp32", "split16"):
            want = ces.forward_on_graphs(x, state, features=features)
            out = ces.forward_on_graphs(x, state, fused=True, features=features)
            err = _nw(out, want)
            print(f"[frozen fused] adaptive heads {features} vs head by head on the same state: {err:.2e}")
            assert bool(torch.isfinite(out).all()) and err <= 1e-4
    out = ces.forward_on_graphs(x, state, fused=True, backward="fused")
    assert out.requires_grad
    out.square().sum().backward()
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            for conv in (hd.thr_conv, hd.bias_conv):
                assert conv.weight.grad is not None and bool(torch.isfinite(conv.weight.grad).all())
                assert conv.bias.grad is not None and bool(torch.isfinite(conv.bias.grad).all())
    assert any(bool(hd.thr_conv.weight.grad.any()) for hd in ces._stage_modules(1)[0])


def test_a_tripped_range_word():
    """``features="split16"``: an operand outside the split-fp16 range NaN-fills the stage's output, hence the module's -- tripped as
    test_gpu_stage_features.py's ``test_range`` trips the word: a non-finite input, and one head's fc2 weight past the range."""
    ces, x, _, state = _setup()
    bad = x.clone()
    bad[0, 3, 2, 5] = float("inf")
    with torch.no_grad():
        assert bool(torch.isnan(ces.forward_on_graphs(bad, state, fused=True, features="split16")).all())
        first = ces._stage_forward_fused(1, bad, state.stages[0], False, "split16")
        assert bool(torch.isnan(first).all())
        hot = copy.deepcopy(ces)
        hot.c1_3.fc2[0].weight.data[7, 300] = 70.0                               # |w_fc| < 64 is the per-head kernels' range
        first = hot._stage_forward_fused(1, x, state.stages[0], False, "split16")
        assert bool(torch.isnan(first).all())
        assert bool(torch.isnan(hot.forward_on_graphs(x, state, fused=True, features="split16")).all())
        assert bool(torch.isfinite(hot.forward_on_graphs(x, state, fused=True, features="fp32")).all())
        assert bool(torch.isfinite(ces.forward_on_graphs(x, state, fused=True, features="split16")).all())


def test_rr_trains_on_the_fused_form():
    from dagl_amd.net import RR, seeded_state_dict
    torch.manual_seed(3)
    rr = RR(n_resblocks=2)
    rr.load_state_dict(seeded_state_dict(rr.state_dict(), 22))
    ces = rr.body[1]
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode, hd.select_k, hd.scan = "topk", 8, "exact"
    rr = rr.to(DEV).eval()
    x = torch.randn(1, 1, 24, 20, generator=torch.Generator().manual_seed(17)).to(DEV)
    with torch.no_grad():
        want, state = rr.forward_with_graphs(x)
    out = rr.forward_on_graphs(x, state, fused=True, backward="fused")
    assert out.requires_grad and out.shape == x.shape
    err = _nw(out, want)
    print(f"[frozen fused] RR.forward_on_graphs(fused=True) vs forward_with_graphs: {err:.2e}")
    assert err <= 1e-4
    out.square().sum().backward()
    for s in (1, 2, 3):
        heads, mix = ces._stage_modules(s)
        for hd in heads:
            assert hd.fc1[0].weight.grad is not None and bool(torch.isfinite(hd.fc1[0].weight.grad).all())
        assert mix.weight.grad is not None and bool(torch.isfinite(mix.weight.grad).all()) and bool(mix.weight.grad.any())
    assert rr.head[0].weight.grad is not None


def test_capture():
    """After ``validate()`` the no-grad ``fused=True, features="stage16"`` call reads nothing on the host: one HIP graph, captured on a
    single stream after an eager warm-up, replayed on a second frame with the eager call's bits."""
    ces, x0, _, state = _setup()
    frames = [torch.roll(x0, (s, s), (2, 3)).contiguous() for s in (1, 2)]
    call = lambda x: ces.forward_on_graphs(x, state, fused=True, features="stage16")
    with torch.no_grad():
        eager = [call(f).clone() for f in frames]                                  # (the warm-up: the workspaces have their sizes)
        x = frames[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert torch.cuda.is_current_stream_capturing()
            out = call(x)
        assert not torch.cuda.is_current_stream_capturing()
        for frame, want in zip(frames, eager):
            x.copy_(frame)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)


def test_refusals_leave_the_module_alone():
    from dagl_amd import DaglError
    from dagl_amd.ce import CE
    ces, x, _, state = _setup()
    before = _module_state(ces)
    grad_x = lambda: x.clone().requires_grad_(True)

    def refused(call, word):
        with pytest.raises(DaglError) as err:
            call()
        assert word in str(err.value), str(err.value)
        _assert_state(ces, before)
    refused(lambda: ces.forward_on_graphs(x, state, fused="stage"), "fixed-width forms")
    refused(lambda: ces.forward_on_graphs(x, state, fused=1), "expected None, False or True")
    for fused in (None, False, True, "stage"):
        refused(lambda: ces.forward_on_graphs(x, state.to_fixed(8), fused=fused), "to_csr()")
    refused(lambda: ces.forward_on_graphs(grad_x(), state, fused=True), "contradicts")
    refused(lambda: ces.forward_on_graphs(grad_x(), state, fused=True, backward="two_ops"), "backward='fused'")
    refused(lambda: ces.forward_on_graphs(grad_x(), state, fused=True, features="stage16", backward="fused"), "has no backward")
    refused(lambda: ces.forward_on_graphs(x, state, features="stage16"), "stage-fused forms")
    refused(lambda: ces.forward_on_graphs(x, state, features="stage16", fused=False), "stage-fused forms")
    refused(lambda: ces.forward_on_graphs(x, state, fused=True, features="fp16"), "features=")
    refused(lambda: ces.forward_on_graphs(x, state, fused=True, backward="both"), "backward=")
    refused(lambda: ces.forward_on_graphs(x[:, :, :20], state, fused=True), "the state was built for B=1 H=24 W=20")
    with torch.no_grad():
        refused(lambda: ces.forward_on_graphs(x.double(), state, fused=True), "stage 1 does not qualify: the input is torch.float64")
    # a stage whose heads disagree: named with its reason; a head in half precision under autograd
    other = copy.deepcopy(ces)
    other.c2_3.select_k = 9
    with torch.no_grad():
        with pytest.raises(DaglError, match="stage 2 does not qualify: its heads do not share select_mode, select_k and softmax_scale"):
            other.forward_on_graphs(x, state, fused=True)
    other.c2_3.select_k = 8
    other.c1_1.half()
    with pytest.raises(DaglError) as err:
        other.forward_on_graphs(grad_x(), state, fused=True, backward="fused")
    assert str(err.value) == CE._FP32_ONLY
    # the defaults still run head by head and keep their bits
    with torch.no_grad():
        assert torch.equal(ces.forward_on_graphs(x, state, fused=False), ces.forward_on_graphs(x, state))
    _assert_state(ces, before)
