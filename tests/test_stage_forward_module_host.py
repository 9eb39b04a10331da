"""``CES.forward_on_graphs(fused=...)`` / ``RR.forward_on_graphs`` (dagl_amd/net.py) where no device is needed, ``ops`` monkeypatched as
in test_stage_features_module_host.py: every refusal of the keyword is raised before any ``ops`` call, ``fused=None`` / ``False`` reach
exactly the calls they reached before the keyword, and ``fused=True`` makes one ``ops.graph_stage_forward`` per stage on head-major
operands and the stage's own ``row_off`` / ``key`` objects."""
import pytest
import torch

SHAPE = (1, 8, 8)
L, N = 4, 64


@pytest.fixture()
def ces():
    from dagl_amd.net import CES
    torch.manual_seed(0)
    ces = CES(64).eval()
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode, hd.select_k = "topk", 8
    return ces


@pytest.fixture()
def no_launch(monkeypatch):
    """Every launch of the stage-fused and the head-by-head routes raises: a refusal that comes later than it should shows."""
    from dagl_amd import ops
    from dagl_amd.ce import CE

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")
    for name in ("graph_stage_features16", "graph_stage_forward", "ces_stage_mix_backward", "graph_forward", "graph_forward_train",
                 "graph_forward_backward", "graph_attend", "graph_apply"):
        monkeypatch.setattr(ops, name, boom)
    for name in ("_graph_features", "forward_on_graph"):
        monkeypatch.setattr(CE, name, boom)


def _states():
    from dagl_amd.sequence import SequenceState
    csr = SequenceState.start(*SHAPE, "cpu", "topk")
    return csr, csr.to_fixed(8)


def _x():
    return torch.zeros(SHAPE[0], 64, *SHAPE[1:])


def _qualifies(monkeypatch, seen=None):
    """A stage that qualifies without a device: ``_stage_step_fusable`` says yes, the heads' own checks are recorded."""
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    monkeypatch.setattr(CES, "_stage_step_fusable", lambda self, s, x: True)
    monkeypatch.setattr(CE, "_attend_arguments", lambda self, b, g, what, margin, normalize, apply, features, fused, backward:
                        (seen.append((what, margin, normalize, apply, features, fused, backward, g.B)) if seen is not None else None)
                        or (self.select_mode != "topk", features == "split16", False, False, False))


def test_the_value_of_fused(ces, no_launch):
    from dagl_amd._lib import DaglError
    csr, _ = _states()
    with pytest.raises(DaglError, match="fused='stage' names the fixed-width forms"):
        ces.forward_on_graphs(_x(), csr, fused="stage")
    for bad in (1, 0, "yes", "fused", 2.0, ()):
        with pytest.raises(DaglError, match="expected None, False or True"):
            ces.forward_on_graphs(_x(), csr, fused=bad)


def test_a_fixed_state_keeps_its_refusal(ces, no_launch):
    from dagl_amd._lib import DaglError
    _, fixed = _states()
    for fused in (None, False, True, "stage"):
        for features in ("fp32", "stage16"):
            with pytest.raises(DaglError, match=r"to_csr\(\)") as e:
                ces.forward_on_graphs(_x(), fixed, fused=fused, features=features)
            assert "FixedGraph" in str(e.value)


def test_a_stage_that_does_not_qualify(ces, no_launch, monkeypatch):
    from dagl_amd._lib import DaglError
    from dagl_amd.net import CES
    csr, _ = _states()
    with torch.no_grad():
        with pytest.raises(DaglError, match=r"fused=True, but stage 1 does not qualify: the input is not on the GPU"):
            ces.forward_on_graphs(_x(), csr, fused=True)
        with pytest.raises(DaglError, match=r"stage 1 does not qualify: the input is not on the GPU"):
            ces.forward_on_graphs(_x(), csr, fused=True, features="stage16")
        # the stage and the reason are named: the second stage's heads disagree on k
        monkeypatch.setattr(CES, "_stage_step_fusable", lambda self, s, x: s != 2)
        ces.c2_3.select_k = 9
        with pytest.raises(DaglError, match=r"stage 2 does not qualify: its heads do not share select_mode, select_k and softmax_scale"):
            ces.forward_on_graphs(_x(), csr, fused=True)
    assert ces._why_not_fusable(1, _x().double()) == "the input is not on the GPU"
    ces.fuse_stage = False
    assert "64 channels" in ces._why_not_fusable(1, _x())


def test_refusals_that_depend_on_a_gradient(ces, no_launch, monkeypatch):
    from dagl_amd._lib import DaglError
    from dagl_amd.ce import CE
    csr, _ = _states()
    _qualifies(monkeypatch)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in ces.parameters())
    for features in ("fp32", "split16", "stage16"):
        with pytest.raises(DaglError, match="fused=True contradicts backward='two_ops'.*backward='fused'"):
            ces.forward_on_graphs(_x(), csr, fused=True, features=features)
    with pytest.raises(DaglError, match="features='stage16' has no backward.*per-head form"):
        ces.forward_on_graphs(_x(), csr, fused=True, features="stage16", backward="fused")
    # ... also when the input alone asks for a gradient
    for p in ces.parameters():
        p.requires_grad_(False)
    with pytest.raises(DaglError, match="contradicts"):
        ces.forward_on_graphs(_x().requires_grad_(True), csr, fused=True)
    with pytest.raises(DaglError, match="has no backward"):
        ces.forward_on_graphs(_x().requires_grad_(True), csr, fused=True, features="stage16", backward="fused")
    # non-fp32 parameters under autograd
    half = ces.half()
    with pytest.raises(DaglError) as e:
        half.forward_on_graphs(_x().requires_grad_(True), csr, fused=True, backward="fused")
    assert str(e.value) == CE._FP32_ONLY


def test_stage16_belongs_to_fused_true(ces, no_launch):
    from dagl_amd._lib import DaglError
    csr, _ = _states()
    named = r"features='stage16'.*stage-fused forms.*'split16' or 'fp32'"
    for fused in (None, False):
        with pytest.raises(DaglError, match=named) as e:
            ces.forward_on_graphs(_x(), csr, features="stage16", fused=fused)
        assert "head by head" in str(e.value)
    with torch.no_grad():
        with pytest.raises(DaglError, match=named):
            ces.forward_on_graphs(_x(), csr, features="stage16")


def test_unknown_features_and_backward(ces, no_launch, monkeypatch):
    from dagl_amd._lib import DaglError
    csr, _ = _states()
    _qualifies(monkeypatch)
    with torch.no_grad():
        with pytest.raises(DaglError, match="features='fp16'"):
            ces.forward_on_graphs(_x(), csr, fused=True, features="fp16")
        with pytest.raises(DaglError, match="backward='both'"):
            ces.forward_on_graphs(_x(), csr, fused=True, backward="both")


def test_rr_hands_the_keyword_through(no_launch):
    from dagl_amd._lib import DaglError
    from dagl_amd.net import RR
    torch.manual_seed(0)
    rr = RR(n_resblocks=2).eval()
    x = torch.zeros(SHAPE[0], 1, *SHAPE[1:])
    csr, fixed = _states()
    with torch.no_grad():
        with pytest.raises(DaglError, match="does not qualify"):
            rr.forward_on_graphs(x, csr, fused=True)
        with pytest.raises(DaglError, match="fixed-width forms"):
            rr.forward_on_graphs(x, csr, fused="stage")
        with pytest.raises(DaglError, match=r"to_csr\(\)"):
            rr.forward_on_graphs(x, fixed, fused=True)


@pytest.mark.parametrize("fused", [None, False])
def test_head_by_head_reaches_the_calls_it_reached(ces, monkeypatch, fused):
    """The twelve heads' checks with the arguments they always had, then ``CE.forward_on_graph`` twelve times on ``state.head(s, h)``:
    the keyword changes nothing there, and no stage-fused call is made."""
    from dagl_amd import ops
    from dagl_amd.ce import CE
    csr, _ = _states()
    x = _x()
    checks, runs = [], []
    monkeypatch.setattr(ops, "graph_stage_forward", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not this route")))
    monkeypatch.setattr(CE, "_attend_arguments", lambda self, *a: checks.append((self,) + a))

    def run(self, b, graph, **kw):
        runs.append((self, b, graph, kw))
        return torch.full((b.shape[0], 16) + tuple(b.shape[2:]), float(len(runs)))
    monkeypatch.setattr(CE, "forward_on_graph", run)
    heads = [hd for s in (1, 2, 3) for hd in ces._stage_modules(s)[0]]
    graphs = [csr.head(s, h) for s in range(3) for h in range(4)]
    for features, backward in (("fp32", "two_ops"), ("split16", "fused")):
        del checks[:], runs[:]
        with torch.no_grad():
            out = ces.forward_on_graphs(x, csr, features=features, backward=backward, **({} if fused is None else {"fused": fused}))
        assert out.shape == x.shape
        assert len(checks) == 12 and len(runs) == 12
        for c, hd, g in zip(checks, heads, graphs):
            assert c[0] is hd and c[1] is x and c[2] is g and c[3:] == ("forward_on_graph", None, "reference", True, features, None, backward)
        for r, hd, g in zip(runs, heads, graphs):
            assert r[0] is hd and r[2] is g and r[3] == dict(features=features, backward=backward)
        assert runs[0][1] is x and all(r[1] is runs[4 * (i // 4)][1] for i, r in enumerate(runs))        # a stage's heads share its input


def _fake_features(calls, stage16):
    from dagl_amd.net import _StageFeatures
    B, H, W = SHAPE

    def features_of(self, s, x, margin, features, grad=False):
        calls.append((s, x, margin, features, grad))
        g = torch.Generator().manual_seed(s)
        wq4, x4, b2p4 = torch.rand(4, B, L, 196, generator=g), torch.rand(4, B, N, 196, generator=g), torch.rand(4, B, H + 6, W + 6, 16, generator=g)
        tau4 = torch.rand(4, B, L, generator=g) if margin else None
        feats = _StageFeatures((wq4[h].clone(), x4[h].clone(), tau4[h].clone() if margin else None, b2p4[h].clone(), lambda t: t + 1.0)
                               for h in range(4))
        if stage16:
            feats.stacked = (wq4, x4, tau4, b2p4)
            return feats
        return list(feats)
    return features_of


@pytest.mark.parametrize("mode", ["topk", "adaptive"])
@pytest.mark.parametrize("features", ["fp32", "split16", "stage16"])
def test_fused_is_one_stage_forward_per_stage(ces, monkeypatch, features, mode):
    from dagl_amd import ops
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode = mode
    margin = mode != "topk"
    csr, _ = _states()
    x = _x()
    seen, feat_calls, calls = [], [], []
    _qualifies(monkeypatch, seen)
    monkeypatch.setattr(CES, "_stage_features", _fake_features(feat_calls, features == "stage16"))
    monkeypatch.setattr(CE, "forward_on_graph", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not this route")))

    def stage_forward(wq4, x4, b2p4, row_off, key, x_, mix_w, mix_b, **kw):
        calls.append((wq4, x4, b2p4, row_off, key, x_, mix_w, mix_b, kw))
        return torch.full_like(x_, float(len(calls)))
    monkeypatch.setattr(ops, "graph_stage_forward", stage_forward)
    with torch.no_grad():
        out = ces.forward_on_graphs(x, csr, fused=True, features=features, backward="fused")
    assert out.shape == x.shape and not out.requires_grad
    # the heads' checks first, all twelve, with the heads' own name of the route and a graph under a head's shape
    assert len(seen) == 12 and all(c == ("forward_on_graph", None, "reference", True, "fp32" if features == "fp32" else "split16", None,
                                         "fused", SHAPE[0]) for c in seen)
    assert [(c[0], c[2], c[3], c[4]) for c in feat_calls] == [(s, margin, features, False) for s in (1, 2, 3)]
    assert len(calls) == 3 and feat_calls[0][1] is x
    B, H, W = SHAPE
    for s, (wq4, x4, b2p4, row_off, key, x_, mix_w, mix_b, kw), fc in zip((1, 2, 3), calls, feat_calls):
        stage, mix = csr.stages[s - 1], ces._stage_modules(s)[1]
        assert row_off is stage.row_off and key is stage.key                                 # the stage's own CSR, no slice, no copy
        assert x_ is fc[1] or torch.equal(x_, fc[1])
        assert wq4.shape == (4, B, L, 196) and x4.shape == (4, B, N, 196) and b2p4.shape == (4, B, H + 6, W + 6, 16)
        assert mix_w.data_ptr() == mix.weight.data_ptr() and mix_b.data_ptr() == mix.bias.data_ptr()
        assert kw["scale"] == 10.0 and kw["normalize"] == "reference" and kw["workspace"] is ces._ws_frozen[s][0] and not kw.get("train")
        assert (kw["tau4"] is None) == (not margin) and (kw["tau4"] is None or kw["tau4"].shape == (4, B, L))
        # head-major: entry h is head h's operand
        g = torch.Generator().manual_seed(s)
        want = (torch.rand(4, B, L, 196, generator=g), torch.rand(4, B, N, 196, generator=g), torch.rand(4, B, H + 6, W + 6, 16, generator=g))
        assert all(torch.equal(a, b) for a, b in zip((wq4, x4, b2p4), want))
        if margin:
            assert torch.equal(kw["tau4"], torch.rand(4, B, L, generator=g))
    # the verdict of the feature route lands on the stage's output: none on "fp32", one per head on "split16", one per call on "stage16"
    assert float(out.flatten()[0]) == 3.0 + {"fp32": 0.0, "split16": 4.0, "stage16": 1.0}[features]


def test_fused_under_autograd_goes_through_the_op(ces, monkeypatch):
    from dagl_amd import ce as ce_mod, ops
    from dagl_amd.net import CES
    csr, _ = _states()
    x = _x()
    feat_calls, calls = [], []
    _qualifies(monkeypatch)
    monkeypatch.setattr(CES, "_stage_features", _fake_features(feat_calls, False))
    monkeypatch.setattr(ops, "graph_stage_forward", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the op makes this call")))

    class Op:
        @staticmethod
        def apply(wq4, x4, tau4, b2p4, x_, mix_w, mix_b, graph, scale, normalize, ws_f, ws_b, ws_mix):
            calls.append((wq4, x4, tau4, b2p4, x_, mix_w, mix_b, graph, scale, normalize, ws_f, ws_b, ws_mix))
            return x_ + mix_b.view(1, 64, 1, 1)
    monkeypatch.setattr(ce_mod, "_GraphStageForward", Op)
    out = ces.forward_on_graphs(x, csr, fused=True, features="split16", backward="fused")
    assert out.requires_grad and len(calls) == 3
    assert [(c[0], c[2], c[3], c[4]) for c in feat_calls] == [(s, False, "split16", True) for s in (1, 2, 3)]
    for s, c in zip((1, 2, 3), calls):
        mix = ces._stage_modules(s)[1]
        assert c[0].shape == (4, SHAPE[0], L, 196) and c[2] is None
        assert c[5] is mix.weight and c[6] is mix.bias and c[7] is csr.stages[s - 1]                    # the parameters themselves
        assert c[8:10] == (10.0, "reference") and c[10:] == ces._ws_frozen[s]


def test_defaults_did_not_move():
    import inspect
    from dagl_amd.net import CES
    prm = inspect.signature(CES.forward_on_graphs).parameters
    assert prm["fused"].default is None and prm["features"].default == "fp32" and prm["backward"].default == "two_ops"
    assert all(prm[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("fused", "features", "backward"))
