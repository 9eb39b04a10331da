"""``features="stage16"`` in ``CES`` / ``RR`` (dagl_amd/net.py) where no device is needed: the refusals of every head-by-head path, raised
before any launch, the heads' own checks made with "split16", and ``CES._stage_features`` -- "fp32" / "split16" still reach
``CE._graph_features`` head by head, "stage16" makes one ``ops.graph_stage_features16`` call."""
import pytest
import torch

SHAPE = (1, 8, 8)


class _Reached(Exception):
    pass


@pytest.fixture()
def ces():
    from dagl_amd.net import CES
    torch.manual_seed(0)
    ces = CES(64).eval()
    for s in (1, 2, 3):
        for hd in ces._stage_modules(s)[0]:
            hd.select_mode, hd.select_k = "topk", 8
    return ces


@pytest.fixture(autouse=True)
def not_capturing(monkeypatch):
    """(``_plan_step`` asks the runtime whether the stream is being captured; without a device that question has no answer)"""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


@pytest.fixture()
def no_launch(monkeypatch):
    """Every launch of the stage-fused and the head-by-head routes raises: a refusal that comes later than it should shows."""
    from dagl_amd import ops
    from dagl_amd.ce import CE

    def boom(*a, **k):
        raise AssertionError("a launch before the refusal")
    for name in ("graph_stage_features16", "graph_stage_step", "graph_stage_step_fixed", "graph_stage_search", "graph_stage_search_step"):
        monkeypatch.setattr(ops, name, boom)
    for name in ("_graph_features", "step_graph", "refresh_graph"):
        monkeypatch.setattr(CE, name, boom)


def _states():
    from dagl_amd.sequence import SequenceState
    csr = SequenceState.start(*SHAPE, "cpu", "topk")
    return csr, csr.to_fixed(8)


def test_head_by_head_paths_refuse_stage16(ces, no_launch):
    from dagl_amd._lib import DaglError
    x = torch.zeros(SHAPE[0], 64, *SHAPE[1:])
    csr, fixed = _states()
    named = r"features='stage16'.*stage-fused forms.*fused=None or True.*fused='stage'.*'split16' or 'fp32'"
    # a CSR state: a stage that does not qualify (here: no GPU input) under fused=None, and fused=False
    for call in (ces.step_graphs, ces.search_graphs):
        for fused in (None, False):
            with pytest.raises(DaglError, match=named) as e:
                call(x, csr, features="stage16", fused=fused)
            assert "head by head" in str(e.value)
        with pytest.raises(DaglError, match="does not qualify"):                 # fused=True there: the refusal it always had
            call(x, csr, features="stage16", fused=True)
    with pytest.raises(DaglError, match=named):
        ces.build_graphs(x, features="stage16", iters=2)
    # the search keywords of step_graphs run head by head on a CSR state
    with pytest.raises(DaglError, match=named):
        ces.step_graphs(x, csr, features="stage16", propagate=True)
    # a state of FixedGraphs: fused=None / False are head by head
    for fused in (None, False):
        with pytest.raises(DaglError, match=named) as e:
            ces.step_graphs(x, fixed, features="stage16", fused=fused)
        assert "FixedGraphs" in str(e.value)
    with pytest.raises(DaglError, match=named):
        ces.search_graphs(x, fixed, features="stage16", fused=False)
    with pytest.raises(DaglError, match="searched by name"):                     # fused=None there: the refusal it always had
        ces.search_graphs(x, fixed, features="stage16")
    with pytest.raises(DaglError, match="fused=True"):
        ces.step_graphs(x, fixed, features="stage16", fused=True)
    with pytest.raises(DaglError):                                               # fused="stage" without a GPU input: the heads' refusal
        ces.step_graphs(x, fixed, features="stage16", fused="stage")


def test_rr_hands_the_refusal_through(no_launch, monkeypatch):
    from dagl_amd._lib import DaglError
    from dagl_amd.net import RR
    torch.manual_seed(0)
    rr = RR(n_resblocks=2).eval()
    x = torch.zeros(SHAPE[0], 1, *SHAPE[1:])
    csr, fixed = _states()
    with torch.no_grad():
        with pytest.raises(DaglError, match="stage-fused forms"):
            rr.step_graphs(x, csr, features="stage16")
        with pytest.raises(DaglError, match="stage-fused forms"):
            rr.search_graphs(x, fixed, features="stage16", fused=False)
        with pytest.raises(DaglError, match="stage-fused forms"):
            rr.build_graphs(x, features="stage16")


def test_ce_methods_keep_refusing_the_value():
    """No ``CE`` code changed: its checks name their two routes."""
    import inspect
    from dagl_amd.ce import CE
    for name in ("_refresh_arguments", "_fixed_arguments", "_attend_arguments"):
        src = inspect.getsource(getattr(CE, name))
        assert 'features not in ("fp32", "split16")' in src and "stage16" not in src, name
    assert "stage16" not in inspect.getsource(CE)


def test_fused_forms_check_the_heads_with_split16(ces, monkeypatch):
    """A stage that qualifies: the heads' own checks see "split16", ``_stage_features`` sees "stage16"."""
    from dagl_amd.ce import CE
    from dagl_amd.net import CES
    x = torch.zeros(SHAPE[0], 64, *SHAPE[1:])
    csr, fixed = _states()
    seen = []
    monkeypatch.setattr(CES, "_stage_step_fusable", lambda self, s, x: True)
    monkeypatch.setattr(CE, "_refresh_arguments", lambda self, b, g, what, radius, margin, normalize, features, **kw:
                        seen.append(features) or (1, 8, False, 1))
    monkeypatch.setattr(CE, "_fixed_arguments", lambda self, b, g, what, radius, margin, normalize, features, **kw:
                        seen.append(features) or (1, 8, False, 8, False, 0, 0))

    def reached(self, s, x, margin, features):
        seen.append(("stage", s, features))
        raise _Reached()
    monkeypatch.setattr(CES, "_stage_features", reached)
    calls = [lambda: ces.step_graphs(x, csr, features="stage16"), lambda: ces.step_graphs(x, csr, features="stage16", fused=True),
             lambda: ces.search_graphs(x, csr, features="stage16"), lambda: ces.build_graphs(x, features="stage16", iters=2),
             lambda: ces.step_graphs(x, fixed, features="stage16", fused="stage"),
             lambda: ces.search_graphs(x, fixed, features="stage16", fused="stage", iters=2)]
    for call in calls:
        del seen[:]
        with pytest.raises(_Reached):
            call()
        assert seen == ["split16"] * 12 + [("stage", 1, "stage16")], seen
    # the other values travel unchanged
    for feat in ("fp32", "split16"):
        del seen[:]
        with pytest.raises(_Reached):
            ces.step_graphs(x, csr, features=feat)
        assert seen == [feat] * 12 + [("stage", 1, feat)]


def test_stage_features_reaches_the_old_line(ces, monkeypatch):
    from dagl_amd import ops
    from dagl_amd.ce import CE
    x = torch.zeros(SHAPE[0], 64, *SHAPE[1:])
    calls = []
    monkeypatch.setattr(CE, "_graph_features", lambda self, b, margin, fast, grad: calls.append((self, b, margin, fast, grad)) or len(calls))
    monkeypatch.setattr(ops, "graph_stage_features16", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not this route")))
    for feat, fast in (("fp32", False), ("split16", True)):
        for margin in (False, True):
            for s in (1, 2, 3):
                del calls[:]
                got = ces._stage_features(s, x, margin, feat)
                assert got == [1, 2, 3, 4]
                assert [c[0] for c in calls] == ces._stage_modules(s)[0]
                assert all(c[1] is x and c[2] is margin and c[3] is fast and c[4] is False for c in calls)


def test_stage_features_stage16_is_one_call(ces, monkeypatch):
    from dagl_amd import ops
    from dagl_amd.ce import CE
    B, H, W = SHAPE
    L, N = 4, H * W
    x = torch.zeros(B, 64, H, W)
    monkeypatch.setattr(CE, "_graph_features", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not this route")))
    calls = []

    def fake(x_, heads, margin, workspace=None):
        calls.append((x_, heads, margin, workspace))
        g = torch.Generator().manual_seed(len(calls))
        return (torch.rand(4, B, L, 196, generator=g), torch.rand(4, B, N, 196, generator=g), torch.rand(4, B, H + 6, W + 6, 16, generator=g),
                torch.rand(4, B, L, generator=g) if margin else None)
    monkeypatch.setattr(ops, "graph_stage_features16", fake)
    for margin in (False, True):
        for s in (1, 2, 3):
            del calls[:]
            feats = ces._stage_features(s, x, margin, "stage16")
            assert len(calls) == 1 and calls[0][0] is x and calls[0][2] is margin
            assert calls[0][3] is ces._ws_feat[s] and calls[0][3] is not ces._ws_step[s]
            heads = ces._stage_modules(s)[0]
            assert len(calls[0][1]) == 4
            for hd, prm in zip(heads, calls[0][1]):
                assert prm["fc1.0.weight"].data_ptr() == hd.fc1[0].weight.data_ptr() and "thr_conv.weight" in prm
            assert len(feats) == 4
            bases = None
            for h, (wq, xk, tau, b2p, poisoned) in enumerate(feats):
                assert wq.shape == (B, L, 196) and xk.shape == (B, N, 196) and b2p.shape == (B, H + 6, W + 6, 16)
                assert wq.is_contiguous() and xk.is_contiguous() and b2p.is_contiguous()
                assert (tau is None) == (not margin) and (tau is None or (tau.shape == (B, L) and tau.is_contiguous()))
                base = (wq._base, xk._base, b2p._base)
                assert all(t is not None for t in base) and (bases is None or all(a is b for a, b in zip(base, bases)))    # views of ONE array
                bases = base
                assert wq.data_ptr() == base[0].data_ptr() + 4 * h * B * L * 196
                t = torch.ones(3)
                assert torch.equal(poisoned(t), t)
            # the verdict reads the new arrays' first elements: NaN there poisons every head's results
            bases[0].view(-1)[0] = float("nan")
            assert all(bool(torch.isnan(f[4](torch.ones(3))).all()) for f in feats)


def test_defaults_did_not_move():
    import inspect
    from dagl_amd.net import CES
    for name in ("step_graphs", "search_graphs", "build_graphs"):
        assert inspect.signature(getattr(CES, name)).parameters["features"].default == "fp32", name
