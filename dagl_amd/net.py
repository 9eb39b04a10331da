"""The caller of the block and the inference driver around it, restated so that the
HIP block can be exercised the way the reference exercises ``CE``: inside the 3-stage x 4-head ``CES`` module
of the EDSR-style trunk ``RR`` and under the recursive 4-way tiling of ``forward_chop``.

Everything here except ``CE`` and the ResBlocks' PReLU (train_ops.PReLU: torch's backward for it was a sixth of the training
step) is stock PyTorch-ROCm convolutions -- unless the model is converted with ``trunk.convert``, which moves every trunk
convolution (and the ResBlocks as fused two-launch blocks) onto the library.  Module / parameter names and registration order
follow the reference (``RR`` DN_Gray/model/dagl.py:11-54, ``CES`` :74-119, ``ResBlock`` DN_Gray/model/common.py:59-79),
so a reference ``state_dict`` loads strictly.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import trunk
from .ce import CE


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, k, padding=k // 2)       # common.default_conv


class ResBlock(nn.Module):
    """conv3x3 - PReLU - conv3x3 + skip (common.py:59-79, bn=False, res_scale=1)."""

    def __init__(self, n_feats, res_scale=1.0):
        super().__init__()
        from .train_ops import PReLU                      # nn.PReLU() whose fp32 GPU calls run on the HIP library (same state_dict)
        self.body = nn.Sequential(_conv(n_feats, n_feats, 3), PReLU(), _conv(n_feats, n_feats, 3))
        self.res_scale = res_scale

    def forward(self, x):
        c1, act, c2 = self.body
        if trunk.fused_resblock_ok(c1, act, c2):
            return trunk.resblock(x, c1, act, c2, self.res_scale)     # converted (trunk.convert): two launches, own autograd op
        return self.body(x).mul(self.res_scale) + x


class _StageFeatures(list):
    """``CES._stage_features``' per-head list where the operands were made head-major in one piece: ``stacked`` holds the arrays."""
    stacked = None


class CES(nn.Module):
    """Three stages of four patch-graph heads, each stage mixed by a 1x1 conv + residual (dagl.py:74-119)."""

    def __init__(self, in_channels, num=4, ce_cls=CE):
        super().__init__()
        self.RBS1 = nn.Sequential(*[ResBlock(in_channels) for _ in range(num)])
        self.RBS2 = nn.Sequential(*[ResBlock(in_channels) for _ in range(num)])
        for stage in (1, 2, 3):
            for head in (1, 2, 3, 4):
                setattr(self, f"c{stage}_{head}", ce_cls(in_channels=in_channels))
            setattr(self, f"c{stage}_c", nn.Conv2d(in_channels, in_channels, 1, 1, 0))
        self.fuse_stage = in_channels == 64       # stage-level launch set (include/dagl_ce.h: dagl_ces_stage_forward)
        self.last_info = None
        from . import ops
        self._ws = {1: ops.Workspace(), 2: ops.Workspace(), 3: ops.Workspace()}     # one per stage: packed weights persist
        self._ws_step = {1: ops.Workspace(), 2: ops.Workspace(), 3: ops.Workspace()}     # step_graphs' own: _ws keeps its packed weights
        self._ws_feat = {1: ops.Workspace(), 2: ops.Workspace(), 3: ops.Workspace()}     # features="stage16": the stage's feature launches
        # forward_on_graphs(fused=True), per stage: the forward's rows; the graph backward's rows and edges; the mix backward's slots
        self._ws_frozen = {s: (ops.Workspace(), ops.Workspace(), ops.Workspace()) for s in (1, 2, 3)}
        self._pack_key = {1: None, 2: None, 3: None}
        self._skip_fused = {1: 0, 2: 0, 3: 0}     # calls for which a stage stays on the per-head path after it met dense masks
        self._fused_calls = {1: 0, 2: 0, 3: 0}    # fused calls since the stage's range word was last looked at

    def _stage(self, s, x):
        heads = [getattr(self, f"c{s}_{h}") for h in (1, 2, 3, 4)]
        mix = getattr(self, f"c{s}_c")
        from ._lib import MAX_TOPK
        mode = heads[0].select_mode if isinstance(heads[0], CE) else None
        k_eff = 0 if mode in (None, "adaptive") else min(int(heads[0].select_k), x.shape[-2] * x.shape[-1])
        # (an eval() stage fed a constant input under an autograd-enabled test loop counts as "no gradient wanted", like CE)
        no_grad = not torch.is_grad_enabled() or (not self.training and not x.requires_grad)
        # the fused launch set has the default head compiled in: a head with another patch geometry or input width, or a subclass
        # with a forward of its own, goes head by head
        if self.fuse_stage and all(isinstance(hd, CE) and not hd._generic and hd.in_channels == 64 and type(hd).forward is CE.forward
                                   for hd in heads) and x.is_cuda and x.dtype == torch.float32 \
                and no_grad and len({(hd.select_mode, hd.select_k, hd.scan) for hd in heads}) == 1 \
                and heads[0].scan == "screened" and self._skip_fused[s] == 0 and 0 <= k_eff <= MAX_TOPK \
                and all(float(hd.softmax_scale) == 10.0 for hd in heads) \
                and all(p.dtype == torch.float32 for hd in heads for p in hd.parameters()):
            # the four heads share x: one launch set with the heads as a batch dimension + the 1x1 mix + residual
            from . import ops
            prm = [{n: p.detach().contiguous() for n, p in hd.named_parameters() if not n.startswith("W.")} for hd in heads]
            ws = self._ws[s]
            fcs = [prm[h][n] for h in range(4) for n in ("fc1.0.weight", "fc2.0.weight", "g.weight", "theta.weight")]
            wsb = ws.peek(x.device)
            key = (tuple(x.shape), heads[0].select_mode, k_eff, tuple(hd._pack_epoch for hd in heads),
                   tuple((t.data_ptr(), t._version) for t in fcs), wsb.data_ptr() if wsb is not None else 0)
            if key != self._pack_key[s] and (self._pack_key[s] is None or key[4] != self._pack_key[s][4]) \
                    and not torch.cuda.is_current_stream_capturing():
                # new weights are about to be packed as fp16 pairs: beyond |w_conv| < 234 / |w_fc| < 58 (never seen on a trained DAGL) the
                # heads take the fp32 path -- which takes them off the fused launch set -- before their first call (CE._forward_infer)
                wmax = torch.stack([t.abs().max() for t in fcs]).view(4, 4).max(dim=0).values.tolist()
                if not (wmax[0] < 57.0 and wmax[1] < 57.0 and wmax[2] < 230.0 and wmax[3] < 230.0):
                    for hd in heads:
                        hd._note_range_violation("weights beyond the split-fp16 range (|w_conv| < 234, |w_fc| < 58)")
                    return self._stage(s, x)
            # the top-k threshold policy ("auto") lives in the stage workspace and is read by the kernels themselves (CE.topk_threshold)
            thr = heads[0].topk_threshold
            out, info = ops.ces_stage_forward(x.contiguous(), prm, mix.weight.detach().contiguous(),
                                              mix.bias.detach().contiguous(), mode=heads[0].select_mode,
                                              k=k_eff, workspace=ws,
                                              weights_packed=(key == self._pack_key[s]),
                                              tight_topk=(mode != "adaptive" and thr == "full"),
                                              sampled_topk=(mode != "adaptive" and thr == "sparse"))
            self._pack_key[s] = key[:-1] + (ws.peek(x.device).data_ptr(),) if out is not None else None
            self.last_info = info
            violated = False
            if out is not None and mode != "adaptive":
                # the top-k modes never read anything back: look at the stage workspace's (sticky) range word every 64th
                # fused call -- one synchronisation.  A call that left the split-fp16 range has NaN-filled outputs (never
                # wrong numbers); the heads move to scan = "exact" (which takes them off the fused path) and this call is redone
                self._fused_calls[s] += 1
                if self._fused_calls[s] >= 64 and not torch.cuda.is_current_stream_capturing():
                    self._fused_calls[s] = 0
                    verdict = ops.ce_range_check((4 * x.shape[0],) + tuple(x.shape[1:]), mode, k_eff, ws, x.device)
                    if verdict & 3:
                        for hd in heads:
                            hd._note_range_violation("a fused CES stage call left the split-fp16 range (outputs NaN-filled)")
                        self._pack_key[s] = None
                        out, violated = None, True
            if out is not None:
                return out
            if violated:
                return self._stage(s, x)                    # (heads now on scan = "exact": per-head path)
            self._skip_fused[s] = 16                        # dense masks: the heads' own dense path serves the next calls
        elif self._skip_fused[s] > 0:
            self._skip_fused[s] -= 1
        outs = [hd(x) for hd in heads]                      # dense adaptive neighbourhoods / foreign heads
        return mix(torch.cat(outs, dim=1)) + x

    def forward(self, x):
        out = self._stage(1, x)
        out = self.RBS1(out)
        out = self._stage(2, out)
        out = self.RBS2(out)
        return self._stage(3, out)

    # ---- sequences: the key frame selects (forward_with_graphs), every following frame moves the graphs at O(edges) (step_graphs) ------
    def _stage_modules(self, s):
        return [getattr(self, f"c{s}_{h}") for h in (1, 2, 3, 4)], getattr(self, f"c{s}_c")

    def _between_stages(self, s, out):
        return self.RBS1(out) if s == 1 else self.RBS2(out) if s == 2 else out

    def forward_with_graphs(self, x):
        """The key frame of a sequence -> ``(out, SequenceState)``: ``forward``'s structure with every head run by
        ``CE.forward_with_graph`` (its output and the patch graph that produced it), the stage's own mix and residual, ``RBS1`` /
        ``RBS2`` between the stages.  The state holds the twelve graphs, one ``PatchGraph`` over ``4 B`` images per stage.  Scope,
        autograd and refusals are ``CE.forward_with_graph``'s, passed through unchanged; the fused stage launch set of ``forward`` is not
        used, so ``out`` differs from ``forward``'s by that route's roundings."""
        from ._lib import DaglError
        from .sequence import SequenceState
        graphs, out = [], x
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            for hd in heads:
                if not isinstance(hd, CE):
                    raise DaglError(f"CES.forward_with_graphs: head {type(hd).__name__} of stage {s} is not a CE: it exports no graph")
            pairs = [hd.forward_with_graph(out) for hd in heads]
            graphs.extend(g for _, g in pairs)
            out = self._between_stages(s, mix(torch.cat([o for o, _ in pairs], dim=1)) + out)
        return out, SequenceState.from_heads(graphs)

    def _stage_step_fusable(self, s, x) -> bool:
        """Whether ``ops.graph_stage_step`` serves stage ``s`` on the input ``x``: four plain ``CE`` heads of the default patch geometry
        that share the selection rule, the scale and hence the margin, a 64-channel fp32 mix, an fp32 input on the GPU."""
        heads, mix = self._stage_modules(s)
        return self.fuse_stage and all(type(hd) is CE and not hd._generic and hd.in_channels == 64 for hd in heads) \
            and len({(hd.select_mode, int(hd.select_k), float(hd.softmax_scale)) for hd in heads}) == 1 \
            and x.is_cuda and x.dtype == torch.float32 and mix.weight.dtype == torch.float32

    @torch.no_grad()
    def step_graphs(self, x, state, *, radius: int = 1, features: str = "fp32", want_graphs: bool = True, fused=None,
                    propagate: bool = False, explore: int = 0, seed: int = 0):
        """A sequence step of the whole module -> ``(out, SequenceState | None)``: per stage the stage's graphs are moved to the stage's
        input exactly as each head's ``CE.refresh_graph`` moves its own, and the stage's output is ``mix(cat(step outputs)) + input`` with
        each head's step output ``CE.step_graph``'s; ``RBS1`` / ``RBS2`` run between the stages as in ``forward``.  For a sequence:
        ``out, state = ces.forward_with_graphs(frame0)``, then ``out, state = ces.step_graphs(frame, state)``.

        ``fused=False``: head by head -- ``CE.step_graph`` four times, ``torch.cat``, the mix convolution: the definition of the result.
        ``fused=True``: the heads' features from ``CE._graph_features`` (either ``features`` route), then ONE ``ops.graph_stage_step`` per
        stage: the four heads' rows in one CSR, one scan, one copy, fold + mix + residual in one launch.  The graphs are the head-by-head
        ones bit for bit; ``out`` differs by the fp32 roundings of the mix product alone.  ``fused=None``: fused for every stage whose
        four heads are plain ``CE`` modules sharing ``select_mode``, ``select_k``, ``softmax_scale`` (hence the margin) and the default
        patch geometry, on an fp32 GPU input; head by head otherwise.  ``fused=True`` on a stage that does not qualify is refused.

        ``want_graphs=False`` keeps the key frame's structure and returns ``(out, None)``: nothing is read on the host, and the call can be
        captured once the state's graphs are validated and their largest degrees known (``validate()`` / ``max_degree()`` on
        ``state.stages``; head by head: on every ``state.head(s, h)``).  ``want_graphs=True`` makes one host read per stage (per head when
        head by head) and is refused under capture.  With ``features="split16"`` a head whose operands leave the split-fp16 range
        NaN-fills ``out`` and that head's rows of the new graph, never wrong numbers.

        ``propagate`` / ``explore`` / ``seed``: ``CE.step_graph``'s search keywords, handed to every head (off by default: the call is
        then exactly the one above).  The stage-fused launch of THIS method has no search flavour (``search_graphs`` is the
        stage-fused search step): with any of them set ``fused=None`` runs head by head and ``fused=True`` is refused, before any launch.

        A state of ``FixedGraph``s (``state.to_fixed()``) runs head by head -- ``CE.step_graph`` on each head's row views,
        ``FixedGraph.cat``, ``torch.cat`` and the mix convolution, as ``fused=False`` does -- and returns a fixed state; the whole call,
        ``want_graphs=True`` included, reads nothing on the host and can be captured (``state.copy_(new_state)`` inside the capture
        carries the graphs to the next replay).  ``fused="stage"`` is the stage-fused form there: the heads' features from
        ``CE._graph_features``, then ONE ``ops.graph_stage_step_fixed`` per stage -- the four heads' rows in one row launch, fold + mix +
        residual in one launch, the stage's new ``FixedGraph`` made of the call's arrays (no ``cat``); the graphs are the head-by-head
        ones bit for bit, ``out`` differs by the fp32 roundings of the mix product alone, and the search keywords are served (the launch
        has the search flavour).  It is refused on a stage that does not qualify (as ``fused=True`` is on a CSR state).  ``fused=None``
        and ``fused=False`` mean head by head, ``fused=True`` is refused on a fixed state (it names the CSR launch; the fixed-width one
        is ``fused="stage"``); on a CSR state ``fused="stage"`` means ``True``.  Heads of a stage whose output widths differ are
        refused before any launch.

        ``features="stage16"``: the stage's features in ONE pass (``ops.graph_stage_features16``: the inference forward's heads-as-batch
        prologue and projection, one copy-out launch that also forms ``tau``) instead of ``CE._graph_features`` head by head.  Served
        wherever a stage runs fused -- a CSR state with ``fused`` None (on a stage that qualifies) or True, a fixed state with
        ``fused="stage"`` -- and refused before any launch, naming those forms, on every head-by-head path (``fused=False``, a fixed
        state under ``fused=None``, a stage that does not qualify, the search keywords on a CSR state); the heads' own checks are made
        with ``"split16"``.  Graphs and output are the stage-fused call's on those features bit for bit; against ``"split16"`` key rows
        differ in last bits (another launch plan of the same projection kernel), so a fixed-k cut may flip on a tie.  Range: the map
        side has the forward's (both tiers of g(x), the input's per-block scale), the word still trips on weights beyond the split's
        range or a non-finite input, and a tripped word NaN-fills the WHOLE stage -- ``out`` and all four heads' rows of the new
        graph --: one word per call, not one per head.

        Always under ``torch.no_grad()``; the modules' state (packed weights, top-k policy, range verdicts, ``_pack_key``) is untouched:
        the fused calls have workspaces of their own, one per stage.  Every refusal -- ``CE.step_graph``'s, per head, and a state that
        does not fit the input -- is raised before any launch of the call."""
        from ._lib import DaglError
        from . import ops
        from .sequence import SequenceState
        what = "CES.step_graphs"
        search = dict(propagate=propagate, explore=explore, seed=seed)
        ops._graph_search_operands(what, propagate, explore, seed)
        self._fused_value(what, fused)
        stage_fixed = isinstance(fused, str) and isinstance(state, SequenceState) and state.fixed
        if isinstance(fused, str) and not stage_fixed:
            fused = True                            # (a CSR state: the stage-fused step it has)
        if (bool(propagate) or explore != 0) and not stage_fixed:
            if fused:
                raise DaglError(f"{what}: fused=True with propagate / explore set: the stage-fused step (ops.graph_stage_step) has no "
                                "search flavour; leave fused at None (head by head) or pass fused=False")
            fused = False
        if not isinstance(state, SequenceState):
            raise DaglError(f"{what}: a SequenceState expected, got {type(state).__name__}")
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise DaglError(f"{what}: expected [B,C,H,W]")
        want_graphs = bool(want_graphs)
        B = x.shape[0]
        if (state.stages[0].B, state.stages[0].H, state.stages[0].W) != (4 * B, x.shape[2], x.shape[3]):
            g0 = state.stages[0]
            raise DaglError(f"{what}: the state was built for B={g0.B // 4} H={g0.H} W={g0.W}, the input is B={B} H={x.shape[2]} W={x.shape[3]}")
        if state.fixed:
            return self._step_graphs_fixed(x, state, radius, features, want_graphs, fused, search)
        plan = self._plan_step(x, state, radius, features, want_graphs, fused, search)
        out, new = x, []
        for s in (1, 2, 3):
            out, g = self._step_stage(s, out, state, plan[s], features, want_graphs, search)
            new.append(g)
            out = self._between_stages(s, out)
        return out, (SequenceState(new) if want_graphs else None)

    _STAGE16_FUSED_ONLY = ("features='stage16' belongs to the stage-fused forms (a CSR state with fused=None or True on a stage that "
                           "qualifies, a state of FixedGraphs with fused='stage'); {why}: pass features='split16' or 'fp32'")

    def _stage_features(self, s, x, margin, features, grad=False):
        """The four heads' features of stage ``s`` on its input ``x`` -> [(wq_rows, x_rows, tau | None, b2p, poisoned)] per head: the
        one place the stage-fused calls get them.  ``"fp32"`` / ``"split16"``: ``CE._graph_features`` head by head (``grad``: on the
        modules' own parameters, for the caller's autograd graph).  ``"stage16"``: ONE
        ``ops.graph_stage_features16`` for the stage (its own workspace per stage), the heads' operands as views of its ``[4, ...]``
        arrays; ``poisoned`` reads the first elements of those arrays, which the call NaN-fills -- all four heads' -- once an operand
        of any head leaves the split-fp16 range.  The list then carries the head-major arrays themselves as ``stacked`` =
        (wq4, x4, tau4 | None, b2p4): what ``ops.graph_stage_forward`` takes, without a copy."""
        heads, _mix = self._stage_modules(s)
        if features != "stage16":
            fast = features == "split16"
            return [hd._graph_features(x, margin, fast, grad) for hd in heads]
        from . import ops
        wq4, x4, b2p4, tau4 = ops.graph_stage_features16(x, [hd._params_f32(scaled=False) for hd in heads], margin,
                                                         workspace=self._ws_feat[s])
        poisoned = lambda t: torch.addcmul(t, wq4.reshape(-1)[:1], x4.reshape(-1)[:1], value=0.0)
        feats = _StageFeatures((wq4[h], x4[h], tau4[h] if margin else None, b2p4[h], poisoned) for h in range(4))
        feats.stacked = (wq4, x4, tau4 if margin else None, b2p4)
        return feats

    @staticmethod
    def _fused_value(what, fused):
        """``fused`` is None, a bool or "stage"."""
        from ._lib import DaglError
        if not (fused is None or isinstance(fused, bool) or (isinstance(fused, str) and fused == "stage")):
            raise DaglError(f"{what}: fused={fused!r}, expected None, False, True or 'stage'")

    def _plan_fixed(self, what, x, state, radius, features, fused, search, iters=1):
        """Every refusal of ``step_graphs`` / ``search_graphs`` on a state of ``FixedGraph``s that depends on a stage, raised before the
        first launch and without a host read -- every stage sees an input of x's shape, dtype and device -- -> {stage: (radius, k_eff,
        margin, width_out)}.  ``iters`` > 1: the row bound of the later iterations too, from the width the first one leaves."""
        from ._lib import ERR_UNSUPPORTED, DaglError
        from . import ops
        if fused is True:
            raise DaglError(f"{what}: fused=True on a state of FixedGraphs: the stage-fused fixed-width launch is fused='stage' "
                            "(ops.graph_stage_step_fixed); leave fused at None (head by head) or pass fused=False")
        if features == "stage16" and fused != "stage":
            raise DaglError(f"{what}: " + self._STAGE16_FUSED_ONLY.format(why=f"fused={fused!r} on a state of FixedGraphs runs head by head"))
        head_features = "split16" if features == "stage16" else features      # (the heads' own checks know their two routes)
        plan = {}
        for s in (1, 2, 3):
            args = []
            for h, hd in enumerate(self._stage_modules(s)[0]):
                if not isinstance(hd, CE):
                    raise DaglError(f"{what}: head {type(hd).__name__} of stage {s} is not a CE: it steps no graph")
                args.append(hd._fixed_arguments(x, state.head(s - 1, h), "step_graph", radius, None, "reference", head_features, **search))
            widths = [a[3] for a in args]
            if len(set(widths)) != 1:
                raise DaglError(f"{what}: the heads of stage {s} give graphs of widths {widths}: one FixedGraph per stage needs one width "
                                "(heads that share select_mode and select_k)")
            if fused == "stage" and not self._stage_step_fusable(s, x):
                raise DaglError(f"{what}: fused='stage', but stage {s} does not qualify (four plain CE heads sharing select_mode, "
                                "select_k, softmax_scale and the default patch geometry, an fp32 input on the GPU)")
            radius_s, _k, _margin, width_out, propagate, explore, _seed = args[0]
            bound, cap = ops.graph_search_row_bound(width_out, radius_s, propagate, explore), ops.graph_refresh_max_candidates()
            if iters > 1 and bound > cap:
                err = DaglError(f"{what}: after 1 iteration a row of stage {s} holds {width_out} slots: with propagate={bool(propagate)}, "
                                f"explore={explore} and radius {radius_s} it may expand into {bound} candidates, more than {cap}")
                err.code = ERR_UNSUPPORTED
                raise err
            plan[s] = args[0][:4]
        return plan

    def _step_graphs_fixed(self, x, state, radius, features, want_graphs, fused, search):
        """``step_graphs`` on a state of ``FixedGraph``s: the refusals of every head of every stage first (no launch, no host read), then
        head by head or (``fused="stage"``) one ``ops.graph_stage_step_fixed`` per stage."""
        from .graph import FixedGraph
        from .sequence import SequenceState
        plan = self._plan_fixed("CES.step_graphs", x, state, radius, features, fused, search)
        out, new = x, []
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            if fused == "stage":
                out_s, g = self._stage_fixed_fused(s, out, state.stages[s - 1], plan[s], features, search, 1)
            else:
                pairs = [hd.step_graph(out, state.head(s - 1, h), radius=radius, features=features, want_graph=want_graphs, **search)
                         for h, hd in enumerate(heads)]
                g = FixedGraph.cat([g for _, g in pairs]) if want_graphs else None
                out_s = mix(torch.cat([o for o, _ in pairs], dim=1)) + out
            new.append(g)
            out = self._between_stages(s, out_s)
        return out, (SequenceState(new) if want_graphs else None)

    def _stage_fixed_fused(self, s, x, stage, plan, features, search, iters):
        """Stage ``s`` on its input ``x`` and its ``FixedGraph`` by ``ops.graph_stage_step_fixed`` -> (the stage's output, its new graph):
        ``iters - 1`` graph-only calls with seeds ``seed + i``, then the step with ``seed + iters - 1``.  The new graph is made of the
        call's arrays as they are; nothing is read on the host."""
        from . import ops
        heads, mix = self._stage_modules(s)
        radius, k_eff, margin, width_out = plan
        fast = features != "fp32"                   # (the split-fp16 routes carry a range verdict)
        x = x.contiguous()
        feats = self._stage_features(s, x, margin, features)                        # (wq_rows, x_rows, tau, b2p, poisoned) per head
        wq4, x4, b2p4 = ([f[i].contiguous() for f in feats] for i in (0, 1, 3))
        common = dict(width_out=width_out, radius=radius, tau4=[f[2].contiguous() for f in feats] if margin else None, k=k_eff,
                      scale=float(heads[0].softmax_scale), workspace=self._ws_step[s], propagate=bool(search["propagate"]),
                      explore=search["explore"], hw=(x.shape[2], x.shape[3]))
        key, deg = stage.key, stage.deg
        for i in range(iters - 1):
            arrays = ops.graph_stage_step_fixed(wq4, x4, None, key, deg, seed=search["seed"] + i, **common)[1]
            key, deg = arrays["key"], arrays["deg"]
        out, arrays, _status = ops.graph_stage_step_fixed(wq4, x4, b2p4, key, deg, x, mix.weight.detach().contiguous(),
                                                          mix.bias.detach().contiguous(), seed=search["seed"] + iters - 1, **common)
        weight, score = arrays["weight"], arrays["score"]
        if fast:
            # a head that left the split-fp16 range NaN-fills the stage's output and its own rows of the graph, filler included: 0 or NaN
            # per head, added to the head's quarter of the arrays
            for f in feats:
                out = f[4](out)
            verdict = torch.cat([f[4](weight.new_zeros(1)) for f in feats])[:, None]
            weight = (weight.view(4, -1) + verdict).view_as(weight)
            score = (score.view(4, -1) + verdict).view_as(score)
        g = stage._like(arrays["key"], weight, score, arrays["deg"])
        g.mode, g.k = heads[0].select_mode, k_eff
        return out, g

    def forward_on_graphs(self, x, state, *, features: str = "fp32", backward: str = "two_ops", fused=None):
        """The module's output for ``x`` on the FROZEN graphs of ``state`` -> ``out``: ``forward``'s wiring with every head run as
        ``hd.forward_on_graph(stage input, state.head(s, h), features=..., backward=...)`` -- its weights recomputed on the head's
        structure, no selection --, the stage's own mix and residual, ``RBS1`` / ``RBS2`` between the stages.  Not under
        ``torch.no_grad()``: differentiable in ``x`` and every parameter it uses (``CE.forward_on_graph`` names the heads'), the
        structures are constants.  For fine-tuning on a sequence: ``_, state = ces.step_graphs(frame, state)`` moves the graphs without
        gradients, ``ces.forward_on_graphs(frame, state, backward="fused")`` trains on the result.

        ``fused=None`` / ``False``: head by head, the definition of the result.  Refused before the first launch: a ``state`` that is no
        ``SequenceState`` or was built for another ``B``, ``H`` or ``W``, a head that is not a ``CE``, and every head's own refusals
        (``CE.forward_on_graph``'s; those that depend on whether a gradient is wanted are looked at with ``x`` as every stage's input and
        once more when the head runs).  The modules' state is untouched.

        ``fused=True``: per stage the heads' features from ``_stage_features`` (``"fp32"`` / ``"split16"``: ``CE._graph_features`` head
        by head and a ``torch.stack`` of the operands; ``"stage16"``: one ``ops.graph_stage_features16``, whose arrays are head-major
        already), then ONE ``ops.graph_stage_forward`` on the stage's own CSR: ``ops.graph_forward``'s launches over the ``4 B L`` rows
        and the fused fold + mix + residual -- no per-head fold, no concat map, no convolution.  With a gradient wanted the same launches
        run as an autograd op (``ce._GraphStageForward``) whose backward is ``ops.ces_stage_mix_backward`` and ONE
        ``ops.graph_forward_backward`` on the stacked operands; it needs ``backward="fused"`` (the default ``"two_ops"`` contradicts it
        and is refused) and ``features`` ``"fp32"`` or ``"split16"`` (the split-fp16 training kernels keep their per-head form).  Every
        row is the head-by-head fused call's bit for bit; ``out`` differs by the fp32 roundings of the mix product.  A tripped range
        word of any feature route NaN-fills the stage's output.  A stage that does not qualify (``_stage_step_fusable``) is refused,
        there is no silent fallback; so is ``fused="stage"``, which names the fixed-width forms.  ``features="stage16"`` without
        ``fused=True`` is refused.  A state of ``FixedGraph``s is refused whatever ``fused`` is: pass ``state.to_csr()``.  After
        ``state.stages[s].validate()`` and, for training, ``.transpose()`` (host reads, cached on the graph) the call reads nothing on
        the host; without a gradient it can be captured.  All refusals are raised before the first launch."""
        from ._lib import DaglError
        from .sequence import SequenceState
        what = "CES.forward_on_graphs"
        if not isinstance(state, SequenceState):
            raise DaglError(f"{what}: a SequenceState expected, got {type(state).__name__}")
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise DaglError(f"{what}: expected [B,C,H,W]")
        g0 = state.stages[0]
        if (g0.B, g0.H, g0.W) != (4 * x.shape[0], x.shape[2], x.shape[3]):
            raise DaglError(f"{what}: the state was built for B={g0.B // 4} H={g0.H} W={g0.W}, the input is B={x.shape[0]} H={x.shape[2]} "
                            f"W={x.shape[3]}")
        if not state.fixed:                         # (a fixed state meets the heads' own refusal below, whatever ``fused`` is)
            if isinstance(fused, str) and fused == "stage":
                raise DaglError(f"{what}: fused='stage' names the fixed-width forms (step_graphs / search_graphs on a state of "
                                "FixedGraphs); a call on frozen graphs takes fused=None, False or True")
            if not (fused is None or isinstance(fused, bool)):
                raise DaglError(f"{what}: fused={fused!r}, expected None, False or True")
            if fused:
                plan = self._plan_forward_fused(what, x, state, features, backward)
                out = x
                for s in (1, 2, 3):
                    out = self._between_stages(s, self._stage_forward_fused(s, out, state.stages[s - 1], plan[s], features))
                return out
            if features == "stage16":
                raise DaglError(f"{what}: " + self._STAGE16_FUSED_ONLY.format(why=f"fused={fused!r} runs head by head here (the frozen-graph "
                                                                               "call serves it with fused=True)"))
        for s in (1, 2, 3):
            for h, hd in enumerate(self._stage_modules(s)[0]):
                if not isinstance(hd, CE):
                    raise DaglError(f"{what}: head {type(hd).__name__} of stage {s} is not a CE: it runs on no graph")
                hd._attend_arguments(x, state.head(s - 1, h), "forward_on_graph", None, "reference", True, features, None, backward)
        out = x
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            outs = [hd.forward_on_graph(out, state.head(s - 1, h), features=features, backward=backward) for h, hd in enumerate(heads)]
            out = self._between_stages(s, mix(torch.cat(outs, dim=1)) + out)
        return out

    def _why_not_fusable(self, s, x) -> str:
        """The first condition of ``_stage_step_fusable`` that stage ``s`` misses on the input ``x``."""
        heads, mix = self._stage_modules(s)
        if not self.fuse_stage:
            return "the module was not built on 64 channels"
        if not all(type(hd) is CE and not hd._generic and hd.in_channels == 64 for hd in heads):
            return "its heads are not four plain CE modules of the default patch geometry on 64 channels"
        if len({(hd.select_mode, int(hd.select_k), float(hd.softmax_scale)) for hd in heads}) != 1:
            return "its heads do not share select_mode, select_k and softmax_scale"
        if not x.is_cuda:
            return "the input is not on the GPU"
        if x.dtype != torch.float32:
            return f"the input is {x.dtype}, not fp32"
        return f"its mix is {mix.weight.dtype}, not fp32"

    def _plan_forward_fused(self, what, x, state, features, backward):
        """Every refusal of ``forward_on_graphs(fused=True)`` on a CSR state, raised before the first launch -- every stage sees an input
        of x's shape, dtype and device, and a gradient counts as wanted when ``x`` or any parameter of the module asks for one --
        -> {stage: margin}.  The stages' graphs are validated here (one host read per graph, once)."""
        from ._lib import DaglError
        if features not in ("fp32", "split16", "stage16"):
            raise DaglError(f"{what}: features={features!r}, expected 'fp32', 'split16' or 'stage16'")
        if backward not in ("two_ops", "fused"):
            raise DaglError(f"{what}: backward={backward!r}, expected 'two_ops' or 'fused'")
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if grad and backward != "fused":
            raise DaglError(f"{what}: fused=True contradicts backward='two_ops' (a gradient is wanted for the input or a parameter, and "
                            "the stage-fused forward has the fused backward alone); pass backward='fused'")
        if grad and features == "stage16":
            raise DaglError(f"{what}: features='stage16' has no backward (a gradient is wanted for the input or a parameter; the "
                            "split-fp16 training kernels keep their per-head form): pass features='split16' or 'fp32'")
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            for hd in heads:
                if not isinstance(hd, CE):
                    raise DaglError(f"{what}: head {type(hd).__name__} of stage {s} is not a CE: it runs on no graph")
            if not self._stage_step_fusable(s, x):
                raise DaglError(f"{what}: fused=True, but stage {s} does not qualify: {self._why_not_fusable(s, x)} (fused=None or False "
                                "runs head by head)")
            if grad and any(p.dtype != torch.float32 for m in heads + [mix] for p in m.parameters()):
                raise DaglError(CE._FP32_ONLY)
        head_features = "split16" if features == "stage16" else features      # (the heads' own checks know their two routes)
        capturing = x.is_cuda and torch.cuda.is_current_stream_capturing()
        plan = {}
        for s in (1, 2, 3):
            stage = state.stages[s - 1]
            if not capturing and x.is_cuda and stage.row_off.device == x.device:
                stage.validate()
            g = stage._like(stage.row_off, stage.key, stage.weight, stage.score)      # the stage's arrays under a head's shape
            g.B = x.shape[0]
            for hd in self._stage_modules(s)[0]:
                margin = hd._attend_arguments(x, g, "forward_on_graph", None, "reference", True, head_features, None, backward)[0]
            plan[s] = margin
        return plan

    def _stage_forward_fused(self, s, x, stage, margin, features):
        """Stage ``s`` on its input ``x`` and its frozen graph by ONE ``ops.graph_stage_forward`` -- under autograd, with a gradient
        wanted for ``x`` or a parameter of the stage, as ``ce._GraphStageForward`` -> the stage's output."""
        from . import ops
        from .ce import _GraphStageForward
        heads, mix = self._stage_modules(s)
        x = x.contiguous()
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for m in heads + [mix] for p in m.parameters()))
        ws_f, ws_b, ws_mix = self._ws_frozen[s]
        with torch.enable_grad() if grad else torch.no_grad():
            # (wq_rows, x_rows, tau, b2p, poisoned) per head
            feats = self._stage_features(s, x, margin, features, grad=True) if grad else self._stage_features(s, x, margin, features)
            stacked = getattr(feats, "stacked", None)
            verdicts = feats[:1] if stacked is not None else feats          # (one range word per call there, one per head here)
            if stacked is None:
                stacked = tuple(torch.stack([f[i] for f in feats]) if i != 2 or margin else None for i in range(4))
            wq4, x4, tau4, b2p4 = stacked
            scale = float(heads[0].softmax_scale)
            if grad:
                out = _GraphStageForward.apply(wq4, x4, tau4, b2p4, x, mix.weight, mix.bias, stage, scale, "reference", ws_f, ws_b, ws_mix)
            else:
                out = ops.graph_stage_forward(wq4, x4, b2p4, stage.row_off, stage.key, x, mix.weight.detach().contiguous(),
                                              mix.bias.detach().contiguous(), tau4=tau4, scale=scale, normalize="reference",
                                              workspace=ws_f)
            if features != "fp32":
                for f in verdicts:
                    out = f[4](out)                 # a feature route that left the split-fp16 range NaN-fills the stage's output
        return out

    def _plan_step(self, x, state, radius, features, want_graphs, fused, search=None, what="CES.step_graphs"):
        """Every refusal of ``step_graphs`` / ``search_graphs`` that depends on a stage, raised before the first launch -- every stage
        sees an input of x's shape, dtype and device -- -> {stage: (fused?, what ``CE._refresh_arguments`` returns for its heads)}."""
        from ._lib import DaglError
        B = x.shape[0]
        capturing = torch.cuda.is_current_stream_capturing()
        plan = {}
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            ok = self._stage_step_fusable(s, x)
            if fused and not ok:
                raise DaglError(f"{what}: fused=True, but stage {s} does not qualify (four plain CE heads sharing select_mode, select_k, "
                                "softmax_scale and the default patch geometry, an fp32 input on the GPU)")
            use = ok if fused is None else bool(fused)
            if features == "stage16" and not use:
                why = f"stage {s} runs head by head here (" + ("fused=False or a search keyword of step_graphs" if ok else "it does not qualify") + ")"
                raise DaglError(f"{what}: " + self._STAGE16_FUSED_ONLY.format(why=why))
            head_features = "split16" if features == "stage16" else features      # (the heads' own checks know their two routes)
            for h, hd in enumerate(heads):
                if not isinstance(hd, CE):
                    raise DaglError(f"{what}: head {type(hd).__name__} of stage {s} is not a CE: it steps no graph")
                if use:
                    stage = state.stages[s - 1]
                    if not capturing and x.is_cuda and stage.row_off.device == x.device:
                        stage.validate()
                        stage.max_degree()
                    g = stage._like(stage.row_off, stage.key, stage.weight, stage.score)      # the stage's arrays under a head's shape
                    g.B, g._max_degree = B, stage._max_degree
                else:
                    if capturing and not state.has_head(s - 1, h):
                        raise DaglError(f"{what}: head by head under capture needs state.head({s - 1}, {h}) taken before the capture "
                                        "(it reads two offsets on the host)")
                    g = state.head(s - 1, h)
                args = hd._refresh_arguments(x, g, "step_graph", radius, None, "reference", head_features, host_read=want_graphs,
                                             **(search or {}))
            plan[s] = (use, args)
        return plan

    def _step_stage(self, s, x, state, plan, features, want_graphs, search=None):
        """Stage ``s`` of ``step_graphs`` on its input ``x`` -> (the stage's output, its new graph | None).  ``plan``: (fused?, what
        ``CE._refresh_arguments`` returned for its heads) -- the refusals are through."""
        from .graph import PatchGraph
        heads, mix = self._stage_modules(s)
        use, (radius, k_eff, margin, longest) = plan
        if use:
            return self._stage_step_fused(s, x, state.stages[s - 1], radius, k_eff, margin, longest, features, want_graphs)
        pairs = [hd.step_graph(x, state.head(s - 1, h), radius=radius, features=features, want_graph=want_graphs, **(search or {}))
                 for h, hd in enumerate(heads)]
        return mix(torch.cat([o for o, _ in pairs], dim=1)) + x, (PatchGraph.cat([g for _, g in pairs]) if want_graphs else None)

    def _stage_step_fused(self, s, x, stage, radius, k_eff, margin, longest, features, want_graphs):
        """One ``ops.graph_stage_step`` on the four heads' features -> (out, the stage's new graph | None)."""
        from . import ops
        heads, mix = self._stage_modules(s)
        fast = features != "fp32"                   # (the split-fp16 routes carry a range verdict)
        x = x.contiguous()
        feats = self._stage_features(s, x, margin, features)                        # (wq_rows, x_rows, tau, b2p, poisoned) per head
        out, csr, _status = ops.graph_stage_step([f[0].contiguous() for f in feats], [f[1].contiguous() for f in feats],
                                                 [f[3].contiguous() for f in feats], stage.row_off, stage.key, x,
                                                 mix.weight.detach().contiguous(), mix.bias.detach().contiguous(), radius=radius,
                                                 tau4=[f[2].contiguous() for f in feats] if margin else None, k=k_eff,
                                                 scale=float(heads[0].softmax_scale), max_row_edges=longest, want_graph=want_graphs,
                                                 workspace=self._ws_step[s])
        if fast:
            for f in feats:
                out = f[4](out)                     # a head that left the split-fp16 range NaN-fills the stage's output
        return out, (self._stage_graph(stage, csr, feats, fast, heads[0].select_mode, k_eff) if want_graphs else None)

    @staticmethod
    def _stage_graph(stage, csr, feats, fast, mode, k_eff):
        """The stage's new ``PatchGraph`` from a stage-fused call's CSR over the four heads' rows."""
        weight, score = csr["weight"], csr["score"]
        if fast:
            # ... and its own rows of the graph: 0 or NaN per head, spread over the edges by the heads' first offsets (no host read)
            verdict = torch.cat([f[4](weight.new_zeros(1)) for f in feats])
            n = stage.B // 4 * stage.L
            head_of = torch.bucketize(torch.arange(weight.numel(), device=weight.device), csr["row_off"][n:4 * n:n].contiguous(), right=True)
            weight, score = weight + verdict[head_of], score + verdict[head_of]
        g = stage._like(csr["row_off"], csr["key"], weight, score)
        g.mode, g.k, g._valid = mode, k_eff, True                               # (every candidate is a key of the map)
        return g

    # ---- the search step of the whole module: step_graphs with propagation and random candidates, stage-fused -------------------------
    @torch.no_grad()
    def search_graphs(self, x, state, *, iters: int = 1, radius: int = 1, propagate: bool = True, explore: int = 8, seed: int = 0,
                      features: str = "fp32", want_graphs: bool = True, fused=None):
        """The search step of the whole module -> ``(out, SequenceState | None)``: ``step_graphs`` with ``CE.step_graph``'s search
        keywords, where the stage-fused form exists.  Per stage, on the stage's input ``x_s``: the four heads' features are computed
        once; then ``iters - 1`` graph-only search iterations with seeds ``seed + i``; then one search step with seed
        ``seed + iters - 1``, which also gives the stage's output.  ``RBS1`` / ``RBS2`` run between the stages as in ``forward``.

        ``fused=False`` is the definition: per head ``refresh_graph(x_s, g, radius=, propagate=, explore=, seed=seed + i, features=)``
        ``iters - 1`` times, then ``step_graph(..., seed=seed + iters - 1)``; the stage's output is ``mix(cat(outputs)) + x_s``.
        ``fused=True``: ``ops.graph_stage_search`` / ``ops.graph_stage_search_step`` -- ONE row launch over the four heads' rows per
        iteration, one scan, one copy, fold + mix + residual in one launch.  The graphs are the head-by-head ones bit for bit; ``out``
        differs by the fp32 roundings of the mix product alone.  ``fused=None``: fused for every stage that qualifies as in
        ``step_graphs``, head by head otherwise; ``fused=True`` on a stage that does not qualify is refused.

        ``want_graphs=False`` requires ``iters == 1``: it keeps the structure, returns ``(out, None)`` and can be captured under the
        conditions ``step_graphs`` states (``seed`` is a launch argument: a replay explores the same keys).  The split-fp16 range
        contract is ``step_graphs``'s.  Every refusal comes before the first launch: ``iters`` that is no int >= 1, every head's
        ``CE._refresh_arguments``, a state that does not fit the input, and ``ops.graph_search_row_bound`` above
        ``ops.graph_refresh_max_candidates()`` (``code == ERR_UNSUPPORTED``) -- that bound is looked at again before every iteration, on
        the graph the previous one left.  Always under ``torch.no_grad()``; the modules' state is untouched; each stage has one workspace
        (``step_graphs``'s).

        A state of ``FixedGraph``s (``state.to_fixed()``) is served without a host read, so the whole call -- any ``iters``,
        ``want_graphs=True`` included -- can be captured: ``SequenceState.start(...).to_fixed(k)`` followed by
        ``search_graphs(iters=n, fused="stage")`` is a capturable key frame.  The form is asked for by name there: ``fused=False``
        runs head by head (``CE.refresh_graph`` / ``CE.step_graph`` on each head's row views: the definition), ``fused="stage"`` runs
        ``ops.graph_stage_step_fixed`` once per iteration and stage (``iters - 1`` graph-only calls, then the step), ``fused=True`` is
        refused as in ``step_graphs``.  ``fused=None`` on a fixed state keeps the refusal callers have met so far -- it names the two
        served values and ``state.to_csr()`` --: the default of this method means "the CSR's fused search where a stage qualifies", and
        no fixed-width form is what that default has ever returned.  On a CSR state ``fused="stage"`` means ``True``.  Every
        iteration's row bound is looked at before the first launch, from the widths alone: a rank-cut mode leaves ``k`` slots per row
        after the first iteration, "adaptive" keeps the state's width.

        ``features="stage16"`` as in ``step_graphs``: the stage's features in one pass, served by the fused forms (a CSR state under
        ``fused`` None / True on a stage that qualifies, a fixed state under ``fused="stage"``), refused before any launch on the
        head-by-head ones; a tripped range word NaN-fills the whole stage."""
        from ._lib import DaglError
        from . import ops
        from .sequence import SequenceState
        what = "CES.search_graphs"
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise DaglError(f"{what}: iters={iters!r}, an int >= 1 expected")
        want_graphs = bool(want_graphs)
        if not want_graphs and iters != 1:
            raise DaglError(f"{what}: want_graphs=False keeps the structure: iters={iters} iterations would be thrown away (iters=1 only)")
        ops._graph_search_operands(what, propagate, explore, seed)
        search = dict(propagate=bool(propagate), explore=explore, seed=seed)
        if not isinstance(state, SequenceState):
            raise DaglError(f"{what}: a SequenceState expected, got {type(state).__name__}")
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise DaglError(f"{what}: expected [B,C,H,W]")
        self._fused_value(what, fused)
        if state.fixed and fused is None:
            raise DaglError(f"{what}: a state of FixedGraphs is searched by name: pass fused='stage' (ops.graph_stage_step_fixed) or "
                            "fused=False (head by head); the default form serves the CSR: pass state.to_csr()")
        B = x.shape[0]
        g0 = state.stages[0]
        if (g0.B, g0.H, g0.W) != (4 * B, x.shape[2], x.shape[3]):
            raise DaglError(f"{what}: the state was built for B={g0.B // 4} H={g0.H} W={g0.W}, the input is B={B} H={x.shape[2]} W={x.shape[3]}")
        if state.fixed:
            return self._search_graphs_fixed(x, state, iters, radius, features, want_graphs, fused, search)
        if isinstance(fused, str):
            fused = True                            # (a CSR state: the stage-fused search step it has)
        plan = self._plan_step(x, state, radius, features, want_graphs, fused, search, what=what)
        out, new = x, []
        for s in (1, 2, 3):
            out, g = self._search_stage(s, out, state, plan[s], iters, features, want_graphs, search)
            new.append(g)
            out = self._between_stages(s, out)
        return out, (SequenceState(new) if want_graphs else None)

    def _search_graphs_fixed(self, x, state, iters, radius, features, want_graphs, fused, search):
        """``search_graphs`` on a state of ``FixedGraph``s: the refusals first (every iteration's row bound from the widths alone: no
        launch, no host read), then head by head -- ``CE.refresh_graph`` / ``CE.step_graph`` on each head's row views -- or
        (``fused="stage"``) ``ops.graph_stage_step_fixed`` once per iteration and stage."""
        from .graph import FixedGraph
        from .sequence import SequenceState
        plan = self._plan_fixed("CES.search_graphs", x, state, radius, features, fused, search, iters)
        seed = search["seed"]
        kw = dict(radius=radius, features=features, propagate=search["propagate"], explore=search["explore"])
        out, new = x, []
        for s in (1, 2, 3):
            heads, mix = self._stage_modules(s)
            if fused == "stage":
                out_s, g = self._stage_fixed_fused(s, out, state.stages[s - 1], plan[s], features, search, iters)
            else:
                pairs = []
                for h, hd in enumerate(heads):
                    g = state.head(s - 1, h)
                    for i in range(iters - 1):
                        g = hd.refresh_graph(out, g, seed=seed + i, **kw)
                    pairs.append(hd.step_graph(out, g, seed=seed + iters - 1, want_graph=want_graphs, **kw))
                g = FixedGraph.cat([g for _, g in pairs]) if want_graphs else None
                out_s = mix(torch.cat([o for o, _ in pairs], dim=1)) + out
            new.append(g)
            out = self._between_stages(s, out_s)
        return out, (SequenceState(new) if want_graphs else None)

    def _search_stage(self, s, x, state, plan, iters, features, want_graphs, search):
        """Stage ``s`` of ``search_graphs`` on its input ``x`` -> (the stage's output, its new graph | None)."""
        from ._lib import ERR_UNSUPPORTED, DaglError
        from . import ops
        from .graph import PatchGraph
        heads, mix = self._stage_modules(s)
        use, (radius, k_eff, margin, longest) = plan
        seed = search["seed"]
        kw = dict(radius=radius, features=features, propagate=search["propagate"], explore=search["explore"])
        if not use:
            pairs = []
            for h, hd in enumerate(heads):
                g = state.head(s - 1, h)
                for i in range(iters - 1):
                    g = hd.refresh_graph(x, g, seed=seed + i, **kw)
                pairs.append(hd.step_graph(x, g, seed=seed + iters - 1, want_graph=want_graphs, **kw))
            return mix(torch.cat([o for o, _ in pairs], dim=1)) + x, (PatchGraph.cat([g for _, g in pairs]) if want_graphs else None)
        fast = features != "fp32"                   # (the split-fp16 routes carry a range verdict)
        x = x.contiguous()
        feats = self._stage_features(s, x, margin, features)                        # (wq_rows, x_rows, tau, b2p, poisoned) per head
        wq4, x4, b2p4 = ([f[i].contiguous() for f in feats] for i in (0, 1, 3))
        common = dict(radius=radius, tau4=[f[2].contiguous() for f in feats] if margin else None, k=k_eff,
                      scale=float(heads[0].softmax_scale), workspace=self._ws_step[s], propagate=search["propagate"],
                      explore=search["explore"])
        stage = state.stages[s - 1]
        g, cap = stage, ops.graph_refresh_max_candidates()
        for i in range(iters):
            if i:
                longest = g.max_degree()                   # (one word read on the host: iters > 1 returns graphs, never captured)
                bound = ops.graph_search_row_bound(longest, radius, search["propagate"], search["explore"])
                if bound > cap:
                    err = DaglError(f"CES.search_graphs: after {i} iteration(s) a row of stage {s} holds {longest} edges: with "
                                    f"propagate={search['propagate']}, explore={search['explore']} and radius {radius} it may expand "
                                    f"into {bound} candidates, more than {cap}")
                    err.code = ERR_UNSUPPORTED
                    raise err
            if i < iters - 1:
                csr = ops.graph_stage_search(wq4, x4, g.row_off, g.key, (x.shape[2], x.shape[3]), max_row_edges=longest,
                                             seed=seed + i, **common)
                g = stage._like(csr["row_off"], csr["key"], csr["weight"], csr["score"])
        out, csr, _status = ops.graph_stage_search_step(wq4, x4, b2p4, g.row_off, g.key, x, mix.weight.detach().contiguous(),
                                                        mix.bias.detach().contiguous(), max_row_edges=longest, want_graph=want_graphs,
                                                        seed=seed + iters - 1, **common)
        if fast:
            for f in feats:
                out = f[4](out)                     # a head that left the split-fp16 range NaN-fills the stage's output
        return out, (self._stage_graph(stage, csr, feats, fast, heads[0].select_mode, k_eff) if want_graphs else None)

    @torch.no_grad()
    def build_graphs(self, x, *, iters: int = 4, radius: int = 1, explore: int = 8, seed: int = 0, features: str = "fp32", fused=None):
        """A key frame of the whole module WITHOUT any scan of the L*N pairs -> ``(out, SequenceState)``: ``search_graphs`` from
        ``SequenceState.start`` with ``propagate=True``.  Head ``h`` of stage ``s`` comes out as
        ``hd.build_graph(x_s, iters=, radius=, explore=, seed=, features=)`` on the stage's input, bit for bit; ``out`` is the module's
        output on those graphs.  How close they come to ``forward_with_graphs``' depends on the input (``CE.build_graph``)."""
        from ._lib import DaglError
        from .sequence import SequenceState
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise DaglError("CES.build_graphs: expected [B,C,H,W]")
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise DaglError(f"CES.build_graphs: iters={iters!r}, an int >= 1 expected")
        mode = self._stage_modules(1)[0][0]
        mode = mode.select_mode if isinstance(mode, CE) else "adaptive"
        start = SequenceState.start(x.shape[0], x.shape[2], x.shape[3], x.device, mode)
        return self.search_graphs(x, start, iters=iters, radius=radius, propagate=True, explore=explore, seed=seed, features=features,
                                  want_graphs=True, fused=fused)


class _MeanShift(nn.Conv2d):
    """Registered by the reference (``add_mean``, dagl.py:41) but never applied; kept for state_dict compatibility."""

    def __init__(self, rgb_range, rgb_mean=(0.4488, 0.4371, 0.4040), rgb_std=(1.0, 1.0, 1.0), sign=1):
        super().__init__(3, 3, kernel_size=1)
        std = torch.tensor(rgb_std)
        self.weight.data = torch.eye(3).view(3, 3, 1, 1) / std.view(3, 1, 1, 1)
        self.bias.data = sign * rgb_range * torch.tensor(rgb_mean) / std
        for p in self.parameters():
            p.requires_grad = False


class RR(nn.Module):
    """head conv - 8 ResBlocks - CES - 8 ResBlocks - conv - tail conv, global residual (dagl.py:11-54)."""

    def __init__(self, n_resblocks=16, n_feats=64, n_colors=1, res_scale=1.0, rgb_range=1.0, ce_cls=CE):
        super().__init__()
        body = [ResBlock(n_feats, res_scale) for _ in range(n_resblocks // 2)]
        body.append(CES(n_feats, ce_cls=ce_cls))
        body += [ResBlock(n_feats, res_scale) for _ in range(n_resblocks // 2)]
        body.append(_conv(n_feats, n_feats, 3))
        self.add_mean = _MeanShift(rgb_range)
        self.head = nn.Sequential(_conv(n_colors, n_feats, 3))
        self.body = nn.Sequential(*body)
        self.tail = nn.Sequential(_conv(n_feats, n_colors, 3))

    def forward(self, x):
        return x + self.tail(self.body(self.head(x)))

    def _forward_around_ces(self, x, ces_call):
        """``forward`` with the trunk's modules run in order and ``ces_call`` in the place of the ``CES``'s forward -> (out, its state)."""
        out, state = self.head(x), None
        for m in self.body:
            if isinstance(m, CES):
                out, state = ces_call(m, out)
            else:
                out = m(out)
        return x + self.tail(out), state

    def forward_with_graphs(self, x):
        """The key frame of a sequence -> ``(out, SequenceState)``: ``forward`` with ``CES.forward_with_graphs`` where the ``CES`` sits."""
        return self._forward_around_ces(x, lambda ces, t: ces.forward_with_graphs(t))

    @torch.no_grad()
    def step_graphs(self, x, state, **kw):
        """A sequence step of the network -> ``(out, SequenceState | None)``: ``forward`` with ``CES.step_graphs(., state, **kw)`` where the
        ``CES`` sits (``radius``, ``features``, ``want_graphs``, ``fused`` -- ``"stage"`` on a fixed state included --, ``propagate``, ``explore``, ``seed`` as there); always under ``torch.no_grad()``.  The ``CES``'s
        refusals are raised when it is reached: the head convolution and the ResBlocks in front of it have run by then."""
        return self._forward_around_ces(x, lambda ces, t: ces.step_graphs(t, state, **kw))

    @torch.no_grad()
    def search_graphs(self, x, state, **kw):
        """The search step of the network -> ``(out, SequenceState | None)``: ``forward`` with ``CES.search_graphs(., state, **kw)`` where
        the ``CES`` sits (``iters``, ``radius``, ``propagate``, ``explore``, ``seed``, ``features``, ``want_graphs``, ``fused`` as there, a
        fixed state and ``fused="stage"`` included); always under ``torch.no_grad()``.  The ``CES``'s refusals are raised when it is reached."""
        return self._forward_around_ces(x, lambda ces, t: ces.search_graphs(t, state, **kw))

    @torch.no_grad()
    def build_graphs(self, x, **kw):
        """A key frame of the network without any L*N scan -> ``(out, SequenceState)``: ``forward`` with ``CES.build_graphs(., **kw)``
        where the ``CES`` sits (``iters``, ``radius``, ``explore``, ``seed``, ``features``, ``fused`` as there)."""
        return self._forward_around_ces(x, lambda ces, t: ces.build_graphs(t, **kw))

    def forward_on_graphs(self, x, state, **kw):
        """The network's output for ``x`` on the frozen graphs of ``state`` -> ``out``: ``forward`` with
        ``CES.forward_on_graphs(., state, **kw)`` where the ``CES`` sits (``features``, ``backward``, ``fused`` as there).  Not under
        ``torch.no_grad()``: with autograd enabled the result trains the trunk and the heads on constant structures.  The ``CES``'s
        refusals are raised when it is reached: the head convolution and the ResBlocks in front of it have run by then."""
        return self._forward_around_ces(x, lambda ces, t: (ces.forward_on_graphs(t, state, **kw), None))[0]

    def load_state_dict(self, state_dict, strict=True):
        """The reference network's own loader rule (``dagl.py:56-73``), which is NOT torch's: checkpoint entries are
        copied in place into the tensors this network owns; an entry whose shape does not fit raises ``RuntimeError``
        and an entry this network does not know raises ``KeyError`` (``strict`` only) -- unless its name contains
        ``tail``: the reference fine-tunes a gray checkpoint into an ``n_colors = 3`` network (and back) that way, so
        anything about the last convolution is tolerated.  Keys the checkpoint lacks are never an error.  Returns
        ``None`` like the reference."""
        own = self.state_dict()
        for name, value in state_dict.items():
            tolerated = "tail" in name
            if name not in own:
                if strict and not tolerated:
                    raise KeyError(f'unexpected key "{name}" in state_dict')
                continue
            src = value.data if isinstance(value, nn.Parameter) else value
            try:
                with torch.no_grad():
                    own[name].copy_(src)          # shares storage (and version counter) with the parameter / buffer
            except Exception:
                if not tolerated:
                    raise RuntimeError(
                        f"While copying the parameter named {name}, whose dimensions in the model are "
                        f"{tuple(own[name].shape)} and whose dimensions in the checkpoint are {tuple(src.shape)}.")
        for m in self.modules():                  # packed / converted weight copies of the heads follow the new values
            if hasattr(m, "invalidate_packed"):
                m.invalidate_packed()


def seeded_state_dict(template: "OrderedDict[str, torch.Tensor]", seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Regenerable stand-in for a trained checkpoint (none ships with the reference): every tensor of ``template`` in
    state_dict order from ONE numpy PCG64 stream -- weights uniform(+-1/sqrt(fan_in)), biases uniform(+-1/sqrt(fan_in)
    of their layer) approximated by +-0.05, PReLU slopes 0.25, ``add_mean`` left as built."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, t in template.items():
        if name.startswith("add_mean"):
            out[name] = t.clone()
        elif t.dim() >= 2:
            fan_in = int(np.prod(t.shape[1:]))
            b = 1.0 / math.sqrt(fan_in)
            out[name] = torch.from_numpy(rng.uniform(-b, b, size=tuple(t.shape)).astype(np.float32))
        elif name.endswith("bias"):
            out[name] = torch.from_numpy(rng.uniform(-0.05, 0.05, size=tuple(t.shape)).astype(np.float32))
        else:                                             # PReLU slope
            out[name] = torch.full(tuple(t.shape), 0.25)
    return out


CHOP_PRESETS = {       # (min_size, shave_size_max) of the four forks' forward_chop
    "dn_gray": (10000, 24),      # DN_Gray/model/__init__.py:179,187
    "car": (10000, 24),          # CAR/model/__init__.py:190,199
    "demosaic": (10000, 12),     # Demosaic/model/__init__.py:179,188
    "dn_real": (70000, 12),      # DN_Real/model/__init__.py:135,144  (no self-ensemble in that fork)
}


def sparse_heads_state_dict(sd: "OrderedDict[str, torch.Tensor]", seed: int, gain: float = 1.65,
                            prefix: str = "body.8.") -> "OrderedDict[str, torch.Tensor]":
    """Replace the parameters of the 12 ``CE`` heads in ``sd`` (keys ``<prefix>c<stage>_<head>.*``) by
    ``synth.make_ce_params(seed + index, "sparse", gain)``: thr / bias heads that keep a handful of neighbours per query
    (mean degrees of ~5-10, long-tailed) -- the regime a trained DAGL works in, as opposed to default-initialised heads
    that keep ~95 % of the keys.  Regenerable anywhere (numpy PCG64)."""
    from .synth import make_ce_params
    out = OrderedDict(sd)
    idx = 0
    for s in (1, 2, 3):
        for h in (1, 2, 3, 4):
            for n, a in make_ce_params(seed + idx, variant="sparse", sparse_gain=gain).items():
                out[f"{prefix}c{s}_{h}.{n}"] = torch.from_numpy(a)
            idx += 1
    return out


def tile_boxes(h: int, w: int, shave_scale: int = 4, shave_size_max: int = 24):
    """Geometry of ONE 4-way split of the reference's ``forward_chop`` (DN_Gray/model/__init__.py:194-198, :222-229) for an
    h x w tile: the four overlapping corner boxes ``(y0, y1, x0, x1)`` of size (h//2//4*4 + 24) x (w//2//4*4 + 24), and per corner
    the pair (destination box in the h x w output, source box inside the corner tile's output) that stitches the inner
    quadrants back.  Every user of the tiling (sequential driver, batched driver, leaf enumeration) takes it from here."""
    hh, wh = h // 2, w // 2
    hs = (hh // shave_scale) * shave_scale + shave_size_max
    ws = (wh // shave_scale) * shave_scale + shave_size_max
    corners = [(0, hs, 0, ws), (0, hs, w - ws, w), (h - hs, h, 0, ws), (h - hs, h, w - ws, w)]
    stitch = [((0, hh, 0, wh), (0, hh, 0, wh)),
              ((0, hh, wh, w), (0, hh, ws - w + wh, ws)),
              ((hh, h, 0, wh), (hs - h + hh, hs, 0, wh)),
              ((hh, h, wh, w), (hs - h + hh, hs, ws - w + wh, ws))]
    return corners, stitch, hs * ws


def _stitch(x: torch.Tensor, outs, stitch) -> torch.Tensor:
    out = x.new_empty(x.shape)
    for o, ((dy0, dy1, dx0, dx1), (sy0, sy1, sx0, sx1)) in zip(outs, stitch):
        out[:, :, dy0:dy1, dx0:dx1] = o[:, :, sy0:sy1, sx0:sx1]
    return out


def chop_leaf_boxes(h: int, w: int, min_size: int = 10000, shave_size_max: int = 24, shave_scale: int = 4, y: int = 0, x: int = 0):
    """The leaf tiles ``(y0, y1, x0, x1)`` (image coordinates, depth-first order) the reference's tiling cuts an h x w image into:
    256 x 256 -> 64 tiles of 72 x 72."""
    corners, _, area = tile_boxes(h, w, shave_scale, shave_size_max)
    boxes = [(y + y0, y + y1, x + x0, x + x1) for (y0, y1, x0, x1) in corners]
    if area < min_size:
        return boxes
    out = []
    for (y0, y1, x0, x1) in boxes:
        out.extend(chop_leaf_boxes(y1 - y0, x1 - x0, min_size, shave_size_max, shave_scale, y0, x0))
    return out


def chop_forward(model, x: torch.Tensor, min_size: int = 10000, shave_size_max: int = 24, shave_scale: int = 4,
                 ensemble: bool = False):
    """Recursive 4-way tiled inference: the reference's ``Model.forward_chop`` for scale 1
    (DN_Gray/model/__init__.py:179-231); ``ensemble`` = its ``--ensemble`` switch: ``test_x8`` on every leaf (:205-208).  A tile of
    h x w is split into four overlapping corner tiles (``tile_boxes``) until the corner area drops below ``min_size``; the outputs'
    inner quadrants are stitched back."""
    corners, stitch, area = tile_boxes(x.shape[2], x.shape[3], shave_scale, shave_size_max)
    tiles = [x[:, :, y0:y1, x0:x1] for (y0, y1, x0, x1) in corners]
    if area < min_size:
        # the reference runs the four leaves one by one with n_GPUs == 1 (__init__.py:203-209)
        outs = [forward_x8(model, t) if ensemble else model(t.contiguous()) for t in tiles]
    else:
        outs = [chop_forward(model, t, min_size, shave_size_max, shave_scale, ensemble) for t in tiles]
    return _stitch(x, outs, stitch)


def chop_forward_batched(model, x: torch.Tensor, min_size: int = 10000, shave_size_max: int = 24, shave_scale: int = 4,
                         max_batch: int = 64, ensemble: bool = False):
    """Same tiling and stitching as ``chop_forward``, but all leaf tiles (they share one shape) go through the network in
    batches of up to ``max_batch`` instead of one by one: tiles are independent, and a batch is just
    another grid dimension of the HIP block.  Device-side equivalent of the reference's per-leaf loop."""
    boxes = chop_leaf_boxes(x.shape[2], x.shape[3], min_size, shave_size_max, shave_scale)   # the order chop_forward visits them
    if len({(y1 - y0, x1 - x0) for (y0, y1, x0, x1) in boxes}) != 1:   # ragged leaves (odd sizes): the sequential driver
        return chop_forward(model, x, min_size, shave_size_max, shave_scale, ensemble)
    plan = [x[:, :, y0:y1, x0:x1] for (y0, y1, x0, x1) in boxes]
    outs = []
    for i in range(0, len(plan), max_batch):
        batch = torch.cat([t for t in plan[i:i + max_batch]], dim=0).contiguous()
        # self-ensemble: each of the 8 variants of ALL leaves of the batch is one network call (the leaves of a variant
        # share a shape); per leaf this is exactly test_x8's stack and mean
        res = forward_x8(model, batch) if ensemble else model(batch)
        outs.extend(res.split(x.shape[0], dim=0))
    return stitch_leaves(x, outs, min_size, shave_size_max, shave_scale)


def stitch_leaves(x: torch.Tensor, outs, min_size: int = 10000, shave_size_max: int = 24, shave_scale: int = 4) -> torch.Tensor:
    """Put the leaf outputs ``outs`` (the order of ``chop_leaf_boxes`` = the order ``chop_forward`` visits them) back together:
    the reference's recursion (DN_Gray/model/__init__.py:216-231) bottom-up, inner quadrants of every 4-way split."""
    it = iter(outs)

    def stitch_tree(h, w):
        corners, stitch, area = tile_boxes(h, w, shave_scale, shave_size_max)
        if area < min_size:
            o = [next(it) for _ in range(4)]
        else:
            o = [stitch_tree(y1 - y0, x1 - x0) for (y0, y1, x0, x1) in corners]
        return _stitch(o[0].new_empty(o[0].shape[0], o[0].shape[1], h, w), o, stitch)

    return stitch_tree(x.shape[2], x.shape[3])


def chop_forward_sharded(model, x: torch.Tensor, dist=None, min_size: int = 10000, shave_size_max: int = 24, shave_scale: int = 4,
                         max_batch: int = 64, ensemble: bool = False):
    """Tile-level multi-GPU inference: the reference hands ``min(n_GPUs, 4)`` leaf tiles per call to ``nn.DataParallel``
    (DN_Gray/model/__init__.py:181, 203-209); here -- one process per GPU, SURVEY.md section 8(e) "tiles/8 leaf tiles at inference"
    -- the leaf tiles of ``chop_leaf_boxes`` are dealt to the ranks as contiguous slices (``shard.shard_range``), every rank runs
    its slice in batches of up to ``max_batch``, ONE ``all_gather`` (RCCL on GPUs, any backend of the process group) brings the
    leaf outputs to every rank, and every rank stitches the full image (``stitch_leaves``).  ``x`` is the same full image on
    every rank.  Without an initialised process group (or at world size 1) this is ``chop_forward_batched``.  Tiles are independent:
    no halo, no exchange besides the gather."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return chop_forward_batched(model, x, min_size, shave_size_max, shave_scale, max_batch, ensemble)
    from .shard import shard_range
    rank, world = dist.get_rank(), dist.get_world_size()
    boxes = chop_leaf_boxes(x.shape[2], x.shape[3], min_size, shave_size_max, shave_scale)
    shapes = {(y1 - y0, x1 - x0) for (y0, y1, x0, x1) in boxes}
    if len(shapes) != 1:
        # ragged leaves (odd sizes) cannot share one gather buffer: every rank runs the sequential driver (same result everywhere)
        return chop_forward(model, x, min_size, shave_size_max, shave_scale, ensemble)
    lo, hi = shard_range(len(boxes), rank, world)
    mine = []
    for i in range(lo, hi, max_batch):
        batch = torch.cat([x[:, :, y0:y1, x0:x1] for (y0, y1, x0, x1) in boxes[i:min(i + max_batch, hi)]], dim=0).contiguous()
        res = forward_x8(model, batch) if ensemble else model(batch)
        mine.extend(res.split(x.shape[0], dim=0))
    # fixed-size slices (they differ by at most one leaf): pad, gather once, trim
    per = -(-len(boxes) // world)
    if mine:
        like = mine[0]
    else:                                                  # more ranks than leaves: the output shape of a leaf from one probe call
        (y0, y1, x0, x1) = boxes[0]
        like = model(x[:, :, y0:y1, x0:x1].contiguous())
    buf = like.new_zeros((per,) + tuple(like.shape))
    for j, o in enumerate(mine):
        buf[j] = o
    gathered = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(gathered, buf)
    outs = []
    for r in range(world):
        l, h = shard_range(len(boxes), r, world)
        outs.extend(gathered[r][j] for j in range(h - l))
    return stitch_leaves(x, outs, min_size, shave_size_max, shave_scale)


# The 8 symmetries of the square in the order the reference enumerates them (``augment_img`` modes 0..7,
# DN_Gray/model/__init__.py:35-51): (quarter turns counter-clockwise in the (H, W) plane, then flip the rows?)
_X8_MODES = ((0, False), (1, True), (0, True), (3, False), (2, True), (1, False), (2, False), (3, True))
_X8_INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)      # modes 3 and 5 undo each other, the rest are involutions (test_x8, :56-59)


def _x8_apply(t: torch.Tensor, mode: int) -> torch.Tensor:
    k, flip = _X8_MODES[mode]
    if k:
        t = t.rot90(k, (-2, -1))
    if flip:
        t = t.flip(-2)
    return t


def forward_x8(forward_fn, x: torch.Tensor) -> torch.Tensor:
    """Geometric self-ensemble of the reference (``test_x8``, DN_Gray/model/__init__.py:53-62): the 8 flip / rotate
    variants go through ``forward_fn``, the outputs are transformed back and averaged -- same variants, same order of the
    stack that is averaged.  The reference round-trips every variant through numpy on the host (``augment_img_tensor``,
    :18-32); here the transforms stay on the device."""
    outs = [_x8_apply(forward_fn(_x8_apply(x, m).contiguous()), _X8_INVERSE[m]) for m in range(8)]
    return torch.stack(outs, dim=0).mean(dim=0, keepdim=False)


def psnr(img: torch.Tensor, ref: torch.Tensor, data_range: float = 1.0) -> float:
    """Per-image PSNR as ``batch_PSNR`` computes it (DN_Gray/utils.py:18-24: skimage compare_psnr on the float images)."""
    mse = torch.mean((img.double() - ref.double()) ** 2).item()
    return float("inf") if mse == 0 else 10.0 * math.log10(data_range ** 2 / mse)


def set12_protocol_noise(clean: torch.Tensor, sigma: float = 50.0, rgb_range: float = 1.0) -> torch.Tensor:
    """Noise of the reference test script (DN_Gray/test.py:55-58): torch.manual_seed(1), CPU normal_()."""
    torch.manual_seed(1)
    noise = torch.FloatTensor(clean.size()).normal_(mean=0, std=sigma / (255.0 / rgb_range))
    return clean + noise
