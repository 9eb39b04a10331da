"""``CE`` -- drop-in replacement of the reference's patch-graph attention head.

Mirrors ``CE`` of /root/reference/DN_Gray/model/dagl.py:174-277 (and its forks in
CAR/, Demosaic/, DN_Real/): same constructor signature, same parameter names and
shapes (including the registered-but-unused ``W``, dagl.py:192), same
``forward(b: [B,in_channels,H,W]) -> [B,inter_channels,H,W]`` -- so ``CES``
(dagl.py:74-119) accepts it by class substitution and reference checkpoints load
unchanged.

The whole method -- the four prologue convolutions (dagl.py:208-215) and
everything from patch extraction to the batch concat (dagl.py:216-274) -- runs
in the HIP library behind ``include/dagl_ce.h``; torch only owns the parameters,
the device memory and the stream.  There is no eager fallback.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import ERR_UNSUPPORTED, FAST_CAP, MAX_TOPK, DaglError
from .synth import same_pad_amounts


class _GraphCore(torch.autograd.Function):
    """dagl.py:250-272 as one differentiable op.  ``route`` = (forward, backward), the pair of HIP entry points the call took
    (``_lists_route`` .. ``_generic_route``): ``forward(wq_rows, x_rows, b2, thr, bias) -> (out, saved, info | None)`` and
    ``backward(d_out, wq_rows, x_rows, b2, thr, bias, *saved) -> (d_wq_rows, d_x_rows, d_b2, d_thr, d_bias)``.  ``thr`` /
    ``bias`` are None in mode "topk"; ``sink`` (a dict or None) takes the forward's info when it has one."""

    @staticmethod
    def forward(ctx, wq_rows, x_rows, b2, thr, bias, route, sink):
        wq_rows, x_rows, b2 = wq_rows.contiguous(), x_rows.contiguous(), b2.contiguous()
        thr_c = thr.contiguous() if thr is not None else None
        bias_c = bias.contiguous() if bias is not None else None
        out, saved, info = route[0](wq_rows, x_rows, b2, thr_c, bias_c)
        ctx.backward_fn, ctx.thr_shape = route[1], thr.shape if thr is not None else None
        ctx.save_for_backward(wq_rows, x_rows, b2, thr_c, bias_c, *saved)
        if sink is not None and info is not None:
            sink.update(info)
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_wq, d_x, d_b2, d_thr, d_bias = ctx.backward_fn(d_out.contiguous().float(), *ctx.saved_tensors)
        if ctx.thr_shape is not None:
            d_thr, d_bias = d_thr.view(ctx.thr_shape), d_bias.view(ctx.thr_shape)
        return d_wq, d_x, d_b2, d_thr, d_bias, None, None


def _lists_route(mode, k, exact_scan, ws_f, ws_b):
    """Each query's neighbour list (``dagl_ce_core_forward`` / ``_backward``): the backward returns the gradients autograd would
    derive from the dense form."""
    def forward(wq_rows, x_rows, b2, thr, bias):
        out, s = ops.ce_core_forward(wq_rows, x_rows, b2, thr, bias, mode=mode, k=k, workspace=ws_f, exact_scan=exact_scan)
        return out, (s["nb_idx"], s["nb_wgt"], s["nb_s"], s["nb_cnt"], s["mu"]), s["info"]

    def backward(d_out, wq_rows, x_rows, b2, thr, bias, nb_idx, nb_wgt, nb_s, nb_cnt, mu):
        saved = dict(nb_idx=nb_idx, nb_wgt=nb_wgt, nb_s=nb_s, nb_cnt=nb_cnt, mu=mu)
        return ops.ce_core_backward(d_out, wq_rows, x_rows, b2, thr, bias, saved, mode=mode, k=k, workspace=ws_b)
    return forward, backward


def _dense_route(want_info, exact, ws_f, ws_b):
    """Dense neighbourhoods (adaptive masks that keep more keys than a fixed-width list holds -- default-initialised heads keep
    ~95 %): the dense formulation (``dagl_ce_core_dense_forward`` / ``_backward``): the forward on the streamed split-fp16 kernel,
    the backward's matrix products on the fp16 matrix cores with split operands (``exact``: both on the fp32 matrix cores;
    dense_train.hip).  Statistics only with ``want_info`` (a host synchronisation)."""
    def forward(wq_rows, x_rows, b2, thr, bias):
        out, s = ops.ce_core_dense_forward(wq_rows, x_rows, b2, thr, bias, workspace=ws_f, want_info=want_info, exact=exact)
        return out, (s["lse"], s["mu"]), s["info"]

    def backward(d_out, wq_rows, x_rows, b2, thr, bias, lse, mu):
        return ops.ce_core_dense_backward(d_out, wq_rows, x_rows, b2, thr, bias, dict(lse=lse, mu=mu), workspace=ws_b, exact=exact)
    return forward, backward


def _wide_route(mode, k, want_info, ws_f, ws_b):
    """The top-k modes when min(k, N) exceeds the lists' width (the fixed-k variant takes any num_edge,
    GReccR2b_3mh_1-checkpoint.py:242-250; CA_model-checkpoint.py:134-143 uses 500): the dense formulation with the row-wise
    selection of the k best scores as its mask (``dagl_ce_core_wide_forward`` / ``_backward``; dense_train.hip, wide_select.h)."""
    def forward(wq_rows, x_rows, b2, thr, bias):
        out, info = ops.ce_core_wide_forward(wq_rows, x_rows, b2, thr, bias, mode, k, workspace=ws_f, want_info=want_info)
        return out, (), info

    def backward(d_out, wq_rows, x_rows, b2, thr, bias):
        return ops.ce_core_wide_backward(d_out, wq_rows, x_rows, b2, thr, bias, mode, k, workspace=ws_b)
    return forward, backward


def _generic_route(geom, mode, k, scale, ws_f, ws_b):
    """A module built with a non-default patch geometry ``geom`` = (H, W, ksize, stride_1, stride_2)
    (``dagl_ce_generic_core_forward`` / ``_backward``, csrc/generic.hip): the dense formulation on the fp32 matrix cores, S and A
    recomputed chunk by chunk in the backward; ``b2`` is the zero-bordered NHWC value map."""
    def forward(wq_rows, x_rows, b2p, thr, bias):
        return ops.ce_generic_core_forward(wq_rows, x_rows, b2p, thr, bias, *geom, mode=mode, k=k, softmax_scale=scale,
                                           workspace=ws_f), (), None

    def backward(d_out, wq_rows, x_rows, b2p, thr, bias):
        return ops.ce_generic_core_backward(d_out, wq_rows, x_rows, b2p, thr, bias, *geom, mode=mode, k=k, softmax_scale=scale,
                                            workspace=ws_b)
    return forward, backward


class _GraphApply(torch.autograd.Function):
    """Value map -> block output on a given patch graph (``ops.graph_apply``): ``fold(A_G . V(b2)) / cnt``, dagl.py:263-272 with ``yi``
    supplied.  Differentiable in the zero-bordered NHWC value map and in the edge weights (``ops.graph_apply_backward``); the graph's
    structure is a constant."""

    @staticmethod
    def forward(ctx, b2p, weight, graph, ws_f, ws_b):
        b2p, weight = b2p.contiguous(), weight.contiguous()
        ctx.graph, ctx.ws_b = graph, ws_b
        ctx.save_for_backward(b2p, weight)
        return ops.graph_apply(b2p, graph.row_off, graph.key, weight, workspace=ws_f)

    @staticmethod
    def backward(ctx, d_out):
        b2p, weight = ctx.saved_tensors
        g = ctx.graph
        need_map, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_b2p, d_w = ops.graph_apply_backward(d_out.contiguous().float(), b2p, g.row_off, g.key, weight,
                                              transposed=g.transpose() if need_map else None, need_b2p=need_map, need_weight=need_w,
                                              workspace=ctx.ws_b)
        return d_b2p, d_w, None, None, None


class _GraphAttend(torch.autograd.Function):
    """Features -> the block's edge weights on a given structure (``ops.graph_attend``): S on the edges, the margin against ``tau`` (None:
    the fixed-k variant), the reference's softmax restricted to the graph.  Returns (weight, score); differentiable in the two feature
    matrices and ``tau`` through ``weight`` (``ops.graph_attend_backward``), ``score`` carries no gradient; the structure is a constant."""

    @staticmethod
    def forward(ctx, wq_rows, x_rows, tau, graph, scale, normalize, ws_f, ws_b):
        wq_rows, x_rows = wq_rows.contiguous(), x_rows.contiguous()
        tau_c = tau.contiguous() if tau is not None else None
        weight, score = ops.graph_attend(wq_rows, x_rows, graph.row_off, graph.key, tau_c, scale=scale, normalize=normalize,
                                         workspace=ws_f, hw=(graph.H, graph.W))
        ctx.graph, ctx.call, ctx.ws_b = graph, (scale, normalize), ws_b
        ctx.tau_shape = tau.shape if tau is not None else None
        ctx.save_for_backward(wq_rows, x_rows, tau_c, score, weight)
        ctx.mark_non_differentiable(score)
        return weight, score

    @staticmethod
    def backward(ctx, d_weight, _d_score):
        wq_rows, x_rows, tau, score, weight = ctx.saved_tensors
        g = ctx.graph
        need_wq, need_x, need_tau = ctx.needs_input_grad[:3]
        d_wq, d_x, d_tau = ops.graph_attend_backward(d_weight.contiguous().float(), wq_rows, x_rows, g.row_off, g.key, score, weight, tau,
                                                     scale=ctx.call[0], normalize=ctx.call[1],
                                                     transposed=g.transpose() if need_x else None, need_wq=need_wq, need_x=need_x,
                                                     need_tau=need_tau and tau is not None, workspace=ctx.ws_b, hw=(g.H, g.W))
        if d_tau is not None:
            d_tau = d_tau.view(ctx.tau_shape)
        return d_wq, d_x, d_tau, None, None, None, None, None


class _GraphForward(torch.autograd.Function):
    """Features and value map -> block output on a given structure in one crossing of the edges (``ops.graph_forward_train``): the
    composition of ``_GraphAttend`` and ``_GraphApply`` with ``ops.graph_forward``'s bits.  Differentiable in the two feature matrices,
    ``tau`` and the value map (``ops.graph_forward_backward``); saved between forward and backward: the operands and (M, D) per row --
    no per-edge tensor; the structure is a constant."""

    @staticmethod
    def forward(ctx, wq_rows, x_rows, tau, b2p, graph, scale, normalize, ws_f, ws_b):
        wq_rows, x_rows, b2p = wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous()
        tau_c = tau.contiguous() if tau is not None else None
        out, row_max, row_sum = ops.graph_forward_train(wq_rows, x_rows, b2p, graph.row_off, graph.key, tau_c, scale=scale,
                                                        normalize=normalize, workspace=ws_f)
        ctx.graph, ctx.call, ctx.ws_b = graph, (scale, normalize), ws_b
        ctx.tau_shape = tau.shape if tau is not None else None
        ctx.save_for_backward(wq_rows, x_rows, tau_c, b2p, row_max, row_sum)
        return out

    @staticmethod
    def backward(ctx, d_out):
        wq_rows, x_rows, tau, b2p, row_max, row_sum = ctx.saved_tensors
        g = ctx.graph
        need_wq, need_x, need_tau, need_map = ctx.needs_input_grad[:4]
        d_wq, d_x, d_tau, d_b2p = ops.graph_forward_backward(d_out.contiguous().float(), wq_rows, x_rows, b2p, g.row_off, g.key, row_max,
                                                             row_sum, tau, scale=ctx.call[0], normalize=ctx.call[1],
                                                             transposed=g.transpose() if need_x or need_map else None, need_wq=need_wq,
                                                             need_x=need_x, need_tau=need_tau and tau is not None, need_b2p=need_map,
                                                             workspace=ctx.ws_b)
        if d_tau is not None:
            d_tau = d_tau.view(ctx.tau_shape)
        return d_wq, d_x, d_tau, d_b2p, None, None, None, None, None


class _GraphStageForward(torch.autograd.Function):
    """A whole ``CES`` stage on its frozen graph (``ops.graph_stage_forward(train=True)``): the four heads' features and value maps
    stacked head-major, the stage's input and its 1x1 mix -> the stage's output.  Differentiable in all of them: the backward is
    ``ops.ces_stage_mix_backward`` (d cat head-major, d mix_w, d mix_b), then ``_GraphForward``'s ``ops.graph_forward_backward`` ONCE on
    the stacked operands as those of 4 B images, with the stage graph's transposed CSR; the gradient of the residual input is ``d_out``.
    Saved between forward and backward: the operands, (M, D) per row and the head-major concat map ``cat4`` (B * 64 * H * W floats, what
    a convolution's autograd keeps as its input) -- no per-edge array, no 784-float row array; the structure is a constant."""

    @staticmethod
    def forward(ctx, wq4, x4, tau4, b2p4, x, mix_w, mix_b, graph, scale, normalize, ws_f, ws_b, ws_mix):
        wq4, x4, b2p4, x = wq4.contiguous(), x4.contiguous(), b2p4.contiguous(), x.contiguous()
        tau_c = tau4.contiguous() if tau4 is not None else None
        mix_w_c, mix_b_c = mix_w.contiguous(), mix_b.contiguous()
        out, row_max, row_sum, cat4 = ops.graph_stage_forward(wq4, x4, b2p4, graph.row_off, graph.key, x, mix_w_c, mix_b_c, tau4=tau_c,
                                                              scale=scale, normalize=normalize, train=True, workspace=ws_f)
        ctx.graph, ctx.call, ctx.ws = graph, (scale, normalize), (ws_b, ws_mix)
        ctx.save_for_backward(wq4, x4, tau_c, b2p4, mix_w_c, row_max, row_sum, cat4)
        return out

    @staticmethod
    def backward(ctx, d_out):
        wq4, x4, tau4, b2p4, mix_w, row_max, row_sum, cat4 = ctx.saved_tensors
        g = ctx.graph
        need_wq, need_x, need_tau, need_map, need_in, need_w, need_b = ctx.needs_input_grad[:7]
        need_tau = need_tau and tau4 is not None
        d_out = d_out.contiguous().float()
        d_cat4, d_w, d_b = ops.ces_stage_mix_backward(d_out, cat4, mix_w, need_w=need_w, need_b=need_b, workspace=ctx.ws[1])
        d_wq = d_x = d_tau = d_b2p = None
        if need_wq or need_x or need_tau or need_map:
            flat = lambda t: t.flatten(0, 1) if t is not None else None
            d_wq, d_x, d_tau, d_b2p = ops.graph_forward_backward(flat(d_cat4), flat(wq4), flat(x4), flat(b2p4), g.row_off, g.key, row_max,
                                                                 row_sum, flat(tau4), scale=ctx.call[0], normalize=ctx.call[1],
                                                                 transposed=g.transpose() if need_x or need_map else None,
                                                                 need_wq=need_wq, need_x=need_x, need_tau=need_tau, need_b2p=need_map,
                                                                 workspace=ctx.ws[0])
        like = lambda d, t: d.view(t.shape) if d is not None else None
        return (like(d_wq, wq4), like(d_x, x4), like(d_tau, tau4) if d_tau is not None else None, like(d_b2p, b2p4),
                d_out if need_in else None, like(d_w, mix_w), d_b, None, None, None, None, None, None)


_CONV_WEIGHTS = ("g.weight", "theta.weight", "thr_conv.weight", "bias_conv.weight")


def _pad_channels4(t):
    """Zero channels along dim -3 -- the channels of a map [B,C,H,W], the input channels of a convolution weight [O,C,kh,kw] -- up to
    a multiple of 4: the library's unfold and prologue kernels work on float4 channel groups; zero channels with zero weight columns
    change nothing (under autograd the pad's backward slices them off)."""
    padc = (-t.shape[-3]) % 4
    return F.pad(t, (0, 0, 0, 0, 0, padc)) if padc else t


class _EvalLazyGrad(torch.autograd.Function):
    """An eval() block inside an autograd-enabled forward (the reference's test loop, DN_Gray/trainer.py:128-140, builds a
    graph it never uses): forward on the inference kernels, nothing saved but the input; a backward -- rare -- recomputes
    the block on the differentiable path (``CE._forward_train``) and hands its gradients on."""

    @staticmethod
    def forward(ctx, module, k_eff, n_params, b, *params):
        ctx.module, ctx.n_params = module, n_params
        ctx.save_for_backward(b, *params)
        with torch.no_grad():
            return module._forward_infer(b, k_eff)

    @staticmethod
    def backward(ctx, d_out):
        b, *params = ctx.saved_tensors
        with torch.enable_grad():
            bb = b.detach().requires_grad_(True)
            out = ctx.module._forward_train(bb)
            used = [p for p in params]
            grads = torch.autograd.grad(out, [bb] + used, d_out.contiguous().float(), allow_unused=True)
        return (None, None, None) + tuple(grads)


class CE(nn.Module):
    def __init__(self, ksize=7, stride_1=4, stride_2=1, softmax_scale=10, shape=64, p_len=64, in_channels=64,
                 inter_channels=16, use_multiple_size=False, use_topk=False, add_SE=False, num_edge=50):
        super().__init__()
        # Patch geometry (dagl.py:175-176).  The reference's own builders never override it (dagl.py:94-109) and every tuned kernel has
        # (7, 4, 1, 16) compiled in; any other geometry runs the reference's dense formulation with the geometry as run-time arguments
        # (dagl_ce_generic_forward, csrc/generic.hip: fp32 matrix cores, inference only).
        self._generic = (int(ksize), int(stride_1), int(stride_2), int(inter_channels)) != (7, 4, 1, 16)
        if self._generic:
            if not (1 <= int(ksize) <= 31 and int(stride_1) >= 1 and int(stride_2) >= 1):
                raise DaglError(f"CE: ksize={ksize} (1..31), stride_1={stride_1}, stride_2={stride_2} (>= 1)")
            if int(inter_channels) < 4 or int(inter_channels) % 4:
                raise DaglError(f"CE: inter_channels={inter_channels} must be a multiple of 4 (16-byte pixels of the NHWC maps)")
        if not float(softmax_scale) > 0.0:
            raise DaglError(f"CE: softmax_scale={softmax_scale} must be positive")
        self.ksize, self.shape, self.p_len = ksize, shape, p_len
        self.stride_1, self.stride_2 = stride_1, stride_2
        self.softmax_scale = softmax_scale
        self.inter_channels, self.in_channels = inter_channels, in_channels
        self.use_multiple_size, self.use_topk, self.add_SE = use_multiple_size, use_topk, add_SE
        self.num_edge = num_edge
        # same registration order and names as dagl.py:190-205
        self.g = nn.Conv2d(in_channels, inter_channels, kernel_size=3, stride=1, padding=1)
        self.W = nn.Conv2d(inter_channels, in_channels, kernel_size=1, stride=1, padding=0)   # never applied
        self.theta = nn.Conv2d(in_channels, inter_channels, kernel_size=1, stride=1, padding=0)
        feat = ksize ** 2 * inter_channels
        self.fc1 = nn.Sequential(nn.Linear(feat, feat // 4), nn.ReLU())
        self.fc2 = nn.Sequential(nn.Linear(feat, feat // 4), nn.ReLU())
        self.thr_conv = nn.Conv2d(in_channels, 1, kernel_size=ksize, stride=stride_1, padding=0)
        self.bias_conv = nn.Conv2d(in_channels, 1, kernel_size=ksize, stride=stride_1, padding=0)
        # Neighbour selection.  The shipped forward ignores use_topk/num_edge (dead arguments,
        # dagl.py:176,187,189) and always applies the adaptive mask; ``select_mode`` makes the fixed-k
        # variant (GReccR2b_3mh_1-checkpoint.py:242-250) and the intersection available:
        #   "adaptive" | "topk" | "adaptive_topk", with k = ``select_k``.
        self.select_mode = "adaptive"
        self.select_k = num_edge       # the fixed-k variant's own default is 50; k > MAX_TOPK: row-wise dense form (no lists)
        # "screened": bf16 matrix-core screen of all L*N scores + exact refinement of the survivors (default);
        # "exact": every score on the fp32 matrix cores.  Same neighbours either way.
        self.scan = "screened"
        self._ws = ops.Workspace()
        self._ws_bwd = ops.Workspace()
        self._ws_graph = ops.Workspace()  # graph() / degrees(): a buffer of their own, so that the forward's packed weights and policy words survive
        self._ws_apply = ops.Workspace()      # apply_graph() and the fused forward_on_graph(): aggregated and partial rows; the backward's rows
        self._ws_apply_bwd = ops.Workspace()
        self._ws_attend = ops.Workspace()     # attend_graph() / forward_on_graph(): the row statistics; the backward's sums and partial rows
        self._ws_attend_bwd = ops.Workspace()
        self._ws_forward_bwd = ops.Workspace()    # forward_on_graph(backward="fused"): dAgg, d V rows, three floats per edge, the rows' sums
        self._ws_lists = ops.Workspace()      # forward_with_graph(): the list-form core's forward and backward, the degrees of the CSR conversion
        self._ws_lists_bwd = ops.Workspace()
        self._ws_lists_csr = ops.Workspace()
        self._ws_refresh = ops.Workspace()    # refresh_graph(): the degrees and the staged candidates
        self._ws_step = ops.Workspace()       # step_graph(): the aggregated rows and, with the graph, the refresh's regions
        self._pack_key = None
        self._pack_epoch = 0           # bumped by invalidate_packed()
        self._f32_cache = {}              # fp32 copies of half-precision parameters (model.half(), DN_Gray/model/__init__.py:98-99)
        self._scaled_cache = {}           # softmax_scale != 10: scaled copies of fc1 / the bias head (_scale_c)
        self._train_calls = 0
        self._wide_calls = 0
        self._last_call = None
        self._calls_since_range_check = 0
        self._train_dense = False      # the differentiable path met dense neighbourhoods last time (dense_train.hip)
        self._train_dense_calls = 0
        self._dense_hint = False       # the last adaptive call ended in the dense formulation: start there next time
        self._dense_calls = 0
        # adaptive mode: "always" (default) = read the call's verdict on the host every call: any neighbourhood structure is
        # served (lists + per-query redo, dense formulation, CSR lists).  "auto" (opt-in, for steady sparse workloads and HIP-graph
        # capture) = once four calls in a row were served in-stream, stop waiting (DAGL_FLAG_NO_WAIT: no synchronisation at
        # all); the device-side verdict NaN-fills a call the in-stream kernels could not serve -- never wrong numbers -- and
        # the sticky word is polled every 16th call, which sends the module back to waiting.
        self.adaptive_sync = "always"
        # top-k modes: where the candidate threshold comes from.  "sparse" = a subset of the keys (DAGL_FLAG_SAMPLED_TOPK): for k <= 16 on
        # maps of >= 1024 k keys the two keys with the largest feature row sum of every 64 (csrc/pivot.hip: a threshold as good as
        # "full"'s from N / 32 keys), otherwise every 8th key tile (enough on maps whose scores are spread evenly); "full" = every second key tile + eight times
        # the candidate slots (DAGL_FLAG_TIGHT_TOPK: +25 us at 256^2) -- on natural-image features the sampled threshold lets
        # hundreds of keys per query through, the slots overflow and the call lands on the fp32 redo pass (2.7 ms instead of 0.25);
        # "auto" (default) = the workspace's own policy word, read by the kernels themselves (round 4: no host poll, valid under
        # HIP-graph replay): sampled until any query of a call overflows (a full segment spills into the query's shared area first),
        # tight from then on; the first call of a shape re-runs tight in-stream; maps of <= 16 384 keys start tight.
        self.topk_threshold = "auto"
        # Top-k modes behind the screen: "always" (default) = every call queues the fp32 redo pass for query groups whose candidate slots
        # overflowed (a launch that finds nothing on a warm workspace: 4.7 us under rocprofv3, which serialises dispatches); "auto" =
        # once three polls of the workspace in a row (every 64th call, as for the range word) have found the last call without redo work, identical
        # calls (same shape, weights, workspace) go without the launch (DAGL_FLAG_NO_REDO) and the workspace is polled every 32nd call;
        # a call that flags a group after all returns NaN -- never wrong numbers --, the next poll reports it and the module queues
        # the pass again from then on.  Not under HIP-graph capture (a replayed graph is never polled).  Measured on the headline
        # (profiles/r05_ab_topk_redo_launch.log, same box, interleaved): 0.2250 ms with "auto" against 0.2254 with "always" -- in the
        # un-profiled stream the empty launch runs under its neighbours' dispatch and the polls cost what is left; hence not the default.
        self.topk_redo = "always"
        self._redo_skip = False        # the last three polls found no redo work
        self._redo_clean_polls = 0
        self._redo_banned = False      # a no-redo call went unserved once: never again on this module
        self._served_streak = 0
        self._served_streaks = {}      # the same for adaptive_sync = "auto"
        self._served_shape = None
        self._nowait_calls = 0
        self.last_info = None
        self.profile = None            # optional ops.StageProfile (benchmark instrumentation)

    def reset_topk_policy(self):
        """Forget what ``topk_threshold = "auto"`` has learnt: the policy word lives in the workspace and starts afresh with a cold
        one (the next call re-packs the weights there)."""
        self._pack_key = None

    def topk_policy_is_tight(self) -> bool:
        """Whether this module's workspace has switched to the tight threshold (bit 3 of ``dagl_ce_range_check``; one host
        synchronisation; reads -- and clears, if set -- the sticky range word like ``range_ok``)."""
        if self._last_call is None or self.select_mode == "adaptive" or self.scan == "exact":
            return False
        shape, dev = self._last_call
        bad = ops.ce_range_check(shape, self.select_mode, min(int(self.select_k), shape[2] * shape[3]), self._ws, dev)
        if bad & 1:
            self._note_range_violation("a call left the split-fp16 range (its output is NaN-filled)")
        return bool(bad & 8)

    def range_ok(self) -> bool:
        """False when an inference call on this module since the last poll met operands the split-fp16 kernels do not hold
        (include/dagl_ce.h "Range": since round 6 that is a non-finite input or |g(x)| >= 1.5e7 -- the input itself has no limit
        and the key / query map two tiers --, or dense-regime features >= 937): that call's output is NaN-filled.  Switches the
        module to ``scan = "exact"`` (the fp32 path, no range limit) in that case.  One host synchronisation."""
        self._calls_since_range_check = 0
        if self.scan == "exact" or self._last_call is None:
            return True
        shape, dev = self._last_call
        bad = ops.ce_range_check(shape, self.select_mode, min(int(self.select_k), shape[2] * shape[3]) if self.select_mode != "adaptive" else 0,
                                 self._ws, dev)
        if self.select_mode != "adaptive":
            if bad & 16:
                import warnings
                warnings.warn("dagl_amd.CE: a top-k call that went without the fp32 redo pass (topk_redo = 'auto') met query groups whose "
                              "candidate slots overflowed: its output is NaN-filled; this module queues the pass again from now on")
                self._redo_banned, self._redo_skip, self._redo_clean_polls = True, False, 0
            else:
                # three polls in a row without redo work (not one: inputs that overflow the candidate slots now and then would hand
                # out NaN-filled calls until the next poll)
                self._redo_clean_polls = 0 if (bad & 4) else self._redo_clean_polls + 1
                self._redo_skip = self._redo_clean_polls >= 3 and not self._redo_banned
        if bad & 2:
            import warnings
            warnings.warn("dagl_amd.CE: an adaptive call that did not wait for its verdict met neighbourhoods the in-stream kernels "
                          "could not serve (its output is NaN-filled); the module reads the verdict on the host again")
            self._served_streak = 0
        if bad & 1:
            self._note_range_violation("a call left the split-fp16 range (its output is NaN-filled)")
        return not (bad & 19)

    def _note_range_violation(self, what):
        import warnings
        warnings.warn(f"dagl_amd.CE: {what}; this module now uses scan='exact' (fp32 matrix cores, no range limit)")
        self.scan = "exact"
        self._pack_key = None

    def invalidate_packed(self):
        """Forget the packed copies of fc1 / fc2 / g / theta kept in the workspace.  The cache is keyed on the weights' storage and
        torch's version counter, which every in-place op and optimizer step bumps -- but edits through ``.data``
        (``w.data.mul_()``, EMA / clipping written that way) do NOT: call this after such an edit.  ``.to()`` / ``.cuda()`` /
        ``.half()`` (``_apply``) and ``load_state_dict`` call it themselves."""
        self._pack_epoch += 1
        self._pack_key = None
        self._f32_cache = {}
        self._scaled_cache = {}

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_packed()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super()._load_from_state_dict(*args, **kwargs)

    def extra_repr(self):
        return f"select_mode={self.select_mode!r}, select_k={self.select_k}"

    def _scale_c(self) -> float:
        """softmax_scale other than the kernels' 10 (dagl.py:175, 260), without touching a kernel: the logits are
        softmax_scale * S * m with m = relu(S - mean(S) thr + bias) (top-k variant: m in {0, 1}).  Scaling the query features by c
        (fc1's weight and bias: ReLU is positively homogeneous) scales S and mean(S) thr by c; scaling the bias head by c as well
        scales m by c, the mask (m > 0) and the top-k order do not move, and the kernels' 10 * S' * m' is 10 c^2 S m (10 c S for the
        top-k variant).  So c = sqrt(softmax_scale / 10), or softmax_scale / 10 in "topk" mode."""
        r = float(self.softmax_scale) / 10.0
        if r == 1.0:
            return 1.0
        return r if self.select_mode == "topk" else math.sqrt(r)

    def _params_f32(self, scaled: bool = True):
        """The block's parameters as contiguous fp32 tensors.  fp32 modules: the parameters themselves.  ``model.half()`` /
        ``.bfloat16()`` modules (the reference's ``--precision half`` test path, DN_Gray/model/__init__.py:98-99,
        option.py:76-78): converted once and kept until the parameter changes (storage or version counter) -- the block
        computes in fp32 on the values the half-precision weights hold.  ``scaled``: fc1 and the bias head carry the factor of
        ``_scale_c`` (the generic route hands ``softmax_scale`` to its kernel instead)."""
        out = {}
        for n, p in self.named_parameters():
            if n.startswith("W."):
                continue
            t = p.detach()
            if t.dtype == torch.float32:
                out[n] = t.contiguous()
                continue
            if t.dtype not in (torch.float16, torch.bfloat16):
                raise DaglError(f"CE: parameter {n} has dtype {t.dtype}; fp32, fp16 or bf16 expected")
            tag = (t.data_ptr(), t._version, t.dtype, t.device)
            hit = self._f32_cache.get(n)
            if hit is None or hit[0] != tag:
                hit = (tag, t.float().contiguous())
                self._f32_cache[n] = hit
            out[n] = hit[1]
        if not scaled:
            return out
        c = self._scale_c()
        if c == 1.0:
            self._scaled_cache = {}
        else:                           # (see _scale_c; scaled copies kept until the PARAMETER -- not its fp32 copy, whose version
                                        # counter never moves -- or the factor changes)
            own = dict(self.named_parameters())
            for n in ("fc1.0.weight", "fc1.0.bias") + (() if self.select_mode == "topk" else ("bias_conv.weight", "bias_conv.bias")):
                src = out[n]
                tag = (own[n].data_ptr(), own[n]._version, own[n].dtype, own[n].device, c)
                hit = self._scaled_cache.get(n)
                if hit is None or hit[0] != tag:
                    hit = (tag, (src * c).contiguous())
                    self._scaled_cache[n] = hit
                out[n] = hit[1]
        return out

    def _topk_threshold(self):
        """``topk_threshold`` as the (tight_topk, sampled_topk) pair of the ``ops`` entry points, which apply it to the top-k modes
        behind the screen only."""
        if self.topk_threshold not in ("auto", "full", "sparse"):
            raise DaglError(f"CE.topk_threshold {self.topk_threshold!r}: expected 'auto', 'full' or 'sparse'")
        return self.topk_threshold == "full", self.topk_threshold == "sparse"

    def _prologue(self, b):
        """The four prologue convolutions of dagl.py:208-215 as stock torch ops (MIOpen) -- kept for the
        stage-level parity tests; forward() computes them inside the HIP library (prologue.hip)."""
        b1 = self.g(b)
        b2 = self.theta(b)
        H, W = b.shape[-2:]
        t, bo = same_pad_amounts(H, self.ksize, self.stride_1)
        l, r = same_pad_amounts(W, self.ksize, self.stride_1)
        b4 = F.pad(b, (l, r, t, bo))
        thr = self.thr_conv(b4).reshape(b.shape[0], -1)
        bias = self.bias_conv(b4).reshape(b.shape[0], -1)
        return b1, b2, thr, bias

    def _forward_train(self, b: torch.Tensor) -> torch.Tensor:
        """Differentiable path (DN_Gray/trainer.py:44-50), every stage on the HIP library: the four prologue convolutions
        and the two patch projections as unfold + fp32 matrix-core GEMM with explicit backward (train_ops.py; fc(unfold(.))
        = a product of the patch rows with the Linear weight, dagl.py:240-249), the graph core (dagl.py:250-272) as a HIP
        op with its own backward: neighbour lists (top-k modes, adaptive masks keeping <= 64 keys per query) or, for
        denser masks, the dense formulation."""
        from . import train_ops as T
        if any(p.dtype != torch.float32 for p in self.parameters()):
            raise DaglError("CE: the differentiable path needs fp32 parameters (the reference's --precision half is a test-time "
                            "switch, DN_Gray/model/__init__.py:98-99); run half-precision modules under torch.no_grad()")
        self._last_call = None         # the shared workspace is about to be reused with the training layout: no range word to poll
        B, _, H, W = b.shape
        ks, c = self.ksize, self.inter_channels
        t, _bo = same_pad_amounts(H, ks, self.stride_1)
        l, _r = same_pad_amounts(W, ks, self.stride_1)
        Lh, Lw = -(-H // self.stride_1), -(-W // self.stride_1)
        # dagl.py:208-215  g (3x3, pad 1), theta (1x1), thr_conv / bias_conv (7x7 stride 4 on the SAME-padded input): one forward
        # call of the library's fp32 prologue kernels, layer-by-layer unfold / GEMM backward (train_ops._PrologueConvs)
        thr = bias = None
        convs = (self.g, self.theta, self.thr_conv, self.bias_conv)
        if self.in_channels % 4:
            from types import SimpleNamespace
            b = _pad_channels4(b)
            convs = tuple(SimpleNamespace(weight=_pad_channels4(m.weight), bias=m.bias) for m in convs)
        if self.select_mode != "topk":                 # (the fixed-k variant has no threshold heads)
            b1p, b2p, thr, bias = T.prologue_convs(b, *convs, fast=self.scan != "exact")
        else:
            b1p, b2p = T.prologue_convs(b, convs[0], convs[1], fast=self.scan != "exact")
        b2 = b2p[:, T.PAD:T.PAD + H, T.PAD:T.PAD + W, :].permute(0, 3, 1, 2)                  # NCHW view of the value map
        # dagl.py:216-249  patches of b1 (stride 4 SAME / stride 1) through fc1 / fc2 + ReLU
        wq_rows = T.patch_linear(b1p, T.fc_weight_rows(self.fc1[0].weight, c, ks), self.fc1[0].bias, ks, self.stride_1,
                                 T.PAD - t, T.PAD - l, Lh, Lw, relu=True, allow_fast=self.scan != "exact")   # [B,L,196]
        x_rows = T.patch_linear(b1p, T.fc_weight_rows(self.fc2[0].weight, c, ks), self.fc2[0].bias, ks, self.stride_2,
                                0, 0, H, W, relu=True, allow_fast=self.scan != "exact")             # [B,N,196]
        sc = self._scale_c()
        if sc != 1.0:                   # softmax_scale != 10: see _scale_c (plain torch ops: autograd carries the factor)
            wq_rows = wq_rows * sc
            if bias is not None:
                bias = bias * sc
        info = {}
        self._pack_key = None          # the shared workspace is reused with another layout
        exact, ws = self.scan == "exact", (self._ws, self._ws_bwd)

        def core(route):
            return _GraphCore.apply(wq_rows, x_rows, b2, thr, bias, route, info)

        k_eff = min(int(self.select_k), H * W) if self.select_mode != "adaptive" else 0
        if k_eff > MAX_TOPK:
            # more neighbours than the lists hold: the dense formulation with the row-wise selection as its mask
            want = self._wide_calls % 64 == 0           # (statistics cost a host synchronisation: every 64th call)
            self._wide_calls += 1
            out = core(_wide_route(self.select_mode, k_eff, want, *ws))
        elif self.select_mode == "adaptive" and self._train_dense:
            # the last training call met dense neighbourhoods: start in the dense formulation; every 16th call reads the
            # degrees back (one host synchronisation) to notice when the masks have become sparse enough for the lists
            self._train_dense_calls += 1
            probe = self._train_dense_calls % 16 == 1
            out = core(_dense_route(probe, exact, *ws))
            if probe and 0 <= info.get("max_degree", -1) <= FAST_CAP:
                self._train_dense = False
        else:
            try:
                out = core(_lists_route(self.select_mode, min(int(self.select_k), H * W), exact, *ws))
            except DaglError as e:
                if self.select_mode != "adaptive" or e.code != ERR_UNSUPPORTED:
                    raise
                self._train_dense, self._train_dense_calls = True, 1
                out = core(_dense_route(True, exact, *ws))
        if info:
            self.last_info = info
        # range guard of the training path: its split-fp16 forward kernels (the two patch projections: |b1| < 4094, |w_fc| < 64; the
        # streamed dense core: |feature| < 937) NaN-fill what they hand out once an operand leaves that range -- never wrong
        # numbers -- and the dense core re-runs itself in fp32 whenever it reads statistics back.  The module finds out from
        # that flag, or by looking at its output every 64th call (one synchronisation), and moves to scan = "exact" (fp32
        # GEMM forward, no range limit); the call at hand is then repeated on that path.
        if self.scan != "exact":
            self._train_calls += 1
            left = bool(info.get("range_fallback"))
            if not left and self._train_calls % 64 == 1:
                left = bool(torch.isnan(out).any())
            if left:
                self._note_range_violation("a training call left the split-fp16 range")
                return self._forward_train(b)
        return out

    def forward(self, b: torch.Tensor) -> torch.Tensor:
        if b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.forward: expected [B,{self.in_channels},H,W], got {tuple(b.shape)}")
        if not b.is_cuda:
            raise DaglError("CE.forward: input must be on the GPU; dagl_amd has no CPU path")
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        k_eff = 0
        if self.select_mode != "adaptive":
            # no silent clamp: the fixed-k variant takes exactly min(num_edge, N) neighbours (GReccR2b_3mh_1-checkpoint.py:243)
            if int(self.select_k) < 1:
                raise DaglError(f"CE: select_k={self.select_k} < 1")
            k_eff = min(int(self.select_k), b.shape[2] * b.shape[3])
            # k_eff > MAX_TOPK (include/dagl_ce.h DAGL_MAX_TOPK): no per-query lists -- the inference entry points take every
            # query's score row in the dense form (csrc/topk_wide.hip), the differentiable path the dense formulation with the
            # row-wise selection as its mask (_wide_route)
        in_dtype = b.dtype
        if in_dtype in (torch.bfloat16, torch.float16):
            # reduced-precision feature maps (BASELINE config 3): the block itself computes in fp32 with the bf16
            # matrix-core screen; I/O is converted at the boundary
            b = b.float()
        elif in_dtype != torch.float32:
            raise DaglError(f"CE.forward: unsupported dtype {in_dtype}")
        # differentiable route: the module is training (its own parameters or a gradient for its input).  An eval() module
        # stays on the inference kernels even when autograd is on -- the reference's test loop relies on the long-dead
        # ``volatile`` flag (DN_Gray/trainer.py:132), i.e. evaluates the whole network with autograd enabled, and inside
        # RR / CES the block's input then "requires grad" although nobody will ask for one.  Such a call keeps its place in
        # the autograd graph (_EvalLazyGrad): should a backward arrive after all, it recomputes the block on the
        # differentiable path then -- same gradients, paid only when used.
        grad = torch.is_grad_enabled()
        if self._generic:
            if grad and (b.requires_grad or (self.training and any(p.requires_grad for p in self.parameters()))):
                out = self._forward_train_generic(b.contiguous(), k_eff)
            else:
                out = self._forward_infer_generic(b, k_eff)
        elif grad and self.training and (b.requires_grad or any(p.requires_grad for p in self.parameters())):
            out = self._forward_train(b.contiguous())
        elif grad and b.requires_grad:
            ps = [p for p in self.parameters() if p.requires_grad]
            out = _EvalLazyGrad.apply(self, k_eff, len(ps), b.contiguous(), *ps)
        else:
            out = self._forward_infer(b, k_eff)
        return out if in_dtype == torch.float32 else out.to(in_dtype)

    def _graph_csr(self, b: torch.Tensor, what: str, **kw):
        """Input checks of ``forward``, the prologue convolutions in fp32, ``ops.ce_graph``."""
        if b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.{what}: expected [B,{self.in_channels},H,W], got {tuple(b.shape)}")
        if not b.is_cuda:
            raise DaglError(f"CE.{what}: input must be on the GPU; dagl_amd has no CPU path")
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        if self._generic:
            raise DaglError(f"CE.{what}: the graph export serves the default patch geometry (ksize 7, stride_1 4, stride_2 1, "
                            f"inter_channels 16) only; this module was built with ({self.ksize}, {self.stride_1}, {self.stride_2}, "
                            f"{self.inter_channels}), which is out of its scope")
        if torch.cuda.is_current_stream_capturing():
            raise DaglError(f"CE.{what}: not available while the stream is being captured"
                            + (" (the edge count is read on the host)" if what == "graph" else ""))
        k_eff = 0
        if self.select_mode != "adaptive":
            if int(self.select_k) < 1:
                raise DaglError(f"CE: select_k={self.select_k} < 1")
            k_eff = min(int(self.select_k), b.shape[2] * b.shape[3])
        if b.dtype in (torch.bfloat16, torch.float16):
            b = b.float()
        elif b.dtype != torch.float32:
            raise DaglError(f"CE.{what}: unsupported dtype {b.dtype}")
        H, W = b.shape[-2:]
        heads = self.select_mode != "topk"
        with torch.no_grad():
            p = self._params_f32()
            b = b.detach().contiguous()
            hw = (p["thr_conv.weight"], p["thr_conv.bias"], p["bias_conv.weight"], p["bias_conv.bias"]) if heads else (None,) * 4
            if self.in_channels == 64:
                b1p, _, thr, bias = ops.ce_prologue(b, p["g.weight"], p["g.bias"], p["theta.weight"], p["theta.bias"], *hw)
            else:
                from . import train_ops as T
                hw = tuple(_pad_channels4(w) if w is not None and w.dim() == 4 else w for w in hw)
                b1p, _, thr, bias = T.prologue_forward_any_width(_pad_channels4(b).contiguous(), _pad_channels4(p["g.weight"]), p["g.bias"],
                                                                 _pad_channels4(p["theta.weight"]), p["theta.bias"], *hw)
            b1 = b1p[:, 3:3 + H, 3:3 + W, :].permute(0, 3, 1, 2).contiguous()
            csr = ops.ce_graph(b1, thr, bias, p["fc1.0.weight"], p["fc1.0.bias"], p["fc2.0.weight"], p["fc2.0.bias"],
                               mode=self.select_mode, k=k_eff, workspace=self._ws_graph, **kw)
        return csr, k_eff

    def graph(self, b: torch.Tensor, *, scores: bool = False, max_edges=None, rows_per_chunk: int = 0):
        """The patch graph this block builds for ``b`` as a ``PatchGraph`` (CSR over the B*L query rows): per query the keys with
        ``mask_b != 0`` and their weights ``A = softmax(softmax_scale S m) mask_b`` -- the non-zeros of ``yi``, dagl.py:256-261, not
        renormalised --, with ``scores`` also ``S``; every ``select_mode``, any ``in_channels``, half modules on their fp32 copies.

        The export is the reference semantics on the all-fp32 route (the projections and thresholds of ``scan = "exact"``), not a
        record of the lists a screened ``forward`` used: the two agree except at pairs whose score lies within fp32 rounding of the
        selection boundary (the adaptive threshold, the k-th best score).  A diagnostic path: one host synchronisation (the edge
        count), no autograd, the module's state (packed weights, ``_train_dense``, top-k policy, range verdicts) untouched.
        ``max_edges``: raise ``DaglError`` instead of allocating a larger graph (dense at 256^2: 2.7e8 edges, 3.2 GB);
        ``rows_per_chunk``: query rows scored at a time (0 = the library's choice); the result does not depend on it."""
        from .graph import PatchGraph
        csr, k_eff = self._graph_csr(b, "graph", scores=bool(scores), max_edges=max_edges, rows_per_chunk=int(rows_per_chunk))
        score = csr["score"]
        c = self._scale_c()
        if score is not None and c != 1.0:
            score = score / c                        # (the query features carry the factor of _scale_c)
        g = PatchGraph(csr["row_off"], csr["key"], csr["weight"], score, b.shape[0], b.shape[2], b.shape[3], self.select_mode, k_eff)
        g._valid = True                              # (the fill kernels write keys 0 .. N-1 only: ``apply_graph`` need not look again)
        return g

    def degrees(self, b: torch.Tensor) -> torch.Tensor:
        """[B, L] int64: keys per query of ``graph(b)`` -- its count pass alone, nothing read on the host."""
        csr, _ = self._graph_csr(b, "degrees", degrees_only=True)
        off = csr["row_off"]
        return (off[1:] - off[:-1]).view(b.shape[0], -1)

    def _check_given_graph(self, b: torch.Tensor, graph, what: str):
        """The refusals of a call on a given graph (``apply_graph``, ``attend_graph``, ``forward_on_graph``), raised before any launch;
        then ``graph.validate()`` (one host read, once per graph; refused under capture)."""
        from .graph import FixedGraph, PatchGraph
        if isinstance(graph, FixedGraph):
            raise DaglError(f"CE.{what}: a FixedGraph serves refresh_graph and step_graph; this route walks CSR edges: pass "
                            "graph.to_csr()")
        if b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.{what}: expected [B,{self.in_channels},H,W], got {tuple(b.shape)}")
        if not b.is_cuda:
            raise DaglError(f"CE.{what}: input must be on the GPU; dagl_amd has no CPU path")
        if self._generic:
            raise DaglError(f"CE.{what}: applying a graph serves the default patch geometry (ksize 7, stride_1 4, stride_2 1, "
                            f"inter_channels 16) only; this module was built with ({self.ksize}, {self.stride_1}, {self.stride_2}, "
                            f"{self.inter_channels}), which is out of its scope")
        if not isinstance(graph, PatchGraph):
            raise DaglError(f"CE.{what}: a PatchGraph expected, got {type(graph).__name__}")
        B, _, H, W = b.shape
        if (graph.B, graph.H, graph.W) != (B, H, W):
            raise DaglError(f"CE.{what}: the graph was built for B={graph.B} H={graph.H} W={graph.W}, the input is B={B} H={H} W={W}")
        for name in ("row_off", "key", "weight"):
            if getattr(graph, name).device != b.device:
                raise DaglError(f"CE.{what}: graph.{name} lives on {getattr(graph, name).device}, the input on {b.device} "
                                "(PatchGraph.to moves a graph)")
        if b.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise DaglError(f"CE.{what}: unsupported dtype {b.dtype}")
        if not graph._valid:
            if torch.cuda.is_current_stream_capturing():
                raise DaglError(f"CE.{what}: the graph has not been validated and the stream is being captured (validate() reads "
                                "one word on the host): call graph.validate() before the capture")
            graph.validate()

    def apply_graph(self, b: torch.Tensor, graph) -> torch.Tensor:
        """This block's output for ``b`` on a GIVEN patch graph instead of the one it would select: ``fold(A_G . V(theta(b))) / cnt``,
        dagl.py:263-272 with ``yi`` = ``graph`` (a ``PatchGraph``: what ``graph(b)`` returned, edited -- ``select`` / ``with_weight`` --,
        taken from another input or module, or built by hand; keys in any order, repeats add up, any weights).  theta, projection,
        screen, selection and softmax are skipped: the value map ``theta(b)`` is a 1x1 ``train_ops.patch_linear`` (fp32 matrix cores,
        any input width), then ``ops.graph_apply`` (csrc/graph_apply.hip).  ``graph.B / H / W`` must be the input's and its arrays on the
        input's device; ``graph.mode`` / ``k`` are not looked at.  Half / bf16 modules and inputs as in ``forward``.

        ``graph.validate()`` runs first (one host read, once per graph).  After that the call has no host synchronisation and can be
        captured; an unvalidated graph under capture is refused.  With autograd enabled and ``b``, theta's parameters or
        ``graph.weight`` requiring grad, the call is differentiable in exactly those (fp32 parameters only); ``g``, the fc layers and
        the heads are not part of it.  The module's state (packed weights, top-k policy, range verdicts, ``_train_dense``) is untouched."""
        from . import train_ops as T
        self._check_given_graph(b, graph, "apply_graph")
        B, _, H, W = b.shape
        in_dtype = b.dtype
        grad = torch.is_grad_enabled() and (b.requires_grad or graph.weight.requires_grad
                                            or any(p.requires_grad for p in self.theta.parameters()))
        if grad:
            if any(p.dtype != torch.float32 for p in self.parameters()):
                raise DaglError("CE: the differentiable path needs fp32 parameters (the reference's --precision half is a test-time "
                                "switch, DN_Gray/model/__init__.py:98-99); run half-precision modules under torch.no_grad()")
            th_w, th_b = self.theta.weight, self.theta.bias
        else:
            p = self._params_f32(scaled=False)
            th_w, th_b = p["theta.weight"], p["theta.bias"]
        with torch.enable_grad() if grad else torch.no_grad():
            x = b.float() if in_dtype != torch.float32 else b
            xp = T.to_padded_nhwc(_pad_channels4(x), H, W)
            b2 = T.patch_linear(xp, T.conv_weight_rows(_pad_channels4(th_w)), th_b, 1, 1, T.PAD, T.PAD, H, W, allow_fast=False)   # dagl.py:209
            b2p = T.to_padded_nhwc(b2, H, W, True)
            out = _GraphApply.apply(b2p, graph.weight, graph, self._ws_apply, self._ws_apply_bwd)
        return out if in_dtype == torch.float32 else out.to(in_dtype)

    _FP32_ONLY = ("CE: the differentiable path needs fp32 parameters (the reference's --precision half is a test-time "
                  "switch, DN_Gray/model/__init__.py:98-99); run half-precision modules under torch.no_grad()")

    def _graph_features(self, b: torch.Tensor, margin: bool, fast: bool, grad: bool):
        """What the calls on a given graph share once their refusals are through (the caller sets the grad mode): one prologue call,
        fc1 / fc2 on the fp32 route or (``fast``) the training path's split-fp16 kernels, ``tau`` in plain torch
        -> (wq_rows [B,L,196], x_rows [B,N,196], tau [B,L] | None, b2p, poisoned)."""
        from types import SimpleNamespace
        from . import train_ops as T
        B, _, H, W = b.shape
        p = {n: t for n, t in self.named_parameters()} if grad else self._params_f32(scaled=False)
        ks, c = self.ksize, self.inter_channels
        t, _bo = same_pad_amounts(H, ks, self.stride_1)
        l, _r = same_pad_amounts(W, ks, self.stride_1)
        Lh, Lw = -(-H // self.stride_1), -(-W // self.stride_1)
        x = b.float() if b.dtype != torch.float32 else b
        x = _pad_channels4(x.contiguous())
        convs = [SimpleNamespace(weight=_pad_channels4(p[n + ".weight"]), bias=p[n + ".bias"])
                 for n in ("g", "theta") + (("thr_conv", "bias_conv") if margin else ())]
        maps = T.prologue_convs(x, *convs, fast=fast)                                       # dagl.py:208-215
        b1p, b2p = maps[0], maps[1]
        wq_rows = T.patch_linear(b1p, T.fc_weight_rows(p["fc1.0.weight"], c, ks), p["fc1.0.bias"], ks, self.stride_1,
                                 T.PAD - t, T.PAD - l, Lh, Lw, relu=True, allow_fast=fast)    # [B,L,196]
        x_rows = T.patch_linear(b1p, T.fc_weight_rows(p["fc2.0.weight"], c, ks), p["fc2.0.bias"], ks, self.stride_2,
                                0, 0, H, W, relu=True, allow_fast=fast)                       # [B,N,196]
        tau = None
        if margin:
            # mean_j S_ij = <wq_i, mean_j x_j>: linear in the key features, autograd carries the heads and the mean (dagl.py:256-258)
            mean_s = torch.bmm(wq_rows, x_rows.mean(dim=1).unsqueeze(2)).squeeze(2)
            tau = mean_s * maps[2].reshape(B, -1) - maps[3].reshape(B, -1)
        # the split-fp16 kernels NaN-fill ALL they hand out once an operand leaves their range; the margin would turn such rows
        # into "no edge passes" and zeros: one element of each feature matrix carries the verdict into every result instead
        # (t + 0 * wq[0] * x[0], one launch per result)
        poisoned = (lambda t: torch.addcmul(t, wq_rows.detach().reshape(-1)[:1], x_rows.detach().reshape(-1)[:1], value=0.0)) if fast \
            else (lambda t: t)
        return wq_rows, x_rows, tau, b2p, poisoned

    def _attend_arguments(self, b: torch.Tensor, graph, what: str, margin, normalize: str, apply: bool, features: str, fused, backward: str):
        """The refusals of ``attend_graph`` / ``forward_on_graph``, raised before any launch -> (margin, split-fp16 features?, gradient
        wanted?, ``ops.graph_forward``?, ``_GraphForward``?)."""
        self._check_given_graph(b, graph, what)
        if normalize not in ("reference", "edges"):
            raise DaglError(f"CE.{what}: normalize={normalize!r}, expected 'reference' or 'edges'")
        if features not in ("fp32", "split16"):
            raise DaglError(f"CE.{what}: features={features!r}, expected 'fp32' or 'split16'")
        if backward not in ("two_ops", "fused"):
            raise DaglError(f"CE.{what}: backward={backward!r}, expected 'two_ops' or 'fused'")
        fast = features == "split16"
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        margin = self.select_mode != "topk" if margin is None else bool(margin)
        used = [self.g, self.fc1, self.fc2] + ([self.theta] if apply else []) + ([self.thr_conv, self.bias_conv] if margin else [])
        grad = torch.is_grad_enabled() and (b.requires_grad or any(p.requires_grad for m in used for p in m.parameters()))
        fused_train = grad and apply and backward == "fused"
        if grad:
            if fused_train and fused is not None and not fused:
                raise DaglError(f"CE.{what}: fused=False contradicts backward='fused' (the fused backward belongs to the fused forward); "
                                "leave fused at None or pass backward='two_ops'")
            if fused and not fused_train:
                raise DaglError(f"CE.{what}: fused=True has no backward (a gradient is wanted for the input or a parameter); "
                                "fused=None or False keeps the two differentiable ops")
            if any(p.dtype != torch.float32 for p in self.parameters()):
                raise DaglError(self._FP32_ONLY)
        # (None: the fused kernel belongs to the opt-in route -- the default call keeps the bits of the two-op composition)
        fused = apply and not grad and (fast if fused is None else bool(fused))
        return margin, fast, grad, fused, fused_train

    def _attend_on_graph(self, b: torch.Tensor, graph, what: str, margin, normalize: str, apply: bool, features: str = "fp32",
                         fused=False, backward: str = "two_ops"):
        """``attend_graph`` (``apply`` False) and ``forward_on_graph``: one prologue call, fc1 / fc2 on the fp32 route or
        (``features="split16"``) the training path's split-fp16 kernels, ``tau`` in plain torch, then ``_GraphAttend`` and -- ``apply`` --
        ``_GraphApply`` on the same value map, or (``fused``; None = with ``features="split16"`` whenever no gradient is wanted)
        ``ops.graph_forward`` in their place, or (``backward="fused"`` with a gradient wanted) ``_GraphForward``.
        -> (weight, score, out | None); the fused calls return (None, None, out)."""
        margin, fast, grad, fused, fused_train = self._attend_arguments(b, graph, what, margin, normalize, apply, features, fused, backward)
        with torch.enable_grad() if grad else torch.no_grad():
            wq_rows, x_rows, tau, b2p, poisoned = self._graph_features(b, margin, fast, grad)
            if fused_train:
                out = _GraphForward.apply(wq_rows, x_rows, tau, b2p, graph, float(self.softmax_scale), normalize, self._ws_apply,
                                          self._ws_forward_bwd)
                return None, None, poisoned(out)
            if fused:
                out = ops.graph_forward(wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous(), graph.row_off, graph.key,
                                        tau.contiguous() if tau is not None else None, scale=float(self.softmax_scale),
                                        normalize=normalize, workspace=self._ws_apply)
                return None, None, poisoned(out)
            weight, score = _GraphAttend.apply(wq_rows, x_rows, tau, graph, float(self.softmax_scale), normalize,
                                               self._ws_attend, self._ws_attend_bwd)
            out = _GraphApply.apply(b2p, weight, graph, self._ws_apply, self._ws_apply_bwd) if apply else None
            weight, score = poisoned(weight), poisoned(score)
            out = poisoned(out) if apply else None
        return weight, score, out

    def attend_graph(self, b: torch.Tensor, graph, *, margin=None, normalize: str = "reference", features: str = "fp32"):
        """This block's own weights for ``b`` on the STRUCTURE of a given ``PatchGraph``: the same offsets and keys with new ``weight`` and
        ``score`` -- S on the edges, the margin, the reference's softmax restricted to the graph (``ops.graph_attend``,
        csrc/graph_attend.hip).  The structure may be ``graph(b)`` of another input or frame, of another module, edited or hand-built.

        ``margin``: None = the module's mode ("topk": no margin, ``z = softmax_scale S``; "adaptive" / "adaptive_topk": the adaptive rule
        ``m = relu(S - mean(S) thr + bias)``, ``z = softmax_scale S m``, edges with ``m = 0`` weigh 0); True / False override it.
        ``normalize="reference"``: the reference's softmax over all N keys, every key off the graph counting as ``e^0`` -- on the
        structure ``graph(b)`` exports this returns the export's weights; ``"edges"``: a plain softmax over each row's edges.  A row's
        degree counts edges: a repeated key is an entry of its own.  ``score`` is the unscaled S.

        ``features="fp32"``: features come from the fp32 route, as in ``graph``: any ``in_channels``, half / bf16 modules on their fp32
        copies under ``torch.no_grad()``.  ``features="split16"``: the prologue and the two patch projections run as the training path
        runs them when ``scan != "exact"`` (the split-fp16 kernels, forward and -- under autograd -- backward; where those do not serve
        a shape or an input width the calls fall back to fp32 by themselves).  Their range contract is the training path's: an operand
        outside the split-fp16 range (|b1| < 4094, |w_fc| < 64) NaN-fills the result, numbers are never wrong.  Because this call leaves
        the module's state alone there is no automatic move to ``scan="exact"`` and no redo: on a NaN result call again with
        ``features="fp32"``.  With autograd enabled and ``b`` or a parameter of g, fc1, fc2, thr_conv, bias_conv requiring grad, the
        returned ``weight`` carries the autograd graph (fp32 parameters only); the structure is a constant.  The refusals are
        ``apply_graph``'s, raised before any launch; after ``graph.validate()`` there is no host synchronisation.  The module's state
        (packed weights, top-k policy, range verdicts, ``_train_dense``) is untouched."""
        weight, score, _ = self._attend_on_graph(b, graph, "attend_graph", margin, normalize, False, features)
        g = graph.with_weight(weight)
        g.score = score
        return g

    def forward_on_graph(self, b: torch.Tensor, graph, *, margin=None, normalize: str = "reference", features: str = "fp32",
                         fused=None, backward: str = "two_ops") -> torch.Tensor:
        """The block's output for ``b`` with its weights recomputed on the structure of ``graph``: ``apply_graph(b, attend_graph(b, graph))``
        from one prologue call -- differentiable in ``b`` and every parameter of g, theta, fc1, fc2 and (with the margin) thr_conv,
        bias_conv; selection over the L*N pairs is skipped.  Arguments (``features`` and its range contract included), refusals and state
        as ``attend_graph``.

        ``fused``: True = ``ops.graph_forward`` (csrc/graph_forward.hip: scores, softmax and aggregation in one crossing of the edges, no
        ``weight`` / ``score`` arrays) -- refused before any launch when a gradient is wanted, it has no backward; False = the two
        differentiable ops; None = the fused kernel whenever no gradient is wanted on the ``features="split16"`` route, the two ops
        otherwise -- so a call with default arguments returns the bits it always did.  The fused result differs from the two-op one
        by fp32 roundings only.  ``graph.weight`` / ``graph.score`` are left alone either way.

        ``backward`` ("two_ops" or "fused"; anything else is refused before any launch) chooses the differentiable route when a gradient
        is wanted and is only validated otherwise.  "two_ops": the two ops and their backwards, autograd keeps ``score`` and ``weight``
        (two fp32 arrays per edge); ``fused=True`` stays refused.  "fused": ``ops.graph_forward_train`` -- the output carries the bits of
        the no-grad ``fused=True`` call on the same features -- and ``ops.graph_forward_backward``, which recomputes scores and weights in
        one crossing of the edges; autograd keeps twelve bytes per row (the row's maximum and sum) instead.  It serves either
        ``features`` route with its range contract, is differentiable in the same tensors as "two_ops", and takes ``fused=None`` or
        True; ``fused=False`` contradicts it and is refused.  For a sequence: ``g = ce.refresh_graph(frame, g)`` (no gradients), then
        ``ce.forward_on_graph(frame, g, backward="fused")`` under autograd."""
        out = self._attend_on_graph(b, graph, "forward_on_graph", margin, normalize, True, features, fused, backward)[2]
        return out if b.dtype == torch.float32 else out.to(b.dtype)

    def refresh_graph(self, b: torch.Tensor, graph, *, radius: int = 1, margin=None, normalize: str = "reference",
                      features: str = "fp32", propagate: bool = False, explore: int = 0, seed: int = 0):
        """``graph`` moved to the input ``b`` -> a new ``PatchGraph``: every query looks only at the keys in the
        ``(2 radius + 1)^2`` windows around its neighbours in ``graph`` (clipped at the map border; repeats count once), scores those
        candidates exactly and applies this module's selection rule to them (``ops.graph_refresh``, csrc/graph_refresh.hip) -- the
        structure update that costs O(edges) where ``graph`` / ``forward`` scan all L*N pairs.  For a sequence (video frames, bursts,
        recurrent passes over slowly changing features): ``g = ce.refresh_graph(frame, g)``, then ``forward_on_graph(frame, g)``.

        Selection by the module's mode: "adaptive" = the margin ``S - tau > 0``, no rank cut; "topk" = the ``min(select_k, N)`` best
        candidates, no margin; "adaptive_topk" = both; a tie at the last place goes to the lower key.  ``margin`` True / False
        overrides whether ``tau`` is used, ``normalize`` and ``features`` (with its range contract) are ``attend_graph``'s, and so are
        the features and ``tau`` themselves.  Because the adaptive threshold is linear in the key features, the result is exactly the
        reference's mask restricted to the candidates; where the candidates contain the true neighbours --
        ``refresh_graph(x, graph(x))`` -- the result is ``graph(x)``.  ``weight`` is what ``attend_graph`` gives on the new structure,
        ``score`` the unscaled S; the result carries the module's ``mode`` and ``k`` and valid keys.

        ``propagate`` / ``explore`` / ``seed`` (keyword-only, off by default: the call is then exactly the one above) add the two
        candidate sources of ``ops.graph_search``: the neighbours of the four queries adjacent in the stride-4 query grid, shifted by
        the query offset, and ``explore`` (0 .. 256) random keys per query from a stateless hash of (row, ``seed``).  With them a
        graph can improve from call to call and find neighbours again that moved farther than ``radius`` -- selection on the
        candidates stays exact, so the result is still the reference's mask restricted to the candidate set.  Further refusals, before
        any launch: ``explore`` outside 0..256, and ``ops.graph_search_row_bound(largest degree, radius, propagate, explore)`` above
        ``ops.graph_refresh_max_candidates()`` (``code == ERR_UNSUPPORTED``).

        Always under ``torch.no_grad()``: the result is a constant structure with constant weights; gradients are
        ``forward_on_graph``'s job on the result.  Refused before any launch: ``attend_graph``'s refusals (patch geometry, device,
        dtype, shape), a stream under capture (the edge count is read on the host), ``select_k < 1`` in the top-k modes, ``radius``
        outside 0..8, and a graph whose largest degree times ``(2 radius + 1)^2`` exceeds ``ops.graph_refresh_max_candidates()``.  The
        largest degree is read once per graph (kept on the object, as ``validate``'s verdict).  The module's state (packed weights,
        top-k policy, range verdicts, ``_train_dense``) is untouched: the call has a workspace of its own.

        A ``FixedGraph`` (``graph.to_fixed()``) gives a ``FixedGraph``: the same rows bit for bit (``result.to_csr()``), from one row
        launch that reads NOTHING on the host -- no ``validate()``, no ``max_degree()``, no edge count -- and is served under stream
        capture.  See ``step_graph``."""
        from .graph import FixedGraph
        if isinstance(graph, FixedGraph):
            return self._step_fixed(b, graph, "refresh_graph", radius, margin, normalize, features, propagate, explore, seed, False)[1]
        radius, k_eff, margin, longest = self._refresh_arguments(b, graph, "refresh_graph", radius, margin, normalize, features,
                                                                 propagate=propagate, explore=explore, seed=seed)
        B, _, H, W = b.shape
        search = bool(propagate) or explore != 0
        with torch.no_grad():
            wq_rows, x_rows, tau, _b2p, poisoned = self._graph_features(b.detach(), margin, features == "split16", False)
            kw = dict(radius=radius, tau=tau.contiguous() if tau is not None else None, k=k_eff, scale=float(self.softmax_scale),
                      normalize=normalize, max_row_edges=longest, hw=(H, W))
            if search:
                csr = ops.graph_search(wq_rows.contiguous(), x_rows.contiguous(), graph.row_off, graph.key, workspace=self._ws_refresh,
                                       propagate=bool(propagate), explore=explore, seed=seed, **kw)
            else:
                csr = ops.graph_refresh(wq_rows.contiguous(), x_rows.contiguous(), graph.row_off, graph.key, workspace=self._ws_refresh,
                                        **kw)
            return self._refreshed(graph, csr, poisoned, k_eff)

    def _refresh_arguments(self, b: torch.Tensor, graph, what: str, radius, margin, normalize: str, features: str, host_read: bool = True,
                           propagate=False, explore=0, seed=0):
        """The refusals ``refresh_graph`` and ``step_graph`` share, raised before any launch -> (radius, k_eff, margin, largest degree).
        ``host_read`` False (the step without its graph): the call itself reads nothing on the host, so a stream under capture is
        served when what the checks read has been read before -- the graph validated, its largest degree known.
        ``propagate`` / ``explore`` / ``seed``: the search keywords, with their own refusals."""
        ops._graph_search_operands(f"CE.{what}", propagate, explore, seed)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and host_read:
            raise DaglError(f"CE.{what}: not available while the stream is being captured (the edge count is read on the host)")
        self._check_given_graph(b, graph, what)
        if normalize not in ("reference", "edges"):
            raise DaglError(f"CE.{what}: normalize={normalize!r}, expected 'reference' or 'edges'")
        if features not in ("fp32", "split16"):
            raise DaglError(f"CE.{what}: features={features!r}, expected 'fp32' or 'split16'")
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        radius = int(radius)
        if not 0 <= radius <= 8:
            raise DaglError(f"CE.{what}: radius={radius} outside [0, 8]")
        B, _, H, W = b.shape
        k_eff = 0
        if self.select_mode != "adaptive":
            if int(self.select_k) < 1:
                raise DaglError(f"CE: select_k={self.select_k} < 1")
            k_eff = min(int(self.select_k), H * W)
        margin = self.select_mode != "topk" if margin is None else bool(margin)
        if capturing and graph._max_degree is None:
            raise DaglError(f"CE.{what}: the graph's largest degree is not known and the stream is being captured (max_degree() reads "
                            "one word on the host): call graph.max_degree() before the capture")
        longest, cap = graph.max_degree(), ops.graph_refresh_max_candidates()
        if longest * (2 * radius + 1) ** 2 > cap:
            err = DaglError(f"CE.{what}: the graph's largest degree {longest} times (2 radius + 1)^2 = {(2 * radius + 1) ** 2} is "
                            f"{longest * (2 * radius + 1) ** 2} candidates, a row may expand into {cap}")
            err.code = ERR_UNSUPPORTED
            raise err
        if (propagate or explore) and ops.graph_search_row_bound(longest, radius, propagate, explore) > cap:
            err = DaglError(f"CE.{what}: with propagate={bool(propagate)} and explore={explore} a row of the graph (largest degree "
                            f"{longest}, radius {radius}) may expand into (1 + 4 propagate) {longest} (2 radius + 1)^2 + explore = "
                            f"{ops.graph_search_row_bound(longest, radius, propagate, explore)} candidates, more than {cap}")
            err.code = ERR_UNSUPPORTED
            raise err
        return radius, k_eff, margin, longest

    def _refreshed(self, graph, csr: dict, poisoned, k_eff: int):
        """The ``PatchGraph`` of a refresh's arrays: this module's ``mode`` and ``k``, valid keys, no second host read."""
        g = graph._like(csr["row_off"], csr["key"], poisoned(csr["weight"]), poisoned(csr["score"]))
        g.mode, g.k = self.select_mode, k_eff
        g._valid = True                              # (every candidate is a key of the map)
        return g

    def step_graph(self, b: torch.Tensor, graph, *, radius: int = 1, margin=None, normalize: str = "reference", features: str = "fp32",
                   want_graph: bool = True, propagate: bool = False, explore: int = 0, seed: int = 0):
        """A sequence step in one call -> ``(out, PatchGraph | None)``: ``graph`` moved to the input ``b`` exactly as
        ``refresh_graph(b, graph, radius=..., margin=..., normalize=..., features=...)`` moves it (the same bits in every array, the same
        ``mode``, ``k`` and valid keys), and the block's output for ``b`` on that result, ``fold(A . V(theta(b))) / cnt`` with the new
        graph's fp32 weights -- from ONE prologue and projection pass and one scoring of the candidates (``ops.graph_step``,
        csrc/graph_refresh.hip), where ``refresh_graph`` followed by ``forward_on_graph`` computes the features twice and scores the
        kept edges a second time.  For a sequence: ``out, g = ce.step_graph(frame, g)``.

        ``out`` [B,16,H,W] has the input's dtype; each element of an aggregated row is one fp32 fmaf chain over the row's kept keys in
        ascending order, so ``out`` carries the same bits with ``want_graph`` True or False and on every repeat; it differs from
        ``forward_on_graph`` on the returned graph by the order of fp32 sums alone.  A query whose row comes out empty contributes zeros.

        ``want_graph=False`` returns ``(out, None)``: the structure of a key frame is kept and only the output is wanted on each
        following frame.  That form reads nothing on the host and can be captured into a HIP graph once the graph has been validated and
        its largest degree read (``graph.validate()``, ``graph.max_degree()``; ``CE.graph`` validates its result); otherwise it is refused
        under capture before any launch.  ``want_graph=True`` makes the one host read ``refresh_graph`` makes and is refused under capture.

        ``propagate`` / ``explore`` / ``seed`` are ``refresh_graph``'s search keywords (``ops.graph_search_step``); off by default, the
        call is then exactly the one above.  ``seed`` is a launch argument: a captured ``want_graph=False`` call replays the seed it
        was captured with, every replay explores the same keys.

        Always under ``torch.no_grad()``, ``out.requires_grad`` is False: gradients are ``forward_on_graph``'s job on the returned graph.
        Arguments, selection, the ``features="split16"`` range contract (both results NaN-filled, never wrong numbers) and refusals are
        ``refresh_graph``'s, all raised before any launch.  The module's state (packed weights, top-k policy, range verdicts,
        ``_train_dense``) is untouched: the call has a workspace of its own.

        On a ``FixedGraph`` (``graph.to_fixed()``: ``width`` slots per row) the call returns ``(out, FixedGraph | None)`` from ONE row
        launch and the fold (``ops.graph_step_fixed``): ``out`` and the rows of the new graph carry the bits of the call on the CSR
        (``new.to_csr()``).  The output width is ``k`` in the rank-cut modes ("topk", "adaptive_topk") and ``graph.width`` in
        "adaptive".  Nothing is read on the host -- no ``validate()``, no ``max_degree()``, no edge count --, so the call is served
        under stream capture WITH ``want_graph=True``: capture ``out, g_new = ce.step_graph(x, g); g.copy_(g_new)`` once and replay it
        per frame.  In "adaptive" mode a row that keeps more than ``graph.width`` entries comes out EMPTY (never truncated); such rows
        are counted on the device, not reported: choose the width with room, or use a rank-cut mode, where no row can overflow.
        Refused before any launch: a graph that does not fit the input, and ``ops.graph_search_row_bound(graph.width, radius,
        propagate, explore)`` above ``ops.graph_refresh_max_candidates()``."""
        from .graph import FixedGraph
        if isinstance(graph, FixedGraph):
            out, new = self._step_fixed(b, graph, "step_graph", radius, margin, normalize, features, propagate, explore, seed, True)
            return out, (new if want_graph else None)
        want_graph = bool(want_graph)
        radius, k_eff, margin, longest = self._refresh_arguments(b, graph, "step_graph", radius, margin, normalize, features,
                                                                 host_read=want_graph, propagate=propagate, explore=explore, seed=seed)
        B, _, H, W = b.shape
        search = bool(propagate) or explore != 0
        with torch.no_grad():
            wq_rows, x_rows, tau, b2p, poisoned = self._graph_features(b.detach(), margin, features == "split16", False)
            kw = dict(radius=radius, tau=tau.contiguous() if tau is not None else None, k=k_eff, scale=float(self.softmax_scale),
                      normalize=normalize, max_row_edges=longest, want_graph=want_graph, hw=(H, W))
            if search:
                out, csr, _status = ops.graph_search_step(wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous(), graph.row_off,
                                                          graph.key, workspace=self._ws_step, propagate=bool(propagate),
                                                          explore=explore, seed=seed, **kw)
            else:
                out, csr, _status = ops.graph_step(wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous(), graph.row_off, graph.key,
                                                   workspace=self._ws_step, **kw)
            out = poisoned(out)
            if b.dtype != torch.float32:
                out = out.to(b.dtype)
            return out, (self._refreshed(graph, csr, poisoned, k_eff) if want_graph else None)

    def _fixed_arguments(self, b: torch.Tensor, graph, what: str, radius, margin, normalize: str, features: str, propagate=False,
                         explore=0, seed=0):
        """The refusals of ``refresh_graph`` / ``step_graph`` on a ``FixedGraph``, raised before any launch -> (radius, k_eff, margin,
        width_out, propagate, explore, seed).  None of them reads the graph's arrays: no host read, served under capture."""
        propagate, explore, seed = ops._graph_search_operands(f"CE.{what}", propagate, explore, seed)
        if b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.{what}: expected [B,{self.in_channels},H,W], got {tuple(b.shape)}")
        if not b.is_cuda:
            raise DaglError(f"CE.{what}: input must be on the GPU; dagl_amd has no CPU path")
        if self._generic:
            raise DaglError(f"CE.{what}: a graph step serves the default patch geometry (ksize 7, stride_1 4, stride_2 1, "
                            f"inter_channels 16) only; this module was built with ({self.ksize}, {self.stride_1}, {self.stride_2}, "
                            f"{self.inter_channels}), which is out of its scope")
        B, _, H, W = b.shape
        if (graph.B, graph.H, graph.W) != (B, H, W):
            raise DaglError(f"CE.{what}: the graph was built for B={graph.B} H={graph.H} W={graph.W}, the input is B={B} H={H} W={W}")
        if graph.device != b.device:
            raise DaglError(f"CE.{what}: the graph lives on {graph.device}, the input on {b.device} (FixedGraph.to moves a graph)")
        if b.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise DaglError(f"CE.{what}: unsupported dtype {b.dtype}")
        if normalize not in ("reference", "edges"):
            raise DaglError(f"CE.{what}: normalize={normalize!r}, expected 'reference' or 'edges'")
        if features not in ("fp32", "split16"):
            raise DaglError(f"CE.{what}: features={features!r}, expected 'fp32' or 'split16'")
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        radius = int(radius)
        if not 0 <= radius <= 8:
            raise DaglError(f"CE.{what}: radius={radius} outside [0, 8]")
        k_eff = 0
        if self.select_mode != "adaptive":
            if int(self.select_k) < 1:
                raise DaglError(f"CE: select_k={self.select_k} < 1")
            k_eff = min(int(self.select_k), H * W)
        margin = self.select_mode != "topk" if margin is None else bool(margin)
        bound, cap = ops.graph_search_row_bound(graph.width, radius, propagate, explore), ops.graph_refresh_max_candidates()
        if bound > cap:
            err = DaglError(f"CE.{what}: a row of {graph.width} slots at radius {radius} with propagate={bool(propagate)} and "
                            f"explore={explore} may expand into {bound} candidates, more than {cap}")
            err.code = ERR_UNSUPPORTED
            raise err
        return radius, k_eff, margin, (k_eff if k_eff > 0 else graph.width), propagate, explore, seed

    def _step_fixed(self, b: torch.Tensor, graph, what: str, radius, margin, normalize: str, features: str, propagate, explore, seed,
                    apply: bool):
        """``refresh_graph`` / ``step_graph`` (``apply``) on a ``FixedGraph`` -> (out | None, FixedGraph): ``ops.graph_step_fixed`` on
        the module's features."""
        from .graph import FixedGraph
        radius, k_eff, margin, width_out, propagate, explore, seed = self._fixed_arguments(b, graph, what, radius, margin, normalize,
                                                                                           features, propagate, explore, seed)
        B, _, H, W = b.shape
        with torch.no_grad():
            wq_rows, x_rows, tau, b2p, poisoned = self._graph_features(b.detach(), margin, features == "split16", False)
            out, arrays, _status = ops.graph_step_fixed(wq_rows.contiguous(), x_rows.contiguous(), b2p.contiguous() if apply else None,
                                                        graph.key, graph.deg, width_out=width_out, radius=radius,
                                                        tau=tau.contiguous() if tau is not None else None, k=k_eff,
                                                        scale=float(self.softmax_scale), normalize=normalize, propagate=bool(propagate),
                                                        explore=explore, seed=seed, workspace=self._ws_step, hw=(H, W))
            new = FixedGraph._like(graph, arrays["key"], poisoned(arrays["weight"]), poisoned(arrays["score"]), arrays["deg"])
            new.mode, new.k = self.select_mode, k_eff
            if apply:
                out = poisoned(out)
                if b.dtype != torch.float32:
                    out = out.to(b.dtype)
            return out, new

    def build_graph(self, b: torch.Tensor, *, iters: int = 4, radius: int = 1, explore: int = 8, seed: int = 0, features: str = "fp32",
                    normalize: str = "reference"):
        """A ``PatchGraph`` for ``b`` WITHOUT any scan of the L*N pairs: the search step iterated from a trivial start.  The initial
        graph holds one edge per query, the key at the query patch's own position (the patch origin of ``synth.query_grid`` + 3, clamped
        to the map); then ``iters`` times ``refresh_graph(b, g, radius=radius, propagate=True, explore=explore, seed=seed + i,
        features=features, normalize=normalize)``, i = 0 .. iters - 1, on features computed once -- the last result is returned, bit for
        bit what those public calls give, with the module's ``mode`` and ``k`` and valid keys.  Every iteration keeps the previous
        keys among its candidates and selects exactly, so in the top-k modes a row's kept scores never get worse from one iteration
        to the next; how close the result comes to ``graph(b)`` depends on the input (``tools/time_patch_graph.py --search`` prints the
        recall per iteration).

        Every ``select_mode``; the refusals are ``refresh_graph``'s, looked at again before every iteration: an adaptive mask that
        grows until ``ops.graph_search_row_bound`` passes ``ops.graph_refresh_max_candidates()`` raises ``DaglError`` with
        ``code == ERR_UNSUPPORTED`` -- a row is never truncated.  ``iters`` >= 1.  One host read per iteration; always under
        ``torch.no_grad()``; the module's state is untouched."""
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise DaglError(f"CE.build_graph: iters={iters!r}, an int >= 1 expected")
        ops._graph_search_operands("CE.build_graph", True, explore, seed)
        if not isinstance(b, torch.Tensor) or b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.build_graph: expected [B,{self.in_channels},H,W], got {tuple(getattr(b, 'shape', ()))}")
        if not b.is_cuda:
            raise DaglError("CE.build_graph: input must be on the GPU; dagl_amd has no CPU path")
        if torch.cuda.is_current_stream_capturing():
            raise DaglError("CE.build_graph: not available while the stream is being captured (the edge count is read on the host)")
        B, _, H, W = b.shape
        with torch.no_grad():
            g = self._build_start(B, H, W, b.device)
            feats = None
            for i in range(iters):
                r, k_eff, margin, longest = self._refresh_arguments(b, g, "build_graph", radius, None, normalize, features,
                                                                    propagate=True, explore=explore, seed=seed + i)
                if feats is None:
                    wq_rows, x_rows, tau, _b2p, poisoned = self._graph_features(b.detach(), margin, features == "split16", False)
                    feats = (wq_rows.contiguous(), x_rows.contiguous(), tau.contiguous() if tau is not None else None)
                csr = ops.graph_search(feats[0], feats[1], g.row_off, g.key, radius=r, tau=feats[2], k=k_eff,
                                       scale=float(self.softmax_scale), normalize=normalize, max_row_edges=longest,
                                       workspace=self._ws_refresh, hw=(H, W), propagate=True, explore=explore, seed=seed + i)
                g = self._refreshed(g, csr, poisoned, k_eff)
            return g

    def _build_start(self, B: int, H: int, W: int, device):
        """``build_graph``'s start (``graph.trivial_graph`` at this module's patch geometry and mode; ``SequenceState.start`` holds
        twelve of them)."""
        from .graph import trivial_graph
        return trivial_graph(B, H, W, device, self.select_mode, self.ksize, self.stride_1)

    def forward_with_graph(self, b: torch.Tensor, *, scores: bool = False, features=None):
        """The block's output for ``b`` AND the patch graph that produced it, from one call -> ``(out, PatchGraph)``: the list-form route
        of the differentiable forward (prologue, fc1 / fc2, the graph core over each query's neighbour list), whose lists
        ``ops.graph_from_lists`` (csrc/graph_lists.hip) turns into the CSR of ``graph`` -- the very neighbours this call aggregated,
        at about the cost of a forward instead of ``graph``'s all-fp32 scan of the L*N pairs.

        ``features``: "split16" = the prologue and the projections on the split-fp16 kernels, the selection behind the bf16 screen (the
        route of ``scan = "screened"``); "fp32" = all on the fp32 route (``scan = "exact"``), which differs from ``graph`` in summation
        order only; None = "split16" unless ``self.scan == "exact"``.  The range contract of "split16" is ``attend_graph``'s: an operand
        outside the split-fp16 range NaN-fills ``out``, ``weight`` and ``score`` (the structure still holds valid keys only), the module's
        state is left alone, the caller repeats with ``features="fp32"``.

        ``out`` is that route's output; with autograd enabled and ``b`` or a parameter requiring grad (fp32 parameters only) it
        carries the autograd graph of the module's own differentiable forward -- same kernels, same bits.  The graph's arrays are
        constants: ``weight = exp(l) / Z`` with the unlisted keys' e^0 in Z, i.e. ``A = softmax(softmax_scale S m) mask_b``; ``scores``:
        also ``S``; ``mode`` / ``k`` the module's, keys valid (``apply_graph`` need not look again).

        Scope: what the lists serve.  Refused before any launch: a non-default patch geometry, ``min(select_k, N) > 64`` (``graph`` is the
        export for those), a stream under capture (the edge count is read on the host), and ``graph``'s refusals for dtype, shape and
        device.  An adaptive mask that keeps more than 64 keys for some query is found by the core and raised as a ``DaglError`` with
        ``code == ERR_UNSUPPORTED``: there is no silent move to ``graph``'s route, the caller decides.  The module's state (packed
        weights, top-k policy, range verdicts, ``_train_dense``, ``last_info``) is untouched: the call has workspaces of its own."""
        from types import SimpleNamespace
        from . import train_ops as T
        from .graph import PatchGraph
        what = "forward_with_graph"
        if b.dim() != 4 or b.shape[1] != self.in_channels:
            raise DaglError(f"CE.{what}: expected [B,{self.in_channels},H,W], got {tuple(b.shape)}")
        if not b.is_cuda:
            raise DaglError(f"CE.{what}: input must be on the GPU; dagl_amd has no CPU path")
        if self.select_mode not in ("adaptive", "topk", "adaptive_topk"):
            raise DaglError(f"CE.select_mode {self.select_mode!r}: expected 'adaptive', 'topk' or 'adaptive_topk'")
        if self._generic:
            raise DaglError(f"CE.{what}: the graph export serves the default patch geometry (ksize 7, stride_1 4, stride_2 1, "
                            f"inter_channels 16) only; this module was built with ({self.ksize}, {self.stride_1}, {self.stride_2}, "
                            f"{self.inter_channels}), which is out of its scope")
        if torch.cuda.is_current_stream_capturing():
            raise DaglError(f"CE.{what}: not available while the stream is being captured (the edge count is read on the host)")
        B, _, H, W = b.shape
        k_eff = 0
        if self.select_mode != "adaptive":
            if int(self.select_k) < 1:
                raise DaglError(f"CE: select_k={self.select_k} < 1")
            k_eff = min(int(self.select_k), H * W)
            if k_eff > MAX_TOPK:
                raise DaglError(f"CE.{what}: min(select_k, N) = {k_eff} neighbours per query, the neighbour lists hold {MAX_TOPK}; "
                                "CE.graph is the export for wider neighbourhoods")
        if features is None:
            features = "fp32" if self.scan == "exact" else "split16"
        if features not in ("fp32", "split16"):
            raise DaglError(f"CE.{what}: features={features!r}, expected 'fp32' or 'split16'")
        fast = features == "split16"
        in_dtype = b.dtype
        if in_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise DaglError(f"CE.{what}: unsupported dtype {in_dtype}")
        grad = torch.is_grad_enabled() and (b.requires_grad or any(p.requires_grad for p in self.parameters()))
        if grad:
            if any(p.dtype != torch.float32 for p in self.parameters()):
                raise DaglError(self._FP32_ONLY)
            p = {n: t for n, t in self.named_parameters()}
        else:
            p = self._params_f32(scaled=False)
        heads = self.select_mode != "topk"
        ks, c = self.ksize, self.inter_channels
        t, _bo = same_pad_amounts(H, ks, self.stride_1)
        l, _r = same_pad_amounts(W, ks, self.stride_1)
        Lh, Lw = -(-H // self.stride_1), -(-W // self.stride_1)
        lists = {}
        fwd, bwd = _lists_route(self.select_mode, k_eff, not fast, self._ws_lists, self._ws_lists_bwd)

        def fwd_keeping_lists(*operands):
            out, saved, info = fwd(*operands)
            lists.update(zip(("nb_idx", "nb_wgt", "nb_s", "nb_cnt"), saved))
            return out, saved, info

        with torch.enable_grad() if grad else torch.no_grad():
            # the calls of _forward_train's list-form route, one for one (dagl.py:208-272)
            x = b.float() if in_dtype != torch.float32 else b
            x = _pad_channels4(x.contiguous())
            convs = [SimpleNamespace(weight=_pad_channels4(p[n + ".weight"]), bias=p[n + ".bias"])
                     for n in ("g", "theta") + (("thr_conv", "bias_conv") if heads else ())]
            maps = T.prologue_convs(x, *convs, fast=fast)
            b1p, b2p = maps[0], maps[1]
            thr, bias = (maps[2], maps[3]) if heads else (None, None)
            b2 = b2p[:, T.PAD:T.PAD + H, T.PAD:T.PAD + W, :].permute(0, 3, 1, 2)
            wq_rows = T.patch_linear(b1p, T.fc_weight_rows(p["fc1.0.weight"], c, ks), p["fc1.0.bias"], ks, self.stride_1,
                                     T.PAD - t, T.PAD - l, Lh, Lw, relu=True, allow_fast=fast)    # [B,L,196]
            x_rows = T.patch_linear(b1p, T.fc_weight_rows(p["fc2.0.weight"], c, ks), p["fc2.0.bias"], ks, self.stride_2,
                                    0, 0, H, W, relu=True, allow_fast=fast)                       # [B,N,196]
            sc = self._scale_c()
            if sc != 1.0:                   # softmax_scale != 10: see _scale_c
                wq_rows = wq_rows * sc
                if bias is not None:
                    bias = bias * sc
            try:
                out = _GraphCore.apply(wq_rows, x_rows, b2, thr, bias, (fwd_keeping_lists, bwd), {})
            except DaglError as e:
                if self.select_mode != "adaptive" or e.code != ERR_UNSUPPORTED:
                    raise
                err = DaglError(f"CE.{what}: an adaptive mask keeps more than {FAST_CAP} keys for some query, more than a neighbour "
                                f"list holds; CE.graph is the export for such neighbourhoods ({e})")
                err.code = ERR_UNSUPPORTED
                raise err from None
            # (as in _attend_on_graph: the split-fp16 kernels NaN-fill the features once an operand leaves their range; one element
            # of each feature matrix carries that verdict into every result)
            poisoned = (lambda v: torch.addcmul(v, wq_rows.detach().reshape(-1)[:1], x_rows.detach().reshape(-1)[:1], value=0.0)) if fast \
                else (lambda v: v)
            out = poisoned(out)
            with torch.no_grad():
                csr = ops.graph_from_lists(lists["nb_idx"], lists["nb_wgt"], lists["nb_s"] if scores else None, lists["nb_cnt"],
                                           (H, W), workspace=self._ws_lists_csr)
                weight, score = poisoned(csr["weight"]), csr["score"]
                if score is not None:
                    score = poisoned(score / sc if sc != 1.0 else score)     # (the query features carry the factor of _scale_c)
        g = PatchGraph(csr["row_off"], csr["key"], weight, score, B, H, W, self.select_mode, k_eff)
        g._valid = True                              # (graph_from_lists drops every key outside [0, N))
        return (out if in_dtype == torch.float32 else out.to(in_dtype)), g

    def _forward_infer_generic(self, b: torch.Tensor, k_eff: int) -> torch.Tensor:
        """A module built with non-default ``ksize / stride_1 / stride_2 / inter_channels`` (dagl.py:175-176): the whole method through
        ``dagl_ce_generic_forward`` (csrc/generic.hip).  ``softmax_scale`` goes to the kernel as it is (no scaled parameter copies);
        an input width that is not a multiple of 4 gets zero channels (and zero weight columns), which change nothing."""
        p = self._params_f32(scaled=False)
        b = _pad_channels4(b)
        for n in _CONV_WEIGHTS:
            p[n] = _pad_channels4(p[n])
        with torch.no_grad():
            out, deg = ops.ce_forward_generic(b.contiguous(), p, self.ksize, self.stride_1, self.stride_2, self.inter_channels,
                                              mode=self.select_mode, k=k_eff, softmax_scale=float(self.softmax_scale),
                                              workspace=self._ws, want_degree=True)
        self._last_call = None
        self._pack_key = None                      # the shared workspace holds another layout now
        self.last_info = dict(path=7, degree=deg)  # (device tensor [B,L]: reading it is the caller's synchronisation)
        return out

    def _forward_train_generic(self, b: torch.Tensor, k_eff: int) -> torch.Tensor:
        """Differentiable route of a module with a non-default patch geometry: every convolution / Linear-over-patches as unfold + fp32
        matrix-core product with explicit adjoints (train_ops.patch_linear: any window, stride, channel count), the graph core as
        ``_generic_route``.  Layout plumbing (NCHW -> zero-bordered NHWC) is torch's: autograd carries it."""
        from . import train_ops as T
        if any(p.dtype != torch.float32 for p in self.parameters()):
            raise DaglError("CE: the differentiable path needs fp32 parameters")
        B, Cin, H, W = b.shape
        ks, s1, s2, c = int(self.ksize), int(self.stride_1), int(self.stride_2), int(self.inter_channels)
        pg = ops.generic_border(ks)
        t1, l1 = same_pad_amounts(H, ks, s1)[0], same_pad_amounts(W, ks, s1)[0]
        t2, l2 = same_pad_amounts(H, ks, s2)[0], same_pad_amounts(W, ks, s2)[0]
        Lh, Lw, Nh, Nw = -(-H // s1), -(-W // s1), -(-H // s2), -(-W // s2)
        def wrows(m):
            return T.conv_weight_rows(_pad_channels4(m.weight))
        def nhwc_bordered(t_nchw):                    # [B,C,H,W] -> zero-bordered NHWC (border pg)
            return F.pad(t_nchw.permute(0, 2, 3, 1), (0, 0, pg, pg, pg, pg)).contiguous()
        xp = nhwc_bordered(_pad_channels4(b))
        heads = self.select_mode != "topk"
        b1 = T.patch_linear(xp, wrows(self.g), self.g.bias, 3, 1, pg - 1, pg - 1, H, W, allow_fast=False)             # [B, H*W, c]   dagl.py:208
        b2 = T.patch_linear(xp, wrows(self.theta), self.theta.bias, 1, 1, pg, pg, H, W, allow_fast=False)               # dagl.py:209
        thr = bias = None
        if heads:                                                                                                        # dagl.py:213-215
            thr = T.patch_linear(xp, wrows(self.thr_conv), self.thr_conv.bias, ks, s1, pg - t1, pg - l1, Lh, Lw, allow_fast=False).reshape(B, -1)
            bias = T.patch_linear(xp, wrows(self.bias_conv), self.bias_conv.bias, ks, s1, pg - t1, pg - l1, Lh, Lw, allow_fast=False).reshape(B, -1)
        b1p = F.pad(b1.view(B, H, W, c), (0, 0, pg, pg, pg, pg)).contiguous()
        b2p = F.pad(b2.view(B, H, W, c), (0, 0, pg, pg, pg, pg)).contiguous()
        wq_rows = T.patch_linear(b1p, T.fc_weight_rows(self.fc1[0].weight, c, ks), self.fc1[0].bias, ks, s1, pg - t1, pg - l1, Lh, Lw,
                                 relu=True, allow_fast=False)                                                          # dagl.py:248
        x_rows = T.patch_linear(b1p, T.fc_weight_rows(self.fc2[0].weight, c, ks), self.fc2[0].bias, ks, s2, pg - t2, pg - l2, Nh, Nw,
                                relu=True, allow_fast=False)                                                           # dagl.py:249
        self._last_call = None
        self._pack_key = None
        route = _generic_route((H, W, ks, s1, s2), self.select_mode, k_eff, float(self.softmax_scale), self._ws, self._ws_bwd)
        return _GraphCore.apply(wq_rows, x_rows, b2p, thr, bias, route, None)

    def _forward_infer_any_width(self, b: torch.Tensor, k_eff: int) -> torch.Tensor:
        """``CE(in_channels = n_feats)`` for n_feats != 64 (CES builds every head that way, dagl.py:94-109; ``--n_feats``,
        DN_Gray/option.py:70): the fused prologue kernels are laid out for 64 input channels, so the four prologue convolutions
        run as unfold + fp32 matrix-core GEMM on the HIP library (train_ops.prologue_forward_any_width) and everything behind
        them -- projections, selection, edge softmax, gather, fold: the 16-channel maps do not know the input width -- through
        ``dagl_ce_forward`` (include/dagl_ce.h), the C ABI's channel-agnostic entry point."""
        from . import train_ops as T
        p = self._params_f32()
        heads = self.select_mode != "topk"
        b = _pad_channels4(b)
        for n in _CONV_WEIGHTS:
            p[n] = _pad_channels4(p[n])
        hw = (p["thr_conv.weight"], p["thr_conv.bias"], p["bias_conv.weight"], p["bias_conv.bias"]) if heads else (None,) * 4
        b1p, b2p, thr, bias = T.prologue_forward_any_width(b.contiguous(), p["g.weight"], p["g.bias"], p["theta.weight"],
                                                           p["theta.bias"], *hw)
        H, W = b.shape[-2:]
        b1 = b1p[:, T.PAD:T.PAD + H, T.PAD:T.PAD + W, :].permute(0, 3, 1, 2).contiguous()
        b2 = b2p[:, T.PAD:T.PAD + H, T.PAD:T.PAD + W, :].permute(0, 3, 1, 2).contiguous()
        tight, sampled = self._topk_threshold()
        out, info = ops.ce_forward(b1, b2, thr, bias, p["fc1.0.weight"], p["fc1.0.bias"], p["fc2.0.weight"], p["fc2.0.bias"],
                                   mode=self.select_mode, k=k_eff, workspace=self._ws, return_info=True,
                                   exact_scan=(self.scan == "exact"), profile=self.profile, tight_topk=tight, sampled_topk=sampled)
        self._last_call = None                     # (this entry point reads its statistics back every call: nothing to poll)
        self.last_info = info
        if info.get("range_fallback"):
            self._note_range_violation("a call left the split-fp16 range and was re-run on the fp32 path")
        return out

    def _forward_infer(self, b: torch.Tensor, k_eff: int) -> torch.Tensor:
        """The inference kernels (``dagl_ce_forward_fused``): fp32 [B,64,H,W] in, fp32 [B,16,H,W] out, no autograd."""
        if self.in_channels != 64:
            return self._forward_infer_any_width(b, k_eff)
        params = self._params_f32()
        # the packed copies of fc1/fc2 and of the g / theta convolutions live in this module's private workspace: skip
        # repacking while neither the weights (torch bumps ._version on every in-place update) nor the call geometry changed
        wsb = self._ws.peek(b.device)
        src = dict(self.named_parameters())       # (keyed on the module's own tensors: the fp32 copies of half weights follow them)
        key = (tuple(b.shape), self.select_mode, k_eff, self.scan, self._pack_epoch, self._scale_c(),
               tuple((src[n].data_ptr(), src[n]._version) for n in ("fc1.0.weight", "fc2.0.weight", "g.weight", "theta.weight")),
               wsb.data_ptr() if wsb is not None else 0)
        # dense regime: the edge statistics (and with them a host synchronisation) are only fetched every 16th call, to
        # notice when the neighbourhoods have become sparse again
        hint = self._dense_hint and self.select_mode == "adaptive" and self.scan != "exact"
        self._dense_calls = self._dense_calls + 1 if hint else 0
        want_info = (not hint) or (self._dense_calls % 16 == 1) or self.profile is not None
        if self._served_shape != tuple(b.shape):
            if self._served_shape is not None:
                self._served_streaks[self._served_shape] = self._served_streak
            self._served_shape = tuple(b.shape)
            self._served_streak = self._served_streaks.get(self._served_shape, 0)
        no_wait = (self.select_mode == "adaptive" and self.scan != "exact" and not hint and self.adaptive_sync == "auto"
                   and self._served_streak >= 4 and key == self._pack_key and self.profile is None)
        tight, sampled = self._topk_threshold()
        topk_screen = self.select_mode != "adaptive" and self.scan != "exact"
        if self.topk_redo not in ("auto", "always"):
            raise DaglError(f"CE.topk_redo {self.topk_redo!r}: expected 'auto' or 'always'")
        no_redo = (topk_screen and self.topk_redo == "auto" and self._redo_skip and not self._redo_banned and key == self._pack_key
                   and not torch.cuda.is_current_stream_capturing())
        if key != self._pack_key:
            self._redo_skip, self._redo_clean_polls = False, 0     # another shape / weights / workspace: what the polls saw no longer applies
            if self.scan != "exact" and key[6] != (self._pack_key[6] if self._pack_key else None) and not torch.cuda.is_current_stream_capturing():
                # new weights are about to be packed as fp16 pairs (256 w_conv, 1024 w_fc): beyond |w_conv| < 234 / |w_fc| < 58 -- never
                # seen on a trained DAGL -- the module takes the fp32 path from its first call (one synchronisation per weight set; the
                # activations have no such limit since round 6: include/dagl_ce.h)
                wmax = torch.stack([params[n].abs().max() for n in ("g.weight", "theta.weight", "fc1.0.weight", "fc2.0.weight")]).tolist()
                if not (wmax[0] < 230.0 and wmax[1] < 230.0 and wmax[2] < 57.0 and wmax[3] < 57.0):
                    self._note_range_violation("weights beyond the split-fp16 range (|w_conv| < 234, |w_fc| < 58)")
                    return self._forward_infer(b, k_eff)
        out, info = ops.ce_forward_fused(b.contiguous(), params, mode=self.select_mode, k=k_eff,
                                         workspace=self._ws, profile=self.profile,
                                         exact_scan=(self.scan == "exact"), weights_packed=(key == self._pack_key),
                                         dense_hint=hint, want_info=want_info, no_wait=no_wait, tight_topk=tight,
                                         sampled_topk=sampled, no_redo=no_redo)
        self._pack_key = key[:-1] + (self._ws.peek(b.device).data_ptr(),)
        self._last_call = (tuple(b.shape), b.device)
        if no_wait:
            self._nowait_calls += 1
            if self._nowait_calls >= 16 and not torch.cuda.is_current_stream_capturing():
                self._nowait_calls = 0
                self.range_ok()                    # (one synchronisation: sticky verdict + range word since the last poll)
        elif self.select_mode == "adaptive" and info is not None:
            served = info.get("path") == 3 and not info.get("range_fallback")
            self._served_streak = self._served_streak + 1 if served else 0
        if info is not None and info.get("range_fallback"):
            self._note_range_violation("an adaptive call left the split-fp16 range and was re-run on the fp32 path")
        elif self.select_mode != "adaptive" and self.scan != "exact":
            # no host round trip in the top-k modes: look at the range word every 64th call (one synchronisation); a call
            # that left the range has returned NaN (never wrong numbers), the module moves to the fp32 path from here on
            self._calls_since_range_check += 1
            if self._calls_since_range_check >= (32 if no_redo else 64) and not torch.cuda.is_current_stream_capturing():
                self.range_ok()
        if info is not None:
            self.last_info = info
            if self.select_mode == "adaptive":
                n_pairs = b.shape[0] * (-(-b.shape[2] // 4)) * (-(-b.shape[3] // 4)) * b.shape[2] * b.shape[3]
                # stay on the dense formulation while the optimistic lists would end there again: most queries beyond the
                # lists' width (the dense call counts them), or a mask that keeps more than 1/96 of all pairs (the library's
                # own limit for redoing the overflowed queries one by one)
                n_q = b.shape[0] * (-(-b.shape[2] // 4)) * (-(-b.shape[3] // 4))
                self._dense_hint = info["path"] == 4 and (96 * info["total_edges"] > n_pairs or
                                                          2 * info.get("redone_queries", 0) > n_q)
        return out
