"""GPU parity of the whole block through the C ABI: committed golden vectors (produced by the reference
itself), the fp64 oracle as yardstick, and size-independent properties at BASELINE's full sizes."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import golden_cases
from tests.helpers import case_inputs, load_golden, normwise

pytestmark = pytest.mark.gpu

CASES = golden_cases()
# north_star: "within 1e-4 rel fp32", evaluated normwise (max|d|/max|ref|), see tests/test_oracle_golden.py
TOL_OUT = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _module(params, mode="adaptive", k=0, scan="screened"):
    from dagl_amd.ce import CE
    ce = CE(in_channels=params["g.weight"].shape[1])       # (goldens at 32 / 96 / 128 input channels: CE(in_channels=n_feats))
    ce.load_state_dict(params, strict=True)
    ce.select_mode = mode
    ce.scan = scan
    if k:
        ce.select_k = k
    return ce.to(_dev()).eval()


def _run_debug(ce, x, sampled_topk=False):
    """Module prologue + debug forward: out, info with deg / rowsum / agg.  ``sampled_topk``: DAGL_FLAG_SAMPLED_TOPK (keep the
    sampled threshold: the workspace's own policy would re-run an overflowing cold call with the tight one)."""
    from dagl_amd import ops
    with torch.no_grad():
        b1, b2, thr, bias = ce._prologue(x)
        out, info = ops.ce_forward(b1.contiguous(), b2.contiguous(), thr.contiguous(), bias.contiguous(),
                                   ce.fc1[0].weight, ce.fc1[0].bias, ce.fc2[0].weight, ce.fc2[0].bias,
                                   mode=ce.select_mode, k=ce.select_k, debug=True, exact_scan=(ce.scan == "exact"),
                                   sampled_topk=sampled_topk)
    return out, info


@pytest.mark.parametrize("scan", ["screened", "exact"])
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_block_matches_reference_golden(path, scan):
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    ce = _module(params, meta["mode"], meta["k"], scan)
    out, info = _run_debug(ce, x.to(_dev()))
    out = out.cpu().numpy()
    assert out.shape == g["out"].shape
    err = normwise(out, g["out"])
    assert err <= TOL_OUT, f"normwise error {err:.3e}"
    # neighbour sets: identical degrees (a key within rounding of the threshold may flip: allow 1e-4 of them)
    deg = info["deg"].cpu().numpy()
    ndiff = int((deg != g["deg"]).sum())
    assert ndiff <= max(0, int(1e-4 * deg.size)), f"{ndiff} queries differ in degree"
    assert normwise(info["rowsum"].cpu().numpy(), g["rowsum"]) <= TOL_OUT
    B, L = deg.shape
    agg = info["agg"].cpu().view(B, L, 7, 7, 16).permute(0, 1, 4, 2, 3).reshape(B, L, 784)   # -> (c,kh,kw)
    assert normwise(agg[:, ::meta["agg_step"]].numpy(), g["agg_sub"]) <= TOL_OUT
    if meta["mode"] == "adaptive":
        assert info["total_edges"] == int(g["deg"].sum()) or ndiff > 0
        screened = scan == "screened" and meta["H"] * meta["W"] >= 2048
        cap = 256 if screened else 64            # DAGL_LIST_CAP behind the screen, DAGL_FAST_CAP on the fp32 scan
        dense = g["deg"].max() > cap
        # some degree beyond the list width: CSR lists (1); most queries beyond the screen's candidate slots: streamed dense
        # formulation (4)
        if dense:
            # screened: most queries past the lists = streamed dense formulation (4); a few = redone one by one behind the
            # lists (overflow.hip, still path 3).  fp32 scan: two-pass CSR lists (1)
            mostly_dense = screened and (g["deg"] > cap).mean() > 0.5
            assert info["path"] == (4 if mostly_dense else (3 if screened else 1)) or (screened and info["path"] in (1, 3, 4))
        else:
            assert info["path"] == (3 if screened else 0)


@pytest.mark.parametrize("name", ["gray_sparse_64x64", "gray_default_b2_23x30", "topk8_b2_45x38"])
def test_block_vs_fp64_oracle(name):
    """Against a rounding-free evaluation the HIP block is no further away than the reference's own fp32."""
    from oracle.ce_oracle import ce_forward_oracle
    path = [p for p in CASES if name in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    ce = _module(params, meta["mode"], meta["k"])
    with torch.no_grad():
        out = ce(x.to(_dev())).cpu().numpy()
    ref64 = ce_forward_oracle(x, params, mode=meta["mode"], k=meta["k"] or None, dtype=torch.float64).numpy()
    e_hip, e_ref = normwise(out, ref64), normwise(g["out"], ref64)
    assert e_hip <= TOL_OUT
    assert e_hip <= 3 * e_ref + 1e-5, (e_hip, e_ref)


@pytest.mark.parametrize("mode,k,variant", [("topk", 8, "default"), ("topk", 16, "default"), ("adaptive", 0, "sparse"),
                                            ("adaptive_topk", 4, "sparse")])
@pytest.mark.parametrize("H,W", [(96, 80), (128, 128)])
def test_screened_scan_selects_the_same_neighbours_as_the_fp32_scan(mode, k, variant, H, W):
    """bf16 screen + refine vs scanning every score in fp32: identical degrees, outputs equal up to the
    rounding of the kept scores (fp64-accumulated vs fp32 chain)."""
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(51, variant=variant, sparse_gain=2.6).items()}
    x = torch.from_numpy(make_features(51, 2, 64, H, W)).to(_dev())
    outs = {}
    for scan in ("screened", "exact"):
        ce = _module(params, mode, k, scan)
        outs[scan] = _run_debug(ce, x)
    (o_s, i_s), (o_e, i_e) = outs["screened"], outs["exact"]
    assert i_s["path"] == 3 and i_e["path"] in (0, 2)
    assert torch.equal(i_s["deg"], i_e["deg"])
    assert normwise(o_s.cpu().numpy(), o_e.cpu().numpy()) <= 5e-5


def test_screen_overflow_is_redone_by_the_fp32_scan():
    """A nearly constant feature map makes all patches near-duplicates: every score lies inside the screen's
    0.8 % band, every key is a candidate, the candidate slots overflow and the flagged query groups must come
    out of the fp32 scan -- with the same neighbours as scanning everything in fp32 from the start."""
    from dagl_amd.synth import make_ce_params
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(52, variant="default").items()}
    g = torch.Generator().manual_seed(3)
    x = (0.25 + 1e-2 * torch.randn(1, 64, 64, 64, generator=g)).to(_dev())
    # (round 4: a full segment spills into its query's shared area first -- 256 records --, which serves the 1e-2 map above
    # without any redo; a map flatter still puts thousands of keys per query inside the band: beyond segments, spill and the
    # refine pass's 1024 candidates)
    x_flat = (0.25 + 2e-4 * torch.randn(1, 64, 64, 64, generator=g)).to(_dev())
    flat = {}
    for scan in ("screened", "exact"):
        flat[scan] = _run_debug(_module(params, "topk", 8, scan), x_flat, sampled_topk=True)
    assert flat["screened"][1]["path"] == 3 and flat["screened"][1]["redone_queries"] > 0
    assert torch.equal(flat["screened"][1]["deg"], flat["exact"][1]["deg"])
    assert normwise(flat["screened"][0].cpu().numpy(), flat["exact"][0].cpu().numpy()) <= TOL_OUT
    res = {}
    for scan in ("screened", "exact"):
        ce = _module(params, "topk", 8, scan)
        res[scan] = _run_debug(ce, x, sampled_topk=True)
    assert res["screened"][1]["path"] == 3                  # (120 of its 256 queries overflowed a segment before the spill area existed)
    assert torch.equal(res["screened"][1]["deg"], res["exact"][1]["deg"])
    assert normwise(res["screened"][0].cpu().numpy(), res["exact"][0].cpu().numpy()) <= TOL_OUT
    # the workspace's own policy (no flag): this cold call flips to the tight threshold and re-runs in-stream -- eight times the
    # slots hold a 64 x 64 map's candidates, nothing is left for the fp32 pass -- with the same neighbours and numbers
    out_p, info_p = _run_debug(_module(params, "topk", 8, "screened"), x)
    assert info_p["path"] == 3 and info_p["redone_queries"] == 0
    assert torch.equal(info_p["deg"], res["exact"][1]["deg"])
    assert normwise(out_p.cpu().numpy(), res["exact"][0].cpu().numpy()) <= TOL_OUT


@pytest.mark.parametrize("mode,k", [("topk", 8), ("adaptive_topk", 12)])
def test_redo_of_one_image_of_a_batch(mode, k):
    """Batch of three where only the middle image is the near-constant map: its query groups are flagged and redone (scan + merge
    in one launch behind a grid barrier, select.hip topk_redo_kernel), its neighbours' groups are skipped -- same result as the
    fp32 scan of everything."""
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(52, variant="default").items()}
    x = torch.from_numpy(make_features(53, 3, 64, 64, 64))
    g = torch.Generator().manual_seed(3)
    x[1] = 0.25 + 2e-4 * torch.randn(64, 64, 64, generator=g)      # (flat enough for thousands of candidates per query: past the spill area)
    x = x.to(_dev())
    res = {}
    for scan in ("screened", "exact"):
        ce = _module(params, mode, k, scan)
        res[scan] = _run_debug(ce, x, sampled_topk=True)
    L = 16 * 16
    assert res["screened"][1]["path"] == 3 and 0 < res["screened"][1]["redone_queries"] < 3 * L
    assert torch.equal(res["screened"][1]["deg"], res["exact"][1]["deg"])
    assert normwise(res["screened"][0].cpu().numpy(), res["exact"][0].cpu().numpy()) <= TOL_OUT


@pytest.mark.parametrize("B,H,W", [(1, 128, 128), (2, 72, 90)])
def test_dense_formulation_equals_csr_lists(B, H, W):
    """Default-initialised thr/bias heads keep ~95 % of the keys: behind the screen that is the streamed dense formulation
    (dense.hip, path 4), on the exact scan two-pass CSR lists (path 1).  Same degrees, same output up to fp32 rounding --
    also for a width that is not a multiple of the 32-key tiles."""
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(53, variant="default").items()}
    x = torch.from_numpy(make_features(53, B, 64, H, W)).to(_dev())
    res = {}
    for scan in ("screened", "exact"):
        ce = _module(params, "adaptive", 0, scan)
        res[scan] = _run_debug(ce, x)
    (o_d, i_d), (o_c, i_c) = res["screened"], res["exact"]
    assert i_d["path"] == 4 and i_c["path"] == 1
    ndiff = int((i_d["deg"] != i_c["deg"]).sum())
    assert ndiff <= max(1, int(1e-3 * i_c["deg"].numel())), ndiff       # rounding-level ties at the threshold
    assert i_d["total_edges"] == int(i_d["deg"].sum()) and i_d["max_degree"] == int(i_d["deg"].max())
    # the two paths also differ in the projection (split fp16 vs fp32 chains): each is ~1e-4 from the truth in this
    # regime (logits of several hundred amplify the features' last bits), so they may be 2e-4 apart
    assert normwise(i_d["rowsum"].cpu().numpy(), i_c["rowsum"].cpu().numpy()) <= 1e-4
    assert normwise(i_d["agg"].cpu().numpy(), i_c["agg"].cpu().numpy()) <= 2e-4
    assert normwise(o_d.cpu().numpy(), o_c.cpu().numpy()) <= 2e-4
    if H * W <= 8192:                                                    # and both against a rounding-free evaluation
        from oracle.ce_oracle import ce_forward_oracle
        ref64 = ce_forward_oracle(x.cpu(), params, mode="adaptive", dtype=torch.float64).numpy()
        assert normwise(o_d.cpu().numpy(), ref64) <= TOL_OUT
        assert normwise(o_c.cpu().numpy(), ref64) <= TOL_OUT


@pytest.mark.parametrize("H,W", [(192, 192), (256, 256)])
def test_dense_row_maxima_through_the_ring_sampling_kernels(H, W):
    """The dense formulation's top-1 screen takes its threshold from the sampling kernel's ``theta_max`` epilogue.  The cases of
    test_dense_formulation_equals_csr_lists run it in 256-query blocks (barrier form); batch 1 at 192 x 192 (L = 2304) and at
    256 x 256 (L = 4096) are the smallest maps whose plan picks 384- and 512-query blocks (12- and 16-wave ring form).  Same
    comparison with the exact scan's CSR lists as there.  A degree differs where one (query, key) pair's mask value lies within
    rounding of zero, so the allowance of that test -- 1e-3 of the queries at its largest map, 16384 keys -- grows with the keys."""
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(53, variant="default").items()}
    x = torch.from_numpy(make_features(53, 1, 64, H, W)).to(_dev())
    (o_d, i_d), (o_c, i_c) = (_run_debug(_module(params, "adaptive", 0, scan), x) for scan in ("screened", "exact"))
    ndiff = int((i_d["deg"] != i_c["deg"]).sum())
    err = normwise(o_d.cpu().numpy(), o_c.cpu().numpy())
    print(f"[dense-ring] {H}x{W}: paths {i_d['path']} / {i_c['path']}, {ndiff} of {i_c['deg'].numel()} degrees differ, out {err:.2e}")
    assert i_d["path"] == 4 and i_c["path"] == 1
    assert ndiff <= int(1e-3 * i_c["deg"].numel() * (H * W / 16384)), ndiff       # rounding-level ties at the threshold
    assert i_d["total_edges"] == int(i_d["deg"].sum()) and i_d["max_degree"] == int(i_d["deg"].max())
    assert err <= 2e-4, err


def test_dense_hint_skips_the_list_attempt_and_recovers():
    """After a call that ended in the dense formulation the module starts there (no screen / refine / read-back first);
    the result is the same, and sparse inputs switch the hint off again at the next statistics read-back."""
    from dagl_amd.synth import make_ce_params, make_features
    dense_p = {n: torch.from_numpy(a) for n, a in make_ce_params(54, variant="default").items()}
    x = torch.from_numpy(make_features(54, 2, 64, 72, 72)).to(_dev())
    ce = _module(dense_p, "adaptive", 0)
    with torch.no_grad():
        first = ce(x)
        assert ce.last_info["path"] == 4 and ce._dense_hint
        second = ce(x)                                     # hinted, with statistics
        assert ce.last_info["path"] == 4
        third = ce(x)                                      # hinted, no read-back
        assert torch.equal(first, second) and torch.equal(first, third)
        # same module, sparse weights: the hinted dense pass still gives the right answer, then the hint goes away
        sparse_p = {n: torch.from_numpy(a) for n, a in make_ce_params(54, variant="sparse", sparse_gain=2.6).items()}
        ce.load_state_dict(sparse_p, strict=True)
        ce._dense_calls = 0                                # next call fetches statistics
        ref = _module(sparse_p, "adaptive", 0)
        want = ref(x)
        got = ce(x)
        assert ce.last_info["path"] == 4 and not ce._dense_hint
        assert normwise(got.cpu().numpy(), want.cpu().numpy()) <= 5e-5
        again = ce(x)
        assert ce.last_info["path"] == 3
        assert torch.equal(again, want)


def test_dense_hint_on_a_dirty_workspace():
    """DAGL_FLAG_DENSE_HINT on a workspace whose bytes are all 0xFF (NaN in every format): a hinted call gets its split-fp16
    features from the projection's epilogue, pad columns and guard rows included -- nothing may be left to what the buffer held."""
    from dagl_amd import ops
    from dagl_amd.synth import make_ce_params, make_features
    prm = {n: torch.from_numpy(a).to(_dev()).contiguous() for n, a in make_ce_params(54, variant="default").items()}
    prm = {n: t for n, t in prm.items() if not n.startswith("W.")}
    for shape in ((2, 64, 72, 72), (1, 64, 96, 80), (3, 64, 52, 44)):
        x = torch.from_numpy(make_features(54, *shape)).to(_dev())
        want, info = ops.ce_forward_fused(x, prm, mode="adaptive", workspace=ops.Workspace())
        assert info["path"] == 4
        ws = ops.Workspace()
        ops.ce_forward_fused(x, prm, mode="adaptive", workspace=ws)          # sizes the buffer for the dense formulation
        ws.buf.fill_(0xFF)
        got, _ = ops.ce_forward_fused(x, prm, mode="adaptive", workspace=ws, dense_hint=True)
        assert torch.equal(got, want), shape
        again, _ = ops.ce_forward_fused(x, prm, mode="adaptive", workspace=ws, dense_hint=True, weights_packed=True)
        assert torch.equal(again, want), shape


@pytest.mark.parametrize("mode,k,variant", [("adaptive", 0, "sparse"), ("adaptive", 0, "default"), ("topk", 8, "default"),
                                            ("adaptive_topk", 16, "sparse"), ("topk", 300, "default")])
def test_cold_calls_do_not_depend_on_what_the_workspace_held(mode, k, variant):
    """Every byte of the workspace set to 0xFF (NaN in every format) before a cold call (no DAGL_FLAG_WEIGHTS_PACKED): guard rows,
    borders, counters, flags and list slots a call relies on are written by that call."""
    from dagl_amd import ops
    from dagl_amd.synth import make_ce_params, make_features
    prm = {n: torch.from_numpy(a).to(_dev()).contiguous() for n, a in make_ce_params(58, variant=variant, sparse_gain=1.7).items()}
    prm = {n: t for n, t in prm.items() if not n.startswith("W.")}
    for shape in ((2, 64, 72, 72), (1, 64, 50, 46)):
        x = torch.from_numpy(make_features(58, *shape)).to(_dev())
        want, _ = ops.ce_forward_fused(x, prm, mode=mode, k=k, workspace=ops.Workspace())
        ws = ops.Workspace()
        ops.ce_forward_fused(x, prm, mode=mode, k=k, workspace=ws)                 # sizes the buffer (whatever path the call ends on)
        for _ in range(2):
            ws.buf.fill_(0xFF)
            got, _ = ops.ce_forward_fused(x, prm, mode=mode, k=k, workspace=ws)
            assert torch.equal(got, want), (mode, shape)


def test_dense_rows_whose_weights_would_underflow_get_an_exact_shift():
    """Logits in the thousands: the streamed dense formulation shifts by an UPPER bound of the row maximum (bf16 scan, within
    ~1.6 % of it) and its weights go through fp16 -- the slack alone would push every weight of a row below the fp16 denormals
    (6e-3 off at logits of 1 700, rows of zeros at 3 300: tools/dense_large_logits.py on the library before this guard).  The
    first pass records every row's largest logit and flags the blocks of 64 queries whose slack is too large; a gated second pass
    runs them again with the exact maxima as shifts.  Same entry point, same path, no host involvement."""
    from dagl_amd.synth import make_ce_params, make_features
    from oracle.ce_oracle import ce_forward_oracle
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(57, variant="default").items()}
    x = torch.from_numpy(make_features(57, 1, 64, 48, 52))
    for scale in (1.0, 1.2, 1.6, 2.5):
        xs = x * scale
        want, st = ce_forward_oracle(xs, params, mode="adaptive", dtype=torch.float64, stages=True)
        top = float((10.0 * st["S"] * torch.relu(st["S"] - st["T"].unsqueeze(-1))).max())
        ce = _module(params, "adaptive", 0)
        with torch.no_grad():
            out = ce(xs.to(_dev())).cpu()
            again = ce(xs.to(_dev())).cpu()                # (hinted: straight to the dense formulation)
        info = ce.last_info
        err = normwise(out.numpy(), want.float().numpy())
        print(f"[parity] dense, input x {scale}: largest logit {top:.0f}, path {info['path']}, range_fallback {info['range_fallback']}, "
              f"normwise {err:.2e}")
        assert info["path"] == 4 and not info["range_fallback"], info
        assert err <= TOL_OUT and torch.equal(out, again)


def test_adaptive_topk_mode_matches_oracle():
    from oracle.ce_oracle import ce_forward_oracle
    path = [p for p in CASES if "gray_sparse_64x64" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    for k in (4, 16):
        ce = _module(params, "adaptive_topk", k)
        out, info = _run_debug(ce, x.to(_dev()))
        want, st = ce_forward_oracle(x, params, mode="adaptive_topk", k=k, stages=True)
        assert normwise(out.cpu().numpy(), want.numpy()) <= TOL_OUT
        assert np.array_equal(info["deg"].cpu().numpy(), st["deg"].numpy().astype(np.int32))


def test_module_is_deterministic_and_reusable():
    path = [p for p in CASES if "gray_sparse_b2_72x72" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    ce = _module(params)
    xd = x.to(_dev())
    with torch.no_grad():
        a = ce(xd).clone()
        small = ce(xd[:1, :, :20, :24].contiguous())          # different shape through the same workspace
        b = ce(xd)
    assert torch.equal(a, b)                                   # bitwise: sorted lists, fixed summation order
    assert small.shape == (1, 16, 20, 24)
    assert a.is_contiguous() and a.dtype == torch.float32 and a.device == xd.device


def test_input_is_not_mutated_and_stream_is_respected():
    path = [p for p in CASES if "gray_sparse_64x64" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    ce = _module(params)
    xd = x.to(_dev())
    keep = xd.clone()
    s = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        out = ce(xd)
    s.synchronize()
    assert torch.equal(xd, keep)
    assert normwise(out.cpu().numpy(), g["out"]) <= TOL_OUT


# ---- BASELINE.json sizes: properties that need no dense oracle ----------------------------------------

def _full_size_module(seed, variant, gain, mode, k):
    from dagl_amd.synth import make_ce_params
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(seed, variant=variant, sparse_gain=gain).items()}
    return _module(params, mode, k)


@pytest.mark.parametrize("H,W,mode,k", [(256, 256, "topk", 8), (256, 256, "adaptive", 0), (512, 512, "topk", 8)])
def test_full_size_properties(H, W, mode, k):
    """config 2/3 shapes: exact-k degrees, softmax mass in (0,1], linearity in the values, zero for no neighbours,
    agreement between the direct gather and the stand-alone gather over materialised rows."""
    from dagl_amd import ops
    from dagl_amd.synth import make_features
    d = _dev()
    ce = _full_size_module(41, "sparse", 2.4, mode, k)
    x = torch.from_numpy(make_features(41, 1, 64, H, W)).to(d)
    out, info = _run_debug(ce, x)
    L = (H // 4) * (W // 4)
    deg = info["deg"].cpu()
    if mode == "topk":
        assert int(deg.min()) == k and int(deg.max()) == k
    else:
        assert info["total_edges"] == int(deg.sum())
    rs = info["rowsum"].cpu()
    assert float(rs.max()) <= 1.0 + 1e-6 and float(rs.min()) >= 0.0
    assert torch.isfinite(out).all()
    # fold(agg) == out (stage consistency at full size)
    out2 = ops.fold_normalize(info["agg"], H, W)
    assert torch.equal(out, out2)
    # linearity in the values: theta scaled by 2 doubles the output (up to the last bit: the split-fp16 prologue rounds a
    # weight's low part on an absolute grid, so doubling is exact only where that part is a normal fp16 number)
    with torch.no_grad():
        out_x1 = ce(x).clone()
        ce.theta.weight.mul_(2.0); ce.theta.bias.mul_(2.0)
        out_x2 = ce(x)
    assert normwise(out_x2.cpu().numpy(), (out_x1 * 2.0).cpu().numpy()) <= 1e-6
    # fused prologue (module path) vs stock-conv prologue + block entry point: rounding-level differences of b1,
    # except where they flip a near-tie of the selection (top-k is discontinuous): allow 0.1 % of the pixels
    d = (out_x1 - out).abs() / out.abs().max()
    assert float((d > TOL_OUT).float().mean()) <= 1e-3
    # no neighbours -> exact zero
    if mode == "adaptive":
        with torch.no_grad():
            ce.bias_conv.weight.zero_(); ce.bias_conv.bias.fill_(-1e4)
            assert float(ce(x).abs().max()) == 0.0


def test_reduced_precision_io_and_large_window_config():
    """BASELINE configs 3 and 4 run through the same kernels: bf16 feature maps (converted at the boundary) and a
    1024x1024 whole-image search window with adaptive selection capped at k_max = 16."""
    from dagl_amd.synth import make_ce_params, make_features
    d = _dev()
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(61, variant="sparse", sparse_gain=2.6).items()}
    ce = _module(params, "topk", 8)
    x = torch.from_numpy(make_features(61, 1, 64, 128, 128)).to(d)
    with torch.no_grad():
        y32 = ce(x)
        y16 = ce(x.to(torch.bfloat16))
    assert y16.dtype == torch.bfloat16 and y16.shape == y32.shape
    with torch.no_grad():
        ref = ce(x.to(torch.bfloat16).float())
    assert torch.equal(y16, ref.to(torch.bfloat16))          # same math, only I/O rounding
    # config 4: 1024x1024, adaptive AND top-16
    ce4 = _module(params, "adaptive_topk", 16)
    x4 = torch.from_numpy(make_features(62, 1, 64, 1024, 1024)).to(d)
    out4, info4 = _run_debug(ce4, x4)
    assert out4.shape == (1, 16, 1024, 1024) and torch.isfinite(out4).all()
    deg = info4["deg"].cpu()
    assert int(deg.max()) <= 16 and int(deg.min()) >= 0
    assert float(info4["rowsum"].max()) <= 1.0 + 1e-6


def test_concurrent_calls_from_two_threads():
    """nn.DataParallel-style use: two host threads, two streams, two module replicas, at the same time."""
    import threading
    path = [p for p in CASES if "gray_sparse_64x64" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    xd = x.to(_dev())
    mods = [_module(params), _module(params)]
    outs, errs = [None, None], []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.no_grad(), torch.cuda.stream(s):
                for _ in range(5):
                    outs[i] = mods[i](xd)
            s.synchronize()
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert torch.equal(outs[0], outs[1])
    assert normwise(outs[0].cpu().numpy(), g["out"]) <= TOL_OUT


@pytest.mark.parametrize("mode,k,variant,gain", [("topk", 8, "default", 2.0), ("adaptive", 0, "sparse", 2.6)])
def test_fused_stage_equals_four_heads_plus_mix(mode, k, variant, gain):
    """dagl_ces_stage_forward (heads as a batch dimension + 1x1 mix + residual) vs four module calls + torch mix."""
    from dagl_amd import ops
    from dagl_amd.synth import make_ce_params, make_features
    d = _dev()
    B, H, W = 2, 72, 72
    x = torch.from_numpy(make_features(71, B, 64, H, W)).to(d)
    heads = []
    for h in range(4):
        params = {n: torch.from_numpy(a) for n, a in make_ce_params(80 + h, variant=variant, sparse_gain=gain).items()}
        heads.append(_module(params, mode, k))
    g = torch.Generator().manual_seed(9)
    mix_w = (torch.rand(64, 64, 1, 1, generator=g) - 0.5).mul(0.25).to(d)
    mix_b = (torch.rand(64, generator=g) - 0.5).mul(0.1).to(d)
    with torch.no_grad():
        want = torch.nn.functional.conv2d(torch.cat([hd(x) for hd in heads], dim=1), mix_w, mix_b) + x
        prm = [{n: p.detach().contiguous() for n, p in hd.named_parameters() if not n.startswith("W.")} for hd in heads]
        got, info = ops.ces_stage_forward(x, prm, mix_w, mix_b, mode=mode, k=heads[0].select_k)
    assert got is not None and info["path"] == 3
    assert normwise(got.cpu().numpy(), want.cpu().numpy()) <= 2e-5


def test_fused_stage_hands_dense_neighbourhoods_back():
    from dagl_amd import ops
    from dagl_amd.synth import make_ce_params, make_features
    d = _dev()
    x = torch.from_numpy(make_features(72, 1, 64, 48, 48)).to(d)
    heads = [_module({n: torch.from_numpy(a) for n, a in make_ce_params(90 + h, variant="default").items()}) for h in range(4)]
    prm = [{n: p.detach().contiguous() for n, p in hd.named_parameters() if not n.startswith("W.")} for hd in heads]
    out, info = ops.ces_stage_forward(x, prm, torch.zeros(64, 64, 1, 1, device=d), torch.zeros(64, device=d), mode="adaptive")
    assert out is None and info["required_bytes"] == -1


def test_packed_weight_cache_is_invalidated_by_inplace_updates():
    """The module skips repacking fc1/fc2 between calls; an optimizer-style in-place update must be picked up."""
    path = [p for p in CASES if "topk4_64x64" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    xd = x.to(_dev())
    ce = _module(params, "topk", 4)
    with torch.no_grad():
        a1 = ce(xd).clone()
        a2 = ce(xd).clone()                       # second call: cached packed weights
        assert torch.equal(a1, a2)
        ce.fc2[0].weight.mul_(0.5)
        ce.fc1[0].weight.add_(0.01)
        b1 = ce(xd).clone()
    params2 = {n: t.clone() for n, t in params.items()}
    params2["fc2.0.weight"] = params2["fc2.0.weight"] * 0.5
    params2["fc1.0.weight"] = params2["fc1.0.weight"] + 0.01
    fresh = _module(params2, "topk", 4)
    with torch.no_grad():
        b2 = fresh(xd)
    assert not torch.equal(a1, b1)
    assert torch.equal(b1, b2)


def test_packed_conv_weights_follow_inplace_updates():
    """g / theta weights are packed once per weight set as well (the prologue's LDS image): an in-place update must be seen."""
    path = [p for p in CASES if "topk4_64x64" in p][0]
    meta, g = load_golden(path)
    x, params = case_inputs(meta)
    xd = x.to(_dev())
    ce = _module(params, "topk", 4)
    with torch.no_grad():
        a1 = ce(xd).clone()
        assert torch.equal(a1, ce(xd))
        ce.g.weight.mul_(0.75)
        ce.theta.weight.add_(0.02)
        b1 = ce(xd).clone()
    params2 = {n: t.clone() for n, t in params.items()}
    params2["g.weight"] = params2["g.weight"] * 0.75
    params2["theta.weight"] = params2["theta.weight"] + 0.02
    fresh = _module(params2, "topk", 4)
    with torch.no_grad():
        b2 = fresh(xd)
    assert not torch.equal(a1, b1)
    assert torch.equal(b1, b2)


@pytest.mark.parametrize("mode,k", [("topk", 50), ("topk", 64), ("adaptive_topk", 40)])
def test_large_k_on_a_large_batch_of_small_maps_needs_no_redo(mode, k):
    """A batch of 96 maps of 48 x 52 (the tiled driver's leaf tiles are such a batch): a query has few key chunks, and with four
    group maxima per (chunk, half) lane the threshold kernel had fewer values than k to take its k-th largest from -- theta = 0,
    every key a candidate, every query group on the fp32 redo pass (12.4 ms per head on 64 leaf tiles at k = 50, found on round 4's
    last day).  Now: all sixteen group maxima per lane, at least k / 4 chunks.  Same neighbours as the fp32 scan, no redo work."""
    from dagl_amd.synth import make_ce_params, make_features
    params = {n: torch.from_numpy(a) for n, a in make_ce_params(57, variant="default" if mode == "topk" else "allpass").items()}
    x = torch.from_numpy(make_features(58, 96, 64, 48, 52)).to(_dev())          # (2 496 keys: behind the bf16 screen)
    res = {}
    for scan in ("screened", "exact"):
        res[scan] = _run_debug(_module(params, mode, k, scan), x)
    assert res["screened"][1]["path"] == 3 and res["screened"][1]["redone_queries"] == 0
    assert torch.equal(res["screened"][1]["deg"], res["exact"][1]["deg"])
    assert normwise(res["screened"][0].cpu().numpy(), res["exact"][0].cpu().numpy()) <= TOL_OUT
