"""The wide top-k inference path (topk_wide.hip: min(k, N) > 64) on CRAFTED score rows, with a read-out of which form served a row.

The fc weights make the score row a channel of b1: fc2 takes feature 0 from channel 0 at the centre tap, fc1 is its bias e_0, so
S[i, j] = b1[0, pixel j] for every query i.  Scores sit on a coarse binary grid (multiples of 2^-12 below 4, or of 4 up to 3000), which the
split-fp16 projection, the split-fp16 score product (N >= 2048) and the fp32 one (N < 2048, exact_scan) all carry exactly: a tie is a tie
on every route, the selected set is unambiguous, and degree and set must match the fp64 oracle exactly.  Rows are built to break what
wide_list_kernel's sample assumes -- the k best keys inside one wave's eighth of the row, flat rows, high keys on sampled positions only,
ties across the waves' segments -- and ops.ce_wide_debug tells which rows the list kernel served and which it declined to the
three-kernel form (wide_select / wide_attend / wide_combine); every case asserts the form it was built for.  B = 1 wherever the path
is asserted.  Every call runs on a workspace poisoned with a large positive finite float.

Reference: oracle.ce_oracle in fp64 from the same b1 and weights (patch_rows + linear + relu, then _graph_core on one row per distinct
(thr, bias) pair: all queries share Wq = e_0), folded as ce_core_oracle folds.

Tolerance, per tensor, normwise (tests.helpers.normwise): e_lib = library vs fp64, e_ref32 = the same oracle run in fp32 vs fp64;
e_lib <= min(3 e_ref32 + FLOOR, 1e-4).  FLOOR = 1e-6: over these cases and tensors the fp32 oracle's own e_ref32 spreads from 3e-9
(b_band k = 600, rowsum) to 6e-6 (h_band, rowsum), four fifths of the figures below 1e-6 -- a case at the low end of that spread is
granted what one in its upper part costs.  One wrong key at the k-th place (the (k+1)-th best in its stead) moves the fp64 agg by
5e-6 (cases e, f: ties at e^-10 of the top weight) to 0.17 -- score ranges are kept narrow for that --, except in case i, whose
top five keys carry all the mass.  One run's ratios: DESIGN.md section 5."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import normwise

DEV = "cuda:0"
CAP = 1e-4
FLOOR = 1e-6
POISON = 1.0e30


# ---- score rows (fp32 on the CPU, [N]) ---------------------------------------------------------------------------------------------

def _grid(g, n, levels, step):
    return torch.randint(0, levels, (n,), generator=g).float() * step


def row_iid(g, H, W):
    """i.i.d. multiples of 2^-12 in [0, 2)"""
    return _grid(g, H * W, 8192, 2.0 ** -12)


def row_distinct(g, H, W):
    """distinct multiples of 2^-12 in [0, 2) (N <= 8192): any number of keys can be made to pass a threshold"""
    return torch.randperm(8192, generator=g)[:H * W].float() * 2.0 ** -12


def wave_share(N):
    """keys of one wave's share in wide_list_kernel phase B: an eighth of the row, rounded up to 256"""
    return (-(-N // 8) + 255) // 256 * 256


def row_band(g, H, W):
    """the 700 best keys (distinct values in [2, 2.25)) all inside wave 0's share of the row, the rest below 1"""
    N = H * W
    s = _grid(g, N, 4096, 2.0 ** -12)
    at = torch.randperm(wave_share(N), generator=g)[:700]
    s[at] = 2.0 + torch.randperm(1024, generator=g)[:700].float() * 2.0 ** -12
    return s


def row_const(g, H, W):
    return torch.full((H * W,), 0.75)


def sampled_positions(N):
    """The keys wide_list_kernel phase A samples (topk_wide.hip): whole 32-key lines, one of every `stride` lines, line
    g * stride + (5 g mod stride) of group g, the last line when that is past the row."""
    n_lines = (N + 31) // 32
    stride = (n_lines * 32 + 4095) // 4096
    n_groups = (n_lines + stride - 1) // stride
    pos = []
    for grp in range(n_groups):
        line = min(grp * stride + ((5 * grp) % stride if stride > 1 else 0), n_lines - 1)
        pos += [j for j in range(line * 32, line * 32 + 32) if j < N]
    return torch.tensor(sorted(set(pos))), stride


def row_sample_only(g, H, W):
    """150 high keys (distinct values in [1, 1.25)), every one on a sampled position; the rest below 1: the sample promises more keys
    above its bound than the row holds.  (The 50 low keys a k = 200 takes lie just under 1: their weights are visible in agg.)"""
    N = H * W
    s = _grid(g, N, 4096, 2.0 ** -12)
    pos, stride = sampled_positions(N)
    assert stride > 1
    at = pos[torch.randperm(len(pos), generator=g)[:150]]
    s[at] = 1.0 + torch.randperm(1024, generator=g)[:150].float() * 2.0 ** -12
    return s


def _row_ties(g, H, W, n_ties):
    """100 keys just above 2, `n_ties` keys exactly 1.0, scattered by a permutation; the rest <= 0.25"""
    N = H * W
    s = _grid(g, N, 1025, 2.0 ** -12)
    perm = torch.randperm(N, generator=g)
    s[perm[:100]] = 2.0 + _grid(g, 100, 128, 2.0 ** -12)
    s[perm[100:100 + n_ties]] = 1.0
    return s


def row_ties_1000(g, H, W):
    return _row_ties(g, H, W, 1000)


def row_ties_4900(g, H, W):
    return _row_ties(g, H, W, 4900)


def row_coarse(g, H, W):
    """i.i.d. multiples of 2^-8 in [0, 1): 256 levels, a tie at the k-th place is near certain"""
    return _grid(g, H * W, 256, 2.0 ** -8)


def row_sparse(g, H, W):
    """150 positive keys (distinct values in [1, 1.25)), every other score exactly 0: the k-th best of a k = 200 is a zero, the bound of
    the list kernel's sample is the smallest key there is and every key of the row a candidate"""
    N = H * W
    s = torch.zeros(N)
    s[torch.randperm(N, generator=g)[:150]] = 1.0 + torch.randperm(1024, generator=g)[:150].float() * 2.0 ** -12
    return s


def row_huge(g, H, W):
    """multiples of 4 up to 3000 (logits 3e4 > WL_RESCORE_LOGIT), five keys tied at the top"""
    N = H * W
    s = _grid(g, N, 700, 4.0)
    s[torch.randperm(N, generator=g)[:5]] = 3000.0
    return s


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# name -> rows (one per image), shape, mode, k, exact_scan, and the form expected of the LAST image's rows: "list" (served by
# wide_list_kernel), "three" (declined), "none" (k > 1024: no list launch, ce_wide_debug refuses), or a tuple over the kinds of
# threshold rows of the intersection mode (KINDS).  tie: the k-th place falls inside a group of equal scores (asserted on the reference).
KINDS = ("none_pass", "fewer", "exactly_k", "all_pass", "more")


def _case(rows, shape, k, form, mode="topk", exact=False, tie=False):
    return dict(rows=rows if isinstance(rows, tuple) else (rows,), shape=shape, k=k, form=form, mode=mode, exact=exact, tie=tie)


CASES = {
    # a: honest rows -- served by the list; fp32 scores (N < 2048), the whole row as the sample (stride 1), strides 2 and 3
    "a_iid_40x44_k65": _case(row_iid, (40, 44), 65, "list"),
    "a_iid_50x60_k200": _case(row_iid, (50, 60), 200, "list"),
    "a_iid_71x73_k65": _case(row_iid, (71, 73), 65, "list"),
    "a_iid_71x73_k200": _case(row_iid, (71, 73), 200, "list"),
    "a_iid_71x73_k200_exact": _case(row_iid, (71, 73), 200, "list", exact=True),
    "a_iid_71x73_k1024": _case(row_iid, (71, 73), 1024, "list"),
    "a_iid_96x96_k200": _case(row_iid, (96, 96), 200, "list"),
    # b: the best keys in one wave's share -- more candidates than its segment holds
    "b_band_71x73_k600": _case(row_band, (71, 73), 600, "three"),
    "b_band_71x73_k600_exact": _case(row_band, (71, 73), 600, "three", exact=True),
    "b_band_71x73_k100": _case(row_band, (71, 73), 100, "list"),
    # c: flat rows -- every key a candidate; at 50 x 60 a wave's share IS a full segment (512 keys) and the list serves the row
    "c_const_50x60_k65": _case(row_const, (50, 60), 65, "list", tie=True),
    "c_const_71x73_k65": _case(row_const, (71, 73), 65, "three", tie=True),
    "c_const_71x73_k700": _case(row_const, (71, 73), 700, "three", tie=True),
    # d: the sample's bound is too high -- fewer than k candidates
    "d_sample_only_96x96_k200": _case(row_sample_only, (96, 96), 200, "three"),
    "d_sample_only_96x96_k200_exact": _case(row_sample_only, (96, 96), 200, "three", exact=True),
    # e / f: a tie at the k-th place across the list's eight segments / across the fallback's (chunk, wave) ranges
    "e_ties1000_96x96_k300": _case(row_ties_1000, (96, 96), 300, "list", tie=True),
    "f_ties4900_96x96_k300": _case(row_ties_4900, (96, 96), 300, "three", tie=True),
    # g: k > 1024 -- the three-kernel form for every row, a real selection with a tie
    "g_coarse_40x44_k1025": _case(row_coarse, (40, 44), 1025, "none", tie=True),
    "g_coarse_71x73_k3000": _case(row_coarse, (71, 73), 3000, "none", tie=True),
    "g_coarse_96x96_k1025": _case(row_coarse, (96, 96), 1025, "none", tie=True),
    # h: the intersection mode, per-row pass sets over one score row (KINDS by query index mod 5)
    "h_distinct_71x73_k200": _case(row_distinct, (71, 73), 200, ("list", "list", "list", "list", "list"), mode="adaptive_topk"),
    "h_band_71x73_k600": _case(row_band, (71, 73), 600, ("list", "three", "three", "three", "three"), mode="adaptive_topk"),
    # i: logits of 3e4 -- the selected keys re-scored from the fp32 feature rows
    "i_huge_50x60_k100": _case(row_huge, (50, 60), 100, "list"),
    # k: a row of zeros under 150 keys at N = 3000 (a multiple of 4, not of 32): the lanes past the row's end in phase B must stay out
    "k_sparse_50x60_k200": _case(row_sparse, (50, 60), 200, "list", tie=True),
    # j: two images (batch indexing); the path of the last one
    "j_iid_band_b2_71x73_k600": _case((row_iid, row_band), (71, 73), 600, "three"),
}


def _seed(name):
    return zlib.crc32(name.encode())


def _gap_at(v, p):
    """smallest p' >= p with v[p' - 1] > v[p'] (v sorted descending): a threshold between them passes exactly p' keys"""
    while v[p - 1] == v[p]:
        p += 1
    return p


def thresholds(s, k, L):
    """Per-query (thr, bias) of the intersection mode over the score row s: thr = 0, so m = S + bias, and bias = -tau with tau midway
    between two grid values (exact in fp32) -- no key, fewer than k, exactly k, every key, more than k keys pass."""
    v = s.sort(descending=True).values
    half = 2.0 ** -13
    p_fewer, p_more = _gap_at(v, k - 50), _gap_at(v, k + k // 2)
    assert v[k - 1] > v[k] and p_fewer < k, "the row cannot pass exactly k / fewer than k keys"
    tau = dict(none_pass=float(v[0]) + half, fewer=float(v[p_fewer]) + half, exactly_k=float(v[k]) + half, all_pass=-0.5,
               more=float(v[p_more]) + half)
    passing = dict(none_pass=0, fewer=p_fewer, exactly_k=k, all_pass=len(s), more=p_more)
    kind = torch.arange(L) % len(KINDS)
    bias = torch.tensor([-tau[KINDS[i]] for i in kind.tolist()], dtype=torch.float32)
    return torch.zeros(L), bias, kind, passing


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """b1, b2 [B,16,H,W], thr / bias [B,L] or None, the fc weights, the intended score rows [B,N] and the rows' kinds [L]."""
    c = CASES[name]
    H, W = c["shape"]
    B, N, L = len(c["rows"]), H * W, -(-H // 4) * -(-W // 4)
    g = torch.Generator().manual_seed(_seed(name))
    s = torch.stack([row(g, H, W) for row in c["rows"]])
    b1 = (torch.randint(-512, 513, (B, 16, H, W), generator=g).float() / 256.0)      # the other channels: grid noise the weights ignore
    b1[:, 0] = s.reshape(B, H, W)
    b2 = torch.randn(B, 16, H, W, generator=g)
    fc1_w, fc1_b = torch.zeros(196, 784), torch.zeros(196)
    fc2_w, fc2_b = torch.zeros(196, 784), torch.zeros(196)
    fc1_b[0] = 1.0
    fc2_w[0, 0 * 49 + 3 * 7 + 3] = 1.0                   # element order (c, kh, kw): channel 0, centre tap
    thr = bias = kind = None
    if c["mode"] == "adaptive_topk":
        assert B == 1
        thr, bias, kind, _ = thresholds(s[0], c["k"], L)
        thr, bias = thr[None], bias[None]
    return dict(b1=b1, b2=b2, thr=thr, bias=bias, w=(fc1_w, fc1_b, fc2_w, fc2_b), s=s, kind=kind, B=B, H=H, W=W, N=N, L=L)


def _reference(name, dtype):
    """The oracle on one query row per distinct (thr, bias) pair, expanded to all L rows and folded: deg [B,L], rowsum [B,L],
    agg [B,L,784] in (c,kh,kw) order, out [B,16,H,W]."""
    from oracle.ce_oracle import KSIZE, STRIDE_KV, STRIDE_Q, _graph_core, overlap_count, patch_rows, same_pad
    c, x = CASES[name], case_inputs(name)
    H, W, L, N = x["H"], x["W"], x["L"], x["N"]
    fc1_w, fc1_b, fc2_w, fc2_b = (t.to(dtype) for t in x["w"])
    b1, b2 = x["b1"].to(dtype), x["b2"].to(dtype)
    q_rows, k_rows, v_rows = patch_rows(b1, KSIZE, STRIDE_Q), patch_rows(b1, KSIZE, STRIDE_KV), patch_rows(b2, KSIZE, STRIDE_KV)
    fold_pad = same_pad(b2[:1, :1], KSIZE, STRIDE_KV)[1][0]
    cnt = overlap_count(H, W, dtype, pad=fold_pad)
    if x["kind"] is None:
        rows, inverse = torch.zeros(1, dtype=torch.long), torch.zeros(L, dtype=torch.long)
    else:
        rows, inverse = torch.arange(len(KINDS)), x["kind"]
    res = dict(deg=[], rowsum=[], agg=[], out=[])
    for n in range(x["B"]):
        Wq = F.relu(F.linear(q_rows[n], fc1_w, fc1_b))
        X = F.relu(F.linear(k_rows[n], fc2_w, fc2_b))
        assert torch.equal(Wq, Wq[:1].expand_as(Wq))                    # every query is the same feature row
        zero = torch.zeros(len(rows), dtype=dtype)
        thr_n = x["thr"][n][rows].to(dtype) if x["thr"] is not None else zero
        bias_n = x["bias"][n][rows].to(dtype) if x["bias"] is not None else zero
        _, st = _graph_core(Wq[rows], X, thr_n, bias_n, v_rows[n], c["mode"], c["k"], H, W, None)
        # the harness itself: the reference's score row IS the intended map (a wrong weight column would show here, not in the kernel)
        assert torch.equal(st["S"], x["s"][n].to(dtype)[None].expand(len(rows), N)), name
        if c["tie"] and dtype == torch.float64:
            v = x["s"][n].sort(descending=True).values
            kk = min(c["k"], N)
            assert kk < N and v[kk - 1] == v[kk], f"{name}: no tie at the k-th place"
        agg = st["agg"][inverse]
        res["deg"].append(st["deg"][inverse]); res["rowsum"].append(st["rowsum"][inverse]); res["agg"].append(agg)
        res["out"].append(F.fold(agg.t().unsqueeze(0), (H, W), (KSIZE, KSIZE), padding=fold_pad, stride=STRIDE_Q) / cnt)
    return {k_: (torch.cat(v) if k_ == "out" else torch.stack(v)) for k_, v in res.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 reference of a case and e_ref32 per tensor (the same oracle in fp32 against it); computed once, never modified."""
    with torch.no_grad():
        r64, r32 = _reference(name, torch.float64), _reference(name, torch.float32)
    assert torch.equal(r32["deg"].long(), r64["deg"].long()), name     # exact scores: both precisions select the same keys
    e32 = {t: normwise(r32[t].numpy(), r64[t].numpy()) for t in ("rowsum", "agg", "out")}
    return r64, e32


def _agg_ckk(agg):                       # [.., 784] (kh,kw,c) -> (c,kh,kw), the reference's row order
    s = agg.shape[:-1]
    return agg.reshape(*s, 7, 7, 16).movedim(-1, -3).reshape(*s, 784)


def run(name):
    """One library call of a case on a poisoned workspace -> (out, info with deg / rowsum / agg, served words or None)."""
    from dagl_amd import _lib, ops
    c, x = CASES[name], case_inputs(name)
    dev = torch.device(DEV)
    flags = _lib.MODES[c["mode"]] | (_lib.FLAG_EXACT_SCAN if c["exact"] else 0)
    nbytes = _lib.load().dagl_ce_workspace_bytes(x["B"], x["H"], x["W"], flags, c["k"])
    assert nbytes > 0
    ws = ops.Workspace()
    buf = ws.get(nbytes, dev)
    buf[:buf.numel() // 4 * 4].view(torch.float32).fill_(POISON)
    d = lambda t: None if t is None else t.to(dev).contiguous()
    out, info = ops.ce_forward(d(x["b1"]), d(x["b2"]), d(x["thr"]), d(x["bias"]), *(d(t) for t in x["w"]), mode=c["mode"], k=c["k"],
                               workspace=ws, debug=True, exact_scan=c["exact"])
    assert ws.peek(dev) is buf                                          # the call ran on the poisoned buffer
    assert info["path"] == 6 and info["range_fallback"] == 0, {k_: v for k_, v in info.items() if not torch.is_tensor(v)}
    if c["form"] == "none":
        with pytest.raises(_lib.DaglError) as err:
            ops.ce_wide_debug((x["B"], 16, x["H"], x["W"]), c["mode"], c["k"], ws, dev, exact_scan=c["exact"])
        assert err.value.code == _lib.ERR_UNSUPPORTED
        served = None
    else:
        served = ops.ce_wide_debug((x["B"], 16, x["H"], x["W"]), c["mode"], c["k"], ws, dev, exact_scan=c["exact"]).cpu()
    torch.cuda.synchronize()
    return out.cpu(), {k_: (v.cpu() if torch.is_tensor(v) else v) for k_, v in info.items()}, served


def check_form(name, served):
    c, x = CASES[name], case_inputs(name)
    if c["form"] == "none":
        assert served is None
        return
    assert served.shape == (x["L"],) and bool(((served == 0) | (served == 1)).all()), (name, served)
    if isinstance(c["form"], tuple):
        want = torch.tensor([1 if c["form"][i] == "list" else 0 for i in x["kind"].tolist()], dtype=served.dtype)
    else:
        want = torch.full((x["L"],), 1 if c["form"] == "list" else 0, dtype=served.dtype)
    assert torch.equal(served, want), f"{name}: rows served by the list kernel {served.tolist()}, expected {want.tolist()}"


def check_values(name, out, info):
    c, x = CASES[name], case_inputs(name)
    ref, e32 = reference(name)
    assert torch.equal(info["deg"].long(), ref["deg"].long()), (name, info["deg"], ref["deg"])
    assert info["total_edges"] == int(ref["deg"].sum()) and info["max_degree"] == int(ref["deg"].max()), name
    got = dict(rowsum=info["rowsum"], agg=_agg_ckk(info["agg"]), out=out)
    ratios = {}
    for t in ("rowsum", "agg", "out"):
        assert e32[t] <= CAP, (name, t, e32[t])            # (a reference that loses its own digits would loosen the bound)
        e = normwise(got[t].numpy(), ref[t].numpy())
        ratios[t] = e / max(e32[t], 1e-30)
        print(f"[wide_rows] {name} {t}: e_lib={e:.3e} e_ref32={e32[t]:.3e} ratio={ratios[t]:.2f}")
        assert e <= min(3.0 * e32[t] + FLOOR, CAP), (name, t, e, e32[t])
    if c["mode"] == "topk":
        # all L rows of an image are the same computation
        for n in range(x["B"]):
            assert torch.equal(info["agg"][n], info["agg"][n, :1].expand_as(info["agg"][n])), name
            assert torch.equal(info["rowsum"][n], info["rowsum"][n, :1].expand_as(info["rowsum"][n])), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_row_takes_its_form_and_matches_the_oracle(name):
    out, info, served = run(name)
    check_form(name, served)
    check_values(name, out, info)


def test_threshold_rows_cover_the_four_kinds():
    """The intersection-mode cases hold rows with no passing key, fewer than k, exactly k, more than k and every key, and the reference's
    degrees are what the thresholds were built for -- min(passing, k)."""
    for name in ("h_distinct_71x73_k200", "h_band_71x73_k600"):
        c, x = CASES[name], case_inputs(name)
        _, _, kind, passing = thresholds(x["s"][0], c["k"], x["L"])
        ref, _ = reference(name)
        want = torch.tensor([min(passing[KINDS[i]], c["k"]) for i in kind.tolist()])
        assert torch.equal(ref["deg"][0].long(), want)
        assert sorted(set(want.tolist()))[0] == 0 and 0 < passing["fewer"] < c["k"] < passing["more"] < x["N"]


def test_tie_rule_takes_the_lowest_key_indices():
    """Cases c, e, f, i state their expected neighbour set in closed form: the reference agrees with it before the library is asked."""
    from oracle.ce_oracle import _k_best
    for name, n_above, tie_value in (("c_const_71x73_k700", 0, 0.75), ("e_ties1000_96x96_k300", 100, 1.0),
                                     ("f_ties4900_96x96_k300", 100, 1.0)):
        s, k = case_inputs(name)["s"][0], CASES[name]["k"]
        sel = _k_best(s[None].double(), k)[0].sort().values
        above = (s > tie_value).nonzero().flatten()
        ties = (s == tie_value).nonzero().flatten()
        assert len(above) == n_above and len(ties) > k - n_above
        assert torch.equal(sel, torch.cat([above, ties[:k - n_above]]).sort().values)
    # case e: the ties lie in all eight wave shares of the list kernel, the 200 taken ones in more than one
    x = case_inputs("e_ties1000_96x96_k300")
    ties = (x["s"][0] == 1.0).nonzero().flatten()
    assert len(set((ties // wave_share(x["N"])).tolist())) == 8 and int(ties[199]) // wave_share(x["N"]) >= 1


@pytest.mark.gpu
def test_huge_logits_give_the_mean_of_the_top_five():
    """Case i in closed form: five keys tied at 3000 carry all the softmax mass -- agg is the mean of their value patches, rowsum 1."""
    from oracle.ce_oracle import KSIZE, STRIDE_KV, patch_rows
    name = "i_huge_50x60_k100"
    x = case_inputs(name)
    out, info, served = run(name)
    check_form(name, served)
    top = (x["s"][0] == 3000.0).nonzero().flatten()
    assert len(top) == 5
    mean = patch_rows(x["b2"].double(), KSIZE, STRIDE_KV)[0][top].mean(dim=0)
    assert normwise(_agg_ckk(info["agg"])[0, 0].numpy(), mean.numpy()) <= 3e-7          # five fp32 products and one rounding of 1 / Z
    assert float((info["rowsum"] - 1.0).abs().max()) <= 2e-7
    assert int(info["deg"].min()) == 100 and int(info["deg"].max()) == 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["b_band_71x73_k600", "e_ties1000_96x96_k300", "h_band_71x73_k600", "g_coarse_71x73_k3000"])
def test_two_calls_return_the_same_bits(name):
    out0, info0, served0 = run(name)
    out1, info1, served1 = run(name)
    assert torch.equal(info0["agg"], info1["agg"]) and torch.equal(info0["deg"], info1["deg"])
    assert torch.equal(info0["rowsum"], info1["rowsum"]) and torch.equal(out0, out1)
    assert served0 is None and served1 is None or torch.equal(served0, served1)
