"""The split-fp16 projection gradients (gemm16s.hip, ``dagl_fc_grad16`` / ``dagl_fc_grad16_dmap``) over every plan one call can expand
into, against fp64: shifted planes and patch rows with one K slice and with several, both tile kernels of d W, every fold segment,
partial tiles, windows other than CE's two grids, every subset of the outputs (both ways d z is split), degenerate and extreme
gradients.  The shapes are tests/test_fc_grad16_plan_host.py's CASES, whose plans are pinned there by hand and asserted here again, so
no case can silently run another plan.

Every call runs on a scratch filled with 0xFF bytes (NaN halfs: a pad no producer writes shows up in the result) between canaries that
must come back untouched, into outputs pre-filled with NaN that are followed by a sentinel tail.  Bounds are those of
tests/test_gpu_gemm.py: d_w, d_rows, d_map normwise <= 5e-6 of fp64, d_b 1e-6 of the largest absolute column sum.

One run's [parity] figures on the MI355X (d_w / d_rows / rows + fold / d_map where folded / d_b):
  a 1,8,32    3.80e-07 3.47e-07 2.60e-07 2.38e-07 1.58e-08      b 1,5,128   6.34e-07 2.14e-07 2.46e-07 1.76e-07 6.76e-09
  c 1,1,256   4.20e-07 3.68e-07 2.12e-07 2.12e-07 1.23e-08      d 1,12,32   4.78e-07 4.23e-07 3.05e-07 1.88e-07 1.26e-08
  e 2,9,64    5.45e-07 3.67e-07 2.89e-07 2.66e-07 8.35e-09      f 1,3,5     1.82e-07 2.36e-07 2.40e-07    --    4.19e-08
  g 3,7,16    3.30e-07 3.74e-07 3.42e-07 2.55e-07 1.23e-08      h 2,40,36   2.11e-07 3.19e-07 2.59e-07    --    5.04e-09
  i (a, 15x39) 3.80e-07 3.47e-07 2.60e-07 2.38e-07 1.58e-08     j1 2,6,7 s2 2.23e-07 2.75e-07 2.25e-07    --    1.81e-08
  j2 1,4,5 s3 1.96e-07 2.43e-07 2.54e-07    --    2.28e-08      k1 3,2,2 s4 2.49e-07 3.64e-07 2.79e-07    --    2.48e-08
  k2 1,6,8 s4 1.68e-07 2.51e-07 2.56e-07    --    1.46e-08
d y x 2^-66 and x 2^66 at a and h: the figures of scale 1 to every printed digit (the per-call power of two takes the scale out exactly).
Before gemm16s_tile sent one-slice shifted-plane plans to the IMPL kernel, cases a - d ran d_w on the 128 x 128 kernel: d_w NaN at a, b, d
(the poison shows through), 1.42e+00 at c (one image row: the planes fill the buffer, every half is a number, none the right one)."""
import functools
import math

import pytest
import torch

from tests.helpers import normwise
from tests.test_fc_grad16_plan_host import CASE, CASES, SUBSET_CASES, WANT, folds, plan_of

pytestmark = pytest.mark.gpu

BOUND, BOUND_B = 5e-6, 1e-6
POISON, CANARY, GUARD = 0xFF, 0x5A, 4096
SENTINEL, TAIL = 12345.0, 1024


@functools.lru_cache(maxsize=None)
def _data(name):
    """Inputs and fp64 references of a case, computed once and shared (read-only).  The map is random everywhere, border included; case i
    is case a's map with a zero row below and a zero column to the right of it."""
    c = CASE[name]
    src = CASE["a"] if name == "i" else c
    g = torch.Generator().manual_seed(4000 + CASES.index(src))
    B, oh, ow, stride, oy, ox, Hp, Wp = (c[k] for k in ("B", "oh", "ow", "stride", "oy", "ox", "Hp", "Wp"))
    n = B * oh * ow
    pmap = torch.zeros(B, Hp, Wp, 16)
    pmap[:, :src["Hp"], :src["Wp"]] = torch.randn(B, src["Hp"], src["Wp"], 16, generator=g)
    w = (torch.rand(196, 784, generator=g) - 0.5) * 0.07
    dy = torch.randn(n, 196, generator=g) * torch.rand(n, 1, generator=g) ** 4          # heavy-tailed magnitudes
    y = torch.randn(n, 196, generator=g)                                                # the layer's output: ReLU mask
    dz = dy * (y > 0)
    x = pmap.double()
    ys, xs = (oh - 1) * stride + 1, (ow - 1) * stride + 1
    cols = [x[:, oy + kh: oy + kh + ys: stride, ox + kw: ox + kw + xs: stride, :] for kh in range(7) for kw in range(7)]
    rows = torch.stack(cols, dim=3).reshape(n, 784)                                     # [B,oh,ow,49,16]: element order (kh,kw,c)
    return dict(pmap=pmap, w=w, dy=dy, y=y, dz=dz, rows=rows, want_w=dz.double().t() @ rows, want_r=dz.double() @ w.double(),
                want_b=dz.double().sum(0), b_den=float(dz.double().abs().sum(0).max()))


def _fold64(c, rows64):
    """fp64 fold of [n,784] rows onto the case's map: the adjoint of the unfold above."""
    B, oh, ow, stride, oy, ox, Hp, Wp = (c[k] for k in ("B", "oh", "ow", "stride", "oy", "ox", "Hp", "Wp"))
    r = rows64.view(B, oh, ow, 7, 7, 16)
    ys, xs = (oh - 1) * stride + 1, (ow - 1) * stride + 1
    out = torch.zeros(B, Hp, Wp, 16, dtype=torch.float64)
    for kh in range(7):
        for kw in range(7):
            out[:, oy + kh: oy + kh + ys: stride, ox + kw: ox + kw + xs: stride, :] += r[:, :, :, kh, kw, :]
    return out


@functools.lru_cache(maxsize=None)
def _want_map(name):
    return _fold64(CASE[name], _data(name)["want_r"])


def _guarded(shape, dev):
    """An output pre-filled with NaN, followed by a tail that must keep its sentinel."""
    n = math.prod(shape)
    full = torch.full((n + TAIL,), float("nan"), device=dev)
    full[n:] = SENTINEL
    return full, full[:n].view(shape)


def _geo(c):
    return tuple(c[k] for k in ("B", "Hp", "Wp", "stride", "oy", "ox", "oh", "ow"))


def _run(c, pmap, w, dy, y, entry, outs=("w", "b", "x")):
    """One call of ``dagl_fc_grad16`` (entry "rows") or ``dagl_fc_grad16_dmap`` ("dmap") for the outputs named in ``outs`` ("x": d_rows /
    d_map), null pointers for the rest; ``y`` None: ``dy`` is d z itself.  -> {name: CPU tensor}."""
    from dagl_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, Hp, Wp = c["B"], c["Hp"], c["Wp"]
    n = B * c["oh"] * c["ow"]
    name = "dagl_fc_grad16_dmap" if entry == "dmap" else "dagl_fc_grad16"
    need = getattr(lib, name + "_scratch_bytes")(B, c["oh"], c["ow"])
    assert need > 0
    buf = torch.full((256 + need + GUARD,), CANARY, device=dev, dtype=torch.uint8)
    off = (-buf.data_ptr()) % 256
    buf[off:off + need] = POISON
    shapes = {"w": (196, 784), "b": (196,), "x": (B, Hp, Wp, 16) if entry == "dmap" else (n, 784)}
    held = {k: _guarded(shapes[k], dev) for k in outs}
    ptr = lambda k: held[k][1].data_ptr() if k in held else None
    pm, wd, dyd = pmap.to(dev), w.to(dev), dy.to(dev)
    yd = y.to(dev) if y is not None else None
    _lib.check(getattr(lib, name)(ops._stream(), *_geo(c), pm.data_ptr(), wd.data_ptr(), yd.data_ptr() if yd is not None else None,
                                  dyd.data_ptr(), ptr("w"), ptr("b"), ptr("x"), buf.data_ptr() + off, need), name)
    torch.cuda.synchronize()
    assert bool((buf[:off] == CANARY).all()) and bool((buf[off + need:] == CANARY).all()), f"{name}: wrote outside its scratch"
    for k, (full, view) in held.items():
        assert bool((full[view.numel():] == SENTINEL).all()), f"{name}: wrote behind output {k}"
    return {k: view.cpu() for k, (full, view) in held.items()}


def _fold_on_device(c, d_rows):
    from dagl_amd import _lib, ops
    dev = torch.device("cuda:0")
    B, Hp, Wp, stride, oy, ox, oh, ow = _geo(c)
    full, d_map = _guarded((B, Hp, Wp, 16), dev)
    rows = d_rows.to(dev)
    _lib.check(_lib.load().dagl_fold_patches(ops._stream(), B, Hp, Wp, 16, 7, stride, oy, ox, oh, ow, rows.data_ptr(), d_map.data_ptr()),
               "dagl_fold_patches")
    return d_map.cpu()


def _entries(c):
    return ("rows", "dmap") if folds(c) else ("rows",)


def _errors(name, out, entry, scale=1.0):
    """Errors of one call's outputs against the case's fp64 references (the outputs divided by ``scale`` first)."""
    d = _data(name)
    e = {}
    if "w" in out:
        e["d_w"] = normwise(out["w"].double().numpy() / scale, d["want_w"].numpy())
    if "b" in out:
        e["d_b"] = float((out["b"].double() / scale - d["want_b"]).abs().max() / d["b_den"])
    if "x" in out:
        want = _want_map(name) if entry == "dmap" else d["want_r"]
        e["d_map" if entry == "dmap" else "d_rows"] = normwise(out["x"].double().numpy() / scale, want.numpy())
    return e


def _assert_within(errors, out):
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), f"output {k} is not finite everywhere"
    for k, v in errors.items():
        assert v <= (BOUND_B if k == "d_b" else BOUND), (k, v)


def _fmt(errors):
    return ", ".join(f"{k} {v:.2e}" for k, v in errors.items())


def _describe(c):
    return (f"case {c['name']} B={c['B']} {c['oh']}x{c['ow']} stride {c['stride']} at ({c['oy']},{c['ox']}) of "
            f"{c['Hp']}x{c['Wp']}")


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_every_plan_matches_fp64(name):
    """All outputs of both entries (the folding one where the geometry allows it; d_rows + ``dagl_fold_patches`` everywhere) against
    fp64, on the plan the host test pins for the case."""
    from dagl_amd import ops
    c, d = CASE[name], _data(name)
    plan = plan_of(ops, c, True, not folds(c), folds(c))
    if name == "i":                                  # a's patches from a larger map: the very same references
        assert torch.equal(d["want_w"], _data("a")["want_w"]) and torch.equal(d["want_r"], _data("a")["want_r"])
    rows = _run(c, d["pmap"], d["w"], d["dy"], d["y"], "rows")
    e = _errors(name, rows, "rows")
    folded = _fold_on_device(c, rows["x"])
    e["rows + fold"] = normwise(folded.numpy(), _want_map(name).numpy())
    outs = [rows, {"fold": folded}]
    if folds(c):
        dm = _run(c, d["pmap"], d["w"], d["dy"], d["y"], "dmap")
        e["d_map"] = _errors(name, dm, "dmap")["d_map"]
        outs.append(dm)
    route = "shifted planes" if plan["im_rps"] else "patch rows"
    print(f"[parity] fc_grad16 plans {_describe(c)}: {route}, {plan['slices']} x K {plan['k_slice']}, d_w tile {plan['w_tile']}"
          f"{' IMPL' if plan['w_impl'] else ''}, fold_seg {plan['fold_seg']}: {_fmt(e)} (normwise vs fp64, bound {BOUND:g}; d_b {BOUND_B:g})")
    assert plan == WANT[name], plan
    for o in outs:
        _assert_within({}, o)
    _assert_within({k: v for k, v in e.items() if k != "rows + fold"}, {})
    assert e["rows + fold"] <= BOUND
    if folds(c):                                      # d W and d b do not know about the fold
        assert torch.equal(dm["w"], rows["w"]) and torch.equal(dm["b"], rows["b"])


SUBSETS = (("w",), ("x",), ("b",), ("w", "b"), ("x", "b"), ("w", "b", "x"))


@pytest.mark.parametrize("name,entry", [("e", "rows"), ("e", "dmap"), ("h", "rows"), ("g", "dmap")])
def test_output_subsets_are_bit_equal_to_the_full_call(name, entry):
    """d_w only, d_rows / d_map only, d_b only, each with d_b, and all outputs again: every output bit for bit that of the all-outputs
    call -- the split copies ``fcg_split_rows_kernel`` and the merged pass write are the same halfs and the products behind them the
    same launches.  The input-gradient-only call takes the other ReLU route (a pre-masked d z, no y)."""
    assert name in SUBSET_CASES and entry in _entries(CASE[name])
    c, d = CASE[name], _data(name)
    full = _run(c, d["pmap"], d["w"], d["dy"], d["y"], entry)
    e = _errors(name, full, entry)
    print(f"[parity] fc_grad16 subsets {_describe(c)} {entry}: {_fmt(e)} (normwise vs fp64, bound {BOUND:g}; d_b {BOUND_B:g})")
    _assert_within(e, full)
    for sub in SUBSETS:
        premasked = sub == ("x",)
        got = _run(c, d["pmap"], d["w"], d["dz"] if premasked else d["dy"], None if premasked else d["y"], entry, sub)
        assert sorted(got) == sorted(sub)
        for k in sub:
            assert torch.equal(got[k], full[k]), (sub, k)


@pytest.mark.parametrize("name", ["a", "h"])
def test_zero_gradients_give_exact_zeros(name):
    """d y all zero (with y, and as a pre-masked d z), and a dead ReLU (y <= 0 everywhere, zeros among them): every output exactly zero."""
    c, d = CASE[name], _data(name)
    dead = -d["y"].abs()
    dead[::3] = 0.0
    for entry in _entries(c):
        for dy, y in ((torch.zeros_like(d["dy"]), d["y"]), (torch.zeros_like(d["dy"]), None), (d["dy"], dead)):
            out = _run(c, d["pmap"], d["w"], dy, y, entry)
            for k, t in out.items():
                assert int(torch.count_nonzero(t)) == 0 and bool(torch.isfinite(t).all()), (entry, k)


@pytest.mark.parametrize("pos", ["first", "last"])
@pytest.mark.parametrize("name", ["a", "h"])
def test_a_single_non_zero_element(name, pos):
    """dz[r, col] = v alone: d_w row col = v x patch row r, d_rows row r = v W[col] (d_map its fold), d_b = v e_col -- and exact zeros
    everywhere else."""
    c, d = CASE[name], _data(name)
    n = c["B"] * c["oh"] * c["ow"]
    r, col = (0, 0) if pos == "first" else (n - 1, 195)
    v = 0.37
    dz = torch.zeros(n, 196)
    dz[r, col] = v
    v = float(dz[r, col])
    want_row = v * d["w"][col].double()
    rows64 = torch.zeros(n, 784, dtype=torch.float64)
    rows64[r] = want_row
    want_map = _fold64(c, rows64)
    for entry in _entries(c):
        out = _run(c, d["pmap"], d["w"], dz, None, entry)
        for t in out.values():
            assert bool(torch.isfinite(t).all())
        e_w = normwise(out["w"][col].numpy(), (v * d["rows"][r]).numpy())
        others = torch.ones(196, dtype=torch.bool)
        others[col] = False
        assert int(torch.count_nonzero(out["w"][others])) == 0
        want_b = torch.zeros(196)
        want_b[col] = v
        assert torch.equal(out["b"], want_b)
        if entry == "rows":
            e_x = normwise(out["x"][r].numpy(), want_row.numpy())
            others = torch.ones(n, dtype=torch.bool)
            others[r] = False
            assert int(torch.count_nonzero(out["x"][others])) == 0
        else:
            e_x = normwise(out["x"].numpy(), want_map.numpy())
            assert int(torch.count_nonzero(out["x"][want_map == 0])) == 0
        print(f"[parity] fc_grad16 single element {_describe(c)} {entry} dz[{r},{col}]: d_w row {e_w:.2e}, "
              f"{'d_rows row' if entry == 'rows' else 'd_map'} {e_x:.2e} (bound {BOUND:g})")
        assert e_w <= BOUND and e_x <= BOUND


@pytest.mark.parametrize("exp", [-66, 66])
@pytest.mark.parametrize("name", ["a", "h"])
def test_extreme_gradient_scales(name, exp):
    """d y x 2^-66 (1.4e-20) and x 2^66 (7.4e19): with the power of two divided out again, every output meets the bounds of scale 1
    against the same fp64 references -- the per-call scale of the split is what the range claim of gemm16s.hip rests on."""
    c, d = CASE[name], _data(name)
    s = 2.0 ** exp
    dy = d["dy"] * s
    for entry in _entries(c):
        out = _run(c, d["pmap"], d["w"], dy, d["y"], entry)
        e = _errors(name, out, entry, scale=s)
        print(f"[parity] fc_grad16 scale 2^{exp} {_describe(c)} {entry}: {_fmt(e)} (normwise vs fp64 after dividing the scale out, "
              f"bound {BOUND:g}; d_b {BOUND_B:g})")
        _assert_within(e, out)


@pytest.mark.parametrize("name", ["e", "j1"])
def test_patch_linear_backward_for_every_set_of_inputs_that_needs_a_gradient(name):
    """``train_ops.patch_linear`` with requires_grad on the map only, on the weight only and on both (needs_input_grad makes the
    calls without d_w / without an input gradient): the split-fp16 route against the fp32 GEMM route at the 1e-5 of
    test_projection_backward_fast_path_equals_the_fp32_gemm_path; a gradient nobody asked for is None."""
    from dagl_amd import train_ops as T
    dev = torch.device("cuda:0")
    c, d = CASE[name], _data(name)
    pmap = torch.zeros_like(d["pmap"])
    pmap[:, 3:-3, 3:-3] = d["pmap"][:, 3:-3, 3:-3]                    # (the forward kernels expect the zero border)
    G = torch.randn(c["B"], c["oh"] * c["ow"], 196, generator=torch.Generator().manual_seed(3)).to(dev)
    for req in (("map",), ("w",), ("map", "w")):
        res = {}
        for fast in (True, False):
            T.FAST_FC_BACKWARD = fast
            try:
                pm = pmap.to(dev).requires_grad_("map" in req)
                w = d["w"].to(dev).requires_grad_("w" in req)
                b = torch.zeros(196, device=dev)
                y = T.patch_linear(pm, w, b, 7, c["stride"], c["oy"], c["ox"], c["oh"], c["ow"], relu=True)
                (y * G).sum().backward()
                res[fast] = {"map": pm.grad, "w": w.grad, "b": b.grad}
            finally:
                T.FAST_FC_BACKWARD = True
        for k in ("map", "w", "b"):
            if k in req:
                err = normwise(res[True][k].cpu().numpy(), res[False][k].cpu().numpy())
                assert bool(torch.isfinite(res[True][k]).all()) and err <= 1e-5, (req, k, err)
            else:
                assert res[True][k] is None and res[False][k] is None, (req, k)
