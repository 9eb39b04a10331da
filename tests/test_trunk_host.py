"""trunk.convert on the host: the converted network keeps its parameters, names and state_dict, refuses what the library does not
run, and a converted convolution refuses a CPU tensor before the library is loaded."""
import json
import os

import pytest
import torch
import torch.nn as nn

from tests.helpers import GOLDEN_DIR


def _rr(n_colors):
    from dagl_amd.net import RR
    torch.manual_seed(0)
    return RR(n_colors=n_colors)


@pytest.mark.parametrize("n_colors", [1, 3])
def test_convert_keeps_state_dict_and_parameters(n_colors):
    from dagl_amd import trunk
    m = _rr(n_colors)
    before = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    params = {n: p for n, p in m.named_parameters()}
    assert trunk.convert(m) is m
    after = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert after == before
    if n_colors == 1:
        want = [(k, tuple(s)) for k, s in json.load(open(os.path.join(GOLDEN_DIR, "rr_state_keys.json")))]
        assert after == want
    for n, p in m.named_parameters():
        assert p is params[n], n


@pytest.mark.parametrize("n_colors", [1, 3])
def test_convert_reclasses_trunk_convs_only(n_colors):
    from dagl_amd import trunk
    from dagl_amd.ce import CE
    from dagl_amd.net import _MeanShift
    m = trunk.convert(_rr(n_colors))
    inside_ce = set()
    for mod in m.modules():
        if isinstance(mod, CE):
            inside_ce |= {id(c) for c in mod.modules() if isinstance(c, nn.Conv2d)}
    n_trunk = 0
    for name, mod in m.named_modules():
        if id(mod) in inside_ce:
            assert type(mod) is nn.Conv2d, name
        elif isinstance(mod, _MeanShift):
            assert type(mod) is _MeanShift, name
        elif isinstance(mod, nn.Conv2d):
            assert type(mod) is trunk.Conv2d, name
            n_trunk += 1
    # head + 24 ResBlocks x 2 + the body's last conv + tail + three 1x1 stage mixes
    assert n_trunk == 1 + 48 + 1 + 1 + 3
    assert type(m.add_mean) is _MeanShift
    assert type(m.body[8].c1_c) is trunk.Conv2d and type(m.body[8].c1_1.g) is nn.Conv2d


def test_converted_model_loads_a_checkpoint():
    from dagl_amd import trunk
    from dagl_amd.net import RR, seeded_state_dict
    m = trunk.convert(RR(n_colors=3))
    sd = seeded_state_dict(RR(n_colors=3).state_dict(), 5)
    w = m.head[0].weight
    m.load_state_dict(sd, strict=True)
    assert m.head[0].weight is w
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("kw,what", [
    (dict(kernel_size=3, stride=2, padding=1), "stride"),
    (dict(kernel_size=3, padding=2, dilation=2), "dilation"),
    (dict(kernel_size=3, padding=1, groups=2), "groups"),
    (dict(kernel_size=5, padding=2), "kernel size"),
])
def test_convert_refuses_out_of_scope_convs(kw, what):
    from dagl_amd import DaglError, trunk
    m = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.Sequential(nn.ReLU(), nn.Conv2d(8, 8, **kw)))
    with pytest.raises(DaglError, match=r"1\.1.*" + what):
        trunk.convert(m)
    assert all(type(c) is nn.Conv2d for c in m.modules() if isinstance(c, nn.Conv2d))     # nothing converted


def test_convert_refuses_wide_convs():
    from dagl_amd import DaglError, trunk
    m = nn.Sequential(nn.Conv2d(3, 128, 3, padding=1))
    with pytest.raises(DaglError, match="128 channels"):
        trunk.convert(m)
    with pytest.raises(DaglError, match="padding"):
        trunk.convert(nn.Conv2d(8, 8, 3, padding=0))


def test_converted_conv_refuses_cpu_input_without_loading_the_library(monkeypatch):
    from dagl_amd import DaglError, _lib, trunk

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    conv = trunk.convert(nn.Conv2d(4, 4, 3, padding=1))
    assert type(conv) is trunk.Conv2d
    with pytest.raises(DaglError, match="fp32 GPU"):
        conv(torch.zeros(1, 4, 5, 5))
    from dagl_amd.net import ResBlock
    rb = trunk.convert(ResBlock(8))
    with pytest.raises(DaglError, match="fp32 GPU"):
        rb(torch.zeros(1, 8, 5, 5))


def test_host_side_argument_errors():
    from dagl_amd import _lib
    from dagl_amd.build import build
    build()
    lib = _lib.load()
    assert lib.dagl_trunk_packed_floats(64, 64, 3, 0) == 4 * 9 * 16 * 64
    assert lib.dagl_trunk_packed_floats(3, 64, 3, 1) == 1 * 9 * 16 * 64
    assert lib.dagl_trunk_packed_floats(65, 64, 3, 0) == 0
    assert lib.dagl_trunk_packed_floats(64, 64, 5, 0) == 0
    assert lib.dagl_trunk_conv_forward(None, 1, 64, 64, 8, 8, 3, None, None, None, None, None, 1.0, None, None) == -1
    assert b"null" in lib.dagl_last_error()
    assert lib.dagl_trunk_conv_forward(None, 1, 64, 65, 8, 8, 3, 0x1000, 0x1000, None, None, None, 1.0, None, 0x1000) == -1
    assert lib.dagl_trunk_weight_grad_scratch_bytes(8, 64, 64, 128, 128, 3) > 0
    assert lib.dagl_trunk_conv_weight_grad(None, 8, 64, 64, 128, 128, 3, 0x1000, 0x1000, 1.0, 0x1000, None, None, 0, None,
                                           0x1000, 16) == -1
    assert b"scratch" in lib.dagl_last_error()


def test_edge_case_table_reaches_every_tiling_class():
    """The case table of tests/test_gpu_trunk_edges.py, seen through the library's host-callable functions alone: if the tiling is
    retuned, this says which class the table no longer reaches."""
    from dagl_amd import _lib
    from dagl_amd.build import build
    from tests.test_gpu_trunk_edges import K1_PAIRS, LARGE, PAIRS, SHAPES
    build()
    lib = _lib.load()

    def nc(c):                                   # 4-channel k-steps of the input side, padded to a power of two
        n, r = divmod(lib.dagl_trunk_packed_floats(c, 1, 3, 0), 9 * 64)
        assert r == 0
        return n

    def groups(c):                               # 16-channel groups of the output side, padded to a power of two
        n, r = divmod(lib.dagl_trunk_packed_floats(1, c, 3, 0), 9 * 64)
        assert r == 0
        return n

    def n_pairs(cin, cout):
        return groups(cin) * groups(cout)

    def wgrad_blocks(B, cin, cout, H, W):        # partial sums per pair = blocks of the weight gradient along x
        n, r = divmod(lib.dagl_trunk_weight_grad_scratch_bytes(B, cin, cout, H, W, 3), 4 * (9 * 256 + 16) * n_pairs(cin, cout))
        assert r == 0
        return n

    assert len(PAIRS) == 18 and len(SHAPES) == 17 and len(K1_PAIRS) >= 6 and set(K1_PAIRS) <= set(PAIRS)
    for table in (PAIRS, K1_PAIRS):
        for side in (0, 1):
            assert {nc(p[side]) for p in table} == {1, 2, 4, 8, 16}, (table, side)
        assert {n_pairs(*p) for p in table} == {1, 2, 4, 8, 16}, table
    for side in (0, 1):
        chans = [p[side] for p in PAIRS]
        assert {groups(c) for c in chans} == {1, 2, 4}, side
        assert any(9 <= c <= 12 for c in chans) and any(33 <= c <= 48 for c in chans), side      # padding adds an empty k-step / group
    # (n_pairs, ksplit, grid.y): 8 waves split over min(n_pairs, 8) pairs per block
    assert {(n, 8 // min(n, 8), n // min(n, 8)) for n in (n_pairs(*p) for p in PAIRS)} == \
        {(1, 8, 1), (2, 4, 1), (4, 2, 1), (8, 1, 1), (16, 1, 2)}
    fwd = {s: lib.dagl_trunk_input_grad_blocks(*s) for s in SHAPES}
    assert all(n >= 1 for n in fwd.values())
    assert any(n > s[0] * s[1] for s, n in fwd.items())            # column tiles
    assert any(n < s[0] * s[1] for s, n in fwd.items())            # strips of several rows
    assert any(wgrad_blocks(s[0], 4, 4, s[1], s[2]) > s[0] * s[1] for s in SHAPES)
    assert any(wgrad_blocks(s[0], 4, 4, s[1], s[2]) < s[0] * s[1] for s in SHAPES)
    B, cin, cout, H, W = LARGE
    assert n_pairs(cin, cout) == 1                                  # the three-level k-split tree
    assert lib.dagl_trunk_input_grad_blocks(B, H, W) == B * -(-H // 64) * -(-W // 128) == 324      # the 64-row cap
    assert wgrad_blocks(B, cin, cout, H, W) == B * -(-H // 64) * -(-W // 64)
