"""CPU checks of ActiveMLP: the module tree and constructor contract of the reference's active_mlp.py (tests/golden/active_mlp.npz, made by
tests/golden/make_active_golden.py from the reference itself), the packers on CPU tensors, the argument checks of mlpk_atm_sample, which return
before anything touches a device, and the tap function the kernel samples with (csrc/mlpk_atm_tap.h through its host entry mlpk_atm_tap) over
every special offset, so that NaN, +-inf, huge values and the boundaries -1, L - 1, L are proven harmless here before a kernel sees them."""
import ctypes
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, ROOT, load_pkg

FIX = os.path.join(GOLDEN, "active_mlp.npz")
ENULL, EDTYPE, ESHAPE, EALIGN = -4, -1, -2, -3
KERNEL_SHAPES = [(1, 1, 8, 1), (1, 5, 8, 2), (5, 1, 8, 8), (3, 4, 40, 4), (7, 9, 24, 2), (14, 14, 320, 4), (56, 56, 64, 2)]


def mp():
    return load_pkg().models_pytorch


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def table(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


def test_state_dict_tables_match_reference(z, meta):
    am = mp().active_mlp
    for name, make in (("tiny", lambda: am.ActiveMLP(**meta["tiny"])), ("ActiveTiny", am.ActiveTiny), ("ActivexTiny", am.ActivexTiny)):
        want = json.loads(str(z["shapes/" + name]))
        got = table(make())
        assert list(got) == list(want), name
        assert got == want, name
    got = table(am.ActiveMLP(**meta["tiny"]))
    for key in ("blocks.1.2.offset_layer.1.weight", "blocks.0.1.downsample.proj.weight", "pos_blocks.3.proj.bias", "blocks.2.0.atm.atm_w.bias",
                "blocks.0.0.atm.fusion.fc2.weight"):
        assert key in got, key
    assert "blocks.2.2.offset_layer.1.weight" not in got and "blocks.0.0.atm.atm_c.bias" not in got     # j % intv == 0 but j == last; atm_c has no bias
    assert got["blocks.1.0.offset_layer.1.weight"] == [2 * 32 // 4, 32]


def test_fixture_offsets_exercise_the_mixer(meta):
    """what the generator asserted before it wrote the file: the reference's own offsets are neither near-integers nor near zero, and some samples
    leave the map"""
    stats = meta["offset_stats"]
    assert set(stats) == {"tiny/s64", "tiny/s40x52", "tiny/intv6_share1", "real/ActiveTiny"}
    for name, s in stats.items():
        assert s["frac_01_09"] >= 0.25 and s["abs_ge_1"] >= 0.10 and s["outside"] >= 0.01, (name, s)
    assert meta["deform_vec_vs_loop"] <= 1e-12


def sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_exports_and_signatures():
    pkg = load_pkg()
    am = pkg.models_pytorch.active_mlp
    E_ = inspect._empty
    for name in ("ActiveMLP", "ActiveSmall", "ActiveBase", "ActiveLarge"):
        assert name in pkg.models_pytorch.__all__ and getattr(pkg, name) is getattr(pkg.models_pytorch, name) is getattr(am, name), name
    for name in ("Mlp", "ATMOp", "ATMLayer", "ActiveBlock", "Downsample", "PEG", "OverlapPatchEmbed", "ActiveMLP"):
        assert inspect.isclass(getattr(am, name)), name
    for name in ("ActivexTiny", "ActiveTiny", "ActiveSmall", "ActiveBase", "ActiveLarge"):
        assert callable(getattr(am, name)) and sig(getattr(am, name))[0] == ("pretrained", False), name
    assert sig(am.ActiveMLP) == [("img_size", 224), ("patch_size", 4), ("in_chans", 3), ("num_classes", 1000), ("depths", [2, 2, 4, 2]),
                                 ("embed_dims", [64, 128, 320, 512]), ("mlp_ratios", [4, 4, 4, 4]), ("share_dims", [1, 1, 1, 1]), ("drop_path_rate", 0.),
                                 ("act_layer", nn.GELU), ("norm_layer", nn.LayerNorm), ("intv", 2), ("kwargs", E_)]
    assert sig(am.ATMOp) == [("in_chans", E_), ("out_chans", E_), ("stride", 1), ("padding", 0), ("dilation", 1), ("bias", True), ("dimension", '')]
    assert sig(am.ATMLayer) == [("dim", E_), ("proj_drop", 0.)]
    assert sig(am.ActiveBlock) == [("dim", E_), ("mlp_ratio", 4.), ("drop_path", 0.), ("act_layer", nn.GELU), ("norm_layer", nn.LayerNorm), ("share_dim", 1),
                                   ("downsample", None), ("new_offset", False)]
    assert sig(am.Downsample) == [("in_chans", E_), ("out_chans", E_)]
    assert sig(am.PEG) == [("in_chans", E_), ("embed_dim", 768), ("stride", 1)]
    assert sig(am.OverlapPatchEmbed) == [("patch_size", 7), ("stride", 4), ("padding", 2), ("in_chans", 3), ("embed_dim", 64)]
    assert sig(am.Mlp) == [("in_features", E_), ("hidden_features", None), ("out_features", None), ("act_layer", nn.GELU), ("drop", 0.)]
    m = am.ActiveSmall(num_classes=0)
    assert (m.depths, m.intv, m.blocks[1][0].share_dim, m.blocks[1][0].mlp.fc1.out_features) == ([3, 4, 18, 3], 6, 4, 8 * 128)
    assert isinstance(m.head, nn.Identity) and [b.new_offset for b in m.blocks[2]] == [j % 6 == 0 and j != 17 for j in range(18)]
    assert am.ActiveMLP(img_size=96, patch_size=8, in_chans=1, depths=[2, 2], embed_dims=[8, 16], mlp_ratios=[2, 2], share_dims=[1, 2],
                        num_classes=3).patch_embed.proj.weight.shape == (8, 3, 7, 7)      # img_size / patch_size / in_chans are accepted and ignored
    with open(am.__file__) as f:
        assert re.search(r"^\s*(from|import)\s+(einops|timm|torchvision)", f.read(), re.M) is None, am.__file__


def test_init_weights_follow_the_reference():
    am = mp().active_mlp
    torch.manual_seed(0)
    m = am.ActiveMLP(depths=[2, 2], embed_dims=[32, 64], mlp_ratios=[2, 2], share_dims=[2, 4], num_classes=5)
    blk = m.blocks[0][0]
    with torch.no_grad():
        assert float(blk.atm.atm_w.bias.abs().max()) == 0.0 and 0.015 < float(blk.atm.atm_w.weight.std()) < 0.025     # trunc_normal_(std=.02)
        assert float(blk.offset_layer[1].bias.abs().max()) == 0.0 and float(blk.norm1.weight.min()) == 1.0
        w = m.pos_blocks[0].proj.weight                                 # Conv2d: normal(0, sqrt(2 / fan_out)), fan_out = 9 * C / groups = 9
        assert float(m.pos_blocks[0].proj.bias.abs().max()) == 0.0 and 0.3 < float(w.std()) < 0.65


def test_atm_entries_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    for name in ("mlpk_atm_sample", "mlpk_atm_sample_supported", "mlpk_atm_tap"):
        assert name in N.PROTOTYPES and "int %s(" % name in h
    assert "mlpk_atm.hip" in importlib.import_module("jittor-mlp_amd.build").SOURCES
    assert N.lib().mlpk_abi_version() == 14


def test_atm_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20                                             # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    base = dict(dtype=N.BF16, x=P, ldx=64, mean=P, rstd=P, gamma=P, beta=P, off=P, ldoff=64, share=2, out_w=P, out_h=P, out_c=P, ldo=64,
                B=2, H=56, W=56, C=64)

    def call(**kw):
        k = dict(base, **kw)
        return lib.mlpk_atm_sample(k["dtype"], k["x"], k["ldx"], k["mean"], k["rstd"], k["gamma"], k["beta"], k["off"], k["ldoff"], k["share"],
                                   k["out_w"], k["out_h"], k["out_c"], k["ldo"], k["B"], k["H"], k["W"], k["C"], None)

    for kw in ({"x": None}, {"off": None}, {"out_w": None, "out_h": None, "out_c": None}, {"mean": None}, {"rstd": None}):
        assert call(**kw) == ENULL, kw
    assert call(dtype=7) == EDTYPE
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"C": 0}, {"share": 0}, {"share": -2}, {"share": 3}, {"ldx": 56}, {"ldo": 56}, {"ldoff": 63},
               {"share": 1, "ldoff": 64}, {"C": 100, "ldx": 104, "ldo": 104, "ldoff": 104}, {"dtype": N.F32, "C": 6, "ldx": 8, "ldo": 8},
               {"H": 4097}, {"W": 5000}):
        assert call(**kw) == ESHAPE, kw
    for kw in ({"x": P + 2}, {"out_w": P + 8}, {"out_h": P + 4}, {"out_c": P + 2}, {"ldx": 68}, {"ldo": 68}, {"off": P + 1},
               {"dtype": N.F32, "x": P + 8}, {"dtype": N.F32, "ldx": 66}, {"dtype": N.F32, "off": P + 2}):
        assert call(**kw) == EALIGN, kw
    i0, i1, w0, w1 = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
    ref = [ctypes.addressof(v) for v in (i0, i1, w0, w1)]
    assert lib.mlpk_atm_tap(0.0, 0, 4, None, ref[1], ref[2], ref[3]) == ENULL
    for pos, L in ((0, 0), (-1, 4), (4, 4)):
        assert lib.mlpk_atm_tap(0.0, pos, L, *ref) == ESHAPE


def test_atm_supported_table():
    N = load_pkg()._native
    S = N.lib().mlpk_atm_sample_supported
    for dtype in (N.F32, N.F16, N.BF16):
        for H, W, C, share in KERNEL_SHAPES:
            assert S(dtype, H, W, C, share) == 1, (dtype, H, W, C, share)
    assert S(N.F32, 3, 4, 12, 4) == 1 and S(N.BF16, 3, 4, 12, 4) == 0 and S(N.F16, 3, 4, 12, 4) == 0      # C % 4 for fp32, C % 8 for 16-bit
    assert S(9, 7, 7, 64, 2) == 0 and S(N.BF16, 7, 7, 8, 3) == 0 and S(N.BF16, 7, 7, 8, 0) == 0 and S(N.BF16, 0, 7, 8, 1) == 0
    assert S(N.BF16, 7, 7, 8, 16) == 1 and S(N.BF16, 7, 7, 8, 32) == 0                                      # 2C % share
    assert S(N.F32, 4096, 3, 512, 1) == 1 and S(N.F32, 4097, 3, 512, 1) == 0 and S(N.F32, 3, 4097, 512, 1) == 0


# ------------------------------------------------------------------ the packers, on CPU tensors
def test_fusion_rows_and_peg_taps():
    am = mp().active_mlp
    C, hid = 8, 2
    w2 = torch.arange(3 * C, dtype=torch.float32).view(3 * C, 1).expand(3 * C, hid).contiguous()      # row r holds r: reference order r = c * 3 + k
    b2 = -torch.arange(3 * C, dtype=torch.float32)
    w, b = am.fusion_rows(w2, b2, C)
    for k in range(3):
        for c in range(C):
            assert float(w[k * C + c, 0]) == c * 3 + k and float(b[k * C + c]) == -(c * 3 + k)
    conv = nn.Conv2d(C, C, 3, padding=1, groups=C)
    taps = am.peg_taps(conv.weight)
    assert tuple(taps.shape) == (9, C) and taps.dtype == torch.float32
    for t in range(9):
        want = conv.weight.detach()[:, 0, t // 3, t % 3] + (1.0 if t == 4 else 0.0)
        assert torch.equal(taps[t], want), t
    atm = am.ATMLayer(C)
    pk = {}
    am.pack_atm(pk, "q.", atm, torch.bfloat16, torch.device("cpu"))
    assert "q.c.b" not in pk and pk["q.f2.w"].dtype == torch.float32 and pk["q.w.w"].dtype == torch.bfloat16
    assert torch.equal(pk["q.f2.w"][:, :hid], am.fusion_rows(atm.fusion.fc2.weight, atm.fusion.fc2.bias, C)[0])
    assert torch.equal(pk["q.h.w"], atm.atm_h.weight.detach().reshape(C, C).bfloat16())


# ------------------------------------------------------------------ the tap function
def rule(off, pos, L):
    """torchvision's sampling rule along one axis, restated in fp32: (flags, i0, i1, w0, w1), flags bit 0 / 1 = the first / second tap contributes"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        p = f32(f32(pos) + f32(off))
        if not (p > f32(-1.0) and p < f32(L)):
            return 0, 0, 0, f32(0), f32(0)
        fl = np.floor(p)
        f = f32(p - fl)
        i = int(fl)
        ok0, ok1 = 0 <= i <= L - 1, 0 <= i + 1 <= L - 1
        return (1 if ok0 else 0) | (2 if ok1 else 0), i if ok0 else 0, i + 1 if ok1 else 0, f32(f32(1.0) - f), f


def offsets_for(L):
    f32 = np.float32
    grid = np.arange(-(L + 2) * 32, (L + 2) * 32 + 1, dtype=np.float64) / 32.0
    offs = list(grid.astype(f32)) + list((grid[::8] + 0.013).astype(f32)) + [f32(v) for v in range(-L - 3, L + 4)]
    edges = [f32(e - pos) for pos in range(L) for e in (-1, 0, L - 1, L)]
    for e in edges:
        offs += [e, np.nextafter(e, f32(np.inf)), np.nextafter(e, f32(-np.inf))]
    special = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 2.0 ** 24, np.inf, -np.inf, np.nan]
    return offs, [f32(v) for v in special]


@pytest.mark.parametrize("L", [1, 2, 7, 56])
def test_tap_function_over_every_special_offset(L):
    lib = load_pkg()._native.lib()
    i0, i1, w0, w1 = ctypes.c_int(), ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
    ref = [ctypes.addressof(v) for v in (i0, i1, w0, w1)]
    offs, special = offsets_for(L)
    seen = set()
    for pos in range(L):
        for off in offs + special:
            flags = lib.mlpk_atm_tap(float(off), pos, L, *ref)
            want = rule(off, pos, L)
            got = (flags, i0.value, i1.value, np.float32(w0.value), np.float32(w1.value))
            assert flags in (0, 1, 2, 3), (off, pos, L, flags)
            assert got[:3] == want[:3] and got[3] == want[3] and got[4] == want[4], (float(off), pos, L, got, want)
            assert np.isfinite(got[3]) and np.isfinite(got[4]) and 0.0 <= got[3] <= 1.0 and 0.0 <= got[4] <= 1.0
            assert 0 <= got[1] <= L - 1 and 0 <= got[2] <= L - 1                     # never an index that was not range-checked
            p = float(pos) + float(off)                                              # (fp64: exact for these magnitudes or far outside)
            if not np.isfinite(off) or p <= -1.0 - 1e-3 or p >= L + 1e-3:
                assert flags == 0 and got[3] == 0.0 and got[4] == 0.0, (float(off), pos, L, got)
            seen.add(flags)
    assert seen == ({0, 1, 2} if L == 1 else {0, 1, 2, 3})
    # the exact boundaries: p = -1 and p = L are outside, p = L - 1 is the last pixel itself, and an integer position has weight 1 / 0
    assert rule(-1.0, 0, L)[0] == 0 and lib.mlpk_atm_tap(-1.0, 0, L, *ref) == 0
    assert lib.mlpk_atm_tap(float(L), 0, L, *ref) == 0 and lib.mlpk_atm_tap(1.0, L - 1, L, *ref) == 0
    assert lib.mlpk_atm_tap(float(L - 1), 0, L, *ref) == 1 and (i0.value, w0.value, w1.value) == (L - 1, 1.0, 0.0)
    assert lib.mlpk_atm_tap(-0.5, 0, L, *ref) == 2 and (i1.value, w1.value) == (0, 0.5)      # i0 = -1 dropped, i1 = 0 kept


# ------------------------------------------------------------------ what cannot run
def test_stage_without_an_offset_raises_value_error():
    am = mp().active_mlp
    for depths in ([1, 2], [2, 1]):
        m = am.ActiveMLP(depths=depths, embed_dims=[8, 16], mlp_ratios=[2, 2], share_dims=[1, 2], num_classes=3).eval()
        with pytest.raises(ValueError, match="offset"):
            m(torch.zeros(1, 3, 32, 32))


def test_containers_and_cpu_inputs_raise(meta):
    am = mp().active_mlp
    m = am.ActiveMLP(**meta["tiny"]).eval()
    x = torch.zeros(1, 16, 16, 16)
    for mod, arg in ((m.blocks[0][0], x), (m.pos_blocks[0], x), (m.blocks[0][1].downsample, x), (m.patch_embed, torch.zeros(1, 3, 64, 64)),
                     (m.blocks[0][0].mlp, x), (am.Mlp(8), torch.zeros(2, 8))):
        with pytest.raises(NotImplementedError, match="ActiveMLP"):
            mod(arg)
    with pytest.raises(NotImplementedError, match="ActiveMLP"):
        m.blocks[0][0].atm.atm_w(x.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2))
    with pytest.raises(NotImplementedError):                    # no CPU implementation, as for every family
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        m.blocks[0][0].atm(x, torch.zeros(1, 32, 16, 16))
