"""CPU checks of ConvMLP: the module tree and constructor contract of the reference's conv_mlp.py (tests/golden/convmlp.npz, made by
tests/golden/make_convmlp_golden.py from the reference itself), the packers on CPU tensors against torch in fp64, the fp64 restatement of
mlpk_ln_dwconv3_nhwc (tests/convmlp_model.py) against torch's own layer_norm + conv2d, the power of the kernel gate against planted faults on the
GPU test's own operands, and the `_supported` tables and argument checks of the three entries, which return before anything touches a device."""
import importlib
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_pkg
import convmlp_model as CM
from convmlp_model import DTYPES, IDS, LN_SHAPES
from test_gpu_ops import EPS

FIX = os.path.join(GOLDEN, "convmlp.npz")
MP = load_pkg().models_pytorch.conv_mlp
ENULL, EDTYPE, ESHAPE, EALIGN = -4, -1, -2, -3
CLASSES = ["ConvMLP", "ConvTokenizer", "ConvStage", "Mlp", "ConvMLPStage", "ConvDownsample", "BasicStage", "DropPath"]
FUNCTIONS = ["drop_path", "convmlp_s", "convmlp_m", "convmlp_l"]


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def table(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


# ------------------------------------------------------------------ the drop-in contract
def test_exports_and_signatures(z):
    pkg = load_pkg()
    impl = importlib.import_module(pkg.__name__ + ".convmlp_impl")
    for name in ("ConvMLP", "convmlp_s", "convmlp_m", "convmlp_l"):
        assert name in pkg.models_pytorch.__all__ and name in MP.__all__
        assert getattr(pkg, name) is getattr(pkg.models_pytorch, name) is getattr(MP, name) is getattr(impl, name), name
    want = json.loads(str(z["signatures"]))
    assert sorted(want) == sorted(CLASSES + FUNCTIONS)
    for name in CLASSES + FUNCTIONS:
        obj = getattr(MP, name)
        assert obj is getattr(impl, name), name
        assert str(inspect.signature(obj)) == want[name], (name, str(inspect.signature(obj)), want[name])
    for name in CLASSES:
        cls = getattr(MP, name)
        assert inspect.isclass(cls) and not cls.__module__.startswith(pkg.__name__ + ".models_pytorch"), name
    with pytest.raises(AssertionError, match="depth, d_model and expansion_factor must agree in size, 2, 3 and 3 passed"):
        MP.ConvMLP([1, 1], [8, 8, 8], [1, 1, 1])
    assert isinstance(MP.ConvMLP([1], [8], [1], channels=8, classifier_head=False).head, type(None))


def test_no_url_and_no_download():
    assert MP.model_urls == {} and isinstance(MP.model_urls, dict)
    hub_before = "torch.hub" in sys.modules
    for fn in (MP.convmlp_s, MP.convmlp_m, MP.convmlp_l):
        with pytest.raises(RuntimeError, match="load_state_dict"):
            fn(pretrained=True)
    assert ("torch.hub" in sys.modules) == hub_before
    pkg = load_pkg()
    for mod in (MP, importlib.import_module(pkg.__name__ + ".convmlp_impl")):
        with open(mod.__file__) as f:
            src = f.read()
        assert "http" not in src and "torch.hub" not in src and "load_state_dict_from_url" not in src, mod.__file__


def test_state_dict_tables_match_reference(z):
    for name, fn in (("S", MP.convmlp_s), ("M", MP.convmlp_m), ("L", MP.convmlp_l)):
        want = json.loads(str(z["shapes/" + name]))
        model = fn()
        got = table(model)
        assert list(got) == list(want), name
        assert got == want, name
        sd = {k: torch.zeros(v, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in want.items()}
        model.load_state_dict(sd, strict=True)
    got = table(MP.convmlp_s())
    assert got["tokenizer.block.0.weight"] == [32, 3, 3, 3] and got["tokenizer.block.7.running_var"] == [64]
    assert got["conv_stages.conv_blocks.1.3.weight"] == [128, 128, 3, 3] and got["conv_stages.downsample.bias"] == [128]
    assert got["stages.1.blocks.3.connect.weight"] == [256, 1, 3, 3] and got["stages.0.downsample_mlp.downsample.weight"] == [256, 128, 3, 3]
    assert got["norm.weight"] == [512] and got["head.weight"] == [1000, 512]
    m = MP.convmlp_s()
    assert isinstance(m.tokenizer.block[1], torch.nn.BatchNorm2d) and isinstance(m.conv_stages.conv_blocks[0][3], torch.nn.Conv2d)


def test_fixture_holds_every_case_and_the_padding_condition(z, meta):
    """what the generator asserted before it wrote the file, and the cases the GPU tests expect"""
    assert meta["limits"] == {"min_beta_pad_over_gate": 5.0}
    assert meta["configs"] == CM.CONFIGS and [tuple(s) for s in meta["sizes"]] == CM.SIZES and meta["tiny_seed"] == CM.TINY_SEED
    probed = ["tiny/%s/%dx%d" % (c, h, w) for c in CM.CONFIGS for h, w in CM.SIZES] + ["block/mlpstage_48_96"]
    assert sorted(meta["beta_pad_over_gate"]) == sorted(probed) and all(v >= 5.0 for v in meta["beta_pad_over_gate"].values())
    for key, kind in CM.golden_keys().items():
        assert "%s/%s" % (key, kind) in z.files, key
        for tag in ("fp16", "bf16"):
            assert float(z["%s/err_%s" % (key, tag)]) > 0.0, (key, tag)
    assert z["real/S/logits"].shape == (2, 1000) and z["tiny/narrow/36x52/logits"].shape == (2, 10)
    assert z["headless/narrow/36x52/out"].shape == (2, 2, 2, 96) and z["block/tokenizer_64/out"].shape == (2, 64, 3, 4)
    assert z["block/convstage_1_32_64_64/out"].shape == (2, 64, 3, 3) and z["block/mlpstage_48_96/out"].shape == (2, 5, 7, 48)
    assert os.path.getsize(FIX) < 1 << 20


def test_entries_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    for name in ("mlpk_ln_dwconv3_nhwc", "mlpk_relu_add", "mlpk_relu_maxpool3s2_nhwc"):
        for n in (name, name + "_supported"):
            assert n in N.PROTOTYPES and "int %s(" % n in h, n
    assert "mlpk_convmlp.hip" in importlib.import_module("jittor-mlp_amd.build").SOURCES
    assert N.lib().mlpk_abi_version() == 14
    E = load_pkg().engine
    for f in ("ln_dwconv3_nhwc", "ln_dwconv3_supported", "relu_add", "relu_add_supported", "relu_maxpool3s2_nhwc", "relu_maxpool3s2_supported"):
        assert callable(getattr(E, f)), f


# ------------------------------------------------------------------ refusals and the _supported twins (nothing is dereferenced)
def test_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20                                             # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    base = dict(dtype=N.BF16, x=P, mean=P, rstd=P, gamma=P, beta=P, w=P, out=2 * P, res=3 * P, B=2, H=7, W=9, C=40, n=4096)

    def ln(**kw):
        k = dict(base, **kw)
        return lib.mlpk_ln_dwconv3_nhwc(k["dtype"], k["x"], k["mean"], k["rstd"], k["gamma"], k["beta"], k["w"], k["out"], k["B"], k["H"], k["W"], k["C"], None)

    def pool(**kw):
        k = dict(base, **kw)
        return lib.mlpk_relu_maxpool3s2_nhwc(k["dtype"], k["x"], k["out"], k["B"], k["H"], k["W"], k["C"], None)

    def radd(**kw):
        k = dict(base, **kw)
        return lib.mlpk_relu_add(k["dtype"], k["x"], k["res"], k["out"], k["n"], None)

    for kw in ({"x": None}, {"out": None}, {"w": None}, {"mean": None}, {"rstd": None}):
        assert ln(**kw) == ENULL, kw
    for kw in ({"x": None}, {"out": None}):
        assert pool(**kw) == ENULL and radd(**kw) == ENULL, kw
    for call in (ln, pool, radd):
        for bad in (3, 7, -1):
            assert call(dtype=bad) == EDTYPE and call(dtype=bad, C=0, n=0) == EDTYPE and call(dtype=bad, C=3, n=3) == EDTYPE     # whatever the shape
        assert call(x=P + 2) == EALIGN and call(out=2 * P + 8) == EALIGN and call(dtype=N.F32, x=P + 4) == EALIGN
    for call in (ln, pool):
        for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"C": 0}, {"C": 12}, {"C": 44}, {"dtype": N.F32, "C": 6}, {"dtype": N.F16, "C": 4}, {"out": P}):
            assert call(**kw) == ESHAPE, (call.__name__, kw)
    assert ln(B=1 << 30, H=64, W=64) == ESHAPE                                        # more workgroups than a grid holds
    for kw in ({"n": 0}, {"n": -8}, {"n": 4100}, {"dtype": N.F32, "n": 6}):
        assert radd(**kw) == ESHAPE, kw
    assert radd(res=3 * P + 4) == EALIGN


def test_supported_tables():
    N = load_pkg()._native
    lib = N.lib()
    SL, SP, SR = lib.mlpk_ln_dwconv3_nhwc_supported, lib.mlpk_relu_maxpool3s2_nhwc_supported, lib.mlpk_relu_add_supported
    rows = [  # (dtype, B, H, W, C) -> accepted
        ((N.BF16, 2, 1, 1, 8), 1), ((N.F16, 256, 28, 28, 128), 1), ((N.F32, 2, 1, 1, 4), 1), ((N.F32, 3, 9, 11, 12), 1), ((N.BF16, 3, 9, 11, 12), 0),
        ((N.F16, 1, 5, 5, 4), 0), ((N.F32, 1, 5, 5, 6), 0), ((N.BF16, 0, 5, 5, 8), 0), ((N.BF16, 1, 0, 5, 8), 0), ((N.BF16, 1, 5, -2, 8), 0),
        ((N.BF16, 1, 5, 5, 0), 0), ((5, 1, 5, 5, 8), 0), ((-1, 1, 5, 5, 8), 0), ((N.BF16, 256, 112, 112, 64), 1), ((N.F32, 2, 17, 33, 96), 1)]
    for args, want in rows:
        assert SL(*args) == want and SP(*args) == want, args
    assert SL(N.BF16, 1 << 30, 64, 64, 8) == 0 and SP(N.BF16, 1 << 30, 64, 64, 8) == 0      # more workgroups than a grid holds (2^35 tiles, 2^32 blocks)
    assert SL(N.BF16, 1 << 20, 64, 64, 8) == 1 and SP(N.BF16, 1 << 20, 64, 64, 8) == 1
    for (dtype, n), want in (((N.BF16, 8), 1), ((N.F16, 8008), 1), ((N.F32, 4), 1), ((N.F32, 12), 1), ((N.BF16, 12), 0), ((N.F32, 6), 0), ((N.BF16, 0), 0),
                             ((N.F16, -8), 0), ((4, 8), 0), ((N.BF16, 1 << 40), 1)):
        assert SR(dtype, n) == want, (dtype, n)


def test_conv_plan():
    plan = MP.conv_plan
    for dt in (torch.float16, torch.bfloat16):
        assert [plan(dt, c) for c in (32, 64, 96, 128, 256)] == ["window"] * 5
        assert [plan(dt, c) for c in (3, 16, 48, 8, 40, 0)] == ["gather"] * 6          # ConvMLP-L's tokenizer has Cin = 48
    assert [plan(torch.float32, c) for c in (16, 32, 48, 64, 128)] == ["gather"] * 5
    E = load_pkg().engine
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        for c in (8, 16, 32, 48, 64, 96, 128, 192):
            for stride in (1, 2):
                assert (plan(dt, c) == "window") == bool(E.conv_gemm_nhwc_supported(dt, c, 3, 3, stride, 1)), (dt, c, stride)


# ------------------------------------------------------------------ the packers, on CPU tensors
def test_batchnorm_scale_shift_against_torch_fp64():
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(6, 10, 3, 1, 1, bias=False).double()
    bn = torch.nn.BatchNorm2d(10).double().eval()
    with torch.no_grad():
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, 6, 5, 7, dtype=torch.float64)
    with torch.no_grad():
        want = F.batch_norm(F.conv2d(x, conv.weight, None, 1, 1), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        s, h = MP.bn_scale_shift(bn, torch.device("cpu"))
        assert s.dtype == torch.float32 and h.dtype == torch.float32 and s.data_ptr() != bn.weight.data_ptr()
        got = F.conv2d(x, conv.weight, None, 1, 1) * s.double().view(1, -1, 1, 1) + h.double().view(1, -1, 1, 1)
    assert float((got - want).abs().max()) <= 4e-7 * float(want.abs().max())          # the scale and shift travel as fp32


@pytest.mark.parametrize("stride", [1, 2])
def test_tap_major_columns_against_conv2d(stride):
    """conv3_columns puts the weight in the column order of the channel-last window: (i kw + j) Cin + ci"""
    torch.manual_seed(4)
    w = torch.randn(10, 6, 3, 3, dtype=torch.float64)
    x = torch.randn(2, 6, 5, 7, dtype=torch.float64)
    want = F.conv2d(x, w, None, stride, 1)
    cols = MP.conv3_columns(w)
    assert cols.shape == (10, 54)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))                               # channel-last, zero padded
    Ho, Wo = want.shape[2:]
    win = torch.stack([xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride] for i in range(3) for j in range(3)], 3)
    got = (win.reshape(2, Ho, Wo, 54) @ cols.t()).permute(0, 3, 1, 2)
    assert float((got - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------ the restatement, and what the kernel gate can tell
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_restatement_against_torch_fp64(shape):
    """the header's formula (per-pixel mean / rstd handed in, tap-major weights, zero padding behind the norm) is connect(connect_norm(x))"""
    x, mean, rstd, gamma, beta, w = CM.ln_operands(*shape, torch.float32)
    mu = x.mean(-1)
    rs = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)
    got = CM.restate_ln_dwconv3(x, mu, rs, gamma, beta, w, torch.float64)
    want = CM.torch_connect(x, gamma, beta, w)
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_gate_tells_planted_faults(dtype):
    """on the GPU test's own operands every planted fault but the last lies at least five gates away somewhere; `unrounded` is recorded"""
    worst = {f: 0.0 for f in CM.FAULTS}
    for shape in LN_SHAPES:
        ops = CM.ln_operands(*shape, dtype)
        ref = CM.restate_ln_dwconv3(*ops, dtype)
        gate = CM.ln_gate(EPS, dtype, ref)
        B, H, W, C = shape
        for fault in CM.FAULTS:
            applies = {"beta_pad": True, "adjacent_image": B > 1, "transposed_taps": H * W > 1, "wrong_mean": B * H * W > 1, "unrounded": True}[fault]
            d = float((CM.restate_ln_dwconv3(*ops, dtype, fault=fault) - ref).abs().max()) / gate
            worst[fault] = max(worst[fault], d)
            print("%s %s %s: %.2f gates" % (IDS[DTYPES.index(dtype)], "x".join(map(str, shape)), fault, d))
            if fault != "unrounded" and applies:
                assert d >= 5.0, (shape, fault, d)
    assert all(worst[f] >= 5.0 for f in CM.FAULTS[:4])
