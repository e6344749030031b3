"""-m gpu: ConvMLP on the MI355X.
  * mlpk_ln_dwconv3_nhwc alone, three dtypes, LN_SHAPES (B, H, W, C): one pixel, one row, one column, a 3 x 3 map, a map inside one tile with a
    ragged channel chunk (C = 40: five vectors of a chunk of eight), and 17 x 33 x 96 -- the kernel's tile is 8 x 16 pixels, so two whole tiles and a
    partial one in each axis, and two channel chunks.  Operands (tests/convmlp_model.py ln_operands): per-pixel means that differ by several sigma,
    the pixels' true statistics, gamma in +-[0.25, 2], beta in +-[2, 4].  Against the fp64 restatement of the header's formula under
    4 EPS[dtype] max(1, max|ref|), EPS the project's op gate (tests/test_gpu_ops.py); tests/test_convmlp_host.py holds that gate against planted
    faults on these operands.  As equalities: NULL statistics / NULL affine equal explicit 0 / 1 vectors, an image of a batch equals the image
    alone, two runs agree, a NaN-filled `out` is fully overwritten and x unchanged, a refused call leaves `out` untouched.
  * mlpk_relu_maxpool3s2_nhwc and mlpk_relu_add against torch's own max_pool2d(relu(.), 3, 2, 1) and res + relu(y) on the device in the same type,
    equal as numbers (a signed zero is a zero).
  * the family against tests/golden/convmlp.npz (the reference's own forwards, tests/golden/make_convmlp_golden.py): fp32 at
    1e-5 max(1, max|ref|), the 16-bit types at twice the reference's own distance in that type on the same case; a batch of 3 against its images
    alone; in-place updates of a LayerNorm weight, a convolution weight and a BatchNorm running_var against a twin loaded from the updated
    state_dict; train() warns; a width off the vector raises."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_pkg
from guard import assert_bits_equal, assert_finite
import convmlp_model as CM
from test_gpu_ops import EPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "convmlp.npz")
MP = load_pkg().models_pytorch.conv_mlp
DTYPES, IDS, LN_SHAPES = CM.DTYPES, CM.IDS, CM.LN_SHAPES
POOL_SHAPES = [(2, 1, 1, 8), (2, 2, 2, 8), (2, 5, 7, 40), (2, 6, 4, 8), (2, 33, 18, 64)]
RELU_GRID = 2048 * 256                                                 # vectors one grid of mlpk_relu_add covers (csrc/mlpk_convmlp.hip RELU_GRID_MAX)
RELU_N = [8, 8 * 1000 + 8, RELU_GRID * 8 + 8 * 77]                     # the last: past one grid of workgroups in every type
BYTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=IDS)


def engine():
    return load_pkg().engine


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


# ------------------------------------------------------------------ mlpk_ln_dwconv3_nhwc
def dev_ops(ops, dtype):
    x, mean, rstd, gamma, beta, w = ops
    return (x.to(dtype).to(DEV).contiguous(),) + tuple(t.float().to(DEV).contiguous() for t in (mean, rstd, gamma, beta, w))


def run_ln(d, shape, stats=True, affine=True, out=None):
    """the kernel on device operands d = (x, mean, rstd, gamma, beta, w) -> out (B, H, W, C)"""
    B, H, W, C = shape
    x, mean, rstd, gamma, beta, w = d
    if out is None:
        out = torch.full((B, H, W, C), float("nan"), dtype=x.dtype, device=DEV)
    engine().ln_dwconv3_nhwc(x, mean if stats else None, rstd if stats else None, gamma if affine else None, beta if affine else None, w, out, B, H, W, C)
    torch.cuda.synchronize()
    return out


LN_CASES = pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))


@LN_CASES
@BYTYPE
def test_ln_dwconv3_against_fp64_restatement(shape, dtype):
    ops = CM.ln_operands(*shape, dtype)
    ref = CM.restate_ln_dwconv3(*ops, dtype)
    d = dev_ops(ops, dtype)
    keep = d[0].clone()
    out = run_ln(d, shape)                                             # (`out` starts as NaN: every element must be written)
    assert_finite(out, "out")
    assert_bits_equal(d[0], keep, "x after the call")
    err, gate = float((out.double().cpu() - ref).abs().max()), CM.ln_gate(EPS, dtype, ref)
    print("ln_dwconv3 %s %s: |d| %.3e gate %.3e ratio %.3f (max|ref| %.3f)" % ("x".join(map(str, shape)), IDS[DTYPES.index(dtype)], err, gate, err / gate,
                                                                             float(ref.abs().max())))
    assert err <= gate, (err, gate)
    assert_bits_equal(run_ln(d, shape), out, "the second run")


@LN_CASES
@BYTYPE
def test_ln_dwconv3_null_operands_are_zero_and_one(shape, dtype):
    B, H, W, C = shape
    x, mean, rstd, gamma, beta, w = dev_ops(CM.ln_operands(*shape, dtype), dtype)
    zero, one = torch.zeros(B * H * W, device=DEV), torch.ones(B * H * W, device=DEV)
    assert_bits_equal(run_ln((x, None, None, gamma, beta, w), shape, stats=False), run_ln((x, zero, one, gamma, beta, w), shape), "NULL statistics")
    cz, co = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    assert_bits_equal(run_ln((x, mean, rstd, None, None, w), shape, affine=False), run_ln((x, mean, rstd, co, cz, w), shape), "NULL affine")
    assert_bits_equal(run_ln((x, mean, rstd, None, beta, w), shape), run_ln((x, mean, rstd, co, beta, w), shape), "NULL gamma alone")


@LN_CASES
@BYTYPE
def test_ln_dwconv3_image_of_a_batch_equals_the_image_alone(shape, dtype):
    B, H, W, C = shape
    x, mean, rstd, gamma, beta, w = dev_ops(CM.ln_operands(*shape, dtype), dtype)
    full = run_ln((x, mean, rstd, gamma, beta, w), shape)
    for b in range(B):
        alone = run_ln((x[b:b + 1].contiguous(), mean[b:b + 1].contiguous(), rstd[b:b + 1].contiguous(), gamma, beta, w), (1, H, W, C))
        assert_bits_equal(alone[0], full[b], "image %d alone" % b)


@BYTYPE
def test_ln_dwconv3_refusals_leave_out_untouched(dtype):
    pkg = load_pkg()
    N = pkg._native
    shape = (2, 3, 5, 8)
    B, H, W, C = shape
    x, mean, rstd, gamma, beta, w = dev_ops(CM.ln_operands(*shape, dtype), dtype)
    out = torch.full((B, H, W, C + 8), 3.0, dtype=dtype, device=DEV)
    keep = out.clone()
    code = engine().dtype_code(dtype)
    es = out.element_size()

    def call(dt=code, xp=x.data_ptr(), op=out.data_ptr(), mp=mean.data_ptr(), c=C, h=H):
        return N.lib().mlpk_ln_dwconv3_nhwc(dt, xp, mp, rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), op, B, h, W, c, None)
    assert call(dt=9) == -1 and call(xp=None) == -4 and call(mp=None) == -4 and call(c=C + (2 if es == 4 else 4)) == -2 and call(h=0) == -2
    assert call(xp=out.data_ptr()) == -2 and call(op=out.data_ptr() + es) == -3 and call(xp=x.data_ptr() + es) == -3
    torch.cuda.synchronize()
    assert_bits_equal(out, keep, "out after the refused calls")
    with pytest.raises(N.MlpkError, match="mlpk_ln_dwconv3_nhwc"):
        engine().ln_dwconv3_nhwc(x, mean, rstd, gamma, beta, w, x, B, H, W, C)


# ------------------------------------------------------------------ mlpk_relu_maxpool3s2_nhwc, mlpk_relu_add
def pool_input(shape, dtype, seed=3):
    return CM.case_input(shape, seed).to(dtype).to(DEV).contiguous()


def run_pool(y):
    B, H, W, C = y.shape
    out = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), float("nan"), dtype=y.dtype, device=DEV)
    engine().relu_maxpool3s2_nhwc(y, out, B, H, W, C)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@BYTYPE
def test_relu_maxpool_equals_torch(shape, dtype):
    y = pool_input(shape, dtype)
    keep = y.clone()
    out = run_pool(y)
    assert_finite(out, "out")
    assert_bits_equal(y, keep, "y after the call")
    want = F.max_pool2d(F.relu(y.permute(0, 3, 1, 2)), 3, 2, 1).permute(0, 2, 3, 1)
    assert out.shape == want.shape and torch.equal(out.float(), want.float())                 # equal as numbers
    assert bool((out >= 0).all())
    neg = run_pool(-y.abs() - 1)                                       # every window all negative: the padding (and the ReLU) gives 0
    assert torch.equal(neg.float(), torch.zeros_like(neg).float())
    for b in range(shape[0]):
        assert_bits_equal(run_pool(y[b:b + 1].contiguous())[0], out[b], "image %d alone" % b)


@BYTYPE
def test_relu_maxpool_keeps_a_nan_like_torch(dtype):
    """a NaN in a window is that window's result, wherever in the window it lies and whatever follows it; other windows do not see it"""
    y = pool_input((1, 7, 9, 8), dtype)
    for (r, c, ch) in ((0, 0, 0), (3, 4, 1), (4, 4, 2), (6, 8, 3), (2, 1, 4)):
        y[0, r, c, ch] = float("nan")
    out = run_pool(y)
    want = F.max_pool2d(F.relu(y.permute(0, 3, 1, 2)), 3, 2, 1).permute(0, 2, 3, 1)
    assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all())
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(out.float(), nan=-1.0), torch.nan_to_num(want.float(), nan=-1.0))


@BYTYPE
def test_relu_maxpool_refusals_leave_out_untouched(dtype):
    N = load_pkg()._native
    y = pool_input((2, 5, 7, 8), dtype)
    out = torch.full((2, 3, 4, 8), 3.0, dtype=dtype, device=DEV)
    keep = out.clone()
    code, f = engine().dtype_code(dtype), N.lib().mlpk_relu_maxpool3s2_nhwc
    assert f(9, y.data_ptr(), out.data_ptr(), 2, 5, 7, 8, None) == -1 and f(code, None, out.data_ptr(), 2, 5, 7, 8, None) == -4
    assert f(code, y.data_ptr(), out.data_ptr(), 2, 5, 7, 6, None) == -2 and f(code, out.data_ptr(), out.data_ptr(), 2, 5, 7, 8, None) == -2
    assert f(code, y.data_ptr(), out.data_ptr() + out.element_size(), 2, 5, 7, 8, None) == -3
    torch.cuda.synchronize()
    assert_bits_equal(out, keep, "out after the refused calls")


@pytest.mark.parametrize("n", RELU_N)
@BYTYPE
def test_relu_add_equals_torch(n, dtype):
    E = engine()
    y = CM.case_input((n,), 5).to(dtype).to(DEV)
    res = CM.case_input((n,), 6).to(dtype).to(DEV)
    want_plain, want_res = F.relu(y), res + F.relu(y)

    def same(got, want, what):
        torch.cuda.synchronize()
        assert torch.equal(got.float(), want.float()), what           # equal as numbers

    out = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
    ky, kr = y.clone(), res.clone()
    E.relu_add(y, None, out, n)
    same(out, want_plain, "relu(y)")
    out.fill_(float("nan"))
    E.relu_add(y, res, out, n)
    same(out, want_res, "res + relu(y)")
    assert_bits_equal(y, ky, "y")
    assert_bits_equal(res, kr, "res")
    a = y.clone()
    E.relu_add(a, None, a, n)                                          # out is y, without res
    same(a, want_plain, "in place, no res")
    a = y.clone()
    E.relu_add(a, res, a, n)                                           # out is y
    same(a, want_res, "out = y")
    assert_bits_equal(res, kr, "res")
    r = res.clone()
    E.relu_add(y, r, r, n)                                             # out is res
    same(r, want_res, "out = res")
    assert_bits_equal(y, ky, "y")
    a = y.clone()
    E.relu_add(a, a, a, n)                                             # all three one buffer: y + relu(y)
    same(a, y + F.relu(y), "out = y = res")


@BYTYPE
def test_relu_add_refusals_leave_out_untouched(dtype):
    N = load_pkg()._native
    y = CM.case_input((64,), 5).to(dtype).to(DEV)
    out = torch.full((64,), 3.0, dtype=dtype, device=DEV)
    keep = out.clone()
    code, f = engine().dtype_code(dtype), N.lib().mlpk_relu_add
    assert f(9, y.data_ptr(), None, out.data_ptr(), 64, None) == -1 and f(code, None, None, out.data_ptr(), 64, None) == -4
    assert f(code, y.data_ptr(), None, out.data_ptr(), 62, None) == -2 and f(code, y.data_ptr(), None, out.data_ptr(), 0, None) == -2
    assert f(code, y.data_ptr() + out.element_size(), None, out.data_ptr(), 32, None) == -3
    torch.cuda.synchronize()
    assert_bits_equal(out, keep, "out after the refused calls")


# ------------------------------------------------------------------ the family against the reference's own forwards
def build(key):
    """the module of a golden case on the CPU, with the fixture's parameters, and its input"""
    parts = key.split("/")
    if parts[0] in ("tiny", "headless"):
        h, w = (int(v) for v in parts[2].split("x"))
        model = MP.ConvMLP(num_classes=CM.TINY_CLASSES, classifier_head=parts[0] == "tiny", **CM.CONFIGS[parts[1]])
        return CM.prepare(model, CM.TINY_SEED), CM.case_input((2, 3, h, w), CM.TINY_SEED)
    if parts[0] == "block":
        cls, args, shape = CM.BLOCKS[parts[1]]
        return CM.prepare(getattr(MP, cls)(*args), CM.BLOCK_SEED), CM.case_input(shape, CM.BLOCK_SEED)
    return CM.prepare(MP.convmlp_s(), 0), CM.case_input((2, 3, 224, 224), 0)


@functools.lru_cache(maxsize=None)
def device_case(key):
    model, x = build(key)
    return model.to(DEV), x.to(DEV)


@pytest.mark.parametrize("key", list(CM.golden_keys()))
@BYTYPE
def test_forward_against_reference(z, key, dtype):
    model, x = device_case(key)
    ref = torch.from_numpy(z["%s/%s" % (key, CM.golden_keys()[key])])
    with torch.no_grad():
        out = model(x.to(dtype))
    torch.cuda.synchronize()
    assert out.dtype == dtype and tuple(out.shape) == tuple(ref.shape)
    assert_finite(out, key)
    name = IDS[DTYPES.index(dtype)]
    gate = 1e-5 * max(1.0, float(ref.abs().max())) if dtype == torch.float32 else 2.0 * float(z["%s/err_%s" % (key, name)])
    err = float((out.float().cpu() - ref).abs().max())
    print("%s %s: |d| %.3e gate %.3e ratio %.3f (max|ref| %.3f)" % (key, name, err, gate, err / gate, float(ref.abs().max())))
    assert err <= gate, (key, name, err, gate)


@pytest.mark.parametrize("key", ["tiny/wide/36x52", "tiny/narrow/36x52", "headless/narrow/36x52", "block/mlpstage_48_96", "block/convstage_1_32_64_64"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_of_three_equals_the_images_alone(key, dtype):
    model, x = device_case(key)
    x3 = torch.cat([x, x[:1].flip(-1)], 0).to(dtype)
    keep = x3.clone()
    with torch.no_grad():
        full = model(x3).clone()
        for b in range(3):
            assert_bits_equal(model(x3[b:b + 1].contiguous())[0], full[b], "image %d alone" % b)
        again = model(x3)
    assert_bits_equal(again, full, "the second run")
    assert again.data_ptr() != full.data_ptr()                         # results are the caller's
    assert_bits_equal(x3, keep, "the input")


UPDATES = {
    "layernorm weight": lambda m: m.stages[0].blocks[0].connect_norm.weight,
    "layernorm bias": lambda m: m.stages[1].blocks[1].norm2.bias,
    "dense conv weight": lambda m: m.conv_stages.conv_blocks[0][3].weight,
    "depthwise conv weight": lambda m: m.stages[1].blocks[0].connect.weight,
    "batchnorm running_var": lambda m: m.tokenizer.block[4].running_var,
    "batchnorm running_mean": lambda m: m.conv_stages.conv_blocks[1][7].running_mean,
}


@pytest.mark.parametrize("what", list(UPDATES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_in_place_update_reaches_the_next_forward(what, dtype):
    """the engine's stamp covers parameters AND buffers: after an in-place change the warm model equals a twin built from its state_dict"""
    model, x = build("tiny/wide/36x52")
    model, x = model.to(DEV), x.to(DEV).to(dtype)
    with torch.no_grad():
        before = model(x).clone()
        t = UPDATES[what](model)
        t.mul_(1.5).add_(0.25)
        after = model(x).clone()
        twin = MP.ConvMLP(num_classes=CM.TINY_CLASSES, **CM.CONFIGS["wide"])
        twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
        want = twin.to(DEV).eval()(x)
    assert not torch.equal(after, before), "the update was a no-op: the case checks nothing"
    assert_bits_equal(after, want, "the warm model after the update")


def test_train_mode_warns_inference_only():
    model, x = build("tiny/narrow/36x52")
    model, x = model.to(DEV), x.to(DEV)
    model.train()
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(x)
    assert out.grad_fn is None
    with torch.enable_grad():
        assert model(x).grad_fn is None
    assert_bits_equal(out, device_case("tiny/narrow/36x52")[0](x), "train mode")


@BYTYPE
def test_width_off_the_vector_raises(dtype):
    """channels = 36: the tokenizer's inner width is 18.  NotImplementedError naming the entry and the width, nothing launched, no fallback"""
    model = MP.ConvMLP([1, 1], [48, 64], [1, 1], channels=36, n_conv_blocks=1, num_classes=3).to(DEV).eval()
    with pytest.raises(NotImplementedError, match=r"mlpk_relu_add.*18"):
        model(torch.zeros(1, 3, 32, 32, device=DEV, dtype=dtype))
    with pytest.raises(NotImplementedError, match=r"mlpk_ln_dwconv3_nhwc.*20"):
        MP.ConvMLPStage(20, 40).to(DEV)(torch.zeros(1, 4, 4, 20, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        MP.ConvMLPStage(16, 32).to(DEV)(torch.zeros(1, 4, 4, 24, device=DEV))
