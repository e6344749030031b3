"""-m gpu: RaftMLP on the MI355X.
  * mlpk_raft_gather_ln / mlpk_raft_scatter_add alone, behind guard bands (tests/guard.py), both axes, three dtypes, tight and padded pitches.  The
    gates are equalities: the gather against mlpk_norm_apply's row-major output re-laid with torch indexing, the scatter against
    (x.float() + y_relaid.float()).to(dtype), an index-code check that names the (b, q, co, j, l) of a misplaced element, and a round trip;
  * the whole model against tests/golden/raft_mlp.npz (the reference's own forwards, tests/golden/make_raft_golden.py): the tiny configuration
    for every mixing type and head variant, the blocks alone, "pyramid" and "single" at 224 x 224 in fp32 / fp16 / bf16;
  * determinism: two forwards give the same bits, and so do two forwards in flight (parallel.InFlight).
16-bit model gates are derived as tests/test_gpu_wave.py derives them: twice the reference's own 16-bit distance from its fp32 logits (relative to
max |logit|), scaled by max |ref| of the case at hand."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
from exact import INT_RANGE
from guard import Guarded, assert_bits_equal, assert_finite
from oracle.portable_init import portable_input, portable_state_dict, portable_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "raft_mlp.npz")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
SHAPES = [(56, 56, 96, 2), (28, 28, 192, 2), (14, 14, 384, 2), (7, 7, 768, 2), (14, 14, 768, 4), (5, 3, 16, 4), (7, 9, 24, 1), (1, 1, 8, 2),
          (3, 4, 40, 2), (6, 5, 24, 4)]
B = 2


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def mp():
    return load_pkg().models_pytorch


def engine():
    return load_pkg().engine


def load_portable(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = portable_state_dict(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


# ------------------------------------------------------------------ the kernels alone
def geom(H, W, C, r, axis):
    L, Q = (H, W) if axis == 0 else (W, H)
    return L, Q, C // r, r * L


def relay(x4, r, axis):
    """(B, H, W, C) -> the operand rows (B Q Co, r L): row (b, q, co), column j L + l  <-  x[b, pix(l, q), j Co + co]"""
    Bn, H, W, C = x4.shape
    L, Q, Co, D = geom(H, W, C, r, axis)
    v = x4.reshape(Bn, H, W, r, Co)
    v = v.permute(0, 2, 4, 3, 1) if axis == 0 else v.permute(0, 1, 4, 3, 2)
    return v.reshape(Bn * Q * Co, D)


def unrelay(y, Bn, H, W, C, r, axis):
    """the inverse: rows (B Q Co, r L) -> (B, H, W, C)"""
    L, Q, Co, D = geom(H, W, C, r, axis)
    v = y.reshape(Bn, Q, Co, r, L)
    v = v.permute(0, 4, 1, 3, 2) if axis == 0 else v.permute(0, 1, 4, 3, 2)
    return v.reshape(Bn, H, W, C)


def pitches(D, C, pad):
    """tight: kp = D (a partial last 16-byte piece where D % 8 != 0), the smallest aligned pitch; padded: kp = D rounded up to 32, pitches + 8"""
    if pad:
        kp = (D + 31) // 32 * 32
        return kp, kp + 8, C + 8, (D + 7) // 8 * 8 + 8
    return D, (D + 7) // 8 * 8, C, (D + 7) // 8 * 8


def rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


CASES = pytest.mark.parametrize("H,W,C,r", SHAPES)
AXES = pytest.mark.parametrize("axis", [0, 1], ids=["vertical", "horizontal"])
TYPES = pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
PADS = pytest.mark.parametrize("pad", [0, 1], ids=["tight", "padded"])


def run_gather(x, mean, rstd, gamma, beta, H, W, C, r, axis, dtype, pad):
    """x (B H W, C) cpu -> (Guarded x, Guarded a, kp) after the call"""
    E = engine()
    L, Q, Co, D = geom(H, W, C, r, axis)
    kp, lda, ldx, _ = pitches(D, C, pad)
    gx = Guarded(B * H * W, C, ldx, dtype, DEV, role="in", data=x)
    ga = Guarded(B * Q * Co, kp, lda, dtype, DEV, role="out")
    E.raft_gather_ln(gx.view, mean, rstd, gamma, beta, ga.view, kp, B, H, W, C, r, axis)
    torch.cuda.synchronize()
    gx.check()
    ga.check()                                                  # lead, tail and the columns [kp, lda) of every row untouched
    assert_finite(ga.view, "gathered operand")
    return gx, ga, kp


@CASES
@AXES
@TYPES
@PADS
def test_gather_matches_norm_apply(H, W, C, r, axis, dtype, pad):
    E = engine()
    rows = B * H * W
    L, Q, Co, D = geom(H, W, C, r, axis)
    seed = H * 1000 + W * 100 + C + axis
    x = rand((rows, C), seed, -2.0, 2.0).to(dtype)
    mean, rstd = rand((rows,), seed + 1).to(DEV), rand((rows,), seed + 2, 0.5, 2.0).to(DEV)
    gamma, beta = rand((C,), seed + 3, 0.25, 4.0).to(DEV), rand((C,), seed + 4).to(DEV)
    gx, ga, kp = run_gather(x, mean, rstd, gamma, beta, H, W, C, r, axis, dtype, pad)
    ref = torch.empty((rows, C), dtype=dtype, device=DEV)
    E.norm_apply(gx.view, rows, C, gx.ld, mean=mean, rstd=rstd, gamma=gamma, beta=beta, out_rm=ref, ld_rm=C)
    torch.cuda.synchronize()
    got = ga.dense()
    assert_bits_equal(got[:, :D].contiguous(), relay(ref.view(B, H, W, C), r, axis).contiguous(), "gathered operand")
    if kp > D:
        assert bool((got[:, D:].view(guard_int(dtype)) == 0).all()), "columns [D, kp) must be +0"


def guard_int(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


@CASES
@AXES
@TYPES
@PADS
def test_scatter_adds_the_relaid_rows(H, W, C, r, axis, dtype, pad):
    E = engine()
    rows = B * H * W
    L, Q, Co, D = geom(H, W, C, r, axis)
    _, _, ldx, ldy = pitches(D, C, pad)
    seed = H * 1000 + W * 100 + C + axis + 7
    x = rand((rows, C), seed, -2.0, 2.0).to(dtype)
    y = rand((B * Q * Co, D), seed + 1, -2.0, 2.0).to(dtype)
    gx = Guarded(rows, C, ldx, dtype, DEV, role="inout", data=x)
    gy = Guarded(B * Q * Co, D, ldy, dtype, DEV, role="in", data=y)
    E.raft_scatter_add(gx.view, gy.view, B, H, W, C, r, axis)
    torch.cuda.synchronize()
    gx.check()                                                  # pad columns of x, lead and tail untouched
    gy.check()                                                  # all of y unchanged
    want = (x.float().view(B, H, W, C) + unrelay(y.float(), B, H, W, C, r, axis)).to(dtype).reshape(rows, C)
    assert_bits_equal(gx.dense().cpu(), want, "scattered map")


def codes(H, W, C, which):
    """small-integer codes of (b, h, w, c), exact in bf16: three residues, one per pass"""
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    w = torch.arange(W).view(1, 1, W, 1)
    c = torch.arange(C).view(1, 1, 1, C)
    m = 251
    code = ((c + 0 * (b + h + w)) % m, (h * W + w + 0 * (b + c)) % m, (b * 97 + h * 31 + w * 7 + c * 3) % m)[which]
    return code.expand(B, H, W, C).contiguous()


@CASES
@AXES
@TYPES
def test_gather_index_code(H, W, C, r, axis, dtype):
    """a[row (b, q, co), column j L + l] holds the code of x[b, pix(l, q), j Co + co]: tells (j co) from (co j) and (j l) from (l j)"""
    L, Q, Co, D = geom(H, W, C, r, axis)
    assert INT_RANGE[torch.bfloat16] >= 251
    for which in range(3):
        code = codes(H, W, C, which)
        x = code.reshape(B * H * W, C).to(torch.float32).to(dtype)
        _, ga, _ = run_gather(x, None, None, None, None, H, W, C, r, axis, dtype, 0)
        got = ga.dense()[:, :D].float().cpu().view(B, Q, Co, r, L)
        b, q, co, j, l = torch.meshgrid(torch.arange(B), torch.arange(Q), torch.arange(Co), torch.arange(r), torch.arange(L), indexing="ij")
        hh, ww = (l, q) if axis == 0 else (q, l)
        want = code[b, hh, ww, j * Co + co].float()
        bad = torch.nonzero(got != want)
        if len(bad):
            ib, iq, ico, ij, il = bad[0].tolist()
            raise AssertionError("code %d: a[(b %d, q %d, co %d), (j %d, l %d)] = %g, its source holds %g (%d elements differ)" % (
                which, ib, iq, ico, ij, il, float(got[ib, iq, ico, ij, il]), float(want[ib, iq, ico, ij, il]), len(bad)))


@CASES
@AXES
@TYPES
def test_gather_scatter_round_trip(H, W, C, r, axis, dtype):
    E = engine()
    rows = B * H * W
    L, Q, Co, D = geom(H, W, C, r, axis)
    x = rand((rows, C), H + W + C + axis, -2.0, 2.0).to(dtype)
    _, ga, _ = run_gather(x, None, None, None, None, H, W, C, r, axis, dtype, 1)
    back = torch.zeros((rows, C), dtype=dtype, device=DEV)
    E.raft_scatter_add(back, ga.view, B, H, W, C, r, axis)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), x)


# ------------------------------------------------------------------ the model against the reference
def lowp_gate(z, dtype, m, cfg="pyramid"):
    """2 x the reference's own 16-bit distance from its fp32 logits (relative to its max |logit|), scaled by max |ref| of the case"""
    tag = "fp16" if dtype == torch.float16 else "bf16"
    rel = float(z["real/%s/err_%s" % (cfg, tag)]) / float(np.abs(z["real/%s/logits" % cfg]).max())
    return 2.0 * rel * m


def check(out, ref, dtype, z, cfg="pyramid"):
    m = float(np.abs(ref).max())
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    gate = 1e-5 * m if dtype == torch.float32 else lowp_gate(z, dtype, m, cfg)
    print("%s: max|d| %.3e gate %.3e max|ref| %.3f" % (dtype, err, gate, m))
    assert err <= gate, (str(dtype), err, gate, m)


def tiny_model(meta, case):
    kw = meta["tiny_cases"][case]
    model = load_portable(mp().RaftMLP(meta["tiny"], num_classes=10, **kw), meta["tiny_seed"]).to(DEV).eval()
    x = torch.from_numpy(portable_input((2, 3, kw["image_size"], kw["image_size"]), seed=meta["tiny_seed"])).to(DEV)
    return model, x


@pytest.mark.parametrize("case", ["ser_pm", "sep_ln_codim_tm", "sep_ln_ch_tm", "original_tm", "ser_pm_nogap", "ser_pm_noshortcut",
                                  "ser_pm_nogap_noshortcut", "ser_pm_42"])
def test_tiny_logits_fp32(case, z, meta):
    model, x = tiny_model(meta, case)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 10)
    check(out, z["tiny/" + case], torch.float32, z)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ["ser_pm", "ser_pm_nogap", "ser_pm_noshortcut", "ser_pm_42"])
def test_tiny_logits_16bit(case, dtype, z, meta):
    model, x = tiny_model(meta, case)
    with torch.no_grad():
        out = model(x.to(dtype))
    assert out.dtype == dtype
    check(out, z["tiny/" + case], dtype, z)


def test_tiny_compute_dtype(z, meta):
    """set_compute_dtype: fp32 input, bf16 kernels, fp32 logits"""
    model, x = tiny_model(meta, "ser_pm")
    model.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32
    ref = z["tiny/ser_pm"]
    m = float(np.abs(ref).max())
    assert float(np.abs(out.cpu().numpy() - ref).max()) <= lowp_gate(z, torch.bfloat16, m)


def test_wrong_input_size_raises(meta):
    model, x = tiny_model(meta, "ser_pm")
    with pytest.raises(ValueError):
        model(x[:, :, :36, :36])


@pytest.mark.parametrize("name", ["permuted_5_16_4", "permuted_7_24_2", "permuted_14_96_2", "separated_7_24", "channel_24"])
def test_blocks_alone_fp32(name, z, meta):
    rm = mp().raft_mlp
    cls, args, _ = meta["blocks"][name]
    blk = load_portable(getattr(rm, cls)(*args), meta["block_seed"])
    ln = blk.norm[1] if isinstance(blk.norm, torch.nn.Sequential) else blk.norm
    with torch.no_grad():                                       # tests/golden/make_raft_golden.py wide_affine
        ln.weight.copy_(torch.from_numpy(portable_tensor("norm.weight", tuple(ln.weight.shape), 0.25, 4.0, seed=meta["block_seed"])))
        ln.bias.copy_(torch.from_numpy(portable_tensor("norm.bias", tuple(ln.bias.shape), -1.0, 1.0, seed=meta["block_seed"])))
    blk = blk.to(DEV).eval()
    x = torch.from_numpy(portable_input(tuple(meta["block_inputs"][name]), seed=meta["block_seed"])).to(DEV)
    with torch.no_grad():
        out = blk(x)
    ref = z["block/" + name]
    assert tuple(out.shape) == ref.shape and out.dtype == torch.float32
    m = float(np.abs(ref).max())
    err = float(np.abs(out.cpu().numpy() - ref).max())
    assert err <= 1e-5 * m, (err, m)


@pytest.fixture(scope="module")
def real_models(meta):
    return {name: load_portable(mp().RaftMLP(meta["real"][name], gap=True), 0).to(DEV).eval() for name in ("pyramid", "single")}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["pyramid", "single"])
def test_real_logits(real_models, name, dtype, z):
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = real_models[name](x.to(dtype))
    check(out, z["real/%s/logits" % name], dtype, z, name)


def test_pyramid_takes_the_fused_route(real_models):
    """16-bit: the raft MLP of the levels whose zero-padded D lies in mlpk_channel_mlp's range (64 .. 192) runs on the fused entry; the pack
    records it, as wave_mlp.pack_block records ff.fused"""
    E = engine()
    model = real_models["pyramid"]
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV).bfloat16()
    with torch.no_grad():
        model(x)
    pk = model._packs[(torch.bfloat16, DEV)][1]
    sizes = [56, 28, 14, 7]
    for li, layer in enumerate(model.layers):
        dp = (layer["raft_size"] * sizes[li] + 31) // 32 * 32
        want = E.channel_mlp_fused_supported(torch.bfloat16, dp, 2 * layer["raft_size"] * sizes[li])
        assert want == (li < 2), (li, dp)                       # padded D = 128, 64: taken; 32, 32: below the kernel's range
        for bi in range(layer["depth"]):
            for half in "vh":
                assert (("l%d.b%d.%s.fused" % (li, bi, half)) in pk) == want, (li, bi, half)
    pk32 = None
    with torch.no_grad():
        model(x.float())
    pk32 = model._packs[(torch.float32, DEV)][1]
    assert not [k for k in pk32 if k.endswith(".fused")]       # fp32: always the GEMM pair


def test_reference_layout_state_dict_strict(z, meta):
    """a state_dict in the reference's layout (keys and shapes of the fixture's table) loads with strict=True and is what the forward uses"""
    shapes = {k: tuple(v) for k, v in json.loads(str(z["shapes/pyramid"])).items()}
    sd = {k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}
    model = mp().RaftMLP(meta["real"]["pyramid"], gap=True)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model = model.to(DEV).eval()
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = model(x)
    check(out, z["real/pyramid/logits"], torch.float32, z)


def test_deterministic_and_in_flight(meta):
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    model, _ = tiny_model(meta, "ser_pm")
    xs = [torch.from_numpy(portable_input((4, 3, 40, 40), seed=90 + i)).to(DEV).bfloat16() for i in range(4)]
    with torch.no_grad():
        serial = [model(x).clone() for x in xs]
        again = [model(x).clone() for x in xs]
        for a, b in zip(serial, again):
            assert torch.equal(a, b)
        slots = parallel.InFlight(model, 2, device=DEV)
        try:
            pending = [slots(x) for x in xs]
            slots.synchronize()
        finally:
            slots.restore_plan()
    for (out, _), want in zip(pending, serial):
        assert torch.equal(out, want)
    assert len({id(s) for _, s in pending}) == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_weight_update_reaches_the_next_forward(dtype, meta):
    """packed weights follow the parameters: an in-place update of a raft block's LayerNorm weight, of its second Linear and of the classifier
    bias each changes the next forward to what a freshly built model with those weights gives"""
    model, x = tiny_model(meta, "ser_pm")
    x = x.to(dtype)
    with torch.no_grad():
        before = model(x).clone()
        blk = model.levels[1].fn[2][3]
        blk.norm[1].weight.mul_(1.5)
        blk.fn[3].weight.mul_(-1.0)
        model.classifier.bias.add_(0.5)
        after = model(x).clone()
    assert not torch.equal(before, after)
    twin = mp().RaftMLP(meta["tiny"], num_classes=10, **meta["tiny_cases"]["ser_pm"])
    twin.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    with torch.no_grad():
        assert torch.equal(twin.to(DEV).eval()(x), after)


def test_train_mode_warns_inference_only(meta):
    model, x = tiny_model(meta, "ser_pm")
    model.train()
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(x)
    assert out.grad_fn is None
