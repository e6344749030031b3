"""-m gpu: WaveMLP on the MI355X.
  * mlpk_wave_patm alone against an fp64 restatement written here (F.conv2d with groups = C on the concatenated cos / sin tensor, on the CPU),
    at WaveMLP's stage shapes and small / odd maps, |theta| up to ~50; and a channel-pairing check with one-hot taps;
  * the whole model against tests/golden/wave_mlp.npz (the reference's own forwards, tests/golden/make_wave_golden.py): tiny T and M at
    64 x 48, T at 224 x 224, in fp32 / fp16 / bf16; Block and PATM called alone; PATM at large phases;
  * determinism: two forwards give the same bits, and so do two forwards in flight (parallel.InFlight).
16-bit model gates are derived from the reference's own 16-bit forward (its distance from its fp32 logits, relative to max |logit|, x 2), scaled
by max |ref| of the case at hand -- logits here are 0.2 - 0.35, where a gate floored at 1 would say nothing."""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_pkg
from oracle.portable_init import portable_input, portable_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "wave_mlp.npz")
STAGE_DIMS = (64, 128, 320, 512)
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def mp():
    return load_pkg().models_pytorch


def load_portable(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = portable_state_dict(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def sample_pin(t):
    """tests/golden/make_golden.py's sample_pin, restated: fp64 sum and |.| sum, then every 17th element (at most 4096)"""
    f = t.detach().double().cpu().reshape(-1)
    return np.concatenate([[f.sum().item(), f.abs().sum().item()], f[::17][:4096].numpy()])


# ------------------------------------------------------------------ the kernel alone
def ref_patm(y, wh, ww, B, H, W, C):
    """fp64 restatement of wave_mlp.py:46-60 after the 1 x 1 convolutions: y (rows, >= 5C) float64 -> h, w as (rows, C)"""
    Y = y[:, :5 * C].reshape(B, H, W, 5 * C).permute(0, 3, 1, 2)
    th, tw, xh, xw = Y[:, :C].relu(), Y[:, C:2 * C].relu(), Y[:, 2 * C:3 * C], Y[:, 3 * C:4 * C]
    ph = torch.cat([xh * torch.cos(th), xh * torch.sin(th)], dim=1)
    pw = torch.cat([xw * torch.cos(tw), xw * torch.sin(tw)], dim=1)
    h = F.conv2d(ph, wh.reshape(C, 2, 1, 7), padding=(0, 3), groups=C)
    w = F.conv2d(pw, ww.reshape(C, 2, 7, 1), padding=(3, 0), groups=C)
    return [t.permute(0, 2, 3, 1).reshape(B * H * W, C) for t in (h, w)]


def run_kernel(y, wh, ww, B, H, W, C, ldo):
    E = load_pkg().engine
    rows = B * H * W
    out = torch.full((rows, ldo), 7.0, dtype=y.dtype, device=DEV)      # sentinel: what the kernel must not touch
    E.wave_patm(y, wh, ww, out[:, :C], out[:, C:], B, H, W, C)
    torch.cuda.synchronize()
    return out


def make_y(B, H, W, C, ldy, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rows = B * H * W
    y = torch.full((rows, ldy), float("nan"), dtype=torch.float32)    # columns past 5C must never be read
    y[:, :2 * C] = torch.rand((rows, 2 * C), generator=g) * 60.0 - 10.0          # theta in [-10, 50)
    y[:, 2 * C:5 * C] = torch.randn((rows, 3 * C), generator=g)
    wh = (torch.rand((C, 2, 7), generator=g) * 2 - 1) / math.sqrt(14)
    ww = (torch.rand((C, 2, 7), generator=g) * 2 - 1) / math.sqrt(14)
    return y.to(dtype), wh, ww


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("pad", [0, 8], ids=["ldy5C", "ldy5C+8"])
@pytest.mark.parametrize("H,W,C", [(56, 56, 64), (28, 28, 128), (14, 14, 320), (7, 7, 512), (1, 1, 64), (12, 9, 40), (2, 2, 512), (3, 4, 128)])
def test_wave_patm_kernel(H, W, C, pad, dtype):
    B = 2
    ldy, ldo = 5 * C + pad, 2 * C + pad
    y, wh, ww = make_y(B, H, W, C, ldy, dtype, seed=H * 1000 + W * 10 + C)
    out = run_kernel(y.to(DEV), wh.to(DEV), ww.to(DEV), B, H, W, C, ldo)
    rh, rw = ref_patm(y.double(), wh.double(), ww.double(), B, H, W, C)   # from the values as stored
    got = out.double().cpu()
    ref = torch.cat([rh, rw], dim=1)
    m = ref.abs().max().item()
    err = (got[:, :2 * C] - ref).abs()
    if dtype == torch.float32:
        assert err.max().item() <= 1e-5 * m, (err.max().item(), m)
    else:                                                       # one storage rounding of a result within the fp32 error
        bound = HALF_ULP[dtype] * (ref.abs() + 1e-5 * m) + 1e-5 * m
        assert bool((err <= bound).all()), (err - bound).max().item()
    if pad:
        assert bool((got[:, 2 * C:] == 7.0).all()), "columns past 2C of the output were written"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wave_patm_channel_pairing(dtype):
    """One-hot centre taps: h[..., g] = P_h[2g + i] at the same pixel.  For g < C/2 that is x_h[2g + i] cos(theta_h[2g + i]), for g >= C/2 it is
    x_h[2g - C + i] sin(theta_h[2g - C + i]) -- NOT cos / sin of channel g, which is what a kernel pairing them that way would give."""
    B, H, W, C = 1, 5, 6, 32
    y, _, _ = make_y(B, H, W, C, 5 * C, dtype, seed=5)
    wh = torch.zeros((C, 2, 7))
    ww = torch.zeros((C, 2, 7))
    picks = [(0, 1), (3, 0), (C // 2 - 1, 1), (C // 2, 0), (C // 2 + 5, 1), (C - 1, 0)]
    for g, i in picks:
        wh[g, i, 3] = 1.0
        ww[g, i, 3] = 1.0
    out = run_kernel(y.to(DEV), wh.to(DEV), ww.to(DEV), B, H, W, C, 2 * C).float().cpu()
    yf = y.float()
    for g, i in picks:
        src = 2 * g + i if g < C // 2 else 2 * g - C + i
        fn = torch.cos if g < C // 2 else torch.sin
        for br, off in ((0, 0), (1, C)):
            th, x = yf[:, off + src].relu(), yf[:, 2 * C + off + src]
            want = x * fn(th)
            wrong = yf[:, 2 * C + off + g] * fn(yf[:, off + g].relu())
            got = out[:, br * C + g]
            tol = 1e-5 if dtype == torch.float32 else 2 ** -8 * want.abs().max().item() + 1e-5
            assert (got - want).abs().max().item() <= tol, (g, i, br)
            assert (got - wrong).abs().max().item() > 10 * tol, (g, i, br)
        others = [c for c in range(C) if c not in {p[0] for p in picks}]
        assert float(out[:, others].abs().max()) == 0.0 and float(out[:, [C + c for c in others]].abs().max()) == 0.0


# ------------------------------------------------------------------ the model against the reference
def lowp_gate(z, dtype, m):
    """2 x the reference's own 16-bit distance from its fp32 logits (relative to its max |logit|), scaled by max |ref| of the case"""
    tag = "fp16" if dtype == torch.float16 else "bf16"
    rel = float(z["real/err_" + tag]) / float(np.abs(z["real/logits"]).max())
    return 2.0 * rel * m


def check(out, ref, dtype, z):
    m = float(np.abs(ref).max())
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    gate = 1e-5 * m if dtype == torch.float32 else lowp_gate(z, dtype, m)
    assert err <= gate, (str(dtype), err, gate, m)
    return err


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["T", "M"])
def test_tiny_logits(name, dtype, z, meta):
    model = load_portable(mp().WaveMLP(name, num_classes=10), meta["tiny_seed"]).to(DEV).eval()
    x = torch.from_numpy(portable_input((2, 3) + tuple(meta["tiny_hw"]), seed=meta["tiny_seed"])).to(DEV)
    with torch.no_grad():
        out = model(x.to(dtype))
    assert out.dtype == dtype and tuple(out.shape) == (2, 10)
    check(out, z["tiny/%s/logits" % name], dtype, z)


def test_tiny_compute_dtype(z, meta):
    """set_compute_dtype: fp32 input, bf16 kernels, fp32 logits"""
    model = load_portable(mp().WaveMLP("T", num_classes=10), meta["tiny_seed"]).to(DEV).eval().set_compute_dtype(torch.bfloat16)
    x = torch.from_numpy(portable_input((2, 3) + tuple(meta["tiny_hw"]), seed=meta["tiny_seed"])).to(DEV)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32
    ref = z["tiny/T/logits"]
    m = float(np.abs(ref).max())
    assert float(np.abs(out.cpu().numpy() - ref).max()) <= lowp_gate(z, torch.bfloat16, m)


@pytest.fixture(scope="module")
def real_model():
    return load_portable(mp().WaveMLP("T"), 0).to(DEV).eval()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_real_logits(real_model, dtype, z):
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = real_model(x.to(dtype))
    check(out, z["real/logits"], dtype, z)


@pytest.mark.parametrize("name", ["T", "M"])
@pytest.mark.parametrize("stage", [0, 2, 4, 6])
def test_stage_pins(name, stage, z, meta):
    """model.network[s][0](x) and model.network[s][0].attn(x) called alone on (B, C, H, W), as in the reference (fp32)"""
    model = load_portable(mp().WaveMLP(name, num_classes=10), meta["tiny_seed"]).to(DEV).eval()
    h, w = meta["tiny_hw"]
    h, w = (h + 4 - 7) // 4 + 1, (w + 4 - 7) // 4 + 1
    for _ in range(stage // 2):
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    xs = torch.from_numpy(portable_input((2, STAGE_DIMS[stage // 2], h, w), seed=meta["pin_seed"] + stage)).to(DEV)
    blk = model.network[stage][0]
    with torch.no_grad():
        for what, fn in (("block", blk), ("attn", blk.attn)):
            out = fn(xs)
            assert tuple(out.shape) == tuple(xs.shape) and out.dtype == torch.float32
            got, want = sample_pin(out), z["tiny/%s/pin/%d/%s" % (name, stage, what)]
            m = np.abs(want[2:]).max()
            assert np.abs(got[2:] - want[2:]).max() <= 1e-5 * m, (what, np.abs(got[2:] - want[2:]).max(), m)
            assert abs(got[0] - want[0]) <= 1e-5 * want[1] and abs(got[1] - want[1]) <= 1e-5 * want[1], what


def test_patm_large_phases(z, meta):
    """PATM alone with theta reaching |theta| ~ 50 (the reference's output in the fixture).  Gate 1e-4 of max |ref|: at |theta| = 48 one fp32
    rounding of theta itself (2^-19 ~ 1.9e-6, already different between the GEMM here and the reference's convolution) moves cos / sin by as
    much, and 14 taps of weight ~0.27 on |x| ~ 2 add that up -- the kernel's own sincos is exact to a few ulp (test_wave_patm_kernel)."""
    wm = importlib.import_module(mp().__name__ + ".wave_mlp")
    patm = load_portable(wm.PATM(meta["patm_shape"][1]), meta["patm_seed"])
    with torch.no_grad():
        patm.theta_h_conv[1].weight.mul_(meta["patm_theta_scale"])
        patm.theta_w_conv[1].weight.mul_(meta["patm_theta_scale"])
    assert float(z["patm/theta_max"]) > 40.0 and float(z["patm/theta_min"]) < 0.0
    patm = patm.to(DEV).eval()
    x = torch.from_numpy(portable_input(tuple(meta["patm_shape"]), seed=meta["patm_seed"])).to(DEV)
    with torch.no_grad():
        out = patm(x).cpu().numpy()
    ref = z["patm/out"]
    m = float(np.abs(ref).max())
    assert float(np.abs(out - ref).max()) <= 1e-4 * m


def test_reference_layout_state_dict_strict(z):
    """a state_dict in the reference's layout (keys and shapes of the fixture's table) loads with strict=True and is what the forward uses"""
    shapes = {k: tuple(v) for k, v in json.loads(str(z["shapes/T"])).items()}
    sd = {k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}
    model = mp().WaveMLP("T")
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model = model.to(DEV).eval()
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = model(x)
    check(out, z["real/logits"], torch.float32, z)


def test_deterministic_and_in_flight(z, meta):
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    model = load_portable(mp().WaveMLP("T", num_classes=10), meta["tiny_seed"]).to(DEV).eval()
    xs = [torch.from_numpy(portable_input((4, 3, 64, 48), seed=90 + i)).to(DEV).bfloat16() for i in range(4)]
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


def test_train_mode_warns_inference_only(meta):
    model = load_portable(mp().WaveMLP("T", num_classes=10), meta["tiny_seed"]).to(DEV)
    model.train()
    x = torch.from_numpy(portable_input((2, 3, 64, 48), seed=1)).to(DEV)
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(x)
    assert out.grad_fn is None
