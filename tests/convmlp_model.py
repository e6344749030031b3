"""Shared by tests/test_convmlp_host.py, tests/test_gpu_convmlp.py and tests/golden/make_convmlp_golden.py (no GPU, no reference needed):
  * `wide_params`   the parameter draws of the ConvMLP fixtures, keyed by the parameter's name: every BatchNorm2d gets drawn running statistics
                    (running_var in [0.5, 2]), weight and bias, every LayerNorm a weight in [0.25, 4] and a bias in [-1, 1].  With the
                    reference's own initialisation the logits are ~0.2, and a LayerNorm bias of 0 hides the padding rule of `connect`;
  * `ln_operands`   the operands of the kernel test of mlpk_ln_dwconv3_nhwc: NaN-free data whose per-pixel means differ by several sigma, the
                    pixels' true statistics, wide gamma / beta, all as CPU tensors holding values the storage type represents;
  * `restate_ln_dwconv3`  the formula of include/mlpk.h in fp64, with the planted faults the host test holds the kernel gate against;
  * CONFIGS / SIZES / BLOCKS  the tiny configurations and block cases of tests/golden/convmlp.npz."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.portable_init import portable_input, portable_state_dict, portable_tensor

TINY_SEED, BLOCK_SEED, KERNEL_SEED = 23, 41, 59
TINY_CLASSES = 10
CONFIGS = {
    "wide": dict(depth=[1, 2, 1], d_model=[64, 96, 128], expansion_factor=[2, 2, 2], channels=64, n_conv_blocks=2),
    "narrow": dict(depth=[1, 2, 1], d_model=[48, 64, 96], expansion_factor=[2, 2, 2], channels=32, n_conv_blocks=1),
}
SIZES = [(64, 64), (40, 72), (36, 52)]
# name -> (class, constructor arguments, input shape)
BLOCKS = {
    "mlpstage_48_96": ("ConvMLPStage", [48, 96], (2, 5, 7, 48)),
    "mlpstage_64_128_1x1": ("ConvMLPStage", [64, 128], (2, 1, 1, 64)),
    "convstage_1_32_64_64": ("ConvStage", [1, 32, 64, 64], (2, 32, 6, 5)),
    "tokenizer_64": ("ConvTokenizer", [64], (2, 3, 10, 14)),
}
HEADLESS = ("narrow", (36, 52))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
# the kernel test's shapes (B, H, W, C) of mlpk_ln_dwconv3_nhwc: tests/test_gpu_convmlp.py says what each is for
LN_SHAPES = [(2, 1, 1, 8), (2, 1, 5, 8), (2, 4, 1, 40), (2, 3, 3, 8), (3, 9, 11, 40), (2, 17, 33, 96)]
FAULTS = ("beta_pad", "adjacent_image", "transposed_taps", "wrong_mean", "unrounded")


def ln_gate(eps, dtype, ref):
    """the kernel gate of mlpk_ln_dwconv3_nhwc: 4 EPS[dtype] max(1, max|ref|), `eps` the project's op gate (tests/test_gpu_ops.py EPS)"""
    return 4.0 * eps[dtype] * max(1.0, float(ref.abs().max()))


def load_portable(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = portable_state_dict(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def wide_params(model, seed):
    def draw(t, name, lo, hi):
        t.copy_(torch.from_numpy(portable_tensor(name, tuple(t.shape), lo, hi, seed=seed)))
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.LayerNorm):
                draw(m.weight, name + ".weight", 0.25, 4.0)
                draw(m.bias, name + ".bias", -1.0, 1.0)
            elif isinstance(m, torch.nn.BatchNorm2d):
                draw(m.running_mean, name + ".running_mean", -0.5, 0.5)
                draw(m.running_var, name + ".running_var", 0.5, 2.0)
                draw(m.weight, name + ".weight", 0.5, 1.5)
                draw(m.bias, name + ".bias", -0.5, 0.5)
    return model


def prepare(model, seed):
    """the fixtures' parameters: portable_state_dict (which draws the convolutions' biases too), then wide_params"""
    return wide_params(load_portable(model, seed), seed).eval()


def storage(t, dtype):
    return t.to(dtype).to(torch.float64)


def ln_operands(B, H, W, C, dtype, seed=KERNEL_SEED):
    """x (B, H, W, C), mean / rstd (B, H, W), gamma / beta (C), w (9, C): float64 tensors holding storage-type (x) and float32 (the rest) values"""
    tag = "lnk%dx%dx%dx%d" % (B, H, W, C)
    noise = torch.from_numpy(portable_input((B, H, W, C), seed=seed, name=tag + ".x")).double()
    centre = torch.from_numpy(portable_tensor(tag + ".centre", (B, H, W, 1), -4.0, 4.0, seed=seed)).double()
    spread = torch.from_numpy(portable_tensor(tag + ".spread", (B, H, W, 1), 0.5, 1.5, seed=seed)).double()
    x = storage(centre + spread * noise, dtype)
    mean = x.mean(-1).float().double()
    rstd = (1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)).float().double()
    # gamma in +-[0.25, 2] and beta in +-[2, 4]: a bias that is never small beside the normalised values, so that padding with beta instead of 0
    # moves a border pixel by a visible share of max|out| (the kernel gate is relative to max|out|, and 4 EPS[bf16] is 3 % of it)
    sign = lambda n: torch.from_numpy(portable_tensor(tag + n, (C,), -1.0, 1.0, seed=seed)).double().sign()
    gamma = torch.from_numpy(portable_tensor(tag + ".gamma", (C,), 0.25, 2.0, seed=seed)).double() * sign(".gsign")
    beta = torch.from_numpy(portable_tensor(tag + ".beta", (C,), 2.0, 4.0, seed=seed)).double() * sign(".bsign")
    w = torch.from_numpy(portable_tensor(tag + ".w", (9, C), -1.0, 1.0, seed=seed)).double()
    return x, mean, rstd, gamma, beta, w


def restate_ln_dwconv3(x, mean, rstd, gamma, beta, w, dtype, fault=None):
    """out[b,y,x,c] = sum_{i,j<3} w[3i+j, c] v[b, y+i-1, x+j-1, c], v = round_to_storage((x - mean) rstd gamma + beta) inside the map and 0 outside
    it, in fp64 (include/mlpk.h, mlpk_ln_dwconv3_nhwc).  mean / rstd / gamma / beta None: 0 / 1 / 1 / 0.  `fault`: one of FAULTS."""
    assert fault is None or fault in FAULTS
    x = x.double()
    B, H, W, C = x.shape
    mu = mean.double() if mean is not None else torch.zeros(B, H, W, dtype=torch.float64)
    rs = rstd.double() if rstd is not None else torch.ones(B, H, W, dtype=torch.float64)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    bt = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    if fault == "wrong_mean":                                          # the statistics of the pixel to the right (the last one: of the first)
        mu = mu.reshape(-1).roll(-1).reshape(B, H, W)
    v = (x - mu[..., None]) * rs[..., None] * g + bt
    if fault != "unrounded":
        v = storage(v, dtype)
    w = w.double().reshape(3, 3, C)
    if fault == "transposed_taps":
        w = w.transpose(0, 1)
    if fault == "adjacent_image":                                      # the batch as one tall image: row -1 of image b is the last row of b - 1
        v = v.reshape(1, B * H, W, C)
    Bv, Hv = v.shape[0], v.shape[1]
    vp = torch.zeros(Bv, Hv + 2, W + 2, C, dtype=torch.float64)
    if fault == "beta_pad":
        vp += bt
    vp[:, 1:-1, 1:-1] = v
    out = torch.zeros(Bv, Hv, W, C, dtype=torch.float64)
    for i in range(3):
        for j in range(3):
            out += w[i, j] * vp[:, i:i + Hv, j:j + W]
    return out.reshape(B, H, W, C)


def torch_connect(x, gamma, beta, w, eps=1e-5):
    """connect(connect_norm(x)) of conv_mlp.py:168 by torch's own layer_norm and conv2d, in x's type; w (9, C) tap-major"""
    C = x.shape[-1]
    v = F.layer_norm(x, (C,), gamma, beta, eps)
    return F.conv2d(v.permute(0, 3, 1, 2), w.t().reshape(C, 1, 3, 3).contiguous(), None, 1, 1, 1, C).permute(0, 2, 3, 1)


def beta_padded_connect(stage):
    """replace `stage.connect` of a ConvMLPStage by the planted fault of the golden file's condition: the map padded with the LayerNorm's bias
    instead of 0 (what a kernel does that normalises its zero padding)"""
    conv, bias = stage.connect, stage.connect_norm.bias

    class Padded(torch.nn.Module):
        def forward(self, v):
            B, C, H, W = v.shape
            vp = bias.detach().to(v.dtype).view(1, C, 1, 1).expand(B, C, H + 2, W + 2).clone()
            vp[:, :, 1:-1, 1:-1] = v
            return F.conv2d(vp, conv.weight, None, 1, 0, 1, C)
    stage.connect = Padded()
    return stage


def case_input(shape, seed):
    return torch.from_numpy(portable_input(tuple(shape), seed=seed))


def golden_keys():
    """every case of tests/golden/convmlp.npz: key -> kind"""
    keys = {}
    for cfg in CONFIGS:
        for h, w in SIZES:
            keys["tiny/%s/%dx%d" % (cfg, h, w)] = "logits"
    for name in BLOCKS:
        keys["block/" + name] = "out"
    keys["real/S"] = "logits"
    keys["headless/%s/%dx%d" % (HEADLESS[0], HEADLESS[1][0], HEADLESS[1][1])] = "out"
    return keys


def np_json(d):
    import json
    return np.array(json.dumps(d))
