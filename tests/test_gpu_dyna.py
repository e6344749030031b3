"""-m gpu: DynaMixer on the MI355X.
  * mlpk_dyna_mix (form "fused") and the unfused form -- mlpk_dyna_gather, the logits, mlpk_dyna_mix_logits: form "unfused" with torch's Linear
    for the logits, form "engine" = engine.dyna_mix_unfused with the library's GEMM, the model's sequence for 16-bit lines of 8 to 32 -- alone, behind guard bands (tests/guard.py), both axes, three dtypes, tight and padded pitches, B = 3 (every line and item count
    below is odd against the kernel's eight items per workgroup somewhere in SHAPES):
      index contract, as equalities -- attend weight and bias 0 or -200 make the softmax exactly one-hot (exp(-200) is 0 in fp32), so the output
      must hold the bits of mlpk_norm_apply's output permuted along the line: (a) the permutation in the bias, (b) one permutation per weight
      column, selected by a single 1.0 in t per (b, line, segment); (c) all zeros and a power-of-two L give the exact line mean of small integers;
      stability -- logits spread over +-200;
      numeric -- random operands at the fixture's logit scale against a float64 restatement of the STORED operands.  fp32 gate: 16 x the error of a
      torch fp32 restatement on the same device + half an ulp of the output (summation order and the exponential differ between two fp32
      evaluations of sums of at most 256 terms); 16-bit gate: 2 x the error of the torch restatement run in that type, as the reference runs it
      (the margin of tests/test_gpu_wave.py).  Every gate must be at most a tenth of the distance to the same restatement with uniform attention.
      The measured ratios are in profiles/dyna_kernel_errors.txt.
  * the model against tests/golden/dyna_mlp.npz (the reference's own forwards, tests/golden/make_dyna_golden.py): fp32 1e-5 max|ref|; 16-bit twice the
    reference's own 16-bit distance from its fp32 logits relative to max |logit|, scaled by max |ref| of the case at hand (tests/test_gpu_raft.py).
  * the lifecycle properties of tests/test_gpu_lifecycle.py on a Config registered in test_lifecycle_host._CACHE."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_pkg
from exact import INT_RANGE
from guard import INT_VIEW, Guarded, assert_bits_equal, assert_finite
from oracle.portable_init import portable_input, portable_state_dict, portable_tensor
import test_lifecycle_host as LH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "dyna_mlp.npz")
DM = load_pkg().models_pytorch.dyna_mlp
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
SHAPES = [(1, 1, 8, 1, 2), (3, 5, 16, 2, 2), (5, 3, 24, 3, 2), (10, 10, 16, 2, 2), (6, 10, 16, 2, 8), (16, 16, 48, 2, 2), (32, 32, 64, 2, 2),
          (32, 4, 256, 8, 8), (16, 2, 512, 16, 8)]
B = 3
NAME = "dynamixer"


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def engine():
    return load_pkg().engine


# ------------------------------------------------------------------ the kernel alone
def rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def cases(shapes=SHAPES):
    return [pytest.param(H, W, C, s, hd, dtype, id="%dx%dx%d-s%d-hd%d-%s" % (H, W, C, s, hd, name))
            for H, W, C, s, hd in shapes for dtype, name in zip(DTYPES, IDS)]


CASES = pytest.mark.parametrize("H,W,C,s,hd,dtype", cases())
PADS = pytest.mark.parametrize("pad", [0, 1], ids=["tight", "padded"])
AXES = pytest.mark.parametrize("axis", [0, 1], ids=["h", "w"])


def field(H, W, C, dtype, seed):
    """x (rows, C) in the storage type and the LayerNorm operands on the device"""
    rows = B * H * W
    x = rand((rows, C), seed, -2.0, 2.0).to(dtype)
    mean, rstd = rand((rows,), seed + 1).to(DEV), rand((rows,), seed + 2, 0.5, 2.0).to(DEV)
    gamma, beta = rand((C,), seed + 3, 0.25, 4.0).to(DEV), rand((C,), seed + 4).to(DEV)
    return x, (mean, rstd, gamma, beta)


FORMS = pytest.mark.parametrize("form", ["fused", "unfused"])


def unfused_mix(E, gx, ln4, gt, t, aw, ab, out, H, W, C, s, hd, dtype, pad, axis, form):
    """the unfused form behind guard bands: mlpk_dyna_gather (its rows must be t's bits in item order, zeros in the K padding), the logits, then
    mlpk_dyna_mix_logits.  form "unfused": the logits by torch's Linear in the storage type (the two new entries alone, at every shape);
    form "engine": engine.dyna_mix_unfused, the model's own sequence with the library's GEMM."""
    L, Q = (W, H) if axis == 1 else (H, W)
    K, nn, items, nt = L * hd, L * L, B * Q * s, s * hd
    mean, rstd, gamma, beta = ln4
    if form == "engine":
        ws = E.Workspace(torch.device(DEV), dtype)
        E.dyna_mix_unfused(ws, "u", gx.view, mean, rstd, gamma, beta, gt.view, axis * nt, E.pack_matrix(aw, dtype, torch.device(DEV)), E.f32(ab, torch.device(DEV)),
                           out, B, H, W, C, s, hd, axis)
        return
    kp = (K + 7) // 8 * 8
    gv = Guarded(items, kp + 2, kp + 9 if pad else kp + 2, dtype, DEV, role="out")
    E.dyna_gather(gt.view, axis * nt, gv.view, kp, B, H, W, s, hd, axis)
    torch.cuda.synchronize()
    gv.check()
    gv.still_poison(kp, kp + 2)
    want = lines(t.to(dtype), H, W, axis, hd).reshape(items, K).contiguous()
    assert_bits_equal(gv.view[:, :K].cpu().contiguous(), want, "the gathered operand rows")
    assert bool((gv.view[:, K:kp].cpu().view(INT_VIEW[dtype]) == 0).all()), "the K padding of the gathered rows is not +0"
    z = F.linear(gv.view[:, :K].contiguous(), aw.to(DEV).to(dtype), ab.to(DEV).to(dtype))
    gz = Guarded(items, nn, nn + 3 if pad else nn, dtype, DEV, role="in", data=z)
    E.dyna_mix_logits(gx.view, mean, rstd, gamma, beta, gz.view, out, B, H, W, C, s, hd, axis)
    torch.cuda.synchronize()
    gz.check()


def run_mix(x, ln, t, aw, ab, H, W, C, s, hd, dtype, pad, axis, form="fused"):
    """t (rows, s hd): this axis's columns; aw (L L, L hd), ab (L L) on the CPU.  -> (xn = mlpk_norm_apply's stored output (rows, C) on the CPU or
    x itself when ln is None, the dense result on the CPU).  Guard bands checked: t sits at column offset axis * s hd of a (rows, 2 s hd)
    buffer whose other half is NaN, the output is column block `axis` of a (rows, 2C + 8) buffer whose other columns must stay untouched."""
    E = engine()
    rows, nt = B * H * W, s * hd
    mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
    gx = Guarded(rows, C, C + 8 if pad else C, dtype, DEV, role="in", data=x)
    both = torch.full((rows, 2 * nt), float("nan"))
    both[:, axis * nt:(axis + 1) * nt] = t.float()
    gt = Guarded(rows, 2 * nt, 2 * nt + 3 if pad else 2 * nt, dtype, DEV, role="in", data=both)
    go = Guarded(rows, 2 * C + 8, 2 * C + 16 if pad else 2 * C + 8, dtype, DEV, role="out")
    out = go.view[:, axis * C:(axis + 1) * C]
    if form == "fused":
        pw, pb = E.pack_dyna_attend(aw, ab, dtype, torch.device(DEV))
        E.dyna_mix(gx.view, mean, rstd, gamma, beta, gt.view, axis * nt, pw, pb, out, B, H, W, C, s, hd, axis)
    else:
        unfused_mix(E, gx, (mean, rstd, gamma, beta), gt, t, aw, ab, out, H, W, C, s, hd, dtype, pad, axis, form)
    torch.cuda.synchronize()
    gx.check()
    gt.check()
    go.check()
    go.still_poison(0, axis * C)
    go.still_poison((axis + 1) * C, 2 * C + 8)
    if ln is not None:
        ref = torch.empty((rows, C), dtype=dtype, device=DEV)
        E.norm_apply(gx.view, rows, C, gx.ld, mean=mean, rstd=rstd, gamma=gamma, beta=beta, out_rm=ref, ld_rm=C)
        torch.cuda.synchronize()
        xn = ref.cpu()
    else:
        xn = x.clone()
    return xn, out.clone().contiguous().cpu()


def lines(v, H, W, axis, inner):
    """(rows, s * inner) -> (B, Q, s, L, inner): the reference's Rearrange 'b h w (s d) -> b h s w d' (axis 1) / '-> b w s h d' (axis 0)"""
    v5 = v.reshape(B, H, W, -1, inner)
    return v5.permute(0, 1, 3, 2, 4) if axis == 1 else v5.permute(0, 2, 3, 1, 4)


def unlines(o, H, W, axis):
    """(B, Q, s, L, d) -> (rows, C)"""
    o = o.permute(0, 1, 3, 2, 4) if axis == 1 else o.permute(0, 3, 1, 2, 4)
    return o.reshape(B * H * W, -1)


def restate(xn, t, aw, ab, H, W, s, hd, axis, dtype, uniform=False):
    """DynaMixerOp's forward between Wd and proc (dyna_mlp.py:58-62 / :89-93) on the given operands in `dtype`, on their device"""
    L = W if axis == 1 else H
    xl = lines(xn.to(dtype), H, W, axis, xn.shape[1] // s)
    tl = lines(t.to(dtype), H, W, axis, hd)
    zl = F.linear(tl.reshape(B, -1, s, L * hd), aw.to(dtype), ab.to(dtype)).reshape(B, -1, s, L, L)
    p = torch.full_like(zl, 1.0 / L) if uniform else torch.softmax(zl, -1)
    return unlines(torch.matmul(p, xl), H, W, axis)


def name_bad(bad, H, W, C, s, axis):
    r, c = torch.nonzero(bad)[0].tolist()
    b, y, x_ = r // (H * W), r // W % H, r % W
    line, l1 = (y, x_) if axis == 1 else (x_, y)
    return "(b %d, line %d, segment %d, l1 %d, c %d)" % (b, line, c // (C // s), l1, c % (C // s))


def permuted(xn, perm, H, W, C, s, axis):
    """xn (rows, C) with out[l1] = xn[perm[..., l1]] along the line; perm (L,) or (B, Q, s, L)"""
    L = W if axis == 1 else H
    xl = lines(xn, H, W, axis, C // s)                                  # (B, Q, s, L, d)
    idx = perm.reshape((1, 1, 1, L) if perm.dim() == 1 else perm.shape).expand(xl.shape[:4])
    return unlines(torch.gather(xl, 3, idx.unsqueeze(-1).expand(xl.shape)), H, W, axis).contiguous()


def one_hot_logits(perm, L):
    """(L,) permutation -> (L L) logits: 0 at [l1 L + perm[l1]], -200 elsewhere"""
    zl = torch.full((L, L), -200.0)
    zl[torch.arange(L), perm] = 0.0
    return zl.reshape(-1)


@CASES
@PADS
@AXES
@FORMS
def test_bias_permutation_moves_norm_apply_bits(H, W, C, s, hd, dtype, pad, axis, form):
    """(a) weight 0, the bias one-hot at l2 = perm[l1]"""
    L = W if axis == 1 else H
    seed = H * 1000 + W * 100 + C + s + hd + axis
    x, ln = field(H, W, C, dtype, seed)
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(seed + 9))
    t = rand((B * H * W, s * hd), seed + 5, -4.0, 4.0).to(dtype)        # (any t: the weight is zero)
    xn, out = run_mix(x, ln, t, torch.zeros(L * L, L * hd), one_hot_logits(perm, L), H, W, C, s, hd, dtype, pad, axis, form)
    want = permuted(xn, perm, H, W, C, s, axis)
    bad = out.view(INT_VIEW[dtype]) != want.view(INT_VIEW[dtype])
    assert not bool(bad.any()), "%s is not norm_apply's element at l2 = perm[l1] (%d elements differ)" % (name_bad(bad, H, W, C, s, axis), int(bad.sum()))


@CASES
@PADS
@AXES
@FORMS
def test_weight_column_permutations_pin_t_and_the_items(H, W, C, s, hd, dtype, pad, axis, form):
    """(b) bias 0, weight column k one-hot for its own permutation; t holds a single 1.0 per (b, line, segment) at a position that varies"""
    L, Q = (W, H) if axis == 1 else (H, W)
    K = L * hd
    seed = H * 1000 + W * 100 + C + s + hd + axis + 40
    g = torch.Generator().manual_seed(seed + 9)
    x, ln = field(H, W, C, dtype, seed)
    perms = torch.stack([torch.randperm(L, generator=g) for _ in range(K)])              # (K, L)
    aw = torch.stack([one_hot_logits(perms[k], L) for k in range(K)], 1)                   # (L L, K)
    kstar = ((torch.arange(B * Q * s) * 5 + seed) % K).reshape(B, Q, s)                   # varies from item to item
    tl = torch.zeros(B, Q, s, K)
    tl.scatter_(3, kstar.unsqueeze(-1), 1.0)
    t = unlines(tl.reshape(B, Q, s, L, hd), H, W, axis).contiguous().to(dtype)            # v[l hd + j] = t[pix(l), g hd + j]
    xn, out = run_mix(x, ln, t, aw, torch.zeros(L * L), H, W, C, s, hd, dtype, pad, axis, form)
    want = permuted(xn, perms[kstar], H, W, C, s, axis)
    bad = out.view(INT_VIEW[dtype]) != want.view(INT_VIEW[dtype])
    assert not bool(bad.any()), "%s is not the element the weight column of its item's t selects (%d elements differ)" % (
        name_bad(bad, H, W, C, s, axis), int(bad.sum()))


POW2 = [pytest.param(H, W, C, s, hd, dtype, axis, id="%dx%dx%d-s%d-hd%d-%s-%s" % (H, W, C, s, hd, name, "hw"[axis]))
        for H, W, C, s, hd in SHAPES for dtype, name in zip(DTYPES, IDS) for axis in (0, 1) if ((H, W)[axis] & ((H, W)[axis] - 1)) == 0]


@pytest.mark.parametrize("H,W,C,s,hd,dtype,axis", POW2)
@PADS
@FORMS
def test_zero_logits_give_the_exact_line_mean(H, W, C, s, hd, dtype, axis, pad, form):
    """(c) weight and bias 0, L a power of two, small integers, no LayerNorm: every p is exactly 1 / L and the sums are exact"""
    L = W if axis == 1 else H
    seed = H * 1000 + W * 100 + C + s + hd + axis + 80
    lim = min(INT_RANGE[dtype] // L, 64)
    x = torch.randint(-lim, lim + 1, (B * H * W, C), generator=torch.Generator().manual_seed(seed)).float().to(dtype)
    t = rand((B * H * W, s * hd), seed + 5, -4.0, 4.0).to(dtype)
    xn, out = run_mix(x, None, t, torch.zeros(L * L, L * hd), torch.zeros(L * L), H, W, C, s, hd, dtype, pad, axis, form)
    xl = lines(xn.double(), H, W, axis, C // s)
    mean = xl.mean(3, keepdim=True).expand(xl.shape)
    want = unlines(mean, H, W, axis)
    assert torch.equal(want.to(dtype).double(), want), "the test's own means are not exact in the storage type"
    bad = out.double() != want
    assert not bool(bad.any()), "%s is not the exact line mean (%d elements differ)" % (name_bad(bad, H, W, C, s, axis), int(bad.sum()))


def operands(H, W, C, s, hd, dtype, axis, seed, scale):
    """random operands at the fixture's logit scale: attend drawn like a Linear (U(+-1 / sqrt K)) times `scale`; everything in its stored form"""
    L = W if axis == 1 else H
    K = L * hd
    x, ln = field(H, W, C, dtype, seed)
    t = rand((B * H * W, s * hd), seed + 5, -1.0, 1.0).to(dtype)
    bound = K ** -0.5
    aw = (rand((L * L, K), seed + 6, -bound, bound) * scale).to(dtype).float()
    ab = rand((L * L,), seed + 7, -bound, bound) * scale
    return x, ln, t, aw, ab


def numeric(H, W, C, s, hd, dtype, pad, axis, scale, what, form="fused"):
    seed = H * 1000 + W * 100 + C + s + hd + axis + (120 if scale == 8.0 else 160)
    x, ln, t, aw, ab = operands(H, W, C, s, hd, dtype, axis, seed, scale)
    xn, out = run_mix(x, ln, t, aw, ab, H, W, C, s, hd, dtype, pad, axis, form)
    assert_finite(out, "out")
    dev = [v.to(DEV) for v in (xn, t, aw, ab)]
    exact = restate(*dev, H, W, s, hd, axis, torch.float64)
    same = restate(*dev, H, W, s, hd, axis, dtype).double()
    flat = restate(*dev, H, W, s, hd, axis, torch.float64, uniform=True)
    ref_err = float((same - exact).abs().max())
    m = float(exact.abs().max())
    gate = 16.0 * ref_err + 2.0 ** -24 * m if dtype == torch.float32 else 2.0 * ref_err
    err = float((out.to(DEV).double() - exact).abs().max())
    far = float((flat - exact).abs().max())
    print("%s %s %dx%dx%d s%d hd%d axis %d %s %s: |d| %.3e gate %.3e ratio %.3f (torch in type %.3e, uniform attention %.3e away, max|exact| %.3f)" % (
        what, form, H, W, C, s, hd, axis, IDS[DTYPES.index(dtype)], "padded" if pad else "tight", err, gate, err / gate if gate else 0.0, ref_err, far, m))
    return err, gate, far


@CASES
@PADS
@AXES
@pytest.mark.parametrize("form", ["fused", "unfused", "engine"])
def test_random_operands_against_fp64(H, W, C, s, hd, dtype, pad, axis, form):
    if form == "engine" and not engine().dyna_unfused_preferred(dtype, (H, W)[axis]):
        form = "fused"                                                 # (where the model takes the fused kernel, that IS its sequence)
    err, gate, far = numeric(H, W, C, s, hd, dtype, pad, axis, 8.0, "numeric", form)
    L = W if axis == 1 else H
    if L > 1:                                                          # (a line of one position has one attention: uniform IS the answer)
        assert gate <= 0.1 * far, "the gate %.3e could not tell a kernel that ignores the logits (uniform attention is %.3e away)" % (gate, far)
    assert err <= gate, (err, gate)


@CASES
@AXES
@FORMS
def test_logits_spread_over_200_stay_finite(H, W, C, s, hd, dtype, axis, form):
    """stability: the same with the attend weight and bias scaled until the logits cover +-200 (exp overflows without the row maximum).  The padded
    pitch only; `numeric` asserts that the output is finite (assert_finite); softmax rows this sharp are not compared with uniform attention."""
    err, gate, far = numeric(H, W, C, s, hd, dtype, 1, axis, 200.0, "stability", form)                  # (logits of standard deviation 200 / 3)
    assert err <= gate, (err, gate)


# ------------------------------------------------------------------ the model against the reference
def sharpen(model, meta):
    """tests/golden/make_dyna_golden.py `sharpen`: every attend.1 weight and bias times meta["scale"]"""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if meta["sharpen"] in "." + name:
                p.mul_(meta["scale"])


def wide_affine(model, meta, seed):
    lo_w, hi_w = meta["affine"]["weight"]
    lo_b, hi_b = meta["affine"]["bias"]
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.from_numpy(portable_tensor(name + ".weight", tuple(m.weight.shape), lo_w, hi_w, seed=seed)))
                m.bias.copy_(torch.from_numpy(portable_tensor(name + ".bias", tuple(m.bias.shape), lo_b, hi_b, seed=seed)))


def load_portable(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = portable_state_dict(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def add_tiny_settings(meta):
    """the tiny entries go into the module-level table exactly as the fixture generator puts them into the reference's"""
    DM.dynamlp_settings.update({k: v for k, v in meta["tiny"].items()})


def tiny_model(meta, cfg, size):
    add_tiny_settings(meta)
    model = load_portable(DM.DynaMixer(cfg, image_size=tuple(size), num_classes=meta["tiny_classes"]), meta["tiny_seed"])
    sharpen(model, meta)
    x = torch.from_numpy(portable_input((2, 3, size[0], size[1]), seed=meta["tiny_seed"])).to(DEV)
    return model.to(DEV).eval(), x


def lowp_gate(z, dtype, m, name="T"):
    tag = "fp16" if dtype == torch.float16 else "bf16"
    rel = float(z["real/%s/err_%s" % (name, tag)]) / float(np.abs(z["real/%s/logits" % name]).max())
    return 2.0 * rel * m


def check(out, ref, dtype, z, name="T"):
    m = float(np.abs(ref).max())
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    gate_ = 1e-5 * m if dtype == torch.float32 else lowp_gate(z, dtype, m, name)
    print("%s: max|d| %.3e gate %.3e max|ref| %.3f" % (dtype, err, gate_, m))
    assert err <= gate_, (str(dtype), err, gate_, m)


TINY_CASES = [(c, s) for c in ("tiny", "tiny8") for s in ((40, 40), (24, 40), (8, 24))]


@pytest.mark.parametrize("cfg,size", TINY_CASES, ids=["%s-%dx%d" % (c, s[0], s[1]) for c, s in TINY_CASES])
def test_tiny_logits_fp32(cfg, size, z, meta):
    model, x = tiny_model(meta, cfg, size)
    with torch.no_grad():
        out = model(x)
    ref = z["tiny/%s/%dx%d" % (cfg, size[0], size[1])]
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
    check(out, ref, torch.float32, z)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cfg,size", [("tiny", (40, 40)), ("tiny8", (24, 40))], ids=["tiny-40x40", "tiny8-24x40"])
def test_tiny_logits_16bit(cfg, size, dtype, z, meta):
    model, x = tiny_model(meta, cfg, size)
    with torch.no_grad():
        out = model(x.to(dtype))
    assert out.dtype == dtype
    check(out, z["tiny/%s/%dx%d" % (cfg, size[0], size[1])], dtype, z)


def test_tiny_compute_dtype(z, meta):
    """set_compute_dtype: fp32 input, bf16 kernels, fp32 logits"""
    model, x = tiny_model(meta, "tiny", (40, 40))
    model.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32
    check(out, z["tiny/tiny/40x40"], torch.bfloat16, z)


def test_blocks_alone_fp32(z, meta):
    for name, (cls, args, shape) in meta["blocks"].items():
        seed = meta["block_seed"]
        blk = load_portable(getattr(DM, cls)(*args), seed)
        sharpen(blk, meta)
        wide_affine(blk, meta, seed)
        blk = blk.to(DEV).eval()
        x = torch.from_numpy(portable_input(tuple(shape), seed=seed)).to(DEV)
        with torch.no_grad():
            out = blk(x)
        ref = z["block/" + name]
        assert tuple(out.shape) == ref.shape and out.dtype == torch.float32, name
        m = float(np.abs(ref).max())
        err = float(np.abs(out.cpu().numpy() - ref).max())
        print("%s: max|d| %.3e gate %.3e" % (name, err, 1e-5 * m))
        assert err <= 1e-5 * m, (name, err, m)


@pytest.fixture(scope="module", params=["T", "M", "L"])
def real_model(request, z, meta):
    """a state_dict in the reference's layout (keys and shapes of the fixture's table), loaded with strict=True"""
    name = request.param
    shapes = {k: tuple(v) for k, v in json.loads(str(z["shapes/" + name])).items()}
    sd = {k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}
    model = DM.DynaMixer(name)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    sharpen(model, meta)
    return name, model.to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_logits(real_model, dtype, z):
    name, model = real_model
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = model(x.to(dtype))
    check(out, z["real/%s/logits" % name], dtype, z, name)


def test_unsupported_shape_raises_and_names_it(meta):
    """a stage whose lines are longer than 32 positions: NotImplementedError that names the shape, nothing launched, no fallback"""
    add_tiny_settings(meta)
    model = DM.DynaMixer("tiny", image_size=(40, 160), num_classes=3).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="10 x 40 map of 16 channels"):
        model(torch.zeros(1, 3, 40, 160, device=DEV))
    with pytest.raises(NotImplementedError, match="mlpk_dyna_mix"):
        DM.DynaMixerOp_w(40, 16, 2, 2).to(DEV)(torch.zeros(1, 2, 40, 16, device=DEV))


# ------------------------------------------------------------------ lifecycle (tests/test_gpu_lifecycle.py's helpers on a registered Config)
def dyna_config():
    """the tiny configuration at 40 x 40 with sharpened attends, registered where tests/test_gpu_lifecycle.py's helpers look rows up"""
    if NAME not in LH._CACHE:
        meta = json.loads(str(np.load(FIX)["meta"]))
        add_tiny_settings(meta)
        ctor, kw = functools.partial(DM.DynaMixer, "tiny"), {"image_size": tuple(meta["tiny_sizes"][0]), "num_classes": meta["tiny_classes"]}
        model = load_portable(ctor(**kw), meta["tiny_seed"])
        sharpen(model, meta)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        LH._CACHE[NAME] = LH.Config(NAME, ctor, kw, sd, tuple(meta["tiny_sizes"][0]), meta["tiny_classes"])
    return LH._CACHE[NAME]


def lifecycle():
    dyna_config()
    return importlib.import_module("test_gpu_lifecycle")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_weight_update_reaches_the_next_forward(dtype):
    """test_gpu_lifecycle.check_updates for an inference-only family (that helper branches on EVAL_ONLY): the visible update forms that need
    no backward, and set_compute_dtype back and forth with an update in between"""
    GL = lifecycle()
    cfg, dt = dyna_config(), GL.DT[dtype]
    x = GL.images(cfg, 2, dt)
    for upd in LH.VISIBLE_UPDATES + [LH.u_data_inplace_then_invalidate]:
        warm = GL.warm_model(cfg)
        before = GL.run(warm, x).clone()
        upd(warm, GL.gen())
        after = GL.run(warm, x)
        assert torch.equal(after, GL.run(GL.cold_model(cfg, warm), x)), (upd.__name__, "the warm model did not run on its updated state")
        assert not torch.equal(after, before), (upd.__name__, "the update was a no-op: the case checks nothing")
    warm = GL.warm_model(cfg)
    xf = GL.images(cfg, 2, torch.float32)
    a1 = GL.run(warm, xf).clone()
    b1 = GL.run(warm.set_compute_dtype(torch.bfloat16), xf).clone()
    assert torch.equal(GL.run(warm.set_compute_dtype(None), xf), a1) and torch.equal(GL.run(warm.set_compute_dtype(torch.bfloat16), xf), b1)
    assert b1.dtype == torch.float32 and not torch.equal(a1, b1)
    LH.u_no_grad_add(warm, GL.gen())
    assert torch.equal(GL.run(warm, xf), GL.run(GL.cold_model(cfg, warm), xf)), "bf16 compute after an update"
    warm.set_compute_dtype(None)
    assert torch.equal(GL.run(warm, xf), GL.run(GL.cold_model(cfg, warm), xf)), "the fp32 pack made before the update was reused"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_parameter_role_reaches_the_next_forward(dtype):
    """one entry per role at a time; attend.1 and Wd.* are the re-laid and concatenated ones, proj_c / proj_o / proc the folded ones"""
    GL = lifecycle()
    roles = LH.one_per_role(dyna_config().fresh())
    assert any("attend..weight" in r for r in roles) and any("Wd..bias" in r for r in roles) and any("proj_o" in r for r in roles)
    GL.test_every_parameter_role_reaches_the_next_forward(NAME, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_forward_leaves_nothing_behind(dtype):
    GL = lifecycle()
    GL.check_nothing_left_behind(NAME, GL.DT[dtype])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_images_of_a_batch_do_not_see_each_other(dtype):
    GL = lifecycle()
    GL.check_rows_do_not_see_each_other(NAME, GL.DT[dtype])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_results_and_inputs_are_the_callers(dtype, meta):
    GL = lifecycle()
    cfg = dyna_config()
    m = GL.warm_model(cfg)
    assert GL.check_callers_own(m, m, GL.images(cfg, 3, GL.DT[dtype], seed=6)) >= 1
    mb = m.stages[0][1]
    for mod, shape in ((mb, (3, 16, 10, 10)), (mb.layers[0][0].fn, (3, 10, 10, 16)), (mb.layers[0][0].fn.DynaMixerOp_h, (3, 10, 10, 16)),
                       (mb.layers[0][0].fn.DynaMixerOp_w, (3, 10, 10, 16))):
        x = torch.from_numpy(portable_input(shape, seed=8)).to(DEV).to(GL.DT[dtype])
        assert GL.check_callers_own(m, mod, x) >= 2


def test_deterministic_and_in_flight():
    """two forwards give the same bits, and so do two in flight: the batches alternate over two streams of the caller's own, each behind the
    stream that made its input, nothing synchronised in between.  (High-priority streams: torch hands them out of a pool of their own, so this
    file leaves the pool the schedules of tests/test_gpu_streams.py draw from as it found it.)"""
    GL = lifecycle()
    cfg = dyna_config()
    model = GL.warm_model(cfg)
    xs = [GL.images(cfg, 4, torch.bfloat16, seed=90 + i) for i in range(4)]
    with torch.no_grad():
        serial = [model(x).clone() for x in xs]
        again = [model(x).clone() for x in xs]
        for a, b in zip(serial, again):
            assert torch.equal(a, b)
        cur = torch.cuda.current_stream()
        streams = [torch.cuda.Stream(DEV, priority=-1) for _ in range(2)]
        pending = []
        for i, x in enumerate(xs):
            st = streams[i % 2]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                out = model(x)
            out.record_stream(cur)
            x.record_stream(st)
            pending.append(out)
        for st in streams:
            cur.wait_stream(st)
    torch.cuda.synchronize()
    for out, want in zip(pending, serial):
        assert torch.equal(out, want)
    assert len(model._spaces) >= 3                                     # the serial stream's workspace and one per stream in flight


def test_deepcopy_and_pickle_of_a_warm_model():
    GL = lifecycle()
    GL.test_deepcopy_and_pickle_of_a_warm_model(NAME, "bf16")


def test_train_mode_warns_inference_only():
    GL = lifecycle()
    cfg = dyna_config()
    model = GL.warm_model(cfg)
    model.train()
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(GL.images(cfg, 2, torch.float32))
    assert out.grad_fn is None
