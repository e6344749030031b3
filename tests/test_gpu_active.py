"""-m gpu: ActiveMLP on the MI355X.
  * mlpk_atm_sample alone, behind guard bands (tests/guard.py), three dtypes, tight and padded pitches: (a) integer offsets -- out_w / out_h are
    mlpk_norm_apply's output shifted with torch indexing, bit for bit, and out_c is that output; (b) real offsets against an fp64 restatement of
    torchvision's rule applied to norm_apply's STORED output and the stored offsets; (c) NaN, +-inf, +-1e30, denormals, signed zeros and the exact
    boundaries p = -1, L - 1, L sprinkled into a random field (tests/test_active_host.py proves the tap function on the same values on the CPU
    first); (d) NULL outputs and outputs as column slices of one buffer.
    Gate of (b), fp32: |d| <= 2^-17 (|v0| + |v1|) -- the position fl(x + off) is off by at most half an fp32 ulp below 64, 2^-19, which moves the
    sample by that times |v1 - v0|; the factor 4 covers the three fp32 operations of the sum.  16-bit: that plus half a unit in the last place of
    the storage type at the magnitude of the exact result.  The rule is continuous in p (also at -1, at L and at integers), so a position that
    rounds across one of them moves the sample by no more than that.
  * the whole model against tests/golden/active_mlp.npz (the reference's own forwards, tests/golden/make_active_golden.py): gates as
    tests/test_gpu_raft.py derives them -- fp32 1e-5 max|ref|; 16-bit twice the reference's own 16-bit distance from its fp32 logits (sampling in fp32,
    relative to max |logit|), scaled by max |ref| of the case at hand."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
from guard import INT_VIEW, Guarded, assert_bits_equal, assert_finite
from oracle.portable_init import portable_input, portable_state_dict, portable_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "active_mlp.npz")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
SHAPES = [(1, 1, 8, 1), (1, 5, 8, 2), (5, 1, 8, 8), (3, 4, 40, 4), (7, 9, 24, 2), (14, 14, 320, 4), (56, 56, 64, 2), (3, 4, 12, 4)]
B = 2
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}       # explicit mantissa bits, smallest normal exponent


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


# ------------------------------------------------------------------ the kernel alone
def rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def skip_shape(C, dtype):
    return C % 8 != 0 and dtype != torch.float32                # (3, 4, 12, 4): whole 16-byte vectors in fp32 only


def cases():
    out = []
    for H, W, C, share in SHAPES:
        for dtype, name in zip(DTYPES, IDS):
            if not skip_shape(C, dtype):
                out.append(pytest.param(H, W, C, share, dtype, id="%dx%dx%d-s%d-%s" % (H, W, C, share, name)))
    return out


CASES = pytest.mark.parametrize("H,W,C,share,dtype", cases())
PADS = pytest.mark.parametrize("pad", [0, 1], ids=["tight", "padded"])


def field(H, W, C, dtype, seed):
    """x (rows, C) in the storage type and the LayerNorm operands on the device"""
    rows = B * H * W
    x = rand((rows, C), seed, -2.0, 2.0).to(dtype)
    mean, rstd = rand((rows,), seed + 1).to(DEV), rand((rows,), seed + 2, 0.5, 2.0).to(DEV)
    gamma, beta = rand((C,), seed + 3, 0.25, 4.0).to(DEV), rand((C,), seed + 4).to(DEV)
    return x, mean, rstd, gamma, beta


def positions(H, W, n):
    """the position along w / along h of every row (pixel), as (rows, n) int64"""
    xs = torch.arange(W).view(1, 1, W).expand(B, H, W).reshape(-1, 1).expand(-1, n)
    ys = torch.arange(H).view(1, H, 1).expand(B, H, W).reshape(-1, 1).expand(-1, n)
    return xs, ys


def run_sample(x, ln, off, H, W, C, share, dtype, pad, which="whc", one_buffer=False):
    """-> (v = mlpk_norm_apply's stored output (rows, C) on the CPU, {"w" | "h" | "c": dense result on the CPU}); guard bands checked"""
    E = engine()
    rows, n_off = B * H * W, 2 * C // share
    mean, rstd, gamma, beta = ln
    gx = Guarded(rows, C, C + 8 if pad else C, dtype, DEV, role="in", data=x)
    go = Guarded(rows, n_off, n_off + 3 if pad else n_off, dtype, DEV, role="in", data=off)
    if one_buffer:
        buf = Guarded(rows, 3 * C + 8, 3 * C + 16 if pad else 3 * C + 8, dtype, DEV, role="out")
        outs = {k: buf.view[:, i * C:(i + 1) * C] for i, k in enumerate("whc")}
        guards = [buf]
    else:
        gs = {k: Guarded(rows, C, C + 8 if pad else C, dtype, DEV, role="out") for k in which}
        outs = {k: g.view for k, g in gs.items()}
        guards = list(gs.values())
    E.atm_sample(gx.view, mean, rstd, gamma, beta, go.view, share, outs.get("w"), outs.get("h"), outs.get("c"), B, H, W, C)
    torch.cuda.synchronize()
    gx.check()
    go.check()
    for g in guards:
        g.check()
    if one_buffer:
        buf.still_poison(3 * C, 3 * C + 8)                          # columns at or beyond the slices are not touched
    if C % 8 == 0:
        ref = torch.empty((rows, C), dtype=dtype, device=DEV)
        E.norm_apply(gx.view, rows, C, gx.ld, mean=mean, rstd=rstd, gamma=gamma, beta=beta, out_rm=ref, ld_rm=C)
    else:                                                           # mlpk_norm_apply takes C % 8 == 0: the same elementwise expression on zero-padded columns
        Cp = (C + 7) // 8 * 8
        xp, gp, bp = torch.zeros((rows, Cp), dtype=dtype, device=DEV), torch.ones((Cp,), device=DEV), torch.zeros((Cp,), device=DEV)
        xp[:, :C], gp[:C], bp[:C] = gx.view, gamma, beta
        ref = torch.empty((rows, Cp), dtype=dtype, device=DEV)
        E.norm_apply(xp, rows, Cp, Cp, mean=mean, rstd=rstd, gamma=gp, beta=bp, out_rm=ref, ld_rm=Cp)
        ref = ref[:, :C].contiguous()
    torch.cuda.synchronize()
    res = {k: v.clone().contiguous().cpu() for k, v in outs.items()}
    for k, v in res.items():
        assert_finite(v, "out_" + k)
    return ref.cpu(), res


def per_channel(off, C, share):
    """(rows, 2C / share) -> the offset of every channel: (rows, C) along w, (rows, C) along h  [column c / share, column (C + c) / share]"""
    full = off.repeat_interleave(share, dim=1)
    return full[:, :C], full[:, C:]


def restate(v, off_c, axis, H, W, C):
    """torchvision's rule in fp64 on the stored operand v (rows, C) and the stored per-channel offsets (rows, C): (exact, |v0| + |v1|, inside)"""
    v4 = v.double().view(B, H, W, C)
    o4 = off_c.double().view(B, H, W, C)
    L = W if axis == "w" else H
    dim = 2 if axis == "w" else 1
    pos = (torch.arange(W).view(1, 1, W, 1) if axis == "w" else torch.arange(H).view(1, H, 1, 1)).double()
    p = pos + o4
    inside = (p > -1) & (p < L)                                     # False for NaN
    pz = torch.where(inside, p, torch.zeros_like(p))
    i0 = torch.floor(pz)
    f = pz - i0
    i0 = i0.long()

    def tap(i):
        ok = inside & (i >= 0) & (i <= L - 1)
        val = torch.gather(v4, dim, i.clamp(0, L - 1))
        return torch.where(ok, val, torch.zeros_like(val))
    v0, v1 = tap(i0), tap(i0 + 1)
    exact = torch.where(inside, (1 - f) * v0 + f * v1, torch.zeros_like(v0))
    return exact.view(-1, C), (v0.abs() + v1.abs()).view(-1, C), inside.view(-1, C)


def gate(exact, mag, dtype):
    g = mag * 2.0 ** -17
    if dtype != torch.float32:
        m, emin = MANT[dtype]
        e = torch.floor(torch.log2(exact.abs().clamp(min=2.0 ** emin))).clamp(min=emin)
        g = g + 0.5 * torch.exp2(e - m)
    return g


def name_bad(bad, H, W, C):
    r, c = torch.nonzero(bad)[0].tolist()
    return "(b %d, y %d, x %d, c %d)" % (r // (H * W), r // W % H, r % W, c)


@CASES
@PADS
def test_integer_offsets_shift_norm_apply_bit_for_bit(H, W, C, share, dtype, pad):
    seed = H * 1000 + W * 100 + C + share
    x, *ln = field(H, W, C, dtype, seed)
    n = C // share
    g = torch.Generator().manual_seed(seed + 9)
    off = torch.cat([torch.randint(-W - 1, W + 2, (B * H * W, n), generator=g), torch.randint(-H - 1, H + 2, (B * H * W, n), generator=g)], 1).float()
    v, res = run_sample(x, ln, off.to(dtype), H, W, C, share, dtype, pad)
    assert_bits_equal(res["c"], v, "out_c")
    ow, oh = per_channel(off.long(), C, share)
    v4 = v.view(B, H, W, C)
    xs, ys = positions(H, W, C)
    for key, o, pos, L, dim in (("w", ow, xs, W, 2), ("h", oh, ys, H, 1)):
        src = (pos + o).view(B, H, W, C)
        ok = (src >= 0) & (src < L)
        want = torch.where(ok, torch.gather(v4, dim, src.clamp(0, L - 1)), torch.zeros_like(v4)).view(-1, C)
        bad = res[key].view(INT_VIEW[dtype]) != want.contiguous().view(INT_VIEW[dtype])
        assert not bool(bad.any()), "out_%s%s is not the operand %d pixels away (%d elements differ)" % (
            key, name_bad(bad, H, W, C), int(o[tuple(torch.nonzero(bad)[0].tolist())]), int(bad.sum()))


@CASES
@PADS
@pytest.mark.parametrize("span", ["wide", "near"])
def test_real_offsets_against_fp64(H, W, C, share, dtype, pad, span):
    seed = H * 1000 + W * 100 + C + share + (50 if span == "near" else 0)
    x, *ln = field(H, W, C, dtype, seed)
    n = C // share
    rows = B * H * W
    if span == "wide":                                              # uniform in [-L - 2, L + 2]
        off = torch.cat([rand((rows, n), seed + 5, -W - 2.0, W + 2.0), rand((rows, n), seed + 6, -H - 2.0, H + 2.0)], 1)
    else:
        off = rand((rows, 2 * n), seed + 5, -1.5, 1.5)
    off = off.to(dtype)
    v, res = run_sample(x, ln, off, H, W, C, share, dtype, pad, which="wh")
    ow, oh = per_channel(off, C, share)
    for key, o in (("w", ow), ("h", oh)):
        exact, mag, inside = restate(v, o, key, H, W, C)
        d = (res[key].double() - exact).abs()
        g = gate(exact, mag, dtype)
        worst = float((d / g.clamp(min=1e-300)).max())
        print("out_%s %s: max |d| %.3e, worst |d| / gate %.3f, inside %.2f" % (key, dtype, float(d.max()), worst, float(inside.double().mean())))
        bad = d > g
        assert not bool(bad.any()), "out_%s%s: |d| %.3e over its gate %.3e (%d elements)" % (
            key, name_bad(bad, H, W, C), float(d[bad][0]), float(g[bad][0]), int(bad.sum()))
        assert bool((res[key].view(INT_VIEW[dtype])[~inside] == 0).all()), "a sample outside the map must be +0"


@CASES
@PADS
def test_special_offsets_give_zero_and_stay_inside(H, W, C, share, dtype, pad):
    seed = H * 1000 + W * 100 + C + share + 77
    x, *ln = field(H, W, C, dtype, seed)
    n, rows = C // share, B * H * W
    off = rand((rows, 2 * n), seed + 5, -1.5, 1.5)
    xs, ys = positions(H, W, n)
    pos = torch.cat([xs, ys], 1).float()
    L = torch.cat([torch.full((rows, n), float(W)), torch.full((rows, n), float(H))], 1)
    consts = [0.0, -0.0, 1e-45, -1e-40, 1e30, -1e30, 3e9, -3e9, float("inf"), float("-inf"), float("nan")]
    cand = [torch.full_like(off, c) for c in consts] + [-1.0 - pos, L - 1.0 - pos, L - pos, -pos]        # p = -1, L - 1, L, 0 exactly
    g = torch.Generator().manual_seed(seed + 6)
    pick = torch.randint(0, len(cand), off.shape, generator=g)
    chosen = torch.stack(cand, 0).gather(0, pick.unsqueeze(0))[0]
    off = torch.where(torch.rand(off.shape, generator=g) < 0.4, chosen, off).to(dtype)
    v, res = run_sample(x, ln, off, H, W, C, share, dtype, pad)           # (finite outputs and intact guard bands are checked inside)
    assert_bits_equal(res["c"], v, "out_c")
    ow, oh = per_channel(off, C, share)
    for key, o in (("w", ow), ("h", oh)):
        exact, mag, inside = restate(v, o, key, H, W, C)
        assert bool((~inside).any())
        assert bool((res[key].view(INT_VIEW[dtype])[~inside] == 0).all()), "out_%s: exactly +0 where the rule says 0" % key
        d = (res[key].double() - exact).abs()
        bad = d > gate(exact, mag, dtype)
        assert not bool(bad.any()), "out_%s%s: |d| %.3e (%d elements)" % (key, name_bad(bad, H, W, C), float(d[bad][0]), int(bad.sum()))


@CASES
def test_null_outputs_and_column_slices_give_the_same_bits(H, W, C, share, dtype):
    seed = H * 1000 + W * 100 + C + share + 13
    x, *ln = field(H, W, C, dtype, seed)
    off = rand((B * H * W, 2 * C // share), seed + 5, -2.5, 2.5).to(dtype)
    _, full = run_sample(x, ln, off, H, W, C, share, dtype, 0)
    for which in ("w", "h", "c", "wh", "hc", "wc"):
        _, part = run_sample(x, ln, off, H, W, C, share, dtype, 1, which=which)
        for k in which:
            assert_bits_equal(part[k], full[k], "out_%s of the call with outputs %r" % (k, which))
    for pad in (0, 1):
        _, sl = run_sample(x, ln, off, H, W, C, share, dtype, pad, one_buffer=True)
        for k in "whc":
            assert_bits_equal(sl[k], full[k], "out_%s as a column slice" % k)


# ------------------------------------------------------------------ the model against the reference
def widen(sd_or_model, meta, seed):
    """tests/golden/make_active_golden.py `widen`: every offset Linear's bias from [-3, 3), keyed by the parameter's name"""
    w = meta["wide"]
    with torch.no_grad():
        for name, p in sd_or_model.named_parameters():
            if name.endswith(w["suffix"]):
                p.copy_(torch.from_numpy(portable_tensor(name, tuple(p.shape), w["lo"], w["hi"], seed=seed)))


def load_portable(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = portable_state_dict(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def lowp_gate(z, dtype, m):
    tag = "fp16" if dtype == torch.float16 else "bf16"
    rel = float(z["real/ActiveTiny/err_%s" % tag]) / float(np.abs(z["real/ActiveTiny/logits"]).max())
    return 2.0 * rel * m


def check(out, ref, dtype, z):
    m = float(np.abs(ref).max())
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    gate_ = 1e-5 * m if dtype == torch.float32 else lowp_gate(z, dtype, m)
    print("%s: max|d| %.3e gate %.3e max|ref| %.3f" % (dtype, err, gate_, m))
    assert err <= gate_, (str(dtype), err, gate_, m)


def tiny_model(meta, case):
    cfg = meta["tiny_cases"][case]
    model = load_portable(mp().ActiveMLP(**dict(meta["tiny"], **cfg["kw"])), meta["tiny_seed"])
    widen(model, meta, meta["tiny_seed"])
    x = torch.from_numpy(portable_input((2, 3, cfg["size"][0], cfg["size"][1]), seed=meta["tiny_seed"])).to(DEV)
    return model.to(DEV).eval(), x


@pytest.mark.parametrize("case", ["s64", "s40x52", "intv6_share1"])
def test_tiny_logits_fp32(case, z, meta):
    model, x = tiny_model(meta, case)
    with torch.no_grad():
        out = model(x)
    ref = z["tiny/" + case]
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
    check(out, ref, torch.float32, z)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ["s64", "s40x52"])
def test_tiny_logits_16bit(case, dtype, z, meta):
    model, x = tiny_model(meta, case)
    with torch.no_grad():
        out = model(x.to(dtype))
    assert out.dtype == dtype
    check(out, z["tiny/" + case], dtype, z)


def test_tiny_compute_dtype(z, meta):
    """set_compute_dtype: fp32 input, bf16 kernels, fp32 logits"""
    model, x = tiny_model(meta, "s64")
    model.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32
    check(out, z["tiny/s64"], torch.bfloat16, z)


@pytest.mark.parametrize("name", ["atm_5_7_16", "atm_14_14_48", "atm_1_6_8"])
def test_atm_layer_alone_fp32(name, z, meta):
    H, W, C = meta["blocks"][name]
    seed = meta["block_seed"]
    blk = load_portable(mp().active_mlp.ATMLayer(C), seed).to(DEV).eval()
    x = torch.from_numpy(portable_input((2, H, W, C), seed=seed)).to(DEV)
    lo, hi = meta["offset_range"]
    off = torch.from_numpy(portable_tensor("offset", (2, 2 * C, H, W), lo, hi, seed=seed)).to(DEV)
    with torch.no_grad():
        out = blk(x, off)
    ref = z["block/" + name]
    assert tuple(out.shape) == ref.shape and out.dtype == torch.float32
    m = float(np.abs(ref).max())
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print("%s: max|d| %.3e gate %.3e" % (name, err, 1e-5 * m))
    assert err <= 1e-5 * m, (err, m)


@pytest.fixture(scope="module")
def real_model(z, meta):
    """ActiveTiny from a state_dict in the reference's layout (keys and shapes of the fixture's table), loaded with strict=True"""
    shapes = {k: tuple(v) for k, v in json.loads(str(z["shapes/ActiveTiny"])).items()}
    sd = {k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}
    model = mp().active_mlp.ActiveTiny()
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    widen(model, meta, 0)
    return model.to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_logits(real_model, dtype, z):
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = real_model(x.to(dtype))
    check(out, z["real/ActiveTiny/logits"], dtype, z)


def test_deterministic_and_in_flight(meta):
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    model, _ = tiny_model(meta, "s64")
    xs = [torch.from_numpy(portable_input((4, 3, 64, 64), seed=90 + i)).to(DEV).bfloat16() for i in range(4)]
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
    """packed weights follow the parameters: an in-place update of an offset Linear's bias, of an atm_w weight and of a PEG tap each changes the
    next forward to what a freshly built model with those weights gives, bit for bit"""
    model, x = tiny_model(meta, "s64")
    x = x.to(dtype)
    with torch.no_grad():
        outs = [model(x).clone()]
        model.blocks[1][2].offset_layer[1].bias.add_(0.75)
        outs.append(model(x).clone())
        model.blocks[2][1].atm.atm_w.weight.mul_(-1.0)
        outs.append(model(x).clone())
        model.pos_blocks[0].proj.weight[:, 0, 0, 2].add_(0.5)
        outs.append(model(x).clone())
    for a, b in zip(outs, outs[1:]):
        assert not torch.equal(a, b)
    twin = mp().ActiveMLP(**meta["tiny"])
    twin.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    with torch.no_grad():
        assert torch.equal(twin.to(DEV).eval()(x), outs[-1])


def test_train_mode_warns_inference_only(meta):
    model, x = tiny_model(meta, "s64")
    model.train()
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(x)
    assert out.grad_fn is None
