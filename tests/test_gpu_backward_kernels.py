"""-m gpu: the backward kernels of mlpk_backward.hip one by one, in fp32 / fp16 / bf16 storage, at the shapes the models use and at the tails.

The kernels promise "fp32 math, one rounding per stored value".  Each case restates the operation in fp64 on the SAME rounded inputs and gates:
  * element-wise kernels: one rounding of the result (EPS[dtype] x |ref|, the storage type's ulp) plus fp32 slack in proportion to the sum of
    the magnitudes of the terms;
  * pure data movement (transposes without an addend, patch rows, shifts, gathers with kmax = 1): bit-exact;
  * reductions (col_sum, col_dot(_seg), dwconv_wgrad, LayerNorm / GroupNorm): a stated multiple of fp32 roundoff (2^-24) x the sum of |terms|.
Adjoint pairs are checked as <A x, y> = <x, A^T y> in fp64 on the kernels' own outputs.  The documented refusals return MLPK_ESHAPE /
MLPK_EMODE and leave a NaN-filled output untouched."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
EPS = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}      # one ulp at 1.0: a rounding is at most half
U32 = 2.0 ** -24                                                                             # fp32 unit roundoff
TINY = {torch.float32: 0.0, torch.float16: 2.0 ** -24, torch.bfloat16: 0.0}                  # fp16's subnormal spacing: a rounding near 0
ESHAPE, EMODE = -2, -5


def ctx():
    pkg = load_pkg()
    return pkg.engine, pkg._native.lib()


def rnd(shape, dtype, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype)


def nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def check_close(got, ref, slack, dtype, what):
    """|got - ref| <= one rounding of ref in the storage type + slack (all fp64, element-wise)"""
    got = got.double().cpu()
    err = (got - ref).abs()
    gate = EPS[dtype] * ref.abs() + slack + TINY[dtype]
    assert torch.isfinite(got).all(), what
    bad = err > gate
    assert not bad.any(), (what, str(dtype), int(bad.sum()), float(err.max()), float((err / gate.clamp_min(1e-300)).max()))
    return float((err / gate.clamp_min(1e-300)).max())


def exact(got, want, what):
    assert torch.equal(got.cpu(), want.cpu()), (what, float((got.cpu().double() - want.cpu().double()).abs().max()))


# ---------------------------------------------------------------- LayerNorm / GroupNorm
LN_CASES = [(4 * 196, 384, 0), (1000, 768, 0), (301, 1536, 0), (257, 2048, 0), (256 * 196, 384, 0), (4 * 196, 768, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C,strided", LN_CASES)
def test_layernorm_backward(rows, C, strided, dtype):
    """rows not a multiple of 256 and rows = 4 196 / 256 196; C up to the LDS limit 2048; strided: x is the right half of a 2C-wide tensor
    (gMLP's SGU normalises the v half in place), dy and dx have pitches of their own (untouched padding)"""
    E, L = ctx()
    seed = rows + C
    ldx, lddy, lddx = (2 * C, C + 8, 3 * C) if strided else (C, C, C)
    xw = (rnd((rows, ldx), dtype, seed) * 2 + 0.3).to(dtype)
    x = xw[:, ldx - C:]
    dyw = rnd((rows, lddy), dtype, seed + 1)
    dy = dyw[:, :C]
    gamma = rnd((C,), torch.float32, seed + 2, 0.5, 1.5)
    x64 = x.double()
    mu64 = x64.mean(1)
    mean = mu64.float()
    rstd = (1.0 / torch.sqrt(((x64 - mu64[:, None]) ** 2).mean(1) + 1e-5)).float()
    nb = L.mlpk_layernorm_backward_blocks(rows)
    part = torch.full((nb, 2, C), float("nan"), device=DEV)
    dxw = nan((rows, lddx), dtype)
    xd, dyd = xw.to(DEV), dyw.to(DEV)
    xptr = xd.data_ptr() + (ldx - C) * xd.element_size()
    m_d, r_d, g_d = mean.to(DEV), rstd.to(DEV), gamma.to(DEV)
    rc = L.mlpk_layernorm_backward(E.dtype_code(dtype), xptr, ldx, m_d.data_ptr(), r_d.data_ptr(), g_d.data_ptr(), dyd.data_ptr(), lddy,
                                   dxw.data_ptr(), lddx, part.data_ptr(), rows, C, E.stream())
    assert rc == 0
    sums = torch.empty(2 * C, device=DEV)
    assert L.mlpk_col_sum(0, part.data_ptr(), None, nb, 2 * C, 2 * C, 0, sums.data_ptr(), E.stream()) == 0
    torch.cuda.synchronize()
    # fp64 restatement with the SAME (fp32) mean / rstd the kernel is given
    xh = (x64 - mean.double()[:, None]) * rstd.double()[:, None]
    g = dy.double() * gamma.double()
    rs = rstd.double()[:, None]
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ref = rs * (g - m1 - xh * m2)
    # slack: the row means (a wave's running sums over C / 64 terms, then a 6-level tree) and x^ recomputed in fp32
    slack = 4 * (C / 64 + 8) * U32 * rs * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True) + xh.abs() * m2.abs())
    check_close(dxw[:, :C], ref, slack, dtype, "layernorm dx")
    assert torch.isnan(dxw[:, C:].float()).all() if lddx > C else True                       # padding columns untouched
    # dgamma = sum dy x^, dbeta = sum dy: per block 64-row running sums per wave, 4 waves, then a Kahan column sum over the blocks
    for j, t in ((0, dy.double() * xh), (1, dy.double())):
        want = t.sum(0)
        err = (sums[j * C:(j + 1) * C].double().cpu() - want).abs()
        gate = 96 * U32 * t.abs().sum(0) + 1e-30
        assert (err <= gate).all(), ("layernorm dgamma/dbeta", j, str(dtype), float((err / gate).max()))


def test_layernorm_backward_refuses_past_the_lds_limit():
    E, L = ctx()
    rows, C = 8, 2049
    x = torch.zeros((rows, C), device=DEV)
    st = torch.ones(rows, device=DEV)
    gam = torch.ones(C, device=DEV)
    dx = nan((rows, C), torch.float32)
    part = torch.full((1, 2, C), float("nan"), device=DEV)
    rc = L.mlpk_layernorm_backward(0, x.data_ptr(), C, st.data_ptr(), st.data_ptr(), gam.data_ptr(), x.data_ptr(), C, dx.data_ptr(), C,
                                   part.data_ptr(), rows, C, E.stream())
    torch.cuda.synchronize()
    assert rc == ESHAPE and torch.isnan(dx).all() and torch.isnan(part).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups,glen", [(2, 56 * 56 * 96), (3, 1000), (2, 4099)])
def test_group_norm_backward(groups, glen, dtype):
    """glen = AS-MLP stage 1's sample (56 56 96), shorter than one workgroup (1000 < 1024), not a multiple of 64"""
    E, L = ctx()
    xh = (rnd((groups, glen), dtype, glen, -2, 2)).to(dtype)
    g = rnd((groups, glen), dtype, glen + 1)
    rstd = rnd((groups,), torch.float32, glen + 2, 0.5, 2.0)
    dx = nan((groups, glen), dtype)
    xd, gd, rd = xh.to(DEV), g.to(DEV), rstd.to(DEV)
    assert L.mlpk_group_norm_backward(E.dtype_code(dtype), xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), dx.data_ptr(), groups, glen, E.stream()) == 0
    torch.cuda.synchronize()
    x64, g64, rs = xh.double(), g.double(), rstd.double()[:, None]
    m1, m2 = g64.mean(1, keepdim=True), (g64 * x64).mean(1, keepdim=True)
    ref = rs * (g64 - m1 - x64 * m2)
    # slack: the sums run glen / 1024 terms per lane, then 6 + 4 tree levels
    slack = 4 * (glen / 1024 + 16) * U32 * rs * (g64.abs() + g64.abs().mean(1, keepdim=True) + x64.abs() * (g64 * x64).abs().mean(1, keepdim=True) +
                                                 x64.abs() * m2.abs())
    check_close(dx, ref, slack, dtype, "group_norm dx")


# ---------------------------------------------------------------- column reductions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [70, 200, 768, 1536])
def test_col_sum_and_col_dot(cols, dtype):
    """64-column tails; a pitch past the row; `sub` and `square`; col_dot_seg with segments = images and seg_rows = H W"""
    E, L = ctx()
    rows, ld = 3001, cols + 5
    x = rnd((rows, ld), dtype, cols)
    y = rnd((rows, ld), dtype, cols + 1)
    xd, yd = x.to(DEV), y.to(DEV)
    code = E.dtype_code(dtype)
    x64, y64 = x[:, :cols].double(), y[:, :cols].double()
    for sub, sq in ((False, False), (True, False), (False, True), (True, True)):
        out = torch.full((cols + 64,), float("nan"), device=DEV)
        assert L.mlpk_col_sum(code, xd.data_ptr(), yd.data_ptr() if sub else None, rows, cols, ld, int(sq), out.data_ptr(), E.stream()) == 0
        torch.cuda.synchronize()
        v = x64 - y64 if sub else x64
        if dtype != torch.float32 and sub:
            v = v.float().double()          # the difference of two 16-bit values is exact in fp32; fp32: one rounding, in the gate below
        t = v * v if sq else v
        err = (out[:cols].double().cpu() - t.sum(0)).abs()
        gate = 8 * U32 * ((x64.abs() + (y64.abs() if sub else 0)) ** (2 if sq else 1)).sum(0)
        assert (err <= gate).all(), ("col_sum", sub, sq, str(dtype), float((err / gate).max()))
        assert torch.isnan(out[cols:]).all()
    out = torch.full((cols,), float("nan"), device=DEV)
    assert L.mlpk_col_dot(code, xd.data_ptr(), ld, yd.data_ptr(), ld, rows, cols, out.data_ptr(), E.stream()) == 0
    B, S = 4, 56 * 56 if cols <= 200 else 196
    xs, ys = rnd((B * S, cols), dtype, 7 * cols), rnd((B * S, cols), dtype, 7 * cols + 1)
    seg = torch.full((B, cols), float("nan"), device=DEV)
    xsd, ysd = xs.to(DEV), ys.to(DEV)
    assert L.mlpk_col_dot_seg(code, xsd.data_ptr(), cols, ysd.data_ptr(), cols, B, S, cols, seg.data_ptr(), E.stream()) == 0
    torch.cuda.synchronize()
    t = x64 * y64
    err = (out.double().cpu() - t.sum(0)).abs()
    assert (err <= 8 * U32 * t.abs().sum(0)).all(), ("col_dot", str(dtype))
    t = (xs.double() * ys.double()).reshape(B, S, cols)
    err = (seg.double().cpu() - t.sum(1)).abs()
    assert (err <= 8 * U32 * t.abs().sum(1)).all(), ("col_dot_seg", str(dtype), float(err.max()))


def test_col_sum_compensates_a_million_rows_of_one_sign():
    """rows > 10^6 of one sign: each of the 4 row lanes adds 2^18 terms; a plain fp32 sum would lose ~1e-5 of the total, the Kahan sum stays
    within a few units of fp32 roundoff of it"""
    E, L = ctx()
    rows, cols = (1 << 20) + 17, 70
    x = rnd((rows, cols), torch.float32, 99, 0.5, 1.5)
    xd = x.to(DEV)
    out = torch.empty(cols, device=DEV)
    assert L.mlpk_col_sum(0, xd.data_ptr(), None, rows, cols, cols, 0, out.data_ptr(), E.stream()) == 0
    dot = torch.empty(cols, device=DEV)
    assert L.mlpk_col_dot(0, xd.data_ptr(), cols, xd.data_ptr(), cols, rows, cols, dot.data_ptr(), E.stream()) == 0
    torch.cuda.synchronize()
    x64 = x.double()
    for got, want in ((out, x64.sum(0)), (dot, (x64 * x64).sum(0))):
        rel = ((got.double().cpu() - want).abs() / want).max().item()
        assert rel < 4 * U32, rel


# ---------------------------------------------------------------- element-wise, past the grid cap
BIG = (65600, 260, 264)          # rows x cols = 17.06 M > 2^24 = ew_grid's 65536 blocks x 256 lanes: the grid-stride loop runs twice


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_elementwise_past_the_grid_cap(dtype):
    E, L = ctx()
    rows, cols, ld = BIG
    a = (rnd((rows, ld), dtype, 5, -4, 4)).to(dtype)
    b = rnd((rows, ld), dtype, 6)
    ad, bd = a.to(DEV), b.to(DEV)
    a64, b64 = a[:, :cols].double(), b[:, :cols].double()
    Phi = 0.5 * (1 + torch.erf(a64 / 2 ** 0.5))
    phi = torch.exp(-0.5 * a64 * a64) / (2 * np.pi) ** 0.5
    for mode, ref in ((0, a64 * Phi), (1, b64 * (Phi + a64 * phi))):
        out = nan((rows, ld), dtype)
        assert L.mlpk_gelu_elementwise(E.dtype_code(dtype), mode, ad.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, cols, ld, E.stream()) == 0
        torch.cuda.synchronize()
        # the kernel's erf / exp are fp32 approximations: a few ulp of fp32 on the factor
        slack = 8 * U32 * (a64.abs() + 1) * (b64.abs() if mode else 1)
        check_close(out[:, :cols], ref, slack, dtype, "gelu mode %d" % mode)
        assert torch.isnan(out[:, cols:].float()).all()
        del out


@pytest.mark.parametrize("dtype", DTYPES)
def test_ew_cols_every_mode_past_the_grid_cap(dtype):
    E, L = ctx()
    rows, cols, ld = BIG
    period = 4096                                  # mode 3 / 5: rows / period = 16 groups, the last one short
    a, b = rnd((rows, ld), dtype, 11), rnd((rows, ld), dtype, 12)
    ad, bd = a.to(DEV), b.to(DEV)
    a64, b64 = a[:, :cols].double(), b[:, :cols].double()
    g, h, k = (rnd((cols,), torch.float32, s) for s in (13, 14, 15))
    ng = (rows + period - 1) // period
    gs = rnd((ng,), torch.float32, 16)
    g5, h5 = rnd((ng, cols), torch.float32, 17), rnd((ng, cols), torch.float32, 18)
    gd, hd, kd, gsd, g5d, h5d = (t.to(DEV) for t in (g, h, k, gs, g5, h5))
    grp = torch.arange(rows) // period
    G, H, K = g.double(), h.double(), k.double()
    cases = [(0, None, gd, hd, None, a64 * G + H, a64.abs() * G.abs() + H.abs()),
             (0, None, None, None, None, a64, a64.abs()),
             (1, bd, None, None, None, a64 * b64, (a64 * b64).abs()),
             (2, bd, gd, None, None, a64 + G * b64, a64.abs() + (G * b64).abs()),
             (2, bd, None, None, None, a64 + b64, a64.abs() + b64.abs()),
             (3, None, gsd, None, None, a64 * gs.double()[grp][:, None], (a64 * gs.double()[grp][:, None]).abs()),
             (4, bd, gd, hd, kd, a64 * G + b64 * H + K, (a64 * G).abs() + (b64 * H).abs() + K.abs()),
             (5, bd, g5d, h5d, None, a64 * g5.double()[grp] + h5.double()[grp] + b64, (a64 * g5.double()[grp]).abs() + h5.double()[grp].abs() + b64.abs()),
             (5, None, g5d, h5d, None, a64 * g5.double()[grp] + h5.double()[grp], (a64 * g5.double()[grp]).abs() + h5.double()[grp].abs()),
             (5, bd, g5d, None, None, a64 * g5.double()[grp] + b64, (a64 * g5.double()[grp]).abs() + b64.abs()),
             (5, None, g5d, None, None, a64 * g5.double()[grp], (a64 * g5.double()[grp]).abs())]
    for mode, bb, gg, hh, kk, ref, mag in cases:
        out = nan((rows, ld), dtype)
        rc = L.mlpk_ew_cols(E.dtype_code(dtype), mode, ad.data_ptr(), ld, E.ptr(bb), ld, E.ptr(gg), E.ptr(hh), E.ptr(kk), out.data_ptr(), ld,
                            rows, cols, period, E.stream())
        assert rc == 0, mode
        torch.cuda.synchronize()
        check_close(out[:, :cols], ref, 3 * U32 * mag, dtype, "ew_cols mode %d" % mode)
        assert torch.isnan(out[:, cols:].float()).all()
        del out


# ---------------------------------------------------------------- layout kernels
@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_batched_tails_pitches_and_addend(dtype):
    E, L = ctx()
    batch, R, Cc, ld_in, ld_out, ld_res = 3, 70, 45, 48, 72, 80
    x = rnd((batch, R, ld_in), dtype, 21)
    res = rnd((batch, Cc, ld_res), dtype, 22)
    xd, rd = x.to(DEV), res.to(DEV)
    code = E.dtype_code(dtype)
    for with_res in (False, True):
        out = nan((batch, Cc, ld_out), dtype)
        assert L.mlpk_transpose_batched(code, xd.data_ptr(), ld_in, out.data_ptr(), ld_out, rd.data_ptr() if with_res else None, ld_res, batch, R, Cc,
                                        E.stream()) == 0
        torch.cuda.synchronize()
        t = x[:, :, :Cc].transpose(1, 2)
        if with_res:
            exact(out[:, :, :R], (t.float() + res[:, :, :R].float()).to(dtype), "transpose + res (fp32 sum, one rounding)")
        else:
            exact(out[:, :, :R], t, "transpose")
        assert torch.isnan(out[:, :, R:].float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [0, 1])
def test_patch_rows_both_orders_and_directions(order, dtype):
    E, L = ctx()
    B, H, W, C, ph, pw = 2, 6, 8, 5, 2, 4
    x = rnd((B, H, W, C), dtype, 31 + order)
    xd = x.to(DEV)
    code = E.dtype_code(dtype)
    out = nan((B, H // ph, W // pw, ph * pw * C), dtype)
    assert L.mlpk_patch_rows_nhwc(code, 0, order, xd.data_ptr(), out.data_ptr(), B, H, W, C, ph, pw, E.stream()) == 0
    back = nan((B, H, W, C), dtype)
    assert L.mlpk_patch_rows_nhwc(code, 1, order, out.data_ptr(), back.data_ptr(), B, H, W, C, ph, pw, E.stream()) == 0
    torch.cuda.synchronize()
    p = x.reshape(B, H // ph, ph, W // pw, pw, C)                     # (b, y, i, x, j, c)
    want = p.permute(0, 1, 3, 2, 4, 5) if order == 0 else p.permute(0, 1, 3, 4, 2, 5)      # column (i pw + j) C + c  |  (j ph + i) C + c
    exact(out, want.reshape(B, H // ph, W // pw, ph * pw * C), "patch_rows order %d" % order)
    exact(back, x, "patch_rows round trip")


@pytest.mark.parametrize("dtype", DTYPES)
def test_broadcast_rows_and_add_periodic(dtype):
    E, L = ctx()
    B, S, C = 3, 49, 70
    x = rnd((B, C), dtype, 41)
    out = nan((B, S, C), dtype)
    xd = x.to(DEV)
    assert L.mlpk_broadcast_rows(E.dtype_code(dtype), xd.data_ptr(), out.data_ptr(), B, S, C, 1.0 / 3.0, E.stream()) == 0
    torch.cuda.synchronize()
    exact(out, (x.float() * np.float32(1.0 / 3.0)).to(dtype)[:, None, :].expand(B, S, C), "broadcast_rows (fp32 product, one rounding)")
    rows, period, ld = 7 * 5 + 3, 7, C + 6                           # the last period is cut short
    y = rnd((rows, ld), dtype, 42)
    t = rnd((period, C), torch.float32, 43)
    yd, td = y.to(DEV), t.to(DEV)
    assert L.mlpk_add_periodic(E.dtype_code(dtype), yd.data_ptr(), ld, td.data_ptr(), rows, C, period, E.stream()) == 0
    torch.cuda.synchronize()
    want = y.clone()
    want[:, :C] = (y[:, :C].float() + t[torch.arange(rows) % period]).to(dtype)
    exact(yd, want, "add_periodic (fp32 sum, one rounding)")


# ---------------------------------------------------------------- depthwise convolution
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 4, 7, 9])
def test_dwconv_plain_adjoint_and_wgrad(k, dtype):
    """odd and even k (9 = ConvMixer-1536/20) at C = 1536: forward and adjoint against fp64 conv2d, <A x, y> = <x, A^T y> on the kernels'
    outputs, the tap gradient against fp64 autograd"""
    E, L = ctx()
    B, H, W, C = 2, 11, 9, 1536
    code = E.dtype_code(dtype)
    x, y = rnd((B, H, W, C), dtype, 50 + k), rnd((B, H, W, C), dtype, 60 + k)
    w = rnd((k * k, C), torch.float32, 70 + k, -0.3, 0.3)
    bias = rnd((C,), torch.float32, 80 + k)
    xd, yd, wd, bd = x.to(DEV), y.to(DEV), w.to(DEV), bias.to(DEV)
    ax, aty = nan((B, H, W, C), dtype), nan((B, H, W, C), dtype)
    assert L.mlpk_dwconv_plain_nhwc(code, 0, xd.data_ptr(), ax.data_ptr(), B, H, W, C, k, wd.data_ptr(), bd.data_ptr(), E.stream()) == 0
    assert L.mlpk_dwconv_plain_nhwc(code, 1, yd.data_ptr(), aty.data_ptr(), B, H, W, C, k, wd.data_ptr(), bd.data_ptr(), E.stream()) == 0
    dw = torch.full((k * k, C), float("nan"), device=DEV)
    assert L.mlpk_dwconv_wgrad_nhwc(code, xd.data_ptr(), yd.data_ptr(), dw.data_ptr(), B, H, W, C, k, E.stream()) == 0
    torch.cuda.synchronize()
    xc = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wc = w.double().t().reshape(C, 1, k, k).requires_grad_(True)
    yc = y.double().permute(0, 3, 1, 2)
    p = (k - 1) // 2
    conv = lambda t, ww: torch.nn.functional.conv2d(torch.nn.functional.pad(t, (p, k // 2, p, k // 2)), ww, groups=C)
    o = conv(xc, wc)
    (o * yc).sum().backward()
    mag = conv(xc.detach().abs(), wc.detach().abs())
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    check_close(ax, nhwc(o.detach()) + bias.double(), 2 * k * k * U32 * (nhwc(mag) + bias.double().abs()), dtype, "dwconv fwd")
    ref_adj = torch.autograd.grad(conv(xc, wc.detach()), xc, yc)[0]
    mag_adj = torch.autograd.grad(conv(xc, wc.detach().abs()), xc, yc.abs())[0]
    check_close(aty, nhwc(ref_adj), 2 * k * k * U32 * nhwc(mag_adj), dtype, "dwconv adjoint")
    # <A x, y> = <x, A^T y> on what the kernels stored (bias off): the adjoint is the transpose of the forward, up to their roundings
    ax0 = nan((B, H, W, C), dtype)
    assert L.mlpk_dwconv_plain_nhwc(code, 0, xd.data_ptr(), ax0.data_ptr(), B, H, W, C, k, wd.data_ptr(), None, E.stream()) == 0
    torch.cuda.synchronize()
    lhs = (ax0.double().cpu() * y.double()).sum().item()
    rhs = (x.double() * aty.double().cpu()).sum().item()
    scale = (nhwc(mag).double() * y.double().abs()).sum().item()
    assert abs(lhs - rhs) <= 2 * EPS[dtype] * scale, (k, str(dtype), lhs, rhs)
    want = wc.grad.reshape(C, k * k).t()
    tw = wc.detach().clone().requires_grad_(True)
    (conv(xc.detach().abs(), tw) * yc.abs()).sum().backward()
    check_close(dw, want, 8 * U32 * tw.grad.reshape(C, k * k).t(), torch.float32, "dwconv wgrad")


# ---------------------------------------------------------------- S2-MLPv2 shifts, SplitAttention softmax
def s2_ref(x, which, mode, adjoint):
    """mlpk.h mlpk_s2_shift2 restated on (B, D1, D2, C): forward = the intended shift (mode 0) or the reference's smear (mode 1);
    adjoint = the adjoint of the INTENDED shift"""
    B, D1, D2, C = x.shape
    out = torch.zeros_like(x)
    bounds = [0, C // 4, C // 2, C * 3 // 4, C]
    for grp in range(4):
        sl = slice(bounds[grp], bounds[grp + 1])
        ax = 1 if (grp < 2) == (which == 1) else 2
        v = x[..., sl].movedim(ax, 1)
        n = v.shape[1]
        o = torch.zeros_like(v)
        if grp % 2 == 0:                         # +1 along the axis
            if not adjoint:
                o[:, 0] = v[:, 0]
                o[:, 1:] = v[:, :1].expand_as(v[:, 1:]) if mode == 1 else v[:, :n - 1]
            else:
                o[:, :n - 1] = v[:, 1:]
                o[:, 0] += v[:, 0]
        else:                                    # -1
            if not adjoint:
                o[:, n - 1] = v[:, n - 1]
                o[:, :n - 1] = v[:, 1:]
            else:
                o[:, 1:] = v[:, :n - 1]
                o[:, n - 1] += v[:, n - 1]
        out[..., sl] = o.movedim(1, ax)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [1, 2])
def test_s2_shift2_forward_and_adjoint(which, dtype):
    """C not a multiple of 32 (nor of 4), row pitches past C, D1 != D2; the adjoint of mode 0 is its transpose"""
    E, L = ctx()
    B, D1, D2, C, ldi, ldo = 2, 5, 7, 38, 40, 44
    code = E.dtype_code(dtype)
    x = rnd((B * D1 * D2, ldi), dtype, 90 + which)
    xd = x.to(DEV)
    x4 = x[:, :C].reshape(B, D1, D2, C)
    outs = {}
    for mode in (0, 1):
        for adjoint in (0, 1):
            out = nan((B * D1 * D2, ldo), dtype)
            assert L.mlpk_s2_shift2(code, which, mode, adjoint, xd.data_ptr(), ldi, out.data_ptr(), ldo, B, D1, D2, C, E.stream()) == 0
            torch.cuda.synchronize()
            want = s2_ref(x4.float(), which, mode, adjoint).to(dtype)            # data movement, or one rounding of a two-term fp32 sum
            exact(out[:, :C].reshape(B, D1, D2, C), want, "s2_shift2 which %d mode %d adjoint %d" % (which, mode, adjoint))
            assert torch.isnan(out[:, C:].float()).all()
            outs[mode, adjoint] = out[:, :C].double().cpu()
    ya = rnd((B * D1 * D2, C), dtype, 95).to(DEV)
    aty = nan((B * D1 * D2, C), dtype)
    assert L.mlpk_s2_shift2(code, which, 0, 1, ya.data_ptr(), C, aty.data_ptr(), C, B, D1, D2, C, E.stream()) == 0
    torch.cuda.synchronize()
    lhs = (outs[0, 0] * ya.double().cpu()).sum().item()
    rhs = (x[:, :C].double() * aty.double().cpu()).sum().item()
    assert abs(lhs - rhs) <= 2 * EPS[dtype] * (x[:, :C].double().abs() * 2 * ya.double().cpu().abs()).sum().item(), (lhs, rhs)


@pytest.mark.parametrize("B,C", [(4, 1000), (64, 768)])
def test_split_softmax_backward_against_the_fp64_jacobian(B, C):
    E, L = ctx()
    hat = rnd((B, 3, C), torch.float32, B + C, -3, 3)
    bar = torch.softmax(hat.double(), 1).float()
    dbar = rnd((B, 3, C), torch.float32, B + C + 1)
    dhat = torch.full((B, 3, C), float("nan"), device=DEV)
    bd, dd = bar.to(DEV), dbar.to(DEV)
    assert L.mlpk_split_softmax_backward(bd.data_ptr(), dd.data_ptr(), dhat.data_ptr(), B, C, E.stream()) == 0
    torch.cuda.synchronize()
    a, d = bar.double(), dbar.double()
    # the Jacobian of softmax over the branch axis applied to dbar: J[k, j] = a_k (delta_kj - a_j)
    J = torch.diag_embed(a.permute(0, 2, 1)) - a.permute(0, 2, 1)[..., :, None] * a.permute(0, 2, 1)[..., None, :]
    ref = (J @ d.permute(0, 2, 1)[..., None])[..., 0].permute(0, 2, 1)
    mag = a * (d.abs() + (a * d).abs().sum(1, keepdim=True))
    check_close(dhat, ref, 4 * U32 * mag, torch.float32, "split_softmax_backward")


# ---------------------------------------------------------------- index tables
def inverse_table(idx, n_in):
    """every source's list of readers, padded with -1 to the largest multiplicity (what the models build for the adjoint)"""
    readers = [[] for _ in range(n_in)]
    for i, j in enumerate(idx.tolist()):
        if j >= 0:
            readers[j].append(i)
    kmax = max(1, max(len(r) for r in readers))
    return torch.tensor([r + [-1] * (kmax - len(r)) for r in readers], dtype=torch.int32).reshape(-1), kmax


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [1, 96])
def test_index_gather_table_and_its_inverse_are_adjoint(width, dtype):
    """kmax = 1 with holes (a padded, rolled, overlapping remap: some sources read 3 times, some never) and the inverse table with kmax > 1;
    width 1 = CycleFC's per-channel shifts"""
    E, L = ctx()
    batch, n_in, n_out = 3, 50, 77
    g = torch.Generator().manual_seed(width)
    idx = torch.randint(0, n_in, (n_out,), generator=g, dtype=torch.int32)
    idx[torch.randperm(n_out, generator=g)[:9]] = -1
    idx[:6] = 17                                                                  # one source read six times
    inv, kmax = inverse_table(idx, n_in)
    assert kmax >= 6
    code = E.dtype_code(dtype)
    x = rnd((batch, n_in, width), dtype, 100 + width)
    y = rnd((batch, n_out, width), dtype, 101 + width)
    xd, yd, idd, ivd = x.to(DEV), y.to(DEV), idx.to(DEV), inv.to(DEV)
    gx, gty = nan((batch, n_out, width), dtype), nan((batch, n_in, width), dtype)
    assert L.mlpk_index_gather(code, xd.data_ptr(), gx.data_ptr(), idd.data_ptr(), batch, n_out, n_in, width, 1, E.stream()) == 0
    assert L.mlpk_index_gather(code, yd.data_ptr(), gty.data_ptr(), ivd.data_ptr(), batch, n_in, n_out, width, kmax, E.stream()) == 0
    torch.cuda.synchronize()
    want = torch.where((idx >= 0)[None, :, None], x[:, idx.clamp_min(0).long()], torch.zeros((), dtype=dtype))
    exact(gx, want, "index_gather kmax 1")
    ref = torch.zeros((batch, n_in, width), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    ok = idx >= 0
    ref.index_add_(1, idx[ok].long(), y[:, ok].double())
    mag.index_add_(1, idx[ok].long(), y[:, ok].double().abs())
    check_close(gty, ref, kmax * U32 * mag, dtype, "index_gather inverse (kmax %d)" % kmax)
    lhs = (gx.double().cpu() * y.double()).sum().item()
    rhs = (x.double() * gty.double().cpu()).sum().item()
    assert abs(lhs - rhs) <= 2 * EPS[dtype] * (x.double().abs()[:, idx.clamp_min(0).long()] * y.double().abs()).sum().item(), (lhs, rhs)


# ---------------------------------------------------------------- refusals
def test_documented_refusals_write_nothing():
    E, L = ctx()
    s = E.stream()
    x = torch.zeros((64, 64), device=DEV)
    w = torch.zeros((9, 64), device=DEV)
    idx = torch.zeros(64, dtype=torch.int32, device=DEV)
    out = nan((64, 64), torch.float32)
    calls = [
        ("s2_shift2 in == out", ESHAPE, lambda: L.mlpk_s2_shift2(0, 1, 0, 0, out.data_ptr(), 64, out.data_ptr(), 64, 1, 8, 8, 64, s)),
        ("s2_shift2 ldo < C", ESHAPE, lambda: L.mlpk_s2_shift2(0, 1, 0, 0, x.data_ptr(), 64, out.data_ptr(), 32, 1, 8, 8, 64, s)),
        ("s2_shift2 which 3", EMODE, lambda: L.mlpk_s2_shift2(0, 3, 0, 0, x.data_ptr(), 64, out.data_ptr(), 64, 1, 8, 8, 64, s)),
        ("patch_rows in == out", ESHAPE, lambda: L.mlpk_patch_rows_nhwc(0, 0, 0, out.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 2, 2, s)),
        ("patch_rows H % ph", ESHAPE, lambda: L.mlpk_patch_rows_nhwc(0, 0, 0, x.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 3, 2, s)),
        ("patch_rows order 2", EMODE, lambda: L.mlpk_patch_rows_nhwc(0, 0, 2, x.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 2, 2, s)),
        ("dwconv in == out", ESHAPE, lambda: L.mlpk_dwconv_plain_nhwc(0, 0, out.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 3, w.data_ptr(), None, s)),
        ("dwconv adjoint 2", EMODE, lambda: L.mlpk_dwconv_plain_nhwc(0, 2, x.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 3, w.data_ptr(), None, s)),
        ("index_gather in == out", ESHAPE, lambda: L.mlpk_index_gather(0, out.data_ptr(), out.data_ptr(), idx.data_ptr(), 1, 64, 64, 64, 1, s)),
        ("transpose batch > 65535", ESHAPE, lambda: L.mlpk_transpose_batched(0, x.data_ptr(), 1, out.data_ptr(), 1, None, 0, 65536, 1, 1, s)),
        ("transpose ld_out < R", ESHAPE, lambda: L.mlpk_transpose_batched(0, x.data_ptr(), 64, out.data_ptr(), 32, None, 0, 1, 64, 64, s)),
        ("col_dot_seg segments > 65535", ESHAPE, lambda: L.mlpk_col_dot_seg(0, x.data_ptr(), 1, x.data_ptr(), 1, 65536, 1, 1, out.data_ptr(), s)),
        ("ew_cols ld < cols", ESHAPE, lambda: L.mlpk_ew_cols(0, 0, x.data_ptr(), 32, None, 0, None, None, None, out.data_ptr(), 64, 64, 64, 1, s)),
        ("ew_cols ldo < cols", ESHAPE, lambda: L.mlpk_ew_cols(0, 0, x.data_ptr(), 64, None, 0, None, None, None, out.data_ptr(), 32, 64, 64, 1, s)),
        ("ew_cols mode 6", EMODE, lambda: L.mlpk_ew_cols(0, 6, x.data_ptr(), 64, None, 0, None, None, None, out.data_ptr(), 64, 64, 64, 1, s)),
        ("gelu ld < cols", ESHAPE, lambda: L.mlpk_gelu_elementwise(0, 0, x.data_ptr(), None, out.data_ptr(), 64, 64, 32, s)),
        ("gelu mode 2", EMODE, lambda: L.mlpk_gelu_elementwise(0, 2, x.data_ptr(), x.data_ptr(), out.data_ptr(), 64, 64, 64, s)),
        ("col_sum ld < cols", ESHAPE, lambda: L.mlpk_col_sum(0, x.data_ptr(), None, 64, 64, 32, 0, out.data_ptr(), s)),
        ("col_dot ld < cols", ESHAPE, lambda: L.mlpk_col_dot(0, x.data_ptr(), 32, x.data_ptr(), 64, 64, 64, out.data_ptr(), s)),
        ("add_periodic ld < C", ESHAPE, lambda: L.mlpk_add_periodic(0, out.data_ptr(), 32, x.data_ptr(), 64, 64, 7, s)),
        ("shift_nhwc_backward in == out", ESHAPE, lambda: L.mlpk_shift_nhwc_backward(0, out.data_ptr(), out.data_ptr(), 1, 8, 8, 64, 3, 2, s)),
    ]
    for what, want, call in calls:
        assert call() == want, what
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
