"""-m gpu, 16-bit storage: the rounding budget of every single-product path.

On Gaussian data the kernel's rms error against the fp64 restatement of its contract (epilogue included) is divided by the rms error
of that fp64 result rounded ONCE to the storage type.  fp32 accumulation and one rounding give 1.000; two roundings about 1.35;
accumulators kept in 16 bits 1.6 at K = 200 and 3.5 at K = 3072.  The gate is

    rms(got - ref64) <= 1.10 * sqrt(r) * rms(round(ref64) - ref64)

with r the number of roundings to the storage type that include/mlpk.h states for the path; the 1.10 covers fp32 accumulation
(well under 1 %) and the 16-bit GELU forms (csrc/mlpk_common.h: +1 .. 3 % rms).  The denominator comes from the reference alone.
Two shapes per path: K about 200 and K = 3072 (or the path's largest K), where accumulation faults separate by 3 x and more.

r by path, as mlpk.h states it:
  mlpk_gemm_nt, 16-bit output, no residual                                        1
  ... with a residual / gate: v is rounded, R applied, rounded again                2   (the token-transposed output of tiles that
      straddle images applies R to the fp32 value: 1)
  mlpk_token_gemm, _ln (the operand's own rounding is part of the reference)        1
  mlpk_token_gemm_ln_post                                                           2
  mlpk_conv_gemm_nhwc (no residual), mlpk_patch_embed4 without LayerNorm, mlpk_stem7  1
Each test prints `RATIO <path> <dtype> <shape> r=<r> <ratio>`; profiles/exact_rounding_ratios.txt holds one run's lines."""
import math

import pytest
import torch

import exact as X
import oracle
from conftest import load_pkg

pytestmark = pytest.mark.gpu
SIXTEEN = [torch.float16, torch.bfloat16]
MARGIN = 1.10


def dev():
    return torch.device("cuda:0")


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def budget(path, dtype, shape, got, ref64, r):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), (path, "non-finite output")
    err = (got - ref64).pow(2).mean().sqrt().item()
    floor = (ref64.to(dtype).double() - ref64).pow(2).mean().sqrt().item()
    ratio = err / floor
    print("RATIO %-34s %-8s %-26s r=%d %.4f" % (path, str(dtype).replace("torch.", ""), "x".join(str(s) for s in shape), r, ratio))
    assert err <= MARGIN * math.sqrt(r) * floor, "%s %s %s: rms error %.4g is %.3f x the one-rounding floor %.4g (budget %.3f for r = %d)" % (
        path, dtype, shape, err, ratio, floor, MARGIN * math.sqrt(r), r)
    # ... and from below where two roundings are stated: a case that quietly took a one-rounding path (ratio 1.00 .. 1.02) would pass the
    # budget; two independent roundings of comparable size give sqrt(2) = 1.41, and 1.2 lies well clear of both
    assert r == 1 or ratio > 1.2, "%s %s %s: ratio %.3f says ONE rounding where mlpk.h states two: the intended path did not run" % (path, dtype, shape, ratio)
    return ratio


def gemm_operands(dtype, M, N, K, seed):
    A = rnd((M, K), dtype, seed)
    B = rnd((N, K), dtype, seed + 1, 1.0 / math.sqrt(K))
    bias = rnd((N,), torch.float32, seed + 2)
    return A, B, bias


TILES = X.TILES


@pytest.mark.parametrize("dtype", SIXTEEN)
@pytest.mark.parametrize("algo", sorted(TILES))
def test_gemm_row_major(dtype, algo):
    E, N = load_pkg().engine, load_pkg()._native
    (bm, bn, _), gran = TILES[algo], X.granule_of(algo, dtype)
    for K in (200 // gran * gran, 3072):
        M, Nn = bm + 1, bn + 8
        A, B, bias = gemm_operands(dtype, M, Nn, K, 100 + algo)
        R = rnd((M, Nn), dtype, 103 + algo)
        acc = A.double() @ B.double().t() + bias.double()
        for name, act, res, r in (("bias", 0, 0, 1), ("gelu", 1, 0, 1), ("res_add", 0, 1, 2), ("res_mul", 0, 2, 2)):
            C = torch.full((M, Nn), float("nan"), dtype=dtype, device=dev())
            E.gemm(A.to(dev()), B.to(dev()), C, M, Nn, K, bias=bias.to(dev()), act=act, R=R.to(dev()) if res else None, res=res, algo=algo)
            torch.cuda.synchronize()
            ref = oracle.gelu(acc) if act else acc
            ref = ref + R.double() if res == 1 else ref * R.double() if res == 2 else ref
            budget("gemm_nt algo %d rowmajor %s" % (algo, name), dtype, (M, Nn, K), C, ref, r)


@pytest.mark.parametrize("dtype", SIXTEEN)
@pytest.mark.parametrize("algo", sorted(TILES))
def test_gemm_token_transposed(dtype, algo):
    """tiles that straddle images (36 channels per image) apply the residual to the fp32 value: one rounding; whole tiles inside
    one image (algos 4, 12, 13: t_rows = the tile height) take the LDS-staged store, which rounds before the residual: two"""
    E, N = load_pkg().engine, load_pkg()._native
    (bm, bn, _), gran = TILES[algo], X.granule_of(algo, dtype)
    forms = [("direct", 36, -(-(bm + 1) // 36), 1)]
    if algo in (4, 12, 13):
        forms.append(("staged", bm, 2, 2))
    for K in (200 // gran * gran, 3072):
        for form, t_rows, nimg, r in forms:
            M, S = nimg * t_rows, bn + 8
            A, B, bias = gemm_operands(dtype, M, S, K, 200 + algo)
            R = rnd((nimg * S, t_rows), dtype, 203 + algo)
            core = (A.double() @ B.double().t() + bias.double()).reshape(nimg, t_rows, S).permute(0, 2, 1)
            for name, res in (("none", 0), ("res_add", 1), ("res_mul", 2)):
                C = torch.full((nimg * S, t_rows), float("nan"), dtype=dtype, device=dev())
                E.gemm(A.to(dev()), B.to(dev()), C, M, S, K, ldc=t_rows, bias=bias.to(dev()), R=R.to(dev()) if res else None, ldr=t_rows if res else None,
                       res=res, out_mode=N.OUT_TOKEN_T, t_rows=t_rows, t_tokens=S, algo=algo)
                torch.cuda.synchronize()
                rr = R.double().reshape(nimg, S, t_rows)
                ref = core + rr if res == 1 else core * rr if res == 2 else core
                budget("gemm_nt algo %d token_t %s %s" % (algo, form, name), dtype, (M, S, K), C.reshape(nimg, S, t_rows), ref, r if res else 1)


@pytest.mark.parametrize("dtype", SIXTEEN)
@pytest.mark.parametrize("algo", [14, 15])
def test_gemm_persistent_and_generated_tiles(dtype, algo):
    """whole tiles only, row-major only (both refuse the token-transposed output).  The generated tile refuses the gate (res_mode MUL) and
    has the GELU + folded-LayerNorm class instead."""
    E, N = load_pkg().engine, load_pkg()._native
    M, Nn = (320, 256) if algo == 14 else (256, 128)
    for K in (192, 3072):
        A, B, bias = gemm_operands(dtype, M, Nn, K, 300 + algo)
        R = rnd((M, Nn), dtype, 303 + algo)
        raw = A.double() @ B.double().t()
        mean, rstd = rnd((M,), torch.float32, 304 + algo, 0.1), rnd((M,), torch.float32, 305 + algo, 0.1) + 1.0
        csum = B.float().sum(dim=1)
        folded = (raw - mean.double()[:, None] * csum.double()[None, :]) * rstd.double()[:, None]
        forms = [("bias", 0, 0, 1, False), ("gelu", 1, 0, 1, False), ("res_add", 0, 1, 2, False)]
        forms.append(("res_mul", 0, 2, 2, False) if algo == 14 else ("gelu_ln", 1, 0, 1, True))
        for name, act, res, r, ln in forms:
            C = torch.full((M, Nn), float("nan"), dtype=dtype, device=dev())
            E.gemm(A.to(dev()), B.to(dev()), C, M, Nn, K, bias=bias.to(dev()), act=act, R=R.to(dev()) if res else None, res=res, algo=algo,
                   ln=(mean.to(dev()), rstd.to(dev()), csum.to(dev())) if ln else None)
            torch.cuda.synchronize()
            acc = (folded if ln else raw) + bias.double()
            ref = oracle.gelu(acc) if act else acc
            ref = ref + R.double() if res == 1 else ref * R.double() if res == 2 else ref
            budget("gemm_nt algo %d rowmajor %s" % (algo, name), dtype, (M, Nn, K), C, ref, r)


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_token_gemm(dtype):
    """S = 196 and S = 224, the largest K the token kernels take.  The LayerNorm / Aff operand is rounded once by contract: the
    reference multiplies the rounded operand, so that rounding is not the product's."""
    E, N = load_pkg().engine, load_pkg()._native
    nimg, C = 3, 96
    for S in (196, 224):
        rows = nimg * S
        w = rnd((S, S), torch.float32, 400 + S, 1.0 / math.sqrt(S))
        bias = rnd((S,), torch.float32, 401 + S)
        wp, bp, ng = E.pack_token_gemm(w, bias, dtype, dev())
        wr = w.to(dtype).double()
        g1 = (rnd((C,), torch.float32, 402 + S) * 0.3 + 0.5)
        # mlpk_token_gemm: residual in place, per-channel scale
        xn = rnd((nimg, S, C), dtype, 403 + S)
        sp = E.round_up(S, 32)
        xt = torch.zeros((nimg * C, sp), dtype=dtype, device=dev())
        xt[:, :S] = xn.permute(0, 2, 1).reshape(nimg * C, S).to(dev())
        x = rnd((rows, C), dtype, 404 + S)
        out = x.to(dev())
        E.token_gemm(xt, sp, nimg * C, S, wp, bp, ng, out, C, C, R=out, ldr=C, res=N.RES_ADD, rscale=g1.to(dev()), rperiod=C)
        torch.cuda.synchronize()
        core = torch.einsum("ts,bsc->btc", wr, xn.double()) + bias.double().view(1, -1, 1)
        budget("token_gemm res_add", dtype, (nimg * C, S, S), out.reshape(nimg, S, C), x.double().reshape(nimg, S, C) + core * g1.double().view(1, 1, -1), 1)
        # mlpk_token_gemm_ln: LayerNorm operand, gate
        gamma, beta = rnd((C,), torch.float32, 405 + S) * 0.3 + 1.0, rnd((C,), torch.float32, 406 + S) * 0.2
        wide = (rnd((rows, 2 * C), dtype, 407 + S) * 1.5 + 0.25).to(dev())
        v = wide[:, C:]
        mean = torch.empty((rows,), dtype=torch.float32, device=dev())
        rstd = torch.empty((rows,), dtype=torch.float32, device=dev())
        E.row_stats(v, rows, C, 2 * C, mean, rstd)
        out = torch.full((rows, C), float("nan"), dtype=dtype, device=dev())
        E.token_gemm_ln(v, 2 * C, nimg * C, S, mean, rstd, gamma.to(dev()), beta.to(dev()), wp, bp, ng, out, C, C, R=wide, ldr=2 * C, res=N.RES_MUL)
        torch.cuda.synchronize()
        vn = ((v.double().cpu() - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None] * gamma.double() + beta.double()).to(dtype).double().reshape(nimg, S, C)
        ref = (torch.einsum("ts,bsc->btc", wr, vn) + bias.double().view(1, -1, 1)) * wide.cpu().double()[:, :C].reshape(nimg, S, C)
        budget("token_gemm_ln res_mul", dtype, (nimg * C, S, S), out.reshape(nimg, S, C), ref, 1)
        # mlpk_token_gemm_ln, affine residual, and _ln_post on top of it
        xa = (x.double() * gamma.double() + beta.double()).to(dtype).double().reshape(nimg, S, C)
        ref = xa + (torch.einsum("ts,bsc->btc", wr, xa) + bias.double().view(1, -1, 1)) * g1.double().view(1, 1, -1)
        xin = x.to(dev())
        E.token_gemm_ln(xin, C, nimg * C, S, None, None, gamma.to(dev()), beta.to(dev()), wp, bp, ng, xin, C, C, R=xin, ldr=C, res=N.RES_ADD_AFFINE,
                        rscale=g1.to(dev()), rperiod=C)
        torch.cuda.synchronize()
        budget("token_gemm_ln res_add_affine", dtype, (nimg * C, S, S), xin.reshape(nimg, S, C), ref, 1)
        pa, pb = rnd((C,), torch.float32, 408 + S) * 0.3 + 1.0, rnd((C,), torch.float32, 409 + S) * 0.2
        assert E.token_gemm_ln_post_supported(dtype, S, C, C)
        xp = x.to(dev())
        E.token_gemm_ln(xp, C, nimg * C, S, None, None, gamma.to(dev()), beta.to(dev()), wp, bp, ng, xp, C, C, R=xp, ldr=C, res=N.RES_ADD_AFFINE,
                        rscale=g1.to(dev()), rperiod=C, post=(pa.to(dev()), pb.to(dev())))
        torch.cuda.synchronize()
        budget("token_gemm_ln_post", dtype, (nimg * C, S, S), xp.reshape(nimg, S, C), ref * pa.double() + pb.double(), 2)


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_conv_gemm_nhwc(dtype):
    """3 x 3 stride 2 pad 1 at 32 channels (K = 288) and 2 x 2 stride 2 at 768 channels (K = 3072)"""
    E = load_pkg().engine
    F = torch.nn.functional
    for ci, (B, H, W, Cin, Cout, k, st, pad) in enumerate([(2, 17, 15, 32, 136, 3, 2, 1), (2, 18, 16, 768, 136, 2, 2, 0)]):
        assert E.conv_gemm_nhwc_supported(dtype, Cin, k, k, st, pad)
        K = k * k * Cin
        x = rnd((B, H, W, Cin), dtype, 500 + ci)
        w = rnd((Cout, k, k, Cin), dtype, 501 + ci, 1.0 / math.sqrt(K))
        bias = rnd((Cout,), torch.float32, 502 + ci)
        Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        out = torch.full((B * Ho * Wo, Cout), float("nan"), dtype=dtype, device=dev())
        E.conv_gemm_nhwc(x.reshape(B * H * W, Cin).to(dev()), w.reshape(Cout, K).to(dev()), out, B, H, W, Cin, k, k, st, pad, bias=bias.to(dev()))
        torch.cuda.synchronize()
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), bias.double(), stride=st, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
        budget("conv_gemm_nhwc %dx%d" % (k, k), dtype, (B * Ho * Wo, Cout, K), out, ref, 1)


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_patch_embed4_and_stem7(dtype):
    """K = 48 and K = 147 are these kernels' only contraction lengths; two widths each"""
    E = load_pkg().engine
    F = torch.nn.functional
    for ci, (B, H, W, C) in enumerate([(2, 32, 36, 32), (1, 64, 36, 128)]):
        assert E.patch_embed4_supported(dtype, dtype, 3, H, W, C)
        x = rnd((B, 3, H, W), dtype, 600 + ci)
        wconv = rnd((C, 3, 4, 4), torch.float32, 601 + ci, 1.0 / math.sqrt(48))
        bias = rnd((C,), torch.float32, 602 + ci, 0.3)
        out = torch.full((B * (H // 4) * (W // 4), C), float("nan"), dtype=dtype, device=dev())
        E.patch_embed4(x.to(dev()), E.pack_matrix(wconv, dtype, dev()), bias.to(dev()), out, B, H, W, C)
        torch.cuda.synchronize()
        ref = F.conv2d(x.double(), wconv.to(dtype).double(), bias.double(), stride=4).flatten(2).transpose(1, 2).reshape(-1, C)
        budget("patch_embed4", dtype, (out.shape[0], C, 48), out, ref, 1)
    for ci, (B, H, W, C, pad) in enumerate([(2, 30, 40, 32, 2), (2, 36, 24, 128, 3)]):
        assert E.stem7_supported(dtype, dtype, 3, H, W, pad, C)
        x = rnd((B, 3, H, W), dtype, 610 + ci)
        wconv = rnd((C, 3, 7, 7), torch.float32, 611 + ci, 1.0 / math.sqrt(147))
        bias = rnd((C,), torch.float32, 612 + ci, 0.3)
        Ho, Wo = (H + 2 * pad - 7) // 4 + 1, (W + 2 * pad - 7) // 4 + 1
        out = torch.full((B * Ho * Wo, C), float("nan"), dtype=dtype, device=dev())
        E.stem7(x.to(dev()), E.pack_stem7(wconv, dtype, dev()), bias.to(dev()), out, B, H, W, pad, C)
        torch.cuda.synchronize()
        ref = F.conv2d(x.double(), wconv.to(dtype).double(), bias.double(), stride=4, padding=pad).permute(0, 2, 3, 1).reshape(-1, C)
        budget("stem7", dtype, (out.shape[0], C, 147), out, ref, 1)


# mlpk_dwconv_nhwc: one geometry of exact.DWCONV_TABLE per form and per k the form has
DWCONV_ROUNDING = {
    "mfma": [(2, 25, 31, 32, 3), (2, 31, 25, 32, 5), (2, 19, 17, 40, 7), (2, 17, 19, 40, 9)],
    "mfma_full": [(3, 32, 32, 32, k) for k in (3, 5, 7, 9)],
    "lds": [(2, 9, 40, 32, 3), (2, 9, 37, 40, 5), (1, 34, 34, 32, 7), (2, 33, 9, 32, 9)],
    "direct": [(1, 6, 6, 8, 1), (2, 7, 9, 68, 3), (2, 7, 9, 20, 5), (1, 48, 40, 32, 9), (1, 6, 6, 8, 11), (1, 20, 20, 40, 13)],
}


@pytest.mark.parametrize("dtype", SIXTEEN)
@pytest.mark.parametrize("form", sorted(DWCONV_ROUNDING))
def test_dwconv(dtype, form):
    """out = x + gelu(dw_k(x) + bias) bn_scale + bn_shift on Gaussian data with a non-trivial bn_scale: fp32 products and sums, the GELU
    (gelu_pk_n in the matrix-core and the LDS-tiled kernel, gelu_f in the generic one), ONE rounding at the store in all three kernels.
    The matrix-core form rounds the taps to the storage type (they are MFMA operands: mlpk.h), so its reference multiplies the rounded
    taps; the other two forms take them as fp32."""
    E = load_pkg().engine
    for (B, H, W, C, k) in DWCONV_ROUNDING[form]:
        assert (B, H, W, C, k) in X.DWCONV_CASES and X.dwconv_form(dtype, H, W, C, k) == form
        x = rnd((B, H, W, C), dtype, 700 + k)
        w = rnd((C, 1, k, k), torch.float32, 701 + k, 1.0 / k)
        bias = rnd((C,), torch.float32, 702 + k)
        bns = rnd((C,), torch.float32, 703 + k) * 0.2 + 1
        bnh = rnd((C,), torch.float32, 704 + k)
        out = torch.full((B, H, W, C), float("nan"), dtype=dtype, device=dev())
        E.dwconv_nhwc(x.to(dev()), out, B, H, W, C, k, w.reshape(C, k * k).t().contiguous().to(dev()), bias.to(dev()), bns.to(dev()), bnh.to(dev()))
        torch.cuda.synchronize()
        wr = (w.to(dtype) if form.startswith("mfma") else w).double()
        xn = x.double().permute(0, 3, 1, 2)
        d = torch.nn.functional.conv2d(xn, wr, bias.double(), padding=k // 2, groups=C)
        ref = (xn + oracle.gelu(d) * bns.double().view(1, C, 1, 1) + bnh.double().view(1, C, 1, 1)).permute(0, 2, 3, 1)
        budget("dwconv_nhwc %s k=%d" % (form, k), dtype, (B, H, W, C), out, ref, 1)
