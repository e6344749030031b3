"""-m gpu: every matrix-core kernel held to EXACT integer results, bit for bit (tests/exact.py).

Operands are small integers, so the mathematically exact result is the only admissible output of a kernel whatever its tile, K
order or pipeline; the gate is equality, and a mismatch names the element and (one-hot pattern) the K index.  Three patterns run on
each kernel: one-hot (which k, which row), ternary (a term from every K slab in every output), cancel (|acc| > 2^12 brought back by
the fp32 bias: 16-bit accumulation or a rounding before the bias shows).  Kernels are reached through engine.py's wrappers and
pack_* functions, so packing orders are under test too.  check_case asserts the premises before any comparison."""
import ctypes

import pytest
import torch

import exact as X
from conftest import load_pkg

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def put(t, dtype):
    return None if t is None else t.to(dtype).to(dev()).contiguous()


class _Space:
    """the two-argument slice of engine.Workspace that engine.gemm(part=...) uses"""

    def get(self, name, shape, dtype):
        return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def run_gemm(c, algo, dbg=0, part=False, defer=False):
    """one mlpk_gemm_nt call for an exact.gemm_case; returns (C as float64 CPU in the shape of c.want, row_part or None)"""
    E, N = load_pkg().engine, load_pkg()._native
    X.check_case(c)
    dt = c.dtype
    A, B = put(c.A, dt), put(c.B, dt)
    f = torch.float32
    kw = dict(bias=put(c.bias, f), cscale=put(c.cscale, f), cshift=put(c.cshift, f), act=N.ACT_GELU if c.gelu else N.ACT_NONE, algo=algo, dbg=dbg)
    if c.rscale is not None:
        kw.update(rscale=put(c.rscale, f), rperiod=c.rperiod)
    if c.ln is not None:
        kw.update(ln=tuple(put(t, f) for t in c.ln), ln_group=c.ln_group)
    if c.t_rows:
        nimg = c.M // c.t_rows
        C = torch.full((nimg * c.t_tokens, c.t_rows), float("nan"), dtype=dt, device=dev())
        kw.update(out_mode=N.OUT_TOKEN_T, t_rows=c.t_rows, t_tokens=c.t_tokens, ldc=c.t_rows)
    else:
        C = torch.full((c.M, c.N), float("nan"), dtype=dt, device=dev())
    if c.res:
        R = put(c.R, dt)
        if c.r_alias:
            assert R.shape == C.shape
            C = R
        kw.update(R=R, ldr=c.ldr, res=N.RES_ADD if c.res == 1 else N.RES_MUL)
    if part:
        kw.update(part=(_Space(), "p"))
    if defer:
        return E.gemm(A, B, C, c.M, c.N, c.K, _defer=True, **kw), C, (A, B, kw)
    out = E.gemm(A, B, C, c.M, c.N, c.K, **kw)
    torch.cuda.synchronize()
    return shape_out(c, C), out


def shape_out(c, C):
    got = C.cpu().double()
    if c.t_rows:
        got = got.reshape(c.M // c.t_rows, c.t_tokens, c.t_rows)[:, :c.N]
    return got


def label(c, *more):
    return " ".join(str(v) for v in (c.pattern, str(c.dtype).replace("torch.", ""), "M=%d N=%d K=%d" % (c.M, c.N, c.K)) + more)


# ------------------------------------------------------------------------------------------------- the GELU premise, on the device
@pytest.mark.parametrize("dtype", X.STORAGE)
def test_gelu_is_the_identity_from_the_threshold_up_on_the_device(dtype):
    """mlpk_norm_apply with act = GELU and no statistics over the integers [threshold, 256]: the output equals the input.  Every fused
    case below relies on it; if it fails on hardware, this test says so first."""
    E, N = load_pkg().engine, load_pkg()._native
    vals = torch.arange(X.GELU_THRESHOLD, 257, dtype=torch.float64)
    C = 24
    rows = -(-vals.numel() // C)
    x = torch.full((rows * C,), 256.0, dtype=torch.float64)
    x[:vals.numel()] = vals
    x = put(x.reshape(rows, C), dtype)
    out = torch.full_like(x, float("nan"))
    E.norm_apply(x, rows, C, C, act=N.ACT_GELU, out_rm=out, ld_rm=C)
    torch.cuda.synchronize()
    X.assert_exact(out, x.cpu().double(), "gelu(x) == x, %s" % dtype)


# ------------------------------------------------------------------------------------------------- mlpk_gemm_nt, algos 1 .. 13
# (tests/test_exact_host.py::test_tile_table_is_the_librarys holds exact.TILES to mlpk_gemm_algo_info)
@pytest.mark.parametrize("dtype", X.STORAGE)
@pytest.mark.parametrize("algo", sorted(X.TILES))
def test_gemm_template_tiles(dtype, algo):
    """edge shapes (a single row, one short of / one past the tile, odd N = the scalar-store path), every K from one granule to two
    slabs past the pipeline depth, every epilogue (bias; column scale / shift; residual aliasing C; gate; periodic row scale; folded
    LayerNorm per row and per group; saturated GELU), token-transposed output on the direct and the LDS-staged path."""
    for (what, pat, M, N, K, kw) in X.template_cases(algo, dtype):
        c = X.gemm_case(pat, dtype, M, N, K, **kw)
        got, _ = run_gemm(c, algo)
        X.assert_exact(got, c.want, label(c, "algo", algo, what), K=K if pat == "onehot" else None, k_off=c.k_off, col_axis=-2 if c.t_rows else -1)


@pytest.mark.parametrize("dtype", X.SIXTEEN)
@pytest.mark.parametrize("algo", [a for a in sorted(X.TILES) if X.TILES[a][1] >= 128])
def test_gemm_template_tiles_row_statistics(dtype, algo):
    """row_part of the tiles that deliver it (128 columns or more): bit-equal to the integer sums of the stored values"""
    bm, bn, _ = X.TILES[algo]
    for pat in X.PATTERNS:
        for kw in (dict(res=1), dict(), dict(gelu=True)):
            c = X.gemm_case(pat, dtype, bm + 1, bn + 8, X.k_plain(algo, dtype), **kw)
            got, part = run_gemm(c, algo, part=True)
            assert part is not None
            X.assert_exact(got, c.want, label(c, "algo", algo, "stats"))
            X.assert_exact(part[0], X.row_part_want(c.want, part[1]), label(c, "algo", algo, "row_part"))


# ------------------------------------------------------------------------------------------------- algo 14, the persistent tile
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_gemm_persistent_tile(dtype):
    for (name, pat, M, N, K, bits, kw) in X.p8_cases():
        c = X.gemm_case(pat, dtype, M, N, K, **kw)
        got, _ = run_gemm(c, 14, dbg=bits)
        X.assert_exact(got, c.want, label(c, "algo 14", name, "bits", bits), K=K if pat == "onehot" else None, k_off=c.k_off)


@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_gemm_persistent_tile_row_statistics(dtype):
    """bias + residual is the persistent tile's statistics class (the direct epilogue, every height)"""
    for (M, N, nslab, bits) in [(64, 256, 2, 0), (320, 512, 3, 0), (448, 256, 5, 16), (192, 512, 8, 128)]:
        for pat in X.PATTERNS:
            c = X.gemm_case(pat, dtype, M, N, nslab * 64, res=1)
            got, part = run_gemm(c, 14, dbg=bits, part=True)
            assert part is not None
            X.assert_exact(got, c.want, label(c, "algo 14 stats"))
            X.assert_exact(part[0], X.row_part_want(c.want, part[1]), label(c, "algo 14 row_part"))


# ------------------------------------------------------------------------------------------------- algo 15, the generated tile
@pytest.mark.parametrize("dtype", X.SIXTEEN)
@pytest.mark.parametrize("K", X.Q4_K)
def test_gemm_generated_tile(dtype, K):
    """every M x N of the table at this K (the f4 / s6 / s12 variants with rolled and peeled iterations), every epilogue class of
    test_gemm_q4_generated_tile; the classes that deliver statistics (residual; GELU + folded LayerNorm) with row_part as well"""
    for (name, pat, M, N, K_, kw) in X.q4_cases(K):
        c = X.gemm_case(pat, dtype, M, N, K_, **kw)
        stats = name in ("res", "gelu_ln")
        got, part = run_gemm(c, 15, part=stats)
        X.assert_exact(got, c.want, label(c, "algo 15", name), K=K_ if pat == "onehot" else None, k_off=c.k_off)
        if stats:
            assert part is not None
            X.assert_exact(part[0], X.row_part_want(c.want, part[1]), label(c, "algo 15 row_part", name))


# ------------------------------------------------------------------------------------------------- algo 16, the skinny fp32 kernel
def test_gemm_skinny_fp32():
    for (M, N, K) in X.SKINNY_CASES:
        for pat in X.PATTERNS:
            for off in (X.onehot_offsets(N, K) if pat == "onehot" else [0]):
                for gelu in (False, True):
                    c = X.gemm_case(pat, torch.float32, M, N, K, gelu=gelu, k_off=off)
                    got, _ = run_gemm(c, 16)
                    X.assert_exact(got, c.want, label(c, "algo 16", "gelu" if gelu else ""), K=K if pat == "onehot" else None, k_off=off)


# ------------------------------------------------------------------------------------------------- mlpk_gemm_nt_pair
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_gemm_pair(dtype):
    """two products of different heights in one launch (the s3 tiles), each exact"""
    E, N = load_pkg().engine, load_pkg()._native
    for pair in X.PAIR_CASES:
        for pat in X.PATTERNS:
            cs = [X.gemm_case(pat, dtype, M, Nn, K, res=1, seed=5 + i) for i, (M, Nn, K) in enumerate(pair)]
            calls = [run_gemm(c, 0, defer=True) for c in cs]
            (d0, _), (d1, _) = calls[0][0], calls[1][0]
            N.check(N.lib().mlpk_gemm_nt_pair(ctypes.byref(d0), ctypes.byref(d1), E.stream()), "mlpk_gemm_nt_pair")
            torch.cuda.synchronize()
            for c, call in zip(cs, calls):
                X.assert_exact(shape_out(c, call[1]), c.want, label(c, "pair"))


# ------------------------------------------------------------------------------------------------- mlpk_conv_gemm_nhwc
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_conv_gemm_nhwc(dtype):
    """3 x 3 stride 2 pad 1 and 2 x 2 stride 2, 32 and 64 channels, maps 5 x 7 and 6 x 6: the one-hot weight names every (tap, channel);
    a tap outside the map gives exactly 0"""
    E = load_pkg().engine
    for geom in X.CONV_CASES:
        B, H, W, Cin, k, stride, pad = geom
        assert E.conv_gemm_nhwc_supported(dtype, Cin, k, k, stride, pad)
        for pat in X.PATTERNS:
            c = X.conv_case(pat, dtype, *geom)
            X.check_conv_case(c)
            x = put(c.x.reshape(B * H * W, Cin), dtype)
            w = put(c.w, dtype)
            out = torch.full((c.A.shape[0], c.N), float("nan"), dtype=dtype, device=dev())
            part = E.conv_gemm_nhwc(x, w, out, B, H, W, Cin, k, k, stride, pad, bias=put(c.bias, torch.float32), part=(_Space(), "p"))
            torch.cuda.synchronize()
            what = "conv %s %s %s" % (pat, dtype, geom)
            X.assert_exact(out, c.want, what, K=c.K if pat == "onehot" else None)      # (k = tap * Cin + channel)
            assert part is not None                                                  # the 128 x 128 s3 tile, N % 8 == 0: statistics are delivered
            X.assert_exact(part[0], X.row_part_want(c.want, part[1]), what + " row_part")


# ------------------------------------------------------------------------------------------------- mlpk_token_gemm, _ln, _ln_post
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_token_gemm(dtype):
    """S = 16 / 49 / 196 (196: the pipelined kernel), 32 and 96 channels per image; gate, residual in place with a per-channel scale,
    the LayerNorm / Aff operand loader, the affine residual rebuilt in the kernel, the post affine"""
    E, N = load_pkg().engine, load_pkg()._native
    f = torch.float32
    for (nimg, C, S, variant, kw) in X.token_gemm_cases():
        for pat in X.PATTERNS:
            c = X.token_case(pat, dtype, nimg, C, S, variant, **kw)
            X.check_token_case(c)
            wp, bp, ng = E.pack_token_gemm(c.B.float(), c.bias.float(), dtype, dev())
            rows = nimg * S
            opt = {}
            if c.rscale is not None:
                opt.update(rscale=put(c.rscale, f), rperiod=c.rperiod)
            out = torch.full((rows, C), float("nan"), dtype=dtype, device=dev())
            if c.res:
                R = put(c.R, dtype)
                if c.r_alias:
                    out = R
                opt.update(R=R, ldr=c.ldr, res=N.RES_ADD if c.res == 1 else N.RES_MUL)
            if variant == "plain":
                sp = E.round_up(S, 32)
                xt = torch.zeros((nimg * C, sp), dtype=dtype, device=dev())
                xt[:, :S] = put(c.A, dtype)
                E.token_gemm(xt, sp, nimg * C, S, wp, bp, ng, out, C, C, **opt)
            else:
                x = put(c.x, dtype)
                if variant in ("affine_res", "post"):
                    out = x                                                   # in place: the residual is rebuilt from x
                    opt.update(R=x, ldr=C, res=N.RES_ADD_AFFINE)
                if variant == "post":
                    assert E.token_gemm_ln_post_supported(dtype, S, C, C)
                    opt.update(post=(put(c.post[0], f), put(c.post[1], f)))
                E.token_gemm_ln(x, C, nimg * C, S, put(c.mean, f), put(c.rstd, f), put(c.gamma, f), put(c.beta, f), wp, bp, ng, out, C, C, **opt)
            torch.cuda.synchronize()
            X.assert_exact(out.cpu().double().reshape(nimg, S, C), c.want, "token_gemm %s %s %s C=%d S=%d %s" % (variant, pat, dtype, C, S, kw),
                           K=S if pat == "onehot" else None, col_axis=-2)


# ------------------------------------------------------------------------------------------------- mlpk_patch_embed4, mlpk_stem7
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_patch_embed4_without_layernorm(dtype):
    """C = 32 and 128, the smallest image and a larger one; the weight goes through engine.pack_matrix"""
    E = load_pkg().engine
    for C in X.EMBED_C:
        for (B, H, W) in X.EMBED4_CASES:
            for pat in X.PATTERNS:
                for off in X.pattern_offsets(pat, C, 48):
                    c = X.gemm_case(pat, dtype, B * (H // 4) * (W // 4), C, 48, k_off=off, slab=16)
                    X.check_case(c)
                    out = torch.full((c.M, C), float("nan"), dtype=dtype, device=dev())
                    E.patch_embed4(put(X.embed4_image(c, B, H, W), dtype), E.pack_matrix(c.B.reshape(C, 3, 4, 4).float(), dtype, dev()), put(c.bias, torch.float32),
                                   out, B, H, W, C)
                    torch.cuda.synchronize()
                    X.assert_exact(out, c.want, "patch_embed4 %s %s C=%d %s" % (pat, dtype, C, (B, H, W)), K=48 if pat == "onehot" else None, k_off=off)


@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_stem7_without_statistics(dtype):
    """pad 3 and pad 2, C = 32 and 128, the smallest image and a larger one; the weight goes through engine.pack_stem7"""
    E = load_pkg().engine
    for C in X.EMBED_C:
        for (B, H, W, pad) in X.STEM7_CASES:
            for pat in X.PATTERNS:
                for off in X.pattern_offsets(pat, C, 147):
                    c = X.stem7_case(pat, dtype, B, H, W, pad, C, k_off=off)
                    X.check_stem7_case(c)
                    out = torch.full((c.want.shape[0], C), float("nan"), dtype=dtype, device=dev())
                    E.stem7(put(c.x, dtype), E.pack_stem7(c.w.reshape(C, 3, 7, 7).float(), dtype, dev()), put(c.bias, torch.float32), out, B, H, W, pad, C)
                    torch.cuda.synchronize()
                    X.assert_exact(out, c.want, "stem7 %s %s C=%d %s" % (pat, dtype, C, (B, H, W, pad)), K=147 if pat == "onehot" else None, k_off=off)


# ------------------------------------------------------------------------------------------------- mlpk_channel_mlp
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_channel_mlp(dtype):
    """C = 64 / 96 / 192, M = 257 / 511 (a partial last tile), with and without the folded norm (per row and per group of 64 rows),
    out aliasing x and R; the GELU saturated to the identity; row_part bit-equal to the integer sums of the stored values.  The
    weights go through engine.pack_channel_mlp_fused (the column and row orders of W2 are under test)."""
    E = load_pkg().engine
    f = torch.float32
    for (C, M, norm, res) in X.CHANNEL_MLP_CASES:
        assert E.channel_mlp_fused_supported(dtype, C, 4 * C)
        for pat in X.PATTERNS:
            for (o1, o2) in X.mlp_offsets(pat, C, 4 * C, C):
                c = X.mlp_case(pat, dtype, M, C, 4 * C, C, norm=norm, off1=o1, off2=o2)
                g = torch.Generator().manual_seed(3)
                other = torch.randint(-4, 5, (M, C), generator=g).double()
                Rw = c.A if res == "x" else other if res == "other" else None
                X.check_mlp_case(c, residual=Rw)
                pack = E.pack_channel_mlp_fused(c.w1.float(), c.b1.float(), c.w2.float(), c.b2.float(), dtype, dev(),
                                                c.gamma.float() if norm else None, c.beta.float() if norm else None)
                x = put(c.A, dtype)
                out = x if res == "x" else torch.full((M, C), float("nan"), dtype=dtype, device=dev())
                R = x if res == "x" else put(other, dtype) if res == "other" else None
                part = E.channel_mlp_fused(x, M, C, pack, out, R=R, ln=(put(c.mean, f), put(c.rstd, f)) if norm else None, ln_group=norm or 1, part=(_Space(), "p"))
                torch.cuda.synchronize()
                want = c.core if Rw is None else c.core + Rw
                what = "channel_mlp %s %s C=%d M=%d norm=%d res=%s" % (pat, dtype, C, M, norm, res)
                X.assert_exact(out, want, what, K=4 * C if pat == "onehot" else None, k_off=o2)       # (k = the hidden unit)
                X.assert_exact(part[0], torch.stack([want.sum(1), (want * want).sum(1)], 1)[None], what + " row_part")


# ------------------------------------------------------------------------------------------------- mlpk_token_mlp, mlpk_token_mlp_ln
def run_token_mlp(E, c, dtype, nimg, C, S, layout, t_rows=None, stats=False):
    sp = E.round_up(S, 32)
    w1p, b1p, w2p, b2p, nch, lay = E.pack_token_mlp(c.w1.float(), c.b1.float(), c.w2.float(), c.b2.float(), dtype, dev(), sp, layout=layout, t_rows=t_rows)
    return sp, (w1p, b1p, w2p, b2p, nch), lay


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_token_mlp(dtype, layout):
    """layouts 0 / 1: S = 16 / 49 / 196, one and three hidden chunks (the hidden 4 short of whole chunks), rows spanning two images and
    a partial last tile; W2 goes through engine.pack_token_mlp's column order"""
    E = load_pkg().engine
    for (nimg, C, S, nch) in X.TOKEN_MLP_CASES:
        T = nch * 32 - 4
        for pat in X.PATTERNS:
            for (o1, o2) in X.mlp_offsets(pat, S, T, S):
                c = X.mlp_case(pat, dtype, nimg * C, S, T, S, off1=o1, off2=o2)
                x0, want = X.token_mlp_residual(c, nimg, C, S)
                X.check_mlp_case(c, residual=want.permute(0, 2, 1).reshape(nimg * C, S) - c.core)
                sp, (w1p, b1p, w2p, b2p, n), lay = run_token_mlp(E, c, dtype, nimg, C, S, layout)
                assert lay == layout and n == nch
                xt = torch.zeros((nimg * C, sp), dtype=dtype, device=dev())
                xt[:, :S] = put(c.A, dtype)
                x = put(x0, dtype)
                E.token_mlp(xt, sp, nimg * C, S, w1p, b1p, w2p, b2p, n, x, C, C, layout=lay)
                torch.cuda.synchronize()
                X.assert_exact(x.cpu().double().reshape(nimg, S, C), want, "token_mlp layout %d %s %s C=%d S=%d nch=%d" % (layout, pat, dtype, C, S, nch),
                               K=T if pat == "onehot" else None, k_off=o2, col_axis=-2)


@pytest.mark.parametrize("nch", X.TOKEN_MLP_T4_NCH)
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_token_mlp_generated_kernel_and_prenorm(dtype, nch):
    """layouts 2 / 3 (bf16: the hidden kept in f16) and mlpk_token_mlp_ln: S = 196, 256 channels per image, two images, 2 / 3 / 28 hidden
    chunks; `stats` bit-equal to the integer sums of the stored values over planes of 64 channels"""
    E = load_pkg().engine
    f = torch.float32
    nimg, C, S = 2, 256, 196
    T = nch * 32 - 4
    for pat in X.PATTERNS:
        for (o1, o2) in X.mlp_offsets(pat, S, T, S):
            c = X.mlp_case(pat, dtype, nimg * C, S, T, S, off1=o1, off2=o2)
            sp, (w1p, b1p, w2p, b2p, n), lay = run_token_mlp(E, c, dtype, nimg, C, S, None, t_rows=C)
            assert lay == (3 if dtype == torch.bfloat16 else 2) and n == nch
            hdt = torch.float16 if lay == 3 else None
            what = "layout %d %s %s nch=%d" % (lay, pat, dtype, nch)
            planes = E.token_mlp_stat_planes(C, lay)
            # mlpk_token_mlp on the transposed operand
            x0, want = X.token_mlp_residual(c, nimg, C, S)
            X.check_mlp_case(c, hidden_dtype=hdt, residual=want.permute(0, 2, 1).reshape(nimg * C, S) - c.core)
            xt = torch.zeros((nimg * C, sp), dtype=dtype, device=dev())
            xt[:, :S] = put(c.A, dtype)
            x = put(x0, dtype)
            part = torch.full((planes, nimg * S, 2), float("nan"), dtype=f, device=dev())
            E.token_mlp(xt, sp, nimg * C, S, w1p, b1p, w2p, b2p, n, x, C, C, stats=part, layout=lay)
            torch.cuda.synchronize()
            X.assert_exact(x.cpu().double().reshape(nimg, S, C), want, "token_mlp " + what, K=T if pat == "onehot" else None, k_off=o2, col_axis=-2)
            X.assert_exact(part, X.token_stats_want(want.reshape(nimg * S, C), planes), "token_mlp stats " + what)
            # mlpk_token_mlp_ln: the LayerNorm as the operand loader, x updated in place
            xl, mean, rstd, gamma, beta, want = X.token_mlp_ln_inputs(c, nimg, C, S)
            assert X.representable(xl, dtype)
            X.check_mlp_case(c, hidden_dtype=hdt, residual=want.permute(0, 2, 1).reshape(nimg * C, S) - c.core)
            x = put(xl, dtype)
            part = torch.full((planes, nimg * S, 2), float("nan"), dtype=f, device=dev())
            E.token_mlp_ln(x, C, nimg * C, S, put(mean, f), put(rstd, f), put(gamma, f), put(beta, f), w1p, b1p, w2p, b2p, n, C, stats=part, layout=lay)
            torch.cuda.synchronize()
            X.assert_exact(x.cpu().double().reshape(nimg, S, C), want, "token_mlp_ln " + what, K=T if pat == "onehot" else None, k_off=o2, col_axis=-2)
            X.assert_exact(part, X.token_stats_want(want.reshape(nimg * S, C), planes), "token_mlp_ln stats " + what)


# ------------------------------------------------------------------------------------------------- mlpk_dwconv_nhwc: every form, tile and launch plan
DW_GROUPS = ("mfma", "mfma_full", "lds", "direct")           # a geometry's group is the form its 16-bit run takes (exact.dwconv_form)
DW_ENULL, DW_ESHAPE, DW_EDTYPE = -4, -2, -1                  # include/mlpk.h


def run_dwconv(c, x_off=0):
    """one mlpk_dwconv_nhwc call for an exact.dwconv_case into a NaN-filled out; x_off: x starts that many elements into its buffer"""
    E = load_pkg().engine
    f = torch.float32
    B, H, W, C, k = c.geom
    x = put(c.x, c.dtype)
    if x_off:
        buf = torch.zeros(x.numel() + x_off, dtype=c.dtype, device=dev())
        buf[x_off:] = x.reshape(-1)
        x = buf[x_off:].view(B, H, W, C)
        assert x.data_ptr() % 16 == (x_off * x.element_size()) % 16 != 0
    out = torch.full((B, H, W, C), float("nan"), dtype=c.dtype, device=dev())
    E.dwconv_nhwc(x, out, B, H, W, C, k, put(c.w, f), put(c.bias, f), put(c.bns, f), put(c.bnh, f))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", X.STORAGE)
@pytest.mark.parametrize("group", DW_GROUPS)
def test_dwconv_matrix_core(dtype, group):
    """exact.DWCONV_TABLE: the matrix-core form (both instantiations, k = 3 / 5 / 7 / 9, all four 16 x 16 blocks, the store's tail, several
    image ranges, the re-deal over the XCDs, degenerate maps), the LDS-tiled and the generic form, in all three storage types (fp32 runs
    the LDS-tiled or the generic kernel on the same geometries).  Saturated GELU; the one-hot taps name (tap, channel); zero differing
    elements is the gate."""
    n = 0
    for geom in X.DWCONV_CASES:
        B, H, W, C, k = geom
        if X.dwconv_form(torch.bfloat16, H, W, C, k) != group:
            continue
        for pat in X.dwconv_patterns(dtype, geom):
            for off in X.dwconv_offsets(pat, C, k):
                c = X.dwconv_case(pat, dtype, *geom, off=off)
                X.check_dwconv_case(c)
                X.assert_exact(run_dwconv(c), c.want, "dwconv %s %s %s" % (pat, dtype, geom), K=k * k if pat == "onehot" else None, k_off=off)
                n += 1
    assert n > 0
    if group == "direct" and dtype != torch.float32:          # the fourth way to the generic kernel: x off a 16-byte boundary
        geom, x_off = X.DWCONV_OFFSET_CASE
        for pat in X.dwconv_patterns(dtype, geom):
            c = X.dwconv_case(pat, dtype, *geom)
            X.check_dwconv_case(c)
            X.assert_exact(run_dwconv(c, x_off), c.want, "dwconv %s %s %s x + %d" % (pat, dtype, geom, x_off), K=geom[4] ** 2 if pat == "onehot" else None)


@pytest.mark.parametrize("dtype", X.SIXTEEN)
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_dwconv_every_tap_in_every_channel_slot(dtype, k):
    """one-hot with every offset on (3, 8, 8, 32, k): each channel slot of each wave meets each of the k k taps, the fragments held in
    registers (tf[j][i]) and those read from the LDS table alike -- the table's own sweep gives a channel 1 .. 3 of them"""
    geom = [g for g in X.DWCONV_SWEEP if g[4] == k][0]
    assert X.dwconv_form(dtype, *geom[1:]) == "mfma"
    for off in X.dwconv_offsets("onehot", geom[3], k, full=True):
        c = X.dwconv_case("onehot", dtype, *geom, off=off)
        X.check_dwconv_case(c)
        X.assert_exact(run_dwconv(c), c.want, "dwconv tap sweep %s %s off %d" % (dtype, geom, off), K=k * k, k_off=off)


def _dw_gaussian(dtype, geom, seed):
    B, H, W, C, k = geom
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, C), generator=g).to(dtype).to(dev())
    w = (torch.randn((k * k, C), generator=g) / k).to(dev())
    bias, bns, bnh = torch.randn((C,), generator=g).to(dev()), (torch.randn((C,), generator=g) * 0.2 + 1).to(dev()), torch.randn((C,), generator=g).to(dev())
    return x, w, bias, bns, bnh


@pytest.mark.parametrize("dtype", X.STORAGE)
def test_dwconv_image_does_not_depend_on_its_batch(dtype):
    """Gaussian data, all three forms, batches that span several image ranges and the re-deal: image b of the batch is bit-equal to the
    same image run alone (B = 1: one range, no prefetch, the plain workgroup order)"""
    E = load_pkg().engine
    for geom in X.DWCONV_BATCH:
        B, H, W, C, k = geom
        x, w, bias, bns, bnh = _dw_gaussian(dtype, geom, 41)
        out = torch.full_like(x, float("nan"))
        E.dwconv_nhwc(x, out, B, H, W, C, k, w, bias, bns, bnh)
        alone = torch.full_like(x, float("nan"))
        for b in range(B):
            E.dwconv_nhwc(x[b], alone[b], 1, H, W, C, k, w, bias, bns, bnh)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        X.assert_exact(out, alone.cpu().double(), "dwconv batch %s %s: (image, y, x, channel)" % (dtype, geom))


@pytest.mark.parametrize("dtype", X.STORAGE)
def test_dwconv_null_epilogue_vectors(dtype):
    """bias / bn_scale / bn_shift NULL mean 0 / 1 / 0 in all three kernels: bit-equal to explicit vectors, one geometry per form"""
    E = load_pkg().engine
    forms = set()
    for geom in [(2, 19, 17, 40, 7), (3, 32, 32, 32, 9), (2, 9, 37, 40, 5), (2, 7, 9, 66, 3)]:
        B, H, W, C, k = geom
        assert geom in X.DWCONV_CASES
        forms.add(X.dwconv_form(dtype, H, W, C, k))
        x, w, bias, bns, bnh = _dw_gaussian(dtype, geom, 43)
        zero, one = torch.zeros_like(bias), torch.ones_like(bias)
        for null in range(1, 8):                             # every non-empty subset of the three
            given = [None if null & 1 else bias, None if null & 2 else bns, None if null & 4 else bnh]
            explicit = [zero if null & 1 else bias, one if null & 2 else bns, zero if null & 4 else bnh]
            got, want = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            E.dwconv_nhwc(x, got, B, H, W, C, k, w, *given)
            E.dwconv_nhwc(x, want, B, H, W, C, k, w, *explicit)
            torch.cuda.synchronize()
            assert torch.isfinite(want).all()
            X.assert_exact(got, want.cpu().double(), "dwconv NULL mask %d %s %s" % (null, dtype, geom))
    assert forms == ({"lds", "direct"} if dtype == torch.float32 else {"mfma", "mfma_full", "lds", "direct"})


def test_dwconv_refusals():
    """every documented refusal returns its code before anything is launched: the NaN-filled output stays NaN.  Small = a map of at most
    32 x 32 with C % 8 == 0 (the matrix-core branch in 16 bits), large = 40 x 40."""
    E, N = load_pkg().engine, load_pkg()._native
    L, s = N.lib(), E.stream()
    w = torch.ones((15 * 15, 8), device=dev())
    vec = torch.ones((8,), device=dev())
    cases = []
    for name, (H, W) in (("small", (8, 8)), ("large", (40, 40))):
        for dt, code in ((torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2)):
            x = torch.ones((1, H, W, 8), dtype=dt, device=dev())
            out = torch.full_like(x, float("nan"))

            def args(k=3, xx=x, oo=out, ww=w, cc=code, H=H, W=W):
                return (cc, E.ptr(xx), E.ptr(oo), 1, H, W, 8, k, E.ptr(ww), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), s)
            cases +=[("%s %s x NULL" % (name, dt), DW_ENULL, args(xx=None), out), ("%s %s out NULL" % (name, dt), DW_ENULL, args(oo=None), out),
                      ("%s %s w NULL" % (name, dt), DW_ENULL, args(ww=None), out), ("%s %s x == out" % (name, dt), DW_ESHAPE, args(xx=out), out)]
            cases += [("%s %s k = %d" % (name, dt, k), DW_ESHAPE, args(k=k), out) for k in (0, 2, 4, 15)]
            if dt == torch.bfloat16:                         # (a 16-bit buffer: what an unknown code was once taken for)
                cases += [("%s dtype %d" % (name, bad), DW_EDTYPE, args(cc=bad), out) for bad in (3, -1)]
    for what, want, a, out in cases:
        rc = L.mlpk_dwconv_nhwc(*a)
        torch.cuda.synchronize()
        assert rc == want, (what, rc, want)
        assert torch.isnan(out).all(), (what, "the output was written")
    # (the wrapper raises on any of them)
    with pytest.raises(N.MlpkError):
        E.dwconv_nhwc(out, out, 1, 40, 40, 8, 3, w, vec, vec, vec)


# ------------------------------------------------------------------------------------------------- mlpk_vip_branch
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_vip_branch(dtype):
    """both branches, K = 128 / 256 / 384, with `sums` bit-equal to the integer sums of the normalised operand"""
    E = load_pkg().engine
    f = torch.float32
    for geom in X.VIP_CASES:
        B, H, W, C, seg = geom
        assert E.vip_branch_supported(dtype, H, W, C, seg)
        for which in (0, 1):
            O = W if which == 0 else H
            for pat in X.PATTERNS:
                c = X.vip_case(pat, dtype, *geom, which)
                X.check_vip_case(c)
                z = torch.full((c.M, c.N), float("nan"), dtype=dtype, device=dev())
                sums = torch.full((B * (C // seg), O * seg), float("nan"), dtype=f, device=dev())
                E.vip_branch(which, put(c.x, dtype), C, B, H, W, C, seg, put(c.mean, f), put(c.rstd, f), put(c.gamma, f), put(c.beta, f),
                             put(c.B, dtype), put(c.bias, f), z, c.N, sums=sums, ld_sum=O * seg)
                torch.cuda.synchronize()
                what = "vip_branch %d %s %s %s" % (which, pat, dtype, geom)
                X.assert_exact(z, c.want, what, K=c.K if pat == "onehot" else None)
                X.assert_exact(sums, c.sums, what + " sums")


# ------------------------------------------------------------------------------------------------- mlpk_smlp_mix, mlpk_smlp_mix_dw
@pytest.mark.parametrize("dw", [False, True])
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_smlp_mix(dtype, dw):
    """maps 7 x 7 and 14 x 14, C = 32 and 64; with the depthwise sublayer in front the intermediate x' is held exact as well"""
    E = load_pkg().engine
    f = torch.float32
    for geom in X.SMLP_CASES:
        B, H, W, C = geom
        assert (E.smlp_mix_dw_supported if dw else E.smlp_mix_supported)(dtype, H, W, C)
        for pat in X.PATTERNS:
            c = X.smlp_case(pat, dtype, *geom, dw=dw)
            X.check_smlp_case(c)
            rows = B * H * W
            whp, bhp = E.pack_smlp_mix(c.wh.float(), c.bh.float(), dtype, dev())
            wwp, bwp = E.pack_smlp_mix(c.ww.float(), c.bw.float(), dtype, dev())
            x = put(c.x.reshape(rows, C), dtype)
            out = torch.full((rows, 3 * C), float("nan"), dtype=dtype, device=dev())
            what = "smlp_mix%s %s %s %s" % ("_dw" if dw else "", pat, dtype, geom)
            if dw:
                xres = torch.full((rows, C), float("nan"), dtype=dtype, device=dev())
                E.smlp_mix_dw(x, C, B, H, W, C, put(c.dw_w, f), put(c.dw_b, f), put(c.dw_s, f), put(c.dw_h, f), xres, C, put(c.bn_s, f), put(c.bn_h, f),
                              whp, bhp, wwp, bwp, out, 3 * C)
                torch.cuda.synchronize()
                X.assert_exact(xres, c.xres.reshape(rows, C), what + " x'")
            else:
                E.smlp_mix(x, C, B, H, W, C, put(c.bn_s, f), put(c.bn_h, f), whp, bhp, wwp, bwp, out, 3 * C)
                torch.cuda.synchronize()
            X.assert_exact(out, c.want, what)


# ------------------------------------------------------------------------------------------------- mlpk_as_conv2, mlpk_as_conv2_stats
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_as_conv2(dtype):
    """C = 96 / 192, maps 7 x 7 and 14 x 9, mean 0, rstd 1, t >= the threshold: all GELUs are the identity, and the zero halo of both
    shifts contributes exactly the bias; the statistics variant must store the same values"""
    E = load_pkg().engine
    f = torch.float32
    for geom in X.ASCONV_CASES:
        B, H, W, C = geom
        assert E.as_conv2_supported(dtype, H, W, C, 5)
        for pat in X.PATTERNS:
            c = X.asconv_case(pat, dtype, *geom)
            X.check_asconv_case(c)
            rows = B * H * W
            t = put(c.t, dtype)
            mean, rstd = torch.zeros(B, dtype=f, device=dev()), torch.ones(B, dtype=f, device=dev())
            gamma, beta = torch.ones(C, dtype=f, device=dev()), torch.zeros(C, dtype=f, device=dev())
            args = (B, H, W, C, 5, mean, rstd, gamma, beta, put(c.w1, dtype), put(c.b1, f), put(c.w2, dtype), put(c.b2, f))
            y = torch.full((rows, C), float("nan"), dtype=dtype, device=dev())
            E.as_conv2(t, y, *args)
            y2 = torch.full((rows, C), float("nan"), dtype=dtype, device=dev())
            E.as_conv2(t, y2, *args, stats=(E.Workspace(dev(), dtype), "asc"))
            torch.cuda.synchronize()
            what = "as_conv2 %s %s %s" % (pat, dtype, geom)
            X.assert_exact(y, c.want, what, K=C if pat == "onehot" else None, k_off=1)
            X.assert_exact(y2, c.want, what + " (statistics variant)")


# ------------------------------------------------------------------------------------------------- mlpk_swin_spatial
@pytest.mark.parametrize("quad", ["1", "0"])
@pytest.mark.parametrize("dtype", X.SIXTEEN)
def test_swin_spatial(dtype, quad, monkeypatch):
    """(window, heads) = (4, 1), (5, 2), (7, 3), (7, 24), (8, 1); shifted and unshifted padding; maps that are not whole windows; both
    values of MLPK_SWIN_SPATIAL_Q.  The cancel pattern runs on the maps of whole, unshifted windows only (exact.swin_cancel_possible
    says why); the weights go through engine.pack_swin_spatial."""
    E = load_pkg().engine
    f = torch.float32
    monkeypatch.setenv("MLPK_SWIN_SPATIAL_Q", quad)
    for geom in X.SWIN_CASES:
        B, H, W, heads, ws, shift = geom
        C, T = heads * 32, ws * ws
        assert E.swin_spatial_supported(dtype, C, heads, ws)
        pad_t, pad_l, Hp, Wp = X.swin_geometry(H, W, ws, shift)
        for pat in X.PATTERNS:
            if pat == "cancel" and not X.swin_cancel_possible(H, W, ws, shift):
                continue
            c = X.swin_case(pat, dtype, *geom)
            X.check_swin_case(c)
            wp, bp = E.pack_swin_spatial(c.wd.reshape(heads * T, T, 1).float(), c.bias.float(), heads, ws, dtype, dev())
            x = put(c.x, dtype)
            E.swin_spatial(x, B, H, W, C, ws, pad_t, pad_l, Hp, Wp, heads, put(c.mean, f), put(c.rstd, f), put(c.gamma, f), put(c.beta, f), wp, bp)
            torch.cuda.synchronize()
            X.assert_exact(x, c.want, "swin_spatial Q=%s %s %s %s" % (quad, pat, dtype, geom))
