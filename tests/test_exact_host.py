"""The exact-integer oracle (tests/exact.py) checked on the CPU: its premises for every case table the GPU file uses, the GELU
threshold from emulations of the three forms of csrc/mlpk_common.h, and a numpy model of a tiled GEMM with planted faults -- which
pattern catches which fault, and that the Gaussian gate of tests/test_gpu_ops.py lets the two precision faults pass.  For the depthwise
convolution: what its geometry table reaches (a restatement of the dispatcher of csrc/mlpk_dwconv.hip), that no row can go, that the
re-deal of its workgroups is a permutation, and planted faults of the matrix-core form that the earlier three-row table did not see."""
import math

import numpy as np
import pytest
import torch

import exact as X


# ------------------------------------------------------------------------------------------------- GELU as the identity
def test_gelu_is_the_identity_on_integers_from_the_threshold_up():
    """For each form, the smallest integer t such that gelu(x) rounded to the storage type is x for every integer x in [t, 256];
    exact.GELU_THRESHOLD must serve all three, with room for the device's 1-ulp reciprocal and exponential in the fp32 form."""
    xs = np.arange(1, 257, dtype=np.float32)

    def first_from(ok):
        bad = np.nonzero(~ok)[0]
        return 1 if bad.size == 0 else int(xs[bad[-1]]) + 1
    g32, pe = X.gelu_f32_emulated(xs)
    t32 = first_from(g32 == xs)
    g16 = torch.from_numpy(X.gelu_f16_emulated(xs)).to(torch.float16).float().numpy()
    t16 = first_from(g16 == xs)
    gb, phi = X.gelu_bf16_emulated(xs)
    tb = first_from(torch.from_numpy(gb).to(torch.bfloat16).float().numpy() == xs)
    assert max(t32, t16, tb) <= X.GELU_THRESHOLD, (t32, t16, tb)
    sel = xs >= X.GELU_THRESHOLD
    assert (phi[sel] == 1.0).all()                          # bf16: Phi clamps to exactly 1, so the product is x before any rounding
    assert (gb[sel] == xs[sel]).all()
    assert (g32[sel] == xs[sel]).all() and pe[sel].max() < 2.0 ** -30          # fp32: 1 - p e rounds to 1 with a factor 32 to spare
    rel = np.abs(X.gelu_f16_emulated(xs)[sel].astype(np.float64) / xs[sel] - 1.0)
    assert rel.max() < 2.0 ** -13                           # f16: x (1 - 3.4e-6), a quarter of half an ulp of f16 at the worst
    # the negative side is NOT zero in the f16 form: exact cases must stay on the positive side
    assert X.gelu_f16_emulated(np.float32([-16.0]))[0] != 0.0
    for dt in X.STORAGE:
        assert X.GELU_OFFSET[dt] - 124 >= X.GELU_THRESHOLD and X.GELU_OFFSET[dt] + 124 <= 256


# ------------------------------------------------------------------------------------------------- premises of every table
def test_tile_table_is_the_librarys():
    import ctypes
    from conftest import load_pkg
    lib = load_pkg()._native.lib()
    for algo, (bm, bn, _) in X.TILES.items():
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.mlpk_gemm_algo_info(algo, ctypes.byref(a), ctypes.byref(b), None, None) == 0
        assert (a.value, b.value) == (bm, bn), algo


@pytest.mark.parametrize("algo", sorted(X.TILES))
def test_premises_of_the_template_tile_cases(algo):
    seen = set()
    for dtype in X.STORAGE:
        for (label, pat, M, N, K, kw) in X.template_cases(algo, dtype):
            c = X.gemm_case(pat, dtype, M, N, K, **kw)
            X.check_case(c)
            seen.add((label.split(":")[0], pat))
        assert K % X.granule_of(algo, dtype) == 0
        ks = X.k_sweep(algo, dtype)
        assert ks[0] == X.granule_of(algo, dtype) and ks[-1] == 4 * 8 * X.epc_of(dtype) and len(set(np.diff(ks))) <= 1
    assert seen == {(l, p) for l in ("edge", "ksweep", "epi", "token_t") for p in X.PATTERNS}


def test_premises_of_the_persistent_tile_cases():
    combos = set()
    for (name, pat, M, N, K, bits, kw) in X.p8_cases():
        for dtype in X.SIXTEEN:
            X.check_case(X.gemm_case(pat, dtype, M, N, K, **kw))
        combos.add((M, N, bits))
        assert M % 64 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 128
    assert {m for m, _, _ in combos} == set(X.P8_HEIGHTS) and {b for _, _, b in combos} == set(X.P8_BITS)
    assert {(K // 64, name) for (name, _, M, N, K, bits, _) in X.p8_cases()} >= {(s, e) for s in X.P8_SLABS for e in X.P8_EPILOGUES}


@pytest.mark.parametrize("K", X.Q4_K)
def test_premises_of_the_generated_tile_cases(K):
    n = 0
    for (name, pat, M, N, K_, kw) in X.q4_cases(K):
        for dtype in X.SIXTEEN:
            X.check_case(X.gemm_case(pat, dtype, M, N, K_, **kw))
        n += 1
    assert n >= len(X.Q4_M) * len(X.Q4_N) * len(X.Q4_EPILOGUES) * 3


def test_premises_of_the_other_gemm_tables():
    for (M, N, K) in X.SKINNY_CASES:
        for pat in X.PATTERNS:
            for off in (X.onehot_offsets(N, K) if pat == "onehot" else [0]):
                for gelu in (False, True):
                    X.check_case(X.gemm_case(pat, torch.float32, M, N, K, gelu=gelu, k_off=off))
    for pair in X.PAIR_CASES:
        for (M, N, K) in pair:
            for pat in X.PATTERNS:
                for dtype in X.SIXTEEN:
                    X.check_case(X.gemm_case(pat, dtype, M, N, K, res=1))
    for dtype in X.SIXTEEN:
        for case in X.token_gemm_cases():
            for pat in X.PATTERNS:
                X.check_token_case(X.token_case(pat, dtype, *case[:-1], **case[-1]))
        for case in X.CONV_CASES:
            for pat in X.PATTERNS:
                X.check_conv_case(X.conv_case(pat, dtype, *case))


def test_premises_of_the_embedding_cases():
    from conftest import load_pkg
    E = load_pkg().engine
    for dtype in X.SIXTEEN:
        for C in X.EMBED_C:
            first = [(H, W) for H in range(1, 9) for W in range(1, 9) if E.patch_embed4_supported(dtype, dtype, 3, H, W, C)][0]
            assert first == X.EMBED4_CASES[0][1:]
            for pad in (3, 2):
                first = [(H, W) for H in range(1, 9) for W in range(1, 17) if E.stem7_supported(dtype, dtype, 3, H, W, pad, C)][0]
                assert (first + (pad,)) in [g[1:] for g in X.STEM7_CASES]
            for (B, H, W) in X.EMBED4_CASES:
                assert E.patch_embed4_supported(dtype, dtype, 3, H, W, C)
                for pat in X.PATTERNS:
                    for off in X.pattern_offsets(pat, C, 48):
                        c = X.gemm_case(pat, dtype, B * (H // 4) * (W // 4), C, 48, k_off=off, slab=16)
                        X.check_case(c)
                        x = X.embed4_image(c, B, H, W)
                        assert torch.equal(torch.nn.functional.unfold(x, 4, stride=4).transpose(1, 2).reshape(-1, 48), c.A)
            for (B, H, W, pad) in X.STEM7_CASES:
                assert E.stem7_supported(dtype, dtype, 3, H, W, pad, C)
                for pat in X.PATTERNS:
                    for off in X.pattern_offsets(pat, C, 147):
                        X.check_stem7_case(X.stem7_case(pat, dtype, B, H, W, pad, C, k_off=off))


def test_premises_of_the_fused_kernel_cases():
    """mlpk_channel_mlp, mlpk_token_mlp / _ln (all layouts), mlpk_dwconv_nhwc, mlpk_vip_branch, mlpk_smlp_mix / _dw, mlpk_as_conv2,
    mlpk_swin_spatial: the tables tests/test_gpu_exact.py runs; and the packed-f16 GELU of the token kernel's bf16 grade (layout 3)
    is the identity from the threshold up as well"""
    import os
    import sys
    sys.path.insert(0, os.path.join(X.ROOT, "jittor-mlp_amd", "csrc", "gen"))
    import t4emu
    xs = np.arange(X.GELU_THRESHOLD, 257, dtype=np.float32)
    assert (t4emu.h2_gelu_ref(xs) == xs).all()
    for dtype in X.SIXTEEN:
        for (C, M, norm, res) in X.CHANNEL_MLP_CASES:
            for pat in X.PATTERNS:
                for (o1, o2) in X.mlp_offsets(pat, C, 4 * C, C):
                    c = X.mlp_case(pat, dtype, M, C, 4 * C, C, norm=norm, off1=o1, off2=o2)
                    X.check_mlp_case(c, residual=c.A if res == "x" else None)
        for (nimg, C, S, nch) in X.TOKEN_MLP_CASES + [(2, 256, 196, n) for n in X.TOKEN_MLP_T4_NCH]:
            T = nch * 32 - 4
            hdt = torch.float16 if (C == 256 and dtype == torch.bfloat16) else None
            for pat in X.PATTERNS:
                offs = X.mlp_offsets(pat, S, T, S)
                if pat == "onehot":                              # together the launches name every k of both products
                    assert {(t + o1) % S for o1, _ in offs for t in range(T)} == set(range(S))
                    assert {(s + o2) % T for _, o2 in offs for s in range(S)} == set(range(T))
                for (o1, o2) in offs:
                    c = X.mlp_case(pat, dtype, nimg * C, S, T, S, off1=o1, off2=o2)
                    x0, want = X.token_mlp_residual(c, nimg, C, S)
                    X.check_mlp_case(c, hidden_dtype=hdt, residual=want.permute(0, 2, 1).reshape(nimg * C, S) - c.core)
                    if C == 256:
                        xl, _, _, _, _, want = X.token_mlp_ln_inputs(c, nimg, C, S)
                        assert X.representable(xl, dtype)
                        X.check_mlp_case(c, hidden_dtype=hdt, residual=want.permute(0, 2, 1).reshape(nimg * C, S) - c.core)
        for g in X.DWCONV_OLD_CASES:                             # (the whole table: test_premises_of_the_dwconv_table)
            for pat in X.PATTERNS:
                for off in X.pattern_offsets(pat, g[3], g[4] ** 2):
                    X.check_dwconv_case(X.dwconv_case(pat, dtype, *g, off=off))
        for g in X.VIP_CASES:
            for which in (0, 1):
                for pat in X.PATTERNS:
                    X.check_vip_case(X.vip_case(pat, dtype, *g, which))
        for g in X.SMLP_CASES:
            for dw in (False, True):
                for pat in X.PATTERNS:
                    X.check_smlp_case(X.smlp_case(pat, dtype, *g, dw=dw))
        for g in X.ASCONV_CASES:
            for pat in X.PATTERNS:
                X.check_asconv_case(X.asconv_case(pat, dtype, *g))
        for g in X.SWIN_CASES:
            for pat in X.PATTERNS:
                if pat != "cancel" or X.swin_cancel_possible(g[1], g[2], g[4], g[5]):
                    X.check_swin_case(X.swin_case(pat, dtype, *g))
    assert any(X.swin_cancel_possible(g[1], g[2], g[4], g[5]) for g in X.SWIN_CASES)


def test_check_case_refuses_a_broken_premise():
    c = X.gemm_case("ternary", torch.bfloat16, 65, 72, 136)
    c.want = c.want + 0.5 + 1.0 / 512                        # not a bf16 value
    with pytest.raises(AssertionError):
        X.check_case(c)
    c = X.gemm_case("cancel", torch.bfloat16, 65, 72, 136)
    c.acc = c.acc * 0 + 64.0                                 # the block no longer leaves the integer range
    with pytest.raises(AssertionError):
        X.check_case(c)
    c = X.gemm_case("ternary", torch.float16, 65, 72, 136)
    c.A[:, 40:72] = 0                                        # a slab without a term
    with pytest.raises(AssertionError):
        X.check_case(c)
    c = X.gemm_case("onehot", torch.float16, 65, 72, 136)    # N < K and a single launch: some k never occurs
    c.k_off = 5
    with pytest.raises(AssertionError):
        X.check_case(c)
    c = X.gemm_case("ternary", torch.float32, 9, 16, 64, gelu=True)
    c.pre_act = c.pre_act - 130                              # below the threshold
    with pytest.raises(AssertionError):
        X.check_case(c)


def test_assert_exact_names_the_element_and_k():
    want = torch.arange(12.0).reshape(3, 4)
    got = want.clone()
    X.assert_exact(got, want, "same")
    got[1, 2] += 1
    got[2, 3] += 1
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, want, "case", K=3)
    assert "first at (1, 2)" in str(e.value) and "2 of 12" in str(e.value) and "(k = 2)" in str(e.value)


def test_row_part_want_is_exact_in_fp32():
    c = X.gemm_case("ternary", torch.bfloat16, 65, 136, 136, res=1)
    p = X.row_part_want(c.want, 5)
    assert X.representable(p, torch.float32) and p.shape == (5, 65, 2)
    assert torch.equal(p[:, :, 0].sum(0), c.want.sum(1))


# ------------------------------------------------------------------------------------------------- planted faults
MODEL = dict(M=97, N=104, K=200, bm=64, bn=64, slab=32)      # ragged in M and N, a short last K slab, four tiles


def _caught(pattern, fault, offsets=(0,)):
    """whether `pattern` sees `fault`, and where (the one-hot pattern runs one model launch per offset, as the GPU file does)"""
    for off in offsets:
        c = X.gemm_case(pattern, torch.bfloat16, MODEL["M"], MODEL["N"], MODEL["K"], k_off=off)
        X.check_case(c)
        good = X.tiled_gemm_model(c.A, c.B, c.bias, c.dtype, MODEL["bm"], MODEL["bn"], MODEL["slab"])
        X.assert_exact(good, c.want, "the fault-free model is exact")
        got = X.tiled_gemm_model(c.A, c.B, c.bias, c.dtype, MODEL["bm"], MODEL["bn"], MODEL["slab"], fault=fault)
        try:
            X.assert_exact(got, c.want, fault, K=c.K, k_off=off)
        except AssertionError as e:
            return e                                         # (assert_exact attaches .index and .k)
    return None


OFFS = X.onehot_offsets(MODEL["N"], MODEL["K"])
# which pattern catches which fault.  The structural faults change integers, so the one-hot and the ternary pattern see them; the
# precision faults leave every small integer alone and show only where the accumulator leaves the 16-bit range: the cancel pattern.
CATCHES = {
    "skip_last_chunk": dict(onehot=True, ternary=True, cancel=True),
    "dup_k": dict(onehot=True, ternary=True, cancel=True),
    "clamped_row": dict(onehot=True, ternary=True, cancel=True),
    "bias_tail": dict(onehot=True, ternary=True, cancel=True),
    "bf16_acc": dict(onehot=False, ternary=False, cancel=True),
    "round_before_bias": dict(onehot=False, ternary=False, cancel=True),
}


@pytest.mark.parametrize("fault", X.FAULTS)
def test_planted_fault(fault):
    for pattern, expect in CATCHES[fault].items():
        msg = _caught(pattern, fault, OFFS if pattern == "onehot" else (0,))
        assert (msg is not None) == expect, (fault, pattern, msg)
    if fault == "skip_last_chunk":
        # the one-hot pattern names the K index, and the element lies inside the last tile
        e = _caught("onehot", fault, OFFS)
        assert MODEL["K"] - 8 <= e.k < MODEL["K"] and "(k = %d)" % e.k in str(e), str(e)
        assert e.index[0] >= MODEL["bm"] and e.index[1] >= MODEL["bn"], str(e)
    if fault == "clamped_row":
        e = _caught("onehot", fault, OFFS)
        assert e.index[0] == MODEL["M"] - 1, str(e)                       # the source row is named
    if fault == "bias_tail":
        e = _caught("ternary", fault)
        assert e.index[1] == MODEL["N"] - 1, str(e)


def test_gaussian_gate_passes_both_precision_faults_at_k_200():
    """The gap, pinned: the gate of tests/test_gpu_ops.py -- max|got - ref| < EPS 4 max(1, max|ref|) -- on the bf16 shape
    (257, 129, 200) of test_gemm_rowmajor_epilogues passes a GEMM whose accumulators are rounded to bf16 between K slabs and one
    that rounds the product before the bias, although both are several times further from fp64 than the correct kernel."""
    EPS = 8e-3
    M, N, K = 257, 129, 200
    g = torch.Generator().manual_seed(11)
    A = torch.randn((M, K), generator=g).to(torch.bfloat16)
    B = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn((N,), generator=g)
    ref = A.double() @ B.double().t() + bias.double()
    gate = EPS * 4 * max(1.0, ref.abs().max().item())
    err = {}
    for fault in (None, "bf16_acc", "round_before_bias"):
        got = X.tiled_gemm_model(A.float().numpy(), B.float().numpy(), bias.numpy(), torch.bfloat16, 64, 64, 32, fault=fault)
        err[fault] = ((got - ref).abs().max().item(), (got - ref).pow(2).mean().sqrt().item())
        assert err[fault][0] < gate, (fault, err[fault], gate)                   # ... and stays green
    floor = (ref.to(torch.bfloat16).double() - ref).pow(2).mean().sqrt().item()
    assert err[None][1] <= 1.02 * floor                                          # the correct kernel: one rounding
    # the faults are real, and the rounding budget of tests/test_gpu_rounding.py (1.10 sqrt(1) x the floor) sees both
    assert err["bf16_acc"][1] > 1.5 * floor and err["round_before_bias"][1] > 1.10 * floor, (err, floor)
    assert gate > 8 * err[None][0]                                               # the gate is an order of magnitude above a correct kernel


# ------------------------------------------------------------------------------------------------- depthwise convolution: the table
@pytest.mark.parametrize("dtype", X.STORAGE)
def test_premises_of_the_dwconv_table(dtype):
    """every geometry x pattern x offset of exact.DWCONV_TABLE, fp32 included (GELU_THRESHOLD serves gelu_f too: the first test of this
    file); the full tap sweep and the case whose x is off a 16-byte boundary.  cancel runs where dwconv_patterns says it can."""
    n = 0
    for g in X.DWCONV_CASES:
        pats = X.dwconv_patterns(dtype, g)
        assert pats[:2] == ["onehot", "ternary"]
        for pat in pats:
            for off in X.dwconv_offsets(pat, g[3], g[4]):
                X.check_dwconv_case(X.dwconv_case(pat, dtype, *g, off=off))
                n += 1
    assert n >= len(X.DWCONV_CASES) * 2
    if dtype != torch.float32:
        carried = [g for g in X.DWCONV_CASES if "cancel" in X.dwconv_patterns(dtype, g)]
        left = [g for g in X.DWCONV_CASES if g not in carried]
        assert sorted(left) == sorted([(2, 1, 32, 8, 7), (2, 32, 1, 8, 7), (1, 1, 1, 8, 9), (1, 6, 6, 8, 1)]), left
        for g in X.DWCONV_SWEEP:
            for off in X.dwconv_offsets("onehot", g[3], g[4], full=True):
                X.check_dwconv_case(X.dwconv_case("onehot", dtype, *g, off=off))
        g, _ = X.DWCONV_OFFSET_CASE
        for pat in X.dwconv_patterns(dtype, g):
            X.check_dwconv_case(X.dwconv_case(pat, dtype, *g))
    else:
        assert all("cancel" not in X.dwconv_patterns(dtype, g) for g in X.DWCONV_CASES)


def _dw_row(g):
    B, H, W, C, k = g
    groups, ranges, per, redeal = X.dwconv_plan(B, C)
    f32, f16, bf16 = (X.dwconv_form(dt, H, W, C, k) for dt in X.STORAGE)
    assert f16 == bf16
    return dict(B=B, H=H, W=W, C=C, k=k, f32=f32, h=f16, groups=groups, ranges=ranges, per=per, redeal=redeal, last=B - (ranges - 1) * per,
                why32=X.dwconv_direct_reason(torch.float32, H, W, C, k), why16=X.dwconv_direct_reason(torch.float16, H, W, C, k))


# what the table claims to reach: (claim, predicate over one row as _dw_row describes it).  `h` is the 16-bit form, `last` the number
# of images in the last range.  Every row of the table is the only one that serves some claim (the test below deletes each in turn).
_MF = ("mfma", "mfma_full")
DW_CLAIMS = [("lds in fp32", lambda r: r["f32"] == "lds"), ("direct in fp32", lambda r: r["f32"] == "direct")] + [
    ("%s in 16 bits" % f, (lambda f: lambda r: r["h"] == f)(f)) for f in ("mfma_full", "mfma", "lds", "direct")]
for _k in (3, 5, 7, 9):
    DW_CLAIMS += [
        ("mfma k=%d: one block, a partial second channel group, one range" % _k,
         (lambda k: lambda r: r["h"] == "mfma" and r["k"] == k and r["H"] <= 16 and r["W"] <= 16 and r["C"] > 32 and r["C"] % 32 and r["ranges"] == 1)(_k)),
        ("mfma k=%d: all four blocks and the store's tail at x >= 16" % _k,
         (lambda k: lambda r: r["h"] == "mfma" and r["k"] == k and r["H"] > 16 and r["W"] > 16 and r["W"] % 4 != 0)(_k)),
        ("mfma_full k=%d: one group, the prefetch runs" % _k,
         (lambda k: lambda r: r["h"] == "mfma_full" and r["k"] == k and r["groups"] == 1 and min(r["B"], r["per"]) >= 2)(_k)),
    ]
DW_CLAIMS += [
    ("mfma_full, two channel groups", lambda r: r["h"] == "mfma_full" and r["groups"] >= 2),
    ("mfma, a full map that is not FULL", lambda r: r["h"] == "mfma" and r["H"] == 32 and r["W"] == 32),
    ("mfma, several ranges, the last partial with a prefetch", lambda r: r["h"] in _MF and r["ranges"] > 1 and 2 <= r["last"] < r["per"] and not r["redeal"]),
    ("mfma, three ranges, the last of one image", lambda r: r["h"] in _MF and r["ranges"] >= 3 and r["last"] == 1 and not r["redeal"]),
    ("mfma, the re-deal with whole ranges", lambda r: r["h"] in _MF and r["redeal"] and r["last"] == r["per"]),
    ("mfma, the re-deal with a partial last range", lambda r: r["h"] in _MF and r["redeal"] and r["last"] < r["per"]),
    ("mfma, one row", lambda r: r["h"] in _MF and r["H"] == 1 and r["W"] > 1),
    ("mfma, one column", lambda r: r["h"] in _MF and r["W"] == 1 and r["H"] > 1),
    ("mfma, one pixel", lambda r: r["h"] in _MF and r["H"] == 1 and r["W"] == 1),
    ("16-bit lds, H past 32 alone", lambda r: r["h"] == "lds" and r["H"] > 32 and r["W"] <= 32),
    ("16-bit lds, five whole strips", lambda r: r["h"] == "lds" and r["W"] >= 40 and r["W"] % 8 == 0 and r["H"] <= 32),
    ("16-bit lds, W % 8 != 0 and a partial channel tile", lambda r: r["h"] == "lds" and r["W"] % 8 != 0 and r["C"] % 32 != 0),
    ("16-bit lds, H and W past 32", lambda r: r["h"] == "lds" and r["H"] > 32 and r["W"] > 32),
    ("direct: the tile does not fit, whole channel tiles", lambda r: r["why16"] == "fit" and r["why32"] == "fit" and r["C"] % 32 == 0),
    ("direct: the tile does not fit, a partial 16-bit channel tile", lambda r: r["why16"] == "fit" and r["why32"] == "fit" and r["C"] % 32 != 0),
    ("direct in 16 bits for C % 8, lds in fp32, k = 3, one channel block", lambda r: r["why16"] == "channels" and r["f32"] == "lds" and r["k"] == 3 and r["C"] <= 64),
    ("direct in 16 bits for C % 8, lds in fp32, k = 5", lambda r: r["why16"] == "channels" and r["f32"] == "lds" and r["k"] == 5),
    ("direct in 16 bits for C % 8, lds in fp32, two channel blocks", lambda r: r["why16"] == "channels" and r["f32"] == "lds" and r["C"] > 64),
    ("direct in fp32 for C % 4, one channel block", lambda r: r["why32"] == "channels" and r["C"] <= 64),
    ("direct in fp32 for C % 4, two channel blocks", lambda r: r["why32"] == "channels" and r["C"] > 64),
] + [("direct for k = %d" % k, (lambda k: lambda r: r["why16"] == "k" and r["why32"] == "k" and r["k"] == k)(k)) for k in (1, 11, 13)]


def _dw_uncovered(table):
    rows = [_dw_row(g) for g in table]
    return [name for name, pred in DW_CLAIMS if not any(pred(r) for r in rows)]


def test_the_dwconv_table_reaches_every_form_tile_and_plan():
    """dwconv_form / dwconv_plan over the table: every form in every type that has it, both matrix-core instantiations at every k, all
    four blocks with the store's tail, partial last ranges, the re-deal twice, the generic kernel for each of its four reasons"""
    assert _dw_uncovered(X.DWCONV_CASES) == []
    assert len(set(X.DWCONV_CASES)) == len(X.DWCONV_CASES) and X.DWCONV_CASES[:3] == X.DWCONV_OLD_CASES
    # the fourth reason is x off a 16-byte boundary: no geometry has it, the offset case does (in 16 bits; it would be mfma otherwise)
    (B, H, W, C, k), off = X.DWCONV_OFFSET_CASE
    for dt in X.SIXTEEN:
        assert (off * 2) % 16 != 0 and X.dwconv_form(dt, H, W, C, k) == "mfma" and X.dwconv_direct_reason(dt, H, W, C, k, aligned=False) == "alignment"
    reasons = {X.dwconv_direct_reason(dt, *g[1:]) for g in X.DWCONV_CASES for dt in X.STORAGE} - {None}
    assert reasons == {"k", "channels", "fit"}
    # what the old table reached: one block of one instantiation, one range, no re-deal
    old = [_dw_row(g) for g in X.DWCONV_OLD_CASES]
    assert all(r["h"] == "mfma" and r["H"] <= 16 and r["W"] <= 16 and r["ranges"] == 1 and not r["redeal"] for r in old)
    # every geometry of the batch test spans more than one image, and the three forms are among them
    assert {X.dwconv_form(torch.bfloat16, *g[1:]).split("_")[0] for g in X.DWCONV_BATCH} == {"mfma", "lds", "direct"}
    assert all(g in X.DWCONV_CASES and g[0] >= 2 for g in X.DWCONV_BATCH)


@pytest.mark.parametrize("row", range(len(X.DWCONV_CASES)))
def test_every_row_of_the_dwconv_table_is_needed(row):
    """with any single row deleted some claim is left without a geometry"""
    rest = X.DWCONV_CASES[:row] + X.DWCONV_CASES[row + 1:]
    assert _dw_uncovered(rest) != [], X.DWCONV_TABLE[row]


def test_the_dwconv_redeal_is_a_permutation():
    """the kernel's map from blockIdx to (channel group, image range) is a bijection onto the grid wherever its condition turns it on;
    the 8 workgroups that start together on one XCD (ids congruent mod 8 in one round of 64) are 8 neighbouring groups of one range"""
    n = 0
    for groups in range(8, 65, 8):
        for ranges in range(1, 65):
            if (groups * ranges) % 64:
                continue
            seen = {X.dwconv_redeal(bx, by, groups, ranges) for by in range(ranges) for bx in range(groups)}
            assert seen == {(gx, gy) for gy in range(ranges) for gx in range(groups)}, (groups, ranges)
            for rnd0 in range(0, groups * ranges, 64):
                for xcd in range(8):
                    got = [X.dwconv_redeal(i % groups, i // groups, groups, ranges) for i in range(rnd0 + xcd, rnd0 + 64, 8)]
                    assert len({gy for _, gy in got}) == 1 and sorted(gx for gx, _ in got) == list(range(got[0][0] // 8 * 8, got[0][0] // 8 * 8 + 8))
            n += 1
    assert n > 50
    for g in X.DWCONV_CASES:                                 # the plan's condition is the one under which the map above is used
        groups, ranges, per, redeal = X.dwconv_plan(g[0], g[3])
        assert redeal == (groups % 8 == 0 and (groups * ranges) % 64 == 0) and (ranges - 1) * per < g[0] <= ranges * per


# ------------------------------------------------------------------------------------------------- depthwise convolution: planted faults
def _dw_cases(table, dtype, old):
    """the launches of a table: the old one ran every pattern with the offsets of onehot_offsets; the new one adds the full tap sweep"""
    for g in table:
        for pat in (X.PATTERNS if old else X.dwconv_patterns(dtype, g)):
            for off in X.dwconv_offsets(pat, g[3], g[4]):
                yield (pat, g, off)
    if not old:
        for g in X.DWCONV_SWEEP:
            for off in X.dwconv_offsets("onehot", g[3], g[4], full=True):
                yield ("onehot", g, off)


_DW_CACHE = {}


def _dw_case(pat, dtype, g, off):
    key = (pat, dtype, g, off)
    if key not in _DW_CACHE:
        _DW_CACHE[key] = X.dwconv_case(pat, dtype, *g, off=off)
    return _DW_CACHE[key]


def _dw_sees(table, old, fault, swap=None, dtype=torch.bfloat16, k=None):
    """the first launch of a table whose exact comparison fails under the planted fault (None: the table is blind to it)"""
    for (pat, g, off) in _dw_cases(table, dtype, old):
        if k is not None and g[4] != k:
            continue
        if fault == "table_swap":
            if g[4] not in (7, 9) or swap[0] < X.DWM_CREG[g[4]] or swap[1] >= g[4] or swap[2] + 1 >= g[4]:
                continue                                     # no table fragment, or no such tap, at this k
        elif pat != "onehot" and not old:
            continue                                         # (one pattern is enough to show that the new table sees a region fault)
        c = _dw_case(pat, dtype, g, off)
        if fault == "table_swap":
            t = swap[1] * g[4] + swap[2]
            sel = torch.arange(g[3]) % X.DWM_CPW == swap[0]
            if torch.equal(c.w[t, sel], c.w[t + 1, sel]):
                continue                                     # (exact, and cheap: equal taps swapped are the same taps)
        got = X.dwconv_fault_model(c, fault, swap)
        try:
            X.assert_exact(got, c.want, fault)
        except AssertionError as e:
            e.case = (pat, g, off)
            return e
    return None


@pytest.mark.parametrize("fault", X.DW_FAULTS[:4])
def test_planted_dwconv_region_fault(fault):
    """the record of why the rows are there: the old three-row table with its one-hot sweep is blind to each of these faults of the
    matrix-core form, and the new table names an element inside the fault's region"""
    assert _dw_sees(X.DWCONV_OLD_CASES, True, fault) is None
    for (pat, g, off) in _dw_cases(X.DWCONV_OLD_CASES, torch.bfloat16, True):
        c = _dw_case(pat, torch.bfloat16, g, off)
        X.assert_exact(X.dwconv_fault_model(c, None), c.want, "the fault-free model is the reference")
    e = _dw_sees(X.DWCONV_CASES, False, fault)
    assert e is not None, fault
    b, y, x, ch = e.index
    (B, H, W, C, k) = e.case[1]
    if fault == "block_10":
        assert y >= 16 and x < 16
    elif fault == "block_01":
        assert y < 16 and x >= 16
    elif fault == "tail_dropped":
        assert x >= 16 and x // 4 * 4 + 3 >= W and W % 4 != 0
    else:
        _, ranges, per, _ = X.dwconv_plan(B, C)
        assert ranges > 1 and b > (ranges - 1) * per


def test_planted_dwconv_table_swap():
    """every (slot j >= CREG, tap row i, d) swap of the LDS-table fragments at k = 7 and k = 9 -- 186 faults.  The old table, whose
    one-hot sweep gives a channel 3 of its 81 taps, is blind to some of them (its ternary taps are sparse); the new table, whose
    sweep gives every channel every tap, sees every one and names a channel of the slot."""
    blind_old, total = [], 0
    for k in (7, 9):
        for j in range(X.DWM_CREG[k], X.DWM_CPW):
            for i in range(k):
                for d in range(k - 1):
                    swap = (j, i, d)
                    total += 1
                    if _dw_sees(X.DWCONV_OLD_CASES, True, "table_swap", swap, k=k) is None:
                        blind_old.append((k,) + swap)
                    new = _dw_sees(X.DWCONV_CASES, False, "table_swap", swap, k=k)
                    assert new is not None and new.index[3] % X.DWM_CPW == j, (k, swap)
    assert total == 7 * 6 + 2 * 9 * 8
    assert blind_old, "the old table saw every planted swap"
    print("table_swap: the old table is blind to %d of %d swaps, e.g. %s" % (len(blind_old), total, blind_old[:4]))
    # a register-held slot is not a table fragment: the fault has no region there
    c = _dw_case("onehot", torch.bfloat16, X.DWCONV_SWEEP[3], 0)
    assert not X.dwconv_fault_region(c, "table_swap", (0, 0, 0)).any() and X.dwconv_fault_region(c, "table_swap", (3, 0, 0)).any()
