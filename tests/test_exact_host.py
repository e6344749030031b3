"""The exact-integer oracle (tests/exact.py) checked on the CPU: its premises for every case table the GPU file uses, the GELU
threshold from emulations of the three forms of csrc/mlpk_common.h, and a numpy model of a tiled GEMM with planted faults -- which
pattern catches which fault, and that the Gaussian gate of tests/test_gpu_ops.py lets the two precision faults pass."""
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
        for g in X.DWCONV_CASES:
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
