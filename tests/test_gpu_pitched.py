"""-m gpu: the pitched / offset-pointer contract of include/mlpk.h, entry point by entry point, behind guard bands (tests/guard.py).

Every call is made twice: once with all pitched operands inside `Guarded` buffers -- padded pitches, bases at an offset into one allocation, column
slices taken the way the models take them -- and once on dense, allocator-aligned copies.  Asserted each time:
  a. output guards intact (lead, tail, pad columns bit-identical to the poison; zero-filled pads exactly +0), inputs bit-unchanged;
  b. the logical output finite everywhere (an input's NaN padding was not read as data, nothing was left unwritten);
  c. the bits of the dense call wherever the same kernel runs (an explicit GEMM `algo`, equal mlpk_gemm_kernel_name, or the header's "does not
     depend on the pitches");
  d. where pitch or alignment legitimately change the kernel (GEMM algo 0): the fp64 restatement and tolerance of test_gpu_ops.py.
PITCHED (below) names the test that covers each entry point; tests/test_guard_host.py holds it against the header."""
import ctypes
import math

import pytest
import torch

from conftest import load_pkg
from guard import Guarded, assert_bits_equal, assert_finite, lead_for
from test_gpu_ops import EPS, gemm_ref, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS16 = [torch.float16, torch.bfloat16]
DTYPES = [torch.float32] + BITS16
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}

# entry point or descriptor -> (pitch parameters covered, covering test)
PITCHED = {
    "mlpk_gemm_desc": (("lda", "ldb", "ldc", "ldr", "row_part_ld"), "test_gemm_rowmajor_pitched, test_gemm_token_transposed_pitched, "
                       "test_gemm_persistent_and_generated_pitched, test_gemm_pair_two_slices_of_one_buffer, test_conv_gemm_pitched"),
    "mlpk_norm_desc": (("ldx", "ld_rm", "ld_tt", "ld_p", "ld_sum"), "test_norm_apply_pitched"),
    "mlpk_row_stats": (("ldx",), "test_row_stats_pitched"),
    "mlpk_layernorm_transpose": (("ldx", "ld_tt"), "test_layernorm_transpose_pitched"),
    "mlpk_pool_mean": (("ldx", "ldo"), "test_pool_mean_pitched"),
    "mlpk_split_sum": (("ld0", "ld1", "ld2"), "test_split_attention_pitched"),
    "mlpk_split_apply": (("ld0", "ld1", "ld2", "ldo"), "test_split_attention_pitched"),
    "mlpk_vip_unpermute": (("ldz",), "test_vip_unpermute_pitched"),
    "mlpk_s2_shift": (("ldi", "ldo"), "test_s2_shift_pitched"),
    "mlpk_s2_shift2": (("ldi", "ldo"), "test_s2_shift2_pitched"),
    "mlpk_cycle_shift": (("ldi", "ldo"), "test_cycle_shift_pitched"),
    "mlpk_cycle_shift_ln": (("ldi", "ldo"), "test_cycle_shift_pitched"),
    "mlpk_hire_gather": (("ld_h", "ld_w"), "test_hire_remaps_pitched"),
    "mlpk_hire_gather_ln": (("ld_h", "ld_w"), "test_hire_remaps_pitched"),
    "mlpk_hire_combine": (("ld_h", "ld_w"), "test_hire_remaps_pitched"),
    "mlpk_hire_combine_from": (("ld_h", "ld_w"), "test_hire_remaps_pitched"),
    "mlpk_hire_combine_stats": (("ld_h", "ld_w"), "test_hire_remaps_pitched"),
    "mlpk_patchify": (("src_px_stride", "ldo"), "test_patchify_im2col_pitched"),
    "mlpk_im2col": (("src_px_stride", "ldo"), "test_patchify_im2col_pitched"),
    "mlpk_add_periodic": (("ldx",), "test_add_periodic_pitched"),
    "mlpk_dropout": (("ldx", "ldy"), "test_dropout_pitched"),
    "mlpk_ew_cols": (("lda", "ldb", "ldo"), "test_ew_cols_pitched"),
    "mlpk_col_sum": (("ld",), "test_column_reductions_pitched"),
    "mlpk_col_dot": (("ldx", "ldy"), "test_column_reductions_pitched"),
    "mlpk_col_dot_seg": (("ldx", "ldy"), "test_column_reductions_pitched"),
    "mlpk_gelu_elementwise": (("ld",), "test_gelu_elementwise_pitched"),
    "mlpk_transpose_batched": (("ld_in", "ld_out", "ld_res"), "test_transpose_batched_pitched"),
    "mlpk_layernorm_backward": (("ldx", "lddy", "lddx"), "test_layernorm_backward_pitched"),
    "mlpk_stats_finalize_planar": (("plane_stride",), "test_stats_finalize_planar_pitched"),
    "mlpk_token_gemm": (("ldr", "ldo"), "test_token_gemm_pitched"),
    "mlpk_token_gemm_ln": (("ldx", "ldr", "ldo"), "test_token_gemm_ln_pitched"),
    "mlpk_token_gemm_ln_post": (("ldx", "ldr", "ldo"), "test_token_gemm_ln_pitched"),
    "mlpk_channel_mlp": (("ldx", "ldr", "ldo", "ldw2"), "test_channel_mlp_pitched"),
    "mlpk_smlp_mix": (("ldx", "ldo"), "test_smlp_mix_pitched"),
    "mlpk_smlp_mix_dw": (("ldx", "ldxr", "ldo"), "test_smlp_mix_pitched"),
    "mlpk_vip_branch": (("ldx", "ldw", "ldz", "ld_sum"), "test_vip_branch_and_split_apply_pitched"),
    "mlpk_vip_split_apply": (("ldh", "ldw", "ldc", "ldo"), "test_vip_branch_and_split_apply_pitched"),
    "mlpk_patch_embed4": (("ldw", "ldo"), "test_embeddings_pitched"),
    "mlpk_stem7": (("ldo",), "test_embeddings_pitched"),
    "mlpk_mixshift_nhwc_stats": (("row_part_ld",), "test_dense_convolutions_guarded"),
    "mlpk_token_mlp": (("ldx", "ldw2"), "test_token_mlp_pitched, test_token_mlp_generated_and_ln_pitched"),
    "mlpk_token_mlp_ln": (("ldx",), "test_token_mlp_generated_and_ln_pitched"),
    "mlpk_as_conv2": (("ldw",), "test_as_conv2_pitched"),
    "mlpk_as_conv2_stats": (("ldw",), "test_as_conv2_pitched"),
    "mlpk_raft_gather_ln": (("x_pitch", "a_pitch"), "test_raft_pitched"),
    "mlpk_raft_scatter_add": (("x_pitch", "y_pitch"), "test_raft_pitched"),
    "mlpk_atm_sample": (("x_pitch", "off_pitch", "out_pitch"), "test_atm_sample_pitched"),
    "mlpk_dyna_mix": (("x_pitch", "t_pitch", "t_off", "out_pitch"), "test_dyna_mix_pitched"),
    "mlpk_dyna_gather": (("t_pitch", "t_off", "v_pitch"), "test_dyna_mix_pitched"),
    "mlpk_dyna_mix_logits": (("x_pitch", "z_pitch", "out_pitch"), "test_dyna_mix_pitched"),
    "mlpk_lstm_scan": (("xp_pitch", "xp_off", "out_pitch", "out_off"), "test_lstm_scan_pitched"),
    "mlpk_wave_patm": (("ldy", "ldo"), "tests/test_gpu_wave.py::test_wave_patm_kernel (a sentinel in the pad columns of the output and NaN in those of the input)"),
}


def pk():
    pkg = load_pkg()
    return pkg.engine, pkg._native


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the two-layout harness
class Ops:
    """Operand factory of one call: pitched=True puts every operand into a Guarded buffer with the pitch and lead offset asked for, pitched=False
    makes the dense, allocator-aligned twin (still guarded: lead, tail and unwritten elements are checked there too)."""

    def __init__(self, pitched):
        self.pitched, self.items = pitched, {}

    def _mk(self, name, rows, cols, dtype, pad, off, role, data=None, zero_pad=False, finite=True, dpad=0):
        ld = cols + (pad if self.pitched else dpad)            # dpad: the padding the DENSE twin needs where the entry point demands ld % 8 == 0
        g = Guarded(rows, cols, ld, dtype, DEV, lead=lead_for(ld, off if self.pitched else 0), role=role, data=data)
        self.items[name] = (g, zero_pad, finite)
        return g.view

    def inp(self, name, data, pad=8, off=0, dpad=0):
        return self._mk(name, data.shape[0], data.shape[1], data.dtype, pad, off, "in", data, dpad=dpad)

    def inout(self, name, data, pad=8, off=0, dpad=0):
        return self._mk(name, data.shape[0], data.shape[1], data.dtype, pad, off, "inout", data, dpad=dpad)

    def out(self, name, rows, cols, dtype, pad=8, off=0, zero_pad=False, finite=True, dpad=0):
        return self._mk(name, rows, cols, dtype, pad, off, "out", zero_pad=zero_pad, finite=finite, dpad=dpad)

    def vec(self, name, n):
        """a float32 vector output (statistics, column sums): dense by contract, guarded at both ends"""
        return self._mk(name, 1, n, torch.float32, 0, 0, "out")[0]

    def g(self, name):
        return self.items[name][0]

    def verify(self):
        for name, (g, zero_pad, finite) in self.items.items():
            try:
                g.check(zero_cols=(g.cols, g.ld) if zero_pad and g.ld > g.cols else None)
                if g.role != "in" and finite:
                    assert_finite(g.view, "logical output")
            except AssertionError as e:
                raise AssertionError("%s [%s]: %s" % (name, "pitched" if self.pitched else "dense", e)) from None


def both(case, bits=True):
    """run `case(ops)` in the pitched and in the dense layout; (a), (b) for each, then (c): the same bits (bits=False: the caller holds both
    layouts to a reference instead, where alignment legitimately selects another kernel)"""
    res = {}
    for pitched in (True, False):
        ops = Ops(pitched)
        post = case(ops)
        sync()
        ops.verify()
        if post is not None:
            post(ops)
        res[pitched] = ops
    for name, (g, _, _) in res[True].items.items():
        if g.role != "in" and bits:
            assert_bits_equal(g.dense(), res[False].g(name).dense(), name)
    return res[True]


def refused(N, fn, *outs):
    """a documented refusal: MlpkError, and not one element of the outputs written"""
    with pytest.raises(N.MlpkError):
        fn()
    sync()
    for g in outs:
        g.all_poison()


def rd(shape, dtype, seed, scale=1.0):
    return rnd(shape, dtype, seed, scale).to(DEV)


# ------------------------------------------------------------------ mlpk_gemm_nt
def vec_class(ld, lead, es):
    """gemm_resolve's store / residual-load class of an operand at element offset `lead` of an allocator-aligned buffer: 0 scalar, 1 = 4-element
    vectors, 2 = 16-byte vectors"""
    c = int(ld % 4 == 0 and (lead * es) % (4 * es) == 0)
    if c and ld % 8 == 0 and (lead * es) % 16 == 0:
        c = 2
    return c


def desc(E, *a, **kw):
    return E.gemm(*a, _defer=True, **kw)[0]


def kernel_name(N, d):
    buf = ctypes.create_string_buffer(96)
    rc = N.lib().mlpk_gemm_kernel_name(ctypes.byref(d), buf, 96)
    return rc, buf.value.decode()


def launch(E, N, d):
    N.check(N.lib().mlpk_gemm_nt(ctypes.byref(d), E.stream()), "mlpk_gemm_nt")


def try_launch(E, N, d):
    """False when the call is refused (an argument error: nothing launched)"""
    try:
        launch(E, N, d)
    except N.MlpkError:
        return False
    return True


# (lda - K, ldb - K, ldc - N, ldr - N) and the (C lead, R lead) offsets run with each
PITCH_SETS = {
    "p8_16_8_16": ((8, 16, 8, 16), [(0, 0), (4, 0), (0, 4), (4, 4), (2, 1)]),
    "p8_8_4_8": ((8, 8, 4, 8), [(0, 0), (2, 4), (0, 1), (4, 0), (2, 0)]),
    "p0_0_2_1": ((0, 0, 2, 1), [(0, 0), (1, 2)]),
}
# K = 136 and 72 are no whole half-slabs: the LDS-DMA tiles 6 .. 13 refuse them (nothing may be written); the two K = 160 shapes are theirs
ROW_SHAPES = [(130, 70, 136), (130, 72, 136), (257, 136, 72), (130, 70, 160), (130, 72, 160)]
EPILOGUES = ["bias_gelu_add", "bias_affine_mul", "rscale13"]


def test_gemm_pitch_sets_reach_every_store_and_load_class():
    """no launch: the cases of test_gemm_rowmajor_pitched reach vec_c x vec_r in {0, 1, 2}^2 for the 16-bit types"""
    seen = set()
    for (_, _, dc, dr), offs in PITCH_SETS.values():
        for M, Nn, K in ROW_SHAPES:
            for oc, orr in offs:
                seen.add((vec_class(Nn + dc, lead_for(Nn + dc, oc), 2), vec_class(Nn + dr, lead_for(Nn + dr, orr), 2)))
    assert seen == {(c, r) for c in range(3) for r in range(3)}, sorted(seen)


def epilogue_kw(name, M, Nn, dtype, seed):
    kw = {}
    if name == "bias_gelu_add":
        kw = dict(bias=rd((Nn,), torch.float32, seed + 1), act=1, res=1)
    elif name == "bias_affine_mul":
        kw = dict(bias=rd((Nn,), torch.float32, seed + 1), cscale=rd((Nn,), torch.float32, seed + 2) * 0.2 + 1, cshift=rd((Nn,), torch.float32, seed + 3), res=2)
    elif name == "rscale13":
        kw = dict(rscale=rd((13,), torch.float32, seed + 4) * 0.3 + 1, rperiod=13)
    return kw


def ref_of(A, B, M, Nn, K, kw, R, **extra):
    c = lambda t: None if t is None else t.cpu()
    return gemm_ref(A.cpu(), B.cpu(), M, Nn, K, bias=c(kw.get("bias")), act=kw.get("act", 0), cscale=c(kw.get("cscale")), cshift=c(kw.get("cshift")),
                    rscale=c(kw.get("rscale")), rperiod=kw.get("rperiod", 1) or 1, R=c(R), res=kw.get("res", 0), **extra)


def close_to_ref(got, ref, dtype, factor, what):
    err = (got.double().cpu() - ref).abs().max().item()
    tol = EPS[dtype] * max(1.0, ref.abs().max().item()) * factor
    assert err < tol, (what, err, tol)


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("si", range(len(ROW_SHAPES)), ids=["%dx%dx%d" % s_ for s_ in ROW_SHAPES])
@pytest.mark.parametrize("pset", list(PITCH_SETS), ids=list(PITCH_SETS))
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_gemm_rowmajor_pitched(dtype, pset, si, epi):
    """row-major algos 1 .. 13 (and 0): one shape, pitch set and epilogue x every tile x the set's lead offsets; explicit algo = the dense call's
    bits, algo 0 = those bits when the dispatch names the same kernel, else the fp64 restatement.  An algo that refuses the shape (K no whole
    half-slab) must write nothing.  The pitched calls are checked before the dense twin: its pad columns do not exist."""
    E, N = pk()
    (da, db, dc, dr), offs = PITCH_SETS[pset]
    M, Nn, K = ROW_SHAPES[si]
    es = 4 if dtype == torch.float32 else 2
    A, B = rd((M, K), dtype, 10 + si), rd((Nn, K), dtype, 20 + si, 1.0 / math.sqrt(K))
    Rd = rd((M, Nn), dtype, 30 + si)
    kw = epilogue_kw(epi, M, Nn, dtype, 100 * si)
    R0 = Rd if kw.get("res") else None
    ref = ref_of(A, B, M, Nn, K, kw, R0)
    reached, ran = set(), {}
    for algo in range(0, 14):
        # the dense, allocator-aligned call (guarded too)
        Cd = Guarded(M, Nn, Nn, dtype, DEV)
        dd = desc(E, A, B, Cd.view, M, Nn, K, R=R0, algo=algo, **kw)
        rc, name_d = kernel_name(N, dd)
        if rc == 0:
            launch(E, N, dd)
        sync()
        for oc, orr in offs:
            ga = Guarded(M, K, K + da, dtype, DEV, role="in", data=A)
            gb = Guarded(Nn, K, K + db, dtype, DEV, role="in", data=B)
            gc = Guarded(M, Nn, Nn + dc, dtype, DEV, lead=lead_for(Nn + dc, oc))
            gr = Guarded(M, Nn, Nn + dr, dtype, DEV, lead=lead_for(Nn + dr, orr), role="in", data=Rd) if R0 is not None else None
            dp = desc(E, ga.view, gb.view, gc.view, M, Nn, K, R=None if gr is None else gr.view, algo=algo, **kw)
            rcp, name_p = kernel_name(N, dp)
            what = (IDS[dtype], pset, (M, Nn, K), epi, algo, (oc, orr), name_p)
            if rc:                                              # the tile refuses the shape, pitched or not
                assert algo and rcp, what
                refused(N, lambda: launch(E, N, dp), gc)
                continue
            assert rcp == 0, what
            launch(E, N, dp)
            sync()
            try:
                for g in (ga, gb, gc, gr):
                    if g is not None:
                        g.check()
                assert_finite(gc.view)
                if algo or name_p == name_d:
                    assert_bits_equal(gc.dense(), Cd.dense())
                else:
                    close_to_ref(gc.view, ref, dtype, 4, what)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (what, e)) from None
            if algo:
                ran[algo] = name_p.split()[0]
            reached.add((name_p, vec_class(Nn + dc, gc.lead, es), vec_class(Nn + dr, gr.lead, es) if gr else None))
        if rc:
            Cd.all_poison()
        else:
            Cd.check()
            assert_finite(Cd.view)
            if algo == 0:
                close_to_ref(Cd.view, ref, dtype, 4, (epi, "dense"))
    print("reached", IDS[dtype], pset, (M, Nn, K), epi, sorted(reached, key=str))
    # what mlpk_gemm_kernel_name answered for the explicit tiles.  The five register-staged tiles take every shape.  The five LDS-DMA tiles and the
    # three "s3" tiles take K in whole half-slabs of 64 bytes (32 16-bit or 16 fp32 elements), in every dtype: K = 160 here, not 136 or 72.
    want = {a: "gemm_nt_kernel" for a in range(1, 6)}
    if K % (64 // es) == 0:
        want.update({a: "gemm_nt_glds_kernel" for a in range(6, 11)})
        want.update({a: "gemm_nt_s3_kernel" for a in range(11, 14)})
    assert ran == want, ran


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_gemm_residual_aliasing_the_pitched_output(dtype):
    """R == C in the pitched layout (the header allows it): the bits of the dense in-place call"""
    E, N = pk()
    M, Nn, K = 130, 72, 136
    A, B, C0 = rd((M, K), dtype, 1), rd((Nn, K), dtype, 2, 1.0 / math.sqrt(K)), rd((M, Nn), dtype, 3)
    bias = rd((Nn,), torch.float32, 4)
    for algo in (0, 1, 4, 5):
        for pad, off in ((8, 0), (4, 4), (2, 1)):
            def case(ops):
                a, b = ops.inp("A", A), ops.inp("B", B, pad=16)
                c = ops.inout("C", C0, pad=pad, off=off)
                E.gemm(a, b, c, M, Nn, K, bias=bias, R=c, res=1, algo=algo)
            got = both(case)
            if algo == 0:
                close_to_ref(got.g("C").view, ref_of(A, B, M, Nn, K, dict(bias=bias, res=1), C0), dtype, 4, (algo, pad, off))


@pytest.mark.parametrize("algo", [0, 1, 4, 5, 12, 13])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_gemm_token_transposed_pitched(dtype, algo):
    """OUT_TOKEN_T: the LDS-staged store (ldc, ldr multiples of 8, aligned), the 4-vector store (C at a lead of 4) and t_tokens > S, whose rows
    [S, t_tokens) of every image in C stay poison"""
    E, N = pk()
    for ci, (nimg, t_rows, S, K, t_tokens, dc, dr, oc) in enumerate([
            (2, 128, 49, 64, 49, 8, 24, 0), (2, 128, 49, 64, 49, 4, 24, 4), (3, 40, 20, 24, 23, 8, 24, 0), (3, 40, 20, 24, 23, 2, 1, 1)]):
        M = nimg * t_rows
        A, B = rd((M, K), dtype, 100 + ci), rd((S, K), dtype, 110 + ci, 1.0 / math.sqrt(K))
        bias, R0 = rd((S,), torch.float32, 120 + ci), rd((nimg * t_tokens, t_rows), dtype, 130 + ci)
        kw = dict(bias=bias, res=1, out_mode=N.OUT_TOKEN_T, t_rows=t_rows, t_tokens=t_tokens, algo=algo)
        names = {}

        def case(ops):
            a, b = ops.inp("A", A), ops.inp("B", B, pad=16)
            r = ops.inp("R", R0, pad=dr)
            c = ops.out("C", nimg * t_tokens, t_rows, dtype, pad=dc, off=oc, finite=False)
            d = desc(E, a, b, c, M, S, K, R=r, **kw)
            rc, names[ops.pitched] = kernel_name(N, d)
            if rc or not try_launch(E, N, d):                   # the tile refuses the shape or the dtype: nothing may be written
                sync()
                ops.g("C").all_poison()
                names[ops.pitched] = "refused"
                return lambda ops: None

            def post(ops):
                g = ops.g("C")
                v = g.view.reshape(nimg, t_tokens, t_rows)
                assert_finite(v[:, :S], "rows [0, S) of every image")
                for b_ in range(nimg):
                    if t_tokens > S:
                        g.still_poison(0, t_rows, b_ * t_tokens + S, (b_ + 1) * t_tokens)
            return post

        ref = gemm_ref(A.cpu(), B.cpu(), M, S, K, bias=bias.cpu(), R=R0.cpu(), res=1, out_mode=1, t_rows=t_rows, t_tokens=t_tokens)
        res = {}
        for pitched in (True, False):
            ops = Ops(pitched)
            post = case(ops)
            sync()
            ops.verify()
            post(ops)
            res[pitched] = ops
            if names[pitched] != "refused":                     # the project's tolerance: x 6 where the staged store can run, x 4 elsewhere
                got = ops.g("C").view.reshape(nimg, t_tokens, t_rows)[:, :S]
                close_to_ref(got, ref, dtype, 6 if t_rows % 64 == 0 else 4, (ci, pitched, names[pitched]))
        assert (names[True] == "refused") == (names[False] == "refused"), names
        # (c) holds where both layouts take the same store path.  The 16-bit staged store (whole tiles inside one image, 16-byte classes of C and R)
        # rounds the product to the storage type BEFORE the residual, the direct stores add the residual in fp32: one more rounding by design (the
        # x 6 of test_gemm_token_transposed_staged), so a lower alignment class legitimately changes the bits there and (d) applies alone.
        es = A.element_size()
        classes = (vec_class(t_rows + dc, lead_for(t_rows + dc, oc), es), vec_class(t_rows + dr, lead_for(t_rows + dr, 0), es))
        same_path = algo != 0 or names[True] == names[False]
        if same_path and (es == 4 or t_rows % 64 or classes == (2, 2)):
            assert_bits_equal(res[True].g("C").dense(), res[False].g("C").dense(), "C (case %d)" % ci)


def p8_operands(dtype, M, Nn, K, oc=0):
    A, B, R0 = rd((M, K), dtype, 1), rd((Nn, K), dtype, 2, 1.0 / math.sqrt(K)), rd((M, Nn), dtype, 3)
    ga = Guarded(M, K, K + 8, dtype, DEV, role="in", data=A)
    gb = Guarded(Nn, K, K + 64, dtype, DEV, role="in", data=B)
    gr = Guarded(M, Nn, Nn + 264, dtype, DEV, role="in", data=R0)
    mk_c = lambda: Guarded(M, Nn, Nn + 8, dtype, DEV, lead=lead_for(Nn + 8, oc))
    return (A, B, R0), (ga, gb, gr), mk_c


@pytest.mark.parametrize("tile", [14, 15], ids=["persistent", "generated"])
@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_gemm_persistent_and_generated_pitched(dtype, tile):
    """algo 14 (persistent tile; mixed tile heights at M = 320, staged epilogue at M = 512 with GELU + residual) and algo 15 (generated tile) on
    lda = K + 8, ldb = K + 64, ldc = N + 8, ldr = N + 264, row_part planes of pitch M + 5: the bits of algo 13 on the same operands, the pairs
    [M, row_part_ld) of every plane still poison"""
    E, N = pk()
    shapes = [(320, 256, 128), (512, 512, 192)]
    if tile == 15:                                              # the smallest shape the name query gives a generated variant for (no trial launches)
        shapes = []
        for M in (256, 512, 768):
            for Nn in (128, 256, 384):
                for K in (192, 256, 320, 384, 512, 768, 1024):
                    if not shapes:
                        _, (ga, gb, gr), mk_c = p8_operands(dtype, M, Nn, K)
                        bias = rd((Nn,), torch.float32, 4)
                        ok = True
                        for kw in (dict(act=1), dict(R=gr.view, res=1)):            # a variant for the GELU and for the residual class
                            rc, name = kernel_name(N, desc(E, ga.view, gb.view, mk_c().view, M, Nn, K, bias=bias, algo=15, **kw))
                            ok = ok and rc == 0 and "no variant" not in name
                        if ok:
                            shapes = [(M, Nn, K)]
        assert shapes, "no generated variant found by name query"
    bias_of = lambda Nn: rd((Nn,), torch.float32, 4)
    for M, Nn, K in shapes:
        (A, B, R0), (ga, gb, gr), mk_c = p8_operands(dtype, M, Nn, K)
        epis = [("bias_gelu", dict(bias=bias_of(Nn), act=1), False), ("bias_res", dict(bias=bias_of(Nn), res=1), False),
                ("bias_res_stats", dict(bias=bias_of(Nn), res=1), True)]
        ran15 = set()
        if M % 256 == 0:
            epis.append(("gelu_res", dict(act=1, res=1), False))
        for label, kw, stats in epis:
            out = {}
            for algo in (tile, 13):
                gc = mk_c()
                d = desc(E, ga.view, gb.view, gc.view, M, Nn, K, R=gr.view if kw.get("res") else None, algo=algo, **kw)
                gp = None
                if stats:
                    nparts = (Nn + 31) // 32
                    gp = Guarded(nparts, 2 * M, 2 * (M + 5), torch.float32, DEV)
                    d.row_part, d.row_part_ld = gp.view.data_ptr(), M + 5
                rc, name = kernel_name(N, d)
                what = (IDS[dtype], (M, Nn, K), label, algo, name)
                if tile == 15 and algo == 15 and (rc or "no variant" in name):      # no generated variant for this epilogue: refused, nothing written
                    refused(N, lambda: launch(E, N, d), *[g for g in (gc, gp) if g is not None])
                    print("refused", what)
                    continue
                assert rc == 0, what
                launch(E, N, d)
                sync()
                try:
                    for g in (ga, gb, gr, gc, gp):
                        if g is not None:
                            g.check()
                    assert_finite(gc.view)
                    if gp is not None:
                        assert_finite(gp.view, "row_part")
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (what, e)) from None
                out[algo] = (gc.dense(), None if gp is None else gp.dense())
                print("reached", what)
            if tile not in out:
                continue
            ran15.add(label)
            assert_bits_equal(out[tile][0], out[13][0], "C against algo 13")
            if stats:
                assert_bits_equal(out[tile][1], out[13][1], "row_part against algo 13")
            ref = ref_of(A, B, M, Nn, K, kw, R0 if kw.get("res") else None)
            close_to_ref(out[13][0], ref, dtype, 4, (label, "algo 13"))
        # the generated tile has no GELU + residual class (it refuses, above); with and without residual, with row_part it must have RUN
        assert ran15 >= {"bias_gelu", "bias_res", "bias_res_stats"}, ran15


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_gemm_persistent_tile_ineligible_at_a_c_lead_of_4(dtype):
    """C at a lead of 4 elements is 8-byte aligned only: the explicit algo 14 call is refused with nothing written, algo 0 falls back to another tile"""
    E, N = pk()
    M, Nn, K = 320, 256, 128
    (A, B, R0), (ga, gb, gr), mk_c = p8_operands(dtype, M, Nn, K, oc=4)
    bias = rd((Nn,), torch.float32, 4)
    gc = mk_c()
    d = desc(E, ga.view, gb.view, gc.view, M, Nn, K, bias=bias, R=gr.view, res=1, algo=14)
    refused(N, lambda: launch(E, N, d), gc)
    d = desc(E, ga.view, gb.view, gc.view, M, Nn, K, bias=bias, R=gr.view, res=1, algo=0)
    rc, name = kernel_name(N, d)
    assert rc == 0 and "p8" not in name, name
    launch(E, N, d)
    sync()
    for g in (ga, gb, gr, gc):
        g.check()
    assert_finite(gc.view)
    close_to_ref(gc.view, ref_of(A, B, M, Nn, K, dict(bias=bias, res=1), R0), dtype, 4, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_gemm_pair_two_slices_of_one_buffer(dtype):
    """mlpk_gemm_nt_pair the way Hire-MLP uses it: two pitched descriptors writing two column slices of ONE buffer; the bits of two calls, the gap
    between the slices still poison"""
    E, N = pk()
    M0, M1, Nn, K, gap = 256, 192, 128, 64, 8
    A0, A1 = rd((M0, K), dtype, 1), rd((M1, K), dtype, 2)
    B0, B1 = rd((Nn, K), dtype, 3, 0.125), rd((Nn, K), dtype, 4, 0.125)
    bias = rd((Nn,), torch.float32, 5)
    outs = {}
    for paired in (True, False):
        ga0, ga1 = Guarded(M0, K, K + 8, dtype, DEV, role="in", data=A0), Guarded(M1, K, K + 16, dtype, DEV, role="in", data=A1)
        gb0, gb1 = Guarded(Nn, K, K + 8, dtype, DEV, role="in", data=B0), Guarded(Nn, K, K + 24, dtype, DEV, role="in", data=B1)
        gc = Guarded(M0, 2 * Nn + gap, 2 * Nn + gap + 8, dtype, DEV)
        c0, c1 = gc.view[:, :Nn], gc.view[:M1, Nn + gap:]
        first = ((ga0.view, gb0.view, c0, M0, Nn, K), dict(bias=bias, act=1))
        second = ((ga1.view, gb1.view, c1, M1, Nn, K), dict(bias=bias))
        if paired:
            E.gemm_pair(first, second)
        else:
            E.gemm(*first[0], **first[1])
            E.gemm(*second[0], **second[1])
        sync()
        for g in (ga0, ga1, gb0, gb1, gc):
            g.check()
        gc.still_poison(Nn, Nn + gap)
        gc.still_poison(Nn + gap, 2 * Nn + gap, M1, M0)
        assert_finite(c0)
        assert_finite(c1)
        outs[paired] = (c0.clone(), c1.clone())
    assert_bits_equal(outs[True][0], outs[False][0], "first product")
    assert_bits_equal(outs[True][1], outs[False][1], "second product")


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_conv_gemm_pitched(dtype):
    """mlpk_conv_gemm_nhwc: Cin 32, 6 x 6 map, k3 s2 p1, ldc = N + 8 (the input is dense by contract: lead and tail guarded)"""
    E, N = pk()
    B_, H, W, Cin, Nn = 2, 6, 6, 32, 64
    x, w = rd((B_ * H * W, Cin), dtype, 1), rd((Nn, 9 * Cin), dtype, 2, 1.0 / math.sqrt(9 * Cin))
    bias = rd((Nn,), torch.float32, 3)

    def case(ops):
        E.conv_gemm_nhwc(ops.inp("x", x, pad=0), ops.inp("w", w, pad=16), ops.out("out", B_ * 3 * 3, Nn, dtype), B_, H, W, Cin, 3, 3, 2, 1, bias=bias)
    both(case)


def test_gemm_refusals():
    """ld < width, a pitch or base off the 16-byte grid of A / B, row_part_ld < M: MlpkError and a fully poisoned output"""
    E, N = pk()
    dtype, M, Nn, K = torch.bfloat16, 64, 64, 64
    A, B = rd((M, K + 16), dtype, 1), rd((Nn, K + 16), dtype, 2)
    gc = Guarded(M, Nn, Nn + 8, dtype, DEV)
    go = lambda **kw: (lambda: launch(E, N, desc(E, A, B, gc.view, M, Nn, K, **kw)))
    refused(N, go(lda=K - 8), gc)
    refused(N, go(ldb=K - 8), gc)
    refused(N, go(ldc=Nn - 1), gc)
    refused(N, go(lda=K + 4), gc)                               # pitch not a multiple of 16 bytes
    refused(N, lambda: launch(E, N, desc(E, A[:, 4:], B, gc.view, M, Nn, K)), gc)          # base 8 bytes off
    refused(N, lambda: launch(E, N, desc(E, A, B[:, 4:], gc.view, M, Nn, K)), gc)
    gp = Guarded(2, 2 * M, 2 * M, torch.float32, DEV)
    d = desc(E, A, B, gc.view, M, Nn, K, algo=13)
    d.row_part, d.row_part_ld = gp.view.data_ptr(), M - 1
    refused(N, lambda: launch(E, N, d), gc, gp)
    gt = Guarded(2 * 20, 32, 40, dtype, DEV)
    refused(N, lambda: launch(E, N, desc(E, A, B[:20], gt.view, M, 20, K, ldc=28, out_mode=N.OUT_TOKEN_T, t_rows=32, t_tokens=20)), gt)


# ------------------------------------------------------------------ statistics, normalisation, pooling
@pytest.mark.parametrize("length", [70, 200])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_row_stats_pitched(dtype, length):
    E, N = pk()
    rows = 37
    x = rd((rows, length), dtype, length) + 0.5
    # Rows longer than the short-row kernel's take 16-byte loads when base and pitch allow and element loads otherwise: two summation orders,
    # so (c) holds for the pitches in the dense call's alignment class and (d) for the others, with the tolerances of
    # test_gpu_ops.py::test_row_stats_and_norm_apply (|mean - ref| < 1e-5, |rstd - ref| < 1e-4).
    xd = x.double().cpu()
    mref, vref = xd.mean(1), xd.var(1, unbiased=False)
    for pad, off in ((8, 0), (4, 4), (2, 2), (1, 1)):
        def case(ops):
            E.row_stats(ops.inp("x", x, pad=pad, off=off), rows, length, length + pad if ops.pitched else length, ops.vec("mean", rows), ops.vec("rstd", rows))
        got = both(case, bits=(pad % 8 == 0 and off == 0))
        merr = (got.g("mean").view[0].double().cpu() - mref).abs().max().item()
        rerr = (got.g("rstd").view[0].double().cpu() - 1 / torch.sqrt(vref + 1e-5)).abs().max().item()
        assert merr < 1e-5 and rerr < 1e-4, (pad, off, merr, rerr)
    gm = Guarded(1, rows, rows, torch.float32, DEV)
    refused(N, lambda: E.row_stats(x, rows, length, length - 1, gm.view[0], gm.view[0]), gm)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_norm_apply_pitched(dtype):
    """all four outputs in one call, ld_rm, ld_tt, ld_p, ld_sum padded: out_tt's and out_ph / out_pw's pad columns exactly +0"""
    E, N = pk()
    B_, H, W, C, seg = 2, 5, 5, 64, 8
    S, rows, G = H * W, B_ * H * W, C // seg
    x = rd((rows, C), dtype, 1) + 0.25
    mean, rstd = x.float().mean(1).contiguous(), (x.float().var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3)
    sums = dtype != torch.float32

    def case(ops):
        p = ops.pitched
        xv = ops.inp("x", x)
        kw = {}
        if sums:
            kw = dict(sum_ph=ops.out("sum_ph", B_ * G, W * seg, torch.float32), sum_pw=ops.out("sum_pw", B_ * G, H * seg, torch.float32),
                      ld_sum=W * seg + (8 if p else 0))
        E.norm_apply(xv, rows, C, xv.stride(0), mean=mean, rstd=rstd, gamma=gamma, beta=beta, act=1,
                     out_rm=ops.out("rm", rows, C, dtype, pad=16), ld_rm=C + (16 if p else 0),
                     out_tt=ops.out("tt", B_ * C, S, dtype, pad=15, dpad=7, zero_pad=True), S=S, ld_tt=S + (15 if p else 7),
                     out_ph=ops.out("ph", B_ * W * G, H * seg, dtype, zero_pad=True), out_pw=ops.out("pw", B_ * H * G, W * seg, dtype, zero_pad=True),
                     H=H, W=W, seg=seg, ld_p=H * seg + (8 if p else 0), **kw)
    both(case)
    go = Guarded(rows, C, C + 8, dtype, DEV)
    refused(N, lambda: E.norm_apply(x, rows, C, C - 8, out_rm=go.view, ld_rm=C + 8), go)
    refused(N, lambda: E.norm_apply(x, rows, C, C, out_rm=go.view, ld_rm=C - 8), go)
    # a bad pitch of ONE output refuses the whole call before anything is launched: the valid outputs stay poison too (the checks of out_ph /
    # out_pw used to come after the launch that writes out_rm / out_tt)
    gt, gp, gq = Guarded(B_ * C, S, S + 7, dtype, DEV), Guarded(B_ * W * G, H * seg, H * seg + 8, dtype, DEV), Guarded(B_ * H * G, W * seg, W * seg + 8, dtype, DEV)
    ok = dict(out_rm=go.view, ld_rm=C + 8, out_tt=gt.view, S=S, ld_tt=S + 7, out_ph=gp.view, out_pw=gq.view, H=H, W=W, seg=seg, ld_p=H * seg + 8)
    refused(N, lambda: E.norm_apply(x, rows, C, C, **dict(ok, ld_p=H * seg - 8)), go, gt, gp, gq)
    refused(N, lambda: E.norm_apply(x, rows, C, C, **dict(ok, ld_tt=S - 1)), go, gt, gp, gq)
    refused(N, lambda: E.norm_apply(x, rows, C, C, **dict(ok, out_pw=None, seg=7)), go, gt, gp, gq)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_layernorm_transpose_pitched(dtype):
    E, N = pk()
    nimg, S, C = 2, 49, 128
    x = rd((nimg * S, C), dtype, 1) + 0.25
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3)

    def case(ops):
        o = ops.out("tt", nimg * C, S, dtype, pad=15, dpad=7, zero_pad=True)            # (ld_tt % 8 == 0 holds for the dense twin too)
        E.layernorm_transpose(ops.inp("x", x), nimg, S, C, gamma, beta, o, o.stride(0))
    both(case)
    gt = Guarded(nimg * C, S, S + 15, dtype, DEV)
    refused(N, lambda: E.layernorm_transpose(x, nimg, S, C, gamma, beta, gt.view, S + 11), gt)             # ld_tt % 8
    refused(N, lambda: E.layernorm_transpose(x[:, 4:], nimg, S, C, gamma, beta, gt.view, S + 15), gt)      # x 8 bytes off (and C no multiple of 128)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_pool_mean_pitched(dtype):
    E, N = pk()
    B_, S, C = 3, 21, 72
    x = rd((B_ * S, C), dtype, 1)
    mean, rstd = x.float().mean(1).contiguous(), (x.float().var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3)
    for ln in (False, True):
        for opad, ooff in ((8, 0), (4, 4), (1, 1)):
            def case(ops):
                xv, o = ops.inp("x", x), ops.out("out", B_, C, dtype, pad=opad, off=ooff)
                kw = dict(mean=mean, rstd=rstd, gamma=gamma, beta=beta) if ln else {}
                E.pool_mean(xv, B_, S, C, xv.stride(0), o, o.stride(0), **kw)
            both(case)
    go = Guarded(B_, C, C + 8, dtype, DEV)
    refused(N, lambda: E.pool_mean(x, B_, S, C, C, go.view, C - 1), go)
    refused(N, lambda: E.pool_mean(x, B_, S, C, C - 8, go.view, C + 8), go)


def test_stats_finalize_planar_pitched():
    """plane_stride > rows: the pairs behind the rows of every plane are NaN and must not be read"""
    E, N = pk()
    rows, nplanes, count = 50, 3, 96
    v = rd((rows, count), torch.float32, 1) + 0.5
    parts = torch.stack([torch.stack([v[:, 32 * q:32 * q + 32].sum(1), (v[:, 32 * q:32 * q + 32] ** 2).sum(1)], dim=1).reshape(-1) for q in range(nplanes)])

    def case(ops):
        p = ops.inp("part", parts, pad=14)
        N.check(N.lib().mlpk_stats_finalize_planar(p.data_ptr(), rows, nplanes, p.stride(0) // 2, 1, count, 1e-5, ops.vec("mean", rows).data_ptr(),
                                                   ops.vec("rstd", rows).data_ptr(), E.stream()), "mlpk_stats_finalize_planar")
    both(case)
    gm = Guarded(1, rows, rows, torch.float32, DEV)
    refused(N, lambda: N.check(N.lib().mlpk_stats_finalize_planar(parts.data_ptr(), rows, nplanes, rows - 1, 1, count, 1e-5, gm.view.data_ptr(),
                                                                  gm.view.data_ptr(), E.stream()), "mlpk_stats_finalize_planar"), gm)


# ------------------------------------------------------------------ split attention and the remaps
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["none", "s2", "s2_ref"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_split_attention_pitched(dtype, mode):
    """the three branches as column slices of one (rows, 3C + 8) buffer"""
    E, N = pk()
    B_, H, W, C = 2, 5, 6, 40
    rows = B_ * H * W
    x = rd((rows, 3 * C), dtype, 1)
    bar = torch.softmax(rd((B_, 3, C), torch.float32, 2), dim=1).contiguous()

    def case(ops):
        xv = ops.inp("x", x)
        ld = xv.stride(0)
        x0, x1, x2 = xv[:, :C], xv[:, C:2 * C], xv[:, 2 * C:]
        E.split_sum(x0, x1, x2, ld, ld, ld, B_, H, W, C, mode, ops.vec("a", B_ * C))
        o = ops.out("out", rows, C, dtype, pad=16)
        E.split_apply(x0, x1, x2, ld, ld, ld, B_, H, W, C, mode, bar, o, o.stride(0))
    both(case)
    go, ga = Guarded(rows, C, C + 8, dtype, DEV), Guarded(1, B_ * C, B_ * C, torch.float32, DEV)
    refused(N, lambda: E.split_sum(x, x, x, 3 * C, C - 1, 3 * C, B_, H, W, C, mode, ga.view), ga)
    refused(N, lambda: E.split_apply(x, x, x, 3 * C, 3 * C, 3 * C, B_, H, W, C, mode, bar, go.view, C - 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_vip_unpermute_pitched(dtype):
    E, N = pk()
    B_, H, W, C, seg = 2, 5, 6, 32, 8
    G = C // seg
    for which, (zr, zc) in enumerate(((B_ * W * G, H * seg), (B_ * H * G, W * seg))):
        z = rd((zr, zc), dtype, 1 + which)

        def case(ops):
            zv = ops.inp("z", z)
            E.vip_unpermute(which, zv, ops.out("out", B_ * H * W, C, dtype, pad=0), B_, H, W, C, seg, zv.stride(0))
        both(case)
        go = Guarded(B_ * H * W, C, C, dtype, DEV)
        refused(N, lambda: E.vip_unpermute(which, z, go.view, B_, H, W, C, seg, zc - 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_s2_shift_pitched(dtype):
    E, N = pk()
    B_, H, W, C = 2, 5, 6, 40
    x = rd((B_ * H * W, C), dtype, 1)
    for mode in (0, 1, 2):
        for pad, off in ((8, 0), (4, 4), (2, 2), (1, 1)):
            def case(ops):
                xv, o = ops.inp("x", x, pad=pad, off=off), ops.out("out", B_ * H * W, C, dtype, pad=pad + 8, off=off)
                E.s2_shift(xv, o, B_, H, W, C, xv.stride(0), o.stride(0), mode)
            both(case)
    go = Guarded(B_ * H * W, C, C + 8, dtype, DEV)
    refused(N, lambda: E.s2_shift(x, go.view, B_, H, W, C, C - 1, C + 8, 1), go)
    refused(N, lambda: E.s2_shift(x, go.view, B_, H, W, C, C, C - 1, 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_s2_shift2_pitched(dtype):
    E, N = pk()
    B_, D1, D2, C = 2, 5, 6, 40
    x = rd((B_ * D1 * D2, C), dtype, 1)
    call = lambda which, mode, adj, xv, ldi, o, ldo: N.check(N.lib().mlpk_s2_shift2(E.dtype_code(dtype), which, mode, adj, xv.data_ptr(), ldi, o.data_ptr(), ldo,
                                                                                   B_, D1, D2, C, E.stream()), "mlpk_s2_shift2")
    for which in (1, 2):
        for mode, adj in ((0, 0), (1, 0), (0, 1)):
            def case(ops):
                xv, o = ops.inp("x", x), ops.out("out", B_ * D1 * D2, C, dtype, pad=4, off=4)
                call(which, mode, adj, xv, xv.stride(0), o, o.stride(0))
            both(case)
    go = Guarded(B_ * D1 * D2, C, C + 8, dtype, DEV)
    refused(N, lambda: call(1, 0, 0, x, C - 1, go.view, C + 8), go)
    refused(N, lambda: call(1, 0, 0, x, C, go.view, C - 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_cycle_shift_pitched(dtype):
    """out_h / out_w as two column slices of one buffer; the LayerNorm form for the 16-bit types"""
    E, N = pk()
    B_, H, W, C = 2, 5, 6, 40
    rows = B_ * H * W
    x = rd((rows, C), dtype, 1) + 0.25
    mean, rstd = x.float().mean(1).contiguous(), (x.float().var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3)
    for ln in ((False, True) if dtype != torch.float32 else (False,)):
        for k in (3, 7):
            def case(ops):
                xv, o = ops.inp("x", x), ops.out("out", rows, 2 * C, dtype)
                if ln:
                    E.cycle_shift_ln(xv, mean, rstd, gamma, beta, o[:, :C], o[:, C:], B_, H, W, C, k, xv.stride(0), o.stride(0))
                else:
                    E.cycle_shift(xv, o[:, :C], o[:, C:], B_, H, W, C, k, xv.stride(0), o.stride(0))
            both(case)
    go = Guarded(rows, C, C + 8, dtype, DEV)
    refused(N, lambda: E.cycle_shift(x, go.view, None, B_, H, W, C, 3, C - 1, C + 8), go)
    refused(N, lambda: E.cycle_shift(x, go.view, None, B_, H, W, C, 3, C, C - 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_hire_remaps_pitched(dtype):
    """gather(_ln) into padded a_h / a_w, combine(_from / _stats) from padded y_h / y_w (x and src are dense by contract: lead and tail guarded)"""
    E, N = pk()
    B_, H, W, C, h, w = 2, 7, 6, 32, 2, 2
    Hp, Wp = H + (h - H % h), W + (w - W % w)
    gh, gw = Hp // h, Wp // w
    rows = B_ * H * W
    x = rd((rows, C), dtype, 1) + 0.25
    mean, rstd = x.float().mean(1).contiguous(), (x.float().var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3)
    yh, yw = rd((B_ * gh * W, h * C), dtype, 4), rd((B_ * H * gw, w * C), dtype, 5)
    for step in (0, 1):
        for ln in ((False, True) if dtype != torch.float32 else (False,)):
            def gather(ops):
                xv = ops.inp("x", x, pad=0)
                ah, aw = ops.out("a_h", B_ * gh * W, h * C, dtype), ops.out("a_w", B_ * H * gw, w * C, dtype, pad=16)
                if ln:
                    E.hire_gather_ln(xv, mean, rstd, gamma, beta, ah, aw, B_, H, W, C, h, w, step, ah.stride(0), aw.stride(0))
                else:
                    E.hire_gather(xv, ah, aw, B_, H, W, C, h, w, step, ah.stride(0), aw.stride(0))
            both(gather)
        for form in ((0, 1, 2) if dtype != torch.float32 else (0, 1)):
            def combine(ops):
                xv = ops.inout("x", x, pad=0)
                a, b = ops.inp("y_h", yh), ops.inp("y_w", yw, pad=16)
                if form == 0:
                    E.hire_combine(xv, a, b, B_, H, W, C, h, w, step, a.stride(0), b.stride(0))
                elif form == 1:
                    E.hire_combine_from(xv, ops.inp("src", x * 0.5, pad=0), a, b, B_, H, W, C, h, w, step, a.stride(0), b.stride(0))
                else:
                    E.hire_combine_stats(xv, ops.inp("src", x * 0.5, pad=0), a, b, B_, H, W, C, h, w, step, a.stride(0), b.stride(0),
                                         ops.vec("mean", rows), ops.vec("rstd", rows))
            both(combine)
    ga, gw_ = Guarded(B_ * gh * W, h * C, h * C + 8, dtype, DEV), Guarded(B_ * H * gw, w * C, w * C + 8, dtype, DEV)
    refused(N, lambda: E.hire_gather(x, ga.view, gw_.view, B_, H, W, C, h, w, 0, h * C - 8, w * C + 8), ga, gw_)
    refused(N, lambda: E.hire_gather(x, ga.view, gw_.view, B_, H, W, C, h, w, 0, h * C + 8, w * C - 8), ga, gw_)
    gx = Guarded(rows, C, C, dtype, DEV)
    refused(N, lambda: E.hire_combine(gx.view, yh, yw, B_, H, W, C, h, w, 0, h * C - 8, w * C), gx)
    refused(N, lambda: E.hire_combine_from(gx.view, x, yh, yw, B_, H, W, C, h, w, 0, h * C, w * C - 8), gx)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_patchify_im2col_pitched(dtype):
    """ldo = K + 8: the pad columns [K, ldo) exactly +0; the NHWC source with a pixel stride of Cin + 8"""
    E, N = pk()
    B_, Cin, H, W = 2, 3, 8, 12
    src = rd((B_ * Cin * H, W), torch.float32, 1)                # NCHW, fp32 source converted on load
    nhwc = rd((B_ * H * W, Cin + 5), dtype, 2)

    def case_patchify(ops):
        K = Cin * 16
        o = ops.out("out", B_ * 2 * 3, K, dtype, zero_pad=True)
        E.patchify(ops.inp("src", src, pad=0), o, B_, Cin, H, W, 4, 4, 0, o.stride(0))
    both(case_patchify)

    def case_patchify_nhwc(ops):
        K = (Cin + 5) * 4
        sv = ops.inp("src", nhwc)
        o = ops.out("out", B_ * 4 * 6, K, dtype, zero_pad=True)
        E.patchify(sv, o, B_, Cin + 5, H, W, 2, 2, 0, o.stride(0), layout=N.LAYOUT_NHWC, px_stride=sv.stride(0), order=1)
    both(case_patchify_nhwc)

    def case_im2col(ops):
        K = (Cin + 5) * 9
        sv = ops.inp("src", nhwc)
        o = ops.out("out", B_ * 4 * 6, K, dtype, zero_pad=True)
        E.im2col(sv, o, B_, Cin + 5, H, W, 3, 3, 2, 2, 1, o.stride(0), layout=N.LAYOUT_NHWC, px_stride=sv.stride(0))
    both(case_im2col)

    def case_im2col_nchw(ops):
        K = Cin * 16
        o = ops.out("out", B_ * 4 * 6, K, dtype, pad=16, zero_pad=True)
        E.im2col(ops.inp("src", src, pad=0), o, B_, Cin, H, W, 4, 4, 2, 2, 1, o.stride(0))
    both(case_im2col_nchw)
    go = Guarded(B_ * 4 * 6, Cin * 16, Cin * 16 + 8, dtype, DEV)
    refused(N, lambda: E.patchify(src, go.view, B_, Cin, H, W, 4, 4, 0, Cin * 16 - 8), go)                                   # ldo < K
    refused(N, lambda: E.im2col(src, go.view, B_, Cin, H, W, 4, 4, 2, 2, 1, Cin * 16 - 8), go)
    refused(N, lambda: E.im2col(nhwc, go.view, B_, Cin + 5, H, W, 3, 3, 2, 2, 1, 80, layout=N.LAYOUT_NHWC, px_stride=Cin + 4), go)   # pixel stride < Cin


# ------------------------------------------------------------------ element-wise and column reductions
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_add_periodic_pitched(dtype):
    E, N = pk()
    rows, C, period = 30, 40, 10
    x, t = rd((rows, C), dtype, 1), rd((period, C), torch.float32, 2)
    for pad, off in ((8, 0), (4, 4), (2, 2), (1, 1)):
        def case(ops):
            xv = ops.inout("x", x, pad=pad, off=off)
            E.add_periodic(xv, xv.stride(0), t, rows, C, period)
        both(case)
    gx = Guarded(rows, C, C + 8, dtype, DEV)
    refused(N, lambda: E.add_periodic(gx.view, C - 1, t, rows, C, period), gx)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_dropout_pitched(dtype):
    """ldx != ldy; the mask of the dense call (the bits are compared, zeros included); in place with one pitch"""
    E, N = pk()
    rows, cols = 33, 44
    x = rd((rows, cols), dtype, 1) + 3.0

    def case(ops):
        E.dropout(ops.inp("x", x, pad=4, off=4), ops.out("y", rows, cols, dtype, pad=9, off=1), rows, cols, 0.3, 1234, 7)
    got = both(case)
    kept = (got.g("y").view != 0).float().mean().item()
    assert 0.6 < kept < 0.8, kept

    def inplace(ops):
        xv = ops.inout("x", x, pad=2, off=2)
        E.dropout(xv, xv, rows, cols, 0.3, 1234, 7)
    assert_bits_equal(both(inplace).g("x").dense(), got.g("y").dense(), "in place")
    gy = Guarded(rows, cols, cols + 8, dtype, DEV)
    bad = lambda ldx, ldy: (lambda: N.check(N.lib().mlpk_dropout(E.dtype_code(dtype), x.data_ptr(), ldx, gy.view.data_ptr(), ldy, rows, cols, 0.3, 1, 1,
                                                                 E.stream()), "mlpk_dropout"))
    refused(N, bad(cols - 1, cols + 8), gy)
    refused(N, bad(cols, cols - 1), gy)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_ew_cols_pitched(dtype, mode):
    """all six modes with lda, ldb, ldo all different"""
    E, N = pk()
    rows, cols, period = 30, 44, 10
    a, b = rd((rows, cols), dtype, 1), rd((rows, cols), dtype, 2)
    n = {3: rows // period, 5: rows // period * cols}.get(mode, cols)
    g, h, k = rd((n,), torch.float32, 3), rd((n if mode == 5 else cols,), torch.float32, 4), rd((cols,), torch.float32, 5)
    call = lambda av, lda, bv, ldb, ov, ldo: N.check(N.lib().mlpk_ew_cols(E.dtype_code(dtype), mode, av.data_ptr(), lda, bv.data_ptr(), ldb, g.data_ptr(),
                                                                         h.data_ptr(), k.data_ptr(), ov.data_ptr(), ldo, rows, cols, period, E.stream()),
                                                     "mlpk_ew_cols")
    for offs in ((0, 0, 0), (4, 2, 1)):
        def case(ops):
            av, bv = ops.inp("a", a, pad=8, off=offs[0]), ops.inp("b", b, pad=3, off=offs[1])
            o = ops.out("out", rows, cols, dtype, pad=13, off=offs[2])
            call(av, av.stride(0), bv, bv.stride(0), o, o.stride(0))
        both(case)
    go = Guarded(rows, cols, cols + 8, dtype, DEV)
    refused(N, lambda: call(a, cols - 1, b, cols, go.view, cols + 8), go)
    refused(N, lambda: call(a, cols, b, cols - 1, go.view, cols + 8), go)
    refused(N, lambda: call(a, cols, b, cols, go.view, cols - 1), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_column_reductions_pitched(dtype):
    """mlpk_col_sum (plain, squared, with `sub`), mlpk_col_dot, mlpk_col_dot_seg"""
    E, N = pk()
    segs, seg_rows, cols = 3, 70, 44
    rows = segs * seg_rows
    x, y = rd((rows, cols), dtype, 1), rd((rows, cols), dtype, 2)
    L, dc = N.lib(), E.dtype_code(dtype)
    for pad, off in ((8, 0), (4, 4), (1, 1)):
        def case(ops):
            xv, yv = ops.inp("x", x, pad=pad, off=off), ops.inp("y", y, pad=pad, off=off)
            ld = xv.stride(0)
            N.check(L.mlpk_col_sum(dc, xv.data_ptr(), None, rows, cols, ld, 0, ops.vec("sum", cols).data_ptr(), E.stream()), "mlpk_col_sum")
            N.check(L.mlpk_col_sum(dc, xv.data_ptr(), None, rows, cols, ld, 1, ops.vec("sq", cols).data_ptr(), E.stream()), "mlpk_col_sum")
            N.check(L.mlpk_col_sum(dc, xv.data_ptr(), yv.data_ptr(), rows, cols, ld, 0, ops.vec("sub", cols).data_ptr(), E.stream()), "mlpk_col_sum")
            N.check(L.mlpk_col_dot(dc, xv.data_ptr(), ld, yv.data_ptr(), ld, rows, cols, ops.vec("dot", cols).data_ptr(), E.stream()), "mlpk_col_dot")
            N.check(L.mlpk_col_dot_seg(dc, xv.data_ptr(), ld, yv.data_ptr(), ld, segs, seg_rows, cols, ops.vec("seg", segs * cols).data_ptr(), E.stream()),
                    "mlpk_col_dot_seg")
        both(case)
    go = Guarded(1, segs * cols, segs * cols, torch.float32, DEV)
    p = go.view.data_ptr()
    refused(N, lambda: N.check(L.mlpk_col_sum(dc, x.data_ptr(), None, rows, cols, cols - 1, 0, p, E.stream()), "mlpk_col_sum"), go)
    refused(N, lambda: N.check(L.mlpk_col_dot(dc, x.data_ptr(), cols, y.data_ptr(), cols - 1, rows, cols, p, E.stream()), "mlpk_col_dot"), go)
    refused(N, lambda: N.check(L.mlpk_col_dot_seg(dc, x.data_ptr(), cols - 1, y.data_ptr(), cols, segs, seg_rows, cols, p, E.stream()), "mlpk_col_dot_seg"), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_gelu_elementwise_pitched(dtype):
    """one pitch for a, b and out: they are three column slices of one padded buffer, as the train-mode MLP keeps them"""
    E, N = pk()
    rows, cols = 30, 44
    ab = rd((rows, 2 * cols), dtype, 1)
    L, dc = N.lib(), E.dtype_code(dtype)
    for mode in (0, 1):
        for pad, off in ((8, 0), (3, 1)):
            def case(ops):
                v = ops.inout("buf", torch.cat([ab, torch.zeros((rows, cols), dtype=dtype, device=DEV)], dim=1), pad=pad, off=off)
                N.check(L.mlpk_gelu_elementwise(dc, mode, v.data_ptr(), v[:, cols:].data_ptr() if mode else None, v[:, 2 * cols:].data_ptr(), rows, cols,
                                                v.stride(0), E.stream()), "mlpk_gelu_elementwise")

                def post(ops):
                    assert_bits_equal(ops.g("buf").view[:, :2 * cols].contiguous(), ab, "a | b")
                return post
            both(case)
    go = Guarded(rows, cols, cols + 8, dtype, DEV)
    refused(N, lambda: N.check(L.mlpk_gelu_elementwise(dc, 0, ab.data_ptr(), None, go.view.data_ptr(), rows, cols, cols - 1, E.stream()), "gelu"), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_transpose_batched_pitched(dtype):
    """ld_in, ld_out, ld_res all different; the padding columns [R, ld_out) of out are NOT written: still poison"""
    E, N = pk()
    batch, R, Cc = 3, 21, 40
    x, res = rd((batch * R, Cc), dtype, 1), rd((batch * Cc, R), dtype, 2)
    L, dc = N.lib(), E.dtype_code(dtype)
    for with_res in (False, True):
        for offs in ((0, 0, 0), (4, 1, 2)):
            def case(ops):
                xv, o = ops.inp("in", x, pad=8, off=offs[0]), ops.out("out", batch * Cc, R, dtype, pad=11, off=offs[1])
                rv = ops.inp("res", res, pad=3, off=offs[2]) if with_res else None
                N.check(L.mlpk_transpose_batched(dc, xv.data_ptr(), xv.stride(0), o.data_ptr(), o.stride(0), rv.data_ptr() if with_res else None,
                                                 rv.stride(0) if with_res else 0, batch, R, Cc, E.stream()), "mlpk_transpose_batched")
            both(case)
    go = Guarded(batch * Cc, R, R + 8, dtype, DEV)
    for ld_in, ld_out, ld_res in ((Cc - 1, R + 8, R), (Cc, R - 1, R), (Cc, R + 8, R - 1)):
        refused(N, lambda: N.check(L.mlpk_transpose_batched(dc, x.data_ptr(), ld_in, go.view.data_ptr(), ld_out, res.data_ptr(), ld_res, batch, R, Cc,
                                                            E.stream()), "mlpk_transpose_batched"), go)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_layernorm_backward_pitched(dtype):
    """ldx, lddy, lddx all different, bases at 0 / 4 / odd offsets"""
    E, N = pk()
    rows, C = 70, 72
    x, dy = rd((rows, C), dtype, 1) + 0.25, rd((rows, C), dtype, 2)
    mean, rstd = x.float().mean(1).contiguous(), (x.float().var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma = rd((C,), torch.float32, 3) * 0.2 + 1
    L, dc = N.lib(), E.dtype_code(dtype)
    blocks = L.mlpk_layernorm_backward_blocks(rows)
    call = lambda xv, ldx, dv, lddy, o, lddx, part: N.check(L.mlpk_layernorm_backward(dc, xv.data_ptr(), ldx, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                                                     dv.data_ptr(), lddy, o.data_ptr(), lddx, part.data_ptr(), rows, C,
                                                                                     E.stream()), "mlpk_layernorm_backward")
    for offs in ((0, 0, 0), (4, 1, 2)):
        def case(ops):
            xv, dv = ops.inp("x", x, pad=8, off=offs[0]), ops.inp("dy", dy, pad=3, off=offs[1])
            o = ops.out("dx", rows, C, dtype, pad=13, off=offs[2])
            call(xv, xv.stride(0), dv, dv.stride(0), o, o.stride(0), ops.vec("part", blocks * 2 * C))
        both(case)
    go, gp = Guarded(rows, C, C + 8, dtype, DEV), Guarded(1, blocks * 2 * C, blocks * 2 * C, torch.float32, DEV)
    refused(N, lambda: call(x, C - 1, dy, C, go.view, C + 8, gp.view), go, gp)
    refused(N, lambda: call(x, C, dy, C - 1, go.view, C + 8, gp.view), go, gp)
    refused(N, lambda: call(x, C, dy, C, go.view, C - 1, gp.view), go, gp)


# ------------------------------------------------------------------ the fused kernels, weights packed by the engine's own helpers
def row_ln(x):
    f = x.float()
    return f.mean(1).contiguous(), (f.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_token_gemm_pitched(dtype):
    """mlpk_token_gemm: xt is dense by contract (its pitch IS the K of the product: lead and tail guarded); R a column slice of a wider padded
    tensor (gMLP's gate), out padded; in place with R == out (ResMLP)"""
    E, N = pk()
    B_, C, S = 2, 64, 49
    sp = E.round_up(S, 32)
    xt = torch.zeros((B_ * C, sp), dtype=dtype, device=DEV)
    xt[:, :S] = rd((B_ * C, S), dtype, 1)
    wp, bp, ng = E.pack_token_gemm(rnd((S, S), torch.float32, 2, 1.0 / math.sqrt(S)), rnd((S,), torch.float32, 3), dtype, DEV)
    wide, g1 = rd((B_ * S, 2 * C), dtype, 4), rd((C,), torch.float32, 5) * 0.3 + 0.5

    def gate(ops):
        r, o = ops.inp("wide", wide), ops.out("out", B_ * S, C, dtype, pad=24)
        E.token_gemm(ops.inp("xt", xt, pad=0), sp, B_ * C, S, wp, bp, ng, o, o.stride(0), C, R=r[:, :C], ldr=r.stride(0), res=N.RES_MUL)
    both(gate)

    def inplace(ops):
        x = ops.inout("x", wide[:, :C].contiguous())
        E.token_gemm(ops.inp("xt", xt, pad=0), sp, B_ * C, S, wp, bp, ng, x, x.stride(0), C, R=x, ldr=x.stride(0), res=N.RES_ADD, rscale=g1, rperiod=C)
    both(inplace)
    go = Guarded(B_ * S, C, C + 8, dtype, DEV)
    refused(N, lambda: E.token_gemm(xt, sp, B_ * C, S, wp, bp, ng, go.view, C - 8, C), go)                                   # ldo < C
    refused(N, lambda: E.token_gemm(xt, sp, B_ * C, S, wp, bp, ng, go.view, C + 8, C, R=wide, ldr=C - 8, res=N.RES_MUL), go)  # ldr < C


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_token_gemm_ln_pitched(dtype):
    """mlpk_token_gemm_ln(_post): x a column slice at channel offset 32 of a wider padded tensor, as the header promises; out == x under
    RES_ADD_AFFINE (the rest of the wider tensor bit-unchanged); the post affine on the pipelined kernel"""
    E, N = pk()
    B_, C, S = 2, 64, 98
    wide = rd((B_ * S, 32 + C + 16), dtype, 1) + 0.25
    xs = wide[:, 32:32 + C]
    mean, rstd = row_ln(xs)
    gamma, beta = rd((C,), torch.float32, 2) * 0.2 + 1, rd((C,), torch.float32, 3) * 0.2
    g1, ps, ph = rd((C,), torch.float32, 5) * 0.3 + 0.5, rd((C,), torch.float32, 6) * 0.2 + 1, rd((C,), torch.float32, 7) * 0.2
    wp, bp, ng = E.pack_token_gemm(rnd((S, S), torch.float32, 4, 1.0 / math.sqrt(S)), rnd((S,), torch.float32, 8), dtype, DEV)
    R0 = rd((B_ * S, C), dtype, 9)
    assert E.token_gemm_ln_post_supported(dtype, S, C, wide.shape[1] + 8)
    for post in (None, (ps, ph)):
        def gate(ops):
            w, r, o = ops.inp("wide", wide), ops.inp("R", R0, pad=16), ops.out("out", B_ * S, C, dtype, pad=24)
            E.token_gemm_ln(w[:, 32:32 + C], w.stride(0), B_ * C, S, mean, rstd, gamma, beta, wp, bp, ng, o, o.stride(0), C, R=r, ldr=r.stride(0),
                            res=N.RES_MUL, post=post)
        both(gate)

        def affine_inplace(ops):
            w = ops.inout("wide", wide)
            x = w[:, 32:32 + C]
            E.token_gemm_ln(x, w.stride(0), B_ * C, S, None, None, gamma, beta, wp, bp, ng, x, w.stride(0), C, R=x, ldr=w.stride(0),
                            res=N.RES_ADD_AFFINE, rscale=g1, rperiod=C, post=post)

            def untouched(ops):
                v = ops.g("wide").view
                assert_bits_equal(v[:, :32].contiguous(), wide[:, :32].contiguous(), "channels in front of the slice")
                assert_bits_equal(v[:, 32 + C:].contiguous(), wide[:, 32 + C:].contiguous(), "channels behind the slice")
            return untouched
        both(affine_inplace)
    go = Guarded(B_ * S, C, C + 8, dtype, DEV)
    refused(N, lambda: E.token_gemm_ln(xs, C - 8, B_ * C, S, mean, rstd, gamma, beta, wp, bp, ng, go.view, C + 8, C), go)       # ldx < t_rows
    refused(N, lambda: E.token_gemm_ln(xs, wide.stride(0), B_ * C, S, mean, rstd, gamma, beta, wp, bp, ng, go.view, C - 8, C), go)   # ldo < t_rows


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_channel_mlp_pitched(dtype):
    """mlpk_channel_mlp: ldx, ldr, ldo all different; out == x == R; the by-product row_part guarded"""
    E, N = pk()
    C, hid, M = 64, 256, 300
    x, other = rd((M, C), dtype, 1) * 1.5 + 0.25, rd((M, C), dtype, 2)
    mean, rstd = row_ln(x)
    pack = E.pack_channel_mlp_fused(rnd((hid, C), torch.float32, 3, 1.0 / math.sqrt(C)), rnd((hid,), torch.float32, 4, 0.3),
                                    rnd((C, hid), torch.float32, 5, 1.0 / math.sqrt(hid)), rnd((C,), torch.float32, 6, 0.3), dtype, DEV,
                                    rd((C,), torch.float32, 7) * 0.3 + 1, rd((C,), torch.float32, 8) * 0.2)
    w1p, b1p, csum, w2p, b2p, nch = pack

    def call(xv, rv, ov, part, w2v=w2p):
        N.check(N.lib().mlpk_channel_mlp(E.dtype_code(dtype), xv.data_ptr(), xv.stride(0), M, C, mean.data_ptr(), rstd.data_ptr(), 1, csum.data_ptr(),
                                         w1p.data_ptr(), w1p.stride(0), b1p.data_ptr(), w2v.data_ptr(), w2v.stride(0), b2p.data_ptr(), nch,
                                         None if rv is None else rv.data_ptr(), 0 if rv is None else rv.stride(0), ov.data_ptr(), ov.stride(0),
                                         part.data_ptr(), E.stream()), "mlpk_channel_mlp")

    def three_pitches(ops):
        call(ops.inp("x", x), ops.inp("R", other, pad=16), ops.out("out", M, C, dtype, pad=24), ops.vec("row_part", 2 * M), ops.inp("w2", w2p, pad=32))
    both(three_pitches)

    def inplace(ops):
        xv = ops.inout("x", x, pad=24)
        call(xv, xv, xv, ops.vec("row_part", 2 * M))
    both(inplace)
    go, gp = Guarded(M, C, C + 8, dtype, DEV), Guarded(1, 2 * M, 2 * M, torch.float32, DEV)
    bad = lambda ldx, ldr, ldo: (lambda: N.check(N.lib().mlpk_channel_mlp(
        E.dtype_code(dtype), x.data_ptr(), ldx, M, C, mean.data_ptr(), rstd.data_ptr(), 1, csum.data_ptr(), w1p.data_ptr(), w1p.stride(0), b1p.data_ptr(),
        w2p.data_ptr(), w2p.stride(0), b2p.data_ptr(), nch, other.data_ptr(), ldr, go.view.data_ptr(), ldo, gp.view.data_ptr(), E.stream()), "mlpk_channel_mlp"))
    refused(N, bad(C - 8, C, C + 8), go, gp)
    refused(N, bad(C, C - 8, C + 8), go, gp)
    refused(N, bad(C, C, C - 8), go, gp)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_smlp_mix_pitched(dtype):
    """mlpk_smlp_mix(_dw): ldx = C + 8, ldo = 3 C + 8, ldxr = C + 16"""
    E, N = pk()
    B_, H, W, C = 2, 9, 12, 64
    rows = B_ * H * W
    x = rd((rows, C), dtype, 1) * 1.5
    s, h = rd((C,), torch.float32, 2) * 0.3 + 1, rd((C,), torch.float32, 3) * 0.5
    dw = [rd((9, C), torch.float32, 4) * 0.3, rd((C,), torch.float32, 5) * 0.2, rd((C,), torch.float32, 6) * 0.3 + 1, rd((C,), torch.float32, 7) * 0.5]
    whp, bhp = E.pack_smlp_mix(rnd((H, H), torch.float32, 8, 1.0 / math.sqrt(H)), rnd((H,), torch.float32, 9), dtype, DEV)
    wwp, bwp = E.pack_smlp_mix(rnd((W, W), torch.float32, 10, 1.0 / math.sqrt(W)), rnd((W,), torch.float32, 11), dtype, DEV)
    assert E.smlp_mix_supported(dtype, H, W, C) and E.smlp_mix_dw_supported(dtype, H, W, C)

    def mix(ops):
        xv, o = ops.inp("x", x), ops.out("out", rows, 3 * C, dtype)
        E.smlp_mix(xv, xv.stride(0), B_, H, W, C, s, h, whp, bhp, wwp, bwp, o, o.stride(0))
    both(mix)

    def mix_dw(ops):
        xv, xr, o = ops.inp("x", x), ops.out("xres", rows, C, dtype, pad=16), ops.out("out", rows, 3 * C, dtype)
        E.smlp_mix_dw(xv, xv.stride(0), B_, H, W, C, *dw, xr, xr.stride(0), s, h, whp, bhp, wwp, bwp, o, o.stride(0))
    both(mix_dw)
    go, gx = Guarded(rows, 3 * C, 3 * C + 8, dtype, DEV), Guarded(rows, C, C + 8, dtype, DEV)
    refused(N, lambda: E.smlp_mix(x, C - 8, B_, H, W, C, s, h, whp, bhp, wwp, bwp, go.view, 3 * C + 8), go)
    refused(N, lambda: E.smlp_mix(x, C, B_, H, W, C, s, h, whp, bhp, wwp, bwp, go.view, 3 * C - 8), go)
    refused(N, lambda: E.smlp_mix_dw(x, C, B_, H, W, C, *dw, gx.view, C - 8, s, h, whp, bhp, wwp, bwp, go.view, 3 * C + 8), go, gx)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_vip_branch_and_split_apply_pitched(dtype):
    """mlpk_vip_branch (ldx, ldw, ldz, ld_sum padded) and mlpk_vip_split_apply on the permuted layout (ldh, ldw, ldc, ldo padded)"""
    E, N = pk()
    B_, H, W, C, seg = 2, 16, 32, 256, 8
    G, rows = C // seg, B_ * H * W
    x = rd((rows, C), dtype, 1) * 1.7 + 0.2
    mean, rstd = row_ln(x)
    gamma, beta = rd((C,), torch.float32, 2) * 0.3 + 1, rd((C,), torch.float32, 3) * 0.2
    assert E.vip_branch_supported(dtype, H, W, C, seg)
    for which, L, O in ((0, H, W), (1, W, H)):
        K = L * seg
        w, bias = rd((K, K), dtype, 4 + which, 1.0 / math.sqrt(K)), rd((K,), torch.float32, 6 + which) * 0.3

        def branch(ops):
            xv, wv = ops.inp("x", x), ops.inp("w", w, pad=16)
            z, sm = ops.out("z", B_ * O * G, K, dtype, pad=24), ops.out("sums", B_ * G, O * seg, torch.float32)
            E.vip_branch(which, xv, xv.stride(0), B_, H, W, C, seg, mean, rstd, gamma, beta, wv, bias, z, z.stride(0), sums=sm, ld_sum=sm.stride(0))
        both(branch)
        gz = Guarded(B_ * O * G, K, K + 8, dtype, DEV)
        refused(N, lambda: E.vip_branch(which, x, C - 8, B_, H, W, C, seg, mean, rstd, gamma, beta, w, bias, gz.view, K + 8), gz)
        refused(N, lambda: E.vip_branch(which, x, C, B_, H, W, C, seg, mean, rstd, gamma, beta, w, bias, gz.view, K - 8), gz)
    H2, W2, C2 = 5, 6, 32
    G2, rows2 = C2 // seg, B_ * H2 * W2
    zh, zw, xc = rd((B_ * W2 * G2, H2 * seg), dtype, 8), rd((B_ * H2 * G2, W2 * seg), dtype, 9), rd((rows2, C2), dtype, 10)
    bar = torch.softmax(rd((B_, 3, C2), torch.float32, 11), dim=1).contiguous()

    def apply(ops):
        a, b, c = ops.inp("zh", zh, pad=4), ops.inp("zw", zw, pad=12), ops.inp("xc", xc)
        o = ops.out("out", rows2, C2, dtype, pad=16)
        E.vip_split_apply(a, b, c, a.stride(0), b.stride(0), c.stride(0), B_, H2, W2, C2, seg, bar, o, o.stride(0))
    both(apply)
    go = Guarded(rows2, C2, C2 + 8, dtype, DEV)
    for lds in ((H2 * seg - 4, W2 * seg, C2, C2 + 8), (H2 * seg, W2 * seg - 4, C2, C2 + 8), (H2 * seg, W2 * seg, C2 - 8, C2 + 8), (H2 * seg, W2 * seg, C2, C2 - 8),
                (H2 * seg + 2, W2 * seg, C2, C2 + 8)):
        refused(N, lambda: E.vip_split_apply(zh, zw, xc, lds[0], lds[1], lds[2], B_, H2, W2, C2, seg, bar, go.view, lds[3]), go)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_embeddings_pitched(dtype):
    """mlpk_patch_embed4 (ldw, ldo padded) and mlpk_stem7 (ldo padded, statistics guarded); the NCHW image is dense by contract"""
    E, N = pk()
    B_, H, W, C = 3, 20, 12, 32
    img = rd((B_ * 3 * H, W), torch.float32, 1)
    wp = E.pack_matrix(rnd((C, 3, 4, 4), torch.float32, 2, 1.0 / math.sqrt(48)), dtype, DEV)
    bias, gamma, beta = rd((C,), torch.float32, 3) * 0.3, rd((C,), torch.float32, 4) * 0.3 + 1, rd((C,), torch.float32, 5) * 0.2
    assert E.patch_embed4_supported(torch.float32, dtype, 3, H, W, C)

    def embed(ops):
        E.patch_embed4(ops.inp("img", img, pad=0), ops.inp("w", wp), bias, ops.out("out", B_ * (H // 4) * (W // 4), C, dtype), B_, H, W, C, gamma=gamma, beta=beta)
    both(embed)
    go = Guarded(B_ * 15, C, C + 8, dtype, DEV)
    L = N.lib()
    refused(N, lambda: N.check(L.mlpk_patch_embed4(0, E.dtype_code(dtype), img.data_ptr(), B_, 3, H, W, wp.data_ptr(), 48, bias.data_ptr(), None, None, 1e-5,
                                                   go.view.data_ptr(), C - 8, C, E.stream()), "mlpk_patch_embed4"), go)
    refused(N, lambda: N.check(L.mlpk_patch_embed4(0, E.dtype_code(dtype), img.data_ptr(), B_, 3, H, W, wp.data_ptr(), 40, bias.data_ptr(), None, None, 1e-5,
                                                   go.view.data_ptr(), C + 8, C, E.stream()), "mlpk_patch_embed4"), go)
    H7, W7, pad = 21, 16, 2
    img7 = rd((B_ * 3 * H7, W7), torch.float32, 6)
    w7 = E.pack_stem7(rnd((C, 3, 7, 7), torch.float32, 7, 1.0 / math.sqrt(147)), dtype, DEV)
    Ho, Wo = (H7 + 2 * pad - 7) // 4 + 1, (W7 + 2 * pad - 7) // 4 + 1
    assert E.stem7_supported(torch.float32, dtype, 3, H7, W7, pad, C)

    def stem(ops):
        n = B_ * Ho * Wo
        E.stem7(ops.inp("img", img7, pad=0), w7, bias, ops.out("out", n, C, dtype, pad=24), B_, H7, W7, pad, C, out_stats=(ops.vec("mean", n), ops.vec("rstd", n)))
    both(stem)
    g7 = Guarded(B_ * Ho * Wo, C, C + 8, dtype, DEV)
    refused(N, lambda: N.check(L.mlpk_stem7(0, E.dtype_code(dtype), img7.data_ptr(), B_, 3, H7, W7, pad, w7.data_ptr(), bias.data_ptr(), g7.view.data_ptr(), C - 8, C,
                                            None, None, 1e-5, E.stream()), "mlpk_stem7"), g7)


# ------------------------------------------------------------------ dense by contract: lead, tail and the statistics buffers guarded
def one(case):
    """a dense-by-contract call: every operand at pad 0 inside its guard bands (a write past the last row or in front of the first shows)"""
    ops = Ops(True)
    post = case(ops)
    sync()
    ops.verify()
    if post is not None:
        post(ops)
    return ops


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_dense_remaps_guarded(dtype):
    """mlpk_shift_nchw(_backward), mlpk_shift_nhwc(_backward), mlpk_window_gather / scatter_add, mlpk_merge2x2_nhwc, mlpk_patch_rows_nhwc,
    mlpk_broadcast_rows, mlpk_index_gather"""
    E, N = pk()
    L, dc = N.lib(), E.dtype_code(dtype)
    n, c, h, w = 2, 20, 6, 5
    x = rd((n * c * h, w), dtype, 1)
    for dim in (2, 3):
        def nchw(ops):
            xv = ops.inp("x", x, pad=0)
            N.check(L.mlpk_shift_nchw(dc, xv.data_ptr(), ops.out("out", n * c * h, w, dtype, pad=0).data_ptr(), n, c, h, w, 5, dim, E.stream()), "shift_nchw")
            N.check(L.mlpk_shift_nchw_backward(dc, xv.data_ptr(), ops.out("gin", n * c * h, w, dtype, pad=0).data_ptr(), n, c, h, w, 5, dim, E.stream()), "shift_bwd")
        one(nchw)
        xl = rd((n * h * w, c), dtype, 2)

        def nhwc(ops):
            xv = ops.inp("x", xl, pad=0)
            E.shift_nhwc(xv, ops.out("out", n * h * w, c, dtype, pad=0), n, h, w, c, 5, dim)
            N.check(L.mlpk_shift_nhwc_backward(dc, xv.data_ptr(), ops.out("gin", n * h * w, c, dtype, pad=0).data_ptr(), n, h, w, c, 5, dim, E.stream()), "shift_bwd")
        one(nhwc)
    B_, H, W, C, ws = 2, 6, 5, 32, 4
    Hp, Wp = 8, 8
    xm = rd((B_ * H * W, C), dtype, 3)
    win = rd((B_ * Hp * Wp, C), dtype, 4)

    def windows(ops):
        E.window_gather(ops.inp("x", xm, pad=0), ops.out("win", B_ * Hp * Wp, C, dtype, pad=0), B_, H, W, C, ws, 1, 2, Hp, Wp)
        E.window_scatter_add(ops.inout("acc", xm, pad=0), ops.inp("w", win, pad=0), B_, H, W, C, ws, 1, 2, Hp, Wp)
    one(windows)
    He, We = 6, 4
    xe = rd((B_ * He * We, C), dtype, 5)

    def merges(ops):
        xv = ops.inp("x", xe, pad=0)
        m = ops.out("merged", B_ * 3 * 2, 4 * C, dtype, pad=0)
        N.check(L.mlpk_merge2x2_nhwc(dc, 0, xv.data_ptr(), m.data_ptr(), B_, He, We, C, E.stream()), "merge2x2")
        N.check(L.mlpk_merge2x2_nhwc(dc, 1, m.data_ptr(), ops.out("back", B_ * He * We, C, dtype, pad=0).data_ptr(), B_, He, We, C, E.stream()), "merge2x2")
        for order in (0, 1):
            pr = ops.out("rows%d" % order, B_ * 2 * 2, 6 * C, dtype, pad=0)
            N.check(L.mlpk_patch_rows_nhwc(dc, 0, order, xv.data_ptr(), pr.data_ptr(), B_, He, We, C, 3, 2, E.stream()), "patch_rows")
            N.check(L.mlpk_patch_rows_nhwc(dc, 1, order, pr.data_ptr(), ops.out("rback%d" % order, B_ * He * We, C, dtype, pad=0).data_ptr(), B_, He, We, C, 3, 2,
                                           E.stream()), "patch_rows")

        def post(ops):
            assert_bits_equal(ops.g("back").dense(), xe, "merge2x2 there and back")
            assert_bits_equal(ops.g("rback0").dense(), xe, "patch_rows there and back")
        return post
    one(merges)
    S = 7
    pooled = rd((B_, C), dtype, 6)

    def bcast(ops):
        N.check(L.mlpk_broadcast_rows(dc, ops.inp("in", pooled, pad=0).data_ptr(), ops.out("out", B_ * S, C, dtype, pad=0).data_ptr(), B_, S, C, 1.0 / S, E.stream()),
                "broadcast_rows")
    one(bcast)
    n_in, n_out, width, kmax = 9, 11, 24, 2
    src = rd((B_ * n_in, width), dtype, 7)
    idx = torch.tensor([[i % n_in, (-1 if i % 3 else (i + 4) % n_in)] for i in range(n_out)], dtype=torch.int32, device=DEV)

    def gather(ops):
        N.check(L.mlpk_index_gather(dc, ops.inp("src", src, pad=0).data_ptr(), ops.out("dst", B_ * n_out, width, dtype, pad=0).data_ptr(), idx.data_ptr(), B_, n_out,
                                    n_in, width, kmax, E.stream()), "index_gather")
    one(gather)


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_dense_convolutions_guarded(dtype):
    """mlpk_dwconv_nhwc, mlpk_dwconv_affine_nhwc, mlpk_dwconv_plain_nhwc (and its adjoint), mlpk_dwconv_wgrad_nhwc, mlpk_mixshift_nhwc(_stats)
    with row_part planes of pitch rows + 5, mlpk_norm_shift_nhwc, mlpk_merge2x2_stats_combine"""
    E, N = pk()
    L, dc = N.lib(), E.dtype_code(dtype)
    B_, H, W, C, k = 2, 6, 5, 64, 3
    rows = B_ * H * W
    x, dy = rd((rows, C), dtype, 1), rd((rows, C), dtype, 2)
    taps, bias = rd((k * k, C), torch.float32, 3) * 0.3, rd((C,), torch.float32, 4) * 0.2
    sc, sh = rd((C,), torch.float32, 5) * 0.2 + 1, rd((C,), torch.float32, 6) * 0.2

    def dw(ops):
        xv = ops.inp("x", x, pad=0)
        E.dwconv_nhwc(xv, ops.out("a", rows, C, dtype, pad=0), B_, H, W, C, k, taps, bias, sc, sh)
        E.dwconv_affine_nhwc(xv, ops.out("b", rows, C, dtype, pad=0), B_, H, W, C, k, taps, bias, sc, sh)
        for adj in (0, 1):
            N.check(L.mlpk_dwconv_plain_nhwc(dc, adj, xv.data_ptr(), ops.out("p%d" % adj, rows, C, dtype, pad=0).data_ptr(), B_, H, W, C, k, taps.data_ptr(),
                                             bias.data_ptr(), E.stream()), "dwconv_plain")
        N.check(L.mlpk_dwconv_wgrad_nhwc(dc, xv.data_ptr(), ops.inp("dy", dy, pad=0).data_ptr(), ops.out("dw", k * k, C, torch.float32, pad=0).data_ptr(), B_, H, W, C, k,
                                         E.stream()), "dwconv_wgrad")
    one(dw)
    shift, ksize = [-1, 0, 1, 2], [1, 3, 5, 7]
    kmax = 7
    wl, wt = rd((kmax * kmax, C), torch.float32, 7) * 0.2, rd((kmax * kmax, C), torch.float32, 8) * 0.2
    arr = ctypes.c_int * 4

    def mix(ops):
        xv = ops.inp("x", x, pad=0)
        E.mixshift_nhwc(xv, ops.out("out", rows, C, dtype, pad=0), B_, H, W, C, shift, ksize, wl, bias, wt, sh)
        nq = L.mlpk_mixshift_stats_planes(dc, B_, H, W, C, 4, arr(*ksize)) if dtype != torch.float32 else 0
        if nq > 0:
            part = ops.out("row_part", nq, 2 * rows, torch.float32, pad=10)
            N.check(L.mlpk_mixshift_nhwc_stats(dc, xv.data_ptr(), ops.out("out2", rows, C, dtype, pad=0).data_ptr(), B_, H, W, C, 4, arr(*shift), arr(*ksize),
                                               wl.data_ptr(), bias.data_ptr(), wt.data_ptr(), sh.data_ptr(), part.data_ptr(), part.stride(0) // 2, E.stream()),
                    "mlpk_mixshift_nhwc_stats")
            return lambda ops: assert_bits_equal(ops.g("out2").dense(), ops.g("out").dense(), "with and without statistics")
    ops = one(mix)
    if dtype != torch.float32:
        assert "row_part" in ops.items, "the statistics form must take this shape"
        go, gp = Guarded(rows, C, C, dtype, DEV), Guarded(2, 2 * rows, 2 * rows, torch.float32, DEV)
        refused(N, lambda: N.check(L.mlpk_mixshift_nhwc_stats(dc, x.data_ptr(), go.view.data_ptr(), B_, H, W, C, 4, arr(*shift), arr(*ksize), wl.data_ptr(), bias.data_ptr(),
                                                              wt.data_ptr(), sh.data_ptr(), gp.view.data_ptr(), rows - 1, E.stream()), "mixshift_stats"), go, gp)
        mean, rstd = rd((B_,), torch.float32, 9) * 0.1, rd((B_,), torch.float32, 10).abs() * 0.3 + 0.6

        def ns(ops):
            E.norm_shift_nhwc(ops.inp("x", x, pad=0), ops.out("w", rows, C, dtype, pad=0), ops.out("h", rows, C, dtype, pad=0), B_, H, W, C, 5, mean, rstd, sc, sh, 1)
        one(ns)
    He, We = 6, 4
    pm, pr = rd((B_ * He * We,), torch.float32, 11), rd((B_ * He * We,), torch.float32, 12).abs() + 0.5

    def combine(ops):
        n = B_ * 3 * 2
        E.merge2x2_stats_combine(ops.inp("mean", pm.view(1, -1), pad=0), ops.inp("rstd", pr.view(1, -1), pad=0), B_, He, We, ops.vec("om", n), ops.vec("or", n))
    one(combine)


# ------------------------------------------------------------------ the fused token-mixing MLP, AxialShift's core, the Swin-MLP spatial half
def token_mlp_operands(E, dtype, B_, C, S, T, seed, **pack_kw):
    sp = E.round_up(S, 32)
    xt = torch.zeros((B_ * C, sp), dtype=dtype, device=DEV)
    xt[:, :S] = rd((B_ * C, S), dtype, seed)
    pack = E.pack_token_mlp(rnd((T, S), torch.float32, seed + 1, 1.0 / math.sqrt(S)), rnd((T,), torch.float32, seed + 2),
                            rnd((S, T), torch.float32, seed + 3, 1.0 / math.sqrt(T)), rnd((S,), torch.float32, seed + 4), dtype, DEV, sp, **pack_kw)
    return sp, xt, pack, rd((B_ * S, C), dtype, seed + 5)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_token_mlp_pitched(dtype, layout):
    """mlpk_token_mlp layouts 0 and 1: x updated in place at ldx = C + 8, w2 at a padded ldw2 (NaN behind its zero padding), the statistics planes
    guarded; xt is dense by contract (its pitch is the K of the first product)"""
    E, N = pk()
    for B_, C, S, T in ((3, 40, 49, 196), (2, 128, 49, 100)):
        sp, xt, (w1p, b1p, w2p, b2p, nch, lay), x = token_mlp_operands(E, dtype, B_, C, S, T, 10 * C, layout=layout)
        assert lay == layout

        def case(ops):
            xv = ops.inout("x", x)
            st = ops.out("stats", C // 128, B_ * S * 2, torch.float32, pad=0) if C % 128 == 0 else None
            E.token_mlp(ops.inp("xt", xt, pad=0), sp, B_ * C, S, w1p, b1p, ops.inp("w2", w2p, pad=32), b2p, nch, xv, xv.stride(0), C, stats=st, layout=lay)
        both(case)
        gx = Guarded(B_ * S, C, C + 8, dtype, DEV)
        refused(N, lambda: E.token_mlp(xt, sp, B_ * C, S, w1p, b1p, w2p, b2p, nch, gx.view, C - 8, C, layout=lay), gx)         # ldx < t_rows


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_token_mlp_generated_and_ln_pitched(dtype):
    """mlpk_token_mlp layouts 2 / 3 and mlpk_token_mlp_ln at one image with t_rows = 256: ldx = C + 8, the 64-channel statistics planes guarded"""
    E, N = pk()
    B_, C, S, T = 1, 256, 196, 96
    sp, xt, (w1p, b1p, w2p, b2p, nch, lay), x = token_mlp_operands(E, dtype, B_, C, S, T, 7, t_rows=C)
    assert sp == 224 and lay == (3 if dtype == torch.bfloat16 else 2)
    planes = E.token_mlp_stat_planes(C, lay)
    x = x * 2 + 0.3
    mean, rstd = row_ln(x)
    gamma, beta = rd((C,), torch.float32, 20) + 1.1, rd((C,), torch.float32, 21)

    def fused(ops):
        xv = ops.inout("x", x)
        E.token_mlp(ops.inp("xt", xt, pad=0), sp, B_ * C, S, w1p, b1p, w2p, b2p, nch, xv, xv.stride(0), C,
                    stats=ops.out("stats", planes, B_ * S * 2, torch.float32, pad=0), layout=lay)
    both(fused)

    def fused_ln(ops):
        xv = ops.inout("x", x)
        E.token_mlp_ln(xv, xv.stride(0), B_ * C, S, mean, rstd, gamma, beta, w1p, b1p, w2p, b2p, nch, C,
                       stats=ops.out("stats", planes, B_ * S * 2, torch.float32, pad=0), layout=lay)
    both(fused_ln)
    gx = Guarded(B_ * S, C, C + 8, dtype, DEV)
    refused(N, lambda: E.token_mlp(xt, sp, B_ * C, S, w1p, b1p, w2p, b2p, nch, gx.view, C - 8, C, layout=lay), gx)
    refused(N, lambda: E.token_mlp_ln(gx.view, C - 8, B_ * C, S, mean, rstd, gamma, beta, w1p, b1p, w2p, b2p, nch, C, layout=lay), gx)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_as_conv2_pitched(dtype):
    """mlpk_as_conv2(_stats): the weights at ldw = C + 8; t and y dense by contract (lead and tail guarded); part, mean_out, rstd_out guarded, the
    counters left zero"""
    E, N = pk()
    B_, H, W, C = 2, 7, 9, 96
    rows = B_ * H * W
    t = rd((rows, C), dtype, 1) * 1.5 + 0.3
    mean, rstd = rd((B_,), torch.float32, 2) * 0.2, rd((B_,), torch.float32, 3).abs() * 0.3 + 0.6
    gamma, beta = rd((C,), torch.float32, 4) * 0.3 + 1, rd((C,), torch.float32, 5) * 0.2
    w1, w2 = rd((C, C), dtype, 6, 1.0 / math.sqrt(C)), rd((C, C), dtype, 7, 1.0 / math.sqrt(C))
    b1, b2 = rd((C,), torch.float32, 8), rd((C,), torch.float32, 9)
    assert E.as_conv2_supported(dtype, H, W, C, 5)
    L, dc = N.lib(), E.dtype_code(dtype)
    steps = L.mlpk_as_conv2_steps(dc, H, W, C, 5)
    counter = torch.zeros((B_,), dtype=torch.int32, device=DEV)

    def case(ops):
        tv, a, b = ops.inp("t", t, pad=0), ops.inp("w1", w1), ops.inp("w2", w2)
        E.as_conv2(tv, ops.out("y", rows, C, dtype, pad=0), B_, H, W, C, 5, mean, rstd, gamma, beta, a, b1, b, b2)
        N.check(L.mlpk_as_conv2_stats(dc, tv.data_ptr(), ops.out("y_stats", rows, C, dtype, pad=0).data_ptr(), B_, H, W, C, 5, mean.data_ptr(), rstd.data_ptr(),
                                      gamma.data_ptr(), beta.data_ptr(), a.data_ptr(), b1.data_ptr(), b.data_ptr(), b2.data_ptr(), a.stride(0),
                                      ops.vec("part", B_ * steps * 2).data_ptr(), ops.vec("mean_out", B_).data_ptr(), ops.vec("rstd_out", B_).data_ptr(),
                                      counter.data_ptr(), 1e-5, E.stream()), "mlpk_as_conv2_stats")

        def post(ops):
            assert_bits_equal(ops.g("y_stats").dense(), ops.g("y").dense(), "y with and without statistics")
            assert int(counter.abs().sum()) == 0, "the counters must be left zeroed"
        return post
    both(case)
    gy = Guarded(rows, C, C, dtype, DEV)
    refused(N, lambda: N.check(L.mlpk_as_conv2(dc, t.data_ptr(), gy.view.data_ptr(), B_, H, W, C, 5, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                               beta.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), C - 8, E.stream()), "mlpk_as_conv2"), gy)


@pytest.mark.parametrize("dtype", BITS16, ids=[IDS[d] for d in BITS16])
def test_swin_spatial_guarded(dtype):
    """mlpk_swin_spatial(_stats): dense by contract, x updated in place inside its guard bands, out_mean / out_rstd guarded; plain and shifted windows"""
    E, N = pk()
    for B_, H, W, heads, ws, shift in ((2, 14, 14, 3, 7, 3), (2, 12, 10, 2, 5, 0)):
        C, t, rows = heads * 32, ws * ws, B_ * H * W
        x = rd((rows, C), dtype, heads) * 1.3 + 0.2
        mean, rstd = row_ln(x)
        gamma, beta = rd((C,), torch.float32, 2) * 0.3 + 1, rd((C,), torch.float32, 3) * 0.2
        wp, bp = E.pack_swin_spatial(rnd((heads * t, t, 1), torch.float32, 4, 1.0 / math.sqrt(t)), rnd((heads * t,), torch.float32, 5, 0.3), heads, ws, dtype, DEV)
        pad_l = pad_t = (ws - shift) if shift else 0
        Hp, Wp = -(-(H + pad_t + shift) // ws) * ws, -(-(W + pad_l + shift) // ws) * ws
        assert E.swin_spatial_supported(dtype, C, heads, ws)

        def case(ops):
            E.swin_spatial(ops.inout("x", x, pad=0), B_, H, W, C, ws, pad_t, pad_l, Hp, Wp, heads, mean, rstd, gamma, beta, wp, bp)
            E.swin_spatial(ops.inout("x_stats", x, pad=0), B_, H, W, C, ws, pad_t, pad_l, Hp, Wp, heads, mean, rstd, gamma, beta, wp, bp,
                           out_stats=(ops.vec("out_mean", rows), ops.vec("out_rstd", rows)))
            return lambda ops: assert_bits_equal(ops.g("x_stats").dense(), ops.g("x").dense(), "x with and without statistics")
        one(case)


# ------------------------------------------------------------------ the *_pitch / *_off families: RaftMLP, ActiveMLP, DynaMixer, Sequencer2D
# Their headers demand 16-byte bases and pitches for the vector operands and say "the results do not depend on the pitches": (c) always holds.
def per16(dtype):
    """elements per 16 bytes"""
    return 4 if dtype == torch.float32 else 8


def aligned_leads(dtype):
    """the lead offsets (of guard.LEAD_OFFSETS) that keep a base on a 16-byte boundary: 4 elements only in fp32"""
    return (0, 4) if dtype == torch.float32 else (0,)


def restride(v, ld, shift=0):
    """the 2-d view v at another row pitch and `shift` elements further on (for the refusals: nothing is read or written through it)"""
    return torch.as_strided(v, tuple(v.shape), (ld, 1), v.storage_offset() + shift)


def wide(rows, cols, dtype, extra):
    """a (rows, cols) view of a zero buffer with `extra` spare columns behind every row"""
    return torch.zeros((rows, cols + extra), dtype=dtype, device=DEV)[:, :cols]


def ln_operands(x, C, seed):
    mean, rstd = row_ln(x)
    return mean, rstd, rd((C,), torch.float32, seed) * 0.3 + 1, rd((C,), torch.float32, seed + 1) * 0.2


@pytest.mark.parametrize("axis", [0, 1], ids=["vertical", "horizontal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_raft_pitched(dtype, axis):
    """mlpk_raft_gather_ln and mlpk_raft_scatter_add on a 5 x 3 map of 16 channels, r = 2, three images: x at C + e, a at kp + 2e (columns [D, kp)
    exactly +0, [kp, a_pitch) poison), y at the first aligned pitch beyond D + e with NaN behind column D, x updated in place inside its bands;
    every 16-byte lead the type has"""
    E, N = pk()
    B_, H, W, C, r = 3, 5, 3, 16, 2
    assert E.raft_supported(dtype, H, W, C, r, axis)
    e = per16(dtype)
    L, Q = (H, W) if axis == 0 else (W, H)
    Co, D, rows = C // r, r * L, B_ * H * W
    items, kp = B_ * Q * Co, E.round_up(D + 1, e)
    dy = E.round_up(D, e) - D                                  # what the dense twin of y needs for a 16-byte pitch
    x, y = rd((rows, C), dtype, 1 + axis) + 0.25, rd((items, D), dtype, 3 + axis)
    mean, rstd, gamma, beta = ln_operands(x, C, 5)
    for lead in aligned_leads(dtype):
        def case(ops):
            a = ops.out("a", items, kp, dtype, pad=2 * e, off=lead)
            E.raft_gather_ln(ops.inp("x", x, pad=e, off=lead), mean, rstd, gamma, beta, a, kp, B_, H, W, C, r, axis)
            E.raft_scatter_add(ops.inout("xs", x, pad=e, off=lead), ops.inp("y", y, pad=dy + e, off=lead, dpad=dy), B_, H, W, C, r, axis)

            def post(ops):
                pad0 = ops.g("a").view[:, D:kp].contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)
                assert kp > D and int((pad0 != 0).sum()) == 0, "columns [D, kp) of a are not +0"
                assert not torch.equal(ops.g("xs").dense(), x), "nothing was added"
            return post
        both(case)
    ga, gx = Guarded(items, kp, kp + e, dtype, DEV), Guarded(rows, C, C + e, dtype, DEV)
    xw, yw = wide(rows, C, dtype, e), wide(items, D, dtype, dy + e)
    gather = lambda xv, av, k=kp: (lambda: E.raft_gather_ln(xv, mean, rstd, gamma, beta, av, k, B_, H, W, C, r, axis))
    scatter = lambda xv, yv: (lambda: E.raft_scatter_add(xv, yv, B_, H, W, C, r, axis))
    refused(N, gather(restride(xw, C - e), ga.view), ga)                        # x_pitch < C
    refused(N, gather(restride(xw, C + e // 2), ga.view), ga)                   # x_pitch off the 16-byte grid
    refused(N, gather(restride(xw, C + e, e // 2), ga.view), ga)                # x 8 bytes off
    refused(N, gather(xw, ga.view, kp + 2 * e), ga)                             # kp beyond a_pitch
    refused(N, gather(xw, restride(ga.view, kp - e)), ga)                       # a_pitch < kp
    refused(N, gather(xw, restride(ga.view, kp + e, e // 2)), ga)               # a 8 bytes off
    refused(N, scatter(restride(gx.view, C - e), yw), gx)                       # x_pitch < C
    refused(N, scatter(restride(gx.view, C + e, e // 2), yw), gx)               # x 8 bytes off
    refused(N, scatter(gx.view, restride(yw, D // e * e if D % e else D - e)), gx)      # y_pitch < D
    refused(N, scatter(gx.view, restride(yw, D + dy + e // 2)), gx)             # y_pitch off the 16-byte grid
    refused(N, scatter(gx.view, restride(yw, D + dy + e, e // 2)), gx)          # y 8 bytes off


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_atm_sample_pitched(dtype):
    """mlpk_atm_sample on a 5 x 7 map of 16 channels, share 2, three images: the three outputs as column slices of one (rows, 3C) buffer at
    3C + e, then out_w and out_c alone with a gap between them that must stay poison; `off` needs element alignment only: an odd lead and an
    odd pitch, NaN behind its 2C / share columns"""
    E, N = pk()
    B_, H, W, C, share = 3, 5, 7, 16, 2
    assert E.atm_sample_supported(dtype, H, W, C, share)
    e, rows, oc = per16(dtype), B_ * H * W, 2 * C // share
    x = rd((rows, C), dtype, 1) + 0.25
    off = rd((rows, oc), dtype, 2, 1.5)                         # positions inside, between and beyond the pixels of a line
    mean, rstd, gamma, beta = ln_operands(x, C, 3)
    for lead in aligned_leads(dtype):
        def case(ops):
            o = ops.out("out", rows, 3 * C, dtype, pad=e, off=lead)
            E.atm_sample(ops.inp("x", x, pad=e, off=lead), mean, rstd, gamma, beta, ops.inp("off", off, pad=3, off=1), share,
                         o[:, :C], o[:, C:2 * C], o[:, 2 * C:], B_, H, W, C)
            g = ops.out("gap", rows, 2 * C + e, dtype, pad=2 * e, off=lead, finite=False)
            E.atm_sample(ops.inp("x2", x, pad=2 * e, off=lead), mean, rstd, gamma, beta, ops.inp("off2", off, pad=1, off=1), share,
                         g[:, :C], None, g[:, C + e:], B_, H, W, C)

            def post(ops):
                gg, oo = ops.g("gap"), ops.g("out").view
                gg.still_poison(C, C + e)
                assert_bits_equal(gg.view[:, :C].contiguous(), oo[:, :C].contiguous(), "out_w without out_h")
                assert_bits_equal(gg.view[:, C + e:].contiguous(), oo[:, 2 * C:].contiguous(), "out_c without out_h")
                assert not torch.equal(oo[:, :C], oo[:, 2 * C:]) and not torch.equal(oo[:, C:2 * C], oo[:, 2 * C:]), "the offsets moved nothing"
            return post
        both(case)
    go = Guarded(rows, 3 * C, 3 * C + e, dtype, DEV)
    xw, ow = wide(rows, C, dtype, e), wide(rows, oc, dtype, 3)
    ov = go.view
    call = lambda xv, fv, o3: (lambda: E.atm_sample(xv, mean, rstd, gamma, beta, fv, share, o3[0], o3[1], o3[2], B_, H, W, C))
    slices = lambda v: (v[:, :C], v[:, C:2 * C], v[:, 2 * C:])
    refused(N, call(restride(xw, C - e), ow, slices(ov)), go)                                   # x_pitch < C
    refused(N, call(restride(xw, C + e // 2), ow, slices(ov)), go)                              # x_pitch off the 16-byte grid
    refused(N, call(restride(xw, C + e, e // 2), ow, slices(ov)), go)                           # x 8 bytes off
    refused(N, call(xw, restride(ow, oc - 1), slices(ov)), go)                                  # off_pitch < 2C / share
    refused(N, call(xw, ow, (restride(ov[:, :C], C - e), None, None)), go)                      # out_pitch < C
    refused(N, call(xw, ow, (restride(ov[:, :C], 3 * C + e // 2), None, None)), go)             # out_pitch off the 16-byte grid
    refused(N, call(xw, ow, tuple(restride(v, 3 * C + e, e // 2) for v in slices(ov))), go)     # the outputs 8 bytes off
    refused(N, call(xw, ow, (ov[:, :C], restride(ov[:, C:2 * C], 3 * C + e, e // 2), ov[:, 2 * C:])), go)      # one of them


@pytest.mark.parametrize("form", ["fused", "unfused"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_dyna_mix_pitched(dtype, form):
    """mlpk_dyna_mix (fused) and mlpk_dyna_gather + mlpk_dyna_mix_logits (unfused) on a 5 x 3 map of 24 channels, s = 3, hd = 2, three images:
    both axes read ONE t (rows, 2 s hd) at t_off = 0 and s hd and write the two column blocks of ONE (rows, 2C) buffer.  t, v and z need element
    alignment only: odd leads and odd pitches."""
    E, N = pk()
    B_, H, W, C, s, hd = 3, 5, 3, 24, 3, 2
    e, rows, nt = per16(dtype), B_ * H * W, s * hd
    x = rd((rows, C), dtype, 1) + 0.25
    t = rd((rows, 2 * nt), dtype, 2, 2.0)
    mean, rstd, gamma, beta = ln_operands(x, C, 3)
    geo, aw, ab, z = {}, {}, {}, {}
    for axis in (0, 1):
        L, Q = (H, W) if axis == 0 else (W, H)
        assert E.dyna_mix_supported(dtype, L, C, s, hd)
        K, nn, items = L * hd, L * L, B_ * Q * s
        kp = E.round_up(K + 1, 8)
        geo[axis] = (L, K, nn, items, kp)
        A, b = rnd((nn, K), torch.float32, 10 + axis, 0.7), rnd((nn,), torch.float32, 12 + axis)
        if form == "fused":
            aw[axis], ab[axis] = E.pack_dyna_attend(A, b, dtype, torch.device(DEV))
        else:                                                   # the logits of the unfused form, once: torch's Linear on the gathered rows
            v = torch.empty((items, kp), dtype=dtype, device=DEV)
            E.dyna_gather(t, axis * nt, v, kp, B_, H, W, s, hd, axis)
            sync()
            z[axis] = torch.nn.functional.linear(v[:, :K].contiguous(), A.to(DEV).to(dtype), b.to(DEV).to(dtype))
            assert_finite(z[axis], "logits")
    for lead in aligned_leads(dtype):
        def case(ops):
            xv, tv = ops.inp("x", x, pad=e, off=lead), ops.inp("t", t, pad=3, off=1)
            o = ops.out("out", rows, 2 * C, dtype, pad=e, off=lead)
            for axis in (0, 1):
                L, K, nn, items, kp = geo[axis]
                ob = o[:, axis * C:(axis + 1) * C]
                if form == "fused":
                    E.dyna_mix(xv, mean, rstd, gamma, beta, tv, axis * nt, aw[axis], ab[axis], ob, B_, H, W, C, s, hd, axis)
                else:
                    E.dyna_gather(tv, axis * nt, ops.out("v%d" % axis, items, kp, dtype, pad=3, off=1), kp, B_, H, W, s, hd, axis)
                    E.dyna_mix_logits(xv, mean, rstd, gamma, beta, ops.inp("z%d" % axis, z[axis], pad=5, off=1), ob, B_, H, W, C, s, hd, axis)
                if axis == 0:
                    sync()
                    ops.g("out").still_poison(C, 2 * C)         # the other axis's block

            def post(ops):
                oo = ops.g("out").view
                assert not torch.equal(oo[:, :C], oo[:, C:]), "the two axes gave one result"
                for axis in (0, 1) if form == "unfused" else ():
                    L, K, nn, items, kp = geo[axis]
                    pad0 = ops.g("v%d" % axis).view[:, K:].contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)
                    assert kp > K and int((pad0 != 0).sum()) == 0, "columns [L hd, kp) of v are not +0"
            return post
        both(case)
    go = Guarded(rows, 2 * C, 2 * C + e, dtype, DEV)
    xw, tw = wide(rows, C, dtype, e), wide(rows, 2 * nt, dtype, 3)
    ob, axis = go.view[:, C:], 1
    L, K, nn, items, kp = geo[axis]
    if form == "fused":
        call = lambda xv, tv, ov, toff=nt: (lambda: E.dyna_mix(xv, mean, rstd, gamma, beta, tv, toff, aw[axis], ab[axis], ov, B_, H, W, C, s, hd, axis))
        refused(N, call(xw, restride(tw, 2 * nt - 1), ob), go)                  # t_pitch < t_off + s hd
        refused(N, call(xw, tw, ob, -1), go)                                    # t_off < 0
    else:
        gv, zw = Guarded(items, kp, kp + 3, dtype, DEV), wide(items, nn, dtype, 5)
        gather = lambda tv, vv, toff=nt, k=kp: (lambda: E.dyna_gather(tv, toff, vv, k, B_, H, W, s, hd, axis))
        refused(N, gather(restride(tw, 2 * nt - 1), gv.view), gv)               # t_pitch < t_off + s hd
        refused(N, gather(tw, gv.view, -1), gv)                                 # t_off < 0
        refused(N, gather(tw, restride(gv.view, kp - 1)), gv)                   # v_pitch < kp
        refused(N, gather(tw, gv.view, nt, K - 1), gv)                          # kp < L hd
        call = lambda xv, zv, ov: (lambda: E.dyna_mix_logits(xv, mean, rstd, gamma, beta, zv, ov, B_, H, W, C, s, hd, axis))
        refused(N, call(xw, restride(zw, nn - 1), ob), go)                      # z_pitch < L L
        tw = zw                                                                 # (the second operand of `call` in this form)
    refused(N, call(restride(xw, C - e), tw, ob), go)                           # x_pitch < C
    refused(N, call(restride(xw, C + e // 2), tw, ob), go)                      # x_pitch off the 16-byte grid
    refused(N, call(restride(xw, C + e, e // 2), tw, ob), go)                   # x 8 bytes off
    refused(N, call(xw, tw, restride(ob, C - e)), go)                           # out_pitch < C
    refused(N, call(xw, tw, restride(ob, 2 * C + e // 2)), go)                  # out_pitch off the 16-byte grid
    refused(N, call(xw, tw, restride(ob, 2 * C + e, e // 2)), go)               # out 8 bytes off


@pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
def test_lstm_scan_pitched(dtype):
    """mlpk_lstm_scan on a 5 x 3 map, hid 16, two and three images (6 / 10 and 9 / 15 sequences): both axes read ONE xp (rows, 16 hid) at
    xp_off = 0 and 8 hid and write the two halves of ONE block buffer (rows, 4 hid) through out_off = 0 and 2 hid.  Pitches of width + 4 (rows
    on 8-byte boundaries only in the 16-bit types) and + 12"""
    E, N = pk()
    H, W, hid = 5, 3, 16
    e = per16(dtype)
    pw = [E.pack_lstm_hh(rnd((4 * hid, hid), torch.float32, 3 + a, 0.5), rnd((4 * hid, hid), torch.float32, 5 + a, 0.5), dtype, torch.device(DEV)) for a in (0, 1)]
    for B_ in (2, 3):
        rows = B_ * H * W
        xp = rd((rows, 16 * hid), dtype, B_)
        for lead in aligned_leads(dtype):
            for pad in (4, 12):
                def case(ops):
                    xv = ops.inp("xp", xp, pad=pad, off=lead)
                    o = ops.out("out", rows, 4 * hid, dtype, pad=pad, off=lead)
                    E.lstm_scan(xv, 0, pw[0], o, 0, B_, H, W, hid, 0)
                    sync()
                    ops.g("out").still_poison(2 * hid, 4 * hid)                 # the other axis's half
                    E.lstm_scan(xv, 8 * hid, pw[1], o, 2 * hid, B_, H, W, hid, 1)

                    def post(ops):
                        oo = ops.g("out").view
                        assert not torch.equal(oo[:, :2 * hid], oo[:, 2 * hid:]), "the two axes gave one result"
                    return post
                both(case)
    go = Guarded(rows, 4 * hid, 4 * hid + 4, dtype, DEV)
    xw = wide(rows, 16 * hid, dtype, 8)
    call = lambda xv, xoff, ov, ooff: (lambda: E.lstm_scan(xv, xoff, pw[1], ov, ooff, B_, H, W, hid, 1))
    refused(N, call(restride(xw, 16 * hid - 4), 8 * hid, go.view, 2 * hid), go)                 # xp_pitch < xp_off + 8 hid
    refused(N, call(xw, 8 * hid + 12, go.view, 2 * hid), go)                                    # ... by the offset (xw's own pitch is 16 hid + 8)
    refused(N, call(xw, 8 * hid, restride(go.view, 4 * hid - 4), 2 * hid), go)                  # out_pitch < out_off + 2 hid
    refused(N, call(xw, 8 * hid, go.view, 2 * hid + 8), go)                                     # ... by the offset
    refused(N, call(xw, -4, go.view, 0), go)                                                    # a negative offset
    refused(N, call(restride(xw, 16 * hid + 8), 2, go.view, 0), go)                             # xp_off no multiple of 4
    refused(N, call(xw, 0, go.view, 2), go)                                                     # out_off no multiple of 4
    refused(N, call(restride(xw, 16 * hid + 2), 0, go.view, 0), go)                             # xp_pitch no multiple of 4
    refused(N, call(xw, 0, restride(go.view, 4 * hid + 2), 0), go)                              # out_pitch no multiple of 4
    refused(N, call(restride(xw, 16 * hid + 8, e // 2), 0, go.view, 0), go)                     # xp 8 bytes off
    refused(N, call(xw, 0, restride(go.view, 4 * hid + 4, e // 2), 0), go)                      # out 8 bytes off
    gb = Guarded(rows, 10 * hid, 10 * hid + 4, dtype, DEV)                                      # xp and out as column blocks of ONE buffer:
    refused(N, call(gb.view, 0, gb.view, 8 * hid), gb)                                          # the span read overlaps the span written
