"""The GEMM dispatch, pinned without a GPU: mlpk_gemm_kernel_name is host logic (validation, the tile choice, the persistent tile's
height plan), and without a device the library assumes 256 compute units -- the MI355X's count -- so the answers are the GPU's.

The (rc, name) column was recorded from the library as it was BEFORE the dispatch resolved each call once (one gemm_resolve behind
every entry point), not from the code under test.  For a call that mlpk_gemm_nt refuses the expected value is mlpk_gemm_nt's error
code: the name query used to answer a kernel name for some of those (an explicit algo 14 / 16 on a descriptor the tile does not
take); it now gives the launch's refusal."""
import ctypes

from conftest import load_pkg

P = 1 << 20                      # a 16-byte aligned address; nothing is dereferenced by the queries
HEADLINE_FC1 = dict(dt="bf16", M=50176, N=3072, K=768, act=1)
HEADLINE_FC2 = dict(dt="bf16", M=50176, N=768, K=3072, res=1)

# (label, descriptor spec, rc, name).  Spec keys: dt, M, N, K; act; res (residual mode); ln (folded LayerNorm); part (row_part);
# trans (t_rows: token-transposed output); algo; bits (desc.reserved); plan (mlpk_gemm_set_plan mode); pair (MLPK_P8_PAIR);
# bias=0 (no bias); a=… / dtype=… / ldc=… override single fields.
CASES = [
    ("headline fc1, mixed plan", dict(HEADLINE_FC1), 0, "q4_bf16_g_s12"),
    ("headline fc1, whole-tile plan", dict(HEADLINE_FC1, plan=1), 0, "q4_bf16_g_s12"),
    ("headline fc2, mixed plan", dict(HEADLINE_FC2), 0, "gemm_nt_p8_pair_kernel<EPI=1> rows 256+192"),
    ("headline fc2, whole-tile plan", dict(HEADLINE_FC2, plan=1), 0, "gemm_nt_p8_kernel<EPI=1> rows 256"),
    ("headline fc2, one launch per height", dict(HEADLINE_FC2, pair="0"), 0, "gemm_nt_p8_kernel<EPI=1> rows 256+192"),
    ("headline fc2 with statistics: on the persistent tile", dict(HEADLINE_FC2, part=1), 0, "gemm_nt_p8_pair_kernel<EPI=2> rows 256+192"),
    ("headline fc1 with statistics: off the persistent tile", dict(HEADLINE_FC1, part=1), 0, "gemm_nt_s3_kernel 128x256"),
    ("gMLP proj_out with statistics", dict(dt="bf16", M=50176, N=256, K=768, res=1, part=1), 0, "gemm_nt_p8_kernel<EPI=2> rows 256"),
    ("N % 256 != 0, enough tiles: generated tile", dict(dt="bf16", M=262144, N=384, K=384, res=1), 0, "q4_bf16_r_s6"),
    ("N % 256 != 0, too few tiles for it", dict(dt="bf16", M=12544, N=384, K=384, res=1), 0, "gemm_nt_s3_kernel 128x128"),
    ("N = 768 with short K: generated tile ahead of the persistent one", dict(dt="f16", M=50176, N=768, K=384), 0, "q4_f16_p_s6"),
    ("ragged K, fp32", dict(dt="f32", M=1000, N=96, K=100), 0, "gemm_nt_kernel 64x64"),
    ("fp32, whole half-slabs", dict(dt="f32", M=1024, N=384, K=384), 0, "gemm_nt_glds_kernel 64x64"),
    ("a few tiles", dict(dt="bf16", M=256, N=1000, K=512), 0, "gemm_nt_glds_kernel 64x64"),
    ("skinny kernel asked for", dict(dt="f32", M=256, N=384, K=384, act=1, algo=16), 0, "gemm_skinny_f32_kernel"),
    ("... and not asked for", dict(dt="f32", M=256, N=384, K=384, act=1), 0, "gemm_nt_glds_kernel 64x64"),
    ("token-transposed output", dict(dt="f16", M=768 * 4, N=196, K=384, res=1, trans=768), 0, "gemm_nt_glds_kernel 64x64"),
    ("residual + GELU: staged epilogue", dict(dt="bf16", M=50176, N=768, K=3072, act=1, res=1), 0, "gemm_nt_p8_kernel<EPI=0> rows 256"),
    ("folded LayerNorm + GELU", dict(dt="bf16", M=50176, N=1536, K=256, act=1, ln=1), 0, "gemm_nt_p8_kernel<EPI=1> rows 256"),
    ("rows that are no whole 256-row tiles", dict(dt="f16", M=12608, N=512, K=512, res=2), 0, "gemm_nt_s3_kernel 128x128"),
    ("plan bit 16: whole tiles and one short panel", dict(dt="bf16", M=448, N=256, K=128, res=1, algo=14, bits=16), 0, "gemm_nt_p8_pair_kernel<EPI=1> rows 256+192"),
    ("plan bit 64: staged epilogue", dict(dt="bf16", M=512, N=256, K=128, algo=14, bits=64), 0, "gemm_nt_p8_kernel<EPI=0> rows 256"),
    ("explicit register-staged tile", dict(dt="bf16", M=130, N=70, K=136, algo=3), 0, "gemm_nt_kernel 128x256"),
    ("explicit LDS-DMA tile", dict(dt="f16", M=130, N=72, K=160, algo=10), 0, "gemm_nt_glds_kernel 64x64"),
    ("explicit s3 tile with statistics", dict(dt="bf16", M=50176, N=256, K=768, res=1, part=1, algo=11), 0, "gemm_nt_s3_kernel 256x128"),
    ("explicit generated tile", dict(dt="bf16", M=512, N=384, K=256, act=1, algo=15), 0, "q4_bf16_g_f4"),
    # ---- refusals, one per class ----
    ("no descriptor", None, -4, ""),
    ("null operand", dict(dt="bf16", M=64, N=64, K=64, a=0), -4, ""),
    ("unknown dtype", dict(dt="bf16", M=64, N=64, K=64, dtype=7), -1, ""),
    ("K not in 16-byte chunks", dict(dt="bf16", M=16, N=16, K=12), -2, ""),
    ("misaligned A", dict(dt="bf16", M=64, N=64, K=64, a=P + 8), -3, ""),
    ("unknown activation", dict(dt="bf16", M=64, N=64, K=64, act=5), -5, ""),
    ("algo out of range", dict(dt="bf16", M=64, N=64, K=64, algo=17), -5, ""),
    ("LDS-DMA tile on ragged K", dict(dt="bf16", M=130, N=70, K=136, algo=6), -2, ""),
    ("statistics of an fp32 product", dict(dt="f32", M=1024, N=384, K=384, part=1), -5, ""),
    ("statistics from a 64-column tile", dict(dt="bf16", M=1024, N=128, K=64, part=1, algo=5), -5, ""),
    ("statistics on the persistent tile without a residual", dict(dt="bf16", M=512, N=256, K=128, part=1, algo=14), -5, ""),
    ("generated tile on fp32", dict(dt="f32", M=512, N=384, K=256, algo=15), -2, ""),
    ("persistent tile on N % 256 != 0", dict(dt="bf16", M=512, N=384, K=256, algo=14), -2, ""),      # (was named gemm_nt_p8_kernel<EPI=1> rows 64)
    ("persistent tile on C rows that are not 16-byte aligned", dict(dt="bf16", M=320, N=256, K=128, res=1, algo=14, ldc=260), -2, ""),      # (was named gemm_nt_p8_kernel<EPI=1> rows 64)
    ("persistent tile on fp32", dict(dt="f32", M=512, N=256, K=128, algo=14), -1, ""),      # (was named gemm_nt_p8_kernel<EPI=1> rows 64)
    ("persistent tile, staged epilogue on short rows", dict(dt="bf16", M=320, N=256, K=128, algo=14, bits=64), -2, ""),      # (was named gemm_nt_p8_kernel<EPI=0> rows 256+64)
    ("skinny kernel on a 16-bit product", dict(dt="bf16", M=256, N=384, K=384, algo=16), -2, ""),      # (was named gemm_skinny_f32_kernel)
]


def descriptor(N, spec):
    """(GemmDesc, plan mode, MLPK_P8_PAIR) of a table row"""
    if spec is None:
        return None, 0, "1"
    s = dict(spec)
    d = N.GemmDesc()
    d.dtype = s.pop("dtype", {"f32": N.F32, "f16": N.F16, "bf16": N.BF16}[s.pop("dt")])
    d.M, d.N, d.K = s.pop("M"), s.pop("N"), s.pop("K")
    d.lda = d.ldb = d.K
    d.A, d.B, d.C = s.pop("a", P), P, P
    d.bias = P if s.pop("bias", 1) else None
    d.rperiod = 1
    d.act = s.pop("act", 0)
    d.res_mode = s.pop("res", 0)
    t_rows = s.pop("trans", 0)
    d.ldc = d.ldr = t_rows or d.N
    if t_rows:
        d.out_mode, d.t_rows, d.t_tokens = N.OUT_TOKEN_T, t_rows, d.N
    d.ldc = s.pop("ldc", d.ldc)
    if d.res_mode:
        d.R = P
    if s.pop("ln", 0):
        d.ln_mean = d.ln_rstd = d.ln_csum = P
        d.ln_group = 1
    if s.pop("part", 0):
        d.row_part, d.row_part_ld = P, d.M
    d.algo, d.reserved = s.pop("algo", 0), s.pop("bits", 0)
    plan, pair = s.pop("plan", 0), s.pop("pair", "1")
    assert not s, s
    return d, plan, pair


def test_gemm_dispatch_table(monkeypatch):
    N = load_pkg()._native
    lib = N.lib()
    try:
        for label, spec, want_rc, want_name in CASES:
            d, plan, pair = descriptor(N, spec)
            ref = None if d is None else ctypes.byref(d)
            monkeypatch.setenv("MLPK_P8_PAIR", pair)
            assert lib.mlpk_gemm_set_plan(plan) == 0
            buf = ctypes.create_string_buffer(96)
            rc = lib.mlpk_gemm_kernel_name(ref, buf, 96)
            assert (rc, buf.value.decode() if rc == 0 else "") == (want_rc, want_name), label
            if want_rc:             # a refused call is refused by every entry point with the same code, before anything is launched
                assert lib.mlpk_gemm_nt(ref, None) == want_rc, label
                if spec is not None and "part" not in spec:
                    n = ctypes.c_int(-1)
                    assert lib.mlpk_gemm_row_parts(ref, ctypes.byref(n)) != 0, label
    finally:
        lib.mlpk_gemm_set_plan(0)


def test_gemm_dispatch_table_covers_what_it_claims():
    names = [c[3] for c in CASES if c[2] == 0]
    for family in ("gemm_nt_kernel ", "gemm_nt_glds_kernel ", "gemm_nt_s3_kernel ", "gemm_nt_p8_kernel<EPI=0>", "gemm_nt_p8_kernel<EPI=1>",
                   "gemm_nt_p8_pair_kernel<EPI=1>", "gemm_nt_p8_pair_kernel<EPI=2>", "q4_", "gemm_skinny_f32_kernel"):
        assert any(n.startswith(family) for n in names), family
    assert {c[2] for c in CASES} >= {0, -1, -2, -3, -4, -5}
