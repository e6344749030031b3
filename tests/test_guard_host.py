"""The guard-band instrument (tests/guard.py) tested on the CPU, and the coverage gate of tests/test_gpu_pitched.py.

Fake "kernels" -- plain torch functions on CPU `Guarded` buffers -- each break the pitched contract in one way; `check()` or the finite-output
assertion must catch every one, and pass a correct fake.  The gate parses include/mlpk.h: every entry point (and descriptor) with a pitch or stride
parameter is either in the PITCHED table that names its GPU test or in EXEMPT with a reason, so a future entry point with a pitch fails here until
it is covered."""
import ast
import os
import re

import pytest
import torch

from conftest import ROOT
from guard import LEAD_OFFSETS, MIN_BAND, POISON, Guarded, assert_bits_equal, assert_finite, lead_for
from test_gpu_pitched import PITCHED

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


# ------------------------------------------------------------------ fake kernels: out[r, :cols] = 2 * x[r, :cols] (+ a row sum)
def fake_ok(x, ldx, out, ldo, rows, cols):
    """x, out: flat buffers addressed from the operand's first element, as a kernel sees its pointers"""
    for r in range(rows):
        out[r * ldo:r * ldo + cols] = x[r * ldx:r * ldx + cols] * 2


def fake_pad_column(x, ldx, out, ldo, rows, cols):
    fake_ok(x, ldx, out, ldo, rows, cols)
    out[2 * ldo + cols] = 1.0                                   # one element past column `cols` of row 2


def fake_row_too_many(x, ldx, out, ldo, rows, cols):
    fake_ok(x, ldx, out, ldo, rows, cols)
    out[rows * ldo:rows * ldo + cols] = 1.0


def fake_tail(x, ldx, out, ldo, rows, cols):
    fake_ok(x, ldx, out, ldo, rows, cols)
    out[rows * ldo + 1500] = 1.0


def fake_zero_pad(x, ldx, out, ldo, rows, cols, flip=False):
    """a contract with zero-filled pad columns [cols, ldo)"""
    fake_ok(x, ldx, out, ldo, rows, cols)
    for r in range(rows):
        out[r * ldo + cols:(r + 1) * ldo] = 0.0
    if flip:
        out[1 * ldo + cols + 1] = -0.0


def fake_modifies_input(x, ldx, out, ldo, rows, cols):
    fake_ok(x, ldx, out, ldo, rows, cols)
    x[3 * ldx + 1] = x[3 * ldx + 1] + 1


def fake_sums_over_ld(x, ldx, out, ldo, rows, cols, width=None):
    """out[r, 0] = sum of row r -- over `width` elements (the bug: ldx where it should be cols)"""
    width = cols if width is None else width
    for r in range(rows):
        out[r * ldo] = x[r * ldx:r * ldx + width].float().sum()
        out[r * ldo + 1:r * ldo + cols] = 0.0


def operands(dtype, off=0, rows=6, cols=10, ldx=14, ldo=12):
    data = (torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) % 7 - 3).to(dtype)
    gx = Guarded(rows, cols, ldx, dtype, "cpu", lead=lead_for(ldx, off), role="in", data=data)
    go = Guarded(rows, cols, ldo, dtype, "cpu", lead=lead_for(ldo, off), role="out")
    return data, gx, go


def run(fake, gx, go, **kw):
    fake(gx.flat[gx.lead:], gx.ld, go.flat[go.lead:], go.ld, gx.rows, gx.cols, **kw)


@pytest.mark.parametrize("off", LEAD_OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_correct_fake_passes(dtype, off):
    data, gx, go = operands(dtype, off)
    assert gx.view.storage_offset() == gx.lead and gx.view.stride() == (gx.ld, 1) and gx.lead % 8 == off
    run(fake_ok, gx, go)
    gx.check()
    go.check()
    assert_finite(go.view)
    assert_bits_equal(go.dense(), data * 2)
    run(fake_zero_pad, gx, go)
    go.check(zero_cols=(go.cols, go.ld))
    with pytest.raises(AssertionError, match=r"row 0, column 10 \(cols 10, ld 12\)"):
        go.check()                                              # ... and zero is not poison: where padding is NOT written it must stay NaN


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_in_a_pad_column_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_pad_column, gx, go)
    with pytest.raises(AssertionError, match=r"guard band written: row 2, column 10 \(cols 10, ld 12\)"):
        go.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_too_many_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_row_too_many, gx, go)
    with pytest.raises(AssertionError, match=r"guard band written: tail element 0 "):
        go.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_write_into_the_tail_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_tail, gx, go)
    with pytest.raises(AssertionError, match=r"guard band written: tail element 1500 "):
        go.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_write_in_front_of_the_first_row_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_ok, gx, go)
    go.flat[go.lead - 1] = 0.0
    with pytest.raises(AssertionError, match=r"lead element %d \(of %d, 1 before the first row\)" % (go.lead - 1, go.lead)):
        go.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_pad_zero_flipped_to_minus_zero_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_zero_pad, gx, go, flip=True)
    assert float(go.flat[go.lead + go.ld + go.cols + 1]) == 0.0         # equal as a number: only the integer view sees it
    with pytest.raises(AssertionError, match=r"row 1, column 11 .* holds 0x80+, expected 0x0+ "):
        go.check(zero_cols=(go.cols, go.ld))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_modified_input_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_modifies_input, gx, go)
    go.check()
    with pytest.raises(AssertionError, match=r"input modified: row 3, column 1 "):
        gx.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_sum_over_the_pitch_is_caught(dtype):
    _, gx, go = operands(dtype)
    run(fake_sums_over_ld, gx, go)
    go.check()
    assert_finite(go.view)
    run(fake_sums_over_ld, gx, go, width=gx.ld)
    go.check()                                                  # it wrote where it may ...
    with pytest.raises(AssertionError, match=r"not finite at \[0, 0\] \(6 elements\)"):
        assert_finite(go.view)                                  # ... but folded the input's NaN padding into the sums


def test_unwritten_output_and_unowned_parts():
    _, gx, go = operands(torch.bfloat16)
    with pytest.raises(AssertionError, match="not finite"):
        assert_finite(go.view)                                  # the logical area starts as NaN: an element left unwritten shows
    go.all_poison()
    go.view[:, :4] = 1.0
    go.still_poison(4, 10)
    with pytest.raises(AssertionError, match=r"unowned part of the output written: row 0, column 3 "):
        go.still_poison(3, 10)
    with pytest.raises(AssertionError, match=r"a refused call wrote: row 0, column 0 "):
        go.all_poison()


def test_bands_are_a_pitch_row_and_2048_elements_at_least():
    for dtype in DTYPES:
        guard, logical = POISON[dtype]
        assert guard != logical
        g = Guarded(3, 5, 9, dtype, "cpu")
        assert g.lead >= MIN_BAND and g.tail >= MIN_BAND and g.flat.numel() == g.lead + 3 * 9 + g.tail
        assert bool(torch.isnan(g.flat.float()).all())
    g = Guarded(2, 3000, 3008, torch.float16, "cpu")
    assert g.lead >= 3008 and g.tail >= 3008
    with pytest.raises(AssertionError):
        Guarded(2, 3000, 3008, torch.float16, "cpu", lead=2048)
    with pytest.raises(AssertionError):
        Guarded(2, 8, 8, torch.float16, "cpu", tail=100)
    data = torch.ones((2, 8), dtype=torch.float16)
    g = Guarded(2, 8, 16, torch.float16, "cpu", role="in", data=data, zero_cols=(8, 12))      # zeros where a contract wants them, NaN only beyond
    body = g.flat[g.lead:g.lead + 32].view(2, 16).float()
    assert bool((body[:, 8:12] == 0).all()) and bool(torch.isnan(body[:, 12:]).all())


# ------------------------------------------------------------------ the coverage gate
# ld*, *_ld and the two strides; *_pitch; and *_off, a column offset, which relocates an operand inside its row exactly as a pitch does
# (not lds_bytes, and not the POINTER `off` of mlpk_atm_sample)
PITCH_NAME = re.compile(r"^(ld|ld[a-z0-9]{1,2}|ld_\w+|\w+_ld|src_px_stride|plane_stride|\w+_pitch|\w+_off)$")

# entry point (or "entry.parameter") -> why no guarded call covers it
EXEMPT = {
    "mlpk_token_mlp.ldw1": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_token_mlp_ln.ldw1": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_channel_mlp.ldw1": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_token_gemm.ldw": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_token_gemm_ln.ldw": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_token_gemm_ln_post.ldw": "weights are packed by the engine to a fixed 256 pitch; the kernel refuses others",
    "mlpk_token_mlp_ln.ldw2": "layouts 2 / 3 take the group-major w2 at a fixed pitch of 32; the kernel refuses others",
    "mlpk_token_mlp.ldxt": "the pitch of xt IS the K of the first product (a multiple of 32, columns >= S zero): dense by contract, lead and tail guarded",
    "mlpk_token_gemm.ldxt": "the pitch of xt IS the K of the product (a multiple of 32, columns >= S zero): dense by contract, lead and tail guarded",
}


def header_pitches():
    """include/mlpk.h -> {entry point or descriptor: set of its pitch / stride parameters or fields}"""
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {}
    for name, body in re.findall(r"typedef\s+struct\s+(mlpk_\w+)\s*\{(.*?)\}", text, flags=re.S):
        fields = {m for decl in body.split(";") for m in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1]) if PITCH_NAME.match(m)}
        if fields:
            found[name] = fields
    for name, args in re.findall(r"\b(mlpk_\w+)\s*\(([^()]*)\)\s*;", text):
        params = {a.strip().split()[-1].lstrip("*") for a in args.split(",") if a.strip() and a.strip() != "void"}
        pitches = {p for p in params if PITCH_NAME.match(p)}
        if pitches:
            found[name] = pitches
    return found


def test_the_header_parser_sees_the_pitches():
    found = header_pitches()
    assert found["mlpk_gemm_desc"] == {"lda", "ldb", "ldc", "ldr", "row_part_ld"}
    assert found["mlpk_norm_desc"] == {"ldx", "ld_rm", "ld_tt", "ld_p", "ld_sum"}
    assert found["mlpk_transpose_batched"] == {"ld_in", "ld_out", "ld_res"}
    assert found["mlpk_patchify"] == {"src_px_stride", "ldo"}
    assert found["mlpk_mixshift_nhwc_stats"] == {"row_part_ld"}
    assert found["mlpk_lstm_scan"] == {"xp_pitch", "xp_off", "out_pitch", "out_off"}
    assert found["mlpk_dyna_mix"] == {"x_pitch", "t_pitch", "t_off", "out_pitch"}
    assert found["mlpk_atm_sample"] == {"x_pitch", "off_pitch", "out_pitch"}                   # (`off` itself is a pointer)
    assert found["mlpk_raft_gather_ln"] == {"x_pitch", "a_pitch"}
    assert PITCH_NAME.match("v_pitch") and PITCH_NAME.match("out_off") and not PITCH_NAME.match("off") and not PITCH_NAME.match("lds_bytes")
    assert "mlpk_split_softmax" not in found and "mlpk_convert" not in found
    assert len(found) >= 52 and "mlpk_gemm_algo_info" not in found                             # (45 before the *_pitch / *_off entry points)


def test_every_pitched_entry_point_is_covered_or_exempt():
    found = header_pitches()
    missing = []
    for name, pitches in sorted(found.items()):
        if name in EXEMPT:
            continue
        covered = set(PITCHED[name][0]) if name in PITCHED else set()
        for p in sorted(pitches - covered):
            if "%s.%s" % (name, p) not in EXEMPT:
                missing.append("%s.%s" % (name, p))
    assert not missing, "pitch parameters of include/mlpk.h with neither a guarded GPU test (PITCHED) nor an EXEMPT reason: %s" % missing
    stale = [k for k in list(PITCHED) + [e.split(".")[0] for e in EXEMPT] if k not in found]
    assert not stale, "listed but not in the header: %s" % stale
    for name, (params, test) in PITCHED.items():
        assert set(params) <= found[name], (name, params)
        assert test and all(len(r) > 10 for r in EXEMPT.values())


def test_the_table_names_tests_that_exist():
    """a bare name is a function of tests/test_gpu_pitched.py; tests/<file>.py::<name> is looked up in that file's syntax tree (the GPU files
    build models at import: they are parsed, not imported)"""
    import test_gpu_pitched
    for name, (_, tests) in PITCHED.items():
        for t in tests.split(", "):
            if not t.startswith("tests/"):
                assert callable(getattr(test_gpu_pitched, t, None)), (name, t)
                continue
            m = re.match(r"^tests/(\w+\.py)::(\w+)\b", t)
            assert m, (name, t)
            path = os.path.join(ROOT, "tests", m.group(1))
            assert os.path.isfile(path), (name, t)
            with open(path) as f:
                tree = ast.parse(f.read(), path)
            assert any(isinstance(n, ast.FunctionDef) and n.name == m.group(2) for n in tree.body), (name, t)
