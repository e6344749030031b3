"""-m gpu: Sequencer2D on the MI355X.
  * mlpk_lstm_scan alone, behind guard bands (tests/guard.py), both axes, three dtypes, dense operands and operands pitched with nonzero column
    offsets.  SHAPES (B, H, W, hid) cover L = 1, short and odd lines, fewer sequences than a tile, a tail tile, every required hid, the
    model's two line lengths (32 and 16) and, for every hid, a tail workgroup behind a full one whose second 16-sequence tile is partly live.
      value -- against a restatement: fp64 torch.nn.LSTM on the CPU on the STORED operands (the projections enter through an identity weight_ih).
      The gate is measured against torch itself: d(dtype) = the distance of the CPU nn.LSTM run in that type from the fp64 one on the same case;
      gate = 4 d in fp32 (another summation order over K <= 96 and the hardware's exp against libm swing a handful of ulps), 2 d in the 16-bit
      types (the project's convention).  Every gate must be at most a fifth of the distance to the same restatement without the recurrence
      (weight_hh = 0).  The measured table is in profiles/sequencer_kernel_errors.txt;
      structure, as equalities -- (a) weight_hh = 0 and the forget gate at -200: the scan equals the same kernel on B H W sequences of length 1;
      (b) the map flipped along the axis with the directions' weights and xp blocks swapped gives the flipped output with the blocks swapped;
      (c) the axis-0 scan equals the axis-1 scan of the transposed map; (d) a NaN in one sequence changes no bit of another; (e) pre-activations
      of +-1e4 stay finite and inside the value gate; (f) two runs agree; (g) every sequence of a map of identical lines has sequence 0's bits.
      the recurrence, bit for bit -- W_hh one-hot (+-1 at column pi(j) of row j of one gate) and the forget gate at -200: the scan equals one more
      launch of single steps whose fed gate is built from the scan's own output (tests/lstm_model.py; tests/test_sequencer_host.py holds the
      checks against planted faults).  The forget gate, which no single step replays, takes the same rows against fp64 nn.LSTM under the value
      rule, the gate at most a fifth of the distance to the identity permutation;
      size -- a 1100 x 1024 map whose rows end past element 2^31 of both buffers equals the kernel on a dense copy of its last sequences.
  * the family against tests/golden/sequencer.npz (the reference's own forwards, tests/golden/make_sequencer_golden.py): fp32 at
    1e-5 max(1, max|ref|), the 16-bit types at twice the reference's own distance in that type on the same case.
  * the lifecycle properties on a Config registered in test_lifecycle_host._CACHE."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
from guard import Guarded, assert_bits_equal, assert_finite
import lstm_model as LM
from lstm_model import from_seqs, random_operands as operands, restate, to_seqs
from oracle.portable_init import portable_input, portable_state_dict, portable_tensor
import test_lifecycle_host as LH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(GOLDEN, "sequencer.npz")
SQ = load_pkg().models_pytorch.sequencer
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["fp32", "fp16", "bf16"]
HIDS = [16, 32, 48, 96]
# (1, 51, 3): along axis 1, 51 sequences of length 3 -- a full workgroup and a tail whose second 16-sequence tile is partly live in the 16-bit
# types (three full workgroups and three sequences in fp32); along axis 0, three sequences of length 51
MASK_MAP = (1, 51, 3)
SHAPES = [(2, 5, 3, 16), (1, 1, 7, 16), (3, 4, 37, 32), (2, 32, 6, 48), (2, 16, 5, 96)] + [MASK_MAP + (hid,) for hid in HIDS]
NAME = "sequencer2d"


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def engine():
    return load_pkg().engine


# ------------------------------------------------------------------ the kernel alone
CASES = pytest.mark.parametrize("B,H,W,hid,dtype", [pytest.param(B, H, W, hid, dtype, id="%dx%dx%d-hid%d-%s" % (B, H, W, hid, name))
                                                    for B, H, W, hid in SHAPES for dtype, name in zip(DTYPES, IDS)])
AXES = pytest.mark.parametrize("axis", [0, 1], ids=["v", "h"])
PADS = pytest.mark.parametrize("pad", [0, 1], ids=["dense", "pitched"])


def run_scan(xp, whh, B, H, W, hid, dtype, axis, pad=0):
    """the kernel on xp (rows, 8 hid) and whh (2, 4 hid, hid), CPU fp32 tensors holding storage-type values -> (rows, 2 hid) in `dtype` on the CPU.
    pad: xp sits at column offset 8 of a wider buffer whose other columns are NaN, at a pitch beyond its width; the output is columns
    [4, 4 + 2 hid) of a wider buffer.  The guard bands and every column outside the written block must stay untouched."""
    E = engine()
    rows = B * H * W
    xoff, ooff, extra = (8, 4, 12) if pad else (0, 0, 0)
    full = torch.full((rows, xoff + 8 * hid + (4 if pad else 0)), float("nan"))
    full[:, xoff:xoff + 8 * hid] = xp
    gx = Guarded(rows, full.shape[1], full.shape[1] + extra, dtype, DEV, role="in", data=full)
    ocols = ooff + 2 * hid + (8 if pad else 0)
    go = Guarded(rows, ocols, ocols + extra, dtype, DEV, role="out")
    pw = E.pack_lstm_hh(whh[0], whh[1], dtype, torch.device(DEV))
    E.lstm_scan(gx.view, xoff, pw, go.view, ooff, B, H, W, hid, axis)
    torch.cuda.synchronize()
    gx.check()
    go.check()
    go.still_poison(0, ooff)
    go.still_poison(ooff + 2 * hid, ocols)
    return go.view[:, ooff:ooff + 2 * hid].clone().contiguous().cpu()


def value_case(what, xp, whh, B, H, W, hid, dtype, axis, pad):
    out = run_scan(xp, whh, B, H, W, hid, dtype, axis, pad)
    assert_finite(out, "out")
    exact = restate(xp, whh, B, H, W, hid, axis, torch.float64)
    d = float((restate(xp, whh, B, H, W, hid, axis, dtype) - exact).abs().max())
    far = float((restate(xp, torch.zeros_like(whh), B, H, W, hid, axis, torch.float64) - exact).abs().max())
    gate = (4.0 if dtype == torch.float32 else 2.0) * d
    err = float((out.double() - exact).abs().max())
    print("%s %dx%dx%d hid%d axis %d %s %s: |d| %.3e gate %.3e ratio %.3f (torch in type d %.3e, without the recurrence %.3e away, max|h| %.3f)" % (
        what, B, H, W, hid, axis, IDS[DTYPES.index(dtype)], "pitched" if pad else "dense", err, gate, err / gate if gate else 0.0, d, far,
        float(exact.abs().max())))
    return out, err, gate, far


@CASES
@AXES
def test_random_operands_against_fp64_lstm(B, H, W, hid, dtype, axis):
    seed = B * 1000 + H * 100 + W * 10 + hid + axis
    xp, whh = operands(B, H, W, hid, dtype, seed)
    dense, err, gate, far = value_case("numeric", xp, whh, B, H, W, hid, dtype, axis, 0)
    pitched = run_scan(xp, whh, B, H, W, hid, dtype, axis, 1)
    assert_bits_equal(pitched, dense, "the pitched call")
    if (H, W)[axis] > 1:                                               # (a line of one step has no recurrence)
        assert gate <= 0.2 * far, "the gate %.3e could not tell a kernel that drops the recurrence (%.3e away)" % (gate, far)
    assert err <= gate, (err, gate)


@CASES
@AXES
@PADS
def test_a_scan_without_recurrence_equals_single_steps(B, H, W, hid, dtype, axis, pad):
    """(a) weight_hh = 0 and the forget gate at -200 (its sigmoid is exactly 0): every step stands alone, so the scan of the map must be the same
    kernel on B H W sequences of length 1, bit for bit -- the addressing of both axes and both directions"""
    seed = B * 1000 + H * 100 + W * 10 + hid + axis + 40
    xp, whh = operands(B, H, W, hid, dtype, seed)
    for d in range(2):
        xp[:, (4 * d + 1) * hid:(4 * d + 2) * hid] = -200.0
    zero = torch.zeros_like(whh)
    got = run_scan(xp, zero, B, H, W, hid, dtype, axis, pad)
    want = run_scan(xp, zero, B * H * W, 1, 1, hid, dtype, axis, pad)
    assert_finite(want, "the single steps")
    assert_bits_equal(got, want, "the scan of the map")


def flip_map(v, B, H, W, axis):
    return v.reshape(B, H, W, -1).flip(1 + axis).reshape(B * H * W, -1).contiguous()


def swap_halves(v):
    n = v.shape[1] // 2
    return torch.cat([v[:, n:], v[:, :n]], 1).contiguous()


@CASES
@AXES
def test_reversal_swaps_the_directions(B, H, W, hid, dtype, axis):
    """(b)"""
    seed = B * 1000 + H * 100 + W * 10 + hid + axis + 80
    xp, whh = operands(B, H, W, hid, dtype, seed)
    base = run_scan(xp, whh, B, H, W, hid, dtype, axis, 1)
    other = run_scan(swap_halves(flip_map(xp, B, H, W, axis)), whh.flip(0).contiguous(), B, H, W, hid, dtype, axis, 1)
    assert_bits_equal(other, swap_halves(flip_map(base, B, H, W, axis)), "the flipped map with the directions swapped")


@CASES
def test_axis_0_is_axis_1_of_the_transposed_map(B, H, W, hid, dtype):
    """(c)"""
    seed = B * 1000 + H * 100 + W * 10 + hid + 120
    xp, whh = operands(B, H, W, hid, dtype, seed)
    tr = lambda v, h, w: v.reshape(B, h, w, -1).transpose(1, 2).reshape(B * h * w, -1).contiguous()
    v = run_scan(xp, whh, B, H, W, hid, dtype, 0, 0)
    h = run_scan(tr(xp, H, W), whh, B, W, H, hid, dtype, 1, 0)
    assert_bits_equal(tr(h, W, H), v, "the axis-1 scan of the transposed map")


@CASES
@AXES
def test_a_nan_sequence_changes_no_other_sequence(B, H, W, hid, dtype, axis):
    """(d) one NaN in the xp of one sequence (a middle one and the last one, which shares its tile with the padding lanes)"""
    seed = B * 1000 + H * 100 + W * 10 + hid + axis + 160
    xp, whh = operands(B, H, W, hid, dtype, seed)
    clean = to_seqs(run_scan(xp, whh, B, H, W, hid, dtype, axis, 0), B, H, W, axis)
    nseq, L = clean.shape[0], clean.shape[1]
    for s in sorted({nseq // 2, nseq - 1}):
        sx = to_seqs(xp, B, H, W, axis).clone()
        sx[s, L // 2, hid // 2] = float("nan")
        dirty = to_seqs(run_scan(from_seqs(sx, B, H, W, axis).contiguous(), whh, B, H, W, hid, dtype, axis, 0), B, H, W, axis)
        assert bool(torch.isnan(dirty[s].float()).any()), "the NaN did not reach its own sequence: the case checks nothing"
        keep = [i for i in range(nseq) if i != s]
        if keep:
            assert_bits_equal(dirty[keep].contiguous(), clean[keep].contiguous(), "the other sequences")


@CASES
@AXES
def test_saturated_gates_stay_finite(B, H, W, hid, dtype, axis):
    """(e) half of the pre-activations at +-1e4 (finite in fp16): exp overflows and must end in 0 / 1 / +-1"""
    seed = B * 1000 + H * 100 + W * 10 + hid + axis + 200
    xp, whh = operands(B, H, W, hid, dtype, seed)
    g = torch.Generator().manual_seed(seed + 1)
    big = torch.rand(xp.shape, generator=g) < 0.5
    sign = torch.where(torch.rand(xp.shape, generator=g) < 0.5, -1.0, 1.0)
    xp = torch.where(big, sign * 1e4, xp).to(dtype).float()
    out, err, gate, far = value_case("saturation", xp, whh, B, H, W, hid, dtype, axis, 1)
    assert err <= gate, (err, gate)


@CASES
@AXES
def test_two_runs_agree(B, H, W, hid, dtype, axis):
    """(f)"""
    xp, whh = operands(B, H, W, hid, dtype, B * 1000 + H * 100 + W * 10 + hid + axis + 240)
    assert_bits_equal(run_scan(xp, whh, B, H, W, hid, dtype, axis, 1), run_scan(xp, whh, B, H, W, hid, dtype, axis, 1), "the second run")


# ------------------------------------------------------------------ the recurrence itself (tests/lstm_model.py)
def gpu_scan(xp, whh, B, H, W, hid, dtype, axis):
    return run_scan(xp, whh, B, H, W, hid, dtype, axis, 1)


ON_MASK_MAP = pytest.mark.parametrize("hid,dtype", [pytest.param(hid, dtype, id="hid%d-%s" % (hid, name)) for hid in HIDS for dtype, name in zip(DTYPES, IDS)])


@ON_MASK_MAP
@AXES
@pytest.mark.parametrize("gate", ["i", "g", "o"])
def test_one_hot_recurrence_replays_bit_for_bit(hid, dtype, axis, gate):
    """W_hh[d] zero but for +-1 at column pi_d(j) of row j of `gate`, f at -200: z of the fed gate is +-h_{t-1}[pi(j)] exactly, so the scan
    must equal one launch of B H W single steps fed with the scan's own output at the previous pixel.  A k slot exchanged, a wave on another
    wave's rows, the other direction's weights or a stale h buffer move bits here; no tolerance."""
    for kind in LM.KINDS:
        fed = LM.replay_check(gpu_scan, *MASK_MAP, hid, dtype, axis, gate, kind)
        assert fed > 0, "no recurrent term was fed: the case checks nothing"


@ON_MASK_MAP
@AXES
def test_one_hot_forget_gate_against_fp64_lstm(hid, dtype, axis):
    """the same one-hot rows in the forget gate, f's xp random: c_{-1} = 0 keeps a single step from replaying it, so the fp64 restatement under
    the value rule (4 d in fp32, 2 d in the 16-bit types), the gate at most a fifth of the distance to pi = identity (both CPU figures, held
    in tests/test_sequencer_host.py as well)"""
    for kind in LM.KINDS:
        LM.forget_check(gpu_scan, *MASK_MAP, hid, dtype, axis, kind)


@ON_MASK_MAP
@AXES
def test_identical_sequences_give_identical_bits(hid, dtype, axis):
    """(g) the header's sentence that the results do not depend on where in the map (in which workgroup and lane) a sequence lies"""
    LM.identical_check(gpu_scan, *MASK_MAP, hid, dtype, axis)


@AXES
def test_element_indices_past_2_31(axis):
    """a 1100 x 1024 map at a row pitch of 2052 elements: the last rows of xp and of out lie past element 2^31 of their buffers (4.6 GB each in
    bf16), and a line is 1100 or 1024 steps long.  The part of the map whose sequences end there -- the last 8 columns (axis 0) or the last 8
    rows (axis 1) -- must equal, bit for bit, the same kernel on a dense copy of that part alone."""
    E = engine()
    H, W, hid, pitch, xoff, ooff, dtype = 1100, 1024, 16, 2052, 1024, 2000, torch.bfloat16
    rows = H * W
    assert (rows - 1) * pitch > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5 + axis)
    xbuf = torch.empty(rows * pitch, dtype=dtype, device=DEV)
    obuf = torch.empty(rows * pitch, dtype=dtype, device=DEV)
    xv, ov = xbuf.as_strided((rows, pitch), (pitch, 1)), obuf.as_strided((rows, pitch), (pitch, 1))
    xv[:, xoff:xoff + 8 * hid] = torch.randn((rows, 8 * hid), device=DEV, generator=g).to(dtype)
    whh = ((torch.rand((2, 4 * hid, hid), generator=torch.Generator().manual_seed(6)) * 2 - 1) * 0.5).to(dtype).float()
    pw = E.pack_lstm_hh(whh[0], whh[1], dtype, torch.device(DEV))
    E.lstm_scan(xv, xoff, pw, ov, ooff, 1, H, W, hid, axis)
    part = (slice(None), slice(W - 8, W)) if axis == 0 else (slice(H - 8, H), slice(None))
    small = xv[:, xoff:xoff + 8 * hid].reshape(H, W, 8 * hid)[part].contiguous()
    h2, w2 = small.shape[:2]
    want = torch.empty((h2 * w2, 2 * hid), dtype=dtype, device=DEV)
    E.lstm_scan(small.reshape(h2 * w2, 8 * hid), 0, pw, want, 0, 1, h2, w2, hid, axis)
    torch.cuda.synchronize()
    got = ov[:, ooff:ooff + 2 * hid].reshape(H, W, 2 * hid)[part].contiguous().reshape(h2 * w2, 2 * hid)
    assert_finite(want.cpu(), "the dense part")
    assert_bits_equal(got.cpu(), want.cpu(), "the part of the map past element 2^31")


# ------------------------------------------------------------------ the family against the reference
def widen(model, meta, scale=None):
    """tests/golden/make_sequencer_golden.py `widen`: every weight_hh times meta["hh_scale"]"""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if meta["widen"] in name:
                p.mul_(meta["hh_scale"] if scale is None else scale)


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
    """the tiny entry goes into the module-level table exactly as the fixture generator puts it into the reference's"""
    SQ.sequencer_settings.update({k: v for k, v in meta["tiny"].items()})


def tiny_model(meta, size):
    add_tiny_settings(meta)
    model = load_portable(SQ.Sequencer2D("tiny", num_classes=meta["tiny_classes"]), meta["tiny_seed"])
    widen(model, meta)
    x = torch.from_numpy(portable_input((2, 3, size[0], size[1]), seed=meta["tiny_seed"])).to(DEV)
    return model.to(DEV).eval(), x


def block_model(meta, name):
    cls, args, shape = meta["blocks"][name]
    seed = meta["block_seed"]
    blk = load_portable(getattr(SQ, cls)(*args), seed)
    widen(blk, meta)
    wide_affine(blk, meta, seed)
    return blk.to(DEV).eval(), torch.from_numpy(portable_input(tuple(shape), seed=seed)).to(DEV)


TAGS = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def check(out, ref, dtype, z, meta, case):
    """fp32: 1e-5 max(1, max|ref|); 16-bit: twice the reference's own distance in that type on the same case"""
    m = float(np.abs(ref).max())
    if dtype == torch.float32:
        gate = 1e-5 * max(1.0, m)
    else:
        key = "%s/%s" % (case, TAGS[dtype])
        if key in meta["lowp_skipped"]:
            pytest.skip("the reference's own %s forward of %s: %s" % (TAGS[dtype], case, meta["lowp_skipped"][key]))
        gate = 2.0 * float(z["%s/err_%s" % (case, TAGS[dtype])])
    assert tuple(out.shape) == ref.shape, (tuple(out.shape), ref.shape)
    assert_finite(out, case)
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    print("%s %s: max|d| %.3e gate %.3e ratio %.3f max|ref| %.3f" % (case, dtype, err, gate, err / gate, m))
    assert err <= gate, (case, str(dtype), err, gate, m)


TINY_SIZES = [(56, 56), (70, 42)]
BLOCK_NAMES = ["bilstm_32_16", "bilstm_192_48", "block_64_1_32"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size", TINY_SIZES, ids=["56x56", "70x42"])
def test_tiny_logits(size, dtype, z, meta):
    assert [list(s) for s in TINY_SIZES] == meta["tiny_sizes"]
    model, x = tiny_model(meta, size)
    with torch.no_grad():
        out = model(x.to(dtype))
    assert out.dtype == dtype
    check(out, z["tiny/%dx%d/logits" % size], dtype, z, meta, "tiny/%dx%d" % size)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_blocks_alone(name, dtype, z, meta):
    assert sorted(BLOCK_NAMES) == sorted(meta["blocks"])
    blk, x = block_model(meta, name)
    with torch.no_grad():
        out = blk(x.to(dtype))
    assert out.dtype == dtype
    check(out, z["block/%s/out" % name], dtype, z, meta, "block/" + name)


def test_tiny_compute_dtype(z, meta):
    """set_compute_dtype: fp32 input, bf16 kernels, fp32 logits"""
    model, x = tiny_model(meta, (56, 56))
    model.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        out = model(x)
    assert out.dtype == torch.float32
    check(out, z["tiny/56x56/logits"], torch.bfloat16, z, meta, "tiny/56x56")


@pytest.fixture(scope="module")
def real_model(z):
    """a state_dict in the reference's layout (keys and shapes of the fixture's table), loaded with strict=True"""
    shapes = {k: tuple(v) for k, v in json.loads(str(z["shapes/S"])).items()}
    sd = {k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}
    model = SQ.Sequencer2D("S")
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_logits(real_model, dtype, z, meta):
    x = torch.from_numpy(portable_input((2, 3, 224, 224), seed=0)).to(DEV)
    with torch.no_grad():
        out = real_model(x.to(dtype))
    check(out, z["real/S/logits"], dtype, z, meta, "real/S")


def test_wrong_input_size_raises(meta):
    model, _ = tiny_model(meta, (56, 56))
    for shape in ((1, 3, 56, 57), (1, 3, 60, 56), (1, 3, 7, 56), (1, 4, 56, 56)):
        with pytest.raises(ValueError, match=r"\(%s\)" % ", ".join(str(s) for s in shape)):
            model(torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        model(torch.zeros(3, 56, 56, device=DEV))
    blk = model.stages[0][1]
    with pytest.raises(ValueError):
        blk(torch.zeros(1, 16, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        blk.model[0][0].fn[0](torch.zeros(1, 8, 8, 16, device=DEV))


def test_unsupported_hidden_width_raises_and_names_it(meta):
    """a hidden width outside the kernel's set: NotImplementedError that names it, nothing launched, no fallback"""
    with pytest.raises(NotImplementedError, match="hidden width of 24"):
        SQ.BiLSTM2D(32, 24).to(DEV)(torch.zeros(1, 4, 4, 32, device=DEV))
    SQ.sequencer_settings["odd"] = [[1, 1, 1, 1], [32, 32, 32, 32], [16, 16, 64, 16], 3]
    try:
        with pytest.raises(NotImplementedError, match="stage 3.*hidden width of 64"):
            SQ.Sequencer2D("odd", num_classes=3).to(DEV).eval()(torch.zeros(1, 3, 28, 28, device=DEV))
    finally:
        del SQ.sequencer_settings["odd"]


# ------------------------------------------------------------------ lifecycle (tests/test_gpu_lifecycle.py's helpers on a registered Config)
def sequencer_config():
    """the tiny configuration at 56 x 56 with widened recurrent weights, registered where tests/test_gpu_lifecycle.py's helpers look rows up"""
    if NAME not in LH._CACHE:
        meta = json.loads(str(np.load(FIX)["meta"]))
        add_tiny_settings(meta)
        ctor, kw = functools.partial(SQ.Sequencer2D, "tiny"), {"num_classes": meta["tiny_classes"]}
        model = load_portable(ctor(**kw), meta["tiny_seed"])
        widen(model, meta)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        LH._CACHE[NAME] = LH.Config(NAME, ctor, kw, sd, tuple(meta["tiny_sizes"][0]), meta["tiny_classes"])
    return LH._CACHE[NAME]


def lifecycle():
    sequencer_config()
    return importlib.import_module("test_gpu_lifecycle")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_weight_update_reaches_the_next_forward(dtype):
    """the visible update forms that need no backward (in place under no_grad and load_state_dict among them), and set_compute_dtype back and
    forth with an update in between"""
    GL = lifecycle()
    cfg, dt = sequencer_config(), GL.DT[dtype]
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
    """one entry per role at a time: weight_ih / bias_ih / bias_hh are the concatenated and folded ones, weight_hh the scan's operand"""
    GL = lifecycle()
    roles = LH.one_per_role(sequencer_config().fresh())
    assert any("weight_hh_l_reverse" in r for r in roles) and any("bias_hh_l" in r for r in roles) and any("rnn_h.weight_ih_l" in r for r in roles)
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
def test_results_and_inputs_are_the_callers(dtype):
    GL = lifecycle()
    cfg = sequencer_config()
    m = GL.warm_model(cfg)
    assert GL.check_callers_own(m, m, GL.images(cfg, 3, GL.DT[dtype], seed=6)) >= 1
    blk = m.stages[0][1]
    for mod, shape in ((blk, (3, 32, 8, 8)), (blk.model[0][0].fn[0], (3, 8, 8, 32))):
        x = torch.from_numpy(portable_input(shape, seed=8)).to(DEV).to(GL.DT[dtype])
        assert GL.check_callers_own(m, mod, x) >= 2


def test_deterministic_and_in_flight():
    """two forwards give the same bits, and so do two in flight: the batches alternate over two streams of the caller's own, each behind the
    stream that made its input, nothing synchronised in between.  (High-priority streams: torch hands them out of a pool of their own, so this
    file leaves the pool the schedules of tests/test_gpu_streams.py draw from as it found it.)"""
    GL = lifecycle()
    cfg = sequencer_config()
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
    cfg = sequencer_config()
    model = GL.warm_model(cfg)
    model.train()
    with pytest.warns(UserWarning, match="inference-only"):
        with torch.no_grad():
            out = model(GL.images(cfg, 2, torch.float32))
    assert out.grad_fn is None
    with torch.enable_grad():
        assert model(GL.images(cfg, 2, torch.float32)).grad_fn is None
