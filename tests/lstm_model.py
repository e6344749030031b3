"""mlpk_lstm_scan as a plain torch loop on the CPU, with planted faults, and the checks that pin the kernel's recurrence (a plain helper module, like
guard.py and philox_ref.py).

`scan_model` is the contract of include/mlpk.h step by step: storage-type operands, fp32 accumulation, h rounded to the storage type ONCE per step,
the layout of `to_seqs` / `from_seqs`.  `fault` breaks it the way the kernel could be broken without the value tests noticing:
  k_swap        two k slots exchanged in every row of W_hh (a wrong lane-to-k map of the A or B fragment)
  row_tile      hidden units 16 .. 31 use the W_hh rows of units 0 .. 15 (a wave that loads another wave's rows; no fault at hid 16: one wave)
  dir_weights   the reverse direction runs on the forward direction's weights
  stale_h       a step reads h of two steps ago (the LDS double buffer not flipped)
  dead_subtile  sequences 16 .. 31 of every 32 are not stored (the second 16-sequence tile of a workgroup masked off)
The checks take a `scan(xp, whh, B, H, W, hid, dtype, axis) -> (B H W, 2 hid)` callable: the kernel on the GPU (tests/test_gpu_sequencer.py) or the
model here (tests/test_sequencer_host.py, which holds every fault against every check):
  replay_check     W_hh one-hot (+-1 at column pi(j) of row j of ONE gate, nothing else), the forget gate at -200: the product term is +-h[pi(j)]
                   exactly and the cell state is forgotten, so the scan equals ONE more launch on B H W sequences of length 1 whose fed gate is
                   built from the scan's own output at the previous pixel.  Bit for bit, no tolerance.
  forget_check     the same one-hot rows in the forget gate (c_{-1} = 0: no single step replays it) against fp64 nn.LSTM, under the rule of
                   tests/test_gpu_sequencer.py; the gate at most a fifth of the distance to the restatement with pi = identity.
  identical_check  every sequence of the map gets the same xp: every sequence's output has sequence 0's bits."""
import torch

from guard import assert_bits_equal, assert_finite

FAULTS = ("k_swap", "row_tile", "dir_weights", "stale_h", "dead_subtile")
GATES = {"i": 0, "f": 1, "g": 2, "o": 3}
KINDS = ("shift", "random")
K_SWAP = (1, 2)                                                        # the two k slots `k_swap` exchanges


def to_seqs(v, B, H, W, axis):
    """(B H W, n) rows of the map -> (sequences, L, n): the reference's reshapes (sequencer.py:40, :42)"""
    v = v.reshape(B, H, W, -1)
    return v.permute(0, 2, 1, 3).reshape(B * W, H, -1) if axis == 0 else v.reshape(B * H, W, -1)


def from_seqs(o, B, H, W, axis):
    """(sequences, L, n) -> (B H W, n) (sequencer.py:41, :43)"""
    o = o.reshape(B, W, H, -1).permute(0, 2, 1, 3) if axis == 0 else o.reshape(B, H, W, -1)
    return o.reshape(B * H * W, -1)


def restate(xp, whh, B, H, W, hid, axis, dtype):
    """torch.nn.LSTM(bidirectional, batch_first) on the CPU in `dtype`: the projections xp enter through weight_ih = [I | 0] (forward) and
    [0 | I] (reverse) with zero biases, so W_ih x + b is xp's own block exactly, in every type"""
    rnn = torch.nn.LSTM(8 * hid, hid, num_layers=1, batch_first=True, bias=True, bidirectional=True)
    eye, zero = torch.eye(4 * hid), torch.zeros(4 * hid, 4 * hid)
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        rnn.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        rnn.weight_hh_l0.copy_(whh[0])
        rnn.weight_hh_l0_reverse.copy_(whh[1])
        for n in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(rnn, n).zero_()
        out, _ = rnn.to(dtype)(to_seqs(xp, B, H, W, axis).to(dtype))
    return from_seqs(out, B, H, W, axis).double()


# ------------------------------------------------------------------ the model
def _sigmoid(z, dtype):
    """fp32 storage: evaluated in fp64 and rounded once; the 16-bit types: in fp32 (csrc/mlpk_lstm.hip)"""
    return torch.sigmoid(z.double()).float() if dtype == torch.float32 else torch.sigmoid(z)


def _tanh(z, dtype):
    return torch.tanh(z.double()).float() if dtype == torch.float32 else torch.tanh(z)


def scan_model(xp, whh, B, H, W, hid, dtype, axis, fault=None):
    """xp (B H W, 8 hid), whh (2, 4 hid, hid): CPU tensors holding storage-type values -> (B H W, 2 hid) in `dtype`; what is not stored is NaN"""
    assert fault is None or fault in FAULTS, fault
    sx = to_seqs(xp.to(dtype).float(), B, H, W, axis)
    w = whh.to(dtype).float()
    nseq, L = sx.shape[0], sx.shape[1]
    out = torch.full((nseq, L, 2 * hid), float("nan"))
    for d in range(2):
        wd = w[0 if fault == "dir_weights" else d].clone()
        if fault == "k_swap":
            wd[:, list(K_SWAP)] = wd[:, list(K_SWAP[::-1])]
        if fault == "row_tile" and hid >= 32:
            for g in range(4):
                wd[g * hid + 16:g * hid + 32] = wd[g * hid:g * hid + 16].clone()
        h = torch.zeros(nseq, hid)                                     # h_{-1} = c_{-1} = 0
        older, c = h, torch.zeros(nseq, hid)
        for t in range(L):
            l = L - 1 - t if d else t
            src = older if fault == "stale_h" else h
            z = sx[:, l, 4 * d * hid:4 * (d + 1) * hid] + src @ wd.t()             # fp32 accumulation
            zi, zf, zg, zo = z.split(hid, 1)
            c = _sigmoid(zf, dtype) * c + _sigmoid(zi, dtype) * _tanh(zg, dtype)
            older, h = h, (_sigmoid(zo, dtype) * _tanh(c, dtype)).to(dtype).float()        # rounded ONCE: the next step's operand
            out[:, l, d * hid:(d + 1) * hid] = h
    if fault == "dead_subtile":
        out[torch.arange(nseq) % 32 >= 16] = float("nan")
    return from_seqs(out, B, H, W, axis).to(dtype).contiguous()


# ------------------------------------------------------------------ operands
def random_operands(B, H, W, hid, dtype, seed, hh_scale=2.0):
    """xp (rows, 8 hid) standard normal and whh (2, 4 hid, hid) drawn like nn.LSTM's default init (U(+-1 / sqrt hid)) times hh_scale, both as
    the storage type holds them, in fp32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    xp = torch.randn((B * H * W, 8 * hid), generator=g).to(dtype).float()
    whh = ((torch.rand((2, 4 * hid, hid), generator=g) * 2 - 1) * hid ** -0.5 * hh_scale).to(dtype).float()
    return xp, whh


def permutations(hid, kind, seed):
    """(2, hid): pi_d(j), without fixed points, different in the two directions.  shift: j + 1 (forward), j - 1 (reverse) modulo hid; random: a
    seeded derangement per direction"""
    j = torch.arange(hid)
    if kind == "shift":
        return torch.stack([(j + 1) % hid, (j - 1) % hid])
    g = torch.Generator().manual_seed(seed)
    found = []
    while len(found) < 2:
        p = torch.randperm(hid, generator=g)
        if not bool((p == j).any()) and not any(bool((p == q).any()) for q in found):
            found.append(p)
    return torch.stack(found)


def one_hot_whh(hid, gate, perm, sign):
    """(2, 4 hid, hid): row j of `gate` holds sign[d][j] at column perm[d][j], everything else is zero"""
    whh = torch.zeros(2, 4 * hid, hid)
    for d in range(2):
        whh[d, GATES[gate] * hid + torch.arange(hid), perm[d]] = sign[d]
    return whh


def one_hot_operands(B, H, W, hid, dtype, axis, gate, kind, seed):
    """-> xp, whh, perm (2, hid), sign (2, hid).  gate i / g / o: the forget blocks at -200, the fed gate's blocks zero except at each
    direction's first step; gate f: every block random"""
    g = torch.Generator().manual_seed(seed)
    xp = torch.randn((B * H * W, 8 * hid), generator=g).to(dtype).float()
    sign = torch.where(torch.rand((2, hid), generator=g) < 0.5, -1.0, 1.0)
    perm = permutations(hid, kind, seed + 1)
    assert not bool((perm == torch.arange(hid)).any()) and not bool((perm[0] == perm[1]).all())
    if gate != "f":
        sx = to_seqs(xp, B, H, W, axis).clone()
        gi = GATES[gate]
        for d in range(2):
            sx[:, :, (4 * d + 1) * hid:(4 * d + 2) * hid] = -200.0
        sx[:, 1:, gi * hid:(gi + 1) * hid] = 0.0                       # forward: the first step is l = 0
        sx[:, :-1, (4 + gi) * hid:(5 + gi) * hid] = 0.0                # reverse: l = L - 1
        xp = from_seqs(sx, B, H, W, axis).contiguous()
    return xp, one_hot_whh(hid, gate, perm, sign), perm, sign


def case_seed(hid, dtype, axis, gate, kind):
    return 7000 + 100 * hid + 10 * [torch.float32, torch.float16, torch.bfloat16].index(dtype) + 5 * axis + 1000 * GATES[gate] + KINDS.index(kind)


# ------------------------------------------------------------------ the checks
def replay_check(scan, B, H, W, hid, dtype, axis, gate, kind):
    """-> the number of recurrent terms (fed-gate pre-activations built from the scan's own output) that were not zero"""
    assert gate in ("i", "g", "o")
    xp, whh, perm, sign = one_hot_operands(B, H, W, hid, dtype, axis, gate, kind, case_seed(hid, dtype, axis, gate, kind))
    got = scan(xp, whh, B, H, W, hid, dtype, axis)
    assert_finite(got, "the scan")
    so = to_seqs(got.float(), B, H, W, axis)                           # (sequences, L, 2 hid)
    sx = to_seqs(xp, B, H, W, axis).clone()
    gi = GATES[gate]
    fed_f = sign[0] * so[:, :-1, :hid][:, :, perm[0]]                  # +-h_{t-1}[pi(j)]: exact, and a value of the storage type
    fed_r = sign[1] * so[:, 1:, hid:][:, :, perm[1]]
    sx[:, 1:, gi * hid:(gi + 1) * hid] = fed_f                         # forward half: from pixel l - 1
    sx[:, :-1, (4 + gi) * hid:(5 + gi) * hid] = fed_r                  # reverse half: from pixel l + 1
    want = scan(from_seqs(sx, B, H, W, axis).contiguous(), whh, B * H * W, 1, 1, hid, dtype, axis)
    assert_finite(want, "the single steps")
    assert_bits_equal(got, want, "the scan against its single-step replay (%s gate, %s permutation)" % (gate, kind))
    return int((fed_f != 0).sum() + (fed_r != 0).sum())


def forget_operands(B, H, W, hid, dtype, axis, kind):
    """-> xp, whh (one-hot in the f rows), the same with pi = identity"""
    xp, whh, perm, sign = one_hot_operands(B, H, W, hid, dtype, axis, "f", kind, case_seed(hid, dtype, axis, "f", kind))
    ident = torch.arange(hid).expand(2, hid)
    return xp, whh, one_hot_whh(hid, "f", ident, sign)


def forget_figures(B, H, W, hid, dtype, axis, kind):
    """CPU only -> xp, whh, the fp64 restatement, the gate (4 d in fp32, 2 d in the 16-bit types, d = torch's own distance in that type on the
    same case) and the distance to the restatement whose pi is the identity"""
    xp, whh, whh_id = forget_operands(B, H, W, hid, dtype, axis, kind)
    exact = restate(xp, whh, B, H, W, hid, axis, torch.float64)
    d = float((restate(xp, whh, B, H, W, hid, axis, dtype) - exact).abs().max())
    far = float((restate(xp, whh_id, B, H, W, hid, axis, torch.float64) - exact).abs().max())
    return xp, whh, exact, (4.0 if dtype == torch.float32 else 2.0) * d, far


def forget_check(scan, B, H, W, hid, dtype, axis, kind):
    """-> (error, gate, far)"""
    xp, whh, exact, gate, far = forget_figures(B, H, W, hid, dtype, axis, kind)
    out = scan(xp, whh, B, H, W, hid, dtype, axis)
    assert_finite(out, "out")
    err = float((out.double() - exact).abs().max())
    name = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}[dtype]
    print("forget one-hot %dx%dx%d hid%d axis %d %s %s: |d| %.3e gate %.3e ratio %.3f (identity permutation %.3e away, gate / that %.2e)" % (
        B, H, W, hid, axis, name, kind, err, gate, err / gate if gate else 0.0, far, gate / far))
    assert gate <= 0.2 * far, "the gate %.3e could not tell the permutation from the identity (%.3e away)" % (gate, far)
    assert err <= gate, (err, gate)
    return err, gate, far


def identical_check(scan, B, H, W, hid, dtype, axis):
    """one line of xp for every sequence of the map, random W_hh: where in the map a sequence lies must change no bit"""
    L, nseq = ((H, B * W), (W, B * H))[axis]
    xp, whh = random_operands(1, L, 1, hid, dtype, 9000 + hid + axis)
    sx = xp.reshape(1, L, 8 * hid).expand(nseq, L, 8 * hid)
    got = scan(from_seqs(sx, B, H, W, axis).contiguous(), whh, B, H, W, hid, dtype, axis)
    assert_finite(got, "out")
    so = to_seqs(got, B, H, W, axis).contiguous()
    assert len(torch.unique(so[0].float())) > 16, "sequence 0 is (nearly) constant: the case checks nothing"
    assert_bits_equal(so, so[:1].expand_as(so).contiguous(), "every sequence against sequence 0")
