"""The table behind test_gpu_autograd_functions.py and test_autograd_host.py: one or more cases per `torch.autograd.Function` of autograd.py.

A case holds the Function's name, a constructor of its operands at a small shape (on any device: the host tests build them on the CPU), the indices
of its differentiable operands, and -- for the Functions whose values no other test checks -- a restatement in plain torch that is evaluated in
fp64 on the stored (already rounded) operands and differentiated by torch's own autograd, with a gate per result:

  "move"            pure data movement: bit-exact against the same indexing in the storage type
  ("ew", r, n)      element-wise: r roundings in the storage type (counted from the Function's code, stated in its docstring) and n fp32
                    operations: EPS |ref| + (r - 1) EPS mag + n U32 mag, mag = the sum of the magnitudes of the terms (the restatement on
                    the operands' absolute values); r = 1 is check_close of test_gpu_backward_kernels.py as it stands
  ("red", k)        an fp32 reduction: k U32 x the sum of |terms|, k the multiple test_gpu_backward_kernels.py uses for the same kernel
                    (8: mlpk_col_sum, mlpk_col_dot, mlpk_col_dot_seg)
  ("softmax",) / ("softmax_bwd",)   see softmax_gates

Shapes (none is a model's): M = 37 rows (no multiple of col_dot_kernel's 4 row lanes nor of the 32-wide transpose tile), C = 24 and 70 (70: no
multiple of 64 nor of 8), B = 3 images of S = 10 tokens (the padded token axis is 16 in 16-bit and 12 in fp32), maps of H x W = 4 x 6.  Where mlpk.h
constrains a kernel further the nearest allowed shape stands in and the case's `note` says so.  Operands have pairwise distinct entries (taken from
the storage type's own grid), so an element read from a wrong place is a wrong value.

`faults` are restatements with one plausible mistake each (axes swapped, the forward remap used as its own adjoint, a term dropped, the images of
a batch exchanged); test_autograd_host.py asserts that every one lies at least five gates from the true restatement, i.e. that the case could
tell that wrong derivative from the right one."""
import importlib
import math

import torch
import torch.nn.functional as F

from conftest import load_pkg
from test_gpu_backward_kernels import EPS, TINY, U32, s2_ref

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
M, B, S, H, W = 37, 3, 10, 4, 6
ROWS = B * H * W


def AG():
    load_pkg()
    return importlib.import_module("jittor-mlp_amd.autograd")


def epc(dtype):
    return 4 if dtype == torch.float32 else 8


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------ operands with pairwise distinct entries
_GRID = {}


def _grid(dtype):
    """every value of a 16-bit type with 2^-24 <= |v| < 2 (bf16) / 2^-6 <= |v| < 2 (fp16: products stay normal), largest magnitudes first"""
    if dtype not in _GRID:
        v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype).float()
        lo = 2.0 ** -24 if dtype == torch.bfloat16 else 2.0 ** -6
        v = v[torch.isfinite(v) & (v.abs() >= lo) & (v.abs() < 2.0)]
        _GRID[dtype] = v[torch.argsort(v.abs(), descending=True, stable=True)]
    return _GRID[dtype]


def distinct(shape, dtype, seed, dev="cpu", lo=-2.0, hi=2.0):
    """a tensor of pairwise distinct values of `dtype`: fp32 a shuffled ramp over (lo, hi), 16-bit the n largest grid values, shuffled"""
    n = int(math.prod(shape))
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n, generator=g)
    if dtype == torch.float32:
        v = ((perm.double() + 0.5) / n * (hi - lo) + lo).float()
    else:
        grid = _grid(dtype)
        assert n <= grid.numel(), (n, grid.numel())
        v = grid[:n][perm].to(dtype)
    assert torch.unique(v.float()).numel() == n
    return v.reshape(shape).to(dev)


def param(shape, seed, dev="cpu", lo=0.5, hi=1.5):
    return distinct(shape, torch.float32, seed, dev, lo, hi)


# ------------------------------------------------------------------ restatements (plain torch; any float dtype; differentiable)
def shift_axis(v, s, axis):
    """out[i] = v[i + s] along axis, zero outside"""
    n = v.shape[axis]
    out = torch.zeros_like(v)
    if abs(s) >= n:
        return out
    src = [slice(None)] * v.dim()
    dst = [slice(None)] * v.dim()
    src[axis] = slice(max(s, 0), n + min(s, 0))
    dst[axis] = slice(max(-s, 0), n - max(s, 0))
    out[tuple(dst)] = v[tuple(src)]
    return out


def r_tokens_to_rows(dt, x, B_, S_):
    C = x.shape[1]
    return F.pad(x.reshape(B_, S_, C).transpose(1, 2), (0, round_up(S_, epc(dt)) - S_)).reshape(B_ * C, -1)


def r_rows_to_tokens_add(dt, y, x, B_, S_):
    C = x.shape[1]
    return x + y.reshape(B_, C, S_).transpose(1, 2).reshape(B_ * S_, C)


def r_rows_to_tokens(dt, y, B_, S_, C):
    return y.reshape(B_, C, S_).transpose(1, 2).reshape(B_ * S_, C)


def r_token_mean(dt, x, B_, S_):
    return x.reshape(B_, S_, -1).mean(1)


def r_image_sum(dt, x, B_, S_):
    return x.reshape(B_, S_, -1).sum(1)


def r_affine(dt, x, alpha, beta):
    y = x * alpha.reshape(-1)
    return y + beta.reshape(-1) if beta is not None else y


def r_scale_add(dt, x, z, gamma):
    return x + (gamma.reshape(-1) * z if gamma is not None else z)


def r_mul(dt, u, v):
    return u * v


def r_row_scale(dt, x, s, period):
    return x * s.repeat_interleave(period)[:, None].to(x.dtype)


def r_shift(dt, x, B_, H_, W_, ksz, dim):
    C = x.shape[1]
    v = x.reshape(B_, H_, W_, C)
    group = (C + ksz - 1) // ksz
    out = torch.zeros_like(v)
    for c0 in range(0, C, group):
        out[..., c0:c0 + group] = shift_axis(v[..., c0:c0 + group], ksz // 2 - c0 // group, 1 if dim == 2 else 2)
    return out.reshape(-1, C)


def r_merge(dt, x, B_, H_, W_):
    v = x.reshape(B_, H_, W_, -1)
    return torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1).reshape(B_ * (H_ // 2) * (W_ // 2), -1)


def r_vip_permute(dt, x, B_, H_, W_, seg, which):
    C = x.shape[1]
    v = x.reshape(B_, H_, W_, C // seg, seg)
    z = v.permute(0, 2, 3, 1, 4).reshape(B_ * W_ * (C // seg), H_ * seg) if which == 0 else v.permute(0, 1, 3, 2, 4).reshape(B_ * H_ * (C // seg), W_ * seg)
    return F.pad(z, (0, round_up(z.shape[1], epc(dt)) - z.shape[1]))


def r_vip_unpermute(dt, z, B_, H_, W_, C, seg, which):
    G = C // seg
    if which == 0:
        return z[:, :H_ * seg].reshape(B_, W_, G, H_, seg).permute(0, 3, 1, 2, 4).reshape(B_ * H_ * W_, C)
    return z[:, :W_ * seg].reshape(B_, H_, G, W_, seg).permute(0, 1, 3, 2, 4).reshape(B_ * H_ * W_, C)


def r_softmax(dt, hat, B_, C):
    return torch.softmax(hat.reshape(B_, 3, C), 1).reshape(B_, 3 * C)


def r_weighted_sum3(dt, x0, x1, x2, bar, B_, S_):
    C = x0.shape[1]
    b3 = bar.reshape(B_, 3, C).to(x0.dtype)
    return sum(b3[:, k, None, :] * xk.reshape(B_, S_, C) for k, xk in enumerate((x0, x1, x2))).reshape(B_ * S_, C)


def r_s2(dt, x, B_, D1, D2, which, smear):
    """the INTENDED shift: what the backward is the adjoint of in both modes"""
    return s2_ref(x.reshape(B_, D1, D2, -1), which, 0, False).reshape(x.shape)


def r_s2_fwd(dt, x, B_, D1, D2, which, smear):
    return s2_ref(x.reshape(B_, D1, D2, -1), which, 1 if smear else 0, False).reshape(x.shape)


def r_patch_rows(dt, x, B_, H_, W_, ph, pw):
    C = x.shape[1]
    p = x.reshape(B_, H_ // ph, ph, W_ // pw, pw, C).permute(0, 1, 3, 2, 4, 5).reshape(B_ * (H_ // ph) * (W_ // pw), ph * pw * C)
    return F.pad(p, (0, round_up(p.shape[1], epc(dt)) - p.shape[1]))


def r_index_map(dt, x, tab, B_, out_cols):
    idx = tab.fwd.long().to(x.device)
    v = x.reshape(B_, tab.n_in, tab.width)
    return torch.where((idx >= 0)[None, :, None], v[:, idx.clamp_min(0)], torch.zeros((), dtype=x.dtype, device=x.device)).reshape(-1, out_cols)


def r_concat(dt, *parts):
    return torch.cat(parts, 1)


def r_add_periodic(dt, x, t, L):
    return x + t.reshape(L, -1).repeat(x.shape[0] // L, 1).to(x.dtype)


# ------------------------------------------------------------------ faults: a restatement with one mistake -> {result name: wrong value}
def swap_images(t, B_):
    v = t.reshape(B_, -1).clone()
    v[[0, 1]] = v[[1, 0]]
    return v.reshape(t.shape)


def f_images(*names):
    """the images of a batch exchanged in the named results (rows grouped by image)"""
    def fault(case, dt, args, dy, true):
        return {n: swap_images(true[n], B) for n in names}
    fault.__name__ = "images_exchanged"
    return fault


def f_alt(ref, name):
    """another restatement (axes swapped, a term dropped): all of its results"""
    def fault(case, dt, args, dy, true):
        return evaluate(case, dt, args, dy, ref=ref)
    fault.__name__ = name
    return fault


def f_fwd_as_adjoint(case, dt, args, dy, true):
    """the forward remap used as its own adjoint: dx = forward(dy)"""
    a = list(args)
    a[0] = dy
    return {"d0": case.ref(dt, *a)}


def f_mul_operands(case, dt, args, dy, true):
    """each factor's gradient taken with the factor itself"""
    return {"d0": dy * args[0], "d1": dy * args[1]}


def f_softmax_no_sum(case, dt, args, dy, true):
    """the Jacobian's rank-one term dropped"""
    return {"d0": true["out"] * dy}


def f_index_first_reader(case, dt, args, dy, true):
    """the adjoint with multiplicities ignored: every source takes its first reader only"""
    x, tab, B_, _ = args
    inv = tab.inv.long().to(dy.device)[:, 0]
    v = dy.reshape(B_, tab.n_out, tab.width)
    return {"d0": torch.where((inv >= 0)[None, :, None], v[:, inv.clamp_min(0)], torch.zeros((), dtype=dy.dtype)).reshape(x.shape)}


# ------------------------------------------------------------------ the table
class Case:
    def __init__(self, name, fn, build, diff, ref=None, ref_fwd=None, fwd=None, grads=None, faults=(), dtypes=None, note="", values=None):
        self.name, self.fn, self.build, self.diff = name, fn, build, tuple(diff)
        self.ref, self.ref_fwd, self.fwd, self.grads = ref, ref_fwd, fwd, grads or {}
        self.faults, self.dtypes, self.note = tuple(faults), dtypes or DTYPES, note
        self.values = values                 # for a Function without a restatement here: the test that checks its values

    def function(self):
        return getattr(AG(), self.fn)

    def __repr__(self):
        return self.name


def evaluate(case, dt, args, dy, ref=None, absolute=False):
    """the restatement in fp64 on the stored operands: {"out": ..., "d<i>": gradient w.r.t. operand i} (absolute: on |operands| and |dy|: the
    sums of the magnitudes of the terms)"""
    ref = ref or case.ref
    a = []
    for i, v in enumerate(args):
        if torch.is_tensor(v):
            v = v.detach().double().cpu()
            v = v.abs() if absolute else v
            v.requires_grad_(i in case.diff)
        a.append(v)
    g = dy.detach().double().cpu()
    g = g.abs() if absolute else g
    out = ref(dt, *a)
    grads = torch.autograd.grad(out, [a[i] for i in case.diff], g, allow_unused=True)
    res = {"out": out.detach()}
    for i, gr in zip(case.diff, grads):
        res["d%d" % i] = gr if gr is not None else torch.zeros_like(a[i])
    if case.ref_fwd is not None and ref is case.ref:
        with torch.no_grad():
            res["out"] = case.ref_fwd(dt, *a)
    return res


def softmax_gates(case, dt, args, dy, true):
    """SoftmaxBranches (fp32).  Forward, from split_softmax_kernel: e_k = __expf(h_k - m) carries the subtraction's and the log2(e) product's
    roundings (|d_k| u each on the exponent, d_k = m - h_k) and the hardware exp2's ulp (2 u); the sum of three adds 2 u on top of the largest
    e_j's error, the reciprocal one ulp (2 u), the product u: relative e = (4 max_j d_j + 9) u.  Backward: the 4 U32 mag, mag = a (|d| + sum |a d|),
    of test_split_softmax_backward_against_the_fp64_jacobian -- which hands the kernel the exact softmax, while the Function's backward reads the
    forward's own stored bar: a relative error e on every a_j moves dhat_k = a_k (d_k - sum_j a_j d_j) by at most e a_k |d_k - sum| + a_k sum_j e a_j |d_j|
    <= 2 e mag, added here."""
    hat, B_, C = args
    h3 = hat.detach().double().cpu().reshape(B_, 3, C)
    dmax = (h3.max(1, keepdim=True).values - h3.min(1, keepdim=True).values).expand_as(h3).reshape(B_, 3 * C)
    a = true["out"].reshape(B_, 3, C)
    d = dy.detach().double().cpu().reshape(B_, 3, C)
    mag = (a * (d.abs() + (a * d).abs().sum(1, keepdim=True))).reshape(B_, 3 * C)
    e32 = EPS[torch.float32]
    return {"out": e32 * true["out"].abs() + (4 * dmax + 9) * U32 * true["out"].abs(), "d0": e32 * true["d0"].abs() + 4 * U32 * mag + 2 * (4 * dmax + 9) * U32 * mag}


def gates(case, dt, args, dy, true=None):
    """{result name: None (bit-exact) or the fp64 tensor of allowed errors}"""
    true = true or evaluate(case, dt, args, dy)
    if case.fwd == ("softmax",):
        return softmax_gates(case, dt, args, dy, true)
    mag = evaluate(case, dt, args, dy, ref=case.ref, absolute=True)
    out = {}
    for name, spec in [("out", case.fwd)] + [("d%d" % i, case.grads[i]) for i in case.diff]:
        if spec is None:                     # not checked here (TokenMean's forward has its own test)
            continue
        sdt = dt if (name == "out" or torch.is_tensor(args[int(name[1:])]) and args[int(name[1:])].dtype == dt) else torch.float32
        if spec == "move":
            out[name] = None
        elif spec[0] == "ew":
            _, r, n = spec
            out[name] = EPS[sdt] * true[name].abs() + TINY[sdt] + (r - 1) * (EPS[sdt] * mag[name] + TINY[sdt]) + n * U32 * mag[name]
        elif spec[0] == "red":
            out[name] = spec[1] * U32 * mag[name] + 1e-30
        else:
            raise ValueError(spec)
    return out


CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


for C in (24, 70):
    c = "C%d" % C
    add("TokensToRows-" + c, "TokensToRows", lambda dt, dev, C=C: [distinct((B * S, C), dt, 1, dev), B, S], (0,), r_tokens_to_rows, fwd="move",
        grads={0: "move"}, faults=[f_images("out", "d0")])
    add("RowsToTokensAdd-" + c, "RowsToTokensAdd", lambda dt, dev, C=C: [distinct((B * C, S), dt, 2, dev), distinct((B * S, C), dt, 3, dev), B, S], (0, 1),
        r_rows_to_tokens_add, fwd=("ew", 1, 1), grads={0: "move", 1: "move"},
        faults=[f_images("out", "d0"), f_alt(lambda dt, y, x, B_, S_: r_rows_to_tokens(dt, y, B_, S_, x.shape[1]) + 0 * x, "residual_dropped")])
    add("RowsToTokens-" + c, "RowsToTokens", lambda dt, dev, C=C: [distinct((B * C, S), dt, 4, dev), B, S, C], (0,), r_rows_to_tokens, fwd="move",
        grads={0: "move"}, faults=[f_images("out", "d0")])
    add("Affine-" + c, "Affine", lambda dt, dev, C=C: [distinct((M, C), dt, 5, dev), param((1, 1, C), 6, dev), param((C,), 7, dev, -1, 1)], (0, 1, 2), r_affine,
        fwd=("ew", 1, 2), grads={0: ("ew", 1, 1), 1: ("red", 8), 2: ("red", 8)},
        faults=[f_alt(lambda dt, x, a, b: r_affine(dt, x, a, None) + 0 * b.sum(), "beta_dropped")])
    add("ScaleAdd-" + c, "ScaleAdd", lambda dt, dev, C=C: [distinct((M, C), dt, 8, dev), distinct((M, C), dt, 9, dev), param((C,), 10, dev)], (0, 1, 2), r_scale_add,
        fwd=("ew", 1, 2), grads={0: "move", 1: ("ew", 1, 1), 2: ("red", 8)},
        faults=[f_alt(lambda dt, x, z, g: r_scale_add(dt, x, z, None) + 0 * g.sum(), "gamma_dropped")])
    add("Mul-" + c, "Mul", lambda dt, dev, C=C: [distinct((M, C), dt, 11, dev), distinct((M, C), dt, 12, dev)], (0, 1), r_mul,
        fwd=("ew", 1, 1), grads={0: ("ew", 1, 1), 1: ("ew", 1, 1)}, faults=[f_mul_operands])
    add("RowScale-" + c, "RowScale", lambda dt, dev, C=C: [distinct((B * S, C), dt, 13, dev), param((B,), 14, dev, 0.0, 2.0), S], (0,), r_row_scale,
        fwd=("ew", 1, 1), grads={0: ("ew", 1, 1)}, faults=[f_images("out", "d0")], note="period = S = 10")
    for ksz, dim in ((3, 2), (3, 3), (5, 2), (5, 3)):
        add("ShiftNHWC-%s-k%d-dim%d" % (c, ksz, dim), "ShiftNHWC", lambda dt, dev, C=C, ksz=ksz, dim=dim: [distinct((ROWS, C), dt, 15, dev), B, H, W, ksz, dim], (0,),
            r_shift, fwd="move", grads={0: "move"},
            faults=[f_fwd_as_adjoint, f_alt(lambda dt, x, B_, H_, W_, k, d: r_shift(dt, x, B_, H_, W_, k, 5 - d), "axes_swapped"), f_images("out", "d0")])
    add("Merge2x2-" + c, "Merge2x2", lambda dt, dev, C=C: [distinct((ROWS, C), dt, 16, dev), B, H, W], (0,), r_merge, fwd="move", grads={0: "move"},
        faults=[f_alt(lambda dt, x, B_, H_, W_: r_merge(dt, x.reshape(B_, H_, W_, -1).transpose(1, 2).reshape(x.shape), B_, W_, H_), "axes_swapped"),
                f_images("out", "d0")])
    add("ScaleAddNoGamma-" + c, "ScaleAdd", lambda dt, dev, C=C: [distinct((M, C), dt, 17, dev), distinct((M, C), dt, 18, dev), None], (0, 1), r_scale_add,
        fwd=("ew", 1, 1), grads={0: "move", 1: "move"}, faults=[f_alt(lambda dt, x, z, g: x + 0 * z, "z_dropped")])
    for which in (1, 2):
        for smear in (False, True):
            add("S2Shift-%s-which%d-%s" % (c, which, "smear" if smear else "intended"), "S2Shift",
                lambda dt, dev, C=C, which=which, smear=smear: [distinct((ROWS, C), dt, 19, dev), B, H, W, which, smear], (0,), r_s2, ref_fwd=r_s2_fwd,
                fwd="move", grads={0: ("ew", 1, 1)},
                faults=[f_fwd_as_adjoint, f_alt(lambda dt, x, B_, D1, D2, w, s: r_s2(dt, x, B_, D1, D2, 3 - w, s), "axes_swapped"), f_images("d0")])
    add("PatchRowsNHWC-" + c, "PatchRowsNHWC", lambda dt, dev, C=C: [distinct((ROWS, C), dt, 20, dev), B, H, W, 2, 3], (0,), r_patch_rows, fwd="move",
        grads={0: "move"},
        faults=[f_alt(lambda dt, x, B_, H_, W_, ph, pw: F.pad(x.reshape(B_, H_ // ph, ph, W_ // pw, pw, -1).permute(0, 1, 3, 4, 2, 5).reshape(B_ * (H_ // ph) * (W_ // pw), -1),
                                                               (0, round_up(ph * pw * x.shape[1], epc(dt)) - ph * pw * x.shape[1])), "axes_swapped"),
                f_images("out", "d0")])
    add("ConcatCols-" + c, "ConcatCols", lambda dt, dev, C=C: [distinct((M, C), dt, 21, dev), distinct((M, 13), dt, 22, dev), distinct((M, C), dt, 23, dev)], (0, 1, 2),
        r_concat, fwd="move", grads={0: "move", 1: "move", 2: "move"}, faults=[f_alt(lambda dt, a, b, c_: torch.cat([c_, b, a], 1), "parts_exchanged")])
    add("AddPeriodic-" + c, "AddPeriodic", lambda dt, dev, C=C: [distinct((B * S, C), dt, 24, dev), param((1, S, C), 25, dev, -1, 1), S], (0, 1), r_add_periodic,
        fwd=("ew", 1, 1), grads={0: "move", 1: ("red", 8)},
        faults=[f_alt(lambda dt, x, t, L: x + 0 * t.sum(), "t_dropped"), f_alt(lambda dt, x, t, L: r_add_periodic(dt, x, t.flip(1), L), "period_reversed")],
        note="L = S = 10")
    add("WeightedSum3-" + c, "WeightedSum3",
        lambda dt, dev, C=C: [distinct((B * S, C), dt, 33, dev), distinct((B * S, C), dt, 34, dev), distinct((B * S, C), dt, 35, dev), param((B, 3 * C), 36, dev, 0.05, 0.95), B, S],
        (0, 1, 2, 3), r_weighted_sum3, fwd=("ew", 3, 6), grads={0: ("ew", 1, 1), 1: ("ew", 1, 1), 2: ("ew", 1, 1), 3: ("red", 8)},
        faults=[f_alt(lambda dt, x0, x1, x2, bar, B_, S_: r_weighted_sum3(dt, x0, x1, 0 * x2, bar, B_, S_), "term_dropped"), f_images("out", "d0", "d3")],
        note="period = S = 10")
    add("BatchNormTrain-" + c, "BatchNormTrain",
        lambda dt, dev, C=C: [distinct((M, C), dt, 43, dev), param((C,), 44, dev), param((C,), 45, dev, -1, 1), param((C,), 46, dev, -0.2, 0.2).double(),
                              param((C,), 47, dev, 0.5, 1.5).double(), 1e-5], (0, 1, 2), values="test_gpu_train.py (ConvMixer's BatchNorm against fp64)")
    add("DepthwiseConv-" + c, "DepthwiseConv", lambda dt, dev, C=C: [distinct((ROWS, C), dt, 48, dev), param((C, 1, 3, 3), 49, dev, -0.3, 0.3), param((C,), 50, dev, -1, 1), B, H, W],
        (0, 1, 2), values="test_gpu_backward_kernels.py::test_dwconv_plain_adjoint_and_wgrad")
    add("Gelu-" + c, "Gelu", lambda dt, dev, C=C: [distinct((M, C), dt, 26, dev)], (0,), values="test_gpu_backward_kernels.py::test_gelu_elementwise_past_the_grid_cap")
    add("Linear-" + c, "Linear", lambda dt, dev, C=C: [distinct((M, C), dt, 27, dev), param((40, C), 28, dev, -0.3, 0.3), param((40,), 29, dev, -1, 1),
                                                         distinct((M, 40), dt, 30, dev)], (0, 1, 2, 3), values="test_gpu_train.py (the Linear backward against fp64)")

for C in (24, 72):
    c = "C%d" % C
    note = "C = 72 for 70: mlpk_norm_apply / mlpk_pool_mean take C % 8 == 0 only"
    add("TokenMean-" + c, "TokenMean", lambda dt, dev, C=C: [distinct((B * S, C), dt, 31, dev), B, S], (0,), r_token_mean, fwd=None, grads={0: ("ew", 1, 2)},
        faults=[f_images("d0")], note=note)
    add("ImageSum-" + c, "ImageSum", lambda dt, dev, C=C: [distinct((B * S, C), dt, 32, dev), B, S], (0,), r_image_sum, fwd=("ew", 2, S + 2), grads={0: "move"},
        faults=[f_images("out", "d0")], note=note)
    add("LayerNorm-" + c, "LayerNorm", lambda dt, dev, C=C: [distinct((M, C), dt, 37, dev), param((C,), 38, dev), param((C,), 39, dev, -1, 1), 1e-5], (0, 1, 2),
        values="test_gpu_backward_kernels.py::test_layernorm_backward", note=note)
    add("GroupNorm1-" + c, "GroupNorm1", lambda dt, dev, C=C: [distinct((B * S, C), dt, 40, dev), param((C,), 41, dev), param((C,), 42, dev, -1, 1), B, 1e-5], (0, 1, 2),
        values="test_gpu_backward_kernels.py::test_group_norm_backward", note=note)
    add("Dropout-" + c, "Dropout", lambda dt, dev, C=C: [distinct((M, C), dt, 51, dev), 0.25, 1234, 3], (0,), values="test_gpu_dropout.py",
        note="C = 72 for 70: mlpk_dropout takes cols % 4 == 0 only")

for which in (0, 1):
    add("VipPermute-which%d" % which, "VipPermute", lambda dt, dev, which=which: [distinct((ROWS, 24), dt, 52, dev), B, H, W, 4, which], (0,), r_vip_permute, fwd="move",
        grads={0: "move"}, faults=[f_images("out", "d0")], note="C = 24, seg = 4")
    add("VipUnpermute-which%d" % which, "VipUnpermute",
        lambda dt, dev, which=which: [distinct((B * (W if which == 0 else H) * 6, (H if which == 0 else W) * 4 + 8), dt, 53, dev), B, H, W, 24, 4, which], (0,),
        r_vip_unpermute, fwd="move", grads={0: "move"}, faults=[f_images("out", "d0")], note="C = 24, seg = 4; z eight padding columns wide")

add("SoftmaxBranches", "SoftmaxBranches", lambda dt, dev: [distinct((B, 3 * 70), torch.float32, 54, dev, -3, 3), B, 70], (0,), r_softmax, fwd=("softmax",),
    grads={0: ("softmax_bwd",)}, faults=[f_softmax_no_sum, f_images("out", "d0")], dtypes=[torch.float32], note="fp32 in and out by contract")


def _index_case(dt, dev):
    tab = AG().conv_window_table(4, 6, 8, 3, 2, 1, dev, {})
    assert tab.kmax == 4 and bool((tab.fwd < 0).any())
    return [distinct((B * 24, 8), dt, 55, dev), tab, B, 72]


add("IndexMap-convwin", "IndexMap", _index_case, (0,), r_index_map, fwd="move", grads={0: ("ew", 1, 4)}, faults=[f_index_first_reader, f_images("out", "d0")],
    note="conv_window_table(4, 6, 8, 3, 2, 1): overlapping windows (multiplicity up to 4) and padding entries; n = kmax fp32 additions")


def cotangent(case, dtype, out_shape, dev="cpu"):
    return distinct(tuple(out_shape), torch.float32 if case.fn == "SoftmaxBranches" else dtype, 99, dev)


def ids(cases_dtypes):
    return ["%s-%s" % (c.name, IDS[d]) for c, d in cases_dtypes]


VALUE_CASES = [(c, d) for c in CASES if c.ref is not None for d in c.dtypes]
ALL_CASES = [(c, d) for c in CASES for d in c.dtypes]
