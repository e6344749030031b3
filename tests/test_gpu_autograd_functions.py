"""-m gpu: every torch.autograd.Function of autograd.py called directly, on the cases of tests/autograd_cases.py (shapes, restatements and gates
are described there; test_autograd_host.py holds the table to the list of Functions and checks that every case can tell a wrong derivative).

  (a) values     forward and every gradient against the fp64 restatement, for the Functions no other test calls with a backward
  (b) layouts    every tensor operand and the cotangent, one at a time, as a column slice of a NaN-filled wider buffer (at column 8; at
                 column 3 of an odd pitch), as a view with a non-unit column stride, as broadcast views with strides (0, 1) and (0, 0), and the
                 cotangent as `y.sum().backward()` delivers it: every output and every gradient has the bits of the run on contiguous copies,
                 and the caller's buffers keep their bits
  (c) subsets    every non-empty subset of requires_grad: the requested gradients have the bits of the all-on run, the others stay None
  (d) tape       backward twice over a retained graph accumulates exactly 2 g (every storage type: doubling is exact); a second differentiation raises once_differentiable's error
The views only ever lie inside buffers allocated here, and every Function copies what its kernels cannot address (autograd._rows, _rows16).
The measured error / gate ratios of (a) are in profiles/autograd_function_errors.txt."""
import itertools

import pytest
import torch

import autograd_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run(case, args, dy, req=None):
    """Function.apply on leaves made of `args` (layouts kept), requires_grad on the operands `req` (default: every differentiable one);
    dy None: y.sum().backward().  Returns (out, {operand index: .grad})"""
    req = case.diff if req is None else req
    a = list(args)
    for i in case.diff:
        a[i] = a[i].detach()
        a[i].requires_grad_(i in req)
    try:
        out = case.function().apply(*a)
        assert out.requires_grad
        if dy is None:
            out.sum().backward()
        else:
            out.backward(dy)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):          # the device is gone for this process: run nothing more on it
            pytest.exit("GPU fault in %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    return out.detach(), {i: a[i].grad for i in case.diff}


def setup(case, dtype):
    args = case.build(dtype, DEV)
    with torch.no_grad():
        shape = case.function().apply(*args).shape
    return args, T.cotangent(case, dtype, shape, DEV)


# ------------------------------------------------------------------ (a) values
@pytest.mark.parametrize("case,dtype", T.VALUE_CASES, ids=T.ids(T.VALUE_CASES))
def test_values_against_the_fp64_restatement(case, dtype):
    args, dy = setup(case, dtype)
    true = T.evaluate(case, dtype, args, dy)
    gate = T.gates(case, dtype, args, dy, true)
    out, grads = run(case, args, dy)
    assert out.dtype == dy.dtype and tuple(out.shape) == tuple(true["out"].shape)
    for name, g in gate.items():
        got = out if name == "out" else grads[int(name[1:])]
        assert got is not None and tuple(got.shape) == tuple(true[name].shape), (case.name, name)
        assert torch.isfinite(got).all(), (case.name, name)
        if g is None:
            ratio = 0.0 if torch.equal(got.cpu(), true[name].to(got.dtype)) else float("inf")
        else:
            ratio = ((got.double().cpu() - true[name]).abs() / g.clamp_min(1e-300)).max().item()
        print("AGF %-34s %-4s %-4s %s error/gate = %.3f" % (case.name, T.IDS[dtype], name, "exact" if g is None else "gated", ratio))
        assert ratio <= 1.0, (case.name, T.IDS[dtype], name, ratio)


# ------------------------------------------------------------------ (b) layouts
def poisoned(shape, like):
    return torch.full(shape, NAN, dtype=like.dtype, device=like.device)


def lay_slice(col, odd):
    def make(t):
        last = t.shape[-1]
        width = last + 16 if not odd else last + 7 + (last % 2)                  # odd: an odd pitch
        buf = poisoned(tuple(t.shape[:-1]) + (width,), t)
        buf[..., col:col + last] = t
        return buf[..., col:col + last], buf
    return make


def lay_strided(t):
    """a non-unit stride on the last axis: the .t() of a transposed copy; a 1-D or single-row operand: every other element of a NaN-filled buffer"""
    if t.dim() == 1 or t.shape[-2] == 1:                                         # (transposing a single row would leave the column stride 1)
        buf = poisoned(tuple(t.shape[:-1]) + (2 * t.shape[-1],), t)
        buf[..., ::2] = t
        return buf[..., ::2], buf
    buf = t.transpose(-1, -2).contiguous()
    return buf.transpose(-1, -2), buf


def lay_rows_same(t):
    buf = t[0:1].clone()
    return buf.expand(t.shape), buf


def lay_all_same(t):
    buf = t.reshape(-1)[0:1].clone()
    return buf[0].expand(t.shape), buf


LAYOUTS = [("slice@8", lay_slice(8, False), False), ("slice@3,odd", lay_slice(3, True), False), ("strided", lay_strided, False),
           ("broadcast(0,1)", lay_rows_same, True), ("broadcast(0,0)", lay_all_same, True)]


def agree(case, what, got, want):
    out, grads = got
    wout, wgrads = want
    assert same_bits(out, wout), (case.name, what, "out")
    for i in case.diff:
        assert (grads[i] is None) == (wgrads[i] is None) and (grads[i] is None or same_bits(grads[i], wgrads[i])), (case.name, what, "d%d" % i)


@pytest.mark.parametrize("case,dtype", T.ALL_CASES, ids=T.ids(T.ALL_CASES))
def test_layouts_compute_the_bits_of_the_contiguous_run(case, dtype):
    args, dy = setup(case, dtype)
    dy0 = dy.clone()
    base = run(case, args, dy)
    assert all(torch.isfinite(g).all() for g in base[1].values() if g is not None) and torch.isfinite(base[0]).all()
    operands = [i for i, v in enumerate(args) if torch.is_tensor(v)]
    for pos in operands + ["dy"]:
        t = dy if pos == "dy" else args[pos]
        for name, make, changes in LAYOUTS:
            if changes and t.dim() == 1 and name == "broadcast(0,1)":
                continue                                                         # a 1-D operand has one broadcast form
            view, buf = make(t)
            before = buf.clone()
            a = list(args)
            if pos == "dy":
                got = run(case, a, view)
                want = base if not changes else run(case, a, view.contiguous())
            else:
                a[pos] = view
                got = run(case, a, dy)
                if changes:
                    a[pos] = view.contiguous()
                    want = run(case, a, dy)
                else:
                    want = base
            agree(case, (pos, name), got, want)
            assert same_bits(buf, before), (case.name, pos, name, "the caller's buffer changed")
    # what y.sum().backward() delivers: the all-ones cotangent, strides (0, 0)
    agree(case, ("dy", "sum"), run(case, args, None), run(case, args, torch.ones_like(dy)))
    for i in operands:
        assert same_bits(args[i], case.build(dtype, DEV)[i]), (case.name, i, "an operand changed")
    assert same_bits(dy, dy0), (case.name, "the cotangent changed")


# single rows: torch calls every (1, C) view contiguous, so `.contiguous()` hands it back with whatever base and row stride it has
def row_in_the_middle(t):
    C = t.shape[1]
    buf = poisoned((4, C + 7 + C % 2), t)                                        # an odd pitch, the row at an odd offset
    buf[2:3, 3:3 + C] = t
    return buf[2:3, 3:3 + C], buf


def column_transposed(width):
    def make(t):
        buf = poisoned((t.shape[1], width), t)                                   # width 1: strides (1, 1), a row stride below the width
        buf[:, width // 2] = t[0]
        return buf[:, width // 2:width // 2 + 1].t(), buf
    return make


ROW_LAYOUTS = [("row@3,odd", row_in_the_middle), ("column.t()", column_transposed(1)), ("column of 5 .t()", column_transposed(5))]
ROW_CASES = [(c, d) for c, d in T.ALL_CASES if c.fn in ("Affine", "ScaleAdd", "Mul", "ConcatCols", "Gelu", "Linear", "LayerNorm", "Dropout", "BatchNormTrain")]


@pytest.mark.parametrize("case,dtype", ROW_CASES, ids=T.ids(ROW_CASES))
def test_single_row_views_compute_the_bits_of_the_plain_row(case, dtype):
    """M = 1 for the Functions whose row count is free: the first row of the case's operands"""
    args = [v[0:1].clone() if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == T.M else v for v in case.build(dtype, DEV)]
    with torch.no_grad():
        shape = case.function().apply(*args).shape
    assert shape[0] == 1
    dy = T.cotangent(case, dtype, shape, DEV)
    base = run(case, args, dy)
    rows = [i for i, v in enumerate(args) if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == 1]
    assert rows
    for pos in rows + ["dy"]:
        t = dy if pos == "dy" else args[pos]
        for name, make in ROW_LAYOUTS:
            view, buf = make(t)
            assert torch.equal(view, t)
            before = buf.clone()
            a = list(args)
            if pos == "dy":
                got = run(case, a, view)
            else:
                a[pos] = view
                got = run(case, a, dy)
            agree(case, (pos, name), got, base)
            assert same_bits(buf, before), (case.name, pos, name, "the caller's buffer changed")


# ------------------------------------------------------------------ (c) gradient subsets
SUBSET_CASES = [(c, d) for c, d in T.ALL_CASES if len(c.diff) > 1]


@pytest.mark.parametrize("case,dtype", SUBSET_CASES, ids=T.ids(SUBSET_CASES))
def test_every_subset_of_requires_grad(case, dtype):
    args, dy = setup(case, dtype)
    _, full = run(case, args, dy)
    assert all(g is not None for g in full.values()), case.name
    for n in range(1, len(case.diff)):
        for req in itertools.combinations(case.diff, n):
            _, grads = run(case, args, dy, req=req)
            for i in case.diff:
                if i in req:
                    assert grads[i] is not None and same_bits(grads[i], full[i]), (case.name, req, i)
                else:
                    assert grads[i] is None, (case.name, req, i)


# ------------------------------------------------------------------ (d) tape
@pytest.mark.parametrize("case,dtype", T.ALL_CASES, ids=T.ids(T.ALL_CASES))
def test_retained_graph_accumulates_and_second_derivative_is_refused(case, dtype):
    args, dy = setup(case, dtype)
    _, once = run(case, args, dy)
    a = list(args)
    for i in case.diff:
        a[i] = a[i].detach().requires_grad_(True)
    out = case.function().apply(*a)
    out.backward(dy, retain_graph=True)
    out.backward(dy)
    torch.cuda.synchronize()
    for i in case.diff:
        assert a[i].grad.dtype == a[i].dtype                                     # fp32 parameters next to 16-bit operands: g + g is exact in both
        assert torch.equal(a[i].grad, once[i] * 2), (case.name, i)
    for i in case.diff:
        a[i] = a[i].detach().requires_grad_(True)
    out = case.function().apply(*a)
    # a cotangent that itself depends on the operands (d/d out of sum out^2), so that a second derivative would have to pass through the backward
    grads = torch.autograd.grad((out.double() ** 2).sum(), [a[i] for i in case.diff], create_graph=True)
    assert all(g.requires_grad for g in grads)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        sum(g.double().sum() for g in grads).backward()


# ================================================================== model level: the conditions no whole-model test varies
# The tiny configurations test_gpu_lifecycle.py registers for the trainable families, fp32 and bf16, drop rates 0.  Every comparison is with the
# all-trainable step on a contiguous cotangent and an image without a gradient -- the one set of conditions the other train tests use.
import warnings                                                                  # noqa: E402

import numpy as np                                                               # noqa: E402
import torch.nn.functional as F                                                  # noqa: E402

from test_gpu_backward_kernels import U32                                        # noqa: E402
from test_gpu_lifecycle import DT, config, grad_mismatches, grads, images, train_step, warm_model     # noqa: E402
from test_lifecycle_host import BN_FAMILIES                                      # noqa: E402
from test_lifecycle_host import TINY as TINY_MODELS                              # noqa: E402

MODEL_CASES = [(n, d) for n in TINY_MODELS for d in ("fp32", "bf16")]
MODEL_IDS = ["%s-%s" % c for c in MODEL_CASES]
_STEPS = {}


def new_model(name):
    cfg = config(name)
    return cfg, warm_model(cfg, **cfg.train_kw())


def all_trainable(name, dtype, batch=2):
    """(x, logits, gradients) of the step every comparison refers to; computed once per configuration and left unchanged"""
    key = (name, dtype, batch)
    if key not in _STEPS:
        cfg, m = new_model(name)
        x = images(cfg, batch, DT[dtype], seed=21)
        logits = train_step(m, x)
        g = grads(m)
        assert any(v is not None for v in g.values()) and all(torch.isfinite(v).all() for v in g.values() if v is not None), name
        _STEPS[key] = (x, logits, g)
    return _STEPS[key]


def head_of(m, classes):
    lin = [mod for mod in m.modules() if isinstance(mod, torch.nn.Linear) and mod.out_features == classes]
    assert lin
    return lin[-1]


def norm_parameters(m):
    """the parameters of every normalisation layer: LayerNorm (torch's and MS-MLP's own), GroupNorm, BatchNorm2d, ResMLP's Aff"""
    out = [p for mod in m.modules() if "Norm" in type(mod).__name__ or type(mod).__name__ == "Aff" for p in mod.parameters(recurse=False)]
    assert out
    return out


def freeze_all_but_head(m, classes):
    keep = {id(p) for p in head_of(m, classes).parameters()}
    for p in m.parameters():
        p.requires_grad_(id(p) in keep)


def freeze_head(m, classes):
    for p in head_of(m, classes).parameters():
        p.requires_grad_(False)


def freeze_norms(m, classes):
    for p in norm_parameters(m):
        p.requires_grad_(False)


@pytest.mark.parametrize("name,dtype", MODEL_CASES, ids=MODEL_IDS)
def test_frozen_subsets_leave_the_other_gradients_their_bits(name, dtype):
    x, logits, full = all_trainable(name, dtype)
    for freeze in (freeze_all_but_head, freeze_head, freeze_norms):
        cfg, m = new_model(name)
        freeze(m, cfg.classes)
        frozen = {k for k, p in m.named_parameters() if not p.requires_grad}
        assert frozen and len(frozen) < len(full), (name, freeze.__name__)
        assert torch.equal(train_step(m, x), logits), (name, freeze.__name__)
        got = grads(m)
        assert all(got[k] is None for k in frozen), (name, freeze.__name__, [k for k in frozen if got[k] is not None][:4])
        rest = {k: v for k, v in got.items() if k not in frozen}
        bad = grad_mismatches(rest, {k: full[k] for k in rest})
        assert not bad, (name, freeze.__name__, bad[:6])


def step_with(name, x, backward):
    cfg, m = new_model(name)
    m.train()
    logits = m(x)
    backward(logits)
    torch.cuda.synchronize()
    return logits.detach(), grads(m)


@pytest.mark.parametrize("name,dtype", MODEL_CASES, ids=MODEL_IDS)
def test_cotangent_forms(name, dtype):
    """sum(): autograd hands the train path an expanded scalar (strides 0, 0).  cross_entropy: the cotangent arrives through the loss's own backward
    and a dtype cast.  Both must equal, bit for bit, the step driven by the same numbers as a plain contiguous tensor.  The loss's own gradient is
    taken on the CPU in fp64 and the cotangent that reached the model is held to it.  (A step driven by the CPU's fp32 gradient is not compared:
    torch's CPU and GPU softmax differ in the last fp32 bits, so the two steps are not bit-equal, and no bound on their parameter gradients follows
    from the cotangent's without the norm of the whole backward.)  Gate of the cotangent g = (p - onehot) / B, counted from torch's fp32
    log_softmax and its backward, u = U32, d = max - min of the row's logits, K classes: z = x - max (|z| u on the exponent), exp(z) (2 u: one
    ulp), the sum of K terms ((K - 1) u), log (u |lse| <= u ln K, plus the sum's relative error), logp = z - lse (u (d + ln K)), p = exp(logp)
    (2 u), p - onehot (u), / B (2 u: the reciprocal or the quotient, and a product): (3 d + K + 2 ln K + 6) u (p + onehot) / B, plus one rounding
    of g in the logits' type."""
    x, logits, _ = all_trainable(name, dtype)
    _, g_sum = step_with(name, x, lambda lg: lg.float().sum().backward())
    _, g_ones = step_with(name, x, lambda lg: lg.float().backward(torch.ones(lg.shape, device=DEV)))
    assert not grad_mismatches(g_sum, g_ones), (name, grad_mismatches(g_sum, g_ones)[:6])
    target = torch.arange(logits.shape[0]) % logits.shape[1]
    seen = []

    def ce(lg):
        lg.register_hook(lambda g: seen.append(g.detach().clone()))
        F.cross_entropy(lg.float(), target.to(DEV)).backward()
    lg_ce, g_ce = step_with(name, x, ce)
    assert torch.equal(lg_ce, logits) and len(seen) == 1 and seen[0].dtype == logits.dtype
    _, g_explicit = step_with(name, x, lambda lg: lg.backward(seen[0].contiguous().clone()))
    assert not grad_mismatches(g_ce, g_explicit), (name, grad_mismatches(g_ce, g_explicit)[:6])
    # the loss's own gradient on the CPU, in fp64
    l64 = logits.double().cpu().requires_grad_(True)
    F.cross_entropy(l64, target).backward()
    p = torch.softmax(l64.detach(), 1)
    eps = {"fp32": 2.0 ** -23, "bf16": 2.0 ** -7}[dtype]
    K = logits.shape[1]
    d = (l64.detach().max(1, keepdim=True).values - l64.detach().min(1, keepdim=True).values)
    gate = eps * l64.grad.abs() + (3 * d + K + 2 * float(np.log(K)) + 6) * U32 * (p + F.one_hot(target, K)) / logits.shape[0]
    err = (seen[0].double().cpu() - l64.grad).abs()
    assert (err <= gate).all(), (name, float((err / gate).max()))


@pytest.mark.parametrize("name,dtype", MODEL_CASES, ids=MODEL_IDS)
def test_an_image_that_requires_grad_warns_once_and_changes_nothing(name, dtype):
    x, logits, full = all_trainable(name, dtype)
    cfg, m = new_model(name)
    xg = x.clone().requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert torch.equal(train_step(m, xg), logits)
        first = grads(m)
        m.zero_grad(set_to_none=True)
        train_step(m, xg)                                                        # the same model object again: no second warning
    mine = [w for w in caught if "gradient with respect to the input image is not produced" in str(w.message)]
    assert len(mine) == 1 and mine[0].category is UserWarning, [str(w.message) for w in caught]
    assert str(mine[0].message) == "%s.train(): the gradient with respect to the input image is not produced (parameter gradients only)" % type(m).__name__
    assert xg.grad is None
    assert not grad_mismatches(first, full), (name, grad_mismatches(first, full)[:6])


@pytest.mark.parametrize("name,dtype", MODEL_CASES, ids=MODEL_IDS)
def test_a_batch_of_one_takes_a_finite_train_step(name, dtype):
    cfg, m = new_model(name)
    x = images(cfg, 1, DT[dtype], seed=22)
    logits = train_step(m, x)
    assert logits.shape == (1, cfg.classes) and torch.isfinite(logits).all()
    got = grads(m)
    assert any(v is not None for v in got.values())
    assert all(torch.isfinite(v).all() for v in got.values() if v is not None), [k for k, v in got.items() if v is not None and not torch.isfinite(v).all()][:6]
    assert all(torch.isfinite(b).all() for b in m.buffers() if b.is_floating_point())
    if name in BN_FAMILIES:
        assert all(int(mod.num_batches_tracked) == 1 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(n for n in BN_FAMILIES if n in TINY_MODELS))
@pytest.mark.parametrize("hw", [(1, 2), (4, 4), (3, 5)])
def test_batch_of_one_running_variance_is_torchs(name, hw, dtype):
    """ConvMixer's and Sparse-MLP's first BatchNorm2d on the map of ONE image (down to two pixels: rows / (rows - 1) = 2) through
    autograd.batch_norm_train, against nn.BatchNorm2d in fp64 on the CPU on the same stored values.  The helper is called directly on a synthetic
    map: the models' own batch-of-one step (test_a_batch_of_one_takes_a_finite_train_step) goes through the same helper (conv_mixer.py, sparse_mlp.py
    _forward_train) but is checked there for finiteness and the batch counter only, not compared with torch.  Gate: the running buffers are fp32 (one
    rounding each), the batch sums mlpk_col_sum's 8 U32 sum |terms| of test_col_sum_and_col_dot, carried through var = s2 / n - mean^2."""
    cfg, m = new_model(name)
    bn = next(mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    C, rows = bn.num_features, hw[0] * hw[1]
    t = T.distinct((rows, C), DT[dtype], 61, DEV)
    ref = torch.nn.BatchNorm2d(C, eps=bn.eps, momentum=bn.momentum).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in bn.state_dict().items()})
    ref.train()
    ref(t.double().cpu().reshape(1, hw[0], hw[1], C).permute(0, 3, 1, 2))
    bn.train()
    old_mean, old_var = (bn.state_dict()[k].detach().double().cpu().clone() for k in ("running_mean", "running_var"))
    T.AG().batch_norm_train(t, bn)
    torch.cuda.synchronize()
    t64 = t.double().cpu()
    mom, factor = bn.momentum, rows / max(rows - 1, 1)
    assert factor > 1
    # the update `running.mul_(1 - mom).add_(mom * stat.to(fp32))`: four fp32 roundings on terms of these magnitudes
    upd_mean = 4 * U32 * ((1 - mom) * old_mean.abs() + mom * t64.mean(0).abs())
    upd_var = 4 * U32 * ((1 - mom) * old_var.abs() + mom * t64.var(0, unbiased=True))
    gate_mean = upd_mean + mom * 8 * U32 * t64.abs().mean(0) + 1e-30
    gate_var = upd_var + mom * factor * 8 * U32 * ((t64 ** 2).mean(0) + 2 * t64.mean(0).abs() * t64.abs().mean(0)) + 1e-30
    em = (bn.running_mean.double().cpu() - ref.running_mean).abs()
    ev = (bn.running_var.double().cpu() - ref.running_var).abs()
    print("AGF batch-of-one %s %s rows %d: running mean %.3f, running var %.3f of the gate" % (name, dtype, rows, float((em / gate_mean).max()), float((ev / gate_var).max())))
    assert (em <= gate_mean).all() and (ev <= gate_var).all(), (name, rows, float((em / gate_mean).max()), float((ev / gate_var).max()))
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)
