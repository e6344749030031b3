"""-m gpu: train-mode Dropout (mlpk_dropout, autograd.Dropout, the Dropout sites of Swin-MLP / AS-MLP / MS-MLP).

  * the kernel: masks bit-equal to tests/philox_ref.py over dtypes, seeds, sites, rates, row pitches and ragged row counts; kept values are
    round(x * scale) exactly; the kept fraction of 2^24 elements; p = 0 / p = 1; in place; independence of sites; argument errors;
  * autograd.Dropout: the gradient is mask * scale * dy bit for bit (the backward is the same call on dy);
  * the models against the REFERENCE's autograd with the same masks (tests/golden/train_dropout_tiny.npz, make_dropout_golden.py):
    logits and every parameter gradient (whole, or evenly spaced entries + max |g| + L2 norm for the large ones), stochastic depth on the
    recorded draws where the case has it;
  * seeding: torch.manual_seed reproduces a run, no_grad train forwards equal grad-enabled ones;
  * the once-only warning of a family whose train path does not apply Dropout."""
import importlib
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import load_pkg
from oracle.portable_init import portable_input

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _nonzero(rows, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand((rows, ld), generator=g) + 0.25) * torch.where(torch.rand((rows, ld), generator=g) < 0.5, -1.0, 1.0)
    return (v * 3.0).to(dtype).to(DEV)


def _expected(x, keep, p):
    """where(keep, round(x * scale), 0) in x's dtype"""
    kept = (x.float() * float(P.scale(p))).to(x.dtype)
    return torch.where(torch.from_numpy(keep).to(DEV), kept, torch.zeros_like(kept))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,ldx,ldy", [(37, 64, 64, 64), (33, 40, 48, 56), (5, 12, 12, 12), (7, 20, 28, 20), (1, 8, 8, 8)])
@pytest.mark.parametrize("seed,site,p", [(0, 0, 0.5), (0x0123456789ABCDEF, 3, 0.1), (2 ** 63 - 5, 17, 0.9), (42, 0xFFFFFFFF, 0.25)])
def test_dropout_mask_matches_numpy(dtype, rows, cols, ldx, ldy, seed, site, p):
    pkg = load_pkg()
    xf = _nonzero(rows, ldx, dtype, seed & 0xFFFF)
    x = xf[:, :cols]
    yf = torch.full((rows, ldy), 7.0, dtype=dtype, device=DEV)
    y = yf[:, :cols]
    pkg.engine.dropout(x, y, rows, cols, p, seed, site)
    torch.cuda.synchronize()
    keep = P.keep_mask(seed, site, p, rows, cols)
    assert torch.equal((y != 0).cpu(), torch.from_numpy(keep)), "mask differs from the numpy restatement"
    assert torch.equal(y, _expected(x, keep, p)), "kept values are not round(x * scale)"
    assert (yf[:, cols:] == 7.0).all(), "wrote past the logical columns"


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_dropout_kept_fraction(p):
    pkg = load_pkg()
    rows, cols = 1 << 14, 1 << 10
    x = torch.ones((rows, cols), dtype=torch.bfloat16, device=DEV)
    y = torch.empty_like(x)
    pkg.engine.dropout(x, y, rows, cols, p, 0xC0FFEE, 1)
    n = rows * cols
    kept = int((y != 0).sum().item())
    sigma = math.sqrt(n * p * (1 - p))
    assert abs(kept - n * (1 - p)) < 6 * sigma, (kept, n * (1 - p), sigma)
    assert torch.equal(y.unique().float().cpu().sort().values, torch.tensor(sorted({0.0, float(torch.tensor(1.0 / (1.0 - p)).bfloat16())})))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_p0_p1_and_in_place(dtype):
    pkg = load_pkg()
    rows, cols = 129, 96
    x = _nonzero(rows, cols, dtype, 3)
    y = torch.full_like(x, 5.0)
    pkg.engine.dropout(x, y, rows, cols, 0.0, 9, 2)
    assert torch.equal(y, x)                                        # p = 0: a copy
    pkg.engine.dropout(x, y, rows, cols, 1.0, 9, 2)
    assert (y == 0).all()                                           # p = 1: nn.Dropout(1.0) -- all zeros
    z = x.clone()
    pkg.engine.dropout(z, z, rows, cols, 0.0, 9, 2)
    assert torch.equal(z, x)                                        # p = 0 in place: nothing
    pkg.engine.dropout(x, y, rows, cols, 0.3, 9, 2)
    pkg.engine.dropout(z, z, rows, cols, 0.3, 9, 2)
    torch.cuda.synchronize()
    assert torch.equal(z, y)                                        # in place == out of place


def test_dropout_sites_are_independent():
    pkg = load_pkg()
    rows, cols, p = 4096, 256, 0.3
    x = torch.ones((rows, cols), dtype=torch.float32, device=DEV)
    a, b = torch.empty_like(x), torch.empty_like(x)
    pkg.engine.dropout(x, a, rows, cols, p, 77, 1)
    pkg.engine.dropout(x, b, rows, cols, p, 77, 2)
    agree = ((a != 0) == (b != 0)).float().mean().item()
    want = p * p + (1 - p) * (1 - p)
    assert abs(agree - want) < 6 * math.sqrt(want * (1 - want) / (rows * cols)), (agree, want)
    pkg.engine.dropout(x, b, rows, cols, p, 78, 1)                  # another seed, same site
    assert abs(((a != 0) == (b != 0)).float().mean().item() - want) < 0.01


def test_dropout_argument_errors():
    pkg = load_pkg()
    N = pkg._native
    lib = N.lib()
    x = torch.zeros((8, 16), dtype=torch.float32, device=DEV)
    y = torch.zeros_like(x)
    px, py = x.data_ptr(), y.data_ptr()
    ok = (N.F32, px, 16, py, 16, 8, 16, 0.5, 1, 0, None)

    def call(**kw):
        names = ["dtype", "x", "ldx", "y", "ldy", "rows", "cols", "p", "seed", "site", "stream"]
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.mlpk_dropout(*[args[n] for n in names])

    assert call() == 0
    torch.cuda.synchronize()
    for kw in ({"p": -0.01}, {"p": 1.01}, {"p": float("nan")}, {"cols": 6, "ldx": 6, "ldy": 6}, {"ldx": 12}, {"ldy": 12}, {"rows": 0},
               {"x": None}, {"y": None}, {"dtype": 7}, {"y": px, "ldy": 20}):
        rc = call(**kw)
        assert rc < 0, (kw, rc)
    assert call(x=None) == -4 and call(dtype=7) == -1 and call(p=2.0) == -2


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_dropout_gradient_is_the_same_mask(dtype):
    load_pkg()
    AG = importlib.import_module("jittor-mlp_amd.autograd")
    rows, cols, p, seed, site = 300, 72, 0.35, 0xDEADBEEF12345, 5
    x = _nonzero(rows, cols, dtype, 11).requires_grad_(True)
    y = AG.Dropout.apply(x, p, seed, site)
    dy = _nonzero(rows, cols, dtype, 12)
    y.backward(dy)
    keep = P.keep_mask(seed, site, p, rows, cols)
    assert torch.equal(y.detach(), _expected(x.detach(), keep, p))
    assert torch.equal(x.grad, _expected(dy, keep, p))


# ---- the models against the reference's autograd -------------------------------------------------------------------------------------------------
CASES = [("swinmlp", "SwinMLP"), ("swinmlp_ape_dp", "SwinMLP"), ("asmlp_dp", "AS_MLP"), ("msmlp", "MS_MLP")]


def _model_case(pkg, tag, ctor):
    z = np.load(os.path.join(GOLDEN, "train_dropout_tiny.npz"))
    kw = json.loads(str(z[tag + "/kwargs"]))
    t = np.load(os.path.join(GOLDEN, str(z[tag + "/fixture"])))
    model = getattr(pkg.models_pytorch, ctor)(**kw)
    model.load_state_dict({k[3:]: torch.from_numpy(t[k]) for k in t.files if k.startswith("sd/")}, strict=True)
    model = model.to(DEV).train()
    seed = int(z[tag + "/seed"])
    seeds = []

    def fixed_seed():
        seeds.append(seed)
        return seed

    model.dropout_seed = fixed_seed
    if (tag + "/draws") in z.files:
        draws = [torch.from_numpy(d) for d in z[tag + "/draws"]]
        calls = []

        def recorded(B, dt, device):
            calls.append(B)
            return draws[len(calls) - 1].to(device)

        model.drop_path_uniform = recorded
    return z, model, seeds


@pytest.mark.parametrize("tag,ctor", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_mode_dropout_matches_reference_autograd(tag, ctor, dtype):
    pkg = load_pkg()
    z, model, seeds = _model_case(pkg, tag, ctor)
    x = torch.from_numpy(portable_input(tuple(z[tag + "/input_shape"]), seed=int(z[tag + "/input_seed"]))).to(DEV).to(dtype)
    G = torch.from_numpy(portable_input(tuple(z[tag + "/logits"].shape), seed=int(z[tag + "/input_seed"]) + 200)).to(DEV)
    logits = model(x)
    assert seeds == [int(z[tag + "/seed"])]                          # one seed per forward
    assert logits.requires_grad and logits.dtype == dtype
    ref = torch.from_numpy(z[tag + "/logits"])
    ftol = 2e-5 if dtype == torch.float32 else 3e-2
    ferr = (logits.float().cpu() - ref).abs().max().item()
    assert ferr < ftol * max(1.0, ref.abs().max().item()), (tag, str(dtype), ferr)
    (logits.float() * G).sum().backward()
    torch.cuda.synchronize()
    # the fixture keeps every entry of the small gradients and evenly spaced entries of the large ones, plus each gradient's max |g| and
    # L2 norm over all its entries (make_dropout_golden.py); the scale of a tensor's tolerance is its max |g|, floored as in test_gpu_train.py
    names = json.loads(str(z[tag + "/grad_names"]))
    params = dict(model.named_parameters())
    assert sorted(names) == sorted(params)
    kept, gmaxes, gnorms = z[tag + "/grad_kept"], z[tag + "/grad_max"], z[tag + "/grad_norm"]
    gmax = float(gmaxes.max())
    gtol = 2e-4 if dtype == torch.float32 else 6e-2
    worst, wname, off = 0.0, "", 0
    for i, k in enumerate(names):
        p = params[k]
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        g = p.grad.reshape(-1).cpu()
        idx = P.grad_sample_index(g.numel())
        want = torch.from_numpy(kept[off:off + len(idx)])
        off += len(idx)
        scale = max(float(gmaxes[i]), (1e-2 if dtype == torch.float32 else 5e-2) * gmax)
        rel = max((g[torch.from_numpy(idx)] - want).abs().max().item(), abs(g.abs().max().item() - float(gmaxes[i]))) / scale
        rel = max(rel, abs(g.double().norm().item() - float(gnorms[i])) / max(float(gnorms[i]), scale))
        if rel > worst:
            worst, wname = rel, k
        assert rel < gtol, (tag, str(dtype), k, rel)
    assert off == kept.size
    print("dropout %s %s: |logits - reference| %.3e, worst relative gradient error %.3e (%s) over %d parameters" % (
        tag, str(dtype)[6:], ferr, worst, wname, len(names)))


def _tiny_swin(pkg, **extra):
    t = np.load(os.path.join(GOLDEN, "tiny_swinmlp.npz"))
    kw = dict(json.loads(str(t["kwargs"])), **extra)
    model = pkg.models_pytorch.SwinMLP(**kw)
    model.load_state_dict({k[3:]: torch.from_numpy(t[k]) for k in t.files if k.startswith("sd/")}, strict=True)
    return model.to(DEV), torch.from_numpy(t["input"]).to(DEV)


def test_manual_seed_reproduces_and_no_grad_matches():
    pkg = load_pkg()
    model, x = _tiny_swin(pkg, drop_rate=0.25, drop_path_rate=0.0)
    model.train()
    torch.manual_seed(1234)
    a = model(x)
    torch.manual_seed(1234)
    b = model(x)
    c = model(x)                                                    # no reseed: another mask
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(1234)
    with torch.no_grad():
        d = model(x)                                                # train mode under no_grad takes the same path when a rate is > 0
    assert not d.requires_grad and torch.equal(d, a.detach())
    model.eval()
    with torch.no_grad():
        e = model(x)
    assert not torch.equal(e, d)
    # a mutated rate is honoured at the next forward (nn.Dropout reads .p when called); all rates 0 -> the dropout-free result
    model.train()
    model.pos_drop.p = 0.0
    for layer in model.layers:
        for blk in layer.blocks:
            blk.mlp.drop.p = 0.0
    torch.manual_seed(1234)
    f = model(x)
    ref, _ = _tiny_swin(pkg, drop_rate=0.0, drop_path_rate=0.0)
    g = ref.train()(x)
    assert torch.equal(f, g)


def test_swinmlp_t_training_step_with_dropout():
    """one bf16 training step of Swin-MLP-T at its benchmark configuration (bench.MODELS, 224 x 224, batch 4) with drop_rate 0.1"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    pkg = load_pkg()
    ctor, kw, _ = bench.MODELS["swinmlp_t"]
    torch.manual_seed(0)
    model = getattr(pkg.models_pytorch, ctor)(**dict(kw, drop_rate=0.1)).to(DEV).train()
    x = torch.rand(4, 3, 224, 224, device=DEV).bfloat16()
    out = model(x)
    assert out.requires_grad and out.shape == (4, 1000)
    (out.float() ** 2).mean().backward()
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), k


def test_unapplied_dropout_warns_once():
    pkg = load_pkg()
    t = np.load(os.path.join(GOLDEN, "tiny_resmlp.npz"))
    model = pkg.models_pytorch.ResMLPForImageClassification(**json.loads(str(t["kwargs"])))
    name, drop = next((n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout))
    model = model.to(DEV).train()
    x = torch.from_numpy(t["input"]).to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model(x)
    assert not [w for w in caught if "nn.Dropout" in str(w.message)]          # p = 0: nothing to say
    drop.p = 0.2
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model(x)
        model(x)
    hits = [w for w in caught if "nn.Dropout" in str(w.message)]
    assert len(hits) == 1 and issubclass(hits[0].category, RuntimeWarning) and name in str(hits[0].message), [str(w.message) for w in caught]
