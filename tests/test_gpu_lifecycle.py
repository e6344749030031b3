"""-m gpu: nothing leaks between forwards, images of a batch or weight updates.

Every other GPU test builds a model, loads weights once and runs it once or twice on one input.  The host layer keeps state between
calls -- packed weights per (dtype, device) behind `_param_stamp`, autograd._PACKS for the train path, up to four workspaces per model whose
buffers are zero-filled ONCE (the GEMM K-padding columns, the counters of mlpk_as_conv2_stats, the fill = 1 vectors of ViP / Sparse-MLP),
logits cloned out of a workspace buffer -- and these tests drive a long-lived ("warm") model through what a user does with one.

The oracle is a COLD model, bit for bit: a freshly constructed instance of the same class, loaded with `warm.state_dict()`, on the same
input, batch and dtype, compared with torch.equal.  The cold model is what test_tiny_golden, the real goldens and the train tests pin to
the reference; every kernel has a fixed summation order (test_tiny_golden asserts run-to-run equality), so zero difference is the gate and
no tolerance appears in this file.

Tables (tests/test_lifecycle_host.py): TINY = one tiny_*.npz configuration per family; EVAL_ONLY = the inference-only families on their own
fixtures' tiny configurations (WaveMLP-T, RaftMLP with either head, ActiveMLP): every update form but the optimizer steps; FUSED = the twelve benchmark
families at benchmark widths and reduced depth (the kwargs of train_grad_widths.npz, portable weights, 224 x 224): the table that reaches
the generated token kernel, as_conv2_stats with its counters, the fused channel MLP, swin_spatial_stats, the tiled mix-shift and the
vip_branch kernels, where the tiny models mostly take the fallback paths."""
import copy
import gc
import importlib
import io
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, load_pkg
from test_gpu_models import build_from_tiny
from test_lifecycle_host import (AT224, BN_FAMILIES, EVAL_ONLY, FUSED, TINY, VISIBLE_UPDATES, WAVE, adamw, config, noise_like, one_per_role, sgd,
                                 u_data_inplace_then_invalidate, u_no_grad_add)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TRAIN_FUSED = [t + AT224 for t in ("mixer_b16", "asmlp_t", "convmixer_1536_20")]


def run(m, x):
    with torch.no_grad():
        return m(x)


def warm_model(cfg, **kw):
    return cfg.fresh(**kw).to(DEV)


def cold_model(cfg, warm, **kw):
    """a freshly constructed instance with the warm model's state: never run, nothing cached"""
    m = cfg.fresh(sd={k: v.detach().cpu() for k, v in warm.state_dict().items()}, **kw).to(DEV)
    m.train(warm.training)
    m.set_compute_dtype(warm._compute_dtype)
    return m


def images(cfg, batch, dtype, seed=0):
    return cfg.images(batch, seed).to(DEV).to(dtype)


def gen(seed=3):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ 1. a weight update reaches the next forward
def train_step(model, x, opt=None, seed=50):
    """one train-mode forward + backward (+ optimizer step) on a fixed cotangent; returns the logits"""
    model.train()
    logits = model(x)
    G = torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(logits.shape)).astype(np.float32)).to(DEV)
    (logits.float() * G).sum().backward()
    if opt is not None:
        opt.step()
    return logits.detach()


def u_optimizer_step(opt_ctor):
    def u(m, g, x):
        train_step(m, x, opt_ctor([p for p in m.parameters()]))
        m.eval()
    u.__name__ = "u_train_backward_" + opt_ctor.__name__
    return u


def u_bn_train_forward(grad):
    def u(m, g, x):
        m.train()
        with torch.set_grad_enabled(grad):
            m(x)
        m.eval()
    u.__name__ = "u_bn_train_forward_" + ("grad" if grad else "no_grad")
    return u


def check_updates(name, dtype, batch=2):
    cfg = config(name)
    x = images(cfg, batch, dtype)
    forms = [(u, False) for u in VISIBLE_UPDATES + [u_data_inplace_then_invalidate]]
    if name not in EVAL_ONLY:
        forms += [(u_optimizer_step(sgd), True), (u_optimizer_step(adamw), True)]
    if name in BN_FAMILIES:                        # (under no_grad only ConvMixer's train mode runs on batch statistics; Sparse-MLP's takes the eval path)
        forms += [(u_bn_train_forward(True), True)] + ([(u_bn_train_forward(False), True)] if name.startswith("convmixer") else [])
    for upd, takes_x in forms:
        warm = warm_model(cfg, **(cfg.train_kw() if takes_x else {}))
        before = run(warm, x).clone()
        if takes_x:
            upd(warm, gen(), x)
        else:
            upd(warm, gen())
        assert not warm.training
        after = run(warm, x)
        want = run(cold_model(cfg, warm), x)
        assert torch.equal(after, want), (name, upd.__name__, "the warm model did not run on its updated state")
        assert not torch.equal(after, before), (name, upd.__name__, "the update was a no-op: the case checks nothing")
    # set_compute_dtype back and forth, with an update while the other dtype's pack is the one in use
    warm = warm_model(cfg)
    xf = images(cfg, batch, torch.float32)
    a1 = run(warm, xf).clone()
    b1 = run(warm.set_compute_dtype(torch.bfloat16), xf).clone()
    assert torch.equal(run(warm.set_compute_dtype(None), xf), a1) and torch.equal(run(warm.set_compute_dtype(torch.bfloat16), xf), b1)
    assert b1.dtype == torch.float32 and not torch.equal(a1, b1)
    u_no_grad_add(warm, gen())
    assert torch.equal(run(warm, xf), run(cold_model(cfg, warm), xf)), (name, "bf16 compute after an update")
    warm.set_compute_dtype(None)
    assert torch.equal(run(warm, xf), run(cold_model(cfg, warm), xf)), (name, "the fp32 pack made before the update was reused")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + EVAL_ONLY)
def test_weight_update_reaches_the_next_forward_tiny(name, dtype):
    """load_state_dict, no_grad add_, `p.data = t`, `mod.weight = nn.Parameter`, .half() / update / .float(), SGD and AdamW steps after a
    train-mode backward, a train-mode forward that moves BatchNorm's running statistics, set_compute_dtype back and forth, and a `.data`
    in-place write followed by invalidate_caches(): after each, warm(x) == cold(x), and != the output before the update."""
    check_updates(name, DT[dtype])


@pytest.mark.parametrize("name", FUSED)
def test_weight_update_reaches_the_next_forward_fused(name):
    check_updates(name, torch.bfloat16)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + EVAL_ONLY)
def test_every_parameter_role_reaches_the_next_forward(name, dtype):
    """one entry per role (the name with its digits stripped; no role skipped) perturbed at a time on ONE long-lived model: the stamp
    moves and warm == cold.  The folded ones are the likely misses: LayerNorm gamma / beta inside the next GEMM's weight, bias and csum,
    BatchNorm inside cscale / cshift, Swin's position table, permuted and regrouped weights.  No "output changed" per entry: a bias in
    front of a LayerNorm legitimately has no effect."""
    cfg = config(name)
    x = images(cfg, 2, DT[dtype])
    warm = warm_model(cfg)
    run(warm, x)
    g = gen(11)
    entries = warm.state_dict(keep_vars=True)
    roles = one_per_role(warm)
    assert len(roles) >= 4
    for r, key in roles.items():
        stamp = warm._param_stamp()
        with torch.no_grad():
            entries[key].add_(noise_like(entries[key], g, scale=0.05))
        assert warm._param_stamp() != stamp, (name, key)
        assert torch.equal(run(warm, x), run(cold_model(cfg, warm), x)), (name, dtype, key, "role %s is stale in the packed weights" % r)


# ------------------------------------------------------------------ 2. a forward leaves nothing behind
def hostile_inputs(cfg, batch, dtype):
    """legal inputs that leave the most behind: another image set, one all-NaN image in the batch, magnitudes at which fp16
    intermediates overflow (1e4 x N(0, 1): finite in every storage dtype, inf after the first product)"""
    x2 = images(cfg, batch, torch.float32, seed=7)
    xn = x2.clone()
    xn[batch // 2] = float("nan")
    return [x2.to(dtype), xn.to(dtype), (x2 * 1e4).to(dtype)]


def check_nothing_left_behind(name, dtype):
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="workspace buffer")       # a buffer re-allocated at another size: the workspace key missed something
        _check_nothing_left_behind(name, dtype)


def _check_nothing_left_behind(name, dtype):
    cfg = config(name)
    warm = warm_model(cfg)
    x1 = images(cfg, 2, dtype, seed=1)
    o1 = run(warm, x1).clone()
    for x in hostile_inputs(cfg, 2, dtype):
        run(warm, x)
    assert torch.equal(run(warm, x1), o1), (name, "a forward on other inputs changed what the model computes")
    first = {}
    for b in (2, 1, 3, 5, 4, 2):                   # six workspaces in one life: past the bound of four, so eviction and re-creation
        x = images(cfg, b, dtype, seed=b)
        out = run(warm, x).clone()
        assert torch.equal(out, run(cold_model(cfg, warm), x)), (name, "batch %d" % b)
        assert torch.equal(first.setdefault(b, out), out)
        assert len(warm._spaces) <= 4
        for xh in hostile_inputs(cfg, b, dtype)[1:]:
            run(warm, xh)
    assert torch.equal(run(warm, x1), o1)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", TINY + EVAL_ONLY)
def test_forward_leaves_nothing_behind_tiny(name, dtype):
    """o1 = m(x1); m(x2), m(one all-NaN image), m(1e4 x inputs); m(x1) == o1.  Then batches 2, 1, 3, 5, 4, 2 in one model's life, NaN and
    large inputs in between: each result equals the cold model at that batch."""
    check_nothing_left_behind(name, DT[dtype])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", FUSED)
def test_forward_leaves_nothing_behind_fused(name, dtype):
    check_nothing_left_behind(name, DT[dtype])


@pytest.mark.parametrize("name", TINY + EVAL_ONLY + FUSED)
def test_dtype_round_trip_on_one_model(name):
    """fp32 -> bf16 -> fp16 -> fp32 inputs on one model: every leg equals the cold model in that dtype, the last the first"""
    cfg = config(name)
    warm = warm_model(cfg)
    x = images(cfg, 3, torch.float32, seed=2)
    outs = []
    for dt in ("fp32", "bf16", "fp16", "fp32"):
        out = run(warm, x.to(DT[dt])).clone()
        assert out.dtype == DT[dt]
        assert torch.equal(out, run(cold_model(cfg, warm), x.to(DT[dt]))), (name, dt)
        outs.append(out)
    assert torch.equal(outs[0], outs[3])


# ------------------------------------------------------------------ 3. images of a batch do not see each other
def check_rows_do_not_see_each_other(name, dtype, B=4):
    cfg = config(name)
    m = warm_model(cfg)
    base = images(cfg, B, torch.float32, seed=4)
    other = images(cfg, 1, torch.float32, seed=5)[0]
    for j in (0, B - 1, B // 2):
        xa, xb = base.clone(), base.clone()
        xa[j] = float("nan")
        xb[j] = other
        oa, ob = run(m, xa.to(dtype)).clone(), run(m, xb.to(dtype)).clone()
        rows = [b for b in range(B) if b != j]
        assert torch.isfinite(oa[rows].float()).all(), (name, j, "a NaN image reached another image's logits")
        assert torch.equal(oa[rows], ob[rows]), (name, j, "the logits of an image depend on another image of its batch")
        assert torch.isfinite(ob.float()).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + EVAL_ONLY)
def test_images_of_a_batch_do_not_see_each_other_tiny(name, dtype):
    """batch X with an all-NaN image at position j (first, last, middle), batch X' with a finite image there, the same batch size: every
    other row is finite and bit-equal -- stat_group, per-sample GroupNorm statistics, SplitAttention's per-image sums and the by-product
    statistics planes index the right rows"""
    check_rows_do_not_see_each_other(name, DT[dtype])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", FUSED)
def test_images_of_a_batch_do_not_see_each_other_fused(name, dtype):
    check_rows_do_not_see_each_other(name, DT[dtype])


# ------------------------------------------------------------------ 4. results and inputs are the caller's
def mp():
    return load_pkg().models_pytorch


def sub(name):
    return importlib.import_module(load_pkg().__name__ + ".models_pytorch." + name)


def randomize(model, seed):
    """non-trivial norms, biases and running statistics (a fresh constructor leaves gamma = 1, beta = 0)"""
    g = gen(seed)
    with torch.no_grad():
        for t in model.state_dict(keep_vars=True).values():
            t.add_(noise_like(t, g, scale=0.05))
    return model.eval()


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=gen(100 + seed))


def _mixer():
    return randomize(mp().MLPMixer(num_patches=49, d_model=64, depth=2, expansion_factor=2), 1)


def _cycle():
    return randomize(mp().CycleNet([1, 1], img_size=32, embed_dims=[16, 32], transitions=[True, True], mlp_ratios=[2, 2], num_classes=10,
                                   mlp_fn=mp().cycle_mlp.CycleMLP), 2)


def _asmlp():
    return randomize(mp().AS_MLP(img_size=32, patch_size=4, embed_dim=64, depths=[1, 2], shift_size=5, num_classes=10), 3)


def _swin():
    return randomize(mp().SwinMLP(img_size=32, patch_size=4, embed_dim=32, depths=[2, 2], num_heads=[2, 4], window_size=4, num_classes=10), 4)


def _msmlp():
    return randomize(mp().MS_MLP(img_size=32, patch_size=4, embed_dim=40, depths=[2, 1], shift_size=5, num_classes=10), 5)


def _s2(ver):
    ctor = mp().S2MLPv2 if ver == 2 else mp().S2MLPv1
    return randomize(ctor(image_size=32, patch_size=[4, 2], d_model=[32, 64], depth=[2, 1], expansion_factor=[2, 2], num_classes=10), 6)


def _tiny(name):
    return config(name).fresh()


def _geom(stage):
    return stage.geom[:3]


def _channel_mlp(width, hid):
    return nn.Sequential(nn.Linear(width, hid), nn.GELU(), nn.Dropout(0.), nn.Linear(hid, width), nn.Dropout(0.))


def _first(model, cls):
    return [m for m in model.modules() if type(m) is cls][0]


class WithOffset(nn.Module):
    """ATMLayer as a one-argument callable: the offsets are a fixed tensor"""

    def __init__(self, layer, offset):
        super().__init__()
        self.layer = layer
        self.register_buffer("offset", offset)

    def forward(self, x):
        return self.layer(x, self.offset.to(x.dtype))


def _atm(B, H, W, C):
    """ATMLayer(C) on x (B, H, W, C) with offsets (B, 2C, H, W) uniform in [-3, 3)"""
    layer = randomize(sub("active_mlp").ATMLayer(C), 30)
    return WithOffset(layer, torch.rand((B, 2 * C, H, W), generator=gen(130)) * 6.0 - 3.0)


# label -> () -> (root module to move to the GPU, the module to call, its input).  The shapes are those of the
# test_*callable_like_the_reference tests of test_gpu_models.py.
STANDALONE = {
    "mixer.backbone": lambda: (lambda m: (m, m, rnd(3, 49, 64)))(_mixer()),
    "mixer.block": lambda: (lambda m: (m, m.model[0], rnd(3, 49, 64)))(_mixer()),
    "mixer.token_prenorm": lambda: (lambda m: (m, m.model[0][0], rnd(3, 49, 64)))(_mixer()),
    "mixer.channel_prenorm": lambda: (lambda m: (m, m.model[0][1], rnd(3, 49, 64)))(_mixer()),
    "mixer.token_ff": lambda: (lambda m: (m, m.model[0][0].fn, rnd(3, 49, 64)))(_mixer()),
    "mixer.channel_ff": lambda: (lambda m: (m, m.model[0][1].fn, rnd(3, 49, 64)))(_mixer()),
    "gmlp.backbone": lambda: (lambda m: (m, m, rnd(3, 16, 32)))(randomize(mp().gMLP(d_model=32, d_ffn=64, seq_len=16, depth=2), 7)),
    "gmlp.block": lambda: (lambda m: (m, m.model[1], rnd(3, 16, 32)))(randomize(mp().gMLP(d_model=32, d_ffn=64, seq_len=16, depth=2), 7)),
    "gmlp.block_in_classifier": lambda: (lambda m: (m, m.model[0], rnd(3, 16, 32)))(_tiny("gmlp")),
    "gmlp.sgu": lambda: (lambda m: (m, m, rnd(3, 10, 48)))(randomize(sub("g_mlp").SpatialGatingUnit(24, 10), 8)),
    "resmlp.backbone": lambda: (lambda m: (m, m, rnd(3, 16, 32)))(randomize(mp().ResMLP(16, 32, 2, 2), 9)),
    "resmlp.block": lambda: (lambda m: (m, m.model[1], rnd(3, 16, 32)))(randomize(mp().ResMLP(16, 32, 2, 2), 9)),
    "resmlp.aff": lambda: (lambda m: (m, m, rnd(3, 5, 32)))(randomize(sub("res_mlp").Aff(32), 10)),
    "resmlp.ff": lambda: (lambda m: (m, m, rnd(3, 5, 32)))(randomize(sub("res_mlp").FeedForward(32, 80), 11)),
    "cycle.block": lambda: (lambda m: (m, m.network[0][0], rnd(2, 8, 6, 16)))(_cycle()),
    "cycle.stage": lambda: (lambda m: (m, m.network[2], rnd(2, 4, 5, 32)))(_cycle()),
    "cycle.patch_embed": lambda: (lambda m: (m, m.patch_embed, rnd(2, 3, 30, 26)))(_cycle()),
    "cycle.downsample": lambda: (lambda m: (m, m.network[1], rnd(2, 7, 6, 16)))(_cycle()),
    "cycle.mlp": lambda: (lambda m: (m, m.network[0][0].mlp, rnd(2, 7, 16)))(_cycle()),
    "asmlp.block": lambda: (lambda m: (m, m.layers[1].blocks[1], rnd(2, 128, 4, 4)))(_asmlp()),
    "asmlp.patch_embed": lambda: (lambda m: (m, m.patch_embed, rnd(2, 3, 32, 32)))(_asmlp()),
    "asmlp.downsample": lambda: (lambda m: (m, m.layers[0].downsample, rnd(2, 64, 8, 8)))(_asmlp()),
    "asmlp.stage": lambda: (lambda m: (m, m.layers[0], rnd(2, 64, 8, 8)))(_asmlp()),
    "asmlp.axial_shift": lambda: (lambda m: (m, m, rnd(2, 32, 7, 6)))(randomize(sub("as_mlp").AxialShift(32, 5), 12)),
    "asmlp.mlp": lambda: (lambda m: (m, m, rnd(2, 32, 7, 6)))(randomize(sub("as_mlp").Mlp(32, 64), 13)),
    "swin.block": lambda: (lambda m: (m, m.layers[0].blocks[1], rnd(2, 64, 32)))(_swin()),
    "swin.patch_embed": lambda: (lambda m: (m, m.patch_embed, rnd(2, 3, 32, 32)))(_swin()),
    "swin.downsample": lambda: (lambda m: (m, m.layers[0].downsample, rnd(2, 64, 32)))(_swin()),
    "swin.stage": lambda: (lambda m: (m, m.layers[0], rnd(2, 64, 32)))(_swin()),
    "swin.mlp": lambda: (lambda m: (m, m.layers[0].blocks[0].mlp, rnd(2, 7, 32)))(_swin()),
    "msmlp.block": lambda: (lambda m: (m, m.layers[0].blocks[1], rnd(2, 40, 8, 8)))(_msmlp()),
    "msmlp.patch_embed": lambda: (lambda m: (m, m.patch_embed, rnd(2, 3, 32, 32)))(_msmlp()),
    "msmlp.downsample": lambda: (lambda m: (m, m.layers[0].downsample, rnd(2, 40, 8, 8)))(_msmlp()),
    "msmlp.stage": lambda: (lambda m: (m, m.layers[0], rnd(2, 40, 8, 8)))(_msmlp()),
    "msmlp.norm_last": lambda: (lambda m: (m, m.norm, rnd(3, 5, 80)))(_msmlp()),
    "msmlp.norm_first": lambda: (lambda m: (m, m, rnd(2, 24, 3, 5)))(randomize(sub("ms_mlp").LayerNorm(24, data_format="channels_first"), 14)),
    "vip.weighted_backbone": lambda: (lambda m: (m, m, rnd(2, 4, 6, 32)))(randomize(mp().WeightedPermutator(4, 6, 32, 2, 8, expansion_factor=2), 15)),
    "vip.backbone": lambda: (lambda m: (m, m, rnd(2, 4, 6, 32)))(randomize(mp().Permutator(4, 6, 32, 2, 8, expansion_factor=2), 16)),
    "vip.block": lambda: (lambda m: (m, m.model[1], rnd(2, 4, 6, 32)))(randomize(mp().WeightedPermutator(4, 6, 32, 2, 8, expansion_factor=2), 15)),
    "vip.prenorm": lambda: (lambda m: (m, m, rnd(2, 5, 7, 256)))(randomize(sub("vip").PreNormResidual(256, _channel_mlp(256, 512)), 17)),
    "vip.split_attention": lambda: (lambda m: (m, m, rnd(2, 3, 4, 5, 32)))(randomize(sub("vip").SplitAttention(32), 18)),
    "vip.parallel_weighted_sum": lambda: (lambda m: (m, _first(m, sub("vip").ParallelWeightedSum), rnd(2, 4, 4, 32)))(
        randomize(mp().ViP(image_size=32, patch_size=8, d_model=32, depth=1, segments=4, expansion_factor=2), 19)),
    "s2v2.block": lambda: (lambda m: (m, m.stages[0][1].model[1], rnd(2, 8, 8, 32)))(_s2(2)),
    "s2v2.stage_in_model": lambda: (lambda m: (m, m.stages[1][1], rnd(2, 64, 4, 4)))(_s2(2)),
    "s2v2.stage": lambda: (lambda m: (m, m, rnd(2, 32, 6, 5)))(randomize(sub("s2_mlp_v2").S2Block(32, 2, expansion_factor=3), 20)),
    "s2v2.prenorm_mlp": lambda: (lambda m: (m, m, rnd(2, 5, 7, 96)))(randomize(sub("s2_mlp_v2").PreNormResidual(96, _channel_mlp(96, 384)), 21)),
    "s2v2.prenorm_attention": lambda: (lambda m: (m, m, rnd(2, 6, 5, 32)))(
        randomize(sub("s2_mlp_v2").PreNormResidual(32, sub("s2_mlp_v2").S2Attention(32)), 22)),
    "s2v2.attention": lambda: (lambda m: (m, m, rnd(2, 6, 5, 32)))(randomize(sub("s2_mlp_v2").S2Attention(32), 23)),
    "s2v2.split_attention": lambda: (lambda m: (m, m, rnd(2, 3, 4, 5, 32)))(randomize(sub("s2_mlp_v2").SplitAttention(32), 24)),
    "s2v1.block": lambda: (lambda m: (m, m.stages[0][1].model[1], rnd(2, 8, 8, 32)))(_s2(1)),
    "s2v1.stage": lambda: (lambda m: (m, m, rnd(2, 32, 6, 5)))(randomize(sub("s2_mlp_v1").S2Block(32, 2, expansion_factor=3), 25)),
    "s2v1.prenorm_mlp": lambda: (lambda m: (m, m, rnd(2, 5, 7, 64)))(randomize(sub("s2_mlp_v1").PreNormResidual(64, _channel_mlp(64, 200)), 26)),
    "convmixer.block": lambda: (lambda m: (m, m.blocks[1], rnd(2, 32, 8, 8)))(
        randomize(mp().ConvMixer(32, 2, kernel_size=5, patch_size=4, n_classes=10), 27)),
    "hire.block": lambda: (lambda m: (m, m.layers[0].model[1], rnd(2, 7, 9, _geom(m.layers[0])[2])))(_tiny("hiremlp")),
    "hire.stage": lambda: (lambda m: (m, m.layers[0], rnd(2, 7, 9, _geom(m.layers[0])[2])))(_tiny("hiremlp")),
    "hire.patcher": lambda: (lambda m: (m, m.patcher, rnd(2, 3, 36, 28)))(_tiny("hiremlp")),
    "hire.patch_merge": lambda: (lambda m: (m, m.layers[0].patch_merge[1], rnd(2, _geom(m.layers[0])[2], 7, 9)))(_tiny("hiremlp")),
    "hire.ff": lambda: (lambda m: (m, m.layers[0].model[0][0].fn[0].proj_w, rnd(2, m.layers[0].model[0][0].fn[0].proj_w.net[0].in_channels, 5, 3)))(
        _tiny("hiremlp")),
    "sparse.block": lambda: (lambda m: (m, m.layers[1].model[1], rnd(2, _geom(m.layers[1])[2], *_geom(m.layers[1])[:2])))(_tiny("sparsemlp")),
    "sparse.stage": lambda: (lambda m: (m, m.layers[0], rnd(2, _geom(m.layers[0])[2], *_geom(m.layers[0])[:2])))(_tiny("sparsemlp")),
    "sparse.patch_merge": lambda: (lambda m: (m, m.layers[0].patch_merge[1], rnd(2, *_geom(m.layers[0])[:3])))(_tiny("sparsemlp")),
    "wave.block": lambda: (lambda m: (m, m.network[0][0], rnd(2, 64, 16, 12)))(_tiny(WAVE)),
    "wave.patm": lambda: (lambda m: (m, m.network[0][0].attn, rnd(2, 64, 16, 12)))(_tiny(WAVE)),
    # the shapes of `blocks` / `block_inputs` in tests/golden/raft_mlp.npz and of `blocks` in active_mlp.npz
    "raft.permuted": lambda: (lambda m: (m, m, rnd(2, 108, 14)))(randomize(sub("raft_mlp").PermutedBlock(7, 24, 2), 28)),
    "raft.separated": lambda: (lambda m: (m, m, rnd(2, 216, 7)))(randomize(sub("raft_mlp").SpatiallySeparatedTokenBlock(7, 24), 29)),
    "raft.channel": lambda: (lambda m: (m, m, rnd(2, 9, 24)))(randomize(sub("raft_mlp").ChannelBlock(24), 31)),
    "active.atm": lambda: (lambda m: (m, m, rnd(3, 5, 7, 16)))(_atm(3, 5, 7, 16)),
}
# the leaf modules of tests/golden/leaf_modules.npz (Hire-MLP's PreNormResidual halves and HireMLPBlock, Sparse-MLP's thirds and sMLPBlock,
# ConvMixer's Residual, ViP's ParallelSum), on the inputs the reference fed them
LEAF_TAGS = ["hiremlp", "sparsemlp", "convmixer", "vip_unweighted"]
# EngineModule subclasses that are bases only: never instantiated by a constructor of the package
BASES = {"EngineModule", "SubModule", "_SubModule", "PreNormResidualMLP", "LinearMlp", "_PermutatorBase",
         "raft_mlp.Block", "raft_mlp._RaftBlock"}                  # (with its module where another family has a concrete class of that name)
# EngineModule subclasses that constructors do instantiate, but only to hold parameters: calling one raises NotImplementedError
HOLDERS = {"raft_mlp.TokenBlock": lambda: (sub("raft_mlp").TokenBlock(5, 12), rnd(2, 12, 5))}


def engine_spaces(*mods):
    """every Workspace of the given modules, of the EngineModules below them and of the backbones that run them"""
    E = load_pkg().engine
    seen, out, stack = set(), [], list(mods)
    while stack:
        m = stack.pop()
        if id(m) in seen:
            continue
        seen.add(id(m))
        if isinstance(m, E.EngineModule):
            out.extend(m._spaces.values())
        if "_owner" in m.__dict__:
            stack.append(m.__dict__["_owner"][0])
        stack.extend(c for c in m._modules.values() if c is not None)
    return out


def span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def check_callers_own(root, mod, x):
    """the four properties of item 4 for one callable on one contiguous input (batch >= 2)"""
    assert x.is_contiguous() and x.shape[0] >= 2
    x0 = x.clone()
    o1 = run(mod, x)
    keep = o1.clone()
    assert torch.equal(x, x0), "the input tensor was written"
    run(mod, x * 0.5 + 0.25)
    run(mod, -x)
    assert torch.equal(o1, keep), "a later forward changed an earlier result"
    lo, hi = span(o1)
    spaces = engine_spaces(root, mod)
    for ws in spaces:
        for k, t in ws.t.items():
            if torch.is_tensor(t):
                a, b = span(t)
                assert b <= lo or hi <= a, "the result shares storage with workspace buffer %r" % (k,)
    assert torch.equal(run(mod, x), keep)
    # a strided batch slice: every second image of a batch whose other images are NaN
    big = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype, device=x.device)
    big[::2] = x
    xs = big[::2]
    assert not xs.is_contiguous()
    assert torch.equal(run(mod, xs), keep), "a strided batch slice does not give the bits of its contiguous copy"
    assert torch.equal(xs, x0)
    if x.dim() == 4:
        xc = x.contiguous(memory_format=torch.channels_last)
        if not xc.is_contiguous():
            assert torch.equal(run(mod, xc), keep), "a channels_last input does not give the bits of its contiguous copy"
            assert torch.equal(xc, x0)
    return len(spaces)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + EVAL_ONLY + [t + AT224 for t in ("mixer_b16", "asmlp_t", "vip_s7")])
def test_results_and_inputs_are_the_callers_full_models(name, dtype):
    """o1 unchanged by later forwards and disjoint from every workspace buffer; the input bit-identical after the call; a strided batch
    slice and a channels_last image batch give the bits of their contiguous copies"""
    cfg = config(name)
    m = warm_model(cfg)
    assert check_callers_own(m, m, images(cfg, 3, DT[dtype], seed=6)) >= 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("label", sorted(STANDALONE))
def test_results_and_inputs_are_the_callers_standalone_modules(label, dtype):
    """the same for every block and inner module that test_gpu_models.py calls "callable like the reference" """
    root, mod, x = STANDALONE[label]()
    root.to(DEV)
    check_callers_own(root, mod, x.to(DEV).to(DT[dtype]))


@pytest.mark.parametrize("tag", LEAF_TAGS)
def test_results_and_inputs_are_the_callers_leaf_modules(tag):
    z = np.load(os.path.join(GOLDEN, "leaf_modules.npz"))
    model = build_from_tiny(load_pkg(), tag)[0].to(DEV)
    mods = dict(model.named_modules())
    paths = json.loads(str(z[tag + "/paths"]))
    assert paths
    for pth in paths:
        xin = torch.from_numpy(z["%s/%s/in" % (tag, pth)])
        check_callers_own(model, mods[pth], xin.to(DEV))


def test_every_engine_module_class_is_in_the_standalone_table():
    """a new EngineModule subclass cannot arrive uncovered: every concrete one defined under models_pytorch is called directly by a row of
    the tables above"""
    pkg = load_pkg()
    E = pkg.engine
    prefix = pkg.__name__ + ".models_pytorch"
    defined = set()
    for name, module in list(sys.modules.items()):
        if name.startswith(prefix) and module is not None:
            for obj in vars(module).values():
                if isinstance(obj, type) and issubclass(obj, E.EngineModule) and obj.__module__.startswith(prefix):
                    defined.add(obj)
    assert len(defined) > 30
    called = {type(config(n).fresh()) for n in TINY + EVAL_ONLY}
    for label in STANDALONE:
        mod = STANDALONE[label]()[1]
        called.add(type(mod.layer if isinstance(mod, WithOffset) else mod))
    labels = {c: c.__module__.rsplit(".", 1)[1] + "." + c.__name__ for c in defined}
    for label, make in HOLDERS.items():                            # on the CPU: nothing is launched
        holder, x = make()
        assert labels.get(type(holder)) == label
        with pytest.raises(NotImplementedError):
            holder(x)
    missing = sorted(labels[c] for c in defined - called if c.__name__ not in BASES and labels[c] not in BASES | set(HOLDERS))
    assert not missing, "EngineModule subclasses without a row in test_gpu_lifecycle.STANDALONE: %s" % missing


# ------------------------------------------------------------------ 5. the train path
def grads(model):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}


def grad_mismatches(a, b):
    """the parameters whose gradients are not bit-equal"""
    assert a.keys() == b.keys()
    return [k for k in a if (a[k] is None) != (b[k] is None) or (a[k] is not None and not torch.equal(a[k], b[k]))]


def check_train_steps(name, dtype):
    cfg = config(name)
    kw = cfg.train_kw()
    x1, x2 = images(cfg, 3, dtype, seed=8), images(cfg, 3, dtype, seed=9)
    # eval -> train step without an optimizer -> eval
    warm = warm_model(cfg, **kw)
    e1 = run(warm, x1).clone()
    train_step(warm, x1)
    warm.eval()
    e2 = run(warm, x1)
    assert torch.equal(e2, run(cold_model(cfg, warm, **kw), x1)), (name, "eval after a train step")
    if name not in BN_FAMILIES:
        assert torch.equal(e2, e1), (name, "a train step without an optimizer changed the eval output")
    # two SGD steps: step 2 of the warm model == that step on a cold model loaded with the state after step 1
    opt = torch.optim.SGD([p for p in warm.parameters()], lr=0.05)
    opt.zero_grad(set_to_none=True)
    train_step(warm, x1, opt, seed=51)
    cold = cold_model(cfg, warm, **kw)
    opt.zero_grad(set_to_none=True)
    l2 = train_step(warm, x2, seed=52)
    l2c = train_step(cold, x2, seed=52)
    assert torch.equal(l2, l2c), (name, "logits of the second step")
    assert not grad_mismatches(grads(warm), grads(cold)), (name, "gradients of the second step", grad_mismatches(grads(warm), grads(cold))[:6])
    assert all(torch.equal(a, b) for a, b in zip(warm.state_dict().values(), cold.state_dict().values())), (name, "running statistics")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + TRAIN_FUSED)
def test_train_steps_on_a_warm_model_equal_a_cold_one(name, dtype):
    """drop rates 0.  eval -> train step without an optimizer -> eval: the last eval equals the cold model (and the first, without
    BatchNorm).  Then two SGD steps: logits, every .grad and the buffers of step 2 equal a cold model's that starts from the state after
    step 1 -- autograd._PACKS must have followed the optimizer's in-place update."""
    check_train_steps(name, DT[dtype])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY + TRAIN_FUSED)
def test_train_packs_survive_address_reuse(name, dtype):
    """a model is deleted and a second one of the same shapes built: the allocator hands the freed parameters' addresses -- with version
    0 again -- to the new parameters (the case autograd._packed's comment describes).  Its train step equals the same step with _PACKS
    cleared."""
    AG = importlib.import_module(load_pkg().__name__ + ".autograd")
    cfg = config(name)
    kw = cfg.train_kw()
    x = images(cfg, 2, DT[dtype], seed=10)
    first = warm_model(cfg, **kw)
    train_step(first, x)
    ptrs = {p.data_ptr() for p in first.parameters()}
    sd2 = {k: v + noise_like(v, gen(13)) for k, v in cfg.sd.items()}
    del first
    gc.collect()
    second = cfg.fresh(sd=sd2, **kw).to(DEV)
    reused = sum(p.data_ptr() in ptrs for p in second.parameters())
    l_second = train_step(second, x)
    AG._PACKS.clear()
    clean = cfg.fresh(sd=sd2, **kw).to(DEV)
    l_clean = train_step(clean, x)
    print("address reuse %s: %d of %d parameters took a freed address" % (name, reused, len(ptrs)))
    assert torch.equal(l_second, l_clean), (name, "the second model ran on the first one's packed weights")
    assert not grad_mismatches(grads(second), grads(clean))


@pytest.mark.parametrize("name", TINY + TRAIN_FUSED)
def test_two_backwards_without_zero_grad_give_twice_the_gradient(name):
    """fp32: .grad accumulates; g + g is exact, so the sum of two identical backwards is exactly 2 g"""
    cfg = config(name)
    m = warm_model(cfg, **cfg.train_kw())
    x = images(cfg, 2, torch.float32, seed=12)
    train_step(m, x)
    g1 = grads(m)
    train_step(m, x)
    g2 = grads(m)
    assert any(v is not None for v in g1.values())
    bad = [k for k in g1 if g1[k] is not None and not torch.equal(g2[k], 2 * g1[k])]
    assert not bad, (name, bad[:6])


# ------------------------------------------------------------------ 6. two streams
@pytest.mark.parametrize("name,dtype", [("mixer", "bf16"), ("hiremlp", "bf16"), ("swinmlp_ape", "fp32"), ("mixer_b16" + AT224, "bf16"),
                                        ("asmlp_t" + AT224, "bf16"), ("vip_s7" + AT224, "bf16"), ("raftmlp", "bf16"), ("activemlp", "bf16")])
def test_two_streams_give_the_serial_results_and_see_a_weight_update(name, dtype):
    """InFlight(model, 2) on alternating different inputs: each result equals the serial one; after synchronize() a load_state_dict is
    seen by both slots (each stream has its own workspace, the packed weights are shared)"""
    parallel = importlib.import_module(load_pkg().__name__ + ".parallel")
    E = load_pkg().engine
    cfg = config(name)
    m = warm_model(cfg)
    xs = [images(cfg, 2, DT[dtype], seed=20 + i) for i in range(2)] * 2 + [images(cfg, 2, DT[dtype], seed=25)]
    serial = [run(m, x).clone() for x in xs]
    plan, side = E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS
    slots = parallel.InFlight(lambda t: run(m, t), 2, device=DEV)
    try:
        got = [slots(x) for x in xs]
        slots.synchronize()
        assert len({id(s) for _, s in got}) == 2
        for (out, _), want in zip(got, serial):
            assert torch.equal(out, want)
        m.load_state_dict({k: v + noise_like(v, gen(14)) for k, v in m.state_dict().items()})
        got = [slots(x) for x in xs[:2]]
        slots.synchronize()
        cold = cold_model(cfg, m)
        for (out, _), x, old in zip(got, xs, serial):
            assert torch.equal(out, run(cold, x)) and not torch.equal(out, old)
    finally:
        slots.synchronize()
        slots.restore_plan()
    assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (plan, side)


# ------------------------------------------------------------------ 7. copies
@pytest.mark.parametrize("name,dtype", [("hiremlp", "fp32"), ("hiremlp", "bf16"), ("mixer", "fp32"), ("mixer", "bf16"), ("hiremlp_s" + AT224, "bf16"),
                                        ("mixer_b16" + AT224, "bf16"), ("raftmlp", "bf16"), ("activemlp", "bf16")])
def test_deepcopy_and_pickle_of_a_warm_model(name, dtype):
    """copy.deepcopy and torch.save / torch.load (through BytesIO) of a model that has run (Hire-MLP's workspace holds torch.cuda.Events):
    both work, give the warm model's bits, carry no cache, and an update of one copy leaves the other models untouched"""
    E = load_pkg().engine
    cfg = config(name)
    warm = warm_model(cfg)
    x = images(cfg, 2, DT[dtype], seed=15)
    o1 = run(warm, x).clone()
    buf = io.BytesIO()
    torch.save(warm, buf)
    buf.seek(0)
    copies = [copy.deepcopy(warm), torch.load(buf, weights_only=False)]
    for c in copies:
        assert all(not e._packs and not e._spaces for e in c.modules() if isinstance(e, E.EngineModule))
        assert torch.equal(run(c, x), o1)
    assert warm._packs and warm._spaces
    u_no_grad_add(copies[0], gen(16))
    o2 = run(copies[0], x)
    assert torch.equal(o2, run(cold_model(cfg, copies[0]), x)) and not torch.equal(o2, o1)
    assert torch.equal(run(copies[1], x), o1) and torch.equal(run(warm, x), o1)
