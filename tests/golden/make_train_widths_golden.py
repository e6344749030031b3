#!/usr/bin/env python3
"""Generate tests/golden/train_grad_widths.npz: the REFERENCE's own train-mode autograd for every benchmarked family at its bench.MODELS
widths (heads, segments, kernel and patch sizes, 224 x 224 input), at the smallest depth that keeps every distinct block variant of every
stage: two blocks where the blocks of a stage differ or chain (Mixer, gMLP, ResMLP, ConvMixer; Swin-MLP's shifted block; Hire-MLP's two
cross-region variants), one per stage elsewhere.  Every drop rate is 0 (stochastic depth and Dropout have fixtures of their own).

Runs ONLY in the authoring container (needs the reference; the shim is make_golden.load_reference); never on the GPU box.

Per case: weights from oracle.portable_init.portable_state_dict(seed), a batch of 4 = portable_input((4, 3, 224, 224), seed) and the logits'
cotangent G = portable_input((4, 1000), seed + 200) (the test regenerates all three from the seed), train(), then
  * the reference in fp64 (.double()): the logits, the gradient of sum(logits * G) w.r.t. every parameter and the running statistics after
    the step, each as tests/grad_digest.py keeps a tensor (64 evenly spaced entries, max |g|, L2 norm, 8 seeded projections); the parameters
    that get no gradient;
  * the reference in bf16 on the CPU, where it runs: per parameter its own error against fp64 (L2 norm, and max over the kept entries) --
    the test's bf16 gates are multiples of these.  CycleMLP's torchvision stand-in cannot run in 16 bit (it builds the sampling
    grid in the input dtype): `lowp` records that, and the test takes ViP's numbers (the same three-branch + reweighting structure).

Usage:  python tests/golden/make_train_widths_golden.py [--check]   (--check: regenerate in memory, compare bit for bit with the file)
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import grad_digest as D  # noqa: E402
from make_golden import _jsonable, ctor_kw, load_reference  # noqa: E402
from oracle.portable_init import portable_input, portable_state_dict  # noqa: E402

OUT = os.path.join(HERE, "train_grad_widths.npz")
T4 = [True] * 4
# tag (= bench.MODELS name), reference module, reference class (= the package's ctor name), kwargs, seed
CASES = (("mixer_b16", "mlp_mixer", "MLPMixerForImageClassification", dict(d_model=768, depth=2, patch_size=16, image_size=224), 71),
         ("gmlp_s", "g_mlp", "gMLPForImageClassification", dict(image_size=224, depth=2), 72),
         ("resmlp_24", "res_mlp", "ResMLPForImageClassification", dict(depth=2), 73),
         ("vip_s7", "vip", "ViP", dict(image_size=224, patch_size=7, d_model=384, depth=1, segments=12, expansion_factor=3), 74),
         ("s2mlpv2", "s2_mlp_v2", "S2MLPv2", dict(depth=[1, 1]), 75),
         ("asmlp_t", "as_mlp", "AS_MLP", dict(depths=[1, 1, 1, 1], drop_path_rate=0.0), 76),
         ("convmixer_1536_20", "conv_mixer", "ConvMixer", dict(dim=1536, depth=2), 77),
         ("sparsemlp_t", "sparse_mlp", "SparseMLP", dict(depth=[1, 1, 1, 1]), 78),
         ("hiremlp_s", "hire_mlp", "HireMLP", dict(depth=[2, 2, 2, 2]), 79),
         ("msmlp_t", "ms_mlp", "MS_MLP", dict(depths=[1, 1, 1, 1], drop_path_rate=0.0), 80),
         ("swinmlp_t", "swin_mlp", "SwinMLP", dict(depths=[2, 2, 2, 2], drop_path_rate=0.0), 81),
         ("cyclemlp_b1", "cycle_mlp", "CycleNet", dict(layers=[1, 1, 1, 1], embed_dims=[64, 128, 320, 512], patch_size=7, transitions=T4,
                                                       mlp_ratios=[4, 4, 4, 4], drop_path_rate=0.0), 82))
BATCH = 4


def run(model, x, G, dtype):
    model = model.to(dtype).train()
    for p_ in model.parameters():
        p_.grad = None
    logits = model(x.to(dtype))
    (logits.double() * G.double()).sum().backward()
    grads = {k: (None if p_.grad is None else p_.grad.double().numpy().reshape(-1)) for k, p_ in model.named_parameters()}
    return logits.detach().double().numpy(), grads, model


def make_case(ref, tag, mod, cls, kw, seed):
    out = {}
    ctor = getattr(ref[mod], cls)
    model = ctor(**ctor_kw(ref, kw))
    sd = portable_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = torch.from_numpy(portable_input((BATCH, 3, 224, 224), seed=seed))
    G = torch.from_numpy(portable_input((BATCH, 1000), seed=seed + 200))
    torch.set_num_threads(1 if tag.startswith("s2") else 8)          # (S2-MLP's in-place shift is only deterministic on one thread)
    logits, g64, m64 = run(model, x, G, torch.float64)
    out[tag + "/kwargs"] = np.array(_jsonable(kw))
    out[tag + "/ctor"] = np.array(cls)
    out[tag + "/seed"] = np.array(seed)
    lk, ls = D.digest("logits", logits)
    out[tag + "/logits_kept"], out[tag + "/logits_stat"] = lk, ls
    names = [k for k, g in g64.items() if g is not None]
    out[tag + "/nograd"] = np.array(json.dumps([k for k, g in g64.items() if g is None]))
    out[tag + "/grad_names"] = np.array(json.dumps(names))
    out[tag + "/grad_sizes"] = np.array(json.dumps([int(g64[k].size) for k in names]))
    dig = [D.digest(k, g64[k]) for k in names]
    out[tag + "/grad_kept"] = np.concatenate([d[0] for d in dig]).astype(np.float32)
    out[tag + "/grad_stat"] = np.stack([d[1] for d in dig])
    after = [(k, v) for k, v in m64.state_dict().items() if "running_" in k]
    if after:
        dig = [D.digest(k, v.numpy()) for k, v in after]
        out[tag + "/after_names"] = np.array(json.dumps([k for k, _ in after]))
        out[tag + "/after_kept"] = np.concatenate([d[0] for d in dig])
        out[tag + "/after_stat"] = np.stack([d[1] for d in dig])
        out[tag + "/after_batches"] = np.array([int(v) for k, v in m64.state_dict().items() if k.endswith("num_batches_tracked")])
    # the reference's own bf16 error per parameter: [L2 norm of the error, max |error| over the kept entries]
    lowp = "bf16"
    try:
        model16 = ctor(**ctor_kw(ref, kw))
        model16.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        l16, g16, _ = run(model16, x, G, torch.bfloat16)
        err = []
        for k in names:
            g, h = g64[k], g16[k]
            err.append([np.linalg.norm(h - g), np.abs(h - g)[D.sample_index(g.size)].max()])
        out[tag + "/ref_bf16_err"] = np.array(err, dtype=np.float64)
        out[tag + "/ref_bf16_logits_err"] = np.array(np.abs(l16 - logits).max())
    except Exception as e:                                           # noqa: BLE001 -- recorded in the fixture, the test reads it
        lowp = "none: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:160])
    out[tag + "/lowp"] = np.array(lowp)
    torch.set_num_threads(8)
    e = out.get(tag + "/ref_bf16_err")
    rel = None if e is None else e[:, 0] / out[tag + "/grad_stat"][:, 1]
    print("train-widths %-18s logits %s max %.3f, %d gradients, %d without; reference bf16: %s" % (
        tag, logits.shape, np.abs(logits).max(), len(names), len(json.loads(str(out[tag + "/nograd"]))),
        lowp if e is None else "rel L2 median %.2e max %.2e" % (np.median(rel), rel.max())), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated tags (with --check: compare only those)")
    args = ap.parse_args()
    ref = load_reference()
    only = set(args.only.split(",")) if args.only else None
    out = {}
    for tag, mod, cls, kw, seed in CASES:
        if only and tag not in only:
            continue
        out.update(make_case(ref, tag, mod, cls, kw, seed))
    if args.check:
        z = np.load(OUT)
        keys = [k for k in z.files if not only or k.split("/")[0] in only]
        bad = sorted(set(keys) ^ set(out)) + [k for k in keys if k in out and not np.array_equal(z[k], out[k])]
        print("check: %d arrays, %d differ" % (len(keys), len(bad)), bad[:10])
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
