#!/usr/bin/env python3
"""ActiveMLP throughput on one GPU (bench.py's MODELS table is not extended for it): images/s of ActiveTiny and ActiveSmall at 224 x 224 through
the HIP path, one step at a time and two steps in flight (parallel.InFlight), against a torch-eager channel-last restatement of the same weights
(written here from the block's formulas; the 1-D sampling with torch.gather, since torchvision's deform_conv2d is not installed) timed the same
way, in the same process.  HIP events around `--steps` steps after `--warmup` steps; portable weights (seed 0) with every offset Linear's bias
drawn from [-3, 3) as in tests/golden/make_active_golden.py, a seeded random batch.  Prints one JSON line per model and writes them to --out.

Also times mlpk_atm_sample alone at each stage's shape and this batch (HIP events around `--kernel-reps` back-to-back calls after a warm-up, real
offsets in [-3, 3)) and reports its EFFECTIVE bandwidth: algorithmic bytes = one read of x and of the offsets + three writes, over the time per
call (the kernel reads x twice, the second time from cache; stages whose tensors fit the 256 MiB Infinity Cache are served from it, as they are
inside a forward).  `atm_share_of_step` = calls per forward x time per call, summed over the stages, over the event-timed step.

    python tools/active_bench.py --models ActiveTiny,ActiveSmall --batch 256 --dtype bf16 --out profiles/active_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.portable_init import portable_state_dict, portable_tensor  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def sample(v, off, dim):
    """v (B, H, W, C), off (B, H, W, C) one offset per channel: linear interpolation of v along `dim` (1: h, 2: w) at position + offset, zero
    outside (-1, L) and for a neighbour outside [0, L - 1]; positions and weights in fp32"""
    L = v.shape[dim]
    shape = [1, 1, 1, 1]
    shape[dim] = L
    p = torch.arange(L, device=v.device, dtype=torch.float32).view(shape) + off.float()
    inside = (p > -1) & (p < L)
    i0 = torch.floor(torch.where(inside, p, torch.zeros_like(p)))
    f = torch.where(inside, p, torch.zeros_like(p)) - i0
    i0 = i0.long()

    def tap(i, w):
        ok = inside & (i >= 0) & (i <= L - 1)
        return torch.gather(v, dim, i.clamp(0, L - 1)).float() * torch.where(ok, w, torch.zeros_like(w))
    return (tap(i0, 1 - f) + tap(i0 + 1, f)).to(v.dtype)


def eager_forward(model, x):
    """the reference's eval-mode forward restated on channel-last tensors, reading the module's parameters"""
    pe = model.patch_embed.proj
    x = F.conv2d(x, pe.weight, pe.bias, stride=4, padding=2).permute(0, 2, 3, 1)
    for si, stage in enumerate(model.blocks):
        off = None
        for blk in stage:
            C = x.shape[-1]
            if blk.offset_layer is not None:
                peg = model.pos_blocks[si].proj
                xc = x.permute(0, 3, 1, 2)
                x = (F.conv2d(xc, peg.weight, peg.bias, padding=1, groups=C) + xc).permute(0, 2, 3, 1)
                off = blk.offset_layer(x).repeat_interleave(blk.share_dim, dim=-1)
            atm = blk.atm
            xn = blk.norm1(x)
            w = F.linear(sample(xn, off[..., :C], 2), atm.atm_w.weight.view(C, C), atm.atm_w.bias)
            h = F.linear(sample(xn, off[..., C:], 1), atm.atm_h.weight.view(C, C), atm.atm_h.bias)
            c = atm.atm_c(xn)
            a = (w + h + c).mean(dim=(1, 2))
            a = F.linear(F.gelu(F.linear(a, atm.fusion.fc1.weight, atm.fusion.fc1.bias)), atm.fusion.fc2.weight, atm.fusion.fc2.bias)
            a = a.reshape(-1, C, 3).permute(2, 0, 1).softmax(dim=0)[:, :, None, None, :]
            x = x + atm.proj(w * a[0] + h * a[1] + c * a[2])
            m = blk.mlp
            x = x + F.linear(F.gelu(F.linear(blk.norm2(x), m.fc1.weight, m.fc1.bias)), m.fc2.weight, m.fc2.bias)
            if blk.downsample is not None:
                d = blk.downsample.proj
                x = F.conv2d(x.permute(0, 3, 1, 2), d.weight, d.bias, stride=2, padding=1).permute(0, 2, 3, 1)
    x = model.norm(x).mean(dim=(1, 2))
    return model.head(x)


def time_steps(fn, x, steps, warmup):
    for _ in range(warmup):
        fn(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def time_in_flight(slots, x, steps, warmup):
    cur = torch.cuda.current_stream()
    for _ in range(warmup):
        slots(x)
    slots.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    for _ in range(steps):
        slots(x)
    for s in slots.streams:
        cur.wait_stream(s)
    e1.record(cur)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def atm_kernel_times(E, model, batch, dtype, dev, reps):
    """mlpk_atm_sample alone at each stage's shape: time per call (HIP events) and effective bandwidth"""
    esz = torch.tensor([], dtype=dtype).element_size()
    out, size = [], (224 + 4 - 7) // 4 + 1
    g = torch.Generator(device=dev).manual_seed(1)
    for si, stage in enumerate(model.blocks):
        C, share = stage[0].atm.dim, stage[0].share_dim
        rows = batch * size * size
        x = torch.randn((rows, C), device=dev, generator=g).to(dtype)
        off = ((torch.rand((rows, 2 * C // share), device=dev, generator=g) - 0.5) * 6.0).to(dtype)
        mean, rstd = torch.zeros((rows,), device=dev), torch.ones((rows,), device=dev)
        gamma, beta = torch.ones((C,), device=dev), torch.zeros((C,), device=dev)
        o = [torch.empty((rows, C), dtype=dtype, device=dev) for _ in range(3)]

        def call():
            E.atm_sample(x, mean, rstd, gamma, beta, off, share, o[0], o[1], o[2], batch, size, size, C)
        us = time_steps(lambda _: call(), None, reps, 5) * 1e3
        nbytes = (rows * C * 4 + rows * (2 * C // share)) * esz
        out.append({"stage": si, "map": size, "C": C, "share": share, "calls_per_forward": len(stage), "us_per_call": round(us, 2),
                    "algorithmic_bytes": nbytes, "effective_TB_per_s": round(nbytes / us * 1e-6, 3)})
        size = (size + 2 - 3) // 2 + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ActiveTiny,ActiveSmall")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DT))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-in-flight", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("active_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    dev = torch.device("cuda:0")
    dt = DT[args.dtype]
    torch.manual_seed(0)
    x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    lines = []
    for name in args.models.split(","):
        model = getattr(pkg.models_pytorch.active_mlp, name)()
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = portable_state_dict(shapes, seed=0)
        for k in sd:
            if k.endswith("offset_layer.1.bias"):
                sd[k] = portable_tensor(k, shapes[k], -3.0, 3.0, seed=0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model = model.to(dev).eval()
        res = {"model": name, "batch": args.batch, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup}
        with torch.no_grad():
            ms1 = time_steps(model, x, args.steps, args.warmup)
            res.update({"hip_ms_per_step": round(ms1, 4), "hip_images_per_s": round(args.batch / ms1 * 1e3, 1)})
            if not args.no_in_flight:
                slots = parallel.InFlight(model, 2, device=dev)
                try:
                    ms2 = time_in_flight(slots, x, args.steps, args.warmup)
                finally:
                    slots.restore_plan()
                res.update({"hip_in_flight_ms_per_step": round(ms2, 4), "hip_in_flight_images_per_s": round(args.batch / ms2 * 1e3, 1)})
            kt = atm_kernel_times(pkg.engine, model, args.batch, dt, dev, args.kernel_reps)
            res["atm_sample"] = kt
            atm_ms = sum(k["calls_per_forward"] * k["us_per_call"] for k in kt) * 1e-3
            res["atm_ms_per_step"] = round(atm_ms, 4)
            res["atm_share_of_step"] = round(atm_ms / ms1, 4)
            res["atm_effective_TB_per_s"] = round(sum(k["calls_per_forward"] * k["algorithmic_bytes"] for k in kt) / atm_ms * 1e-9, 3)
            if not args.no_eager:
                em = model.to(dt)
                ref = eager_forward(em, x).float()
                got = model(x).float()
                res["hip_vs_eager_max_abs"] = float((got - ref).abs().max())
                res["eager_max_abs"] = float(ref.abs().max())
                mse = time_steps(lambda t: eager_forward(em, t), x, max(3, args.steps // 4), 2)
                res.update({"eager_ms_per_step": round(mse, 4), "eager_images_per_s": round(args.batch / mse * 1e3, 1),
                            "speedup_vs_eager": round(mse / ms1, 2)})
        print(json.dumps(res), flush=True)
        lines.append(res)
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
