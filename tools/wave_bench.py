#!/usr/bin/env python3
"""WaveMLP throughput on one GPU (bench.py's MODELS table is not extended for it): images/s of WaveMLP-T / -S through the HIP path, one step at a
time and two steps in flight (parallel.InFlight), against a torch-eager NCHW restatement of the same weights (F.conv2d / F.batch_norm / ...,
written here) timed the same way, in the same process.  HIP events around `--steps` steps after `--warmup` steps; portable weights (seed 0),
a seeded random batch.  Prints one JSON line per model and writes them to --out.

Also prints mlpk_wave_patm's algorithmic traffic per stage at this batch (it reads theta and x of both branches, 4C, and writes h and w, 2C,
per row): the numerator of its effective bandwidth against the kernel times of a `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/wave_bench.py --models T,S --batch 256 --dtype bf16 --out wave_bench.jsonl
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

from oracle.portable_init import portable_state_dict  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def bn(x, m):
    return F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)


def conv(x, c):
    return F.conv2d(x, c.weight, c.bias, c.stride, c.padding, c.dilation, c.groups)


def eager_forward(model, x):
    """the reference's eval-mode forward restated on NCHW with torch's functional ops, reading the module's parameters"""
    x = bn(conv(x, model.patch_embed.proj), model.patch_embed.norm)
    for stage in model.network:
        if hasattr(stage, "proj"):
            x = bn(conv(x, stage.proj), stage.norm)
            continue
        for blk in stage:
            a = blk.attn
            B, C = x.shape[:2]
            n = bn(x, blk.norm1)
            th = F.relu(bn(conv(n, a.theta_h_conv[0]), a.theta_h_conv[1]))
            tw = F.relu(bn(conv(n, a.theta_w_conv[0]), a.theta_w_conv[1]))
            xh, xw, c = conv(n, a.fc_h), conv(n, a.fc_w), conv(n, a.fc_c)
            h = conv(torch.cat([xh * torch.cos(th), xh * torch.sin(th)], 1), a.tfc_h)
            w = conv(torch.cat([xw * torch.cos(tw), xw * torch.sin(tw)], 1), a.tfc_w)
            s = F.adaptive_avg_pool2d(h + w + c, 1)
            r = conv(F.gelu(conv(s, a.reweight.fc1)), a.reweight.fc2).reshape(B, C, 3).permute(2, 0, 1).softmax(0)
            x = x + conv(h * r[0].view(B, C, 1, 1) + w * r[1].view(B, C, 1, 1) + c * r[2].view(B, C, 1, 1), a.proj)
            x = x + conv(F.gelu(conv(bn(x, blk.norm2), blk.mlp.fc1)), blk.mlp.fc2)
    x = F.adaptive_avg_pool2d(bn(x, model.norm), 1).flatten(1)
    return F.linear(x, model.head.weight, model.head.bias)


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


def patm_bytes(batch, dtype, hw=224):
    esz = torch.tensor([], dtype=dtype).element_size()
    h = (hw + 4 - 7) // 4 + 1
    out = []
    for C in (64, 128, 320, 512):
        rows = batch * h * h
        out.append({"map": h, "C": C, "rows": rows, "bytes": rows * 6 * C * esz})
        h = (h + 2 - 3) // 2 + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="T,S")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DT))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    dev = torch.device("cuda:0")
    dt = DT[args.dtype]
    torch.manual_seed(0)
    x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    lines = []
    for name in args.models.split(","):
        model = pkg.models_pytorch.WaveMLP(name)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}, strict=True)
        model = model.to(dev).eval()
        res = {"model": "WaveMLP-" + name, "batch": args.batch, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup}
        with torch.no_grad():
            ms1 = time_steps(model, x, args.steps, args.warmup)
            slots = parallel.InFlight(model, 2, device=dev)
            try:
                ms2 = time_in_flight(slots, x, args.steps, args.warmup)
            finally:
                slots.restore_plan()
            res.update({"hip_ms_per_step": round(ms1, 4), "hip_images_per_s": round(args.batch / ms1 * 1e3, 1),
                        "hip_in_flight_ms_per_step": round(ms2, 4), "hip_in_flight_images_per_s": round(args.batch / ms2 * 1e3, 1)})
            if not args.no_eager:
                em = model.to(dt)
                ref = eager_forward(em, x).float()
                got = model(x).float()
                res["hip_vs_eager_max_abs"] = float((got - ref).abs().max())
                res["eager_max_abs"] = float(ref.abs().max())
                mse = time_steps(lambda t: eager_forward(em, t), x, max(3, args.steps // 4), 2)
                res.update({"eager_ms_per_step": round(mse, 4), "eager_images_per_s": round(args.batch / mse * 1e3, 1),
                            "speedup_vs_eager": round(mse / ms1, 2)})
        res["patm_algorithmic_bytes"] = patm_bytes(args.batch, dt)
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
