#!/usr/bin/env python3
"""RaftMLP throughput on one GPU (bench.py's MODELS table is not extended for it): images/s of the two 224 x 224 configurations of
tests/golden/make_raft_golden.py ("pyramid": four levels, the project's own choice of shape; "single": the reference README's one-level
example) through the HIP path, one step at a time and two steps in flight (parallel.InFlight), against a torch-eager channel-last restatement
of the same weights (written here from the block's formulas: F.layer_norm / permute / F.linear / F.gelu) timed the same way, in the same process.
HIP events around `--steps` steps after `--warmup` steps; portable weights (seed 0), a seeded random batch.  Prints one JSON line per
configuration and writes them to --out.

Also prints the algorithmic traffic of mlpk_raft_gather_ln / mlpk_raft_scatter_add per level at this batch (one read + one write of the
activation per call, 2 x depth calls of each per level): the numerator of their effective bandwidth against the kernel times of a
`rocprofv3 --kernel-trace --stats` run of this tool (`--no-eager --no-in-flight`).

    python tools/raft_bench.py --configs pyramid,single --batch 256 --dtype bf16 --out raft_bench.jsonl
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.portable_init import portable_state_dict  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
CONFIGS = {
    "pyramid": [{"depth": 2, "dim": 96, "patch_size": 4, "raft_size": 2}, {"depth": 2, "dim": 192, "patch_size": 2, "raft_size": 2},
                {"depth": 6, "dim": 384, "patch_size": 2, "raft_size": 2}, {"depth": 2, "dim": 768, "patch_size": 2, "raft_size": 2}],
    "single": [{"depth": 12, "dim": 768, "patch_size": 16, "raft_size": 4}],
}


def mlp(x, fn):
    return F.linear(F.gelu(F.linear(x, fn[0].weight, fn[0].bias)), fn[3].weight, fn[3].bias)


def raft_half(x, blk, r, axis):
    """x (B, H, W, C) += the MLP over z[j L + l] of LayerNorm(x), c = j Co + co; the LayerNorm affine is stored in (co, j) order"""
    B, H, W, C = x.shape
    Co = C // r
    ln = blk.norm[1]
    g, b = ln.weight.view(Co, r).t().reshape(-1), ln.bias.view(Co, r).t().reshape(-1)
    n = F.layer_norm(x, (C,), g, b, ln.eps).view(B, H, W, r, Co)
    if axis == 0:
        y = mlp(n.permute(0, 2, 4, 3, 1).reshape(B, W, Co, r * H), blk.fn).view(B, W, Co, r, H).permute(0, 4, 1, 3, 2)
    else:
        y = mlp(n.permute(0, 1, 4, 3, 2).reshape(B, H, Co, r * W), blk.fn).view(B, H, Co, r, W).permute(0, 1, 4, 3, 2)
    return x + y.reshape(B, H, W, C)


def eager_forward(model, x):
    """the reference's eval-mode forward (ser_pm, shortcut, gap) restated on channel-last tensors, reading the module's parameters"""
    outs = []
    dl = model.layers[-1]["dim"]
    for li, (layer, lvl) in enumerate(zip(model.layers, model.levels)):
        p, r = layer["patch_size"], layer["raft_size"]
        if li > 0:
            x = x.permute(0, 3, 1, 2)
        if lvl._bh != lvl._h:
            x = F.interpolate(x, (lvl._h * p, lvl._h * p), mode="bilinear", align_corners=False)
        B, c, S, _ = x.shape
        h = S // p
        x = x.reshape(B, c, h, p, h, p).permute(0, 2, 4, 3, 5, 1).reshape(B, h, h, p * p * c)
        x = F.linear(x, lvl.fn[1].weight, lvl.fn[1].bias)
        for bi in range(layer["depth"]):
            seq = lvl.fn[2 + bi]
            x = raft_half(x, seq[1], r, 0)
            x = raft_half(x, seq[3], r, 1)
            cb = seq[5]
            x = x + mlp(F.layer_norm(x, (x.shape[-1],), cb.norm.weight, cb.norm.bias, cb.norm.eps), cb.fn)
        hd = model.heads[li]
        o = F.layer_norm(x, (x.shape[-1],), hd[1].weight, hd[1].bias, hd[1].eps).mean(dim=(1, 2))
        if li + 1 < len(model.layers):
            o = F.linear(o, hd[4].weight, hd[4].bias)
        outs.append(o)
    a = outs[-1]
    for o in reversed(outs[:-1]):
        a = o[:, :dl] * a + o[:, dl:]
    return F.linear(a, model.classifier.weight, model.classifier.bias)


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


def raft_bytes(layers, batch, dtype, size=224):
    esz = torch.tensor([], dtype=dtype).element_size()
    out = []
    for layer in layers:
        size = math.ceil(size / layer["patch_size"])
        act = batch * size * size * layer["dim"] * esz
        out.append({"map": size, "C": layer["dim"], "r": layer["raft_size"], "calls_per_forward_each": 2 * layer["depth"], "bytes_per_call": 2 * act})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="pyramid,single")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DT))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-in-flight", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raft_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    dev = torch.device("cuda:0")
    dt = DT[args.dtype]
    torch.manual_seed(0)
    x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    lines = []
    for name in args.configs.split(","):
        model = pkg.models_pytorch.RaftMLP(CONFIGS[name], gap=True)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}, strict=True)
        model = model.to(dev).eval()
        res = {"model": "RaftMLP-" + name, "batch": args.batch, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup}
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
            if not args.no_eager:
                em = model.to(dt)
                ref = eager_forward(em, x).float()
                got = model(x).float()
                res["hip_vs_eager_max_abs"] = float((got - ref).abs().max())
                res["eager_max_abs"] = float(ref.abs().max())
                mse = time_steps(lambda t: eager_forward(em, t), x, max(3, args.steps // 4), 2)
                res.update({"eager_ms_per_step": round(mse, 4), "eager_images_per_s": round(args.batch / mse * 1e3, 1),
                            "speedup_vs_eager": round(mse / ms1, 2)})
        res["raft_algorithmic_bytes"] = raft_bytes(CONFIGS[name], args.batch, dt)
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
