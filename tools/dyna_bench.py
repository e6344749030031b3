#!/usr/bin/env python3
"""DynaMixer throughput on one GPU (bench.py's MODELS table is not extended for it): images/s of DynaMixer T and M at 224 x 224 through the HIP
path, one step at a time and two steps in flight (parallel.InFlight), against a torch-eager channel-last restatement of the same weights (written
here from the block's formulas: the 2 s `Wd` Linears of both axes as one Linear, the attend Linear, softmax and matmul on permuted views) timed
the same way, in the same process.  HIP events around `--steps` steps after `--warmup` steps; portable weights (seed 0) with every attend.1
weight and bias times 8 as in tests/golden/make_dyna_golden.py, a seeded random batch.  Prints one JSON line per model and writes them to --out.

Also times the dynamic mixing alone, in the form the model takes (`form`: the unfused gather + GEMM + mlpk_dyna_mix_logits, or the fused
mlpk_dyna_mix), at each stage's shape and this batch, per axis (HIP events around `--kernel-reps` back-to-back calls after a
warm-up) and reports its EFFECTIVE bandwidth: algorithmic bytes = one read of x and of the axis's columns of t, one write of the mix and one read
of the attend weight, over the time per call.  The figure says how far from a pure data-movement pass the kernel is; `TFLOP_per_s` counts the
logits product (on the matrix pipe in the 16-bit types) and the mix (fp32, vector pipe).  `dyna_mix_share_of_step` = calls per forward x time per call, summed over stages and axes, over the event-timed step.

    python tools/dyna_bench.py --models T,M --batch 256 --dtype bf16 --out profiles/dyna_bench.jsonl
"""
import argparse
import copy
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
SCALE = 8.0


def eager_op(op, xn, t, axis):
    """DynaMixerOp on channel-last xn (B, H, W, C); t (B, H, W, s hd) = this op's Wd outputs"""
    B, H, W, C = xn.shape
    s = op.segment
    perm = (0, 1, 3, 2, 4) if axis == 1 else (0, 2, 3, 1, 4)
    L = W if axis == 1 else H
    xl = xn.view(B, H, W, s, C // s).permute(*perm)
    tl = t.reshape(B, H, W, s, -1).permute(*perm).reshape(B, -1, s, L * (t.shape[-1] // s))
    lin = op.attend[1]
    p = F.linear(tl, lin.weight, lin.bias).view(B, -1, s, L, L).softmax(-1)
    o = torch.matmul(p, xl)
    o = o.permute(0, 1, 3, 2, 4) if axis == 1 else o.permute(0, 3, 1, 2, 4)
    return op.proc(o.reshape(B, H, W, C))


def eager_forward(model, cat, x):
    """the reference's eval-mode forward restated on channel-last tensors, reading the module's parameters; cat[block] = the concatenated Wd
    weights and biases of both ops (made once, outside the timing)"""
    for stage in model.stages:
        conv = stage[0]
        x = F.conv2d(x, conv.weight, conv.bias, stride=conv.stride).permute(0, 2, 3, 1)              # NCHW between the stages
        for attn, ff in stage[1].layers:
            blk = attn.fn
            xn = attn.norm(x)
            w, b = cat[blk]
            t = F.linear(xn, w, b)
            n = t.shape[-1] // 2
            y = eager_op(blk.DynaMixerOp_h, xn, t[..., :n], 0) + eager_op(blk.DynaMixerOp_w, xn, t[..., n:], 1) + blk.proj_c(xn)
            x = x + blk.proj_o(y)
            x = x + ff.fn.net[3](F.gelu(ff.fn.net[0](ff.norm(x))))
        x = x.permute(0, 3, 1, 2)
    return model.mlp_head[1](x.mean(dim=(2, 3)))


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


def dyna_kernel_times(E, model, batch, dtype, dev, reps):
    """mlpk_dyna_mix alone at each stage's shape and axis: time per call (HIP events) and effective bandwidth"""
    esz = torch.tensor([], dtype=dtype).element_size()
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    for si, stage in enumerate(model.stages):
        depth, H, W, C, hd, s, _ = stage[1].__dict__["_geom"]
        rows = batch * H * W
        x = torch.randn((rows, C), device=dev, generator=g).to(dtype)
        t = (torch.rand((rows, 2 * s * hd), device=dev, generator=g) - 0.5).to(dtype)
        mean, rstd = torch.zeros((rows,), device=dev), torch.ones((rows,), device=dev)
        gamma, beta = torch.ones((C,), device=dev), torch.zeros((C,), device=dev)
        cat = torch.empty((rows, 3 * C), dtype=dtype, device=dev)
        for axis, opn in ((0, "DynaMixerOp_h"), (1, "DynaMixerOp_w")):
            lin = getattr(stage[1].layers[0][0].fn, opn).attend[1]
            aw, ab = E.pack_dyna_attend(lin.weight, lin.bias, dtype, dev)
            awr, ws = E.pack_matrix(lin.weight, dtype, dev), E.Workspace(dev, dtype)
            unfused = E.dyna_unfused_preferred(dtype, (H, W)[axis])             # the form the model takes at this shape

            def call():
                if unfused:
                    E.dyna_mix_unfused(ws, "k", x, mean, rstd, gamma, beta, t, axis * s * hd, awr, ab, cat[:, axis * C:(axis + 1) * C], batch, H, W, C, s, hd, axis)
                else:
                    E.dyna_mix(x, mean, rstd, gamma, beta, t, axis * s * hd, aw, ab, cat[:, axis * C:(axis + 1) * C], batch, H, W, C, s, hd, axis)
            us = time_steps(lambda _: call(), None, reps, 5) * 1e3
            L = (H, W)[axis]
            nbytes = (rows * (2 * C + s * hd) + aw.numel()) * esz
            flops = 2.0 * (rows // L * s) * (L * L * L * hd + L * L * (C // s))
            out.append({"stage": si + 1, "axis": "hw"[axis], "L": L, "C": C, "segment": s, "hd": hd, "form": "unfused" if unfused else "fused", "calls_per_forward": depth,
                        "us_per_call": round(us, 2), "algorithmic_bytes": nbytes, "effective_TB_per_s": round(nbytes / us * 1e-6, 3),
                        "TFLOP_per_s": round(flops / us * 1e-6, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="T,M")
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
        raise SystemExit("dyna_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    dev = torch.device("cuda:0")
    dt = DT[args.dtype]
    torch.manual_seed(0)
    x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    lines = []
    for name in args.models.split(","):
        model = pkg.models_pytorch.DynaMixer(name)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = portable_state_dict(shapes, seed=0)
        for k in sd:
            if ".attend.1." in k:
                sd[k] = sd[k] * SCALE
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model = model.to(dev).eval()
        res = {"model": "DynaMixer-" + name, "batch": args.batch, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup}
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
            kt = dyna_kernel_times(pkg.engine, model, args.batch, dt, dev, args.kernel_reps)
            res["dyna_mix"] = kt
            mix_ms = sum(k["calls_per_forward"] * k["us_per_call"] for k in kt) * 1e-3
            res["dyna_mix_ms_per_step"] = round(mix_ms, 4)
            res["dyna_mix_share_of_step"] = round(mix_ms / ms1, 4)
            res["dyna_mix_effective_TB_per_s"] = round(sum(k["calls_per_forward"] * k["algorithmic_bytes"] for k in kt) / mix_ms * 1e-9, 3)
            if not args.no_eager:
                em = copy.deepcopy(model).to(dt)                       # (a copy: the model under test keeps the weights it was timed with)
                cat = {}
                for stage in em.stages:
                    for attn, _ in stage[1].layers:
                        ops = [attn.fn.DynaMixerOp_h, attn.fn.DynaMixerOp_w]
                        cat[attn.fn] = (torch.cat([lin.weight for op in ops for lin in op.Wd], 0), torch.cat([lin.bias for op in ops for lin in op.Wd], 0))
                ref = eager_forward(em, cat, x).float()
                got = model(x).float()
                res["hip_vs_eager_max_abs"] = float((got - ref).abs().max())
                res["eager_max_abs"] = float(ref.abs().max())
                mse = time_steps(lambda t: eager_forward(em, cat, t), x, max(3, args.steps // 4), 2)
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
