#!/usr/bin/env python3
"""ConvMLP on one GPU (bench.py's MODELS table is not extended for it): a driver that starts every measurement as a child process of its own
behind `timeout`, with a limit sized to that run, stops at the first run that fails, and writes one JSON line per run to --out (the file is
REWRITTEN from this invocation's runs, after every run that finishes: one file holds one session).

Runs, per model (convmlp_s, convmlp_m; 256 images, bf16, 224 x 224, portable weights of seed 0, a seeded random batch, HIP events):
  step      images/s through the HIP path, one step at a time and with two steps in flight (parallel.InFlight)
  eager     the same weights through `eager_forward`, a torch-eager restatement of conv_mlp.py written from its formulas (conv2d, batch_norm,
            relu, max_pool2d, layer_norm, linear, gelu on the device), timed the same way; the distance of the two outputs
  profile   ONE step with HIP events around every launch of the new kernels, of the dense 3 x 3 products read through the window
            (`dense_3x3`) and of the tokenizer's first convolution (`stem_im2col` + `stem_gemm`, its own buckets; the engine's wrappers are
            wrapped for that step): the share of the step spent in the ReLU passes (mlpk_relu_add without and with the residual,
            mlpk_relu_maxpool3s2_nhwc), in mlpk_ln_dwconv3_nhwc and in the dense 3 x 3 products, without and with the stem
and for S only:
  kernels   each new kernel alone at every shape S gives it: time per call and effective bandwidth = the bytes it must move (every operand
            once) over that time.  Consecutive calls rotate over operand sets of at least ROTATE_BYTES in all, four times the 256 MB last-level
            cache, so no call finds its operands there (inside a step a ReLU pass follows the product that wrote its tensor and may)
  connect   mlpk_ln_dwconv3_nhwc against mlpk_norm_apply + mlpk_dwconv_plain_nhwc on the same tensors at the three stage shapes of S, ALTERNATING
            in one process -- `--kernel-reps` back-to-back calls of one, then of the other, `--rounds` times, the median round reported

    python tools/convmlp_bench.py --out profiles/convmlp_bench.jsonl
"""
import argparse
import copy
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# run -> (models, time limit in seconds: import + packing + warm-up + the timed steps, with a wide margin; a run that needs longer has hung)
RUNS = [("step", ("S", "M"), 240), ("eager", ("S", "M"), 240), ("profile", ("S", "M"), 180), ("kernels", ("S",), 180), ("connect", ("S",), 180)]
FACTORY = {"S": "convmlp_s", "M": "convmlp_m"}
ROTATE_BYTES = 1 << 30


# ------------------------------------------------------------------ the torch-eager restatement (conv_mlp.py's forward, eval mode)
def eager_forward(model, x):
    import torch.nn.functional as F

    def conv_bn_relu(x, conv, bn):
        x = F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding)
        return F.relu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))

    def mlp(x, norm, m):
        h = F.layer_norm(x, norm.normalized_shape, norm.weight, norm.bias, norm.eps)
        return F.linear(F.gelu(F.linear(h, m.fc1.weight, m.fc1.bias)), m.fc2.weight, m.fc2.bias)

    tok = model.tokenizer.block
    for i in (0, 3, 6):
        x = conv_bn_relu(x, tok[i], tok[i + 1])
    x = F.max_pool2d(x, 3, 2, 1)
    for blk in model.conv_stages.conv_blocks:
        y = x
        for i in (0, 3, 6):
            y = conv_bn_relu(y, blk[i], blk[i + 1])
        x = x + y
    d = model.conv_stages.downsample
    x = F.conv2d(x, d.weight, d.bias, d.stride, d.padding).permute(0, 2, 3, 1)
    for stage in model.stages:
        for b in stage.blocks:
            x = x + mlp(x, b.norm1, b.channel_mlp1)
            n = b.connect_norm
            v = F.layer_norm(x, n.normalized_shape, n.weight, n.bias, n.eps).permute(0, 3, 1, 2)
            x = F.conv2d(v, b.connect.weight, None, 1, 1, 1, b.connect.groups).permute(0, 2, 3, 1)
            x = x + mlp(x, b.norm2, b.channel_mlp2)
        if hasattr(stage.downsample_mlp, "downsample"):
            d = stage.downsample_mlp.downsample
            x = F.conv2d(x.permute(0, 3, 1, 2), d.weight, d.bias, d.stride, d.padding).permute(0, 2, 3, 1)
    n = model.norm
    x = F.layer_norm(x, n.normalized_shape, n.weight, n.bias, n.eps).flatten(1, 2).mean(1)
    return F.linear(x, model.head.weight, model.head.bias)


# ------------------------------------------------------------------ timing
def time_steps(fn, x, steps, warmup):
    import torch
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
    import torch
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


def s_shapes(batch):
    """the shapes ConvMLP-S at 224 x 224 gives the new kernels: name -> [(calls per forward, B, H, W, C)]"""
    return {"relu_add": [(2, batch, 112, 112, 32), (4, batch, 56, 56, 128)], "relu_add_res": [(2, batch, 56, 56, 64)],
            "relu_maxpool3s2": [(1, batch, 112, 112, 64)], "ln_dwconv3": [(2, batch, 28, 28, 128), (4, batch, 14, 14, 256), (2, batch, 7, 7, 512)]}


def load_model(pkg, name, dev):
    import torch
    from oracle.portable_init import portable_state_dict
    model = getattr(pkg.models_pytorch, FACTORY[name])()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}, strict=True)
    return model.to(dev).eval()


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("convmlp_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    E = pkg.engine
    dev = torch.device("cuda:0")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    esz = torch.tensor([], dtype=dt).element_size()
    torch.manual_seed(0)
    res = {"run": args.run, "model": "ConvMLP-" + args.model, "batch": args.batch, "dtype": args.dtype}
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)

    if args.run in ("step", "eager", "profile"):
        model = load_model(pkg, args.model, dev)
        x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    with torch.no_grad():
        if args.run == "step":
            parallel = importlib.import_module("jittor-mlp_amd.parallel")
            ms1 = time_steps(model, x, args.steps, args.warmup)
            slots = parallel.InFlight(model, 2, device=dev)
            try:
                ms2 = time_in_flight(slots, x, args.steps, args.warmup)
            finally:
                slots.restore_plan()
            res.update({"steps": args.steps, "warmup": args.warmup, "hip_ms_per_step": round(ms1, 4), "hip_images_per_s": round(args.batch / ms1 * 1e3, 1),
                        "hip_in_flight_ms_per_step": round(ms2, 4), "hip_in_flight_images_per_s": round(args.batch / ms2 * 1e3, 1)})
        elif args.run == "eager":
            em = copy.deepcopy(model).to(dt)                           # (a copy: the model under test keeps the weights it was timed with)
            ref = eager_forward(em, x).float()
            ms1 = time_steps(model, x, args.steps, args.warmup)
            got = model(x).float()
            mse = time_steps(lambda t: eager_forward(em, t), x, max(3, args.steps // 2), 2)
            res.update({"hip_ms_per_step": round(ms1, 4), "hip_images_per_s": round(args.batch / ms1 * 1e3, 1), "eager_ms_per_step": round(mse, 4),
                        "eager_images_per_s": round(args.batch / mse * 1e3, 1), "speedup_vs_eager": round(mse / ms1, 2),
                        "hip_vs_eager_max_abs": float((got - ref).abs().max()), "eager_max_abs": float(ref.abs().max())})
        elif args.run == "profile":
            for _ in range(args.warmup):
                model(x)
            torch.cuda.synchronize()
            ms1 = time_steps(model, x, args.steps, 0)
            events, orig = [], {}

            def wrap(name, label):
                fn = orig[name] = getattr(E, name)

                def timed(*a, **k):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn(*a, **k)
                    e1.record()
                    if label(a, k) is not None:
                        events.append((label(a, k), e0, e1))
                    return out
                setattr(E, name, timed)
            wrap("relu_add", lambda a, k: "relu_add_res" if a[1] is not None else "relu_add")
            wrap("relu_maxpool3s2_nhwc", lambda a, k: "relu_maxpool3s2")
            wrap("ln_dwconv3_nhwc", lambda a, k: "ln_dwconv3")
            wrap("conv_gemm_nhwc", lambda a, k: "dense_3x3")
            wrap("im2col", lambda a, k: "stem_im2col" if a[0].dim() == 4 else "im2col")                 # (the NCHW image: the tokenizer's first convolution)
            wrap("gemm", lambda a, k: {"convmlp_stem": "stem_gemm", "convmlp_3x3": "dense_3x3"}.get(k.get("tag")) if not k.get("_defer") else None)
            try:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(x)
                e1.record()
                torch.cuda.synchronize()
            finally:
                for name, fn in orig.items():
                    setattr(E, name, fn)
            tot, cnt = {}, {}
            for label, a, b in events:
                tot[label] = tot.get(label, 0.0) + a.elapsed_time(b)
                cnt[label] = cnt.get(label, 0) + 1
            relu = sum(tot.get(k, 0.0) for k in ("relu_add", "relu_add_res", "relu_maxpool3s2"))
            stem = tot.get("stem_im2col", 0.0) + tot.get("stem_gemm", 0.0)
            res.update({"ms_per_step": round(ms1, 4), "profiled_step_ms": round(e0.elapsed_time(e1), 4), "launches": cnt,
                        "ms": {k: round(v, 4) for k, v in tot.items()}, "relu_ms": round(relu, 4), "relu_share_of_step": round(relu / ms1, 4),
                        "ln_dwconv3_share_of_step": round(tot.get("ln_dwconv3", 0.0) / ms1, 4), "dense_3x3_share_of_step": round(tot.get("dense_3x3", 0.0) / ms1, 4),
                        "relu_over_dense_3x3": round(relu / tot["dense_3x3"], 3) if tot.get("dense_3x3") else None,
                        "stem_ms": round(stem, 4), "relu_over_dense_3x3_and_stem": round(relu / (tot.get("dense_3x3", 0.0) + stem), 3) if stem else None})
        elif args.run == "kernels":
            out = []
            for kind, shapes in s_shapes(args.batch).items():
                for calls, B, H, W, C in shapes:
                    n = B * H * W * C
                    if kind == "relu_add":
                        nbytes = 2 * n * esz
                        make = lambda: (rnd(B, H, W, C).to(dt),)
                        call = lambda y: E.relu_add(y, None, y, n)
                    elif kind == "relu_add_res":
                        nbytes = 3 * n * esz
                        make = lambda: (rnd(B, H, W, C).to(dt), rnd(B, H, W, C).to(dt))
                        call = lambda y, r: E.relu_add(y, r, r, n)
                    elif kind == "relu_maxpool3s2":
                        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                        nbytes = (n + B * Ho * Wo * C) * esz
                        make = lambda: (rnd(B, H, W, C).to(dt), torch.empty((B, Ho, Wo, C), dtype=dt, device=dev))
                        call = lambda y, o: E.relu_maxpool3s2_nhwc(y, o, B, H, W, C)
                    else:
                        nbytes = 2 * n * esz + B * H * W * 8 + 11 * C * 4
                        make = lambda: (rnd(B, H, W, C).to(dt), rnd(B * H * W), rnd(B * H * W).abs() + 0.5, rnd(C), rnd(C), rnd(9, C),
                                        torch.empty((B, H, W, C), dtype=dt, device=dev))
                        call = lambda y, mean, rstd, ga, be, w, o: E.ln_dwconv3_nhwc(y, mean, rstd, ga, be, w, o, B, H, W, C)
                    sets = [make() for _ in range(max(2, -(-ROTATE_BYTES // nbytes)))]
                    turn = [0]

                    def fn(_):
                        call(*sets[turn[0] % len(sets)])
                        turn[0] += 1
                    us = statistics.median(time_steps(fn, None, args.kernel_reps, 3) for _ in range(args.rounds)) * 1e3
                    out.append({"kernel": kind, "shape": [B, H, W, C], "calls_per_forward": calls, "us_per_call": round(us, 2), "bytes": nbytes,
                                "operand_sets": len(sets), "effective_TB_per_s": round(nbytes / us * 1e-6, 3)})
                    del sets
            res["kernels"] = out
        elif args.run == "connect":
            out = []
            for calls, B, H, W, C in s_shapes(args.batch)["ln_dwconv3"]:
                rows = B * H * W
                y = rnd(rows, C).to(dt)
                o, xn = torch.empty_like(y), torch.empty_like(y)
                mean, rstd, ga, be, w = rnd(rows), rnd(rows).abs() + 0.5, rnd(C), rnd(C), rnd(9, C)

                def fused(_):
                    E.ln_dwconv3_nhwc(y, mean, rstd, ga, be, w, o, B, H, W, C)

                def two_pass(_):
                    E.norm_apply(y, rows, C, C, mean=mean, rstd=rstd, gamma=ga, beta=be, out_rm=xn, ld_rm=C)
                    E.dwconv_plain_nhwc(xn, o, B, H, W, C, 3, w, None)
                two_pass(None)
                want = o.clone()
                fused(None)
                torch.cuda.synchronize()
                diff = float((o.float() - want.float()).abs().max())
                f, t = [], []
                for _ in range(args.rounds):                           # alternating: both sides see the same clocks and the same neighbours
                    f.append(time_steps(fused, None, args.kernel_reps, 3) * 1e3)
                    t.append(time_steps(two_pass, None, args.kernel_reps, 3) * 1e3)
                fu, tu = statistics.median(f), statistics.median(t)
                out.append({"shape": [B, H, W, C], "calls_per_forward": calls, "fused_us": round(fu, 2), "two_pass_us": round(tu, 2),
                            "two_pass_over_fused": round(tu / fu, 3), "fused_us_rounds": [round(v, 2) for v in f], "two_pass_us_rounds": [round(v, 2) for v in t],
                            "max_abs_difference": diff})
            res["connect"] = out
            res["fused_not_slower_everywhere"] = all(r["fused_us"] <= r["two_pass_us"] for r in out)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="S,M")
    ap.add_argument("--runs", default=",".join(r[0] for r in RUNS))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--run", default=None, help="(internal) one run in this process")
    ap.add_argument("--model", default="S")
    args = ap.parse_args()
    if args.run:
        return child(args)
    lines = []
    for run, models, limit in RUNS:
        if run not in args.runs.split(","):
            continue
        for name in models:
            if name not in args.models.split(","):
                continue
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--run", run, "--model", name, "--batch", str(args.batch),
                   "--dtype", args.dtype, "--steps", str(args.steps), "--warmup", str(args.warmup), "--kernel-reps", str(args.kernel_reps),
                   "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                      # a failed, faulted or hung run ends the session: nothing more is started
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("convmlp_bench: run %s of ConvMLP-%s ended with status %d; stopping" % (run, name, r.returncode))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(line)
            if args.out:                                               # written run by run: what finished stays on disk
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
