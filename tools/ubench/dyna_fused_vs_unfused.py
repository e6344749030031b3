#!/usr/bin/env python3
"""The two forms of DynaMixer's dynamic token mixing, at the stage shapes of DynaMixer T and M, batch 256, bf16, both axes, in one process,
alternating:
  fused     one mlpk_dyna_mix launch: the logits never leave the chip;
  unfused   engine.dyna_mix_unfused: mlpk_dyna_gather (the GEMM's operand rows v[item][l hd + j] from t), the logits through engine.gemm -- rows =
            (line, segment) items, N = L L, K = L hd, bias in the epilogue -- into a 16-bit (items, L L) buffer, then mlpk_dyna_mix_logits, which runs
            the fused kernel's own device code for the softmax and the mix (csrc/mlpk_dyna.h).
Per shape and axis: `--rounds` rounds, each timing `--reps` back-to-back calls of one form and then of the other with HIP events after a warm-up;
the median, the fastest and the slowest round of each form are reported, the gather and the GEMM alone as columns of their own, and the largest
difference between the two outputs (the unfused logits are rounded to bf16, so the outputs differ in the last bits).  The model takes the form that
wins here (engine.dyna_unfused_preferred).  One JSON line per shape and axis, also to --out.

    python tools/ubench/dyna_fused_vs_unfused.py --out profiles/dyna_mix_fused_vs_unfused.jsonl
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# (model, stage, H, W, C, segment, hidden_dim_DMO) at 224 x 224
SHAPES = [("T", 1, 32, 32, 192, 8, 2), ("T", 2, 16, 16, 384, 16, 2), ("M", 1, 32, 32, 256, 8, 2), ("M", 2, 16, 16, 512, 16, 2)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3            # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dyna_fused_vs_unfused needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    E = pkg.engine
    dev, dt, B = torch.device("cuda:0"), torch.bfloat16, args.batch
    g = torch.Generator(device=dev).manual_seed(2)
    lines = []
    for model, stage, H, W, C, s, hd in SHAPES:
        rows = B * H * W
        x = torch.randn((rows, C), device=dev, generator=g).to(dt)
        t = (torch.rand((rows, 2 * s * hd), device=dev, generator=g) * 2 - 1).to(dt)
        mean, rstd = torch.zeros((rows,), device=dev), torch.ones((rows,), device=dev)
        gamma, beta = torch.ones((C,), device=dev), torch.zeros((C,), device=dev)
        for axis in (0, 1):
            L, Q = (W, H) if axis == 1 else (H, W)
            K, NN, items = L * hd, L * L, B * Q * s
            bound = K ** -0.5
            w = (torch.rand((NN, K), device=dev, generator=g) * 2 - 1) * bound * 8.0
            b = (torch.rand((NN,), device=dev, generator=g) * 2 - 1) * bound * 8.0
            aw, ab = E.pack_dyna_attend(w, b, dt, dev)
            wrm = E.pack_matrix(w, dt, dev)                                      # (L L, K) row-major for the GEMM
            kp = wrm.shape[1]
            v = torch.zeros((items, kp), dtype=dt, device=dev)
            z = torch.empty((items, NN), dtype=dt, device=dev)
            ws = E.Workspace(dev, dt)
            outs = [torch.empty((rows, C), dtype=dt, device=dev) for _ in range(2)]

            def fused():
                E.dyna_mix(x, mean, rstd, gamma, beta, t, axis * s * hd, aw, ab, outs[0], B, H, W, C, s, hd, axis)

            def unfused():
                E.dyna_mix_unfused(ws, "u", x, mean, rstd, gamma, beta, t, axis * s * hd, wrm, ab, outs[1], B, H, W, C, s, hd, axis)

            def gather():
                E.dyna_gather(t, axis * s * hd, v, kp, B, H, W, s, hd, axis)

            def gemm_only():
                E.gemm(v, wrm, z, items, NN, kp, bias=ab)

            for fn in (fused, unfused):                                          # warm-up
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            diff = float((outs[0].float() - outs[1].float()).abs().max())
            tf, tu, tg, tv = [], [], [], []
            for _ in range(args.rounds):
                tf.append(timed(fused, args.reps))
                tu.append(timed(unfused, args.reps))
                tg.append(timed(gemm_only, args.reps))
                tv.append(timed(gather, args.reps))
            esz = 2
            res = {"model": "DynaMixer-" + model, "stage": stage, "axis": "hw"[axis], "L": L, "C": C, "segment": s, "hd": hd, "batch": B, "dtype": "bf16",
                   "rounds": args.rounds, "reps": args.reps,
                   "fused_us": {"median": round(statistics.median(tf), 2), "min": round(min(tf), 2), "max": round(max(tf), 2)},
                   "unfused_us": {"median": round(statistics.median(tu), 2), "min": round(min(tu), 2), "max": round(max(tu), 2)},
                   "unfused_gemm_only_us": {"median": round(statistics.median(tg), 2)},
                   "unfused_gather_us": {"median": round(statistics.median(tv), 2)},
                   "logits_bytes_written_and_read_unfused": 2 * items * NN * esz,
                   "unfused_over_fused": round(statistics.median(tu) / statistics.median(tf), 3),
                   "max_abs_difference_of_outputs": diff, "max_abs_output": float(outs[0].float().abs().max())}
            print(json.dumps(res), flush=True)
            lines.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
