#!/usr/bin/env python3
"""Sequencer2D throughput on one GPU (bench.py's MODELS table is not extended for it): images/s of Sequencer2D S and M at 224 x 224 through the
HIP path, one step at a time and two steps in flight (parallel.InFlight), against a torch-eager channel-last restatement of the same weights
whose LSTMs are the module's own torch.nn.LSTM run on the device -- the library baseline a user would otherwise get -- timed the same way, in
the same process.  HIP events around `--steps` steps after `--warmup` steps; portable weights (seed 0), a seeded random batch.  Prints one JSON
line per model and writes them to --out.

Also times the recurrence alone: mlpk_lstm_scan at each stage's shape and this batch, per axis, beside nn.LSTM on the same sequences (nn.LSTM
computes its input projections itself, so the projection GEMM is timed too and added to the scan for the comparison: see `lstm_alone`),
ALTERNATING in one process -- `--kernel-reps` back-to-back calls of one, then of the other, `--rounds` times, the median round reported.
`effective_TB_per_s` = algorithmic bytes (one read of
the 8 hid projection columns, one write of the 2 hid hidden states, one read of W_hh) over the time per call; `scan_share_of_step` = calls per
forward x time per call, summed over stages and axes, over the event-timed step.

If nn.LSTM does not run in the requested type on the device, the eager side runs in the first of fp16 / fp32 that does and the record says so
(`eager_dtype`, `eager_note`).

    python tools/sequencer_bench.py --models S,M --batch 256 --dtype bf16 --out profiles/sequencer_bench.jsonl
"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.portable_init import portable_state_dict  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NAME = {v: k for k, v in DT.items()}


def eager_bilstm(mod, x):
    """BiLSTM2D on channel-last x (B, H, W, C) with the module's own nn.LSTMs (sequencer.py:38-46)"""
    B, H, W, C = x.shape
    v, _ = mod.rnn_v(x.permute(0, 2, 1, 3).reshape(-1, H, C))
    v = v.reshape(B, W, H, -1).permute(0, 2, 1, 3)
    h, _ = mod.rnn_h(x.reshape(-1, W, C))
    h = h.reshape(B, H, W, -1)
    return mod.fc(torch.cat([v, h], dim=-1))


def eager_forward(model, x):
    """the reference's eval-mode forward restated on channel-last tensors, reading the module's parameters"""
    for stage in model.stages:
        conv = stage[0]
        x = F.conv2d(x, conv.weight, conv.bias, stride=conv.stride).permute(0, 2, 3, 1)              # NCHW between the stages
        for mix, ff in stage[1].model:
            x = x + eager_bilstm(mix.fn[0], mix.norm(x))
            x = x + ff.fn[3](F.gelu(ff.fn[0](ff.norm(x))))
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


def first_working_dtype(make, dt):
    """(dtype, note): the requested type if `make(dtype)` runs in it on the device, else the first of fp16 / fp32 that does"""
    note = None
    for cand in [dt] + [c for c in (torch.float16, torch.float32) if c != dt]:
        try:
            make(cand)
            torch.cuda.synchronize()
            return cand, note
        except Exception as e:                                         # nn.LSTM's device library does not take every type
            note = "%s in %s: %s: %s" % ("nn.LSTM", NAME[cand], type(e).__name__, str(e).splitlines()[0][:160])
    raise RuntimeError(note)


def lstm_alone(E, model, batch, dt, dev, reps, rounds):
    """mlpk_lstm_scan at each stage's shape and axis beside nn.LSTM on the same sequences.  The scan reads ready projections; nn.LSTM computes its
    own from an input of the stage's width, so `nn_lstm_us` includes the projection GEMM the scan's figure leaves to the model's `lstm_ih` GEMM
    (`ih_gemm_us`, timed here too, is added in `scan_plus_ih_us` for a like-for-like figure)."""
    esz = torch.tensor([], dtype=dt).element_size()
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    hw = 224
    for si, stage in enumerate(model.stages):
        depth, C, hid, _ = stage[1].__dict__["_geom"]
        hw //= model.patch_size[si]
        H = W = hw
        rows = batch * H * W
        mod = stage[1].model[0][0].fn[0]
        x = torch.randn((rows, C), device=dev, generator=g).to(dt)
        xp = torch.randn((rows, 16 * hid), device=dev, generator=g).to(dt)
        cat = torch.empty((rows, 4 * hid), dtype=dt, device=dev)
        wih = E.pack_matrix(torch.cat([mod.rnn_v.weight_ih_l0, mod.rnn_v.weight_ih_l0_reverse], 0), dt, dev)
        bih = torch.zeros((8 * hid,), device=dev)
        xph = torch.empty((rows, 8 * hid), dtype=dt, device=dev)
        ih_us = time_steps(lambda _: E.gemm(x, wih, xph, rows, 8 * hid, C, bias=bih), None, reps, 5) * 1e3
        for axis, rn in ((0, "rnn_v"), (1, "rnn_h")):
            rnn = getattr(mod, rn)
            whh = E.pack_lstm_hh(rnn.weight_hh_l0, rnn.weight_hh_l0_reverse, dt, dev)
            L = (H, W)[axis]

            def make(cand):
                r = copy.deepcopy(rnn).to(dev).to(cand)
                seqs = x.view(batch, H, W, C).permute(0, 2, 1, 3).reshape(-1, H, C) if axis == 0 else x.view(-1, W, C)
                seqs = seqs.to(cand).contiguous()
                r(seqs)
                return r, seqs
            edt, note = first_working_dtype(make, dt)
            r, seqs = make(edt)
            scan, ref = [], []
            for _ in range(rounds):                                    # alternating: both sides see the same clocks and the same neighbours
                scan.append(time_steps(lambda _: E.lstm_scan(xp, axis * 8 * hid, whh, cat, axis * 2 * hid, batch, H, W, hid, axis), None, reps, 3) * 1e3)
                ref.append(time_steps(lambda _: r(seqs), None, reps, 3) * 1e3)
            us, rus = statistics.median(scan), statistics.median(ref)
            nbytes = (rows * 10 * hid + whh.numel()) * esz
            rec = {"stage": si + 1, "axis": "vh"[axis], "L": L, "sequences": rows // L, "hid": hid, "calls_per_forward": depth, "us_per_call": round(us, 2),
                   "algorithmic_bytes": nbytes, "effective_TB_per_s": round(nbytes / us * 1e-6, 3), "ih_gemm_us": round(ih_us, 2),
                   "scan_plus_ih_us": round(us + ih_us, 2), "nn_lstm_us": round(rus, 2), "nn_lstm_dtype": NAME[edt],
                   "nn_lstm_over_scan_plus_ih": round(rus / (us + ih_us), 2)}
            if note:
                rec["nn_lstm_note"] = note
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="S,M")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DT))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-in-flight", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sequencer_bench needs a GPU")
    pkg = importlib.import_module("jittor-mlp_amd")
    parallel = importlib.import_module("jittor-mlp_amd.parallel")
    dev = torch.device("cuda:0")
    dt = DT[args.dtype]
    torch.manual_seed(0)
    x = torch.randn((args.batch, 3, 224, 224), device=dev).to(dt)
    lines = []
    for name in args.models.split(","):
        model = pkg.models_pytorch.Sequencer2D(name)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in portable_state_dict(shapes, seed=0).items()}, strict=True)
        model = model.to(dev).eval()
        res = {"model": "Sequencer2D-" + name, "batch": args.batch, "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup}
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
            kt = lstm_alone(pkg.engine, model, args.batch, dt, dev, args.kernel_reps, args.rounds)
            res["lstm_scan"] = kt
            scan_ms = sum(k["calls_per_forward"] * k["us_per_call"] for k in kt) * 1e-3
            res["scan_ms_per_step"] = round(scan_ms, 4)
            res["scan_share_of_step"] = round(scan_ms / ms1, 4)
            res["scan_effective_TB_per_s"] = round(sum(k["calls_per_forward"] * k["algorithmic_bytes"] for k in kt) / scan_ms * 1e-9, 3)
            if not args.no_eager:
                def make(cand):
                    em = copy.deepcopy(model).to(cand)                 # (a copy: the model under test keeps the weights it was timed with)
                    eager_forward(em, x[:2].to(cand))
                    return em
                edt, note = first_working_dtype(make, dt)
                em, xe = make(edt), x.to(edt)
                ref = eager_forward(em, xe).float()
                got = model(x).float()
                res.update({"eager_dtype": NAME[edt], "hip_vs_eager_max_abs": float((got - ref).abs().max()), "eager_max_abs": float(ref.abs().max())})
                if note:
                    res["eager_note"] = note
                mse = time_steps(lambda t: eager_forward(em, t), xe, max(3, args.steps // 4), 2)
                res.update({"eager_ms_per_step": round(mse, 4), "eager_images_per_s": round(args.batch / mse * 1e3, 1),
                            "speedup_vs_eager": round(mse / ms1, 2)})
                del em
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
