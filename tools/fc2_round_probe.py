#!/usr/bin/env python3
"""Round-6 probe for the review's question "where do fc2's 2.9 round-times for 2.3 rounds of work go?".
The persistent tile (algo 14) on the channel-MLP fc2 shape (rows x 768 x 3072, bias + residual + by-product statistics,
the epilogue the model runs), timed in 1.5-second loops with the shader clock / power sampled beside it:
  * the real 50176-row plan, one round of 255 tiles, two rounds, three rounds (256-row tiles only);
  * each of them with the A operand WARM (one buffer, re-read every launch: 133 MB of a single round sits in the 256 MB
    Infinity Cache) and COLD (launches rotate over enough distinct A buffers to exceed it) -- the round-2 numbers that
    contradicted each other (profiles/r02_gemm_power_probe.txt vs r02_gemm_tile_height_calib_v1.txt) differed in exactly that.
usage: python tools/fc2_round_probe.py"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("jittor-mlp_amd")
E, N = pkg.engine, pkg._native
dev = "cuda:0"
dt = torch.bfloat16
Nn, K = 768, 3072


class WS:
    def __init__(self):
        self.t = {}

    def get(self, name, shape, dtype=None, fill=0.0):
        if name not in self.t:
            self.t[name] = torch.zeros(shape, dtype=dtype, device=dev)
        return self.t[name]


def case(M, dbg, nbuf, stats=True, Nn=Nn, K=K, gelu=False, algo=14, ln=False):
    As = [(torch.rand((M, K), device=dev) * 2 - 1).to(dt) for _ in range(nbuf)]
    B = ((torch.rand((Nn, K), device=dev) * 2 - 1) / K ** 0.5).to(dt)
    bias = torch.rand(Nn, device=dev)
    C = torch.zeros((M, Nn), dtype=dt, device=dev)
    R = (torch.rand((M, Nn), device=dev) * 2 - 1).to(dt)
    ws = WS()
    kw = {}
    if not gelu:
        kw.update(R=R, res=N.RES_ADD)
        if stats:
            kw["part"] = (ws, "p")
    if ln:
        kw["ln"] = (torch.rand(M, device=dev) * 0.1, torch.rand(M, device=dev) + 0.5, B.float().sum(dim=1).contiguous())
    state = {"i": 0}

    def f():
        A = As[state["i"] % nbuf]
        state["i"] += 1
        E.gemm(A, B, C, M, Nn, K, bias=bias, act=N.ACT_GELU if gelu else 0, algo=algo, dbg=dbg, **kw)
    return f


def loops():
    import gemm_power_probe as gp     # (prints its own table first: the sensors, fc1 / fc2 / 8192^3 as in round 2)
    print("---- fc2 rounds, warm vs cold A (rows x 768 x 3072, bias + residual + statistics) ----", flush=True)
    for name, M, dbg in (("real plan 50176 rows (588 tiles)", 50176, 0), ("256-row tiles only, 50176 rows", 50176, 16),
                         ("1 round: 255 tiles", 21760, 16), ("2 rounds: 510 tiles", 43520, 16), ("3 rounds: 765 tiles", 65280, 16),
                         ("1 round of 192-row tiles", 85 * 192, 0)):
        for nbuf, label in ((1, "warm"), (max(2, int(np.ceil(700e6 / (M * K * 2)))), "cold")):
            f = case(M, dbg, nbuf)
            gp.loop("%-34s %s x%d" % (name, label, nbuf), f, 2.0 * M * Nn * K)
            del f
            torch.cuda.empty_cache()
    print("---- fc1 on the generated tile (algo 15) and on the persistent tile (14), warm vs cold ----", flush=True)
    for algo in (15, 14):
        for nbuf, label in ((1, "warm"), (4, "cold")):
            f = case(50176, 0, nbuf, Nn=3072, K=768, gelu=True, algo=algo, ln=True)
            gp.loop("fc1 algo %d %s x%d" % (algo, label, nbuf), f, 2.0 * 50176 * 3072 * 768)
            del f
            torch.cuda.empty_cache()


if __name__ == "__main__":
    loops()
