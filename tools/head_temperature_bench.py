#!/usr/bin/env python3
"""Time of the contrastive head on its own (head_kernel + reduce_rows_kernel + head_finalize_kernel, gradients on) without and with
the learnable temperature (cp_head against cp_head_temp) at 8 and 4096 groups, f32 / bf16 / 8-bit logits, in alternating rounds:
off, on, off, on, ... so that clock drift lands on both alike.  Prints the median of the rounds and their spread.
usage: python tools/head_temperature_bench.py [> profiles/head_temperature.txt]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from contrastiveprosthetics_amd.engine import Engine

T, ROUNDS, CALLS = 41, 9, 50


def timed(e, z, labels):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        e.head(z, labels, 1, want_grad=True)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


print("head alone, gradients on: microseconds per call (median of %d alternating rounds of %d calls; min .. max)" % (ROUNDS, CALLS))
for dtype in ("f32", "bf16", "fp8"):
    engines = {"off": Engine(adabn=True, dtype=dtype, device="cuda", seed=1),
               "on": Engine(adabn=True, dtype=dtype, device="cuda", seed=1, temperature=1 / 0.07)}
    for e in engines.values():
        e.init_parameters(5)
    for groups in (8, 4096):
        g = torch.Generator().manual_seed(groups)
        z = torch.randn(groups * T, 16, generator=g).cuda()
        labels = torch.arange(T).repeat(groups).cuda()
        for e in engines.values():
            for _ in range(5):
                e.head(z, labels, 1, want_grad=True)
        torch.cuda.synchronize()
        t = {"off": [], "on": []}
        for _ in range(ROUNDS):
            for k in ("off", "on"):
                t[k].append(timed(engines[k], z, labels))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{dtype:5s} {groups:5d} groups | off {med['off']:7.2f} ({min(t['off']):.2f} .. {max(t['off']):.2f})"
              f" | on {med['on']:7.2f} ({min(t['on']):.2f} .. {max(t['on']):.2f}) | on - off {med['on'] - med['off']:+6.2f} us"
              f" ({100 * (med['on'] / med['off'] - 1):+.1f} %)")
