#!/usr/bin/env python3
"""What the gather augmentation (cp_gather_groups_aug) costs and what it buys, on the MI355X:
  (a) the plain against the augmented gather (everything on, with mean_std) at 4096 groups V = 1 and 160 groups V = 25,
      alternating rounds, median of --rounds; and each draw on its own, to say which one costs what;
  (b) the bf16 4096-group training step with and without augmentation, five alternating rounds of --steps steps: the median
      of each round, and the spread (max - min of the five medians) of the plain side;
  (c) load_synthetic trained with and without --aug_shift 1 --aug_gain 0.35, same steps: both models' robustness tables
      (reported, not asserted: synthetic channels, nothing is claimed for real subjects).
usage: python tools/augment_bench.py --out profiles/augment_gather.txt"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from contrastiveprosthetics_amd import results, train
from contrastiveprosthetics_amd.augment import Augment
from contrastiveprosthetics_amd.engine import Engine
from contrastiveprosthetics_amd.load import DB23
from contrastiveprosthetics_amd.utils import TaskWrapper

T = 41
BEST = dict(d_e=16, lr_emg=9.761e-4, reg_emg=7.103e-5, dp_emg=0.0635, lr_glove=2.653e-3, reg_glove=2.840e-6, dp_glove=0.3817)
MEAN_STD = np.concatenate([np.linspace(5, 60, 12), np.linspace(1, 9, 12)]).astype(np.float32)
FULL = dict(shift=(-3, 3), p_drop=0.1, gain_sigma=0.35, amp_sigma=0.2, noise_sigma=0.05, mean_std=MEAN_STD)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def sampler(groups, V, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(T * D * V, 12, generator=g).cuda()
    emg_rand = (torch.rand(T, D, generator=g).argsort(-1) + torch.arange(T).reshape(T, 1) * D).cuda()
    perm = torch.randperm(D, generator=g)[:groups].cuda()
    return table, emg_rand, perm


def gather_ab(e, rounds, reps):
    say("(a) gather: plain against augmented, us per launch (median of %d alternating rounds of %d launches)" % (rounds, reps))
    for groups, V, D in ((4096, 1, 20000), (160, 25, 2000)):
        table, emg_rand, perm = sampler(groups, V, D)
        variants = [("plain", None), ("everything on, mean_std", Augment(seed=1, **FULL))]
        if V == 1:
            variants += [("shift -3..3 only", Augment(shift=(-3, 3))), ("shift + mean_std only", Augment(shift=(-3, 3), mean_std=MEAN_STD)),
                         ("p_drop 0.1 only", Augment(p_drop=0.1)), ("gain_sigma 0.35 only", Augment(gain_sigma=0.35)),
                         ("amp_sigma 0.2 only", Augment(amp_sigma=0.2)), ("noise_sigma 0.05 only", Augment(noise_sigma=0.05))]
        fns = [(name, (lambda a=a: e.gather(table, emg_rand, perm, V, augment=a))) for name, a in variants]
        for _, fn in fns:
            timed(fn, 5)
        samples = {name: [] for name, _ in fns}
        for _ in range(rounds):
            for name, fn in fns:
                samples[name].append(timed(fn, reps))
        nbytes = groups * T * V * 12 * 4 * 2
        say(f"  {groups} groups, V = {V}: {groups * T * V} windows, {nbytes / 1e6:.1f} MB read + written")
        base = float(np.median(samples["plain"]))
        for name, _ in fns:
            m, lo, hi = float(np.median(samples[name])), float(np.percentile(samples[name], 10)), float(np.percentile(samples[name], 90))
            say(f"    {name:26s} {m:7.2f} us  (10-90 %: {lo:6.2f} - {hi:6.2f})  {m - base:+6.2f} us against plain  {nbytes / m / 1e3:7.1f} GB/s")


def step_ab(steps, rounds=5):
    say()
    say("(b) bf16 training step, 4096 groups (167,936 windows), dp_emg 0.0635: ms per step, median of %d steps per round" % steps)
    table, emg_rand, _ = sampler(4096, 1, 20000)
    g = torch.Generator().manual_seed(1)
    perms = [torch.randperm(20000, generator=g)[:4096].cuda() for _ in range(8)]
    labels = torch.arange(T).repeat(4096).cuda()
    e = Engine(adabn=False, dtype="bf16", dp_emg=BEST["dp_emg"], device="cuda", seed=1)
    e.init_parameters(5)
    aug = Augment(seed=1, **FULL)

    def step(i, a):
        x = e.gather(table, emg_rand, perms[i % len(perms)], 1, augment=a)
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(BEST)

    for i in range(5):
        step(i, None)
        step(i, aug)
    torch.cuda.synchronize()
    med = {"plain": [], "augmented": []}
    for r in range(rounds):
        for name, a in (("plain", None), ("augmented", aug)):
            ts = []
            for i in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(i, a)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            med[name].append(float(np.median(ts)))
    for name in med:
        say(f"    {name:10s} " + "  ".join(f"{m:.4f}" for m in med[name]) + f"   median {np.median(med[name]):.4f}")
    spread = max(med["plain"]) - min(med["plain"])
    diff = float(np.median(med["augmented"]) - np.median(med["plain"]))
    say(f"    spread of the plain side (max - min of its medians): {spread:.4f} ms;  augmented - plain: {diff:+.4f} ms")
    say("    -> " + ("inside the plain side's spread" if diff <= spread else
                    "outside the plain side's spread: (a) lists what each draw adds to the gather's launch"))


def train_ab(epochs, batch):
    say()
    say(f"(c) load_synthetic, {epochs} epochs at batch {batch}, bf16, with and without --aug_shift 1 --aug_gain 0.35: robustness of both")
    shifts, dead = list(range(-3, 4)), [None] + list(range(12))
    for name, extra in (("no augmentation", []), ("--aug_shift 1 --aug_gain 0.35", ["--aug_shift", "1", "--aug_gain", "0.35"])):
        argv = ["--final_epochs", str(epochs), "--batch_size", str(batch), "--synthetic", "--dtype", "bf16", "--crossval_load"] + extra
        train.args = train.build_parser().parse_args(argv)
        results.args = results.build_parser().parse_args(["--batch_size", "8", "--synthetic", "--dtype", "bf16"])
        torch.manual_seed(42)
        ds = DB23()
        ds.load_synthetic()
        ds = TaskWrapper(ds)
        params = dict(BEST, epochs=epochs)
        (loss_val, acc_val), model = train.train_loop(ds, params, checkpoint=False, annealing=True, verbose=False)
        torch.manual_seed(7)
        tab = results.robustness(model, ds, shifts, dead)
        say(f"  {name}: validation loss {loss_val:.4f}, accuracy {acc_val:.4f}")
        for which, what in ((0, "per-window accuracy"), (1, "voted accuracy (25 samples)")):
            say(f"    {what}: rows = ring shift, columns = dead channel")
            say("    shift " + " ".join(f"{'none' if d is None else d:>6}" for d in dead))
            for s, row in zip(shifts, tab[:, :, which]):
                say(f"    {s:5d} " + " ".join(f"{v:6.4f}" for v in row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed sample of (a)")
    ap.add_argument("--steps", type=int, default=20, help="steps per round of (b)")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    say("tools/augment_bench.py on " + torch.cuda.get_device_name(0))
    e = Engine(adabn=False, dtype="bf16", dp_emg=0.0, device="cuda", seed=1)
    gather_ab(e, a.rounds, a.reps)
    step_ab(a.steps)
    train_ab(a.epochs, a.batch)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
