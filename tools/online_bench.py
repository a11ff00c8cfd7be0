"""Latency of the online decoder against the composition of existing calls that computes the same result.

For pushes of 20 and 500 raw samples (1 and 25 windows) in f32 and bf16:
  decoder      OnlineDecoder.push (contrastiveprosthetics_amd/online.py)
  composition  preprocess_segments over the last 2,010 samples (the offline transform restarts its filter from zero on every
               call, so it needs a segment of history) + normalize_ + Engine.encoder_forward(training=False) + z/|z| . E/|E| +
               argmax over the subset
With --adapt the adaptive form (OnlineDecoder(..., adapt=0.01), csrc/online_adapt.cuh) is timed next to the folded decoder
instead of the composition, plus the wall time of calibrate() on 6,000 windows (60 s of stream).
With --streams the multi-stream decoder (MultiStreamDecoder.push, csrc/online_multi.cuh) is timed against S single-stream
decoders pushing one after another, for S in 1, 8, 64, 256 streams of 1 and 25 windows each.
With --streams --adapt the adaptive multi-stream decoder (AdaptiveMultiStreamDecoder.push, csrc/online_multi_adapt.cuh, alpha
0.01) is timed against S OnlineDecoder(adapt=0.01) pushing one after another and against the folded MultiStreamDecoder at
the same S, plus the library part of calibrate(stream) on 6,000 windows (cp_online_multi_adapt_calibrate alone).
Each push is timed from the host with a synchronisation behind it (the latency a control loop sees); kernels per push are
counted with torch.profiler over a few pushes.  One JSON line per case, and a table with --out.

    python tools/online_bench.py --iters 200 --out profiles/online_latency.txt
    python tools/online_bench.py --adapt --iters 200 --out profiles/online_adapt_latency.txt
    python tools/online_bench.py --streams --iters 50 --out profiles/online_multi_latency.txt
    python tools/online_bench.py --streams --adapt --iters 100 --out profiles/online_multi_adapt_latency.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastiveprosthetics_amd import AdaptiveMultiStreamDecoder, MultiStreamDecoder, OnlineDecoder  # noqa: E402
from contrastiveprosthetics_amd.engine import Engine                       # noqa: E402
from contrastiveprosthetics_amd.preprocess import normalize_, preprocess_segments   # noqa: E402


def count_kernels(fn, pushes=5):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(pushes):
            fn()
        torch.cuda.synchronize()
    n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in ev.name
            and "Memset" not in ev.name)
    return n / pushes


def time_pushes(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--adapt", action="store_true", help="adaptive form against the folded decoder, and calibrate()")
    ap.add_argument("--streams", action="store_true", help="multi-stream decoder against S single-stream decoders in turn")
    ap.add_argument("--counts", default="1,8,64,256", help="--streams: stream counts")
    a = ap.parse_args()
    torch.manual_seed(0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    stream = (torch.randn(200000, 12) * 2e-3).cuda()
    mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
    classes = list(range(41))
    table = (e.values.views["glove_net.easy.0.weight"].t() + e.values.views["glove_net.easy.0.bias"]).contiguous()
    tn = table / table.norm(dim=-1, keepdim=True)
    rows = []
    if a.adapt and a.streams:
        return streams_adapt_main(a, e, stream, mean, std, classes)
    if a.adapt:
        return adapt_main(a, e, stream, mean, std, classes)
    if a.streams:
        return streams_main(a, e, stream, mean, std, classes)
    for dtype in ("f32", "bf16"):
        e.dtype = 0 if dtype == "f32" else 1
        e._ws = None                                           # the engine's workspace is carved per dtype
        for n in (20, 500):
            m = n // 20
            dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
            pos = [0]

            def push():
                s = pos[0] % (stream.shape[0] - n)
                pos[0] += n
                return dec.push(stream[s:s + n])

            keep = 2000 - 20 * np.arange(m)[::-1]                    # the last m windows of a 2,010-sample segment

            def compose():
                s = pos[0] % (stream.shape[0] - 2010)
                pos[0] += n
                w = normalize_(preprocess_segments(stream[s:s + 2010][None].contiguous(), keep=keep - 10), mean, std)[0]
                x = torch.zeros(41, 12, device=w.device)                 # the encoder takes whole groups of 41 rows
                x[:m] = w
                z = e.encoder_forward(x, training=False)[:m]
                return ((z / z.norm(dim=-1, keepdim=True)) @ tn.t()).argmax(1)

            for name, fn in (("decoder", push), ("composition", compose)):
                med, p90 = time_pushes(fn, a.iters, a.warmup)
                k = count_kernels(fn)
                r = dict(kind=name, dtype=dtype, samples=n, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                         kernels_per_push=k)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# per-push wall time, host-synchronised (median, p90), and kernels per push (torch.profiler)\n")
            f.write(f"{'kind':<12} {'dtype':<5} {'samples':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8}\n")
            for r in rows:
                f.write(f"{r['kind']:<12} {r['dtype']:<5} {r['samples']:>7} {r['windows']:>7} {r['median_us']:>10.1f} "
                        f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f}\n")


def adapt_main(a, e, stream, mean, std, classes):
    rows, cal = [], []
    for dtype in ("f32", "bf16"):
        for n in (20, 500):
            m = n // 20
            for kind, adapt in (("folded", None), ("adaptive", 0.01)):
                dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype, adapt=adapt)
                pos = [0]

                def push():
                    s = pos[0] % (stream.shape[0] - n)
                    pos[0] += n
                    return dec.push(stream[s:s + n])

                med, p90 = time_pushes(push, a.iters, a.warmup)
                k = count_kernels(push)
                r = dict(kind=kind, dtype=dtype, samples=n, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                         kernels_per_push=k)
                print(json.dumps(r), flush=True)
                rows.append(r)
        dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype, adapt=0.01)
        rec = stream[:20 * 6000 + 10].contiguous()
        dec.calibrate(rec)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            dec.calibrate(rec)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        r = dict(kind="calibrate", dtype=dtype, windows=6000, median_ms=round(float(np.median(ts)) * 1e3, 2))
        print(json.dumps(r), flush=True)
        cal.append(r)
        ts = []
        for _ in range(5):                                     # of which: the windows by the offline transform
            t0 = time.perf_counter()
            dec.calibration_windows(rec)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        r = dict(kind="cal_windows", dtype=dtype, windows=6000, median_ms=round(float(np.median(ts)) * 1e3, 2))
        print(json.dumps(r), flush=True)
        cal.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --adapt --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# per-push wall time, host-synchronised (median, p90), and kernels per push (torch.profiler);\n")
            f.write("# adaptive: OnlineDecoder(..., adapt=0.01), statistics tracked on every window\n")
            f.write(f"{'kind':<12} {'dtype':<5} {'samples':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8}\n")
            for r in rows:
                f.write(f"{r['kind']:<12} {r['dtype']:<5} {r['samples']:>7} {r['windows']:>7} {r['median_us']:>10.1f} "
                        f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f}\n")
            f.write("# calibrate() on 6,000 windows (60 s of stream), host-synchronised wall time, median of 5; cal_windows: the\n"
                    "# part of it that makes the windows with the offline transform (preprocess_segments + normalize_)\n")
            for r in cal:
                f.write(f"{r['kind']:<12} {r['dtype']:<5} {'':>7} {r['windows']:>7} {r['median_ms']:>8.2f} ms\n")


def streams_main(a, e, stream, mean, std, classes):
    rows = []
    counts = [int(x) for x in a.counts.split(",")]
    for dtype in ("f32", "bf16"):
        for S in counts:
            for n in (20, 500):
                m = n // 20
                multi = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                for s in range(S):
                    multi.set_classes(s, classes=classes)
                singles = [OnlineDecoder(e, mean, std, classes=classes, dtype=dtype) for _ in range(S)]
                pos = [0]
                span = stream.shape[0] - S * n

                def batched():
                    base = pos[0] % span
                    pos[0] += S * n
                    return multi.push_packed(stream[base:base + S * n], [n] * S)

                def sequential():
                    base = pos[0] % span
                    pos[0] += S * n
                    return [d.push(stream[base + i * n:base + (i + 1) * n]) for i, d in enumerate(singles)]

                res = {}
                for name, fn in (("batched", batched), ("sequential", sequential)):
                    med, p90 = time_pushes(fn, a.iters, a.warmup)
                    k = count_kernels(fn, pushes=2)
                    res[name] = med
                    r = dict(kind=name, dtype=dtype, streams=S, samples=n, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                             kernels_per_push=k)
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                rows[-2]["speedup"] = rows[-1]["speedup"] = round(res["sequential"] / res["batched"], 2)
                del multi, singles
                torch.cuda.empty_cache()
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --streams --counts {a.counts} --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# one push of S streams x `windows` windows each: batched = MultiStreamDecoder.push_packed, sequential = S\n"
                    "# OnlineDecoder.push one after another; host-synchronised wall time (median, p90), kernels per push\n"
                    "# (torch.profiler: library kernels plus torch's own, e.g. the copy of the counts), speedup = sequential / batched\n")
            f.write(f"{'kind':<11} {'dtype':<5} {'streams':>7} {'samples':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} "
                    f"{'kernels':>8} {'speedup':>8}\n")
            for r in rows:
                f.write(f"{r['kind']:<11} {r['dtype']:<5} {r['streams']:>7} {r['samples']:>7} {r['windows']:>7} {r['median_us']:>10.1f} "
                        f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f} {r['speedup']:>8.2f}\n")


def streams_adapt_main(a, e, stream, mean, std, classes):
    import ctypes as C
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import _calibration_windows
    rows, cal = [], []
    counts = [int(x) for x in a.counts.split(",")]
    for dtype in ("f32", "bf16"):
        for S in counts:
            for n in (20, 500):
                m = n // 20
                multi = AdaptiveMultiStreamDecoder(e, mean, std, S, 0.01, dtype=dtype, max_rows=S * m)
                folded = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                for s in range(S):
                    multi.set_classes(s, classes=classes)
                    folded.set_classes(s, classes=classes)
                singles = [OnlineDecoder(e, mean, std, classes=classes, dtype=dtype, adapt=0.01) for _ in range(S)]
                pos = [0]
                span = stream.shape[0] - S * n

                def batched():
                    base = pos[0] % span
                    pos[0] += S * n
                    return multi.push_packed(stream[base:base + S * n], [n] * S)

                def sequential():
                    base = pos[0] % span
                    pos[0] += S * n
                    return [d.push(stream[base + i * n:base + (i + 1) * n]) for i, d in enumerate(singles)]

                def folded_push():
                    base = pos[0] % span
                    pos[0] += S * n
                    return folded.push_packed(stream[base:base + S * n], [n] * S)

                res = {}
                for name, fn in (("batched", batched), ("sequential", sequential), ("folded", folded_push)):
                    med, p90 = time_pushes(fn, a.iters, a.warmup)
                    k = count_kernels(fn, pushes=2)
                    res[name] = med
                    r = dict(kind=name, dtype=dtype, streams=S, samples=n, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                             kernels_per_push=k)
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                for r in rows[-3:]:
                    r["seq_over_batched"] = round(res["sequential"] / res["batched"], 2)
                    r["batched_over_folded"] = round(res["batched"] / res["folded"], 2)
                del multi, folded, singles
                torch.cuda.empty_cache()
        # the library part of calibrate(stream): cp_online_multi_adapt_calibrate on 6,000 windows, windows and scratch made once
        dec = AdaptiveMultiStreamDecoder(e, mean, std, 64, 0.01, dtype=dtype, max_rows=64)
        rec = stream[:20 * 6000 + 10].contiguous()
        w = _calibration_windows(rec, dec._b, dec._a, dec.phase, dec.mean_std).contiguous()
        scratch = torch.empty(dec.lib.cp_online_adapt_calibrate_scratch_bytes(w.shape[0], dec._cfg.dtype), dtype=torch.uint8,
                              device=dec.device)

        def lib_calibrate():
            _lib.check(dec.lib.cp_online_multi_adapt_calibrate(*dec._args(), 17, w.data_ptr(), w.shape[0], scratch.data_ptr(),
                                                               scratch.numel(), C.c_void_p(dec._stream())), "calibrate")

        lib_calibrate()
        torch.cuda.synchronize()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            lib_calibrate()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        r = dict(kind="calibrate_lib", dtype=dtype, windows=int(w.shape[0]), median_ms=round(float(np.median(ts)) * 1e3, 2))
        print(json.dumps(r), flush=True)
        cal.append(r)
        del dec, scratch
        torch.cuda.empty_cache()
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --streams --adapt --counts {a.counts} --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# one push of S streams x `windows` windows each, alpha 0.01: batched = AdaptiveMultiStreamDecoder.push_packed,\n"
                    "# sequential = S OnlineDecoder(adapt=0.01).push one after another, folded = MultiStreamDecoder.push_packed;\n"
                    "# host-synchronised wall time (median, p90), kernels per push (torch.profiler: library kernels plus torch's own);\n"
                    "# seq/bat = sequential / batched, bat/fold = batched / folded\n")
            f.write(f"{'kind':<11} {'dtype':<5} {'streams':>7} {'samples':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} "
                    f"{'kernels':>8} {'seq/bat':>8} {'bat/fold':>8}\n")
            for r in rows:
                f.write(f"{r['kind']:<11} {r['dtype']:<5} {r['streams']:>7} {r['samples']:>7} {r['windows']:>7} {r['median_us']:>10.1f} "
                        f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f} {r['seq_over_batched']:>8.2f} {r['batched_over_folded']:>8.2f}\n")
            f.write("# cp_online_multi_adapt_calibrate of one stream (of 64) on 6,000 windows, host-synchronised, median of 20\n")
            for r in cal:
                f.write(f"{r['kind']:<13} {r['dtype']:<5} {r['windows']:>7} {r['median_ms']:>8.2f} ms\n")


if __name__ == "__main__":
    main()
