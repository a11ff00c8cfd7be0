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
With --enroll class enrolment (OnlineDecoder.enroll, csrc/online_enroll.cuh) is measured: (a) enroll() of 41 classes x 500
windows, split into windows / accumulate / table, next to the same table composed from the offline windows, the engine's
eval forward and index_add_; (b) recording_windows against the offline windows on a 60 s recording; (c) on synthetic people
(a channel-amplitude pattern per class times a gain pattern per person) the accuracy of the model's one-hot rows and of
enrolled rows on a held-out recording of a person the model has not seen.
With --gate the command gate (CommandGate.push, csrc/online_gate.cuh) is timed against the ungated decoder.push(
return_logits=True) in the same run: 1 and 25 windows on OnlineDecoder and 256 streams x 1 window on MultiStreamDecoder, plus
the gate's launch alone (CommandGate.apply on the logits of one push).
With --gate-sweep the gate sweep (sweep_gate, csrc/online_gate.cuh og_sweep_kernel) is timed against the way without it: G
CommandGate.apply calls one after another over the same logits plus the copy of each one's commands to the host; synthetic
cued logits of 8 classes, 6,000 and 60,000 windows, G = 64, 256 and 1,024 configs, every timed case under a time limit of its own.
With --subset-sweep the grasp-set search's sweep (sweep_subsets, csrc/online_subsets.cuh) is timed on synthetic cued logits of
41 classes, 6,000 and 20,500 windows, G = 64, 1,024, 10,660 (all triples) and 112,750 (all pairs, triples and quadruples)
subsets at vote 25; for G = 64 the same scores are also computed the way without it (per subset a row and column select plus
a one-config sweep_gate), must be equal, and the ratio of the two times is stated.
With --sequence the sequence decoder (SequenceGate.push, csrc/online_sequence.cuh) at lag 0 and lag 63 is timed next to the
ungated and the CommandGate push of the same run: 1 and 25 windows on OnlineDecoder, 256 streams x 1 window, f32 and bf16.
With --sequence-sweep sweep_sequence runs 4,096 configs over 14,514 windows at lag 0 and at lag 63 next to the numpy definition
for 16 of them (scaled up; their scores must be equal), and the best config of sweep_gate and of sweep_sequence under pick_gate's
default limits are set side by side on one synthetic recording of 41 classes.
With --drive the grasp drive (GraspDrive.push, csrc/online_drive.cuh) is timed behind gate-wrapped decoders next to the gate
itself in the same run: ungated, gated and driven pushes of 1 and 25 windows on OnlineDecoder and of 256 streams x 1 window on
MultiStreamDecoder, plus the drive's launch alone (GraspDrive.apply on the windows and commands of one push).  A driven push
must launch one kernel more than a gated one.
With --map-sweep the electrode-map sweep (score_channel_maps, csrc/online_maps.cuh) is measured: (a) 16 and 64 maps over a
recording of 41 classes x 500 windows in f32 and bf16 against the way without it, a decoder that is reset, given each map in
turn and pushed the recording in 256-window pushes, its pred and voted copied to the host and counted there (both must give
the same counts); (b) a mapped against an unmapped push of 1 and 25 windows on OnlineDecoder and of 256 streams x 1 window
on MultiStreamDecoder, alternating in the same run, with the run-to-run spread of the unmapped medians next to the difference.
With --finetune head fine-tuning (OnlineDecoder.finetune, csrc/online_finetune.cuh) is measured: (a) at 41 classes x 500
windows in f32 and bf16 the embedding pass, one step (median run of 100 steps), the bytes a step must move and the same step
composed from torch ops on the same u; (c) on the synthetic people of --enroll the held-out accuracy of one-hot rows, enrolled
rows and the fine-tuned head.
With --track the prototype tracker (track.PrototypeTracker.push, csrc/online_track.cuh) is timed against the plain decoder.push
in the same run: 1 and 25 windows on OnlineDecoder and 256 streams x 1 window on MultiStreamDecoder, a push that only gives out
its embeddings, and the stage's launch alone (PrototypeTracker.apply on the embeddings of one push).  With --track-sweep the
tracker sweep (track.sweep_tracker, ot_sweep_kernel) is timed on the synthetic drifting stream of 41 classes at 2,400 and 24,000
rows for 64, 1,024 and 16,384 settings, next to the numpy definition for one setting.  Both together write one file.
With --holdout held-out enrolment scoring (holdout.score_plans, csrc/online_holdout.cuh) is timed on a synthetic person of 41
classes x 6 repetitions (about 14,500 windows): the embedding pass, the 30 learning-curve plans and a 4,096-plan grid, the numpy
definition for the 30 plans, the host loop it replaces (masked enroll + set_classes + push per leave-one-out fold) and
score_enrolment as a whole; the loop's hits per fold are written next to the sweep's.
With --prototypes posture prototypes (prototypes.fit_prototypes and PostureRows, csrc/online_prototypes.cuh) are timed: the fit
of the synthetic posture person of 41 classes (about 14,500 windows, 10 Lloyd rounds) with two rows per class for the first 23
classes and with four rows for the first 7 (the sum stays at 64 rows or below), next to fit_reference on the host, and the
per-push latency and kernels of OnlineDecoder.push with logits against PostureRows.push behind it at 1 and 25 windows.
With --metric the user metric (metric.fit_metric, Metric.apply, pick_shrink and MetricRows, csrc/online_metric.cuh) is timed on
the synthetic person of 41 classes (about 14,500 windows, 6 repetitions): the fit for 5 shrink values next to fit_reference on
the host, the transform of the recording, pick_shrink over the 6 folds, and the per-push latency and kernels of
OnlineDecoder.push with logits against MetricRows.push behind it at 1 and 25 windows.
With --readout the closed-form head fit (readout.moments, solve, apply and pick_ridge_inputs, csrc/online_readout.cuh) is timed
on the synthetic person of 41 classes (14,514 windows of 512 tail inputs, 6 repetitions): the moments of the 6 repetitions, the
solve for 1, 8 and 48 plans, the apply of 24 projections and the ridge pick over 6 folds x 4 ridges, next to numpy's
X.T @ diag(w) @ X and numpy.linalg.solve on the host.
With --stream-projections the pushes of MultiStreamDecoder and AdaptiveMultiStreamDecoder built with stream_projections=True
(csrc/online_projections.cuh) are timed with no slot set and with every slot set, next to the same decoder built without the
option, alternating in the same run: 1, 16 and 256 streams of 1 and 25 windows each in f32 and bf16, with the run-to-run spread
of the option-off medians and the kernels per push of all three.
Each push is timed from the host with a synchronisation behind it (the latency a control loop sees); kernels per push are
counted with torch.profiler over a few pushes.  One JSON line per case, and a table with --out.

    python tools/online_bench.py --iters 200 --out profiles/online_latency.txt
    python tools/online_bench.py --adapt --iters 200 --out profiles/online_adapt_latency.txt
    python tools/online_bench.py --streams --iters 50 --out profiles/online_multi_latency.txt
    python tools/online_bench.py --streams --adapt --iters 100 --out profiles/online_multi_adapt_latency.txt
    python tools/online_bench.py --enroll --iters 10 --out profiles/online_enroll.txt
    python tools/online_bench.py --gate --iters 200 --out profiles/online_gate_latency.txt
    python tools/online_bench.py --drive --iters 200 --out profiles/online_drive_latency.txt
    python tools/online_bench.py --gate-sweep --iters 20 --out profiles/online_gate_sweep.txt
    python tools/online_bench.py --sequence --sequence-sweep --iters 200 --out profiles/online_sequence.txt
    python tools/online_bench.py --subset-sweep --iters 20 --out profiles/online_subset_sweep.txt
    python tools/online_bench.py --map-sweep --iters 5 --out profiles/online_map_sweep.txt
    python tools/online_bench.py --finetune --iters 10 --out profiles/online_finetune.txt
    python tools/online_bench.py --realign --iters 20 --out profiles/online_realign.txt
    python tools/online_bench.py --track --track-sweep --iters 100 --out profiles/online_track.txt
    python tools/online_bench.py --holdout --iters 10 --out profiles/online_holdout.txt
    python tools/online_bench.py --prototypes --iters 200 --out profiles/online_prototypes.txt
    python tools/online_bench.py --metric --iters 200 --out profiles/online_metric.txt
    python tools/online_bench.py --readout --iters 200 --out profiles/online_readout.txt
    python tools/online_bench.py --stream-projections --iters 50 --out profiles/online_stream_projections.txt
    python tools/online_bench.py --kinematics --iters 100 --out profiles/online_kinematics.txt
    python tools/online_bench.py --kalman --iters 100 --out profiles/online_kalman.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from contrastiveprosthetics_amd import (AdaptiveMultiStreamDecoder, CommandGate, GraspDrive, MultiStreamDecoder,  # noqa: E402
                                        OnlineDecoder)
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
    ap.add_argument("--enroll", action="store_true", help="class enrolment: time, one-pass windows, accuracy on a synthetic person")
    ap.add_argument("--gate", action="store_true", help="the command gate against the ungated push with logits")
    ap.add_argument("--drive", action="store_true", help="the grasp drive behind gate-wrapped decoders, next to the gate's own cost")
    ap.add_argument("--gate-sweep", action="store_true", help="sweep_gate against G CommandGate.apply calls in turn")
    ap.add_argument("--sequence", action="store_true", help="the sequence decoder's push next to the ungated and the gated push")
    ap.add_argument("--sequence-sweep", action="store_true", help="sweep_sequence against the numpy definition, and its best config "
                    "next to sweep_gate's on one recording")
    ap.add_argument("--subset-sweep", action="store_true", help="sweep_subsets, and for 64 subsets a select + sweep_gate per subset")
    ap.add_argument("--map-sweep", action="store_true", help="score_channel_maps against a reset / set_channel_map / push loop, and "
                    "a mapped against an unmapped push")
    ap.add_argument("--case-seconds", type=float, default=150.0, help="--gate-sweep: time limit of each timed case")
    ap.add_argument("--finetune", action="store_true", help="head fine-tuning: embedding pass, step against torch ops, accuracy on a "
                    "synthetic person")
    ap.add_argument("--realign", action="store_true", help="cue realignment: realign_cues against the definition, and enroll + "
                    "finetune on the raw cue, the realigned labels and the planted truth")
    ap.add_argument("--track", action="store_true", help="the prototype tracker against the plain push, and its launch alone")
    ap.add_argument("--track-sweep", action="store_true", help="sweep_tracker over a synthetic drifting stream, next to the definition")
    ap.add_argument("--holdout", action="store_true", help="held-out enrolment scoring: score_plans against the definition and against "
                    "a masked enroll + set_classes + push loop per fold")
    ap.add_argument("--prototypes", action="store_true", help="posture prototypes: fit_prototypes against the definition, and the "
                    "push with and without PostureRows behind it")
    ap.add_argument("--metric", action="store_true", help="the user metric: fit_metric against the definition, apply, pick_shrink, and "
                    "the push with and without MetricRows behind it")
    ap.add_argument("--readout", action="store_true", help="the closed-form head fit: moments, solve for 1 / 8 / 48 plans and pick_ridge "
                    "over 6 folds, next to numpy's X.T @ X and numpy.linalg.solve")
    ap.add_argument("--stream-projections", action="store_true", help="the multi-stream pushes with stream_projections=True, no slot "
                    "set and every slot set, next to the same decoder built without the option")
    ap.add_argument("--kinematics", action="store_true", help="joint-angle decoding: the push with and without JointAngles behind it at "
                    "1, 16 and 256 streams, and moments, solve, apply and score of a 14,514-window recording x 20 joints")
    ap.add_argument("--kalman", action="store_true", help="the pose filter: the push bare, with JointAngles and with PoseFilter behind it "
                    "at 1, 16 and 256 streams, and cross-fit, moments, design, sweep and pick_filter of a 14,514-window recording x 20 joints")
    a = ap.parse_args()
    if a.readout:
        return readout_main(a)
    if a.metric:
        return metric_main(a)
    if a.prototypes:
        return prototypes_main(a)
    if a.holdout:
        return holdout_main(a)
    if a.track or a.track_sweep:
        return track_main(a)
    if a.enroll:
        return enroll_main(a)
    if a.realign:
        return realign_main(a)
    if a.finetune:
        return finetune_main(a)
    if a.gate_sweep:
        return gate_sweep_main(a)
    if a.subset_sweep:
        return subset_sweep_main(a)
    if a.map_sweep:
        return map_sweep_main(a)
    torch.manual_seed(0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    stream = (torch.randn(200000, 12) * 2e-3).cuda()
    mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
    classes = list(range(41))
    table = (e.values.views["glove_net.easy.0.weight"].t() + e.values.views["glove_net.easy.0.bias"]).contiguous()
    tn = table / table.norm(dim=-1, keepdim=True)
    rows = []
    if a.sequence or a.sequence_sweep:
        return sequence_main(a, e, stream, mean, std, classes)
    if a.stream_projections:
        return stream_projections_main(a, e, stream, mean, std, classes)
    if a.gate:
        return gate_main(a, e, stream, mean, std, classes)
    if a.drive:
        return drive_main(a, e, stream, mean, std, classes)
    if a.kalman:
        return kalman_main(a, e, stream, mean, std, classes)
    if a.kinematics:
        return kinematics_main(a, e, stream, mean, std, classes)
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


def _cue_recording(rng, pattern, gain, windows_per_class, order):
    """a cued recording of one synthetic person: per class a block of 20 * windows_per_class + 10 samples of noise with the
    class's channel amplitudes times the person's channel gains, 100 unlabelled samples in between"""
    raws, labs = [], []
    for c in order:
        n = 20 * windows_per_class + 10
        raws += [rng.standard_normal((100, 12)) * gain, rng.standard_normal((n, 12)) * pattern[c] * gain]
        labs += [np.full(100, -1), np.full(n, c)]
    raw = torch.from_numpy((np.concatenate(raws) * 2e-3).astype(np.float32)).cuda()
    return raw, np.concatenate(labs).astype(np.int64)


def _wall(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def enroll_main(a):
    import ctypes as C
    from contrastiveprosthetics_amd.online import _calibration_windows, recording_windows, window_labels
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    classes = list(range(41))
    pattern = rng.uniform(0.4, 3.0, (41, 12))
    people = np.exp(rng.normal(0.0, 0.35, (10, 12)))              # per-person channel gains; person 9 is never trained on
    params = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    raw0, _ = _cue_recording(rng, pattern, people[0], 30, classes)
    ident = torch.stack([torch.zeros(12), torch.ones(12)]).cuda()  # (r - 0) / 1: the RMS windows as they are
    w0 = recording_windows(raw0, ident)
    mean, std = w0.mean(0), w0.std(0)
    lines = []

    def out(r):
        print(json.dumps(r), flush=True)
        lines.append(r)

    # (c) first, so that (a) and (b) run on the trained model: train on people 0..8, one window per class and group
    probe = OnlineDecoder(e, mean, std, classes=classes)
    train = []
    for p in range(9):
        raw, lab = _cue_recording(rng, pattern, people[p], 40, classes)
        w = recording_windows(raw, probe.mean_std, probe._b, probe._a, 0)
        wl = window_labels(lab, 0)
        train.append(torch.stack([w[torch.as_tensor(np.nonzero(wl == c)[0][:40]).cuda()] for c in classes]))     # (41, 40, 12)
    train = torch.stack(train)                                     # (9, 41, 40, 12)
    labels = torch.arange(41).repeat(8).cuda()
    for step in range(400):
        pi = torch.randint(0, 9, (8,))
        wi = torch.randint(0, 40, (8, 41))
        x = torch.stack([train[pi[g], torch.arange(41), wi[g]] for g in range(8)]).reshape(-1, 12).contiguous()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(params)
    torch.cuda.synchronize()
    rawE, labE = _cue_recording(rng, pattern, people[9], 100, rng.permutation(41))
    rawT, labT = _cue_recording(rng, pattern, people[9], 100, rng.permutation(41))
    wlT = window_labels(labT, 0)
    for dtype in ("f32", "bf16"):
        dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
        acc = {}
        for name in ("one-hot rows", "enrolled rows"):
            if name == "enrolled rows":
                dec.enroll(rawE, labE)
            dec.reset()
            pred, voted = (t.cpu().numpy() for t in dec.push(rawT))
            ok = wlT >= 0
            acc[name] = (float((pred[ok] == wlT[ok]).mean()), float((voted[ok] == wlT[ok]).mean()))
        out(dict(part="c", dtype=dtype, windows=int((wlT >= 0).sum()), acc_onehot=round(acc["one-hot rows"][0], 4),
                 acc_onehot_voted=round(acc["one-hot rows"][1], 4), acc_enrolled=round(acc["enrolled rows"][0], 4),
                 acc_enrolled_voted=round(acc["enrolled rows"][1], 4)))

    # (a) 41 classes x 500 windows
    raw, lab = _cue_recording(rng, pattern, people[9], 500, classes)
    wl = window_labels(lab, 0)
    keep = torch.as_tensor(np.nonzero(wl >= 0)[0]).cuda()
    slots_np = wl[wl >= 0]
    slots = torch.as_tensor(slots_np.astype(np.int32)).cuda()
    for dtype in ("f32", "bf16"):
        dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
        prior = dec.class_table()[0]
        lib = dec.lib

        def whole():
            dec.enroll_reset()
            dec.enroll(raw, lab)

        def windows():
            return recording_windows(raw, dec.mean_std, dec._b, dec._a, 0)[keep].contiguous()

        w = windows()
        accb = torch.zeros(64, 17, dtype=torch.float64, device="cuda")
        scratch = torch.empty(lib.cp_online_enroll_scratch_bytes(w.shape[0], dec._cfg.dtype), dtype=torch.uint8, device="cuda")
        tab = torch.empty_like(prior)
        st = torch.cuda.current_stream().cuda_stream

        def accumulate():
            lib.cp_online_enroll(C.byref(dec._cfg), dec.ws.data_ptr(), dec.ws.numel(), w.data_ptr(), w.shape[0], slots.data_ptr(), 41,
                                 accb.data_ptr(), scratch.data_ptr(), scratch.numel(), st)

        def table():
            lib.cp_online_enroll_table(accb.data_ptr(), 41, prior.data_ptr(), C.c_double(1.0), 25, tab.data_ptr(), st)

        def composed():
            wc = _calibration_windows(raw, dec._b, dec._a, 0, dec.mean_std)[keep]
            x = torch.zeros((wc.shape[0] + 40) // 41 * 41, 12, device="cuda")
            x[:wc.shape[0]] = wc
            z = e.encoder_forward(x, training=False)[:wc.shape[0]].double()
            zn = z / z.norm(dim=-1, keepdim=True)
            S = torch.zeros(41, 16, dtype=torch.float64, device="cuda").index_add_(0, slots.long(), zn)
            return (S / S.norm(dim=-1, keepdim=True)).float()

        e.dtype = 0 if dtype == "f32" else 1
        e._ws = None                                           # the engine's workspace is carved per dtype
        out(dict(part="a", dtype=dtype, windows=int(w.shape[0]), enroll_ms=round(_wall(whole, a.iters), 3),
                 windows_ms=round(_wall(windows, a.iters), 3), accumulate_ms=round(_wall(accumulate, a.iters), 3),
                 table_ms=round(_wall(table, a.iters), 3), composed_ms=round(_wall(composed, max(2, a.iters // 3)), 3)))
    e.dtype = 0
    e._ws = None

    # (b) a 60 s recording
    raw60 = (torch.randn(120000, 12) * 2e-3).cuda()
    one = _wall(lambda: recording_windows(raw60, probe.mean_std, probe._b, probe._a, 0), a.iters)
    off = _wall(lambda: _calibration_windows(raw60, probe._b, probe._a, 0, probe.mean_std), max(2, a.iters // 3))
    w_one = recording_windows(raw60, probe.mean_std, probe._b, probe._a, 0)
    w_off = _calibration_windows(raw60, probe._b, probe._a, 0, probe.mean_std)
    push = OnlineDecoder(e, mean, std, classes=classes).push(raw60, return_windows=True)[2]
    out(dict(part="b", samples=120000, recording_windows_ms=round(one, 3), calibration_windows_ms=round(off, 3),
             ratio=round(off / one, 1), equal_to_push=torch.equal(w_one, push), equal_to_offline=torch.equal(w_one, w_off)))
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --enroll --iters {a.iters} on {dev}\n")
            f.write("# wall time, host-synchronised, median.  (a) enroll() of 41 classes x 500 windows and its parts, next to the same\n"
                    "# table from _calibration_windows + Engine.encoder_forward(training=False) + index_add_;  (b) one-pass windows\n"
                    "# against the offline windows on 60 s;  (c) accuracy on a held-out recording of a synthetic person the model was\n"
                    "# not trained on (class amplitude pattern x per-person channel gains; 400 training steps on nine other people),\n"
                    "# per window and voted over 25 windows\n")
            for r in lines:
                f.write(json.dumps(r) + "\n")


def _torch_step(u, uf, st, slots, wi, scale, lr, lr_rows, t):
    """one fine-tuning step composed from torch ops on the device, on the same u: the baseline of finetune_main.  st: masters
    W, b, E and their moments (f32); the forward multiplies u by W rounded to u's dtype, dW takes dz in f32 and u widened."""
    W, b, E = st["W"], st["b"], st["E"]
    z = (u @ W.to(u.dtype).t()).float() + b
    zl = z.norm(dim=1, keepdim=True)
    zn = z / zl
    el = E.norm(dim=1, keepdim=True)
    en = E / el
    l = scale * (zn @ en.t())
    lse = torch.logsumexp(l, dim=1)
    loss = (wi * (lse - l.gather(1, slots[:, None])[:, 0])).sum()
    g = torch.softmax(l, dim=1)
    g.scatter_add_(1, slots[:, None], torch.full_like(lse, -1.0)[:, None])
    g *= (wi * scale)[:, None]
    dzn = g @ en
    dz = (dzn - zn * (zn * dzn).sum(1, keepdim=True)) / zl
    den = g.t() @ zn
    grads = dict(W=dz.t() @ uf, b=dz.sum(0), E=(den - en * (en * den).sum(1, keepdim=True)) / el)
    bc1, bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
    for k, rate in (("W", lr), ("b", lr), ("E", lr_rows)):
        m, v = st["m" + k], st["v" + k]
        m.mul_(0.9).add_(grads[k], alpha=0.1)
        v.mul_(0.999).addcmul_(grads[k], grads[k], value=0.001)
        st[k].addcdiv_(m, v.sqrt().div_(bc2 ** 0.5).add_(1e-8), value=-rate / bc1)
    return loss


def finetune_main(a):
    """--finetune: (a) the embedding pass and the step of OnlineDecoder.finetune at 41 classes x 500 windows against the same
    step composed from torch ops on the same u; (c) held-out accuracy of one-hot rows, enrolled rows and the fine-tuned head on
    the synthetic people of --enroll."""
    import ctypes as C
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.online import recording_windows, window_labels
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    classes = list(range(41))
    pattern = rng.uniform(0.4, 3.0, (41, 12))
    people = np.exp(rng.normal(0.0, 0.35, (10, 12)))              # per-person channel gains; person 9 is never trained on
    params = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    raw0, _ = _cue_recording(rng, pattern, people[0], 30, classes)
    ident = torch.stack([torch.zeros(12), torch.ones(12)]).cuda()
    w0 = recording_windows(raw0, ident)
    mean, std = w0.mean(0), w0.std(0)
    lines = []

    def out(r):
        print(json.dumps(r), flush=True)
        lines.append(r)

    # (c) the people, the training and the two recordings of person 9 are those of --enroll, draw for draw
    probe = OnlineDecoder(e, mean, std, classes=classes)
    train = []
    for p in range(9):
        raw, lab = _cue_recording(rng, pattern, people[p], 40, classes)
        w = recording_windows(raw, probe.mean_std, probe._b, probe._a, 0)
        wl = window_labels(lab, 0)
        train.append(torch.stack([w[torch.as_tensor(np.nonzero(wl == c)[0][:40]).cuda()] for c in classes]))
    train = torch.stack(train)
    labels = torch.arange(41).repeat(8).cuda()
    for step in range(400):
        pi = torch.randint(0, 9, (8,))
        wi = torch.randint(0, 40, (8, 41))
        x = torch.stack([train[pi[g], torch.arange(41), wi[g]] for g in range(8)]).reshape(-1, 12).contiguous()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(params)
    torch.cuda.synchronize()
    rawE, labE = _cue_recording(rng, pattern, people[9], 100, rng.permutation(41))
    rawT, labT = _cue_recording(rng, pattern, people[9], 100, rng.permutation(41))
    wlT = window_labels(labT, 0)
    ok = wlT >= 0
    tune = dict(steps=200, lr=1e-3, lr_rows=1e-2, scale=10.0)
    for dtype in ("f32", "bf16"):
        r = dict(part="c", dtype=dtype, windows=int(ok.sum()), **tune)
        for name in ("onehot", "enrolled", "finetuned", "enrolled_finetuned"):
            dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
            if name.startswith("enrolled"):
                dec.enroll(rawE, labE)
            if name.endswith("finetuned"):
                dec.finetune(rawE, labE, **tune)
            pred, voted = (t.cpu().numpy() for t in dec.push(rawT))
            r["acc_" + name] = round(float((pred[ok] == wlT[ok]).mean()), 4)
            r["acc_" + name + "_voted"] = round(float((voted[ok] == wlT[ok]).mean()), 4)
        out(r)

    # (a) 41 classes x 500 windows
    raw, lab = _cue_recording(rng, pattern, people[9], 500, classes)
    wl = window_labels(lab, 0)
    keep = torch.as_tensor(np.nonzero(wl >= 0)[0]).cuda()
    slots = torch.as_tensor(wl[wl >= 0].astype(np.int32)).cuda()
    n, steps = int(keep.numel()), 100
    st = torch.cuda.current_stream().cuda_stream
    for dtype in ("f32", "bf16"):
        dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
        lib = dec.lib
        w = recording_windows(raw, dec.mean_std, dec._b, dec._a, 0)[keep].contiguous()
        tdt = torch.float32 if dtype == "f32" else torch.bfloat16
        u = torch.empty(n, 512, dtype=tdt, device="cuda")
        scratch = torch.empty(lib.cp_online_enroll_scratch_bytes(n, dec._cfg.dtype), dtype=torch.uint8, device="cuda")
        embed = lambda: dec._tail_inputs_call(None, w.data_ptr(), n, u.data_ptr(), scratch.data_ptr(), scratch.numel())
        embed_ms = _wall(embed, a.iters)
        W, b = dec.projection()
        E = dec.class_table()[0]
        state = torch.zeros(lib.cp_online_finetune_state_bytes(n, 41), dtype=torch.uint8, device="cuda")
        loss = torch.empty(steps, dtype=torch.float64, device="cuda")

        def init():
            _lib.check(lib.cp_online_finetune_init(state.data_ptr(), state.numel(), dec._cfg.dtype, W.data_ptr(), b.data_ptr(), E.data_ptr(),
                                                   slots.data_ptr(), n, 41, 1, st), "cp_online_finetune_init")

        def run():
            _lib.check(lib.cp_online_finetune_steps(C.byref(dec._cfg), state.data_ptr(), state.numel(), u.data_ptr(), n, 41, steps, 1e-3,
                                                    1e-2, 10.0, 0.0, 3, loss.data_ptr(), st), "cp_online_finetune_steps")

        init()
        step_us = _wall(run, a.iters) * 1e3 / steps
        init()
        run()
        torch.cuda.synchronize()
        first, last = float(loss[0]), float(loss[-1])
        counts = torch.bincount(slots.long(), minlength=41).float()
        wi = (1.0 / (41 * counts))[slots.long()]
        uf = u.float()
        ts = {}

        def torch_run():
            ts.update(W=W.clone(), b=b.clone(), E=E.clone())
            for k in ("W", "b", "E"):
                ts["m" + k], ts["v" + k] = torch.zeros_like(ts[k]), torch.zeros_like(ts[k])
            for t in range(1, steps + 1):
                ts["loss"] = _torch_step(u, uf, ts, slots.long(), wi, 10.0, 1e-3, 1e-2, t)

        torch_us = _wall(torch_run, max(2, a.iters // 2)) * 1e3 / steps
        chunks = (n + _lib.CP_ONLINE_FINETUNE_CHUNK - 1) // _lib.CP_ONLINE_FINETUNE_CHUNK
        slab_bytes = chunks * (8208 + 64 * 16 + 16) * 4
        moved = n * 512 * u.element_size() + 2 * slab_bytes          # u read once, the slabs written and read
        out(dict(part="a", dtype=dtype, windows=n, chunks=chunks, embed_ms=round(embed_ms, 3), step_us=round(step_us, 2),
                 torch_step_us=round(torch_us, 2), ratio=round(torch_us / step_us, 2), bytes_per_step=moved,
                 gb_per_s=round(moved / step_us / 1e3, 1), loss_first=round(first, 5), loss_last=round(last, 5),
                 torch_loss_last=round(float(ts["loss"]), 5)))
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --finetune --iters {a.iters} on {dev}\n")
            f.write("# wall time, host-synchronised, median.  (a) 41 classes x 500 windows: the embedding pass (cp_online_tail_inputs),\n"
                    "# one step of cp_online_finetune_steps (median run of 100 steps / 100), the same step composed from torch ops on\n"
                    "# the same u, and the bytes a step must move (u once, the slabs written and read);  (c) accuracy, per window and\n"
                    "# voted over 25 windows, on a held-out recording of a synthetic person the model was not trained on (the\n"
                    "# people, training and recordings of --enroll): one-hot rows, enrolled rows, the head fine-tuned from either\n")
            for r in lines:
                f.write(json.dumps(r) + "\n")


def _lagged_recording(rng, pattern, gain, cue_windows, rest_windows, order, rest_label, rest_level=0.25):
    """A cued recording of one synthetic person who follows the cue late: per class a cue of `cue_windows` windows and then
    `rest_windows` of rest; the class's amplitudes start a drawn 20..80 windows behind the cue's start and end a drawn -20..+60
    windows behind its end, and everything else is noise at `rest_level` times the person's channel gains.  Returns raw (n, 12)
    on the GPU, the cue and the planted truth as one label per sample (`rest_label` between movements), and the planted
    (onset, offset) of every cue in windows."""
    n = 20 * (rest_windows + len(order) * (cue_windows + rest_windows)) + 11
    cue, truth = np.full(n, rest_label, dtype=np.int64), np.full(n, rest_label, dtype=np.int64)
    amp = np.tile(rest_level * gain, (n, 1))
    planted = []
    for i, c in enumerate(order):
        s = rest_windows + i * (cue_windows + rest_windows)
        e = s + cue_windows
        o, f = s + int(rng.integers(20, 81)), e + int(rng.integers(-20, 61))
        cue[20 * s:20 * e] = c
        truth[20 * o:20 * f] = c
        amp[20 * o:20 * f] = pattern[c] * gain
        planted.append((o, f))
    raw = torch.from_numpy((rng.standard_normal((n, 12)) * amp * 2e-3).astype(np.float32)).cuda()
    return raw, cue, truth, np.array(planted)


def realign_main(a):
    """--realign: (a) realign_cues on a cued recording of the synthetic person of --enroll who follows the cue late, against
    the definition on the host; (b) how far the found onsets and offsets lie from the planted ones; (c) held-out accuracy of
    enroll + finetune fed with the raw cue, the realigned labels and the planted truth."""
    from contrastiveprosthetics_amd.online import expected_commands, recording_windows, window_labels
    from contrastiveprosthetics_amd.realign import (activity_profile, activity_reference, cue_segments, realign_cues, realign_reference,
                                                    sample_labels)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    classes, rest = list(range(41)), 41
    pattern = rng.uniform(0.4, 3.0, (41, 12))
    people = np.exp(rng.normal(0.0, 0.35, (10, 12)))              # per-person channel gains; person 9 is never trained on
    params = dict(d_e=16, lr_emg=1e-3, reg_emg=1e-5, dp_emg=0.0, lr_glove=1e-3, reg_glove=1e-6, dp_glove=0.0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    raw0, _ = _cue_recording(rng, pattern, people[0], 30, classes)
    ident = torch.stack([torch.zeros(12), torch.ones(12)]).cuda()
    w0 = recording_windows(raw0, ident)
    mean, std = w0.mean(0), w0.std(0)
    lines = []

    def out(r):
        print(json.dumps(r), flush=True)
        lines.append(r)

    # the model of --enroll: 400 steps on people 0..8, one window per class and group
    probe = OnlineDecoder(e, mean, std, classes=classes)
    train = []
    for p in range(9):
        raw, lab = _cue_recording(rng, pattern, people[p], 40, classes)
        w = recording_windows(raw, probe.mean_std, probe._b, probe._a, 0)
        wl = window_labels(lab, 0)
        train.append(torch.stack([w[torch.as_tensor(np.nonzero(wl == c)[0][:40]).cuda()] for c in classes]))
    train = torch.stack(train)
    labels = torch.arange(41).repeat(8).cuda()
    for step in range(400):
        pi = torch.randint(0, 9, (8,))
        wi = torch.randint(0, 40, (8, 41))
        x = torch.stack([train[pi[g], torch.arange(41), wi[g]] for g in range(8)]).reshape(-1, 12).contiguous()
        z = e.encoder_forward(x, training=True)
        e.head(z, labels, 1, want_grad=True)
        e.encoder_backward(x)
        e.adam_step(params)
    torch.cuda.synchronize()

    # person 9 follows the cue late, in the recording to personalise on and in the held-out one
    rawE, cueE, truthE, plantedE = _lagged_recording(rng, pattern, people[9], 200, 150, rng.permutation(41), rest)
    rawT, cueT, truthT, plantedT = _lagged_recording(rng, pattern, people[9], 200, 150, rng.permutation(41), rest)
    wE = recording_windows(rawE, probe.mean_std, probe._b, probe._a, 0)
    cue = expected_commands(cueE, classes, 0, rest=rest)
    prof = activity_profile(wE, cue)

    # (a) time: the device call with its one copy of the results, against the definition on the same windows on the host
    dev_ms = _wall(lambda: realign_cues(wE, cue, prof), a.iters)
    host_w = wE.cpu().numpy()
    segs = cue_segments(cue)
    t_act = _wall(lambda: activity_reference(host_w, prof["base"], prof["gain"]), max(2, a.iters // 3), warmup=1)
    act = activity_reference(host_w, prof["base"], prof["gain"])
    defaults = dict(max_lag=100, max_lead=50, min_len=25, min_rest=10, context=100, min_contrast=0, guard=5)
    t_ref = _wall(lambda: realign_reference(act, cue, segs, **defaults), max(2, a.iters // 3), warmup=1)
    got = realign_cues(wE, cue, prof)
    want = realign_reference(act, cue, segs, **defaults)
    out(dict(part="a", windows=int(wE.shape[0]), segments=int(segs.shape[0]), realign_cues_ms=round(dev_ms, 3),
             activity_reference_ms=round(t_act, 3), realign_reference_ms=round(t_ref, 3), ratio=round((t_act + t_ref) / dev_ms, 1),
             equal=bool(np.array_equal(got["expected"], want[0]))))

    # (b) the pairs found against the planted ones (rows in cue order, as the planted ones are)
    seg = got["segments"]
    d_on, d_off = np.abs(seg["onset"] - plantedE[:, 0]), np.abs(seg["offset"] - plantedE[:, 1])
    truth_w = expected_commands(truthE, classes, 0, rest=rest)
    scored = (got["expected"] != -2) & (truth_w != -2)
    out(dict(part="b", status_0=int((seg["status"] == 0).sum()), onset_err_mean=round(float(d_on.mean()), 2), onset_err_max=int(d_on.max()),
             offset_err_mean=round(float(d_off.mean()), 2), offset_err_max=int(d_off.max()),
             cue_windows_wrong=round(float((cue != truth_w)[(cue != -2) & (truth_w != -2)].mean()), 4),
             realigned_windows_wrong=round(float((got["expected"] != truth_w)[scored].mean()), 4)))

    # (c) enroll + finetune on the three labellings, scored on the held-out recording's planted truth
    n = int(rawE.shape[0])
    feeds = dict(cue=np.where(cueE == rest, -1, cueE), realigned=sample_labels(got["expected"], n), truth=np.where(truthE == rest, -1, truthE))
    wlT = window_labels(np.where(truthT == rest, -1, truthT), 0)
    ok = wlT >= 0
    tune = dict(steps=200, lr=1e-3, lr_rows=1e-2, scale=10.0)
    for dtype in ("f32", "bf16"):
        r = dict(part="c", dtype=dtype, windows=int(ok.sum()), **tune)
        for name, lab in feeds.items():
            dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
            counts = dec.enroll(rawE, lab)
            dec.finetune(rawE, lab, **tune)
            pred, voted = (t.cpu().numpy() for t in dec.push(rawT))
            r["labelled_" + name] = int(sum(counts.values()))
            r["acc_" + name] = round(float((pred[ok] == wlT[ok]).mean()), 4)
            r["acc_" + name + "_voted"] = round(float((voted[ok] == wlT[ok]).mean()), 4)
        out(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --realign --iters {a.iters} on {dev}\n")
            f.write("# A synthetic person (the people, patterns and training of --enroll; rest at a quarter of the channel gains) who\n"
                    "# follows each cue of 200 windows late: the movement starts a drawn 20..80 windows behind the cue's start and ends a\n"
                    "# drawn -20..+60 windows behind its end.  Noise with planted amplitude steps proves nothing about real subjects:\n"
                    "# the numbers are recorded, not asserted.  (a) wall time, host-synchronised, median: realign_cues with a given\n"
                    "# profile (two launches of cp_online_realign* and one copy) against activity_reference + realign_reference on the\n"
                    "# host;  (b) the found onsets and offsets against the planted ones, in windows, and the share of scored windows\n"
                    "# whose label differs from the planted truth, for the cue and for the realigned labels;  (c) accuracy on the\n"
                    "# planted movements of a held-out recording of the same person, per window and voted over 25 windows, after\n"
                    "# enroll + finetune fed with the raw cue, the realigned labels and the planted truth\n")
            for r in lines:
                f.write(json.dumps(r) + "\n")


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


def gate_main(a, e, stream, mean, std, classes):
    """gated against ungated pushes, interleaved case by case in one run; the gate closes nothing here (its work per window
    does not depend on the thresholds) but runs dwell, release and margin weights"""
    rows = []
    settings = dict(min_cosine=0.2, min_margin=0.02, min_votes=3, dwell=5, release=10, weight="margin")
    for dtype in ("f32", "bf16"):
        for S, n in ((1, 20), (1, 500), (256, 20)):
            m = n // 20
            if S == 1:
                plain = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
                gated = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
            else:
                plain = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                gated = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                for s in range(S):
                    plain.set_classes(s, classes=classes)
                    gated.set_classes(s, classes=classes)
            gate = CommandGate(gated, **settings)
            pos = [0]
            span = stream.shape[0] - S * n

            def chunk():
                base = pos[0] % span
                pos[0] += S * n
                return stream[base:base + S * n]

            if S == 1:
                fns = (("ungated", lambda: plain.push(chunk(), return_logits=True)), ("gated", lambda: gate.push(chunk())))
            else:
                fns = (("ungated", lambda: plain.push_packed(chunk(), [n] * S, return_logits=True)),
                       ("gated", lambda: gate.push_packed(chunk(), [n] * S)))
            res = {}
            for name, fn in fns:
                med, p90 = time_pushes(fn, a.iters, a.warmup)
                res[name] = med
                rows.append(dict(kind=name, dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                                 kernels_per_push=count_kernels(fn, pushes=3)))
            logits = [r[2] for r in plain.push_packed(chunk(), [n] * S, return_logits=True)] if S > 1 \
                else plain.push(chunk(), return_logits=True)[2]
            alone = CommandGate(plain, **settings)
            med, p90 = time_pushes(lambda: alone.apply(logits), a.iters, a.warmup)
            rows.append(dict(kind="gate alone", dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                             kernels_per_push=count_kernels(lambda: alone.apply(logits), pushes=3)))
            for r in rows[-3:]:
                r["gated_minus_ungated_us"] = round(res["gated"] - res["ungated"], 1)
                print(json.dumps(r), flush=True)
            del plain, gated, gate, alone
            torch.cuda.empty_cache()
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --gate --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# ungated = decoder.push(return_logits=True), gated = CommandGate.push on a decoder of its own, gate alone =\n"
                    "# CommandGate.apply on the logits of one push; per-push wall time, host-synchronised (median, p90), kernels per\n"
                    "# push (torch.profiler: library kernels plus torch's own), delta = gated - ungated median\n")
            f.write(f"{'kind':<11} {'dtype':<5} {'streams':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8} {'delta_us':>9}\n")
            for r in rows:
                f.write(f"{r['kind']:<11} {r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['median_us']:>10.1f} {r['p90_us']:>9.1f} "
                        f"{r['kernels_per_push']:>8.1f} {r['gated_minus_ungated_us']:>9.1f}\n")


def drive_main(a, e, stream, mean, std, classes):
    """ungated, gated and driven pushes, interleaved case by case in one run, each on a decoder of its own; the profile uses
    every channel of every class, and its range lies off the stream's windows, so that every channel goes bad (bad_mask_seen in
    the JSON lines): the health part of the walk does all it can do"""
    rows = []
    settings = dict(min_cosine=0.2, min_margin=0.02, min_votes=3, dwell=5, release=10, weight="margin")
    rng = np.random.default_rng(0)
    K = len(classes)
    profile = dict(ids=np.asarray(classes), rest=np.full(12, -4.2, np.float32), span=rng.uniform(0.2, 1.0, (K, 12)).astype(np.float32),
                   weight=rng.integers(1, 256, (K, 12)).astype(np.int32), low=np.full(12, -3.95, np.float32),
                   high=np.full(12, -3.75, np.float32))
    for dtype in ("f32", "bf16"):
        for S, n in ((1, 20), (1, 500), (256, 20)):
            m = n // 20

            def decoder():
                if S == 1:
                    return OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
                d = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                for s in range(S):
                    d.set_classes(s, classes=classes)
                return d

            plain, gate, under = decoder(), CommandGate(decoder(), **settings), CommandGate(decoder(), **settings)
            drive = GraspDrive(under, profile=profile)
            pos = [0]
            span = stream.shape[0] - S * n

            def chunk():
                base = pos[0] % span
                pos[0] += S * n
                return stream[base:base + S * n]

            if S == 1:
                fns = (("ungated", lambda: plain.push(chunk(), return_logits=True)), ("gated", lambda: gate.push(chunk())),
                       ("driven", lambda: drive.push(chunk())))
            else:
                fns = (("ungated", lambda: plain.push_packed(chunk(), [n] * S, return_logits=True)),
                       ("gated", lambda: gate.push_packed(chunk(), [n] * S)), ("driven", lambda: drive.push_packed(chunk(), [n] * S)))
            res, kernels = {}, {}
            for name, fn in fns:
                med, p90 = time_pushes(fn, a.iters, a.warmup)
                res[name], kernels[name] = med, count_kernels(fn, pushes=3)
                rows.append(dict(kind=name, dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                                 kernels_per_push=kernels[name]))
            if kernels["driven"] != kernels["gated"] + 1:
                raise SystemExit(f"a driven push launches {kernels['driven']} kernels, a gated one {kernels['gated']}: not one more")
            if S > 1:
                out = gate.push_packed(chunk(), [n] * S, return_windows=True)
                wins, cmd = [r[2] for r in out], [r[3] for r in out]
            else:
                out = gate.push(chunk(), return_windows=True)
                wins, cmd = out[2], out[3]
            alone = GraspDrive(plain, profile=profile, follow="voted")
            med, p90 = time_pushes(lambda: alone.apply(wins, cmd), a.iters, a.warmup)
            rows.append(dict(kind="drive alone", dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                             kernels_per_push=count_kernels(lambda: alone.apply(wins, cmd), pushes=3)))
            bad = drive.push_packed(chunk(), [n] * S)[0][-1] if S > 1 else drive.push(chunk())[-1]
            for r in rows[-4:]:
                r["gate_adds_us"] = round(res["gated"] - res["ungated"], 1)
                r["drive_adds_us"] = round(res["driven"] - res["gated"], 1)
                r["bad_mask_seen"] = int(bad.max()) if bad.numel() else 0
                print(json.dumps(r), flush=True)
            del plain, gate, under, drive, alone
            torch.cuda.empty_cache()
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --drive --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# ungated = decoder.push(return_logits=True), gated = CommandGate.push, driven = GraspDrive.push on a CommandGate, each\n"
                    "# on a decoder of its own; drive alone = GraspDrive.apply on the windows and commands of one push; per-push wall\n"
                    "# time, host-synchronised (median, p90), kernels per push (torch.profiler: library kernels plus torch's own);\n"
                    "# gate_adds = gated - ungated median, drive_adds = driven - gated median, of the same run\n"
                    "# the profile's range lies off the stream's windows: all twelve channels go bad, the worst case for the health part of the walk\n")
            f.write(f"{'kind':<11} {'dtype':<5} {'streams':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8} {'gate_adds':>10} "
                    f"{'drive_adds':>10}\n")
            for r in rows:
                f.write(f"{r['kind']:<11} {r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['median_us']:>10.1f} {r['p90_us']:>9.1f} "
                        f"{r['kernels_per_push']:>8.1f} {r['gate_adds_us']:>10.1f} {r['drive_adds_us']:>10.1f}\n")


def kinematics_main(a, e, stream, mean, std, classes):
    """--kinematics.  Part 1: a push of 1 and of 25 windows per stream with and without a `JointAngles` stage (20 joints, smooth
    5) behind it, at 1, 16 and 256 streams, f32 and bf16, each on a decoder of its own in this one process: host-synchronised
    medians and kernels per push.  The bare push is timed twice, before and after the posed one; the difference of the two
    medians is the run-to-run spread the stage's cost is read against.  Part 2: moments, solve, apply and score on the synthetic
    person of kinematics.kinematics_recording(41, 6, 59): 14,514 windows x 512 tail inputs x 20 joints, 6 repetitions, beside
    the numpy definitions (the moments' definition on the first 1,024 windows only: it walks a 513 x 513 matrix per window)."""
    from contrastiveprosthetics_amd import kinematics as K
    rng = np.random.default_rng(0)
    D = 20
    W = (0.05 * rng.standard_normal((D, 512))).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    lo, span, rest = np.full(D, -2.0, np.float32), np.full(D, 4.0, np.float32), np.full(D, 2048, np.int32)
    rows = []
    for dtype in ("f32", "bf16"):
        for S in (1, 16, 256):
            for n in (20, 500):
                m = n // 20

                def decoder():
                    if S == 1:
                        return OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
                    d = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                    for s in range(S):
                        d.set_classes(s, classes=classes)
                    return d

                plain, under = decoder(), decoder()
                stage = K.JointAngles(under, smooth=5, rate=400)
                for s in range(S):
                    stage.set_model(*((s,) if S > 1 else ()), W, b, lo, span, rest)
                pos = [0]
                span_s = stream.shape[0] - S * n

                def chunk():
                    base = pos[0] % span_s
                    pos[0] += S * n
                    return stream[base:base + S * n]

                if S == 1:
                    bare, posed = (lambda: plain.push(chunk())), (lambda: stage.push(chunk()))
                else:
                    bare, posed = (lambda: plain.push_packed(chunk(), [n] * S)), (lambda: stage.push_packed(chunk(), [n] * S))
                b1, _ = time_pushes(bare, a.iters, a.warmup)
                pm, pp90 = time_pushes(posed, a.iters, a.warmup)
                b2, bp90 = time_pushes(bare, a.iters, a.warmup)
                kb, kp = count_kernels(bare, pushes=3), count_kernels(posed, pushes=3)
                if kp != kb + 1:
                    raise SystemExit(f"a posed push launches {kp} kernels, a bare one {kb}: not one more")
                bm = 0.5 * (b1 + b2)
                r = dict(dtype=dtype, streams=S, windows=m, bare_us=round(bm, 1), posed_us=round(pm, 1), posed_p90_us=round(pp90, 1),
                         stage_adds_us=round(pm - bm, 1), bare_spread_us=round(abs(b1 - b2), 1), kernels_bare=kb, kernels_posed=kp)
                print(json.dumps(r), flush=True)
                rows.append(r)
                del plain, under, stage
                torch.cuda.empty_cache()
    # ---- part 2: the fit on a whole recording
    k, reps, seg = 41, 6, 59
    p = K.kinematics_recording(k, reps, seg, joints=D, seed=0)
    u, y, rep = p["u"], p["y"], p["rep"]
    m = int(u.shape[0])
    u_d = torch.from_numpy(u).cuda()
    iters = max(a.iters // 20, 3)
    fits = []

    def row(case, fn, n_iter, definition, note=""):
        fn()
        med, p90 = time_pushes(fn, n_iter, 1)
        t0 = time.perf_counter()
        definition()
        r = dict(case=case, windows=m, device_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3),
                 definition_ms=round((time.perf_counter() - t0) * 1e3, 1), note=note)
        print(json.dumps(r), flush=True)
        fits.append(r)

    full = (1 << reps) - 1
    plans = [(full & ~(1 << h), lam) for h in range(reps) for lam in (1e-2, 1.0)]
    tests = [1 << h for h in range(reps) for _ in range(2)]
    row(f"moments ({reps} groups)", lambda: K.moments(u_d, y, None, rep, reps), iters,
        lambda: K.moments_reference(u[:1024], y[:1024], None, rep[:1024], reps), "definition: the first 1,024 windows")
    G, Cm = K.moments(u_d, y, None, rep, reps)
    Gh, Ch = G.cpu().numpy(), np.concatenate(list(Cm.cpu().numpy()), axis=2)[:, :, :D]
    row("solve (1 plan, 2 blocks)", lambda: K.solve(G, Cm, [(full, 0.1)], D), iters, lambda: K.solve_reference(Gh, Ch, [(full, 0.1)]))
    row(f"solve ({len(plans)} plans, 2 blocks)", lambda: K.solve(G, Cm, plans, D), iters, lambda: K.solve_reference(Gh, Ch, plans[:1]),
        "definition: one plan")
    Wp, bp, _ = K.solve(G, Cm, plans, D)
    Wh, bh = Wp.cpu().numpy(), bp.cpu().numpy()
    row(f"apply ({len(plans)} plans)", lambda: K.apply(u_d, Wp, bp), iters, lambda: K.pose_reference(u, Wh[0], bh[0]), "definition: one plan")
    pred = K.apply(u_d, Wp, bp)
    ph = pred[:1].cpu().numpy()
    row(f"score ({len(plans)} plans)", lambda: K.score(pred, y, rep, tests), iters, lambda: K.score_reference(ph, y, rep, tests[:1]),
        "definition: one plan")
    pick = K.pick_pose_inputs(u_d, p["glove"], (rep, reps), (1e-2, 1.0), (0, 2))
    if a.out:
        name = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --kinematics --iters {a.iters} --warmup {a.warmup} on {name}\n")
            f.write("# bare = decoder.push / push_packed, posed = JointAngles.push on a decoder of its own (20 joints, smooth 5); per-push wall\n"
                    "# time, host-synchronised medians; bare is timed before and after posed: bare_us is the mean of the two medians,\n"
                    "# spread their difference; stage_adds = posed - bare; kernels per push (torch.profiler)\n")
            f.write(f"{'dtype':<5} {'streams':>7} {'windows':>7} {'bare_us':>9} {'posed_us':>9} {'p90_us':>9} {'stage_adds':>10} {'spread':>8} "
                    f"{'kernels':>9}\n")
            for r in rows:
                f.write(f"{r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['bare_us']:>9.1f} {r['posed_us']:>9.1f} {r['posed_p90_us']:>9.1f} "
                        f"{r['stage_adds_us']:>10.1f} {r['bare_spread_us']:>8.1f} {r['kernels_bare']:>4.0f}+{r['kernels_posed'] - r['kernels_bare']:.0f}\n")
            f.write(f"# the synthetic person of kinematics.kinematics_recording({k}, {reps}, {seg}): {m} windows x 512 tail inputs x {D} joints, f32\n")
            f.write("# wall time, host-synchronised (median, p90); definition_ms: the numpy definition on the host, once\n")
            f.write(f"{'call':<28} {'windows':>8} {'device_ms':>10} {'p90_ms':>9} {'definition_ms':>14}  note\n")
            for r in fits:
                f.write(f"{r['case']:<28} {r['windows']:>8} {r['device_ms']:>10.3f} {r['p90_ms']:>9.3f} {r['definition_ms']:>14.1f}  {r['note']}\n")
            f.write(f"# pick_pose on the synthetic person (tail inputs lead the angles by 2 windows): mean held-out RMSE per (lag, ridge) "
                    f"{np.round(pick['rmse_mean'], 3).tolist()} degrees, picked lag {pick['lag']} ridge {pick['ridge']}\n")


def kalman_main(a, e, stream, mean, std, classes):
    """--kalman.  Part 1: a push of 1 and of 25 windows per stream bare, with a `JointAngles` stage (smooth 5) and with a
    `PoseFilter` stage behind it (20 joints), at 1, 16 and 256 streams, f32 and bf16, each on a decoder of its own in this one
    process: host-synchronised medians and kernels per push.  The bare push is timed twice, before and after the staged ones; the
    difference of the two medians is the run-to-run spread the stages' cost is read against.  Part 2: the cross-fit, moments,
    design and sweep on the synthetic person of kinematics.kinematics_recording(41, 6, 59): 14,514 windows x 20 joints, 6
    repetitions, beside the numpy definitions, and `pick_filter`'s table at lag 0 and 2."""
    from contrastiveprosthetics_amd import kalman as KF
    from contrastiveprosthetics_amd import kinematics as K
    rng = np.random.default_rng(0)
    D = 20
    W = (0.05 * rng.standard_normal((D, 512))).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    lo, span, rest = np.full(D, -2.0, np.float32), np.full(D, 4.0, np.float32), np.full(D, 2048, np.int32)
    walk = np.cumsum(rng.standard_normal((400, D)), axis=0).astype(np.float32) * 0.1
    noisy = (walk + 0.3 * rng.standard_normal((400, D))).astype(np.float32)
    des = KF.design_reference(KF.moments_reference(noisy, walk, None, 1, KF.centre(lo, span, rest)), [(1, 1e-3, 1.0, 1.0, 64)])
    if des["status"][0] != 0:
        raise SystemExit("the bench's filter has no solution")
    Mf, Kf = des["M"][0], des["K"][0]
    rows = []
    for dtype in ("f32", "bf16"):
        for S in (1, 16, 256):
            for n in (20, 500):
                m = n // 20

                def decoder():
                    if S == 1:
                        return OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
                    d = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                    for s in range(S):
                        d.set_classes(s, classes=classes)
                    return d

                plain, under_j, under_f = decoder(), decoder(), decoder()
                joint, filt = K.JointAngles(under_j, smooth=5, rate=400), KF.PoseFilter(under_f, rate=400)
                for s in range(S):
                    joint.set_model(*((s,) if S > 1 else ()), W, b, lo, span, rest)
                    filt.set_model(*((s,) if S > 1 else ()), W, b, lo, span, rest, Mf, Kf)
                pos = [0]
                span_s = stream.shape[0] - S * n

                def chunk():
                    base = pos[0] % span_s
                    pos[0] += S * n
                    return stream[base:base + S * n]

                if S == 1:
                    bare, posed, filtered = (lambda: plain.push(chunk())), (lambda: joint.push(chunk())), (lambda: filt.push(chunk()))
                else:
                    bare, posed, filtered = ((lambda: plain.push_packed(chunk(), [n] * S)), (lambda: joint.push_packed(chunk(), [n] * S)),
                                             (lambda: filt.push_packed(chunk(), [n] * S)))
                b1, _ = time_pushes(bare, a.iters, a.warmup)
                jm, _ = time_pushes(posed, a.iters, a.warmup)
                fm, fp90 = time_pushes(filtered, a.iters, a.warmup)
                b2, _ = time_pushes(bare, a.iters, a.warmup)
                kb, kj, kf = count_kernels(bare, pushes=3), count_kernels(posed, pushes=3), count_kernels(filtered, pushes=3)
                if kf != kb + 1 or kj != kb + 1:
                    raise SystemExit(f"a filtered push launches {kf} kernels, a posed one {kj}, a bare one {kb}: not one more")
                bm = 0.5 * (b1 + b2)
                r = dict(dtype=dtype, streams=S, windows=m, bare_us=round(bm, 1), joint_us=round(jm, 1), filtered_us=round(fm, 1),
                         filtered_p90_us=round(fp90, 1), joint_adds_us=round(jm - bm, 1), filter_adds_us=round(fm - bm, 1),
                         bare_spread_us=round(abs(b1 - b2), 1), kernels_bare=kb, kernels_filtered=kf)
                print(json.dumps(r), flush=True)
                rows.append(r)
                del plain, under_j, under_f, joint, filt
                torch.cuda.empty_cache()
    # ---- part 2: the fit on a whole recording
    k, reps, seg = 41, 6, 59
    p = K.kinematics_recording(k, reps, seg, joints=D, seed=0)
    iters = max(a.iters // 20, 3)
    fits, picks = [], []

    def row(case, fn, n_iter, definition, m, note=""):
        fn()
        med, p90 = time_pushes(fn, n_iter, 1)
        t0 = time.perf_counter()
        definition()
        r = dict(case=case, windows=m, device_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3),
                 definition_ms=round((time.perf_counter() - t0) * 1e3, 1), note=note)
        print(json.dumps(r), flush=True)
        fits.append(r)

    for lag in (0, 2):
        y = K.window_targets(p["glove"], 0, lag)
        m = int(y.shape[0])
        rep = (p["rep"][:m], reps)
        u_d = torch.from_numpy(p["u"][:m]).cuda()
        a_d = KF.crossfit_inputs(u_d, y, rep, 0.01)
        lo_p, span_p, rest_p = K.limits(y, p["cls"][:m], 0)
        fit = K.PoseFit(torch.zeros(1, D, 512), torch.zeros(1, D), [0], [(tuple(range(reps)), 0.01)], {}, lo_p, span_p, rest_p, lag)
        c = KF.centre(lo_p, span_p, rest_p)
        if lag == 0:
            a_h = a_d.cpu().numpy()
            rows_g, plans, tests = KF._pick_grid(KF.KAPPAS, (1.0,), 1e-3, 128, reps)
            row("crossfit (6 folds)", lambda: KF.crossfit_inputs(u_d, y, rep, 0.01), iters, lambda: None, m, "no definition timed")
            row(f"moments ({reps} groups)", lambda: KF.moments(a_d, y, rep[0], reps, c), iters,
                lambda: KF.moments_reference(a_h, y, rep[0], reps, c), m)
            mom = KF.moments(a_d, y, rep[0], reps, c)
            mom_h = {key: v.cpu().numpy() for key, v in mom.items()}
            row("design (1 plan, T = 128)", lambda: KF.design(mom, plans[:1]), iters, lambda: KF.design_reference(mom_h, plans[:1]), m)
            row(f"design ({len(plans)} plans, T = 128)", lambda: KF.design(mom, plans), iters, lambda: KF.design_reference(mom_h, plans), m)
            des = KF.design(mom, plans)
            Mh, Kh = des["M"].cpu().numpy(), des["K"].cpu().numpy()
            row(f"sweep ({len(plans)} plans)", lambda: KF.sweep(a_d, y, rep[0], tests, des["M"], des["K"], c), iters,
                lambda: KF.sweep_reference(a_h, y, rep[0], tests[:1], Mh[:1], Kh[:1], c), m, "definition: one plan")
        pick = KF.pick_filter(a_d, y, rep, fit)
        picks.append((lag, pick))
        print(json.dumps(dict(lag=lag, table=np.round(pick["table"], 4).tolist(), pick=pick["pick"], delta=float(pick["delta"].max()))), flush=True)
    if a.out:
        name = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --kalman --iters {a.iters} --warmup {a.warmup} on {name}\n")
            f.write("# bare = decoder.push / push_packed, joint = JointAngles.push (smooth 5), filtered = PoseFilter.push, each on a decoder of\n"
                    "# its own (20 joints); per-push wall time, host-synchronised medians; bare is timed before and after the staged pushes:\n"
                    "# bare_us is the mean of the two medians, spread their difference; adds = staged - bare; kernels per push (torch.profiler)\n")
            f.write(f"{'dtype':<5} {'streams':>7} {'windows':>7} {'bare_us':>9} {'joint_us':>9} {'filtered_us':>11} {'p90_us':>9} {'joint_adds':>10} "
                    f"{'filter_adds':>11} {'spread':>8} {'kernels':>9}\n")
            for r in rows:
                f.write(f"{r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['bare_us']:>9.1f} {r['joint_us']:>9.1f} {r['filtered_us']:>11.1f} "
                        f"{r['filtered_p90_us']:>9.1f} {r['joint_adds_us']:>10.1f} {r['filter_adds_us']:>11.1f} {r['bare_spread_us']:>8.1f} "
                        f"{r['kernels_bare']:>4.0f}+{r['kernels_filtered'] - r['kernels_bare']:.0f}\n")
            f.write(f"# the synthetic person of kinematics.kinematics_recording({k}, {reps}, {seg}): 14,514 windows x {D} joints, f32\n")
            f.write("# wall time, host-synchronised (median, p90); definition_ms: the numpy definition on the host, once\n")
            f.write(f"{'call':<28} {'windows':>8} {'device_ms':>10} {'p90_ms':>9} {'definition_ms':>14}  note\n")
            for r in fits:
                f.write(f"{r['case']:<28} {r['windows']:>8} {r['device_ms']:>10.3f} {r['p90_ms']:>9.3f} {r['definition_ms']:>14.1f}  {r['note']}\n")
            for lag, pick in picks:
                f.write(f"# pick_filter at lag {lag} (ridge 0.01, T = 128): rows (rho, kappa, mean held-out RMSE in degrees, jitter) "
                        f"{np.round(pick['table'], 4).tolist()}, picked row {pick['pick']}, largest delta {float(pick['delta'].max()):.2e}\n")


class _Ids:
    """the part of a single-stream decoder that CommandGate.apply reads"""
    phase, n_seen = 0, 0

    def __init__(self, ids, vote, device):
        self.class_ids, self.vote, self.device = torch.as_tensor(ids, dtype=torch.int32), vote, device

    def push(self, *a, **k):
        raise RuntimeError("apply() does not push the decoder")


def track_main(a):
    """--track: tracked against plain pushes, interleaved case by case in one run (rate 0.05 and every bound open, so that
    every window runs the float64 update); --track-sweep: one sweep_tracker call per case (scores on the host)."""
    from contrastiveprosthetics_amd import track as T
    rows, sweeps = [], []
    if a.track:
        torch.manual_seed(0)
        e = Engine(adabn=False, dtype="f32", device="cuda:0")
        e.init_parameters(1)
        stream = (torch.randn(200000, 12) * 2e-3).cuda()
        mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
        classes = list(range(41))
        settings = dict(rate=0.05, min_cosine=-2.0, min_margin=0.0, min_anchor_cosine=-2.0, agree=False)
        for dtype in ("f32", "bf16"):
            for S, n in ((1, 20), (1, 500), (256, 20)):
                m = n // 20
                if S == 1:
                    plain, tracked = (OnlineDecoder(e, mean, std, classes=classes, dtype=dtype) for _ in range(2))
                else:
                    plain, tracked = (MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m) for _ in range(2))
                    for s in range(S):
                        plain.set_classes(s, classes=classes)
                        tracked.set_classes(s, classes=classes)
                tracker = T.PrototypeTracker(tracked, **settings)
                pos = [0]
                span = stream.shape[0] - S * n

                def chunk():
                    base = pos[0] % span
                    pos[0] += S * n
                    return stream[base:base + S * n]

                if S == 1:
                    fns = (("plain", lambda: plain.push(chunk())), ("embeddings", lambda: plain.push(chunk(), return_embeddings=True)),
                           ("tracked", lambda: tracker.push(chunk())))
                else:
                    fns = (("plain", lambda: plain.push_packed(chunk(), [n] * S)),
                           ("embeddings", lambda: plain.push_packed(chunk(), [n] * S, return_embeddings=True)),
                           ("tracked", lambda: tracker.push_packed(chunk(), [n] * S)))
                res = {}
                for name, fn in fns:
                    med, p90 = time_pushes(fn, a.iters, a.warmup)
                    res[name] = med
                    rows.append(dict(kind=name, dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                                     kernels_per_push=count_kernels(fn, pushes=3)))
                emb = [r[-1] for r in plain.push_packed(chunk(), [n] * S, return_embeddings=True)] if S > 1 \
                    else plain.push(chunk(), return_embeddings=True)[-1]
                alone = T.PrototypeTracker(plain, **settings)
                med, p90 = time_pushes(lambda: alone.apply(emb), a.iters, a.warmup)
                rows.append(dict(kind="stage alone", dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                                 kernels_per_push=count_kernels(lambda: alone.apply(emb), pushes=3)))
                for r in rows[-4:]:
                    r["tracked_minus_plain_us"] = round(res["tracked"] - res["plain"], 1)
                    print(json.dumps(r), flush=True)
                del plain, tracked, tracker, alone
                torch.cuda.empty_cache()
    if a.track_sweep:
        base = dict(min_cosine=0.3, min_margin=0.02, min_anchor_cosine=0.5)
        grids = {64: dict(rate=[0.0, 0.01, 0.02, 0.05], agree=[True, False], vote=[10, 25], min_anchor_cosine=[0.5, 0.7, 0.8, 0.9])}
        grids[1024] = dict(grids[64], min_cosine=[0.2, 0.3, 0.4, 0.5], min_margin=[0.0, 0.02, 0.05, 0.1])
        grids[16384] = dict(grids[1024], rate=[i / 256 for i in range(64)])
        for m in (2400, 24000):
            emb, exp, anchor = T.drifting_stream(m, 41, seed=3, noise=0.4, degrees=40.0, segment=50)
            ids = np.arange(41)
            dev = torch.from_numpy(emb).cuda()
            t0 = time.perf_counter()
            ref = T.track_reference(emb, anchor, ids, expected=exp, **dict(base, rate=0.05, agree=True, vote=25))["scores"]
            ref_ms = (time.perf_counter() - t0) * 1e3
            for G, lists in grids.items():
                configs = [dict(base, **c) for c in T.track_grid(**lists)]
                assert len(configs) == G
                sc = T.sweep_tracker(dev, exp, ids, anchor, configs)
                ts = []
                for _ in range(min(a.iters, 10)):
                    t0 = time.perf_counter()
                    T.sweep_tracker(dev, exp, ids, anchor, configs)          # (returns host arrays: it has synchronised)
                    ts.append(time.perf_counter() - t0)
                g = T.pick_tracker(sc)
                frozen = int(np.max(sc["voted_hit_tail"][[i for i, c in enumerate(configs) if c["rate"] == 0.0]]))
                r = dict(rows=m, configs=G, sweep_ms=round(float(np.median(ts)) * 1e3, 3), reference_one_setting_ms=round(ref_ms, 1),
                         picked=configs[g] if g is not None else None, picked_voted_hit_tail=int(sc["voted_hit_tail"][g]) if g is not None else -1,
                         frozen_voted_hit_tail=frozen, tail_rows=int(sc["n_cue"][0]) // 4,
                         reference_voted_hit_tail=ref["voted_hit_tail"])
                print(json.dumps(r), flush=True)
                sweeps.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py{' --track' if a.track else ''}{' --track-sweep' if a.track_sweep else ''} --iters {a.iters} "
                    f"--warmup {a.warmup} on {dev}\n")
            if rows:
                f.write("# plain = decoder.push, embeddings = decoder.push(return_embeddings=True), tracked = PrototypeTracker.push on a\n"
                        "# decoder of its own, stage alone = PrototypeTracker.apply on the embeddings of one push; per-push wall time,\n"
                        "# host-synchronised (median, p90), kernels per push (torch.profiler: library kernels plus torch's own), delta =\n"
                        "# tracked - plain median\n")
                f.write(f"{'kind':<12} {'dtype':<5} {'streams':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8} {'delta_us':>9}\n")
                for r in rows:
                    f.write(f"{r['kind']:<12} {r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['median_us']:>10.1f} {r['p90_us']:>9.1f} "
                            f"{r['kernels_per_push']:>8.1f} {r['tracked_minus_plain_us']:>9.1f}\n")
            if sweeps:
                f.write("# sweep = one sweep_tracker call over the synthetic drifting stream of 41 classes (scores on the host), wall time,\n"
                        "# median; reference = track_reference (numpy) for ONE setting; hits in the last quarter of the cue rows: the\n"
                        "# picked setting's and the best frozen (rate 0) setting's\n")
                f.write(f"{'rows':>6} {'configs':>7} {'sweep_ms':>9} {'reference_ms':>13} {'tail_rows':>9} {'picked_hits':>11} {'frozen_hits':>11}  picked\n")
                for r in sweeps:
                    f.write(f"{r['rows']:>6} {r['configs']:>7} {r['sweep_ms']:>9.3f} {r['reference_one_setting_ms']:>13.1f} {r['tail_rows']:>9} "
                            f"{r['picked_voted_hit_tail']:>11} {r['frozen_voted_hit_tail']:>11}  {json.dumps(r['picked'])}\n")


def holdout_main(a):
    """--holdout: a synthetic person of 41 classes x 6 repetitions (a cue of 45 windows, 14 windows of rest behind it, about
    14,500 windows) through an untrained model's folded decoder.  Timed: the embedding pass; score_plans over the 30
    learning-curve plans and over a grid of 4,096 plans (32 plans x 16 mixes x 8 min_windows); holdout_reference for the 30
    plans; the host loop this replaces for the 6 leave-one-out plans (masked enroll, which installs the rows, reset, push, hits
    counted on the host); score_enrolment as a whole.  The loop's hits are compared with the sweep's."""
    from contrastiveprosthetics_amd import holdout as H
    from contrastiveprosthetics_amd.online import expected_commands
    from contrastiveprosthetics_amd.track import embed_recording
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
    K, REPS, REST_LABEL = 41, 6, 41
    ids = np.arange(K)
    pattern = 0.3 + 1.7 * rng.random((K, 12))
    raws, labs, sreps = [], [], []
    for r in range(REPS):
        for c in rng.permutation(K):
            raws += [rng.standard_normal((900, 12)) * pattern[c] * (1.0 + 0.1 * rng.standard_normal(12)), rng.standard_normal((280, 12)) * 0.2]
            labs += [np.full(900, c), np.full(280, REST_LABEL)]
            sreps += [np.full(900, r), np.full(280, -1)]
    raw = torch.from_numpy((np.concatenate(raws) * 2e-3).astype(np.float32)).cuda()
    lab, srep = np.concatenate(labs).astype(np.int64), np.concatenate(sreps)
    dec = OnlineDecoder(e, mean, std, classes=list(range(K)), dtype="f32")
    exp = expected_commands(lab, ids, rest=REST_LABEL)
    rep, n_rep = H.repetitions(exp)
    assert n_rep == REPS
    prior = dec.class_table()[0]
    iters = min(a.iters, 10)
    embed_ms = _wall(lambda: embed_recording(dec, raw), iters)
    emb = embed_recording(dec, raw)
    curve = H.learning_curve(REPS)
    loo = H.leave_one_out(REPS)
    both = [dict(train=2 ** REPS - 1, eval=2 ** REPS - 1, mix=1.0, min_windows=25), dict(train=0, eval=2 ** REPS - 1, mix=1.0, min_windows=25)]
    grid = H.plan_grid(curve + both, mix=[i / 15 for i in range(16)], min_windows=[1, 5, 10, 25, 50, 100, 150, 200])
    assert len(grid) == 4096
    got = H.score_plans(emb, exp, ids, rep, prior, curve, vote=dec.vote)
    t0 = time.perf_counter()
    ref = H.holdout_reference(emb, exp, ids, rep, prior, curve, vote=dec.vote)
    ref_ms = (time.perf_counter() - t0) * 1e3
    equal = all(np.array_equal(got[k], ref[k]) for k in H.HOLDOUT_SCORE_KEYS) and \
        got["rows"].cpu().numpy().tobytes() == ref["rows"].tobytes()
    curve_ms = _wall(lambda: H.score_plans(emb, exp, ids, rep, prior, curve, vote=dec.vote), iters)       # (host arrays: it has synchronised)
    grid_ms = _wall(lambda: H.score_plans(emb, exp, ids, rep, prior, grid, vote=dec.vote), iters)
    whole_ms = _wall(lambda: H.score_enrolment(dec, raw, exp, plan="learning_curve"), iters)
    table0 = dec.class_table()
    cue = torch.from_numpy(exp).cuda()

    def host_loop():
        hits = []
        for h in range(REPS):
            dec.set_classes(table=table0[0], ids=table0[1])
            dec.enroll(raw, np.where((lab == REST_LABEL) | (srep == h), -1, lab), mix=1.0, min_windows=25)
            dec.reset()
            pred = dec.push(raw)[0]
            held = torch.from_numpy((rep == h) & (exp >= 0)).cuda()
            hits.append(int(((pred == cue) & held).sum()))
        return hits

    loop_hits = host_loop()
    loop_ms = _wall(host_loop, min(iters, 3), warmup=1)
    dec.set_classes(table=table0[0], ids=table0[1])
    dec.reset()
    sweep = H.score_plans(emb, exp, ids, rep, prior, loo, vote=dec.vote)
    r = dict(windows=int(emb.shape[0]), classes=K, repetitions=REPS, embed_ms=round(embed_ms, 3), curve_plans=len(curve),
             curve_ms=round(curve_ms, 3), grid_plans=len(grid), grid_ms=round(grid_ms, 3), reference_curve_ms=round(ref_ms, 1),
             device_equals_reference=bool(equal), score_enrolment_ms=round(whole_ms, 3), host_loop_folds=REPS, host_loop_ms=round(loop_ms, 3),
             host_loop_hits=loop_hits, sweep_pred_hits=[int(x) for x in sweep["pred_hit"]],
             curve={n: list(v) for n, v in H.score_enrolment(dec, raw, exp, plan="learning_curve")["curve"].items()})
    print(json.dumps(r), flush=True)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --holdout --iters {a.iters} on {dev}\n")
            f.write("# A synthetic person (41 classes x 6 repetitions, cue 45 windows, rest 14; an untrained model's folded f32 decoder),\n"
                    "# nothing about real subjects.  Wall time, host-synchronised, median.  embed = track.embed_recording; curve, grid = one\n"
                    "# score_plans call (three launches, scores on the host); reference = holdout_reference (numpy) for the curve's plans;\n"
                    "# host loop = per leave-one-out fold: set_classes, masked enroll, reset, push, hits counted; score_enrolment = embed +\n"
                    "# curve + held-out logits.  The last lines: per fold the loop's and the sweep's raw hits on the held-out repetition, and\n"
                    "# the curve, training repetitions -> (voted hits, cue windows) summed over the held-out repetitions.\n")
            f.write(f"windows {r['windows']}  classes {K}  repetitions {REPS}\n")
            f.write(f"{'what':<34} {'plans':>6} {'ms':>12}\n")
            for what, plans, ms in (("embed", "", r["embed_ms"]), ("score_plans: learning curve", len(curve), r["curve_ms"]),
                                    ("score_plans: grid", len(grid), r["grid_ms"]), ("holdout_reference: learning curve", len(curve), r["reference_curve_ms"]),
                                    ("host loop: leave-one-out", REPS, r["host_loop_ms"]), ("score_enrolment: learning curve", len(curve), r["score_enrolment_ms"])):
                f.write(f"{what:<34} {plans:>6} {ms:>12.3f}\n")
            f.write(f"device equals reference: {r['device_equals_reference']}\n")
            f.write(f"host loop hits  {r['host_loop_hits']}\nsweep pred_hit  {r['sweep_pred_hits']}\ncurve  {json.dumps(r['curve'])}\n")


def prototypes_main(a):
    """--prototypes: the fit at the workload's shape (the synthetic posture person of 41 classes, about 14,500 windows, three
    arm positions, 10 Lloyd rounds) for two and for four rows per class, cut so that the table stays at 64 rows, against
    fit_reference on the host; and a decoder's push with logits against PostureRows.push behind the same decoder, 1 and 25
    windows per push, with the kernels per push of each."""
    from contrastiveprosthetics_amd import prototypes as P
    torch.manual_seed(0)
    k, m = 41, 14_514
    emb, exp, _ = P.posture_recording(m, k, 3, seed=0, segment=45, rest=14)
    ids = np.arange(k)
    emb_d = torch.from_numpy(emb).cuda()
    rows = []
    for name, rpc in (("R=2 (23 classes), 1 (18)", [2] * 23 + [1] * 18), ("R=4 (7 classes), 1 (34)", [4] * 7 + [1] * 34)):
        fit = lambda: P.fit_prototypes(emb_d, exp, ids, rpc, iters=10, min_windows=25)
        got = fit()
        t0 = time.perf_counter()
        ref = P.fit_reference(emb, exp, ids, rpc, iters=10, min_windows=25)
        ref_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(got.rows.cpu().numpy().view(np.int32), ref["rows"].view(np.int32))
                    and np.array_equal(got.counts, ref["counts"]) and np.array_equal(got.moved, ref["moved"])
                    and np.array_equal(got.assign.cpu().numpy(), ref["assign"]))
        med, p90 = time_pushes(fit, max(a.iters // 10, 5), 2)
        r = dict(kind="fit", case=name, windows=m, classes=k, table_rows=int(got.valid.sum()), rounds_that_moved=int((ref["moved"] > 0).sum(axis=1).max()),
                 fit_prototypes_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3), fit_reference_ms=round(ref_ms, 1), equal=same)
        print(json.dumps(r), flush=True)
        rows.append(r)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    stream = (torch.randn(200000, 12) * 2e-3).cuda()
    mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
    table, rid = got.table()
    for n in (20, 500):
        plain = OnlineDecoder(e, mean, std, dtype="f32")
        plain.set_classes(table=torch.from_numpy(table), ids=rid)
        staged = OnlineDecoder(e, mean, std, dtype="f32")
        stage = got.install(staged)
        pos = [0]

        def chunk():
            s = pos[0] % (stream.shape[0] - n)
            pos[0] += n
            return stream[s:s + n]

        for name, fn in (("decoder.push", lambda: plain.push(chunk(), return_logits=True)),
                         ("PostureRows.push", lambda: stage.push(chunk(), return_logits=True))):
            med, p90 = time_pushes(fn, a.iters, a.warmup)
            r = dict(kind="push", case=name, samples=n, windows=n // 20, table_rows=int(rid.shape[0]), median_us=round(med, 1),
                     p90_us=round(p90, 1), kernels_per_push=count_kernels(fn))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --prototypes --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# the fit: one cp_online_proto_fit launch and the copy of counts / valid / moved, host-synchronised (median, p90),\n"
                    "# next to fit_reference (numpy) on the same recording; `equal`: rows, counts, moved and assign agree in every bit\n")
            f.write(f"{'fit':<28} {'windows':>8} {'classes':>8} {'rows':>5} {'rounds':>7} {'device_ms':>10} {'p90_ms':>8} {'reference_ms':>13} {'equal':>6}\n")
            for r in rows:
                if r["kind"] == "fit":
                    f.write(f"{r['case']:<28} {r['windows']:>8} {r['classes']:>8} {r['table_rows']:>5} {r['rounds_that_moved']:>7} "
                            f"{r['fit_prototypes_ms']:>10.3f} {r['p90_ms']:>8.3f} {r['fit_reference_ms']:>13.1f} {str(r['equal']):>6}\n")
            f.write("# per-push wall time with logits, host-synchronised (median, p90), and kernels per push (torch.profiler)\n")
            f.write(f"{'push':<18} {'samples':>7} {'windows':>7} {'rows':>5} {'median_us':>10} {'p90_us':>9} {'kernels':>8}\n")
            for r in rows:
                if r["kind"] == "push":
                    f.write(f"{r['case']:<18} {r['samples']:>7} {r['windows']:>7} {r['table_rows']:>5} {r['median_us']:>10.1f} "
                            f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f}\n")


def metric_main(a):
    """--metric: the fit at the workload's shape (the synthetic person of 41 classes, about 14,500 windows in 6 repetitions, 5
    shrink values) against fit_reference on the host, the transform of the recording, pick_shrink over the 6 folds, and a
    decoder's push with logits against MetricRows.push behind the same decoder, 1 and 25 windows per push, with the kernels per
    push of each.  The decoder holds the 52-row table of --prototypes, so that its push is the one profiles/online_prototypes.txt
    timed."""
    from contrastiveprosthetics_amd import metric as M
    from contrastiveprosthetics_amd import prototypes as P
    torch.manual_seed(0)
    k, m = 41, 14_514
    emb, exp = M.metric_recording(m, k, seed=0, segment=45, rest=14)
    ids = np.arange(k)
    emb_d = torch.from_numpy(emb).cuda()
    rows = []
    fit = lambda: M.fit_metric(emb_d, exp, ids, M.SHRINKS, min_windows=25)
    got = fit()
    t0 = time.perf_counter()
    ref = M.fit_reference(emb, exp, ids, M.SHRINKS, min_windows=25)
    ref_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(got.A.cpu().numpy().view(np.int32), ref["A"].view(np.int32)) and np.array_equal(got.counts, ref["counts"])
                and np.array_equal(got.valid, ref["valid"]) and np.array_equal(got.moments.cpu().numpy().view(np.int64), ref["moments"].view(np.int64)))
    med, p90 = time_pushes(fit, max(a.iters // 10, 5), 2)
    rows.append(dict(kind="host", case="fit_metric (5 shrink values)", windows=m, classes=k, device_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3),
                     reference_ms=round(ref_ms, 1), equal=same))
    t0 = time.perf_counter()
    ref2 = M.apply_reference(emb, ref["A"][2])
    ref_ms = (time.perf_counter() - t0) * 1e3
    e2 = got.apply(emb_d, 2).cpu().numpy()
    med, p90 = time_pushes(lambda: got.apply(emb_d, 2), max(a.iters // 10, 5), 2)
    rows.append(dict(kind="host", case="Metric.apply", windows=m, classes=k, device_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3),
                     reference_ms=round(ref_ms, 1), equal=bool(np.array_equal(e2.view(np.int32), ref2.view(np.int32)))))
    pick = M.pick_shrink(emb_d, exp, ids, M.SHRINKS, min_windows=25)
    med, p90 = time_pushes(lambda: M.pick_shrink(emb_d, exp, ids, M.SHRINKS, min_windows=25), 3, 1)
    rows.append(dict(kind="host", case=f"pick_shrink ({pick['n_rep']} folds x 5)", windows=m, classes=k, device_ms=round(med / 1e3, 3),
                     p90_ms=round(p90 / 1e3, 3), reference_ms=None, equal=None, voted_hit=pick["voted_hit"].tolist(), n_cue=int(pick["n_cue"][0]),
                     baseline=list(pick["baseline"]), shrink=pick["shrink"]))
    for r in rows:
        print(json.dumps(r), flush=True)
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    stream = (torch.randn(200000, 12) * 2e-3).cuda()
    mean, std = torch.full((12,), 0.4).cuda(), torch.full((12,), 0.1).cuda()
    pemb, pexp, _ = P.posture_recording(m, k, 3, seed=0, segment=45, rest=14)
    table, rid = P.fit_prototypes(torch.from_numpy(pemb).cuda(), pexp, ids, [4] * 7 + [1] * 34, iters=10, min_windows=25).table()
    class_rows, valid = got.rows(emb_d, exp, 2)
    assert valid.all()
    for n in (20, 500):
        plain = OnlineDecoder(e, mean, std, dtype="f32")
        plain.set_classes(table=torch.from_numpy(table), ids=rid)
        staged = OnlineDecoder(e, mean, std, dtype="f32")
        staged.set_classes(table=torch.from_numpy(table), ids=rid)
        stage = got.install(staged, class_rows, t=2)
        pos = [0]

        def chunk():
            s = pos[0] % (stream.shape[0] - n)
            pos[0] += n
            return stream[s:s + n]

        for name, fn in (("decoder.push", lambda: plain.push(chunk(), return_logits=True)),
                         ("MetricRows.push", lambda: stage.push(chunk(), return_logits=True))):
            med, p90 = time_pushes(fn, a.iters, a.warmup)
            r = dict(kind="push", case=name, samples=n, windows=n // 20, table_rows=int(rid.shape[0]), median_us=round(med, 1),
                     p90_us=round(p90, 1), kernels_per_push=count_kernels(fn))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --metric --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# wall time, host-synchronised (median, p90), next to the numpy definition on the same recording; `equal`: every bit agrees\n")
            f.write(f"{'call':<32} {'windows':>8} {'classes':>8} {'device_ms':>10} {'p90_ms':>8} {'reference_ms':>13} {'equal':>6}\n")
            for r in rows:
                if r["kind"] == "host":
                    ref_s = "-" if r["reference_ms"] is None else f"{r['reference_ms']:.1f}"
                    f.write(f"{r['case']:<32} {r['windows']:>8} {r['classes']:>8} {r['device_ms']:>10.3f} {r['p90_ms']:>8.3f} {ref_s:>13} "
                            f"{'-' if r['equal'] is None else str(r['equal']):>6}\n")
            f.write(f"# pick_shrink on the synthetic person: voted hits per shrink value {list(M.SHRINKS)} = {pick['voted_hit'].tolist()} of "
                    f"{int(pick['n_cue'][0])} held-out cue windows, plain cosine {pick['baseline'][0]}, picked {pick['shrink']}\n")
            f.write("# per-push wall time with logits, host-synchronised (median, p90), and kernels per push (torch.profiler)\n")
            f.write(f"{'push':<18} {'samples':>7} {'windows':>7} {'rows':>5} {'median_us':>10} {'p90_us':>9} {'kernels':>8}\n")
            for r in rows:
                if r["kind"] == "push":
                    f.write(f"{r['case']:<18} {r['samples']:>7} {r['windows']:>7} {r['table_rows']:>5} {r['median_us']:>10.1f} "
                            f"{r['p90_us']:>9.1f} {r['kernels_per_push']:>8.1f}\n")


def readout_main(a):
    """--readout: the closed-form head fit at the workload's shape (the synthetic person of readout.readout_recording: 41 classes,
    6 repetitions of 59 windows, 14,514 windows of 512 tail inputs): the moments of the 6 repetitions, the solve for 1, 8 and 48
    plans, the apply of 24 projections, and pick_ridge over the 6 folds and 4 ridges behind the encoder, next to what numpy takes
    for X.T @ diag(w) @ X and numpy.linalg.solve of one plan (BLAS and LAPACK: not the definition's order, a yardstick only)."""
    from contrastiveprosthetics_amd import readout as R
    torch.manual_seed(0)
    k, reps, seg = 41, 6, 59
    p = R.readout_recording(k, reps, seg, seed=0)
    u, slots, rep = p["u"], p["slots"], p["rep"]
    m = int(u.shape[0])
    u_d = torch.from_numpy(u).cuda()
    emb0 = R.apply(u_d, p["W0"][None], p["b0"][None])[0].contiguous()
    table = R.enrolled_rows_reference(emb0.cpu().numpy(), slots, k, np.ones(m, dtype=bool))
    targets = R.unit_targets(table)
    w = R.window_weights(slots, k, True, rep)
    iters = max(a.iters // 20, 3)
    rows = []

    def row(case, fn, n_iter, reference_ms=None, **more):
        fn()
        med, p90 = time_pushes(fn, n_iter, 1)
        r = dict(case=case, windows=m, device_ms=round(med / 1e3, 3), p90_ms=round(p90 / 1e3, 3), reference_ms=reference_ms, **more)
        print(json.dumps(r), flush=True)
        rows.append(r)

    t0 = time.perf_counter()
    xm = np.concatenate([u.astype(np.float64), np.ones((m, 1))], axis=1)
    a_np = xm.T @ (w[:, None] * xm)
    b_np = xm.T @ (w[:, None] * targets.astype(np.float64)[slots])
    gram_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    x_np = np.linalg.solve(a_np + 0.1 * np.diag(np.r_[np.ones(512), 0.0]), b_np)
    solve_ms = (time.perf_counter() - t0) * 1e3
    row(f"moments ({reps} groups)", lambda: R.moments(u_d, slots, w, targets, rep, reps), iters, round(gram_ms, 1))
    G, Cm = R.moments(u_d, slots, w, targets, rep, reps)
    full = (1 << reps) - 1
    for n_plans in (1, 8, 48):
        plans = [(full & ~(1 << (t % reps)) if n_plans > 1 else full, 0.1 * 2.0 ** (t // reps)) for t in range(n_plans)]
        row(f"solve ({n_plans} plans)", lambda: R.solve(G, Cm, plans), iters, round(solve_ms * n_plans, 1))
    W, b, status = R.solve(G, Cm, [(full, 0.1)])
    dev = float(np.abs(W[0].cpu().numpy().T.astype(np.float64) - x_np[:512]).max() / np.abs(x_np[:512]).max())
    plans = [(full & ~(1 << h), lam) for h in range(reps) for lam in R.RIDGES]
    W24, b24, _ = R.solve(G, Cm, plans)
    row("apply (24 projections)", lambda: R.apply(u_d, W24, b24), iters)
    pick = R.pick_ridge_inputs(u_d, emb0, slots, np.arange(k), table, R.RIDGES)
    row(f"pick_ridge ({pick['n_rep']} folds x {len(R.RIDGES)} ridges)", lambda: R.pick_ridge_inputs(u_d, emb0, slots, np.arange(k), table, R.RIDGES), 3,
        raw_hit=pick["raw_hit"].tolist(), voted_hit=pick["voted_hit"].tolist(), n_cue=int(pick["n_cue"][0]), baseline=pick["baseline"], ridge=pick["ridge"])
    if a.out:
        name = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --readout --iters {a.iters} on {name}\n")
            f.write(f"# the synthetic person of readout.readout_recording({k}, {reps}, {seg}): {m} windows x 512 tail inputs, f32\n")
            f.write("# wall time, host-synchronised (median, p90); reference_ms: numpy on the host for the same shape, X.T @ diag(w) @ X\n")
            f.write("# (BLAS) beside the moments and numpy.linalg.solve (LAPACK) per plan beside the solve: not the definition's order\n")
            f.write(f"{'call':<34} {'windows':>8} {'device_ms':>10} {'p90_ms':>9} {'reference_ms':>13}\n")
            for r in rows:
                ref_s = "-" if r["reference_ms"] is None else f"{r['reference_ms']:.1f}"
                f.write(f"{r['case']:<34} {r['windows']:>8} {r['device_ms']:>10.3f} {r['p90_ms']:>9.3f} {ref_s:>13}\n")
            f.write(f"# W of the plan (all repetitions, ridge 0.1) against numpy.linalg.solve: largest deviation {dev:.2e} of the largest entry\n")
            f.write(f"# pick_ridge: held-out raw hits per ridge {list(R.RIDGES)} = {pick['raw_hit'].tolist()}, voted {pick['voted_hit'].tolist()} of "
                    f"{int(pick['n_cue'][0])} cue windows; the unfitted projection with enrolled rows {pick['baseline']}; picked {pick['ridge']}\n")


def _cued_logits(m, k, seed=0):
    """synthetic cosines of a cued session on the device: 3 s of a class (raised by 0.5 over its first 12 windows), two
    unscored windows, 2 s of rest, over noise as wide as the raise -> logits (m, k) f32, expected (m,) class ids / REST / IGNORE"""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    g = torch.Generator().manual_seed(seed)
    lg = torch.rand(m, k, generator=g) * 0.6 - 0.2
    exp = np.full(m, IGNORE, dtype=np.int64)
    j, c = 0, 0
    while j < m:
        n = min(300, m - j)
        lg[j:j + n, c % k] += 0.5 * torch.clamp((torch.arange(n) + 1) / 12.0, max=1.0)
        exp[j:j + n] = c % k
        exp[j + 302:j + 500] = REST
        j += 502
        c += 1
    return lg.cuda(), exp


def gate_sweep_main(a):
    """one sweep_gate call against G CommandGate.apply calls in turn plus the copy of their commands to the host, in one
    process, case by case.  Every timed case has its own time limit (--case-seconds): repetitions stop when it is used up, and
    a sequential pass that has used it up stops between two configs and is reported as partial, per config."""
    from contrastiveprosthetics_amd.online import gate_grid, sweep_gate
    K = 8
    ids = list(range(K))
    grids = {64: dict(min_cosine=[0.2, 0.3, 0.4, 0.5], dwell=[1, 3, 5, 8], release=[2, 5, 10, 20])}
    grids[256] = dict(grids[64], weight=["count", "margin"], min_votes=[1, 3])
    grids[1024] = dict(grids[256], vote=[10, 25, 50, 100])
    device = torch.device("cuda:0")
    rows = []
    for m in (6000, 60000):
        logits, exp = _cued_logits(m, K)
        for G, lists in grids.items():
            configs = gate_grid(**lists)
            assert len(configs) == G

            def swept():
                return sweep_gate(logits, exp, ids, configs)

            def sequential(limit):
                """-> configs done within the limit"""
                t0 = time.perf_counter()
                for g, c in enumerate(configs):
                    if time.perf_counter() - t0 > limit:
                        return g
                    gate = CommandGate(_Ids(ids, 25, device), vote=c.get("vote", 25))
                    gate.use(c)
                    gate.apply(logits)[0].cpu()
                return G

            swept()
            torch.cuda.synchronize()
            ts, t_case = [], time.perf_counter()
            while len(ts) < a.iters and (not ts or time.perf_counter() - t_case < a.case_seconds):
                t0 = time.perf_counter()
                swept()                                          # (returns host arrays: it has synchronised)
                ts.append(time.perf_counter() - t0)
            sweep_ms = float(np.median(ts)) * 1e3
            sequential(min(a.case_seconds, 2.0))                 # warm-up: a part of a pass
            torch.cuda.synchronize()
            qs, done, t_case = [], G, time.perf_counter()
            while len(qs) < min(a.iters, 5) and (not qs or time.perf_counter() - t_case + 1.5 * qs[-1] < a.case_seconds):
                t0 = time.perf_counter()
                done = sequential(a.case_seconds - (t0 - t_case))
                torch.cuda.synchronize()
                if done < G:
                    qs = [(time.perf_counter() - t0) / max(done, 1) * G]     # partial: scaled from the configs it got through
                    break
                qs.append(time.perf_counter() - t0)
            seq_ms = float(np.median(qs)) * 1e3
            r = dict(windows=m, configs=G, sweep_ms=round(sweep_ms, 3), sweep_reps=len(ts), sequential_ms=round(seq_ms, 1),
                     sequential_reps=len(qs), sequential_configs_done=done, ratio=round(seq_ms / sweep_ms, 1))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --gate-sweep --iters {a.iters} --case-seconds {a.case_seconds:g} on {dev}\n")
            f.write("# synthetic cued logits, 8 classes; sweep = one sweep_gate call (scores on the host), sequential = G\n"
                    "# CommandGate.apply calls in turn over the same logits, each one's commands copied to the host; wall time,\n"
                    "# median over reps; done < configs: the sequential pass hit its time limit and is scaled from the configs done\n")
            f.write(f"{'windows':>7} {'configs':>7} {'sweep_ms':>9} {'reps':>5} {'sequential_ms':>14} {'reps':>5} {'done':>6} {'ratio':>8}\n")
            for r in rows:
                f.write(f"{r['windows']:>7} {r['configs']:>7} {r['sweep_ms']:>9.3f} {r['sweep_reps']:>5} {r['sequential_ms']:>14.1f} "
                        f"{r['sequential_reps']:>5} {r['sequential_configs_done']:>6} {r['ratio']:>8.1f}\n")


def subset_sweep_main(a):
    """one sweep_subsets call (score table on the host) for growing numbers of subsets of 41 classes; for 64 subsets also the
    composition: per subset a row and column select plus a one-config sweep_gate, whose hit and n_cue must equal the sweep's
    voted_hit and n_cue.  Every timed case has its own time limit (--case-seconds): repetitions stop when it is used up."""
    import itertools
    from contrastiveprosthetics_amd.online import sweep_gate, sweep_subsets
    K, vote = 41, 25
    ids = np.arange(K)
    sets = {n: np.array([sum(1 << i for i in c) for c in itertools.combinations(range(K), n)], dtype=np.uint64) for n in (2, 3, 4)}
    rng = np.random.default_rng(0)
    cases = {64: rng.choice(sets[3], 64, replace=False), 1024: rng.choice(sets[3], 1024, replace=False), 10660: sets[3],
             112750: np.concatenate([sets[2], sets[3], sets[4]])}
    assert [len(v) for v in cases.values()] == list(cases)
    rows = []

    def timed(fn, reps):
        fn()                                                     # (returns host arrays: it has synchronised)
        ts, t_case = [], time.perf_counter()
        while len(ts) < reps and (not ts or time.perf_counter() - t_case < a.case_seconds):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, len(ts)

    for m in (6000, 20500):
        logits, exp = _cued_logits(m, K)
        for G, masks in cases.items():
            ms, reps = timed(lambda: sweep_subsets(logits, exp, ids, masks, vote=vote), a.iters)
            r = dict(windows=m, subsets=G, sweep_ms=round(ms, 3), sweep_reps=reps)
            if G == 64:
                members = [np.array([i for i in range(K) if int(mk) >> i & 1]) for mk in masks]

                def composed():
                    out = []
                    for s in members:
                        keep = (exp < 0) | np.isin(exp, s)
                        sub = logits[torch.from_numpy(keep).to(logits.device)][:, torch.from_numpy(s).to(logits.device)].contiguous()
                        sc = sweep_gate(sub, exp[keep], s, [dict(vote=vote)])
                        out.append((int(sc["n_cue"][0]), int(sc["hit"][0])))
                    return out

                got = sweep_subsets(logits, exp, ids, masks, vote=vote)
                if composed() != list(zip(got["n_cue"].tolist(), got["voted_hit"].tolist())):
                    raise SystemExit(f"the composition's scores differ from the sweep's at {m} windows")
                cms, creps = timed(composed, min(a.iters, 5))
                r.update(composed_ms=round(cms, 1), composed_reps=creps, ratio=round(cms / ms, 1), scores_equal=True)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --subset-sweep --iters {a.iters} --case-seconds {a.case_seconds:g} on {dev}\n")
            f.write("# synthetic cued logits, 41 classes, vote 25; sweep = one sweep_subsets call (masks in, score table on the host),\n"
                    "# wall time, median over reps; 10660 = all triples, 112750 = all pairs, triples and quadruples.  composed (64\n"
                    "# subsets only) = per subset a row and column select plus a one-config sweep_gate; its n_cue and hit equal the\n"
                    "# sweep's n_cue and voted_hit (checked in this run); ratio = composed / sweep\n")
            f.write(f"{'windows':>7} {'subsets':>7} {'sweep_ms':>9} {'reps':>5} {'composed_ms':>12} {'reps':>5} {'ratio':>8}\n")
            for r in rows:
                tail = f"{r['composed_ms']:>12.1f} {r['composed_reps']:>5} {r['ratio']:>8.1f}" if "ratio" in r else f"{'-':>12} {'-':>5} {'-':>8}"
                f.write(f"{r['windows']:>7} {r['subsets']:>7} {r['sweep_ms']:>9.3f} {r['sweep_reps']:>5} {tail}\n")


def map_sweep_main(a):
    from contrastiveprosthetics_amd.online import leave_one_out, recording_windows, rotations, score_channel_maps, window_labels
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    classes = list(range(41))
    pattern = rng.uniform(0.4, 3.0, (41, 12))
    e = Engine(adabn=False, dtype="f32", device="cuda:0")
    e.init_parameters(1)
    raw, lab = _cue_recording(rng, pattern, np.ones(12), 500, classes)
    ident = torch.stack([torch.zeros(12), torch.ones(12)]).cuda()
    w0 = recording_windows(raw[:200000], ident)
    mean, std = w0.mean(0), w0.std(0)
    wl = window_labels(lab, 0)
    scored = wl >= 0
    cand = np.concatenate([rotations(reflect=True), leave_one_out()])
    cand = np.concatenate([cand, cand[:, rotations()[1]], cand[:, rotations()[2]], cand[:, rotations()[3]]])[:64]   # 64 distinct-ish maps
    lines = []

    def out(r):
        print(json.dumps(r), flush=True)
        lines.append(r)

    # ---- (a) the sweep against the push loop
    for dtype in ("f32", "bf16"):
        dec = OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
        for G in (16, 64):
            maps = cand[:G]
            got = {}

            def sweep():
                got["sweep"] = [(s["rows"], s["raw_hits"], s["voted_hits"]) for s in score_channel_maps(dec, raw, lab, maps)]

            def loop():
                res = []
                for g in range(G):
                    dec.reset()
                    dec.set_channel_map(maps[g])
                    p, v = dec.push(raw)                          # split into pushes of 256 windows
                    p, v = p.cpu().numpy(), v.cpu().numpy()
                    res.append((int(scored.sum()), int((p == wl)[scored].sum()), int((v == wl)[scored].sum())))
                dec.set_channel_map(None)
                got["loop"] = res

            t_sweep = _wall(sweep, a.iters, warmup=1)
            t_loop = _wall(loop, max(1, a.iters // 2), warmup=1)
            assert got["sweep"] == got["loop"], "the sweep and the push loop disagree"
            out(dict(kind="map_sweep", dtype=dtype, maps=G, windows=int(wl.shape[0]), rows=G * int(wl.shape[0]),
                     sweep_ms=round(t_sweep, 2), push_loop_ms=round(t_loop, 2), ratio=round(t_loop / t_sweep, 1)))
    # ---- (b) a mapped against an unmapped push, alternating
    perm = rotations()[3]
    stream = (torch.randn(200000, 12) * 2e-3).cuda()
    cases = []
    for n in (20, 500):
        plain = OnlineDecoder(e, mean, std, classes=classes, dtype="f32")
        mapped = OnlineDecoder(e, mean, std, classes=classes, dtype="f32")
        mapped.set_channel_map(perm)
        cases.append((f"single {n // 20} windows", plain, mapped, lambda d, s, n=n: d.push(stream[s:s + n]), n))
    S = 256
    plain = MultiStreamDecoder(e, mean, std, S, dtype="f32")
    mapped = MultiStreamDecoder(e, mean, std, S, dtype="f32")
    for s_ in range(S):
        plain.set_classes(s_, classes)
        mapped.set_classes(s_, classes)
        mapped.set_channel_map(s_, rotations()[s_ % 8] if s_ % 8 else perm)
    counts = np.full(S, 20)
    cases.append((f"{S} streams x 1 window", plain, mapped, lambda d, s: d.push_packed(stream[s:s + 20 * S], counts), 20 * S))
    for name, plain, mapped, fn, n in cases:
        pos = {id(plain): 0, id(mapped): 0}

        def push(d):
            s = pos[id(d)] % (stream.shape[0] - n)
            pos[id(d)] += n
            return fn(d, s)

        meds = {"unmapped": [], "mapped": []}
        for _ in range(5):                                       # alternate, so that a drift of the machine hits both
            for key, d in (("unmapped", plain), ("mapped", mapped)):
                meds[key].append(time_pushes(lambda: push(d), a.iters * 20, a.warmup)[0])
        u, m = np.array(meds["unmapped"]), np.array(meds["mapped"])
        out(dict(kind="mapped_push", case=name, unmapped_us=round(float(np.median(u)), 1), mapped_us=round(float(np.median(m)), 1),
                 difference_us=round(float(np.median(m) - np.median(u)), 1), unmapped_spread_us=round(float(u.max() - u.min()), 1),
                 mapped_spread_us=round(float(m.max() - m.min()), 1),
                 kernels_unmapped=count_kernels(lambda: push(plain)), kernels_mapped=count_kernels(lambda: push(mapped))))
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --map-sweep --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# (a) score_channel_maps against reset / set_channel_map / push (256-window pushes) / count per map, one decoder;\n")
            f.write("#     wall time of the whole call, host-synchronised, median; both sides in the same run and with equal counts\n")
            f.write(f"{'dtype':<5} {'maps':>5} {'windows':>8} {'rows':>9} {'sweep_ms':>10} {'push_loop_ms':>13} {'ratio':>7}\n")
            for r in lines:
                if r["kind"] == "map_sweep":
                    f.write(f"{r['dtype']:<5} {r['maps']:>5} {r['windows']:>8} {r['rows']:>9} {r['sweep_ms']:>10.2f} "
                            f"{r['push_loop_ms']:>13.2f} {r['ratio']:>7.1f}\n")
            f.write("# (b) a mapped against an unmapped push, f32: 5 alternating rounds of host-synchronised medians; spread = max - min\n")
            f.write("#     of the 5 medians of one side\n")
            f.write(f"{'case':<24} {'unmapped_us':>12} {'mapped_us':>10} {'difference_us':>14} {'unmapped_spread_us':>19} "
                    f"{'mapped_spread_us':>17} {'kernels':>12}\n")
            for r in lines:
                if r["kind"] == "mapped_push":
                    f.write(f"{r['case']:<24} {r['unmapped_us']:>12.1f} {r['mapped_us']:>10.1f} {r['difference_us']:>14.1f} "
                            f"{r['unmapped_spread_us']:>19.1f} {r['mapped_spread_us']:>17.1f} "
                            f"{r['kernels_unmapped']:>5.1f} /{r['kernels_mapped']:>5.1f}\n")


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


def stream_projections_main(a, e, stream, mean, std, classes):
    """--stream-projections: a push of the two multi-stream decoders built without the option (`off`), with it and no slot set
    (`unset`) and with it and every slot set (`set`), for S = 1, 16, 256 streams at 1 and 25 windows per stream: 5 alternating
    rounds of host-synchronised medians per case, and the kernels per push of each."""
    rows = []
    g = torch.Generator().manual_seed(0)
    for adaptive in (False, True):
        for dtype in ("f32", "bf16"):
            for S in (1, 16, 256):
                for n in (20, 500):
                    m = n // 20

                    def build(on):
                        kw = dict(dtype=dtype, max_rows=S * m, stream_projections=on)
                        d = AdaptiveMultiStreamDecoder(e, mean, std, S, 0.01, **kw) if adaptive else MultiStreamDecoder(e, mean, std, S, **kw)
                        for s in range(S):
                            d.set_classes(s, classes=classes)
                        return d

                    decs = {"off": build(False), "unset": build(True), "set": build(True)}
                    W, b = decs["set"].projection(0)
                    for s in range(S):                               # every stream its own 16 x 512 + 16 numbers
                        decs["set"].set_projection(s, W + 0.01 * torch.randn(W.shape, generator=g).cuda(),
                                                   b + 0.01 * torch.randn(b.shape, generator=g).cuda())
                    pos = {k: 0 for k in decs}
                    span = stream.shape[0] - S * n

                    def push(k):
                        base = pos[k] % span
                        pos[k] += S * n
                        return decs[k].push_packed(stream[base:base + S * n], [n] * S)

                    meds = {k: [] for k in decs}
                    for _ in range(5):                               # alternate, so that a drift of the machine hits all three
                        for k in decs:
                            meds[k].append(time_pushes(lambda: push(k), a.iters, a.warmup)[0])
                    med = {k: float(np.median(v)) for k, v in meds.items()}
                    r = dict(form="adaptive" if adaptive else "folded", dtype=dtype, streams=S, windows=m,
                             off_us=round(med["off"], 1), unset_us=round(med["unset"], 1), set_us=round(med["set"], 1),
                             off_spread_us=round(float(max(meds["off"]) - min(meds["off"])), 1),
                             unset_minus_off_us=round(med["unset"] - med["off"], 1), set_minus_off_us=round(med["set"] - med["off"], 1),
                             kernels={k: count_kernels(lambda: push(k), pushes=2) for k in decs})
                    print(json.dumps(r), flush=True)
                    rows.append(r)
                    del decs
                    torch.cuda.empty_cache()
    if a.out:
        dev = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py --stream-projections --iters {a.iters} --warmup {a.warmup} on {dev}\n")
            f.write("# one push_packed of S streams x `windows` windows each on MultiStreamDecoder (folded) and\n"
                    "# AdaptiveMultiStreamDecoder (adaptive): off = built without stream_projections, unset = built with it and no slot\n"
                    "# set, set = every stream with a projection of its own.  5 alternating rounds of host-synchronised medians, the\n"
                    "# median of the 5; off_spread = max - min of the 5 medians of `off`; kernels per push (torch.profiler: library\n"
                    "# kernels plus torch's own, e.g. the copy of the counts) as off / unset / set\n")
            f.write(f"{'form':<9} {'dtype':<5} {'streams':>7} {'windows':>7} {'off_us':>9} {'unset_us':>9} {'set_us':>9} {'off_spread':>11} "
                    f"{'unset-off':>10} {'set-off':>9} {'kernels':>17}\n")
            for r in rows:
                k = r["kernels"]
                f.write(f"{r['form']:<9} {r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['off_us']:>9.1f} {r['unset_us']:>9.1f} "
                        f"{r['set_us']:>9.1f} {r['off_spread_us']:>11.1f} {r['unset_minus_off_us']:>10.1f} {r['set_minus_off_us']:>9.1f} "
                        f"{k['off']:>5.1f}/{k['unset']:>5.1f}/{k['set']:>5.1f}\n")


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


def _cued_recording_41(m=600, K=41, seed=0):
    """a synthetic person's cued logits on the host: rest stretches, then cue segments of 30..80 windows in which the cued class
    is raised by a margin that ramps up over the first 12 windows, over noise as wide as the raise -> ids, logits (m, K), expected"""
    from contrastiveprosthetics_amd.online import IGNORE, REST
    rng = np.random.default_rng(1000 * K + seed)
    ids = np.sort(rng.choice(200, K, replace=False)).astype(np.int64)
    lg = rng.uniform(-0.25, 0.35, (m, K))
    exp = np.full(m, IGNORE, dtype=np.int64)
    j = int(rng.integers(3, 10))
    exp[:j] = REST
    while j < m:
        c, n = int(rng.integers(K)), int(rng.integers(30, 81))
        t = np.arange(min(n, m - j))
        lg[j:j + n, c] += 0.45 * np.minimum(1.0, (t + 1) / 12.0)
        exp[j:j + n] = ids[c]
        j += n + 2
        r = int(rng.integers(0, 40))
        exp[j:j + r] = REST
        j += r + (2 if r else 0)
    return ids, lg.astype(np.float32), exp


def sequence_main(a, e, stream, mean, std, classes):
    """--sequence: ungated, gated and sequence-decoded pushes (lag 0 and lag 63), interleaved case by case in one run, each on a
    decoder of its own.  --sequence-sweep: sweep_sequence next to the numpy definition, and the comparison with the gate."""
    from contrastiveprosthetics_amd.online import SCORE_KEYS, gate_grid, pick_gate, score_commands, sweep_gate
    from contrastiveprosthetics_amd.sequence import SequenceGate, SequenceReference, _matrix_for, sequence_grid, sweep_sequence
    rows, sweeps, versus = [], [], []
    settings = dict(min_cosine=0.2, min_margin=0.02, min_votes=3, dwell=5, release=10, weight="margin")
    seq = dict(transitions=dict(switch=0.5, engage=0.5, release=0.5), min_cosine=0.2)
    for dtype in ("f32", "bf16") if a.sequence else ():
        for S, n in ((1, 20), (1, 500), (256, 20)):
            m = n // 20

            def decoder():
                if S == 1:
                    return OnlineDecoder(e, mean, std, classes=classes, dtype=dtype)
                d = MultiStreamDecoder(e, mean, std, S, dtype=dtype, max_rows=S * m)
                for s in range(S):
                    d.set_classes(s, classes=classes)
                return d

            plain, gate = decoder(), CommandGate(decoder(), **settings)
            seq0, seq63 = SequenceGate(decoder(), lag=0, **seq), SequenceGate(decoder(), lag=63, **seq)
            pos = [0]
            span = stream.shape[0] - S * n

            def chunk():
                base = pos[0] % span
                pos[0] += S * n
                return stream[base:base + S * n]

            if S == 1:
                fns = (("ungated", lambda: plain.push(chunk(), return_logits=True)), ("gated", lambda: gate.push(chunk())),
                       ("sequence lag 0", lambda: seq0.push(chunk())), ("sequence lag 63", lambda: seq63.push(chunk())))
            else:
                fns = (("ungated", lambda: plain.push_packed(chunk(), [n] * S, return_logits=True)),
                       ("gated", lambda: gate.push_packed(chunk(), [n] * S)),
                       ("sequence lag 0", lambda: seq0.push_packed(chunk(), [n] * S)),
                       ("sequence lag 63", lambda: seq63.push_packed(chunk(), [n] * S)))
            res = {}
            for name, fn in fns:
                med, p90 = time_pushes(fn, a.iters, a.warmup)
                res[name] = med
                rows.append(dict(kind=name, dtype=dtype, streams=S, windows=m, median_us=round(med, 1), p90_us=round(p90, 1),
                                 kernels_per_push=count_kernels(fn, pushes=3)))
            gate_adds = res["gated"] - res["ungated"]
            for r in rows[-4:]:
                r["adds_us"] = round(res[r["kind"]] - res["ungated"], 1)
                r["of_gate"] = round((res[r["kind"]] - res["ungated"]) / gate_adds, 2) if gate_adds > 0 else float("nan")
                r["lag63_per_window_us"] = round((res["sequence lag 63"] - res["sequence lag 0"]) / m, 2)
                print(json.dumps(r), flush=True)
            del plain, gate, seq0, seq63
            torch.cuda.empty_cache()
    if a.sequence_sweep:
        from contrastiveprosthetics_amd.sequence import potts
        K, M, G = 8, 14514, 4096
        ids = list(range(K))
        logits, exp = _cued_logits(M, K)
        mats = [potts(K, sw, en, rl, tr) for sw in (0.25, 0.5) for en in (0.25, 0.5) for rl in (0.25, 0.5) for tr in (False, True)]
        for lag in (0, 63):
            configs = sequence_grid(transitions=mats, min_cosine=[0.1 + 0.4 * i / 255 for i in range(256)], lag=[lag])
            assert len(configs) == G
            scores = sweep_sequence(logits, exp, ids, configs)
            ts, t_case = [], time.perf_counter()
            while len(ts) < min(a.iters, 10) and (not ts or time.perf_counter() - t_case < a.case_seconds):
                t0 = time.perf_counter()
                sweep_sequence(logits, exp, ids, configs)      # (returns host arrays: it has synchronised)
                ts.append(time.perf_counter() - t0)
            host, t0 = logits.cpu().numpy(), time.perf_counter()
            some = list(range(0, G, G // 16))
            for g in some:
                c = configs[g]
                cmd = SequenceReference(ids, c["min_cosine"], _matrix_for(c["transitions"], np.arange(K)), lag).run_rows(host)[0]
                want = score_commands(cmd, exp)
                if any(int(scores[k][g]) != want[k] for k in SCORE_KEYS):
                    raise SystemExit(f"config {g} at lag {lag}: the sweep's scores are not the definition's")
            ref_ms = (time.perf_counter() - t0) * 1e3 * G / len(some)
            r = dict(windows=M, configs=G, models=len(mats), lag=lag, sweep_ms=round(float(np.median(ts)) * 1e3, 3), reps=len(ts),
                     definition_ms_scaled_from_16=round(ref_ms, 0), ratio=round(ref_ms / (float(np.median(ts)) * 1e3), 0))
            print(json.dumps(r), flush=True)
            sweeps.append(r)
        # the best gate next to the best sequence decoder on one recording of 41 classes, 600 windows
        cid, lg, exp41 = _cued_recording_41()
        dev = torch.from_numpy(lg).cuda()
        gates = gate_grid(min_cosine=[0.2, 0.3, 0.4, 0.5], dwell=[1, 2, 3, 5], release=[1, 2, 5, 10], weight=["count", "margin"],
                          min_votes=[1, 2], vote=[1, 3, 5, 10, 25])
        seqs = sequence_grid(transitions=[dict(switch=sw, engage=en, release=rl, through_rest=tr) for sw in (0.125, 0.25, 0.5, 1.0)
                                          for en in (0.125, 0.25, 0.5, 1.0) for rl in (0.125, 0.25, 0.5, 1.0) for tr in (False, True)],
                             min_cosine=[0.2, 0.3, 0.4, 0.5], lag=[0, 2, 5, 10])
        for name, grid, table in (("sweep_gate", gates, sweep_gate(dev, exp41, cid, gates)),
                                  ("sweep_sequence", seqs, sweep_sequence(dev, exp41, cid, seqs))):
            g = pick_gate(table)
            r = dict(sweep=name, configs=len(grid), picked=g)
            if g is not None:
                r.update({k: int(table[k][g]) for k in ("n_cue", "n_rest", "hit", "wrong", "false_active", "switches", "reached")})
                r["mean_latency_windows"] = round(int(table["latency_sum"][g]) / max(int(table["reached"][g]), 1), 2)
                r["config"] = {k: v for k, v in grid[g].items()}
            print(json.dumps(r, default=str), flush=True)
            versus.append(r)
    if a.out:
        dev_name = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            f.write(f"# tools/online_bench.py{' --sequence' if a.sequence else ''}{' --sequence-sweep' if a.sequence_sweep else ''} "
                    f"--iters {a.iters} --warmup {a.warmup} on {dev_name}\n")
            if rows:
                f.write("# ungated = decoder.push(return_logits=True), gated = CommandGate.push, sequence = SequenceGate.push (potts 0.5, min_cosine\n"
                        "# 0.2), each on a decoder of its own; per-push wall time, host-synchronised (median, p90), kernels per push\n"
                        "# (torch.profiler); adds = median - ungated median of the same run, of_gate = adds / the gate's adds,\n"
                        "# lag63/window = (sequence lag 63 - sequence lag 0) / windows of one stream's push\n")
                f.write(f"{'kind':<16} {'dtype':<5} {'streams':>7} {'windows':>7} {'median_us':>10} {'p90_us':>9} {'kernels':>8} {'adds_us':>8} "
                        f"{'of_gate':>8} {'lag63/window':>13}\n")
                for r in rows:
                    f.write(f"{r['kind']:<16} {r['dtype']:<5} {r['streams']:>7} {r['windows']:>7} {r['median_us']:>10.1f} {r['p90_us']:>9.1f} "
                            f"{r['kernels_per_push']:>8.1f} {r['adds_us']:>8.1f} {r['of_gate']:>8.2f} {r['lag63_per_window_us']:>13.2f}\n")
            if sweeps:
                f.write("# sweep_sequence: synthetic cued logits, 8 classes, 16 cost matrices x 256 thresholds at one lag; wall time of one call\n"
                        "# (scores on the host), median over reps; definition = SequenceReference + score_commands on the host for 16 of the\n"
                        "# configs, scaled to all of them; the 16 score rows equal the sweep's\n")
                f.write(f"{'windows':>7} {'configs':>7} {'lag':>4} {'sweep_ms':>9} {'reps':>5} {'definition_ms':>14} {'ratio':>8}\n")
                for r in sweeps:
                    f.write(f"{r['windows']:>7} {r['configs']:>7} {r['lag']:>4} {r['sweep_ms']:>9.3f} {r['reps']:>5} "
                            f"{r['definition_ms_scaled_from_16']:>14.0f} {r['ratio']:>8.0f}\n")
            if versus:
                f.write("# one synthetic recording, 41 classes, 600 windows: the config pick_gate takes (default limits) from each sweep\n")
                f.write(f"{'sweep':<15} {'configs':>7} {'hit':>5} {'n_cue':>6} {'wrong':>6} {'false_active':>13} {'n_rest':>7} {'switches':>9} "
                        f"{'mean_latency':>13}  config\n")
                for r in versus:
                    if r["picked"] is None:
                        f.write(f"{r['sweep']:<15} {r['configs']:>7}  no config within the limits\n")
                    else:
                        f.write(f"{r['sweep']:<15} {r['configs']:>7} {r['hit']:>5} {r['n_cue']:>6} {r['wrong']:>6} {r['false_active']:>13} "
                                f"{r['n_rest']:>7} {r['switches']:>9} {r['mean_latency_windows']:>13.2f}  {r['config']}\n")


if __name__ == "__main__":
    main()
