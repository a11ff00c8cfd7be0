"""The launch plan of the training encoder (csrc/encoder_api.cuh): how many launches of each profiler kind one training step
(forward, head, backward) and one evaluation forward record, at the sizes and switches where the host layer chooses between kernels --
the small-batch form up to 64 groups (2,624 windows) and the large one from 65, dropout or not, the 8-bit path, the unfused / unpaired /
bridge test routes, the second stream, the dynamic tile schedule, running statistics against batch statistics.  Counts only, no times.
The table was recorded from the library BEFORE the host layer moved out of api.hip, on an MI355X: a launch gained, lost or filed under
another kind by a change of the host code shows here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
T = 41

# (name, dtype, groups, dp_emg, options, second stream, dynamic tiles, mode); mode: "train" = one training step, "eval" = an evaluation
# forward with the running statistics, "adabn" = an evaluation forward with batch statistics
CASES = []
for _dt in ("f32", "bf16"):
    for _dp in (0.0, 0.0635):
        for _g, _opts in ((8, ()), (64, ()), (65, ()), (8, ("no_small",))):
            CASES.append((f"{_dt}-{_g}g-dp{_dp}" + "".join("-" + o for o in _opts), _dt, _g, _dp, _opts, False, False, "train"))
CASES += [
    ("fp8-65g-dp0.0", "fp8", 65, 0.0, (), False, False, "train"),
    ("fp8-65g-dp0.0635", "fp8", 65, 0.0635, (), False, False, "train"),
    ("bf16-65g-unfused_bn_bwd", "bf16", 65, 0.0635, ("unfused_bn_bwd",), False, False, "train"),
    ("bf16-65g-unpaired_wgrad", "bf16", 65, 0.0635, ("unpaired_wgrad",), False, False, "train"),
    ("fp8-65g-fp8_bridge", "fp8", 65, 0.0635, ("fp8_bridge",), False, False, "train"),
    ("bf16-65g-second_stream", "bf16", 65, 0.0635, (), True, False, "train"),
    ("fp8-65g-second_stream", "fp8", 65, 0.0635, (), True, False, "train"),
    ("bf16-65g-dynamic_tiles", "bf16", 65, 0.0635, (), False, True, "train"),
    ("bf16-65g-eval", "bf16", 65, 0.0, (), False, False, "eval"),
    ("fp8-65g-eval", "fp8", 65, 0.0, (), False, False, "eval"),
    ("bf16-65g-adabn", "bf16", 65, 0.0, (), False, False, "adabn"),
]

# profiler kind -> records, kinds without a record left out
PLAN = {
    "bf16-64g-dp0.0": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "bf16-64g-dp0.0635": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "bf16-65g-adabn": {"bn_finalize": 9, "conv1_fwd": 1, "conv2_fwd": 1, "fc_fwd": 1, "fc_fwd_ws": 6, "fold": 8, "prep": 1, "proj_fwd": 1},
    "bf16-65g-dp0.0": {"bn_bwd": 15, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad_bn": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 7, "fold": 8, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "bf16-65g-dp0.0635": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 5, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "bf16-65g-dynamic_tiles": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 7, "fc_wgrad": 5, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "bf16-65g-eval": {"conv2_fwd": 1, "fc_fwd": 1, "fc_fwd_ws": 6, "prep": 1, "proj_fwd": 1},
    "bf16-65g-second_stream": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 6, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 6},
    "bf16-65g-unfused_bn_bwd": {"bn_bwd": 10, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 5, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "bf16-65g-unpaired_wgrad": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 7, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "bf16-8g-dp0.0": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "bf16-8g-dp0.0-no_small": {"bn_bwd": 15, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad_bn": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 7, "fold": 8, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "bf16-8g-dp0.0635": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "bf16-8g-dp0.0635-no_small": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 5, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "f32-64g-dp0.0": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "f32-64g-dp0.0635": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "f32-65g-dp0.0": {"bn_bwd": 10, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 7, "fc_wgrad": 7, "fold": 8, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "f32-65g-dp0.0635": {"bn_bwd": 10, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad": 4, "fc_dgrad_stats": 3, "fc_fwd": 7, "fc_wgrad": 7, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "f32-8g-dp0.0": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "f32-8g-dp0.0-no_small": {"bn_bwd": 10, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 7, "fc_wgrad": 7, "fold": 8, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "f32-8g-dp0.0635": {"conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad": 7, "fc_fwd": 1, "fc_fwd_ws": 6, "head": 1, "prep": 1, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 1},
    "f32-8g-dp0.0635-no_small": {"bn_bwd": 10, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad": 4, "fc_dgrad_stats": 3, "fc_fwd": 7, "fc_wgrad": 7, "fold": 4, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "fp8-65g-dp0.0": {"bn_bwd": 15, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "fc_dgrad_bn": 6, "fc_dgrad_conv": 1, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 7, "fold": 8, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 7},
    "fp8-65g-dp0.0635": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 3, "fc_dgrad_conv": 1, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 5, "fold": 5, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "fp8-65g-eval": {"conv2_fwd": 1, "fc_fwd": 1, "fc_fwd_ws": 6, "fold": 2, "prep": 1, "proj_fwd": 1},
    "fp8-65g-fp8_bridge": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 4, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 5, "fold": 5, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 5},
    "fp8-65g-second_stream": {"bn_bwd": 12, "bn_finalize": 9, "conv1_bwd": 1, "conv1_fwd": 1, "conv2_dgrad": 1, "conv2_fwd": 1, "conv2_wgrad": 1, "dropout": 3, "fc_dgrad_bn": 3, "fc_dgrad_conv": 1, "fc_dgrad_stats": 3, "fc_fwd": 1, "fc_fwd_ws": 6, "fc_wgrad": 6, "fold": 5, "head": 1, "prep": 2, "proj_bwd": 1, "proj_fwd": 1, "reduce_slabs": 6},
}


def make_engine(case):
    from contrastiveprosthetics_amd import _lib
    from contrastiveprosthetics_amd.engine import Engine
    _, dtype, groups, dp, opts, second, dynamic, mode = case
    e = Engine(adabn=(mode == "adabn"), dtype=dtype, dp_emg=dp, device="cuda", seed=11)
    e.aux_stream_enabled = second
    e.tile_schedule = _lib.CP_TILES_DYNAMIC if dynamic else _lib.CP_TILES_STATIC
    for o in opts:
        e.options[o] = 1
    e.init_parameters(7)
    g = torch.Generator().manual_seed(5)
    mu = torch.randn(T, 12, generator=g)
    x = (mu[None] + torch.randn(groups, T, 12, generator=g)).reshape(groups * T, 12).cuda()
    return e, x, torch.arange(T).repeat(groups).cuda()


def run_pass(e, x, labels, mode):
    """one training step (forward, head, backward) or one evaluation forward; returns z and the head's output (or None)"""
    if mode != "train":
        return e.encoder_forward(x, training=False), None
    z = e.encoder_forward(x, training=True)
    out, _, _ = e.head(z, labels, 1, want_grad=True)
    e.encoder_backward(x)
    return z, out


def launch_counts(case):
    e, x, labels = make_engine(case)
    if case[1] == "fp8" and case[7] != "train":
        e.encoder_forward(x, training=False)          # (an engine's first 8-bit evaluation runs twice, to measure its scales: not counted)
    e.profile_enable(None, max_records=1024)
    run_pass(e, x, labels, case[7])
    e.profile_disable()
    torch.cuda.synchronize()
    return {k: n for k, (_, n) in e.profile_summary().items() if n}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launches_per_kind(case):
    got = launch_counts(case)
    print(case[0], got)
    assert got == PLAN[case[0]], (case[0], got)
