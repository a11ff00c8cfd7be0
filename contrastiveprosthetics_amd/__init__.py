"""MI355X-native (gfx950) contrastive sEMG training path.

Drop-in for the hot path of FibonacciDude/ContrastiveProsthetics: the class surface of
``code/models.py`` (``Model``), ``code/load.py`` (``DB23``), ``code/utils.py``
(``TaskWrapper``) and the ``code/train.py`` CLI, over hand-written HIP kernels behind the
C ABI of ``include/cpnative.h``.  Importing the package never touches the GPU; the first
kernel call loads ``libcpnative.so`` and fails loudly if it is absent.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # OnlineDecoder pulls in torch and the engine; importing the package stays light until it is asked for
    if name in ("OnlineDecoder", "MultiStreamDecoder", "AdaptiveMultiStreamDecoder", "recording_windows", "window_labels",
                "CommandGate", "thresholds_from_logits", "REST", "IGNORE", "expected_commands", "score_commands", "pick_gate",
                "sweep_gate", "gate_grid", "SUBSET_SCORE_KEYS", "score_subset", "sweep_subsets", "rank_subsets",
                "search_grasp_sets", "GraspDrive", "drive_profile", "rotations", "leave_one_out", "score_channel_maps",
                "pick_channel_map"):
        from . import online
        return getattr(online, name)
    if name == "finetune_reference":
        from .finetune import finetune_reference
        return finetune_reference
    if name in ("realign_cues", "realign_reference", "activity_profile", "activity_reference", "cue_segments", "sample_labels"):
        from . import realign
        return getattr(realign, name)
    if name in ("PrototypeTracker", "track_reference", "sweep_tracker", "pick_tracker", "track_grid", "embed_recording",
                "TRACK_SCORE_KEYS"):
        from . import track
        return getattr(track, name)
    if name in ("score_enrolment", "score_plans", "holdout_logits", "holdout_reference", "holdout_logits_reference", "repetitions",
                "learning_curve", "plan_grid", "assign_folds", "HOLDOUT_SCORE_KEYS"):       # (holdout.leave_one_out: by module)
        from . import holdout
        return getattr(holdout, name)
    if name in ("fit_prototypes", "fit_reference", "Prototypes", "PostureRows", "group_reference", "posture_recording",
                "prototype_table"):                            # (prototypes.class_of_row, row_id: by module)
        from . import prototypes
        return getattr(prototypes, name)
    if name in ("fit_metric", "Metric", "MetricRows", "pick_shrink", "metric_enrolment", "metric_recording", "apply_reference",
                "stage_reference"):                            # (metric.fit_reference: by module)
        from . import metric
        return getattr(metric, name)
    if name in ("fit_projection", "Readout", "pick_ridge", "readout_recording"):   # (readout.fit_reference, apply_reference: by module)
        from . import readout
        return getattr(readout, name)
    if name in ("SequenceGate", "SequenceReference", "potts", "transitions_from_cues", "sweep_sequence", "sequence_grid"):
        from . import sequence
        return getattr(sequence, name)
    raise AttributeError(name)
