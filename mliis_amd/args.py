"""Command-line surface of run_metasegnet.py: the same flag names, types and defaults as the reference's
meta_learners/args.py:16-118 (pinned by tests/golden/host_logic.json -> argparse_defaults / argparse_runsh_like), and the kwargs
builders of args.py:121-236 re-stated for the device learner.  Flags whose feature is outside the hot-path scope are accepted
(so existing command lines parse) and rejected with a clear error only if they would change behaviour.
"""
from __future__ import annotations

import argparse
from functools import partial

from .lr_schedulers import supported_learning_rate_schedulers
from .steplog import capacity_for

SUPPORTED_MODELS = {"efficientlab"}
SUPPORTED_SEARCH_ALGS = {"GP"}

# (flag, kwargs) in the reference's order
def _positive_float(v) -> float:
    """argparse type of a threshold: a finite float above zero."""
    import math
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise argparse.ArgumentTypeError("{!r} is not a number".format(v)) from None
    if not (math.isfinite(f) and f > 0):
        raise argparse.ArgumentTypeError("{!r} is not a finite positive number".format(v))
    return f


def _nonnegative_float(v) -> float:
    """argparse type of an exponent: a finite float at or above zero."""
    import math
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise argparse.ArgumentTypeError("{!r} is not a number".format(v)) from None
    if not (math.isfinite(f) and f >= 0):
        raise argparse.ArgumentTypeError("{!r} is not a finite number >= 0".format(v))
    return f


def _tversky_pair(t) -> tuple:
    """(alpha, beta) of the Tversky index: two finite floats >= 0 whose sum is positive (ArgumentTypeError / ValueError otherwise)."""
    try:
        alpha, beta = t
    except (TypeError, ValueError):
        raise ValueError("tversky takes two numbers (alpha, beta), got {!r}".format(t)) from None
    alpha, beta = _nonnegative_float(alpha), _nonnegative_float(beta)
    if not alpha + beta > 0:
        raise ValueError("tversky: alpha + beta must be positive, got {!r}".format(t))
    return alpha, beta


class _TverskyPair(argparse.Action):
    """--tversky ALPHA BETA: the values pass _nonnegative_float one by one; the pair is refused here when both are zero."""

    def __call__(self, parser, namespace, values, option_string=None):
        try:
            setattr(namespace, self.dest, _tversky_pair(values))
        except (ValueError, argparse.ArgumentTypeError) as e:
            parser.error("argument {}: {}".format(option_string, e))


_FLAGS = [
    ("--fine-tune-task", dict(type=str, default=None)),
    ("--fine-tuned-checkpoint", dict(type=str, default=None)),
    ("--pretrained", dict(action="store_true", default=False)),
    ("--seed", dict(type=int, default=0)),
    ("--checkpoint", dict(default="model_checkpoint")),
    ("--classes", dict(type=int, default=1)),
    ("--shots", dict(type=int, default=5)),
    ("--train-shots", dict(type=int, default=5)),
    ("--inner-batch", dict(type=int, default=8)),
    ("--inner-iters", dict(type=int, default=8)),
    ("--replacement", dict(action="store_true")),
    ("--learning-rate", dict(type=float, default=1e-3)),
    ("--meta-step", dict(type=float, default=0.1)),
    ("--meta-step-final", dict(type=float, default=0.1)),
    ("--meta-batch", dict(type=int, default=5)),
    ("--meta-iters", dict(type=int, default=400000)),
    ("--eval-batch", dict(type=int, default=8)),
    ("--eval-iters", dict(type=int, default=4)),
    ("--eval-samples", dict(type=int, default=200)),
    ("--eval-interval", dict(type=int, default=10)),
    ("--weight-decay", dict(type=float, default=1)),
    ("--transductive", dict(action="store_true")),
    ("--foml", dict(action="store_true")),
    ("--foml-tail", dict(type=int, default=None)),
    ("--sgd", dict(action="store_true")),
    ("--n_unet_encoding_stacks", dict(type=int, default=4)),
    ("--data-dir", dict()),
    ("--loss_name", dict(default="cross_entropy")),
    ("--save_fine_tuned_checkpoints", dict(action="store_true")),
    ("--save_fine_tuned_checkpoints_train", dict(action="store_true")),
    ("--save_fine_tuned_checkpoints_dir", dict(default="/tmp/checkpoints/fine-tuned")),
    ("--model_name", dict(default="efficientlab")),
    ("--start_num_feature_maps_power", dict(type=int, default=5)),
    ("--restore_efficient_net_weights_from", dict(type=str, default=None)),
    ("--spatial_pyramid_pooling", dict(action="store_true")),
    ("--skip_decoding", dict(action="store_true")),
    ("--rsd", dict(type=int, nargs="+")),
    ("--feature_extractor_name", dict(type=str, default="efficientnet-b0")),
    ("--learning_rate_scheduler", dict(type=str, default="fixed")),
    ("--step_decay_rate", dict(type=float, default=0.5)),
    ("--decay_after_n_steps", dict(type=int, default=5)),
    ("--l2", dict(action="store_true")),
    ("--l1", dict(action="store_true")),
    ("--darc1", dict(action="store_true")),
    ("--augment", dict(action="store_true")),
    ("--final_layer_dropout_rate", dict(type=float, default=0.0)),
    ("--image_size", dict(type=int, default=320)),
    ("--label_smoothing", dict(type=float, default=0.0)),
    ("--continue_training_from_checkpoint", dict(default=None)),
    ("--fss_1000", dict(action="store_true")),
    ("--num_val_tasks", dict(type=int, default=0)),
    ("--eval_val_tasks", dict(action="store_true")),
    ("--serially_eval_all_test_tasks", dict(action="store_true")),
    ("--optimize_update_hyperparms_on_val_set", dict(action="store_true")),
    ("--num_configs_to_sample", dict(type=int, default=100)),
    ("--meta_fine_tune_steps_on_train_val", dict(type=int, default=0)),
    ("--uho_outer_iters", dict(type=int, default=2)),
    ("--lr_search_range_low", dict(type=float, default=0.0005)),
    ("--lr_search_range_high", dict(type=float, default=0.05)),
    ("--drop_rate_search_range_low", dict(type=float, default=0.2)),
    ("--drop_rate_search_range_high", dict(type=float, default=0.2)),
    ("--aug_rate_search_range_low", dict(type=float, default=0.5)),
    ("--aug_rate_search_range_high", dict(type=float, default=0.5)),
    ("--batch_size_search_range_low", dict(type=int, default=8)),
    ("--batch_size_search_range_high", dict(type=int, default=8)),
    ("--run_k_shot_learning_curves_experiment", dict(action="store_true")),
    ("--fp_k_test_set", dict(action="store_true")),
    ("--disable_rsd_residual_connections", dict(action="store_true")),
    ("--do_not_restore_final_layer_weights", dict(action="store_true")),
    ("--eval_tasks_with_median_early_stopping_iterations", dict(action="store_true")),
    ("--min_steps", dict(type=int, default=0)),
    ("--max_steps", dict(type=int, default=80)),
    ("--k_shot_iter_range", dict(nargs="+", type=int, default=None)),
    ("--sample_foml_train_val_with_replacement", dict(action="store_true")),
    ("--aug_rate", dict(type=float, default=0.5)),
    ("--uho_results_csv_name", dict(type=str, default="val-set_hyper_param_search_results.csv")),
    ("--uho_estimator", dict(type=str, default="GP")),
]
# extensions of this build (not in the reference)
_EXT = [
    ("--synthetic-tasks", dict(type=int, default=0, help="use N synthetic tasks instead of --data-dir (no dataset needed)")),
    ("--no-hip-graph", dict(action="store_true", help="launch inner steps eagerly instead of replaying a captured HIP graph")),
    ("--k-shot-range", dict(nargs="+", type=int, default=None,
                            help="ks of --run_k_shot_learning_curves_experiment (default: the reference's 1 5 10 50 100 200 400)")),
    ("--k-shot-test-samples", dict(type=int, default=20, help="held-out examples per task in the k-shot experiment (reference: 20)")),
    ("--skip-train-task-eval", dict(action="store_true",
                                    help="skip the evaluation pass over the meta-TRAIN tasks that the reference always runs before the test tasks")),
    ("--augment-on-host", dict(action="store_true",
                               help="with --augment: compute the augmented pixels in numpy / scipy on the host, draw- and pixel-identical to "
                                    "the reference -- REQUIRED for reference-parity runs.  Default: same scalar draws, pixel work on the device "
                                    "(csrc/augment.hip): Philox noise fields, Keys-cubic rotation instead of scipy's prefiltered B-spline, "
                                    "constant-mode holes by coordinate range -- statistically, not pixel-, identical")),
    ("--augment-workers", dict(type=int, default=-1,
                               help="worker processes for the pixel half of --augment (-1: host cores - 1, 0: inline like the reference)")),
    ("--concurrent-tasks", dict(type=int, default=1,
                                help="adapt this many tasks of a meta-batch at once on separate learners / streams (same meta-update; "
                                     "4 is the optimum on MI355X, needs meta_batch_size / ranks >= 2 to matter).  Also with --augment "
                                     "(pixels on the device: every learner augments its own batches); --augment-on-host adapts one task "
                                     "at a time")),
    ("--matmul-precision", dict(choices=["fp32", "fp32-native", "bf16", "fp8", "bf16-storage"], default="fp32",
                                help="operand precision of the matrix cores in the dense convs (bf16: fp32 tensors rounded on the fly, fp32 accumulation); "
                                     "bf16-storage: bf16 operands and the expanded MBConv tensors (z0, z1, a1, their gradients) as bf16 in HBM during "
                                     "training steps, fp32 statistics / accumulation / weights (BASELINE configs[3])")),
    ("--checkpoint-format", dict(choices=["npz", "tf"], default="npz",
                                 help="tensor container of written checkpoints: numpy .npz or a TensorFlow TensorBundle (.index/.data)")),
    ("--device-metrics", dict(action="store_true", help="score evaluation images on the device (Learner.score_resident: four pixel counts per image come back instead "
                                   "of the prediction mask; the same IoUs bit for bit; its speed against the default host path has not been "
                                   "measured)")),
    ("--save-predictions", dict(type=str, default=None, metavar="DIR",
                                help="save every test image's predicted mask of the final evaluation passes as DIR/<task>/sample<k>_query<j>_mask.png "
                                     "(1-bit PNG; with --device-metrics the mask comes back bit-packed beside the counts).  The environment "
                                     "variable SAVE_PREDICTIONS (the reference's switch), set to a non-empty string, acts like "
                                     "--save-predictions predictions --save-prediction-overlays; an explicit DIR wins")),
    ("--save-prediction-overlays", dict(action="store_true",
                                        help="with --save-predictions: also save the query image tinted where the mask is set (..._overlay.png)")),
    ("--resident-dataset", dict(action="store_true",
                                help="keep every task on the device as the bytes the dataset stores (4 per pixel instead of 20 as floats, "
                                     "metaseg.ByteTask); a task's shots are expanded -- and resampled to --image_size -- on the device "
                                     "when it becomes resident (csrc/taskload.hip).  Same floats as the default path at the stored size")),
    ("--stored-image-size", dict(type=int, default=None, metavar="N",
                                 help="side of the examples the --data-dir shards hold (default: --image_size); another size than "
                                      "--image_size needs --resident-dataset, which resamples on the device")),
    ("--inner-loop-log", dict(action="store_true",
                              help="log the inner loop: every training step appends its loss, IoU, learning rate, gradient norm and the "
                                   "non-finite counts of gradient and parameters to a ring on the device (csrc/steplog.hip: one more launch "
                                   "in the step's graph, no host round trip per step); once per meta-iteration the ring is read and one "
                                   "summary line goes to <checkpoint>/train/inner_loop.jsonl")),
    ("--on-divergence", dict(choices=["off", "skip", "abort"], default="off",
                             help="what a non-finite loss, gradient or parameter in an inner step of any rank does to the meta-update: "
                                  "off = nothing (logged with --inner-loop-log), skip = the meta-iteration's update is left out on all "
                                  "ranks, abort = stop with an error before the update and before any checkpoint is written; skip and "
                                  "abort imply --inner-loop-log")),
    ("--inner-loop-layer-log", dict(action="store_true",
                                    help="log the inner loop per tensor as well: every training step also writes, for each trainable tensor, "
                                         "the norm and largest magnitude of its gradient and of its parameters and their non-finite counts to "
                                         "a second ring on the device (csrc/layerlog.hip: two more launches in the step's graph), and every "
                                         "task the per-tensor distance it moved from the initialisation; every "
                                         "--inner-loop-layer-log-interval meta-iterations one line goes to "
                                         "<checkpoint>/train/inner_loop_layers.jsonl, and a non-finite step is attributed to tensors.  "
                                         "Implies --inner-loop-log")),
    ("--inner-loop-layer-log-interval", dict(type=int, default=100, metavar="N",
                                             help="with --inner-loop-layer-log: read the per-tensor rings and write a line every N "
                                                  "meta-iterations (the checkpoint cadence)")),
    ("--inner-clip-norm", dict(type=_positive_float, default=None, metavar="C",
                               help="clip every training step's loss gradient by its global L2 norm, on the device, between the backward "
                                    "pass and the optimizer launch (csrc/clip.hip: two more launches in the step's graph): every element "
                                    "times C / ||g|| when ||g|| > C.  Applies wherever a model is adapted: meta-training and its "
                                    "--concurrent-tasks lanes, evaluation fine-tunes, early stopping, the k-shot curves, the "
                                    "update-hyperparameter search, --no-hip-graph, both optimizers.  The --l2 / --l1 terms are formed "
                                    "inside the optimizer launch and stay outside the clip; a gradient with a NaN or inf in it is left "
                                    "exactly as it was (--on-divergence sees what it sees without the flag).  Not with --inner-clip-ratio")),
    ("--inner-clip-ratio", dict(type=_positive_float, default=None, metavar="LAMBDA",
                                help="clip every training step's loss gradient per trainable tensor instead: tensor t times "
                                     "LAMBDA max(||theta_t||, eps) / ||g_t|| when ||g_t|| exceeds that bound; the same launches, places "
                                     "and exclusions as --inner-clip-norm.  Not with --inner-clip-norm")),
    ("--inner-clip-ratio-eps", dict(type=_positive_float, default=1e-3, metavar="EPS",
                                    help="with --inner-clip-ratio: the floor of ||theta_t||, which lets zero-initialised biases and "
                                         "batch-norm betas move")),
    ("--focal-gamma", dict(type=_nonnegative_float, default=None, metavar="G",
                           help="focal modulation of the inner loop's pixel loss (Lin et al.): every pixel's cross-entropy term of class c "
                                "times (1 - p_c)^G, on the device (csrc/focal.hip: the fused head's counterpart, one launch more per "
                                "step).  0 is the cross-entropy.  Composes with --loss_name bce_dice, --label_smoothing, --l2, --l1, "
                                "--darc1 and --fg-weight; applies wherever a model is adapted (the same places as --inner-clip-norm); "
                                "evaluation and prediction are unchanged.  `ce` in inner_loop.jsonl is then the focal pixel term")),
    ("--fg-weight", dict(type=_positive_float, default=None, metavar="W",
                         help="weight of the foreground pixels in the inner loop's pixel loss: a pixel counts 1 + (W - 1) * label.  The sum is "
                              "still divided by N H W, not by the sum of the weights, so W > 1 raises the loss scale and usually wants a "
                              "smaller --learning-rate or a clip.  The same kernels and places as --focal-gamma")),
    ("--tversky", dict(nargs=2, type=_nonnegative_float, action=_TverskyPair, default=None, metavar=("ALPHA", "BETA"),
                       help="Tversky region term in the inner loop's loss, on the device (csrc/tversky.hip): -ln(2T / (T + 1)) with T the "
                            "batch mean of (I + eps) / (I + ALPHA * FP + BETA * FN + eps) on the foreground probability, added to the "
                            "pixel term whatever --loss_name says.  1 1 is the soft IoU of --loss_name bce_dice, 0.5 0.5 the soft Dice "
                            "coefficient; BETA > ALPHA weighs a missed foreground pixel more than a false alarm.  Both >= 0, not both 0.  "
                            "The step's tail stays on the decoder's map (three launches, no full-resolution tensor).  Composes with "
                            "--focal-gamma, --fg-weight, --label_smoothing, --l2, --l1 and --darc1; applies wherever a model is adapted "
                            "(the same places as --inner-clip-norm); evaluation and prediction are unchanged.  `iou` in "
                            "inner_loop.jsonl stays the soft IoU")),
    ("--threshold-sweep", dict(action="store_true",
                               help="sweep the decision threshold in the final evaluation pass over the meta-test (or, with "
                                    "--eval_val_tasks, meta-val) tasks: every test image leaves a 2 x 256 histogram of its foreground "
                                    "probability by label class on the device (csrc/sweep.hip: 2 KB per image come back in place of the "
                                    "four counts of --device-metrics), from which the IoU at every threshold k/256, the best threshold and "
                                    "a reliability table are derived exactly; written to <checkpoint>/meta-<test|val>_threshold_sweep.json.  "
                                    "Predictions, saved masks, printed lines and meta-test_results.json stay those of a --device-metrics "
                                    "run at 0.5.  Not applied to the train-task pass, the update-hyperparameter search, the k-shot curves "
                                    "or meta-training")),
    ("--threshold-sweep-val", dict(action="store_true",
                                   help="with --threshold-sweep (implied): after the meta-test pass run the same pass over the --num_val_tasks "
                                        "validation tasks and add selected_on_val = {threshold, val_iou, test_iou_at_threshold} to the file: "
                                        "the threshold chosen on tasks the test score never saw.  Needs --num_val_tasks > 0; not with "
                                        "--eval_val_tasks")),
    ("--eval-tta", dict(nargs="+", choices=["hflip", "vflip", "hvflip"], default=None, metavar="VIEW",
                        help="flip test-time augmentation in the final evaluation passes (the train-task pass, the meta-test / meta-val "
                             "pass and the validation pass of --threshold-sweep-val): every test batch is also predicted mirrored -- hflip: "
                             "columns, vflip: rows, hvflip: both; one more forward pass per view -- each view's decoder-resolution LOGITS "
                             "are mirrored back and averaged with the plain view's on the device (csrc/tta.hip) before anything scores "
                             "them, so the printed IoUs, meta-test_results.json, saved masks and the threshold sweep are those of the "
                             "merged prediction on every scoring path alike.  Averaging logits is a geometric mean of the views' odds, not "
                             "a mean of probabilities.  Not applied to early stopping, the update-hyperparameter search, the k-shot curves "
                             "or meta-training")),
]


def grad_clip(a):
    """The `grad_clip` argument of the Learner from --inner-clip-norm / --inner-clip-ratio / --inner-clip-ratio-eps, None without them."""
    c, lam = getattr(a, "inner_clip_norm", None), getattr(a, "inner_clip_ratio", None)
    if c is not None and lam is not None:
        raise ValueError("--inner-clip-norm and --inner-clip-ratio exclude each other: one clipping mode per run")
    if c is not None:
        return ("norm", _positive_float(c))
    if lam is not None:
        return ("ratio", _positive_float(lam), _positive_float(getattr(a, "inner_clip_ratio_eps", 1e-3)))
    return None


def focal_loss(a) -> dict:
    """The `focal_gamma` / `fg_weight` arguments of the Learner from --focal-gamma / --fg-weight: only the keys whose flag was given."""
    g, w = getattr(a, "focal_gamma", None), getattr(a, "fg_weight", None)
    out = {}
    if g is not None:
        out["focal_gamma"] = _nonnegative_float(g)
    if w is not None:
        out["fg_weight"] = _positive_float(w)
    return out


def tversky(a) -> dict:
    """The `tversky` argument of the Learner from --tversky ALPHA BETA: absent without the flag."""
    t = getattr(a, "tversky", None)
    if t is None:
        return {}
    return dict(tversky=_tversky_pair(t))


def threshold_sweep(a):
    """(sweep, on_val) from --threshold-sweep / --threshold-sweep-val.  Kept out of evaluate_kwargs like the prediction writer: only the final
    evaluation pass over the test (or val) tasks is swept."""
    on_val = bool(getattr(a, "threshold_sweep_val", False))
    sweep = bool(getattr(a, "threshold_sweep", False)) or on_val
    if on_val and getattr(a, "num_val_tasks", 0) <= 0:
        raise ValueError("--threshold-sweep-val selects the threshold on validation tasks: it needs --num_val_tasks > 0")
    if on_val and getattr(a, "eval_val_tasks", False):
        raise ValueError("--threshold-sweep-val with --eval_val_tasks would select and report on the same tasks: use --threshold-sweep alone")
    return sweep, on_val


def eval_views(a) -> tuple:
    """The canonical view tuple of --eval-tta (views.canonical: hflip, vflip, hvflip in that order whatever order was given; a repeat is
    refused), () without the flag.  Kept out of evaluate_kwargs like the prediction writer: only the final evaluation passes merge views."""
    from .views import canonical
    return canonical(getattr(a, "eval_tta", None) or ())


def argument_parser(extensions: bool = True) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flag, kw in _FLAGS + (_EXT if extensions else []):
        p.add_argument(flag, **kw)
    return p


def _max_shots(a) -> int:
    """Examples a task can make resident at once: training / evaluation shots, or the whole k-shot pool."""
    n = max(16, a.train_shots or 0, a.shots + 5)
    if getattr(a, "run_k_shot_learning_curves_experiment", False):
        n = max(n, max(getattr(a, "k_shot_range", None) or [400]) + getattr(a, "k_shot_test_samples", 20))
    return n


def augment_mode(a):
    """False | True (host pixels, --augment-on-host) | "device" -- the `augment` argument of the meta-learners."""
    if not a.augment:
        return False
    return True if getattr(a, "augment_on_host", False) else "device"


def stored_image_size(a) -> int:
    """The side the shards are parsed at (--stored-image-size, default --image_size); a size other than --image_size is only served by
    the device resampler of --resident-dataset."""
    n = getattr(a, "stored_image_size", None)
    n = a.image_size if n is None else int(n)
    if n < 1:
        raise ValueError("--stored-image-size must be positive, got {}".format(n))
    if n != a.image_size and not getattr(a, "resident_dataset", False):
        raise ValueError("--stored-image-size {} differs from --image_size {}: the examples are resampled on the device, which needs "
                         "--resident-dataset".format(n, a.image_size))
    return n


def inner_loop_log(a) -> bool:
    """--inner-loop-log, or an --on-divergence / --inner-loop-layer-log that needs it."""
    return bool(getattr(a, "inner_loop_log", False)) or getattr(a, "on_divergence", "off") != "off" or inner_loop_layer_log(a)


def inner_loop_layer_log(a) -> bool:
    """--inner-loop-layer-log."""
    return bool(getattr(a, "inner_loop_layer_log", False))


def model_kwargs(a) -> dict:
    """Keyword arguments of mliis_amd.learner.Learner from parsed flags (reference: args.py:121-160)."""
    a.model_name = a.model_name.lower()
    if a.model_name not in SUPPORTED_MODELS:
        raise ValueError("Model name must be in the set: {} but is {}".format(SUPPORTED_MODELS, a.model_name))
    # (the step log's ring holds the steps of one task; the key is absent without the flags: the learner is built as always)
    steps = a.inner_iters
    if getattr(a, "meta_fine_tune_steps_on_train_val", 0) > 0:   # (that phase adapts with the searched step count, two steps per batch)
        steps = max(steps, 2 * a.max_steps)
    log = dict(step_log=capacity_for(steps)) if inner_loop_log(a) else {}
    if inner_loop_layer_log(a):   # (the per-tensor ring is sized like the step log's: the same rows)
        log["layer_log"] = True
    clip = grad_clip(a)
    if clip is not None:   # (absent without the flags as well; its ring holds the steps of one task like the step log's)
        log.update(grad_clip=clip, clip_log=capacity_for(steps))
    log.update(focal_loss(a))   # (absent without the flags as well)
    log.update(tversky(a))      # (likewise)
    return dict(feature_extractor_name=a.feature_extractor_name, image_size=a.image_size, rsd=a.rsd or None,
                learning_rate=a.learning_rate, optimizer="sgd" if a.sgd else "adam", l2=a.l2, l1=a.l1, darc1=a.darc1,
                dice=("dice" in a.loss_name), label_smoothing=a.label_smoothing, final_layer_dropout_rate=a.final_layer_dropout_rate,
                spatial_pyramid_pooling=a.spatial_pyramid_pooling, skip_decoding=a.skip_decoding, seed=a.seed,
                use_graph=not getattr(a, "no_hip_graph", False), max_shots=_max_shots(a),
                matmul_precision=getattr(a, "matmul_precision", "fp32"),
                augment_batch_capacity=(max(16, a.inner_batch, a.eval_batch, getattr(a, "batch_size_search_range_high", 0) or 0)
                                        if augment_mode(a) == "device" else 0), **log)
    # --disable_rsd_residual_connections is a no-op in the reference too (kwarg name mismatch)


def _meta_fn(a):
    from .reptile import FOMLIS, Gecko
    if a.foml:
        return partial(FOMLIS, train_shots=a.train_shots, tail_shots=a.foml_tail,
                       sample_train_val_with_replacement=a.sample_foml_train_val_with_replacement)
    return Gecko


def train_kwargs(a) -> dict:
    if a.learning_rate_scheduler not in supported_learning_rate_schedulers:
        raise ValueError("Learning rate scheduler, {}, not in supported set: {}".format(a.learning_rate_scheduler,
                                                                                       supported_learning_rate_schedulers.keys()))
    return dict(num_classes=a.classes, num_shots=a.shots, train_shots=(a.train_shots or None), inner_batch_size=a.inner_batch,
                inner_iters=a.inner_iters, replacement=a.replacement, meta_step_size=a.meta_step, meta_step_size_final=a.meta_step_final,
                meta_batch_size=a.meta_batch, meta_iters=a.meta_iters, eval_inner_batch_size=a.eval_batch, eval_inner_iters=a.eval_iters,
                eval_interval=a.eval_interval, weight_decay_rate=a.weight_decay, transductive=a.transductive, meta_fn=_meta_fn(a),
                aug_rate=a.aug_rate, device_metrics=bool(getattr(a, "device_metrics", False)),
                **(dict(inner_loop_log=True, on_divergence=a.on_divergence) if inner_loop_log(a) else {}),
                **(dict(inner_loop_layer_log=True, inner_loop_layer_log_interval=a.inner_loop_layer_log_interval)
                   if inner_loop_layer_log(a) else {}))


def evaluate_kwargs(a) -> dict:
    return dict(num_classes=a.classes, num_shots=a.shots, eval_inner_batch_size=a.eval_batch, eval_inner_iters=a.eval_iters,
                replacement=a.replacement, weight_decay_rate=a.weight_decay, num_samples=a.eval_samples, transductive=a.transductive,
                meta_fn=_meta_fn(a), augment=augment_mode(a), lr=None, aug_rate=a.aug_rate,
                eval_tasks_with_median_early_stopping_iterations=a.eval_tasks_with_median_early_stopping_iterations,
                save_fine_tuned_checkpoints=a.save_fine_tuned_checkpoints, save_fine_tuned_checkpoints_dir=a.save_fine_tuned_checkpoints_dir,
                device_metrics=bool(getattr(a, "device_metrics", False)))


def prediction_writer(a, environ=None):
    """The predictions.PredictionWriter of --save-predictions / --save-prediction-overlays / SAVE_PREDICTIONS, or None.  Kept out of
    evaluate_kwargs: only the final evaluation passes save (not the hyperparameter search, the k-shot curves or meta-training)."""
    import os
    directory, overlays = getattr(a, "save_predictions", None), bool(getattr(a, "save_prediction_overlays", False))
    if (os.environ if environ is None else environ).get("SAVE_PREDICTIONS", ""):   # reptile.py:495-513: the reference's switch and directory
        directory, overlays = directory or "predictions", True
    if not directory:
        return None
    from .predictions import PredictionWriter
    return PredictionWriter(directory, overlays=overlays)


def hyper_search_kwargs(a) -> dict:
    """args.py:163-176."""
    from .hyperparam_search import SUPPORTED_SEARCH_ALGS
    assert a.uho_estimator in SUPPORTED_SEARCH_ALGS, "{} not in supported hyperparam search algs {}".format(a.uho_estimator, SUPPORTED_SEARCH_ALGS)
    return dict(lr_search_range_low=a.lr_search_range_low, lr_search_range_high=a.lr_search_range_high,
                drop_rate_search_range_low=a.drop_rate_search_range_low, drop_rate_search_range_high=a.drop_rate_search_range_high,
                aug_rate_search_range_low=a.aug_rate_search_range_low, aug_rate_search_range_high=a.aug_rate_search_range_high,
                batch_size_search_range_low=a.batch_size_search_range_low, batch_size_search_range_high=a.batch_size_search_range_high,
                estimator=a.uho_estimator)


def make_lr_scheduler(a):
    """run_metasegnet.py:55-65: the scheduler horizon is eval_inner_iters."""
    cls = supported_learning_rate_schedulers[a.learning_rate_scheduler]
    if cls is None:
        return None
    kw = {"decay_rate": a.step_decay_rate, "decay_after_n_steps": a.decay_after_n_steps} if "step" in a.learning_rate_scheduler else {}
    return cls(a.learning_rate, a.eval_iters, **kw)
