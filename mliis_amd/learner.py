"""EfficientLab learner: the MI355X replacement for `session.run(model.minimize_op, feed_dict)`.

Mirrors the handles the reference's meta-learner uses on the model object (models/efficientlab.py:42-61,94-100,108,173-176,
298-317) as methods:

    reference handle                                   here
    -------------------------------------------------  ------------------------------------------------
    sess.run(minimize_op, {X, Y[, lr_ph]})             Learner.inner_step(batch_idx, lr=None)
    sess.run(predictions, {X, is_training_ph: False})  Learner.predict(images, training=False)
    VariableState(trainable).export/import             Learner.export_trainable() / import_trainable()
    VariableState(global).export/import                Learner.export_all() / import_all()
    model.loss                                         Learner.last_loss (device scalar, read lazily)

One inner step = forward + backward + BN moving-average update + fused SGD/Adam apply, entirely on the device, in a fixed
sequence of C-ABI kernel launches over preallocated HBM buffers; after the first (eager) step of a given batch size the
sequence is captured into a HIP graph and replayed, so the host does no per-op work in the hot loop.

Graph semantics restated from: models/efficientlab.py:111-119,126-231,294-317; models/efficientnet/efficientnet_model.py:
253-290,396-441; models/efficientnet/utils.py:87-170.  Backward formulas: SURVEY.md Appendix B.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops, spec
from . import clip as clip_mod
from . import layerlog
from ._lib import MliisError, clip_lib, layerlog_lib, lib, loss_lib, region_lib, score_lib, steplog_lib, sweep_lib
from .arena import Arena
from .metrics import unpack_mask
from .passes import _Passes
from .plan import _Plan, layer_names
from .steplog import MIN_CAPACITY as MIN_LOG_CAPACITY
from .steplog import decode as decode_step_log
from .views import canonical as canonical_views


def _queue_ring_fetch(pin, ring, cursor):
    """Queue, on the current stream, the copies of a device ring and of its cursor into the pinned buffer `pin` (ring.numel() + 1 words)."""
    n = ring.numel()
    pin[:n].copy_(ring.view(-1), non_blocking=True)
    pin[n:].copy_(cursor, non_blocking=True)


class Learner(_Passes):
    def __init__(self, feature_extractor_name: str = "efficientnet-b0", image_size: int = 224, rsd: Optional[Sequence[int]] = (2, 4),
                 learning_rate: float = 1e-3, optimizer: str = "sgd", l2: bool = False, l1: bool = False, darc1: bool = False,
                 dice: bool = False, label_smoothing: float = 0.0, final_layer_dropout_rate: float = 0.0,
                 spatial_pyramid_pooling: bool = False, skip_decoding: bool = False, drop_connect: bool = True, seed: int = 0,
                 device="cuda:0", use_graph: bool = True, max_shots: int = 16, matmul_precision: str = "fp32",
                 small_fused: Optional[bool] = None, dw_march: Optional[bool] = None, fuse_bn2: Optional[bool] = None, fuse_head: Optional[bool] = None,
                 augment_batch_capacity: int = 0, rng_stream: int = 0, step_log: int = 0, layer_log: bool = False, grad_clip=None, clip_log: int = 0,
                 focal_gamma: float = 0.0, fg_weight: float = 1.0, tversky=None):
        if optimizer not in ("sgd", "adam"):
            raise ValueError("optimizer must be 'sgd' or 'adam' (Adam with beta1=0, the reference default)")
        if not torch.cuda.is_available():
            raise MliisError("mliis_amd.Learner needs an MI355X (HIP device); there is no CPU path")
        lib.load()  # fail loudly if the HIP extension is missing
        # focal_gamma G >= 0, fg_weight W > 0: the pixel term of the loss becomes -w (t0 p1^G l0 + t1 p0^G l1) with w = 1 + (W - 1) y1, over
        # N H W (include/mliis_loss.h) -- ops.head_focal_fused / ops.focal_ce where the step issues ops.head_ce_fused / ops.softmax_ce.
        # Active only when one of the two differs from its default; then the library is loaded here (a missing library is an error here,
        # not at the first step).  The scalars are by-value kernel arguments, captured into the step's graph: fixed at construction.
        # Inactive (the default): nothing is loaded or allocated and the step's launches are what they were.
        self.focal_gamma, self.fg_weight = float(focal_gamma), float(fg_weight)
        if not (math.isfinite(self.focal_gamma) and self.focal_gamma >= 0.0):
            raise ValueError("focal_gamma must be a finite float >= 0, got {!r}".format(focal_gamma))
        if not (math.isfinite(self.fg_weight) and self.fg_weight > 0.0):
            raise ValueError("fg_weight must be a finite float > 0, got {!r}".format(fg_weight))
        self.focal = self.focal_gamma != 0.0 or self.fg_weight != 1.0
        if self.focal:
            loss_lib.load()
        # tversky = (alpha, beta), both >= 0 and not both 0: the loss gains the region term -ln(2T / (T + 1)), T the batch mean of the Tversky
        # index (I + eps) / (I + alpha FP + beta FN + eps) on the channel-1 probability (include/mliis_region.h), whatever `dice` says --
        # (1, 1) is the dice term -- on the pixel term above: ops.head_tversky_fused / ops.tversky_ce where the step issues the heads and
        # chains above.  The library is loaded here; the pair is by-value kernel arguments, captured into the step's graph.  None (the
        # default): nothing is loaded or allocated and the step's launches are what they were.
        self.tversky = None
        if tversky is not None:
            try:
                alpha, beta = (float(v) for v in tversky)
            except (TypeError, ValueError):
                raise ValueError("tversky must be a pair (alpha, beta) of floats, got {!r}".format(tversky)) from None
            if not (math.isfinite(alpha) and math.isfinite(beta) and alpha >= 0.0 and beta >= 0.0 and alpha + beta > 0.0):
                raise ValueError("tversky needs finite alpha, beta >= 0 with alpha + beta > 0, got {!r}".format(tversky))
            self.tversky = (alpha, beta)
            region_lib.load()
        # operand precision of the matrix cores in the dense convs: "fp32" (BASELINE configs 1-3) or "bf16" (operands rounded to bf16 on
        # the fly, fp32 accumulation; everything else stays fp32).  Passed with every dense-conv call (nothing process-wide).
        # "bf16-storage" (BASELINE configs[3]): bf16 operands AND the expanded tensors of the MBConv blocks (z0, z1, a1 and their
        # gradients) stored as bf16 in HBM during training steps; statistics, sums, accumulators, block outputs, the decoder and the
        # master weights stay fp32; inference (predict) runs on fp32 tensors
        self.act_dtype = torch.float32
        if matmul_precision == "bf16-storage":
            matmul_precision, self.act_dtype = "bf16", torch.bfloat16
        # "fp32" multiplies the long-K decoder convs as fp32 EQUIVALENT products on the bf16 matrix cores (every operand value split
        # exactly into three bf16 terms, six term products, fp32 accumulation: csrc/conv_x3.hip -- closer to float64 than the fp32
        # instruction's own accumulation, 1.5x faster on the dominant launch); every other conv takes the native fp32 instruction.
        # "fp32-native": the native fp32 matrix instruction (v_mfma_f32_16x16x4_f32) everywhere.  Same tolerances in every parity test.
        self.x3_on = matmul_precision == "fp32"
        if matmul_precision == "fp32-native":
            matmul_precision = "fp32"
        if matmul_precision not in ops.PRECISIONS:
            raise ValueError("matmul_precision must be one of {}, 'fp32-native' or 'bf16-storage', got {!r}".format(sorted(ops.PRECISIONS), matmul_precision))
        self.matmul_precision = matmul_precision
        self._conv_fwd = functools.partial(ops.conv2d_fwd, precision=matmul_precision)
        self._conv_bwd_data = functools.partial(ops.conv2d_bwd_data, precision=matmul_precision)
        self._conv_bwd_filter = functools.partial(ops.conv2d_bwd_filter, precision=matmul_precision)
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.arch = spec.derive(feature_extractor_name, image_size, list(rsd or []), final_layer_dropout_rate, spatial_pyramid_pooling,
                                skip_decoding=bool(skip_decoding))
        self.feature_extractor_name = feature_extractor_name
        self.final_layer_scope = "decode/final_layer_weights"
        self.lr, self.optimizer = float(learning_rate), optimizer
        self.l2, self.dice, self.label_smoothing = bool(l2), bool(dice), float(label_smoothing)
        self.l1, self.darc1 = bool(l1), bool(darc1)
        self.final_layer_dropout_rate = float(final_layer_dropout_rate or 0.0)
        self.drop_connect = drop_connect
        # small-map blocks through the one-launch-per-direction kernels of mbconv_small.hip, the other blocks through the row-marching
        # kernels of dwmarch.hip; a block whose shape neither family takes (their *_supported queries) runs op by op (dwconv.hip).
        # small_fused / dw_march = False force that op-by-op path (tests of the fallback).
        self.small_fused = True if small_fused is None else bool(small_fused)
        self.dw_march = True if dw_march is None else bool(dw_march)
        # fuse_bn2 = True: a block's project batch norm (+ drop-connect, + identity skip) is applied by the NEXT block's expand conv while
        # it loads its rows (ops.conv2d_fwd_bnin: ten launches fewer per step).  Built and parity-tested in round 5, measured SLOWER
        # than the stand-alone apply launches (-0.8 % on the step: every one of the 390-512 workgroups of an expand conv needs all K
        # channels' statistics and folds all the producer's partial blocks itself -- 24-44 MB of redundant L2 reads per launch against
        # 3 MB in the 39-52 workgroups of the apply kernel; profiles/r05_notes.md), so OFF by default; MLIIS_FUSE_BN2=1 turns it on
        self.fuse_bn2 = (os.environ.get("MLIIS_FUSE_BN2") == "1") if fuse_bn2 is None else bool(fuse_bn2)
        # fuse_head = False: resize -> softmax cross-entropy -> gradient -> resize^T as four launches (the form before round 5)
        self.fuse_head = (os.environ.get("MLIIS_NO_FUSE_HEAD") is None) if fuse_head is None else bool(fuse_head)
        self.use_graph = use_graph
        self.stream = torch.cuda.Stream(device=self.device)
        # batch indices go up through a ring of pinned slots: an upload from pageable memory makes the host wait for this stream
        self._idx_pin = torch.empty((16, 64), dtype=torch.int32).pin_memory()
        self._idx_ev = [None] * 16
        self._idx_n = 0
        self.arena = Arena(self.arch, self.device)
        self.arena.init_weights(seed)
        self.variables_initialized = True
        self._capturing = False
        self.ws = ops.Workspace(self.device, 1 << 22, on_grow=self._on_workspace_grow)
        # K-contiguous ("HWOI") shadow of the dense-conv weights, refreshed by ONE batched transpose at the top of every
        # forward, so the forward GEMMs read their B operand as 16-byte k-fragments like backward-data does
        A = self.arena
        self.theta_t = torch.zeros_like(A.theta)
        fe = self.arch.name
        dense = [p for p in A.trainable if p.kind == "conv" and p.executed and "/se/" not in p.name and
                 p.name not in (f"{fe}/stem/conv2d/kernel", "decode/final_layer_weights/kernel")]
        desc = [[A.t_off[p.name], p.shape[0] * p.shape[1], p.shape[2], p.shape[3]] for p in dense]
        for p in A.trainable:   # the squeeze-excite reduce weights [C, R] too: the MLP's backward reads a column of them per channel
            if p.kind == "conv" and p.executed and p.name.endswith("/se/conv2d/kernel"):
                desc.append([A.t_off[p.name], 1, p.shape[2], p.shape[3]])
        self.wt_desc = torch.tensor(desc, dtype=torch.int32, device=self.device)
        self.wt_tiles = ops.transpose_tiles(desc)
        # fp8 mode: max |w| of every dense-conv weight, refreshed by the same launch that refreshes the shadow copies
        self.w_amax = torch.zeros(len(desc), dtype=torch.float32, device=self.device) if matmul_precision == "fp8" else None   # ([:len(dense)] used)
        self._amax_of = {}
        if self.w_amax is not None:
            self._amax_of = {p.name: self.w_amax[i:i + 1] for i, p in enumerate(dense)}
        self.wt = {p.name: self.theta_t[A.t_off[p.name]:A.t_off[p.name] + p.size] for p in A.trainable}
        self.lr_dev = torch.tensor([self.lr], dtype=torch.float32, device=self.device)
        self._lr_dev_val = float(self.lr)
        self.adam_v = torch.zeros_like(self.arena.theta) if optimizer == "adam" else None
        self.adam_t = torch.zeros(1, dtype=torch.float32, device=self.device)          # Adam steps applied so far
        self.adam_ticket = torch.zeros(1, dtype=torch.int32, device=self.device)   # the optimizer launch advances adam_t itself
        self.adam_epoch = 0     # bumped whenever the Adam slots are REPLACED from outside (restore / import_all): lanes follow (reptile.py)
        # step_log = CAPACITY > 0: every training step ends with one more launch (ops.steplog_append, captured into the step's graph like the
        # rest) that appends a record of the step -- loss / ce / iou, the rate, the gradient's norm and largest magnitude, the non-finite
        # counts of gradient and parameters -- to a ring of CAPACITY records in device memory; read_step_log() fetches them.  Fixed at
        # construction; 0 (the default): no buffer exists and the step issues exactly the launches it always did.
        self.step_log = int(step_log)
        if self.step_log < 0:
            raise ValueError("step_log is a ring capacity: 0 (off) or a positive number of records, got {}".format(step_log))
        self._log_ring = self._log_cursor = self._log_ws = self._log_pin = None
        self._log_seen = 0      # the device cursor at the last read_step_log() (or skip_step_log())
        self._log_issued = 0    # steps issued since construction: what the device cursor reaches once the stream has drained
        if self.step_log:
            steplog_lib.load()  # (a missing library is an error here, not at the first step)
            words = steplog_lib.size("mliis_steplog_record_words")
            self._log_ring = torch.zeros((self.step_log, words), dtype=torch.int32, device=self.device)
            self._log_cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._log_ws = ops.steplog_workspace(self.device)
            self._log_pin = torch.zeros(self.step_log * words + 1, dtype=torch.int32).pin_memory()
        # layer_log = True (needs step_log = CAPACITY > 0): two more launches in front of the step log's (ops.layerlog_append, captured with
        # it) write one record PER TRAINABLE TENSOR -- norm and largest magnitude of its gradient and of its parameters, their non-finite
        # counts and where the first one sits -- into row (step log cursor) % CAPACITY of a [CAPACITY, T] ring: row k is the step of the
        # step log's record k; read_layer_log() fetches them.  A second ring of the same size takes layer_delta()'s rows (||a - b|| per
        # tensor).  False (the default): nothing is allocated and the step issues the launches it issues without the argument.
        self.layer_log = bool(layer_log)
        if self.layer_log and not self.step_log:
            raise ValueError("layer_log=True needs a step log (step_log=CAPACITY > 0): its rows are addressed by the step log's cursor")
        self._layer_table = self._layer_ring = self._layer_ws = self._layer_pin = self._delta_ring = self._delta_ws = None
        self._log_window = (0, 0)   # the counter values the last read_step_log() read between
        if self.layer_log:
            layerlog_lib.load()  # (a missing library is an error here, not at the first step)
            A = self.arena
            self._layer_table = ops.layerlog_table([p.size for p in A.trainable], self.device)
            if self._layer_table.n != A.n_trainable_padded or \
                    any(int(q) * 4 != A.t_off[p.name] for q, p in zip(self._layer_table.segs[:, 0].tolist(), A.trainable)):
                raise MliisError("the per-tensor log's table does not follow the arena's layout")
            T, words = len(A.trainable), layerlog_lib.size("mliis_layerlog_record_words")
            self._layer_ring = torch.zeros((self.step_log, T, words), dtype=torch.int32, device=self.device)
            self._delta_ring = torch.zeros((self.step_log, T, words), dtype=torch.int32, device=self.device)
            self._layer_ws = ops.layerlog_workspace(self._layer_table)
            self._delta_ws = ops.layerlog_workspace(self._layer_table)
            self._layer_pin = torch.zeros(self.step_log * T * words + 1, dtype=torch.int32).pin_memory()
        # grad_clip = ("norm", C) | ("ratio", LAMBDA, EPS): two more launches between the backward pass and the optimizer launch
        # (ops.clip_apply, captured into the step's graph like the rest) bound the LOSS gradient in arena.grad in place -- by its global L2
        # norm, or per trainable tensor by LAMBDA * max(||theta_t||, EPS) -- in every training step; the L2 / L1 terms, which the optimizer
        # launch forms itself, stay outside the clip, and a gradient with a non-finite element is left exactly as it was.  One row of R
        # records (R = 1 / T) per step goes into a ring of clip_log rows (default steplog.MIN_CAPACITY) addressed by a device cursor of
        # its own; read_clip_log() fetches them.  Fixed at construction; None (the default): nothing is loaded or allocated and the step
        # issues the launches it issues without the argument.
        self.grad_clip = clip_mod.parse(grad_clip)
        self.clip_log = int(clip_log)
        if self.clip_log < 0 or (self.clip_log and self.grad_clip is None):
            raise ValueError("clip_log is the ring capacity of grad_clip: a positive number of rows with it, 0 without, got {}".format(clip_log))
        self._clip_table = self._clip_ws = self._clip_ring = self._clip_cursor = self._clip_pin = None
        self._clip_seen = 0      # the clip's device cursor at the last read_clip_log() (or skip_clip_log())
        self._clip_issued = 0    # steps issued since construction: what that cursor reaches once the stream has drained
        self._clip_fetched = False   # the pinned copy holds what the last read_step_log() fetched with its own copies
        if self.grad_clip is not None:
            clip_lib.load()  # (a missing library is an error here, not at the first step)
            A = self.arena
            self.clip_log = self.clip_log or MIN_LOG_CAPACITY
            self._clip_table = ops.clip_table([p.size for p in A.trainable], self.device)
            if self._clip_table.n != A.n_trainable_padded or \
                    any(int(q) * 4 != A.t_off[p.name] for q, p in zip(self._clip_table.segs[:, 0].tolist(), A.trainable)):
                raise MliisError("the clip's table does not follow the arena's layout")
            R, words = (len(A.trainable) if self.grad_clip[0] == "ratio" else 1), clip_lib.size("mliis_clip_record_words")
            self._clip_ring = torch.zeros((self.clip_log, R, words), dtype=torch.int32, device=self.device)
            self._clip_cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._clip_ws = ops.clip_workspace(self._clip_table)
            self._clip_pin = torch.zeros(self.clip_log * R * words + 1, dtype=torch.int32).pin_memory()
        self.plans: Dict[object, _Plan] = {}   # key: batch size (training plan) or (batch size, "infer") in bf16-storage mode
        self.max_shots = max_shots
        H = image_size
        # resident shots [0, max_shots) + (on-device augmentation) the slots of one augmented mini-batch behind them: the step's kernels
        # address images through an index vector, so an augmented batch is just another set of indices -- same HIP graph
        self.aug_capacity = int(augment_batch_capacity)
        self.shots_x = torch.zeros(max_shots + self.aug_capacity, H, H, 3, dtype=torch.float32, device=self.device)
        self.shots_y = torch.zeros(max_shots + self.aug_capacity, H, H, 2, dtype=torch.float32, device=self.device)
        if self.aug_capacity:
            self._alloc_augment_buffers()
        self.n_shots = 0
        self._aug_valid = 0   # samples of the last augment_batch() behind the resident shots (load_task() invalidates them)
        # device RNG of the stochastic ops (drop-connect, dropout): Philox state advanced by the mask kernel itself (csrc/rng.hip)
        # `seed` is the same on every rank (the weights must start identical); `rng_stream` -- the rank -- goes into the high word of
        # the Philox KEY only, so ranks that step in lock-step on different tasks do not draw identical drop-connect / dropout masks
        self.rng_state = ops.rng_state((int(seed) & 0xFFFFFFFF) ^ ((int(rng_stream) & 0xFFFFFFFF) << 32) if rng_stream else seed, self.device)
        self._dc_keeps = torch.tensor([1.0 - b.drop_rate for b in self.arch.executed() if b.skip] or [1.0], dtype=torch.float32, device=self.device)
        self.drop_keep_dev = torch.tensor([1.0 - self.final_layer_dropout_rate], dtype=torch.float32, device=self.device)
        self._drop_keep_val = 1.0 - self.final_layer_dropout_rate
        self._rng_now = None   # (generator state, mask plan) of a training step that draws its masks: set by _train_sequence, taken by _forward
        # variable names per layer (plan.layer_names): passes.py, the tools and the tests read them here
        self.n_stem, self.n_blocks, self.n_rsd, self.n_rsd_up, self.n_skipdec, self.n_final, self.n_aspp = layer_names(self.arch)
        # fp32x3: weight images of the decoder's 3x3 convs (the dilated branch over the whole concat, the fuse conv over its convolved
        # channels), both directions, re-split once per step beside the shadow transpose
        self.x3 = None
        if self.x3_on:
            self.x3 = ops.X3Images(self.device)
            shapes = {p.name: p.shape for p in A.trainable}
            for m, nm in zip(self.arch.rsd, self.n_rsd):
                (k0, _, _), (k1, _, _), (kf, _, _) = nm
                for name, cin in ((k1, None), (kf, 2 * m.c_out)):
                    kk, _, cin_total, cout = shapes[name]
                    win = cin_total if cin is None else cin
                    if ops.X3Images.eligible(win, cout, kk) and ops.X3Images.eligible(cout, win, kk):
                        self.x3.add(name, "fwd", A.t_off[name], kk, cin_total, cout, 0, win)
                        self.x3.add(name, "bwd", A.t_off[name], kk, cin_total, cout, 0, win)
            self.x3.finish()
        torch.cuda.synchronize(self.device)   # arena was initialised on the default stream; steps run on self.stream

    # ------------------------------------------------------------------------------------------- variable state
    @property
    def n_trainable(self) -> int:
        return self.arena.n_trainable

    def _out(self, t):
        """Hand a tensor produced on the learner stream to the caller's current stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            cur.wait_stream(self.stream)
            if torch.is_tensor(t):
                t.record_stream(cur)
        return t

    def _in(self):
        """Order the learner stream after work the caller queued on its current stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)

    def export_trainable(self) -> torch.Tensor:
        """Device clone of the (padded) trainable arena -- VariableState.export_variables (variables.py:70-74)."""
        with torch.cuda.stream(self.stream):
            t = self.arena.theta.clone()
        return self._out(t)

    def import_trainable(self, flat: torch.Tensor):
        self._in()
        with torch.cuda.stream(self.stream):
            self.arena.theta.copy_(flat)

    def export_bn(self) -> torch.Tensor:
        with torch.cuda.stream(self.stream):
            t = self.arena.bn_moving.clone()
        return self._out(t)

    def import_bn(self, flat: torch.Tensor):
        self._in()
        with torch.cuda.stream(self.stream):
            self.arena.bn_moving.copy_(flat)

    def export_all(self):
        """All global variables (trainable + BN moving [+ Adam slots]) -- Gecko._full_state (reptile.py:35-36,258)."""
        with torch.cuda.stream(self.stream):
            st = {"theta": self.arena.theta.clone(), "bn": self.arena.bn_moving.clone()}
            if self.adam_v is not None:
                st["adam_v"], st["adam_t"] = self.adam_v.clone(), self.adam_t.clone()
        for v in st.values():
            self._out(v)
        return st

    def import_all(self, st):
        """Restore every variable from an export_all() state of THIS run (the evaluation path's save / restore around a fine-tune,
        reptile.py: _evaluate): the lanes' second-moment history stays.  State from outside the run (a checkpoint) arrives through
        load_named, which advances adam_epoch so that concurrent lanes take over its Adam slots too."""
        self._in()
        with torch.cuda.stream(self.stream):
            self.arena.theta.copy_(st["theta"])
            self.arena.bn_moving.copy_(st["bn"])
            if self.adam_v is not None and "adam_v" in st:
                self.adam_v.copy_(st["adam_v"])
                self.adam_t.copy_(st["adam_t"])

    def import_adam(self, adam_v: torch.Tensor, adam_t: torch.Tensor):
        """Replace only the Adam slots (second moments + step count): how a lane takes over the main learner's restored optimizer state."""
        if self.adam_v is None:
            return
        self._in()
        with torch.cuda.stream(self.stream):
            self.adam_v.copy_(adam_v)
            self.adam_t.copy_(adam_t)
        self.adam_epoch += 1

    def axpby(self, a: float, x: torch.Tensor, b: float, y: torch.Tensor):
        """y <- a*x + b*y on flat arena-shaped buffers (meta_learners/variables.py:9-45 on the device)."""
        self._in()
        with torch.cuda.stream(self.stream):
            ops.axpby(a, x, b, y)

    def comm_context(self):
        """Context in which collectives on arena buffers must be issued (orders them after this learner's stream)."""
        return torch.cuda.stream(self.stream)

    def synchronize(self):
        self.stream.synchronize()

    def loss_value(self) -> float:
        self.stream.synchronize()
        return float(self.last_loss[0].item())

    ADAM_BETA2 = 0.999

    def named_numpy(self) -> Dict[str, np.ndarray]:
        """All global variables under their TF names, read after everything queued on the learner's stream has finished: what
        `tf.train.Saver()` stores (train.py:54,131) -- trainables, BN moving statistics and, for the Adam inner optimizer
        (--sgd absent), its persistent slots: `<var>/Adam_1` (second moment), `beta1_power` / `beta2_power` in TF's convention
        (beta^(t+1) after t steps; beta1 = 0).  The first-moment slot `<var>/Adam` equals the last gradient when beta1 = 0 and is
        not stored."""
        self.stream.synchronize()
        torch.cuda.synchronize(self.device)
        out = self.arena.named_numpy()
        if self.adam_v is not None:
            A = self.arena
            v = self.adam_v.detach().cpu().numpy()
            for p in A.trainable:
                o = A.t_off[p.name]
                out[p.name + "/Adam_1"] = v[o:o + p.size].reshape(p.shape).copy()
            from .checkpoint import adam_step_entries
            out.update(adam_step_entries(int(round(float(self.adam_t.item()))), self.ADAM_BETA2))
        return out

    def load_named(self, values, **kw) -> int:
        """Restore by name with the scope filters of EfficientLab.restore_model (prefixes / exclude_prefix / strict, forwarded to the
        arena).  The Adam slots follow the SAME filters (a final layer that is not restored keeps fresh slots too).  The step count
        (`beta2_power` / `adam_step`, top-level names) is restored unless a `prefixes` whitelist excludes it: restore_model's
        `filter_out_scope=final_layer_scope` keeps every global variable that does not start with that scope, the beta powers among
        them (efficientlab.py restore_model) -- so a --pretrained --do_not_restore_final_layer_weights run fine-tunes with a
        warm bias correction, as the reference does."""
        from .checkpoint import adam_step_from
        self.stream.synchronize()
        n = self.arena.load_named(values, **kw)
        if self.adam_v is not None:
            A = self.arena
            prefixes, exclude = kw.get("prefixes"), kw.get("exclude_prefix")
            for p in A.trainable:
                key = p.name + "/Adam_1"
                if key not in values:
                    continue
                if prefixes is not None and not any(p.name.startswith(x) for x in prefixes):
                    continue
                if exclude is not None and p.name.startswith(exclude):
                    continue
                o = A.t_off[p.name]
                self.adam_v[o:o + p.size].copy_(torch.from_numpy(np.asarray(values[key], dtype=np.float32).reshape(-1)))
            t = adam_step_from(values, self.ADAM_BETA2)
            if t is not None and prefixes is None:
                self.adam_t.fill_(float(t))
            self.adam_epoch += 1
        torch.cuda.synchronize(self.device)
        return n

    def disable_split_products(self):
        """Back to the native fp32 matrix instruction for the decoder convs (matmul_precision "fp32-native") on a live learner.
        Captured graphs hold the x3 launches: dropped, the next step of each plan is eager again."""
        if self.x3 is None:
            return
        self.stream.synchronize()
        self.x3 = None
        self.x3_on = False
        for P in self._destroy_graphs():
            P.steps_run = 0
        for P in self.plans.values():
            P.wbatch_ready = False   # (the deferred filter-gradient batch is launched with the learner's precision: rebuilt)

    def _on_workspace_grow(self, floats: int):
        """The shared scratch buffer is about to be replaced by a larger one (a plan with more images than any before).  Captured
        HIP graphs hold the old address: finish the queued work and drop them (the next step of each plan captures again)."""
        if self._capturing:
            raise MliisError("workspace would grow to {} floats during HIP-graph capture (the eager first step of a plan sizes it)".format(floats))
        self.stream.synchronize()
        for P in self._destroy_graphs():
            P.steps_run = 0   # next step eager (re-sizes), the one after captures

    def _destroy_graphs(self) -> List[_Plan]:
        """Destroy every captured graph of every plan; returns the plans that had any."""
        had = [P for P in self.plans.values() if P.graphs]
        for P in had:
            for gexec in P.graphs.values():
                lib.call("mliis_graph_destroy", gexec)
            P.graphs = {}
        return had

    # ------------------------------------------------------------------------------------------- task data
    def load_task(self, images, labels):
        """Make a task's shots resident: images [S,H,W,3] f32 0..255, labels [S,H,W,2] (numpy or tensors), or the pair of
        metaseg.ByteViews a ByteTask samples: their bytes are expanded (and resampled to the learner's image size) on the device."""
        from .metaseg import ByteView
        if isinstance(images, ByteView) or isinstance(labels, ByteView):
            return self._load_task_bytes(images, labels)
        images = torch.as_tensor(images)
        labels = torch.as_tensor(labels)
        S = images.shape[0]
        if S > self.max_shots:
            raise ValueError("task has {} shots; Learner was built with max_shots={}".format(S, self.max_shots))
        H = self.arch.image_size
        if tuple(images.shape[1:]) != (H, H, 3) or tuple(labels.shape) != (S, H, H, 2):
            raise ValueError("expected images [S,{0},{0},3] and labels [S,{0},{0},2], got {1} / {2}".format(H, tuple(images.shape),
                                                                                                    tuple(labels.shape)))
        self._in()
        with torch.cuda.stream(self.stream):
            self.shots_x[:S].copy_(images.to(torch.float32), non_blocking=True)
            self.shots_y[:S].copy_(labels.to(torch.float32), non_blocking=True)
        self.n_shots = S
        self._aug_valid = 0

    def _load_task_bytes(self, images, labels):
        """load_task for the (images, labels) ByteViews of one ByteTask: one launch of ops.task_expand_u8 on the learner's stream reads the
        byte pool and writes shots_x[:S] / shots_y[:S] -- no float copy of the task beside them and, for a pool resident on this device
        sampled as sample() samples it (its first S examples), no host-to-device traffic at all.  Any other selection uploads its S
        int32 rows; a pool that lives elsewhere (the host) uploads the selected examples' bytes, 4 per stored pixel."""
        from .metaseg import ByteView
        if not (isinstance(images, ByteView) and isinstance(labels, ByteView)) or images.task is not labels.task or images.kind != "x" or \
                labels.kind != "y" or len(images.shape) != 4 or len(labels.shape) != 4 or not np.array_equal(images.rows, labels.rows):
            raise ValueError("load_task: byte views come as the (images, labels) pair of one ByteTask over the same examples")
        task, S, H = images.task, int(images.rows.size), self.arch.image_size
        if S > self.max_shots:
            raise ValueError("task has {} shots; Learner was built with max_shots={}".format(S, self.max_shots))
        if task.image_size != H:
            raise ValueError("expected images [S,{0},{0},3] and labels [S,{0},{0},2], got {1} / {2}".format(H, images.shape, labels.shape))
        if S:
            pool_x, pool_y, idx = task.images_u8, task.masks_u8, None
            self._in()
            with torch.cuda.stream(self.stream):
                if pool_x.device != self.shots_x.device:
                    rows = images.rows.tolist()
                    pool_x = pool_x[rows].to(self.shots_x.device, non_blocking=True)
                    pool_y = pool_y[rows].to(self.shots_x.device, non_blocking=True)
                elif not images.is_prefix():
                    idx = torch.from_numpy(images.rows.astype(np.int32)).to(self.shots_x.device, non_blocking=True)
                ops.task_expand_u8(pool_x, pool_y, idx, self.shots_x[:S], self.shots_y[:S])
        self.n_shots = S
        self._aug_valid = 0

    def _alloc_augment_buffers(self):
        """What augment_batch() needs besides the batch slots behind the shots: the ping-pong buffers of a multi-stage recipe, the device
        copy of a batch's encoded stages and the ring of pinned slots (with their events) it is uploaded through."""
        H = self.arch.image_size
        self._aug_tmp_x = torch.zeros(self.aug_capacity, H, H, 3, dtype=torch.float32, device=self.device)
        self._aug_tmp_y = torch.zeros(self.aug_capacity, H, H, 2, dtype=torch.float32, device=self.device)
        self._aug_ops_dev = torch.zeros(8 * self.aug_capacity * 48, dtype=torch.uint8, device=self.device)
        self._aug_ops_pin = torch.zeros((4, 8 * self.aug_capacity * 48), dtype=torch.uint8).pin_memory()
        self._aug_ev = [None] * 4
        self._aug_n = 0

    def reserve_augment_capacity(self, n: int):
        """Give a learner that was built with fewer (or no) augmentation slots `n` of them (augment_batch_capacity=n after the fact): the
        resident shots move into a larger allocation with the batch slots behind them, contents kept.  Captured graphs hold the old
        address and a plan may have been sized against it, so this is only allowed while the learner has neither."""
        n = int(n)
        if self.plans:
            raise ValueError("reserve_augment_capacity: the learner has already stepped (plans / captured graphs hold the shot buffers)")
        if n <= self.aug_capacity:
            return
        H = self.arch.image_size
        self.stream.synchronize()
        self._in()
        with torch.cuda.stream(self.stream):
            for name, ch in (("shots_x", 3), ("shots_y", 2)):
                old = getattr(self, name)
                new = torch.zeros(self.max_shots + n, H, H, ch, dtype=torch.float32, device=self.device)
                new[:old.shape[0]].copy_(old)
                setattr(self, name, new)
        self.aug_capacity = n
        self._alloc_augment_buffers()
        self._aug_valid = 0
        torch.cuda.synchronize(self.device)   # (the old buffers are released and the new ones zeroed before anything else runs)

    def augment_batch(self, src_idx: Sequence[int], recipes) -> List[int]:
        """On-device augmentation of one mini-batch (csrc/augment.hip): sample b = shot src_idx[b] of the resident task through the
        planned steps recipes[b] (mliis_amd.augment.Augmenter(fields=False).plan; None = the original).  Returns the indices of the
        augmented samples -- slots behind the resident shots -- to hand to inner_step()."""
        from .augment import encode_device_ops
        B = len(src_idx)
        if not self.aug_capacity or B > self.aug_capacity:
            raise ValueError("Learner was built with augment_batch_capacity={}; batch has {} samples".format(self.aug_capacity, B))
        if max(src_idx) >= self.n_shots or min(src_idx) < 0:
            raise ValueError("augment_batch: shot index out of range of the resident task ({} shots)".format(self.n_shots))
        ops_np = encode_device_ops(recipes, src_idx)
        n = ops_np.shape[0]
        if n > 8:
            raise ValueError("at most 8 augmentation stages per sample")
        base = self.max_shots
        for i in range(n):    # stage i reads: the shots (i = 0) or the previous stage's output; the LAST stage writes the batch slots
            prev_in_shots = i > 0 and (n - 1 - (i - 1)) % 2 == 0
            ops_np[i]["src"] = np.asarray(src_idx, dtype=np.int32) if i == 0 else (np.arange(B, dtype=np.int32) + (base if prev_in_shots else 0))
        H = self.arch.image_size
        nbytes = ops_np.nbytes
        with torch.cuda.stream(self.stream):
            slot = self._aug_n % 4
            self._aug_n += 1
            if self._aug_ev[slot] is not None:
                self._aug_ev[slot].synchronize()
            else:
                self._aug_ev[slot] = torch.cuda.Event()
            pin = self._aug_ops_pin[slot, :nbytes]
            pin.copy_(torch.from_numpy(ops_np.reshape(-1).view(np.uint8)))
            dev = self._aug_ops_dev[:nbytes]
            dev.copy_(pin, non_blocking=True)
            self._aug_ev[slot].record(self.stream)
            for i in range(n):
                to_shots = (n - 1 - i) % 2 == 0
                from_shots = i == 0 or (n - 1 - (i - 1)) % 2 == 0
                xin, yin = (self.shots_x, self.shots_y) if from_shots else (self._aug_tmp_x, self._aug_tmp_y)
                xout, yout = (self.shots_x, self.shots_y) if to_shots else (self._aug_tmp_x, self._aug_tmp_y)
                if xin is xout:   # (stage 0 reading the shots and writing the batch slots of the same allocation: disjoint sample ranges)
                    xin_p, yin_p = xin.data_ptr(), yin.data_ptr()
                    xout_p, yout_p = xout[base:].data_ptr(), yout[base:].data_ptr()
                    ob = 0
                else:
                    xin_p, yin_p, xout_p, yout_p, ob = xin.data_ptr(), yin.data_ptr(), xout.data_ptr(), yout.data_ptr(), (base if to_shots else 0)
                lib.call("mliis_augment_stage", xin_p, yin_p, xout_p, yout_p, dev.data_ptr() + i * B * 48, B, H, H, ob, self.stream.cuda_stream)
        self._aug_valid = B
        return [base + b for b in range(B)]

    def _plan(self, N: int, infer: bool = False) -> _Plan:
        """The buffers of a batch size.  bf16-storage mode keeps a second, fp32 plan for inference (the op-by-op inference kernels read
        fp32 tensors); in every other mode training and inference share one."""
        key = (N, "infer") if (infer and self.act_dtype != torch.float32) else N
        if key not in self.plans:
            with torch.cuda.stream(self.stream):
                self.plans[key] = _Plan(self, N, torch.float32 if isinstance(key, tuple) else self.act_dtype)
        return self.plans[key]

    # ------------------------------------------------------------------------------------------- one optimisation step
    def _apply(self):
        A = self.arena
        l2 = spec.L2_WEIGHT if self.l2 else 0.0
        l1 = spec.L2_WEIGHT if self.l1 else 0.0     # (models/regularizers.py:13: the same 5e-4 default)
        if self.optimizer == "sgd":
            ops.sgd_fused(A.theta, A.grad, self.lr, A.l2_quad_mask, l2, self.lr_dev, l1=l1)
        else:
            # (the launch reads the step count from device memory, uses t + 1 and stores it: the same graph replays every step)
            ops.adam_b1zero_fused(A.theta, A.grad, self.adam_v, self.adam_t, self.lr, A.l2_quad_mask, l2, self.lr_dev, l1=l1,
                                  ticket=self.adam_ticket)

    def _train_sequence(self, P: _Plan, draw_masks: bool):
        # (the masks of the step are drawn by the launch that builds the weight shadows at the head of the forward pass: passes.py)
        self._rng_now = (self.rng_state, P.mask_plan) if (draw_masks and P.mask_plan is not None) else None
        # Without the dice term (and DARC1, which reads the full-resolution logits) the tail of the step -- resize to the image size,
        # softmax cross-entropy, its gradient, the resize's transpose -- is ONE launch on the decoder's map (ops.head_ce_fused)
        hd_, H_ = self.arch.h_dec, self.arch.image_size
        hlib, hname = (loss_lib, "mliis_head_focal_fused") if self.focal else (lib, "mliis_head_ce_fused")
        if self.tversky is not None:   # (the region term is the head's own second pass: `dice` does not keep it off the decoder's map)
            hlib, hname = region_lib, "mliis_head_tversky_fused"
        head_fused = bool(self.fuse_head and (self.tversky is not None or not self.dice) and not self.darc1 and
                          hlib.size(hname + "_supported", hd_, hd_, H_, H_))
        logits = self._forward(P, self.shots_x, P.idx, True, upsample=not head_fused)
        if head_fused:
            if P.head_ws is None:
                wdims = (P.N, hd_, hd_, H_, H_) if self.tversky is not None else (P.N, hd_, hd_)
                P.head_ws = ops.Workspace(self.device, hlib.size(hname + "_workspace_floats", *wdims))
            if self.tversky is not None:   # THREE launches on the decoder's map: the sums, their fold, the gradient tiles
                ops.head_tversky_fused(P.small, self.shots_y, P.idx, (H_, H_), self.label_smoothing, self.focal_gamma, self.fg_weight,
                                       self.tversky[0], self.tversky[1], P.dsmall, P.loss_out, ws=P.head_ws)
                P.head_fin = None
            elif self.focal:   # TWO launches: the focal head and its own fold (the other library's backward-data launch cannot fold for it)
                ops.head_focal_fused(P.small, self.shots_y, P.idx, (H_, H_), self.label_smoothing, self.focal_gamma, self.fg_weight, P.dsmall,
                                     P.loss_out, ws=P.head_ws)
                P.head_fin = None
            else:   # ONE launch: the fold of the loss partials rides in the final conv's backward-data launch (passes.py)
                _, _, buf = ops.head_ce_fused(P.small, self.shots_y, P.idx, (H_, H_), self.label_smoothing, P.dsmall, P.loss_out, ws=P.head_ws,
                                              finalize=False)
                P.head_fin = (buf, (H_, H_), 0.0, P.loss_out)
        else:
            if self.tversky is not None:
                ops.tversky_ce(logits, self.shots_y, P.idx, self.label_smoothing, self.focal_gamma, self.fg_weight, self.tversky[0], self.tversky[1],
                               0.0, want_grad=True, dlogits=P.dlogits, out=P.loss_out, ws=self.ws)
            elif self.focal:
                ops.focal_ce(logits, self.shots_y, P.idx, self.label_smoothing, self.focal_gamma, self.fg_weight, self.dice, 0.0, want_grad=True,
                             dlogits=P.dlogits, out=P.loss_out, ws=self.ws)
            else:
                ops.softmax_ce(logits, self.shots_y, P.idx, self.label_smoothing, self.dice, 0.0, want_grad=True, want_pred=False,
                               dlogits=P.dlogits, out=P.loss_out, ws=self.ws)
            if self.darc1:
                ops.darc1(logits, spec.L2_WEIGHT, dlogits=P.dlogits, out=P.loss_out, ws=self.ws)
        self._backward(P, self.shots_x, P.idx, head_fused=head_fused)
        if self.grad_clip is not None:   # arena.grad is the loss gradient as the backward pass left it; _apply() consumes what this leaves
            mode, threshold, eps = self.grad_clip
            ops.clip_apply(self.arena.grad, self.arena.theta, self._clip_table, self._clip_ws, self._clip_cursor, mode, threshold, eps,
                           out=self._clip_ring)
        self._apply()
        if self.layer_log:   # the same two arenas per tensor, into the row the step log's cursor names (read here, advanced below)
            ops.layerlog_append(self.arena.grad, self.arena.theta, self._layer_table, self._layer_ws, self._log_cursor, out=self._layer_ring)
        if self.step_log:   # the step's record: P.loss_out is final here, arena.grad is what _apply() consumed, theta what it left
            ops.steplog_append(P.loss_out, self.lr_dev, self.arena.grad, self.arena.theta, self._log_ws, self._log_cursor, out=self._log_ring)

    def _upload_idx(self, P: _Plan, idx: Sequence[int]):
        """A batch's image indices into P.idx through the ring of pinned slots (call on the learner's stream): inner_step's upload, for
        the callers outside the training step (score_resident).  inner_step keeps its own inline form -- the training step's code is
        left exactly as it was; the two share the ring (slots, events, counter)."""
        N = len(idx)
        if N <= self._idx_pin.shape[1]:
            slot = self._idx_n % len(self._idx_ev)
            self._idx_n += 1
            if self._idx_ev[slot] is not None:
                self._idx_ev[slot].synchronize()   # the upload that last used this slot (16 uploads ago) has been consumed
            else:
                self._idx_ev[slot] = torch.cuda.Event()
            src = self._idx_pin[slot, :N]
            src.copy_(torch.tensor(list(idx), dtype=torch.int32))
            ops.copy_words(src, P.idx)   # one small kernel reading the pinned slot: no copy engine between two steps
            self._idx_ev[slot].record(self.stream)
        else:
            P.idx.copy_(torch.tensor(list(idx), dtype=torch.int32), non_blocking=True)

    def inner_step(self, batch_idx: Sequence[int], lr: Optional[float] = None, dc_scales: Optional[Dict[int, torch.Tensor]] = None,
                   dropout_mask: Optional[torch.Tensor] = None, weight_decay_rate: float = 1.0, drop_rate: Optional[float] = None,
                   aspp_masks: Optional[Sequence[torch.Tensor]] = None):
        """One `session.run(minimize_op)` on images `batch_idx` of the resident task.  Returns the device loss scalar.
        `drop_rate` overrides the final-layer dropout rate for this step (the reference feeds `final_layer_dropout_rate_ph`, a
        placeholder that only exists when the model was built with dropout, models/efficientlab.py:94-100)."""
        N = len(batch_idx)
        if N == 0:
            raise ValueError("empty mini-batch")
        lim = self.max_shots + self._aug_valid if self._aug_valid else self.n_shots
        if min(batch_idx) < 0 or max(batch_idx) >= lim or any(self.n_shots <= i < self.max_shots for i in batch_idx):
            raise ValueError("batch index out of range of the resident task ({} shots)".format(self.n_shots))
        P = self._plan(N)
        with torch.cuda.stream(self.stream):
            if N <= self._idx_pin.shape[1]:
                slot = self._idx_n % len(self._idx_ev)
                self._idx_n += 1
                if self._idx_ev[slot] is not None:
                    self._idx_ev[slot].synchronize()   # the upload that last used this slot (16 steps ago) has been consumed
                else:
                    self._idx_ev[slot] = torch.cuda.Event()
                src = self._idx_pin[slot, :N]
                src.copy_(torch.tensor(list(batch_idx), dtype=torch.int32))
                ops.copy_words(src, P.idx)   # one small kernel reading the pinned slot: no copy engine between two steps
                self._idx_ev[slot].record(self.stream)
            else:
                P.idx.copy_(torch.tensor(list(batch_idx), dtype=torch.int32), non_blocking=True)
            lr_now = self.lr if lr is None else float(lr)
            if lr_now != self._lr_dev_val:   # the fused optimizer kernels read the rate from device memory (graph-replay safe)
                self.lr_dev.fill_(lr_now)
                self._lr_dev_val = lr_now
            if weight_decay_rate != 1.0:  # pre_step_op (variables.py:48-55)
                ops.axpby(0.0, None, float(weight_decay_rate), self.arena.theta)
            draw = self._fill_masks(P, dc_scales, dropout_mask, drop_rate, aspp_masks)
            if self.use_graph and P.steps_run >= 1:
                if draw not in P.graphs:
                    gexec = C.c_void_p()
                    lib.call("mliis_graph_begin_capture", self.stream.cuda_stream)
                    self._capturing = True
                    try:
                        self._train_sequence(P, draw)
                    finally:
                        self._capturing = False
                        lib.call("mliis_graph_end_capture", self.stream.cuda_stream, C.byref(gexec))
                    P.graphs[draw] = gexec
                lib.call("mliis_graph_launch", P.graphs[draw], self.stream.cuda_stream)
            else:
                self._train_sequence(P, draw)
            P.steps_run += 1
        if self.step_log:
            self._log_issued += 1
        if self.grad_clip is not None:
            self._clip_issued += 1
        self.last_loss = P.loss_out
        return P.loss_out

    # ------------------------------------------------------------------------------------------- step log
    def read_step_log(self):
        """(records, dropped): the records of the inner steps taken since the last call (or skip_step_log()), in step order, as a
        steplog.RECORD_DTYPE array, and the number of steps whose records the ring no longer held -- more steps ran than step_log records
        fit, and the oldest were overwritten.  Waits for the learner's stream; ring and cursor come back through pinned memory in one
        copy each.  This is the only host synchronisation the log costs: the steps themselves append on the device."""
        if not self.step_log:
            raise MliisError("this Learner was built without a step log (step_log=0)")
        n = self._log_ring.numel()
        with torch.cuda.stream(self.stream):
            _queue_ring_fetch(self._log_pin, self._log_ring, self._log_cursor)
            if self.grad_clip is not None:   # the clip's ring rides along: read_clip_log(last_read=True) needs no wait of its own
                _queue_ring_fetch(self._clip_pin, self._clip_ring, self._clip_cursor)
        self.stream.synchronize()
        self._clip_fetched = self.grad_clip is not None
        host = self._log_pin.numpy()
        cursor = int(host[n]) & 0xFFFFFFFF
        records, dropped = decode_step_log(host[:n].reshape(self.step_log, -1), cursor, self._log_seen)
        self._log_window = (self._log_seen, cursor)
        self._log_seen = cursor
        return records, dropped

    def step_log_pending(self) -> int:
        """Steps issued since the last read_step_log() / skip_step_log() (host count: nothing is read from the device)."""
        return (self._log_issued - self._log_seen) & 0xFFFFFFFF

    def skip_step_log(self):
        """Forget the records of the steps issued so far without reading them (no synchronisation): the next read_step_log() starts behind
        them."""
        self._log_seen = self._log_issued & 0xFFFFFFFF

    # ------------------------------------------------------------------------------------------- gradient clipping
    def read_clip_log(self, last_read: bool = False):
        """(records [steps, R], dropped): the clip's rows (clip.RECORD_DTYPE; R = 1 by global norm, R = T tensors in arena order per
        tensor) of the training steps taken since the last call (or skip_clip_log()), in step order, and the number of steps whose rows
        the ring no longer held.  Waits for the learner's stream.  last_read=True (needs a step log): the rows of exactly the steps the
        LAST read_step_log() returned, from the copy that call fetched beside its own -- nothing is waited for, queued or consumed (the
        clip's cursor and the step log's count the same steps)."""
        if self.grad_clip is None:
            raise MliisError("this Learner was built without gradient clipping (grad_clip=None)")
        n = self._clip_ring.numel()
        if last_read:
            if not self._clip_fetched:
                raise MliisError("read_clip_log(last_read=True) follows a read_step_log()")
            host = self._clip_pin.numpy()
            first, end = self._log_window
            return clip_mod.decode(host[:n].reshape(tuple(self._clip_ring.shape)), end, first)
        with torch.cuda.stream(self.stream):
            _queue_ring_fetch(self._clip_pin, self._clip_ring, self._clip_cursor)
        self.stream.synchronize()
        self._clip_fetched = False
        host = self._clip_pin.numpy()
        cursor = int(host[n]) & 0xFFFFFFFF
        records, dropped = clip_mod.decode(host[:n].reshape(tuple(self._clip_ring.shape)), cursor, self._clip_seen)
        self._clip_seen = cursor
        return records, dropped

    def skip_clip_log(self):
        """Forget the clip rows of the steps issued so far without reading them (no synchronisation)."""
        self._clip_seen = self._clip_issued & 0xFFFFFFFF

    # ------------------------------------------------------------------------------------------- per-tensor log
    @property
    def layer_log_names(self) -> List[str]:
        """The tensor names of a layer-log row, in table order (arena.trainable)."""
        return [p.name for p in self.arena.trainable]

    def _fetch_layer_ring(self, ring):
        """(host words [rows, T, 8], device cursor) after the learner's stream has drained; ring and cursor through pinned memory."""
        n = ring.numel()
        with torch.cuda.stream(self.stream):
            _queue_ring_fetch(self._layer_pin, ring, self._log_cursor)
        self.stream.synchronize()
        host = self._layer_pin.numpy()
        return host[:n].reshape(tuple(ring.shape)), int(host[n]) & 0xFFFFFFFF

    def read_layer_log(self, last_read: bool = False):
        """(records [steps, T], dropped): the per-tensor rows (layerlog.RECORD_DTYPE: x = gradient, y = parameters; T tensors in
        layer_log_names order) of the steps read_step_log() would return now, and how many of those steps' rows the ring no longer held.
        Nothing is consumed: the "seen" cursor is the step log's and only read_step_log() / skip_step_log() advance it, so the rows stay
        readable until then -- and after it as well: last_read=True returns the rows of exactly the steps the LAST read_step_log()
        returned (as far as the ring still holds them: steps issued since then overwrite the oldest).  Waits for the learner's stream."""
        if not self.layer_log:
            raise MliisError("this Learner was built without a per-tensor log (layer_log=False)")
        host, cursor = self._fetch_layer_ring(self._layer_ring)
        if not last_read:
            return layerlog.decode(host, cursor, self._log_seen)
        first, end = self._log_window
        records, dropped = layerlog.decode(host, end, first)
        lost = min(len(records), max(0, ((cursor - first) & 0xFFFFFFFF) - self.step_log - dropped))   # overwritten since that read
        return records[lost:], dropped + lost

    def layer_delta(self, a: torch.Tensor, b: torch.Tensor, row: int):
        """Launch, on the learner's stream, the per-tensor reduction of a - b (and of b) into row `row` of the delta ring: a, b arena-shaped
        fp32 device buffers (export_trainable()'s layout).  read_layer_deltas() fetches rows."""
        if not self.layer_log:
            raise MliisError("this Learner was built without a per-tensor log (layer_log=False)")
        if not 0 <= int(row) < self.step_log:
            raise ValueError("layer_delta row {} outside the ring of {} rows".format(row, self.step_log))
        self._in()
        with torch.cuda.stream(self.stream):
            for t in (a, b):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(self.stream)
            ops.layerlog_append(a, b, self._layer_table, self._delta_ws, None, out=self._delta_ring, row_offset=int(row), mode="delta")

    def read_layer_deltas(self, rows: Sequence[int]) -> np.ndarray:
        """records [len(rows), T] of the delta ring (layerlog.RECORD_DTYPE: x = a - b, y = b).  Waits for the learner's stream."""
        if not self.layer_log:
            raise MliisError("this Learner was built without a per-tensor log (layer_log=False)")
        rows = [int(r) for r in rows]
        if any(not 0 <= r < self.step_log for r in rows):
            raise ValueError("layer delta rows {} outside the ring of {} rows".format(rows, self.step_log))
        host, _ = self._fetch_layer_ring(self._delta_ring)
        return host.view(np.uint32)[rows].copy().view(layerlog.RECORD_DTYPE).reshape(len(rows), host.shape[1])

    def _fill_masks(self, P: _Plan, dc_scales, dropout_mask, drop_rate=None, aspp_masks=None) -> bool:
        """Masks handed in by the caller (parity tests) are copied into the plan's buffers; returns True when the step has to draw its
        masks itself -- on the device, inside the step (ops.rng_masks: no host RNG and no torch op on the path)."""
        if drop_rate is not None and P.drop_mask is None:
            raise ValueError("drop_rate given but the model was built without final-layer dropout (final_layer_dropout_rate = 0)")
        if drop_rate is not None and not 0.0 <= float(drop_rate) < 1.0:
            raise ValueError("drop_rate must be in [0, 1), got {}".format(drop_rate))
        injected = dc_scales is not None or dropout_mask is not None or aspp_masks is not None
        if P.drop_mask is not None and dropout_mask is None:   # keep probability of the final-layer dropout: a device scalar (graph-replay safe)
            keep = 1.0 - (self.final_layer_dropout_rate if drop_rate is None else float(drop_rate))
            if keep != self._drop_keep_val:
                self.drop_keep_dev.fill_(keep)
                self._drop_keep_val = keep
        if not injected:
            return P.mask_plan is not None
        # ---- injected masks: every stochastic site not given explicitly is drawn once here with the same device generator
        if P.mask_plan is not None:
            ops.rng_masks(self.rng_state, P.mask_plan)
        if P.aspp is not None and aspp_masks is not None:   # four tf.layers.dropout(rate=0.5) sites: scale 0 or 1/keep
            for i, mbuf in enumerate(P.aspp["masks"]):
                mbuf.copy_(torch.as_tensor(aspp_masks[i], dtype=torch.float32).reshape(mbuf.shape))
        if self.drop_connect and dc_scales is not None:
            for b, B in zip(self.arch.executed(), P.blocks):
                if b.skip and "dc" in B:
                    v = dc_scales.get(b.idx)
                    if v is None:
                        B["dc"].fill_(1.0)
                    else:
                        B["dc"].copy_(torch.as_tensor(v, dtype=torch.float32))
        if P.drop_mask is not None and dropout_mask is not None:
            P.drop_mask.copy_(torch.as_tensor(dropout_mask, dtype=torch.float32))
        return False

    # ------------------------------------------------------------------------------------------- inference
    def _forward_views(self, P: _Plan, x, idx, training: bool, views):
        """Flip test-time augmentation (views: a canonical, non-empty tuple of views.VIEWS): P.small = the mean of the decoder-resolution
        logits of the batch and of its mirrored views, each view's logits mirrored back,
            merged = (z_id + (F_v1(z_v1) + F_v2(z_v2) + ...)) * fl32(1 / (K + 1))          fp32, every sum and the product rounded once.
        Per view: ops.view_gather mirrors the whole batch into P.view_x, one more forward pass of the same mode runs on it, ops.view_merge
        mirrors its logits back into the running sum P.view_acc (the first view is stored as it is, not added to zero); then the identity
        pass exactly as without views, and one in-place merge into P.small.  Flips commute with the align-corners resize, so everything
        downstream reads P.small as always.  Logits are averaged, not probabilities.  Call on the learner's stream."""
        H, hd = self.arch.image_size, self.arch.h_dec
        if P.view_x is None:
            P.view_x = torch.zeros((P.N, H, H, 3), dtype=torch.float32, device=self.device)
            P.view_acc = torch.zeros((P.N, hd, hd, 2), dtype=torch.float32, device=self.device)
        for k, v in enumerate(views):
            ops.view_gather(x, idx, v, out=P.view_x)
            self._forward(P, P.view_x, None, training, upsample=False, stochastic=False)
            ops.view_merge(P.view_acc, P.view_acc if k else None, P.small, v, 1.0)
        self._forward(P, x, idx, training, upsample=False, stochastic=False)
        ops.view_merge(P.small, P.small, P.view_acc, (False, False), 1.0 / (len(views) + 1))

    def predict(self, images, training: bool = False, return_logits: bool = False, views=()):
        """predictions tensor of the reference: (softmax(logits) > 0.5) as float, [N,H,W,2].  training=True: batch statistics in every
        batch norm; the stochastic sites (drop-connect, final-layer and ASPP dropout) stay off -- their masks belong to a training step.
        views: flip test-time augmentation (_forward_views); () = off, the launches of a call without the keyword."""
        views = canonical_views(views)
        images = torch.as_tensor(images)
        N = images.shape[0]
        P = self._plan(N, infer=True)
        with torch.cuda.stream(self.stream):
            x = images.to(device=self.device, dtype=torch.float32).contiguous()
            if views:
                self._forward_views(P, x, None, training, views)
                H = self.arch.image_size
                logits = ops.resize_bilinear_fwd(P.small, (H, H), out=P.logits)
            else:
                logits = self._forward(P, x, None, training, stochastic=False)
            dummy = torch.zeros_like(logits)
            ops.softmax_ce(logits, dummy, None, 0.0, False, 0.0, want_grad=False, want_pred=True, pred=P.pred, out=P.loss_out, ws=self.ws)
            out = P.pred.clone()
            lg = logits.clone() if return_logits else None
        self.stream.synchronize()
        return (out, lg) if return_logits else out

    def predict_resident(self, idx: Sequence[int], training: bool = False, views=()):
        """predict() on images `idx` of the task made resident by load_task()."""
        views = canonical_views(views)
        with torch.cuda.stream(self.stream):
            x = self.shots_x[torch.tensor(list(idx), dtype=torch.long, device=self.device)]
        return self.predict(x, training=training, views=views) if views else self.predict(x, training=training)

    def score_resident(self, idx: Sequence[int], training: bool = False, views=()) -> np.ndarray:
        """The score of predict_resident(idx) against the resident labels without its mask: int64 [len(idx), 4] =
        {|P & L|, |P | L|, |P|, |L|} per image (ops.mask_iou_counts; metrics.iou_from_counts(row[0], row[1]) is metrics.iou of that
        image's prediction).  The images are read through the index vector and the decoder-resolution logits are scored in place: no
        gather, no resize launch, no full-resolution tensor, 16 bytes per image back to the host.  views: flip test-time augmentation
        (_forward_views: the counts are those of the merged logits); () = off, the launches of a call without the keyword."""
        views = canonical_views(views)
        idx = [int(i) for i in idx]
        N = len(idx)
        if N == 0:
            raise ValueError("empty batch")
        lim = self.max_shots + self._aug_valid if self._aug_valid else self.n_shots
        if min(idx) < 0 or max(idx) >= lim or any(self.n_shots <= i < self.max_shots for i in idx):
            raise ValueError("image index out of range of the resident task ({} shots)".format(self.n_shots))
        P = self._plan(N, infer=True)
        H = self.arch.image_size
        with torch.cuda.stream(self.stream):
            if P.counts is None:
                P.counts = torch.zeros((N, 4), dtype=torch.int32, device=self.device)
                P.counts_pin = torch.zeros((N, 4), dtype=torch.int32).pin_memory()
            self._upload_idx(P, idx)
            if views:
                self._forward_views(P, self.shots_x, P.idx, training, views)
            else:
                self._forward(P, self.shots_x, P.idx, training, upsample=False, stochastic=False)
            ops.mask_iou_counts(P.small, self.shots_y, P.idx, (H, H), counts=P.counts)
            P.counts_pin.copy_(P.counts, non_blocking=True)
        self.stream.synchronize()
        return P.counts_pin.numpy().astype(np.int64)

    def mask_resident(self, idx: Sequence[int], training: bool = False, counts: bool = False, last_only: bool = False, views=()):
        """The prediction masks of predict_resident(idx) -- bool [len(idx), H, W], = predict_resident(idx)[..., 1] > 0.5 -- read back as one
        bit per pixel (ops.mask_pack on the decoder-resolution logits of score_resident's forward pass; metrics.unpack_mask on the host):
        H W / 8 bytes per image instead of the 8 H W of the fp32 prediction tensor.  counts=True: (masks, int64 [len(idx), 4]), the rows of
        score_resident from the same launch.  last_only=True: only the last image of the batch is packed and returned ([1,H,W] / [1,4]) --
        the per-sample evaluation's "train images + one test image, keep the last".  views: as in score_resident."""
        views = canonical_views(views)
        idx = [int(i) for i in idx]
        N = len(idx)
        if N == 0:
            raise ValueError("empty batch")
        lim = self.max_shots + self._aug_valid if self._aug_valid else self.n_shots
        if min(idx) < 0 or max(idx) >= lim or any(self.n_shots <= i < self.max_shots for i in idx):
            raise ValueError("image index out of range of the resident task ({} shots)".format(self.n_shots))
        P = self._plan(N, infer=True)
        H = self.arch.image_size
        n0 = N - 1 if last_only else 0
        with torch.cuda.stream(self.stream):
            if P.bits is None:
                words = score_lib.size("mliis_mask_pack_words", H, H)
                P.bits = torch.zeros((N, words), dtype=torch.int64, device=self.device)
                P.bits_pin = torch.zeros((N, words), dtype=torch.int64).pin_memory()
            if counts and P.counts is None:
                P.counts = torch.zeros((N, 4), dtype=torch.int32, device=self.device)
                P.counts_pin = torch.zeros((N, 4), dtype=torch.int32).pin_memory()
            self._upload_idx(P, idx)
            if views:
                self._forward_views(P, self.shots_x, P.idx, training, views)
            else:
                self._forward(P, self.shots_x, P.idx, training, upsample=False, stochastic=False)
            if counts:
                ops.mask_pack(P.small[n0:], (H, H), self.shots_y, P.idx[n0:], bits=P.bits[n0:], counts=P.counts[n0:])
                P.counts_pin[n0:].copy_(P.counts[n0:], non_blocking=True)
            else:
                ops.mask_pack(P.small[n0:], (H, H), bits=P.bits[n0:])
            P.bits_pin[n0:].copy_(P.bits[n0:], non_blocking=True)
        self.stream.synchronize()
        masks = unpack_mask(P.bits_pin[n0:].numpy(), H, H)
        return (masks, P.counts_pin[n0:].numpy().astype(np.int64)) if counts else masks

    def histogram_resident(self, idx: Sequence[int], training: bool = False, last_only: bool = False, masks: bool = False, views=()):
        """The threshold sweep's view of predict_resident(idx): int64 [n, 2, 256], per image the histogram of its channel-1 probability
        split by label class (ops.prob_histogram on the decoder-resolution logits of score_resident's forward pass: 2 KB per image come
        back).  metrics.counts_from_histogram(...)[..., 128, :] are score_resident's rows bit for bit; the other rows are the counts at the
        other thresholds k/256.  last_only=True: only the last image of the batch ([1,2,256]), as in mask_resident.  masks=True:
        (hist, bool [n,H,W]) -- mask_resident's masks packed from the same logits, no second forward pass.  views: as in score_resident."""
        views = canonical_views(views)
        idx = [int(i) for i in idx]
        N = len(idx)
        if N == 0:
            raise ValueError("empty batch")
        lim = self.max_shots + self._aug_valid if self._aug_valid else self.n_shots
        if min(idx) < 0 or max(idx) >= lim or any(self.n_shots <= i < self.max_shots for i in idx):
            raise ValueError("image index out of range of the resident task ({} shots)".format(self.n_shots))
        P = self._plan(N, infer=True)
        H = self.arch.image_size
        n0 = N - 1 if last_only else 0
        with torch.cuda.stream(self.stream):
            if P.hist is None:
                bins = sweep_lib.size("mliis_prob_hist_bins")
                P.hist = torch.zeros((N, 2, bins), dtype=torch.int32, device=self.device)
                P.hist_pin = torch.zeros((N, 2, bins), dtype=torch.int32).pin_memory()
            if masks and P.bits is None:   # (mask_resident's buffers: either call allocates both, each call ends synchronised)
                words = score_lib.size("mliis_mask_pack_words", H, H)
                P.bits = torch.zeros((N, words), dtype=torch.int64, device=self.device)
                P.bits_pin = torch.zeros((N, words), dtype=torch.int64).pin_memory()
            self._upload_idx(P, idx)
            if views:
                self._forward_views(P, self.shots_x, P.idx, training, views)
            else:
                self._forward(P, self.shots_x, P.idx, training, upsample=False, stochastic=False)
            ops.prob_histogram(P.small[n0:], (H, H), self.shots_y, P.idx[n0:], hist=P.hist[n0:])
            P.hist_pin[n0:].copy_(P.hist[n0:], non_blocking=True)
            if masks:
                ops.mask_pack(P.small[n0:], (H, H), bits=P.bits[n0:])
                P.bits_pin[n0:].copy_(P.bits[n0:], non_blocking=True)
        self.stream.synchronize()
        hist = P.hist_pin[n0:].numpy().astype(np.int64)
        return (hist, unpack_mask(P.bits_pin[n0:].numpy(), H, H)) if masks else hist

    def close(self):
        """Destroy the captured HIP graphs (the buffers themselves are torch tensors and go with the object)."""
        self.synchronize()
        self._destroy_graphs()

    def gradients_packed(self) -> torch.Tensor:
        return self.arena.export_grad_packed()
