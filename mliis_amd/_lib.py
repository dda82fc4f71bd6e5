"""ctypes binding of libmliis_hip.so (the C ABI declared in include/mliis_hip.h).

The library is built in-tree (mliis_amd/libmliis_hip.so) by `__graft_entry__.build()` / `make -C mliis_amd/csrc`.
There is NO fallback: if the shared object is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MLIIS_HIP_LIB: path of an alternative build of the library (kernel experiments); the default is the in-tree build
_DEFAULT_LIB = os.path.join(_HERE, "libmliis_hip.so")
LIB_PATH = os.environ.get("MLIIS_HIP_LIB", _DEFAULT_LIB)

_f = C.c_float
_i = C.c_int
_ll = C.c_longlong
_p = C.c_void_p
_sz = C.c_size_t

# name -> (restype, argtypes)
SIGNATURES = {
    "mliis_version": (_i, []),
    "mliis_last_error": (C.c_char_p, []),
    "mliis_stem_conv_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "mliis_stem_conv_fwd_stats_floats": (_sz, [_i, _i, _i, _i]),
    "mliis_stem_conv_fwd_stats": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _sz, _p, _p]),
    "mliis_stem_conv_bwd_filter_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "mliis_stem_conv_bwd_filter": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "mliis_dwconv_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _sz, _p, _p]),
    "mliis_dwconv_bwd_data": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "mliis_dwconv_bwd_data_bn": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _sz, _p, _p]),
    "mliis_dwconv_bwd_filter_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "mliis_dwconv_bwd_filter": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "mliis_dwconv_bn_fwd_blocks": (_i, [_i, _i, _i, _i, _i, _i]),
    "mliis_dwconv_bn_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "mliis_dwconv_bn_bwd_blocks": (_i, [_i, _i, _i, _i, _i, _i]),
    "mliis_dwconv_bn_fwd": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _f, _f, _p, _p, _i, _i, _i, _i, _i, _i, _p, _sz, _p, _i, _i, _p]),
    "mliis_dwconv_bn_bwd": (_i, [_p] * 9 + [_i, _i, _i, _i, _i, _i, _p, _sz, _p, _sz, _p, _i, _i, _p]),
    "mliis_mbconv_dw_bwd_march": (_i, [_p] * 9 + [_i] + [_p] * 9 + [_i, _i, _i, _i, _i, _i, _p, _sz, _p, _sz, _p, _i, _i, _p]),
    "mliis_augment_stage": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "mliis_rng_masks": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "mliis_mbconv_dw_small_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "mliis_mbconv_dw_small_group_width": (_i, [_i, _i]),
    "mliis_mbconv_dw_fwd_small": (_i, [_p, _p, _i] + [_p] * 17 + [_i, _i, _i, _i, _i, _f, _f, _i, _i, _p, _i, _p]),
    "mliis_mbconv_dw_bwd_small": (_i, [_p] * 20 + [_i, _i, _i, _i, _i, _i, _i, _p, _i, _p]),
    "mliis_conv2d_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "mliis_conv2d_plan": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "mliis_conv1x1_occupancy": (_i, [_i, _i, _i, _p]),
    "mliis_conv2d_kernel_name": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _p, _sz]),
    "mliis_conv2d_fwd": (_i, [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _sz, _i, _f, _p, _i, _i, _p]),
    "mliis_head_ce_fused_supported": (_i, [_i, _i, _i, _i]),
    "mliis_head_ce_fused_workspace_floats": (_sz, [_i, _i, _i]),
    "mliis_head_ce_fused": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _p, _p, _p, _sz, _p]),
    "mliis_conv2d_fwd_bnin_ok": (_i, [_i, _i, _i, _i, _i]),
    "mliis_conv2d_fwd_bnin": (_i, [_p, _i, _p, _i, _f, _f, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p, _i, _p, _i,
                                   _f, _p, _i, _p]),
    "mliis_rsd_concat_pool_floats": (_sz, [_i, _i, _i, _i]),
    "mliis_rsd_concat_pool": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _i, _i, _i, _i, _p, _sz, _p, _p]),
    "mliis_rsd_pool_fwd": (_i, [_p, _i, _f, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "mliis_rsd_pool_bwd_workspace_floats": (_sz, [_i, _i]),
    "mliis_rsd_pool_bwd": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "mliis_transpose_weights": (_i, [_p, _p, _p, _i, _ll, _p, _p]),
    "mliis_weight_shadows": (_i, [_p, _p, _p, _i, _ll, _p, _p, _p, _i, _i, _p]),
    "mliis_weight_shadows_rng": (_i, [_p, _p, _p, _i, _ll, _p, _p, _p, _i, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "mliis_conv2d_bwd_data": (_i, [_p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _i, _i, _i, _p]),
    "mliis_conv2d_bwd_data_bn": (_i, [_p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _i, _p, _i, _p, _p, _p, _p, _sz, _p, _i, _i, _p]),
    "mliis_conv2d_bwd_data_gate": (_i, [_p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _i, _p, _i, _p, _sz, _p, _i, _i, _p]),
    "mliis_x3_image_bytes": (_sz, [_i, _i, _i]),
    "mliis_x3_image_blocks": (_i, [_i, _i, _i]),
    "mliis_x3_pack_weights": (_i, [_p, _p, _p, _i, _i, _p]),
    "mliis_conv2d_x3_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "mliis_conv2d_x3_plan": (_i, [_i, _i, _i, _i, _i, _i, _p]),
    "mliis_conv2d_fwd_x3": (_i, [_p, _i, _p, _sz, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _sz, _p]),
    "mliis_conv2d_bwd_data_x3": (_i, [_p, _i, _p, _sz, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "mliis_conv2d_bwd_filter_workspace_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "mliis_conv2d_bwd_filter": (_i, [_p, _i, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _sz, _i, _p]),
    "mliis_conv2d_bwd_filter_plan": (_i, [_i, _i, _i, _i, _i, _i, _p]),
    "mliis_conv2d_bwd_filter_batched": (_i, [_p, _i, _i, _i, _i, _i, _i, _p]),
    "mliis_colreduce_workspace_floats": (_sz, [_ll, _i, _i, _i]),
    "mliis_bn_stats": (_i, [_p, _i, _ll, _i, _i, _f, _f, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "mliis_bn_apply": (_i, [_p, _i, _p, _i, _ll, _i, _i, _p, _p, _p, _p, _i, _i, _p, _p, _i, _p]),
    "mliis_bn_stats_partial": (_i, [_p, _i, _ll, _i, _i, _p, _sz, _p, _p]),
    "mliis_bn_apply_fused": (_i, [_p, _i, _p, _i, _ll, _i, _i, _p, _i, _f, _f, _i, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _i, _p, _sz, _p, _i, _p]),
    "mliis_bn_bwd": (_i, [_p, _i, _p, _i, _p, _i, _ll, _i, _i, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _i, _p, _sz, _p, _sz, _p, _i, _i, _p]),
    "mliis_bn_apply_fused_pair": (_i, [_p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _ll, _i, _f, _f, _i, _i, _i, _p]),
    "mliis_bn_bwd_pair": (_i, [_p] * 20 + [_i, _i, _i, _ll, _i, _i, _i, _sz, _p, _sz, _p]),
    "mliis_bn_bwd_dxsum_floats": (_sz, [_ll, _i]),
    "mliis_colsum": (_i, [_p, _i, _p, _i, _ll, _i, _i, _f, _p, _i, _p, _sz, _i, _p]),
    "mliis_se_mlp_fwd": (_i, [_p, _i, _f, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "mliis_se_mlp_bwd": (_i, [_p, _i] + [_p] * 13 + [_i, _i, _i, _i, _p]),
    "mliis_se_bn_bwd_sums_floats": (_sz, [_i, _i, _i]),
    "mliis_se_bn_bwd_sums": (_i, [_p, _i, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _sz, _p, _i, _p]),
    "mliis_se_mlp_bwd_bn": (_i, [_p, _i] + [_p] * 9 + [_i, _i, _i, _i, _p]),
    "mliis_se_wgrad_batched": (_i, [_p, _i, _ll, _p]),
    "mliis_chan_affine": (_i, [_p, _i, _p, _p, _p, _i, _ll, _i, _i, _i, _p]),
    "mliis_chan_split": (_i, [_p, _i, _p, _p, _i, _i, _i, _p, _i, _i, _ll, _i, _i, _p]),
    "mliis_swish_mask_fwd": (_i, [_p, _i, _p, _i, _p, _i, _ll, _i, _i, _p]),
    "mliis_swish_mask_bwd": (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _ll, _i, _i, _p]),
    "mliis_resize_bilinear_fwd": (_i, [_p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "mliis_resize_bilinear_bwd": (_i, [_p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "mliis_final_conv_fwd": (_i, [_p, _i, _p, _p, _p, _p, _ll, _i, _p]),
    "mliis_final_conv_bwd_data": (_i, [_p, _p, _p, _p, _i, _ll, _i, _p]),
    "mliis_final_conv_bwd_data_fin": (_i, [_p, _p, _p, _p, _i, _ll, _i, _p, _i, _i, _i, _i, _i, _f, _p, _p]),
    "mliis_final_conv_bwd_filter": (_i, [_p, _i, _p, _p, _ll, _i, _p, _p, _p, _sz, _p]),
    "mliis_softmax_ce_workspace_floats": (_sz, [_i, _i, _i]),
    "mliis_softmax_ce": (_i, [_p, _p, _p, _i, _i, _i, _f, _i, _f, _p, _p, _p, _p, _sz, _p]),
    "mliis_darc1": (_i, [_p, _i, _ll, _f, _p, _p, _p, _sz, _p]),
    "mliis_sgd_fused": (_i, [_p, _p, _p, _ll, _f, _p, _f, _f, _p]),
    "mliis_adam_b1zero_fused": (_i, [_p, _p, _p, _p, _ll, _f, _p, _f, _f, _f, _f, _p, _p, _p]),
    "mliis_axpby": (_i, [_f, _p, _f, _p, _ll, _p]),
    "mliis_lincomb": (_i, [_f, _p, _f, _p, _p, _ll, _p]),
    "mliis_copy_words": (_i, [_p, _p, _i, _p]),
    "mliis_fold_batched": (_i, [_p, _p, _p, _i, _ll, _p, _i, _ll, _p]),
    "mliis_fold_tile_outputs": (_i, []),
    "mliis_graph_begin_capture": (_i, [_p]),
    "mliis_graph_end_capture": (_i, [_p, C.POINTER(C.c_void_p)]),
    "mliis_graph_launch": (_i, [_p, _p]),
    "mliis_graph_destroy": (_i, [_p]),
}


# libmliis_score.so (include/mliis_score.h): the evaluation scores, a library of its own beside the training step's
SCORE_LIB_PATH = os.path.join(_HERE, "libmliis_score.so")
SCORE_SIGNATURES = {
    "mliis_score_last_error": (C.c_char_p, []),
    "mliis_mask_iou_counts": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "mliis_mask_pack_words": (_ll, [_i, _i]),
    "mliis_mask_pack": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
}

# libmliis_data.so (include/mliis_data.h): a task's shots expanded / resampled from stored bytes, a library of its own as well
DATA_LIB_PATH = os.path.join(_HERE, "libmliis_data.so")
DATA_SIGNATURES = {
    "mliis_data_last_error": (C.c_char_p, []),
    "mliis_task_expand_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
}

# libmliis_steplog.so (include/mliis_steplog.h): the inner loop's step log, a library of its own as well
STEPLOG_LIB_PATH = os.path.join(_HERE, "libmliis_steplog.so")
STEPLOG_SIGNATURES = {
    "mliis_steplog_last_error": (C.c_char_p, []),
    "mliis_steplog_workspace_bytes": (_sz, []),
    "mliis_steplog_record_words": (_i, []),
    "mliis_steplog_append": (_i, [_p, _p, _p, _p, _ll, _p, _p, _i, _p, _p]),
}

# libmliis_layerlog.so (include/mliis_layerlog.h): the inner loop's per-tensor log, a library of its own as well
LAYERLOG_LIB_PATH = os.path.join(_HERE, "libmliis_layerlog.so")
LAYERLOG_SIGNATURES = {
    "mliis_layerlog_last_error": (C.c_char_p, []),
    "mliis_layerlog_chunk_quads": (_i, []),
    "mliis_layerlog_workspace_bytes": (_sz, [_i]),
    "mliis_layerlog_record_words": (_i, []),
    "mliis_layerlog_append": (_i, [_i, _p, _p, _ll, _p, _i, _p, _i, _p, _sz, _p, _i, _p, C.c_uint, _p]),
}

# libmliis_clip.so (include/mliis_clip.h): the inner loop's gradient clipping, a library of its own as well
CLIP_LIB_PATH = os.path.join(_HERE, "libmliis_clip.so")
CLIP_SIGNATURES = {
    "mliis_clip_last_error": (C.c_char_p, []),
    "mliis_clip_chunk_quads": (_i, []),
    "mliis_clip_workspace_bytes": (_sz, [_i, _i]),
    "mliis_clip_record_words": (_i, []),
    "mliis_clip_apply": (_i, [_i, _p, _p, _ll, _p, _i, _p, _i, _f, _f, _p, _sz, _p, _i, _p, _p]),
}

# libmliis_sweep.so (include/mliis_sweep.h): the evaluation threshold sweep's probability histograms, a library of its own as well.
# MLIIS_SWEEP_LIB: path of an alternative build (kernel experiments, tools/bench_sweep.py); the default is the in-tree build
SWEEP_LIB_PATH = os.environ.get("MLIIS_SWEEP_LIB", os.path.join(_HERE, "libmliis_sweep.so"))
SWEEP_SIGNATURES = {
    "mliis_sweep_last_error": (C.c_char_p, []),
    "mliis_prob_hist_bins": (_i, []),
    "mliis_prob_histogram": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
}

# libmliis_loss.so (include/mliis_loss.h): the focal, foreground-weighted pixel loss of the inner loop, a library of its own as well; loaded
# only by a learner built with focal_gamma != 0 or fg_weight != 1
LOSS_LIB_PATH = os.path.join(_HERE, "libmliis_loss.so")
LOSS_SIGNATURES = {
    "mliis_loss_last_error": (C.c_char_p, []),
    "mliis_focal_ce_workspace_floats": (_sz, [_i, _i, _i]),
    "mliis_focal_ce": (_i, [_p, _p, _p, _i, _i, _i, _f, _f, _f, _i, _f, _p, _p, _p, _sz, _p]),
    "mliis_head_focal_fused_supported": (_i, [_i, _i, _i, _i]),
    "mliis_head_focal_fused_workspace_floats": (_sz, [_i, _i, _i]),
    "mliis_head_focal_fused": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _sz, _p]),
}

# libmliis_region.so (include/mliis_region.h): the Tversky region term of the inner loop's loss on that pixel loss, a library of its own as
# well; loaded only by a learner built with tversky=(alpha, beta)
REGION_LIB_PATH = os.path.join(_HERE, "libmliis_region.so")
REGION_SIGNATURES = {
    "mliis_region_last_error": (C.c_char_p, []),
    "mliis_tversky_ce_workspace_floats": (_sz, [_i, _i, _i]),
    "mliis_tversky_ce": (_i, [_p, _p, _p, _i, _i, _i, _f, _f, _f, _f, _f, _f, _p, _p, _p, _sz, _p]),
    "mliis_head_tversky_fused_supported": (_i, [_i, _i, _i, _i]),
    "mliis_head_tversky_fused_workspace_floats": (_sz, [_i, _i, _i, _i, _i]),
    "mliis_head_tversky_fused": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _p, _p, _p, _sz, _p]),
}

# libmliis_tta.so (include/mliis_tta.h): evaluation's flip test-time augmentation -- the mirrored copy of a batch and the merge of the views'
# decoder-resolution logits, a library of its own as well; loaded only by an evaluation call with views= (--eval-tta)
TTA_LIB_PATH = os.path.join(_HERE, "libmliis_tta.so")
TTA_SIGNATURES = {
    "mliis_tta_last_error": (C.c_char_p, []),
    "mliis_view_gather": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "mliis_view_merge": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p]),
}


class MliisError(RuntimeError):
    pass


class _Lib:
    def __init__(self, path=None, signatures=None, last_error="mliis_last_error"):
        """Default: libmliis_hip.so at the module's LIB_PATH with SIGNATURES; (path, signatures, name of its error query): another
        library of the same conventions (score_lib, data_lib, steplog_lib, layerlog_lib, clip_lib, sweep_lib, loss_lib, tta_lib, region_lib)."""
        self._dll = None
        self._path, self._signatures, self._last_error = path, signatures, last_error

    def load(self):
        if self._dll is None:
            path, signatures = (self._path or LIB_PATH), (SIGNATURES if self._signatures is None else self._signatures)
            if not os.path.exists(path):
                raise MliisError(
                    "{} not found at {} -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "or `make -C mliis_amd/csrc`.  There is no CPU fallback.".format(os.path.basename(path), path))
            # PyTorch-ROCm carries its own HIP runtime: import it FIRST so that this library resolves libamdhip64 to the copy torch
            # has already loaded.  Loaded the other way round, the process ends up with two HIP runtimes and the one this library is
            # bound to sees no device ("no ROCm-capable device is detected" at the first launch).
            import torch  # noqa: F401
            dll = C.CDLL(path)
            for name, (res, args) in signatures.items():
                fn = getattr(dll, name)
                fn.restype = res
                fn.argtypes = args
            self._dll = dll
        return self._dll

    def raw(self, name):
        return getattr(self.load(), name)

    trace = None   # profiling aid (tools/site_times.py): a list that receives (entry point, args) of every call while it is set

    def call(self, name, *args):
        """Call an int-returning entry point; raise MliisError with the library's message on failure."""
        if self.trace is not None:
            self.trace.append((name, args))
        rc = getattr(self.load(), name)(*args)
        if rc != 0:
            msg = getattr(self._dll, self._last_error)()
            raise MliisError("{} failed ({}): {}".format(name, rc, msg.decode() if msg else "?"))

    def size(self, name, *args) -> int:
        return int(getattr(self.load(), name)(*args))


lib = _Lib()
score_lib = _Lib(SCORE_LIB_PATH, SCORE_SIGNATURES, "mliis_score_last_error")
data_lib = _Lib(DATA_LIB_PATH, DATA_SIGNATURES, "mliis_data_last_error")
steplog_lib = _Lib(STEPLOG_LIB_PATH, STEPLOG_SIGNATURES, "mliis_steplog_last_error")
layerlog_lib = _Lib(LAYERLOG_LIB_PATH, LAYERLOG_SIGNATURES, "mliis_layerlog_last_error")
clip_lib = _Lib(CLIP_LIB_PATH, CLIP_SIGNATURES, "mliis_clip_last_error")
sweep_lib = _Lib(SWEEP_LIB_PATH, SWEEP_SIGNATURES, "mliis_sweep_last_error")
loss_lib = _Lib(LOSS_LIB_PATH, LOSS_SIGNATURES, "mliis_loss_last_error")
tta_lib = _Lib(TTA_LIB_PATH, TTA_SIGNATURES, "mliis_tta_last_error")
region_lib = _Lib(REGION_LIB_PATH, REGION_SIGNATURES, "mliis_region_last_error")
