"""ctypes binding of librau.so (the C ABI declared in include/rau.h).

The library is the product: if it is missing, or no gfx950 device is usable,
loading / rau_create raise -- there is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# Nothing here touches the process environment.  (rau_graph_step replays fastest with the HIP runtime
# variable DEBUG_HIP_FORCE_GRAPH_QUEUES=2; a host that wants that sets it itself
# before its first HIP call -- `bench.py --graph` does, for its own process only.)
# RAU_LIB overrides the library path (A/B runs of two builds on one GPU box)
LIB_PATH = os.environ.get("RAU_LIB") or os.path.join(_HERE, "librau.so")
CSRC = os.path.join(_HERE, "csrc")

GROUP_EMBED, GROUP_RNN, GROUP_MULT = 0, 1, 2
GROUPS = {"embed": GROUP_EMBED, "rnn": GROUP_RNN, "mult": GROUP_MULT}
MODE_TRAIN, MODE_EVAL = 0, 1
MASK_SITES = {"we": 0, "rnn": 1, "q": 2, "x": 3, "mf": 4}
XDROP_PER_HOP, XDROP_TIED = 0, 1
LOSS_CE, LOSS_BCE = 0, 1
LOSSES = {"ce": LOSS_CE, "bce": LOSS_BCE}
FEAT_GRAD_OFF, FEAT_GRAD_SAMPLES, FEAT_GRAD_IMAGES = 0, 1, 2
XNORM_NONE, XNORM_L2 = 0, 1


class RauConfig(C.Structure):
    """Mirror of ``rau_config`` (include/rau.h)."""
    _fields_ = [(n, C.c_int32) for n in
                ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")] + \
               [(n, C.c_float) for n in ("p_we", "p_rnn", "p_q", "p_x", "p_mf")] + \
               [("dtype", C.c_int32), ("device_id", C.c_int32)]


OPT_ADAM, OPT_ADAMAX = 0, 1
OPT_RULES = {"adam": OPT_ADAM, "adamax": OPT_ADAMAX}
CLIP_GROUP, CLIP_GLOBAL = 0, 1
CLIP_SCOPES = {"group": CLIP_GROUP, "global": CLIP_GLOBAL}


class RauUpdateOpts(C.Structure):
    """Mirror of ``rau_update_opts`` (include/rau.h)."""
    _fields_ = [("rule", C.c_int32), ("clip_scope", C.c_int32)] + \
               [(n, C.c_float) for n in ("lr", "mult_lr", "beta1", "beta2", "eps", "eta", "gamma", "clip")] + \
               [("noise_seed", C.c_uint64)]


class RauUpdateExtras(C.Structure):
    """Mirror of ``rau_update_extras`` (include/rau.h): what rau_update_ex takes beside rau_update_opts."""
    _fields_ = [("weight_decay", C.c_float), ("ema_decay", C.c_float)]


STAT_GRAD, STAT_PARAM, STAT_DIR = 1, 2, 4
GUARD_OFF, GUARD_SKIP = 0, 1


class RauLayerStat(C.Structure):
    """Mirror of ``rau_layer_stat`` (include/rau.h): one layout entry's statistics, [grad, param, dir]."""
    _fields_ = [("sumsq", C.c_float * 3), ("absmax", C.c_float * 3), ("nonfinite", C.c_int64 * 3),
                ("n", C.c_int64)]


class RauOutGrads(C.Structure):
    """Mirror of ``rau_out_grads`` (include/rau.h): device pointers, None = no such term."""
    _fields_ = [(n, C.c_void_p) for n in ("d_logits", "d_dopred", "d_attprob")]


class RauStateGrads(C.Structure):
    """Mirror of ``rau_state_grads`` (include/rau.h): device pointers, None = no such term."""
    _fields_ = [(n, C.c_void_p) for n in ("d_h", "d_c_last")]


class RauError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile librau.so for gfx950 with the in-tree Makefile (hipcc)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB_PATH):
        raise RauError("build did not produce " + LIB_PATH)
    return LIB_PATH


_SIGS = {
    # name: (restype, argtypes)
    "rau_default_config": (None, [C.POINTER(RauConfig)]),
    "rau_last_error": (C.c_char_p, []),
    "rau_abi_version": (C.c_int, []),
    "rau_create": (C.c_int, [C.POINTER(RauConfig), C.POINTER(C.c_void_p)]),
    "rau_destroy": (None, [C.c_void_p]),
    "rau_set_batch_size": (C.c_int, [C.c_void_p, C.c_int32]),
    "rau_batch_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rau_params": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                             C.POINTER(C.c_size_t)]),
    "rau_layout_count": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_layout_entry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32)]),
    "rau_set_params": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_get_params": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_get_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_set_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_init_uniform": (C.c_int, [C.c_void_p, C.c_uint64, C.c_float, C.c_float]),
    "rau_zero_grads": (C.c_int, [C.c_void_p]),
    "rau_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_set_dropout_seed": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "rau_set_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_get_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    # feature-map dropout: a mask per hop clone (0) or one mask tied across the hops (1)
    "rau_set_feat_dropout": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_feat_dropout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # answer criterion of the step path: softmax cross-entropy (0) or per-answer sigmoid BCE (1)
    "rau_set_answer_loss": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_answer_loss": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_set_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_batch_feats": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rau_batch_slot": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rau_set_batch_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int]),
    "rau_use_batch": (C.c_int, [C.c_void_p, C.c_int]),
    # answer sets: multi-answer ground truth on a batch
    "rau_set_answers": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_batch_answers": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    # region counts: attention over a sample's valid positions only
    "rau_set_regions": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rau_batch_regions": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_set_sample_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rau_batch_sample_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # multiple-choice candidates of a batch: the criterion head restricted to them
    "rau_set_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_void_p]),
    "rau_batch_candidates": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    # packed region rows: transposed and zero-padded on the device, counts attached in the same call
    "rau_set_batch_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "rau_set_batch_async_packed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rau_bank_put_packed": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]),
    "rau_set_batch_typed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "rau_set_batch_async_typed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int]),
    "rau_batch_feat_type": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_set_batch_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "rau_set_batch_async_images": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rau_batch_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    # feature bank: maps resident in device memory, batches name their images by row
    "rau_bank_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int]),
    "rau_bank_destroy": (C.c_int, [C.c_void_p]),
    "rau_bank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_int32)]),
    "rau_bank_put": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int]),
    "rau_bank_get": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rau_set_batch_bank": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "rau_set_batch_async_bank": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int]),
    "rau_forward": (C.c_int, [C.c_void_p]),
    "rau_backward": (C.c_int, [C.c_void_p, C.c_void_p]),
    # the same with the step-selection head's BCE gradient, weighted per hop (NULL = zeros)
    "rau_backward_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_graph_step_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    # attention supervision: per-sample target maps on a batch, their loss at the attprob output
    "rau_set_att_targets": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rau_batch_att_targets": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_backward_att": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_graph_step_att": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rau_att_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rau_att_criterion_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_float)]),
    "rau_att_criterion_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                             C.POINTER(C.c_void_p)]),
    # the merged answers' cross-entropies (uni, select) as training terms
    "rau_backward_merged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_graph_step_merged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rau_merge_criterion_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    # custom objectives: the outputs on the device, caller-supplied gradients into the step-level backward
    "rau_outputs_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int32)]),
    "rau_logits_pitch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rau_backward_ext": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(RauOutGrads)]),
    # feature-map gradient of the step-level backward; a batch whose maps are already on the device
    "rau_set_feat_grad": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_feat_grad": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_feat_grad_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "rau_feat_grad_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rau_get_feat_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    # per-position L2 normalisation of the batch's maps in front of the image side
    "rau_set_feat_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "rau_feat_norm": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "rau_norm_feats_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rau_get_norm_feats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_set_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_set_batch_dev_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    # question state from the caller: the step path behind another question encoder, dq back
    "rau_set_question_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rau_batch_question": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_question_grad_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rau_get_question_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    # the hop recurrence's ends: initial state in, state gradients in and out
    "rau_set_state_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rau_batch_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_state_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rau_backward_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(RauOutGrads), C.POINTER(RauStateGrads)]),
    "rau_state_grad_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rau_get_state_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # attention bias from the caller: masks and priors in, its gradient out
    "rau_set_att_bias_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rau_batch_att_bias": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rau_att_bias_grad_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "rau_get_att_bias_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    # module-level entry points: device pointers in, pointers to ctx-owned slots out
    "rau_embed_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rau_embed_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rau_deeplstm_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_void_p)]),
    "rau_deeplstm_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rau_multimodal_forward": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 +
                               [C.POINTER(C.c_void_p)] * 5),
    "rau_multimodal_forward_regions": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 +
                                       [C.POINTER(C.c_void_p)] * 5),
    "rau_multimodal_forward_bias": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6 +
                                    [C.POINTER(C.c_void_p)] * 5),
    "rau_multimodal_backward": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 9 +
                                [C.POINTER(C.c_void_p)] * 4),
    "rau_criterion_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_float)]),
    "rau_criterion_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                         C.POINTER(C.c_void_p)]),
    "rau_criterion_forward_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_float)]),
    "rau_criterion_backward_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_float, C.POINTER(C.c_void_p)]),
    # the per-answer sigmoid criterion: labels, or (labels NULL) an answer set
    "rau_criterion_forward_bce": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_float)]),
    "rau_criterion_backward_bce": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_float, C.POINTER(C.c_void_p)]),
    "rau_criterion_forward_cand": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "rau_criterion_backward_cand": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_float,
                                              C.POINTER(C.c_void_p)]),
    # device tensors (the tensor algebra feval does between module calls)
    "rau_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "rau_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_dev_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rau_dev_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_dev_axpy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rau_dev_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rau_dev_addcmul": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_dev_addcdiv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_dev_sqrt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_dev_add_scalar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rau_dev_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32]),
    "rau_dev_adamax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32]),
    "rau_dev_scale_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rau_dev_l2norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rau_dev_l2norm_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32,
                                          C.c_void_p]),
    "rau_dev_select_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_int32]),
    "rau_dev_rowmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p]),
    "rau_dev_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                               C.c_void_p]),
    "rau_dev_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]),
    "rau_dev_count_eq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.POINTER(C.c_int32)]),
    "rau_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rau_graph_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rau_sync": (C.c_int, [C.c_void_p]),
    "rau_get_losses": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_loss_rows": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_argmax": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_logits": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_dopred": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_attention": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_question_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rau_get_att_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # merged hops: feval's statistics and predict_result on the device
    "rau_step_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_step_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_predict_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rau_get_merged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_topk": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_cand_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rau_topk_cand": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_noise_clip_adam": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_float] * 8 +
                            [C.c_uint64, C.c_void_p]),
    # the update with a rule and a clip scope; optimizer state in and out
    "rau_update_opts_default": (None, [C.POINTER(RauUpdateOpts)]),
    "rau_update": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(RauUpdateOpts), C.c_void_p]),
    "rau_get_opt_state": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32)]),
    "rau_set_opt_state": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    # decoupled weight decay, per-layer options, the weight average
    "rau_update_extras_default": (None, [C.POINTER(RauUpdateExtras)]),
    "rau_update_ex": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(RauUpdateOpts), C.POINTER(RauUpdateExtras),
                                C.c_void_p]),
    "rau_set_layer_opts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]),
    "rau_get_layer_opts": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 3),
    "rau_ema_reset": (C.c_int, [C.c_void_p]),
    "rau_ema_swap": (C.c_int, [C.c_void_p]),
    "rau_ema_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rau_get_ema": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_set_ema": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    # per-layer statistics on the device; the non-finite guard in front of the update
    "rau_layer_stats_count": (C.c_int, [C.c_void_p]),
    "rau_layer_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(RauLayerStat)]),
    "rau_layer_stats_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)]),
    "rau_set_update_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_update_guard": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64)]),
    "rau_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rau_wait_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rau_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rau_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "rau_allreduce_grads": (C.c_int, [C.c_void_p]),
    "rau_comm_destroy": (C.c_int, [C.c_void_p]),
    "rau_timer_begin": (C.c_int, [C.c_void_p]),
    "rau_timer_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rau_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rau_prof_reset": (C.c_int, [C.c_void_p]),
    "rau_prof_count": (C.c_int, [C.c_void_p]),
    "rau_prof_entry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rau_split_guard_check": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.c_size_t]),
    "rau_image_lists": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rau_enc_ws_coresident": (C.c_int, [C.c_int, C.c_int, C.c_int]),
}

_lib = None


def lib() -> C.CDLL:
    """Load librau.so and bind every symbol include/rau.h declares."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RauError(f"{LIB_PATH} not found: build it with "
                           "`python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        # PyTorch wheels bundle their own libamdhip64; if librau pulled in the system copy
        # first, a later `import torch` would bring up a SECOND HIP runtime in the process,
        # which then finds no GPU.  Loading torch first makes both share one runtime.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            if os.environ.get("RAU_LIB") and not hasattr(l, name):
                continue           # A/B runs against an older build (development only)
            fn = getattr(l, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise RauError(f"librau error {rc}: {lib().rau_last_error().decode()}")
