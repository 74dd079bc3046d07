"""ctypes binding of librsaf.so (the C ABI in include/rsaf.h).

The product path has NO CPU fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "librsaf.so")

RSAF_OK = 0


class RsafError(RuntimeError):
    pass


class ProfRecord(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_F = C.c_float


class TrainItem(C.Structure):
    """``rsaf_cnnlstm_train_item``: one replica of a group training step (``mask_lstm_host``: host array of device pointers)."""
    _fields_ = [("x", _P), ("B", _I), ("T", _I), ("params", _P), ("mask_block1", _P), ("mask_block2", _P),
                ("mask_lstm_host", _P), ("mask_fc", _P), ("saved", _P), ("saved_floats", _L), ("scratch", _P),
                ("scratch_floats", _L), ("logits", _P), ("bn_stats_out", _P), ("dlogits", _P), ("grads", _P)]


class TrainDxItem(C.Structure):
    """``rsaf_cnnlstm_train_dx_item``: a backward item of ``rsaf_cnnlstm_train_item`` plus where the gradient of its input goes
    (``dx`` NULL: none wanted) and the scratch of that part."""
    _fields_ = TrainItem._fields_ + [("dx", _P), ("dx_scratch", _P), ("dx_scratch_floats", _L)]


class ForwardItem(C.Structure):
    """``rsaf_cnnlstm_forward_item``: one eval-mode forward of a group call."""
    _fields_ = [("x", _P), ("B", _I), ("T", _I), ("weights", _P), ("workspace", _P), ("workspace_bytes", _L), ("logits", _P)]


class CeLossItem(C.Structure):
    """``rsaf_ce_loss_item``: logits and labels of one replica, its loss and (optionally) the gradient of its logits."""
    _fields_ = [("logits", _P), ("labels", _P), ("B", _I), ("loss_out", _P), ("dlogits_out", _P)]


class AdamItem(C.Structure):
    """``rsaf_cnnlstm_adam_item``: one replica of a group Adam step (``table``: device array of device pointers)."""
    _fields_ = [("grads", _P), ("table", _P), ("skip", C.c_uint64), ("lr", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step", _L)]


class CeLossWeightedItem(C.Structure):
    """``rsaf_ce_loss_weighted_item``: ``rsaf_ce_loss_item`` plus the class weights of the replica (NULL: unweighted)."""
    _fields_ = CeLossItem._fields_ + [("class_weight", _P)]


class GradNormItem(C.Structure):
    """``rsaf_cnnlstm_grad_norm_item``: the gradients of one replica as ``rsaf_cnnlstm_adam_item`` names them, the clipping
    norm, scratch for the partial sums and where the norm and the scale go."""
    _fields_ = [("grads", _P), ("table", _P), ("skip", C.c_uint64), ("max_norm", C.c_double), ("partials", _P),
                ("partials_count", _L), ("norm_out", _P), ("scale_out", _P)]


class AdamScaledItem(C.Structure):
    """``rsaf_cnnlstm_adam_scaled_item``: ``rsaf_cnnlstm_adam_item`` plus the device float its gradients are scaled by."""
    _fields_ = AdamItem._fields_ + [("grad_scale", _P)]


class PackItem(C.Structure):
    """``rsaf_cnnlstm_pack_item``: the pointer table of one replica's parameters and the blob to write."""
    _fields_ = [("table", _P), ("params", _P)]


class BnRunningItem(C.Structure):
    """``rsaf_bn_running_item``: the five BatchNorm layers of one replica (NULL ``running_mean``: layer left out)."""
    _fields_ = [("stats", _P), ("running_mean", _P * 5), ("running_var", _P * 5), ("momentum", C.c_double * 5),
                ("unbias", C.c_double * 5)]


class DropoutItem(C.Structure):
    """``rsaf_dropout_item``: seed and step of one replica's stream and its up to six masks (NULL ``mask``: slot not drawn)."""
    _fields_ = [("seed", C.c_uint64), ("step", C.c_uint64), ("mask", _P * 6), ("n", _L * 6), ("p", C.c_double * 6)]


class Arch(C.Structure):
    """``rsaf_cnnlstm_arch``: what may differ between the items of a mixed group (``act``: 1 gelu, 2 silu)."""
    _fields_ = [("channels", _I), ("hidden", _I), ("act", _I)]


class CollateItem(C.Structure):
    """``rsaf_collate_item``: one padded batch of a group collate (``frames``: what the host knows the item copies)."""
    _fields_ = [("arena", _P), ("arena_rows", _L), ("row_start", _P), ("row_count", _P), ("B", _I), ("T", _I), ("out", _P),
                ("label_src", _P), ("label_count", _L), ("label_index", _P), ("label_out", _P), ("frames", _L)]


class AugmentOp(C.Structure):
    """``rsaf_augment_op``: one op of an augmentation pipeline (``kind``: 0 Scale, 1 GaussianNoise, 2 TimeMask, 3 FeatureMask)."""
    _fields_ = [("kind", _I), ("fire_threshold", C.c_uint32), ("always", _I), ("a", C.c_double), ("b", C.c_double)]


class CollateAugmentItem(C.Structure):
    """``rsaf_collate_augment_item``: ``rsaf_collate_item`` plus the pipeline of its members (``n_ops`` 0: a plain item)."""
    _fields_ = CollateItem._fields_ + [("ops", _P), ("ops_host", _P), ("n_ops", _I), ("seed", C.c_uint64), ("epoch", C.c_uint64),
                                       ("sample_id", _P)]


class CollateMixItem(C.Structure):
    """``rsaf_collate_mix_item``: one mixed, padded batch out of resident layer stacks (``row_start``: first arena row of a
    member's block of ``L * row_count`` rows)."""
    _fields_ = [("arena", _P), ("arena_rows", _L), ("row_start", _P), ("row_count", _P), ("B", _I), ("T", _I), ("L", _I), ("p", _P),
                ("out", _P), ("label_src", _P), ("label_count", _L), ("label_index", _P), ("label_out", _P), ("frames", _L)]


class CollateMixBackwardItem(C.Structure):
    """``rsaf_collate_mix_backward_item``: dL/dp of one such batch from the resident stacks and the step's ``dx``."""
    _fields_ = [("arena", _P), ("arena_rows", _L), ("row_start", _P), ("row_count", _P), ("B", _I), ("T", _I), ("L", _I), ("dx", _P),
                ("partials", _P), ("partials_count", _L), ("dp_out", _P), ("frames", _L)]


LAYER_MIX_FROM_DP, LAYER_MIX_FROM_DW, LAYER_MIX_SOFTMAX_ONLY = 0, 1, 2


class LayerMixAdamItem(C.Structure):
    """``rsaf_layer_mix_adam_item``: the step of one mix's weights (``mode``: from ``p`` and ``dp``, from ``dw``, softmax only)."""
    _fields_ = [("L", _I), ("mode", _I), ("p", _P), ("dp", _P), ("dw", _P), ("dw_out", _P), ("w", _P), ("exp_avg", _P),
                ("exp_avg_sq", _P), ("p_next", _P), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("step", _L)]


# symbol -> (restype, argtypes); must list every function declared in include/rsaf.h
SIGNATURES = {
    "rsaf_abi_version": (_I, []),
    "rsaf_last_error": (C.c_char_p, []),
    "rsaf_init_device": (_I, [_I]),
    "rsaf_prof_begin": (_I, []),
    "rsaf_prof_end": (_I, [C.POINTER(ProfRecord), _I, C.POINTER(_I)]),
    "rsaf_smile_geometry": (_I, [_I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "rsaf_smile_n_frames": (_L, [_L, _I]),
    "rsaf_smile_lld_batch": (_I, [_P, _P, _P, _I, _L, _L, _I, _P, _P, _P, _P]),
    "rsaf_smile_workspace_bytes": (_L, [_L]),
    "rsaf_smile_pitch_track": (_I, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _P]),
    "rsaf_smile_functionals": (_I, [_P, _P, _I, _L, _I, _P, _P]),
    "rsaf_gemm_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _L, _I, _I,
                           C.POINTER(_L), _I, _I, _F, _I, _P]),
    "rsaf_f16x2_row_scales": (_I, [_P, _L, _I, _L, _P, _P, _P]),
    "rsaf_split_f16x2": (_I, [_P, _L, _I, _L, _P, _I, _P, _L, _I, _P]),
    "rsaf_gemm_f16x3": (_I, [_P, _L, _P, _I, _P, _L, _P, _P, _P, _L, _P, _I, _P, _P, _P, _I, _I, _I, _L, _L, _L, _L, _I, _F,
                             _I, _I, _I, _P]),
    "rsaf_cnnlstm_weight_floats": (_L, [_I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_weight_offsets": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), _I, C.POINTER(_I)]),
    "rsaf_cnnlstm_workspace_bytes": (_L, [_I, _I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_forward": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P, _P]),
    "rsaf_cnnlstm_forward_stages": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "rsaf_cnn_resblock_workspace_bytes": (_L, [_I, _I, _I]),
    "rsaf_cnn_resblock_forward": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P]),
    "rsaf_attnpool_forward": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "rsaf_cnnlstm_train_param_floats": (_L, [_I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_train_param_offsets": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), _I, C.POINTER(_I)]),
    "rsaf_cnnlstm_train_saved_floats": (_L, [_I, _I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_train_scratch_floats": (_L, [_I, _I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_train_forward": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P]),
    "rsaf_cnnlstm_train_backward": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P]),
    "rsaf_cnnlstm_train_group_max": (_I, []),
    "rsaf_cnnlstm_train_forward_group": (_I, [C.POINTER(TrainItem), _I, _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_train_backward_group": (_I, [C.POINTER(TrainItem), _I, _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_ce_loss_group": (_I, [C.POINTER(CeLossItem), _I, _I, _P]),
    "rsaf_cnnlstm_pack_params_group": (_I, [C.POINTER(PackItem), _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_adam_param_count": (_I, [_I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_adam_group": (_I, [C.POINTER(AdamItem), _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_ce_loss_weighted_group": (_I, [C.POINTER(CeLossWeightedItem), _I, _I, _P]),
    "rsaf_cnnlstm_grad_norm_partials": (_L, [_I, _I, _I, _I, _I]),
    "rsaf_cnnlstm_grad_norm_group": (_I, [C.POINTER(GradNormItem), _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_adam_scaled_group": (_I, [C.POINTER(AdamScaledItem), _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_bn_running_stats_group": (_I, [C.POINTER(BnRunningItem), _I, _I, _P]),
    "rsaf_dropout_masks_group": (_I, [C.POINTER(DropoutItem), _I, _P]),
    "rsaf_cnnlstm_forward_group": (_I, [C.POINTER(ForwardItem), _I, _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_train_forward_group_mixed": (_I, [C.POINTER(TrainItem), C.POINTER(Arch), _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_train_backward_group_mixed": (_I, [C.POINTER(TrainItem), C.POINTER(Arch), _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_forward_group_mixed": (_I, [C.POINTER(ForwardItem), C.POINTER(Arch), _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_train_dx_scratch_floats": (_L, [_I, _I]),
    "rsaf_cnnlstm_train_backward_dx": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P, _L,
                                            _P]),
    "rsaf_cnnlstm_train_backward_group_dx": (_I, [C.POINTER(TrainDxItem), _I, _I, _I, _I, _I, _I, _I, _P]),
    "rsaf_cnnlstm_train_backward_group_mixed_dx": (_I, [C.POINTER(TrainDxItem), C.POINTER(Arch), _I, _I, _I, _I, _P]),
    "rsaf_layer_mix_forward": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "rsaf_layer_mix_partials": (_L, [_I, _I, _I, _I]),
    "rsaf_layer_mix_backward": (_I, [_P, _P, _I, _I, _I, _I, _P, _L, _P, _P]),
    "rsaf_collate_mix_group": (_I, [C.POINTER(CollateMixItem), _I, _I, _P]),
    "rsaf_collate_mix_backward_group": (_I, [C.POINTER(CollateMixBackwardItem), _I, _I, _P]),
    "rsaf_layer_mix_adam_group": (_I, [C.POINTER(LayerMixAdamItem), _I, _P]),
    "rsaf_mshds_frameout_doubles": (_I, []),
    "rsaf_mshds_clip_peak": (_I, [_P, _P, _I, _P, _P]),
    "rsaf_mshds_intensity": (_I, [_P, _P, _I, _I, _P, _I, C.c_double, _I, _P, _P, _P]),
    "rsaf_mshds_pitch_workspace_bytes_per_clip": (_L, [_I, C.POINTER(C.c_double)]),
    "rsaf_mshds_pitch": (_I, [_P, _P, _I, _I, _P, _P, _P, C.POINTER(C.c_double), _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "rsaf_mshds_pitch_dual": (_I, [_P, _P, _I, _I, _P, _P, _P, C.POINTER(C.c_double), _P, _P, _P, _P, _P, _P,
                                   C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "rsaf_mshds_speechrate_workspace_doubles": (_L, [_I]),
    "rsaf_mshds_speechrate": (_I, [_P, _P, _I, _I, C.c_double, _P, _P, C.c_double, C.c_double, _P, _P, _P]),
    "rsaf_mshds_resample10k_table_stride": (_I, [_I]),
    "rsaf_mshds_resample10k": (_I, [_P, _P, _I, _I, _P, _I, _P, _I, _P, _P]),
    "rsaf_mshds_formants": (_I, [_P, _P, _P, _I, _I, _P, _I, C.c_double, C.c_double, C.c_double, _P, _P]),
    "rsaf_mshds_pulses_workspace_bytes": (_L, [_I, _I, C.c_double, C.c_double]),
    "rsaf_mshds_pulses": (_I, [_P, _P, _I, _I, _P, C.c_double, C.c_double, _P, _L, _P, _I, _P, _P]),
    "rsaf_mshds_ltas_slope_tilt": (_I, [_P, _P, _I, _P, _I, _P, C.c_double, C.c_double, C.c_double, _P, _P]),
    "rsaf_mshds_cpp_seg_doubles": (_I, []),
    "rsaf_mshds_cpp": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P, _L, _I, _P, _P]),
    "rsaf_mshds_formant_stats": (_I, [_P, _P, _I, C.c_double, _P, _I, _P, _P, _P]),
    "rsaf_mshds_hnr_mean": (_I, [_P, _P, _P, _I, _P, _P]),
    "rsaf_mshds_spectral_moments": (_I, [_P, _P, _P, _I, _I, _P, C.c_double, C.c_double, _P, _P, _I, _I, _I,
                                        C.c_double, C.c_double, _P, _P, _P]),
    "rsaf_pcm_to_mono_f32": (_I, [_P, _I, _I, _L, _P, _P]),
    "rsaf_resample_sinc_hann": (_I, [_P, _L, _P, _P, _I, _I, _I, _P, _L, _P]),
    "rsaf_praat_lowpass_batch": (_I, [_P, _P, _I, _I, C.c_double, _P, _L, _P, _P]),
    "rsaf_resample_praat_work_bytes": (_L, [_L, C.c_double, C.c_double]),
    "rsaf_praat_lowpass_max_samples": (_L, []),
    "rsaf_resample_praat": (_I, [_P, _L, C.c_double, C.c_double, _I, _P, _L, _P, _L, _P]),
    "rsaf_segment_mean_std": (_I, [_P, _L, _P, _P, _I, _I, _P, _P]),
    "rsaf_rows_segment_mean_f32": (_I, [_P, _L, _L, _I, _P, _I, _I, _P, _P]),
    "rsaf_gather_rows_f32": (_I, [_P, _L, _P, _L, _I, _P, _L, _P]),
    "rsaf_collate_pad_group": (_I, [C.POINTER(CollateItem), _I, _I, _P]),
    "rsaf_collate_augment_group": (_I, [C.POINTER(CollateAugmentItem), _I, _I, _P]),
    "rsaf_w2v2_frames": (_I, [_I]),
    "rsaf_w2v2_weight_floats": (_L, [_I] * 7),
    "rsaf_w2v2_weight_offsets": (_I, [_I] * 7 + [C.POINTER(_L), _I, C.POINTER(_I)]),
    "rsaf_w2v2_workspace_bytes": (_L, [_I] * 9),
    "rsaf_w2v2_forward": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _L, _P, _P, _P]),
    "rsaf_w2v2_workspace_bytes_ragged": (_L, [C.POINTER(_I), _I] + [_I] * 7),
    "rsaf_w2v2_forward_ragged": (_I, [_P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _L, _P, _P, _P]),
    "rsaf_w2v2_weight_floats_ex": (_L, [_I] * 8),
    "rsaf_w2v2_weight_offsets_ex": (_I, [_I] * 8 + [C.POINTER(_L), _I, C.POINTER(_I)]),
    "rsaf_w2v2_workspace_bytes_ragged_ex": (_L, [C.POINTER(_I), _I] + [_I] * 8),
    "rsaf_w2v2_forward_ragged_ex": (_I, [_P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P, _P, _L, _P, _P, _P]),
    "rsaf_w2v2_forward_ragged_hidden": (_I, [_P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P, _P, _L, _P, _P,
                                             C.POINTER(_I), _I, _P, _L, _P]),
}

_lib = None


def load():
    """Load librsaf.so (once).  Raises RsafError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RsafError(
            f"{LIB_PATH} not found: build it with "
            "`python -m robust_speech_analysis_framework_amd.build` (needs hipcc, gfx950). "
            "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (soname
    # libamdhip64.so.7).  Load it first so librsaf.so's NEEDED libamdhip64.so.7 resolves to that
    # already-loaded copy instead of /opt/rocm's (two runtimes in one process do not share the
    # device: the second reports "no ROCm-capable device").
    import torch
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        C.CDLL(tl, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != RSAF_OK:
        msg = load().rsaf_last_error()
        raise RsafError(f"{what or 'librsaf'} failed (code {rc}): {msg.decode() if msg else ''}")


def stream_ptr(stream=None):
    """hipStream_t of a torch stream (default: torch's current stream) as void*.

    Contract of every ``stream=`` parameter of this package: the stream, if given, must BE torch's current stream (enter it
    with ``with torch.cuda.stream(s):``).  Host-built tables travel through pinned staging buffers queued on the current
    stream and temporaries return to the current stream's allocator pool, so a kernel launched on any other stream could
    read a table before its copy lands; that is refused here instead of left as a race."""
    import torch
    cur = torch.cuda.current_stream()
    if stream is not None and stream.cuda_stream != cur.cuda_stream:
        raise RsafError("stream= must be torch's current stream: enter it with `with torch.cuda.stream(s):` "
                        "(host tables are staged on the current stream)")
    return C.c_void_p(cur.cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (must be contiguous)."""
    if not t.is_contiguous():
        raise RsafError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def optr(t):
    """``ptr(t)``, or NULL for ``None`` (an operand the call may leave out)."""
    return ptr(t) if t is not None else None


def c_void_p_off(t, elems: int):
    """Device pointer of element ``elems`` of a contiguous torch tensor."""
    if not t.is_contiguous():
        raise RsafError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr() + int(elems) * t.element_size())


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RsafError("no HIP device visible: the MI355X path has no CPU fallback")


def prof_begin():
    check(load().rsaf_prof_begin(), "rsaf_prof_begin")


def prof_end():
    lib = load()
    cap = 64
    recs = (ProfRecord * cap)()
    n = C.c_int(0)
    check(lib.rsaf_prof_end(recs, cap, C.byref(n)), "rsaf_prof_end")
    out = {}
    for i in range(min(n.value, cap)):
        r = recs[i]
        out[r.name.decode()] = {"launches": int(r.launches), "ms": float(r.ms),
                                "flops": float(r.flops), "bytes": float(r.bytes)}
    return out
