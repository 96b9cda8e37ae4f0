"""ctypes binding of include/difacto_hip.h (the reference-side stub for a Python
host; the C++ host in difacto_amd/host/ binds the same symbols)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFACTO_HIP_LIB: another build of the same library (tools/var_<name>.so of a same-box A/B); it must exist
LIB_PATH = os.environ.get("DIFACTO_HIP_LIB") or os.path.join(_HERE, "libdifacto_hip.so")

FEA_COUNT, WEIGHT, GRADIENT = 1, 2, 3
INIT_REFRAND, INIT_HASH = 0, 1
U64MAX = 2 ** 64 - 1

# every symbol include/difacto_hip.h declares (tests check the .so exports them all)
SYMBOLS = [
    "dfh_last_error", "dfh_updater_param_default", "dfh_ctx_create", "dfh_ctx_destroy", "dfh_ctx_sync",
    "dfh_ctx_stream", "dfh_ctx_device", "dfh_reverse_bytes", "dfh_encode_fea_grp_id", "dfh_table_create",
    "dfh_table_destroy", "dfh_table_size", "dfh_table_param", "dfh_table_bytes", "dfh_pull", "dfh_push",
    "dfh_table_export", "dfh_table_import", "dfh_fm_predict", "dfh_fm_calcgrad", "dfh_loss_evaluate",
    "dfh_auc_times_n", "dfh_batch_create", "dfh_batch_destroy", "dfh_batch_load_host", "dfh_batch_load_device",
    "dfh_localize", "dfh_batch_load_localized_host", "dfh_batch_get_localized", "dfh_batch_shape", "dfh_sgd_step",
    "dfh_batch_progress", "dfh_batch_get_pred", "dfh_row_stride", "dfh_shard_pull", "dfh_shard_push_count",
    "dfh_shard_push_grad", "dfh_batch_forward", "dfh_batch_backward", "dfh_batch_device_keys", "dfh_malloc",
    "dfh_free", "dfh_memcpy_h2d", "dfh_memcpy_d2h", "dfh_ctx_set_timing", "dfh_ctx_get_timing", "dfh_kernel_name",
    "dfh_table_warm_start", "dfh_ctx_set_pipeline", "dfh_batch_lookup", "dfh_localize_lookup", "dfh_rowbuf_create", "dfh_rowbuf_destroy", "dfh_rowbuf_load_host", "dfh_batch_gather_rows", "dfh_batch_set_option", "dfh_batch_key_ranges", "dfh_batch_attach_device",
    "dfh_batch_key_ranges_device", "dfh_shard_resolve", "dfh_shard_pull_resolved", "dfh_shard_push_count_resolved",
    "dfh_shard_push_grad_resolved", "dfh_table_check", "dfh_ctx_set_timing_mask", "dfh_table_save", "dfh_table_load", "dfh_shard_resolve_multi", "dfh_shard_push_count_multi",
    "dfh_shard_push_grad_multi", "dfh_shard_count_pull_multi", "dfh_shard_push_grad_listed", "dfh_shard_release", "dfh_ctx_set_option", "dfh_table_set_has_aux", "dfh_table_has_aux",
    "dfh_comm_unique_id", "dfh_comm_create_rccl", "dfh_comm_create_callback", "dfh_comm_destroy", "dfh_comm_rank", "dfh_comm_world",
    "dfh_comm_allreduce_sum", "dfh_shard_create", "dfh_shard_destroy", "dfh_shard_owned_range", "dfh_shard_step", "dfh_shard_prefetch_counts",
    "dfh_shard_pull_host", "dfh_shard_push_host", "dfh_comm_allgather", "dfh_shard_balanced_splits", "dfh_shard_set_exchange", "dfh_shard_set_timing", "dfh_shard_get_timing",
    "dfh_comm_stats", "dfh_comm_info", "dfh_comm_selfcheck", "dfh_comm_wire_probe", "dfh_table_capacity", "dfh_batch_prepare_rows", "dfh_rowbuf_load_host_slices",
    "dfh_rowbuf_set_labels", "dfh_batch_prepare_cached", "dfh_batch_get_rows",
    "dfh_batch_create_many", "dfh_shard_multi_words", "dfh_shard_reserve", "dfh_comm_create_loopback", "dfh_comm_loopback_feed", "dfh_comm_loopback_wire", "dfh_comm_loopback_wire_time",
    "dfh_vec_inner_multi", "dfh_vec_combine", "dfh_vec_line_step", "dfh_lbfgs_create", "dfh_lbfgs_destroy", "dfh_lbfgs_add_chunk",
    "dfh_lbfgs_init_model", "dfh_lbfgs_shape", "dfh_lbfgs_get_model", "dfh_lbfgs_set_weights", "dfh_lbfgs_calc_grad",
    "dfh_lbfgs_prepare_direction", "dfh_lbfgs_calc_direction", "dfh_lbfgs_line_search", "dfh_lbfgs_evaluate", "dfh_lbfgs_create_sharded",
    "dfh_lbfgs_owned_range", "dfh_lbfgs_set_model", "dfh_lbfgs_get_vector", "dfh_bcd_set_model",
    "dfh_lbfgs_set_l1", "dfh_lbfgs_get_owlqn_vector", "dfh_lbfgs_drop_last_pair", "dfh_lbfgs_get_owlqn_moved",
    "dfh_bcd_create", "dfh_bcd_destroy", "dfh_bcd_add_chunk", "dfh_bcd_build", "dfh_bcd_shape", "dfh_bcd_block_info",
    "dfh_bcd_epoch", "dfh_bcd_step", "dfh_bcd_get_model", "dfh_bcd_get_pred", "dfh_batch_split_entries",
    "dfh_bcd_create_sharded",
    "dfh_textchunk_create", "dfh_textchunk_destroy", "dfh_textchunk_parse_criteo", "dfh_textchunk_rows", "dfh_textchunk_ids",
    "dfh_lz4_decompress", "dfh_textchunk_decode_crb",
    "dfh_rowbuf_load_slices",
    "dfh_lz4_compress", "dfh_crb_create", "dfh_crb_destroy", "dfh_crb_encode_host", "dfh_crb_encode_textchunk", "dfh_crb_record",
    "dfh_eval_create", "dfh_eval_destroy", "dfh_eval_reset", "dfh_eval_append_batch", "dfh_eval_append_host", "dfh_eval_finish",
    "dfh_predtext_create", "dfh_predtext_destroy", "dfh_predtext_reset", "dfh_predtext_append_batch", "dfh_predtext_append_host",
    "dfh_predtext_count", "dfh_predtext_values", "dfh_predtext_format", "dfh_predtext_read", "dfh_predtext_tile",
    "dfh_batch_key_view_info", "dfh_batch_get_key_view",
    "dfh_dump_open", "dfh_dump_close", "dfh_dump_shape", "dfh_dump_format", "dfh_dump_read", "dfh_dump_entries", "dfh_dump_tile",
    "dfh_rowstore_create", "dfh_rowstore_destroy", "dfh_rowstore_append_host", "dfh_rowstore_append_textchunk", "dfh_rowstore_shape",
    "dfh_rowstore_order", "dfh_rowstore_get_order", "dfh_rowstore_read", "dfh_crb_encode_rowstore",
]
XCHG_COUNTS, XCHG_KEYS, XCHG_CNT, XCHG_ROWS, XCHG_GRADS, XCHG_OTHER = range(6)
SHARD_STAGES = ("counts", "L", "K", "R", "RW", "F", "G", "P")
K_COUNT = 8
K_LOCALIZE, K_LOOKUP, K_FORWARD, K_BACKWARD, K_PULL, K_PUSH, K_MISC, K_AUC = range(8)


class UpdaterParam(C.Structure):
    """SGDUpdaterParam (src/sgd/sgd_param.h:66-107)"""
    _fields_ = [("l1", C.c_float), ("l2", C.c_float), ("V_l2", C.c_float), ("lr", C.c_float),
                ("lr_beta", C.c_float), ("V_lr", C.c_float), ("V_lr_beta", C.c_float),
                ("V_init_scale", C.c_float), ("V_dim", C.c_int), ("V_threshold", C.c_int),
                ("seed", C.c_uint), ("init_mode", C.c_int)]


class Progress(C.Structure):
    """sgd::Progress (src/sgd/sgd_utils.h:40-75)"""
    _fields_ = [("loss", C.c_float), ("penalty", C.c_float), ("auc", C.c_float),
                ("nnz_w", C.c_float), ("nrows", C.c_float)]


class EvalResult(C.Structure):
    """dfh_eval_result: the exact whole-set metrics (auc2 = 2 x pairs ranked right + tied pairs)"""
    _fields_ = [("n", C.c_uint64), ("n_pos", C.c_uint64), ("n_neg", C.c_uint64), ("n_nan", C.c_uint64), ("auc2", C.c_uint64),
                ("correct", C.c_uint64), ("objv", C.c_double)]


class Slice(C.Structure):
    """dfh_slice: host arrays (chunk = NULL), or ids [first, first + nnz) of a parsed text chunk"""
    _fields_ = [("index", C.c_void_p), ("value", C.c_void_p), ("chunk", C.c_void_p), ("first", C.c_size_t), ("nnz", C.c_size_t)]


class KeyViewInfo(C.Structure):
    """dfh_key_view_info: the sizes of what dfh_batch_get_key_view fills, and the class bounds of the build"""
    _fields_ = [("U", C.c_uint64), ("nnz", C.c_uint64), ("has_value", C.c_uint32), ("seg_nb", C.c_uint32), ("P", C.c_uint32),
                ("split_n", C.c_uint32), ("few_cap", C.c_uint64), ("mid_cap", C.c_uint64), ("hot_cap", C.c_uint64),
                ("split_cap", C.c_uint64), ("bwd_small", C.c_uint32), ("bwd_mid", C.c_uint32), ("hot_split", C.c_uint32),
                ("hot_split_min", C.c_uint32)]


# dfh_alltoallv_fn: int (*)(void* user, const void* send, const size_t* send_bytes, void* recv, const size_t* recv_bytes)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t))
COMM_ID_BYTES = 128


class DfhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("difacto_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """load libdifacto_hip.so; raises (no fallback) if it has not been built"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            "%s is missing: build it with `python -m difacto_amd.build` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    # Load order matters when PyTorch is used in the same process (multi-GPU driver, bench.py):
    # torch bundles its own libamdhip64; if ours (linked to the system ROCm runtime of the same
    # soname) is mapped first, torch later brings up a second HIP runtime and sees no GPU.
    # Importing torch first makes both share one runtime.
    if os.environ.get("DIFACTO_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u64, f32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_float
    PP = C.POINTER
    L.dfh_last_error.restype = C.c_char_p
    L.dfh_updater_param_default.argtypes = [PP(UpdaterParam), i32]
    L.dfh_ctx_create.argtypes = [i32, vp, PP(vp)]
    L.dfh_ctx_destroy.argtypes = [vp]
    L.dfh_ctx_sync.argtypes = [vp]
    L.dfh_ctx_stream.restype = vp
    L.dfh_ctx_stream.argtypes = [vp]
    L.dfh_ctx_device.argtypes = [vp]
    L.dfh_reverse_bytes.restype = u64
    L.dfh_reverse_bytes.argtypes = [u64]
    L.dfh_encode_fea_grp_id.restype = u64
    L.dfh_encode_fea_grp_id.argtypes = [u64, i32, i32]
    L.dfh_table_create.argtypes = [vp, PP(UpdaterParam), u64, PP(vp)]
    L.dfh_table_destroy.argtypes = [vp]
    L.dfh_table_size.argtypes = [vp, PP(u64)]
    L.dfh_table_param.argtypes = [vp, PP(UpdaterParam)]
    L.dfh_table_capacity.argtypes = [vp, PP(u64), PP(u64)]
    L.dfh_table_bytes.restype = u64
    L.dfh_table_bytes.argtypes = [vp]
    L.dfh_pull.argtypes = [vp, vp, sz, vp, PP(sz), vp, PP(sz)]
    L.dfh_push.argtypes = [vp, vp, sz, i32, vp, sz, vp, sz]
    L.dfh_table_export.argtypes = [vp, u64, vp, vp, vp, vp, PP(u64)]
    L.dfh_table_import.argtypes = [vp, u64, vp, vp, vp, vp]
    L.dfh_fm_predict.argtypes = [vp, i32, sz, vp, vp, vp, vp, sz, vp, vp, sz, vp]
    L.dfh_fm_calcgrad.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp]
    L.dfh_loss_evaluate.argtypes = [vp, vp, vp, sz, PP(f32)]
    L.dfh_auc_times_n.argtypes = [vp, vp, vp, sz, PP(f32)]
    L.dfh_batch_create.argtypes = [vp, sz, sz, PP(vp)]
    L.dfh_batch_destroy.argtypes = [vp]
    L.dfh_batch_create_many.argtypes = [vp, i32, sz, sz, PP(vp)]
    L.dfh_batch_split_entries.argtypes = [vp, vp]
    L.dfh_batch_key_view_info.argtypes = [vp, PP(KeyViewInfo)]
    L.dfh_batch_get_key_view.argtypes = [vp] * 12
    L.dfh_batch_load_host.argtypes = [vp, sz, vp, vp, vp, vp]
    L.dfh_batch_load_device.argtypes = [vp, sz, sz, vp, vp, vp, vp]
    L.dfh_batch_attach_device.argtypes = [vp, sz, sz, vp, vp, vp, vp]
    L.dfh_localize.argtypes = [vp, u64]
    L.dfh_batch_load_localized_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, sz]
    L.dfh_batch_get_localized.argtypes = [vp, PP(sz), vp, vp, vp]
    L.dfh_batch_shape.argtypes = [vp, PP(sz), PP(sz), PP(sz)]
    L.dfh_sgd_step.argtypes = [vp, vp, i32, i32]
    L.dfh_batch_progress.argtypes = [vp, PP(Progress), i32]
    L.dfh_batch_get_pred.argtypes = [vp, vp]
    L.dfh_row_stride.restype = sz
    L.dfh_row_stride.argtypes = [i32]
    L.dfh_shard_pull.argtypes = [vp, vp, sz, vp]
    L.dfh_shard_push_count.argtypes = [vp, vp, sz, vp]
    L.dfh_shard_push_grad.argtypes = [vp, vp, sz, vp]
    L.dfh_batch_forward.argtypes = [vp, i32, vp]
    L.dfh_batch_backward.argtypes = [vp, i32, vp, vp]
    L.dfh_batch_device_keys.argtypes = [vp, PP(vp), PP(vp), PP(sz)]
    L.dfh_malloc.argtypes = [vp, sz, PP(vp)]
    L.dfh_free.argtypes = [vp, vp]
    L.dfh_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.dfh_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.dfh_table_warm_start.argtypes = [vp, vp, sz, f32, f32]
    L.dfh_ctx_set_pipeline.argtypes = [vp, i32]
    L.dfh_batch_lookup.argtypes = [vp, vp]
    L.dfh_localize_lookup.argtypes = [vp, vp, C.c_uint64]
    L.dfh_rowbuf_create.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.dfh_rowbuf_destroy.argtypes = [vp]
    L.dfh_rowbuf_load_host.argtypes = [vp, C.c_size_t, vp, vp, vp]
    L.dfh_rowbuf_load_host_slices.argtypes = [vp, C.c_size_t, vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.dfh_textchunk_create.argtypes = [vp, sz, PP(vp)]
    L.dfh_textchunk_destroy.argtypes = [vp]
    L.dfh_textchunk_parse_criteo.argtypes = [vp, vp, sz, i32, PP(i32), PP(sz), PP(sz)]
    L.dfh_textchunk_rows.argtypes = [vp, vp, vp]
    L.dfh_textchunk_ids.argtypes = [vp, vp]
    L.dfh_lz4_compress.argtypes = [vp, vp, sz, vp, sz, PP(sz)]
    L.dfh_lz4_decompress.argtypes = [vp, vp, sz, vp, sz, PP(i32)]
    L.dfh_textchunk_decode_crb.argtypes = [vp, vp, sz, PP(i32), PP(sz), PP(sz)]
    L.dfh_crb_create.argtypes = [vp, PP(vp)]
    L.dfh_crb_destroy.argtypes = [vp]
    L.dfh_crb_encode_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, PP(sz)]
    L.dfh_crb_encode_textchunk.argtypes = [vp, vp, PP(sz)]
    L.dfh_crb_record.argtypes = [vp, vp]
    L.dfh_rowstore_create.argtypes = [vp, sz, PP(vp)]
    L.dfh_rowstore_destroy.argtypes = [vp]
    L.dfh_rowstore_append_host.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.dfh_rowstore_append_textchunk.argtypes = [vp, vp]
    L.dfh_rowstore_shape.argtypes = [vp, PP(C.c_uint64), PP(C.c_uint64), PP(i32), PP(i32), PP(C.c_uint64)]
    L.dfh_rowstore_order.argtypes = [vp, i32, C.c_uint64]
    L.dfh_rowstore_get_order.argtypes = [vp, vp]
    L.dfh_rowstore_read.argtypes = [vp, C.c_uint64, sz, vp, vp, vp, vp, vp, PP(sz)]
    L.dfh_crb_encode_rowstore.argtypes = [vp, vp, C.c_uint64, sz, PP(sz)]
    L.dfh_eval_create.argtypes = [vp, sz, PP(vp)]
    L.dfh_eval_destroy.argtypes = [vp]
    L.dfh_eval_reset.argtypes = [vp]
    L.dfh_eval_append_batch.argtypes = [vp, vp]
    L.dfh_eval_append_host.argtypes = [vp, vp, vp, sz]
    L.dfh_eval_finish.argtypes = [vp, PP(EvalResult)]
    L.dfh_predtext_create.argtypes = [vp, sz, PP(vp)]
    L.dfh_predtext_destroy.argtypes = [vp]
    L.dfh_predtext_reset.argtypes = [vp]
    L.dfh_predtext_append_batch.argtypes = [vp, vp]
    L.dfh_predtext_append_host.argtypes = [vp, vp, sz]
    L.dfh_predtext_count.argtypes = [vp, PP(C.c_uint64)]
    L.dfh_predtext_values.argtypes = [vp, vp]
    L.dfh_predtext_format.argtypes = [vp, PP(sz), PP(C.c_uint64)]
    L.dfh_predtext_read.argtypes = [vp, vp]
    L.dfh_predtext_tile.argtypes = []
    L.dfh_dump_open.argtypes = [vp, i32, PP(vp), PP(C.c_uint64)]
    L.dfh_dump_close.argtypes = [vp]
    L.dfh_dump_shape.argtypes = [vp, PP(C.c_uint64), PP(C.c_uint64), PP(i32)]
    L.dfh_dump_format.argtypes = [vp, C.c_uint64, sz, PP(sz), PP(C.c_uint64)]
    L.dfh_dump_read.argtypes = [vp, vp]
    L.dfh_dump_entries.argtypes = [vp, C.c_uint64, sz, vp, vp, vp, vp]
    L.dfh_dump_tile.argtypes = [vp]
    L.dfh_rowbuf_load_slices.argtypes = [vp, sz, vp, i32, PP(Slice)]
    L.dfh_batch_gather_rows.argtypes = [vp, C.c_size_t, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.dfh_batch_prepare_rows.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_uint64]
    L.dfh_rowbuf_set_labels.argtypes = [vp, C.c_size_t, vp]
    L.dfh_batch_get_rows.argtypes = [vp, vp, vp]
    L.dfh_batch_prepare_cached.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_uint64]
    L.dfh_batch_set_option.argtypes = [vp, C.c_char_p, i32]
    L.dfh_batch_key_ranges.argtypes = [vp, i32, vp]
    L.dfh_batch_key_ranges_device.argtypes = [vp, i32, vp, vp]
    L.dfh_shard_resolve.argtypes = [vp, vp, sz, vp]
    L.dfh_shard_pull_resolved.argtypes = [vp, vp, sz, vp]
    L.dfh_shard_push_count_resolved.argtypes = [vp, vp, vp, sz, vp]
    L.dfh_shard_push_grad_resolved.argtypes = [vp, vp, vp, sz, vp]
    L.dfh_table_check.argtypes = [vp]
    L.dfh_table_save.argtypes = [vp, C.c_char_p, i32, PP(u64)]
    L.dfh_table_load.argtypes = [vp, C.c_char_p, u64, u64, PP(i32), PP(u64)]
    L.dfh_shard_resolve_multi.argtypes = [vp, vp, vp, i32, i32, vp]
    L.dfh_shard_push_count_multi.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.dfh_shard_push_grad_multi.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.dfh_shard_count_pull_multi.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp]
    L.dfh_shard_push_grad_listed.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.dfh_shard_release.argtypes = [vp, vp, sz, i32]
    L.dfh_shard_multi_words.restype = sz
    L.dfh_shard_multi_words.argtypes = [sz, i32]
    L.dfh_ctx_set_timing.argtypes = [vp, i32]
    L.dfh_ctx_set_timing_mask.argtypes = [vp, C.c_uint32]
    L.dfh_ctx_get_timing.argtypes = [vp, i32, vp, vp]
    L.dfh_kernel_name.restype = C.c_char_p
    L.dfh_kernel_name.argtypes = [i32]
    L.dfh_ctx_set_option.argtypes = [vp, C.c_char_p, i32]
    L.dfh_table_set_has_aux.argtypes = [vp, i32]
    L.dfh_table_has_aux.argtypes = [vp]
    L.dfh_comm_unique_id.argtypes = [vp]
    L.dfh_comm_create_rccl.argtypes = [vp, i32, i32, vp, PP(vp)]
    L.dfh_comm_create_callback.argtypes = [vp, i32, i32, ALLTOALLV_FN, vp, PP(vp)]
    L.dfh_comm_destroy.argtypes = [vp]
    L.dfh_comm_rank.argtypes = [vp]
    L.dfh_comm_world.argtypes = [vp]
    L.dfh_comm_allreduce_sum.argtypes = [vp, vp, i32]
    L.dfh_shard_create.argtypes = [vp, vp, vp, PP(vp)]
    L.dfh_shard_destroy.argtypes = [vp]
    L.dfh_shard_owned_range.argtypes = [vp, vp, PP(u64), PP(u64)]
    L.dfh_shard_step.argtypes = [vp, vp, i32, i32, PP(i32)]
    L.dfh_shard_prefetch_counts.argtypes = [vp, vp]
    L.dfh_shard_pull_host.argtypes = [vp, vp, C.c_size_t, vp, PP(C.c_size_t), vp, PP(C.c_size_t)]
    L.dfh_shard_push_host.argtypes = [vp, vp, C.c_size_t, i32, vp, C.c_size_t, vp, C.c_size_t]
    L.dfh_comm_allgather.argtypes = [vp, vp, C.c_size_t, vp]
    L.dfh_comm_stats.argtypes = [vp, i32, vp, vp, vp]
    L.dfh_comm_info.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.dfh_comm_selfcheck.argtypes = [vp, C.c_double]
    L.dfh_comm_wire_probe.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.dfh_shard_balanced_splits.argtypes = [vp, vp, C.c_size_t, vp]
    L.dfh_shard_set_exchange.argtypes = [vp, i32]
    L.dfh_shard_reserve.argtypes = [vp, sz, sz]
    L.dfh_comm_create_loopback.argtypes = [vp, i32, i32, PP(vp)]
    L.dfh_comm_loopback_feed.argtypes = [vp, i32, vp, i32]
    L.dfh_comm_loopback_wire.argtypes = [vp, C.c_double, C.c_double]
    L.dfh_comm_loopback_wire_time.argtypes = [vp, i32, PP(C.c_double)]
    L.dfh_shard_set_timing.argtypes = [vp, i32]
    L.dfh_shard_get_timing.argtypes = [vp, i32, vp, PP(u64)]
    dp = PP(C.c_double)
    L.dfh_vec_inner_multi.argtypes = [vp, u64, i32, vp, i32, vp, dp]
    L.dfh_vec_combine.argtypes = [vp, u64, i32, vp, vp, f32, vp, vp, dp]
    L.dfh_vec_line_step.argtypes = [vp, u64, vp, vp, f32, vp, f32, f32, dp]
    L.dfh_lbfgs_create.argtypes = [vp, i32, i32, PP(vp)]
    L.dfh_lbfgs_create_sharded.argtypes = [vp, vp, i32, i32, PP(vp)]
    L.dfh_lbfgs_destroy.argtypes = [vp]
    L.dfh_lbfgs_add_chunk.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.dfh_lbfgs_init_model.argtypes = [vp, f32, i32, f32, f32, f32, PP(u64), PP(u64)]
    L.dfh_lbfgs_shape.argtypes = [vp, PP(u64), PP(u64), PP(i32), PP(i32)]
    L.dfh_lbfgs_get_model.argtypes = [vp, vp, vp, vp, vp]
    L.dfh_lbfgs_set_weights.argtypes = [vp, vp]
    L.dfh_lbfgs_owned_range.argtypes = [vp, PP(u64), PP(u64)]
    L.dfh_lbfgs_set_model.argtypes = [vp, u64, vp, vp, vp, PP(u64)]
    L.dfh_lbfgs_calc_grad.argtypes = [vp, f32, PP(f32), PP(f32)]
    L.dfh_lbfgs_prepare_direction.argtypes = [vp, vp, PP(i32)]
    L.dfh_lbfgs_calc_direction.argtypes = [vp, vp, PP(f32)]
    L.dfh_lbfgs_line_search.argtypes = [vp, f32, f32, PP(f32), PP(f32), PP(f32)]
    L.dfh_lbfgs_evaluate.argtypes = [vp, PP(f32), PP(f32), PP(f32)]
    L.dfh_lbfgs_get_vector.argtypes = [vp, i32, i32, vp]
    L.dfh_lbfgs_set_l1.argtypes = [vp, f32]
    L.dfh_lbfgs_get_owlqn_vector.argtypes = [vp, i32, vp]
    L.dfh_lbfgs_drop_last_pair.argtypes = [vp]
    L.dfh_lbfgs_get_owlqn_moved.argtypes = [vp, dp]
    L.dfh_bcd_create.argtypes = [vp, PP(vp)]
    L.dfh_bcd_create_sharded.argtypes = [vp, vp, PP(vp)]
    L.dfh_bcd_destroy.argtypes = [vp]
    L.dfh_bcd_add_chunk.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.dfh_bcd_build.argtypes = [vp, f32, i32, vp, vp, f32, f32, PP(u64)]
    L.dfh_bcd_shape.argtypes = [vp, PP(u64), PP(i32), PP(i32), PP(i32)]
    L.dfh_bcd_block_info.argtypes = [vp, i32, PP(i32), PP(i32), PP(u64), PP(u64)]
    L.dfh_bcd_epoch.argtypes = [vp, vp, i32, vp]
    L.dfh_bcd_step.argtypes = [vp, i32, vp, vp, vp]
    L.dfh_bcd_set_model.argtypes = [vp, u64, vp, vp, PP(u64)]
    L.dfh_bcd_get_model.argtypes = [vp, vp, vp, vp, vp, vp]
    L.dfh_bcd_get_pred.argtypes = [vp, i32, i32, vp, PP(sz)]
    _lib = L
    return L


def _ck(rc):
    if rc != 0:
        raise DfhError(rc, lib().dfh_last_error().decode())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(x):
    """device pointer: int, c_void_p or a torch tensor"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return x if isinstance(x, C.c_void_p) else C.c_void_p(int(x))


def make_param(V_dim=0, init_mode=INIT_HASH, **kw):
    p = UpdaterParam()
    lib().dfh_updater_param_default(C.byref(p), V_dim)
    p.init_mode = init_mode
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def reverse_bytes(x):
    return int(lib().dfh_reverse_bytes(int(x)))


class Context:
    """a HIP device + stream (dfh_ctx)"""

    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        _ck(lib().dfh_ctx_create(device, _dp(stream), C.byref(self.h)))

    def sync(self):
        _ck(lib().dfh_ctx_sync(self.h))

    def set_pipeline(self, on=True):
        """prepare later batches (copy, localize, lookup) on `on` preparation streams (True = 1)
        while an earlier batch trains on the main stream"""
        _ck(lib().dfh_ctx_set_pipeline(self.h, int(on)))

    def set_option(self, name, value):
        """validated launch tuning: fwd_depth, fwd_blocks, bwd_small_blocks, prep_priority"""
        _ck(lib().dfh_ctx_set_option(self.h, name.encode(), int(value)))

    def set_timing(self, on=True):
        _ck(lib().dfh_ctx_set_timing(self.h, 1 if on else 0))

    def set_timing_mask(self, mask):
        """time only the kernels whose bit (1 << K_*) is set"""
        _ck(lib().dfh_ctx_set_timing_mask(self.h, mask))

    def get_timing(self, reset=True):
        """{kernel name: (total_ms, calls)} from HIP events on this context's stream"""
        ms = np.zeros(K_COUNT, np.float64)
        calls = np.zeros(K_COUNT, np.uint64)
        _ck(lib().dfh_ctx_get_timing(self.h, 1 if reset else 0, _p(ms), _p(calls)))
        return {lib().dfh_kernel_name(i).decode(): (float(ms[i]), int(calls[i])) for i in range(K_COUNT)}

    @property
    def stream(self):
        return lib().dfh_ctx_stream(self.h)

    def close(self):
        if self.h:
            lib().dfh_ctx_destroy(self.h)
            self.h = None

    # literal Loss API ------------------------------------------------------
    def fm_predict(self, V_dim, offset, index, value, weights, w_pos=None, V_pos=None, pred0=None):
        """FMLoss::Predict (src/loss/fm_loss.h:67-119)"""
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint32)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        weights = np.ascontiguousarray(weights, np.float32)
        n = len(offset) - 1
        pred = np.zeros(n, np.float32) if pred0 is None else np.array(pred0, np.float32)
        npos = 0 if w_pos is None else len(w_pos)
        w_pos = None if w_pos is None else np.ascontiguousarray(w_pos, np.int32)
        V_pos = None if V_pos is None else np.ascontiguousarray(V_pos, np.int32)
        _ck(lib().dfh_fm_predict(self.h, V_dim, n, _p(offset), _p(index), _p(value), _p(weights), len(weights),
                                 _p(w_pos), _p(V_pos), npos, _p(pred)))
        return pred

    def fm_calcgrad(self, V_dim, offset, index, value, label, weights, pred, w_pos=None, V_pos=None):
        """FMLoss::CalcGrad (src/loss/fm_loss.h:148-199)"""
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint32)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        weights = np.ascontiguousarray(weights, np.float32)
        label = np.ascontiguousarray(label, np.float32)
        pred = np.ascontiguousarray(pred, np.float32)
        n = len(offset) - 1
        grad = np.zeros(len(weights), np.float32)
        npos = 0 if w_pos is None else len(w_pos)
        w_pos = None if w_pos is None else np.ascontiguousarray(w_pos, np.int32)
        V_pos = None if V_pos is None else np.ascontiguousarray(V_pos, np.int32)
        _ck(lib().dfh_fm_calcgrad(self.h, V_dim, n, _p(offset), _p(index), _p(value), _p(label), _p(weights),
                                  len(weights), _p(w_pos), _p(V_pos), npos, _p(pred), _p(grad)))
        return grad

    def auc_times_n(self, label, pred):
        """BinClassMetric::AUC (src/loss/bin_class_metric.h:35-56): AUC * n"""
        label = np.ascontiguousarray(label, np.float32)
        pred = np.ascontiguousarray(pred, np.float32)
        o = C.c_float(0)
        _ck(lib().dfh_auc_times_n(self.h, _p(label), _p(pred), len(pred), C.byref(o)))
        return o.value

    def loss_evaluate(self, label, pred):
        label = np.ascontiguousarray(label, np.float32)
        pred = np.ascontiguousarray(pred, np.float32)
        o = C.c_float(0)
        _ck(lib().dfh_loss_evaluate(self.h, _p(label), _p(pred), len(pred), C.byref(o)))
        return o.value


class Table:
    """one shard of the model in HBM (dfh_table): replaces Store + SGDUpdater state"""

    def __init__(self, ctx, capacity, V_dim=0, init_mode=INIT_HASH, **kw):
        self.ctx = ctx
        self.param = make_param(V_dim, init_mode, **kw)
        self.V_dim = V_dim
        self.h = C.c_void_p()
        _ck(lib().dfh_table_create(ctx.h, C.byref(self.param), capacity, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().dfh_table_destroy(self.h)
            self.h = None

    def size(self):
        n = C.c_uint64(0)
        _ck(lib().dfh_table_size(self.h, C.byref(n)))
        return n.value

    def capacity(self):
        """(rows the arrays hold now, number of growths) — a table created with capacity 0 grows"""
        c, g = C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_table_capacity(self.h, C.byref(c), C.byref(g)))
        return c.value, g.value

    def bytes(self):
        return int(lib().dfh_table_bytes(self.h))

    def pull(self, keys):
        """Store::Pull(kWeight) -> (vals ragged, lens)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(keys)
        vals = np.zeros(max(n * (1 + self.V_dim), 1), np.float32)
        lens = np.zeros(max(n, 1), np.int32)
        nv, nl = C.c_size_t(0), C.c_size_t(0)
        _ck(lib().dfh_pull(self.h, _p(keys), n, _p(vals), C.byref(nv), _p(lens), C.byref(nl)))
        return vals[:nv.value].copy(), lens[:nl.value].copy()

    def push(self, keys, val_type, vals, lens=None):
        """Store::Push(kFeaCount | kGradient)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.float32)
        lens = np.zeros(0, np.int32) if lens is None else np.ascontiguousarray(lens, np.int32)
        _ck(lib().dfh_push(self.h, _p(keys), len(keys), val_type, _p(vals), len(vals), _p(lens), len(lens)))

    def export(self):
        n = self.size()
        k = self.V_dim
        keys = np.zeros(max(n, 1), np.uint64)
        scal = np.zeros(max(n, 1) * 4, np.float32)
        has = np.zeros(max(n, 1), np.int32)
        V = np.zeros(max(n * 2 * k, 1), np.float32)
        m = C.c_uint64(0)
        _ck(lib().dfh_table_export(self.h, max(n, 1), _p(keys), _p(scal), _p(has), _p(V), C.byref(m)))
        n = m.value
        return dict(keys=keys[:n], scal=scal[:4 * n].reshape(n, 4), has_V=has[:n], V=V[:n * 2 * k].reshape(n, 2 * k) if k else None)

    def import_(self, keys, scal, has_V, V=None):
        keys = np.ascontiguousarray(keys, np.uint64)
        scal = np.ascontiguousarray(scal, np.float32)
        has_V = np.ascontiguousarray(has_V, np.int32)
        V = None if V is None else np.ascontiguousarray(V, np.float32)
        _ck(lib().dfh_table_import(self.h, len(keys), _p(keys), _p(scal), _p(has_V), _p(V)))

    def save(self, path, save_aux=True):
        """Updater::Save to a file (the C++ host's model format); returns the number of entries written"""
        n = C.c_uint64(0)
        _ck(lib().dfh_table_save(self.h, str(path).encode(), 1 if save_aux else 0, C.byref(n)))
        return n.value

    def load(self, path, key_lo=0, key_hi=0):
        """Updater::Load of the keys in [key_lo, key_hi) (key_hi = 0: unbounded) -> (entries loaded, has_aux)"""
        n, aux = C.c_uint64(0), C.c_int(0)
        _ck(lib().dfh_table_load(self.h, str(path).encode(), key_lo, key_hi, C.byref(aux), C.byref(n)))
        return n.value, bool(aux.value)

    @property
    def has_aux(self):
        """SGDUpdater::has_aux_: False after loading a model saved without optimiser state"""
        return bool(lib().dfh_table_has_aux(self.h))

    def set_has_aux(self, on):
        _ck(lib().dfh_table_set_has_aux(self.h, 1 if on else 0))

    def warm_start(self, d_keys, n, w0=0.01, cnt0=100.0):
        _ck(lib().dfh_table_warm_start(self.h, _dp(d_keys), n, w0, cnt0))

    # device-pointer (sharded) calls
    def shard_pull(self, d_keys, n, d_rows):
        _ck(lib().dfh_shard_pull(self.h, _dp(d_keys), n, _dp(d_rows)))

    def shard_push_count(self, d_keys, n, d_cnt):
        _ck(lib().dfh_shard_push_count(self.h, _dp(d_keys), n, _dp(d_cnt)))

    def shard_push_grad(self, d_keys, n, d_grads):
        _ck(lib().dfh_shard_push_grad(self.h, _dp(d_keys), n, _dp(d_grads)))

    # resolved form: probe all received keys once, then work on row ids
    def shard_resolve(self, d_keys, n, d_rowid):
        _ck(lib().dfh_shard_resolve(self.h, _dp(d_keys), n, _dp(d_rowid)))

    def shard_pull_resolved(self, d_rowid, n, d_rows):
        _ck(lib().dfh_shard_pull_resolved(self.h, _dp(d_rowid), n, _dp(d_rows)))

    def shard_push_count_resolved(self, d_rowid, d_keys, n, d_cnt):
        _ck(lib().dfh_shard_push_count_resolved(self.h, _dp(d_rowid), _dp(d_keys), n, _dp(d_cnt)))

    def shard_push_grad_resolved(self, d_rowid, d_keys, n, d_grads):
        _ck(lib().dfh_shard_push_grad_resolved(self.h, _dp(d_rowid), _dp(d_keys), n, _dp(d_grads)))

    # all source ranks of a step in one launch (seg: nsrc+1 host offsets into the concatenated lists)
    @staticmethod
    def _seg(seg):
        a = np.ascontiguousarray(seg, dtype=np.uint64)
        return a, len(a) - 1

    def shard_resolve_multi(self, d_keys, seg, d_rowid, mask_slot=0):
        a, n = self._seg(seg)
        _ck(lib().dfh_shard_resolve_multi(self.h, _dp(d_keys), _p(a), n, mask_slot, _dp(d_rowid)))

    def shard_push_count_multi(self, d_rowid, d_keys, seg, d_cnt, mask_slot=0):
        a, n = self._seg(seg)
        _ck(lib().dfh_shard_push_count_multi(self.h, _dp(d_rowid), _dp(d_keys), _p(a), n, mask_slot, _dp(d_cnt)))

    def shard_push_grad_multi(self, d_rowid, d_keys, seg, d_grads, mask_slot=0):
        a, n = self._seg(seg)
        _ck(lib().dfh_shard_push_grad_multi(self.h, _dp(d_rowid), _dp(d_keys), _p(a), n, mask_slot, _dp(d_grads)))

    def shard_count_pull_multi(self, d_rowid, d_keys, seg, d_cnt, d_rows, mask_slot=0):
        """Push(kFeaCount) of all sources (d_cnt or None) + Pull per distinct key; leaves the key lists of push_grad_listed"""
        a, n = self._seg(seg)
        _ck(lib().dfh_shard_count_pull_multi(self.h, _dp(d_rowid), _dp(d_keys), _p(a), n, mask_slot,
                                             _dp(d_cnt) if d_cnt is not None else None, _dp(d_rows)))

    def shard_push_grad_listed(self, d_rowid, d_keys, seg, d_grads, mask_slot=0):
        a, n = self._seg(seg)
        _ck(lib().dfh_shard_push_grad_listed(self.h, _dp(d_rowid), _dp(d_keys), _p(a), n, mask_slot, _dp(d_grads)))

    def shard_release(self, d_rowid, n, mask_slot=0):
        _ck(lib().dfh_shard_release(self.h, _dp(d_rowid), n, mask_slot))

    def check(self):
        """raise if the device-side error word is set (capacity / duplicate key / V mismatch)"""
        _ck(lib().dfh_table_check(self.h))


class RowBuf:
    """a shuffle buffer in HBM (dfh_rowbuf): rows are gathered out of it on the device (Batch.gather_rows)"""

    def __init__(self, ctx, max_rows, max_nnz):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_rowbuf_create(ctx.h, max_rows, max_nnz, C.byref(self.h)))

    def load_host(self, offset, index, value=None):
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint64)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        _ck(lib().dfh_rowbuf_load_host(self.h, len(offset) - 1, _p(offset), _p(index), _p(value)))

    def load_host_slices(self, offset, slices):
        """dfh_rowbuf_load_host_slices: the ids / values as consecutive pieces [(index, value or None), ...]"""
        offset = np.ascontiguousarray(offset, np.uint64)
        idx = [np.ascontiguousarray(i, np.uint64) for i, _ in slices]
        val = [None if v is None else np.ascontiguousarray(v, np.float32) for _, v in slices]
        n = len(slices)
        ip = (C.c_void_p * n)(*[i.ctypes.data for i in idx])
        vp = (C.c_void_p * n)(*[None if v is None else v.ctypes.data for v in val])
        cnt = (C.c_size_t * n)(*[len(i) for i in idx])
        _ck(lib().dfh_rowbuf_load_host_slices(self.h, len(offset) - 1, _p(offset), n, ip, vp, cnt))

    def load_slices(self, offset, slices):
        """dfh_rowbuf_load_slices: the ids as consecutive pieces, each (index, value or None) host arrays or
        (TextChunk, first, nnz) = ids [first, first + nnz) of a parsed chunk, copied device to device"""
        offset = np.ascontiguousarray(offset, np.uint64)
        arr = (Slice * max(len(slices), 1))()
        keep = []
        for g, sl in enumerate(slices):
            if isinstance(sl[0], TextChunk):
                arr[g] = Slice(None, None, sl[0].h, int(sl[1]), int(sl[2]))
            else:
                idx = np.ascontiguousarray(sl[0], np.uint64)
                val = None if sl[1] is None else np.ascontiguousarray(sl[1], np.float32)
                keep.append((idx, val))
                arr[g] = Slice(idx.ctypes.data, None if val is None else val.ctypes.data, None, 0, len(idx))
        _ck(lib().dfh_rowbuf_load_slices(self.h, len(offset) - 1, _p(offset), len(slices), arr))

    def set_labels(self, label):
        """dfh_rowbuf_set_labels: the labels of the loaded rows (a buffer that stays: Batch.prepare_cached)"""
        label = np.ascontiguousarray(label, np.float32)
        _ck(lib().dfh_rowbuf_set_labels(self.h, len(label), _p(label)))

    def close(self):
        if self.h:
            lib().dfh_rowbuf_destroy(self.h)
            self.h = None


class TextChunk:
    """one chunk of criteo text parsed on the device (dfh_textchunk): its ids stay in HBM"""

    def __init__(self, ctx, max_bytes=1 << 16):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_textchunk_create(ctx.h, max_bytes, C.byref(self.h)))

    def parse_criteo(self, text, is_train=True, address=None):
        """-> None when the chunk is not regular (the caller parses it on the host), else (offset u32 [nrows + 1], label
        [nrows], nnz).  `address`: parse len(text) bytes at that address instead of a copy of `text`"""
        buf = None
        if address is None:
            buf = C.create_string_buffer(bytes(text), len(text)) if len(text) else C.create_string_buffer(1)
            address = C.addressof(buf)
        reg, nrows, nnz = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        _ck(lib().dfh_textchunk_parse_criteo(self.h, C.c_void_p(address), len(text), 1 if is_train else 0, C.byref(reg), C.byref(nrows),
                                             C.byref(nnz)))
        if not reg.value:
            return None
        off = np.zeros(nrows.value + 1, np.uint32)
        lab = np.zeros(max(nrows.value, 1), np.float32)
        _ck(lib().dfh_textchunk_rows(self.h, _p(off), _p(lab)))
        return off, lab[:nrows.value], nnz.value

    def decode_crb(self, record):
        """one CompressedRowBlock record (bytes) decoded on the device (dfh_textchunk_decode_crb) -> None when the record is not
        regular (the caller inflates it on the host), else (offset u32 [nrows + 1], label [nrows], nnz)"""
        record = bytes(record)
        buf = C.create_string_buffer(record, len(record)) if len(record) else C.create_string_buffer(1)
        reg, nrows, nnz = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        _ck(lib().dfh_textchunk_decode_crb(self.h, buf, len(record), C.byref(reg), C.byref(nrows), C.byref(nnz)))
        if not reg.value:
            return None
        off = np.zeros(nrows.value + 1, np.uint32)
        lab = np.zeros(max(nrows.value, 1), np.float32)
        _ck(lib().dfh_textchunk_rows(self.h, _p(off), _p(lab)))
        return off, lab[:nrows.value], nnz.value

    def ids(self, nnz):
        out = np.zeros(max(nnz, 1), np.uint64)
        _ck(lib().dfh_textchunk_ids(self.h, _p(out)))
        return out[:nnz]

    def close(self):
        if self.h:
            lib().dfh_textchunk_destroy(self.h)
            self.h = None


def lz4_compress(ctx, data):
    """one LZ4 block of `data` (bytes), encoded on the device (dfh_lz4_compress)"""
    data = bytes(data)
    n = len(data)
    cap = n + n // 255 + 16
    src = C.create_string_buffer(data, n) if n else C.create_string_buffer(1)
    dst = C.create_string_buffer(cap)
    out = C.c_size_t(0)
    _ck(lib().dfh_lz4_compress(ctx.h, src, n, dst, cap, C.byref(out)))
    return dst.raw[:out.value]


def lz4_decompress(ctx, block, expect, fill=0xA5):
    """the LZ4 block `block` (bytes) decoded on the device (dfh_lz4_decompress) into a buffer of `expect` bytes that held `fill`
    in every byte -> (ok, the buffer's bytes afterwards)"""
    block = bytes(block)
    n = len(block)
    src = C.create_string_buffer(block, n) if n else C.create_string_buffer(1)
    dst = C.create_string_buffer(bytes([fill]) * max(expect, 1), max(expect, 1))
    ok = C.c_int(-1)
    _ck(lib().dfh_lz4_decompress(ctx.h, src, n, dst, expect, C.byref(ok)))
    return ok.value, dst.raw[:expect]


class CrbEncoder:
    """writes CompressedRowBlock records on the device (dfh_crb): the payload of one RecordIO record of a .rec file"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_crb_create(ctx.h, C.byref(self.h)))

    def _record(self, nbytes):
        dst = C.create_string_buffer(nbytes)
        _ck(lib().dfh_crb_record(self.h, dst))
        return dst.raw

    def encode_host(self, offset, label, index=None, value=None, weight=None):
        """offset u64 [nrows + 1], label f32 [nrows], index u64 / value f32 [nnz] (the block's own), weight f32 [nrows] -> bytes"""
        offset = np.ascontiguousarray(offset, np.uint64)
        label = np.ascontiguousarray(label, np.float32)
        keep = [offset, label]
        ptr = []
        for a, t in ((index, np.uint64), (value, np.float32), (weight, np.float32)):
            if a is None:
                ptr.append(None)
            else:
                a = np.ascontiguousarray(a, t)
                keep.append(a)
                ptr.append(C.c_void_p(a.ctypes.data) if a.size else None)   # (an array of zero elements is written as absent)
        n = C.c_size_t(0)
        lab = _p(label) if label.size else C.create_string_buffer(8)
        _ck(lib().dfh_crb_encode_host(self.h, len(offset) - 1, _p(offset), lab, ptr[0], ptr[1], ptr[2], C.byref(n)))
        return self._record(n.value)

    def encode_textchunk(self, tc):
        """the record of the regular chunk last parsed into the TextChunk `tc`"""
        n = C.c_size_t(0)
        _ck(lib().dfh_crb_encode_textchunk(self.h, tc.h, C.byref(n)))
        return self._record(n.value)

    def encode_rowstore(self, store, first, count):
        """the record of rows order[first .. first + count) of the ordered RowStore `store`"""
        n = C.c_size_t(0)
        _ck(lib().dfh_crb_encode_rowstore(self.h, store.h, first, count, C.byref(n)))
        return self._record(n.value)

    def close(self):
        if self.h:
            lib().dfh_crb_destroy(self.h)
            self.h = None


class RowStore:
    """the rows of a whole data set in HBM (dfh_rowstore): appended chunk by chunk, ordered once, read or encoded block by block"""

    def __init__(self, ctx, slab_bytes=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_rowstore_create(ctx.h, slab_bytes, C.byref(self.h)))

    def append_host(self, offset, label, index=None, value=None, weight=None):
        """offset u64 [nrows + 1], label f32 [nrows], index u64 / value f32 [nnz] (the chunk's own), weight f32 [nrows]"""
        offset = np.ascontiguousarray(offset, np.uint64)
        label = np.ascontiguousarray(label, np.float32)
        arrs = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((index, np.uint64), (value, np.float32), (weight, np.float32))]
        ptr = [None if a is None else (_p(a) if a.size else C.create_string_buffer(8)) for a in arrs]
        lab = _p(label) if label.size else C.create_string_buffer(8)
        _ck(lib().dfh_rowstore_append_host(self.h, len(offset) - 1, _p(offset), lab, ptr[0], ptr[1], ptr[2]))

    def append_textchunk(self, tc):
        """the regular chunk last parsed into the TextChunk `tc`, device to device"""
        _ck(lib().dfh_rowstore_append_textchunk(self.h, tc.h))

    def shape(self):
        """-> dict(nrows, nnz, has_value, has_weight, device_bytes)"""
        nrows, nnz, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        hv, hw = C.c_int(0), C.c_int(0)
        _ck(lib().dfh_rowstore_shape(self.h, C.byref(nrows), C.byref(nnz), C.byref(hv), C.byref(hw), C.byref(nb)))
        return dict(nrows=nrows.value, nnz=nnz.value, has_value=bool(hv.value), has_weight=bool(hw.value), device_bytes=nb.value)

    def order(self, shuffle, seed=0):
        _ck(lib().dfh_rowstore_order(self.h, int(shuffle), seed))

    def get_order(self):
        out = np.zeros(max(self.shape()["nrows"], 1), np.uint32)
        _ck(lib().dfh_rowstore_get_order(self.h, _p(out)))
        return out[:self.shape()["nrows"]]

    def read(self, first, count):
        """rows order[first .. first + count) -> (offset u64 [count + 1], label, index, value, weight | None)"""
        off = np.zeros(count + 1, np.uint64)
        lab = np.zeros(max(count, 1), np.float32)
        nnz = C.c_size_t(0)
        _ck(lib().dfh_rowstore_read(self.h, first, count, _p(off), _p(lab), None, None, None, C.byref(nnz)))
        idx = np.zeros(max(nnz.value, 1), np.uint64)
        val = np.zeros(max(nnz.value, 1), np.float32)
        wgt = np.zeros(max(count, 1), np.float32) if self.shape()["has_weight"] else None
        _ck(lib().dfh_rowstore_read(self.h, first, count, _p(off), _p(lab), _p(idx), _p(val), _p(wgt), C.byref(nnz)))
        return off, lab[:count], idx[:nnz.value], val[:nnz.value], None if wgt is None else wgt[:count]

    def close(self):
        if self.h:
            lib().dfh_rowstore_destroy(self.h)
            self.h = None


class Eval:
    """whole-set evaluation on the device (dfh_eval): exact AUC, logloss and accuracy of the appended rows"""

    def __init__(self, ctx, capacity_hint=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_eval_create(ctx.h, capacity_hint, C.byref(self.h)))

    def reset(self):
        _ck(lib().dfh_eval_reset(self.h))

    def append_batch(self, batch):
        """the batch's predictions and labels, queued behind its last step; does not wait"""
        _ck(lib().dfh_eval_append_batch(self.h, batch.h))

    def append_host(self, label, pred):
        label = np.ascontiguousarray(label, np.float32)
        pred = np.ascontiguousarray(pred, np.float32)
        assert label.shape == pred.shape and label.ndim == 1
        _ck(lib().dfh_eval_append_host(self.h, _p(label), _p(pred), label.size))

    def finish(self):
        """-> EvalResult; everything appended since the last reset (waits; nothing is consumed)"""
        r = EvalResult()
        _ck(lib().dfh_eval_finish(self.h, C.byref(r)))
        return r

    def close(self):
        if self.h:
            lib().dfh_eval_destroy(self.h)
            self.h = None


class _LibInt:
    """a class attribute whose value the library exports as an int function of no arguments"""

    def __init__(self, symbol):
        self.symbol = symbol

    def __get__(self, obj, cls):
        return int(getattr(lib(), self.symbol)())


class PredText:
    """prediction text on the device (dfh_predtext): the bytes of fprintf("%.9g\\n", v) for the appended values"""

    TILE = _LibInt("dfh_predtext_tile")   # the values a block of the format kernels takes

    def __init__(self, ctx, capacity_hint=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_predtext_create(ctx.h, capacity_hint, C.byref(self.h)))

    def reset(self):
        _ck(lib().dfh_predtext_reset(self.h))

    def append_batch(self, batch):
        """the batch's predictions, queued behind its last step; does not wait"""
        _ck(lib().dfh_predtext_append_batch(self.h, batch.h))

    def append_host(self, v):
        v = np.ascontiguousarray(v, np.float32)
        assert v.ndim == 1
        _ck(lib().dfh_predtext_append_host(self.h, _p(v), v.size))

    def count(self):
        n = C.c_uint64(0)
        _ck(lib().dfh_predtext_count(self.h, C.byref(n)))
        return n.value

    def values(self):
        """the appended floats (waits)"""
        out = np.zeros(max(self.count(), 1), np.float32)
        _ck(lib().dfh_predtext_values(self.h, _p(out)))
        return out[:self.count()]

    def format(self):
        """-> (text bytes, irregular); everything appended since the last reset (waits; nothing is consumed).  The text is
        valid when irregular == 0, else it is b'' and the caller formats values() itself"""
        nb, irr = C.c_size_t(0), C.c_uint64(0)
        _ck(lib().dfh_predtext_format(self.h, C.byref(nb), C.byref(irr)))
        if irr.value or nb.value == 0:
            return b"", irr.value
        buf = C.create_string_buffer(nb.value)
        _ck(lib().dfh_predtext_read(self.h, buf))
        return buf.raw, irr.value

    def close(self):
        if self.h:
            lib().dfh_predtext_destroy(self.h)
            self.h = None


DUMP_IDS_FEATURE, DUMP_IDS_KEY = 0, 1


class ModelDump:
    """a table's kept entries in ascending order of their printed id, and their text "<id>\\t<w>[\\t<V_j>]\\n" formatted on the
    device (dfh_dump).  The table must stay open and unchanged while the dump is"""

    def __init__(self, table, ids_mode=DUMP_IDS_FEATURE):
        self.table = table
        self.V_dim = table.V_dim
        self.h = C.c_void_p()
        n = C.c_uint64(0)
        _ck(lib().dfh_dump_open(table.h, ids_mode, C.byref(self.h), C.byref(n)))
        self.n = n.value

    @property
    def tile(self):
        """the entries a block of the format kernels takes (by V_dim; tiles count from a unit's first entry)"""
        return int(lib().dfh_dump_tile(self.h))

    def shape(self):
        """-> (kept entries, those with V, V_dim)"""
        n, nv, k = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        _ck(lib().dfh_dump_shape(self.h, C.byref(n), C.byref(nv), C.byref(k)))
        return n.value, nv.value, k.value

    def format(self, first=0, count=None):
        """-> (text bytes, irregular) of entries [first, first + count) (count None: to the end).  The text is valid when
        irregular == 0, else it is b'' and the caller formats entries(first, count) itself"""
        count = self.n - first if count is None else count
        nb, irr = C.c_size_t(0), C.c_uint64(0)
        _ck(lib().dfh_dump_format(self.h, first, count, C.byref(nb), C.byref(irr)))
        if irr.value or nb.value == 0:
            return b"", irr.value
        buf = C.create_string_buffer(nb.value)
        _ck(lib().dfh_dump_read(self.h, buf))
        return buf.raw, irr.value

    def entries(self, first=0, count=None):
        """-> dict(ids, w, has_V, V [count x V_dim] or None) of the same entries"""
        count = self.n - first if count is None else count
        k = self.V_dim
        ids = np.zeros(max(count, 1), np.uint64)
        w = np.zeros(max(count, 1), np.float32)
        has = np.zeros(max(count, 1), np.int32)
        V = np.zeros(max(count * k, 1), np.float32)
        _ck(lib().dfh_dump_entries(self.h, first, count, _p(ids), _p(w), _p(has), _p(V)))
        return dict(ids=ids[:count], w=w[:count], has_V=has[:count], V=V[:count * k].reshape(count, k) if k else None)

    def close(self):
        if self.h:
            lib().dfh_dump_close(self.h)
            self.h = None


def create_batches(ctx, n, max_rows, max_nnz):
    """n Batch objects carved from one device allocation (dfh_batch_create_many)"""
    hs = (C.c_void_p * n)()
    _ck(lib().dfh_batch_create_many(ctx.h, n, max_rows, max_nnz, hs))
    out = []
    for i in range(n):
        b = Batch.__new__(Batch)
        b.ctx, b.h = ctx, C.c_void_p(hs[i])
        out.append(b)
    return out


class Batch:
    """a device-resident minibatch + workspace (dfh_batch)"""

    def __init__(self, ctx, max_rows, max_nnz):
        self.ctx = ctx
        self.h = C.c_void_p()
        _ck(lib().dfh_batch_create(ctx.h, max_rows, max_nnz, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().dfh_batch_destroy(self.h)
            self.h = None

    def load_host(self, offset, index, value, label):
        """raw CSR with u64 feature ids (what Reader::Value() yields)"""
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint64)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        label = np.ascontiguousarray(label, np.float32)
        _ck(lib().dfh_batch_load_host(self.h, len(offset) - 1, _p(offset), _p(index), _p(value), _p(label)))

    def load_device(self, nrows, nnz, d_offset, d_index, d_value, d_label):
        _ck(lib().dfh_batch_load_device(self.h, nrows, nnz, _dp(d_offset), _dp(d_index), _dp(d_value), _dp(d_label)))

    def attach_device(self, nrows, nnz, d_offset, d_index, d_value, d_label):
        """zero-copy: read the caller's device arrays in place"""
        _ck(lib().dfh_batch_attach_device(self.h, nrows, nnz, _dp(d_offset), _dp(d_index), _dp(d_value), _dp(d_label)))

    def localize(self, max_index=U64MAX, table=None):
        """Localizer::Compact on device; with a table also the key-index probe (dfh_localize_lookup)"""
        if table is None:
            _ck(lib().dfh_localize(self.h, max_index))
        else:
            _ck(lib().dfh_localize_lookup(table.h, self.h, max_index))

    def set_option(self, name, value):
        _ck(lib().dfh_batch_set_option(self.h, name.encode(), int(value)))

    def lookup(self, table):
        _ck(lib().dfh_batch_lookup(table.h, self.h))

    def gather_rows(self, offset, label, segments):
        """dfh_batch_gather_rows: the minibatch = rows `rows` of row buffer `rb` for every (rb, rows) of `segments`, in order;
        offset / label are the minibatch's own (cumulative row lengths, labels)"""
        offset = np.ascontiguousarray(offset, np.uint64)
        label = np.ascontiguousarray(label, np.float32)
        rows = [np.ascontiguousarray(r, np.uint32) for _, r in segments]
        n = len(segments)
        bufs = (C.c_void_p * n)(*[rb.h for rb, _ in segments])
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        cnts = (C.c_size_t * n)(*[len(r) for r in rows])
        _ck(lib().dfh_batch_gather_rows(self.h, len(label), _p(offset), _p(label), n, bufs, ptrs, cnts))

    def prepare_rows(self, table, offset, label, segments, max_index=2 ** 64 - 1):
        """dfh_batch_prepare_rows: gather_rows + localize + lookup(table) as one preparation phase"""
        offset = np.ascontiguousarray(offset, np.uint64)
        label = np.ascontiguousarray(label, np.float32)
        rows = [np.ascontiguousarray(r, np.uint32) for _, r in segments]
        n = len(segments)
        bufs = (C.c_void_p * n)(*[rb.h for rb, _ in segments])
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        cnts = (C.c_size_t * n)(*[len(r) for r in rows])
        _ck(lib().dfh_batch_prepare_rows(table.h, self.h, len(label), _p(offset), _p(label), n, bufs, ptrs, cnts, max_index))

    def prepare_cached(self, table, segments, max_index=2 ** 64 - 1):
        """dfh_batch_prepare_cached: prepare_rows out of row buffers that carry their labels — the row numbers are all the host
        sends, the minibatch's offsets and labels are derived on the device"""
        rows = [np.ascontiguousarray(r, np.uint32) for _, r in segments]
        n = len(segments)
        bufs = (C.c_void_p * n)(*[rb.h for rb, _ in segments])
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        cnts = (C.c_size_t * n)(*[len(r) for r in rows])
        _ck(lib().dfh_batch_prepare_cached(table.h, self.h, sum(len(r) for r in rows), n, bufs, ptrs, cnts, max_index))

    def load_localized_host(self, offset, index, value, label, feaids, feacnt=None):
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint32)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        label = np.ascontiguousarray(label, np.float32)
        feaids = np.ascontiguousarray(feaids, np.uint64)
        feacnt = None if feacnt is None else np.ascontiguousarray(feacnt, np.float32)
        _ck(lib().dfh_batch_load_localized_host(self.h, len(offset) - 1, _p(offset), _p(index), _p(value), _p(label),
                                                _p(feaids), _p(feacnt), len(feaids)))

    def shape(self, want_U=True):
        a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _ck(lib().dfh_batch_shape(self.h, C.byref(a), C.byref(b), C.byref(c) if want_U else None))
        return a.value, b.value, c.value

    def get_localized(self):
        nrows, nnz, U = self.shape()
        feaids = np.zeros(max(U, 1), np.uint64)
        cnt = np.zeros(max(U, 1), np.float32)
        index = np.zeros(max(nnz, 1), np.uint32)
        u = C.c_size_t(0)
        _ck(lib().dfh_batch_get_localized(self.h, C.byref(u), _p(feaids), _p(cnt), _p(index)))
        return dict(U=U, feaids=feaids[:U], feacnt=cnt[:U], index=index[:nnz])

    def get_rows(self):
        """the loaded minibatch's offsets and labels as the device holds them"""
        nrows, _, _ = self.shape(want_U=False)
        off = np.zeros(nrows + 1, np.uint32)
        lab = np.zeros(nrows, np.float32)
        _ck(lib().dfh_batch_get_rows(self.h, _p(off), _p(lab)))
        return off, lab

    def sgd_step(self, table, is_train=True, push_cnt=False):
        """the batch executor of SGDLearner::IterateData, on device (async)"""
        _ck(lib().dfh_sgd_step(table.h, self.h, 1 if is_train else 0, 1 if push_cnt else 0))

    def progress(self, reset=True):
        p = Progress()
        _ck(lib().dfh_batch_progress(self.h, C.byref(p), 1 if reset else 0))
        return p

    def pred(self):
        nrows, _, _ = self.shape(want_U=False)
        out = np.zeros(nrows, np.float32)
        _ck(lib().dfh_batch_get_pred(self.h, _p(out)))
        return out

    def split_entries(self):
        """entries the last training step put on the split list (parts of the keys with more than 4 096 occurrences)"""
        n = C.c_uint32(0)
        _ck(lib().dfh_batch_split_entries(self.h, C.byref(n)))
        return int(n.value)

    def get_key_view(self):
        """the key-ordered view and the segment lists as the backward and update passes walk them (dfh_batch_get_key_view):
        col_ptr, s_row, s_val (None: binary); few / mid / hot = dict(desc [seg_nb, 2] {cnt, off}, cap, buckets = the entries
        [cnt, 4] of every list bucket's [off, off + cnt), None where that range leaves the array); split [split_n, 4];
        P and bstart [P + 1] where the minibatch came out of the sample sort (else P = 0, bstart None); the class bounds"""
        info = KeyViewInfo()
        _ck(lib().dfh_batch_key_view_info(self.h, C.byref(info)))
        U, nnz, nb = int(info.U), int(info.nnz), int(info.seg_nb)
        col_ptr = np.zeros(U + 1, np.uint32)
        s_row = np.zeros(max(nnz, 1), np.uint32)
        s_val = np.zeros(max(nnz, 1), np.float32) if info.has_value else None
        caps = dict(few=int(info.few_cap), mid=int(info.mid_cap), hot=int(info.hot_cap))
        desc = {k: np.zeros((max(nb, 1), 2), np.uint32) for k in caps}
        ent = {k: np.zeros((caps[k], 4), np.uint32) for k in caps}
        ns = min(int(info.split_n), int(info.split_cap))
        split = np.zeros((max(ns, 1), 4), np.uint32)
        bstart = np.zeros(int(info.P) + 1, np.uint32) if info.P else None
        _ck(lib().dfh_batch_get_key_view(self.h, _p(col_ptr), _p(s_row), _p(s_val), _p(desc["few"]), _p(ent["few"]),
                                         _p(desc["mid"]), _p(ent["mid"]), _p(desc["hot"]), _p(ent["hot"]), _p(split), _p(bstart)))
        out = dict(U=U, nnz=nnz, col_ptr=col_ptr, s_row=s_row[:nnz], s_val=None if s_val is None else s_val[:nnz],
                   seg_nb=nb, P=int(info.P), bstart=bstart, split_n=int(info.split_n), split_cap=int(info.split_cap),
                   split=split[:ns], BWD_SMALL=int(info.bwd_small), BWD_MID=int(info.bwd_mid), HOT_SPLIT=int(info.hot_split),
                   HOT_SPLIT_MIN=int(info.hot_split_min))
        for k in caps:
            d = desc[k][:nb]
            out[k] = dict(desc=d, cap=caps[k],
                          buckets=[ent[k][int(o):int(o) + int(c)].copy() if int(o) + int(c) <= caps[k] else None for c, o in d])
        return out

    def forward(self, V_dim, d_rows):
        _ck(lib().dfh_batch_forward(self.h, V_dim, _dp(d_rows)))

    def backward(self, V_dim, d_rows, d_grads):
        _ck(lib().dfh_batch_backward(self.h, V_dim, _dp(d_rows), _dp(d_grads)))

    def key_ranges(self, nparts):
        """bounds[nparts+1]: shard d owns feaids[bounds[d]:bounds[d+1]] (key-range partition)"""
        out = np.zeros(nparts + 1, np.uint32)
        _ck(lib().dfh_batch_key_ranges(self.h, nparts, _p(out)))
        return out

    def device_keys(self):
        a, b, u = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        _ck(lib().dfh_batch_device_keys(self.h, C.byref(a), C.byref(b), C.byref(u)))
        return a.value, b.value, u.value

    def device_key_ptrs(self):
        """device pointers of feaids / feacnt without synchronising (U comes from key_ranges_device)"""
        a, b = C.c_void_p(), C.c_void_p()
        _ck(lib().dfh_batch_device_keys(self.h, C.byref(a), C.byref(b), None))
        return a.value, b.value

    def key_ranges_device(self, nparts, d_bounds, d_splits=None):
        _ck(lib().dfh_batch_key_ranges_device(self.h, nparts, _dp(d_splits), _dp(d_bounds)))


class DeviceBuffer:
    """raw device memory owned through the C ABI (dfh_malloc)"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = C.c_void_p()
        _ck(lib().dfh_malloc(ctx.h, nbytes, C.byref(self.ptr)))

    @classmethod
    def from_numpy(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, max(arr.nbytes, 16))
        if arr.nbytes:
            _ck(lib().dfh_memcpy_h2d(ctx.h, b.ptr, _p(arr), arr.nbytes))
        return b

    def to_numpy(self, dtype, count):
        out = np.zeros(count, dtype)
        if out.nbytes:
            _ck(lib().dfh_memcpy_d2h(self.ctx.h, _p(out), self.ptr, out.nbytes))
        return out

    def at(self, byte_offset):
        return C.c_void_p(self.ptr.value + byte_offset)

    def close(self):
        if self.ptr:
            lib().dfh_free(self.ctx.h, self.ptr)
            self.ptr = None


def _ptrs(ptrs):
    """a host array of device pointers (DeviceBuffer, int, c_void_p or torch tensors)"""
    arr = (C.c_void_p * max(len(ptrs), 1))()
    for i, x in enumerate(ptrs):
        arr[i] = (x.ptr if isinstance(x, DeviceBuffer) else _dp(x)).value
    return arr


def vec_inner_multi(ctx, n, a, b):
    """[len(a) x len(b)] inner products of device vectors (fp32 products summed in fp64)"""
    out = np.zeros(len(a) * len(b), np.float64)
    _ck(lib().dfh_vec_inner_multi(ctx.h, n, len(a), _ptrs(a), len(b), _ptrs(b), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out.reshape(len(a), len(b))


def vec_combine(ctx, n, vecs, coef, out, dot=None, clamp=5.0):
    """out = clamp(sum of lbfgs::Add(coef[k], vecs[k]) in order); returns <dot, out> (None without dot)"""
    c = np.ascontiguousarray(coef, np.float32)
    d = C.c_double(0)
    _ck(lib().dfh_vec_combine(ctx.h, n, len(vecs), _ptrs(vecs), _p(c), clamp, _ptrs([out])[0],
                              _ptrs([dot])[0] if dot is not None else None, C.byref(d)))
    return d.value if dot is not None else None


def vec_line_step(ctx, n, w, p, x, vmask=None, l2=0.0, V_l2=0.0):
    """w += x p (lbfgs::Add); returns (r(w), <grad r(w), p>, nnz(w))"""
    out = np.zeros(3, np.float64)
    _ck(lib().dfh_vec_line_step(ctx.h, n, _ptrs([w])[0], _ptrs([p])[0] if p is not None else None, x,
                                _ptrs([vmask])[0] if vmask is not None else None, l2, V_l2,
                                out.ctypes.data_as(C.POINTER(C.c_double))))
    return tuple(out)


class Lbfgs:
    """the full-batch L-BFGS state resident in HBM (dfh_lbfgs): data chunks, model, gradients, s / y history"""

    def __init__(self, ctx, V_dim, m, comm=None):
        """comm (a Comm): the sharded object of dfh_lbfgs_create_sharded; every call is then collective and shape / model
        calls see this rank's slice of the keys"""
        self.ctx, self.V_dim, self.m, self.comm = ctx, V_dim, m, comm
        self.h = C.c_void_p()
        if comm is None:
            _ck(lib().dfh_lbfgs_create(ctx.h, V_dim, m, C.byref(self.h)))
        else:
            _ck(lib().dfh_lbfgs_create_sharded(ctx.h, comm.h, V_dim, m, C.byref(self.h)))

    def add_chunk(self, offset, index, value, label, is_val=False):
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint64)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        label = np.ascontiguousarray(label, np.float32)
        _ck(lib().dfh_lbfgs_add_chunk(self.h, int(is_val), len(offset) - 1, _p(offset), _p(index), _p(value), _p(label)))

    def init_model(self, tail_feature_filter=0, V_threshold=0, V_init_scale=0.01, l2=0.0, V_l2=0.0):
        k, n = C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_lbfgs_init_model(self.h, tail_feature_filter, V_threshold, V_init_scale, l2, V_l2, C.byref(k), C.byref(n)))
        self.nkeys, self.n = k.value, n.value
        return self.nkeys, self.n

    def get_model(self):
        keys = np.zeros(max(self.nkeys, 1), np.uint64)
        lens = np.zeros(max(self.nkeys, 1), np.int32)
        cnt = np.zeros(max(self.nkeys, 1), np.float32)
        w = np.zeros(max(self.n, 1), np.float32)
        _ck(lib().dfh_lbfgs_get_model(self.h, _p(keys), _p(lens), _p(cnt), _p(w)))
        return dict(keys=keys[:self.nkeys], lens=lens[:self.nkeys], cnt=cnt[:self.nkeys], w=w[:self.n])

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float32)
        _ck(lib().dfh_lbfgs_set_weights(self.h, _p(w)))

    def owned_range(self):
        """-> [key_lo, key_hi) of this rank's keys (key_hi = 0: no upper bound)"""
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_lbfgs_owned_range(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def set_model(self, keys, lens, vals):
        """start from a model given by key (unique keys in any order, lens in {1, 1 + V_dim}, vals ragged: w then V);
        -> the number of input keys that are keys of the model (summed over ranks on a sharded object)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        lens = np.ascontiguousarray(lens, np.int32)
        vals = np.ascontiguousarray(vals, np.float32)
        assert len(lens) == len(keys) and len(vals) == int(lens.sum())
        m = C.c_uint64(0)
        _ck(lib().dfh_lbfgs_set_model(self.h, len(keys), _p(keys), _p(lens), _p(vals), C.byref(m)))
        return m.value

    def calc_grad(self, gamma=1.0):
        loss, auc = C.c_float(0), C.c_float(0)
        _ck(lib().dfh_lbfgs_calc_grad(self.h, gamma, C.byref(loss), C.byref(auc)))
        return loss.value, auc.value

    def prepare_direction(self):
        """-> incr_B [6 mcur + 1] (float32), or None at the first epoch"""
        incr = np.zeros(6 * self.m + 1, np.float32)
        mc = C.c_int(0)
        _ck(lib().dfh_lbfgs_prepare_direction(self.h, _p(incr), C.byref(mc)))
        return incr[:6 * mc.value + 1] if mc.value else None

    def calc_direction(self, coef=None):
        pg = C.c_float(0)
        c = None if coef is None else np.ascontiguousarray(coef, np.float32)
        _ck(lib().dfh_lbfgs_calc_direction(self.h, _p(c), C.byref(pg)))
        return pg.value

    def line_search(self, alpha, gamma=1.0):
        """-> (f(w + alpha p), <grad f, p>, AUC x n)"""
        f, pg, auc = C.c_float(0), C.c_float(0), C.c_float(0)
        _ck(lib().dfh_lbfgs_line_search(self.h, alpha, gamma, C.byref(f), C.byref(pg), C.byref(auc)))
        return f.value, pg.value, auc.value

    def evaluate(self, val=False):
        """-> (validation AUC x n or None, nnz(w), r(w))"""
        va, nnz, r = C.c_float(0), C.c_float(0), C.c_float(0)
        _ck(lib().dfh_lbfgs_evaluate(self.h, C.byref(va) if val else None, C.byref(nnz), C.byref(r)))
        return (va.value if val else None), nnz.value, r.value

    def vector(self, which, i=0):
        """-> a copy of g_new (which = 0), g (1), s (2) or y (3) [n]; i: logical history index of s / y, oldest first"""
        out = np.zeros(max(self.n, 1), np.float32)
        _ck(lib().dfh_lbfgs_get_vector(self.h, int(which), int(i), _p(out)))
        return out[:self.n]

    def set_l1(self, l1):
        """l1 on w (OWL-QN), after init_model and before the first calc_grad; 0 changes nothing"""
        _ck(lib().dfh_lbfgs_set_l1(self.h, l1))

    def owlqn_vector(self, which):
        """-> a copy of the pseudo-gradient (which = 0) or of the line search's origin w0 (1) [n]"""
        out = np.zeros(max(self.n, 1), np.float32)
        _ck(lib().dfh_lbfgs_get_owlqn_vector(self.h, int(which), _p(out)))
        return out[:self.n]

    def drop_last_pair(self):
        """between prepare_direction and calc_direction: drop the newest (s, y) pair"""
        _ck(lib().dfh_lbfgs_drop_last_pair(self.h))

    def owlqn_moved(self):
        """-> elements the last line_search trial moved off w0"""
        v = C.c_double(0)
        _ck(lib().dfh_lbfgs_get_owlqn_moved(self.h, C.byref(v)))
        return v.value

    def close(self):
        if self.h:
            lib().dfh_lbfgs_destroy(self.h)
            self.h = None


class Bcd:
    """the block coordinate descent state resident in HBM (dfh_bcd): data chunks with their per-block layouts,
    predictions, and the model w / delta / delta w"""

    def __init__(self, ctx, comm=None):
        """comm (a Comm): the sharded object of dfh_bcd_create_sharded; every call is then collective, the chunks are this
        rank's rows and the model is the whole, replicated model"""
        self.ctx, self.comm = ctx, comm
        self.h = C.c_void_p()
        self.nkeys = 0
        if comm is None:
            _ck(lib().dfh_bcd_create(ctx.h, C.byref(self.h)))
        else:
            _ck(lib().dfh_bcd_create_sharded(ctx.h, comm.h, C.byref(self.h)))

    def add_chunk(self, offset, index, value, label, is_val=False):
        offset = np.ascontiguousarray(offset, np.uint64)
        index = np.ascontiguousarray(index, np.uint64)
        value = None if value is None else np.ascontiguousarray(value, np.float32)
        label = np.ascontiguousarray(label, np.float32)
        _ck(lib().dfh_bcd_add_chunk(self.h, int(is_val), len(offset) - 1, _p(offset), _p(index), _p(value), _p(label)))

    def build(self, ranges, tail_feature_filter=0, l1=1.0, lr=0.9):
        """ranges: [(begin, end)] of ReverseBytes keys, sorted and disjoint (PartitionFeature); -> number of keys"""
        beg = np.ascontiguousarray([r[0] for r in ranges], np.uint64)
        end = np.ascontiguousarray([r[1] for r in ranges], np.uint64)
        k = C.c_uint64(0)
        _ck(lib().dfh_bcd_build(self.h, tail_feature_filter, len(ranges), _p(beg), _p(end), l1, lr, C.byref(k)))
        self.nkeys = k.value
        self.nblk = len(ranges)
        return self.nkeys

    def block_info(self, blk):
        """-> (model positions [begin, end), training entries, touched rows)"""
        b, e, z, r = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_bcd_block_info(self.h, blk, C.byref(b), C.byref(e), C.byref(z), C.byref(r)))
        return b.value, e.value, z.value, r.value

    def epoch(self, order):
        """-> progress {count, objv, AUC x n, accuracy} as float32 [4]"""
        order = np.ascontiguousarray(order, np.int32)
        prog = np.zeros(4, np.float32)
        _ck(lib().dfh_bcd_epoch(self.h, _p(order), len(order), _p(prog)))
        return prog

    def step(self, blk, grad=False, progress=False):
        """one block; -> (g, h) in fp64 before the update when grad, and the progress [4] when progress"""
        b, e, _, _ = self.block_info(blk)
        g = np.zeros(max(e - b, 1), np.float64) if grad else None
        h = np.zeros(max(e - b, 1), np.float64) if grad else None
        prog = np.zeros(4, np.float32) if progress else None
        _ck(lib().dfh_bcd_step(self.h, blk, _p(g), _p(h), _p(prog)))
        return (g[:e - b] if grad else None), (h[:e - b] if grad else None), prog

    def set_model(self, keys, w):
        """start from a model (unique ReverseBytes keys in any order); the predictions of every chunk are rebuilt;
        -> the number of input keys that are keys of the model"""
        keys = np.ascontiguousarray(keys, np.uint64)
        w = np.ascontiguousarray(w, np.float32)
        assert len(keys) == len(w)
        m = C.c_uint64(0)
        _ck(lib().dfh_bcd_set_model(self.h, len(keys), _p(keys), _p(w), C.byref(m)))
        return m.value

    def get_model(self):
        n = max(self.nkeys, 1)
        keys, cnt = np.zeros(n, np.uint64), np.zeros(n, np.float32)
        w, delta, dw = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        _ck(lib().dfh_bcd_get_model(self.h, _p(keys), _p(cnt), _p(w), _p(delta), _p(dw)))
        k = self.nkeys
        return dict(keys=keys[:k], cnt=cnt[:k], w=w[:k], delta=delta[:k], dw=dw[:k])

    def get_pred(self, chunk=0, is_val=False):
        n = C.c_size_t(0)
        _ck(lib().dfh_bcd_get_pred(self.h, int(is_val), chunk, None, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _ck(lib().dfh_bcd_get_pred(self.h, int(is_val), chunk, _p(out), None))
        return out

    def close(self):
        if self.h:
            lib().dfh_bcd_destroy(self.h)
            self.h = None


def row_stride(V_dim):
    return int(lib().dfh_row_stride(V_dim))


def multi_words(n, nsrc):
    """32-bit words of the row-word buffer dfh_shard_resolve_multi fills for n entries of nsrc sources"""
    return int(lib().dfh_shard_multi_words(n, nsrc))


class Comm:
    """dfh_comm: the transport of the sharded store — RCCL (product) or a host callback (tests)"""

    def __init__(self, handle, keep=None):
        self.h, self._keep = handle, keep

    @staticmethod
    def unique_id():
        buf = (C.c_char * COMM_ID_BYTES)()
        _ck(lib().dfh_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    @classmethod
    def rccl(cls, ctx, rank, world, unique_id):
        h = C.c_void_p()
        buf = C.create_string_buffer(unique_id, COMM_ID_BYTES)
        _ck(lib().dfh_comm_create_rccl(ctx.h, rank, world, C.cast(buf, C.c_void_p), C.byref(h)))
        return cls(h)

    @classmethod
    def callback(cls, ctx, rank, world, fn):
        """fn(send: np.uint8[...], send_bytes: list, recv: np.uint8[...] (to fill), recv_bytes: list)"""
        def tramp(_user, p_send, p_sb, p_recv, p_rb):
            try:
                sb = [int(p_sb[i]) for i in range(world)]
                rb = [int(p_rb[i]) for i in range(world)]
                send = np.ctypeslib.as_array(C.cast(p_send, C.POINTER(C.c_uint8)), shape=(max(sum(sb), 1),))[:sum(sb)]
                recv = np.ctypeslib.as_array(C.cast(p_recv, C.POINTER(C.c_uint8)), shape=(max(sum(rb), 1),))[:sum(rb)]
                fn(send, sb, recv, rb)
                return 0
            except Exception:  # noqa: BLE001 - reported through the C return code
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLTOALLV_FN(tramp)
        h = C.c_void_p()
        _ck(lib().dfh_comm_create_callback(ctx.h, rank, world, cb, None, C.byref(h)))
        return cls(h, keep=cb)

    @classmethod
    def loopback(cls, ctx, rank, world):
        """measurement only: rank `rank` of a `world`-rank job alone on its GPU; the peers' messages are device copies
        out of buffers fed with feed() (include/difacto_hip.h, dfh_comm_create_loopback)"""
        h = C.c_void_p()
        _ck(lib().dfh_comm_create_loopback(ctx.h, rank, world, C.byref(h)))
        return cls(h)

    def feed(self, kind, d_src, sticky=False):
        """source (device pointer) of the next exchange of `kind` (XCHG_*), laid out like its receive side"""
        _ck(lib().dfh_comm_loopback_feed(self.h, kind, d_src, 1 if sticky else 0))

    def wire(self, link_gbps, latency_us):
        _ck(lib().dfh_comm_loopback_wire(self.h, float(link_gbps), float(latency_us)))

    def wire_time_us(self, reset=True):
        v = C.c_double(0)
        _ck(lib().dfh_comm_loopback_wire_time(self.h, 1 if reset else 0, C.byref(v)))
        return v.value

    def allreduce_sum(self, vals):
        a = np.ascontiguousarray(vals, np.float64).copy()
        _ck(lib().dfh_comm_allreduce_sum(self.h, _p(a), len(a)))
        return a

    def allgather(self, arr):
        """every rank's array (same dtype and length on every rank) -> [world, len]"""
        a = np.ascontiguousarray(arr)
        out = np.zeros((lib().dfh_comm_world(self.h),) + a.shape, a.dtype)
        _ck(lib().dfh_comm_allgather(self.h, _p(a), a.nbytes, _p(out)))
        return out

    def stats(self, reset=False):
        """(bytes sent to other ranks, bytes received from them, message groups) since the last reset"""
        a, b, g = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_comm_stats(self.h, 1 if reset else 0, C.byref(a), C.byref(b), C.byref(g)))
        return a.value, b.value, g.value

    def info(self):
        """the bound transport: RCCL version + the file it was bound from, or the host callback"""
        buf = C.create_string_buffer(512)
        _ck(lib().dfh_comm_info(self.h, buf, 512))
        return buf.value.decode()

    def wire_probe(self, bytes_per_peer, reps=20):
        """microseconds per grouped exchange in which every rank sends bytes_per_peer to (and receives as much from) every
        other rank; COLLECTIVE"""
        us = C.c_double(0)
        _ck(lib().dfh_comm_wire_probe(self.h, int(bytes_per_peer), int(reps), C.byref(us)))
        return us.value

    def selfcheck(self, timeout_s=60.0):
        """collective start-up check (first exchange polled with a timeout): raises instead of hanging"""
        _ck(lib().dfh_comm_selfcheck(self.h, float(timeout_s)))

    def balanced_splits(self, sample_keys):
        """collective: split keys (world-1, identical on every rank) at the quantiles of the union of the ranks' key samples"""
        k = np.ascontiguousarray(sample_keys, np.uint64)
        w = lib().dfh_comm_world(self.h)
        out = np.zeros(max(w - 1, 1), np.uint64)
        _ck(lib().dfh_shard_balanced_splits(self.h, _p(k) if len(k) else None, len(k), _p(out)))
        return out[:w - 1]

    def close(self):
        if self.h:
            lib().dfh_comm_destroy(self.h)
            self.h = None


class Shard:
    """dfh_shard: this rank's part of the key-range-sharded model + the per-step exchange"""

    def __init__(self, table, comm, splits=None):
        self.h = C.c_void_p()
        self.table, self.comm = table, comm
        self.splits = None if splits is None else np.ascontiguousarray(splits, np.uint64)
        _ck(lib().dfh_shard_create(table.h, comm.h, _p(self.splits), C.byref(self.h)))

    def step(self, batch, is_train=True, push_cnt=False):
        """collective; batch = None when this rank's data is exhausted.  -> True while any rank had a minibatch"""
        act = C.c_int(0)
        _ck(lib().dfh_shard_step(self.h, batch.h if batch is not None else None, 1 if is_train else 0, 1 if push_cnt else 0,
                                 C.byref(act)))
        return bool(act.value)

    def prefetch_counts(self, next_batch):
        """collective, right before step(): the minibatch of the FOLLOWING step (localize queued) or None"""
        _ck(lib().dfh_shard_prefetch_counts(self.h, next_batch.h if next_batch is not None else None))

    def pull_host(self, keys):
        """collective literal Store::Pull(kWeight) -> (vals ragged, lens)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        n, k = len(keys), self.table.V_dim
        vals = np.zeros(max(n * (1 + k), 1), np.float32)
        lens = np.zeros(max(n, 1), np.int32)
        nv, nl = C.c_size_t(0), C.c_size_t(0)
        _ck(lib().dfh_shard_pull_host(self.h, _p(keys) if n else None, n, _p(vals), C.byref(nv), _p(lens), C.byref(nl)))
        return vals[:nv.value], lens[:nl.value]

    def push_host(self, keys, val_type, vals, lens=None):
        """collective literal Store::Push(kFeaCount | kGradient)"""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.float32)
        lens = np.zeros(0, np.int32) if lens is None else np.ascontiguousarray(lens, np.int32)
        _ck(lib().dfh_shard_push_host(self.h, _p(keys) if len(keys) else None, len(keys), val_type, _p(vals) if len(vals) else None,
                                      len(vals), _p(lens) if len(lens) else None, len(lens)))

    def set_exchange(self, mode):
        """"sync" (one minibatch at a time, zero staleness) or "overlap" (two in flight, staleness <= 1); between epochs"""
        _ck(lib().dfh_shard_set_exchange(self.h, {"sync": 0, "overlap": 1}[mode]))

    def reserve(self, batch_keys, recv_keys):
        """exchange buffers for these sizes now, so that no step re-allocates (after set_exchange)"""
        _ck(lib().dfh_shard_reserve(self.h, int(batch_keys), int(recv_keys)))

    def set_timing(self, on):
        _ck(lib().dfh_shard_set_timing(self.h, 1 if on else 0))

    def get_timing(self, reset=True):
        """-> ({stage: ms}, steps covered)"""
        ms = np.zeros(len(SHARD_STAGES), np.float64)
        n = C.c_uint64(0)
        _ck(lib().dfh_shard_get_timing(self.h, 1 if reset else 0, _p(ms), C.byref(n)))
        return dict(zip(SHARD_STAGES, ms.tolist())), n.value

    def owned_range(self):
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        _ck(lib().dfh_shard_owned_range(self.h, _p(self.splits), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def close(self):
        if self.h:
            lib().dfh_shard_destroy(self.h)
            self.h = None
