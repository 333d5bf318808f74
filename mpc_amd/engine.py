"""ctypes binding of the C ABI (include/gcengine.h -> mpc_amd/csrc/libgcengine.so).

This is the same boundary the Go shim binds through cgo; the tests and bench.py
drive the product exclusively through it.  There is no CPU fallback: if the HIP library is
missing or no GPU is present, the calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .circuit import GATE, LABEL, WIRE

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("GC_LIB") or os.path.join(CSRC, "libgcengine.so")  # GC_LIB: developer builds
HEADER = os.path.join(os.path.dirname(HERE), "include", "gcengine.h")

ABI_VERSION = 2  # GC_ABI_VERSION of include/gcengine.h
GC_OK, GC_E_KEYSIZE, GC_E_RAND, GC_E_GATE, GC_E_ROWS, GC_E_ARG, GC_E_HIP, GC_E_NOMEM, GC_E_WIRE, GC_E_POINT = (
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9)
GC_E_BUSY = -10  # gc_stream_batch_out_garble: no free window


class EngineError(RuntimeError):
    """Carries the C-ABI status; str() follows the reference's error text where one exists."""

    def __init__(self, code, what=""):
        self.code = code
        msg = lib().gc_strerror(code).decode() if _lib is not None else "status %d" % code
        detail = lib().gc_last_error().decode() if _lib is not None and code in (GC_E_HIP, GC_E_NOMEM) else ""
        super().__init__("%s%s%s" % (what + ": " if what else "", msg, " [" + detail + "]" if detail else ""))


def build(force=False):
    """Compile libgcengine.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", CSRC, "-j8"]
    if force:
        subprocess.check_call(cmd + ["clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


class PlanInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "ngates", "nwires", "ninputs", "noutputs", "nlevels", "max_width", "slab_rows", "n_xor", "n_xnor", "n_and",
        "n_or", "n_inv", "nslots", "n_steps", "n_hash_phases", "n_fused_steps", "n_lds_slots", "n_flat_slots",
        "n_flat_outs", "n_flat_terms", "n_flat_steps", "n_flat_units")]


class GmwInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "ngates", "nwires", "ninputs", "noutputs", "nlevels", "n_and_levels", "triple_words", "max_level_words", "n_xor",
        "n_xnor", "n_and", "n_inv", "max_free_depth")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is the product; there is no CPU fallback)" % LIB_PATH)
    # A streaming host wants 8 hardware queues (the HIP runtime's default is 4: streams that share one run one after the other;
    # mpc_amd/csrc/engine.cpp).  The HOST decides that, before its first HIP call — this binding is the host of the test-suite
    # and of bench.py; the library itself never touches the environment.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    L = C.CDLL(LIB_PATH)
    vp, u32, sz, i32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_int
    ip = C.POINTER(C.c_int)
    sigs = {
        "gc_strerror": (C.c_char_p, [i32]),
        "gc_last_error": (C.c_char_p, []),
        "gc_abi_version": (i32, []),
        "gc_plan_create": (vp, [vp, u32, u32, u32, u32, ip]),
        "gc_plan_create_chain": (vp, [vp, vp, vp, vp, vp, vp, u32, ip]),
        "gc_plan_free": (None, [vp]),
        "gc_plan_get_info": (i32, [vp, C.POINTER(PlanInfo)]),
        "gc_plan_simulate": (i32, [vp, vp, vp]),
        "gc_plan_describe": (i32, [vp, vp, vp, vp, vp]),
        "gc_plan_fingerprint": (i32, [vp, vp]),
        "gc_plan_flat_geometry": (i32, [vp, vp, vp]),
        "gc_device_count": (i32, []),
        "gc_ctx_create": (vp, [i32, ip]),
        "gc_ctx_destroy": (None, [vp]),
        "gc_ctx_sync": (i32, [vp]),
        "gc_ctx_stream": (vp, [vp]),
        "gc_circ_load": (vp, [vp, vp, u32, u32, u32, u32, ip]),
        "gc_circ_free": (None, [vp]),
        "gc_circ_plan": (vp, [vp]),
        "gc_circ_set_schedule": (i32, [vp, i32]),
        "gc_garble": (i32, [vp, vp, sz, vp, sz, u32, vp, vp, vp, vp]),
        "gc_eval": (i32, [vp, vp, sz, u32, vp, vp, vp, sz, vp]),
        "gc_garble_labels": (i32, [vp, vp, sz, vp, vp, vp, vp]),
        "gc_stream_create": (vp, [vp, vp, sz, vp, sz, vp, u32, ip]),
        "gc_stream_free": (None, [vp]),
        "gc_stream_get_wire": (i32, [vp, u32, vp]),
        "gc_stream_garble": (i32, [vp, vp, u32, u32, vp, u32, vp, u32, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_stream_garble_begin": (i32, [vp, vp, u32, u32, vp, u32, vp, u32]),
        "gc_stream_garble_finish": (i32, [vp, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_stream_garble_flush": (i32, [vp]),
        "gc_stream_intern": (i32, [vp, vp, u32, u32, u32, u32, C.POINTER(C.c_uint32)]),
        "gc_stream_garble_begin_h": (i32, [vp, u32, vp, vp]),
        "gc_stream_release": (i32, [vp, u32]),
        "gc_stream_garble_finish_view": (i32, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
        "gc_stream_garble_finish_async": (i32, [vp, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_stream_garble_copies_wait": (i32, [vp]),
        "gc_stream_stats": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "gc_stream_deep_stats": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "gc_stream_fuse_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_stream_eval_fuse_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_stream_wait_stats": (i32, [vp, C.POINTER(C.c_uint64)]),
        "gc_stream_eval_wait_stats": (i32, [vp, C.POINTER(C.c_uint64)]),
        "gc_stream_eval_dev_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 2),
        "gc_ctx_coop_stats": (i32, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
        "gc_ctx_pci_bus_id": (i32, [vp, C.c_char_p, sz]),
        "gc_stream_eval_deep_stats": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "gc_stream_eval_create": (vp, [vp, vp, sz, ip]),
        "gc_stream_eval_free": (None, [vp]),
        "gc_stream_eval_set_wire": (i32, [vp, u32, vp]),
        "gc_stream_eval_get_wire": (i32, [vp, u32, vp]),
        "gc_stream_eval_circuit": (i32, [vp, u32, u32, u32, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_stream_eval_blocks": (i32, [vp, vp, sz, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
        "gc_stream_eval_stats": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "gc_stream_batch_create": (vp, [vp, u32, vp, sz, vp, vp, u32, ip]),
        "gc_stream_batch_free": (None, [vp]),
        "gc_stream_batch_step_bytes": (sz, [vp, u32, u32, vp, u32, vp, u32]),
        "gc_stream_batch_garble": (i32, [vp, vp, u32, u32, vp, u32, vp, u32, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_stream_batch_get_wire": (i32, [vp, u32, vp]),
        "gc_stream_batch_gather_wires": (i32, [vp, vp, u32, vp]),
        "gc_stream_batch_cache_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_stream_eval_batch_cache_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_stream_eval_batch_create": (vp, [vp, u32, vp, sz, ip]),
        "gc_stream_eval_batch_free": (None, [vp]),
        "gc_stream_eval_batch_set_wires": (i32, [vp, vp, u32, vp]),
        "gc_stream_eval_batch_get_wire": (i32, [vp, u32, vp]),
        "gc_stream_eval_batch_circuit": (i32, [vp, u32, u32, u32, vp, sz, vp, sz, vp, C.POINTER(C.c_size_t)]),
        "gc_stream_batch_select_labels_dev": (i32, [vp, vp, u32, vp, vp]),
        "gc_stream_batch_decode_dev": (i32, [vp, vp, u32, vp, vp, vp]),
        "gc_stream_batch_select_labels": (i32, [vp, vp, u32, vp, vp]),
        "gc_stream_batch_decode": (i32, [vp, vp, u32, vp, vp, vp]),
        "gc_stream_batch_out_create": (vp, [vp, sz, u32, ip]),
        "gc_stream_batch_out_free": (None, [vp]),
        "gc_stream_batch_out_garble": (i32, [vp, vp, sz, vp, u32, u32, vp, u32, vp, u32, C.POINTER(C.c_size_t)]),
        "gc_stream_batch_out_flush": (i32, [vp]),
        "gc_stream_batch_out_next": (i32, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "gc_stream_batch_out_release": (i32, [vp]),
        "gc_stream_batch_out_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_stream_batch_out_create_split": (vp, [vp, sz, u32, ip]),
        "gc_stream_batch_out_split_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 2),
        "gc_stream_batch_set_fallback": (i32, [vp, i32]),
        "gc_stream_eval_batch_set_fallback": (i32, [vp, i32]),
        "gc_stream_eval_batch_circuit_host": (i32, [vp, u32, u32, u32, vp, sz, sz, u32, C.POINTER(C.c_size_t)]),
        "gc_stream_eval_batch_uploads_wait": (i32, [vp]),
        "gc_stream_eval_batch_bad": (i32, [vp, vp]),
        "gc_stream_eval_batch_return_labels_dev": (i32, [vp, vp, u32, vp]),
        "gc_stream_eval_batch_return_labels": (i32, [vp, vp, u32, vp]),
        "gc_stream_eval_batch_in_create": (vp, [vp, u32, sz, ip]),
        "gc_stream_eval_batch_in_free": (None, [vp]),
        "gc_stream_eval_batch_in_feed": (i32, [vp, vp, sz, sz, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
        "gc_stream_eval_batch_in_stats": (i32, [vp] + [C.POINTER(C.c_uint64)] * 4),
        "gc_batch_create": (vp, [vp, u32, ip]),
        "gc_batch_free": (None, [vp]),
        "gc_ctx_capture_begin": (i32, [vp]),
        "gc_ctx_capture_end": (i32, [vp, C.POINTER(vp)]),
        "gc_graph_launch": (i32, [vp]),
        "gc_graph_free": (None, [vp]),
        "gc_batch_stride": (u32, [vp]),
        "gc_batch_tile_instances": (u32, [vp]),
        "gc_batch_wires_in_lds": (i32, [vp]),
        "gc_batch_set_schedule": (i32, [vp, i32]),
        "gc_batch_set_graph": (i32, [vp, i32]),
        "gc_batch_set_store_all": (i32, [vp, i32]),
        "gc_batch_garble": (i32, [vp, vp, sz, vp]),
        "gc_batch_select_inputs": (i32, [vp, vp, vp]),
        "gc_batch_set_inputs": (i32, [vp, vp]),
        "gc_batch_eval": (i32, [vp, vp, sz, vp]),
        "gc_batch_decode": (i32, [vp, vp, vp, vp]),
        "gc_batch_garble_keyed": (i32, [vp, vp, sz, vp]),
        "gc_batch_eval_keyed": (i32, [vp, vp, sz, vp]),
        "gc_batch_keyed_supported": (i32, [vp]),
        "gc_batch_keyed_path": (i32, [vp]),
        "gc_batch_set_keyed_path": (i32, [vp, i32]),
        "gc_batch_set_keyed_hbm_form": (i32, [vp, i32]),
        "gc_batch_keyed_hbm_form": (i32, [vp]),
        "gc_batch_debug_keyed_hbm_hash_waves": (i32, [vp, u32, u32]),
        "gc_batch_debug_keyed_schedule": (i32, [vp, vp, sz, vp, vp]),
        "gc_batch_read_r": (i32, [vp, vp]),
        "gc_batch_read_slab": (i32, [vp, vp]),
        "gc_batch_read_wires": (i32, [vp, vp]),
        "gc_batch_read_labels": (i32, [vp, vp]),
        "gc_batch_read_outputs": (i32, [vp, vp]),
        "gc_batch_write_slab": (i32, [vp, vp]),
        "gc_batch_dev_wires": (vp, [vp]),
        "gc_batch_dev_slab": (vp, [vp]),
        "gc_batch_dev_r": (vp, [vp]),
        "gc_batch_gather_outputs": (i32, [vp, vp]),
        "gc_tables_wire_bytes": (sz, [vp]),
        "gc_batch_egress_tables": (i32, [vp, vp, sz]),
        "gc_batch_ingest_tables": (i32, [vp, vp, sz, vp]),
        "gc_batch_gather_input_wires": (i32, [vp, u32, u32, vp]),
        "gc_batch_set_input_range": (i32, [vp, u32, u32, vp]),
        "gc_cot_send_pads_dev": (i32, [vp, vp, vp, vp, vp, sz, vp]),
        "gc_cot_receive_unpad_dev": (i32, [vp, vp, vp, vp, vp, sz]),
        "gc_batch_egress_tables_dense": (i32, [vp, vp, sz]),
        "gc_batch_ingest_tables_dense": (i32, [vp, vp, sz]),
        "gc_batch_last_ms": (C.c_float, [vp]),
        "gc_batch_last_launches": (u32, [vp]),
        "gc_batch_debug_profile": (i32, [vp, i32, vp]),
        "gc_iknp_receiver_create": (vp, [vp, vp, ip]),
        "gc_iknp_sender_create": (vp, [vp, vp, vp, ip]),
        "gc_iknp_free": (None, [vp]),
        "gc_iknp_u_bytes": (sz, [sz]),
        "gc_iknp_receive": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_send": (i32, [vp, vp, sz, sz, vp]),
        "gc_iknp_receive_dev": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_send_dev": (i32, [vp, vp, sz, vp]),
        "gc_iknp_last_ms": (C.c_float, [vp]),
        "gc_iknp_receive_bits": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_send_bits": (i32, [vp, vp, sz, sz, vp]),
        "gc_iknp_receive_bits_dev": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_send_bits_dev": (i32, [vp, vp, sz, vp]),
        "gc_kos_receiver_tags": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]),
        "gc_kos_sender_check": (i32, [vp, vp, vp, sz, vp, vp, vp, vp, vp, ip]),
        "gc_kos_receiver_tags_dev": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]),
        "gc_kos_sender_check_dev": (i32, [vp, vp, vp, sz, vp, vp, vp, vp, vp, ip]),
        "gc_mitccrh_hash": (i32, [vp, vp, C.c_uint64, vp, sz, u32]),
        "gc_cot_send_pads": (i32, [vp, vp, vp, vp, vp, sz, vp]),
        "gc_cot_receive_unpad": (i32, [vp, vp, vp, vp, vp, sz]),
        "gc_rot_send": (i32, [vp, vp, vp, vp, sz, vp]),
        "gc_rot_receive": (i32, [vp, vp, vp, sz]),
        "gc_rot_send_dev": (i32, [vp, vp, vp, vp, sz, vp]),
        "gc_rot_receive_dev": (i32, [vp, vp, vp, sz]),
        "gc_garble_wire": (i32, [vp, vp, sz, vp, sz, u32, vp, vp, vp, sz]),
        "gc_eval_wire": (i32, [vp, vp, sz, u32, vp, vp, sz, vp, vp]),
        "gc_dev_alloc": (vp, [vp, sz, ip]),
        "gc_dev_free": (None, [vp, vp]),
        "gc_dev_upload": (i32, [vp, vp, vp, sz]),
        "gc_dev_download": (i32, [vp, vp, vp, sz]),
        "gc_dev_memset": (i32, [vp, vp, i32, sz]),
        "gc_dev_copy": (i32, [vp, vp, vp, sz]),
        "gc_host_alloc": (vp, [sz]),
        "gc_host_free": (None, [vp]),
        "gc_host_register": (i32, [vp, sz]),
        "gc_host_unregister": (i32, [vp]),
        "gc_host_is_pinned": (i32, [vp]),
        "gc_comm_available": (i32, []),
        "gc_comm_version": (i32, []),
        "gc_comm_get_unique_id": (i32, [vp, sz]),
        "gc_comm_init_rank": (vp, [vp, vp, sz, i32, i32, ip]),
        "gc_comm_init_all": (i32, [vp, i32, vp]),
        "gc_comm_destroy": (None, [vp]),
        "gc_comm_rank": (i32, [vp]),
        "gc_comm_nranks": (i32, [vp]),
        "gc_comm_allgather": (i32, [vp, vp, vp, sz]),
        "gc_comm_allgather_all": (i32, [vp, i32, vp, vp, sz]),
        "gc_comm_allreduce_max": (i32, [vp, C.POINTER(C.c_double)]),
        "gc_comm_barrier": (i32, [vp]),
        "gc_gmw_plan_describe": (i32, [vp, u32, u32, u32, u32, C.POINTER(GmwInfo), vp, vp, vp]),
        "gc_gmw_create": (vp, [vp, vp, u32, u32, u32, u32, u32, u32, u32, ip]),
        "gc_gmw_free": (None, [vp]),
        "gc_gmw_get_info": (i32, [vp, C.POINTER(GmwInfo)]),
        "gc_gmw_set_inputs": (i32, [vp, vp]),
        "gc_gmw_set_inputs_dev": (i32, [vp, vp]),
        "gc_gmw_set_triples": (i32, [vp, vp, vp, vp]),
        "gc_gmw_set_triples_dev": (i32, [vp, vp, vp, vp]),
        "gc_gmw_step": (i32, [vp, vp, u32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
        "gc_gmw_step_dev": (i32, [vp, vp, u32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
        "gc_gmw_get_outputs": (i32, [vp, vp]),
        "gc_gmw_get_outputs_dev": (i32, [vp, vp]),
        "gc_gmw_last_launches": (u32, [vp]),
        "gc_gmw_triples_local_dev": (i32, [vp, vp, vp, vp, sz]),
        "gc_gmw_triples_sender_u_dev": (i32, [vp, u32, vp, vp, sz]),
        "gc_gmw_triples_sender_fold_dev": (i32, [vp, vp, vp, vp, vp, sz]),
        "gc_gmw_triples_receiver_fold_dev": (i32, [vp, vp, vp, sz]),
        "gc_vole_sender_mul": (i32, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "gc_vole_sender_mul_dev": (i32, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "gc_vole_receiver_reduce": (i32, [vp, vp, vp, sz, vp]),
        "gc_vole_receiver_reduce_dev": (i32, [vp, vp, vp, sz, vp]),
        "gc_co_sender_setup": (i32, [vp, vp, vp]),
        "gc_co_sender_encrypt": (i32, [vp, vp, vp, vp, vp, sz, C.c_uint64, vp, C.POINTER(C.c_size_t)]),
        "gc_co_sender_encrypt_dev": (i32, [vp, vp, vp, vp, vp, sz, C.c_uint64, vp, vp]),
        "gc_co_receiver_choices": (i32, [vp, vp, vp, vp, sz, vp]),
        "gc_co_receiver_choices_dev": (i32, [vp, vp, vp, vp, sz, vp]),
        "gc_co_receiver_decrypt": (i32, [vp, vp, vp, vp, vp, sz, C.c_uint64, vp]),
        "gc_co_receiver_decrypt_dev": (i32, [vp, vp, vp, vp, vp, sz, C.c_uint64, vp]),
        "gc_co_base_create": (vp, [vp, vp, ip]),
        "gc_co_base_free": (None, [vp]),
        "gc_co_base_choices": (i32, [vp, vp, vp, sz, vp]),
        "gc_co_base_choices_dev": (i32, [vp, vp, vp, sz, vp]),
        "gc_co_base_decrypt": (i32, [vp, vp, vp, vp, sz, C.c_uint64, vp]),
        "gc_co_base_decrypt_dev": (i32, [vp, vp, vp, vp, sz, C.c_uint64, vp]),
        "gc_co_multi_sender_setup": (i32, [vp, vp, sz, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_co_multi_sender_setup_dev": (i32, [vp, vp, sz, vp, vp, vp]),
        "gc_co_multi_sender_encrypt": (i32, [vp, vp, vp, vp, vp, sz, sz, C.c_uint64, vp, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t)]),
        "gc_co_multi_sender_encrypt_dev": (i32, [vp, vp, vp, vp, vp, sz, sz, C.c_uint64, vp, vp]),
        "gc_co_multi_receiver_choices": (i32, [vp, vp, vp, vp, sz, sz, vp, C.POINTER(C.c_size_t)]),
        "gc_co_multi_receiver_choices_dev": (i32, [vp, vp, vp, vp, sz, sz, vp, vp]),
        "gc_co_multi_receiver_decrypt": (i32, [vp, vp, vp, vp, vp, sz, sz, C.c_uint64, vp, C.POINTER(C.c_size_t)]),
        "gc_co_multi_receiver_decrypt_dev": (i32, [vp, vp, vp, vp, vp, sz, sz, C.c_uint64, vp, vp]),
        "gc_co_multi_base_create": (vp, [vp, vp, sz, ip]),
        "gc_co_multi_base_create_dev": (vp, [vp, vp, sz, ip]),
        "gc_co_multi_base_free": (None, [vp]),
        "gc_co_multi_base_info": (i32, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "gc_co_multi_base_decrypt": (i32, [vp, vp, vp, vp, sz, C.c_uint64, vp, C.POINTER(C.c_size_t)]),
        "gc_co_multi_base_decrypt_dev": (i32, [vp, vp, vp, vp, sz, C.c_uint64, vp, vp]),
        "gc_iknp_multi_sender_create": (vp, [vp, vp, vp, sz, ip]),
        "gc_iknp_multi_sender_create_dev": (vp, [vp, vp, vp, sz, ip]),
        "gc_iknp_multi_receiver_create": (vp, [vp, vp, sz, ip]),
        "gc_iknp_multi_receiver_create_dev": (vp, [vp, vp, sz, ip]),
        "gc_iknp_multi_free": (None, [vp]),
        "gc_iknp_multi_info": (i32, [vp, C.POINTER(C.c_size_t), ip, C.POINTER(C.c_uint64)]),
        "gc_iknp_multi_receive": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_multi_send": (i32, [vp, vp, sz, sz, vp]),
        "gc_iknp_multi_receive_dev": (i32, [vp, vp, sz, vp, vp]),
        "gc_iknp_multi_send_dev": (i32, [vp, vp, sz, vp]),
        "gc_iknp_multi_receive_bits_dev": (i32, [vp, vp, sz, sz, vp, vp]),
        "gc_iknp_multi_send_bits_dev": (i32, [vp, vp, sz, vp]),
        "gc_iknp_multi_receive_bits": (i32, [vp, vp, sz, sz, vp, vp]),
        "gc_iknp_multi_send_bits": (i32, [vp, vp, sz, sz, vp]),
        "gc_gmw_triples_multi_sender_u_dev": (i32, [vp, vp, vp, sz]),
        "gc_gmw_triples_multi_sender_fold_dev": (i32, [vp, vp, vp, vp, vp, sz, sz]),
        "gc_gmw_triples_multi_receiver_fold_dev": (i32, [vp, vp, vp, sz, sz]),
        "gc_cot_multi_send_pads": (i32, [vp, vp, vp, vp, vp, sz, sz, vp]),
        "gc_cot_multi_send_pads_dev": (i32, [vp, vp, vp, vp, vp, sz, sz, vp]),
        "gc_cot_multi_receive_unpad": (i32, [vp, vp, vp, vp, vp, sz, sz]),
        "gc_cot_multi_receive_unpad_dev": (i32, [vp, vp, vp, vp, vp, sz, sz]),
        "gc_kos_multi_receiver_tags": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp]),
        "gc_kos_multi_receiver_tags_dev": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp]),
        "gc_kos_multi_sender_check": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp]),
        "gc_kos_multi_sender_check_dev": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp]),
        "gc_sha2pc_garbler_create": (vp, [vp, vp, C.c_uint32, C.c_uint32, sz, ip]),
        "gc_sha2pc_evaluator_create": (vp, [vp, vp, C.c_uint32, C.c_uint32, sz, ip]),
        "gc_sha2pc_garbler_free": (None, [vp]),
        "gc_sha2pc_evaluator_free": (None, [vp]),
        "gc_sha2pc_layout": (i32, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t)]),
        "gc_sha2pc_layout_plan": (i32, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_size_t)]),
        "gc_sha2pc_garbler_round1_dev": (i32, [vp, vp, vp, vp, vp, vp, sz, vp]),
        "gc_sha2pc_evaluator_round2_dev": (i32, [vp, vp, sz, vp, vp, vp, vp, vp, sz, vp]),
        "gc_sha2pc_garbler_round3_dev": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]),
        "gc_sha2pc_evaluator_round4_dev": (i32, [vp, vp, vp, vp, vp, vp, sz, vp, vp]),
        "gc_sha2pc_garbler_round1": (i32, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_sha2pc_evaluator_round2": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_sha2pc_garbler_round3": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_sha2pc_evaluator_round4": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_rand_create": (vp, [vp, vp, sz, vp, sz, ip]),
        "gc_rand_create_dev": (vp, [vp, vp, sz, vp, sz, ip]),
        "gc_rand_free": (None, [vp]),
        "gc_rand_info": (i32, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
        "gc_rand_seek": (i32, [vp, C.c_uint64]),
        "gc_rand_fill_dev": (i32, [vp, sz, vp, sz]),
        "gc_rand_fill": (i32, [vp, sz, vp, sz]),
        "gc_rand_gmw_shares_dev": (i32, [vp, sz, vp, vp]),
        "gc_rand_cur_set_dev": (i32, [vp, vp, C.c_uint64]),
        "gc_rand_fill_cur_dev": (i32, [vp, vp, sz, vp, sz, vp]),
        "gc_rand_scalars_cur_dev": (i32, [vp, vp, vp, sz, vp, vp]),
        "gc_rand_fill_cur": (i32, [vp, vp, sz, vp, sz, C.POINTER(C.c_size_t)]),
        "gc_rand_scalars_cur": (i32, [vp, vp, vp, sz, vp, C.POINTER(C.c_size_t)]),
        "gc_yao_garbler_create": (vp, [vp, vp, C.c_uint32, C.c_uint32, sz, sz, ip]),
        "gc_yao_evaluator_create": (vp, [vp, vp, C.c_uint32, C.c_uint32, sz, sz, ip]),
        "gc_yao_garbler_free": (None, [vp]),
        "gc_yao_evaluator_free": (None, [vp]),
        "gc_yao_layout": (i32, [vp, C.c_uint32, C.c_uint32, sz, C.POINTER(C.c_size_t)]),
        "gc_yao_layout_plan": (i32, [vp, C.c_uint32, C.c_uint32, sz, C.POINTER(C.c_size_t)]),
        "gc_yao_kernel_shape": (i32, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "gc_yao_garbler_batch": (vp, [vp]),
        "gc_yao_evaluator_batch": (vp, [vp]),
        "gc_yao_garbler_send_dev": (i32, [vp, vp, vp, vp, vp, sz]),
        "gc_yao_garbler_ot_wires_dev": (i32, [vp, vp]),
        "gc_yao_garbler_result_dev": (i32, [vp, vp, sz, vp, sz, vp, vp, vp]),
        "gc_yao_evaluator_accept_dev": (i32, [vp, vp, sz, vp]),
        "gc_yao_evaluator_eval_dev": (i32, [vp, vp, vp, sz, vp]),
        "gc_yao_evaluator_result_dev": (i32, [vp, vp, sz, vp, vp]),
        "gc_yao_garbler_send": (i32, [vp, vp, vp, vp, vp]),
        "gc_yao_garbler_ot_wires": (i32, [vp, vp]),
        "gc_yao_garbler_result": (i32, [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_yao_evaluator_accept": (i32, [vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_yao_evaluator_eval": (i32, [vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
        "gc_yao_evaluator_result": (i32, [vp, vp, vp, vp, C.POINTER(C.c_size_t)]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    if L.gc_abi_version() != ABI_VERSION:
        raise ImportError("libgcengine.so ABI %d != %d" % (L.gc_abi_version(), ABI_VERSION))
    return L


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _dp(d):
    """device pointer argument: a DeviceBuffer, or a raw device address (int)"""
    return C.c_void_p(d.ptr if isinstance(d, DeviceBuffer) else d)


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _check(rc, what):
    if rc != GC_OK:
        raise EngineError(rc, what)


def device_count():
    return lib().gc_device_count()


class PinnedArray:
    """numpy array backed by gc_host_alloc (pinned, DMA-able host memory): what the Go shim's scratch pool hands to
    gc_garble / gc_eval.  Keep the object alive as long as views of .a are in use."""

    def __init__(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        self.ptr = lib().gc_host_alloc(max(n, 16))
        if not self.ptr:
            raise EngineError(GC_E_NOMEM, "gc_host_alloc(%d)" % n)
        buf = (C.c_uint8 * max(n, 1)).from_address(self.ptr)
        self.a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self.ptr:
            self.a = None
            lib().gc_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- plan (host only) ---------------------------------------------------------------------


def _flat_geometry(plan_h):
    us, mp = C.c_uint32(0), C.c_uint32(0)
    _check(lib().gc_plan_flat_geometry(plan_h, C.byref(us), C.byref(mp)), "gc_plan_flat_geometry")
    return us.value, mp.value


class Plan:
    """Levelised plan of a circuit; needs no GPU (gc_plan_*)."""

    def __init__(self, gates, nwires, ninputs, noutputs):
        L = lib()
        g = np.ascontiguousarray(gates, dtype=GATE)
        st = C.c_int(0)
        self.h = L.gc_plan_create(_p(g), len(g), nwires, ninputs, noutputs, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_plan_create")
        self._describe(len(g))

    def _describe(self, n):
        L = lib()
        self.info = PlanInfo()
        _check(L.gc_plan_get_info(self.h, C.byref(self.info)), "gc_plan_get_info")
        self.level_of_gate = np.zeros(n, np.uint32)
        self.tweak_of_gate = np.zeros(n, np.uint32)
        self.row_of_gate = np.zeros(n + 1, np.uint32)
        self.slot_of_gate = np.zeros(n, np.uint32)
        _check(L.gc_plan_describe(self.h, _p(self.level_of_gate), _p(self.tweak_of_gate), _p(self.row_of_gate),
                                  _p(self.slot_of_gate)), "gc_plan_describe")

    @classmethod
    def chain(cls, steps):
        """the merged plan of a fused chain (gc_plan_create_chain).  steps: [(gates, nwires, nin, nout, wiring)], wiring per
        input 0xffffffff (wire store) or m << 24 | j (output j of step m); None for a step that reads the store only"""
        L = lib()
        n = len(steps)
        keep = []
        gp, wp = (C.c_void_p * n)(), (C.c_void_p * n)()
        ng, nw, ni, no = (np.zeros(n, np.uint32) for _ in range(4))
        for k, (gates, nwires, nin, nout, wiring) in enumerate(steps):
            g = np.ascontiguousarray(gates, dtype=GATE)
            w = np.full(nin, 0xFFFFFFFF, np.uint32) if wiring is None else np.ascontiguousarray(wiring, dtype=np.uint32)
            assert len(w) == nin
            keep += [g, w]
            gp[k], wp[k] = g.ctypes.data, w.ctypes.data
            ng[k], nw[k], ni[k], no[k] = len(g), nwires, nin, nout
        st = C.c_int(0)
        self = cls.__new__(cls)
        self.h = L.gc_plan_create_chain(gp, _p(ng), _p(nw), _p(ni), _p(no), wp, n, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_plan_create_chain")
        self._describe(int(ng.sum()))
        self.gate_base = np.concatenate([[0], np.cumsum(ng)]).astype(np.uint32)
        return self

    def fingerprint(self):
        """64-bit fingerprint of the device program of this plan (gc_plan_fingerprint), as 16 hex digits"""
        fp = C.c_uint64(0)
        _check(lib().gc_plan_fingerprint(self.h, C.byref(fp)), "gc_plan_fingerprint")
        return "%016x" % fp.value

    def flat_geometry(self):
        """(uint4 per LDS stage buffer, largest part count of an XOR list) of the flattened schedule"""
        return _flat_geometry(self.h)

    def simulate(self, in_bits):
        """plaintext walk of the flattened unit program (gc_plan_simulate): output bits"""
        b = np.ascontiguousarray(in_bits, dtype=np.uint8)
        assert len(b) == self.info.ninputs
        out = np.zeros(max(self.info.noutputs, 1), np.uint8)
        _check(lib().gc_plan_simulate(self.h, _p(b) if len(b) else None, _p(out)), "gc_plan_simulate")
        return out[: self.info.noutputs]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gc_plan_free(self.h)
            self.h = None


# ---- device objects -----------------------------------------------------------------------


class Context:
    def __init__(self, device=0):
        st = C.c_int(0)
        self.h = lib().gc_ctx_create(device, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_ctx_create(%d)" % device)
        self.device = device

    def coop_stats(self):
        """(state of the cooperative one-instance passes: 0 unused / 1 in use / -1 off, passes that lost a workgroup and were
        done again on the device)"""
        a, b = C.c_int(0), C.c_uint64(0)
        _check(lib().gc_ctx_coop_stats(self.h, C.byref(a), C.byref(b)), "gc_ctx_coop_stats")
        return a.value, b.value

    def pci_bus_id(self):
        """the device's PCI bus id ("0000:75:00.0"): tells the ranks' GPUs apart when every process sees its own as device 0"""
        b = C.create_string_buffer(32)
        _check(lib().gc_ctx_pci_bus_id(self.h, b, 32), "gc_ctx_pci_bus_id")
        return b.value.decode()

    def sync(self):
        _check(lib().gc_ctx_sync(self.h), "gc_ctx_sync")

    @property
    def stream(self):
        return lib().gc_ctx_stream(self.h)

    def capture(self, fn):
        """record the device-resident calls fn() makes on this ctx into a Graph (gc_ctx_capture_*)"""
        _check(lib().gc_ctx_capture_begin(self.h), "gc_ctx_capture_begin")
        g = C.c_void_p()
        try:
            fn()
        except BaseException:  # leave capture mode and drop the partial graph before the error travels on
            if lib().gc_ctx_capture_end(self.h, C.byref(g)) == GC_OK and g:
                lib().gc_graph_free(g)
            raise
        _check(lib().gc_ctx_capture_end(self.h, C.byref(g)), "gc_ctx_capture_end")
        return Graph(g)

    def zeros(self, shape, dtype=np.uint8):
        """zero-filled device buffer (gc_dev_alloc + gc_dev_memset)"""
        return DeviceBuffer(self, shape, dtype, zero=True)

    def empty(self, shape, dtype=np.uint8):
        return DeviceBuffer(self, shape, dtype)

    def random_u8(self, shape, high=256, seed=0):
        """synthetic uniform bytes in [0, high) (numpy Generator on the host, uploaded once): bench / profiling inputs"""
        return DeviceBuffer(self, data=np.random.default_rng(seed).integers(0, high, shape, dtype=np.uint8))

    def to_device(self, data):
        """host bytes / array -> device buffer (gc_dev_alloc + gc_dev_upload)"""
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(bytes(data), np.uint8)
        return DeviceBuffer(self, data=data)

    def close(self):
        if self.h:
            lib().gc_ctx_destroy(self.h)
            self.h = None


class DeviceBuffer:
    """gc_dev_alloc: a device buffer owned through the C ABI (no torch, no HIP binding on the host side) — what the
    device-resident calls take as d_* pointers.  .ptr is the device address (int); offsets are plain arithmetic.
    dtype / shape are host-side book-keeping for numpy() only."""

    def __init__(self, ctx, shape=None, dtype=np.uint8, data=None, zero=False):
        self.ctx = ctx
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, data.dtype
        self.dtype = np.dtype(dtype)
        self.shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        st = C.c_int(0)
        self.ptr = lib().gc_dev_alloc(ctx.h, max(self.nbytes, 16), C.byref(st))
        if not self.ptr:
            raise EngineError(st.value, "gc_dev_alloc(%d)" % self.nbytes)
        if data is not None:
            self.upload(data)
        elif zero:
            self.zero()

    def upload(self, data, offset=0):
        a = np.ascontiguousarray(data)
        assert offset + a.nbytes <= self.nbytes
        _check(lib().gc_dev_upload(self.ctx.h, C.c_void_p(self.ptr + offset), _p(a) if a.nbytes else None, a.nbytes),
               "gc_dev_upload")
        return self

    def download(self, dtype=np.uint8, shape=None, offset=0, nbytes=None):
        dtype = np.dtype(dtype)
        n = (self.nbytes - offset if nbytes is None else nbytes) if shape is None else int(np.prod(shape)) * dtype.itemsize
        assert offset + n <= self.nbytes
        out = np.empty(n // dtype.itemsize, dtype)
        _check(lib().gc_dev_download(self.ctx.h, _p(out) if n else None, C.c_void_p(self.ptr + offset), n),
               "gc_dev_download")
        return out if shape is None else out.reshape(shape)

    def __add__(self, offset):
        """device address `offset` bytes into the buffer (plain pointer arithmetic)"""
        assert 0 <= offset <= self.nbytes
        return self.ptr + int(offset)

    def numpy(self):
        """the whole buffer as a host array of the buffer's dtype / shape (waits for the ctx stream)"""
        return self.download(self.dtype, self.shape)

    def zero(self, value=0):
        _check(lib().gc_dev_memset(self.ctx.h, C.c_void_p(self.ptr), value, self.nbytes), "gc_dev_memset")
        return self

    def copy_from(self, d_src, nbytes, offset=0):
        """device -> device on the ctx stream (d_src: DeviceBuffer or device address)"""
        src = d_src.ptr if isinstance(d_src, DeviceBuffer) else int(d_src)
        _check(lib().gc_dev_copy(self.ctx.h, C.c_void_p(self.ptr + offset), C.c_void_p(src), nbytes), "gc_dev_copy")

    def close(self):
        if getattr(self, "ptr", None) and self.ctx.h:
            lib().gc_dev_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    def __init__(self, h):
        self.h = h

    def launch(self):
        _check(lib().gc_graph_launch(self.h), "gc_graph_launch")

    def close(self):
        if self.h:
            lib().gc_graph_free(self.h)
            self.h = None


class DeviceCircuit:
    """gc_circ: a circuit.Circuit uploaded to one device."""

    def __init__(self, ctx, circuit, schedule=None):
        self.ctx = ctx
        self.c = circuit
        st = C.c_int(0)
        g = np.ascontiguousarray(circuit.Gates, dtype=GATE)
        self.h = lib().gc_circ_load(ctx.h, _p(g), len(g), circuit.NumWires, circuit.num_inputs, circuit.num_outputs,
                                    C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_circ_load")
        self.info = PlanInfo()
        _check(lib().gc_plan_get_info(lib().gc_circ_plan(self.h), C.byref(self.info)), "gc_plan_get_info")
        if schedule is not None:
            self.set_schedule(schedule)

    def set_schedule(self, schedule):
        _check(lib().gc_circ_set_schedule(self.h, schedule), "gc_circ_set_schedule")

    def flat_geometry(self):
        """Plan.flat_geometry of the uploaded circuit's plan"""
        return _flat_geometry(lib().gc_circ_plan(self.h))

    @property
    def tables_wire_bytes(self):
        return int(lib().gc_tables_wire_bytes(self.h))

    # -- host-buffer API: Circuit.Garble / Circuit.Eval with a batch dimension --

    def garble(self, key, rnd, batch=1, want_wires=False, want_io=True):
        """gc_garble.  Returns dict(R[batch], slab[batch,rows], wires[batch,nwires]?, io[batch,nin+nout]?)."""
        k, r = _u8(key), _u8(rnd)
        R = np.zeros(batch, LABEL)
        slab = np.zeros((batch, max(self.info.slab_rows, 1)), LABEL)
        wires = np.zeros((batch, self.c.NumWires), WIRE) if want_wires else None
        io = np.zeros((batch, self.c.num_inputs + self.c.num_outputs), WIRE) if want_io else None
        rc = lib().gc_garble(self.h, _p(k), len(k), _p(r), len(r), batch, _p(R), _p(wires), _p(io), _p(slab))
        _check(rc, "gc_garble")
        out = {"R": R, "slab": slab[:, : self.info.slab_rows]}
        if want_wires:
            out["wires"] = wires
        if want_io:
            out["io"] = io
        return out

    def eval(self, key, slab, wires=None, inputs=None, batch=1, slab_rows=None):
        """gc_eval.  wires: LABEL [batch,nwires] (in place) or inputs: LABEL [batch,ninputs].
        Returns output labels [batch,noutputs]."""
        k = _u8(key)
        slab = np.ascontiguousarray(slab, dtype=LABEL)
        rows = slab.size // batch if slab_rows is None else slab_rows
        out = np.zeros((batch, max(self.c.num_outputs, 1)), LABEL)
        if wires is not None:
            assert wires.dtype == LABEL and wires.flags.c_contiguous and wires.size == batch * self.c.NumWires
        if inputs is not None:
            inputs = np.ascontiguousarray(inputs, dtype=LABEL)
        rc = lib().gc_eval(self.h, _p(k), len(k), batch, _p(wires), _p(inputs), _p(slab) if slab.size else None,
                           rows, _p(out))
        _check(rc, "gc_eval")
        return out[:, : self.c.num_outputs]

    def garble_wire(self, key, rnd, batch=1):
        """gc_garble_wire: dict(R, io, wire[batch, tables_wire_bytes] as uint8)"""
        k, r = _u8(key), _u8(rnd)
        stride = (self.tables_wire_bytes + 3) & ~3
        R = np.zeros(batch, LABEL)
        io = np.zeros((batch, self.c.num_inputs + self.c.num_outputs), WIRE)
        wire = np.zeros((batch, stride), np.uint8)
        _check(lib().gc_garble_wire(self.h, _p(k), len(k), _p(r), len(r), batch, _p(R), _p(io), _p(wire), stride),
               "gc_garble_wire")
        return {"R": R, "io": io, "wire": wire}

    def eval_wire(self, key, wire, inputs, batch=1):
        """gc_eval_wire: output labels [batch, noutputs]; raises GC_E_ROWS on malformed headers"""
        k = _u8(key)
        w = np.ascontiguousarray(wire, dtype=np.uint8).reshape(batch, -1)
        inp = np.ascontiguousarray(inputs, dtype=LABEL)
        out = np.zeros((batch, max(self.c.num_outputs, 1)), LABEL)
        bad = C.c_uint32(0)
        _check(lib().gc_eval_wire(self.h, _p(k), len(k), batch, _p(inp), _p(w), w.shape[1], _p(out), C.byref(bad)),
               "gc_eval_wire")
        return out[:, : self.c.num_outputs]

    def close(self):
        if self.h:
            lib().gc_circ_free(self.h)
            self.h = None


class Batch:
    """gc_batch: device-resident state of `batch` instances (garbler or evaluator role)."""

    def __init__(self, dcirc, batch):
        self.dc = dcirc
        self.batch = batch
        st = C.c_int(0)
        self.h = lib().gc_batch_create(dcirc.h, batch, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_batch_create")

    @property
    def stride(self):
        """instances per row of the device arrays (gc_batch_stride); set_schedule can change it"""
        return int(lib().gc_batch_stride(self.h))

    @property
    def tile_instances(self):
        return int(lib().gc_batch_tile_instances(self.h))

    @property
    def lds_wires(self):
        return bool(lib().gc_batch_wires_in_lds(self.h))

    def set_graph(self, on):
        _check(lib().gc_batch_set_graph(self.h, 1 if on else 0), "gc_batch_set_graph")

    def set_schedule(self, s):
        _check(lib().gc_batch_set_schedule(self.h, s), "gc_batch_set_schedule")

    def set_store_all(self, on):
        _check(lib().gc_batch_set_store_all(self.h, 1 if on else 0), "gc_batch_set_store_all")

    def garble(self, key, d_rnd):
        k = _u8(key)
        _check(lib().gc_batch_garble(self.h, _p(k), len(k), _dp(d_rnd)), "gc_batch_garble")

    def select_inputs(self, garbler, d_bits):
        _check(lib().gc_batch_select_inputs(self.h, garbler.h, _dp(d_bits)), "gc_batch_select_inputs")

    def set_inputs(self, d_labels):
        _check(lib().gc_batch_set_inputs(self.h, _dp(d_labels)), "gc_batch_set_inputs")

    def eval(self, key, tables):
        k = _u8(key)
        _check(lib().gc_batch_eval(self.h, _p(k), len(k), tables.h), "gc_batch_eval")

    def keyed_supported(self):
        """can this batch run garble_keyed / eval_keyed (gc_batch_keyed_supported)?"""
        return bool(lib().gc_batch_keyed_supported(self.h))

    @property
    def keyed_path(self):
        """which kernels garble_keyed / eval_keyed run on this batch now (gc_batch_keyed_path): 0 none, 1 the flattened kernels
        with the wires in LDS, 2 the level-walking kernels with the wires in HBM"""
        return int(lib().gc_batch_keyed_path(self.h))

    def set_keyed_path(self, path):
        """gc_batch_set_keyed_path: 2 sends the keyed calls to the HBM-wire kernels whatever the batch's geometry, 0 is the rule"""
        _check(lib().gc_batch_set_keyed_path(self.h, int(path)), "gc_batch_set_keyed_path")

    @property
    def keyed_hbm_form(self):
        """which form of the HBM-wire kernels the keyed calls run on this batch now (gc_batch_keyed_hbm_form): 0 when keyed_path
        is not 2, 1 the plain form, 2 the split form (hash waves and free waves on levels wider than 1 024 column lanes)"""
        return int(lib().gc_batch_keyed_hbm_form(self.h))

    def set_keyed_hbm_form(self, form):
        """gc_batch_set_keyed_hbm_form: 0 the rule, 1 always the plain form, 2 always the split form"""
        _check(lib().gc_batch_set_keyed_hbm_form(self.h, int(form)), "gc_batch_set_keyed_hbm_form")

    def debug_keyed_hbm_hash_waves(self, garble_h, eval_h):
        """gc_batch_debug_keyed_hbm_hash_waves: fix the hash waves of every split level (1 .. 15, 0 the rule), for measurements"""
        _check(lib().gc_batch_debug_keyed_hbm_hash_waves(self.h, int(garble_h), int(eval_h)), "gc_batch_debug_keyed_hbm_hash_waves")

    def garble_keyed(self, d_keys, keylen, d_rnd):
        """gc_batch_garble_keyed: d_keys = device u8 [batch][keylen], one AES key per instance"""
        _check(lib().gc_batch_garble_keyed(self.h, _dp(d_keys), keylen, _dp(d_rnd)), "gc_batch_garble_keyed")

    def eval_keyed(self, d_keys, keylen, tables):
        _check(lib().gc_batch_eval_keyed(self.h, _dp(d_keys), keylen, tables.h), "gc_batch_eval_keyed")

    def debug_keyed_schedule(self, d_keys, keylen):
        """(device, host) round-key words [batch][4 * (rounds + 1)] of the keyed passes (gc_batch_debug_keyed_schedule)"""
        nw = 4 * (keylen // 4 + 7)
        dev, host = np.zeros((self.batch, nw), np.uint32), np.zeros((self.batch, nw), np.uint32)
        _check(lib().gc_batch_debug_keyed_schedule(self.h, _dp(d_keys), keylen, _p(dev), _p(host)), "gc_batch_debug_keyed_schedule")
        return dev, host

    def decode(self, evaluator, d_bits_out, d_mismatch):
        _check(lib().gc_batch_decode(self.h, evaluator.h, _dp(d_bits_out), _dp(d_mismatch)),
               "gc_batch_decode")

    def read_r(self):
        out = np.zeros(self.batch, LABEL)
        _check(lib().gc_batch_read_r(self.h, _p(out)), "gc_batch_read_r")
        return out

    def read_slab(self):
        out = np.zeros((self.batch, max(self.dc.info.slab_rows, 1)), LABEL)
        _check(lib().gc_batch_read_slab(self.h, _p(out)), "gc_batch_read_slab")
        return out[:, : self.dc.info.slab_rows]

    def read_wires(self):
        out = np.zeros((self.batch, self.dc.c.NumWires), WIRE)
        _check(lib().gc_batch_read_wires(self.h, _p(out)), "gc_batch_read_wires")
        return out

    def read_labels(self):
        out = np.zeros((self.batch, self.dc.c.NumWires), LABEL)
        _check(lib().gc_batch_read_labels(self.h, _p(out)), "gc_batch_read_labels")
        return out

    def read_outputs(self):
        out = np.zeros((self.batch, max(self.dc.c.num_outputs, 1)), LABEL)
        _check(lib().gc_batch_read_outputs(self.h, _p(out)), "gc_batch_read_outputs")
        return out[:, : self.dc.c.num_outputs]

    def write_slab(self, slab):
        s = np.ascontiguousarray(slab, dtype=LABEL)
        assert s.size == self.batch * self.dc.info.slab_rows
        _check(lib().gc_batch_write_slab(self.h, _p(s)), "gc_batch_write_slab")

    def egress_tables(self, d_out, stride):
        _check(lib().gc_batch_egress_tables(self.h, _dp(d_out), stride), "gc_batch_egress_tables")

    def gather_input_wires(self, first, count, d_out):
        _check(lib().gc_batch_gather_input_wires(self.h, first, count, _dp(d_out)), "gc_batch_gather_input_wires")

    def set_input_range(self, first, count, d_labels):
        _check(lib().gc_batch_set_input_range(self.h, first, count, _dp(d_labels)), "gc_batch_set_input_range")

    def egress_tables_dense(self, d_out, stride):
        _check(lib().gc_batch_egress_tables_dense(self.h, _dp(d_out), stride), "gc_batch_egress_tables_dense")

    def ingest_tables_dense(self, d_in, stride):
        _check(lib().gc_batch_ingest_tables_dense(self.h, _dp(d_in), stride), "gc_batch_ingest_tables_dense")

    def ingest_tables(self, d_in, stride, d_bad):
        _check(lib().gc_batch_ingest_tables(self.h, _dp(d_in), stride, _dp(d_bad)),
               "gc_batch_ingest_tables")

    def gather_outputs(self, d_out):
        _check(lib().gc_batch_gather_outputs(self.h, _dp(d_out)), "gc_batch_gather_outputs")

    def debug_profile(self, enable=True, read=False):
        out = np.zeros(16, np.uint64) if read else None
        _check(lib().gc_batch_debug_profile(self.h, 1 if enable else 0, _p(out)), "gc_batch_debug_profile")
        return out

    @property
    def last_ms(self):
        return float(lib().gc_batch_last_ms(self.h))

    @property
    def last_launches(self):
        return int(lib().gc_batch_last_launches(self.h))

    def close(self):
        if self.h:
            lib().gc_batch_free(self.h)
            self.h = None


class Stream:
    """gc_stream: NewStreaming / Streaming.Garble / GetInput (circuit/stream_garble.go)"""

    def __init__(self, ctx, key, rnd, inputs):
        k, r = _u8(key), _u8(rnd)
        inp = np.ascontiguousarray(inputs, dtype=np.uint32)
        st = C.c_int(0)
        self.h = lib().gc_stream_create(ctx.h, _p(k), len(k), _p(r), len(r), _p(inp), len(inp), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_create")

    def get(self, w):
        out = np.zeros(1, WIRE)
        _check(lib().gc_stream_get_wire(self.h, w, _p(out)), "gc_stream_get_wire")
        return out[0]

    def garble(self, gates, nwires, in_, out_):
        g = np.ascontiguousarray(gates, dtype=GATE)
        i = np.ascontiguousarray(in_, dtype=np.uint32)
        o = np.ascontiguousarray(out_, dtype=np.uint32)
        need = len(g) * 61 + 16  # upper bound: 13 header bytes + 3 rows per gate
        buf = getattr(self, "_buf", None)
        if buf is None or len(buf) < need:  # reused across calls: a fresh 8 MB array per step costs more than the step
            buf = self._buf = np.empty(need + need // 2, np.uint8)
        n = C.c_size_t(0)
        _check(lib().gc_stream_garble(self.h, _p(g), len(g), nwires, _p(i), len(i), _p(o), len(o), _p(buf), len(buf),
                                      C.byref(n)), "gc_stream_garble")
        return buf[: n.value].tobytes()

    def intern(self, gates, nwires, nin, nout):
        """gc_stream_intern: handle of a circuit (looked up by content once)"""
        g = np.ascontiguousarray(gates, dtype=GATE)
        h = C.c_uint32(0)
        _check(lib().gc_stream_intern(self.h, _p(g), len(g), nwires, nin, nout, C.byref(h)), "gc_stream_intern")
        need = len(g) * 61 + 16  # the buffer garble_finish fills must hold the largest circuit in flight
        buf = getattr(self, "_buf", None)
        if buf is None or len(buf) < need:
            self._buf = np.empty(need + need // 2, np.uint8)
        return h.value

    def release(self, handle):
        """gc_stream_release: the interned circuit goes back to the bounded cache, the handle is invalid afterwards"""
        _check(lib().gc_stream_release(self.h, handle), "gc_stream_release")

    def garble_begin_h(self, handle, in_, out_):
        """gc_stream_garble_begin_h: queue an interned circuit"""
        i = np.ascontiguousarray(in_, dtype=np.uint32)
        o = np.ascontiguousarray(out_, dtype=np.uint32)
        _check(lib().gc_stream_garble_begin_h(self.h, handle, _p(i), _p(o)), "gc_stream_garble_begin_h")

    def flush(self):
        """gc_stream_garble_flush: launch the queued group without waiting"""
        _check(lib().gc_stream_garble_flush(self.h), "gc_stream_garble_flush")

    def stats(self):
        """(groups launched, steps that ran in groups, steps with a launch sequence of their own)"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().gc_stream_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "gc_stream_stats")
        return a.value, b.value, c.value

    def deep_stats(self):
        """(steps that ran on a deep lane — long one-workgroup passes beside the step groups —, lanes in use)"""
        a, b = C.c_uint64(0), C.c_uint32(0)
        _check(lib().gc_stream_deep_stats(self.h, C.byref(a), C.byref(b)), "gc_stream_deep_stats")
        return a.value, b.value

    def fuse_stats(self):
        """chain fusion (gc_stream_fuse_stats): (launch units of several steps, steps in them, merged plans built, units that
        ran step by step for want of a one-workgroup plan)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_fuse_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_fuse_stats")
        return tuple(x.value for x in v)

    def wait_stats(self):
        """units that joined the group they conflict with and wait for units of it on the device (gc_stream_wait_stats)"""
        v = C.c_uint64(0)
        _check(lib().gc_stream_wait_stats(self.h, C.byref(v)), "gc_stream_wait_stats")
        return v.value

    def garble_begin(self, gates, nwires, in_, out_):
        """gc_stream_garble_begin: queue one circuit, do not wait (up to 4 096 in flight; small independent circuits
        share a launch sequence)"""
        g = np.ascontiguousarray(gates, dtype=GATE)
        i = np.ascontiguousarray(in_, dtype=np.uint32)
        o = np.ascontiguousarray(out_, dtype=np.uint32)
        need = len(g) * 61 + 16
        buf = getattr(self, "_buf", None)
        if buf is None or len(buf) < need:
            self._buf = np.empty(need + need // 2, np.uint8)
        _check(lib().gc_stream_garble_begin(self.h, _p(g), len(g), nwires, _p(i), len(i), _p(o), len(o)),
               "gc_stream_garble_begin")

    def garble_finish(self):
        """gc_stream_garble_finish: the bytes of the oldest circuit in flight"""
        n = C.c_size_t(0)
        _check(lib().gc_stream_garble_finish(self.h, _p(self._buf), len(self._buf), C.byref(n)), "gc_stream_garble_finish")
        return self._buf[: n.value].tobytes()

    def garble_finish_async(self, dst, offset):
        """gc_stream_garble_finish_async: the bytes of the oldest circuit in flight into dst[offset:] (a numpy uint8 array the
        caller keeps alive and untouched until copies_wait) — copied by the stream's copier threads; returns the byte count"""
        n = C.c_size_t(0)
        _check(lib().gc_stream_garble_finish_async(self.h, C.c_void_p(dst.ctypes.data + offset), len(dst) - offset, C.byref(n)),
               "gc_stream_garble_finish_async")
        return n.value

    def copies_wait(self):
        _check(lib().gc_stream_garble_copies_wait(self.h), "gc_stream_garble_copies_wait")

    def garble_finish_view(self):
        """gc_stream_garble_finish_view: the same bytes without the engine's copy — read in place from its pinned staging
        (the pointer is valid until the next finish call; the copy made here is the caller's own)"""
        ptr, n = C.c_void_p(None), C.c_size_t(0)
        _check(lib().gc_stream_garble_finish_view(self.h, C.byref(ptr), C.byref(n)), "gc_stream_garble_finish_view")
        return C.string_at(ptr, n.value) if n.value else b""

    def close(self):
        if self.h:
            lib().gc_stream_free(self.h)
            self.h = None


class StreamEval:
    """gc_stream_eval: StreamEval store + the per-gate loop of one OpCircuit block (stream_evaluator.go)"""

    def __init__(self, ctx, key):
        k = _u8(key)
        st = C.c_int(0)
        self.h = lib().gc_stream_eval_create(ctx.h, _p(k), len(k), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_eval_create")

    def set(self, w, label):
        _check(lib().gc_stream_eval_set_wire(self.h, w, _p(_lab1(label))), "gc_stream_eval_set_wire")

    def get(self, w):
        out = np.zeros(1, LABEL)
        _check(lib().gc_stream_eval_get_wire(self.h, w, _p(out)), "gc_stream_eval_get_wire")
        return (int(out[0]["d0"]), int(out[0]["d1"]))

    def circuit(self, ngates, ntmp, nwires, data):
        b = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        n = C.c_size_t(0)
        _check(lib().gc_stream_eval_circuit(self.h, ngates, ntmp, nwires, _p(b), len(data), C.byref(n)),
               "gc_stream_eval_circuit")
        return n.value

    def blocks(self, data):
        """gc_stream_eval_blocks: framed OpCircuit blocks (20-byte headers included) -> (bytes used, blocks evaluated, more)"""
        b = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        n, nb, more = C.c_size_t(0), C.c_uint32(0), C.c_int(0)
        rc = lib().gc_stream_eval_blocks(self.h, _p(b), len(data), C.byref(n), C.byref(nb), C.byref(more))
        self.last_blocks = (n.value, nb.value, bool(more.value))  # (also when a block is refused: the ones before it are done)
        _check(rc, "gc_stream_eval_blocks")
        return self.last_blocks

    def stats(self):
        """(blocks parsed gate by gate, blocks recognised by their byte skeleton)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().gc_stream_eval_stats(self.h, C.byref(a), C.byref(b)), "gc_stream_eval_stats")
        return a.value, b.value

    def deep_stats(self):
        """(blocks that ran on a deep lane, lanes in use)"""
        a, b = C.c_uint64(0), C.c_uint32(0)
        _check(lib().gc_stream_eval_deep_stats(self.h, C.byref(a), C.byref(b)), "gc_stream_eval_deep_stats")
        return a.value, b.value

    def dev_stats(self):
        """(blocks of read buffers handed to gc_stream_eval_blocks that were scheduled on a DEVICE verdict, blocks the device was
        asked about that went to the host's matcher / parser after all): disjoint counts"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().gc_stream_eval_dev_stats(self.h, C.byref(a), C.byref(b)), "gc_stream_eval_dev_stats")
        return a.value, b.value

    def blocks_at(self, address, nbytes):
        """gc_stream_eval_blocks on caller memory given by address (a piece of a pinned read buffer: no copy)"""
        n, nb, more = C.c_size_t(0), C.c_uint32(0), C.c_int(0)
        rc = lib().gc_stream_eval_blocks(self.h, C.c_void_p(address), nbytes, C.byref(n), C.byref(nb), C.byref(more))
        self.last_blocks = (n.value, nb.value, bool(more.value))
        _check(rc, "gc_stream_eval_blocks")
        return self.last_blocks

    def fuse_stats(self):
        """chain fusion on the evaluator's side (gc_stream_eval_fuse_stats)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_eval_fuse_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_eval_fuse_stats")
        return tuple(x.value for x in v)

    def wait_stats(self):
        """the evaluator's counterpart of Stream.wait_stats (gc_stream_eval_wait_stats)"""
        v = C.c_uint64(0)
        _check(lib().gc_stream_eval_wait_stats(self.h, C.byref(v)), "gc_stream_eval_wait_stats")
        return v.value

    def close(self):
        if self.h:
            lib().gc_stream_eval_free(self.h)
            self.h = None


def stream_batch_step_bytes(gates, nwires, in_, out_):
    """gc_stream_batch_step_bytes (host only): the bytes Streaming.Garble writes for this step, the same for every session; 0
    for a step gc_stream_batch_garble refuses by its shape (lib().gc_last_error() says why)"""
    g = np.ascontiguousarray(gates, dtype=GATE)
    i = np.ascontiguousarray(in_, dtype=np.uint32)
    o = np.ascontiguousarray(out_, dtype=np.uint32)
    return lib().gc_stream_batch_step_bytes(_p(g), len(g), nwires, _p(i), len(i), _p(o), len(o))


class StreamBatch:
    """gc_stream_batch: NewStreaming / Streaming.Garble / GetInput for S sessions of one program per call.  d_keys: device
    u8 [S][keylen]; d_rnd: device u8 [S][1 + len(inputs)][16]."""

    def __init__(self, ctx, sessions, d_keys, keylen, d_rnd, inputs):
        self.sessions = sessions
        inp = np.ascontiguousarray(inputs, dtype=np.uint32)
        st = C.c_int(0)
        self.h = lib().gc_stream_batch_create(ctx.h, sessions, _dp(d_keys), keylen, _dp(d_rnd), _p(inp), len(inp), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_batch_create")

    def garble(self, gates, nwires, in_, out_, d_out, stride):
        """queues one step for every session; returns its byte count (session s's bytes: d_out + s * stride)"""
        g = np.ascontiguousarray(gates, dtype=GATE)
        i = np.ascontiguousarray(in_, dtype=np.uint32)
        o = np.ascontiguousarray(out_, dtype=np.uint32)
        n = C.c_size_t(0)
        _check(lib().gc_stream_batch_garble(self.h, _p(g), len(g), nwires, _p(i), len(i), _p(o), len(o), _dp(d_out), stride,
                                            C.byref(n)), "gc_stream_batch_garble")
        return n.value

    def get(self, w):
        """WIRE [S]: both labels of global wire w in every session (waits for the ctx stream)"""
        out = np.zeros(self.sessions, WIRE)
        _check(lib().gc_stream_batch_get_wire(self.h, w, _p(out)), "gc_stream_batch_get_wire")
        return out

    def gather_wires(self, ids, d_wires_out):
        """{L0, L0 ^ R} of the named wires as gc_wire [S][len(ids)] in device memory; asynchronous"""
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        _check(lib().gc_stream_batch_gather_wires(self.h, _p(i), len(i), _dp(d_wires_out)), "gc_stream_batch_gather_wires")

    def select_labels(self, ids, bits, labels_out=None):
        """the garbler's own input labels: L0 of wire ids[j], ^ R where the bit is not zero.  bits: a DeviceBuffer u8
        [S][len(ids)] with labels_out a DeviceBuffer gc_label [S][len(ids)] (gc_stream_batch_select_labels_dev, asynchronous), or
        a host array, which returns LABEL [S, len(ids)] (gc_stream_batch_select_labels, synchronous)"""
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if isinstance(bits, DeviceBuffer):
            _check(lib().gc_stream_batch_select_labels_dev(self.h, _p(i), len(i), _dp(bits), _dp(labels_out)),
                   "gc_stream_batch_select_labels_dev")
            return labels_out
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        if b.shape != (self.sessions, len(i)):
            raise EngineError(GC_E_ARG, "select_labels: bits must be u8 [sessions, len(ids)]")
        out = np.zeros((self.sessions, len(i)), LABEL)
        _check(lib().gc_stream_batch_select_labels(self.h, _p(i), len(i), _p(b), _p(out)), "gc_stream_batch_select_labels")
        return out

    def decode(self, ids, labels, bits_out=None, d_bad=None):
        """the result: 0 / 1 / 0xff per label equal to L0 / L1 / neither of wire ids[j], and per session the number of 0xff.
        labels: a DeviceBuffer gc_label [S][len(ids)] with bits_out (u8 [S][len(ids)]) and d_bad (u32 [S]) DeviceBuffers
        (gc_stream_batch_decode_dev, asynchronous), or a host LABEL array, which returns (bits [S, len(ids)], bad [S])"""
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if isinstance(labels, DeviceBuffer):
            _check(lib().gc_stream_batch_decode_dev(self.h, _p(i), len(i), _dp(labels), _dp(bits_out), _dp(d_bad)),
                   "gc_stream_batch_decode_dev")
            return bits_out, d_bad
        lab = np.ascontiguousarray(labels, dtype=LABEL)
        if lab.shape != (self.sessions, len(i)):
            raise EngineError(GC_E_ARG, "decode: labels must be LABEL [sessions, len(ids)]")
        bits, bad = np.zeros((self.sessions, len(i)), np.uint8), np.zeros(self.sessions, np.uint32)
        _check(lib().gc_stream_batch_decode(self.h, _p(i), len(i), _p(lab), _p(bits), _p(bad)), "gc_stream_batch_decode")
        return bits, bad

    def out(self, window_bytes, nwindows, split=False):
        """a StreamBatchOut of this handle: windows of stream bytes in pinned host memory; close it before this handle.
        split: a step is cut over the windows instead of sealing one short or growing it (gc_stream_batch_out_create_split)"""
        return StreamBatchOut(self, window_bytes, nwindows, split)

    def set_fallback(self, on=True):
        """circuits loaded from now on whose key table alone keeps them out of the keyed scope run on the HBM-wire kernels"""
        _check(lib().gc_stream_batch_set_fallback(self.h, 1 if on else 0), "gc_stream_batch_set_fallback")

    def cache_stats(self):
        """the circuit cache (gc_stream_batch_cache_stats): (entries, device bytes, loads, evictions)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_batch_cache_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_batch_cache_stats")
        return tuple(int(x.value) for x in v)

    def close(self):
        if self.h:
            lib().gc_stream_batch_free(self.h)
            self.h = None


class StreamBatchOut:
    """gc_stream_batch_out: the steps of a StreamBatch written into a ring of windows [S][cap] whose bytes arrive in pinned
    host memory while the next window fills.  One thread may garble / flush while one other takes windows and releases them."""

    def __init__(self, sb, window_bytes, nwindows, split=False):
        self.sessions = sb.sessions
        st = C.c_int(0)
        create = lib().gc_stream_batch_out_create_split if split else lib().gc_stream_batch_out_create
        self.h = create(sb.h, window_bytes, nwindows, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_batch_out_create_split" if split else "gc_stream_batch_out_create")

    def garble(self, prefix, gates, nwires, in_, out_):
        """one step behind `prefix` (bytes, at most 64) for every session; returns the bytes written per session.  Raises
        EngineError with code GC_E_BUSY when no window is free: release one and call again"""
        g = np.ascontiguousarray(gates, dtype=GATE)
        i = np.ascontiguousarray(in_, dtype=np.uint32)
        o = np.ascontiguousarray(out_, dtype=np.uint32)
        pre = bytes(prefix)
        pb = np.frombuffer(pre, np.uint8) if pre else np.zeros(1, np.uint8)
        n = C.c_size_t(0)
        _check(lib().gc_stream_batch_out_garble(self.h, _p(pb), len(pre), _p(g), len(g), nwires, _p(i), len(i), _p(o), len(o),
                                                C.byref(n)), "gc_stream_batch_out_garble")
        return n.value

    def flush(self):
        _check(lib().gc_stream_batch_out_flush(self.h), "gc_stream_batch_out_flush")

    def next(self):
        """the oldest sealed window, its copy complete: (address of session 0's bytes, stride, len), or None"""
        base, stride, n = C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
        _check(lib().gc_stream_batch_out_next(self.h, C.byref(base), C.byref(stride), C.byref(n)), "gc_stream_batch_out_next")
        return (base.value, stride.value, n.value) if n.value else None

    def next_view(self):
        """next() as a numpy view u8 [S, len] of the pinned window (valid until it is released), or None"""
        w = self.next()
        if w is None:
            return None
        base, stride, n = w
        raw = (C.c_uint8 * (self.sessions * stride)).from_address(base)
        return np.frombuffer(raw, np.uint8).reshape(self.sessions, stride)[:, :n]

    def release(self):
        _check(lib().gc_stream_batch_out_release(self.h), "gc_stream_batch_out_release")

    def stats(self):
        """(windows sealed, bytes per session, windows grown, GC_E_BUSY answers)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_batch_out_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_batch_out_stats")
        return tuple(int(x.value) for x in v)

    def split_stats(self):
        """(steps that touched more than one window, serialiser launches); zeros on an unsplit handle"""
        v = [C.c_uint64(0) for _ in range(2)]
        _check(lib().gc_stream_batch_out_split_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_batch_out_split_stats")
        return tuple(int(x.value) for x in v)

    def close(self):
        if self.h:
            lib().gc_stream_batch_out_free(self.h)
            self.h = None


class StreamEvalBatch:
    """gc_stream_eval_batch: the store of StreamEval and one OpCircuit block per call for S sessions of one program"""

    def __init__(self, ctx, sessions, d_keys, keylen):
        self.sessions = sessions
        st = C.c_int(0)
        self.h = lib().gc_stream_eval_batch_create(ctx.h, sessions, _dp(d_keys), keylen, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_eval_batch_create")

    def set_wires(self, ids, d_labels):
        """d_labels: device gc_label [S][len(ids)]; asynchronous"""
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        _check(lib().gc_stream_eval_batch_set_wires(self.h, _p(i), len(i), _dp(d_labels)), "gc_stream_eval_batch_set_wires")

    def set_fallback(self, on=True):
        """blocks whose circuit is loaded from now on and kept out of the keyed scope by the key table alone run on the HBM-wire
        kernels (circuit, circuit_host and the intake)"""
        _check(lib().gc_stream_eval_batch_set_fallback(self.h, 1 if on else 0), "gc_stream_eval_batch_set_fallback")

    def get(self, w):
        """LABEL [S]: the active label of global wire w in every session (waits for the ctx stream)"""
        out = np.zeros(self.sessions, LABEL)
        _check(lib().gc_stream_eval_batch_get_wire(self.h, w, _p(out)), "gc_stream_eval_batch_get_wire")
        return out

    def circuit(self, ngates, ntmp, nwires, ref_block, d_blocks, stride, d_bad):
        """one OpCircuit block of every session: ref_block = host bytes of any one session's block, d_blocks = all of them in
        device memory `stride` apart, d_bad = device u32 [S] (differing skeleton bytes per session); returns the bytes used"""
        b = np.frombuffer(bytes(ref_block), np.uint8) if len(ref_block) else np.zeros(1, np.uint8)
        n = C.c_size_t(0)
        _check(lib().gc_stream_eval_batch_circuit(self.h, ngates, ntmp, nwires, _p(b), len(ref_block), _dp(d_blocks), stride,
                                                  _dp(d_bad), C.byref(n)), "gc_stream_eval_batch_circuit")
        return n.value

    def circuit_host(self, ngates, ntmp, nwires, blocks, stride, length, ref_session=0):
        """one OpCircuit block of every session from HOST memory: blocks = the address of session 0's block (an int, e.g. a
        window's base + offset) or a numpy u8 array, session s's block `stride` bytes further; session ref_session's is the
        reference block.  Pinned memory must stay unchanged until uploads_wait() / bad() / close(); returns the bytes used"""
        addr = blocks if isinstance(blocks, int) else blocks.ctypes.data
        n = C.c_size_t(0)
        _check(lib().gc_stream_eval_batch_circuit_host(self.h, ngates, ntmp, nwires, C.c_void_p(addr), stride, length, ref_session,
                                                       C.byref(n)), "gc_stream_eval_batch_circuit_host")
        return n.value

    def uploads_wait(self):
        _check(lib().gc_stream_eval_batch_uploads_wait(self.h), "gc_stream_eval_batch_uploads_wait")

    def bad(self):
        """u32 [S]: differing structure bytes per session over every circuit_host since create (waits)"""
        out = np.zeros(self.sessions, np.uint32)
        _check(lib().gc_stream_eval_batch_bad(self.h, _p(out)), "gc_stream_eval_batch_bad")
        return out

    def return_labels(self, ids, labels_out=None):
        """OpReturn: the active label of wire ids[j] in every session as gc_label [S][len(ids)], what StreamBatch.decode reads.
        labels_out: a DeviceBuffer (gc_stream_eval_batch_return_labels_dev, asynchronous) or None, which returns LABEL
        [S, len(ids)] (gc_stream_eval_batch_return_labels, synchronous)"""
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        if isinstance(labels_out, DeviceBuffer):
            _check(lib().gc_stream_eval_batch_return_labels_dev(self.h, _p(i), len(i), _dp(labels_out)),
                   "gc_stream_eval_batch_return_labels_dev")
            return labels_out
        out = np.zeros((self.sessions, len(i)), LABEL)
        _check(lib().gc_stream_eval_batch_return_labels(self.h, _p(i), len(i), _p(out)), "gc_stream_eval_batch_return_labels")
        return out

    def return_labels_dev(self, ids, d_labels_out):
        return self.return_labels(ids, d_labels_out)

    def intake(self, ref_session=0, max_message_bytes=1 << 26):
        """a StreamEvalBatchIn of this handle: chunks of the S byte streams in, evaluated steps out; close it before this handle"""
        return StreamEvalBatchIn(self, ref_session, max_message_bytes)

    def cache_stats(self):
        """the circuit cache (gc_stream_eval_batch_cache_stats): (entries, device bytes, loads, evictions)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_eval_batch_cache_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_eval_batch_cache_stats")
        return tuple(int(x.value) for x in v)

    def close(self):
        if self.h:
            lib().gc_stream_eval_batch_free(self.h)
            self.h = None


class StreamEvalBatchIn:
    """gc_stream_eval_batch_in: the message loop of StreamEvaluator over S byte streams that arrive in chunks of any size.
    Every complete OpCircuit message is evaluated as StreamEvalBatch.circuit_host evaluates it; an unfinished one is kept."""

    def __init__(self, se, ref_session=0, max_message_bytes=1 << 26):
        self.sessions = se.sessions
        self.fed = 0  # bytes per session that feed() has taken
        st = C.c_int(0)
        self.h = lib().gc_stream_eval_batch_in_create(se.h, ref_session, max_message_bytes, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_stream_eval_batch_in_create")

    def feed(self, chunk, stride=None, length=None):
        """the next `length` bytes of every session: chunk = the address of session 0's bytes (an int, e.g. a window's base)
        with stride and length, or a numpy u8 array [S, length].  Returns (taken, next_op): next_op == 1 and taken == length
        while the messages are OpCircuit, else the op word the feed stopped in front of.  Raises EngineError with the
        parser's code for a refused message; self.taken then says where in the chunk it began"""
        if isinstance(chunk, int):
            addr = chunk
        else:
            if chunk.dtype != np.uint8 or chunk.ndim != 2 or chunk.shape[0] != self.sessions or chunk.strides[1] != 1:
                raise EngineError(GC_E_ARG, "feed: chunk must be u8 [sessions, length] with contiguous rows")
            addr, stride, length = chunk.ctypes.data, (chunk.strides[0] if self.sessions > 1 else chunk.shape[1]), chunk.shape[1]
        taken, op = C.c_size_t(0), C.c_uint32(0)
        rc = lib().gc_stream_eval_batch_in_feed(self.h, C.c_void_p(addr), stride, length, C.byref(taken), C.byref(op))
        self.taken = taken.value
        self.fed += taken.value
        _check(rc, "gc_stream_eval_batch_in_feed")
        return taken.value, op.value

    def word_bytes_taken(self):
        """after a stop or a refusal with taken == 0: the bytes of that word or message that earlier feeds took (and dropped)"""
        return self.fed - self.stats()[1]

    def stats(self):
        """(messages evaluated, their bytes per session, chunks uploaded, bytes per session kept over the feeds)"""
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().gc_stream_eval_batch_in_stats(self.h, *[C.byref(x) for x in v]), "gc_stream_eval_batch_in_stats")
        return tuple(int(x.value) for x in v)

    def close(self):
        if self.h:
            lib().gc_stream_eval_batch_in_free(self.h)
            self.h = None


# ---- multi-GPU (gc_comm_*: RCCL all-gather of the shards' outputs) ----------------------------

COMM_ID_BYTES = 128


def comm_available():
    return bool(lib().gc_comm_available())


def comm_version():
    """ncclGetVersion of the RCCL the library opened (0: no RCCL)"""
    return int(lib().gc_comm_version())


def comm_unique_id():
    """rank 0: the 128-byte ncclUniqueId the host hands to the other ranks"""
    buf = np.zeros(COMM_ID_BYTES, np.uint8)
    _check(lib().gc_comm_get_unique_id(_p(buf), len(buf)), "gc_comm_get_unique_id")
    return buf.tobytes()


class Comm:
    """gc_comm: one rank of the output gather (one ctx = one device)"""

    def __init__(self, ctx, uid, nranks, rank, _h=None):
        self.ctx = ctx
        if _h is not None:
            self.h = _h
        else:
            u = _u8(uid)
            st = C.c_int(0)
            self.h = lib().gc_comm_init_rank(ctx.h, _p(u), len(u), nranks, rank, C.byref(st))
            if not self.h:
                raise EngineError(st.value, "gc_comm_init_rank")
        self.rank = lib().gc_comm_rank(self.h)
        self.nranks = lib().gc_comm_nranks(self.h)

    @classmethod
    def init_all(cls, ctxs):
        """one process driving len(ctxs) devices (gc_comm_init_all)"""
        n = len(ctxs)
        hs = (C.c_void_p * n)(*[c.h for c in ctxs])
        out = (C.c_void_p * n)()
        _check(lib().gc_comm_init_all(hs, n, out), "gc_comm_init_all")
        return [cls(ctxs[i], None, n, i, _h=out[i]) for i in range(n)]

    def allgather(self, d_send, d_recv, nbytes):
        _check(lib().gc_comm_allgather(self.h, _dp(d_send), _dp(d_recv), nbytes), "gc_comm_allgather")

    @staticmethod
    def allgather_all(comms, d_sends, d_recvs, nbytes):
        n = len(comms)
        hs = (C.c_void_p * n)(*[c.h for c in comms])
        ss = (C.c_void_p * n)(*[_dp(x) for x in d_sends])
        rs = (C.c_void_p * n)(*[_dp(x) for x in d_recvs])
        _check(lib().gc_comm_allgather_all(hs, n, ss, rs, nbytes), "gc_comm_allgather_all")

    def allgather_host(self, local):
        """host array [rows, ...] -> [nranks, rows, ...]; staged through gc_dev_* buffers"""
        a = np.ascontiguousarray(local)
        d_in = DeviceBuffer(self.ctx, data=a)
        d_out = DeviceBuffer(self.ctx, a.nbytes * self.nranks)
        try:
            self.allgather(d_in.ptr, d_out.ptr, a.nbytes)
            return d_out.download(a.dtype, (self.nranks,) + a.shape)
        finally:
            d_in.close()
            d_out.close()

    def allreduce_max(self, value):
        v = C.c_double(value)
        _check(lib().gc_comm_allreduce_max(self.h, C.byref(v)), "gc_comm_allreduce_max")
        return v.value

    def barrier(self):
        _check(lib().gc_comm_barrier(self.h), "gc_comm_barrier")

    def close(self):
        if self.h:
            lib().gc_comm_destroy(self.h)
            self.h = None


# ---- OT -------------------------------------------------------------------------------------


def _lab1(x):
    a = np.zeros(1, LABEL)
    a[0] = (int(x[0]), int(x[1])) if isinstance(x, (tuple, list)) else (int(x["d0"]), int(x["d1"]))
    return a


class IKNPReceiver:
    """tail of NewIKNPReceiver + receive() (ot/iknp.go:347-356, 468-511)"""

    def __init__(self, ctx, base_wires):
        bw = np.ascontiguousarray(base_wires, dtype=WIRE)
        assert len(bw) == 128
        st = C.c_int(0)
        self.h = lib().gc_iknp_receiver_create(ctx.h, _p(bw), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_iknp_receiver_create")

    def receive(self, b):
        bb = np.ascontiguousarray(b, dtype=np.uint8)
        n = len(bb)
        u = np.zeros(max(lib().gc_iknp_u_bytes(n), 1), np.uint8)
        res = np.zeros(max(n, 1), LABEL)
        _check(lib().gc_iknp_receive(self.h, _p(bb), n, _p(u), _p(res)), "gc_iknp_receive")
        return u[: lib().gc_iknp_u_bytes(n)].tobytes(), res[:n]

    def receive_dev(self, d_choice_packed, n, d_u_out, d_labels_out):
        """device pointers (ints); asynchronous on the ctx stream"""
        _check(lib().gc_iknp_receive_dev(self.h, _dp(d_choice_packed), n, _dp(d_u_out), _dp(d_labels_out)), "gc_iknp_receive_dev")

    @property
    def last_ms(self):
        return float(lib().gc_iknp_last_ms(self.h))

    def receive_bits_dev(self, d_choices, n, d_u_out, d_result):
        _check(lib().gc_iknp_receive_bits_dev(self.h, _dp(d_choices), n, _dp(d_u_out), _dp(d_result)), "gc_iknp_receive_bits_dev")

    def receive_bits(self, choices, n):
        ch = np.ascontiguousarray(choices, dtype=np.uint64)
        u = np.zeros(max(lib().gc_iknp_u_bytes(n), 1), np.uint8)
        res = np.zeros(max((n + 63) // 64, 1), np.uint64)
        _check(lib().gc_iknp_receive_bits(self.h, _p(ch), n, _p(u), _p(res)), "gc_iknp_receive_bits")
        return u[: lib().gc_iknp_u_bytes(n)].tobytes(), res[: (n + 63) // 64]

    def close(self):
        if self.h:
            lib().gc_iknp_free(self.h)
            self.h = None


class IKNPSender:
    """tail of NewIKNPSender + send() (ot/iknp.go:104-122, 197-226)"""

    def __init__(self, ctx, delta, k0):
        k = np.ascontiguousarray(k0, dtype=LABEL)
        assert len(k) == 128
        d = _lab1(delta)
        st = C.c_int(0)
        self.h = lib().gc_iknp_sender_create(ctx.h, _p(d), _p(k), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_iknp_sender_create")

    def send(self, u, n):
        ub = np.frombuffer(bytes(u), np.uint8) if len(u) else np.zeros(1, np.uint8)
        res = np.zeros(max(n, 1), LABEL)
        _check(lib().gc_iknp_send(self.h, _p(ub), len(u), n, _p(res)), "gc_iknp_send")
        return res[:n]

    def send_dev(self, d_u_in, n, d_labels_out):
        """device pointers (ints); asynchronous on the ctx stream"""
        _check(lib().gc_iknp_send_dev(self.h, _dp(d_u_in), n, _dp(d_labels_out)), "gc_iknp_send_dev")

    @property
    def last_ms(self):
        return float(lib().gc_iknp_last_ms(self.h))

    def send_bits_dev(self, d_u_in, n, d_result):
        _check(lib().gc_iknp_send_bits_dev(self.h, _dp(d_u_in), n, _dp(d_result)), "gc_iknp_send_bits_dev")

    def send_bits(self, u, n):
        ub = np.frombuffer(bytes(u), np.uint8) if len(u) else np.zeros(1, np.uint8)
        res = np.zeros(max((n + 63) // 64, 1), np.uint64)
        _check(lib().gc_iknp_send_bits(self.h, _p(ub), len(u), n, _p(res)), "gc_iknp_send_bits")
        return res[: (n + 63) // 64]

    def close(self):
        if self.h:
            lib().gc_iknp_free(self.h)
            self.h = None


def mitccrh_hash(ctx, seed, gid0, blks, h):
    b = np.ascontiguousarray(blks, dtype=LABEL).copy()
    assert len(b) % h == 0
    s = _lab1(seed)
    _check(lib().gc_mitccrh_hash(ctx.h, _p(s), gid0, _p(b), len(b) // h, h), "gc_mitccrh_hash")
    return b


def cot_send_pads(ctx, seed, delta, data, wires):
    d = np.ascontiguousarray(data, dtype=LABEL)
    w = np.ascontiguousarray(wires, dtype=WIRE)
    out = np.zeros(max(2 * len(d), 1), LABEL)
    _check(lib().gc_cot_send_pads(ctx.h, _p(_lab1(seed)), _p(_lab1(delta)), _p(d), _p(w), len(d), _p(out)),
           "gc_cot_send_pads")
    return out[: 2 * len(d)]


def cot_send_pads_dev(ctx, seed, delta, d_data, d_wires, n, d_out):
    _check(lib().gc_cot_send_pads_dev(ctx.h, _p(_lab1(seed)), _p(_lab1(delta)), _dp(d_data), _dp(d_wires),
                                      n, _dp(d_out)), "gc_cot_send_pads_dev")


def cot_receive_unpad_dev(ctx, seed, d_flags, d_sent, d_result, n):
    _check(lib().gc_cot_receive_unpad_dev(ctx.h, _p(_lab1(seed)), _dp(d_flags), _dp(d_sent),
                                          _dp(d_result), n), "gc_cot_receive_unpad_dev")


def rot_send(ctx, seed, delta, data):
    """gc_rot_send: ROT.Send's pad loop (ot/rot.go:156-172) -> WIRE[n]"""
    d = np.ascontiguousarray(data, dtype=LABEL)
    out = np.zeros(max(len(d), 1), WIRE)
    _check(lib().gc_rot_send(ctx.h, _p(_lab1(seed)), _p(_lab1(delta)), _p(d) if len(d) else None, len(d), _p(out)),
           "gc_rot_send")
    return out[: len(d)]


def rot_receive(ctx, seed, result):
    """gc_rot_receive: ROT.Receive's pad loop (ot/rot.go:194-199)"""
    r = np.ascontiguousarray(result, dtype=LABEL).copy()
    _check(lib().gc_rot_receive(ctx.h, _p(_lab1(seed)), _p(r) if len(r) else None, len(r)), "gc_rot_receive")
    return r


def rot_send_dev(ctx, seed, delta, d_data, n, d_wires_out):
    _check(lib().gc_rot_send_dev(ctx.h, _p(_lab1(seed)), _p(_lab1(delta)), _dp(d_data), n, _dp(d_wires_out)), "gc_rot_send_dev")


def rot_receive_dev(ctx, seed, d_result, n):
    _check(lib().gc_rot_receive_dev(ctx.h, _p(_lab1(seed)), _dp(d_result), n), "gc_rot_receive_dev")


def cot_receive_unpad(ctx, seed, flags, sent, result):
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    s = np.ascontiguousarray(sent, dtype=LABEL)
    r = np.ascontiguousarray(result, dtype=LABEL).copy()
    _check(lib().gc_cot_receive_unpad(ctx.h, _p(_lab1(seed)), _p(f), _p(s), _p(r), len(f)), "gc_cot_receive_unpad")
    return r


def kos_receiver_tags(ctx, seed2, result, b, choice_vec, bcv):
    r = np.ascontiguousarray(result, dtype=LABEL)
    bb = np.ascontiguousarray(b, dtype=np.uint8)
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL)
    bc = np.ascontiguousarray(bcv, dtype=np.uint8)
    x, t0, t1 = np.zeros(1, LABEL), np.zeros(1, LABEL), np.zeros(1, LABEL)
    _check(lib().gc_kos_receiver_tags(ctx.h, _p(_lab1(seed2)), _p(r) if len(r) else None, _p(bb) if len(r) else None,
                                      len(r), _p(cv), _p(bc), _p(x), _p(t0), _p(t1)), "gc_kos_receiver_tags")
    f = lambda a: (int(a[0]["d0"]), int(a[0]["d1"]))
    return f(x), f(t0), f(t1)


def kos_receiver_tags_dev(ctx, seed2, d_result, d_b, n, choice_vec, bcv):
    """as kos_receiver_tags with the n labels / choice bytes in HBM (device pointers)"""
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL)
    bc = np.ascontiguousarray(bcv, dtype=np.uint8)
    x, t0, t1 = np.zeros(1, LABEL), np.zeros(1, LABEL), np.zeros(1, LABEL)
    _check(lib().gc_kos_receiver_tags_dev(ctx.h, _p(_lab1(seed2)), _dp(d_result), _dp(d_b), n, _p(cv), _p(bc),
                                          _p(x), _p(t0), _p(t1)), "gc_kos_receiver_tags_dev")
    f = lambda a: (int(a[0]["d0"]), int(a[0]["d1"]))
    return f(x), f(t0), f(t1)


def kos_sender_check_dev(ctx, seed2, d_result, n, choice_vec, delta, x, t0, t1):
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL)
    ok = C.c_int(0)
    _check(lib().gc_kos_sender_check_dev(ctx.h, _p(_lab1(seed2)), _dp(d_result), n, _p(cv), _p(_lab1(delta)),
                                         _p(_lab1(x)), _p(_lab1(t0)), _p(_lab1(t1)), C.byref(ok)), "gc_kos_sender_check_dev")
    return bool(ok.value)


def kos_sender_check(ctx, seed2, result, choice_vec, delta, x, t0, t1):
    r = np.ascontiguousarray(result, dtype=LABEL)
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL)
    ok = C.c_int(0)
    _check(lib().gc_kos_sender_check(ctx.h, _p(_lab1(seed2)), _p(r) if len(r) else None, len(r), _p(cv), _p(_lab1(delta)),
                                     _p(_lab1(x)), _p(_lab1(t0)), _p(_lab1(t1)), C.byref(ok)), "gc_kos_sender_check")
    return bool(ok.value)


# ---- GMW party engine (gmw/network.go, gmw/triples.go) ---------------------------------------


def gmw_plan_describe(gates, nwires, ninputs, noutputs):
    """host-only GMW plan (gc_gmw_plan_describe): (GmwInfo, level_of_gate, and_index_of_gate, words_of_level)"""
    g = np.ascontiguousarray(gates, dtype=GATE)
    info = GmwInfo()
    _check(lib().gc_gmw_plan_describe(_p(g) if len(g) else None, len(g), nwires, ninputs, noutputs, C.byref(info), None, None,
                                      None), "gc_gmw_plan_describe")
    lv = np.zeros(max(len(g), 1), np.uint32)
    ai = np.zeros(max(len(g), 1), np.uint32)
    wl = np.zeros(max(info.nlevels, 1), np.uint32)
    _check(lib().gc_gmw_plan_describe(_p(g) if len(g) else None, len(g), nwires, ninputs, noutputs, None, _p(lv), _p(ai), _p(wl)),
           "gc_gmw_plan_describe")
    return info, lv[: len(g)], ai[: len(g)], wl[: info.nlevels]


class Gmw:
    """One GMW party over `batch` instances (gc_gmw_*).  Buffers are u64 [words][batch] (word-major, instance inside);
    host forms take / return numpy arrays, *_dev forms take device pointers and run asynchronously on the ctx stream."""

    def __init__(self, ctx, circuit, nparties, party, batch):
        self.ctx, self.batch, self.nparties, self.party = ctx, batch, nparties, party
        g = np.ascontiguousarray(circuit.Gates, dtype=GATE)
        st = C.c_int(0)
        self.h = lib().gc_gmw_create(ctx.h, _p(g) if len(g) else None, len(g), circuit.NumWires, circuit.num_inputs,
                                     circuit.num_outputs, nparties, party, batch, C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_gmw_create")
        self.info = GmwInfo()
        _check(lib().gc_gmw_get_info(self.h, C.byref(self.info)), "gc_gmw_get_info")
        self.in_words = (self.info.ninputs + 63) // 64
        self.out_words = (self.info.noutputs + 63) // 64

    def set_inputs(self, inputs):
        a = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(self.in_words, self.batch)
        _check(lib().gc_gmw_set_inputs(self.h, _p(a) if a.size else None), "gc_gmw_set_inputs")

    def set_inputs_dev(self, d_inputs):
        _check(lib().gc_gmw_set_inputs_dev(self.h, _dp(d_inputs)), "gc_gmw_set_inputs_dev")

    def set_triples(self, a, b, c):
        arrs = [np.ascontiguousarray(x, dtype=np.uint64).reshape(self.info.triple_words, self.batch) for x in (a, b, c)]
        _check(lib().gc_gmw_set_triples(self.h, *[_p(x) if x.size else None for x in arrs]), "gc_gmw_set_triples")

    def set_triples_dev(self, d_a, d_b, d_c):
        _check(lib().gc_gmw_set_triples_dev(self.h, _dp(d_a), _dp(d_b), _dp(d_c)), "gc_gmw_set_triples_dev")

    def step(self, peer_msgs=None):
        """one exchange round (host form): peer_msgs [npeers][2][w][batch] of the pending level (None on the first step).
        Returns (level, msg [2][w][batch]); w == 0 (an empty msg) when the pass is complete."""
        npeers = self.nparties - 1
        pm = None if peer_msgs is None else np.ascontiguousarray(peer_msgs, dtype=np.uint64)
        out = np.zeros(2 * max(self.info.max_level_words, 1) * self.batch, np.uint64)
        lv, w = C.c_uint32(0), C.c_size_t(0)
        _check(lib().gc_gmw_step(self.h, _p(pm) if pm is not None and pm.size else None, npeers, _p(out), C.byref(lv),
                                 C.byref(w)), "gc_gmw_step")
        return lv.value, out[: 2 * w.value * self.batch].reshape(2, w.value, self.batch)

    def step_dev(self, d_peer_msgs, d_msg_out, npeers=None):
        """device form: returns (level, words)"""
        lv, w = C.c_uint32(0), C.c_size_t(0)
        _check(lib().gc_gmw_step_dev(self.h, None if d_peer_msgs is None else _dp(d_peer_msgs),
                                     self.nparties - 1 if npeers is None else npeers,
                                     None if d_msg_out is None else _dp(d_msg_out), C.byref(lv), C.byref(w)), "gc_gmw_step_dev")
        return lv.value, w.value

    def get_outputs(self):
        out = np.zeros(max(self.out_words * self.batch, 1), np.uint64)
        _check(lib().gc_gmw_get_outputs(self.h, _p(out)), "gc_gmw_get_outputs")
        return out[: self.out_words * self.batch].reshape(self.out_words, self.batch)

    def get_outputs_dev(self, d_out):
        _check(lib().gc_gmw_get_outputs_dev(self.h, _dp(d_out)), "gc_gmw_get_outputs_dev")

    @property
    def last_launches(self):
        return int(lib().gc_gmw_last_launches(self.h))

    def close(self):
        if self.h:
            lib().gc_gmw_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gmw_triples_local_dev(ctx, d_a, d_b, d_c, words):
    """c = a & b (triples.go:312-315)"""
    _check(lib().gc_gmw_triples_local_dev(ctx.h, _dp(d_a), _dp(d_b), _dp(d_c), words), "gc_gmw_triples_local_dev")


def gmw_triples_sender_u_dev(ctx, delta_bit, d_a, d_u, words):
    """u = a ^ (Delta.Bit(0) ? ~0 : 0) (triples.go:340-349)"""
    _check(lib().gc_gmw_triples_sender_u_dev(ctx.h, int(delta_bit) & 1, _dp(d_a), _dp(d_u), words), "gc_gmw_triples_sender_u_dev")


def gmw_triples_sender_fold_dev(ctx, d_s, d_u, d_v, d_c, words):
    """c ^= s ^ (u & v) (triples.go:362-364)"""
    _check(lib().gc_gmw_triples_sender_fold_dev(ctx.h, _dp(d_s), _dp(d_u), _dp(d_v), _dp(d_c), words),
           "gc_gmw_triples_sender_fold_dev")


def gmw_triples_receiver_fold_dev(ctx, d_r, d_c, words):
    """c ^= r (triples.go:387-389)"""
    _check(lib().gc_gmw_triples_receiver_fold_dev(ctx.h, _dp(d_r), _dp(d_c), words), "gc_gmw_triples_receiver_fold_dev")


# ---- VOLE over packed IKNP (vole/vole.go, vole/prg.go) ----------------------------------------


def vole_modulus(p):
    """the modulus as the ABI takes it: 32 bytes big-endian, from an int or from 32 bytes.  A p that does not fit 32 bytes
    is refused here (GC_E_ARG), as the library refuses an even p or p < 3."""
    if isinstance(p, (bytes, bytearray, memoryview, np.ndarray)):
        b = bytes(p)
        if len(b) != 32:
            raise EngineError(GC_E_ARG, "vole: the modulus takes 32 bytes, got %d" % len(b))
    else:
        p = int(p)
        if p < 0 or p >= 1 << 256:
            raise EngineError(GC_E_ARG, "vole: the modulus does not fit 32 bytes")
        b = p.to_bytes(32, "big")
    return np.frombuffer(b, np.uint8).copy()


def _v32(a):
    """values as the ABI takes them: uint8 [m, 32], element i = 32 bytes big-endian"""
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)


def vole_sender_mul(ctx, p, labels, x, y_msg):
    """gc_vole_sender_mul: (*Sender).Mul's per-label work (vole/vole.go:58-97) -> (r, u_msg), uint8 [m, 32] each"""
    lab = np.ascontiguousarray(labels, dtype=LABEL)
    xs, ys = _v32(x), _v32(y_msg)
    m = len(lab)
    assert len(xs) == m and len(ys) == m
    r, u = np.zeros((max(m, 1), 32), np.uint8), np.zeros((max(m, 1), 32), np.uint8)
    _check(lib().gc_vole_sender_mul(ctx.h, _p(vole_modulus(p)), _p(lab) if m else None, _p(xs) if m else None,
                                    _p(ys) if m else None, m, _p(r), _p(u)), "gc_vole_sender_mul")
    return r[:m], u[:m]


def vole_sender_mul_dev(ctx, p, d_labels, d_x, d_y_msg, m, d_r_out, d_u_msg_out):
    """device pointers; asynchronous on the ctx stream"""
    _check(lib().gc_vole_sender_mul_dev(ctx.h, _p(vole_modulus(p)), _dp(d_labels), _dp(d_x), _dp(d_y_msg), m, _dp(d_r_out),
                                        _dp(d_u_msg_out)), "gc_vole_sender_mul_dev")


def vole_receiver_reduce(ctx, p, u_msg):
    """gc_vole_receiver_reduce: (*Receiver).Mul's reduction (vole/vole.go:182-187) -> us, uint8 [m, 32]"""
    u = _v32(u_msg)
    m = len(u)
    out = np.zeros((max(m, 1), 32), np.uint8)
    _check(lib().gc_vole_receiver_reduce(ctx.h, _p(vole_modulus(p)), _p(u) if m else None, m, _p(out)),
           "gc_vole_receiver_reduce")
    return out[:m]


def vole_receiver_reduce_dev(ctx, p, d_u_msg, m, d_u_out):
    """device pointers; asynchronous on the ctx stream; d_u_out may be d_u_msg"""
    _check(lib().gc_vole_receiver_reduce_dev(ctx.h, _p(vole_modulus(p)), _dp(d_u_msg), m, _dp(d_u_out)),
           "gc_vole_receiver_reduce_dev")


# ---- Chou-Orlandi base OT on P-256 (ot/co.go, ot/co_helpers.go) --------------------------------


class CoPointError(EngineError):
    """GC_E_POINT of gc_co_sender_encrypt: .bad_index = the lowest index of a point that is not on the curve, .ct = the
    ciphertexts all the same (zeros at the bad points)"""

    def __init__(self, what, bad_index, ct):
        super().__init__(GC_E_POINT, what)
        self.bad_index, self.ct = bad_index, ct


def _b32(v):
    """a scalar as the ABI takes it: 32 bytes big-endian, from an int below 2^256 or from 32 bytes"""
    if isinstance(v, (bytes, bytearray, memoryview, np.ndarray)):
        b = bytes(v)
        if len(b) != 32:
            raise EngineError(GC_E_ARG, "co: a scalar takes 32 bytes, got %d" % len(b))
        return np.frombuffer(b, np.uint8).copy()
    v = int(v)
    if v < 0 or v >= 1 << 256:
        raise EngineError(GC_E_ARG, "co: the scalar does not fit 32 bytes")
    return np.frombuffer(v.to_bytes(32, "big"), np.uint8).copy()


def _scalars(a):
    """scalars as the ABI takes them: uint8 [n, 32] from such an array or from a sequence of ints"""
    if isinstance(a, np.ndarray):
        return _v32(a)
    a = list(a)
    if not a:
        return np.zeros((0, 32), np.uint8)
    return np.stack([_b32(v) for v in a])


def co_point(pt):
    """gc_p256_point (uint8 [64]) from 64 bytes or from an (x, y) pair of ints below 2^256"""
    if isinstance(pt, (tuple, list)):
        pt = int(pt[0]).to_bytes(32, "big") + int(pt[1]).to_bytes(32, "big")
    b = bytes(pt)
    if len(b) != 64:
        raise EngineError(GC_E_ARG, "co: a point takes 64 bytes, got %d" % len(b))
    return np.frombuffer(b, np.uint8).copy()


def _points(a):
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 64)
    a = list(a)
    if not a:
        return np.zeros((0, 64), np.uint8)
    return np.stack([co_point(p) for p in a])


def co_sender_setup(a):
    """gc_co_sender_setup (GenerateCOSenderSetup, ot/co_helpers.go:77-101) -> (A, AaInv), uint8 [64] each; host only"""
    A, ainv = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    _check(lib().gc_co_sender_setup(_p(_b32(a)), _p(A), _p(ainv)), "gc_co_sender_setup")
    return A, ainv


def co_sender_encrypt(ctx, a, AaInv, points, wires, id0=0):
    """gc_co_sender_encrypt (EncryptCOCiphertexts, :104-137) -> ct, uint8 [n, 2, 16]; raises CoPointError when a point is
    not on the curve"""
    pts = _points(points)
    w = np.ascontiguousarray(wires, dtype=WIRE)
    n = len(pts)
    assert len(w) == n
    ct = np.zeros((max(n, 1), 2, 16), np.uint8)
    bad = C.c_size_t(0)
    rc = lib().gc_co_sender_encrypt(ctx.h, _p(_b32(a)), _p(co_point(AaInv)), _p(pts) if n else None, _p(w) if n else None, n,
                                    id0, _p(ct), C.byref(bad))
    if rc == GC_E_POINT:
        raise CoPointError("gc_co_sender_encrypt", bad.value, ct[:n])
    _check(rc, "gc_co_sender_encrypt")
    return ct[:n]


def co_sender_encrypt_dev(ctx, a, AaInv, d_points, d_wires, n, id0, d_ct, d_status):
    """device pointers; asynchronous on the ctx stream; d_status: uint64 [2] = {bad points, lowest bad index}"""
    _check(lib().gc_co_sender_encrypt_dev(ctx.h, _p(_b32(a)), _p(co_point(AaInv)), _dp(d_points), _dp(d_wires), n, id0,
                                          _dp(d_ct), _dp(d_status)), "gc_co_sender_encrypt_dev")


def _choices(choice, n):
    c = np.ascontiguousarray(choice, dtype=np.uint8).reshape(-1)
    assert len(c) == n
    return c


def co_receiver_choices(ctx, A, scalars, choice):
    """gc_co_receiver_choices (BuildCOChoices, :140-177) -> points, uint8 [n, 64]"""
    sc = _scalars(scalars)
    n = len(sc)
    ch = _choices(choice, n)
    out = np.zeros((max(n, 1), 64), np.uint8)
    _check(lib().gc_co_receiver_choices(ctx.h, _p(co_point(A)), _p(sc) if n else None, _p(ch) if n else None, n, _p(out)),
           "gc_co_receiver_choices")
    return out[:n]


def co_receiver_choices_dev(ctx, A, d_scalars, d_choice, n, d_points_out):
    """device pointers; asynchronous on the ctx stream"""
    _check(lib().gc_co_receiver_choices_dev(ctx.h, _p(co_point(A)), _dp(d_scalars), _dp(d_choice), n, _dp(d_points_out)),
           "gc_co_receiver_choices_dev")


def co_receiver_decrypt(ctx, A, scalars, choice, ct, id0=0):
    """gc_co_receiver_decrypt (DecryptCOCiphertexts, :191-219) -> labels [n]"""
    sc = _scalars(scalars)
    n = len(sc)
    ch = _choices(choice, n)
    c = np.ascontiguousarray(ct, dtype=np.uint8).reshape(-1, 32)
    assert len(c) == n
    out = np.zeros(max(n, 1), LABEL)
    _check(lib().gc_co_receiver_decrypt(ctx.h, _p(co_point(A)), _p(sc) if n else None, _p(ch) if n else None,
                                        _p(c) if n else None, n, id0, _p(out)), "gc_co_receiver_decrypt")
    return out[:n]


def co_receiver_decrypt_dev(ctx, A, d_scalars, d_choice, d_ct, n, id0, d_labels_out):
    """device pointers; asynchronous on the ctx stream"""
    _check(lib().gc_co_receiver_decrypt_dev(ctx.h, _p(co_point(A)), _dp(d_scalars), _dp(d_choice), _dp(d_ct), n, id0,
                                            _dp(d_labels_out)), "gc_co_receiver_decrypt_dev")


class CoBase:
    """gc_co_base: the receiver's side of one session.  The handle checks A once and owns its fixed-base window table; the
    calls are co_receiver_choices / co_receiver_decrypt byte for byte, without their double-and-add ladder"""

    def __init__(self, ctx, A):
        st = C.c_int(0)
        self.ctx = ctx  # gc_co_base_free waits for this ctx's stream: the handle has to go first
        self.h = lib().gc_co_base_create(ctx.h, _p(co_point(A)), C.byref(st))
        if not self.h:
            raise EngineError(st.value, "gc_co_base_create")

    def choices(self, scalars, choice):
        """gc_co_base_choices -> points, uint8 [n, 64]"""
        sc = _scalars(scalars)
        n = len(sc)
        ch = _choices(choice, n)
        out = np.zeros((max(n, 1), 64), np.uint8)
        _check(lib().gc_co_base_choices(self.h, _p(sc) if n else None, _p(ch) if n else None, n, _p(out)), "gc_co_base_choices")
        return out[:n]

    def choices_dev(self, d_scalars, d_choice, n, d_points_out):
        """device pointers; asynchronous on the ctx stream"""
        _check(lib().gc_co_base_choices_dev(self.h, _dp(d_scalars), _dp(d_choice), n, _dp(d_points_out)), "gc_co_base_choices_dev")

    def decrypt(self, scalars, choice, ct, id0=0):
        """gc_co_base_decrypt -> labels [n]"""
        sc = _scalars(scalars)
        n = len(sc)
        ch = _choices(choice, n)
        c = np.ascontiguousarray(ct, dtype=np.uint8).reshape(-1, 32)
        assert len(c) == n
        out = np.zeros(max(n, 1), LABEL)
        _check(lib().gc_co_base_decrypt(self.h, _p(sc) if n else None, _p(ch) if n else None, _p(c) if n else None, n, id0,
                                        _p(out)), "gc_co_base_decrypt")
        return out[:n]

    def decrypt_dev(self, d_scalars, d_choice, d_ct, n, id0, d_labels_out):
        """device pointers; asynchronous on the ctx stream"""
        _check(lib().gc_co_base_decrypt_dev(self.h, _dp(d_scalars), _dp(d_choice), _dp(d_ct), n, id0, _dp(d_labels_out)),
               "gc_co_base_decrypt_dev")

    def close(self):
        if self.h:
            if self.ctx.h is None:  # the stream the free would wait for is gone with the ctx
                raise EngineError(GC_E_ARG, "CoBase.close: close the handle before its Context")
            lib().gc_co_base_free(self.h)
            self.h = None


# ---- several sessions per call (gc_co_multi_*): S sessions of `per` OTs each, session-major ----


class CoSessionError(EngineError):
    """a bad session of a gc_co_multi_* host call (GC_E_ARG from the sender calls, GC_E_POINT from the receiver calls):
    .bad_session = the lowest one, .out = the outputs all the same (zeros in the bad sessions), .bad_index = the lowest bad
    point's OT index when the sender met one as well, else None"""

    def __init__(self, code, what, bad_session, out, bad_index=None):
        super().__init__(code, what)
        self.bad_session, self.out, self.bad_index = bad_session, out, bad_index


def _multi(S, per, *arrays):
    S, per = int(S), int(per)
    n = S * per
    for a in arrays:
        assert len(a) == n, (len(a), S, per)
    return S, per, n


_NONE = C.c_size_t(-1).value  # what *bad_session and *bad_index hold when the call did not set them


def _bad(v):
    return None if v.value == _NONE else v.value


def co_multi_sender_setup(ctx, a):
    """gc_co_multi_sender_setup: a = S scalars -> (A, AaInv), uint8 [S, 64] each; raises CoSessionError (.out = (A, AaInv))
    when an a_s is 0 mod N"""
    sc = _scalars(a)
    S = len(sc)
    A, ainv = np.zeros((max(S, 1), 64), np.uint8), np.zeros((max(S, 1), 64), np.uint8)
    bad_s = C.c_size_t(_NONE)
    rc = lib().gc_co_multi_sender_setup(ctx.h, _p(sc) if S else None, S, _p(A), _p(ainv), C.byref(bad_s))
    if rc == GC_E_ARG and _bad(bad_s) is not None:
        raise CoSessionError(rc, "gc_co_multi_sender_setup", bad_s.value, (A[:S], ainv[:S]))
    _check(rc, "gc_co_multi_sender_setup")
    return A[:S], ainv[:S]


def co_multi_sender_setup_dev(ctx, d_a, S, d_A_out, d_AaInv_out, d_status):
    """device pointers; asynchronous on the ctx stream; d_status: uint64 [4] = {bad points, lowest bad OT index, bad
    sessions, lowest bad session}"""
    _check(lib().gc_co_multi_sender_setup_dev(ctx.h, _dp(d_a), S, _dp(d_A_out), _dp(d_AaInv_out), _dp(d_status)),
           "gc_co_multi_sender_setup_dev")


def co_multi_sender_encrypt(ctx, a, AaInv, points, wires, S, per, id0=0):
    """gc_co_multi_sender_encrypt -> ct, uint8 [S * per, 2, 16]; raises CoSessionError (.out = ct) when a session is bad,
    else CoPointError when a point is not on the curve"""
    sc, ai, pts = _scalars(a), _points(AaInv), _points(points)
    w = np.ascontiguousarray(wires, dtype=WIRE)
    S, per, n = _multi(S, per, pts, w)
    assert len(sc) == S and len(ai) == S
    ct = np.zeros((max(n, 1), 2, 16), np.uint8)
    bad, bad_s = C.c_size_t(_NONE), C.c_size_t(_NONE)
    rc = lib().gc_co_multi_sender_encrypt(ctx.h, _p(sc) if n else None, _p(ai) if n else None, _p(pts) if n else None,
                                          _p(w) if n else None, S, per, id0, _p(ct), C.byref(bad), C.byref(bad_s))
    if rc == GC_E_ARG and _bad(bad_s) is not None:
        raise CoSessionError(rc, "gc_co_multi_sender_encrypt", bad_s.value, ct[:n], _bad(bad))
    if rc == GC_E_POINT:
        raise CoPointError("gc_co_multi_sender_encrypt", bad.value, ct[:n])
    _check(rc, "gc_co_multi_sender_encrypt")
    return ct[:n]


def co_multi_sender_encrypt_dev(ctx, d_a, d_AaInv, d_points, d_wires, S, per, id0, d_ct, d_status):
    """device pointers, the session constants included; asynchronous on the ctx stream"""
    _check(lib().gc_co_multi_sender_encrypt_dev(ctx.h, _dp(d_a), _dp(d_AaInv), _dp(d_points), _dp(d_wires), S, per, id0,
                                                _dp(d_ct), _dp(d_status)), "gc_co_multi_sender_encrypt_dev")


def co_multi_receiver_choices(ctx, A, scalars, choice, S, per):
    """gc_co_multi_receiver_choices -> points, uint8 [S * per, 64]; raises CoSessionError (.out = points) when an A_s is not
    on the curve"""
    As, sc = _points(A), _scalars(scalars)
    S, per, n = _multi(S, per, sc)
    ch = _choices(choice, n)
    assert len(As) == S
    out = np.zeros((max(n, 1), 64), np.uint8)
    bad_s = C.c_size_t(_NONE)
    rc = lib().gc_co_multi_receiver_choices(ctx.h, _p(As) if n else None, _p(sc) if n else None, _p(ch) if n else None, S, per,
                                            _p(out), C.byref(bad_s))
    if rc == GC_E_POINT:
        raise CoSessionError(rc, "gc_co_multi_receiver_choices", _bad(bad_s), out[:n])
    _check(rc, "gc_co_multi_receiver_choices")
    return out[:n]


def co_multi_receiver_choices_dev(ctx, d_A, d_scalars, d_choice, S, per, d_points_out, d_status):
    """device pointers, the session constants included; asynchronous on the ctx stream"""
    _check(lib().gc_co_multi_receiver_choices_dev(ctx.h, _dp(d_A), _dp(d_scalars), _dp(d_choice), S, per, _dp(d_points_out),
                                                  _dp(d_status)), "gc_co_multi_receiver_choices_dev")


def co_multi_receiver_decrypt(ctx, A, scalars, choice, ct, S, per, id0=0):
    """gc_co_multi_receiver_decrypt -> labels [S * per]; raises CoSessionError (.out = labels) when an A_s is not on the
    curve"""
    As, sc = _points(A), _scalars(scalars)
    S, per, n = _multi(S, per, sc)
    ch = _choices(choice, n)
    c = np.ascontiguousarray(ct, dtype=np.uint8).reshape(-1, 32)
    assert len(As) == S and len(c) == n
    out = np.zeros(max(n, 1), LABEL)
    bad_s = C.c_size_t(_NONE)
    rc = lib().gc_co_multi_receiver_decrypt(ctx.h, _p(As) if n else None, _p(sc) if n else None, _p(ch) if n else None,
                                            _p(c) if n else None, S, per, id0, _p(out), C.byref(bad_s))
    if rc == GC_E_POINT:
        raise CoSessionError(rc, "gc_co_multi_receiver_decrypt", _bad(bad_s), out[:n])
    _check(rc, "gc_co_multi_receiver_decrypt")
    return out[:n]


def co_multi_receiver_decrypt_dev(ctx, d_A, d_scalars, d_choice, d_ct, S, per, id0, d_labels_out, d_status):
    """device pointers, the session constants included; asynchronous on the ctx stream"""
    _check(lib().gc_co_multi_receiver_decrypt_dev(ctx.h, _dp(d_A), _dp(d_scalars), _dp(d_choice), _dp(d_ct), S, per, id0,
                                                  _dp(d_labels_out), _dp(d_status)), "gc_co_multi_receiver_decrypt_dev")


class CoMultiBase:
    """gc_co_multi_base: the receiver's decrypt of S sessions.  The handle checks every A_s once and owns one fixed-base
    window table per good session, built on the device (61 440 bytes each); decrypt is co_multi_receiver_decrypt byte for
    byte, without its double-and-add ladder.  A: S points (host), or a device buffer of S gc_p256_point with S given"""

    def __init__(self, ctx, A, S=None):
        st = C.c_int(0)
        self.ctx = ctx  # gc_co_multi_base_free waits for this ctx's stream: the handle has to go first
        if S is None:
            As = _points(A)
            self.S = len(As)
            self.h = lib().gc_co_multi_base_create(ctx.h, _p(As) if self.S else None, self.S, C.byref(st))
            what = "gc_co_multi_base_create"
        else:
            self.S = int(S)
            self.h = lib().gc_co_multi_base_create_dev(ctx.h, _dp(A), self.S, C.byref(st))
            what = "gc_co_multi_base_create_dev"
        if not self.h:
            raise EngineError(st.value, what)

    def info(self):
        """gc_co_multi_base_info -> (S, bad sessions, the lowest bad session or None)"""
        S, bad, low = C.c_size_t(0), C.c_size_t(0), C.c_size_t(_NONE)
        _check(lib().gc_co_multi_base_info(self.h, C.byref(S), C.byref(bad), C.byref(low)), "gc_co_multi_base_info")
        return S.value, bad.value, _bad(low)

    def decrypt(self, scalars, choice, ct, per, id0=0):
        """gc_co_multi_base_decrypt -> labels [S * per]; raises CoSessionError (.out = labels) when an A_s was not on the
        curve"""
        sc = _scalars(scalars)
        S, per, n = _multi(self.S, per, sc)
        ch = _choices(choice, n)
        c = np.ascontiguousarray(ct, dtype=np.uint8).reshape(-1, 32)
        assert len(c) == n
        out = np.zeros(max(n, 1), LABEL)
        bad_s = C.c_size_t(_NONE)
        rc = lib().gc_co_multi_base_decrypt(self.h, _p(sc) if n else None, _p(ch) if n else None, _p(c) if n else None, per, id0,
                                            _p(out), C.byref(bad_s))
        if rc == GC_E_POINT:
            raise CoSessionError(rc, "gc_co_multi_base_decrypt", _bad(bad_s), out[:n])
        _check(rc, "gc_co_multi_base_decrypt")
        return out[:n]

    def decrypt_dev(self, d_scalars, d_choice, d_ct, per, id0, d_labels_out, d_status):
        """device pointers; asynchronous on the ctx stream; d_status: uint64 [4] as the gc_co_multi_*_dev calls fill it"""
        _check(lib().gc_co_multi_base_decrypt_dev(self.h, _dp(d_scalars), _dp(d_choice), _dp(d_ct), per, id0, _dp(d_labels_out),
                                                  _dp(d_status)), "gc_co_multi_base_decrypt_dev")

    def close(self):
        if self.h:
            if self.ctx.h is None:  # the stream the free would wait for is gone with the ctx
                raise EngineError(GC_E_ARG, "CoMultiBase.close: close the handle before its Context")
            lib().gc_co_multi_base_free(self.h)
            self.h = None


# ---- IKNP extension and COT pads for several sessions per call (gc_iknp_multi_*, gc_cot_multi_*) ----


class _IKNPMulti:
    """what the two roles of a gc_iknp_multi handle share"""

    h = None

    def _created(self, ctx, S, h, st, what):
        self.ctx = ctx  # gc_iknp_multi_free waits for this ctx's stream: the handle has to go first
        self.S = S
        self.h = h
        if not self.h:
            raise EngineError(st.value, what)

    def info(self):
        """gc_iknp_multi_info -> (S, receiver, pos)"""
        S, r, pos = C.c_size_t(0), C.c_int(0), C.c_uint64(0)
        _check(lib().gc_iknp_multi_info(self.h, C.byref(S), C.byref(r), C.byref(pos)), "gc_iknp_multi_info")
        return S.value, bool(r.value), pos.value

    @property
    def pos(self):
        return self.info()[2]

    def u_bytes(self, per):
        """bytes of the u-matrices of one call: S * gc_iknp_u_bytes(per)"""
        return self.S * lib().gc_iknp_u_bytes(per)

    def close(self):
        if self.h:
            if self.ctx.h is None:  # the stream the free would wait for is gone with the ctx
                raise EngineError(GC_E_ARG, "%s.close: close the handle before its Context" % type(self).__name__)
            lib().gc_iknp_multi_free(self.h)
            self.h = None


class IKNPMultiReceiver(_IKNPMulti):
    """gc_iknp_multi, receiver: S sessions of equal length per call, each byte for byte IKNPReceiver on that session alone.
    base: WIRE [S, 128] (host), or a device buffer of S * 128 gc_wire with S given"""

    def __init__(self, ctx, base, S=None):
        st = C.c_int(0)
        if S is None:
            bw = np.ascontiguousarray(base, dtype=WIRE).reshape(-1, 128)
            S = len(bw)
            h = lib().gc_iknp_multi_receiver_create(ctx.h, _p(bw) if S else None, S, C.byref(st))
            what = "gc_iknp_multi_receiver_create"
        else:
            S = int(S)
            h = lib().gc_iknp_multi_receiver_create_dev(ctx.h, _dp(base), S, C.byref(st))
            what = "gc_iknp_multi_receiver_create_dev"
        self._created(ctx, S, h, st, what)

    def receive(self, b, per):
        """b: one byte per OT, [S * per] session-major -> (u bytes of all sessions, labels [S * per])"""
        bb = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        S, per, n = _multi(self.S, per, bb)
        ub = self.u_bytes(per)
        u = np.zeros(max(ub, 1), np.uint8)
        res = np.zeros(max(n, 1), LABEL)
        _check(lib().gc_iknp_multi_receive(self.h, _p(bb) if n else None, per, _p(u), _p(res)), "gc_iknp_multi_receive")
        return u[:ub].tobytes(), res[:n]

    def receive_dev(self, d_choice_packed, per, d_u_out, d_labels_out):
        """device pointers; asynchronous on the ctx stream.  d_choice_packed: 64 * ceil(per / 512) bytes per session"""
        _check(lib().gc_iknp_multi_receive_dev(self.h, _dp(d_choice_packed), per, _dp(d_u_out), _dp(d_labels_out)),
               "gc_iknp_multi_receive_dev")

    def receive_bits(self, choices, per, stride=None):
        """bit-COT.  choices: u64 words, [S, W] (W = ceil(per / 64)) or, shared by all sessions, [W]; with `stride` given the
        flat words as they are, session s from word s * stride -> (u bytes of all sessions, result u64 [S, W])"""
        ch = np.ascontiguousarray(choices, dtype=np.uint64)
        per = int(per)
        W = (per + 63) // 64
        if stride is None:
            stride = 0 if ch.ndim == 1 else W
            assert ch.size == (W if ch.ndim == 1 else self.S * W)
        ch = ch.reshape(-1)
        ub = self.u_bytes(per)
        u = np.zeros(max(ub, 1), np.uint8)
        res = np.zeros(max(self.S * W, 1), np.uint64)
        _check(lib().gc_iknp_multi_receive_bits(self.h, _p(ch) if ch.size else None, stride, per, _p(u), _p(res)),
               "gc_iknp_multi_receive_bits")
        return u[:ub].tobytes(), res[:self.S * W].reshape(self.S, W)

    def receive_bits_dev(self, d_choices, stride, per, d_u_out, d_result):
        """device pointers; asynchronous on the ctx stream, one kernel.  d_choices: u64 words, session s from word
        s * stride (0: one vector for every session); d_result: u64 [S, ceil(per / 64)]"""
        _check(lib().gc_iknp_multi_receive_bits_dev(self.h, _dp(d_choices), stride, per, _dp(d_u_out), _dp(d_result)),
               "gc_iknp_multi_receive_bits_dev")


class IKNPMultiSender(_IKNPMulti):
    """gc_iknp_multi, sender: delta LABEL [S] and k0 LABEL [S, 128] (host), or device buffers of those with S given"""

    def __init__(self, ctx, delta, k0, S=None):
        st = C.c_int(0)
        if S is None:
            k = np.ascontiguousarray(k0, dtype=LABEL).reshape(-1, 128)
            d = np.ascontiguousarray(delta, dtype=LABEL).reshape(-1)
            S = len(k)
            assert len(d) == S
            h = lib().gc_iknp_multi_sender_create(ctx.h, _p(d) if S else None, _p(k) if S else None, S, C.byref(st))
            what = "gc_iknp_multi_sender_create"
        else:
            S = int(S)
            h = lib().gc_iknp_multi_sender_create_dev(ctx.h, _dp(delta), _dp(k0), S, C.byref(st))
            what = "gc_iknp_multi_sender_create_dev"
        self._created(ctx, S, h, st, what)

    def send(self, u, per):
        """u: the receiver's u bytes of all sessions -> labels [S * per]"""
        ub = np.frombuffer(bytes(u), np.uint8) if len(u) else np.zeros(1, np.uint8)
        n = self.S * int(per)
        res = np.zeros(max(n, 1), LABEL)
        _check(lib().gc_iknp_multi_send(self.h, _p(ub), len(u), per, _p(res)), "gc_iknp_multi_send")
        return res[:n]

    def send_dev(self, d_u_in, per, d_labels_out):
        """device pointers; asynchronous on the ctx stream"""
        _check(lib().gc_iknp_multi_send_dev(self.h, _dp(d_u_in), per, _dp(d_labels_out)), "gc_iknp_multi_send_dev")

    def send_bits(self, u, per):
        """bit-COT.  u: the receiver's u bytes of all sessions -> result u64 [S, ceil(per / 64)]"""
        ub = np.frombuffer(bytes(u), np.uint8) if len(u) else np.zeros(1, np.uint8)
        W = (int(per) + 63) // 64
        res = np.zeros(max(self.S * W, 1), np.uint64)
        _check(lib().gc_iknp_multi_send_bits(self.h, _p(ub), len(u), per, _p(res)), "gc_iknp_multi_send_bits")
        return res[:self.S * W].reshape(self.S, W)

    def send_bits_dev(self, d_u_in, per, d_result):
        """device pointers; asynchronous on the ctx stream, one kernel that reads column 0 of d_u_in only"""
        _check(lib().gc_iknp_multi_send_bits_dev(self.h, _dp(d_u_in), per, _dp(d_result)), "gc_iknp_multi_send_bits_dev")


def gmw_triples_multi_sender_u_dev(sender, d_a, d_u, words):
    """d_u [S, words] = d_a [words] ^ (Delta_s.Bit(0) ? ~0 : 0) for the S sessions of an IKNPMultiSender (triples.go:340-349)"""
    _check(lib().gc_gmw_triples_multi_sender_u_dev(sender.h, _dp(d_a), _dp(d_u), words), "gc_gmw_triples_multi_sender_u_dev")


def gmw_triples_multi_sender_fold_dev(ctx, d_s, d_u, d_v, d_c, S, words):
    """d_c [words] ^= XOR over s of (d_s[s] ^ (d_u[s] & d_v[s])), all [S, words] (triples.go:362-364)"""
    _check(lib().gc_gmw_triples_multi_sender_fold_dev(ctx.h, _dp(d_s), _dp(d_u), _dp(d_v), _dp(d_c), S, words),
           "gc_gmw_triples_multi_sender_fold_dev")


def gmw_triples_multi_receiver_fold_dev(ctx, d_r, d_c, S, words):
    """d_c [words] ^= XOR over s of d_r[s], [S, words] (triples.go:387-389)"""
    _check(lib().gc_gmw_triples_multi_receiver_fold_dev(ctx.h, _dp(d_r), _dp(d_c), S, words),
           "gc_gmw_triples_multi_receiver_fold_dev")


def cot_multi_send_pads(ctx, seeds, deltas, data, wires, S, per):
    """gc_cot_multi_send_pads: seeds, deltas LABEL [S]; data LABEL [S * per], wires WIRE [S * per] -> LABEL [S * per * 2]"""
    sd = np.ascontiguousarray(seeds, dtype=LABEL).reshape(-1)
    dl = np.ascontiguousarray(deltas, dtype=LABEL).reshape(-1)
    d = np.ascontiguousarray(data, dtype=LABEL).reshape(-1)
    w = np.ascontiguousarray(wires, dtype=WIRE).reshape(-1)
    S, per, n = _multi(S, per, d, w)
    assert len(sd) == S and len(dl) == S
    out = np.zeros(max(2 * n, 1), LABEL)
    _check(lib().gc_cot_multi_send_pads(ctx.h, _p(sd) if S else None, _p(dl) if S else None, _p(d) if n else None,
                                        _p(w) if n else None, S, per, _p(out)), "gc_cot_multi_send_pads")
    return out[: 2 * n]


def cot_multi_send_pads_dev(ctx, d_seeds, d_deltas, d_data, d_wires, S, per, d_out):
    """device pointers for every array, the seeds and deltas included; asynchronous on the ctx stream"""
    _check(lib().gc_cot_multi_send_pads_dev(ctx.h, _dp(d_seeds), _dp(d_deltas), _dp(d_data), _dp(d_wires), S, per, _dp(d_out)),
           "gc_cot_multi_send_pads_dev")


def cot_multi_receive_unpad(ctx, seeds, flags, sent, result, S, per):
    """gc_cot_multi_receive_unpad: seeds LABEL [S]; flags u8 [S * per], sent LABEL [S * per * 2], result LABEL [S * per] (the
    receiver's IKNP labels) -> the unpadded labels"""
    sd = np.ascontiguousarray(seeds, dtype=LABEL).reshape(-1)
    f = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    s = np.ascontiguousarray(sent, dtype=LABEL).reshape(-1)
    r = np.ascontiguousarray(result, dtype=LABEL).reshape(-1).copy()
    S, per, n = _multi(S, per, f, r)
    assert len(sd) == S and len(s) == 2 * n
    _check(lib().gc_cot_multi_receive_unpad(ctx.h, _p(sd) if S else None, _p(f) if n else None, _p(s) if n else None,
                                            _p(r) if n else None, S, per), "gc_cot_multi_receive_unpad")
    return r


def cot_multi_receive_unpad_dev(ctx, d_seeds, d_flags, d_sent, d_result, S, per):
    """device pointers; asynchronous on the ctx stream; d_result holds the IKNP labels on entry"""
    _check(lib().gc_cot_multi_receive_unpad_dev(ctx.h, _dp(d_seeds), _dp(d_flags), _dp(d_sent), _dp(d_result), S, per),
           "gc_cot_multi_receive_unpad_dev")


# ---- KOS check for several sessions per call (gc_kos_multi_*) ----


def kos_multi_receiver_tags(ctx, seed2, result, b, choice_vec, bcv, S, per):
    """gc_kos_multi_receiver_tags: seed2 LABEL [S]; result LABEL [S * per], b u8 [S * per]; choice_vec LABEL [S * 256], bcv u8
    [S * 256] -> tags LABEL [S, 3] (x, t0, t1 of every session)"""
    sd = np.ascontiguousarray(seed2, dtype=LABEL).reshape(-1)
    r = np.ascontiguousarray(result, dtype=LABEL).reshape(-1)
    bb = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL).reshape(-1)
    bc = np.ascontiguousarray(bcv, dtype=np.uint8).reshape(-1)
    S, per, n = _multi(S, per, r, bb)
    assert len(sd) == S and len(cv) == 256 * S and len(bc) == 256 * S
    tags = np.zeros((max(S, 1), 3), LABEL)
    _check(lib().gc_kos_multi_receiver_tags(ctx.h, _p(sd) if S else None, _p(r) if n else None, _p(bb) if n else None,
                                            _p(cv) if S else None, _p(bc) if S else None, S, per, _p(tags)),
           "gc_kos_multi_receiver_tags")
    return tags[:S]


def kos_multi_receiver_tags_dev(ctx, d_seed2, d_result, d_choice_packed, d_choice_vec, d_bcv_packed, S, per, d_tags_out):
    """device pointers for every array; asynchronous on the ctx stream.  d_choice_packed / d_bcv_packed: the packed choice
    buffers of the gc_iknp_multi_receive_dev calls at `per` and at 256"""
    _check(lib().gc_kos_multi_receiver_tags_dev(ctx.h, _dp(d_seed2), _dp(d_result), _dp(d_choice_packed), _dp(d_choice_vec),
                                                _dp(d_bcv_packed), S, per, _dp(d_tags_out)), "gc_kos_multi_receiver_tags_dev")


def kos_multi_sender_check(ctx, seed2, result, choice_vec, delta, tags, S, per):
    """gc_kos_multi_sender_check: seed2, delta LABEL [S]; result LABEL [S * per]; choice_vec LABEL [S * 256]; tags LABEL [S, 3]
    -> (ok u8 [S], lowest failing session or None)"""
    sd = np.ascontiguousarray(seed2, dtype=LABEL).reshape(-1)
    r = np.ascontiguousarray(result, dtype=LABEL).reshape(-1)
    cv = np.ascontiguousarray(choice_vec, dtype=LABEL).reshape(-1)
    dl = np.ascontiguousarray(delta, dtype=LABEL).reshape(-1)
    tg = np.ascontiguousarray(tags, dtype=LABEL).reshape(-1)
    S, per, n = _multi(S, per, r)
    assert len(sd) == S and len(dl) == S and len(cv) == 256 * S and len(tg) == 3 * S
    ok = np.zeros(max(S, 1), np.uint8)
    bad = C.c_size_t(0)
    _check(lib().gc_kos_multi_sender_check(ctx.h, _p(sd) if S else None, _p(r) if n else None, _p(cv) if S else None,
                                           _p(dl) if S else None, _p(tg) if S else None, S, per, _p(ok), C.byref(bad)),
           "gc_kos_multi_sender_check")
    return ok[:S], (None if not S or bad.value == C.c_size_t(-1).value else bad.value)


def kos_multi_sender_check_dev(ctx, d_seed2, d_result, d_choice_vec, d_delta, d_tags, S, per, d_ok, d_status):
    """device pointers; asynchronous on the ctx stream.  d_ok: [S] bytes; d_status: two uint64 {failed sessions, lowest
    failing session (all ones: none)}"""
    _check(lib().gc_kos_multi_sender_check_dev(ctx.h, _dp(d_seed2), _dp(d_result), _dp(d_choice_vec), _dp(d_delta), _dp(d_tags),
                                               S, per, _dp(d_ok), _dp(d_status)), "gc_kos_multi_sender_check_dev")


# ---- the sha2pc rounds for S sessions per call (gc_sha2pc_*) -----------------------------------------------------------------

SHA2PC_MAGIC, SHA2PC_CURVE, SHA2PC_SESSION, SHA2PC_SETUP, SHA2PC_POINT, SHA2PC_LABEL = 1, 2, 3, 4, 5, 6


class Sha2pcSessionError(EngineError):
    """a bad session of a gc_sha2pc_* host call: .bad_session = the lowest one, .verdict = u32 [S] (code | index << 8),
    .out = the outputs all the same (zeros in the bad sessions)"""

    def __init__(self, code, what, bad_session, verdict, out):
        super().__init__(code, what)
        self.bad_session, self.verdict, self.out = bad_session, verdict, out


def sha2pc_layout(plan_or_circ, ng, ne):
    """gc_sha2pc_layout / _layout_plan -> (len [3], lead [3], digest bytes) of Rounds 1 .. 3; a Plan needs no device"""
    ln, ld, db = (C.c_size_t * 3)(), (C.c_size_t * 3)(), C.c_size_t(0)
    if isinstance(plan_or_circ, DeviceCircuit):
        rc = lib().gc_sha2pc_layout(plan_or_circ.h, ng, ne, ln, ld, C.byref(db))
    else:
        rc = lib().gc_sha2pc_layout_plan(plan_or_circ.h if plan_or_circ is not None else None, ng, ne, ln, ld, C.byref(db))
    _check(rc, "gc_sha2pc_layout")
    return list(ln), list(ld), db.value


class _Sha2pc:
    """what the two handles share: geometry, the strides of device payload arrays, the verdict of a host call"""

    def __init__(self, dcirc, ng, ne, S, create, free, what):
        self.ctx, self.dc, self.ng, self.ne, self.S = dcirc.ctx, dcirc, int(ng), int(ne), int(S)
        self._free, self.h = free, None
        st = C.c_int(0)
        self.h = create(self.ctx.h, dcirc.h, ng, ne, S, C.byref(st))
        if not self.h:
            raise EngineError(st.value, what)
        self.len, self.lead, self.digest_bytes = sha2pc_layout(dcirc, ng, ne)
        self.stride = [(ld + ln + 15) // 16 * 16 for ln, ld in zip(self.len, self.lead)]

    def _host(self, rc, what, verdict, bad, out):
        if rc in (GC_E_ARG, GC_E_POINT) and _bad(bad) is not None:
            raise Sha2pcSessionError(rc, what, bad.value, verdict, out)
        _check(rc, what)
        return out

    def close(self):
        """free the handle BEFORE its circuit and its ctx; behind either the handle is dropped unfreed (its free would wait
        for a stream that is gone)"""
        if self.h and self.dc.h and self.ctx.h:
            self._free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bytes2(a, S, per):
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(S, -1)
    assert a.shape[1] == per, (a.shape, per)
    return a


class Sha2pcGarbler(_Sha2pc):
    """gc_sha2pc_garbler: GarblerRound1 / GarblerRound3 with EncodeRound1 / EncodeRound3 for S sessions per call"""

    def __init__(self, dcirc, ng, ne, S):
        super().__init__(dcirc, ng, ne, S, lib().gc_sha2pc_garbler_create, lib().gc_sha2pc_garbler_free,
                         "gc_sha2pc_garbler_create")

    def round1_dev(self, d_a, d_sid, d_A_out, d_AaInv_out, d_r1_out, stride1, d_verdict):
        _check(lib().gc_sha2pc_garbler_round1_dev(self.h, _dp(d_a), _dp(d_sid), _dp(d_A_out), _dp(d_AaInv_out), _dp(d_r1_out),
                                                  stride1, _dp(d_verdict)), "gc_sha2pc_garbler_round1_dev")

    def round3_dev(self, d_a, d_AaInv, d_sid, d_r2, stride2, d_keys, d_rnd, d_bits, d_r3_out, stride3, d_verdict):
        _check(lib().gc_sha2pc_garbler_round3_dev(self.h, _dp(d_a), _dp(d_AaInv), _dp(d_sid), _dp(d_r2), stride2, _dp(d_keys),
                                                  _dp(d_rnd), _dp(d_bits), _dp(d_r3_out), stride3, _dp(d_verdict)),
               "gc_sha2pc_garbler_round3_dev")

    def round1(self, a, sid):
        """a u8 [S, 32], sid u8 [S, 8] -> (A [S, 64], AaInv [S, 64], r1 [S, 80]); raises Sha2pcSessionError"""
        S = self.S
        a, sid = _bytes2(a, S, 32), _bytes2(sid, S, 8)
        A, ainv, r1 = np.zeros((S, 64), np.uint8), np.zeros((S, 64), np.uint8), np.zeros((S, self.len[0]), np.uint8)
        v, bad = np.zeros(S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_sha2pc_garbler_round1(self.h, _p(a), _p(sid), _p(A), _p(ainv), _p(r1), _p(v), C.byref(bad))
        return self._host(rc, "gc_sha2pc_garbler_round1", v, bad, (A, ainv, r1))

    def round3(self, a, AaInv, sid, r2, keys, rnd, bits):
        """packed r2 u8 [S, len2], keys [S, 32], rnd [S, 16 * (1 + ng + ne)], bits u8 [S, ng] -> r3 u8 [S, len3]"""
        S = self.S
        a, ai, sid, keys = _bytes2(a, S, 32), _bytes2(AaInv, S, 64), _bytes2(sid, S, 8), _bytes2(keys, S, 32)
        r2, rnd = _bytes2(r2, S, self.len[1]), _bytes2(rnd, S, 16 * (1 + self.ng + self.ne))
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(S, self.ng)
        r3 = np.zeros((S, self.len[2]), np.uint8)
        v, bad = np.zeros(S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_sha2pc_garbler_round3(self.h, _p(a), _p(ai), _p(sid), _p(r2), _p(keys), _p(rnd),
                                            _p(bits) if self.ng else None, _p(r3), _p(v), C.byref(bad))
        return self._host(rc, "gc_sha2pc_garbler_round3", v, bad, r3)


class Sha2pcEvaluator(_Sha2pc):
    """gc_sha2pc_evaluator: EvaluatorRound2 / EvaluatorRound4 with EncodeRound2 for S sessions per call"""

    def __init__(self, dcirc, ng, ne, S):
        super().__init__(dcirc, ng, ne, S, lib().gc_sha2pc_evaluator_create, lib().gc_sha2pc_evaluator_free,
                         "gc_sha2pc_evaluator_create")

    def round2_dev(self, d_r1, stride1, d_scalars, d_bits, d_A_out, d_sid_out, d_r2_out, stride2, d_verdict):
        _check(lib().gc_sha2pc_evaluator_round2_dev(self.h, _dp(d_r1), stride1, _dp(d_scalars), _dp(d_bits), _dp(d_A_out),
                                                    _dp(d_sid_out), _dp(d_r2_out), stride2, _dp(d_verdict)),
               "gc_sha2pc_evaluator_round2_dev")

    def round4_dev(self, d_A, d_sid, d_scalars, d_bits, d_r3, stride3, d_digest_out, d_verdict):
        _check(lib().gc_sha2pc_evaluator_round4_dev(self.h, _dp(d_A), _dp(d_sid), _dp(d_scalars), _dp(d_bits), _dp(d_r3),
                                                    stride3, _dp(d_digest_out), _dp(d_verdict)),
               "gc_sha2pc_evaluator_round4_dev")

    def round2(self, r1, scalars, bits):
        """packed r1 u8 [S, 80], scalars u8 [S, ne, 32], bits u8 [S, ne] -> (A [S, 64], sid [S, 8], r2 [S, len2])"""
        S = self.S
        r1, sc = _bytes2(r1, S, self.len[0]), _bytes2(scalars, S, 32 * self.ne)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(S, self.ne)
        A, sid, r2 = np.zeros((S, 64), np.uint8), np.zeros((S, 8), np.uint8), np.zeros((S, self.len[1]), np.uint8)
        v, bad = np.zeros(S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_sha2pc_evaluator_round2(self.h, _p(r1), _p(sc), _p(bits), _p(A), _p(sid), _p(r2), _p(v), C.byref(bad))
        return self._host(rc, "gc_sha2pc_evaluator_round2", v, bad, (A, sid, r2))

    def round4(self, A, sid, scalars, bits, r3):
        """packed r3 u8 [S, len3] -> digests u8 [S, digest_bytes]"""
        S = self.S
        A, sid, sc = _bytes2(A, S, 64), _bytes2(sid, S, 8), _bytes2(scalars, S, 32 * self.ne)
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(S, self.ne)
        r3 = _bytes2(r3, S, self.len[2])
        dg = np.zeros((S, self.digest_bytes), np.uint8)
        v, bad = np.zeros(S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_sha2pc_evaluator_round4(self.h, _p(A), _p(sid), _p(sc), _p(bits), _p(r3), _p(dg), _p(v), C.byref(bad))
        return self._host(rc, "gc_sha2pc_evaluator_round4", v, bad, dg)


# ---- circuit.Garbler / circuit.Evaluator for S sessions per call (gc_yao_*) ---------------------------------------------------

YAO_KEY, YAO_GATES, YAO_ROWS, YAO_LABEL, YAO_LENGTH = 1, 2, 3, 4, 5


class YaoSessionError(EngineError):
    """a bad session of a gc_yao_* host call: .bad_session = the lowest one, .verdict = u32 [S] (code | index << 8),
    .out = the outputs all the same (zeros in the bad sessions)"""

    def __init__(self, code, what, bad_session, verdict, out):
        super().__init__(code, what)
        self.bad_session, self.verdict, self.out = bad_session, verdict, out


def yao_layout(plan_or_circ, ng, ne, keylen):
    """gc_yao_layout / _layout_plan -> [len of M1, len of M2, slot bytes of M3]; a Plan needs no device"""
    ln = (C.c_size_t * 3)()
    if isinstance(plan_or_circ, DeviceCircuit):
        rc = lib().gc_yao_layout(plan_or_circ.h, ng, ne, keylen, ln)
    else:
        rc = lib().gc_yao_layout_plan(plan_or_circ.h if plan_or_circ is not None else None, ng, ne, keylen, ln)
    _check(rc, "gc_yao_layout")
    return list(ln)


def yao_kernel_shape():
    """gc_yao_kernel_shape -> (sessions per workgroup, bytes per piece) of the M1 kernels as create would choose them now"""
    tile, piece = C.c_uint32(0), C.c_uint32(0)
    _check(lib().gc_yao_kernel_shape(C.byref(tile), C.byref(piece)), "gc_yao_kernel_shape")
    return tile.value, piece.value


class _HandleBatch(Batch):
    """the gc_batch a gc_yao_* handle owns (path, form, last_ms): closing it leaves the batch to its handle"""

    def __init__(self, dcirc, batch, h):
        self.dc, self.batch, self.h = dcirc, batch, h

    def close(self):
        self.h = None


class _Yao:
    """what the two handles share: geometry, the strides of device message arrays, the verdict of a host call"""

    def __init__(self, dcirc, ng, ne, keylen, S, create, free, batch_of, what):
        self.ctx, self.dc, self.ng, self.ne, self.keylen, self.S = dcirc.ctx, dcirc, int(ng), int(ne), int(keylen), int(S)
        self._free, self.h = free, None
        st = C.c_int(0)
        self.h = create(self.ctx.h, dcirc.h, ng, ne, keylen, S, C.byref(st))
        if not self.h:
            raise EngineError(st.value, what)
        self.len = yao_layout(dcirc, ng, ne, keylen)
        self.stride = [(ln + 15) // 16 * 16 for ln in self.len]
        self.bits_bytes = self.len[2] - 4
        self.batch = _HandleBatch(dcirc, self.S, batch_of(self.h))

    def _host(self, rc, what, verdict, bad, out):
        if rc in (GC_E_ARG, GC_E_ROWS) and _bad(bad) is not None:
            raise YaoSessionError(rc, what, bad.value, verdict, out)
        _check(rc, what)
        return out

    def close(self):
        """free the handle BEFORE its circuit and its ctx; behind either the handle is dropped unfreed (its free would wait
        for a stream that is gone)"""
        if self.h and self.dc.h and self.ctx.h:
            self._free(self.h)
        self.h = None
        self.batch.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class YaoGarbler(_Yao):
    """gc_yao_garbler: circuit.Garbler's messages (circuit/garbler.go:38-180) for S sessions per call"""

    def __init__(self, dcirc, ng, ne, keylen, S):
        super().__init__(dcirc, ng, ne, keylen, S, lib().gc_yao_garbler_create, lib().gc_yao_garbler_free,
                         lib().gc_yao_garbler_batch, "gc_yao_garbler_create")

    def send_dev(self, d_keys, d_rnd, d_bits, d_m1_out, stride1):
        _check(lib().gc_yao_garbler_send_dev(self.h, _dp(d_keys), _dp(d_rnd), _dp(d_bits), _dp(d_m1_out), stride1),
               "gc_yao_garbler_send_dev")

    def ot_wires_dev(self, d_wires_out):
        _check(lib().gc_yao_garbler_ot_wires_dev(self.h, _dp(d_wires_out)), "gc_yao_garbler_ot_wires_dev")

    def result_dev(self, d_m2, stride2, d_m3_out, stride3, d_len3_out, d_bits_out, d_verdict):
        _check(lib().gc_yao_garbler_result_dev(self.h, _dp(d_m2), stride2, _dp(d_m3_out), stride3, _dp(d_len3_out),
                                               _dp(d_bits_out), _dp(d_verdict)), "gc_yao_garbler_result_dev")

    def send(self, keys, rnd, bits):
        """keys u8 [S, keylen], rnd u8 [S, 16 * (1 + ng + ne)], bits u8 [S, ng] -> packed M1 u8 [S, len1]"""
        S = self.S
        keys, rnd = _bytes2(keys, S, self.keylen), _bytes2(rnd, S, 16 * (1 + self.ng + self.ne))
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(S, self.ng)
        m1 = np.zeros((S, self.len[0]), np.uint8)
        _check(lib().gc_yao_garbler_send(self.h, _p(keys), _p(rnd), _p(bits) if self.ng else None, _p(m1)), "gc_yao_garbler_send")
        return m1

    def ot_wires(self):
        """-> WIRE [S, ne]: oti.Send's argument of every session"""
        w = np.zeros((self.S, self.ne), WIRE)
        _check(lib().gc_yao_garbler_ot_wires(self.h, _p(w)), "gc_yao_garbler_ot_wires")
        return w

    def result(self, m2):
        """packed M2 u8 [S, 16 nout] -> (M3 u8 [S, 4 + bits_bytes], len3 u32 [S], bits u8 [S, bits_bytes]); raises YaoSessionError"""
        S = self.S
        m2 = _bytes2(m2, S, self.len[1])
        m3, len3, bits = np.zeros((S, self.len[2]), np.uint8), np.zeros(S, np.uint32), np.zeros((S, self.bits_bytes), np.uint8)
        v, bad = np.zeros(S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_yao_garbler_result(self.h, _p(m2), _p(m3), _p(len3), _p(bits), _p(v), C.byref(bad))
        return self._host(rc, "gc_yao_garbler_result", v, bad, (m3, len3, bits))


class YaoEvaluator(_Yao):
    """gc_yao_evaluator: circuit.Evaluator's messages (circuit/evaluator.go:20-157) for S sessions per call"""

    def __init__(self, dcirc, ng, ne, keylen, S):
        super().__init__(dcirc, ng, ne, keylen, S, lib().gc_yao_evaluator_create, lib().gc_yao_evaluator_free,
                         lib().gc_yao_evaluator_batch, "gc_yao_evaluator_create")

    def accept_dev(self, d_m1, stride1, d_verdict):
        _check(lib().gc_yao_evaluator_accept_dev(self.h, _dp(d_m1), stride1, _dp(d_verdict)), "gc_yao_evaluator_accept_dev")

    def eval_dev(self, d_labels, d_m2_out, stride2, d_verdict):
        _check(lib().gc_yao_evaluator_eval_dev(self.h, _dp(d_labels), _dp(d_m2_out), stride2, _dp(d_verdict)),
               "gc_yao_evaluator_eval_dev")

    def result_dev(self, d_m3, stride3, d_bits_out, d_verdict):
        _check(lib().gc_yao_evaluator_result_dev(self.h, _dp(d_m3), stride3, _dp(d_bits_out), _dp(d_verdict)),
               "gc_yao_evaluator_result_dev")

    def accept(self, m1):
        """packed M1 u8 [S, len1] -> verdicts u32 [S] (all zero); raises YaoSessionError"""
        m1 = _bytes2(m1, self.S, self.len[0])
        v, bad = np.zeros(self.S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_yao_evaluator_accept(self.h, _p(m1), _p(v), C.byref(bad))
        return self._host(rc, "gc_yao_evaluator_accept", v, bad, v)

    def eval(self, labels):
        """labels LABEL [S, ne] from the OT -> packed M2 u8 [S, 16 nout]; raises YaoSessionError for a session accept found bad"""
        lab = np.ascontiguousarray(labels, dtype=LABEL).reshape(self.S, self.ne)
        m2 = np.zeros((self.S, self.len[1]), np.uint8)
        v, bad = np.zeros(self.S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_yao_evaluator_eval(self.h, _p(lab), _p(m2), _p(v), C.byref(bad))
        return self._host(rc, "gc_yao_evaluator_eval", v, bad, m2)

    def result(self, m3):
        """packed M3 u8 [S, 4 + bits_bytes] -> bits u8 [S, bits_bytes]; raises YaoSessionError"""
        m3 = _bytes2(m3, self.S, self.len[2])
        bits = np.zeros((self.S, self.bits_bytes), np.uint8)
        v, bad = np.zeros(self.S, np.uint32), C.c_size_t(_NONE)
        rc = lib().gc_yao_evaluator_result(self.h, _p(m3), _p(bits), _p(v), C.byref(bad))
        return self._host(rc, "gc_yao_evaluator_result", v, bad, bits)


# ---- device random streams: AES-CTR draws for S sessions per call (gc_rand_*) ----


def rand_kernel_shape():
    """(grid cap, threads per workgroup, blocks per wave and unit) of the fill kernel, from the sources the library was built
    from (csrc/kernels.h, rand_ctr.h): one sweep of the capped grid covers grid * threads blocks"""
    import re
    out = []
    for name, header in (("kRandGrid", "kernels.h"), ("kRandThreads", "kernels.h"), ("kRandRun", "rand_ctr.h")):
        with open(os.path.join(CSRC, header)) as f:
            m = re.findall(r"^\s*constexpr\s+(?:int|unsigned|uint32_t|size_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), re.M)
        if len(m) != 1:
            raise EngineError(GC_E_ARG, "%s: %d definitions of %s" % (header, len(m), name))
        out.append(int(m[0]))
    return tuple(out)


class RandSessionError(EngineError):
    """a bad session of a host-form cursor draw (GC_E_ARG): .bad_session = the lowest one, .out = the outputs all the same
    (a bad session's part as it came), .cur = the cursors (a bad session's unchanged)"""

    def __init__(self, what, bad_session, out, cur):
        super().__init__(GC_E_ARG, what)
        self.bad_session, self.out, self.cur = bad_session, out, cur


P256_N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551  # Chou-Orlandi draws its scalars below it


def _max32(mx):
    """the modulus of a scalar draw as gc_rand_scalars_cur* take it: 32 bytes big-endian"""
    mx = int(mx)
    if not 0 <= mx < 1 << 256:
        raise EngineError(GC_E_ARG, "RandStreams: max must lie below 2^256")
    return np.frombuffer(mx.to_bytes(32, "big"), np.uint8)


class RandStreams:
    """gc_rand: S AES-CTR keystreams, stream s what Go reads from cipher.StreamReader{cipher.NewCTR(aes.NewCipher(seed[s]),
    iv[s]), zeros}.  seeds: u8 [S, keylen] (host), ivs u8 [S, 16] or None (all zero); or device buffers of those with S and
    keylen given.  One byte position for all streams, or with the *_cur methods one per session in an array of the caller's
    (u64 [S]: device for the device forms, numpy for the _host forms); close the handle before its Context."""

    def __init__(self, ctx, seeds, ivs=None, S=None, keylen=None):
        st = C.c_int(0)
        if S is None:
            k = np.ascontiguousarray(seeds, dtype=np.uint8)
            assert k.ndim == 2, "seeds: [S, keylen]"
            S, keylen = k.shape
            v = None if ivs is None else np.ascontiguousarray(ivs, dtype=np.uint8).reshape(S, 16)
            h = lib().gc_rand_create(ctx.h, _p(k) if k.size else None, keylen, _p(v), S, C.byref(st))
            what = "gc_rand_create"
        else:
            S, keylen = int(S), int(keylen)
            h = lib().gc_rand_create_dev(ctx.h, _dp(seeds), keylen, None if ivs is None else _dp(ivs), S, C.byref(st))
            what = "gc_rand_create_dev"
        self.ctx, self.S, self.keylen, self.h = ctx, S, keylen, h  # gc_rand_free waits for this ctx's stream
        if not self.h:
            raise EngineError(st.value, what)

    def info(self):
        """gc_rand_info -> (S, keylen, pos)"""
        S, k, pos = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        _check(lib().gc_rand_info(self.h, C.byref(S), C.byref(k), C.byref(pos)), "gc_rand_info")
        return S.value, k.value, pos.value

    @property
    def pos(self):
        return self.info()[2]

    def seek(self, pos):
        _check(lib().gc_rand_seek(self.h, pos), "gc_rand_seek")

    def fill(self, nbytes, d_out, stride=None):
        """device pointer; asynchronous on the ctx stream, one kernel.  Stream s -> d_out + s * stride (default: nbytes)"""
        _check(lib().gc_rand_fill_dev(self.h, nbytes, _dp(d_out), nbytes if stride is None else stride), "gc_rand_fill_dev")

    def fill_host(self, nbytes, out=None, stride=None):
        """gc_rand_fill -> u8 [S, stride]; with `out` given (u8 [S, stride]) only the first nbytes of every row are written"""
        stride = nbytes if stride is None else stride
        if out is None:
            out = np.zeros((self.S, max(stride, 1)), np.uint8)[:, :stride]
            out = np.ascontiguousarray(out)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= self.S * stride
        _check(lib().gc_rand_fill(self.h, nbytes, _p(out) if out.size else None, stride), "gc_rand_fill")
        return out

    def gmw_shares(self, words, d_a, d_b):
        """tripleBatch's draws: u64 [S, words] each, a = BE64 of the first half of every 16-byte draw, b of the second"""
        _check(lib().gc_rand_gmw_shares_dev(self.h, words, _dp(d_a), _dp(d_b)), "gc_rand_gmw_shares_dev")

    def draw_garbler(self, ninputs, d_keys, d_rnd):
        """circuit.Garbler's order (garbler.go:47-53): the 32-byte key, then R and the input labels: the d_keys [S, 32] and
        d_rnd [S, 1 + ninputs, 16] of Batch.garble_keyed"""
        self.fill(32, d_keys)
        self.fill(16 * (1 + ninputs), d_rnd)

    # ---- per-session cursors: d_cur u64 [S] and d_status u64 [2] = {bad sessions, lowest bad session} on the device; every
    # call is asynchronous on the ctx stream, leaves .pos alone and may be captured ----

    def cur_set(self, d_cur, pos=0):
        """d_cur[s] = pos for every s"""
        _check(lib().gc_rand_cur_set_dev(self.h, _dp(d_cur), pos), "gc_rand_cur_set_dev")

    def fill_cur(self, d_cur, nbytes, d_out, d_status, stride=None):
        """bytes [cur[s], cur[s] + nbytes) of stream s -> d_out + s * stride (default: nbytes); cur[s] += nbytes"""
        _check(lib().gc_rand_fill_cur_dev(self.h, _dp(d_cur), nbytes, _dp(d_out), nbytes if stride is None else stride,
                                          _dp(d_status)), "gc_rand_fill_cur_dev")

    def scalars_cur(self, d_cur, mx, count, d_out, d_status):
        """`count` crand.Int(reader_s, mx) draws per session -> d_out u8 [S, count, 32] big-endian; mx a Python int"""
        _check(lib().gc_rand_scalars_cur_dev(self.h, _dp(d_cur), _p(_max32(mx)), count, _dp(d_out), _dp(d_status)),
               "gc_rand_scalars_cur_dev")

    def _cur_host(self, cur):
        cur = np.ascontiguousarray(cur, dtype=np.uint64).reshape(self.S).copy()
        return cur, C.c_size_t(_NONE)

    def fill_cur_host(self, cur, nbytes, out=None, stride=None):
        """gc_rand_fill_cur: cur u64 [S] -> (out u8 [S, stride], the new cursors); raises RandSessionError"""
        stride = nbytes if stride is None else stride
        if out is None:
            out = np.zeros((self.S, stride), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= self.S * stride
        cur, bad = self._cur_host(cur)
        rc = lib().gc_rand_fill_cur(self.h, _p(cur), nbytes, _p(out) if out.size else None, stride, C.byref(bad))
        if rc == GC_E_ARG and _bad(bad) is not None:
            raise RandSessionError("gc_rand_fill_cur", bad.value, out, cur)
        _check(rc, "gc_rand_fill_cur")
        return out, cur

    def scalars_cur_host(self, cur, mx, count, out=None):
        """gc_rand_scalars_cur: cur u64 [S] -> (out u8 [S, count, 32], the new cursors); raises RandSessionError"""
        if out is None:
            out = np.zeros((self.S, count, 32), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= self.S * count * 32
        cur, bad = self._cur_host(cur)
        rc = lib().gc_rand_scalars_cur(self.h, _p(cur), _p(_max32(mx)), count, _p(out) if out.size else None, C.byref(bad))
        if rc == GC_E_ARG and _bad(bad) is not None:
            raise RandSessionError("gc_rand_scalars_cur", bad.value, out, cur)
        _check(rc, "gc_rand_scalars_cur")
        return out, cur

    def draw_co_sender(self, d_cur, d_a, d_status):
        """GenerateCOSenderSetup's draw (ot/co_helpers.go:83): one crand.Int(rand, N) per session: the d_a [S, 32] of
        gc_co_multi_sender_setup_dev"""
        self.scalars_cur(d_cur, P256_N, 1, d_a, d_status)

    def draw_co_receiver(self, per, d_cur, d_scalars, d_status):
        """BuildCOChoices' draws (ot/co_helpers.go:150-151): `per` crand.Int(rand, N) one after the other per session: the
        d_scalars [S, per, 32] of gc_co_multi_receiver_choices_dev"""
        self.scalars_cur(d_cur, P256_N, per, d_scalars, d_status)

    def close(self):
        if self.h:
            if self.ctx.h is None:  # the stream the free would wait for is gone with the ctx
                raise EngineError(GC_E_ARG, "RandStreams.close: close the handle before its Context")
            lib().gc_rand_free(self.h)
            self.h = None
