"""ctypes binding of libldpc_hip.so (include/ldpc_hip.h).  The library is the product; there is
no Python or CPU fallback: if the shared object is missing or a call fails this module raises."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = (os.environ.get("LDPC_SO") or None) or os.path.join(HERE, "libldpc_hip.so")  # LDPC_SO: ablation builds (tools/)

OK, EINVAL, ENOMEM, EHIP, ENODEVICE, EUNSUPPORTED, EDEGREE, EFORMAT, ENOTFOUND = 0, -1, -2, -3, -4, -5, -6, -7, -8
TANH, MINSUM, TANH_CM, TANH_CUDA32 = 0, 1, 2, 3
F32, F64, F16, F16PK, I8 = 0, 1, 2, 3, 4
PATH_AUTO, PATH_FLOOD, PATH_FUSED = 0, 1, 2
SCHED_FLOODING, SCHED_LAYERED = 0, 1
SUM_REFERENCE, SUM_ARRAYLET, SUM_SPARSE = 0, 1, 2
BITS_BYTES, BITS_PACKED = 0, 1   # ldpc_bit_format
MOD_BPSK, MOD_QPSK, MOD_8PSK, MOD_16QAM = 1, 2, 3, 4
MOD_64QAM, MOD_256QAM, MOD_1024QAM, MOD_4096QAM = 6, 8, 10, 12   # product constellations: the kind number is m
DEMAP_MAXLOG, DEMAP_LOGMAP = 0, 1   # ldpc_demap_rule
LLR_F32, LLR_F16, LLR_I8 = 0, 1, 2   # LDPC_LLR_*: the output formats of the demapper
SOFT_POSTERIOR, SOFT_EXTRINSIC = 0, 1   # LDPC_SOFT_*: the kinds of ldpc_decode_batch_dev_soft
_SOFT_KINDS = {"posterior": SOFT_POSTERIOR, "extrinsic": SOFT_EXTRINSIC}
CN_MINSUM, CN_AMINSTAR = 0, 1   # ldpc_cn_rule
_CN_RULES = {None: CN_MINSUM, "minsum": CN_MINSUM, "aminstar": CN_AMINSTAR, CN_MINSUM: CN_MINSUM, CN_AMINSTAR: CN_AMINSTAR}


class CtxConfig(C.Structure):   # ldpc_ctx_config
    _fields_ = [("struct_size", C.c_size_t), ("device", C.c_int), ("variant", C.c_int), ("dtype", C.c_int), ("max_batch", C.c_int),
                ("path", C.c_int), ("schedule", C.c_int), ("sum_order", C.c_int), ("llr_qscale", C.c_float), ("cn_scale", C.c_float), ("cn_offset", C.c_float), ("cn_rule", C.c_int)]

class FadingStruct(C.Structure):   # ldpc_fading
    _fields_ = [("struct_size", C.c_size_t), ("block", C.c_int), ("k_factor", C.c_float)]


# every symbol include/ldpc_hip.h declares (tests/test_abi.py checks the library exports them all)
ABI_SYMBOLS = [
    "ldpc_init", "ldpc_decode_batch_dev_soft", "ldpc_decode_state_create", "ldpc_decode_state_destroy", "ldpc_decode_state_frames", "ldpc_decode_state_bytes", "ldpc_decode_state_reset", "ldpc_decode_batch_dev_continue", "ldpc_cascade_create", "ldpc_cascade_destroy", "ldpc_cascade_capacity", "ldpc_cascade_bytes", "ldpc_cascade_decode_dev", "ldpc_demap_dev_il_apriori", "ldpc_shutdown", "ldpc_current_device", "ldpc_ctx_create_on", "ldpc_sim_create_on", "ldpc_ctx_create_cfg", "ldpc_ctx_schedule", "ldpc_ctx_code", "ldpc_ctx_max_batch", "ldpc_ctx_device",
    "ldpc_batcher_create", "ldpc_batcher_destroy", "ldpc_batcher_decode_one", "ldpc_batcher_stats",
    "ldpc_ecc_create_replicas", "ldpc_ecc_replicas", "ldpc_ecc_ctx_at", "ldpc_ecc_sim_at", "ldpc_ecc_decode_on", "ldpc_ecc_set_coalescing", "ldpc_ecc_coalescing_stats", "ldpc_code_set_layers", "ldpc_code_layers", "ldpc_qc_layer_order", "ldpc_csr_layer_order", "ldpc_last_error", "ldpc_last_error_code", "ldpc_abi_version", "ldpc_device_count",
    "ldpc_code_create_qc", "ldpc_code_create_csr", "ldpc_code_destroy", "ldpc_code_dims", "ldpc_code_csr",
    "ldpc_ctx_create", "ldpc_ctx_create_ex", "ldpc_ctx_destroy", "ldpc_ctx_path", "ldpc_ctx_synchronize",
    "ldpc_decode_one", "ldpc_decode_batch", "ldpc_decode_batch_f64", "ldpc_decode_batch_dev",
    "ldpc_decode_batch_i8", "ldpc_decode_batch_dev_i8", "ldpc_ctx_llr_qscale", "ldpc_ctx_cn_scale", "ldpc_ctx_cn_offset", "ldpc_ctx_cn_rule",
    "ldpc_decode_batch_f16", "ldpc_decode_batch_dev_f16", "ldpc_sim_generate_f16", "ldpc_decode_batch_dev_packed", "ldpc_decode_batch_packed",
    "ldpc_debug_step", "ldpc_decode_trace",
    "ldpc_host_alloc", "ldpc_host_free",
    "ldpc_ctx_set_timing", "ldpc_ctx_kernel_time", "ldpc_ctx_kernel_name", "ldpc_ctx_kernel_geometry", "ldpc_jit_cache_dir", "ldpc_jit_source", "ldpc_jit_prepare", "ldpc_jit_source_for", "ldpc_jit_prepare_for",
    "ldpc_sim_create", "ldpc_sim_destroy", "ldpc_sim_generate", "ldpc_sim_tally", "ldpc_sim_encode_host",
    "ldpc_sim_create_qc_on", "ldpc_sim_encoder", "ldpc_sim_encode_batch", "ldpc_matrix_qc_words", "ldpc_matrix_rank",
    "ldpc_csr_triangular_order", "ldpc_sim_create_sparse_on",
    "ldpc_csr_systematic_form", "ldpc_sim_create_systematic_on", "ldpc_sim_message_length", "ldpc_sim_positions",
    "ldpc_sim_encode_messages", "ldpc_sim_generate_from", "ldpc_sim_extract_messages",
    "ldpc_modulation_create", "ldpc_modulation_create_builtin", "ldpc_modulation_destroy", "ldpc_modulation_bits", "ldpc_modulation_points", "ldpc_modulation_energy",
    "ldpc_modulation_symbols", "ldpc_modulation_create_product", "ldpc_modulation_axis_levels", "ldpc_modulation_with_rule", "ldpc_modulation_rule", "ldpc_demap_dev", "ldpc_sim_noise_var", "ldpc_sim_transmit", "ldpc_sim_generate_mod",
    "ldpc_interleaver_create_on", "ldpc_interleaver_destroy", "ldpc_interleaver_dims", "ldpc_interleaver_positions", "ldpc_interleaver_block_positions",
    "ldpc_demap_dev_il", "ldpc_sim_transmit_il", "ldpc_sim_generate_mod_il", "ldpc_interleave_bits_dev", "ldpc_deinterleave_llr_dev",
    "ldpc_demap_dev_il_csi", "ldpc_sim_transmit_il_fading", "ldpc_sim_generate_mod_il_fading",
    "ldpc_ratematch_create_on", "ldpc_ratematch_destroy", "ldpc_ratematch_dims", "ldpc_ratematch_positions", "ldpc_ratematch_fanin", "ldpc_ratematch_circular_positions",
    "ldpc_demap_dev_rm", "ldpc_ratematch_llr_dev", "ldpc_ratematch_bits_dev", "ldpc_sim_noise_var_rm", "ldpc_sim_transmit_rm",
    "ldpc_crc_builtin", "ldpc_crc_bits_host", "ldpc_crc_table", "ldpc_crc_create_on", "ldpc_crc_destroy", "ldpc_crc_params",
    "ldpc_crc_attach_dev", "ldpc_crc_check_dev", "ldpc_sim_crc_check", "ldpc_sim_tally_crc",
    "ldpc_bch_create_on", "ldpc_bch_destroy", "ldpc_bch_builtin", "ldpc_bch_params", "ldpc_bch_generator", "ldpc_bch_encode_host", "ldpc_bch_decode_host",
    "ldpc_bch_encode_dev", "ldpc_bch_decode_dev", "ldpc_sim_bch_decode",
    "ldpc_matrix_load", "ldpc_matrix_load_mackay", "ldpc_matrix_destroy", "ldpc_matrix_info", "ldpc_matrix_dense",
    "ldpc_matrix_qc_offsets", "ldpc_code_from_matrix",
    "ldpc_ecc_create", "ldpc_ecc_destroy", "ldpc_ecc_name", "ldpc_ecc_message_length", "ldpc_ecc_codeword_length",
    "ldpc_ecc_unpunctured_length", "ldpc_ecc_max_iters", "ldpc_ecc_encode", "ldpc_ecc_decode", "ldpc_ecc_ctx",
    "ldpc_ecc_sim", "ldpc_ecc_code",
]


class LdpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libldpc_hip error {code}: {msg}")
        self.code = code


_lib = None

# ---- deterministic teardown.  Every object that owns a native handle registers here; close_all() -- run by atexit,
# i.e. at the START of interpreter finalisation, while the HIP runtime and every module are still intact -- releases
# them in dependency order (records, replicas, frame sources, graphs, page-locked buffers).  After that, and whenever
# the interpreter is finalising, __del__ does nothing: no hipFree / hipStreamDestroy ever runs from a finaliser during
# shutdown, when the order against the HIP runtime's own exit handlers is not defined.
_live = weakref.WeakSet()
_CLOSE_ORDER = {"ECC": 0, "Batcher": 1, "DecodeState": 1, "Cascade": 1, "Decoder": 2, "Sim": 3, "Code": 4, "Matrix": 5, "PinnedArray": 6, "Modulation": 7, "Interleaver": 8}
_closed_all = False


def _register(obj):
    _live.add(obj)


def _finalizing():
    return _closed_all or sys is None or sys.is_finalizing()


def close_all():
    """Release every live native object now (idempotent).  Called automatically at interpreter exit."""
    for o in sorted(list(_live), key=lambda o: _CLOSE_ORDER.get(type(o).__name__, 9)):
        try:
            o.close()
        except Exception:
            pass


def _at_exit():
    global _closed_all
    close_all()
    _closed_all = True
    if _lib is not None:
        try:
            _lib.ldpc_shutdown()
        except Exception:
            pass


atexit.register(_at_exit)


def _preload_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch wheels bundle their own libamdhip64.so; if
    libldpc_hip.so pulled in /opt/rocm's copy first, a later `import torch` would bring up a second
    runtime that sees no GPUs.  So when a torch wheel is installed, load ITS runtime first (by file,
    without importing torch); libldpc_hip.so then binds to the already-loaded libamdhip64.so.N."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH) and "LDPC_SO" not in os.environ:
        # a fresh checkout (built artefacts are not in git): compile the product, never substitute for it
        try:
            import fcntl
            from . import build as _build
            # several ranks of one job may get here together on a fresh checkout: one builds, the others wait
            with open(os.path.join(HERE, ".build.lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if not os.path.exists(SO_PATH):
                    print(f"[ecc_ldpc_amd] {SO_PATH} missing: building it with hipcc", file=sys.stderr, flush=True)
                    _build.build(verbose=False)
        except Exception as e:
            raise ImportError(f"{SO_PATH} is missing and could not be built ({e}); run `python ecc_ldpc_amd/build.py` "
                              "(the HIP library is the only decode path; there is no fallback)") from e
    if not os.path.exists(SO_PATH):
        raise ImportError(f"{SO_PATH} is missing: build it with `python ecc_ldpc_amd/build.py` "
                          "(the HIP library is the only decode path; there is no fallback)")
    _preload_hip_runtime()
    L = C.CDLL(SO_PATH)
    vp, i32p, u8p, f64p, f32p, ip = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.ldpc_last_error.restype = C.c_char_p
    L.ldpc_init.argtypes = [C.c_int]
    L.ldpc_code_create_qc.restype = vp
    L.ldpc_code_create_qc.argtypes = [C.c_int, C.c_int, C.c_int, i32p]
    L.ldpc_code_create_csr.restype = vp
    L.ldpc_code_create_csr.argtypes = [C.c_int, C.c_int, i32p, i32p]
    L.ldpc_code_destroy.restype = None
    L.ldpc_code_destroy.argtypes = [vp]
    L.ldpc_code_dims.argtypes = [vp, ip, ip, ip]
    L.ldpc_code_csr.argtypes = [vp, i32p, i32p]
    L.ldpc_ctx_create.restype = vp
    L.ldpc_ctx_create.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.ldpc_ctx_create_ex.restype = vp
    L.ldpc_ctx_create_ex.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ldpc_ctx_create_on.restype = vp
    L.ldpc_ctx_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ldpc_ctx_create_cfg.restype = vp
    L.ldpc_ctx_create_cfg.argtypes = [vp, C.POINTER(CtxConfig)]
    L.ldpc_ctx_schedule.argtypes = [vp]
    L.ldpc_code_set_layers.argtypes = [vp, C.c_int, i32p]
    L.ldpc_qc_layer_order.argtypes = [C.c_int, C.c_int, i32p, C.c_int, i32p]
    L.ldpc_csr_layer_order.argtypes = [C.c_int, C.c_int, i32p, i32p, C.c_int, i32p, i32p]
    L.ldpc_code_layers.argtypes = [vp, ip, i32p]
    L.ldpc_sim_create_on.restype = vp
    L.ldpc_sim_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_int]
    L.ldpc_ctx_destroy.restype = None
    L.ldpc_ctx_destroy.argtypes = [vp]
    L.ldpc_ctx_path.argtypes = [vp]
    L.ldpc_ctx_synchronize.argtypes = [vp]
    L.ldpc_decode_one.argtypes = [vp, C.c_int, f64p, u8p, ip, ip]
    L.ldpc_decode_batch.argtypes = [vp, C.c_int, C.c_int, f32p, u8p, i32p, u8p]
    L.ldpc_decode_batch_f64.argtypes = [vp, C.c_int, C.c_int, f64p, u8p, i32p, u8p, f64p]
    L.ldpc_decode_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.ldpc_decode_batch_f16.argtypes = [vp, C.c_int, C.c_int, vp, u8p, i32p, u8p]
    L.ldpc_decode_batch_dev_f16.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.ldpc_decode_batch_i8.argtypes = [vp, C.c_int, C.c_int, vp, u8p, i32p, u8p]
    L.ldpc_decode_batch_dev_i8.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.ldpc_decode_batch_dev_soft.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp]
    L.ldpc_decode_state_create.restype = vp
    L.ldpc_decode_state_create.argtypes = [vp, C.c_int]
    L.ldpc_decode_state_destroy.restype = None
    L.ldpc_decode_state_destroy.argtypes = [vp]
    L.ldpc_decode_state_frames.argtypes = [vp]
    L.ldpc_decode_state_bytes.restype = C.c_size_t
    L.ldpc_decode_state_bytes.argtypes = [vp]
    L.ldpc_decode_state_reset.argtypes = [vp, C.c_int, C.c_int, vp]
    L.ldpc_cascade_create.restype = vp
    L.ldpc_cascade_create.argtypes = [vp, vp, C.c_int]
    L.ldpc_cascade_destroy.restype = None
    L.ldpc_cascade_destroy.argtypes = [vp]
    L.ldpc_cascade_capacity.argtypes = [vp]
    L.ldpc_cascade_bytes.restype = C.c_size_t
    L.ldpc_cascade_bytes.argtypes = [vp]
    L.ldpc_cascade_decode_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ldpc_decode_batch_dev_continue.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp]
    L.ldpc_ctx_llr_qscale.restype = C.c_float
    L.ldpc_ctx_llr_qscale.argtypes = [vp]
    L.ldpc_ctx_cn_scale.restype = C.c_float
    L.ldpc_ctx_cn_scale.argtypes = [vp]
    L.ldpc_ctx_cn_offset.restype = C.c_float
    L.ldpc_ctx_cn_offset.argtypes = [vp]
    L.ldpc_ctx_cn_rule.restype = C.c_int
    L.ldpc_ctx_cn_rule.argtypes = [vp]
    L.ldpc_decode_batch_dev_packed.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.ldpc_decode_batch_packed.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, u8p, i32p, u8p]
    L.ldpc_debug_step.argtypes = [vp, C.c_int, f64p, f64p, f64p, f64p, f64p, u8p]
    L.ldpc_decode_trace.argtypes = [vp, C.c_int, C.c_int, f64p, u8p, i32p, u8p, f64p]
    L.ldpc_host_alloc.restype = vp
    L.ldpc_host_alloc.argtypes = [C.c_size_t]
    L.ldpc_host_free.restype = None
    L.ldpc_host_free.argtypes = [vp]
    L.ldpc_ctx_set_timing.argtypes = [vp, C.c_int]
    L.ldpc_ctx_kernel_time.argtypes = [vp, ip, f64p]
    L.ldpc_ctx_kernel_name.restype = C.c_char_p
    L.ldpc_ctx_kernel_name.argtypes = [vp]
    L.ldpc_ctx_kernel_geometry.argtypes = [vp, ip, ip]
    L.ldpc_jit_cache_dir.restype = C.c_char_p
    L.ldpc_jit_source.restype = C.c_long
    L.ldpc_jit_source.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.ldpc_jit_prepare.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t, ip, f64p]
    L.ldpc_jit_source_for.restype = C.c_long
    L.ldpc_jit_source_for.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.ldpc_jit_prepare_for.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, ip, f64p]
    L.ldpc_sim_create.restype = vp
    L.ldpc_sim_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, u8p, C.c_int]
    L.ldpc_sim_destroy.restype = None
    L.ldpc_sim_destroy.argtypes = [vp]
    L.ldpc_sim_generate.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, vp, vp]
    L.ldpc_sim_generate_f16.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, vp, vp]
    L.ldpc_sim_tally.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.ldpc_sim_encode_host.argtypes = [vp, u8p, u8p]
    L.ldpc_sim_create_qc_on.restype = vp
    L.ldpc_sim_create_qc_on.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int]
    L.ldpc_sim_encoder.argtypes = [vp]
    L.ldpc_csr_triangular_order.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p]
    L.ldpc_sim_create_sparse_on.restype = vp
    L.ldpc_sim_create_sparse_on.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.ldpc_csr_systematic_form.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p, i32p, ip, ip, u8p]
    L.ldpc_sim_create_systematic_on.restype = vp
    L.ldpc_sim_create_systematic_on.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.ldpc_sim_message_length.argtypes = [vp]
    L.ldpc_sim_positions.argtypes = [vp, i32p, i32p]
    L.ldpc_sim_encode_batch.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp, vp]
    L.ldpc_sim_encode_messages.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_sim_generate_from.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_sim_extract_messages.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
    L.ldpc_modulation_create.restype = vp
    L.ldpc_modulation_create.argtypes = [C.c_int, C.POINTER(C.c_float)]
    L.ldpc_modulation_create_builtin.restype = vp
    L.ldpc_modulation_create_builtin.argtypes = [C.c_int]
    L.ldpc_modulation_destroy.restype = None
    L.ldpc_modulation_destroy.argtypes = [vp]
    L.ldpc_modulation_bits.argtypes = [vp]
    L.ldpc_modulation_points.argtypes = [vp, C.POINTER(C.c_float)]
    L.ldpc_modulation_energy.restype = C.c_double
    L.ldpc_modulation_energy.argtypes = [vp]
    L.ldpc_modulation_symbols.argtypes = [vp, C.c_int]
    L.ldpc_modulation_create_product.restype = vp
    L.ldpc_modulation_create_product.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ldpc_modulation_axis_levels.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ldpc_modulation_with_rule.restype = vp
    L.ldpc_modulation_with_rule.argtypes = [vp, C.c_int]
    L.ldpc_modulation_rule.argtypes = [vp]
    L.ldpc_demap_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_double, vp, C.c_int, C.c_float, vp]
    L.ldpc_sim_noise_var.restype = C.c_double
    L.ldpc_sim_noise_var.argtypes = [vp, vp, C.c_double]
    L.ldpc_sim_transmit.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, vp, vp]
    L.ldpc_sim_generate_mod.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int, C.c_float, vp, vp]
    L.ldpc_interleaver_create_on.restype = vp
    L.ldpc_interleaver_create_on.argtypes = [C.c_int, C.c_int, C.c_int, i32p]
    L.ldpc_interleaver_destroy.restype = None
    L.ldpc_interleaver_destroy.argtypes = [vp]
    L.ldpc_interleaver_dims.argtypes = [vp, ip, ip]
    L.ldpc_interleaver_positions.argtypes = [vp, i32p]
    L.ldpc_interleaver_block_positions.argtypes = [C.c_int, C.c_int, i32p, i32p, i32p]
    L.ldpc_demap_dev_il.argtypes = [vp, vp, C.c_int, vp, C.c_double, vp, C.c_int, C.c_float, vp]
    L.ldpc_sim_transmit_il.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, vp, vp]
    L.ldpc_sim_generate_mod_il.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int, C.c_float, vp, vp]
    L.ldpc_interleave_bits_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_deinterleave_llr_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
    L.ldpc_demap_dev_il_csi.argtypes = [vp, vp, C.c_int, vp, vp, C.c_double, vp, C.c_int, C.c_float, vp]
    L.ldpc_demap_dev_il_apriori.argtypes = [vp, vp, C.c_int, vp, vp, C.c_double, vp, vp, C.c_int, C.c_float, vp]
    L.ldpc_sim_transmit_il_fading.argtypes = [vp, vp, vp, C.POINTER(FadingStruct), C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, vp, vp, vp]
    L.ldpc_sim_generate_mod_il_fading.argtypes = [vp, vp, vp, C.POINTER(FadingStruct), C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int, C.c_float, vp, vp, vp]
    L.ldpc_ratematch_create_on.restype = vp
    L.ldpc_ratematch_create_on.argtypes = [C.c_int, C.c_int, C.c_int, i32p]
    L.ldpc_ratematch_destroy.restype = None
    L.ldpc_ratematch_destroy.argtypes = [vp]
    L.ldpc_ratematch_dims.argtypes = [vp, ip, ip]
    L.ldpc_ratematch_positions.argtypes = [vp, i32p]
    L.ldpc_ratematch_fanin.argtypes = [vp, i32p]
    L.ldpc_ratematch_circular_positions.argtypes = [C.c_int, i32p, C.c_int, C.c_int, i32p]
    L.ldpc_demap_dev_rm.argtypes = [vp, vp, C.c_int, vp, vp, C.c_double, vp, C.c_int, C.c_float, C.c_int, vp]
    L.ldpc_ratematch_llr_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_int, vp]
    L.ldpc_ratematch_bits_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_sim_noise_var_rm.restype = C.c_double
    L.ldpc_sim_noise_var_rm.argtypes = [vp, vp, vp, C.c_double]
    L.ldpc_sim_transmit_rm.argtypes = [vp, vp, vp, C.POINTER(FadingStruct), C.c_uint64, C.c_uint64, C.c_int, C.c_double, vp, C.c_int, vp, vp, vp, vp]
    u32p = C.POINTER(C.c_uint32)
    L.ldpc_crc_builtin.argtypes = [C.c_int, ip, u32p, u32p, u32p]
    L.ldpc_crc_bits_host.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, u8p, u32p]
    L.ldpc_crc_table.argtypes = [C.c_int, C.c_uint32, C.c_int, u32p]
    L.ldpc_crc_create_on.restype = vp
    L.ldpc_crc_create_on.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.ldpc_crc_destroy.restype = None
    L.ldpc_crc_destroy.argtypes = [vp]
    L.ldpc_crc_params.argtypes = [vp, ip, u32p, u32p, u32p, ip]
    L.ldpc_crc_attach_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_crc_check_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.ldpc_sim_crc_check.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.ldpc_sim_tally_crc.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.ldpc_bch_create_on.restype = vp
    L.ldpc_bch_create_on.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int]
    L.ldpc_bch_destroy.restype = None
    L.ldpc_bch_destroy.argtypes = [vp]
    L.ldpc_bch_builtin.argtypes = [C.c_int, ip, u32p, ip]
    L.ldpc_bch_params.argtypes = [vp, ip, u32p, ip, ip, ip]
    L.ldpc_bch_generator.argtypes = [vp, u8p]
    L.ldpc_bch_encode_host.argtypes = [vp, u8p]
    L.ldpc_bch_decode_host.argtypes = [vp, u8p, ip]
    L.ldpc_bch_encode_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.ldpc_bch_decode_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.ldpc_sim_bch_decode.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.ldpc_matrix_qc_words.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.ldpc_matrix_rank.argtypes = [vp]
    L.ldpc_matrix_load.restype = vp
    L.ldpc_matrix_load.argtypes = [C.c_char_p, C.c_char_p]
    L.ldpc_matrix_load_mackay.restype = vp
    L.ldpc_matrix_load_mackay.argtypes = [C.c_char_p]
    L.ldpc_matrix_destroy.restype = None
    L.ldpc_matrix_destroy.argtypes = [vp]
    L.ldpc_matrix_info.argtypes = [vp, ip, ip, ip, ip, ip]
    L.ldpc_matrix_dense.argtypes = [vp, u8p]
    L.ldpc_matrix_qc_offsets.argtypes = [vp, i32p]
    L.ldpc_code_from_matrix.restype = vp
    L.ldpc_code_from_matrix.argtypes = [vp]
    L.ldpc_ecc_create.restype = vp
    L.ldpc_ecc_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.ldpc_ecc_create_replicas.restype = vp
    L.ldpc_ecc_create_replicas.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, ip]
    L.ldpc_ecc_replicas.argtypes = [vp]
    L.ldpc_ecc_ctx_at.restype = vp
    L.ldpc_ecc_ctx_at.argtypes = [vp, C.c_int]
    L.ldpc_ecc_sim_at.restype = vp
    L.ldpc_ecc_sim_at.argtypes = [vp, C.c_int]
    L.ldpc_ecc_decode_on.argtypes = [vp, C.c_int, f64p, u8p, ip]
    L.ldpc_ecc_set_coalescing.argtypes = [vp, C.c_int, C.c_int]
    L.ldpc_ecc_coalescing_stats.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.ldpc_ctx_code.restype = vp
    L.ldpc_ctx_code.argtypes = [vp]
    L.ldpc_ctx_max_batch.argtypes = [vp]
    L.ldpc_ctx_device.argtypes = [vp]
    L.ldpc_batcher_create.restype = vp
    L.ldpc_batcher_create.argtypes = [vp, C.c_int, C.c_int]
    L.ldpc_batcher_destroy.restype = None
    L.ldpc_batcher_destroy.argtypes = [vp]
    L.ldpc_batcher_decode_one.argtypes = [vp, C.c_int, f64p, u8p, ip, ip]
    L.ldpc_batcher_stats.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.ldpc_ecc_destroy.restype = None
    L.ldpc_ecc_destroy.argtypes = [vp]
    L.ldpc_ecc_name.restype = C.c_char_p
    L.ldpc_ecc_name.argtypes = [vp]
    for f in ("message_length", "codeword_length", "unpunctured_length", "max_iters"):
        getattr(L, "ldpc_ecc_" + f).argtypes = [vp]
    L.ldpc_ecc_encode.argtypes = [vp, u8p, u8p]
    L.ldpc_ecc_decode.argtypes = [vp, f64p, u8p, ip]
    L.ldpc_ecc_ctx.restype = vp
    L.ldpc_ecc_ctx.argtypes = [vp]
    L.ldpc_ecc_sim.restype = vp
    L.ldpc_ecc_sim.argtypes = [vp]
    L.ldpc_ecc_code.restype = vp
    L.ldpc_ecc_code.argtypes = [vp]
    _lib = L
    return L


def last_error() -> str:
    return lib().ldpc_last_error().decode(errors="replace")


def check(rc):
    if rc != OK:
        raise LdpcError(rc, last_error())


def ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


class PinnedArray:
    """numpy view of page-locked host memory from ldpc_host_alloc (freed with the object)."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib().ldpc_host_alloc(self.nbytes)
        if not self._p:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        buf = (C.c_char * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)
        _register(self)

    def close(self):
        if self._p:
            self.array = None
            lib().ldpc_host_free(self._p)
            self._p = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def init(device: int = 0):
    check(lib().ldpc_init(int(device)))


_VARIANTS = {"tanh": TANH, "min": MINSUM, "minsum": MINSUM, "min-sum": MINSUM, "cm": TANH_CM, "tanh-cm": TANH_CM, TANH: TANH, MINSUM: MINSUM,
             TANH_CM: TANH_CM, "cuda32": TANH_CUDA32, "cuda-arraylet2": TANH_CUDA32, TANH_CUDA32: TANH_CUDA32}
_DTYPES = {"f32": F32, "f64": F64, "f16": F16, "f16pk": F16PK, "i8": I8, F32: F32, F64: F64, F16: F16, F16PK: F16PK, I8: I8}
_PATHS = {"auto": PATH_AUTO, "flood": PATH_FLOOD, "fused": PATH_FUSED, 0: 0, 1: 1, 2: 2}
_SUM_ORDERS = {"reference": SUM_REFERENCE, "arraylet": SUM_ARRAYLET, "sparse": SUM_SPARSE, 0: 0, 1: 1, 2: 2}
_SCHEDULES = {"flooding": SCHED_FLOODING, "flood": SCHED_FLOODING, "layered": SCHED_LAYERED, 0: 0, 1: 1}


class Code:
    """Parity-check graph handle (ldpc_code)."""

    def __init__(self, handle, owned=True):
        if not handle:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = handle
        self._owned = owned
        _register(self)
        M, N, E = C.c_int(), C.c_int(), C.c_int()
        check(lib().ldpc_code_dims(self._h, C.byref(M), C.byref(N), C.byref(E)))
        self.M, self.N, self.E = M.value, N.value, E.value

    @classmethod
    def from_qc(cls, sz, offsets):
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        assert off.ndim == 2
        return cls(lib().ldpc_code_create_qc(int(sz), off.shape[0], off.shape[1], ptr(off, C.c_int32)))

    @staticmethod
    def qc_layer_order(offsets, run=4):
        """-> (perm, full_runs): an order of the block rows in which runs of up to `run` consecutive rows share no block column
        (ldpc_qc_layer_order; offsets[perm] is the matrix to hand to from_qc for the layered schedule)"""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        perm = np.zeros(off.shape[0], np.int32)
        n = lib().ldpc_qc_layer_order(off.shape[0], off.shape[1], ptr(off, C.c_int32), int(run), ptr(perm, C.c_int32))
        if n < 0:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        return perm, n

    @staticmethod
    def csr_layer_order(row_ptr, col_idx, N, max_rows=0):
        """-> (perm, layer_ptr): an order of the rows of any H in which consecutive rows form few column-disjoint layers
        (ldpc_csr_layer_order; the rows perm of H are the matrix to hand to from_csr, layer_ptr what its set_layers takes)"""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        M = max(len(rp) - 1, 0)
        perm = np.zeros(max(M, 1), np.int32)
        lp = np.zeros(M + 1, np.int32)
        n = lib().ldpc_csr_layer_order(M, int(N), ptr(rp, C.c_int32), ptr(ci, C.c_int32), int(max_rows), ptr(perm, C.c_int32), ptr(lp, C.c_int32))
        if n < 0:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        return perm[:M], lp[: n + 1]

    @staticmethod
    def csr_triangular_order(row_ptr, col_idx, N):
        """-> order: order[j] = the row of H whose largest column is K + j, K = N - M (ldpc_csr_triangular_order): in that order the
        parity part of H is unit lower-triangular and H encodes by back-substitution (Sim(..., from_H=True)).  LdpcError -5, naming
        the offending row or rows, for an H that does not qualify"""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        M = max(len(rp) - 1, 0)
        order = np.zeros(max(M, 1), np.int32)
        check(lib().ldpc_csr_triangular_order(M, int(N), ptr(rp, C.c_int32), ptr(ci, C.c_int32), ptr(order, C.c_int32)))
        return order[:M]

    @staticmethod
    def csr_systematic_form(row_ptr, col_idx, N, want_P=True):
        """-> (msg_pos [K], par_pos [rank], P [K][rank] uint8 or None): the systematic form of any H (ldpc_csr_systematic_form) --
        columns taken from the right, a column is a parity position iff it is independent of the parity positions after it;
        c[msg_pos[i]] = m[i], c[par_pos[j]] = XOR_i m[i] P[i][j].  LdpcError -5 for M * N > 2^28 and for a code without message bits"""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        M, N = max(len(rp) - 1, 0), int(N)
        mp, pp = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32)
        K, r = C.c_int(0), C.c_int(0)
        check(lib().ldpc_csr_systematic_form(M, N, ptr(rp, C.c_int32), ptr(ci, C.c_int32), ptr(mp, C.c_int32), ptr(pp, C.c_int32), C.byref(K), C.byref(r), None))
        P = None
        if want_P:
            P = np.zeros((K.value, r.value), np.uint8)
            check(lib().ldpc_csr_systematic_form(M, N, ptr(rp, C.c_int32), ptr(ci, C.c_int32), ptr(mp, C.c_int32), ptr(pp, C.c_int32), C.byref(K), C.byref(r),
                                                 ptr(P, C.c_uint8)))
        return mp[:K.value].copy(), pp[:r.value].copy(), P

    @staticmethod
    def permute_rows(row_ptr, col_idx, perm):
        """-> (row_ptr, col_idx) of H with its rows in the order perm (perm[i] = the row put at place i)"""
        rp = np.asarray(row_ptr, np.int64)
        ci = np.asarray(col_idx, np.int32)
        deg = np.diff(rp)[perm]
        nrp = np.zeros(len(perm) + 1, np.int32)
        nrp[1:] = np.cumsum(deg)
        nci = np.concatenate([ci[rp[m]:rp[m + 1]] for m in perm]).astype(np.int32) if len(perm) else ci[:0]
        return nrp, nci

    @classmethod
    def from_csr(cls, row_ptr, col_idx, N):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        return cls(lib().ldpc_code_create_csr(len(rp) - 1, int(N), ptr(rp, C.c_int32), ptr(ci, C.c_int32)))

    @classmethod
    def from_dense(cls, H):
        H = np.asarray(H)
        M, N = H.shape
        rp = np.zeros(M + 1, np.int32)
        rp[1:] = np.cumsum(H.astype(bool).sum(1))
        ci = np.nonzero(H)[1].astype(np.int32)
        return cls.from_csr(rp, ci, N)

    def csr(self):
        rp = np.zeros(self.M + 1, np.int32)
        ci = np.zeros(self.E, np.int32)
        check(lib().ldpc_code_csr(self._h, ptr(rp, C.c_int32), ptr(ci, C.c_int32)))
        return rp, ci

    def set_layers(self, layer_ptr):
        lp = np.ascontiguousarray(layer_ptr, dtype=np.int32)
        check(lib().ldpc_code_set_layers(self._h, len(lp) - 1, ptr(lp, C.c_int32)))

    def layers(self):
        n = C.c_int()
        check(lib().ldpc_code_layers(self._h, C.byref(n), None))
        lp = np.zeros(n.value + 1, np.int32)
        check(lib().ldpc_code_layers(self._h, C.byref(n), ptr(lp, C.c_int32)))
        return lp

    def jit_source(self, variant="min", dtype="f32", schedule="flooding") -> str:
        """the translation unit the run-time compiler would be given for this code (LdpcError -5 if there is none)"""
        sch = _SCHEDULES[schedule]
        n = lib().ldpc_jit_source_for(self._h, _VARIANTS[variant], _DTYPES[dtype], sch, None, 0)
        if n < 0:
            raise LdpcError(int(n), last_error())
        buf = C.create_string_buffer(n + 1)
        lib().ldpc_jit_source_for(self._h, _VARIANTS[variant], _DTYPES[dtype], sch, buf, n + 1)
        return buf.value.decode()

    def jit_prepare(self, variant="min", dtype="f32", schedule="flooding"):
        """compile this code's specialised kernel into the disk cache (no GPU needed) -> (kernel name, from_cache, seconds)"""
        name = C.create_string_buffer(128)
        fc, sec = C.c_int(), C.c_double()
        check(lib().ldpc_jit_prepare_for(self._h, _VARIANTS[variant], _DTYPES[dtype], _SCHEDULES[schedule], name, 128, C.byref(fc), C.byref(sec)))
        return name.value.decode(), bool(fc.value), sec.value

    @classmethod
    def from_matrix(cls, matrix: "Matrix"):
        return cls(lib().ldpc_code_from_matrix(matrix._h))

    def close(self):
        if self._h and self._owned:
            lib().ldpc_code_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Decoder:
    """One decoder replica (ldpc_ctx): the object behind the reference's per-frame closure."""

    def __init__(self, code: Code, variant="min", dtype="f32", max_batch=64, path="auto", _handle=None, device=None, schedule="flooding",
                 sum_order="reference", qscale=None, cn_scale=None, cn_offset=None, cn_rule=None):
        """sum_order: "reference" | "arraylet" | "sparse" -- the column-sum order of that family of the reference's decoders
        (ldpc_sum_order: parity modes, flood path); qscale: the quantiser's scale of dtype "i8" (None: the library's default, 4);
        cn_scale, cn_offset: the check-node rule |msg'| = max(cn_scale * min - cn_offset, 0) of layered min-sum with dtype "f16", "f32"
        or "i8" on the on-chip kernel for any H (None: the 3/4 of every other kernel, and no offset); cn_rule: None or "minsum" for that,
        "aminstar" for the A-min* check-node rule of the same kernel (dtype "f16" or "f32"; it has no scale and no offset)"""
        self.code = code
        self.max_batch = int(max_batch)
        self._owned = _handle is None
        if _handle is not None:
            self._h = _handle
        elif device is None and _SCHEDULES[schedule] == SCHED_FLOODING and _SUM_ORDERS[sum_order] == SUM_REFERENCE and qscale is None and cn_scale is None and cn_offset is None and _CN_RULES[cn_rule] == CN_MINSUM:
            self._h = lib().ldpc_ctx_create_ex(code._h, _VARIANTS[variant], _DTYPES[dtype], int(max_batch), _PATHS[path])
        else:   # explicit device (replicas of one code on several GPUs of this process) and/or the layered schedule
            cfg = CtxConfig(C.sizeof(CtxConfig), -1 if device is None else int(device), _VARIANTS[variant], _DTYPES[dtype], int(max_batch),
                            _PATHS[path], _SCHEDULES[schedule], _SUM_ORDERS[sum_order], 0.0 if qscale is None else float(qscale),
                            0.0 if cn_scale is None else float(cn_scale), 0.0 if cn_offset is None else float(cn_offset), _CN_RULES[cn_rule])
            self._h = lib().ldpc_ctx_create_cfg(code._h, C.byref(cfg))
        if not self._h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        _register(self)
        self.path = {PATH_FLOOD: "flood", PATH_FUSED: "fused"}[lib().ldpc_ctx_path(self._h)]
        self.schedule = {SCHED_FLOODING: "flooding", SCHED_LAYERED: "layered"}[lib().ldpc_ctx_schedule(self._h)]
        self.qscale = float(lib().ldpc_ctx_llr_qscale(self._h))    # 0.0 unless dtype "i8"

    @property
    def cn_scale(self):
        """the scale of the min-sum check-node rule this context computes with (an "i8" context: a / 16); 0.0 on a tanh context"""
        return float(lib().ldpc_ctx_cn_scale(self._h))

    @property
    def cn_rule(self):
        """"aminstar" on a context of the A-min* check-node rule, "minsum" on every other"""
        return {CN_MINSUM: "minsum", CN_AMINSTAR: "aminstar"}[lib().ldpc_ctx_cn_rule(self._h)]

    @property
    def cn_offset(self):
        """the offset of that rule in LLR units (an "i8" context: b / qscale)"""
        return float(lib().ldpc_ctx_cn_offset(self._h))

    def decode_one(self, llr, max_iters):
        llr = np.ascontiguousarray(llr, np.float64)
        assert llr.shape == (self.code.N,)
        bits = np.zeros(self.code.N, np.uint8)
        it, cv = C.c_int(), C.c_int()
        check(lib().ldpc_decode_one(self._h, int(max_iters), ptr(llr, C.c_double), ptr(bits, C.c_uint8), C.byref(it), C.byref(cv)))
        return bits, it.value, bool(cv.value)

    def decode_batch(self, llr, max_iters, want_lam=False, out_bits=None):
        """llr [F][N] float16, float32 or float64 (host); int8 on an "i8" decoder.  -> bits [F][N], iters [F], converged [F] (, lam)"""
        llr = np.asarray(llr)
        F = llr.shape[0]
        assert llr.shape == (F, self.code.N)
        bits = out_bits if out_bits is not None else np.zeros((F, self.code.N), np.uint8)
        assert bits.shape == (F, self.code.N) and bits.dtype == np.uint8 and bits.flags.c_contiguous
        iters = np.zeros(F, np.int32)
        conv = np.zeros(F, np.uint8)
        if llr.dtype == np.int8:
            assert not want_lam, "final LLRs come with float64 input (ldpc_decode_batch_f64)"
            llr = np.ascontiguousarray(llr)
            check(lib().ldpc_decode_batch_i8(self._h, int(max_iters), F, llr.ctypes.data_as(C.c_void_p), ptr(bits, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8)))
            return bits, iters, conv
        if llr.dtype == np.float16 and not want_lam:
            llr = np.ascontiguousarray(llr)
            check(lib().ldpc_decode_batch_f16(self._h, int(max_iters), F, llr.ctypes.data_as(C.c_void_p), ptr(bits, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8)))
            return bits, iters, conv
        if llr.dtype == np.float32 and not want_lam:
            llr = np.ascontiguousarray(llr)
            check(lib().ldpc_decode_batch(self._h, int(max_iters), F, ptr(llr, C.c_float), ptr(bits, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8)))
            return bits, iters, conv
        llr = np.ascontiguousarray(llr, np.float64)
        lam = np.zeros((F, self.code.N), np.float64) if want_lam else None
        check(lib().ldpc_decode_batch_f64(self._h, int(max_iters), F, ptr(llr, C.c_double), ptr(bits, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8), ptr(lam, C.c_double)))
        return (bits, iters, conv, lam) if want_lam else (bits, iters, conv)

    def decode_batch_packed(self, llr, max_iters):
        """llr [F][N] float16 or float32 (host), int8 on an "i8" decoder -> packed bits [F][ceil(N/8)] (bit i of a frame: byte i // 8, bit i % 8), iters, converged"""
        llr = np.ascontiguousarray(llr)
        assert llr.dtype in (np.float16, np.float32, np.int8) and llr.shape[1] == self.code.N
        F = llr.shape[0]
        packed = np.zeros((F, (self.code.N + 7) // 8), np.uint8)
        iters = np.zeros(F, np.int32)
        conv = np.zeros(F, np.uint8)
        check(lib().ldpc_decode_batch_packed(self._h, int(max_iters), F, llr.ctypes.data_as(C.c_void_p), {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.int8): 2}[llr.dtype],
                                             ptr(packed, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8)))
        return packed, iters, conv

    def decode_batch_dev_packed(self, d_llr_ptr, d_packed_ptr, batch, max_iters, d_iters_ptr=None, d_conv_ptr=None, stream=None, llr_f16=False, llr_i8=False):
        """device pointers; d_packed [batch][ceil(N/8)] bytes; d_llr float32, float16 with llr_f16=True, int8 with llr_i8=True"""
        check(lib().ldpc_decode_batch_dev_packed(self._h, int(max_iters), int(batch), d_llr_ptr, 2 if llr_i8 else 1 if llr_f16 else 0, d_packed_ptr, d_iters_ptr, d_conv_ptr, stream))

    def decode_batch_dev(self, d_llr_ptr, d_bits_ptr, batch, max_iters, d_iters_ptr=None, d_conv_ptr=None, stream=None, llr_f16=False, llr_i8=False):
        """device pointers; d_llr [batch][N] float32, float16 with llr_f16=True, or int8 with llr_i8=True (an "i8" decoder)"""
        fn = lib().ldpc_decode_batch_dev_i8 if llr_i8 else lib().ldpc_decode_batch_dev_f16 if llr_f16 else lib().ldpc_decode_batch_dev
        check(fn(self._h, int(max_iters), int(batch), d_llr_ptr, d_bits_ptr, d_iters_ptr, d_conv_ptr, stream))

    def decode_batch_dev_soft(self, d_llr_ptr, d_bits_ptr, d_soft_ptr, batch, max_iters, kind="posterior", soft_fmt="f32", soft_qscale=0.0, d_iters_ptr=None,
                              d_conv_ptr=None, stream=None, llr_fmt="f32"):
        """ldpc_decode_batch_dev_soft: device pointers; d_llr [batch][N] of llr_fmt "f32" / "f16" / "i8"; d_soft [batch][N] of soft_fmt;
        kind "posterior" (lam as it stands when the frame stops) or "extrinsic" (that less the channel LLR as the cell took it in).
        Contexts of the on-chip layered min-sum kernel for any H only"""
        k = _SOFT_KINDS[kind] if isinstance(kind, str) else int(kind)
        check(lib().ldpc_decode_batch_dev_soft(self._h, int(max_iters), int(batch), d_llr_ptr, _llr_fmt(llr_fmt), d_bits_ptr, d_iters_ptr, d_conv_ptr, d_soft_ptr,
                                               _llr_fmt(soft_fmt), float(soft_qscale), k, stream))

    def decode_batch_soft(self, llr, max_iters, kind="posterior", soft_fmt="f32", soft_qscale=0.0):
        """llr [F][N] float32, float16 or (an "i8" decoder) int8, host -> bits [F][N], iters [F], converged [F], soft [F][N] of soft_fmt
        (numpy float32 / float16 / int8).  The arrays travel through torch tensors on the context's device"""
        import torch
        llr = np.ascontiguousarray(llr)
        fmt = {np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int8): "i8"}[llr.dtype]
        F = llr.shape[0]
        assert llr.shape == (F, self.code.N)
        dev = torch.device("cuda", lib().ldpc_ctx_device(self._h))
        d_llr = torch.from_numpy(llr).to(dev)
        d_bits = torch.zeros((F, self.code.N), dtype=torch.uint8, device=dev)
        d_iters = torch.zeros(F, dtype=torch.int32, device=dev)
        d_conv = torch.zeros(F, dtype=torch.uint8, device=dev)
        d_soft = torch.zeros((F, self.code.N), dtype={"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}[soft_fmt], device=dev)
        torch.cuda.synchronize(dev)
        self.decode_batch_dev_soft(d_llr.data_ptr(), d_bits.data_ptr(), d_soft.data_ptr(), F, max_iters, kind, soft_fmt, soft_qscale, d_iters.data_ptr(),
                                   d_conv.data_ptr(), None, fmt)
        self.synchronize()
        return d_bits.cpu().numpy(), d_iters.cpu().numpy(), d_conv.cpu().numpy(), d_soft.cpu().numpy()

    def decode_batch_dev_continue(self, state, d_llr_ptr, d_bits_ptr, batch, max_iters, d_soft_ptr=None, kind="posterior", soft_fmt="f32", soft_qscale=0.0,
                                  d_iters_ptr=None, d_conv_ptr=None, stream=None, llr_fmt="f32", first=0):
        """ldpc_decode_batch_dev_continue: decode_batch_dev_soft that starts from slots first .. first + batch - 1 of `state` (a DecodeState made
        for this decoder) and leaves the new state there; d_soft_ptr may be None.  From a reset state it is decode_batch_dev_soft"""
        k = _SOFT_KINDS[kind] if isinstance(kind, str) else int(kind)
        check(lib().ldpc_decode_batch_dev_continue(self._h, state._h if state is not None else None, int(first), int(max_iters), int(batch), d_llr_ptr, _llr_fmt(llr_fmt),
                                                   d_bits_ptr, d_iters_ptr, d_conv_ptr, d_soft_ptr, _llr_fmt(soft_fmt), float(soft_qscale), k, stream))

    def decode_batch_continue(self, state, llr, max_iters, kind="posterior", soft_fmt="f32", soft_qscale=0.0, first=0):
        """decode_batch_soft on slots first .. first + F - 1 of `state`: llr [F][N] host -> bits, iters, converged, soft (through torch tensors)"""
        import torch
        llr = np.ascontiguousarray(llr)
        fmt = {np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int8): "i8"}[llr.dtype]
        F = llr.shape[0]
        assert llr.shape == (F, self.code.N)
        dev = torch.device("cuda", lib().ldpc_ctx_device(self._h))
        d_llr = torch.from_numpy(llr).to(dev)
        d_bits = torch.zeros((F, self.code.N), dtype=torch.uint8, device=dev)
        d_iters = torch.zeros(F, dtype=torch.int32, device=dev)
        d_conv = torch.zeros(F, dtype=torch.uint8, device=dev)
        d_soft = torch.zeros((F, self.code.N), dtype={"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}[soft_fmt], device=dev)
        torch.cuda.synchronize(dev)
        self.decode_batch_dev_continue(state, d_llr.data_ptr(), d_bits.data_ptr(), F, max_iters, d_soft.data_ptr(), kind, soft_fmt, soft_qscale, d_iters.data_ptr(),
                                       d_conv.data_ptr(), None, fmt, first)
        self.synchronize()
        return d_bits.cpu().numpy(), d_iters.cpu().numpy(), d_conv.cpu().numpy(), d_soft.cpu().numpy()

    def synchronize(self):
        check(lib().ldpc_ctx_synchronize(self._h))

    def decode_trace(self, llr, max_iters):
        llr = np.ascontiguousarray(llr, np.float64)
        F = llr.shape[0]
        bits = np.zeros((F, self.code.N), np.uint8)
        iters = np.zeros(F, np.int32)
        conv = np.zeros(F, np.uint8)
        trace = np.zeros((F, max_iters + 1, self.code.N), np.float64)
        check(lib().ldpc_decode_trace(self._h, int(max_iters), F, ptr(llr, C.c_double), ptr(bits, C.c_uint8), ptr(iters, C.c_int32), ptr(conv, C.c_uint8), ptr(trace, C.c_double)))
        return bits, iters, conv, trace

    def debug_step(self, orig, lam, ne):
        orig = np.ascontiguousarray(orig, np.float64)
        lam = np.ascontiguousarray(lam, np.float64)
        ne = np.ascontiguousarray(ne, np.float64)
        F = orig.shape[0]
        assert orig.shape == lam.shape == (F, self.code.N) and ne.shape == (F, self.code.E)
        ne2 = np.zeros_like(ne)
        lam2 = np.zeros_like(lam)
        syn = np.zeros(F, np.uint8)
        check(lib().ldpc_debug_step(self._h, F, ptr(orig, C.c_double), ptr(lam, C.c_double), ptr(ne, C.c_double), ptr(ne2, C.c_double), ptr(lam2, C.c_double), ptr(syn, C.c_uint8)))
        return ne2, lam2, syn.astype(bool)

    def set_timing(self, enabled=True):
        check(lib().ldpc_ctx_set_timing(self._h, int(bool(enabled))))

    def kernel_time(self):
        """-> (launches, total_ms) of the dominant kernel since the last call (HIP events)."""
        n, ms = C.c_int(), C.c_double()
        check(lib().ldpc_ctx_kernel_time(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    @property
    def kernel_name(self):
        return lib().ldpc_ctx_kernel_name(self._h).decode()

    @property
    def kernel_geometry(self):
        """-> (threads per workgroup, frames per workgroup) of the dominant kernel's last launch (0, 0: flood path)"""
        t, f = C.c_int(), C.c_int()
        check(lib().ldpc_ctx_kernel_geometry(self._h, C.byref(t), C.byref(f)))
        return t.value, f.value

    def close(self):
        if self._h and self._owned:
            lib().ldpc_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class DecodeState:
    """ldpc_decode_state: the check messages of `frames` frame slots of one Decoder, kept between Decoder.decode_batch_dev_continue calls;
    all slots reset.  Bound to the decoder it was made for; close it before that decoder (close_all does)"""

    def __init__(self, dec, frames):
        self._h = lib().ldpc_decode_state_create(dec._h, int(frames))
        if not self._h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self.decoder = dec
        _register(self)

    @property
    def frames(self):
        return int(lib().ldpc_decode_state_frames(self._h))

    @property
    def nbytes(self):
        """the device bytes the state holds"""
        return int(lib().ldpc_decode_state_bytes(self._h))

    def reset(self, first=0, count=None, stream=None):
        """zero-fill slots first .. first + count - 1 (count None: to the last one); enqueued on `stream` (None: the decoder's), not synchronised"""
        check(lib().ldpc_decode_state_reset(self._h, int(first), self.frames - int(first) if count is None else int(count), stream))

    def close(self):
        if self._h:
            lib().ldpc_decode_state_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Cascade:
    """ldpc_cascade: two Decoders in a row -- dec1 decodes the batch, the frames it does not converge on (the first `capacity` in frame
    order) are decoded again from the channel LLRs by dec2 and take its result.  capacity None: dec2's max_batch.  Close it before its
    decoders (close_all does)"""

    def __init__(self, dec1, dec2, capacity=None):
        cap = dec2.max_batch if capacity is None else capacity
        self._h = lib().ldpc_cascade_create(dec1._h if dec1 is not None else None, dec2._h if dec2 is not None else None, int(cap))
        if not self._h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self.dec1, self.dec2 = dec1, dec2
        _register(self)

    @property
    def capacity(self):
        return int(lib().ldpc_cascade_capacity(self._h))

    @property
    def nbytes(self):
        """the device bytes the cascade holds"""
        return int(lib().ldpc_cascade_bytes(self._h))

    def decode_batch_dev(self, d_llr_ptr, d_bits_ptr, batch, max_iters1, max_iters2, d_iters_ptr=None, d_conv_ptr=None, d_stage_ptr=None, d_stats_ptr=None, stream=None,
                         llr_fmt="f32"):
        """ldpc_cascade_decode_dev: device pointers; d_llr [batch][N] of llr_fmt "f32" / "f16" / "i8"; d_stage [batch] bytes (1 or 2) and
        d_stats [3] uint32 (failed stage 1, sent to stage 2, sent and failed again) may be None like d_iters and d_conv.  Enqueued on
        `stream` (None: dec1's own), not synchronised"""
        check(lib().ldpc_cascade_decode_dev(self._h, int(max_iters1), int(max_iters2), int(batch), d_llr_ptr, _llr_fmt(llr_fmt), d_bits_ptr, d_iters_ptr, d_conv_ptr,
                                            d_stage_ptr, d_stats_ptr, stream))

    def decode_batch(self, llr, max_iters1, max_iters2):
        """llr [F][N] float32, float16 or (two "i8" decoders) int8, host -> bits [F][N], iters [F], converged [F], stage [F], stats [3]
        (through torch tensors on the decoders' device)"""
        import torch
        llr = np.ascontiguousarray(llr)
        fmt = {np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int8): "i8"}[llr.dtype]
        F, N = llr.shape[0], self.dec1.code.N
        assert llr.shape == (F, N)
        dev = torch.device("cuda", lib().ldpc_ctx_device(self.dec1._h))
        d_llr = torch.from_numpy(llr).to(dev)
        d_bits = torch.zeros((F, N), dtype=torch.uint8, device=dev)
        d_iters = torch.zeros(F, dtype=torch.int32, device=dev)
        d_conv = torch.zeros(F, dtype=torch.uint8, device=dev)
        d_stage = torch.zeros(F, dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.decode_batch_dev(d_llr.data_ptr(), d_bits.data_ptr(), F, max_iters1, max_iters2, d_iters.data_ptr(), d_conv.data_ptr(), d_stage.data_ptr(), d_stats.data_ptr(),
                              None, fmt)
        self.dec1.synchronize()
        return d_bits.cpu().numpy(), d_iters.cpu().numpy(), d_conv.cpu().numpy(), d_stage.cpu().numpy(), d_stats.cpu().numpy().view(np.uint32)

    def close(self):
        if self._h:
            lib().ldpc_cascade_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Batcher:
    """ldpc_batcher on one decoder replica: concurrent per-frame decode_one() calls (one per host thread, the reference
    harness's calling convention, Utils.hs:63-69) are collected into one launch.  This is the object the Haskell binding
    shares between the replicas of one GPU (haskell/ECC/Code/LDPC/GPU/HIP.hs closureFor)."""

    def __init__(self, decoder: Decoder, max_frames=64, max_wait_us=200):
        self.decoder = decoder
        self._h = lib().ldpc_batcher_create(decoder._h, int(max_frames), int(max_wait_us))
        if not self._h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        _register(self)

    def decode_one(self, llr, max_iters):
        llr = np.ascontiguousarray(llr, np.float64)
        N = self.decoder.code.N
        assert llr.shape == (N,)
        bits = np.zeros(N, np.uint8)
        it, cv = C.c_int(), C.c_int()
        check(lib().ldpc_batcher_decode_one(self._h, int(max_iters), ptr(llr, C.c_double), ptr(bits, C.c_uint8), C.byref(it), C.byref(cv)))
        return bits, it.value, bool(cv.value)

    def stats(self):
        """-> (decode calls, launches) so far"""
        a, b = C.c_long(), C.c_long()
        check(lib().ldpc_batcher_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self._h:
            lib().ldpc_batcher_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Matrix:
    """A loaded matrix file (ldpc_matrix): the reference's LoaderMatrix (Data/BitMatrix/Loader.hs:49-52)."""

    def __init__(self, handle):
        if not handle:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = handle
        _register(self)
        v = [C.c_int() for _ in range(5)]
        check(lib().ldpc_matrix_info(self._h, *[C.byref(x) for x in v]))
        self.rows, self.cols, self.sz, self.block_rows, self.block_cols = [x.value for x in v]

    @classmethod
    def load(cls, codes_dir, name):
        return cls(lib().ldpc_matrix_load(str(codes_dir).encode(), name.encode()))

    @classmethod
    def load_mackay(cls, path):
        return cls(lib().ldpc_matrix_load_mackay(str(path).encode()))

    def dense(self):
        out = np.zeros((self.rows, self.cols), np.uint8)
        check(lib().ldpc_matrix_dense(self._h, ptr(out, C.c_uint8)))
        return out

    def rank(self):
        """rank over GF(2) of the expanded matrix"""
        r = lib().ldpc_matrix_rank(self._h)
        if r < 0:
            raise LdpcError(r, last_error())
        return r

    def qc_words(self):
        """first-row patterns of a QC source as little-endian 32-bit words [block_rows][block_cols][ceil(sz/32)]"""
        out = np.zeros((self.block_rows, self.block_cols, (self.sz + 31) // 32), np.uint32)
        check(lib().ldpc_matrix_qc_words(self._h, ptr(out, C.c_uint32)))
        return out

    def qc_offsets(self):
        out = np.zeros((self.block_rows, self.block_cols), np.int32)
        check(lib().ldpc_matrix_qc_offsets(self._h, ptr(out, C.c_int32)))
        return out

    def close(self):
        if self._h:
            lib().ldpc_matrix_destroy(self._h)
            self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def _llr_fmt(fmt):
    """"f32" / "f16" / "i8" (or the integer LDPC_LLR_*, passed through for the library to judge)"""
    return {"f32": LLR_F32, "f16": LLR_F16, "i8": LLR_I8}[fmt] if isinstance(fmt, str) else int(fmt)


class Modulation:
    """A labelled constellation (ldpc_modulation): points [2^m][2] float32 (I, Q), m = 1..6, or a built-in by name.  Symbol s of a
    frame carries codeword bits m s .. m s + m - 1, the first one the MSB of the label = the index into the table.
    Modulation.product(levels_i, levels_q) and the built-ins "64qam" .. "4096qam" are product constellations: 2^b levels an axis,
    b = 1..6, m = 2 b, label = (index into levels_i) << b | (index into levels_q).
    The demappers' LLR rule travels with the object: max-log unless with_rule("logmap") made it (include/ldpc_hip.h, THE LLR RULE)."""

    RULES = {"maxlog": DEMAP_MAXLOG, "logmap": DEMAP_LOGMAP}

    BUILTIN = {"bpsk": MOD_BPSK, "qpsk": MOD_QPSK, "8psk": MOD_8PSK, "16qam": MOD_16QAM,
               "64qam": MOD_64QAM, "256qam": MOD_256QAM, "1024qam": MOD_1024QAM, "4096qam": MOD_4096QAM}

    def __init__(self, points, _handle=None):
        if _handle is not None:
            h = _handle
        elif isinstance(points, str):
            h = lib().ldpc_modulation_create_builtin(self.BUILTIN.get(points.lower(), -1))
        elif isinstance(points, int):
            h = lib().ldpc_modulation_create_builtin(points)
        else:
            pts = np.ascontiguousarray(points, np.float32)
            n = pts.shape[0] if pts.ndim == 2 and pts.shape[1] == 2 else 0
            m = n.bit_length() - 1
            if n < 2 or n != 1 << m:
                raise LdpcError(EINVAL, "Modulation: points must be [2^m][2]")
            h = lib().ldpc_modulation_create(m, ptr(pts, C.c_float))
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = h
        self.bits = int(lib().ldpc_modulation_bits(h))
        _register(self)

    @property
    def points(self):
        out = np.zeros((1 << self.bits, 2), np.float32)
        assert lib().ldpc_modulation_points(self._h, ptr(out, C.c_float)) == 1 << self.bits
        return out

    @classmethod
    def product(cls, levels_i, levels_q):
        """ldpc_modulation_create_product: two level sets [2^b] float32, b = 1..6"""
        li, lq = np.ascontiguousarray(levels_i, np.float32), np.ascontiguousarray(levels_q, np.float32)
        n = li.shape[0] if li.ndim == 1 and li.shape == lq.shape else 0
        b = n.bit_length() - 1
        if n < 2 or n != 1 << b:
            raise LdpcError(EINVAL, "Modulation.product: the two level sets must be [2^b] each")
        h = lib().ldpc_modulation_create_product(b, ptr(li, C.c_float), ptr(lq, C.c_float))
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        return cls(None, _handle=h)

    @property
    def axis_levels(self):
        """(levels_i, levels_q), [2^b] float32 each, of a product object; None for a table object"""
        b = int(lib().ldpc_modulation_axis_levels(self._h, None, None))
        if b <= 0:
            return None
        li, lq = np.zeros(1 << b, np.float32), np.zeros(1 << b, np.float32)
        assert lib().ldpc_modulation_axis_levels(self._h, ptr(li, C.c_float), ptr(lq, C.c_float)) == b
        return li, lq

    @property
    def energy(self):
        return float(lib().ldpc_modulation_energy(self._h))

    def with_rule(self, rule):
        """ldpc_modulation_with_rule: a new object with this constellation, demapped by "maxlog" or "logmap" (or the rule's number)"""
        r = self.RULES.get(rule.lower(), -1) if isinstance(rule, str) else int(rule)
        h = lib().ldpc_modulation_with_rule(self._h, r)
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        return type(self)(None, _handle=h)

    @property
    def rule(self):
        """the demappers' LLR rule, "maxlog" or "logmap" (ldpc_modulation_rule)"""
        r = int(lib().ldpc_modulation_rule(self._h))
        return {v: k for k, v in self.RULES.items()}[r]

    def symbols(self, n_tx):
        n = lib().ldpc_modulation_symbols(self._h, int(n_tx))
        if n < 0:
            raise LdpcError(n, last_error())
        return n

    def close(self):
        if self._h:
            lib().ldpc_modulation_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def demap(mod: Modulation, batch, n_tx, N, d_sym_ptr, noise_var, d_llr_ptr, llr_fmt="f32", qscale=0.0, stream=None):
    """ldpc_demap_dev: samples [batch][ceil(n_tx / m)][2] float32 -> max-log LLRs [batch][N] in llr_fmt ("f32", "f16", "i8"), on the
    calling thread's device"""
    check(lib().ldpc_demap_dev(mod._h if mod is not None else None, int(batch), int(n_tx), int(N), d_sym_ptr, float(noise_var), d_llr_ptr, _llr_fmt(llr_fmt),
                               float(qscale), stream))


class Interleaver:
    """A bit interleaver (ldpc_interleaver): transmitted bit t is codeword bit pos[t], pos [n_tx] injective into 0..N-1; the codeword
    positions no entry names are punctured (LLR 0).  Interleaver.block(rows, cols, twist, order) is the block rule.  The table is
    checked before the device is touched; it then lives on `device` (None: the calling thread's)."""

    def __init__(self, pos, N, device=None):
        a = np.asarray(pos)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
            raise LdpcError(EINVAL, "Interleaver: pos must be a one-dimensional array of 32-bit integers")
        p = np.ascontiguousarray(a, np.int32)
        dev = int(device) if device is not None else lib().ldpc_current_device()
        h = lib().ldpc_interleaver_create_on(dev, p.shape[0], int(N), ptr(p, C.c_int32) if p.size else None)
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = h
        self.n_tx, self.N = int(p.shape[0]), int(N)
        _register(self)

    @staticmethod
    def block_positions(rows, cols, twist=None, order=None):
        """ldpc_interleaver_block_positions (host only): pos[r cols + j] = c rows + ((r - twist[c]) mod rows), c = order[j] -> [rows * cols] int32"""
        rows, cols = int(rows), int(cols)
        tw = None if twist is None else np.ascontiguousarray(twist, np.int32)
        od = None if order is None else np.ascontiguousarray(order, np.int32)
        if (tw is not None and tw.shape != (cols,)) or (od is not None and od.shape != (cols,)):
            raise LdpcError(EINVAL, "Interleaver.block_positions: twist and order must be [cols]")
        n = rows * cols if rows > 0 and cols > 0 and rows * cols < 2 ** 31 else 1
        out = np.zeros(n, np.int32)
        check(lib().ldpc_interleaver_block_positions(rows, cols, None if tw is None else ptr(tw, C.c_int32), None if od is None else ptr(od, C.c_int32),
                                                     ptr(out, C.c_int32)))
        return out

    @classmethod
    def block(cls, rows, cols, twist=None, order=None, N=None, device=None):
        """the block interleaver of rows x cols bits; N (default rows * cols) > rows * cols punctures the tail"""
        pos = cls.block_positions(rows, cols, twist, order)
        return cls(pos, pos.shape[0] if N is None else N, device=device)

    @property
    def positions(self):
        out = np.zeros(self.n_tx, np.int32)
        assert lib().ldpc_interleaver_positions(self._h, ptr(out, C.c_int32)) == self.n_tx
        return out

    @property
    def dims(self):
        a, b = C.c_int(), C.c_int()
        check(lib().ldpc_interleaver_dims(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self._h:
            lib().ldpc_interleaver_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def _h(o):
    return o._h if o is not None else None


def demap_il(mod: Modulation, il: Interleaver, batch, d_sym_ptr, noise_var, d_llr_ptr, llr_fmt="f32", qscale=0.0, stream=None):
    """ldpc_demap_dev_il: demap() through the table: the LLR of transmitted bit t at element il.positions[t] of its row of [batch][il.N],
    0 at the punctured positions"""
    check(lib().ldpc_demap_dev_il(_h(mod), _h(il), int(batch), d_sym_ptr, float(noise_var), d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), stream))


def demap_il_csi(mod: Modulation, il: Interleaver, batch, d_sym_ptr, d_gain_ptr, noise_var, d_llr_ptr, llr_fmt="f32", qscale=0.0, stream=None):
    """ldpc_demap_dev_il_csi: demap_il() with the power gain of every symbol, d_gain [batch][n_sym] float32: the noise variance of symbol
    s is noise_var / gain, its LLRs are scaled by float32(1 / (2 noise_var)) * gain"""
    check(lib().ldpc_demap_dev_il_csi(_h(mod), _h(il), int(batch), d_sym_ptr, d_gain_ptr, float(noise_var), d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), stream))


def demap_il_apriori(mod: Modulation, il: Interleaver, batch, d_sym_ptr, d_gain_ptr, noise_var, d_apriori_ptr, d_llr_ptr, llr_fmt="f32", qscale=0.0, stream=None):
    """ldpc_demap_dev_il_apriori: demap_il_csi() with bit knowledge, d_apriori [batch][N] float32 in codeword order (LLR > 0 <=> bit 1; the
    extrinsic output of Decoder.decode_batch_dev_soft, or zeros).  d_gain_ptr may be None (gains of 1).  Table objects only; the LLRs
    written are extrinsic: every bit's own a-priori value is taken out again"""
    check(lib().ldpc_demap_dev_il_apriori(_h(mod), _h(il), int(batch), d_sym_ptr, d_gain_ptr, float(noise_var), d_apriori_ptr, d_llr_ptr, _llr_fmt(llr_fmt), float(qscale),
                                          stream))


class Fading:
    """ldpc_fading: block fading with `block` symbols per block and the Rician factor k_factor (linear; 0 = Rayleigh).  A plain value:
    nothing is checked here, the entry points judge it.  struct_size: for the tests of that field"""

    def __init__(self, block=1, k_factor=0.0, struct_size=None):
        self.block, self.k_factor = int(block), float(k_factor)
        self.struct = FadingStruct(C.sizeof(FadingStruct) if struct_size is None else int(struct_size), self.block, self.k_factor)

    def _ref(self):
        return C.byref(self.struct)


def _fad(f):
    return f._ref() if f is not None else None


def interleave_bits(il: Interleaver, batch, d_cw_ptr, d_tx_ptr, cw_fmt="bytes", tx_fmt="bytes", stream=None):
    """ldpc_interleave_bits_dev: codewords [batch][N] ("bytes", or "packed" rows of ceil(N / 8) bytes) -> transmitted bits [batch][n_tx]"""
    check(lib().ldpc_interleave_bits_dev(_h(il), int(batch), d_cw_ptr, Sim._bits_fmt(cw_fmt), d_tx_ptr, Sim._bits_fmt(tx_fmt), stream))


def deinterleave_llr(il: Interleaver, batch, d_llr_tx_ptr, d_llr_ptr, llr_fmt="f32", stream=None):
    """ldpc_deinterleave_llr_dev: LLRs [batch][n_tx] in transmitted order -> [batch][N], 0 at the punctured positions, same element type"""
    check(lib().ldpc_deinterleave_llr_dev(_h(il), int(batch), d_llr_tx_ptr, d_llr_ptr, _llr_fmt(llr_fmt), stream))


class Ratematch:
    """A rate-matching table (ldpc_ratematch): transmitted bit t is codeword bit pos[t], pos [E] ANY map into 0..N-1 -- entries may
    repeat, E may exceed N; the positions no entry names are not sent in this round.  Ratematch.circular(...) is the circular-buffer
    rule.  The table is checked before the device is touched; it then lives on `device` (None: the calling thread's) with its inverse."""

    def __init__(self, pos, N, device=None):
        a = np.asarray(pos)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
            raise LdpcError(EINVAL, "Ratematch: pos must be a one-dimensional array of 32-bit integers")
        p = np.ascontiguousarray(a, np.int32)
        dev = int(device) if device is not None else lib().ldpc_current_device()
        h = lib().ldpc_ratematch_create_on(dev, p.shape[0], int(N), ptr(p, C.c_int32) if p.size else None)
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = h
        self.E, self.N = int(p.shape[0]), int(N)
        _register(self)

    @staticmethod
    def circular_positions(n_buf, start, E, buf=None):
        """ldpc_ratematch_circular_positions (host only): pos[t] = buf[(start + t) mod n_buf], buf None = the identity -> [E] int32"""
        n_buf, start, E = int(n_buf), int(start), int(E)
        b = None if buf is None else np.ascontiguousarray(buf, np.int32)
        if b is not None and b.shape != (n_buf,):
            raise LdpcError(EINVAL, "Ratematch.circular_positions: buf must be [n_buf]")
        out = np.zeros(max(E, 1), np.int32)
        check(lib().ldpc_ratematch_circular_positions(n_buf, None if b is None else ptr(b, C.c_int32), start, E, ptr(out, C.c_int32)))
        return out

    @classmethod
    def circular(cls, N, start, E, buf=None, n_buf=None, device=None):
        """the table of a circular buffer of n_buf (default: len(buf), or N) positions read for E bits from `start`"""
        n_buf = (N if buf is None else len(buf)) if n_buf is None else n_buf
        return cls(cls.circular_positions(n_buf, start, E, buf), N, device=device)

    @property
    def positions(self):
        out = np.zeros(self.E, np.int32)
        assert lib().ldpc_ratematch_positions(self._h, ptr(out, C.c_int32)) == self.E
        return out

    @property
    def fanin(self):
        """[N] int32: how many transmitted bits name each codeword position"""
        out = np.zeros(self.N, np.int32)
        check(lib().ldpc_ratematch_fanin(self._h, ptr(out, C.c_int32)))
        return out

    @property
    def dims(self):
        a, b = C.c_int(), C.c_int()
        check(lib().ldpc_ratematch_dims(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self._h:
            lib().ldpc_ratematch_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def demap_rm(mod: Modulation, rm: Ratematch, batch, d_sym_ptr, d_gain_ptr, noise_var, d_llr_ptr, llr_fmt="f32", qscale=0.0, accumulate=False, stream=None):
    """ldpc_demap_dev_rm: per codeword position the left-to-right float32 sum of the LLRs of the transmitted bits that name it (d_gain_ptr
    None: no channel state), written to [batch][rm.N] (accumulate False; 0 where nothing was sent) or added to the soft buffer there"""
    check(lib().ldpc_demap_dev_rm(_h(mod), _h(rm), int(batch), d_sym_ptr, d_gain_ptr, float(noise_var), d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), int(accumulate),
                                  stream))


def ratematch_llr(rm: Ratematch, batch, d_llr_tx_ptr, d_llr_ptr, llr_fmt="f32", qscale=0.0, accumulate=False, stream=None):
    """ldpc_ratematch_llr_dev: demap_rm() with the LLRs of the transmitted bits given, [batch][rm.E] float32"""
    check(lib().ldpc_ratematch_llr_dev(_h(rm), int(batch), d_llr_tx_ptr, d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), int(accumulate), stream))


def ratematch_bits(rm: Ratematch, batch, d_cw_ptr, d_tx_ptr, cw_fmt="bytes", tx_fmt="bytes", stream=None):
    """ldpc_ratematch_bits_dev: codewords [batch][N] ("bytes", or "packed" rows of ceil(N / 8) bytes) -> transmitted bits [batch][E]"""
    check(lib().ldpc_ratematch_bits_dev(_h(rm), int(batch), d_cw_ptr, Sim._bits_fmt(cw_fmt), d_tx_ptr, Sim._bits_fmt(tx_fmt), stream))


CRC_KINDS = {"crc6": 0, "crc11": 1, "crc16": 2, "crc24a": 3, "crc24b": 4, "crc24c": 5, "crc32": 6}   # LDPC_CRC_*


class Crc:
    """A CRC (ldpc_crc): width w, poly (the generator without x^w), init, xorout, over the first n_bits bits of a message of
    k = n_bits + w bits; unreflected, the CRC appended MSB first.  The parameters are checked before the device is touched; the table
    then lives on `device` (None: the calling thread's).  Crc.builtin("crc24a", n_bits) takes a built-in parameter set."""

    def __init__(self, width, poly, init=0, xorout=0, n_bits=None, device=None):
        if n_bits is None:
            raise LdpcError(EINVAL, "Crc: n_bits (the payload length) is required")
        for name, v in (("width", width), ("n_bits", n_bits)):
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise LdpcError(EINVAL, f"Crc: {name} does not fit an int")
        for name, v in (("poly", poly), ("init", init), ("xorout", xorout)):
            if not 0 <= int(v) < 2 ** 32:
                raise LdpcError(EINVAL, f"Crc: {name} must be in 0 .. 2^32 - 1")
        dev = int(device) if device is not None else lib().ldpc_current_device()
        h = lib().ldpc_crc_create_on(dev, int(width), int(poly), int(init), int(xorout), int(n_bits))
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = h
        self.width, self.n_bits, self.k = int(width), int(n_bits), int(n_bits) + int(width)
        _register(self)

    @staticmethod
    def _kind(kind):
        return CRC_KINDS[kind] if isinstance(kind, str) else int(kind)

    @staticmethod
    def builtin_params(kind):
        """ldpc_crc_builtin (host only) -> (width, poly, init, xorout); kind: a name of CRC_KINDS or the integer of LDPC_CRC_*"""
        w, p, i, x = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().ldpc_crc_builtin(Crc._kind(kind), C.byref(w), C.byref(p), C.byref(i), C.byref(x)))
        return w.value, p.value, i.value, x.value

    @classmethod
    def builtin(cls, kind, n_bits, device=None):
        w, p, i, x = cls.builtin_params(kind)
        return cls(w, p, i, x, n_bits=n_bits, device=device)

    @staticmethod
    def bits_host(width, poly, init, xorout, bits):
        """ldpc_crc_bits_host (host only): the bit-serial rule over `bits` (one byte each, bit 0 read) -> the CRC"""
        b = np.ascontiguousarray(bits, np.uint8).reshape(-1)
        out = C.c_uint32()
        check(lib().ldpc_crc_bits_host(int(width), int(poly), int(init), int(xorout), b.shape[0], ptr(b, C.c_uint8) if b.size else None, C.byref(out)))
        return out.value

    @staticmethod
    def table(width, poly, n_bits):
        """ldpc_crc_table (host only): T [n_bits] uint32 of the linear form crc = C0 ^ XOR over the set bits i of T[i]"""
        out = np.zeros(max(int(n_bits), 1), np.uint32)
        check(lib().ldpc_crc_table(int(width), int(poly), int(n_bits), ptr(out, C.c_uint32)))
        return out[:int(n_bits)]

    def params(self):
        """ldpc_crc_params -> (width, poly, init, xorout, n_bits)"""
        w, p, i, x, n = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
        check(lib().ldpc_crc_params(self._h, C.byref(w), C.byref(p), C.byref(i), C.byref(x), C.byref(n)))
        return w.value, p.value, i.value, x.value, n.value

    def attach(self, batch, d_msg_ptr, msg_fmt="bytes", stream=None):
        """ldpc_crc_attach_dev, in place: messages [batch][k] bytes, or "packed" rows of 4 * ceil(k / 32) bytes; bits n_bits .. k - 1 are written"""
        check(lib().ldpc_crc_attach_dev(self._h, int(batch), d_msg_ptr, Sim._bits_fmt(msg_fmt), stream))

    def check(self, batch, d_msg_ptr, d_ok_ptr, msg_fmt="bytes", stream=None):
        """ldpc_crc_check_dev: d_ok [batch] bytes <- 1 where the trailing w bits are the CRC of the first n_bits, else 0"""
        check(lib().ldpc_crc_check_dev(self._h, int(batch), d_msg_ptr, Sim._bits_fmt(msg_fmt), d_ok_ptr, stream))

    def close(self):
        if self._h:
            lib().ldpc_crc_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


BCH_KINDS = {"m16t8": 0, "m16t10": 1, "m16t12": 2, "m14t12": 3}   # LDPC_BCH_*


class Bch:
    """A binary, narrow-sense, primitive BCH code (ldpc_bch) over GF(2^m) from prim_poly (the x^m term included), correcting t errors,
    shortened to n bits: k = n - p message bits, then the p bits of the remainder of m(x) x^p mod g, MSB first.  The parameters are
    checked before the device is touched; the tables then live on `device` (None: the calling thread's; -1: a host-only object that
    serves encode_host / decode_host alone).  Bch.builtin("m16t12", n) takes a built-in parameter set."""

    def __init__(self, m, prim_poly, t, n, device=None):
        for name, v in (("m", m), ("t", t), ("n", n)):
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise LdpcError(EINVAL, f"Bch: {name} does not fit an int")
        if not 0 <= int(prim_poly) < 2 ** 32:
            raise LdpcError(EINVAL, "Bch: prim_poly must be in 0 .. 2^32 - 1")
        dev = int(device) if device is not None else lib().ldpc_current_device()
        h = lib().ldpc_bch_create_on(dev, int(m), int(prim_poly), int(t), int(n))
        if not h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = h
        self.m, self.prim_poly, self.t, self.n, self.k = self.params()
        self.p = self.n - self.k
        _register(self)

    @staticmethod
    def builtin_params(kind):
        """ldpc_bch_builtin (host only) -> (m, prim_poly, t); kind: a name of BCH_KINDS or the integer of LDPC_BCH_*"""
        m, p, t = C.c_int(), C.c_uint32(), C.c_int()
        check(lib().ldpc_bch_builtin(BCH_KINDS[kind] if isinstance(kind, str) else int(kind), C.byref(m), C.byref(p), C.byref(t)))
        return m.value, p.value, t.value

    @classmethod
    def builtin(cls, kind, n, device=None):
        m, p, t = cls.builtin_params(kind)
        return cls(m, p, t, n, device=device)

    def params(self):
        """ldpc_bch_params -> (m, prim_poly, t, n, k)"""
        m, p, t, n, k = C.c_int(), C.c_uint32(), C.c_int(), C.c_int(), C.c_int()
        check(lib().ldpc_bch_params(self._h, C.byref(m), C.byref(p), C.byref(t), C.byref(n), C.byref(k)))
        return m.value, p.value, t.value, n.value, k.value

    def generator(self):
        """ldpc_bch_generator -> g [p + 1] uint8, g[j] = the coefficient of x^j"""
        g = np.zeros(self.p + 1, np.uint8)
        got = lib().ldpc_bch_generator(self._h, ptr(g, C.c_uint8))
        if got != self.p:
            raise LdpcError(got, last_error())
        return g

    def _row(self, row):
        r = np.array(row, np.uint8, copy=True).reshape(-1)
        if r.shape[0] != self.n:
            raise LdpcError(EINVAL, f"Bch: a row has n = {self.n} bytes, got {r.shape[0]}")
        return r

    def encode_host(self, row):
        """ldpc_bch_encode_host: the serial rule on one row [n] bytes (bit 0 of each read) -> the row with its p parity bytes written"""
        r = self._row(row)
        check(lib().ldpc_bch_encode_host(self._h, ptr(r, C.c_uint8)))
        return r

    def decode_host(self, row):
        """ldpc_bch_decode_host: -> (the row with bit 0 of the corrected bytes flipped, or as it was; nerr, -1 if not decodable)"""
        r, e = self._row(row), C.c_int(-2)
        check(lib().ldpc_bch_decode_host(self._h, ptr(r, C.c_uint8), C.byref(e)))
        return r, e.value

    def encode(self, batch, d_rows_ptr, fmt="bytes", stream=None):
        """ldpc_bch_encode_dev, in place: rows [batch][n] bytes, or "packed" rows of 4 * ceil(n / 32) bytes; bits k .. n - 1 are written"""
        check(lib().ldpc_bch_encode_dev(self._h, int(batch), d_rows_ptr, Sim._bits_fmt(fmt), stream))

    def decode(self, batch, d_rows_ptr, d_nerr_ptr, fmt="bytes", stream=None):
        """ldpc_bch_decode_dev, in place: d_nerr [batch] int32 <- the bits corrected in each row, or -1 for a row left as it was"""
        check(lib().ldpc_bch_decode_dev(self._h, int(batch), d_rows_ptr, Sim._bits_fmt(fmt), d_nerr_ptr, stream))

    def close(self):
        if self._h:
            lib().ldpc_bch_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Sim:
    """Device-side frame source + error tally (ldpc_sim)."""

    def __init__(self, code: Code, k, n_tx, G=None, max_batch=64, _handle=None, device=None, G_qc=None, from_H=False, systematic=False):
        """G: dense generator [k][p] bytes; G_qc = (sz, words [block_rows][block_cols][sz/32] uint32): the quasi-cyclic form
        (Matrix.qc_words), encoded by rotate-and-xor like Fast/Encoder.hs; from_H: the code's own parity-check matrix, by
        back-substitution (k must be N - M; Code.csr_triangular_order says whether H qualifies); systematic: ANY parity-check matrix,
        through Code.csr_systematic_form (k must be None: the library fills it, K = N - rank H; see positions()); none of them:
        all-zero codewords"""
        self.code, self.k, self.n_tx = code, (None if k is None else int(k)), int(n_tx)
        self._owned = _handle is None
        if _handle is None:
            dev = int(device) if device is not None else lib().ldpc_current_device()
            if dev < 0:
                raise LdpcError(ENODEVICE, "ldpc_init() has not succeeded")
            if systematic:
                if G is not None or G_qc is not None or from_H or k is not None:
                    raise LdpcError(EINVAL, "Sim(systematic=True): no generator is taken and k must be None (it is N - rank H)")
                _handle = lib().ldpc_sim_create_systematic_on(code._h, dev, int(n_tx), int(max_batch))
            elif from_H:
                if G is not None or G_qc is not None or int(k) != code.N - code.M:
                    raise LdpcError(EINVAL, f"Sim(from_H=True): no generator is taken and k must be N - M = {code.N - code.M}")
                _handle = lib().ldpc_sim_create_sparse_on(code._h, dev, int(n_tx), int(max_batch))
            elif G_qc is not None:
                sz, words = G_qc
                words = np.ascontiguousarray(words, np.uint32)
                _handle = lib().ldpc_sim_create_qc_on(code._h, dev, int(k), int(n_tx), int(sz), words.shape[0], words.shape[1], ptr(words, C.c_uint32), int(max_batch))
            elif G is not None:
                G = np.ascontiguousarray(G, np.uint8)
                assert G.shape[0] == k
                _handle = lib().ldpc_sim_create_on(code._h, dev, int(k), int(n_tx), G.shape[1], ptr(G, C.c_uint8), int(max_batch))
            else:
                _handle = lib().ldpc_sim_create_on(code._h, dev, int(k), int(n_tx), 0, None, int(max_batch))
        if not _handle:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        self._h = _handle
        if self.k is None:
            self.k = int(lib().ldpc_sim_message_length(_handle))
        _register(self)

    def positions(self):
        """-> (msg_pos [k], par_pos): where the message and the parity bits sit in the codeword (ldpc_sim_positions)"""
        mp, pp = np.zeros(max(self.k, 1), np.int32), np.zeros(max(self.code.N, 1), np.int32)
        n = lib().ldpc_sim_positions(self._h, ptr(mp, C.c_int32), ptr(pp, C.c_int32))
        if n < 0:
            raise LdpcError(n, last_error())
        return mp[:self.k].copy(), pp[:n].copy()

    def generate(self, seed, first_frame, batch, ebn0_db, d_llr_ptr, d_msg_ptr=None, stream=None, llr_f16=False):
        fn = lib().ldpc_sim_generate_f16 if llr_f16 else lib().ldpc_sim_generate
        check(fn(self._h, int(seed), int(first_frame), int(batch), float(ebn0_db), d_llr_ptr, d_msg_ptr, stream))

    @property
    def encoder(self):
        return {0: "none", 1: "dense", 2: "qc", 3: "sparse", 4: "systematic"}[lib().ldpc_sim_encoder(self._h)]

    def encode_batch(self, seed, first_frame, batch, d_codewords_ptr, d_msg_ptr=None, stream=None):
        """the encoder alone: codewords [batch][n_tx] bytes on the device"""
        check(lib().ldpc_sim_encode_batch(self._h, int(seed), int(first_frame), int(batch), d_codewords_ptr, d_msg_ptr, stream))

    @staticmethod
    def _bits_fmt(fmt):
        """"bytes" / "packed" (or the integer of ldpc_bit_format, passed through for the library to judge)"""
        return {"bytes": BITS_BYTES, "packed": BITS_PACKED}[fmt] if isinstance(fmt, str) else int(fmt)

    def encode_messages(self, batch, d_msg_ptr, d_cw_ptr, msg_fmt="bytes", cw_fmt="bytes", stream=None):
        """the encoder alone on the caller's messages (device pointers).  "bytes": messages [batch][k], codewords [batch][n_tx], one
        byte per bit; "packed": message rows of 4 * ceil(k / 32) bytes, codeword rows of ceil(n_tx / 8) bytes, bit i in byte i / 8 at
        bit i % 8.  Messages are in the order of positions()[0]."""
        check(lib().ldpc_sim_encode_messages(self._h, int(batch), d_msg_ptr, self._bits_fmt(msg_fmt), d_cw_ptr, self._bits_fmt(cw_fmt), stream))

    def generate_from(self, seed, first_frame, batch, ebn0_db, d_msg_ptr, d_llr_ptr, msg_fmt="bytes", stream=None, llr_f16=False):
        """generate() with the caller's messages in place of the drawn ones: the same noise, LLRs [batch][N] float32 or fp16"""
        check(lib().ldpc_sim_generate_from(self._h, int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_ptr, self._bits_fmt(msg_fmt),
                                           d_llr_ptr, int(llr_f16), stream))

    def extract_messages(self, batch, d_bits_ptr, d_msg_ptr, msg_fmt="bytes", stream=None):
        """decoded bytes [batch][N] -> the messages (bit i = decoded bit positions()[0][i]) in msg_fmt"""
        check(lib().ldpc_sim_extract_messages(self._h, int(batch), d_bits_ptr, d_msg_ptr, self._bits_fmt(msg_fmt), stream))

    def noise_var(self, mod: "Modulation", ebn0_db):
        """sigma^2 per real dimension at Eb/N0 (dB) for this source's rate and that constellation (ldpc_sim_noise_var)"""
        return float(lib().ldpc_sim_noise_var(self._h, mod._h if mod is not None else None, float(ebn0_db)))

    def transmit(self, mod: "Modulation", seed, first_frame, batch, ebn0_db, d_sym_ptr, d_msg_in_ptr=None, msg_fmt="bytes", d_msg_ptr=None, stream=None):
        """the noisy symbols [batch][mod.symbols(n_tx)][2] float32 of the drawn messages (d_msg_in_ptr None) or the caller's"""
        check(lib().ldpc_sim_transmit(self._h, mod._h if mod is not None else None, int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr,
                                      self._bits_fmt(msg_fmt), d_sym_ptr, d_msg_ptr, stream))

    def generate_mod(self, mod: "Modulation", seed, first_frame, batch, ebn0_db, d_llr_ptr, llr_fmt="f32", qscale=0.0, d_msg_in_ptr=None, msg_fmt="bytes", d_msg_ptr=None,
                     stream=None):
        """transmit() and demap() in one kernel: LLRs [batch][N] in llr_fmt ("f32", "f16", "i8")"""
        check(lib().ldpc_sim_generate_mod(self._h, mod._h if mod is not None else None, int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr,
                                          self._bits_fmt(msg_fmt), d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), d_msg_ptr, stream))

    def transmit_il(self, mod: "Modulation", il: "Interleaver", seed, first_frame, batch, ebn0_db, d_sym_ptr, d_msg_in_ptr=None, msg_fmt="bytes", d_msg_ptr=None,
                    stream=None):
        """transmit() with the labels gathered through the table (ldpc_sim_transmit_il)"""
        check(lib().ldpc_sim_transmit_il(self._h, _h(mod), _h(il), int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr, self._bits_fmt(msg_fmt),
                                         d_sym_ptr, d_msg_ptr, stream))

    def generate_mod_il(self, mod: "Modulation", il: "Interleaver", seed, first_frame, batch, ebn0_db, d_llr_ptr, llr_fmt="f32", qscale=0.0, d_msg_in_ptr=None,
                        msg_fmt="bytes", d_msg_ptr=None, stream=None):
        """transmit_il() and demap_il() in one kernel (ldpc_sim_generate_mod_il)"""
        check(lib().ldpc_sim_generate_mod_il(self._h, _h(mod), _h(il), int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr, self._bits_fmt(msg_fmt),
                                             d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), d_msg_ptr, stream))

    def transmit_il_fading(self, mod: "Modulation", il: "Interleaver", fad: "Fading", seed, first_frame, batch, ebn0_db, d_sym_ptr, d_gain_ptr=None, d_msg_in_ptr=None,
                           msg_fmt="bytes", d_msg_ptr=None, stream=None):
        """transmit_il() over a fading channel (ldpc_sim_transmit_il_fading): the equalised samples, and the power gains [batch][n_sym]
        float32 at d_gain_ptr if given"""
        check(lib().ldpc_sim_transmit_il_fading(self._h, _h(mod), _h(il), _fad(fad), int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr,
                                                self._bits_fmt(msg_fmt), d_sym_ptr, d_gain_ptr, d_msg_ptr, stream))

    def generate_mod_il_fading(self, mod: "Modulation", il: "Interleaver", fad: "Fading", seed, first_frame, batch, ebn0_db, d_llr_ptr, llr_fmt="f32", qscale=0.0,
                               d_gain_ptr=None, d_msg_in_ptr=None, msg_fmt="bytes", d_msg_ptr=None, stream=None):
        """transmit_il_fading() and demap_il_csi() in one kernel (ldpc_sim_generate_mod_il_fading)"""
        check(lib().ldpc_sim_generate_mod_il_fading(self._h, _h(mod), _h(il), _fad(fad), int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr,
                                                    self._bits_fmt(msg_fmt), d_llr_ptr, _llr_fmt(llr_fmt), float(qscale), d_gain_ptr, d_msg_ptr, stream))

    def noise_var_rm(self, mod: "Modulation", rm: "Ratematch", ebn0_db):
        """noise_var() at the rate of one transmission through the table, R = k / E (ldpc_sim_noise_var_rm)"""
        return float(lib().ldpc_sim_noise_var_rm(self._h, _h(mod), _h(rm), float(ebn0_db)))

    def transmit_rm(self, mod: "Modulation", rm: "Ratematch", fad: "Fading", seed, first_frame, batch, ebn0_db, d_sym_ptr, d_gain_ptr=None, d_msg_in_ptr=None,
                    msg_fmt="bytes", d_msg_ptr=None, stream=None):
        """one transmission through a rate-matching table (ldpc_sim_transmit_rm): samples [batch][mod.symbols(rm.E)][2]; fad None: AWGN.
        A retransmission: the first round's messages as d_msg_in_ptr and another seed"""
        check(lib().ldpc_sim_transmit_rm(self._h, _h(mod), _h(rm), _fad(fad), int(seed), int(first_frame), int(batch), float(ebn0_db), d_msg_in_ptr,
                                         self._bits_fmt(msg_fmt), d_sym_ptr, d_gain_ptr, d_msg_ptr, stream))

    def tally(self, batch, d_bits_ptr, d_iters_ptr, d_tally_ptr, stream=None):
        check(lib().ldpc_sim_tally(self._h, int(batch), d_bits_ptr, d_iters_ptr, d_tally_ptr, stream))

    def crc_check(self, crc: "Crc", batch, d_bits_ptr, d_ok_ptr, bits_fmt="bytes", stream=None):
        """ldpc_sim_crc_check: Crc.check() straight on decoded codewords ([batch][N] bytes, or "packed" rows of ceil(N / 8) bytes): the flags
        of extract_messages() followed by crc.check(), with no message buffer in between"""
        check(lib().ldpc_sim_crc_check(self._h, _h(crc), int(batch), d_bits_ptr, self._bits_fmt(bits_fmt), d_ok_ptr, stream))

    def bch_decode(self, bch: "Bch", batch, d_bits_ptr, d_nerr_ptr, bits_fmt="bytes", stream=None):
        """ldpc_sim_bch_decode: Bch.decode() straight on decoded codewords ([batch][N] bytes, or "packed" rows of ceil(N / 8) bytes): BCH row
        bit i is decoded bit msg_pos[i], corrected where it lies; d_nerr [batch] int32"""
        check(lib().ldpc_sim_bch_decode(self._h, _h(bch), int(batch), d_bits_ptr, self._bits_fmt(bits_fmt), d_nerr_ptr, stream))

    def tally_crc(self, batch, d_bits_ptr, d_ok_ptr, d_tally_ptr, stream=None):
        """ldpc_sim_tally_crc: d_tally [4] uint64 += {frames, CRC passes, frames with a message-bit error, passes with an error (undetected)}"""
        check(lib().ldpc_sim_tally_crc(self._h, int(batch), d_bits_ptr, d_ok_ptr, d_tally_ptr, stream))

    def encode_host(self, msg, p):
        msg = np.ascontiguousarray(msg, np.uint8)
        par = np.zeros(p, np.uint8)
        check(lib().ldpc_sim_encode_host(self._h, ptr(msg, C.c_uint8), ptr(par, C.c_uint8)))
        return par

    def close(self):
        if self._h and self._owned:
            lib().ldpc_sim_destroy(self._h)
        self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class ECC:
    """The plug-in record mkLDPC builds (src/ECC/Code/LDPC/Utils.hs:59-75), by code name:
    ECC(codes_dir, "ldpc/hip-minsum/jpl.4096.4.5/50/4/5")."""

    def __init__(self, codes_dir, code_name, max_batch=64, replicas=1, devices=None):
        """replicas / devices: the reference's maxThreadCount decoder replicas in one process (Utils.hs:53), replica i on
        HIP device devices[i] (None: the calling thread's device)"""
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            replicas = len(devices)
        else:
            devs = None
        self._h = lib().ldpc_ecc_create_replicas(str(codes_dir).encode(), code_name.encode(), int(max_batch), int(replicas), devs)
        if not self._h:
            raise LdpcError(lib().ldpc_last_error_code(), last_error())
        _register(self)
        L = lib()
        self.name = L.ldpc_ecc_name(self._h).decode()
        self.message_length = L.ldpc_ecc_message_length(self._h)
        self.codeword_length = L.ldpc_ecc_codeword_length(self._h)
        self.unpunctured_length = L.ldpc_ecc_unpunctured_length(self._h)
        self.max_iters = L.ldpc_ecc_max_iters(self._h)
        self.code = Code(L.ldpc_ecc_code(self._h), owned=False)
        self.decoder = Decoder(self.code, max_batch=max_batch, _handle=L.ldpc_ecc_ctx(self._h))
        self.sim = Sim(self.code, self.message_length, self.codeword_length, _handle=L.ldpc_ecc_sim(self._h))

    def encode(self, msg):
        msg = np.ascontiguousarray(msg, np.uint8)
        assert msg.shape == (self.message_length,)
        cw = np.zeros(self.codeword_length, np.uint8)
        check(lib().ldpc_ecc_encode(self._h, ptr(msg, C.c_uint8), ptr(cw, C.c_uint8)))
        return cw

    def decode(self, llr, replica=None):
        """the record's decode (Utils.hs:62-72); replica None = picked by the calling thread, as the reference does"""
        llr = np.ascontiguousarray(llr, np.float64)
        assert llr.shape == (self.codeword_length,)
        out = np.zeros(self.message_length, np.uint8)
        ok = C.c_int()
        if replica is None:
            check(lib().ldpc_ecc_decode(self._h, ptr(llr, C.c_double), ptr(out, C.c_uint8), C.byref(ok)))
        else:
            check(lib().ldpc_ecc_decode_on(self._h, int(replica), ptr(llr, C.c_double), ptr(out, C.c_uint8), C.byref(ok)))
        return out, bool(ok.value)

    @property
    def replicas(self):
        return lib().ldpc_ecc_replicas(self._h)

    def replica(self, i):
        """-> (Decoder, Sim) views of replica i (owned by the record)"""
        L = lib()
        return (Decoder(self.code, max_batch=self.decoder.max_batch, _handle=L.ldpc_ecc_ctx_at(self._h, int(i))),
                Sim(self.code, self.message_length, self.codeword_length, _handle=L.ldpc_ecc_sim_at(self._h, int(i))))

    def coalescing_stats(self):
        """-> (decode calls, launches) through the batchers so far"""
        c, l = C.c_long(), C.c_long()
        check(lib().ldpc_ecc_coalescing_stats(self._h, C.byref(c), C.byref(l)))
        return c.value, l.value

    def set_coalescing(self, max_frames, max_wait_us=200):
        """concurrent decode() calls share launches (ldpc_batcher): up to max_frames per launch, a lone caller waits at
        most max_wait_us for company; 0 switches it off"""
        check(lib().ldpc_ecc_set_coalescing(self._h, int(max_frames), int(max_wait_us)))

    def close(self):
        if self._h:
            self.decoder._h = None
            self.sim._h = None
            self.code._h = None
            lib().ldpc_ecc_destroy(self._h)
            self._h = None

    def __del__(self):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass
