"""ctypes binding of libzethprover.so (include/zeth_prover.h) -- the host side of the C-ABI.

This is the Python stand-in for the Rust host BASELINE.json's north_star names (no Rust toolchain in
the image; INTEGRATION.md shows the equivalent `extern "C"` block).  It mirrors the boundary
one-to-one: every method is one zp_* call.  There is NO CPU fallback: if the HIP library is missing
or no GPU is present, construction raises.

Reference call sites this path serves: src/prover/provider.rs:358-390 (GenChunkProof) of eigen-zeth.
"""
from __future__ import annotations

import ctypes as C
import threading
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZP_LIB_PATH") or os.path.join(_HERE, "csrc", "libzethprover.so")  # override: A/B builds

P = 0xFFFFFFFF00000001
ROOT32_DEFAULT = 1753635133440165772
ROOT32_ALT = 7277203076849721926
SHIFT_DEFAULT = 49

ZP_CONST_ROOT32 = 1
ZP_CONST_POSEIDON_RC = 2
ZP_CONST_POSEIDON_MDS = 3
ZP_CONST_COSET_SHIFT = 4

_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p

# every symbol include/zeth_prover.h declares: (restype, argtypes)
class AggStatement(C.Structure):
    """zp_agg_statement: one kind of proof that can occur in an aggregated proof's tree"""
    _fields_ = [("shape_json", C.c_char_p), ("h_program", C.POINTER(C.c_uint64)), ("program_words", C.c_size_t), ("logn", C.c_int32), ("logb", C.c_int32),
                ("fri_logf", C.c_int32), ("fri_final_log", C.c_int32), ("n_queries", C.c_int32), ("pow_bits", C.c_int32), ("n_slots", C.c_int32)]


SIGNATURES = {
    "zp_create": (C.c_int32, [C.POINTER(_vp), C.c_int32]),
    "zp_destroy": (None, [_vp]),
    "zp_last_error": (C.c_char_p, [_vp]),
    "zp_version": (C.c_char_p, []),
    "zp_device_count": (C.c_int32, []),
    "zp_set_stream": (C.c_int32, [_vp, _vp]),
    "zp_get_stream": (C.c_int32, [_vp, C.POINTER(C.c_void_p)]),
    "zp_sync": (C.c_int32, [_vp]),
    "zp_set_constants": (C.c_int32, [_vp, C.c_int32, _u64p, C.c_size_t]),
    "zp_get_constants": (C.c_int32, [_vp, C.c_int32, _u64p, C.c_size_t]),
    "zp_dev_alloc": (C.c_int32, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "zp_dev_free": (C.c_int32, [_vp, _vp]),
    "zp_host_alloc": (C.c_int32, [_vp, C.c_size_t, C.POINTER(C.c_void_p)]),
    "zp_host_free": (C.c_int32, [_vp, _vp]),
    "zp_h2d": (C.c_int32, [_vp, _vp, _vp, C.c_size_t]),
    "zp_d2h": (C.c_int32, [_vp, _vp, _vp, C.c_size_t]),
    "zp_d2d": (C.c_int32, [_vp, _vp, _vp, C.c_size_t]),
    "zp_dev_zero": (C.c_int32, [_vp, _vp, C.c_size_t]),
    "zp_ntt": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "zp_intt": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "zp_twiddle_rows": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32]),
    "zp_lde": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64]),
    "zp_poseidon_perm": (C.c_int32, [_vp, _vp, C.c_size_t]),
    "zp_poseidon_trace": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t]),
    "zp_pow_grind": (C.c_int32, [_vp, _vp, C.c_int32, _vp]),
    "zp_stark_prove": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "zp_stark_prove_bn128": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "zp_poseidon_bn254_sponge": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp]),
    "zp_poseidon_bn254_sponge_caps": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp]),
    "zp_free_buffer": (C.c_int32, [_vp]),
    "zp_stark_set_air_kernel": (C.c_int32, [C.c_void_p, _u64p, C.c_size_t, C.c_void_p]),
    "zp_stark_set_air_kernel_rows": (C.c_int32, [C.c_void_p, _u64p, C.c_size_t, C.c_void_p]),
    "zp_stark_set_air_kernel_witness": (C.c_int32, [C.c_void_p, _u64p, C.c_size_t, C.c_void_p]),
    "zp_stark_set_air_kernel_witness_rows": (C.c_int32, [C.c_void_p, _u64p, C.c_size_t, C.c_void_p]),
    "zp_stark_prove_witness_report": (C.c_int32, [_vp, _u64p, _u64p, _u64p, _u64p, C.c_int32]),
    "zp_poseidon_sponge": (C.c_int32, [_vp, _u64p, _u64p, C.c_size_t, C.c_size_t, _u64p]),
    "zp_poseidon_sponge_caps": (C.c_int32, [_vp, _u64p, _u64p, C.c_size_t, C.c_size_t, _u64p, _u64p]),
    "zp_deep_quotient_rows": (C.c_int32, [_vp, _vp, C.c_int32, C.c_size_t, _vp, C.c_int32, C.c_size_t, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32,
                                          _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_size_t]),
    "zp_eval_quotient_rows": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int32, C.c_int32, C.c_size_t, C.c_size_t,
                                          _vp, C.c_int32, _vp, _vp, C.c_uint64, C.c_uint64, _vp, C.c_size_t]),
    "zp_set_poseidon_bn254": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    "zp_poseidon_bn254_perm": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32]),
    "zp_merkle16_nodes": (C.c_size_t, [C.c_size_t]),
    "zp_merkle16_commit_bn254": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32, _vp]),
    "zp_merkle16_open_bn254": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_size_t, _vp]),
    "zp_merkle16_open_batch_bn254": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, C.c_int32, _vp]),
    "zp_ntt_bn254": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    "zp_qap_quotient_bn254": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, _vp]),
    "zp_pack_blocks": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int32]),
    "zp_transpose": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_size_t]),
    "zp_synth_g1_points": (C.c_int32, [C.c_uint64, C.c_size_t, _vp, C.c_int32]),
    "zp_hbm_copy_probe": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_int32, C.POINTER(C.c_float)]),
    "zp_fixed_columns_words": (C.c_size_t, [_vp, C.c_size_t, C.c_int32, C.c_int32]),
    "zp_fixed_columns": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _vp, C.c_size_t]),
    "zp_eval_quotient": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_uint64,
                                     C.c_uint64, _vp]),
    "zp_merkle_commit": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32, _vp]),
    "zp_merkle_commit_rows": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_size_t, _vp]),
    "zp_merkle_open": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_size_t, _u64p]),
    "zp_fri_fold": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, _u64p, C.c_uint64]),
    "zp_poly_eval_ext": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _u64p, _u64p]),
    "zp_program_eval_ext": (C.c_int32, [_u64p, C.c_size_t, _u64p, C.c_int32, C.c_int32, C.c_uint64, _u64p, _u64p, _u64p, C.c_int32, _u64p, C.c_int32, C.c_int32]),
    "zp_program_fixed_eval_ext": (C.c_int32, [_u64p, C.c_size_t, _u64p, C.c_int32, C.c_int32, C.c_uint64, _u64p, _u64p, C.c_int32, C.c_int32]),
    "zp_poseidon_bn254_chains": (C.c_int32, [_vp, _u64p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_int32, C.c_int32, _u64p, _u64p, _u64p]),
    "zp_verify_counters": (C.c_int32, [_vp, _u64p]),
    "zp_aggregate_verify": (C.c_int32, [_vp, C.POINTER(AggStatement), C.c_int32, C.c_char_p, C.c_size_t, C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zp_aggregate_verify_batch": (C.c_int32, [_vp, C.POINTER(AggStatement), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int32, C.c_uint32, C.c_int32,
                                              C.POINTER(C.c_int32)]),
    "zp_program_fixed_eval_ext_batch": (C.c_int32, [_vp, _u64p, C.c_size_t, _u64p, C.c_int32, C.c_int32, C.c_uint64, _u64p, C.c_int32, _u64p, C.c_int32,
                                                    C.POINTER(C.c_uint8), C.c_int32]),
    "zp_ood_eval": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_uint64, _u64p, C.c_int32, _u64p, _u64p]),
    "zp_deep_quotient": (C.c_int32, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _u64p, _u64p, _u64p,
                                     _u64p, _u64p, C.c_uint64, _vp]),
    "zp_grand_product": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, _u64p, _vp]),
    "zp_logup_columns": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_size_t, _u64p, _vp]),
    "zp_gather_rows": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32, _u64p, C.c_int32, _u64p]),
    "zp_merkle_open_batch": (C.c_int32, [_vp, _vp, C.c_size_t, _u64p, C.c_int32, _u64p]),
    "zp_domain_tables": (C.c_int32, [_vp, C.c_int32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int32)]),
    "zp_synth_trace": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _u64p, _u64p]),
    "zp_synth_trace_bound": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _u64p, C.c_int32, _u64p, _u64p]),
    "zp_synth_checkpoint_words": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "zp_synth_checkpoints": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _u64p, _u64p, C.c_int32, C.c_void_p]),
    "zp_synth_trace_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _u64p, C.c_int32, C.c_void_p, C.c_void_p, _u64p]),
    "zp_json_key_span": (C.c_int32, [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "zp_proof_queries_scan": (C.c_int32, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), _vp, _vp, C.c_int32]),
    "zp_proof_queries_parse": (C.c_int32, [C.c_char_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "zp_verifier_arith_host": (C.c_int32, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32]),
    "zp_verifier_arith_trace": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32]),
    "zp_fixed_base_mul_bn254": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_int32]),
    "zp_fixed_base_mul_bn254_g2": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_int32]),
    "zp_r1cs_eval": (C.c_int32, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zp_r1cs_key_scalars": (C.c_int32, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_int32]),
    "zp_stark_openings": (C.c_int32, [_vp, _vp, _vp]),
    "zp_wrap_assign": (C.c_int32, [_vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "zp_wrap_aux": (C.c_int32, [_vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_uint64, _vp, _vp, C.c_size_t, _vp, _vp]),
    "zp_groth16_prove": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zp_sha256": (C.c_int32, [_vp, C.c_size_t, _vp]),
    "zp_r1cs_eval_device": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zp_program_digest": (C.c_int32, [_vp, C.c_size_t, _vp, _vp]),
    "zp_recursion_witness": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int32]),
    "zp_recursion_publics_words": (C.c_size_t, [_vp, C.c_size_t]),
    "zp_comm_unique_id": (C.c_int32, [_vp]),
    "zp_comm_create": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, C.POINTER(_vp)]),
    "zp_comm_destroy": (C.c_int32, [_vp]),
    "zp_comm_rank": (C.c_int32, [_vp]),
    "zp_comm_world": (C.c_int32, [_vp]),
    "zp_comm_info": (C.c_int32, [_vp, _vp]),
    "zp_comm_release_scratch": (C.c_int32, [_vp]),
    "zp_comm_abort": (C.c_int32, [_vp]),
    "zp_comm_set_timeout_ms": (C.c_int32, [_vp, C.c_int32]),
    "zp_comm_all_to_all": (C.c_int32, [_vp, _vp, _vp, C.c_size_t]),
    "zp_comm_all_gather": (C.c_int32, [_vp, _vp, _vp, C.c_size_t]),
    "zp_comm_broadcast": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32]),
    "zp_comm_all_reduce_sum": (C.c_int32, [_vp, _vp, C.c_size_t]),
    "zp_comm_group_create": (C.c_int32, [C.c_int32, C.POINTER(_vp)]),
    "zp_comm_group_destroy": (C.c_int32, [_vp]),
    "zp_comm_create_local": (C.c_int32, [_vp, C.c_int32, _vp, C.POINTER(_vp)]),
    "zp_stark_prove_sharded": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "zp_stark_prove_sharded_bn128": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "zp_exchange_columns_to_rows": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp]),
    "zp_ntt_sharded": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32]),
    "zp_merkle_commit_sharded": (C.c_int32, [_vp, _vp, C.c_size_t, C.c_int32, _vp, _u64p]),
    "zp_msm_bn254_sharded": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint32)]),
    "zp_msm_bn254_g2_sharded": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint32)]),
    "zp_groth16_prove_sharded": (C.c_int32, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _vp]),
    "zp_msm_bn254": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint32)]),
    "zp_msm_bn254_g2": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint32)]),
    "zp_ntt_host": (C.c_int32, [_vp, _u64p, C.c_int32, C.c_int32, C.c_int32]),
    "zp_lde_host": (C.c_int32, [_vp, _u64p, _u64p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64]),
    "zp_merkle_commit_host": (C.c_int32, [_vp, _u64p, C.c_size_t, C.c_int32, _u64p]),
    "zp_stark_verify": (C.c_int32, [_vp, _u64p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                    C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u64p]),
    "zp_stark_verify_batch": (C.c_int32, [_vp, _u64p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.POINTER(C.c_int32)]),
    "zp_merkle_verify_batch": (C.c_int32, [_vp, _u64p, C.c_size_t, _u64p, _u64p, C.c_int32, _u64p, C.c_size_t, C.POINTER(C.c_uint8)]),
    "zp_stark_verify_bn128": (C.c_int32, [_vp, _u64p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _u64p, _u64p,
                                          C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u64p]),
    "zp_stark_verify_batch_bn128": (C.c_int32, [_vp, _u64p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, _u64p, _u64p, C.c_uint32, C.c_int32, C.POINTER(C.c_int32)]),
    "zp_merkle16_verify_batch_bn254": (C.c_int32, [_vp, _u64p, C.c_size_t, _u64p, _u64p, C.c_size_t, _u64p, C.c_size_t, C.POINTER(C.c_uint8)]),
    "zp_set_tuning": (C.c_int32, [_vp, C.c_char_p, C.c_int32]),
    "zp_set_profiling": (C.c_int32, [_vp, C.c_int32]),
    "zp_get_pass_timings": (C.c_int32, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32,
                                        C.POINTER(C.c_int32)]),
    "zp_stage_timings": (C.c_int32, [_vp, C.c_char_p, C.c_size_t]),
    "zp_ntt_plan_json": (C.c_int32, [_vp, C.c_int32, C.c_char_p, C.c_size_t]),
    "zp_device_info_json": (C.c_int32, [_vp, C.c_char_p, C.c_size_t]),
    "zp_pairing_bn254": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_int32, _vp, _vp]),
    "zp_pairing_check_bn254": (C.c_int32, [_vp, _vp, _vp, C.c_size_t, C.c_int32, C.POINTER(C.c_int32)]),
    "zp_groth16_verify": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.POINTER(C.c_int32)]),
    "zp_groth16_verify_batch": (C.c_int32, [_vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, C.c_int32, _vp]),
    "zp_stark_check_witness": (C.c_int32, [_vp, _u64p, C.c_size_t, _vp, C.c_size_t, _u64p, C.c_int32, C.c_int32, _u64p, _u64p, _u64p, _u64p, C.c_int32, C.c_int32]),
    "zp_stark_diagnose_stage2": (C.c_int32, [_vp, _u64p, C.c_size_t, _vp, C.c_size_t, C.c_int32, _u64p, C.c_int32, C.c_int32]),
    "zp_stark_check_witness_sharded": (C.c_int32, [_vp, _u64p, C.c_size_t, _vp, C.c_size_t, _u64p, C.c_int32, C.c_int32, _u64p, _u64p, _u64p, _u64p, C.c_int32]),
}


def synth_g1_points(n, start=1025, threads=0):
    """uint32 [n][16]: n distinct BN254 G1 points (start + i) * G in the zp_msm_bn254 layout (host generator of the library)"""
    out = np.empty((n, 16), dtype=np.uint32)
    rc = load_library().zp_synth_g1_points(start, n, out.ctypes.data, threads)
    if rc != 0:
        raise ValueError("zp_synth_g1_points: bad arguments (start must exceed 1024)")
    return out


BIND_SLOTS = {0: 2, 1: 4, 3: 6}     # trace kind -> starting values a caller may dictate (zp_synth_trace_bound)


def synth_trace(kind, logn, W, seed, out=None, bind=None):
    """synthetic witness (host code inside the library, no GPU needed): (trace [W][N], publics);
    `out`: optional uint64 [W][N] array to fill (e.g. page-locked memory from Prover.host_array);
    `bind`: starting values dictated by the caller (the block statement's limbs) -- they come back as public inputs"""
    lib = load_library()
    tr = np.empty((W, 1 << logn), dtype=np.uint64) if out is None else out
    assert tr.shape == (W, 1 << logn) and tr.dtype == np.uint64 and tr.flags["C_CONTIGUOUS"]
    pub = np.zeros(8, dtype=np.uint64)
    if bind is not None and len(bind):
        b = np.ascontiguousarray(np.asarray(bind, dtype=np.uint64))
        rc = lib.zp_synth_trace_bound(kind, logn, W, seed, b.ctypes.data_as(_u64p), len(b), tr.ctypes.data_as(_u64p), pub.ctypes.data_as(_u64p))
    else:
        rc = lib.zp_synth_trace(kind, logn, W, seed, tr.ctypes.data_as(_u64p), pub.ctypes.data_as(_u64p))
    if rc != 0:
        raise ValueError("zp_synth_trace: bad arguments")
    return tr, pub[:{0: 3, 2: 1, 3: 8}.get(kind, min(4, W))].copy()


class ZpError(RuntimeError):
    """bad: the row or wire a refusal of the R1CS evaluators names (*bad of zp_r1cs_eval / zp_r1cs_eval_device), None elsewhere"""

    def __init__(self, code, msg, bad=None):
        super().__init__("libzethprover error %d: %s" % (code, msg))
        self.code = code
        self.bad = bad


_lib = None


def load_library():
    """dlopen the HIP library and bind every declared symbol.  Raises if the .so is missing --
    the product path never degrades to a CPU implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libzethprover.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C eigen_zeth_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(x):
    """device pointer of a DeviceBuffer / torch tensor / raw int"""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class DeviceBuffer:
    """u64 device array owned through zp_dev_alloc / zp_dev_free"""

    def __init__(self, prover, n_elems):
        self.prover = prover
        self.n = int(n_elems)
        self.shape = (self.n,)
        if prover.pooling:
            with prover._lock:
                pool = prover._pool.get(self.n)
                if pool:
                    self.ptr = pool.pop()     # reuse: hipMalloc/hipFree and the first touch of fresh memory are slow
                    return
        p = _vp()
        prover._chk(prover.lib.zp_dev_alloc(prover.ctx, self.n * 8, C.byref(p)))
        self.ptr = p.value or 0

    def offset(self, elems):
        return self.ptr + 8 * int(elems)

    def free(self):
        if self.ptr and self.prover.ctx:
            if self.prover.pooling and self.n >= 1024:
                with self.prover._lock:
                    self.prover._pool.setdefault(self.n, []).append(self.ptr)
            else:
                self.prover.lib.zp_dev_free(self.prover.ctx, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count():
    """visible HIP devices, through the library (no torch: a process that loads the system RCCL must not import torch's copy later)"""
    return int(load_library().zp_device_count())


def fr_words(vals):
    """ints < 2^256 -> u64[n][4] (little-endian words, standard form)"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def fr_ints(a):
    raw = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 4)).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def r1cs_eval(blob, witness, mask):
    """zp_r1cs_eval: witness u64[n_wires][4] with `mask` (bytes) saying which wires the caller set -> (completed witness, a_ev, b_ev, c_ev each
    u64[2^logm][4]); raises ValueError when the assignment does not satisfy the circuit"""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    w = np.ascontiguousarray(witness, dtype=np.uint64).copy()
    st = np.ascontiguousarray(mask, dtype=np.uint8).copy()
    m = 1 << int(blob[3])
    ev = [np.empty((m, 4), dtype=np.uint64) for _ in range(3)]
    bad = C.c_int64(-1)
    rc = load_library().zp_r1cs_eval(blob.ctypes.data, blob.size, w.ctypes.data, st.ctypes.data, ev[0].ctypes.data, ev[1].ctypes.data, ev[2].ctypes.data,
                                     C.byref(bad))
    if rc == -20:
        raise ValueError("the assignment does not satisfy the circuit (constraint %d): no proof for a false statement" % bad.value)
    if rc != 0:
        raise ZpError(rc, "zp_r1cs_eval: malformed circuit or unset wire (%d)" % bad.value, bad=bad.value)
    return w, ev[0], ev[1], ev[2]


def wrap_assign(script, openings, aux):
    """zp_wrap_assign: (wire indices u64[n], values u64[n][4]) of the caller-set wires of the wrap circuit, from the binary openings of a final STARK.
    aux: the element the proof is bound to (an int), or the list [that element, further elements the circuit takes from its caller ...]"""
    script = np.ascontiguousarray(script, dtype=np.uint64)
    openings = np.ascontiguousarray(openings, dtype=np.uint64)
    cap = int(script[2])
    idx, val = np.empty(cap, dtype=np.uint64), np.empty((cap, 4), dtype=np.uint64)
    aux = [int(v) for v in aux] if isinstance(aux, (list, tuple)) else [int(aux)]
    a = fr_words(aux)
    n = C.c_size_t(0)
    rc = load_library().zp_wrap_assign(script.ctypes.data, script.size, openings.ctypes.data, openings.size, a.ctypes.data, len(aux), idx.ctypes.data, val.ctypes.data,
                                       cap, C.byref(n))
    if rc != 0:
        raise ValueError("final STARK does not have the shape the wrap circuit was built for")
    return idx[:n.value], val[:n.value]


def program_eval_ext(program, pubchal, logn, root32, zeta, ev_z, ev_zw, threads=0):
    """zp_program_eval_ext: the K constraints of a program at the out-of-domain point, u64[K][3] (host code; ValueError: malformed input)"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    pc = np.ascontiguousarray(np.array([int(v) for v in pubchal] or [0], dtype=np.uint64))
    z = np.array([int(v) for v in zeta], dtype=np.uint64)
    ez, ezw = np.ascontiguousarray(np.asarray(ev_z, dtype=np.uint64)), np.ascontiguousarray(np.asarray(ev_zw, dtype=np.uint64))
    out = np.zeros((int(prog[8]), 3), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(_u64p)
    if ez.shape != ezw.shape or ez.ndim != 2 or ez.shape[1] != 3:
        raise ValueError("zp_program_eval_ext: evaluations must be two [columns][3] arrays")
    rc = load_library().zp_program_eval_ext(p(prog), prog.size, p(pc), len(pubchal), logn, int(root32), p(z), p(ez), p(ezw), ez.shape[0], p(out), out.shape[0],
                                            threads)
    if rc != 0:
        raise ValueError("zp_program_eval_ext: malformed program or evaluations (%d)" % rc)
    return out


WITNESS_SATISFIED, WITNESS_VIOLATED, WITNESS_NONCANONICAL = range(3)
ZP_ERR_WITNESS = -7     # zp_stark_prove / zp_stark_prove_bn128 / the sharded provers under set_tuning("prove_check", 1): a false witness, no proof (include/zeth_prover.h)
_NONE64 = (1 << 64) - 1


class WitnessReport:
    """what zp_stark_check_witness says of a trace: ok / verdict (WITNESS_*); first_row and first_constraint (the smallest violated row, the smallest
    violated constraint on it; None when nothing is violated); violations (violated (row, constraint) pairs); violated_constraints (distinct ones);
    counts[k] (rows at which constraint k is violated) and first_rows[k] (the smallest such row or None); noncanonical (trace words >= p) and
    first_noncanonical ((column, row) of the first in memory order, or None)"""

    def __init__(self, report, counts, first_rows):
        opt = lambda v: None if int(v) == _NONE64 else int(v)
        self.verdict = int(report[0])
        self.ok = self.verdict == WITNESS_SATISFIED
        self.first_row, self.first_constraint = opt(report[1]), opt(report[2])
        self.violations, self.violated_constraints, self.noncanonical = int(report[3]), int(report[4]), int(report[5])
        self.first_noncanonical = None if int(report[6]) == _NONE64 else (int(report[6]), int(report[7]))
        self.counts = [int(v) for v in counts]
        self.first_rows = [opt(v) for v in first_rows]

    def __str__(self):
        if self.verdict == WITNESS_NONCANONICAL:
            return "witness not canonical: %d trace word(s) >= p, the first in column %d at row %d" % ((self.noncanonical,) + self.first_noncanonical)
        if self.ok:
            return "witness satisfies all %d constraints" % len(self.counts)
        return "witness violates constraint %d at row %d (that constraint at %d row(s); %d constraint(s) violated, %d violations in all)" % (
            self.first_constraint, self.first_row, self.counts[self.first_constraint], self.violated_constraints, self.violations)


class WitnessError(ValueError):
    """a trace that does not satisfy its constraint program was handed to a prover that checks first; .report: the WitnessReport (.report.chal: the
    stage-2 challenge it was judged at, when the check ran inside a proof)"""

    def __init__(self, report):
        super().__init__(str(report))
        self.report = report
        self.stage2 = None      # [Stage2Diagnosis] per stage-2 argument, where whoever raised it was asked to diagnose (EngineConfig(diagnose_stage2=True))


S2_HOLDS, S2_FAILS, S2_NONCANONICAL = range(3)
S2_WORDS = 12


class Stage2Diagnosis:
    """one record of zp_stark_diagnose_stage2 (include/zeth_prover.h): verdict (S2_*) / ok; kind (1 permutation, 2 lookup); unbalanced (distinct
    values v with lhs(v) != rhs(v)); row_a, value_a, lhs_a, rhs_a: the smallest row of column a holding an unbalanced value, that value, its
    occurrences in a and its count on the other side (occurrences in b; the sum of m over the rows with t = v, mod p) -- None when there is no such
    row; row_b, value_b, lhs_b, rhs_b: the same for the smallest row of b (t); rows_a: rows of a holding an unbalanced value; words: the record"""

    def __init__(self, words):
        w = self.words = [int(v) for v in words]
        self.verdict, self.kind, self.unbalanced, self.rows_a = w[0], w[1], w[2], w[11]
        self.ok = self.verdict == S2_HOLDS
        self.row_a, self.value_a, self.lhs_a, self.rhs_a = w[3:7] if w[3] != _NONE64 else (None,) * 4
        self.row_b, self.value_b, self.lhs_b, self.rhs_b = w[7:11] if w[7] != _NONE64 else (None,) * 4

    def __str__(self):
        what = {1: "permutation", 2: "lookup"}.get(self.kind, "argument")
        if self.verdict == S2_NONCANONICAL:
            return "%s not compared: the trace holds words >= p" % what
        if self.ok:
            return "%s holds" % what
        side = lambda name, r, v, l, h: "" if r is None else "; %s row %d holds %d (%d in a, %d on the other side)" % (name, r, v, l, h)
        return "%s fails: %d unbalanced value(s) on %d row(s) of a%s%s" % (
            what, self.unbalanced, self.rows_a, side("a", self.row_a, self.value_a, self.lhs_a, self.rhs_a),
            side("b" if self.kind == 1 else "t", self.row_b, self.value_b, self.lhs_b, self.rhs_b))


def _diagnose_stage2(ctx, program, trace_ptr, trace_words, logn, threads):
    prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
    if prog.ndim != 1 or prog.size < 12 or int(prog[10]) > (1 << 16):
        return -1, None
    n = int(prog[10])
    diag = np.zeros(max(n, 1) * S2_WORDS, dtype=np.uint64)
    rc = load_library().zp_stark_diagnose_stage2(ctx, prog.ctypes.data_as(_u64p), prog.size, trace_ptr, trace_words, logn, diag.ctypes.data_as(_u64p), n, threads)
    return rc, ([Stage2Diagnosis(diag[S2_WORDS * j:S2_WORDS * (j + 1)]) for j in range(n)] if rc == 0 else None)


def diagnose_stage2_host(program, trace, logn, threads=0):
    """zp_stark_diagnose_stage2 without a ctx: host trace uint64 [W][2^logn] (or flat) -> [Stage2Diagnosis], one per stage-2 argument of the program in
    its table's order (none: []).  Names the rows and values that break a permutation or a lookup, which zp_stark_check_witness reports at row N - 1.
    ZpError: a malformed blob or argument"""
    tr = np.ascontiguousarray(np.asarray(trace, dtype=np.uint64))
    rc, out = _diagnose_stage2(None, program, tr.ctypes.data, tr.size, logn, threads)
    if rc != 0:
        raise ZpError(rc, "zp_stark_diagnose_stage2: malformed program, or a trace that is not the program's")
    return out


def _check_witness(ctx, program, trace_ptr, trace_words, pubs, logn, chal, threads, comm=None):
    """comm: a zp_comm handle -- zp_stark_check_witness_sharded on it (trace_ptr = this rank's columns) instead of zp_stark_check_witness on ctx"""
    prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
    if prog.ndim != 1 or prog.size < 12:
        return -1, None
    K = int(prog[8])
    if K > (1 << 24):
        return -1, None
    pb = np.ascontiguousarray(np.asarray([int(v) for v in pubs] + [0], dtype=np.uint64))
    ch = None if chal is None else np.ascontiguousarray(np.asarray([int(v) for v in chal], dtype=np.uint64))
    if ch is not None and ch.size != 3:
        return -1, None
    rep, counts, first = np.zeros(8, dtype=np.uint64), np.zeros(max(K, 1), dtype=np.uint64), np.zeros(max(K, 1), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(_u64p)
    head = (p(prog), prog.size, trace_ptr, trace_words, p(pb), len(pb) - 1, logn, None if ch is None else p(ch), p(rep), p(counts), p(first), K)
    rc = load_library().zp_stark_check_witness_sharded(comm, *head) if comm is not None else load_library().zp_stark_check_witness(ctx, *head, threads)
    return rc, (WitnessReport(rep, counts[:K], first[:K]) if rc == 0 else None)


def check_witness_host(program, trace, pubs, logn, chal=None, threads=0):
    """zp_stark_check_witness without a ctx: host trace uint64 [W][2^logn] (or flat) against the program, on `threads` host threads -> WitnessReport.
    chal: the stage-2 challenge (3 canonical words), None = derived from the program.  ZpError: a malformed blob or argument"""
    tr = np.ascontiguousarray(np.asarray(trace, dtype=np.uint64))
    rc, rep = _check_witness(None, program, tr.ctypes.data, tr.size, pubs, logn, chal, threads)
    if rc != 0:
        raise ZpError(rc, "zp_stark_check_witness: malformed program, or a trace / public inputs / challenge that are not the program's")
    return rep


# zp_stark_verify: the verdict classes and the flags (include/zeth_prover.h)
VERDICT_ACCEPT, VERDICT_MALFORMED, VERDICT_PARAMS, VERDICT_IDENTITY, VERDICT_POW, VERDICT_INDICES, VERDICT_FINAL_DEGREE, VERDICT_OPENING, VERDICT_FRI = range(9)
VERIFY_HEADER_ONLY, VERIFY_TRUST_OPENINGS = 1, 2
VERDICT_TRANSCRIPT, VERDICT_PUBLICS, VERDICT_TREE = 9, 10, 11      # zp_aggregate_verify*; PUBLICS also groth16_verify*
VERDICT_POINT, VERDICT_PAIRING = 12, 13                             # groth16_verify* only



def _verify_params(params):
    d = params.to_dict() if hasattr(params, "to_dict") else dict(params)
    if d.get("hash", "gl") != "gl":
        raise ValueError("zp_stark_verify reads Goldilocks-mode proofs")
    return [int(d[k]) for k in ("logn", "logb", "fri_logf", "fri_final_log", "n_queries")] + [int(d.get("pow_bits", 0))]


def _verify_error(prover, rc, what):
    if prover is not None:
        prover._chk(rc)
    raise ZpError(rc, what + ": bad arguments, a malformed program blob or a proof in BN128-hash mode")


def stark_verify(program, text, params, flags=0, prover=None, threads=0):
    """zp_stark_verify: (verdict, where, indices) of a chunk proof TEXT (str or bytes) of the statement `program` under the verifier's own
    `params` (StarkParams or its dict).  verdict: VERDICT_*; where: the first failing query or -1; indices: the query indices the transcript
    dictates (None when a check before them failed).  prover = None: on the host, default tables and domain; otherwise through that ctx"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    raw = text.encode() if isinstance(text, str) else bytes(text)
    pv = _verify_params(params)
    idx = np.zeros(pv[4], dtype=np.uint64)
    verdict, where = C.c_int32(0), C.c_int32(-1)
    rc = load_library().zp_stark_verify(prover.ctx if prover is not None else None, prog.ctypes.data_as(_u64p), prog.size, raw, len(raw), *pv, int(flags), threads,
                                        C.byref(verdict), C.byref(where), idx.ctypes.data_as(_u64p))
    if rc != 0:
        _verify_error(prover, rc, "zp_stark_verify")
    got = verdict.value == VERDICT_ACCEPT or verdict.value >= VERDICT_INDICES      # when the library writes the indices (include/zeth_prover.h)
    return verdict.value, where.value, ([int(v) for v in idx] if got else None)


def stark_verify_batch(program, texts, params, flags=0, prover=None, threads=0):
    """zp_stark_verify_batch: the verdicts of several proof texts of one statement and parameter set (the openings of all of them in one launch)"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    raws = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    n = len(raws)
    ptrs, lens, out = (C.c_char_p * n)(*raws), (C.c_size_t * n)(*[len(r) for r in raws]), (C.c_int32 * n)()
    rc = load_library().zp_stark_verify_batch(prover.ctx if prover is not None else None, prog.ctypes.data_as(_u64p), prog.size, ptrs, lens, n, *_verify_params(params),
                                              int(flags), threads, out)
    if rc != 0:
        _verify_error(prover, rc, "zp_stark_verify_batch")
    return list(out)


def _verify_params_bn128(params, prover, bn_tables):
    """[logn, logb, fri_logf, fri_final_log, n_queries, rp, h_rc, h_mds] of a BN128-mode call, and what keeps the tables alive"""
    d = params.to_dict() if hasattr(params, "to_dict") else dict(params)
    pv = [int(d[k]) for k in ("logn", "logb", "fri_logf", "fri_final_log", "n_queries")]
    if prover is not None:
        return pv + [0, None, None], None
    if bn_tables is None:
        raise ValueError("zp_stark_verify_bn128 without a ctx needs the t = 17 tables: bn_tables = (rc, mds, rp)")
    rc, mds, rp = bn_tables
    flat = [v for row in mds for v in row] if isinstance(mds[0], (list, tuple)) else list(mds)
    keep = (Prover._fr_words(rc), Prover._fr_words(flat))
    return pv + [int(rp), keep[0].ctypes.data_as(_u64p), keep[1].ctypes.data_as(_u64p)], keep


def stark_verify_bn128(program, text, params, flags=0, prover=None, threads=0, bn_tables=None):
    """zp_stark_verify_bn128: (verdict, where, indices) of a BN128-hash-mode proof TEXT, as stark_verify gives them.  prover = None: on the host with
    bn_tables = (rc, mds, rp) of the t = 17 instance (poseidon_constants.bn254_poseidon_params(17)); otherwise through that ctx and the tables
    installed on it (install_poseidon_bn254(17))"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    raw = text.encode() if isinstance(text, str) else bytes(text)
    pv, keep = _verify_params_bn128(params, prover, bn_tables)
    idx = np.zeros(pv[4], dtype=np.uint64)
    verdict, where = C.c_int32(0), C.c_int32(-1)
    rc = load_library().zp_stark_verify_bn128(prover.ctx if prover is not None else None, prog.ctypes.data_as(_u64p), prog.size, raw, len(raw), *pv, int(flags), threads,
                                              C.byref(verdict), C.byref(where), idx.ctypes.data_as(_u64p))
    del keep
    if rc != 0:
        _verify_error(prover, rc, "zp_stark_verify_bn128")
    got = verdict.value == VERDICT_ACCEPT or verdict.value >= VERDICT_INDICES
    return verdict.value, where.value, ([int(v) for v in idx] if got else None)


def stark_verify_batch_bn128(program, texts, params, flags=0, prover=None, threads=0, bn_tables=None):
    """zp_stark_verify_batch_bn128: the verdicts of several BN128-mode proof texts of one statement and parameter set (every hash of every opening in one launch)"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    raws = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    n = len(raws)
    pv, keep = _verify_params_bn128(params, prover, bn_tables)
    ptrs, lens, out = (C.c_char_p * n)(*raws), (C.c_size_t * n)(*[len(r) for r in raws]), (C.c_int32 * n)()
    rc = load_library().zp_stark_verify_batch_bn128(prover.ctx if prover is not None else None, prog.ctypes.data_as(_u64p), prog.size, ptrs, lens, n, *pv, int(flags), threads, out)
    del keep
    if rc != 0:
        _verify_error(prover, rc, "zp_stark_verify_batch_bn128")
    return list(out)


def poseidon_bn254_chains(blocks, absorb, first, prover=None, bn_tables=None):
    """zp_poseidon_bn254_chains: sponge chains of the width-17 transcript.  blocks u64[nsteps][16][4] (standard form, < r), absorb u8[nsteps],
    first u32[nchains + 1] -> rates u64[nsteps][16][4], the rate after every step.  Chain c starts from the zero state and walks the steps
    [first[c], first[c + 1]); a step overwrites the rate with its block when absorb says so, then permutes.  prover = None: on the host with
    bn_tables = (rc, mds, rp); otherwise one launch on that ctx with the tables installed on it"""
    fi = np.ascontiguousarray(first, dtype=np.uint32).reshape(-1)
    ab = np.ascontiguousarray(absorb, dtype=np.uint8).reshape(-1)
    bl = np.ascontiguousarray(blocks, dtype=np.uint64).reshape(-1)
    rates = np.zeros(max(bl.size, 1), dtype=np.uint64)
    tb, keep = _verify_params_bn128({"logn": 0, "logb": 0, "fri_logf": 0, "fri_final_log": 0, "n_queries": 0}, prover, bn_tables)
    rc = load_library().zp_poseidon_bn254_chains(prover.ctx if prover is not None else None, bl.ctypes.data_as(_u64p) if bl.size else None,
                                                 ab.ctypes.data_as(C.POINTER(C.c_uint8)) if ab.size else None, fi.ctypes.data_as(C.POINTER(C.c_uint32)) if fi.size else None,
                                                 fi.size - 1, *tb[5:], rates.ctypes.data_as(_u64p))
    del keep
    if rc != 0:
        if prover is not None:
            prover._chk(rc)
        raise ZpError(rc, "zp_poseidon_bn254_chains: bad arguments")
    return rates[:bl.size].reshape(-1, 16, 4)


def verify_counters(prover):
    """zp_verify_counters: what the verifier calls of this ctx ran where since it was made -- {"launches": chain launches, "steps": chain steps run on
    the device, "digests": public-input commitments made on the device, "fallbacks": texts that took the host sponge on the device path}"""
    out = np.zeros(4, dtype=np.uint64)
    prover._chk(load_library().zp_verify_counters(prover.ctx, out.ctypes.data_as(_u64p)))
    return dict(zip(("launches", "steps", "digests", "fallbacks"), (int(v) for v in out)))


def agg_statements(entries):
    """the zp_agg_statement table of zp_aggregate_verify* from (shape dict or None, program, params, n_slots) tuples: shape None is the leaf statement
    (chunk proofs; n_slots ignored), otherwise the dictionary a node carries under "shape" with the verifier AIR's program for inner proofs of that shape,
    the verifier's StarkParams (or its dict) of a STARK over it and the query slots of its trace.  Returns (table, what keeps its pointers alive)"""
    import json
    table, keep = (AggStatement * len(entries))(), []
    for st, (shape, program, params, n_slots) in zip(table, entries):
        prog = np.ascontiguousarray(program, dtype=np.uint64)
        text = None if shape is None else json.dumps(shape).encode()
        keep += [prog, text]
        st.shape_json, st.h_program, st.program_words = text, prog.ctypes.data_as(C.POINTER(C.c_uint64)), prog.size
        st.logn, st.logb, st.fri_logf, st.fri_final_log, st.n_queries, st.pow_bits = _verify_params(params)
        st.n_slots = int(n_slots or 0)
    return table, keep


def aggregate_verify(statements, text, flags=0, prover=None, threads=0):
    """zp_aggregate_verify: (verdict, where) of an aggregated proof TEXT (str or bytes) of any level under the statements `statements` (tuples as
    agg_statements takes them).  verdict: VERDICT_*; where: the pre-order number of the failing node, -1 for the outer STARK.  prover = None: on the host"""
    table, keep = agg_statements(statements)
    raw = text.encode() if isinstance(text, str) else bytes(text)
    verdict, where = C.c_int32(-1), C.c_int32(-1)
    rc = load_library().zp_aggregate_verify(prover.ctx if prover is not None else None, table, len(table), raw, len(raw), int(flags), threads, C.byref(verdict), C.byref(where))
    del keep
    if rc != 0:
        _verify_error(prover, rc, "zp_aggregate_verify")
    return verdict.value, where.value


def aggregate_verify_batch(statements, texts, flags=0, prover=None, threads=0):
    """zp_aggregate_verify_batch: the verdicts of several aggregated proof texts under one table of statements: the fixed columns of every header of
    every text in one evaluation per statement, the openings of the outer STARKs in one launch per statement"""
    table, keep = agg_statements(statements)
    raws = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    n = len(raws)
    ptrs, lens, out = (C.c_char_p * n)(*raws), (C.c_size_t * n)(*[len(r) for r in raws]), (C.c_int32 * n)()
    rc = load_library().zp_aggregate_verify_batch(prover.ctx if prover is not None else None, table, len(table), ptrs, lens, n, int(flags), threads, out)
    del keep
    if rc != 0:
        _verify_error(prover, rc, "zp_aggregate_verify_batch")
    return list(out)


# ---- the BN254 pairing and the Groth16 verifier (csrc/pairing.hip): host code, with or without a Prover
PAIRING_STATUS_OK, PAIRING_STATUS_RANGE, PAIRING_STATUS_CURVE, PAIRING_STATUS_SUBGROUP = range(4)


def _pairs(g1, g2):
    a = np.ascontiguousarray(np.asarray(g1, dtype=np.uint32).reshape(-1, 16))
    b = np.ascontiguousarray(np.asarray(g2, dtype=np.uint32).reshape(-1, 32))
    if a.shape[0] != b.shape[0]:
        raise ValueError("as many G1 as G2 points")
    return a, b


def pairing_bn254(g1, g2, prover=None, threads=0):
    """zp_pairing_bn254: (gt u32[n][12][8], status u8[n]) of n pairs in the MSM point layouts (u32[n][16], u32[n][32]; all-zero = infinity).  gt[j] are
    the flat-basis words of e(P_j, Q_j), all-zero unless status[j] is PAIRING_STATUS_OK"""
    a, b = _pairs(g1, g2)
    n = a.shape[0]
    gt, st = np.zeros((n, 12, 8), dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    rc = load_library().zp_pairing_bn254(prover.ctx if prover is not None else None, a.ctypes.data, b.ctypes.data, n, threads, gt.ctypes.data, st.ctypes.data)
    if rc != 0:
        _verify_error(prover, rc, "zp_pairing_bn254")
    return gt, st


def pairing_check_bn254(g1, g2, prover=None, threads=0):
    """zp_pairing_check_bn254: True iff every point is valid and the product of the e(P_j, Q_j) is 1 (EIP-197); no pairs: True"""
    a, b = _pairs(g1, g2)
    ok = C.c_int32(0)
    rc = load_library().zp_pairing_check_bn254(prover.ctx if prover is not None else None, a.ctypes.data, b.ctypes.data, a.shape[0], threads, C.byref(ok))
    if rc != 0:
        _verify_error(prover, rc, "zp_pairing_check_bn254")
    return bool(ok.value)


def _groth16_args(vk_words, proofs, publics):
    vk = np.ascontiguousarray(np.asarray(vk_words, dtype=np.uint32).reshape(-1))
    if vk.size < 112 + 16 or (vk.size - 112) % 16:
        raise ValueError("a key is alpha1[16] | beta2[32] | gamma2[32] | delta2[32] | ic[n_ic][16] words")
    n_ic = (vk.size - 112) // 16
    pr = np.ascontiguousarray(np.asarray(proofs, dtype=np.uint32).reshape(-1, 64))
    flat = [int(v) for row in publics for v in row]
    if len(flat) != pr.shape[0] * (n_ic - 1) or any(v < 0 or v >> 256 for v in flat):
        raise ValueError("n_ic - 1 public inputs below 2^256 per proof")
    pub = np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in flat] or [[0] * 4], dtype=np.uint64)
    return vk, n_ic, pr, pub


def groth16_verify(vk_words, proof_words, publics, prover=None):
    """zp_groth16_verify: the verdict (VERDICT_ACCEPT, _PUBLICS, _POINT or _PAIRING) of one proof (u32[64]: pi_a | pi_b | pi_c) with its public inputs
    (integers) under the key words (alpha1 | beta2 | gamma2 | delta2 | ic ...).  ZpError: a bad key"""
    vk, n_ic, pr, pub = _groth16_args(vk_words, proof_words, [publics])
    verdict = C.c_int32(-1)
    rc = load_library().zp_groth16_verify(prover.ctx if prover is not None else None, vk.ctypes.data, n_ic, pr.ctypes.data, pub.ctypes.data, C.byref(verdict))
    if rc != 0:
        _verify_error(prover, rc, "zp_groth16_verify")
    return verdict.value


def groth16_verify_batch(vk_words, proofs_words, publics_list, prover=None, threads=0):
    """zp_groth16_verify_batch: the verdicts of n proofs (u32[n][64]) under one key, each what groth16_verify gives (host threads; a Prover only receives
    the error text)"""
    vk, n_ic, pr, pub = _groth16_args(vk_words, proofs_words, publics_list)
    out = np.zeros(max(pr.shape[0], 1), dtype=np.int32)
    rc = load_library().zp_groth16_verify_batch(prover.ctx if prover is not None else None, vk.ctypes.data, n_ic, pr.ctypes.data, pub.ctypes.data, pr.shape[0],
                                                threads, out.ctypes.data)
    if rc != 0:
        _verify_error(prover, rc, "zp_groth16_verify_batch")
    return [int(v) for v in out[:pr.shape[0]]]


def wrap_aux(openings, program, pubs, logn, root32, addr):
    """zp_wrap_aux: ([addr, packed sparse fixed columns at zeta ...] as ints, zeta) for a stage B-2 wrap"""
    openings = np.ascontiguousarray(openings, dtype=np.uint64)
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    pb = np.ascontiguousarray(np.array([int(v) for v in pubs] or [0], dtype=np.uint64))
    a = fr_words([int(addr)])
    cap = int(prog[3])
    out = np.zeros((cap, 4), dtype=np.uint64)
    n, z = C.c_size_t(0), np.zeros(3, dtype=np.uint64)
    rc = load_library().zp_wrap_aux(openings.ctypes.data, openings.size, prog.ctypes.data, prog.size, pb.ctypes.data, len(pubs), logn, int(root32), a.ctypes.data,
                                    out.ctypes.data, cap, C.byref(n), z.ctypes.data)
    if rc != 0:
        raise ValueError("zp_wrap_aux: the openings record or the statement is malformed (%d)" % rc)
    return fr_ints(out[:n.value]), [int(v) for v in z]


def program_fixed_eval_ext(program, pubchal, logn, root32, zeta, threads=0):
    """zp_program_fixed_eval_ext: the fixed columns of a program at the out-of-domain point, u64[n_fixed][3]: the two boundary selectors, then the sparse
    periodic columns (host code; ValueError: malformed input)"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    pc = np.ascontiguousarray(np.array([int(v) for v in pubchal] or [0], dtype=np.uint64))
    z = np.array([int(v) for v in zeta], dtype=np.uint64)
    out = np.zeros((int(prog[3]), 3), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(_u64p)
    rc = load_library().zp_program_fixed_eval_ext(p(prog), prog.size, p(pc), len(pubchal), logn, int(root32), p(z), p(out), out.shape[0], threads)
    if rc != 0:
        raise ValueError("zp_program_fixed_eval_ext: malformed program or point (%d)" % rc)
    return out


def program_fixed_eval_ext_batch(program, pubchal, logn, root32, zetas, prover=None, threads=0):
    """zp_program_fixed_eval_ext_batch: the fixed columns of a program at many points, each with its own public inputs (and challenges).
    pubchal: n_points rows of n_pub + n_chal values; zetas: n_points rows of 3.  Returns (u64[n_points][n_fixed][3], on_domain bool[n_points]): a point on
    the trace domain or on a column's domain is flagged and its rows are zero.  prover=None: host code; with a Prover the sparse columns of all points
    run on the device from the knob "fixed_eval_dev_min" (points x entries) on -- the same words either way.  ValueError: malformed input"""
    prog = np.ascontiguousarray(program, dtype=np.uint64)
    as_rows = lambda a: a.astype(np.uint64) if isinstance(a, np.ndarray) else np.array([[int(v) for v in row] for row in a], dtype=np.uint64)
    z = np.ascontiguousarray(as_rows(zetas).reshape(-1, 3))
    n = z.shape[0]
    if len(pubchal) != n or any(len(r) != len(pubchal[0]) for r in pubchal):
        raise ValueError("zp_program_fixed_eval_ext_batch: one row of public inputs per point, all of one length")
    n_pubchal = len(pubchal[0]) if n else 0
    pc = np.ascontiguousarray(as_rows(pubchal).reshape(-1)) if n and n_pubchal else np.zeros(1, dtype=np.uint64)
    n_fixed = int(prog[3]) if prog.size > 3 and int(prog[3]) <= 4096 else 0
    out = np.zeros((n, n_fixed, 3), dtype=np.uint64)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(_u64p)
    rc = load_library().zp_program_fixed_eval_ext_batch(prover.ctx if prover is not None else None, p(prog), prog.size, p(pc), n_pubchal, logn, int(root32),
                                                        p(z if n else np.zeros(3, dtype=np.uint64)), n, p(out if out.size else np.zeros(3, dtype=np.uint64)), n_fixed,
                                                        flags.ctypes.data_as(C.POINTER(C.c_uint8)), threads)
    if rc == -1:
        raise ValueError("zp_program_fixed_eval_ext_batch: malformed program or point (%d)" % rc)
    if rc != 0:
        if prover is not None:
            prover._chk(rc)
        raise ZpError(rc, "zp_program_fixed_eval_ext_batch")
    return out, flags[:n].astype(bool)


def sha256(data):
    out = (C.c_uint8 * 32)()
    buf = bytes(data)
    rc = load_library().zp_sha256(buf, len(buf), out)
    if rc != 0:
        raise ZpError(rc, "zp_sha256")
    return bytes(out)


def r1cs_key_scalars(blob, tau, alpha, beta, gamma, delta):
    """zp_r1cs_key_scalars -> (u, v, l each u64[n_wires][4], h u64[2^logm - 1][4])"""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    nw, m = int(blob[1]), 1 << int(blob[3])
    par = fr_words([tau, alpha, beta, gamma, delta])
    u, v, l = (np.empty((nw, 4), dtype=np.uint64) for _ in range(3))
    h = np.empty((m - 1, 4), dtype=np.uint64)
    rc = load_library().zp_r1cs_key_scalars(blob.ctypes.data, blob.size, par.ctypes.data, u.ctypes.data, v.ctypes.data, l.ctypes.data, h.ctypes.data, 0)
    if rc != 0:
        raise ZpError(rc, "zp_r1cs_key_scalars: malformed circuit or parameters")
    return u, v, l, h


def json_key_span(data, key):
    """(begin, end) of the value of member `key` of the JSON object in `data` (bytes), or None"""
    b, e = C.c_size_t(0), C.c_size_t(0)
    if load_library().zp_json_key_span(data, len(data), key.encode(), C.byref(b), C.byref(e)) != 0:
        return None
    return b.value, e.value


def parse_proof_queries(data):
    """The query openings of a proof text (bytes) as arrays, parsed by the library (csrc/proofparse.hip): returns (q_begin, q_end, {"index":
    u64[nq], "values": [u64[nq][w] per tree], "paths": [u64[nq][depth][4] per tree], "has_stage2", "n_fri"}) with the trees in the order trace,
    [stage2], quotient, fri0 ..; None when the text is not in the grammar the provers write (the caller then uses its JSON parser)."""
    lib = load_library()
    qb, qe = C.c_size_t(0), C.c_size_t(0)
    nq, s2, nf = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    w, d = np.zeros(48, dtype=np.int32), np.zeros(48, dtype=np.int32)
    if lib.zp_proof_queries_scan(data, len(data), C.byref(qb), C.byref(qe), C.byref(nq), C.byref(s2), C.byref(nf), w.ctypes.data, d.ctypes.data, 48) != 0:
        return None
    T, n = 2 + s2.value + nf.value, nq.value
    w, d = w[:T].copy(), d[:T].copy()
    index = np.empty(n, dtype=np.uint64)
    values = np.empty(n * int(w.sum()), dtype=np.uint64)
    paths = np.empty(n * int(d.sum()) * 4, dtype=np.uint64)
    if lib.zp_proof_queries_parse(data, qb.value, qe.value, n, s2.value, nf.value, w.ctypes.data, d.ctypes.data, index.ctypes.data, values.ctypes.data,
                                  paths.ctypes.data) != 0:
        return None
    vs, ps, vo, po = [], [], 0, 0
    for t in range(T):
        vs.append(values[vo:vo + n * int(w[t])].reshape(n, int(w[t])))
        ps.append(paths[po:po + n * int(d[t]) * 4].reshape(n, int(d[t]), 4))
        vo += n * int(w[t])
        po += n * int(d[t]) * 4
    return qb.value, qe.value, {"index": index, "values": vs, "paths": ps, "has_stage2": bool(s2.value), "n_fri": nf.value}


def _arith_args(desc, a):
    """contiguous arrays of the arithmetic-witness inputs (stark/verifier_air.py: build_witness -> arith_in)"""
    d = np.ascontiguousarray(np.asarray(desc, dtype=np.uint64))
    vals = np.ascontiguousarray(a["vals"], dtype=np.uint64)
    index = np.ascontiguousarray(a["index"], dtype=np.uint64)
    dbit = np.ascontiguousarray(a["dbit"], dtype=np.uint64)
    blk_op = np.ascontiguousarray(a["blk_op"], dtype=np.int64)
    aps = np.ascontiguousarray(np.asarray(a["aps"], dtype=np.uint64))
    fin = np.ascontiguousarray(a["fin"], dtype=np.uint64)
    assert vals.shape[1] == int(d[7]) and vals.shape[0] == int(d[8]) and len(dbit) == int(d[1]) * int(d[2]) == len(blk_op)
    assert aps.shape == (int(d[4]), int(d[9])) and fin.size == int(d[2]) * int(d[3]) * int(d[4]) * 3
    return d, vals, index, dbit, blk_op, aps, fin


def _arith_error(rc):
    if rc in (-10, -11):
        return ValueError("the opened values of an inner proof are inconsistent (%s): no accepting witness"
                          % ("a FRI layer does not hold the value the layer before it claims" if rc == -10 else "the last fold does not give its final layer"))
    return ZpError(rc, "zp_verifier_arith: malformed descriptor or inputs")


def verifier_arith_host(desc, a, threads=0):
    """zp_verifier_arith_host: the 21 arithmetic columns of the verifier trace as a host array u64[21][N] -- host code, no GPU needed"""
    d, vals, index, dbit, blk_op, aps, fin = _arith_args(desc, a)
    out = np.empty((21, 32 * len(dbit)), dtype=np.uint64)
    rc = load_library().zp_verifier_arith_host(d.ctypes.data, d.size, vals.ctypes.data, index.ctypes.data, dbit.ctypes.data, blk_op.ctypes.data,
                                               aps.ctypes.data, fin.ctypes.data, out.ctypes.data, threads)
    if rc != 0:
        raise _arith_error(rc)
    return out


def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 makes it, every rank passes it to Comm)"""
    buf = (C.c_uint8 * 128)()
    rc = load_library().zp_comm_unique_id(buf)
    if rc != 0:
        raise ZpError(rc, "zp_comm_unique_id failed (librccl.so not loadable?)")
    return bytes(buf)


class CommGroup:
    """zp_comm_group: ranks that live in one process (threads, one Prover each); Comm(prover, rank, world, group=...) joins it"""

    def __init__(self, world):
        self.world = world
        h = _vp()
        rc = load_library().zp_comm_group_create(world, C.byref(h))
        if rc != 0:
            raise ZpError(rc, "zp_comm_group_create: world must be a power of two <= 64")
        self.h = h

    def close(self):
        if self.h:
            load_library().zp_comm_group_destroy(self.h)
            self.h = None


class Comm:
    """zp_comm: this rank's Prover joined to an RCCL communicator (one process per GPU) or to an in-process CommGroup;
    collectives on the ctx stream"""

    def __init__(self, prover, rank, world, unique_id=None, group=None):
        self.prover, self.rank, self.world = prover, rank, world
        h = _vp()
        if group is not None:
            assert group.world == world
            prover._chk(prover.lib.zp_comm_create_local(prover.ctx, rank, group.h, C.byref(h)))
        else:
            idb = (C.c_uint8 * 128).from_buffer_copy(unique_id)
            prover._chk(prover.lib.zp_comm_create(prover.ctx, rank, world, idb, C.byref(h)))
        self.h = h

    def all_reduce_sum(self, d_buf, words):
        self.prover._chk(self.prover.lib.zp_comm_all_reduce_sum(self.h, _ptr(d_buf), words))

    def my_columns(self, width):
        """the trace columns of this rank, (first, count): ceil(width / world) per rank, the tail ranks fewer (include/zeth_prover.h)"""
        wl = -(-width // self.world)
        first = min(self.rank * wl, width)
        return first, min(wl, width - first)

    def stark_prove_sharded(self, air_name, program, d_trace_local, pubs, logn, logb, fri_logf, fri_final_log, n_queries, pow_bits=0, bn128=False):
        """zp_stark_prove_sharded (bn128: zp_stark_prove_sharded_bn128): this rank's columns in, the whole proof text out (the same on every rank)"""
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        out, n = C.c_void_p(), C.c_size_t(0)
        words = d_trace_local.n if isinstance(d_trace_local, DeviceBuffer) else self.my_columns(int(prog[1]))[1] << logn
        head = (self.h, air_name.encode(), prog.ctypes.data, prog.size, _ptr(d_trace_local), words, pb.ctypes.data, len(pubs), logn, logb, fri_logf,
                fri_final_log, n_queries)
        if bn128:
            assert pow_bits == 0
            self.prover._chk_proof(self.prover.lib.zp_stark_prove_sharded_bn128(*head, C.byref(out), C.byref(n)), prog)
        else:
            self.prover._chk_proof(self.prover.lib.zp_stark_prove_sharded(*head, pow_bits, C.byref(out), C.byref(n)), prog)
        try:
            return C.string_at(out.value, n.value).decode()
        finally:
            self.prover.lib.zp_free_buffer(out)

    def check_witness_sharded(self, program, d_trace_local, pubs, logn, chal=None):
        """zp_stark_check_witness_sharded: this rank's columns of the trace (my_columns; None when it has none) against the program -> the
        WitnessReport of the WHOLE trace, the same on every rank.  Collective: every rank calls it"""
        prog = np.asarray(program, dtype=np.uint64)
        if prog.ndim != 1 or prog.size < 12:
            raise ZpError(-1, "zp_stark_check_witness_sharded: malformed program")
        words = d_trace_local.n if isinstance(d_trace_local, DeviceBuffer) else self.my_columns(int(prog[1]))[1] << logn
        rc, rep = _check_witness(None, prog, _ptr(d_trace_local), words, pubs, logn, chal, 0, comm=self.h)
        self.prover._chk(rc)
        return rep

    def close(self):
        if self.h:
            self.prover.lib.zp_comm_destroy(self.h)
            self.h = None

    def abort(self):
        """zp_comm_abort: this rank gives up; no peer is left waiting for it (they return ZP_ERR_COMM)"""
        self.prover._chk(self.prover.lib.zp_comm_abort(self.h))

    def set_timeout_ms(self, ms):
        self.prover._chk(self.prover.lib.zp_comm_set_timeout_ms(self.h, int(ms)))

    def info(self):
        """zp_comm_info: what the transport itself reports -- {"transport": "rccl" | "local", "ranks_seen", "user_rank", "device"}"""
        out = (C.c_int32 * 4)()
        self.prover._chk(self.prover.lib.zp_comm_info(self.h, out))
        return {"transport": "rccl" if out[0] == 1 else "local", "ranks_seen": int(out[1]), "user_rank": int(out[2]), "device": int(out[3])}

    def release_scratch(self):
        self.prover._chk(self.prover.lib.zp_comm_release_scratch(self.h))

    def all_to_all(self, d_send, d_recv, words_per_peer):
        self.prover._chk(self.prover.lib.zp_comm_all_to_all(self.h, _ptr(d_send), _ptr(d_recv), words_per_peer))

    def all_gather(self, d_send, d_recv, words):
        self.prover._chk(self.prover.lib.zp_comm_all_gather(self.h, _ptr(d_send), _ptr(d_recv), words))

    def broadcast(self, d_buf, words, root=0):
        self.prover._chk(self.prover.lib.zp_comm_broadcast(self.h, _ptr(d_buf), words, root))

    def exchange_columns_to_rows(self, d_cols, Wl, M, d_pack, d_rows):
        self.prover._chk(self.prover.lib.zp_exchange_columns_to_rows(self.h, _ptr(d_cols), Wl, M, _ptr(d_pack), _ptr(d_rows)))

    def ntt_sharded(self, d_data, d_tmp, logn, inverse=False, natural_output=True):
        """four-step NTT of one column of 2^logn elements split over the ranks, in place on this rank's contiguous block
        (d_tmp: scratch of 2 * 2^logn / world words)"""
        self.prover._chk(self.prover.lib.zp_ntt_sharded(self.h, _ptr(d_data), _ptr(d_tmp), logn, int(bool(inverse)), int(bool(natural_output))))

    def merkle_commit_sharded(self, d_cols, M, Wl, d_tree_local):
        """-> the global root (4 ints)"""
        root = (C.c_uint64 * 4)()
        self.prover._chk(self.prover.lib.zp_merkle_commit_sharded(self.h, _ptr(d_cols), M, Wl, _ptr(d_tree_local), root))
        return [int(v) for v in root]

    def my_range(self, n_total):
        """this rank's slice of n_total indices, (first, count): the rule of my_columns (and of every sharded entry point)"""
        return self.my_columns(n_total)

    def msm_bn254_sharded(self, d_points_local, d_scalars_local, n_total, g2=False):
        """zp_msm_bn254_sharded (g2: zp_msm_bn254_g2_sharded): this rank's slice of the points and scalars in (device, my_range(n_total); None for
        an empty slice), the affine sum of ALL n_total terms out on every rank: u32[16] (G2: u32[32]), all zero = infinity"""
        out = (C.c_uint32 * (32 if g2 else 16))()
        fn = self.prover.lib.zp_msm_bn254_g2_sharded if g2 else self.prover.lib.zp_msm_bn254_sharded
        self.prover._chk(fn(self.h, _ptr(d_points_local), _ptr(d_scalars_local), int(n_total), out))
        return np.array(out, dtype=np.uint32)

    def groth16_prove_sharded(self, blob, dev, delta1_words, set_idx, set_val, r, s):
        """zp_groth16_prove_sharded: Prover.groth16_prove over the ranks -- dev holds THIS rank's slices of the key's point arrays (u1x, v1x, v2x,
        l1, h1; None where the slice is empty) and of "v_wires", and "n_v" (the total); the same result on every rank"""
        return self.prover._groth16(self.prover.lib.zp_groth16_prove_sharded, self.h, blob, dev, delta1_words, set_idx, set_val, r, s)


def over_ranks(provers, fn, timeout_ms=None):
    """fn(rank, prover, comm) on one thread per rank: provers[r] joined as rank r to a fresh in-process CommGroup (the ranks of
    prove_native_sharded).  Returns the list of results; raises the first rank's own error -- not a peer's ZP_ERR_COMM -- after every thread
    has ended (a rank that fails calls zp_comm_abort first, so no peer waits for it)."""
    world = len(provers)
    group = CommGroup(world)
    out, errs = [None] * world, [None] * world

    def body(r):
        c = None
        try:
            c = Comm(provers[r], r, world, group=group)
            if timeout_ms is not None:
                c.set_timeout_ms(timeout_ms)
            out[r] = fn(r, provers[r], c)
        except BaseException as e:          # noqa: every rank's error is looked at below
            errs[r] = e
            if c is not None:
                try:
                    c.abort()
                except Exception:
                    pass
        finally:
            if c is not None:
                c.close()
    ts = [threading.Thread(target=body, args=(r,), name="rank-%d" % r) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    group.close()
    bad = [e for e in errs if e is not None]
    if bad:
        real = [e for e in bad if not (isinstance(e, ZpError) and e.code == -6)]       # ZP_ERR_COMM: a peer of the rank that failed
        raise (real or bad)[0]
    return out


class Prover:
    """One zp_ctx = one GPU + one stream."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        ctx = _vp()
        rc = self.lib.zp_create(C.byref(ctx), device)
        if rc != 0:
            raise ZpError(rc, "zp_create failed (no HIP device %d?) -- the prover requires an MI355X" % device)
        self.ctx = ctx
        self.pooling = False      # device-buffer reuse by exact size (set True for repeated same-shape work)
        self._pool = {}
        self._hpool = {}          # page-locked host buffers by byte size
        self._host_ptrs = {}      # numpy data address -> (pointer, bytes) of the arrays handed out by host_array
        self._lock = threading.Lock()
        if stream is not None:
            self.set_stream(stream)

    def trim(self):
        """release every pooled device buffer"""
        for ptrs in self._hpool.values():
            for ptr in ptrs:
                self.lib.zp_host_free(self.ctx, ptr)
        self._hpool = {}
        for ptrs in self._pool.values():
            for ptr in ptrs:
                self.lib.zp_dev_free(self.ctx, ptr)
        self._pool = {}

    def close(self):
        if self.ctx:
            self.trim()
            self.lib.zp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise ZpError(rc, (self.lib.zp_last_error(self.ctx) or b"").decode())

    # ---- plumbing
    def stream_handle(self):
        """the hipStream_t every launch of this ctx goes to (None = the legacy default stream)"""
        out = C.c_void_p()
        self._chk(self.lib.zp_get_stream(self.ctx, C.byref(out)))
        return out.value

    def set_stream(self, stream):
        self._chk(self.lib.zp_set_stream(self.ctx, int(stream) if stream else None))

    def sync(self):
        self._chk(self.lib.zp_sync(self.ctx))

    def set_constants(self, kind, values):
        a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).ravel())
        self._chk(self.lib.zp_set_constants(self.ctx, kind, a.ctypes.data_as(_u64p), a.size))

    def get_constants(self, kind, n):
        a = np.zeros(n, dtype=np.uint64)
        self._chk(self.lib.zp_get_constants(self.ctx, kind, a.ctypes.data_as(_u64p), n))
        return a

    def alloc(self, n_elems):
        return DeviceBuffer(self, n_elems)

    def host_array(self, shape):
        """uint64 numpy array in page-locked host memory (zp_host_alloc), pooled by size; hand it back with
        release_host_array when the copy that read it has completed"""
        nbytes = int(np.prod(shape)) * 8
        with self._lock:
            pool = self._hpool.get(nbytes)
            ptr = pool.pop() if pool else None
        if ptr is None:
            p = C.c_void_p()
            self._chk(self.lib.zp_host_alloc(self.ctx, nbytes, C.byref(p)))
            ptr = p.value
        arr = np.ctypeslib.as_array((C.c_uint64 * (nbytes // 8)).from_address(ptr)).reshape(shape)
        self._host_ptrs[arr.ctypes.data] = (ptr, nbytes)
        return arr

    def release_host_array(self, arr):
        ptr, nbytes = self._host_ptrs.pop(arr.ctypes.data)
        with self._lock:
            self._hpool.setdefault(nbytes, []).append(ptr)

    def upload(self, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64))
        buf = DeviceBuffer(self, a.size)
        self._chk(self.lib.zp_h2d(self.ctx, buf.ptr, a.ctypes.data, a.nbytes))
        return buf

    def download(self, buf, shape, offset_elems=0):
        out = np.empty(shape, dtype=np.uint64)
        self._chk(self.lib.zp_d2h(self.ctx, out.ctypes.data, _ptr(buf) + 8 * offset_elems, out.nbytes))
        return out

    def d2d(self, dst, src, nbytes):
        self._chk(self.lib.zp_d2d(self.ctx, _ptr(dst), _ptr(src), nbytes))

    def memset(self, dst, value, nbytes):
        assert value == 0
        self._chk(self.lib.zp_dev_zero(self.ctx, _ptr(dst), nbytes))

    def h2d(self, dst, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64))
        self._chk(self.lib.zp_h2d(self.ctx, _ptr(dst), a.ctypes.data, a.nbytes))

    # ---- hot path (device pointers)
    def ntt(self, d_in, d_out, logn, W):
        self._chk(self.lib.zp_ntt(self.ctx, _ptr(d_in), _ptr(d_out), logn, W))

    def intt(self, d_in, d_out, logn, W):
        self._chk(self.lib.zp_intt(self.ctx, _ptr(d_in), _ptr(d_out), logn, W))

    def twiddle_rows(self, d_rows, logn_row, W, row0, logn_total, inverse=False):
        self._chk(self.lib.zp_twiddle_rows(self.ctx, _ptr(d_rows), logn_row, W, row0, logn_total, 1 if inverse else 0))

    # ---- synthetic witnesses generated in HBM (csrc/synth.hip): the traces of synth_trace, word for word
    def synth_checkpoints(self, kind, logn, W, seeds, binds=None):
        """checkpoints of the wide-mix recurrences of len(seeds) chunks (one wave per chunk, synchronous): a DeviceBuffer holding
        synth_checkpoint_words words per chunk; binds: per chunk the starting values a caller dictates (all of the same length)"""
        words = int(self.lib.zp_synth_checkpoint_words(kind, logn, W))
        if words == 0:
            raise ValueError("zp_synth_checkpoints: this kind / shape has no recurrence columns")
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        nb = len(binds[0]) if binds is not None and len(binds) else 0
        b = np.ascontiguousarray(np.asarray(binds, dtype=np.uint64).reshape(len(s), nb)) if nb else None
        d = DeviceBuffer(self, words * len(s))
        self._chk(self.lib.zp_synth_checkpoints(self.ctx, kind, logn, W, len(s), s.ctypes.data_as(_u64p), b.ctypes.data_as(_u64p) if nb else None, nb, d.ptr))
        d.words_per_chunk = words
        return d

    def synth_trace_device(self, kind, logn, W, seed, bind=None, ckpt=None, ckpt_index=0, out=None):
        """(device trace [W][2^logn], publics): zp_synth_trace_device on this ctx's stream; ckpt: the buffer of synth_checkpoints and this chunk's
        position in it (None: made inside the call)"""
        d = out if out is not None else DeviceBuffer(self, W << logn)
        d.shape = (W, 1 << logn)
        pub = np.zeros(8, dtype=np.uint64)
        b = np.ascontiguousarray(np.asarray(bind, dtype=np.uint64)) if bind is not None and len(bind) else None
        cp = (ckpt.ptr + 8 * ckpt.words_per_chunk * int(ckpt_index)) if ckpt is not None else None
        self._chk(self.lib.zp_synth_trace_device(self.ctx, kind, logn, W, seed, b.ctypes.data_as(_u64p) if b is not None else None, len(b) if b is not None else 0,
                                                 cp, d.ptr, pub.ctypes.data_as(_u64p)))
        return d, pub[:{0: 3, 2: 1, 3: 8}.get(kind, min(4, W))].copy()

    def lde(self, d_in, d_out, logn, logb, W, shift=0, d_coef=None):
        self._chk(self.lib.zp_lde(self.ctx, _ptr(d_in), _ptr(d_out), _ptr(d_coef), logn, logb, W, shift))

    def verifier_arith_trace(self, desc, a, d_out, threads=0):
        """zp_verifier_arith_trace: the 21 arithmetic columns of the verifier trace written in HBM at d_out (u64[21][N])"""
        d, vals, index, dbit, blk_op, aps, fin = _arith_args(desc, a)
        rc = self.lib.zp_verifier_arith_trace(self.ctx, d.ctypes.data, d.size, vals.ctypes.data, index.ctypes.data, dbit.ctypes.data, blk_op.ctypes.data,
                                              aps.ctypes.data, fin.ctypes.data, _ptr(d_out), threads)
        if rc in (-10, -11):
            raise _arith_error(rc)
        self._chk(rc)

    def recursion_witness(self, desc, index, values, paths, streams, d_trace, threads=0):
        """zp_recursion_witness: the whole verifier-AIR witness of inner proofs given as arrays (per proof: index u64[nq], values / paths in
        the layout of zp_proof_queries_parse, the transcript stream); the trace is written at d_trace, the public inputs are returned"""
        d = np.ascontiguousarray(np.asarray(desc, dtype=np.uint64))
        n = len(index)
        keep = [[np.ascontiguousarray(a, dtype=np.uint64) for a in arrs] for arrs in (index, values, paths, streams)]
        ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in arrs]) for arrs in keep]
        sw = (C.c_size_t * n)(*[a.size for a in keep[3]])
        npub = int(self.lib.zp_recursion_publics_words(d.ctypes.data, d.size))
        if npub == 0:
            raise ZpError(-1, "malformed witness descriptor")
        pubs = np.empty(npub, dtype=np.uint64)
        rc = self.lib.zp_recursion_witness(self.ctx, d.ctypes.data, d.size, ptrs[0], ptrs[1], ptrs[2], ptrs[3], sw, _ptr(d_trace), pubs.ctypes.data, npub, threads)
        if rc in (-10, -11, -13, -14):
            raise ValueError((self.lib.zp_last_error(self.ctx) or b"inner proof does not verify: no accepting witness").decode())
        self._chk(rc)
        return pubs

    def poseidon_perm(self, d_states, count):
        self._chk(self.lib.zp_poseidon_perm(self.ctx, _ptr(d_states), count))

    def poseidon_trace(self, d_inputs, count, d_states, d_cubes, stride):
        self._chk(self.lib.zp_poseidon_trace(self.ctx, _ptr(d_inputs), count, _ptr(d_states), _ptr(d_cubes), stride))

    def eval_quotient(self, program, d_cols, d_fixed, logm, logb, pubs, apow, zhinv, shift, w_last, d_out):
        """constraint program blob (numpy u64) interpreted on the GPU: quotient planes u64[3][2^logm] into d_out"""
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        ap = np.ascontiguousarray(np.asarray(apow, dtype=np.uint64).reshape(-1))
        zh = np.ascontiguousarray(np.asarray(zhinv, dtype=np.uint64))
        self._chk(self.lib.zp_eval_quotient(self.ctx, prog.ctypes.data, prog.size, _ptr(d_cols), _ptr(d_fixed), logm, logb, pb.ctypes.data,
                                            len(pubs), ap.ctypes.data, zh.ctypes.data, shift, w_last, _ptr(d_out)))

    def fixed_columns(self, program, pubs, logn, logb, shift=0):
        """the d_fixed of eval_quotient for this statement (zp_fixed_columns): selectors + one extended period per periodic column"""
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        words = int(self.lib.zp_fixed_columns_words(prog.ctypes.data, prog.size, logn, logb))
        if words == 0:
            raise ValueError("malformed constraint program (or a fixed column longer than the trace)")
        out = DeviceBuffer(self, words)
        self._chk(self.lib.zp_fixed_columns(self.ctx, prog.ctypes.data, prog.size, pb.ctypes.data, len(pubs), logn, logb, shift, out.ptr, words))
        return out

    # ---- BN128-hash mode (Poseidon over the BN254 scalar field); field elements = 4 little-endian u64 words
    @staticmethod
    def _fr_words(vals):
        a = np.zeros((len(vals), 4), dtype=np.uint64)
        for i, v in enumerate(vals):
            for k in range(4):
                a[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        return a

    @staticmethod
    def _fr_ints(a):
        a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
        return [sum(int(a[i, k]) << (64 * k) for k in range(4)) for i in range(a.shape[0])]

    def install_poseidon_bn254(self, t):
        """derive (poseidon_constants.bn254_poseidon_params) and install the tables of width t (3 or 17)"""
        from .poseidon_constants import bn254_poseidon_params
        rc, mds, rp = bn254_poseidon_params(t)
        rcw = self._fr_words(rc)
        mw = self._fr_words([v for row in mds for v in row])
        self._chk(self.lib.zp_set_poseidon_bn254(self.ctx, t, rp, rcw.ctypes.data, mw.ctypes.data))

    def poseidon_bn254_perm(self, states):
        """states: list of lists of t ints < r -> permuted (host convenience around zp_poseidon_bn254_perm)"""
        t = len(states[0])
        buf = self.upload(self._fr_words([v for st in states for v in st]).reshape(-1))
        self._chk(self.lib.zp_poseidon_bn254_perm(self.ctx, buf.ptr, len(states), t))
        out = self._fr_ints(self.download(buf, (len(states) * t * 4,)))
        return [out[i * t:(i + 1) * t] for i in range(len(states))]

    def merkle16_nodes(self, M):
        return int(self.lib.zp_merkle16_nodes(M))

    def merkle16_commit_bn254(self, d_cols, M, W, d_tree):
        self._chk(self.lib.zp_merkle16_commit_bn254(self.ctx, _ptr(d_cols), M, W, _ptr(d_tree)))

    def merkle16_open_bn254(self, d_tree, M, idx):
        levels, n = 0, M
        while n > 1:
            n = (n + 15) // 16
            levels += 1
        out = np.zeros((max(levels, 1), 16, 4), dtype=np.uint64)
        self._chk(self.lib.zp_merkle16_open_bn254(self.ctx, _ptr(d_tree), M, idx, out.ctypes.data))
        return [self._fr_ints(out[l]) for l in range(levels)]

    def merkle16_open_batch_bn254(self, d_tree, M, idx):
        """-> per query: per level the 16 digests (ints) of the group on the path"""
        levels, n = 0, M
        while n > 1:
            n = (n + 15) // 16
            levels += 1
        ii = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        out = np.zeros((len(ii), max(levels, 1), 16, 4), dtype=np.uint64)
        self._chk(self.lib.zp_merkle16_open_batch_bn254(self.ctx, _ptr(d_tree), M, ii.ctypes.data, len(ii), out.ctypes.data))
        return [[self._fr_ints(out[q, l]) for l in range(levels)] for q in range(len(ii))]

    def ntt_bn254(self, d_data, logn, inverse=False, coset=None):
        """in-place NTT over the BN254 scalar field on d_data u64[2^logn][4]; coset: int g or None"""
        cw = self._fr_words([coset]) if coset is not None else None
        self._chk(self.lib.zp_ntt_bn254(self.ctx, _ptr(d_data), logn, 1 if inverse else 0, cw.ctypes.data if cw is not None else None))

    def qap_quotient_bn254(self, a_ev, b_ev, c_ev, logm, coset):
        """lists of ints (evaluations of A, B, C on <w>) -> coefficients of H = (A B - C) / (x^m - 1), list of ints"""
        m = 1 << logm
        bufs = [self.upload(self._fr_words(v).reshape(-1)) for v in (a_ev, b_ev, c_ev)]
        cw = self._fr_words([coset])
        self._chk(self.lib.zp_qap_quotient_bn254(self.ctx, _ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), logm, cw.ctypes.data))
        out = self._fr_ints(self.download(bufs[0], (m, 4)))
        for b in bufs:
            b.free()
        return out

    def pack_blocks(self, d_in, d_out, rows, row_len, parts):
        self._chk(self.lib.zp_pack_blocks(self.ctx, _ptr(d_in), _ptr(d_out), rows, row_len, parts))

    def transpose(self, d_in, d_out, rows, cols):
        self._chk(self.lib.zp_transpose(self.ctx, _ptr(d_in), _ptr(d_out), rows, cols))

    def hbm_copy_probe(self, d_src, d_dst, nbytes, reps=5):
        """average ms of one device copy of nbytes with the library's own 16 B/lane kernel"""
        ms = C.c_float(0)
        self._chk(self.lib.zp_hbm_copy_probe(self.ctx, _ptr(d_src), _ptr(d_dst), nbytes, reps, C.byref(ms)))
        return float(ms.value)

    @staticmethod
    def _words(d_trace, prog, logn):
        """u64 words behind a trace handle: what the buffer says it holds (DeviceBuffer.n / tensor.numel()); a raw pointer has no
        size of its own, so the caller vouches for W * 2^logn"""
        if isinstance(d_trace, DeviceBuffer):
            return d_trace.n
        if hasattr(d_trace, "numel"):
            return int(d_trace.numel())
        return int(prog[1]) << logn

    def stark_prove(self, air_name, program, d_trace, pubs, logn, logb, fri_logf, fri_final_log, n_queries, pow_bits):
        """the whole chunk STARK in one C-ABI call (zp_stark_prove): device trace u64[W][2^logn] + constraint program blob -> proof text"""
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        out, n = C.c_void_p(), C.c_size_t(0)
        self._chk_proof(self.lib.zp_stark_prove(self.ctx, air_name.encode(), prog.ctypes.data, prog.size, _ptr(d_trace), self._words(d_trace, prog, logn),
                                                pb.ctypes.data, len(pubs),
                                                logn, logb, fri_logf, fri_final_log, n_queries, pow_bits, C.byref(out), C.byref(n)), prog)
        try:
            return C.string_at(out.value, n.value).decode()
        finally:
            self.lib.zp_free_buffer(out)

    def _chk_proof(self, rc, prog):
        """a one-call prover's return code (sharded ones included: the report is on this rank's ctx): ZP_ERR_WITNESS ("prove_check") becomes WitnessError
        with the report attached"""
        if rc == ZP_ERR_WITNESS:
            raise WitnessError(self.prove_witness_report(int(prog[8])))      # its line is zp_last_error's (compared in tests/test_gpu_witness_inproof.py)
        self._chk(rc)

    def prove_witness_report(self, n_constraints):
        """zp_stark_prove_witness_report: the WitnessReport of the last proof this ctx checked under set_tuning("prove_check", 1), accepted or refused;
        .chal = the stage-2 challenge it was judged at (the proof's own; zeros without stage 2)"""
        K = int(n_constraints)
        rep, chal = np.zeros(8, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        counts, first = np.zeros(max(K, 1), dtype=np.uint64), np.zeros(max(K, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(_u64p)
        self._chk(self.lib.zp_stark_prove_witness_report(self.ctx, p(rep), p(chal), p(counts), p(first), K))
        out = WitnessReport(rep, counts[:K], first[:K])
        out.chal = [int(v) for v in chal]
        return out

    def check_witness(self, program, d_trace, pubs, logn, chal=None):
        """zp_stark_check_witness on this ctx: the device trace u64[W][2^logn] (only read) against the program -> WitnessReport"""
        prog = np.asarray(program, dtype=np.uint64)
        rc, rep = _check_witness(self.ctx, prog, _ptr(d_trace), self._words(d_trace, prog, logn), pubs, logn, chal, 0)
        if rc != 0 and prog.size < 12:
            raise ZpError(rc, "zp_stark_check_witness: malformed program")
        self._chk(rc)
        return rep

    def diagnose_stage2(self, program, d_trace, logn):
        """zp_stark_diagnose_stage2 on this ctx: the device trace u64[W][2^logn] (only read) -> [Stage2Diagnosis] per stage-2 argument of the program"""
        prog = np.asarray(program, dtype=np.uint64)
        rc, out = _diagnose_stage2(self.ctx, prog, _ptr(d_trace), self._words(d_trace, prog, logn), logn, 0)
        if rc != 0 and prog.size < 12:
            raise ZpError(rc, "zp_stark_diagnose_stage2: malformed program")
        self._chk(rc)
        return out

    def stark_prove_bn128(self, air_name, program, d_trace, pubs, logn, logb, fri_logf, fri_final_log, n_queries):
        """zp_stark_prove_bn128: the one-call prover in BN128-hash mode (install_poseidon_bn254(17) first)"""
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        out, n = C.c_void_p(), C.c_size_t(0)
        self._chk_proof(self.lib.zp_stark_prove_bn128(self.ctx, air_name.encode(), prog.ctypes.data, prog.size, _ptr(d_trace),
                                                      self._words(d_trace, prog, logn), pb.ctypes.data, len(pubs),
                                                      logn, logb, fri_logf, fri_final_log, n_queries, C.byref(out), C.byref(n)), prog)
        try:
            return C.string_at(out.value, n.value).decode()
        finally:
            self.lib.zp_free_buffer(out)

    def poseidon_bn254_sponge(self, state, blocks, extra=0):
        """state: 17 ints, blocks: list of 16-int blocks -> (new state, [rates (16 ints) after absorbing and after each extra permutation])"""
        st = self._fr_words(state)
        bl = self._fr_words([v for b in blocks for v in b]) if blocks else np.zeros((1, 4), dtype=np.uint64)
        rates = np.zeros(((1 + extra) * 16, 4), dtype=np.uint64)
        self._chk(self.lib.zp_poseidon_bn254_sponge(self.ctx, st.ctypes.data, bl.ctypes.data, len(blocks), extra, rates.ctypes.data))
        r = self._fr_ints(rates)
        return self._fr_ints(st), [r[16 * k:16 * k + 16] for k in range(1 + extra)]

    def poseidon_sponge(self, state, blocks, extra=0):
        """state: 12 ints, blocks: list of 8-int blocks -> (new state, [rate after absorbing, rate after each extra permutation])"""
        st = np.array(state, dtype=np.uint64)
        bl = np.ascontiguousarray(np.array(blocks, dtype=np.uint64).reshape(-1)) if blocks else np.zeros(1, dtype=np.uint64)
        rates = np.zeros((1 + extra) * 8, dtype=np.uint64)
        self._chk(self.lib.zp_poseidon_sponge(self.ctx, st.ctypes.data_as(_u64p), bl.ctypes.data_as(_u64p), len(blocks), extra,
                                              rates.ctypes.data_as(_u64p)))
        return st.tolist(), rates.reshape(-1, 8).tolist()

    def poseidon_sponge_caps(self, state, blocks, extra=0):
        """poseidon_sponge that also returns the capacity after every permutation: (new state, rates, caps [(max(blocks, 1) + extra)][4])"""
        st = np.array(state, dtype=np.uint64)
        bl = np.ascontiguousarray(np.array(blocks, dtype=np.uint64).reshape(-1)) if blocks else np.zeros(1, dtype=np.uint64)
        rates = np.zeros((1 + extra) * 8, dtype=np.uint64)
        caps = np.zeros((max(len(blocks), 1) + extra) * 4, dtype=np.uint64)
        self._chk(self.lib.zp_poseidon_sponge_caps(self.ctx, st.ctypes.data_as(_u64p), bl.ctypes.data_as(_u64p), len(blocks), extra,
                                                   rates.ctypes.data_as(_u64p), caps.ctypes.data_as(_u64p)))
        return st.tolist(), rates.reshape(-1, 8).tolist(), caps.reshape(-1, 4).tolist()

    def pow_grind(self, seed4, bits):
        sd = (C.c_uint64 * 4)(*[int(v) for v in seed4])
        out = C.c_uint64(0)
        self._chk(self.lib.zp_pow_grind(self.ctx, sd, int(bits), C.byref(out)))
        return int(out.value)

    def merkle16_verify_batch_bn254(self, values, index, paths, M, root):
        """zp_merkle16_verify_batch_bn254: values u64[n][width], index u64[n], paths u64[n][levels][16][4] (merkle16_open_batch_bn254's words), the tree's
        leaf count M, root u64[4] -> uint8[n], 1 = the opening hashes into the root"""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        ix = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
        pt = np.ascontiguousarray(paths, dtype=np.uint64).reshape(-1)
        rt = np.ascontiguousarray(root, dtype=np.uint64).reshape(4)
        n = ix.size
        assert v.ndim == 2 and v.shape[0] == n
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        self._chk(self.lib.zp_merkle16_verify_batch_bn254(self.ctx, v.ctypes.data_as(_u64p), v.shape[1], ix.ctypes.data_as(_u64p), pt.ctypes.data_as(_u64p) if pt.size else None,
                                                          int(M), rt.ctypes.data_as(_u64p), n, ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return ok[:n]

    def merkle_verify_batch(self, values, index, paths, root):
        """zp_merkle_verify_batch: values u64[n][width], index u64[n], paths u64[n][depth][4] (bottom-up), root u64[4] -> uint8[n], 1 = the opening hashes to the root"""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        ix = np.ascontiguousarray(index, dtype=np.uint64)
        pt = np.ascontiguousarray(paths, dtype=np.uint64).reshape(len(ix), -1, 4)
        rt = np.ascontiguousarray(root, dtype=np.uint64)
        assert v.ndim == 2 and v.shape[0] == len(ix) and rt.size == 4
        ok = np.zeros(max(len(ix), 1), dtype=np.uint8)
        self._chk(self.lib.zp_merkle_verify_batch(self.ctx, v.ctypes.data_as(_u64p), v.shape[1], ix.ctypes.data_as(_u64p), pt.ctypes.data_as(_u64p) if pt.size else None,
                                                  pt.shape[1], rt.ctypes.data_as(_u64p), len(ix), ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return ok[:len(ix)]

    def merkle_commit(self, d_cols, M, W, d_tree):
        self._chk(self.lib.zp_merkle_commit(self.ctx, _ptr(d_cols), M, W, _ptr(d_tree)))

    def merkle_commit_rows(self, d_rows, M, length, d_tree):
        self._chk(self.lib.zp_merkle_commit_rows(self.ctx, _ptr(d_rows), M, length, _ptr(d_tree)))

    def merkle_open(self, d_tree, M, idx):
        depth = int(M).bit_length() - 1
        path = np.zeros((max(depth, 1), 4), dtype=np.uint64)
        self._chk(self.lib.zp_merkle_open(self.ctx, _ptr(d_tree), M, idx, path.ctypes.data_as(_u64p)))
        return path[:depth]

    def fri_fold(self, d_in, d_out, logn, logf, beta, shift):
        b = (C.c_uint64 * 3)(*[int(x) for x in beta])
        self._chk(self.lib.zp_fri_fold(self.ctx, _ptr(d_in), _ptr(d_out), logn, logf, b, shift))

    # ---- STARK stages
    def poly_eval_ext(self, d_coef, logn, W, z):
        zz = (C.c_uint64 * 3)(*[int(v) for v in z])
        out = np.zeros((W, 3), dtype=np.uint64)
        self._chk(self.lib.zp_poly_eval_ext(self.ctx, _ptr(d_coef), logn, W, zz, out.ctypes.data_as(_u64p)))
        return out

    def ood_eval(self, d_cols, col_stride, row_stride, W, logn, shift, z, want_next=False):
        """(p_c(z))[W][3] and, with want_next, (p_c(z w))[W][3] from the columns' VALUES on the coset shift <w> (barycentric form)"""
        zz = (C.c_uint64 * 3)(*[int(v) for v in z])
        out = np.zeros((W, 3), dtype=np.uint64)
        nxt = np.zeros((W, 3), dtype=np.uint64) if want_next else None
        self._chk(self.lib.zp_ood_eval(self.ctx, _ptr(d_cols), col_stride, row_stride, W, logn, int(shift), zz, 1 if want_next else 0,
                                       out.ctypes.data_as(_u64p), nxt.ctypes.data_as(_u64p) if want_next else None))
        return (out, nxt) if want_next else out

    def deep_quotient(self, d_cols_a, Wa, d_cols_b, Wb, logm, n_next, z, zw, gamma, ev_z, ev_zw, shift, d_out):
        a3 = lambda v: (C.c_uint64 * 3)(*[int(x) for x in v])
        ez = np.ascontiguousarray(np.asarray(ev_z, dtype=np.uint64))
        ezw = np.ascontiguousarray(np.asarray(ev_zw, dtype=np.uint64)) if n_next else np.zeros((1, 3), dtype=np.uint64)
        self._chk(self.lib.zp_deep_quotient(self.ctx, _ptr(d_cols_a), Wa, _ptr(d_cols_b), Wb, logm, n_next, a3(z),
                                            a3(zw), a3(gamma), ez.ctypes.data_as(_u64p), ezw.ctypes.data_as(_u64p),
                                            shift, _ptr(d_out)))

    def deep_quotient_rows(self, d_cols_a, Wa, stride_a, d_cols_b, Wb, stride_b, logm, row0, nrows, n_next, z, zw, gamma, ev_z, ev_zw, shift,
                           d_out, stride_out):
        a3 = lambda v: (C.c_uint64 * 3)(*[int(x) for x in v])
        ez = np.ascontiguousarray(np.asarray(ev_z, dtype=np.uint64))
        ezw = np.ascontiguousarray(np.asarray(ev_zw, dtype=np.uint64)) if n_next else np.zeros((1, 3), dtype=np.uint64)
        self._chk(self.lib.zp_deep_quotient_rows(self.ctx, _ptr(d_cols_a), Wa, stride_a, _ptr(d_cols_b), Wb, stride_b, logm, row0, nrows,
                                                 n_next, a3(z), a3(zw), a3(gamma), ez.ctypes.data, ezw.ctypes.data, shift, _ptr(d_out),
                                                 stride_out))

    def eval_quotient_rows(self, program, d_cols, stride_cols, d_fixed, stride_fixed, logm, logb, row0, nrows, pubs, apow, zhinv, shift,
                           w_last, d_out, stride_out):
        prog = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        pb = np.ascontiguousarray(np.asarray(list(pubs) + [0], dtype=np.uint64))
        ap = np.ascontiguousarray(np.asarray(apow, dtype=np.uint64).reshape(-1))
        zh = np.ascontiguousarray(np.asarray(zhinv, dtype=np.uint64))
        self._chk(self.lib.zp_eval_quotient_rows(self.ctx, prog.ctypes.data, prog.size, _ptr(d_cols), stride_cols, _ptr(d_fixed), stride_fixed,
                                                 logm, logb, row0, nrows, pb.ctypes.data, len(pubs), ap.ctypes.data, zh.ctypes.data, shift,
                                                 w_last, _ptr(d_out), stride_out))

    def grand_product(self, d_a, d_b, n, gamma, d_out):
        g = (C.c_uint64 * 3)(*[int(x) for x in gamma])
        self._chk(self.lib.zp_grand_product(self.ctx, _ptr(d_a), _ptr(d_b), n, g, _ptr(d_out)))

    def logup_columns(self, d_a, d_t, d_m, n, gamma, d_out):
        g = (C.c_uint64 * 3)(*[int(x) for x in gamma])
        self._chk(self.lib.zp_logup_columns(self.ctx, _ptr(d_a), _ptr(d_t), _ptr(d_m), n, g, _ptr(d_out)))

    def gather_rows(self, d_cols, M, W, idx):
        ii = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        out = np.zeros((len(ii), W), dtype=np.uint64)
        self._chk(self.lib.zp_gather_rows(self.ctx, _ptr(d_cols), M, W, ii.ctypes.data_as(_u64p), len(ii),
                                          out.ctypes.data_as(_u64p)))
        return out

    def merkle_open_batch(self, d_tree, M, idx):
        ii = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
        depth = int(M).bit_length() - 1
        out = np.zeros((len(ii), max(depth, 1), 4), dtype=np.uint64)
        self._chk(self.lib.zp_merkle_open_batch(self.ctx, _ptr(d_tree), M, ii.ctypes.data_as(_u64p), len(ii),
                                                out.ctypes.data_as(_u64p)))
        return out[:, :depth]

    def domain_tables(self, logm):
        lo, hi, lb = _vp(), _vp(), C.c_int32(0)
        self._chk(self.lib.zp_domain_tables(self.ctx, logm, C.byref(lo), C.byref(hi), C.byref(lb)))
        return lo.value, hi.value, lb.value

    # ---- N6
    def set_air_kernel(self, program, fn):
        """zp_stark_set_air_kernel: the generated constraint kernel (a ctypes function of the AIR's library, or None) for proofs of `program`"""
        blob = np.ascontiguousarray(program, dtype=np.uint64)
        addr = C.cast(fn, C.c_void_p).value if fn is not None else None
        self._chk(self.lib.zp_stark_set_air_kernel(self.ctx, blob.ctypes.data_as(_u64p), blob.size, addr))

    def set_air_kernel_rows(self, program, fn):
        """zp_stark_set_air_kernel_rows: the row-window form of the generated constraint kernel (`<symbol>_rows`), for the sharded provers of this ctx"""
        blob = np.ascontiguousarray(program, dtype=np.uint64)
        addr = C.cast(fn, C.c_void_p).value if fn is not None else None
        self._chk(self.lib.zp_stark_set_air_kernel_rows(self.ctx, blob.ctypes.data_as(_u64p), blob.size, addr))

    def set_air_kernel_witness_rows(self, program, fn):
        """zp_stark_set_air_kernel_witness_rows: the row-window witness form (`<symbol>_witness_rows`), for the sharded provers of this ctx under
        set_tuning("prove_check", 1) and for Comm.check_witness_sharded; set_tuning("witness_kernel", 0) keeps the interpreter"""
        blob = np.ascontiguousarray(np.asarray(program, dtype=np.uint64))
        addr = C.cast(fn, C.c_void_p) if fn is not None else None
        self._chk(self.lib.zp_stark_set_air_kernel_witness_rows(self.ctx, blob.ctypes.data_as(_u64p), blob.size, addr))

    def set_air_kernel_witness(self, program, fn):
        """zp_stark_set_air_kernel_witness: the witness form of the generated constraint kernel (`<symbol>_witness`), for check_witness on this ctx and
        for the one-call provers under set_tuning("prove_check", 1); set_tuning("witness_kernel", 0) keeps the interpreter"""
        blob = np.ascontiguousarray(program, dtype=np.uint64)
        addr = C.cast(fn, C.c_void_p).value if fn is not None else None
        self._chk(self.lib.zp_stark_set_air_kernel_witness(self.ctx, blob.ctypes.data_as(_u64p), blob.size, addr))

    def stark_openings(self):
        """zp_stark_openings: the binary openings of the last BN128-mode proof of this ctx (a copy)"""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        self._chk(self.lib.zp_stark_openings(self.ctx, C.byref(ptr), C.byref(n)))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(n.value,)).copy()

    def r1cs_eval_device(self, blob, set_idx, set_val):
        """zp_r1cs_eval_device -> (witness, a_ev, b_ev, c_ev downloaded, public inputs): the GPU's witness completion, for comparison with r1cs_eval"""
        blob = np.ascontiguousarray(blob, dtype=np.uint64)
        set_idx = np.ascontiguousarray(set_idx, dtype=np.uint64)
        set_val = np.ascontiguousarray(set_val, dtype=np.uint64)
        n, m, n_pub = int(blob[1]), 1 << int(blob[3]), int(blob[9])
        dw, da, db, dc = self.alloc(4 * n), self.alloc(4 * m), self.alloc(4 * m), self.alloc(4 * m)
        pub = np.zeros((n_pub, 4), dtype=np.uint64)
        bad = C.c_int64(-1)
        try:
            rc = self.lib.zp_r1cs_eval_device(self.ctx, blob.ctypes.data, blob.size, set_idx.ctypes.data, set_val.ctypes.data, set_idx.size, dw.ptr, da.ptr, db.ptr,
                                              dc.ptr, pub.ctypes.data, C.byref(bad))
            if rc == -20:
                raise ValueError("the assignment does not satisfy the circuit (constraint %d): no proof for a false statement" % bad.value)
            if rc != 0:
                raise ZpError(rc, (self.lib.zp_last_error(self.ctx) or b"").decode(), bad=bad.value)
            return self.download(dw, (n, 4)), self.download(da, (m, 4)), self.download(db, (m, 4)), self.download(dc, (m, 4)), fr_ints(pub)
        finally:
            for d in (dw, da, db, dc):
                d.free()

    def groth16_prove(self, blob, dev, delta1_words, set_idx, set_val, r, s):
        """zp_groth16_prove -> (pi_a u32[16], pi_b u32[32], pi_c u32[16], public inputs [int], [ms witness, ms QAP, ms MSMs]); dev: name -> device
        buffer of the key's points (u1x, v1x, v2x, l1, h1) + "v_wires" (device u32 list of the wires in B) and "n_v"; ValueError when the assignment does not satisfy the circuit"""
        return self._groth16(self.lib.zp_groth16_prove, self.ctx, blob, dev, delta1_words, set_idx, set_val, r, s)

    def _groth16(self, fn, handle, blob, dev, delta1_words, set_idx, set_val, r, s):
        blob = np.ascontiguousarray(blob, dtype=np.uint64)
        set_idx = np.ascontiguousarray(set_idx, dtype=np.uint64)
        set_val = np.ascontiguousarray(set_val, dtype=np.uint64)
        d1 = np.ascontiguousarray(delta1_words, dtype=np.uint32)
        rw, sw = fr_words([r]), fr_words([s])
        a, b, c = np.zeros(16, dtype=np.uint32), np.zeros(32, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
        n_pub = int(blob[9])
        pub = np.zeros((n_pub, 4), dtype=np.uint64)
        ms = (C.c_double * 8)()
        bad = C.c_int64(-1)
        rc = fn(handle, blob.ctypes.data, blob.size, _ptr(dev["u1x"]), _ptr(dev["v_wires"]), int(dev["n_v"]), _ptr(dev["v1x"]),
                                       _ptr(dev["v2x"]), _ptr(dev["l1"]), _ptr(dev["h1"]),
                                       d1.ctypes.data, set_idx.ctypes.data, set_val.ctypes.data, set_idx.size, rw.ctypes.data, sw.ctypes.data, a.ctypes.data,
                                       b.ctypes.data, c.ctypes.data, pub.ctypes.data, ms, C.byref(bad))
        if rc == -20:
            raise ValueError("the assignment does not satisfy the circuit (constraint %d): no proof for a false statement" % bad.value)
        self._chk(rc)
        return a, b, c, fr_ints(pub), [float(x) for x in ms]

    def fixed_base_mul(self, base_words, scalars, g2=False):
        """zp_fixed_base_mul_bn254(_g2): scalars u64[n][4] / u32[n][8] (standard form) times ONE base point (u32[16] / u32[32], affine) -> points
        u32[n][16] / u32[n][32] in the MSM layout ((0, 0) = infinity)"""
        sc = np.ascontiguousarray(scalars).view(np.uint32).reshape(-1, 8)
        base = np.ascontiguousarray(base_words, dtype=np.uint32)
        out = np.empty((sc.shape[0], 32 if g2 else 16), dtype=np.uint32)
        fn = self.lib.zp_fixed_base_mul_bn254_g2 if g2 else self.lib.zp_fixed_base_mul_bn254
        self._chk(fn(self.ctx, base.ctypes.data, sc.ctypes.data, sc.shape[0], out.ctypes.data, 0))
        return out

    def msm_bn254(self, points_xy, scalars):
        """points_xy: list of (x, y) ints ((0,0) = infinity); scalars: ints.  Returns (x, y) or None."""
        n = len(points_xy)
        pts = np.zeros((max(n, 1), 16), dtype=np.uint32)
        scs = np.zeros((max(n, 1), 8), dtype=np.uint32)
        for i, ((x, y), s) in enumerate(zip(points_xy, scalars)):
            for k in range(8):
                pts[i, k] = (x >> (32 * k)) & 0xFFFFFFFF
                pts[i, 8 + k] = (y >> (32 * k)) & 0xFFFFFFFF
                scs[i, k] = (s >> (32 * k)) & 0xFFFFFFFF
        return self.msm_bn254_arrays(pts[:n], scs[:n])

    def msm_bn254_arrays(self, pts, scs):
        pts = np.ascontiguousarray(pts, dtype=np.uint32)
        scs = np.ascontiguousarray(scs, dtype=np.uint32)
        n = pts.shape[0]
        d_p = DeviceBuffer(self, max(1, pts.size // 2 + 1))
        d_s = DeviceBuffer(self, max(1, scs.size // 2 + 1))
        if n:
            self._chk(self.lib.zp_h2d(self.ctx, d_p.ptr, pts.ctypes.data, pts.nbytes))
            self._chk(self.lib.zp_h2d(self.ctx, d_s.ptr, scs.ctypes.data, scs.nbytes))
        out = (C.c_uint32 * 16)()
        self._chk(self.lib.zp_msm_bn254(self.ctx, d_p.ptr, d_s.ptr, n, out))
        x = sum(int(out[k]) << (32 * k) for k in range(8))
        y = sum(int(out[8 + k]) << (32 * k) for k in range(8))
        return None if (x == 0 and y == 0) else (x, y)

    def msm_bn254_g2(self, points, scalars):
        """points: list of ((x0, x1), (y0, y1)) ints over F_q2 (None or zeros = infinity); scalars: ints.
        Returns ((x0, x1), (y0, y1)) or None."""
        n_ = len(points)
        pts = np.zeros((max(n_, 1), 32), dtype=np.uint32)
        scs = np.zeros((max(n_, 1), 8), dtype=np.uint32)
        for i, (p, s) in enumerate(zip(points, scalars)):
            if p is not None:
                for c, v in enumerate((p[0][0], p[0][1], p[1][0], p[1][1])):
                    for k in range(8):
                        pts[i, 8 * c + k] = (v >> (32 * k)) & 0xFFFFFFFF
            for k in range(8):
                scs[i, k] = (s >> (32 * k)) & 0xFFFFFFFF
        return self.msm_bn254_g2_arrays(pts[:n_], scs[:n_])

    def msm_bn254_g2_arrays(self, pts, scs):
        """pts u32[n][32] (x0, x1, y0, y1, eight words each; all zero = infinity), scs u32[n][8] -> ((x0, x1), (y0, y1)) or None"""
        pts = np.ascontiguousarray(pts, dtype=np.uint32)
        scs = np.ascontiguousarray(scs, dtype=np.uint32)
        n_ = pts.shape[0]
        d_p = DeviceBuffer(self, max(1, pts.size // 2 + 1))
        d_s = DeviceBuffer(self, max(1, scs.size // 2 + 1))
        if n_:
            self._chk(self.lib.zp_h2d(self.ctx, d_p.ptr, pts.ctypes.data, pts.nbytes))
            self._chk(self.lib.zp_h2d(self.ctx, d_s.ptr, scs.ctypes.data, scs.nbytes))
        out = (C.c_uint32 * 32)()
        self._chk(self.lib.zp_msm_bn254_g2(self.ctx, d_p.ptr, d_s.ptr, n_, out))
        v = [sum(int(out[8 * c + k]) << (32 * k) for k in range(8)) for c in range(4)]
        return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))

    # ---- host-buffer forms
    def ntt_host(self, cols, inverse=False):
        a = np.ascontiguousarray(np.asarray(cols, dtype=np.uint64)).copy()
        W, N = a.shape
        self._chk(self.lib.zp_ntt_host(self.ctx, a.ctypes.data_as(_u64p), N.bit_length() - 1, W, int(inverse)))
        return a

    def lde_host(self, cols, logb, shift=0):
        a = np.ascontiguousarray(np.asarray(cols, dtype=np.uint64))
        W, N = a.shape
        out = np.empty((W, N << logb), dtype=np.uint64)
        self._chk(self.lib.zp_lde_host(self.ctx, a.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p),
                                       N.bit_length() - 1, logb, W, shift))
        return out

    def merkle_commit_host(self, cols):
        a = np.ascontiguousarray(np.asarray(cols, dtype=np.uint64))
        W, M = a.shape
        tree = np.empty((2 * M - 1, 4), dtype=np.uint64)
        self._chk(self.lib.zp_merkle_commit_host(self.ctx, a.ctypes.data_as(_u64p), M, W,
                                                 tree.ctypes.data_as(_u64p)))
        return tree

    # ---- measurement
    def set_tuning(self, key, value):
        self._chk(self.lib.zp_set_tuning(self.ctx, key.encode(), int(value)))

    def set_profiling(self, on):
        self._chk(self.lib.zp_set_profiling(self.ctx, int(bool(on))))

    def pass_timings(self, cap=4096):
        ms = (C.c_float * cap)()
        rl = (C.c_int32 * cap)()
        n = C.c_int32(0)
        self._chk(self.lib.zp_get_pass_timings(self.ctx, ms, rl, cap, C.byref(n)))
        return [(rl[i], ms[i]) for i in range(n.value)]

    def stage_timings(self):
        buf = C.create_string_buffer(1 << 20)
        self._chk(self.lib.zp_stage_timings(self.ctx, buf, 1 << 20))
        return json.loads(buf.value.decode())

    # ---- introspection
    def ntt_plan(self, logn):
        buf = C.create_string_buffer(4096)
        self._chk(self.lib.zp_ntt_plan_json(self.ctx, logn, buf, 4096))
        return json.loads(buf.value.decode())

    def device_info(self):
        buf = C.create_string_buffer(4096)
        self._chk(self.lib.zp_device_info_json(self.ctx, buf, 4096))
        return json.loads(buf.value.decode())
