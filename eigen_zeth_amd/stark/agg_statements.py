"""The statements an aggregated proof is verified under (zp_aggregate_verify, include/zeth_prover.h), as tuples for native.agg_statements and as a
FILE for compiled hosts: host/verify_chunk.cpp reads it in its "aggregated" mode, and this is the only way such a host gets verifier-AIR programs
(they are made per shape by stark/verifier_air.py).

File layout, little-endian u64 words:  b"ZPAGST1\\0" | n_statements | per statement:
    shape_bytes (0: the leaf statement) | the shape dictionary as JSON text, zero padded to whole words | program_words | the program blob |
    logn | logb | fri_logf | fri_final_log | n_queries | pow_bits | n_slots"""
import json

import numpy as np

from . import verifier_air as VA

MAGIC = int.from_bytes(b"ZPAGST1\0", "little")


def shapes_of(agg):
    """the distinct shape dictionaries of an aggregated proof's tree, outermost first (untrusted text: Shape.from_dict bounds every member)"""
    seen, out = set(), []

    def walk(node, depth):
        if depth > 8 or not isinstance(node, dict):
            raise ValueError("aggregated proof nested too deep")
        d = node.get("shape")
        if d is not None:
            key = VA.Shape.from_dict(d).key()
            if key not in seen:
                seen.add(key)
                out.append(dict(d))
        for kid in node.get("children") or []:
            walk(kid, depth + 1)
    walk(agg, 1)
    return out


def statements_for(agg, leaf_program, leaf_params, params_of_shape, rc, mds):
    """[(shape dict or None, program, params, n_slots)]: the leaf statement, then one per shape of the tree.  params_of_shape(Shape) -> the VERIFIER's
    StarkParams of a STARK over the verifier AIR of that shape (it must not come from the text)"""
    out = [(None, np.ascontiguousarray(leaf_program, dtype=np.uint64), leaf_params, 0)]
    for d in shapes_of(agg):
        sh = VA.Shape.from_dict(d)
        out.append((d, np.ascontiguousarray(VA.verifier_air(sh, rc, mds).program(), dtype=np.uint64), params_of_shape(sh), sh.n_slots()))
    return out


def write_table(path, statements):
    """the statement-table file of `statements` (tuples as above)"""
    words = [np.array([MAGIC, len(statements)], dtype=np.uint64)]
    for shape, program, params, n_slots in statements:
        d = params.to_dict() if hasattr(params, "to_dict") else dict(params)
        text = b"" if shape is None else json.dumps(shape).encode()
        padded = text + b"\0" * (-len(text) % 8)
        prog = np.ascontiguousarray(program, dtype=np.uint64)
        words += [np.array([len(text)], dtype=np.uint64), np.frombuffer(padded, dtype=np.uint64), np.array([prog.size], dtype=np.uint64), prog,
                  np.array([d["logn"], d["logb"], d["fri_logf"], d["fri_final_log"], d["n_queries"], d.get("pow_bits", 0), int(n_slots or 0)], dtype=np.uint64)]
    np.concatenate(words).tofile(path)
