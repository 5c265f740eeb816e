"""zp_r1cs_eval_device (csrc/r1cs.hip, r1cs_poseidon17_kernel of csrc/poseidon_bn254.hip) against the host evaluator zp_r1cs_eval on the seeded
small circuits of tests/r1cs_cases.py -- the witness step of every Groth16 wrap at its own seams: gadget waves that are no multiple of the
three instances a block takes and do not start at one, more than 256 explicit rows, a chain of definitions, 256 + 1 arithmetic instances,
explicit rows and gadget inputs that read an arithmetic instance's wire, no gadget at all, two circuits in turn on one ctx.  Every comparison
is exact: witness, A w, B w, C w (the zero rows up to 2^logm included), public inputs, and for a refused assignment the code and *bad."""
import functools
import time

import numpy as np
import pytest

import r1cs_cases as RC
from eigen_zeth_amd import native
from oracle import r1cs_blob as RB

pytestmark = pytest.mark.gpu
ZP_ERR_ARG = -1


@pytest.fixture(scope="module")
def dev(prover):
    prover.install_poseidon_bn254(17)
    return prover


@functools.lru_cache(maxsize=None)
def host(name, value_seed=None):
    """the host's evaluation of a case, once: (witness, A w, B w, C w)"""
    cs = RC.case(name, value_seed)
    return native.r1cs_eval(cs.blob, *cs.arrays())


def assert_equals_host(got, name, value_seed=None):
    cs = RC.case(name, value_seed)
    wf, a, b, c = host(name, value_seed)
    gw, ga, gb, gc, gpub = got
    assert ga.shape == a.shape == (1 << cs.logm, 4)
    for what, x, y in (("witness", gw, wf), ("A w", ga, a), ("B w", gb, b), ("C w", gc, c)):
        diff = np.flatnonzero((x != y).any(axis=1))
        assert diff.size == 0, "%s of %s differs from the host at %d places, first %d" % (what, name, diff.size, diff[0])
    assert gpub == native.fr_ints(wf[1:1 + cs.n_pub])


def device_refusal(dev, cs, set_idx, set_val):
    """(code, bad) of zp_r1cs_eval_device for an assignment it refuses"""
    try:
        dev.r1cs_eval_device(cs.blob, set_idx, set_val)
    except ValueError as e:
        return -20, int(str(e).split("constraint ")[1].split(")")[0])
    except native.ZpError as e:
        return e.code, e.bad
    raise AssertionError("accepted")


@pytest.mark.parametrize("name", sorted(RC.SHAPES))
def test_device_evaluator_equals_the_host_word_for_word(dev, name):
    cs = RC.case(name)
    host(name)
    t0 = time.perf_counter()
    got = dev.r1cs_eval_device(cs.blob, *cs.set_lists())
    print("%s: %d wires, %d constraints, zp_r1cs_eval_device + downloads %.1f ms" % (name, cs.n_wires, cs.n_cons, 1e3 * (time.perf_counter() - t0)))
    assert_equals_host(got, name)
    if name != "S3":             # the checker's own reader of the blob (Python integers: seconds at S3's size, and S3's rows are the other shapes' rows)
        assert RB.first_violated(cs.blob, native.fr_ints(got[0])) == -1


@pytest.mark.parametrize("fault", ["unset: wave0_input", "unset: only_wave1", "unset: only_plain", "unset: only_mid_def", "unset: arith_input", "unset: unread",
                                   "violated: a defined wire set off by one", "violated: a plain row", "violated: a plain row, in the top limb only",
                                   "violated: e3_inv of zero in the second arithmetic instance"])
def test_device_refuses_what_the_host_refuses_with_the_same_code_and_place(dev, fault):
    cs = RC.case("S2")
    vals = RC.faults(cs)[fault]
    want = RC.host_refusal(cs, vals)
    assert want[0] == (-21 if fault.startswith("unset") else -20) and want[1] >= 0
    assert device_refusal(dev, cs, *cs.set_lists(vals)) == want


def test_one_ctx_two_circuits_in_turn_and_nothing_carried_over(dev):
    """the blob cache replaced and refilled, the host witness of the arithmetic templates (hW, its set flags, the wires the last proof touched)
    between proofs: after another circuit, after a refused proof, with other values on the same wires, after a larger and a smaller circuit"""
    s2, s4 = RC.case("S2"), RC.case("S4")
    first = dev.r1cs_eval_device(s2.blob, *s2.set_lists())
    assert_equals_host(first, "S2")
    assert_equals_host(dev.r1cs_eval_device(s4.blob, *s4.set_lists()), "S4")
    missing = s2.without(s2.tags["arith_input"])
    assert device_refusal(dev, s2, *s2.set_lists(missing)) == RC.host_refusal(s2, missing)
    again = dev.r1cs_eval_device(s2.blob, *s2.set_lists(order_seed=8))
    assert all((x == y).all() for x, y in zip(first[:4], again[:4])) and first[4] == again[4]
    other = RC.case("S2", 9)
    assert (other.blob == s2.blob).all() and sorted(other.vals) == sorted(s2.vals) and other.vals != s2.vals
    assert_equals_host(dev.r1cs_eval_device(other.blob, *other.set_lists()), "S2", 9)
    for name in ("S3", "S1"):
        cs = RC.case(name)
        assert_equals_host(dev.r1cs_eval_device(cs.blob, *cs.set_lists()), name)


def test_entry_refuses_wires_inside_an_instance_and_wires_named_twice(dev):
    """zp_r1cs_eval_device takes caller-set wires only (include/zeth_prover.h): a wire internal to a gadget or arithmetic instance, or one wire
    named twice (the scatter kernel would write both values in no order), is ZP_ERR_ARG -- and the next correct call is unharmed"""
    cs = RC.case("S2")
    ref = native.fr_ints(host("S2")[0])
    idx, val = cs.set_lists()
    gadget_wire = cs.circuit.instances[0][1]                     # the first internal wire of gadget instance 0
    arith_wire = cs.circuit.ariths[0][1][1][1]                   # ... of the second arithmetic instance
    for wire in (gadget_wire, gadget_wire + RC.TC - 1, arith_wire, arith_wire + cs.tags["arith_n_int"] - 1):
        vals = cs.with_value(wire, ref[wire])                   # the RIGHT value: refused for where it is, not for what it is
        assert device_refusal(dev, cs, *cs.set_lists(vals))[0] == ZP_ERR_ARG, wire
    twice_idx = np.concatenate([idx, idx[5:6]])
    for v in (val[5:6], native.fr_words([(native.fr_ints(val[5:6])[0] + 1) % RC.R])):      # the same value again, and another
        assert device_refusal(dev, cs, twice_idx, np.concatenate([val, v]))[0] == ZP_ERR_ARG
    assert_equals_host(dev.r1cs_eval_device(cs.blob, idx, val), "S2")


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_groth16_over_a_small_circuit_equals_the_trapdoor_proof(dev, tables, name):
    """the whole prover on circuits that are not the wrap's: r1cs_gather_kernel on another subset of B's columns, QAP transforms on 2^10 and
    2^14 points, MSMs over scalars full of 0, 1 and r - 1"""
    from eigen_zeth_amd.poseidon_constants import bn254_poseidon_params
    from eigen_zeth_amd.service import groth16 as G16
    from eigen_zeth_amd.stark.backend_hip import HipBackend
    from oracle import groth16_verify as GV
    from cpu_wrap_backend import CpuWrapBackend
    cs = RC.case(name)
    hip = HipBackend(prover=dev, hash_mode="bn128")
    cpu = CpuWrapBackend(*tables, hash_mode="bn128", bn_tables=bn254_poseidon_params(17))
    key = G16.Key(cs.blob)
    rand = (0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321)
    idx, val = cs.set_lists()
    p_gpu, pubs, _ = G16.prove(key, idx, val, hip, rand)
    p_cpu, pubs_c, _ = G16.prove(key, idx, val, cpu, rand)
    assert pubs == pubs_c == native.fr_ints(host(name)[0][1:1 + cs.n_pub])
    assert p_gpu == p_cpu
    assert GV.verify(key.vk, p_gpu, pubs)
    assert not GV.verify(key.vk, p_gpu, [(pubs[0] + 1) % G16.R])
