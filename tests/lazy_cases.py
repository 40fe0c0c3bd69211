"""The one table of the lazy-state contract: every exported function of include/qsim.h, and of the headers it pulls in with
#include "qsim_*.h", whose first parameter is a qsim_state.

A state handle does not always hold its amplitudes in memory (engine_state.h): |0...0> may be PENDING, the state may be PARTIAL —
written only inside `support`, the memory outside it zero by definition and never written — or it may hold nothing.  Every entry
point that is not a tile pass opens with settle() / written(), which launches the queued gates and writes the promised zeros.  That
rule is kept by hand, once per entry point; this table is where each entry point either gets a CASE that tests/test_gpu_lazy_states.py
runs from every lazy start over poisoned memory, or an EXEMPTION with its reason.  tests/test_lazy_cases_cpu.py holds the table's
keys to the header: a new entry point without an entry here fails there.

A case names the Simulator method that drives the call, its operands for n = 15 as plain data, and how its result is compared:
  bits  the returned values, the destination buffers and the state afterwards equal those of the same call on a dense twin bit for
        bit.  After settle() the two buffers are identical and every one of these calls promises equal bits for equal calls.
  ref   only for calls that pass through the gate queue: knowing the support, the scheduler groups passes differently (the comment in
        test_gpu_parity.py::test_sparse_start_visits_only_the_support), so the result is held to the feature's numpy checker with
        the tolerance its module derives.  `why_ref` names the line that queues the gates.

Plain Python: nothing here imports the library or touches a device."""
import math

N = 15
FULL = (1 << N) - 1

# the two partial supports of the starts: the pattern of test_support_api_and_zero_shard_semantics, and one with the top qubit
# inside and qubit 0 outside, so that every 16-byte unit of an fp32 state has a slot that is NaN in memory
SUPPORT_LOW = (0, 1, 2, 3, 5, 6, 9, 10, 12)
SUPPORT_HIGH = (1, 2, 4, 7, 8, 11, 13, 14)
STARTS = ("pending", "support_low", "support_high", "circuit")
SUPPORTS = {"support_low": SUPPORT_LOW, "support_high": SUPPORT_HIGH}

# the `circuit` start: (n, depth, seed, vocabulary) of circuits.random_gates — a dense run that leaves garbage in both buffers, then,
# after a reset, gates on qubits 0..4 (X gates among them) that stay queued
DENSE_CIRCUIT = (N, 300, 6, "all")
FEW_CIRCUIT = (5, 80, 13, "all")

READ, IN_PLACE, INTO, GRADIENT = "read-only", "in place", "into another buffer", "gradient"
PLAN_MAIN, PLAN_SMALL, PLAN_FORWARDED = 1, 0, 2  # the *path a feature's plan call reports


class Exempt:
    def __init__(self, reason):
        self.reason = reason


class Case:
    """name: the test id; method: the Simulator attribute that drives the call; group: one of the four above; compare: "bits" or
    "ref" (then why_ref says where the gates are queued); operands: keyword data the driver of `method` understands."""

    def __init__(self, name, method, group, compare="bits", why_ref="", **operands):
        self.name, self.method, self.group, self.compare, self.why_ref, self.operands = name, method, group, compare, why_ref, operands


def _mask(bits):
    return sum(1 << b for b in bits)


def affine_table(k, a, b):
    """The bijection j -> (a j + b) mod 2^k of range(2^k), a odd."""
    assert a % 2 == 1
    return [(a * j + b) % (1 << k) for j in range(1 << k)]


def matrix_entries(k, seed):
    """A dense complex 2^k x 2^k matrix as nested lists (nothing checks unitarity): entries of modulus below 1 from a fixed recurrence."""
    d = 1 << k
    x = seed
    rows = []
    for _ in range(d):
        row = []
        for _ in range(d):
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            re = ((x >> 11) % 2001 - 1000) / 1000.0
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            im = ((x >> 11) % 2001 - 1000) / 1000.0
            row.append(complex(re, im) / math.sqrt(d))
        rows.append(row)
    return rows


# ---- operands ---------------------------------------------------------------------------------------------------------------------
# Qubit sets: LOW_ONLY lies inside SUPPORT_LOW and wholly outside SUPPORT_HIGH, HIGH_ONLY the other way round, so that a case on one
# of them has all its targets and controls inside the support from one partial start and a target AND a control outside it from the other.
LOW_ONLY = (0, 3, 5, 9, 12)
HIGH_ONLY = (4, 7, 13, 8, 14)
assert set(LOW_ONLY) <= set(SUPPORT_LOW) and not set(LOW_ONLY) & set(SUPPORT_HIGH)
assert set(HIGH_ONLY) <= set(SUPPORT_HIGH) and not set(HIGH_ONLY) & set(SUPPORT_LOW)

PAULIS = ["X0 Z3", "Y14 X7", "Z14", "X4 Y5 Z6", "Z0 Z1", "", "X13", "Y2 Y11 X12", "Z9 Z10 Z12"]
HAMILTONIAN = [(-1.0, "Z0 Z1"), (-0.7, "X0"), (-0.7, "X14"), (0.5, "Y3 Z9"), (0.3, "X7 X8"), (0.25, "Z4 Z13"), (-0.4, "Y2 X11")]
DIAGONAL_TERMS = [(0.8, "Z0"), (-0.6, "Z14"), (0.45, "Z3 Z7"), (0.3, "Z1 Z8 Z13"), (-0.2, "Z5 Z9"), (0.15, "")]
DRAWS = [0.0, 1e-9, 0.03, 0.1, 0.25, 0.4, 0.5, 0.61, 0.75, 0.9, 0.999, 0.9999999, 1.0]

# multi-qubit strings only: every term goes to a sweep (plans.pauli_rotation_plan reports no term queued as a gate)
ROTATIONS_MULTI = [(0.6, "X14 X0"), (-1.2, "X14 X0 Z9"), (0.4, "Z12 Z3"), (2.2, "Y10 X5"), (0.3, "Z7 Z13"), (-0.9, "X4 Y8 Z1"), (1.1, "Y13 Y2")]
# single-qubit X / Y strings travel through the gate queue; from either partial start some of their qubits lie outside the support
ROTATIONS_MIXED = [(0.7, "X4"), (0.6, "X14 X0"), (-0.5, "Y13"), (0.4, "Z12 Z3"), (0.9, "X0"), (2.2, "Y10 X5"), (-1.3, "Y9"), (0.3, "X2 Z11")]
# under controls only "one control and X or Y on one qubit" is queued (as its 4x4): none of these is
ROTATIONS_CONTROLLED = [(0.8, "X1 X13", (2,)), (-0.6, "Z5", (0, 14)), (1.4, "Y4", (7, 8)), (0.5, "", (3, 12)), (0.35, "X6 Z10", ()), (-1.1, "Y11 Z2", (1,))]
GRADIENT_ROTATIONS = [(0.6, "X14 X0"), (-1.2, "Y3 Z9"), (0.4, "Z12 Z3"), (0.7, "X7 Y8"), (0.3, "Z13")]
GRADIENT_CONTROLLED = [(0.8, "X1 X13", (2,)), (0.6, "X14 X0"), (-0.6, "Z5", (0, 14)), (1.4, "Y4", (7, 8)), (0.5, "", (3, 12))]
# (gamma, "diagonal") stands for a step exp(-i gamma D) on the table of DIAGONAL_TERMS
GRADIENT_DIAGONAL = [(0.6, "X14 X0"), (0.35, "diagonal"), (-1.2, "Y3 Z9"), (-0.2, "diagonal"), (0.7, "X7 Y8")]

# the Fourier transform's register: its first ten qubits are one in-place sweep, all twelve under a cap of 4 bits a digit are three
# sweeps, two of them into the second buffer
QFT_REGISTER = (14, 0, 3, 7, 9, 1, 12, 5, 13, 10, 4, 8)
# measured qubits: one set inside SUPPORT_LOW; no qubit lies outside BOTH partial supports (together they cover the register), so the
# other set has a qubit outside each of them — 4 outside SUPPORT_LOW, 0 outside SUPPORT_HIGH, both outside what `pending` holds
MEASURE_INSIDE_LOW = (9, 0, 5)
MEASURE_OUTSIDE = (4, 14, 0)
assert set(MEASURE_INSIDE_LOW) <= set(SUPPORT_LOW)
assert set(MEASURE_OUTSIDE) - set(SUPPORT_LOW) and set(MEASURE_OUTSIDE) - set(SUPPORT_HIGH)

CASES = {
    # ---- read-only ----------------------------------------------------------------------------------------------------------------
    "qsim_read": [Case("read_subrange", "read", READ, first=1001, count=20000)],
    "qsim_norm2": [Case("norm2", "norm2", READ)],
    "qsim_expect_paulis": [Case("expectation_terms", "expectation_terms", READ, paulis=PAULIS)],
    "qsim_sample": [Case("sample", "sample", READ, randoms=DRAWS)],
    "qsim_sample_shots": [Case("sample_shots_all", "sample_shots", READ, draws=DRAWS, qubits=None),
                          Case("sample_shots_subset", "sample_shots", READ, draws=DRAWS, qubits=(14, 0, 7, 3))],
    "qsim_block_prob_masked": [Case("block_prob_masked", "block_prob_masked", READ, hi_mask=_mask((0, 4, 9, 13, 14)), lo_mask=FULL & ~_mask((0, 4, 9, 13, 14)))],
    "qsim_gather_masked": [Case("gather_masked", "gather_masked", READ, base=_mask((1, 12)), lo_mask=_mask((0, 2, 3, 4, 7, 9, 13, 14)))],
    "qsim_reduced_density": [Case("reduced_density_3", "reduced_density_matrix", READ, qubits=(13, 2, 6), plan=PLAN_MAIN),
                             Case("reduced_density_5", "reduced_density_matrix", READ, qubits=(14, 0, 5, 9, 11), plan=PLAN_MAIN)],
    # (n = 15 offers the density calls one path each: the plain kernels need n - k < 2; k <= 5 is forwarded to qsim_reduced_density)
    "qsim_subsystem_density": [Case("subsystem_density_7", "subsystem_density_matrix", READ, qubits=(13, 0, 3, 14, 8, 4, 11), plan=PLAN_MAIN),
                               Case("subsystem_density_forwarded", "subsystem_density_matrix", READ, qubits=(14, 1, 7), plan=PLAN_FORWARDED)],
    "qsim_expect_diagonal": [Case("expectation_diagonal", "expectation_diagonal", READ, terms=DIAGONAL_TERMS)],
    "qsim_inner": [Case("inner", "inner", READ)],
    "qsim_device_ptr": [Case("device_ptr", "device_ptr", READ)],
    # ---- in place -----------------------------------------------------------------------------------------------------------------
    "qsim_write": [Case("write_subrange", "write", IN_PLACE, first=3001, count=5000, seed=71)],
    "qsim_apply_pauli_rotations": [
        Case("rotations_multi", "apply_pauli_rotations", IN_PLACE, rotations=ROTATIONS_MULTI, queued=0),
        Case("rotations_mixed", "apply_pauli_rotations", IN_PLACE, "ref",
             "pauli.cpp apply_rotations: `QSIM_TRY(qsim_apply_1q(s, U, target))` for a term that is X or Y on one qubit",
             rotations=ROTATIONS_MIXED, queued=4)],
    "qsim_apply_controlled_pauli_rotations": [Case("rotations_controlled", "apply_pauli_rotations", IN_PLACE, rotations=ROTATIONS_CONTROLLED, queued=0)],
    "qsim_apply_matrix": [
        Case("matrix_low", "apply_matrix", IN_PLACE, targets=LOW_ONLY[:3], controls=LOW_ONLY[3:], seed=11, plan=PLAN_MAIN),
        Case("matrix_high", "apply_matrix", IN_PLACE, targets=HIGH_ONLY[:3], controls=HIGH_ONLY[3:], seed=12, plan=PLAN_MAIN),
        Case("matrix_five", "apply_matrix", IN_PLACE, targets=(2, 6, 11, 1, 14), controls=(), seed=13, plan=PLAN_MAIN),
        Case("matrix_small", "apply_matrix", IN_PLACE, targets=(13, 1), controls=(0, 2, 3, 4, 5, 6, 7, 8, 9, 10), seed=14, plan=PLAN_SMALL)],
    "qsim_apply_permutation": [
        Case("permutation_low", "apply_permutation", IN_PLACE, targets=LOW_ONLY[:3], controls=LOW_ONLY[3:], table=affine_table(3, 5, 3), plan=PLAN_MAIN),
        Case("permutation_high", "apply_permutation", IN_PLACE, targets=HIGH_ONLY[:3], controls=HIGH_ONLY[3:], table=affine_table(3, 3, 6), plan=PLAN_MAIN),
        Case("permutation_ten", "apply_permutation", IN_PLACE, targets=(14, 0, 3, 7, 9, 1, 12, 5, 13, 10), controls=(), table=affine_table(10, 421, 77), plan=PLAN_MAIN),
        Case("permutation_small", "apply_permutation", IN_PLACE, targets=(14, 0, 6), controls=(1, 2, 4, 8), table=affine_table(3, 7, 1), plan=PLAN_SMALL)],
    "qsim_apply_diagonal_phase": [Case("diagonal_phase", "apply_diagonal_phase", IN_PLACE, terms=DIAGONAL_TERMS, gamma=0.37)],
    # (qft.cpp queues nothing: settle(), then one sweep per digit.  The operands are tests/test_gpu_qft.py's LAZY_SINGLE and LAZY_MOVING)
    "qsim_apply_qft": [Case("qft_single", "apply_qft", IN_PLACE, qubits=QFT_REGISTER[:10], max_digit_bits=0, moving=False),
                       Case("qft_moving", "apply_qft", IN_PLACE, qubits=QFT_REGISTER, max_digit_bits=4, moving=True)],
    # (measure.hip queues nothing: settle(), the weight sweep, the collapse sweep.  The outcome post-selected is the most probable one
    # of the start's state, which the driver works out; the qubit sets and the draw are tests/test_gpu_measure.py's)
    "qsim_postselect": [Case("postselect_inside_low", "postselect", IN_PLACE, qubits=MEASURE_INSIDE_LOW),
                        Case("postselect_outside", "postselect", IN_PLACE, qubits=MEASURE_OUTSIDE)],
    "qsim_measure": [Case("measure_inside_low", "measure", IN_PLACE, qubits=MEASURE_INSIDE_LOW, draw=0.37),
                     Case("measure_outside", "measure", IN_PLACE, qubits=MEASURE_OUTSIDE, draw=0.37)],
    "qsim_scale": [Case("scale", "scale", IN_PLACE, "ref", "engine.cpp qsim_scale: `return qsim_apply_1q(s, U, 0)` — diag(z, z) on qubit 0, queued",
                        z=(0.6, -0.35))],
    # (lanczos.cpp queues nothing: settle(), then sweeps on buffers — both forms compare as bits)
    "qsim_lanczos_ground": [Case("ground_state_estimate", "ground_state", IN_PLACE, terms=HAMILTONIAN, tol=1e-12, max_steps=4, vector=False),
                            Case("ground_state_vector", "ground_state", IN_PLACE, terms=HAMILTONIAN, tol=1e-12, max_steps=4, vector=True)],
    # ---- into another buffer ------------------------------------------------------------------------------------------------------
    "qsim_pauli_sum_into": [Case("pauli_sum_into", "pauli_sum_into", INTO, terms=HAMILTONIAN)],
    "qsim_diagonal_apply_into": [Case("diagonal_into", "diagonal_into", INTO, terms=DIAGONAL_TERMS, weight=0.75)],
    "qsim_copy_state": [Case("copy_from", "copy_from", INTO)],
    "qsim_combine": [Case("combine", "combine", INTO, d=(0.5, -0.25), a=(0.3, 0.7), b=(-0.4, 0.2))],
    "qsim_pack_bits": [Case("pack_bits", "pack_bits", INTO, bits=(3, 11))],
    "qsim_pack_bits_to": [Case("pack_bits_to", "pack_bits_to", INTO, bits=(0, 13))],
    # ---- gradients: lambda in the state's own second buffer, and in a lent spare buffer full of NaN ----------------------------------
    "qsim_pauli_gradient": [Case("pauli_gradient_own", "energy_and_gradient", GRADIENT, rotations=GRADIENT_ROTATIONS, terms=HAMILTONIAN, lent=False),
                            Case("pauli_gradient_lent", "energy_and_gradient", GRADIENT, rotations=GRADIENT_ROTATIONS, terms=HAMILTONIAN, lent=True)],
    "qsim_controlled_pauli_gradient": [
        Case("controlled_gradient_own", "energy_and_gradient", GRADIENT, rotations=GRADIENT_CONTROLLED, terms=HAMILTONIAN, lent=False),
        Case("controlled_gradient_lent", "energy_and_gradient", GRADIENT, rotations=GRADIENT_CONTROLLED, terms=HAMILTONIAN, lent=True)],
    "qsim_diagonal_gradient": [
        Case("diagonal_gradient_own", "energy_and_gradient", GRADIENT, rotations=GRADIENT_DIAGONAL, terms=HAMILTONIAN, observable=0.5, lent=False),
        Case("diagonal_gradient_lent", "energy_and_gradient", GRADIENT, rotations=GRADIENT_DIAGONAL, terms=HAMILTONIAN, observable=0.5, lent=True)],
}

_HOST = "host only: reads fields of the handle, never the amplitude buffer"
_DEFINES = "sets or reports the lazy condition itself; every start of test_gpu_lazy_states.py goes through it"
_QUEUE = "a gate-queue call: tile passes over a partial state are test_gpu_sparse_reads.py's and test_gpu_affine_support.py's"
_KEEP = "the keep-partial path (settle(s, keep_partial)): test_gpu_sparse_reads.py and test_gpu_fp32_paths.py own it"
_PLANNING = "planning: schedules (and times) a circuit, the state's contents are clobbered and left reset by contract"
_LOG = "profile bookkeeping: returns host records of past launches, never amplitudes"

EXEMPT = {
    "qsim_precision_bits": Exempt(_HOST),
    "qsim_num_qubits": Exempt(_HOST),
    "qsim_get_option": Exempt(_HOST),
    "qsim_set_option": Exempt("launches the queued gates (options apply to gates queued later) and sets a host field; looks at no amplitude"),
    "qsim_plan_cache_stats": Exempt(_HOST),
    "qsim_deferred_flip_stats": Exempt(_HOST),
    "qsim_holds_nothing": Exempt(_DEFINES),
    "qsim_destroy": Exempt("frees the buffers without looking at them"),
    "qsim_reset": Exempt(_DEFINES),
    "qsim_reset_shard": Exempt(_DEFINES),
    "qsim_set_support": Exempt(_DEFINES),
    "qsim_get_support": Exempt(_DEFINES),
    "qsim_flush": Exempt("launches the queue and nothing else: a partial state stays partial by contract"),
    "qsim_sync": Exempt("written() and a wait: it is what settles a state, and every case's final read() goes through it"),
    "qsim_stream": Exempt(_HOST),
    "qsim_state_buffer": Exempt("documented to launch nothing and write nothing first: for a caller about to overwrite the buffer"),
    "qsim_swap_buffer": Exempt("flushes only, by contract: the buffer handed in IS the state afterwards, written everywhere"),
    "qsim_set_spare_buffer": Exempt("flushes only, by contract: the lent buffer's contents are garbage to the engine (the lent-spare gradient cases lend NaN)"),
    "qsim_apply_1q": Exempt(_QUEUE),
    "qsim_apply_cx": Exempt(_QUEUE),
    "qsim_apply_2q": Exempt(_QUEUE),
    "qsim_run_circuit": Exempt(_QUEUE),
    "qsim_flush_pack": Exempt(_KEEP),
    "qsim_pack_bits_sparse": Exempt(_KEEP),
    "qsim_sample_stage_times": Exempt("a measurement aid of tools/sample_bench.py: returns two event times, nothing that depends on an amplitude"),
    "qsim_tune_circuit": Exempt(_PLANNING),
    "qsim_tune_circuit_from": Exempt(_PLANNING),
    "qsim_tune_circuit_support": Exempt(_PLANNING),
    "qsim_choose_schedule": Exempt("planning on the host: schedules candidates, launches nothing"),
    "qsim_choose_schedule_while_allocating": Exempt("planning on the host while the buffer is still being allocated: launches nothing"),
    "qsim_choose_schedule_for": Exempt("planning on the host: schedules candidates, launches nothing"),
    "qsim_support_after": Exempt("planning on the host: the circuit is scheduled, nothing runs"),
    "qsim_get_stats": Exempt(_LOG),
    "qsim_reset_stats": Exempt(_LOG),
    "qsim_launch_log": Exempt(_LOG),
    "qsim_launch_log_order": Exempt(_LOG),
    "qsim_launch_log_visited": Exempt(_LOG),
    "qsim_launch_log_read_share": Exempt(_LOG),
    "qsim_launch_log_blocks": Exempt(_LOG),
    "qsim_launch_log_block_flags": Exempt(_LOG),
}

TABLE = {**CASES, **EXEMPT}
assert len(TABLE) == len(CASES) + len(EXEMPT), "an entry point is both a case and an exemption"


def all_cases():
    """[(C function, Case)] in table order."""
    return [(fn, case) for fn, cases in CASES.items() for case in cases]
