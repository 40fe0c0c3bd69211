"""The tests' own checker for controlled Pauli rotations (1 - Pi) + Pi exp(-i theta/2 P), Pi = "every control qubit is 1":
pauli_rot_ref.apply_rotation with its result kept where (j & c) == c and the input kept elsewhere, in complex128 or complex64
(tests/test_controlled_rot_cpu.py pins it against dense operators), and the sequences of tests/test_gpu_controlled_rot.py as data,
so that the CPU test can hold every fp32 sequence to fp32_ref.REF_CAP.

A term is (theta, c, x, z): the control mask and the string's two masks (tests/pauli_ref.py); c & (x | z) == 0."""
import itertools
import math

import numpy as np

import pauli_ref
import pauli_rot_ref
from pauli_rot_ref import rand_state  # noqa: F401  (the start states of the sequences)


def apply_rotation(psi, c, x, z, theta, dtype=np.complex128):
    psi = np.asarray(psi, dtype=dtype)
    j = np.arange(psi.size, dtype=np.uint64)
    inside = (j & np.uint64(c)) == np.uint64(c)
    return np.where(inside, pauli_rot_ref.apply_rotation(psi, x, z, theta, dtype), psi).astype(dtype)


def replay(psi, rotations, dtype=np.complex128):
    """`rotations` = [(theta, c, x, z), ...] applied in order, the first one first."""
    out = np.asarray(psi, dtype=dtype)
    for theta, c, x, z in rotations:
        out = apply_rotation(out, c, x, z, theta, dtype)
    return out


def dense_controlled(c, x, z, n, theta):
    j = np.arange(1 << n)
    pi = np.diag(((j & c) == c).astype(np.float64))
    return (np.eye(1 << n) - pi) + pi @ pauli_rot_ref.dense_rotation(x, z, n, theta)


def controls_of(c, n):
    return tuple(q for q in range(n) if c >> q & 1)


def mask_of(qubits):
    return sum(1 << q for q in qubits)


def entries(rotations, n):
    """[(theta, c, x, z)] -> [(theta, "X0 Z3 ...", (controls...))] as Simulator.apply_pauli_rotations takes them."""
    return [(theta, pauli_ref.masks_to_text(x, z, n), controls_of(c, n)) for theta, c, x, z in rotations]


def uncontrolled(rotations):
    """The same terms without their controls, as pauli_rot_ref takes them."""
    return [(theta, x, z) for theta, _, x, z in rotations]


def plan(rotations, n, precision=64):
    """(sweeps, terms queued as gates, units visited) of [(theta, c, x, z)] on n qubits: plans.controlled_rotation_plan."""
    from gpu_quantum_simulator_amd import plans
    cs, xs, zs = ([r[i] for r in rotations] for i in (1, 2, 3))
    p = plans.ok(plans.controlled_rotation_plan(cs, xs, zs, n, precision, num_terms=len(cs)))
    return p["sweeps"], p["queued_as_gates"], p["units_visited"]


def takes_the_gate_queue(c, x, z):
    return bin(c).count("1") <= 1 and bin(x).count("1") == 1 and not z & ~x


def random_string(rng, n, c, weight=None):
    """A random string on the qubits outside c (of `weight` factors, default random, at least one where there is room)."""
    free = [q for q in range(n) if not c >> q & 1]
    if not free:
        return 0, 0
    weight = int(rng.integers(1, len(free) + 1)) if weight is None else min(weight, len(free))
    x = z = 0
    for q in rng.choice(free, size=weight, replace=False):
        letter = "XYZ"[rng.integers(3)]
        x |= (letter in "XY") << int(q)
        z |= (letter in "ZY") << int(q)
    return x, z


# ---- the sequences of tests/test_gpu_controlled_rot.py, as data ---------------------------------------------------------------
EXHAUSTIVE_SIZES = (1, 2, 3, 4)


def exhaustive_terms(n):
    """Every assignment of {control, I, X, Y, Z} to the n qubits with at least one control: 5^n - 4^n terms, random angles."""
    rng = np.random.default_rng(500 + n)
    out = []
    for letters in itertools.product("CIXYZ", repeat=n):
        if "C" not in letters:
            continue
        c = mask_of(q for q in range(n) if letters[q] == "C")
        x = mask_of(q for q in range(n) if letters[q] in "XY")
        z = mask_of(q for q in range(n) if letters[q] in "ZY")
        out.append((float(rng.uniform(-math.pi, math.pi)), c, x, z))
    assert len(out) == 5 ** n - 4 ** n
    return out


def every_position_terms(n=13):
    """One control at each position, each with a paired string whose top x bit lies below the control (where there is a qubit
    below), one whose top x bit lies above it (where there is one above) and an all-Z string; none takes the gate queue."""
    rng = np.random.default_rng(131)
    out = []
    for q in range(n):
        c = 1 << q
        free = ((1 << n) - 1) & ~c
        if q >= 1:
            x = 1 << (q - 1) | (int(rng.integers(0, 1 << (q - 1))) if q >= 2 else 0)
            out.append((float(rng.uniform(-3, 3)), c, x, (int(rng.integers(0, 1 << n)) | 1 << (q + 1) % n) & free))
        if q < n - 1:
            top = int(rng.integers(q + 1, n))
            x = (1 << top | int(rng.integers(0, 1 << top))) & free
            out.append((float(rng.uniform(-3, 3)), c, x, (int(rng.integers(0, 1 << n)) | 1 << (q - 1) % n) & free))
        out.append((float(rng.uniform(-3, 3)), c, 0, int(rng.integers(1, 1 << n)) & free or 1 << (q + 1) % n))
    assert not any(takes_the_gate_queue(c, x, z) for _, c, x, z in out)
    return out


SLOT_N = 10
# fp32: a control on qubit 0 (only the odd slot of a unit is active) with a partner unit (x = 2, x = 0b110) and without (x = 0);
# a control on qubit 1 (and on 1 and 9) with the pair inside one unit (x = 1); Z factors keep all of them out of the gate queue
SLOT_TERMS = [(0.9, 1, 0b10, 1 << 4), (-1.3, 1, 0b110, 0b100 | 1 << 7), (0.7, 1, 0, 0b1010), (2.1, 1, 0, 0), (1.1, 0b10, 1, 1 << 5), (-0.6, 0b10, 1, 1 | 1 << 8),
              (0.8, 1 << 9 | 0b10, 1, 0), (1.7, 1 | 1 << 9, 1 << 8 | 0b10, 0b10)]

SEVERAL_N = 13


def several_controls_terms(n=SEVERAL_N):
    """Random control sets of every size 2..12 with random strings on the rest; controls on both sides of unit bits 7 / 8; all
    but one qubit as controls (two amplitudes visited, or one unit in fp32) and the controlled identity on every qubit (one)."""
    rng = np.random.default_rng(1300)
    out = []
    for size in list(range(2, n)) * 2:
        c = mask_of(int(q) for q in rng.choice(n, size=size, replace=False))
        out.append((float(rng.uniform(-math.pi, math.pi)), c) + random_string(rng, n, c))
    for c in (1 << 7 | 1 << 8, 1 << 6 | 1 << 7 | 1 << 8 | 1 << 9, 1 << 8 | 1 << 9, 1 << 7 | 1):
        out.append((float(rng.uniform(-math.pi, math.pi)), c) + random_string(rng, n, c, 3))
        out.append((float(rng.uniform(-math.pi, math.pi)), c, 0, random_string(rng, n, c, 4)[1] | random_string(rng, n, c, 1)[0]))
    full = (1 << n) - 1
    for q in (0, 1, 7, n - 1):
        out.append((1.3, full & ~(1 << q), 1 << q, 0))         # X on the one free qubit
        out.append((0.8, full & ~(1 << q), 1 << q, 1 << q))    # Y
        out.append((-0.9, full & ~(1 << q), 0, 1 << q))        # Z
    out.append((2.2, full, 0, 0))                              # the phase of |1...1> alone
    return out


BITEXACT_N = 12
BITEXACT_CONTROLS = (1 << 3 | 1 << 9, 1 | 1 << 7 | 1 << 8 | 1 << 11)


def bitexact_terms(c, n=BITEXACT_N):
    """Strings that take a sweep with and without controls: weight >= 2 in x, or all-Z."""
    rng = np.random.default_rng(1200 + c)
    out = []
    while len(out) < 12:
        x, z = random_string(rng, n, c)
        if x == 0 or bin(x).count("1") >= 2:
            out.append((float(rng.uniform(-math.pi, math.pi)), c, x, z))
    return out


RUN_N = 12
RUN_CONTROLS = (1 << 1 | 1 << 8, 1 << 3)  # both outside pauli_rot_ref.LONG_RUN_X


def run_terms(K, controls=RUN_CONTROLS[:1]):
    """The paired run of pauli_rot_ref.long_run_rotations (3K + 5 terms of one x, special angles, anticommuting neighbours) under
    `controls`, term i under controls[i % len(controls)]; the z masks keep clear of every control of RUN_CONTROLS."""
    _, paired = pauli_rot_ref.long_run_rotations(K, RUN_N)
    clear = ~(RUN_CONTROLS[0] | RUN_CONTROLS[1])
    return [(theta, controls[i % len(controls)], x, z & clear) for i, (theta, x, z) in enumerate(paired)]


ORDER_N = 6
ORDER_PAIR = [(theta, 1 << 3, x, z) for theta, x, z in pauli_rot_ref.ORDER_PAIR]  # "X0 X1" and "Y0 X1" under qubit 3

GRID_N = 16
GRID_CONTROLS = (1 << 14, 1 << 2 | 1 << 9 | 1 << 15)


def grid_terms(c, n=GRID_N):
    rng = np.random.default_rng(1600 + bin(c).count("1"))
    return [(float(rng.uniform(-2, 2)), c) + random_string(rng, n, c) for _ in range(24)]


GATE_N = 7
# one control and X or Y on one qubit, the control above and below the target, next to it and far from it
GATE_TERMS = [(0.7, 1 << 5, 1 << 2, 0), (-1.1, 1 << 1, 1 << 4, 1 << 4), (2.3, 1, 1 << 1, 0), (0.4, 1 << 6, 1, 1), (math.pi, 1 << 3, 1 << 4, 0)]
GATE_CIRCUIT = (GATE_N, 60, 61, "all")  # circuits.random_gates: half of it before the terms, half after


def queued_terms(n=13):
    """Controlled and uncontrolled terms mixed, for the run behind live_n13_seed104.qasm."""
    rng = np.random.default_rng(1040)
    out = []
    for i in range(30):
        c = mask_of(int(q) for q in rng.choice(n, size=i % 4, replace=False))
        out.append((float(rng.uniform(-2, 2)), c) + random_string(rng, n, c))
    return out + [(0.5, 0, 1, 0), (0.3, 1 << 4, 1 << 12, 1 << 12), (0.25, 0, 0, 1 << 6), (-0.4, 1 << 2 | 1 << 11, 0, 0)]


FRESH_SIZES = (1, 4, 13)


def fresh_term(n):
    """A controlled term for a never-touched register: no control is 1 in |0...0>, so it changes nothing."""
    return (0.9, 1, 0, 0) if n == 1 else (0.9, 1 << (n - 1), 1 | 1 << (n - 2), 0) if n > 2 else (0.9, 2, 1, 1)


# after fp32_ref.FEW_CIRCUIT (qubits 0..6) on 18 qubits: controls among the touched qubits carry X to the untouched qubit 17 (as a
# sweep under two controls and through the gate queue under one); a control on the untouched qubit 12 finds nothing to rotate
AFTER_FEW_N = 18
AFTER_FEW_REACH = [(1.2, 1 << 2 | 1 << 5, 1 << 17, 0), (0.7, 1 << 4, 1 << 17, 1 << 17), (-0.8, 1 | 1 << 6, 1 << 17 | 1 << 3, 1 << 9)]
AFTER_FEW_NOTHING = [(1.2, 1 << 12, 0b11, 0), (0.5, 1 << 12 | 1, 0, 0b110), (0.9, 1 << 12, 0, 0)]

HELPER_N = 9
MCX_CASES = [((), 4), ((7,), 2), ((0, 8), 3), ((1, 3, 4, 6, 8), 0), ((8, 7, 6, 5, 4), 3)]
MCZ_CASES = [(0, 5), (1, 2, 3), (0, 1, 2, 3, 4, 5, 6, 7, 8), (8,)]
MCPHASE_CASES = [(0.37, (2, 6)), (-2.1, (0, 1, 8)), (1.0, (4,))]


def mcx_terms(controls, target):
    """What Simulator.apply_mcx applies for two or more controls."""
    c = mask_of(controls)
    return [(math.pi, c, 1 << target, 0), (-math.pi, c, 0, 0)]


def fp32_sequences(K):
    """(label, n, start state, [(theta, c, x, z)]) of every controlled sequence the GPU tests run on an fp32 state."""
    for n in EXHAUSTIVE_SIZES:
        yield f"exhaustive_n{n}", n, rand_state(n, 50 + n), exhaustive_terms(n)
    yield "every_position", 13, rand_state(13, 131), every_position_terms()
    yield "slots", SLOT_N, rand_state(SLOT_N, 10), SLOT_TERMS
    yield "several", SEVERAL_N, rand_state(SEVERAL_N, 1300), several_controls_terms()
    for c in BITEXACT_CONTROLS:
        yield f"bitexact_{c:#x}", BITEXACT_N, rand_state(BITEXACT_N, 12), bitexact_terms(c)
    yield "run", RUN_N, rand_state(RUN_N, 12), run_terms(K)
    yield "run_alternating", RUN_N, rand_state(RUN_N, 12), run_terms(K, RUN_CONTROLS)
    yield "order_ab", ORDER_N, rand_state(ORDER_N, 6), ORDER_PAIR
    yield "order_ba", ORDER_N, rand_state(ORDER_N, 6), ORDER_PAIR[::-1]
    for c in GRID_CONTROLS:
        yield f"grid_{c:#x}", GRID_N, rand_state(GRID_N, 160), grid_terms(c)
    yield "gates", GATE_N, rand_state(GATE_N, 7), GATE_TERMS
    yield "queued", 13, rand_state(13, 104), queued_terms()
    for n in FRESH_SIZES:
        zero = np.zeros(1 << n, dtype=np.complex128)
        zero[0] = 1.0
        yield f"fresh_n{n}", n, zero, [fresh_term(n)]
    yield "after_few", AFTER_FEW_N, rand_state(AFTER_FEW_N, 18), AFTER_FEW_REACH + AFTER_FEW_NOTHING  # on a dense stand-in
    for controls, target in MCX_CASES:
        if len(controls) >= 2:
            yield "mcx_" + "_".join(map(str, controls)), HELPER_N, rand_state(HELPER_N, 9), mcx_terms(controls, target)
    yield "mcphase", HELPER_N, rand_state(HELPER_N, 9), [(-2.0 * phi, mask_of(q), 0, 0) for phi, q in MCPHASE_CASES] + [(-2.0 * math.pi, mask_of(q), 0, 0) for q in MCZ_CASES]
