"""State calls in sequence, as data: programs of steps on one state, their numpy model, and the generators of the programs that
tests/test_gpu_sequences.py runs (tests/test_sequence_ref_cpu.py pins all of it on the CPU).

The engine's contract is that calls take effect in the order issued without the caller synchronising anything.  What keeps it are
things the calls SHARE: the per-state sweep scratch (operands of qsim_apply_matrix / qsim_apply_permutation / qsim_apply_qft lie where
the partial sums of every reducing sweep lie), the pinned ring of STAGING_SLOTS operand slots per device, the ring of OPS_CAP tile-op
records per state, and the state's second buffer.  A program is a list of steps (kind, operands), operands being plain data; Model
applies one to a numpy vector in complex128 (`want`) and in complex64 (`ref32`, the replay fp32_ref.check_fp32 asks for).  Nothing is
re-derived here: the model of a step is a call into the checker its feature already has (fp32_ref.replay, pauli_rot_ref,
controlled_rot_ref, matrix_ref, permutation_ref, qft_ref, diagonal_ref, measure_ref), and returned() forms the values a step hands
back from pauli_ref, density_ref, diagonal_ref, sample_ref, adjoint_ref and measure_ref.

Conditions the generators enforce (conditions, not measurements; Builder.add redraws a step's seed until they hold and counts it):
  * every matrix is unitary (helpers.random_unitary) and `scale` multiplies by |z| in [0.5, 2], so the model's norm is known;
  * a `postselect` takes the outcome the complex128 model finds most probable on k <= 3 qubits, so W >= 1/8 of the squared norm;
    a program has at most MAX_COLLAPSES collapses (postselect and measure);
  * a draw of `measure` or `sample_shots` keeps MARGIN of the total from every boundary of the model's cumulative distribution, in
    the complex128 and in the complex64 model, and both give the same outcome.  Those two kinds read the TOP qubits of the register
    (in any order): the sampler draws a basis index and returns its bits, so only there are the outcomes intervals of the running sum
    and not a comb of 2^n teeth in which no draw has a margin.
  * in the ring programs and the random walks every state-changing step moves the complex128 model by at least EFFECT (an operator
    under controls that the collapses have emptied, an identity table, a collapse onto what was collapsed before test nothing, and
    losing such a step could not be seen); those redraws are counted apart (Builder.idle);
  * the gradient a `gradient` step returns is at least GRADIENT_FLOOR sum|c_t| <psi|psi> long.
The fp32 condition, rel_err(ref32, want) <= fp32_ref.REF_CAP, is checked per program by the CPU test.

Plain numpy: nothing here loads the library or touches a device (gpu_quantum_simulator_amd.circuits is pure Python)."""
import math

import numpy as np

import adjoint_ref
import controlled_rot_ref
import density_ref
import diagonal_ref
import fp32_ref
import matrix_ref
import measure_ref
import pauli_ref
import pauli_rot_ref
import permutation_ref
import qft_ref
import sample_ref
from helpers import random_unitary

STAGING_SLOTS = 16   # kSlots of csrc/matrix.cpp: pinned operand slots per device
OPS_CAP = 512        # kOpsCap of csrc/engine.cpp: tile-op records per state
MARGIN = 1e-3
EFFECT = 1e-2        # what a state-changing step of a ring program or a random walk moves the model by, at least (Builder)
GRADIENT_FLOOR = 1e-4  # |grad| of a `gradient` step, at least, as a share of sum|c_t| <psi|psi>
MAX_COLLAPSES = 3
MAX_REDRAWN_SHARE = 0.10
MAX_ATTEMPTS = 60

IN_PLACE = ("gates", "rotations", "rotations_mixed", "rotations_controlled", "matrix_main", "matrix_small", "permutation_main",
            "permutation_small", "qft_single", "qft_moving", "diagonal_phase", "scale", "write_subrange", "postselect", "measure")
READ_ONLY = ("expectation_terms", "expectation_diagonal", "norm2", "reduced_density", "subsystem_density", "sample_shots",
             "block_prob_masked", "read_subrange")
TWO = ("gradient", "inner", "combine_into", "copy_into")
HOUSEKEEPING = ("lend_spare", "withdraw_spare", "grid_cap", "reset", "partial_write")
KINDS = IN_PLACE + READ_ONLY + TWO            # what pair_programs pairs; `write`, the start of a program, is no kind of its own
PARTNERED = ("inner", "combine_into", "copy_into")
COLLAPSES = ("postselect", "measure")
DRAWN = ("measure", "sample_shots")
STAGING = ("matrix_main", "permutation_main", "permutation_small", "qft_moving")   # the calls the ring tests interleave
# kinds that only queue gates: nothing is launched until a later call flushes the queue (qsim_scale is diag(z, z) on qubit 0, queued)
QUEUES = ("gates", "scale")
# kinds whose call makes the HOST wait for the state's stream (a value comes back, or qsim_write's copy): behind one of them the
# stream is empty, so the free-running side of a GPU test queues its next blocker there
WAITS = READ_ONLY + ("write", "write_subrange", "postselect", "measure", "gradient", "inner", "combine_into", "partial_write")

# the vocabulary of circuits.random_gates as matrices: a `gates` step hands the engine these very entries, so the model and the
# device apply the same numbers whatever a token means elsewhere
_R = math.sqrt(0.5)
GATE_MATRICES = {
    "h": np.array([[_R, _R], [_R, -_R]], dtype=np.complex128),
    "s": np.diag([1.0, 1j]), "sdg": np.diag([1.0, -1j]),
    "t": np.diag([1.0, complex(_R, _R)]), "tdg": np.diag([1.0, complex(_R, -_R)]),
    "x": np.array([[0, 1], [1, 0]], dtype=np.complex128), "z": np.diag([1.0 + 0j, -1.0]),
    "sx": 0.5 * np.array([[1 + 1j, 1 - 1j], [1 - 1j, 1 + 1j]]),
}


def gate_tuples(gates):
    """circuits.random_gates' tuples as the ("u1", q, U) / ("cx", c, t) that fp32_ref.replay takes."""
    out = []
    for g in gates:
        if g[0] == "cx":
            out.append(("cx", int(g[1]), int(g[2])))
        elif g[0] == "rz":
            out.append(("u1", int(g[2]), np.diag([np.exp(-0.5j * g[1]), np.exp(0.5j * g[1])])))
        else:
            out.append(("u1", int(g[1]), GATE_MATRICES[g[0]]))
    return out


def start_state(n, seed, precision):
    """A random unit vector as a state of this precision holds it (fp32_ref: the write rounds, the checkers start from the rounded state)."""
    s = pauli_rot_ref.rand_state(n, seed)
    return s.astype(np.complex64).astype(np.complex128) if precision == 32 else s


def _held(values, precision):
    values = np.asarray(values, dtype=np.complex128)
    return values.astype(np.complex64).astype(np.complex128) if precision == 32 else values


def _mask(qubits):
    return sum(1 << int(q) for q in qubits)


# ---- operand recipes ------------------------------------------------------------------------------------------------------------------
def _rng(kind, n, seed):
    return np.random.default_rng([(IN_PLACE + READ_ONLY + TWO + HOUSEKEEPING + ("write",)).index(kind), n, seed])


def _pick(rng, n, k):
    return [int(q) for q in rng.permutation(n)[:k]]


def _string(rng, n, weight, avoid=0, single="Z"):
    """(x, z) of a random string on `weight` qubits outside the mask `avoid`; a one-qubit string is Z (X and Y on one qubit travel
    through the gate queue, and the kinds that want that say so) unless `single` offers more letters (an observable's term)."""
    free = [q for q in range(n) if not avoid >> q & 1]
    weight = min(weight, len(free))
    x = z = 0
    for q in rng.permutation(free)[:weight]:
        letter = (single if weight == 1 else "XYZ")[rng.integers(len(single) if weight == 1 else 3)]
        x |= (letter in "XY") << int(q)
        z |= (letter in "ZY") << int(q)
    return x, z


def _angle(rng):
    return float(rng.uniform(0.3, 2.8) * (1 if rng.integers(2) else -1))


def _unitary_op(rng, n, k, controls):
    k = min(k, n)
    qs = _pick(rng, n, min(n, k + controls))
    return dict(U=random_unitary(1 << k, rng), targets=qs[:k], controls=qs[k:])


def _permutation_op(rng, n, k, controls):
    k = min(k, n)
    qs = _pick(rng, n, min(n, k + controls))
    return dict(table=[int(v) for v in rng.permutation(1 << k)], targets=qs[:k], controls=qs[k:])


def _hamiltonian(rng, n, count):
    return [(float(rng.uniform(-1, 1)),) + _string(rng, n, int(rng.integers(1, 4)), single="XYZ") for _ in range(count)]


def _diagonal_terms(rng, n, count):
    return [(float(rng.uniform(-1, 1)), _string(rng, n, int(rng.integers(1, 4)))[1] | 1 << int(rng.integers(n))) for _ in range(count)]


def _top_qubits(rng, n):
    k = int(rng.integers(1, _most_collapsed(n) + 1))
    return [int(q) for q in rng.permutation(np.arange(n - k, n))]


def _most_collapsed(n):
    """How many qubits a collapse or a draw reads at most: three, and never the whole of a register of two or more qubits (a collapse
    of the whole register leaves a basis state: nothing before it could be seen afterwards)."""
    return min(3, max(n - 1, 1))


def _partner(rng, n):
    """A partner state with sweeps of its own pending — a matrix sweep and a moving Fourier transform — and the permutation it
    receives directly after the call."""
    return dict(seed=int(rng.integers(1 << 30)), matrix=_unitary_op(rng, n, 5, 1), qft=draw_step("qft_moving", n, int(rng.integers(1 << 30))),
                after=_permutation_op(rng, n, 10, 0))


def draw_step(kind, n, seed, **options):
    """The operands of one step of `kind` on n qubits, from a seed.  `postselect` comes without its outcome and the drawn kinds are
    not yet checked against the model: Builder.add does both."""
    rng = _rng(kind, n, seed)
    if kind == "write":
        return dict(seed=int(seed))
    if kind == "gates":
        from gpu_quantum_simulator_amd import circuits
        depth = options.get("depth", 6 + int(rng.integers(5)))
        for attempt in range(1000):
            gates = circuits.random_gates(n, depth, 1000 * seed + attempt, "all")
            if any(g[0] == "x" for g in gates):
                return dict(gates=gate_tuples(gates))
        raise AssertionError("no x gate in 1000 circuits")
    if kind == "rotations":        # multi-qubit strings (a single qubit: Z): sweeps only
        count = options.get("count", 5)
        return dict(rotations=[(_angle(rng),) + _string(rng, n, int(rng.integers(2, 4))) for _ in range(count)])
    if kind == "rotations_mixed":  # X or Y on one qubit goes through the gate queue
        out = []
        for i in range(6):
            if i % 2 == 0:
                q = int(rng.integers(n))
                out.append((_angle(rng), 1 << q, (1 << q) * int(rng.integers(2))))
            else:
                out.append((_angle(rng),) + _string(rng, n, int(rng.integers(2, 4))))
        return dict(rotations=out)
    if kind == "rotations_controlled":
        out = []
        for _ in range(4):
            c = _mask(_pick(rng, n, min(int(rng.integers(1, 3)), n - 1)))
            out.append((_angle(rng), c) + _string(rng, n, int(rng.integers(1, 3)), avoid=c))
        return dict(rotations=out)
    if kind == "matrix_main":
        return _unitary_op(rng, n, 5 if n > 5 else n - 1 if n > 1 else 1, 1)
    if kind == "matrix_small":     # two targets under so many controls that the matrix path has too few environments
        return _unitary_op(rng, n, 2, max(n - 5, 0))
    if kind == "permutation_main":
        return _permutation_op(rng, n, 10, 0)
    if kind == "permutation_small":
        return _permutation_op(rng, n, 3, 4)
    if kind == "qft_single":
        return dict(qubits=_pick(rng, n, min(10, n)), inverse=bool(rng.integers(2)), max_digit_bits=0)
    if kind == "qft_moving":       # n = 14: twelve qubits in digits of at most four bits, three sweeps, two of them out of place
        k = min(12, n)
        return dict(qubits=_pick(rng, n, k), inverse=bool(rng.integers(2)), max_digit_bits=4 if k > 8 else 1)
    if kind == "diagonal_phase":
        return dict(terms=_diagonal_terms(rng, n, 6), gamma=_angle(rng))
    if kind == "scale":
        r, phi = math.exp(rng.uniform(math.log(0.5), math.log(2.0))), rng.uniform(0, 2 * math.pi)
        return dict(z=(r * math.cos(phi), r * math.sin(phi)))
    if kind == "write_subrange":
        count = int(rng.integers(1, max((1 << n) // 3, 1) + 1))
        return dict(first=int(rng.integers(0, (1 << n) - count + 1)), count=count, seed=int(seed))
    if kind == "postselect":
        return dict(qubits=_pick(rng, n, int(rng.integers(1, _most_collapsed(n) + 1))), outcome=None)
    if kind == "measure":
        return dict(qubits=_top_qubits(rng, n), draw=float(rng.uniform(0.0, 1.0)))
    if kind == "expectation_terms":  # more than one batch of result rows at n >= 8: 130 distinct x masks, as test_gpu_sweep_scratch.STRINGS
        return dict(masks=[(x % (1 << n), int(rng.integers(0, 1 << n))) for x in range(1, 131)])
    if kind == "expectation_diagonal":
        return dict(terms=_diagonal_terms(rng, n, 6))
    if kind in ("norm2", "lend_spare", "withdraw_spare", "reset"):
        return dict()
    if kind == "reduced_density":
        return dict(qubits=_pick(rng, n, min(5, n)))
    if kind == "subsystem_density":
        return dict(qubits=_pick(rng, n, min(7, n)))
    if kind == "sample_shots":
        return dict(qubits=_top_qubits(rng, n), draws=[float(u) for u in rng.uniform(0.0, 1.0, size=6)])
    if kind == "block_prob_masked":
        hi = _mask(_pick(rng, n, min(4, n)))
        return dict(hi_mask=hi, lo_mask=((1 << n) - 1) & ~hi)
    if kind == "read_subrange":
        count = int(rng.integers(1, (1 << n) + 1))
        return dict(first=int(rng.integers(0, (1 << n) - count + 1)), count=count)
    if kind == "gradient":
        return dict(rotations=[(_angle(rng),) + _string(rng, n, int(rng.integers(2, 4))) for _ in range(5)], terms=_hamiltonian(rng, n, 6))
    if kind == "inner":
        return dict(partner=_partner(rng, n))
    if kind == "combine_into":      # self <- d self + a partner with |d|^2 + |a|^2 = 1
        phi, alpha, beta = rng.uniform(0.3, 1.2), rng.uniform(0, 2 * math.pi), rng.uniform(0, 2 * math.pi)
        return dict(partner=_partner(rng, n), d=(math.cos(phi) * math.cos(alpha), math.cos(phi) * math.sin(alpha)),
                    a=(math.sin(phi) * math.cos(beta), math.sin(phi) * math.sin(beta)))
    if kind == "copy_into":         # the partner <- this state
        return dict(partner=_partner(rng, n))
    if kind == "grid_cap":
        return dict(value=int((0, 1, 2, 7)[rng.integers(4)]))
    if kind == "partial_write":     # amplitudes inside a support only; the memory outside it is poisoned, then set_support
        k = max(n - int(rng.integers(1, 4)), 0)
        return dict(support=_mask(_pick(rng, n, k)), seed=int(seed))
    raise ValueError(f"no kind {kind!r}")


def subrange_values(op, n, precision):
    """The amplitudes a write_subrange step writes, of the size a unit vector's are, as the state holds them."""
    rng = np.random.default_rng([77, op["seed"]])
    v = (rng.standard_normal(op["count"]) + 1j * rng.standard_normal(op["count"])) / math.sqrt(2.0 * (1 << n))
    return _held(v, precision)


def partial_values(op, n, precision):
    """(the state a partial_write step stands for, zeros spelled out; which indices lie inside its support)"""
    rng = np.random.default_rng([78, op["seed"]])
    inside = (np.arange(1 << n) & ~op["support"]) == 0
    v = np.where(inside, rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n), 0)
    return _held(v / np.linalg.norm(v), precision), inside


# ---- the draws: where the running sum changes outcome ---------------------------------------------------------------------------------
def draw_outcome(psi, qubits, u):
    """(outcome, margin): the outcome of `qubits` that the draw u in [0, 1] reads on psi — the bits of the first index whose running
    sum reaches u * total — and the draw's distance, as a share of the total, from the nearest place where the running sum passes
    from one outcome to another (0 and 1, the ends, included)."""
    n = int(np.asarray(psi).size).bit_length() - 1
    p, want, _, _, E, r, _ = sample_ref.classify(n, psi, [u])
    total = E[-1]
    outcomes = sample_ref.outcome_bits(np.arange(p.size), qubits)
    change = np.flatnonzero(outcomes[1:] != outcomes[:-1])       # between index j and j + 1 the outcome changes: boundary E[j]
    edges = np.concatenate(([np.longdouble(0)], E[change], [total]))
    return int(outcomes[int(want[0])]), float(np.min(np.abs(edges - r[0])) / total)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def partner_states(op, n, precision):
    """(complex128, complex64) of the partner of a two-state step when the call reads it: its start with the pending sweeps applied."""
    p, start = op["partner"], start_state(n, op["partner"]["seed"], precision)
    out = []
    for dtype in (np.complex128, np.complex64):
        s = matrix_ref.apply_matrix(start.astype(dtype), p["matrix"]["U"], p["matrix"]["targets"], p["matrix"]["controls"], dtype=dtype)
        out.append(qft_ref.apply_qft(s, p["qft"]["qubits"], p["qft"]["inverse"], dtype=dtype))
    return out


def _apply(kind, op, psi, dtype, n, precision):
    """One in-place step on one vector in `dtype`: a call into the feature's own checker."""
    if kind == "gates":
        return fp32_ref.replay(n, op["gates"], start=psi, dtype=dtype)
    if kind in ("rotations", "rotations_mixed"):
        return pauli_rot_ref.replay(psi, op["rotations"], dtype)
    if kind == "rotations_controlled":
        return controlled_rot_ref.replay(psi, op["rotations"], dtype)
    if kind in ("matrix_main", "matrix_small"):
        return matrix_ref.apply_matrix(psi, op["U"], op["targets"], op["controls"], dtype=dtype)
    if kind in ("permutation_main", "permutation_small"):
        return permutation_ref.apply_permutation(psi, op["table"], op["targets"], op["controls"])
    if kind in ("qft_single", "qft_moving"):
        return qft_ref.apply_qft(psi, op["qubits"], op["inverse"], dtype=dtype)
    if kind == "diagonal_phase":
        return diagonal_ref.apply_phase(psi, diagonal_ref.table_from_terms(n, op["terms"]), op["gamma"], dtype)
    if kind == "scale":
        return (dtype(complex(*op["z"])) * psi).astype(dtype)
    if kind == "write_subrange":
        out = np.array(psi, dtype=dtype, copy=True)
        out[op["first"]:op["first"] + op["count"]] = subrange_values(op, n, precision).astype(dtype)
        return out
    if kind in ("postselect", "measure"):
        return measure_ref.postselect(psi, op["qubits"], op["outcome"], dtype)[1]
    if kind == "gradient":  # the forward pass and the backward pass: the state is left as the call found it, to rounding
        back = [(-theta, x, z) for theta, x, z in reversed(op["rotations"])]
        return pauli_rot_ref.replay(pauli_rot_ref.replay(psi, op["rotations"], dtype), back, dtype)
    if kind == "combine_into":
        p64, p32 = partner_states(op, n, precision)
        partner = p64 if dtype == np.complex128 else p32
        return (dtype(complex(*op["d"])) * psi + dtype(complex(*op["a"])) * partner).astype(dtype)
    if kind == "reset":
        out = np.zeros(1 << n, dtype=dtype)
        out[0] = 1
        return out
    if kind == "partial_write":
        return partial_values(op, n, precision)[0].astype(dtype)
    if kind == "write":
        return start_state(n, op["seed"], precision).astype(dtype)
    assert kind in READ_ONLY + ("inner", "copy_into", "lend_spare", "withdraw_spare", "grid_cap"), kind
    return psi


class Model:
    """A program's state in complex128 (`want`) and in complex64 (`ref32`), step by step."""

    def __init__(self, n, precision):
        self.n, self.precision = n, precision
        self.want = _apply("reset", {}, None, np.complex128, n, precision)
        self.ref32 = _apply("reset", {}, None, np.complex64, n, precision)
        self.partners = []  # per partnered step, in order: (complex128, complex64) of the partner's final state

    def outcome_of(self, op, u):
        """(outcome of the draw in the complex128 model, the smaller of its margins in the two models, whether the models agree)"""
        o64, m64 = draw_outcome(self.want, op["qubits"], u)
        o32, m32 = draw_outcome(self.ref32, op["qubits"], u)
        return o64, min(m64, m32), o64 == o32

    def apply(self, step):
        kind, op = step
        if kind == "measure" and op.get("outcome") is None:
            op["outcome"] = self.outcome_of(op, op["draw"])[0]
        if kind in PARTNERED:
            p64, p32 = partner_states(op, self.n, self.precision)
            if kind == "copy_into":
                p64, p32 = self.want.copy(), self.ref32.copy()
            after = op["partner"]["after"]
            self.partners.append(tuple(permutation_ref.apply_permutation(p, after["table"], after["targets"], after["controls"]) for p in (p64, p32)))
        self.want = np.asarray(_apply(kind, op, self.want, np.complex128, self.n, self.precision), dtype=np.complex128)
        self.ref32 = np.asarray(_apply(kind, op, self.ref32, np.complex64, self.n, self.precision), dtype=np.complex64)

    def run(self, program):
        for step in program:
            self.apply(step)
        return self


def run_model(n, precision, program):
    return Model(n, precision).run(program)


# ---- what a step returns, from the amplitudes the state holds before it ---------------------------------------------------------------
def returned(step, psi, partner=None):
    """{name: value} of the values a step hands back, in float64 from `psi` (the amplitudes before the step; `partner`: those of the
    partner when the call reads it), by the checker of the step's feature."""
    kind, op = step
    psi = np.asarray(psi, dtype=np.complex128)
    n = int(psi.size).bit_length() - 1
    if kind == "expectation_terms":
        return {"values": np.array([pauli_ref.pauli_expectation(psi, x, z) for x, z in op["masks"]])}
    if kind == "expectation_diagonal":
        return {"moments": np.array(diagonal_ref.moments(psi, diagonal_ref.table_from_terms(n, op["terms"])))}
    if kind == "norm2":
        return {"norm2": np.array(float(np.vdot(psi, psi).real))}
    if kind in ("reduced_density", "subsystem_density"):
        return {"rho": density_ref.reduced_density(psi, op["qubits"])}
    if kind == "sample_shots":
        return {"outcomes": np.array([draw_outcome(psi, op["qubits"], u)[0] for u in op["draws"]], dtype=np.uint64)}
    if kind == "block_prob_masked":
        hi = [q for q in range(n) if op["hi_mask"] >> q & 1]
        return {"sums": density_ref.marginal(psi, hi)}
    if kind == "read_subrange":
        return {"amps": psi[op["first"]:op["first"] + op["count"]].copy()}
    if kind == "gradient":
        energy, grad, _ = adjoint_ref.gradient(psi, op["rotations"], op["terms"])
        return {"energy": np.array(energy), "grad": grad}
    if kind == "inner":
        return {"inner": np.array(np.vdot(psi, partner))}
    if kind == "combine_into":
        out = complex(*op["d"]) * psi + complex(*op["a"]) * np.asarray(partner, dtype=np.complex128)
        return {"norm2": np.array(float(np.vdot(out, out).real))}
    if kind == "postselect":
        return {"weight": np.array(measure_ref.weight(psi, op["qubits"], op["outcome"]))}
    if kind == "measure":
        return {"outcome": np.array(op["outcome"], dtype=np.uint64),
                "probability": np.array(measure_ref.weight(psi, op["qubits"], op["outcome"]) / float(np.vdot(psi, psi).real))}
    return {}


# ---- the generators -------------------------------------------------------------------------------------------------------------------
class NoSeed(AssertionError):
    """No operands of a kind meet the conditions on the state as it is (a walk then takes another kind)."""


class Builder:
    """A program under construction with its model beside it: add() draws a step, binds what the model decides (the outcome a
    postselect takes) and redraws the step's seed until the module's conditions hold."""

    def __init__(self, n, precision, effect=False):
        """effect: every step that changes the state moves the complex128 model by at least EFFECT relative, or is drawn again (an
        operator under controls that the state no longer populates, a collapse onto what was collapsed before, an identity table:
        such a step tests nothing, and losing it could not be seen).  Those draws are counted apart, in `idle`."""
        self.n, self.precision, self.effect = n, precision, effect
        self.model = Model(n, precision)
        self.program, self.drawn, self.redrawn, self.idle, self.collapses = [], 0, 0, 0, 0

    def _holds(self, kind, op):
        m = self.model
        if kind == "postselect":
            p = density_ref.marginal(m.want, op["qubits"])
            op["outcome"] = int(np.argmax(p))
            return bool(p[op["outcome"]] >= float(np.sum(p)) / 8.0)
        if kind == "gradient":  # a gradient that vanishes (observable and rotations commute) has no relative error to hold the fp32 one to
            _, grad, _ = adjoint_ref.gradient(m.want, op["rotations"], op["terms"])
            return bool(np.linalg.norm(grad) >= GRADIENT_FLOOR * adjoint_ref.weight(op["terms"]) * float(np.vdot(m.want, m.want).real))
        if kind in DRAWN:
            for u in (op["draws"] if kind == "sample_shots" else [op["draw"]]):
                _, margin, agree = m.outcome_of(op, u)
                if margin < MARGIN or not agree:
                    return False
        return True

    def _moves(self, kind, op):
        if not self.effect or kind not in IN_PLACE + ("combine_into",):
            return True
        if kind == "measure":
            op = dict(op, outcome=self.model.outcome_of(op, op["draw"])[0])
        after = _apply(kind, op, self.model.want, np.complex128, self.n, self.precision)
        return fp32_ref.rel_err(after, self.model.want) >= EFFECT

    def add(self, kind, seed, **options):
        if kind in COLLAPSES:
            assert self.collapses < MAX_COLLAPSES, "a program has at most three collapses"
        failed = idle = False
        for attempt in range(MAX_ATTEMPTS):
            op = draw_step(kind, self.n, seed + 104729 * attempt, **options)
            if not self._holds(kind, op):
                failed = True
            elif not self._moves(kind, op):
                idle = True
            else:
                break
        else:
            raise NoSeed(f"{kind}: no seed in {MAX_ATTEMPTS} meets the conditions")
        self.drawn += 1
        self.collapses += kind in COLLAPSES
        self.redrawn += failed
        self.idle += idle and not failed
        self.program.append((kind, op))
        self.model.apply(self.program[-1])
        return self


def pair_programs(n, precision, first=None):
    """[(A, B, program, builder)] for every ordered pair of KINDS (or those with A == first): [write(start), gates, A, B, gates]."""
    out = []
    for ia, a in enumerate(KINDS):
        if first is not None and a != first:
            continue
        for ib, b in enumerate(KINDS):
            seed = 1000 * (ia + 1) + 10 * ib
            bld = Builder(n, precision)
            bld.add("write", seed).add("gates", seed + 1).add(a, seed + 2).add(b, seed + 3).add("gates", seed + 4)
            out.append((a, b, bld.program, bld))
    return out


RING_CALLS = 3 * STAGING_SLOTS + 5


def _staging_run(bld, count, seed):
    """`count` operand-staging calls, the four STAGING kinds in turn, every operand drawn anew (another unitary, table, register)."""
    for i in range(count):
        bld.add(STAGING[i % len(STAGING)], seed + i)
    return bld


def ring_programs(n, precision):
    """{name: (program, builder)} of the ring tests.
    one:            write, then RING_CALLS staging calls, for one state behind one blocker.
    two_a, two_b:   for two states that take turns: 2 * STAGING_SLOTS calls each — the first 20 of each before the third state comes
                    and goes, the other 12 (another lap of the ring between them) after.
    third:          three staging calls for the state that is created and closed in the middle.
    tile_ops_0 ...: TILE_OP_PROGRAMS programs for ONE state, run one after the other (the engine's count of used records goes on from
                    program to program): write, then TILE_OP_ROUNDS times (a `gates` step of 8 gates, one Z rotation that flushes it).
                    A flush of so few gates is a pass of one to three blocks, so it takes some 900 of them to go through OPS_CAP records
                    twice; in one program the complex64 model of as many gates would pass fp32_ref.REF_CAP."""
    out = {}  # (the three long ones close with a `gates` step: a call that cannot wait for a slot is the last one issued)
    out["one"] = _staging_run(Builder(n, precision, effect=True).add("write", 501), RING_CALLS, 5100).add("gates", 5290)
    out["two_a"] = _staging_run(Builder(n, precision, effect=True).add("write", 502), 2 * STAGING_SLOTS, 5300).add("gates", 5490)
    out["two_b"] = _staging_run(Builder(n, precision, effect=True).add("write", 503), 2 * STAGING_SLOTS, 5500).add("gates", 5690)
    out["third"] = _staging_run(Builder(n, precision, effect=True).add("write", 504), 3, 5700)
    for k in range(TILE_OP_PROGRAMS):
        bld = Builder(n, precision).add("write", 505 + k)
        for i in range(TILE_OP_ROUNDS):
            bld.add("gates", 10000 * (k + 1) + i, depth=8).add("rotations", 10000 * (k + 1) + 5000 + i, count=1)
        out[f"tile_ops_{k}"] = bld.add("gates", 10000 * (k + 1) + 9999)
    return {name: (b.program, b) for name, b in out.items()}


TENANTS = ("own", "lent", "toggled")


def tenant_program(n, precision, lent):
    """(program, builder) of the second-buffer test: gradient (lambda in the second buffer), a moving Fourier transform (its other
    side), gates (flushed out of place by the next call), gradient, the transform again, gates.  lent: "own" — the state's own second
    buffer throughout; "lent" — a spare buffer lent before the first call; "toggled" — lent and withdrawn between the calls."""
    assert lent in TENANTS
    bld = Builder(n, precision).add("write", 601)
    calls = ("gradient", "qft_moving", "gates", "gradient", "qft_moving", "gates")
    if lent == "lent":
        bld.add("lend_spare", 0)
    for i, kind in enumerate(calls):
        if lent == "toggled":
            bld.add("lend_spare" if i % 2 == 0 else "withdraw_spare", 0)
        bld.add(kind, 6200 + 10 * TENANTS.index(lent) + i)
    return bld.program, bld


def partner_program(n, precision):
    """(program, builder): inner, combine_into and copy_into, each with a partner that has sweeps pending and receives a permutation
    directly afterwards, then gates on the state itself."""
    bld = Builder(n, precision).add("write", 602)
    for i, kind in enumerate(PARTNERED):
        bld.add(kind, 6300 + i)
    return bld.add("gates", 6310).program, bld


TWO_STATES_FIRST_HALF = 20
TILE_OP_PROGRAMS, TILE_OP_ROUNDS = 4, 220
DEFINERS = ("write", "reset", "partial_write")  # steps after which nothing of the state's past is left
EARLY = 12                                      # a random walk redefines its state only within its first EARLY steps


def random_program(n, length, seed, precision):
    """(program, builder): write(start), then `length` steps: length - 1 drawn from every kind, housekeeping included, and a closing
    `gates` step, so that the last call of a walk never waits for the device.  At most MAX_COLLAPSES collapses; a spare is withdrawn
    where one was lent and lent where none is; one `measure` at most; `reset` and `partial_write` (and, on one qubit, a collapse or
    a write of one amplitude: they leave little else) come only among the first EARLY steps, so that at least four fifths of a walk
    of 60 steps can still be seen in its final state.  Every state-changing step moves the model (Builder's `effect`)."""
    rng = np.random.default_rng([99, n, length, seed])
    kinds = IN_PLACE + READ_ONLY + TWO + HOUSEKEEPING
    weights = np.array([3.0] * len(IN_PLACE) + [1.0] * len(READ_ONLY) + [1.5] * len(TWO) + [1.0] * len(HOUSEKEEPING))
    bld = Builder(n, precision, effect=True).add("write", 7000 + seed)
    lent = measured = False
    while len(bld.program) < length:
        kind = kinds[int(rng.choice(len(kinds), p=weights / weights.sum()))]
        if kind in COLLAPSES and bld.collapses >= MAX_COLLAPSES:
            continue
        if kind in ("lend_spare", "withdraw_spare"):  # either draw toggles: a spare is lent where none is, withdrawn where one is
            kind = "withdraw_spare" if lent else "lend_spare"
        if (kind in DEFINERS or (n == 1 and kind in COLLAPSES + ("write_subrange",))) and len(bld.program) > EARLY:
            continue
        if kind == "measure" and measured:  # (its qubits are the top ones: a second one reads what the first has left and changes nothing)
            continue
        try:
            bld.add(kind, int(rng.integers(1 << 30)))
        except NoSeed:  # e.g. a small matrix under nine controls once the collapses have emptied most control subspaces
            continue
        lent = kind == "lend_spare" or (lent and kind != "withdraw_spare")
        measured = measured or kind == "measure"
    return bld.add("gates", 7100 + seed).program, bld
