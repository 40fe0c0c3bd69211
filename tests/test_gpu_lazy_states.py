"""Every state call of tests/lazy_cases.py on a lazily held state over poisoned memory, against the same call on a dense twin.

A state may be PENDING (|0...0> asked for, not written) or PARTIAL (written inside its support only; the memory outside is zero by
definition and has never been written).  Every entry point that is not a tile pass must open with settle() / written(), which launches
the queued gates and writes the promised zeros; the rule is kept by hand, once per entry point.  Here each start leaves the state lazy
over memory that holds NaN (or the amplitudes of an unrelated dense run), so a call that looks at the buffer before it settles, or
that takes a second buffer for clean, cannot pass because the allocator happened to hand out zeros.

The twin is a second Simulator with the same precision and options that received the same state densely through write(), zeros spelled
out; where a case uses a spare or destination buffer the lazy side's holds NaN and the twin's zeros.  The identical call runs on both.
Checks, in this order: (1) no NaN in any returned value, in read() afterwards or in a destination buffer; (2) `bits` cases: returned
values, destination buffers and the final read() equal the twin's bit for bit — no tolerance: after settle() the two buffers are
identical and every one of these calls promises equal bits for equal calls; (3) `ref` cases, the ones that pass through the gate queue
(lazy_cases.py names the line): the feature's numpy checker with its module's tolerance — 1e-10 for fp64, fp32_ref.check_fp32 for
fp32 — because the scheduler, knowing the support, fuses other blocks; (4) a read-only call leaves the state's bits alone; (5) the
state is dense afterwards.  One process, one device, n = 15: two or three states of 512 KiB a test."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import fp32_ref
import lazy_cases as L
import pauli_rot_ref
from gpu_quantum_simulator_amd import Circuit, Diagonal, Simulator, circuits, pauli_masks, plans
from gpu_quantum_simulator_amd.pauli import control_mask

pytestmark = pytest.mark.gpu
N, FULL = L.N, L.FULL
TOL = 1e-10  # fp64, the project's parity tolerance (test_gpu_pauli_rot.TOL); fp32: fp32_ref.check_fp32
NAN = complex(float("nan"), float("nan"))
OPTIONS = dict(fuse=3, pingpong=2)  # tile passes out of place: a dense run leaves its garbage in both of a state's buffers
CASES = [case for _, case in L.all_cases()]


def _circuit(spec):
    return Circuit.from_gates(N, circuits.random_gates(*spec))


def _held(amps, precision):
    """`amps` as a state of this precision holds them."""
    amps = np.asarray(amps, dtype=np.complex128)
    return amps.astype(np.complex64).astype(np.complex128) if precision == 32 else amps


@functools.lru_cache(maxsize=None)
def _dense(start, precision):
    """The state a start stands for, zeros spelled out, as 2^n complex128 that write() stores exactly."""
    if start == "pending":
        out = np.zeros(1 << N, dtype=np.complex128)
        out[0] = 1.0
    elif start in L.SUPPORTS:
        rng = np.random.default_rng(1500 + L.STARTS.index(start))
        mask = sum(1 << b for b in L.SUPPORTS[start])
        inside = (np.arange(1 << N) & ~mask) == 0
        out = np.where(inside, rng.standard_normal(1 << N) + 1j * rng.standard_normal(1 << N), 0)
        out = _held(out / np.linalg.norm(out), precision)
    else:  # what the queued circuit leaves, read from a probe: the read writes the zeros out, so it cannot be the state under test
        assert any(g[0] == "x" for g in circuits.random_gates(*L.FEW_CIRCUIT))
        with Simulator(N, precision=precision, **OPTIONS) as probe:
            probe.run(_circuit(L.FEW_CIRCUIT))
            assert probe.get_support()[0] != FULL  # after its passes the state is partial: the start is lazy
            out = probe.read()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _truth(start, precision):
    """(fp64 truth, complex64 replay) of the state a start stands for, for the `ref` cases.  The gates of `circuit` are still queued
    when such a case adds its own, so the checker replays them from |0...0> as test_queued_gates_go_first_and_the_call_does_not_wait does."""
    if start != "circuit":
        return _dense(start, precision), _dense(start, precision).astype(np.complex64)
    c = _circuit(L.FEW_CIRCUIT)
    gl = [c.gate(i) for i in range(len(c))]
    return fp32_ref.replay(N, gl, dtype=np.complex128), fp32_ref.replay(N, gl)


def _make_lazy(sim, start, precision):
    """Leaves `sim` holding _dense(start) lazily over poisoned memory."""
    if start == "pending":
        sim.write(np.full(1 << N, NAN))
        sim.reset()
    elif start in L.SUPPORTS:
        mask = sum(1 << b for b in L.SUPPORTS[start])
        inside = (np.arange(1 << N) & ~mask) == 0
        sim.write(np.where(inside, _dense(start, precision), NAN))
        sim.set_support(mask)
    else:
        dense = _circuit(L.DENSE_CIRCUIT)
        sim.run(dense); sim.sync()  # dense garbage in the state's buffer ...
        sim.run(dense); sim.sync()  # ... and, the passes going out of place, in its second one
        sim.reset()
        sim.run(_circuit(L.FEW_CIRCUIT))  # queued, not flushed
        return  # (asking for the support would flush the queue: _dense asserts on the probe that this start is partial)
    support, pending, _ = sim.get_support()
    assert pending or support != FULL, (start, hex(support))


@functools.lru_cache(maxsize=None)
def _engine_hip():
    """The HIP runtime libqsim is linked against, by its soname: already loaded, so this opens nothing new."""
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipStreamSynchronize.restype, hip.hipStreamSynchronize.argtypes = ctypes.c_int, [ctypes.c_void_p]
    return hip


class Side:
    """One side of a test — the lazy states over poison, or their dense twins over zeros — and what it lends its case."""

    def __init__(self, precision, lazy):
        import torch
        self.torch, self.precision, self.lazy = torch, precision, lazy
        self.stack = contextlib.ExitStack()
        self.states, self.tensors, self.kept = [], {}, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.stack.close()

    def _sim(self):
        return self.stack.enter_context(Simulator(N, precision=self.precision, **OPTIONS))

    def state(self, start, own_tensor=False):
        """A state holding _dense(start): lazily over poison, or densely.  own_tensor: its amplitude buffer is a torch tensor,
        swapped in before anything is written (and out again before the state goes)."""
        sim = self._sim()
        if own_tensor:
            t = self.buffer(poison=False)
            was = sim.swap_buffer(t.data_ptr())
            self.stack.callback(sim.swap_buffer, was)
            self.tensors[id(sim)] = t
        if self.lazy:
            _make_lazy(sim, start, self.precision)
        else:
            sim.write(_dense(start, self.precision))
        self.states.append(sim)
        return sim

    def poisoned_state(self):
        """A DENSE state whose every amplitude is NaN (zero on the twin's side): a destination that is overwritten without being read."""
        sim = self._sim()
        sim.write(np.full(1 << N, NAN if self.lazy else 0.0))
        self.states.append(sim)
        return sim

    def buffer(self, amps=1 << N, poison=True):
        """A device tensor of `amps` amplitudes of this precision: NaN on the lazy side, zeros on the twin's."""
        torch = self.torch
        fill = float("nan") if self.lazy and poison else 0.0
        t = torch.full((amps, 2), fill, dtype=torch.float32 if self.precision == 32 else torch.float64, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the engine on its own
        self.kept.append(t)       # the engine holds raw pointers: the memory stays until this side is done
        return t

    def fetch(self, tensor):
        """The tensor's amplitudes in the state's own number format; call after sync() or wait()."""
        return tensor.cpu().numpy().reshape(-1).view(np.complex64 if self.precision == 32 else np.complex128)

    def wait(self, sim):
        """Waits for the state's stream WITHOUT the engine's help: qsim_sync settles the state itself and would hide a call that did not."""
        assert _engine_hip().hipStreamSynchronize(ctypes.c_void_p(sim.stream)) == 0

    def lend_spare(self, sim):
        t = self.buffer()
        sim.set_spare_buffer(t.data_ptr())
        self.stack.callback(sim.set_spare_buffer, None)
        return t

    def diagonal(self, terms):
        return self.stack.enter_context(Diagonal.from_terms(N, terms))


def _plan_path(case, precision):
    """The *path the feature's plan call reports for the case's operands at n = 15 (host only)."""
    o = case.operands
    if case.method == "apply_matrix":
        probe = plans.apply_matrix_plan(o["targets"], o["controls"], N, precision)
    elif case.method == "apply_permutation":
        probe = plans.apply_permutation_plan(o["targets"], o["controls"], N, precision)
    elif case.method == "reduced_density_matrix":
        probe = plans.reduced_density_plan(o["qubits"], N, precision)
    else:
        probe = plans.subsystem_density_plan(o["qubits"], N, precision)
    return plans.ok(probe)["path"]


def _queued_as_gates(rotations, precision):
    """How many of the (theta, string[, controls]) entries the rotation calls send through the gate queue (host only)."""
    rotations = [tuple(r) + ((),) * (3 - len(r)) for r in rotations]
    masks = [pauli_masks(text, N) for _, text, _ in rotations]
    cs = [control_mask(c, N, text) for _, text, c in rotations]
    return plans.ok(plans.controlled_rotation_plan(cs, [m[0] for m in masks], [m[1] for m in masks], N, precision, num_terms=len(rotations)))["queued_as_gates"]


def _qft_moves(case, precision):
    """Whether the plan of the case's Fourier transform has a sweep that writes the second buffer (host only)."""
    return any(plans.ok(plans.apply_qft_plan(case.operands["qubits"], N, precision, case.operands["max_digit_bits"]))["out_of_place"])


def _likely_outcome(start, precision, qubits):
    """The most probable outcome of `qubits` on the state a start stands for: non-zero probability, and bits of 0 on every qubit
    outside a sparse start's support, where a 1 never happens."""
    p = np.abs(_dense(start, precision)) ** 2
    idx = np.arange(p.size)
    outcome_of = sum(((idx >> q) & 1) << j for j, q in enumerate(qubits))
    return int(np.argmax(np.bincount(outcome_of, weights=p, minlength=1 << len(qubits))))


def _others(start, count):
    """The starts of a case's further states: each a different one."""
    at = L.STARTS.index(start)
    return [L.STARTS[(at + 1 + i) % len(L.STARTS)] for i in range(count)]


def _drive(case, side, start):
    """Runs the case's call on one side; returns (the state under test, {name: array} of everything the call handed back)."""
    o, m, out = case.operands, case.method, {}
    sim = side.state(start, own_tensor=(m == "device_ptr"))
    amp_bytes = 8 if side.precision == 32 else 16
    if m == "read":
        out["amps"] = sim.read(o["first"], o["count"])
    elif m == "norm2":
        out["norm2"] = np.array(sim.norm2())
    elif m == "expectation_terms":
        out["values"] = sim.expectation_terms(o["paulis"])
    elif m == "sample":
        out["indices"] = sim.sample(o["randoms"])
    elif m == "sample_shots":
        out["outcomes"] = sim.sample_shots(draws=o["draws"], qubits=o["qubits"])
    elif m == "block_prob_masked":
        out["sums"] = sim.block_prob_masked(o["hi_mask"], o["lo_mask"])
    elif m == "gather_masked":
        out["amps"] = sim.gather_masked(o["base"], o["lo_mask"])
    elif m in ("reduced_density_matrix", "subsystem_density_matrix"):
        out["rho"] = getattr(sim, m)(o["qubits"])
    elif m == "expectation_diagonal":
        out["moments"] = np.array(sim.expectation_diagonal(side.diagonal(o["terms"]), moments=True))
    elif m == "inner":
        other = side.state(_others(start, 1)[0])
        out["inner"] = np.array(sim.inner(other))
    elif m == "device_ptr":
        t = side.tensors[id(sim)]
        assert sim.device_ptr == t.data_ptr()  # the call under test: it launches what the buffer is owed, on the state's stream
        side.wait(sim)
        out["buffer"] = side.fetch(t)
    elif m == "write":
        rng = np.random.default_rng(o["seed"])
        sim.write(rng.standard_normal(o["count"]) + 1j * rng.standard_normal(o["count"]), first=o["first"])
    elif m == "apply_pauli_rotations":
        sim.apply_pauli_rotations(o["rotations"])
    elif m == "apply_matrix":
        sim.apply_matrix(np.array(L.matrix_entries(len(o["targets"]), o["seed"])), o["targets"], o["controls"])
    elif m == "apply_permutation":
        sim.apply_permutation(o["table"], o["targets"], o["controls"])
    elif m == "apply_diagonal_phase":
        sim.apply_diagonal_phase(side.diagonal(o["terms"]), o["gamma"])
    elif m == "apply_qft":
        sim.apply_qft(o["qubits"], max_digit_bits=o["max_digit_bits"])
    elif m == "postselect":
        out["weight"] = np.array(sim.postselect(o["qubits"], _likely_outcome(start, side.precision, o["qubits"])))
    elif m == "measure":
        outcome, probability = sim.measure(o["qubits"], draw=o["draw"], return_probability=True)
        out["outcome"], out["probability"] = np.array(outcome, dtype=np.uint64), np.array(probability)
    elif m == "scale":
        sim.scale(complex(*o["z"]))
    elif m == "ground_state":
        r = sim.ground_state(o["terms"], o["tol"], o["max_steps"], vector=o["vector"])
        out["scalars"] = np.array([r["energy"], r["residual"], r["steps"]], dtype=np.float64)
        out["alphas"], out["betas"] = r["alphas"], r["betas"]
    elif m in ("pauli_sum_into", "diagonal_into", "pack_bits"):
        dst = side.buffer()
        if m == "pauli_sum_into":
            sim.pauli_sum_into(o["terms"], dst.data_ptr())
        elif m == "diagonal_into":
            sim.diagonal_into(side.diagonal(o["terms"]), dst.data_ptr(), o["weight"], accumulate=False)
        else:
            sim.pack_bits(o["bits"], dst.data_ptr())
        sim.sync()  # (the call has looked at the state by now: settling it here hides nothing)
        out["dst"] = side.fetch(dst)
    elif m == "pack_bits_to":
        dst = side.buffer()
        blocks = 1 << len(o["bits"])
        size = amp_bytes * ((1 << N) // blocks)
        sim.pack_bits_to(o["bits"], [dst.data_ptr() + size * (blocks - 1 - b) for b in range(blocks)])  # the blocks in reverse order
        sim.sync()
        out["dst"] = side.fetch(dst)
    elif m == "copy_from":
        dst = side.poisoned_state()  # dense and poisoned; the source is the lazy one
        dst.copy_from(sim)
        out["dst"] = dst.read()
    elif m == "combine":
        p, q = (side.state(s) for s in _others(start, 2))
        out["norm2"] = np.array(sim.combine(complex(*o["d"]), (complex(*o["a"]), p), (complex(*o["b"]), q), norm=True))
    elif m == "energy_and_gradient":
        if o["lent"]:
            side.lend_spare(sim)  # lambda will live there
        diag = side.diagonal(L.DIAGONAL_TERMS) if "observable" in o else None
        rotations = [(r[0], diag) if r[1] == "diagonal" else r for r in o["rotations"]]
        terms = list(o["terms"]) + ([(o["observable"], diag)] if diag is not None else [])
        energy, grad = sim.energy_and_gradient(rotations, terms)
        out["energy"], out["grad"] = np.array(energy), grad
    else:
        raise AssertionError(f"no driver for Simulator.{m}")
    return sim, out


def _no_nan(label, arrays):
    for name, a in arrays.items():
        if a.dtype.kind in "fc":
            assert not np.isnan(a).any(), f"{label}: NaN in {name} ({int(np.isnan(a).sum())} of {a.size})"


def _same_bits(label, got, want):
    assert got.keys() == want.keys()
    for name in got:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (label, name)
        assert a.tobytes() == b.tobytes(), f"{label}: {name} differs from the dense twin's in {int(np.sum(a.view(np.uint8) != b.view(np.uint8)))} bytes"


def _check_ref(case, precision, start, got):
    before64, before32 = _truth(start, precision)
    if case.method == "apply_pauli_rotations":
        rotations = pauli_rot_ref.masks_of(case.operands["rotations"], N)
        want, ref32 = pauli_rot_ref.replay(before64, rotations), pauli_rot_ref.replay(before32, rotations, np.complex64)
    else:
        assert case.method == "scale"
        z = complex(*case.operands["z"])
        want, ref32 = z * before64, (np.complex64(z) * before32).astype(np.complex64)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"{case.name} from {start}: fp64 max abs err {worst:.3e}")
        assert worst < TOL
    else:
        fp32_ref.report(f"{case.name} from {start}", fp32_ref.check_fp32(got, want, ref32))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("start", L.STARTS)
@pytest.mark.parametrize("precision", [64, 32])
def test_lazy_state(precision, start, case):
    label = f"{case.name} from {start}, fp{precision}"
    if "plan" in case.operands:  # the operands really take the path they are in the table for
        assert _plan_path(case, precision) == case.operands["plan"], label
    if "queued" in case.operands:
        assert _queued_as_gates(case.operands["rotations"], precision) == case.operands["queued"], label
    if "moving" in case.operands:
        assert _qft_moves(case, precision) == case.operands["moving"], label
    if case.method == "energy_and_gradient":  # the forward pass of a gradient case queues nothing: it compares as bits
        assert _queued_as_gates([r for r in case.operands["rotations"] if r[1] != "diagonal"], precision) == 0, label
    with Side(precision, lazy=True) as lazy, Side(precision, lazy=False) as twin:
        sim, got = _drive(case, lazy, start)
        ref, want = _drive(case, twin, start)
        after = [s.read() for s in lazy.states]
        after_twin = [s.read() for s in twin.states]
        # 1. nothing of the poison came through
        _no_nan(label, got)
        _no_nan(label, {f"read() of state {i}": a for i, a in enumerate(after)})
        # 2. / 3.
        if case.compare == "bits":
            _same_bits(label, got, want)
            _same_bits(label, {f"read() of state {i}": a for i, a in enumerate(after)}, {f"read() of state {i}": a for i, a in enumerate(after_twin)})
        else:
            assert not got and not want  # a `ref` case changes the state and returns nothing
            _check_ref(case, precision, start, after[0])
            _check_ref(case, precision, start, after_twin[0])
        # 4. a read-only call leaves the bits alone: the state is still the one the start stands for
        if case.group == L.READ:
            assert after[0].tobytes() == _dense(start, precision).tobytes(), label
        # 5. dense once something has looked at it
        for s in lazy.states:
            assert s.get_support()[:2] == (FULL, False), label
