"""State calls in sequence, the host never waiting in between: every ordered pair of calls, the operand ring going round, two states
on one ring, the tile-op ring wrapping, the tenants of the second buffer, partners with sweeps pending, random walks.

Every feature file tests its call alone.  What the calls SHARE — the sweep scratch (operands of matrix, permutation and Fourier sweeps
lie where the partial sums of every reducing sweep lie), the pinned ring of 16 operand slots per device, the ring of 512 tile-op
records, the second buffer — is kept right by stream order and by the host's bookkeeping, and is under load only when the host runs
ahead of the device.  At n = 14 a sweep is over before the next call is issued, so the free-running side of every test first queues a
BLOCKER on the state's own stream (a chain of torch matmuls on torch.cuda.ExternalStream(sim.stream), with a torch event behind it)
and queues the next one whenever a call has made the host wait (sequence_ref.WAITS: a value came back).  Each test asserts that the
event behind the last blocker had NOT completed when the last call under test returned, and that NO call found its blocker ended when
it returned ("the stream was not backed up" otherwise) except those that wait by contract: the kinds of sequence_ref.WAITS, MAY_WAIT
below, a staging call that comes when more than a ring of uploads has been made behind the running blocker, and in the tile-op test
the flush that finds the record ring full.  A blocker ends by itself; nothing waits on the host for it but those calls and sync().

Two checks for every program (tests/sequence_ref.py has the programs and their numpy model; tests/test_sequence_ref_cpu.py pins both):
  * the stepped twin, bit for bit: the same program on a second Simulator with the same options and no blocker, with sync() and a
    device-wide wait after every step that does more than queue gates.  (sequence_ref.QUEUES: `gates`, and `scale`, which is a queued
    diag(z, z): a sync() there would flush early and the passes would be grouped differently.  After a housekeeping step the
    device-wide wait alone: sync() would write a lazily held state out, and again the next flush would group its passes differently.)
    The final read(), every returned value and every partner state equal the free-running side's in every byte: each call promises
    equal bits for equal calls, so no tolerance.
  * the model: fp64 max|got - want| <= 1e-10 max(1, |want|_2) — 1e-10 is the project's parity tolerance (test_gpu_pauli_rot.TOL,
    test_gpu_lazy_states.TOL); the operands are unitary and a program has at most three collapses with W >= 1/8, so a program amplifies
    an error by at most sqrt(8)^3; an ordering or stale-operand mistake shows at 1e-2 (the CPU test shows that it does).  fp32:
    fp32_ref.check_fp32(got, want, ref32) with ref32 the complex64 model, both from the start state as fp32 holds it.
Returned values are checked on the stepped side (whose bits the free-running side's equal) at the step that returns them, against the
feature's checker on the amplitudes read back before the step and with the feature file's own bound, restated in _check_values with
the line it comes from.  Those bounds are stated for unit vectors and are applied as they stand, although `scale` and `combine_into`
take the squared norm up to 4 here.  To read those amplitudes the twin calls read() in front of every value-returning step, which
launches the queued gates and writes a lazily held state out before the call under test: on the twin such a call never flushes the
queue itself and never starts from a lazy state.  The free-running side does both, and is held to the twin bit for bit.

Host issue time and blocker lengths.  Measured on one MI355X: the host time the stepped twin spends in the calls of a program that
do not wait for the device (those of sequence_ref.WAITS drain the stream anyway, and the next blocker goes in behind them), for the
longest program of each family; every test prints both figures again.  Host times on a shared machine jitter by small integer
factors, so a blocker is at least ten times that, and never below 20 ms:
  every ordered pair      0.72 ms (median 0.1 ms; one program in 1458 took 9.1 ms, a first-use allocation)    ->  20 ms
  operand ring, 53 calls  1.75 ms  ->  20 ms          two states on one ring   1.31 ms  ->  20 ms
  tile-op ring            14.90 ms (442 steps, 8 gates each)  ->  150 ms
  second buffer           0.23 ms  ->  20 ms          partners                 0.30 ms  ->  20 ms
  walks of 60 calls       2.84 ms  ->  60 ms          the same on 1 to 3 qubits  2.35 ms  ->  45 ms
(the walks' blockers are ten times 5.96 and 4.37 ms, measured while a walk still created its Diagonals and wrote its partners between
its calls; both are made in front of the first call now).
A blocker is a chain of 2048 x 2048 fp32 matmuls, 0.12 ms each, counted out from a timing at the start of the session.
"""
import contextlib
import math
import time

import numpy as np
import pytest

import adjoint_ref
import controlled_rot_ref
import diagonal_ref
import fp32_ref
import measure_ref
import pauli_ref
import pauli_rot_ref
import sequence_ref as S
from gpu_quantum_simulator_amd import Diagonal, Simulator, _lib, plans

pytestmark = pytest.mark.gpu
N = 14
TOL = 1e-10
PRECISIONS = [64, 32]
# Tile passes out of place: a flush, a gradient and a moving transform all want the second buffer.  No plan cache: once eight plans
# are held, a flush of a circuit not seen before evicts one and waits for the state's stream first (engine.cpp keep_plan), so on a
# Simulator that runs many programs the call behind a `gates` step would wait its blocker out and run on an empty stream.  No program
# here repeats a circuit, so nothing would be replayed from the cache either.
OPTIONS = dict(fuse=3, pingpong=2, plan_cache=0)
# Calls outside sequence_ref.WAITS that may still wait for the state's stream, with the line that says so; any other call that finds
# its blocker ended fails its test (the ring tests expect a staging call to wait for a slot, and assert that it does).
MAY_WAIT = ("lend_spare",)  # pack.cpp qsim_set_spare_buffer: a state that owns a spare waits for its stream and frees it
NAN = complex(float("nan"), float("nan"))
WALK_SEEDS = list(range(8))
SMALL_SEEDS = list(range(4))
# Host milliseconds in the non-waiting calls of each family's longest program, as measured (docstring), and the blockers' lengths
MEASURED_ISSUE_MS = {"pair": 0.72, "ring": 1.75, "two": 1.31, "tile_ops": 14.90, "tenants": 0.23, "partners": 0.30, "walk": 2.84, "small": 2.35}
BLOCKER_MS = {"pair": 20.0, "ring": 20.0, "two": 20.0, "tile_ops": 150.0, "tenants": 20.0, "partners": 20.0, "walk": 60.0, "small": 45.0}
assert all(BLOCKER_MS[family] >= max(10.0 * ms, 20.0) for family, ms in MEASURED_ISSUE_MS.items())
THIRD_STATE_MS = 300.0  # the blockers that keep two states backed up while a third one is created, used and closed
UPLOADS = ("matrix_main", "matrix_small", "permutation_main", "permutation_small", "qft_single", "qft_moving") + S.PARTNERED  # stage operands
VALUE_KINDS = S.READ_ONLY + ("gradient", "inner", "combine_into", "postselect", "measure")


# ---- the blocker ----------------------------------------------------------------------------------------------------------------------
class _Blockers:
    """Finite device work of a chosen length on any stream: a chain of 2048 x 2048 fp32 matmuls, timed once per session."""
    SIZE = 2048

    def __init__(self):
        import torch
        self.torch = torch
        self.a = torch.full((self.SIZE, self.SIZE), 1.0 / self.SIZE, dtype=torch.float32, device="cuda")
        self.b = torch.full((self.SIZE, self.SIZE), 1.0, dtype=torch.float32, device="cuda")
        self.out = {}
        c = torch.empty_like(self.a)
        for _ in range(5):
            torch.mm(self.a, self.b, out=c)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(40):
            torch.mm(self.a, self.b, out=c)
        t1.record()
        t1.synchronize()
        self.ms_per_matmul = max(t0.elapsed_time(t1) / 40.0, 1e-3)
        print(f"blocker: one {self.SIZE}^2 fp32 matmul takes {self.ms_per_matmul:.3f} ms")

    def arm(self, stream, ms):
        """Queues about `ms` milliseconds of matmuls on the stream with this handle; returns the torch event recorded behind them."""
        torch = self.torch
        ext = torch.cuda.ExternalStream(stream)
        if stream not in self.out:
            self.out[stream] = torch.empty_like(self.a)
        with torch.cuda.stream(ext):
            for _ in range(max(1, math.ceil(ms / self.ms_per_matmul))):
                torch.mm(self.a, self.b, out=self.out[stream])
        event = torch.cuda.Event()
        event.record(ext)
        return event


_blockers = None


def blockers():
    global _blockers
    if _blockers is None:
        _blockers = _Blockers()
    return _blockers


# ---- one side of a test -----------------------------------------------------------------------------------------------------------------
class Run:
    """What one side handed back for one program."""

    def __init__(self):
        self.values, self.before, self.partner_before, self.after = {}, {}, {}, {}
        self.final, self.partners = None, []
        self.issue_ms, self.free_ms, self.ahead, self.stalls, self.backed_up, self.partner_backed_up = 0.0, 0.0, 0, [], None, []
        self.slot_waits = []  # calls that waited for a slot of the operand ring with the ring full behind the running blocker


class Side:
    """A Simulator that runs programs: free-running behind blockers (free=True), or stepped (the twin)."""

    def __init__(self, n, precision, free, blocker_ms=0.0, partner_blockers=False, profile=False, options=OPTIONS, drain=True):
        """blocker_ms = 0 on a free side: no blocker, and no wait between the calls either.  drain=False: the side goes away without
        a device-wide wait first (qsim_destroy waits for its own streams)."""
        import torch
        self.drain = drain
        self.torch, self.n, self.precision, self.free, self.blocker_ms, self.partner_blockers = torch, n, precision, free, blocker_ms, partner_blockers
        self.stack = contextlib.ExitStack()
        self.sim = self.stack.enter_context(Simulator(n, precision=precision, profile=profile, **options))
        self.options, self.pool, self.kept, self.event = options, [], [], None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.drain:
            self.torch.cuda.synchronize()
        self.stack.close()

    # -- resources a program needs, made before its first call so that no allocation waits for the device in the middle of it
    def _prepare(self, program):
        need = sum(kind in S.PARTNERED for kind, _ in program)
        while len(self.pool) < need:
            self.pool.append(self.stack.enter_context(Simulator(self.n, precision=self.precision, **self.options)))
        partnered = [op for kind, op in program if kind in S.PARTNERED]
        for p, op in zip(self.pool, partnered):  # (qsim_write waits for the partner's stream and copies synchronously)
            p.write(S.start_state(self.n, op["partner"]["seed"], self.precision))
        self.diagonals = {id(op): self.stack.enter_context(Diagonal.from_terms(self.n, diagonal_ref.texts(op["terms"], self.n)))
                          for kind, op in program if kind in ("diagonal_phase", "expectation_diagonal")}
        self.spares = []
        for kind, _ in program:
            if kind == "lend_spare":  # full of NaN: a tenant that took the second buffer for clean cannot pass
                real = self.torch.float32 if self.precision == 32 else self.torch.float64
                self.spares.append(self.torch.full((1 << self.n, 2), float("nan"), dtype=real, device="cuda"))
        self.kept.extend(self.spares)  # the engine holds raw pointers: the memory stays until this side is done
        if self.spares or self.diagonals:
            self.torch.cuda.synchronize()
        self.used = 0

    # -- the calls
    def _partnered(self, kind, op, run, i):
        sim, p, po = self.sim, self.pool[self.used], op["partner"]
        self.used += 1
        event = blockers().arm(p.stream, self.blocker_ms) if self.free and self.partner_blockers else None
        p.apply_matrix(po["matrix"]["U"], po["matrix"]["targets"], po["matrix"]["controls"])  # the partner's own sweeps, pending
        p.apply_qft(po["qft"]["qubits"], po["qft"]["inverse"], max_digit_bits=po["qft"]["max_digit_bits"])
        if event is not None:
            run.partner_backed_up.append(not event.query())
        if not self.free:
            run.partner_before[i] = p.read()
        out = {}
        if kind == "inner":
            out["inner"] = np.array(sim.inner(p))
        elif kind == "combine_into":
            out["norm2"] = np.array(sim.combine(complex(*op["d"]), (complex(*op["a"]), p), norm=True))
        else:
            p.copy_from(sim)
        p.apply_permutation(po["after"]["table"], po["after"]["targets"], po["after"]["controls"])  # directly afterwards: it must not overtake
        return out

    def _issue(self, step, run, i):
        (kind, op), sim, n = step, self.sim, self.n
        if kind == "write":
            sim.write(S.start_state(n, op["seed"], self.precision))
        elif kind == "gates":
            for g in op["gates"]:
                sim.apply_cx(g[1], g[2]) if g[0] == "cx" else sim.apply_1q(g[2], g[1])
        elif kind in ("rotations", "rotations_mixed"):
            sim.apply_pauli_rotations(pauli_rot_ref.texts(op["rotations"], n))
        elif kind == "rotations_controlled":
            sim.apply_pauli_rotations(controlled_rot_ref.entries(op["rotations"], n))
        elif kind in ("matrix_main", "matrix_small"):
            sim.apply_matrix(op["U"], op["targets"], op["controls"])
        elif kind in ("permutation_main", "permutation_small"):
            sim.apply_permutation(op["table"], op["targets"], op["controls"])
        elif kind in ("qft_single", "qft_moving"):
            sim.apply_qft(op["qubits"], op["inverse"], max_digit_bits=op["max_digit_bits"])
        elif kind == "diagonal_phase":
            sim.apply_diagonal_phase(self.diagonals[id(op)], op["gamma"])
        elif kind == "scale":
            sim.scale(complex(*op["z"]))
        elif kind == "write_subrange":
            sim.write(S.subrange_values(op, n, self.precision), first=op["first"])
        elif kind == "postselect":
            return {"weight": np.array(sim.postselect(op["qubits"], op["outcome"]))}
        elif kind == "measure":
            outcome, p = sim.measure(op["qubits"], draw=op["draw"], return_probability=True)
            return {"outcome": np.array(outcome, dtype=np.uint64), "probability": np.array(p)}
        elif kind == "expectation_terms":
            return {"values": sim.expectation_terms([pauli_ref.masks_to_text(x, z, n) for x, z in op["masks"]])}
        elif kind == "expectation_diagonal":
            return {"moments": np.array(sim.expectation_diagonal(self.diagonals[id(op)], moments=True))}
        elif kind == "norm2":
            return {"norm2": np.array(sim.norm2())}
        elif kind == "reduced_density":
            return {"rho": sim.reduced_density_matrix(op["qubits"])}
        elif kind == "subsystem_density":
            return {"rho": sim.subsystem_density_matrix(op["qubits"])}
        elif kind == "sample_shots":
            return {"outcomes": sim.sample_shots(draws=op["draws"], qubits=op["qubits"])}
        elif kind == "block_prob_masked":
            return {"sums": sim.block_prob_masked(op["hi_mask"], op["lo_mask"])}
        elif kind == "read_subrange":
            return {"amps": sim.read(op["first"], op["count"])}
        elif kind == "gradient":
            energy, grad = sim.energy_and_gradient(pauli_rot_ref.texts(op["rotations"], n), adjoint_ref.term_texts(op["terms"], n))
            return {"energy": np.array(energy), "grad": grad}
        elif kind in S.PARTNERED:
            return self._partnered(kind, op, run, i)
        elif kind == "lend_spare":
            sim.set_spare_buffer(self.spares.pop(0).data_ptr())
        elif kind == "withdraw_spare":
            sim.set_spare_buffer(None)
        elif kind == "grid_cap":
            sim.set_option(_lib.OPT_GRID_CAP, op["value"])
        elif kind == "reset":
            sim.reset()
        elif kind == "partial_write":
            values, inside = S.partial_values(op, n, self.precision)
            sim.write(np.where(inside, values, NAN))
            sim.set_support(op["support"])
        else:
            raise AssertionError(f"no driver for {kind}")
        return {}

    def begin(self, program):
        """Starts a program; step() issues its steps one by one (two sides can take turns); finish() reads everything back."""
        self._prepare(program)
        self.program, self.at, self.result, self.event = program, 0, Run(), None
        return self

    def step(self):
        i, (kind, op), run = self.at, self.program[self.at], self.result
        self.at += 1
        if not self.free and kind in VALUE_KINDS:
            run.before[i] = self.sim.read()
        t0 = time.perf_counter()
        values = self._issue((kind, op), run, i)
        run.issue_ms += 1e3 * (time.perf_counter() - t0)
        if kind not in S.WAITS:
            run.free_ms += 1e3 * (time.perf_counter() - t0)
        if values:
            run.values[i] = values
        if self.free:
            done = self.event is None or self.event.query()
            if self.event is not None:
                run.backed_up = not done  # as of the call that returned last
                run.ahead += not done
                if done and kind not in S.WAITS:
                    # a call that stages operands waits, by the ring's contract, once more than a ring of uploads has been made
                    # behind the blocker that is running: the slot it is given is still in flight
                    full = kind in UPLOADS and _uploads() - self.armed_at > S.STAGING_SLOTS
                    (run.slot_waits if full else run.stalls).append((i, kind))
            if done and self.blocker_ms > 0:
                self._arm(self.blocker_ms)
        elif kind not in S.QUEUES:
            if kind not in S.HOUSEKEEPING:
                self.sim.sync()
            self.torch.cuda.synchronize()
            if kind == "combine_into":
                run.after[i] = self.sim.read()
        return self.at < len(self.program)

    def rearm(self, ms=None):
        """A fresh blocker where the last one has ended (after something outside the program made the host wait); with `ms`, one of
        that length behind whatever is queued."""
        if self.free and (ms is not None or self.event is None or self.event.query()):
            self._arm(ms or self.blocker_ms)

    def _arm(self, ms):
        self.event, self.armed_at = blockers().arm(self.sim.stream, ms), _uploads()

    def finish(self):
        run = self.result
        self.sim.sync()
        run.final = self.sim.read()
        run.partners = [p.read() for p in self.pool[:self.used]]
        return run

    def run(self, program):
        self.begin(program)
        while self.step():
            pass
        return self.finish()


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def _same_bits(label, name, a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (label, name)
    assert a.tobytes() == b.tobytes(), f"{label}: {name} differs from the stepped twin's in {int(np.sum(a.view(np.uint8) != b.view(np.uint8)))} bytes"


def _check_twin(label, free, twin):
    assert free.values.keys() == twin.values.keys(), label
    for i in free.values:
        assert free.values[i].keys() == twin.values[i].keys(), (label, i)
        for name in free.values[i]:
            _same_bits(label, f"{name} of step {i}", free.values[i][name], twin.values[i][name])
    _same_bits(label, "the final read()", free.final, twin.final)
    assert len(free.partners) == len(twin.partners), label
    for k, (a, b) in enumerate(zip(free.partners, twin.partners)):
        _same_bits(label, f"partner {k}", a, b)


class Worst:
    """The worst fp64 error (as a share of its bound's scale) and fp32 ratio of a test, printed at its end."""

    def __init__(self):
        self.fp64, self.fp32 = 0.0, 0.0

    def state(self, label, precision, got, want, ref32):
        assert not np.isnan(got).any(), f"{label}: NaN in the state"
        if precision == 64:
            err = float(np.max(np.abs(got - want))) / max(1.0, float(np.linalg.norm(want)))
            self.fp64 = max(self.fp64, err)
            assert err <= TOL, f"{label}: max|got - want| / max(1, |want|) = {err:.3e} > {TOL}"
        else:
            try:
                e_got, e_ref = fp32_ref.check_fp32(got, want, ref32)
            except AssertionError as e:
                raise AssertionError(f"{label}: {e}") from None
            self.fp32 = max(self.fp32, e_got / max(e_ref, fp32_ref.FLOOR))

    def report(self, label):
        print(f"{label}: worst fp64 error {self.fp64:.3e} of max(1, |want|), worst fp32 rel_err(got) / max(rel_err(ref32), 2^-24) {self.fp32:.3f} (bound {fp32_ref.C:g})")


def _check_model(label, precision, run, model, worst):
    worst.state(f"{label}, final state", precision, run.final, model.want, model.ref32)
    assert len(run.partners) == len(model.partners), label
    for k, (got, (want, ref32)) in enumerate(zip(run.partners, model.partners)):
        worst.state(f"{label}, partner {k}", precision, got, want, ref32)


def _check_values(label, precision, program, run):
    """The stepped side's returned values against the feature's checker on the amplitudes read back before the step."""
    for i, got in run.values.items():
        kind, op = program[i]
        before, partner = run.before[i], run.partner_before.get(i)
        want = S.returned((kind, op), before, partner)
        n = int(before.size).bit_length() - 1
        norm2 = float(np.vdot(before, before).real)
        where = f"{label}, step {i} ({kind})"

        def close(name, tol):
            err = float(np.max(np.abs(np.asarray(got[name]) - np.asarray(want[name]))))
            assert err <= tol, f"{where}: {name} off by {err:.3e} > {tol:.3e}"

        if kind == "expectation_terms":          # test_gpu_expectation.py: TOL = 1e-10 absolute
            close("values", TOL)
        elif kind == "expectation_diagonal":     # test_gpu_diagonal.py _check_moments: TOL max|d| and TOL max|d|^2
            scale = float(np.max(np.abs(diagonal_ref.table_from_terms(n, op["terms"]))))
            assert abs(got["moments"][0] - want["moments"][0]) <= TOL * scale, where
            assert abs(got["moments"][1] - want["moments"][1]) <= TOL * scale * scale, where
        elif kind == "norm2":                    # test_gpu_state_algebra.py _check: norm2 within TOL
            close("norm2", TOL)
        elif kind in ("reduced_density", "subsystem_density"):  # test_gpu_density.py / test_gpu_subsystem.py: TOL = 1e-10 absolute
            close("rho", TOL)
        elif kind == "sample_shots":             # the draws keep sequence_ref.MARGIN from every boundary: the outcome is determined
            assert np.array_equal(got["outcomes"], want["outcomes"]), (where, got["outcomes"], want["outcomes"])
        elif kind == "block_prob_masked":        # sums of exactly formed squares in fp64, as the norm: TOL
            close("sums", TOL)
        elif kind == "read_subrange":
            _same_bits(where, "amps", got["amps"], want["amps"])
        elif kind == "gradient":                 # test_gpu_adjoint.py _check and _energy_tol
            weight = adjoint_ref.weight(op["terms"])
            if precision == 64:
                close("energy", TOL * weight)
                close("grad", TOL * weight)
            else:
                rot = list(op["rotations"])
                fwd64 = pauli_rot_ref.replay(before, rot)
                forward = fp32_ref.C * max(fp32_ref.rel_err(pauli_rot_ref.replay(before.astype(np.complex64), rot, np.complex64), fwd64), fp32_ref.FLOOR)
                close("energy", ((len(op["terms"]) + 2) * 2.0 ** -24 + 2.0 * forward) * weight)
                _, g32, _ = adjoint_ref.gradient(before.astype(np.complex64), rot, op["terms"], np.complex64)
                fp32_ref.check_fp32(got["grad"], want["grad"], g32)
        elif kind == "inner":                    # test_gpu_state_algebra.py: "the same holds for inner products", TOL
            close("inner", TOL)
        elif kind == "combine_into":             # test_gpu_state_algebra.py _check: against the norm of the state read back AFTER the call
            after = float(np.vdot(run.after[i], run.after[i]).real)
            assert abs(float(got["norm2"]) - after) <= TOL, where
        elif kind == "postselect":               # test_gpu_measure.py _check_weight
            W = float(want["weight"])
            assert abs(float(got["weight"]) - W) <= measure_ref.weight_tolerance(1 << (n - len(op["qubits"])), W), where
        elif kind == "measure":                  # test_gpu_measure.py test_measure_is_the_sampler...: the outcome, and p within weight_tolerance
            assert int(got["outcome"]) == op["outcome"], (where, int(got["outcome"]), op["outcome"])
            p = float(want["probability"])
            assert abs(float(got["probability"]) - p) <= measure_ref.weight_tolerance(1 << (n - len(op["qubits"])), p), where
        else:
            raise AssertionError(f"{where}: no check for its values")


def _ran_ahead(label, family, run, program, may_wait=MAY_WAIT):
    """The host ran ahead: no call but those that wait by contract (sequence_ref.WAITS) or by `may_wait` found its blocker ended when
    it returned, and the blocker was still running when the last call returned."""
    waits = sum(kind in S.WAITS for kind, _ in program)
    print(f"{label}: host issued {len(program)} steps in {run.issue_ms:.2f} ms (blockers of {BLOCKER_MS[family]:g} ms, waits included); "
          f"{run.ahead} calls returned behind a running blocker, {waits} calls wait by contract, with the operand ring full: {run.slot_waits}, others that waited: {run.stalls}")
    assert run.backed_up, f"{label}: the stream was not backed up when the last call returned"
    unexpected = [(i, kind) for i, kind in run.stalls if kind not in may_wait]
    assert not unexpected, f"{label}: the stream was not backed up: these calls do not wait by contract and found their blocker ended: {unexpected}"


def _both(n, precision, family, program, model, label, worst, free, twin, may_wait=MAY_WAIT):
    """Runs one program on both sides and makes every check."""
    got = free.run(program)
    _ran_ahead(label, family, got, program, may_wait)
    ref = twin.run(program)
    print(f"{label}: the stepped twin's calls took {ref.issue_ms:.2f} ms on the host, no blocker anywhere, {ref.free_ms:.2f} ms of it in calls that do not wait for the device")
    failed = []
    for check in (lambda: _check_twin(label, got, ref), lambda: _check_values(label, precision, program, ref),
                  lambda: _check_model(label, precision, got, model, worst), lambda: _check_model(label + " (stepped twin)", precision, ref, model, worst)):
        try:  # every check speaks: which of them fail together says where a mistake lies
            check()
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, " | ".join(failed)
    return got, ref


def _sides(n, precision, family, **kw):
    return Side(n, precision, True, BLOCKER_MS[family], **kw), Side(n, precision, False, **kw)


def _path(kind, op, n, precision):
    """The *path the plan call of a matrix or permutation step reports (host only)."""
    probe = plans.apply_matrix_plan if kind.startswith("matrix") else plans.apply_permutation_plan
    return plans.ok(probe(op["targets"], op["controls"], n, precision))["path"]


def _uploads():
    return plans.sweeps_launched("matrix") + plans.sweeps_launched("permutation") + plans.sweeps_launched("qft")


# ---- a. every ordered pair ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("first", S.KINDS)
def test_every_ordered_pair(first, precision):
    """[write(start), gates, A, B, gates] for every B, on one pair of Simulators."""
    worst, failed = Worst(), []
    free, twin = _sides(N, precision, "pair")
    with free, twin:
        for a, b, program, bld in S.pair_programs(N, precision, first=first):
            for kind, op in program:
                if kind in ("matrix_main", "matrix_small", "permutation_main", "permutation_small"):
                    assert _path(kind, op, N, precision) == (1 if kind.endswith("main") else 0), (kind, op["targets"], op["controls"])
            try:
                _both(N, precision, "pair", program, bld.model, f"{a} -> {b}, fp{precision}", worst, free, twin)
            except AssertionError as e:
                failed.append(f"{a} -> {b}: {e}")
    worst.report(f"pairs from {first}, fp{precision}")
    assert not failed, "\n".join(failed)


# ---- b. the operand ring goes round -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_operand_ring_goes_round(precision):
    program, bld = S.ring_programs(N, precision)["one"]
    assert sum(kind in S.STAGING for kind, _ in program) == S.RING_CALLS == 3 * S.STAGING_SLOTS + 5
    worst = Worst()
    free, twin = _sides(N, precision, "ring")
    with free, twin:
        count = _uploads()
        got = free.run(program)
        uploads = _uploads() - count
        label = f"operand ring, fp{precision}"
        _ran_ahead(label, "ring", got, program, may_wait=S.STAGING)  # a staging call waits where the slot it is given is still in flight
        print(f"{label}: {uploads} operand uploads in {S.RING_CALLS} calls; calls that waited for a slot: {got.slot_waits + got.stalls}")
        assert uploads > 3 * S.STAGING_SLOTS
        assert len(got.stalls) + len(got.slot_waits) >= 2, f"{label}: the host went round the ring without ever waiting for a slot: the stream was not backed up"
        ref = twin.run(program)
        print(f"{label}: the stepped twin's calls took {ref.issue_ms:.2f} ms on the host, no blocker anywhere, {ref.free_ms:.2f} ms of it in calls that do not wait for the device")
        _check_twin(label, got, ref)
        _check_model(label, precision, got, bld.model, worst)
    worst.report(label)


# ---- c. two states share the ring -------------------------------------------------------------------------------------------------------
def _turn(side):
    """One step of a side that shares the host with another: where the other side's call waited for a slot that this side's blocker
    was holding, that blocker has ended, so a fresh one goes in front of the call."""
    side.rearm()
    return side.step()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_states_share_the_ring(precision):
    programs = S.ring_programs(N, precision)
    (prog_a, bld_a), (prog_b, bld_b), (prog_c, bld_c) = programs["two_a"], programs["two_b"], programs["third"]
    worst, label = Worst(), f"two states on one ring, fp{precision}"
    half = 1 + S.TWO_STATES_FIRST_HALF
    with contextlib.ExitStack() as stack:
        a = stack.enter_context(Side(N, precision, True, BLOCKER_MS["two"])).begin(prog_a)
        b = stack.enter_context(Side(N, precision, True, BLOCKER_MS["two"])).begin(prog_b)
        count = _uploads()
        for _ in range(half):  # taking turns: adjacent slots of the ring belong to different streams
            _turn(a), _turn(b)
        # The third state comes, stages three operands and goes (forget_staged_operands) while the other two are backed up: a long
        # blocker behind what each has queued, no blocker of its own, and no device-wide wait of the test's in front of its closing.
        # Their uploads are then still in flight in the slots next to the ones it lets go of.
        a.rearm(THIRD_STATE_MS), b.rearm(THIRD_STATE_MS)
        third = Side(N, precision, True, 0.0, drain=False)
        got_c = third.run(prog_c)
        still = [not side.event.query() for side in (a, b)]
        assert still == [True, True], f"{label}: a stream was not backed up any more when the third state had made its calls: {still}"
        # qsim_destroy waits for the state's own stream, lets go of its slots (forget_staged_operands) and only then frees the state's
        # buffers; hipFree waits for every stream of the device, so the two blockers have ended by the time the call returns.  What
        # can be held is that they were running when it was made, and with them the two states' uploads in the neighbouring slots.
        third.__exit__(None, None, None)
        print(f"{label}: backed up when the third state was closed: {still}, when qsim_destroy had returned: {[not side.event.query() for side in (a, b)]}")
        a.rearm(), b.rearm()
        more = True
        while more:
            more = _turn(a)
            _turn(b)
        uploads = _uploads() - count
        got_a, got_b = a.finish(), b.finish()
        print(f"{label}: {uploads} operand uploads by three states")
        _ran_ahead(label + ", first state", "two", got_a, prog_a, may_wait=S.STAGING)
        _ran_ahead(label + ", second state", "two", got_b, prog_b, may_wait=S.STAGING)
        assert uploads > 3 * S.STAGING_SLOTS
        twin = stack.enter_context(Side(N, precision, False))
        for name, got, program, bld in (("first", got_a, prog_a, bld_a), ("second", got_b, prog_b, bld_b), ("third", got_c, prog_c, bld_c)):
            ref = twin.run(program)
            print(f"{label}, {name} state: the stepped twin's calls took {ref.issue_ms:.2f} ms on the host, no blocker anywhere, {ref.free_ms:.2f} ms of it in calls that do not wait for the device")
            _check_twin(f"{label}, {name} state", got, ref)
            _check_model(f"{label}, {name} state", precision, got, bld.model, worst)
    worst.report(label)


# ---- d. the tile-op ring wraps under load -------------------------------------------------------------------------------------------------
def test_the_tile_op_ring_wraps_under_load():
    precision = 64
    programs = S.ring_programs(N, precision)
    worst, label = Worst(), "tile-op ring"
    # Without the plan cache (OPTIONS) every pass takes its records from the ring.  The only call that may find its blocker ended is
    # the `rotations` step whose flush finds the ring full: launch_tile_pass then waits for the stream, blocker included, which IS the
    # wrap under load; two of them are asserted.  The blocks are counted on a third Simulator, profiled so that it keeps a launch
    # log, which runs the same programs afterwards: what a flush schedules depends on the gates and the options, not on when it runs.
    assert OPTIONS["plan_cache"] == 0
    free, twin = _sides(N, precision, "tile_ops")
    wraps = []
    with free, twin, Side(N, precision, False, profile=2) as census:
        for k in range(S.TILE_OP_PROGRAMS):  # one state throughout: the count of used records goes on from program to program
            program, bld = programs[f"tile_ops_{k}"]
            got, _ = _both(N, precision, "tile_ops", program, bld.model, f"{label}, program {k}", worst, free, twin, may_wait=("rotations",))
            wraps += [(k, i) for i, _ in got.stalls]
            census.run(program)
        print(f"{label}: flushes that waited for the stream behind a running blocker (program, step): {wraps}")
        assert len(wraps) >= 2, f"{label}: the ring did not wrap twice while the stream was backed up"
        blocks = sum(len(b) for b in census.sim.launch_log_blocks())
        passes = [side.sim.stats()["kernels"]["tile"]["launches"] for side in (free, twin, census)]
        print(f"{label}: {blocks} blocks in {passes[0]} tile passes went through the ring of {S.OPS_CAP} records")
        assert passes[0] == passes[1] == passes[2], passes
        assert free.sim.plan_cache_stats()["replays"] == 0
        assert blocks > 2 * S.OPS_CAP
    worst.report(label)


# ---- e. the tenants of the second buffer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lent", S.TENANTS)
def test_second_buffer_tenants(lent, precision):
    program, bld = S.tenant_program(N, precision, lent)
    worst, label = Worst(), f"second buffer {lent}, fp{precision}"
    free, twin = _sides(N, precision, "tenants")
    with free, twin:
        pointers = [side.sim.device_ptr for side in (free, twin)]
        _both(N, precision, "tenants", program, bld.model, label, worst, free, twin)
        assert [side.sim.device_ptr for side in (free, twin)] == pointers, f"{label}: the state ended in another buffer"
    worst.report(label)


# ---- f. partners with sweeps pending ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_partner_states_with_pending_sweeps(precision):
    program, bld = S.partner_program(N, precision)
    worst, label = Worst(), f"partners, fp{precision}"
    free, twin = _sides(N, precision, "partners", partner_blockers=True)
    with free, twin:
        got, _ = _both(N, precision, "partners", program, bld.model, label, worst, free, twin)
        assert got.partner_backed_up == [True] * len(S.PARTNERED), f"{label}: a partner's stream was not backed up when the call that reads it was issued"
    worst.report(label)


# ---- g. random walks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_random_walks(seed, precision):
    program, bld = S.random_program(N, 60, seed, precision)
    worst, label = Worst(), f"walk {seed}, fp{precision}"
    free, twin = _sides(N, precision, "walk")
    with free, twin:
        _both(N, precision, "walk", program, bld.model, label, worst, free, twin)
    worst.report(label)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed", SMALL_SEEDS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_random_walks_on_small_registers(n, seed, precision):
    """Registers smaller than a tile, a wave or a 16-byte unit; the operand recipes clip to k <= n."""
    program, bld = S.random_program(n, 60, seed, precision)
    worst, label = Worst(), f"walk {seed} on {n} qubits, fp{precision}"
    free, twin = _sides(n, precision, "small")
    with free, twin:
        _both(n, precision, "small", program, bld.model, label, worst, free, twin)
    worst.report(label)
