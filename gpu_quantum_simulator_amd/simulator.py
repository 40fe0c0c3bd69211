"""Python mirror of the C host: thin objects over the C ABI handles, nothing computed in Python.

`Simulator` = qsim_state (state vector in HBM; execute_single_qubit_gate :81-92 -> apply_1q,
execute_cnot :94-106 -> apply_cx, kernel_gate_4 quantum_simulator_4x4.cu:109-146 -> apply_2q).  `Circuit` lives in circuit.py, the
Pauli-list arguments in pauli_args.py, `Diagonal` in diagonal.py and the sharding handles in sharding.py; their names are re-exported
here, where they used to live."""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int, c_ubyte, c_uint32, c_uint64, c_void_p
from typing import Optional, Sequence

import numpy as np

from . import _lib, channels, permutations
from ._lib import QsimStats, check
from ._marshal import dp as _dp, ints as _ints, mat as _mat, u64p as _u64p
from .circuit import Circuit, gate_matrix
from .diagonal import Diagonal, _split_diagonal_observable, _split_diagonal_steps
from .pauli_args import _control_masks, _hamiltonian_arrays, _PauliStrings, _rotation_arrays, _split_controls
from .sharding import Cluster, RankComm, ShardPlanHandle  # noqa: F401  (re-exported)


class Simulator(_PauliStrings, _lib.Handle):
    """One state vector resident on one GPU."""
    _expect_fn, _rotate_fn, _check, _free = "qsim_expect_paulis", "qsim_apply_pauli_rotations", staticmethod(check), "qsim_destroy"

    def __init__(self, num_q: int, device: int = 0, *, fuse: Optional[int] = None, profile: bool = False,
                 external_ptr: Optional[int] = None, precision: int = 64, **options):
        self._h = c_void_p()
        lib = _lib.load()
        if precision not in (32, 64):
            raise ValueError("precision must be 64 (fp64 complex, the parity configuration) or 32")
        self.precision = precision
        if precision == 32:
            if external_ptr is not None:
                raise ValueError("external buffers are fp64 only")
            check(lib.qsim_create_f32(byref(self._h), num_q, device))
        elif external_ptr is None:
            check(lib.qsim_create(byref(self._h), num_q, device))
        else:
            check(lib.qsim_create_external(byref(self._h), num_q, device, c_void_p(external_ptr)))
        self.num_qubits = num_q
        if fuse is not None:
            self.set_option(_lib.OPT_FUSE, fuse)
        if profile:
            self.set_option(_lib.OPT_PROFILE, int(profile))  # True / 1: HIP events per launch; 2: block forms as well (launch_log_blocks)
        names = {"tile_bits": _lib.OPT_TILE_BITS, "tile_low_bits": _lib.OPT_TILE_LOW_BITS,
                 "max_pending": _lib.OPT_MAX_PENDING, "tile_max_ops": _lib.OPT_TILE_MAX_OPS,
                 "grid_cap": _lib.OPT_GRID_CAP, "tile_threads": _lib.OPT_TILE_THREADS,
                 "tile_pad_from": _lib.OPT_TILE_PAD_FROM, "debug_tile_order": _lib.OPT_DEBUG_TILE_ORDER, "plan_cache": _lib.OPT_PLAN_CACHE,
                 "pingpong": _lib.OPT_PINGPONG, "sparse_start": _lib.OPT_SPARSE_START, "debug_plan_key": _lib.OPT_DEBUG_PLAN_KEY,
                 "defer_flips": _lib.OPT_DEFER_FLIPS, "affine_support": _lib.OPT_AFFINE_SUPPORT}
        # tile_low_bits first when shrinking, tile_bits first when growing: keep every intermediate valid
        for key in sorted(options, key=lambda k: k != "tile_low_bits"):
            self.set_option(names[key], options[key])

    # -- options / lifecycle
    def set_option(self, opt: int, value: int) -> None:
        check(_lib.load().qsim_set_option(self._h, opt, value))

    # -- adjoint gradients (single states only: a Cluster has no counterpart)
    def energy_and_gradient(self, rotations, terms):
        """(E, grad): E = <psi|H|psi> after the rotations and grad[k] = dE/dtheta_k, for `rotations` as apply_pauli_rotations
        takes them and H = `terms` as expectation takes them, real coefficients (ValueError for a complex one).  Adjoint
        differentiation on the device (qsim_pauli_gradient): one forward pass, one application of H, one backward pass.  The
        state is left as the call found it, to rounding.
        Entries may be (theta, string, controls), mixed with plain ones, as apply_pauli_rotations takes them, with the same
        ValueErrors (qsim_controlled_pauli_gradient): the derivative with respect to the angle of a controlled rotation, which the
        two-term shift rule gets wrong; its backward sweep touches 2^-c of the state and of lambda for c controls.
        An entry may also be (gamma, diag) with a Diagonal: the step exp(-i gamma D) of apply_diagonal_phase, one sweep forwards and
        one backwards whatever the number of terms D has, and grad[k] = dE/dgamma.  `terms` may be a Diagonal (H = D) or hold one
        (w, diag) among its pairs (H = sum_t c_t P_t + w D): a QAOA loop is energy_and_gradient(layers, cost)
        (qsim_diagonal_gradient).  ValueError, before any launch, for controls on a diagonal entry, two diagonal parts in `terms`, a
        complex weight or gamma."""
        rotations, tables = _split_diagonal_steps(rotations)
        terms, obs, weight = _split_diagonal_observable(terms)
        pairs, controls = _split_controls(rotations)
        rxs, rzs, thetas, rxp, rzp, tp = _rotation_arrays(pairs, self.num_qubits)
        hxs, hzs, coeffs, hxp, hzp, cp = _hamiltonian_arrays(terms, self.num_qubits)
        energy, grad = c_double(0.0), np.zeros(rxs.size, dtype=np.float64)
        cs, csp = _control_masks(pairs, controls, self.num_qubits)  # None where no entry has controls
        if obs is not None or any(t is not None for t in tables):
            steps = (c_void_p * max(len(tables), 1))(*[t._h.value if t is not None else None for t in tables])
            check(_lib.load().qsim_diagonal_gradient(self._h, rxs.size, steps, csp, rxp, rzp, tp, hxp, hzp, cp, hxs.size, obs._h if obs is not None else None,
                                                     weight, byref(energy), _dp(grad)))
        elif cs is not None:
            check(_lib.load().qsim_controlled_pauli_gradient(self._h, csp, rxp, rzp, tp, rxs.size, hxp, hzp, cp, hxs.size, byref(energy), _dp(grad)))
        else:
            check(_lib.load().qsim_pauli_gradient(self._h, rxp, rzp, tp, rxs.size, hxp, hzp, cp, hxs.size, byref(energy), _dp(grad)))
        return float(energy.value), grad

    # -- state algebra and the Lanczos solver (single states only: a Cluster has no counterpart)
    def copy_from(self, other: "Simulator") -> None:
        """This state <- `other`, bit for bit (qsim_copy_state); same qubit count, precision and device.  Not waited for."""
        check(_lib.load().qsim_copy_state(self._h, other._h))

    def inner(self, other: "Simulator") -> complex:
        """<self|other> = sum_i conj(self_i) other_i, one sweep on the device (qsim_inner); inner(self) is the squared norm."""
        re, im = c_double(), c_double()
        check(_lib.load().qsim_inner(self._h, other._h, byref(re), byref(im)))
        return complex(re.value, im.value)

    def combine(self, d, ap, bq=None, norm: bool = False):
        """self <- d self + a p + b q for ap = (a, p) and bq = (b, q) or None, complex numbers and Simulators other than self
        (qsim_combine).  d == 0: self is overwritten without being read.  norm=True returns the squared norm of the result from
        the same sweep (and waits for it); otherwise None, not waited for."""
        def pair(z):
            z = complex(z)
            return np.array([z.real, z.imag], dtype=np.float64)

        dd, aa = pair(d), pair(ap[0])
        bb = pair(bq[0]) if bq is not None else None
        out = c_double()
        check(_lib.load().qsim_combine(self._h, _dp(dd), ap[1]._h, _dp(aa), bq[1]._h if bq is not None else None,
                                       _dp(bb) if bb is not None else None, byref(out) if norm else None))
        return float(out.value) if norm else None

    def ground_state(self, terms, tol: float, max_steps: int = 200, vector: bool = True) -> dict:
        """The lowest eigenvalue of H = `terms` (as expectation takes them, real coefficients: ValueError for a complex one) by
        Lanczos iteration from the current state (qsim_lanczos_ground): keys energy, residual, steps, converged, alphas, betas.
        `tol` bounds |H y - E y| for the unit Ritz vector y.  vector=True leaves the state as y and returns the MEASURED residual;
        vector=False leaves the state's bits alone and returns the estimate.  converged: the iteration stopped before max_steps
        (the residual estimate met tol, or the start vector's Krylov space was exhausted) or the returned residual meets tol."""
        xs, zs, coeffs, xp, zp, cp = _hamiltonian_arrays(terms, self.num_qubits)
        energy, residual, steps = c_double(), c_double(), c_int()
        alphas, betas = np.zeros(max(int(max_steps), 1)), np.zeros(max(int(max_steps), 1))
        check(_lib.load().qsim_lanczos_ground(self._h, xp, zp, cp, xs.size, int(max_steps), float(tol), 1 if vector else 0, byref(energy),
                                              byref(residual), byref(steps), _dp(alphas), _dp(betas)))
        m = steps.value
        return {"energy": float(energy.value), "residual": float(residual.value), "steps": m,
                "converged": bool(m < max_steps or residual.value <= tol), "alphas": alphas[:m].copy(), "betas": betas[:m].copy()}

    # -- controlled rotations (single states only)
    def _apply_controlled(self, pairs, controls, xp, zp, tp) -> None:
        cs, csp = _control_masks(pairs, controls, self.num_qubits)
        check(_lib.load().qsim_apply_controlled_pauli_rotations(self._h, csp, xp, zp, tp, cs.size))

    def apply_mcphase(self, phi: float, qubits) -> None:
        """diag(1, ..., 1, e^(i phi)) on `qubits`: the phase e^(i phi) where all of them are 1 — the controlled identity string
        with theta = -2 phi, one sweep over 2^-len(qubits) of the state.  Symmetric in the qubits."""
        self.apply_pauli_rotation(-2.0 * phi, "", qubits)

    def apply_mcz(self, qubits) -> None:
        """The multi-controlled Z on `qubits` (a Grover oracle's phase flip of |1...1>): apply_mcphase(pi, qubits)."""
        self.apply_mcphase(np.pi, qubits)

    def apply_mcx(self, controls, target: int) -> None:
        """X on `target` where every qubit of `controls` is 1 (two controls: the Toffoli gate).  No control: the X gate; one:
        apply_cx.  More: the controlled rotation by pi about X on the target, which is -i X there, then the controlled identity
        with theta = -pi, the phase i — two sweeps, each over 2^-len(controls) of the state, together exactly X."""
        controls = tuple(controls)
        if len(controls) == 0:
            self.apply_1q(np.array([[0, 1], [1, 0]]), target)
        elif len(controls) == 1:
            if controls[0] == target:
                raise ValueError(f"control qubit {target} is the target")
            self.apply_cx(controls[0], target)
        else:
            self.apply_pauli_rotations([(np.pi, f"X{target}", controls), (-np.pi, "", controls)])

    def pauli_sum_into(self, terms, dst_ptr: int) -> None:
        """dst = sum_t c_t Q_t |state> for (real coefficient, string) pairs, written to the device buffer at `dst_ptr` (2^n
        amplitudes of this state's precision, not this state's own buffer); queued on the state's stream, not waited for."""
        xs, zs, coeffs, xp, zp, cp = _hamiltonian_arrays(terms, self.num_qubits)
        check(_lib.load().qsim_pauli_sum_into(self._h, xp, zp, cp, xs.size, c_void_p(dst_ptr)))

    def reset(self, holds_index0: bool = True) -> None:
        check(_lib.load().qsim_reset_shard(self._h, 1 if holds_index0 else 0))

    # -- gates
    def apply_1q(self, U, target: int) -> None:
        check(_lib.load().qsim_apply_1q(self._h, _dp(_mat(U, 2)), target))

    def apply_cx(self, control: int, target: int) -> None:
        check(_lib.load().qsim_apply_cx(self._h, control, target))

    def apply_2q(self, U, q_hi: int, q_lo: int) -> None:
        check(_lib.load().qsim_apply_2q(self._h, _dp(_mat(U, 4)), q_hi, q_lo))

    def apply_matrix(self, U, targets, controls=()) -> None:
        """The (2^k, 2^k) matrix `U` on `targets` (at most 5, distinct, any order; bit j of a row or column index is targets[j])
        where every qubit of `controls` (any number, disjoint from the targets) is 1, the identity elsewhere.  Any complex matrix:
        a unitary, a Kraus operator, a projector — nothing checks unitarity; k = 0: a complex scalar on the control subspace.
        One in-place sweep of 2^-len(controls) of the state on the device (qsim_apply_matrix), launched after the queued gates
        and not waited for; it does not pass through the gate queue.  Single states only: a Cluster has no such method, sharded
        states have no controlled operations."""
        ts, cs = [int(q) for q in targets], [int(q) for q in controls]
        m = np.asarray(U, dtype=np.complex128)
        dim = 1 << min(len(ts), 5)
        if len(ts) > 5 or m.size != dim * dim or m.ndim > 2 or (m.ndim == 2 and m.shape != (dim, dim)):
            raise ValueError(f"apply_matrix: at most 5 targets and a matrix of shape (2^k, 2^k); got {len(ts)} targets and shape {m.shape}")
        check(_lib.load().qsim_apply_matrix(self._h, _dp(_mat(m, dim)), _ints(ts), len(ts), _ints(cs), len(cs)))

    # -- permutations of the basis states of up to ten qubits (single states only: a Cluster has no counterpart)
    def apply_permutation(self, perm, targets, controls=(), inverse: bool = False) -> None:
        """Basis state j of `targets` (at most 10, distinct, any order; bit i of j is targets[i]) goes to basis state perm[j] where
        every qubit of `controls` (any number, disjoint from the targets) is 1; nothing is read or written elsewhere.  `perm` is a
        bijection of range(2**k); inverse=True applies permutations.inverse_table(perm).  Amplitudes are moved bit for bit, fp64 and
        fp32: apply_matrix with U[perm[j], j] = 1 without the arithmetic.  One in-place sweep of 2^-len(controls) of the state
        (qsim_apply_permutation), launched after the queued gates and not waited for; it does not pass through the gate queue.
        ValueError, before the library is called: a table of the wrong length, a non-integer entry, not a bijection."""
        ts, cs = [int(q) for q in targets], [int(q) for q in controls]
        if len(ts) > permutations.MAX_QUBITS:
            raise ValueError(f"apply_permutation: at most {permutations.MAX_QUBITS} targets, got {len(ts)}")
        table = permutations.as_table(perm, len(ts))
        if inverse:
            table = permutations.inverse_table(table)
        table = np.ascontiguousarray(table, dtype=np.uint32)
        check(_lib.load().qsim_apply_permutation(self._h, table.ctypes.data_as(ctypes.POINTER(c_uint32)), _ints(ts), len(ts),
                                                 _ints(cs), len(cs)))

    def apply_function_xor(self, values, inputs, outputs, controls=()) -> None:
        """|x>|y> -> |x>|y ^ values[x]>: bit i of x is inputs[i], bit i of y is outputs[i]; a bit oracle for any function of up to
        10 - len(outputs) bits (permutations.xor_function_table)."""
        ins, outs = [int(q) for q in inputs], [int(q) for q in outputs]
        self.apply_permutation(permutations.xor_function_table(values, len(ins), len(outs)), ins + outs, controls)

    def apply_modular_add(self, a: int, modulus: int, targets, controls=()) -> None:
        """x -> (x + a) mod `modulus` on the register `targets` (bit i of x is targets[i]), the identity on x >= modulus
        (permutations.modular_add_table)."""
        ts = [int(q) for q in targets]
        self.apply_permutation(permutations.modular_add_table(a, modulus, len(ts)), ts, controls)

    def apply_modular_multiply(self, a: int, modulus: int, targets, controls=()) -> None:
        """x -> a x mod `modulus` on the register `targets`, the identity on x >= modulus; gcd(a, modulus) = 1
        (permutations.modular_multiply_table).  Under one control per counting qubit: the modular exponentiation of order finding."""
        ts = [int(q) for q in targets]
        self.apply_permutation(permutations.modular_multiply_table(a, modulus, len(ts)), ts, controls)

    # -- the quantum Fourier transform on any qubits (single states only: a Cluster has no counterpart)
    def apply_qft(self, qubits, inverse: bool = False, *, max_digit_bits: int = 0) -> None:
        """The quantum Fourier transform on the register `qubits` (any number up to the whole state, distinct, any order and places;
        bit j of the register value is qubits[j]): new[y] = 2^(-k/2) sum_x exp(+2 pi i x y / 2^k) old[x] for every setting of the other
        qubits, exp(-...) with inverse=True; in numpy terms forwards is ifft * sqrt(2^k) along the register axis.  The output is in
        natural order (the textbook circuit with its final swaps).  One sweep per digit of at most ten qubits (qsim_apply_qft),
        launched after the queued gates and not waited for; it does not pass through the gate queue.  max_digit_bits (1 ... 10) caps
        the digits, for tests and tuning; 0 leaves the choice to the plan.  An empty register is accepted and does nothing."""
        qs = [int(q) for q in qubits]
        check(_lib.load().qsim_apply_qft(self._h, _ints(qs), len(qs), 1 if inverse else 0, int(max_digit_bits)))

    # -- whole-register diagonal operators from a table (single states only: a Cluster has no counterpart)
    def apply_diagonal_phase(self, diag: Diagonal, gamma: float) -> None:
        """a_i <- exp(-i gamma d_i) a_i for the table of `diag`: one in-place sweep (qsim_apply_diagonal_phase), launched after
        the queued gates and not waited for.  For diag = Diagonal.from_terms(n, [(c_k, P_k)]) it equals
        apply_pauli_rotations([(2 gamma c_k, P_k)]) — a QAOA phase separator in one sweep whatever the number of terms."""
        check(_lib.load().qsim_apply_diagonal_phase(self._h, diag._h, float(gamma)))

    def diagonal_into(self, diag: Diagonal, dst_ptr: int, weight: float = 1.0, accumulate: bool = False) -> None:
        """dst = weight D |state>, or dst += with accumulate=True, for the table of `diag`, written to the device buffer at `dst_ptr`
        (2^n amplitudes of this state's precision, not this state's own buffer): one out-of-place sweep
        (qsim_diagonal_apply_into), queued on the state's stream, not waited for.  When storing, dst's old contents are not read."""
        check(_lib.load().qsim_diagonal_apply_into(self._h, diag._h, float(weight), c_void_p(dst_ptr), 1 if accumulate else 0))

    def expectation_diagonal(self, diag: Diagonal, moments: bool = False):
        """<D> = sum_i d_i |a_i|^2 for the table of `diag`, one read-only sweep (qsim_expect_diagonal); moments=True returns
        (<D>, <D^2>), the variance being their <D^2> - <D>^2."""
        out = np.zeros(2, dtype=np.float64)
        check(_lib.load().qsim_expect_diagonal(self._h, diag._h, _dp(out)))
        return (float(out[0]), float(out[1])) if moments else float(out[0])

    def run(self, circuit: Circuit, first: int = 0, count: int = -1) -> None:
        check(_lib.load().qsim_run_circuit(self._h, circuit._h, first, count))

    def flush(self) -> None:
        check(_lib.load().qsim_flush(self._h))

    def plan_cache_stats(self) -> dict:
        """qsim_plan_cache_stats: plans held, replays, key matches rejected by the identity check."""
        a, b, c = c_uint64(), c_uint64(), c_uint64()
        check(_lib.load().qsim_plan_cache_stats(self._h, byref(a), byref(b), byref(c)))
        return {"plans": int(a.value), "replays": int(b.value), "key_collisions": int(c.value)}

    def deferred_flip_stats(self) -> dict:
        """qsim_deferred_flip_stats: flushes whose last tile pass applied the deferred X gates' index flip, and flushes that
        had to run them in a pass of their own."""
        a, b = c_uint64(), c_uint64()
        check(_lib.load().qsim_deferred_flip_stats(self._h, byref(a), byref(b)))
        return {"applied": int(a.value), "fallbacks": int(b.value)}

    def choose_schedule(self, circuit: Circuit) -> None:
        """qsim_choose_schedule: the schedule choice of the planning step alone (no timing)."""
        check(_lib.load().qsim_choose_schedule(self._h, circuit._h))

    def tune(self, circuit: Circuit, max_candidates: int = 32, budget_ms: float = 6000.0, dense_start: bool = False) -> dict:
        """qsim_tune_circuit(_from): times every pass of the circuit's schedule under candidate orders of its tile bits and
        keeps the fastest per geometry in the library's process-wide table (planning; leaves the state reset).
        dense_start: the circuit will run on a state that is not fresh from a reset (its first passes are scheduled differently)."""
        rep = _lib.QsimTuneReport()
        check(_lib.load().qsim_tune_circuit_from(self._h, circuit._h, max_candidates, budget_ms, byref(rep), 1 if dense_start else 0))
        return rep.as_dict()

    def flush_pack(self, bits: Sequence[int], out_ptr: Optional[int] = None, to_bits: Optional[Sequence[int]] = None, konst: int = 0,
                   needed: int = (1 << 64) - 1, skip_blocks: int = 0):
        """qsim_flush_pack: everything queued is launched and the state ends re-laid-out in `out_ptr` (default: the spare
        buffer); returns (buffer holding the packed state, whether the last tile pass did the re-layout)."""
        k = len(bits)
        arr = _ints(bits)
        to = _ints(to_bits) if to_bits is not None else None
        at, fused = c_void_p(), c_int()
        check(_lib.load().qsim_flush_pack(self._h, arr, k, to, konst, c_void_p(out_ptr or 0), needed, skip_blocks, byref(at), byref(fused)))
        return int(at.value or 0), bool(fused.value)

    def pack_bits_to(self, bits: Sequence[int], dst_ptrs: Sequence[int]) -> None:
        """qsim_pack_bits_to: block b of the packed layout goes to dst_ptrs[b]."""
        arr = _ints(bits)
        ptrs = (c_void_p * len(dst_ptrs))(*dst_ptrs)
        check(_lib.load().qsim_pack_bits_to(self._h, arr, len(bits), ptrs))

    def set_support(self, support: int) -> None:
        """qsim_set_support: amplitudes whose index has a bit outside `support` are zero by definition from now on."""
        check(_lib.load().qsim_set_support(self._h, support))

    def support_after(self, circuit: Circuit, support: int = 0) -> int:
        """qsim_support_after: where the state can be non-zero after `circuit` ran on a state with this support, as the engine
        will track it (scheduled as a flush would schedule it; nothing runs)."""
        out = c_uint64()
        check(_lib.load().qsim_support_after(self._h, circuit._h, support & 0xFFFFFFFFFFFFFFFF, byref(out)))
        return int(out.value)

    def get_support(self):
        """(support mask, pending basis state?, its amplitude) — qsim_get_support."""
        m, k, a = c_uint64(), c_int(), c_double()
        check(_lib.load().qsim_get_support(self._h, byref(m), byref(k), byref(a)))
        return int(m.value), bool(k.value), float(a.value)

    def set_spare_buffer(self, ptr: Optional[int]):
        """qsim_set_spare_buffer: lends the state a second device buffer for out-of-place tile passes (None takes it back)."""
        check(_lib.load().qsim_set_spare_buffer(self._h, c_void_p(ptr or 0)))

    def swap_buffer(self, ptr: int) -> int:
        """qsim_swap_buffer: the state takes `ptr` as its amplitude buffer; returns the buffer it held before."""
        p = c_void_p(ptr)
        check(_lib.load().qsim_swap_buffer(self._h, byref(p)))
        return int(p.value)

    def block_prob_masked(self, hi_mask: int, lo_mask: int) -> np.ndarray:
        out = np.zeros(1 << bin(hi_mask).count("1"), dtype=np.float64)
        check(_lib.load().qsim_block_prob_masked(self._h, hi_mask, lo_mask, _dp(out)))
        return out

    def gather_masked(self, base: int, lo_mask: int) -> np.ndarray:
        out = np.zeros(2 << bin(lo_mask).count("1"), dtype=np.float64)
        check(_lib.load().qsim_gather_masked(self._h, base, lo_mask, _dp(out)))
        return out.view(np.complex128)

    # -- subsystems (single states only: a Cluster has no counterpart)
    def reduced_density_matrix(self, qubits) -> np.ndarray:
        """rho_A = Tr_B |psi><psi| for A = `qubits` (at most 5, distinct, any order) as a (2^k, 2^k) complex128 array; bit j of a
        row or column index is qubits[j].  One read-only sweep of the state on the device (qsim_reduced_density); exactly
        Hermitian, fp64 sums in both precisions, equal calls return equal bits.  Not normalised: its trace is norm2()."""
        qs = [int(q) for q in qubits]
        arr = _ints(qs)
        out = np.zeros(2 << (2 * len(qs)) if len(qs) <= 5 else 2, dtype=np.float64)  # more than 5: the library refuses
        check(_lib.load().qsim_reduced_density(self._h, arr, len(qs), _dp(out)))
        return out.view(np.complex128).reshape(1 << len(qs), 1 << len(qs))

    def marginal_probabilities(self, qubits) -> np.ndarray:
        """The joint distribution of `qubits` (distinct, any order) as 2^k float64, bit j of an outcome being qubits[j].  Up to 5
        qubits: the diagonal of reduced_density_matrix; more: block_prob_masked over the subset, reordered here."""
        qs = [int(q) for q in qubits]
        k = len(qs)
        if k <= 5:
            return np.ascontiguousarray(np.real(np.diagonal(self.reduced_density_matrix(qs))))
        if len(set(qs)) != k or any(q < 0 or q >= self.num_qubits for q in qs):
            raise ValueError(f"marginal_probabilities: {qs} are not distinct qubits of a register of {self.num_qubits}")
        mask = sum(1 << q for q in qs)
        p = self.block_prob_masked(mask, ((1 << self.num_qubits) - 1) & ~mask)  # outcome bits in ascending qubit order
        rank = {q: r for r, q in enumerate(sorted(qs))}
        return np.ascontiguousarray(p.reshape((2,) * k).transpose([k - 1 - rank[q] for q in reversed(qs)]).reshape(-1))

    def subsystem_density_matrix(self, qubits) -> np.ndarray:
        """rho_A for up to 10 qubits (distinct, any order), with reduced_density_matrix's conventions: (2^k, 2^k) complex128, bit j of
        an index is qubits[j], not normalised, exactly Hermitian, equal calls return equal bits.  Up to 5 qubits this IS
        reduced_density_matrix, bit for bit; 6 to 10 run R R^T in blocks and slices on the matrix cores (qsim_subsystem_density;
        DESIGN §7m) and read the state 2^(k-6) times."""
        qs = [int(q) for q in qubits]
        arr = _ints(qs)
        out = np.zeros(2 << (2 * len(qs)) if len(qs) <= 10 else 2, dtype=np.float64)  # more than 10: the library refuses
        check(_lib.load().qsim_subsystem_density(self._h, arr, len(qs), _dp(out)))
        return out.view(np.complex128).reshape(1 << len(qs), 1 << len(qs))

    def _block_or_complement(self, qubits):
        """rho of `qubits`, or — only when they are more than 10 and the other qubits are not — of the OTHER qubits: a Simulator holds a
        pure state vector, and the two sides of a pure state share their non-zero spectrum (Schmidt), hence purity and entropy."""
        qs = [int(q) for q in qubits]
        n = self.num_qubits
        if len(qs) > 10 and n - len(qs) <= 10 and len(set(qs)) == len(qs) and all(0 <= q < n for q in qs):
            qs = [q for q in range(n) if q not in qs]
        return self.subsystem_density_matrix(qs)

    def entanglement_spectrum(self, qubits) -> np.ndarray:
        """The eigenvalues of rho_A / Tr rho_A for A = `qubits`, descending, float64: 2^k values for up to 10 qubits.  More than 10
        qubits whose complement has at most 10: the complement's 2^(n-k) values, which are all the non-zero ones of a pure state."""
        rho = self._block_or_complement(qubits)
        return np.ascontiguousarray(np.linalg.eigvalsh(rho / np.real(np.trace(rho)))[::-1])

    def purity(self, qubits) -> float:
        """Tr rho_A^2 for the reduced density matrix of `qubits`, normalised by its trace (1 for a pure product, 2^-k fully mixed).
        Up to 10 qubits; more when the other qubits are at most 10 (the complement's rho: the same value for a pure state)."""
        rho = self._block_or_complement(qubits)
        tr = float(np.real(np.trace(rho)))
        return float(np.real(np.sum(rho * rho.T))) / (tr * tr)  # Tr rho^2 = sum |rho_ab|^2 for a Hermitian rho

    def entanglement_entropy(self, qubits, base: float = 2) -> float:
        """The von Neumann entropy -Tr rho_A log rho_A of `qubits` against the rest, in units of log `base` (bits by default), from
        the eigenvalues of the small matrix (normalised by its trace); eigenvalues <= 0 are rounding and are left out.  Up to 10
        qubits; more when the other qubits are at most 10 (the complement's rho: the same value for a pure state)."""
        rho = self._block_or_complement(qubits)
        w = np.linalg.eigvalsh(rho / np.real(np.trace(rho)))
        w = w[w > 0.0]
        return float(-np.sum(w * np.log(w)) / np.log(base))

    def pack_bits(self, bits: Sequence[int], dst_ptr: int) -> None:
        """Shard re-layout ahead of a global<->local qubit exchange (qsim_pack_bits)."""
        arr = _ints(bits)
        check(_lib.load().qsim_pack_bits(self._h, arr, len(bits), c_void_p(dst_ptr)))

    def scale(self, z: complex) -> None:
        check(_lib.load().qsim_scale(self._h, float(z.real), float(z.imag)))

    def sync(self) -> None:
        check(_lib.load().qsim_sync(self._h))

    # -- amplitudes
    def read(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = (1 << self.num_qubits) - first
        out = np.empty(2 * count, dtype=np.float64)
        check(_lib.load().qsim_read(self._h, first, count, _dp(out)))
        return out.view(np.complex128)

    def write(self, amps: np.ndarray, first: int = 0) -> None:
        a = np.ascontiguousarray(amps, dtype=np.complex128)
        check(_lib.load().qsim_write(self._h, first, a.size, _dp(a.view(np.float64))))

    def sample(self, randoms) -> np.ndarray:
        """Basis index measurement() (quantum_simulator.c:270-283) returns for each random number in [0, 1]."""
        r = np.ascontiguousarray(randoms, dtype=np.float64)
        out = np.zeros(r.size, dtype=np.uint64)
        check(_lib.load().qsim_sample(self._h, _dp(r), r.size, _u64p(out)))
        return out

    def sample_shots(self, shots: Optional[int] = None, qubits=None, *, seed=None, draws=None) -> np.ndarray:
        """Basis states drawn on the device (qsim_sample_shots): one uint64 per shot — the basis index, or with `qubits`
        the outcome on them (bit j of a result is qubit qubits[j]).  Pass either `draws`, the caller's own numbers in [0, 1] (a
        reproducible pipeline), or `shots`, for which np.random.default_rng(seed).random(shots) is drawn here.  The draws are scaled by
        the state's own total, so an unnormalised state samples |a|^2 / norm2; an index of probability zero is never returned.  Pending
        gates are launched first; the state is not changed."""
        if (draws is None) == (shots is None):
            raise ValueError("sample_shots takes either shots or draws")
        if draws is None:
            if int(shots) < 0:
                raise ValueError("shots must not be negative")
            draws = np.random.default_rng(seed).random(int(shots))
        elif seed is not None:
            raise ValueError("a seed goes with shots, not with draws")
        u = np.ascontiguousarray(draws, dtype=np.float64).reshape(-1)
        qs = [] if qubits is None else [int(q) for q in qubits]
        arr = _ints(qs) if qs else None
        out = np.zeros(u.size, dtype=np.uint64)
        check(_lib.load().qsim_sample_shots(self._h, _dp(u), u.size, arr, len(qs), _u64p(out)))
        return out

    def sample_counts(self, shots: int, qubits=None, seed=None) -> dict:
        """{outcome: how often it was drawn} over sample_shots(shots, qubits, seed=seed), keys ascending."""
        values, counts = np.unique(self.sample_shots(shots, qubits, seed=seed), return_counts=True)
        return {int(v): int(c) for v, c in zip(values, counts)}

    # -- measurement: collapse, post-selection, reset, Kraus channels (single states only: a Cluster has no counterpart)
    @staticmethod
    def _one_draw(who: str, seed, draw) -> float:
        """The number in [0, 1] a measuring call goes by: the caller's `draw`, or the first of np.random.default_rng(seed).random(1) —
        what sample_shots(1, seed=seed) would draw."""
        if draw is None:
            return float(np.random.default_rng(seed).random(1)[0])
        if seed is not None:
            raise ValueError(f"{who}: a seed or a draw, not both")
        return float(draw)

    def postselect(self, qubits, outcome: int) -> float:
        """Projects the state onto `outcome` of `qubits` (any number up to the whole state, distinct, any order and places; bit j of the
        outcome is qubits[j]) and normalises it: the other amplitudes become +0.0, the kept ones are divided by sqrt(W).  Returns W, the
        squared norm of the kept part before the call — the outcome's probability on a normalised state.  Two sweeps on the device
        (qsim_postselect), after the queued gates; the discarded amplitudes are overwritten without being read.  QsimError
        for an outcome of probability zero, the state's bits then unchanged."""
        qs = [int(q) for q in qubits]
        if int(outcome) < 0 or int(outcome) >> 64:
            raise ValueError(f"postselect: the outcome is a non-negative integer below 2^k, got {outcome!r}")
        w = c_double()
        check(_lib.load().qsim_postselect(self._h, _ints(qs), len(qs), int(outcome), byref(w)))
        return w.value

    def measure(self, qubits, *, seed=None, draw=None, return_probability: bool = False):
        """Measures `qubits` in the computational basis and collapses the state onto what was read: returns the outcome (bit j is
        qubits[j]), with return_probability=True (outcome, its probability).  The outcome is exactly sample_shots(draws=[u],
        qubits=qubits)[0] for the same state and number u in [0, 1]: `draw` is that number (a reproducible pipeline), otherwise it comes
        from `seed` the way sample_shots(1, seed=seed) makes its draw.  An unnormalised state measures |a|^2 / norm2; afterwards the
        state has norm 1 (qsim_measure)."""
        qs = [int(q) for q in qubits]
        out, p = c_uint64(), c_double()
        check(_lib.load().qsim_measure(self._h, _ints(qs), len(qs), self._one_draw("measure", seed, draw), byref(out), byref(p)))
        return (int(out.value), p.value) if return_probability else int(out.value)

    def reset_qubits(self, qubits, *, seed=None, draw=None) -> int:
        """Measures `qubits` and returns every one of them to |0>: measure(), then an x gate through the ordinary gate queue on each
        qubit that read 1 — an index flip deferred to, or folded into, the next pass; nothing is launched for it here.  Returns the
        outcome that was measured."""
        qs = [int(q) for q in qubits]
        outcome = self.measure(qs, seed=seed, draw=draw)
        for j, q in enumerate(qs):
            if (outcome >> j) & 1:
                self.apply_1q(gate_matrix("x"), q)
        return outcome

    def apply_channel(self, kraus, targets, *, seed=None, draw=None, return_probability: bool = False):
        """One quantum-trajectory step of the channel rho -> sum_i K_i rho K_i^dagger on `targets` (at most 5; bit j of a matrix index
        is targets[j]; channels.py has the usual lists): operator i is picked with probability p_i = Tr(K_i rho_A K_i^dagger) / Tr rho_A
        from reduced_density_matrix(targets) — by the draw against the running sum, lowest index first, never one of probability zero —
        and the state becomes K_i |psi> / sqrt(p_i Tr rho_A), norm 1, through apply_matrix.  Returns i, with
        return_probability=True (i, p_i).  Averaged over the draws the states reproduce the channel.  ValueError for a list that is not trace-preserving (channels.TRACE_TOLERANCE)."""
        ts = [int(q) for q in targets]
        if len(ts) > 5:
            raise ValueError(f"apply_channel: at most 5 targets, got {len(ts)}")
        ks = channels.as_kraus_list(kraus, len(ts))
        u = self._one_draw("apply_channel", seed, draw)
        if not 0.0 <= u <= 1.0:
            raise ValueError(f"apply_channel: the draw is {u!r}, not a number in [0, 1]")
        rho = self.reduced_density_matrix(ts)
        total = float(np.real(np.trace(rho)))
        if not (total > 0.0 and np.isfinite(total)):
            raise ValueError(f"apply_channel: the state's total probability is {total!r}, nothing to draw from")
        p = channels.probabilities(ks, rho)
        i = channels.pick(p, u)
        self.apply_matrix(ks[i] / np.sqrt(p[i] * total), ts)
        return (i, float(p[i])) if return_probability else i

    def norm2(self) -> float:
        v = c_double()
        check(_lib.load().qsim_norm2(self._h, byref(v)))
        return v.value

    @property
    def device_ptr(self) -> int:
        return int(_lib.load().qsim_device_ptr(self._h) or 0)

    @property
    def stream(self) -> int:
        return int(_lib.load().qsim_stream(self._h) or 0)

    # -- stats
    def stats(self) -> dict:
        st = QsimStats()
        check(_lib.load().qsim_get_stats(self._h, byref(st)))
        return st.as_dict()

    def launch_log(self) -> list:
        """[(kernel, n_ops, high_mask, ms)] per launch since reset_stats (profile mode)."""
        lib = _lib.load()
        n = lib.qsim_launch_log(self._h, -1, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            k, o, hm, ms = c_int(), c_int(), c_uint64(), c_double()
            lib.qsim_launch_log(self._h, i, byref(k), byref(o), byref(hm), byref(ms))
            out.append((_lib.K_NAMES[k.value], o.value, hm.value, ms.value))
        return out

    def launch_log_orders(self) -> list:
        """Per launch since reset_stats: the tile pass's high tile bits in tile-local order ([] for other kernels)."""
        lib = _lib.load()
        n = lib.qsim_launch_log(self._h, -1, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            order, cnt = (c_int * 10)(), c_int()
            check(lib.qsim_launch_log_order(self._h, i, order, byref(cnt)))
            out.append([order[j] for j in range(cnt.value)])
        return out

    def launch_log_blocks(self) -> list:
        """Per launch since reset_stats: [(entries_per_row, tile_qubits, mostly_identity, selector_qubits)] of a tile pass's blocks
        ([] for other kernels) — qsim_launch_log_blocks, the data behind the pass-time model."""
        lib = _lib.load()
        n = lib.qsim_launch_log(self._h, -1, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            codes, cnt = (c_ubyte * 64)(), c_int()
            check(lib.qsim_launch_log_blocks(self._h, i, codes, 64, byref(cnt)))
            out.append([(1 << (codes[j] & 3), (codes[j] >> 2) & 7, bool(codes[j] & 32), codes[j] >> 6) for j in range(min(cnt.value, 64))])
        return out

    def launch_log_block_flags(self) -> list:
        """Per launch since reset_stats: [(nq, terms, nsel, flags, info)] of a tile pass's blocks ([] for other kernels), read from
        the headers of the records the kernel was given — nq after padding, entries per row, selector qubits, TileOp::flags and
        b[7] (qsim_launch_log_block_flags; profile = 2)."""
        lib = _lib.load()
        n = lib.qsim_launch_log(self._h, -1, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            codes, cnt = (c_ubyte * (5 * 64))(), c_int()
            check(lib.qsim_launch_log_block_flags(self._h, i, codes, 64, byref(cnt)))
            out.append([tuple(codes[5 * j + k] for k in range(5)) for j in range(min(cnt.value, 64))])
        return out

    def reset_stats(self) -> None:
        check(_lib.load().qsim_reset_stats(self._h))


def run_qasm(path: str, device: int = 0, **sim_options) -> np.ndarray:
    """QASM file in, amplitude vector out (the drop-in path of BASELINE.json's north_star)."""
    c = Circuit.from_file(path)
    with Simulator(c.num_qubits, device, **sim_options) as sim:
        sim.run(c)
        return sim.read()
