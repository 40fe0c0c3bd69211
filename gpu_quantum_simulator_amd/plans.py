"""Every host-only probe of the library, once: the `qsim_*_plan` calls, the two geometry calls, the two `*_operand` calls, the limits
and the process-wide sweep counters.  Nothing here touches a qsim_state or a device.

A probe is a plain function named after its C symbol without the `qsim_` prefix.  Its inputs come in the header's order: qubit
lists are Python lists, masks Python ints, precision 64 or 32.  A list may be None, which passes NULL, and the count that follows a
list in the header is a keyword of the header's name (`k=`, `num_controls=`, `num_terms=` ...) that defaults to the list's length.
The result is `(rc, fields)`: `fields` is a dict keyed by the header's out-parameter names, signed fields preset to -1 and unsigned
ones to 0, so a refused probe that wrote nothing shows its presets.  `ok((rc, fields))` raises for rc != 0 and returns the fields."""
from __future__ import annotations

import ctypes
import inspect
from ctypes import byref, c_double, c_int, c_long, c_ubyte, c_uint16, c_uint32, c_uint64

import numpy as np

from . import _lib, _marshal

QFT_MAX_PASSES = 40  # the arrays qsim_apply_qft_plan fills have 40 entries each (include/qsim_qft.h)

_SCALARS = {"int": c_int, "long": c_long, "u64": c_uint64, "double": c_double}
_PRESET = {"int": -1, "long": -1, "u64": 0, "double": -1.0}

# symbol -> (inputs, outputs), both in the header's order.
#   inputs:  "ints:NAME" a qubit list, "masks:NAME" a list of uint64 masks, "bytes:NAME" a list of 0/1 flags (each None -> NULL);
#            "len:NAME:LIST" the count of LIST (keyword, defaults to len(LIST)); "int:NAME" / "long:NAME" / "u64:NAME" scalars.
#   outputs: "int:NAME" / "long:NAME" / "u64:NAME" / "double:NAME" scalars; "int[]:NAME" / "u64[]:NAME" arrays of QFT_MAX_PASSES,
#            returned as lists trimmed to the field "passes".
_PROBES = {
    "qsim_pauli_sweeps": ("masks:x_masks len:num_terms:x_masks", "long:sweeps"),
    "qsim_pauli_rotation_plan": ("masks:x_masks masks:z_masks len:num_terms:x_masks", "long:sweeps long:queued_as_gates"),
    "qsim_controlled_rotation_plan": ("masks:c_masks masks:x_masks masks:z_masks len:num_terms:x_masks int:num_q int:precision_bits",
                                      "long:sweeps long:queued_as_gates u64:units_visited"),
    "qsim_pauli_gradient_plan": ("masks:rot_x len:num_rot:rot_x masks:ham_x len:num_ham:ham_x", "long:adjoint_sweeps long:sum_sweeps"),
    "qsim_controlled_gradient_plan": ("masks:rot_c masks:rot_x len:num_rot:rot_x masks:ham_x len:num_ham:ham_x int:num_q int:precision_bits",
                                      "long:adjoint_sweeps long:sum_sweeps u64:units_visited"),
    "qsim_lanczos_plan": ("masks:ham_x len:num_ham:ham_x int:max_steps int:want_vector",
                          "long:sum_sweeps_per_step long:other_sweeps_per_step double:volumes_per_step"),
    "qsim_reduced_density_plan": ("ints:qubits len:k:qubits int:num_q int:precision_bits",
                                  "int:path int:padded_k u64:kernel_mask u64:units_visited long:trips_per_workgroup_at_grid_cap"),
    "qsim_subsystem_density_plan": ("ints:qubits len:k:qubits int:num_q int:precision_bits",
                                    "int:path int:block_rows long:upper_blocks long:slices u64:units_read u64:scratch_bytes long:trips_per_workgroup"),
    "qsim_apply_matrix_plan": ("ints:targets len:k:targets ints:controls len:num_controls:controls int:num_q int:precision_bits",
                               "int:path int:padded_k u64:kernel_mask u64:units long:trips_per_workgroup"),
    "qsim_apply_permutation_plan": ("ints:targets len:k:targets ints:controls len:num_controls:controls int:num_q int:precision_bits",
                                    "int:path int:tile_bits u64:tile_mask u64:tiles u64:units long:trips_per_workgroup"),
    "qsim_diagonal_plan": ("int:num_q int:precision_bits",
                           "u64:items int:items_per_trip_phase int:items_per_trip_expect long:trips_at_cap_phase long:trips_at_cap_expect"),
    "qsim_diagonal_gradient_plan": ("bytes:is_diag masks:step_c masks:step_x len:num_steps:step_x masks:ham_x len:num_ham:ham_x int:has_obs int:num_q "
                                    "int:precision_bits",
                                    "long:pauli_adjoint_sweeps long:diag_adjoint_sweeps long:sum_sweeps int:diag_adjoint_items_per_trip "
                                    "long:diag_adjoint_trips_at_cap"),
    "qsim_sample_geometry": ("int:n", "int:chunk_bits int:group_bits u64:scratch_bytes"),
    "qsim_apply_qft_plan": ("ints:qubits len:k:qubits int:num_q int:precision_bits int:max_digit_bits",
                            "int:passes int[]:digit_bits int[]:out_of_place u64[]:tile_mask u64:tiles u64:units long:trips_per_workgroup"),
    "qsim_collapse_plan": ("ints:qubits len:k:qubits u64:outcome int:num_q int:precision_bits",
                           "u64:weight_units u64:collapse_units long:weight_trips long:collapse_trips"),
}

LIMITS = ("pauli_terms_per_sweep", "pauli_rotations_per_sweep", "reduced_density_max_qubits", "subsystem_density_max_qubits",
          "apply_matrix_max_qubits", "apply_permutation_max_qubits", "apply_qft_max_digit_bits")
COUNTERS = ("pauli_rotation", "pauli_adjoint", "density", "subsystem", "matrix", "permutation", "diagonal", "diagonal_adjoint", "qft", "collapse")


def _list_arg(kind: str, values):
    """(what to keep alive, what to pass) for one list input; None passes NULL."""
    if values is None or kind == "masks":
        return (None, None) if values is None else _marshal.masks(values)
    arr = _marshal.ints(values) if kind == "ints" else (c_ubyte * max(len(values), 1))(*[int(v) for v in values])
    return arr, arr


def _count(values, override) -> int:
    """The count that follows a list: the caller's override, else the list's length (0 for NULL)."""
    return int(override) if override is not None else (0 if values is None else len(values))


def _probe(symbol: str):
    inputs = [spec.split(":") for spec in _PROBES[symbol][0].split()]
    outputs = [spec.split(":") for spec in _PROBES[symbol][1].split()]
    P = inspect.Parameter
    signature = inspect.Signature([P(spec[1], P.POSITIONAL_OR_KEYWORD) for spec in inputs if spec[0] != "len"]
                                  + [P(spec[1], P.KEYWORD_ONLY, default=None) for spec in inputs if spec[0] == "len"])

    def call(*args, **kwargs):
        given = signature.bind(*args, **kwargs)
        given.apply_defaults()
        given = given.arguments
        keep, c_args = [], []
        for spec in inputs:
            if spec[0] == "len":
                c_args.append(_count(given[spec[2]], given.get(spec[1])))
            elif spec[0] in _SCALARS:
                c_args.append(int(given[spec[1]]))
            else:
                alive, passed = _list_arg(spec[0], given[spec[1]])
                keep.append(alive)
                c_args.append(passed)
        slots = []
        for kind, name in outputs:
            if kind.endswith("[]"):
                slot = (_SCALARS[kind[:-2]] * QFT_MAX_PASSES)()
                c_args.append(slot)
            else:
                slot = _SCALARS[kind](_PRESET[kind])
                c_args.append(byref(slot))
            slots.append(slot)
        rc = getattr(_lib.load(), symbol)(*c_args)
        fields = {name: slot.value for (kind, name), slot in zip(outputs, slots) if not kind.endswith("[]")}
        for (kind, name), slot in zip(outputs, slots):
            if kind.endswith("[]"):
                fields[name] = list(slot[:min(max(fields["passes"], 0), QFT_MAX_PASSES)])
        return rc, {name: fields[name] for _, name in outputs}

    call.__name__ = call.__qualname__ = symbol[len("qsim_"):]
    call.__doc__ = f"{symbol}({', '.join(spec[1] for spec in inputs)}) -> (rc, {{{', '.join(name for _, name in outputs)}}})"
    call.outputs, call.__signature__ = tuple(name for _, name in outputs), signature
    return call


def _limit(name: str):
    def call() -> int:
        return int(getattr(_lib.load(), "qsim_" + name)())

    call.__name__ = call.__qualname__ = name
    call.__doc__ = f"qsim_{name}()"
    return call


PROBES = {symbol: _probe(symbol) for symbol in _PROBES}
globals().update({symbol[len("qsim_"):]: fn for symbol, fn in PROBES.items()})
globals().update({name: _limit(name) for name in LIMITS})


def ok(result) -> dict:
    """The fields of a probe's (rc, fields); QsimError where the probe refused."""
    rc, fields = result
    _lib.check(rc)
    return fields


def limits() -> dict:
    """The seven limits by name: terms and rotations per sweep, the largest qubit lists, the largest QFT digit."""
    return {name: globals()[name]() for name in LIMITS}


def sweeps_launched(kind: str) -> int:
    """The process-wide counter qsim_<kind>_sweeps_launched(); kind is one of COUNTERS."""
    if kind not in COUNTERS:
        raise ValueError(f"sweeps_launched: {kind!r} is not one of {COUNTERS}")
    return int(getattr(_lib.load(), f"qsim_{kind}_sweeps_launched")())


def apply_matrix_operand(U, targets, controls, num_q, precision_bits, *, k=None, num_controls=None):
    """qsim_apply_matrix_operand: (rc, {"M", "row_amp", "row_part", "rows"}) — M as a (rows, rows) float64 array, row_amp and row_part as
    int arrays of `rows` entries; rows = 0 (and empty arrays) on the plain path, -1 where the probe refused.  U is a (2^k, 2^k) matrix; None passes NULL."""
    flat = None if U is None else np.ascontiguousarray(np.asarray(U, dtype=np.complex128).reshape(-1)).view(np.float64)
    M = np.zeros(64 * 64)
    amp, part, rows = (c_int * 64)(), (c_int * 64)(), c_int(-1)
    rc = _lib.load().qsim_apply_matrix_operand(None if flat is None else _marshal.dp(flat), None if targets is None else _marshal.ints(targets), _count(targets, k),
                                               None if controls is None else _marshal.ints(controls), _count(controls, num_controls),
                                               num_q, precision_bits, _marshal.dp(M), amp, part, byref(rows))
    r = min(max(rows.value, 0), 64)
    return rc, {"M": M[:r * r].reshape(r, r).copy(), "row_amp": np.array(amp[:r], dtype=np.int64), "row_part": np.array(part[:r], dtype=np.int64),
                "rows": rows.value}


def apply_permutation_operand(perm, targets, controls, num_q, precision_bits, *, k=None, num_controls=None):
    """qsim_apply_permutation_operand: (rc, {"local_map", "entries"}) — the tile-local map as an int64 array of `entries` values; entries = -1
    (and an empty map) where the probe refused.  perm is a table of 2^k entries; None passes NULL."""
    table = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32)
    out, entries = (c_uint16 * 8192)(), c_int(-1)
    rc = _lib.load().qsim_apply_permutation_operand(None if table is None else table.ctypes.data_as(ctypes.POINTER(c_uint32)), None if targets is None else _marshal.ints(targets),
                                                    _count(targets, k), None if controls is None else _marshal.ints(controls),
                                                    _count(controls, num_controls), num_q, precision_bits, out, byref(entries))
    return rc, {"local_map": np.array(out[:min(max(entries.value, 0), 8192)], dtype=np.int64), "entries": entries.value}
