"""gpu_quantum_simulator_amd.plans, the package's one home for the host-only probes: a census against _lib's signature tables, the
keys of every returned dict against the out-parameter names the headers under include/ declare, one refusal per probe that leaves
the presets standing, and one success per probe at a small register, held against the numpy model where a *_ref.py has one.
Needs the built library, no device; milliseconds."""
import os
import re

import numpy as np
import pytest

import density_ref
import subsystem_ref
from gpu_quantum_simulator_amd import _lib, plans

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
OPERANDS = {"qsim_apply_matrix_operand": plans.apply_matrix_operand, "qsim_apply_permutation_operand": plans.apply_permutation_operand}
# qsim_cluster_plan is no probe: it takes a cluster handle and plans (and may time) every shard's local steps on the devices — Cluster.plan.
EXEMPT = {"qsim_cluster_plan"}


def _probe_symbols():
    names = {**_lib.SIGNATURES, **_lib.QFT_SIGNATURES, **_lib.MEASURE_SIGNATURES}
    return sorted(s for s in names if s not in EXEMPT and (re.search(r"(_plan|_operand|_sweeps_launched|_per_sweep)$", s) or "_max_" in s
                                                          or s in ("qsim_pauli_sweeps", "qsim_sample_geometry")))


def _header_out_params():
    """symbol -> the names of its non-const pointer parameters, in order, from the prototypes under include/."""
    out = {}
    for header in ("qsim.h", "qsim_qft.h", "qsim_measure.h"):
        with open(os.path.join(INCLUDE, header)) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        for m in re.finditer(r"^\s*(?:int|long|uint64_t)\s+(qsim_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.M | re.S):
            params = [" ".join(p.split()) for p in m.group(2).split(",")]
            out[m.group(1)] = [re.search(r"(\w+)$", p).group(1) for p in params if "*" in p and not p.startswith("const ")]
    return out


# One refused and one accepted call per probe: symbol -> (refusal args, refusal keywords, success args).
H = [0b0011, 0b0000, 0b0100]  # x masks of a small Hamiltonian
CALLS = {
    "qsim_pauli_sweeps": ((None,), dict(num_terms=2), (H,)),
    "qsim_pauli_rotation_plan": ((None, None), dict(num_terms=2), (H, [0, 5, 0])),
    "qsim_controlled_rotation_plan": (([0, 8, 8], H, [0, 5, 0], 41, 64), {}, ([0, 8, 8], H, [0, 5, 0], 10, 64)),
    "qsim_pauli_gradient_plan": ((None, H), dict(num_rot=2), (H, H)),
    "qsim_controlled_gradient_plan": (([0, 8, 8], H, H, 41, 64), {}, ([0, 8, 8], H, H, 10, 32)),
    "qsim_lanczos_plan": ((None, 10, 1), dict(num_ham=3), (H, 10, 1)),
    "qsim_reduced_density_plan": (([3, 3], 10, 64), {}, ([7, 0, 3], 10, 64)),
    "qsim_subsystem_density_plan": ((None, 12, 64), dict(k=2), ([9, 1, 4, 0, 6, 2, 11], 12, 32)),
    "qsim_apply_matrix_plan": (([2, 5, 2], [], 10, 64), {}, ([5, 2, 8], [0], 10, 32)),
    "qsim_apply_permutation_plan": (([1, 2], [2], 10, 64), {}, ([1, 2, 7], [4], 10, 64)),
    "qsim_diagonal_plan": ((41, 64), {}, (10, 32)),
    "qsim_diagonal_gradient_plan": (([1, 0], [0, 0], [0, 1], H, 1, 41, 64), {}, ([1, 0], [0, 0], [0, 1], H, 1, 10, 64)),
    "qsim_sample_geometry": ((-1,), {}, (12,)),
    "qsim_apply_qft_plan": (([4, 4], 10, 64, 0), {}, ([0, 9, 3, 4, 1, 2, 5], 10, 64, 3)),
    "qsim_collapse_plan": (([1, 1], 0, 10, 64), {}, ([1, 8], 2, 10, 32)),
}


def test_census_every_probe_symbol_has_exactly_one_entry():
    symbols = _probe_symbols()
    assert set(CALLS) == set(plans.PROBES)                       # every probe has its refused and its accepted call below
    assert len(symbols) == 15 + 2 + 7 + 10 and "qsim_cluster_plan" not in symbols
    for s in symbols:
        homes = [s in plans.PROBES, s in OPERANDS, s[5:] in plans.LIMITS, s.endswith("_sweeps_launched") and s[5:-len("_sweeps_launched")] in plans.COUNTERS]
        assert sum(homes) == 1, s
        if homes[0] or homes[1] or homes[2]:
            assert callable(getattr(plans, s[5:])), s
    # and nothing in plans names a symbol the tables do not have
    assert set(plans.PROBES) | set(OPERANDS) | {"qsim_" + n for n in plans.LIMITS} | {f"qsim_{k}_sweeps_launched" for k in plans.COUNTERS} == set(symbols)
    assert len(set(plans.LIMITS)) == len(plans.LIMITS) and len(set(plans.COUNTERS)) == len(plans.COUNTERS)
    assert plans.limits() == {name: getattr(_lib.load(), "qsim_" + name)() for name in plans.LIMITS}
    for kind in plans.COUNTERS:
        assert plans.sweeps_launched(kind) == getattr(_lib.load(), f"qsim_{kind}_sweeps_launched")()
    with pytest.raises(ValueError):
        plans.sweeps_launched("cluster")


@pytest.mark.parametrize("symbol", sorted(CALLS))
def test_dict_keys_are_the_headers_out_parameter_names(symbol):
    fn = plans.PROBES[symbol]
    assert fn is getattr(plans, symbol[5:]) and fn.__name__ == symbol[5:]
    want = _header_out_params()[symbol]
    for args, kwargs in (CALLS[symbol][:2], (CALLS[symbol][2], {})):
        rc, fields = fn(*args, **kwargs)
        assert list(fields) == want == list(fn.outputs), symbol
    # one output slot per out-parameter, and inputs + outputs fill the signature _lib declares
    argtypes = {**_lib.SIGNATURES, **_lib.QFT_SIGNATURES, **_lib.MEASURE_SIGNATURES}[symbol][1]
    assert len(argtypes) == len(want) + len(plans._PROBES[symbol][0].split())


def test_operand_dict_keys_are_the_headers_out_parameter_names():
    outs = _header_out_params()
    rc, fields = plans.apply_matrix_operand(np.eye(8), [5, 2, 8], [0], 10, 64)
    assert rc == _lib.QSIM_OK and list(fields) == outs["qsim_apply_matrix_operand"]
    r = fields["rows"]
    assert r == 16 and fields["M"].shape == (r, r) and len(fields["row_amp"]) == len(fields["row_part"]) == r
    rc, fields = plans.apply_permutation_operand([1, 0, 3, 2], [3, 7], [1], 10, 64)
    assert rc == _lib.QSIM_OK and list(fields) == outs["qsim_apply_permutation_operand"]
    assert fields["entries"] == len(fields["local_map"]) == 1 << plans.ok(plans.apply_permutation_plan([3, 7], [1], 10, 64))["tile_bits"]
    assert sorted(fields["local_map"]) == list(range(fields["entries"]))
    # refused: a repeated target; nothing is reported
    rc, fields = plans.apply_matrix_operand(np.eye(4), [2, 2], [], 10, 64)
    assert rc == _lib.ERR_ARG and fields["rows"] == -1 and fields["M"].size == 0
    rc, fields = plans.apply_permutation_operand([0, 1, 2, 3], [2, 2], [], 10, 64)
    assert rc == _lib.ERR_ARG and fields["entries"] == -1 and fields["local_map"].size == 0


@pytest.mark.parametrize("symbol", sorted(CALLS))
def test_a_refused_probe_leaves_the_presets(symbol):
    args, kwargs, _ = CALLS[symbol]
    rc, fields = plans.PROBES[symbol](*args, **kwargs)
    assert rc == _lib.ERR_ARG, (symbol, rc)
    kinds = dict(reversed(spec.split(":")) for spec in plans._PROBES[symbol][1].split())
    for name, value in fields.items():
        want = [] if kinds[name].endswith("[]") else plans._PRESET[kinds[name]]
        assert value == want and type(value) is type(want), (symbol, name, value)
    with pytest.raises(_lib.QsimError):
        plans.ok((rc, fields))


@pytest.mark.parametrize("symbol", sorted(CALLS))
def test_an_accepted_probe_fills_every_field(symbol):
    rc, fields = plans.PROBES[symbol](*CALLS[symbol][2])
    assert rc == _lib.QSIM_OK, symbol
    assert plans.ok((rc, fields)) is fields
    kinds = dict(reversed(spec.split(":")) for spec in plans._PROBES[symbol][1].split())
    for name, value in fields.items():
        if kinds[name] in ("int", "long", "double"):
            assert value >= 0, (symbol, name)                     # the signed presets are gone
    if symbol == "qsim_apply_qft_plan":
        p = fields["passes"]
        assert p == 3 and sum(fields["digit_bits"]) == 7 and max(fields["digit_bits"]) <= 3
        assert len(fields["digit_bits"]) == len(fields["out_of_place"]) == len(fields["tile_mask"]) == p


def test_list_arguments_none_counts_and_keywords():
    full = plans.apply_matrix_plan([5, 2, 8], [0], 10, 64)
    assert full[0] == _lib.QSIM_OK
    assert plans.apply_matrix_plan(targets=[5, 2, 8], controls=[0], num_q=10, precision_bits=64) == full
    assert plans.apply_matrix_plan([5, 2, 8, 1], [0, 3], 10, 64, k=3, num_controls=1) == full       # the counts rule, not the lists
    assert plans.apply_matrix_plan([5, 2, 8], None, 10, 64)[0] == _lib.QSIM_OK                      # no controls: NULL with count 0
    assert plans.apply_matrix_plan([5, 2, 8], None, 10, 64, num_controls=1)[0] == _lib.ERR_ARG
    assert plans.apply_matrix_plan(None, [0], 10, 64, k=1)[0] == _lib.ERR_ARG
    for bad in (lambda: plans.apply_matrix_plan([1], [0], 10), lambda: plans.apply_matrix_plan([1], [0], 10, 64, 3),
                lambda: plans.apply_matrix_plan([1], [0], 10, 64, units=3), lambda: plans.apply_matrix_plan([1], [0], 10, 64, targets=[2])):
        with pytest.raises(TypeError):
            bad()


@pytest.mark.parametrize("bits", [64, 32])
def test_density_plans_agree_with_the_numpy_models(bits):
    f32 = bits == 32
    for qubits, n in (([7, 0, 3], 10), ([2], 12), ([1, 2, 3, 4, 5], 6), ([], 4)):
        got, want = plans.ok(plans.reduced_density_plan(qubits, n, bits)), density_ref.plan(qubits, n, f32)
        assert (got["path"], got["padded_k"], got["kernel_mask"], got["units_visited"], got["trips_per_workgroup_at_grid_cap"]) == \
            (want["path"], want["padded_k"], want["mask"], want["units"], want["trips"]), (qubits, n)
    for qubits, n in (([9, 1, 4, 0, 6, 2, 11], 12), ([0, 1, 2, 3, 4, 5], 7), ([3, 1], 9), (list(range(10)), 12)):
        got, want = plans.ok(plans.subsystem_density_plan(qubits, n, bits)), subsystem_ref.plan(qubits, n, f32)
        assert (got["path"], got["block_rows"], got["upper_blocks"], got["slices"], got["units_read"], got["scratch_bytes"], got["trips_per_workgroup"]) == \
            (want["path"], want["block_rows"], want["upper_blocks"], want["slices"], want["units_read"], want["scratch_bytes"], want["trips"]), (qubits, n)
    assert density_ref.plan([3, 3], 10, f32) is None and subsystem_ref.plan([3, 3], 10, f32) is None
    assert plans.reduced_density_plan([3, 3], 10, bits)[0] == plans.subsystem_density_plan([3, 3], 10, bits)[0] == _lib.ERR_ARG
