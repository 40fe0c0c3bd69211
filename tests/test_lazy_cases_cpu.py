"""tests/lazy_cases.py against include/qsim.h and every header it pulls in with #include "qsim_*.h": every exported function whose
first parameter is a qsim_state has exactly one entry in the table — a case that tests/test_gpu_lazy_states.py runs from every lazy start, or an exemption with its reason.  This is the check
that fails when an entry point is added without saying how it treats a state that is pending or partial."""
import os
import re

import lazy_cases
from gpu_quantum_simulator_amd import simulator

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "qsim.h")


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _abi_text(name, directory=INCLUDE, read=None, seen=None):
    """The text of header `name` followed by that of every header it pulls in with `#include "qsim_*.h"`, transitively and each file
    once: the include lines are followed, no file name is listed here.  An include line inside a comment pulls nothing in."""
    read = read or (lambda path: open(path).read())
    seen = set() if seen is None else seen
    if name in seen:
        return ""
    seen.add(name)
    text = _strip_comments(read(os.path.join(directory, name)))
    return text + "".join("\n" + _abi_text(inc, directory, read, seen) for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"(qsim_\w+\.h)"', text, flags=re.M))


def _state_entry_points(text):
    """Names of the qsim_* functions declared in `text` whose first parameter is `qsim_state *` or `const qsim_state *` (not
    `qsim_state **`: the constructors hand a state out, they are not called on one)."""
    text = _strip_comments(text)
    return set(re.findall(r"\b(qsim_\w+)\s*\(\s*(?:const\s+)?qsim_state\s*\*\s*(?!\*)\w", text))


def test_the_parser_reads_declarations_not_comments():
    text = """
    /* qsim_in_a_comment(qsim_state *s) is not a declaration */
    int qsim_create(qsim_state **out, int num_q, int device);
    int qsim_precision_bits(const qsim_state *s);
    void *qsim_stream(qsim_state *s);
    int qsim_combine(qsim_state *dst, const double d[2], qsim_state *p);
    int qsim_diagonal_gradient(qsim_state *s, long num_steps,
            const qsim_diagonal *const *step_diag);
    qsim_state *qsim_cluster_shard(qsim_cluster *c, int shard);
    int qsim_rank_comm_create(qsim_rank_comm **out, qsim_state *s, int device);
    """
    assert _state_entry_points(text) == {"qsim_precision_bits", "qsim_stream", "qsim_combine", "qsim_diagonal_gradient"}


def test_the_census_follows_the_include_lines():
    files = {
        "qsim.h": 'int qsim_norm2(const qsim_state *s, double *out);\n#include <stdint.h>\n#include "qsim_part.h"\n/* #include "qsim_commented.h" */\n#include "other.h"\n',
        "qsim_part.h": '#include "qsim.h"\n  #  include "qsim_deeper.h"\nint qsim_in_part(qsim_state *s, int k);\n',
        "qsim_deeper.h": "int qsim_in_deeper(qsim_state *s);\nint qsim_plan_only(const int *qubits, int k);\n",
        "qsim_commented.h": "int qsim_never_included(qsim_state *s);\n",
        "other.h": "int qsim_not_an_abi_header(qsim_state *s);\n",
    }
    text = _abi_text("qsim.h", "", lambda path: files[path])
    assert _state_entry_points(text) == {"qsim_norm2", "qsim_in_part", "qsim_in_deeper"}


def test_the_census_reaches_the_headers_qsim_h_pulls_in():
    with open(HEADER) as f:
        own = _state_entry_points(f.read())
    pulled = _state_entry_points(_abi_text("qsim.h")) - own
    assert {"qsim_apply_qft", "qsim_postselect", "qsim_measure"} <= pulled


def test_the_table_names_every_entry_point_and_no_other():
    declared = _state_entry_points(_abi_text("qsim.h"))
    assert len(declared) > 60  # the parser found the header's calls, not a handful of them
    table = set(lazy_cases.TABLE)
    assert not declared - table, f"entry points without a lazy-state case or exemption: {sorted(declared - table)}"
    assert not table - declared, f"stale keys, no such entry point in include/qsim.h or a header it includes: {sorted(table - declared)}"
    assert not set(lazy_cases.CASES) & set(lazy_cases.EXEMPT)


def test_every_exemption_says_why():
    for fn, entry in lazy_cases.EXEMPT.items():
        assert isinstance(entry, lazy_cases.Exempt), fn
        assert isinstance(entry.reason, str) and len(entry.reason.strip()) >= 20 and "\n" not in entry.reason, fn


def test_every_case_is_well_formed():
    names = [case.name for _, case in lazy_cases.all_cases()]
    assert len(names) == len(set(names))
    for fn, cases in lazy_cases.CASES.items():
        assert cases, fn
        for case in cases:
            assert isinstance(case, lazy_cases.Case), fn
            assert hasattr(simulator.Simulator, case.method), (fn, case.name, case.method)
            assert case.group in (lazy_cases.READ, lazy_cases.IN_PLACE, lazy_cases.INTO, lazy_cases.GRADIENT), case.name
            assert case.compare in ("bits", "ref"), case.name
            # a case leaves the bit-for-bit comparison only with the code line that queues its gates
            assert (case.compare == "ref") == bool(case.why_ref.strip()), case.name


def test_the_required_cases_are_there():
    """What the contract was written down to cover, by the method that drives it."""
    by_method = {}
    for _, case in lazy_cases.all_cases():
        by_method.setdefault(case.method, []).append(case)
    for method in ("read", "norm2", "expectation_terms", "sample", "sample_shots", "block_prob_masked", "gather_masked", "reduced_density_matrix",
                   "subsystem_density_matrix", "expectation_diagonal", "inner", "device_ptr", "write", "apply_pauli_rotations", "apply_matrix",
                   "apply_permutation", "apply_diagonal_phase", "scale", "ground_state", "pauli_sum_into", "diagonal_into", "copy_from", "combine",
                   "pack_bits", "pack_bits_to", "energy_and_gradient", "apply_qft", "postselect", "measure"):
        assert method in by_method, method
    assert by_method["read"][0].operands["first"] > 0
    assert {c.operands["qubits"] is None for c in by_method["sample_shots"]} == {True, False}
    assert any(len(c.operands["qubits"]) <= 5 for c in by_method["reduced_density_matrix"])
    assert any(6 <= len(c.operands["qubits"]) <= 10 for c in by_method["subsystem_density_matrix"])
    assert {c.operands["vector"] for c in by_method["ground_state"]} == {True, False}
    assert {c.operands["lent"] for c in by_method["energy_and_gradient"]} == {True, False}
    assert len({fn for fn, c in lazy_cases.all_cases() if c.method == "energy_and_gradient"}) == 3
    assert [c.name for _, c in lazy_cases.all_cases() if c.compare == "ref"] == ["rotations_mixed", "scale"]
    low, high = set(lazy_cases.SUPPORT_LOW), set(lazy_cases.SUPPORT_HIGH)
    for method in ("apply_matrix", "apply_permutation"):
        sets = [set(c.operands["targets"]) | set(c.operands["controls"]) for c in by_method[method]]
        tc = [(set(c.operands["targets"]), set(c.operands["controls"])) for c in by_method[method]]
        for support in (low, high):
            assert any(s <= support for s in sets), method                      # all targets and controls inside the support
            assert any(t - support and c - support for t, c in tc), method      # a target and a control outside it
        assert {c.operands["plan"] for c in by_method[method]} == {lazy_cases.PLAN_MAIN, lazy_cases.PLAN_SMALL}
    assert 14 in high and 0 not in high and len(lazy_cases.STARTS) == 4
    # the Fourier transform: one call that is a single in-place sweep and one whose sweeps move through the second buffer
    assert {c.operands["moving"] for c in by_method["apply_qft"]} == {True, False}
    for c in by_method["apply_qft"]:
        cap = c.operands["max_digit_bits"] or 10
        assert (len(c.operands["qubits"]) > cap) == c.operands["moving"], c.name
    # measurement: one qubit set inside SUPPORT_LOW, one with a qubit outside either partial support
    for method in ("postselect", "measure"):
        sets = [set(c.operands["qubits"]) for c in by_method[method]]
        assert any(s <= low for s in sets) and any(s - low and s - high for s in sets), method
    assert all(c.compare == "bits" for m in ("apply_qft", "postselect", "measure") for c in by_method[m])
