#!/usr/bin/env python3
"""Regenerates tests/golden/ from the REAL reference (container only).

Recipe: `make -C oracle ref` compiles /root/reference/quantum_simulator.c, from where it lies, into
oracle/_ref/libqsref.so (main renamed away).  This script calls its compute_state_vector()
(quantum_simulator.c:115) through ctypes on each circuit below and stores the returned amplitudes as
.npy (float64, shape [2^n, 2] = re, im) next to the circuit text.  The two reference sample circuits
are copied in as data; everything else is produced by gpu_quantum_simulator_amd.circuits with fixed
seeds.  Only inputs and expected outputs are stored here — no reference source.

Besides the circuits above it records what tests/test_oracle_golden.py and tests/test_scheduler_cpu.py compare the
oracle with, so that they need nothing outside the repository: the reference's amplitudes for the LIVE_CASES circuits,
its two kernels on a random state (kernels_n9_*), its cumulative distribution and measurement() draws on
rand_n10_all (rand_n10_all_cumulative.npy, rand_n10_all_measurement.npy) and the parser corners (parser_*).

Tests read the committed files and never call this script.
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from gpu_quantum_simulator_amd import circuits  # noqa: E402

REFERENCE = os.environ.get("REFERENCE", "/root/reference")

# name, n, depth, seed, vocabulary, text options
RANDOM_CASES = [
    ("rand_n3_all_lf", 3, 60, 11, "all", {}),
    ("rand_n5_all_crlf_physical", 5, 120, 12, "all", {"crlf": True, "physical": True}),
    ("rand_n8_all_suffix", 8, 200, 13, "all", {"qubit_style": "suffix"}),
    ("rand_n9_clifford_t", 9, 300, 14, "clifford_t", {"crlf": True}),
    ("rand_n10_all", 10, 400, 15, "all", {}),
    ("rand_n12_all", 12, 500, 16, "all", {}),
    ("rand_n12_clifford_t_physical", 12, 500, 17, "clifford_t", {"physical": True}),
]


# the oracle-vs-reference circuits of test_oracle_equals_live_reference: name, n, seed, text options (150 gates, "all")
LIVE_CASES = [
    ("live_n4_seed101", 4, 101, {}),
    ("live_n7_seed102", 7, 102, {"crlf": True}),
    ("live_n11_seed103", 11, 103, {"physical": True}),
    ("live_n13_seed104", 13, 104, {"qubit_style": "suffix"}),
]
PARSER_HEADER = 'OPENQASM 3.0;\ninclude "stdgates.inc";\n'
# the parser corners of test_parser_corners_pinned_to_the_oracle: name, text (None as the reference's answer = rejected)
PARSER_CASES = [
    ("parser_qubit_twice", PARSER_HEADER + "qubit[3] q;\nh q[0];\ncx q[0], q[2];\nqubit[2] q;\nx q[1];\nh q[0];\n"),
    ("parser_qubit_last", PARSER_HEADER + "qubit[3] q;"),
    ("parser_qubit_last_newline", PARSER_HEADER + "qubit[3] q;\n"),
]


def record_reference_calls(lib, run_reference, manifest):
    """The reference's kernels and measurement path called directly, and its answers on the parser corners."""
    dp = ctypes.POINTER(ctypes.c_double)
    lib.execute_single_qubit_gate.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int]
    lib.execute_cnot.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    rng = np.random.default_rng(5)
    n = 9
    state = (rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)).astype(np.complex128)
    U = (rng.standard_normal(4) + 1j * rng.standard_normal(4)).astype(np.complex128)  # NOT symmetric
    np.save(os.path.join(HERE, "kernels_n9_state.npy"), state.view(np.float64).reshape(-1, 2))
    np.save(os.path.join(HERE, "kernels_n9_matrix.npy"), U.view(np.float64).reshape(-1, 2))
    for q in range(n):
        lib.execute_single_qubit_gate(state.view(np.float64).ctypes.data_as(dp), n, U.view(np.float64).ctypes.data_as(dp), q)
        lib.execute_cnot(state.view(np.float64).ctypes.data_as(dp), n, q, (q + 3) % n)
    np.save(os.path.join(HERE, "kernels_n9_out.npy"), state.view(np.float64).reshape(-1, 2))
    manifest["kernels_n9"] = {"n": n, "source": "execute_single_qubit_gate(matrix, q) then execute_cnot(q, (q + 3) % 9) for q = 0..8 "
                                                "on kernels_n9_state.npy"}

    lib.compute_state_cumulative_distribution.argtypes = [dp, ctypes.c_int]
    lib.compute_state_cumulative_distribution.restype = ctypes.c_void_p
    lib.measurement.argtypes = [dp, ctypes.c_int]
    lib.measurement.restype = ctypes.c_longlong
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    n, amps = run_reference(os.path.join(HERE, "rand_n10_all.qasm"))
    p = lib.compute_state_cumulative_distribution(np.ascontiguousarray(amps).ctypes.data_as(dp), n)
    cumul = np.ctypeslib.as_array(ctypes.cast(p, dp), shape=(1 << n,)).copy()
    libc.free(p)
    draws = []
    for seed in range(1, 40):
        libc.srand(seed)
        draws.append(lib.measurement(cumul.ctypes.data_as(dp), n))
    np.save(os.path.join(HERE, "rand_n10_all_cumulative.npy"), cumul)
    np.save(os.path.join(HERE, "rand_n10_all_measurement.npy"), np.array(draws, dtype=np.int64))
    manifest["rand_n10_all_measurement"] = {"n": n, "source": "compute_state_cumulative_distribution of rand_n10_all, then "
                                                                 "measurement() after srand(seed) for seed = 1..39"}

    for name, text in PARSER_CASES:
        path = os.path.join(HERE, name + ".qasm")
        with open(path, "w", newline="") as f:
            f.write(text)
        try:
            rn, amps = run_reference(path)
        except RuntimeError:
            manifest[name] = {"rejected": True}
            continue
        np.save(os.path.join(HERE, name + ".npy"), amps)
        manifest[name] = {"n": rn}


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libqsref.so"))
    lib.compute_state_vector.restype = ctypes.c_void_p
    lib.compute_state_vector.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]

    def run_reference(path):
        n = ctypes.c_int(0)
        p = lib.compute_state_vector(path.encode(), ctypes.byref(n))
        if not p:
            raise RuntimeError(f"reference rejected {path}")
        a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), shape=((1 << n.value), 2)).copy()
        libc.free(p)
        return n.value, a

    manifest = {}
    for name in ("entanglement", "grover_3_18"):
        dst = os.path.join(HERE, name + ".qasm")
        shutil.copyfile(os.path.join(REFERENCE, name + ".qasm"), dst)
        n, amps = run_reference(dst)
        np.save(os.path.join(HERE, name + ".npy"), amps)
        manifest[name] = {"n": n, "source": "reference sample circuit (data file)"}

    # grover_3_18 with the register widened to 18 qubits: gates touch q0..q5 only, so only
    # the first 64 amplitudes are non-zero; store those plus the exact-zero count.
    wide = os.path.join(HERE, "grover_3_18_n18.qasm")
    with open(os.path.join(REFERENCE, "grover_3_18.qasm"), newline="") as f:
        text = f.read().replace("qubit[6] q;", "qubit[18] q;")
    with open(wide, "w", newline="") as f:
        f.write(text)
    n, amps = run_reference(wide)
    assert n == 18 and not amps[64:].any()
    np.save(os.path.join(HERE, "grover_3_18_n18.first64.npy"), amps[:64])
    manifest["grover_3_18_n18"] = {"n": 18, "stored": "first 64 amplitudes; all others are exactly 0",
                                   "source": "grover_3_18.qasm with line 3 rewritten to qubit[18] q;"}

    for name, n, depth, seed, vocab, opts in RANDOM_CASES:
        path = os.path.join(HERE, name + ".qasm")
        circuits.random_circuit_file(path, n, depth, seed, vocab, **opts)
        rn, amps = run_reference(path)
        assert rn == n
        np.save(os.path.join(HERE, name + ".npy"), amps)
        manifest[name] = {"n": n, "depth": depth, "seed": seed, "vocabulary": vocab, "text": opts}

    for name, n, seed, opts in LIVE_CASES:
        path = os.path.join(HERE, name + ".qasm")
        circuits.random_circuit_file(path, n, 150, seed, "all", **opts)
        rn, amps = run_reference(path)
        assert rn == n
        np.save(os.path.join(HERE, name + ".npy"), amps)
        manifest[name] = {"n": n, "depth": 150, "seed": seed, "vocabulary": "all", "text": opts}

    record_reference_calls(lib, run_reference, manifest)

    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("golden fixtures written:", ", ".join(sorted(manifest)))


if __name__ == "__main__":
    main()
