"""The per-state sweep scratch (qsim_state's d_expect; csrc/pauli.cpp owns it, csrc/pauli_sweep.h has its layout) works whoever
touches it first: expectation values (partial sums and more than one batch of result rows), qsim_apply_matrix (its operand lies
where the partial sums lie), qsim_inner and qsim_lanczos_ground each come first once, on a fresh state, and the others follow.

fp64, n = 10: the allocation does not depend on the precision.  The checkers are tests/pauli_ref.py and tests/matrix_ref.py on the
amplitudes READ BACK from the same state, within 1e-10 absolute, the project's parity tolerance (tests/test_gpu_expectation.py and
tests/test_gpu_matrix.py say why that holds for a sweep of 2^10 amplitudes); a stale or overwritten part of the scratch shows at
1e-2 or above.  Every case runs in a child process of its own under `timeout -k 10 60`, which saves what the device returned; the
assertions are made here, and after a case that failed no further one is started.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import matrix_ref
import pauli_ref
from helpers import random_unitary
from pauli_rot_ref import ising_terms, rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
N = 10
STRINGS = 130  # as many distinct x masks: 130 sweeps, two more than one batch of result rows, so the second batch reuses row 0
TARGETS, CONTROLS = [9, 0, 5, 2, 7], [3]  # five targets: the full operand of 4096 doubles
CASES = ("expectation_first", "matrix_first", "inner_first", "lanczos_first")


def _masks():
    rng = np.random.default_rng(130)
    return [(x, int(rng.integers(0, 1 << N))) for x in range(1, STRINGS + 1)]


def _unitary():
    return random_unitary(32, np.random.default_rng(32))


# ---- the child: the calls of one case on a fresh Simulator, everything the device returned into an .npz -------------------------
def _child(case, out):
    from gpu_quantum_simulator_amd import Simulator
    texts = [pauli_ref.masks_to_text(x, z, N) for x, z in _masks()]
    got = {}
    with Simulator(N) as sim, Simulator(N) as other:
        sim.write(rand_state(N, 21))
        other.write(rand_state(N, 22))

        def expectation(tag):
            got[f"state_{tag}"] = sim.read()
            got[f"expect_{tag}"] = sim.expectation_terms(texts)

        def matrix():
            sim.apply_matrix(_unitary(), TARGETS, CONTROLS)
            got["state_after_matrix"] = sim.read()

        def inner(tag):
            got[f"state_{tag}"] = sim.read()
            got[f"inner_{tag}"] = np.array([sim.inner(other)])

        if case == "expectation_first":
            expectation("first"), matrix(), expectation("after_matrix")
        elif case == "matrix_first":
            got["state_first"] = sim.read()
            matrix(), expectation("after_matrix")
        elif case == "inner_first":
            inner("first"), expectation("second"), matrix(), inner("after_matrix")
        elif case == "lanczos_first":
            got["lanczos_steps"] = np.array([sim.ground_state(ising_terms(N), tol=0.0, max_steps=2)["steps"]])
            expectation("after_lanczos")
        else:
            raise SystemExit(f"no case {case}")
        got["other"] = other.read()
    np.savez(out, **got)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ---- the parent: never opens the GPU ------------------------------------------------------------------------------------------------
_failed = []


@pytest.fixture(scope="module")
def run_case(tmp_path_factory):
    directory = tmp_path_factory.mktemp("sweep_scratch")

    @functools.lru_cache(maxsize=None)
    def run(case):
        if _failed:
            pytest.fail(f"not started: case {_failed[0]} failed before")
        out = str(directory / f"{case}.npz")
        p = subprocess.run(["timeout", "-k", "10", "60", sys.executable, os.path.abspath(__file__), case, out], capture_output=True, text=True)
        if p.returncode != 0:
            _failed.append(case)
            pytest.fail(f"case {case}: exit status {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
        with np.load(out) as f:
            return {key: f[key] for key in f.files}

    return run


def _check_expectation(got, tag):
    want = np.array([pauli_ref.pauli_expectation(got[f"state_{tag}"], x, z) for x, z in _masks()])
    worst = float(np.max(np.abs(got[f"expect_{tag}"] - want)))
    print(f"expectation {tag}: max abs err {worst:.3e}")
    assert got[f"expect_{tag}"].shape == (STRINGS,) and worst < TOL


def _check_matrix(got, before):
    want = matrix_ref.apply_matrix(got[f"state_{before}"], _unitary(), TARGETS, CONTROLS)
    worst = float(np.max(np.abs(got["state_after_matrix"] - want)))
    print(f"matrix after {before}: max abs err {worst:.3e}")
    assert worst < TOL


def _check_inner(got, tag):
    err = abs(complex(got[f"inner_{tag}"][0]) - np.vdot(got[f"state_{tag}"], got["other"]))
    print(f"inner {tag}: abs err {err:.3e}")
    assert err < TOL


def test_the_calls_are_what_they_are_meant_to_be():
    """Host only: 130 sweeps for the strings, and the matrix call takes the matrix path on five kernel qubits."""
    from gpu_quantum_simulator_amd import plans
    assert plans.ok(plans.pauli_sweeps([x for x, _ in _masks()]))["sweeps"] == STRINGS > 128
    plan = plans.ok(plans.apply_matrix_plan(TARGETS, CONTROLS, N, 64))
    assert (plan["path"], plan["padded_k"]) == (1, 5)


def test_expectation_first(run_case):
    got = run_case("expectation_first")
    _check_expectation(got, "first")
    _check_matrix(got, "first")
    _check_expectation(got, "after_matrix")


def test_matrix_first(run_case):
    got = run_case("matrix_first")
    _check_matrix(got, "first")
    _check_expectation(got, "after_matrix")


def test_inner_first(run_case):
    got = run_case("inner_first")
    _check_inner(got, "first")
    _check_expectation(got, "second")
    _check_matrix(got, "second")
    _check_inner(got, "after_matrix")


def test_lanczos_first(run_case):
    got = run_case("lanczos_first")
    assert got["lanczos_steps"][0] == 2
    _check_expectation(got, "after_lanczos")


def test_equal_calls_give_equal_bits_whoever_allocated(run_case):
    """The same matrix on the same state, then the same strings: the scratch was allocated by the expectation call in one case
    and by the matrix call in the other, and neither the state nor the sums may differ in one bit."""
    a, b = run_case("expectation_first"), run_case("matrix_first")
    assert np.array_equal(a["state_after_matrix"].view(np.uint64), b["state_after_matrix"].view(np.uint64))
    assert np.array_equal(a["expect_after_matrix"].view(np.uint64), b["expect_after_matrix"].view(np.uint64))
