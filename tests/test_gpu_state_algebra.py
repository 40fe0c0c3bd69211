"""Calls that take more than one state, on the device: Simulator.copy_from, inner and combine (qsim_copy_state, qsim_inner,
qsim_combine; csrc/combine.hip, csrc/state_algebra.cpp).

The checker is numpy on the amplitudes READ BACK before the call — for an fp32 state `read()` is the exact widened contents, so
the rounding of a write cancels.  Unit-norm states, coefficients of modulus <= 1.
fp64: max abs error < 1e-10, the project's parity tolerance (rounding stays near 1e-16 per amplitude; a wrong stream, sign or
coefficient shows at 1e-1).
fp32: fp32_ref.check_fp32(got, want64, ref32) with ref32 the same expression evaluated in complex64.
norm2 (both precisions) against the fp64 norm of the state read back AFTER the call, < 1e-10: the kernel sums exactly formed
products of the stored values in fp64 (a product of two floats is exact in fp64), so only the order of 2^n additions of
non-negative terms differs — the argument of tests/test_gpu_expectation.py.  The same holds for inner products.
Sizes: n = 0 (one amplitude: 8 bytes in fp32, no 16-byte unit), 1, 2, 9, and n = 22 (fp64) / 23 (fp32), where the 2^22 units
exceed kExpectGrid * kTPB * 8 = 2^21, so every workgroup walks its loop more than once whatever units-per-trip a shape has."""
import numpy as np
import pytest

import fp32_ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
D, A, B = 0.3 - 0.5j, -0.6 + 0.2j, 0.1 + 0.7j
SHAPES = ["three", "two", "d0_two", "d0_one"]  # sources in: dst + p + q, dst + p, p + q (dst not read), p alone (the scaled copy)


def _loop_n(precision):
    return 22 if precision == 64 else 23


def _bits(sim):
    return sim.read().view(np.uint64).copy()


def _want(shape, x, p, q, dtype):
    """The expression of `shape` in `dtype`: coefficients rounded once, multiply-adds in dtype."""
    c = dtype
    x, p, q = x.astype(c), p.astype(c), q.astype(c)
    d, a, b = c(D), c(A), c(B)
    if shape == "three":
        return (d * x + a * p + b * q).astype(c)
    if shape == "two":
        return (d * x + a * p).astype(c)
    if shape == "d0_two":
        return (a * p + b * q).astype(c)
    return (a * p).astype(c)


def _call(shape, dst, p, q, norm=True):
    d = 0 if shape.startswith("d0") else D
    return dst.combine(d, (A, p), (B, q) if shape in ("three", "d0_two") else None, norm=norm)


def _check(precision, shape, got, norm2, x, p, q, label):
    want = _want(shape, x, p, q, np.complex128)
    after = float(np.vdot(got, got).real)
    print(f"{label} {shape} p{precision}: max abs err {np.max(np.abs(got - want)):.3e}, norm2 err {abs(norm2 - after):.3e}")
    if precision == 64:
        assert np.max(np.abs(got - want)) < TOL
    else:
        report(f"{label} {shape}", check_fp32(got, want, _want(shape, x, p, q, np.complex64)))
    assert abs(norm2 - after) < TOL


@pytest.fixture(scope="module")
def loop_states():
    """Random unit states at the looping sizes, computed once: precision -> (x, p, q)."""
    return {precision: tuple(rand_state(_loop_n(precision), 900 + k) for k in range(3)) for precision in PRECISIONS}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 2, 9])
def test_combine(n, precision):
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as p, Simulator(n, precision=precision) as q:
        p.write(rand_state(n, 11 + n))
        q.write(rand_state(n, 31 + n))
        pv, qv = p.read(), q.read()
        for shape in SHAPES:
            dst.write(rand_state(n, 51 + n))
            x = dst.read()
            norm2 = _call(shape, dst, p, q)
            _check(precision, shape, dst.read(), norm2, x, pv, qv, f"combine n={n}")
        assert np.array_equal(p.read(), pv) and np.array_equal(q.read(), qv)
        assert _call("three", dst, p, q, norm=False) is None


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 9])
def test_combine_overwrites_garbage_when_d_is_zero(n, precision):
    """dst holds NaN in every amplitude: with d == 0 it is not loaded, the result is finite and right."""
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as p, Simulator(n, precision=precision) as q:
        p.write(rand_state(n, 12 + n))
        q.write(rand_state(n, 32 + n))
        pv, qv = p.read(), q.read()
        for shape in ("d0_two", "d0_one"):
            dst.write(np.full(1 << n, complex(np.nan, np.nan)))
            assert np.isnan(dst.read()).all()
            norm2 = _call(shape, dst, p, q)
            got = dst.read()
            assert np.isfinite(got).all() and np.isfinite(norm2)
            _check(precision, shape, got, norm2, np.zeros(1 << n, dtype=np.complex128), pv, qv, f"garbage n={n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_combine_and_inner_where_every_workgroup_loops(precision, loop_states):
    n = _loop_n(precision)
    xs, ps, qs = loop_states[precision]
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as p, Simulator(n, precision=precision) as q:
        p.write(ps)
        q.write(qs)
        pv, qv = p.read(), q.read()
        got = p.inner(q)
        print(f"inner n={n} p{precision}: err {abs(got - np.vdot(pv, qv)):.3e}")
        assert abs(got - np.vdot(pv, qv)) < TOL
        for shape in ("three", "two", "d0_one"):
            dst.write(xs)
            x = dst.read()
            norm2 = _call(shape, dst, p, q)
            _check(precision, shape, dst.read(), norm2, x, pv, qv, f"looping n={n}")
        dst.copy_from(p)
        assert np.array_equal(_bits(dst), pv.view(np.uint64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 9])
def test_inner(n, precision):
    with Simulator(n, precision=precision) as a, Simulator(n, precision=precision) as b:
        a.write(rand_state(n, 13 + n) * 0.8)
        b.write(rand_state(n, 33 + n))
        av, bv = a.read(), b.read()
        ab, ba, aa = a.inner(b), b.inner(a), a.inner(a)
        print(f"inner n={n} p{precision}: err {abs(ab - np.vdot(av, bv)):.3e}, <a|a> - norm2 = {aa.real - a.norm2():.3e}")
        assert abs(ab - np.vdot(av, bv)) < TOL
        assert abs(ab - ba.conjugate()) < TOL
        assert aa.imag == 0.0 and abs(aa.real - a.norm2()) < TOL and abs(aa.real - np.vdot(av, av).real) < TOL
        assert a.inner(b) == ab  # equal calls, equal bits


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 2, 9])
def test_copy_from_is_bit_exact(n, precision):
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as src:
        v = rand_state(n, 14 + n)
        v[0] = complex(-0.0, 0.0)  # a signed zero survives a copy; it would not survive a multiplication by one plus zero
        src.write(v)
        dst.write(rand_state(n, 34 + n))
        dst.copy_from(src)
        assert np.array_equal(_bits(dst), _bits(src))
        assert dst.get_support()[0] == (1 << n) - 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lazy_states(precision):
    """A source fresh from reset(), never written; a destination a short circuit left with a partial support; an overwritten
    destination that was never written.  Results as from the dense equivalents."""
    n = 18
    few = Circuit.from_gates(n, circuits.random_gates(*fp32_ref.FEW_CIRCUIT))
    with Simulator(n, precision=precision) as probe, Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as src:
        probe.run(few)
        x = probe.read()  # the read writes the zeros out: the destination's contents are read from a twin
        dst.run(few)
        assert dst.get_support()[0] != (1 << n) - 1  # partial: most of the buffer has never been written
        src.reset()
        assert src.get_support()[1]  # |0...0> is still held lazily
        norm2 = dst.combine(D, (A, src), norm=True)
        got = dst.read()
        assert dst.get_support()[0] == (1 << n) - 1
        zero = np.zeros(1 << n, dtype=np.complex128)
        zero[0] = 1
        _check(precision, "two", got, norm2, x, zero, zero, "lazy source, partial destination")
        # inner with a lazy state on either side
        src.reset()
        assert abs(src.inner(dst) - got[0]) < TOL
        src.reset()
        assert abs(dst.inner(src) - np.conj(got[0])) < TOL
        # a shard that holds nothing counts as zeros
        src.reset(holds_index0=False)
        assert dst.inner(src) == 0
        # an overwritten destination that holds a pending |0...0> and queued gates: neither is seen
        with Simulator(n, precision=precision) as fresh:
            fresh.apply_1q(np.array([[0, 1], [1, 0]]), 3)
            norm2 = fresh.combine(0, (A, dst), norm=True)
            assert fresh.get_support() == ((1 << n) - 1, False, 0.0)
            _check(precision, "d0_one", fresh.read(), norm2, zero, got, got, "lazy destination, overwritten")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_on_a_source_are_applied_first(precision):
    n = 9
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as p, Simulator(n, precision=precision) as twin:
        for s in (p, twin):
            s.write(rand_state(n, 15))
            s.apply_1q(h, 4)
            s.apply_cx(4, 7)
        pv = twin.read()  # the twin's read flushes the twin; p still has its gates queued
        dst.write(rand_state(n, 35))
        x = dst.read()
        norm2 = dst.combine(D, (A, p), norm=True)
        _check(precision, "two", dst.read(), norm2, x, pv, pv, "queued gates on p")
        assert np.array_equal(p.read(), pv)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_later_gate_on_a_source_does_not_overtake_the_read(precision):
    """States have streams of their own: combine with p = A, then at once a gate on A, flushed.  The combine saw the old A."""
    n = _loop_n(precision) - 2
    xgate = np.array([[0, 1], [1, 0]])
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as a:
        a.write(rand_state(n, 16))
        dst.write(rand_state(n, 36))
        av, x = a.read(), dst.read()
        dst.combine(D, (A, a))          # not waited for
        a.apply_1q(xgate, n - 1)
        a.flush()
        got, after = dst.read(), a.read()
        assert np.array_equal(after, np.roll(av, 1 << (n - 1)))  # the gate did run
        _check(precision, "two", got, float(np.vdot(got, got).real), x, av, av, "ordering")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_calls_give_equal_bits_whatever_the_grid_cap(precision):
    n = 15
    results = []
    for options in ({}, {}, {"grid_cap": 7}):
        with Simulator(n, precision=precision, **options) as dst, Simulator(n, precision=precision) as p, Simulator(n, precision=precision) as q:
            p.write(rand_state(n, 17))
            q.write(rand_state(n, 37))
            dst.write(rand_state(n, 57))
            norm2 = _call("three", dst, p, q)
            results.append((_bits(dst), norm2, p.inner(q)))
    for bits, norm2, inner in results[1:]:
        assert np.array_equal(bits, results[0][0]) and norm2 == results[0][1] and inner == results[0][2]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_destination_alone(precision):
    n = 6
    other = 32 if precision == 64 else 64
    with Simulator(n, precision=precision) as dst, Simulator(n, precision=precision) as p, Simulator(n + 1, precision=precision) as wide, \
            Simulator(n, precision=other) as rounded:
        dst.write(rand_state(n, 18))
        p.write(rand_state(n, 38))
        before = _bits(dst)
        calls = [lambda: dst.combine(D, (A, dst)),
                 lambda: dst.combine(D, (A, p), (B, dst)),
                 lambda: dst.combine(D, (A, wide)),
                 lambda: dst.combine(D, (A, p), (B, rounded)),
                 lambda: dst.combine(D, (complex(np.nan, 0), p)),
                 lambda: dst.combine(complex(0, np.inf), (A, p)),
                 lambda: dst.combine(D, (A, p), (complex(np.nan, 0), p)),
                 lambda: dst.copy_from(dst),
                 lambda: dst.copy_from(wide),
                 lambda: dst.copy_from(rounded),
                 lambda: dst.inner(wide),
                 lambda: dst.inner(rounded)]
        for call in calls:
            with pytest.raises(_lib.QsimError) as err:
                call()
            assert err.value.code == _lib.ERR_ARG
            assert np.array_equal(_bits(dst), before)
