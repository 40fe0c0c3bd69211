"""fp32 states on the paths the fp32 suite did not reach: every fp32 instantiation of the tile kernel, out-of-place passes and a
lent spare buffer, the sparse start over stale memory, the pack family, the masked sums and gather, and reads of a state whose
support is still partial.  Arithmetic is held to the criterion of tests/fp32_ref.py (run with -s for the figures); whatever
only moves data is compared bit for bit with a numpy index map applied to read()."""
import numpy as np
import pytest

import fp32_ref
import pauli_ref
from fp32_ref import check_fp32, gate_list, replay, report
from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

pytestmark = pytest.mark.gpu
_TRUTH = {}


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (s / np.linalg.norm(s)).astype(np.complex128)


def _case(oracle, tmp_path, spec, n=None):
    """(circuit, oracle amplitudes, complex64 replay) of random_gates(*spec) on a register of n >= spec[0] qubits."""
    n = spec[0] if n is None else n
    key = (spec, n)
    if key not in _TRUTH:
        path = circuits.write_qasm(str(tmp_path / "t.qasm"), n, circuits.random_gates(*spec))
        _, want, _, _ = oracle.run_qasm(path)
        _TRUTH[key] = (want, replay(n, gate_list(*spec)))
    return (Circuit.from_gates(n, circuits.random_gates(*spec)),) + _TRUTH[key]


def _pack_src_index(n, bits):
    """qsim_pack_bits layout: packed index (block << (n-k)) | rest reads source index src[packed]."""
    k = len(bits)
    d = np.arange(1 << n, dtype=np.int64)
    rest, blk = d & ((1 << (n - k)) - 1), d >> (n - k)
    keep = [b for b in range(n) if b not in bits]
    src = np.zeros_like(d)
    for i, b in enumerate(keep):
        src |= ((rest >> i) & 1) << b
    for i, b in enumerate(bits):
        src |= ((blk >> i) & 1) << b
    return src


def _c64(t):
    return t.cpu().numpy().reshape(-1).view(np.complex64).astype(np.complex128)


# ---- 1. every fp32 tile instantiation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_bits,threads", fp32_ref.TILE_SHAPES)
def test_every_fp32_tile_instantiation(oracle, tmp_path, tile_bits, threads):
    """Each (tile_bits, tile_threads) pair launch_tile can reach in fp32 — for 10..13 the nine pairs of its switch, which run
    under QSIM_TILE_MIN_WAVES = 4 from 512 threads up, unlike any fp64 kernel — with the smallest and largest low-bit count the
    engine accepts, an uncapped and a capped grid (several tiles per workgroup), on many tiles and on exactly one."""
    lows = sorted({max(2, tile_bits - 10), min(6, tile_bits - 2)})
    for spec in (fp32_ref.TILE_MANY, fp32_ref.tile_single(tile_bits)):
        n = spec[0]
        c, want, ref32 = _case(oracle, tmp_path, spec)
        for low in lows:
            for cap in (0, 3):
                with Simulator(n, fuse=3, profile=True, precision=32, tile_bits=tile_bits, tile_low_bits=low, grid_cap=cap,
                               tile_threads=threads) as sim:
                    assert _lib.load().qsim_get_option(sim._h, _lib.OPT_TILE_THREADS) == threads
                    sim.reset_stats()
                    sim.run(c)
                    got = sim.read()
                    tiles = sum(1 for k, *_ in sim.launch_log() if k == "tile")
                label = f"tile B={tile_bits} T={threads} low={low} cap={cap} n={n}"
                assert tiles > 0, label
                report(label, check_fp32(got, want, ref32))


# ---- 2. out of place -----------------------------------------------------------------------------------------------------
def test_out_of_place_passes_fp32(oracle, tmp_path):
    """QSIM_OPT_PINGPONG = 2 on an fp32 state: odd and even numbers of tile passes, fresh and replayed plans, one gate per
    flush and a written state — device_ptr never changes and the result is bit-identical to in-place passes."""
    n = 16
    with Simulator(n, fuse=3, profile=True, pingpong=2, tile_bits=10, precision=32) as pp, \
            Simulator(n, fuse=3, pingpong=0, tile_bits=10, precision=32) as ip:
        home = pp.device_ptr
        counts = set()
        for i, spec in enumerate(fp32_ref.OOP_CIRCUITS):
            c, want, ref32 = _case(oracle, tmp_path, spec)
            ip.reset(); ip.run(c)
            ref = ip.read()
            report(f"in place {spec}", check_fp32(ref, want, ref32))
            for rep in range(2):  # the second run replays the cached plan
                pp.reset(); pp.reset_stats(); pp.run(c)
                got = pp.read()
                assert pp.device_ptr == home, (i, rep)
                assert np.array_equal(got, ref), (i, rep)
            counts.add(sum(1 for k, *_ in pp.launch_log() if k == "tile") % 2)
        assert counts == {0, 1}  # both an even and an odd number of tile passes were exercised
        s0 = _rand_state(n, 5)
        pp.write(s0); ip.write(s0)
        for g in circuits.random_gates(*fp32_ref.OOP_CIRCUITS[1])[:25]:
            for sim in (pp, ip):
                sim.run(Circuit.from_gates(n, [g])); sim.flush()
        assert np.array_equal(pp.read(), ip.read()) and pp.device_ptr == home


def test_lent_spare_buffer_fp32(oracle, tmp_path):
    """qsim_set_spare_buffer on an fp32 state that owns its buffer: the result lands in the state's own buffer, the lent one
    is scratch, and once it is taken back the state no longer touches it."""
    import torch
    spec = fp32_ref.SPARE_CIRCUIT
    n = spec[0]
    c, want, ref32 = _case(oracle, tmp_path, spec)
    spare = torch.full((1 << n, 2), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with Simulator(n, fuse=3, profile=True, pingpong=2, tile_bits=10, precision=32) as sim:
        home = sim.device_ptr
        sim.set_spare_buffer(spare.data_ptr())
        for rep in range(2):
            sim.reset(); sim.reset_stats(); sim.run(c)
            got = sim.read()
            assert sim.device_ptr == home
            assert sum(1 for k, *_ in sim.launch_log() if k == "tile") >= 2
            report(f"lent spare rep={rep}", check_fp32(got, want, ref32))
        assert not bool((spare == 7.0).all())  # the lent buffer was written to
        sim.set_spare_buffer(None)
        spare.fill_(3.0); torch.cuda.synchronize()
        sim.reset(); sim.run(c)
        got = sim.read()
        sim.sync(); torch.cuda.synchronize()
        assert bool((spare == 3.0).all())
        assert sim.device_ptr == home
        report("spare taken back", check_fp32(got, want, ref32))
        with pytest.raises(_lib.QsimError):
            sim.set_spare_buffer(sim.device_ptr)


# ---- 3. sparse start -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pingpong", [0, 2])
def test_sparse_start_fp32(oracle, tmp_path, pingpong):
    """QSIM_OPT_SPARSE_START on fp32 states, over stale amplitudes of a dense run in both buffers: a circuit on qubits 0..6
    reads back exact zeros above index 127, a full circuit passes the checker like the sparse_start = 0 state does, and a
    write in the middle of the sparse phase followed by more gates is bit-identical to the same calls on that state."""
    n = 18
    dense = Circuit.from_gates(n, circuits.random_gates(n, 400, 5, "all"))
    c_few, want_few, ref_few = _case(oracle, tmp_path, fp32_ref.FEW_CIRCUIT, n)
    spec = fp32_ref.SPARSE_CIRCUIT
    c, want, ref32 = _case(oracle, tmp_path, spec)
    gates = circuits.random_gates(*spec)
    with Simulator(n, fuse=3, profile=True, pingpong=pingpong, tile_bits=10, precision=32) as sim, \
            Simulator(n, fuse=3, pingpong=pingpong, tile_bits=10, sparse_start=0, precision=32) as full:
        for st in (sim, full):
            st.run(dense); st.sync()  # leaves dense garbage behind
        sim.reset(); sim.run(c_few)
        assert sim.get_support()[0] != (1 << n) - 1  # the state is partial: most of the buffer is stale
        got = sim.read()
        assert not got[128:].any()
        report(f"sparse few pp={pingpong}", check_fp32(got, want_few, ref_few))
        sim.reset(); sim.run(c)
        got = sim.read()
        full.reset(); full.run(c)
        report(f"sparse start pp={pingpong}", check_fp32(got, want, ref32))
        report(f"full sweeps pp={pingpong}", check_fp32(full.read(), want, ref32))
        # a dense single-qubit kernel (its own launch at fuse 0) in the middle of the sparse phase
        sim.reset(); sim.run(Circuit.from_gates(n, gates[:40])); sim.flush()
        sim.set_option(_lib.OPT_FUSE, 0)
        sim.run(Circuit.from_gates(n, gates[40:45])); sim.flush()
        sim.set_option(_lib.OPT_FUSE, 3)
        sim.run(Circuit.from_gates(n, gates[45:])); sim.flush()
        report(f"sparse + fuse 0 pp={pingpong}", check_fp32(sim.read(), want, ref32))
        s0 = _rand_state(n, 77)
        sim.reset(); sim.run(Circuit.from_gates(n, gates[:30])); sim.flush()
        sim.write(s0)
        sim.run(Circuit.from_gates(n, gates[:60]))
        full.write(s0); full.run(Circuit.from_gates(n, gates[:60]))
        assert np.array_equal(sim.read(), full.read())


# ---- 4. the pack family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits", [(14, (0,)), (14, (13,)), (14, (0, 13)), (14, (1, 5, 9)), (14, (0, 3, 4, 11, 13)),
                                    (14, (2, 3, 5, 7, 8, 12)), (14, (0, 1, 2, 3, 4, 5, 13)), (14, (0, 2, 4, 6, 8, 10, 12, 13)),
                                    (8, (0,)), (8, (7,)), (8, (1, 3, 6)), (8, (0, 1, 2, 3, 4, 5, 6, 7))])
def test_pack_bits_fp32(n, bits):
    """qsim_pack_bits on an fp32 state, 1..8 bits, bit 0 and the top bit; n = 8 is below the pack kernel's 10-bit work tile."""
    import torch
    s = _rand_state(n, 50 + len(bits))
    with Simulator(n, precision=32) as sim:
        sim.write(s)
        state = sim.read()
        dst = torch.full((1 << n, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the pack on the engine's: order them
        sim.pack_bits(bits, dst.data_ptr())
        sim.sync()
        assert np.array_equal(_c64(dst), state[_pack_src_index(n, bits)])


@pytest.mark.parametrize("bits", [(0,), (13,), (3, 11), (0, 5, 13)])
def test_pack_bits_to_and_buffer_swap_fp32(bits):
    """qsim_pack_bits_to into scattered, reverse-ordered blocks at 8-byte amplitude offsets (the gaps stay untouched), and a
    qsim_swap_buffer round trip of an fp32 state."""
    import torch
    n = 14
    k = len(bits)
    blk = 1 << (n - k)
    s = _rand_state(n, 51)
    src = _pack_src_index(n, bits)
    with Simulator(n, precision=32) as sim:
        sim.write(s)
        state = sim.read()
        big = torch.zeros((2 << n, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        starts = [(2 * ((1 << k) - 1 - b)) * blk for b in range(1 << k)]  # reverse order, a gap after every block
        sim.pack_bits_to(bits, [big.data_ptr() + 8 * st for st in starts])
        sim.sync()
        got = _c64(big)
        for b, st in enumerate(starts):
            assert np.array_equal(got[st:st + blk], state[src][b * blk:(b + 1) * blk]), b
            assert not got[st + blk:st + 2 * blk].any()  # the gaps stay untouched
        with pytest.raises(_lib.QsimError, match="overlaps the state"):
            sim.pack_bits_to(bits, [sim.device_ptr] * (1 << k))
    with Simulator(n, precision=32) as sim:
        sim.write(s)
        state = sim.read()
        spare_t = torch.zeros((1 << n, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        spare = spare_t.data_ptr()
        old_ptr = sim.device_ptr
        sim.pack_bits_to(bits[:1], [spare, spare + 8 * (1 << (n - 1))])  # spare = the state packed on bits[0]
        was = sim.swap_buffer(spare)
        assert was == old_ptr and sim.device_ptr == spare
        assert np.array_equal(sim.read(), state[_pack_src_index(n, bits[:1])])
        assert sim.swap_buffer(was) == spare  # hand the original back before the state is destroyed (torch owns `spare`)
        assert np.array_equal(sim.read(), state)


@pytest.mark.parametrize("bits,skip", [((3, 12), 0b0101), ((1, 7, 13), 0b10010010), ((0, 4, 9, 12, 13), 0x80000001)])
def test_pack_bits_sparse_on_a_partial_fp32_state(bits, skip):
    """qsim_pack_bits_sparse packs a partially written fp32 state as it is: amplitudes outside the support come out as exact
    zeros although the memory there holds a stale dense run (k_pack zero_mask), and skipped blocks keep their NaNs."""
    import torch
    from ctypes import c_int, c_void_p
    n = 14
    k = len(bits)
    blk = 1 << (n - k)
    dense = Circuit.from_gates(n, circuits.random_gates(n, 300, 6, "all"))
    few = Circuit.from_gates(n, circuits.random_gates(5, 80, 13, "all"))
    with Simulator(n, fuse=3, precision=32) as sim:
        sim.run(dense); sim.sync()
        sim.reset(); sim.run(few)
        assert sim.get_support()[0] != (1 << n) - 1
        dst = torch.full((1 << n, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.load().qsim_pack_bits_sparse(sim._h, (c_int * k)(*bits), k, c_void_p(dst.data_ptr()), None, skip))
        sim.sync()
        got = dst.cpu().numpy().reshape(-1).view(np.complex64)
        want = sim.read()[_pack_src_index(n, bits)]
    assert 0 < np.count_nonzero(want) < want.size // 4  # mostly zeros by definition
    for b in range(1 << k):
        piece = got[b * blk:(b + 1) * blk]
        if skip >> b & 1:
            assert np.isnan(piece.view(np.float32)).all(), b
        else:
            assert np.array_equal(piece.astype(np.complex128), want[b * blk:(b + 1) * blk]), b


@pytest.mark.parametrize("bits", [(5,), (0, 13), (1, 5, 9, 13), (0, 3, 4, 11, 13), (0, 2, 4, 6, 8, 10),
                                  (1, 2, 3, 5, 8, 12, 13), (0, 1, 2, 3, 4, 5, 6, 13)])
def test_flush_pack_fp32(bits):
    """qsim_flush_pack on an fp32 state always takes flush + the pack kernel (fused = 0), refuses the steered forms
    (to_bits / konst) with the fp32 message, honours skip_blocks up to 5 bits and writes every block from 6 on."""
    import torch
    n = 14
    k = len(bits)
    blk = 1 << (n - k)
    src = _pack_src_index(n, bits)
    c = Circuit.from_gates(n, circuits.random_gates(n, 300, 1400, "all"))
    skip = 0b1010010010 & ((1 << (1 << k)) - 1)
    with Simulator(n, fuse=3, precision=32) as sim:
        out = torch.full((1 << n, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for rep in range(2):
            sim.reset(); sim.run(c)
            at, fused = sim.flush_pack(bits, out.data_ptr())
            sim.sync()
            assert not fused and at == out.data_ptr()
            assert np.array_equal(_c64(out), sim.read()[src]), rep
        out.fill_(float("nan")); torch.cuda.synchronize()
        sim.reset(); sim.run(c)
        at, fused = sim.flush_pack(bits, out.data_ptr(), skip_blocks=skip)
        sim.sync()
        assert not fused
        got = out.cpu().numpy().reshape(-1).view(np.complex64)
        want = sim.read()[src]
        for b in range(1 << k):
            piece = got[b * blk:(b + 1) * blk]
            if k <= 5 and skip >> b & 1:
                assert np.isnan(piece.view(np.float32)).all(), b
            else:
                assert np.array_equal(piece.astype(np.complex128), want[b * blk:(b + 1) * blk]), b
        for kw in ({"to_bits": [n - k + j for j in range(k)]}, {"konst": 1 << n}):
            with pytest.raises(_lib.QsimError, match="of an fp32 state"):
                sim.flush_pack(bits, out.data_ptr(), **kw)


# ---- 5. masked sums and gather -----------------------------------------------------------------------------------------
def test_masked_block_sums_and_gather_fp32():
    """qsim_block_prob_masked against fp64 sums of the widened read() (products of two floats are exact in fp64; only the
    additions round: 1e-15), and qsim_gather_masked bit-identical to read() at the deposited indices."""
    n = 13
    s = _rand_state(n, 52)
    rng = np.random.default_rng(3)

    def deposit(x, mask):
        out, j = 0, 0
        for b in range(64):
            if mask >> b & 1:
                out |= ((x >> j) & 1) << b
                j += 1
        return out

    full = (1 << n) - 1
    masks = []
    for _ in range(6):
        bits = rng.permutation(n)
        nlo = int(rng.integers(1, 9))
        masks.append(sum(1 << int(b) for b in bits[:nlo]))
    masks += [1 << 9, 1, 0b1111110, 0b1010100110000]  # a single bit, bit 0 alone, masks without bit 0
    with Simulator(n, precision=32) as sim:
        sim.write(s)
        r = sim.read()
        p = r.real * r.real + r.imag * r.imag
        for lo_mask in masks:
            hi_mask = full & ~lo_mask
            nlo = bin(lo_mask).count("1")
            sums = sim.block_prob_masked(hi_mask, lo_mask)
            idx = np.array([[deposit(w, hi_mask) | deposit(i, lo_mask) for i in range(1 << nlo)] for w in range(1 << (n - nlo))])
            want = p[idx].sum(axis=1)
            assert np.max(np.abs(sums - want)) < 1e-15, lo_mask
            for w in (0, int(rng.integers(0, 1 << (n - nlo))), (1 << (n - nlo)) - 1):
                assert np.array_equal(sim.gather_masked(deposit(w, hi_mask), lo_mask), r[idx[w]]), (lo_mask, w)


# ---- 6. reads of a partial state over garbage ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_reads_of_a_partial_state_over_stale_memory(precision):
    """A dense run, a reset, then a circuit on five of sixteen qubits with nothing read in between: the state's support is
    partial and the rest of its buffer holds the dense run.  Expectation values, norm2 and sample of that state agree with
    the same computations on read() (the zeros outside the support included)."""
    n = 16
    dense = Circuit.from_gates(n, circuits.random_gates(n, 300, 6, "all"))
    few = Circuit.from_gates(n, circuits.random_gates(5, 80, 13, "all"))
    rng = np.random.default_rng(8)
    masks = [pauli_ref.random_masks(rng, n, 1 + i % 6) for i in range(40)] + [(0, 1 << 15), (1 << 15, 0), (0b11111, 0), (0, 0b11111)]
    paulis = [pauli_ref.masks_to_text(x, z, n) for x, z in masks]
    randoms = np.array([0.0, 1e-9, 0.1, 0.25, 0.5, 0.75, 0.999, 0.9999999, 1.0])
    with Simulator(n, fuse=3, precision=precision) as sim:
        def partial():
            sim.run(dense); sim.sync()
            sim.reset(); sim.run(few)
            assert sim.get_support()[0] != (1 << n) - 1

        partial()
        vals = sim.expectation_terms(paulis)
        r = sim.read()
        for v, (x, z) in zip(vals, masks):
            assert abs(v - pauli_ref.pauli_expectation(r, x, z)) < 1e-10, pauli_ref.masks_to_text(x, z, n)
        partial()
        nv = sim.norm2()
        r = sim.read()
        assert abs(nv - float(np.sum(r.real * r.real + r.imag * r.imag))) < 1e-12
        partial()
        idx = sim.sample(randoms)
        r = sim.read()
    with Simulator(n) as wide:
        wide.write(r)
        assert np.array_equal(idx, wide.sample(randoms))
