// amp.inc — the amplitude type and its complex arithmetic in the precision of the enclosing namespace.  Like every .inc here it
// is included twice by kernels.hip (namespace f64: QSIM_REAL = double, 16-byte amplitudes; namespace f32: QSIM_REAL = float,
// 8-byte amplitudes — the precision of the reference's CUDA variants, quantum_simulator_naive.cu:145-149): no include guards
// on purpose.  The head of kernels.hip says which file owns what.

// Amplitudes travel as clang's native 2 x real vector (fp64: one global_load_dwordx4 / ds_read_b128 each; fp32: dwordx2 /
// b64) and, unlike the HIP_vector_type wrapper, a first-class value (arrays of it stay in registers).
typedef QSIM_REAL real_t;
typedef real_t amp_t __attribute__((ext_vector_type(2)));
constexpr int kAmpShift = QSIM_AMP_SHIFT; // log2(sizeof(amp_t))
static_assert(sizeof(amp_t) == (1u << kAmpShift), "QSIM_AMP_SHIFT must match the amplitude size");

// r = a*u (complex), then r += b*w — written as explicit FMAs so hipcc keeps one v_fma_f64 each.
__device__ __forceinline__ amp_t cmul(amp_t a, real_t ur, real_t ui) {
    amp_t r;
    r.x = fma(a.x, ur, -(a.y * ui));
    r.y = fma(a.x, ui, a.y * ur);
    return r;
}
__device__ __forceinline__ amp_t cfma(amp_t a, real_t ur, real_t ui, amp_t acc) {
    amp_t r;
    r.x = fma(a.x, ur, fma(-a.y, ui, acc.x));
    r.y = fma(a.x, ui, fma(a.y, ur, acc.y));
    return r;
}
__device__ __forceinline__ amp_t shfl_xor2(amp_t a, int mask) {
    amp_t r;
    r.x = __shfl_xor(a.x, mask, 64);
    r.y = __shfl_xor(a.y, mask, 64);
    return r;
}
