"""The one place Python values turn into what ctypes hands the C ABI.  Private: the package's modules and plans.py use these and
nothing else for these jobs, so an empty list, a mask array or a matrix is spelled one way everywhere."""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int, c_uint64

import numpy as np

U64P = ctypes.POINTER(c_uint64)


def ints(values):
    """An int list as a c_int array that is never zero-length: an empty list still gives the library a pointer it may name."""
    values = [int(v) for v in values]
    return (c_int * max(len(values), 1))(*values)


def masks(values):
    """Python ints as a uint64 numpy array and its pointer; the caller keeps the array alive for as long as the pointer is used."""
    arr = np.array([int(v) for v in values], dtype=np.uint64)
    return arr, arr.ctypes.data_as(U64P)


def u64p(arr: np.ndarray):
    """The uint64_t * of a numpy uint64 array."""
    return arr.ctypes.data_as(U64P)


def dp(arr: np.ndarray):
    """The double * of a numpy float64 array."""
    return arr.ctypes.data_as(ctypes.POINTER(c_double))


def mat(U, dim: int) -> np.ndarray:
    """A (dim, dim) complex matrix, row-major, as 2 dim^2 doubles."""
    m = np.ascontiguousarray(np.asarray(U, dtype=np.complex128).reshape(dim * dim))
    return m.view(np.float64)


def is_complex(number) -> bool:
    return isinstance(number, complex) or (hasattr(number, "dtype") and number.dtype.kind == "c")
