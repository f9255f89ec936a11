"""CPU-only checks of the assembled-input entry points (plk_setup_from_polynomials, plk_prove_assembled, plk_prove_assembled_dev):
null handles and pointers are refused with PLK_ERR_ARG before any device is touched, and the Python wrapper refuses badly shaped
arrays before it calls the library.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

import plonkit_amd as pa

PLK_ERR_ARG = 1


def _vec(n=8):
    return np.zeros((n, 4), dtype=np.uint64)


def test_null_arguments_are_refused_before_any_device_work():
    L = pa.lib()
    v = [_vec() for _ in range(11)]
    sel = (ctypes.c_void_p * 6)(*[x.ctypes.data for x in v[:6]])
    sig = (ctypes.c_void_p * 4)(*[x.ctypes.data for x in v[7:]])
    nxt = ctypes.c_void_p(v[6].ctypes.data)
    out = ctypes.c_void_p()
    u64 = ctypes.c_uint64
    # plk_setup_from_polynomials: no context, no selector array, a NULL vector inside it, no next-step selector, no sigmas, no out
    assert L.plk_setup_from_polynomials(None, u64(7), u64(1), sel, nxt, sig, u64(8), ctypes.c_uint32(0), ctypes.byref(out)) == PLK_ERR_ARG
    assert L.plk_setup_from_polynomials(None, u64(7), u64(1), None, nxt, sig, u64(8), ctypes.c_uint32(0), ctypes.byref(out)) == PLK_ERR_ARG
    holes = (ctypes.c_void_p * 6)(*([x.ctypes.data for x in v[:5]] + [None]))
    assert L.plk_setup_from_polynomials(None, u64(7), u64(1), holes, nxt, sig, u64(8), ctypes.c_uint32(0), ctypes.byref(out)) == PLK_ERR_ARG
    assert L.plk_setup_from_polynomials(None, u64(7), u64(1), sel, None, sig, u64(8), ctypes.c_uint32(0), ctypes.byref(out)) == PLK_ERR_ARG
    assert L.plk_setup_from_polynomials(None, u64(7), u64(1), sel, nxt, None, u64(8), ctypes.c_uint32(0), None) == PLK_ERR_ARG
    assert not out.value
    # the prove entry points: no context, no setup, no columns, no output buffer
    cols = (ctypes.c_void_p * 4)(*[x.ctypes.data for x in v[:4]])
    buf = ctypes.create_string_buffer(64)
    n = ctypes.c_uint64(123)
    assert L.plk_prove_assembled(None, None, cols, u64(8), buf, u64(64), ctypes.byref(n)) == PLK_ERR_ARG
    assert L.plk_prove_assembled(None, None, None, u64(8), buf, u64(64), ctypes.byref(n)) == PLK_ERR_ARG
    assert L.plk_prove_assembled(None, None, cols, u64(8), None, u64(64), None) == PLK_ERR_ARG
    assert L.plk_prove_assembled_dev(None, None, cols, u64(8), buf, u64(64), ctypes.byref(n), None) == PLK_ERR_ARG
    assert L.plk_prove_assembled_dev(None, None, None, u64(8), buf, u64(64), ctypes.byref(n), None) == PLK_ERR_ARG
    assert "bad argument" in pa.last_error()


@pytest.mark.parametrize("bad", [
    np.zeros((8, 4), dtype=np.int64),            # wrong dtype
    np.zeros((8, 3), dtype=np.uint64),           # not 4 limbs
    np.zeros(32, dtype=np.uint64),               # flat
    np.zeros((4, 8, 4), dtype=np.uint64),        # a stack, not one vector
    np.zeros((7, 4), dtype=np.uint64),           # length differs from the others
    np.zeros((0, 4), dtype=np.uint64),           # empty
    None,
])
def test_wrapper_rejects_badly_shaped_setup_vectors(bad):
    vecs = [_vec() for _ in range(11)]
    vecs[3] = bad
    with pytest.raises(ValueError):
        pa.SetupForProver.from_polynomials(None, 7, 1, vecs[:6], vecs[6], vecs[7:])


def test_wrapper_rejects_wrong_vector_counts():
    vecs = [_vec() for _ in range(11)]
    with pytest.raises(ValueError):
        pa.SetupForProver.from_polynomials(None, 7, 1, vecs[:5], vecs[6], vecs[7:])
    with pytest.raises(ValueError):
        pa.SetupForProver.from_polynomials(None, 7, 1, vecs[:6], vecs[6], vecs[7:10])


def test_wrapper_rejects_badly_shaped_columns():
    s = pa.SetupForProver.__new__(pa.SetupForProver)          # no setup is needed to refuse the arrays
    s.ctx, s._h = None, ctypes.c_void_p()
    with pytest.raises(ValueError):
        s.prove_assembled([_vec()] * 3)
    with pytest.raises(ValueError):
        s.prove_assembled([_vec(), _vec(), _vec(), _vec(7)])
    with pytest.raises(ValueError):
        s.prove_assembled([_vec(), _vec(), np.zeros((8, 4), dtype=np.float64), _vec()])
    with pytest.raises(ValueError):
        s.prove_assembled_dev([0, 0, 0], 8)
