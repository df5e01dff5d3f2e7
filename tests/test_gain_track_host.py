"""CPU tier: the argument checks cmpc_gain_track and cmpc_solve_batch_gain_consts make on the host, before any device call."""
import ctypes

import pytest

import build as _b
from cmpc_amd import capi


@pytest.fixture(scope="module")
def lib():
    _b.build_hip()
    return capi.load()


def test_track_refuses_bad_arguments_on_the_host(lib):
    err = lambda: lib.cmpc_last_error(None).decode()
    p = ctypes.c_void_p(16)                                                    # never dereferenced: every call ends on the host
    track = lambda N, nv, B, columns, params=p: lib.cmpc_gain_track(N, nv, B, params, p, p, p, ctypes.c_uint32(columns), p, p, p, None)
    assert track(10, 4, 3, 1 << 20) != 0 and "columns" in err()
    assert track(10, 4, 3, 0x80000FFF) != 0 and "columns" in err()
    for N, nv, B in ((0, 4, 3), (65, 4, 3), (10, 5, 3), (10, 4, -1)):
        assert track(N, nv, B, 0xFFF) != 0 and "cmpc_gain_track: bad argument" in err(), (N, nv, B)
    assert track(10, 4, 3, 0xFFF, params=None) != 0 and "null buffer" in err()
    assert track(10, 8, 0, 0xFFFFF) == 0                                       # an empty batch: nothing to do


def test_gain_consts_needs_a_handle(lib):
    assert lib.cmpc_solve_batch_gain_consts(None, 1, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert "cmpc_solve_batch_gain_consts: null handle" in lib.cmpc_last_error(None).decode()
    assert lib.cmpc_version().decode() == "cmpc_amd 0.6 (gfx950)"
