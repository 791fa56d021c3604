"""The inflate decoder (csrc/inflate_core.hpp) on the host, through ``snpmi_inflate_host``: every
valid stream of ``inflate_cases`` gives its payload, every malformed one its status, and nothing
outside the destination's D bytes is touched.  No GPU is used; tests/test_gpu_inflate.py runs the same
lists through the device kernel."""
import os

import numpy as np
import pytest

import inflate_cases as C
from conftest import DATA
from pysnptools_amd import _native as N
from pysnptools_amd.distreader import Bgen

GUARD = 64


def inflate_host(stream, d, shift=0):
    """(status, the D bytes, guards intact) with dst ``shift`` bytes off an 8-byte boundary."""
    src = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(0, dtype=np.uint8)
    room = np.full(GUARD + d + GUARD + 8, 0xa5, dtype=np.uint8)
    at = GUARD + (-room.ctypes.data - GUARD) % 8 + shift
    status = np.full(1, 99, dtype=np.uint32)
    N.call("snpmi_inflate_host", N.ptr(src), len(src), room[at:].ctypes.data if d else N.ptr(room), d,
           N.ptr(status))
    intact = bool(np.all(room[:at] == 0xa5) and np.all(room[at + d:] == 0xa5))
    return int(status[0]), room[at:at + d].tobytes(), intact


@pytest.mark.parametrize("case", C.valid_cases(), ids=[c[0] for c in C.valid_cases()])
def test_valid_streams_give_their_payload(case):
    name, stream, payload = case
    for shift in (0, 3):  # the 8-byte stores of an aligned dst, and the byte stores
        status, got, intact = inflate_host(stream, len(payload), shift)
        assert status == C.OK and got == payload and intact


@pytest.mark.parametrize("case", C.malformed_cases(), ids=[c[0] for c in C.malformed_cases()])
def test_malformed_streams_give_their_status(case):
    name, stream, d, want = case
    status, _, intact = inflate_host(stream, d)
    assert status == want and intact


def test_every_status_is_reached():
    assert {inflate_host(stream, d)[0] for _, stream, d, _ in C.malformed_cases()} == set(range(1, 11))


def test_refusals():
    one, four = np.zeros(1, dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    with pytest.raises(ValueError):
        N.call("snpmi_inflate_host", None, 4, N.ptr(four), 4, N.ptr(one))
    with pytest.raises(ValueError):
        N.call("snpmi_inflate_host", N.ptr(four), 1 << 28, None, 0, N.ptr(one))


@pytest.mark.parametrize("value", ["x", None, "Device", 1])
def test_inflate_setting_is_checked_at_construction(value):
    with pytest.raises(ValueError, match="inflate"):
        Bgen(os.path.join(DATA, "example.bgen"), inflate=value)
    assert Bgen(os.path.join(DATA, "example.bgen"), inflate="device")._inflate_on == "device"
    assert Bgen(os.path.join(DATA, "example.bgen"))._inflate_on == "host"
