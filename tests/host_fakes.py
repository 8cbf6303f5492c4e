"""What the `test_*_host.py` files put in an engine's place to reach the refusals that need no GPU: memory that passes for a
`szs_engine_s` on the C side, and a Python engine with no handle and no scope."""
import ctypes

import stringzilla_amd as szs

ENGINE_MAGIC = 0x535A5345  # csrc/host/szs_internal.h


class _EngineHead(ctypes.Structure):
    """The first members of `szs_engine_s` (csrc/host/szs_internal.h), up to the flag the calls read."""
    _fields_ = [("magic", ctypes.c_uint32), ("family", ctypes.c_int), ("costs", ctypes.c_int8 * 4), ("byte_to_class", ctypes.c_uint8 * 256),
                ("class_costs", ctypes.c_int8 * 1024), ("is_linear", ctypes.c_int), ("is_unit_cost", ctypes.c_int)]


def _fake_engine(family=0, unit_cost=1):
    """Memory that passes for an engine up to the point where a GPU would be needed: the magic, the family, the unit-cost flag."""
    blank = ctypes.create_string_buffer(1 << 16)
    head = _EngineHead.from_buffer(blank)
    head.magic, head.family, head.is_linear, head.is_unit_cost = ENGINE_MAGIC, family, 1, unit_cost
    head.costs[:] = [0, 1, 1, 1] if unit_cost else [0, 2, 3, 1]
    return blank


def _no_gpu_engine():
    return object.__new__(szs.LevenshteinDistances)  # no handle, no GPU: the arguments must be refused before either is needed
