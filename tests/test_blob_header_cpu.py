"""The header checks of tr_bvh_deserialize (csrc/api.hip), without a GPU.

The blob is what save() persists: an 80-byte header and the arena, byte for byte.  tr_bvh_deserialize checks the header
before it touches a device, so every rejection is reachable here through ctypes.  The header is written by hand -- the
magic as bytes, the three record sizes as literals -- which pins the file format: a library that changes one of them
without a new magic version fails here."""
import ctypes as C
import struct

import pytest
import torch

import triro.backend.ops as hops

MAGIC = b"TRBVH\x00\x00\x04"
HEADER_BYTES = 80
SIZEOF_NODE, SIZEOF_TRI, SIZEOF_LINK = 64, 48, 8
INVALID_ARG, NO_DEVICE = 1, 3


def header(magic=MAGIC, num_tris=2, num_nodes=1, arena_bytes=0, depth=1, key_mode=0, sizeof_node=SIZEOF_NODE,
           sizeof_tri=SIZEOF_TRI, sizeof_link=SIZEOF_LINK):
    """magic[8] | num_tris, num_nodes, arena_bytes i64 | depth, key_mode i32 | aabb_min[3], aabb_max[3] f32 |
    sizeof_node, sizeof_tri, sizeof_link, pad u32"""
    h = magic + struct.pack("<3q2i6f4I", num_tris, num_nodes, arena_bytes, depth, key_mode, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0,
                            sizeof_node, sizeof_tri, sizeof_link, 0)
    assert len(h) == HEADER_BYTES
    return h


def deserialize(blob, size=None):
    """(status, *out, message); *out starts as a non-NULL sentinel"""
    lib = hops.get_module()
    buf = C.create_string_buffer(bytes(blob), len(blob))
    out = C.c_void_p(0xDEAD)
    status = lib.tr_bvh_deserialize(C.cast(buf, C.c_void_p), len(blob) if size is None else size, None, C.byref(out))
    return status, out.value, lib.tr_last_error().decode()


BAD_LAYOUT = "blob was written with a different record layout"
INCONSISTENT = "inconsistent blob header"
REJECTED = {
    "shorter than the header": (header()[:HEADER_BYTES - 1], None, "blob too small"),
    "magic of version 3": (header(magic=b"TRBVH\x00\x00\x03"), None, "not a triro BVH blob (bad magic/version)"),
    "magic of another file": (header(magic=b"\x93NUMPY\x01\x00"), None, "not a triro BVH blob (bad magic/version)"),
    "sizeof_node + 1": (header(sizeof_node=SIZEOF_NODE + 1), None, BAD_LAYOUT),
    "sizeof_node - 1": (header(sizeof_node=SIZEOF_NODE - 1), None, BAD_LAYOUT),
    "sizeof_tri + 1": (header(sizeof_tri=SIZEOF_TRI + 1), None, BAD_LAYOUT),
    "sizeof_tri - 1": (header(sizeof_tri=SIZEOF_TRI - 1), None, BAD_LAYOUT),
    "sizeof_link + 1": (header(sizeof_link=SIZEOF_LINK + 1), None, BAD_LAYOUT),
    "sizeof_link - 1": (header(sizeof_link=SIZEOF_LINK - 1), None, BAD_LAYOUT),
    "num_nodes == num_tris": (header(num_tris=2, num_nodes=2), None, INCONSISTENT),
    "num_nodes == num_tris - 2": (header(num_tris=3, num_nodes=1), None, INCONSISTENT),
    "a node for one triangle": (header(num_tris=1, num_nodes=1), None, INCONSISTENT),
    "num_tris < 0": (header(num_tris=-1, num_nodes=0), None, INCONSISTENT),
    "depth 65": (header(depth=65), None, INCONSISTENT),
    "size < header + arena_bytes": (header(arena_bytes=256) + bytes(256), HEADER_BYTES + 255, INCONSISTENT),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_device_is_touched(case):
    blob, size, message = REJECTED[case]
    status, out, got = deserialize(blob, size)
    assert status == INVALID_ARG and out is None and got == message, (case, status, out, got)


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU a header that passes is loaded")
def test_a_header_that_passes_needs_a_device():
    """the same header as in every case above, with nothing wrong: the first failure is the missing device"""
    for blob in (header(), header(depth=64), header(arena_bytes=256) + bytes(256)):
        status, out, got = deserialize(blob)
        assert status == NO_DEVICE and out is None, (status, out, got)
