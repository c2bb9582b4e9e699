"""Python op shims over the C ABI of libtriro_hip.so (include/triro_hip.h).

Mirrors triro/backend/ops.py of the reference function for function:

  get_module()                                   ops.py:12-46   (JIT build + import of the
                                                 pybind11 module) -> ctypes load of the
                                                 PREBUILT library; no JIT, no pybind11
  init_optix ... build_sbts                      ops.py:49-81   -> tr_init (idempotent)
  intersects_any/first/closest/count/location    ops.py:84-192  -> tr_intersects_*

Differences that are deliberate: inputs are validated and errors raise
(ValueError / RuntimeError) instead of printing and returning undefined tensors
(ray.cpp:104-123,164-165); float32 is enforced (the reference silently reinterprets other
dtypes); work is enqueued on torch's CURRENT stream of the tensors' device instead of a
private stream (base.cpp:34); outputs are allocated here (_new_output: torch.empty) and handed to the
library as raw pointers.

There is no CPU fallback: without the library or without a GPU every query raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Tuple

import torch

_INT64_MAX = (1 << 63) - 1
MAX_ANYHIT_SIZE = 8   # LaunchParams.h:8
MAX_SIZE_LENGTH = 4   # LaunchParams.h:9

_LIB_NAME = "libtriro_hip.so"
ABI_VERSION = 10    # TR_ABI_VERSION of include/triro_hip.h this binding was written against
_lib = None
_lib_error = None


class TrRays(C.Structure):
    """tr_rays (include/triro_hip.h) == RayInput of LaunchParams.h:11-28."""
    _fields_ = [("d_origins", C.c_void_p), ("d_directions", C.c_void_p), ("nray", C.c_int64),
                ("shape", C.c_int64 * 4), ("ostride", C.c_int64 * 4), ("dstride", C.c_int64 * 4)]


class TrTopology(C.Structure):
    """tr_topology (include/triro_hip.h)"""
    _fields_ = [("num_cus", C.c_int32), ("num_xcd", C.c_int32), ("waves_per_cu", C.c_int32), ("reserved", C.c_int32),
                ("l2_bytes", C.c_int64), ("resident_lanes", C.c_int64), ("steal_max_rays", C.c_int64),
                ("wide_min_rays", C.c_int64), ("count_stream_min_rays", C.c_int64)]


class TrBvhInfo(C.Structure):
    _fields_ = [("device", C.c_int32), ("num_tris", C.c_int64), ("num_nodes", C.c_int64),
                ("depth", C.c_int32), ("key_mode", C.c_int32), ("arena_bytes", C.c_int64),
                ("node_bytes", C.c_int64), ("tri_bytes", C.c_int64),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3)]


class TrLaunchInfo(C.Structure):
    _fields_ = [("rays", C.c_int64), ("blocks", C.c_int64), ("slots", C.c_int64), ("query", C.c_int32),
                ("shape", C.c_int32), ("tile_rows_lg", C.c_int32), ("split_blocks", C.c_int32),
                ("learned_order", C.c_int32), ("grid_nodes", C.c_int32), ("addressing", C.c_int32),
                ("sort_carried", C.c_int32)]


class TrTraceStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("climb_steps", C.c_uint64)]


def library_path() -> str:
    env = os.environ.get("TRIRO_HIP_LIBRARY")
    if env:
        return env
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                        "lib", _LIB_NAME)


# every symbol include/triro_hip.h declares: (restype, argtypes)
_vp, _i64, _i32, _int = C.c_void_p, C.c_int64, C.c_int32, C.c_int
ABI = {
    "tr_init": (_int, [_int]),
    "tr_abi_version": (_int, []),
    "tr_last_error": (C.c_char_p, []),
    "tr_bvh_build": (_int, [_vp, _i64, _vp, _i64, _vp, C.POINTER(_vp)]),
    "tr_bvh_update": (_int, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "tr_bvh_refit": (_int, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "tr_bvh_destroy": (_int, [_vp]),
    "tr_bvh_serialized_size": (_i64, [_vp]),
    "tr_bvh_serialize": (_int, [_vp, _vp, _i64, _vp]),
    "tr_bvh_deserialize": (_int, [_vp, _i64, _vp, C.POINTER(_vp)]),
    "tr_bvh_get_info": (_int, [_vp, C.POINTER(TrBvhInfo)]),
    "tr_bvh_last_launch": (_int, [_vp, C.POINTER(TrLaunchInfo)]),
    "tr_device_topology": (_int, [_int, C.POINTER(TrTopology)]),
    "tr_bvh_replica_hash": (_int, [_vp, C.POINTER(C.c_uint64), _vp]),
    "tr_bvh_download": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "tr_bvh_download_qnodes": (_int, [_vp, _vp, _vp, _vp]),
    "tr_intersects_any": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_intersects_first": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_intersects_closest": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_intersects_count": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_intersects_closest_packed": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_closest_expand": (_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_intersects_closest_packed_slots": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_closest_expand_slots": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_closest_expand_slots_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_intersects_closest_slots": (_int, [_vp, C.POINTER(TrRays), _vp, _vp]),
    "tr_closest_from_slots": (_int, [_vp, C.POINTER(TrRays), _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_hits_scan": (_int, [_vp, _i64, _i32, _vp, _vp, C.POINTER(_i64), _vp]),
    "tr_intersects_location_fill": (_int, [_vp, C.POINTER(TrRays), _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tr_intersects_count_topk": (_int, [_vp, C.POINTER(TrRays), _i32, _vp, _vp, _vp]),
    "tr_location_fill_slots": (_int, [_vp, C.POINTER(TrRays), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "tr_mask_scan": (_int, [_vp, _i64, _vp, _vp, C.POINTER(_i64), _vp]),
    "tr_compact_closest": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tr_trace_stats_closest": (_int, [_vp, C.POINTER(TrRays), C.POINTER(TrTraceStats), _vp]),
    "tr_trace_stats_query": (_int, [_vp, C.POINTER(TrRays), _int, C.POINTER(TrTraceStats), _vp]),
    "tr_set_option": (_int, [C.c_char_p, _i64]),
}


def get_module():
    """Load libtriro_hip.so (the counterpart of ops.py:12-46's JIT build + import)."""
    global _lib, _lib_error
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        _lib_error = (f"{path} not found: build it with `make -C trimesh-ray-optix_amd/csrc` "
                      f"(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                      f"There is no CPU fallback.")
        raise RuntimeError(_lib_error)
    lib = C.CDLL(path)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.tr_abi_version() != ABI_VERSION and os.environ.get("TRIRO_ABI_ANY") != "1":      # (TRIRO_ABI_ANY=1: A/B runs against an older build)
        raise RuntimeError(f"libtriro_hip.so ABI version {lib.tr_abi_version()} != {ABI_VERSION} expected by this binding")
    _lib = lib
    return _lib


def _check(status: int):
    if status != 0:
        msg = get_module().tr_last_error().decode("utf-8", "replace")
        if status == 1:
            raise ValueError(f"triro_hip: {msg}")
        raise RuntimeError(f"triro_hip (status {status}): {msg}")


# --- the five bring-up shims of ops.py:49-81 --------------------------------------------------
def init_optix():
    """ops.py:49-53.  Loads the library; initialises the current GPU if there is one."""
    try:
        lib = get_module()
    except RuntimeError:
        return   # import must not fail without the library; queries will
    if torch.cuda.is_available():
        _check(lib.tr_init(torch.cuda.current_device()))


def create_optix_context():
    """ops.py:56-60 -- nothing left to do (no OptiX context on gfx950)."""


def create_optix_module():
    """ops.py:63-67 -- kernels are linked into libtriro_hip.so."""


def create_optix_pipelines():
    """ops.py:70-74 -- the five pipelines are five kernel instantiations."""


def build_sbts():
    """ops.py:77-81 -- no shader binding tables."""


# --- marshaling -------------------------------------------------------------------------------
def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _fill4(vals, default):
    """fillArray of ray.cpp:151-159: right-align into MAX_SIZE_LENGTH slots."""
    vals = list(vals)
    return (C.c_int64 * 4)(*([default] * (MAX_SIZE_LENGTH - len(vals)) + vals))


def check_rays(origins: torch.Tensor, dirs: torch.Tensor):
    """tensorInputCheck (ray.cpp:104-123) plus the checks the reference forgets."""
    for name, t in (("origins", origins), ("directions", dirs)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must reside on a GPU (cuda/HIP) device")
        if t.layout != torch.strided:
            raise ValueError(f"{name} layout must be torch.strided")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if t.dim() < 1 or t.dim() > MAX_SIZE_LENGTH or t.shape[-1] != 3:
            raise ValueError(f"{name} must have shape [*b, 3] with at most 3 batch dims, got {tuple(t.shape)}")
    if origins.shape != dirs.shape:
        raise ValueError(f"origins {tuple(origins.shape)} and directions {tuple(dirs.shape)} differ in shape")
    if origins.device != dirs.device:
        raise ValueError("origins and directions are on different devices")


def make_rays(origins: torch.Tensor, dirs: torch.Tensor) -> TrRays:
    """LaunchParams marshaling of ray.cpp:173-179."""
    r = TrRays()
    r.d_origins = origins.data_ptr()
    r.d_directions = dirs.data_ptr()
    r.nray = origins.numel() // 3
    r.shape = _fill4(origins.shape, _INT64_MAX)
    r.ostride = _fill4(origins.stride(), 0)
    r.dstride = _fill4(dirs.stride(), 0)
    return r


def _handle(accel_structure, rays_tensor=None):
    h = accel_structure._inner
    if not h:
        raise RuntimeError("acceleration structure has not been built")
    if rays_tensor is not None:
        # the kernels dereference both the rays and the BVH arena: they must share a GPU
        bdev = getattr(accel_structure, "device_index", None)
        if bdev is not None and rays_tensor.device.index != bdev:
            raise ValueError(f"rays are on {rays_tensor.device} but the acceleration structure lives on "
                             f"cuda:{bdev}; move the rays or build the intersector on that device")
    return h


def _new_output(shape, dtype, device) -> torch.Tensor:
    """Every tensor the library writes into -- results and the intermediates count / slots / offsets / total_d -- is born
    here, uninitialised.  One seam, so that a run can swap it to see which bytes no kernel ever wrote (tests/poison.py)."""
    return torch.empty(shape, dtype=dtype, device=device)


# --- queries (ops.py:84-192) ----------------------------------------------------------------------
def intersects_any(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:84-100 / ray.cpp:161-189.  Bool[*b]."""
    check_rays(origins, dirs)
    out = _new_output(origins.shape[:-1], torch.bool, origins.device)
    with torch.cuda.device(origins.device):
        _check(get_module().tr_intersects_any(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                              out.data_ptr(), _stream_ptr(origins.device)))
    return out


def intersects_first(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:103-119 / ray.cpp:191-219.  Int32[*b], -1 on miss."""
    check_rays(origins, dirs)
    out = _new_output(origins.shape[:-1], torch.int32, origins.device)
    with torch.cuda.device(origins.device):
        _check(get_module().tr_intersects_first(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                                out.data_ptr(), _stream_ptr(origins.device)))
    return out


def intersects_closest(accel_structure, origins, dirs, outs=None) -> Tuple[torch.Tensor, ...]:
    """ops.py:122-149 / ray.cpp:231-289.  (hit, front, tri_idx, loc, uv).  `outs`: optional preallocated
    contiguous destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2] with n = the
    number of rays -- e.g. this rank's rows of gathered full-size outputs, triro.ray.sharded)."""
    check_rays(origins, dirs)
    b, dev = origins.shape[:-1], origins.device
    if outs is not None:
        n = origins.numel() // 3
        want = ((torch.bool, (n,)), (torch.bool, (n,)), (torch.int32, (n,)), (torch.float32, (n, 3)), (torch.float32, (n, 2)))
        if len(outs) != 5 or any(t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                                 for t, (dt, sh) in zip(outs, want)):
            raise ValueError("outs must be contiguous (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on the rays' device")
        hit, front, tri, loc, uv = outs
    else:
        hit = _new_output(b, torch.bool, dev)
        front = _new_output(b, torch.bool, dev)
        tri = _new_output(b, torch.int32, dev)
        loc = _new_output((*b, 3), torch.float32, dev)
        uv = _new_output((*b, 2), torch.float32, dev)
    with torch.cuda.device(dev):
        _check(get_module().tr_intersects_closest(
            _handle(accel_structure, origins), C.byref(make_rays(origins, dirs)), hit.data_ptr(), front.data_ptr(),
            tri.data_ptr(), loc.data_ptr(), uv.data_ptr(), _stream_ptr(dev)))
    return hit, front, tri, loc, uv


def intersects_closest_packed(accel_structure, origins, dirs, out: torch.Tensor = None, slots: bool = False) -> torch.Tensor:
    """Closest hit as 12 bytes per ray: int32 [n, 3] rows {face | front << 30 (-1 on a miss), u bits,
    v bits} (tr_packed_hit).  What a ray-sharded run sends over xGMI instead of the 26 B/ray of the five
    dense outputs; `closest_expand` rebuilds those bit for bit.  `out`: optional preallocated [n, 3]
    int32 destination (a slice of a gather buffer)."""
    check_rays(origins, dirs)
    n, dev = origins.numel() // 3, origins.device
    if out is None:
        out = _new_output((n, 3), torch.int32, dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (n, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int32 [n, 3] tensor on the rays' device")
    # slots: the record names the ARENA SLOT of the triangle instead of its face index (tr_intersects_closest_packed_slots):
    # cheaper to expand (closest_expand_slots), valid only for this hierarchy or a bit-identical replica of it
    fn = get_module().tr_intersects_closest_packed_slots if slots else get_module().tr_intersects_closest_packed
    with torch.cuda.device(dev):
        _check(fn(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)), out.data_ptr(), _stream_ptr(dev)))
    return out


def intersects_closest_slots(accel_structure, origins, dirs, out: torch.Tensor = None) -> torch.Tensor:
    """tr_intersects_closest_slots: closest hit as 4 bytes per ray -- int32 [n]: the arena slot of the nearest
    triangle, -1 for a miss.  For a destination that holds the rays (closest_from_slots finishes the query there);
    valid for this hierarchy or a bit-identical replica.  `out`: optional preallocated int32 [n] destination."""
    check_rays(origins, dirs)
    n, dev = origins.numel() // 3, origins.device
    if out is None:
        out = _new_output((n,), torch.int32, dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (n,) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int32 [n] tensor on the rays' device")
    with torch.cuda.device(dev):
        _check(get_module().tr_intersects_closest_slots(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                                        out.data_ptr(), _stream_ptr(dev)))
    return out


def closest_from_slots(accel_structure, origins, dirs, slots: torch.Tensor, outs=None, row_length: int = 0):
    """tr_closest_from_slots: (rays, their slots from intersects_closest_slots on any bit-identical replica) ->
    (hit, front, tri_idx, loc, uv), the bits of intersects_closest on the same rays.  `outs`: optional preallocated
    contiguous destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2]); otherwise the outputs
    take the rays' batch shape.  row_length: the rays are whole rows of an image of that width."""
    check_rays(origins, dirs)
    n, dev = origins.numel() // 3, origins.device
    if slots.dtype != torch.int32 or tuple(slots.shape) != (n,) or not slots.is_contiguous() or slots.device != dev:
        raise ValueError("slots must be a contiguous int32 [n] tensor on the rays' device, one per ray")
    if outs is not None:
        want = ((torch.bool, (n,)), (torch.bool, (n,)), (torch.int32, (n,)), (torch.float32, (n, 3)), (torch.float32, (n, 2)))
        if len(outs) != 5 or any(t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                                 for t, (dt, sh) in zip(outs, want)):
            raise ValueError("outs must be contiguous (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on the rays' device")
        hit, front, tri, loc, uv = outs
    else:
        b = origins.shape[:-1]
        hit = _new_output(b, torch.bool, dev)
        front = _new_output(b, torch.bool, dev)
        tri = _new_output(b, torch.int32, dev)
        loc = _new_output((*b, 3), torch.float32, dev)
        uv = _new_output((*b, 2), torch.float32, dev)
    with torch.cuda.device(dev):
        _check(get_module().tr_closest_from_slots(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                                  slots.data_ptr(), int(row_length), hit.data_ptr(), front.data_ptr(),
                                                  tri.data_ptr(), loc.data_ptr(), uv.data_ptr(), _stream_ptr(dev)))
    return hit, front, tri, loc, uv


def closest_expand_slots(accel_structure, packed: torch.Tensor, batch_shape=None, outs=None, row_length: int = 0):
    """tr_closest_expand_slots: slot-form records (intersects_closest_packed(..., slots=True), of this hierarchy or of a
    bit-identical replica) -> (hit, front, tri_idx, loc, uv), bit-identical to intersects_closest on the same rays."""
    if packed.dtype != torch.int32 or packed.dim() != 2 or packed.shape[1] != 3 or not packed.is_contiguous() or not packed.is_cuda:
        raise ValueError("packed must be a contiguous int32 [n, 3] tensor on the GPU")
    dev, n = packed.device, packed.shape[0]
    if outs is not None:
        want = ((torch.bool, (n,)), (torch.bool, (n,)), (torch.int32, (n,)), (torch.float32, (n, 3)), (torch.float32, (n, 2)))
        if len(outs) != 5 or any(t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                                 for t, (dt, sh) in zip(outs, want)):
            raise ValueError("outs must be contiguous (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on the device of packed")
        hit, front, tri, loc, uv = outs
    else:
        b = tuple(batch_shape) if batch_shape is not None else (n,)
        hit = _new_output(b, torch.bool, dev)
        front = _new_output(b, torch.bool, dev)
        tri = _new_output(b, torch.int32, dev)
        loc = _new_output((*b, 3), torch.float32, dev)
        uv = _new_output((*b, 2), torch.float32, dev)
        if hit.numel() != n:
            raise ValueError(f"batch_shape {b} does not hold {n} rays")
    # row_length: the records are whole rows of an image of that width (tr_closest_expand_slots_rows: 8x8 tiles per wave)
    with torch.cuda.device(dev):
        _check(get_module().tr_closest_expand_slots_rows(_handle(accel_structure, packed), packed.data_ptr(), n, int(row_length),
                                                         hit.data_ptr(), front.data_ptr(), tri.data_ptr(), loc.data_ptr(),
                                                         uv.data_ptr(), _stream_ptr(dev)))
    return hit, front, tri, loc, uv


def closest_expand(packed: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, batch_shape=None, outs=None):
    """tr_closest_expand: packed [n, 3] int32 -> (hit, front, tri_idx, loc, uv) shaped `batch_shape`
    (default [n]), bit-identical to intersects_closest on the same rays.  vertices / faces: the float32
    [nv, 3] / int32 [nf, 3] arrays the BVH was built from, on the device of `packed`.  `outs`: optional
    preallocated contiguous destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2]
    -- e.g. row slices of full-size outputs)."""
    if packed.dtype != torch.int32 or packed.dim() != 2 or packed.shape[1] != 3 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous int32 [n, 3] tensor")
    if vertices.dtype != torch.float32 or faces.dtype != torch.int32 or not vertices.is_contiguous() or not faces.is_contiguous():
        raise ValueError("vertices must be contiguous float32 [nv, 3] and faces contiguous int32 [nf, 3]")
    dev = packed.device
    if not packed.is_cuda or vertices.device != dev or faces.device != dev:
        raise ValueError("packed, vertices and faces must live on the same GPU")
    n = packed.shape[0]
    if outs is not None:
        want = ((torch.bool, (n,)), (torch.bool, (n,)), (torch.int32, (n,)), (torch.float32, (n, 3)), (torch.float32, (n, 2)))
        if len(outs) != 5 or any(t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                                 for t, (dt, sh) in zip(outs, want)):
            raise ValueError("outs must be contiguous (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on the device of packed")
        with torch.cuda.device(dev):
            _check(get_module().tr_closest_expand(packed.data_ptr(), n, vertices.data_ptr(), vertices.shape[0],
                                                  faces.data_ptr(), faces.shape[0], *(t.data_ptr() for t in outs), _stream_ptr(dev)))
        return tuple(outs)
    b = tuple(batch_shape) if batch_shape is not None else (n,)
    hit = _new_output(b, torch.bool, dev)
    front = _new_output(b, torch.bool, dev)
    tri = _new_output(b, torch.int32, dev)
    loc = _new_output((*b, 3), torch.float32, dev)
    uv = _new_output((*b, 2), torch.float32, dev)
    if hit.numel() != n:
        raise ValueError(f"batch_shape {b} does not hold {n} rays")
    with torch.cuda.device(dev):
        _check(get_module().tr_closest_expand(packed.data_ptr(), n, vertices.data_ptr(), vertices.shape[0],
                                              faces.data_ptr(), faces.shape[0], hit.data_ptr(), front.data_ptr(),
                                              tri.data_ptr(), loc.data_ptr(), uv.data_ptr(), _stream_ptr(dev)))
    return hit, front, tri, loc, uv


def intersects_count(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:152-168 / ray.cpp:291-322.  Int32[*b]."""
    check_rays(origins, dirs)
    out = _new_output(origins.shape[:-1], torch.int32, origins.device)
    with torch.cuda.device(origins.device):
        _check(get_module().tr_intersects_count(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                                out.data_ptr(), _stream_ptr(origins.device)))
    return out


def intersects_location(accel_structure, origins, dirs, ray_base: int = 0, fused: bool = True) -> Tuple[torch.Tensor, ...]:
    """ops.py:171-192 / ray.cpp:324-378.  (loc[h,3], ray_idx[h], tri_idx[h]); at most
    MAX_ANYHIT_SIZE hits per ray, grouped by ray; within a ray ordered by distance (the
    reference leaves that order unspecified).

    fused=True (default): one traversal (count + slots of the 8 nearest hits), scan, fill from
    the slots.  fused=False: the reference's protocol, count pass -> scan -> second traversal
    (ray.cpp:330, 333-342, 372-374); both give identical results."""
    check_rays(origins, dirs)
    dev = origins.device
    lib = get_module()
    n = origins.numel() // 3
    _check_ray_idx_range(n, ray_base, "intersects_location / intersects_id")
    if fused:
        with torch.cuda.device(dev):
            stream = _stream_ptr(dev)
            rays = make_rays(origins, dirs)
            count = _new_output(n, torch.int32, dev)
            slots = _new_output((n, MAX_ANYHIT_SIZE, 2), torch.int32, dev)   # tr_hit_entry {t_key, slot}
            _check(lib.tr_intersects_count_topk(_handle(accel_structure, origins), C.byref(rays), MAX_ANYHIT_SIZE,
                                                count.data_ptr(), slots.data_ptr(), stream))
            offsets = _new_output(n, torch.int64, dev)
            total_d = _new_output(1, torch.int64, dev)
            total = C.c_int64(0)
            _check(lib.tr_hits_scan(count.data_ptr(), n, MAX_ANYHIT_SIZE, offsets.data_ptr(), total_d.data_ptr(),
                                    C.byref(total), stream))
            nhits = int(total.value)
            loc = _new_output((nhits, 3), torch.float32, dev)
            tri = _new_output(nhits, torch.int32, dev)
            ray = _new_output(nhits, torch.int32, dev)
            _check(lib.tr_location_fill_slots(_handle(accel_structure, origins), C.byref(rays), MAX_ANYHIT_SIZE,
                                              count.data_ptr(), offsets.data_ptr(), slots.data_ptr(),
                                              loc.data_ptr(), ray.data_ptr(), tri.data_ptr(), ray_base, stream))
        return loc, ray, tri
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        rays = make_rays(origins, dirs)
        count = _new_output(n, torch.int32, dev)
        _check(lib.tr_intersects_count(_handle(accel_structure, origins), C.byref(rays), count.data_ptr(), stream))
        offsets = _new_output(n, torch.int64, dev)
        total_d = _new_output(1, torch.int64, dev)
        total = C.c_int64(0)
        _check(lib.tr_hits_scan(count.data_ptr(), n, MAX_ANYHIT_SIZE, offsets.data_ptr(), total_d.data_ptr(),
                                C.byref(total), stream))   # host sync == ray.cpp:339 .item<int>()
        nhits = int(total.value)
        loc = _new_output((nhits, 3), torch.float32, dev)
        tri = _new_output(nhits, torch.int32, dev)
        ray = _new_output(nhits, torch.int32, dev)
        _check(lib.tr_intersects_location_fill(_handle(accel_structure, origins), C.byref(rays), MAX_ANYHIT_SIZE,
                                               offsets.data_ptr(), loc.data_ptr(), ray.data_ptr(),
                                               tri.data_ptr(), ray_base, stream))
    return loc, ray, tri


def _check_ray_idx_range(n: int, ray_base: int, what: str):
    """ray_idx outputs are int32 by API (ray_optix.py:143-144 `arange(..., dtype=int32)`, ray.cpp:352): a flat ray index of
    2^31 or more does not fit.  The reference's device code overflows silently far earlier (`int` arithmetic on idx * 3
    in getRay, shaders.cu:37: from 715 827 883 rays on); here the traversal is 64-bit throughout (intersects_any / first /
    closest / count take batches of 2^31 rays and more, tests/test_gpu_round6.py) and the queries that RETURN ray indices
    refuse what their output type cannot hold."""
    if n + int(ray_base) >= (1 << 31):
        raise ValueError(f"{what}: {n} rays (+ ray_base {ray_base}) reach 2^31: beyond the int32 ray_idx of the API; split the batch")


def compact_closest(hit, front, tri, loc, uv, ray_base: int = 0):
    """Fused stream compaction (ray_optix.py:142-144: five boolean-mask gathers, one host
    sync each) -> one scan + one gather kernel, one host sync for the size.
    Returns (front[h], ray_idx[h], tri[h], loc[h,3], uv[h,2])."""
    dev = hit.device
    lib = get_module()
    n = hit.numel()
    _check_ray_idx_range(n, ray_base, "stream compaction")
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        offsets = _new_output(n, torch.int64, dev)
        total_d = _new_output(1, torch.int64, dev)
        total = C.c_int64(0)
        _check(lib.tr_mask_scan(hit.data_ptr(), n, offsets.data_ptr(), total_d.data_ptr(), C.byref(total), stream))
        h = int(total.value)
        front_o = _new_output(h, torch.bool, dev) if front is not None else None
        ray_o = _new_output(h, torch.int32, dev)
        tri_o = _new_output(h, torch.int32, dev) if tri is not None else None
        loc_o = _new_output((h, 3), torch.float32, dev) if loc is not None else None
        uv_o = _new_output((h, 2), torch.float32, dev) if uv is not None else None
        p = lambda t: t.data_ptr() if t is not None else None
        _check(lib.tr_compact_closest(hit.data_ptr(), offsets.data_ptr(), n, p(front), p(tri), p(loc), p(uv),
                                      ray_base, p(front_o), ray_o.data_ptr(), p(tri_o), p(loc_o), p(uv_o), stream))
    return front_o, ray_o, tri_o, loc_o, uv_o


def trace_stats_closest(accel_structure, origins, dirs) -> dict:
    """Diagnostic: per-launch traversal counters of the instrumented closest-hit kernel."""
    check_rays(origins, dirs)
    st = TrTraceStats()
    with torch.cuda.device(origins.device):
        _check(get_module().tr_trace_stats_closest(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                                   C.byref(st), _stream_ptr(origins.device)))
    return dict(rays=st.rays, node_visits=st.node_visits, tri_tests=st.tri_tests, climb_steps=st.climb_steps)


QUERY_IDS = {"any": 0, "first": 1, "closest": 2, "count": 3, "location": 4}


def trace_stats(accel_structure, origins, dirs, query: str = "closest") -> dict:
    """Diagnostic: traversal counters of the instrumented kernel of any query."""
    check_rays(origins, dirs)
    st = TrTraceStats()
    with torch.cuda.device(origins.device):
        _check(get_module().tr_trace_stats_query(_handle(accel_structure, origins), C.byref(make_rays(origins, dirs)),
                                           QUERY_IDS[query], C.byref(st), _stream_ptr(origins.device)))
    return dict(rays=st.rays, node_visits=st.node_visits, tri_tests=st.tri_tests, climb_steps=st.climb_steps)


def device_topology(device: int = 0) -> dict:
    """tr_device_topology: what the launch policy reads from the device and the ray-count boundaries it derives"""
    t = TrTopology()
    _check(get_module().tr_device_topology(int(device), C.byref(t)))
    return {k: int(getattr(t, k)) for k, _ in TrTopology._fields_ if k != "reserved"}


def set_option(name: str, value: int):
    _check(get_module().tr_set_option(name.encode(), int(value)))


# --- the satellite libraries libtriro_<key>.so: one loader, one list protocol, the shared argument checks -------------------
class _Satellite:
    """One library libtriro_<key>.so beside libtriro_hip.so: its ABI table {symbol: (restype, argtypes)} and the loader of
    the library whose handles it works on.  The file name, the TRIRO_<KEY>_LIBRARY override, the version symbol
    tr_<key>_abi_version and the expected <KEY>_ABI_VERSION of this module (read when the library is loaded; None: the
    library has no version symbol) follow from the key.  Each section below registers its library in one line and binds
    the public names x_library_path / get_x_module to it."""

    def __init__(self, key, abi, prerequisite):
        self.key, self.abi, self.prerequisite, self.lib = key, abi, prerequisite, None

    def path(self) -> str:
        return os.environ.get(f"TRIRO_{self.key.upper()}_LIBRARY") or \
            os.path.join(os.path.dirname(library_path()), f"libtriro_{self.key}.so")

    def load(self):
        """The library, loaded once per process.  Raises when it is not built or does not match this binding."""
        if self.lib is None:
            self.prerequisite()                # libtriro_hip.so (and libtriro_scene.so) first: the library links against it
            path = self.path()
            if not os.path.exists(path):
                raise RuntimeError(f"{path} not found: build it (make -C trimesh-ray-optix_amd/csrc all, __graft_entry__.build())")
            lib = C.CDLL(path)
            for name, (res, args) in self.abi.items():
                fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            want = globals()[f"{self.key.upper()}_ABI_VERSION"]
            if want is not None:
                have = getattr(lib, f"tr_{self.key}_abi_version")()
                if have != want:
                    raise RuntimeError(f"libtriro_{self.key}.so ABI version {have} != {want} expected by this binding")
            self.lib = lib
        return self.lib


def _ptr(t):
    """the device pointer of an optional tensor: None if absent"""
    return t.data_ptr() if t is not None else None


def _ptr_rows(t):
    """the device pointer of an optional output of a fill: None if absent or empty (the fills take NULL for zero rows)"""
    return t.data_ptr() if t is not None and t.numel() else None


def _check_points(points):
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or \
            points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a float32 GPU tensor of shape [n, 3]")


def _check_pair(name_a, a, name_b, b):
    """two float32 GPU tensors [n, 3] of one shape on one device (the corners of boxes, the origins and normals of planes)"""
    for name, t in ((name_a, a), (name_b, b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be a float32 GPU tensor of shape [n, 3]")
    if b.device != a.device or b.shape != a.shape:
        raise ValueError(f"{name_a} {tuple(a.shape)} on {a.device} and {name_b} {tuple(b.shape)} on {b.device} "
                         f"must have one shape and one device")


def _any_or_count(query, satellite):
    """(the dtype of the output, the entry point) of the any / count pair of a library: bool and tr_<key>_any, or int32 and
    tr_<key>_count"""
    if query not in ("any", "count"):
        raise ValueError(f"query must be 'any' or 'count', got {query!r}")
    return (torch.bool if query == "any" else torch.int32), getattr(satellite.load(), f"tr_{satellite.key}_{query}")


def _scan_counts(count):
    """(offsets int64[n + 1], total) of a flat int32[n] count: the exclusive scan that a fill takes as offsets[:n], and one
    host read of the total to size its outputs (as intersects_location)."""
    n, dev = count.shape[0], count.device
    offsets = _new_output((n + 1,), torch.int64, dev)
    total = C.c_int64(0)
    with torch.cuda.device(dev):
        # the grand total lands in offsets[n] on the device and, after the stream is synchronised, on the host
        _check(get_module().tr_hits_scan(count.data_ptr(), n, 0x7fffffff, offsets.data_ptr(), offsets[n:].data_ptr(),
                                         C.byref(total), _stream_ptr(dev)))
    return offsets, int(total.value)


def _check_fill(count, offsets, total, n, dev, whose) -> int:
    """what every fill is given besides its queries: count int32[n], offsets int64[n] on the device of `whose` (the noun of
    the queries), and the total, returned as an int"""
    for name, t, dt in (("count", count, torch.int32), ("offsets", offsets, torch.int64)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of {n} elements on the {whose}' device")
    total = int(total)
    if total < 0:
        raise ValueError("total must not be negative")
    return total


# --- the native N-rank step (include/triro_rccl.h, csrc/gather_rccl.cpp) --------------------------------------------

class TrShardStep(C.Structure):
    """tr_shard_step of include/triro_rccl.h"""
    _fields_ = [("n_total", C.c_int64), ("world", C.c_int32), ("rank", C.c_int32), ("dst", C.c_int32), ("chunks", C.c_int32),
                ("per_row", C.c_int64), ("bounds", C.POINTER(C.c_int64)), ("my_rays", C.POINTER(TrRays)),
                ("all_rays", C.POINTER(TrRays)), ("d_records", C.c_void_p), ("d_staging", C.c_void_p), ("d_hit", C.c_void_p),
                ("d_front", C.c_void_p), ("d_tri", C.c_void_p), ("d_loc3", C.c_void_p), ("d_uv2", C.c_void_p),
                ("stream", C.c_void_p), ("side_stream", C.c_void_p), ("done_event", C.c_void_p), ("flags", C.c_int32)]


STEP_NO_EXCHANGE, STEP_LOOPBACK, STEP_TEST_DROP_SEND = 1, 2, 4
COMM_ID_BYTES = 128


RCCL_ABI_VERSION = None    # include/triro_rccl.h declares no version symbol

# the symbols of include/triro_rccl.h this binding calls: (restype, argtypes)
RCCL_ABI = {
    "tr_rccl_last_error": (C.c_char_p, []),
    "tr_rccl_available": (_int, []),
    "tr_comm_unique_id": (_int, [_vp]),
    "tr_comm_create": (_int, [_vp, _int, _int, _int, C.POINTER(_vp)]),
    "tr_comm_destroy": (_int, [_vp]),
    "tr_comm_abort": (_int, [_vp]),
    "tr_sharded_closest_step": (_int, [_vp, _vp, C.POINTER(TrShardStep)]),
}

# one C call per pipelined step of a ray-sharded closest-hit query.  get_rccl_module raises when the library is not built;
# whether RCCL itself can be found is a question for rccl_available()
_rccl = _Satellite("rccl", RCCL_ABI, get_module)
rccl_library_path = _rccl.path
get_rccl_module = _rccl.load


def rccl_available() -> bool:
    try:
        return get_rccl_module().tr_rccl_available() == 0
    except Exception:
        return False


def _check_rccl(rc: int):
    if rc != 0:
        raise RuntimeError("libtriro_rccl: " + (get_rccl_module().tr_rccl_last_error() or b"?").decode())


# --- contains_points as one launch (include/triro_points.h, csrc/points.hip) ------------------------------------------
POINTS_ABI_VERSION = 1    # TR_POINTS_ABI_VERSION of include/triro_points.h

# every symbol include/triro_points.h declares: (restype, argtypes)
POINTS_ABI = {
    "tr_points_abi_version": (_int, []),
    "tr_contains_addressing": (_int, [_vp]),
    "tr_contains_points": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
}


_points = _Satellite("points", POINTS_ABI, get_module)
points_library_path = _points.path
get_points_module = _points.load


def contains_addressing(accel_structure) -> int:
    """the instantiation of k_contains_points a call on this handle takes now: 0 generic, 1 compact, 2 deep"""
    return int(get_points_module().tr_contains_addressing(_handle(accel_structure)))


def contains_points_native(accel_structure, points, direction, box_lo, box_hi, want_counts=False):
    """tr_contains_points: (inside bool[n], broken bool[n], counts int32[2, n] or None, summary int64[2] = {points in the
    box, broken points}) for float32 points [n, 3] and 3-float device tensors direction / box_lo / box_hi (both boxes None:
    no box test).  Nothing is synchronised: the caller reads `summary` when it needs it."""
    _check_points(points)
    dev = points.device
    handle = _handle(accel_structure, points)
    points = points.contiguous()
    small = [direction, box_lo, box_hi]
    if (box_lo is None) != (box_hi is None):
        raise ValueError("box_lo and box_hi must both be given or both be None")
    for k, t in enumerate(small):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.numel() != 3:
            raise ValueError("direction, box_lo and box_hi must be tensors of 3 elements")
        small[k] = t.to(device=dev, dtype=torch.float32).contiguous()
    direction, box_lo, box_hi = small
    n = points.shape[0]
    inside = _new_output((n,), torch.bool, dev)
    broken = _new_output((n,), torch.bool, dev)
    counts = _new_output((2, n), torch.int32, dev) if want_counts else None
    summary = _new_output((2,), torch.int64, dev)
    with torch.cuda.device(dev):
        _check(get_points_module().tr_contains_points(
            handle, points.data_ptr(), n, direction.data_ptr(), _ptr(box_lo), _ptr(box_hi),
            inside.data_ptr(), broken.data_ptr(), _ptr(counts), summary.data_ptr(), None, _stream_ptr(dev)))
    return inside, broken, counts, summary


# --- closest_point as one launch (include/triro_nearest.h, csrc/nearest.hip) -------------------------------------------
NEAREST_ABI_VERSION = 1    # TR_NEAREST_ABI_VERSION of include/triro_nearest.h

# every symbol include/triro_nearest.h declares: (restype, argtypes)
NEAREST_ABI = {
    "tr_nearest_abi_version": (_int, []),
    "tr_nearest_stack_capacity": (_int, []),
    "tr_closest_point": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _int, _vp]),
}


_nearest = _Satellite("nearest", NEAREST_ABI, get_module)
nearest_library_path = _nearest.path
get_nearest_module = _nearest.load


def closest_point_native(accel_structure, points, stack_entries=0, want_closest=True, want_distance=True):
    """tr_closest_point: (closest float32[n, 3] or None, distance float32[n] or None, tri int32[n]) for float32 points
    [n, 3] on the handle's GPU.  stack_entries: 0 = the whole far-child stack, 1 .. capacity for tests (same results).
    Nothing is allocated by the library and nothing is synchronised."""
    _check_points(points)
    lib = get_nearest_module()
    dev = points.device
    handle = _handle(accel_structure, points)
    points = points.contiguous()
    n = points.shape[0]
    closest = _new_output((n, 3), torch.float32, dev) if want_closest else None
    distance = _new_output((n,), torch.float32, dev) if want_distance else None
    tri = _new_output((n,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_closest_point(handle, points.data_ptr(), n, _ptr(closest), _ptr(distance), tri.data_ptr(),
                                    int(stack_entries), _stream_ptr(dev)))
    return closest, distance, tri


# --- any / closest on a per-ray interval [tmin, tmax] (include/triro_range.h, csrc/range.hip) --------------------------
RANGE_ABI_VERSION = 1    # TR_RANGE_ABI_VERSION of include/triro_range.h

# every symbol include/triro_range.h declares: (restype, argtypes)
RANGE_ABI = {
    "tr_range_abi_version": (_int, []),
    "tr_range_stack_capacity": (_int, []),
    "tr_range_any": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _int, _vp]),
    "tr_range_closest": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
}


_range = _Satellite("range", RANGE_ABI, get_module)
range_library_path = _range.path
get_range_module = _range.load


def _range_bound(t, name, n, dev):
    """a bound of the range queries: None (the default) or a dense float32 [n] tensor on the rays' device"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.float32 or \
            tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f"{name} must be None or a contiguous float32 tensor of {n} elements on the rays' device")
    return t


def range_any_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_range_any: bool[*b], is anything hit within [tmin, tmax] (closed, measured from the origin given, no anchoring).
    Rays as for intersects_any (any strides); tmin / tmax: None or dense float32 [n], n = the number of rays.
    stack_entries: 0 = the whole far-child stack, 1 .. capacity for tests (same results).  Nothing is allocated by the
    library and nothing is synchronised."""
    check_rays(origins, dirs)
    lib = get_range_module()
    dev, n = origins.device, origins.numel() // 3
    handle = _handle(accel_structure, origins)
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    out = _new_output(origins.shape[:-1], torch.bool, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_range_any(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), out.data_ptr(), int(stack_entries),
                                _stream_ptr(dev)))
    return out


def range_closest_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0, want_t=True, want_dense=True):
    """tr_range_closest: (hit bool[*b], front bool[*b], tri int32[*b], loc float32[*b, 3], uv float32[*b, 2], t float32[*b])
    of the first hit within [tmin, tmax]; a miss is (False, False, -1, 0, 0, +Inf).  want_t=False: t is None;
    want_dense=False: hit, front, loc and uv are None (tri, and t, alone).  Arguments as range_any_native."""
    check_rays(origins, dirs)
    lib = get_range_module()
    b, dev, n = origins.shape[:-1], origins.device, origins.numel() // 3
    handle = _handle(accel_structure, origins)
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    tri = _new_output(b, torch.int32, dev)
    t = _new_output(b, torch.float32, dev) if want_t else None
    hit = _new_output(b, torch.bool, dev) if want_dense else None
    front = _new_output(b, torch.bool, dev) if want_dense else None
    loc = _new_output((*b, 3), torch.float32, dev) if want_dense else None
    uv = _new_output((*b, 2), torch.float32, dev) if want_dense else None
    with torch.cuda.device(dev):
        _check(lib.tr_range_closest(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), tri.data_ptr(), _ptr(t), _ptr(hit),
                                    _ptr(front), _ptr(loc), _ptr(uv), int(stack_entries), _stream_ptr(dev)))
    return hit, front, tri, loc, uv, t


# --- any / closest over placed copies of several meshes (include/triro_scene.h, csrc/scene.hip) --------------------------
SCENE_ABI_VERSION = 1    # TR_SCENE_ABI_VERSION of include/triro_scene.h


class TrSceneInfo(C.Structure):
    """tr_scene_info_t (include/triro_scene.h)"""
    _fields_ = [("device", C.c_int32), ("stack_capacity", C.c_int32), ("num_members", C.c_int64), ("num_instances", C.c_int64),
                ("valid_instances", C.c_int64), ("table_bytes", C.c_int64), ("commits", C.c_int64)]


# every symbol include/triro_scene.h declares: (restype, argtypes)
SCENE_ABI = {
    "tr_scene_abi_version": (_int, []),
    "tr_scene_create": (_int, [_int, C.POINTER(_vp)]),
    "tr_scene_destroy": (_int, [_vp]),
    "tr_scene_commit": (_int, [_vp, C.POINTER(_vp), _i64, _vp, _vp, _i64, _vp]),
    "tr_scene_info": (_int, [_vp, C.POINTER(TrSceneInfo)]),
    "tr_scene_any": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _int, _vp]),
    "tr_scene_closest": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
}


_scene = _Satellite("scene", SCENE_ABI, get_module)
scene_library_path = _scene.path
get_scene_module = _scene.load


def scene_create(device_index: int) -> int:
    """tr_scene_create: an empty scene on cuda:device_index; the handle (an integer) is the caller's to scene_destroy"""
    handle = C.c_void_p()
    _check(get_scene_module().tr_scene_create(int(device_index), C.byref(handle)))
    return handle.value


def scene_destroy(handle):
    if handle:
        get_scene_module().tr_scene_destroy(handle)


def scene_commit(handle, member_handles, mesh_of_instance, transforms, device_index: int):
    """tr_scene_commit: member_handles a list of tr_bvh* (integers), mesh_of_instance int32 [n] and transforms float32
    [n, 12] HOST numpy arrays.  The one scene call that allocates, copies and synchronises (the current stream)."""
    import numpy as np
    mesh_of = np.ascontiguousarray(mesh_of_instance, np.int32).reshape(-1)
    M = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
    if len(M) != len(mesh_of):
        raise ValueError(f"{len(mesh_of)} instances but {len(M)} transforms")
    for k, h in enumerate(member_handles):
        if not h:
            raise RuntimeError(f"member {k}: its acceleration structure has not been built")
    members = (_vp * max(len(member_handles), 1))(*member_handles)
    with torch.cuda.device(device_index):
        _check(get_scene_module().tr_scene_commit(handle, members, len(member_handles), mesh_of.ctypes.data, M.ctypes.data, len(mesh_of),
                                                  _stream_ptr(torch.device("cuda", device_index))))


def scene_info(handle) -> dict:
    inf = TrSceneInfo()
    _check(get_scene_module().tr_scene_info(handle, C.byref(inf)))
    return {k: int(getattr(inf, k)) for k, _ in inf._fields_}


def _scene_rays(origins, dirs, device_index):
    check_rays(origins, dirs)
    if origins.device.index != device_index:
        raise ValueError(f"rays are on {origins.device} but the scene lives on cuda:{device_index}; move the rays")


def scene_any_native(handle, device_index, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_scene_any: bool[*b], does any instance have a hit within [tmin, tmax] of the world ray.  Arguments as
    range_any_native, with the scene handle and its device in place of the acceleration structure.  Nothing is allocated
    by the library and nothing is synchronised."""
    _scene_rays(origins, dirs, device_index)
    lib = get_scene_module()
    dev, n = origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    out = _new_output(origins.shape[:-1], torch.bool, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_any(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), out.data_ptr(), int(stack_entries),
                                _stream_ptr(dev)))
    return out


def scene_closest_native(handle, device_index, origins, dirs, tmin=None, tmax=None, stack_entries=0, want_t=True, want_dense=True):
    """tr_scene_closest: (hit bool[*b], front bool[*b], instance int32[*b], tri int32[*b], t float32[*b], loc float32[*b, 3],
    uv float32[*b, 2]) of the first hit within [tmin, tmax] over all instances; a miss is (False, False, -1, -1, +Inf, 0, 0).
    want_t=False: t is None; want_dense=False: hit, front, loc and uv are None (instance, tri and t alone)."""
    _scene_rays(origins, dirs, device_index)
    lib = get_scene_module()
    b, dev, n = origins.shape[:-1], origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    inst = _new_output(b, torch.int32, dev)
    tri = _new_output(b, torch.int32, dev)
    t = _new_output(b, torch.float32, dev) if want_t else None
    hit = _new_output(b, torch.bool, dev) if want_dense else None
    front = _new_output(b, torch.bool, dev) if want_dense else None
    loc = _new_output((*b, 3), torch.float32, dev) if want_dense else None
    uv = _new_output((*b, 2), torch.float32, dev) if want_dense else None
    with torch.cuda.device(dev):
        _check(lib.tr_scene_closest(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), inst.data_ptr(), tri.data_ptr(), _ptr(t),
                                    _ptr(hit), _ptr(front), _ptr(loc), _ptr(uv), int(stack_entries), _stream_ptr(dev)))
    return hit, front, inst, tri, t, loc, uv


# --- the faces within a distance of each point (include/triro_within.h, csrc/within.hip) -------------------------------
WITHIN_ABI_VERSION = 1    # TR_WITHIN_ABI_VERSION of include/triro_within.h
_f32 = C.c_float

# every symbol include/triro_within.h declares: (restype, argtypes)
WITHIN_ABI = {
    "tr_within_abi_version": (_int, []),
    "tr_within_stack_capacity": (_int, []),
    "tr_within_any": (_int, [_vp, _vp, _i64, _vp, _f32, _vp, _int, _vp]),
    "tr_within_count": (_int, [_vp, _vp, _i64, _vp, _f32, _vp, _int, _vp]),
    "tr_within_fill": (_int, [_vp, _vp, _i64, _vp, _f32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _vp]),
    "tr_within_closest": (_int, [_vp, _vp, _i64, _vp, _f32, _vp, _vp, _vp, _int, _vp]),
}


_within = _Satellite("within", WITHIN_ABI, get_module)
within_library_path = _within.path
get_within_module = _within.load


def _within_args(accel_structure, points, radius):
    """(handle, contiguous points, n, device, radius pointer or None, scalar radius, the radius tensor kept alive)"""
    _check_points(points)
    dev, n = points.device, points.shape[0]
    handle = _handle(accel_structure, points)
    if isinstance(radius, torch.Tensor):
        if not radius.is_cuda or radius.device != dev or radius.dtype != torch.float32 or tuple(radius.shape) != (n,) or \
                not radius.is_contiguous():
            raise ValueError(f"radius must be a number or a contiguous float32 tensor of {n} elements on the points' device")
        return handle, points.contiguous(), n, dev, radius.data_ptr(), 0.0, radius
    r = C.c_float(float(radius)).value      # rounded to float32 (beyond its range: +Inf, as a float32 tensor would hold it)
    return handle, points.contiguous(), n, dev, None, r, None


def within_native(accel_structure, points, radius, query="any", stack_entries=0) -> torch.Tensor:
    """tr_within_any (query="any": bool[n]) / tr_within_count (query="count": int32[n]) for float32 points [n, 3] on the
    handle's GPU.  radius: a number, or a dense float32 [n] tensor on that GPU.  stack_entries: 0 = the whole stack,
    1 .. capacity for tests (same results).  Nothing is allocated by the library and nothing is synchronised."""
    dtype, fn = _any_or_count(query, _within)
    handle, points, n, dev, rptr, r, _keep = _within_args(accel_structure, points, radius)
    out = _new_output((n,), dtype, dev)
    with torch.cuda.device(dev):
        _check(fn(handle, points.data_ptr(), n, rptr, r, out.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return out


def within_fill_native(accel_structure, points, radius, count, offsets, total, want_distance=False, want_closest=False,
                       stack_entries=0):
    """tr_within_fill: (face int32[total], distance float32[total] or None, closest float32[total, 3] or None), the faces of
    point i ascending at rows offsets[i] .. offsets[i] + count[i].  count int32[n] is within_native(..., "count") and
    offsets int64[n] its exclusive scan (tr_hits_scan) for the same points and radii; total (a Python int) sizes the
    outputs.  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_within_module()
    handle, points, n, dev, rptr, r, _keep = _within_args(accel_structure, points, radius)
    total = _check_fill(count, offsets, total, n, dev, "points")
    face = _new_output((total,), torch.int32, dev)
    distance = _new_output((total,), torch.float32, dev) if want_distance else None
    closest = _new_output((total, 3), torch.float32, dev) if want_closest else None
    slot = _new_output((total,), torch.int32, dev) if (want_distance or want_closest) and total > 0 else None
    with torch.cuda.device(dev):
        _check(lib.tr_within_fill(handle, points.data_ptr(), n, rptr, r, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(face),
                                  _ptr_rows(distance), _ptr_rows(closest), _ptr_rows(slot), int(stack_entries), _stream_ptr(dev)))
    return face, distance, closest


def faces_within_native(accel_structure, points, radius, want_distance=False, want_closest=False, stack_entries=0):
    """(offsets int64[n + 1], face, distance or None, closest or None): one count launch, one scan, one host read of the
    total to size the outputs (as intersects_location), one fill."""
    handle, points, n, dev, rptr, r, keep = _within_args(accel_structure, points, radius)
    radius = keep if keep is not None else r
    count = within_native(accel_structure, points, radius, "count", stack_entries)
    offsets, total = _scan_counts(count)
    face, distance, closest = within_fill_native(accel_structure, points, radius, count, offsets[:n], total,
                                                 want_distance, want_closest, stack_entries)
    return offsets, face, distance, closest


def within_closest_native(accel_structure, points, radius, stack_entries=0, want_closest=True, want_distance=True):
    """tr_within_closest: closest_point_native bounded by the radius -- (closest float32[n, 3] or None, distance float32[n]
    or None, tri int32[n]), (NaN, +Inf, -1) where no face is within.  radius as for within_native."""
    lib = get_within_module()
    handle, points, n, dev, rptr, r, _keep = _within_args(accel_structure, points, radius)
    closest = _new_output((n, 3), torch.float32, dev) if want_closest else None
    distance = _new_output((n,), torch.float32, dev) if want_distance else None
    tri = _new_output((n,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_within_closest(handle, points.data_ptr(), n, rptr, r, _ptr(closest), _ptr(distance), tri.data_ptr(),
                                     int(stack_entries), _stream_ptr(dev)))
    return closest, distance, tri


# --- the faces that meet each axis-aligned box (include/triro_boxes.h, csrc/boxes.hip) ------------------------------------
BOXES_ABI_VERSION = 1    # TR_BOXES_ABI_VERSION of include/triro_boxes.h

# every symbol include/triro_boxes.h declares: (restype, argtypes)
BOXES_ABI = {
    "tr_boxes_abi_version": (_int, []),
    "tr_boxes_stack_capacity": (_int, []),
    "tr_boxes_any": (_int, [_vp, _vp, _vp, _i64, _vp, _int, _vp]),
    "tr_boxes_count": (_int, [_vp, _vp, _vp, _i64, _vp, _int, _vp]),
    "tr_boxes_fill": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _int, _vp]),
}


_boxes = _Satellite("boxes", BOXES_ABI, get_module)
boxes_library_path = _boxes.path
get_boxes_module = _boxes.load


def _boxes_args(accel_structure, lo, hi):
    """(handle, contiguous lo, contiguous hi, n, device)"""
    _check_pair("lo", lo, "hi", hi)
    return _handle(accel_structure, lo), lo.contiguous(), hi.contiguous(), lo.shape[0], lo.device


def boxes_native(accel_structure, lo, hi, query="any", stack_entries=0) -> torch.Tensor:
    """tr_boxes_any (query="any": bool[n]) / tr_boxes_count (query="count": int32[n]) for the closed boxes [lo, hi], float32
    [n, 3] each, on the handle's GPU.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing
    is allocated by the library and nothing is synchronised."""
    dtype, fn = _any_or_count(query, _boxes)
    handle, lo, hi, n, dev = _boxes_args(accel_structure, lo, hi)
    out = _new_output((n,), dtype, dev)
    with torch.cuda.device(dev):
        _check(fn(handle, lo.data_ptr(), hi.data_ptr(), n, out.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return out


def boxes_fill_native(accel_structure, lo, hi, count, offsets, total, want_inside=False, stack_entries=0):
    """tr_boxes_fill: (face int32[total], inside bool[total] or None), the faces of box i ascending at rows offsets[i] ..
    offsets[i] + count[i].  count int32[n] is boxes_native(..., "count") and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same boxes; total (a Python int) sizes the outputs.  Nothing is allocated by the library and
    nothing is synchronised."""
    lib = get_boxes_module()
    handle, lo, hi, n, dev = _boxes_args(accel_structure, lo, hi)
    total = _check_fill(count, offsets, total, n, dev, "boxes")
    face = _new_output((total,), torch.int32, dev)
    inside = _new_output((total,), torch.bool, dev) if want_inside else None
    with torch.cuda.device(dev):
        _check(lib.tr_boxes_fill(handle, lo.data_ptr(), hi.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(face),
                                 _ptr_rows(inside), int(stack_entries), _stream_ptr(dev)))
    return face, inside


def faces_in_boxes_native(accel_structure, lo, hi, want_inside=False, stack_entries=0):
    """(offsets int64[n + 1], face, inside or None): one count launch, one scan, one host read of the total to size the
    outputs (as faces_within_native), one fill."""
    handle, lo, hi, n, dev = _boxes_args(accel_structure, lo, hi)
    count = boxes_native(accel_structure, lo, hi, "count", stack_entries)
    offsets, total = _scan_counts(count)
    face, inside = boxes_fill_native(accel_structure, lo, hi, count, offsets[:n], total, want_inside, stack_entries)
    return offsets, face, inside


# --- the faces that meet each query triangle (include/triro_tris.h, csrc/tris.hip) ----------------------------------------
TRIS_ABI_VERSION = 1    # TR_TRIS_ABI_VERSION of include/triro_tris.h

# every symbol include/triro_tris.h declares: (restype, argtypes)
TRIS_ABI = {
    "tr_tris_abi_version": (_int, []),
    "tr_tris_stack_capacity": (_int, []),
    "tr_tris_any": (_int, [_vp, _vp, _i64, _vp, _int, _vp]),
    "tr_tris_count": (_int, [_vp, _vp, _i64, _vp, _int, _vp]),
    "tr_tris_fill": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _int, _vp]),
}


_tris = _Satellite("tris", TRIS_ABI, get_module)
tris_library_path = _tris.path
get_tris_module = _tris.load


def _tris_args(accel_structure, tri):
    """(handle, contiguous triangles, n, device)"""
    if not isinstance(tri, torch.Tensor) or not tri.is_cuda or tri.dtype != torch.float32 or tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3):
        raise ValueError("triangles must be a float32 GPU tensor of shape [n, 3, 3]")
    return _handle(accel_structure, tri), tri.contiguous(), tri.shape[0], tri.device


def tris_native(accel_structure, tri, query="any", stack_entries=0) -> torch.Tensor:
    """tr_tris_any (query="any": bool[n]) / tr_tris_count (query="count": int32[n]) for the query triangles, float32 [n, 3, 3],
    on the handle's GPU.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing is allocated
    by the library and nothing is synchronised."""
    dtype, fn = _any_or_count(query, _tris)
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    out = _new_output((n,), dtype, dev)
    with torch.cuda.device(dev):
        _check(fn(handle, tri.data_ptr(), n, out.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return out


def tris_fill_native(accel_structure, tri, count, offsets, total, stack_entries=0) -> torch.Tensor:
    """tr_tris_fill: face int32[total], the faces of query i ascending at rows offsets[i] .. offsets[i] + count[i].  count
    int32[n] is tris_native(..., "count") and offsets int64[n] its exclusive scan (tr_hits_scan) for the same queries; total (a
    Python int) sizes the output.  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_tris_module()
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    total = _check_fill(count, offsets, total, n, dev, "triangles")
    face = _new_output((total,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_tris_fill(handle, tri.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total,
                                _ptr_rows(face), int(stack_entries), _stream_ptr(dev)))
    return face


def faces_meeting_triangles_native(accel_structure, tri, stack_entries=0):
    """(offsets int64[n + 1], face int32[h]): one count launch, one scan, one host read of the total to size the output (as
    faces_in_boxes_native), one fill."""
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    count = tris_native(accel_structure, tri, "count", stack_entries)
    offsets, total = _scan_counts(count)
    face = tris_fill_native(accel_structure, tri, count, offsets[:n], total, stack_entries)
    return offsets, face


# --- the faces that each plane meets or cuts, and the section segments (include/triro_planes.h, csrc/planes.hip) -----------
PLANES_ABI_VERSION = 1    # TR_PLANES_ABI_VERSION of include/triro_planes.h

# every symbol include/triro_planes.h declares: (restype, argtypes)
PLANES_ABI = {
    "tr_planes_abi_version": (_int, []),
    "tr_planes_frontier_capacity": (_int, []),
    "tr_planes_any": (_int, [_vp, _vp, _vp, _i64, _vp, _int, _int, _vp]),
    "tr_planes_count": (_int, [_vp, _vp, _vp, _i64, _vp, _int, _int, _vp]),
    "tr_planes_fill": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _int, _int, _vp]),
    "tr_planes_order": (_int, [_int, _i64, _vp, _vp, _i64, _vp, _vp]),
}


_planes = _Satellite("planes", PLANES_ABI, get_module)
planes_library_path = _planes.path
get_planes_module = _planes.load


def _planes_args(accel_structure, origins, normals):
    """(handle, contiguous origins, contiguous normals, n, device)"""
    _check_pair("origins", origins, "normals", normals)
    return _handle(accel_structure, origins), origins.contiguous(), normals.contiguous(), origins.shape[0], origins.device


def planes_native(accel_structure, origins, normals, query="any", cut=False, frontier_entries=0) -> torch.Tensor:
    """tr_planes_any (query="any": bool[n]) / tr_planes_count (query="count": int32[n]) for the planes (origin, normal), float32
    [n, 3] each, on the handle's GPU.  cut: the faces the plane CUTS (those that own a row of the section) instead of the faces
    it meets.  frontier_entries: 0 = the whole frontier, 1 .. capacity for tests (same results).  Nothing is allocated by the
    library and nothing is synchronised."""
    dtype, fn = _any_or_count(query, _planes)
    handle, origins, normals, n, dev = _planes_args(accel_structure, origins, normals)
    out = _new_output((n,), dtype, dev)
    with torch.cuda.device(dev):
        _check(fn(handle, origins.data_ptr(), normals.data_ptr(), n, out.data_ptr(), 1 if cut else 0, int(frontier_entries),
                  _stream_ptr(dev)))
    return out


def planes_fill_native(accel_structure, origins, normals, count, offsets, total, cut=False, want_segments=False, frontier_entries=0):
    """tr_planes_fill: (face int32[total], segments float32[total, 2, 3] or None), the faces of plane i ascending at rows
    offsets[i] .. offsets[i] + count[i].  count int32[n] is planes_native(..., "count", cut) and offsets int64[n] its exclusive
    scan (tr_hits_scan) for the same planes; total (a Python int) sizes the outputs.  Segments need cut.  Nothing is allocated
    by the library and nothing is synchronised."""
    lib = get_planes_module()
    handle, origins, normals, n, dev = _planes_args(accel_structure, origins, normals)
    total = _check_fill(count, offsets, total, n, dev, "planes")
    if want_segments and not cut:
        raise ValueError("segments are those of the cut faces: want_segments needs cut=True")
    face = _new_output((total,), torch.int32, dev)
    segments = _new_output((total, 2, 3), torch.float32, dev) if want_segments else None
    with torch.cuda.device(dev):
        _check(lib.tr_planes_fill(handle, origins.data_ptr(), normals.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total,
                                  _ptr_rows(face), _ptr_rows(segments), 1 if cut else 0, int(frontier_entries), _stream_ptr(dev)))
    return face, segments


def faces_on_planes_native(accel_structure, origins, normals, cut=False, want_segments=False, frontier_entries=0):
    """(offsets int64[n + 1], face, segments or None): one count launch, one scan, one host read of the total to size the
    outputs (as faces_in_boxes_native), one fill."""
    handle, origins, normals, n, dev = _planes_args(accel_structure, origins, normals)
    count = planes_native(accel_structure, origins, normals, "count", cut, frontier_entries)
    offsets, total = _scan_counts(count)
    face, segments = planes_fill_native(accel_structure, origins, normals, count, offsets[:n], total, cut, want_segments,
                                        frontier_entries)
    return offsets, face, segments


# --- every crossing of a ray on a per-ray interval [tmin, tmax] (include/triro_cross.h, csrc/cross.hip) -------------------
CROSS_ABI_VERSION = 1    # TR_CROSS_ABI_VERSION of include/triro_cross.h

# every symbol include/triro_cross.h declares: (restype, argtypes)
CROSS_ABI = {
    "tr_cross_abi_version": (_int, []),
    "tr_cross_stack_capacity": (_int, []),
    "tr_cross_count": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _int, _vp]),
    "tr_cross_fill": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _int, _vp]),
}


_cross = _Satellite("cross", CROSS_ABI, get_module)
cross_library_path = _cross.path
get_cross_module = _cross.load


def cross_count_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_cross_count: int32[*b], how many triangles each ray crosses within [tmin, tmax] (closed, measured from the origin
    given, no anchoring), uncapped.  Rays as for intersects_any (any strides); tmin / tmax: None or dense float32 [n], n =
    the number of rays.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing is allocated by
    the library and nothing is synchronised."""
    check_rays(origins, dirs)
    lib = get_cross_module()
    dev, n = origins.device, origins.numel() // 3
    handle = _handle(accel_structure, origins)
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    out = _new_output(origins.shape[:-1], torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_cross_count(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), out.data_ptr(), int(stack_entries),
                                  _stream_ptr(dev)))
    return out


def cross_fill_native(accel_structure, origins, dirs, tmin, tmax, count, offsets, total, want_front=False, want_loc=False,
                      want_uv=False, want_ray=False, ray_base: int = 0, stack_entries=0):
    """tr_cross_fill: (face int32[total], t float32[total], front bool[total] or None, loc float32[total, 3] or None,
    uv float32[total, 2] or None, ray int64[total] or None): the crossings of ray i by (t, face) ascending at rows offsets[i]
    .. offsets[i] + count[i].  count int32[n] is cross_count_native's (flattened) and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same rays and bounds; total (a Python int) sizes the outputs.  Nothing is allocated by the library
    and nothing is synchronised."""
    check_rays(origins, dirs)
    lib = get_cross_module()
    dev, n = origins.device, origins.numel() // 3
    handle = _handle(accel_structure, origins)
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    total = _check_fill(count, offsets, total, n, dev, "rays")
    face = _new_output((total,), torch.int32, dev)
    t = _new_output((total,), torch.float32, dev)
    front = _new_output((total,), torch.bool, dev) if want_front else None
    loc = _new_output((total, 3), torch.float32, dev) if want_loc else None
    uv = _new_output((total, 2), torch.float32, dev) if want_uv else None
    ray = _new_output((total,), torch.int64, dev) if want_ray else None
    slot = _new_output((total,), torch.int32, dev) if (want_front or want_loc or want_uv) and total > 0 else None
    with torch.cuda.device(dev):
        _check(lib.tr_cross_fill(handle, C.byref(make_rays(origins, dirs)), _ptr_rows(tmin), _ptr_rows(tmax), count.data_ptr(),
                                 offsets.data_ptr(), total, _ptr_rows(face), _ptr_rows(t), _ptr_rows(front), _ptr_rows(loc),
                                 _ptr_rows(uv), _ptr_rows(ray), int(ray_base), _ptr_rows(slot), int(stack_entries), _stream_ptr(dev)))
    return face, t, front, loc, uv, ray


def cross_all_native(accel_structure, origins, dirs, tmin=None, tmax=None, want_front=False, want_loc=False, want_uv=False,
                     want_ray=False, ray_base: int = 0, stack_entries=0):
    """(offsets int64[n + 1], face, t, front or None, loc or None, uv or None, ray or None) for the rays flattened in order:
    one count launch, one scan, one host read of the total to size the outputs (as faces_within_native), one fill."""
    count = cross_count_native(accel_structure, origins, dirs, tmin, tmax, stack_entries).reshape(-1)
    offsets, total = _scan_counts(count)
    return (offsets,) + cross_fill_native(accel_structure, origins, dirs, tmin, tmax, count, offsets[:-1], total, want_front,
                                          want_loc, want_uv, want_ray, ray_base, stack_entries)


# --- every crossing of a world ray over an instanced scene (include/triro_scene_cross.h, csrc/scene_cross.hip) ------------
SCENE_CROSS_ABI_VERSION = 1    # TR_SCENE_CROSS_ABI_VERSION of include/triro_scene_cross.h

# every symbol include/triro_scene_cross.h declares: (restype, argtypes)
SCENE_CROSS_ABI = {
    "tr_scene_cross_abi_version": (_int, []),
    "tr_scene_cross_stack_capacity": (_int, []),
    "tr_scene_cross_count": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _int, _vp]),
    "tr_scene_cross_fill": (_int, [_vp, C.POINTER(TrRays), _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _int, _vp]),
}


_scene_cross = _Satellite("scene_cross", SCENE_CROSS_ABI, get_scene_module)      # the scene handles are libtriro_scene.so's
scene_cross_library_path = _scene_cross.path
get_scene_cross_module = _scene_cross.load


def scene_cross_count_native(handle, device_index, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_scene_cross_count: int32[*b], how many (instance, triangle) pairs each world ray crosses within [tmin, tmax],
    uncapped.  Arguments as scene_any_native.  Nothing is allocated by the library and nothing is synchronised."""
    _scene_rays(origins, dirs, device_index)
    lib = get_scene_cross_module()
    dev, n = origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    out = _new_output(origins.shape[:-1], torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_cross_count(handle, C.byref(make_rays(origins, dirs)), _ptr(tmin), _ptr(tmax), out.data_ptr(), int(stack_entries),
                                        _stream_ptr(dev)))
    return out


def scene_cross_fill_native(handle, device_index, origins, dirs, tmin, tmax, count, offsets, total, want_front=False, want_loc=False,
                            want_uv=False, want_ray=False, ray_base: int = 0, stack_entries=0):
    """tr_scene_cross_fill: (instance int32[total], face int32[total], t float32[total], front bool[total] or None,
    loc float32[total, 3] or None, uv float32[total, 2] or None, ray int64[total] or None): the crossings of ray i by
    (t, instance, face) ascending at rows offsets[i] .. offsets[i] + count[i].  count int32[n] is scene_cross_count_native's
    (flattened) and offsets int64[n] its exclusive scan (tr_hits_scan) for the same rays and bounds; total (a Python int)
    sizes the outputs.  Nothing is allocated by the library and nothing is synchronised."""
    _scene_rays(origins, dirs, device_index)
    lib = get_scene_cross_module()
    dev, n = origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    total = _check_fill(count, offsets, total, n, dev, "rays")
    inst = _new_output((total,), torch.int32, dev)
    face = _new_output((total,), torch.int32, dev)
    t = _new_output((total,), torch.float32, dev)
    front = _new_output((total,), torch.bool, dev) if want_front else None
    loc = _new_output((total, 3), torch.float32, dev) if want_loc else None
    uv = _new_output((total, 2), torch.float32, dev) if want_uv else None
    ray = _new_output((total,), torch.int64, dev) if want_ray else None
    slot = _new_output((total,), torch.int32, dev) if (want_front or want_loc or want_uv) and total > 0 else None
    with torch.cuda.device(dev):
        _check(lib.tr_scene_cross_fill(handle, C.byref(make_rays(origins, dirs)), _ptr_rows(tmin), _ptr_rows(tmax), count.data_ptr(),
                                       offsets.data_ptr(), total, _ptr_rows(inst), _ptr_rows(face), _ptr_rows(t), _ptr_rows(front),
                                       _ptr_rows(loc), _ptr_rows(uv), _ptr_rows(ray), int(ray_base), _ptr_rows(slot), int(stack_entries),
                                       _stream_ptr(dev)))
    return inst, face, t, front, loc, uv, ray


def scene_cross_all_native(handle, device_index, origins, dirs, tmin=None, tmax=None, want_front=False, want_loc=False, want_uv=False,
                           want_ray=False, ray_base: int = 0, stack_entries=0):
    """(offsets int64[n + 1], instance, face, t, front or None, loc or None, uv or None, ray or None) for the rays flattened
    in order: one count launch, one scan, one host read of the total to size the outputs, one fill: as cross_all_native."""
    count = scene_cross_count_native(handle, device_index, origins, dirs, tmin, tmax, stack_entries).reshape(-1)
    offsets, total = _scan_counts(count)
    return (offsets,) + scene_cross_fill_native(handle, device_index, origins, dirs, tmin, tmax, count, offsets[:-1], total,
                                                want_front, want_loc, want_uv, want_ray, ray_base, stack_entries)


# --- which instances of a scene hold a point (include/triro_scene_points.h, csrc/scene_points.hip) -------------------------
SCENE_POINTS_ABI_VERSION = 1    # TR_SCENE_POINTS_ABI_VERSION of include/triro_scene_points.h

# every symbol include/triro_scene_points.h declares: (restype, argtypes)
SCENE_POINTS_ABI = {
    "tr_scene_points_abi_version": (_int, []),
    "tr_scene_points_stack_capacity": (_int, []),
    "tr_scene_points_any": (_int, [_vp, _vp, _i64, _vp, _vp, _int, _vp]),
    "tr_scene_points_count": (_int, [_vp, _vp, _i64, _vp, _vp, _int, _vp]),
    "tr_scene_points_fill": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _int, _vp]),
}


_scene_points = _Satellite("scene_points", SCENE_POINTS_ABI, get_scene_module)   # the scene handles are libtriro_scene.so's
scene_points_library_path = _scene_points.path
get_scene_points_module = _scene_points.load


def _scene_points_args(points, direction, device_index):
    """(contiguous points, contiguous direction, n, device)"""
    _check_points(points)
    if points.device.index != device_index:
        raise ValueError(f"points are on {points.device} but the scene lives on cuda:{device_index}; move the points")
    if not isinstance(direction, torch.Tensor) or direction.device != points.device or direction.dtype != torch.float32 or direction.numel() != 3:
        raise ValueError("direction must be a float32 tensor of three elements on the points' device")
    return points.contiguous(), direction.reshape(3).contiguous(), points.shape[0], points.device


def scene_points_any_native(handle, device_index, points, direction, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_any: bool[n], is each of points float32 [n, 3] inside some instance, by the parity of the crossings of
    (p, direction) and (p, -direction) per instance.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same
    results).  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_scene_points_module()
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    out = _new_output((n,), torch.bool, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_points_any(handle, points.data_ptr(), n, direction.data_ptr(), out.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return out


def scene_points_count_native(handle, device_index, points, direction, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_count: int32[n], how many instances each point is inside.  Arguments as scene_points_any_native."""
    lib = get_scene_points_module()
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    out = _new_output((n,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_points_count(handle, points.data_ptr(), n, direction.data_ptr(), out.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return out


def scene_points_fill_native(handle, device_index, points, direction, count, offsets, total, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_fill: instance int32[total], the instances that hold point i ascending at rows offsets[i] ..
    offsets[i] + count[i].  count int32[n] is scene_points_count_native's and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same points and direction; total (a Python int) sizes the output.  Nothing is allocated by the
    library and nothing is synchronised."""
    lib = get_scene_points_module()
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    total = _check_fill(count, offsets, total, n, dev, "points")
    inst = _new_output((total,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_points_fill(handle, points.data_ptr(), n, direction.data_ptr(), count.data_ptr(), offsets.data_ptr(), total,
                                        _ptr_rows(inst), int(stack_entries), _stream_ptr(dev)))
    return inst


def scene_points_list_native(handle, device_index, points, direction, stack_entries=0):
    """(offsets int64[n + 1], instance int32[h]): one count launch, one scan, one host read of the total to size the output
    (as faces_in_boxes_native), one fill."""
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    count = scene_points_count_native(handle, device_index, points, direction, stack_entries)
    offsets, total = _scan_counts(count)
    return offsets, scene_points_fill_native(handle, device_index, points, direction, count, offsets[:n], total, stack_entries)


# --- the nearest placed triangle of a scene (include/triro_scene_nearest.h, csrc/scene_nearest.hip) ------------------------
SCENE_NEAREST_ABI_VERSION = 1    # TR_SCENE_NEAREST_ABI_VERSION of include/triro_scene_nearest.h

# every symbol include/triro_scene_nearest.h declares: (restype, argtypes)
SCENE_NEAREST_ABI = {
    "tr_scene_nearest_abi_version": (_int, []),
    "tr_scene_nearest_stack_capacity": (_int, []),
    "tr_scene_closest_point": (_int, [_vp, _vp, _i64, _vp, C.c_float, _vp, _vp, _vp, _vp, _int, _vp]),
}


_scene_nearest = _Satellite("scene_nearest", SCENE_NEAREST_ABI, get_scene_module)   # the scene handles are libtriro_scene.so's
scene_nearest_library_path = _scene_nearest.path
get_scene_nearest_module = _scene_nearest.load


def scene_closest_point_native(handle, device_index, points, max_distance=None, stack_entries=0, want_closest=True, want_distance=True):
    """tr_scene_closest_point: (closest float32[n, 3] or None, distance float32[n] or None, instance int32[n], tri int32[n])
    for float32 points [n, 3] on the scene's GPU: the nearest placed triangle, the instance it belongs to and its face index
    in the member mesh; (NaN, +Inf, -1, -1) where there is none.  max_distance: None (unbounded), a number, or a dense
    float32 [n] tensor on that GPU.  stack_entries: 0 = the whole far-child stack, 1 .. capacity for tests (same results).
    Nothing is allocated by the library and nothing is synchronised."""
    _check_points(points)
    if points.device.index != device_index:
        raise ValueError(f"points are on {points.device} but the scene lives on cuda:{device_index}; move the points")
    lib = get_scene_nearest_module()
    dev, n = points.device, points.shape[0]
    points = points.contiguous()
    rptr, r = None, float("inf")
    if isinstance(max_distance, torch.Tensor):
        if not max_distance.is_cuda or max_distance.device != dev or max_distance.dtype != torch.float32 or \
                tuple(max_distance.shape) != (n,) or not max_distance.is_contiguous():
            raise ValueError(f"max_distance must be a number or a contiguous float32 tensor of {n} elements on the points' device")
        rptr = max_distance.data_ptr()
    elif max_distance is not None:
        r = C.c_float(float(max_distance)).value      # rounded to float32 (beyond its range: +Inf, as a float32 tensor would hold it)
    closest = _new_output((n, 3), torch.float32, dev) if want_closest else None
    distance = _new_output((n,), torch.float32, dev) if want_distance else None
    inst = _new_output((n,), torch.int32, dev)
    tri = _new_output((n,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib.tr_scene_closest_point(handle, points.data_ptr(), n, rptr, r, _ptr(closest), _ptr(distance), inst.data_ptr(),
                                          tri.data_ptr(), int(stack_entries), _stream_ptr(dev)))
    return closest, distance, inst, tri
