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
    "tr_bvh_download_top": (_int, [_vp, _vp, _vp, _vp]),
    "tr_bvh_set_float_top": (_int, [_vp, _int]),
    "tr_bvh_poke_top": (_int, [_vp, C.c_int64, _vp, _vp]),
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


def _bind(path, abi):
    """the library at `path` with every symbol of the table {symbol: (restype, argtypes)} declared"""
    lib = C.CDLL(path)
    for name, (res, args) in abi.items():
        fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


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
    lib = _bind(path, ABI)
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


# --- marshaling: the one path of every query --------------------------------------------------
def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _call(fn, device, *args):
    """Every native call that enqueues work: made on `device`, with torch's current stream of that device as the last
    argument (each entry of the C ABI takes its stream last), and checked."""
    if torch.cuda.current_device() == device.index:      # (the usual case; entering a device context costs microseconds)
        _check(fn(*args, _stream_ptr(device)))
    else:
        with torch.cuda.device(device):
            _check(fn(*args, _stream_ptr(device)))


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


def _call_rays(fn, handle, origins, dirs, *args):
    """_call for an entry that takes (handle, rays, ...): on the rays' device"""
    _call(fn, origins.device, handle, C.byref(make_rays(origins, dirs)), *args)


def _new_output(shape, dtype, device) -> torch.Tensor:
    """Every tensor the library writes into -- results and the intermediates count / slots / offsets / total_d -- is born
    here, uninitialised.  One seam, so that a run can swap it to see which bytes no kernel ever wrote (tests/poison.py)."""
    return torch.empty(shape, dtype=dtype, device=device)


# the columns of the outputs: (dtype, trailing shape)
_BOOL, _I32, _I64, _F32 = (torch.bool, ()), (torch.int32, ()), (torch.int64, ()), (torch.float32, ())
_F32X3, _F32X2 = (torch.float32, (3,)), (torch.float32, (2,))


def _outputs(lead, device, *columns):
    """one new output per column, of shape (*lead, *trailing shape); None for a column that is not wanted (given as False)"""
    return tuple(_new_output((*lead, *c[1]), c[0], device) if c else None for c in columns)


def _ptr(t):
    """the device pointer of an optional tensor: None if absent"""
    return t.data_ptr() if t is not None else None


def _ptr_rows(t):
    """the device pointer of an optional output of a fill: None if absent or empty (the fills take NULL for zero rows)"""
    return t.data_ptr() if t is not None and t.numel() else None


_DENSE = (_BOOL, _BOOL, _I32, _F32X3, _F32X2)


def _dense_outputs(n, batch, device, outs=None, whose="the rays' device", want_dense=True, want_t=False):
    """(hit, front, tri, loc, uv, t) of a closest-hit query of n rays: new, of the batch shape, or the caller's `outs`, which
    must be the five contiguous flat destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2]) on the
    query's device.  want_dense=False: hit, front, loc and uv are None; t float32 is new only with want_t."""
    if outs is not None:
        if len(outs) != 5 or any(t.dtype != dt or tuple(t.shape) != (n, *tail) or not t.is_contiguous() or t.device != device
                                 for t, (dt, tail) in zip(outs, _DENSE)):
            raise ValueError(f"outs must be contiguous (bool[n], bool[n], int32[n], float32[n,3], float32[n,2]) on {whose}")
        return (*outs, None)
    if batch is None:
        batch = (n,)
    hit, front, tri, loc, uv = _DENSE if want_dense else (False, False, _I32, False, False)      # (the triangle index: always)
    dense = _outputs(batch, device, hit, front, tri, loc, uv, want_t and _F32)
    if dense[2].numel() != n:
        raise ValueError(f"batch_shape {tuple(batch)} does not hold {n} rays")
    return dense


def _ray_query(symbol, accel_structure, origins, dirs, column):
    """a query of libtriro_hip.so with one output per ray"""
    check_rays(origins, dirs)
    out, = _outputs(origins.shape[:-1], origins.device, column)
    _call_rays(getattr(get_module(), symbol), _handle(accel_structure, origins), origins, dirs, out.data_ptr())
    return out


# --- queries (ops.py:84-192) ----------------------------------------------------------------------
def intersects_any(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:84-100 / ray.cpp:161-189.  Bool[*b]."""
    return _ray_query("tr_intersects_any", accel_structure, origins, dirs, _BOOL)


def intersects_first(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:103-119 / ray.cpp:191-219.  Int32[*b], -1 on miss."""
    return _ray_query("tr_intersects_first", accel_structure, origins, dirs, _I32)


def intersects_closest(accel_structure, origins, dirs, outs=None) -> Tuple[torch.Tensor, ...]:
    """ops.py:122-149 / ray.cpp:231-289.  (hit, front, tri_idx, loc, uv).  `outs`: optional preallocated
    contiguous destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2] with n = the
    number of rays -- e.g. this rank's rows of gathered full-size outputs, triro.ray.sharded)."""
    check_rays(origins, dirs)
    dense = _dense_outputs(origins.numel() // 3, origins.shape[:-1], origins.device, outs)[:5]
    _call_rays(get_module().tr_intersects_closest, _handle(accel_structure, origins), origins, dirs, *(t.data_ptr() for t in dense))
    return dense


def _flat_output(out, name, shape, device):
    """the caller's `out` (`slots`), checked, or a new one: contiguous int32 of shape (n,) or (n, 3) on the rays' device"""
    if out is None:
        return _new_output(shape, torch.int32, device)
    if out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{name} must be a contiguous int32 {'[n]' if len(shape) == 1 else '[n, 3]'} tensor on the rays' device, one row per ray")
    return out


def intersects_closest_packed(accel_structure, origins, dirs, out: torch.Tensor = None, slots: bool = False) -> torch.Tensor:
    """Closest hit as 12 bytes per ray: int32 [n, 3] rows {face | front << 30 (-1 on a miss), u bits,
    v bits} (tr_packed_hit).  What a ray-sharded run sends over xGMI instead of the 26 B/ray of the five
    dense outputs; `closest_expand` rebuilds those bit for bit.  `out`: optional preallocated [n, 3]
    int32 destination (a slice of a gather buffer)."""
    check_rays(origins, dirs)
    out = _flat_output(out, "out", (origins.numel() // 3, 3), origins.device)
    # slots: the record names the ARENA SLOT of the triangle instead of its face index (tr_intersects_closest_packed_slots):
    # cheaper to expand (closest_expand_slots), valid only for this hierarchy or a bit-identical replica of it
    fn = get_module().tr_intersects_closest_packed_slots if slots else get_module().tr_intersects_closest_packed
    _call_rays(fn, _handle(accel_structure, origins), origins, dirs, out.data_ptr())
    return out


def intersects_closest_slots(accel_structure, origins, dirs, out: torch.Tensor = None) -> torch.Tensor:
    """tr_intersects_closest_slots: closest hit as 4 bytes per ray -- int32 [n]: the arena slot of the nearest
    triangle, -1 for a miss.  For a destination that holds the rays (closest_from_slots finishes the query there);
    valid for this hierarchy or a bit-identical replica.  `out`: optional preallocated int32 [n] destination."""
    check_rays(origins, dirs)
    out = _flat_output(out, "out", (origins.numel() // 3,), origins.device)
    _call_rays(get_module().tr_intersects_closest_slots, _handle(accel_structure, origins), origins, dirs, out.data_ptr())
    return out


def closest_from_slots(accel_structure, origins, dirs, slots: torch.Tensor, outs=None, row_length: int = 0):
    """tr_closest_from_slots: (rays, their slots from intersects_closest_slots on any bit-identical replica) ->
    (hit, front, tri_idx, loc, uv), the bits of intersects_closest on the same rays.  `outs`: optional preallocated
    contiguous destinations (bool [n], bool [n], int32 [n], float32 [n, 3], float32 [n, 2]); otherwise the outputs
    take the rays' batch shape.  row_length: the rays are whole rows of an image of that width."""
    check_rays(origins, dirs)
    n, dev = origins.numel() // 3, origins.device
    _flat_output(slots, "slots", (n,), dev)
    dense = _dense_outputs(n, origins.shape[:-1], dev, outs)[:5]
    _call_rays(get_module().tr_closest_from_slots, _handle(accel_structure, origins), origins, dirs, slots.data_ptr(), int(row_length),
               *(t.data_ptr() for t in dense))
    return dense


def closest_expand_slots(accel_structure, packed: torch.Tensor, batch_shape=None, outs=None, row_length: int = 0):
    """tr_closest_expand_slots: slot-form records (intersects_closest_packed(..., slots=True), of this hierarchy or of a
    bit-identical replica) -> (hit, front, tri_idx, loc, uv), bit-identical to intersects_closest on the same rays."""
    if packed.dtype != torch.int32 or packed.dim() != 2 or packed.shape[1] != 3 or not packed.is_contiguous() or not packed.is_cuda:
        raise ValueError("packed must be a contiguous int32 [n, 3] tensor on the GPU")
    dev, n = packed.device, packed.shape[0]
    dense = _dense_outputs(n, batch_shape, dev, outs, "the device of packed")[:5]
    # row_length: the records are whole rows of an image of that width (tr_closest_expand_slots_rows: 8x8 tiles per wave)
    _call(get_module().tr_closest_expand_slots_rows, dev, _handle(accel_structure, packed), packed.data_ptr(), n, int(row_length),
          *(t.data_ptr() for t in dense))
    return dense


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
    dev, n = packed.device, packed.shape[0]
    if not packed.is_cuda or vertices.device != dev or faces.device != dev:
        raise ValueError("packed, vertices and faces must live on the same GPU")
    dense = _dense_outputs(n, batch_shape, dev, outs, "the device of packed")[:5]
    _call(get_module().tr_closest_expand, dev, packed.data_ptr(), n, vertices.data_ptr(), vertices.shape[0], faces.data_ptr(), faces.shape[0],
          *(t.data_ptr() for t in dense))
    return dense


def intersects_count(accel_structure, origins, dirs) -> torch.Tensor:
    """ops.py:152-168 / ray.cpp:291-322.  Int32[*b]."""
    return _ray_query("tr_intersects_count", accel_structure, origins, dirs, _I32)


def _scan_counts(count, cap=0x7fffffff):
    """(offsets int64[n + 1], total) of a flat int32[n] count, each clamped to `cap`: the exclusive scan that a fill takes
    as offsets[:n], and one host read of the total to size its outputs (ray.cpp:339 .item<int>()).  The grand total lands
    in offsets[n] on the device and, after the stream is synchronised, on the host."""
    n, dev = count.shape[0], count.device
    offsets = _new_output((n + 1,), torch.int64, dev)
    total = C.c_int64(0)
    start = offsets.data_ptr()
    _call(get_module().tr_hits_scan, dev, count.data_ptr(), n, cap, start, start + 8 * n, C.byref(total))
    return offsets, int(total.value)


def intersects_location(accel_structure, origins, dirs, ray_base: int = 0, fused: bool = True) -> Tuple[torch.Tensor, ...]:
    """ops.py:171-192 / ray.cpp:324-378.  (loc[h,3], ray_idx[h], tri_idx[h]); at most
    MAX_ANYHIT_SIZE hits per ray, grouped by ray; within a ray ordered by distance (the
    reference leaves that order unspecified).

    fused=True (default): one traversal (count + slots of the 8 nearest hits), scan, fill from
    the slots.  fused=False: the reference's protocol, count pass -> scan -> second traversal
    (ray.cpp:330, 333-342, 372-374); both give identical results."""
    check_rays(origins, dirs)
    dev, n, lib = origins.device, origins.numel() // 3, get_module()
    _check_ray_idx_range(n, ray_base, "intersects_location / intersects_id")
    handle, rays = _handle(accel_structure, origins), C.byref(make_rays(origins, dirs))
    count = _new_output((n,), torch.int32, dev)
    if fused:
        slots = _new_output((n, MAX_ANYHIT_SIZE, 2), torch.int32, dev)   # tr_hit_entry {t_key, slot}
        _call(lib.tr_intersects_count_topk, dev, handle, rays, MAX_ANYHIT_SIZE, count.data_ptr(), slots.data_ptr())
    else:
        _call(lib.tr_intersects_count, dev, handle, rays, count.data_ptr())
    offsets, nhits = _scan_counts(count, MAX_ANYHIT_SIZE)
    loc, tri, ray = _outputs((nhits,), dev, _F32X3, _I32, _I32)
    if fused:
        _call(lib.tr_location_fill_slots, dev, handle, rays, MAX_ANYHIT_SIZE, count.data_ptr(), offsets.data_ptr(), slots.data_ptr(),
              loc.data_ptr(), ray.data_ptr(), tri.data_ptr(), ray_base)
    else:
        _call(lib.tr_intersects_location_fill, dev, handle, rays, MAX_ANYHIT_SIZE, offsets.data_ptr(), loc.data_ptr(), ray.data_ptr(),
              tri.data_ptr(), ray_base)
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
    dev, n, lib = hit.device, hit.numel(), get_module()
    _check_ray_idx_range(n, ray_base, "stream compaction")
    offsets, total_d = _outputs((), dev, (torch.int64, (n,)), (torch.int64, (1,)))
    total = C.c_int64(0)
    _call(lib.tr_mask_scan, dev, hit.data_ptr(), n, offsets.data_ptr(), total_d.data_ptr(), C.byref(total))
    outs = _outputs((int(total.value),), dev, front is not None and _BOOL, _I32, tri is not None and _I32, loc is not None and _F32X3,
                    uv is not None and _F32X2)
    _call(lib.tr_compact_closest, dev, hit.data_ptr(), offsets.data_ptr(), n, _ptr(front), _ptr(tri), _ptr(loc), _ptr(uv), ray_base,
          *(_ptr(t) for t in outs))
    return outs


QUERY_IDS = {"any": 0, "first": 1, "closest": 2, "count": 3, "location": 4}


def _trace_stats(accel_structure, origins, dirs, query=None) -> dict:
    """the counters of tr_trace_stats_closest (query None) or of tr_trace_stats_query for the query of that name"""
    check_rays(origins, dirs)
    st = TrTraceStats()
    handle, lib = _handle(accel_structure, origins), get_module()
    if query is None:
        _call_rays(lib.tr_trace_stats_closest, handle, origins, dirs, C.byref(st))
    else:
        _call_rays(lib.tr_trace_stats_query, handle, origins, dirs, QUERY_IDS[query], C.byref(st))
    return dict(rays=st.rays, node_visits=st.node_visits, tri_tests=st.tri_tests, climb_steps=st.climb_steps)


def trace_stats_closest(accel_structure, origins, dirs) -> dict:
    """Diagnostic: per-launch traversal counters of the instrumented closest-hit kernel."""
    return _trace_stats(accel_structure, origins, dirs)


def trace_stats(accel_structure, origins, dirs, query: str = "closest") -> dict:
    """Diagnostic: traversal counters of the instrumented kernel of any query."""
    return _trace_stats(accel_structure, origins, dirs, query)


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
            lib = _bind(path, self.abi)
            want = globals()[f"{self.key.upper()}_ABI_VERSION"]
            if want is not None:
                have = getattr(lib, f"tr_{self.key}_abi_version")()
                if have != want:
                    raise RuntimeError(f"libtriro_{self.key}.so ABI version {have} != {want} expected by this binding")
            self.lib = lib
        return self.lib


def _points_args(points):
    """(contiguous points, n, device) of float32 points [n, 3] on a GPU"""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or \
            points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a float32 GPU tensor of shape [n, 3]")
    return points.contiguous(), points.shape[0], points.device


def _pair_args(accel_structure, name_a, a, name_b, b):
    """(handle, contiguous a, contiguous b, n, device) of two float32 GPU tensors [n, 3] of one shape on one device (the
    corners of boxes, the origins and normals of planes)"""
    for name, t in ((name_a, a), (name_b, b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be a float32 GPU tensor of shape [n, 3]")
    if b.device != a.device or b.shape != a.shape:
        raise ValueError(f"{name_a} {tuple(a.shape)} on {a.device} and {name_b} {tuple(b.shape)} on {b.device} "
                         f"must have one shape and one device")
    return _handle(accel_structure, a), a.contiguous(), b.contiguous(), a.shape[0], a.device


def _dense_f32(t, name, n, device, otherwise, whose):
    """a per-query float32 argument given as a tensor: dense [n] on the queries' device"""
    if not t.is_cuda or t.device != device or t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f"{name} must be {otherwise} or a contiguous float32 tensor of {n} elements on the {whose}' device")
    return t


def _range_bound(t, name, n, device):
    """a bound of the range queries: None (the default) or a dense float32 [n] tensor on the rays' device"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be None or a contiguous float32 tensor of {n} elements on the rays' device")
    return _dense_f32(t, name, n, device, "None", "rays")


def _radius(radius, name, n, device, unused=0.0):
    """(pointer or None, scalar) of a radius as the entries take it: a dense float32 [n] tensor on the points' device (the
    scalar is then `unused`), or a number, rounded to float32 (beyond its range: +Inf, as a float32 tensor would hold it)"""
    if isinstance(radius, torch.Tensor):
        return _dense_f32(radius, name, n, device, "a number", "points").data_ptr(), unused
    return None, C.c_float(float(radius)).value


def _on_scene_device(t, what, device_index):
    if t.device.index != device_index:
        raise ValueError(f"{what} are on {t.device} but the scene lives on cuda:{device_index}; move the {what}")


def _any_or_count(query, satellite):
    """(the column of the output, the entry point) of the any / count pair of a library: bool and tr_<key>_any, or int32 and
    tr_<key>_count"""
    if query not in ("any", "count"):
        raise ValueError(f"query must be 'any' or 'count', got {query!r}")
    return (_BOOL if query == "any" else _I32), getattr(satellite.load(), f"tr_{satellite.key}_{query}")


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


def _count_scan_fill(count_native, fill_native, queries, count_args, fill_args):
    """The list form of a family: (offsets int64[n + 1], *the outputs of its fill) -- one count launch, one scan, one host
    read of the total to size the outputs (as intersects_location), one fill.  `queries`: the arguments both entries take
    first, as the caller gave them; each entry checks them once."""
    count = count_native(*queries, *count_args).reshape(-1)
    offsets, total = _scan_counts(count)
    filled = fill_native(*queries, count, offsets[:-1], total, *fill_args)
    return (offsets, *filled) if isinstance(filled, tuple) else (offsets, filled)


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
    points, n, dev = _points_args(points)
    handle = _handle(accel_structure, points)
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
    inside, broken = _outputs((n,), dev, _BOOL, _BOOL)
    counts, = _outputs((2, n), dev, want_counts and _I32)
    summary, = _outputs((2,), dev, _I64)
    _call(get_points_module().tr_contains_points, dev, handle, points.data_ptr(), n, direction.data_ptr(), _ptr(box_lo), _ptr(box_hi),
          inside.data_ptr(), broken.data_ptr(), _ptr(counts), summary.data_ptr(), None)
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
    points, n, dev = _points_args(points)
    lib = get_nearest_module()
    handle = _handle(accel_structure, points)
    closest, distance, tri = _outputs((n,), dev, want_closest and _F32X3, want_distance and _F32, _I32)
    _call(lib.tr_closest_point, dev, handle, points.data_ptr(), n, _ptr(closest), _ptr(distance), tri.data_ptr(), int(stack_entries))
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


def _range_query(fn, handle, origins, dirs, tmin, tmax, column, stack_entries):
    """an entry (handle, rays, tmin, tmax, out, stack_entries) with one output per ray, for checked rays: on a mesh or on a
    scene, any or a count of crossings"""
    dev, n = origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    out, = _outputs(origins.shape[:-1], dev, column)
    _call_rays(fn, handle, origins, dirs, _ptr(tmin), _ptr(tmax), out.data_ptr(), int(stack_entries))
    return out


def _range_closest(fn, handle, with_instance, origins, dirs, tmin, tmax, stack_entries, want_t, want_dense):
    """an entry (handle, rays, tmin, tmax, [instance,] tri, t, hit, front, loc, uv, stack_entries) for checked rays ->
    (hit, front, instance or None, tri, loc, uv, t)"""
    b, dev, n = origins.shape[:-1], origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    inst, = _outputs(b, dev, with_instance and _I32)
    hit, front, tri, loc, uv, t = _dense_outputs(n, b, dev, want_dense=want_dense, want_t=want_t)
    _call_rays(fn, handle, origins, dirs, _ptr(tmin), _ptr(tmax), *((inst.data_ptr(),) if with_instance else ()), tri.data_ptr(), _ptr(t),
               _ptr(hit), _ptr(front), _ptr(loc), _ptr(uv), int(stack_entries))
    return hit, front, inst, tri, loc, uv, t


def range_any_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_range_any: bool[*b], is anything hit within [tmin, tmax] (closed, measured from the origin given, no anchoring).
    Rays as for intersects_any (any strides); tmin / tmax: None or dense float32 [n], n = the number of rays.
    stack_entries: 0 = the whole far-child stack, 1 .. capacity for tests (same results).  Nothing is allocated by the
    library and nothing is synchronised."""
    check_rays(origins, dirs)
    return _range_query(get_range_module().tr_range_any, _handle(accel_structure, origins), origins, dirs, tmin, tmax, _BOOL, stack_entries)


def range_closest_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0, want_t=True, want_dense=True):
    """tr_range_closest: (hit bool[*b], front bool[*b], tri int32[*b], loc float32[*b, 3], uv float32[*b, 2], t float32[*b])
    of the first hit within [tmin, tmax]; a miss is (False, False, -1, 0, 0, +Inf).  want_t=False: t is None;
    want_dense=False: hit, front, loc and uv are None (tri, and t, alone).  Arguments as range_any_native."""
    check_rays(origins, dirs)
    hit, front, _, tri, loc, uv, t = _range_closest(get_range_module().tr_range_closest, _handle(accel_structure, origins), False, origins, dirs,
                                                    tmin, tmax, stack_entries, want_t, want_dense)
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
    _call(get_scene_module().tr_scene_commit, torch.device("cuda", device_index), handle, members, len(member_handles), mesh_of.ctypes.data,
          M.ctypes.data, len(mesh_of))


def scene_info(handle) -> dict:
    inf = TrSceneInfo()
    _check(get_scene_module().tr_scene_info(handle, C.byref(inf)))
    return {k: int(getattr(inf, k)) for k, _ in inf._fields_}


def _scene_rays(origins, dirs, device_index):
    check_rays(origins, dirs)
    _on_scene_device(origins, "rays", device_index)


def scene_any_native(handle, device_index, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_scene_any: bool[*b], does any instance have a hit within [tmin, tmax] of the world ray.  Arguments as
    range_any_native, with the scene handle and its device in place of the acceleration structure.  Nothing is allocated
    by the library and nothing is synchronised."""
    _scene_rays(origins, dirs, device_index)
    return _range_query(get_scene_module().tr_scene_any, handle, origins, dirs, tmin, tmax, _BOOL, stack_entries)


def scene_closest_native(handle, device_index, origins, dirs, tmin=None, tmax=None, stack_entries=0, want_t=True, want_dense=True):
    """tr_scene_closest: (hit bool[*b], front bool[*b], instance int32[*b], tri int32[*b], t float32[*b], loc float32[*b, 3],
    uv float32[*b, 2]) of the first hit within [tmin, tmax] over all instances; a miss is (False, False, -1, -1, +Inf, 0, 0).
    want_t=False: t is None; want_dense=False: hit, front, loc and uv are None (instance, tri and t alone)."""
    _scene_rays(origins, dirs, device_index)
    hit, front, inst, tri, loc, uv, t = _range_closest(get_scene_module().tr_scene_closest, handle, True, origins, dirs, tmin, tmax,
                                                       stack_entries, want_t, want_dense)
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
    """(handle, contiguous points, n, device, radius pointer or None, scalar radius)"""
    points, n, dev = _points_args(points)
    return (_handle(accel_structure, points), points, n, dev, *_radius(radius, "radius", n, dev))


def within_native(accel_structure, points, radius, query="any", stack_entries=0) -> torch.Tensor:
    """tr_within_any (query="any": bool[n]) / tr_within_count (query="count": int32[n]) for float32 points [n, 3] on the
    handle's GPU.  radius: a number, or a dense float32 [n] tensor on that GPU.  stack_entries: 0 = the whole stack,
    1 .. capacity for tests (same results).  Nothing is allocated by the library and nothing is synchronised."""
    column, fn = _any_or_count(query, _within)
    handle, points, n, dev, rptr, r = _within_args(accel_structure, points, radius)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, points.data_ptr(), n, rptr, r, out.data_ptr(), int(stack_entries))
    return out


def within_fill_native(accel_structure, points, radius, count, offsets, total, want_distance=False, want_closest=False,
                       stack_entries=0):
    """tr_within_fill: (face int32[total], distance float32[total] or None, closest float32[total, 3] or None), the faces of
    point i ascending at rows offsets[i] .. offsets[i] + count[i].  count int32[n] is within_native(..., "count") and
    offsets int64[n] its exclusive scan (tr_hits_scan) for the same points and radii; total (a Python int) sizes the
    outputs.  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_within_module()
    handle, points, n, dev, rptr, r = _within_args(accel_structure, points, radius)
    total = _check_fill(count, offsets, total, n, dev, "points")
    face, distance, closest, slot = _outputs((total,), dev, _I32, want_distance and _F32, want_closest and _F32X3,
                                             (want_distance or want_closest) and total > 0 and _I32)
    _call(lib.tr_within_fill, dev, handle, points.data_ptr(), n, rptr, r, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(face),
          _ptr_rows(distance), _ptr_rows(closest), _ptr_rows(slot), int(stack_entries))
    return face, distance, closest


def faces_within_native(accel_structure, points, radius, want_distance=False, want_closest=False, stack_entries=0):
    """(offsets int64[n + 1], face, distance or None, closest or None): one count launch, one scan, one host read of the
    total to size the outputs (as intersects_location), one fill."""
    return _count_scan_fill(within_native, within_fill_native, (accel_structure, points, radius), ("count", stack_entries),
                            (want_distance, want_closest, stack_entries))


def within_closest_native(accel_structure, points, radius, stack_entries=0, want_closest=True, want_distance=True):
    """tr_within_closest: closest_point_native bounded by the radius -- (closest float32[n, 3] or None, distance float32[n]
    or None, tri int32[n]), (NaN, +Inf, -1) where no face is within.  radius as for within_native."""
    lib = get_within_module()
    handle, points, n, dev, rptr, r = _within_args(accel_structure, points, radius)
    closest, distance, tri = _outputs((n,), dev, want_closest and _F32X3, want_distance and _F32, _I32)
    _call(lib.tr_within_closest, dev, handle, points.data_ptr(), n, rptr, r, _ptr(closest), _ptr(distance), tri.data_ptr(), int(stack_entries))
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


def boxes_native(accel_structure, lo, hi, query="any", stack_entries=0) -> torch.Tensor:
    """tr_boxes_any (query="any": bool[n]) / tr_boxes_count (query="count": int32[n]) for the closed boxes [lo, hi], float32
    [n, 3] each, on the handle's GPU.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing
    is allocated by the library and nothing is synchronised."""
    column, fn = _any_or_count(query, _boxes)
    handle, lo, hi, n, dev = _pair_args(accel_structure, "lo", lo, "hi", hi)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, lo.data_ptr(), hi.data_ptr(), n, out.data_ptr(), int(stack_entries))
    return out


def boxes_fill_native(accel_structure, lo, hi, count, offsets, total, want_inside=False, stack_entries=0):
    """tr_boxes_fill: (face int32[total], inside bool[total] or None), the faces of box i ascending at rows offsets[i] ..
    offsets[i] + count[i].  count int32[n] is boxes_native(..., "count") and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same boxes; total (a Python int) sizes the outputs.  Nothing is allocated by the library and
    nothing is synchronised."""
    lib = get_boxes_module()
    handle, lo, hi, n, dev = _pair_args(accel_structure, "lo", lo, "hi", hi)
    total = _check_fill(count, offsets, total, n, dev, "boxes")
    face, inside = _outputs((total,), dev, _I32, want_inside and _BOOL)
    _call(lib.tr_boxes_fill, dev, handle, lo.data_ptr(), hi.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(face),
          _ptr_rows(inside), int(stack_entries))
    return face, inside


def faces_in_boxes_native(accel_structure, lo, hi, want_inside=False, stack_entries=0):
    """(offsets int64[n + 1], face, inside or None): one count launch, one scan, one host read of the total to size the
    outputs (as faces_within_native), one fill."""
    return _count_scan_fill(boxes_native, boxes_fill_native, (accel_structure, lo, hi), ("count", stack_entries), (want_inside, stack_entries))


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
    """(handle, contiguous triangles, n, device); accel_structure None (the queries of a scene, whose handle the caller holds):
    the handle is None"""
    if not isinstance(tri, torch.Tensor) or not tri.is_cuda or tri.dtype != torch.float32 or tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3):
        raise ValueError("triangles must be a float32 GPU tensor of shape [n, 3, 3]")
    return None if accel_structure is None else _handle(accel_structure, tri), tri.contiguous(), tri.shape[0], tri.device


def tris_native(accel_structure, tri, query="any", stack_entries=0) -> torch.Tensor:
    """tr_tris_any (query="any": bool[n]) / tr_tris_count (query="count": int32[n]) for the query triangles, float32 [n, 3, 3],
    on the handle's GPU.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing is allocated
    by the library and nothing is synchronised."""
    column, fn = _any_or_count(query, _tris)
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, tri.data_ptr(), n, out.data_ptr(), int(stack_entries))
    return out


def tris_fill_native(accel_structure, tri, count, offsets, total, stack_entries=0) -> torch.Tensor:
    """tr_tris_fill: face int32[total], the faces of query i ascending at rows offsets[i] .. offsets[i] + count[i].  count
    int32[n] is tris_native(..., "count") and offsets int64[n] its exclusive scan (tr_hits_scan) for the same queries; total (a
    Python int) sizes the output.  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_tris_module()
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    total = _check_fill(count, offsets, total, n, dev, "triangles")
    face, = _outputs((total,), dev, _I32)
    _call(lib.tr_tris_fill, dev, handle, tri.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(face), int(stack_entries))
    return face


def faces_meeting_triangles_native(accel_structure, tri, stack_entries=0):
    """(offsets int64[n + 1], face int32[h]): one count launch, one scan, one host read of the total to size the output (as
    faces_in_boxes_native), one fill."""
    return _count_scan_fill(tris_native, tris_fill_native, (accel_structure, tri), ("count", stack_entries), (stack_entries,))


# --- the nearest face to each query triangle (include/triro_tri_nearest.h, csrc/tri_nearest.hip) -------------------------
TRI_NEAREST_ABI_VERSION = 1    # TR_TRI_NEAREST_ABI_VERSION of include/triro_tri_nearest.h

# every symbol include/triro_tri_nearest.h declares: (restype, argtypes)
TRI_NEAREST_ABI = {
    "tr_tri_nearest_abi_version": (_int, []),
    "tr_tri_nearest_stack_capacity": (_int, []),
    "tr_triangles_nearest": (_int, [_vp, _vp, _i64, _vp, _f32, _vp, _vp, _vp, _vp, _int, _vp]),
}


_tri_nearest = _Satellite("tri_nearest", TRI_NEAREST_ABI, get_module)
tri_nearest_library_path = _tri_nearest.path
get_tri_nearest_module = _tri_nearest.load


def triangles_nearest_native(accel_structure, tri, max_distance=None, stack_entries=0, want=(True, True, True)):
    """tr_triangles_nearest: (tri int32[n], distance float32[n] or None, closest_mesh float32[n, 3] or None, closest_query
    float32[n, 3] or None) for the query triangles, float32 [n, 3, 3], on the handle's GPU: the nearest face, its distance and
    the two nearest points; (-1, +Inf, NaN, NaN) where there is none.  max_distance: None (unbounded), a number, or a dense
    float32 [n] tensor on that GPU.  want: which of the three optional outputs to produce.  stack_entries: 0 = the whole
    far-child stack, 1 .. capacity for tests (same results).  Nothing is allocated by the library and nothing is synchronised."""
    lib = get_tri_nearest_module()
    handle, tri, n, dev = _tris_args(accel_structure, tri)
    rptr, r = (None, float("inf")) if max_distance is None else _radius(max_distance, "max_distance", n, dev, float("inf"))
    want_distance, want_mesh, want_query = want
    face, distance, on_mesh, on_query = _outputs((n,), dev, _I32, want_distance and _F32, want_mesh and _F32X3, want_query and _F32X3)
    _call(lib.tr_triangles_nearest, dev, handle, tri.data_ptr(), n, rptr, r, face.data_ptr(), _ptr(distance), _ptr(on_mesh), _ptr(on_query),
          int(stack_entries))
    return face, distance, on_mesh, on_query


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


def planes_native(accel_structure, origins, normals, query="any", cut=False, frontier_entries=0) -> torch.Tensor:
    """tr_planes_any (query="any": bool[n]) / tr_planes_count (query="count": int32[n]) for the planes (origin, normal), float32
    [n, 3] each, on the handle's GPU.  cut: the faces the plane CUTS (those that own a row of the section) instead of the faces
    it meets.  frontier_entries: 0 = the whole frontier, 1 .. capacity for tests (same results).  Nothing is allocated by the
    library and nothing is synchronised."""
    column, fn = _any_or_count(query, _planes)
    handle, origins, normals, n, dev = _pair_args(accel_structure, "origins", origins, "normals", normals)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, origins.data_ptr(), normals.data_ptr(), n, out.data_ptr(), 1 if cut else 0, int(frontier_entries))
    return out


def planes_fill_native(accel_structure, origins, normals, count, offsets, total, cut=False, want_segments=False, frontier_entries=0):
    """tr_planes_fill: (face int32[total], segments float32[total, 2, 3] or None), the faces of plane i ascending at rows
    offsets[i] .. offsets[i] + count[i].  count int32[n] is planes_native(..., "count", cut) and offsets int64[n] its exclusive
    scan (tr_hits_scan) for the same planes; total (a Python int) sizes the outputs.  Segments need cut.  Nothing is allocated
    by the library and nothing is synchronised."""
    lib = get_planes_module()
    handle, origins, normals, n, dev = _pair_args(accel_structure, "origins", origins, "normals", normals)
    total = _check_fill(count, offsets, total, n, dev, "planes")
    if want_segments and not cut:
        raise ValueError("segments are those of the cut faces: want_segments needs cut=True")
    face, segments = _outputs((total,), dev, _I32, want_segments and (torch.float32, (2, 3)))
    _call(lib.tr_planes_fill, dev, handle, origins.data_ptr(), normals.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total,
          _ptr_rows(face), _ptr_rows(segments), 1 if cut else 0, int(frontier_entries))
    return face, segments


def faces_on_planes_native(accel_structure, origins, normals, cut=False, want_segments=False, frontier_entries=0):
    """(offsets int64[n + 1], face, segments or None): one count launch, one scan, one host read of the total to size the
    outputs (as faces_in_boxes_native), one fill."""
    return _count_scan_fill(planes_native, planes_fill_native, (accel_structure, origins, normals), ("count", cut, frontier_entries),
                            (cut, want_segments, frontier_entries))


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


def _cross_fill(fn, handle, with_instance, origins, dirs, tmin, tmax, count, offsets, total, want_front, want_loc, want_uv, want_ray,
                ray_base, stack_entries):
    """an entry (handle, rays, tmin, tmax, count, offsets, total, [instance,] face, t, front, loc, uv, ray, ray_base, slot,
    stack_entries) for checked rays -> ([instance,] face, t, front or None, loc or None, uv or None, ray or None)"""
    dev, n = origins.device, origins.numel() // 3
    tmin, tmax = _range_bound(tmin, "tmin", n, dev), _range_bound(tmax, "tmax", n, dev)
    total = _check_fill(count, offsets, total, n, dev, "rays")
    rows = _outputs((total,), dev, with_instance and _I32, _I32, _F32, want_front and _BOOL, want_loc and _F32X3, want_uv and _F32X2,
                    want_ray and _I64, (want_front or want_loc or want_uv) and total > 0 and _I32)
    rows, slot = rows[0 if with_instance else 1:-1], rows[-1]
    _call_rays(fn, handle, origins, dirs, _ptr_rows(tmin), _ptr_rows(tmax), count.data_ptr(), offsets.data_ptr(), total,
               *(_ptr_rows(t) for t in rows), int(ray_base), _ptr_rows(slot), int(stack_entries))
    return rows


def cross_count_native(accel_structure, origins, dirs, tmin=None, tmax=None, stack_entries=0) -> torch.Tensor:
    """tr_cross_count: int32[*b], how many triangles each ray crosses within [tmin, tmax] (closed, measured from the origin
    given, no anchoring), uncapped.  Rays as for intersects_any (any strides); tmin / tmax: None or dense float32 [n], n =
    the number of rays.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same results).  Nothing is allocated by
    the library and nothing is synchronised."""
    check_rays(origins, dirs)
    return _range_query(get_cross_module().tr_cross_count, _handle(accel_structure, origins), origins, dirs, tmin, tmax, _I32, stack_entries)


def cross_fill_native(accel_structure, origins, dirs, tmin, tmax, count, offsets, total, want_front=False, want_loc=False,
                      want_uv=False, want_ray=False, ray_base: int = 0, stack_entries=0):
    """tr_cross_fill: (face int32[total], t float32[total], front bool[total] or None, loc float32[total, 3] or None,
    uv float32[total, 2] or None, ray int64[total] or None): the crossings of ray i by (t, face) ascending at rows offsets[i]
    .. offsets[i] + count[i].  count int32[n] is cross_count_native's (flattened) and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same rays and bounds; total (a Python int) sizes the outputs.  Nothing is allocated by the library
    and nothing is synchronised."""
    check_rays(origins, dirs)
    return _cross_fill(get_cross_module().tr_cross_fill, _handle(accel_structure, origins), False, origins, dirs, tmin, tmax, count, offsets,
                       total, want_front, want_loc, want_uv, want_ray, ray_base, stack_entries)


def cross_all_native(accel_structure, origins, dirs, tmin=None, tmax=None, want_front=False, want_loc=False, want_uv=False,
                     want_ray=False, ray_base: int = 0, stack_entries=0):
    """(offsets int64[n + 1], face, t, front or None, loc or None, uv or None, ray or None) for the rays flattened in order:
    one count launch, one scan, one host read of the total to size the outputs (as faces_within_native), one fill."""
    return _count_scan_fill(cross_count_native, cross_fill_native, (accel_structure, origins, dirs, tmin, tmax), (stack_entries,),
                            (want_front, want_loc, want_uv, want_ray, ray_base, stack_entries))


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
    return _range_query(get_scene_cross_module().tr_scene_cross_count, handle, origins, dirs, tmin, tmax, _I32, stack_entries)


def scene_cross_fill_native(handle, device_index, origins, dirs, tmin, tmax, count, offsets, total, want_front=False, want_loc=False,
                            want_uv=False, want_ray=False, ray_base: int = 0, stack_entries=0):
    """tr_scene_cross_fill: (instance int32[total], face int32[total], t float32[total], front bool[total] or None,
    loc float32[total, 3] or None, uv float32[total, 2] or None, ray int64[total] or None): the crossings of ray i by
    (t, instance, face) ascending at rows offsets[i] .. offsets[i] + count[i].  count int32[n] is scene_cross_count_native's
    (flattened) and offsets int64[n] its exclusive scan (tr_hits_scan) for the same rays and bounds; total (a Python int)
    sizes the outputs.  Nothing is allocated by the library and nothing is synchronised."""
    _scene_rays(origins, dirs, device_index)
    return _cross_fill(get_scene_cross_module().tr_scene_cross_fill, handle, True, origins, dirs, tmin, tmax, count, offsets, total,
                       want_front, want_loc, want_uv, want_ray, ray_base, stack_entries)


def scene_cross_all_native(handle, device_index, origins, dirs, tmin=None, tmax=None, want_front=False, want_loc=False, want_uv=False,
                           want_ray=False, ray_base: int = 0, stack_entries=0):
    """(offsets int64[n + 1], instance, face, t, front or None, loc or None, uv or None, ray or None) for the rays flattened
    in order: one count launch, one scan, one host read of the total to size the outputs, one fill: as cross_all_native."""
    return _count_scan_fill(scene_cross_count_native, scene_cross_fill_native, (handle, device_index, origins, dirs, tmin, tmax),
                            (stack_entries,), (want_front, want_loc, want_uv, want_ray, ray_base, stack_entries))


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
    flat, n, dev = _points_args(points)
    _on_scene_device(points, "points", device_index)
    if not isinstance(direction, torch.Tensor) or direction.device != dev or direction.dtype != torch.float32 or direction.numel() != 3:
        raise ValueError("direction must be a float32 tensor of three elements on the points' device")
    return flat, direction.reshape(3).contiguous(), n, dev


def _scene_points_query(query, handle, device_index, points, direction, stack_entries):
    column, fn = _any_or_count(query, _scene_points)
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, points.data_ptr(), n, direction.data_ptr(), out.data_ptr(), int(stack_entries))
    return out


def scene_points_any_native(handle, device_index, points, direction, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_any: bool[n], is each of points float32 [n, 3] inside some instance, by the parity of the crossings of
    (p, direction) and (p, -direction) per instance.  stack_entries: 0 = the whole stack, 1 .. capacity for tests (same
    results).  Nothing is allocated by the library and nothing is synchronised."""
    return _scene_points_query("any", handle, device_index, points, direction, stack_entries)


def scene_points_count_native(handle, device_index, points, direction, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_count: int32[n], how many instances each point is inside.  Arguments as scene_points_any_native."""
    return _scene_points_query("count", handle, device_index, points, direction, stack_entries)


def scene_points_fill_native(handle, device_index, points, direction, count, offsets, total, stack_entries=0) -> torch.Tensor:
    """tr_scene_points_fill: instance int32[total], the instances that hold point i ascending at rows offsets[i] ..
    offsets[i] + count[i].  count int32[n] is scene_points_count_native's and offsets int64[n] its exclusive scan
    (tr_hits_scan) for the same points and direction; total (a Python int) sizes the output.  Nothing is allocated by the
    library and nothing is synchronised."""
    lib = get_scene_points_module()
    points, direction, n, dev = _scene_points_args(points, direction, device_index)
    total = _check_fill(count, offsets, total, n, dev, "points")
    inst, = _outputs((total,), dev, _I32)
    _call(lib.tr_scene_points_fill, dev, handle, points.data_ptr(), n, direction.data_ptr(), count.data_ptr(), offsets.data_ptr(), total,
          _ptr_rows(inst), int(stack_entries))
    return inst


def scene_points_list_native(handle, device_index, points, direction, stack_entries=0):
    """(offsets int64[n + 1], instance int32[h]): one count launch, one scan, one host read of the total to size the output
    (as faces_in_boxes_native), one fill."""
    return _count_scan_fill(scene_points_count_native, scene_points_fill_native, (handle, device_index, points, direction),
                            (stack_entries,), (stack_entries,))


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
    flat, n, dev = _points_args(points)
    _on_scene_device(points, "points", device_index)
    lib = get_scene_nearest_module()
    rptr, r = (None, float("inf")) if max_distance is None else _radius(max_distance, "max_distance", n, dev, float("inf"))
    closest, distance, inst, tri = _outputs((n,), dev, want_closest and _F32X3, want_distance and _F32, _I32, _I32)
    _call(lib.tr_scene_closest_point, dev, handle, flat.data_ptr(), n, rptr, r, _ptr(closest), _ptr(distance), inst.data_ptr(), tri.data_ptr(),
          int(stack_entries))
    return closest, distance, inst, tri


# --- the placed faces of a scene that meet each query triangle (include/triro_scene_tris.h, csrc/scene_tris.hip) -----------
SCENE_TRIS_ABI_VERSION = 1    # TR_SCENE_TRIS_ABI_VERSION of include/triro_scene_tris.h

# every symbol include/triro_scene_tris.h declares: (restype, argtypes)
SCENE_TRIS_ABI = {
    "tr_scene_tris_abi_version": (_int, []),
    "tr_scene_tris_stack_capacity": (_int, []),
    "tr_scene_tris_any": (_int, [_vp, _vp, _i64, _vp, _int, _vp]),
    "tr_scene_tris_count": (_int, [_vp, _vp, _i64, _vp, _int, _vp]),
    "tr_scene_tris_fill": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _int, _vp]),
}


_scene_tris = _Satellite("scene_tris", SCENE_TRIS_ABI, get_scene_module)   # the scene handles are libtriro_scene.so's
scene_tris_library_path = _scene_tris.path
get_scene_tris_module = _scene_tris.load


def _scene_tris_args(tri, device_index):
    """(contiguous triangles, n, device) of float32 triangles [n, 3, 3] on the scene's GPU"""
    _, flat, n, dev = _tris_args(None, tri)
    _on_scene_device(tri, "triangles", device_index)
    return flat, n, dev


def scene_tris_native(handle, device_index, tri, query="any", stack_entries=0) -> torch.Tensor:
    """tr_scene_tris_any (query="any": bool[n]) / tr_scene_tris_count (query="count": int32[n]) for the world triangles, float32
    [n, 3, 3], on the scene's GPU: does any / how many (instance, face) pairs of the placed copies meet each.  stack_entries:
    0 = the whole stack, 1 .. capacity for tests (same results).  Nothing is allocated by the library and nothing is
    synchronised."""
    column, fn = _any_or_count(query, _scene_tris)
    tri, n, dev = _scene_tris_args(tri, device_index)
    out, = _outputs((n,), dev, column)
    _call(fn, dev, handle, tri.data_ptr(), n, out.data_ptr(), int(stack_entries))
    return out


def scene_tris_fill_native(handle, device_index, tri, count, offsets, total, stack_entries=0):
    """tr_scene_tris_fill: (instance int32[total], face int32[total]), the pairs of query i ascending by (instance, face index in
    the member mesh) at rows offsets[i] .. offsets[i] + count[i].  count int32[n] is scene_tris_native(..., "count") and offsets
    int64[n] its exclusive scan (tr_hits_scan) for the same queries; total (a Python int) sizes the outputs.  Nothing is
    allocated by the library and nothing is synchronised."""
    lib = get_scene_tris_module()
    tri, n, dev = _scene_tris_args(tri, device_index)
    total = _check_fill(count, offsets, total, n, dev, "triangles")
    inst, face = _outputs((total,), dev, _I32, _I32)
    _call(lib.tr_scene_tris_fill, dev, handle, tri.data_ptr(), n, count.data_ptr(), offsets.data_ptr(), total, _ptr_rows(inst),
          _ptr_rows(face), int(stack_entries))
    return inst, face


def scene_faces_meeting_triangles_native(handle, device_index, tri, stack_entries=0):
    """(offsets int64[n + 1], instance int32[h], face int32[h]): one count launch, one scan, one host read of the total to size
    the outputs (as faces_meeting_triangles_native), one fill."""
    return _count_scan_fill(scene_tris_native, scene_tris_fill_native, (handle, device_index, tri), ("count", stack_entries),
                            (stack_entries,))
