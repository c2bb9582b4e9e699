"""CPU checks of how triro.backend.ops finds, loads and binds the satellite libraries libtriro_<key>.so: the same five
properties for every key, through the public names only (X_ABI, X_ABI_VERSION, x_library_path, get_x_module).  What has to
be seen before a library is loaded (a missing file, a version that does not match, the order of the prerequisites) runs in a
fresh child process: this process may hold the library already."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("rccl", "points", "nearest", "range", "scene", "within", "cross", "scene_cross", "scene_points", "boxes", "tris", "planes",
        "scene_nearest", "tri_nearest", "scene_tris")
VERSIONED = tuple(k for k in KEYS if k != "rccl")          # libtriro_rccl.so has no version symbol
ON_THE_SCENE = ("scene_cross", "scene_points", "scene_nearest", "scene_tris")      # their handles are libtriro_scene.so's: it loads first

_vp, _int = ctypes.c_void_p, ctypes.c_int
# what get_rccl_module binds (include/triro_rccl.h), written out here so that the check does not depend on the table it checks
RCCL_BOUND = {
    "tr_rccl_last_error": (ctypes.c_char_p, []),
    "tr_rccl_available": (_int, []),
    "tr_comm_unique_id": (_int, [_vp]),
    "tr_comm_create": (_int, [_vp, _int, _int, _int, ctypes.POINTER(_vp)]),
    "tr_comm_destroy": (_int, [_vp]),
    "tr_comm_abort": (_int, [_vp]),
    "tr_sharded_closest_step": (_int, [_vp, _vp, None]),       # None: POINTER(hops.TrShardStep), filled in by _table
}


def _table(hops, key):
    if key != "rccl":
        return getattr(hops, f"{key.upper()}_ABI")
    table = {name: (res, list(args)) for name, (res, args) in RCCL_BOUND.items()}
    table["tr_sharded_closest_step"][1][2] = ctypes.POINTER(hops.TrShardStep)
    return table


def _child(code, **env):
    """run `code` in a fresh interpreter that can import triro; the environment is this one's plus `env`"""
    paths = [ROOT, os.path.join(ROOT, "trimesh-ray-optix_amd")]
    head = f"import sys; sys.path[:0] = {paths!r}; import triro.backend.ops as hops\n"
    return subprocess.run([sys.executable, "-c", head + code], env={**os.environ, **env}, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("key", KEYS)
def test_the_path_follows_from_the_key_and_the_environment_overrides_it(key, monkeypatch):
    import triro.backend.ops as hops
    var = f"TRIRO_{key.upper()}_LIBRARY"
    monkeypatch.delenv(var, raising=False)
    path = getattr(hops, f"{key}_library_path")
    assert path() == os.path.join(os.path.dirname(hops.library_path()), f"libtriro_{key}.so")
    monkeypatch.setenv(var, "/somewhere/else.so")
    assert path() == "/somewhere/else.so"


@pytest.mark.parametrize("key", KEYS)
def test_a_missing_library_raises_with_its_path(key, tmp_path):
    missing = str(tmp_path / f"no_such_{key}.so")
    r = _child(f"""
try:
    hops.get_{key}_module()
except RuntimeError as e:
    assert {missing!r} in str(e), str(e)
    print("RAISED")
""", **{f"TRIRO_{key.upper()}_LIBRARY": missing})
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("key", KEYS)
def test_the_library_loads_once_and_every_symbol_of_the_table_is_bound(key):
    import triro.backend.ops as hops
    get = getattr(hops, f"get_{key}_module")
    lib = get()
    assert get() is lib
    table = _table(hops, key)
    assert len(table) >= 3
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes or []) == list(args), name      # (a function without arguments may be left undeclared)
    if key in VERSIONED:
        assert getattr(lib, f"tr_{key}_abi_version")() == getattr(hops, f"{key.upper()}_ABI_VERSION")


def test_the_rccl_table_is_what_the_loader_binds():
    import triro.backend.ops as hops
    assert hops.RCCL_ABI == _table(hops, "rccl")


@pytest.mark.parametrize("key", VERSIONED)
def test_a_version_mismatch_raises_with_both_numbers(key):
    r = _child(f"""
have = hops.{key.upper()}_ABI_VERSION
hops.{key.upper()}_ABI_VERSION = 99
try:
    hops.get_{key}_module()
except RuntimeError as e:
    assert f"version {{have}} " in str(e) and "99" in str(e) and "libtriro_{key}.so" in str(e), str(e)
    print("RAISED")
""")
    assert r.returncode == 0 and "RAISED" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("key", ON_THE_SCENE)
def test_the_scene_library_is_loaded_before_a_library_on_its_handles(key):
    r = _child(f"""
import os
mapped = lambda: {{line.split()[-1] for line in open("/proc/self/maps") if "libtriro_" in line}}
scene, own = os.path.realpath(hops.scene_library_path()), os.path.realpath(hops.{key}_library_path())
assert scene not in mapped()                 # nothing is loaded at import time
hops.get_{key}_module()
assert {{scene, own, os.path.realpath(hops.library_path())}} <= mapped(), mapped()
print("LOADED")
""")
    assert r.returncode == 0 and "LOADED" in r.stdout, r.stdout + r.stderr
