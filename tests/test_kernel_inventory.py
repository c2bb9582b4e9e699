"""Which test checks which kernel (CPU only).

INVENTORY has one row per kernel of the gfx950 code object in libtriro_hip.so (demangled name, as
scripts/code_object_notes.kernels() reads it).  A row names the GPU test(s) that launch the kernel deterministically and
compare what it computes with the oracle or with an exact host computation -- or, as a string, why no such check
exists.  A kernel added to the library without a row, or a row whose kernel is gone, fails here.

The same module checks the options tests set: tests/launch_options.DEFAULTS against the initialisers of
`struct tr_options`, and that no test or fuzz dimension sets an option the library only accepts and ignores."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trimesh-ray-optix_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# ---- the new flavour matrix (tests/test_gpu_kernel_matrix.py) -----------------------------------------------------------
MATRIX = "test_gpu_kernel_matrix.py::test_flavour_matches_the_oracle"
CAPS = "test_gpu_kernel_matrix.py::test_multi_hit_lists_match_the_oracle_at_every_cap"
CAP_EDGES = "test_gpu_kernel_matrix.py::test_multi_hit_cap_range_and_ray_base"
SCANS = "test_gpu_kernel_matrix.py::test_scans_match_an_int64_cumsum"
COMPACTION = "test_gpu_kernel_matrix.py::test_compact_closest_with_a_ray_base"
# ---- the same flavours on rays at the ends of the float range (tests/test_gpu_hostile_rays.py): non-finite, zero, denormal and
# 3e38 components, origins at 2^60 ... 3.4e38, whole waves of invalid rays -- the oracle's bits and rules that need no oracle
HOSTILE = "test_gpu_hostile_rays.py::test_flavour_on_hostile_rays"
# ---- older tests ----------------------------------------------------------------------------------------------------------
BUILDER = "test_gpu_parity.py::test_builder_invariants_and_host_traversal_of_gpu_tree"
UPDATE = "test_gpu_parity.py::test_update_raw_rebuilds"
REFIT = "test_gpu_parity.py::test_refit_and_serialization"
PROBE = "test_gpu_round2.py::test_large_flat_batches_probe_and_both_launch_shapes"
STEADY = "test_gpu_round3.py::test_c2_steady_state_launches_match_the_oracle"
MOVING = "test_gpu_round3.py::test_c5i_moving_camera_sequence_matches_the_oracle"
PACKED = "test_gpu_round3.py::test_packed_closest_expands_to_the_dense_outputs_bit_for_bit"
PACKED_EDGES = "test_gpu_round3.py::test_packed_closest_edge_cases"
SLOTS = "test_gpu_round4.py::test_slot_form_records_expand_to_the_dense_outputs"
REPLICA = "test_gpu_round5.py::test_replica_hash_is_exact_and_stable"
WIDE = "test_gpu_wide.py::test_wide_streaming_matches_the_oracle"
# ---- the builder matrix (tests/test_gpu_builder_matrix.py): downloaded arrays against numpy references ---------------------
SIZES = "test_gpu_builder_matrix.py::test_size_ladder"
TIES = "test_gpu_builder_matrix.py::test_equal_keys_keep_their_input_order"
HEIGHTS = "test_gpu_builder_matrix.py::test_height_boundaries"
LAYOUT0 = "test_gpu_builder_matrix.py::test_node_layout_0"
BAD_FACE = "test_gpu_builder_matrix.py::test_bad_face_beyond_the_grid_cap"
REFIT_STRUCT = "test_gpu_builder_matrix.py::test_refit_structure"
REFIT_HANDLES = "test_gpu_builder_matrix.py::test_refit_of_loaded_saved_and_layout_0_handles"

STATS_ONLY = ("instrumented launch (tr_trace_stats_query): its query results go to internal scratch that is freed "
              "unread, only the traversal counters come back -- there is nothing to compare with the oracle")

INVENTORY = {}
# k_query_direct<Q, STATS, COMPACT (32-bit offsets), MODE (0 plain, 1 stealing, 2 unordered), DEEP (64-bit trail), QN (grid nodes)>
for q in (0, 1, 2):
    for flags in ("false, false, 0, false, false", "false, false, 1, false, false",          # generic: plain, stealing
                  "false, true, 0, false, false", "false, true, 0, true, false",             # compact / deep plain
                  "false, true, 1, false, false", "false, true, 1, true, false",             # stealing on exact nodes
                  "false, true, 1, false, true", "false, true, 1, true, true"):              # stealing on grid nodes
        INVENTORY[f"void k_query_direct<{q}, {flags}>"] = (MATRIX, HOSTILE)
    INVENTORY[f"void k_query_direct<{q}, true, false, 0, false, false>"] = STATS_ONLY
    # the stealing grid-node launch that carries the deferred sort of the learned order: <Q, DEEP, ...>
    INVENTORY[f"void k_query_direct_sort<{q}, false, true, true>"] = (MATRIX, HOSTILE)
    INVENTORY[f"void k_query_direct_sort<{q}, true, true, true>"] = (MATRIX, HOSTILE)
for q in (3, 4):
    for flags in ("false, false, 2, false, false", "false, true, 2, false, false", "false, true, 2, true, false"):
        INVENTORY[f"void k_query_direct<{q}, {flags}>"] = (MATRIX, HOSTILE, CAPS) if q == 4 else (MATRIX, HOSTILE)
    INVENTORY[f"void k_query_direct<{q}, true, false, 2, false, false>"] = STATS_ONLY
# the stealing count launch <COMPACT, DEEP> and its sort-carrying form
for flags in ("false, false", "true, false", "true, true"):
    INVENTORY[f"void k_query_count_steal<{flags}>"] = (MATRIX, HOSTILE)
INVENTORY["void k_query_count_steal_sort<false, true>"] = (MATRIX, HOSTILE)
INVENTORY["void k_query_count_steal_sort<true, true>"] = (MATRIX, HOSTILE)
for q in range(5):
    INVENTORY[f"void k_query_direct_wide<{q}>"] = (MATRIX, HOSTILE)
# streaming launches <Q, 32-bit offsets, block, DEEP> (no location query: it keeps the direct launch)
for q in range(4):
    for flags in ("false, 128, false", "true, 128, false", "true, 128, true"):
        INVENTORY[f"void k_query_stream<{q}, {flags}>"] = (MATRIX, HOSTILE)
    INVENTORY[f"void k_query_stream_stats<{q}, false, 128, false>"] = STATS_ONLY
    INVENTORY[f"void k_query_wide<{q}>"] = (MATRIX, HOSTILE, WIDE)
INVENTORY.update({
    # multi-hit lists: the two-pass fill (cap <= 8 / 16 / 32) and the fill from the fused traversal's slots
    "void k_location<8>": (CAPS, CAP_EDGES),
    "void k_location<16>": (CAPS,),
    "void k_location<32>": (CAPS,),
    "k_fill_list": (CAPS, CAP_EDGES, MATRIX, HOSTILE),
    "void k_scan_partial<int>": (SCANS, CAPS),
    "void k_scan_final<int>": (SCANS, CAPS),
    "void k_scan_partial<unsigned char>": (SCANS, COMPACTION),
    "void k_scan_final<unsigned char>": (SCANS, COMPACTION),
    "k_scan_partials": (SCANS,),
    "k_compact_closest": (COMPACTION,),
    # expansion of packed / slot records into the five dense outputs: bit-equal to the dense query
    "void k_closest_expand<1>": (PACKED_EDGES,),
    "void k_closest_expand_buf<4>": (PACKED,),
    "void k_closest_expand_slots<1, false>": (SLOTS,),
    "void k_closest_expand_slots<1, true>": (SLOTS,),
    "void k_closest_expand_slots<4, false>": (SLOTS,),
    "void k_closest_expand_slots<4, true>": (SLOTS,),
    "void k_closest_expand_slots_tiled<false, false>": (SLOTS,),
    "void k_closest_expand_slots_tiled<false, true>": (SLOTS,),
    "void k_closest_expand_slots_tiled<true, false>": (SLOTS,),
    "void k_closest_expand_slots_tiled<true, true>": (SLOTS,),
    # the builder: its output is a hierarchy, checked structurally and by a host traversal against the oracle
    "k_tri_bounds": (BUILDER, SIZES, BAD_FACE), "k_init_bounds": (BUILDER, SIZES), "k_morton": (BUILDER, SIZES),
    "k_rs_count": (BUILDER, SIZES, TIES), "k_rs_scan": (BUILDER, SIZES, TIES), "k_rs_scatter": (BUILDER, SIZES, TIES),
    "void k_karras<0>": (BUILDER, SIZES, HEIGHTS), "void k_karras<1>": (BUILDER, HEIGHTS),    # (launched only when plain keys give a height above 64)
    "k_refit_round": (BUILDER, REFIT, SIZES, HEIGHTS), "k_emit": (BUILDER, SIZES, HEIGHTS, LAYOUT0), "k_gather": (BUILDER, SIZES),
    "k_regather": (BUILDER, UPDATE, REFIT_STRUCT, REFIT_HANDLES, BAD_FACE),
    "k_layout_init": (BUILDER, SIZES), "k_layout_round": (BUILDER, SIZES, HEIGHTS), "k_qframe": (BUILDER, SIZES),
    "k_qframe_box": (REFIT, REFIT_STRUCT, REFIT_HANDLES),
    "k_refit_nodes_round": (REFIT, REFIT_STRUCT, REFIT_HANDLES), "k_update_boxes": (REFIT, REFIT_STRUCT, REFIT_HANDLES),
    # the 8-wide nodes are built on first use by the launches that walk them
    "k_wide_mark": (WIDE, MATRIX, HOSTILE), "k_wide_emit": (WIDE, MATRIX, HOSTILE),
    "k_replica_hash": (REPLICA,),
    # scheduling: these decide only the ORDER in which blocks run; the launches behind them are compared with the oracle
    "k_probe_coherence": (PROBE,),
    "k_sched_sort": (STEADY, MATRIX),
    "k_sched_rescale": (MOVING,),
})


def _shipped_kernels():
    import code_object_notes as con
    so = os.path.join(ROOT, "trimesh-ray-optix_amd", "lib", "libtriro_hip.so")
    if not os.path.exists(so) or not os.path.exists(con.READELF):
        pytest.skip("library not built / llvm-readelf not available")
    return {k["name"] for k in con.kernels(so)}


def test_every_shipped_kernel_has_one_inventory_row():
    names = _shipped_kernels()
    missing = sorted(names - set(INVENTORY))
    stale = sorted(set(INVENTORY) - names)
    assert not missing, f"kernels in libtriro_hip.so without an inventory row: {missing}"
    assert not stale, f"inventory rows of kernels that are not in libtriro_hip.so: {stale}"


def test_inventory_rows_name_existing_tests_or_a_reason():
    for kernel, row in INVENTORY.items():
        if isinstance(row, str):
            assert len(row) > 40, (kernel, row)
            continue
        assert row, kernel
        for test_id in row:
            module, func = test_id.split("::")
            src = open(os.path.join(ROOT, "tests", module)).read()
            assert re.search(rf"^def {func}\(", src, re.M), f"{kernel}: {test_id} does not exist"
            assert "pytest.mark.gpu" in src, f"{kernel}: {test_id} is not a GPU test"
    # the families the flavour matrix exists for: every 64-bit-addressing traversal kernel, the wide list kernels
    # (<Q, STATS = false, COMPACT = false, ...> direct: plain and stealing for 3 queries + unordered for 2; streaming
    # <Q, COMPACT = false, ...> for 4; the stealing count launch <COMPACT = false, DEEP = false>)
    generic = [k for k in INVENTORY if re.match(r"void k_query_direct<\d, false, false,", k)
               or re.match(r"void k_query_stream<\d, false,", k) or k == "void k_query_count_steal<false, false>"]
    assert len(generic) == 3 * 2 + 2 + 4 + 1
    for k in generic + ["void k_location<16>", "void k_location<32>"]:
        assert isinstance(INVENTORY[k], tuple) and any(t.startswith("test_gpu_kernel_matrix.py") for t in INVENTORY[k]), k


def _struct_tr_options():
    src = open(os.path.join(CSRC, "tr_internal.h")).read()
    body = re.search(r"struct tr_options \{(.*?)\n\};", src, re.S).group(1)
    fields = re.findall(r"^\s*int (\w+) = (-?\d+);", body, re.M)
    assert len(fields) == len(re.findall(r"^\s*int ", body, re.M)), "a field of tr_options without an integer initialiser"
    return {k: int(v) for k, v in fields}


def _fuzz_defaults():
    """the DEFAULTS literal of scripts/fuzz_parity.py (a script: parsed, not imported)"""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "DEFAULTS" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("scripts/fuzz_parity.py has no DEFAULTS")


def test_option_defaults_match_struct_tr_options():
    from launch_options import DEFAULTS
    assert DEFAULTS == _struct_tr_options()
    # the fuzz script restores the same values after every iteration
    assert _fuzz_defaults() == DEFAULTS
    # ... and every field is an option tr_set_option knows by that name (csrc/api.hip's table)
    api = open(os.path.join(CSRC, "api.hip")).read()
    table = dict(re.findall(r'\{"(\w+)", &tr_options::(\w+),', api))
    assert all(k == v for k, v in table.items()) and set(table) == set(DEFAULTS), table


def _retired_names():
    api = open(os.path.join(CSRC, "api.hip")).read()
    lst = re.search(r"for \(const char\* retired : \{(.*?)\}\)", api, re.S).group(1)
    names = re.findall(r'"(\w+)"', lst)
    assert len(names) >= 13
    return names


def test_no_test_or_fuzz_dimension_sets_a_retired_option():
    """A retired name is accepted and ignored by tr_set_option: a test that sets one claims coverage of a launch shape
    that no longer exists.  Quoted option keys ('name' / "name") and keyword arguments (name=) are caught; the one
    place allowed is the check that retired names are still accepted."""
    names = _retired_names()
    pat = re.compile(r"""(["'])(%s)\1|\b(%s)\s*=""" % ("|".join(names), "|".join(names)))
    files = sorted(os.path.join(ROOT, "tests", f) for f in os.listdir(os.path.join(ROOT, "tests")) if f.endswith(".py"))
    files.append(os.path.join(ROOT, "scripts", "fuzz_parity.py"))
    hits = []
    for path in files:
        for n, line in enumerate(open(path), 1):
            if pat.search(line):
                hits.append((os.path.relpath(path, ROOT), n, line.strip()))
    allowed = [h for h in hits if h[0] == os.path.join("tests", "test_gpu_round2.py") and h[2].startswith("for retired, value in (")]
    assert len(allowed) == 1, hits
    assert [h for h in hits if h not in allowed] == []


# the occupancy budgets (tests/test_round4_cpu.py pins them) and the branch hint of the open fault investigation
# (scripts/round6/fault_probe.py builds with it)
KEPT_SWITCHES = {"TR_DIRECT_WAVES", "TR_DEEP_WAVES", "TR_COUNT_WAVES", "TR_STREAM_WAVES", "TR_WIDE_WAVES", "TR_DRAIN_COLD"}


def test_kernel_sources_keep_only_the_listed_build_switches():
    """Every TR_ name the kernel sources test in the preprocessor (#ifdef / #ifndef / #if / #elif, defined(...)) is a
    build switch: a `make EXTRA=-DTR_...` build swaps in another kernel.  The closed experiments' switches were retired
    (experiments/README.md, "Retired build switches") so that the source shows exactly what ships, and so that a -D build
    of a switch that stopped mattering cannot measure the default and report it as a variant.  A new switch has to be
    added to KEPT_SWITCHES on purpose."""
    directive = re.compile(r"^\s*#\s*(?:ifdef|ifndef|if|elif)\b(.*)$")
    tested = {}
    for f in sorted(os.listdir(CSRC)):
        for n, line in enumerate(open(os.path.join(CSRC, f), errors="replace"), 1):
            m = directive.match(line.split("//")[0])
            if m:
                for name in re.findall(r"\bTR_\w+", m.group(1)):
                    tested.setdefault(name, []).append(f"{f}:{n}")
    assert set(tested) == KEPT_SWITCHES, {k: v for k, v in tested.items() if k not in KEPT_SWITCHES}


# ---- poisoned outputs (tests/poison.py) stay on ------------------------------------------------------------------------------
# a GPU test module that may run without poisoned outputs: {file name: why what it compares cannot be stale memory}
UNPOISONED_GPU_MODULES = {}
# the standalone GPU scripts (children of GPU tests) that compare query results: they call poison.install() themselves
POISONED_SCRIPTS = ("native_step_world1.py", "nccl_world1.py", "gloo_world2_gpu.py", "native_abort_world1.py")
# a function of ops.py / sharded.py that may allocate uninitialised memory besides the seam: {(file, function): why}
UNINITIALISED_ALLOCATIONS = {}


def _applies_the_gpu_marker(src):
    return bool(re.search(r"^pytestmark\s*=.*\bpytest\.mark\.gpu\b", src, re.M) or re.search(r"^\s*@pytest\.mark\.gpu\b", src, re.M))


def test_every_gpu_test_module_runs_on_poisoned_outputs():
    """A result read from a torch.empty buffer that the caching allocator recycled from an earlier, correct launch proves
    nothing about the launch under test (tests/poison.py).  Every module that applies the GPU marker imports the autouse
    fixture; every standalone GPU script installs the net itself."""
    tests = os.path.join(ROOT, "tests")
    gpu_modules = []
    for f in sorted(os.listdir(tests)):
        if not f.endswith(".py"):
            continue
        src = open(os.path.join(tests, f)).read()
        if not _applies_the_gpu_marker(src):
            continue
        gpu_modules.append(f)
        if f in UNPOISONED_GPU_MODULES:
            assert len(UNPOISONED_GPU_MODULES[f]) > 40, f
            continue
        assert re.search(r"^from poison import (?:\w+, )*poisoned_outputs\b", src, re.M), \
            f"tests/{f} applies pytest.mark.gpu but does not import poison.poisoned_outputs"
    assert len(gpu_modules) >= 18 and "test_poison.py" in gpu_modules, gpu_modules
    assert "test_kernel_inventory.py" not in gpu_modules          # (it only names the marker in a string)
    assert not set(UNPOISONED_GPU_MODULES) - set(gpu_modules), "an exemption for a module that is gone"
    for f in POISONED_SCRIPTS:
        src = open(os.path.join(tests, f)).read()
        assert re.search(r"^import poison\b", src, re.M) and re.search(r"^poison\.install\(\)", src, re.M), f"tests/{f} does not install the poison"


def test_the_backend_allocates_uninitialised_memory_only_in_the_seam():
    """`_new_output` of triro/backend/ops.py and of triro/ray/sharded.py is what tests/poison.py swaps: a torch.empty
    (empty_like, new_empty, empty_strided) anywhere else is an output the net does not see."""
    import ast
    for rel in (("backend", "ops.py"), ("ray", "sharded.py")):
        path = os.path.join(ROOT, "trimesh-ray-optix_amd", "triro", *rel)
        tree = ast.parse(open(path).read())
        assert any(isinstance(n, ast.FunctionDef) and n.name == "_new_output" for n in tree.body), f"{rel[1]} has no module-level _new_output"
        found = []

        def walk(node, func):
            for child in ast.iter_child_nodes(node):
                inner = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else func
                if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and \
                        child.func.attr in ("empty", "empty_like", "empty_strided", "new_empty"):
                    found.append((rel[1], func, child.lineno))
                walk(child, inner)
        walk(tree, None)
        outside = [x for x in found if x[1] != "_new_output" and (x[0], x[1]) not in UNINITIALISED_ALLOCATIONS]
        assert [x for x in found if x[1] == "_new_output"], f"{rel[1]}: _new_output no longer allocates with torch.empty"
        assert not outside, f"uninitialised allocations outside the seam (file, function, line): {outside}"
    assert all(len(why) > 40 for why in UNINITIALISED_ALLOCATIONS.values())
