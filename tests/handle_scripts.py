"""Scripted histories of ONE handle (tests/test_gpu_handle_scripts.py runs them, tests/test_handle_scripts_cpu.py checks the
table itself); not a test module.

A tr_bvh and its (stream, class) scheduling slots carry state from call to call: the arena (grows, never shrinks, re-carved
in place), the learned block order (two buffers, `cur`, a stamp, `launches`), a deferred sort waiting for a launch that can
carry it, the kept costs of the last sort, the 8-wide nodes and their temporaries, refit_temp, and the grid frame / depth /
key mode that pick the addressing flavour.  The rest of the suite enters each of these from a fresh handle; the scripts here
are short, named sequences of meshes, batches and options on one handle, each aimed at a piece of that state, each launch
compared with the oracle bit for bit, and each script asserting through tr_bvh_last_launch that it reached the state it names.

A script is a list of steps (tuples):

    ("opts", {...})                    set library options (names of launch_options.DEFAULTS); they stay until changed
    ("build", mesh)                    a fresh RayMeshIntersector
    ("update", mesh)                   update_raw on the handle
    ("refit", mesh)                    refit to a mesh with the same faces
    ("save_load",)                     save, load: the script goes on with the LOADED handle
    ("fail_update",)                   update_raw to "bad" raises and leaves an empty handle
    ("launch", query, batch, times)    `times` launches, each compared with the oracle and checked for unwritten elements
    ("points",)                        contains_points, closest_point and signed_distance on the mesh's points
    ("stream", k)                      go on on stream k (0: the default stream)
    ("sync",)                          device synchronisation
    ("capture", query, batch)          record one launch into a graph on the current stream
    ("replay",)                        replay it, compare with the oracle for the mesh the handle holds now
    ("expect", {...})                  about the records of the last launch step: see EXPECT

Ordering across streams is the caller's duty and not what is tested: ("stream", k) and every mesh transition
run between two device synchronisations.  Between a capture and its last replay a script holds no update, save_load,
fail_update or build: a rebuild may move the arena the recorded launch points into (check_table enforces it on the table)."""
import contextlib
import functools

import numpy as np

import hostile_meshes as M
import workloads as W

F32 = np.float32
QUERIES = ("any", "first", "closest", "count", "location")
STREAMING = ("any", "first", "closest", "count")                 # (the location query has no streaming launch)
STEPS = {"opts": 1, "build": 1, "update": 1, "refit": 1, "save_load": 0, "fail_update": 0, "launch": 3, "points": 0,
         "stream": 1, "sync": 0, "capture": 2, "replay": 0, "expect": 1}
TRANSITIONS = ("build", "update", "refit", "save_load", "fail_update")
MOVES_THE_ARENA = ("build", "update", "save_load", "fail_update")
DIRECTION = np.array([-0.3, 0.2, 0.9], F32)                      # contains_points: explicit, so no retry direction is drawn
RETRY = np.array([0.21, -0.43, 0.37], F32)                        # ... and the default direction with this retry handed in
PILE_RAY = (np.array([1e-10, 1e-10, 1.0], F32), np.array([0.0, 0.0, -1.0], F32))
IMAGES = {"img128": (128, 128), "img256x64": (256, 64), "img136": (128, 136)}      # (width, height)
BATCHES = tuple(IMAGES) + ("flat",)
# what ("expect", {...}) can say about the records (tr_bvh_last_launch) of the launch step before it
EXPECT = {
    "learned_from": "launch k (0-based) and every later one ran on a learned order",
    "cold_first": "the first launch had no learned order",
    "carried": "exactly these launches (0-based) carried the deferred sort",
    "split_some": "at least one launch had split blocks",
    "blocks": "block count of every launch",
    "blocks_not": "no launch had this block count",
    "shape": "tr_launch_info.shape of every launch",
    "addressing": "tr_launch_info.addressing of every launch",
    "tile_rows_lg": "rows-per-tile exponent of every launch",
    "depth_above": "bvh_info()['depth'] is above this",
    "depth_up_to": "bvh_info()['depth'] is at most this",
}


# ---- meshes -------------------------------------------------------------------------------------------------------------
def _sphere():
    v, f = W.icosphere(5)
    return W.displaced(v, seed=4, amplitude=0.07), f


def _sphere_moved():
    v, f = _sphere()
    return (W.displaced(v, seed=9, amplitude=0.08) * F32(1.35) + F32([0.2, -0.1, 0.15])).astype(F32), f


def _soup():
    """24 000 triangles: MORE than `sphere` (20 480), so that an update from it grows the arena and outgrows the 8-wide
    buffers.  (20 000, the first plan, is fewer: the arena would have been re-carved, not grown.)"""
    return W.random_soup(24000, seed=5)


def _soup_moved():
    v, f = _soup()
    return (v * F32(0.8) + F32([-0.15, 0.1, 0.2])).astype(F32), f


def _shells_moved():
    v, f = W.nested_shells(3)
    return (v * F32(1.2) + F32([0.1, -0.25, 0.05])).astype(F32), f


def _deep():
    """the deep tree (its triangles are 1e-9 wide: no camera sees them) plus a sphere inside its box that a camera does see"""
    v, f = W.deep_tree_mesh(3000)
    sv, sf = W.icosphere(3)
    sv = (W.displaced(sv, seed=6, amplitude=0.05) * F32(0.375) + F32(0.5)).astype(F32)
    return np.concatenate([v, sv]).astype(F32), np.concatenate([f, sf + np.int32(len(v))]).astype(np.int32)


def _bad():
    v, f = _sphere()
    f = f.copy()
    f[777, 1] = len(v) + 5
    return v, f


def _hostile():
    c = M.case("nonfinite", 0)
    assert np.isnan(c.v).any() and np.isinf(c.v).any()
    return c.v, c.f


_MESHES = {
    "sphere": _sphere, "sphere_moved": _sphere_moved, "soup": _soup, "soup_moved": _soup_moved,
    "shells": lambda: W.nested_shells(3), "shells_moved": _shells_moved, "deep": _deep,
    "two": W.two_triangles, "one": lambda: (W.two_triangles()[0], W.two_triangles()[1][:1]),
    "none": lambda: (W.two_triangles()[0], W.two_triangles()[1][:0]), "hostile": _hostile, "bad": _bad,
}
MESHES = tuple(_MESHES)
SAME_FACES = {"sphere_moved": "sphere", "sphere": "sphere_moved", "shells_moved": "shells", "shells": "shells_moved",
              "soup_moved": "soup", "soup": "soup_moved"}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices float32 [nv, 3], faces int32 [nf, 3]), read-only"""
    v, f = _MESHES[name]()
    v, f = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def answering(name):
    """the mesh a handle answers for after a transition to `name`: "bad" leaves an empty handle"""
    v, f = mesh(name)
    return (v, f[:0]) if name == "bad" else (v, f)


def box(name):
    """bounds of the mesh's finite vertices"""
    v = mesh(name)[0]
    v = v[np.isfinite(v).all(1)]
    return v.min(0).astype(np.float64), v.max(0).astype(np.float64)


# ---- batches ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(mesh_name, name):
    """(origins, directions) float32: [h, w, 3] for the images, [16384, 3] for "flat"; read-only"""
    lo, hi = box(mesh_name)
    if name in IMAGES:
        w, h = IMAGES[name]
        o, d = W.pinhole_grid(w, h, distance=1.25 * float(np.linalg.norm(hi - lo)), center=(lo + hi) / 2)
    elif name == "flat":
        ext = hi - lo
        o, d = W.hash_rays(16384, 41, lo - 0.2 * ext, hi + 0.2 * ext)
        if mesh_name == "deep":                        # a wave of rays down the pile of 3000 identical triangles
            o[:64], d[:64] = PILE_RAY
    else:
        raise KeyError(name)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def points(mesh_name):
    lo, hi = box(mesh_name)
    c, ext = (lo + hi) / 2, hi - lo
    p = np.ascontiguousarray(W.hash_rays(2048, 43, c - 0.6 * ext, c + 0.6 * ext)[0], F32)
    p.setflags(write=False)
    return p


# ---- expected values (each computed once, never changed) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(mesh_name):
    from oracle.oracle import OracleIntersector
    return OracleIntersector(*answering(mesh_name), 1)


@functools.lru_cache(maxsize=None)
def expected(mesh_name, batch_name, rays_of=None):
    """the oracle's results of `mesh_name` on the batch made for mesh `rays_of` (None: for itself), in the form
    test_gpu_kernel_matrix.check_query takes"""
    R = _oracle(mesh_name)
    o, d = batch(rays_of or mesh_name, batch_name)
    of, df = o.reshape(-1, 3), d.reshape(-1, 3)
    out = {"closest": R.closest_raw(of, df)[:5], "count": R.intersects_count(of, df), "location": R.intersects_location(of, df)}
    for x in (*out["closest"], out["count"], *out["location"]):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_points(mesh_name):
    """{"nearest": (closest, distance, tri) of the brute force, "contains": the oracle's contains_points along DIRECTION (one
    unresolved point makes that all False: the reference's quirk), "contains_retry": along the default direction, unresolved
    points retried along RETRY}"""
    import nearest_sim
    v, f = answering(mesh_name)
    p = points(mesh_name)
    out = {"nearest": nearest_sim.brute(v, f, p), "contains": _oracle(mesh_name).contains_points(p, DIRECTION),
           "contains_retry": _oracle(mesh_name).contains_points(p, None, _retry_dirs=iter([RETRY] * 4))}
    for x in (*out["nearest"], out["contains"], out["contains_retry"]):
        x.setflags(write=False)
    return out


# ---- the scripts --------------------------------------------------------------------------------------------------------
TILED = {"tile": 2, "split": 2}          # 8 x 8 tiles and split blocks at 128 blocks (test_image_tiles_split_blocks_and_the_learned_order)


def _pending_meets_rebuild():
    """1.  Under TILED the first launch of a shape runs plain, the second takes the wanted shape and resets `launches`, so
    it is the FIFTH launch that measures in the steady state and defers its sort (launches == 3 in sched_measure), and the
    sixth that carries it and flips `cur`.  (The issue counted the fourth and the fifth: that holds where the plain and the
    wanted shape are the same, as in scripts 2 and 7.)  The mesh changes once while the sort is pending and once right
    after it was carried; afterwards the waiting sort cannot ride in a launch that measures and runs as a kernel of its own."""
    s = []
    for query in ("closest", "first", "any", "count"):
        # update_raw keeps the order and resets `launches`: the waiting sort runs in front of launch 0 (which measures), launch 2
        # defers the next one, launch 3 carries it.  refit leaves `launches` alone: launch 0 carries the waiting sort itself.
        for before, transition, carried in ((5, ("update", "soup"), [3]), (6, ("update", "soup"), [3]), (5, ("refit", "sphere_moved"), [0, 4])):
            s += [("opts", dict(TILED)), ("build", "sphere"), ("launch", query, "img128", before),
                  ("expect", {"cold_first": True, "learned_from": 1, "blocks": 128, "addressing": 1, "tile_rows_lg": 3,
                              "carried": [5] if before == 6 else []}),
                  transition, ("launch", query, "img128", 6),
                  ("expect", {"learned_from": 0, "carried": carried, "split_some": True, "blocks": 128})]
    return s


def _pending_meets_option_flips():
    """2.  Default options: the plain and the wanted shape are one, so the fourth launch of the shape (launches == 3 in
    sched_measure, and every fourth after it) measures and defers its sort.  Each flip meets such a waiting sort: the option
    changes for its launches, goes back, and default launches run on to the next deferred sort (`launches` is in the
    comments).  sort_inline = 0, grid_nodes = 0, compact = 0 and steal = 0 cannot carry it -- it runs as a kernel of its own
    in front --, adaptive = 0 leaves the slot alone and the sort waiting (the first launch under adaptive = 1 carries it),
    steal = 2 carries it.  Then the other queries on the slot the closest launches taught."""
    img = ("closest", "img128")
    s = [("build", "sphere"), ("launch", *img, 4),                                                           # 0 1 2 3: pending
         ("expect", {"cold_first": True, "learned_from": 1, "carried": [], "blocks": 128, "shape": 1, "addressing": 1}),
         ("opts", {"sort_inline": 0}), ("launch", *img, 1), ("expect", {"carried": [], "learned_from": 0}),      # 4
         ("opts", {"sort_inline": 1}), ("launch", *img, 3), ("expect", {"carried": [], "learned_from": 0}),      # 5 6 7: pending
         ("opts", {"grid_nodes": 0}), ("launch", *img, 1), ("expect", {"carried": [], "learned_from": 0}),       # 8
         ("opts", {"grid_nodes": 1}), ("launch", *img, 3), ("expect", {"carried": [], "learned_from": 0}),       # 9 10 11: pending
         ("opts", {"adaptive": 0}), ("launch", *img, 1), ("expect", {"carried": [], "cold_first": True}),        # (no slot)
         ("opts", {"adaptive": 1}), ("launch", *img, 3), ("expect", {"carried": [0], "learned_from": 0}),        # 12 13 14
         ("launch", *img, 1), ("expect", {"carried": []}),                                                       # 15: pending
         ("opts", {"compact": 0}), ("launch", *img, 3), ("expect", {"carried": [], "addressing": 0, "learned_from": 0}),   # 16 17 18
         ("opts", {"compact": 1}), ("launch", *img, 1), ("expect", {"carried": [], "addressing": 1}),            # 19: pending
         ("opts", {"steal": 0}), ("launch", *img, 1), ("expect", {"carried": [], "shape": 0, "learned_from": 0}),          # 20
         ("opts", {"steal": 1}), ("launch", *img, 3), ("expect", {"carried": [], "shape": 1}),                   # 21 22 23: pending
         ("opts", {"steal": 2}), ("launch", *img, 1), ("expect", {"carried": [0], "shape": 1, "learned_from": 0}),         # 24
         ("opts", {"steal": 1}),
         ("launch", "count", "img128", 3), ("expect", {"shape": 3, "blocks": 128}),
         ("launch", "location", "img128", 2), ("expect", {"shape": 2, "blocks": 128})]
    return s


def _shared_block_counts():
    """3.  Three batch shapes of 128 blocks and one of 136, five queries, one scheduling slot per class: every launch reads
    an order some other (query, shape) left behind, or has to notice by the stamp that it cannot."""
    s = [("opts", dict(TILED)), ("build", "sphere")]
    for query, name, times in (("closest", "img128", 4), ("count", "flat", 2), ("first", "img256x64", 2), ("location", "img128", 2),
                               ("closest", "img136", 3), ("count", "img128", 2), ("any", "flat", 4), ("closest", "img128", 2)):
        s += [("launch", query, name, times),
              ("expect", dict({"blocks": 136, "blocks_not": 128} if name == "img136" else {"blocks": 128}, learned_from=1))]
    s[3] = ("expect", {"blocks": 128, "cold_first": True, "learned_from": 1, "split_some": True, "tile_rows_lg": 3})
    return s


def _every_query(expect):
    s = []
    for name in ("img128", "flat"):
        for query in QUERIES:
            s += [("launch", query, name, 3), ("expect", dict(expect))]
    return s + [("points",)]


def _size_classes():
    """4.  The arena grows, is re-carved in place for smaller meshes, holds meshes without a hierarchy and an empty mesh, is
    refitted, saved, loaded (a loaded arena is exactly as large as the saved mesh: the next update grows it), emptied by a
    failed update, and changes between 32- and 64-bit trail words (`deep`)."""
    with_tree = {"addressing": 1, "depth_up_to": 32}
    deep = {"addressing": 2, "depth_above": 32}
    s = [("build", "sphere")] + _every_query(with_tree)
    for step, expect in ((("update", "deep"), deep), (("update", "two"), {}), (("update", "one"), {}), (("update", "none"), {}),
                         (("update", "soup"), with_tree), (("update", "shells"), with_tree), (("refit", "shells_moved"), with_tree),
                         (("save_load",), with_tree), (("update", "sphere"), with_tree), (("fail_update",), {}),
                         (("update", "sphere"), with_tree), (("update", "hostile"), with_tree), (("update", "deep"), deep)):
        s += [step] + _every_query(expect)
    return s


def _wide_follows_the_handle():
    """5.  The 8-wide nodes are built by the first launch that wants them and have to follow every later mesh: more nodes
    than the buffers hold, fewer, a refit, a deep hierarchy (the node stack spills), a mesh without a hierarchy."""
    def both(direct_expect):
        s = [("opts", {"stream": 2, "wide": 1, "wide_direct": 1})]
        s += [("launch", query, "flat", 1) for query in STREAMING]
        s += [("opts", {"stream": 0, "wide_direct": 3})]
        for query in QUERIES:
            s += [("launch", query, "img128", 1), ("expect", dict(direct_expect))]
        return s
    s = [("opts", {"stream": 2, "wide": 1}), ("build", "sphere")] + both({"shape": 4, "addressing": 1})
    for step, expect in ((("update", "soup"), {"shape": 4, "addressing": 1}), (("update", "shells"), {"shape": 4, "addressing": 1}),
                         (("refit", "shells_moved"), {"shape": 4, "addressing": 1}), (("update", "deep"), {"shape": 4, "addressing": 2}),
                         (("update", "two"), {}), (("update", "sphere"), {"shape": 4, "addressing": 1})):
        s += [step] + both(expect)
    return s


def _two_streams():
    """6.  Each stream has scheduling slots of its own on the one handle; a transition enqueued on one stream changes what
    both read."""
    def interleaved():
        s = []
        for _ in range(3):
            s += [("stream", 1), ("launch", "closest", "img128", 1), ("expect", {"blocks": 128}),
                  ("stream", 2), ("launch", "count", "flat", 1), ("expect", {"blocks": 128, "shape": 3})]
        return s
    s = [("build", "sphere"),
         ("stream", 1), ("launch", "closest", "img128", 5), ("expect", {"cold_first": True, "learned_from": 1, "carried": [4]}),
         ("stream", 2), ("launch", "count", "flat", 5), ("expect", {"cold_first": True, "learned_from": 1, "shape": 3}),
         ("sync",), ("stream", 1), ("update", "soup"), ("sync",)] + interleaved()
    s += [("sync",), ("stream", 2), ("refit", "soup_moved"), ("sync",)] + interleaved()
    return s + [("stream", 0)]


def _replay_after_the_slot_was_rewritten():
    """7.  A recorded launch has the pointer of the order buffer it read frozen in the graph.  Eager launches of other batch
    shapes on the stream rewrite both buffers and their stamps; the replayed kernel has to notice by the stamp (a stale order
    of 136 blocks under a launch of 128 would leave blocks out or run them twice).  Refits move the bounds under it."""
    return [("build", "sphere"), ("stream", 1), ("launch", "closest", "img128", 4),
            ("expect", {"learned_from": 1, "carried": [], "blocks": 128}),
            ("capture", "closest", "img128"), ("expect", {"carried": [], "blocks": 128}),
            ("launch", "closest", "flat", 4), ("expect", {"blocks": 128}),
            ("launch", "closest", "img136", 4), ("expect", {"blocks": 136}),
            ("replay",), ("refit", "sphere_moved"), ("replay",),
            ("launch", "count", "img128", 4), ("expect", {"blocks": 128, "shape": 3}), ("replay",),
            ("refit", "sphere"), ("replay",), ("stream", 0)]


SCRIPTS = {
    "pending_sort_meets_a_rebuild": _pending_meets_rebuild(),
    "pending_sort_meets_option_flips": _pending_meets_option_flips(),
    "shapes_share_a_block_count": _shared_block_counts(),
    "size_classes_on_one_handle": _size_classes(),
    "wide_nodes_follow_the_handle": _wide_follows_the_handle(),
    "two_streams_one_handle": _two_streams(),
    "graph_replay_after_the_slot_was_rewritten": _replay_after_the_slot_was_rewritten(),
}


# ---- the table's own rules (no GPU) -------------------------------------------------------------------------------------
def check_table(script):
    """vocabulary, names, and the safety rule: nothing that may move the arena between a capture and its last replay"""
    from launch_options import DEFAULTS
    assert script and script[0][0] in ("opts", "build"), "a script starts by building a handle"
    current, built, captured_at, last_replay, stream = None, False, None, None, 0
    for k, step in enumerate(script):
        kind, args = step[0], step[1:]
        assert kind in STEPS and len(args) == STEPS[kind], f"step {k}: {step}"
        if kind == "opts":
            assert args[0] and all(name in DEFAULTS for name in args[0]), f"step {k}: {step}"
        elif kind in ("build", "update"):
            assert args[0] in MESHES and args[0] != "bad", f"step {k}: {step}"
            current = args[0]
        elif kind == "refit":
            assert SAME_FACES.get(args[0]) == current or args[0] == current, f"step {k}: refit from {current} to {args[0]}"
            assert np.array_equal(mesh(args[0])[1], mesh(current)[1])
            current = args[0]
        elif kind == "fail_update":
            current = "bad"
        elif kind in ("launch", "capture"):
            assert args[0] in QUERIES and args[1] in BATCHES and (kind == "capture" or args[2] >= 1), f"step {k}: {step}"
            assert kind == "launch" or args[0] != "location", f"step {k}: the list query reads its total on the host"
        elif kind == "stream":
            assert isinstance(args[0], int) and 0 <= args[0] <= 2, f"step {k}: {step}"
            stream = args[0]
        elif kind == "expect":
            assert args[0] is not None and all(name in EXPECT for name in args[0]), f"step {k}: {step}"
            assert k > 0 and script[k - 1][0] in ("launch", "capture"), f"step {k}: an expect follows a launch or a capture"
        built = built or kind == "build"
        assert built or kind == "opts", f"step {k}: {kind} before the build"
        if kind == "capture":
            assert captured_at is None, f"step {k}: one capture per script"
            assert stream != 0, f"step {k}: a capture needs a side stream"
            captured_at = k
        if kind == "replay":
            assert captured_at is not None, f"step {k}: replay without a capture"
            last_replay = k
    if captured_at is not None:
        assert last_replay is not None, "a capture that is never replayed"
        between = [s[0] for s in script[captured_at:last_replay] if s[0] in MOVES_THE_ARENA]
        assert not between, f"{between} between a capture and its last replay: the arena may move under the recorded launch"
    assert script[-1] == ("stream", 0) or not any(s[0] == "stream" for s in script), "a script ends on the default stream"


def count_launches(script):
    return sum(s[3] for s in script if s[0] == "launch") + sum(1 for s in script if s[0] in ("capture", "replay"))


# ---- the interpreter (GPU) ----------------------------------------------------------------------------------------------
def _check_expect(want, records, info, what):
    lis = [li for li in records if li is not None]
    assert lis and len(lis) == len(records), f"{what}: a launch left no record of a direct launch: {records}"
    brief = [(li["learned_order"], li["split_blocks"], li["sort_carried"], li["blocks"], li["shape"], li["addressing"]) for li in lis]
    tell = f"{what}: expected {want}; (learned order, split blocks, sort carried, blocks, shape, addressing) per launch: {brief}"
    for name, value in want.items():
        if name == "learned_from":
            assert all(li["learned_order"] == 1 for li in lis[value:]), tell
        elif name == "cold_first":
            assert lis[0]["learned_order"] == 0, tell
        elif name == "carried":
            assert [k for k, li in enumerate(lis) if li["sort_carried"]] == list(value), tell
        elif name == "split_some":
            assert any(li["split_blocks"] > 0 for li in lis), tell
        elif name == "blocks_not":
            assert all(li["blocks"] != value for li in lis), tell
        elif name in ("blocks", "shape", "addressing", "tile_rows_lg"):
            assert all(li[name] == value for li in lis), tell
        elif name == "depth_above":
            assert info["depth"] > value, f"{what}: depth {info['depth']}"
        elif name == "depth_up_to":
            assert info["depth"] <= value, f"{what}: depth {info['depth']}"
        else:
            raise KeyError(name)


@contextlib.contextmanager
def _checked_point_queries():
    """closest_point_native / contains_points_native are not among poison's entry points: every eager call of the script
    comes back through assert_written here"""
    import torch
    import poison
    import triro.backend.ops as hops
    saved = {name: getattr(hops, name) for name in ("closest_point_native", "contains_points_native")}

    def checked(name):
        def call(*args, **kwargs):
            res = saved[name](*args, **kwargs)
            if not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize()
                poison.assert_written(*res, what=name)
            return res
        return call
    for name in saved:
        setattr(hops, name, checked(name))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(hops, name, fn)


def run_script(script, device, tmp_path, label="script"):
    """runs the script on `device`; returns the number of launches it compared with the oracle.  The caller's module has
    the poisoned outputs installed (poison.poisoned_outputs): the interpreter refuses to run without them."""
    import torch
    import nearest_cases as NC
    import poison
    from launch_options import DEFAULTS, options
    from test_gpu_kernel_matrix import check_query, run_query
    from triro.ray.ray_optix import RayMeshIntersector
    assert poison.installed(), "handle scripts run with poisoned outputs"
    check_table(script)

    def T(x):
        return torch.from_numpy(np.array(x, order="C")).to(device)          # (a copy: the shared arrays are read-only)

    r, current, live = None, None, dict(DEFAULTS)
    streams, records, graph, launches = {}, [], None, 0
    rays = {}                                              # (mesh, batch) -> device tensors, made on the default stream
    default_stream = torch.cuda.current_stream(device)

    def tensors(batch_name):
        key = (current, batch_name)
        if key not in rays:
            with torch.cuda.stream(default_stream):
                rays[key] = tuple(T(x) for x in batch(current, batch_name))
            torch.cuda.synchronize()
        return rays[key]

    def record():
        if live["stream"] == 2:                            # a streaming launch leaves the record of an earlier direct one
            return None
        try:
            return r.as_wrapper.last_launch()
        except ValueError:
            return None

    with options(), _checked_point_queries():
        try:
            for k, step in enumerate(script):
                kind, args = step[0], step[1:]
                what = f"{label} step {k} {step if kind != 'expect' else ''} on {current}"
                if kind == "opts":
                    import triro.backend.ops as hops
                    for name, value in args[0].items():
                        hops.set_option(name, value)
                        live[name] = value
                elif kind in TRANSITIONS:
                    torch.cuda.synchronize()
                    if kind == "build":
                        v, f = mesh(args[0])
                        r, current = RayMeshIntersector(vertices=T(v), faces=T(f)), args[0]
                    elif kind == "update":
                        v, f = mesh(args[0])
                        r.update_raw(T(v), T(f))
                        current = args[0]
                    elif kind == "refit":
                        r.refit(T(mesh(args[0])[0]))
                        current = args[0]
                    elif kind == "save_load":
                        path = str(tmp_path / f"{label}_{k}.npz")
                        r.save(path)
                        r = RayMeshIntersector.load(path, device=device)
                    else:
                        v, f = mesh("bad")
                        try:
                            r.update_raw(T(v), T(f))
                        except ValueError as e:
                            assert "face 777" in str(e), e
                        else:
                            raise AssertionError(f"{what}: update_raw took a face index out of range")
                        current = "bad"
                    torch.cuda.synchronize()
                    info = r.bvh_info()
                    assert current == "hostile" or info["num_tris"] == len(answering(current)[1]), f"{what}: {info}"
                elif kind == "launch":
                    query, name, times = args
                    ot, dt = tensors(name)
                    exp = expected(current, name)
                    records = []
                    for j in range(times):
                        got = run_query(r, query, ot, dt)          # (poison checks every output for unwritten elements)
                        check_query(query, got, exp, f"{what} launch {j}")
                        records.append(record())
                        launches += 1
                elif kind == "points":
                    p, exp = T(points(current)), expected_points(current)
                    c, d, t = (x.cpu().numpy() for x in r.closest_point(p))
                    NC.assert_same_bits((c, d, t), exp["nearest"], f"{what}: closest_point")
                    inside = r.contains_points(p, T(DIRECTION)).cpu().numpy()
                    assert np.array_equal(inside, exp["contains"]), f"{what}: contains_points, {int(np.sum(inside != exp['contains']))} points differ"
                    inside2 = r.contains_points(p, None, _retry_direction=torch.from_numpy(RETRY)).cpu().numpy()
                    assert np.array_equal(inside2, exp["contains_retry"]), f"{what}: contains_points with a retry, {int(np.sum(inside2 != exp['contains_retry']))} points differ"
                    sd = r.signed_distance(p, T(DIRECTION)).cpu().numpy()
                    want = np.where(exp["contains"], exp["nearest"][1], -exp["nearest"][1]).astype(F32)
                    assert np.array_equal(NC.bits(sd), NC.bits(want)), f"{what}: signed_distance"
                    if len(answering(current)[1]) == 0:
                        assert np.isnan(c).all() and np.isposinf(d).all() and (t == -1).all() and not inside.any() and not inside2.any(), f"{what}: an empty handle"
                elif kind == "stream":
                    torch.cuda.synchronize()
                    if args[0] and args[0] not in streams:
                        streams[args[0]] = torch.cuda.Stream(device=device)
                    torch.cuda.set_stream(streams[args[0]] if args[0] else default_stream)
                    torch.cuda.synchronize()
                elif kind == "sync":
                    torch.cuda.synchronize()
                elif kind == "capture":
                    query, name = args
                    ot, dt = tensors(name)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=torch.cuda.current_stream(device)):
                        out = run_query(r, query, ot, dt)
                    graph = (g, query, name, out, current)
                    records = [record()]
                    launches += 1
                elif kind == "replay":
                    g, query, name, out, rays_of = graph
                    g.replay()
                    torch.cuda.synchronize()
                    poison.assert_written(*(out if isinstance(out, (tuple, list)) else (out,)), what=f"{what}: replay")
                    check_query(query, out, expected(current, name, rays_of), f"{what}: replay")
                    launches += 1
                elif kind == "expect":
                    _check_expect(args[0], records, r.bvh_info(), what)
            torch.cuda.synchronize()
        finally:
            torch.cuda.set_stream(default_stream)
            graph = None
    return launches
