"""The table of tests/handle_scripts.py itself, without a GPU: a script cannot quietly lose its point.

The vocabulary and the names; the mesh properties the scripts rely on, under the host builder (tests/host_sim/sim.SimBVH, to
which the GPU builder is held equal); that every batch sees enough of its mesh and misses enough of it; that the list cap
bites on the soup; the pile of exact ties; and the safety rule: nothing that may move the arena stands between a capture and
its last replay, because such a replay would read freed memory -- it is outside the library's contract and must never run."""
import numpy as np
import pytest

import handle_scripts as S
from launch_options import DEFAULTS

WITH_HIERARCHY = ("sphere", "sphere_moved", "soup", "soup_moved", "shells", "shells_moved", "deep")


@pytest.mark.parametrize("name", list(S.SCRIPTS))
def test_script_is_well_formed(name):
    script = S.SCRIPTS[name]
    S.check_table(script)
    for step in script:
        assert step[0] in S.STEPS
        if step[0] == "opts":
            assert set(step[1]) <= set(DEFAULTS)
    assert S.count_launches(script) > 0
    assert any(s[0] == "expect" for s in script), "a script asserts the state it is about"


def test_there_are_seven_scripts_and_each_names_its_state():
    assert len(S.SCRIPTS) == 7

    def expects(name, key):
        return [s[1][key] for s in S.SCRIPTS[name] if s[0] == "expect" and key in s[1]]
    assert any(expects("pending_sort_meets_a_rebuild", "carried")) and expects("pending_sort_meets_a_rebuild", "split_some")
    assert any(expects("pending_sort_meets_option_flips", "carried"))
    assert 136 in expects("shapes_share_a_block_count", "blocks") and 128 in expects("shapes_share_a_block_count", "blocks")
    assert 2 in expects("size_classes_on_one_handle", "addressing") and 32 in expects("size_classes_on_one_handle", "depth_above")
    assert 4 in expects("wide_nodes_follow_the_handle", "shape")
    assert {s[1] for s in S.SCRIPTS["two_streams_one_handle"] if s[0] == "stream"} == {0, 1, 2}
    kinds = [s[0] for s in S.SCRIPTS["graph_replay_after_the_slot_was_rewritten"]]
    assert kinds.count("capture") == 1 and kinds.count("replay") == 4 and "refit" in kinds


@pytest.mark.parametrize("bad", ["update", "save_load", "fail_update", "build"])
def test_the_safety_rule_refuses_a_transition_under_a_capture(bad):
    step = {"update": ("update", "soup"), "save_load": ("save_load",), "fail_update": ("fail_update",), "build": ("build", "sphere")}[bad]
    script = [("build", "sphere"), ("stream", 1), ("capture", "closest", "img128"), step, ("replay",), ("stream", 0)]
    with pytest.raises(AssertionError, match="between a capture and its last replay"):
        S.check_table(script)
    S.check_table([("build", "sphere"), ("stream", 1), ("capture", "closest", "img128"), ("refit", "sphere_moved"), ("replay",), step, ("stream", 0)])


def test_the_table_refuses_what_is_outside_the_vocabulary():
    for script in ([("build", "sphere"), ("launch", "closest", "img512", 1)], [("build", "sphere"), ("opts", {"no_such_option": 1})],
                   [("build", "sphere"), ("refit", "soup")], [("build", "sphere"), ("rebuild",)], [("launch", "any", "flat", 1)],
                   [("build", "sphere"), ("replay",)], [("build", "sphere"), ("capture", "closest", "img128"), ("replay",)],
                   [("build", "sphere"), ("stream", 1), ("capture", "location", "img128"), ("replay",), ("stream", 0)],
                   [("build", "sphere"), ("stream", 1), ("launch", "any", "flat", 1)]):
        with pytest.raises(AssertionError):
            S.check_table(script)


@pytest.fixture(scope="module")
def built():
    from sim import SimBVH
    return {name: SimBVH(*S.mesh(name)) for name in WITH_HIERARCHY + ("hostile",)}


def test_mesh_properties_under_the_host_builder(built):
    for name, B in built.items():
        if name == "deep":
            assert B.depth > 32 and B.key_mode == 1, (name, B.depth, B.key_mode)
        else:
            assert B.depth <= 32 and B.key_mode == 0, (name, B.depth, B.key_mode)
    n = {name: len(S.mesh(name)[1]) for name in S.MESHES}
    assert n["soup"] > n["sphere"] > n["shells"] > n["deep"] > n["hostile"] > n["two"] > n["one"] > n["none"] == 0
    assert n["sphere"] == 20480 and n["shells"] == 5120 and n["deep"] == 4344 and n["bad"] == n["sphere"]
    for a, b in S.SAME_FACES.items():
        assert np.array_equal(S.mesh(a)[1], S.mesh(b)[1]) and S.mesh(a)[0].shape == S.mesh(b)[0].shape
        assert not np.allclose(S.box(a)[0], S.box(b)[0]) and not np.allclose(S.box(a)[1] - S.box(a)[0], S.box(b)[1] - S.box(b)[0])
    v, f = S.mesh("bad")
    assert int((f >= len(v)).sum()) == 1 and f[777, 1] >= len(v)
    v, f = S.mesh("hostile")
    assert np.isnan(v).any() and np.isinf(v).any()


@pytest.mark.parametrize("name", WITH_HIERARCHY)
def test_every_batch_sees_its_mesh_and_misses_it(name):
    for b in S.BATCHES:
        o, d = S.batch(name, b)
        assert o.shape == d.shape and o.reshape(-1, 3).shape[0] == (136 * 128 if b == "img136" else 16384)
        frac = float(np.mean(S.expected(name, b)["count"] > 0))
        print(f"{name} / {b}: hit fraction {frac:.3f}")
        assert 0.04 <= frac <= 0.96, (name, b, frac)


def test_replayed_rays_see_the_refitted_mesh():
    """script 7 replays rays made for `sphere` on `sphere_moved`"""
    frac = float(np.mean(S.expected("sphere_moved", "img128", "sphere")["count"] > 0))
    assert 0.04 <= frac <= 0.96, frac
    assert not np.array_equal(S.expected("sphere_moved", "img128", "sphere")["closest"][2], S.expected("sphere", "img128")["closest"][2])


def test_the_list_cap_bites_on_the_soup_and_the_pile_ray_counts_its_ties():
    for b in ("img128", "flat"):
        cnt = S.expected("soup", b)["count"]
        print(f"soup / {b}: up to {int(cnt.max())} hits, {float(np.mean(cnt > 8)):.3f} of the rays above 8")
        assert (cnt > 8).any(), b
    cnt = S.expected("deep", "flat")["count"]
    assert (cnt[:64] >= 3000).all() and (cnt[:64] == cnt[0]).all(), cnt[:4]


def test_points_fall_on_both_sides_and_an_empty_handle_answers_nothing():
    for name in ("sphere", "shells", "deep"):
        inside = S.expected_points(name)["contains_retry"]
        assert inside.any() and not inside.all(), name
    for name in ("none", "bad"):
        e = S.expected_points(name)
        c, d, t = e["nearest"]
        assert np.isnan(c).all() and np.isposinf(d).all() and (t == -1).all() and not e["contains"].any() and not e["contains_retry"].any()
        for b in ("img128", "flat"):
            assert not S.expected(name, b)["count"].any() and (S.expected(name, b)["closest"][2] == -1).all()
