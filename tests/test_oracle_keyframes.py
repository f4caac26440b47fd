"""The numpy restatement of the key-frame rule (tests/keyframe_oracle.py): known answers for quat2vec /
poses_diff, every branch of the state machine on hand-built sequences, and the margins the GPU scenes keep.  CPU only."""
import json
import os

import numpy as np
import pytest

import keyframe_oracle as ko
import keyframe_scene as ks

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_bounds.json")
I7 = np.array([0, 0, 0, 1, 0, 0, 0], F)


def sig(c):
    return np.diag(np.full(7, c / 7.0)).astype(F)


def pose(x, y=0.0, z=0.0):
    return np.array([x, y, z, 1, 0, 0, 0], F)


def test_quat2vec_known_answers():
    assert np.array_equal(ko.quat2vec([1, 0, 0, 0]), np.zeros(3, F))                    # identity
    assert np.array_equal(ko.quat2vec([F(1.0000001), 0.3, 0.2, 0.1]), np.zeros(3, F))     # q0 > 1: acos is NaN -> zero
    assert np.array_equal(ko.quat2vec([np.nan, 0.3, 0.2, 0.1]), np.zeros(3, F))
    h = np.deg2rad(30.0) / 2
    v = ko.quat2vec([np.cos(h), 0, np.sin(h), 0])
    assert v.dtype == F and v[0] == 0 and v[2] == 0 and abs(float(v[1]) - np.deg2rad(30.0)) < 4e-7


def test_poses_diff_known_answers():
    assert ko.poses_diff(I7, I7, np.zeros(3, F)) == 0
    assert ko.poses_diff(np.zeros(7, F), pose(1.0), np.zeros(3, F)) == F(3.33)          # 1 m of pure translation
    assert ko.poses_diff(pose(0, 0, 2.0), pose(0, 0, 1.0), np.zeros(3, F)) == F(3.33)
    h = np.deg2rad(1.0) / 2
    for axis in range(3):
        q = np.zeros(4)
        q[0], q[1 + axis] = np.cos(h), np.sin(h)
        d = ko.poses_diff(I7, np.concatenate([[0, 0, 0], q]), np.zeros(3, F))
        # 1 degree: acos near 1 amplifies the fp32 rounding of q0 (d acos / dx = 1 / sin(0.5 deg) = 115) -> 115 * 6e-8 * 2 rad
        assert d.dtype == F and abs(float(d) - 1.0) < 115 * 6e-8 * 2 * 57.3 + 1e-6, d
    # the absolute value is the floating-point one: a rotation of -0.4 degrees is 0.4, not (int) 0
    q = np.array([np.cos(-0.0035), np.sin(-0.0035), 0, 0])
    assert 0.39 < float(ko.poses_diff(I7, np.concatenate([[0, 0, 0], q]), np.zeros(3, F))) < 0.41
    assert np.isnan(ko.poses_diff(I7, pose(np.nan), np.zeros(3, F)))


def test_covariance_parameter_order():
    S = np.diag([1e8, 1.0, -1e8, 3.0, 0.5, 0.25, 0.125]).astype(F)
    assert ko.covariance_parameter(S) == F(F(F(F(1e8) + F(1)) + F(-1e8)) + F(F(F(F(0.5) + F(0.25)) + F(0.125)) + F(3)))
    assert ko.covariance_parameter(S) == F(3.875)                                      # (1e8 + 1) - 1e8 = 0 in fp32


def test_first_frames():
    sel = ko.Selector(18.0)
    assert sel.observe(1, pose(0), sig(0.5))["action"] == ko.NONE
    r = sel.observe(2, pose(6.0), sig(0.5))                                             # D = 19.98, no candidate, id < 5
    assert r["action"] == ko.EMIT_FIRST and r["id"] == 2 and np.array_equal(r["projections"], [[0, 0, 0]])
    assert np.array_equal(sel.last_pose, pose(6.0)) and sel.min_cov == F(1e7)
    r = sel.observe(4, pose(12.0), sig(0.5))
    assert r["action"] == ko.EMIT_FIRST and r["id"] == 4
    # from id 5 on a frame beyond the threshold without a candidate emits nothing and leaves last_*
    r = sel.observe(5, pose(18.0), sig(0.5))
    assert r["action"] == ko.NONE and "id" not in r and np.array_equal(sel.last_pose, pose(12.0))
    assert np.array_equal(sel.last_vrot, np.zeros(3, F)) and sel.min_cov == F(1e7)


def test_window_improving_and_not_improving():
    sel = ko.Selector(18.0)
    sel.observe(2, pose(6.0), sig(0.5))
    assert sel.observe(6, pose(8.0), sig(0.1))["action"] == ko.NONE                    # D = 6.66: below the window
    r = sel.observe(7, pose(9.0), sig(0.4), [[3, 10, 20]])                               # D = 9.99
    assert r["action"] == ko.CANDIDATE and sel.cand_id == 7 and sel.min_cov == ko.covariance_parameter(sig(0.4))
    assert sel.observe(8, pose(9.5), sig(0.45))["action"] == ko.NONE and sel.cand_id == 7      # not improving
    assert sel.observe(9, pose(10.0), sig(0.3), [[4, 11, 21]])["action"] == ko.CANDIDATE and sel.cand_id == 9
    assert np.array_equal(sel.last_pose, pose(6.0))                                     # candidates do not move last_*


@pytest.mark.parametrize("delta,action,eid", [(0.00007, ko.EMIT_CURRENT, 12), (0.0001, ko.EMIT_CANDIDATE, 9),
                                              (-0.1, ko.EMIT_CURRENT, 12)])
def test_emit_current_against_candidate(delta, action, eid):
    sel = ko.Selector(18.0)
    sel.observe(2, pose(6.0), sig(0.5))
    sel.observe(9, pose(10.0), sig(0.28), [[4, 11, 21], [5, 12, 22]])
    cmin = sel.min_cov
    S = sig(0.28)
    S[3, 3] = F(S[3, 3] + F(delta))
    diff = F(ko.covariance_parameter(S) - cmin)
    assert (diff < ko.COV_SLACK) == (action == ko.EMIT_CURRENT)
    r = sel.observe(12, pose(12.0), S, [[9, 1, 2]])
    assert r["action"] == action and r["id"] == eid
    if action == ko.EMIT_CANDIDATE:
        assert np.array_equal(r["pose"], pose(10.0)) and np.array_equal(r["projections"], [[4, 11, 21], [5, 12, 22]])
        assert np.array_equal(r["sigma"], sig(0.28))
    else:
        assert np.array_equal(r["pose"], pose(12.0)) and np.array_equal(r["projections"], [[0, 0, 0]])
    # in both cases last_* come from the CURRENT state and min_cov is reset
    assert np.array_equal(sel.last_pose, pose(12.0)) and sel.min_cov == F(1e7)


def test_keep_current_projections_changes_only_current_emits():
    a, b = ko.Selector(18.0), ko.Selector(18.0, keep_current_projections=True)
    seq = [(2, pose(6.0), sig(0.5), [[1, 5, 6]]), (9, pose(10.0), sig(0.28), [[4, 11, 21]]),
           (12, pose(12.0), sig(0.5), [[9, 1, 2]]), (13, pose(15.0), sig(0.2), [[7, 7, 7]]),
           (14, pose(18.0), sig(0.2), [[8, 8, 8]])]
    ra = [a.observe(*s) for s in seq]
    rb = [b.observe(*s) for s in seq]
    assert [r["action"] for r in ra] == [r["action"] for r in rb] == [ko.EMIT_FIRST, ko.CANDIDATE, ko.EMIT_CANDIDATE,
                                                                    ko.CANDIDATE, ko.EMIT_CURRENT]
    assert np.array_equal(ra[0]["projections"], [[0, 0, 0]]) and np.array_equal(rb[0]["projections"], [[1, 5, 6]])
    assert np.array_equal(ra[2]["projections"], rb[2]["projections"]) and np.array_equal(ra[2]["projections"], [[4, 11, 21]])
    assert np.array_equal(ra[4]["projections"], [[0, 0, 0]]) and np.array_equal(rb[4]["projections"], [[8, 8, 8]])


def test_min_cov_reset_and_nan():
    sel = ko.Selector(18.0)
    sel.observe(2, pose(6.0), sig(0.5))
    sel.observe(9, pose(10.0), sig(2.1e6))                                              # a candidate with a useless figure
    assert sel.min_cov == ko.covariance_parameter(sig(2.1e6)) and sel.min_cov >= F(1e6)
    r = sel.observe(10, pose(13.0), sig(0.5))                                           # beyond, min_cov >= 1e6, id >= 5
    assert r["action"] == ko.NONE and sel.min_cov == F(1e7) and np.array_equal(sel.last_pose, pose(6.0))
    before = sel.state()
    r = sel.observe(11, pose(np.nan), sig(0.1))
    assert r["action"] == ko.NONE and np.isnan(r["dist"])
    after = sel.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    sel.reset()
    assert sel.state()["min_cov"] == 1e7 and sel.state()["candidate_id"] == 0 and not sel.last_pose.any()


def test_scenes_reach_every_action():
    seen = set()
    for name, fn in ks.SCENES.items():
        _, res = ks.run_oracle(fn())
        seen |= {r["action"] for r in res}
    assert seen == {ko.NONE, ko.CANDIDATE, ko.EMIT_CURRENT, ko.EMIT_CANDIDATE, ko.EMIT_FIRST}
    _, res = ks.run_oracle(ks.scene_walk())
    assert {r["action"] for r in res} == seen                                           # one scene alone reaches them all


def test_scenes_keep_the_committed_margins():
    """The margin test: 100 x the largest |D_gpu - D_oracle| / |c_gpu - c_oracle| measured on the MI355X over these scenes
    (tests/golden/keyframe_bounds.json).  No frame's D lies within it of move_thresh / 2 or move_thresh, no c - min_cov
    within it of 0.000085, no c within it of the min_cov it is compared with.  Every frame of every scene is looked at."""
    b = json.load(open(GOLDEN))
    assert b["margin"]["D"] == 100 * b["measured"]["D"] and b["margin"]["c"] == 100 * b["measured"]["c"]
    assert b["bound"]["D"] == 10 * b["measured"]["D"] and b["bound"]["c"] == 10 * b["measured"]["c"]
    assert b["margin"]["D"] <= ks.BUILD_MARGIN_D and b["margin"]["c"] <= ks.BUILD_MARGIN_C
    for name, fn in ks.SCENES.items():
        frames = fn()
        sel, res = ks.run_oracle(frames)
        assert len(sel.margins) == len(frames)
        bad = ko.margin_violations(sel.margins, b["margin"]["D"], b["margin"]["c"])
        print(name, len(frames), "frames, closest calls:", bad)
        assert not bad, (name, bad)
