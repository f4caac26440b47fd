"""Scripted pose / covariance streams for the key-frame selector.  A frame is (id, pose7, diagonal of
Sigma[0:7,0:7], feature centres); every value is exactly representable in float32, so an fp32 and an fp64 filter are given
the same numbers.  The device's acos / sin need not round as numpy's do, so the builder keeps every decision away from its
threshold by BUILD_MARGIN_D / BUILD_MARGIN_C, judged by the oracle alone: a random frame that comes too close is drawn
again, a hand-built one is an error.  tests/test_oracle_keyframes.py asserts the (much smaller) committed margins of
tests/golden/keyframe_bounds.json on every frame of every scene."""
import numpy as np

import keyframe_oracle as ko

F = np.float32
MOVE_THRESH = 18.0
BUILD_MARGIN_D = 1e-2          # in units of D (degrees / 3.33 m)
BUILD_MARGIN_C = 1e-5          # in units of the covariance figure
N_FEATURES = 6


def _quat(axis, deg):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    h = np.deg2rad(deg) / 2.0
    return np.concatenate([[np.cos(h)], np.sin(h) * axis]).astype(F)


def _frame(fid, xyz, quat, c, k):
    pose = np.concatenate([np.asarray(xyz, F), np.asarray(quat, F)]).astype(F)
    # c spread over the diagonal with unequal weights; off-diagonals small and NOT symmetric (the upper triangle is twice the
    # lower one; only the setters and the selector see this block, no update does), to tell rows from columns
    w = np.array([0.10, 0.12, 0.14, 0.16, 0.18, 0.14, 0.16], np.float64)
    sig = np.zeros((7, 7), F)
    sig[np.arange(7), np.arange(7)] = (w * c).astype(F)
    for r in range(7):
        for cc in range(r):
            sig[r, cc] = F(1e-3 * c * (r + 2 * cc + 1) / 20.0)
            sig[cc, r] = F(2.0) * sig[r, cc]
    centers = np.array([[40.0 + 30.0 * i + k, 50.0 + 20.0 * i + 2 * (k % 7)] for i in range(N_FEATURES)], F)
    inn = np.array([(i + k) % 3 != 0 for i in range(N_FEATURES)])
    return {"id": int(fid), "pose": pose, "sigma": sig, "centers": centers, "in_innovation": inn}


def _x(d):
    """Translation along x that contributes d to D."""
    return d / 3.33


def scene_walk():
    """Hand-built: every action and every branch, ids from 1."""
    I = _quat([0, 0, 1], 0.0)
    f = []
    f.append(_frame(1, [0, 0, 0], I, 0.9, 0))                       # D = 0: nothing
    f.append(_frame(2, [_x(20), 0, 0], I, 0.8, 1))                  # D >= T, no candidate, id < 5: EMIT_FIRST
    f.append(_frame(3, [_x(25), 0, 0], I, 0.7, 2))                  # D = 5: nothing
    f.append(_frame(4, [_x(30), 0, 0], I, 0.5, 3))                  # D = 10: CANDIDATE
    f.append(_frame(5, [_x(32), 0, 0], I, 0.7, 4))                  # window, not improving: nothing
    f.append(_frame(6, [_x(34), 0, 0], I, 0.3, 5))                  # window, improving: CANDIDATE
    f.append(_frame(7, [_x(39), 0, 0], I, 0.301, 6))                # D = 19, c - min = 1e-3: EMIT_CANDIDATE (6)
    f.append(_frame(8, [_x(39), _x(11), 0], I, 0.4, 7))             # D = 11: CANDIDATE
    f.append(_frame(9, [_x(39), _x(20), 0], I, 0.40001, 8))         # D = 20, c - min = 1e-5: EMIT_CURRENT
    f.append(_frame(10, [_x(39), _x(45), 0], I, 0.6, 9))            # D = 25, no candidate, id >= 5: nothing, last_* stay
    f.append(_frame(11, [_x(39), _x(33), 0], I, 0.2, 10))           # D = 13 (still from frame 9): CANDIDATE
    f.append(_frame(12, [_x(39), _x(33), 0], _quat([0, 0, 1], 21.0), 0.1, 11))   # D = 13 + 21, c below min: EMIT_CURRENT
    bad = _frame(13, [np.nan, _x(33), 0], _quat([0, 0, 1], 21.0), 0.3, 12)       # NaN D: nothing
    f.append(bad)
    f.append(_frame(14, [_x(39), _x(33), _x(4)], _quat([0, 0, 1], 28.0), 0.6, 13))   # D = 4 + 7: CANDIDATE
    f.append(_frame(15, [_x(39), _x(33), _x(4)], _quat([1, 1, 0], 40.0), 0.9, 14))   # far: EMIT_CANDIDATE (14)
    f.append(_frame(16, [_x(39), _x(33), _x(4)], np.array([1.0000001, 0, 0, 0], F), 0.9, 15))   # q0 > 1: vrot = 0
    return f


def scene_first():
    """The first frames: EMIT_FIRST at ids 2 and 4 (no candidate), nothing from id 5 on without one."""
    I = _quat([1, 0, 0], 0.0)
    return [_frame(1, [0, 0, 0], I, 0.5, 0), _frame(2, [0, 0, 7.0], I, 0.5, 1), _frame(3, [0, 0, 8.0], I, 0.5, 2),
            _frame(4, [0, 0, 14.0], I, 0.5, 3), _frame(5, [0, 0, 21.0], I, 0.5, 4), _frame(6, [0, 0, 28.0], I, 0.5, 5),
            _frame(7, [0, 0, 24.0], I, 0.4, 6), _frame(8, [0, 0, 21.0], I, 0.45, 7)]


def scene_random(seed=7, frames=120, move_thresh=MOVE_THRESH):
    """A seeded random walk with rotations about drifting axes and a covariance figure that falls and jumps; a frame whose
    decision comes within the build margins of a threshold is drawn again."""
    rng = np.random.default_rng(seed)
    sel = ko.Selector(move_thresh)
    out = []
    xyz, axis, deg, c = np.zeros(3), np.array([0.2, 1.0, 0.1]), 0.0, 0.5
    for k in range(frames):
        fid = k + 1
        for attempt in range(100):
            step = rng.normal(size=3) * 0.9
            nd = deg + rng.uniform(-1.0, 4.0)
            na = axis + rng.normal(size=3) * 0.02
            nc = max(c * rng.uniform(0.8, 1.0), 1e-3) if rng.uniform() > 0.15 else c + rng.uniform(0.0, 0.4)
            if rng.uniform() < 0.1:
                nc = c + rng.uniform(-2e-4, 2e-4)                   # figures on either side of the 0.000085 slack
            fr = _frame(fid, xyz + step, _quat(na, nd), max(nc, 1e-3), k)
            D = float(ko.poses_diff(sel.last_pose, fr["pose"], sel.last_vrot))
            cc = float(ko.covariance_parameter(fr["sigma"]))
            T = float(sel.move_thresh)
            near = min(abs(D - T), abs(D - T / 2)) <= BUILD_MARGIN_D
            near |= abs(cc - float(sel.min_cov)) <= BUILD_MARGIN_C
            near |= abs(float(F(F(cc) - sel.min_cov)) - float(ko.COV_SLACK)) <= BUILD_MARGIN_C
            if not near:
                break
        else:
            raise AssertionError("no safe frame after 100 draws")
        sel.observe(fid, fr["pose"], fr["sigma"])
        xyz, axis, deg, c = xyz + step, na, nd, max(nc, 1e-3)
        out.append(fr)
    return out


SCENES = {"walk": scene_walk, "first": scene_first, "random": scene_random}


def run_oracle(frames, move_thresh=MOVE_THRESH, keep_current_projections=False, projections=None):
    """The oracle over a scene: (selector, list of per-frame results).  `projections`: per-frame rows, or None."""
    sel = ko.Selector(move_thresh, keep_current_projections)
    res = []
    for k, fr in enumerate(frames):
        res.append(sel.observe(fr["id"], fr["pose"], fr["sigma"], None if projections is None else projections[k]))
    return sel, res
