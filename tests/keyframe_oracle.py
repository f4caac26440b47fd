"""numpy restatement of the key-frame rule: quat2vec / poses_diff of mono-slam monoslam_ransac.cpp:40-60
and the per-frame selection of :585-687.  Everything is fp32, one rounding per operation and no fused multiply-add, in the
order §12 pins; only acos / sin / sqrt are library calls (numpy's float32 ones).  Test-only: the checker of
csrc/ekf_keyframe.hpp, as tests/sba_oracle.py is for the bundle adjuster."""
import numpy as np

F = np.float32
NONE, CANDIDATE, EMIT_CURRENT, EMIT_CANDIDATE, EMIT_FIRST = 0, 1, 2, 3, 4
ACTION_NAMES = {NONE: "NONE", CANDIDATE: "CANDIDATE", EMIT_CURRENT: "EMIT_CURRENT", EMIT_CANDIDATE: "EMIT_CANDIDATE",
                EMIT_FIRST: "EMIT_FIRST"}
MIN_COV_INIT, MIN_COV_VALID, COV_SLACK = F(1e7), F(1e6), F(0.000085)
METRE, DEGREE = F(3.33), F(57.29577951308232)
NO_PROJECTION = np.zeros((1, 3), np.int64)


def quat2vec(q):
    """n = 2 acos(q0); n > 0.0001: q[1:4] * (n / sin(n / 2)); otherwise (a NaN n too) zero."""
    q = np.asarray(q, F)
    with np.errstate(invalid="ignore"):
        n = F(np.arccos(q[0]) * F(2))
    if n > F(0.0001):
        n1 = F(n / np.sin(F(n / F(2))))
        return np.array([F(q[1] * n1), F(q[2] * n1), F(q[3] * n1)], F)
    return np.zeros(3, F)


def poses_diff(old7, new7, last_rot):
    """D = |old.xyz - new.xyz| * 3.33 + sum |(last_rot - quat2vec(new.q)) * 57.29578|, floating-point absolute values."""
    old7, new7, last_rot = np.asarray(old7, F), np.asarray(new7, F), np.asarray(last_rot, F)
    d = [F(old7[k] - new7[k]) for k in range(3)]
    a = F(np.sqrt(F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))) * METRE)
    v = quat2vec(new7[3:7])
    b = [F(F(last_rot[k] - v[k]) * DEGREE) for k in range(3)]
    return F(F(F(a + np.abs(b[0])) + np.abs(b[1])) + np.abs(b[2]))


def covariance_parameter(sigma):
    """Covariance_Parameter (vslamRansac.cpp:854-855) in fp32: (S00 + S11 + S22) + (S44 + S55 + S66 + S33)."""
    d = np.diagonal(np.asarray(sigma)[:7, :7]).astype(F)
    return F(F(F(d[0] + d[1]) + d[2]) + F(F(F(d[4] + d[5]) + d[6]) + d[3]))


class Selector:
    """The state machine.  observe() returns a dict: action, dist, cov, and on an emit id / pose / sigma / projections."""

    def __init__(self, move_thresh=18.0, keep_current_projections=False):
        self.move_thresh = F(move_thresh)
        self.keep_current = bool(keep_current_projections)
        self.reset()

    def reset(self):
        self.last_pose = np.zeros(7, F)
        self.last_vrot = np.zeros(3, F)
        self.min_cov = MIN_COV_INIT
        self.cand_id = 0
        self.cand_pose = np.zeros(7, F)
        self.cand_sigma = np.zeros((7, 7), F)
        self.cand_prj = NO_PROJECTION
        self.cand_image = None
        self.margins = []          # per frame: what the decision compared, for the margin test

    def observe(self, frame_id, state, sigma, projections=None, image=None):
        s = np.asarray(state)[:7].astype(F)
        S = np.asarray(sigma)[:7, :7].astype(F)
        prj = NO_PROJECTION if projections is None else np.asarray(projections, np.int64).reshape(-1, 3)
        c = covariance_parameter(S)
        D = poses_diff(self.last_pose, s, self.last_vrot)
        T, H = self.move_thresh, F(self.move_thresh * F(0.5))
        m = {"frame": int(frame_id), "D": float(D), "c": float(c), "half": float(H), "full": float(T),
             "min_cov": None, "slack": None}
        out = {"action": NONE, "dist": D, "cov": c}
        emit = None
        if D > H and D < T:
            m["min_cov"] = float(self.min_cov)
            if c < self.min_cov:
                self.min_cov, self.cand_id, self.cand_pose, self.cand_sigma = c, int(frame_id), s, S
                self.cand_prj, self.cand_image = prj, image
                out.update(action=CANDIDATE, id=int(frame_id), pose=s, sigma=S)
        elif D >= T:
            current = (int(frame_id), s, S, prj if self.keep_current else NO_PROJECTION, image)
            if self.min_cov < MIN_COV_VALID:
                diff = F(c - self.min_cov)
                m["slack"] = float(diff)
                if diff < COV_SLACK:
                    out["action"], emit = EMIT_CURRENT, current
                else:
                    out["action"] = EMIT_CANDIDATE
                    emit = (self.cand_id, self.cand_pose, self.cand_sigma, self.cand_prj, self.cand_image)
            elif frame_id < 5:
                out["action"], emit = EMIT_FIRST, current
            if emit is not None:
                self.last_pose, self.last_vrot = s, quat2vec(s[3:7])
            self.min_cov = MIN_COV_INIT
        if emit is not None:
            out.update(id=emit[0], pose=emit[1], sigma=emit[2], projections=emit[3], image=emit[4])
        self.margins.append(m)
        return out

    def state(self):
        return {"last_pose": self.last_pose.copy(), "last_vrot": self.last_vrot.copy(), "min_cov": float(self.min_cov),
                "candidate_id": self.cand_id}


def margin_violations(margins, margin_d, margin_c):
    """Frames whose decision sits within a margin of a threshold: D against move_thresh / 2 and move_thresh, c - min_cov
    against 0.000085, c against the min_cov it was compared with.  Every frame is looked at."""
    bad = []
    for m in margins:
        if np.isnan(m["D"]):
            # a NaN D fails every comparison on either side: no c was compared with anything, there is no margin to keep
            assert m["slack"] is None and m["min_cov"] is None, m
        if abs(m["D"] - m["half"]) <= margin_d or abs(m["D"] - m["full"]) <= margin_d:
            bad.append((m["frame"], "D", m["D"]))
        if m["slack"] is not None and abs(m["slack"] - float(COV_SLACK)) <= margin_c:
            bad.append((m["frame"], "slack", m["slack"]))
        if m["min_cov"] is not None and abs(m["c"] - m["min_cov"]) <= margin_c:
            bad.append((m["frame"], "min_cov", m["c"]))
    return bad
