"""Directed scenes for the device patch matcher and the template blur, shared by
tests/test_oracle_matcher_edges.py (CPU: the conditions below hold for the oracle alone), tools/image_host_check.py (the
kernel bodies on the host under the sanitizers) and tests/test_gpu_matcher_edges.py (the device through VSlamFilter).

A scene is a configuration, the pixels features are added at with the camera at rest, a change to mu / Sigma after the
adds, the frame the templates are cut from and the frame that is searched.  A feature added at (u, v) with the camera
unmoved predicts at (u, v) after measure(), so the add pixels steer the search region; a constant factor on Sigma steers
the size of the search box (x 1: du = dv = 5.7, x 25: 20.4, clamped to 20) and k v v^T added to the quaternion block of
Sigma makes the 2 x 2 innovation block oblique.  Pure numpy plus the oracle; nothing here is random at run time: the seeds
were chosen when this was written so that every condition tests/test_oracle_matcher_edges.py asserts holds for the oracle
alone, and no case skips or reseeds itself.

How two of the conditions are read.  "Every feature's region extends outside the frame" holds for the features on the add
margin (the first N_BORDER of border_pixels()); the two interior features of the same scenes cannot overhang and are there
for contrast (in `small` every feature overhangs, on all four sides).  "At least half of the admissible candidates are
rejected by the ellipse" is counted over the scene, all features together (67 % in oblique_swap, 54 % in oblique_noswap): a
feature in a frame corner has a quarter of its box admissible, and that quarter may lie along the ellipse's long axis; every
feature still accepts at least one candidate.  The oblique scenes EXERCISE the row-swap branch of the 2 x 2 LU inverse (six of
eight features take it in oblique_swap, none in oblique_noswap); they do not tell it from the branch without the swap, since
pivoting a well-conditioned 2 x 2 moves the inverse in its last place only and no candidate lies that close to the ellipse.
A wrong permutation, or swapping always, is caught.
"""
import dataclasses
import math

import numpy as np

import ekf_oracle as o
import image_oracle as io_

F = np.float32
FLAT = 100                                  # grey value of flat templates, frames and occluders


@dataclasses.dataclass
class Scene:
    name: str
    cfg: o.Config
    pixels: list
    template_frame: np.ndarray
    search_frame: np.ndarray
    sigma_scale: float = 1.0
    oblique: tuple = None                   # (k, v): Sigma[3:7, 3:7] += k v v^T
    flat_templates: tuple = ()              # features whose template is replaced by a flat one (setPatch)
    omega: tuple = (0.0, 0.0, 0.0)          # angular velocity of a blur scene, camera frame (z = optical axis)
    dT: float = 1.0 / 30.0
    blur: bool = False                      # predict() with the blur instead of measure()

    @property
    def shape(self):
        return self.cfg.image_height, self.cfg.image_width


def config(window=15, **kw):
    return dataclasses.replace(o.Config.kinect(), window_size=window, **kw)


def border_pixels(cfg):
    """The four corners of the add margin, two edge mid-points and two interior pixels."""
    W, H, hw = cfg.image_width, cfg.image_height, cfg.window_size // 2
    return [(hw + 1.5, hw + 1.5), (W - hw - 1.5, hw + 1.5), (hw + 1.5, H - hw - 1.5), (W - hw - 1.5, H - hw - 1.5),
            (W / 2, hw + 1.25), (hw + 1.25, H / 2), (0.4 * W + 0.3, 0.45 * H + 0.6), (0.7 * W + 0.2, 0.6 * H + 0.4)]


N_BORDER = 6                                # of border_pixels(): the first six lie on the margin


def shifted(frame, du, dv):
    """The scene moved by (du, dv) pixels."""
    return np.roll(np.roll(frame, du, axis=1), dv, axis=0)


def pushed(frame, d):
    """Every quadrant of the frame moved d pixels away from the centre: what stood on the add margin now lies beyond it."""
    H, W = frame.shape
    out = np.empty_like(frame)
    for sy, ys in ((-d, slice(0, H // 2)), (d, slice(H // 2, H))):
        for sx, xs in ((-d, slice(0, W // 2)), (d, slice(W // 2, W))):
            out[ys, xs] = shifted(frame, sx, sy)[ys, xs]
    return out


def tiled(height, width, seed, period_u=10, period_v=6):
    """A random period_v x period_u tile repeated over the frame: every window recurs at that period."""
    tile = np.random.default_rng(seed).integers(0, 256, size=(period_v, period_u)).astype(np.uint8)
    return np.tile(tile, (height // period_v + 1, width // period_u + 1))[:height, :width].copy()


# ---- the oracle's filter, predictions and templates of a scene -----------------------------------------------------------
def oracle_filter(sc, dtype):
    """The oracle filter after the adds and the scene's change to mu / Sigma (before measure / predict)."""
    ref = o.DenseFilter(sc.cfg, dtype)
    T = ref.T
    ref.dT = sc.dT
    for (u, v) in sc.pixels:
        assert ref.add_feature(u, v) == 1
    ref.Sigma = ref.Sigma * T(sc.sigma_scale)
    if sc.oblique is not None:
        k, v = sc.oblique
        v = np.asarray(v, T)
        ref.Sigma[3:7, 3:7] += T(k) * np.outer(v, v)
    if sc.blur:
        # the camera turns back by omega dT first, so that predict() brings every feature to the pixel it was added at
        omega = np.asarray(sc.omega, T)
        ref.mu[3:7] = o.quat_product(ref.mu[3:7], o.vec2quat(-T(sc.dT) * omega, T), T)
        ref.mu[10:13] = omega
    return ref


def oracle_predictions(sc, dtype):
    """(ref, h (N, 2), S (N, 2, 2), visible (N,), hb (N, 2) or None): what the matcher and the blur consume."""
    ref = oracle_filter(sc, dtype)
    if sc.blur:
        ref.predict()
    else:
        ref.measure()
    vis = ref.visible_indices()
    St = ref.innovation_covariance(vis)
    N = len(ref.features)
    h = np.stack([ft.h for ft in ref.features]).astype(ref.T)
    S = np.zeros((N, 2, 2), ref.T)
    for k, i in enumerate(vis):
        S[i] = St[2 * k:2 * k + 2, 2 * k:2 * k + 2]
    visible = np.array([ft.is_in_innovation for ft in ref.features])
    hb = np.stack([io_.blur_point(ref, ft) for ft in ref.features]).astype(ref.T) if sc.blur else None
    return ref, h, S, visible, hb


def templates(sc):
    w = sc.cfg.window_size
    tpl = [io_.capture_patch(sc.template_frame, u, v, w) for (u, v) in sc.pixels]
    for i in sc.flat_templates:
        tpl[i] = np.full((w, w), FLAT, np.uint8)
    return tpl


# ---- what the search does, candidate by candidate (Patch.cpp:215-293 as image_oracle.find_match walks it) -------------
@dataclasses.dataclass
class Scan:
    i0: int
    j0: int
    ni: int
    nj: int
    swap: bool
    admissible: np.ndarray                  # (ni * nj,) scan order, u outer, v inner: inside the frame gate
    inside: np.ndarray                      # admissible and inside the ellipse
    score: np.ndarray                       # float32, NaN where not scored or 0 / 0

    def best(self):
        """Scan index of the first maximum, or -1."""
        s = np.where(np.isnan(self.score), -np.inf, self.score)
        return int(np.argmax(s)) if np.any(s > -1) else -1


def scan(frame, tpl, h, S, sigma_size, scores=True):
    frame = np.asarray(frame, np.uint8)
    fh, fw = frame.shape
    w = tpl.shape[1]
    hw = w // 2
    uc, vc = int(F(h[0])), int(F(h[1]))
    S = np.asarray(S, F)
    inv = io_.lu_inverse_2x2(S)
    x2, y2, yx = inv[0, 0], inv[1, 1], F(F(2) * inv[1, 0])
    sig = F(sigma_size)
    s2 = F(sig * sig)
    du = min(F(np.float64(sig) * np.sqrt(np.float64(S[0, 0]))), F(20))
    dv = min(F(np.float64(sig) * np.sqrt(np.float64(S[1, 1]))), F(20))
    i0, i1 = int(F(F(uc) - du)), int(math.floor(F(F(uc) + du)))
    j0, j1 = int(F(F(vc) - dv)), int(math.floor(F(F(vc) + dv)))
    ni, nj = i1 - i0 + 1, j1 - j0 + 1
    adm = np.zeros(ni * nj, bool)
    ins = np.zeros(ni * nj, bool)
    val = np.full(ni * nj, np.nan, F)
    for c in range(ni * nj):
        i, j = i0 + c // nj, j0 + c % nj
        adm[c] = i > hw and j > hw and i < fw - hw and j < fh - hw
        if not adm[c]:
            continue
        fi, fj = F(i - uc), F(j - vc)
        g = F(F(F(F(x2 * fi) * fi) + F(F(y2 * fj) * fj)) + F(F(yx * fi) * fj))
        ins[c] = g <= s2
        if ins[c] and scores:
            val[c] = io_.compute_correlation(tpl, frame[j - hw:j - hw + w, i - hw:i - hw + w])
    return Scan(i0, j0, ni, nj, bool(abs(S[1, 0]) > abs(S[0, 0])), adm, ins, val)


def expected(sc, tpl, h, S, visible, threshold=io_.PATCH_MATCHING_THRESHOLD):
    """found (N,), z (N, 2) int, score (N,) float32, matching templates after the search: image_oracle.find_match."""
    N = len(tpl)
    found = np.zeros(N, bool)
    z = -np.ones((N, 2), np.int64)
    score = -np.ones(N, F)
    after = [t.copy() for t in tpl]
    for i in range(N):
        if not visible[i]:
            continue
        ok, zz, s, win = io_.find_match(sc.search_frame, tpl[i], h[i], S[i], sc.cfg.sigma_size, threshold)
        found[i], z[i], score[i] = ok, zz, s
        if ok:
            after[i] = win
    return found, z, score, after


# ---- the scenes ----------------------------------------------------------------------------------------------------------
def _kinect_scene(name, window=15, seed=0, move=(2, -1), **kw):
    cfg = config(window)
    frame = io_.random_texture(cfg.image_height, cfg.image_width, seed=seed)
    return Scene(name, cfg, border_pixels(cfg), frame, shifted(frame, *move), **kw)


OBLIQUE_SWAP = (0.002, (0.0, 0.6, 0.8, 0.0))
OBLIQUE_NOSWAP = (0.004, (0.0, 1.0, 0.0, 0.0))
SEARCH_WINDOWS = (15, 32, 9, 5, 4)          # on the device and in the host check
HOST_ONLY_WINDOWS = (1, 2, 3)               # window 1: every score is 0 / 0 and nothing is ever found


def _occluded(sc, feature, dtype=np.float32):
    """sc with a flat occluder over every window the search of `feature` scores, and over nothing else: part of its
    region only (the ellipse is thin)."""
    _, h, S, _, _ = oracle_predictions(sc, dtype)
    w = sc.cfg.window_size
    hw = w // 2
    s = scan(sc.search_frame, templates(sc)[feature], h[feature], S[feature], sc.cfg.sigma_size, scores=False)
    frame = sc.search_frame.copy()
    for c in np.flatnonzero(s.inside):
        i, j = s.i0 + c // s.nj, s.j0 + c % s.nj
        frame[j - hw:j - hw + w, i - hw:i - hw + w] = FLAT
    return dataclasses.replace(sc, search_frame=frame)


def _small():
    cfg = config(15, image_width=48, image_height=40, u0=24.3, v0=19.6)
    frame = io_.random_texture(40, 48, seed=77)
    # (every predicted pixel close enough to the centre for the 56-pixel region to overhang left and right, top and bottom)
    px = [(25.5, 21.25), (20.25, 25.5), (20.5, 12.75), (26.25, 14.5), (22.75, 18.5)]
    return Scene("small", cfg, px, frame, shifted(frame, 3, -2), sigma_scale=25.0)


def _ties(name, period_u, period_v=6):
    """The maximum 1.0 recurs at the tile's period (u, v).  10 x 6: many equal maxima in different lanes and passes.  9 x 6:
    the first in scan order sits in a higher lane than a later one, so lane order would pick another.  6 x 10: with 41
    rows a box column, one period in u and one in v is 6 * 41 + 10 = 256 candidates, so the first maximum and a later one
    are visited by the SAME lane, where the strict `val > best` keeps the first."""
    cfg = config(15)
    frame = tiled(cfg.image_height, cfg.image_width, seed=5, period_u=period_u, period_v=period_v)
    return Scene(name, cfg, border_pixels(cfg), frame, frame, sigma_scale=25.0)


def _build_search_scenes():
    s = {}
    s["border"] = _kinect_scene("border", seed=101)
    b = s["border"]
    s["border_pushed"] = dataclasses.replace(b, name="border_pushed", search_frame=pushed(b.template_frame, 3))
    s["clamped"] = _kinect_scene("clamped", seed=102, move=(9, -7), sigma_scale=25.0)
    for w in SEARCH_WINDOWS[1:]:
        s["window_%d" % w] = _kinect_scene("window_%d" % w, window=w, seed=110 + w, move=(-5, 6), sigma_scale=25.0)
    s["oblique_swap"] = _kinect_scene("oblique_swap", seed=103, move=(1, 2), oblique=OBLIQUE_SWAP)
    ob = s["oblique_swap"]
    s["oblique_outside"] = dataclasses.replace(ob, name="oblique_outside", search_frame=shifted(ob.template_frame, 5, -6))
    s["oblique_noswap"] = _kinect_scene("oblique_noswap", seed=104, move=(-2, 1), oblique=OBLIQUE_NOSWAP)
    s["small"] = _small()
    s["ties"] = _ties("ties", 10)
    s["ties_lanes"] = _ties("ties_lanes", 9)
    s["ties_same_lane"] = _ties("ties_same_lane", 6, 10)
    s["flat_template"] = dataclasses.replace(b, name="flat_template", flat_templates=(0, 4, 6))
    s["flat_frame"] = dataclasses.replace(b, name="flat_frame", search_frame=np.full_like(b.search_frame, FLAT))
    s["flat_occluder"] = dataclasses.replace(_occluded(ob, OCCLUDED_FEATURE), name="flat_occluder")
    assert tuple(s) == SEARCH_SCENES
    return s


OCCLUDED_FEATURE = 6                        # of oblique_swap: an interior feature
NON_PERIODIC = ("border", "border_pushed", "clamped", "window_32", "window_9", "window_5", "window_4", "oblique_swap",
                "oblique_outside", "oblique_noswap", "small")
TIE_SCENES = ("ties", "ties_lanes", "ties_same_lane")
DEGENERATE = {"flat_template": (0, 4, 6), "flat_frame": tuple(range(8)), "flat_occluder": (OCCLUDED_FEATURE,)}
SEARCH_SCENES = NON_PERIODIC + TIE_SCENES + tuple(DEGENERATE)          # every search scene, in the order they are built
BORDER_SCENES = ("border", "border_pushed", "clamped", "window_32", "window_9", "window_5", "window_4", "small")
CLAMPED_SCENES = ("clamped", "window_32", "window_9", "window_5", "window_4", "small") + TIE_SCENES
OBLIQUE_SCENES = ("oblique_swap", "oblique_outside", "oblique_noswap")
BOTH_TYPES = ("border", "border_pushed", "clamped", "window_32", "oblique_swap", "oblique_outside", "oblique_noswap")


def _blur_pixels(cfg):
    W, H = cfg.image_width, cfg.image_height
    px = [(cfg.u0 + r * math.cos(a), cfg.v0 + r * math.sin(a))
          for r, n, a0 in ((95.0, 8, 0.2), (50.0, 4, 0.9)) for a in (a0 + 2 * math.pi * k / n for k in range(n))]
    return px + [(cfg.u0 + 0.3, cfg.v0 - 0.2), (cfg.u0 + 60.0, cfg.v0 + 0.1), (cfg.u0 - 0.2, cfg.v0 + 70.0), (W - 30.5, 40.25)]


# name -> (angular velocity, window): roll about the optical axis (tangential displacement: every direction occurs), pure
# yaw and pitch (one-row and one-column kernels near the principal point's row and column), lines longer than twice the
# window, and a motion below kernel_size (a plain copy)
BLUR_MOTIONS = {"blur_roll_pos": ((0.0, 0.0, 4.0), 15), "blur_roll_neg": ((0.0, 0.0, -4.0), 15),
                "blur_yaw_pos": ((0.0, 1.5, 0.0), 15), "blur_yaw_neg": ((0.0, -1.5, 0.0), 15),
                "blur_pitch_pos": ((1.5, 0.0, 0.0), 15), "blur_pitch_neg": ((-1.5, 0.0, 0.0), 15),
                "blur_long": ((1.0, 5.0, 2.0), 9), "blur_copy": ((0.05, 0.1, 0.1), 15)}
# |h - hb| >= 1024: the device keeps the sharp template (kMaxTaps), the oracle would build the kernel
BLUR_FALLBACK = {"blur_fallback": ((0.0, 82.0, 0.0), 9)}


def _build_blur_scenes(fallback=False):
    s = {}
    for name, (omega, window) in (BLUR_FALLBACK if fallback else BLUR_MOTIONS).items():
        cfg = config(window, kernel_size=2, T_camera=0.5)
        frame = io_.random_texture(cfg.image_height, cfg.image_width, seed=120 + window)
        s[name] = Scene(name, cfg, _blur_pixels(cfg), frame, frame, omega=omega, blur=True)
    return s


def blur_line(h, hb):
    """(dx, dy, kernel rows, kernel columns, length, octant) of the blur line of evaluateKernel (libblur.cpp:17-52)."""
    dx, dy = F(F(h[0]) - F(hb[0])), F(F(h[1]) - F(hb[1]))
    rows, cols = int(F(abs(dy)) + F(1)), int(F(abs(dx)) + F(1))
    length = math.sqrt(float(dx) * float(dx) + float(dy) * float(dy))
    octant = 4 * int(dx < 0) + 2 * int(dy < 0) + int(abs(dy) > abs(dx))
    return dx, dy, rows, cols, length, octant


MAX_TAPS = 1024                            # csrc/ekf_image.hpp kMaxTaps


def expected_blur(cfg, tpl, h, hb, visible, before=None):
    """The matching templates after the blur: image_oracle.matching_patch for every visible feature -- but the sharp
    template where the line is MAX_TAPS pixels or longer (the device's documented deviation) -- and `before` (default: the
    template) untouched for the others."""
    out = [np.array(t if before is None else before[i], np.uint8, copy=True) for i, t in enumerate(tpl)]
    for i, t in enumerate(tpl):
        if visible[i]:
            fallback = blur_line(h[i], hb[i])[4] >= MAX_TAPS and np.hypot(*blur_line(h[i], hb[i])[:2]) > cfg.kernel_size
            out[i] = t.copy() if fallback else io_.matching_patch(t, h[i], hb[i], cfg.kernel_size)
    return out


_CACHE = {}


def scenes():
    """name -> Scene for every scene (SEARCH_SCENES, BLUR_MOTIONS, BLUR_FALLBACK), built once per process at the first call:
    importing this module, and so collecting the tests, builds nothing."""
    if not _CACHE:
        _CACHE.update(_build_search_scenes())
        _CACHE.update(_build_blur_scenes())
        _CACHE.update(_build_blur_scenes(fallback=True))
    return _CACHE


def dtypes(name):
    """The filter types a scene runs in: fp32, and fp64 too for the border, clamped and oblique scenes."""
    return (np.float32, np.float64) if name in BOTH_TYPES else (np.float32,)


# ---- the host check's cases: the scenes restated as raw kernel inputs, and what the API cannot reach -------------------
# (tools/image_host_check.py writes one file per name; tests/test_host_checks.py compares the list)
RAW_SEARCH = ("frac_below_f32", "frac_below_f64", "outside_frame", "invisible", "window_1", "window_2", "window_3",
              "threshold_equal", "threshold_above")
THRESHOLD_FEATURE = 4                       # of `border`: found with a score below 1
RAW_BLUR = ("blur_fallback", "blur_raw_fallback", "blur_raw_longest")


def host_only_scenes():
    """Windows the device API takes but a real configuration never has: 1 (every score 0 / 0), 2 and 3."""
    return {"window_%d" % w: _kinect_scene("window_%d" % w, window=w, seed=130 + w, move=(-5, 6), sigma_scale=25.0)
            for w in HOST_ONLY_WINDOWS}


def _suffix(T):
    return "f64" if T == np.float64 else "f32"


# scene name -> the types it is written in; every case name of the host check
HOST_CHECK_TYPES = {name: dtypes(name) for name in SEARCH_SCENES + tuple(BLUR_MOTIONS)}
_SCENE_CASES = ["%s_%s" % (name, _suffix(T)) for name, types in HOST_CHECK_TYPES.items() for T in types]
HOST_CHECK_CASES = tuple(sorted(_SCENE_CASES + list(RAW_SEARCH) + list(RAW_BLUR)))
