"""Shapes, lenses and cases shared by tests/test_oracle_rectify.py and tests/test_gpu_rectify.py.

The matcher frame is 61 x 47 (odd sizes: the last workgroup has a tail), the raw frame 122 x 94 at scale 2.  BARREL is the
firewire camera of the reference's conf_firewire.cfg scaled from its 640 x 480 frame to 61 x 47 (the coefficients act on
normalised coordinates and stay): every source position lies inside the image.  PINCUSHION (k1 > 0, p1, p2 != 0) pushes
the corners' source positions out of the image, some fully, some partly.
"""
import numpy as np

import rectify_oracle as ro
import sba_scene as sc

MW, MH, SCALE = 61, 47, 2
RW, RH = MW * SCALE, MH * SCALE

_FIREWIRE = dict(fx=563.21765, fy=558.45293, u0=347.75115, v0=246.19144, k1=-0.45720, k2=0.30980, k3=-0.13950,
                 p1=-0.00265, p2=0.00078)
BARREL = dict(_FIREWIRE, fx=_FIREWIRE["fx"] * MW / 640.0, fy=_FIREWIRE["fy"] * MH / 480.0,
              u0=_FIREWIRE["u0"] * MW / 640.0, v0=_FIREWIRE["v0"] * MH / 480.0)
PINCUSHION = dict(BARREL, k1=0.35, k2=0.10, k3=0.0, p1=0.010, p2=-0.008)
PINHOLE = dict(BARREL, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0)
LENSES = {"barrel": BARREL, "pincushion": PINCUSHION}


def config(base, lens_params, scale=SCALE):
    """A filter config for the test frame: `base` (the package's kinect_config()) with the frame size, scale and lens."""
    return dict(base, image_width=MW, image_height=MH, scale=scale, window_size=5, **lens_params)


def raw_image(seed, channels=3):
    rng = np.random.default_rng(seed)
    shape = (RH, RW, 3) if channels == 3 else (RH, RW)
    return rng.integers(0, 256, size=shape).astype(np.uint8)


def gray_image(seed):
    return np.random.default_rng(seed).integers(0, 256, size=(MH, MW)).astype(np.uint8)


def probe_points(w, h, seed=3):
    """64 pixels of a w x h image: its four corners, its centre, one NaN row, the rest seeded random (some a little outside)."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-2.0, w + 1.0, 64), rng.uniform(-2.0, h + 1.0, 64)], axis=1)
    pts[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    pts[4] = [(w - 1) / 2.0, (h - 1) / 2.0]
    pts[5] = [np.nan, 7.0]
    return pts


# ---- end to end: a distorted camera in front of the pinhole bundle adjuster ---------------------------------------------
# The camera of tests/sba_scene.py (520, 520, 320, 240 on 640 x 480) with the firewire coefficients: at the frame's edge
# (r^2 ~ 0.4) the lens moves a pixel by tens of pixels, so the distorted rows are far above the 4 px the test asks for.
SBA_LENS = dict(fx=sc.CAMERA[0], fy=sc.CAMERA[1], u0=sc.CAMERA[2], v0=sc.CAMERA[3], k1=_FIREWIRE["k1"], k2=_FIREWIRE["k2"],
                k3=_FIREWIRE["k3"], p1=_FIREWIRE["p1"], p2=_FIREWIRE["p2"])


def sba_case():
    """make_scene at its smallest (one free node, 16 points: no point behind a camera), noise-free, repeats dropped:
    true poses and points, the (node, point) pairs, their exact pinhole projections and the rows the distorted lens gives."""
    scene = sc.make_scene(1, 16, seed=4, noise_px=0.0)
    seen, keep = set(), []
    for k, (n, p) in enumerate(zip(scene["node"], scene["point"])):
        if (int(n), int(p)) not in seen:
            seen.add((int(n), int(p)))
            keep.append(k)
    L = ro.lens(SBA_LENS)
    # the exact keypoints under the adjuster's own pose convention (as tests/test_oracle_sba.py builds its converged start)
    import sba_oracle as so
    K = tuple(ro.camera(L))
    w2i = [so.node_mats(p[:3], so.norm_rot(p[3:7]), K)[1] for p in scene["true_nodes"]]
    pin = []
    for n, p in zip(scene["node"][keep], scene["point"][keep]):
        h = w2i[int(n)] @ np.append(scene["true_points"][int(p)], 1.0)
        assert h[2] > 0
        pin.append(h[:2] / h[2])
    pin = np.array(pin)
    return dict(nodes=scene["true_nodes"], points=scene["true_points"], node=scene["node"][keep], point=scene["point"][keep],
                pinhole=pin, distorted=ro.distort_pixels(pin, L), lens=L, camera=tuple(ro.camera(L)))


def sba_rms(case, rows):
    """calcRMSCost of the oracle's SysSBA at the true poses and points for the given rows."""
    import sba_oracle as so
    s = so.SysSBA(case["camera"])
    for p in case["nodes"]:
        s.add_node(p)
    for x in case["points"]:
        s.add_point(x)
    for n, p, m in zip(case["node"], case["point"], rows):
        s.add_proj(int(n), int(p), m)
    return s.calc_rms_cost()
