"""Dense plane-sweep depth maps for key frames: posed, rectified key frames in, depth maps and world
points out.  ``DenseStereo`` mirrors the ``ekf_dense_*`` functions; ``depth_maps_from_recording`` drives it over what a
rectifying ``KeyframeRecorder`` wrote, with the poses ``sba.sba_add`` refined when its ``Nodes_Out.txt`` is given.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi, formats
from .capi import ptr as _ptr

MAX_VIEWS, MAX_SOURCES = 16, 8
UNIQUE_KERNELS = ("k_plane_sweep_unique", "k_plane_sweep_census_unique", "k_plane_sweep_best_unique",
                  "k_plane_sweep_best_census_unique", "k_sgm_winner_unique", "k_depth_filter_unique")
SPECKLE_KERNELS = ("k_speckle_label", "k_speckle_merge", "k_speckle_count", "k_speckle_apply")


@dataclass
class DepthMap:
    """One key frame's result of ``depth_maps_from_recording``."""
    id: int
    pose: np.ndarray               # (7,) float64: t, q (w x y z) as it was set
    sources: tuple                 # ids of the key frames it was swept against
    depth: np.ndarray              # (H, W) float32, filtered; 0 = none
    plane: np.ndarray              # (H, W) int32, filtered; -1 = none
    swept_depth: np.ndarray        # (H, W) float32, before the filter
    cost: np.ndarray               # (H, W) uint32
    views: np.ndarray              # (H, W) uint8
    points: np.ndarray             # (H, W, 3) float64 of the filtered map, NaN where there is no depth
    runner_up: Optional[np.ndarray] = None    # (H, W) uint32, 0xFFFFFFFF = absent (§22); None when not recorded
    segment_size: Optional[np.ndarray] = None  # (H, W) uint32, a pixel's segment before the speckle filter (§23); None without it


class DenseStereo(capi.Handle):
    """Up to ``max_views`` (<= 16) pinhole views of one size on the device; slots are 0 .. max_views - 1."""
    _family = "ekf_dense"

    def __init__(self, width: int, height: int, max_views: int = MAX_VIEWS, device: int = 0):
        self._create("ekf_dense_create", int(width), int(height), int(max_views), int(device))
        self.width, self.height, self.max_views, self.device = int(width), int(height), int(max_views), int(device)
        self.shape = (self.height, self.width)

    # ---- views ----
    def set_view(self, slot: int, image, K, pose7):
        """``image``: (height, width) uint8 on the host, or a CUDA/HIP ``torch`` tensor of that shape (no host round trip).
        A (height, width, 3) image in B, G, R order, from either place, makes a colour view: the slot keeps
        it and sweeps its grey conversion."""
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        if hasattr(image, "data_ptr") and getattr(image, "is_cuda", False):
            if image.dim() == 3:
                if (tuple(image.shape) != self.shape + (3,) or str(image.dtype) != "torch.uint8" or image.stride(2) != 1
                        or image.stride(1) != 3 or image.stride(0) < 3 * self.width):
                    raise ValueError("a device colour image is (height, width, 3) uint8 with unit channel stride, pixel stride 3 "
                                     "and rows at least 3 widths apart")
                if (image.device.index or 0) != self.device:
                    raise ValueError("the device image lives on device %r, the handle on device %d" % (image.device.index, self.device))
                self._check(self._lib.ekf_dense_set_view_colour_device(self._h, int(slot), C.c_void_p(image.data_ptr()),
                                                                       int(image.stride(0)), _ptr(K), _ptr(pose)))
                return
            if tuple(image.shape) != self.shape or str(image.dtype) != "torch.uint8" or image.stride(1) != 1 or image.stride(0) < self.width:
                raise ValueError("a device image is (height, width) uint8 with unit column stride and rows at least a width apart")
            if (image.device.index or 0) != self.device:
                raise ValueError("the device image lives on device %r, the handle on device %d" % (image.device.index, self.device))
            self._check(self._lib.ekf_dense_set_view_device(self._h, int(slot), C.c_void_p(image.data_ptr()),
                                                            int(image.stride(0)), _ptr(K), _ptr(pose)))
            return
        img = np.ascontiguousarray(image, np.uint8)
        if img.shape == self.shape + (3,):
            self._check(self._lib.ekf_dense_set_view_colour(self._h, int(slot), _ptr(img), img.strides[0], _ptr(K), _ptr(pose)))
            return
        if img.shape != self.shape:
            raise ValueError("image must be (height, width) = %r, or (height, width, 3) for colour" % (self.shape,))
        self._check(self._lib.ekf_dense_set_view(self._h, int(slot), _ptr(img), img.strides[0], _ptr(K), _ptr(pose)))

    def set_view_from_keyframe(self, slot: int, selector, pose7, raw: bool = False, colour: bool = False):
        """The selector's last emitted key frame, rectified on the device straight into the slot; K is the selector's
        rectified camera of that resolution.  ``colour``: the raw key frame of a 3-channel raw selector, as a colour view."""
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        if colour:
            self._check(self._lib.ekf_dense_set_view_colour_from_keyframe(self._h, int(slot), selector._h, _ptr(pose)))
            return
        self._check(self._lib.ekf_dense_set_view_from_keyframe(self._h, int(slot), selector._h, 1 if raw else 0, _ptr(pose)))

    def set_pose(self, slot: int, pose7):
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        self._check(self._lib.ekf_dense_set_pose(self._h, int(slot), _ptr(pose)))

    def view(self, slot: int):
        """(image, K, pose7) a set slot holds; q is normalised."""
        img, K, pose = np.zeros(self.shape, np.uint8), np.zeros(4, np.float64), np.zeros(7, np.float64)
        self._check(self._lib.ekf_dense_get_view(self._h, int(slot), _ptr(img), img.strides[0], _ptr(K), _ptr(pose)))
        return img, K, pose

    def has_colour(self, slot: int) -> bool:
        return self._lib.ekf_dense_get_view_colour(self._h, int(slot), None, 0) == 0

    def view_colour(self, slot: int) -> np.ndarray:
        """The (height, width, 3) B, G, R image of a colour view; an error for a slot that holds none."""
        bgr = np.zeros(self.shape + (3,), np.uint8)
        self._check(self._lib.ekf_dense_get_view_colour(self._h, int(slot), _ptr(bgr), bgr.strides[0]))
        return bgr

    # ---- the two launches ----
    def sweep(self, ref: int, sources: Sequence[int], w_min: float, w_max: float, planes: int = 64, radius: int = 2,
              trunc: int = 40, cost: str = "ad", best: Optional[int] = None):
        """``cost``: ``"ad"``, the truncated absolute grey difference, or ``"census"``, the truncated
        Hamming distance of 9 x 7 census descriptors (§20), for key frames whose exposure or gain differ.
        ``best``: ``None`` sums the cost over all sources; an int keeps, per pixel and plane, that many cheapest sources
        (§21), for sources that do not all see every pixel of ``ref``."""
        fn = _cost_entry(self._lib, cost, "ekf_dense_sweep")
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        if best is not None:
            self._check(self._lib.ekf_dense_sweep_best(self._h, int(ref), _ptr(src), len(src), int(best), float(w_min), float(w_max),
                                                       int(planes), int(radius), int(trunc), int(cost == "census"), 0, 0, 0))
            return
        self._check(fn(self._h, int(ref), _ptr(src), len(src), float(w_min), float(w_max), int(planes), int(radius), int(trunc)))

    def sweep_sgm(self, ref: int, sources: Sequence[int], w_min: float, w_max: float, planes: int = 64, radius: int = 1,
                  trunc: int = 40, p1: Optional[int] = None, p2: Optional[int] = None, paths: int = 8, cost: str = "ad",
                  best: Optional[int] = None):
        """The sweep with semi-global cost aggregation: the slot's swept map, for ``filter``, ``depth``,
        ``points`` and the fusion exactly as after ``sweep``.  With n = (2 radius + 1)^2 len(sources), ``None`` means
        p1 = 2 n and p2 = 16 n: the values of the synthetic flat-patch scenes, not measured on real imagery -- with
        ``cost="census"`` (§20) as with ``"ad"``.  ``best``: as in ``sweep`` (§21); an int takes its place in n, which is
        then (2 radius + 1)^2 best."""
        fn = _cost_entry(self._lib, cost, "ekf_dense_sweep_sgm")
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        n = (2 * int(radius) + 1) ** 2 * (len(src) if best is None else int(best))
        p1 = 2 * n if p1 is None else int(p1)
        p2 = 16 * n if p2 is None else int(p2)
        if best is not None:
            self._check(self._lib.ekf_dense_sweep_best(self._h, int(ref), _ptr(src), len(src), int(best), float(w_min), float(w_max),
                                                       int(planes), int(radius), int(trunc), int(cost == "census"), int(paths), p1, p2))
            self._sgm_planes = int(planes)
            return
        self._check(fn(self._h, int(ref), _ptr(src), len(src), float(w_min), float(w_max), int(planes), int(radius), int(trunc),
                       p1, p2, int(paths)))
        self._sgm_planes = int(planes)

    def volume(self, slot: int, aggregated: bool = True) -> np.ndarray:
        """(planes, height, width) uint32: the aggregated or the raw cost volume of the last ``sweep_sgm``, whose slot
        ``slot`` must be, with no setter or sweep of it since."""
        out = np.zeros((getattr(self, "_sgm_planes", 1),) + self.shape, np.uint32)
        self._check(self._lib.ekf_dense_get_volume(self._h, int(slot), 1 if aggregated else 0, _ptr(out)))
        return out

    def census(self, slot: int) -> np.ndarray:
        """(height, width) uint64: the census descriptors of a set slot's image (bits 0 .. 61)."""
        out = np.zeros(self.shape, np.uint64)
        self._check(self._lib.ekf_dense_get_census(self._h, int(slot), _ptr(out)))
        return out

    def filter(self, ref: int, sources: Sequence[int], rel_tol: float = 0.01, min_agree: int = 1, uniqueness: int = 0):
        """``uniqueness``: 0 .. 100 per cent.  0 is the geometric filter alone; u > 0 also drops the pixels of ``ref`` whose
        runner-up cost C2 has (C2 - cost) 100 < u C2 and needs ``ref`` swept under ``keep_runner_up()``."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        if uniqueness == 0:
            self._check(self._lib.ekf_dense_filter(self._h, int(ref), _ptr(src), len(src), float(rel_tol), int(min_agree)))
            return
        self._check(self._lib.ekf_dense_filter_unique(self._h, int(ref), _ptr(src), len(src), float(rel_tol), int(min_agree),
                                                      int(uniqueness)))

    # ---- the runner-up cost ----
    def keep_runner_up(self, on: bool = True):
        """While on, every sweep also records its slot's runner-up cost, the least cost at least two planes from the winner."""
        self._check(self._lib.ekf_dense_keep_runner_up(self._h, 1 if on else 0))

    def runner_up(self, slot: int) -> np.ndarray:
        """(height, width) uint32 of a slot swept under ``keep_runner_up()``; 0xFFFFFFFF where no plane is two away."""
        out = np.zeros(self.shape, np.uint32)
        self._check(self._lib.ekf_dense_get_runner_up(self._h, int(slot), _ptr(out)))
        return out

    # ---- the speckle filter ----
    def filter_speckle(self, slot: int, min_size: int, max_diff: int = 1):
        """Drops, from the slot's filtered map in place, the connected segments of fewer than ``min_size`` pixels; two
        4-neighbours are in one segment if both have a plane and the planes differ by at most ``max_diff``.  The swept map
        stays; a later ``filter`` of the slot starts again from it."""
        self._check(self._lib.ekf_dense_filter_speckle(self._h, int(slot), int(min_size), int(max_diff)))

    def segments(self, slot: int):
        """(label, size), both (height, width) uint32, before the removal of the last ``filter_speckle``, whose slot ``slot``
        must be, with no setter, sweep or filter of it since: a pixel's label is the least index y width + x of its segment
        (0xFFFFFFFF: no plane), its size the segment's pixel count."""
        label, size = np.zeros(self.shape, np.uint32), np.zeros(self.shape, np.uint32)
        self._check(self._lib.ekf_dense_get_segments(self._h, int(slot), _ptr(label), _ptr(size)))
        return label, size

    def speckle_maps(self, depth, plane, min_size: int, max_diff: int = 1) -> dict:
        """The speckle filter of (height, width) maps from the host, whatever made them: dict(depth, plane, label, size), the
        filtered copies and the segments before the removal.  The inputs are not modified; no slot is touched."""
        if np.shape(depth) != self.shape or np.shape(plane) != self.shape:
            raise ValueError("depth and plane must be (height, width) = %r" % (self.shape,))
        out = dict(depth=np.array(depth, np.float32, order="C"), plane=np.array(plane, np.int32, order="C"),
                   label=np.zeros(self.shape, np.uint32), size=np.zeros(self.shape, np.uint32))
        self._check(self._lib.ekf_dense_speckle_host(self._h, _ptr(out["depth"]), _ptr(out["plane"]), int(min_size), int(max_diff),
                                                     _ptr(out["label"]), _ptr(out["size"])))
        return out

    # ---- results ----
    def depth(self, slot: int, filtered: bool = False) -> dict:
        """depth float32 (0 = none), plane int32 (-1 = none), and of the sweep cost uint32 and views uint8."""
        out = dict(depth=np.zeros(self.shape, np.float32), plane=np.zeros(self.shape, np.int32),
                   cost=np.zeros(self.shape, np.uint32), views=np.zeros(self.shape, np.uint8))
        self._check(self._lib.ekf_dense_get_depth(self._h, int(slot), 1 if filtered else 0, _ptr(out["depth"]), _ptr(out["plane"]),
                                                  _ptr(out["cost"]), _ptr(out["views"])))
        return out

    def points(self, slot: int, filtered: bool = False) -> np.ndarray:
        """(height, width, 3) float64 world points; NaN where there is no depth."""
        xyz = np.zeros(self.shape + (3,), np.float64)
        self._check(self._lib.ekf_dense_get_points(self._h, int(slot), 1 if filtered else 0, _ptr(xyz)))
        return xyz

    def write_ply(self, path: str, slot: int, filtered: bool = True) -> int:
        """ASCII PLY of the finite points of a slot with the grey value of their pixel; returns their number."""
        xyz = self.points(slot, filtered)
        grey = self.view(slot)[0]
        ok = np.isfinite(xyz).all(axis=2)
        pts, g = xyz[ok], grey[ok]
        with open(path, "w") as fh:
            fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                     "property uchar intensity\nend_header\n" % len(pts))
            for (x, y, z), v in zip(pts, g):
                fh.write("%.17g %.17g %.17g %d\n" % (x, y, z, int(v)))
        return len(pts)

    def profile(self, enable: bool = True):
        self._check(self._lib.ekf_dense_profile(self._h, 1 if enable else 0))

    def get_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the two kernels since the last ``profile()``."""
        ms, cnt = np.zeros(2, np.float64), np.zeros(2, np.int64)
        self._check(self._lib.ekf_dense_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {"k_plane_sweep": (float(ms[0]), int(cnt[0])), "k_depth_filter_points": (float(ms[1]), int(cnt[1]))}


    def get_sgm_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the kernels of ``sweep_sgm`` since the last ``profile()``:
        ``k_sweep_volume``, ``k_sgm_path[0]`` .. ``k_sgm_path[7]`` (one per direction) and ``k_sgm_winner``."""
        ms, cnt = np.zeros(10, np.float64), np.zeros(10, np.int64)
        self._check(self._lib.ekf_dense_get_sgm_profile(self._h, _ptr(ms), _ptr(cnt)))
        names = ["k_sweep_volume"] + ["k_sgm_path[%d]" % i for i in range(8)] + ["k_sgm_winner"]
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(names)}

    def get_census_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the kernels of the census cost (§20) since the last ``profile()``."""
        ms, cnt = np.zeros(3, np.float64), np.zeros(3, np.int64)
        self._check(self._lib.ekf_dense_get_census_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(("k_census", "k_plane_sweep_census", "k_sweep_volume_census"))}

    def get_best_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the four kernels of the best-K selection (§21) since the last
        ``profile()``."""
        ms, cnt = np.zeros(4, np.float64), np.zeros(4, np.int64)
        self._check(self._lib.ekf_dense_get_best_profile(self._h, _ptr(ms), _ptr(cnt)))
        names = ("k_plane_sweep_best", "k_plane_sweep_best_census", "k_sweep_volume_best", "k_sweep_volume_best_census")
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(names)}

    def get_unique_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the six kernels of the runner-up cost and the uniqueness test (§22)
        since the last ``profile()``."""
        ms, cnt = np.zeros(len(UNIQUE_KERNELS), np.float64), np.zeros(len(UNIQUE_KERNELS), np.int64)
        self._check(self._lib.ekf_dense_get_unique_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(UNIQUE_KERNELS)}

    def get_speckle_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the four kernels of the speckle filter (§23) since the last
        ``profile()``."""
        ms, cnt = np.zeros(len(SPECKLE_KERNELS), np.float64), np.zeros(len(SPECKLE_KERNELS), np.int64)
        self._check(self._lib.ekf_dense_get_speckle_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(SPECKLE_KERNELS)}


def _cost_entry(lib, cost, name):
    """The C function of a sweep for the matching cost ``cost``."""
    if cost not in ("ad", "census"):
        raise ValueError('cost is "ad" or "census"')
    return getattr(lib, name if cost == "ad" else name + "_census")


def read_ply(path: str):
    """What ``write_ply`` wrote: ((n, 3) float64 points, (n,) uint8 grey values)."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    end = lines.index("end_header")
    n = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[2])
    rows = [ln.split() for ln in lines[end + 1:end + 1 + n]]
    return (np.array([[float(t) for t in r[:3]] for r in rows], np.float64).reshape(-1, 3),
            np.array([int(r[3]) for r in rows], np.uint8))


def read_pgm(path: str) -> np.ndarray:
    """Binary P5, 8 bit (what ``keyframes.write_pgm`` writes)."""
    data = open(path, "rb").read()
    m = re.match(rb"P5\s+(\d+)\s+(\d+)\s+255\s", data)
    if not m:
        raise ValueError("%s is not an 8-bit binary PGM" % path)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():m.end() + w * h], np.uint8).reshape(h, w).copy()


def read_ppm(path: str) -> np.ndarray:
    """Binary P6, 8 bit (what ``keyframes.write_ppm`` writes), as a (H, W, 3) image swapped back to B, G, R order."""
    data = open(path, "rb").read()
    m = re.match(rb"P6\s+(\d+)\s+(\d+)\s+255\s", data)
    if not m:
        raise ValueError("%s is not an 8-bit binary PPM" % path)
    w, h = int(m.group(1)), int(m.group(2))
    return np.ascontiguousarray(np.frombuffer(data[m.end():m.end() + 3 * w * h], np.uint8).reshape(h, w, 3)[:, :, ::-1])


def read_recording(directory: str, nodes_out=None):
    """(K, ids, poses (n, 7) float64, images) of a recording of ``KeyframeRecorder(rectify=True, images=True)``; the poses
    are those of ``nodes_and_prjcts.txt`` (float32 widened) unless ``nodes_out`` (``Nodes_Out.txt`` of ``sba_add``) has the id.
    A key frame is ``<id>.pgm``, a (H, W) image, or where that is absent ``<id>.ppm``, a (H, W, 3) image in B, G, R order."""
    K = np.array(formats.read_camera(os.path.join(directory, "camera.txt")), np.float64)
    records = formats.read_pose_records(os.path.join(directory, "nodes_and_prjcts.txt"))
    ids = [int(r[0]) for r in records]
    poses = np.array([np.asarray(r[1], np.float32).astype(np.float64) for r in records], np.float64).reshape(-1, 7)
    if nodes_out is not None:
        oid, opose = formats.read_nodes_out(nodes_out)
        adjusted = {int(i): p for i, p in zip(oid, opose)}
        for k, i in enumerate(ids):
            if i in adjusted:
                poses[k] = adjusted[i]
    images = []
    for i in ids:
        path = os.path.join(directory, "%d.pgm" % i)
        if os.path.exists(path):
            images.append(read_pgm(path))
            continue
        colour = os.path.join(directory, "%d.ppm" % i)
        if not os.path.exists(colour):
            raise ValueError("%s is missing, and so is %s" % (path, colour))
        images.append(read_ppm(colour))
    return K, ids, poses, images


def neighbours_of(i: int, n: int, neighbours: int):
    """The indices of the `neighbours` nearest key frames on each side of i in file order."""
    return [j for j in range(i - neighbours, i + neighbours + 1) if j != i and 0 <= j < n]


def depth_maps_from_recording(directory: str, nodes_out: Optional[str] = None, neighbours: int = 2, w_min: float = 0.05,
                              w_max: float = 2.0, planes: int = 64, radius: int = 2, trunc: int = 40, rel_tol: float = 0.01,
                              min_agree: int = 1, device: int = 0, sgm=None, cost: str = "ad",
                              best: Optional[int] = None, uniqueness: int = 0, speckle=None):
    """Sweeps every key frame of a rectified recording against its ``neighbours`` nearest key frames on each side in file
    order, filters each map against the swept maps of the same neighbours and returns one ``DepthMap`` per key frame.
    The views pass through a ring of 16 device slots, so ``neighbours`` is 1 .. 3 (a map needs the views two
    neighbourhoods away) and the recording may be of any length >= 2.  Colour key frames become colour views.
    ``sgm``: ``None`` sweeps with ``sweep``; ``True`` or a dict of ``p1`` / ``p2`` / ``paths`` with ``sweep_sgm`` (§19).
    ``cost``: ``"ad"`` or ``"census"`` (§20), the matching cost of either sweep.
    ``best``: ``None``, or the number of cheapest sources either sweep keeps per pixel and plane (§21); a key frame with fewer
    sources than that keeps them all, as with ``min_agree``.
    ``uniqueness``: 0, or the per cent of the uniqueness test every map's filter also applies (§22); the sweeps then record
    their runner-up costs, which each ``DepthMap`` carries.
    ``speckle``: ``None``, an int ``min_size`` or ``(min_size, max_diff)``: the speckle filter (§23) of every map right after
    its filter (``max_diff`` 1 for an int); each ``DepthMap`` then carries its pixels' segment sizes."""
    if speckle is not None:
        speckle = (speckle, 1) if isinstance(speckle, (int, np.integer)) and not isinstance(speckle, bool) else speckle
        if not (isinstance(speckle, tuple) and len(speckle) == 2 and 1 <= int(speckle[0]) <= 1 << 26 and 0 <= int(speckle[1]) <= 1023):
            raise ValueError("speckle is None, an int min_size in 1 .. 2^26, or (min_size, max_diff) with max_diff in 0 .. 1023")
    if not 0 <= int(uniqueness) <= 100:
        raise ValueError("uniqueness is 0 .. 100")
    if best is not None and int(best) < 1:
        raise ValueError("best is None or an int >= 1")
    if cost not in ("ad", "census"):
        raise ValueError('cost is "ad" or "census"')
    if sgm is not None and sgm is not True and not (isinstance(sgm, dict) and set(sgm) <= {"p1", "p2", "paths"}):
        raise ValueError("sgm is None, True or a dict of p1 / p2 / paths")
    if not 1 <= int(neighbours) <= 3:
        raise ValueError("neighbours is 1 .. 3")
    K, ids, poses, images = read_recording(directory, nodes_out)
    n = len(ids)
    if n < 2:
        raise ValueError("a depth map needs at least two key frames")
    h, w = images[0].shape[:2]
    ds = DenseStereo(w, h, min(MAX_VIEWS, n), device)
    ring = ds.max_views
    loaded = swept = 0                                             # key frames [0, loaded) are in their slots, [0, swept) swept
    out = []
    try:
        if uniqueness:
            ds.keep_runner_up(True)
        for i in range(n):
            while loaded < min(n, i + 2 * neighbours + 1):
                ds.set_view(loaded % ring, images[loaded], K, poses[loaded])
                loaded += 1
            while swept < min(n, i + neighbours + 1):
                src = [j % ring for j in neighbours_of(swept, n, neighbours)]
                keep = None if best is None else min(int(best), len(src))
                if sgm is None:
                    ds.sweep(swept % ring, src, w_min, w_max, planes, radius, trunc, cost=cost, best=keep)
                else:
                    ds.sweep_sgm(swept % ring, src, w_min, w_max, planes, radius, trunc, cost=cost, best=keep,
                                 **({} if sgm is True else sgm))
                swept += 1
            src = neighbours_of(i, n, neighbours)
            ds.filter(i % ring, [j % ring for j in src], rel_tol, min(min_agree, len(src)), int(uniqueness))
            if speckle is not None:
                ds.filter_speckle(i % ring, int(speckle[0]), int(speckle[1]))
            raw, flt = ds.depth(i % ring, False), ds.depth(i % ring, True)
            out.append(DepthMap(ids[i], poses[i].copy(), tuple(ids[j] for j in src), flt["depth"], flt["plane"], raw["depth"],
                                raw["cost"], raw["views"], ds.points(i % ring, True),
                                ds.runner_up(i % ring) if uniqueness else None,
                                ds.segments(i % ring)[1] if speckle is not None else None))
    finally:
        ds.close()
    return out
