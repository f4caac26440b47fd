"""Key-frame selection: the per-frame rule of the reference's node (mono-slam
monoslam_ransac.cpp:585-687) on the device, and a recorder that writes what the node writes.

``KeyframeSelector.observe(frame_id)`` after every update is one small launch on the filter's stream and one
read-back; the candidate's and the emitted frame's image stay on the device until ``emitted_image()`` asks for
the one that was selected.  ``KeyframeRecorder`` appends each emitted key frame to ``nodes_and_prjcts.txt`` and
``cams_cov.txt`` (``formats``) and ``finish()`` adds ``points.txt``: the three files ``sba.sba_add`` reads.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi, formats
from .capi import EkfError

NONE, CANDIDATE, EMIT_CURRENT, EMIT_CANDIDATE, EMIT_FIRST = (capi.EKF_KF_NONE, capi.EKF_KF_CANDIDATE, capi.EKF_KF_EMIT_CURRENT,
                                                             capi.EKF_KF_EMIT_CANDIDATE, capi.EKF_KF_EMIT_FIRST)
ACTION_NAMES = {NONE: "NONE", CANDIDATE: "CANDIDATE", EMIT_CURRENT: "EMIT_CURRENT", EMIT_CANDIDATE: "EMIT_CANDIDATE",
                EMIT_FIRST: "EMIT_FIRST"}


@dataclass
class KeyframeRecord:
    """One emitted key frame: what a record of nodes_and_prjcts.txt / cams_cov.txt holds."""
    id: int
    pose: np.ndarray               # (7,) float32: r, q
    sigma: np.ndarray              # (7, 7) float32
    projections: np.ndarray        # (k, 3) int64 rows (real_index, u, v); the single row 0 0 0 = none


@dataclass
class KeyframeResult:
    action: int
    dist: float                    # poses_diff against the last key frame
    cov: float                     # Covariance_Parameter in fp32
    record: Optional[KeyframeRecord] = None

    @property
    def emitted(self) -> bool:
        return self.record is not None

    @property
    def action_name(self) -> str:
        return ACTION_NAMES.get(self.action, str(self.action))


class KeyframeSelector(capi.Handle):
    """monoslam_ransac.cpp:585-687 for one (unsharded) filter."""
    _family = "ekf_keyframe"

    def __init__(self, filter, move_thresh: float = 18.0, keep_current_projections: bool = False, raw_shape=None):
        """``raw_shape`` = (H, W) or (H, W, 3) of the camera's own frame makes a raw selector: it also keeps the frame
        given to ``VSlamFilter.setFrameRaw`` / ``captureNewFrame`` for the candidate and the emitted key frame."""
        self._filter = filter
        self.raw_shape = None if raw_shape is None else tuple(int(v) for v in raw_shape)
        if self.raw_shape is None:
            self._create("ekf_keyframe_create", filter._h, float(move_thresh))
        else:
            if len(self.raw_shape) not in (2, 3):
                raise ValueError("raw_shape is (H, W) or (H, W, 3)")
            self._create("ekf_keyframe_create_raw", filter._h, float(move_thresh), self.raw_shape[1], self.raw_shape[0],
                         1 if len(self.raw_shape) == 2 else self.raw_shape[2])
        self.move_thresh = float(move_thresh)
        self.image_shape = (int(filter._cfg.image_height), int(filter._cfg.image_width))
        if keep_current_projections:
            self._check(self._lib.ekf_keyframe_set_option(self._h, capi.EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS, 1))

    def observe(self, frame_id: int) -> KeyframeResult:
        """Call after the frame's update.  On EMIT_* the result carries the emitted record."""
        action, dist, cov = C.c_int(0), C.c_float(0), C.c_float(0)
        self._check(self._lib.ekf_keyframe_observe(self._h, self._filter._h, int(frame_id), C.byref(action),
                                                   C.byref(dist), C.byref(cov)))
        res = KeyframeResult(action.value, dist.value, cov.value)
        if action.value in (EMIT_CURRENT, EMIT_CANDIDATE, EMIT_FIRST):
            res.record = self.emitted()
        return res

    def emitted(self) -> KeyframeRecord:
        """The last emitted key frame (EKF_ERR_STATE before the first)."""
        kid, n = C.c_int(0), C.c_int(0)
        pose, cov = np.zeros(7, np.float64), np.zeros(49, np.float64)
        self._check(self._lib.ekf_keyframe_get_emitted(self._h, C.byref(kid), pose.ctypes.data_as(C.c_void_p),
                                                       cov.ctypes.data_as(C.c_void_p), 0, None, C.byref(n)))
        rows = np.zeros((n.value, 3), np.int32)                    # the number of rows first, then a buffer that holds them
        self._check(self._lib.ekf_keyframe_get_emitted(self._h, None, None, None, n.value,
                                                       rows.ctypes.data_as(C.c_void_p), C.byref(n)))
        return KeyframeRecord(kid.value, pose.astype(np.float32), cov.reshape(7, 7).T.astype(np.float32),
                              rows[:n.value].astype(np.int64))

    def emitted_image(self) -> np.ndarray:
        """The image of the last emitted key frame, uint8 (height, width): the frame that was set when it was observed."""
        out = np.zeros(self.image_shape, np.uint8)
        self._check(self._lib.ekf_keyframe_get_image(self._h, out.ctypes.data_as(C.c_void_p), out.strides[0]))
        return out

    def emitted_raw_image(self) -> np.ndarray:
        """The raw frame of the last emitted key frame, uint8 of ``raw_shape`` (B, G, R): a raw selector only."""
        if self.raw_shape is None:
            raise EkfError(4, "not a raw selector (KeyframeSelector(..., raw_shape=...))")
        out = np.zeros(self.raw_shape, np.uint8)
        self._check(self._lib.ekf_keyframe_get_raw_image(self._h, out.ctypes.data_as(C.c_void_p), out.strides[0]))
        return out

    # ---- rectified for pinhole consumers ----
    def rectified_camera(self, raw: bool = False) -> np.ndarray:
        """(fx, fy, cx, cy) that ``emitted_image_rectified(raw)`` and ``emitted_rows_rectified(raw)`` belong to."""
        return self._filter.rectifiedCamera(raw) if not raw else self._raw_camera()

    def _raw_camera(self) -> np.ndarray:
        if self.raw_shape is None:
            raise EkfError(4, "not a raw selector (KeyframeSelector(..., raw_shape=...))")
        cfg = self._filter._cfg
        s = np.float64(int(cfg.scale))
        fx, fy, u0, v0 = (np.float64(np.float32(v)) for v in (cfg.fx, cfg.fy, cfg.u0, cfg.v0))
        return np.array([fx * s, fy * s, (u0 + 0.5) * s - 0.5, (v0 + 0.5) * s - 0.5], np.float64)

    def emitted_image_rectified(self, raw: bool = False) -> np.ndarray:
        """The last emitted key frame's image with the lens distortion removed, on the device from the kept copy: the
        matcher's grey frame, or with ``raw`` the raw frame of a raw selector."""
        if raw and self.raw_shape is None:
            raise EkfError(4, "not a raw selector (KeyframeSelector(..., raw_shape=...))")
        out = np.zeros(self.raw_shape if raw else self.image_shape, np.uint8)
        self._check(self._lib.ekf_keyframe_get_image_rectified(self._h, 1 if raw else 0, out.ctypes.data_as(C.c_void_p),
                                                               out.strides[0]))
        return out

    def emitted_rows_rectified(self, raw: bool = False) -> np.ndarray:
        """(k, 2) float64: the undistorted track centres behind the rows of ``emitted().projections``, same order, in
        matcher or (``raw``) raw pixels; k = 0 when the record carries the ``0 0 0`` placeholder."""
        n = C.c_int(0)
        self._check(self._lib.ekf_keyframe_get_emitted_rectified(self._h, 1 if raw else 0, 0, None, C.byref(n)))
        uv = np.zeros((n.value, 2), np.float64)
        if n.value:
            self._check(self._lib.ekf_keyframe_get_emitted_rectified(self._h, 1 if raw else 0, n.value,
                                                                     uv.ctypes.data_as(C.c_void_p), C.byref(n)))
        return uv[:n.value]

    def state(self) -> dict:
        pose, vrot = np.zeros(7, np.float32), np.zeros(3, np.float32)
        mc, cid = C.c_float(0), C.c_int(0)
        self._check(self._lib.ekf_keyframe_get_state(self._h, pose.ctypes.data_as(C.c_void_p), vrot.ctypes.data_as(C.c_void_p),
                                                     C.byref(mc), C.byref(cid)))
        return {"last_pose": pose, "last_vrot": vrot, "min_cov": mc.value, "candidate_id": cid.value}

    def reset(self):
        self._check(self._lib.ekf_keyframe_reset(self._h))


def write_pgm(path: str, gray) -> None:
    """Binary P5."""
    g = np.ascontiguousarray(gray, np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]))
        fh.write(g.tobytes())


def write_ppm(path: str, bgr) -> None:
    """Binary P6 from a (H, W, 3) image in B, G, R order (the channels are swapped to R, G, B)."""
    a = np.asarray(bgr, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_ppm takes a (H, W, 3) image")
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        fh.write(np.ascontiguousarray(a[:, :, ::-1]).tobytes())


class KeyframeRecorder:
    """What the node writes around the selector: ``observe()`` per frame, ``finish()`` at the end.  With ``images`` a raw
    selector's key frames are written at raw size, as the node saves them: ``<id>.ppm`` (3 channels) or ``<id>.pgm`` (1);
    a plain selector's as the matcher's grey frame, ``<id>.pgm``.

    ``rectify=True`` records for a pinhole consumer: the images are the rectified ones (same names and
    sizes), the projection rows are the undistorted track centres at the resolution of the images, rounded to the nearest
    integer (``floor(x + 0.5)``, so the reference's ``int u, v`` reader still reads them), and ``camera.txt`` holds the
    ``fx fy cx cy`` that both belong to.  The default writes what it always wrote, byte for byte."""

    def __init__(self, selector: KeyframeSelector, directory: str, images: bool = False, rectify: bool = False):
        self.selector = selector
        self.directory = directory
        self.images = bool(images)
        self.rectify = bool(rectify)
        self.raw = getattr(selector, "raw_shape", None) is not None    # the resolution of the images and, rectified, of the rows
        os.makedirs(directory, exist_ok=True)
        self.nodes_path = os.path.join(directory, "nodes_and_prjcts.txt")
        self.covs_path = os.path.join(directory, "cams_cov.txt")
        self.points_path = os.path.join(directory, "points.txt")
        open(self.nodes_path, "w").close()
        open(self.covs_path, "w").close()
        self.ids = []
        if self.rectify:
            self.camera_path = os.path.join(directory, "camera.txt")
            formats.write_camera(self.camera_path, selector.rectified_camera(self.raw))

    def observe(self, frame_id: int) -> KeyframeResult:
        res = self.selector.observe(frame_id)
        if res.emitted and self.rectify:
            self._append_rectified(res.record)
        elif res.emitted:
            self.append(res.record)
            if self.images and getattr(self.selector, "raw_shape", None) is not None:
                raw = self.selector.emitted_raw_image()
                if raw.ndim == 3 and raw.shape[2] == 3:
                    write_ppm(os.path.join(self.directory, "%d.ppm" % res.record.id), raw)
                else:
                    write_pgm(os.path.join(self.directory, "%d.pgm" % res.record.id), raw.reshape(raw.shape[0], raw.shape[1]))
            elif self.images:
                write_pgm(os.path.join(self.directory, "%d.pgm" % res.record.id), self.selector.emitted_image())
        return res

    def _append_rectified(self, record: KeyframeRecord) -> None:
        prj = record.projections
        uv = self.selector.emitted_rows_rectified(self.raw)
        if len(uv):                                                   # same rows, same order: only the coordinates change
            prj = prj.copy()
            prj[:, 1:] = np.floor(uv + 0.5).astype(np.int64)
        self.append(KeyframeRecord(record.id, record.pose, record.sigma, prj))
        if not self.images:
            return
        img = self.selector.emitted_image_rectified(self.raw)
        if img.ndim == 3 and img.shape[2] == 3:
            write_ppm(os.path.join(self.directory, "%d.ppm" % record.id), img)
        else:
            write_pgm(os.path.join(self.directory, "%d.pgm" % record.id), img.reshape(img.shape[0], img.shape[1]))

    def append(self, record: KeyframeRecord) -> None:
        prj = record.projections
        none = len(prj) == 0 or (len(prj) == 1 and not prj[0].any())
        with open(self.nodes_path, "a") as fh:
            fh.write(formats.pose_record(record.id, record.pose, None if none else prj))
        with open(self.covs_path, "a") as fh:
            fh.write(formats.camera_cov_record(record.sigma))
        self.ids.append(int(record.id))

    def finish(self):
        """points.txt from the filter's table; (points, nodes_and_prjcts, cams_cov) as ``sba.sba_add`` takes them."""
        formats.write_points(self.points_path, self.selector._filter.getPointsTable())
        return self.points_path, self.nodes_path, self.covs_path
