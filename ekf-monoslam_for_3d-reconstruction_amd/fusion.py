"""Fusion of key-frame depth maps into a TSDF volume and a triangle mesh: ``TsdfVolume`` mirrors the
``ekf_fusion_*`` functions, ``weld`` joins the triangle soup by its vertex keys on the host, ``write_mesh_ply`` /
``read_mesh_ply`` store the result, and ``mesh_from_recording`` drives ``dense.depth_maps_from_recording`` and the volume
over a rectified recording.  ``TsdfVolume.raycast`` / ``raycast_view`` mirror ``ekf_raycast_*`` (§17): the volume seen from a
pose as a depth, a normal and a grey image; ``shade`` turns one into a picture and ``audit_recording`` compares the
reconstruction of a recording with its own key frames.  ``TsdfVolume(..., colour=True)`` is a colour volume (§18): meshes,
renders and audits then carry B, G, R beside the grey.  ``TsdfVolume.weld`` mirrors ``ekf_mesh_*`` (§24): the same indexed mesh
welded on the device, with per-vertex normals on request; ``TsdfVolume.components`` and ``.prune`` find its connected
components there and drop the small ones (§25); ``TsdfVolume.smooth`` smooths either mesh there with Taubin's scheme and gives
it normals from its own triangles (§26); ``TsdfVolume.simplify`` clusters the vertices of any of the three on a grid of cells
(§28); ``TsdfVolume.texture_begin`` / ``texture_add_view`` / ``texture_finish`` fill a per-triangle texture atlas of any of the
four from views (§29), and ``write_mesh_obj`` stores a mesh with its atlas; ``TsdfVolume.rasterise`` / ``rasterise_view``
render any of the four, or a mesh given with ``set_raster_mesh``, from a pose with its vertex colours or that atlas (§30);
``TsdfVolume.distance`` / ``distance_points`` / ``distance_stats`` and ``compare_meshes`` measure how far the vertices of one of
them, or points of the caller's, lie from another, or from a mesh given with ``set_distance_mesh`` (§31).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi, dense
from .capi import ptr as _ptr

MAX_DIM, MAX_VOXELS, MAX_MAPS = 1024, 1 << 28, 65535
KERNELS = ("k_tsdf_integrate", "k_tsdf_count", "k_tsdf_scan", "k_tsdf_emit")
RAYCAST_KERNELS = ("k_tsdf_mean", "k_tsdf_raycast")
COLOUR_KERNELS = ("k_tsdf_integrate_colour", "k_tsdf_colour_vertices", "k_tsdf_raycast_colour")
MESH_KERNELS = ("k_mesh_cells", "k_mesh_edges", "k_tsdf_scan", "k_mesh_vertices", "k_mesh_faces")
COMPONENT_KERNELS = ("k_comp_init", "k_comp_union", "k_comp_count", "k_comp_largest", "k_comp_flags", "k_tsdf_scan", "k_comp_vertices",
                     "k_comp_faces")
SMOOTH_KERNELS = ("k_smooth_count", "k_smooth_offsets", "k_tsdf_scan", "k_smooth_fill", "k_smooth_lists", "k_smooth_step",
                  "k_smooth_normals")
SIMPLIFY_KERNELS = ("k_simp_cells", "k_simp_count", "k_simp_offsets", "k_tsdf_scan", "k_simp_fill", "k_simp_lists", "k_simp_flags",
                    "k_simp_vertices", "k_simp_faces", "k_simp_map")
SIMPLIFY_SOURCES = {"weld": 0, "pruned": 1, "smoothed": 2}
TEXTURE_KERNELS = ("k_tex_project", "k_tex_select", "k_tex_fill", "k_tex_fallback")
TEXTURE_SOURCES = {"weld": 0, "pruned": 1, "smoothed": 2, "simplified": 3}
RASTER_KERNELS = ("k_rast_project", "k_rast_small", "k_rast_large", "k_rast_resolve")
RASTER_SOURCES = {"weld": 0, "pruned": 1, "smoothed": 2, "simplified": 3, "mesh": 4}
RASTER_SHADINGS = {"vertex": 0, "texture": 1}
DISTANCE_KERNELS = ("k_dist_box", "k_dist_grid", "k_dist_count", "k_dist_offsets", "k_tsdf_scan", "k_dist_fill", "k_dist_query",
                    "k_dist_stats", "k_dist_reduce")
DISTANCE_SOURCES = RASTER_SOURCES


@dataclass
class Mesh:
    """The triangle soup of ``TsdfVolume.extract`` in its fixed order."""
    xyz: np.ndarray                # (n, 3, 3) float64
    key: np.ndarray                # (n, 3) uint64: equal keys are bit-equal vertices
    grey: np.ndarray               # (n, 3) uint8
    colour: Optional[np.ndarray] = None       # (n, 3, 3) uint8, B G R of each vertex: colour volumes only


@dataclass
class IndexedMesh:
    """The welded mesh of ``TsdfVolume.weld``: one vertex per distinct key of the soup, by ascending key; what ``weld`` makes
    of ``TsdfVolume.extract`` on the host, bit for bit."""
    vertices: np.ndarray           # (m, 3) float64
    faces: np.ndarray              # (n, 3) uint32 into vertices, in the soup's triangle order
    grey: np.ndarray               # (m,) uint8
    colour: Optional[np.ndarray] = None       # (m, 3) uint8, B G R: colour volumes only
    normals: Optional[np.ndarray] = None      # (m, 3) float32, unit, towards free space (0 0 0: no gradient): ``normals=True`` only
    key: Optional[np.ndarray] = None          # (m,) uint64, ascending


@dataclass
class MeshComponents:
    """The connected components of the last ``TsdfVolume.weld``: two vertices are linked iff a triangle has
    both, by index, not by coordinate."""
    label: np.ndarray              # (m,) uint32: the least vertex index of the vertex's component
    size: np.ndarray               # (m,) uint32: the number of triangles of that component
    count: int                     # the number of components


@dataclass
class MeshAdjacency:
    """The adjacency of the mesh the last ``TsdfVolume.smooth`` ran on: a function of its faces alone."""
    inc: np.ndarray                # (m,) uint32: the number of triangles that contain the vertex
    deg: np.ndarray                # (m,) uint32: the number of distinct vertices that share a triangle with it
    boundary: np.ndarray           # (m,) uint8: 1 iff it has an edge that lies in exactly one triangle


@dataclass
class SimplifyStats:
    """The triangles the last ``TsdfVolume.simplify`` dropped: kept + degenerate + duplicate = the source's."""
    degenerate: int                # two of the three vertices fell into one cell
    duplicate: int                 # a triangle with a smaller index has the same unordered triple of cells


@dataclass
class TextureAtlas:
    """What ``TsdfVolume.texture_finish`` returns: triangle t of the source owns one half of block t >> 1."""
    atlas: np.ndarray              # (A, A) uint8, or (A, A, 3) in B, G, R order; row 0 first
    uv: np.ndarray                 # (n, 3, 2) float64: u, v of the three corners, v measured from row 0
    view: np.ndarray               # (n,) int32: the number of the view that textured the triangle, -1: none (vertex colours)
    score: np.ndarray              # (n,) float64: twice the triangle's area in that view's pixels, 0: none
    n_textured: int                # the number of triangles with a view


@dataclass
class Render:
    """What ``TsdfVolume.raycast`` returns; a pixel without a hit has depth 0, normal 0 and grey 0."""
    depth: np.ndarray              # (H, W) float32: camera-z depth of the surface
    normal: np.ndarray             # (H, W, 3) float32: unit, world frame, towards free space
    grey: np.ndarray               # (H, W) uint8
    colour: Optional[np.ndarray] = None       # (H, W, 3) uint8, B G R: colour volumes only


@dataclass
class MeshRender(Render):
    """What ``TsdfVolume.rasterise`` returns: a mesh seen from a pose.  ``normal`` is the winning triangle's own,
    not flipped for a back face; a pixel without a hit has depth 0, tri -1, bary 0, normal 0 and colour 0."""
    tri: Optional[np.ndarray] = None          # (H, W) int32: the triangle of the source that the pixel shows, -1: none
    bary: Optional[np.ndarray] = None         # (H, W, 2) float32: its perspective-correct barycentrics l1, l2 (l0 = 1 - l1 - l2)
    cover: Optional[np.ndarray] = None        # (H, W) uint32: the triangles that cover the pixel; ``cover=True`` only


@dataclass
class MeshDistance:
    """What ``TsdfVolume.distance`` and ``distance_points`` return: for every query point the nearest point on the
    target mesh.  A point that is not finite has dist NaN, tri 0xffffffff, closest NaN and side 0."""
    dist: np.ndarray               # (n,) float64
    tri: np.ndarray                # (n,) uint32: the nearest triangle of the target, the least index among equally near ones
    closest: np.ndarray            # (n, 3) float64: the nearest point on it
    side: np.ndarray               # (n,) int8: the sign of (p - closest) . n of that triangle: +1 is the free-space side of a weld


@dataclass
class DistanceStats:
    """``TsdfVolume.distance_stats``: the last distance run summed up in a fixed order, over its finite points."""
    n: int                         # the points with a distance
    n_bad: int                     # the others
    max: float                     # the one-sided Hausdorff distance, and the least index that has it
    argmax: int
    mean: float
    rms: float
    within: int                    # the points with dist <= threshold


@dataclass
class FrameAudit:
    """One key frame of ``audit_recording``: the volume rendered at its pose against its filtered depth map and image."""
    id: int
    render: Render
    overlap: float                 # share of the pixels where the render and the filtered map both have depth
    median: float                  # of |render - filtered| / filtered over those pixels (NaN if there are none)
    p90: float                     # its 90th percentile
    grey_error: float              # mean |grey - image| over the pixels the render hit (NaN if there are none)
    colour_error: float = float("nan")        # the mean over those pixels of the mean |channel - image channel|; NaN for grey
    # with ``audit_recording(render="mesh")`` a second FrameAudit: the last mesh of the chain rasterised at the same pose (§30)
    # against the same depth map and image.  An attribute beside the fields, as ``RecordingMesh.normals`` is
    mesh = None


@dataclass
class RecordingAudit:
    mesh: "RecordingMesh"
    frames: list                   # one FrameAudit per key frame, in file order
    z_near: float
    z_far: float
    step: float


@dataclass
class RecordingMesh:
    """What ``mesh_from_recording`` returns: the welded mesh and the grid it was fused on."""
    vertices: np.ndarray           # (m, 3) float64
    faces: np.ndarray              # (n, 3) int64 into vertices
    grey: np.ndarray               # (m,) uint8
    origin: np.ndarray
    dims: tuple
    voxel: float
    trunc: float
    maps: list                     # the DepthMaps that were fused
    colour: Optional[np.ndarray] = None       # (m, 3) uint8, B G R: colour recordings only
    # (m, 3) float32 vertex normals, set by ``normals=True`` only.  An attribute beside the fields, not a field: ``colour`` stays
    # the last positional argument of the constructor
    normals = None
    # the TextureAtlas of ``texture=``, an attribute like ``normals``
    texture = None


class TsdfVolume(capi.Handle):
    """``dims`` = (nx, ny, nz) voxels of side ``voxel`` on the device; the centre of voxel (i, j, k) is origin + (i, j, k) voxel.
    The planes are numpy arrays of shape (nz, ny, nx): x fastest.  ``colour``: a colour volume, which also sums B, G and R."""
    _family = "ekf_fusion"

    def __init__(self, dims, origin, voxel: float, trunc: float, device: int = 0, colour: bool = False):
        nx, ny, nz = (int(v) for v in dims)
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        self._create("ekf_colour_create" if colour else "ekf_fusion_create", nx, ny, nz, _ptr(o), float(voxel),
                     float(trunc), int(device))
        self.colour = bool(colour)
        self.dims, self.origin, self.voxel, self.trunc, self.device = (nx, ny, nz), o, float(voxel), float(trunc), int(device)
        self.shape = (nz, ny, nx)
        self._weld_counts = (0, 0, False)       # vertices, triangles and normals of the last weld
        self.pruned_components = 0              # the number of components the last prune kept
        self._pruned_vertices = 0               # the vertices of the last prune
        self._smooth_vertices = 0               # the vertices of the last smooth
        self._smooth_normals = False            # whether it made normals
        self._simplify_vertices = 0             # the vertices of the source of the last simplify
        self._pruned_triangles = self._smooth_triangles = self._simplify_triangles = 0      # the triangles of the last of each
        self._simplify_cell = 0.0               # the cell of the last simplify
        self.simplify_stats = SimplifyStats(0, 0)
        self._texture = None                    # (triangles, atlas side, channels, source) of the last texture_begin
        self._raster_mesh_colour = False        # whether the last set_raster_mesh gave B, G, R

    def integrate(self, dense_stereo, slot: int, filtered: bool = True):
        """The swept or filtered map of a slot of a ``DenseStereo``, straight from its device buffers."""
        self._check(self._lib.ekf_fusion_integrate(self._h, dense_stereo._h, int(slot), 1 if filtered else 0))

    def integrate_host(self, depth, image, K, pose7):
        """``depth``: (H, W) float32, 0 = none; ``image``: (H, W) uint8, or (H, W, 3) in B, G, R order for a colour volume;
        any size up to 8192 x 8192."""
        d = np.ascontiguousarray(depth, np.float32)
        img = np.ascontiguousarray(image, np.uint8)
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        if d.ndim == 2 and img.shape == d.shape + (3,):
            self._check(self._lib.ekf_colour_integrate_host(self._h, _ptr(d), _ptr(img), img.strides[0], d.shape[1],
                                                                   d.shape[0], _ptr(K), _ptr(pose)))
            return
        if d.ndim != 2 or img.shape != d.shape:
            raise ValueError("depth and image are (H, W) arrays of one shape, or the image is (H, W, 3)")
        self._check(self._lib.ekf_fusion_integrate_host(self._h, _ptr(d), _ptr(img), img.strides[0], d.shape[1], d.shape[0],
                                                        _ptr(K), _ptr(pose)))

    def reset(self):
        self._check(self._lib.ekf_fusion_reset(self._h))

    def volume(self) -> dict:
        """sum float32, cnt uint16, gsum uint32, each (nz, ny, nx), and maps: the number of maps integrated; of a colour
        volume also csum uint32 (3, nz, ny, nx): the sums of B, G and R."""
        out = dict(sum=np.zeros(self.shape, np.float32), cnt=np.zeros(self.shape, np.uint16), gsum=np.zeros(self.shape, np.uint32))
        maps = C.c_int(0)
        self._check(self._lib.ekf_fusion_get_volume(self._h, _ptr(out["sum"]), _ptr(out["cnt"]), _ptr(out["gsum"]), C.byref(maps)))
        out["maps"] = int(maps.value)
        if self.colour:
            out["csum"] = np.zeros((3,) + self.shape, np.uint32)
            self._check(self._lib.ekf_colour_get_volume(self._h, _ptr(out["csum"])))
        return out

    def set_volume(self, sum=None, cnt=None, gsum=None, maps: int = -1, csum=None):
        """Writes the given planes (tests).  ``maps`` = -1 keeps the map counter; it is raised to the largest count given.
        ``csum``: the (3, nz, ny, nx) colour planes of a colour volume."""
        if csum is not None:
            csum = np.ascontiguousarray(csum, np.uint32)
            if csum.shape != (3,) + self.shape:
                raise ValueError("csum is (3, nz, ny, nx) = %r" % ((3,) + self.shape,))
            self._check(self._lib.ekf_colour_set_volume(self._h, _ptr(csum)))
        arrs = []
        for a, t in ((sum, np.float32), (cnt, np.uint16), (gsum, np.uint32)):
            if a is not None:
                a = np.ascontiguousarray(a, t)
                if a.shape != self.shape:
                    raise ValueError("a plane is (nz, ny, nx) = %r" % (self.shape,))
            arrs.append(a)
        self._check(self._lib.ekf_fusion_set_volume(self._h, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), int(maps)))

    def extract(self, min_count: int = 1) -> Mesh:
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_fusion_extract(self._h, int(min_count), C.byref(n)))
        n = int(n.value)
        m = Mesh(np.zeros((n, 3, 3), np.float64), np.zeros((n, 3), np.uint64), np.zeros((n, 3), np.uint8))
        self._check(self._lib.ekf_fusion_get_mesh(self._h, _ptr(m.xyz), _ptr(m.key), _ptr(m.grey), n))
        if self.colour:
            m.colour = np.zeros((n, 3, 3), np.uint8)
            self._check(self._lib.ekf_colour_get_mesh(self._h, _ptr(m.colour), n))
        return m

    def _indexed_mesh(self, getter, nv: int, nt: int, normals: bool) -> IndexedMesh:
        """The arrays of a mesh of ``nv`` vertices and ``nt`` triangles on the device, fetched by one of the three getters."""
        m = IndexedMesh(np.zeros((nv, 3), np.float64), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint8),
                        np.zeros((nv, 3), np.uint8) if self.colour else None, np.zeros((nv, 3), np.float32) if normals else None,
                        np.zeros(nv, np.uint64))
        self._check(getter(self._h, _ptr(m.vertices), _ptr(m.faces), _ptr(m.grey), _ptr(m.colour), _ptr(m.normals), _ptr(m.key), nv, nt))
        return m

    def weld(self, min_count: int = 1, normals: bool = False) -> IndexedMesh:
        """The indexed mesh, welded on the device: ``weld(self.extract(min_count))`` bit for bit, without the
        soup's way over the host and without a sort.  It extracts first unless the handle holds the soup of this
        ``min_count``; ``extract``'s mesh stays valid.  ``normals``: unit vertex normals from the gradient of the mean field.
        The first weld allocates 4 bytes a voxel and 1 byte a cell of scratch on the device."""
        nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.ekf_mesh_weld(self._h, int(min_count), 1 if normals else 0, C.byref(nv), C.byref(nt)))
        nv, nt = int(nv.value), int(nt.value)
        self._weld_counts = (nv, nt, bool(normals))
        return self._indexed_mesh(self._lib.ekf_mesh_get, nv, nt, normals)

    def components(self) -> MeshComponents:
        """The connected components of the last ``weld``, found on the device.  The first call allocates 16 bytes
        a vertex and 4 bytes a triangle of scratch."""
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_components_find(self._h, C.byref(n)))
        nv = self._weld_counts[0]
        out = MeshComponents(np.zeros(nv, np.uint32), np.zeros(nv, np.uint32), int(n.value))
        self._check(self._lib.ekf_components_get(self._h, _ptr(out.label), _ptr(out.size), nv))
        return out

    def prune(self, min_triangles: int = 1, largest: bool = False) -> IndexedMesh:
        """The last ``weld`` without its small components: a component is kept iff it has at least
        ``min_triangles`` triangles and, with ``largest``, is the one of greatest size (the least label among equals).  Vertices
        and triangles keep their order, the kept rows are the weld's bit for bit (normals iff the weld had them), and the faces
        are re-indexed; ``prune(1)`` is the identity.  The components are found first unless the handle holds them for this
        weld; the weld itself stays as it was."""
        nv, nt, nk = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.ekf_components_prune(self._h, int(min_triangles), 1 if largest else 0, C.byref(nv), C.byref(nt), C.byref(nk)))
        nv, nt, normals = int(nv.value), int(nt.value), self._weld_counts[2]
        m = self._indexed_mesh(self._lib.ekf_components_get_pruned, nv, nt, normals)
        self.pruned_components = int(nk.value)
        self._pruned_vertices = nv
        self._pruned_triangles = nt
        return m

    def get_component_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the eight kinds of launch of ``components`` and ``prune`` since the last
        ``profile()``."""
        ms, cnt = np.zeros(8, np.float64), np.zeros(8, np.int64)
        self._check(self._lib.ekf_components_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(COMPONENT_KERNELS)}

    def smooth(self, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, pin_boundary: bool = False,
               normals: bool = False, source: str = "weld") -> IndexedMesh:
        """The last ``weld`` (``source="weld"``) or the last ``prune`` (``"pruned"``) smoothed on the device with Taubin's scheme
        (DESIGN.md §26): ``iterations`` times a step towards the mean of a vertex's neighbours with factor ``lam`` and then,
        unless ``mu`` is 0, one with ``mu`` (Taubin wants ``mu < -lam``, which does not shrink; ``mu=0`` is plain Laplacian
        smoothing).  ``pin_boundary`` keeps the bits of the vertices on an open edge.  ``normals``: unit vertex normals from
        the smoothed triangles, weighted by area; without it the result has none (the weld's describe another surface).
        Faces, grey, colour and key are the source's; the source itself stays as it was.  The adjacency is built by the first
        run on a mesh (13 bytes a vertex and 36 bytes a triangle of scratch) and kept for the next."""
        if source not in ("weld", "pruned"):
            raise ValueError('source is "weld" or "pruned"')
        nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.ekf_smooth_run(self._h, 1 if source == "pruned" else 0, int(iterations), float(lam), float(mu),
                                             1 if pin_boundary else 0, 1 if normals else 0, C.byref(nv), C.byref(nt)))
        nv, nt = int(nv.value), int(nt.value)
        self._smooth_vertices = nv
        self._smooth_triangles = nt
        self._smooth_normals = bool(normals)
        return self._indexed_mesh(self._lib.ekf_smooth_get, nv, nt, normals)

    def adjacency(self) -> MeshAdjacency:
        """The adjacency of the mesh the last ``smooth`` ran on."""
        nv = self._smooth_vertices
        out = MeshAdjacency(np.zeros(nv, np.uint32), np.zeros(nv, np.uint32), np.zeros(nv, np.uint8))
        self._check(self._lib.ekf_smooth_get_adjacency(self._h, _ptr(out.inc), _ptr(out.deg), _ptr(out.boundary), nv))
        return out

    def get_smooth_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the seven kinds of launch of ``smooth`` since the last ``profile()``."""
        ms, cnt = np.zeros(7, np.float64), np.zeros(7, np.int64)
        self._check(self._lib.ekf_smooth_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(SMOOTH_KERNELS)}

    def simplify(self, cell: float, source: str = "weld") -> IndexedMesh:
        """The last ``weld`` (``source="weld"``), the last ``prune`` (``"pruned"``) or the last ``smooth`` (``"smoothed"``)
        simplified on the device by vertex clustering: the vertices that fall into one cell of side ``cell``
        (>= the voxel) of a grid from the volume's origin become one vertex, their mean, with the cell's id as its key; a
        triangle whose vertices share a cell goes, and so does one whose three cells an earlier triangle has; a cell that no
        kept triangle has gives no vertex.  Normals iff the source has them.  ``simplify_stats`` holds the numbers of
        degenerate and duplicate triangles.  The source stays as it was.  Scratch: 20 bytes a cell, 12 a source vertex and 20 a
        source triangle."""
        if source not in SIMPLIFY_SOURCES:
            raise ValueError('source is "weld", "pruned" or "smoothed"')
        nv, nt, nd, nu = (C.c_ulonglong(0) for _ in range(4))
        self._check(self._lib.ekf_simplify_run(self._h, SIMPLIFY_SOURCES[source], float(cell), C.byref(nv), C.byref(nt), C.byref(nd),
                                               C.byref(nu)))
        self.simplify_stats = SimplifyStats(int(nd.value), int(nu.value))
        self._simplify_triangles, self._simplify_cell = int(nt.value), float(cell)
        normals = self._smooth_normals if source == "smoothed" else self._weld_counts[2]
        m = self._indexed_mesh(self._lib.ekf_simplify_get, int(nv.value), int(nt.value), normals)
        # the source's vertices, for simplify_map: a copy of none of them, only their number
        self._simplify_vertices = {"weld": self._weld_counts[0], "pruned": self._pruned_vertices,
                                   "smoothed": self._smooth_vertices}[source]
        return m

    def simplify_map(self) -> np.ndarray:
        """For every vertex of the source of the last ``simplify``, the number of its vertex in the result, or 0xffffffff where
        its cell gave none: (m,) uint32."""
        out = np.zeros(self._simplify_vertices, np.uint32)
        self._check(self._lib.ekf_simplify_get_map(self._h, _ptr(out), len(out)))
        return out

    def get_simplify_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the ten kinds of launch of ``simplify`` since the last ``profile()``."""
        ms, cnt = np.zeros(10, np.float64), np.zeros(10, np.int64)
        self._check(self._lib.ekf_simplify_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(SIMPLIFY_KERNELS)}

    def texture_begin(self, source: str = "weld", patch: int = 8, channels: Optional[int] = None) -> int:
        """Starts a texture atlas of the last ``weld``, ``prune`` (``"pruned"``), ``smooth`` (``"smoothed"``) or
        ``simplify`` (``"simplified"``): every pair of triangles gets a block of ``patch`` + 2 texels a side.  ``channels``: 1 or
        3, by default 3 for a colour volume.  Returns the atlas's side.  Views are then added one at a time; the source is only
        read.  Device memory: the atlas, 13 bytes a triangle and 17 bytes a source vertex."""
        if source not in TEXTURE_SOURCES:
            raise ValueError('source is "weld", "pruned", "smoothed" or "simplified"')
        channels = (3 if self.colour else 1) if channels is None else int(channels)
        side = C.c_int(0)
        self._check(self._lib.ekf_texture_begin(self._h, TEXTURE_SOURCES[source], int(patch), channels, C.byref(side)))
        self._texture = (int(side.value), channels, source)
        return int(side.value)

    def _texture_tol(self, tol):
        """The default of ``tol``: the voxel, and for a simplified source the cell of that run."""
        if tol is not None:
            return float(tol)
        return self._simplify_cell if self._texture and self._texture[2] == "simplified" else self.voxel

    def texture_add_view(self, dense_stereo, slot: int, occlusion=None, tol: Optional[float] = None, min_area2: float = 0.0) -> int:
        """Adds the image, K and pose of a set slot of a ``DenseStereo`` as the next view, straight from its device buffers, and
        returns the number of triangles it won: those it sees whole, from the free-space side and larger (in pixels) than every
        earlier view did.  ``occlusion``: None, or ``(z_near, z_far[, step, min_count])``: the volume is ray-cast at the slot's
        pose first, and a vertex counts as seen only if it lies no more than ``tol`` (default: the voxel; for a simplified
        source its cell) behind that render.  ``min_area2``: twice the least area in pixels a triangle must have."""
        if occlusion is not None:
            self.raycast_view(dense_stereo, slot, *occlusion)
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_texture_add_view(self._h, dense_stereo._h, int(slot), 0 if occlusion is None else 1,
                                                   self._texture_tol(tol), float(min_area2), C.byref(n)))
        return int(n.value)

    def texture_add_view_host(self, image, K, pose7, occlusion=None, tol: Optional[float] = None, min_area2: float = 0.0) -> int:
        """``texture_add_view`` for an image from the host: (H, W) uint8, or (H, W, 3) in B, G, R order."""
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
            raise ValueError("the image is (H, W) or (H, W, 3)")
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        h, w = img.shape[:2]
        if occlusion is not None:
            self.raycast((w, h), K, pose, *occlusion)
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_texture_add_view_host(self._h, _ptr(img), img.strides[0], 3 if img.ndim == 3 else 1, w, h, _ptr(K),
                                                        _ptr(pose), 0 if occlusion is None else 1, self._texture_tol(tol),
                                                        float(min_area2), C.byref(n)))
        return int(n.value)

    def _texture_get(self, n_textured: int) -> "TextureAtlas":
        side, channels, source = self._texture
        nt = {"weld": self._weld_counts[1], "pruned": self._pruned_triangles, "smoothed": self._smooth_triangles,
              "simplified": self._simplify_triangles}[source]
        out = TextureAtlas(np.zeros((side, side) if channels == 1 else (side, side, 3), np.uint8), np.zeros((nt, 3, 2), np.float64),
                           np.zeros(nt, np.int32), np.zeros(nt, np.float64), n_textured)
        self._check(self._lib.ekf_texture_get(self._h, _ptr(out.atlas), side * channels, _ptr(out.uv), _ptr(out.view), _ptr(out.score), nt))
        return out

    def texture_finish(self) -> "TextureAtlas":
        """Fills the triangles that no view won with the blend of their vertices' grey (or B, G, R) and returns the atlas."""
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_texture_finish(self._h, C.byref(n)))
        return self._texture_get(int(n.value))

    def texture_peek(self) -> "TextureAtlas":
        """The atlas as it is now, any time after ``texture_begin`` (``n_textured`` counts the triangles with a view)."""
        if self._texture is None:                            # the library says so: EKF_ERR_STATE with its message
            self._check(self._lib.ekf_texture_get(self._h, None, 0, None, None, None, 0))
            raise ValueError("texture_peek: no texture_begin through this object")
        out = self._texture_get(0)
        out.n_textured = int((out.view >= 0).sum())
        return out

    def get_texture_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the four kinds of launch of the texture since the last ``profile()``."""
        ms, cnt = np.zeros(4, np.float64), np.zeros(4, np.int64)
        self._check(self._lib.ekf_texture_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(TEXTURE_KERNELS)}

    def set_raster_mesh(self, vertices, faces, grey, colour=None):
        """Gives the rasteriser a mesh of the caller's (source ``"mesh"``), for instance one read back with
        ``read_mesh_ply``: ``vertices`` (m, 3) finite, ``faces`` (n, 3) with every index < m, ``grey`` (m,) uint8 and optionally
        ``colour`` (m, 3) uint8 in B, G, R order.  It is copied to buffers of the rasteriser's own."""
        X = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        F = np.asarray(faces).reshape(-1, 3)
        if F.size and (F.min() < 0 or F.max() > 0xFFFFFFFF):
            raise ValueError("a face index is negative or does not fit 32 bits")
        F = np.ascontiguousarray(F, np.uint32)
        g = np.ascontiguousarray(grey, np.uint8).reshape(-1)
        c = None if colour is None else np.ascontiguousarray(colour, np.uint8).reshape(-1, 3)
        if len(g) != len(X) or (c is not None and len(c) != len(X)):
            raise ValueError("grey and colour have one row a vertex")
        self._check(self._lib.ekf_raster_set_mesh(self._h, _ptr(X), _ptr(F), _ptr(g), _ptr(c), len(X), len(F)))
        self._raster_mesh_colour = c is not None

    def _raster_args(self, source, shading):
        if source not in RASTER_SOURCES:
            raise ValueError('source is "weld", "pruned", "smoothed", "simplified" or "mesh"')
        if shading not in RASTER_SHADINGS:
            raise ValueError('shading is "vertex" or "texture"')
        return RASTER_SOURCES[source], RASTER_SHADINGS[shading]

    def _mesh_render(self, source: str, shading: str, cover: bool) -> MeshRender:
        w, h = C.c_int(0), C.c_int(0)
        self._check(self._lib.ekf_raster_get(self._h, None, None, None, None, None, None, None, C.byref(w), C.byref(h)))
        n = (h.value, w.value)
        if shading == "texture":
            colour = self._texture is not None and self._texture[1] == 3
        else:
            colour = self._raster_mesh_colour if source == "mesh" else self.colour
        r = MeshRender(np.zeros(n, np.float32), np.zeros(n + (3,), np.float32), np.zeros(n, np.uint8),
                       np.zeros(n + (3,), np.uint8) if colour else None, np.zeros(n, np.int32), np.zeros(n + (2,), np.float32),
                       np.zeros(n, np.uint32) if cover else None)
        self._check(self._lib.ekf_raster_get(self._h, _ptr(r.depth), _ptr(r.normal), _ptr(r.grey), _ptr(r.colour), _ptr(r.tri),
                                             _ptr(r.bary), _ptr(r.cover), None, None))
        return r

    def rasterise(self, shape, K, pose7, source: str = "weld", z_near: float = 0.0, cull: bool = True, shading: str = "vertex",
                  cover: bool = False) -> MeshRender:
        """The last ``weld``, ``prune`` (``"pruned"``), ``smooth`` (``"smoothed"``) or ``simplify`` (``"simplified"``), or the mesh
        of ``set_raster_mesh`` (``"mesh"``), seen by a pinhole camera of ``shape`` = (width, height) pixels, ``K`` = (fx, fy, cx,
        cy), at ``pose7``: the nearest triangle of every pixel, its depth, its barycentrics, its normal and its
        colour.  A triangle with a vertex at or in front of ``z_near`` is dropped whole; ``cull`` drops the triangles seen from
        behind.  ``shading``: ``"vertex"`` blends the vertex grey (and B, G, R), ``"texture"`` samples the finished texture of
        that source.  ``cover`` also counts the triangles that cover every pixel.  The source is only read."""
        src, shade_ = self._raster_args(source, shading)
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        self._check(self._lib.ekf_raster_render(self._h, src, int(shape[0]), int(shape[1]), _ptr(K), _ptr(pose), float(z_near),
                                                1 if cull else 0, shade_, 1 if cover else 0))
        return self._mesh_render(source, shading, cover)

    def rasterise_view(self, dense_stereo, slot: int, source: str = "weld", z_near: float = 0.0, cull: bool = True,
                       shading: str = "vertex", cover: bool = False) -> MeshRender:
        """``rasterise`` with the size, K and pose of a set slot of a ``DenseStereo``."""
        src, shade_ = self._raster_args(source, shading)
        self._check(self._lib.ekf_raster_render_view(self._h, src, dense_stereo._h, int(slot), float(z_near), 1 if cull else 0,
                                                     shade_, 1 if cover else 0))
        return self._mesh_render(source, shading, cover)

    def set_raster_small_limit(self, limit: int = 16):
        """A triangle whose box on the image has at most ``limit`` pixels (0..65536) is walked by one lane, a larger one by a
        workgroup; the images do not depend on it."""
        self._check(self._lib.ekf_raster_set_small_limit(self._h, int(limit)))

    def get_raster_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the four kinds of launch of the rasteriser since the last ``profile()``."""
        ms, cnt = np.zeros(4, np.float64), np.zeros(4, np.int64)
        self._check(self._lib.ekf_raster_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(RASTER_KERNELS)}

    def set_distance_mesh(self, vertices, faces):
        """Gives the distance a mesh of the caller's (source ``"mesh"``), for instance a ground truth:
        ``vertices`` (m, 3) finite, ``faces`` (n, 3) with every index < m.  It is copied to buffers of the distance's own and is
        independent of ``set_raster_mesh``."""
        X = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        F = np.asarray(faces).reshape(-1, 3)
        if F.size and (F.min() < 0 or F.max() > 0xFFFFFFFF):
            raise ValueError("a face index is negative or does not fit 32 bits")
        F = np.ascontiguousarray(F, np.uint32)
        self._check(self._lib.ekf_distance_set_mesh(self._h, _ptr(X), _ptr(F), len(X), len(F)))

    def _distance_source(self, source):
        if source not in DISTANCE_SOURCES:
            raise ValueError('a source is "weld", "pruned", "smoothed", "simplified" or "mesh"')
        return DISTANCE_SOURCES[source]

    def _distance(self, n: int) -> MeshDistance:
        r = MeshDistance(np.zeros(n, np.float64), np.zeros(n, np.uint32), np.zeros((n, 3), np.float64), np.zeros(n, np.int8))
        self._check(self._lib.ekf_distance_get(self._h, _ptr(r.dist), _ptr(r.tri), _ptr(r.closest), _ptr(r.side), n))
        return r

    def distance(self, target: str = "weld", query: str = "simplified") -> MeshDistance:
        """For every vertex of ``query`` the nearest point on the mesh ``target``: each is the last ``weld``,
        ``prune`` (``"pruned"``), ``smooth`` (``"smoothed"``), ``simplify`` (``"simplified"``) or the mesh of
        ``set_distance_mesh`` (``"mesh"``); they may be the same.  Both are only read."""
        n = C.c_ulonglong(0)
        self._check(self._lib.ekf_distance_run(self._h, self._distance_source(target), self._distance_source(query), C.byref(n)))
        return self._distance(int(n.value))

    def distance_points(self, target: str, points) -> MeshDistance:
        """The same for ``points`` (n, 3) of the caller's, n >= 1."""
        P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self._check(self._lib.ekf_distance_run_points(self._h, self._distance_source(target), _ptr(P), len(P)))
        return self._distance(len(P))

    def distance_stats(self, threshold: float = 0.0) -> DistanceStats:
        """The last ``distance`` or ``distance_points`` summed up: the maximum (the one-sided Hausdorff distance) and where, the
        mean, the RMS and the number of points within ``threshold`` >= 0, in a fixed order of summation."""
        n, bad, arg, within = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        mx, mean, rms = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.ekf_distance_get_stats(self._h, float(threshold), C.byref(n), C.byref(bad), C.byref(mx), C.byref(arg),
                                                     C.byref(mean), C.byref(rms), C.byref(within)))
        return DistanceStats(int(n.value), int(bad.value), mx.value, int(arg.value), mean.value, rms.value, int(within.value))

    def set_distance_grid(self, g: int = 0):
        """The cells of the search grid along the longest axis of the target's box: 1..128, or 0 for the automatic choice; 1 is
        brute force on the device.  The result does not depend on it."""
        self._check(self._lib.ekf_distance_set_grid(self._h, int(g)))

    def distance_grid(self) -> dict:
        """Of the last run, for measurements: the cells along x, y, z, the entries of all cell lists and the longest list."""
        cells, entries, longest = np.zeros(3, np.int32), C.c_ulonglong(0), C.c_uint(0)
        self._check(self._lib.ekf_distance_get_grid(self._h, _ptr(cells), C.byref(entries), C.byref(longest)))
        return dict(cells=tuple(int(c) for c in cells), entries=int(entries.value), longest=int(longest.value))

    def get_distance_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the nine kinds of launch of the distance since the last ``profile()``."""
        ms, cnt = np.zeros(9, np.float64), np.zeros(9, np.int64)
        self._check(self._lib.ekf_distance_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(DISTANCE_KERNELS)}

    def _render(self) -> Render:
        w, h = C.c_int(0), C.c_int(0)
        self._check(self._lib.ekf_raycast_get(self._h, None, None, None, C.byref(w), C.byref(h)))
        r = Render(np.zeros((h.value, w.value), np.float32), np.zeros((h.value, w.value, 3), np.float32),
                   np.zeros((h.value, w.value), np.uint8))
        self._check(self._lib.ekf_raycast_get(self._h, _ptr(r.depth), _ptr(r.normal), _ptr(r.grey), None, None))
        if self.colour:
            r.colour = np.zeros((h.value, w.value, 3), np.uint8)
            self._check(self._lib.ekf_colour_get_render(self._h, _ptr(r.colour)))
        return r

    def raycast(self, shape, K, pose7, z_near: float, z_far: float, step: Optional[float] = None, min_count: int = 1) -> Render:
        """The volume seen by a pinhole camera of ``shape`` = (width, height) pixels, ``K`` = (fx, fy, cx, cy), at ``pose7``:
        samples of the camera-z depth at z_near + n step up to z_far (``step`` None: voxel / 2) over the voxels with at
        least ``min_count`` maps.  The mesh of the last ``extract`` stays valid."""
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        pose = np.ascontiguousarray(pose7, np.float64).reshape(7)
        step = self.voxel / 2.0 if step is None else float(step)
        self._check(self._lib.ekf_raycast_render(self._h, int(shape[0]), int(shape[1]), _ptr(K), _ptr(pose), float(z_near),
                                                 float(z_far), step, int(min_count)))
        return self._render()

    def raycast_view(self, dense_stereo, slot: int, z_near: float, z_far: float, step: Optional[float] = None,
                     min_count: int = 1) -> Render:
        """``raycast`` with the size, K and pose of a set slot of a ``DenseStereo``."""
        step = self.voxel / 2.0 if step is None else float(step)
        self._check(self._lib.ekf_raycast_render_view(self._h, dense_stereo._h, int(slot), float(z_near), float(z_far), step,
                                                      int(min_count)))
        return self._render()

    def profile(self, enable: bool = True):
        self._check(self._lib.ekf_fusion_profile(self._h, 1 if enable else 0))

    def get_raycast_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of k_tsdf_mean and k_tsdf_raycast since the last ``profile()``."""
        ms, cnt = np.zeros(2, np.float64), np.zeros(2, np.int64)
        self._check(self._lib.ekf_raycast_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(RAYCAST_KERNELS)}

    def get_colour_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the three colour kernels since the last ``profile()``."""
        ms, cnt = np.zeros(3, np.float64), np.zeros(3, np.int64)
        self._check(self._lib.ekf_colour_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(COLOUR_KERNELS)}

    def get_mesh_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the five launches of a weld since the last ``profile()``."""
        ms, cnt = np.zeros(5, np.float64), np.zeros(5, np.int64)
        self._check(self._lib.ekf_mesh_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(MESH_KERNELS)}

    def get_profile(self) -> dict:
        """HIP-event milliseconds and launch counts of the four kernels since the last ``profile()``."""
        ms, cnt = np.zeros(4, np.float64), np.zeros(4, np.int64)
        self._check(self._lib.ekf_fusion_get_profile(self._h, _ptr(ms), _ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(KERNELS)}


def weld(mesh: Mesh, colour: bool = False):
    """(vertices (m, 3) float64, faces (n, 3) int64, grey (m,) uint8): one vertex per distinct key (ascending), exact because
    equal keys carry bit-equal coordinates.  ``colour``: a fourth array, (m, 3) uint8 in B, G, R order (equal keys carry
    equal colours too: a colour is a function of the key)."""
    _, first, inverse = np.unique(mesh.key.reshape(-1), return_index=True, return_inverse=True)
    out = mesh.xyz.reshape(-1, 3)[first], inverse.reshape(-1, 3).astype(np.int64), mesh.grey.reshape(-1)[first]
    if not colour:
        return out
    if mesh.colour is None:
        raise ValueError("the mesh has no colour: it was not extracted from a colour volume")
    return out + (mesh.colour.reshape(-1, 3)[first],)


def write_mesh_ply(path: str, vertices, faces, grey, colour=None, normals=None) -> None:
    """ASCII PLY: vertices ``x y z`` as doubles with ``intensity``, faces as ``list uchar int vertex_indices``.  ``colour``
    ((m, 3), B, G, R) adds ``red green blue`` after the intensity; ``normals`` ((m, 3) float32) adds ``nx ny nz`` as the last
    vertex properties, written with ``%.9g`` (which a float32 survives)."""
    rgb = "" if colour is None else "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    if normals is not None:
        rgb += "property float nx\nproperty float ny\nproperty float nz\n"
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                 "property uchar intensity\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(vertices), rgb, len(faces)))
        tail = [""] * len(vertices) if normals is None else [" %.9g %.9g %.9g" % (float(a), float(b), float(c)) for a, b, c in normals]
        if colour is None:
            for (x, y, z), g, t in zip(vertices, grey, tail):
                fh.write("%.17g %.17g %.17g %d%s\n" % (x, y, z, int(g), t))
        else:
            for (x, y, z), g, (b, gr, r), t in zip(vertices, grey, colour, tail):
                fh.write("%.17g %.17g %.17g %d %d %d %d%s\n" % (x, y, z, int(g), int(r), int(gr), int(b), t))
        for a, b, c in faces:
            fh.write("3 %d %d %d\n" % (a, b, c))


def read_mesh_ply(path: str, colour: bool = False, normals: bool = False):
    """What ``write_mesh_ply`` wrote: (vertices (m, 3) float64, faces (n, 3) int64, grey (m,) uint8), with ``colour`` the
    (m, 3) uint8 colours swapped back to B, G, R order, and with ``normals`` the (m, 3) float32 normals last."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    end = lines.index("end_header")
    count = lambda what: int([ln for ln in lines[:end] if ln.startswith("element " + what)][0].split()[2])
    nv, nf = count("vertex"), count("face")
    rows = [ln.split() for ln in lines[end + 1:end + 1 + nv]]
    faces = [ln.split() for ln in lines[end + 1 + nv:end + 1 + nv + nf]]
    out = (np.array([[float(t) for t in r[:3]] for r in rows], np.float64).reshape(-1, 3),
           np.array([[int(t) for t in r[1:4]] for r in faces], np.int64).reshape(-1, 3),
           np.array([int(r[3]) for r in rows], np.uint8))
    has_colour = "property uchar red" in lines[:end]
    if colour:
        if not has_colour:
            raise ValueError("%s has no colour" % path)
        out += (np.array([[int(r[6]), int(r[5]), int(r[4])] for r in rows], np.uint8).reshape(-1, 3),)
    if normals:
        if "property float nx" not in lines[:end]:
            raise ValueError("%s has no normals" % path)
        at = 7 if has_colour else 4
        out += (np.array([[float(t) for t in r[at:at + 3]] for r in rows], np.float64).astype(np.float32).reshape(-1, 3),)
    return out


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path: str, image) -> None:
    """An 8-bit PNG of an (H, W) grey or an (H, W, 3) B, G, R image, with the standard library's ``zlib``: filter 0 on every row."""
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim == 3:
        img = np.ascontiguousarray(img[:, :, ::-1])
    h, w = img.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, -1)], axis=1)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if img.ndim == 2 else 2, 0, 0, 0)) +
                 _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """An 8-bit grey or RGB PNG without interlace as (H, W) or (H, W, 3) uint8 in B, G, R order: what ``write_png`` wrote, and
    any of the five row filters."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s is no PNG" % path)
    at, idat, head = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError("%s: a chunk's CRC is wrong" % path)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    if head is None or head[2] != 8 or head[3] not in (0, 2) or head[6] != 0:
        raise ValueError("%s: only 8-bit grey or RGB without interlace" % path)
    w, h, c = head[0], head[1], 1 if head[3] == 0 else 3
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
    out = np.zeros((h, w * c), np.uint8)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1].astype(np.int64) if y else np.zeros(w * c, np.int64)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) & 255
        else:                                                # 1, 3, 4 need the pixel to the left: byte by byte
            cur = np.zeros(w * c, np.int64)
            for i in range(w * c):
                a = cur[i - c] if i >= c else 0
                b, cc = up[i], (up[i - c] if i >= c else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                elif f == 4:
                    pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
                else:
                    raise ValueError("%s: row filter %d" % (path, f))
                cur[i] = (line[i] + pred) & 255
            out[y] = cur
    return out.reshape(h, w) if c == 1 else np.ascontiguousarray(out.reshape(h, w, 3)[:, :, ::-1])


def write_mesh_obj(path: str, vertices, faces, atlas: TextureAtlas) -> None:
    """Wavefront OBJ of a mesh with its ``TextureAtlas``: ``path`` itself (``v`` with ``%.17g``, three ``vt`` a triangle that
    carry u and 1 - v, since OBJ measures v from the bottom row, ``f`` lines of ``v/vt``), beside it a ``.mtl`` that names the
    atlas as ``map_Kd`` and the atlas as an 8-bit ``.png``."""
    base = os.path.splitext(path)[0]
    name = os.path.basename(base)
    faces = np.asarray(faces).reshape(-1, 3)
    if len(atlas.uv) != len(faces):
        raise ValueError("the atlas is of %d triangles, the mesh has %d" % (len(atlas.uv), len(faces)))
    write_png(base + ".png", atlas.atlas)
    with open(base + ".mtl", "w") as fh:
        fh.write("newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd %s.png\n" % (name, name))
    with open(path, "w") as fh:
        fh.write("mtllib %s.mtl\nusemtl %s\n" % (name, name))
        for x, y, z in np.asarray(vertices, np.float64).reshape(-1, 3):
            fh.write("v %.17g %.17g %.17g\n" % (x, y, z))
        for u, v in np.asarray(atlas.uv, np.float64).reshape(-1, 2):
            fh.write("vt %.17g %.17g\n" % (u, 1.0 - v))
        for t, (a, b, c) in enumerate(faces):
            fh.write("f %d/%d %d/%d %d/%d\n" % (a + 1, 3 * t + 1, b + 1, 3 * t + 2, c + 1, 3 * t + 3))


def auto_grid(points, voxel: Optional[float] = None, bounds=None, trunc: Optional[float] = None):
    """(origin, dims, voxel, trunc) of ``mesh_from_recording``.  The box is ``bounds`` = (lo, hi), or the
    box of all finite ``points`` padded by trunc; voxel = its longest side before the padding / 128, doubled until the
    limits of a volume hold; trunc = 4 voxel; a side of n = ceil(extent / voxel) + 1 >= 2 voxels."""
    if bounds is None:
        pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in points])
        pts = pts[np.isfinite(pts).all(axis=1)]
        if not len(pts):
            raise ValueError("no depth map has a point: nothing to bound the volume with")
        lo, hi = pts.min(axis=0), pts.max(axis=0)
    else:
        lo, hi = np.asarray(bounds[0], np.float64).reshape(3), np.asarray(bounds[1], np.float64).reshape(3)
    auto = voxel is None
    vx = np.float64((hi - lo).max()) / 128.0 if auto else np.float64(voxel)
    if not (np.isfinite(vx) and vx > 0.0):
        raise ValueError("the box has no extent")
    while True:
        tr = 4.0 * vx if trunc is None else np.float64(trunc)
        a, b = (lo - tr, hi + tr) if bounds is None else (lo, hi)
        dims = np.maximum(np.ceil((b - a) / vx).astype(np.int64) + 1, 2)
        if dims.max() <= MAX_DIM and int(dims[0]) * int(dims[1]) * int(dims[2]) <= MAX_VOXELS:
            return a, tuple(int(v) for v in dims), float(vx), float(tr)
        if not auto:
            raise ValueError("the volume exceeds 1024 voxels a side or 2^28 in all")
        vx = vx * 2.0


def _fuse_recording(directory, nodes_out, voxel, bounds, trunc, sweep_kwargs):
    """The steps of ``mesh_from_recording`` up to the filled volume: (vol, maps, K, images, origin, dims, voxel, trunc).  A
    recording with colour key frames fills a colour volume."""
    maps = dense.depth_maps_from_recording(directory, nodes_out, **sweep_kwargs)
    K, ids, poses, images = dense.read_recording(directory, nodes_out)
    origin, dims, vx, tr = auto_grid([m.points for m in maps], voxel, bounds, trunc)
    vol = TsdfVolume(dims, origin, vx, tr, int(sweep_kwargs.get("device", 0)), colour=any(img.ndim == 3 for img in images))
    try:
        for m, img in zip(maps, images):
            vol.integrate_host(m.depth, img, K, m.pose)
    except Exception:
        vol.close()
        raise
    return vol, maps, K, images, origin, dims, vx, tr


def mesh_from_recording(directory: str, nodes_out: Optional[str] = None, voxel: Optional[float] = None, bounds=None,
                        trunc: Optional[float] = None, min_count: int = 2, sweep_trunc: Optional[int] = None,
                        weld: str = "host", normals: bool = False, components=None, smooth=None, simplify=None, texture=None,
                        **sweep_kwargs) -> RecordingMesh:
    """``dense.depth_maps_from_recording(directory, nodes_out, **sweep_kwargs)``, then every filtered map with its key
    frame's image into one volume (``auto_grid`` where voxel / bounds / trunc are None), extract, weld.  ``trunc`` is the
    truncation distance of the volume; the sweep's cost truncation, also called ``trunc`` there, is ``sweep_trunc`` here.
    ``sgm=True`` (or a dict of ``p1`` / ``p2`` / ``paths``) among ``sweep_kwargs`` sweeps with semi-global aggregation
    (DESIGN.md §19), for recordings with textureless surfaces; ``cost="census"`` sweeps with the census matching cost
    (§20), for recordings whose key frames differ in exposure or gain; ``best=n`` keeps the n cheapest sources per pixel and
    plane (§21), for neighbours that do not all see every pixel of a key frame; ``uniqueness=u`` (per cent) also drops the
    pixels whose runner-up cost is within u % of the winner's (§22), for recordings with untextured surfaces;
    ``speckle=min_size`` or ``speckle=(min_size, max_diff)`` then drops from every filtered map the connected segments of fewer
    than ``min_size`` pixels (§23), the islands that would become floating fragments of the mesh.  ``weld="device"`` welds on
    the device (§24): the same arrays without the soup's way over the host; ``normals=True`` does so too and fills
    ``RecordingMesh.normals``.  ``components=n`` drops the connected components of the mesh of fewer than ``n`` triangles and
    ``components="largest"`` keeps the largest one alone (§25); either welds on the device, and ``None`` makes today's
    launches.  ``smooth=n`` then smooths the mesh (the pruned one, if ``components`` is given) with ``n`` rounds of
    ``TsdfVolume.smooth`` at its defaults, and ``smooth=dict(...)`` with those keyword arguments (§26); it welds on the device
    too, with ``normals=True`` the normals are the smoothed mesh's own, and ``None`` makes today's launches.  ``simplify=f`` (a
    float >= 1) is applied last, after ``components`` and ``smooth``: ``TsdfVolume.simplify`` of that mesh with cells of
    ``f`` voxels (§28); it welds on the device too, and ``None`` makes today's launches.  ``texture=P`` (an int, the patch size)
    or ``texture=dict(patch=, channels=, tol=, min_area2=, occlusion=)`` then textures that mesh (§29): every key frame's image
    is added in recording order with ``K`` and the pose of its map, behind a ray cast of the volume over ``audit_range`` unless
    ``occlusion=False``, and the ``TextureAtlas`` lands in ``RecordingMesh.texture``; it welds on the device too, and ``None``
    makes today's launches."""
    _weld_mode(weld, components)
    smooth = _smooth_kwargs(smooth)
    simplify = _simplify_factor(simplify)
    texture = _texture_kwargs(texture)
    if sweep_trunc is not None:
        sweep_kwargs["trunc"] = sweep_trunc
    vol, maps, K, images, origin, dims, vx, tr = _fuse_recording(directory, nodes_out, voxel, bounds, trunc, sweep_kwargs)
    try:
        welded = _welded(vol, min_count, weld, normals, components, smooth, simplify, texture is not None)
        atlas = _textured(vol, texture, _last_source(components, smooth, simplify), maps, images, K, tr, min_count)
    finally:
        vol.close()
    out = RecordingMesh(*welded[:3], origin, dims, vx, tr, maps, welded[3])
    out.normals = welded[4]
    out.texture = atlas
    return out


def _weld_mode(mode, components=None):
    if mode not in ("host", "device"):
        raise ValueError('weld is "host" or "device"')
    if not (components is None or components == "largest" or (isinstance(components, (int, np.integer)) and
                                                              not isinstance(components, bool) and components >= 1)):
        raise ValueError('components is None, an int >= 1 or "largest"')


def _smooth_kwargs(smooth):
    """The keyword arguments of ``TsdfVolume.smooth`` that ``smooth=`` of ``mesh_from_recording`` stands for, or None."""
    if smooth is None:
        return None
    if isinstance(smooth, dict):
        if not set(smooth) <= {"iterations", "lam", "mu", "pin_boundary"}:
            raise ValueError("smooth takes iterations, lam, mu and pin_boundary")
        return dict(smooth)
    if isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool) and smooth >= 1:
        return dict(iterations=int(smooth))
    raise ValueError("smooth is None, an int >= 1 or a dict of keyword arguments of TsdfVolume.smooth")


def _simplify_factor(simplify):
    """The cell size in voxels that ``simplify=`` of ``mesh_from_recording`` stands for, or None."""
    if simplify is None:
        return None
    if isinstance(simplify, (int, float, np.integer, np.floating)) and not isinstance(simplify, bool) and np.isfinite(simplify) \
            and simplify >= 1:
        return float(simplify)
    raise ValueError("simplify is None or a finite number >= 1: the side of a cell in voxels")


def _texture_kwargs(texture):
    """What ``texture=`` of ``mesh_from_recording`` stands for: a dict of patch, channels, tol, min_area2 and occlusion, or None."""
    if texture is None:
        return None
    out = dict(patch=8, channels=None, tol=None, min_area2=0.0, occlusion=True)
    if isinstance(texture, dict):
        if not set(texture) <= set(out):
            raise ValueError("texture takes patch, channels, tol, min_area2 and occlusion")
        out.update(texture)
        return out
    if isinstance(texture, (int, np.integer)) and not isinstance(texture, bool) and 2 <= texture <= 32:
        out["patch"] = int(texture)
        return out
    raise ValueError("texture is None, a patch size 2..32 or a dict of patch, channels, tol, min_area2 and occlusion")


def _last_source(components, smooth, simplify) -> str:
    """The name of the mesh ``_welded`` returned on the device path."""
    return "simplified" if simplify is not None else "smoothed" if smooth is not None else "pruned" if components is not None else "weld"


def _textured(vol: TsdfVolume, texture, source: str, maps, images, K, trunc: float, min_count: int):
    """The ``TextureAtlas`` of the mesh ``_welded`` has just made from every key frame in recording order, or None."""
    if texture is None:
        return None
    vol.texture_begin(source, texture["patch"], texture["channels"])
    occlusion = audit_range(maps, trunc) + (None, min_count) if texture["occlusion"] else None
    for m, img in zip(maps, images):
        vol.texture_add_view_host(img, K, m.pose, occlusion, texture["tol"], texture["min_area2"])
    return vol.texture_finish()


def _welded(vol: TsdfVolume, min_count: int, mode: str = "host", normals: bool = False, components=None, smooth=None,
            simplify=None, device: bool = False):
    """(vertices, faces, grey, colour or None, normals or None) of the volume's mesh.  ``smooth``: what ``_smooth_kwargs`` gave;
    ``simplify``: what ``_simplify_factor`` gave; ``device``: weld on the device whatever ``mode`` says."""
    if mode == "device" or device or normals or components is not None or smooth is not None or simplify is not None:
        m = vol.weld(min_count, normals and smooth is None)
        source = "weld"
        if components is not None:
            m = vol.prune(largest=True) if components == "largest" else vol.prune(int(components))
            source = "pruned"
        if smooth is not None:
            m = vol.smooth(normals=normals, source=source, **smooth)
            source = "smoothed"
        if simplify is not None:
            m = vol.simplify(simplify * vol.voxel, source)
        return m.vertices, m.faces.astype(np.int64), m.grey, m.colour, m.normals
    mesh = vol.extract(min_count)
    return (weld(mesh, True) if vol.colour else weld(mesh) + (None,)) + (None,)


def compare_meshes(vol: TsdfVolume, a: str, b: str, threshold: float = 0.0):
    """Both one-sided distances between two meshes of a volume: the ``DistanceStats`` of the vertices of ``a``
    against ``b`` and of the vertices of ``b`` against ``a``, and the symmetric maximum over vertices (the larger of the two
    one-sided Hausdorff distances)."""
    vol.distance(b, a)
    ab = vol.distance_stats(threshold)
    vol.distance(a, b)
    ba = vol.distance_stats(threshold)
    return ab, ba, max(ab.max, ba.max)


def shade(render: Render, light=(0.0, 0.0, -1.0), albedo: bool = False) -> np.ndarray:
    """An 8-bit Lambert image of a render, on the host: floor(255 max(0, n . l / |l|) + 0.5) where the render has depth, 0
    elsewhere.  ``light`` is the direction towards the light in the world frame.  ``albedo``: the (H, W, 3) picture
    floor(colour max(0, n . l / |l|) + 0.5) of a colour render."""
    l = np.asarray(light, np.float64).reshape(3)
    l = l / np.sqrt(l @ l)
    lam = np.maximum(render.normal.astype(np.float64) @ l, 0.0)
    if albedo:
        if render.colour is None:
            raise ValueError("the render has no colour: it was not made from a colour volume")
        lit = np.floor(render.colour.astype(np.float64) * lam[:, :, None] + 0.5)
        return np.where((render.depth > 0)[:, :, None], lit, 0.0).astype(np.uint8)
    return np.where(render.depth > 0, np.floor(255.0 * lam + 0.5), 0.0).astype(np.uint8)


def audit_range(maps, trunc: float):
    """(z_near, z_far) of ``audit_recording``: the smallest and largest depth of the filtered maps, widened by trunc."""
    z = np.concatenate([m.depth[m.depth > 0].astype(np.float64) for m in maps])
    if not len(z):
        raise ValueError("no depth map has a depth: nothing to render")
    return max(0.0, float(z.min()) - float(trunc)), float(z.max()) + float(trunc)


def audit_frame(kid: int, render: Render, depth, image) -> FrameAudit:
    """The figures of one key frame from its render, its filtered depth map and its image ((H, W), or (H, W, 3) in B, G, R
    order with a colour render: the grey error is then taken against ``grey_image`` of it)."""
    both = (render.depth > 0) & (depth > 0)
    hit = render.depth > 0
    rel = np.abs(render.depth[both].astype(np.float64) - depth[both].astype(np.float64)) / depth[both].astype(np.float64)
    nan = float("nan")
    image = np.asarray(image)
    grey = grey_image(image) if image.ndim == 3 else image
    colour_error = nan
    if image.ndim == 3 and render.colour is not None and hit.any():
        colour_error = float(np.abs(render.colour[hit].astype(np.float64) - image[hit].astype(np.float64)).mean(axis=1).mean())
    return FrameAudit(int(kid), render, float(both.mean()), float(np.median(rel)) if len(rel) else nan,
                      float(np.percentile(rel, 90)) if len(rel) else nan,
                      float(np.abs(render.grey[hit].astype(np.float64) - grey[hit].astype(np.float64)).mean()) if hit.any() else nan,
                      colour_error)


def grey_image(bgr) -> np.ndarray:
    """(H, W) uint8 from a (H, W, 3) B, G, R image: (b 1868 + g 9617 + r 4899 + 8192) >> 14, the library's conversion on the
    host, for the audit.  It must track ``bgr2gray`` of ``csrc/ekf_pixel.hpp``; ``tests/test_oracle_colour.py`` holds it against
    the oracle."""
    a = np.asarray(bgr, np.uint8).astype(np.uint32)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def audit_recording(directory: str, nodes_out: Optional[str] = None, voxel: Optional[float] = None, bounds=None,
                    trunc: Optional[float] = None, min_count: int = 2, sweep_trunc: Optional[int] = None,
                    weld: str = "host", normals: bool = False, components=None, smooth=None, simplify=None, texture=None,
                    render: Optional[str] = None, **sweep_kwargs) -> RecordingAudit:
    """``mesh_from_recording`` with the same arguments, then the volume rendered at every key frame's pose with the
    recording's camera (samples voxel / 2 apart over ``audit_range``, the mesh's ``min_count``) and compared with that key
    frame's filtered depth map and image: the only end-to-end check that needs no ground truth.  ``sgm=…``, ``cost=…``, ``best=…``,
    ``uniqueness=…`` and ``speckle=…`` reach the sweep and the filters, and ``weld=…``, ``normals=…``, ``components=…``, ``smooth=…``
    ``simplify=…`` and ``texture=…`` the mesh, as they do through ``mesh_from_recording``.  ``render="mesh"`` also rasterises the
    last mesh of the chain at every key frame's pose (§30; z_near 0, culling on, ``shading="texture"`` when ``texture=`` was given
    and ``"vertex"`` otherwise) and puts the ``FrameAudit`` of that image against the same depth map and image into the frame's
    ``mesh`` attribute: the check that sees the mesh itself.  It welds on the device too; ``None`` makes today's launches."""
    if render not in (None, "mesh"):
        raise ValueError('render is None or "mesh"')
    _weld_mode(weld, components)
    smooth = _smooth_kwargs(smooth)
    simplify = _simplify_factor(simplify)
    texture = _texture_kwargs(texture)
    if sweep_trunc is not None:
        sweep_kwargs["trunc"] = sweep_trunc
    vol, maps, K, images, origin, dims, vx, tr = _fuse_recording(directory, nodes_out, voxel, bounds, trunc, sweep_kwargs)
    try:
        vertices, faces, grey, colour, vertex_normals = _welded(vol, min_count, weld, normals, components, smooth, simplify,
                                                                texture is not None or render is not None)
        source = _last_source(components, smooth, simplify)
        atlas = _textured(vol, texture, source, maps, images, K, tr, min_count)
        z_near, z_far = audit_range(maps, tr)
        h, w = images[0].shape[:2]
        frames = [audit_frame(m.id, vol.raycast((w, h), K, m.pose, z_near, z_far, None, min_count), m.depth, img)
                  for m, img in zip(maps, images)]
        if render is not None:
            for fr, m, img in zip(frames, maps, images):
                fr.mesh = audit_frame(m.id, vol.rasterise((w, h), K, m.pose, source, 0.0, True, "vertex" if texture is None else "texture"),
                                      m.depth, img)
    finally:
        vol.close()
    mesh = RecordingMesh(vertices, faces, grey, origin, dims, vx, tr, maps, colour)
    mesh.normals = vertex_normals
    mesh.texture = atlas
    return RecordingAudit(mesh, frames, z_near, z_far, vx / 2.0)
