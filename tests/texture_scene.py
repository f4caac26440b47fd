"""Meshes, views and one volume shared by tests/test_oracle_texture.py, tests/test_gpu_texture.py and
tools/texture_host_check.py; tests/component_scene.py, tests/raycast_scene.py and tests/colour_scene.py are
imported read-only.

The views are raycast_scene's poses A, B and AWAY at its 29 x 23 sphere shape with colour_scene's pattern images.  ``AXES`` are
six cameras on the axes, four units from the origin and looking at it: every triangle of the sphere's weld faces one of them.

The occlusion volume holds two flat sheets one behind the other, both facing a camera at the world's origin that looks along
+z: a small front sheet (voxels 3..8 x 2..7 of the layers 0..3, the rest of those layers has no count) and a back sheet over the
whole of the layers 5..8; layer 4 has no count, so that no triangle joins them.  Seen without a z-buffer the camera wins the
triangles of the back sheet that lie behind the front one; with the ray cast of the volume as z-buffer it does not.
"""
import functools

import numpy as np

import colour_scene as col
import component_scene as cs
import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import raycast_oracle as ro
import raycast_scene as rsc
import simplify_oracle as so

W, H = rsc.SPHERE_SHAPE
K = rsc.SPHERE_K
POSES = (rsc.POSE_A, rsc.POSE_B, rsc.AWAY)
_S = np.sqrt(0.5)
AXES = (np.array([0.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 0.0]),
        np.array([4.0, 0.0, 0.0, _S, 0.0, -_S, 0.0]), np.array([-4.0, 0.0, 0.0, _S, 0.0, _S, 0.0]),
        np.array([0.0, 4.0, 0.0, _S, _S, 0.0, 0.0]), np.array([0.0, -4.0, 0.0, _S, -_S, 0.0, 0.0]))


def views(colour=True, poses=POSES, **more):
    """One view a pose with pattern image n (its channel 0 for a grey view)."""
    out = []
    for n, pose in enumerate(poses):
        img = col.pattern(W, H, n)
        out.append(dict(image=img if colour else np.ascontiguousarray(img[:, :, 0]), K=K, pose=pose, **more))
    return out


def main_views(colour=True, **more):
    """The main volume of component_scene seen from the three poses it was fused from, at raycast_scene's main shape."""
    w, h = rsc.MAIN_SHAPE
    out = []
    for n, pose in enumerate(fs.POSES):
        img = col.pattern(w, h, n + 5)
        out.append(dict(image=img if colour else np.ascontiguousarray(img[:, :, 2]), K=fs.K_MAP, pose=pose, **more))
    return out


def constant_views(values, poses=POSES):
    return [dict(image=np.full((H, W), v, np.uint8), K=K, pose=pose) for v, pose in zip(values, poses)]


@functools.lru_cache(maxsize=None)
def simplified(name, mc, factor):
    """The weld of a case of component_scene simplified at ``factor`` voxels, as a mesh: computed once, shared, left unchanged."""
    _, dims, origin, voxel, _, _ = cs.cases()[name]
    return so.as_mesh(so.simplify(cs.oracle_mesh(name, mc), origin, dims, voxel, factor * voxel))


# ---- the occlusion volume ----------------------------------------------------------------------------------------------------
OCC_DIMS = (12, 10, 9)
OCC_ORIGIN = np.array([-0.55, -0.45, 1.0], np.float64)
OCC_VOXEL, OCC_TRUNC = 0.1, 0.4
OCC_SHAPE = (32, 24)
OCC_K = np.array([30.0, 30.0, 15.5, 11.5], np.float64)
OCC_POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], np.float64)
OCC_NEAR, OCC_FAR = 0.5, 2.5


def occlusion_volume():
    """(sum, cnt, gsum) of shape (nz, ny, nx)."""
    nx, ny, nz = OCC_DIMS
    s = np.zeros((nz, ny, nx), np.float32)
    c = np.zeros((nz, ny, nx), np.uint16)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    sign = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 1.0, 1.0, -1.0, -1.0], np.float32)
    s[:] = sign[:, None, None]
    c[5:] = 1
    c[:4, 2:8, 3:9] = 1
    s[c == 0] = 0.0
    g = (((i * 7 + j * 13 + k * 29) % 256) * c).astype(np.uint32)
    return s, c, g


@functools.lru_cache(maxsize=None)
def occlusion_mesh():
    vol = occlusion_volume()
    _, soup_key, _, _ = fo.extract(vol, OCC_DIMS, OCC_ORIGIN, OCC_VOXEL, 1)
    return mo.weld(vol, OCC_DIMS, OCC_ORIGIN, OCC_VOXEL, soup_key, 1, False)


@functools.lru_cache(maxsize=None)
def occlusion_depth():
    """The ray cast of the volume at the camera: the z-buffer.  Samples half a voxel apart, as the wrappers render."""
    return ro.raycast(occlusion_volume(), OCC_DIMS, OCC_ORIGIN, OCC_VOXEL, OCC_SHAPE, OCC_K, OCC_POSE, OCC_NEAR, OCC_FAR,
                      OCC_VOXEL / 2.0, 1)["depth"]


def occlusion_view(occluded):
    w, h = OCC_SHAPE
    v = dict(image=np.ascontiguousarray(col.pattern(w, h, 3)[:, :, 1]), K=OCC_K, pose=OCC_POSE)
    if occluded:
        v.update(zbuf=occlusion_depth(), tol=OCC_VOXEL)
    return v


# ---- one triangle: a hand-set 3 x 3 x 2 volume whose weld of 36 triangles keeps exactly one at cells of 1.5 voxels --------------
ONE_DIMS, ONE_ORIGIN, ONE_VOXEL, ONE_TRUNC, ONE_FACTOR = (3, 3, 2), np.zeros(3, np.float64), 0.1, 0.4, 1.5
ONE_POSE = np.array([0.1, 0.1, 1.0, 0.0, 0.0, 1.0, 0.0], np.float64)        # from +z, half a turn about y: the triangle faces it
ONE_BEHIND = np.array([0.1, 0.1, -1.0, 1.0, 0.0, 0.0, 0.0], np.float64)     # from -z: it sees the triangle's back


def one_triangle_volume():
    s = np.array([[[1.0, 1.0, 1.0], [1.0, -0.25, -1.0], [-1.0, -1.0, -0.25]],
                  [[1.0, 1.0, -0.25], [1.0, -1.0, -1.0], [-0.25, 1.0, 0.5]]], np.float32)
    return s, np.ones(s.shape, np.uint16), np.full(s.shape, 100, np.uint32) + np.arange(18, dtype=np.uint32).reshape(s.shape) * 7


@functools.lru_cache(maxsize=None)
def one_triangle_mesh():
    vol = one_triangle_volume()
    _, soup_key, _, _ = fo.extract(vol, ONE_DIMS, ONE_ORIGIN, ONE_VOXEL, 1)
    weld = mo.weld(vol, ONE_DIMS, ONE_ORIGIN, ONE_VOXEL, soup_key, 1, False)
    return so.as_mesh(so.simplify(weld, ONE_ORIGIN, ONE_DIMS, ONE_VOXEL, ONE_FACTOR * ONE_VOXEL))


# ---- mesh_from_recording(texture=...) restated on the oracle -------------------------------------------------------------------
def oracle_texture_of_audit(texture_oracle, audit, K, images, patch, channels, occlusion=True, tol=None, min_area2=0.0):
    """What ``audit_recording(texture=...)`` must have put into ``audit.mesh.texture``: the oracle on the mesh it returned, with
    every key frame's image, ``K`` and the pose of its map in recording order, behind the render of that key frame (the audit
    renders every key frame with the ray cast the texture used as z-buffer: the same size, camera, pose, range, step and
    min_count)."""
    m = audit.mesh
    mesh = dict(vertices=m.vertices, faces=m.faces, grey=m.grey, colour=m.colour)
    views = []
    for dm, img, fr in zip(m.maps, images, audit.frames):
        v = dict(image=img, K=K, pose=dm.pose, min_area2=min_area2)
        if occlusion:
            v.update(zbuf=fr.render.depth, tol=m.voxel if tol is None else tol)
        views.append(v)
    return texture_oracle.texture(mesh, patch, channels, views)
