"""Volumes shared by tests/test_oracle_components.py, tests/test_gpu_components.py and tools/component_host_check.py (DESIGN.md
§25.5); tests/mesh_scene.py and tests/fusion_scene.py are imported read-only.

Beside the volumes of §24.5, whose meshes hold fragments (the main volume: components of 262, 8 and 2 triangles at min_count 1;
the wave volumes: 58 components at 257 x 2 x 2, 46 at 41 x 41 x 41 with min_count 2), two made for this contract:
  - ``sheets((9, 8, 10))``: four parallel sheets of exactly 448 triangles each, labels 0, 255, 510 and 765: a four-way tie,
    of which ``largest`` must keep label 0;
  - ``sheets((129, 129, 3))``: one sheet, one component of 131 072 triangles and 66 049 vertices: 512 triangle workgroups and
    259 vertex blocks, the last of one vertex, so k_tsdf_scan's chunk is 2 for both, and every workgroup shares one root.
"""
import functools

import numpy as np

import fusion_oracle as fo
import fusion_scene as fs
import mesh_oracle as mo
import mesh_scene as ms

TIE_DIMS = (9, 8, 10)
SHEET_DIMS = (129, 129, 3)
THRESHOLDS = (1, 3, 9, 41)


def sheets(dims):
    """(sum, cnt, gsum): sum[k] = (1, 1, -1, -1)[k mod 4] in every voxel of layer k, cnt = 2, gsum = 200: a flat sheet between
    the layers 4 n + 1 and 4 n + 2 and between 4 n + 3 and 4 n + 4."""
    nx, ny, nz = dims
    s = np.empty((nz, ny, nx), np.float32)
    s[:] = np.array([1.0, 1.0, -1.0, -1.0], np.float32)[np.arange(nz) % 4][:, None, None]
    return s, np.full((nz, ny, nx), 2, np.uint16), np.full((nz, ny, nx), 200, np.uint32)


def cases():
    """name -> (planes, dims, origin, voxel, trunc, min_counts)."""
    out = {}
    for d, mcs in (((2, 2, 2), (1,)), ((257, 2, 2), (1,)), ((16, 16, 3), (2,)), ((41, 41, 41), (1, 2))):
        out[ms.shape_id(d)] = (ms.wave_volume(d, 0, colour=True), d, fs.ORIGIN, ms.VOXEL, fs.TRUNC, mcs)
    out["main"] = (ms.main_volume(), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, (1, 2))
    out["tie"] = (sheets(TIE_DIMS), TIE_DIMS, fs.ORIGIN, ms.VOXEL, fs.TRUNC, (1,))
    out["sheet"] = (sheets(SHEET_DIMS), SHEET_DIMS, fs.ORIGIN, ms.VOXEL, fs.TRUNC, (1,))
    out["sphere"] = (fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC, (1,))
    return out


NAMES = ("2x2x2", "257x2x2", "16x16x3", "41x41x41", "main", "tie", "sheet", "sphere")


@functools.lru_cache(maxsize=None)
def oracle_mesh(name, min_count, normals=False):
    """The welded mesh of a case by the oracles of §16 and §24: computed once, shared, and left unchanged."""
    planes, dims, origin, voxel, _, _ = cases()[name]
    _, soup_key, _, _ = fo.extract(planes[:3], dims, origin, voxel, min_count)
    return mo.weld(planes, dims, origin, voxel, soup_key, min_count, normals)


def sizes(size, label):
    """The triangle counts of the components, by ascending label."""
    return [int(size[r]) for r in np.unique(label)]


# the cases tools/component_host_check.py writes: name -> (case name, min_count)
def host_check_cases():
    return {"main_min1": ("main", 1), "main_min2": ("main", 2), "wave_257x2x2": ("257x2x2", 1), "wave_16x16x3_min2": ("16x16x3", 2),
            "tie": ("tie", 1), "sphere": ("sphere", 1), "empty": (None, 1)}
