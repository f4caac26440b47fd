"""Volumes and shapes shared by tests/test_oracle_mesh.py, tests/test_gpu_mesh.py and tools/mesh_host_check.py (DESIGN.md
§24.5); tests/fusion_scene.py and tests/colour_scene.py are imported read-only.

The shapes are the smallest at which each index path of the weld can go wrong: one cell; two cells that share a face (and
its diagonal); a row that crosses a 256-voxel workgroup; exactly three workgroups; the main volume of §16.5 (neither the
voxels nor the cells a multiple of 256); the sphere; and 41 x 41 x 41 = 68921 voxels = 270 workgroups, so that every lane
of k_tsdf_scan owns a chunk of 2 blocks.
"""
import numpy as np

import fusion_scene as fs

WAVE_SHAPES = ((2, 2, 2), (3, 2, 2), (257, 2, 2), (16, 16, 3), (41, 41, 41))
VOXEL = 0.1


def shape_id(dims):
    return "%dx%dx%d" % tuple(dims)


def wave_volume(dims, seed=0, colour=False):
    """(sum, cnt, gsum[, csum]) of a rippled surface through the middle of the grid, with noise large enough to make
    isolated sign changes, cnt in 0..3 (about one voxel in ten below 2, one in thirty at 0) and sums that are not multiples
    of the counts.  Deterministic in (dims, seed)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(1000 * seed + nx + 7 * ny + 31 * nz)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    field = (k - (nz - 1) / 2.0) + 0.9 * np.sin(0.45 * i + 0.2) * np.cos(0.3 * j) + 0.35 * rng.standard_normal((nz, ny, nx))
    cnt = rng.choice(np.array([0, 1, 2, 3], np.uint16), size=(nz, ny, nx), p=[0.03, 0.07, 0.4, 0.5])
    s = (np.clip(field / 2.5, -1.0, 1.0) * cnt).astype(np.float32)
    gsum = (rng.integers(0, 256, size=(nz, ny, nx)) * cnt - (cnt > 1) * rng.integers(0, 2, size=(nz, ny, nx))).clip(0).astype(np.uint32)
    if not colour:
        return s, cnt, gsum
    csum = np.stack([(rng.integers(0, 256, size=(nz, ny, nx)) * cnt).astype(np.uint32) for _ in range(3)])
    return s, cnt, gsum, csum


def random_volume(dims, seed):
    """Random signs and cnt drawn from {0, 1, 2, 3}: crossing edges none of whose cells is valid occur, and so do crossing
    edges with exactly one valid cell (tests/test_oracle_mesh.py asserts both)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 4, size=(nz, ny, nx)).astype(np.uint16)
    s = (rng.uniform(-1.0, 1.0, size=(nz, ny, nx)) * np.maximum(cnt, 1)).astype(np.float32)
    s[rng.random((nz, ny, nx)) < 0.05] = 0.0                          # an exact zero is outside, and so is -0
    s[rng.random((nz, ny, nx)) < 0.02] = -0.0
    gsum = (rng.integers(0, 256, size=(nz, ny, nx)) * cnt).astype(np.uint32)
    csum = np.stack([(rng.integers(0, 256, size=(nz, ny, nx)) * cnt).astype(np.uint32) for _ in range(3)])
    return s, cnt, gsum, csum


RANDOM_DIMS = ((4, 3, 3), (5, 4, 3), (3, 5, 4), (6, 2, 5), (2, 2, 7))


def random_cases(n=24):
    """(dims, seed, min_count) of the random volumes of tests/test_oracle_mesh.py."""
    return [(RANDOM_DIMS[s % len(RANDOM_DIMS)], s, 1 + s % 3) for s in range(n)]


def main_volume():
    return fs.fused()[0][-1]


def sphere_radial(vertices):
    """The unit radial direction of the analytic sphere at each vertex (its centre is the world origin)."""
    v = np.asarray(vertices, np.float64)
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


# the cases tools/mesh_host_check.py writes: name -> (volume, dims, origin, voxel, min_count)
def host_check_cases():
    out = {}
    for mc in (1, 2, 4):
        out["main_min%d" % mc] = (main_volume(), fs.DIMS, fs.ORIGIN, fs.VOXEL, mc)
    out["sphere"] = (fs.sphere_volume(), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    out["empty"] = (tuple(np.zeros_like(p) for p in main_volume()), fs.DIMS, fs.ORIGIN, fs.VOXEL, 1)
    for dims in WAVE_SHAPES[:4]:
        for mc in (1, 2):
            out["wave_%s_min%d" % (shape_id(dims), mc)] = (wave_volume(dims, 0, colour=True), dims, fs.ORIGIN, VOXEL, mc)
    return out
