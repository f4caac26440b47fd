"""numpy restatement of the colour contract of the dense chain, written from the contract and built on the
grey oracles, which stay as they are: tests/dense_oracle.py (§15), tests/fusion_oracle.py (§16), tests/raycast_oracle.py (§17).

Channel order is B, G, R.  A colour volume is (sum, cnt, gsum, csum) with csum of shape (3, nz, ny, nx).  Its colour planes are
built as its grey plane is, with one channel in the place of the grey value: where the grey oracle already states an
operation (the voxels a map updates, the blend along an edge, the trilinear blend at a hit), this file calls it with the
channel's plane in gsum's place and states nothing twice.  `vertex_colours` is the exception: it restates the kernel's way
from the vertex key alone, and tests/test_oracle_colour.py holds it against the extraction of the channel planes.
"""
import numpy as np

import fusion_oracle as fo
import raycast_oracle as ro


def bgr2gray(b, g, r):
    """(b 1868 + g 9617 + r 4899 + 8192) >> 14 in 32-bit unsigned integers; the weights sum to 2^14."""
    b, g, r = (np.asarray(v).astype(np.uint32) for v in (b, g, r))
    return (b * np.uint32(1868) + g * np.uint32(9617) + r * np.uint32(4899) + np.uint32(8192)) >> np.uint32(14)


def grey_of(bgr):
    """The (H, W) uint8 grey image of a (H, W, 3) B, G, R image."""
    a = np.asarray(bgr, np.uint8)
    return bgr2gray(a[..., 0], a[..., 1], a[..., 2]).astype(np.uint8)


def as_colour(image):
    """A (H, W, 3) image as it is; a (H, W) image as the colour image a colour volume sees: its grey value in every channel."""
    a = np.asarray(image, np.uint8)
    return a if a.ndim == 3 else np.repeat(a[:, :, None], 3, axis=2)


def empty_volume(dims):
    nx, ny, nz = (int(v) for v in dims)
    return fo.empty_volume(dims) + (np.zeros((3, nz, ny, nx), np.uint32),)


def integrate(vol, dims, origin, voxel, trunc, depth, image, K, pose7):
    """One map into vol = (sum, cnt, gsum, csum) in place; image is (H, W, 3), or (H, W) for a map without colour.  sum, cnt
    and gsum are those of a plain volume fed the grey image; csum[c] is the gsum of a plain volume fed channel c.  Returns
    the class of every voxel."""
    s_, c_, g_, cs = vol
    image = np.asarray(image, np.uint8)
    bgr = as_colour(image)
    grey = grey_of(image) if image.ndim == 3 else image
    for c in range(3):
        fo.integrate((s_.copy(), c_.copy(), cs[c]), dims, origin, voxel, trunc, depth, np.ascontiguousarray(bgr[..., c]), K, pose7)
    return fo.integrate((s_, c_, g_), dims, origin, voxel, trunc, depth, grey, K, pose7)


def vertex_colours(vol, dims, key):
    """(n, 3, 3) uint8, B G R of each vertex, from the keys alone: la = key >> 3, the bits of d = key & 7 are the steps to the
    edge's other end, u = va / (va - vb) with v = (double) sum / (double) cnt, a channel C = (double) csum / (double) cnt
    blended as Ca + u (Cb - Ca) and rounded floor(. + 0.5)."""
    s_, c_, _, cs = vol
    nx, ny, nz = (int(v) for v in dims)
    key = np.asarray(key, np.uint64)
    la = (key >> np.uint64(3)).astype(np.int64)
    d = (key & np.uint64(7)).astype(np.int64)
    lb = la + (d & 1) + ((d >> 1) & 1) * nx + (d >> 2) * (nx * ny)
    s1, c1 = s_.reshape(-1), c_.reshape(-1)
    out = np.zeros(key.shape + (3,), np.uint8)
    with np.errstate(all="ignore"):
        na, nb = c1[la].astype(np.float64), c1[lb].astype(np.float64)
        va, vb = s1[la].astype(np.float64) / na, s1[lb].astype(np.float64) / nb
        u = va / (va - vb)
        for c in range(3):
            p = cs[c].reshape(-1)
            Ca, Cb = p[la].astype(np.float64) / na, p[lb].astype(np.float64) / nb
            cv = Ca + u * (Cb - Ca)
            out[..., c] = np.floor(cv + 0.5).astype(np.int64).astype(np.uint8)
    return out


def extract(vol, dims, origin, voxel, min_count=1):
    """(xyz, key, grey, colour (n, 3, 3) uint8): the mesh of the first three planes, unchanged, and its vertex colours."""
    xyz, key, grey, _ = fo.extract(vol[:3], dims, origin, voxel, min_count)
    return xyz, key, grey, vertex_colours(vol, dims, key)


def raycast(vol, dims, origin, voxel, shape, K, pose7, z_near, z_far, step, min_count=1):
    """The grey render of the first three planes, unchanged, with `colour` (H, W, 3) uint8: at the hit, channel c is the
    trilinear blend of the eight corners' csum[c] / cnt with the grey's fractions, rounded the same way -- what the grey
    oracle computes with csum[c] in gsum's place; 0, 0, 0 without a hit."""
    out = ro.raycast(vol[:3], dims, origin, voxel, shape, K, pose7, z_near, z_far, step, min_count)
    planes = [ro.raycast((vol[0], vol[1], vol[3][c]), dims, origin, voxel, shape, K, pose7, z_near, z_far, step, min_count)
              for c in range(3)]
    for p in planes:
        assert p["depth"].tobytes() == out["depth"].tobytes()
    out["colour"] = np.stack([p["grey"] for p in planes], axis=2)
    return out
