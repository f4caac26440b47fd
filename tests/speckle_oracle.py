"""Plain numpy / Python restatement of the speckle filter of the dense depth maps, written from the contract.

For a plane map ``plane`` (H, W) int with its depth map, ``min_size >= 1`` and ``max_diff >= 0``:

  - a pixel is valid iff plane >= 0 (the depth plays no part);
  - two 4-neighbours are linked iff both are valid and |plane_a - plane_b| <= max_diff, the difference taken in Python ints
    (no overflow: planes 0 and 2^31 - 1 are simply not linked);
  - a segment is a connected component of the links (linkage is per edge: a ramp 0, 1, 2, ... is one segment at max_diff 1);
  - the label of a valid pixel is the least linear index y W + x of its segment, its size the segment's pixel count; an invalid
    pixel has label 0xFFFFFFFF and size 0;
  - the filter sets depth = 0, plane = -1 where size < min_size and leaves every other element as it was, bit for bit.

``segments`` is a union-find over the linked edges, ``segments_flood`` a breadth-first flood fill: two statements of one
definition that share only ``links``.
"""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF


def links(plane, max_diff):
    """(right, down): bool (H, W - 1) and (H - 1, W), the links of every pixel to its right and its lower neighbour."""
    assert int(max_diff) >= 0
    p = np.asarray(plane).astype(object)                            # Python ints: no difference overflows
    v = np.asarray(plane) >= 0
    right = v[:, :-1] & v[:, 1:] & np.array(abs(p[:, :-1] - p[:, 1:]) <= int(max_diff), bool).reshape(v[:, 1:].shape)
    down = v[:-1, :] & v[1:, :] & np.array(abs(p[:-1, :] - p[1:, :]) <= int(max_diff), bool).reshape(v[1:, :].shape)
    return right, down


def _sizes(label, shape):
    flat = label.reshape(-1)
    ok = flat != NONE
    count = np.bincount(flat[ok].astype(np.int64), minlength=flat.size)
    size = np.zeros(flat.size, np.uint32)
    size[ok] = count[flat[ok].astype(np.int64)]
    return label.reshape(shape).astype(np.uint32), size.reshape(shape)


def segments(plane, max_diff):
    """(label, size), both (H, W) uint32, by a union-find over the linked edges; the smaller root always wins, so a
    segment's root is its least index."""
    plane = np.asarray(plane)
    H, W = plane.shape
    right, down = links(plane, max_diff)
    parent = list(range(H * W))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for (ys, xs), step in ((np.nonzero(right), 1), (np.nonzero(down), W)):
        for a in (ys * W + xs).tolist():
            ra, rb = find(a), find(a + step)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    valid = (plane >= 0).reshape(-1)
    label = np.array([find(i) if valid[i] else NONE for i in range(H * W)], np.int64)
    return _sizes(label, (H, W))


def segments_flood(plane, max_diff):
    """The same two maps by a breadth-first flood fill from every valid pixel not yet reached, in row-major order: the
    pixel a fill starts from is the least index of its segment."""
    plane = np.asarray(plane)
    H, W = plane.shape
    right, down = links(plane, max_diff)
    label = np.full(H * W, NONE, np.int64)
    for start in np.nonzero((plane >= 0).reshape(-1))[0].tolist():
        if label[start] != NONE:
            continue
        label[start] = start
        todo = deque([start])
        while todo:
            i = todo.popleft()
            y, x = divmod(i, W)
            near = []
            if x + 1 < W and right[y, x]:
                near.append(i + 1)
            if x > 0 and right[y, x - 1]:
                near.append(i - 1)
            if y + 1 < H and down[y, x]:
                near.append(i + W)
            if y > 0 and down[y - 1, x]:
                near.append(i - W)
            for j in near:
                if label[j] == NONE:
                    label[j] = start
                    todo.append(j)
    return _sizes(label, (H, W))


def speckle_filter(depth, plane, min_size, max_diff, how=segments):
    """dict(depth, plane, label, size): the filtered maps, and the labels and sizes before the removal.  The inputs stay."""
    assert int(min_size) >= 1
    depth, plane = np.asarray(depth, np.float32), np.asarray(plane, np.int32)
    label, size = how(plane, max_diff)
    drop = size < int(min_size)
    return dict(depth=np.where(drop, np.float32(0), depth).astype(np.float32), plane=np.where(drop, -1, plane).astype(np.int32),
                label=label, size=size)
