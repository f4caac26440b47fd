"""The plane maps and the case table shared by tests/test_oracle_speckle.py, tests/test_gpu_speckle.py and
tools/speckle_host_check.py: the shapes and patterns at which a tiled labelling kernel can go wrong.  The
kernels label 32 x 16 tiles and then merge across their borders, so 70 x 37 is a 3 x 3 grid of tiles with ragged edges.

A case: (name, width, height, pattern, max_diff, min_size); ``plane_map(case)`` builds its (height, width) int32 map and
``depth_map(plane)`` a depth map whose every element has bits of its own.
"""
import numpy as np

TW, TH = 32, 16                                                    # the kernels' tile
MIN_SIZE = 4


def one_plane(w, h):
    return np.full((h, w), 7, np.int32)


def all_invalid(w, h):
    return np.full((h, w), -1, np.int32)


def checkerboard(w, h):
    """Planes 0 / 5: all singletons at max_diff 1, one segment at 5."""
    y, x = np.mgrid[0:h, 0:w]
    return (5 * ((x + y) & 1)).astype(np.int32)


def serpentine(w, h):
    """One pixel wide: the even rows, joined at alternating ends by one pixel of the odd rows.  One segment of
    ceil(h / 2) w + floor(h / 2) pixels that crosses every vertical tile border in every even row and whose order along the
    path runs against the linear index in every other row: the long chains of a find."""
    p = np.full((h, w), -1, np.int32)
    p[0::2, :] = 0
    p[1::4, w - 1] = 0
    p[3::4, 0] = 0
    return p


def serpentine_size(w, h):
    return (h + 1) // 2 * w + h // 2


def serpentine_v(w, h):
    return np.ascontiguousarray(serpentine(h, w).T)


def spiral(w, h):
    """A rectangular spiral, one pixel wide with one pixel between its turns, from the top left corner inwards; the plane
    grows by one every four steps along it: one segment at max_diff 1, pieces of four pixels at 0."""
    p = np.full((h, w), -1, np.int32)
    inside = lambda x, y: 0 <= x < w and 0 <= y < h
    x = y = n = 0
    dx, dy = 1, 0
    p[0, 0] = 0
    while True:
        for _ in range(2):
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and p[ny, nx] < 0 and (not inside(fx, fy) or p[fy, fx] < 0):
                x, y, n = nx, ny, n + 1
                p[y, x] = n // 4
                break
            dx, dy = -dy, dx
        else:
            return p


def comb(w, h):
    """Teeth in the even columns that join only along the bottom row: the equivalence is found last, at the largest indices."""
    p = np.full((h, w), -1, np.int32)
    p[:, 0::2] = 0
    p[h - 1, :] = 0
    return p


def comb_up(w, h):
    return np.ascontiguousarray(comb(w, h)[::-1])


def split(w, h):
    """Two segments one pixel apart: a column of invalid pixels at the first tile border (or the middle of a narrow map)."""
    p = np.full((h, w), 3, np.int32)
    p[:, TW if w > TW + 1 else w // 2] = -1
    return p


def corner_sizes(w, h):
    """Segments of MIN_SIZE - 1, MIN_SIZE and MIN_SIZE + 1 pixels, each across a corner where four tiles meet."""
    assert w >= 2 * TW + 2 and h >= 2 * TH + 1 and MIN_SIZE == 4
    p = np.full((h, w), -1, np.int32)
    for x, y in ((TW - 1, TH - 1), (TW, TH - 1), (TW, TH)):                                   # 3 pixels
        p[y, x] = 1
    p[TH - 1:TH + 1, 2 * TW - 1:2 * TW + 1] = 2                                                # 4 pixels
    p[2 * TH - 1:2 * TH + 1, TW - 1:TW + 1] = 3                                                # 5 pixels
    p[2 * TH, TW + 1] = 3
    return p


def random_planes(seed):
    def make(w, h):
        rng = np.random.default_rng(2300 + seed)
        return rng.choice(np.array([-1, 0, 1, 2, 3], np.int32), size=(h, w), p=[0.3, 0.175, 0.175, 0.175, 0.175]).astype(np.int32)
    return make


PATTERNS = dict(one_plane=one_plane, all_invalid=all_invalid, checkerboard=checkerboard, serpentine=serpentine,
                serpentine_v=serpentine_v, spiral=spiral, comb=comb, comb_up=comb_up, split=split, corner_sizes=corner_sizes,
                **{"random%d" % s: random_planes(s) for s in range(5)})

W3, H3 = 70, 37
# the shapes: one pixel, one row, one column, exactly one tile (the merge has nothing to do), one pixel into each neighbour tile
SHAPE_CASES = [("%s_%dx%d" % (pat, w, h), w, h, pat, 1, MIN_SIZE)
               for w, h in ((1, 1), (1, 70), (70, 1), (TW, TH), (TW + 1, TH + 1)) for pat in ("one_plane", "random0")]
# 70 x 37, at max_diff 0 and 1 where it matters
GRID_CASES = [("%s_d%d" % (pat, md), W3, H3, pat, md, MIN_SIZE)
              for pat, diffs in (("one_plane", (0,)), ("all_invalid", (0,)), ("checkerboard", (1, 5)), ("serpentine", (0,)),
                                 ("serpentine_v", (0,)), ("spiral", (0, 1)), ("comb", (0,)), ("comb_up", (0,)), ("split", (0,)),
                                 ("corner_sizes", (1,))) + tuple(("random%d" % s, (0, 1)) for s in range(5))
              for md in diffs]
# the widest handle: 256 tiles in a row
WIDE_CASES = [("serpentine_8192x2", 8192, 2, "serpentine", 0, MIN_SIZE), ("one_plane_8192x2", 8192, 2, "one_plane", 0, MIN_SIZE)]
CASES = SHAPE_CASES + GRID_CASES + WIDE_CASES
# what the host check runs with 256 real threads a workgroup (the wide maps cost it minutes and show it nothing new)
HOST_CASES = SHAPE_CASES + GRID_CASES


def plane_map(case):
    return PATTERNS[case[3]](case[1], case[2])


def depth_map(plane):
    """float32, positive, every element with bits of its own, also where the plane is invalid: the filter must clear those
    and keep the others bit for bit."""
    h, w = plane.shape
    return (1.0 + np.arange(h * w, dtype=np.float64).reshape(h, w) / 1024.0 + 0.25 * np.maximum(plane, 0)).astype(np.float32)
