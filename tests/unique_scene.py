"""The case tables shared by tests/test_oracle_unique.py, tests/test_gpu_unique.py and tools/unique_host_check.py
(DESIGN.md §22): the existing tiny cases of the four cost curves, in one form, and the three rows of the flat-patch table.

A case: (name, width, height, planes, radius, trunc, source slots, census, n_best, paths, p1, p2, views), where n_best = 0 sums
all sources, paths = 0 takes the pixel-wise winner, and `views` names the scene: "step" (dense_scene), "exposed" (census_scene:
the step scene with the sources re-exposed), "best" (best_scene's nine cameras), "sgm" (sgm_scene.case_views of the case of
that name) and "sgm_exposed".
"""
import best_scene as bs
import census_scene as cs
import dense_scene as ds
import sgm_scene as ss
import unique_oracle as uo

SW, SH = ds.SMALL_W, ds.SMALL_H


def _plain(c, census=0, views="step"):
    return c[:7] + (census, 0, 0, 0, 0, views)


def _sgm(c, census=0, views="sgm"):
    return c[:7] + (census, 0, c[9], c[7], c[8], views)


def _best(name):
    c = [x for x in bs.CASES if x[0] == name][0]
    return ("best_" + c[0],) + c[1:7] + (c[8], c[7], c[9], c[10], c[11], "best")


_SGM = {c[0]: c for c in ss.CASES + ss.MANY_PLANES_CASES}
_DENSE = {c[0]: c for c in ds.CASES}

# plain grey: the seven of dense_scene (two_planes: every runner-up absent; small: less than a tile), and the small shape at
# the least plane counts at which the runner-up is sometimes absent (3) and always present (4): winners on plane 0 and D - 1
PLAIN_CASES = [_plain(c) for c in ds.CASES] + [
    ("small_d3", SW, SH, 3, 1, 255, (1, 2), 0, 0, 0, 0, 0, "step"),
    ("small_d4", SW, SH, 4, 1, 255, (1, 2), 0, 0, 0, 0, 0, "step"),
]
CENSUS_CASES = [("census_" + c[0],) + _plain(c, 1, "exposed")[1:] for c in (_DENSE["r1_t20_v2"], _DENSE["small"])]
BEST_CASES = [_best("v2_b1_t20"), _best("census_v3_b2")]                    # n_best < n_src, both costs
# one, two, three and many planes a lane in the winner's reduction (12, 70, 130, 300), and the textureless patch
SGM_CASES = [("sgm_" + n,) + _sgm(_SGM[n])[1:] for n in ("paths8", "planes70", "planes130", "flat_plane", "planes300")]
# the aggregated curve of the other costs: the winner's twin is one kernel, the volume in front of it is not
SGM_OTHER_CASES = [("sgm_census_paths4",) + _sgm([c for c in cs.SGM_CASES if c[0] == "paths4"][0], 1, "sgm_exposed")[1:],
                   _best("sgm8_v3_b2")]
CASES = PLAIN_CASES + CENSUS_CASES + BEST_CASES + SGM_CASES + SGM_OTHER_CASES
# one case of each of the five sweep kinds (plain, census, best, sgm, sgm_census)
KIND_CASES = [PLAIN_CASES[1], CENSUS_CASES[0], BEST_CASES[0], SGM_CASES[0], SGM_OTHER_CASES[0]]


def case_views(case):
    """slot -> (image, K, pose) of a case's scene at its size."""
    name, w, h, views = case[0], case[1], case[2], case[12]
    if views == "step":
        return ds.case_views(w, h)
    if views == "exposed":
        return cs.exposed(ds.case_views(w, h))
    if views == "best":
        return bs.case_views(w, h)
    sgm_case = (name,) + case[1:7] + (case[10], case[11], case[9], "flat_plane" if name == "sgm_flat_plane" else "step")
    v = ss.case_views(sgm_case)
    return cs.exposed(v) if views == "sgm_exposed" else v


def case_oracle(case, ref=0):
    """(views, the oracle's five maps) of slot `ref` swept against the case's other slots."""
    name, w, h, D, radius, trunc, src, census, n_best, paths, p1, p2, _ = case
    views = case_views(case)
    slots = (0,) + tuple(src)
    want = uo.sweep(views[ref][0], views[ref][1], views[ref][2], [views[s] for s in slots if s != ref], ds.W_MIN, ds.W_MAX, D,
                    radius, trunc, bool(census), n_best, paths, p1, p2)
    return views, want


# The flat-patch table: (name, scene, surface, radius, trunc).  Slots 0, 1, 2 are each swept against the other two with
# W_MIN, W_MAX and 12 planes; slot 0 is filtered against 1 and 2 at rel_tol 0.01, min_agree 1.
FLAT_ROWS = [
    ("flat_plane_r1_t20", ss.flat_plane_scene, ss.PLANE_SURFACE, 1, 20),
    ("flat_step_r1_t20", ss.flat_step_scene, ss.STEP_SURFACE, 1, 20),
    ("flat_plane_r2_t40", ss.flat_plane_scene, ss.PLANE_SURFACE, 2, 40),
]
FLAT_PLANES, FLAT_REL_TOL, FLAT_MIN_AGREE, FLAT_U = 12, 0.01, 1, 5


def flat_row(row):
    """(scene, {slot: the oracle's five maps}, the true inverse depth of slot 0) of a row of FLAT_ROWS."""
    name, make, surface, radius, trunc = row
    scene = make()
    swept = {s: uo.sweep(*scene[s], [scene[o] for o in (0, 1, 2) if o != s], ds.W_MIN, ds.W_MAX, FLAT_PLANES, radius, trunc)
             for s in (0, 1, 2)}
    return scene, swept, ds.true_inverse_depth(surface)


def flat_filter(scene, swept, u):
    """The oracle's filtered (depth, plane) of slot 0 of a flat row at uniqueness u."""
    src = [(swept[s]["depth"], scene[s][1], scene[s][2]) for s in (1, 2)]
    return uo.unique_filter(swept[0]["depth"], swept[0]["plane"], swept[0]["cost"], swept[0]["runner"], scene[0][1], scene[0][2],
                            src, FLAT_REL_TOL, FLAT_MIN_AGREE, u)
