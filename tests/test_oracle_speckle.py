"""The speckle filter in tests/speckle_oracle.py alone: the union-find against the flood fill on every case of
tests/speckle_scene.py, the three consequences of the definition, the threshold's edge, the ramp, the difference that must not
overflow, the effect on the flat-patch scenes of §22, and the prototype table.  CPU only."""
import inspect

import numpy as np
import pytest

import dense_oracle as do
import dense_scene as ds
import speckle_oracle as so
import speckle_scene as sc
import unique_oracle as uo
import unique_scene as us

# the wide maps add nothing to a comparison of two Python loops
CASES = [c for c in sc.CASES if c[1] * c[2] <= sc.W3 * sc.H3]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_union_find_equals_flood_fill_and_the_consequences_hold(case):
    name, w, h, _, max_diff, min_size = case
    plane = sc.plane_map(case)
    depth = sc.depth_map(plane)
    assert plane.shape == (h, w) and plane.dtype == np.int32
    keep_p, keep_d = plane.copy(), depth.copy()
    a = so.speckle_filter(depth, plane, min_size, max_diff)
    b = so.speckle_filter(depth, plane, min_size, max_diff, how=so.segments_flood)
    assert np.array_equal(plane, keep_p) and np.array_equal(depth, keep_d)          # the inputs stay
    for k in ("label", "size", "plane"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)
    assert np.array_equal(_bits(a["depth"]), _bits(b["depth"]))
    label, size = a["label"], a["size"]
    valid = plane >= 0
    print(name, "segments", int((label.reshape(-1) == np.arange(h * w)).sum()), "valid", int(valid.sum()), "kept", int((a["plane"] >= 0).sum()))
    # labels: none where invalid, else the least index of the pixels that carry the label, whose number is the size
    assert (label[~valid] == so.NONE).all() and (size[~valid] == 0).all() and (size[valid] >= 1).all()
    flat = label.reshape(-1)
    for root in np.unique(flat[flat != so.NONE]):
        members = np.nonzero(flat == root)[0]
        assert members[0] == root and (size.reshape(-1)[members] == len(members)).all()
    # min_size = 1 is the identity on the valid pixels (an invalid one is cleared, whatever it held)
    one = so.speckle_filter(depth, plane, 1, max_diff)
    assert np.array_equal(one["plane"][valid], plane[valid]) and np.array_equal(_bits(one["depth"])[valid], _bits(depth)[valid])
    assert (one["plane"][~valid] == -1).all() and (one["depth"][~valid] == 0).all()
    # the output is a subset of the input, bit for bit where it stays
    kept = a["plane"] >= 0
    assert not (kept & ~valid).any() and np.array_equal(kept, size >= min_size)
    assert np.array_equal(a["plane"][kept], plane[kept]) and np.array_equal(_bits(a["depth"])[kept], _bits(depth)[kept])
    assert (a["plane"][~kept] == -1).all() and (a["depth"][~kept] == 0).all()
    # idempotent: a removal never changes another segment
    again = so.speckle_filter(a["depth"], a["plane"], min_size, max_diff)
    assert np.array_equal(again["plane"], a["plane"]) and np.array_equal(_bits(again["depth"]), _bits(a["depth"]))
    assert np.array_equal(again["size"][kept], size[kept]) and np.array_equal(again["label"][kept], label[kept])


def test_the_patterns_are_what_their_names_say():
    w, h = sc.W3, sc.H3
    seg = lambda pat, md: so.segments(sc.PATTERNS[pat](w, h), md)
    count = lambda label: int((label.reshape(-1) == np.arange(label.size)).sum())
    label, size = seg("serpentine", 0)
    assert count(label) == 1 and int(size.max()) == sc.serpentine_size(w, h) == 1348 and (label[size > 0] == 0).all()
    assert sc.serpentine_size(640, 480) == 153840 and sc.serpentine_size(8192, 2) == 8193
    assert count(seg("serpentine_v", 0)[0]) == 1 and count(seg("comb", 0)[0]) == 1 and count(seg("comb_up", 0)[0]) == 1
    assert count(seg("spiral", 1)[0]) == 1 and count(seg("spiral", 0)[0]) > 300
    assert count(seg("checkerboard", 1)[0]) == w * h and count(seg("checkerboard", 5)[0]) == 1
    label, size = seg("split", 0)
    assert count(label) == 2 and sorted(np.unique(label).tolist()) == [0, sc.TW + 1, so.NONE]
    label, size = seg("corner_sizes", 1)
    assert sorted(np.unique(size).tolist()) == [0, sc.MIN_SIZE - 1, sc.MIN_SIZE, sc.MIN_SIZE + 1]
    for s in range(5):
        p = sc.PATTERNS["random%d" % s](w, h)
        assert set(np.unique(p)) == {-1, 0, 1, 2, 3} and 0.25 < float((p < 0).mean()) < 0.35


def test_the_threshold_edge():
    """A segment of exactly min_size pixels stays, one of min_size - 1 goes."""
    for m in (1, 2, 4, 7):
        plane = np.full((5, 2 * m + 3), -1, np.int32)
        plane[1, 1:1 + m] = 2                                        # m pixels
        plane[3, 1:m] = 2                                            # m - 1 pixels (none for m = 1)
        out = so.speckle_filter(np.ones(plane.shape, np.float32), plane, m, 0)
        assert (out["plane"][1, 1:1 + m] == 2).all() and (out["plane"][3] == -1).all() and int((out["plane"] >= 0).sum()) == m
        assert (out["size"][1, 1:1 + m] == m).all() and (out["size"][3, 1:m] == m - 1).all()


def test_the_ramp_and_the_difference_that_must_not_overflow():
    w = 40
    ramp = np.arange(w, dtype=np.int32)[None, :].repeat(3, axis=0)
    label, size = so.segments(ramp[:1], 1)                           # linkage is per edge, not transitive in value
    assert (label == 0).all() and (size == w).all()
    label, size = so.segments(ramp[:1], 0)
    assert np.array_equal(label[0], np.arange(w)) and (size == 1).all()
    label, size = so.segments(ramp, 0)                               # ... and the columns of equal planes are segments
    assert np.array_equal(label, ramp.astype(np.uint32)) and (size == 3).all()
    big = np.array([[0, 2 ** 31 - 1, 0], [2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 1]], np.int32)
    for how in (so.segments, so.segments_flood):
        label, size = how(big, 1023)
        assert np.array_equal(label, [[0, 1, 2], [1, 1, 1]]) and np.array_equal(size, [[1, 4, 1], [4, 4, 4]])


ROWS = {"flat_plane_r1_t20": (((3, 1816), (0, 1801)), ((76, 1830), (53, 1769))),
        "flat_step_r1_t20": (((3, 1712), (2, 1679)), ((36, 1712), (18, 1616))),
        "flat_plane_r2_t40": (((1, 1870), (0, 1866)), ((30, 1886), (0, 1822)))}
_EFFECT = {}


def _effect(row):
    """((wrong, right) before, after) at u = 5 with (min_size 4, max_diff 1), and the same at u = 0 with (16, 0): kept and wrong /
    kept and right over all pixels of slot 0, counted as test_oracle_unique.py counts them.  Computed once a row."""
    if row[0] not in _EFFECT:
        scene, swept, truth = us.flat_row(row)
        bad = uo.wrong(swept[0], truth, us.FLAT_PLANES, ds.W_MIN, ds.W_MAX)
        with np.errstate(invalid="ignore"):
            good = np.abs(swept[0]["inv_depth"] - truth) <= do.plane_step(ds.W_MIN, ds.W_MAX, us.FLAT_PLANES)
        got = []
        for u, min_size, max_diff in ((us.FLAT_U, 4, 1), (0, 16, 0)):
            fd, fp = us.flat_filter(scene, swept, u)
            out = so.speckle_filter(fd, fp, min_size, max_diff)
            before, after = fd > 0, out["depth"] > 0
            got.append(((int((before & bad).sum()), int((before & good).sum())), (int((after & bad).sum()), int((after & good).sum()))))
            print(row[0], "u", u, "min_size", min_size, "max_diff", max_diff, "wrong / right", got[-1][0], "->", got[-1][1])
        _EFFECT[row[0]] = tuple(got)
    return _EFFECT[row[0]]


@pytest.mark.parametrize("row", us.FLAT_ROWS, ids=[r[0] for r in us.FLAT_ROWS])
def test_the_effect_on_the_flat_patch_scenes(row):
    """Before and after the speckle filter behind the uniqueness test: ROWS holds the figures of DESIGN.md §23.1."""
    got = _effect(row)
    (before, after), _ = got
    assert after[0] <= before[0] and 100 * after[1] >= 98 * before[1]      # the tightest row is flat_step: 98.07 %
    assert got == ROWS[row[0]]


def test_wrong_falls_in_at_least_one_row():
    assert any(_effect(row)[0][1][0] < _effect(row)[0][0][0] for row in us.FLAT_ROWS)


def test_prototype_table_covers_the_speckle_section():
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, dense, fusion
    names = set(pkg.declared_symbols())
    for n in ("ekf_dense_filter_speckle", "ekf_dense_get_segments", "ekf_dense_speckle_host", "ekf_dense_get_speckle_profile"):
        assert n in names and n in capi._PROTOS
    assert len(capi._PROTOS["ekf_dense_filter_speckle"][1]) == 4 and len(capi._PROTOS["ekf_dense_speckle_host"][1]) == 7
    assert all(hasattr(pkg.DenseStereo, m) for m in ("filter_speckle", "segments", "speckle_maps", "get_speckle_profile"))
    assert inspect.signature(pkg.DenseStereo.filter_speckle).parameters["max_diff"].default == 1
    assert inspect.signature(pkg.DenseStereo.speckle_maps).parameters["max_diff"].default == 1
    assert inspect.signature(dense.depth_maps_from_recording).parameters["speckle"].default is None
    assert pkg.DepthMap.__dataclass_fields__["segment_size"].default is None
    assert dense.SPECKLE_KERNELS == ("k_speckle_label", "k_speckle_merge", "k_speckle_count", "k_speckle_apply")
    for bad in (0, -3, (4,), (4, -1), (4, 1024), (0, 1), "4", True, [4, 1]):
        with pytest.raises(ValueError):
            dense.depth_maps_from_recording("nowhere", speckle=bad)
    assert "speckle" in fusion.mesh_from_recording.__doc__ and "speckle" in fusion.audit_recording.__doc__
