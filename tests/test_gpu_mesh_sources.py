"""Which mesh a source number means, and when a result made from it stops being current, through every entry
point that takes a source: on the analytic sphere of tests/fusion_scene.py the chain weld -> prune -> smooth("pruned") ->
simplify("smoothed") -> texture_begin("simplified") / finish is built and then broken at each link in turn.  After each break
every one of sources 0..3 is put to ekf_raster_render (shading 0 and 1), ekf_distance_run (as target and as query), its mesh
getter and ekf_texture_begin; status and message are compared whole.  What stayed current is read again and compared bit for
bit with what was read before the break.  No oracle runs: the data are the library's own, read twice."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_dense.py: one HIP runtime for both)

import fusion_scene as fs
import raycast_scene as rsc
import texture_scene as ts

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
STATE = 4
GETTERS = ("ekf_mesh_get", "ekf_components_get_pruned", "ekf_smooth_get", "ekf_simplify_get")
GETTER_TAILS = (": no ekf_mesh_weld since the volume last changed", ": no ekf_components_prune since the last ekf_mesh_weld",
                ": no ekf_smooth_run on the current mesh", ": no ekf_simplify_run on the current mesh")
NO_TEXTURE = ": shading 1 needs a finished texture (ekf_texture_finish) of the source that is rendered"

# The launches of the whole walk below per kind, as the getters name them, recorded on the commit before the stamps
# (f983858): the host bookkeeping decides which launches are made again, so the counts pin it.
LAUNCHES = {
    "fusion": [0, 2, 2, 2], "colour": [0, 0, 0], "raycast": [0, 0], "mesh": [3, 3, 3, 3, 3],
    "component": [4, 4, 4, 0, 6, 15, 5, 5], "smooth": [5, 5, 5, 5, 5, 24, 0], "simplify": [7, 7, 7, 35, 7, 7, 7, 7, 7, 7],
    "texture": [0, 0, 0, 7], "raster": [18, 18, 18, 18], "distance": [30, 30, 30, 30, 30, 30, 30, 0, 0],
}


def _tail(source, ok, weld_current):
    """The message tail of a call about `source` when the sources in `ok` resolve: None, or what the resolver says.  Source 3
    names itself whatever the reason; 1 and 2 do so only under a current weld."""
    if source in ok:
        return None
    if source == 3:
        return ": source 3 needs an ekf_simplify_run on the current mesh"
    if not weld_current:
        return ": no ekf_mesh_weld since the volume last changed"
    return (None, ": source 1 needs an ekf_components_prune since the last ekf_mesh_weld",
            ": source 2 needs an ekf_smooth_run on the current mesh")[source]


class Walk:
    def __init__(self, pkg):
        self.lib = pkg.load_library()
        self.v = pkg.TsdfVolume(fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC)
        self.v.set_volume(*fs.sphere_volume())
        self.K = np.ascontiguousarray(ts.K, np.float64)
        self.pose = np.ascontiguousarray(rsc.POSE_A, np.float64)
        self.v.set_distance_mesh([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[0, 1, 2]])
        self.mesh = {}

    def err(self):
        return self.lib.ekf_fusion_last_error(self.v._h).decode()

    def build(self, first):
        """The chain from link `first` on; the meshes and the atlas as the wrapper returns them."""
        v, m = self.v, self.mesh
        if first <= 0:
            m[0] = v.weld(1)
        if first <= 1:
            m[1] = v.prune(2)
        if first <= 2:
            m[2] = v.smooth(2, source="pruned")
        if first <= 3:
            m[3] = v.simplify(2.0 * v.voxel, "smoothed")
        v.texture_begin("simplified", patch=4, channels=1)
        self.atlas = v.texture_finish()

    def fetch(self, source):
        """The rows of a source as its getter delivers them now, into arrays of the sizes the wrapper reported."""
        like = self.mesh[source]
        nv, nt = len(like.key), len(like.faces)
        xyz, faces = np.full((nv, 3), -1.0), np.full((nt, 3), 0xFFFFFFFF, np.uint32)
        grey, key = np.full(nv, 0xA5, np.uint8), np.full(nv, 2**64 - 1, np.uint64)
        assert getattr(self.lib, GETTERS[source])(self.v._h, P(xyz), P(faces), P(grey), None, None, P(key), nv, nt) == 0
        return xyz, faces, grey, key

    def same(self, source):
        like = self.mesh[source]
        return all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
                   for a, b in zip(self.fetch(source), (like.vertices, like.faces, like.grey, like.key)))

    def probe(self, ok, weld_current, textured=None):
        """Every entry point that takes a source, for sources 0..3; ekf_texture_begin last, since it replaces the texture."""
        lib, h = self.lib, self.v._h
        n = C.c_ulonglong(0)
        side = C.c_int(0)
        for s in range(4):
            tail = _tail(s, ok, weld_current)
            want = (0, None) if tail is None else (STATE, tail)
            render = lambda shading: lib.ekf_raster_render(h, s, ts.W, ts.H, P(self.K), P(self.pose), C.c_double(0.0), 1, shading, 0)
            calls = [("ekf_raster_render", lambda: render(0), want),
                     ("ekf_raster_render", lambda: render(1), want if tail is not None or s == textured else (STATE, NO_TEXTURE)),
                     ("ekf_distance_run", lambda: lib.ekf_distance_run(h, s, 4, C.byref(n)), want),
                     ("ekf_distance_run", lambda: lib.ekf_distance_run(h, 4, s, C.byref(n)), want),
                     (GETTERS[s], lambda: getattr(lib, GETTERS[s])(h, None, None, None, None, None, None, 0, 0),
                      (0, None) if s in ok else (STATE, GETTER_TAILS[s]))]
            for who, call, (status, msg) in calls:
                assert call() == status, (s, who, self.err())
                assert msg is None or self.err() == who + msg, (s, who, self.err())
            if s in ok:
                assert self.same(s), s
        for s in range(4):
            tail = _tail(s, ok, weld_current)
            assert lib.ekf_texture_begin(h, s, 4, 1, C.byref(side)) == (0 if tail is None else STATE), (s, self.err())
            assert tail is None or self.err() == "ekf_texture_begin" + tail, (s, self.err())

    def counts(self):
        v = self.v
        got = dict(fusion=v.get_profile(), colour=v.get_colour_profile(), raycast=v.get_raycast_profile(), mesh=v.get_mesh_profile(),
                   component=v.get_component_profile(), smooth=v.get_smooth_profile(), simplify=v.get_simplify_profile(),
                   texture=v.get_texture_profile(), raster=v.get_raster_profile(), distance=v.get_distance_profile())
        return {k: [c for _, c in d.values()] for k, d in got.items()}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def test_every_source_through_every_break_of_the_chain(pkg):
    w = Walk(pkg)
    v, lib = w.v, w.lib
    try:
        v.profile(True)
        w.build(0)
        atlas = np.zeros_like(w.atlas.atlas)
        read_atlas = lambda: lib.ekf_texture_get(v._h, P(atlas), atlas.shape[1], None, None, None, 0)
        assert read_atlas() == 0 and np.array_equal(atlas, w.atlas.atlas)
        assert lib.ekf_raster_render(v._h, 3, ts.W, ts.H, P(w.K), P(w.pose), C.c_double(0.0), 1, 1, 0) == 0
        w.probe({0, 1, 2, 3}, True, textured=3)
        none = "ekf_texture_get: no ekf_texture_begin on the current mesh"

        w.build(3)
        w.mesh[2] = v.smooth(2, source="pruned")                             # a new smooth run: the simplified mesh and its texture go
        assert read_atlas() == STATE and w.err() == none
        w.probe({0, 1, 2}, True)

        w.build(3)
        w.mesh[1] = v.prune(2)                                               # a new prune: the smoothed mesh goes too
        assert read_atlas() == STATE and w.err() == none
        w.probe({0, 1}, True)

        w.build(2)
        v.components()                                                       # the components again: the pruned mesh goes
        assert read_atlas() == STATE and w.err() == none
        w.probe({0}, True)

        w.build(1)
        w.mesh[0] = v.weld(1)                                                # a new weld: only it is left
        assert read_atlas() == STATE and w.err() == none
        w.probe({0}, True)

        w.build(1)
        v.set_volume(*fs.sphere_volume())                                    # a change of the volume: nothing is left
        assert read_atlas() == STATE and w.err() == none
        w.probe(set(), False)

        w.build(0)                                                           # and the chain stands again
        assert read_atlas() == 0 and np.array_equal(atlas, w.atlas.atlas)
        w.probe({0, 1, 2, 3}, True, textured=3)
        got = w.counts()
        print("launches of the walk:", got)
        assert got == LAUNCHES
    finally:
        v.close()
