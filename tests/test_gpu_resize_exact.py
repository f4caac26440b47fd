"""Map resizing (remove, convert, add) element by element, beyond one column block of k_compact_transform.

A resize is mostly a copy, so most of it is tested EXACTLY: on a patterned state (tests/resize_reference.py: every
entry of Sigma's upper triangle and of mu a different number) every pass-through entry of the result must equal its
source entry bit for bit, in fp32 and fp64, with no oracle and no tolerance; Sigma stays exactly symmetric and the
padding exactly zero.  Only the entries of converted features are arithmetic; they are held element-wise to
|S - ref| <= 40 u A against the fp64 J Sigma J^T, A = |J| |Sigma| |J|^T (the ceiling and its derivation: DESIGN.md,
"Resizing the map"; tests/golden/parity_bounds.json tightens each site to what the MI355X measured).

The cases (resize_reference.CASES) are the smallest shapes that reach each index-dependent path of the kernel, and
test_cases_reach_every_path asserts that they do.  No update runs on a patterned state: it is not positive definite."""
import ctypes as C

import numpy as np
import pytest

import ekf_oracle as o
import resize_reference as rr
from helpers import bound, gpu_filter, oracle_cfg

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
CEILING = 40.0
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def _filter(n_feat, dtype, camera_dim=14, xyz=(), capacity=None):
    """A filter with `n_feat` features through addFeature, those in `xyz` converted by a first convert2XYZ_ifLinearAll
    on a patterned state; returns it with its layout."""
    g = gpu_filter(n_feat, dtype, capacity=capacity, camera_dim=camera_dim)
    for (u, v) in o.synthetic_pixels(oracle_cfg(), n_feat):
        assert g.addFeature((u, v)) == 1
    pos, cod = rr.layout(n_feat, camera_dim)
    _same_layout(g, pos, cod)
    if len(xyz):
        _inject(g, pos, cod, convert=xyz)
        assert g.convert2XYZ_ifLinearAll() == len(xyz)
        pos, cod = rr.layout(n_feat, camera_dim, xyz)
        _same_layout(g, pos, cod)
    return g, pos, cod


def _same_layout(g, pos, cod):
    gp, gc = g.featureLayout()
    assert g.numOfFeatures() == len(pos) and g.stateDim() == rr.state_dim(pos, cod, g.camera_dim)
    assert np.array_equal(gp, pos) and np.array_equal(gc, cod)


def _inject(g, pos, cod, convert=()):
    mu, S = rr.patterned_state(pos, cod, g.camera_dim, g.dtype.type, convert=convert)
    g.setFullState(mu)
    g.setSigmaBlock(S)
    return mu, S


def _invariants(g, S):
    assert np.array_equal(S, S.T)
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and asym == 0.0 and big == float(np.float32(np.abs(S).max())), (pad, asym, big)


def _remove_exact(g, pos, cod, drop):
    """One removal on a patterned state: everything is a copy."""
    mu, S = _inject(g, pos, cod)
    e_mu, e_S, npos, ncod = rr.after_remove(mu, S, pos, cod, g.camera_dim, drop)
    g.removeFeatures(list(drop))
    _same_layout(g, npos, ncod)
    mu2, S2 = g.getFullState(), g.getFullSigma()
    assert np.array_equal(mu2, e_mu)
    assert np.array_equal(S2, e_S), f"{int((S2 != e_S).sum())} entries differ, first at {np.argwhere(S2 != e_S)[:4].tolist()}"
    _invariants(g, S2)
    return npos, ncod


def _convert_bounded(g, pos, cod, conv):
    """One conversion on a patterned state: pass-through entries exact, those of converted features within 40 u A."""
    dt = g.dtype.type
    mu, S = _inject(g, pos, cod, convert=conv)
    r = rr.after_convert(mu, S, pos, cod, g.camera_dim, conv)
    assert g.convert2XYZ_ifLinearAll() == len(conv)
    _same_layout(g, r.pos, r.coding)
    mu2, S2 = g.getFullState(), g.getFullSigma()
    assert np.array_equal(mu2[r.mu_exact], r.ref_mu[r.mu_exact].astype(dt))
    assert np.array_equal(S2[r.exact], r.ref[r.exact].astype(dt)), f"{int((S2[r.exact] != r.ref[r.exact]).sum())} pass-through entries differ"
    _invariants(g, S2)
    rest = ~r.exact
    w_S = rr.worst_ratio(S2[rest], r.ref[rest], r.A[rest], U[dt])
    w_mu = rr.worst_ratio(mu2[~r.mu_exact], r.ref_mu[~r.mu_exact], r.A_mu[~r.mu_exact], U[dt])
    print(f"converted entries: Sigma {w_S:.2f} u A, mu {w_mu:.2f} u A")
    assert bound("Sigma of converted features / (u A)", w_S, CEILING)
    assert bound("mu of converted features / (u A)", w_mu, CEILING)
    return r, mu2, S2


def _run_case(name, dtype):
    c = rr.CASES[name]
    g, pos, cod = _filter(c.n_feat, dtype, c.camera_dim, c.xyz)
    if c.op == "remove":
        return g, _remove_exact(g, pos, cod, c.arg)
    return g, _convert_bounded(g, pos, cod, c.arg)


def test_cases_reach_every_path():
    rr.assert_coverage()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["two_blocks_tail", "exactly_1024", "odd_sizes_1", "odd_sizes_2", "odd_sizes_3", "three_blocks"])
def test_remove_is_a_copy(name, dtype):
    _run_case(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_across_1024_and_back(dtype):
    """n 1046 -> 1016 (two column blocks of sources, one of results), then two addFeature back across 1024: the old
    block untouched, the new rows and columns mirror each other, nothing beyond them."""
    g, (pos, cod) = _run_case("across_1024", dtype)
    assert g.stateDim() == 1016
    for k in range(2):
        _, S0 = g.getFullState(), g.getFullSigma()
        n = g.stateDim()
        assert g.addFeature((200.0 + 10 * k, 150.0)) == 1
        S1 = g.getFullSigma()
        assert g.stateDim() == n + 6 and np.array_equal(S1[:n, :n], S0)
        assert np.array_equal(S1[n:, :], S1[:, n:].T) and np.isfinite(S1).all() and S1[n:, :].any()
        assert g.checkInvariants()[0] == 0.0
    assert g.stateDim() == 1028


def _expected_table(g, mu, S, pos, cod, ids, archived):
    """RosVSLAM::getPointsFeatures by hand (oracle get_points_features): rows by real_index, live XYZ features
    [X Y Z] * map_scale and their 3 x 3 block row by row, the archived rows written over them."""
    dt = g.dtype.type
    scale = mu[13] if g.camera_dim == 14 else dt(1)
    tab = np.zeros((ids[-1] + 1, 12), dt)
    for p, c, ri in zip(pos, cod, ids):
        if c:
            tab[ri, :3] = mu[p:p + 3] * scale
            tab[ri, 3:] = S[p:p + 3, p:p + 3].reshape(-1)
    for ri, xyz, cov in archived:
        if ri < len(tab):
            tab[ri, :3] = xyz * scale
            tab[ri, 3:] = cov
    return tab


@pytest.mark.parametrize("dtype", DTYPES)
def test_phases_remove_and_archive(dtype):
    """Removals at every phase of a four-column group on a mixed map; then 22 XYZ features with n_find = 6 leave in
    ONE removal (more than one 256-lane block of k_archive_points): the archive and the points table are copies too."""
    c = rr.CASES["phases"]
    g, pos, cod = _filter(c.n_feat, dtype, c.camera_dim, c.xyz)
    for i in np.flatnonzero(cod):
        g.setFeatureMeta(int(i), n_find=6)
    ids0, _ = g.featureIds()
    mu, S = rr.patterned_state(pos, cod, c.camera_dim, dtype)
    archived = [(ids0[i], mu[pos[i]:pos[i] + 3], S[pos[i]:pos[i] + 3, pos[i]:pos[i] + 3].reshape(-1)) for i in c.arg if cod[i]]
    assert len(archived) == 2
    pos, cod = _remove_exact(g, pos, cod, c.arg)
    assert g.numArchived() == 2
    ids, nf = g.featureIds()
    assert list(ids) == [r for i, r in enumerate(ids0) if i not in c.arg] and (nf[cod != 0] == 6).all()
    mu, S = g.getFullState(), g.getFullSigma()
    assert np.array_equal(g.getPointsTable(), _expected_table(g, mu, S, pos, cod, ids, archived))
    # the second removal: 22 of the 23 XYZ features left, spread over the whole map, on a fresh pattern
    drop = tuple(int(i) for i in np.flatnonzero(cod)[:22])
    mu, S = rr.patterned_state(pos, cod, c.camera_dim, dtype)
    archived += [(ids[i], mu[pos[i]:pos[i] + 3], S[pos[i]:pos[i] + 3, pos[i]:pos[i] + 3].reshape(-1)) for i in drop]
    assert len(drop) == 22 and 22 * 12 > 256
    pos, cod = _remove_exact(g, pos, cod, drop)
    assert g.numArchived() == 24
    ids = [r for i, r in enumerate(ids) if i not in drop]
    mu, S = g.getFullState(), g.getFullSigma()
    tab = g.getPointsTable()
    assert np.array_equal(tab, _expected_table(g, mu, S, pos, cod, ids, archived))
    assert int(tab.any(axis=1).sum()) == 25                              # 24 archived rows and the one live XYZ feature


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["dense_convert", "convert_across_1024"])
def test_convert_is_exact_outside_the_converted_features(name, dtype):
    _run_case(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_convert_and_export(dtype):
    g, (r, mu, S) = _run_case("sparse_convert", dtype)
    pts = g.getPointsFeatures()
    ids, _ = g.featureIds()
    assert np.array_equal(pts, _expected_table(g, mu, S, r.pos, r.coding, np.arange(len(r.pos)), []))
    assert not pts[r.coding == 0].any() and pts[r.coding != 0].all() and int((r.coding != 0).sum()) == 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_and_none(dtype):
    """The empty map (n = camera_dim, N = 0), a feature added to it again, and the removal of nothing."""
    g, pos, cod = _filter(20, dtype)
    mu, S = _inject(g, pos, cod)
    g.removeFeatures([])
    _same_layout(g, pos, cod)
    assert np.array_equal(g.getFullState(), mu) and np.array_equal(g.getFullSigma(), S)
    _invariants(g, S)
    npos, ncod = _remove_exact(g, pos, cod, tuple(range(20)))
    assert g.numOfFeatures() == 0 and g.stateDim() == 14 and len(npos) == 0
    S0 = g.getFullSigma()
    assert g.addFeature((200.0, 150.0)) == 1
    S1 = g.getFullSigma()
    assert g.stateDim() == 20 and np.array_equal(S1[:14, :14], S0) and np.array_equal(S1, S1.T)
    assert np.isfinite(S1).all() and S1[14:, 14:].any() and g.checkInvariants()[0] == 0.0
    assert list(g.featureLayout()[0]) == [14]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ping_pong_extents(dtype):
    """Streaming predict flips between the two Sigma buffers; after a large removal both carry a larger old extent than
    the live block, and every step must leave the padding exactly zero and the pass-through block untouched."""
    g, pos, cod = _filter(172, dtype)
    g.set_option(0, 1)                                  # EKF_OPT_PROPAGATE_STREAMING
    cd = g.camera_dim
    _inject(g, pos, cod)
    pix = o.synthetic_pixels(oracle_cfg(), 70, seed=77)
    state = dict(pos=pos, cod=cod, added=0)

    def remove(drop):
        mu, S = g.getFullState(), g.getFullSigma()
        e_mu, e_S, npos, ncod = rr.after_remove(mu, S, state["pos"], state["cod"], cd, drop)
        g.removeFeatures(list(drop))
        _same_layout(g, npos, ncod)
        S2 = g.getFullSigma()
        assert np.array_equal(g.getFullState(), e_mu) and np.array_equal(S2, e_S)
        assert g.checkInvariants()[0] == 0.0
        state.update(pos=npos, cod=ncod)

    def predict():
        S = g.getFullSigma()
        g.predict()
        S2 = g.getFullSigma()
        assert np.array_equal(S2[cd:, cd:], S[cd:, cd:]) and np.isfinite(S2).all()
        assert g.checkInvariants()[0] == 0.0

    def add(count):
        for _ in range(count):
            S, n = g.getFullSigma(), g.stateDim()
            assert g.addFeature(pix[state["added"]]) == 1
            state["added"] += 1
            S2 = g.getFullSigma()
            assert g.stateDim() == n + 6 and np.array_equal(S2[:n, :n], S)
            assert np.array_equal(S2[n:, :], S2[:, n:].T) and np.isfinite(S2).all()
            assert g.checkInvariants()[0] == 0.0
        state["pos"], state["cod"] = g.featureLayout()

    remove(tuple(range(3, 172, 1))[:100])               # n 1046 -> 446: buffer 0 keeps an extent of 1046
    predict()                                           # ... and is the target of this flip
    add(60)
    remove(tuple(range(0, 132, 13))[:10])
    predict()
    add(10)
    assert g.numOfFeatures() == 132
    remove(tuple(range(100, 130)))                      # n 806 -> 626, into the buffer the last removal left at 746
    assert g.stateDim() == 626


# ---- ekf_check_invariants must see a NaN ---------------------------------------------------------------------------

def _hip():
    """The HIP runtime the library itself has loaded (the process's own copy, found in its memory map)."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    return C.CDLL(path)


def _poke(g, row, col, value):
    """One element of the CURRENT device Sigma buffer, padding included, through hipMemcpy."""
    _, s, ld = g.device_pointers()
    n_pad = -(-(g.camera_dim + 6 * 32) // 128) * 128                     # capacity 32 below
    assert ld == n_pad and 0 <= row < n_pad and 0 <= col < ld
    g.synchronize()
    v = np.array([value], g.dtype)
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(s + (row * ld + col) * v.itemsize), v.ctypes.data_as(C.c_void_p), C.c_size_t(v.itemsize), 1) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_invariants_sees_a_nan(dtype):
    g, pos, cod = _filter(20, dtype, capacity=32)
    mu, S = _inject(g, pos, cod)
    n = g.stateDim()
    assert n == 134
    nan = np.full((1, 1), np.nan, dtype)
    finite = lambda: all(np.isfinite(x) for x in g.checkInvariants())
    _invariants(g, S)
    # an off-diagonal live entry and its mirror
    g.setSigmaBlock(nan, 40, 97)
    g.setSigmaBlock(nan, 97, 40)
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and np.isnan(asym) and np.isnan(big)
    # one side only
    g.setSigmaBlock(S[40:41, 97:98], 40, 97)
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and np.isnan(asym) and np.isnan(big)
    g.setSigmaBlock(S[97:98, 40:41], 97, 40)
    _invariants(g, S)
    g.setSigmaBlock(nan, 40, 97)                                         # ... and the other side
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and np.isnan(asym) and np.isnan(big)
    g.setSigmaBlock(S[40:41, 97:98], 40, 97)
    _invariants(g, S)
    # a diagonal entry: the live maximum only
    g.setSigmaBlock(nan, 50, 50)
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and asym == 0.0 and np.isnan(big)
    g.setSigmaBlock(S[50:51, 50:51], 50, 50)
    _invariants(g, S)
    # the padding: beside the live block, below it, and in the buffer's last element
    for (row, col) in ((10, n), (n, 10), (255, 255)):
        _poke(g, row, col, np.nan)
        pad, asym, big = g.checkInvariants()
        assert np.isnan(pad) and asym == 0.0 and big == float(np.float32(np.abs(S).max())), (row, col, pad, asym, big)
        assert not (pad == 0.0 and asym <= 1e-6 * big)                   # the form every other test asserts
        _poke(g, row, col, 0.0)
        assert finite()
    _invariants(g, S)
    assert np.array_equal(g.getFullSigma(), S)
