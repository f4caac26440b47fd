"""The numpy reference of the resize operations (tests/resize_reference.py) against the oracle, its own guarantees, and
an fp32 emulation of k_compact_transform's summation order against its fp64 value.  No GPU.

The GPU test (tests/test_gpu_resize_exact.py) holds the kernels to this reference bit for bit where a resize copies
and to 40 u A where it computes; this file is what makes the reference itself trustworthy."""
import numpy as np
import pytest

import ekf_oracle as o
import resize_reference as rr

CEILING = 40.0               # of |result - ref| / (u A) for the entries of converted features ("Resizing the map")


def _mixed_oracle():
    """N = 12 in fp64 after one predict + update (a realistic, dense Sigma), features 2 and 7 converted to XYZ."""
    ref = o.build_scenario(o.StructuredFilter, o.Config.kinect(), 12, np.float64)
    ref.predict()
    vis = ref.visible_indices()
    ref.update(o.synthetic_measurements(ref, vis), vis)
    for i in (2, 7):
        p = ref.features[i].position_in_state
        ref.Sigma[p + 5, p + 5] = 1e-9
    assert ref.convert2xyz_if_linear_all() == 2
    return ref


def _layout_of(ref):
    return (np.array([f.position_in_state for f in ref.features], np.int32),
            np.array([f.coding for f in ref.features], np.int32))


def test_after_remove_is_the_oracle_bit_for_bit():
    ref = _mixed_oracle()
    pos, cod = _layout_of(ref)
    drop = (0, 2, 4, 9, 11)                                     # the first, the last, an XYZ feature among them
    mu, S, npos, ncod = rr.after_remove(ref.mu, ref.Sigma, pos, cod, ref.camera_dim, drop)
    for i in sorted(drop, reverse=True):                        # descending, like vR.cpp:1296-1299
        ref.remove_feature(i)
    p2, c2 = _layout_of(ref)
    assert list(npos) == list(p2) and list(ncod) == list(c2)
    assert np.array_equal(mu, ref.mu) and np.array_equal(S, ref.Sigma)


def test_after_convert_is_the_oracle_up_to_rounding():
    ref = _mixed_oracle()
    pos, cod = _layout_of(ref)
    conv = (0, 3, 4, 11)                                        # the first, two neighbours, the last
    for i in conv:
        p = ref.features[i].position_in_state
        ref.Sigma[p + 5, p + 5] = 1e-9
    c = rr.after_convert(ref.mu, ref.Sigma, pos, cod, ref.camera_dim, conv)
    S_old = ref.Sigma.copy()
    msrc, _, _, _ = rr.sources(pos, cod, ref.camera_dim, conv=conv)
    done = [i for i in range(12) if ref.convert2xyz_if_linear(i)]          # one feature at a time
    assert tuple(done) == conv
    p2, c2 = _layout_of(ref)
    assert list(c.pos) == list(p2) and list(c.coding) == list(c2)
    assert c.ref.shape == ref.Sigma.shape and not c.exact.all() and c.exact.any()
    assert np.array_equal(ref.Sigma[c.exact], S_old[np.ix_(msrc, msrc)][c.exact])     # what is a copy is a copy in the oracle
    assert np.array_equal(c.ref[c.exact], ref.Sigma[c.exact])
    u = 2.0 ** -53
    rest = ~c.exact
    worst = rr.worst_ratio(ref.Sigma[rest], c.ref[rest], c.A[rest], u)
    print(f"oracle one-at-a-time against J Sigma J^T all at once: {worst:.2f} u A")
    assert 0.0 < worst <= 8.0, worst
    assert np.array_equal(ref.mu[c.mu_exact], c.ref_mu[c.mu_exact])
    worst_mu = rr.worst_ratio(ref.mu[~c.mu_exact], c.ref_mu[~c.mu_exact], c.A_mu[~c.mu_exact], u)
    assert worst_mu <= 8.0, worst_mu


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_patterned_state_keeps_its_promises_at_the_largest_size(dtype):
    big = rr.CASES["three_blocks"]
    assert max(c.n_feat for c in rr.CASES.values()) == big.n_feat
    conv = tuple(range(1, big.n_feat, 3))
    pos, cod = rr.layout(big.n_feat, big.camera_dim, big.xyz)
    mu, S = rr.patterned_state(pos, cod, big.camera_dim, dtype, convert=conv)
    n = rr.state_dim(pos, cod, big.camera_dim)
    assert n == 2084 and mu.shape == (n,) and S.shape == (n, n) and mu.dtype == dtype and S.dtype == dtype
    assert np.array_equal(S, S.T)
    upper = S[np.triu_indices(n)]
    assert np.unique(upper).size == upper.size and np.unique(mu).size == n
    mu64, S64 = rr.patterned_state(pos, cod, big.camera_dim, np.float64, convert=conv)
    assert np.array_equal(S.astype(np.float64), S64) and np.array_equal(S64.astype(np.float32).astype(np.float64), S64)
    assert np.array_equal(mu.astype(np.float64), mu64) and np.array_equal(mu64.astype(np.float32).astype(np.float64), mu64)
    for i, p in enumerate(pos):
        assert -1 < mu[p + 3] < 1 and -1 < mu[p + 4] < 1 and 0.1 <= mu[p + 5] <= 2
        L = rr.linearity_index(mu64, S64, p)
        assert (L <= 1e-4) if i in conv else (L >= 1.0)


def test_patterned_state_on_a_mixed_layout():
    pos, cod = rr.layout(9, 13, xyz=(0, 4, 8))
    mu, S = rr.patterned_state(pos, cod, 13, np.float32, convert=(1, 7))
    assert list(pos) == [13, 16, 22, 28, 34, 37, 43, 49, 55] and S.shape == (58, 58)
    assert np.array_equal(S, S.T) and np.unique(S[np.triu_indices(58)]).size == 58 * 59 // 2
    with pytest.raises(AssertionError):
        rr.patterned_state(pos, cod, 13, np.float32, convert=(4,))          # an XYZ feature


def test_column_paths_on_layouts_with_known_answers():
    # camera 14, four inverse-depth features (n = 38); remove feature 1: columns 14..19 stay, 20 jumps to old 26
    pos, cod = rr.layout(4, 14)
    msrc, mconv, npos, ncod = rr.sources(pos, cod, 14, drop=(1,))
    assert list(msrc) == list(range(20)) + list(range(26, 38)) and (mconv == -1).all()
    assert list(npos) == [14, 20, 26] and not ncod.any()
    p = rr.column_paths(pos, cod, 14, drop=(1,))
    assert p == dict(n_new=32, blocks=1, mod4=0, mod32=0, removed_phases={0}, converted_phases=set(),
                     mixed_row_group=False, converted_pair=False)
    # the last feature removed: no jump at all; the first: a jump at column 14
    assert rr.column_paths(pos, cod, 14, drop=(3,))["removed_phases"] == set()
    assert rr.column_paths(pos, cod, 14, drop=(0,))["removed_phases"] == {2}
    # two neighbours are one jump
    assert rr.column_paths(pos, cod, 14, drop=(0, 1))["removed_phases"] == {2}
    # convert feature 1: new columns 20, 21, 22 all read from old 20, the rest shifts by three
    msrc, mconv, npos, ncod = rr.sources(pos, cod, 14, conv=(1,))
    assert list(msrc) == list(range(20)) + [20, 20, 20] + list(range(26, 38))
    assert list(mconv) == [-1] * 20 + [3, 4, 5] + [-1] * 12 and list(npos) == [14, 20, 23, 29] and list(ncod) == [0, 1, 0, 0]
    p = rr.column_paths(pos, cod, 14, conv=(1,))
    assert p == dict(n_new=35, blocks=1, mod4=3, mod32=3, removed_phases=set(), converted_phases={0},
                     mixed_row_group=True, converted_pair=False)
    # a feature of eight rows' worth: camera 13 with XYZ features 0 and 1, converting 2 and 3 fills rows 19..24:
    # the group 16..23 mixes, and two converted features make a pair
    pos, cod = rr.layout(5, 13, xyz=(0, 1))
    p = rr.column_paths(pos, cod, 13, conv=(2, 3))
    assert p["converted_phases"] == {19 % 4, 22 % 4} and p["mixed_row_group"] and p["converted_pair"] and p["n_new"] == 31
    # sizes around a column block
    pos, cod = rr.layout(172, 14)
    assert [rr.column_paths(pos, cod, 14, drop=range(k))["blocks"] for k in (0, 3, 4)] == [2, 2, 1]
    pos, cod = rr.layout(345, 14)
    assert rr.column_paths(pos, cod, 14)["blocks"] == 3 and rr.column_paths(pos, cod, 14, drop=(1,))["n_new"] == 2078


def test_the_cases_reach_every_path():
    rr.assert_coverage()


def _emulate_f32(mu, S, pos, cod, camera_dim, conv):
    """k_linearity's J_y and k_compact_transform's sums in float32, every operation rounded once, in the written order
    (no FMA; the kernel fuses each multiply-add, which rounds once where this rounds twice): the entries of converted
    features only; the rest of the result is NaN."""
    f = np.float32
    msrc, mconv, _, _ = rr.sources(pos, cod, camera_dim, conv=conv)
    n_new = len(msrc)
    out = np.full((n_new, n_new), np.nan, f)
    Jy = {}
    for i in conv:
        p = pos[i]
        th, ph, ro = f(mu[p + 3]), f(mu[p + 4]), f(mu[p + 5])
        st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
        assert st.dtype == f
        m = [st * cp, -sp, ct * cp]
        J = np.zeros((3, 6), f)
        J[0, 0] = J[1, 1] = J[2, 2] = 1
        J[:, 3] = [ct * cp / ro, 0, -st * cp / ro]
        J[:, 4] = [-st * sp / ro, -cp / ro, -ct * sp / ro]
        J[:, 5] = [-m[k] / (ro * ro) for k in range(3)]
        Jy[i] = J
    plain = np.flatnonzero(mconv < 0)
    first = {i: int(np.flatnonzero(mconv == 3 * i)[0]) for i in conv}          # first new index of each converted feature
    for i in conv:
        p, c0 = pos[i], first[i]
        # plain row, converted column (and its mirror, the same products in the same sequence)
        for e in range(3):
            acc = np.zeros(len(plain), f)
            for b in range(6):
                acc = acc + S[msrc[plain], p + b] * Jy[i][e, b]
            out[plain, c0 + e] = acc
            out[c0 + e, plain] = acc
        # converted by converted, lower triangle: sum_a Jy_i[a] (sum_b S[i + a][j + b] Jy_j[b]); the upper one mirrors it
        for j in conv:
            if first[j] > c0:
                continue
            q = pos[j]
            B = S[p:p + 6, q:q + 6]
            inner = np.zeros((6, 3), f)                                    # [a, g]
            for b in range(6):
                inner = inner + B[:, b, None] * Jy[j][None, :, b]
            blk = np.zeros((3, 3), f)                                      # [e, g]
            for a in range(6):
                blk = blk + Jy[i][:, a, None] * inner[None, a, :]
            if i == j:
                blk = np.tril(blk) + np.tril(blk, -1).T
            out[c0:c0 + 3, first[j]:first[j] + 3] = blk
            out[first[j]:first[j] + 3, c0:c0 + 3] = blk.T
    return out


def test_fp32_summation_order_stays_under_the_ceiling():
    worst = {}
    for name in rr.CONVERT_CASES:
        c = rr.CASES[name]
        pos, cod = rr.layout(c.n_feat, c.camera_dim, c.xyz)
        conv = c.arg
        mu, S = rr.patterned_state(pos, cod, c.camera_dim, np.float32, convert=conv)
        r = rr.after_convert(mu, S, pos, cod, c.camera_dim, conv)
        emu = _emulate_f32(mu, S, pos, cod, c.camera_dim, conv)
        rest = ~r.exact
        assert np.isfinite(emu[rest]).all() and np.isnan(emu[r.exact]).all() and (r.A[rest] > 0).all()
        assert np.array_equal(emu[rest], emu.T[rest])
        cc = (~r.mu_exact)[:, None] & (~r.mu_exact)[None, :]
        worst[name] = tuple(rr.worst_ratio(emu[k], r.ref[k], r.A[k], 2.0 ** -24) for k in (cc, rest & ~cc))
        print(f"{name}: converted x converted {worst[name][0]:.2f} u A, mixed {worst[name][1]:.2f} u A")
    assert max(max(w) for w in worst.values()) < CEILING, worst
