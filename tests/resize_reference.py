"""Reference of the map-resizing operations (remove, convert) in numpy alone: no GPU, no import of the package.

A resize is mostly a copy: an entry of the new Sigma whose row and column are pass-through equals one entry of the old
Sigma bit for bit, in either precision.  Only the rows and columns of a converted feature are arithmetic
(Sigma' = J Sigma J^T with the 3 x 6 block J_y of k_linearity), and there the error is bounded element by element by
u * A, A = |J| |Sigma| |J|^T.  `patterned_state` builds a state on which a misplaced entry cannot hide: every entry of
the upper triangle of Sigma and every entry of mu is a different number, exactly representable in fp32.

`column_paths` restates FeatureTable::compacted (csrc/ekf_feature_table.hpp) and says which of the index-dependent
paths of k_compact_transform (csrc/ekf_kernels.hpp) a case takes; CASES is the table the GPU test runs
(tests/test_gpu_resize_exact.py) and the CPU test checks the coverage of (tests/test_oracle_resize.py)."""
import collections

import numpy as np

COMPACT_COLS = 1024          # columns of the new matrix per workgroup of k_compact_transform (256 lanes x 4)
COMPACT_ROWS = 32            # rows per workgroup (kCompactRows), walked in groups of ROW_GROUP
ROW_GROUP = 8
SIGMA_SHIFT = 6              # Sigma[i, j] = (j (j + 1) / 2 + i + 1) * 2^-6, i <= j: below 2^24 * 2^-6 for n <= 2200
MU_SHIFT = 16                # every entry of mu is an integer multiple of 2^-16 below 2^24 * 2^-16
MAX_N = 2200


def layout(n_feat, camera_dim, xyz=()):
    """(pos, coding) of `n_feat` features in insertion order, those listed in `xyz` in XYZ coding (1), the rest
    inverse depth (0)."""
    coding = np.zeros(n_feat, np.int32)
    coding[list(xyz)] = 1
    size = np.where(coding != 0, 3, 6)
    pos = camera_dim + np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int32) if n_feat else np.zeros(0, np.int32)
    return pos.astype(np.int32), coding


def state_dim(pos, coding, camera_dim):
    return int(camera_dim if len(pos) == 0 else pos[-1] + (3 if coding[-1] else 6))


def _m(theta, phi):
    return np.array([np.sin(theta) * np.cos(phi), -np.sin(phi), np.cos(theta) * np.cos(phi)])


def linearity_index(mu, S, p):
    """L_d = 4 sigma_rho |d^T m| / (rho^2 |d|^2) of the inverse-depth feature at state offset p, in fp64 (sigma_rho is
    the VARIANCE Sigma[p + 5, p + 5], as in k_linearity and the reference)."""
    mu = np.asarray(mu, np.float64)
    theta, phi, rho = mu[p + 3], mu[p + 4], mu[p + 5]
    m = _m(theta, phi)
    d = mu[p:p + 3] + m / rho - mu[0:3]
    return 4.0 * float(S[p + 5, p + 5]) * abs(float(d @ m)) / (rho * rho * float(d @ d))


def patterned_state(pos, coding, camera_dim, dtype, convert=()):
    """mu, Sigma of the given layout in `dtype`: Sigma exactly symmetric, the entries of its upper triangle pairwise
    distinct, those of mu pairwise distinct, all exactly representable in fp32; theta, phi in (-1, 1) and rho in
    [0.1, 2] for every inverse-depth feature; L_d <= 1e-4 for the features in `convert` and >= 1 for every other
    inverse-depth feature (the kernel converts below 0.01), asserted in fp64."""
    pos, coding = np.asarray(pos), np.asarray(coding)
    n = state_dim(pos, coding, camera_dim)
    assert n <= MAX_N, n
    j = np.arange(n, dtype=np.int64)
    tri = (j * (j + 1) // 2)[None, :] + j[:, None] + 1                   # [i, j], valid for i <= j
    up = np.triu(tri)
    S = (up + np.triu(tri, 1).T).astype(np.float64) * 2.0 ** -SIGMA_SHIFT
    # mu in units of 2^-16: the residue mod 4 keeps the four kinds of entries apart, a multiplier coprime to the
    # modulus keeps the entries of one kind apart
    q = 4 * (np.arange(n, dtype=np.int64) + 1)                           # camera, anchors, XYZ points: (0, 0.135)
    convert = set(int(c) for c in convert)
    for i, (p, c) in enumerate(zip(pos, coding)):
        if c:
            assert i not in convert, "an XYZ feature cannot be converted"
            continue
        q[p + 3] = 4 * ((37 * p) % 28000 - 14000) + 1                    # theta in (-0.86, 0.86)
        q[p + 4] = 4 * ((53 * p) % 28000 - 14000) + 2                    # phi   in (-0.86, 0.86)
        q[p + 5] = 4 * (1700 + (29 * p) % 30000) + 3                     # rho   in (0.10, 1.94)
        if i in convert:
            S[p + 5, p + 5] = (i + 1) * 2.0 ** -32                       # < 6e-7: below every other entry (>= 2^-6)
    mu = q.astype(np.float64) * 2.0 ** -MU_SHIFT
    for i, (p, c) in enumerate(zip(pos, coding)):
        if c:
            continue
        assert -1.0 < mu[p + 3] < 1.0 and -1.0 < mu[p + 4] < 1.0 and 0.1 <= mu[p + 5] <= 2.0
        L = linearity_index(mu, S, p)
        assert (L <= 1e-4) if i in convert else (L >= 1.0), (i, L)
    return mu.astype(dtype), S.astype(dtype)


def sources(pos, coding, camera_dim, drop=(), conv=()):
    """FeatureTable::compacted restated: per NEW state index its first OLD index (msrc) and -1 for a pass-through
    entry or 3 * feature + component for a converted one (mconv); then the new pos and coding."""
    drop, conv = set(int(d) for d in drop), set(int(c) for c in conv)
    msrc, mconv = list(range(camera_dim)), [-1] * camera_dim
    npos, ncod = [], []
    for i, (p, c) in enumerate(zip(pos, coding)):
        if i in drop:
            continue
        npos.append(len(msrc))
        if i in conv:
            assert c == 0
            msrc += [int(p)] * 3
            mconv += [3 * i + e for e in range(3)]
            ncod.append(1)
        else:
            fs = 3 if c else 6
            msrc += [int(p) + e for e in range(fs)]
            mconv += [-1] * fs
            ncod.append(int(c))
    return (np.array(msrc, np.int64), np.array(mconv, np.int64), np.array(npos, np.int32), np.array(ncod, np.int32))


def after_remove(mu, S, pos, coding, camera_dim, drop):
    """Expected mu, Sigma, pos, coding after the features `drop` are removed: fancy indexing alone."""
    msrc, _, npos, ncod = sources(pos, coding, camera_dim, drop=drop)
    return mu[msrc].copy(), S[np.ix_(msrc, msrc)].copy(), npos, ncod


def jacobian_y(theta, phi, rho):
    """The 3 x 6 Jacobian of y = a + m(theta, phi) / rho (the formulae of k_linearity), in fp64."""
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    J = np.zeros((3, 6))
    J[:, 0:3] = np.eye(3)
    J[:, 3] = [ct * cp / rho, 0.0, -st * cp / rho]
    J[:, 4] = [-st * sp / rho, -cp / rho, -ct * sp / rho]
    J[:, 5] = -_m(theta, phi) / (rho * rho)
    return J


Converted = collections.namedtuple("Converted", "ref ref_mu pos coding exact A mu_exact A_mu")


def after_convert(mu, S, pos, coding, camera_dim, conv):
    """The features `conv` converted all at once, in fp64 from the given numbers: ref = J Sigma J^T, ref_mu, the new
    layout, `exact` (true where neither row nor column belongs to a converted feature: ref is a copy there),
    A = |J| |Sigma| |J|^T, and for mu the pass-through mask and A_mu = |anchor| + |m / rho|."""
    msrc, mconv, npos, ncod = sources(pos, coding, camera_dim, conv=conv)
    mu64, S64 = np.asarray(mu, np.float64), np.asarray(S, np.float64)
    n_new, n = len(msrc), len(mu64)
    J = np.zeros((n_new, n))
    ref_mu, A_mu = mu64[msrc].copy(), np.abs(mu64[msrc])
    plain = mconv < 0
    J[np.flatnonzero(plain), msrc[plain]] = 1.0
    for ip in np.flatnonzero(~plain):
        p, e = msrc[ip], int(mconv[ip] % 3)
        theta, phi, rho = mu64[p + 3], mu64[p + 4], mu64[p + 5]
        J[ip, p:p + 6] = jacobian_y(theta, phi, rho)[e]
        mr = _m(theta, phi)[e] / rho
        ref_mu[ip] = mu64[p + e] + mr
        A_mu[ip] = abs(mu64[p + e]) + abs(mr)
    ref = J @ S64 @ J.T
    A = np.abs(J) @ np.abs(S64) @ np.abs(J).T
    exact = plain[:, None] & plain[None, :]
    ref[exact] = S64[np.ix_(msrc, msrc)][exact]                          # (a copy, whatever order the product summed zeros in)
    return Converted(ref, ref_mu, npos, ncod, exact, A, plain, A_mu)


def worst_ratio(got, ref, A, u):
    """max |got - ref| / (u A) over the given entries; an entry whose A is 0 is a sum of exact zeros and must be 0."""
    got, ref, A = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, A))
    zero = A == 0
    assert not got[zero].any(), "an entry whose magnitude bound A is 0 is not exactly 0"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got - ref)[~zero] / (u * A[~zero])))


def column_paths(pos, coding, camera_dim, drop=(), conv=()):
    """Which index-dependent paths of k_compact_transform the resize takes.  A lane owns the four new columns
    [4g, 4g + 4); it moves them as one 16-byte run only when their sources are contiguous and none is converted.

    blocks          column blocks of the grid (blockIdx.x < blocks)
    mod4, mod32     n_new % 4 (columns of the scalar tail group), n_new % 32 (rows of the last row block)
    removed_phases  {c % 4}: c the new column at which the sources jump over a removed feature -- 0 is a jump between
                    two groups, 1..3 a jump inside one (a removed last feature leaves no jump and is not counted)
    converted_phases {c % 4}: c the first new column of a converted feature
    mixed_row_group a row group of eight that holds converted and plain rows
    converted_pair  two different converted features: their 3 x 3 blocks lie on both sides of the diagonal"""
    msrc, mconv, _, _ = sources(pos, coding, camera_dim, drop, conv)
    n_new = len(msrc)
    jumps = [c for c in range(1, n_new) if mconv[c] < 0 and mconv[c - 1] < 0 and msrc[c] != msrc[c - 1] + 1]
    starts = [c for c in range(n_new) if mconv[c] >= 0 and mconv[c] % 3 == 0]
    mixed = False
    for r0 in range(0, n_new, ROW_GROUP):
        g = mconv[r0:min(r0 + ROW_GROUP, n_new)] >= 0
        mixed = mixed or bool(g.any() and not g.all())
    return dict(n_new=n_new, blocks=(n_new + COMPACT_COLS - 1) // COMPACT_COLS, mod4=n_new % 4, mod32=n_new % COMPACT_ROWS,
                removed_phases={c % 4 for c in jumps}, converted_phases={c % 4 for c in starts},
                mixed_row_group=mixed, converted_pair=len(set(int(c) for c in conv)) >= 2)


# The cases of tests/test_gpu_resize_exact.py: name -> (camera_dim, features, those in XYZ coding before the
# operation, operation, its features).  The smallest shapes that reach each path; what each is for stands beside it.
Case = collections.namedtuple("Case", "camera_dim n_feat xyz op arg")
_SEVENTH = tuple(range(6, 180, 7))
CASES = collections.OrderedDict([
    # n 1046 -> 1034: a second column block of 10 columns, n_new % 4 = 2
    ("two_blocks_tail", Case(14, 172, (), "remove", (5, 100))),
    # n 1046 (two column blocks of sources) -> 1016 (one); the test adds two features after it, back across 1024
    ("across_1024", Case(14, 172, (), "remove", (0, 40, 41, 99, 171))),
    # n 1030 -> 1024: a full last group of four, no tail (camera_dim 13: 13 + 168 * 6 + 3)
    ("exactly_1024", Case(13, 170, (60,), "remove", (7,))),
    # n_new 1055 (% 4 = 3, % 32 = 31), 1052, 1025 (% 4 = 1, % 32 = 1: a second column block of ONE column; 171 features,
    # since 14 + 6 a + 3 b = 1 (mod 32) has no solution between 930 and 1120 but 1025)
    ("odd_sizes_1", Case(14, 175, (20,), "remove", (100,))),
    ("odd_sizes_2", Case(14, 175, (20, 90), "remove", (3,))),
    ("odd_sizes_3", Case(14, 171, (20, 90, 91), "remove", (150,))),
    # every seventh feature XYZ; feature 0, the last one, two neighbours (30, 31), both neighbours of an XYZ feature
    # (12 and 14 around 13: two jumps three columns apart), XYZ features (27, 90): a jump at each of the four phases
    ("phases", Case(14, 180, _SEVENTH, "remove", (0, 12, 14, 27, 30, 31, 58, 90, 101, 133, 161, 179))),
    # n 2084 -> 2066: blockIdx.x = 2
    ("three_blocks", Case(14, 345, (), "remove", (0, 170, 344))),
    # row groups of eight that mix converted and plain rows beside run lanes, neighbours (50, 51), the last feature
    ("sparse_convert", Case(14, 180, (), "convert", (3, 50, 51, 120, 179))),
    # every second feature: no run of four anywhere in the feature columns, n_new = 14 + 86 * 9 = 788
    ("dense_convert", Case(14, 172, (), "convert", tuple(range(0, 172, 2)))),
    # n 1214 -> 1004: a conversion whose sources span two column blocks
    ("convert_across_1024", Case(14, 200, (), "convert", tuple(range(10, 150, 2)))),
])
CONVERT_CASES = [k for k, c in CASES.items() if c.op == "convert"]


def case_paths(name):
    c = CASES[name]
    pos, cod = layout(c.n_feat, c.camera_dim, c.xyz)
    drop, conv = (c.arg, ()) if c.op == "remove" else ((), c.arg)
    return column_paths(pos, cod, c.camera_dim, drop, conv)


def assert_coverage():
    """The union of CASES reaches every path the issue lists; a case that stops doing so is changed, not this."""
    paths = {k: case_paths(k) for k in CASES}
    assert {p["blocks"] for p in paths.values()} >= {1, 2, 3}
    assert {p["mod4"] for p in paths.values()} == {0, 1, 2, 3}
    assert {p["mod32"] for p in paths.values()} >= {1, 31}
    assert set().union(*(p["removed_phases"] for p in paths.values())) == {0, 1, 2, 3}
    assert set().union(*(p["converted_phases"] for p in paths.values())) == {0, 1, 2, 3}
    assert any(p["mixed_row_group"] for p in paths.values())
    assert any(p["converted_pair"] for p in paths.values())
    # ... and each case gives what its row of the table claims
    expect = dict(two_blocks_tail=(1034, 2, 2), across_1024=(1016, 1, 0), exactly_1024=(1024, 1, 0),
                  odd_sizes_1=(1055, 2, 3), odd_sizes_2=(1052, 2, 0), odd_sizes_3=(1025, 2, 1), three_blocks=(2066, 3, 2),
                  dense_convert=(788, 1, 0), convert_across_1024=(1004, 1, 0))
    for k, (n_new, blocks, mod4) in expect.items():
        assert (paths[k]["n_new"], paths[k]["blocks"], paths[k]["mod4"]) == (n_new, blocks, mod4), (k, paths[k])
    assert paths["odd_sizes_1"]["mod32"] == 31 and paths["odd_sizes_3"]["mod32"] == 1
    assert paths["phases"]["removed_phases"] == {0, 1, 2, 3}
    assert paths["sparse_convert"]["converted_phases"] == {0, 1, 2, 3}
    assert paths["sparse_convert"]["mixed_row_group"] and paths["sparse_convert"]["converted_pair"]
    return paths
