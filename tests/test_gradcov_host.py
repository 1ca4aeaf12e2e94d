"""Host half of the gradient-covariance maps (vi_eval_resident_gradcov_f64, kernel K2c): the packed order and its unpacking,
the launch formula restated, and the check that the case list of tests/test_gpu_resident_gradcov.py reaches every class of it.
No GPU needed.

  K2c  k_eval_resident_gradcov   NB = ceil(N / 16) = 1 .. 9 (N <= 144), any Q, no alignment condition.  A wave takes 16
       <NB>                      points, a workgroup of 4 waves 64 points per pass; groups = clamp(Q >> 14, 1, 32)
                                 (VINTERP_K2C_GROUPS: 1 .. 256) passes, npg = ceil(Q / (64 groups)) groups of points, one
                                 timestep per block, blocks in XCD order (npg rounded up to 8).  Anything else, and
                                 VINTERP_EVAL_RESIDENT=blas: the library's product plus nine row dots, in chunks of
                                 2^25 / (3 N) points."""
import numpy as np
import pytest


def k2c_geometry(N, Q, T, groups=None, blas=False):
    """The launch vi_eval_resident_gradcov_f64 chooses (vi_eval_resident_gradcov_mfma, else the library)."""
    NB = -(-N // 16)
    g = min(max(Q >> 14, 1), 32)
    if groups is not None and 1 <= groups <= 256:
        g = groups
    npg = -(-Q // (64 * g))
    kernel = not blas and 1 <= N <= 144 and (npg + 7) // 8 * 8 * T < 2 ** 31
    chunk = min(max(1, 2 ** 25 // (3 * N)), max(Q, 1))
    return dict(path='kernel' if kernel else 'library', NB=NB, shm=NB * (NB + 1) // 2 * 2048, groups=g, npg=npg,
                nblk=(npg + 7) // 8 * 8 * T, passes=min(g, -(-Q // 64)), waves=-(-Q // 16),
                chunks=-(-Q // chunk) if Q else 0, cls='NB %d%s' % (NB, ' (N%%16 %d)' % (N % 16) if N % 16 else ''))


K2C_NS = [12, 16, 18, 32, 48, 50, 64, 80, 81, 96, 112, 128, 144]
LIB_NS = [147, 288]
K2C_QS = [1, 15, 16, 17, 63, 64, 65, 260, 1029, 4100]
K2C_TS = [1, 3, 17]


def k2c_cases():
    """(N, Q, T, groups) of the integer suite: every (N, Q, T) of the eight kernel orders and the two library orders, the
    remaining NB at Q = 260, and the group settings (None: the default; the others run in a child process with
    VINTERP_K2C_GROUPS set)."""
    c = [(N, Q, T, None) for N in (12, 16, 18, 32, 50, 81, 128, 144) + tuple(LIB_NS) for Q in K2C_QS for T in K2C_TS]
    c += [(N, 260, 1, None) for N in (48, 64, 80, 96, 112)]
    c += [(N, Q, 3, g) for g in (1, 3) for N in (18, 81, 144) for Q in (63, 260, 1029, 4100)]
    return c


def case_line(N, Q, T, groups, blas=False):
    g = k2c_geometry(N, Q, T, groups, blas)
    extra = 'groups %3d npg %4d' % (g['groups'], g['npg']) if g['path'] == 'kernel' else 'chunks %d' % g['chunks']
    return 'K2c N %3d  %-16s Q %5d T %2d  %-20s %s' % (N, g['cls'], Q, T, extra, g['path'])


def test_packed_order_and_matrix_round_trip():
    from volumetricinterp_amd.estimate import GRADCOV_PAIRS, gradcov_matrix
    assert GRADCOV_PAIRS == ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    rng = np.random.default_rng(6)
    packed = rng.standard_normal((4, 6, 11))
    packed[1, 3, 5] = np.nan
    cov = gradcov_matrix(packed)
    assert cov.shape == (4, 11, 3, 3)
    assert np.array_equal(cov, np.swapaxes(cov, -1, -2), equal_nan=True)
    for k, (c, d) in enumerate(GRADCOV_PAIRS):
        assert np.array_equal(cov[..., c, d], packed[:, k, :], equal_nan=True)
        assert np.array_equal(cov[..., d, c], packed[:, k, :], equal_nan=True)
    back = np.stack([cov[..., c, d] for c, d in GRADCOV_PAIRS], axis=-2)
    assert np.array_equal(back, packed, equal_nan=True)
    one = gradcov_matrix(np.arange(6.)[:, None])                       # (6, 1): one point
    assert one.shape == (1, 3, 3)
    assert np.array_equal(one[0], [[0., 3., 4.], [3., 1., 5.], [4., 5., 2.]])
    # the error along a unit vector is sqrt(u^T cov u): along an axis the diagonal entry
    u = np.array([0., 1., 0.])
    assert np.einsum('...i,...ij,...j', u, one, u)[0] == 1.0
    for bad in (np.zeros(6), np.zeros((5, 3)), np.zeros((6, 3, 2))):
        with pytest.raises(ValueError, match='packed gradient covariances'):
            gradcov_matrix(bad)


def test_geometry_list_covers_every_class():
    """The case list of the GPU suite reaches every class of the restated launch formula."""
    cs = [(N, Q, T, g, k2c_geometry(N, Q, T, g)) for N, Q, T, g in k2c_cases()]
    ke = [x for x in cs if x[4]['path'] == 'kernel']
    le = [x for x in cs if x[4]['path'] == 'library']
    for NB in range(1, 10):
        ns = {x[0] for x in ke if x[4]['NB'] == NB}
        assert 16 * NB in ns, NB                                        # N % 16 == 0 at every NB
    assert {x[4]['NB'] for x in ke if x[0] % 16} >= {1, 2, 4, 6}        # padded rows in the last block column
    assert {x[0] for x in ke} >= {12, 16, 18, 32, 50, 81, 128, 144}
    for N in (12, 16, 18, 32, 50, 81, 128, 144):
        assert {x[1] for x in ke if x[0] == N} >= set(K2C_QS), N
    assert {x[2] for x in ke} >= set(K2C_TS) and {x[2] for x in le} >= set(K2C_TS)
    qs = {x[1] for x in ke}
    assert any(q % 16 == 0 for q in qs) and any(q % 16 for q in qs)
    assert any(q < 16 for q in qs)                                      # below one wave
    assert any(16 < q < 64 for q in qs)                                 # below one workgroup pass, more than one wave
    assert any(x[4]['npg'] > 8 for x in ke)                             # more than one round of the eight XCDs
    assert any(x[4]['npg'] % 8 for x in ke)                             # blocks that return at once
    assert {x[3] for x in ke} == {None, 1, 3}
    assert any(x[4]['groups'] == 3 and x[4]['passes'] == 3 for x in ke)              # several passes in a workgroup
    assert any(x[4]['groups'] == 3 and x[4]['passes'] < 3 for x in ke)               # ... and a Q that ends them early
    assert any(x[4]['groups'] == 3 and (x[1] - 1) % 192 < 128 and x[1] > 192 for x in ke)   # a last workgroup with empty passes
    assert all(x[3] is None or k2c_geometry(x[0], x[1], x[2])['groups'] == 1 for x in ke)    # default at these Q: 1
    assert {x[0] for x in le} == set(LIB_NS)
    assert any(x[1] % 2 for x in le) and any(x[1] > 4096 for x in le)
    # the formula itself
    assert k2c_geometry(144, 1 << 21, 1)['groups'] == 32 and k2c_geometry(144, 1 << 17, 1)['groups'] == 8
    assert k2c_geometry(144, 4100, 1)['shm'] == 90 * 1024
    assert k2c_geometry(145, 4100, 1)['path'] == 'library' and k2c_geometry(144, 4100, 1, blas=True)['path'] == 'library'
    assert k2c_geometry(144, 64 * 2 ** 28, 8, groups=1)['path'] == 'library'          # the 32-bit guard on the block count
    assert 2 ** 25 // (3 * 144) == 77672 and k2c_geometry(288, 4100, 1)['chunks'] == 1
    for x in cs:
        assert case_line(*x[:4])
