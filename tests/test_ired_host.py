"""
Host side of the iRED analysis (spinrelax_amd/ired.py): the window tables, the eigen-decomposition step and the reduction
over windows.  No GPU: the matrix itself is built here from its definition for a rigid body, where the answer is known.
"""
import numpy as np
import pytest

from spinrelax_amd import ired


def test_rigid_matrix_gives_S2_one_and_rank_five():
    """M[i][j] = P2(b_i . b_j) for fixed unit vectors: by the addition theorem M = (4 pi / 5) Y Y^T with the five l = 2
    harmonics, rank <= 5, so nothing is left outside five global modes: S2 = 1, lambda_6 .. lambda_N = 0."""
    rng = np.random.default_rng(3)
    b = rng.standard_normal((12, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    M = 1.5 * (b @ b.T) ** 2 - 0.5
    S2, lam = ired.ired_S2(M)
    assert S2.shape == (1, 12) and lam.shape == (1, 12)
    assert np.all(np.diff(lam[0]) <= 0)
    assert np.max(np.abs(S2 - 1.0)) < 1e-12
    assert np.max(np.abs(lam[0, 5:])) < 1e-12
    assert abs(lam.sum() - 12.0) < 1e-12
    # several windows at once, and fewer global modes: the fifth mode then counts as internal motion
    S2b, lamb = ired.ired_S2(np.stack((M, M)), n_global=4)
    np.testing.assert_array_equal(lamb[0], lamb[1])
    lam_np, vec_np = np.linalg.eigh(M)
    assert np.max(np.abs(S2b[0] - (1.0 - lam_np[-5] * vec_np[:, -5] ** 2))) < 1e-12


def test_window_tables():
    ws, wl = ired.ired_windows([1000, 777], dt=10.0, window=3000.0)
    assert ws.dtype == np.int64 and wl.dtype == np.int64
    assert ws.tolist() == [0, 300, 600, 1000, 1300] and wl.tolist() == [300] * 5
    ws, wl = ired.ired_windows([1000, 777], dt=10.0)
    assert ws.tolist() == [0, 1000] and wl.tolist() == [1000, 777]
    ws, wl = ired.ired_windows([1000, 777], dt=10.0, tau=600.0)              # 5 tau = 300 frames
    assert ws.tolist() == [0, 300, 600, 1000, 1300] and wl.tolist() == [300] * 5
    ws, wl = ired.ired_windows([1000, 777], dt=10.0, window=8000.0, tau=600.0)   # an explicit window wins over tau
    assert ws.tolist() == [0] and wl.tolist() == [800]
    ws, wl = ired.ired_windows([100, 777], dt=10.0, window=3000.0)           # a file shorter than a window gives none
    assert ws.tolist() == [100, 400] and wl.tolist() == [300, 300]
    with pytest.raises(ValueError):
        ired.ired_windows([1000], dt=10.0, window=5.0)


def test_reduce_over_windows():
    rng = np.random.default_rng(5)
    one = rng.random((1, 7))
    S2, dS2 = ired.ired_reduce(one)
    np.testing.assert_array_equal(S2, one[0])
    np.testing.assert_array_equal(dS2, np.zeros(7))
    four = rng.random((4, 7))
    S2, dS2 = ired.ired_reduce(four)
    mean = four.sum(axis=0) / 4.0
    std = np.sqrt(((four - mean) ** 2).sum(axis=0) / 4.0)
    assert np.max(np.abs(S2 - mean)) < 1e-15
    assert np.max(np.abs(dS2 - std / (np.sqrt(4.0) - 1.0))) < 1e-15


def test_too_few_vectors_are_refused():
    M = np.eye(5)
    with pytest.raises(ValueError):
        ired.ired_S2(M)
    with pytest.raises(ValueError):
        ired.ired_S2(np.eye(4), n_global=4)
    ired.ired_S2(np.eye(6))
    with pytest.raises(ValueError):
        ired.calculate_iRED([np.zeros((10, 5, 3), dtype=np.float32)], dt=1.0)
