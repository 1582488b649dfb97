"""
CPU tests of the host side of the distance-weighted pair cross-correlation functions (no GPU): the new entry points in the header, the
binding and the library, what spinrelax_amd.ct.calculate_Ct_dipolar_cross and scripts/calculate-Ct-from-traj.py --dipolarCrossCt refuse
before the GPU is touched, and the two identities the formulation rests on.  The kernels: tests/test_gpu_ct_dipolar_cross.py.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import _lib
from spinrelax_amd import ct as hostct
from spinrelax_amd import hip

SCRIPT = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
NEW = {'sr_ct_dipolar_cross_max_frames': 1, 'sr_ct_dipolar_cross_f32_dev': 18, 'sr_vectors_ct_dipolar_cross_f32': 16}


def test_library_exports_the_new_entry_points():
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.sr_ct_dipolar_cross_max_frames(None) == -1                 # no context: refused on the host, nothing touched


def test_abi_declares_the_new_entry_points():
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        text = re.sub(r'/\*.*?\*/', '', fp.read(), flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'\b(int|int64_t) %s\((.*?)\);' % name, text, flags=re.S)
        assert m and len(m.group(2).split(',')) == nargs, name
    assert _lib.SIGNATURES['sr_ct_dipolar_cross_max_frames'][0] is ctypes.c_int64
    assert _lib.ABI_VERSION == 13 and re.search(r'#define SR_ABI_VERSION 13\b', text)


def test_arguments_are_checked_before_any_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError('a context was asked for before the arguments were checked')
    monkeypatch.setattr(hip, 'default_context', no_context)
    vecs = np.ones((2, 10, 3, 3), dtype=np.float32)
    good = np.ones((2, 10, 3), dtype=np.float32)
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1, 2)], [], [(0.5, 1.0)]):
        with pytest.raises(ValueError):
            hostct.calculate_Ct_dipolar_cross(vecs, bad)
    with pytest.raises(ValueError, match='replicates, frames, vectors, 3'):
        hostct.calculate_Ct_dipolar_cross(vecs[0], [(0, 1)])
    with pytest.raises(ValueError, match='shape'):
        hostct.calculate_Ct_dipolar_cross(vecs, [(0, 1)], dist=good[:, :9])
    with pytest.raises(ValueError, match='shape'):
        hostct.calculate_Ct_dipolar_cross(vecs, [(0, 1)], dist=np.ones((2, 10, 3, 1), dtype=np.float32))
    for bad in (0.0, -0.3, np.nan, np.inf):
        d = good.copy()
        d[1, 4, 2] = bad
        with pytest.raises(ValueError, match='positive and finite'):
            hostct.calculate_Ct_dipolar_cross(vecs, [(0, 1)], dist=d)
    # good arguments get as far as the context
    with pytest.raises(AssertionError, match='a context was asked for'):
        hostct.calculate_Ct_dipolar_cross(vecs, [(0, 1)], dist=good)


def test_formulation_identities():
    """P2(u . u') w w' = 1.5 (a . a')^2 - 0.5 w w' with a = u sqrt(w), and the normalised function does not depend on the reference
    distances: scaling w_i by s_i^3 and w_j by s_j^3 (another r_ref per vector) scales numerator and normaliser alike.  1e-14."""
    rng = np.random.default_rng(1)
    n = 400
    u = rng.standard_normal((2, n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    r = 0.2 + 0.3 * rng.random((2, n))

    def planes(rref):
        w = (rref[:, None] / r) ** 3
        return u * np.sqrt(w)[..., None], w

    def p2(x):
        return 1.5 * x * x - 0.5

    a, w = planes(r.min(axis=1))
    k = 7
    lhs = p2((u[0, :n - k] * u[1, k:]).sum(-1)) * w[0, :n - k] * w[1, k:]
    rhs = 1.5 * ((a[0, :n - k] * a[1, k:]).sum(-1)) ** 2 - 0.5 * w[0, :n - k] * w[1, k:]
    assert np.max(np.abs(lhs - rhs)) <= 1e-14

    def normalised(rref):
        a, w = planes(rref)
        c = (1.5 * ((a[0, :n - k] * a[1, k:]).sum(-1)) ** 2 - 0.5 * w[0, :n - k] * w[1, k:]).mean()
        return c / np.sqrt((w[0] ** 2).mean() * (w[1] ** 2).mean())

    c0 = normalised(r.min(axis=1))
    direct = (p2((u[0, :n - k] * u[1, k:]).sum(-1)) * r[0, :n - k] ** -3 * r[1, k:] ** -3).mean() / np.sqrt((r[0] ** -6).mean() * (r[1] ** -6).mean())
    assert abs(c0 - direct) <= 1e-14
    assert abs(normalised(np.array([0.11, 0.37])) - c0) <= 1e-14


def run_script(*args):
    return subprocess.run([sys.executable, SCRIPT] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize('given,missing', [(['--tau', '100'], b'--pairs'), (['--pairs', 'none.txt'], b'--tau')])
def test_dipolarCrossCt_without_pairs_or_tau_is_an_argparse_error(given, missing):
    p = run_script('-s', 'none.pdb', '-f', 'none.npy', '--dipolarCrossCt', *given)
    assert p.returncode == 2
    assert b'usage:' in p.stderr and missing in p.stderr and b'Traceback' not in p.stderr


def test_dipolarCrossCt_refuses_trajectory_input(tmp_path):
    p = run_script('-s', 'none.pdb', '-f', str(tmp_path / 'traj.xtc'), '--tau', 100, '--pairs', 'none.txt', '-o', str(tmp_path / 'o'),
                   '--dipolarCrossCt')
    assert p.returncode == 1, p.stderr.decode()[-2000:]
    assert b'--dipolarCrossCt works on vector-file input' in p.stderr
    assert os.listdir(str(tmp_path)) == []


def test_dipolarCrossCt_is_documented():
    p = run_script('--help')
    assert p.returncode == 0
    text = ' '.join(p.stdout.decode().split())
    assert '--dipolarCrossCt' in text and '4896' in text
