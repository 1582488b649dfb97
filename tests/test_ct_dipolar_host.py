"""
CPU tests of the host side of the distance-weighted dipolar correlation function: what scripts/calculate-Ct-from-traj.py --dipolarCt
and spinrelax_amd.ct.calculate_Ct_dipolar refuse before the GPU is touched.  The kernels: tests/test_gpu_ct_dipolar.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import ct as hostct
from spinrelax_amd import hip


def run_script(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')] + [str(a) for a in args],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_dipolarCt_needs_tau(tmp_path):
    fn = str(tmp_path / 'v.npy')
    np.save(fn, np.ones((10, 2, 3), dtype=np.float32))
    p = run_script('-s', 'none.pdb', '-f', fn, '-o', str(tmp_path / 'o'), '--dipolarCt')
    out = p.stdout.decode()
    assert p.returncode == 1, out[-2000:]
    assert 'Refusing to do dipolar correlation analysis without using a block averaging over memory_time tau' in out
    assert os.listdir(str(tmp_path)) == ['v.npy']


def test_dipolarCt_refuses_trajectory_input(tmp_path):
    p = run_script('-s', 'none.pdb', '-f', str(tmp_path / 'traj.xtc'), '--tau', 100, '-o', str(tmp_path / 'o'), '--dipolarCt')
    out = p.stdout.decode()
    assert p.returncode == 1, out[-2000:]
    assert '--dipolarCt works on vector-file input' in out


def test_calculate_Ct_dipolar_checks_dist_before_any_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError('a context was asked for before the arguments were checked')
    monkeypatch.setattr(hip, 'default_context', no_context)
    vecs = np.ones((2, 10, 3, 3), dtype=np.float32)
    good = np.ones((2, 10, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='shape'):
        hostct.calculate_Ct_dipolar(vecs, dist=good[:, :9])
    with pytest.raises(ValueError, match='shape'):
        hostct.calculate_Ct_dipolar(vecs, dist=np.ones((2, 10, 3, 1), dtype=np.float32))
    for bad in (0.0, -0.3, np.nan, np.inf):
        d = good.copy()
        d[1, 4, 2] = bad
        with pytest.raises(ValueError, match='positive and finite'):
            hostct.calculate_Ct_dipolar(vecs, dist=d)
    with pytest.raises(ValueError, match='replicates, frames, vectors, 3'):
        hostct.calculate_Ct_dipolar(vecs[0])
    # a good dist gets as far as the context
    with pytest.raises(AssertionError, match='a context was asked for'):
        hostct.calculate_Ct_dipolar(vecs, dist=good)
