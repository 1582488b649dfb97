"""
The drop-in scripts at a long memory time (marker gpu): calculate-Ct-from-traj.py with --tau / dt giving F = 25000 frames per
chunk (the blocked C(t) kernels), then calculate-fitted-Ct.py on the file it wrote.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from spinrelax_amd import synth
from spinrelax_amd import general_scripts as gs
from spinrelax_amd import fitting_Ct_functions as fitCt

pytestmark = pytest.mark.gpu
SCR = os.path.join(ROOT, 'scripts')


def run(script, *args):
    cmd = [sys.executable, os.path.join(SCR, script)] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode()
    return p.stdout.decode()


def test_long_tau_through_the_scripts(tmp_path):
    """C(t) of the written _Ctint.dat against the plain-C float64 oracle at 1e-6 relative (the north-star bar, through the 8
    printed digits).  The fit of that file must run, and its _fittedCt.dat must read back with finite parameters; no parity
    figure is claimed for the fit: no reference fixture exists at this chunk length."""
    F, R, V, dt = 25000, 2, 3, 2.0
    vecs = synth.synth_vectors(R * F + 11, V, seed=61)
    vecfn = str(tmp_path / 'vecs.npz')
    np.savez(vecfn, vecs=vecs, names=np.arange(2, 2 + V), dt=dt)
    out = str(tmp_path / 'long')
    run('calculate-Ct-from-traj.py', '-s', 'reference.pdb', '-f', vecfn, '--tau', F * dt, '-o', out, '--Ct')
    leg, t, C, dC = gs.load_sxydylist(out + '_Ctint.dat', 'legend')
    C, t = np.array(C), np.array(t)
    assert C.shape == (V, F // 2) and np.allclose(t[0], (np.arange(F // 2) + 1.0) * dt)

    so = os.path.join(ROOT, 'oracle', 'libsr_oracle.so')
    if not os.path.isfile(so):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle'), 'libsr_oracle.so'])
    lib = ctypes.CDLL(so)
    lib.sr_oracle_ct_palmer_f64.restype = ctypes.c_int
    v4 = np.ascontiguousarray(vecs[:R * F].reshape(R, F, V, 3), dtype=np.float32)
    Cr, dCr = np.empty((F // 2, V)), np.empty((F // 2, V))
    assert lib.sr_oracle_ct_palmer_f64(v4.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(R), ctypes.c_int64(F), ctypes.c_int64(V),
                                       Cr.ctypes.data_as(ctypes.c_void_p), dCr.ctypes.data_as(ctypes.c_void_p), None) == 0
    e = np.max(np.abs(C.T - Cr) / np.abs(Cr))
    print('\n[long tau] F=%d: C(t) of the written file against the oracle, relative %.2e' % (F, e))
    assert e < 1e-6, e

    run('calculate-fitted-Ct.py', '-f', out + '_Ctint.dat', '-o', out)
    fit = fitCt.read_fittedCt_parameters(out + '_fittedCt.dat')
    assert len(fit.model) == V
    for m in fit.model.values():
        assert np.isfinite(m.S2) and np.all(np.isfinite(m.C)) and np.all(np.isfinite(m.tau))
