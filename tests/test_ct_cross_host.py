"""
CPU tests of the host side of the pair cross-correlation functions (no GPU): the pair-file parser spinrelax_amd.ct.read_pairs, the
argument handling of scripts/calculate-Ct-from-traj.py --crossCt, and the new entry points in the header, the binding and the library.
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

SCRIPT = os.path.join(ROOT, 'scripts', 'calculate-Ct-from-traj.py')
NEW = {'sr_ct_cross_max_frames': 1, 'sr_ct_cross_f32_dev': 17, 'sr_vectors_ct_cross_f32': 13, 'sr_vectors_ct_cross_err_f32': 14}


def write(tmp_path, text):
    fn = str(tmp_path / 'pairs.txt')
    with open(fn, 'w') as fp:
        fp.write(text)
    return fn


def test_read_pairs_good_file(tmp_path):
    fn = write(tmp_path, '# methylene pairs\n0 1\n\n  3\t3   # the same vector twice\n6 2\n0 1\n')
    p = hostct.read_pairs(fn, 7)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1], [3, 3], [6, 2], [0, 1]]


@pytest.mark.parametrize('text,what', [('0 7\n', 'outside'), ('-1 2\n', 'outside'), ('0 1\n2\n', 'line 2'), ('0 1 2\n', 'two integers'),
                                       ('0 1.5\n', 'two integers'), ('a b\n', 'two integers'), ('# nothing\n\n', 'no pairs')])
def test_read_pairs_bad_files(tmp_path, text, what):
    with pytest.raises(ValueError) as exc:
        hostct.read_pairs(write(tmp_path, text), 7)
    assert what in str(exc.value)


def test_pairs_are_checked_before_any_device_call():
    """the Python entry points refuse a bad pair table themselves: no context is created (there is no GPU here to create one on)"""
    v4 = np.zeros((2, 8, 3, 3), dtype=np.float32)
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1, 2)], [], [(0.5, 1.0)]):
        with pytest.raises(ValueError):
            hostct.calculate_Ct_cross(v4, bad)
        with pytest.raises(ValueError):
            hostct.calculate_Ct_cross_from_files([v4[0], v4[1]], 1.0, 8.0, bad)
    with pytest.raises(ValueError):
        hostct.calculate_Ct_cross(v4[0], [(0, 1)])                       # not 4-dimensional


def test_crossCt_without_pairs_is_an_argparse_error():
    p = subprocess.run([sys.executable, SCRIPT, '-s', 'none.pdb', '-f', 'none.npy', '--tau', '100', '--crossCt'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2
    assert b'usage:' in p.stderr and b'--pairs' in p.stderr and b'Traceback' not in p.stderr


def test_crossCt_flags_are_documented():
    p = subprocess.run([sys.executable, SCRIPT, '--help'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0
    text = ' '.join(p.stdout.decode().split())
    for flag in ('--crossCt', '--pairs', '--asym'):
        assert flag in text
    assert '--vecRot has no effect' in text


def test_abi_declares_the_new_entry_points():
    with open(os.path.join(ROOT, 'include', 'spinrelax_hip.h')) as fp:
        text = re.sub(r'/\*.*?\*/', '', fp.read(), flags=re.S)
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r'\b(int|int64_t) %s\((.*?)\);' % name, text, flags=re.S)
        assert m and len(m.group(2).split(',')) == nargs, name
    assert _lib.SIGNATURES['sr_ct_cross_max_frames'][0] is ctypes.c_int64


def test_library_exports_the_new_entry_points():
    if not os.path.isfile(_lib.LIB_PATH):
        from spinrelax_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.sr_ct_cross_max_frames(None) == -1                         # no context: refused on the host, nothing touched
