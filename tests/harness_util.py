"""The test-only C++ harnesses (tests/*_harness.cpp): compiled into tests/_build when missing or older than what they are made of."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', '_build')
CSRC = os.path.join(ROOT, 'sca_amd', 'csrc')


def load_harness(name, headers):
    """tests/<name>.cpp as a loaded library; headers: the files of sca_amd/csrc it includes (include/sca_hip.h and sca_constants.h are always among them)"""
    out = os.path.join(BUILD, 'lib%s.so' % name)
    src = os.path.join(ROOT, 'tests', name + '.cpp')
    deps = [src, os.path.join(ROOT, 'include', 'sca_hip.h')] + [os.path.join(CSRC, f) for f in tuple(headers) + ('sca_constants.h',)]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        # (no ROCm include path: the headers must be plain C++)
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-fPIC', '-shared', '-I' + CSRC, '-o', out, src])
    return C.CDLL(out)
