"""sca_step_host without a GPU: the three exports, the block's layout (ONE function in sca_core.h, reached here through the library and through
the host-compiled harness), and the row arithmetic of k_host_ingest / k_host_egress (sca_amd/csrc/sca_hostio.hip.h) compiled for the host --
tests/hostio_harness.cpp runs the lanes of every workgroup one after the other.  The harness is not part of the product."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', '_build')
NEW = ('sca_host_state_layout', 'sca_host_state_get', 'sca_step_host')
ERR_ARG = -1
ROW_BYTES = (24, 12, 24, 1, 8, 4, 24, 1, 28)                  # pos, vel, heading, flags, total_dist, step_num, vpref, vpref_mode, action
SIZES = (1, 2, 63, 64, 65, 1000, 4096, 100000)


@pytest.fixture(scope='module')
def harness():
    out = os.path.join(BUILD, 'libhostio_harness.so')
    src = os.path.join(ROOT, 'tests', 'hostio_harness.cpp')
    deps = [src, os.path.join(ROOT, 'include', 'sca_hip.h')] + [os.path.join(ROOT, 'sca_amd', 'csrc', h) for h in
                                                               ('sca_hostio.hip.h', 'sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h')]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-ffp-contract=off', '-mfma', '-fno-builtin-pow',
                               '-I' + os.path.join(ROOT, 'sca_amd', 'csrc'), '-o', out, src])
    H = C.CDLL(out)
    p = C.c_void_p
    H.hio_layout.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    H.hio_ingest.restype = None
    H.hio_ingest.argtypes = [p, p, p, p, p, p, p, C.c_int, C.c_uint32]
    H.hio_egress.restype = None
    H.hio_egress.argtypes = [p, p, p, p, p, p, C.c_int]
    return H


def test_the_three_symbols_are_exported_declared_and_bound():
    from sca_amd import _lib
    L = _lib.lib()
    txt = open(os.path.join(ROOT, 'include', 'sca_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(sca_[a-z0-9_]+)\s*\(', txt))
    for s in NEW:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(L, s), s
    assert L.sca_version() == 103                               # callers detect the feature by the symbol
    hdr = {k: int(v) for k, v in re.findall(r'#define\s+(SCA_HOST_IN_[A-Z]+)\s+(\d+)\b', txt)}
    assert hdr == {'SCA_HOST_IN_STATE': _lib.HOST_IN_STATE, 'SCA_HOST_IN_VPREF': _lib.HOST_IN_VPREF} and hdr['SCA_HOST_IN_STATE'] == 1 and hdr['SCA_HOST_IN_VPREF'] == 2


def test_the_ctypes_mirror_has_the_size_and_the_offsets_of_the_headers_struct(harness):
    """sizeof(sca_host_state) as a C compiler and as a C++ compiler see the header against the ctypes mirror, member by member."""
    from sca_amd import _lib
    names = [f[0] for f in _lib.HostState._fields_]
    assert names == ['struct_bytes', 'n', 'pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'vpref', 'vpref_mode', 'action']
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(BUILD, 'host_state_size.c')
    with open(src, 'w') as f:
        f.write('#include <stddef.h>\n#include "sca_hip.h"\n'
                'int hs_size(void) { return (int)sizeof(sca_host_state); }\n'
                'int hs_offset(int k) { const size_t o[] = {' + ', '.join(f'offsetof(sca_host_state, {m})' for m in names) + '}; return (int)o[k]; }\n')
    out = os.path.join(BUILD, 'libhost_state_size.so')
    subprocess.check_call(['gcc', '-std=c99', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'include'), '-o', out, src])
    Z = C.CDLL(out)
    assert Z.hs_size() == C.sizeof(_lib.HostState) == harness.hio_sizeof_host_state() == 80
    for k, m in enumerate(names):
        assert Z.hs_offset(k) == getattr(_lib.HostState, m).offset, m


def _layout(fn, n):
    off = (C.c_int64 * 9)()
    total = C.c_int64(0)
    rc = fn(n, off, C.byref(total))
    return rc, [int(x) for x in off], int(total.value)


@pytest.mark.parametrize('n', SIZES)
def test_layout(harness, n):
    from sca_amd import _lib
    rc, off, total = _layout(_lib.lib().sca_host_state_layout, n)
    assert rc == 0
    assert (harness.hio_layout(n, (C.c_int64 * 9)(), C.byref(C.c_int64(0)))) == 9
    assert _layout(harness.hio_layout, n)[1:] == (off, total)   # the harness and the library call the same function
    assert off[0] == 0
    ends = off[1:] + [total]
    for s in range(9):
        assert off[s] % 64 == 0, (n, s)                          # every section on a 64-byte boundary
        size = ROW_BYTES[s] * n
        assert off[s] + size <= ends[s], (n, s)                  # disjoint, increasing, in the struct's order
        if s < 8:
            assert ends[s] - (off[s] + size) < 64, (n, s)        # the up-going sections contiguous up to padding
    assert total % 64 == 0 and total >= n * (73 + 25 + 28)


@pytest.mark.parametrize('n', [0, -1, -100000])
def test_layout_refuses_a_non_positive_n(n):
    from sca_amd import _lib
    assert _layout(_lib.lib().sca_host_state_layout, n)[0] == ERR_ARG
    assert _lib.lib().sca_host_state_layout(5, None, None) == ERR_ARG


def test_null_context_is_an_argument_error_without_a_gpu():
    from sca_amd import _lib
    L = _lib.lib()
    h = _lib.HostState()
    v = C.c_int(0)
    assert L.sca_host_state_get(None, C.byref(h), C.sizeof(h)) == ERR_ARG
    assert L.sca_step_host(None, 0, 1, C.byref(v)) == ERR_ARG
    assert L.sca_step_host(None, 0, 0, None) == ERR_ARG


def _aligned(nbytes, fill=0):
    raw = np.full(nbytes + 64, fill, np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + nbytes]


REC = np.dtype([('px', '<f8'), ('py', '<f8'), ('pz', '<f8'), ('vx', '<f4'), ('vy', '<f4'), ('vz', '<f4'), ('flags', '<u4'), ('radius', '<f8')])


@pytest.mark.parametrize('n', [1, 3, 63, 65, 255, 257, 1000, 4099])
def test_ingest_then_egress_gives_the_block_back_and_the_records_between_are_right(harness, n):
    """random block -> ingest -> device-side arrays -> egress -> the same bytes in every state section; the PubRecs in between hold, field by
    field, what this test computes from the input (radius untouched, the upper 24 bits of flags zero: rec.flags = flags[i])."""
    assert REC.itemsize == harness.hio_sizeof_pubrec() == 48
    rng = np.random.default_rng(n)
    _, off, total = _layout(harness.hio_layout, n)
    blk = _aligned(total)
    blk[:] = rng.integers(0, 256, total, dtype=np.uint8)         # random BYTES: NaN payloads, denormals and all must survive

    def sec(b, s, dt, shape):
        return b[off[s]:off[s] + ROW_BYTES[s] * n].view(dt).reshape(shape)
    pos, vel, head = sec(blk, 0, np.float64, (n, 3)), sec(blk, 1, np.float32, (n, 3)), sec(blk, 2, np.float64, (n, 3))
    flags, td, sn = sec(blk, 3, np.uint8, (n,)), sec(blk, 4, np.float64, (n,)), sec(blk, 5, np.int32, (n,))
    vp, vm = sec(blk, 6, np.float64, (n, 3)), sec(blk, 7, np.uint8, (n,))

    rec_b = _aligned(48 * n)
    rec = rec_b.view(REC)
    rec_b[:] = rng.integers(0, 256, 48 * n, dtype=np.uint8)      # stale records: everything but radius is replaced
    radius = rec['radius'].copy()
    d_head, d_td, d_sn = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    d_vp, d_vm = np.full((n, 3), 7.0), np.full(n + 8, 0xEE, np.uint8)   # (guard bytes behind the n the device array has)

    def P(a):
        return a.ctypes.data
    harness.hio_ingest(P(rec_b), P(d_head), P(d_td), P(d_sn), P(d_vp), P(d_vm), P(blk), n, 1)   # SCA_HOST_IN_STATE
    for k, col in (('px', pos[:, 0]), ('py', pos[:, 1]), ('pz', pos[:, 2]), ('vx', vel[:, 0]), ('vy', vel[:, 1]), ('vz', vel[:, 2])):
        assert rec[k].tobytes() == np.ascontiguousarray(col).tobytes(), (n, k)
    assert np.array_equal(rec['flags'], flags.astype(np.uint32)), n
    assert rec['radius'].tobytes() == radius.tobytes(), n
    assert d_head.tobytes() == head.tobytes() and d_td.tobytes() == td.tobytes() and np.array_equal(d_sn, sn)
    assert (d_vp == 7.0).all() and (d_vm == 0xEE).all()          # v_pref not asked for: not touched
    harness.hio_ingest(P(rec_b), P(d_head), P(d_td), P(d_sn), P(d_vp), P(d_vm), P(blk), n, 2)   # SCA_HOST_IN_VPREF
    assert d_vp.tobytes() == vp.tobytes() and np.array_equal(d_vm[:n], vm) and (d_vm[n:] == 0xEE).all()

    act8 = rng.standard_normal((n, 8)).astype(np.float32)
    rec['flags'] |= rng.integers(0, 1 << 24, n).astype(np.uint32) << 8   # down: (uint8_t)rec.flags -- the upper bits do not come along
    out = _aligned(total, 0x5A)
    harness.hio_egress(P(rec_b), P(d_head), P(d_td), P(d_sn), P(act8), P(out), n)
    for s in range(6):
        a, b = off[s], off[s] + ROW_BYTES[s] * n
        assert out[a:b].tobytes() == blk[a:b].tobytes(), (n, s)
    assert (out[off[6]:off[8]] == 0x5A).all(), n                 # the caller's v_pref sections are never written
    assert np.array_equal(sec(out, 8, np.float32, (n, 7)), act8[:, :7]), n
    # nothing outside a section but its own padding was written, and nothing beyond the block
    for s in (0, 1, 2, 4, 5, 8):
        end = (off[s + 1] if s < 8 else total)
        assert (out[off[s] + ROW_BYTES[s] * n:end] == 0x5A).all(), (n, s)
