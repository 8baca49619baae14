"""The host side's form decisions (sca_amd/csrc/sca_forms.h) without a GPU: which kernels a pass runs at which shard size, SIMD count and
read-back count.  tests/forms_harness.cpp puts the plan functions behind a C interface.  Every expectation below is a literal worked out by
hand from the documented thresholds (1024 SIMDs unless a row says otherwise) -- none comes from the code under test."""
import ctypes as C
import itertools
import os
import re

import pytest

from harness_util import CSRC, ROOT, load_harness

INT_MAX = 2 ** 31 - 1
SPLIT, TRACK_FUSED, LANE, FEW, LP_LANE, SOLVE_FB, ACTION_FB = 1, 2, 4, 8, 16, 32, 64          # include/sca_hip.h
G64, G32, G16, G4, RP_LANE, TRACK_GROUP, TRACK_REPLAN = range(7)                               # ReplanKernel

DEFAULTS_1024 = {'SCA_K1_PACKED': -1, 'SCA_AUTO_BACKOFF_DIV': 8, 'SCA_AUTO_NO_TAIL': 0, 'SCA_AUTO_TAIL_MAX': 0, 'SCA_SOLVE_SPLIT': -1,
                 'SCA_HOST_STEP_STAGED': 0, 'SCA_KD_TOP': 1, 'SCA_EXT_STOP': 1, 'SCA_KD_TICKET': 0, 'SCA_KD_WAVE_CAP': 0,
                 'SCA_SOLVE_FB_MAX': 2048, 'SCA_ACTION_FB_MAX': 16384, 'SCA_LP_FORM': -1, 'SCA_TRACKER_FUSE': 0, 'SCA_TRACKER_NOGROUPFUSE': 1,
                 'SCA_TRK_SPEC4_MAX': 1024, 'SCA_TRK_SPEC3_MAX': 4096, 'SCA_TRK_SPEC2_MAX': 8192, 'SCA_TRK_MID_MAX': 32768}
REMOVED = ('SCA_TRACKER_SERIAL', 'SCA_TRACKER_NOQUAD', 'SCA_KD_NOHINT', 'SCA_KD_TAIL_LEVEL', 'SCA_AUTO_EVENT_WAIT', 'SCA_TRACKER_NOFUSE')


@pytest.fixture(scope='module')
def H():
    h = load_harness('forms_harness', ('sca_forms.h',))
    h.forms_tunable_name.restype = C.c_char_p
    h.forms_plan_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return h


@pytest.fixture()
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith('SCA_'):
            monkeypatch.delenv(k)
    return monkeypatch


def names(H):
    return [H.forms_tunable_name(i).decode() for i in range(H.forms_tunable_count())]


def from_env(H, simds=1024):
    out = (C.c_int * H.forms_tunable_count())()
    H.forms_tunables_from_env(simds, out)
    return dict(zip(names(H), out))


def tun(H, **over):
    """the defaults at 1024 SIMDs as the harness wants them, with overrides by environment name"""
    d = dict(DEFAULTS_1024, **{'SCA_' + k: v for k, v in over.items()})
    return (C.c_int * len(d))(*[d[k] for k in names(H)])


def solve(H, cnt, simds=1024, part_on=0, nranks=1, lp_total=0, lp=0, overlap=0, last=-1, no_scratch=0, t=None, **over):
    out = (C.c_int * 7)()
    H.forms_plan_solve(t or tun(H, **over), simds, cnt, part_on, nranks, lp_total, lp, overlap, last, no_scratch, out)
    return dict(zip(('packed', 'split', 'solve_fb', 'lpw', 'lp_kernel', 'action_fb', 'forms'), out))


def replans(H, cnt, last, many=0, in_pass=1, part_on=0, **over):
    out = (C.c_int * 29)()
    H.forms_plan_replans(tun(H, **over), cnt, last, many, in_pass, part_on, out)
    return {'fused': out[0], 'group_fused': out[1], 'forms': out[2], 'launches': [tuple(out[4 + 5 * i:9 + 5 * i]) for i in range(out[3])]}


def kd(H, n, beside=0, hint=0, chunk_cap=1 << 30, rank_cap=1 << 30, t=None, **over):
    out = (C.c_int * 9)()
    H.forms_plan_kd_build(t or tun(H, **over), n, beside, hint, chunk_cap, rank_cap, out)
    return dict(zip(('top', 'wave_max', 'block', 'level_passes', 'first_single', 'grid', 'ticket', 'levels', 'sgrid'), out))


def auto(H, fits=1, tracked=0, ahead=0, kdq_last=-1, div=8, backoff=0, shard=100000):
    out = (C.c_int * 4)()
    H.forms_plan_auto(fits, tracked, ahead, kdq_last, div, backoff, shard, out)
    return tuple(out)                                                                          # (AUTO pass, auto_backoff, kdq_last, kdq blocks)


# ---- the tunables ------------------------------------------------------------------------------------------------------------------------------

def test_the_table_lists_exactly_the_documented_switches_with_their_defaults(H, clean_env):
    assert from_env(H) == DEFAULTS_1024
    half = from_env(H, 512)                                                                    # "so many wavefronts per SIMD"
    assert {k: v for k, v in half.items() if v != DEFAULTS_1024[k]} == {
        'SCA_SOLVE_FB_MAX': 1024, 'SCA_ACTION_FB_MAX': 8192, 'SCA_TRK_SPEC4_MAX': 512, 'SCA_TRK_SPEC3_MAX': 2048, 'SCA_TRK_SPEC2_MAX': 4096,
        'SCA_TRK_MID_MAX': 16384}
    k = (C.c_int * 7)()
    H.forms_constants(k)
    assert tuple(k) == (1536, 128, 2048, 40, 4096, 1024, 64)


def test_every_switch_parses_as_documented(H, clean_env):
    def one(name, value, simds=1024):
        clean_env.setenv(name, value)
        got = from_env(H, simds)
        clean_env.delenv(name)
        assert {k for k, v in got.items() if v != DEFAULTS_1024[k]} <= {name}                  # no switch moves another
        return got[name]
    for name in ('SCA_K1_PACKED', 'SCA_SOLVE_SPLIT', 'SCA_HOST_STEP_STAGED', 'SCA_KD_TOP', 'SCA_EXT_STOP', 'SCA_KD_TICKET'):
        assert (one(name, '0'), one(name, '1'), one(name, '7')) == (0, 1, 1), name
    assert (one('SCA_AUTO_NO_TAIL', '1'), one('SCA_AUTO_NO_TAIL', '0'), one('SCA_AUTO_NO_TAIL', '')) == (1, 1, 1)      # being set is the switch
    assert (one('SCA_TRACKER_FUSE', '1'), one('SCA_TRACKER_FUSE', '0')) == (1, 1)
    assert (one('SCA_TRACKER_NOGROUPFUSE', '1'), one('SCA_TRACKER_NOGROUPFUSE', '0')) == (0, 0)
    assert [one('SCA_AUTO_BACKOFF_DIV', v) for v in ('0', '1', '4', '64', '65')] == [1, 1, 4, 64, 64]
    assert [one('SCA_AUTO_TAIL_MAX', v) for v in ('-3', '0', '32')] == [0, 0, 32]
    assert [one('SCA_KD_WAVE_CAP', v) for v in ('100', '256', '512', '1536', '5000')] == [256, 256, 512, 1536, 1536]
    assert [one('SCA_LP_FORM', v) for v in ('lane', 'wave', 'l', 'w', 'other')] == [1, 0, 1, 0, -1]
    for name in ('SCA_SOLVE_FB_MAX', 'SCA_ACTION_FB_MAX', 'SCA_TRK_SPEC4_MAX', 'SCA_TRK_SPEC3_MAX', 'SCA_TRK_SPEC2_MAX', 'SCA_TRK_MID_MAX'):
        assert [one(name, v) for v in ('0', '1000000', '-1')] == [0, 1000000, -1], name        # as given: not clamped


def test_a_switch_keeps_the_moment_at_which_it_is_read(H, clean_env):
    """the tracker's rows are read again by every sca_device_tracker_enable, the solver's only by sca_create"""
    t = tun(H)
    clean_env.setenv('SCA_TRACKER_FUSE', '1')
    clean_env.setenv('SCA_TRK_MID_MAX', '0')
    clean_env.setenv('SCA_SOLVE_SPLIT', '1')
    clean_env.setenv('SCA_LP_FORM', 'lane')
    H.forms_tunables_tracker_again(1024, t)
    got = dict(zip(names(H), t))
    assert {k: v for k, v in got.items() if v != DEFAULTS_1024[k]} == {'SCA_TRACKER_FUSE': 1, 'SCA_TRK_MID_MAX': 0}
    clean_env.delenv('SCA_TRACKER_FUSE')
    H.forms_tunables_tracker_again(1024, t)
    assert dict(zip(names(H), t))['SCA_TRACKER_FUSE'] == 0


def test_the_host_reads_the_environment_in_one_place_and_the_documents_name_the_switches_that_exist(H):
    src = open(os.path.join(CSRC, 'sca_hip.hip')).read()
    assert re.findall(r'getenv\("(\w+)"\)', src) == ['SCA_QUIET'] and src.count('getenv') == 1
    assert src.count('tunables_from_env(') == 2                                                # sca_create, sca_device_tracker_enable
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in names(H):
        assert name in doc, name
    product = doc + src + open(os.path.join(CSRC, 'sca_forms.h')).read()
    for name in REMOVED:
        assert name not in product, name


# ---- the solve and its neighbours ---------------------------------------------------------------------------------------------------------------

def test_packed_k1_from_six_wavefronts_of_four_agents_per_simd(H):
    assert [solve(H, n)['packed'] for n in (6143, 6144)] == [0, 1]
    assert [solve(H, n, simds=512)['packed'] for n in (3071, 3072)] == [0, 1]
    assert [solve(H, n, K1_PACKED=f)['packed'] for n, f in ((100000, 0), (10, 1))] == [0, 1]


def test_solve_fb_and_action_fb(H):
    assert [solve(H, n)['solve_fb'] for n in (1, 2048, 2049)] == [1, 1, 0]
    assert [solve(H, n, simds=512, t=tun(H, SOLVE_FB_MAX=1024, ACTION_FB_MAX=8192))['solve_fb'] for n in (1024, 1025)] == [1, 0]
    assert solve(H, 2048, lp=1, lp_total=1)['solve_fb'] == 0                                   # somebody else feeds the fallback list
    assert solve(H, 2048, SOLVE_SPLIT=1)['solve_fb'] == 0
    assert solve(H, 2048, SOLVE_SPLIT=1, no_scratch=1) == dict(packed=0, split=0, solve_fb=0, lpw=0, lp_kernel=0, action_fb=1, forms=ACTION_FB)
    assert solve(H, 2048, part_on=1, nranks=2)['solve_fb'] == 0
    assert [(solve(H, n)['action_fb'], solve(H, n)['forms']) for n in (2048, 2049, 16384, 16385)] == [(0, SOLVE_FB), (1, ACTION_FB), (1, ACTION_FB), (0, 0)]
    assert solve(H, 2048, SOLVE_FB_MAX=0)['forms'] == ACTION_FB and solve(H, 2048, SOLVE_FB_MAX=0, ACTION_FB_MAX=0)['forms'] == 0


def test_lp_form(H):
    assert [solve(H, 100000, lp=k, lp_total=k)['lp_kernel'] for k in (0, 16383, 16384)] == [0, 0, 1]
    assert [solve(H, 100000, simds=512, lp=k, lp_total=k)['lp_kernel'] for k in (8191, 8192)] == [0, 1]
    assert solve(H, 100000, lp=16383, lp_total=16383) == dict(packed=1, split=0, solve_fb=0, lpw=1, lp_kernel=0, action_fb=0, forms=0)
    assert solve(H, 100000, lp=16384, lp_total=16384) == dict(packed=1, split=0, solve_fb=0, lpw=0, lp_kernel=1, action_fb=0, forms=LP_LANE)
    # the partition: the LP agents of the whole swarm per rank; the range the kernels walk (lp) is the owned agents
    assert [solve(H, 50000, part_on=1, nranks=2, lp_total=k, lp=50000)['lp_kernel'] for k in (32767, 32768)] == [0, 1]
    assert solve(H, 50000, part_on=1, nranks=2, lp_total=32768, lp=50000, LP_FORM=0)['lp_kernel'] == 1      # SCA_LP_FORM is a switch of the shard rule
    # a split pass: k_solve_pick4 carries no LP
    assert solve(H, 30000, lp=5, lp_total=5, SOLVE_SPLIT=1) == dict(packed=1, split=1, solve_fb=0, lpw=0, lp_kernel=1, action_fb=0, forms=SPLIT | LP_LANE)
    assert solve(H, 30000, lp=0, SOLVE_SPLIT=1)['lp_kernel'] == 0
    assert [solve(H, 30000, lp=k, lp_total=k, LP_FORM=1)['lp_kernel'] for k in (0, 5)] == [0, 1]
    assert solve(H, 30000, lp=20000, lp_total=20000, LP_FORM=0) == dict(packed=1, split=0, solve_fb=0, lpw=1, lp_kernel=0, action_fb=0, forms=0)


def test_choose_solve_split(H):
    def split(cnt, last, overlap=1, simds=1024, **over):
        return H.forms_choose_solve_split(tun(H, **over), simds, overlap, cnt, last)
    assert [split(50000, 40000, SOLVE_SPLIT=v, overlap=o) for v in (0, 1) for o in (0, 1)] == [0, 0, 1, 1]
    assert split(50000, 40000, overlap=0) == 0
    assert [split(50000, e) for e in (32768, 32769)] == [0, 1]                                 # the many-lanes-per-plan forms: nothing to hide behind
    assert [split(n, 32769) for n in (61440, 61441)] == [1, 0] and [split(n, 65536) for n in (61440, 61441)] == [1, 0]      # one round
    assert [split(n, 65537) for n in (61441, 114688, 114689)] == [1, 1, 0] and split(114688, 131072) == 1                   # two
    assert [split(n, 131073) for n in (50000, 114688, 200000)] == [0, 0, 0]                                                 # three
    assert [split(n, -1) for n in (32768, 32769, 61440, 61441, 65536, 65537, 114688, 114689, 131073)] == [0, 1, 1, 0, 0, 1, 1, 0, 0]
    half = dict(TRK_MID_MAX=16384)
    assert [split(n, e, simds=512, **half) for n, e in ((30000, 16384), (30720, 16385), (30721, 16385), (57344, 32769), (57345, 32769))] == [0, 1, 0, 1, 0]
    assert solve(H, 50000, overlap=1, last=40000)['forms'] == SPLIT and solve(H, 50000, overlap=0, last=40000)['forms'] == 0


# ---- the tracker's re-plans -----------------------------------------------------------------------------------------------------------------------

def test_replans_count_unknown_launches_every_possible_form_with_its_natural_range(H):
    assert replans(H, 100000, -1) == dict(fused=0, group_fused=0, forms=FEW | LANE, launches=[
        (G64, -1, 1024, 1024, 64), (G32, 1024, 4096, 4096, 32), (G16, 4096, 8192, 8192, 16), (G4, 8192, 32768, 32768, 4), (RP_LANE, 32768, INT_MAX, 100000, 1)])
    assert replans(H, 5000, -1) == dict(fused=0, group_fused=0, forms=FEW, launches=[
        (G64, -1, 1024, 1024, 64), (G32, 1024, 4096, 4096, 32), (G16, 4096, INT_MAX, 5000, 16)])
    assert replans(H, 5000, -1, in_pass=0)['launches'] == replans(H, 5000, -1)['launches']


def test_replans_known_count_hysteresis_of_a_quarter_on_both_sides(H):
    r = lambda last, cnt=100000, **kw: replans(H, cnt, last, **kw)
    assert r(5000) == dict(fused=0, group_fused=0, forms=FEW, launches=[(G32, -1, 4096, 4096, 32), (G16, 4096, INT_MAX, 100000, 16)])
    assert [[l[0] for l in r(v)['launches']] for v in (5120, 5121)] == [[G32, G16], [G16]]                  # 4096 + 1024
    assert [[l[0] for l in r(v)['launches']] for v in (3072, 3073)] == [[G32], [G32, G16]]                  # 4096 - 1024
    assert r(3072)['launches'] == [(G32, -1, INT_MAX, 100000, 32)]
    assert [[l[0] for l in r(v)['launches']] for v in (0, 768, 769, 1280, 1281)] == [[G64], [G64], [G64, G32], [G64, G32], [G32]]
    assert [[l[0] for l in r(v)['launches']] for v in (24576, 24577, 40960, 40961)] == [[G4], [G4, RP_LANE], [G4, RP_LANE], [RP_LANE]]
    assert r(24577) == dict(fused=0, group_fused=0, forms=FEW | LANE, launches=[(G4, -1, 32768, 32768, 4), (RP_LANE, 32768, INT_MAX, 100000, 1)])
    assert r(90000) == dict(fused=0, group_fused=0, forms=LANE, launches=[(RP_LANE, -1, INT_MAX, 100000, 1)])
    assert r(90000, cnt=20000)['launches'] == [(RP_LANE, -1, INT_MAX, 20000, 1)]               # no form is possible AND wanted: the lane form takes all


def test_replans_fused_forms(H):
    lane_alone = [(TRACK_REPLAN, -1, INT_MAX, 100000, 1)]
    assert replans(H, 100000, 75000, TRACKER_FUSE=1) == dict(fused=1, group_fused=0, forms=TRACK_FUSED | LANE, launches=lane_alone)
    assert replans(H, 100000, 74999, TRACKER_FUSE=1)['fused'] == 0                              # 3/4 of the shard
    assert replans(H, 100000, 40000, TRACKER_FUSE=1)['fused'] == 0                              # not in lane form ALONE (k_replan_group<4> is launched too)
    assert replans(H, 100000, 75000)['fused'] == 0                                              # opt-in
    assert replans(H, 100000, 75000, TRACKER_FUSE=1, in_pass=0)['fused'] == 0
    assert replans(H, 100000, 75000, TRACKER_FUSE=1, part_on=1)['fused'] == 0
    assert replans(H, 100000, -1, TRACKER_FUSE=1)['fused'] == 0
    for last in (-1, 0, 1024):
        assert replans(H, 1024, last) == dict(fused=0, group_fused=1, forms=TRACK_FUSED | FEW, launches=[(TRACK_GROUP, -1, INT_MAX, 1024, 64)])
    assert replans(H, 1025, -1)['group_fused'] == 0
    assert replans(H, 1024, -1, TRACKER_NOGROUPFUSE=0)['group_fused'] == 0
    assert replans(H, 1024, -1, in_pass=0)['group_fused'] == 0 and replans(H, 1024, -1, part_on=1)['group_fused'] == 0
    assert replans(H, 2048, -1, TRK_SPEC4_MAX=2048)['group_fused'] == 1
    # the per-agent form: a wavefront per plan at any count
    assert replans(H, 100000, 90000, many=1, TRACKER_FUSE=1) == dict(fused=0, group_fused=0, forms=FEW, launches=[(G64, -1, INT_MAX, 100000, 64)])
    assert replans(H, 100000, -1, many=1)['launches'] == [(G64, -1, INT_MAX, 100000, 64)]
    assert replans(H, 500, 3, many=1)['launches'] == [(TRACK_GROUP, -1, INT_MAX, 500, 64)]


def test_replans_every_count_is_exactly_one_launchs(H):
    """over a grid of shard sizes, read-back counts and bounds (the tests' forcing values and non-monotone ones among them): the launched
    ranges start at -1, end at INT_MAX, and every count 1 .. cnt falls into exactly one of them, whose grid holds it"""
    bounds = [(1024, 4096, 8192, 32768), (0, 0, 0, 0), (1000000,) * 4, (0, 1000000, 1000000, 1000000), (0, 0, 1000000, 1000000),
              (0, 0, 0, 1000000), (4096, 1024, 8192, 2048), (512, 2048, 4096, 16384), (-5, 7, 7, 9), (1, 2, 3, 4), (32768, 8192, 4096, 1024)]
    cnts = (1, 2, 5, 100, 1024, 1025, 5000, 40000, 100000, 2000000)
    lasts = (-1, 0, 1, 3, 768, 769, 1280, 1281, 3072, 5121, 8192, 24577, 40961, 99999, 1999999)
    checked = 0
    for (s4, s3, s2, mid), cnt, last, many, fuse in itertools.product(bounds, cnts, lasts, (0, 1), (0, 1)):
        r = replans(H, cnt, last, many=many, TRK_SPEC4_MAX=s4, TRK_SPEC3_MAX=s3, TRK_SPEC2_MAX=s2, TRK_MID_MAX=mid, TRACKER_FUSE=fuse, TRACKER_NOGROUPFUSE=0)
        L = r['launches']
        ctx = (s4, s3, s2, mid, cnt, last, many, fuse, L)
        assert 1 <= len(L) <= 5 and L[-1][2] == INT_MAX, ctx
        assert L[0][1] <= 0, ctx                                   # (-1, or the bound of a range that could only hold the count 0: nothing to launch)
        for a, b in zip(L, L[1:]):
            assert a[2] == b[1] and a[1] < a[2], ctx               # contiguous: so exactly one range holds each count above the first lo
        for k, lo, hi, plans, lanes in L:
            assert plans >= min(cnt, hi) and lanes == (64, 32, 16, 4, 1, 64, 1)[k], ctx
        checked += 1
    assert checked == len(bounds) * len(cnts) * len(lasts) * 4


# ---- SCA_NBR_AUTO ------------------------------------------------------------------------------------------------------------------------------------

def test_plan_auto(H):
    assert auto(H, kdq_last=125, shard=1000) == (1, 0, 125, 64)                                 # 125 * 8 = 1000: not MORE than the shard
    assert auto(H, kdq_last=126, shard=1000) == (0, 255, -1, 1024)                              # back-off: this pass is the first of 256 kd passes
    assert auto(H, kdq_last=126, shard=1000, ahead=1) == (1, 0, 126, 64)                        # a tree was built ahead: an AUTO pass whatever the counts say
    assert auto(H, kdq_last=300, shard=1000, div=1) == (1, 0, 300, 1024) and auto(H, kdq_last=300, shard=1000, div=4) == (0, 255, -1, 1024)
    assert auto(H, backoff=5) == (0, 4, -1, 1024) and auto(H, backoff=1) == (0, 0, -1, 1024) and auto(H, backoff=0) == (1, 0, -1, 1024)
    assert auto(H, backoff=5, kdq_last=10**6) == (0, 4, 10**6, 1024)                            # (already backing off: the count is kept)
    assert auto(H, backoff=5, ahead=1) == (1, 5, -1, 1024)
    assert auto(H, fits=0) == (0, 0, -1, 1024) and auto(H, tracked=1) == (0, 0, -1, 1024)
    assert auto(H, fits=0, ahead=1)[0] == 1 and auto(H, tracked=1, ahead=1)[0] == 1
    assert [auto(H, kdq_last=k)[3] for k in (-1, 0, 1, 256, 257, 12500)] == [1024, 64, 64, 64, 1024, 1024]
    nxt = lambda fits=1, tracked=0, part=0, last=-1, div=8, backoff=0, shard=1000: H.forms_auto_next(fits, tracked, part, last, div, backoff, shard)
    assert [nxt(), nxt(fits=0), nxt(tracked=1), nxt(part=1), nxt(backoff=1), nxt(last=125), nxt(last=126)] == [1, 0, 0, 0, 0, 1, 0]
    tail = lambda ok=1, wv=1, seq=7, last=0, mx=0: H.forms_auto_tail_form(ok, wv, seq, last, mx)
    assert [tail(), tail(last=-1), tail(last=1), tail(ok=0), tail(wv=0), tail(seq=0)] == [1, 0, 0, 0, 0, 0]
    assert [tail(last=k, mx=8) for k in (-1, 0, 8, 9)] == [0, 1, 1, 0]


# ---- SCA_NBR_AUTO: the slot rule -------------------------------------------------------------------------------------------------------------------
# From the comments of sca_ctx::Auto: pass `seq` fills and reads the list of parity seq & 1; event slot [seq & 3] of ev_kdq is recorded behind
# its kd query (a launch on the kd stream) or, in the launch-free (tail) form, behind its build's last kernel; the pass two on reuses the list
# and waits for slot [(seq - 2) & 3] if that query was a launch on the kd stream (bit [seq & 3] of on_kd); the gather kernels of the last two
# builds alternate between the two slots of ev_gather, and the integrate stage waits for the build before the last.
NONE = -1
WAIT_NONE, WAIT_VALUE, WAIT_EVENT = 0, 1, 2
U32 = 1 << 32


def abuild(H, auto_seq, on_kd=0, builds=0, last=-1, tail_ok=1, wv=1, tail_max=0):
    out = (C.c_longlong * 5)()
    H.forms_plan_auto_build(tail_ok, wv, C.c_uint(auto_seq % U32), last, tail_max, C.c_uint(on_kd), C.c_uint(builds), out)
    return dict(zip(('seq', 'tail', 'record', 'wait', 'gather'), out))


def apass(H, auto_seq, tail_seq=0, on_kd=0, wv=1, pending=0, passes=0, builds=0):
    out = (C.c_longlong * 11)()
    H.forms_plan_auto_pass(C.c_uint(auto_seq % U32), C.c_uint(tail_seq % U32), C.c_uint(on_kd), wv, pending, C.c_uint(passes), C.c_uint(builds), out)
    return dict(zip(('seq', 'parity', 'reuse', 'tail', 'slot', 'on_kd_stream', 'on_kd', 'copy', 'passes', 'wait', 'gather'), out))


def test_auto_slots_first_five_passes_in_the_launch_form(H):
    """no list length has come back (last = -1): every build without a tail, every kd query a launch on the kd stream"""
    for k in (1, 2, 3, 4, 5):
        assert abuild(H, k - 1, on_kd=0b1111, builds=k - 1) == dict(seq=k, tail=0, record=NONE, wait=NONE, gather=(k - 1) & 1), k
    on_kd_before = {1: 0b0000, 2: 0b0010, 3: 0b0110, 4: 0b1110, 5: 0b1111}
    want = {1: dict(parity=1, reuse=NONE, slot=1, on_kd=0b0010, gather=1), 2: dict(parity=0, reuse=NONE, slot=2, on_kd=0b0110, gather=0),
            3: dict(parity=1, reuse=1, slot=3, on_kd=0b1110, gather=1), 4: dict(parity=0, reuse=2, slot=0, on_kd=0b1111, gather=0),
            5: dict(parity=1, reuse=3, slot=1, on_kd=0b1111, gather=1)}
    for k, w in want.items():
        got = apass(H, k - 1, on_kd=on_kd_before[k], builds=k, passes=k - 1, pending=1)
        assert got == dict(w, seq=k, tail=0, on_kd_stream=1, copy=0, passes=k - 1, wait=WAIT_VALUE), k


def test_auto_slots_first_five_passes_in_the_tail_form(H):
    """lengths of 0 have come back: every build records its pass's slot behind its last kernel, no pass launches a kd query or waits"""
    for k in (1, 2, 3, 4, 5):
        assert abuild(H, k - 1, builds=k - 1, last=0) == dict(seq=k, tail=1, record=k & 3, wait=NONE, gather=(k - 1) & 1), k
        assert apass(H, k - 1, tail_seq=k, builds=k, passes=1, pending=1) == dict(
            seq=k, parity=k & 1, reuse=NONE, tail=1, slot=k & 3, on_kd_stream=0, on_kd=0, copy=0, passes=1, wait=WAIT_NONE, gather=k & 1), k
    assert abuild(H, 4, last=0, tail_ok=0)['tail'] == 0 and abuild(H, 4, last=0, wv=0)['tail'] == 0 and abuild(H, 4, last=1)['tail'] == 0
    assert abuild(H, 4, last=1, tail_max=1)['tail'] == 1


def test_auto_slots_where_the_two_forms_meet(H):
    # pass 3 a launch (bit 3), pass 5 in the tail form: the wait for slot 3 is due, at the build; the pass itself does not wait again
    assert abuild(H, 4, on_kd=0b1000, builds=4, last=0) == dict(seq=5, tail=1, record=1, wait=3, gather=0)
    got = apass(H, 4, tail_seq=5, on_kd=0b1010, builds=5)
    assert (got['reuse'], got['tail'], got['on_kd_stream'], got['on_kd'], got['wait']) == (NONE, 1, 0, 0b1000, WAIT_NONE)
    # ... also when that build was enqueued ahead: nothing but tail_seq tells the pass
    assert apass(H, 4, tail_seq=0, on_kd=0b1000, builds=5)['reuse'] == 3 and apass(H, 4, tail_seq=5, on_kd=0b1000, builds=5)['reuse'] == NONE
    # pass 3 in the tail form (it ran inside the pass's own grid query), pass 5 a launch: no wait
    got = apass(H, 4, tail_seq=3, on_kd=0b0101, builds=5)
    assert (got['reuse'], got['tail'], got['slot'], got['on_kd_stream'], got['on_kd']) == (NONE, 0, 1, 1, 0b0111)
    assert abuild(H, 4, on_kd=0b0111, last=0)['wait'] == NONE
    # a tail form's stale tail_seq is no tail pass
    assert apass(H, 6, tail_seq=5)['tail'] == 0 and apass(H, 6, tail_seq=7)['tail'] == 1


def test_auto_count_copy_every_fourth_pass_and_never_while_one_is_pending(H):
    got = [(apass(H, 7, passes=k)['copy'], apass(H, 7, passes=k)['passes']) for k in range(10)]
    assert got == [(1, 1), (0, 2), (0, 3), (0, 4), (1, 5), (0, 6), (0, 7), (0, 8), (1, 9), (0, 10)]
    assert [(apass(H, 7, passes=k, pending=1)['copy'], apass(H, 7, passes=k, pending=1)['passes']) for k in (0, 4, 8)] == [(0, 0), (0, 4), (0, 8)]


def test_auto_wait_forms(H):
    assert apass(H, 7, tail_seq=8, wv=1)['wait'] == WAIT_NONE
    assert apass(H, 7, tail_seq=0, wv=1)['wait'] == WAIT_VALUE
    assert apass(H, 7, tail_seq=0, wv=0)['wait'] == WAIT_EVENT


def test_auto_slots_around_the_wrap_of_seq(H):
    """seq = 2^32 - 2 .. 2 with every earlier kd query a launch: what the guards give there today (a pass numbered 0 never takes the tail form
    and reads tail_seq = 0 as "this pass's build made the stream wait"; passes 1 and 2 skip the reuse wait like a context's first two)"""
    seqs = (U32 - 2, U32 - 1, 0, 1, 2)
    assert [(b['seq'], b['tail'], b['record'], b['wait']) for b in (abuild(H, s - 1, on_kd=0b1111, last=0) for s in seqs)] == [
        (U32 - 2, 1, 2, 0), (U32 - 1, 1, 3, 1), (0, 0, NONE, NONE), (1, 1, 1, NONE), (2, 1, 2, NONE)]
    got = [apass(H, s - 1, tail_seq=U32 - 4, on_kd=0b1111) for s in seqs]
    assert [(p['seq'], p['parity'], p['reuse'], p['tail'], p['slot']) for p in got] == [
        (U32 - 2, 0, 0, 0, 2), (U32 - 1, 1, 1, 0, 3), (0, 0, 2, 0, 0), (1, 1, NONE, 0, 1), (2, 0, NONE, 0, 2)]
    zero = apass(H, U32 - 1, tail_seq=0, on_kd=0b1111)
    assert (zero['seq'], zero['tail'], zero['reuse']) == (0, 0, NONE)


def test_auto_slot_model_no_list_refilled_and_no_record_buffer_written_under_a_reader(H):
    """A few hundred passes, each in the tail or the launch form, its build inside the pass or ahead of it (fixed seed), on a model of the two
    streams: the kd stream runs what it is given in order, so "the pass's stream has waited for an event" means everything the kd stream was
    given up to that event's record is through.  The wait-value form counts as no wait at all (it returns at once when nobody is listed).
    (i) a list is never reset and refilled before the kd query that last read it has been waited for, or ran on the pass's own stream;
    (ii) the integrate stage never writes the record buffer that an unwaited gather still reads."""
    import random
    rng = random.Random(20240607)
    kd_pos = 0                                   # operations the kd stream has been given
    synced = 0                                   # ... of which the pass's stream has waited for this many
    ev_kdq, ev_gather = [0] * 4, [0] * 2         # where each event was last recorded (0: never, fires at once)
    list_reader = [None, None]                   # per list parity: the kd stream position of the query that read it last, 'own': on the pass's stream
    buf_reader = [0, 0]                          # per record buffer: the kd stream position of the gather that read it last
    cur = 0                                      # the record buffer that holds the current positions
    st = dict(seq=0, tail_seq=0, on_kd=0, builds=0, passes=0, pending=0, wv=1)
    seen = dict(tail=0, launch=0, ahead=0, reuse=0, build_wait=0)

    def build(last):
        nonlocal kd_pos, synced
        b = abuild(H, st['seq'], on_kd=st['on_kd'], builds=st['builds'], last=last, wv=st['wv'])
        assert b['seq'] == st['seq'] + 1
        if b['wait'] != NONE:
            synced = max(synced, ev_kdq[b['wait']]); seen['build_wait'] += 1
        kd_pos += 1; ev_gather[b['gather']] = kd_pos; buf_reader[cur] = kd_pos; st['builds'] += 1       # the gather
        kd_pos += 1                                                                                  # ... the build's last kernel
        if b['tail']:
            ev_kdq[b['record']] = kd_pos; st['tail_seq'] = b['seq']

    ahead = False
    for n in range(1, 401):
        if not ahead:
            build(rng.choice((-1, 0)))
        p = apass(H, st['seq'], tail_seq=st['tail_seq'], on_kd=st['on_kd'], wv=st['wv'], pending=st['pending'], passes=st['passes'], builds=st['builds'])
        assert p['seq'] == n and p['on_kd_stream'] == (not p['tail'])
        if p['reuse'] != NONE:
            synced = max(synced, ev_kdq[p['reuse']]); seen['reuse'] += 1
        r = list_reader[p['parity']]             # (i): the grid build resets this list now
        assert r is None or r == 'own' or synced >= r, (n, p, r, synced)
        if p['tail']:
            list_reader[p['parity']] = 'own'; seen['tail'] += 1
        else:
            kd_pos += 1; ev_kdq[p['slot']] = kd_pos; list_reader[p['parity']] = kd_pos; seen['launch'] += 1
        if p['copy']:
            st['pending'] = 1
        elif st['pending'] and rng.random() < 0.4:
            st['pending'] = 0                    # the copy has arrived
        wait = p['wait']
        if wait == WAIT_VALUE and n >= 300:
            st['wv'], wait = 0, WAIT_EVENT       # hipStreamWaitValue32 refused: the event wait in its place, and from here on
        if wait == WAIT_EVENT:
            synced = max(synced, ev_kdq[p['slot']])
        if st['wv']:                             # (the event form has waited for this pass's build with its kd query)
            synced = max(synced, ev_gather[p['gather']])
        g = buf_reader[1 - cur]                  # (ii): the integrate stage writes the other buffer now
        assert synced >= g, (n, p, g, synced)
        cur = 1 - cur
        st.update(seq=p['seq'], on_kd=p['on_kd'], passes=p['passes'])
        ahead = rng.random() < 0.5
        if ahead:
            build(rng.choice((-1, 0))); seen['ahead'] += 1
    assert min(seen.values()) > 20, seen         # every branch of the model ran


# ---- a step of a burst: the events that ride ---------------------------------------------------------------------------------------------------------
# From sca_run_steps' loop and launch_collide_finish as they stood before plan_step / plan_finish existed (the conditions are quoted in the tests).
KD, GRID, HOSTBUILD, AUTO = 0, 1, 2, 3                                                          # include/sca_hip.h
STEP_IN = ('mode', 'step', 'steps', 'kd_stream', 'ext_stop', 'comm', 'whole', 'trk_on', 'trk_in_pass', 'trk_fork', 'paths_on', 'clear_on', 'auto_ran',
           'fits', 'part_on', 'kdq_last', 'auto_div', 'auto_backoff', 'shard_count')
AUTO_BURST = dict(mode=AUTO, step=0, steps=3, kd_stream=1, ext_stop=1, comm=0, whole=1, trk_on=0, trk_in_pass=0, trk_fork=0, paths_on=0, clear_on=0,
                  auto_ran=1, fits=1, part_on=0, kdq_last=-1, auto_div=8, auto_backoff=0, shard_count=1000)
TRACKED_BURST = dict(AUTO_BURST, mode=KD, kd_stream=0, auto_ran=0, trk_on=1, trk_in_pass=1, trk_fork=1)
K4_SCENE_OBS, K4_SCENES, K4_GRID, K4_PLAIN = range(4)
ON_K4, ON_HARVEST, ON_OTHERS = range(3)


def step(H, base, **over):
    d = dict(base, **over)
    out = (C.c_int * 3)()
    H.forms_plan_step((C.c_int * 19)(*[d[k] for k in STEP_IN]), out)
    return tuple(out)                                                                          # (ev_moved on k_action, build ahead, fork on the last kernel)


def finish(H, scenes=0, obs=0, harvest=0, part=0, below=0, mode=KD):
    out = (C.c_int * 4)()
    H.forms_plan_finish(scenes, obs, harvest, part, below, mode, out)
    return tuple(out)                                                                          # (K4 instance, carrier, harvest runs, k_goal_flags_others runs)


def test_plan_step_the_moved_event_on_k_action(H):
    """mode == AUTO && s + 1 < steps && the kd stream && ext_stop && !comm && shard_count == n"""
    assert step(H, AUTO_BURST) == (1, 1, 0) and step(H, AUTO_BURST, step=1) == (1, 1, 0)
    assert step(H, AUTO_BURST, step=2) == (0, 0, 0) and step(H, AUTO_BURST, steps=1) == (0, 0, 0)    # the last step of a burst: no event, nothing ahead
    assert step(H, AUTO_BURST, whole=0) == (0, 1, 0)                                            # a shard: the records of the others arrive after k_action
    assert step(H, AUTO_BURST, comm=1) == (0, 1, 0)
    assert step(H, AUTO_BURST, kd_stream=0) == (0, 1, 0)                                        # (a context's first AUTO pass creates the stream: a record of its own then)
    assert step(H, AUTO_BURST, ext_stop=0) == (0, 1, 0)
    assert [step(H, AUTO_BURST, mode=m, auto_ran=0)[0] for m in (KD, GRID, HOSTBUILD)] == [0, 0, 0]
    assert step(H, AUTO_BURST, clear_on=1)[0] == 1 and step(H, AUTO_BURST, auto_ran=0)[0] == 1  # (none of the build-ahead's own terms is one of this event's)


def test_plan_step_the_build_ahead(H):
    """mode == AUTO && au.ran && s + 1 < steps && !clear && auto_next(fits, trk_on && trk_in_pass, part_on, last, auto_div, backoff, shard_count)"""
    assert step(H, AUTO_BURST, clear_on=1) == (1, 0, 0)                                         # k_clearance reads this step's tree
    assert step(H, AUTO_BURST, auto_ran=0) == (1, 0, 0)
    assert step(H, AUTO_BURST, mode=KD)[1] == 0 and step(H, AUTO_BURST, mode=GRID)[1] == 0
    assert [step(H, AUTO_BURST, **{k: v})[1] for k, v in (('fits', 0), ('part_on', 1), ('auto_backoff', 1), ('kdq_last', 126), ('kdq_last', 125))] == [0, 0, 0, 0, 1]
    assert step(H, AUTO_BURST, kdq_last=300, auto_div=1)[1] == 1 and step(H, AUTO_BURST, kdq_last=300, auto_div=4)[1] == 0
    assert step(H, AUTO_BURST, trk_on=1, trk_in_pass=1)[1] == 0 and step(H, AUTO_BURST, trk_on=1, trk_in_pass=0)[1] == 1      # a tracked pass is a plain kd pass
    assert step(H, AUTO_BURST, trk_on=0, trk_in_pass=1)[1] == 1


def test_plan_step_the_fork_on_the_last_kernel(H):
    """(no build ahead: that branch ends the step) s + 1 < steps && ext_stop && trk_on && trk_in_pass && trk_fork && !paths_on"""
    assert step(H, TRACKED_BURST) == (0, 0, 1) and step(H, TRACKED_BURST, mode=GRID) == (0, 0, 1)
    assert step(H, TRACKED_BURST, step=2) == (0, 0, 0)
    assert step(H, TRACKED_BURST, paths_on=1) == (0, 0, 0)                                      # the next pass's k_waypoint must come before its fork
    assert [step(H, TRACKED_BURST, **{k: 0})[2] for k in ('ext_stop', 'trk_on', 'trk_in_pass', 'trk_fork')] == [0, 0, 0, 0]
    assert step(H, TRACKED_BURST, clear_on=1, comm=1, whole=0, part_on=1) == (0, 0, 1)          # none of them is a term of the fork's
    assert step(H, TRACKED_BURST, mode=AUTO, kd_stream=1, auto_ran=1) == (1, 0, 1)              # AUTO with the tracker in the pass: kd passes, which fork
    # with a build ahead the fork does not ride -- over every flag combination (the tracker's terms exclude auto_next's)
    flags = [k for k in STEP_IN if k not in ('mode', 'step', 'steps', 'kdq_last', 'auto_div', 'auto_backoff', 'shard_count')]
    for bits in itertools.product((0, 1), repeat=len(flags)):
        got = step(H, AUTO_BURST, **dict(zip(flags, bits)))
        assert not (got[1] and got[2]), (bits, got)


def test_plan_finish_which_kernel_carries_the_event_and_which_k4_runs(H):
    """others = part_on || cnt < n; harvest = scenes.on && hv_host; the event: k_goal_flags_others if others, else k_scene_harvest if harvest, else K4.
    K4: scenes.on ? (obs_on ? <SceneObsRoots> : <SceneRoots>) : nbr_mode == SCA_NBR_GRID ? _grid : plain"""
    assert finish(H) == (K4_PLAIN, ON_K4, 0, 0) and finish(H, mode=HOSTBUILD) == (K4_PLAIN, ON_K4, 0, 0)
    assert finish(H, mode=GRID) == (K4_GRID, ON_K4, 0, 0)
    assert finish(H, scenes=1) == (K4_SCENES, ON_K4, 0, 0) and finish(H, scenes=1, mode=GRID) == (K4_SCENES, ON_K4, 0, 0)
    assert finish(H, scenes=1, obs=1) == (K4_SCENE_OBS, ON_K4, 0, 0)
    assert finish(H, obs=1) == (K4_PLAIN, ON_K4, 0, 0) and finish(H, obs=1, mode=GRID) == (K4_GRID, ON_K4, 0, 0)      # obstacle sets per scene are a scene form
    assert finish(H, scenes=1, harvest=1) == (K4_SCENES, ON_HARVEST, 1, 0) and finish(H, scenes=1, obs=1, harvest=1) == (K4_SCENE_OBS, ON_HARVEST, 1, 0)
    assert finish(H, harvest=1) == (K4_PLAIN, ON_K4, 0, 0)                                      # (a harvest block without scenes: nothing to launch)
    assert finish(H, part=1, mode=GRID) == (K4_GRID, ON_OTHERS, 0, 1) and finish(H, below=1) == (K4_PLAIN, ON_OTHERS, 0, 1)
    assert finish(H, part=1, below=1) == (K4_PLAIN, ON_OTHERS, 0, 1)
    assert finish(H, scenes=1, harvest=1, below=1) == (K4_SCENES, ON_OTHERS, 1, 1)              # k_goal_flags_others is behind the harvest: the step's last


def test_step_model_bursts_of_one_to_six_over_every_flag_combination(H):
    """A burst of S steps as sca_run_steps runs it, for every combination of the boolean inputs of both plans in every mode: the fork is ready for
    step s + 1 exactly when step s's update carried it; at most one kernel of a step carries it, and that kernel is launched; an event is chosen
    only where ext_stop and its owner (the kd stream, trk_fork) exist; the plan of step s depends on nothing after s but "another step follows"."""
    flags = [k for k in STEP_IN if k not in ('mode', 'step', 'steps', 'kdq_last', 'auto_div', 'auto_backoff', 'shard_count')]
    arr, out = (C.c_int * 19)(*[AUTO_BURST[k] for k in STEP_IN]), (C.c_int * 3)()
    at = {k: STEP_IN.index(k) for k in STEP_IN}
    fin = {key: finish(H, *key) for key in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (KD, GRID, HOSTBUILD, AUTO))}
    checked = carried = 0
    for mode in (KD, GRID, HOSTBUILD, AUTO):
        arr[at['mode']] = mode
        for bits in itertools.product((0, 1), repeat=len(flags)):
            d = dict(zip(flags, bits))
            for k, v in d.items():
                arr[at[k]] = v
            by_more = {}
            for S in range(1, 7):
                for s in range(S):
                    arr[at['step']], arr[at['steps']] = s, S
                    H.forms_plan_step(arr, out)
                    moved, ahead, fork = out
                    assert by_more.setdefault(s + 1 < S, (moved, ahead, fork)) == (moved, ahead, fork), (mode, d, s, S)
                    assert not (ahead and fork) and (s + 1 < S or (moved, ahead, fork) == (0, 0, 0)), (mode, d, s, S)
                    assert not moved or (d['ext_stop'] and d['kd_stream']), (mode, d)
                    assert not fork or (d['ext_stop'] and d['trk_fork']), (mode, d)
                    # the update of this step, in every scene / harvest form (the shard and the partition are the step's own flags)
                    # (fork: what the loop hands to the pass of step s + 1 as "the fork is ready")
                    for scenes, obs, harvest in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1)):
                        k4, carrier, hv, others = fin[(scenes, obs, harvest, d['part_on'], 1 - d['whole'], GRID if mode in (GRID, AUTO) else mode)]
                        launched = {ON_K4: 1, ON_HARVEST: hv, ON_OTHERS: others}
                        carriers = [kern for kern in (ON_K4, ON_HARVEST, ON_OTHERS) if fork and carrier == kern and launched[kern]]
                        assert len(carriers) == (1 if fork else 0), (mode, d, scenes, obs, harvest)
                        assert not fork or carriers[0] == (ON_OTHERS if others else ON_HARVEST if hv else ON_K4)      # ... and it is the step's LAST kernel
                    carried += fork
                    checked += 1
                assert not fork                                                                # nothing is left over for the next call
    assert checked == 4 * 2 ** len(flags) * 21 and carried > 1000


def test_step_refusals_say_what_they_said_in_the_order_they_were_made(H):
    """step_check / step_fault_text against the literals of sca_run_steps, sca_step_begin and sca_step_host as they stood (state, steps, mode,
    several ranks, the partition's mode -- in this order); each entry point's mask picks its own."""
    STATE, STEPS, MODE, RANKS, PART_MODE, ALL = 1, 2, 4, 8, 16, 31
    RANKS_TEXT = ('cell-owner partition over several ranks: drive the step with sca_step_begin / sca_partition_pack / [exchange] / '
                  'sca_partition_unpack / sca_partition_commit / sca_step_end (sca_amd.distributed.PartitionedStepper)')
    ARG, ST, UNSUPPORTED = -1, -3, -5

    def check(checks, state=1, steps=1, mode=KD, part=0, apart=0):
        out, text = (C.c_int * 2)(), C.create_string_buffer(256)
        H.forms_step_check(checks, state, steps, mode, part, apart, out, text, 256)
        assert out[1] == len(text.value)
        return out[0], text.value.decode()
    assert check(ALL) == (0, '') and check(ALL, steps=0, mode=AUTO) == (0, '')
    assert check(ALL, state=0, steps=-1, mode=7, part=1, apart=1) == (ST, 'sca_set_state first')
    assert check(ALL, steps=-1, mode=7, part=1, apart=1) == (ARG, 'steps must not be negative')
    assert [check(ALL, steps=0, mode=m, part=1, apart=1) for m in (-1, 4)] == [(UNSUPPORTED, 'neighbor mode not available in this build')] * 2
    assert check(ALL, mode=KD, part=1, apart=1) == (ST, RANKS_TEXT) and check(ALL, mode=GRID, part=1, apart=1) == (ST, RANKS_TEXT)
    assert check(ALL, mode=GRID, part=0, apart=1) == (0, '')
    assert [check(ALL, mode=m, part=1) for m in (KD, HOSTBUILD, AUTO)] == [(UNSUPPORTED, 'the cell-owner partition is a mode of SCA_NBR_GRID')] * 3
    assert check(ALL, mode=GRID, part=1) == (0, '')
    # sca_step_begin: the state and the partition's mode; a mode out of range is the pass's to refuse, behind its first launches as ever
    assert check(STATE | PART_MODE, state=0, mode=7, part=1) == (ST, 'sca_set_state first')
    assert check(STATE | PART_MODE, mode=7) == (0, '') and check(STATE | PART_MODE, steps=-1, part=1, apart=1, mode=GRID) == (0, '')
    assert check(STATE | PART_MODE, mode=AUTO, part=1) == (UNSUPPORTED, 'the cell-owner partition is a mode of SCA_NBR_GRID')
    # sca_policy_pass, sca_env_update, sca_active_count: the state alone; sca_step_host: the mode alone, under its own name
    assert check(STATE, state=0) == (ST, 'sca_set_state first') and check(STATE, steps=-1, mode=7, part=1, apart=1) == (0, '')
    assert check(MODE, state=0, steps=-1, mode=4, part=1, apart=1) == (UNSUPPORTED, 'neighbor mode not available in this build')
    assert check(MODE, state=0, steps=-1, mode=AUTO, part=1, apart=1) == (0, '') and check(0, state=0, steps=-1, mode=9, part=1, apart=1) == (0, '')
    src = open(os.path.join(CSRC, 'sca_hip.hip')).read()
    assert 'step_refuse(c, "sca_step_host: ", STEP_CHK_MODE, 0, neighbor_mode)' in src
    counts = {'"sca_set_state first"': 1, '"steps must not be negative"': 0, '"the cell-owner partition is a mode of SCA_NBR_GRID"': 0, 'CLR_UPDATE': 1}
    for literal, times in counts.items():                                                      # one place each (sca_get_scene_state keeps a text of its own)
        assert src.count(literal) == times, literal
    for member in ('action_stop', 'finish_stop', 'fork_ready'):
        assert not re.search(r'c->' + member + r'\b', src), member                              # arguments, no longer members of the context


def test_forms_harness_standalone_under_sanitizers():
    """the plan functions as a program of their own (FORMS_MAIN: every entry point into heap arrays of exactly the documented length, the two
    AUTO plans over every slot state on both sides of the wrap) under -fsanitize=address,undefined.  Host code only; nothing of it is loaded
    into python."""
    import subprocess
    import harness_util
    exe = os.path.join(harness_util.BUILD, 'forms_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-DFORMS_MAIN', '-Wall', '-Wextra', '-Werror', '-I' + harness_util.CSRC, '-o', exe,
                           os.path.join(harness_util.ROOT, 'tests', 'forms_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'forms_harness: ok' in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ---- the kd build -----------------------------------------------------------------------------------------------------------------------------------

def test_plan_kd_build(H, clean_env):
    P = lambda top, wave_max, block, level_passes, first_single, grid, ticket, levels, sgrid: dict(
        top=top, wave_max=wave_max, block=block, level_passes=level_passes, first_single=first_single, grid=grid, ticket=ticket, levels=levels, sgrid=sgrid)
    assert kd(H, 700) == P(1, 768, 768, 0, 0, 0, 0, 0, 5)                                       # one workgroup: no top, no level passes
    assert kd(H, 1000) == P(1, 625, 768, 0, 0, 0, 0, 1, 8)                                      # k_kd_top, cap 768: 1.25 x 500
    assert kd(H, 1000, beside=1) == P(0, 1024, 1024, 0, 0, 0, 0, 0, 5)                          # beside the re-plans: cap 1024, the tree fits one workgroup
    assert kd(H, 4096) == P(1, 640, 768, 0, 0, 0, 0, 1, 27)                                     # 1.25 x 512
    assert kd(H, 4097)['top'] == 0
    assert kd(H, 16384, beside=1) == P(0, 640, 768, 1, 4, 8 + 51 + 8, 0, 5, 104)
    assert kd(H, 100000) == P(0, 977, 1024, 1, 7, 48 + 204 + 8, 0, 8, 411)                      # 1.25 x 781.25
    assert kd(H, 4096, KD_TOP=0) == P(0, 1280, 1280, 1, 2, 2 + 6 + 8, 0, 3, 14)                 # 1.25 x 1024, cap 1536
    assert [(kd(H, 100000, hint=h)['first_single'], kd(H, 100000, hint=h)['levels']) for h in (0, 1, 5, 39, 100)] == [(7, 8), (0, 1), (4, 5), (38, 39), (38, 39)]
    assert kd(H, 100000, hint=5) == dict(kd(H, 100000), first_single=4, levels=5)               # only where the tail launch takes over
    assert [kd(H, 100000, chunk_cap=1 << 30, rank_cap=r)['ticket'] for r in (259, 260)] == [1, 0]
    assert kd(H, 100000, KD_TICKET=1)['ticket'] == 1 and kd(H, 100000, chunk_cap=100)['grid'] == 100
    for env, cap, wave_max, block in (('100', 256, 245, 256), ('512', 512, 489, 512), ('5000', 1536, 977, 1024)):      # 1.25 x 195.3125 / 390.625 / 781.25
        clean_env.setenv('SCA_KD_WAVE_CAP', env)
        t = from_env(H)
        assert t['SCA_KD_WAVE_CAP'] == cap
        got = kd(H, 100000, t=(C.c_int * len(t))(*t.values()))
        assert (got['wave_max'], got['block']) == (wave_max, block), env
