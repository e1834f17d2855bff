"""CPU: the time-lag statement harness/lag.py and the host rule csrc/lag_pick.h on their own -- the declarations and the
binding, the statement tied to the calibration statement at W = 0, true lags recovered from true poses, the pick against
the stand-alone program bit for bit, the re-pairing of a recording and the alternation on triangulated poses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lag_cases as lc
from conftest import ROOT, pkg

LAG_FUNCTIONS = ('create', 'reset', 'destroy', 'batch', 'launches', 'read', 'estimate')
_made = {}


def LG():
    return pkg('harness.lag')


def scene(key, *a, **kw):
    if key not in _made:
        _made[key] = lc.Scene(*a, **kw)
    return _made[key]


def on_grid():
    return scene('on grid', 'panoptic', 16, (0, 1, -2, 0.5, 0.25), seed=5101)


def off_grid():
    return scene('off grid', 'panoptic', 16, (0, 0.37, -1.3, 2.6, -0.1), seed=5102, weave=0.05)


def test_declarations_binding_and_struct_layout(tmp_path):
    """include/mpe.h declares the seven mpe_lag_* functions, lib.SYMBOLS binds exactly those, and the three structs (and
    the per-camera report) have the sizes and offsets a C compiler gives the header's."""
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        header = fh.read()
    want = {'mpe_lag_' + s for s in LAG_FUNCTIONS}
    assert {n for n in re.findall(r'\b(mpe_[a-z0-9_]+)\s*\(', header) if n.startswith('mpe_lag_')} == want
    assert {n for n in L.SYMBOLS if n.startswith('mpe_lag_')} == want
    assert not any(n.startswith('mpe_sync_') for n in want)
    structs = {'mpe_lag_config': L.mpe_lag_config, 'mpe_lag_args': L.mpe_lag_args, 'mpe_lag_cam_report': L.mpe_lag_cam_report,
               'mpe_lag_report': L.mpe_lag_report}
    gcc = shutil.which('gcc') or shutil.which('cc')
    assert gcc, 'no host C compiler'
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mpe.h"', 'int main(void) {']
    for name, st in structs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in st._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines.append('printf("caps %d %d %d\\n", MPE_LAG_MAX_WINDOW, MPE_LAG_MAX_SUB, MPE_LAG_FEW_OBS | MPE_LAG_EDGE << 4 | MPE_LAG_FLAT << 8); return 0; }')
    (tmp_path / 'layout.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'layout')
    subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', exe],
                   check=True, capture_output=True, timeout=120)
    got = dict(ln.rsplit(' ', 1) for ln in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines())
    for name, st in structs.items():
        assert int(got[name + ' size']) == C.sizeof(st), name
        for field, _ in st._fields_:
            assert int(got['%s %s' % (name, field)]) == getattr(st, field).offset, (name, field)
    assert got['caps %d %d' % (L.MPE_LAG_MAX_WINDOW, L.MPE_LAG_MAX_SUB)] == str(L.MPE_LAG_FEW_OBS | L.MPE_LAG_EDGE << 4 | L.MPE_LAG_FLAT << 8)
    assert (LG().FEW_OBS, LG().EDGE, LG().FLAT, LG().MAX_WINDOW, LG().MAX_SUB) == (1, 2, 4, 8, 8)


@pytest.mark.parametrize('huber', [0.0, 5.0])
def test_window_zero_is_the_calibration_cost(huber):
    """W = 0 (K = 1): the one cost of every camera is the calibration statement's acc[c][27] at the engine's extrinsics,
    bit for bit, and the counts agree -- every id of the scene is >= 0, so nothing is unsupported."""
    CB = pkg('harness.calibrate')
    s = scene('w0', 'panoptic', 12, (0, 1, -2, 0.5, 0.37), seed=5100, weave=0.05)
    got = s.one_pass(0, 1, huber_px=huber)
    want = CB.calib_pass_host(s.calib, CB.start_extrinsics(s.calib), s.pb, s.persons, s.n_persons, s.truth, s.flags, lc.ALL_JOINTS, huber_px=huber)
    assert got['cost'].shape == (5, 1) and lc.same_bits(got['cost'][:, 0], want['acc'][:, 27])
    assert np.array_equal(got['n_obs'][:, 0], want['n_obs']) and np.array_equal(got['n_skipped'][:, 0], want['n_skipped'])
    assert np.array_equal(got['n_support'], want['n_obs'] + want['n_skipped']) and not got['n_unsupported'].any()
    assert want['n_obs'].min() > 300 and want['acc'][1:, 27].min() > 0.0


def test_true_lags_from_true_poses():
    """Straight walks, exact detections, true poses at the integer frames.  Lags on the grid: k_best is the true index and
    the mean cost there is exactly 0.0.  Lags off the grid (0.37 at sub = 4), weaving walks: the refined lag lies within the
    grid's own half step, 1 / (2 * sub), of the truth."""
    s = on_grid()
    rep = LG().lag_estimate_host(s.one_pass(3, 4), 3, 4, 50)
    assert rep['k_best'].tolist() == lc.true_k(s, 4) == [0, 4, -8, 2, 1]
    assert np.all(rep['cost_best'] == 0.0) and not rep['status'].any()
    assert lc.same_bits(rep['lag_grid'], np.array(s.lags, np.float64)) and rep['cost_zero'][0] == 0.0 and np.all(rep['cost_zero'][1:] > 1.0)
    assert rep['n_support'].min() > 300 and rep['n_unsupported'].min() > 150                 # the windows at either end reach outside
    s = off_grid()
    rep = LG().lag_estimate_host(s.one_pass(3, 4), 3, 4, 50)
    err = np.abs(rep['lag_refined'] - np.array(s.lags))
    print('refined', rep['lag_refined'].tolist(), 'error', err.tolist())
    assert np.all(err < 1.0 / (2 * 4)) and not rep['status'].any()


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = str(tmp_path_factory.mktemp('lag_pick') / 'lag_pick_test')
    subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'lag_pick_test.cpp'), '-o', out],
                   check=True, capture_output=True, timeout=300)
    return out


def test_pick_header_equals_the_statement(exe, tmp_path):
    """csrc/lag_pick.h through the stand-alone program against lag_pick, bit for bit: the curves of the two scenes above
    at several min_obs, and hand-made curves -- the minimum at either edge, a flat curve, a tie (the lowest index), NaN
    entries, an invalid neighbour, an invalid zero entry, too few observations, an offset at its bound."""
    cases = list(lc.curves())
    for name, s in (('on grid', on_grid()), ('off grid', off_grid())):
        sums = s.one_pass(3, 4)
        for c in range(5):
            for min_obs in (1, 50, 10 ** 6):
                cases.append(('%s camera %d' % (name, c), sums['cost'][c].tolist(), sums['n_obs'][c].tolist(), 3, 4, min_obs))
    words = [float(len(cases))]
    for _, cost, n_obs, W, sub, min_obs in cases:
        assert len(cost) == len(n_obs) == 2 * W * sub + 1
        words += [float(W), float(sub), float(min_obs)] + [float(x) for x in cost] + [float(x) for x in n_obs]
    src, dst = str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')
    np.asarray(words, np.float64).tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    got = np.fromfile(dst, np.float64).reshape(len(cases), 7)
    seen = set()
    for row, (name, cost, n_obs, W, sub, min_obs) in zip(got, cases):
        want = LG().lag_pick(cost, n_obs, W, sub, min_obs)
        flat = np.array([want[k] for k in ('status', 'k_best', 'lag_grid', 'lag_refined', 'cost_best', 'cost_zero', 'n_obs')], np.float64)
        assert lc.same_bits(row, flat), (name, row.tolist(), flat.tolist())
        seen.add((name, want['status'], want['k_best']))
    picked = {n: (s, k) for n, s, k in seen}
    E, F, Fw = LG().EDGE, LG().FLAT, LG().FEW_OBS
    assert picked['edge low'] == (E, -2) and picked['edge high'] == (E, 2) and picked['flat'] == (E, -3) and picked['tie'] == (0, -1)
    assert picked['nan entries'] == (E, 3) and picked['nan neighbour'] == (F, 0) and picked['all nan'] == (E, -2)
    assert picked['inf neighbours'] == (F, 0) and picked['invalid neighbour'] == (E, 0) and picked['invalid zero'] == (E, -1)
    assert picked['few'] == (Fw, 0) and picked['one entry'] == (E, 0) and picked['parabola'] == (0, 1)
    half = LG().lag_pick(*[c for c in lc.curves() if c[0] == 'half step'][0][1:])         # the offset's bound: the upper neighbour ties
    assert half['lag_refined'] == 0.5 and half['k_best'] == 0 and half['status'] == 0
    assert LG().lag_pick([4.0, 1.0, 4.0], [2, 2, 2], 1, 1, 1)['lag_refined'] == 0.0
    with pytest.raises(ValueError):
        LG().lag_estimate_host({'cost': np.zeros((1, 1)), 'n_obs': np.zeros((1, 1), np.int64), 'n_support': [0], 'n_unsupported': [0]}, 0, 1, 0)


def test_retime_frames():
    """Frame f takes camera c's entry of frame f - shift[c]: either way, nothing at the recording's ends, the held camera
    and an unnamed camera untouched, the input unchanged."""
    frames = [{'a': ('a', f), 'b': ('b', f), 'c': ('c', f), 'x': ('x', f)} for f in range(6)]
    del frames[3]['c']
    before = [dict(f) for f in frames]
    out = LG().retime_frames(frames, ['a', 'b', 'c'], [0, 2, -1])
    assert frames == before and len(out) == 6
    for f in range(6):
        assert out[f]['a'] == ('a', f) and out[f]['x'] == ('x', f)
        assert out[f].get('b') == (('b', f - 2) if f >= 2 else None)
        assert out[f].get('c') == (('c', f + 1) if f + 1 < 6 and f + 1 != 3 else None)
    assert LG().retime_frames(frames, ['a', 'b', 'c'], {'b': 0}) == frames
    assert LG().retime_frames(frames, ['a'], [7]) == [{k: v for k, v in f.items() if k != 'a'} for f in frames]
    assert LG().relative_shifts([0.3, 2.5, -1.5, 0.79, -0.2], 0) == [0, 2, -2, 0, -1] and LG().relative_shifts([1.0, 1.4, -1.2], 1) == [0, 0, -3]
    assert [g[0] for g in LG().grid(1, 3)] == [-3, -2, -1, 0, 1, 2, 3] and [g[1:3] for g in LG().grid(1, 3)][:4] == [(-1, 0), (-1, 1), (-1, 2), (0, 0)]
    assert LG().grid(8, 4)[-1][1:] == (8, 0, 0.0) and len(LG().grid(8, 4)) == 65
    with pytest.raises(ValueError):
        LG().grid(9, 1)


def test_alternation_on_triangulated_poses():
    """The realistic case by the numpy route alone: poses triangulated (the oracle's DLT restatement) from the
    desynchronised detections themselves, lags (0, 2, -1, 0, 1): the rounds apply exactly the true integer shifts within
    three rounds and the round after applies nothing."""
    applied, total = lc.alternate_host(**lc.ALTERNATION)
    print('applied per round', applied)
    assert total == [0, 2, -1, 0, 1] and len(applied) <= 4 and not any(applied[-1])
