"""CPU: the time-aware refinement statement harness/refine_timed.py on its own -- the declaration and the binding, every lag
zero against harness/refine.py bit for bit, an exact lagged scene solved from the true table and from the untimed result,
one round against the table the untimed refinement made, chunking, and which cameras are timed on the messy table."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refine_timed_cases as tc
from conftest import ROOT, pkg

_made = {}


def made(key, maker):
    if key not in _made:
        _made[key] = maker()
    return _made[key]


def exact_scene():
    return made('exact', lambda: tc.Scene('panoptic', 24, tc.LAGS))


def untimed_of_exact():
    return made('exact untimed', lambda: tc.untimed(exact_scene(), 'triang'))


def messy_scene():
    return made('messy', lambda: tc.messy('panoptic', 14, tc.MESSY_LAGS))


def test_declaration_binding_and_struct_layout(tmp_path):
    """include/mpe.h declares mpe_refine_timed_batch with pointer and struct arguments only, lib.SYMBOLS binds it, and the
    argument struct has the size and the offsets a C compiler gives the header's."""
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        header = fh.read()
    assert re.search(r'\bint mpe_refine_timed_batch\(mpe_ctx \*ctx, void \*stream, const mpe_batch \*b, const mpe_refine_timed_args \*a\);', header)
    assert [n for n in L.SYMBOLS if n.startswith('mpe_refine_')] == ['mpe_refine_batch', 'mpe_refine_timed_batch']
    assert L.SYMBOLS['mpe_refine_timed_batch'][1][:2] == [C.c_void_p, C.c_void_p] and L.MPE_REFINE_TIMED_MAX_LAG == L.MPE_LAG_MAX_WINDOW == 8
    gcc = shutil.which('gcc') or shutil.which('cc')
    assert gcc, 'no host C compiler'
    st = L.mpe_refine_timed_args
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mpe.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(mpe_refine_timed_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mpe_refine_timed_args, %s));' % (f, f) for f, _ in st._fields_]
    lines.append('return 0; }')
    (tmp_path / 'layout.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'layout')
    subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', exe],
                   check=True, capture_output=True, timeout=120)
    got = dict(ln.rsplit(' ', 1) for ln in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_split_lag():
    """s = floor(L), alpha = L - s; a lag that is not finite or beyond the window is refused."""
    M = tc.RT()
    assert [M.split_lag(x) for x in (0, 0.5, -0.25, 1.25, -1.5, -2, 8, -8, -0.0)] == \
        [(0, 0.0), (0, 0.5), (-1, 0.75), (1, 0.25), (-2, 0.5), (-2, 0.0), (8, 0.0), (-8, 0.0), (0, 0.0)]
    s, alpha = M.split_lag(-0.1)
    assert s == -1 and alpha == -0.1 - (-1.0) and 0.0 <= alpha < 1.0       # one subtraction, rounded once
    for bad in (float('nan'), float('inf'), 8.5, -9):
        with pytest.raises(ValueError):
            M.split_lag(bad)


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_all_lags_zero_is_the_untimed_refinement(kind):
    """(a) every output equals harness.refine.refine bit for bit on the messy scene, and nothing is timed."""
    s = messy_scene()
    for huber in (0.0, 5.0):
        got = tc.statement(s, kind, [0.0] * 5, huber_px=huber)
        want = tc.untimed(s, kind, huber_px=huber)
        for k in tc.SHARED:
            assert tc.same_bits(got[k], want[k]), (kind, huber, k)
        assert not got['n_timed'].any() and (got['status'] & 2).any()


def test_exact_scene_true_table():
    """(b) exact detections of lagged cameras, the true table: at the truth the timed cost is exactly 0.0 and nothing moves;
    from where the untimed refinement ends, the timed rule returns to the truth within 1e-9 m (the project's DLT bar;
    measured 6e-16); the untimed refinement itself ends more than 5 mm RMS from the truth it started at (measured 11.4)."""
    s = exact_scene()
    truth = s.truth
    at_truth = tc.statement(s, 'triang', tc.LAGS)
    full = tc.every_camera_timed(s, 'triang', tc.LAGS, at_truth)              # every observing camera with a lag is timed
    solved = (at_truth['status'] & 1) != 0
    seen_by_all = at_truth['n_views'] == 5                                    # lags -1.5 and 1.25 reach two frames either way
    assert np.array_equal(full[2:22], solved[2:22]) and not (full & seen_by_all)[[0, 1, 22, 23]].any() and full.sum() > 600
    print('joints with every camera timed', int(full.sum()), 'max cost0', at_truth['cost0'][full].max())
    assert np.all(at_truth['cost0'][full] == 0.0) and not (at_truth['status'][full] & 2).any()
    assert tc.same_bits(at_truth['poses'][full], truth[full])
    plain = untimed_of_exact()
    away = tc.rms_mm(plain['poses'], truth, full)
    back = tc.statement(s, 'triang', tc.LAGS, start=plain['poses'])
    worst = float(np.linalg.norm(back['poses'] - truth, axis=-1)[full].max())
    print('untimed refinement: %.2f mm RMS from the truth, mean start cost %.1f px^2; timed from there: worst %.2e m'
          % (away, plain['cost0'][full].mean(), worst))
    assert away > 5.0
    assert worst < 1e-9


@pytest.mark.parametrize('weave', [0.0, 0.05])
def test_table_from_the_untimed_result(weave):
    """(c) the realistic case: the table is what the untimed refinement made of the lagged detections, so the offsets come
    from wrong poses.  One round brings the RMS error over frames 6..17 below a quarter of the untimed one (measured: 0.04
    of it on straight walks, 0.10 with weave = 0.05)."""
    s = exact_scene() if weave == 0.0 else made('weave', lambda: tc.Scene('panoptic', 24, tc.LAGS, weave=0.05))
    plain = untimed_of_exact() if weave == 0.0 else tc.untimed(s, 'triang')
    got = tc.statement(s, 'triang', tc.LAGS, table=tc.table_of(s, 'triang', plain['poses']))
    where = np.zeros(s.truth.shape[:3], bool)
    where[6:18, :2] = True
    where &= (got['status'] & 1) != 0
    before, after = tc.rms_mm(plain['poses'], s.truth, where), tc.rms_mm(got['poses'], s.truth, where)
    print('weave', weave, 'untimed %.3f mm, one timed round %.3f mm, ratio %.3f' % (before, after, after / before))
    assert np.array_equal(tc.every_camera_timed(s, 'triang', tc.LAGS, got)[6:18], ((got['status'] & 1) != 0)[6:18]) and where.sum() > 400
    assert after < 0.25 * before


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_chunks_give_the_bits_of_the_whole(kind):
    """(d) frames [a, b) packed on their own against the whole table: the bits of the whole-recording call."""
    s = messy_scene()
    whole = tc.statement(s, kind, tc.MESSY_LAGS, huber_px=5.0)
    for a, b in ((0, 5), (5, 12), (12, 14), (7, 8)):
        part = tc.statement(s, kind, tc.MESSY_LAGS, frames=(a, b), huber_px=5.0)
        for k in tc.KEYS:
            assert tc.same_bits(part[k], whole[k][a:b]), (kind, a, b, k)
    empty = tc.statement(s, kind, tc.MESSY_LAGS, frames=(3, 3))
    assert all(empty[k].shape[0] == 0 for k in tc.KEYS)


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_timed_cameras_on_the_messy_table(kind):
    """(e) lags (0, 1.5, -0.5, 0, 2) on lc.messy: n_timed is what the rule gives joint by joint in plain loops, and in
    particular: the row whose id is -1 has no timed camera (and is still solved); the duplicate id does not shadow the
    lowest row; the NaN neighbour and a dropped flag untime exactly the joints they hit; the table's first and last frames
    lose the cameras whose neighbours lie outside.  An untimed camera has a zero offset: the joint's result is that of the
    statement with that camera's lag set to 0."""
    s = messy_scene()
    poses, flags, mask = s.kinds[kind]
    F, m, P = 14, 7, 3
    row = lambda f, b: int(s.row_of[f, b])                   # noqa: E731
    out = tc.statement(s, kind, tc.MESSY_LAGS)
    want = tc.expected_timed(s, kind, tc.MESSY_LAGS)
    assert np.array_equal(out['n_timed'], want.sum(axis=2).astype(np.uint8))
    assert (out['n_timed'] <= out['n_views']).all() and out['n_timed'].max() == 3 and (out['status'] & 1)[out['n_timed'] > 0].any()
    j = 5                                                    # in both masks
    used = [q for q in range(tc.J) if mask >> q & 1]
    # the absent id: frame m, body 0
    lost = out['n_timed'][m, row(m, 0)]
    assert not lost.any() and (out['status'][m, row(m, 0), used] & 1).all()
    assert not want[m - 2, row(m - 2, 0), 4].any() and not want[m - 1, row(m - 1, 0), 1].any()       # lag 2 and lag 1.5 reach frame m
    # the duplicate id in frame m + 2 (row P, other coordinates): camera 4 (lag 2, alpha 0) of frame m reads body 1's own row
    d, has = tc.RT().offsets(0, F, poses, flags, s.n_persons, s.ids, tc.MESSY_LAGS)
    assert s.ids[m + 2, P] == 1 and row(m + 2, 1) < P and has[m, row(m, 1), 4, j]
    X = poses.astype(np.float64)
    assert tc.same_bits(d[m, row(m, 1), 4, j], X[m + 2, row(m + 2, 1), j] - X[m, row(m, 1), j])
    assert not out['n_views'][m + 2, P].any() and not out['n_timed'][m + 2, P].any()
    # the NaN of body 1, joint 4, frame m - 2: frame m - 4 loses camera 4 for that joint only
    assert not has[m - 4, row(m - 4, 1), 4, 4] and has[m - 4, row(m - 4, 1), 4, 5]
    if kind == 'triang':
        dropped = np.argwhere(flags[m + 3:m + 5, :P] == 0)                 # a dropped joint flag two frames ahead
        assert len(dropped)
        g, r, jd = int(dropped[0][0]) + m + 3, int(dropped[0][1]), int(dropped[0][2])
        body = int(np.nonzero(s.row_of[g] == r)[0][0])
        assert not has[g - 2, row(g - 2, body), 4, jd]
    else:
        assert flags[m - 1, row(m - 1, 2)] == 0 and not has[m - 3, row(m - 3, 2), 4].any()         # the dropped row flag
    # the table's ends: frame 0 has no f - 1 (camera 2), the last frames no f + 1 / f + 2 (cameras 1 and 4)
    assert not want[0, :, 2].any() and not want[F - 1, :, 1].any() and not want[F - 1, :, 4].any() and not want[F - 2, :, 4].any()
    assert not want[F - 2, :, 1].any() and want[F - 3, :, 1].any() and want[F - 1, :, 2].any() and want[3, :, 2].any()
    assert not d[F - 1, :, 4].any() and not d[0, :, 2].any() and not d[:, :, 0].any() and not d[:, :, 3].any()
    last = tc.statement(s, kind, (0, 0, -0.5, 0, 0), frames=(F - 1, F))      # the last frame: only camera 2 is timed
    for k in tc.KEYS:
        assert tc.same_bits(last[k], out[k][F - 1:]), k


def test_cli_options(tmp_path):
    """The part of the scripts that needs no GPU: absent options parse to "off"; --lags reads the file harness.lag writes, a
    bare dict and a list; it refuses a camera the rig does not use, and a run without --track."""
    import json
    CM = pkg('harness.common')
    a = pkg('harness.lag').build_own_parser().parse_args([])
    assert (a.correct, a.correct_inner) == (0, 2)
    p = CM.add_lags_option(CM.build_parser('x'))
    assert p.parse_args([]).lags_file is None and not hasattr(CM.build_parser('x').parse_args([]), 'lags_file')
    names = ['a', 'b', 'c']
    for doc, want in (({'lags': {'b': 0.5, 'c': -1.25}, 'hold': 'a'}, [0.0, 0.5, -1.25]), ({'c': 2}, [0.0, 0.0, 2.0]), ([1, 0, 0.25], [1.0, 0.0, 0.25])):
        (tmp_path / 'l.json').write_text(json.dumps(doc))
        assert CM.load_lags(str(tmp_path / 'l.json'), names) == want
    for doc in ({'lags': {'d': 1}}, [1, 2], 3):
        (tmp_path / 'l.json').write_text(json.dumps(doc))
        with pytest.raises(ValueError):
            CM.load_lags(str(tmp_path / 'l.json'), names)
    (tmp_path / 'l.json').write_text(json.dumps({'lags': {}}))
    with pytest.raises(ValueError, match='--track'):
        CM.run(p.parse_args(['--synthetic', '2', '--lags', str(tmp_path / 'l.json')]), 'tri')
