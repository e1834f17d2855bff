"""CPU: harness/track_score.py, the numpy statement of mpe_track_score_batch / _result, against answers the rule alone
decides; its IDTP against scipy's assignment and brute force; chunk invariance; csrc/assign_int.h as a stand-alone
program under AddressSanitizer and UBSan."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_score_cases as tsc
from conftest import ROOT, pkg

CASES = tsc.hand_made()


def run(case, chunks=()):
    T = pkg('harness.track_score')
    ref = T.TrackScoreRef(case.threshold_mm, case.gid_cap, case.tid_cap)
    frames = tsc.in_chunks(lambda a, skip: ref.update(joint_flags=case.joint_flags, skip=skip, **a), case, chunks)
    return frames, ref.result(), ref.state()


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(name):
    frames, result, _ = run(CASES[name])
    tsc.check(result, frames, CASES[name], name)


def test_the_cases_cover_what_they_claim():
    assert len(CASES) >= 14 and all(c.cap <= 6 and len(c.n_gt) <= 40 for c in CASES.values())
    c = tsc.random_sequence(1, 0)
    _, r, st = run(c)
    # the generator reaches every branch of the rule
    assert r['idsw'] > 0 and r['frag'] > 0 and r['ignored'] > 0 and r['over_ids'] > 0 and r['fp'] > 0 and r['fn'] > 0 and r['tp'] > 0
    assert r['status'] == 1 and r['frames'] < 40 and (np.flatnonzero(st['pred_count']) >= 1000).all()


@pytest.mark.parametrize('joint_flags', [0, 1])
def test_chunking_changes_nothing(joint_flags):
    c = tsc.random_sequence(3 + joint_flags, joint_flags)
    whole = run(c)
    for chunks in ((1, 7), (1,) * 39, (13, 13)):
        tsc.same(*run(c, chunks), *whole, what=str(chunks[:3]))


def brute(table):
    t = table if table.shape[0] <= table.shape[1] else table.T
    n, m = t.shape
    return max(sum(int(t[i, p[i]]) for i in range(n)) for p in itertools.permutations(range(m), n)) if n else 0


def test_idtp_against_scipy_and_brute_force():
    T = pkg('harness.track_score')
    scipy_optimize = pytest.importorskip('scipy.optimize')
    rng = np.random.RandomState(0)
    for k in range(200):
        n, m = rng.randint(1, 13), rng.randint(1, 31)
        table = rng.randint(0, [4, 50, 2 ** 31 - 1][k % 3], size=(n, m)).astype(np.int64)
        table[rng.rand(n, m) < 0.5] = 0
        if k % 2:
            table = table.T
        ref = T.TrackScoreRef(gid_cap=table.shape[0], tid_cap=table.shape[1])
        ref.table[:] = table
        rows, cols = scipy_optimize.linear_sum_assignment(table, maximize=True)
        assert ref.result()['idtp'] == int(table[rows, cols].sum()), (k, table)
    for k in range(100):
        n, m = rng.randint(0, 7), rng.randint(0, 7)
        table = rng.randint(0, 6, size=(n, m))
        assert T.assign_int_max(table) == brute(table), table
    assert T.assign_int_max(np.zeros((3, 0), np.int32)) == 0 and T.assign_int_max(np.zeros((4, 4), np.int32)) == 0


def test_result_ratios_and_classes():
    T = pkg('harness.track_score')
    ref = T.TrackScoreRef(gid_cap=8, tid_cap=8)
    r = ref.result()
    assert all(r[k] != r[k] for k in ('mota', 'motp_mm', 'idp', 'idr', 'idf1')) and r['idtp'] == 0 and r['n_ids'] == 0
    # 5 * matched >= 4 * present: mostly tracked; 5 * matched < present: mostly lost; in integers, at the edges
    ref.present[:6] = (5, 5, 5, 5, 10, 1)
    ref.matched[:6] = (4, 3, 1, 0, 1, 0)
    r = ref.result()
    assert (r['mt'], r['pt'], r['ml'], r['n_ids']) == (1, 2, 3, 6)


def test_assign_int_header_under_sanitizers(tmp_path):
    """csrc/assign_int.h built for the host with -fsanitize=address,undefined and run against brute force inside the
    program (tests/native/assign_int_test.cpp): rectangular both ways, zero rows and columns, ties, entries near 2^31."""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'assign_int_test')
    subprocess.run([gxx, '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'assign_int_test.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r'tested (\d+) bad (\d+)', r.stdout)
    assert m and int(m.group(1)) > 600 and int(m.group(2)) == 0, r.stdout


def test_abi_and_flags_are_declared():
    """lib.py's structs follow include/mpe.h field for field, and the harness has the flags."""
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        header = fh.read()
    for name, struct in (('mpe_track_score_args', L.mpe_track_score_args), ('mpe_track_score_totals', L.mpe_track_score_totals)):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % name, header).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [f.strip().lstrip('*') for decl in body.split(';') if decl.strip() for f in decl.strip().split(None, 1)[1].replace(
            'int32_t', '').replace('uint8_t', '').replace('double', '').replace('const', '').split(',')]
        assert fields == [f for f, _ in struct._fields_], (name, fields)
    for sym in ('create', 'reset', 'destroy', 'batch', 'launches', 'result', 'read'):
        assert 'mpe_track_score_' + sym in L.SYMBOLS
    args = pkg('harness.common').build_parser('x').parse_args(['--synthetic', '4', '--track-score'])
    assert args.track_score and args.track_score_mm == 150.
    with pytest.raises(ValueError):
        pkg('pipeline').Tracker(None, 'gtx', 2, 0.5, 4)
