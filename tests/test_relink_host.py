"""CPU: harness/relink.py, the numpy statement of mpe_relink_batch, against answers the rule alone decides (a plain return
at the ends of the gap window, a cost at the gate, bone samples, common bones, a long bone, births and records that
compete, a continuing track, a chain, the position gate, non-finite coordinates, ids over the cap, degenerate calls), in
chunks, on a behavioural case with noise, and the pieces around it that need no GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import relink_cases as rc
from conftest import ROOT, pkg

CASES = rc.hand_made()


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(name):
    c = CASES[name]
    out, st = rc.run_statement(pkg('harness.relink'), c)
    rc.same(out, c.want, what=name)
    if c.state_check:
        c.state_check(st)


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_made_in_single_frames(name):
    """the state carries everything: frame by frame gives the bits of one call"""
    R, c = pkg('harness.relink'), CASES[name]
    rc.same(rc.run_statement(R, c, [1] * len(c.poses))[0], c.want, what=name)


def test_an_empty_call_changes_nothing():
    R, c = pkg('harness.relink'), CASES['chain_tri']
    B = len(c.poses)
    out, st = rc.run_statement(R, c, [3, 0, B - 3, 0])
    assert out['ids'].shape == (B, c.pcap)
    rc.same(out, c.want)
    c.state_check(st)
    empty, st0 = R.relink_sequence(c.poses[:0], c.flags[:0], c.n_persons[:0], c.track_ids[:0], 'tri', rc.BONES, c.options)
    assert empty['ids'].shape == (0, c.pcap) and empty['counters'].tolist() == [0, 0, 0] and st0['frame'] == 0


def test_the_state_given_is_not_modified():
    R, c = pkg('harness.relink'), CASES['chain_mlp']
    _, st = R.relink_sequence(c.poses[:4], c.flags[:4], c.n_persons[:4], c.track_ids[:4], 'mlp', rc.BONES, c.options)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    R.relink_sequence(c.poses[4:], c.flags[4:], c.n_persons[4:], c.track_ids[4:], 'mlp', rc.BONES, c.options, st)
    for k, v in before.items():
        assert np.array_equal(st[k], v), k


@pytest.mark.parametrize('tri', [False, True])
@pytest.mark.parametrize('seed', [3, 4, 5])
def test_chunks_do_not_change_the_result(seed, tri):
    R = pkg('harness.relink')
    arrays = rc.random_sequence(seed, tri)
    mode = 'tri' if tri else 'mlp'
    for options in (rc.RANDOM_OPTIONS, dict(rc.RANDOM_OPTIONS, reach_m=1.0, reach_per_frame_m=0.05)):
        whole, st = rc.statement(R, arrays, mode, options)
        parts, st2 = rc.statement(R, arrays, mode, options, rc.CHUNKS)
        rc.same(parts, whole, what=(seed, mode))
        for k in st:
            assert np.asarray(st[k]).tobytes() == np.asarray(st2[k]).tobytes(), k
        assert whole['counters'][1] >= 2 or options.get('reach_m'), whole['counters']      # the sequences do have returns


def test_wide_case_links_every_body():
    R = pkg('harness.relink')
    poses, flags, n_persons, ids = rc.wide_sequence(11, True)
    out, _ = rc.statement(R, (poses, flags, n_persons, ids), 'tri', rc.WIDE_OPTIONS)
    n = poses.shape[1]
    assert out['counters'].tolist() == [n, n, 0] and (out['link_gap'][6] == 3).all() and (out['ids'][6:] < n).all()
    assert sorted(out['ids'][6].tolist()) == list(range(n)) and (out['ids'][9] == out['ids'][6]).all()


def test_options_are_validated():
    R = pkg('harness.relink')
    assert R.check_options()['gate_m'] == 0.02 and R.check_options({'min_gap': 4.0})['min_gap'] == 4
    assert R.DEFAULTS['used_joint_mask'] == sum(1 << j for j in pkg('parameters').parameters.used_joints)
    for bad in ({'gate_m': 0.0}, {'gate_m': float('nan')}, {'gate_m': float('inf')}, {'min_gap': 0}, {'min_gap': 5, 'max_gap': 4},
                {'max_gap': (1 << 30) + 1}, {'min_samples': 0}, {'min_bones': 0}, {'min_bones': 19}, {'max_bone_m': 0.0},
                {'max_bone_m': float('inf')}, {'reach_m': -1.0}, {'reach_per_frame_m': float('nan')}, {'reach_per_frame_m': -0.1},
                {'tid_cap': 0}, {'tid_cap': 4097}, {'min_gap': 2.5}, {'joint_mask': -1}, {'used_joint_mask': 1 << 32}, {'gate': 0.02}):
        with pytest.raises(ValueError):
            R.check_options(bad, 18)
    c = CASES['chain_tri']
    with pytest.raises(ValueError):
        R.relink_sequence(*c.arrays(), 'gt', rc.BONES, c.options)
    with pytest.raises(ValueError):
        R.relink_sequence(*c.arrays(), 'tri', [(0, 0)], c.options)
    _, st = rc.run_statement(R, c)
    with pytest.raises(ValueError):
        R.relink_sequence(*c.arrays(), 'tri', rc.BONES, dict(c.options, tid_cap=9), st)


def _fragments(who, ids):
    """{body: the ids its rows carry, in order of first appearance}"""
    out = {}
    for f in range(who.shape[0]):
        for p in range(who.shape[1]):
            if who[f, p] >= 0 and ids[f, p] not in out.setdefault(int(who[f, p]), []):
                out[int(who[f, p])].append(int(ids[f, p]))
    return out


def _run_scorer(TS, who, ids):
    """harness/track_score.py on `ids` with the bodies as ground truth: body k is GT row k with identity k in EVERY frame (a
    person behind a pillar is still there, so the frames it is away are misses); every detection matches its body at 0 mm"""
    B, P = who.shape
    G = int(who.max()) + 1
    ref = TS.TrackScoreRef(150., gid_cap=G, tid_cap=64)
    ref.update(None, (who >= 0).sum(axis=1), ids, who, np.zeros((B, P)), None, np.full(B, P), np.full(B, G),
               np.tile(np.arange(G, dtype=np.int32), (B, 1)), np.ones((B, G), np.uint8), 1)
    return ref.result()


def test_behaviour_with_noise():
    """Three bodies of statures 1.33, 1.66 and 1.99 m (scales 0.8, 1.0, 1.2 of skel_cases.BODY), 3 mm of seeded Gaussian
    noise on every coordinate, 120 frames; each body is away twice for 14 to 19 frames (the tracker waits 2), the absences
    overlap, and a body returns 1.5 m from where it left.  With the DEFAULT options (min_gap = the tracker's gap + 2, as
    the harness passes it) the statement alone must make no wrong link, link every true return, price every wrong
    candidate at twice the gate or more and every true one at half the gate or less.

    Measured on harness/relink.py, mode 'tri': 6 returns, 6 links, none wrong; the true costs are 3.228, 4.362, 3.898,
    3.237, 3.487 and 2.681 mm (half the gate: 10 mm); the 3 wrong candidates (a body that returns while another is still
    away) cost 54.114, 54.938 and 109.692 mm (twice the gate: 40 mm).  The numpy scorer (harness/track_score.py), the
    bodies being the ground truth in every frame: on the tracker's ids 9 tracks, 6 ID switches, 6 fragmentations, IDF1
    0.5346; on the relinked ids 3 tracks, 0 ID switches, 6 fragmentations, IDF1 0.8406.  The scorer's fragmentation is
    CLEAR-MOT's: an identity that is matched, missed and matched again, whatever id it comes back under.  No choice of
    ids can lower it, so `fewer fragmentations` can only be asserted as `not more`; what the relinker repairs shows in
    the ID switches, the track count and IDF1, and those are asserted strictly."""
    R = pkg('harness.relink')
    poses, flags, n_persons, ids, who = rc.behaviour()
    o = R.check_options(rc.BEHAVE_OPTIONS, 18)
    assert all(o[k] == R.DEFAULTS[k] for k in R.DEFAULTS if k not in ('min_gap', 'tid_cap')) and o['min_gap'] == rc.TRACK_GAP + 2 == 4
    before = _fragments(who, ids)
    n_returns = sum(len(v) for v in rc.BEHAVE_AWAY.values())
    assert sorted(len(v) for v in before.values()) == sorted(1 + len(rc.BEHAVE_AWAY[k]) for k in range(3))     # the tracker does lose them
    out, st = rc.statement(R, (poses, flags, n_persons, ids), 'tri', rc.BEHAVE_OPTIONS)
    after = _fragments(who, out['ids'])
    assert all(len(v) == 1 for v in after.values()) and len({v[0] for v in after.values()}) == 3            # no wrong link, every return linked
    assert out['counters'].tolist() == [3, n_returns, 0]
    true = out['link_cost'][out['link_gap'] > 0]
    print('true costs (mm):', np.round(1000 * true, 3).tolist())
    assert len(true) == n_returns and (true <= 0.5 * o['gate_m']).all()
    # every candidate the rule looked at: the frame's births against the eligible records, priced again here
    wrong = []
    state = None
    for f in range(len(poses)):
        sl = slice(f, f + 1)
        if state is not None:
            for p in range(poses.shape[1]):
                t = ids[f, p]
                if t < 0 or state['canon'][t] >= 0:
                    continue
                x = poses[f, p]
                lengths = np.array([np.sqrt(((x[jc] - x[jp]) ** 2).sum()) for jp, jc in rc.BONES])
                for c in range(o['tid_cap']):
                    g = f - state['last_frame'][c]
                    if state['last_frame'][c] >= 0 and o['min_gap'] <= g <= o['max_gap'] and c != after[int(who[f, p])][0]:
                        wrong.append(float(R.bone_cost(lengths, state['sum'][c], state['cnt'][c], o['min_samples'], o['min_bones'])))
        _, state = R.relink_sequence(poses[sl], flags[sl], n_persons[sl], ids[sl], 'tri', rc.BONES, rc.BEHAVE_OPTIONS, state)
    print('wrong candidates (mm): %d, %.3f .. %.3f' % (len(wrong), 1000 * min(wrong), 1000 * max(wrong)))
    assert len(wrong) >= 3 and min(wrong) >= 2.0 * o['gate_m']

    TS = pkg('harness.track_score')
    scores = []
    for use in (ids, out['ids']):
        scores.append(_run_scorer(TS, who, use))
        print('scorer: tracks %d frag %d idsw %d idf1 %.4f' % tuple(scores[-1][k] for k in ('n_tracks', 'frag', 'idsw', 'idf1')))
    assert scores[1]['frag'] <= scores[0]['frag'] and scores[1]['idsw'] < scores[0]['idsw'] and scores[1]['idf1'] > scores[0]['idf1']
    assert scores[1]['n_tracks'] == 3 and scores[0]['n_tracks'] == 3 + n_returns


def test_relink_symbols_in_header_and_binding():
    L, R = pkg('lib'), pkg('harness.relink')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    names = ('mpe_relink_create', 'mpe_relink_reset', 'mpe_relink_destroy', 'mpe_relink_batch', 'mpe_relink_launches', 'mpe_relink_read')
    for name in names:
        assert re.search(r'\bint %s\(mpe_ctx \*ctx, ' % name, hdr) and name in L.SYMBOLS
    assert sorted(n for n in L.SYMBOLS if n.startswith('mpe_relink_')) == sorted(names)
    assert sorted(set(re.findall(r'\bmpe_relink_\w+(?=\()', hdr))) == sorted(names)
    for struct in ('mpe_relink_config', 'mpe_relink_args'):
        body = hdr[:hdr.index('} %s;' % struct)].rsplit('typedef struct {', 1)[1]
        assert re.findall(r'\b(\w+)(?=[,;])', re.sub(r'/\*.*?\*/', '', body, flags=re.S)) == [n for n, _ in getattr(L, struct)._fields_]
    assert '#define MPE_RELINK_MAX_TID_CAP 4096' in hdr and '#define MPE_RELINK_MAX_GAP (1 << 30)' in hdr and '#define MPE_RELINK_OVER_IDS 1' in hdr
    assert (L.MPE_RELINK_MAX_TID_CAP, L.MPE_RELINK_MAX_GAP, L.MPE_RELINK_OVER_IDS) == (4096, 1 << 30, 1) == (R.MAX_TID_CAP, R.MAX_GAP, R.OVER_IDS)
    assert rc.BONES == pkg('harness.skeleton').BONES_18


def test_relink_flags_are_opt_in():
    common = pkg('harness.common')
    a = common.build_parser('x').parse_args([])
    assert (a.relink, a.relink_max_gap, a.relink_reach, a.relink_speed, a.relink_min_bones, a.track) == (0.0, 150, 0.0, 0.0, 8, False)
    a = common.build_parser('x').parse_args(['--relink', '20', '--relink-max-gap', '90', '--relink-reach', '1.5', '--relink-speed', '0.05',
                                             '--relink-min-bones', '6'])
    assert (a.relink, a.relink_max_gap, a.relink_reach, a.relink_speed, a.relink_min_bones) == (20.0, 90, 1.5, 0.05, 6)
    assert 'options, not findings' in ' '.join(common.build_parser('x').format_help().split())
    for bad in (['--relink', '-1'], ['--relink', 'nan'], ['--relink', '20', '--relink-max-gap', '1'], ['--relink', '20', '--relink-reach', '-1'],
                ['--relink', '20', '--relink-min-bones', '0']):                      # before any work is done
        with pytest.raises(ValueError, match='--relink'):
            common.run(common.build_parser('x').parse_args(bad), 'tri')


def test_summary_and_report_line():
    R, c = pkg('harness.relink'), CASES['chain_tri']
    out, _ = rc.run_statement(R, c)
    s = R.RelinkSummary()
    s.add(c.track_ids[:4], {k: out[k][:4] for k in ('ids', 'link_gap')})
    s.add(c.track_ids[4:], {k: out[k][4:] for k in ('ids', 'link_gap')})
    r = s.result(out)
    assert r == {'births': 1, 'links': 2, 'tracks_before': 3, 'tracks_after': 1, 'mean_gap': 2.5, 'max_gap': 3, 'over_ids': 0}
    assert r == s.result({'births': 1, 'linked': 2, 'over_ids': 0, 'status': 0})
    assert R.report_line(20.0, 150, r) == 'Relinked (gate 20 mm, gap up to 150): 1 births, 2 links, 3 -> 1 tracks, link gap mean/max 2.500/3 frames'
    assert R.report_line(20.0, 150, dict(r, over_ids=2)).endswith('3 frames, 2 rows over the id capacity')


def test_config_checks_under_the_host_sanitizers(tmp_path):
    """csrc/relink_config.h -- what mpe_relink_create checks and the copy it keeps, host code that touches no device -- in
    a stand-alone program (tests/native/relink_config_test.cpp) built with -fsanitize=address,undefined and run as a child."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'relink_config_test')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'relink_config_test.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and re.fullmatch(r'ok \d+\n', r.stdout), r.stdout + r.stderr
