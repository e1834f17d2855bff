"""CPU: harness/skeleton.py, the numpy statement of mpe_skel_observe_batch / mpe_skel_update / mpe_skel_fit_batch, against
answers the rule alone decides (one exact bone, the lower median, the bin edges, ids and rows, a pose that already has its
lengths, the sweep order, the noise property), and the pieces around it that need no GPU."""
import json
import os
import re

import numpy as np
import pytest

import skel_cases as sc
from conftest import GOLDEN, ROOT, pkg

CASES = sc.hand_made()


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(name):
    c = CASES[name]
    c.expect(sc.run_statement(pkg('harness.skeleton'), c))


def test_chunks_and_frame_order_do_not_change_the_table():
    S = pkg('harness.skeleton')
    c = CASES['ids_and_rows_tri']
    whole = sc.run_statement(S, c)[0]
    st = S.new_state(c.tid_cap, c.bones, c.bin_width, sc.J)
    for f in reversed(range(12)):
        S.observe_sequence(st, *c.frames(slice(f, f + 1)), c.mode, c.joint_mask)
    S.length_table(st, 10)
    sc.same(st, whole, sc.KEYS_LEN)


def test_the_sweep_order_shows_in_the_bits():
    """the same frames and the same lengths with the bone list reversed: other bits, so a bit comparison sees the order"""
    S = pkg('harness.skeleton')
    _, poses, flags, n_persons, ids = sc.noise('tri', B=12)
    outs = []
    for bones in (S.BONES_18, S.BONES_18[::-1]):
        st = S.new_state(4, bones, 0.002)
        S.observe_sequence(st, poses, flags, n_persons, ids, 'tri', sc.ALL)
        S.length_table(st, 10)
        outs.append((st['len'][1], S.fit_sequence(st, poses, flags, n_persons, ids, 'tri', sc.ALL, 3)))
    assert outs[0][0].tobytes() == outs[1][0][::-1].tobytes() and (outs[0][0] > 0).all()
    assert outs[0][1]['poses'].tobytes() != outs[1][1]['poses'].tobytes()
    assert (outs[0][1]['n_bones'] == 18).all() and (outs[1][1]['n_bones'] == 18).all()


@pytest.mark.parametrize('mode', ['mlp', 'tri'])
def test_noise_property(mode):
    S = pkg('harness.skeleton')
    truth, poses, flags, n_persons, ids = sc.noise(mode)
    assert poses.shape == (200, 1, 18, 3)
    st = S.new_state(8, S.BONES_18, 0.002)
    S.observe_sequence(st, poses, flags, n_persons, ids, mode, sc.ALL)
    S.length_table(st, 10)
    out = S.fit_sequence(st, poses, flags, n_persons, ids, mode, sc.ALL, 16)
    raw, rms = sc.rms(poses, truth), sc.rms(out['poses'], truth)
    print('rms in %.6f out %.6f ratio %.4f bound %.4f; worst bone %.3f -> %.3f mm'
          % (raw, rms, rms / raw, sc.NOISE_BOUND, 1000 * out['err'][..., 0].max(), 1000 * out['err'][..., 1].max()))
    assert abs(rms / raw - sc.NOISE_RATIO) < 5e-4           # the figure written beside the bound is this run's
    assert rms < raw * sc.NOISE_BOUND
    assert (out['n_bones'] == 18).all() and (out['err'][..., 1] < out['err'][..., 0]).all()
    assert st['out_of_range'] == 0 and (st['count'][1] == 200).all() and (st['len'][1] > 0).all() and not st['len'][0].any()


def test_summary_and_report_line():
    S = pkg('harness.skeleton')
    c = CASES['ids_and_rows_tri']
    ln, fit = sc.run_statement(S, c)
    s = S.SkeletonSummary()
    s.add(c.poses[12:13], fit)
    s.add(c.poses[:0], {k: fit[k][:0] for k in sc.KEYS_FIT})
    r = s.result(ln)
    assert r == {'tracks': 2, 'rows': 2, 'bones': 2, 'over_ids': 12, 'out_of_range': 0, 'err_mean_mm': [1000 * (1.0 - sc.L32 - sc.L64) / 2, 0.0],
                 'err_max_mm': [1000 * (0.5 - sc.L32), 0.0], 'mean_move_mm': 1000 * (0.1865234375 + 0.1240234375) / 2}
    assert S.report_line(16, 2.0, 10, r) == ('Bones (16 sweeps, bin 2 mm, min 10): 2 tracks, 2 rows, 2 bones, length error mean/max '
                                             '310.547/373.047 -> 0.000/0.000 mm, mean move 155.273 mm, 12 rows over the id capacity')
    assert S.report_line(16, 2.0, 10, dict(r, over_ids=0, out_of_range=3)).endswith('mean move 155.273 mm, 3 lengths out of range')
    assert S.report_line(16, 2.0, 10, dict(r, over_ids=0)).endswith('mean move 155.273 mm')


def test_skel_symbols_in_header_and_binding():
    L, S = pkg('lib'), pkg('harness.skeleton')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    names = ('mpe_skel_create', 'mpe_skel_reset', 'mpe_skel_destroy', 'mpe_skel_observe_batch', 'mpe_skel_update', 'mpe_skel_set_lengths',
             'mpe_skel_get_lengths', 'mpe_skel_fit_batch', 'mpe_skel_launches')
    for name in names:
        assert re.search(r'\bint %s\(mpe_ctx \*ctx, ' % name, hdr) and name in L.SYMBOLS
    assert sorted(n for n in L.SYMBOLS if n.startswith('mpe_skel_')) == sorted(names)
    assert sorted(set(re.findall(r'\bmpe_skel_\w+(?=\()', hdr))) == sorted(names)
    cfg = hdr[:hdr.index('} mpe_skel_config;')].rsplit('typedef struct {', 1)[1]
    assert re.findall(r'\b(\w+)(?=[,;])', re.sub(r'/\*.*?\*/', '', cfg, flags=re.S)) == [n for n, _ in L.mpe_skel_config._fields_]
    fields = [n for n, _ in L.mpe_skel_args._fields_]
    body = hdr[:hdr.index('} mpe_skel_args;')].rsplit('typedef struct {', 1)[1]
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|pose_f64|joint_flags|iters|joint_mask|reserved)\b',
                      re.sub(r'/\*.*?\*/', '', body, flags=re.S)) == fields
    defs = {n: re.search(r'#define %s \(?(\d+)u?(?: << (\d+))?\)?' % n, hdr).groups()
            for n in ('MPE_SKEL_BINS', 'MPE_SKEL_MAX_BONES', 'MPE_SKEL_MAX_ITERS', 'MPE_SKEL_OVER_IDS', 'MPE_SKEL_MAX_HIST_BYTES')}
    vals = tuple(int(a) << int(b or 0) for a, b in defs.values())
    assert vals == (512, 32, 64, 1, 256 << 20)
    assert vals == (L.MPE_SKEL_BINS, L.MPE_SKEL_MAX_BONES, L.MPE_SKEL_MAX_ITERS, L.MPE_SKEL_OVER_IDS, L.MPE_SKEL_MAX_HIST_BYTES)
    assert vals == (S.BINS, S.MAX_BONES, S.MAX_ITERS, S.OVER_IDS, S.MAX_HIST_BYTES)


def test_bones_18_is_the_skeleton_of_the_joint_names():
    S = pkg('harness.skeleton')
    with open(os.path.join(GOLDEN, 'skeleton', 'human_pose.json')) as fh:
        ref = json.load(fh)
    assert len(ref['keypoints']) == 18 == len(pkg('parameters').parameters.joint_list) and ref['keypoints'][17] == 'neck'
    assert {frozenset(b) for b in S.BONES_18} == {frozenset(b) for b in ref['skeleton']} and len(S.BONES_18) == len(ref['skeleton']) == 18
    assert S.BONES_18 == ((17, 0), (0, 1), (0, 2), (1, 3), (2, 4), (17, 5), (17, 6), (5, 7), (6, 8), (7, 9), (8, 10), (17, 11), (17, 12),
                          (11, 12), (11, 13), (12, 14), (13, 15), (14, 16))
    reached = {17}
    for parent, child in S.BONES_18:                         # every parent before its subtree
        assert parent in reached
        reached.add(child)
    assert reached == set(range(18))


def test_bones_flags_are_opt_in():
    a = pkg('harness.common').build_parser('x').parse_args([])
    assert (a.bones, a.bones_min, a.bones_bin, a.track) == (0, 10, 2.0, False)
    a = pkg('harness.common').build_parser('x').parse_args(['--bones', '8', '--bones-min', '2', '--bones-bin', '4'])
    assert (a.bones, a.bones_min, a.bones_bin) == (8, 2, 4.0)
    assert 'up to and including' in ' '.join(pkg('harness.common').build_parser('x').format_help().split())
    for bad in (['--bones', '65'], ['--bones', '-1'], ['--bones', '8', '--bones-bin', '0']):          # before any work is done
        with pytest.raises(ValueError, match='--bones'):
            pkg('harness.common').run(pkg('harness.common').build_parser('x').parse_args(bad), 'tri')


def test_bad_parameters():
    S = pkg('harness.skeleton')
    c = CASES['one_bone_tri']
    for bones in ([], [(0, 0)], [(0, 18)], [(-1, 2)], [(0, 1)] * 33, [(0, 1, 2)]):
        with pytest.raises(ValueError):
            S.new_state(8, bones, 0.002)
    for tid_cap, width in ((0, 0.002), (8, 0.0), (8, float('nan')), (8, float('inf')), ((256 << 20) // 2048 + 1, 0.002)):
        with pytest.raises(ValueError):
            S.new_state(tid_cap, [(17, 0)], width)
    st = S.new_state(8, [(17, 0)], 0.002)
    for iters in (0, 65):
        with pytest.raises(ValueError):
            S.fit_sequence(st, *c.frames(slice(0, 1)), 'tri', sc.ALL, iters)
    with pytest.raises(ValueError):
        S.set_lengths(st, np.zeros((8, 2)))
