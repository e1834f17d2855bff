"""CPU: harness/smoothing.py, the numpy statement of mpe_smooth_batch, against answers the rule alone decides (exact
lines, row swaps, fills, gaps, non-finite samples, the noise bound), and the pieces around it that need no GPU."""
import os
import re

import numpy as np
import pytest

import smooth_cases as sc
import track_cases as tc
from conftest import ROOT, pkg

CASES = sc.hand_made()


def run(c, state=None, **kw):
    S = pkg('harness.smoothing')
    return S.smooth_sequence(c.poses, c.flags, c.n_persons, c.ids, c.mode, kw.get('joint_mask', sc.ALL), kw.get('window', c.window),
                             c.decay, c.fill, state)


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(name):
    sc.check(run(CASES[name]), CASES[name])


def test_window_zero_and_joint_mask_copy_through():
    c = CASES['fill_on']
    out = run(c, window=0)
    assert out['poses'].tobytes() == c.poses.tobytes() and not out['vel'].any()
    assert (out['flags'] == (c.flags != 0)).all() and (out['n_samples'] == ((c.flags != 0) & (c.ids >= 0)[..., None])).all()
    out, full = run(c, joint_mask=sc.ALL & ~(1 << 5)), run(c)
    assert out['poses'][:, :, 5].tobytes() == c.poses[:, :, 5].tobytes() and not out['vel'][:, :, 5].any()
    assert out['flags'][:, :, 5].tobytes() == c.flags[:, :, 5].tobytes() and not out['n_samples'][:, :, 5].any()
    keep = [j for j in range(sc.J) if j != 5]
    for k in ('poses', 'flags', 'vel', 'n_samples'):
        assert out[k][:, :, keep].tobytes() == full[k][:, :, keep].tobytes(), k


def test_a_row_without_an_id_is_no_detection():
    c = sc.linear('tri', 6, 1.0)
    c.ids[4, 0] = -1
    out = run(c)
    assert out['poses'][4, 0].tobytes() == c.poses[4, 0].tobytes() and not out['n_samples'][4, 0].any()
    assert out['flags'][4, 0].tobytes() == c.flags[4, 0].tobytes()
    assert (out['n_samples'][5, 0] == 5).all() and (out['vel'][5, 0] == np.array((0.046875, -0.015625, 0.03125))).all()


@pytest.mark.parametrize('mode', ['mlp', 'tri'])
def test_noise_stays_under_the_derived_bound(mode):
    S = pkg('harness.smoothing')
    truth, poses, flags, n_persons, ids = sc.noise(mode)
    assert poses.shape == (40, 4, 18, 3)
    raw = sc.noise_rms(poses, truth)
    out = S.smooth_sequence(poses, flags, n_persons, ids, mode, sc.ALL, 6, 1.0)
    rms = sc.noise_rms(out['poses'], truth)
    print('rms in %.5f out %.5f bound %.5f' % (raw, rms, sc.NOISE_BOUND))
    assert 0.9 * sc.NOISE_SIGMA < raw < 1.1 * sc.NOISE_SIGMA
    assert rms < sc.NOISE_BOUND


@pytest.mark.parametrize('tri', [False, True])
def test_chunks_with_carried_state_give_the_bits_of_one_call(tri):
    S = pkg('harness.smoothing')
    mode = 'tri' if tri else 'mlp'
    poses, flags, n_persons, ids = sc.random_sequence(5 + tri, tri, pkg('harness.tracking'), B=37, away=tc.AWAY)
    whole = S.smooth_sequence(poses, flags, n_persons, ids, mode, sc.ALL, 3, 0.8, tri)
    state = [None]

    def step(p, f, n, i):
        out = S.smooth_sequence(p, f, n, i, mode, sc.ALL, 3, 0.8, tri, state[0])
        state[0] = out['state']
        return out
    sc.same(sc.in_chunks(step, (poses, flags, n_persons, ids), tc.CHUNKS), whole)
    # the sequence does what it is for
    assert ids.max() > 1000 and (whole['n_samples'] == 4).any() and (whole['n_samples'] == 1).any() and whole['vel'].any()
    assert not tri or (whole['flags'] == 2).any()
    assert not np.isfinite(poses).all() and np.isfinite(whole['vel']).all()


def test_summary():
    S = pkg('harness.smoothing')
    c = CASES['fill_on']
    out = run(c)
    s = S.SmoothSummary('tri')
    s.add(c.poses[:4], c.flags[:4], {k: out[k][:4] for k in ('poses', 'flags', 'n_samples')})
    s.add(c.poses[4:], c.flags[4:], {k: out[k][4:] for k in ('poses', 'flags', 'n_samples')})
    r = s.result()
    present = c.flags != 0
    assert r == {'fitted': int((present & (out['n_samples'] >= 2)).sum()), 'filled': 2, 'mean_move_mm': 0.0} and r['fitted'] > 300


def test_smooth_symbols_in_header_and_binding():
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    for name in ('mpe_smooth_create', 'mpe_smooth_reset', 'mpe_smooth_destroy', 'mpe_smooth_batch', 'mpe_smooth_launches'):
        assert re.search(r'\bint %s\(mpe_ctx \*ctx, ' % name, hdr) and name in L.SYMBOLS
    names = [n.rstrip('_') for n, _ in L.mpe_smooth_args._fields_]
    body = hdr[:hdr.index('} mpe_smooth_args;')].rsplit('typedef struct {', 1)[1]
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|pose_f64|joint_flags|fill|joint_mask|lambda)\b', re.sub(r'/\*.*?\*/', '', body, flags=re.S)) == names
    assert (L.MPE_SMOOTH_MAX_WINDOW, L.MPE_SMOOTH_FILLED) == tuple(int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
                                                                   for n in ('MPE_SMOOTH_MAX_WINDOW', 'MPE_SMOOTH_FILLED'))
    assert (pkg('harness.smoothing').MAX_WINDOW, pkg('harness.smoothing').FILLED) == (L.MPE_SMOOTH_MAX_WINDOW, L.MPE_SMOOTH_FILLED)


def test_smooth_flags_are_opt_in():
    a = pkg('harness.common').build_parser('x').parse_args([])
    assert (a.smooth, a.smooth_decay, a.smooth_fill, a.track) == (0, 0.8, False, False)
    a = pkg('harness.common').build_parser('x').parse_args(['--smooth', '4', '--smooth-decay', '0.5', '--smooth-fill'])
    assert (a.smooth, a.smooth_decay, a.smooth_fill) == (4, 0.5, True)


def test_bad_parameters():
    c = CASES['fill_on']
    S = pkg('harness.smoothing')
    for window, decay in ((16, 0.8), (-1, 0.8), (6, 0.2), (6, 1.5)):
        with pytest.raises(ValueError):
            S.smooth_sequence(c.poses, c.flags, c.n_persons, c.ids, 'tri', sc.ALL, window, decay)
