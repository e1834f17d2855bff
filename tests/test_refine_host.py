"""CPU: harness/refine.py, the numpy statement of mpe_refine_batch -- that it finds the minimum (noise-free recovery, an
independent optimiser), that it never raises the cost, what it leaves alone, Huber, the early stop -- and the pieces
around it that need no GPU (declarations, flags)."""
import os
import re

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT, env, pkg

_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = rc.Case(name)
    return _cases[name]


def RF():
    return pkg('harness.refine')


def clean():
    """The one-frame case with exact detections, started 5 cm off the bodies along every axis (float64, joint flags)."""
    if 'clean' not in _cases:
        c = case('one frame')
        flags = np.repeat((np.arange(c.pcap)[None, :] < c.n_persons[:, None])[..., None], rc.J, axis=2).astype(np.uint8)
        _cases['clean'] = (c, rc.noise_free(c), c.truth + 0.05, flags)
    return _cases['clean']


def run(c, kind, pb=None, **kw):
    poses, flags, mask = rc.kinds(c)[kind]
    return RF().refine(env().calib, pb if pb is not None else c.pb, c.persons, c.n_persons, poses, flags, mask, **kw)


def test_noise_free_recovery():
    """1: exact detections, a start 5 cm off per axis: the bodies come back to 1e-9 m, the bound the DLT stage is held to."""
    c, pb, start, flags = clean()
    out = RF().refine(env().calib, pb, c.persons, c.n_persons, start, flags, (1 << rc.J) - 1, max_iters=30, step_tol=0.0)
    solved = (out['status'] & RF().SOLVED) != 0
    err = np.linalg.norm(out['poses'] - c.truth, axis=-1)
    print('solved', int(solved.sum()), 'of', solved.size, 'worst |X - truth|', err[solved].max(), 'worst cost', out['cost1'][solved].max())
    assert solved.sum() > 40 and np.all(out['n_views'][solved] >= 2)
    assert np.all((out['status'][solved] & RF().MOVED) != 0)
    assert err[solved].max() < 1e-9
    assert np.all(out['iters'][solved] == 30) and not (out['status'] & RF().CONVERGED).any()


def scalar_residuals(obs):
    """The residual vector of one joint, written on its own: plain Python floats, one camera after the other."""
    def fn(X):
        out = []
        for P, kd, K, x, y in obs:
            pc = [P[i][0] * X[0] + P[i][1] * X[1] + P[i][2] * X[2] + P[i][3] for i in range(3)]
            a, b = pc[0] / pc[2], pc[1] / pc[2]
            r = a * a + b * b
            f = 1.0 + kd[0] * r + kd[1] * r * r + kd[2] * r ** 3
            u = [K[i][0] * a * f + K[i][1] * b * f + K[i][2] for i in range(3)]
            out += [u[0] / u[2] - x, u[1] / u[2] - y]
        return np.array(out)
    return fn


def test_same_minimum_as_scipy():
    """2: on the messy batch's triangulated poses (2 px noise) the result is scipy.optimize.least_squares' minimum.  The
    allowed distance is ten times the largest distance between scipy's own 'lm' and 'trf' answers on the same joints
    (all tolerances 1e-15), at least 1e-9 m; joints on which the two differ by more than 1e-6 m are left out, at most
    2 % of the solved ones.  Measured: 767 joints, none left out, lm-trf 1.41e-08 m, ours-lm 1.41e-08 m."""
    least_squares = pytest.importorskip('scipy.optimize').least_squares
    R, calib = pkg('harness.reprojection'), env().calib
    c = case('messy')
    poses, flags, mask = rc.kinds(c)['triang']
    out = run(c, 'triang', max_iters=64, step_tol=0.0)
    sel, xy = R.selection(c.pb, c.persons, c.n_persons, flags, mask)
    T, kd, K = RF().camera_constants64(calib)
    solved = np.argwhere((out['status'] & RF().SOLVED) != 0)
    between, ours = [], []
    for f, p, j in solved:
        obs = [(T[k].tolist(), kd[k].tolist(), K[k].tolist(), float(xy[f, p, k, j, 0]), float(xy[f, p, k, j, 1]))
               for k in range(sel.shape[2]) if sel[f, p, k, j]]
        a, b = (least_squares(scalar_residuals(obs), poses[f, p, j], method=m, xtol=1e-15, ftol=1e-15, gtol=1e-15).x for m in ('lm', 'trf'))
        between.append(np.linalg.norm(a - b))
        ours.append(np.linalg.norm(out['poses'][f, p, j] - a))
    between, ours = np.array(between), np.array(ours)
    keep = between <= 1e-6
    bound = max(10.0 * between[keep].max(), 1e-9)
    print('solved', len(solved), 'left out', int((~keep).sum()), 'scipy lm - trf', between[keep].max(), 'ours - lm', ours[keep].max(), 'bound', bound)
    assert len(solved) > 500 and (~keep).sum() <= 0.02 * len(solved)
    assert ours[keep].max() <= bound


@pytest.mark.parametrize('kind', ['est', 'triang'])
@pytest.mark.parametrize('name', ['messy', '5x10', 'hand made'])
def test_cost_never_rises_and_the_rest_is_left_alone(name, kind):
    """3: cost1 <= cost0 where solved; without MOVED the input bits and equal costs; unsolved joints keep their bits, cost
    -1 and carry the right status; n_views counts the entries reprojection.residuals counts."""
    R, M = pkg('harness.reprojection'), RF()
    c = case(name)
    poses, flags, mask = rc.kinds(c)[kind]
    out = run(c, kind, huber_px=0.0 if kind == 'est' else 5.0)
    st = out['status']
    solved, moved = (st & M.SOLVED) != 0, (st & M.MOVED) != 0
    assert out['poses'].dtype == poses.dtype and solved.any() and not (moved & ~solved).any()
    assert np.all(out['cost1'][solved] <= out['cost0'][solved]) and np.all(out['cost1'][solved] >= 0)
    assert np.all(out['cost1'][solved & ~moved] == out['cost0'][solved & ~moved])
    assert rc.same_bits(out['poses'][~moved], poses[~moved])
    assert np.all(out['cost0'][~solved] == -1.0) and np.all(out['cost1'][~solved] == -1.0) and not out['iters'][~solved].any()
    res = R.residuals(env().calib, c.pb, c.persons, c.n_persons, poses, flags, mask)
    views = (res != R.SENTINEL).sum(axis=2)
    assert np.array_equal(out['n_views'], views.astype(np.uint8))
    assert np.all(st[views == 0] == 0) and np.all(st[views == 1] == M.FEW_VIEWS)
    assert np.all(np.isin(st[views >= 2] & (M.SOLVED | M.BAD_START), (M.SOLVED, M.BAD_START)))
    if name == 'hand made':
        assert st[0, 2, 8] == M.BAD_START and (st == M.BAD_START).sum() == 1 and (views == 2).any() and (st[views == 2] & M.SOLVED).all()
        assert (views == 1).sum() == (14 if kind == 'est' else 0)
    if name == 'messy':
        assert (views == 2).any() and (views == 1).any() and (views == 0).any()


def test_huber_bounds_an_outlier():
    """4: five cameras, exact detections, one detection of one joint 80 px off: with huber_px = 5 the joint ends strictly
    closer to the body than with plain least squares, and both lower the cost."""
    c, pb0, start, flags = clean()
    import copy
    pb = copy.copy(pb0)
    pb.xy = pb0.xy.copy()
    f, p, j = 0, int(np.argmax((c.persons[0] >= 0).sum(axis=1))), 6
    assert (c.persons[f, p] >= 0).all()
    pb.xy[rc.head_of(c, f, p, 0), j] += np.array([80.0, 0.0])
    d = {}
    for huber in (0.0, 5.0):
        out = RF().refine(env().calib, pb, c.persons, c.n_persons, start, flags, (1 << rc.J) - 1, max_iters=30, step_tol=0.0, huber_px=huber)
        assert out['n_views'][f, p, j] == 5 and out['cost1'][f, p, j] < out['cost0'][f, p, j]
        d[huber] = np.linalg.norm(out['poses'][f, p, j] - c.truth[f, p, j])
    print('distance to the body: least squares', d[0.0], 'huber 5 px', d[5.0])
    assert d[5.0] < d[0.0]


def test_early_stop():
    """5: step_tol = 1e-6 stops before step_tol = 0 does, within 1e-6 m of its result."""
    c, pb, start, flags = clean()
    a = RF().refine(env().calib, pb, c.persons, c.n_persons, start, flags, (1 << rc.J) - 1, max_iters=30, step_tol=0.0)
    b = RF().refine(env().calib, pb, c.persons, c.n_persons, start, flags, (1 << rc.J) - 1, max_iters=30, step_tol=1e-6)
    solved = (a['status'] & RF().SOLVED) != 0
    assert np.array_equal(solved, (b['status'] & RF().SOLVED) != 0)
    print('iterations with the early stop', np.bincount(b['iters'][solved]).tolist())
    assert np.all(b['iters'][solved] < a['iters'][solved]) and np.all((b['status'][solved] & RF().CONVERGED) != 0)
    assert np.linalg.norm(a['poses'] - b['poses'], axis=-1).max() < 1e-6


def test_improvement_as_the_residual_kernel_sees_it():
    """6: 2 px noise: the sum of the squared float32 residuals of the refined triangulated poses is below the input's."""
    R = pkg('harness.reprojection')
    c = case('messy')
    poses, flags, mask = rc.kinds(c)['triang']
    out = run(c, 'triang')
    sq = [R.residuals(env().calib, c.pb, c.persons, c.n_persons, x, flags, mask, squared=True) for x in (poses, out['poses'])]
    before, after = (float(s[s >= 0].sum()) for s in sq)
    print('sum of squared residuals', before, '->', after)
    assert after < before


def test_flags_are_opt_in():
    """7 (the part that needs no GPU): absent flags parse to "off", and the three scripts share them."""
    a = pkg('harness.common').build_parser('x').parse_args([])
    assert (a.refine, a.refine_huber) == (0, 0.0)
    a = pkg('harness.reprojection_error').build_own_parser().parse_args(['--refine', '10', '--refine-huber', '5'])
    assert (a.refine, a.refine_huber, a.device_metrics) == (10, 5.0, False)


def test_refine_symbol_in_header_and_binding():
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    assert re.search(r'\bint mpe_refine_batch\(mpe_ctx \*ctx, void \*stream, const mpe_batch \*b, const mpe_refine_args \*a\);', hdr)
    assert 'mpe_refine_batch' in L.SYMBOLS
    names = [n for n, _ in L.mpe_refine_args._fields_]
    body = re.sub(r'/\*.*?\*/', '', hdr[:hdr.index('} mpe_refine_args;')].rsplit('typedef struct {', 1)[1], flags=re.S)
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|pose_f64|joint_flags|joint_mask|threshold|max_iters|step_tol|huber_px)\b', body) == names
    bits = {n: int(v) for n, v in re.findall(r'MPE_REFINE_(\w+) = (\d+)', hdr)}
    assert bits == {'SOLVED': L.MPE_REFINE_SOLVED, 'MOVED': L.MPE_REFINE_MOVED, 'CONVERGED': L.MPE_REFINE_CONVERGED,
                    'FEW_VIEWS': L.MPE_REFINE_FEW_VIEWS, 'BAD_START': L.MPE_REFINE_BAD_START}
    M = RF()
    assert (M.SOLVED, M.MOVED, M.CONVERGED, M.FEW_VIEWS, M.BAD_START, M.MAX_ITERS) == (1, 2, 4, 8, 16, L.MPE_REFINE_MAX_ITERS)
    assert int(re.search(r'#define MPE_REFINE_MAX_ITERS (\d+)', hdr).group(1)) == L.MPE_REFINE_MAX_ITERS


@pytest.mark.parametrize('name', rc.RIGS)
def test_rig_cases_take_their_branches(name):
    """the 23-camera case (cameras in lanes that own no joint, a person in two of them, one in a single camera, an odd row
    capacity) and the camera-subset case (two views, slots 0 and 1 = calibration indices 4 and 5) are what they are for"""
    info = rc.check(rc.Case(name))
    print(name, info)
    assert info['V'] == {'ring23': 23, 'arprobot': 2}[name]
