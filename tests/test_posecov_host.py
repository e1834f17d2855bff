"""CPU: harness/uncertainty.py, the numpy statement of mpe_posecov_batch -- that its inverse is the inverse, that the
covariance it reports is calibrated on the synthetic scenes (the Mahalanobis distance of the refined joints from the truth
has the mean of a chi-square with three degrees of freedom), the pooled pixel sigma, what is exact -- csrc/cov3.h on the
host under the sanitizers, and the declarations."""
import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT, env, oracle, pkg

NOISE_PX = {'5x10': 1.0, 'messy': 2.0}
_cases, _refined = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = rc.Case(name)
    return _cases[name]


def U():
    return pkg('harness.uncertainty')


def run(c, kind, poses=None, **kw):
    start, flags, mask = rc.kinds(c)[kind]
    return U().pose_covariance(c.calib, c.pb, c.persons, c.n_persons, start if poses is None else poses, flags, mask, **kw)


def refined(name, kind):
    """The case refined to the minimum (64 iterations, step_tol 1e-9, plain least squares), once."""
    if (name, kind) not in _refined:
        c = case(name)
        poses, flags, mask = rc.kinds(c)[kind]
        _refined[name, kind] = pkg('harness.refine').refine(c.calib, c.pb, c.persons, c.n_persons, poses, flags, mask, max_iters=64,
                                                            step_tol=1e-9, huber_px=0.0)
    return _refined[name, kind]


def mahalanobis(U_, cov, err):
    """d2 = e^T Sigma^-1 e of every row"""
    return np.einsum('ni,ni->n', err, np.linalg.solve(U_.full(cov), err[..., None])[..., 0])


@pytest.mark.parametrize('kind', ['est', 'triang'])
@pytest.mark.parametrize('name', rc.NAMES)
def test_statement_against_linear_algebra(name, kind):
    """1: on every COMPUTED joint cov is sigma_px^2 * inv(A) to 16 * eps * cond(A), relative to the largest entry."""
    M = U()
    c = case(name)
    out = run(c, kind, sigma_px=1.5, diagnostics=True)
    done = (out['status'] & M.COMPUTED) != 0
    assert out['cov'].shape == out['status'].shape + (6,) and out['sigma'].dtype == np.float64 and out['status'].dtype == np.uint8
    assert np.all(out['sigma'][~done] == -1.0) and not out['cov'][~done].any() and np.all(out['sigma'][done] > 0)
    if name == 'zero frames':
        assert out['status'].size == 0
        return
    assert done.sum() > 0 and np.all(out['n_views'][done] >= 2)
    A = M.full(out['A'][done])
    ref = (1.5 * 1.5) * np.linalg.inv(A)
    got = M.full(out['cov'][done])
    rel = np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    bound = 16 * np.finfo(np.float64).eps * np.linalg.cond(A)
    print(name, kind, 'computed', int(done.sum()), 'worst rel / (eps cond)', (rel / (bound / 16)).max(), 'largest cond', np.linalg.cond(A).max())
    assert np.all(rel <= bound)


@pytest.mark.parametrize('kind', ['est', 'triang'])
@pytest.mark.parametrize('name', ['5x10', 'messy'])
def test_calibration(name, kind):
    """2: refined to the minimum, with sigma_px the noise that was put in, the mean Mahalanobis distance from the truth over
    all SOLVED and COMPUTED joints is 3 to five standard errors, 5 * sqrt(6 / n) (chi-square(3) has variance 6).
    Measured: 5x10 est 3.087 (n 1105), triang 3.107 (1359); messy est 3.041 (623), triang 3.116 (767)."""
    M = U()
    c = case(name)
    ref = refined(name, kind)
    out = run(c, kind, poses=ref['poses'], sigma_px=NOISE_PX[name])
    use = ((ref['status'] & 1) != 0) & ((out['status'] & M.COMPUTED) != 0)
    assert np.array_equal(use, (ref['status'] & 1) != 0)                  # what the refinement solved has a covariance
    err = (ref['poses'].astype(np.float64) - c.truth)[use]
    d2 = mahalanobis(M, out['cov'][use], err)
    n = d2.size
    sig = out['sigma'][use]
    print(name, kind, 'n', n, 'mean d2 %.4f' % d2.mean(), 'bound %.4f' % (5 * np.sqrt(6 / n)), 'median sigma %.3f mm' % (1000 * np.median(sig)),
          'corr(sigma, |err|) %.3f' % np.corrcoef(sig, np.linalg.norm(err, axis=1))[0, 1])
    assert abs(d2.mean() - 3.0) <= 5 * np.sqrt(6 / n)


@pytest.mark.parametrize('kind', ['est', 'triang'])
@pytest.mark.parametrize('name', ['5x10', 'messy'])
def test_pooled_pixel_sigma(name, kind):
    """3: pixel_sigma of the refinement's own outputs against the noise put in, within five standard errors of a pooled
    standard deviation, 5 / sqrt(2 * dof).  Asserted on messy.  5x10 misses it and is recorded only: 1.0608 px
    (est) and 1.0604 px (triang) of 1 put in, bounds 0.0420 and 0.0379.  The cause is not the noise but the model: synthetic.
    make_frame projects with the tangential lens terms, which the camera model of the geometry stages leaves out (0.28 px rms
    per coordinate on these bodies, up to 2.8 px), and dividing by 2n - 3 scales that bias up; next to 2 px it is within the
    bound.  test_pooled_pixel_sigma_own_model has the 5x10 case with detections of the stages' own model: 1.0067."""
    ps, dof = U().pixel_sigma([refined(name, kind)])
    rel, bound = abs(ps / NOISE_PX[name] - 1.0), 5 / np.sqrt(2 * dof)
    print(name, kind, 'pooled pixel sigma %.4f px of %g put in, dof %d, relative distance %.4f, bound %.4f' % (ps, NOISE_PX[name], dof, rel, bound))
    if name == 'messy':
        assert rel <= bound


def test_pooled_pixel_sigma_own_model():
    """3: the 5x10 batch with detections that are the stages' own projection of the bodies plus 1 px of seeded normal noise:
    the pooled pixel sigma is 1 within the bound, and so is the calibration of item 2."""
    M, c = U(), case('5x10')
    pb = rc.noise_free(c)
    pb.xy = pb.xy + np.random.default_rng(5).normal(0.0, 1.0, pb.xy.shape)
    poses, flags, mask = rc.kinds(c)['est']
    ref = pkg('harness.refine').refine(c.calib, pb, c.persons, c.n_persons, poses, flags, mask, max_iters=64, step_tol=1e-9)
    ps, dof = M.pixel_sigma([ref])
    print('own model: pooled pixel sigma %.4f px, dof %d, bound %.4f' % (ps, dof, 5 / np.sqrt(2 * dof)))
    assert abs(ps - 1.0) <= 5 / np.sqrt(2 * dof)
    out = M.pose_covariance(c.calib, pb, c.persons, c.n_persons, ref['poses'], flags, mask, 1.0)
    use = (ref['status'] & 1) != 0
    d2 = mahalanobis(M, out['cov'][use], (ref['poses'].astype(np.float64) - c.truth)[use])
    print('own model: mean d2 %.4f, n %d' % (d2.mean(), d2.size))
    assert abs(d2.mean() - 3.0) <= 5 * np.sqrt(6 / d2.size)


def test_pixel_sigma_and_summary_of_nothing():
    M = U()
    ps, dof = M.pixel_sigma([])
    assert np.isnan(ps) and dof == 0
    r = M.summary([])
    assert r['computed'] == 0 and r['gated'] == 0 and np.isnan(r['median_mm'])
    out = run(case('one frame'), 'triang', sigma_px=1.0, gate_m=1e-4)
    r = M.summary([out, out])
    done = (out['status'] & M.COMPUTED) != 0
    assert r['computed'] == 2 * done.sum() and r['gated'] == 2 * ((out['status'] & M.GATED) != 0).sum() > 0
    assert r['median_mm'] == 1000.0 * np.median(out['sigma'][done]) and r['max_mm'] == 1000.0 * out['sigma'][done].max()
    assert 'Uncertainty (sigma 1 px)' in M.report_line(1.0, 0.1, r, 1.02)


@pytest.mark.parametrize('kind', ['est', 'triang'])
def test_doubling_sigma_px_is_exactly_four_times(kind):
    """4: cov scales by exactly 4 and sigma by exactly 2, bit for bit, and nothing else changes."""
    for name in ('messy', 'hand made'):
        c = case(name)
        one, two = run(c, kind, sigma_px=1.25), run(c, kind, sigma_px=2.5)
        assert rc.same_bits(two['cov'], 4.0 * one['cov']) and one['cov'].any()
        assert rc.same_bits(two['sigma'], np.where(one['sigma'] > 0, 2.0 * one['sigma'], one['sigma']))
        assert np.array_equal(one['status'], two['status']) and np.array_equal(one['n_views'], two['n_views'])


def test_hiding_a_camera_never_lowers_sigma():
    """4: one person of the one-frame case loses a camera: every joint COMPUTED before and after has at least the sigma
    (relative 1e-12 for rounding), and some have more."""
    M, onp = U(), oracle()
    base = rc.Case('one frame')
    every = np.repeat((np.arange(base.pcap)[None, :] < base.n_persons[:, None])[..., None], rc.J, axis=2).astype(np.uint8)
    mask = (1 << rc.J) - 1
    full = M.pose_covariance(base.calib, base.pb, base.persons, base.n_persons, base.truth, every, mask, sigma_px=1.0)
    cams = list(base.calib.params.camera_names)
    grew = 0
    for person, hidden in ((0, 0), (1, 2), (2, len(cams) - 1), (3, 1)):
        c = rc.Case('one frame')
        frame, owner = copy.deepcopy(c.frames[0]), copy.deepcopy(c.owners[0])
        rc.only_seen_by(frame, owner, person, [k for i, k in enumerate(cams) if i != hidden])
        pb = pkg('packing').pack_frames([onp.processed_input(frame)], c.calib.params, keep_json=True)
        persons, n_persons = rc.persons_from_owners(pb, [owner], [int(c.n_persons[0])], c.pcap)
        assert (persons[0, person, hidden] == -1) and (base.persons[0, person, hidden] >= 0)
        less = M.pose_covariance(c.calib, pb, persons, n_persons, base.truth, every, mask, sigma_px=1.0)
        assert np.array_equal(less['n_views'][0, person], full['n_views'][0, person] - rc_selected(base, person, hidden, every, mask))
        both = ((full['status'] & M.COMPUTED) != 0) & ((less['status'] & M.COMPUTED) != 0)
        assert both[0, person].sum() >= 10
        assert np.all(less['sigma'][both] >= full['sigma'][both] * (1 - 1e-12))
        others = [p for p in range(c.pcap) if p != person]
        assert rc.same_bits(less['cov'][0, others], full['cov'][0, others])
        grew += int((less['sigma'][both] > full['sigma'][both] * (1 + 1e-9)).sum())
    assert grew >= 40


def rc_selected(c, person, cam, flags, mask):
    """[J]: camera `cam` observes the joint of `person` in frame 0"""
    sel, _ = pkg('harness.reprojection').selection(c.pb, c.persons, c.n_persons, flags, mask)
    return sel[0, person, cam].astype(np.uint8)


def test_hand_made_statuses():
    """4: the joint started behind camera 2 is BAD_POSE, the person one camera sees FEW_VIEWS, and the person two cameras see
    is less certain than the frame's median."""
    M = U()
    c = case('hand made')
    for kind in ('est', 'triang'):
        out = run(c, kind, sigma_px=1.0)
        st = out['status']
        assert st[0, 2, 8] == M.BAD_POSE and out['sigma'][0, 2, 8] == -1.0 and not out['cov'][0, 2, 8].any() and out['n_views'][0, 2, 8] >= 2
        assert (st == M.BAD_POSE).sum() == 1
        done = (st & M.COMPUTED) != 0
        two = done & (out['n_views'] == 2)
        median = np.median(out['sigma'][done])
        print(kind, 'computed', int(done.sum()), 'two views', int(two.sum()), 'median sigma %.3f mm' % (1000 * median),
              'two-view sigma %.3f .. %.3f mm' % (1000 * out['sigma'][two].min(), 1000 * out['sigma'][two].max()))
        assert two[0, 1].sum() >= 10 and np.all(out['sigma'][two] > median)
        if kind == 'est':
            picked = out['n_views'][0, 0] > 0
            assert picked.sum() >= 10 and np.all(st[0, 0][picked] == M.FEW_VIEWS) and np.all(out['n_views'][0, 0][picked] == 1)
            assert np.all(out['sigma'][0, 0] == -1.0)
        assert not (st & M.SINGULAR).any() and not (st & M.GATED).any()


def test_gate_and_flags_out():
    """the gate marks the COMPUTED joints above it and clears exactly their flags; a joint that is not COMPUTED keeps its flag"""
    M = U()
    c = case('hand made')
    poses, flags, mask = rc.kinds(c)['triang']
    plain = run(c, 'triang', sigma_px=1.0)
    done = (plain['status'] & M.COMPUTED) != 0
    gate = float(np.median(plain['sigma'][done]))
    out = run(c, 'triang', sigma_px=1.0, gate_m=gate, flags_out=True)
    gated = (out['status'] & M.GATED) != 0
    assert np.array_equal(gated, done & (plain['sigma'] > gate)) and 0 < gated.sum() < done.sum()
    assert np.array_equal(out['status'] & ~np.uint8(M.GATED), plain['status']) and rc.same_bits(out['cov'], plain['cov'])
    assert np.array_equal(out['flags'], np.where(gated, 0, flags)) and out['flags'].dtype == flags.dtype
    assert out['flags'][0, 2, 8] == flags[0, 2, 8] == 1                  # BAD_POSE: not judged
    with pytest.raises(ValueError):
        run(c, 'est', sigma_px=1.0, gate_m=gate, flags_out=True)
    for kw in ({'sigma_px': 0.0}, {'sigma_px': np.inf}, {'sigma_px': np.nan}, {'sigma_px': 1.0, 'gate_m': -1.0}, {'sigma_px': 1.0, 'gate_m': np.nan},
               {'sigma_px': 1.0, 'huber_px': -1.0}):
        with pytest.raises(ValueError):
            run(c, 'triang', **kw)


def test_huber_weight_widens():
    """a Huber threshold below the residuals takes weight from A: no joint gets more certain, and some get less"""
    M = U()
    c = case('messy')
    plain, hub = run(c, 'triang', sigma_px=2.0), run(c, 'triang', sigma_px=2.0, huber_px=1.0)
    both = ((plain['status'] & M.COMPUTED) != 0) & ((hub['status'] & M.COMPUTED) != 0)
    assert both.sum() > 100 and np.all(hub['sigma'][both] >= plain['sigma'][both] * (1 - 1e-12))
    assert (hub['sigma'][both] > plain['sigma'][both] * 1.01).any()


def test_header_on_the_host_under_sanitizers(tmp_path):
    """5: csrc/cov3.h in a stand-alone program (tests/native/cov3_test.cpp) built with -fsanitize=address,undefined: a table of
    systems from the statement's own normal matrices, the all-ones matrix (D1 = 0: SINGULAR), a NaN, zeros and infinities,
    every finite output bit for bit and what is not finite in the same places."""
    M = U()
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'cov3_test')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'cov3_test.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)
    c = case('messy')
    out = run(c, 'triang', sigma_px=1.0, diagnostics=True)
    real = out['A'][(out['status'] & M.COMPUTED) != 0][:300]
    rng = np.random.default_rng(3)
    B = rng.normal(size=(100, 3, 3)) * 10.0 ** rng.uniform(-3, 3, (100, 1, 1))
    G = B @ B.transpose(0, 2, 1)
    rand = np.stack([G[:, k, l] for k, l in M.ORDER], axis=1)
    nan = np.nan
    hard = np.array([[1, 1, 1, 1, 1, 1], [1, 0, nan, 1, 0, 1], [nan, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 0], [-1, 0, 0, 1, 0, 1],
                     [np.inf, 0, 0, 1, 0, 1], [1e-320, 0, 0, 1e-320, 0, 1e-320], [1, 2, 3, 4, 5, 6], [2, 1, 0, 2, 1, 2]], np.float64)
    table = np.concatenate([real, rand, hard])
    s2 = np.concatenate([np.ones(len(real)), rng.uniform(0.1, 9.0, len(rand)), np.full(len(hard), 2.25)])
    src, dst = str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')
    np.concatenate([[float(len(table))], np.concatenate([table, s2[:, None]], axis=1).reshape(-1)]).tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, np.float64).reshape(len(table), 15)
    S, pivots = M.inverse3({kl: table[:, q] for q, kl in enumerate(M.ORDER)})
    cov, sigma, finite = M.finish(S, s2)
    want = np.concatenate([np.stack([S[kl] for kl in M.ORDER], axis=1), pivots[:, None].astype(np.float64), cov, sigma[:, None],
                           finite[:, None].astype(np.float64)], axis=1)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    assert np.array_equal(got[fin].view(np.int64), want[fin].view(np.int64)), int((got[fin].view(np.int64) != want[fin].view(np.int64)).sum())
    n = len(real) + len(rand)
    assert len(real) == 300 and pivots[:n].all() and finite[:n].all()
    ones, with_nan = n, n + 1
    assert not pivots[ones] and not pivots[with_nan] and not finite[with_nan] and not pivots[n + 2:n + 6].any()
    assert pivots[-1] and finite[-1] and (~fin).sum() > 0
    # the statement's own cov of the real systems is this table's
    assert rc.same_bits(cov[:len(real)], out['cov'][(out['status'] & M.COMPUTED) != 0][:300])


def test_singular_systems_are_not_computed():
    """a person seen by the same pixels twice over has a rank-2 A; whatever rounding leaves of the last pivot, the joint is
    either SINGULAR with nothing reported or COMPUTED with a finite covariance -- never a non-finite output"""
    M = U()
    for name in rc.NAMES:
        for kind in ('est', 'triang'):
            out = run(case(name), kind, sigma_px=1.0)
            assert np.isfinite(out['cov']).all() and np.isfinite(out['sigma']).all()
            done = (out['status'] & M.COMPUTED) != 0
            assert not (out['status'][~done] & M.GATED).any()
            assert np.all(np.isin(out['status'], (0, M.COMPUTED, M.FEW_VIEWS, M.BAD_POSE, M.SINGULAR)))


def test_symbol_in_header_and_binding():
    """6"""
    L, M = pkg('lib'), U()
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    assert re.search(r'\bint mpe_posecov_batch\(mpe_ctx \*ctx, void \*stream, const mpe_batch \*b, const mpe_posecov_args \*a\);', hdr)
    assert 'mpe_posecov_batch' in L.SYMBOLS and not any(n.startswith('mpe_refine_') and 'cov' in n for n in L.SYMBOLS)
    names = [n for n, _ in L.mpe_posecov_args._fields_]
    body = re.sub(r'/\*.*?\*/', '', hdr[:hdr.index('} mpe_posecov_args;')].rsplit('typedef struct {', 1)[1], flags=re.S)
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|pose_f64|joint_flags|joint_mask|threshold|huber_px|sigma_px|gate_m)\b', body) == names
    refine = [n for n, _ in L.mpe_refine_args._fields_]
    upto = [n for n in refine[:refine.index('huber_px') + 1] if n not in ('max_iters', 'step_tol')]
    assert names[:len(upto)] == upto and names[len(upto):len(upto) + 2] == ['sigma_px', 'gate_m']
    bits = {n: int(v) for n, v in re.findall(r'MPE_POSECOV_(\w+) = (\d+)', hdr)}
    assert bits == {'COMPUTED': 1, 'FEW_VIEWS': 8, 'BAD_POSE': 16, 'SINGULAR': 32, 'GATED': 64}
    assert bits == {'COMPUTED': L.MPE_POSECOV_COMPUTED, 'FEW_VIEWS': L.MPE_POSECOV_FEW_VIEWS, 'BAD_POSE': L.MPE_POSECOV_BAD_POSE,
                    'SINGULAR': L.MPE_POSECOV_SINGULAR, 'GATED': L.MPE_POSECOV_GATED}
    assert (M.COMPUTED, M.FEW_VIEWS, M.BAD_POSE, M.SINGULAR, M.GATED) == (1, 8, 16, 32, 64)


def test_struct_layout(tmp_path):
    """the ctypes struct has the size and the offsets a C compiler gives the header's"""
    L = pkg('lib')
    gcc = shutil.which('gcc') or shutil.which('cc')
    assert gcc, 'no host C compiler'
    st = L.mpe_posecov_args
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "mpe.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(mpe_posecov_args));']
    lines += ['printf("%s %%zu\\n", offsetof(mpe_posecov_args, %s));' % (f, f) for f, _ in st._fields_]
    lines.append('return 0; }')
    (tmp_path / 'layout.c').write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'layout')
    subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', exe], check=True,
                   capture_output=True, timeout=120)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(got['size']) == __import__('ctypes').sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_flags_parse():
    a = pkg('harness.common').build_parser('x').parse_args([])
    assert (a.uncertainty, a.uncertainty_gate) == (0.0, 0.0)
    a = pkg('harness.common').build_parser('x').parse_args(['--uncertainty', '2', '--uncertainty-gate', '9.5'])
    assert (a.uncertainty, a.uncertainty_gate) == (2.0, 9.5)
