"""mpe_reproject_batch and mpe_residual_stats (csrc/reproject.hip) against their host statement
harness/reprojection.py, and harness/reprojection_error.py --device-metrics / --showgt end to end."""
import importlib
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, env, harness_model_files, oracle, pkg

pytestmark = pytest.mark.gpu
HD = os.path.join(GOLDEN, 'harness')
HARNESS = '3d_multi_pose_estimator_amd.harness.reprojection_error'


def same_bits(a, b):
    """Bit-equal, NaN matching NaN (numpy and the device need not agree on a NaN's payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def make_engine(frames, max_frames=64):
    import torch  # noqa: F401
    e = env()
    most = max([1] + [f[c][0].count('{') for f in frames for c in f])
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=max(max_frames, len(frames), 1), max_persons_per_camera=max(4, most))
    eng.load_gat(*e.gat)
    eng.load_mlp(e.mlp_room)
    return eng


def damaged(frames):
    """Cameras missing and detections that must not count: valid at 0.5, below it, just above it; a joint removed."""
    out = []
    for i, fr in enumerate(frames):
        fr = {c: list(v) for c, v in fr.items()}
        if i % 3 == 0:
            del fr[list(fr)[i % len(fr)]]
        for k, c in enumerate(fr):
            sks = json.loads(fr[c][0])
            for s, sk in enumerate(sks):
                keys = [q for q in sk if q != 'ID']
                for n, q in enumerate(keys):
                    if (n + s + k + i) % 4 == 0:
                        sk[q][3] = [0.5, 0.0, 0.25, 0.5000001, 0.75][(n + i) % 5]
                if keys and (s + i) % 2 == 0:
                    del sk[keys[(s + k) % len(keys)]]
            fr[c][0] = json.dumps(sks)
        out.append(fr)
    return out


def batches():
    onp, syn, calib = oracle(), pkg('synthetic'), env().calib
    fixture = json.load(open(os.path.join(HD, 'syn_pinning_test.json')))[::3]
    crowd = [syn.make_frame(calib, 900 + i, syn.FrameSpec(persons=10, noise_px=1.0))[0] for i in range(8)]
    messy = damaged([syn.make_frame(calib, 300 + i, syn.FrameSpec(persons=3 + i % 3, noise_px=2.0, joint_drop=0.1))[0] for i in range(12)])
    return {'harness fixture': [onp.processed_input(f) for f in fixture], '5x10': [onp.processed_input(f) for f in crowd],
            'cameras missing, valid <= 0.5': [onp.processed_input(f) for f in messy], 'zero frames': []}


def test_reproject_bit_equal_to_host_statement():
    """6: every entry of d_res, sentinels included, for MLP poses (person flag, used joints), binary64 triangulated poses
    (joint flags, all joints) and a one-joint mask, on the four batches the issue names.  The final binary64 root is
    compared bit for bit like everything else: no ulp allowance was needed."""
    import torch
    R = pkg('harness.reprojection')
    calib = env().calib
    used_mask = sum(1 << j for j in calib.params.used_joints)
    for name, frames in batches().items():
        eng = make_engine(frames)
        try:
            db = eng.to_device(eng.pack(frames))
            _, persons, n_persons = eng.match(db, want_scores=False)
            poses, valid = eng.mlp3d(db, persons, n_persons)
            tri, jv = eng.triangulate(db, persons, n_persons, all_joints=True, positive_ids_only=True)
            got = {'est': eng.reproject(db, persons, n_persons, poses, valid, 'est'),
                   'triang': eng.reproject(db, persons, n_persons, tri, jv, 'triang'),
                   'gt': eng.reproject(db, persons, n_persons, poses, valid, 'gt'),
                   'joint 3': eng.reproject(db, persons, n_persons, tri, jv, 'triang', joint_mask=1 << 3)}
            eng.sync_status()
            h = [t.cpu().numpy() for t in (persons, n_persons, poses, valid, tri, jv)]
            J = eng.J
            want = {'est': R.residuals(calib, db.host, h[0], h[1], h[2], h[3], used_mask),
                    'triang': R.residuals(calib, db.host, h[0], h[1], h[4], h[5], (1 << J) - 1),
                    'gt': R.residuals(calib, db.host, h[0], h[1], h[2], h[3], 1 << (J - 1)),
                    'joint 3': R.residuals(calib, db.host, h[0], h[1], h[4], h[5], 1 << 3)}
            for kind in got:
                g = got[kind].cpu().numpy()
                assert g.shape == (len(frames), eng.pcap, eng.V, J)
                n = int((g >= 0).sum())
                print(name, kind, 'entries', g.size, 'counted', n, 'differing', int((g != want[kind]).sum()) if g.size else 0)
                assert same_bits(g, want[kind]), (name, kind)
                if frames and kind in ('est', 'triang'):
                    assert n > 0, (name, kind)
                assert np.all(g[~(g >= 0) & ~np.isnan(g)] == R.SENTINEL)
            if frames:
                one = got['joint 3'].cpu().numpy()
                assert np.all(one[..., [j for j in range(J) if j != 3]] == R.SENTINEL)
        finally:
            eng.close()


@pytest.mark.parametrize('name', ['ring23', 'arprobot'])
def test_reproject_and_stats_on_rig_cases(name):
    """The rig cases of refine_cases (persons from the generator's pairing, no network): 23 cameras, of which 18..22 sit in
    lanes that own no joint, with an odd Pcap; and the camera-subset rig, whose slots 0 and 1 are calibration indices 4
    and 5.  Every entry of d_res for the four kinds of test_reproject_bit_equal_to_host_statement -- float32 poses with
    person flags ('est', and 'gt' with its one-joint mask), binary64 poses with joint flags, a one-joint mask -- and the
    per-camera statistics (V rows, every camera counted)."""
    import torch

    import refine_cases as rc
    R = pkg('harness.reprojection')
    case = rc.Case(name)
    info = rc.check(case)
    print(name, info)
    e = case.env
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=16, max_persons_per_camera=4, **rc.ENGINE.get(name, {}))
    try:
        case = rc.Case(name, pcap=eng.pcap)
        assert eng.V == info['V'] and eng.pcap == info.get('pcap', eng.pcap)
        db = eng.to_device(eng.pack(case.processed))
        persons, n_persons = torch.from_numpy(case.persons).cuda(), torch.from_numpy(case.n_persons).cuda()
        J = eng.J
        every = np.ones((len(case.frames), eng.pcap, J), np.uint8)
        used_mask = sum(1 << j for j in e.params.used_joints)
        runs = {'est': (case.est, case.est_flags, 'est', used_mask, None), 'triang': (case.truth, every, 'triang', (1 << J) - 1, None),
                'gt': (case.est, case.est_flags, 'gt', 1 << (J - 1), None),
                'joint 3': (case.truth, every, 'triang', 1 << 3, 1 << 3)}
        for what, (poses, flags, kind, mask, arg) in runs.items():
            g = eng.reproject(db, persons, n_persons, torch.from_numpy(poses).cuda(), torch.from_numpy(flags).cuda(), kind, joint_mask=arg)
            want = R.residuals(e.calib, db.host, case.persons, case.n_persons, poses, flags, mask)
            got = g.cpu().numpy()
            print(name, what, 'entries', got.size, 'counted', int((got >= 0).sum()), 'differing', int((got != want).sum()))
            assert got.shape == (len(case.frames), eng.pcap, eng.V, J) and same_bits(got, want), (name, what)
            assert (got >= 0).sum() > 0 and np.all(got[~(got >= 0)] == R.SENTINEL)
            if what == 'triang':
                st, ref = eng.residual_stats(g), R.stats([want.reshape(-1, eng.V, J)])
                assert len(st['count']) == eng.V and st['count'].tolist() == ref['count'].tolist() == info['count']
                assert same_bits(st['mid'], ref['mid']) and same_bits(st['median'], ref['median'])
                assert np.allclose(st['sum'], ref['sum'], rtol=1e-12, atol=0)
        eng.sync_status()
    finally:
        eng.close()


def stat_buffers(rng, V, J):
    """Residual-shaped buffers whose cameras hold the cases of the issue."""
    def buf(groups, fill):
        a = np.full((groups, V, J), -1.0)
        for c, f in enumerate(fill):
            flat = a[:, c, :].reshape(-1)
            vals = np.asarray(f(groups * J), np.float64)
            idx = rng.permutation(groups * J)[:len(vals)]
            flat[idx] = vals
            a[:, c, :] = flat.reshape(groups, J)
        return a
    wide = lambda n: np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-8, 9, n)
    a = buf(400, [lambda n: wide(2001), lambda n: wide(2000), lambda n: [], lambda n: [3.25], lambda n: [7.5, 1.25]])
    b = buf(300, [lambda n: rng.integers(0, 4, 1000) * 0.5,                                    # ties
                  lambda n: np.concatenate([wide(500), [np.inf, np.inf, 0.0, 5e-324]]),        # +inf on top, zero, a denormal
                  lambda n: np.concatenate([wide(301), [np.nan]]),                             # NaN in, NaN out
                  lambda n: wide(n),                                                           # every entry counted
                  lambda n: np.concatenate([np.full(10, 2.0), np.full(10, 3.0)])])             # even n, middle straddles a tie edge
    c = buf(5000, [lambda n, k=k: wide(n // 2 + k) for k in range(5)])
    # -0.0 is >= 0 and sorts with 0 (numpy), although its bit pattern lies above +inf's
    d = buf(200, [lambda n: np.concatenate([np.full(5, -0.0), wide(2000)]), lambda n: np.concatenate([np.full(3, -0.0), [0.0], wide(1000)]),
                  lambda n: [-0.0, 2.0, 4.0], lambda n: [4.0, -0.0], lambda n: np.concatenate([np.full(2, -0.0), [np.inf, 1.0, 2.0]])])
    return {'odd even 0 1 2': a, 'ties inf nan full': b, 'large': c, 'negative zero': d}


def check_stats(got, want, bufs):
    V = len(want['count'])
    assert got['count'].dtype == np.int64 and got['nonfinite'].dtype == np.int64
    assert got['count'].tolist() == want['count'].tolist()
    assert got['nonfinite'].tolist() == want['nonfinite'].tolist()
    for c in range(V):
        a = np.concatenate([b[:, c, :].reshape(-1) for b in bufs])
        keep = a[a >= 0]
        if len(keep):
            ref = np.median(a[~(a < 0)])                    # with the NaN entries, as numpy sees them
            print('camera', c, 'n', len(keep), 'median', got['median'][c], 'numpy', ref, 'sum', got['sum'][c])
            assert same_bits(got['median'][c], ref), (c, got['median'][c], ref)
            if not np.isnan(ref):
                assert same_bits(got['mid'][c], want['mid'][c])
        else:
            assert np.isnan(got['median'][c]) and np.isnan(got['mean'][c])
        if np.isnan(a).any():
            assert np.isnan(got['sum'][c]) and np.isnan(got['mean'][c]) and np.isnan(got['median'][c])
        elif np.isinf(keep).any():
            assert got['sum'][c] == np.inf
        else:
            exact = math.fsum(keep.tolist())
            # any summation order of n non-negative terms is within (n - 1) u of the exact sum, relatively (u = 2^-53)
            assert abs(got['sum'][c] - exact) <= max(len(keep) - 1, 0) * 2.0 ** -53 * exact, (c, got['sum'][c], exact)


def test_residual_stats_exact_median_and_fixed_order_sum():
    """7: counts equal, the median EQUAL to np.median (odd and even n, n = 0, 1, 2, ties, +inf, NaN in -> NaN out), the sum
    within (n-1) 2^-53 of math.fsum and bit-equal between two runs, several buffers at once == their concatenation."""
    import torch
    R = pkg('harness.reprojection')
    eng = make_engine([])
    try:
        V, J = eng.V, eng.J
        bufs = stat_buffers(np.random.default_rng(5), V, J)
        dev = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
        for name, a in bufs.items():
            got = eng.residual_stats(dev[name])
            check_stats(got, R.stats([a]), [a])
            again = eng.residual_stats(dev[name])
            assert same_bits(got['sum'], again['sum']) and same_bits(got['mid'], again['mid'])
        # several buffers at once, and the same entries as one concatenated buffer
        parts = list(bufs.values())
        many = eng.residual_stats([dev[k] for k in bufs])
        whole = np.concatenate(parts)
        one = eng.residual_stats(torch.from_numpy(whole).cuda())
        check_stats(many, R.stats(parts), parts)
        check_stats(one, R.stats([whole]), [whole])
        assert many['count'].tolist() == one['count'].tolist() and many['nonfinite'].tolist() == one['nonfinite'].tolist()
        assert same_bits(many['mid'], one['mid']) and same_bits(many['median'], one['median'])
        # a buffer split in two gives the statistics of the whole
        a = bufs['large']
        halves = eng.residual_stats([torch.from_numpy(a[:1234].copy()).cuda(), torch.from_numpy(a[1234:].copy()).cuda()])
        check_stats(halves, R.stats([a]), [a])
        # no buffers / an empty buffer: nothing counted
        for empty in ([], [torch.zeros((0, V, J), dtype=torch.float64, device='cuda')]):
            z = eng.residual_stats(empty)
            assert z['count'].tolist() == [0] * V and np.isnan(z['median']).all() and np.isnan(z['mean']).all()
    finally:
        eng.close()


def check_report(got, want):
    rows = {(kind, cam) for cam, kinds in want.items() for kind in kinds}
    assert set(got) == rows, sorted(set(got) ^ rows)
    for cam, kinds in want.items():
        for kind, (mean, median) in kinds.items():
            g = got[(kind, cam)]
            print(cam, kind, 'got', g, 'reference', (mean, median))
            assert g[1] == pytest.approx(median, rel=2e-4), (cam, kind, g, median)
            assert abs(np.log10(g[0]) - np.log10(mean)) < 0.5, (cam, kind, g, mean)


def test_cli_device_metrics_and_showgt_report(tmp_path):
    """8: the CLI prints the same report with and without --device-metrics, with and without --showgt, and the device
    reports meet what the reference script printed (harness_expected.json, reprojection_showgt_expected.json)."""
    R = pkg('harness.reprojection')
    m = importlib.import_module(HARNESS)
    base = json.load(open(os.path.join(HD, 'harness_expected.json')))
    exp = json.load(open(os.path.join(HD, 'reprojection_showgt_expected.json')))
    mdir = harness_model_files(str(tmp_path), base['inputs'])
    frames = json.load(open(os.path.join(HD, base['inputs']['testfile'])))
    assert R.add_joint2_from_minus1(frames) == exp['inputs']['bodies_changed']
    ddir = os.path.join(str(tmp_path), 'derived')
    os.makedirs(ddir)
    derived = os.path.join(ddir, base['inputs']['testfile'])
    json.dump(frames, open(derived, 'w'))
    common = ['--tmdir', HD, '--modelsdir', mdir, '--datastep', str(base['inputs']['datastep']), '--batch', '7']
    for testfile, flag, want in ((os.path.join(HD, base['inputs']['testfile']), [], base['reprojection_error']),
                                 (derived, ['--showgt'], exp['reprojection_error'])):
        host = m.main(['--testfiles', testfile] + common + flag)
        dev = m.main(['--testfiles', testfile] + common + flag + ['--device-metrics'])
        assert set(host) == set(dev)
        for key in host:
            print(key, 'host', host[key], 'device', dev[key])
            assert dev[key][2] == host[key][2], key
            assert dev[key][1] == pytest.approx(host[key][1], rel=2e-4), key
            assert abs(np.log10(dev[key][0]) - np.log10(host[key][0])) < 0.5, key
        check_report(dev, want)
        check_report(host, want)
    assert any(kind == 'GT' for kind, _ in dev)
    with pytest.raises(FileNotFoundError):
        m.main(['--testfiles', derived, '--tmdir', ddir, '--modelsdir', mdir, '--showgt', '--datastep', '3'])


def test_device_metrics_clean_synthetic_triangulation_below_a_pixel():
    """9: triangulated joints of correctly grouped, noise-free detections reproject onto the detections, now on the
    device path: the median of every camera is below 1 px."""
    m = importlib.import_module(HARNESS)
    argv = ['--synthetic', '16', '--random-weights', '--teacher-scores', '--batch', '16']
    dev = m.main(argv + ['--device-metrics'])
    tri = {cam: v for (kind, cam), v in dev.items() if kind == 'triang'}
    print(tri)
    assert len(tri) == 5 and max(t[1] for t in tri.values()) < 1.0
    assert any(kind == 'est' for kind, _ in dev)
    host = m.main(argv)
    assert set(host) == set(dev)
    for key in host:
        assert dev[key][2] == host[key][2] and dev[key][1] == pytest.approx(host[key][1], rel=2e-4), key
