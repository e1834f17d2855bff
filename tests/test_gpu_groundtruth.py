"""GPU: the ground-truth bodies of the frame JSON parsed on the device (mpe_json_parse_bodies_device), the GT arrays of the
metrics scripts (mpe_gt_from_bodies) and the harness's --device-gt, held bit for bit to harness/groundtruth.py -- which
tests/test_groundtruth_host.py holds to torch and to pack_bodies."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, env, harness_model_files, pkg
from test_groundtruth_host import fixture, transforms

pytestmark = pytest.mark.gpu

_eng = {}


def G():
    return pkg('harness.groundtruth')


def engine():
    if 'e' not in _eng:
        e = env()
        _eng['e'] = pkg('pipeline').Engine(e.params, e.calib, max_frames=48, max_persons_per_camera=4)
    return _eng['e']


def same_bodies(pb, want, frames=None):
    """ParsedBodies == parse_bodies' arrays (all rows, all slots), for `frames` of `want` (default: all)."""
    got = pb.numpy()
    sel = np.arange(len(want['n'])) if frames is None else np.asarray(frames)
    assert pb.n_frames == len(sel)
    assert np.array_equal(got['xyz'].view(np.uint64), want['xyz'][sel].view(np.uint64)), 'xyz'
    for k in ('mask', 'nkeys', 'order', 'm1', 'n', 'body_cam'):
        assert np.array_equal(got[k], want[k][sel]), k
    feo = want['frame_entry_off']
    ec = np.concatenate([want['entry_count'][feo[f]:feo[f + 1]] for f in sel] + [np.zeros(0, np.int32)])
    cam = np.concatenate([want['entry_cam'][feo[f]:feo[f + 1]] for f in sel] + [np.zeros(0, np.int32)])
    assert np.array_equal(got['entry_count'], ec) and np.array_equal(got['entries'][:, 1], cam)
    assert np.array_equal(np.diff(got['frame_entry_off']), np.array([feo[f + 1] - feo[f] for f in sel]))


def test_parse_bit_equal_on_the_fixture():
    text, frames = fixture()
    eng, par = engine(), pkg('parameters').parameters
    want = G().parse_bodies(frames, par.used_cameras, scap=40)
    assert len(frames) == 48 and int(want['n'].max()) >= 6
    pb = eng.bodies_from_json(text, max_frames=48, scap=40)
    assert pb.status == 0 and pb.n_entries == len(want['entry_count']) == sum(len(f) for f in frames)
    same_bodies(pb, want)


HAND = '''[
 {"camA": ["[]", 0.5, "no_image", [ ]],
  "camX": ["[]", 0.5, "no_image", [{"-1": [1, 2, 3], "0": [-0.0, 12, 1e-05]}, {}]],
  "camB": ["[]", 0.5, "no_image", [
     {"17": [-3.25E+1, 0.1, 123456.78901234567], "3": [1.5, -2.5e2, 7], "0": [0, 0.0, -0.0]},
     { "2" : [ 1.0 ,
               2.0 , 3.0 ] ,  "-1" : [ 4 , 5 , 6 ] }
  ]]},
 {"camB": ["[]", 1, "no_image", [{"30": [9.007199254740993e15, 2.5e-20, 1.7976931348623157e30], "-1": [0.3, 0.7, 1e22]}]],
  "camA": ["[]", 1, "no_image", [{}]]},
 {"camA": ["[]", 2, "no_image", []], "camB": ["[]", 2, "no_image", []], "camX": ["[]", 2, "no_image", []]}
]'''


def test_parse_of_a_hand_written_document():
    """Empty lists and bodies, a body without '-1', '-1' first, keys in descending order, signed zeros, integers, exponents
    of both signs and cases, 17-digit values, an integer above 2^53, blanks and line breaks between tokens:
    the numbers are Python's float() of the text."""
    frames = json.loads(HAND)
    eng, g = engine(), G()
    want = g.parse_bodies(frames, ['camA', 'camB'], scap=5)
    pb = eng.bodies_from_json(HAND.encode(), max_frames=8, scap=5, cameras=['camA', 'camB'])
    assert pb.status == 0 and pb.n_frames == 3
    same_bodies(pb, want)
    got = pb.numpy()
    assert list(got['n']) == [2, 2, 0] and list(got['entry_count']) == [0, 2, 2, 1, 1, 0, 0, 0]
    # frame 0: camB's two bodies first, camX's (not configured) behind them
    assert list(got['body_cam'][0]) == [1, 1, -1, -1, -1] and list(got['nkeys'][0]) == [3, 2, 2, 0, 0]
    assert list(got['order'][0, 0, :3]) == [17, 3, 0] and list(got['order'][0, 2, :2]) == [31, 0]
    assert list(got['m1'][0]) == [0, 1, 1, 0, 0]
    assert got['xyz'][0, 0, 17].tolist() == [float('-3.25E+1'), float('0.1'), float('123456.78901234567')]
    assert got['xyz'][0, 0, 3].tolist() == [1.5, -250.0, 7.0]
    z = got['xyz'][0, 2, 0]
    assert z.tolist() == [0.0, 12.0, float('1e-05')] and np.signbit(z[0]) and np.signbit(got['xyz'][0, 0, 0, 2])
    assert got['xyz'][1, 0, 30].tolist() == [float('9.007199254740993e15'), float('2.5e-20'), float('1.7976931348623157e30')]
    assert int(got['mask'][1, 0]) == (1 << 30) | (1 << 31) and int(got['mask'][1, 1]) == 0


def test_windows_give_the_same_rows():
    text, frames = fixture()
    eng, par = engine(), pkg('parameters').parameters
    want = G().parse_bodies(frames, par.used_cameras, scap=32)
    index = pkg('packing').JsonIndex(text)
    try:
        for size in (1, 7, 48):
            for start in range(0, 48, size) if size > 1 else (0, 13, 47):
                pb = eng.bodies_from_json(index, start, 1, size, scap=32)
                assert pb.status == 0
                same_bodies(pb, want, range(start, min(48, start + size)))
        pb = eng.bodies_from_json(index, 5, 12, 48, scap=32)
        assert pb.status == 0
        same_bodies(pb, want, [5, 17, 29, 41])
    finally:
        index.close()


DECLINES = {
    'twenty digits': '{"0": [1.2345678901234567891, 2, 3], "-1": [1, 2, 3]}',
    'key 40': '{"0": [1, 2, 3], "40": [1, 2, 3], "-1": [1, 2, 3]}',
    'two numbers': '{"0": [1, 2, 3], "25": [1, 2], "-1": [1, 2, 3]}',
    'null': '{"0": [1, 2, 3], "25": null, "-1": [1, 2, 3]}',
    'duplicate key': '{"0": [1, 2, 3], "0": [4, 5, 6], "-1": [1, 2, 3]}',
}
MORE_DECLINES = {
    'NaN': '{"0": [NaN, 2, 3]}', 'Infinity': '{"0": [1, -Infinity, 3]}', 'nesting': '{"0": [1, 2, 3], "1": {"2": [1, 2, 3]}}',
    'four numbers': '{"0": [1, 2, 3, 4]}', 'leading zero in a key': '{"07": [1, 2, 3]}', 'key -2': '{"-2": [1, 2, 3]}',
    'key 31': '{"31": [1, 2, 3]}', 'text key': '{"ID": [1, 2, 3]}', 'string value': '{"0": "abc"}', 'plus sign': '{"0": [+1, 2, 3]}',
    'nested list': '{"0": [[1], 2, 3]}', 'subnormal': '{"0": [1e-320, 2, 3]}', 'a list in the list': '[{"0": [1, 2, 3]}]',
    'missing comma': '{"0": [1, 2, 3] "1": [1, 2, 3]}',
}


@pytest.mark.parametrize('name', list(DECLINES) + list(MORE_DECLINES))
def test_declines_set_bit_0_and_nothing_else(name):
    body = {**DECLINES, **MORE_DECLINES}[name]
    doc = '[{"camA": ["[]", 0, "x", [{"1": [1, 2, 3], "-1": [0, 0, 0]}, %s, {"2": [1, 2, 3]}]], "camB": ["[]", 0, "x", [{"-1": [7, 8, 9]}]]}]' % body
    eng = engine()
    assert eng.bodies_from_json(doc.encode(), max_frames=4, scap=8, cameras=['camA', 'camB']).status == 1
    ok = doc.replace(body, '{"5": [1, 2, 3]}')
    assert eng.bodies_from_json(ok.encode(), max_frames=4, scap=8, cameras=['camA', 'camB']).status == 0


def test_capacity_sets_bit_1():
    text, frames = fixture()
    eng, par = engine(), pkg('parameters').parameters
    most = max(sum(len(f[c][3]) for c in f) for f in frames)
    assert eng.bodies_from_json(text, max_frames=48, scap=most).status == 0
    assert eng.bodies_from_json(text, max_frames=48, scap=most - 1).status == 2
    one = '[{"camA": ["[]", 0, "x", [%s]]}]' % ', '.join(['{"-1": [1, 2, 3]}'] * 5)
    assert eng.bodies_from_json(one.encode(), max_frames=2, scap=4, cameras=['camA']).status == 2
    assert eng.bodies_from_json(one.encode(), max_frames=2, scap=5, cameras=['camA']).status == 0


def rigid(seed):
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.standard_normal(3) * 2
    return T.astype(np.float32)


def same_gt(got, want):
    assert np.array_equal(got['xyz'].cpu().numpy().view(np.uint32), want['xyz'].view(np.uint32)), 'xyz'
    for k in ('joint', 'valid', 'n'):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_gt_bit_equal_on_the_fixture_two_files_in_one_batch():
    """The fixture's own transforms for the even frames, another dataset transform for the odd ones: one batch, two files.
    No ulp allowance."""
    text, frames = fixture()
    eng, g, par = engine(), G(), pkg('parameters').parameters
    T_d1, T_i1 = (t.numpy() for t in transforms())
    Ts, fof = [T_d1, rigid(3)], np.arange(48) % 2
    pb = eng.bodies_from_json(text, max_frames=48, scap=32)
    assert pb.status == 0
    want = g.gt_from_bodies(g.parse_bodies(frames, par.used_cameras, scap=32), Ts, fof, T_i1, eng.J)
    same_gt(eng.ground_truth(pb, Ts, fof, T_i1), want)
    assert int(want['joint'].sum()) * 3 > 5000
    # and against torch itself, one file: pack_ground_truth
    import torch as th
    ref = pkg('harness.common').pack_ground_truth(frames, [th.from_numpy(T_d1)] * 48, th.from_numpy(T_i1))
    got = eng.ground_truth(pb, [T_d1], np.zeros(48, np.int32), T_i1)
    gc = ref['xyz'].shape[1]
    assert np.array_equal(got['xyz'].cpu().numpy()[:, :gc].view(np.uint32), ref['xyz'].view(np.uint32))
    assert np.array_equal(got['n'].cpu().numpy(), ref['n']) and not got['joint'].cpu().numpy()[:, gc:].any()


def test_gt_selects_the_camera_per_frame():
    body = lambda x, m1=True: dict([(str(j), [x + j, -x, 100.0 * j]) for j in (0, 5, 17)] + ([('-1', [x, x, x])] if m1 else []))
    cam = lambda bodies: ['[]', 0, 'x', bodies]
    frames = [{'a': cam([body(1.0)]), 'b': cam([body(2.0), body(3.0, False)]), 'zz': cam([])},
              {'a': cam([body(4.0), body(5.0)]), 'zz': cam([body(6.0)]), 'b': cam([body(7.0), body(8.0)])},
              {'zz': cam([body(9.0)]), 'a': cam([]), 'b': cam([]), 'yy': cam([body(10.0), body(11.0), body(12.0)])},
              {'b': cam([body(13.0)]), 'yy': cam([body(14.0), body(15.0)]), 'a': cam([body(16.0), body(17.0)])},
              {'a': cam([]), 'b': cam([])}]
    eng, g = engine(), G()
    Ts, fof, T_i1 = [rigid(1), rigid(2)], [0, 1, 1, 0, 1], rigid(7)
    parsed = g.parse_bodies(frames, ['a', 'b'], scap=6)
    want = g.gt_from_bodies(parsed, Ts, fof, T_i1, eng.J)
    assert list(want['n']) == [2, 2, 3, 2, 0] and list(want['valid'][0, :2]) == [1, 0]
    pb = eng.bodies_from_json(json.dumps(frames).encode(), max_frames=8, scap=6, cameras=['a', 'b'])
    assert pb.status == 0
    same_bodies(pb, parsed)
    same_gt(eng.ground_truth(pb, Ts, fof, T_i1), want)
    # frame 3: 'yy' (not configured, rows behind the configured ones) is the first camera with two bodies
    x = want['xyz'][3, :2, 0]
    assert np.array_equal(x[0], g.to_world([14.0, -14.0, 0.0], Ts[0], T_i1)) and np.array_equal(x[1], g.to_world([15.0, -15.0, 0.0], Ts[0], T_i1))


def test_group_bodies_on_device_parsed_bodies():
    text, frames = fixture()
    eng, P = engine(), pkg('harness.partition')
    pb = eng.bodies_from_json(text, max_frames=48, scap=32)
    assert pb.status == 0
    got = eng.group_bodies(pb.packed())
    want = eng.group_bodies(P.pack_bodies(frames))
    torch.cuda.synchronize()
    w = want['labels'].shape[1]
    assert np.array_equal(got['labels'].cpu().numpy()[:, :w], want['labels'].cpu().numpy())
    assert (got['labels'].cpu().numpy()[:, w:] == -1).all()
    for k in ('n_groups', 'skip', 'count', 'status'):
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k


@pytest.fixture(scope='module')
def pinned(tmp_path_factory):
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'harness_expected.json')) as fh:
        exp = json.load(fh)
    mdir = harness_model_files(str(tmp_path_factory.mktemp('models')), exp['inputs'])
    return hd, exp, mdir


def flatten(out):
    flat = {}
    for k, v in out.items():
        if k in ('gt_windows', 'gt_declined'):
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                flat[(k, kk)] = vv
        else:
            flat[k] = v
    return flat


@pytest.mark.parametrize('script', ['metrics_from_model', 'metrics_from_triangulation', 'sm_metrics'])
def test_harness_device_gt_prints_what_device_metrics_prints(script, pinned):
    hd, exp, mdir = pinned
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.' + script)
    argv = ['--testfiles', os.path.join(hd, exp['inputs']['testfile']), '--tmdir', hd, '--modelsdir', mdir,
            '--datastep', str(exp['inputs']['datastep']), '--batch', '7']
    base = m.main(argv + ['--device-metrics'])
    out = m.main(argv + ['--device-gt'])
    assert out['gt_windows'] >= 1 and out['gt_declined'] == 0         # status == 0 on every window: no frame left to the host
    a, b = flatten(base), flatten(out)
    assert a.keys() == b.keys() and a['n_data'] == b['n_data'] > 0
    for k in a:
        assert b[k] == pytest.approx(a[k], rel=1e-12, abs=1e-12), k


def test_harness_device_gt_over_two_files_keeps_the_datastep_counter(pinned, tmp_path):
    """Two files with different frame counts and --datastep 5: the stride runs across the files, a batch spans both."""
    hd, exp, mdir = pinned
    _, frames = fixture()
    name = exp['inputs']['testfile']
    a, b = tmp_path / name, tmp_path / name.replace('.json', '_b.json')
    a.write_text(json.dumps(frames[:13]))
    b.write_text(json.dumps(frames[13:40]))
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.metrics_from_triangulation')
    argv = ['--testfiles', str(a), str(b), '--tmdir', hd, '--modelsdir', mdir, '--datastep', '5', '--batch', '6']
    base, out = flatten(m.main(argv + ['--device-metrics'])), m.main(argv + ['--device-gt'])
    assert out['gt_declined'] == 0 and out['gt_windows'] >= 3
    for k, v in flatten(out).items():
        assert v == pytest.approx(base[k], rel=1e-12, abs=1e-12), k


@pytest.mark.parametrize('name', list(DECLINES))
def test_harness_redoes_a_declined_window_on_the_host(name, pinned, tmp_path):
    """One declined body in an otherwise valid file (in a key the host's ground truth does not read, or a value that
    json.load resolves): the window is redone on the host and the report equals the host path's."""
    hd, exp, mdir = pinned
    _, frames = fixture()
    text = json.dumps(frames[:24])
    cam = list(frames[0])[0]
    first = json.dumps(frames[0][cam][3][0])
    edited = {'twenty digits': first.replace('{', '{"25": [1.2345678901234567891, 2, 3], ', 1),
              'key 40': first.replace('{', '{"40": [1, 2, 3], ', 1),
              'two numbers': first.replace('{', '{"25": [1, 2], ', 1),
              'null': first.replace('{', '{"25": null, ', 1),
              'duplicate key': first.replace('{', '{"25": [1, 2, 3], "25": [4, 5, 6], ', 1)}[name]
    assert text.count(first) >= 1
    path = tmp_path / exp['inputs']['testfile']
    path.write_text(text.replace(first, edited, 1))
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.metrics_from_triangulation')
    argv = ['--testfiles', str(path), '--tmdir', hd, '--modelsdir', mdir, '--datastep', '6', '--batch', '2']
    base, out = flatten(m.main(argv + ['--device-metrics'])), m.main(argv + ['--device-gt'])
    assert out['gt_declined'] == 1 and out['gt_windows'] == 2
    for k, v in flatten(out).items():
        assert v == base[k] or v == pytest.approx(base[k], rel=1e-12, abs=1e-12), k
