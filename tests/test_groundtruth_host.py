"""Ground truth from the frame JSON without a GPU: the host staging of the bodies (mpe_json_stage_gt_window) and
harness/groundtruth.py, the numpy statement of the device parse and of mpe_gt_from_bodies, against what they restate:
harness.partition.pack_bodies and harness.common.pack_ground_truth (torch on the CPU)."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, pkg

FIXTURE = os.path.join(GOLDEN, 'harness', 'syn_pinning_test.json')
_cache = {}


def G():
    return pkg('harness.groundtruth')


def fixture():
    if 'frames' not in _cache:
        with open(FIXTURE, 'rb') as fh:
            _cache['bytes'] = fh.read()
        _cache['frames'] = json.loads(_cache['bytes'])
    return _cache['bytes'], _cache['frames']


def transforms():
    """The fixture's own transforms, as harness.common.run takes them."""
    if 'T' not in _cache:
        import torch
        common, par = pkg('harness.common'), pkg('parameters').parameters
        calib = pkg('calibration').Calibration(par)
        T_d1 = torch.from_numpy(common.dataset_transform(os.path.join(GOLDEN, 'harness'), FIXTURE).get_transform('root', par.camera_names[1])).type(torch.float32)
        _cache['T'] = (T_d1, torch.from_numpy(calib.T_i32[1]))
    return _cache['T']


def stage(text, cameras, frame_start=0, frame_step=1, max_frames=4096):
    """mpe_json_stage_gt_window on a document -> (rc, entries [(frame, cam, begin, end)], frame_entry_off, staged text)."""
    L = pkg('lib')
    lib = L.load()
    ix = C.c_void_p()
    assert lib.mpe_json_index_create(text, len(text), C.byref(ix)) == 0
    try:
        ecap, tcap = max_frames * 16, len(text) + 16 * max_frames * 16 + 256
        buf = C.create_string_buffer(tcap)
        entries = (C.c_int32 * (4 * ecap))()
        feo = (C.c_int32 * (max_frames + 1))()
        names = (C.c_char_p * len(cameras))(*[c.encode() for c in cameras])
        nf, ne, tb = C.c_int32(), C.c_int32(), C.c_size_t()
        rc = lib.mpe_json_stage_gt_window(ix, names, len(cameras), frame_start, frame_step, max_frames, 1, C.cast(buf, C.c_void_p), tcap,
                                          C.cast(entries, C.c_void_p), ecap, C.cast(feo, C.c_void_p), C.byref(nf), C.byref(ne), C.byref(tb))
        if rc != 0:
            return rc, None, None, None
        e = np.frombuffer(entries, np.uint32)[:4 * ne.value].reshape(-1, 4).copy()
        return rc, [(int(a), int(np.int32(b)), int(c), int(d)) for a, b, c, d in e], list(feo[:nf.value + 1]), buf.raw[:tb.value]
    finally:
        lib.mpe_json_index_free(ix)


def test_staging_extents_are_the_body_lists_in_key_order():
    text, frames = fixture()
    par = pkg('parameters').parameters
    cams = list(par.used_cameras)[:-1]                    # the last configured camera left out: it must come back as -1
    rc, entries, feo, staged = stage(text, cams)
    assert rc == 0 and len(feo) == len(frames) + 1
    for f, frame in enumerate(frames):
        mine = entries[feo[f]:feo[f + 1]]
        assert len(mine) == len(frame)
        for (fr, cam, b, e), key in zip(mine, frame):     # entry order == frame key order
            assert fr == f and b % 16 == 0
            assert cam == (cams.index(key) if key in cams else -1)
            assert json.loads(staged[b:e]) == frame[key][3]
    assert any(c == -1 for _, c, _, _ in entries)
    # a window with a stride: the same extents' contents
    rc, e2, feo2, st2 = stage(text, cams, 5, 12, 3)
    assert rc == 0 and len(feo2) == 4
    for i, f in enumerate((5, 17, 29)):
        assert [json.loads(st2[b:e]) for _, _, b, e in e2[feo2[i]:feo2[i + 1]]] == [frames[f][k][3] for k in frames[f]]


@pytest.mark.parametrize('entry', ['["[]", 1.0, "no_image"]', '["[]", 1.0, "no_image", [], 5]', '["[]", 1.0, "no_image", {"0": [1, 2, 3]}]',
                                   '["[]", 1.0, "no_image", 7]', '[]', '{"a": 1}'])
def test_staging_declines_entries_without_a_body_list(entry):
    L = pkg('lib')
    doc = ('[{"cam_a": ["[]", 1.0, "no_image", [{"0": [1, 2, 3]}]], "cam_b": %s}]' % entry).encode()
    assert stage(doc, ['cam_a', 'cam_b'])[0] == L.MPE_ERR_UNSUPPORTED
    ok = b'[{"cam_a": ["[]", 1.0, "no_image", [{"0": [1, 2, 3]}]], "cam_b": ["[{}]", 2, "x", [ ]]}]'
    rc, entries, feo, staged = stage(ok, ['cam_b'])
    assert rc == 0 and [c for _, c, _, _ in entries] == [-1, 0]
    assert [json.loads(staged[b:e]) for _, _, b, e in entries] == [[{'0': [1, 2, 3]}], []]


def remap(packed, f, s):
    """A row of pack_bodies in the fixed slots."""
    g = G()
    slots = [g.slot_of(k) for k in packed['keys']]
    xyz = np.zeros((g.KEY_SLOTS, 3))
    mask = 0
    for k, slot in enumerate(slots):
        if (int(packed['mask'][f, s]) >> k) & 1:
            xyz[slot] = packed['xyz'][f, s, k]
            mask |= 1 << slot
    order = [slots[k] for k in packed['order'][f, s, :packed['nkeys'][f, s]]]
    return xyz, mask, order


def test_statement_equals_pack_bodies_in_fixed_slots():
    _, frames = fixture()
    g, P = G(), pkg('harness.partition')
    par = pkg('parameters').parameters
    packed = P.pack_bodies(frames)
    mine = g.parse_bodies(frames, par.used_cameras)
    assert mine['status'] == 0
    assert np.array_equal(mine['n'], packed['n'])
    checked = 0
    for f in range(len(frames)):
        for s in range(int(packed['n'][f])):
            xyz, mask, order = remap(packed, f, s)
            assert np.array_equal(mine['xyz'][f, s].view(np.uint64), xyz.view(np.uint64))
            assert int(mine['mask'][f, s]) == mask
            assert int(mine['nkeys'][f, s]) == int(packed['nkeys'][f, s]) == len(order)
            assert list(mine['order'][f, s, :len(order)]) == order
            assert int(mine['m1'][f, s]) == int(packed['m1'][f, s])
            checked += 1
    assert checked == int(packed['n'].sum()) > 100
    with pytest.raises(g.Unsupported):
        g.slot_of('40')
    for bad in ('07', '-2', '31', 'ID', '-0', ''):
        with pytest.raises(g.Unsupported):
            g.slot_of(bad)
    assert g.slot_of('-1') == 31 and g.slot_of('0') == 0 and g.slot_of('30') == 30


def test_grouping_does_not_depend_on_the_slot_numbering():
    _, frames = fixture()
    g, P = G(), pkg('harness.partition')
    par = pkg('parameters').parameters
    packed = P.pack_bodies(frames)
    mine = g.parse_bodies(frames, par.used_cameras)
    for f in range(len(frames)):
        a = P.group_bodies(packed['n'][f], packed['xyz'][f], packed['mask'][f], packed['nkeys'][f], packed['order'][f], packed['m1'][f])
        b = P.group_bodies(mine['n'][f], mine['xyz'][f], mine['mask'][f], mine['nkeys'][f], mine['order'][f], mine['m1'][f])
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_statement_is_bit_equal_to_torch_on_the_fixture():
    """Pins the fma chain of harness/groundtruth.py (and of csrc/gt.hip) to what torch's fp32 matmul gives on this host."""
    _, frames = fixture()
    g, common = G(), pkg('harness.common')
    par = pkg('parameters').parameters
    T_d1, T_i1 = transforms()
    assert len(frames) == 48
    want = common.pack_ground_truth(frames, [T_d1] * len(frames), T_i1)
    J = len(par.joint_list)
    got = g.gt_from_bodies(g.parse_bodies(frames, par.used_cameras), [T_d1.numpy()], np.zeros(len(frames), np.int32), T_i1.numpy(), J,
                           gcap=want['xyz'].shape[1])
    assert int(want['joint'].sum()) * 3 > 5000
    for k in ('n', 'valid', 'joint'):
        assert np.array_equal(got[k], want[k]), k
    diff = got['xyz'].view(np.uint32) != want['xyz'].view(np.uint32)
    assert not diff.any(), '%d of %d values differ from torch' % (int(diff.sum()), diff.size)


def test_statement_within_the_derived_bound_of_float64():
    """Two chained four-term fp32 dot products: |w - w64| <= 8 * 2^-24 * (|T_i| |T_d| |x|) componentwise.  Each product row is
    one rounded product and three rounded fma, so a term carries at most four roundings: (1 + u)^4 - 1 per product, 8 u for
    the chain to first order.  The rounding of g = v / 100 to fp32 adds at most u on three of the four terms and the second-
    order terms ~28 u^2; both fit because no term carries all four roundings of both products (the k-th term of a row
    carries 5 - k of them, the first two terms 4), which leaves more than 1 u of slack on the terms g enters."""
    _, frames = fixture()
    g = G()
    par = pkg('parameters').parameters
    T_d1, T_i1 = (t.numpy() for t in transforms())
    parsed = g.parse_bodies(frames, par.used_cameras)
    rng = np.random.RandomState(5)
    pts = [(f, s, j) for f in range(len(frames)) for s in range(int(parsed['n'][f])) for j in range(len(par.joint_list))
           if (int(parsed['mask'][f, s]) >> j) & 1]
    for i in rng.choice(len(pts), 300, replace=False):
        f, s, j = pts[i]
        v = parsed['xyz'][f, s, j]
        w = g.to_world(v, T_d1, T_i1).astype(np.float64)
        x = np.array([v[0] / 100., v[1] / 100., v[2] / 100., 1.0])
        Td, Ti = T_d1.astype(np.float64), T_i1.astype(np.float64)
        exact = (Ti @ (Td @ x))[:3]
        bound = 8 * 2.0 ** -24 * (np.abs(Ti) @ (np.abs(Td) @ np.abs(x)))[:3]
        assert np.all(np.abs(w - exact) <= bound), (f, s, j, w, exact, bound)


def test_fma32_is_correctly_rounded():
    g = G()
    rng = np.random.RandomState(9)
    for _ in range(2000):
        a, b, c = (np.float32(x) for x in rng.standard_normal(3) * 10.0 ** rng.randint(-3, 4, 3))
        got = g.fma32(a, b, c)
        fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        assert abs(Fraction(float(got)) - fr) <= min(abs(Fraction(float(lo)) - fr), abs(Fraction(float(hi)) - fr))
    # a tie of the double rounding: 1 + 2^-24 + 2^-60 must round up, which rounding to float64 first gets wrong
    assert g._round32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert g._round32(Fraction(1) + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 60)) == np.float32(1.0)


def test_camera_selection():
    g = G()
    assert g.select_entry([2, 3, 3]) == 1
    assert g.select_entry([3, 3]) == 0
    assert g.select_entry([0, 0, 0]) is None and g.select_entry([]) is None
    body = lambda x: {'0': [x, 0.0, 0.0], '-1': [x, 1, 1]}
    frame = {'a': ['[]', 0, 'x', [body(1.0)]], 'zz': ['[]', 0, 'x', [body(2.0), body(3.0), body(4.0)]], 'b': ['[]', 0, 'x', [body(5.0), body(6.0)]]}
    parsed = g.parse_bodies([frame, {'a': ['[]', 0, 'x', []], 'b': ['[]', 0, 'x', []]}], ['a', 'b'])
    assert list(parsed['entry_cam']) == [0, -1, 1, 0, 1] and list(parsed['n']) == [3, 0]
    # rows: the configured cameras' bodies first (1, 5, 6), the other camera's behind them (2, 3, 4)
    assert list(parsed['xyz'][0, :, 0, 0]) == [1.0, 5.0, 6.0, 2.0, 3.0, 4.0]
    assert list(parsed['body_cam'][0]) == [0, 1, 1, -1, -1, -1]
    eye = np.eye(4, dtype=np.float32)
    gt = g.gt_from_bodies(parsed, [eye], [0, 0], eye, 2)
    assert list(gt['n']) == [3, 0]                        # the camera outside the configured list holds the most bodies
    assert np.array_equal(gt['xyz'][0, :3, 0, 0], np.array([2.0, 3.0, 4.0]) / np.float32(100.)) or \
        np.array_equal(gt['xyz'][0, :3, 0, 0], (np.array([2.0, 3.0, 4.0]) / 100.).astype(np.float32))
    assert list(gt['joint'][0, 0]) == [1, 0] and list(gt['valid'][0, :3]) == [1, 1, 1]
    # the host's ground_truth() picks the same bodies
    import torch
    want = pkg('harness.common').pack_ground_truth([frame], [torch.eye(4)], torch.eye(4))
    assert int(want['n'][0]) == 3 and np.array_equal(want['xyz'][0, :, :2], gt['xyz'][0, :3])
