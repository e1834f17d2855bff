"""The yardstick and the checkers of the non-finite-input tests on their own, on the CPU (nonfinite_cases.py): the poisons hit what
they say and nothing else, the structural checker rejects bad person tables, the oracle really is disturbed by every poison kind
(and only in the poisoned frame), the magnitude of the large-but-finite poison is the one its recipe gives, and a 1e39 in a
document reaches the packed batch as a finite double."""
import json

import numpy as np
import pytest

import nonfinite_cases as nc
from conftest import oracle, pkg


@pytest.fixture(scope='module')
def s3(calib):
    return nc.batch(calib, 'S3')


def _person_head(frames, f, calib, gat_weights):
    """A head of frame f that the oracle puts into a person."""
    sd, prm = gat_weights
    res = oracle().run_frame(frames[f], calib, sd, prm, None, mode='tri')
    person = [(-1 if x is None else int(x)) for x in res['persons'][0]]
    return person, [x for x in person if x >= 0][0]


def test_batches_have_the_shapes_the_tests_rely_on(calib):
    a, p, c, s = (nc.batch(calib, n)['pb'] for n in ('A18', 'P18', 'C17', 'S3'))
    heads = [a.frame_counts(f)[1] for f in range(a.n_frames)]
    assert {5, 10, 15, 20} <= set(heads) and 18 in heads and 13 in heads               # 1 .. 4 persons, persons missing from cameras
    assert any(a.frame_counts(f)[1] > 0 and a.frame_counts(f)[3] == 0 for f in range(a.n_frames))      # heads, no graph
    assert any(bin(int(m)).count('1') < a.J for m in a.joint_mask)                                     # dropped joints
    for other in (a, c, s):
        assert p.n_heads + p.n_edge_nodes >= other.n_heads + other.n_edge_nodes and p.n_heads >= other.n_heads
    assert nc.node_ranges(a) != nc.node_ranges(c)[:a.n_frames] and nc.node_ranges(c)[1] != nc.node_ranges(p)[1]
    for name, (first, mid) in nc.POSITIONS.items():
        pb = nc.batch(calib, name)['pb']
        assert first == 0 and nc.shares_tiles_with_both_neighbours(pb, mid), (name, mid)
        for f in (first, mid):
            assert pb.frame_counts(f)[3] > 0
    assert nc.batch(calib, 'T17')['pb'].max_heads_per_frame() == 50


@pytest.mark.parametrize('kind', nc.KINDS)
def test_poison_hits_a_present_joint_and_nothing_else(s3, kind):
    pb = s3['pb']
    before = {n: getattr(pb, n).tobytes() for n in nc.ARRAY_NAMES}
    out = nc.poison(pb, 1, kind)
    assert {n: getattr(pb, n).tobytes() for n in nc.ARRAY_NAMES} == before                 # the input is left alone
    info = out.poisoned
    h = int(pb.frame_head_off[1]) + info['head']
    assert int(pb.frame_head_off[1]) <= h < int(pb.frame_head_off[2])
    for n in nc.ARRAY_NAMES[:8]:
        assert getattr(out, n).tobytes() == before[n], n
    present = bool(int(pb.joint_mask[h]) >> info['joint'] & 1)
    if kind == 'masked_nan':
        assert not present and len(info['writes']) == 3
    else:
        assert present and int(pb.tri_mask[h]) >> info['joint'] & 1 and len(info['writes']) == 1
    touched = {'xy': set(), 'vp': set()}
    for name, comp, value in info['writes']:
        got = getattr(out, name)[h, info['joint'], comp]
        assert (np.isnan(got) and np.isnan(value)) or got == getattr(out, name).dtype.type(value)
        touched[name].add((h, info['joint'], comp))
    for name in ('xy', 'vp'):
        a, b = getattr(pb, name), getattr(out, name)
        diff = {tuple(int(x) for x in i) for i in np.argwhere(a.view(a.dtype.str.replace('f', 'u')) != b.view(b.dtype.str.replace('f', 'u')))}
        assert diff == touched[name], (name, diff)
    if kind == 'xy_f32_overflow':
        v = out.xy[h, info['joint'], 0]
        with np.errstate(over='ignore'):
            assert np.isfinite(v) and np.isinf(np.float32(v))
    if kind == 'xy_3e38':
        assert np.isfinite(np.float32(out.xy[h, info['joint'], 0]))


def test_poison_takes_the_head_it_is_given(s3):
    out = nc.poison(s3['pb'], 2, 'xy_inf', head=7)
    assert out.poisoned['head'] == 7 and out.poisoned['frame'] == 2
    many = nc.poison_more(s3['pb'], (0, 1, 2), 'xy_nan')
    assert [m['frame'] for m in many.poisoned_all] == [0, 1, 2] and int(np.isnan(many.xy).sum()) == 3


def test_structural_checker_rejects_bad_tables(s3):
    pb = s3['pb']
    V, pcap = pb.V, 10
    h0, H, _, _ = pb.frame_counts(1)
    first_of_cam = [next(lh for lh in range(H) if pb.head_cam[h0 + lh] == c) for c in range(V)]
    good = np.full((3, pcap, V), -1, np.int32)
    good[1, 0] = first_of_cam
    good[1, 1, 0] = first_of_cam[0] + 1
    n = np.array([0, 2, 0], np.int32)
    assert int(pb.head_cam[h0 + first_of_cam[0] + 1]) == 0
    assert nc.structurally_valid(good, n, pb, 1, pcap) and nc.structurally_valid(good, n, pb, 0, pcap)
    for what, edit in (('out of range', lambda t, m: t.__setitem__((1, 1, 2), H)), ('below -1', lambda t, m: t.__setitem__((1, 1, 2), -2)),
                       ('a head of another camera', lambda t, m: t.__setitem__((1, 1, 1), first_of_cam[0] + 1)),
                       ('a duplicate head', lambda t, m: t.__setitem__((1, 1, 0), first_of_cam[0])),
                       ('n > pcap', lambda t, m: m.__setitem__(1, pcap + 1)), ('n < 0', lambda t, m: m.__setitem__(1, -1))):
        t, m = good.copy(), n.copy()
        edit(t, m)
        assert not nc.structurally_valid(t, m, pb, 1, pcap), what
        assert nc.structural_fault(t, m, pb, 1, pcap)
        assert nc.structurally_valid(t, m, pb, 2, pcap), what                                # the other frames are not judged by it


@pytest.mark.parametrize('kind', nc.KINDS)
def test_the_oracle_is_disturbed_in_the_poisoned_frame_only(s3, calib, gat_weights, kind):
    """The oracle is per frame, so the clean frames of a poisoned batch score as they did; the poisoned frame's scores are non-finite
    or different (a kind for which neither held would poison nothing); masked_nan never reaches the oracle at all."""
    pb, frames = s3['pb'], s3['frames']
    _, lh = _person_head(frames, 1, calib, gat_weights)
    out = nc.poison(pb, 1, kind, head=lh)
    seen = list(frames)
    seen[1] = nc.poisoned_frame(frames, out, calib)
    clean = [nc.oracle_scores(f, calib, gat_weights) for f in frames]
    got = [nc.oracle_scores(f, calib, gat_weights) for f in seen]
    for f in (0, 2):
        assert got[f][0] == clean[f][0] and np.array_equal(got[f][1].view(np.int32), clean[f][1].view(np.int32))
    assert np.isfinite(clean[1][1]).all()
    if kind == 'masked_nan':
        assert seen[1] == frames[1] and np.array_equal(got[1][1], clean[1][1])
    elif kind == 'large_finite':
        assert np.isfinite(got[1][1]).all() and not np.array_equal(got[1][1], clean[1][1])
    else:
        assert not np.isfinite(got[1][1]).all() or not np.array_equal(got[1][1], clean[1][1])
    # the JSON twin holds the very values of the packed batch
    repacked = pkg('packing').pack_frames(seen, calib.params)
    for n in nc.ARRAY_NAMES:
        if kind != 'masked_nan':
            assert getattr(repacked, n).tobytes() == getattr(out, n).tobytes(), n


def test_large_finite_is_the_magnitude_of_its_recipe(calib, gat_weights):
    """Test D's condition: with x at LARGE_FINITE_M the oracle's fp32 and f64 forwards of every frame Test D poisons are entirely
    finite, and M is the largest power of ten for which that holds on all of them (10^38 is the largest that is a float)."""
    powers = []
    for name, f in nc.LARGE_FINITE_FRAMES:
        b = nc.batch(calib, name)
        env_gat = gat_weights
        powers.append(nc.find_large_finite_power(b['frames'], b['pb'], f, calib, env_gat))
        out = nc.poison(b['pb'], f, 'large_finite')
        fr = nc.poisoned_frame(b['frames'], out, calib)
        assert np.isfinite(nc.oracle_scores(fr, calib, env_gat)[1]).all() and np.isfinite(nc.oracle_scores(fr, calib, env_gat, f64=True)[1]).all()
    assert 10.0 ** min(powers) == nc.LARGE_FINITE_M, powers
    with np.errstate(over='ignore'):
        assert np.isfinite(np.float32(nc.LARGE_FINITE_M)) and np.isinf(np.float32(10 * nc.LARGE_FINITE_M))


def test_the_oracles_row_test_on_poisoned_rows(s3, calib, gat_weights):
    """sum(|row|) > 1 on the reference's row: NaN anywhere in the row says no, an infinity alone says yes, and 1e39 -- a finite
    double that the row's f64 arithmetic scales down before the cast -- leaves a finite row."""
    frames, pb = s3['frames'], s3['pb']
    person, lh = _person_head(frames, 1, calib, gat_weights)
    want = {'xy_nan': False, 'prob_nan': False, 'xy_f32_overflow': True, 'masked_nan': True, 'large_finite': True}
    for kind, kept_want in want.items():
        fr = nc.poisoned_frame(frames, nc.poison(pb, 1, kind, head=lh), calib)
        row, kept = nc.oracle_person_row(fr, person, calib)
        assert kept == kept_want, kind
        if kind in ('xy_f32_overflow', 'masked_nan', 'large_finite'):
            assert np.isfinite(row).all(), kind
    assert bool(np.sum(np.abs(np.array([np.inf, 1.0], np.float32))) > 1) and not bool(np.sum(np.abs(np.array([np.inf, np.nan], np.float32))) > 1)


def test_the_host_packer_takes_1e39_as_a_finite_double(s3, calib):
    """1e39 is a legal JSON number: the native host packer (strtod) keeps it as the double it is."""
    pb = s3['pb']
    out = nc.poison(pb, 1, 'xy_f32_overflow')
    raw = [dict(f) for f in s3['frames']]
    raw[1] = nc.poisoned_frame(s3['frames'], out, calib)
    text = json.dumps(raw)
    assert '1e+39' in text
    got = pkg('packing').pack_json(text, calib.params)
    h = int(pb.frame_head_off[1]) + out.poisoned['head']
    assert got.xy[h, out.poisoned['joint'], 0] == float('1e39')
    for n in nc.ARRAY_NAMES:
        assert getattr(got, n).tobytes() == getattr(out, n).tobytes(), n
