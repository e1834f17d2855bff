"""harness/partition.py, the numpy statement of the clustering-quality kernels (csrc/partition.hip), against what it restates:
sklearn's adjusted_rand_score / homogeneity_completeness_v_measure, the label loop of harness/sm_metrics.py and its
gt_labels().  No GPU."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg


def P():
    return pkg('harness.partition')


def label_pairs():
    """>= 4000 seeded pairs: n from 1 to 230, 1 to 12 classes per side, plus the special shapes."""
    rng = np.random.RandomState(20240607)
    out = []
    for i in range(4000):
        n = 1 + (i % 230) if i < 460 else int(rng.randint(1, 231))
        kt, kp = int(rng.randint(1, 13)), int(rng.randint(1, 13))
        out.append((rng.randint(0, kt, n), rng.randint(0, kp, n)))
    for n in (1, 2, 3, 7, 64, 65, 230):
        a = rng.randint(0, 5, n)
        out.append((a, a.copy()))                                  # identical
        out.append((a, (a + 3) % 5))                               # identical up to names
        out.append((np.zeros(n, int), rng.randint(0, 4, n)))       # one class on the true side
        out.append((rng.randint(0, 4, n), np.full(n, 7)))          # one class on the predicted side
        out.append((np.zeros(n, int), np.zeros(n, int)))
        out.append((np.arange(n), np.arange(n)))                   # all singletons
        out.append((np.arange(n), np.zeros(n, int)))
        out.append((rng.randint(0, 3, n), np.arange(n)[::-1].copy()))
    return out


def test_partition_scores_against_sklearn():
    """ARI equal (one division of exact integers on both sides); homogeneity, completeness and V-measure within 1e-12
    absolute, the bound tests/test_gpu_harness.py puts on these numbers (sklearn sums pairwise and takes some of its
    logarithms from libm, the statement sums from the left and reads one table)."""
    from sklearn.metrics import adjusted_rand_score, homogeneity_completeness_v_measure
    p = P()
    pairs = label_pairs()
    assert len(pairs) >= 4000
    worst = 0.0
    for lt, lp in pairs:
        got = p.partition_scores(lt, lp)
        assert all(isinstance(x, float) for x in got)
        assert got[0] == adjusted_rand_score(lt, lp), (lt, lp)
        want = homogeneity_completeness_v_measure(lt, lp)
        d = max(abs(g - w) for g, w in zip(got[1:], want))
        worst = max(worst, d)
        assert d <= 1e-12, (lt, lp, got, want)
    print('largest difference to sklearn in h / c / v: %.3g' % worst)
    assert p.partition_scores([], []) == (1.0, 1.0, 1.0, 1.0)
    assert p.partition_scores([5], [9]) == (1.0, 1.0, 1.0, 1.0)


def test_partition_scores_ignore_label_names_and_read_one_table():
    p = P()
    rng = np.random.RandomState(3)
    lt, lp = rng.randint(0, 6, 150), rng.randint(0, 9, 150)
    ref = p.partition_scores(lt, lp)
    # order-preserving renaming: the summation order, hence every bit, is kept
    assert p.partition_scores(lt * 10 + 3, lp * 7 - 100) == ref
    lg = p.log_table()
    assert lg.dtype == np.float64 and len(lg) >= 65536 and lg[0] == 0.0
    head = lg[:65536].copy()
    big = p.log_table(230 * 230 * 4)
    assert len(big) >= 230 * 230 * 4 and np.array_equal(big[:65536], head)      # grown at the end only


def test_batch_scores_marks_the_frames_that_are_not_scored():
    p = P()
    lt = np.array([[0, 0, 1, 1], [0, 1, 2, 3], [0, 0, 0, 0]], np.int32)
    lp = np.array([[0, 1, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1]], np.int32)
    out = p.batch_scores(lt, lp, count=[4, 0, 3], skip=[0, 0, 0], count_true=[4, 0, 4])
    assert out.shape == (3, 4) and out.dtype == np.float64
    assert tuple(out[0]) == p.partition_scores(lt[0], lp[0])
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all()
    assert np.isnan(p.batch_scores(lt, lp, count=[4, 4, 4], skip=[1, 0, 0])[0]).all()


def loop_labels(proposals, H):
    """harness/sm_metrics.py evaluate(), the label loop, verbatim."""
    est = []
    for h in range(H):
        idx = len(proposals)
        for p, members in enumerate(proposals):
            if h in members:
                idx = p
                break
        est.append(idx)
    return est


def test_proposal_labels_against_the_loop():
    p = P()
    rng = np.random.RandomState(11)
    for case in range(300):
        V, H = int(rng.randint(1, 7)), int(rng.randint(0, 40))
        pcap = int(rng.randint(1, 12))
        n = int(rng.randint(0, pcap + 1))
        rows = np.full((pcap, V), -1, np.int32)
        heads = rng.permutation(max(H, 1))
        k = 0
        for q in range(pcap):
            for c in range(V):
                if rng.rand() < 0.5 and H:
                    # mostly disjoint proposals, sometimes a head that an earlier proposal holds already
                    rows[q, c] = heads[k % H] if rng.rand() < 0.9 else heads[int(rng.randint(0, H))]
                    k += 1
        proposals = [[int(h) for h in rows[q] if h >= 0] for q in range(n)]
        got = p.proposal_labels(rows, n, H)
        assert got.dtype == np.int32 and got.tolist() == loop_labels(proposals, H), case
        assert p.proposal_labels([set(m) for m in proposals], n, H).tolist() == loop_labels(proposals, H)


def _golden_frames():
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'harness_expected.json')) as fh:
        exp = json.load(fh)
    with open(os.path.join(hd, exp['inputs']['testfile'])) as fh:
        return json.load(fh)


def _synthetic_frames():
    """1 to 10 persons, noise-free and noisy bodies, and the special frames: a body without '-1', a body that shares no
    joint with any person, two persons closer than one unit, bodies in another key order, a frame without bodies."""
    syn = pkg('synthetic')
    calib = pkg('calibration').Calibration(pkg('parameters').parameters)
    rng = np.random.RandomState(5)
    frames = []
    for persons in range(1, 11):
        for noise in (0.0, 0.2, 0.8):
            f, _ = syn.make_frame(calib, 100 * persons + int(noise * 10), syn.FrameSpec(persons=persons, noise_px=0.0))
            f = copy.deepcopy(f)
            if noise:
                for cam in f:
                    for body in f[cam][3]:
                        for k in body:
                            body[k] = [float(v + rng.normal(0.0, noise)) for v in body[k]]
            frames.append(f)
    base = [copy.deepcopy(frames[9]), copy.deepcopy(frames[12]), copy.deepcopy(frames[16]), copy.deepcopy(frames[21]),
            copy.deepcopy(frames[6])]
    cams = list(base[0].keys())
    del base[0][cams[1]][3][0]['-1']                                           # a body without '-1'
    base[1][cams[0]][3][1] = {'40': [1.0, 2.0, 3.0], '41': [0.0, 0.0, 0.0]}    # shares no joint with anybody (and has no '-1')
    bodies = base[2][cams[0]][3]                                               # two persons 0.35 apart: they merge
    src = next(b for b in bodies if b)
    for cam in cams:
        base[2][cam][3].append({k: [v[0] + 0.2, v[1] - 0.2, v[2] + 0.2] for k, v in src.items()})
    for cam in cams[::2]:                                                       # the founder's key order decides the summation order
        base[3][cam][3] = [dict(reversed(list(b.items()))) for b in base[3][cam][3]]
    for cam in cams:
        base[4][cam][3] = []                                                    # no bodies at all
    few = copy.deepcopy(frames[13])                                             # bodies with few joints, integer coordinates
    for cam in cams:
        few[cam][3] = [{k: [int(round(x)) for x in v] for k, v in list(b.items())[:4 + i % 3]} for i, b in enumerate(few[cam][3])]
    return frames + base + [few]


def test_group_bodies_against_gt_labels():
    """Every frame of the committed harness input and the synthetic frames: the packed statement gives gt_labels()'s
    labels and its skip decision, packed alone and packed as one batch with other frames."""
    p = P()
    sm = pkg('harness.sm_metrics')
    frames = _golden_frames() + _synthetic_frames()
    n_valid = n_skip = n_merge = 0
    for start in range(0, len(frames), 7):
        chunk = frames[start:start + 7]
        pk = p.pack_bodies(chunk)
        assert pk['xyz'].dtype == np.float64 and pk['xyz'].shape[2] == len(pk['keys']) <= p.KEY_CAP
        for i, f in enumerate(chunk):
            want = sm.gt_labels(f)
            labels, n_groups, skip = p.group_bodies(pk['n'][i], pk['xyz'][i], pk['mask'][i], pk['nkeys'][i], pk['order'][i], pk['m1'][i])
            assert skip == (want is None), (start, i)
            one = p.pack_bodies([f])
            alone = p.group_bodies(one['n'][0], one['xyz'][0], one['mask'][0], one['nkeys'][0], one['order'][0], one['m1'][0])
            assert alone[0].tolist() == labels.tolist() and alone[1:] == (n_groups, skip)
            if want is None:
                n_skip += 1
                continue
            n_valid += 1
            assert labels.dtype == np.int32 and labels.tolist() == want, (start, i)
            assert n_groups == max(want) + 1
    assert n_valid >= 60 and n_skip >= 3
    # the merged pair: the added bodies joined an existing person, so no more persons than before
    syn = _synthetic_frames()
    before, after = sm.gt_labels(syn[16]), sm.gt_labels(syn[32])
    assert before is not None and after is not None and len(after) > len(before) and max(after) == max(before)


def test_pack_bodies_declines_what_it_cannot_hold():
    p = P()
    cam = pkg('parameters').parameters.used_cameras[0]
    with pytest.raises(ValueError):
        p.pack_bodies([{cam: ['[]', 0.0, 'no_image', [{str(k): [0.0, 0.0, 0.0] for k in range(p.KEY_CAP + 1)}]]}])
    with pytest.raises(ValueError):
        p.pack_bodies([{cam: ['[]', 0.0, 'no_image', [{'-1': [0.0, 0.0]}]]}])
    # a camera outside used_cameras is passed over, as gt_labels does
    pk = p.pack_bodies([{cam: ['[]', 0.0, 'no_image', [{'-1': [0, 0, 0]}]], 'no such camera': ['[]', 0.0, 'no_image', [{'-1': [1, 1, 1]}]]}])
    assert pk['n'].tolist() == [1]
