"""GPU: the clustering-quality kernels (csrc/partition.hip: mpe_partition_labels, mpe_group_bodies, mpe_partition_scores)
against their numpy statement harness/partition.py, bit for bit, and the two sm_metrics harnesses with --device-metrics
against their host paths and against the numbers the reference's scripts printed."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, env, harness_model_files, pkg
from test_partition_host import _golden_frames, _synthetic_frames, label_pairs

pytestmark = pytest.mark.gpu

KEYS = ('rand score', 'homogeneity', 'completeness', 'v_measure')


def P():
    return pkg('harness.partition')


def _engine(variant='panoptic', max_frames=16, persons=11):
    e = env(variant)
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=max_frames, max_persons_per_camera=persons)
    eng.load_gat(*e.gat)
    return eng


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _score_batches(eng, pairs, width, B=250):
    """pairs padded to batches [B, width]; every seventh frame skipped, every eleventh with count 0."""
    p, L = P(), pkg('lib')
    n_frames = 0
    for start in range(0, len(pairs), B):
        chunk = pairs[start:start + B]
        lt = np.full((len(chunk), width), -1, np.int32)
        lp = np.full((len(chunk), width + 3), -1, np.int32)          # the two arrays need not have one row length
        count = np.zeros(len(chunk), np.int32)
        for i, (a, b) in enumerate(chunk):
            lt[i, :len(a)], lp[i, :len(b)], count[i] = a, b, len(a)
        count[10::11] = 0
        skip = np.zeros(len(chunk), np.uint8)
        skip[6::7] = 1
        scores, status = eng.partition_scores(_dev(lt, torch.int32), _dev(lp, torch.int32), _dev(count, torch.int32), skip=_dev(skip, torch.uint8))
        want = p.batch_scores(lt, lp, count, skip)
        got, status = scores.cpu().numpy(), status.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))[:5]
        assert np.array_equal(status != 0, np.isnan(want[:, 0])) and not (status & L.MPE_PART_OVER_CAP).any()
        n_frames += len(chunk)
    return n_frames


def test_partition_scores_bit_equal_on_random_partitions():
    """The random partitions of tests/test_partition_host.py, padded to batches: every score has the statement's bits, NaN
    rows included -- through the 256-thread kernel and, for the short ones, through the one-wave kernel."""
    eng = _engine()
    pairs = label_pairs()
    assert _score_batches(eng, pairs, 256) >= 4000
    short = [pr for pr in pairs if len(pr[0]) <= 61]
    assert _score_batches(eng, short, 61) >= 500
    eng.close()


def test_partition_scores_raise_the_status_bit_over_the_cap():
    p, L = P(), pkg('lib')
    eng = _engine()
    rng = np.random.RandomState(8)
    n = [300, 200, L.MPE_PART_MAX_SAMPLES, L.MPE_PART_MAX_SAMPLES + 1, 40]
    lt = rng.randint(0, 9, (5, 320)).astype(np.int32)
    lp = rng.randint(0, 7, (5, 320)).astype(np.int32)
    ct = np.array([300, 200, 256, 257, 41], np.int32)
    scores, status = eng.partition_scores(_dev(lt, torch.int32), _dev(lp, torch.int32), _dev(n, torch.int32), count_true=_dev(ct, torch.int32))
    scores, status = scores.cpu().numpy(), status.cpu().numpy()
    assert status.tolist() == [L.MPE_PART_OVER_CAP, 0, 0, L.MPE_PART_OVER_CAP, L.MPE_PART_SKIPPED]
    assert np.isnan(scores[[0, 3, 4]]).all()
    for f in (1, 2):
        assert np.array_equal(_bits(scores[f]), _bits(p.partition_scores(lt[f, :n[f]], lp[f, :n[f]])))
    # a row length below the count is over the cap too, not a read past the row
    scores, status = eng.partition_scores(_dev(lt[:, :100], torch.int32), _dev(lp, torch.int32), _dev(n, torch.int32))
    assert status.cpu().tolist() == [L.MPE_PART_OVER_CAP] * 4 + [0]
    eng.close()


@pytest.mark.parametrize('variant,persons,frames', [('panoptic', 4, 24), ('panoptic', 10, 12), ('ring23', 10, 3)])
def test_engine_methods_bit_equal_on_match_output(variant, persons, frames):
    """Real `match` output of synthetic 5 x 4, 5 x 10 and 23 x 10 batches: labels, GT groups, skip flags and scores of the
    three Engine methods equal the statement's."""
    p, syn = P(), pkg('synthetic')
    e = env(variant)
    eng = _engine(variant, max_frames=frames, persons=persons + 1)
    made = [syn.make_frame(e.calib, 50 + i, syn.FrameSpec(persons=persons, noise_px=1.0 if i % 2 else 0.0)) for i in range(frames)]
    full = [f for f, _ in made]
    if variant == 'panoptic':
        full[1] = _synthetic_frames()[30]                       # a body without '-1'
    packed = p.pack_bodies(full, e.params.used_cameras)
    db = eng.to_device(eng.pack([{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f in full]))
    _, persons_t, n_t = eng.match(db, want_scores=False)
    B = len(full)
    H = np.diff(np.asarray(db.host.frame_head_off[:B + 1]))
    M = np.diff(np.asarray(db.host.frame_en_off[:B + 1]))
    skip_in = (M == 0)
    skip_in[-1] = True                                          # one frame the caller excludes
    gt = eng.group_bodies(packed, skip_in=skip_in)
    est = eng.partition_labels(db, persons_t, n_t)
    scores, status = eng.partition_scores(gt['labels'], est['labels'], est['count'], skip=gt['skip'], count_true=gt['count'])
    eng.sync_status()
    pr, npn = persons_t.cpu().numpy(), n_t.cpu().numpy()
    g_lab, g_n, g_skip, g_cnt = (gt[k].cpu().numpy() for k in ('labels', 'n_groups', 'skip', 'count'))
    e_lab, e_cnt = est['labels'].cpu().numpy(), est['count'].cpu().numpy()
    assert np.array_equal(e_cnt, H) and np.array_equal(g_cnt, packed['n']) and not est['status'].cpu().numpy().any()
    want_skip = np.zeros(B, np.uint8)
    for f in range(B):
        want = p.proposal_labels(pr[f], int(npn[f]), int(H[f]))
        assert np.array_equal(e_lab[f, :H[f]], want) and (e_lab[f, H[f]:] == -1).all(), f
        if skip_in[f]:
            want_skip[f] = 1
            assert (g_lab[f] == -1).all() and g_n[f] == 0
            continue
        labels, n_groups, skip = p.group_bodies(packed['n'][f], packed['xyz'][f], packed['mask'][f], packed['nkeys'][f], packed['order'][f],
                                                packed['m1'][f])
        S = int(packed['n'][f])
        assert np.array_equal(g_lab[f, :S], labels) and (g_lab[f, S:] == -1).all() and g_n[f] == n_groups, f
        want_skip[f] = skip
    assert np.array_equal(g_skip, want_skip) and want_skip.sum() < B
    want = p.batch_scores(g_lab, e_lab, H, want_skip, packed['n'])
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(want))
    assert (~np.isnan(want[:, 0])).sum() >= B // 2
    eng.close()


def test_group_bodies_bit_equal_on_the_host_test_frames():
    """The frames of the host test (the committed harness input, noisy bodies, the special frames), grouped in batches."""
    p = P()
    eng = _engine()
    frames = _golden_frames()[::2] + _synthetic_frames()
    for start in range(0, len(frames), 16):
        chunk = frames[start:start + 16]
        pk = p.pack_bodies(chunk)
        gt = eng.group_bodies(pk)
        lab, ng, sk, st = (gt[k].cpu().numpy() for k in ('labels', 'n_groups', 'skip', 'status'))
        assert not st.any()
        for f in range(len(chunk)):
            labels, n_groups, skip = p.group_bodies(pk['n'][f], pk['xyz'][f], pk['mask'][f], pk['nkeys'][f], pk['order'][f], pk['m1'][f])
            S = int(pk['n'][f])
            assert np.array_equal(lab[f, :S], labels) and (lab[f, S:] == -1).all() and ng[f] == n_groups and sk[f] == skip, (start, f)
    eng.close()


def test_generated_scenes_bit_equal(tmp_path, monkeypatch):
    """The composed scenes of tests/golden/generated/ through sm_metrics_without_gt's device path: labels and scores of
    every graph equal the statement's on the proposals the harness returns."""
    from conftest import generated_fixture
    p = P()
    exp, arr, files, probs = generated_fixture()
    mdir = harness_model_files(str(tmp_path), {'gat': exp['gat'], 'mlp': {'kind': 'decoder', 'noise_seed': 3, 'noise_bound': 2e-4}})
    monkeypatch.chdir(tmp_path)
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.sm_metrics_without_gt')
    seen = []
    pipeline = pkg('pipeline')
    orig = pipeline.Engine.partition_scores

    def spy(self, lt, lp, count, **kw):
        scores, status = orig(self, lt, lp, count, **kw)
        seen.append((lt.cpu().numpy(), lp.cpu().numpy(), count.cpu().numpy(), scores.cpu().numpy()))
        return scores, status

    monkeypatch.setattr(pipeline.Engine, 'partition_scores', spy)
    out = m.main(['--testfiles'] + files + ['--modelsdir', mdir, '--datastep', '1', '--batch', '5', '--seed', str(exp['seed']), '--device-metrics'])
    assert out['n_data'] == exp['n_graphs'] and sum(len(s[2]) for s in seen) == exp['n_graphs']
    i = 0
    for lt, lp, count, scores in seen:
        assert np.array_equal(_bits(scores), _bits(p.batch_scores(lt, lp, count)))
        for f in range(len(count)):
            pg = out['per_graph'][i]
            assert np.array_equal(lt[f, :count[f]], p.proposal_labels(pg['gt'], len(pg['gt']), int(count[f])))
            assert np.array_equal(lp[f, :count[f]], p.proposal_labels(pg['est'], len(pg['est']), int(count[f])))
            i += 1


def _no_sklearn(monkeypatch, module=None):
    import sklearn.metrics

    def boom(*a, **k):
        raise AssertionError('sklearn.metrics was called on the device path')
    for name in ('adjusted_rand_score', 'homogeneity_completeness_v_measure'):
        monkeypatch.setattr(sklearn.metrics, name, boom)
        if module is not None and hasattr(module, name):
            monkeypatch.setattr(module, name, boom)


def _same(a, b):
    assert a['n_data'] == b['n_data'] and a['n_data'] > 0
    for k in KEYS:
        assert abs(a[k] - b[k]) <= 1e-12, (k, a[k], b[k])


@pytest.mark.parametrize('argv', [['--synthetic', '32', '--random-weights', '--teacher-scores', '--batch', '16'],
                                  ['--synthetic', '24', '--random-weights', '--batch', '16'],
                                  ['--synthetic', '12', '--random-weights', '--persons', '10', '--noise-px', '2', '--batch', '5']])
def test_sm_metrics_with_and_without_device_metrics(argv, monkeypatch):
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.sm_metrics')
    host = m.main(argv)
    with monkeypatch.context() as mp:
        _no_sklearn(mp, m)
        dev = m.main(argv + ['--device-metrics'])
    _same(host, dev)


def test_sm_metrics_device_metrics_on_the_golden_input(tmp_path, monkeypatch):
    """With the flag the harness still prints what /root/reference/test/sm_metrics.py printed for the committed files,
    the same as without it, and sklearn is not called."""
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'harness_expected.json')) as fh:
        exp = json.load(fh)
    mdir = harness_model_files(str(tmp_path), exp['inputs'])
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.sm_metrics')
    argv = ['--testfiles', os.path.join(hd, exp['inputs']['testfile']), '--tmdir', hd, '--modelsdir', mdir,
            '--datastep', str(exp['inputs']['datastep']), '--batch', '7']
    host = m.main(argv)
    with monkeypatch.context() as mp:
        _no_sklearn(mp, m)
        dev = m.main(argv + ['--device-metrics'])
    _same(host, dev)
    for k, v in exp['sm_metrics'].items():
        assert dev[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k


def test_sm_metrics_finishes_frames_over_the_cap_on_the_host(monkeypatch):
    """A frame over a compiled cap raises its status bit and comes back as NaN; the harness finishes it with the numpy
    statement, so the result is still the host path's.  The cap is reached here by a batch whose label rows are cut short."""
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.sm_metrics')
    L, pipeline = pkg('lib'), pkg('pipeline')
    argv = ['--synthetic', '20', '--random-weights', '--teacher-scores', '--batch', '8']
    host = m.main(argv)
    orig = pipeline.Engine.partition_labels
    raised = []

    def short_rows(self, db, persons, n_persons, hcap=None):
        out = orig(self, db, persons, n_persons, hcap=max(1, db.host.max_heads_per_frame() - 1))
        raised.append(int((out['status'].cpu().numpy() & L.MPE_PART_OVER_CAP != 0).sum()))
        return out

    monkeypatch.setattr(pipeline.Engine, 'partition_labels', short_rows)
    dev = m.main(argv + ['--device-metrics'])
    assert sum(raised) > 0
    _same(host, dev)


def test_sm_metrics_without_gt_with_and_without_device_metrics(tmp_path, monkeypatch):
    """--seed: the same four numbers and an equal per_graph with and without the flag; with it, the reference's printed
    numbers at the tolerance of tests/test_gpu_generated.py, and no sklearn call."""
    from conftest import generated_fixture
    exp, arr, files, probs = generated_fixture()
    mdir = harness_model_files(str(tmp_path), {'gat': exp['gat'], 'mlp': {'kind': 'decoder', 'noise_seed': 3, 'noise_bound': 2e-4}})
    monkeypatch.chdir(tmp_path)
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.sm_metrics_without_gt')
    argv = ['--testfiles'] + files + ['--modelsdir', mdir, '--datastep', '1', '--batch', '5', '--seed', str(exp['seed'])]
    host = m.main(argv)
    with monkeypatch.context() as mp:
        _no_sklearn(mp, m)
        dev = m.main(argv + ['--device-metrics'])
    _same(host, dev)
    assert dev['per_graph'] == host['per_graph']
    assert dev['n_data'] == exp['n_graphs']
    for k, v in exp['printed'].items():
        assert dev[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
