"""Without a GPU: the registry of tests/stream_cases.py against include/mpe.h -- every function that takes a `void *stream`
is run by an entry of the registry or exempt with a reason, so an entry point cannot arrive untested -- and
runtime.start_frame's use of the matcher hint across host threads, with fake engines."""
import os
import re
import threading
import types

import numpy as np
import pytest

import stream_cases as sc
from conftest import ROOT, env, pkg


def header_functions():
    """(name, takes a `void *stream`) of every function include/mpe.h declares with an int, void or size_t result, in its order."""
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        text = re.sub(r'/\*.*?\*/', ' ', fh.read(), flags=re.S)
    return [(m.group(1), bool(re.search(r'\bvoid\s*\*\s*stream\b', m.group(2))))
            for m in re.finditer(r'\b(?:int|void|size_t)\s+(mpe_\w+)\s*\(([^;{}]*?)\)\s*;', text)]


def stream_functions():
    return [name for name, stream in header_functions() if stream]


# The registry as it was reviewed: an entry that leaves, or arrives, changes this list too.
ENTRIES = '''match-3 match-40 gat_scores-3 gat_scores-40 gat_scores-feats gat_layer-0-featurised gat_layer-middle edge_softmax_aggregate cluster
dense_rows head_features mlp_input_rows mlp_forward mlp3d-3 mlp3d-40 match+mlp3d-3 triangulate linear dlt_pairs geom_scores geom_match
parse_json_device+finish_parse bodies_from_json ground_truth write_poses format_f64
evaluate reproject-est reproject-triang residual_stats partition_labels group_bodies partition_scores
refine-est refine-triang pose_covariance-est pose_covariance-triang regroup-est regroup-triang consolidate-est consolidate-triang
refine_timed-est refine_timed-triang body_refine-est body_refine-triang
Tracker.update+reset Smoother.update+reset Skeleton.observe+update+fit+reset+lengths Skeleton.set_lengths Relinker.update+reset+counters
TrackScore.update+reset+result+read_state
Calibrator.accumulate+read Calibrator.reset Calibrator.set_extrinsics Calibrator.step
CameraFitter.accumulate+read CameraFitter.reset CameraFitter.set_cameras CameraFitter.step
LagEstimator.accumulate+read LagEstimator.reset LagEstimator.estimate'''.split()


def test_the_header_parse_finds_the_stream_functions():
    names = stream_functions()
    assert len(names) == len(set(names)) >= 60
    for known in ('mpe_match_batch', 'mpe_calib_read', 'mpe_skel_get_lengths', 'mpe_format_f64', 'mpe_status_wait', 'mpe_lag_estimate'):
        assert known in names
    for no_stream in ('mpe_create', 'mpe_set_threshold', 'mpe_calib_get_extrinsics', 'mpe_profile_read', 'mpe_track_launches'):
        assert no_stream not in names


def test_every_stream_function_is_run_by_the_registry_or_exempt():
    names, covered = stream_functions(), sc.covered()
    missing = [n for n in names if n not in covered and n not in sc.EXEMPT]
    assert not missing, 'no entry of stream_cases.REGISTRY runs %s (and they are not in EXEMPT)' % ', '.join(missing)
    assert not [n for n in sc.EXEMPT if n in covered], 'exempt and covered at once'
    assert all(isinstance(why, str) and len(why) > 10 for why in sc.EXEMPT.values())
    strangers = sorted((covered | set(sc.EXEMPT)) - set(names))
    assert not strangers, 'not functions of include/mpe.h with a stream: %s' % strangers


def test_every_function_without_a_stream_has_its_reason():
    plain = [name for name, stream in header_functions() if not stream]
    assert len(plain) >= 40
    lost = [n for n in plain if not any(re.fullmatch(pat, n) for pat, _ in sc.NO_STREAM)]
    assert not lost, 'neither a stream nor a reason in stream_cases.NO_STREAM: %s' % ', '.join(lost)
    assert not [n for n in stream_functions() if any(re.fullmatch(pat, n) for pat, _ in sc.NO_STREAM)]
    assert all(any(re.fullmatch(pat, n) for n in plain) and len(why) > 10 for pat, why in sc.NO_STREAM)


def test_the_registry_is_the_reviewed_one():
    assert [e.name for e in sc.REGISTRY] == ENTRIES
    assert all(e.sync in (sc.NONE, sc.STREAM, sc.WRAPPER, sc.EITHER) and e.covers for e in sc.REGISTRY)
    assert all(name in ENTRIES for name, _ in sc.CONTROLS.values()) and sorted(sc.CONTROLS) == ['kernel', 'read', 'reset']


def test_decoy_batches_have_the_counts_of_the_true_ones():
    """What the matching cases rely on, on the host: 3 and 40 clean frames from two places of the generator pack to the same
    offsets with other pixels."""
    e = env('panoptic')
    packing = pkg('packing')
    fake = types.SimpleNamespace(calib=e.calib, V=len(e.params.used_cameras_skeleton_matching), pack=lambda frames: packing.pack_frames(frames, e.params))
    for n in (3, 40):
        x, d = fake.pack(sc.twin_frames(fake, 500, n)), fake.pack(sc.twin_frames(fake, 700, n))
        assert x.n_frames == n and np.array_equal(x.frame_head_off, d.frame_head_off) and np.array_equal(x.frame_en_off, d.frame_en_off)
        assert x.n_heads == 20 * n and not np.array_equal(x.xy, d.xy)


# ---- runtime.start_frame and host threads -----------------------------------------------------------------------------------------
class FakeEngine:
    """What start_frame touches of an engine, recording the thread of every call."""

    def __init__(self, fail=None):
        self.ctx, self._state, self.calls, self.fail = object(), {}, [], fail

    def _stream(self):
        return types.SimpleNamespace(value=0)

    def gat_scores_joined(self, db):
        import torch
        self.calls.append(threading.current_thread().name)
        out = torch.zeros(3)
        return out, out[1:]


class FakeGraph:
    batch_size, M = 1, 2
    packed = types.SimpleNamespace(en_pair=None)

    def device_batch(self, eng):
        if eng.fail is not None:
            raise eng.fail
        eng.calls.append(threading.current_thread().name)
        return types.SimpleNamespace(n_frames=2, n_edge_nodes=2, host=self.packed)      # (two frames: queue_proposals declines)


def _in_thread(name, fn):
    box = {}

    def body():
        try:
            box['value'] = fn()
        except BaseException as e:                            # noqa: B902 (handed to the caller's thread)
            box['error'] = e
    t = threading.Thread(target=body, name=name)
    t.start()
    t.join()
    if 'error' in box:
        raise box['error']
    return box.get('value')


def _note_and_start(runtime, eng):
    if eng is not None:
        runtime.note_matcher(eng)
    g = FakeGraph()
    runtime.start_frame(g)
    return g


def test_start_frame_stays_on_the_engine_its_own_thread_noted(monkeypatch):
    """One context per host thread: a dataset built on one thread must not enter the engine another thread's
    matcher noted."""
    runtime = pkg('runtime')
    monkeypatch.setenv('MPE_DROPIN_PREFETCH', '1')
    a, b = FakeEngine(), FakeEngine()
    g = _in_thread('thread-a', lambda: _note_and_start(runtime, a))
    assert g.__dict__['_scored'].engine is a and set(a.calls) == {'thread-a'}
    # a thread that has noted nothing queues nothing, whatever another thread's matcher noted
    g = _in_thread('thread-c', lambda: _note_and_start(runtime, None))
    assert '_scored' not in g.__dict__ and set(a.calls) == {'thread-a'}
    g = _in_thread('thread-b', lambda: _note_and_start(runtime, b))
    assert g.__dict__['_scored'].engine is b and set(b.calls) == {'thread-b'} and set(a.calls) == {'thread-a'}
    # two threads alive at once, each with its own matcher
    gate, out = threading.Barrier(2), {}

    def both(name, eng):
        runtime.note_matcher(eng)
        gate.wait()
        out[name] = _note_and_start(runtime, None)
    ts = [threading.Thread(target=both, args=(n, e), name=n) for n, e in (('thread-d', a), ('thread-e', b))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out['thread-d'].__dict__['_scored'].engine is a and out['thread-e'].__dict__['_scored'].engine is b
    assert set(a.calls) == {'thread-a', 'thread-d'} and set(b.calls) == {'thread-b', 'thread-e'}


def test_start_frame_declines_a_frame_beyond_capacity_and_nothing_else(monkeypatch):
    """check_capacity's ValueError is the expected decline; a failed launch (MpeError) or a bug propagates."""
    runtime, L = pkg('runtime'), pkg('lib')
    monkeypatch.setenv('MPE_DROPIN_PREFETCH', '1')
    g = FakeGraph()
    g.__dict__['_scored'] = 'stale'
    eng = FakeEngine(fail=ValueError('a frame holds 21 skeletons, capacity is 20'))
    runtime.note_matcher(eng)
    runtime.start_frame(g)
    assert '_scored' not in g.__dict__
    for err in (RuntimeError('a bug'), L.MpeError(-3, 'hipErrorLaunchFailure')):
        eng = FakeEngine(fail=err)
        runtime.note_matcher(eng)
        with pytest.raises(type(err)):
            runtime.start_frame(FakeGraph())
