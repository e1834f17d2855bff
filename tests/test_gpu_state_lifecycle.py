"""GPU: what the five device-state objects of the sequence stages (Tracker, Smoother, Skeleton, TrackScore, Calibrator)
have in common -- the launch count from creation on, reset() giving the same bytes again, close() twice, what every
public method raises on a closed object, and the NULL-state refusals of *_reset / *_launches / *_destroy.  The stages'
own tests hold their arithmetic; this one holds the lifecycle, at pcap 4 and two frames."""
import ctypes as C

import numpy as np
import pytest
import torch

import calib_cases as cc
import skel_cases as sc
import smooth_cases as smc
import track_cases as tc
import track_score_cases as tsc
from conftest import env, pkg

pytestmark = pytest.mark.gpu

PCAP, FRAMES = 4, slice(0, 2)


@pytest.fixture(scope='module')
def eng():
    e = env('panoptic')
    en = pkg('pipeline').Engine(e.params, e.calib, max_frames=32, max_persons_per_camera=4)
    assert en.J == tc.J
    yield en
    en.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frozen(x):
    """anything a stage returns, as something == compares byte for byte"""
    if isinstance(x, dict):
        return tuple((k, frozen(x[k])) for k in sorted(x) if not k.startswith('_'))
    if isinstance(x, (tuple, list)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return float(x).hex() if isinstance(x, float) else x


class Stage:
    """prefix: the C prefix; make(eng) -> the object; update(obj) -> what one update gives (synchronised); launches: the
    kernels that update enqueues; closed: {method: (arguments, exception)} for every public method of a closed object."""

    def __init__(self, prefix, make, update, launches, closed):
        self.prefix, self.make, self.update, self.launches, self.closed = prefix, make, update, launches, closed


def track_stage():
    seq = tc.hand_made()['swap_rows'][0]
    assert seq.poses.shape[1] == PCAP
    args = lambda: (dev(seq.poses[FRAMES]), dev(seq.flags[FRAMES]), dev(seq.n_persons[FRAMES]))
    return Stage('mpe_track', lambda eng: eng.tracker('mlp', max_gap=2, gate=0.5, pcap=PCAP), lambda eng, o: o.update(*args()),
                 6 + 3,                                      # init, a stage per frame of history, carry, two for births, resolve, finish
                 {'update': (args, RuntimeError), 'launches': (tuple, 'MpeError'), 'reset': (tuple, 'MpeError')})


def smooth_stage():
    c = smc.row_swap('tri')
    assert c.poses.shape[1] == PCAP
    args = lambda: tuple(dev(a[FRAMES]) for a in (c.poses, c.flags, c.n_persons, c.ids))
    return Stage('mpe_smooth', lambda eng: eng.smoother('tri', window=c.window, decay=c.decay, pcap=PCAP), lambda eng, o: o.update(*args()),
                 2, {'update': (args, RuntimeError), 'launches': (tuple, 'MpeError'), 'reset': (tuple, 'MpeError')})


def skel_stage():
    c = sc.one_bone('tri')
    assert c.pcap == PCAP and c.tid_cap == 8
    args = lambda: tuple(dev(a) for a in c.frames(FRAMES))

    def update(eng, o):
        o.observe(*args())
        o.update(1)
        return o.fit(*args(), iters=2), o.lengths()
    table = np.zeros((c.tid_cap, len(c.bones)))
    return Stage('mpe_skel', lambda eng: eng.skeleton('tri', bones=c.bones, bin_mm=c.bin_width * 1000.0, tid_cap=c.tid_cap, pcap=PCAP), update,
                 3,                                          # one kernel per call: observe, update, fit
                 {'observe': (args, RuntimeError), 'fit': (args, RuntimeError), 'set_lengths': (lambda: (table,), RuntimeError),
                  'update': (tuple, 'MpeError'), 'lengths': (tuple, 'MpeError'), 'launches': (tuple, 'MpeError'), 'reset': (tuple, 'MpeError')})


def track_score_stage():
    c = tsc.Case([([(0, 1), (1, 1)], [tsc.D(1, 0), tsc.D(2, 1, 30.)]), ([(0, 1), (1, 1)], [tsc.D(2, 0), tsc.D(1, 1)])], None,
                 gid_cap=4, tid_cap=8, cap=PCAP)
    a = c.arrays()

    def args():
        ev = {k: dev(a[k]) for k in ('assign', 'err', 'invalid', 'n_res', 'n_gt')}
        return ev, dev(a['flags']), dev(a['n_persons']), dev(a['track_ids']), dev(a['gt_ids']), dev(a['gt_valid'])

    def update(eng, o):
        out = o.update(*args())
        return {k: out[k].cpu() for k in out}, o.result(), o.read_state()
    return Stage('mpe_track_score', lambda eng: eng.track_scorer('mlp', gid_cap=c.gid_cap, tid_cap=c.tid_cap, max_frames=4, gcap=PCAP, pcap=PCAP),
                 update, 3,
                 {'update': (args, RuntimeError), 'result': (tuple, 'MpeError'), 'read_state': (tuple, 'MpeError'),
                  'launches': (tuple, 'MpeError'), 'reset': (tuple, 'MpeError')})


def calib_stage():
    made = {}

    def args(eng):
        if not made:
            s = cc.small('panoptic', n_frames=2, n_bodies=2, pcap=eng.pcap)
            poses, flags, mask = s.kinds['triang']
            made['a'] = (eng.to_device(s.pb), dev(s.persons), dev(s.n_persons), dev(poses), dev(flags))
            made['mask'] = mask
        return made['a']

    def update(eng, o):
        a = args(eng)
        o.accumulate(*a, joint_mask=made['mask'])
        return o.read()
    E = np.zeros((5, 3, 4))
    closed = {k: (tuple, RuntimeError) for k in ('read', 'step', 'extrinsics', 'calibration', 'launches', 'reset')}
    closed['accumulate'] = (lambda: made['a'], RuntimeError)
    closed['set_extrinsics'] = (lambda: (E,), RuntimeError)
    return Stage('mpe_calib', lambda eng: eng.calibrator('triang', min_obs=6), update, 2, closed)


STAGES = {'track': track_stage, 'smooth': smooth_stage, 'skel': skel_stage, 'track_score': track_score_stage, 'calib': calib_stage}


@pytest.mark.parametrize('name', sorted(STAGES))
def test_lifecycle(eng, name):
    L = pkg('lib')
    st = STAGES[name]()
    obj = st.make(eng)
    try:
        assert obj.launches() == 0
        first = frozen(st.update(eng, obj))
        torch.cuda.synchronize()
        assert obj.launches() == st.launches, obj.launches()
        obj.reset()
        again = frozen(st.update(eng, obj))
        torch.cuda.synchronize()
        assert again == first
    finally:
        obj.close()
    obj.close()                                              # twice: harmless
    assert not obj.state
    for method, (args, exc) in sorted(st.closed.items()):
        exc = L.MpeError if exc == 'MpeError' else exc
        with pytest.raises(exc) as err:
            getattr(obj, method)(*args())
        assert type(err.value) is exc, (method, type(err.value))
        if exc is L.MpeError:
            assert err.value.code == -1 and (st.prefix + '_') in str(err.value), (method, str(err.value))
    public = {m for m in dir(obj) if not m.startswith('_') and callable(getattr(obj, m))} - {'close'}
    assert public == set(st.closed), public ^ set(st.closed)


@pytest.mark.parametrize('name', sorted(STAGES))
def test_null_state(eng, name):
    prefix = STAGES[name]().prefix
    lib, n = eng.lib, C.c_int64(7)
    for entry, call in (('_reset', lambda f: f(eng.ctx, eng._stream(), None)), ('_launches', lambda f: f(eng.ctx, None, C.byref(n))),
                        ('_destroy', lambda f: f(eng.ctx, None))):
        assert call(getattr(lib, prefix + entry)) == -1
        assert (prefix + entry).encode() in lib.mpe_last_error(eng.ctx), lib.mpe_last_error(eng.ctx)
    assert n.value == 7
