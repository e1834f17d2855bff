"""What tests/test_gpu_streams.py and tests/test_streams_host.py share: the delayed-producer protocol and the registry of
entry points it is run on.  Not a test module.

include/mpe.h promises of every function that takes a `void *stream` that its work is ordered on that stream.  On torch's
default stream (the legacy null stream, which orders itself against every blocking stream) a launch, a memset or a copy
that is handed 0 instead of the caller's stream cannot be told from a correct one, so the protocol runs every call on a
side stream S behind a producer that is late:

  1. default stream, synchronised: want = call(X), other = call(D) on fresh state.  D (the decoy) has X's shapes and counts
     and is valid data of its own; want != other, else the case could notice nothing.
  2. on S: buffers holding D; a spin kernel that keeps S busy for `delay` and leaves the GPU free; the event `busy`; X copied
     into the buffers device to device; the call; still_running = not busy.query(); S.synchronize().
  3. a call documented as not synchronising must have returned while the delay ran; one documented as synchronising
     `stream` must not have.
  4. every output equals `want` bit for bit.  Whatever the call put on another stream ran during the delay, on D.

A stateful stage runs update(D), reset(), update(X) and then its read, all behind the delay: an early reset, an early read
and a stray launch each change the answer.  Every comparison is bitwise; no tolerance exists here.

REGISTRY holds one Entry per call; Entry.covers names the functions of include/mpe.h the call goes through.
tests/test_streams_host.py holds the header to REGISTRY + EXEMPT, so an entry point cannot arrive untested."""
import contextlib
import ctypes as C
import json
import time

import numpy as np

from conftest import env, oracle, pkg

# ---- the functions with a `void *stream` that the protocol does not run, each with its reason ------------------------------
EXEMPT = {
    'mpe_sync_status': 'the status word has tests of its own in test_gpu_streams.py (test_status_word_*): its answer is an '
                       'error code, not a buffer the protocol could compare',
    'mpe_status_queue': 'as mpe_sync_status',
    'mpe_status_wait': 'as mpe_sync_status',
}
# The functions WITHOUT a stream, by pattern (first match), each with the reason it needs no case here.  The header test holds every
# such function to one of them, so a new one gets a decision as well.
NO_STREAM = (
    (r'mpe_profile_\w+', 'profiling switches and read-backs: mpe_profile_read synchronises the whole device, by its documentation'),
    (r'mpe_(\w+_)?create', 'creators allocate and fill with blocking calls before any stream holds work of theirs'),
    (r'mpe_(\w+_)?destroy', 'destroyers: the caller has synchronised (mpe_destroy synchronises the device itself)'),
    (r'mpe_set_(gat|mlp)_(params|layer)|mpe_set_precision|mpe_set_gat_output|mpe_set_log_table|mpe_upload_linear|mpe_free_device',
     'weight and mode setters: blocking uploads, made before the batches that use them'),
    (r'mpe_set_threshold', 'no stream in its signature; include/mpe.h: call it only with nothing pending on the context'),
    (r'mpe_\w+_launches', 'host-side counters'),
    (r'mpe_calib_get_extrinsics|mpe_camfit_get_cameras', 'host copies of the state the library keeps on the host'),
    (r'mpe_pack\w*|mpe_json_index_\w+|mpe_json_stage_\w+|mpe_json_\w*(bytes|bound)', 'host-only: packer, staging and size arithmetic'),
)

NONE, STREAM, WRAPPER, EITHER = 'none', 'stream', 'wrapper', 'either'
# Entry.sync: NONE    documented as not synchronising: the call must return while the delay runs (a read that follows it
#                     in the case, Case.read, is documented as synchronising `stream` and must not);
#             STREAM  the C function is documented as synchronising `stream`;
#             WRAPPER the function does not synchronise, its pipeline.py wrapper does after the launch (it reads the result
#                     back or says so): the wrapper must have waited;
#             EITHER  the header says neither (the *_reset / *_set_* of the calibrator family synchronise today): only the
#                     order is checked.


class Entry:
    def __init__(self, name, covers, sync, build, note):
        self.name, self.covers, self.sync, self.build, self.note = name, tuple(covers), sync, build, note


REGISTRY = []


def entry(name, covers, sync, note=''):
    def deco(fn):
        assert name not in [e.name for e in REGISTRY], name
        REGISTRY.append(Entry(name, covers, sync, fn, note))
        return fn
    return deco


def by_name(name):
    return next(e for e in REGISTRY if e.name == name)


def covered():
    return {c for e in REGISTRY for c in e.covers}


class Case:
    """X / D: {name: device tensor or DeviceBatch}, the true inputs and the decoy, same keys, shapes and counts.
    fresh(r): makes the state objects of a run in r (default stream or S, before the delay); run(r, b, dec) -> the outputs of the
    call(s) on the buffers b, dec = D for the calls of a stateful stage that come before its reset; read(r) -> what the
    stage's synchronising read gives; canon(out) -> out with the rows no kernel writes masked; close(r)."""

    def __init__(self, X, D, run, read=None, fresh=None, canon=None, close=None):
        self.X, self.D, self.run, self.read, self.fresh = X, D, run, read, fresh
        self.canon = canon or (lambda out: out)
        self._close = close

    def close(self, r):
        for o in r.objects:
            o.close()
        if self._close:
            self._close(r)


class Run:
    """What one run of a case keeps: the engine, the state objects to close, and `on(label)`: the context a control puts
    around the call it misplaces (nothing otherwise)."""

    def __init__(self, eng, hook=None, skip=()):
        self.eng, self._hook, self.skip, self.objects = eng, hook, set(skip), []

    def on(self, label):
        return self._hook(label) if self._hook else contextlib.nullcontext()

    def own(self, obj):
        self.objects.append(obj)
        return obj


def frozen(x):
    """anything a call returns, as something == compares byte for byte"""
    import torch
    if isinstance(x, dict):
        return tuple((k, frozen(x[k])) for k in sorted(x) if not k.startswith('_'))
    if isinstance(x, (tuple, list)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    return x


class Host:
    """An input that lives on the host (a document the call stages and uploads itself): it changes hands at once."""

    def __init__(self, value):
        self.value = value


def _is_batch(v):
    return hasattr(v, 'struct') and hasattr(v, 'buf')


def clone_inputs(eng, inputs):
    """Buffers of their own holding `inputs` (current stream)."""
    out = {}
    for k, v in inputs.items():
        out[k] = pkg('packing').DeviceBatch(v.host, eng.device) if _is_batch(v) else Host(v.value) if isinstance(v, Host) else v.clone()
    return out


def fill_inputs(bufs, inputs):
    """inputs -> the same buffers, device to device, on the current stream, without waiting."""
    for k, v in inputs.items():
        if isinstance(v, Host):
            bufs[k].value = v.value
        elif _is_batch(v):
            assert bufs[k].buf.numel() == v.buf.numel() and (bufs[k].n_frames, bufs[k].n_heads, bufs[k].n_edge_nodes) == (v.n_frames, v.n_heads, v.n_edge_nodes)
            bufs[k].buf.copy_(v.buf, non_blocking=True)
            bufs[k].rebind(v.host)                       # new contents at the same addresses: a new generation
        else:
            assert bufs[k].shape == v.shape and bufs[k].dtype == v.dtype, k
            bufs[k].copy_(v, non_blocking=True)


def reference(eng, case, inputs, skip=()):
    """Step 1 for one set of inputs: the call on the default stream, fresh state, synchronised before and after.
    -> (frozen outputs, host seconds of the call including its wait)."""
    import torch
    torch.cuda.synchronize()
    r = Run(eng, skip=skip)
    try:
        b = clone_inputs(eng, inputs)
        if case.fresh:
            case.fresh(r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = case.run(r, b, case.D)
        if case.read:
            out = (out, case.read(r))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return frozen(case.canon(out)), dt
    finally:
        case.close(r)
        eng.sync_status()


class Delayed:
    """What step 2 saw: out (frozen), still_running (after the last call that is not a read), read_waited (busy.query() after the
    read; None without one), delay_ms as measured by events around the spin kernel."""


def delayed(eng, case, S, cycles, hook=None):
    import torch
    torch.cuda.synchronize()
    r = Run(eng, hook)
    res = Delayed()
    try:
        with torch.cuda.stream(S):
            b = clone_inputs(eng, case.D)
            if case.fresh:
                case.fresh(r)
            S.synchronize()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(S)
            torch.cuda._sleep(int(cycles))
            t1.record(S)
            busy = torch.cuda.Event()
            busy.record(S)
            fill_inputs(b, case.X)
            out = case.run(r, b, case.D)
            res.still_running = not busy.query()
            res.read_waited = None
            if case.read:
                out = (out, case.read(r))
                res.read_waited = busy.query()
            S.synchronize()
        torch.cuda.synchronize()
        res.delay_ms = t0.elapsed_time(t1)
        res.out = frozen(case.canon(out))
        return res
    finally:
        torch.cuda.synchronize()
        case.close(r)
        eng.sync_status()


def calibrate_spin(S):
    """Cycles of torch.cuda._sleep per millisecond on this device, from events around two spins of different length (their
    difference: the launch cost cancels)."""
    import torch
    torch.cuda.synchronize()
    ms = []
    for cycles in (2_000_000, 2_000_000, 22_000_000):        # (the first: warm-up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            a.record(S)
            torch.cuda._sleep(cycles)
            b.record(S)
        S.synchronize()
        ms.append(a.elapsed_time(b))
    rate = 20_000_000 / max(ms[2] - ms[1], 1e-3)
    return rate


def delay_cycles(rate, call_seconds):
    """At least ten times the host-side duration of the call, and at least 20 ms."""
    ms = max(20.0, 10.0 * call_seconds * 1e3)
    return int(ms * rate), ms


@contextlib.contextmanager
def forced_stream(eng, handle):
    """Engine._stream gives `handle` (0: the NULL stream) inside: what a launch site that forgot its stream does."""
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(type(eng), '_stream', lambda self: C.c_void_p(handle))
        yield


# ---- the inputs -------------------------------------------------------------------------------------------------------------
class World:
    """The engine of the module and what its cases share, made once."""

    def __init__(self, eng):
        self.eng, self.device, self._memo = eng, eng.device, {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def frames(self, n):
        """(X, D): n processed frames each of four persons whom every camera sees (20 heads, 160 edge-nodes a frame), from
        the generator's frames 500 ... and 700 ...: equal counts, other pixels."""
        return self.memo(('frames', n), lambda: (twin_frames(self.eng, 500, n), twin_frames(self.eng, 700, n)))

    def batches(self, n):
        def make():
            fx, fd = self.frames(n)
            px, pd = self.eng.pack(fx), self.eng.pack(fd)
            assert np.array_equal(px.frame_head_off, pd.frame_head_off) and np.array_equal(px.frame_en_off, pd.frame_en_off)
            assert not np.array_equal(px.xy, pd.xy)
            return self.eng.to_device(px), self.eng.to_device(pd)
        return self.memo(('batches', n), make)

    def persons(self, n):
        """((persons, n_persons) of X, of D): what match gives for the two batches."""
        def make():
            out = []
            for db in self.batches(n):
                _, p, k = self.eng.match(db)
                out.append((p, k))
            self.eng.sync_status()
            return tuple(out)
        return self.memo(('persons', n), make)

    def scenes(self, n_frames=4):
        """(X, D): calib_cases.small at two seeds with the engine's Pcap: persons, poses of both kinds, detections."""
        import calib_cases as cc
        return self.memo(('scenes', n_frames), lambda: tuple(cc.small('panoptic', n_frames=n_frames, n_bodies=2, pcap=self.eng.pcap, seed=s)
                                                             for s in (4300, 4400)))

    def walks(self, n_frames=6, pcap=4):
        """(X, D): lag_cases.Scene at two seeds: a recording of two bodies on seeded walks with its table and track ids."""
        import lag_cases as lc
        return self.memo(('walks', n_frames, pcap), lambda: tuple(lc.Scene('panoptic', n_frames, (0, 0.5, -0.25, 1.25, -1.5), n_bodies=2, seed=s, pcap=pcap)
                                                                  for s in (5100, 5500)))


def twin_frames(eng, start, n):
    syn, onp = pkg('synthetic'), oracle()
    out, i = [], start
    while len(out) < n:
        f = onp.processed_input(syn.make_frame(eng.calib, i, syn.FrameSpec(persons=4))[0])
        i += 1
        pb = eng.pack([f])
        if pb.n_heads == 4 * eng.V and list(np.asarray(pb.slot_n).reshape(-1)) == [4] * eng.V:
            out.append(f)
        assert i < start + 4 * n + 40, 'too few clean frames'
    return out


def mask_persons(persons, n_persons):
    """persons [B,Pcap,V] with the rows from n_persons[f] on (which no kernel writes) set to -1"""
    import torch
    p = persons.clone()
    rows = torch.arange(p.shape[1], device=p.device)[None, :] >= n_persons.clamp(0, p.shape[1])[:, None].to(torch.int64)
    p[rows] = -1
    return p


def mask_by(values, flags):
    """values [..., k...] with the entries whose flag (leading dimensions) is 0 zeroed"""
    v = values.clone()
    v[flags == 0] = 0
    return v


def scene_inputs(w, s, kind):
    poses, flags, mask = s.kinds[kind]
    return {'db': w.eng.to_device(s.pb), 'persons': w.dev(s.persons), 'n': w.dev(s.n_persons), 'poses': w.dev(poses), 'flags': w.dev(flags)}, mask


def walk_inputs(w, s, kind, with_batch=True):
    poses, flags, mask = s.kinds[kind]
    t = {'poses': w.dev(poses), 'flags': w.dev(flags), 'n': w.dev(s.n_persons), 'ids': w.dev(s.ids)}
    if with_batch:
        t['db'], t['persons'] = w.eng.to_device(s.pb), w.dev(s.persons)
    return t, mask


def same_layout(a, b):
    """two PackedBatches of equal counts, frame by frame"""
    assert np.array_equal(a.frame_head_off, b.frame_head_off) and np.array_equal(a.frame_en_off, b.frame_en_off)


# ---- matching / 3D ----------------------------------------------------------------------------------------------------------
def _match_case(n):
    def build(w):
        X, D = w.batches(n)

        def run(r, b, dec):
            s, p, k = r.eng.match(b['db'])
            return s, p, k
        return Case({'db': X}, {'db': D}, run, canon=lambda o: (o[0], mask_persons(o[1], o[2]), o[2]))
    return build


entry('match-3', ['mpe_match_batch'], NONE, 'the latency launches (<= 16 frames)')(_match_case(3))
entry('match-40', ['mpe_match_batch'], NONE, 'the tile kernels')(_match_case(40))


def _gat_scores_case(n):
    def build(w):
        X, D = w.batches(n)
        return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.gat_scores(b['db'], heads=True))
    return build


entry('gat_scores-3', ['mpe_gat_forward'], NONE)(_gat_scores_case(3))
entry('gat_scores-40', ['mpe_gat_forward'], NONE)(_gat_scores_case(40))


@entry('gat_scores-feats', ['mpe_gat_forward'], NONE, 'the caller\'s dense rows: one frame, the rows late, the batch in place')
def _gat_feats(w):
    X, D = w.batches(1)
    fx, fd = w.eng.dense_rows(X).clone(), w.eng.dense_rows(D).clone()
    return Case({'feats': fx}, {'feats': fd}, lambda r, b, dec: r.eng.gat_scores(X, heads=True, feats=b['feats']))


@entry('gat_layer-0-featurised', ['mpe_gat_layer'], NONE, 'layer 0 with x = None: rows featurised on the device')
def _gat_layer0(w):
    X, D = w.batches(3)
    return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.gat_layer(b['db'], 0, None))


@entry('gat_layer-middle', ['mpe_gat_layer'], NONE, 'a middle layer on the caller\'s rows')
def _gat_layer_mid(w):
    X, D = w.batches(3)
    layer = 1
    assert len(w.eng.gat_dims) > 2                            # layer 1 is neither the first nor the last
    xx, xd = w.eng.gat_layer(X, 0, None).clone(), w.eng.gat_layer(D, 0, None).clone()
    return Case({'db': X, 'x': xx}, {'db': D, 'x': xd}, lambda r, b, dec: r.eng.gat_layer(b['db'], layer, b['x']))


@entry('edge_softmax_aggregate', ['mpe_edge_softmax_aggregate'], NONE)
def _esa(w):
    import torch
    X, D = w.batches(3)
    _, nh, od = w.eng.gat_dims[1]
    n_nodes = X.n_heads + X.n_edge_nodes
    g = torch.Generator().manual_seed(77)
    fx, fd = (torch.randn((n_nodes, nh * od), generator=g, dtype=torch.float32).to(w.device) for _ in range(2))
    return Case({'db': X, 'ft2': fx}, {'db': D, 'ft2': fd}, lambda r, b, dec: r.eng.edge_softmax_aggregate(b['db'], 1, b['ft2']))


@entry('cluster', ['mpe_cluster_batch'], NONE)
def _cluster(w):
    X, D = w.batches(3)
    sx, sd = w.eng.gat_scores(X).clone(), w.eng.gat_scores(D).clone()

    def run(r, b, dec):
        return r.eng.cluster(b['db'], b['scores'])
    return Case({'db': X, 'scores': sx}, {'db': D, 'scores': sd}, run, canon=lambda o: (mask_persons(o[0], o[1]), o[1]))


@entry('dense_rows', ['mpe_dense_rows'], NONE, 'one graph per call')
def _dense_rows(w):
    X, D = w.batches(1)
    return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.dense_rows(b['db']))


@entry('head_features', ['mpe_head_features'], NONE)
def _head_features(w):
    X, D = w.batches(3)
    return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.head_features(b['db']))


def _rows_inputs(w, n):
    X, D = w.batches(n)
    (px, kx), (pd, kd) = w.persons(n)
    return {'db': X, 'persons': px, 'n': kx}, {'db': D, 'persons': pd, 'n': kd}


@entry('mlp_input_rows', ['mpe_mlp_input_rows'], NONE)
def _mlp_rows(w):
    X, D = _rows_inputs(w, 3)
    return Case(X, D, lambda r, b, dec: r.eng.mlp_input_rows(b['db'], b['persons'], b['n']), canon=lambda o: (mask_by(o[0], o[1]), o[1]))


@entry('mlp_forward', ['mpe_mlp_forward'], NONE)
def _mlp_forward(w):
    X, D = _rows_inputs(w, 3)
    rx, rd = (w.eng.mlp_input_rows(t['db'], t['persons'], t['n'])[0].reshape(-1, w.eng.V * w.eng.J * w.eng.params.numbers_per_joint).contiguous() for t in (X, D))
    return Case({'x': rx}, {'x': rd}, lambda r, b, dec: r.eng.mlp_forward(b['x']))


def _mlp3d_case(n):
    def build(w):
        X, D = _rows_inputs(w, n)
        return Case(X, D, lambda r, b, dec: r.eng.mlp3d(b['db'], b['persons'], b['n']), canon=lambda o: (mask_by(o[0], o[1]), o[1]))
    return build


entry('mlp3d-3', ['mpe_mlp3d_batch'], NONE)(_mlp3d_case(3))
entry('mlp3d-40', ['mpe_mlp3d_batch'], NONE)(_mlp3d_case(40))


@entry('match+mlp3d-3', ['mpe_match_batch', 'mpe_mlp3d_batch'], NONE, 'the pair solves match leaves for mlp3d travel on the stream as well')
def _match_mlp3d(w):
    X, D = w.batches(3)

    def run(r, b, dec):
        _, p, k = r.eng.match(b['db'], want_scores=False)
        return (p, k) + tuple(r.eng.mlp3d(b['db'], p, k))
    return Case({'db': X}, {'db': D}, run, canon=lambda o: (mask_persons(o[0], o[1]), o[1], mask_by(o[2], o[3]), o[3]))


@entry('triangulate', ['mpe_triangulate_batch'], NONE)
def _triangulate(w):
    X, D = _rows_inputs(w, 3)
    return Case(X, D, lambda r, b, dec: r.eng.triangulate(b['db'], b['persons'], b['n']), canon=lambda o: (mask_by(o[0], o[1]), o[1]))


@entry('linear', ['mpe_linear'], WRAPPER, 'Engine.linear synchronises the device after the launch')
def _linear(w):
    rng = np.random.default_rng(31)
    wt, bias = rng.normal(size=(20, 70)).astype(np.float32), rng.normal(size=20).astype(np.float32)
    xx, xd = (w.dev(rng.normal(size=(33, 70)).astype(np.float32)) for _ in range(2))
    return Case({'x': xx}, {'x': xd}, lambda r, b, dec: r.eng.linear(b['x'], wt, bias, slope=0.1))


@entry('dlt_pairs', ['mpe_dlt_pairs'], NONE)
def _dlt_pairs(w):
    import dlt_cases
    s = dlt_cases.systems('panoptic')
    X = {'pts': w.dev(s.pix[:64]), 'cams': w.dev(s.cams[:64])}
    D = {'pts': w.dev(s.pix[64:128]), 'cams': w.dev(s.cams[64:128])}
    return Case(X, D, lambda r, b, dec: r.eng.dlt_pairs(b['pts'], b['cams']))


@entry('geom_scores', ['mpe_geom_scores_batch'], NONE)
def _geom_scores(w):
    X, D = w.batches(3)
    return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.geom_scores(b['db'], details=True))


@entry('geom_match', ['mpe_geom_match_batch'], NONE)
def _geom_match(w):
    X, D = w.batches(3)
    return Case({'db': X}, {'db': D}, lambda r, b, dec: r.eng.geom_match(b['db']), canon=lambda o: (o[0], mask_persons(o[1], o[2]), o[2]))


# ---- JSON / ground truth ------------------------------------------------------------------------------------------------------
def _wire_text(eng, start, order):
    syn = pkg('synthetic')
    frames = [syn.make_frame(eng.calib, start + i, syn.FrameSpec(persons=2))[0] for i in range(4)]
    return json.dumps([frames[i] for i in order]).encode()


@entry('parse_json_device+finish_parse', ['mpe_json_parse_device'], WRAPPER,
       'the producer is the wrapper\'s own upload of the staged strings; finish_parse waits for the event behind the parse')
def _parse_json(w):
    import torch
    packing = pkg('packing')
    eng = w.eng
    tx, td = _wire_text(eng, 40, (0, 1, 2, 3)), _wire_text(eng, 40, (3, 2, 1, 0))       # the decoy: the same frames in another order
    cap = 2 * max(len(tx), len(td)) + 16 * 4 * eng.V + 256
    staged = {}
    for name, text in (('X', tx), ('D', td)):
        bufs = eng.json_device_buffers(4, text_cap=cap)
        index = packing.JsonIndex(text)
        try:
            staged[name] = (bufs, packing.stage_json_window(index, eng.params, bufs['host'], 0, 1, 4, 0))
        finally:
            index.close()
    assert staged['X'][1][:2] == staged['D'][1][:2]                                        # frames and entries: equal counts
    host = {k: torch.empty_like(staged[k][0]['host'].buf).copy_(staged[k][0]['host'].buf) for k in staged}

    def fresh(r):
        # the device staging and the arena hold the decoy, parsed: what a stray launch would read and leave
        r.bufs = eng.json_device_buffers(4, text_cap=cap)
        r.bufs['host'].buf.copy_(host['D'])
        eng.parse_json_device(r.bufs, *staged['D'][1])
        assert eng.finish_parse(r.bufs) is not None

    def run(r, b, dec):
        which = b['which'].value
        r.bufs['host'].buf.copy_(host[which])
        eng.parse_json_device(r.bufs, *staged[which][1])
        pd = eng.finish_parse(r.bufs)
        assert pd is not None
        got = pd.download()
        return tuple(np.asarray(getattr(got, f)) for f in ('frame_head_off', 'frame_en_off', 'slot_cam', 'slot_n', 'head_cam', 'skeleton_index',
                                                           'joint_mask', 'tri_mask', 'xy', 'vp'))
    return Case({'which': Host('X')}, {'which': Host('D')}, run, fresh=fresh)


HAND_BODIES = '''[
 {"camA": ["[]", 0.5, "no_image", [ ]],
  "camX": ["[]", 0.5, "no_image", [{"-1": [1, 2, 3], "0": [-0.0, 12, 1e-05]}, {}]],
  "camB": ["[]", 0.5, "no_image", [
     {"17": [-3.25E+1, 0.1, 123456.78901234567], "3": [1.5, -2.5e2, 7], "0": [0, 0.0, -0.0]},
     { "2" : [ 1.0 ,
               2.0 , 3.0 ] ,  "-1" : [ 4 , 5 , 6 ] }
  ]]},
 {"camB": ["[]", 1, "no_image", [{"30": [9.007199254740993e15, 2.5e-20, 1.7976931348623157e30], "-1": [0.3, 0.7, 1e22]}]],
  "camA": ["[]", 1, "no_image", [{}]]},
 {"camA": ["[]", 2, "no_image", []], "camB": ["[]", 2, "no_image", []], "camX": ["[]", 2, "no_image", []]},
 {"camA": ["[]", 3, "no_image", [{"4": [0.25, -7, 1e3], "-1": [2, 2, 2]}]], "camB": ["[]", 3, "no_image", [{"1": [5, 6, 7]}]]}
]'''                                                              # test_gpu_groundtruth.py's document and a fourth frame


@entry('bodies_from_json', ['mpe_json_parse_bodies_device'], WRAPPER,
       'the producer is the wrapper\'s own upload of the staged lists; it reads the status word back and says so')
def _bodies(w):
    eng = w.eng
    frames = json.loads(HAND_BODIES)
    text = {'X': json.dumps(frames).encode(), 'D': json.dumps(frames[::-1]).encode()}
    kw = dict(max_frames=4, scap=5, cameras=['camA', 'camB'])

    def fresh(r):
        assert eng.bodies_from_json(text['D'], **kw).status == 0      # the engine's device staging holds the decoy

    def run(r, b, dec):
        pb = eng.bodies_from_json(text[b['which'].value], **kw)
        assert pb.status == 0
        return pb.numpy()
    return Case({'which': Host('X')}, {'which': Host('D')}, run, fresh=fresh)


GT_SCAP = 24                                                      # rows of a frame: the bodies of all its cameras (the fixture: up to 5 x 4)


def _fixture_bodies(w, start):
    from test_groundtruth_host import fixture
    pb = w.eng.bodies_from_json(fixture()[0], frame_start=start, max_frames=4, scap=GT_SCAP)
    assert pb.status == 0 and pb.n_frames == 4
    return pb


@entry('ground_truth', ['mpe_gt_from_bodies'], NONE,
       'through the C entry point with Engine.ground_truth\'s arguments: the wrapper uploads its transforms with a blocking copy '
       'BEFORE the launch, which would let the delay pass and hide a misplaced launch')
def _ground_truth(w):
    import torch
    from test_groundtruth_host import transforms
    eng, L = w.eng, pkg('lib')
    bx, bd = _fixture_bodies(w, 0), _fixture_bodies(w, 4)
    assert bx.n_entries == bd.n_entries
    keys = ('entries', 'frame_entry_off', 'entry_count', 'xyz', 'mask', 'm1')
    T_d1, T_i1 = transforms()
    Td = w.dev(np.ascontiguousarray(T_d1.numpy().reshape(1, 4, 4), np.float32))
    fof = w.dev(np.zeros(4, np.int32))
    Ti = np.ascontiguousarray(T_i1.numpy().reshape(16), np.float32)

    def run(r, b, dec):
        d = eng.device
        G = GT_SCAP
        out = {'xyz': torch.empty((4, G, eng.J, 3), dtype=torch.float32, device=d), 'joint': torch.empty((4, G, eng.J), dtype=torch.uint8, device=d),
               'valid': torch.empty((4, G), dtype=torch.uint8, device=d), 'n': torch.empty((4,), dtype=torch.int32, device=d)}
        a = L.mpe_gt_args()
        a.n_frames, a.scap, a.gcap, a.n_joints, a.n_files = 4, G, G, eng.J, 1
        a.d_entries, a.d_frame_entry_off, a.d_entry_count = b['entries'].data_ptr(), b['frame_entry_off'].data_ptr(), b['entry_count'].data_ptr()
        a.d_xyz, a.d_mask, a.d_m1 = b['xyz'].data_ptr(), b['mask'].data_ptr(), b['m1'].data_ptr()
        a.d_T_d, a.d_file_of_frame, a.T_i1 = Td.data_ptr(), fof.data_ptr(), Ti.ctypes.data_as(L.c_f32p)
        a.d_gt_xyz, a.d_gt_joint, a.d_gt_valid, a.d_n_gt_in = (out[k].data_ptr() for k in ('xyz', 'joint', 'valid', 'n'))
        eng._chk(eng.lib.mpe_gt_from_bodies(eng.ctx, eng._stream(), C.byref(a)))
        return out
    return Case({k: getattr(bx, k).contiguous() for k in keys}, {k: getattr(bd, k).contiguous() for k in keys}, run)


def _walk_tri(w):
    sx, sd = w.walks()
    return walk_inputs(w, sx, 'triang', False)[0], walk_inputs(w, sd, 'triang', False)[0]


def _written(o):
    total = int(o._total.cpu()[0])
    return (o.text[:total], o.frame_off, o.rows_written, o.status, o._total)


@entry('write_poses', ['mpe_json_write_poses'], NONE)
def _write_poses(w):
    X, D = _walk_tri(w)
    X, D = ({k: v[:4].contiguous() for k, v in t.items()} for t in (X, D))
    return Case(X, D, lambda r, b, dec: r.eng.write_poses(b['poses'], b['flags'], b['n'], 'triang', ids=b['ids'], frame_start=7, scale=100.0), canon=_written)


@entry('format_f64', ['mpe_format_f64'], NONE)
def _format_f64(w):
    import write_cases as wc
    return Case({'v': w.dev(wc.ADVERSARIAL)}, {'v': w.dev(wc.ADVERSARIAL[::-1].copy())}, lambda r, b, dec: r.eng.format_f64(b['v']))


# ---- metrics ------------------------------------------------------------------------------------------------------------------
@entry('evaluate', ['mpe_eval_batch'], NONE, 'ground truth and skip as device tensors, which the wrapper takes as they are')
def _evaluate(w):
    import types
    sx, sd = w.scenes()

    def inputs(s):
        poses, flags, _ = s.kinds['triang']
        return {'poses': w.dev(poses), 'flags': w.dev(flags), 'n': w.dev(s.n_persons), 'gt_xyz': w.dev(s.truth.astype(np.float32)),
                'gt_joint': w.dev(s.flags), 'gt_valid': w.dev((s.flags.max(axis=2) > 0).astype(np.uint8)), 'gt_n': w.dev(s.n_persons),
                'skip': w.dev(np.zeros(len(s.n_persons), np.uint8))}

    def run(r, b, dec):
        gt = {'xyz': b['gt_xyz'], 'joint': b['gt_joint'], 'valid': b['gt_valid'], 'n': b['gt_n']}
        return r.eng.evaluate(types.SimpleNamespace(n_frames=int(b['n'].shape[0])), b['poses'], b['flags'], b['n'], gt, 'tri', skip=b['skip'])
    return Case(inputs(sx), inputs(sd), run)


def _scene_case(call, kinds=('triang',)):
    def make(kind):
        def build(w):
            sx, sd = w.scenes()
            same_layout(sx.pb, sd.pb)
            (X, mask), (D, _) = scene_inputs(w, sx, kind), scene_inputs(w, sd, kind)
            return Case(X, D, lambda r, b, dec: call(r, b, kind, mask))
        return build
    return {k: make(k) for k in kinds}


def _args(b):
    return b['db'], b['persons'], b['n'], b['poses'], b['flags']


for _kind, _b in _scene_case(lambda r, b, kind, mask: _reproject(r, b, kind, mask), ('est', 'triang')).items():
    entry('reproject-%s' % _kind, ['mpe_reproject_batch'], NONE)(_b)


def _reproject(r, b, kind, mask):
    with r.on('call'):
        return r.eng.reproject(*_args(b), kind, joint_mask=mask)


@entry('residual_stats', ['mpe_residual_stats'], WRAPPER, 'Engine.residual_stats reads the sums back')
def _residual_stats(w):
    sx, sd = w.scenes()
    res = []
    for s in (sx, sd):
        t, mask = scene_inputs(w, s, 'triang')
        res.append(w.eng.reproject(*_args(t), 'triang', joint_mask=mask).clone())
    return Case({'res': res[0]}, {'res': res[1]}, lambda r, b, dec: r.eng.residual_stats(b['res']))


@entry('partition_labels', ['mpe_partition_labels'], NONE)
def _partition_labels(w):
    sx, sd = w.scenes()
    (X, _), (D, _) = scene_inputs(w, sx, 'triang'), scene_inputs(w, sd, 'triang')
    X, D = ({k: t[k] for k in ('db', 'persons', 'n')} for t in (X, D))
    D['persons'] = D['persons'].flip(1).contiguous()               # (the two scenes name the same heads: the decoy's rows in reverse)
    return Case(X, D, lambda r, b, dec: r.eng.partition_labels(b['db'], b['persons'], b['n'], hcap=2 * r.eng.V))


@entry('group_bodies', ['mpe_group_bodies'], NONE, 'ParsedBodies.packed(): device tensors, taken as they are')
def _group_bodies(w):
    bx, bd = _fixture_bodies(w, 0), _fixture_bodies(w, 4)
    X, D = ({k: v.contiguous() for k, v in pb.packed().items()} for pb in (bx, bd))

    def run(r, b, dec):
        out = r.eng.group_bodies(b)
        return {k: out[k] for k in ('labels', 'n_groups', 'skip', 'status')}
    return Case(X, D, run)


@entry('partition_scores', ['mpe_partition_scores'], NONE)
def _partition_scores(w):
    def inputs(seed):
        rng = np.random.default_rng(seed)
        return {'lt': w.dev(rng.integers(0, 3, (4, 8)).astype(np.int32)), 'lp': w.dev(rng.integers(0, 4, (4, 8)).astype(np.int32)),
                'count': w.dev(np.array([8, 5, 2, 7], np.int32))}
    return Case(inputs(5), inputs(6), lambda r, b, dec: r.eng.partition_scores(b['lt'], b['lp'], b['count']))


# ---- per-batch geometry -------------------------------------------------------------------------------------------------------
for _kind, _b in _scene_case(lambda r, b, kind, mask: r.eng.refine(*_args(b), kind, joint_mask=mask, huber_px=3.0), ('est', 'triang')).items():
    entry('refine-%s' % _kind, ['mpe_refine_batch'], NONE)(_b)
for _kind, _b in _scene_case(lambda r, b, kind, mask: r.eng.pose_covariance(*_args(b), kind, 1.5, joint_mask=mask), ('est', 'triang')).items():
    entry('pose_covariance-%s' % _kind, ['mpe_posecov_batch'], NONE)(_b)
for _kind, _b in _scene_case(lambda r, b, kind, mask: r.eng.regroup(*_args(b), kind, joint_mask=mask), ('est', 'triang')).items():
    entry('regroup-%s' % _kind, ['mpe_regroup_batch'], NONE)(_b)
for _kind, _b in _scene_case(lambda r, b, kind, mask: r.eng.consolidate(*_args(b), kind, joint_mask=mask), ('est', 'triang')).items():
    entry('consolidate-%s' % _kind, ['mpe_consolidate_batch'], NONE)(_b)


def _walk_case(kind, call, fresh=None, read=None, n_frames=None):
    def build(w):
        sx, sd = w.walks()
        same_layout(sx.pb, sd.pb)
        (X, mask), (D, _) = walk_inputs(w, sx, kind), walk_inputs(w, sd, kind)
        return Case(X, D, lambda r, b, dec: call(r, b, dec, kind, mask), fresh=(lambda r: fresh(r, sx, kind)) if fresh else None, read=read)
    return build


def _table(b):
    return b['poses'], b['flags'], b['n'], b['ids']


LAGS = (0, 0.5, -0.25, 1.25, -1.5)                                # refine_timed_cases.LAGS
for _kind in ('est', 'triang'):
    entry('refine_timed-%s' % _kind, ['mpe_refine_timed_batch'], NONE)(
        _walk_case(_kind, lambda r, b, dec, kind, mask: r.eng.refine_timed(b['db'], 0, b['persons'], *_table(b), kind, LAGS, joint_mask=mask)))


def _bone_table(scene, tid_cap, bones):
    """the first frame's bone lengths of the scene's two bodies, by track id"""
    t = np.zeros((tid_cap, len(bones)))
    for row in range(scene.truth.shape[1]):
        tid = int(scene.ids[0, row])
        if tid >= 0:
            for k, (a, c) in enumerate(bones):
                t[tid, k] = np.linalg.norm(scene.truth[0, row, a] - scene.truth[0, row, c])
    return t


def _skeleton(r, kind, pcap=4):
    return r.own(r.eng.skeleton('tri' if kind == 'triang' else 'mlp', bin_mm=2.0, tid_cap=8, pcap=pcap))


def _body_refine_fresh(r, scene, kind):
    r.sk = _skeleton(r, kind)
    r.sk.set_lengths(_bone_table(scene, 8, r.sk.bones) * 1.02)


for _kind in ('est', 'triang'):
    entry('body_refine-%s' % _kind, ['mpe_body_refine_batch'], NONE)(
        _walk_case(_kind, lambda r, b, dec, kind, mask: r.eng.body_refine(r.sk, b['db'], b['persons'], b['n'], b['poses'], b['flags'], b['ids'], sweeps=2,
                                                                         joint_mask=mask), fresh=_body_refine_fresh))


# ---- states: update(D), reset(), update(X), then the read -----------------------------------------------------------------------
def _sequence_case(make, update, read=None, kind='triang', decoy_ids=0):
    """make(r) -> the state object; update(r, t) -> what one update on the tensors t gives; decoy_ids: added to the decoy's
    track ids (a stage whose answer is the ids themselves)."""
    def build(w):
        sx, sd = w.walks()
        (X, _), (D, _) = walk_inputs(w, sx, kind, False), walk_inputs(w, sd, kind, False)
        if decoy_ids:
            D['ids'] = w.dev(np.where(sd.ids >= 0, sd.ids + decoy_ids, -1).astype(np.int32))

        def fresh(r):
            r.obj = r.own(make(r))

        def run(r, b, dec):
            update(r, dec)
            if 'reset' not in r.skip:
                with r.on('reset'):
                    r.obj.reset()
            return update(r, b)
        return Case(X, D, run, fresh=fresh, read=read)
    return build


entry('Tracker.update+reset', ['mpe_track_batch', 'mpe_track_reset'], NONE)(
    _sequence_case(lambda r: r.eng.tracker('tri', max_gap=2, gate=0.5, pcap=4), lambda r, t: r.obj.update(t['poses'], t['flags'], t['n'])))
entry('Smoother.update+reset', ['mpe_smooth_batch', 'mpe_smooth_reset'], NONE)(
    _sequence_case(lambda r: r.eng.smoother('tri', window=3, decay=0.8, pcap=4), lambda r, t: r.obj.update(*_table(t))))


def _skel_update(r, t):
    r.obj.observe(*_table(t))
    r.obj.update(1)
    return r.obj.fit(*_table(t), iters=2)


entry('Skeleton.observe+update+fit+reset+lengths', ['mpe_skel_observe_batch', 'mpe_skel_update', 'mpe_skel_fit_batch', 'mpe_skel_reset',
                                                    'mpe_skel_get_lengths'], NONE)(
    _sequence_case(lambda r: r.eng.skeleton('tri', bin_mm=2.0, tid_cap=8, pcap=4), _skel_update, read=lambda r: r.obj.lengths()))


@entry('Skeleton.set_lengths', ['mpe_skel_set_lengths'], NONE, 'a device table: nothing is uploaded')
def _set_lengths(w):
    sx, sd = w.walks()
    pose, _ = walk_inputs(w, sx, 'triang', False)
    bones = pkg('harness.skeleton').BONES_18

    def fresh(r):
        r.obj = _skeleton(r, 'triang')
        r.obj.set_lengths(_bone_table(sd, 8, bones))

    def run(r, b, dec):
        r.obj.set_lengths(b['table'])
        return r.obj.fit(*_table(pose), iters=2)
    return Case({'table': w.dev(_bone_table(sx, 8, bones) * 1.05)}, {'table': w.dev(_bone_table(sd, 8, bones))}, run, fresh=fresh, read=lambda r: r.obj.lengths())


entry('Relinker.update+reset+counters', ['mpe_relink_batch', 'mpe_relink_reset', 'mpe_relink_read'], NONE)(
    _sequence_case(lambda r: r.eng.relinker('tri', tid_cap=8, pcap=4, max_frames=8), lambda r, t: r.obj.update(*_table(t)), read=lambda r: r.obj.counters(),
                   decoy_ids=2))


@entry('TrackScore.update+reset+result+read_state', ['mpe_track_score_batch', 'mpe_track_score_reset', 'mpe_track_score_result', 'mpe_track_score_read'], NONE)
def _track_score(w):
    import track_score_cases as tsc
    cases = tsc.hand_made()
    cx, cd = cases['exchange'], cases['rows_permuted']
    X, D = ({k: w.dev(v) for k, v in c.arrays().items()} for c in (cx, cd))

    def fresh(r):
        r.obj = r.own(r.eng.track_scorer('mlp', gid_cap=cx.gid_cap, tid_cap=cx.tid_cap, max_frames=8, gcap=cx.cap, pcap=cx.cap))

    def update(r, t):
        ev = {k: t[k] for k in ('assign', 'err', 'invalid', 'n_res', 'n_gt')}
        out = r.obj.update(ev, t['flags'], t['n_persons'], t['track_ids'], t['gt_ids'], t['gt_valid'])
        return {k: out[k] for k in ('frame_counts', 'match_tid')}

    def run(r, b, dec):
        update(r, dec)
        r.obj.reset()
        return update(r, b)
    return Case(X, D, run, fresh=fresh, read=lambda r: (r.obj.result(), r.obj.read_state(), r.obj._status))


def _lm_entries(prefix, name, make, restart):
    """Calibrator / CameraFitter: accumulate + read; reset; set_*; step.  make(r) -> the object; restart(r): its set_* call."""
    def inputs(w):
        sx, sd = w.scenes(6)
        same_layout(sx.pb, sd.pb)
        (X, mask), (D, _) = scene_inputs(w, sx, 'triang'), scene_inputs(w, sd, 'triang')
        return X, D, mask

    def fresh(r):
        r.obj = r.own(make(r))

    def read(r):
        with r.on('read'):
            return r.obj.read()

    def acc_build(w):
        X, D, mask = inputs(w)
        return Case(X, D, lambda r, b, dec: r.obj.accumulate(*_args(b), joint_mask=mask), fresh=fresh, read=read)

    def restart_build(call):
        def build(w):
            X, D, mask = inputs(w)

            def run(r, b, dec):
                r.obj.accumulate(*_args(dec), joint_mask=mask)
                call(r)
                r.obj.accumulate(*_args(b), joint_mask=mask)
            return Case(X, D, run, fresh=fresh, read=read)
        return build

    def step_build(w):
        X, D, mask = inputs(w)

        def step(r):
            rep = r.obj.step()
            return rep, (r.obj.extrinsics() if hasattr(r.obj, 'extrinsics') else r.obj.cameras())
        return Case(X, D, lambda r, b, dec: r.obj.accumulate(*_args(b), joint_mask=mask), fresh=fresh, read=step)
    entry(name + '.accumulate+read', [prefix + '_batch', prefix + '_read'], NONE)(acc_build)
    entry(name + '.reset', [prefix + '_reset'], EITHER, 'accumulate(D), reset(), accumulate(X), read()')(restart_build(lambda r: r.obj.reset()))
    entry(name + '.' + restart.__name__, [prefix + '_' + restart.__name__], EITHER, 'accumulate(D), the call, accumulate(X), read()')(restart_build(restart))
    entry(name + '.step', [prefix + '_step'], NONE, 'accumulate(X), then step(): it synchronises `stream` and reads the sums')(step_build)


def set_extrinsics(r):
    import calib_cases as cc
    E = cc.CB().start_extrinsics(r.eng.calib)
    r.obj.set_extrinsics(cc.perturbed_start(E, 0.2, 3.0, 91))


def set_cameras(r):
    import calib_cases as cc
    (E, k, dist), _ = r.obj.cameras()
    r.obj.set_cameras(cc.perturbed_start(E, 0.2, 3.0, 91), k * np.float32(1.001), dist)


_lm_entries('mpe_calib', 'Calibrator', lambda r: r.eng.calibrator('triang', min_obs=6), set_extrinsics)
_lm_entries('mpe_camfit', 'CameraFitter', lambda r: r.eng.camera_fitter('triang', min_obs=13), set_cameras)


def _lag_entries():
    def inputs(w):
        sx, sd = w.walks()
        same_layout(sx.pb, sd.pb)
        (X, mask), (D, _) = walk_inputs(w, sx, 'triang'), walk_inputs(w, sd, 'triang')
        return X, D, mask

    def fresh(r):
        r.obj = r.own(r.eng.lag_estimator('triang', window=2, sub=2, pcap=4, max_frames=8))

    def acc(r, t, mask):
        r.obj.accumulate(t['db'], 0, t['persons'], *_table(t), joint_mask=mask)

    def acc_build(w):
        X, D, mask = inputs(w)
        return Case(X, D, lambda r, b, dec: acc(r, b, mask), fresh=fresh, read=lambda r: r.obj.read())

    def reset_build(w):
        X, D, mask = inputs(w)

        def run(r, b, dec):
            acc(r, dec, mask)
            r.obj.reset()
            acc(r, b, mask)
        return Case(X, D, run, fresh=fresh, read=lambda r: r.obj.read())

    def estimate_build(w):
        X, D, mask = inputs(w)
        return Case(X, D, lambda r, b, dec: acc(r, b, mask), fresh=fresh, read=lambda r: r.obj.estimate(min_obs=1))
    entry('LagEstimator.accumulate+read', ['mpe_lag_batch', 'mpe_lag_read'], NONE)(acc_build)
    entry('LagEstimator.reset', ['mpe_lag_reset'], NONE, 'stream-ordered memsets: accumulate(D), reset(), accumulate(X), read()')(reset_build)
    entry('LagEstimator.estimate', ['mpe_lag_estimate'], NONE, 'accumulate(X), then estimate(): it synchronises `stream`')(estimate_build)


_lag_entries()

# the three controls of tests/test_gpu_streams.py: (entry, the label of the call that is misplaced)
CONTROLS = {'kernel': ('reproject-triang', 'call'), 'reset': ('Tracker.update+reset', 'reset'), 'read': ('Calibrator.accumulate+read', 'read')}
