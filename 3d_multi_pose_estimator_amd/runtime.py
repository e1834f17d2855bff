"""Process-wide engines for the per-frame API mirrors (gat2.GAT2, graph_generator.*, ...).

The reference's symbols work on one frame per call; here each call becomes a 1-frame batch
through the same C-ABI entry points the batched engine uses.  Engines without weights
(clustering, featurisation, triangulation) are shared; GAT2 / PoseEstimatorMLP instances own
theirs because weights are frozen into a context's padded device copies.
"""
import os
import threading

import numpy as np

_shared = {}


class ParamWatch:
    """(data_ptr, version) of every parameter of a module tree, without walking the tree per call (0.13 ms per forward in the
    one-frame-per-call loop) and without trusting that the tree never changes: the walk's result is kept, and every call checks
    with plain dict lookups that it still describes the tree -- every module still sits under its parent's name, every parameter
    still IS the object registered under its owner's name, no module gained or lost a child or a parameter.  A swapped submodule,
    `layer.fc1.weight = nn.Parameter(...)`, a pruning re-parametrisation or `register_parameter` rebuilds the snapshot; an
    in-place update or a `.to()` changes the tuple as before."""

    def __init__(self, root):
        self.root = root
        self.links = None        # (parent, name, child, n_children of child, n_parameters of child)
        self.slots = None        # (owner, name, parameter)

    def _rebuild(self):
        self.links, self.slots = [], []
        stack = [self.root]
        self.root_counts = (len(self.root._modules), len(self.root._parameters))
        while stack:
            mod = stack.pop()
            for name, p in mod._parameters.items():
                if p is not None:
                    self.slots.append((mod, name, p))
            for name, child in mod._modules.items():
                if child is not None:
                    self.links.append((mod, name, child, len(child._modules), len(child._parameters)))
                    stack.append(child)

    def _valid(self):
        if (len(self.root._modules), len(self.root._parameters)) != self.root_counts:
            return False
        for parent, name, child, n_mod, n_par in self.links:
            if parent._modules.get(name) is not child or len(child._modules) != n_mod or len(child._parameters) != n_par:
                return False
        for owner, name, p in self.slots:
            if owner._parameters.get(name) is not p:
                return False
        return True

    def version(self):
        if self.links is None or not self._valid():
            self._rebuild()
        return tuple((p.data_ptr(), p._version) for _, _, p in self.slots)


def max_persons_per_camera():
    return int(os.environ.get('MPE_MAX_PERSONS_PER_CAMERA', '10'))


def device():
    return os.environ.get('MPE_DEVICE', 'cuda:0')


def new_engine(params=None, calib=None, max_frames=1):
    from .parameters import parameters as default_params
    from .pipeline import Engine, explicit_m_cap
    p = params or default_params
    hpf = len(p.used_cameras_skeleton_matching) * max_persons_per_camera()
    # the mirrors also take the graphs of mode='test_generated' (explicit edge-node lists: up to explicit_m_cap per graph)
    eng = Engine(params, calib, max_frames=max_frames, max_persons_per_camera=max_persons_per_camera(),
                 device=device(), max_edge_nodes_per_frame=explicit_m_cap(hpf) or None)
    # opt-ins for callers of the mirrors, who have no Engine to call set_precision on.  MPE_GAT_ACC64=1: f64 running sums in EVERY GAT GEMM
    # (scores then sit closer to the float64 network than the reference's own fp32 evaluation on every frame measured,
    # profiles/r06_shape_fuzz_seeds.txt; the matching network's GEMMs take ~10 % longer and small batches leave the latency launches for the
    # batch path's kernels).  MPE_MLP_PRECISION=max_accuracy | f64: the MLP with an f64 flush per K stage (mode 4) or evaluated on the f64
    # matrix pipe (mode 5: every output of every golden row bit-equal to the network evaluated in f64; several times slower).
    acc, mlp = os.environ.get('MPE_GAT_ACC64', '0') == '1', os.environ.get('MPE_MLP_PRECISION', '')
    if mlp not in ('', 'default', 'max_accuracy', 'f64'):
        raise ValueError("MPE_MLP_PRECISION must be 'max_accuracy' or 'f64' (or unset), not %r" % mlp)
    if acc or mlp in ('max_accuracy', 'f64'):
        eng.set_precision(gat_acc64=acc, mlp_max_accuracy=mlp == 'max_accuracy', mlp_f64=mlp == 'f64')
    return eng


def shared_engine(params=None, calib=None, max_frames=1):
    """Weight-less engine keyed by the calibration it was built from; rebuilt larger when a batch of graphs needs more
    frames than it has."""
    key = 'default' if calib is None else _calib_key(calib)
    if key in _shared and _shared[key].max_frames < max_frames:
        _shared.pop(key).close()
    if key not in _shared:
        _shared[key] = new_engine(params, calib, max_frames=max(1, int(max_frames)))
    return _shared[key]


def _calib_key(calib):
    return hash((calib.K32.tobytes(), calib.dist.tobytes(), calib.P.tobytes(), calib.T_i32.tobytes()))


def calibration_from_dicts(params, camera_matrices, distortion_coefficients, projection_matrices):
    """Calibration object from the explicit dicts `triangulate` receives
    (reference pose_estimator_utils.py:52)."""
    from .calibration import Calibration, TransformManager
    names = list(params.camera_names)
    tm = TransformManager()
    for c in names:
        T = np.eye(4)
        T[0:3, :] = np.asarray(projection_matrices[c], np.float64)
        tm.add_transform('root', c, T)
    cal = Calibration(params, tm)
    for i, c in enumerate(names):
        cal.K32[i] = np.asarray(camera_matrices[c], np.float32)
        cal.dist[i] = np.asarray(distortion_coefficients[c], np.float64)
        cal.P[i] = np.asarray(projection_matrices[c], np.float64)
    return cal


# ---- MLP input rows of a frame's persons, computed in ONE launch --------------------------------------------------------
# The reference's caller builds one PoseEstimatorDataset per PERSON (metrics_from_model.py:243-277), each from the JSON text
# of that person's skeletons.  get_person_proposal_from_network_output (the call right before, :214) knows all persons of the
# frame and has the frame's arrays on the device, so it computes every person's row with one mpe_mlp_input_rows launch and
# leaves them here, keyed by exactly the strings the caller is about to hand to PoseEstimatorDataset
# (json.dumps([jsons_for_head[head]]) per camera, :250-252).  A row is a pure function of those strings and the
# calibration, and the key holds both BY CONTENT (the calibration as the hash of its arrays, not the object's id, which
# CPython may hand to another calibration later), so an entry cannot be stale; PoseEstimatorDataset falls back to its
# own launch on a miss.
# MPE_DROPIN_PREFETCH=0 switches the prefetch off.
_ROW_CACHE_CAP = 64


class _RecentRows:
    """The rows of the last few frames' persons, newest first, found by COMPARING the key strings (a mismatch shows within the first
    bytes, a match costs one memcmp): hashing ~1 KB of JSON text per skeleton, once here and once for the caller's copy of the same
    text, cost more per frame than the lookup it was meant to speed up."""

    def __init__(self):
        from collections import deque
        self.items = deque(maxlen=_ROW_CACHE_CAP)

    def put(self, engine_key, key, row, valid):
        self.items.appendleft((engine_key, key, row, valid))

    def get(self, engine_key, key):
        for ek, k, row, valid in self.items:
            if ek == engine_key and k == key:
                return row, valid
        return None

    def clear(self):
        self.items.clear()

    def __len__(self):
        return len(self.items)


_row_cache = _RecentRows()


def prefetch_enabled():
    return os.environ.get('MPE_DROPIN_PREFETCH', '1') != '0'


def prefetch_mlp_rows(eng, db, persons, n_persons, rows, jsons_for_head, cams, launched=None):
    """rows: the frame's persons as lists of head ids per camera of `cams` (-1 = none).  launched: (rows, valid) device tensors
    of an mpe_mlp_input_rows launch the caller has already queued behind the clustering (one synchronisation for both)."""
    import json
    used = [c for c in eng.params.used_cameras]
    r, valid = launched if launched is not None else eng.mlp_input_rows(db, persons, n_persons)
    n = len(rows)
    r, valid = r[0, :n].cpu(), valid[0, :n].cpu()
    text_of = getattr(jsons_for_head, 'json_text', None)

    def text(h):
        t = text_of(h) if text_of is not None else None
        return t if t is not None else json.dumps([jsons_for_head[h]])
    for p, row in enumerate(rows):
        key = tuple((cam, text(row[cams.index(cam)])) for cam in used if cam in cams and row[cams.index(cam)] >= 0)
        _row_cache.put(_engine_key(eng), key, r[p].clone(), bool(valid[p]))


# ---- the caller's next two steps, queued behind the scores ---------------------------------------------------------------
# The reference's per-frame caller goes from GAT2.__call__ straight to get_person_proposal_from_network_output and from there to one
# PoseEstimatorDataset per person (metrics_from_model.py:206-277).  Done step by step each of those is a chain of its own on an idle
# GPU: an index upload that waits for the scores, a gather, the clustering launch, the row launch, three copies back.  GAT2.forward
# therefore queues clustering + row assembly on its own engine (whose topology tables already describe the frame) right behind the
# scores, into a small ring of preallocated buffers, with ONE copy back into page-locked memory; the proposal function then only
# waits and reads.  Nothing is assumed about what the caller does next: the result is used only when the proposal function is handed
# the very tensor forward returned (same storage, unmodified), the graph's own edge-node ids and the threshold the clustering ran
# with; anything else takes the step-by-step route.  MPE_DROPIN_PREFETCH=0 switches this off together with the row prefetch.
_AHEAD_RING = 4


class _AheadSlot:
    def __init__(self, eng):
        import torch
        pcap, V = eng.pcap, eng.V
        width = eng.V * eng.J * eng.params.numbers_per_joint
        self.ld = (width + 127) // 128 * 128
        self.width = width
        o_n, o_p = 0, 256
        o_v = o_p + (pcap * V * 4 + 255) // 256 * 256
        o_r = o_v + (pcap + 255) // 256 * 256
        nbytes = o_r + pcap * self.ld * 4
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        base = self.dev.data_ptr()
        self.p_n, self.p_persons, self.p_valid, self.p_rows = base + o_n, base + o_p, base + o_v, base + o_r
        h = self.host.numpy()
        self.h_n = h[o_n:o_n + 4].view(np.int32)
        self.h_persons = h[o_p:o_p + pcap * V * 4].view(np.int32).reshape(pcap, V)
        self.h_valid = h[o_v:o_v + pcap]
        self.h_rows = h[o_r:o_r + pcap * self.ld * 4].view(np.float32).reshape(pcap, self.ld)
        self.gen = 0
        self.stream = None


class FrameAhead:
    """Clustering + MLP input rows of one frame, queued by GAT2.forward behind the scores it returned."""
    __slots__ = ('out', 'version', 'threshold', 'engine', 'slot', 'gen', 'db', 'stream')

    def matches(self, outputs, threshold):
        import torch
        out = self.out
        if not getattr(self.engine, 'ctx', None):          # the matcher has replaced its engine since (new weights): nothing to wait on
            return False
        if self.stream != self.engine._stream().value:
            # queued on another stream than the caller is on now (GAT2.forward under `with torch.cuda.stream(s)`, the proposals asked
            # for outside it): the step-by-step route answers, on the caller's stream.  That stream is ordered behind neither the
            # slot's copy nor the scores themselves, so the chain is waited for first: the status read-back is its last link, and
            # status_wait synchronises the stream it was queued on (it raises what that read-back saw, as take_proposals would).
            self.engine.status_wait()
            return False
        return (isinstance(outputs, torch.Tensor) and outputs.data_ptr() == out.data_ptr() and outputs.numel() == out.numel()
                and outputs.dtype == out.dtype and outputs._version == self.version and float(threshold) == self.threshold
                and self.slot.gen == self.gen)


def queue_proposals(eng, db, scores, out):
    """-> FrameAhead, or None where the frame cannot go this way."""
    import ctypes as C

    import torch
    if db.n_frames != 1 or db.n_edge_nodes < 1 or getattr(db.host, 'en_pair', None) is not None:
        return None
    ring = eng.__dict__.get('_ahead_ring')
    if ring is None:
        ring = eng.__dict__['_ahead_ring'] = [[_AheadSlot(eng) for _ in range(_AHEAD_RING)], 0]
    slot = ring[0][ring[1] % _AHEAD_RING]
    ring[1] += 1
    stream = eng._stream()
    if slot.stream is not None and slot.stream != stream.value:
        torch.cuda.synchronize(eng.device)        # the slot's last copy was ordered on another stream
    slot.stream = stream.value
    slot.gen += 1
    lib, st = eng.lib, C.byref(db.struct)
    eng._chk(lib.mpe_cluster_batch(eng.ctx, stream, st, C.c_void_p(scores.data_ptr()), C.c_void_p(slot.p_persons), C.c_void_p(slot.p_n)))
    eng._chk(lib.mpe_mlp_input_rows(eng.ctx, stream, st, C.c_void_p(slot.p_persons), C.c_void_p(slot.p_n), C.c_void_p(slot.p_rows), slot.ld,
                                    C.c_void_p(slot.p_valid)))
    slot.host.copy_(slot.dev, non_blocking=True)
    eng._chk(lib.mpe_status_queue(eng.ctx, stream))       # the status word travels with the results: take_proposals only waits
    ah = FrameAhead()
    ah.out, ah.version, ah.engine, ah.slot, ah.gen, ah.db = out, out._version, eng, slot, slot.gen, db
    ah.threshold = float(eng._state.get('threshold', eng._made_with['threshold']))
    ah.stream = stream.value
    return ah


# ---- ... and the scores themselves, queued behind the frame's arrays ---------------------------------------------------------
# One step further back: a frame dict handed to MergedMultipleHumansDataset(mode='test') is scored next by the matcher the caller
# built once (metrics_from_model.py:73-100, 199-209).  The dataset therefore queues the matcher's launches (and, behind them, the
# proposals above) on the engine of the GAT2 mirror that scored the previous frame, as soon as the frame's arrays exist: the chain
# of ~20 dependent launches (0.2 ms on the device) then runs while the caller is still unpacking the dataset object, instead of
# being waited for inside get_person_proposal_from_network_output.  GAT2.forward hands the queued scores out only if it is that
# very engine (same weights: a changed parameter makes GAT2 build a new engine), the same output activation, the same stream,
# the graph's own features; everything else is computed as before.  A frame nobody scores costs idle GPU time, nothing else.
# The hint is kept PER THREAD: a context belongs to one host thread at a time, so a dataset built on one thread
# never enters the engine another thread's matcher noted.
_matcher_hint = threading.local()


class FrameScores:
    __slots__ = ('engine', 'out', 'version', 'sigmoid', 'stream', 'ahead')


def note_matcher(eng):
    import weakref
    ref = getattr(_matcher_hint, 'ref', None)
    if ref is None or ref() is not eng:
        _matcher_hint.ref = weakref.ref(eng)


def start_frame(graph):
    """Queue scoring + proposals of a one-frame graph on the engine of the last matcher THIS thread ran.  A frame the engine has no
    room for (ValueError from check_capacity) is declined here and reported where the step-by-step route reports it; any other
    failure (an MpeError from a launch, a bug) propagates."""
    ref = getattr(_matcher_hint, 'ref', None)
    if ref is None or not prefetch_enabled():
        return
    eng = ref()
    try:
        if eng is None or not getattr(eng, 'ctx', None) or graph.batch_size != 1 or graph.M < 1 or getattr(graph.packed, 'en_pair', None) is not None:
            return
        db = graph.device_batch(eng)
        out, sc = eng.gat_scores_joined(db)
        fs = FrameScores()
        fs.out = out.reshape(-1, 1, 1)
        fs.engine, fs.version, fs.sigmoid, fs.stream = eng, fs.out._version, bool(eng._state.get('gat_output', True)), eng._stream().value
        fs.ahead = queue_proposals(eng, db, sc, fs.out)
        graph.__dict__['_scored'] = fs
    except ValueError:
        graph.__dict__.pop('_scored', None)


def queued_scores(graph, eng, sigmoid):
    """The scores start_frame queued for this graph on this engine, or None."""
    fs = graph.__dict__.get('_scored')
    if fs is None or fs.engine is not eng or fs.sigmoid != bool(sigmoid) or fs.out._version != fs.version or fs.stream != eng._stream().value:
        return None
    return fs


def take_proposals(ah, jsons_for_head, cams):
    """Wait for what queue_proposals queued -> the persons as lists of head ids per camera of `cams` (-1 = none); their MLP input rows
    go into the row cache under the keys PoseEstimatorDataset will ask with (prefetch_mlp_rows)."""
    import json

    import torch
    eng, slot = ah.engine, ah.slot
    eng.status_wait()
    if slot.gen != ah.gen:
        return None
    n = int(slot.h_n[0])
    rows = slot.h_persons[:n].tolist()
    if jsons_for_head is not None and n:
        used = [(c, cams.index(c)) for c in eng.params.used_cameras if c in cams]
        text_of = getattr(jsons_for_head, 'json_text', None)
        ek = _engine_key(eng)
        data = torch.from_numpy(slot.h_rows[:n, :slot.width].copy())
        ok = slot.h_valid[:n].tolist()
        put = _row_cache.put
        for p, row in enumerate(rows):
            key = []
            for cam, c in used:
                h = row[c]
                if h >= 0:
                    t = text_of(h) if text_of is not None else None
                    key.append((cam, t if t is not None else json.dumps([jsons_for_head[h]])))
            put(ek, tuple(key), data[p], ok[p] != 0)
    return rows


def cached_mlp_row(eng, key):
    return _row_cache.get(_engine_key(eng), key)


def _engine_key(eng):
    k = getattr(eng, '_calib_content_key', None)
    if k is None:
        k = eng._calib_content_key = _calib_key(eng.calib)
    return k
