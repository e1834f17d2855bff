"""Batched engine over libmpe_hip.so: the frame-batched form of the reference's per-frame
loop body (test/metrics_from_model.py:178-294, test/metrics_from_triangulation.py:187-272).

PyTorch is plumbing here (device memory, current stream); every computation on the path is
a HIP kernel behind the C ABI of include/mpe.h.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import lib as L
from .calibration import Calibration
from .logtable import DEVICE_ENTRIES, log_table
from .packing import (CapacityArena, DeviceBatch, JsonIndex, JsonStage, NeedsHostParser, PackedBatch, ParsedBodies, ParsedOnDevice,
                      pack_frames, pack_json, pack_json_into, stage_gt_window, stage_json_window)


def _f32p(a):
    return a.ctypes.data_as(L.c_f32p)


class Engine:
    def __init__(self, params=None, calib=None, max_frames=1024, max_heads_per_frame=None,
                 max_persons_per_camera=4, device='cuda:0', threshold=0.5, max_edge_nodes_per_frame=None):
        from .parameters import parameters as default_params
        self.params = params or default_params
        self.calib = calib or Calibration(self.params)
        self.lib = L.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('Engine needs a GPU device (there is no CPU fallback)')
        torch.cuda.set_device(self.device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        p = self.params
        sm = list(p.used_cameras_skeleton_matching)
        if sm != list(p.used_cameras) or sm != [c for c in p.camera_names if c in sm]:
            raise ValueError('used_cameras_skeleton_matching must equal used_cameras in camera_names order')
        self.V, self.J = len(sm), len(p.joint_list)
        cal_idx = [self.calib.index(c) for c in sm]
        hpf = max_heads_per_frame or self.V * max_persons_per_camera
        self.max_frames = int(max_frames)
        self.hpf = int(hpf)
        self.pcap = max(1, hpf // max(1, p.min_number_of_views))
        # largest edge-node count of a frame with `hpf` heads (even spread over V cameras)
        m_frame = hpf * hpf * (self.V - 1) // (2 * self.V) + 1
        # batches with an explicit edge-node list (process_training graphs: one edge-node per ORDERED head pair) hold up to
        # explicit_m_cap(hpf) edge-nodes per frame; `max_edge_nodes_per_frame` sizes the batch totals for them
        if max_edge_nodes_per_frame:
            m_frame = max(m_frame, int(max_edge_nodes_per_frame))
        self._keep = {
            'Kinv': np.ascontiguousarray(self.calib.Kinv32[cal_idx].reshape(-1), np.float32),
            'K': np.ascontiguousarray(self.calib.K32[cal_idx].reshape(-1), np.float32),
            'T_i': np.ascontiguousarray(self.calib.T_i32[cal_idx].reshape(-1), np.float32),
            'P': np.ascontiguousarray(self.calib.P[cal_idx].reshape(-1), np.float64),
            'dist': np.ascontiguousarray(self.calib.dist[cal_idx].reshape(-1), np.float64),
        }
        cfg = L.mpe_config()
        cfg.n_cameras, cfg.n_joints = self.V, self.J
        cfg.image_width, cfg.image_height = p.image_width, p.image_height
        cfg.numbers_per_joint = p.numbers_per_joint
        cfg.min_views = p.min_number_of_views
        cfg.median_axis = p.axes_3D['Y'][0]
        cfg.used_joint_mask = sum(1 << j for j in p.used_joints)
        cfg.threshold = threshold
        cfg.median_window = 0.05
        cfg.max_frames = self.max_frames
        cfg.max_heads = self.max_frames * hpf
        cfg.max_edge_nodes = self.max_frames * m_frame
        cfg.max_heads_per_frame = hpf
        cfg.max_persons_per_frame = self.pcap
        cfg.Kinv = _f32p(self._keep['Kinv'])
        cfg.K = _f32p(self._keep['K'])
        cfg.T_i = _f32p(self._keep['T_i'])
        cfg.P = self._keep['P'].ctypes.data_as(L.c_f64p)
        cfg.dist = self._keep['dist'].ctypes.data_as(L.c_f64p)
        self.ctx = C.c_void_p()
        rc = self.lib.mpe_create(C.byref(cfg), C.byref(self.ctx))
        if rc != 0:
            raise L.MpeError(rc, 'mpe_create failed')
        self.gat_dims = None
        self.mlp_out = None
        self.m_frame = m_frame
        self._made_with = dict(params=self.params, calib=self.calib, max_frames=self.max_frames, max_heads_per_frame=self.hpf,
                               max_persons_per_camera=max_persons_per_camera, device=str(self.device), threshold=threshold,
                               max_edge_nodes_per_frame=max_edge_nodes_per_frame)
        self._state = {}                 # what was loaded / set, so that sibling() can repeat it
        self._siblings = []
        self._json_streams = None
        self._gt_bufs = None             # staging buffers of bodies_from_json, kept between calls
        self._log_table_set = False      # partition_scores hands the table of logarithms to the context at its first call
        if os.environ.get('MPE_JSON_STREAMS_EARLY', '0') == '1':           # diagnostics (see _make_json_streams)
            self._make_json_streams()

    def _make_json_streams(self):
        """The three streams of the JSON pipeline (parse; matching / 3D compute), made at the first stream_json call.
        Compute at high priority, parse at normal: the parse kernels of window i+1 take the slots the GEMMs of window i
        leave.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); with the 6-9 streams of
        an application that also pipelines its copies, the parse stream and the compute stream can land on one queue
        and then serialise (measured inside bench.py: 145-159 k or 171 k frames/s depending on the order in which streams
        were first used).  With 8 hardware queues (GPU_MAX_HW_QUEUES=8 before HIP initialises: bench.py sets it for itself, lib.py on
        import when MPE_SET_HW_QUEUES=1 asks for it): 170.5-170.7 k in 5 of 5 runs."""
        if self._json_streams is None:
            self._json_streams = (torch.cuda.Stream(self.device, priority=int(os.environ.get('MPE_JSON_PARSE_PRIO', '0'))),
                                  torch.cuda.Stream(self.device, priority=int(os.environ.get('MPE_JSON_COMPUTE_PRIO', '-1'))),
                                  torch.cuda.Stream(self.device, priority=int(os.environ.get('MPE_JSON_COMPUTE_PRIO', '-1'))))
            for s_ in self._json_streams:
                with torch.cuda.stream(s_):
                    torch.zeros(8, device=self.device).add_(1)
        return self._json_streams

    def close(self):
        for e in getattr(self, '_siblings', []):
            e.close()
        self._siblings = []
        if getattr(self, 'ctx', None):
            self.lib.mpe_destroy(self.ctx)
            self.ctx = None

    def sibling(self, k=1):
        """The k-th further context with the same configuration, weights, precision mode and threshold (own workspace,
        124 MB of weights again).  A context is one dependent chain of ~45 kernels per batch; two contexts that take
        turns on the batches (run_pipelined(contexts=2), stream_json(contexts=2), bench.py) keep two such chains in
        flight and fill each other's launch tails: 195.6 k against 186-189 k frames/s for one context with its two stages
        on two streams (tools/two_engines.py, MPE_ALTERNATE=1).  Results are bit-identical: same kernels, same data."""
        while len(self._siblings) < k:
            e = Engine(**self._made_with)
            st = self._state
            if 'gat' in st:
                e.load_gat(*st['gat'])
            if 'mlp' in st:
                e.load_mlp(*st['mlp'])
            if 'precision' in st:
                e.set_precision(*st['precision'])
            if 'threshold' in st:
                e.set_threshold(st['threshold'])
            if 'gat_output' in st:
                e.set_gat_output(st['gat_output'])
            self._siblings.append(e)
        return self._siblings[k - 1]

    def contexts(self, n):
        """[self, sibling(1), ..., sibling(n - 1)]"""
        return [self] + [self.sibling(k) for k in range(1, int(n))]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----------------------------------------------------------------------
    def _chk(self, rc):
        L.check(self.ctx, rc)

    def load_gat(self, state_dict, prm):
        """state_dict: reference names ``layers.{l}.{fc1,fc2}.{weight,bias}``, ``attn_l/r``
        (numpy or torch); prm: contents of skeleton_matching.prms."""
        sd = {k: _np32(v) for k, v in state_dict.items()}
        self._state['gat'] = (sd, prm)
        for e in self._siblings:
            e.load_gat(sd, prm)
        n_layers = int(prm['gnn_layers'])
        heads = list(prm['heads']) + [1]
        slope = prm.get('nonlinearity', 0.01)
        slope = getattr(slope, 'negative_slope', slope)
        self._chk(self.lib.mpe_set_gat_params(self.ctx, n_layers, float(prm['alpha']), float(slope)))
        dims = []
        for l in range(n_layers):
            w1 = sd['layers.%d.fc1.weight' % l]
            w2 = sd['layers.%d.fc2.weight' % l]
            in_dim, nh = w1.shape[1], heads[l]
            out_dim = w2.shape[0] // nh
            al = np.ascontiguousarray(sd['layers.%d.attn_l' % l].reshape(nh, out_dim))
            ar = np.ascontiguousarray(sd['layers.%d.attn_r' % l].reshape(nh, out_dim))
            self._chk(self.lib.mpe_set_gat_layer(
                self.ctx, l, in_dim, nh, out_dim, _f32p(w1), _f32p(sd['layers.%d.fc1.bias' % l]),
                _f32p(w2), _f32p(sd['layers.%d.fc2.bias' % l]), _f32p(al), _f32p(ar)))
            dims.append((in_dim, nh, out_dim))
        self.gat_dims = dims

    def load_mlp(self, state_dict, slope=0.1):
        sd = {k: _np32(v) for k, v in state_dict.items()}
        self._state['mlp'] = (sd, slope)
        for e in self._siblings:
            e.load_mlp(sd, slope)
        keys = sorted({int(k.split('.')[1]) for k in sd})
        self._chk(self.lib.mpe_set_mlp_params(self.ctx, len(keys), float(slope)))
        for n, k in enumerate(keys):
            w = sd['layers.%d.weight' % k]
            self._chk(self.lib.mpe_set_mlp_layer(self.ctx, n, w.shape[1], w.shape[0], _f32p(w),
                                                 _f32p(sd['layers.%d.bias' % k])))
            self.mlp_out = w.shape[0]

    # ---- batches ----------------------------------------------------------------------
    def pack(self, frames, keep_json=False):
        return pack_frames(frames, self.params, keep_json=keep_json)

    def pack_json(self, text, frame_start=0, frame_step=1, max_frames=0, n_threads=0):
        """Native (C++) packer: JSON text of a list of frames -> PackedBatch."""
        return pack_json(text, self.params, frame_start, frame_step, max_frames, n_threads)

    def stream_json(self, text, chunk_frames=None, mode='mlp', frame_step=1, n_threads=0, parser='device', contexts=1, matcher='gat',
                    geom=None):
        """Frame JSON (bytes, the reference's wire format) -> 3D poses, chunk by chunk, with the
        host side off the critical path: the native packer parses chunk i+1 straight into a
        page-locked arena (worker thread; the C call releases the GIL) while chunk i is copied to
        the device in ONE transfer and runs mpe_match_batch + the 3D stage; results come back into
        page-locked memory.  Yields (PackedBatch view, poses [B,Pcap,J,3], n_persons [B]) per chunk.
        LIFETIME: the yielded view and arrays are valid until the next `next()` on the generator only (with contexts = 2
        there are four buffer sets instead of two and two windows in flight; the rule is the same) --
        resuming it starts the parse of a later chunk into the arena behind the view (two host arenas)
        and the result arrays of the slot are rewritten one chunk after that.  With the device parser the
        page-locked result buffers belong to the ENGINE (kept across calls: pinning them costs more than a
        window), so arrays from an earlier call are rewritten by the next call as well.  Copy what you keep.

        parser = 'device' (default): the host keeps the first level of the format only (frame extents, camera
        keys, the extent of every skeleton STRING: stage_json_window) and the strings are parsed ON THE DEVICE
        (csrc/jsonparse.hip) on a side stream while the previous chunk computes; the first element yielded is
        then a ParsedOnDevice (n_frames, n_heads, ...; `.download()` for the arrays; a window that fell back to the host
        packer yields a PackedBatch there instead -- both carry n_frames / n_heads / n_edge_nodes / frame_counts-style
        offsets, test with isinstance if you need the host arrays).  A chunk holding a shape
        the device parser leaves to the host (literals, nested values, numbers beyond the exact fast path)
        is packed by the host packer instead -- same arrays either way.  parser = 'host': the round-2 path.
        contexts = 2 (device parser only): windows take turns on two contexts (sibling()), two windows in flight.
        matcher = 'geometric': geom_match (options in the dict `geom`) in the place of match; no GAT weights are needed."""
        from concurrent.futures import ThreadPoolExecutor
        match_stage = self._match_stage(matcher, geom)
        if isinstance(text, str):
            text = text.encode()
        B = int(chunk_frames or self.max_frames)
        if B > self.max_frames:
            raise ValueError('chunk of %d frames exceeds max_frames=%d' % (B, self.max_frames))
        if int(contexts) not in (1, 2):
            raise ValueError('stream_json takes contexts = 1 or 2 (two compute streams exist; more contexts measured slower, DESIGN 7.1)')
        if parser == 'device':
            # the page-locked result buffers, the arenas and the streams of the device parser belong to the ENGINE: a second
            # generator running on it at the same time would overwrite the first one's results
            if getattr(self, '_json_busy', False):
                raise RuntimeError('another stream_json(parser="device") generator is still open on this engine; exhaust or close() it '
                                   'first, or use a second Engine / Engine.sibling()')
            self._json_busy = True
            try:
                yield from self._stream_json_device(text, B, mode, frame_step, n_threads, contexts, match_stage)
            finally:
                self._json_busy = False
            return
        H = B * self.hpf
        host = [CapacityArena(self.V, self.J, B, H, 'pinned') for _ in range(2)]
        dev = [CapacityArena(self.V, self.J, B, H, self.device) for _ in range(2)]
        dbs = [None, None]
        out_dt = torch.float32 if mode == 'mlp' else torch.float64
        out = [(torch.empty((B, self.pcap, self.J, 3), dtype=out_dt).pin_memory(),
                torch.empty((B,), dtype=torch.int32).pin_memory()) for _ in range(2)]
        uploaded = [torch.cuda.Event() for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        pool = ThreadPoolExecutor(1)
        index = JsonIndex(text)                 # the document is scanned once, window by window

        def parse(i):
            return pack_json_into(index, self.params, host[i & 1], frame_start=i * B * frame_step, frame_step=frame_step,
                                  max_frames=B, n_threads=n_threads)
        try:
            fut = pool.submit(parse, 0)
            i = 0
            pending = None                                  # (slot, pb) whose results are still in flight
            while True:
                pb = fut.result()
                if pb.n_frames == 0:
                    break
                k = i & 1
                self.check_capacity(pb)
                # arrays of the views are exact-size; keep a private copy of the offsets the caller may read
                if dbs[k] is None:
                    dbs[k] = DeviceBatch(pb, self.device, arena=dev[k])
                db = dbs[k].rebind(pb)
                dev[k].buf.copy_(host[k].buf, non_blocking=True)
                uploaded[k].record()
                _, persons, n_persons = match_stage(self, db)
                poses = (self.mlp3d(db, persons, n_persons) if mode == 'mlp' else self.triangulate(db, persons, n_persons))[0]
                out[k][0][:pb.n_frames].copy_(poses, non_blocking=True)
                out[k][1][:pb.n_frames].copy_(n_persons, non_blocking=True)
                done[k].record()
                last = pb.n_frames < B
                if pending is not None:
                    pk, ppb = pending
                    done[pk].synchronize()
                    yield ppb, out[pk][0][:ppb.n_frames].numpy(), out[pk][1][:ppb.n_frames].numpy()
                pending = (k, pb)
                if last:
                    break
                # the other host arena may be parsed into again once ITS upload has completed
                # (that was chunk i-1, whose results were just handed out)
                fut = pool.submit(parse, i + 1)
                i += 1
            if pending is not None:
                pk, ppb = pending
                done[pk].synchronize()
                yield ppb, out[pk][0][:ppb.n_frames].numpy(), out[pk][1][:ppb.n_frames].numpy()
        finally:
            pool.shutdown(wait=True)
            index.close()

    def _stream_json_device(self, text, B, mode, frame_step, n_threads, contexts=1, match_stage=None):
        from concurrent.futures import ThreadPoolExecutor
        import os
        import time
        t_call = time.perf_counter()
        match_stage = match_stage or self._match_stage('gat', None)
        H = B * self.hpf
        # page-locked staging, the device arenas, the page-locked result buffers and the streams are kept with the engine:
        # allocating and pinning ~150 MB per call cost more than parsing a few windows
        cache = self.__dict__.setdefault('_json_bufs', {})
        if B not in cache:
            cache[B] = ([self.json_device_buffers(B) for _ in range(2)], {}, {}, self._make_json_streams())
        bufs, fb, outs, (s_parse, s_m, s_d) = cache[B]      # fb: host-packer fallback buffers, made on first use
        K = 2 if int(contexts) >= 2 else 1                   # contexts taking turns on the windows (two compute streams exist)
        # Window slots (staging + arena + result buffers): S = K + 2 -- K windows computing, one parsed and about to compute,
        # one being uploaded and parsed (the loop below queues the parse one window ahead).  A slot is reused when its window
        # has been handed out.
        S = K + 2
        while len(bufs) < S:
            bufs.append(self.json_device_buffers(B))
        engs = self.contexts(K)
        if K == 2:
            # window i on context i & 1, each context on its own stream: two windows in flight fill each other's tails
            lanes = [(s_m, s_m), (s_d, s_d)]
        elif os.environ.get('MPE_JSON_STREAMS', '1') == '1':
            # ONE compute stream beside the parse stream: a second compute stream (matching of window i+1 beside the 3D stage
            # of window i, what run_pipelined does for resident batches) measured the same or worse here -- the parse kernels
            # already fill what the GEMMs leave
            lanes = [(s_m, s_m)]
        else:
            lanes = [(s_m, s_d)]
        out_dt = torch.float32 if mode == 'mlp' else torch.float64
        outs.setdefault(mode, [])
        while len(outs[mode]) < S:
            outs[mode].append((torch.empty((B, self.pcap, self.J, 3), dtype=out_dt).pin_memory(),
                               torch.empty((B,), dtype=torch.int32).pin_memory()))
        out = outs[mode]
        done = [None] * S
        cur = torch.cuda.current_stream(self.device)
        for s_ in (s_parse, s_m, s_d):
            s_.wait_stream(cur)
        pool = ThreadPoolExecutor(1)
        index = JsonIndex(text)
        t_setup = time.perf_counter() - t_call

        def stage(i):
            try:
                return stage_json_window(index, self.params, bufs[i % S]['host'], frame_start=i * B * frame_step, frame_step=frame_step,
                                         max_frames=B, n_threads=n_threads)
            except NeedsHostParser:
                return None
            except ValueError as e:
                if 'too small' in str(e):                    # an unusually long window: let the host packer size it
                    return None
                raise

        def host_pack(i):
            # rare path: everything that is in flight finishes first (the two fallback arenas and the context are then free)
            for j in range(S):
                copy_out(j)
            torch.cuda.synchronize(self.device)
            k = i & 1
            if not fb:
                fb['host'] = CapacityArena(self.V, self.J, B, H, 'pinned')
                fb['dev'] = [CapacityArena(self.V, self.J, B, H, self.device) for _ in range(2)]
                fb['db'] = [None, None]
            pb = pack_json_into(index, self.params, fb['host'], frame_start=i * B * frame_step, frame_step=frame_step, max_frames=B,
                                n_threads=n_threads)
            if pb.n_frames == 0:
                return None
            self.check_capacity(pb)
            import copy
            keep = copy.copy(pb)
            for name in ('frame_head_off', 'frame_en_off', 'slot_cam', 'slot_n', 'head_cam', 'skeleton_index', 'joint_mask', 'tri_mask', 'xy', 'vp'):
                setattr(keep, name, np.array(getattr(pb, name)))      # the one host arena is reused by the next fallback
            if fb['db'][k] is None:
                fb['db'][k] = DeviceBatch(keep, self.device, arena=fb['dev'][k])
            db = fb['db'][k].rebind(keep)
            fb['dev'][k].buf.copy_(fb['host'].buf, non_blocking=True)
            cur.synchronize()                                  # the pinned arena is free again (rare path)
            return db
        timing = [] if os.environ.get('MPE_JSON_TIMING') else None
        gpu_ev = []
        # Copy engines serve their requests in order: a D2H of results queued behind kernels that are still running holds up the
        # H2D of a later window's strings until those kernels are done (measured: 6.4 ms instead of 0.57 ms).  So the results of
        # a window are queued for copy-out only after the upload of the window that is parsed next.
        res = [None] * S                                     # (poses, n_persons, n, lane) of the slot, still on the device

        def copy_out(k):
            if res[k] is None:
                return
            poses_, n_persons_, n_, lane_ = res[k]
            with torch.cuda.stream(lane_):                 # behind the 3D stage that produced them
                out[k][0][:n_].copy_(poses_, non_blocking=True)
                out[k][1][:n_].copy_(n_persons_, non_blocking=True)
                done[k] = torch.cuda.Event()
                done[k].record()
            res[k] = None
        # The loop runs the PARSE ONE WINDOW AHEAD of the compute: in iteration i the upload and the parse kernels of window
        # i+1 are queued first, then the host waits for the totals of window i (queued an iteration ago, so they are there or
        # nearly), launches its compute and hands out the results of window i-K.  Queued in the same iteration as its own
        # compute, a parse was on the host's critical path for its whole duration beside K computes (3 ms of a 5.5 ms window).
        futs, pev = {}, {}

        def queue(i):
            """Stage result of window i -> its upload + parse on the parse stream.  ('dev', frames) | ('host', B) | ('end', 0)"""
            t0_ = time.perf_counter()
            st = futs.pop(i).result()
            t1_ = time.perf_counter()
            if st is None:
                return ('host', B, t1_ - t0_, 0.0)
            nf, ne, used = st
            if nf == 0:
                return ('end', 0, t1_ - t0_, 0.0)
            k = i % S
            assert res[k] is None, 'window slot reused before its results were handed out'
            with torch.cuda.stream(s_parse):
                if done[k] is not None:
                    s_parse.wait_event(done[k])          # the arena of this slot: window i - S has computed and its results are out
                if timing is not None:
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    bufs[k]['ev_h2d'] = torch.cuda.Event(enable_timing=True)
                self.parse_json_device(bufs[k], nf, ne, used)
                if timing is not None:
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record()
                    pev[i] = (e0, e1, bufs[k]['ev_h2d'])
            return ('dev', nf, t1_ - t0_, time.perf_counter() - t1_)

        def may_continue(w):
            return w[0] == 'host' or (w[0] == 'dev' and w[1] == B)
        try:
            futs[0] = pool.submit(stage, 0)
            w_cur = queue(0)
            if may_continue(w_cur):
                futs[1] = pool.submit(stage, 1)
            i = 0
            pending = []
            while w_cur[0] != 'end':
                k = i % S                                   # slot of this window
                w_nxt = ('end', 0, 0.0, 0.0)
                if i + 1 in futs:
                    w_nxt = queue(i + 1)
                    if may_continue(w_nxt):
                        futs[i + 2] = pool.submit(stage, i + 2)   # into the staging buffer of window i + 2 - S, uploaded long ago
                t_c = time.perf_counter()
                db = None
                if w_cur[0] == 'dev':
                    db = self.finish_parse(bufs[k])
                    if db is not None:
                        if db.max_heads_per_frame() > self.hpf:
                            raise ValueError('a frame holds %d skeletons, capacity is %d (raise max_persons_per_camera / '
                                             'max_heads_per_frame)' % (db.max_heads_per_frame(), self.hpf))
                        lanes[i % K][0].wait_event(bufs[k]['ready'])
                t_d = time.perf_counter()
                from_device = db is not None
                if db is None:                                  # this window goes through the host packer
                    db = host_pack(i)
                    if db is None:
                        break
                n_here = db.n_frames
                eng, (l_m, l_d) = engs[i % K], lanes[i % K]
                # the results of window i-K (same context, same stream) leave the device BEFORE this window's kernels are queued
                # behind them on that stream; this window's upload is already in the copy queue, the next one's comes an
                # iteration later, when window i-K has long finished (copy engines serve in order)
                if len(pending) >= K:
                    copy_out(pending[0][0])
                if timing is not None:
                    ev_c0 = torch.cuda.Event(enable_timing=True)
                    ev_c0.record(l_m)
                if db.host is not None:
                    l_m.wait_stream(cur)                     # host-packed window: its upload went over the caller's stream
                with torch.cuda.stream(l_m):
                    _, persons, n_persons = match_stage(eng, db)
                    ev_m = torch.cuda.Event()
                    ev_m.record()
                with torch.cuda.stream(l_d):
                    if l_d is not l_m:
                        l_d.wait_event(ev_m)
                    poses = (eng.mlp3d(db, persons, n_persons) if mode == 'mlp' else eng.triangulate(db, persons, n_persons))[0]
                if l_d is not l_m:
                    for t_ in (persons, n_persons):
                        t_.record_stream(l_d)
                res[k] = (poses, n_persons, n_here, l_d)
                done[k] = None
                if timing is not None and from_device and i in pev:
                    ev_c1 = torch.cuda.Event(enable_timing=True)
                    ev_c1.record(l_d)
                    gpu_ev.append(pev.pop(i)[:2] + (ev_c0, ev_c1) + (bufs[k]['ev_h2d'],))
                t_e = time.perf_counter()
                pending.append((k, db if db.host is None else db.host, n_here))
                if len(pending) > K:                          # K windows stay in flight; the oldest one is handed out
                    pk, pinfo, pn = pending.pop(0)
                    copy_out(pk)                              # (already queued above)
                    done[pk].synchronize()
                    if timing is not None:
                        timing.append((w_nxt[2], w_nxt[3], t_d - t_c, t_e - t_d, time.perf_counter() - t_e))
                    yield pinfo, out[pk][0][:pn].numpy(), out[pk][1][:pn].numpy()
                if n_here < B:
                    break
                w_cur = w_nxt
                i += 1
            while pending:
                pk, pinfo, pn = pending.pop(0)
                copy_out(pk)
                done[pk].synchronize()
                yield pinfo, out[pk][0][:pn].numpy(), out[pk][1][:pn].numpy()
        finally:
            for f_ in list(futs.values()):
                f_.cancel()
            pool.shutdown(wait=True)
            for s_ in (s_parse, s_m, s_d):
                cur.wait_stream(s_)
            torch.cuda.synchronize(self.device)
            index.close()
            if timing and len(timing) > 2:
                import sys
                m = np.array(timing[1:]).mean(axis=0) * 1e3
                print('stream_json(device): buffers, streams and the frame index ready after %.2f ms; first window staged after %.2f ms'
                      % (1e3 * t_setup, 1e3 * timing[0][0] + 1e3 * t_setup), file=sys.stderr)
                print('stream_json(device) per window, ms: wait staging %.2f | queue parse %.2f | wait parse %.2f | launch compute %.2f | '
                      'wait previous results %.2f' % tuple(m), file=sys.stderr)
                worst = np.array(timing[1:]).max(axis=0) * 1e3
                print('  slowest window of each, ms:            wait staging %.2f | queue parse %.2f | wait parse %.2f | launch compute %.2f | '
                      'wait previous results %.2f' % tuple(worst), file=sys.stderr)
                base = gpu_ev[2][0]
                for w in range(2, min(7, len(gpu_ev))):
                    p0, p1, c0, c1, h = gpu_ev[w]
                    print('  window %d on the GPU clock, ms: H2D %.2f .. %.2f, parse kernels .. %.2f | compute %.2f .. %.2f'
                          % (w, base.elapsed_time(p0), base.elapsed_time(h), base.elapsed_time(p1), base.elapsed_time(c0), base.elapsed_time(c1)), file=sys.stderr)

    # ---- device-side parse -----------------------------------------------
    def json_device_buffers(self, max_frames, text_cap=None):
        """Buffers of one in-flight window of the device-side parse: pinned + device staging, the device
        arena the arrays are parsed into, scratch and the totals (device + pinned mirror)."""
        B = int(max_frames)
        H = B * self.hpf
        if text_cap is None:
            text_cap = B * self.V * (64 + 96 * self.J * max(1, self.hpf // self.V) * 2)      # ~2x a full camera string
        text_cap = (int(text_cap) + 255) // 256 * 256
        return {'host': JsonStage(self.V, B, text_cap, 'pinned'), 'dev': JsonStage(self.V, B, text_cap, self.device),
                'arena': CapacityArena(self.V, self.J, B, H, self.device),
                'kcap': self.hpf,
                'scratch': torch.empty(int(self.lib.mpe_json_scratch_bytes(B * self.V, self.hpf, self.J)), dtype=torch.uint8, device=self.device),
                'totals': torch.zeros(4, dtype=torch.int32, device=self.device),
                'totals_host': torch.zeros(4, dtype=torch.int32).pin_memory(), 'ready': torch.cuda.Event()}

    def parse_json_device(self, bufs, n_frames, n_entries, used_bytes):
        """Queue (current stream): staging H2D (one copy of the used prefix) -> mpe_json_parse_device -> totals
        D2H into pinned memory; records bufs['ready'].  `finish_parse` turns the totals into a batch."""
        bufs['dev'].buf[:used_bytes].copy_(bufs['host'].buf[:used_bytes], non_blocking=True)
        if bufs.get('ev_h2d') is not None:
            bufs['ev_h2d'].record()
        arena = bufs['arena']
        out = L.mpe_batch()
        for name in ('frame_head_off', 'frame_en_off', 'slot_cam', 'slot_n', 'head_cam', 'joint_mask', 'tri_mask', 'xy', 'vp'):
            setattr(out, 'd_' + name, C.c_void_p(arena.ptr(name)))
        dev = bufs['dev']
        self._chk(self.lib.mpe_json_parse_device(self.ctx, self._stream(), C.c_void_p(dev.ptr('text')), C.c_void_p(dev.ptr('entries')),
                                                 C.c_void_p(dev.ptr('frame_entry_off')), n_entries, n_frames, arena.max_heads,
                                                 bufs['kcap'], _ptr(bufs['scratch']), bufs['scratch'].numel(), C.byref(out),
                                                 C.c_void_p(arena.ptr('skeleton_index')), _ptr(bufs['totals'])))
        bufs['totals_host'].copy_(bufs['totals'], non_blocking=True)
        bufs['ready'].record()
        bufs['n_frames'] = n_frames

    def finish_parse(self, bufs):
        """Wait for the parse of `bufs` and return the batch (ParsedOnDevice), or None if the window holds
        something the device parser leaves to the host packer (status bit 0) -- the caller then packs it
        on the host.  More heads than the arena holds raises like the host packer does."""
        bufs['ready'].synchronize()
        n_heads, n_en, status, max_h = (int(x) for x in bufs['totals_host'].tolist())
        if status & 1:                       # first: a window the device declines is sized (and refused, if need be) by the host packer
            return None
        if status & 2:
            raise ValueError('device-side parse: %d skeletons exceed the arena capacity %d' % (n_heads, bufs['arena'].max_heads))
        return ParsedOnDevice(bufs['arena'], self.V, self.J, bufs['n_frames'], n_heads, n_en, max_h)

    def pack_json_device(self, text, frame_start=0, frame_step=1, max_frames=0, n_threads=0):
        """One window of a document through the device-side parser (tests, one-off calls): JSON bytes ->
        ParsedOnDevice, or None where the host packer has to take over."""
        index = text if isinstance(text, JsonIndex) else JsonIndex(text)
        try:
            B = int(max_frames) if max_frames > 0 else self.max_frames
            if B > self.max_frames:
                raise ValueError('window of %d frames exceeds max_frames=%d' % (B, self.max_frames))
            size = len(index.text)
            bufs = self.json_device_buffers(B, text_cap=size + 16 * B * self.V + 256)
            try:
                nf, ne, used = stage_json_window(index, self.params, bufs['host'], frame_start, frame_step, B, n_threads)
            except NeedsHostParser:
                return None
            self.parse_json_device(bufs, nf, ne, used)
            pd = self.finish_parse(bufs)
            if pd is not None:
                pd.keep = bufs
            return pd
        finally:
            if index is not text:
                index.close()

    # ---- ground-truth bodies parsed on the device ------------------------------------------------
    def bodies_from_json(self, index_or_text, frame_start=0, frame_step=1, max_frames=0, scap=None, cameras=None, n_threads=0,
                         entries_per_frame=None):
        """bodies_3D (element [3] of every camera entry) of one window of a document, parsed on the device: host staging
        of the first level (mpe_json_stage_gt_window), one copy, mpe_json_parse_bodies_device, the status word read back.
        cameras: the configured cameras (default params.used_cameras); scap: rows per frame (default 2 * hpf);
        entries_per_frame: camera keys a frame may hold (default 2 * V).  -> packing.ParsedBodies; with a non-zero status
        the caller takes the host path for the window (json.load, harness.common.ground_truth / partition.pack_bodies)."""
        index = index_or_text if isinstance(index_or_text, JsonIndex) else JsonIndex(index_or_text)
        try:
            B = int(max_frames) if max_frames > 0 else self.max_frames
            cameras = list(self.params.used_cameras if cameras is None else cameras)
            scap = int(scap) if scap else 2 * self.hpf
            epf = int(entries_per_frame) if entries_per_frame else 2 * self.V
            size = len(index.text)
            bound = size + 16 * B * epf + 256                           # the whole document, every entry padded: always enough
            bufs = self._gt_bufs
            if bufs is None or bufs['B'] < B or bufs['epf'] < epf:
                bufs = None
            while True:
                if bufs is None:
                    cap = min(bound, max(1 << 20, B * epf * 4096))
                    cap = (cap + 255) // 256 * 256
                    bufs = {'B': B, 'epf': epf, 'cap': cap, 'host': JsonStage(epf, B, cap, 'pinned'), 'dev': JsonStage(epf, B, cap, self.device),
                            'status_host': torch.zeros(1, dtype=torch.int32).pin_memory()}
                try:
                    nf, ne, used = stage_gt_window(index, cameras, bufs['host'], frame_start, frame_step, B, n_threads)
                    break
                except NeedsHostParser:
                    return ParsedBodies(1)
                except MemoryError:
                    if bufs['cap'] >= bound:
                        raise ValueError('a frame holds more than %d camera entries' % bufs['epf'])
                    cap = (min(bound, 4 * bufs['cap']) + 255) // 256 * 256
                    bufs = {'B': bufs['B'], 'epf': bufs['epf'], 'cap': cap, 'host': JsonStage(bufs['epf'], bufs['B'], cap, 'pinned'),
                            'dev': JsonStage(bufs['epf'], bufs['B'], cap, self.device), 'status_host': bufs['status_host']}
            self._gt_bufs = bufs
            dev, d = bufs['dev'], self.device
            dev.buf[:used].copy_(bufs['host'].buf[:used], non_blocking=True)
            rows = (nf, scap)
            t = {'xyz': torch.empty(rows + (L.MPE_GT_KEY_SLOTS, 3), dtype=torch.float64, device=d),
                 'mask': torch.empty(rows, dtype=torch.int32, device=d), 'nkeys': torch.empty(rows, dtype=torch.int32, device=d),
                 'order': torch.empty(rows + (L.MPE_GT_KEY_SLOTS,), dtype=torch.uint8, device=d), 'm1': torch.empty(rows, dtype=torch.uint8, device=d),
                 'n': torch.empty((nf,), dtype=torch.int32, device=d), 'entry_count': torch.empty((max(1, ne),), dtype=torch.int32, device=d),
                 'body_cam': torch.empty(rows, dtype=torch.int32, device=d)}
            status = torch.empty((1,), dtype=torch.int32, device=d)
            nsc = int(self.lib.mpe_json_bodies_scratch_bytes(ne, scap))
            scratch = torch.empty(nsc, dtype=torch.uint8, device=d)
            a = L.mpe_json_bodies_args()
            a.n_frames, a.n_entries, a.scap = nf, ne, scap
            a.d_text, a.d_entries, a.d_frame_entry_off = dev.ptr('text'), dev.ptr('entries'), dev.ptr('frame_entry_off')
            a.d_xyz, a.d_mask, a.d_nkeys, a.d_order, a.d_m1 = (t[k].data_ptr() for k in ('xyz', 'mask', 'nkeys', 'order', 'm1'))
            a.d_n, a.d_entry_count, a.d_body_cam = t['n'].data_ptr(), t['entry_count'].data_ptr(), t['body_cam'].data_ptr()
            a.d_status, a.d_scratch, a.scratch_bytes = status.data_ptr(), scratch.data_ptr(), nsc
            self._chk(self.lib.mpe_json_parse_bodies_device(self.ctx, self._stream(), C.byref(a)))
            # the entry tables leave the staging buffer (it is reused by the next window)
            t['entries'] = dev.buf[dev.off_entries: dev.off_entries + 16 * max(1, ne)].clone().view(torch.int32).reshape(-1, 4)
            t['frame_entry_off'] = dev.buf[dev.off_feo: dev.off_feo + 4 * (nf + 1)].clone().view(torch.int32)
            bufs['status_host'].copy_(status, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            t['entry_count'] = t['entry_count'][:ne] if ne else t['entry_count'][:0]
            t['entries'] = t['entries'][:ne]
            return ParsedBodies(int(bufs['status_host'][0]), nf, ne, scap, **t)
        finally:
            if index is not index_or_text:
                index.close()

    def ground_truth(self, bodies, T_d_list, file_of_frame, T_i1, gcap=None):
        """The metrics scripts' ground truth of every frame of `bodies` (a ParsedBodies with status 0) on the device
        (mpe_gt_from_bodies): the camera with the most bodies (the first of equals, any camera of the frame), centimetres
        -> metres, then T_i1 @ (T_d @ x) in the fp32 arithmetic of torch's CPU matmul.  T_d_list: one 4x4 per file,
        file_of_frame [B]: the file of every frame; T_i1: 4x4.  -> harness.common.pack_ground_truth's dict as device
        tensors ('xyz' [B,gcap,J,3] f32, 'joint' [B,gcap,J] u8, 'valid' [B,gcap] u8, 'n' [B] i32), which Engine.evaluate
        takes as it is; gcap defaults to bodies.scap."""
        if bodies.status != 0:
            raise ValueError('the window was not parsed on the device (status %d)' % bodies.status)
        B, d = bodies.n_frames, self.device
        gcap = int(gcap) if gcap else bodies.scap
        Td = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float32).reshape(4, 4) for T in T_d_list]), np.float32)
        fof = np.ascontiguousarray(np.asarray(file_of_frame, dtype=np.int32).reshape(-1))
        if len(fof) != B or (B and (fof.min() < 0 or fof.max() >= len(Td))):
            raise ValueError('file_of_frame must name one of the %d transforms for each of the %d frames' % (len(Td), B))
        Ti = np.ascontiguousarray(np.asarray(T_i1, dtype=np.float32).reshape(16))
        Td_d, fof_d = torch.from_numpy(Td).to(d), torch.from_numpy(fof).to(d)
        out = {'xyz': torch.empty((B, gcap, self.J, 3), dtype=torch.float32, device=d),
               'joint': torch.empty((B, gcap, self.J), dtype=torch.uint8, device=d),
               'valid': torch.empty((B, gcap), dtype=torch.uint8, device=d), 'n': torch.empty((B,), dtype=torch.int32, device=d)}
        a = L.mpe_gt_args()
        a.n_frames, a.scap, a.gcap, a.n_joints, a.n_files = B, bodies.scap, gcap, self.J, len(Td)
        ec = bodies.entry_count if bodies.n_entries else torch.zeros(1, dtype=torch.int32, device=d)
        en = bodies.entries if bodies.n_entries else torch.zeros((1, 4), dtype=torch.int32, device=d)
        a.d_entries, a.d_frame_entry_off, a.d_entry_count = en.data_ptr(), bodies.frame_entry_off.data_ptr(), ec.data_ptr()
        a.d_xyz, a.d_mask, a.d_m1 = bodies.xyz.data_ptr(), bodies.mask.data_ptr(), bodies.m1.data_ptr()
        a.d_T_d, a.d_file_of_frame, a.T_i1 = Td_d.data_ptr(), fof_d.data_ptr(), _f32p(Ti)
        a.d_gt_xyz, a.d_gt_joint, a.d_gt_valid, a.d_n_gt_in = (out[k].data_ptr() for k in ('xyz', 'joint', 'valid', 'n'))
        self._chk(self.lib.mpe_gt_from_bodies(self.ctx, self._stream(), C.byref(a)))
        out['_keep'] = (Td_d, fof_d, ec, en)
        return out

    def run_pipelined(self, batches, mode='mlp', contexts=1, matcher='gat', geom=None):
        """Batches (DeviceBatch or PackedBatch) -> (poses, n_persons, persons) per batch, in order.

        contexts == 1: the two stages on their own streams: the matching stage of batch i+1 (GAT workspace) runs while
        the 3D stage of batch i (MLP workspace / DLT) is still in flight -- the two workspaces are disjoint, and
        concurrent kernels fill the tails of each other's dependent launch chains (+2-5 % throughput at 1000-frame
        batches).  contexts == K > 1: K contexts (sibling()) take turns on the batches, each on its own stream, so K whole
        batches are in flight (195.6 k against 186-189 k frames/s at K = 2; K = 3: 194.7 k).  Either way the results are
        the same bits as match() + mlp3d() / triangulate() called one after the other.  Each result is yielded once its
        3D stage has finished (with K contexts: when K - 1 later batches have been queued).
        matcher = 'geometric': geom_match (options in the dict `geom`) in the place of match; no GAT weights are needed."""
        match_stage = self._match_stage(matcher, geom)
        K = max(1, int(contexts))
        engs = self.contexts(K)
        two = K == 1
        s_match = [torch.cuda.Stream(self.device) for _ in range(K)]
        s_3d = [torch.cuda.Stream(self.device)] if two else s_match
        cur = torch.cuda.current_stream(self.device)
        pending = []
        try:
            for i, b in enumerate(batches):
                e, sm, sd = engs[i % K], s_match[i % K], s_3d[i % K]
                db = self.to_device(b)
                # whatever produced this batch (an upload the iterator queued on the current stream) is ordered
                # before its matching stage -- per batch, not once in front of the loop
                sm.wait_stream(cur)
                with torch.cuda.stream(sm):
                    _, persons, n_persons = match_stage(e, db)
                    ev = torch.cuda.Event()
                    ev.record(sm)
                with torch.cuda.stream(sd):
                    if two:
                        sd.wait_event(ev)
                    poses = (e.mlp3d(db, persons, n_persons) if mode == 'mlp' else e.triangulate(db, persons, n_persons))[0]
                    done = torch.cuda.Event()
                    done.record(sd)
                # tensors allocated on one stream and consumed on another: the allocator must not hand
                # their memory out again before the consumer is done
                if two:
                    for t_ in (persons, n_persons):
                        t_.record_stream(sd)
                pending.append((done, poses, n_persons, persons, db))   # db: keeps the batch alive while it is in flight
                if len(pending) > K:
                    prev = pending.pop(0)
                    prev[0].synchronize()
                    yield prev[1:]
            while pending:
                last = pending.pop(0)
                last[0].synchronize()
                yield last[1:]
        finally:
            # also on early exit (the consumer closed the generator): nothing of ours is still running on
            # the side streams when the caller's stream goes on, and nothing in flight is freed under them
            for s_ in set(s_match + s_3d):
                cur.wait_stream(s_)
            for p_ in pending:
                p_[0].synchronize()

    def to_device(self, pb):
        if isinstance(pb, DeviceBatch):
            return pb
        assert isinstance(pb, PackedBatch)
        self.check_capacity(pb)
        return pb.to(self.device)

    def check_capacity(self, pb):
        """The kernels size their LDS / scratch from the capacities given at construction; a
        batch beyond them must be rejected here (the C ABI cannot see per-frame counts)."""
        if pb.n_frames > self.max_frames:
            raise ValueError('batch of %d frames exceeds max_frames=%d' % (pb.n_frames, self.max_frames))
        if pb.n_frames == 1 and pb.n_heads <= self.hpf and pb.V == self.V and pb.J == self.J and getattr(pb, 'en_pair', None) is None:
            return                           # (one frame of the per-frame mirrors: nothing below can fail)
        if pb.n_frames and pb.max_heads_per_frame() > self.hpf:
            raise ValueError('a frame holds %d skeletons, capacity is %d (raise max_persons_per_camera / '
                             'max_heads_per_frame)' % (pb.max_heads_per_frame(), self.hpf))
        if pb.V != self.V or pb.J != self.J:
            raise ValueError('batch packed for %d cameras x %d joints, engine built for %d x %d'
                             % (pb.V, pb.J, self.V, self.J))
        if getattr(pb, 'en_pair', None) is not None and pb.n_frames:
            cap = explicit_m_cap(self.hpf)
            if cap == 0:
                raise ValueError('explicit edge-node lists need max_heads_per_frame <= 1024 and 16-bit node ids (capacity %d)' % self.hpf)
            if pb.max_edge_nodes_per_frame() > cap:
                raise ValueError('a graph holds %d edge-nodes, an engine with max_heads_per_frame = %d takes %d per frame'
                                 % (pb.max_edge_nodes_per_frame(), self.hpf, cap))
            if pb.n_edge_nodes > self.max_frames * self.m_frame:
                raise ValueError('batch of %d edge-nodes exceeds the capacity %d (max_edge_nodes_per_frame)'
                                 % (pb.n_edge_nodes, self.max_frames * self.m_frame))
            ep = np.asarray(pb.en_pair).reshape(-1, 2)
            H = np.repeat(np.diff(pb.frame_head_off), np.diff(pb.frame_en_off))
            if ep.size and (ep.min() < 0 or (ep >= H[:, None]).any() or (ep[:, 0] == ep[:, 1]).any()):
                raise ValueError('explicit edge-node list: a pair lies outside its frame or joins a head with itself')

    def _stream(self):
        # torch.cuda.current_stream() builds a Stream object (~80 us on the GPU box's host; ten calls per frame in the
        # one-frame-per-call mirrors); the raw handle is what the C ABI takes
        try:
            return C.c_void_p(torch._C._cuda_getCurrentRawStream(self.device.index or 0))
        except AttributeError:
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def match(self, db, want_scores=True):
        """-> (scores[n_edge_nodes] f32 or None, persons[B,Pcap,V] i32, n_persons[B] i32)."""
        B = db.n_frames
        scores = torch.empty(max(db.n_edge_nodes, 1), dtype=torch.float32, device=self.device) if want_scores else None
        persons = torch.empty((B, self.pcap, self.V), dtype=torch.int32, device=self.device)
        n_persons = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.mpe_match_batch(self.ctx, self._stream(), C.byref(db.struct),
                                           _ptr(scores), _ptr(persons), _ptr(n_persons)))
        return (scores[:db.n_edge_nodes] if want_scores else None), persons, n_persons

    def _geom_args(self, sigma, clip, min_joints, joint_mask, min_conf):
        a = L.mpe_geom_args()
        a.sigma_m, a.clip_m, a.min_joints = float(sigma), float(clip), int(min_joints)
        a.joint_mask, a.min_conf = int(joint_mask or 0), float(min_conf)
        return a

    def geom_scores(self, db, sigma=0.10, clip=0.5, min_joints=1, joint_mask=None, min_conf=0.0, details=False):
        """Matching scores from the calibration alone (mpe_geom_scores_batch; no weights needed): per edge-node the mean
        distance between the back-projected rays of its two skeletons over the joints both have (joint_mask: the joints
        that may vote, None = all; min_conf: the detection confidence a vote needs in both views), clipped per joint at
        `clip` metres (0: no clip), as score = sigma / (sigma + mean); 0 with fewer than min_joints votes.  include/mpe.h
        has the rule, harness/geometric.py states it in numpy and the two agree bit for bit.  The scores feed cluster()
        like the GAT's.  -> scores [n_edge_nodes] f32, or with details (scores, n_votes u8, mean f64: -1 without a vote)."""
        M = db.n_edge_nodes
        sc = torch.empty(max(M, 1), dtype=torch.float32, device=self.device)
        a = self._geom_args(sigma, clip, min_joints, joint_mask, min_conf)
        a.d_scores = sc.data_ptr()
        if details:
            nv = torch.empty(max(M, 1), dtype=torch.uint8, device=self.device)
            mean = torch.empty(max(M, 1), dtype=torch.float64, device=self.device)
            a.d_n_votes, a.d_mean = nv.data_ptr(), mean.data_ptr()
        self._chk(self.lib.mpe_geom_scores_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return (sc[:M], nv[:M], mean[:M]) if details else sc[:M]

    def geom_match(self, db, want_scores=True, sigma=0.10, clip=0.5, min_joints=1, joint_mask=None, min_conf=0.0):
        """match() with the geometric scores of geom_scores in the GAT's place (mpe_geom_match_batch: scores + clustering).
        -> (scores[n_edge_nodes] f32 or None, persons[B,Pcap,V] i32, n_persons[B] i32)."""
        B = db.n_frames
        scores = torch.empty(max(db.n_edge_nodes, 1), dtype=torch.float32, device=self.device) if want_scores else None
        persons = torch.empty((B, self.pcap, self.V), dtype=torch.int32, device=self.device)
        n_persons = torch.empty((B,), dtype=torch.int32, device=self.device)
        a = self._geom_args(sigma, clip, min_joints, joint_mask, min_conf)
        a.d_scores = scores.data_ptr() if want_scores else None
        self._chk(self.lib.mpe_geom_match_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a), _ptr(persons), _ptr(n_persons)))
        return (scores[:db.n_edge_nodes] if want_scores else None), persons, n_persons

    def _match_stage(self, matcher, geom):
        """matcher 'gat' | 'geometric' (geom: the options of geom_match) -> the matching call of the pipelines, f(engine, db)."""
        if matcher == 'gat':
            return lambda e, db: e.match(db, want_scores=False)
        if matcher != 'geometric':
            raise ValueError("matcher must be 'gat' or 'geometric'")
        opts = dict(geom or {})
        return lambda e, db: e.geom_match(db, want_scores=False, **opts)

    def gat_scores(self, db, heads=False, feats=None):
        """GAT2.forward; `feats` (optional) = dense [n_nodes, F] rows supplied by the caller."""
        sc = torch.empty(max(db.n_edge_nodes, 1), dtype=torch.float32, device=self.device)
        sh = torch.empty(max(db.n_heads, 1), dtype=torch.float32, device=self.device) if heads else None
        ld = 0
        if feats is not None:
            feats = feats.to(self.device, torch.float32).contiguous()
            ld = feats.shape[1]
        self._chk(self.lib.mpe_gat_forward(self.ctx, self._stream(), C.byref(db.struct), _ptr(feats), ld,
                                           _ptr(sc), _ptr(sh)))
        return (sc[:db.n_edge_nodes], sh[:db.n_heads]) if heads else sc[:db.n_edge_nodes]

    def gat_scores_joined(self, db, feats=None):
        """GAT2.forward of a one-graph batch in the node order of the reference's output (heads, then edge-nodes): both halves are
        written into ONE [n_heads + n_edge_nodes] buffer (the last layer's rows are single floats: no alignment beyond 4 bytes is
        asked of either half).  -> (all scores, the edge-node part as a view)."""
        H, M = db.n_heads, db.n_edge_nodes
        out = torch.empty(H + M, dtype=torch.float32, device=self.device)
        ld = 0
        if feats is not None:
            feats = feats.to(self.device, torch.float32).contiguous()
            ld = feats.shape[1]
        base = out.data_ptr()
        self._chk(self.lib.mpe_gat_forward(self.ctx, self._stream(), C.byref(db.struct), _ptr(feats), ld,
                                           C.c_void_p(base + 4 * H), C.c_void_p(base)))
        return out, out[H:]

    def set_gat_output(self, sigmoid=True):
        """Last-layer activation: sigmoid (deployed model) or identity (final_activation=None)."""
        if self._state.get('gat_output', True) == bool(sigmoid):
            return
        self._chk(self.lib.mpe_set_gat_output(self.ctx, 1 if sigmoid else 2))
        self._state['gat_output'] = bool(sigmoid)
        for e in self._siblings:
            e.set_gat_output(sigmoid)

    def gat_layer(self, db, layer, x, activation=0):
        """One GraphAttention2 layer + the activation GAT2.forward applies (mpe_gat_layer).
        x [n_nodes, in_dim] rows in node order -> [n_nodes, heads*out_dim].  Layer 0 with x = None: the rows are featurised on
        the device, the production route of layer 0 (implicit topology)."""
        _, nh, od = self.gat_dims[layer]
        if x is None:
            out = torch.empty((db.n_heads + db.n_edge_nodes, nh * od), dtype=torch.float32, device=self.device)
            self._chk(self.lib.mpe_gat_layer(self.ctx, self._stream(), C.byref(db.struct), layer, None, 0,
                                             _ptr(out), out.shape[1], int(activation)))
            return out
        x = x.to(self.device, torch.float32).contiguous()
        out = torch.empty((x.shape[0], nh * od), dtype=torch.float32, device=self.device)
        self._chk(self.lib.mpe_gat_layer(self.ctx, self._stream(), C.byref(db.struct), layer, _ptr(x), x.shape[1],
                                         _ptr(out), out.shape[1], int(activation)))
        return out

    def l0_attention_launches(self):
        """How often this engine's context queued the whole-row layer-0 attention launch (mpe_l0_attention_launches)."""
        n = C.c_int64()
        self._chk(self.lib.mpe_l0_attention_launches(self.ctx, C.byref(n)))
        return n.value

    def edge_softmax_aggregate(self, db, layer, ft2):
        """The DGL half of a layer (gat2.py:57-66): ft2 [n_nodes, heads*out_dim] -> aggregated rows."""
        ft2 = ft2.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(ft2)
        self._chk(self.lib.mpe_edge_softmax_aggregate(self.ctx, self._stream(), C.byref(db.struct), layer, _ptr(ft2),
                                                      ft2.shape[1], _ptr(out), out.shape[1]))
        return out

    def sync_status(self):
        """Synchronise and raise MpeError(MPE_ERR_CAPACITY) if a frame of a batch since the last
        call exceeded max_heads_per_frame (detected on the device)."""
        self._chk(self.lib.mpe_sync_status(self.ctx, self._stream()))

    def status_queue(self):
        """First half of sync_status: the read-back of the status word joins what is queued so far (mpe_status_queue)."""
        self._chk(self.lib.mpe_status_queue(self.ctx, self._stream()))

    def status_wait(self):
        """Second half: synchronise and raise what the read-back saw (mpe_status_wait)."""
        self._chk(self.lib.mpe_status_wait(self.ctx, self._stream()))

    def set_threshold(self, thr):
        """The clustering threshold (mpe_set_threshold takes no stream: call this with nothing pending on the engine)."""
        if self._state.get('threshold', self._made_with['threshold']) == float(thr):
            return                          # (the C call re-uploads the whole device-side configuration, synchronously)
        self._chk(self.lib.mpe_set_threshold(self.ctx, float(thr)))
        self._state['threshold'] = float(thr)
        for e in self._siblings:
            e.set_threshold(thr)

    def cluster(self, db, scores):
        B = db.n_frames
        scores = scores.to(self.device, torch.float32).contiguous()
        persons = torch.empty((B, self.pcap, self.V), dtype=torch.int32, device=self.device)
        n_persons = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.mpe_cluster_batch(self.ctx, self._stream(), C.byref(db.struct), _ptr(scores),
                                             _ptr(persons), _ptr(n_persons)))
        return persons, n_persons

    def dense_rows(self, db):
        """graph.ndata['h'] of a one-frame batch: the dense [N, 2 + V*J*10] rows in node order (mpe_dense_rows)."""
        F = 2 + self.V * self.J * 10
        out = torch.empty((db.n_heads + db.n_edge_nodes, F), dtype=torch.float32, device=self.device)
        self._chk(self.lib.mpe_dense_rows(self.ctx, self._stream(), C.byref(db.struct), _ptr(out), F))
        return out

    def head_features(self, db):
        out = torch.empty((max(db.n_heads, 1), self.J, 10), dtype=torch.float32, device=self.device)
        self._chk(self.lib.mpe_head_features(self.ctx, self._stream(), C.byref(db.struct), _ptr(out)))
        return out[:db.n_heads]

    def mlp_input_rows(self, db, persons, n_persons):
        B = db.n_frames
        width = self.V * self.J * self.params.numbers_per_joint
        ld = (width + 127) // 128 * 128
        rows = torch.zeros((B * self.pcap, ld), dtype=torch.float32, device=self.device)
        valid = torch.zeros((B * self.pcap,), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.mpe_mlp_input_rows(self.ctx, self._stream(), C.byref(db.struct), _ptr(persons),
                                              _ptr(n_persons), _ptr(rows), ld, _ptr(valid)))
        return rows.view(B, self.pcap, ld)[:, :, :width], valid.view(B, self.pcap)

    def mlp_forward(self, x):
        """x [m, in_dim] f32 (device) -> [m, out_dim]."""
        m, k = x.shape
        ld = (k + 127) // 128 * 128
        stream = self._stream()
        st = self.__dict__.get('_mlp_stage')
        if m <= 64 and (st is None or st[0].shape[1] != ld or st[1] != stream.value):
            # small batches (the one-frame-per-call mirrors): one padded staging buffer per engine and stream, zeroed once -- the pad
            # columns stay zero, a call costs one copy instead of a fill and a copy
            st = self.__dict__['_mlp_stage'] = (torch.zeros((64, ld), dtype=torch.float32, device=self.device), stream.value)
        if m <= 64:
            xp = st[0][:m]
            xp[:, :k].copy_(x)
        else:
            xp = torch.zeros((m, ld), dtype=torch.float32, device=self.device)
            xp[:, :k] = x
        y = torch.empty((m, self.mlp_out), dtype=torch.float32, device=self.device)
        self._chk(self.lib.mpe_mlp_forward(self.ctx, stream, _ptr(xp), ld, m, _ptr(y), self.mlp_out))
        return y

    def mlp3d(self, db, persons, n_persons):
        """-> (poses[B,Pcap,J,3] f32 metres, valid[B,Pcap] u8)."""
        B = db.n_frames
        poses = torch.empty((B, self.pcap, self.J, 3), dtype=torch.float32, device=self.device)
        valid = torch.empty((B, self.pcap), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.mpe_mlp3d_batch(self.ctx, self._stream(), C.byref(db.struct), _ptr(persons),
                                           _ptr(n_persons), _ptr(poses), _ptr(valid)))
        return poses, valid

    def triangulate(self, db, persons, n_persons, all_joints=False, positive_ids_only=False):
        """-> (poses[B,Pcap,J,3] f64, joint_valid[B,Pcap,J] u8).  positive_ids_only: the gather of
        test/reprojection_error.py:296-300 (joints with values[0] > 0 only)."""
        B = db.n_frames
        poses = torch.empty((B, self.pcap, self.J, 3), dtype=torch.float64, device=self.device)
        jv = torch.empty((B, self.pcap, self.J), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.mpe_triangulate_batch(self.ctx, self._stream(), C.byref(db.struct), _ptr(persons),
                                                 _ptr(n_persons), _ptr(poses), _ptr(jv),
                                                 (1 if all_joints else 0) | (2 if positive_ids_only else 0)))
        return poses, jv

    def evaluate(self, db, poses, flags, n_persons, gt, mode, skip=None):
        """Error table and pose-to-ground-truth assignment of every frame on the device (mpe_eval_batch).
        poses / flags / n_persons: what mlp3d (mode 'mlp': f32 poses, person flags) or triangulate (mode 'tri': f64
        poses, joint flags) returned for `db`; gt: harness.common.pack_ground_truth's arrays for the same frames.  Frames
        without a cross-camera pair (M == 0) are skipped unless `skip` ([B] bool) says otherwise.  -> dict of device
        tensors: table [B,Gcap,Pcap] f64, assign / err / invalid [B,Pcap] (detection order), n_gt / n_res / status [B];
        frames with MPE_EVAL_OVER_CAP / _OVER_BUDGET in status are the caller's to finish from the table."""
        B = db.n_frames
        if mode not in ('mlp', 'tri'):
            raise ValueError('mode must be mlp or tri')
        _check_pose_rows(self.J, self.pcap, mode == 'tri', mode == 'tri', poses, flags, n_persons, B=B)
        on_device = isinstance(gt['xyz'], torch.Tensor)          # Engine.ground_truth's tensors are taken as they are
        if gt['xyz'].shape[0] != B or (not on_device and np.any(np.asarray(gt['n']) > gt['xyz'].shape[1])):
            raise ValueError('ground truth for %d frames, batch has %d' % (gt['xyz'].shape[0], B))
        if skip is None:
            skip = (np.diff(np.asarray(db.host.frame_en_off[:B + 1])) == 0).astype(np.uint8)
        dev = self.device
        gcap = max(1, gt['xyz'].shape[1])

        def up(a, dt):
            if isinstance(a, torch.Tensor):
                if a.dtype != dt or a.device != dev:
                    raise ValueError('ground-truth tensors must be %s on %s' % (dt, dev))
                return a.contiguous()
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev, non_blocking=False)
        gx = up(gt['xyz'], torch.float32) if gt['xyz'].shape[1] else torch.zeros((B, 1, self.J, 3), dtype=torch.float32, device=dev)
        gj = up(gt['joint'], torch.uint8) if gt['xyz'].shape[1] else torch.zeros((B, 1, self.J), dtype=torch.uint8, device=dev)
        gv = up(gt['valid'], torch.uint8) if gt['xyz'].shape[1] else torch.zeros((B, 1), dtype=torch.uint8, device=dev)
        gn = up(gt['n'], torch.int32)
        sk = up(skip if isinstance(skip, torch.Tensor) else np.asarray(skip, dtype=np.uint8), torch.uint8)      # (a device tensor: taken as it is)
        out = {'table': torch.empty((B, gcap, self.pcap), dtype=torch.float64, device=dev),
               'assign': torch.empty((B, self.pcap), dtype=torch.int32, device=dev),
               'err': torch.empty((B, self.pcap), dtype=torch.float64, device=dev),
               'invalid': torch.empty((B, self.pcap), dtype=torch.uint8, device=dev)}
        for k in ('n_gt', 'n_res', 'status'):
            out[k] = torch.empty((B,), dtype=torch.int32, device=dev)
        a = L.mpe_eval_args()
        a.n_frames, a.pcap, a.n_joints, a.gcap = B, self.pcap, self.J, gcap
        a.pose_f64, a.joint_flags = int(mode == 'tri'), int(mode == 'tri')
        a.used_joint_mask = sum(1 << j for j in self.params.used_joints)
        a.d_poses, a.d_flags, a.d_n_persons = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr()
        a.d_gt_xyz, a.d_gt_joint, a.d_gt_valid, a.d_n_gt_in, a.d_skip = gx.data_ptr(), gj.data_ptr(), gv.data_ptr(), gn.data_ptr(), sk.data_ptr()
        a.d_table, a.d_assign, a.d_err, a.d_invalid = (out[k].data_ptr() for k in ('table', 'assign', 'err', 'invalid'))
        a.d_n_gt, a.d_n_res, a.d_status = (out[k].data_ptr() for k in ('n_gt', 'n_res', 'status'))
        self._chk(self.lib.mpe_eval_batch(self.ctx, self._stream(), C.byref(a)))
        out['_keep'] = (gx, gj, gv, gn, sk)          # inputs stay alive until the caller has synchronised
        return out

    def tracker(self, mode, max_gap=2, gate=0.5, pcap=None):
        """A Tracker for one sequence of poses in `mode` ('mlp': what mlp3d returns, 'tri': what triangulate returns,
        'gt': ground-truth arrays, f32 poses with per-joint flags and pcap = Gcap):
        person identities over the frames (mpe_track_batch).  A lost person is taken up again after up to `max_gap`
        frames without a detection, within `gate` metres of mean joint distance.  pcap: rows per frame when the poses
        are not this engine's (default: the engine's Pcap)."""
        return Tracker(self, mode, max_gap, gate, self.pcap if pcap is None else int(pcap))

    def track_scorer(self, mode, threshold_mm=150., gid_cap=256, tid_cap=4096, max_frames=None, gcap=None, pcap=None):
        """A TrackScore for one recording of poses in `mode` ('mlp' or 'tri'): CLEAR-MOT and identity measures of the
        track ids against ground-truth identities (mpe_track_score_batch).  A detection matches its assigned GT body
        below threshold_mm.  gid_cap / tid_cap: identities and track ids the tables hold (gid_cap * tid_cap <= 2^22);
        max_frames: frames per update (default: the engine's); gcap / pcap: GT rows and pose rows per frame (default:
        the engine's Pcap)."""
        return TrackScore(self, mode, threshold_mm, gid_cap, tid_cap, self.max_frames if max_frames is None else int(max_frames),
                          self.pcap if gcap is None else int(gcap), self.pcap if pcap is None else int(pcap))

    def smoother(self, mode, window=6, decay=0.8, fill=False, pcap=None):
        """A Smoother for one tracked sequence of poses in `mode` ('mlp' or 'tri', as Engine.tracker takes it): every
        joint of every track is fitted with a line over the current frame and the `window` frames before it, weighted
        by decay ** age (mpe_smooth_batch), which gives a position with less jitter and a velocity.  fill (mode 'tri'):
        a joint that is missing now but was seen twice or more in the window gets the line's value and the flag 2.
        pcap: rows per frame when the poses are not this engine's (default: the engine's Pcap)."""
        return Smoother(self, mode, window, decay, fill, self.pcap if pcap is None else int(pcap))

    def skeleton(self, mode, bones=None, bin_mm=2.0, tid_cap=256, pcap=None):
        """A Skeleton for one tracked sequence of poses in `mode` ('mlp' or 'tri', as Engine.tracker takes it): the
        bone lengths of every track are learned from its own frames (a histogram per track and bone with bins of bin_mm,
        its lower median) and the poses are moved towards them frame by frame (mpe_skel_*).  bones: (parent, child) joint
        pairs, at most 32, swept in list order (default: harness.skeleton.BONES_18, for 18 joints only); tid_cap: track
        ids the tables hold (tid_cap * bones <= 2^17); pcap: rows per frame when the poses are not this engine's
        (default: the engine's Pcap)."""
        return Skeleton(self, mode, bones, bin_mm, tid_cap, self.pcap if pcap is None else int(pcap))

    def relinker(self, mode, bones=None, tid_cap=256, pcap=None, max_frames=None, **options):
        """A Relinker for one tracked sequence of poses in `mode` ('mlp' or 'tri', as Engine.skeleton takes it): a track
        that is born takes the id of a track lost min_gap .. max_gap frames ago when their bone lengths agree within
        gate_m and, with reach_m > 0, the position is plausible (mpe_relink_batch).  It goes right after Tracker.update;
        its ids, not the tracker's, then go to the smoother, the skeleton, the body fit and the scorer.  bones as
        Engine.skeleton takes them; tid_cap: ids that have a record, 1 .. 4096; pcap: rows per frame when the poses are not
        this engine's; max_frames: frames per update (default: the engine's).  options: harness.relink.DEFAULTS names them
        (gate_m, min_gap, max_gap, min_samples, min_bones, max_bone_m, reach_m, reach_per_frame_m, used_joint_mask --
        default: the parameters' used joints --, joint_mask); the defaults are options, not findings."""
        return Relinker(self, mode, bones, tid_cap, self.pcap if pcap is None else int(pcap),
                        self.max_frames if max_frames is None else int(max_frames), options)

    def write_poses(self, poses, flags, n_persons, kind, ids=None, frame_start=0, scale=1.0, joint_mask=None):
        """The poses of B frames as a JSON document on the device (mpe_json_write_poses): one line per frame,
        {"frame": frame_start + f, "ids": [...], "bodies": [{"<j>": [x, y, z], ...}, ...]}, byte for byte what
        harness.write_poses.write_lines states with json.dumps.  kind 'est': f32 poses with person flags (what mlp3d
        returns); 'triang': f64 poses with joint flags (what triangulate returns); rows per frame are those of `poses`
        (the engine's Pcap or any other, up to 1024).  ids ([B,Pcap] int32, a tracker's or relinker's): written as "ids"
        when given.  Every coordinate is written as (double)x * scale (100.0: centimetres, the unit of bodies_3D);
        joint_mask: the joints to write (default: all).  Nothing is synchronised or read back here.  -> WrittenPoses"""
        if kind not in ('est', 'triang'):
            raise ValueError('kind must be est or triang')
        tri = kind == 'triang'
        if poses.dim() != 4 or not 1 <= int(poses.shape[1]) <= L.MPE_JSON_WRITE_MAX_PERSONS:
            raise ValueError('poses must be [B,Pcap,%d,3] with Pcap within 1 .. %d' % (self.J, L.MPE_JSON_WRITE_MAX_PERSONS))
        pcap = int(poses.shape[1])
        B = _check_pose_rows(self.J, pcap, tri, tri, poses, flags, n_persons, ids, device=self.device)
        if int(frame_start) < 0 or not np.isfinite(float(scale)):
            raise ValueError('frame_start must not be negative and scale must be finite')
        lib, dev = self.lib, self.device
        bound = int(lib.mpe_json_write_bound(B, pcap, self.J, int(ids is not None)))
        if bound >= 1 << 32:
            raise ValueError('%d frames of %d rows can take %d bytes; a call writes less than 2^32' % (B, pcap, bound))
        w = WrittenPoses()
        w.text = torch.zeros((bound + 16,), dtype=torch.uint8, device=dev)
        w.frame_off = torch.empty((B + 1,), dtype=torch.int64, device=dev)
        w.bodies_extent = torch.empty((B, 2), dtype=torch.uint32, device=dev)
        w.rows_written = torch.empty((B,), dtype=torch.int32, device=dev)
        w.status = torch.empty((B,), dtype=torch.int32, device=dev)
        w._total = torch.empty((2,), dtype=torch.int64, device=dev)
        scratch_bytes = int(lib.mpe_json_write_scratch_bytes(B, pcap, self.J))
        scratch = torch.empty((max(16, scratch_bytes),), dtype=torch.uint8, device=dev)
        a = L.mpe_json_write_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, pcap, self.J, int(tri), int(tri)
        a.joint_mask = (1 << self.J) - 1 if joint_mask is None else int(joint_mask)
        a.frame_start, a.scale = int(frame_start), float(scale)
        a.d_poses, a.d_flags, a.d_n_persons = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr()
        a.d_track_id = None if ids is None else ids.data_ptr()
        a.d_text, a.text_cap = w.text.data_ptr(), bound
        a.d_frame_off, a.d_bodies_extent, a.d_rows_written = w.frame_off.data_ptr(), w.bodies_extent.data_ptr(), w.rows_written.data_ptr()
        a.d_status, a.d_total = w.status.data_ptr(), w._total.data_ptr()
        a.d_scratch, a.scratch_bytes = scratch.data_ptr(), scratch_bytes
        self._chk(lib.mpe_json_write_poses(self.ctx, self._stream(), C.byref(a)))
        w._keep = (poses, flags, n_persons, ids, scratch)      # inputs and scratch stay alive until the caller has synchronised
        return w

    def json_write_launches(self):
        """Kernels this engine's context has queued for write_poses (counted on the host)."""
        n = C.c_int64(0)
        self._chk(self.lib.mpe_json_write_launches(self.ctx, C.byref(n)))
        return n.value

    def format_f64(self, values):
        """repr of every finite double of `values` (a device f64 tensor) on the device (mpe_format_f64) -> (slots [n,32]
        u8, zeroed behind the tokens, len [n] u8; 0 for an infinity or a NaN), device tensors."""
        if values.dtype != torch.float64 or values.dim() != 1 or not values.is_contiguous() or values.device != self.device:
            raise ValueError('values must be a contiguous float64 vector on %s' % self.device)
        n = int(values.shape[0])
        slots = torch.zeros((n, L.MPE_JSON_WRITE_SLOT_BYTES), dtype=torch.uint8, device=self.device)
        length = torch.empty((n,), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.mpe_format_f64(self.ctx, self._stream(), values.data_ptr(), n, slots.data_ptr(), length.data_ptr()))
        return slots, length

    def _pose_args(self, db, persons, n_persons, poses, flags, kind, joint_mask, kinds):
        """The argument checks reproject and refine share -> (B, tri, joint_mask)."""
        B = db.n_frames
        if kind not in kinds:
            raise ValueError('kind must be ' + ' or '.join((', '.join(kinds[:-1]), kinds[-1])))
        tri = kind == 'triang'
        _check_pose_rows(self.J, self.pcap, tri, tri, poses, flags, n_persons, B=B)
        if persons.dtype != torch.int32 or tuple(persons.shape) != (B, self.pcap, self.V) or not persons.is_contiguous():
            raise ValueError('persons must be int32 [%d,%d,%d], contiguous' % (B, self.pcap, self.V))
        if joint_mask is None:
            joint_mask = {'est': sum(1 << j for j in self.params.used_joints), 'triang': (1 << self.J) - 1,
                          'gt': 1 << int(list(self.params.joint_list)[-1])}[kind]
        return B, tri, int(joint_mask)

    def reproject(self, db, persons, n_persons, poses, flags, kind, joint_mask=None, threshold=0.5):
        """Reprojection residuals on the device (mpe_reproject_batch): how far every joint of every 3D pose lands from
        the 2D detection it came from, per camera -- a quality signal that needs no ground truth.  kind 'est': what mlp3d
        returned (f32 poses, person flags; the used joints); 'triang': what triangulate returned (f64 poses, joint flags;
        all joints); 'gt': f32 poses with person flags and the script's one GT joint (the last of joint_list).
        joint_mask overrides the kind's joints.  -> res [B,Pcap,V,J] f64 pixels, -1 where nothing is counted."""
        B, tri, joint_mask = self._pose_args(db, persons, n_persons, poses, flags, kind, joint_mask, ('est', 'triang', 'gt'))
        res = torch.empty((B, self.pcap, self.V, self.J), dtype=torch.float64, device=self.device)
        a = L.mpe_reproject_args()
        a.n_frames, a.pcap, a.n_joints = B, self.pcap, self.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), int(joint_mask), float(threshold)
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_res = res.data_ptr()
        self._chk(self.lib.mpe_reproject_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def refine(self, db, persons, n_persons, poses, flags, kind, joint_mask=None, threshold=0.5, max_iters=10, step_tol=1e-6,
               huber_px=0.0, out=None):
        """Every joint moved to the minimum of its reprojection cost over the cameras that saw it (mpe_refine_batch: one
        Levenberg-Marquardt problem of three unknowns per joint, binary64; include/mpe.h has the rule, harness/refine.py
        states it in numpy and the two agree bit for bit).  kind 'est': what mlp3d returned (f32 poses, person flags; the
        used joints); 'triang': what triangulate returned (f64 poses, joint flags; all joints); the observing cameras of
        a joint are the entries reproject would count.  huber_px > 0 bounds the pull of an outlying detection; out: the
        tensor that takes the poses (`poses` itself refines in place).  -> dict of device tensors: poses [B,Pcap,J,3] in
        the type of the input (joints that are not solved are copied through), status u8 (MPE_REFINE_* bits), cost0 /
        cost1 f64 (-1 where not solved), iters u8, n_views u8, all [B,Pcap,J]; one launch on the current stream.  The
        poses feed evaluate, reproject and Tracker.update like the ones that went in."""
        B, tri, joint_mask = self._pose_args(db, persons, n_persons, poses, flags, kind, joint_mask, ('est', 'triang'))
        if out is None:
            out = torch.empty_like(poses)
        elif out.dtype != poses.dtype or tuple(out.shape) != tuple(poses.shape) or not out.is_contiguous() or out.device != poses.device:
            raise ValueError('out must be a contiguous tensor of the type, shape and device of poses')
        shape = (B, self.pcap, self.J)
        res = {'poses': out, 'status': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'cost0': torch.empty(shape, dtype=torch.float64, device=self.device),
               'cost1': torch.empty(shape, dtype=torch.float64, device=self.device),
               'iters': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'n_views': torch.empty(shape, dtype=torch.uint8, device=self.device)}
        a = L.mpe_refine_args()
        a.n_frames, a.pcap, a.n_joints = B, self.pcap, self.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), joint_mask, float(threshold)
        a.max_iters, a.step_tol, a.huber_px = int(max_iters), float(step_tol), float(huber_px)
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_poses_out, a.d_status, a.d_cost0, a.d_cost1 = out.data_ptr(), res['status'].data_ptr(), res['cost0'].data_ptr(), res['cost1'].data_ptr()
        a.d_iters, a.d_n_views = res['iters'].data_ptr(), res['n_views'].data_ptr()
        self._chk(self.lib.mpe_refine_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def pose_covariance(self, db, persons, n_persons, poses, flags, kind, sigma_px, joint_mask=None, threshold=0.5, huber_px=0.0,
                        gate_m=0.0, flags_out=None):
        """How far every joint can be trusted (mpe_posecov_batch): its 3 x 3 covariance in metres^2 from the cameras that
        saw it, sigma_px^2 * A^-1 with A the normal matrix refine builds at that point (the Gauss-Newton approximation;
        with huber_px > 0 the usual weighted one, not the sandwich estimator; include/mpe.h has the rule,
        harness/uncertainty.py states it in numpy and the two agree bit for bit).  Arguments as for refine; sigma_px is the
        standard deviation of a detection in x and in y.  It is the covariance of the per-frame estimate: untimed, and
        silent on what smoothing or a bone fit do afterwards.  gate_m > 0 marks the computed joints whose sigma is larger
        (MPE_POSECOV_GATED); flags_out (kind 'triang' only: True for a new tensor, or a u8 tensor like flags, flags itself
        included) takes the flags with the gated joints cleared.  -> dict of device tensors: cov f64 [B,Pcap,J,6] in the
        order (00, 01, 02, 11, 12, 22), sigma f64 (metres; -1 where not computed), status u8 (MPE_POSECOV_* bits),
        n_views u8, all [B,Pcap,J], and flags when flags_out was given; one launch on the current stream."""
        B, tri, joint_mask = self._pose_args(db, persons, n_persons, poses, flags, kind, joint_mask, ('est', 'triang'))
        if flags_out is not None and flags_out is not False:
            if not tri:
                raise ValueError("flags_out needs kind 'triang': the gate clears joint flags, and kind 'est' has person flags")
            if flags_out is True:
                flags_out = torch.empty_like(flags)
            elif (flags_out.dtype != flags.dtype or tuple(flags_out.shape) != tuple(flags.shape) or not flags_out.is_contiguous()
                  or flags_out.device != flags.device):
                raise ValueError('flags_out must be a contiguous tensor of the type, shape and device of flags')
        else:
            flags_out = None
        shape = (B, self.pcap, self.J)
        res = {'cov': torch.empty(shape + (6,), dtype=torch.float64, device=self.device),
               'sigma': torch.empty(shape, dtype=torch.float64, device=self.device),
               'status': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'n_views': torch.empty(shape, dtype=torch.uint8, device=self.device)}
        a = L.mpe_posecov_args()
        a.n_frames, a.pcap, a.n_joints = B, self.pcap, self.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), joint_mask, float(threshold)
        a.huber_px, a.sigma_px, a.gate_m = float(huber_px), float(sigma_px), float(gate_m)
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_cov, a.d_sigma, a.d_status, a.d_n_views = res['cov'].data_ptr(), res['sigma'].data_ptr(), res['status'].data_ptr(), res['n_views'].data_ptr()
        if flags_out is not None:
            a.d_flags_out = flags_out.data_ptr()
            res['flags'] = flags_out
        self._chk(self.lib.mpe_posecov_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def refine_timed(self, db, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids, kind, lags, joint_mask=None,
                     threshold=0.5, max_iters=10, step_tol=1e-6, huber_px=0.0, out=None):
        """refine with every camera looking at the joint where its track says it was at that camera's time
        (mpe_refine_timed_batch; include/mpe.h has the rule, harness/refine_timed.py states it in numpy and the two agree
        bit for bit): what corrects the sub-frame lags LagEstimator.estimate reports.  db holds the detections of the
        table frames frame_start .. frame_start + db.n_frames - 1, persons [B,pcap,V] i32 their rows; the table (poses,
        flags, n_persons, ids of the whole sequence, of `kind` 'est' or 'triang' as LagEstimator.accumulate takes them; pcap
        is the table's) gives the start poses and, through the tracks, the offsets; lags: V floats, frames, with the sign
        of the lag report.  out: the tensor [B,pcap,J,3] that takes the poses; it must not share storage with table_poses.
        -> the dict of refine plus n_timed u8 [B,pcap,J] (observing cameras that used an offset); one launch on the
        current stream.  With every lag 0 the result is refine's on the call's frames of the table, bit for bit."""
        if kind not in ('est', 'triang'):
            raise ValueError('kind must be est or triang')
        tri, B = kind == 'triang', db.n_frames
        pcap = int(table_poses.shape[1]) if table_poses.dim() == 4 else -1
        n_table = _check_pose_rows(self.J, pcap, tri, tri, table_poses, table_flags, table_n_persons, table_ids, device=self.device)
        if persons.dtype != torch.int32 or tuple(persons.shape) != (B, pcap, self.V) or not persons.is_contiguous():
            raise ValueError('persons must be int32 [%d,%d,%d], contiguous' % (B, pcap, self.V))
        lags = [float(x) for x in lags]
        if len(lags) != self.V:
            raise ValueError('lags must be %d floats, one per camera' % self.V)
        if joint_mask is None:
            joint_mask = (1 << self.J) - 1 if tri else sum(1 << j for j in self.params.used_joints)
        if out is None:
            out = torch.empty((B, pcap, self.J, 3), dtype=table_poses.dtype, device=self.device)
        elif out.dtype != table_poses.dtype or tuple(out.shape) != (B, pcap, self.J, 3) or not out.is_contiguous() or out.device != table_poses.device:
            raise ValueError('out must be a contiguous tensor [%d,%d,%d,3] of the type and device of table_poses' % (B, pcap, self.J))
        elif out.numel() and out.untyped_storage().data_ptr() == table_poses.untyped_storage().data_ptr():
            raise ValueError('out must not share storage with table_poses: other frames read their neighbours from the table')
        shape = (B, pcap, self.J)
        res = {'poses': out, 'status': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'cost0': torch.empty(shape, dtype=torch.float64, device=self.device),
               'cost1': torch.empty(shape, dtype=torch.float64, device=self.device),
               'iters': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'n_views': torch.empty(shape, dtype=torch.uint8, device=self.device),
               'n_timed': torch.empty(shape, dtype=torch.uint8, device=self.device)}
        a = L.mpe_refine_timed_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, pcap, self.J, int(tri), int(tri)
        a.frame_start, a.n_table, a.joint_mask, a.threshold = int(frame_start), n_table, int(joint_mask), float(threshold)
        a.max_iters, a.step_tol, a.huber_px = int(max_iters), float(step_tol), float(huber_px)
        for c, x in enumerate(lags):
            a.lag[c] = x
        a.d_persons, a.d_poses, a.d_flags = persons.data_ptr(), table_poses.data_ptr(), table_flags.data_ptr()
        a.d_n_persons, a.d_tid = table_n_persons.data_ptr(), table_ids.data_ptr()
        a.d_poses_out, a.d_status, a.d_cost0, a.d_cost1 = out.data_ptr(), res['status'].data_ptr(), res['cost0'].data_ptr(), res['cost1'].data_ptr()
        a.d_iters, a.d_n_views, a.d_n_timed = res['iters'].data_ptr(), res['n_views'].data_ptr(), res['n_timed'].data_ptr()
        self._chk(self.lib.mpe_refine_timed_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def body_refine(self, sk, db, persons, n_persons, poses, flags, ids, sweeps=8, bone_weight=300.0, huber_px=0.0, joint_mask=None,
                    threshold=0.5, frames=None):
        """The body-level fit (mpe_body_refine_batch; include/mpe.h has the rule, harness/skeleton_refine.py states it in
        numpy and the two agree bit for bit): every row whose track has lengths in the Skeleton `sk` is fitted to the
        pixels and to the lengths together -- `sweeps` (1 .. 64) sweeps in which every free joint takes one
        Levenberg-Marquardt step on its reprojection error over the cameras that saw it plus bone_weight (pixels per metre)
        times the length error of its bones.  db: the batch the poses came from; persons [B,Pcap,V] / n_persons / poses / flags / ids: the pose rows of
        B frames and the rows' heads; frames: int32 [B] device tensor, the frame of db each pose frame is observed in
        (None: the poses have the frames of db, in order).  -> dict of device tensors: poses (a new tensor), status u8
        and n_views u8 [B,Pcap,J] (MPE_BODY_REFINE_* bits), cost f64 [B,Pcap,4] (pixel and bone part before, then after;
        -1 for a row that is not fitted), err f64 [B,Pcap,2], n_bones u8 [B,Pcap] as fit() returns them.  One launch on
        the current stream; the state of `sk` is not changed (its launch count goes up by one)."""
        if not isinstance(sk, Skeleton) or sk.eng is not self:
            raise ValueError('sk must be a Skeleton of this engine')
        if not 1 <= int(sweeps) <= L.MPE_SKEL_MAX_ITERS:
            raise ValueError('sweeps must be within 1 .. %d' % L.MPE_SKEL_MAX_ITERS)
        if not float(bone_weight) >= 0.0 or not float(huber_px) >= 0.0 or not float(threshold) >= 0.0:
            raise ValueError('bone_weight, huber_px and threshold must not be negative')
        base, B = sk._args(poses, flags, n_persons, ids, joint_mask)
        if persons.dtype != torch.int32 or tuple(persons.shape) != (B, sk.pcap, self.V) or not persons.is_contiguous() or persons.device != poses.device:
            raise ValueError('persons must be int32 [%d,%d,%d], contiguous, on the device of the poses' % (B, sk.pcap, self.V))
        if frames is None:
            if B != db.n_frames:
                raise ValueError('without frames the poses must have the %d frames of the batch' % db.n_frames)
        elif frames.dtype != torch.int32 or tuple(frames.shape) != (B,) or not frames.is_contiguous() or frames.device != poses.device:
            raise ValueError('frames must be int32 [%d], contiguous, on the device of the poses' % B)
        dev = self.device
        out = {'poses': torch.empty_like(poses), 'status': torch.empty((B, sk.pcap, self.J), dtype=torch.uint8, device=dev),
               'n_views': torch.empty((B, sk.pcap, self.J), dtype=torch.uint8, device=dev),
               'cost': torch.empty((B, sk.pcap, 4), dtype=torch.float64, device=dev),
               'err': torch.empty((B, sk.pcap, 2), dtype=torch.float64, device=dev),
               'n_bones': torch.empty((B, sk.pcap), dtype=torch.uint8, device=dev)}
        if B == 0:                           # nothing to do, and an empty frame map has no address to hand on
            return out
        a = L.mpe_body_refine_args()
        for k in ('n_frames', 'pcap', 'n_joints', 'pose_f64', 'joint_flags', 'joint_mask', 'd_poses', 'd_flags', 'd_n_persons', 'd_track_id'):
            setattr(a, k, getattr(base, k))
        a.sweeps, a.threshold, a.bone_weight, a.huber_px = int(sweeps), float(threshold), float(bone_weight), float(huber_px)
        a.d_persons, a.d_frame = persons.data_ptr(), None if frames is None else frames.data_ptr()
        a.d_poses_out, a.d_status, a.d_n_views, a.d_cost, a.d_err, a.d_n_bones = (out[k].data_ptr() for k in ('poses', 'status', 'n_views', 'cost',
                                                                                                               'err', 'n_bones'))
        self._chk(self.lib.mpe_body_refine_batch(self.ctx, self._stream(), sk.state, C.byref(db.struct), C.byref(a)))
        return out

    def regroup(self, db, persons, n_persons, poses, flags, kind, gate_px=15.0, clip_px=0.0, min_joints=3, joint_mask=None,
                threshold=0.5, release=True, attach=True, out=None):
        """The person proposals repaired by reprojection consistency (mpe_regroup_batch; include/mpe.h has the rule,
        harness/regroup.py states it in numpy and the two agree bit for bit): the mean pixel distance of every head of a
        frame from every person's projected pose, heads released from rows they miss by gate_px or more, free heads
        attached (least cost first) to rows that lack their camera.  kind and joint_mask as refine takes them; clip_px > 0
        bounds a joint's distance; a pair needs min_joints counting joints to be scored; out: the tensor that takes the
        rows (`persons` itself regroups in place).  -> dict of device tensors: persons [B,Pcap,V] i32, change [B,Pcap,V]
        u8 (0 kept, 1 released, 2 attached, 3 both), n_views [B,Pcap] i32, cost [n_heads,Pcap] f64 (-1: unscored), counts
        [B,4] i32 (released, attached, free heads, rows below min_views), status [B] i32 (MPE_REGROUP_* bits: such
        frames are copied through); one launch on the current stream.  The poses are not updated: run the 3D stage again
        on the new rows."""
        B, tri, joint_mask = self._pose_args(db, persons, n_persons, poses, flags, kind, joint_mask, ('est', 'triang'))
        if out is None:
            out = torch.empty_like(persons)
        elif out.dtype != persons.dtype or tuple(out.shape) != tuple(persons.shape) or not out.is_contiguous() or out.device != persons.device:
            raise ValueError('out must be a contiguous tensor of the type, shape and device of persons')
        i32 = dict(dtype=torch.int32, device=self.device)
        # a batch without heads has an empty table: its data_ptr() may be 0, and the entry point takes a NULL d_cost then
        res = {'persons': out, 'change': torch.empty((B, self.pcap, self.V), dtype=torch.uint8, device=self.device),
               'n_views': torch.empty((B, self.pcap), **i32),
               'cost': torch.empty((db.n_heads, self.pcap), dtype=torch.float64, device=self.device),
               'counts': torch.empty((B, 4), **i32), 'status': torch.empty((B,), **i32)}
        a = L.mpe_regroup_args()
        a.n_frames, a.pcap, a.n_joints = B, self.pcap, self.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), joint_mask, float(threshold)
        a.min_joints, a.gate_px, a.clip_px = int(min_joints), float(gate_px), float(clip_px)
        a.flags = (L.MPE_REGROUP_RELEASE if release else 0) | (L.MPE_REGROUP_ATTACH if attach else 0)
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_persons_out, a.d_change, a.d_n_views = out.data_ptr(), res['change'].data_ptr(), res['n_views'].data_ptr()
        a.d_cost, a.d_counts, a.d_status = res['cost'].data_ptr(), res['counts'].data_ptr(), res['status'].data_ptr()
        self._chk(self.lib.mpe_regroup_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def consolidate(self, db, persons, n_persons, poses, flags, kind, merge_m=0.10, found_m=0.05, clip_m=0.0, min_joints=3,
                    found_min_views=None, fcap=None, joint_mask=None, threshold=0.5, merge=True, found=True, out=None, n_out=None):
        """The two repairs regroup leaves open (mpe_consolidate_batch; include/mpe.h has the rule, harness/consolidate.py
        states it in numpy and the two agree bit for bit): rows whose poses lie within merge_m metres of each other (the
        tracker's cost) and share no camera are merged into the lower row, and the skeletons no row names found new rows
        where their rays pass within found_m metres of each other (the geometric matcher's distance, complete linkage).
        kind and joint_mask as refine takes them; a pair of rows or of skeletons needs min_joints common joints to be
        scored; clip_m > 0 bounds a joint's ray distance; found_min_views (default: max(2, the context's min_views)) heads
        a founded row needs; fcap (default: min(max_heads_per_frame, 64)) free skeletons per frame the founding takes;
        out / n_out: the tensors that take the rows and the row counts (`persons` / `n_persons` themselves consolidate in
        place).  The two gate defaults are options, not findings.  -> dict of device tensors: persons [B,Pcap,V] i32,
        n_persons [B] i32, change [B,Pcap,V] u8 (regroup's coding), n_views [B,Pcap] i32, dist [B,Pcap,Pcap] f64 and pair
        [B,fcap,fcap] f64 (-1: unscored), free [B,fcap] i32 (head id per rank), counts [B,4] i32 (rows merged away, rows
        founded, heads placed, heads left free), status [B] i32 (MPE_CONSOLIDATE_* bits); one launch on the current stream.
        A founded row has no pose: run the 3D stage again on the new rows and the new n_persons."""
        B, tri, joint_mask = self._pose_args(db, persons, n_persons, poses, flags, kind, joint_mask, ('est', 'triang'))
        if out is None:
            out = torch.empty_like(persons)
        elif out.dtype != persons.dtype or tuple(out.shape) != tuple(persons.shape) or not out.is_contiguous() or out.device != persons.device:
            raise ValueError('out must be a contiguous tensor of the type, shape and device of persons')
        if n_out is None:
            n_out = torch.empty_like(n_persons)
        elif n_out.dtype != n_persons.dtype or tuple(n_out.shape) != tuple(n_persons.shape) or not n_out.is_contiguous() or n_out.device != n_persons.device:
            raise ValueError('n_out must be a contiguous tensor of the type, shape and device of n_persons')
        if found_min_views is None:
            found_min_views = max(2, int(self.params.min_number_of_views))
        if fcap is None:
            fcap = max(1, min(self.hpf, L.MPE_CONSOLIDATE_MAX_FREE, L.MPE_CONSOLIDATE_RAY_DOUBLES // (3 * self.J + 1)))
        fcap = int(fcap)
        side = min(max(fcap, 0), L.MPE_CONSOLIDATE_MAX_FREE)         # (the entry point refuses an fcap outside 1..64)
        i32 = dict(dtype=torch.int32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        res = {'persons': out, 'n_persons': n_out, 'change': torch.empty((B, self.pcap, self.V), dtype=torch.uint8, device=self.device),
               'n_views': torch.empty((B, self.pcap), **i32), 'dist': torch.empty((B, self.pcap, self.pcap), **f64),
               'pair': torch.empty((B, side, side), **f64), 'free': torch.empty((B, side), **i32),
               'counts': torch.empty((B, 4), **i32), 'status': torch.empty((B,), **i32)}
        a = L.mpe_consolidate_args()
        a.n_frames, a.pcap, a.n_joints = B, self.pcap, self.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), joint_mask, float(threshold)
        a.min_joints, a.merge_m, a.found_m, a.clip_m = int(min_joints), float(merge_m), float(found_m), float(clip_m)
        a.found_min_views, a.fcap = int(found_min_views), fcap
        a.flags = (L.MPE_CONSOLIDATE_MERGE if merge else 0) | (L.MPE_CONSOLIDATE_FOUND if found else 0)
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_persons_out, a.d_n_persons_out, a.d_change, a.d_n_views = out.data_ptr(), n_out.data_ptr(), res['change'].data_ptr(), res['n_views'].data_ptr()
        a.d_dist, a.d_pair, a.d_free = res['dist'].data_ptr(), res['pair'].data_ptr(), res['free'].data_ptr()
        a.d_counts, a.d_status = res['counts'].data_ptr(), res['status'].data_ptr()
        self._chk(self.lib.mpe_consolidate_batch(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return res

    def calibrator(self, kind, huber_px=0.0, min_obs=50, hold=()):
        """A Calibrator for poses of `kind` ('est' or 'triang', as refine takes them): the camera extrinsics refined from
        a recording's own poses, the joints held fixed (mpe_calib_*; include/mpe.h has the rule, harness/calibrate.py
        states it in numpy).  huber_px > 0 bounds the pull of an outlying detection; a camera with fewer than min_obs
        (>= 6) observations is held, as are the cameras in `hold` (names or engine indices).  This engine's own
        calibration is never modified: Calibrator.calibration() gives the one to build the next engine from."""
        return Calibrator(self, kind, huber_px, min_obs, hold)

    def camera_fitter(self, kind, free=('pose', 'focal', 'centre', 'k1', 'k2', 'k3'), huber_px=0.0, min_obs=50, hold=()):
        """A CameraFitter for poses of `kind` ('est' or 'triang'): the calibrator with seven more unknowns per camera --
        fx, fy, cx, cy and the radial lens terms kd0, kd1, kd2 fitted together with the extrinsics from a recording's own
        poses (mpe_camfit_*; include/mpe.h has the rule, harness/camfit.py states it in numpy).  free: the groups that
        are unknowns; the others keep their values.  min_obs is at least the larger of 6 and the number of free unknowns.
        This engine's own calibration is never modified: CameraFitter.calibration() gives the one to build the next
        engine from."""
        return CameraFitter(self, kind, free, huber_px, min_obs, hold)

    def lag_estimator(self, kind, window=4, sub=4, huber_px=0.0, pcap=None, max_frames=None):
        """A LagEstimator for a table of tracked poses of `kind` ('est': f32 poses with per-row flags, 'triang': f64 poses
        with per-joint flags, as the calibrator takes them): how many frames every camera runs ahead of or behind the
        poses of the recording, on a grid of lags within +- `window` frames with `sub` entries per frame (mpe_lag_*;
        include/mpe.h has the rule, harness/lag.py states it in numpy).  huber_px > 0 bounds the pull of an outlying
        detection.  pcap: rows per frame (default: the engine's Pcap); max_frames: frames per accumulate() (default: the
        engine's)."""
        return LagEstimator(self, kind, window, sub, huber_px, self.pcap if pcap is None else int(pcap),
                            self.max_frames if max_frames is None else int(max_frames))

    def residual_stats(self, res_list):
        """Per-camera statistics of one or more residual tensors [..., V, J] f64 on the device (mpe_residual_stats): the
        exact middle elements by radix select, a sum reduced in a fixed order.  -> dict of numpy arrays over the cameras:
        count, nonfinite (int64), sum, mean, median (NaN for a camera without entries or with a NaN entry), mid [V,2]."""
        if isinstance(res_list, torch.Tensor):
            res_list = [res_list]
        res_list = list(res_list)
        for r in res_list:
            if r.dtype != torch.float64 or r.dim() < 2 or tuple(r.shape[-2:]) != (self.V, self.J) or not r.is_contiguous() or not r.is_cuda:
                raise ValueError('residual buffers must be contiguous float64 device tensors [..., %d, %d]' % (self.V, self.J))
        n = len(res_list)
        ptrs = (C.c_void_p * max(n, 1))(*[r.data_ptr() for r in res_list])
        groups = (C.c_int64 * max(n, 1))(*[r.numel() // (self.V * self.J) for r in res_list])
        cnt = torch.empty((2, self.V), dtype=torch.int64, device=self.device)
        val = torch.empty((3, self.V), dtype=torch.float64, device=self.device)          # sum | mid as [V][2]
        a = L.mpe_residual_stats_args()
        a.n_buffers, a.n_joints = n, self.J
        a.d_res, a.n_groups = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(groups, C.POINTER(C.c_int64))
        a.d_count, a.d_nonfinite = cnt[0].data_ptr(), cnt[1].data_ptr()
        a.d_sum, a.d_mid = val[0].data_ptr(), val[1].data_ptr()
        self._chk(self.lib.mpe_residual_stats(self.ctx, self._stream(), C.byref(a)))
        cnt, val = cnt.cpu().numpy(), val.cpu().numpy()
        out = {'count': cnt[0], 'nonfinite': cnt[1], 'sum': val[0], 'mid': val[1:].reshape(self.V, 2)}
        with np.errstate(all='ignore'):
            out['mean'] = np.where(out['count'] > 0, out['sum'] / np.maximum(out['count'], 1), np.nan)
            med = (out['mid'][:, 0] + out['mid'][:, 1]) / 2
        out['median'] = np.where(np.isnan(out['sum']), np.nan, med)
        return out

    def partition_labels(self, db, persons, n_persons, hcap=None):
        """One label per head of every frame on the device (mpe_partition_labels): the index of the first proposal that
        holds the head, else n_persons -- the rule of test/sm_metrics.py:211-218 (harness/partition.py:proposal_labels).
        -> dict of device tensors: labels [B,Hcap] i32 (-1 beyond the frame's heads), count [B] i32 (heads), status [B]."""
        B = db.n_frames
        if persons.dtype != torch.int32 or tuple(persons.shape) != (B, self.pcap, self.V) or not persons.is_contiguous():
            raise ValueError('persons must be contiguous int32 [%d,%d,%d]' % (B, self.pcap, self.V))
        if n_persons.dtype != torch.int32 or tuple(n_persons.shape) != (B,) or not n_persons.is_contiguous():
            raise ValueError('n_persons must be contiguous int32 [%d]' % B)
        hcap = max(1, int(hcap if hcap is not None else (db.host.max_heads_per_frame() if B else 1)))
        out = {'labels': torch.empty((B, hcap), dtype=torch.int32, device=self.device),
               'count': torch.empty((B,), dtype=torch.int32, device=self.device),
               'status': torch.empty((B,), dtype=torch.int32, device=self.device)}
        a = L.mpe_partition_labels_args()
        a.n_frames, a.pcap, a.hcap = B, self.pcap, hcap
        a.d_persons, a.d_n_persons = persons.data_ptr(), n_persons.data_ptr()
        a.d_labels, a.d_count, a.d_status = out['labels'].data_ptr(), out['count'].data_ptr(), out['status'].data_ptr()
        self._chk(self.lib.mpe_partition_labels(self.ctx, self._stream(), C.byref(db.struct), C.byref(a)))
        return out

    def group_bodies(self, packed, skip_in=None):
        """Ground-truth persons of every frame by greedy 3D proximity on the device (mpe_group_bodies; test/sm_metrics.py:
        125-157).  packed: harness.partition.pack_bodies' arrays, or ParsedBodies.packed() (device tensors, taken as they
        are); skip_in [B]: frames not to group.  -> dict of device
        tensors: labels [B,Scap] i32 (-1 beyond the frame's skeletons), count [B] i32 (skeletons), n_groups [B] i32,
        skip [B] u8 (no person, a body without '-1', or skip_in), status [B] i32."""
        B = len(packed['n'])
        scap, kcap = packed['xyz'].shape[1:3]
        if kcap > L.MPE_PART_MAX_KEYS:
            raise ValueError('%d distinct joint keys, at most %d' % (kcap, L.MPE_PART_MAX_KEYS))
        dev = self.device
        up = lambda v, dt: v.contiguous() if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v, dtype=dt)).to(dev)
        mask = packed['mask'] if isinstance(packed['mask'], torch.Tensor) else packed['mask'].view(np.int32)
        t = {'xyz': up(packed['xyz'], np.float64), 'mask': up(mask, np.int32), 'nkeys': up(packed['nkeys'], np.int32),
             'order': up(packed['order'], np.uint8), 'm1': up(packed['m1'], np.uint8), 'n': up(packed['n'], np.int32)}
        sk = up(np.asarray(skip_in).astype(np.uint8), np.uint8) if skip_in is not None else None
        out = {'labels': torch.empty((B, scap), dtype=torch.int32, device=dev), 'count': t['n'],
               'n_groups': torch.empty((B,), dtype=torch.int32, device=dev), 'skip': torch.empty((B,), dtype=torch.uint8, device=dev),
               'status': torch.empty((B,), dtype=torch.int32, device=dev)}
        a = L.mpe_group_bodies_args()
        a.n_frames, a.scap, a.kcap = B, scap, kcap
        a.d_xyz, a.d_mask, a.d_nkeys, a.d_order, a.d_m1, a.d_n = (t[k].data_ptr() for k in ('xyz', 'mask', 'nkeys', 'order', 'm1', 'n'))
        a.d_skip_in = sk.data_ptr() if sk is not None else None
        a.d_labels, a.d_n_groups, a.d_skip, a.d_status = (out[k].data_ptr() for k in ('labels', 'n_groups', 'skip', 'status'))
        self._chk(self.lib.mpe_group_bodies(self.ctx, self._stream(), C.byref(a)))
        out['_keep'] = (t, sk)                       # inputs stay alive until the caller has synchronised
        return out

    def partition_scores(self, labels_true, labels_pred, count, skip=None, count_true=None):
        """Adjusted Rand index, homogeneity, completeness and V-measure of two labelings per frame on the device
        (mpe_partition_scores): sklearn's numbers in the written summation order of harness/partition.py, bit for bit.
        labels_true [B,Lt] / labels_pred [B,Lp] i32 device tensors, count [B] i32 labels per frame; skip [B] u8 and
        count_true [B] i32 optional (a frame with skip set or with count_true != count is not scored).  -> (scores [B,4]
        f64, NaN rows for frames not scored, status [B] i32: MPE_PART_SKIPPED / MPE_PART_OVER_CAP)."""
        B = int(count.shape[0])
        for t, dt, name in ((labels_true, torch.int32, 'labels_true'), (labels_pred, torch.int32, 'labels_pred'), (count, torch.int32, 'count'),
                            (skip, torch.uint8, 'skip'), (count_true, torch.int32, 'count_true')):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or not t.is_cuda or t.shape[0] != B):
                raise ValueError('%s must be a contiguous %s device tensor over %d frames' % (name, dt, B))
        if labels_true.dim() != 2 or labels_pred.dim() != 2 or labels_true.shape[1] < 1 or labels_pred.shape[1] < 1:
            raise ValueError('labels must be [B, L >= 1]')
        if not self._log_table_set:
            lg = np.ascontiguousarray(log_table()[:DEVICE_ENTRIES])
            self._chk(self.lib.mpe_set_log_table(self.ctx, lg.ctypes.data_as(L.c_f64p), len(lg)))
            self._log_table_set = True
        scores = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        status = torch.empty((B,), dtype=torch.int32, device=self.device)
        a = L.mpe_partition_scores_args()
        a.n_frames, a.ld_true, a.ld_pred = B, labels_true.shape[1], labels_pred.shape[1]
        a.d_labels_true, a.d_labels_pred, a.d_count = labels_true.data_ptr(), labels_pred.data_ptr(), count.data_ptr()
        a.d_count_true = count_true.data_ptr() if count_true is not None else None
        a.d_skip = skip.data_ptr() if skip is not None else None
        a.d_scores, a.d_status = scores.data_ptr(), status.data_ptr()
        self._chk(self.lib.mpe_partition_scores(self.ctx, self._stream(), C.byref(a)))
        return scores, status

    def dlt_pairs(self, pts, cams):
        pts = torch.as_tensor(pts, dtype=torch.float64, device=self.device).contiguous()
        cams = torch.as_tensor(cams, dtype=torch.int32, device=self.device).contiguous()
        n = pts.shape[0]
        out = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        self._chk(self.lib.mpe_dlt_pairs(self.ctx, self._stream(), _ptr(pts), _ptr(cams), n, _ptr(out)))
        return out

    def set_precision(self, gat_acc64=False, mlp_acc64=True, mlp_bf16=False, gat_reduced=False, attn_fp16=False, mlp_split=None,
                      gat_split=None, mlp_max_accuracy=False, mlp_f64=False):
        """GAT: plain fp32 MFMA chain / f64 running sums / `attn_fp16` (BASELINE configs[4] as worded: the transformed
        features ft2 travel to the attention stage as fp16 rows, the GEMMs stay fp32) / `gat_reduced` (additionally
        bf16 MFMA for fc1/fc2); MLP: fp32 / f64 running sums (default, parity) / bf16 MFMA.  The reduced modes are
        never used on the parity path."""
        # gat_split (default True): fc1 / fc2 of the layers >= 1 in the split-bf16 form (fp32-accurate, bf16 matrix pipe);
        # gat_split=False = the fp32 MFMA of rounds 1-3.  Layer 0 always runs on the fp32 MFMA (head rows only).
        if gat_split is None:
            gat_split = not gat_reduced
        gat = 2 if gat_reduced else 3 if attn_fp16 else int(gat_acc64)
        if gat_split and gat != 2:
            gat = {0: 4, 1: 5, 3: 6}[gat]
        # The parity MLP (mlp_acc64=True, not bf16) has two forms of the same accuracy class: the library default
        # (mlp_split=None / True: fp32 operands as three bf16 planes, six products on the bf16 matrix pipe, f64 sums every
        # second K stage; csrc/gemm_sb16.hip) and the fp32 MFMA with f64 sums per stage of rounds 1-3 (mlp_split=False).
        # mlp_max_accuracy: the split form with an f64 flush after EVERY K stage (MLP mode 4): rms error of a launch 0.13-0.18
        # instead of 0.24-0.26 ulp of its output scale, the MLP launches ~7 % slower.
        if mlp_split is None:
            mlp_split = bool(mlp_acc64) and not mlp_bf16
        # mlp_f64: the f64-evaluated network (MLP mode 5; LeakyReLU slope as the decimal double, include/mpe.h): exact products, f64 accumulation on the f64 matrix pipe; several times slower.
        if mlp_max_accuracy and (mlp_bf16 or not mlp_split or mlp_f64):
            raise ValueError('mlp_max_accuracy is a mode of the split-bf16 MLP (mlp_acc64=True, not mlp_bf16, mlp_split not False)')
        if mlp_f64 and mlp_bf16:
            raise ValueError('mlp_f64 and mlp_bf16 exclude each other')
        self._chk(self.lib.mpe_set_precision(self.ctx, gat, 5 if mlp_f64 else 2 if mlp_bf16 else 4 if mlp_max_accuracy else 3 if mlp_split else int(mlp_acc64)))
        self._state['precision'] = (gat_acc64, mlp_acc64, mlp_bf16, gat_reduced, attn_fp16, mlp_split, gat_split, mlp_max_accuracy, mlp_f64)
        for e in self._siblings:
            e.set_precision(gat_acc64, mlp_acc64, mlp_bf16, gat_reduced, attn_fp16, mlp_split, gat_split, mlp_max_accuracy, mlp_f64)

    def linear(self, x, w, b, slope=None, acc64=False, split=False, split_f64=True, split_flush_per_stage=False, f64mm=False):
        """act(x @ w.T + b) through the MFMA GEMM (parity tests). x device [m,k]; w,b host.  split: the split-bf16
        arithmetic of csrc/gemm_sb16.hip."""
        w = _np32(w)
        b = _np32(b)
        n, k = w.shape
        dw, dbias, ldw = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._chk(self.lib.mpe_upload_linear(self.ctx, _f32p(w), _f32p(b), n, k, C.byref(dw), C.byref(dbias),
                                             C.byref(ldw)))
        try:
            m = x.shape[0]
            xp = torch.zeros((m, ldw.value), dtype=torch.float32, device=self.device)
            xp[:, :k] = x
            ldc = (n + 3) // 4 * 4
            y = torch.empty((m, ldc), dtype=torch.float32, device=self.device)
            self._chk(self.lib.mpe_linear(self.ctx, self._stream(), _ptr(xp), ldw.value, dw, ldw.value, dbias,
                                          _ptr(y), ldc, m, None, n, k, (0 if slope is None else 1) | (2 if acc64 else 0) | (4 if split else 0) | (0 if split_f64 else 8) | (16 if split_flush_per_stage else 0) | (32 if f64mm else 0),
                                          0.0 if slope is None else float(slope)))
            torch.cuda.synchronize(self.device)
            return y[:, :n].contiguous()
        finally:
            self.lib.mpe_free_device(self.ctx, dw)
            self.lib.mpe_free_device(self.ctx, dbias)

    # ---- profiling --------------------------------------------------------------------
    def profile(self, on, resume=False):
        """Per-GEMM HIP event pairs on/off.  resume=True keeps the records taken so far (sampling: events
        on every n-th batch only, since the event packets cost ~2 % of a step)."""
        self._chk(self.lib.mpe_profile_enable(self.ctx, (2 if resume else 1) if on else 0))

    def profile_read(self):
        ms, fl, n, tot = C.c_double(), C.c_double(), C.c_int64(), C.c_double()
        self._chk(self.lib.mpe_profile_read(self.ctx, C.byref(ms), C.byref(fl), C.byref(n), C.byref(tot)))
        out = {'gemm_ms': ms.value, 'gemm_flop': fl.value, 'gemm_launches': n.value}
        self._chk(self.lib.mpe_profile_read_split(self.ctx, C.byref(ms), C.byref(fl), C.byref(n)))
        out.update({'split_ms': ms.value, 'split_flop': fl.value, 'split_launches': n.value})    # MLP launches on the bf16 MFMA
        self._chk(self.lib.mpe_profile_read_bf16(self.ctx, C.byref(ms), C.byref(fl), C.byref(n)))
        out.update({'bf16_ms': ms.value, 'bf16_flop': fl.value, 'bf16_launches': n.value})       # plain bf16 launches (reduced modes)
        return out


def _check_pose_rows(J, pcap, tri, per_joint, poses, flags, n_persons, ids=None, B=None, device=None):
    """The tensors of the pose-row contract: poses f64 (tri) or f32 [B,pcap,J,3]; flags u8, [B,pcap,J]
    (per_joint) or [B,pcap]; n_persons i32 [B]; ids i32 [B,pcap] where a stage takes them; all contiguous, and on `device`
    where one is given.  B: the frames they must have (default: as many as poses has).  -> B"""
    if B is None:
        B = int(poses.shape[0]) if poses.dim() == 4 else -1
    want = torch.float64 if tri else torch.float32
    if poses.dtype != want or tuple(poses.shape) != (B, pcap, J, 3):
        raise ValueError('poses must be %s [%s,%d,%d,3]' % (want, 'B' if B < 0 else B, pcap, J))
    if flags.dtype != torch.uint8 or tuple(flags.shape) != ((B, pcap, J) if per_joint else (B, pcap)):
        raise ValueError('flags must be uint8 %s' % ('[B,Pcap,J], one per joint' if per_joint else '[B,Pcap], one per row'))
    if n_persons.dtype != torch.int32 or tuple(n_persons.shape) != (B,):
        raise ValueError('n_persons must be int32 [%d]' % B)
    if ids is not None and (ids.dtype != torch.int32 or tuple(ids.shape) != (B, pcap)):
        raise ValueError('ids must be int32 [%d,%d]' % (B, pcap))
    given = [t for t in (poses, flags, n_persons, ids) if t is not None]
    if not all(t.is_contiguous() for t in given):
        raise ValueError('poses, flags, n_persons and ids must be contiguous')
    if device is not None and any(t.device != device for t in given):
        raise ValueError('poses, flags, n_persons and ids must be on %s' % device)
    return B


class WrittenPoses:
    """Engine.write_poses' result, device tensors: text (uint8; the document, then zeros for at least 16 bytes),
    frame_off [B+1] i64 (line f is text[frame_off[f]:frame_off[f+1]]), bodies_extent [B,2] u32 (the "bodies" list of
    every line with its brackets, offsets into text), rows_written [B] i32, status [B] i32 (MPE_WRITE_NONFINITE: a
    flagged joint was dropped).  total_bytes and total_status (the OR of status) read two words back and synchronise;
    bytes() makes one copy of the document through pinned memory."""

    def _totals(self):
        if not hasattr(self, '_host_total'):
            self._host_total = [int(v) for v in self._total.cpu()]
            self._keep = None
            if self._host_total[1] & L.MPE_WRITE_CAPACITY:     # the bound is a bound: this is a defect, not an input
                raise RuntimeError('the document needs %d bytes, mpe_json_write_bound gave %d' % (self._host_total[0], self.text.numel() - 16))
        return self._host_total

    @property
    def total_bytes(self):
        return self._totals()[0]

    @property
    def total_status(self):
        return self._totals()[1]

    def bytes(self):
        n = self.total_bytes
        if n == 0:
            return b''
        host = torch.empty((n,), dtype=torch.uint8).pin_memory()
        host.copy_(self.text[:n])
        return host.numpy().tobytes()


class _DeviceState:
    """What the state objects below share: the opaque state `_prefix`_create made on the engine's device, its launch
    count, reset() and close().  `_noun` is the object's name in 'the ... is closed'."""
    _prefix = _noun = None

    def _create(self, eng, *args):
        self.eng, self.state = eng, C.c_void_p()
        eng._chk(getattr(eng.lib, self._prefix + '_create')(eng.ctx, *args, C.byref(self.state)))

    def _open(self):
        if not self.state:
            raise RuntimeError('the %s is closed' % self._noun)

    def launches(self):
        """Kernels this object has enqueued so far."""
        n = C.c_int64()
        self.eng._chk(getattr(self.eng.lib, self._prefix + '_launches')(self.eng.ctx, self.state, C.byref(n)))
        return n.value

    def reset(self):
        """Back to the state after creation: a new sequence or recording (ordered on the current stream)."""
        self.eng._chk(getattr(self.eng.lib, self._prefix + '_reset')(self.eng.ctx, self.eng._stream(), self.state))

    def close(self):
        if getattr(self, 'state', None) and self.eng.ctx:
            getattr(self.eng.lib, self._prefix + '_destroy')(self.eng.ctx, self.state)
        self.state = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tracker(_DeviceState):
    """Engine.tracker's object: the device state of one sequence (the detections of the last max_gap + 1 frames with
    their ids, and the id count).  Mode 'gt' takes the ground-truth arrays as they are -- f32 poses [B,Gcap,J,3] with
    joint flags [B,Gcap,J], pcap = Gcap -- and gives the GT bodies the identities the wire format does not carry.  update() takes the frames of the sequence in order, in chunks of any size; the ids
    do not depend on the chunking.  Everything stays on the device and on the current stream: update() neither
    synchronises nor reads anything back."""
    _prefix, _noun = 'mpe_track', 'tracker'

    def __init__(self, eng, mode, max_gap, gate, pcap):
        if mode not in ('mlp', 'tri', 'gt'):
            raise ValueError('mode must be mlp, tri or gt')
        if not gate > 0:
            raise ValueError('gate must be > 0')
        self.mode, self.max_gap, self.gate, self.pcap = mode, int(max_gap), float(gate), pcap
        self._issued = None
        self._create(eng, self.pcap, eng.J, self.max_gap, int(mode == 'tri'))

    def update(self, poses, flags, n_persons):
        """poses / flags / n_persons of the next B >= 0 frames, as mlp3d or triangulate returned them (shapes and types
        as Engine.evaluate takes them).  -> {'ids' [B,Pcap] i32 (-1: no detection), 'cost' [B,Pcap] f64 (the link's
        cost; -1.0 for a birth or no detection), 'gap' [B,Pcap] i32 (frames back to the parent; 0 birth, -1 no
        detection), 'issued' [1] i32 (ids issued so far)}, device tensors."""
        eng, tri = self.eng, self.mode == 'tri'
        per_joint = self.mode != 'mlp'                   # 'gt': f32 poses like 'mlp', per-joint flags like 'tri'
        self._open()
        B = _check_pose_rows(eng.J, self.pcap, tri, per_joint, poses, flags, n_persons, device=eng.device)
        dev = eng.device
        out = {'ids': torch.empty((B, self.pcap), dtype=torch.int32, device=dev),
               'cost': torch.empty((B, self.pcap), dtype=torch.float64, device=dev),
               'gap': torch.empty((B, self.pcap), dtype=torch.int32, device=dev)}
        if B:
            self._issued = torch.empty((1,), dtype=torch.int32, device=dev)
        elif self._issued is None:                       # nothing tracked yet: the count is 0
            self._issued = torch.zeros((1,), dtype=torch.int32, device=dev)
        out['issued'] = self._issued
        a = L.mpe_track_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, self.pcap, eng.J, int(tri), int(per_joint)
        a.used_joint_mask = sum(1 << j for j in eng.params.used_joints)
        a.gate = self.gate
        a.d_poses, a.d_flags, a.d_n_persons = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr()
        a.d_track_id, a.d_link_cost, a.d_link_gap, a.d_issued = (out[k].data_ptr() for k in ('ids', 'cost', 'gap', 'issued'))
        eng._chk(eng.lib.mpe_track_batch(eng.ctx, eng._stream(), self.state, C.byref(a)))
        return out

    def reset(self):
        """Start a new sequence (ordered on the current stream)."""
        super().reset()
        self._issued = None


class _CameraLM(_DeviceState):
    """What Calibrator and CameraFitter share (normal_state of csrc/api.hip, one algorithm at two sizes): trial cameras and
    `_sums` sums per camera on the device, the Levenberg-Marquardt state of the cameras in the library, `_unknowns` of them
    per camera; `_last` names the step sizes a report carries."""
    _sums = _unknowns = None
    _last = ('last_rot', 'last_trans')

    def __init__(self, eng, kind, huber_px, min_obs, hold):
        if kind not in ('est', 'triang'):
            raise ValueError('kind must be est or triang')
        if not huber_px >= 0.0:
            raise ValueError('huber_px must be >= 0')
        names = list(eng.params.used_cameras_skeleton_matching)
        idx = [names.index(h) if isinstance(h, str) else int(h) for h in hold]
        if any(not 0 <= i < eng.V for i in idx):
            raise ValueError('hold names cameras of the engine')
        self.kind, self.huber_px, self.min_obs = kind, float(huber_px), int(min_obs)
        self.hold_mask = sum(1 << i for i in set(idx))
        self._batch = getattr(eng.lib, self._prefix + '_batch')
        self._create(eng)

    def accumulate(self, db, persons, n_persons, poses, flags, joint_mask=None, threshold=0.5):
        """The observations of one batch added to the pass (arguments as Engine.refine takes them)."""
        self._open()
        eng = self.eng
        B, tri, joint_mask = eng._pose_args(db, persons, n_persons, poses, flags, self.kind, joint_mask, ('est', 'triang'))
        a = L.mpe_calib_args()
        a.n_frames, a.pcap, a.n_joints = B, eng.pcap, eng.J
        a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = int(tri), int(tri), joint_mask, float(threshold)
        a.huber_px = self.huber_px
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        eng._chk(self._batch(eng.ctx, eng._stream(), self.state, C.byref(db.struct), C.byref(a)))

    def read(self):
        """The sums of the pass so far (synchronises) -> {'acc' [V,28] f64 (the CameraFitter: [V,105]), 'n_obs' [V] i64,
        'n_skipped' [V] i64}."""
        self._open()
        eng = self.eng
        acc, n, k = np.zeros((eng.V, self._sums)), np.zeros(eng.V, np.int64), np.zeros(eng.V, np.int64)
        i64p = C.POINTER(C.c_int64)
        eng._chk(getattr(eng.lib, self._prefix + '_read')(eng.ctx, eng._stream(), self.state, acc.ctypes.data_as(L.c_f64p),
                                                          n.ctypes.data_as(i64p), k.ctypes.data_as(i64p)))
        return {'acc': acc, 'n_obs': n, 'n_skipped': k}

    def _step(self, a, rep):
        """`_prefix`_step with the filled step arguments -> the report struct as step()'s dictionary."""
        self._open()
        eng = self.eng
        a.min_obs, a.hold_mask = self.min_obs, self.hold_mask
        eng._chk(getattr(eng.lib, self._prefix + '_step')(eng.ctx, eng._stream(), self.state, C.byref(a), C.byref(rep)))
        cams = [rep.cam[c] for c in range(rep.n_cameras)]
        out = {k: np.array([getattr(c, k) for c in cams], np.int32) for k in ('status', 'passes')}
        out.update({k: np.array([getattr(c, k) for c in cams], np.int64) for k in ('n_obs', 'n_skipped')})
        out.update({k: np.array([getattr(c, k) for c in cams], np.float64) for k in ('cost_start', 'cost') + self._last})
        out['lambda'] = np.array([c.lambda_ for c in cams], np.float64)
        out['delta'] = np.array([list(c.delta) for c in cams], np.float64).reshape(-1, self._unknowns)
        out['all_done'] = bool(rep.all_done)
        return out

    def launches(self):
        self._open()
        return super().launches()

    def reset(self):
        """Start afresh from the engine's own cameras (the Calibrator: from their extrinsics)."""
        self._open()
        super().reset()


class Calibrator(_CameraLM):
    """Engine.calibrator's object: trial extrinsics and the 28 sums per camera on the device, the Levenberg-Marquardt
    state of the cameras in the library.  A pass is accumulate() over every batch of the recording, in any chunking (the
    sums are the same bits), then step(); passes repeat on the same batches and poses until the report says all_done.
    accumulate() stays on the current stream and neither synchronises nor reads back; step() synchronises."""
    _prefix, _noun = 'mpe_calib', 'calibrator'
    _sums, _unknowns = L.MPE_CALIB_SUMS, 6

    def step(self, rot_tol=1e-7, trans_tol=1e-6):
        """The end of a pass: per camera the pass is accepted or rejected and the next trial extrinsics are set
        (mpe_calib_step).  -> {'status' (MPE_CALIB_* bits), 'passes', 'n_obs', 'n_skipped', 'cost_start', 'cost',
        'lambda', 'last_rot', 'last_trans'} as arrays over the cameras, 'delta' [V,6] (the perturbation of the last trial
        built) and 'all_done'."""
        a = L.mpe_calib_step_args()
        a.rot_tol, a.trans_tol = float(rot_tol), float(trans_tol)
        return self._step(a, L.mpe_calib_report())

    def extrinsics(self):
        """-> (accepted [V,3,4], trial [V,3,4]) f64, in the engine's camera order."""
        self._open()
        eng = self.eng
        acc, tri = np.zeros((eng.V, 3, 4)), np.zeros((eng.V, 3, 4))
        eng._chk(eng.lib.mpe_calib_get_extrinsics(eng.ctx, self.state, acc.ctypes.data_as(L.c_f64p), tri.ctypes.data_as(L.c_f64p)))
        return acc, tri

    def calibration(self):
        """A new Calibration: the engine's, with the accepted extrinsics (Calibration.with_extrinsics)."""
        calib = self.eng.calib
        E = np.array(calib.P, np.float64)
        for i, cam in enumerate(self.eng.params.used_cameras_skeleton_matching):
            E[calib.index(cam)] = self.extrinsics()[0][i]
        return calib.with_extrinsics(E)

    def set_extrinsics(self, E):
        """Start afresh from E [V,3,4] (engine camera order): accepted = trial = E, the sums zeroed."""
        self._open()
        eng = self.eng
        E = np.ascontiguousarray(E, np.float64)
        if E.shape != (eng.V, 3, 4):
            raise ValueError('E must be [%d,3,4]' % eng.V)
        eng._chk(eng.lib.mpe_calib_set_extrinsics(eng.ctx, eng._stream(), self.state, E.ctypes.data_as(L.c_f64p)))


class CameraFitter(_CameraLM):
    """Engine.camera_fitter's object: the trial set (extrinsics, fx fy cx cy as float32, lens terms) and the 105 sums per
    camera on the device, the Levenberg-Marquardt state of the cameras in the library.  Used as the Calibrator is: a pass
    is accumulate() over every batch of the recording, in any chunking (the sums are the same bits), then step().
    accumulate() stays on the current stream and neither synchronises nor reads back; step() synchronises."""
    _prefix, _noun = 'mpe_camfit', 'camera fitter'
    _sums, _unknowns = L.MPE_CAMFIT_SUMS, L.MPE_CAMFIT_UNKNOWNS
    _last = _CameraLM._last + ('last_pix', 'last_lens')

    def __init__(self, eng, kind, free, huber_px, min_obs, hold):
        if isinstance(free, str):
            free = [g for g in free.split(',') if g]
        unknown = [g for g in free if g not in L.MPE_CAMFIT_GROUPS]
        if unknown or not free:
            raise ValueError('free names groups out of %s' % ', '.join(L.MPE_CAMFIT_GROUPS))
        self.free_mask = sum(L.MPE_CAMFIT_GROUPS[g] for g in set(free))
        super().__init__(eng, kind, huber_px, min_obs, hold)

    def step(self, rot_tol=1e-7, trans_tol=1e-6, pix_tol=1e-3, lens_tol=1e-7):
        """The end of a pass: per camera the pass is accepted or rejected and the next trial set is built
        (mpe_camfit_step).  -> Calibrator.step's keys with 'last_pix', 'last_lens' and 'delta' [V,13]."""
        a = L.mpe_camfit_step_args()
        a.rot_tol, a.trans_tol, a.pix_tol, a.lens_tol = float(rot_tol), float(trans_tol), float(pix_tol), float(lens_tol)
        a.free_mask = self.free_mask
        return self._step(a, L.mpe_camfit_report())

    def cameras(self):
        """-> (accepted, trial), each (E [V,3,4] f64, k [V,4] f32: fx fy cx cy, dist [V,5] f64), in the engine's camera order."""
        self._open()
        eng = self.eng
        sets = [(np.zeros((eng.V, 3, 4)), np.zeros((eng.V, 4), np.float32), np.zeros((eng.V, 5))) for _ in range(2)]
        ptrs = [p for E, k, d in sets for p in (E.ctypes.data_as(L.c_f64p), k.ctypes.data_as(L.c_f32p), d.ctypes.data_as(L.c_f64p))]
        eng._chk(eng.lib.mpe_camfit_get_cameras(eng.ctx, self.state, *ptrs))
        return sets[0], sets[1]

    def set_cameras(self, E, k, dist):
        """Start afresh from E [V,3,4], k [V,4] (fx fy cx cy, rounded to float32) and dist [V,5] (engine camera order):
        accepted = trial = these, the sums zeroed."""
        self._open()
        eng = self.eng
        E, k, dist = np.ascontiguousarray(E, np.float64), np.ascontiguousarray(k, np.float32), np.ascontiguousarray(dist, np.float64)
        if E.shape != (eng.V, 3, 4) or k.shape != (eng.V, 4) or dist.shape != (eng.V, 5):
            raise ValueError('E, k, dist must be [%d,3,4], [%d,4], [%d,5]' % (eng.V, eng.V, eng.V))
        eng._chk(eng.lib.mpe_camfit_set_cameras(eng.ctx, eng._stream(), self.state, E.ctypes.data_as(L.c_f64p), k.ctypes.data_as(L.c_f32p),
                                                dist.ctypes.data_as(L.c_f64p)))

    def calibration(self):
        """A new Calibration: the engine's, with the accepted extrinsics (Calibration.with_extrinsics) and then the accepted
        intrinsics and lens terms (Calibration.with_intrinsics)."""
        calib = self.eng.calib
        (Ea, ka, da), _ = self.cameras()
        E, k, dist = np.array(calib.P, np.float64), calib.intrinsics(), np.array(calib.dist, np.float64)
        for i, cam in enumerate(self.eng.params.used_cameras_skeleton_matching):
            at = calib.index(cam)
            E[at], k[at], dist[at] = Ea[i], ka[i], da[i]
        return calib.with_extrinsics(E).with_intrinsics(k, dist)


class LagEstimator(_DeviceState):
    """Engine.lag_estimator's object: per camera the cost of every grid lag and the counts on the device.  A pass is
    accumulate() over every batch of the recording with the same table, in any chunking (the sums are the same bits), then
    estimate().  accumulate() stays on the current stream and neither synchronises nor reads back; read() and estimate()
    synchronise."""
    _prefix, _noun = 'mpe_lag', 'lag estimator'

    def __init__(self, eng, kind, window, sub, huber_px, pcap, max_frames):
        if kind not in ('est', 'triang'):
            raise ValueError('kind must be est or triang')
        if not 0 <= int(window) <= L.MPE_LAG_MAX_WINDOW or not 1 <= int(sub) <= L.MPE_LAG_MAX_SUB:
            raise ValueError('window must be within 0 .. %d and sub within 1 .. %d' % (L.MPE_LAG_MAX_WINDOW, L.MPE_LAG_MAX_SUB))
        if not huber_px >= 0.0:
            raise ValueError('huber_px must be >= 0')
        if int(max_frames) < 1:
            raise ValueError('max_frames must be at least 1')
        self.kind, self.window, self.sub, self.huber_px = kind, int(window), int(sub), float(huber_px)
        self.pcap, self.max_frames = int(pcap), int(max_frames)
        self.K = 2 * self.window * self.sub + 1
        self._keep = None
        cfg = L.mpe_lag_config()
        cfg.pcap, cfg.n_joints, cfg.window, cfg.sub = self.pcap, eng.J, self.window, self.sub
        cfg.pose_f64 = cfg.joint_flags = int(kind == 'triang')
        cfg.max_frames = self.max_frames
        self._create(eng, C.byref(cfg))

    def accumulate(self, db, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids, joint_mask=None, threshold=0.5):
        """The observations of one batch added to the pass: db holds the detections of the table frames frame_start ..
        frame_start + db.n_frames - 1, persons [B,Pcap,V] i32 their rows; the table (poses, flags, n_persons, ids of the
        whole sequence, as the sequence stages take them) is the same at every call of a pass."""
        self._open()
        eng, tri = self.eng, self.kind == 'triang'
        B = db.n_frames
        n_table = _check_pose_rows(eng.J, self.pcap, tri, tri, table_poses, table_flags, table_n_persons, table_ids, device=eng.device)
        if persons.dtype != torch.int32 or tuple(persons.shape) != (B, self.pcap, eng.V) or not persons.is_contiguous():
            raise ValueError('persons must be int32 [%d,%d,%d], contiguous' % (B, self.pcap, eng.V))
        if joint_mask is None:
            joint_mask = (1 << eng.J) - 1 if tri else sum(1 << j for j in eng.params.used_joints)
        a = L.mpe_lag_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, self.pcap, eng.J, int(tri), int(tri)
        a.frame_start, a.n_table, a.joint_mask, a.threshold, a.huber_px = int(frame_start), n_table, int(joint_mask), float(threshold), self.huber_px
        a.d_persons, a.d_poses, a.d_flags = persons.data_ptr(), table_poses.data_ptr(), table_flags.data_ptr()
        a.d_n_persons, a.d_tid = table_n_persons.data_ptr(), table_ids.data_ptr()
        eng._chk(eng.lib.mpe_lag_batch(eng.ctx, eng._stream(), self.state, C.byref(db.struct), C.byref(a)))
        self._keep = (db, persons, table_poses, table_flags, table_n_persons, table_ids)      # alive until the caller has synchronised

    def read(self):
        """The sums of the pass so far (synchronises) -> {'cost' [V,K] f64, 'n_obs' [V,K], 'n_skipped' [V,K], 'n_support'
        [V], 'n_unsupported' [V] i64}."""
        self._open()
        eng = self.eng
        out = {'cost': np.zeros((eng.V, self.K)), 'n_obs': np.zeros((eng.V, self.K), np.int64), 'n_skipped': np.zeros((eng.V, self.K), np.int64),
               'n_support': np.zeros(eng.V, np.int64), 'n_unsupported': np.zeros(eng.V, np.int64)}
        i64p = C.POINTER(C.c_int64)
        eng._chk(eng.lib.mpe_lag_read(eng.ctx, eng._stream(), self.state, out['cost'].ctypes.data_as(L.c_f64p),
                                      *(out[k].ctypes.data_as(i64p) for k in ('n_obs', 'n_skipped', 'n_support', 'n_unsupported'))))
        self._keep = None
        return out

    def estimate(self, min_obs=50):
        """The lag of every camera from the sums of the pass so far (mpe_lag_estimate; synchronises) -> {'status'
        (MPE_LAG_* bits), 'k_best' i32, 'lag_grid', 'lag_refined', 'cost_best', 'cost_zero' f64, 'n_obs', 'n_support',
        'n_unsupported' i64} as arrays over the cameras."""
        self._open()
        eng = self.eng
        rep = L.mpe_lag_report()
        eng._chk(eng.lib.mpe_lag_estimate(eng.ctx, eng._stream(), self.state, int(min_obs), C.byref(rep)))
        self._keep = None
        cams = [rep.cam[c] for c in range(rep.n_cameras)]
        out = {k: np.array([getattr(c, k) for c in cams], np.int32) for k in ('status', 'k_best')}
        out.update({k: np.array([getattr(c, k) for c in cams], np.float64) for k in ('lag_grid', 'lag_refined', 'cost_best', 'cost_zero')})
        out.update({k: np.array([getattr(c, k) for c in cams], np.int64) for k in ('n_obs', 'n_support', 'n_unsupported')})
        return out

    def launches(self):
        self._open()
        return super().launches()

    def reset(self):
        """The sums and the counts back to zero: a new pass (ordered on the current stream)."""
        self._open()
        super().reset()


class Smoother(_DeviceState):
    """Engine.smoother's object: the device state of one sequence (the raw poses, presence and ids of the last `window`
    frames).  update() takes the frames of the sequence in order, in chunks of any size, with the ids Tracker.update
    gave them; the result does not depend on the chunking.  Everything stays on the device and on the current stream:
    update() neither synchronises nor reads anything back."""
    _prefix, _noun = 'mpe_smooth', 'smoother'

    def __init__(self, eng, mode, window, decay, fill, pcap):
        if mode not in ('mlp', 'tri'):
            raise ValueError('mode must be mlp or tri')
        if not 0 <= int(window) <= L.MPE_SMOOTH_MAX_WINDOW:
            raise ValueError('window must be within 0 .. %d' % L.MPE_SMOOTH_MAX_WINDOW)
        if not 0.25 <= decay <= 1.0:
            raise ValueError('decay must be within [0.25, 1]')
        self.mode, self.window, self.decay, self.fill, self.pcap = mode, int(window), float(decay), bool(fill), pcap
        self._create(eng, self.pcap, eng.J, self.window, int(mode == 'tri'))

    def update(self, poses, flags, n_persons, ids, joint_mask=None):
        """poses / flags / n_persons of the next B >= 0 frames as Tracker.update took them, and the 'ids' it returned.
        joint_mask: the joints to process (default: all).  -> {'poses', 'flags' (the types and shapes of the inputs,
        new tensors; flags 2: a filled joint), 'vel' [B,Pcap,J,3] f64 (metres per frame), 'n_samples' [B,Pcap,J] u8
        (samples the window held)}, device tensors."""
        eng, tri = self.eng, self.mode == 'tri'
        self._open()
        B = _check_pose_rows(eng.J, self.pcap, tri, tri, poses, flags, n_persons, ids, device=eng.device)
        dev = eng.device
        out = {'poses': torch.empty_like(poses), 'flags': torch.empty_like(flags),
               'vel': torch.empty((B, self.pcap, eng.J, 3), dtype=torch.float64, device=dev),
               'n_samples': torch.empty((B, self.pcap, eng.J), dtype=torch.uint8, device=dev)}
        a = L.mpe_smooth_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.fill = B, self.pcap, eng.J, int(tri), int(tri), int(self.fill)
        a.joint_mask = (1 << eng.J) - 1 if joint_mask is None else int(joint_mask)
        a.lambda_ = self.decay
        a.d_poses, a.d_flags, a.d_n_persons, a.d_track_id = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr(), ids.data_ptr()
        a.d_poses_out, a.d_flags_out, a.d_vel, a.d_n_samples = (out[k].data_ptr() for k in ('poses', 'flags', 'vel', 'n_samples'))
        eng._chk(eng.lib.mpe_smooth_batch(eng.ctx, eng._stream(), self.state, C.byref(a)))
        return out

class Skeleton(_DeviceState):
    """Engine.skeleton's object: the device state of one sequence (a histogram of lengths per track id and bone, the
    length table, the counters).  observe() adds frames in any order and chunking, update() reads the lengths off the
    histograms, fit() moves poses towards the lengths of their tracks.  Everything stays on the device and on the
    current stream: only lengths() synchronises and reads back.  reset(): empty histograms, no lengths, counters at zero."""
    _prefix, _noun = 'mpe_skel', 'skeleton'

    def __init__(self, eng, mode, bones, bin_mm, tid_cap, pcap):
        from .harness import skeleton as S
        if mode not in ('mlp', 'tri'):
            raise ValueError('mode must be mlp or tri')
        if bones is None:
            if eng.J != 18:
                raise ValueError('bones must be given for %d joints (the default list is for 18)' % eng.J)
            bones = S.BONES_18
        self.bones = S.check_bones(bones, eng.J)
        if not (bin_mm > 0 and np.isfinite(bin_mm)):
            raise ValueError('bin_mm must be finite and > 0')
        if int(tid_cap) < 1 or int(tid_cap) * len(self.bones) * L.MPE_SKEL_BINS * 4 > L.MPE_SKEL_MAX_HIST_BYTES:
            raise ValueError('tid_cap must be within 1 .. %d for %d bones' % (L.MPE_SKEL_MAX_HIST_BYTES // (4 * L.MPE_SKEL_BINS * len(self.bones)),
                                                                            len(self.bones)))
        self.mode, self.bin_width, self.tid_cap, self.pcap = mode, float(bin_mm) / 1000.0, int(tid_cap), int(pcap)
        flat = np.ascontiguousarray(self.bones, np.int32)
        cfg = L.mpe_skel_config()
        cfg.pcap, cfg.n_joints, cfg.pose_f64, cfg.tid_cap, cfg.n_bones = self.pcap, eng.J, int(mode == 'tri'), self.tid_cap, len(self.bones)
        cfg.bin_width, cfg.bones = self.bin_width, flat.ctypes.data_as(L.c_i32p)
        self._create(eng, C.byref(cfg))

    def _args(self, poses, flags, n_persons, ids, joint_mask):
        eng, tri = self.eng, self.mode == 'tri'
        self._open()
        B = _check_pose_rows(eng.J, self.pcap, tri, tri, poses, flags, n_persons, ids, device=eng.device)
        a = L.mpe_skel_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, self.pcap, eng.J, int(tri), int(tri)
        a.joint_mask = (1 << eng.J) - 1 if joint_mask is None else int(joint_mask)
        a.d_poses, a.d_flags, a.d_n_persons, a.d_track_id = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr(), ids.data_ptr()
        return a, B

    def observe(self, poses, flags, n_persons, ids, joint_mask=None):
        """poses / flags / n_persons of B >= 0 frames as Tracker.update took them, and the 'ids' it returned: the length
        of every bone whose two joints are there (and inside joint_mask, default: all) goes into its track's histogram."""
        a, _ = self._args(poses, flags, n_persons, ids, joint_mask)
        self.eng._chk(self.eng.lib.mpe_skel_observe_batch(self.eng.ctx, self.eng._stream(), self.state, C.byref(a)))

    def update(self, min_samples=10):
        """The length table from the histograms as they stand: the lower median of every (track, bone) that has
        min_samples lengths or more, none for the others."""
        self.eng._chk(self.eng.lib.mpe_skel_update(self.eng.ctx, self.eng._stream(), self.state, int(min_samples)))

    def fit(self, poses, flags, n_persons, ids, iters=16, joint_mask=None):
        """`iters` (1 .. 64) sweeps over the bones of every row whose track has lengths.  -> {'poses' (the type and
        shape of the input, a new tensor), 'err' [B,Pcap,2] f64 (the row's worst bone-length error in metres before and
        after, -1 for a row that is not fitted), 'n_bones' [B,Pcap] u8 (bones held to a length)}, device tensors."""
        if not 1 <= int(iters) <= L.MPE_SKEL_MAX_ITERS:
            raise ValueError('iters must be within 1 .. %d' % L.MPE_SKEL_MAX_ITERS)
        a, B = self._args(poses, flags, n_persons, ids, joint_mask)
        dev = self.eng.device
        out = {'poses': torch.empty_like(poses), 'err': torch.empty((B, self.pcap, 2), dtype=torch.float64, device=dev),
               'n_bones': torch.empty((B, self.pcap), dtype=torch.uint8, device=dev)}
        a.iters = int(iters)
        a.d_poses_out, a.d_err, a.d_n_bones = (out[k].data_ptr() for k in ('poses', 'err', 'n_bones'))
        self.eng._chk(self.eng.lib.mpe_skel_fit_batch(self.eng.ctx, self.eng._stream(), self.state, C.byref(a)))
        return out

    def lengths(self):
        """The table as it stands (synchronises) -> {'len' [tid_cap, n_bones] f64 metres (an entry > 0 and finite is a
        length), 'count' i32 of the same shape (numpy), 'out_of_range', 'over_ids', 'status' (int)}."""
        n = (self.tid_cap, len(self.bones))
        table, count = np.empty(n, np.float64), np.empty(n, np.int32)
        ctr, status = (C.c_int64 * 2)(), C.c_int32()
        self.eng._chk(self.eng.lib.mpe_skel_get_lengths(self.eng.ctx, self.eng._stream(), self.state, table.ctypes.data, count.ctypes.data,
                                                        C.addressof(ctr), C.addressof(status)))
        return {'len': table, 'count': count, 'out_of_range': int(ctr[0]), 'over_ids': int(ctr[1]), 'status': int(status.value)}

    def set_lengths(self, table):
        """A caller's table [tid_cap, n_bones] (metres; an entry <= 0 or not finite: no length) in the place of the
        learned one, ordered on the current stream.  A host array is uploaded first."""
        self._open()
        if not isinstance(table, torch.Tensor):
            table = torch.from_numpy(np.ascontiguousarray(table, np.float64))
        if table.dtype != torch.float64 or tuple(table.shape) != (self.tid_cap, len(self.bones)):
            raise ValueError('the table must be float64 [%d,%d]' % (self.tid_cap, len(self.bones)))
        table = table.to(self.eng.device).contiguous()
        self.eng._chk(self.eng.lib.mpe_skel_set_lengths(self.eng.ctx, self.eng._stream(), self.state, table.data_ptr()))
        table.record_stream(torch.cuda.current_stream(self.eng.device))

class Relinker(_DeviceState):
    """Engine.relinker's object: the device state of one sequence (the canonical id of every tracker id seen, and per
    canonical id the frame and pose it was last seen in and the sums and counts of its bone lengths).  update() takes the
    frames of the sequence in order, in chunks of any size, with the ids Tracker.update gave them; the result does not
    depend on the chunking.  Everything stays on the device and on the current stream: update() neither synchronises nor
    reads anything back; counters() does both.  reset(): a new sequence."""
    _prefix, _noun = 'mpe_relink', 'relinker'

    def __init__(self, eng, mode, bones, tid_cap, pcap, max_frames, options):
        from .harness import relink as R, skeleton as S
        if mode not in ('mlp', 'tri'):
            raise ValueError('mode must be mlp or tri')
        if bones is None:
            if eng.J != 18:
                raise ValueError('bones must be given for %d joints (the default list is for 18)' % eng.J)
            bones = S.BONES_18
        self.bones = S.check_bones(bones, eng.J)
        options = dict(options)
        options.setdefault('used_joint_mask', sum(1 << j for j in eng.params.used_joints))
        self.options = o = R.check_options(dict(options, tid_cap=tid_cap), len(self.bones))
        if int(max_frames) < 1:
            raise ValueError('max_frames must be at least 1')
        self.mode, self.tid_cap, self.pcap, self.max_frames = mode, o['tid_cap'], int(pcap), int(max_frames)
        flat = np.ascontiguousarray(self.bones, np.int32)
        cfg = L.mpe_relink_config()
        cfg.pcap, cfg.n_joints, cfg.pose_f64, cfg.tid_cap, cfg.n_bones = self.pcap, eng.J, int(mode == 'tri'), self.tid_cap, len(self.bones)
        cfg.max_frames = self.max_frames
        cfg.min_gap, cfg.max_gap, cfg.min_samples, cfg.min_bones = o['min_gap'], o['max_gap'], o['min_samples'], o['min_bones']
        cfg.used_joint_mask, cfg.joint_mask = o['used_joint_mask'], o['joint_mask']
        cfg.gate_m, cfg.max_bone_m, cfg.reach_m, cfg.reach_per_frame_m = o['gate_m'], o['max_bone_m'], o['reach_m'], o['reach_per_frame_m']
        cfg.bones = flat.ctypes.data_as(L.c_i32p)
        self._create(eng, C.byref(cfg))

    def update(self, poses, flags, n_persons, ids):
        """poses / flags / n_persons of the next B >= 0 frames as Tracker.update took them, and the 'ids' it returned.
        -> {'ids' [B,Pcap] i32 (the canonical id; -1: no detection), 'link_cost' [B,Pcap] f64 (the bone-length cost of
        a link in metres; -1.0 for a row that is no linked birth), 'link_gap' [B,Pcap] i32 (frames since the record was
        last seen for a linked birth; 0 any other detection, -1 none)}, device tensors."""
        eng, tri = self.eng, self.mode == 'tri'
        self._open()
        B = _check_pose_rows(eng.J, self.pcap, tri, tri, poses, flags, n_persons, ids, device=eng.device)
        if B > self.max_frames:
            raise ValueError('%d frames, the relinker was made for %d per update' % (B, self.max_frames))
        dev = eng.device
        out = {'ids': torch.empty((B, self.pcap), dtype=torch.int32, device=dev),
               'link_cost': torch.empty((B, self.pcap), dtype=torch.float64, device=dev),
               'link_gap': torch.empty((B, self.pcap), dtype=torch.int32, device=dev)}
        a = L.mpe_relink_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = B, self.pcap, eng.J, int(tri), int(tri)
        a.d_poses, a.d_flags, a.d_n_persons, a.d_track_id = poses.data_ptr(), flags.data_ptr(), n_persons.data_ptr(), ids.data_ptr()
        a.d_ids, a.d_link_cost, a.d_link_gap = (out[k].data_ptr() for k in ('ids', 'link_cost', 'link_gap'))
        eng._chk(eng.lib.mpe_relink_batch(eng.ctx, eng._stream(), self.state, C.byref(a)))
        return out

    def counters(self):
        """The counters as they stand (synchronises) -> {'births' (tracks that began as themselves), 'linked' (births that
        took a lost track's id), 'over_ids' (rows whose id has no record), 'status' (MPE_RELINK_OVER_IDS)}."""
        ctr, status = (C.c_int64 * 3)(), C.c_int32()
        self.eng._chk(self.eng.lib.mpe_relink_read(self.eng.ctx, self.eng._stream(), self.state, C.addressof(ctr), C.addressof(status)))
        return {'births': int(ctr[0]), 'linked': int(ctr[1]), 'over_ids': int(ctr[2]), 'status': int(status.value)}


class TrackScore(_DeviceState):
    """Engine.track_scorer's object: the device state of one recording (the totals, the per-identity carry, the
    identity x track table).  update() takes the frames in order, in chunks of any size; nothing depends on the chunking.
    Everything stays on the device and on the current stream: update() neither synchronises nor reads anything back;
    result() does both."""
    _prefix, _noun = 'mpe_track_score', 'track scorer'

    def __init__(self, eng, mode, threshold_mm, gid_cap, tid_cap, max_frames, gcap, pcap):
        if mode not in ('mlp', 'tri'):
            raise ValueError('mode must be mlp or tri')
        if not threshold_mm > 0:
            raise ValueError('threshold_mm must be > 0')
        self.mode, self.threshold_mm = mode, float(threshold_mm)
        self.gid_cap, self.tid_cap, self.max_frames, self.gcap, self.pcap = int(gid_cap), int(tid_cap), int(max_frames), int(gcap), int(pcap)
        self._status = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        self._create(eng, self.pcap, self.gcap, self.gid_cap, self.tid_cap, self.max_frames)

    def update(self, ev, flags, n_persons, track_ids, gt_ids, gt_valid, skip=None):
        """ev: Engine.evaluate's dict for the next B >= 0 frames ('assign', 'err', 'invalid', 'n_res', 'n_gt' are read);
        flags / n_persons: what Engine.evaluate took; track_ids [B,Pcap] i32: Tracker.update's 'ids' for the same rows;
        gt_ids [B,Gcap] i32 and gt_valid [B,Gcap] u8: identity (< 0: none) and validity of every GT row; skip [B] u8:
        frames to leave out.  -> {'frame_counts' [B,4] i32 (tp, fp, fn, idsw), 'match_tid' [B,Gcap] i32 (the matched
        track, -1 miss, -2 not counted), 'status' [1] i32 (sticky MPE_TRACK_SCORE_OVER_IDS)}, device tensors."""
        eng, tri = self.eng, self.mode == 'tri'
        self._open()
        B = int(track_ids.shape[0]) if track_ids.dim() == 2 else -1
        P, G = self.pcap, self.gcap
        want = {'flags': (flags, torch.uint8, (B, P, eng.J) if tri else (B, P)), 'n_persons': (n_persons, torch.int32, (B,)),
                'track_ids': (track_ids, torch.int32, (B, P)), 'gt_ids': (gt_ids, torch.int32, (B, G)),
                'gt_valid': (gt_valid, torch.uint8, (B, G)), 'assign': (ev['assign'], torch.int32, (B, P)),
                'err': (ev['err'], torch.float64, (B, P)), 'invalid': (ev['invalid'], torch.uint8, (B, P)),
                'n_res': (ev['n_res'], torch.int32, (B,)), 'n_gt': (ev['n_gt'], torch.int32, (B,))}
        if skip is not None:
            want['skip'] = (skip, torch.uint8, (B,))
        for k, (t, dt, shape) in want.items():
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != eng.device:
                raise ValueError('%s must be %s %s, contiguous, on %s' % (k, dt, list(shape), eng.device))
        dev = eng.device
        out = {'frame_counts': torch.empty((B, 4), dtype=torch.int32, device=dev),
               'match_tid': torch.empty((B, G), dtype=torch.int32, device=dev), 'status': self._status}
        a = L.mpe_track_score_args()
        a.n_frames, a.pcap, a.gcap, a.joint_flags, a.threshold_mm = B, P, G, int(tri), self.threshold_mm
        a.d_flags, a.d_n_persons, a.d_track_id = flags.data_ptr(), n_persons.data_ptr(), track_ids.data_ptr()
        a.d_assign, a.d_err, a.d_invalid = ev['assign'].data_ptr(), ev['err'].data_ptr(), ev['invalid'].data_ptr()
        a.d_n_res, a.d_n_gt, a.d_gt_id, a.d_gt_valid = ev['n_res'].data_ptr(), ev['n_gt'].data_ptr(), gt_ids.data_ptr(), gt_valid.data_ptr()
        a.d_skip = skip.data_ptr() if skip is not None else None
        a.d_frame_counts, a.d_match_tid, a.d_status = out['frame_counts'].data_ptr(), out['match_tid'].data_ptr(), self._status.data_ptr()
        eng._chk(eng.lib.mpe_track_score_batch(eng.ctx, eng._stream(), self.state, C.byref(a)))
        return out

    def result(self):
        """The totals and ratios of the recording so far (synchronises; the IDTP pairing runs on the host) -> dict:
        frames, n_gt, n_pred, tp, fp, fn, idsw, frag, ignored, over_ids, idtp, n_ids, n_tracks, mt, pt, ml, status
        (int); err_sum, mota, motp_mm, idp, idr, idf1 (float, NaN for a zero denominator)."""
        r = L.mpe_track_score_totals()
        self.eng._chk(self.eng.lib.mpe_track_score_result(self.eng.ctx, self.eng._stream(), self.state, C.byref(r)))
        return {k: getattr(r, k) for k, _ in r._fields_ if k != 'reserved'}

    def read_state(self):
        """The per-identity and per-track state (synchronises) -> numpy {'last', 'present', 'matched', 'bits' [gid_cap],
        'pred_count' [tid_cap], 'table' [gid_cap, tid_cap]} i32."""
        ident = np.empty((4, self.gid_cap), np.int32)
        pred, table = np.empty(self.tid_cap, np.int32), np.empty((self.gid_cap, self.tid_cap), np.int32)
        self.eng._chk(self.eng.lib.mpe_track_score_read(self.eng.ctx, self.eng._stream(), self.state, ident.ctypes.data, pred.ctypes.data,
                                                        table.ctypes.data))
        return {'last': ident[0], 'present': ident[1], 'matched': ident[2], 'bits': ident[3], 'pred_count': pred, 'table': table}

    def reset(self):
        """Start a new recording (ordered on the current stream)."""
        super().reset()
        self._status.zero_()


def explicit_m_cap(max_heads_per_frame):
    """Edge-nodes a frame of an explicit edge-node list may hold on a context of that capacity (include/mpe.h: the power of
    two >= max(512, hmax^2 / 2 + 1), the clustering scratch; 0 = mode unavailable)."""
    need, n = max_heads_per_frame * max_heads_per_frame // 2 + 1, 512
    while n < need:
        n <<= 1
    return n if max_heads_per_frame <= 1024 and max_heads_per_frame + n <= 65535 else 0


def _np32(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
