"""GPU: every golden frame of a rig in ONE batch of more than LAT_MAX_FRAMES frames, so that the arrays the reference itself
produced meet the batch kernels (tile GEMMs, k_gat_fused, the batch clustering launch, k_mlp_rows solving its own pairs,
k_person_scan) and not only the small-batch launches the one-frame golden tests take (csrc/api.hip: lat_gat_ok, LAT_MAX_FRAMES = 16).

Per rig the frames of all its cases (the random-shape case included) are concatenated -- 50 / 33 / 3 / 10 frames for panoptic /
arplab / arprobot / ring23 -- and sent in two orders: 'listed', and 'shuffled' = a seeded permutation with an empty frame {} and a
single-camera frame in the middle.  The list is repeated cyclically up to the batch length T of the case.  Every golden frame of the
batch is then held (golden_checks.py, the bounds of the one-frame tests on the same fixtures) against the reference's arrays, and bit
for bit against the one-frame call of the same engine; as both orders equal the one-frame call, they equal each other.

Batch length and capacity.  What the launch rules read is not the engine's max_frames (it sizes the workspaces and nothing else) but
  * the MLP: m_cap = n_frames of the BATCH x Pcap rows (mpe_mlp3d_batch -> mlp_chain).  An f64-sum layer of more than four 16-wide
    column tiles takes the tile kernel when ceil(m_cap / 16) > few_rows_tiles = 32 (widths >= 2048) or 48 (narrower ones)
    (gemm_sb16.hip: launch_linear_sb16 / linear_sb16_uses_tile_kernel); the 54-wide last layer is `narrow` and always K-split;
  * the GAT: m = the rows PRESENT (gat_layer_linear -> gat_linear).  Layers >= 1 run on n_heads + n_edge_nodes rows, tile kernel
    when ceil(m / 16) x ceil(n / 16) > 1024 (MPE_SKINNY_WAVES' default): n = 400 from 657 rows, 320 from 817, 150 from 1633.
    Layer 0 runs on the head rows: the grouped fc1 under the same product rule with n = F (linear_uses_tile_kernel), fc2 (K > 512,
    so f64 sums: gemm_form.h) under the MLP's rule, more than 48 row tiles = 769 heads;
  * the clustering: max_heads_per_frame, the same in every case here.
So a case is (batch length T, engine max_frames):
  tight   T = max(17, frames of the rig) + 2 -- the two places of the inserted frames, cyclic golden frames in 'listed' -- and
          max_frames = T.  panoptic 52, arplab 35, arprobot 19, ring23 19.
  roomy   T = the smallest length >= tight's at which every rule above chooses the tile kernel for the 'shuffled' batch (the one
          with fewer rows), from the rules as `routes` restates them.  The MLP needs T x Pcap > 768: T >= 31 (panoptic, Pcap 25),
          26 (arplab, 30), 257 (arprobot, 3), 23 (ring23, 34); layer 0's fc2 needs 769 heads: 817 in panoptic's 52 frames, 785 in
          47 frames of arplab, 772 in 30 of ring23, and arprobot has 1363 by then; 1633 node rows are there in each.  Hence
          panoptic 52 (the tight batch already qualifies), arplab 47 and ring23 30 (layer 0's fc2 decides), arprobot 257 (the MLP
          decides: its frames hold 8 ... 15 nodes).  max_frames = 2 T, capacity to spare as a production engine has, except
          ring23: T, no larger than the derivation asks (a frame of capacity is 2347 node rows of 4142 features there).
The derived lengths are asserted (test_roomy_lengths_follow_from_the_launch_rules) and so are the routes per case: roomy means tile
kernels everywhere; tight arplab keeps layer 0's fc2 on the K-split kernel, tight ring23 that and the 1024-wide MLP layers (646
rows, 41 row tiles: over 32, not over 48), tight arprobot everything on the wave-per-tile / K-split kernels.  (arprobot's one-frame
calls take the batch path's launches as well: its layer 0 is 362 wide and lat_gat_ok asks for more than 512.)

mpe_dense_rows is one graph per call by its contract (MPE_ERR_UNSUPPORTED otherwise, asserted here), so it is called per frame on the
batch engine; mpe_gat_layer takes a multi-frame batch (node rows frame by frame: heads, then edge-nodes) and is run layer by layer
on the whole batch."""
import numpy as np
import pytest
import torch

import golden_checks as gc
from conftest import FUZZ_CASES, VARIANT_CASES, env, load_case, oracle, pkg

pytestmark = pytest.mark.gpu

LAT_MAX_FRAMES = 16                    # csrc/api.hip
SKINNY_WAVES = 1024                    # csrc/gemm.hip, gemm_sb16.hip: 16 x 16 tiles up to which the wave-per-tile / K-split kernels run
N_FRAMES = {'panoptic': 50, 'arplab': 33, 'arprobot': 3, 'ring23': 10}
TIGHT = {'panoptic': 52, 'arplab': 35, 'arprobot': 19, 'ring23': 19}
ROOMY = {'panoptic': 52, 'arplab': 47, 'arprobot': 257, 'ring23': 30}
CASES = [(v, c, o) for v in VARIANT_CASES for c in ('tight', 'roomy') for o in ('listed', 'shuffled')]


def _tiles(n):
    return (n + 15) // 16


def routes(n_frames, n_heads, n_nodes, pcap, gat_dims, mlp_widths, num_feats):
    """The launch rules of the module docstring -> {launch: takes the tile kernel}."""
    r = {}
    rows = _tiles(n_frames * pcap)
    for i, n in enumerate(mlp_widths):
        nt = _tiles(n)
        if nt <= 4:                                         # narrow: K-split at any batch size
            continue
        r['mlp%d' % i] = rows * nt > SKINNY_WAVES and rows > (32 if nt >= 128 else 48)
    # layer 0 runs on the head rows: the grouped fc1 (fp32 MFMA), fc2 with f64 sums (K > 512) and so under the MLP's rule
    heads, nt = _tiles(n_heads), _tiles(gat_dims[0][1] * gat_dims[0][2])
    r['gat0_fc1'] = heads * _tiles(num_feats) > SKINNY_WAVES
    r['gat0_fc2'] = heads * nt > SKINNY_WAVES and heads > (32 if nt >= 128 else 48)
    for l, (in_dim, nh, od) in enumerate(gat_dims):
        if l == 0:
            continue
        r['gat%d_fc1' % l] = _tiles(n_nodes) * _tiles(in_dim) > SKINNY_WAVES
        if nh * od > 16:                                    # (the last layer's one output column is `narrow`: wave per tile always)
            r['gat%d_fc2' % l] = _tiles(n_nodes) * _tiles(nh * od) > SKINNY_WAVES
    return r


class Rig:
    """The golden frames of one variant, the two special frames, and the engines / one-frame baselines built on them."""

    def __init__(self, variant):
        self.variant = variant
        self.env = env(variant)
        onp = oracle()
        self.frames, self.ref = [], []                      # processed frame, (arrays of its case, key prefix, wire frame)
        for name in list(VARIANT_CASES[variant]) + [n for v, n in FUZZ_CASES if v == variant]:
            arr, frames = load_case(name, variant)
            for n, fr in enumerate(frames):
                self.frames.append(onp.processed_input(fr))
                self.ref.append((arr, 'f%d_' % n, fr))
        assert len(self.frames) == N_FRAMES[variant]
        first = next(f for f in self.frames if f)
        cam = next(iter(first))
        self.special = {'empty': {}, 'one_cam': {cam: first[cam]}}     # as test_ragged_and_empty_frames builds them
        self.ppc = 10 if variant in ('panoptic', 'arplab') else 3
        self.engines, self.base = {}, {}
        pb = pkg('packing').pack_frames(self.frames + [self.special['one_cam']], self.env.params)
        self.counts = [pb.frame_counts(f) for f in range(pb.n_frames)]      # (h0, H, e0, M) per golden frame, then of one_cam

    def batch(self, T, order):
        """-> the batch's entries: an index into the golden list, or 'empty' / 'one_cam'."""
        G = len(self.frames)
        if order == 'listed':
            return [i % G for i in range(T)]
        cyc = [i % G for i in range(T - 2)]
        perm = np.random.default_rng(20 + G).permutation(T - 2)
        out = [cyc[i] for i in perm]
        mid = len(out) // 2
        return out[:mid] + ['empty', 'one_cam'] + out[mid:]

    def totals(self, entries):
        H = sum(self.counts[-1 if e == 'one_cam' else e][1] for e in entries if e != 'empty')
        M = sum(self.counts[e][3] for e in entries if not isinstance(e, str))
        return H, H + M

    def routes(self, entries):
        H, N = self.totals(entries)
        par = self.env.params
        pcap = len(par.used_cameras_skeleton_matching) * self.ppc // par.min_number_of_views       # Engine.pcap
        widths = [w.shape[0] for k, w in sorted(self.env.mlp.items(), key=lambda kv: int(kv[0].split('.')[1])) if k.endswith('weight')]
        sd, prm = self.env.gat
        heads = list(prm['heads']) + [1]
        dims = [(sd['layers.%d.fc1.weight' % l].shape[1], heads[l], sd['layers.%d.fc2.weight' % l].shape[0] // heads[l])
                for l in range(prm['gnn_layers'])]                                                   # Engine.gat_dims
        return routes(len(entries), H, N, pcap, dims, widths, self.env.meta['num_feats'])

    def engine(self, capacity):
        if capacity not in self.engines:
            T = (TIGHT if capacity == 'tight' else ROOMY)[self.variant]
            mf = T if capacity == 'tight' or self.variant == 'ring23' else 2 * T
            eng = pkg('pipeline').Engine(self.env.params, self.env.calib, max_frames=mf, max_persons_per_camera=self.ppc)
            eng.load_gat(*self.env.gat)
            eng.load_mlp(self.env.mlp)
            self.engines[capacity] = eng
        return self.engines[capacity]

    def stages(self, eng, frames, layers=False):
        """Every stage on one pack of `frames` -> (db, dict of host arrays)."""
        db = eng.to_device(eng.pack(frames))
        r = {'feat': eng.head_features(db)}
        r['sc'], r['sh'] = eng.gat_scores(db, heads=True)
        sc2, r['persons'], r['n'] = eng.match(db)
        r['rows'], r['valid'] = eng.mlp_input_rows(db, r['persons'], r['n'])
        r['poses'], r['pvalid'] = eng.mlp3d(db, r['persons'], r['n'])
        r['tri'], r['jv'] = eng.triangulate(db, r['persons'], r['n'])
        eng.sync_status()
        assert torch.equal(sc2, r['sc'])                  # match's scores are gat_scores'
        rows_dev = r['rows']
        return db, {k: v.cpu().numpy() for k, v in r.items()}, rows_dev

    def baseline(self, capacity):
        """The one-frame call of every golden frame and of the single-camera frame on the engine of `capacity`: once per engine,
        shared by the orders.  Also the dense rows of every frame (one graph per call), held against the reference here."""
        if capacity not in self.base:
            eng = self.engine(capacity)
            F = self.env.meta['num_feats']
            base = {}
            for key, frame in list(enumerate(self.frames)) + [('one_cam', self.special['one_cam'])]:
                db, r, _ = self.stages(eng, [frame])
                r['dense'] = eng.dense_rows(db).cpu().numpy() if db.n_heads else np.zeros((0, F), np.float32)
                if not isinstance(key, str):
                    arr, p, _ = self.ref[key]
                    if (p + 'N') in arr and int(arr[p + 'N']) and db.n_heads + db.n_edge_nodes:
                        gc.dense_rows(r['dense'], arr, p, F)
                base[key] = r
            self.base[capacity] = base
        return self.base[capacity]

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines.clear()
        self.base.clear()


_rigs = {}


def rig(variant):
    if variant not in _rigs:
        _rigs[variant] = Rig(variant)
    return _rigs[variant]


@pytest.fixture(scope='module', autouse=True)
def _close_rigs():
    yield
    for r in _rigs.values():
        r.close()
    _rigs.clear()


def _note(variant, capacity, order, worst):
    """The largest deviations from the golden arrays, printed as a record (pytest -s; profiles/golden_batched_routes.txt holds one
    run's); nothing is asserted about them beyond the bounds of golden_checks.py."""
    print('%-9s %-6s %-9s %s' % (variant, capacity, order, ' '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('variant', list(VARIANT_CASES))
def test_roomy_lengths_follow_from_the_launch_rules(variant):
    """ROOMY[variant] is the smallest batch length >= TIGHT[variant] at which every GEMM of the 'shuffled' batch takes its tile
    kernel, TIGHT is max(17, frames) + 2, and both orders of both lengths are batches of more than LAT_MAX_FRAMES frames."""
    g = rig(variant)
    assert TIGHT[variant] == max(LAT_MAX_FRAMES + 1, N_FRAMES[variant]) + 2
    T = TIGHT[variant]
    while not all(g.routes(g.batch(T, 'shuffled')).values()):
        T += 1
        assert T < 2000
    assert T == ROOMY[variant], (T, g.routes(g.batch(T - 1, 'shuffled')))
    assert all(g.routes(g.batch(T, 'listed')).values())
    tight = [k for k, v in g.routes(g.batch(TIGHT[variant], 'shuffled')).items() if not v]
    slow_mlp = ['mlp%d' % i for i in (4, 5, 6, 7)]
    assert sorted(tight) == sorted({'panoptic': [], 'arplab': ['gat0_fc2'], 'ring23': slow_mlp + ['gat0_fc2']}.get(variant, tight)), tight
    if variant == 'arprobot':       # 57 rows, 95 heads, 223 nodes
        assert len(tight) == len(g.routes(g.batch(TIGHT[variant], 'shuffled')))


@pytest.mark.parametrize('variant,capacity,order', CASES)
def test_golden_frames_in_one_batch(variant, capacity, order):
    g = rig(variant)
    eng = g.engine(capacity)
    base = g.baseline(capacity)
    T = (TIGHT if capacity == 'tight' else ROOMY)[variant]
    entries = g.batch(T, order)
    frames = [g.special[e] if isinstance(e, str) else g.frames[e] for e in entries]
    db, r, rows_dev = g.stages(eng, frames)
    assert db.n_frames == T and db.n_frames > LAT_MAX_FRAMES          # LAT_MAX_FRAMES = 16 (csrc/api.hip): the batch route
    assert eng.max_frames >= T and (capacity == 'roomy' or eng.max_frames == T)
    if capacity == 'roomy':
        assert all(g.routes(entries).values())
    assert set(e for e in entries if not isinstance(e, str)) == set(range(len(g.frames)))       # every golden frame is there
    F = g.env.meta['num_feats']
    worst = {'scores': 0.0, 'rows': 0.0, 'tri': 0.0, 'poses': 0.0}
    first_copy = {}
    for f, e in enumerate(entries):
        h0, H, e0, M = db.host.frame_counts(f)
        n = int(r['n'][f])
        if e == 'empty':
            assert H == 0 and M == 0 and n == 0 and not r['valid'][f].any() and not r['pvalid'][f].any()
            assert not r['poses'][f].any() and not r['jv'][f].any() and not r['tri'][f].any()
            continue
        b = base[e]
        # ---- bit for bit: the one-frame call of the same engine (and with it every other copy of the frame, and the other order)
        assert n == int(b['n'][0]), (f, e)
        assert np.array_equal(r['feat'][h0:h0 + H], b['feat']), (f, e)
        assert np.array_equal(r['sc'][e0:e0 + M], b['sc']), (f, e, np.abs(r['sc'][e0:e0 + M] - b['sc']).max())
        if M:           # (heads of a frame without a cross-camera pair belong to no graph, metrics_from_model.py:195-196: their score slots are unspecified)
            assert np.array_equal(r['sh'][h0:h0 + H], b['sh']), (f, e, np.abs(r['sh'][h0:h0 + H] - b['sh']).max())
        for k in ('persons', 'rows', 'valid', 'pvalid', 'poses', 'tri', 'jv'):
            assert np.array_equal(r[k][f], b[k][0]), (k, f, e)
        if e in first_copy:
            f1 = first_copy[e]
            for k in ('persons', 'n', 'rows', 'valid', 'poses', 'tri', 'jv'):
                assert np.array_equal(r[k][f], r[k][f1]), (k, f, f1)
        first_copy.setdefault(e, f)
        if e == 'one_cam':
            # heads but no cross-camera pair: no graph (metrics_from_model.py:195-196), nothing comes back
            assert H > 0 and n == 0 and M == 0 and not r['valid'][f].any() and not r['pvalid'][f].any()
            assert not r['poses'][f].any() and not r['jv'][f].any() and not r['tri'][f].any()
            continue
        # ---- the reference's arrays, with the bounds of the one-frame tests
        arr, p, wire = g.ref[e]
        gc.head_features(r['feat'][h0:h0 + H], db.host.head_cam[h0:h0 + H], arr, p, F)
        gc.gat_scores(r['sc'][e0:e0 + M], r['sh'][h0:h0 + H], arr, p)
        want = arr[p + 'scores']
        if len(want):
            worst['scores'] = max(worst['scores'], float(np.abs(np.concatenate([r['sh'][h0:h0 + H], r['sc'][e0:e0 + M]]) - want).max()))
        people = gc.persons(r['persons'][f], n, arr, p)
        if len(people) == 0:
            continue
        gc.mlp_rows(r['rows'][f], r['valid'][f], arr, p, n)
        worst['rows'] = max(worst['rows'], float(np.abs(r['rows'][f][:n] - arr[p + 'mlp_in']).max()))
        if first_copy[e] == f:                              # (further copies have the first copy's bits, asserted above)
            worst['poses'] = max(worst['poses'], gc.poses(eng, variant, arr, p, rows_dev[f], r['poses'][f], n))
        d = gc.triangulation(wire, arr, p, r['tri'][f], r['jv'][f], n)
        if d is not None:
            worst['tri'] = max(worst['tri'], d)
    _note(variant, capacity, order, worst)



@pytest.mark.parametrize('variant,capacity', [(v, c) for v in VARIANT_CASES for c in ('tight', 'roomy')])
def test_gat_layers_of_one_batch_vs_reference_activations(variant, capacity):
    """mpe_gat_layer on the whole 'shuffled' batch, layer by layer on the reference graphs' own feature rows (node order: frame by
    frame, heads then edge-nodes; the single-camera frame's rows from mpe_dense_rows): per golden frame the hidden activations the
    REFERENCE kept (act{l}_head / act{l}_en) at 2e-5 relative and the last layer's scores at 3e-5, as
    test_gat_layers_vs_reference_activations holds them one frame at a time."""
    g = rig(variant)
    eng = g.engine(capacity)
    base = g.baseline(capacity)
    T = (TIGHT if capacity == 'tight' else ROOMY)[variant]
    entries = g.batch(T, 'shuffled')
    db = eng.to_device(eng.pack([g.special[e] if isinstance(e, str) else g.frames[e] for e in entries]))
    F = g.env.meta['num_feats']
    n_layers = g.env.gat[1]['gnn_layers']
    x = np.zeros((db.n_heads + db.n_edge_nodes, F), np.float32)
    off = []
    for f, e in enumerate(entries):
        h0, H, e0, M = db.host.frame_counts(f)
        off.append(h0 + e0)
        if e == 'empty':
            continue
        if e == 'one_cam' or (g.ref[e][1] + 'N') not in g.ref[e][0] or int(g.ref[e][0][g.ref[e][1] + 'N']) != H + M:
            x[h0 + e0:h0 + e0 + H + M] = base[e]['dense']
        else:
            x[h0 + e0:h0 + e0 + H + M] = gc.dense_features(g.ref[e][0], g.ref[e][1], F)
    x = torch.from_numpy(x).cuda()
    checked = 0
    for l in range(n_layers - 1):
        x = eng.gat_layer(db, l, x, activation=0)
        got = x.cpu().numpy()
        for f, e in enumerate(entries):
            h0, H, e0, M = db.host.frame_counts(f)
            if isinstance(e, str) or (g.ref[e][1] + 'act%d_head' % l) not in g.ref[e][0] or M == 0:
                continue
            gc.layer_activations(got[off[f]:off[f] + H + M], H, g.ref[e][0], g.ref[e][1], l)
            checked += 1
    sc = eng.gat_layer(db, n_layers - 1, x, activation=1).cpu().numpy().reshape(-1)
    eng.sync_status()
    for f, e in enumerate(entries):
        h0, H, e0, M = db.host.frame_counts(f)
        if not isinstance(e, str) and M:
            np.testing.assert_allclose(sc[off[f]:off[f] + H + M], g.ref[e][0][g.ref[e][1] + 'scores'], rtol=0, atol=gc.LAYER_SCORES_ATOL)
    assert checked >= (n_layers - 1) * min(len(g.frames), 3)


def test_dense_rows_is_one_graph_per_call():
    """The contract the module docstring relies on: a multi-frame batch is refused, not answered in some other row order."""
    g = rig('arprobot')
    eng = g.engine('tight')
    db = eng.to_device(eng.pack(g.frames[:2]))
    with pytest.raises(pkg('lib').MpeError) as ei:
        eng.dense_rows(db)
    assert ei.value.code == -6                              # MPE_ERR_UNSUPPORTED
