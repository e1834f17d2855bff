"""GPU parity tests of the stage-level entry points and of the evidence gaps the round-1 review
listed: the DGL replacement in isolation (mpe_edge_softmax_aggregate), single GAT layers against
the per-layer fixtures the reference produced (mpe_gat_layer), a full-shape 23-view x 10-person
frame against the oracle, the reduced-precision mode against the ORACLE (not against the HIP fp32
path), the device-side per-frame capacity check, and the MLP error budget over every golden row
without additive slack."""
import json
import os

import numpy as np
import pytest
import torch

import golden_checks as gc
from conftest import ALL_CASES, ALL_CASES_FZ, ROOT, env, load_case, oracle, pkg

pytestmark = pytest.mark.gpu

_engines = {}


def engine_for(variant, ppc=None):
    key = (variant, ppc)
    if key not in _engines:
        e = env(variant)
        eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=4,
                                     max_persons_per_camera=ppc or (10 if variant in ('panoptic', 'arplab') else 3))
        eng.load_gat(*e.gat)
        eng.load_mlp(e.mlp)
        _engines[key] = eng
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


def _dense_features(arr, p, nf):
    N = int(arr[p + 'N'])
    feats = np.zeros((N, nf), np.float32)
    rc = arr[p + 'feat_rc']
    feats[rc[:, 0], rc[:, 1]] = arr[p + 'feat_v']
    return feats


def _close(a, b, tol):
    """|a - b| <= tol * max(1, |b|): activations reach a few units; fp32 reordering noise scales
    with the magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) <= tol


@pytest.mark.parametrize('variant,name', ALL_CASES_FZ)
def test_gat_layers_vs_reference_activations(variant, name):
    """mpe_gat_layer, layer by layer, on the reference graph's own feature rows: the hidden
    activations the REFERENCE computed (fixtures act{l}_head / act{l}_en, first four heads and
    first four edge-nodes, gat2.py:137-149) and every row of the oracle's."""
    onp = oracle()
    e = env(variant)
    eng = engine_for(variant)
    sd, prm = e.gat
    arr, frames = load_case(name, variant)
    for n, frame in enumerate(frames):
        p = 'f%d_' % n
        db = eng.to_device(eng.pack([onp.processed_input(frame)]))
        feats = _dense_features(arr, p, e.meta['num_feats'])
        H = db.n_heads
        _, inter = onp.gat_forward(sd, prm, feats, arr[p + 'src'], arr[p + 'dst'], keep=True)
        x = torch.from_numpy(feats).cuda()
        for l in range(prm['gnn_layers'] - 1):
            # (i) chained: the layer consumes the HIP path's own previous output
            x = eng.gat_layer(db, l, x, activation=0)
            got = x.cpu().numpy()
            gc.layer_activations(got, H, arr, p, l)    # the fixture holds rows [0:4] and [H:H+4] of the N x HD matrix
            assert _close(got, inter[l].numpy(), 2e-5), (l, 'all rows vs oracle')
            # (ii) isolated: the layer alone on the oracle's input rows
            if l > 0:
                alone = eng.gat_layer(db, l, inter[l - 1].cuda(), activation=0).cpu().numpy()
                assert _close(alone, inter[l].numpy(), 1e-5), (l, 'isolated layer vs oracle')
        # last layer through the same entry point: sigmoid scores in node order
        # (3e-5 here, 2e-5 on the production path: through this entry point layer 0 runs DENSE, one fp32
        #  chain over all F columns, and the fixture weights multiply the last logits by 25)
        sc = eng.gat_layer(db, prm['gnn_layers'] - 1, x, activation=1).cpu().numpy().reshape(-1)
        np.testing.assert_allclose(sc, arr[p + 'scores'], rtol=0, atol=gc.LAYER_SCORES_ATOL)
        logits = eng.gat_layer(db, prm['gnn_layers'] - 1, x, activation=2).cpu().numpy().reshape(-1)
        np.testing.assert_allclose(1.0 / (1.0 + np.exp(-logits.astype(np.float64))), arr[p + 'scores'], rtol=0, atol=3e-5)


@pytest.mark.parametrize('variant,name', [('panoptic', 'c2_5x4_clean'), ('panoptic', 'c2_5x4_messy'),
                                          ('panoptic', 'c4_5x10'), ('panoptic', 'c1_2view_1person'),
                                          ('arplab', 'arp_6x3'), ('ring23', 'ring23x3')])
def test_edge_softmax_aggregate_vs_oracle(variant, name):
    """The part the reference delegates to DGL (gat2.py:57-66,78-88) in isolation: identical ft2
    rows in, a1/a2 + apply_edges + edge_softmax(norm_by='dst') + update_all(u_mul_e, sum) out.
    The only freedom is the summation order over a destination's in-edges (<= 1 + in-degree
    terms), so the bound is a few ulp of the row magnitude."""
    onp = oracle()
    e = env(variant)
    eng = engine_for(variant)
    sd, prm = e.gat
    arr, frames = load_case(name, variant)
    p = 'f0_'
    db = eng.to_device(eng.pack([onp.processed_input(frames[0])]))
    feats = _dense_features(arr, p, e.meta['num_feats'])
    heads = list(prm['heads']) + [1]
    h = torch.from_numpy(feats)
    for l in range(prm['gnn_layers']):
        out, aux = onp.gat_layer(sd, l, h, arr[p + 'src'], arr[p + 'dst'], prm['alpha'], heads[l])
        ft2 = aux['ft2'].reshape(h.shape[0], -1)
        got = eng.edge_softmax_aggregate(db, l, ft2.cuda()).cpu().numpy()
        want = out.reshape(h.shape[0], -1).numpy()
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(got - want).max() <= 4e-6 * scale, (l, np.abs(got - want).max(), scale)
        h = torch.nn.functional.leaky_relu(out.flatten(1), prm.get('nonlinearity', 0.01))


def _first_divergence(s_gpu, s_ref, thr=0.5):
    """Both score vectors drive the same integer logic (stable sort by descending score of the
    matchings above the threshold, then sequential rules), so two runs can only differ from the
    first position where the sorted sequences differ.  Returns (gap, allowed): the oracle-score gap
    that decided that position and the largest gap the measured score deviation can explain."""
    dev = float(np.abs(s_gpu - s_ref).max())
    og = [m for m in np.argsort(-s_gpu, kind='stable') if s_gpu[m] > thr]
    orf = [m for m in np.argsort(-s_ref, kind='stable') if s_ref[m] > thr]
    for k in range(max(len(og), len(orf))):
        a = og[k] if k < len(og) else None
        b = orf[k] if k < len(orf) else None
        if a == b:
            continue
        if a is None or b is None:                 # one list ended: a score crossed the threshold
            m = b if a is None else a
            return abs(float(s_ref[m]) - thr), dev
        return abs(float(s_ref[a]) - float(s_ref[b])), 2.0 * dev
    return None, dev


def test_ring23_full_shape_frame_vs_oracle():
    """BASELINE configs[4] at its real shape in fp32: 23 views x 10 persons (230 heads, 25 300
    edge-nodes, head in-degree 221).  Covers k_attn_coef / the head aggregation at that in-degree,
    the per-camera grouped layer-0 GEMM and k_cluster_block on real scores, against the oracle
    (scores 2e-5, clusters exact, MLP input rows 3e-7)."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('ring23')
    sd, prm = e.gat
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=1, max_persons_per_camera=10)
    try:
        eng.load_gat(sd, prm)
        eng.load_mlp(e.mlp)
        frame = onp.processed_input(syn.make_frame(e.calib, 77, syn.FrameSpec(persons=10, noise_px=0.5))[0])
        db = eng.to_device(eng.pack([frame]))
        assert db.n_heads >= 200 and db.n_edge_nodes >= 19000
        scores, persons, n_persons = eng.match(db)
        eng.sync_status()
        res = onp.run_frame(frame, e.calib, sd, prm, e.mlp, mode='mlp')
        s = scores.cpu().numpy()
        np.testing.assert_allclose(s, res['scores'], rtol=0, atol=2e-5)
        sm = list(e.params.used_cameras_skeleton_matching)
        H = db.n_heads
        head_cam = [sm.index(c) for c in res['graph']['nodes_camera'][:H]]
        own = onp.cluster(s, res['graph']['pairs'], H, head_cam, len(sm))
        k = min(len(own), eng.pcap)
        assert int(n_persons[0]) == k
        got = persons[0, :k].cpu().numpy()
        assert np.array_equal(got, np.array(own, np.int32).reshape(-1, len(sm))[:k])
        if own != res['persons']:
            gap, allowed = _first_divergence(s, res['scores'])
            assert gap is not None and gap <= allowed, (gap, allowed)
        else:
            rows, valid = eng.mlp_input_rows(db, persons, n_persons)
            want = res['mlp_in'].numpy()
            assert want.shape[0] == k
            np.testing.assert_allclose(rows[0, :k].cpu().numpy(), want, rtol=0, atol=3e-7)
    finally:
        eng.close()


@pytest.mark.parametrize('variant,name', [('panoptic', 'c2_5x4_clean'), ('panoptic', 'c4_5x10'),
                                          ('ring23', 'ring23x3')])
def test_reduced_mode_vs_oracle(variant, name):
    """BASELINE configs[4] precision (bf16 MFMA GEMMs, fp16 ft2 rows) against the fp32 ORACLE
    scores (reference fixtures), with a stated bound: bf16 carries 8 significant bits, five layers
    and a logit gain of 25 in the fixture weights put the sigmoid outputs within 0.1 of fp32 (measured 0.087);
    decisions further than 0.1 from the threshold are unchanged.  Restoring fp32 restores parity."""
    onp = oracle()
    eng = engine_for(variant)
    arr, frames = load_case(name, variant)
    db = eng.to_device(eng.pack([onp.processed_input(f) for f in frames]))
    want = np.concatenate([arr['f%d_scores' % n][int(arr['f%d_N' % n]) - len(arr['f%d_edge_nodes_indices' % n]):]
                           for n in range(len(frames))])
    try:
        eng.set_precision(gat_reduced=True)
        s16 = eng.gat_scores(db).cpu().numpy()
    finally:
        eng.set_precision()
    d = np.abs(s16 - want)
    assert 1e-6 < d.max() < 0.1, d.max()
    far = np.abs(want - 0.5) > 0.1
    assert far.sum() > 0 and np.array_equal(s16[far] > 0.5, want[far] > 0.5)
    s32 = eng.gat_scores(db).cpu().numpy()
    np.testing.assert_allclose(s32, want, rtol=0, atol=2e-5)


ATTN_FP16_FLOOR = 0.9        # measured 46 of 48 (0.958)
# |score - oracle| in the attn_fp16 mode: 2.5e-3 measured with the coefficients a1/a2 taken from the fp32 values in the GEMM
# epilogue (the mode as defined); with MPE_NO_COEF_EPILOGUE=1 (switch matrix) k_attn_coef computes them from the fp16 rows: 5.2e-3
ATTN_FP16_SCORE_BOUND = 8e-3 if os.environ.get('MPE_NO_COEF_EPILOGUE') else 5e-3


@pytest.mark.parametrize('mode', ['attn_fp16', 'gat_gemm_bf16'])
def test_reduced_mode_cluster_agreement_with_oracle(tmp_path, mode):
    """Cluster agreement of the two reduced modes with the ORACLE's fp32 clusters over a 48-frame 5x4 batch, and the
    pose shift of the bf16 MLP on those frames (no parity claim).  `attn_fp16` = configs[4] as worded (fp16 ft2 rows,
    fp32 GAT GEMMs); `gat_gemm_bf16` = additionally bf16 MFMA for fc1/fc2.  Floors = the measured rates minus a margin."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('panoptic')
    sd, prm = e.gat
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=48, max_persons_per_camera=4)
    try:
        eng.load_gat(sd, prm)
        eng.load_mlp(e.mlp)
        frames = [onp.processed_input(syn.make_frame(e.calib, 4000 + i, syn.FrameSpec(persons=4, noise_px=1.0))[0])
                  for i in range(48)]
        db = eng.to_device(eng.pack(frames))
        eng.set_precision(False, False, mlp_bf16=True, gat_reduced=mode == 'gat_gemm_bf16', attn_fp16=mode == 'attn_fp16')
        scores, persons, n_persons = eng.match(db)
        poses, _ = eng.mlp3d(db, persons, n_persons)
        scores, persons, n_persons, poses = (t.cpu().numpy() for t in (scores, persons, n_persons, poses))
        sm = list(e.params.used_cameras_skeleton_matching)
        agree, dmax, pose_d = 0, 0.0, 0.0
        for f, frame in enumerate(frames):
            h0, H, e0, M = db.host.frame_counts(f)
            res = onp.run_frame(frame, e.calib, sd, prm, e.mlp, mode='mlp')
            dmax = max(dmax, float(np.abs(scores[e0:e0 + M] - res['scores']).max()))
            want = np.array(res['persons'], np.int32).reshape(-1, len(sm))
            if n_persons[f] == len(want) and np.array_equal(persons[f, :len(want)], want):
                agree += 1
                if len(want):
                    mag = max(1.0, float(np.abs(res['poses']).max()) / 4.0)
                    pose_d = max(pose_d, float(np.abs(poses[f, :len(want)] - res['poses']).max()) / mag)
        frac = agree / len(frames)
        print(mode + ': clusters equal to the oracle in %d of %d frames, max |score - oracle| %.3g, '
              'max |pose - oracle| %.3g m' % (agree, len(frames), dmax, pose_d))
        # measured on MI355X (profiles/r02_*): 0.087 and 28 of 48 frames -- with the fixture weights
        # (logit gain 25, scores spread over (0,1)) every frame holds ~80 matchings above the
        # threshold, so one swapped near-tie changes a frame; a trained model's margins are wider
        if mode == 'attn_fp16':
            assert dmax < ATTN_FP16_SCORE_BOUND, dmax
            assert frac >= ATTN_FP16_FLOOR, frac
        else:
            assert dmax < 0.1
            assert frac >= 0.5, frac
        assert pose_d < 0.5            # bf16 MLP: centimetres, not the parity path
    finally:
        eng.close()


@pytest.mark.parametrize('n_frames', [1, 3, 9])
def test_attn_fp16_small_batches_split_form_equals_fp32_mfma_form(n_frames):
    """`attn_fp16` at batch sizes BELOW the split tile kernel's switch-over (a few 5x4 frames: the wave-per-tile kernels, which
    store fp32 rows only).  Round 4 routed the fp16-row fc2 launches of GAT mode 6 there: fp32 rows written into a buffer strided
    in halves.  Mode 6 (split GEMMs) must give what mode 3 (fp32 MFMA, whose wave-per-tile kernels store fp16
    rows) gives up to the fp16 rounding of the rows, and both must sit within the mode's bound of the fp32 scores."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('panoptic')
    sd, prm = e.gat
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=n_frames, max_persons_per_camera=4)
    try:
        eng.load_gat(sd, prm)
        frames = [onp.processed_input(syn.make_frame(e.calib, 4100 + i, syn.FrameSpec(persons=4, noise_px=1.0))[0])
                  for i in range(n_frames)]
        db = eng.to_device(eng.pack(frames))
        eng.set_precision(False, False)
        s32 = eng.gat_scores(db).cpu().numpy()
        eng.set_precision(False, False, attn_fp16=True, gat_split=False)
        s_mfma = eng.gat_scores(db).cpu().numpy()
        eng.set_precision(False, False, attn_fp16=True)                 # gat_split defaults to True: mode 6
        s_split = eng.gat_scores(db).cpu().numpy()
        eng.sync_status()
        assert np.isfinite(s_split).all()
        assert np.abs(s_mfma - s32).max() < ATTN_FP16_SCORE_BOUND
        assert np.abs(s_split - s32).max() < ATTN_FP16_SCORE_BOUND, np.abs(s_split - s32).max()
        assert np.abs(s_split - s_mfma).max() < ATTN_FP16_SCORE_BOUND
    finally:
        eng.close()


def test_cfg4_as_worded_full_shape_vs_oracle():
    """BASELINE configs[4] as it is worded -- "23-view x 10-person stress; fp16 GATv2 attention + bf16 MLP MFMA GEMM" -- at
    its FULL shape: fp16 ft2 rows in the attention stage only (the GAT GEMMs stay on the fp32 MFMA, the attention
    coefficients come from the fp32 values in the GEMM epilogue), bf16 MFMA for the MLP.  Against the fp32 ORACLE on
    whole 23 x 10 frames: score bound, cluster agreement (a differing frame has to be explained by the score gap at
    the first diverging decision of the greedy pass), pose shift.  Numbers go to gpurun_out/cfg4_full_shape.json
    (profiles/r03_cfg4_full_shape.json).  Measured: |score - oracle| 2.5e-3 (fp16 keeps 11 significant bits of the
    rows, the GEMMs lose nothing; 0.087 when the GAT GEMMs are bf16 as well); at this shape a frame holds 25 300
    candidate matchings, ~20 000 of them above the threshold with the fixture weights, so a 2.5e-3 perturbation
    reorders near-ties in most frames: clusters identical in 1 of 4 frames, the other 3 explained by the gap at
    the first diverging decision (no unexplained frame is tolerated).  At 5 x 4 the same mode agrees in 45+ of 48
    frames (test_reduced_mode_cluster_agreement_with_oracle)."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('ring23')
    sd, prm = e.gat
    n = 4
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=n, max_persons_per_camera=10)
    try:
        eng.load_gat(sd, prm)
        eng.load_mlp(e.mlp)
        frames = [onp.processed_input(syn.make_frame(e.calib, 300 + i, syn.FrameSpec(persons=10, noise_px=0.5))[0]) for i in range(n)]
        db = eng.to_device(eng.pack(frames))
        assert db.n_heads >= 200 * n and db.n_edge_nodes >= 19000 * n
        eng.set_precision(False, False, mlp_bf16=True, attn_fp16=True)
        scores, persons, n_persons = eng.match(db)
        poses, _ = eng.mlp3d(db, persons, n_persons)
        eng.sync_status()
        scores, persons, n_persons, poses = (t.cpu().numpy() for t in (scores, persons, n_persons, poses))
        sm = list(e.params.used_cameras_skeleton_matching)
        equal, explained, dmax, pose_rel = 0, 0, 0.0, 0.0
        for f, frame in enumerate(frames):
            h0, H, e0, M = db.host.frame_counts(f)
            res = onp.run_frame(frame, e.calib, sd, prm, e.mlp, mode='mlp')
            s = scores[e0:e0 + M]
            dmax = max(dmax, float(np.abs(s - res['scores']).max()))
            want = np.array(res['persons'], np.int32).reshape(-1, len(sm))
            k = min(len(want), eng.pcap)
            if n_persons[f] == k and np.array_equal(persons[f, :k], want[:k]):
                equal += 1
                if k and len(want) <= eng.pcap:
                    mag = max(1.0, float(np.abs(res['poses']).max()))
                    pose_rel = max(pose_rel, float(np.abs(poses[f, :k] - res['poses'][:k]).max()) / mag)
            else:
                gap, allowed = _first_divergence(s, res['scores'])
                assert gap is not None and gap <= allowed, (f, gap, allowed)
                explained += 1
        rec = {'frames': n, 'shape': '23 views x 10 persons', 'max_abs_score_diff': dmax, 'clusters_equal': equal,
               'clusters_explained_by_first_divergence': explained, 'max_pose_shift_relative_to_largest_output': pose_rel,
               'mode': 'attn_fp16 (fp16 ft2 rows, fp32 GAT GEMMs) + bf16 MLP'}
        out = os.path.join(ROOT, 'gpurun_out')
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'cfg4_full_shape.json'), 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec))
        assert dmax < ATTN_FP16_SCORE_BOUND, rec
        # measured 1 equal + 3 explained (0 + 4 under MPE_NO_COEF_EPILOGUE / MPE_L0_GROUPED=0, tools/run_switch_matrix.sh): how
        # many near-ties a 2.5e-3 perturbation reorders among 20 000 matchings is not a property to pin; that every differing
        # frame is explained by the gap at its first diverging decision is (asserted in the loop above)
        assert equal + explained == n, rec
        assert pose_rel < 0.05, rec                     # bf16 MLP: per cent of the output scale, not the parity path
    finally:
        eng.close()


@pytest.mark.parametrize('general_path', [False, True])
def test_frame_beyond_capacity_is_flagged_on_device(general_path, monkeypatch):
    """mpe.h per-frame capacity contract: a frame with more skeletons than max_heads_per_frame
    that slips past the host (here: the packed batch is uploaded without Engine.check_capacity)
    is detected by k_topology, yields zero scores and no persons, leaves its neighbours intact,
    and mpe_sync_status returns MPE_ERR_CAPACITY exactly once -- on the fused attention kernel and on
    the general kernels (what larger frames run on)."""
    if general_path:
        monkeypatch.setenv('MPE_NO_FUSED_ATTENTION', '1')
    else:
        monkeypatch.delenv('MPE_NO_FUSED_ATTENTION', raising=False)
    onp = oracle()
    syn = pkg('synthetic')
    L = pkg('lib')
    e = env('panoptic')
    sd, prm = e.gat
    big = pkg('pipeline').Engine(e.params, e.calib, max_frames=3, max_persons_per_camera=4)
    small = pkg('pipeline').Engine(e.params, e.calib, max_frames=4, max_heads_per_frame=14)
    try:
        for eng in (big, small):
            eng.load_gat(sd, prm)
        ok = onp.processed_input(syn.make_frame(e.calib, 31, syn.FrameSpec(persons=2))[0])       # 10 heads
        over = onp.processed_input(syn.make_frame(e.calib, 32, syn.FrameSpec(persons=4))[0])     # 20 heads > 14
        pb = big.pack([ok, over, ok])
        want_s, want_p, want_n = big.match(big.to_device(pb))
        big.sync_status()
        with pytest.raises(ValueError):
            small.to_device(pb)                                     # the Python engine refuses on the host
        db = pb.to(small.device)                                    # the C ABI alone: device-side detection
        assert pb.n_heads <= small.max_frames * small.hpf
        s, p, n = small.match(db)
        with pytest.raises(L.MpeError) as ei:
            small.sync_status()
        assert ei.value.code == -2
        small.sync_status()                                         # sticky bit was cleared
        s, n, p = s.cpu().numpy(), n.cpu().numpy(), p.cpu().numpy()
        e_off = pb.frame_en_off
        assert n[1] == 0 and not s[e_off[1]:e_off[2]].any()
        ws, wn, wp = want_s.cpu().numpy(), want_n.cpu().numpy(), want_p.cpu().numpy()
        for f in (0, 2):
            assert np.array_equal(s[e_off[f]:e_off[f + 1]], ws[e_off[f]:e_off[f + 1]])
            assert n[f] == wn[f] and np.array_equal(p[f, :n[f], :], wp[f, :n[f], :])
    finally:
        big.close()
        small.close()


def _exact_mlp(x, weights):
    keys = sorted({int(k.split('.')[1]) for k in weights})
    h = x.double()
    for n, k in enumerate(keys):
        W = torch.from_numpy(weights['layers.%d.weight' % k]).double()
        b = torch.from_numpy(weights['layers.%d.bias' % k]).double()
        h = h @ W.T + b
        if n != len(keys) - 1:
            h = torch.nn.functional.leaky_relu(h, 0.1)
        h = h.float().double()
    return h


def test_mlp_error_budget_every_golden_row():
    """3D tolerance, pinned without slack (north star: 1e-3 mm vs the reference).  For EVERY MLP
    input row the reference produced (all fixture variants): with `exact` = the network evaluated
    in f64 with fp32 rounding between layers,
        |gpu - exact| <= |ref - exact|            (the HIP path is at least as accurate as torch-CPU)
        |gpu - ref|   <= |gpu - exact| + |ref - exact|   (triangle inequality, no additive constant)
    per variant, on the maxima over its rows; the measured figures are written to
    gpurun_out/mlp_error_budget.json (millimetres after the x10 decode)."""
    report = {}
    for variant in ('panoptic', 'arplab', 'arprobot', 'ring23'):
        e = env(variant)
        eng = engine_for(variant)
        xs, refs = [], []
        for v, name in ALL_CASES:
            if v != variant:
                continue
            arr, frames = load_case(name, variant)
            for n in range(len(frames)):
                if 'f%d_mlp_in' % n in arr:
                    xs.append(arr['f%d_mlp_in' % n])
                    refs.append(arr['f%d_mlp_out' % n])
        x = torch.from_numpy(np.concatenate(xs))
        ref = torch.from_numpy(np.concatenate(refs)).double()
        exact = _exact_mlp(x, e.mlp)
        gpu = eng.mlp_forward(x.cuda()).cpu().double()
        e_ref = (ref - exact).abs().max().item()
        e_gpu = (gpu - exact).abs().max().item()
        d = (gpu - ref).abs().max().item()
        # metres = MLP units x 10 (metrics_from_model.py:281); mm = x 1e4
        report[variant] = {'rows': int(x.shape[0]), 'gpu_vs_exact_mm': e_gpu * 1e4, 'ref_vs_exact_mm': e_ref * 1e4,
                           'gpu_vs_ref_mm': d * 1e4, 'output_scale': float(ref.abs().max())}
        assert e_gpu <= e_ref, (variant, e_gpu, e_ref)
        assert d <= e_gpu + e_ref, (variant, d, e_gpu, e_ref)
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mlp_error_budget.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))


def test_mlp_capture_volume_regime_every_golden_row():
    """The 1e-3 mm item of the north star, made decidable in the regime it is about: MLP outputs inside
    the capture volume (|pose| <= 5 m).  Fixtures `mlp_out_room` / `poses_room` = the REFERENCE's MLP
    (utils/mlp.py:8-28, torch-CPU) with the capture-volume weights (`Env.mlp_room`: a decoder of the row's
    triangulated points with dense hash noise, 5 %% of the He scale, on every weight) on the reference's own
    input rows.  Rows whose persons are mixed-up skeletons triangulate far outside the room and are left
    to test_mlp_error_budget_every_golden_row.  Per variant, on the rows in the room:

        max_abs_mm        |gpu - ref| after the x10 decode (metrics_from_model.py:278-294)
        max_abs_ulp       the same in fp32 ulps of the compared output element
        ref_vs_exact_mm   the reference's own distance from the network evaluated in f64 (fp32 between layers)
        gpu_vs_exact_mm   ours

    Asserted: |gpu - exact| <= |ref - exact| and |gpu - ref| <= the sum (no additive slack); where the
    reference's own noise floor allows it (ref_vs_exact <= 5e-4 mm) |gpu - ref| <= 1e-3 mm as the north star
    words it, otherwise the item is recorded as UNMET with the floor next to it and the HIP side is held to
    gpu_vs_exact <= 4e-3 mm and <= 14 ulp of the row's largest output (regression guards around the measured
    1.9-3.6e-3 mm / 6.5-12 ulp; the reference sits at 3.6-5.4e-3 mm / 14-18 ulp).  Neither side can be within
    1.5 ulp of the exact network: a layer is a sum of 32-deep fp32 fma chains (ours, f64 across the chains) or
    of blocked fp32 sums (torch-CPU), and eight layers of that are worth a few ulp each.
    Written to gpurun_out/mlp_capture_volume.json (profiles/r03_mlp_capture_volume.json)."""
    report = {}
    for variant in ('panoptic', 'arplab', 'arprobot', 'ring23'):
        e = env(variant)
        eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=16, max_persons_per_camera=10)      # row capacity 16 x pcap
        try:
            eng.load_mlp(e.mlp_room)
            xs, refs = [], []
            for v, name in ALL_CASES:
                if v != variant:
                    continue
                arr, frames = load_case(name, variant)
                for n in range(len(frames)):
                    if 'f%d_mlp_in' % n in arr:
                        xs.append(arr['f%d_mlp_in' % n])
                        refs.append(arr['f%d_mlp_out_room' % n])
            x = torch.from_numpy(np.concatenate(xs))
            ref = np.concatenate(refs).astype(np.float64)
            room = np.abs(ref).max(axis=1) <= 0.5                     # MLP units = metres / 10
            assert room.sum() >= max(1, len(room) // 2), (variant, int(room.sum()), len(room))
            exact = _exact_mlp(x, e.mlp_room).numpy()
            gpu = eng.mlp_forward(x.cuda()).cpu().numpy().astype(np.float64)
        finally:
            eng.close()
        ref, exact, gpu = ref[room], exact[room], gpu[room]
        row_ulp = np.spacing(np.abs(ref).max(axis=1, keepdims=True).astype(np.float32)).astype(np.float64)
        e_ref, e_gpu, d = np.abs(ref - exact), np.abs(gpu - exact), np.abs(gpu - ref)
        rec = {'rows_in_room': int(room.sum()), 'rows': int(len(room)), 'largest_pose_m': float(np.abs(ref).max() * 10),
               'max_abs_mm': float(d.max() * 1e4), 'max_abs_row_ulp': float((d / row_ulp).max()),
               'ref_vs_exact_mm': float(e_ref.max() * 1e4), 'gpu_vs_exact_mm': float(e_gpu.max() * 1e4),
               'ref_vs_exact_row_ulp': float((e_ref / row_ulp).max()), 'gpu_vs_exact_row_ulp': float((e_gpu / row_ulp).max())}
        rec['north_star_1e-3_mm'] = 'met' if rec['max_abs_mm'] <= 1e-3 else 'unmet: reference noise floor %.2e mm' % rec['ref_vs_exact_mm']
        report[variant] = rec
        assert e_gpu.max() <= e_ref.max(), (variant, rec)
        assert d.max() <= e_gpu.max() + e_ref.max(), (variant, rec)
        if rec['ref_vs_exact_mm'] <= 5e-4:
            assert rec['max_abs_mm'] <= 1e-3, (variant, rec)
        else:
            assert rec['gpu_vs_exact_mm'] <= 4e-3 and rec['gpu_vs_exact_row_ulp'] <= 14.0, (variant, rec)
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mlp_capture_volume.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))


def test_mlp_within_1e_3_mm_of_the_exact_network():
    """The reachable form of the north star's 3D tolerance.  "Within 1e-3 mm of the reference" cannot hold: the
    reference's own torch-CPU MLP sits 1.6-6e-3 mm from its exactly evaluated network (f64 sums, fp32 rounding between layers,
    test above).  What the path can claim, and what is asserted here on every capture-volume golden row of the four rigs, is
    |gpu - exact| * 10 <= 1e-6 m in the MLP's REFERENCE-EXACT mode (mpe_set_precision MLP 5 = Engine.set_precision(mlp_f64=True):
    exact fp32 x fp32 products accumulated in f64 over the whole K on the f64 matrix pipe, csrc/gemm_f64.hip) -- there the path
    IS the exact network up to the f64 summation order.  Beside it the record holds the default mode and the MAXIMUM-ACCURACY
    mode of the fast form (MLP 4: the split-bf16 form with an f64 flush after every K stage, rms error of a launch 0.13-0.18 ulp
    against 0.24-0.26): it is asserted to be at least as close as the default on every rig and closer than the reference, and
    reported against the 1e-3 mm line (measured: met on three rigs, 1.19e-3 mm on the fourth; mode 5: 0 on all four) with the layer whose own
    deviation is largest.  gpurun_out/mlp_max_accuracy.json -> profiles/r05_mlp_max_accuracy.json."""
    report = {}
    for variant in ('panoptic', 'arplab', 'arprobot', 'ring23'):
        e = env(variant)
        eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=16, max_persons_per_camera=10)
        try:
            eng.load_mlp(e.mlp_room)
            xs, refs = [], []
            for v, name in ALL_CASES:
                if v != variant:
                    continue
                arr, frames = load_case(name, variant)
                for n in range(len(frames)):
                    if 'f%d_mlp_in' % n in arr:
                        xs.append(arr['f%d_mlp_in' % n])
                        refs.append(arr['f%d_mlp_out_room' % n])
            x = torch.from_numpy(np.concatenate(xs))
            ref = np.concatenate(refs).astype(np.float64)
            room = np.abs(ref).max(axis=1) <= 0.5                     # MLP units = metres / 10
            exact = _exact_mlp(x, e.mlp_room).numpy()
            y_def = eng.mlp_forward(x.cuda()).cpu().numpy().astype(np.float64)
            eng.set_precision(False, True, mlp_max_accuracy=True)
            y_max = eng.mlp_forward(x.cuda()).cpu().numpy().astype(np.float64)
            y_one = eng.mlp_forward(x[:1].cuda()).cpu().numpy().astype(np.float64)
            # per layer: the mode's own layer on the EXACT network's input of that layer (which layer's rounding is the largest?)
            keys = sorted({int(k.split('.')[1]) for k in e.mlp_room})
            h = x.double()
            worst = (0.0, -1)
            for li, k in enumerate(keys):
                w = torch.as_tensor(np.asarray(e.mlp_room['layers.%d.weight' % k])).double()
                b = torch.as_tensor(np.asarray(e.mlp_room['layers.%d.bias' % k])).double()
                last = li == len(keys) - 1
                y = h @ w.T + b
                if not last:
                    y = torch.where(y > 0, y, 0.1 * y)
                got = eng.linear(h.float().cuda(), w.float().numpy(), b.float().numpy(), None if last else 0.1, split=True,
                                 split_flush_per_stage=True).cpu().double()
                y32 = y.float().double()
                ulp = float(np.spacing(np.float32(y32.abs().max().item())))
                dev = ((got - y32).abs().max().item()) / ulp
                if dev > worst[0]:
                    worst = (dev, li)
                h = y32                                             # the exact network rounds to fp32 between layers
            eng.set_precision(False, True, mlp_f64=True)
            y_f64 = eng.mlp_forward(x.cuda()).cpu().numpy().astype(np.float64)
            y_f64_one = eng.mlp_forward(x[:1].cuda()).cpu().numpy().astype(np.float64)
            eng.set_precision(False, True)
            assert np.array_equal(eng.mlp_forward(x.cuda()).cpu().numpy().astype(np.float64), y_def)      # the default's bits are back
        finally:
            eng.close()
        assert np.array_equal(y_one[0], y_max[0]) and np.array_equal(y_f64_one[0], y_f64[0])       # same bits alone and in the batch
        ref, exact, y_def, y_max, y_f64 = ref[room], exact[room], y_def[room], y_max[room], y_f64[room]
        rec = {'rows_in_room': int(room.sum()), 'largest_pose_m': float(np.abs(ref).max() * 10),
               'ref_vs_exact_mm': float(np.abs(ref - exact).max() * 1e4),
               'default_vs_exact_mm': float(np.abs(y_def - exact).max() * 1e4),
               'max_accuracy_vs_exact_mm': float(np.abs(y_max - exact).max() * 1e4),
               'max_accuracy_vs_ref_mm': float(np.abs(y_max - ref).max() * 1e4),
               'max_accuracy_within_1e-3_mm_of_exact': bool(np.abs(y_max - exact).max() * 1e4 <= 1e-3),
               'largest_single_layer_deviation_ulp': worst[0], 'in_layer': worst[1],
               'f64_mode_vs_exact_mm': float(np.abs(y_f64 - exact).max() * 1e4),
               'f64_mode_outputs_equal_to_exact': float((y_f64 == exact).mean()),
               'f64_mode_vs_ref_mm': float(np.abs(y_f64 - ref).max() * 1e4)}
        report[variant] = rec
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'mlp_max_accuracy.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))
    for variant, rec in report.items():
        assert rec['f64_mode_vs_exact_mm'] <= 1e-3, (variant, rec)                       # the north star's number, against the exact network
        # ... and in fact (nearly) every output bit for bit: only the f64 summation order can move one
        assert rec['f64_mode_outputs_equal_to_exact'] >= 0.999, (variant, rec)
        assert rec['max_accuracy_vs_exact_mm'] <= rec['default_vs_exact_mm'] <= rec['ref_vs_exact_mm'], (variant, rec)
        assert rec['max_accuracy_vs_exact_mm'] <= 1.25e-3, (variant, rec)                # regression guard around the measured 0.8-1.2e-3 mm


def test_attention_paths_give_identical_bits(monkeypatch):
    """The attention stage has two kernels (k_gat_fused for frames whose slice fits in LDS, the
    general k_aggregate_en / k_aggregate_heads pair otherwise) and two sources of the coefficients
    a1/a2 (fc2 GEMM epilogue, or k_attn_coef / the fused kernel itself).  All of them use the same
    summation orders, so every combination must give bit-identical scores and hidden rows."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('panoptic')
    sd, prm = e.gat
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=96, max_persons_per_camera=5)
    try:
        eng.load_gat(sd, prm)
        specs = [syn.FrameSpec(persons=4), syn.FrameSpec(persons=5, joint_drop=0.2), syn.FrameSpec(persons=2, empty_cameras=('trackerb',)),
                 syn.FrameSpec(persons=3, cameras=['trackerd', 'trackera', 'trackere'])]
        frames = [onp.processed_input(syn.make_frame(e.calib, 6000 + i, specs[i % 4])[0]) for i in range(96)]
        db = eng.to_device(eng.pack(frames))
        res = {}

        def switch(name, on):
            if on:
                monkeypatch.setenv(name, '1')
            else:
                monkeypatch.delenv(name, raising=False)

        # ... and two sources of the heads' in-edge lists (the per-batch table of k_head_sources, or the
        # arithmetic inside the kernels that frames too large for the table fall back to), and the fused
        # kernel stages its image with or without the overlapped softmax phase
        for fused in (True, False):
            for epi in (True, False):
                for table in (True, False):
                    for overlap in ((True, False) if fused else (True,)):
                        switch('MPE_NO_FUSED_ATTENTION', not fused)
                        switch('MPE_NO_COEF_EPILOGUE', not epi)
                        switch('MPE_NO_HEAD_SRC_TABLE', not table)
                        switch('MPE_FUSED_NO_OVERLAP', not overlap)
                        sc, sh = eng.gat_scores(db, heads=True)
                        res[(fused, epi, table, overlap)] = (sc.cpu().numpy(), sh.cpu().numpy())
        ref = res[(True, True, True, True)]
        for key, (sc, sh) in res.items():
            assert np.array_equal(sc, ref[0]) and np.array_equal(sh, ref[1]), key
    finally:
        eng.close()


def test_native_packer_into_pinned_arena_feeds_the_device_path():
    """f1: frame JSON -> mpe_pack_json_into (page-locked capacity arena) -> ONE H2D copy -> match:
    persons equal the reference's (golden fixtures), and Engine.stream_json (parse of chunk i+1
    overlapped with the device work of chunk i) gives bit-identical poses to the Python-packed path."""
    onp = oracle()
    packing = pkg('packing')
    e = env('panoptic')
    eng = engine_for('panoptic')
    names = ['c2_5x4_clean', 'c2_5x4_messy', 'c2_5x4_reordered', 'c2_3x2', 'c4_5x10', 'c1_2view_1person']
    frames, want = [], []
    for name in names:
        arr, fr = load_case(name)
        for n, f in enumerate(fr):
            frames.append(onp.processed_input(f))
            want.append(arr['f%d_persons' % n])
    text = json.dumps(frames).encode()
    pinned = packing.CapacityArena(eng.V, eng.J, 4, 4 * eng.hpf, 'pinned')
    dev = packing.CapacityArena(eng.V, eng.J, 4, 4 * eng.hpf, eng.device)
    got = []
    for start in range(0, len(frames), 4):
        pb = packing.pack_json_into(text, e.params, pinned, frame_start=start, max_frames=4)
        eng.check_capacity(pb)
        db = packing.DeviceBatch(pb, eng.device, arena=dev)
        dev.buf.copy_(pinned.buf, non_blocking=True)
        _, persons, n_persons = eng.match(db)
        persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
        got += [persons[f, :n_persons[f]] for f in range(pb.n_frames)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # streaming form against the batch form
    ref_poses, ref_n = [], []
    for start in range(0, len(frames), 4):
        db = eng.to_device(eng.pack(frames[start:start + 4]))
        _, persons, n_persons = eng.match(db)
        ref_poses.append(eng.mlp3d(db, persons, n_persons)[0].cpu().numpy())
        ref_n.append(n_persons.cpu().numpy())
    chunks = list((poses.copy(), n.copy()) for _, poses, n in eng.stream_json(text, chunk_frames=4, mode='mlp'))
    assert len(chunks) == len(ref_poses)
    for (poses, n), rp, rn in zip(chunks, ref_poses, ref_n):
        assert np.array_equal(n, rn)
        for f in range(len(n)):
            assert np.array_equal(poses[f, :n[f]], rp[f, :n[f]])


def test_weights_can_be_set_twice_before_the_first_batch():
    """mpe_set_gat_layer / mpe_set_mlp_layer called again for the same layer replace the first
    upload (the old device copies are freed), and the workspace flags make a context whose
    weights are complete only later usable: MPE_ERR_STATE first, normal results afterwards."""
    onp = oracle()
    L = pkg('lib')
    e = env('panoptic')
    sd, prm = e.gat
    arr, frames = load_case('c2_5x4_clean')
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=2, max_persons_per_camera=4)
    try:
        db = eng.to_device(eng.pack([onp.processed_input(frames[0])]))
        with pytest.raises(L.MpeError) as ei:
            eng.gat_scores(db)                           # no weights yet
        assert ei.value.code == -3
        wrong = {k: (v * 0.5).astype(np.float32) for k, v in sd.items()}
        eng.load_gat(wrong, prm)
        eng.load_gat(sd, prm)                            # second upload wins
        eng.load_mlp({k: v * 2 for k, v in e.mlp.items()})
        eng.load_mlp(e.mlp)
        sc = eng.gat_scores(db).cpu().numpy()
        H = db.n_heads
        np.testing.assert_allclose(sc, arr['f0_scores'][H:], rtol=0, atol=2e-5)
        y = eng.mlp_forward(torch.from_numpy(arr['f0_mlp_in']).cuda()).cpu().numpy()
        np.testing.assert_allclose(y, arr['f0_mlp_out'], rtol=0, atol=2e-6)
        with pytest.raises(L.MpeError):
            eng.load_gat(sd, prm)                        # frozen after the first batch
    finally:
        eng.close()


def test_empty_batch_and_graphless_batch():
    """Degenerate batches through every batch entry point: zero frames, and frames without any
    cross-camera pair (no graph: the reference skips them, metrics_from_model.py:195-196)."""
    onp = oracle()
    e = env('panoptic')
    eng = engine_for('panoptic')
    _, frames = load_case('c2_5x4_clean')
    one_cam = {'trackerb': onp.processed_input(frames[0])['trackerb']}
    for batch in ([], [{}], [one_cam, {}, one_cam]):
        db = eng.to_device(eng.pack(batch))
        scores, persons, n_persons = eng.match(db)
        poses, valid = eng.mlp3d(db, persons, n_persons)
        tri, jv = eng.triangulate(db, persons, n_persons)
        eng.sync_status()
        assert scores.numel() == 0 and n_persons.shape[0] == len(batch)
        assert int(n_persons.sum()) == 0 and not bool(valid.any()) and not bool(jv.any())
    text = json.dumps([one_cam, {}])
    chunks = list(eng.stream_json(text, chunk_frames=4))
    assert len(chunks) == 1 and chunks[0][2].tolist() == [0, 0]
    assert list(eng.stream_json('[]', chunk_frames=4)) == []


def test_score_noise_against_the_f64_network():
    """Where the 2e-5 score bound comes from: for every fixture frame, `exact` = the same network
    evaluated in float64 (oracle, no fp32 rounding anywhere).  The reference's own fp32 scores sit
    e_ref from it (torch-CPU summation order, amplified by the fixture weights' logit gain of 25);
    the HIP path sits e_gpu from it.  Required: the HIP path is not a noisier fp32 evaluation than
    the reference by more than a factor (its GEMMs are single fp32 chains over K <= 512 where MKL
    blocks; longer sums, i.e. layer 0, carry f64 running sums by default), and with f64 running sums (`mpe_set_precision(ctx, 1, .)`) it is at least as close
    to the f64 network as the reference.  The figures go to gpurun_out/score_noise.json."""
    onp = oracle()
    report = {}
    worst_ratio, worst_ratio64, ratios64 = 0.0, 0.0, []
    for variant, name in ALL_CASES:
        e = env(variant)
        eng = engine_for(variant)
        sd, prm = e.gat
        arr, frames = load_case(name, variant)
        for n, frame in enumerate(frames):
            p = 'f%d_' % n
            feats = _dense_features(arr, p, e.meta['num_feats'])
            exact = onp.gat_forward(sd, prm, feats, arr[p + 'src'], arr[p + 'dst'], dtype=torch.float64).numpy()
            db = eng.to_device(eng.pack([onp.processed_input(frame)]))
            H = db.n_heads
            sc, sh = eng.gat_scores(db, heads=True)
            gpu = np.concatenate([sh.cpu().numpy(), sc.cpu().numpy()])
            try:
                eng.set_precision(gat_acc64=True)
                sc64, sh64 = eng.gat_scores(db, heads=True)
            finally:
                eng.set_precision()
            gpu64 = np.concatenate([sh64.cpu().numpy(), sc64.cpu().numpy()])
            e_ref = float(np.abs(arr[p + 'scores'] - exact).max())
            e_gpu = float(np.abs(gpu - exact).max())
            e_gpu64 = float(np.abs(gpu64 - exact).max())
            report['%s/%s/%d' % (variant, name, n)] = {'e_ref': e_ref, 'e_gpu_fp32_chain': e_gpu, 'e_gpu_f64_sums': e_gpu64}
            # small graphs (2 cameras): both sides sit a handful of fp32 roundings of a score in [0, 1] from the f64
            # network and which of them is closer is a coin toss -- measured on arprobot/arp_robot_only frame 1: reference
            # 1.01e-6, f64-sum mode 1.59e-6.  Below a tenth of the 2e-5 score bound the comparison is not made per frame
            floor = max(e_ref, 2e-6)
            worst_ratio = max(worst_ratio, e_gpu / floor)
            worst_ratio64 = max(worst_ratio64, e_gpu64 / floor)
            ratios64.append(e_gpu64 / max(e_ref, 1e-12))
    out = os.path.join(ROOT, 'gpurun_out')
    os.makedirs(out, exist_ok=True)
    report['worst_ratio_fp32_chain'] = worst_ratio
    report['worst_ratio_f64_sums'] = worst_ratio64
    report['median_ratio_f64_sums'] = float(np.median(ratios64))
    with open(os.path.join(out, 'score_noise.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: v for k, v in report.items() if k.startswith(('worst', 'median'))}))
    # default path; with MPE_L0_GROUPED=0 (switch matrix) layer 0 is one dense fp32 chain over K = 902: measured 2.504
    assert worst_ratio <= (3.0 if os.environ.get('MPE_L0_GROUPED') == '0' else 2.5), worst_ratio
    # over all fixture frames the f64-sum mode sits at about half the reference's distance (measured median 0.56)
    assert report['median_ratio_f64_sums'] <= (1.0 if os.environ.get('MPE_L0_GROUPED') == '0' else 0.75), report['median_ratio_f64_sums']
    # the switch matrix (tools/run_switch_matrix.sh) also runs this suite with MPE_L0_GROUPED=0: the dense K = 902 / 1082
    # layer-0 fc1 then sums in another order than the per-camera K = 180 form and the f64-sum mode sits up to 1.3x the
    # reference's own distance from the f64 network (measured 1.30) instead of below it -- every parity bound still holds
    assert worst_ratio64 <= (1.5 if os.environ.get('MPE_L0_GROUPED') == '0' else 1.0), worst_ratio64


def test_run_pipelined_gives_the_same_bits_as_sequential_calls():
    """Engine.run_pipelined: matching of batch i+1 overlaps the 3D stage of batch i on two streams
    (disjoint workspaces); every batch must come out with the bits of the plain call sequence."""
    onp = oracle()
    syn = pkg('synthetic')
    e = env('panoptic')
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=12, max_persons_per_camera=5)
    eng.load_gat(*e.gat)
    eng.load_mlp(e.mlp)
    specs = [syn.FrameSpec(persons=4), syn.FrameSpec(persons=2, joint_drop=0.2), syn.FrameSpec(persons=3, empty_cameras=('trackerc',))]
    batches = []
    for b in range(5):
        frames = [onp.processed_input(syn.make_frame(e.calib, 7000 + 40 * b + i, specs[(b + i) % 3])[0]) for i in range(3 + 2 * b)]
        batches.append(eng.to_device(eng.pack(frames)))
    want = []
    for db in batches:
        _, persons, n_persons = eng.match(db, want_scores=False)
        want.append((eng.mlp3d(db, persons, n_persons)[0].cpu().numpy(), n_persons.cpu().numpy(), persons.cpu().numpy()))
    got = [(p.cpu().numpy(), n.cpu().numpy(), q.cpu().numpy()) for p, n, q, _ in eng.run_pipelined(batches)]
    assert len(got) == len(want)
    for (p1, n1, q1), (p2, n2, q2) in zip(want, got):
        assert np.array_equal(n1, n2) and np.array_equal(q1, q2)
        for f in range(len(n1)):
            assert np.array_equal(p1[f, :n1[f]], p2[f, :n1[f]])
    tri_want = [eng.triangulate(db, torch.from_numpy(w[2]).to(eng.device), torch.from_numpy(w[1]).to(eng.device))[0].cpu().numpy()
                for db, w in zip(batches, want)]
    tri_got = [p.cpu().numpy() for p, n, q, _ in eng.run_pipelined(batches, mode='tri')]
    for a, b, w in zip(tri_want, tri_got, want):
        for f in range(len(w[1])):
            assert np.array_equal(a[f, :w[1][f]], b[f, :w[1][f]], equal_nan=True)

    # an iterator that uploads LAZILY (DeviceBatch.upload from pinned memory on the current stream, inside
    # next()): each batch's copy must be ordered before its matching stage on the side stream
    packing = pkg('packing')
    pbs = [db.host for db in batches]

    def lazy():
        for pb in pbs:
            pinned = packing.BatchArena(pb, 'pinned').fill(pb)
            arena = packing.BatchArena(pb, eng.device)
            db = packing.DeviceBatch(pb, eng.device, arena=arena)
            arena.buf.zero_()                       # stale contents if the copy were not waited for
            db.upload(pinned)
            yield db
    got2 = [(p.cpu().numpy(), n.cpu().numpy(), q.cpu().numpy()) for p, n, q, _ in eng.run_pipelined(lazy())]
    for (p1, n1, q1), (p2, n2, q2) in zip(want, got2):
        assert np.array_equal(n1, n2) and np.array_equal(q1, q2)
        for f in range(len(n1)):
            assert np.array_equal(p1[f, :n1[f]], p2[f, :n1[f]])
    # several contexts taking turns on the batches (Engine.sibling: own workspace, same weights): same bits again,
    # with the lazily uploading iterator too; a precision mode set afterwards reaches the siblings
    for K in (2, 3):
        for src in (batches, lazy()):
            gotk = [(p.cpu().numpy(), n.cpu().numpy(), q.cpu().numpy()) for p, n, q, _ in eng.run_pipelined(src, contexts=K)]
            assert len(gotk) == len(want)
            for (p1, n1, q1), (p2, n2, q2) in zip(want, gotk):
                assert np.array_equal(n1, n2) and np.array_equal(q1, q2)
                for f in range(len(n1)):
                    assert np.array_equal(p1[f, :n1[f]], p2[f, :n1[f]])
    assert len(eng._siblings) == 2
    eng.set_precision(False, False)
    try:
        plain = []
        for db in batches:
            _, persons, n_persons = eng.match(db, want_scores=False)
            plain.append(eng.mlp3d(db, persons, n_persons)[0].cpu().numpy())
        for w, (p, n, q, _) in zip(plain, eng.run_pipelined(batches, contexts=2)):
            assert np.array_equal(w, p.cpu().numpy())
    finally:
        eng.set_precision()
    # closing the generator early must leave nothing running on the side streams
    for K in (1, 2):
        gen = eng.run_pipelined(batches, contexts=K)
        first = next(gen)
        gen.close()
        torch.cuda.synchronize()
        assert np.array_equal(first[1].cpu().numpy(), want[0][1])
    eng.close()
    assert eng._siblings == []


def test_gemm_launch_census_is_the_parents():
    """Which GEMM launches every precision mode makes (tools/gemm_census.py: 7 GAT and 6 MLP settings x MPE_LATENCY_PATH unset / 0 x
    MPE_NO_COEF_EPILOGUE unset / set x batches of 1, 17 and 40 frames, one match + mlp3d each): the launch counts and the FLOP
    figures of the fp32 MFMA, split-bf16 and plain bf16 forms must equal, exactly, what the commit before the dispatch became one
    function (csrc/api.hip: gemm(), csrc/gemm_form.h) gave -- tests/golden/harness/gemm_census.json is that tool's output there.
    The counts are integers and the FLOP figures sums of integers below 2^53; the millisecond fields are not compared."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('gemm_census', os.path.join(ROOT, 'tools', 'gemm_census.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, 'tests', 'golden', 'harness', 'gemm_census.json')) as fh:
        want = json.load(fh)
    e = env('panoptic')
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=64, max_persons_per_camera=10)
    saved = {k: os.environ.get(k) for k in ('MPE_LATENCY_PATH', 'MPE_NO_COEF_EPILOGUE')}
    try:
        eng.load_gat(*e.gat)
        eng.load_mlp(e.mlp)
        got = tool.census(eng, e.calib)
    finally:
        eng.set_precision()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        eng.close()
    assert sorted(got) == sorted(want) and len(want) == 13 * 4 * 3
    diff = {k: ([got[k][f] for f in tool.COMPARED], [want[k][f] for f in tool.COMPARED])
            for k in want if any(got[k][f] != want[k][f] for f in tool.COMPARED)}
    assert not diff, diff
