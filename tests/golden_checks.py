"""What the GPU tests assert of ONE golden frame against the arrays the reference produced for it (tests/golden/*.npz, key prefix
`f<n>_`).  The one-frame tests (test_gpu_parity.py, test_gpu_stages.py) and the batched ones (test_gpu_golden_batched.py) call the
same functions on their slices of a frame, so the bounds are stated once.  Everything here takes host arrays except `poses`, which
runs the network on the frame's rows through the engine it is given."""
import json

import numpy as np
import torch

from conftest import env, oracle

FEATURES_ATOL = 5e-7          # rays are 3-term f32 dot products: 2 ulp of the largest term
SCORES_ATOL = 2e-5
ROWS_ATOL = 3e-7
TRI_TOL = 1e-9
LAYER_RTOL = 2e-5             # |a - b| <= tol * max(1, |b|)
LAYER_SCORES_ATOL = 3e-5      # the last layer through mpe_gat_layer (layer 0 ran dense there)


def dense_features(arr, p, num_feats):
    """graph.ndata['h'] of the frame as the reference built it (stored sparse): [N, F]."""
    N = int(arr[p + 'N'])
    feats = np.zeros((N, num_feats), np.float32)
    rc = arr[p + 'feat_rc']
    feats[rc[:, 0], rc[:, 1]] = arr[p + 'feat_v']
    return feats


def head_features(feat, head_cam, arr, p, num_feats):
    """feat [H, J, 10] (mpe_head_features) against the camera block of the reference's head rows."""
    H = len(head_cam)
    dense = np.zeros((H, num_feats), np.float32)
    rc = arr[p + 'feat_rc']
    sel = rc[:, 0] < H
    dense[rc[sel, 0], rc[sel, 1]] = arr[p + 'feat_v'][sel]
    for h in range(H):
        c = head_cam[h]
        want = dense[h, 2 + c * 180: 2 + (c + 1) * 180].reshape(18, 10)
        np.testing.assert_allclose(feat[h], want, rtol=0, atol=FEATURES_ATOL)
        assert dense[h, 0] == 1.0


def dense_rows(got, arr, p, num_feats):
    """got [N, F] (mpe_dense_rows): every entry of the reference's matrix, and the same zeros."""
    want = dense_features(arr, p, num_feats)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=FEATURES_ATOL)
    assert np.array_equal(got == 0, want == 0) or np.abs(got[(got == 0) != (want == 0)]).max() < FEATURES_ATOL


def gat_scores(sc_en, sc_heads, arr, p):
    """Edge-node and head scores of the frame against the reference's node scores (heads first)."""
    want = arr[p + 'scores']
    H = len(sc_heads)
    np.testing.assert_allclose(sc_en, want[H:], rtol=0, atol=SCORES_ATOL)
    np.testing.assert_allclose(sc_heads, want[:H], rtol=0, atol=SCORES_ATOL)


def persons(persons_f, n_f, arr, p):
    """persons_f [Pcap, V], n_f: the reference's clusters, bit for bit.  -> the reference's persons."""
    want = arr[p + 'persons']
    assert int(n_f) == len(want)
    assert np.array_equal(persons_f[:len(want)], want)
    return want


def mlp_rows(rows_f, valid_f, arr, p, n):
    np.testing.assert_allclose(rows_f[:n], arr[p + 'mlp_in'], rtol=0, atol=ROWS_ATOL)
    assert valid_f[:n].all()


_cpu = {}


def _cpu_side(variant, x, what):
    """torch-CPU / exactly evaluated network on rows x (memoised: the batched tests meet the same rows many times)."""
    key = (variant, what, x.shape, x.tobytes())
    if key not in _cpu:
        fn = oracle().mlp_exact if what == 'exact' else oracle().mlp_forward
        _cpu[key] = fn(env(variant).mlp, torch.from_numpy(x)).numpy()
    return _cpu[key]


def poses(engine, variant, arr, p, rows_own, poses_f, n):
    """The error-budget rule of the 3D output.  rows_own [n, width]: the HIP path's own rows of the frame (device tensor),
    poses_f [>= n, J, 3]: what mpe_mlp3d_batch made of them."""
    # MLP on IDENTICAL rows (the reference's): |gpu - ref| is bounded by the two sides' distances
    # to the exactly evaluated network, and the HIP side is the closer one.  No additive slack.
    x_ref = np.ascontiguousarray(arr[p + 'mlp_in'])
    y = engine.mlp_forward(torch.from_numpy(x_ref).cuda()).cpu().numpy()
    exact = _cpu_side(variant, x_ref, 'exact')
    e_cpu = np.abs(arr[p + 'mlp_out'] - exact).max()
    e_gpu = np.abs(y - exact).max()
    assert e_gpu <= e_cpu, (e_gpu, e_cpu)
    assert np.abs(y - arr[p + 'mlp_out']).max() <= e_cpu + e_gpu
    # end to end the HIP path feeds its OWN rows (<= 3e-7 from the reference's).  Same
    # rule on those rows with torch-CPU (= the reference's MLP arithmetic) as the other side;
    # the batched path must give the bits of the stage call and the x10 decode must be exact fp32.
    x_gpu = rows_own[:n].contiguous()
    x_own = np.ascontiguousarray(x_gpu.cpu().numpy())
    y_gpu_own = engine.mlp_forward(x_gpu).cpu().numpy()
    y_cpu_own = _cpu_side(variant, x_own, 'forward')
    ex_own = _cpu_side(variant, x_own, 'exact')
    e_gpu_own, e_cpu_own = np.abs(y_gpu_own - ex_own).max(), np.abs(y_cpu_own - ex_own).max()
    assert e_gpu_own <= e_cpu_own, (e_gpu_own, e_cpu_own)
    got_pose = poses_f[:n]
    assert np.array_equal(got_pose.reshape(n, -1), y_gpu_own * np.float32(10.0))
    # distance to the reference's poses = MLP budget + what the reference network itself makes of
    # the row difference (torch-CPU on both sets of rows) + one fp32 quantum of the decode
    drift = 10 * np.abs(y_cpu_own - arr[p + 'mlp_out']).max()
    q = float(np.spacing(np.float32(np.abs(arr[p + 'poses']).max())))
    d = np.abs(got_pose - arr[p + 'poses']).max()
    assert d <= 10 * (e_gpu_own + e_cpu_own) + drift + q, (d, e_gpu_own, e_cpu_own, drift)
    return d


def has_id_keys(frame):
    return any('ID' in sk for cam in frame for sk in json.loads(frame[cam][0]))


def triangulation(frame, arr, p, tri_f, jv_f, n):
    """tri_f [>= n, J, 3] f64, jv_f [>= n, J]: the reference's joints and validity, for frames without `ID` keys.
    -> the largest deviation (None for a frame with `ID` keys)."""
    if has_id_keys(frame):
        return None
    tv = arr[p + 'tri_valid'].astype(bool)
    assert np.array_equal(jv_f[:n].astype(bool), tv)
    got = tri_f[:n]
    np.testing.assert_allclose(got[tv], arr[p + 'tri'][tv], rtol=TRI_TOL, atol=TRI_TOL)
    return float(np.abs(got[tv] - arr[p + 'tri'][tv]).max()) if tv.any() else 0.0


def close(a, b, tol):
    """|a - b| <= tol * max(1, |b|): activations reach a few units; fp32 reordering noise scales
    with the magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) <= tol


def layer_activations(got, H, arr, p, l):
    """got [N, heads*out_dim]: layer l's output rows of the frame (heads, then edge-nodes) against the rows the REFERENCE kept
    (rows [0:4] and [H:H+4] of its N x HD matrix)."""
    nh = min(4, H)
    assert close(got[:nh], arr[p + 'act%d_head' % l][:nh], LAYER_RTOL), (l, 'head rows vs reference')
    want_en = arr[p + 'act%d_en' % l]
    assert close(got[H:H + len(want_en)], want_en, LAYER_RTOL), (l, 'edge-node rows vs reference')
