"""harness/geometric.py on its own (CPU): the distance against an independent formula, the rays against the generator's
projection, the clustering of its scores against the generator's ground-truth pairing, and what it refuses."""
import numpy as np
import pytest

import geom_cases as gc
from conftest import env, oracle, pkg


def test_distance_is_the_common_perpendicular():
    """(a) votes that are neither clamped nor parallel: dist = |w . (r1 x r2)| / |r1 x r2|, to 1e-9 m."""
    G = pkg('harness.geometric')
    seen = 0
    for name in ('clean', 'noisy', 'messy', 'arplab'):
        c = gc.case(name)
        w = c.statement(clip=0.0)
        pairs = G.batch_pairs(c.pb)
        o, r = G.rays(c.calib, c.pb.head_cam, c.pb.xy)
        r1, r2 = r[pairs[:, 0]], r[pairs[:, 1]]
        ww = (o[c.pb.head_cam[pairs[:, 0]]] - o[c.pb.head_cam[pairs[:, 1]]])[:, None, :]
        n = np.cross(r1, r2)
        with np.errstate(all='ignore'):
            want = np.abs((ww * n).sum(axis=-1)) / np.linalg.norm(n, axis=-1)
        plain = w['vote'] & ~w['clamped'] & ~w['parallel']
        err = np.abs(w['dist'] - want)[plain]
        print(name, 'plain votes', int(plain.sum()), 'of', int(w['vote'].sum()), 'max |dist - independent|', err.max())
        assert plain.any() and err.max() <= 1e-9
        seen += int(plain.sum())
    assert seen > 1000


def test_rays_reproject_onto_their_pixels():
    """(b) noise-free frames (clean, 5x10, c1): a point on the ray projects back onto the pixel the ray was made from, to
    1e-6 px.  (undistort_point's five iterations alone leave 1.5e-2 px on `clean`; the rule's two Newton steps bring the
    worst pixel of the three cases to 2.2e-7 px.)"""
    G, syn = pkg('harness.geometric'), pkg('synthetic')
    worst = {}
    for name in ('clean', '5x10', 'c1'):
        c = gc.case(name)
        pb, calib = c.pb, c.calib
        o, r = G.rays(calib, pb.head_cam, pb.xy)
        assert np.allclose(np.linalg.norm(r, axis=-1), 1.0, rtol=0, atol=4e-16)
        idx = [calib.index(n) for n in c.params.used_cameras_skeleton_matching]
        errs = []
        for h in range(pb.n_heads):
            k = idx[int(pb.head_cam[h])]
            js = [j for j in range(pb.J) if (int(pb.joint_mask[h]) >> j) & 1]
            for s in (1.5, 4.0):
                X = o[pb.head_cam[h]][None, :] + s * r[h, js]
                uv, z = syn.project_panoptic(X.T, calib.K32[k].astype(np.float64), calib.T_d[k], calib.dist[k])
                assert (z > 0).all()
                errs.append(np.abs(uv.T - pb.xy[h, js]).max(axis=1))
        errs = np.concatenate(errs)
        worst[name] = float(errs.max())
        print(name, 'reprojection of a ray point, px: max %.3g, median %.3g, share within 1e-6 px %.3f' % (errs.max(), np.median(errs), (errs <= 1e-6).mean()))
    assert max(worst.values()) <= 1e-6, worst


@pytest.mark.parametrize('persons,noise,sigma', [(4, 0.0, 0.10), (4, 2.0, 0.10), (10, 0.0, 0.10), (10, 2.0, 0.05)])
def test_clusters_are_the_true_partition(persons, noise, sigma):
    """(c) 32 frames of the generator: the statement's scores through the oracle's clustering give, in every frame, exactly
    the persons seen by two cameras or more."""
    G, syn, onp = pkg('harness.geometric'), pkg('synthetic'), oracle()
    e = env()
    frames, gts = syn.make_frames(e.calib, 32, syn.FrameSpec(persons=persons, noise_px=noise), seed=1234)
    c = gc.Case.__new__(gc.Case)
    c.params, c.calib, c.owners = e.params, e.calib, [g['owner'] for g in gts]
    c.pb = pkg('packing').pack_frames([onp.processed_input(f) for f in frames], e.params)
    sc = G.scores(e.calib, c.pb, sigma=sigma, clip=0.5, min_joints=1)['scores']
    got = gc.oracle_persons(c, sc)
    good = 0
    for f in range(32):
        mine = {frozenset(h for h in p if h >= 0) for p in got[f]}
        good += mine == gc.true_partition(c, f)
    print('persons', persons, 'noise', noise, 'sigma', sigma, 'frames with the true partition:', good, 'of 32')
    assert good == 32


def test_arguments():
    """(d) what the statement refuses."""
    G = pkg('harness.geometric')
    c = gc.case('c1')
    for kw in ({'sigma': 0.0}, {'sigma': -1.0}, {'sigma': float('nan')}, {'clip': -0.1}, {'min_joints': 0}, {'min_joints': gc.J + 1},
               {'min_conf': -0.5}):
        with pytest.raises(ValueError):
            G.scores(c.calib, c.pb, **kw)
    w = G.scores(c.calib, c.pb, joint_mask=0)
    assert gc.same_bits(w['scores'], c.statement()['scores'])


def test_cases_hit_their_branches():
    """Every case of the GPU tests builds, and its own assertions (geom_cases.Case.check) hold."""
    for name in gc.NAMES:
        c = gc.case(name)
        w = c.statement()
        print(name, 'frames', c.pb.n_frames, 'heads', c.pb.n_heads, 'edge-nodes', c.pb.n_edge_nodes, 'votes', int(w['vote'].sum()),
              'clamped', int(w['clamped'].sum()), 'parallel', int(w['parallel'].sum()))
        assert len(w['scores']) == c.pb.n_edge_nodes and w['scores'].dtype == np.float32
