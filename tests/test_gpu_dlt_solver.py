"""GPU: the one two-view DLT solver (csrc/dlt_solve.h) through every kernel that calls it.  mpe_dlt_pairs on the seeded systems of
dlt_cases.py against numpy's SVD, with the bounds of the host test; then the row kernel, the triangulation kernel and the small-batch
pair launch against the same pairs pushed through mpe_dlt_pairs: one definition, so the same bits."""
import numpy as np
import pytest
import torch

import dlt_cases as dc
from conftest import env, oracle, pkg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('variant', ['panoptic', 'arplab'])
def test_dlt_pairs_against_lapack(variant):
    """4000 pairs of one calibration in one launch: matched pairs to 1e-10 m of LAPACK's point, the well-posed mismatched ones to
    1e-10 m x max(1, |X|), every mismatched one the right vector by its residual."""
    e = env(variant)
    s = dc.systems(variant)
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=2, max_persons_per_camera=2)
    try:
        X = eng.dlt_pairs(s.pix, s.cams)
        eng.sync_status()
        dc.check(s, X.cpu().numpy(), 'gpu')
    finally:
        eng.close()


@pytest.fixture(scope='module')
def engine(calib, gat_weights, mlp_weights):
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=64, max_persons_per_camera=6)
    sd, prm = gat_weights
    eng.load_gat(sd, prm)
    eng.load_mlp(mlp_weights)
    yield eng
    eng.close()


def person_pairs(host, persons, n_persons, V, J, masks):
    """(frame, person, joint, first pixel point, second, cameras) of every pair the 3D kernels solve, in their order: frame, person,
    joint, camera pairs lexicographically; a camera takes part when the person has a head there whose mask holds the joint."""
    xy = np.asarray(host.xy).reshape(-1, J, 2)
    key, pts, cams = [], [], []
    for f in range(len(n_persons)):
        h0 = int(host.frame_head_off[f])
        for p in range(int(n_persons[f])):
            heads = [h0 + int(h) if h >= 0 else -1 for h in persons[f, p]]
            for j in range(J):
                seen = [c for c in range(V) if heads[c] >= 0 and (int(masks[heads[c]]) >> j) & 1]
                for a in range(len(seen)):
                    for b in range(a + 1, len(seen)):
                        c1, c2 = seen[a], seen[b]
                        key.append((f, p, j))
                        pts.append(np.concatenate([xy[heads[c1], j], xy[heads[c2], j]]))
                        cams.append((c1, c2))
    return key, np.array(pts, np.float64).reshape(-1, 4), np.array(cams, np.int32).reshape(-1, 2)


def grouped(key, X):
    out = {}
    for k, x in zip(key, X):
        out.setdefault(k, []).append(x)
    return out


@pytest.mark.parametrize('n_frames', [3, 40])
def test_every_call_site_gives_the_bits_of_dlt_pairs(engine, calib, n_frames):
    """5 cameras x 4 persons with 1 px of noise and dropped joints, 3 frames (the small-batch route: the pairs are solved beside the
    clustering by k_lat_tail and fetched by the row kernel) and 40 (the row kernel solves them).  The triangulated joints in the MLP's
    input rows are the mean, in pair order, of the same pairs through mpe_dlt_pairs; mlp3d's poses are the network on exactly those
    rows; triangulate's joints are the median-filtered mean of the same pairs.  All of it bit for bit."""
    syn = pkg('synthetic')
    V, J, npj = engine.V, engine.J, engine.params.numbers_per_joint
    frames = [oracle().processed_input(syn.make_frame(calib, 900 + i, syn.FrameSpec(persons=4, noise_px=1.0, joint_drop=0.1 if i % 2 else 0.0))[0])
              for i in range(n_frames)]
    db = engine.to_device(engine.pack(frames))
    _, persons, n_persons = engine.match(db)
    poses, _ = engine.mlp3d(db, persons, n_persons)
    rows, _ = engine.mlp_input_rows(db, persons, n_persons)
    tri, jv = engine.triangulate(db, persons, n_persons, all_joints=True)
    engine.sync_status()
    pn, nn = persons.cpu().numpy(), n_persons.cpu().numpy()
    assert nn.sum() >= 3 * n_frames
    # the rows: float32((mean over pairs) / 10) in the columns 11..13 of every camera block, pairs on the tri mask
    key, pts, cams = person_pairs(db.host, pn, nn, V, J, db.host.tri_mask)
    assert len(key) > 100 * n_frames
    X = grouped(key, engine.dlt_pairs(pts, cams).cpu().numpy())
    rows_np = rows.cpu().numpy().reshape(n_frames, engine.pcap, V, J, npj)
    for (f, p, j), xs in X.items():
        acc = np.zeros(3)
        for x in xs:
            acc = acc + x
        want = ((acc / len(xs)) / 10.0).astype(np.float32)
        assert np.array_equal(rows_np[f, p, :, j, 11:14], np.broadcast_to(want, (V, 3))), (f, p, j)
    # mlp3d on the same batch (3 frames: rows from the pairs k_lat_tail solved): the network on those rows, times ten
    sel = torch.tensor([(f, p) for f in range(n_frames) for p in range(int(nn[f]))], device=rows.device)
    y = engine.mlp_forward(rows[sel[:, 0], sel[:, 1]].contiguous())
    assert torch.equal(poses[sel[:, 0], sel[:, 1]].reshape(len(sel), -1), y * 10.0)
    # triangulate: pairs on the joint mask, upper median of the Y axis, mean of the pairs within the window of it
    key, pts, cams = person_pairs(db.host, pn, nn, V, J, db.host.joint_mask)
    X = grouped(key, engine.dlt_pairs(pts, cams).cpu().numpy())
    axis, win = engine.params.axes_3D['Y'][0], 0.05
    tri_np, jv_np = tri.cpu().numpy(), jv.cpu().numpy()
    for f in range(n_frames):
        for p in range(int(nn[f])):
            for j in range(J):
                xs = X.get((f, p, j))
                assert bool(jv_np[f, p, j]) == (xs is not None)
                if xs is None:
                    continue
                med = sorted(x[axis] for x in xs)[len(xs) // 2]
                acc, kept = np.zeros(3), 0
                for x in xs:
                    if abs(x[axis] - med) < win:
                        acc, kept = acc + x, kept + 1
                assert np.array_equal(tri_np[f, p, j], acc / kept), (f, p, j)


def test_triangulate_window_edge(engine, calib):
    """The 5 cm median window is the reference's `dist_to_median < 0.05` in doubles (pose_estimator_utils.py:73), to the last bit: the
    frame of window_edge_case.py, persons from the clustering kernel on the ground-truth pairing, and a bisection on the displacement
    t of one pixel that runs on the GPU's own pair points (mpe_dlt_pairs; numpy's differ by up to ~1e-10 m, the band is 5e-10).  At
    the t where one moved pair sits within 5e-10 m OUTSIDE the window the joint is the mean of the pairs strictly inside 0.05 -- the
    pair is dropped -- and at the t where it sits within 5e-10 m inside it is kept.  A window carried as a float (0.05 + 7.45e-10)
    keeps the pair at both."""
    import window_edge_case as we
    syn, common = pkg('synthetic'), pkg('harness.common')
    V, J = engine.V, engine.J
    axis = engine.params.axes_3D['Y'][0]
    assert V == 5 and we.JOINT in engine.params.used_joints

    def solve(t):
        fr, owner = we.frame(calib, syn, t)
        db = engine.to_device(engine.pack([oracle().processed_input(fr)], keep_json=True))
        persons, n_persons = engine.cluster(db, common.teacher_scores(db, [owner]))
        pn, nn = persons.cpu().numpy(), n_persons.cpu().numpy()
        assert nn[0] == 1 and (pn[0, 0] >= 0).all()                # one person, seen by all five cameras
        key, pts, cams = person_pairs(db.host, pn, nn, V, J, db.host.joint_mask)
        X = grouped(key, engine.dlt_pairs(pts, cams).cpu().numpy())[(0, 0, we.JOINT)]
        assert len(X) == 10
        return db, persons, n_persons, np.array(X)

    t_out, t_in, k, steps = we.bisect(lambda t: we.window_distances(solve(t)[3], axis))
    kept = {}
    for name, t in (('inside', t_in), ('outside', t_out)):
        db, persons, n_persons, X = solve(t)                        # the frame packed again at this t
        d = we.window_distances(X, axis)[k]
        want, kept[name] = we.filtered_mean(X, axis, we.WINDOW)
        tri, jv = engine.triangulate(db, persons, n_persons, all_joints=True)
        engine.sync_status()
        got = tri[0, 0, we.JOINT].cpu().numpy()
        print('%s: t = %.12f px, distance - 0.05 = %.3g m, %d of 10 pairs inside 0.05, |kernel - expected| = %.3g m (%d steps)'
              % (name, t, d - we.WINDOW, kept[name], np.abs(got - want).max(), steps))
        assert (we.WINDOW <= d < we.WINDOW + we.BAND) if name == 'outside' else (we.WINDOW - we.BAND < d < we.WINDOW)
        assert bool(jv[0, 0, we.JOINT])
        assert np.array_equal(got, want), (name, t, got, want)
    assert kept['outside'] == kept['inside'] - 1, kept
