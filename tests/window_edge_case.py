"""The edge of the triangulation's 5 cm median window (pose_estimator_utils.py:73: `dist_to_median < 0.05`, doubles), as one
constructible frame: a noise-free person seen by all five Panoptic cameras, joint JOINT at POINT, and the `y` pixel of that joint in
the camera with index CAM moved by t.  Six of the ten camera pairs do not involve the moved camera and stay together, so the upper
median (element 5 of the ten sorted values) is one of them for any t, and the four moved pairs leave the window one after the other
as t grows.  `bisect` finds, on whatever arithmetic `distances` is given (numpy's SVD on the host, mpe_dlt_pairs on the GPU), a t at
which one moved pair sits less than BAND outside the window and a t at which it sits less than BAND inside: a window carried as a
float (0.05000000074505806) keeps the pair at the first t, the reference drops it."""
import json

import numpy as np

POINT = (0.3, -1.2, 0.4)
JOINT = 8
CAM = 2                       # index into parameters.camera_names
WINDOW = 0.05
WINDOW_AS_FLOAT = float(np.float32(0.05))        # 0.05 + 7.45e-10
BAND = 5e-10                  # narrower than WINDOW_AS_FLOAT - WINDOW
BRACKET = (0.0, 160.0)        # px
MAX_STEPS = 80


def body(n_joints=18):
    """[1, J, 3]: JOINT at POINT, the other joints within 0.2 m of it."""
    j = np.arange(n_joints, dtype=np.float64)
    b = np.array(POINT) + 0.15 * np.stack([np.sin(1.0 + j), np.cos(2.0 * j), np.sin(3.0 * j + 0.5)], axis=1)
    b[JOINT] = POINT
    return b[None]


def frame(calib, syn, t):
    """(wire-format frame, owners) with the y pixel of JOINT in camera CAM moved by t."""
    fr, owner = syn.frame_from_bodies(calib, 0, body(len(calib.params.joint_list)))
    cam = calib.params.camera_names[CAM]
    sks = json.loads(fr[cam][0])
    sks[0][str(JOINT)][2] = sks[0][str(JOINT)][2] + float(t)
    fr[cam][0] = json.dumps(sks)
    assert all(str(JOINT) in json.loads(fr[c][0])[0] for c in calib.params.camera_names), 'every camera must see the joint'
    return fr, owner


def moved_pairs(n_cameras=5):
    """Which of the pairs, in combination order, involve CAM."""
    return np.array([CAM in (a, b) for a in range(n_cameras) for b in range(a + 1, n_cameras)])


def window_distances(points, axis):
    """|Y - upper median| of a joint's pair points [n, 3]."""
    d = np.asarray(points, np.float64)[:, axis]
    return np.abs(d - np.sort(d)[len(d) // 2])


def filtered_mean(points, axis, window):
    """(mean, in pair order, of the pairs strictly inside the window; how many)."""
    points = np.asarray(points, np.float64)
    acc, kept = np.zeros(3), 0
    for x, d in zip(points, window_distances(points, axis)):
        if d < window:
            acc, kept = acc + x, kept + 1
    return acc / kept, kept


def bisect(distances):
    """distances(t) -> window_distances of JOINT's ten pairs at displacement t.  -> (t_outside, t_inside, pair, steps): the moved
    pair with the smallest distance at the upper end of BRACKET, a t at which its distance lies in [WINDOW, WINDOW + BAND) and a t at
    which it lies in (WINDOW - BAND, WINDOW)."""
    lo, hi = BRACKET
    d_lo, d_hi = distances(lo), distances(hi)
    moved = moved_pairs()
    assert len(d_hi) == len(moved)
    k = int(np.flatnonzero(moved)[np.argmin(d_hi[moved])])
    assert d_lo[k] < WINDOW <= d_hi[k], ('the bracket does not hold the crossing', d_lo[k], d_hi[k])
    for step in range(1, MAX_STEPS + 1):
        if d_hi[k] < WINDOW + BAND and d_lo[k] > WINDOW - BAND:
            return hi, lo, k, step - 1
        mid = 0.5 * (lo + hi)
        assert lo < mid < hi, 'the bracket is down to one ulp of t and the band is not reached'
        d = distances(mid)
        if d[k] < WINDOW:
            lo, d_lo = mid, d
        else:
            hi, d_hi = mid, d
    raise AssertionError('band of %.1e m not reached in %d steps: %.17g (inside) %.17g (outside)' % (BAND, MAX_STEPS, d_lo[k], d_hi[k]))
