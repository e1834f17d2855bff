"""Inputs for the time-aware refinement tests (test_refine_timed_host.py: harness/refine_timed.py on its own;
test_gpu_refine_timed.py: mpe_refine_timed_batch against it).  The scenes are those of the lag tests: bodies on seeded
walks, every camera seeing them at its own time, persons and ids from the generator's ownership.  Not a test module."""
import math

import numpy as np

from lag_cases import ALL_JOINTS, J, Scene, messy, same_bits  # noqa: F401  (the tests take them from here)
from conftest import pkg

KEYS = ('poses', 'status', 'cost0', 'cost1', 'iters', 'n_views', 'n_timed')
SHARED = KEYS[:6]                                             # what mpe_refine_batch writes, too
LAGS = (0, 0.5, -0.25, 1.25, -1.5)                            # the issue's scene: every fractional part a binary fraction
MESSY_LAGS = (0, 1.5, -0.5, 0, 2)


def RT():
    return pkg('harness.refine_timed')


def RF():
    return pkg('harness.refine')


def table_of(scene, kind, poses=None):
    p, flags, _ = scene.kinds[kind]
    return (p if poses is None else poses, flags, scene.n_persons, scene.ids)


def statement(scene, kind, lags, table=None, frames=None, **kw):
    """refine_timed over the scene, or over the frames [a, b) of it packed on their own, against the whole table (or
    `table` = (poses, flags, n_persons, ids))."""
    mask = scene.kinds[kind][2]
    tab = table_of(scene, kind) if table is None else table
    a, b = (0, scene.pb.n_frames) if frames is None else frames
    pb = scene.pb if frames is None else scene.sub_batch(a, b)
    return RT().refine_timed(scene.calib, pb, a, scene.persons[a:b], *tab, lags, mask, **kw)


def untimed(scene, kind, poses=None, **kw):
    """harness.refine.refine over the scene from the kind's poses (or `poses`)."""
    p, flags, mask = scene.kinds[kind]
    return RF().refine(scene.calib, scene.pb, scene.persons, scene.n_persons, p if poses is None else poses, flags, mask, **kw)


def rms_mm(poses, truth, where):
    """RMS distance in millimetres over the joints `where` [F,Pcap,J]."""
    d = np.linalg.norm(np.asarray(poses, np.float64) - truth, axis=-1)[where]
    return 1e3 * float(np.sqrt((d * d).mean()))


def every_camera_timed(scene, kind, lags, out):
    """-> [F,Pcap,J] bool: the solved joints of `out` whose every observing camera with a lag used an offset."""
    _, flags, mask = scene.kinds[kind]
    sel, _ = pkg('harness.reprojection').selection(scene.pb, scene.persons, scene.n_persons, flags, mask, 0.5)
    lagged = sel[:, :, [c for c, x in enumerate(lags) if x != 0]].sum(axis=2)
    return ((out['status'] & 1) != 0) & (lagged > 0) & (out['n_timed'] == lagged)


def expected_timed(scene, kind, lags):
    """The header's rule for a timed camera, joint by joint in plain loops (no array code shared with the statement) ->
    timed [F,Pcap,V,J] bool."""
    poses, flags, mask = scene.kinds[kind]
    ids, n_persons = scene.ids, scene.n_persons
    n_table, pcap = ids.shape
    sel, _ = pkg('harness.reprojection').selection(scene.pb, scene.persons, n_persons, flags, mask, 0.5)

    def row(g, t):
        if not 0 <= g < n_table:
            return -1
        for p in range(min(max(int(n_persons[g]), 0), pcap)):
            if ids[g, p] == t and (flags.ndim == 3 or flags[g, p]):
                return p
        return -1

    def good(g, r, j):
        return r >= 0 and bool(flags[g, r, j] if flags.ndim == 3 else flags[g, r]) and bool(np.isfinite(poses[g, r, j]).all())

    out = np.zeros(sel.shape, bool)
    for f in range(n_table):
        for p in range(pcap):
            t = int(ids[f, p])
            for c, L in enumerate(lags):
                if L == 0 or t < 0 or not sel[f, p, c].any():
                    continue
                s = math.floor(L)
                need = [f, f + s] + ([f + s + 1] if L != s else [])
                rows = [row(g, t) for g in need]
                for j in range(J):
                    out[f, p, c, j] = sel[f, p, c, j] and all(good(g, r, j) for g, r in zip(need, rows))
    return out
