"""Camera calibration for the inference path.

Restates the "calibration globals" every hot-path module of the reference builds at
import time (graph_generator.py:32-52, pose_estimator_dataset_from_json.py:28-47,
metrics_from_triangulation.py:54-72, pose_estimator_utils.py:17-30):

  T_d[c]  = tm.get_transform("root", cam)        4x4 f64 (stored matrix)
  T_i[c]  = tm.get_transform(cam, "root")        4x4 f64, inverse of T_d
  K[c]    = [[fx,0,cx],[0,fy,cy],[0,0,1]]        f32 (torch.tensor of python floats)
  Kinv[c] = torch.inverse(K[c])                  f32
  centre  = T_i(f32) @ [0,0,0,1]                 f32
  dist[c] = [kd0, kd1, p1, p2, kd2]              f64 (OpenCV order k1,k2,p1,p2,k3)
  P[c]    = T_d[c][0:3, :]                       3x4 f64

The extrinsics come from a pickled ``pytransform3d.transform_manager.TransformManager``
(pytransform3d 1.9.1, not vendored by the reference).  That package is not in this
image; `TransformManager` below restates the two code paths the reference uses
(`get_transform` of a stored edge and of its reverse = ``numpy.linalg.inv`` of the
stored 4x4, as pytransform3d's ``invert_transform`` does) and the pickle is read with
a restricted unpickler that only materialises numpy arrays.
"""
import io
import json
import os
import pickle

import numpy as np
import torch

_DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data')


class TransformManager:
    """Minimal stand-in for pytransform3d's TransformManager (direct edges only)."""

    def __init__(self, transforms=None):
        self.transforms = dict(transforms or {})

    def __setstate__(self, state):
        self.transforms = dict(state.get('transforms', {}))

    def add_transform(self, from_frame, to_frame, A2B):
        self.transforms[(from_frame, to_frame)] = np.asarray(A2B, dtype=np.float64)
        return self

    def get_transform(self, from_frame, to_frame):
        key = (from_frame, to_frame)
        if key in self.transforms:
            return self.transforms[key]
        rev = (to_frame, from_frame)
        if rev in self.transforms:
            return np.linalg.inv(self.transforms[rev])
        raise KeyError('Cannot compute path from frame %r to frame %r' % key)


class _Opaque:
    """Placeholder for pickled classes we do not need (scipy csr_matrix, ...)."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self._state = state


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module == 'pytransform3d.transform_manager' and name == 'TransformManager':
            return TransformManager
        if module in ('numpy.core.multiarray', 'numpy._core.multiarray') and \
                name in ('_reconstruct', 'scalar'):
            import numpy.core.multiarray as m
            return getattr(m, name)
        if module == 'numpy' and name in ('ndarray', 'dtype'):
            return getattr(np, name)
        return type(name, (_Opaque,), {})


def load_transform_manager(path):
    """Load a ``tm_*.pickle`` (reference format) or our ``tm_*.json`` (hex floats)."""
    if path.endswith('.json'):
        with open(path) as fh:
            doc = json.load(fh)
        tm = TransformManager()
        for t in doc['transforms']:
            mat = np.array([[float.fromhex(x) for x in row] for row in t['matrix']], dtype=np.float64)
            tm.add_transform(t['from'], t['to'], mat)
        return tm
    with open(path, 'rb') as fh:
        tm = _RestrictedUnpickler(io.BytesIO(fh.read())).load()
    if not isinstance(tm, TransformManager):
        raise TypeError('%s does not hold a TransformManager' % path)
    return tm


def load_intrinsics(path, params=None):
    """The "intrinsics" list of a ``tm_*.json`` that harness.camfit wrote -> (k [n,4] float32, dist [n,5] float64) in the
    order of ``params.camera_names`` (default: the package's parameters), what Calibration takes as `intrinsics`; None
    when the file has no such list."""
    if params is None:
        from .parameters import parameters as params
    with open(path) as fh:
        doc = json.load(fh)
    if 'intrinsics' not in doc:
        return None
    by_name = {e['camera']: e for e in doc['intrinsics']}
    k = np.array([[float.fromhex(by_name[c][key]) for key in ('fx', 'fy', 'cx', 'cy')] for c in params.camera_names], np.float32)
    dist = np.array([[float.fromhex(x) for x in by_name[c]['dist']] for c in params.camera_names], np.float64)
    return k, dist


def default_transform_path(params):
    """Resolve ``parameters.transformations_path`` the way the reference does (cwd
    relative), falling back to the calibration shipped with this package."""
    p = params.transformations_path
    if p and os.path.exists(p):
        return p
    base = os.path.splitext(os.path.basename(p or 'tm_panoptic.pickle'))[0]
    return os.path.join(_DATA_DIR, base + '.json')


def camera_matrix_f32(params, cam_idx):
    """3x3 f32 intrinsics, as pose_estimator_utils.camera_matrix (reference :17-30)."""
    return torch.tensor([[params.fx[cam_idx], 0.0, params.cx[cam_idx]],
                         [0.0, params.fy[cam_idx], params.cy[cam_idx]],
                         [0.0, 0.0, 1.0]])


class Calibration:
    """All per-camera constants of the path, indexed by position in
    ``params.camera_names`` (== ``used_cameras`` for the shipped presets)."""

    def __init__(self, params, tm=None, intrinsics=None):
        """intrinsics: None (the numbers of `params`), or (k [n,4]: fx fy cx cy, dist [n,5]) in the order of
        ``params.camera_names``: K32 is built from the four numbers rounded to float32, dist is taken as given."""
        if tm is None:
            tm = load_transform_manager(default_transform_path(params))
        self.params = params
        self.tm = tm
        if intrinsics is not None:
            k, dist = intrinsics
            k, dist = np.array(k, np.float32), np.array(dist, np.float64)
            if k.shape != (len(params.camera_names), 4) or dist.shape != (len(params.camera_names), 5) or \
                    not (np.isfinite(k).all() and np.isfinite(dist).all() and (k[:, :2] > 0).all()):
                raise ValueError('intrinsics must be finite k [%d,4] with fx, fy > 0 and dist [%d,5]' % ((len(params.camera_names),) * 2))
            intrinsics = (k, dist)
        self._intrinsics = intrinsics
        names = list(params.camera_names)
        self.names = names
        n = len(names)
        self.T_d = np.zeros((n, 4, 4), np.float64)
        self.T_i = np.zeros((n, 4, 4), np.float64)
        self.T_i32 = np.zeros((n, 4, 4), np.float32)
        self.K32 = np.zeros((n, 3, 3), np.float32)
        self.Kinv32 = np.zeros((n, 3, 3), np.float32)
        self.centre32 = np.zeros((n, 4), np.float32)
        self.dist = np.zeros((n, 5), np.float64)
        self.P = np.zeros((n, 3, 4), np.float64)
        for i, cam in enumerate(names):
            self.T_d[i] = tm.get_transform('root', cam)
            self.T_i[i] = tm.get_transform(cam, 'root')
            ti = torch.from_numpy(self.T_i[i]).type(torch.float32)
            self.T_i32[i] = ti.numpy()
            if intrinsics is None:
                k = camera_matrix_f32(params, params.cameras[i])
            else:
                fx, fy, cx, cy = (float(x) for x in intrinsics[0][i])
                k = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
            self.K32[i] = k.numpy()
            self.Kinv32[i] = torch.inverse(k).numpy()
            self.centre32[i] = torch.matmul(ti, torch.tensor([0.0, 0.0, 0.0, 1.0])).numpy()
            ci = params.cameras[i]
            self.dist[i] = [params.kd0[ci], params.kd1[ci], params.p1[ci], params.p2[ci], params.kd2[ci]] if intrinsics is None else intrinsics[1][i]
            self.P[i] = self.T_d[i][0:3, :]

    @property
    def n_cameras(self):
        return len(self.names)

    def index(self, cam_name):
        return self.names.index(cam_name)

    def with_extrinsics(self, E):
        """A new Calibration with root -> camera i given by E[i] (3 x 4, or 4 x 4 whose last row is 0 0 0 1), E in the
        order of ``names``: T_d, T_i, T_i32, centre32 and P are rebuilt from E the way __init__ builds them from the
        transform manager (T_i = numpy.linalg.inv of the stored matrix); intrinsics and distortion are kept.  This
        object is not modified."""
        E = np.asarray(E, dtype=np.float64)
        if E.shape not in ((self.n_cameras, 3, 4), (self.n_cameras, 4, 4)) or not np.isfinite(E).all():
            raise ValueError('E must be finite and [%d,3,4] or [%d,4,4]' % (self.n_cameras, self.n_cameras))
        tm = TransformManager()
        for i, cam in enumerate(self.names):
            T = np.eye(4)
            T[:3, :] = E[i][:3, :]
            tm.add_transform('root', cam, T)
        return Calibration(self.params, tm, self._intrinsics)

    def intrinsics(self):
        """-> k [n,4] float32: fx, fy, cx, cy of every camera, read out of K32."""
        return np.ascontiguousarray(np.stack([self.K32[:, 0, 0], self.K32[:, 1, 1], self.K32[:, 0, 2], self.K32[:, 1, 2]], axis=1), np.float32)

    def with_intrinsics(self, k, dist):
        """A new Calibration with K32 rebuilt from k [n,4] (fx, fy, cx, cy, rounded to float32), Kinv32 by torch.inverse as
        __init__ does it, and dist [n,5] in the place of the stored one, in the order of ``names``; the extrinsics are
        kept, ``params`` is untouched and this object is not modified."""
        return Calibration(self.params, self.tm, (k, dist))
