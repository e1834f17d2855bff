"""numpy statement of what mpe_reproject_batch and mpe_residual_stats compute (csrc/reproject.hip), and of the
bookkeeping of test/reprojection_error.py around them.  The GPU tests hold the kernels to this module bit for bit; with
the oracle as the inference side it replays the reference's report on the CPU.

Projection.  `get_projected_coordinates` (reprojection_error.py:89-107) in float32, every operation rounded on its own
(nothing fused), divisions and roots correctly rounded, in this order:

    T  = float32(calib.P[c])                    rows 0..2 of root -> camera (camera_d_transforms, :78)
    kd = float32(calib.dist[c][0], [1], [4])    radial terms only (get_distortion_coefficients)
    pc_i = ((T[i][0]*X + T[i][1]*Y) + T[i][2]*Z) + T[i][3]
    h0 = pc_0 / pc_2 ; h1 = pc_1 / pc_2
    n  = sqrt(h0*h0 + h1*h1) ; r = n*n          (:100-101: the norm, then its square)
    f  = ((1 + kd0*r) + (kd1*r)*r) + ((kd2*r)*r)*r
    d0 = h0*f ; d1 = h1*f
    u_i = (K[c][i][0]*d0 + K[c][i][1]*d1) + K[c][i][2]
    px = u_0 / u_2 ; py = u_1 / u_2
    res = sqrt((float64(px) - x)*(float64(px) - x) + (float64(py) - y)*(float64(py) - y))      float64 (:366)

Selection.  res[f][p][c][j] is counted when p < n_persons[f], persons[f][p][c] names a head, bit j of the joint mask is
set, the pose flag (per person) or joint flag (per joint) is on, joint j is in that skeleton's dict and its `valid`
(the float32 of the packed batch) is > 0.5 (:365, strict).  Everything else is SENTINEL (negative).

Statistics.  Per camera over any number of residual arrays: the count of entries >= 0, their mean and np.median, the
count of non-finite entries; a NaN entry makes mean and median NaN, as numpy does.  An entry of -0.0 counts as 0.
"""
import numpy as np

from .assignment import error_table

SENTINEL = -1.0
TRANSFORM_NAME = 'add_joint2_from_minus1'


def add_joint2_from_minus1(frames):
    """The derived --showgt input: every GT body that has '-1' and no '2' gets '2' as a copy of '-1' (in place).
    -> the number of bodies changed.  Bodies without '-1' stay as they are (invalid, :203-204)."""
    n = 0
    for frame in frames:
        for cam in frame:
            if len(frame[cam]) < 4:
                continue
            for body in frame[cam][3]:
                if '-1' in body and '2' not in body:
                    body['2'] = list(body['-1'])
                    n += 1
    return n


def engine_cameras(calib):
    """Indices into the calibration's arrays of the cameras an Engine is built for, in its order."""
    return [calib.index(c) for c in calib.params.used_cameras_skeleton_matching]


def engine_calibration(calib):
    """-> (P [V,3,4] float64, dist [V,5] float64, K32 [V,3,3] float32) as the calibration stores them, over the cameras an
    Engine is built for, in its order: row c belongs to camera slot c, the index head_cam and the columns of `persons`
    hold.  A calibration may configure more cameras than are used (a camera-subset preset), so its own arrays are not
    indexed by slot; every statement module takes its camera constants from here."""
    idx = engine_cameras(calib)
    return (np.ascontiguousarray(np.asarray(calib.P, np.float64)[idx]), np.ascontiguousarray(np.asarray(calib.dist, np.float64)[idx]),
            np.ascontiguousarray(np.asarray(calib.K32, np.float32)[idx]))


def camera_constants(calib):
    """-> (T [V,3,4], kd [V,3], K [V,3,3]) float32, by camera slot (engine_calibration)."""
    P, dist, K32 = engine_calibration(calib)
    return P.astype(np.float32), np.ascontiguousarray(dist[:, [0, 1, 4]]).astype(np.float32), K32


def project(T, kd, K, X, Y, Z):
    """float32 arrays that broadcast against each other: T [...,3,4], kd [...,3], K [...,3,3], X / Y / Z [...]
    -> (px, py) float32, the arithmetic of the module docstring."""
    f32 = np.float32
    X, Y, Z = (np.asarray(a, f32) for a in (X, Y, Z))
    with np.errstate(all='ignore'):
        pc = [((T[..., i, 0] * X + T[..., i, 1] * Y) + T[..., i, 2] * Z) + T[..., i, 3] for i in range(3)]
        h0 = pc[0] / pc[2]
        h1 = pc[1] / pc[2]
        n = np.sqrt(h0 * h0 + h1 * h1)
        r = n * n
        f = ((f32(1) + kd[..., 0] * r) + (kd[..., 1] * r) * r) + ((kd[..., 2] * r) * r) * r
        d0 = h0 * f
        d1 = h1 * f
        u = [(K[..., i, 0] * d0 + K[..., i, 1] * d1) + K[..., i, 2] for i in range(3)]
        px = u[0] / u[2]
        py = u[1] / u[2]
    assert px.dtype == np.float32 and py.dtype == np.float32
    return px, py


def pixel_distance(px, py, x, y):
    """float32 projection against the float64 detection -> float64 distance (:366)."""
    with np.errstate(all='ignore'):
        dx = np.asarray(px, np.float32).astype(np.float64) - x
        dy = np.asarray(py, np.float32).astype(np.float64) - y
        return dx * dx + dy * dy, np.sqrt(dx * dx + dy * dy)


def selection(pb, persons, n_persons, flags, joint_mask, threshold=0.5):
    """The module docstring's selection -> (sel [F,Pcap,V,J] bool, xy [F,Pcap,V,J,2] float64: the detection each counted
    entry is compared with; unspecified where sel is False).  harness/refine.py takes its observing cameras from here."""
    persons = np.asarray(persons)
    F, Pcap, V = persons.shape
    J = pb.J
    if F == 0 or pb.n_heads == 0:
        return np.zeros((F, Pcap, V, J), bool), np.zeros((F, Pcap, V, J, 2), np.float64)
    flags = np.asarray(flags) != 0
    n_persons = np.asarray(n_persons).astype(np.int64)
    off = np.asarray(pb.frame_head_off).astype(np.int64)
    n_heads = (off[1:F + 1] - off[:F])[:, None, None]
    ok = (np.arange(Pcap)[None, :, None] < n_persons[:, None, None]) & (persons >= 0) & (persons < n_heads)
    head = np.where(ok, off[:F, None, None] + persons, 0)
    j = np.arange(J)
    in_dict = ((np.asarray(pb.joint_mask)[head][..., None] >> j.astype(np.uint32)) & 1) != 0
    xy = np.asarray(pb.xy, np.float64).reshape(-1, J, 2)[head]                # [F,Pcap,V,J,2]
    valid = np.asarray(pb.vp, np.float32).reshape(-1, J, 2)[head][..., 0]
    picked = ((int(joint_mask) >> j) & 1) != 0
    flag = flags[:, :, None, :] if flags.ndim == 3 else flags[:, :, None, None]
    return ok[..., None] & in_dict & picked & flag & (valid > np.float32(threshold)), xy


def residuals(calib, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, squared=False):
    """pb: the packed batch (host arrays); persons [F,Pcap,V] / n_persons [F] as the matching stage wrote them; poses
    [F,Pcap,J,3] float32 or float64 (rounded to float32 first, :405); flags [F,Pcap] (per person) or [F,Pcap,J] (per
    joint); joint_mask: bit j selects joint j.  -> res [F,Pcap,V,J] float64 (squared=True: the squared distances)."""
    F, Pcap, V = np.asarray(persons).shape
    J = pb.J
    if F == 0:
        return np.zeros((0, Pcap, V, J), np.float64)
    if pb.n_heads == 0:
        return np.full((F, Pcap, V, J), SENTINEL)
    poses = np.asarray(poses).astype(np.float32)
    sel, xy = selection(pb, persons, n_persons, flags, joint_mask, threshold)
    T, kd, K = camera_constants(calib)
    px, py = project(T[None, None, :, None], kd[None, None, :, None], K[None, None, :, None],
                     poses[:, :, None, :, 0], poses[:, :, None, :, 1], poses[:, :, None, :, 2])
    sq, res = pixel_distance(px, py, xy[..., 0], xy[..., 1])
    return np.where(sel, sq if squared else res, SENTINEL)


def stats(res_list):
    """One or more residual arrays [..., V, J] -> {'count' [V] int64, 'nonfinite' [V] int64, 'sum', 'mean', 'median',
    'mid' [V,2]} with numpy's own mean / median over the entries >= 0 of every camera (NaN entries poison both)."""
    res_list = [np.asarray(r, np.float64) for r in (res_list if isinstance(res_list, (list, tuple)) else [res_list])]
    V = res_list[0].shape[-2]
    out = {'count': np.zeros(V, np.int64), 'nonfinite': np.zeros(V, np.int64), 'sum': np.zeros(V), 'mean': np.full(V, np.nan),
           'median': np.full(V, np.nan), 'mid': np.full((V, 2), np.nan)}
    for c in range(V):
        a = np.concatenate([r[..., c, :].reshape(-1) for r in res_list])
        keep = a[a >= 0] + 0.0                     # -0.0 counts as 0 and is returned as +0.0
        nan = bool(np.isnan(a).any())
        out['count'][c] = len(keep)
        out['nonfinite'][c] = int((~np.isfinite(a)).sum())
        out['sum'][c] = np.nan if nan else keep.sum()
        if len(keep):
            s = np.sort(keep)
            out['mid'][c] = s[(len(s) - 1) // 2], s[len(s) // 2]
            out['mean'][c] = np.nan if nan else keep.mean()
            out['median'][c] = np.nan if nan else np.median(keep)
    return out


def showgt_frame_ok(frame, joint_list):
    """The --showgt frame filter (:183-233): None when the frame has no GT field (the script exits), False when it has no
    bodies or a body lacks '-1' or a joint of joint_list."""
    first = list(frame.keys())[0]
    if len(frame[first]) != 4:
        return None
    for c in frame:
        if len(frame[c][3]) > len(frame[first][3]):
            first = c
    bodies = frame[first][3]
    if len(bodies) == 0:
        return False
    return all('-1' in b and all(str(j) in b for j in joint_list) for b in bodies)


def select_gt(poses, valid, n_persons, gt, used_joints):
    """The GT body of every person (:331-349): the first body with the smallest mean distance over used_joints to the MLP
    pose (strict <, below 1e10), -1 without one.  poses [F,Pcap,J,3] float32, valid [F,Pcap], gt: pack_ground_truth's
    arrays.  The distances are mpe_eval_batch's table (assignment.error_table).  -> [F,Pcap] int32."""
    poses = np.asarray(poses, np.float32)
    F, Pcap, J, _ = poses.shape
    used = np.zeros(J, bool)
    used[list(used_joints)] = True
    out = np.full((F, Pcap), -1, np.int32)
    for f in range(F):
        G = int(gt['n'][f])
        ps = [p for p in range(min(int(n_persons[f]), Pcap)) if valid[f, p]]
        if not G or not ps:
            continue
        table, _ = error_table(poses[f, ps], np.ones((len(ps), J), bool), gt['xyz'][f, :G], gt['joint'][f, :G], used)
        has = (gt['joint'][f, :G].astype(bool) & used[None]).any(axis=1)
        t = np.where(has[:, None], table, np.inf)
        best = np.argmin(t, axis=0)
        out[f, ps] = np.where(t[best, np.arange(len(ps))] < 10000000000., best, -1)
    return out


def gt_pose_tensor(gt, sel):
    """GT bodies as a pose tensor for the projection: (poses [F,Pcap,J,3] float32, flags [F,Pcap] uint8)."""
    F, Pcap = sel.shape
    idx = np.maximum(sel, 0)
    poses = np.asarray(gt['xyz'], np.float32)[np.arange(F)[:, None], idx]
    return np.ascontiguousarray(poses), (sel >= 0).astype(np.uint8)


def gt_joint_mask(joint_list):
    """The one joint the script books per (person, camera) in its GT row: its `if` sits outside its `for` (:382-390), so
    only the last key of the body's dict -- built in joint_list order (:223-226) -- is compared."""
    return 1 << int(list(joint_list)[-1])
