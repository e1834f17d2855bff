"""numpy statement of what mpe_body_refine_batch computes (csrc/skel_refine.hip): the body-level fit.  One cost per tracked
row -- the reprojection error of every joint over the cameras that saw it plus the deviation of every bone from the length
learned for its track -- minimised joint by joint, each joint by Levenberg-Marquardt steps of three unknowns with its
neighbours held.  The tests hold the kernel to `refine_sequence`, bit for bit.  include/mpe.h words the rule; the lines
below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing), in the header's order.

Rows.  Detections, ACTIVE joints, LIVE and CONSTRAINED bones and PROCESSED rows exactly as harness/skeleton.py has them
for the fit.  Every row that is not processed is copied through bit for bit.

Frame map.  frames[f] is the frame of the packed batch whose heads pose-frame f is observed in (None: f itself).  An entry
outside 0 .. pb.n_frames - 1: the frame's rows are copied through and every status of the frame is BAD_FRAME.

Observations.  Camera c observes active joint j of a processed row when harness/reprojection.py's `selection` counts
(f, p, c, j) on the heads of frame frames[f]; n_views = the number of such cameras.  An active joint whose start has
pc_2 <= 0 (or NaN) in an observing camera is BAD_START: it is held at its input and still anchors its bones.  A joint is
FREE when it is active, not BAD_START and has an observing camera or is an end of a constrained bone.

Colours.  Over j increasing, colour[j] = the least colour no lower-numbered joint that shares a bone with j holds.

Local cost of joint j at Y, neighbours at their working values: the left fold from 0.0 over the observing cameras in
increasing c of rho(e_c) (projection, e, rho and the weight w_c of harness/refine.py), then, with kappa = bone_weight > 0,
over the constrained bones incident to j in list order, N the other end: d_a = Y_a - N_a; s = (d_0*d_0 + d_1*d_1) +
d_2*d_2; l = sqrt(s); q = kappa*(l - L); C = C + q*q.

One update of a free joint.  A_kl, g_k from the observing cameras as in harness/refine.py, then per incident constrained
bone in list order with l > 0: n_a = d_a / l; m_a = kappa*n_a; A_kl = A_kl + m_k*m_l; g_k = g_k + m_k*q.  M = A +
lambda_j*diag(A), the LDL^T lines of harness/refine.py.  A pivot not > 0 or a delta not finite rejects; the trial Y +
delta is accepted only if pc_2 > 0 there in every observing camera and C_j(trial) < C_j(Y).  lambda_j starts at 1e-3 and
lives across sweeps: accepted max(lambda_j / 10, 1e-12), rejected lambda_j * 10.

Order.  For sweep = 1 .. sweeps, for colour = 0 .. n_colours - 1, every free joint of that colour takes one update; two
joints of one colour share no bone, so the order within a colour does not matter.  No early exit.

Outputs.  poses: a joint that accepted an update gets its working value rounded once to the pose type, everything else
keeps its bits.  status u8 [F,Pcap,J]: FREE, MOVED, BAD_START, ONE_VIEW (n_views == 1), BAD_FRAME; n_views u8 [F,Pcap,J];
both 0 in a row that is not processed (BAD_FRAME apart).  cost [F,Pcap,4] = the pixel part and the bone part of the row's
cost at the start, then at the end; -1.0 for a row that is not processed.  Pixel part: the fold from 0.0 over the active
joints in increasing j of the joint's camera fold; bone part: the fold from 0.0 over the constrained bones in list order of
q*q, 0.0 when bone_weight is 0.  Held joints count.  err [F,Pcap,2] and n_bones [F,Pcap] as the fit defines them.
"""
import numpy as np

from . import reprojection as R
from . import skeleton as S
from .refine import PAIRS, camera_constants64, huber_weight, lm_step3, project64, _rho

FREE, MOVED, BAD_START, ONE_VIEW, BAD_FRAME = 1, 2, 4, 8, 16
MAX_SWEEPS = 64
KEYS = ('poses', 'status', 'n_views', 'cost', 'err', 'n_bones')


def colours(bones, J):
    """-> colour [J] int: over j increasing, the least colour no lower-numbered joint that shares a bone with j holds"""
    near = [set() for _ in range(J)]
    for jp, jc in np.asarray(bones, np.int64).reshape(-1, 2):
        near[jp].add(int(jc))
        near[jc].add(int(jp))
    col = np.zeros(J, np.int64)
    for j in range(J):
        taken = {int(col[i]) for i in near[j] if i < j}
        k = 0
        while k in taken:
            k += 1
        col[j] = k
    return col


def incident(bones, J):
    """-> per joint the list of (bone, other end) in list order"""
    inc = [[] for _ in range(J)]
    for b, (jp, jc) in enumerate(np.asarray(bones, np.int64).reshape(-1, 2)):
        inc[jp].append((b, int(jc)))
        inc[jc].append((b, int(jp)))
    return inc


class _Heads:
    """The packed batch as `selection` reads it, its frames taken in the order of the frame map (a bad entry: no heads)."""

    def __init__(self, pb, frames):
        off = np.asarray(pb.frame_head_off).astype(np.int64)
        idx, counts = [], []
        for bf in frames:
            n = int(off[bf + 1] - off[bf]) if 0 <= bf < pb.n_frames else 0
            idx.append(np.arange(off[bf], off[bf] + n) if n else np.zeros(0, np.int64))
            counts.append(n)
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        self.J, self.n_heads = pb.J, len(idx)
        self.frame_head_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.joint_mask = np.asarray(pb.joint_mask)[idx]
        self.xy = np.asarray(pb.xy, np.float64).reshape(-1, pb.J, 2)[idx]
        self.vp = np.asarray(pb.vp, np.float32).reshape(-1, pb.J, 2)[idx]


def _bone(Y, N, kappa, L):
    """-> (d [3 arrays], l, q) of the bone from N to Y"""
    d = [Y[..., a] - N[..., a] for a in range(3)]
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    l = np.sqrt(s)
    return d, l, kappa * (l - L)


def refine_sequence(state, calib, pb, persons, n_persons, poses, flags, ids, mode, joint_mask, sweeps=8, bone_weight=300.0,
                    huber_px=0.0, threshold=0.5, frames=None):
    """state: harness/skeleton.py's (bones, len, tid_cap are read); pb: the packed batch (host arrays); persons
    [F,Pcap,V], n_persons [F], poses [F,Pcap,J,3], flags, ids [F,Pcap] of the pose frames; frames: int [F] or None.
    -> {'poses', 'status', 'n_views', 'cost', 'err', 'n_bones'}; the state is read only."""
    if not 1 <= int(sweeps) <= MAX_SWEEPS or not bone_weight >= 0.0 or not huber_px >= 0.0 or not threshold >= 0.0:
        raise ValueError('sweeps in 1..%d, bone_weight, huber_px and threshold >= 0' % MAX_SWEEPS)
    poses, flags, ids, persons = np.asarray(poses), np.asarray(flags), np.asarray(ids), np.asarray(persons)
    F, pcap, J = poses.shape[:3]
    if frames is None:
        if F != pb.n_frames:
            raise ValueError('without a frame map the poses have the frames of the batch')
        frames = np.arange(F)
    frames = np.asarray(frames).astype(np.int64)
    bones, table = state['bones'], state['len']
    kappa, huber = np.float64(bone_weight), float(huber_px)
    col, inc = colours(bones, J), incident(bones, J)
    out = poses.copy()
    status = np.zeros((F, pcap, J), np.uint8)
    n_views = np.zeros((F, pcap, J), np.uint8)
    cost = np.full((F, pcap, 4), -1.0)
    err = np.full((F, pcap, 2), -1.0)
    n_bones = np.zeros((F, pcap), np.uint8)
    bad_frame = (frames < 0) | (frames >= pb.n_frames)
    status[bad_frame] = BAD_FRAME

    # the processed rows, their active joints and their constrained bones
    rows, act, con, Ls = [], [], [], []
    for f, p, t, active in S._rows(poses, flags, n_persons, ids, mode, joint_mask):
        if t >= state['tid_cap'] or bad_frame[f]:
            continue
        c = np.array([bool(active[jp] and active[jc] and table[t, b] > 0 and np.isfinite(table[t, b])) for b, (jp, jc) in enumerate(bones)])
        if c.any():
            rows.append((f, p))
            act.append(active)
            con.append(c)
            Ls.append(table[t])
    result = {'poses': out, 'status': status, 'n_views': n_views, 'cost': cost, 'err': err, 'n_bones': n_bones}
    if not rows:
        return result
    fi, pi = (np.array(a) for a in zip(*rows))
    act, con, Ls = np.array(act), np.array(con), np.array(Ls, np.float64)
    n = len(rows)
    sel, xy = R.selection(_Heads(pb, frames), persons, n_persons, flags, joint_mask, threshold)
    obs = np.moveaxis(sel[fi, pi], 1, 2) & act[:, :, None]                    # [n, J, V]
    xy = np.moveaxis(xy[fi, pi], 1, 2)                                        # [n, J, V, 2]
    cams = list(zip(*camera_constants64(calib)))
    X = poses[fi, pi].astype(np.float64)                                      # the working poses [n, J, 3]
    views = obs.sum(axis=2)
    ends = np.zeros((n, J), bool)
    for b, (jp, jc) in enumerate(bones):
        ends[:, jp] |= con[:, b]
        ends[:, jc] |= con[:, b]

    def pixels(Y, o, z):
        """Y [..., 3], o [..., V], z [..., V, 2] -> (the camera fold, pc_2 > 0 in every observing camera)"""
        C = np.zeros(Y.shape[:-1])
        front = np.ones(Y.shape[:-1], bool)
        for c, (T, kd, K) in enumerate(cams):
            pr = project64(T, kd, K, Y[..., 0], Y[..., 1], Y[..., 2])
            rx = pr['px'] - z[..., c, 0]
            ry = pr['py'] - z[..., c, 1]
            C = np.where(o[..., c], C + _rho(np.sqrt(rx * rx + ry * ry), huber), C)
            front &= ~o[..., c] | (pr['pc2'] > 0.0)
        return C, front

    def row_cost():
        """-> (pixel part [n], bone part [n], worst |l - L| [n]) of the working poses"""
        Cj, _ = pixels(X, obs, xy)
        pix = np.zeros(n)
        for j in range(J):
            pix = np.where(act[:, j], pix + Cj[:, j], pix)
        bone, worst = np.zeros(n), np.zeros(n)
        for b, (jp, jc) in enumerate(bones):
            _, l, q = _bone(X[:, jc], X[:, jp], kappa, Ls[:, b])
            if kappa > 0.0:
                bone = np.where(con[:, b], bone + q * q, bone)
            v = np.abs(l - Ls[:, b])
            worst = np.where(con[:, b] & (v > worst), v, worst)
        return pix, bone, worst

    with np.errstate(all='ignore'):
        _, front = pixels(X, obs, xy)
        bad = act & ~front
        free = act & ~bad & ((views >= 1) | ends)
        moved = np.zeros((n, J), bool)
        lam = np.full((n, J), 1e-3)
        pix0, bone0, worst0 = row_cost()
        groups = [np.flatnonzero(col == k) for k in range(int(col.max()) + 1)]
        depth = max(len(i) for i in inc)
        for _ in range(int(sweeps)):
            for js in groups:
                Y, o, z, fr = X[:, js], obs[:, js], xy[:, js], free[:, js]
                m = len(js)
                A = {kl: np.zeros((n, m)) for kl in PAIRS}
                g = [np.zeros((n, m)) for _ in range(3)]
                C = np.zeros((n, m))
                for c, (T, kd, K) in enumerate(cams):
                    pr = project64(T, kd, K, Y[..., 0], Y[..., 1], Y[..., 2], jacobian=True)
                    rx = pr['px'] - z[..., c, 0]
                    ry = pr['py'] - z[..., c, 1]
                    e = np.sqrt(rx * rx + ry * ry)
                    w = huber_weight(e, huber)
                    jx, jy = pr['jx'], pr['jy']
                    oc = o[..., c]
                    C = np.where(oc, C + _rho(e, huber), C)
                    for (k, l) in A:
                        A[k, l] = np.where(oc, A[k, l] + w * (jx[k] * jx[l] + jy[k] * jy[l]), A[k, l])
                    for k in range(3):
                        g[k] = np.where(oc, g[k] + w * (jx[k] * rx + jy[k] * ry), g[k])
                # the incident bones, the i-th of every joint of the colour side by side
                held = []
                for i in range(depth if kappa > 0.0 else 0):
                    has = np.array([i < len(inc[j]) for j in js])
                    b = np.array([inc[j][i][0] if i < len(inc[j]) else 0 for j in js])
                    other = np.array([inc[j][i][1] if i < len(inc[j]) else 0 for j in js])
                    on = con[:, b] & has[None, :]
                    N, L = X[:, other], Ls[:, b]
                    held.append((on, N, L))
                    d, l, q = _bone(Y, N, kappa, L)
                    C = np.where(on, C + q * q, C)
                    on = on & (l > 0.0)
                    mk = [kappa * (d[a] / l) for a in range(3)]
                    for (k, l_) in A:
                        A[k, l_] = np.where(on, A[k, l_] + mk[k] * mk[l_], A[k, l_])
                    for k in range(3):
                        g[k] = np.where(on, g[k] + mk[k] * q, g[k])
                lm = lam[:, js]
                delta, ok = lm_step3(A, g, lm)
                ok = fr & ok
                trial = Y + delta
                Ct, front = pixels(trial, o, z)
                for on, N, L in held:
                    _, _, q = _bone(trial, N, kappa, L)
                    Ct = np.where(on, Ct + q * q, Ct)
                accept = ok & front & (Ct < C)
                X[:, js] = np.where(accept[..., None], trial, Y)
                lam[:, js] = np.where(accept, np.maximum(lm / 10.0, 1e-12), np.where(fr, lm * 10.0, lm))
                moved[:, js] |= accept
        pix1, bone1, worst1 = row_cost()
    st = np.where(free, FREE, 0) | np.where(moved, MOVED, 0) | np.where(bad, BAD_START, 0) | np.where(act & (views == 1), ONE_VIEW, 0)
    status[fi, pi] = st.astype(np.uint8)
    n_views[fi, pi] = views.astype(np.uint8)
    cost[fi, pi] = np.stack([pix0, bone0, pix1, bone1], axis=1)
    err[fi, pi] = np.stack([worst0, worst1], axis=1)
    n_bones[fi, pi] = con.sum(axis=1).astype(np.uint8)
    out[fi, pi] = np.where(moved[..., None], X.astype(poses.dtype), poses[fi, pi])
    return result


class RefineSummary:
    """What the body fit did to a sequence, from the inputs and outputs of its chunks."""

    def __init__(self):
        self.rows = self.bones = self.free = self.one_view_moved = self.joints = 0
        self.pix0 = self.pix1 = self.err0 = self.err1 = self.moved = 0.0

    def add(self, poses_in, out):
        """rows: the processed rows; bones: their constrained bones; free: their free joints; one_view_moved: the joints
        one camera saw that moved; the pixel cost is the rows' pixel part, the length error the rows' worst bone."""
        p0, p1 = np.asarray(poses_in, np.float64), np.asarray(out['poses'], np.float64)
        st, cost, err, nb = (np.asarray(out[k]) for k in ('status', 'cost', 'err', 'n_bones'))
        sel = nb > 0
        self.rows += int(sel.sum())
        self.bones += int(nb.sum())
        self.free += int(((st & FREE) != 0).sum())
        self.one_view_moved += int(((st & (ONE_VIEW | MOVED)) == (ONE_VIEW | MOVED)).sum())
        for k, name in ((0, 'pix0'), (2, 'pix1')):
            v = cost[..., k][sel]
            setattr(self, name, getattr(self, name) + float(v[np.isfinite(v)].sum()))
        for k, name in ((0, 'err0'), (1, 'err1')):
            v = err[..., k][sel]
            setattr(self, name, getattr(self, name) + float(v[np.isfinite(v)].sum()))
        d = p1 - p0
        changed = ((st & MOVED) != 0) & np.isfinite(d).all(axis=3) & (d != 0).any(axis=3)
        self.joints += int(changed.sum())
        self.moved += float(np.sqrt((d[changed] ** 2).sum(axis=1)).sum())

    def result(self, lengths=None):
        """lengths: Skeleton.lengths()'s dict or a state of harness/skeleton.py -> {'tracks' (ids with a length), 'rows',
        'bones', 'free', 'one_view_moved', 'pixel_cost' [before, after] (mean over the rows, px^2), 'err_mean_mm' [before,
        after] (over the rows' worst bone), 'mean_move_mm' (over the joints that moved)}"""
        tracks = 0
        if lengths is not None:
            table = np.asarray(lengths['len'])
            tracks = int(((table > 0) & np.isfinite(table)).any(axis=1).sum())
        n = max(self.rows, 1)
        return {'tracks': tracks, 'rows': self.rows, 'bones': self.bones, 'free': self.free, 'one_view_moved': self.one_view_moved,
                'pixel_cost': [self.pix0 / n, self.pix1 / n], 'err_mean_mm': [1000.0 * self.err0 / n, 1000.0 * self.err1 / n],
                'mean_move_mm': 1000.0 * self.moved / self.joints if self.joints else 0.0}


def report_line(sweeps, weight, huber, r):
    """the harness's line"""
    return ('Body fit (%d sweeps, %g px/m, Huber %g px): %d tracks, %d rows, %d bones, %d free joints, %d one-view joints moved, '
            'mean pixel cost %.6g -> %.6g px^2, length error %.3f -> %.3f mm, mean move %.3f mm'
            % (sweeps, weight, huber, r['tracks'], r['rows'], r['bones'], r['free'], r['one_view_moved'], r['pixel_cost'][0],
               r['pixel_cost'][1], r['err_mean_mm'][0], r['err_mean_mm'][1], r['mean_move_mm']))
