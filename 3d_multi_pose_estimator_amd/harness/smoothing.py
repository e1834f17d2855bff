"""numpy statement of what mpe_smooth_batch computes (csrc/smooth.hip): tracked poses filtered over time.  A causal,
windowed, weighted line fit per (track, joint, axis) over the RAW poses of the current frame and the W frames before it.
There is no feedback: every output is a function of W + 1 frames of input.  It follows the track ids (mpe_track_batch,
harness/tracking.py), not person rows.  The tests hold the kernel to `smooth_sequence`, bit for bit.

The rule -- the contract of the device path:

Detections and presence.  As in mpe_track_batch.  Row p of frame f is a detection when p < n_persons[f], ids[f, p] >= 0
and, in mode 'mlp', flags[f, p] != 0.  Mode 'mlp': float32 poses, every joint of a detection is present.  Mode 'tri':
float64 poses, joint j is present when flags[f, p, j] != 0.  Only joints of joint_mask are processed.

Samples of joint j of a detection with id t.  For age a = 0 .. W the sample of age a exists when frame f - a exists in
the sequence (frames count over the whole sequence, the state supplies those before the call), that frame has a
detection with id t (the lowest such row; for a = 0 the row itself, which it is when ids are unique within a frame),
joint j is present in that row by the INPUT flags, and its three stored coordinates are finite.  Value: the stored input
coordinate widened to float64.  Weight: w_0 = 1, w_a = w_(a-1) * decay, every product rounded on its own.

Sums.  n = the number of samples, r = the youngest one.  Per axis, y_a = x_a - x_r, u_a = float(a), c_a = w_a * u_a;
left-fold sums from 0.0 over the samples in increasing a, every product and sum rounded on its own:
S0 += w_a; S1 += c_a; S2 += c_a * u_a; T0 += w_a * y_a; T1 += c_a * y_a.

Fit.  D = S0*S2 - S1*S1; alpha = x_r + (S2*T0 - S1*T1) / D; beta = (S0*T1 - S1*T0) / D.  A fit exists when n >= 2, D > 0
and alpha and beta are finite on all three axes.

Joint present now (the sample of age 0 exists): with a fit, poses = alpha rounded once to the pose type and vel = -beta
(metres per frame); without one the input bits and vel = 0.  A joint that is present but not finite now is copied
likewise.  flags: 1 for a present joint in mode 'tri', the input flag in mode 'mlp'.

Joint missing now (mode 'tri' only): with fill and a fit, poses = alpha, vel = -beta, flags = FILLED (2); otherwise the
input bits, flags = 0, vel = 0.

n_samples = n for every processed joint.  Rows that are no detection and joints outside joint_mask are copied through
bit for bit with vel = 0, n_samples = 0 and the input flag.  W = 0 copies everything.

State.  The raw input of the last W frames (ids, presence, coordinates widened to float64): a sequence fed in any
chunking gives the same bits.
"""
import numpy as np

FILLED = 2
MAX_WINDOW = 15


def new_state():
    return {'frames': []}


def _frame(poses_f, flags_f, n, ids_f, mode):
    """-> (ids [pcap] with -1 where the row is no detection, present [pcap,J], coordinates [pcap,J,3] float64)"""
    pcap, J = poses_f.shape[:2]
    det = (np.arange(pcap) < max(0, min(int(n), pcap))) & (ids_f >= 0)
    if mode == 'mlp':
        det &= flags_f != 0
        present = np.repeat(det[:, None], J, axis=1)
    else:
        present = (flags_f != 0) & det[:, None]
    return np.where(det, ids_f, -1).astype(np.int32), present, poses_f.astype(np.float64)


def smooth_sequence(poses, flags, n_persons, ids, mode, joint_mask, window, decay=0.8, fill=False, state=None):
    """poses [B,Pcap,J,3], flags, n_persons [B], ids [B,Pcap] (the tracker's) -> {'poses' (the type of poses), 'flags'
    (the shape of flags), 'vel' [B,Pcap,J,3] float64, 'n_samples' [B,Pcap,J] uint8, 'state'}.  `state` is a former
    call's (it is not modified); None starts a sequence."""
    if mode not in ('mlp', 'tri'):
        raise ValueError('mode must be mlp or tri')
    W, lam = int(window), np.float64(decay)
    if not 0 <= W <= MAX_WINDOW or not 0.25 <= lam <= 1.0:
        raise ValueError('window is within 0 .. %d and decay within [0.25, 1]' % MAX_WINDOW)
    poses, flags, ids = np.asarray(poses), np.asarray(flags), np.asarray(ids)
    B, pcap, J = poses.shape[:3]
    tri = mode == 'tri'
    in_mask = np.array([(int(joint_mask) >> j) & 1 for j in range(J)], bool)
    history = list((new_state() if state is None else state)['frames'])
    out_p, out_f = poses.copy(), flags.copy()
    vel = np.zeros((B, pcap, J, 3))
    n_samples = np.zeros((B, pcap, J), np.uint8)
    for f in range(B):
        cur = _frame(poses[f], flags[f], n_persons[f], ids[f], mode)
        frames = history + [cur]                             # frames[-1 - a] is the frame of age a
        history = frames[-W:] if W else []
        t, present = cur[0], cur[1]
        work = (t >= 0)[:, None] & in_mask[None]             # [pcap,J] the joints that are processed
        S0, S1, S2 = np.zeros((pcap, J)), np.zeros((pcap, J)), np.zeros((pcap, J))
        T0, T1, xr = np.zeros((pcap, J, 3)), np.zeros((pcap, J, 3)), np.zeros((pcap, J, 3))
        n = np.zeros((pcap, J), np.int64)
        now = np.zeros((pcap, J), bool)
        w = np.float64(1.0)
        with np.errstate(all='ignore'):
            for a in range(min(W, len(frames) - 1) + 1):
                if a > 0:
                    w = w * lam
                ids_a, present_a, x_a = frames[-1 - a]
                if a == 0:
                    src, found = np.arange(pcap), t >= 0
                else:
                    eq = (ids_a[None, :] == t[:, None]) & (t >= 0)[:, None]
                    src, found = np.argmax(eq, axis=1), eq.any(axis=1)          # the lowest row with the id
                x = x_a[src]                                                     # [pcap,J,3]
                m = work & found[:, None] & present_a[src] & np.isfinite(x).all(axis=2)
                first = m & (n == 0)
                xr = np.where(first[..., None], x, xr)
                now |= first & (a == 0)
                n += m
                u = np.float64(a)
                c = w * u
                S0 = np.where(m, S0 + w, S0)
                S1 = np.where(m, S1 + c, S1)
                S2 = np.where(m, S2 + c * u, S2)
                y = x - xr
                T0 = np.where(m[..., None], T0 + w * y, T0)
                T1 = np.where(m[..., None], T1 + c * y, T1)
            D = S0 * S2 - S1 * S1
            Dx = D[..., None]
            alpha = xr + (S2[..., None] * T0 - S1[..., None] * T1) / Dx
            beta = (S0[..., None] * T1 - S1[..., None] * T0) / Dx
            fit = (n >= 2) & (D > 0) & np.isfinite(alpha).all(axis=2) & np.isfinite(beta).all(axis=2)
            take = work & fit & (now | (~present & bool(fill)))
            out_p[f] = np.where(take[..., None], alpha.astype(poses.dtype), poses[f])
            vel[f] = np.where(take[..., None], -beta, 0.0)
        n_samples[f] = np.where(work, n, 0)
        if tri:
            out_f[f] = np.where(work, np.where(present, 1, np.where(take, FILLED, 0)), flags[f])
    return {'poses': out_p, 'flags': out_f, 'vel': vel, 'n_samples': n_samples, 'state': {'frames': history}}


class SmoothSummary:
    """What smoothing did to a sequence, from the inputs and outputs of its chunks (mode 'tri': per-joint flags)."""

    def __init__(self, mode):
        self.tri = mode == 'tri'
        self.fitted = self.filled = 0
        self.moved_mm = 0.0

    def add(self, poses_in, flags_in, out):
        """fitted: the joints present now that have two samples or more (where no fit exists for them -- a non-finite
        result -- they keep the input and add no displacement); filled: the joints with the flag FILLED."""
        p0, p1, ns = np.asarray(poses_in, np.float64), np.asarray(out['poses'], np.float64), np.asarray(out['n_samples'])
        fin = np.asarray(flags_in) != 0
        present = fin if self.tri else np.repeat(fin[..., None], ns.shape[2], axis=2)
        sel = present & (ns >= 2)
        self.fitted += int(sel.sum())
        if self.tri:
            self.filled += int((np.asarray(out['flags']) == FILLED).sum())
        d = (p1 - p0)[sel]
        d = d[np.isfinite(d).all(axis=1)]
        self.moved_mm += float(np.sqrt((d * d).sum(axis=1)).sum()) * 1000.0

    def result(self):
        """-> {'fitted', 'filled', 'mean_move_mm' (over the fitted joints)}"""
        return {'fitted': self.fitted, 'filled': self.filled, 'mean_move_mm': self.moved_mm / self.fitted if self.fitted else 0.0}
