"""numpy statement of what mpe_json_parse_bodies_device and mpe_gt_from_bodies compute (csrc/jsonparse.hip, csrc/gt.hip):
the ground-truth side of the metrics scripts, from the frames as json.load gives them.  The GPU tests hold the kernels to
this module bit for bit; the host tests hold this module to harness.common.pack_ground_truth (torch on the CPU) and to
harness.partition.pack_bodies.

Bodies.  frame[cam][3] of EVERY camera key of a frame is one entry, in the frame's key order; an entry's cam is the
camera's position in the configured list, -1 outside it.  The bodies of a frame get rows: those of the configured cameras
first, in (entry order, list order) -- what pack_bodies packs -- and those of the other cameras behind them in the same
order.  Key slots are fixed: joint key "j" (j in 0..30, written without a leading zero) is slot j and "-1" is slot 31; any
other key, a value that is not three plain numbers, or a non-finite number is outside the device's language (Unsupported:
status bit 0); more bodies in a frame than rows is status bit 1.

Selection (test/metrics_from_model.py:126-138).  The frame's first entry, replaced by a later one only when it holds
strictly more bodies; every key of the frame takes part, configured or not.  No bodies: the frame is skipped.

Ground truth (:139-174).  Per body of the selected entry and joint j of joint_list with the key present:
  g_k = float32(float64(v_k) / 100.)  ;  x = (g_0, g_1, g_2, 1)
  y = T_d x ; w = T_i1 y, every row as acc = T[i][0] * x_0 ; acc = fma(T[i][k], x_k, acc) for k = 1, 2, 3 in fp32
which is what torch's fp32 matmul gives on the CPU for these shapes (test_groundtruth_host.py holds the two together).
fma32 below is exact: the product and the sum are taken as fractions and rounded once.
"""
from fractions import Fraction

import numpy as np

KEY_SLOTS = 32
M1_SLOT = 31
STATUS_HOST, STATUS_CAPACITY = 1, 2


class Unsupported(ValueError):
    """The document holds something the device parser leaves to the host."""


def slot_of(key):
    """Fixed slot of a body's key, or Unsupported."""
    if key == '-1':
        return M1_SLOT
    if key.isascii() and key.isdigit() and len(key) <= 2 and (len(key) == 1 or key[0] != '0') and int(key) < M1_SLOT:
        return int(key)
    raise Unsupported('key %r' % (key,))


def parse_bodies(frames, cameras, scap=None):
    """The arrays of mpe_json_parse_bodies_device for frames as json.load gives them -> dict: xyz [B,scap,32,3] f64, mask
    [B,scap] u32, nkeys [B,scap] i32, order [B,scap,32] u8, m1 [B,scap] u8, n [B] i32, entry_count [E] i32, body_cam
    [B,scap] i32 (-1: a camera that is not configured, or an unused row), entry_cam [E] i32, frame_entry_off [B+1] i32,
    status.  scap defaults to the largest body count of a frame (at least 1)."""
    cameras = list(cameras)
    B = len(frames)
    entry_cam, entry_count, feo, rows = [], [], [0], []
    for f in frames:
        conf, other = [], []
        for cam in f:
            c = cameras.index(cam) if cam in cameras else -1
            bodies = f[cam][3]
            if not isinstance(bodies, list):
                raise Unsupported('bodies of %r are not a list' % (cam,))
            entry_cam.append(c)
            entry_count.append(len(bodies))
            (conf if c >= 0 else other).extend((c, b) for b in bodies)
        feo.append(len(entry_cam))
        rows.append((len(conf), conf + other))
    if scap is None:
        scap = max([1] + [len(r) for _, r in rows])
    out = {'xyz': np.zeros((B, scap, KEY_SLOTS, 3), np.float64), 'mask': np.zeros((B, scap), np.uint32),
           'nkeys': np.zeros((B, scap), np.int32), 'order': np.zeros((B, scap, KEY_SLOTS), np.uint8), 'm1': np.zeros((B, scap), np.uint8),
           'n': np.zeros(B, np.int32), 'entry_count': np.array(entry_count, np.int32).reshape(-1),
           'body_cam': np.full((B, scap), -1, np.int32), 'entry_cam': np.array(entry_cam, np.int32).reshape(-1),
           'frame_entry_off': np.array(feo, np.int32), 'status': 0}
    for f, (n_conf, bodies) in enumerate(rows):
        out['n'][f] = min(n_conf, scap)
        if len(bodies) > scap:
            out['status'] |= STATUS_CAPACITY
        for s, (c, body) in enumerate(bodies[:scap]):
            if not isinstance(body, dict):
                raise Unsupported('a body is not a dict')
            for i, (k, v) in enumerate(body.items()):
                slot = slot_of(k)
                if (not isinstance(v, list) or len(v) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in v)
                        or not all(np.isfinite(float(x)) for x in v)):
                    raise Unsupported('value of key %r' % (k,))
                out['xyz'][f, s, slot] = [float(x) for x in v]
                out['mask'][f, s] |= np.uint32(1 << slot)
                out['order'][f, s, i] = slot
            out['nkeys'][f, s] = len(body)
            out['m1'][f, s] = '-1' in body
            out['body_cam'][f, s] = c
    return out


def select_entry(counts):
    """Index of the selected entry among a frame's body counts (the first, replaced only by a strictly greater one), or
    None when the frame has no bodies (skipped)."""
    sel = None
    for i, c in enumerate(counts):
        if sel is None or c > counts[sel]:
            sel = i
    return None if sel is None or counts[sel] == 0 else sel


def entry_row(entry_cam, entry_count, i):
    """First row of entry i of a frame: configured entries first, the others behind them, each group in entry order."""
    conf = entry_cam[i] >= 0
    return int(sum(n for e, (c, n) in enumerate(zip(entry_cam, entry_count)) if ((c >= 0 and e < i) if conf else (c >= 0 or e < i))))


def _round32(fr):
    """A non-zero fraction -> the nearest float32, ties to even, rounded once."""
    d = float(fr)                       # correctly rounded to float64
    f = np.float32(d)
    if Fraction(d) == fr or Fraction(float(f)) == Fraction(d):
        return f                        # one rounding took place
    # d was rounded already: if it sits exactly halfway between two float32 the second rounding may go the wrong way
    other = np.nextafter(f, np.float32(np.inf) if d > float(f) else np.float32(-np.inf))
    mid = (Fraction(float(f)) + Fraction(float(other))) / 2
    if Fraction(d) != mid:
        return f
    return f if (fr < mid) == (float(f) < float(other)) else other


def fma32(a, b, c):
    """float32 fma(a, b, c), exact."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if fr == 0:
        if a != 0 and b != 0:           # an exact cancellation gives +0
            return np.float32(0.0)
        return np.float32(np.float32(a * b) + c)      # (+-0) + c: the sign rules of the addition
    return _round32(fr)


def row4(T, x):
    acc = np.float32(np.float32(T[0]) * np.float32(x[0]))
    for k in (1, 2, 3):
        acc = fma32(T[k], x[k], acc)
    return acc


def to_world(v, T_d, T_i1):
    """One joint: three float64 centimetre coordinates -> (3,) float32 world metres."""
    g = [np.float32(np.float64(x) / 100.) for x in v] + [np.float32(1.0)]
    y = [row4(T_d[i], g) for i in range(4)]
    return np.array([row4(T_i1[i], y) for i in range(3)], np.float32)


def gt_from_bodies(parsed, T_d_list, file_of_frame, T_i1, J, gcap=None):
    """mpe_gt_from_bodies on parse_bodies' arrays -> pack_ground_truth's dict ('xyz' [B,gcap,J,3] f32, 'joint' [B,gcap,J]
    u8, 'valid' [B,gcap] u8, 'n' [B] i32); gcap defaults to the rows per frame."""
    B, scap = parsed['mask'].shape
    gcap = scap if gcap is None else int(gcap)
    T_i1 = np.asarray(T_i1, np.float32).reshape(4, 4)
    out = {'xyz': np.zeros((B, gcap, J, 3), np.float32), 'joint': np.zeros((B, gcap, J), np.uint8),
           'valid': np.zeros((B, gcap), np.uint8), 'n': np.zeros(B, np.int32)}
    feo = parsed['frame_entry_off']
    for f in range(B):
        cams, counts = parsed['entry_cam'][feo[f]:feo[f + 1]], [int(c) for c in parsed['entry_count'][feo[f]:feo[f + 1]]]
        sel = select_entry(counts)
        if sel is None:
            continue
        base = entry_row(cams, counts, sel)
        n = max(0, min(counts[sel], scap - base, gcap))
        out['n'][f] = n
        T_d = np.asarray(T_d_list[int(file_of_frame[f])], np.float32).reshape(4, 4)
        for g in range(n):
            r = base + g
            out['valid'][f, g] = parsed['m1'][f, r]
            for j in range(J):
                if (int(parsed['mask'][f, r]) >> j) & 1:
                    out['joint'][f, g, j] = 1
                    out['xyz'][f, g, j] = to_world(parsed['xyz'][f, r, j], T_d, T_i1)
    return out
