"""The pose document mpe_json_write_poses writes on the device, stated with numpy and json.dumps, and its reader.

One line per frame, in frame order, each exactly json.dumps(obj) + "\\n" (default separators) for

    obj  = {"frame": frame_start + f, "ids": [id of each written row], "bodies": [body, ...]}
    body = {"<j>": [x, y, z], ...}            j ascending

"ids" is there exactly when ids are given.  Row p of frame f is looked at when p < min(max(n_persons[f], 0), pcap); its
written joints are the flagged ones (a row flag stands for every joint) within joint_mask whose three coordinates
(double)x * scale are all finite; a flagged joint of the mask that is dropped for a coordinate that is not finite sets
MPE_WRITE_NONFINITE in the frame's status; a row without a written joint appears in neither list.  A line is a function
of its own frame alone, so the lines of any chunking of a recording, joined, are the lines of the recording.  The body
grammar is the one mpe_json_parse_bodies_device reads (scale 100: the centimetres of bodies_3D).
"""
import json

import numpy as np

MPE_WRITE_NONFINITE, MPE_WRITE_CAPACITY = 1, 2


def write_lines(poses, flags, n_persons, ids=None, frame_start=0, scale=1.0, joint_mask=None, details=False):
    """poses [B,pcap,J,3] f32 or f64; flags [B,pcap] or [B,pcap,J]; n_persons [B]; ids [B,pcap] or None -> the document
    (bytes); with details also {'frame_off' [B+1] i64, 'bodies_extent' [B,2] u32 (the "bodies" list with its brackets,
    offsets into the document), 'rows_written' [B] i32, 'status' [B] i32, 'joints_written', 'joints_dropped'}."""
    poses = np.asarray(poses)
    flags = np.asarray(flags)
    B, pcap, J = poses.shape[:3]
    mask = (1 << J) - 1 if joint_mask is None else int(joint_mask)
    with np.errstate(over='ignore', invalid='ignore'):
        scaled = poses.astype(np.float64) * np.float64(scale)
    out = []
    off = np.zeros(B + 1, dtype=np.int64)
    extent = np.zeros((B, 2), dtype=np.uint32)
    rows = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    written = dropped = 0
    for f in range(B):
        bodies, row_ids = [], []
        for p in range(min(max(int(n_persons[f]), 0), pcap)):
            body = {}
            for j in range(J):
                flagged = flags[f, p, j] if flags.ndim == 3 else flags[f, p]
                if not flagged or not (mask >> j) & 1:
                    continue
                xyz = scaled[f, p, j]
                if not np.all(np.isfinite(xyz)):
                    status[f] |= MPE_WRITE_NONFINITE
                    dropped += 1
                    continue
                body[str(j)] = [float(xyz[0]), float(xyz[1]), float(xyz[2])]
            if body:
                bodies.append(body)
                written += len(body)
                if ids is not None:
                    row_ids.append(int(ids[f, p]))
        obj = {'frame': int(frame_start) + f}
        if ids is not None:
            obj['ids'] = row_ids
        obj['bodies'] = bodies
        line = (json.dumps(obj) + '\n').encode('ascii')
        head = dict(obj)
        del head['bodies']
        begin = len(json.dumps(head)) - 1 + len(', "bodies": ')
        extent[f] = (off[f] + begin, off[f] + len(line) - 2)
        assert line[begin:len(line) - 2] == json.dumps(bodies).encode('ascii')
        rows[f] = len(bodies)
        off[f + 1] = off[f] + len(line)
        out.append(line)
    data = b''.join(out)
    if not details:
        return data
    return data, {'frame_off': off, 'bodies_extent': extent, 'rows_written': rows, 'status': status,
                  'joints_written': written, 'joints_dropped': dropped}


def read_lines(data, n_joints=None, pcap=None):
    """A written document (bytes or str) -> (frame [B] i64, ids [B,pcap] i32 or None, poses [B,pcap,J,3] f64, joint
    flags [B,pcap,J] u8), the bodies of a line in rows 0 .. of their frame in list order; rows and joints that are not
    there are 0 (ids: -1).  J and pcap default to the smallest that hold the document.  The coordinates are the written
    ones (after the scale), bit for bit: json.loads reads a float as float() does."""
    if isinstance(data, bytes):
        data = data.decode('ascii')
    objs = [json.loads(line) for line in data.split('\n') if line]
    B = len(objs)
    if pcap is None:
        pcap = max([len(o['bodies']) for o in objs] + [1])
    if n_joints is None:
        n_joints = max([int(k) + 1 for o in objs for b in o['bodies'] for k in b] + [1])
    with_ids = B > 0 and 'ids' in objs[0]
    frame = np.zeros(B, dtype=np.int64)
    ids = np.full((B, pcap), -1, dtype=np.int32) if with_ids else None
    poses = np.zeros((B, pcap, n_joints, 3), dtype=np.float64)
    flags = np.zeros((B, pcap, n_joints), dtype=np.uint8)
    for f, o in enumerate(objs):
        frame[f] = o['frame']
        if with_ids and len(o['ids']) != len(o['bodies']):
            raise ValueError('line %d: %d ids for %d bodies' % (f, len(o['ids']), len(o['bodies'])))
        for r, body in enumerate(o['bodies']):
            if with_ids:
                ids[f, r] = o['ids'][r]
            for k, xyz in body.items():
                poses[f, r, int(k)] = xyz
                flags[f, r, int(k)] = 1
    return frame, ids, poses, flags
