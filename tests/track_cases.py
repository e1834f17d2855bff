"""Sequences for the tracking tests (test_track_host.py: harness/tracking.py against written-out ids; test_gpu_track.py:
mpe_track_batch against the same ids and against harness/tracking.py).  Not a test module."""
import numpy as np

J = 18
USED = [0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]          # parameters.used_joints
SHAPE = np.stack([np.zeros(J), 0.0625 * np.arange(J), np.zeros(J)], axis=1)      # a person: joints up the y axis
CHUNKS = (1, 1, 5, 16, 14)
# a dropout across every border of CHUNKS (frames 1, 2, 7, 23), for a tracker with max_gap >= 2
AWAY = {1: {1}, 0: {6, 7, 22, 23}}


def person(x, y=0.0, z=0.0):
    return SHAPE + np.array([x, y, z])


class Seq:
    """poses / flags / n_persons of a hand-made sequence.  frames: per frame a list of rows, each None (a row below
    n_persons that is no detection), a pose [J,3], or (pose, joints present) in mode 'tri'."""

    def __init__(self, mode, frames, pcap=4):
        self.mode = mode
        B = len(frames)
        self.poses = np.zeros((B, pcap, J, 3), np.float64 if mode == 'tri' else np.float32)
        self.flags = np.zeros((B, pcap, J) if mode == 'tri' else (B, pcap), np.uint8)
        self.n_persons = np.array([len(f) for f in frames], np.int32)
        for f, rows in enumerate(frames):
            for p, row in enumerate(rows):
                if row is None:
                    continue
                pose, joints = row if isinstance(row, tuple) else (row, range(J))
                self.poses[f, p] = pose
                if mode == 'tri':
                    self.flags[f, p, list(joints)] = 1
                else:
                    self.flags[f, p] = 1


def hand_made():
    """-> {name: (Seq, max_gap, gate, expected ids [B,pcap])}; rows past the written ones are -1."""
    A = lambda t: person(0.02 * t)                       # walks 2 cm per frame
    Bp = lambda t: person(2.0 - 0.02 * t)
    far = person(5.0)
    cases = {}
    cases['swap_rows'] = (Seq('mlp', [[A(t), Bp(t)] if t % 2 == 0 else [Bp(t), A(t)] for t in range(6)]), 2, 0.5,
                          [[0, 1], [1, 0], [0, 1], [1, 0], [0, 1], [1, 0]])
    # costs of frame 1 against (A at 0, B at 0.3): row 0 at 0.2 -> 0.2 / 0.1, row 1 at 0.45 -> 0.45 / 0.15.  The least cost
    # (row 0, B) goes first, row 1 is left with A at 0.45 < gate; the assignment of least total cost is the other one
    cases['greedy_crossing'] = (Seq('mlp', [[person(0.0), person(0.3)], [person(0.2), person(0.45)]]), 2, 0.5, [[0, 1], [1, 0]])
    # max_gap 2: A away for 2 frames keeps its id (a link over 3 frames), away for 3 frames comes back as a new track
    cases['gap_limit'] = (Seq('mlp', [[A(0), far], [far], [far], [far, A(3)], [far], [far], [far], [A(7), far]]), 2, 0.5,
                          [[0, 1], [1], [1], [1, 0], [1], [1], [1], [2, 1]])
    # every used joint 0.5 away (0.25 -> 0.75, exact in float32): the cost is 0.5 == gate, no link; 0.4375 links
    cases['cost_equals_gate_mlp'] = (Seq('mlp', [[person(0.25), person(3.0)], [person(0.75), person(3.4375)]]), 0, 0.5, [[0, 1], [2, 1]])
    cases['cost_equals_gate_tri'] = (Seq('tri', [[(person(0.25), [0]), (person(3.0), [0])], [(person(0.75), [0]), (person(3.4375), [0])]]), 0, 0.5,
                                     [[0, 1], [2, 1]])
    # equal poses: all four costs are equal, the lowest row takes the lowest column
    cases['duplicates'] = (Seq('mlp', [[person(1.0), person(1.0)], [far, person(1.0), person(1.0)]]), 1, 0.5, [[0, 1], [2, 0, 1]])
    cases['empty_frames'] = (Seq('mlp', [[A(0)], [], [A(2)], [], [], [A(5)]]), 1, 0.5, [[0], [], [0], [], [], [1]])
    # births: by frame, then by row; the row without a flag takes no id
    cases['birth_order'] = (Seq('mlp', [[A(0), None, Bp(0)], [far, A(1), Bp(1)], [A(2), person(8.0), far, person(-4.0)]]), 1, 0.5,
                            [[0, -1, 1], [2, 0, 1], [0, 3, 2, 4]])
    # joints 1-4 are not used: a person seen only there is no detection and takes no id
    cases['no_used_joint'] = (Seq('tri', [[(A(0), [1, 2, 3, 4]), (far, range(J))], [(A(1), range(J)), (far, range(J))]]), 1, 0.5,
                              [[-1, 0], [1, 0]])
    cases['no_common_joint'] = (Seq('tri', [[(A(0), [0, 5]), (far, range(J))], [(A(0), [6, 7]), (far, [0, 1])]]), 1, 0.5, [[0, 1], [2, 1]])
    out = {}
    for name, (seq, max_gap, gate, ids) in cases.items():
        want = np.full(seq.n_persons.shape + (seq.poses.shape[1],), -1, np.int32)
        for f, row in enumerate(ids):
            want[f, :len(row)] = row
        out[name] = (seq, max_gap, gate, want)
    return out


def random_sequence(seed, tri, B=40, pcap=6, away=None):
    """B frames of up to `pcap` people on random walks of 2 cm per frame: four regulars with 15 % dropouts, rows permuted
    per frame, now and then a duplicated pose or a row without a flag, every 9th frame empty, every 13th full; in mode
    'tri' 10 % of the joints missing.  away: {person: frames in which nobody sees them} (those frames and the ones after
    them are never the empty ones).  -> (poses, flags, n_persons)"""
    away = away or {}
    busy = set().union(*away.values()) if away else set()
    rng = np.random.default_rng(seed)
    dt = np.float64 if tri else np.float32
    pos = rng.uniform(-2, 2, (pcap, 3))
    poses = np.zeros((B, pcap, J, 3), dt)
    flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
    n_persons = np.zeros(B, np.int32)
    for f in range(B):
        step = rng.normal(size=(pcap, 3))
        pos = pos + 0.02 * step / np.linalg.norm(step, axis=1, keepdims=True)
        if f % 9 == 4 and f not in busy and f - 1 not in busy:
            continue
        full = f % 13 == 6
        seen = [k for k in range(pcap if full else 4) if full or rng.random() >= 0.15]
        seen = [k for k in seen if f not in away.get(k, ())]
        rows = [('p', k) for k in seen]
        if len(rows) < pcap and rows and rng.random() < 0.3:
            rows.append(('p', rows[0][1]))                       # the same pose twice
        if len(rows) < pcap and rng.random() < 0.3:
            rows.append(('x', 0))                                # a row below n_persons that is no detection
        rows = [rows[i] for i in rng.permutation(len(rows))]
        n_persons[f] = len(rows)
        for p, (kind, k) in enumerate(rows):
            poses[f, p] = (SHAPE + pos[k]).astype(dt)
            if kind == 'x':
                continue
            if tri:
                flags[f, p] = rng.random(J) >= 0.1
            else:
                flags[f, p] = 1
    return poses, flags, n_persons


def lattice_sequence(seed, n, tri, B=4, pcap=128):
    """B frames of n people on a 0.3 m lattice with 1 cm of jitter per frame, rows permuted per frame; the last person
    stands exactly where the first one does (a deliberate tie)."""
    rng = np.random.default_rng(seed)
    dt = np.float64 if tri else np.float32
    base = np.stack([0.3 * (np.arange(n) % 12), np.zeros(n), 0.3 * (np.arange(n) // 12)], axis=1)
    poses = np.zeros((B, pcap, J, 3), dt)
    flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
    for f in range(B):
        at = base + rng.uniform(-0.01, 0.01, (n, 3))
        at[n - 1] = at[0]
        order = rng.permutation(n)
        poses[f, :n] = (SHAPE[None] + at[order][:, None]).astype(dt)
        flags[f, :n] = 1
    return poses, flags, np.full(B, n, np.int32)


def in_chunks(run, poses, flags, n_persons, chunks):
    """run(poses, flags, n_persons) per chunk, in order -> the outputs of the chunks joined."""
    outs, at = [], 0
    for n in chunks:
        outs.append(run(poses[at:at + n], flags[at:at + n], n_persons[at:at + n]))
        at += n
    assert at == len(poses)
    return {k: np.concatenate([o[k] for o in outs]) for k in ('ids', 'cost', 'gap')}
