"""What the tests of the pose writer share (test_write_host.py, test_gpu_write.py): the doubles every conversion is held
to repr on, and small pose batches with every kind of row the format has to deal with."""
import struct

import numpy as np


def _bits(x):
    return struct.unpack('<Q', struct.pack('<d', float(x)))[0]


def format_values():
    """The bit patterns (uint64) of the value set: both zeros; the least and greatest subnormal, the least normal, the
    greatest finite; every power of two 2^k, k = -1074 .. 1023, with the double on each side of it (the intervals that
    are not symmetric); the ends of repr's positional range; 1e21 .. 1e23; 0.1 + 0.2, 5e-324, 2^53 + 1 as Python reads
    it; integral doubles up to 2^53; 20 000 seeded uniform 64-bit patterns without NaN and infinity; 20 000 seeded
    float32 values, widened.  All with both signs where the list names one."""
    v = [0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF]
    for k in range(-1074, 1024):
        b = _bits(2.0 ** k) if k >= -1022 else 1 << (k + 1074)
        v += [b - 1, b, b + 1] if b > 1 else [b, b + 1]
    for x in (1e-5, 1e-4, 9.999999999999999e-05, 1e15, 1e16, 9999999999999998.0, 1e21, 1e22, 1e23, 0.1 + 0.2, 5e-324,
              9007199254740993.0, 123456.789, 1.5, 0.001, 1e-3, 1234567890123456.0, 12345678901234567.0, 0.3, 2.5e-5, 4.35,
              1.2345678901234568e+17, 1.7976931348623157e308, 2.2250738585072014e-308, 2.225073858507201e-308):
        v += [_bits(x), _bits(-x)]
    ints = [0, 1, 2, 3, 9, 10, 11, 99, 100, 101, 999, 1000, 123456789, 2 ** 31, 2 ** 32 - 1, 10 ** 15, 10 ** 15 + 1, 2 ** 53 - 1, 2 ** 53]
    ints += [10 ** e for e in range(16)] + [10 ** e - 1 for e in range(1, 16)] + [7 * 10 ** e for e in range(16)]
    rng = np.random.default_rng(20240607)
    ints += [int(x) for x in rng.integers(0, 2 ** 53, 2000)]
    v += [_bits(float(i)) for i in ints] + [_bits(-float(i)) for i in ints[1:40]]
    r = rng.integers(0, 2 ** 64, 20000, dtype=np.uint64)
    r = r[((r >> np.uint64(52)) & np.uint64(0x7FF)) != np.uint64(0x7FF)]
    v += [int(x) for x in r]
    f = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    f = f[((f >> np.uint32(23)) & np.uint32(0xFF)) != np.uint32(0xFF)]
    v += [int(x) for x in f.view(np.float32).astype(np.float64).view(np.uint64)]
    return np.array(v, dtype=np.uint64)


def expected_tokens(bits):
    """repr of every value: what json.dumps writes for a float."""
    return [repr(x) for x in np.asarray(bits, dtype=np.uint64).view(np.float64).tolist()]


# coordinates whose tokens have all lengths up to 24 bytes, in both notations
ADVERSARIAL = np.array([-1.2345678901234567e-300, -1.7976931348623157e+308, 1e-05, 1e+16, 5e-324, -0.0, 0.0, 3.0, 0.0001, 9.999999999999999e-05,
                        1e22, 1e23, 0.30000000000000004, -1234567.8901234567, 9999999999999998.0, 1e15, 123.456, -2.5, 1.2345678901234568e+17,
                        -2.2250738585072014e-308, 0.1, 100.0, 1e-07, -9.87654321e-05], dtype=np.float64)
LONGEST = -1.2345678901234567e-300               # 24 bytes, and 24 bytes again after a scale of 100
assert len(repr(LONGEST)) == 24 == len(repr(LONGEST * 100.0))


def pose_batch(B, pcap, J, tri, seed, ids=True, adversarial=False):
    """poses f64 [B,pcap,J,3] with joint flags [B,pcap,J] (tri) or f32 with row flags [B,pcap]; n_persons [B] with 0, pcap
    and more than pcap among them; ids [B,pcap] with -1 among them, or None.  Some flagged joints hold NaN or an infinity,
    and one row with a flag has no joint left (tri: no joint flagged; otherwise: every joint NaN)."""
    rng = np.random.default_rng(seed)
    if adversarial:
        poses = ADVERSARIAL[rng.integers(0, len(ADVERSARIAL), (B, pcap, J, 3))]
    else:
        poses = rng.normal(0.0, 2.0, (B, pcap, J, 3))
    with np.errstate(over='ignore'):
        poses = poses.astype(np.float64 if tri else np.float32)
    flags = (rng.random((B, pcap, J)) < 0.7).astype(np.uint8) if tri else (rng.random((B, pcap)) < 0.8).astype(np.uint8)
    n = rng.integers(0, pcap + 1, B).astype(np.int32)
    n[0] = pcap
    if B > 1:
        n[1] = 0
    if B > 2:
        n[2] = pcap + 3
    bad = rng.random((B, pcap, J, 3)) < 0.03
    poses[bad] = np.nan
    poses[rng.random((B, pcap, J, 3)) < 0.01] = np.inf
    poses[rng.random((B, pcap, J, 3)) < 0.01] = -np.inf
    f, p = 0, pcap - 1                               # a row with nothing to write, in a frame that has it
    if tri:
        flags[f, p] = 0
        flags[0, 0, 0] = 1
        poses[0, 0, 0] = [1.0, np.nan, 2.0]
    else:
        flags[f, p] = 1
        poses[f, p] = np.nan
        flags[0, 0] = 1
        poses[0, 0, 1] = [np.inf, 0.5, 2.0]
    tid = None
    if ids:
        tid = rng.integers(-1, 1000, (B, pcap)).astype(np.int32)
        tid[0, 0] = -1
        tid[B - 1, 0] = 2147483647
        tid[B - 1, pcap - 1] = -2147483648
    return poses, flags, n, tid
