"""Cases, buffers and references for the contract tests of the GEMM entry points (test_linear_cases_host.py: the table, the
canary checker and the reference on their own; test_gpu_linear_contract.py: mpe_linear / mpe_mlp_forward against them).
What the other GEMM tests never vary: the row count as a device word beside a capacity, row strides wider than the rows,
what lies around the rows of A and C.  Everything is seeded.  Not a test module.

Dispatch arithmetic of the table (csrc/gemm.hip launch_linear, csrc/gemm_sb16.hip launch_linear_sb16, csrc/gemm_f64.hip
launch_linear_f64; MPE_SKINNY_WAVES = 1024, MPE_GEMM_NARROW on, 256 CUs; ldw = round_up(k, 32), nk = ldw / 32, nt16 =
ceil(n / 16), waves16 = ceil(m_cap / 16) * nt16):
  40 x 70:    nt16 = 5, waves16 = 3 * 5 = 15 <= 1024 -> the wave-per-tile kernels; with f64 sums and nk >= 8 (k = 270: ldw = 288,
              nk = 9) the K-split ones, below (k = 33: nk = 2; k = 72: nk = 3) one wave per tile
  40 x 2064:  nt16 = 129, waves16 = 387; 2 * 129 = 258 > 256 CUs and three row tiles -> two row tiles per workgroup (RT = 2):
              workgroup rows {0, 1} and {2, -}, the second tile of the second one holds rows 32 .. 39
  2750 x 96:  nt16 = 6 (not narrow: > 4), waves16 = 172 * 6 = 1032 > 1024, 172 row tiles > few_rows_tiles = 48 -> the tile
              kernels: fp32 MFMA 22 row tiles x 2 = 44 tiles either width, the tie goes to 64-wide (NTT = 4); split with f64
              sums 64-wide, 11 x 2 tiles of 256 rows; split without 80-wide (NTT = 5: features 80 .. 95 in a second tile)
  300 x 70:   the f64 form has one kernel; three 128-row tiles, the last with 44 rows
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

# flag bits of mpe_linear (include/mpe.h)
LEAKY, ACC64, SPLIT, SPLIT_NO_F64, SPLIT_FLUSH1, F64MM = 1, 2, 4, 8, 16, 32
MPE_OK, MPE_ERR_INVALID = 0, -1

Case = namedtuple('Case', 'form flags m_cap n k slope reaches')

# form: which bound of tests/test_gpu_parity.py the result answers to ('f32' chain, 'acc64', 'split', 'flush1', 'f64mm')
CASES = [
    Case('f32', 0, 40, 70, 33, 0.1, 'k_linear_skinny'),                                  # nk = 2 < SK_DEPTH
    Case('f32', 0, 2750, 96, 72, None, 'k_linear_dma<NTT=4>'),
    Case('acc64', ACC64, 40, 70, 33, None, 'k_linear_skinny<ACC64>'),                    # nk = 2 < 8
    Case('acc64', ACC64, 40, 70, 270, 0.1, 'k_linear_skinny_ks'),                        # nk = 9
    Case('acc64', ACC64, 2750, 96, 72, 0.1, 'k_linear_dma<ACC64,NTT=4>'),
    Case('split', SPLIT, 40, 70, 33, 0.1, 'k_linear_sb_skinny<F64>'),
    Case('split', SPLIT | SPLIT_NO_F64, 40, 70, 72, None, 'k_linear_sb_skinny<!F64>'),   # nk = 3: even / odd chains
    Case('split', SPLIT, 40, 70, 270, None, 'k_linear_sb_ks<FL=2,RT=1>'),
    Case('split', SPLIT, 40, 2064, 270, 0.1, 'k_linear_sb_ks<FL=2,RT=2>'),
    Case('split', SPLIT, 2750, 96, 72, None, 'k_linear_sb<NTT=4,F64,FL=2>'),
    Case('flush1', SPLIT | SPLIT_FLUSH1, 2750, 96, 72, 0.1, 'k_linear_sb<NTT=4,F64,FL=1>'),
    Case('flush1', SPLIT | SPLIT_FLUSH1, 40, 70, 270, 0.1, 'k_linear_sb_ks<FL=1,RT=1>'),
    Case('f64mm', F64MM, 300, 70, 33, None, 'k_linear_f64'),
    # beside the issue's table: the tile kernel of the GAT launches (no f64 sums, 80-wide tiles), which production runs with a
    # device-side row count as well
    Case('split', SPLIT | SPLIT_NO_F64, 2750, 96, 72, 0.1, 'k_linear_sb<NTT=5,!F64>'),
]


def case_id(c):
    return '%s-%dx%dx%d' % (c.reaches, c.m_cap, c.n, c.k)


def round_up(x, m):
    return (x + m - 1) // m * m


def ldw_of(k):
    return round_up(k, 32)


def flags_of(c):
    return c.flags | (LEAKY if c.slope is not None else 0)


# ---- the launchers' rules, restated -----------------------------------------------------------------------------------------

def dispatch(flags, m_cap, n, k, cu=256, skinny_waves=1024, narrow_on=1):
    """-> (kernel, rows per tile) that mpe_linear reaches for these flags and this shape under the default environment."""
    k_pad = ldw_of(k)
    nk, nt16, row_tiles = k_pad // 32, (n + 15) // 16, (m_cap + 15) // 16
    waves16 = row_tiles * nt16
    if flags & F64MM:                                             # launch_linear_f64: one kernel
        return 'k_linear_f64', 128
    if flags & SPLIT:                                             # launch_linear_sb16
        f64 = not flags & SPLIT_NO_F64
        fl = 1 if flags & SPLIT_FLUSH1 else 2
        narrow = bool(narrow_on) and nt16 <= (4 if f64 else 1)
        few_rows = f64 and skinny_waves > 0 and row_tiles <= (32 if nt16 >= 128 else 48) and nt16 > 4
        if f64 and (waves16 <= skinny_waves or narrow or few_rows) and 8 <= nk <= 128 * fl:
            rt2 = row_tiles > 1 and 2 * nt16 > cu and (nk + fl - 1) // fl * 2048 <= 128 * 1024
            return 'k_linear_sb_ks<FL=%d,RT=%d>' % (fl, 2 if rt2 else 1), 16
        if waves16 <= skinny_waves or narrow:
            return 'k_linear_sb_skinny<%sF64>' % ('' if f64 else '!'), 16
        if f64:
            return 'k_linear_sb<NTT=4,F64,FL=%d>' % fl, 256
        return 'k_linear_sb<NTT=5,!F64>', 256
    acc64 = bool(flags & ACC64)                                   # launch_linear
    narrow = bool(narrow_on) and nt16 <= (4 if acc64 else 1)
    if (waves16 <= skinny_waves or narrow) and acc64 and 8 <= nk <= 128:
        return 'k_linear_skinny_ks', 16
    if waves16 <= skinny_waves or narrow:
        return 'k_linear_skinny' + ('<ACC64>' if acc64 else ''), 16
    ntm = (m_cap + 127) // 128
    tiles64, tiles80 = ntm * ((n + 63) // 64), ntm * ((n + 79) // 80)
    wide = (tiles80 + 255) // 256 * 80 < (tiles64 + 255) // 256 * 64          # (256: a constant of the rule, not the CU count)
    return 'k_linear_dma<%sNTT=%d>' % ('ACC64,' if acc64 else '', 5 if wide else 4), 128


def row_counts(c):
    """The device-side row counts Test A runs a case over: around the tile borders of the kernel it reaches."""
    rows = dispatch(flags_of(c), c.m_cap, c.n, c.k)[1]
    edges = [15, 16, 17, 31, 32, 33] if rows == 16 else [127, 128, 129, 255, 256, 257]
    return [-1, 0, 1] + edges + [c.m_cap - 1, c.m_cap, c.m_cap + 7]


# ---- operands, buffers, canaries ---------------------------------------------------------------------------------------------

CANARY = 0x7FC5A5A5        # a NaN no arithmetic produces (quiet, payload 0x45A5A5): a cell that still holds it was not written


def operands(c, seed=None):
    """-> x [m_cap][k], w [n][k], b [n] (float32, CPU): randn rows through a leaky 0.1, weights / sqrt(k), as the GEMM tests
    of test_gpu_parity.py."""
    g = torch.Generator().manual_seed(17 * c.k + c.n + 3 * c.m_cap if seed is None else seed)
    x = torch.randn(c.m_cap, c.k, generator=g)
    x = torch.where(x > 0, x, 0.1 * x)
    w = torch.randn(c.n, c.k, generator=g) / np.sqrt(c.k)
    b = torch.randn(c.n, generator=g)
    return x, w, b


def build_a(c, x, lda, M=None, pad=None):
    """A as the kernel may find it, [m_cap + 2][lda] with a guard row in front and behind (the entry point gets row 1):
    columns [0, k) = x, [k, ldw) zero (or `pad` [m_cap][ldw - k]), [ldw, lda) NaN, the guard rows NaN; with the row count
    known every row >= M is NaN over its whole length."""
    ldw = ldw_of(c.k)
    assert lda >= ldw and tuple(x.shape) == (c.m_cap, c.k)
    a = torch.full((c.m_cap + 2, lda), float('nan'), dtype=torch.float32)
    a[1:-1, :c.k] = x
    a[1:-1, c.k:ldw] = 0.0 if pad is None else pad
    if M is not None:
        a[1 + max(M, 0):] = float('nan')
    return a


def build_c(rows, ldc):
    """C [rows + 2][ldc] as int32, every cell the canary (guard rows included; the entry point gets row 1)."""
    return torch.full((rows + 2, ldc), CANARY, dtype=torch.int32)


def stray_writes(c_buf, M, n):
    """Cells of a build_c buffer (CPU) that changed outside [0, M) x [0, n) -> set of (row, column), rows counted from the
    entry point's row 0: -1 is the front guard row, the buffer's row count - 2 the back one."""
    changed = (c_buf != CANARY).numpy().copy()
    changed[1:1 + max(M, 0), :n] = False
    return {(int(r) - 1, int(col)) for r, col in np.argwhere(changed)}


def unwritten(c_buf, M, n):
    """Number of cells inside [0, M) x [0, n) that still hold the canary."""
    return int((c_buf[1:1 + max(M, 0), :n] == CANARY).sum())


def result_of(c_buf, M, n):
    """The rows [0, M) x [0, n) of a build_c buffer as float32."""
    return c_buf[1:1 + M, :n].contiguous().view(torch.float32)


def ref_slope(c):
    """The slope the form multiplies by, as a double: the f64 form takes the decimal (include/mpe.h, MLP mode 5), the others
    the fp32 number the ABI carries."""
    if c.slope is None:
        return None
    return float(c.slope) if c.flags & F64MM else float(np.float32(c.slope))


def reference64(a_buf, w, b, M, k, slope):
    """act(A[:M, :k] W^T + b) in float64 from a build_a buffer: nothing else of the buffer is looked at."""
    ex = a_buf[1:1 + M, :k].double() @ w.double().T + b.double()
    return ex if slope is None else torch.where(ex > 0, ex, slope * ex)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ---- the raw entry point (needs a GPU) ---------------------------------------------------------------------------------------

class Layer:
    """Weights on the device as mpe_upload_linear pads them."""

    def __init__(self, eng, w, b):
        from conftest import pkg
        f32p = pkg('lib').c_f32p
        self.eng = eng
        w, b = np.ascontiguousarray(w.numpy(), np.float32), np.ascontiguousarray(b.numpy(), np.float32)
        self.n, self.k = w.shape
        self.dw, self.db, ldw = C.c_void_p(), C.c_void_p(), C.c_int32()
        eng._chk(eng.lib.mpe_upload_linear(eng.ctx, w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), self.n, self.k,
                                           C.byref(self.dw), C.byref(self.db), C.byref(ldw)))
        self.ldw = ldw.value

    def free(self):
        self.eng.lib.mpe_free_device(self.eng.ctx, self.dw)
        self.eng.lib.mpe_free_device(self.eng.ctx, self.db)


def raw_linear(eng, layer, flags, slope, d_a, lda, d_c, ldc, m, d_m, d_w=None):
    """eng.lib.mpe_linear on raw device addresses (ints) -> its return code, the stream drained."""
    rc = eng.lib.mpe_linear(eng.ctx, eng._stream(), C.c_void_p(d_a), lda, layer.dw if d_w is None else C.c_void_p(d_w), layer.ldw,
                            layer.db, C.c_void_p(d_c), ldc, m, None if d_m is None else C.c_void_p(d_m.data_ptr()),
                            layer.n, layer.k, flags, 0.0 if slope is None else float(slope))
    torch.cuda.synchronize(eng.device)
    return rc


def guarded_linear(eng, layer, c, a_buf, c_buf, m, d_m=None):
    """mpe_linear of case `c` on a build_a / build_c pair (CPU tensors; the entry point gets their rows 1) -> (return code,
    the C buffer read back)."""
    a_dev, c_dev = a_buf.cuda(), c_buf.cuda()
    lda, ldc = a_buf.shape[1], c_buf.shape[1]
    dm = None if d_m is None else torch.tensor([d_m], dtype=torch.int32, device='cuda')
    rc = raw_linear(eng, layer, flags_of(c), c.slope, a_dev.data_ptr() + 4 * lda, lda, c_dev.data_ptr() + 4 * ldc, ldc, m, dm)
    return rc, c_dev.cpu()


def plain_linear(eng, layer, c, x):
    """The route the arithmetic tests pin to float64 (Engine.linear): host row count, no device count, packed strides, A
    freshly zeroed, C sliced to n columns -> [m][n] float32 on the CPU."""
    m = x.shape[0]
    a = torch.zeros((m, layer.ldw), dtype=torch.float32, device='cuda')
    a[:, :c.k] = x.cuda()
    ldc = round_up(c.n, 4)
    y = torch.empty((m, ldc), dtype=torch.float32, device='cuda')
    rc = raw_linear(eng, layer, flags_of(c), c.slope, a.data_ptr(), layer.ldw, y.data_ptr(), ldc, m, None)
    assert rc == MPE_OK, rc
    return y[:, :c.n].cpu().contiguous()
