"""GPU: what mpe_linear and mpe_mlp_forward read and write around their rows (include/mpe.h) -- the calling pattern of the
batch entry points, which the arithmetic tests never use: the row count as a device word beside a capacity that picks the
kernel and the grid, strides wider than the rows, NaN in everything the kernels must not read, a canary in everything
they must not write.  Cases, buffers and references: linear_cases.py (test_linear_cases_host.py checks them on the CPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_cases as lc

pytestmark = pytest.mark.gpu

IDS = [lc.case_id(c) for c in lc.CASES]


@pytest.fixture(scope='module')
def engine(calib, mlp_weights):
    from conftest import pkg
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=8, max_persons_per_camera=10)
    eng.load_mlp(mlp_weights)
    yield eng
    eng.close()


class Bench:
    """Per case, made once: the operands, the weights on the device and the plain call's result per row count."""

    def __init__(self, eng):
        self.eng, self.ops, self.layers, self.plain = eng, {}, {}, {}

    def of(self, i):
        if i not in self.ops:
            self.ops[i] = lc.operands(lc.CASES[i])
            self.layers[i] = lc.Layer(self.eng, self.ops[i][1], self.ops[i][2])
        return self.ops[i] + (self.layers[i],)

    def plain_rows(self, i, M):
        if (i, M) not in self.plain:
            x, _, _, layer = self.of(i)
            self.plain[(i, M)] = lc.plain_linear(self.eng, layer, lc.CASES[i], x[:M])
        return self.plain[(i, M)]

    def free(self):
        for layer in self.layers.values():
            layer.free()


@pytest.fixture(scope='module')
def bench(engine):
    b = Bench(engine)
    yield b
    b.free()


def _bound(c, ex, x, w, b):
    """The bound tests/test_gpu_parity.py states for the form against the float64 layer (its rms bounds were measured on
    3000-row operands and are not used here)."""
    scale = ex.abs().max().item()
    ulp = 2.0 ** (np.floor(np.log2(scale)) - 23)
    if c.form == 'f32':                    # test_linear_vs_torch_fp32: one fp32 chain of length k (16 * 4e-7 * sqrt(k) would be wider)
        return 4e-7 * np.sqrt(c.k) * 4
    if c.form == 'acc64':                  # test_linear_vs_torch_fp32: at least as close as torch's sgemm, or a rounding of the scale
        ref = torch.nn.functional.linear(x, w, b)
        if c.slope is not None:
            ref = torch.nn.functional.leaky_relu(ref, c.slope)
        return max(2.0 * (ref.double() - ex).abs().max().item(), 2.5e-7 * scale)
    if c.form == 'split':                  # test_split_bf16_linear_is_fp32_accurate_and_batch_invariant
        return 2.0 * ulp
    if c.form == 'flush1':                 # test_split_bf16_flush_per_stage_is_more_accurate_and_batch_invariant
        return 1.5 * ulp
    assert c.form == 'f64mm'               # test_f64_matrix_pipe_linear_is_the_exact_layer
    return 1.01 * float(np.spacing(np.float32(scale)))


A_PARAMS = [(i, dm) for i, c in enumerate(lc.CASES) for dm in lc.row_counts(c)]


@pytest.mark.parametrize('i,dm', A_PARAMS, ids=['%s-dm%d' % (IDS[i], dm) for i, dm in A_PARAMS])
def test_device_side_row_count(engine, bench, i, dm):
    """Test A.  m = the capacity, the rows as a device word: M = clamp(*d_m, 0, m_cap) rows come out with the bits of the
    plain call on M rows and within the form's bound of the float64 layer; nothing else of C changes (rows >= M, columns
    [n, ldc), the guard rows), whatever NaN stands in the rows >= M and the columns >= ldw of A.  -1 and 0 write nothing."""
    c = lc.CASES[i]
    x, w, b, layer = bench.of(i)
    M = min(max(dm, 0), c.m_cap)
    lda, ldc = layer.ldw + 8, lc.round_up(c.n, 4) + 8
    assert layer.ldw == lc.ldw_of(c.k)
    a_buf = lc.build_a(c, x, lda, M)
    rc, c_buf = lc.guarded_linear(engine, layer, c, a_buf, lc.build_c(c.m_cap, ldc), c.m_cap, d_m=dm)
    assert rc == lc.MPE_OK
    stray = lc.stray_writes(c_buf, M, c.n)
    assert not stray, (len(stray), sorted(stray)[:8])
    if M == 0:
        return
    assert lc.unwritten(c_buf, M, c.n) == 0
    got = lc.result_of(c_buf, M, c.n)
    want = bench.plain_rows(i, M)
    diff = (got != want) | got.isnan()
    assert lc.same_bits(got, want), (int(diff.sum()), np.argwhere(diff.numpy())[:8].tolist())
    ex = lc.reference64(a_buf, w, b, M, c.k, lc.ref_slope(c))
    err, bound = (got.double() - ex).abs().max().item(), _bound(c, ex, x[:M], w, b)
    print('%s *d_m=%d: max error %.3e, bound %.3e' % (IDS[i], dm, err, bound))
    assert err <= bound, (err, bound)


STRIDES = [(0, 0), (32, 4), (4, 36)]       # (lda - ldw, ldc - round_up(n, 4))


@pytest.mark.parametrize('extra', STRIDES, ids=['lda+%d-ldc+%d' % s for s in STRIDES])
@pytest.mark.parametrize('i', range(len(lc.CASES)), ids=IDS)
def test_strides_alone(engine, bench, i, extra):
    """Test B.  Host row count (d_m = NULL, m = m_cap); A and C as views of wider rows: the bits of the packed call, and the
    pad columns of C (n = 70: the last four-float store straddles n; n = 96: every store is full) and the guard rows keep
    theirs."""
    c = lc.CASES[i]
    x, w, b, layer = bench.of(i)
    lda, ldc = layer.ldw + extra[0], lc.round_up(c.n, 4) + extra[1]
    rc, c_buf = lc.guarded_linear(engine, layer, c, lc.build_a(c, x, lda), lc.build_c(c.m_cap, ldc), c.m_cap)
    assert rc == lc.MPE_OK
    stray = lc.stray_writes(c_buf, c.m_cap, c.n)
    assert not stray, (len(stray), sorted(stray)[:8])
    assert lc.same_bits(lc.result_of(c_buf, c.m_cap, c.n), bench.plain_rows(i, c.m_cap))


@pytest.mark.parametrize('i', range(len(lc.CASES)), ids=IDS)
def test_finite_padding_of_a_changes_nothing(engine, bench, i):
    """Test C.  Columns [k, ldw) of A meet the zero padding of W: finite values there (in [1, 2)) leave every bit as it is --
    the rule include/mpe.h states at mpe_linear."""
    c = lc.CASES[i]
    x, w, b, layer = bench.of(i)
    assert layer.ldw > c.k
    pad = torch.rand(c.m_cap, layer.ldw - c.k, generator=torch.Generator().manual_seed(900 + i)) + 1.0
    assert (pad >= 1).all() and (pad < 2).all()
    lda, ldc = layer.ldw + 8, lc.round_up(c.n, 4) + 8
    rc, c_buf = lc.guarded_linear(engine, layer, c, lc.build_a(c, x, lda, pad=pad), lc.build_c(c.m_cap, ldc), c.m_cap)
    assert rc == lc.MPE_OK
    assert not lc.stray_writes(c_buf, c.m_cap, c.n)
    assert lc.same_bits(lc.result_of(c_buf, c.m_cap, c.n), bench.plain_rows(i, c.m_cap))


# one case per form, the smallest of each
FORMS = [i for i, c in enumerate(lc.CASES) if c.reaches in ('k_linear_skinny', 'k_linear_skinny<ACC64>', 'k_linear_sb_skinny<F64>',
                                                            'k_linear_sb_skinny<!F64>', 'k_linear_sb_ks<FL=1,RT=1>', 'k_linear_f64')]


@pytest.mark.parametrize('what', ['lda % 4', 'd_a', 'd_w', 'd_c', 'lda beyond the offset', 'lda far beyond the offset'])
@pytest.mark.parametrize('i', FORMS, ids=[IDS[i] for i in FORMS])
def test_linear_refuses_what_it_cannot_address(engine, bench, i, what):
    """Test D.  Every form moves its operands in 16-byte pieces and the split form's tile kernel addresses 255 rows of lda
    floats by a 32-bit byte offset: a stride or a pointer that does not fit is refused on the host (MPE_ERR_INVALID), nothing
    is launched and C keeps its canary."""
    assert len(FORMS) == 6
    c = lc.CASES[i]
    x, w, b, layer = bench.of(i)
    lda, ldc, m = layer.ldw + 8, lc.round_up(c.n, 4) + 8, c.m_cap
    a_off = w_off = c_off = 0
    if what == 'lda % 4':
        lda = layer.ldw + 2
    elif what == 'lda beyond the offset':
        lda, m = (1 << 21) + 4, 1                             # (the check precedes any launch: no buffer of that size)
    elif what == 'lda far beyond the offset':
        lda, m = 1 << 23, 1                                   # 255 * 2^23 * 4 bytes: does not fit 32 bits
    else:
        a_off, w_off, c_off = 4 * (what == 'd_a'), 4 * (what == 'd_w'), 4 * (what == 'd_c')
    a_dev = lc.build_a(c, x, lda if m > 1 else layer.ldw + 8).cuda()
    c_dev = lc.build_c(c.m_cap, ldc).cuda()
    row_a = 4 * a_dev.shape[1]
    rc = lc.raw_linear(engine, layer, lc.flags_of(c), c.slope, a_dev.data_ptr() + row_a + a_off, lda, c_dev.data_ptr() + 4 * ldc + c_off,
                       ldc, m, None, d_w=layer.dw.value + w_off)
    assert rc == lc.MPE_ERR_INVALID
    assert not lc.stray_writes(c_dev.cpu(), 0, c.n)
    # the same call with the argument put right goes through (the refusal was about that argument alone)
    if what in ('d_a', 'd_w', 'd_c', 'lda % 4'):
        a_buf = lc.build_a(c, x, layer.ldw + 8)
        rc, c_buf = lc.guarded_linear(engine, layer, c, a_buf, lc.build_c(c.m_cap, ldc), c.m_cap)
        assert rc == lc.MPE_OK and lc.same_bits(lc.result_of(c_buf, c.m_cap, c.n), bench.plain_rows(i, c.m_cap))


def _mlp_dims(engine, mlp_weights):
    first = min(int(k.split('.')[1]) for k in mlp_weights)
    k = int(np.asarray(mlp_weights['layers.%d.weight' % first]).shape[1])
    return k, lc.round_up(k, 128), engine.mlp_out


def _mlp_rows(k, m):
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(4100 + m))
    return torch.where(x > 0, x, 0.1 * x)


def _mlp_strided(engine, x, ld_in, ld_x, ld_y, x_off=0):
    """mpe_mlp_forward on x as a view of wider rows (NaN beyond the columns it reads, NaN guard rows) into a canary buffer
    -> (return code, the buffer read back)."""
    m, k = x.shape
    xb = torch.full((m + 2, ld_x), float('nan'), dtype=torch.float32)
    xb[1:-1, :k] = x
    xb[1:-1, k:ld_in] = 0.0
    xd, yd = xb.cuda(), lc.build_c(m, ld_y).cuda()
    rc = engine.lib.mpe_mlp_forward(engine.ctx, engine._stream(), C.c_void_p(xd.data_ptr() + 4 * ld_x + x_off), ld_x, m,
                                    C.c_void_p(yd.data_ptr() + 4 * ld_y), ld_y)
    torch.cuda.synchronize(engine.device)
    return rc, yd.cpu()


@pytest.mark.parametrize('what', ['ld_x % 4', 'ld_y < n_out', 'd_x'])
def test_mlp_forward_refuses_what_it_cannot_address(engine, mlp_weights, what):
    """Test D, mpe_mlp_forward: ld_x % 4 != 0, a misaligned d_x and ld_y < n_out are refused on the host; y keeps its canary."""
    k, ld_in, n_out = _mlp_dims(engine, mlp_weights)
    ld_x = ld_in + (2 if what == 'ld_x % 4' else 8)
    ld_y = n_out - 2 if what == 'ld_y < n_out' else n_out + 10
    rc, y = _mlp_strided(engine, _mlp_rows(k, 5), ld_in, ld_x, ld_y, x_off=4 if what == 'd_x' else 0)
    assert rc == lc.MPE_ERR_INVALID
    assert not lc.stray_writes(y, 0, n_out)


@pytest.mark.parametrize('m', [1, 37])
def test_mlp_forward_through_strided_views(engine, mlp_weights, m):
    """Test E.  The panoptic MLP on rows that are views of wider ones (ld_x = mlp_ld_in + 8, NaN behind the columns it reads;
    ld_y = n_out + 10 into a canary buffer): the bits of Engine.mlp_forward on the same rows and nothing written outside them,
    in the default mode, in mode 1 and in mode 5; back in the default mode the default's bits return."""
    k, ld_in, n_out = _mlp_dims(engine, mlp_weights)
    x = _mlp_rows(k, m)

    def both(tag):
        want = engine.mlp_forward(x.cuda()).cpu()
        rc, y = _mlp_strided(engine, x, ld_in, ld_in + 8, n_out + 10)
        assert rc == lc.MPE_OK, tag
        stray = lc.stray_writes(y, m, n_out)
        assert not stray, (tag, sorted(stray)[:8])
        got = lc.result_of(y, m, n_out)
        assert torch.isfinite(got).all() and lc.same_bits(got, want), tag
        return got

    y_def = both('default')
    try:
        engine.set_precision(False, True, mlp_split=False)
        y_m1 = both('mode 1')
        engine.set_precision(False, True, mlp_f64=True)
        y_m5 = both('mode 5')
    finally:
        engine.set_precision(False, True)
    assert lc.same_bits(both('default again'), y_def)
    # (the three modes are three arithmetics: were they bit-equal on all 37 x 54 outputs, a mode switch would not have happened)
    if m == 37:
        assert not lc.same_bits(y_m1, y_def) and not lc.same_bits(y_m5, y_def)
