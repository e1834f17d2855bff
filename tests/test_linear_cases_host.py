"""CPU: the helpers of the GEMM contract tests on their own (linear_cases.py) -- the case table against the restated dispatch
rules, the canary checker against planted stray writes, the float64 reference against the NaN regions of its buffer."""
import numpy as np
import pytest
import torch

import linear_cases as lc


@pytest.mark.parametrize('case', lc.CASES, ids=lc.case_id)
def test_table_reaches_what_the_restated_dispatch_says(case):
    """Each row of the table names the kernel the launchers' rules send its shape to (256 CUs, default environment): a row
    edited to a shape that lands elsewhere fails here, without a GPU."""
    kernel, rows = lc.dispatch(lc.flags_of(case), case.m_cap, case.n, case.k, cu=256)
    assert kernel == case.reaches
    assert rows == (16 if 'skinny' in kernel or '_ks' in kernel else 256 if kernel.startswith('k_linear_sb<') else 128)
    # the leaky bit is no part of the rule
    assert lc.dispatch(case.flags, case.m_cap, case.n, case.k)[0] == lc.dispatch(case.flags | lc.LEAKY, case.m_cap, case.n, case.k)[0]


def test_table_covers_every_reachable_kernel_and_both_slopes():
    reached = {c.reaches for c in lc.CASES}
    assert len(reached) == len(lc.CASES)                     # no kernel twice
    assert {'k_linear_skinny', 'k_linear_skinny<ACC64>', 'k_linear_skinny_ks', 'k_linear_dma<NTT=4>', 'k_linear_dma<ACC64,NTT=4>',
            'k_linear_sb_skinny<F64>', 'k_linear_sb_skinny<!F64>', 'k_linear_sb_ks<FL=2,RT=1>', 'k_linear_sb_ks<FL=2,RT=2>',
            'k_linear_sb_ks<FL=1,RT=1>', 'k_linear_sb<NTT=4,F64,FL=2>', 'k_linear_sb<NTT=4,F64,FL=1>', 'k_linear_f64'} <= reached
    leaky = sum(c.slope is not None for c in lc.CASES)
    assert abs(2 * leaky - len(lc.CASES)) <= 2


def test_dispatch_thresholds():
    """The rule's own borders: one more row tile, one more CU, one K stage fewer send a shape elsewhere."""
    # waves16 = 1024 stays on the wave-per-tile kernel, 1030 > 1024 goes to the tiles (nt16 = 6: not narrow)
    assert lc.dispatch(0, 2720, 96, 72)[0] == 'k_linear_skinny'                    # 170 x 6 = 1020
    assert lc.dispatch(0, 2736, 96, 72)[0] == 'k_linear_dma<NTT=4>'                # 171 x 6 = 1026
    assert lc.dispatch(lc.ACC64, 40, 70, 224)[0] == 'k_linear_skinny<ACC64>'       # nk = 7
    assert lc.dispatch(lc.ACC64, 40, 70, 225)[0] == 'k_linear_skinny_ks'           # nk = 8
    assert lc.dispatch(lc.ACC64, 2750, 64, 72)[0] == 'k_linear_skinny<ACC64>'      # narrow (nt16 = 4) at any batch size
    # two row tiles per workgroup only where 2 nt16 exceeds the CU count, and never for a single row tile
    assert lc.dispatch(lc.SPLIT, 40, 2064, 270, cu=256)[0] == 'k_linear_sb_ks<FL=2,RT=2>'
    assert lc.dispatch(lc.SPLIT, 40, 2048, 270, cu=256)[0] == 'k_linear_sb_ks<FL=2,RT=1>'   # 2 x 128 = 256: not more than the CUs
    assert lc.dispatch(lc.SPLIT, 40, 2064, 270, cu=304)[0] == 'k_linear_sb_ks<FL=2,RT=1>'
    assert lc.dispatch(lc.SPLIT, 16, 2064, 270, cu=256)[0] == 'k_linear_sb_ks<FL=2,RT=1>'
    # few row tiles of a wide layer stay on the K-split kernel beyond 1024 waves (48 row tiles x 40 = 1920), 49 do not
    assert lc.dispatch(lc.SPLIT, 768, 640, 270)[0] == 'k_linear_sb_ks<FL=2,RT=1>'
    assert lc.dispatch(lc.SPLIT, 784, 640, 270)[0] == 'k_linear_sb<NTT=4,F64,FL=2>'
    assert lc.dispatch(lc.F64MM, 1, 1, 1) == ('k_linear_f64', 128)


def test_row_counts_walk_the_tile_borders():
    for c in lc.CASES:
        counts = lc.row_counts(c)
        rows = lc.dispatch(lc.flags_of(c), c.m_cap, c.n, c.k)[1]
        assert len(counts) == 12 and counts[:3] == [-1, 0, 1] and counts[-3:] == [c.m_cap - 1, c.m_cap, c.m_cap + 7]
        edge = 16 if rows == 16 else 128
        assert counts[3:9] == [edge - 1, edge, edge + 1, 2 * edge - 1, 2 * edge, 2 * edge + 1]
        assert max(counts[3:9]) < c.m_cap                     # every border lies inside the capacity


CASE = lc.CASES[0]          # 40 x 70 x 33


def _buffers(M, lda_extra=8, ldc_extra=8):
    x, w, b = lc.operands(CASE)
    a = lc.build_a(CASE, x, lc.ldw_of(CASE.k) + lda_extra, M)
    c = lc.build_c(CASE.m_cap, lc.round_up(CASE.n, 4) + ldc_extra)
    return x, w, b, a, c


def test_buffers_are_laid_out_as_stated():
    M = 17
    x, w, b, a, c = _buffers(M)
    ldw = lc.ldw_of(CASE.k)
    assert a.shape == (CASE.m_cap + 2, ldw + 8) and c.shape == (CASE.m_cap + 2, 72 + 8) and c.dtype == torch.int32
    assert torch.equal(a[1:1 + M, :CASE.k], x[:M]) and (a[1:1 + M, CASE.k:ldw] == 0).all()
    assert a[1:1 + M, ldw:].isnan().all() and a[0].isnan().all() and a[1 + M:].isnan().all()
    assert (c == lc.CANARY).all()
    f = c.view(torch.float32)
    assert f.isnan().all() and lc.CANARY != np.float32('nan').view(np.int32)          # a NaN, but not the one arithmetic makes
    full = lc.build_a(CASE, x, ldw)                                                    # no row count: every row of x is there
    assert torch.equal(full[1:-1, :CASE.k], x) and full.shape[1] == ldw and full[-1].isnan().all()
    pad = torch.rand(CASE.m_cap, ldw - CASE.k) + 1.0
    assert torch.equal(lc.build_a(CASE, x, ldw, pad=pad)[1:-1, CASE.k:], pad)


def test_checker_reports_nothing_on_an_untouched_buffer():
    for M in (-1, 0, 1, 17, CASE.m_cap):
        c = lc.build_c(CASE.m_cap, 80)
        assert lc.stray_writes(c, M, CASE.n) == set()
        assert lc.unwritten(c, M, CASE.n) == max(M, 0) * CASE.n


@pytest.mark.parametrize('where,cell', [('a row >= M', (17, 3)), ('a column in [n, ldc)', (5, 70)), ('the last pad column', (0, 79)),
                                        ('the front guard row', (-1, 0)), ('the back guard row', (CASE.m_cap, 79)),
                                        ('the last row of the capacity', (CASE.m_cap - 1, 0))])
def test_checker_reports_a_planted_stray_write(where, cell):
    M = 17
    c = lc.build_c(CASE.m_cap, 80)
    c[1:1 + M, :CASE.n] = 0                                   # what a correct kernel writes
    assert lc.stray_writes(c, M, CASE.n) == set() and lc.unwritten(c, M, CASE.n) == 0
    c[cell[0] + 1, cell[1]] = torch.tensor(1.0).view(torch.int32)
    assert lc.stray_writes(c, M, CASE.n) == {cell}, where
    # a canonical NaN written over the canary is a write as well
    c[cell[0] + 1, cell[1]] = torch.tensor(float('nan')).view(torch.int32)
    assert lc.stray_writes(c, M, CASE.n) == {cell}, where


def test_checker_counts_rows_from_zero_for_an_empty_launch():
    c = lc.build_c(CASE.m_cap, 80)
    c[1, 0] = 0
    assert lc.stray_writes(c, 0, CASE.n) == {(0, 0)} and lc.stray_writes(c, -1, CASE.n) == {(0, 0)}
    assert lc.stray_writes(c, 1, CASE.n) == set()


def test_reference_ignores_the_nan_regions():
    M = 17
    x, w, b, a, _ = _buffers(M)
    for slope in (None, 0.1):
        ex = lc.reference64(a, w, b, M, CASE.k, slope)
        assert ex.dtype == torch.float64 and ex.shape == (M, CASE.n) and torch.isfinite(ex).all()
        want = x[:M].double() @ w.double().T + b.double()
        if slope is not None:
            want = torch.where(want > 0, want, slope * want)
        assert torch.equal(ex, want)
    # and it is what numpy computes from the plain operands, to float64 rounding
    ref = x[:M].numpy().astype(np.float64) @ w.numpy().astype(np.float64).T + b.numpy().astype(np.float64)
    assert np.abs(lc.reference64(a, w, b, M, CASE.k, None).numpy() - ref).max() <= 1e-14 * np.abs(ref).max() * CASE.k
    # one row more would read a NaN row: the reference does not hide a wrong row count
    assert lc.reference64(a, w, b, M + 1, CASE.k, None)[M].isnan().all()


def test_reference_slope_per_form():
    f64 = [c for c in lc.CASES if c.flags & lc.F64MM][0]._replace(slope=0.1)
    assert lc.ref_slope(f64) == 0.1 and lc.ref_slope(CASE) == float(np.float32(0.1)) != 0.1
    assert lc.ref_slope(CASE._replace(slope=None)) is None


def test_same_bits_tells_nans_apart():
    a = torch.tensor([1.0, float('nan')])
    assert lc.same_bits(a, a.clone())
    assert not lc.same_bits(a, torch.tensor([1.0, 2.0])) and not lc.same_bits(a, a[:1])
    b = a.clone()
    b.view(torch.int32)[1] = lc.CANARY
    assert not lc.same_bits(a, b)
