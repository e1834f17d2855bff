"""The GAT stage on architectures other than the deployed one (tests/gat_arch_cases.py), against oracle_np.gat_layer in float64.

Routes on paper (read in csrc/gat.hip, api.hip, gemm.hip, lat.hip before the first run; V = 5, max_persons_per_camera 5, so
hmax = 25, m_cap = 251, n_cap = 276, max in-degree 26; every row stride the kernels see is ctx->act_ld, a multiple of LD_ALIGN = 32
floats, also through the stage entry points, which copy the caller's rows into the workspace):

  vector loads   agg_vec gives 4 only for out_dim % 4 == 0 and 2 only for out_dim % 2 == 0, so a column group of the head / fused
                 kernels starts at hh * out_dim + d with both terms multiples of VEC: fp32 groups are VEC * 4 bytes aligned, fp16
                 groups VEC * 2 (row stride in halves = 2 * act_ld).  The edge-node kernel also takes 16-byte groups when out_dim
                 is not a multiple of 4 (`wide`: fp32 rows, hd rounded up to 4 <= ld): group start c = 4 k, aligned; the padded last
                 group (hd = 30: columns 28..31) reads and writes inside the row stride (32 <= act_ld) and clamps its head index.
                 fp16 rows with out_dim % 8 != 0 (h16 layer 1, out_dim 12) take VEC 4 = 8-byte loads at multiples of 4 halves.
  row_coef       float4 loads only for out_dim == 40 (hh * 160 bytes), float2 only for out_dim == 30 (hh * 120 bytes); every other
                 width reads scalars.  Reached only without coefficients in a12 (latency route).
  k_attn_coef    16-byte loads need ld % 4 == 0 and hd4 * 4 <= ld: hd4 * 4 <= round_up(hd, 32) = act_ld.  LDS rows hd4 * 4 + 4
                 floats, at most 32 rows: 33 KiB for hd = 256 (`wide`).
  agg_store_row  vector store at row * ld_out + c, ld_out = act_ld: aligned as the loads.  Plane stores (latency route) go through
                 store_planes1 unless VEC == 4.
  fused LDS      tables 3072 floats + image n_cap * out_dim + 256: out_dim 40 -> 57 472 B, 64 (`wide`) -> 83 968 B (above 64 KiB:
                 the launch raises the kernel's dynamic-LDS attribute), 12 -> 26 560 B; all under FUSED_LDS_LIMIT = 160 KiB, so at 5
                 persons per camera EVERY architecture takes k_gat_fused.  `wide` at max_persons_per_camera 4: 55 552 B (fused), at 10:
                 hmax 50, m_cap 1001, n_cap 1051, tables 11 520 floats, 316 160 B -> the general kernels.  10 flips it: `wide` has a
                 second engine.  (n_cap 276 > 256 and hmax (hmax + 1) = 650 > 512: the overlapped staging is off at 5 persons per
                 camera for every shape, so MPE_FUSED_NO_OVERLAP switches phase 3's form only; engines built with 4 reach it.)
  general LDS    k_aggregate_heads: 2 * (heads * 26 + 26 + 6 + 25 + 16) floats <= 3.9 KiB at 16 heads; k_aggregate_en: static
                 s_w[16][16][3] = 3 KiB holds 16 heads.
  a12            rows of 32 floats: a1 of head h at [h], a2 at [16 + h], h < 16 (ensure_gat_workspace refuses more).
  coefficient    epilogue only for out_dim == 40 on the tile kernels (gemm.hip:896, gemm_sb16.hip); with an odd head count the last
  epilogue       80-wide tile is half filled: attn_l / attn_r are loaded only where nb + 3 < n and written only where head * 40 < n.
  latency route  lat_gat_ok asks lat_gemm_form for every layer >= 1: K stages 13 / 10 / 5 only.  lat4 = 902 -> 10x40, 400 -> 8x40
                 (forms 1, 4), 320 -> 5x30 (2, 5), 150 -> 1 (3, 6 fused): accepted.  odd40 (K = 200: 7 stages), deep8 (80: 3),
                 wide (256: 8), vec1 / vec2 / h16: declined, batch route at every batch size.  `deployed` and lat4 take it up to 16
                 frames, unless a switch of the batch route is set.
No mismatch was found on paper.  One gap was: a last layer other than 1 head x 1 output would run the score mode, where every
column group of a row writes the row's one score; ensure_gat_workspace now refuses it (test_limits_are_errors)."""

import numpy as np
import pytest
import torch

import gat_arch_cases as gc
from conftest import env, oracle, pkg

pytestmark = pytest.mark.gpu

MPE_ERR_INVALID = -1        # include/mpe.h

_engines = {}


def engine(tag, kind='tight'):
    """One engine per architecture: max_frames 96, max_persons_per_camera 5, the tight gains.  kind 'edge': the gain-20 weights
    (weights are frozen after the first batch, so they need a context of their own); 'ppc10': `wide` on the general kernels."""
    key = (tag, kind)
    if key not in _engines:
        e = env('panoptic')
        ppc = 10 if kind == 'ppc10' else gc.PPC
        eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=gc.MAX_FRAMES if kind == 'tight' else 8, max_persons_per_camera=ppc)
        eng.load_gat(*gc.weights(tag, gc.GAIN_EDGE if kind == 'edge' else None))
        _engines[key] = eng
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


_batches = {}


def batch(eng, n, ppc=gc.PPC):
    key = (id(eng), n, ppc)
    if key not in _batches:
        _batches[key] = eng.to_device(eng.pack(gc.frames(n, ppc)))
    return _batches[key]


def _sync(eng):
    eng.sync_status()


def _act(x, last, slope=0.01):
    return x if last else torch.nn.functional.leaky_relu(x, slope)


# ---- (a) the attention stage alone -------------------------------------------------------------------------------------------

def _attention_stage(tag, kind, ppc):
    eng = engine(tag, kind)
    g = gc.graph(gc.N_KINDS, ppc)
    f64 = gc.forward64(tag, gc.N_KINDS, None, ppc)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    db = batch(eng, gc.N_KINDS, ppc)
    assert db.n_heads + db.n_edge_nodes == g.N
    for l in range(f64.L):
        ft2 = f64.ft2[l].float()
        got = eng.edge_softmax_aggregate(db, l, ft2.cuda()).cpu().numpy()
        _sync(eng)
        want = gc.aggregate(sd, l, ft2.double(), g.src, g.dst, prm['alpha'], heads[l])[0].numpy()
        err = gc.metric_agg(got, want)
        print('%s/%s layer %d: (a) %.2e of %.0e' % (tag, kind, l, err, gc.BOUND_AGG))
        assert np.isfinite(got).all()
        assert err <= gc.BOUND_AGG, (tag, l, err)


@pytest.mark.parametrize('tag', gc.TAGS)
def test_attention_stage_vs_f64(tag):
    """(a) mpe_edge_softmax_aggregate, every layer, all six frame kinds in one batch: the f64 oracle's ft2 rounded once to fp32
    in, the f64 aggregation of those rows as reference.  Bound of test_gpu_stages.py: 4e-6 * max(1, |want|max)."""
    _attention_stage(tag, 'tight', gc.PPC)


def test_attention_stage_wide_on_the_general_kernels():
    """(a) for `wide` with 10 persons per camera: 316 160 B of LDS asked, so k_attn_coef + k_aggregate_en / _heads run."""
    _attention_stage('wide', 'ppc10', 10)


# ---- (b) one layer alone -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', gc.TAGS)
def test_single_layers_vs_f64(tag):
    """(b) mpe_gat_layer on the f64 oracle's input rows (rounded to fp32), every layer, layer 0 on dense rows; the last layer
    with activation 2 (logits).  _close(..., 1e-5) of test_gpu_stages.py."""
    onp = oracle()
    eng = engine(tag)
    g = gc.graph(gc.N_KINDS)
    f64 = gc.forward64(tag, gc.N_KINDS)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    db = batch(eng, gc.N_KINDS)
    for l in range(f64.L):
        last = l == f64.L - 1
        x = f64.x[l].float()
        got = eng.gat_layer(db, l, x.cuda(), activation=2 if last else 0).cpu().numpy()
        _sync(eng)
        out = onp.gat_layer(sd, l, x.double(), g.src, g.dst, prm['alpha'], heads[l])[0].reshape(g.N, -1)
        want = _act(out, last, prm['nonlinearity']).numpy()
        err = gc.metric_rel(got, want)
        print('%s layer %d: (b) %.2e of %.0e' % (tag, l, err, gc.BOUND_LAYER))
        assert err <= gc.BOUND_LAYER, (tag, l, err)


# ---- (c) the whole network ---------------------------------------------------------------------------------------------------

def _ulps(a, ref):
    ref32 = ref.astype(np.float32)
    return np.abs(a.astype(np.float64) - ref) / np.spacing(np.abs(ref32)).astype(np.float64)


@pytest.mark.parametrize('tag', gc.TAGS)
def test_whole_network_vs_f64(tag):
    """(c) logits (mpe_set_gat_output 2) through the implicit route and through the dense route, heads included, against the f64
    oracle's pre-sigmoid output: _close(..., 2e-5).  Then the sigmoid back on, and the bits of the default are back; the scores
    are sigmoid(logits) to 1 ulp of fp32 in the kernel's own statement 1 / (1 + expf(-x)): with the exponential anywhere within
    one ulp of its exact value (expf's last bit) and the sum and the quotient rounded once each, the score lies between the two
    fp32 evaluations below, give or take one ulp.  (Against the exactly evaluated sigmoid that is up to 2.5 ulp of the score --
    three roundings; measured 1.72 on `deployed` -- and the kernel cannot do better without changing the deployed bits.)"""
    eng = engine(tag)
    g = gc.graph(gc.N_KINDS)
    f64 = gc.forward64(tag, gc.N_KINDS)
    db = batch(eng, gc.N_KINDS)
    want_en, want_h = f64.logits.numpy()[g.is_en], f64.logits.numpy()[~g.is_en]
    s0, h0 = (t.cpu().numpy() for t in eng.gat_scores(db, heads=True))
    try:
        eng.set_gat_output(False)
        for route, feats in (('implicit', None), ('dense', g.feats.cuda())):
            sc, sh = (t.cpu().numpy() for t in eng.gat_scores(db, heads=True, feats=feats))
            _sync(eng)
            err = max(gc.metric_rel(sc, want_en), gc.metric_rel(sh, want_h))
            print('%s %s route: (c) %.2e of %.0e' % (tag, route, err, gc.BOUND_NET))
            assert err <= gc.BOUND_NET, (tag, route, err)
            if feats is None:
                lg_en, lg_h = sc, sh
    finally:
        eng.set_gat_output(True)
    s1, h1 = (t.cpu().numpy() for t in eng.gat_scores(db, heads=True))
    _sync(eng)
    assert np.array_equal(s1, s0) and np.array_equal(h1, h0)
    one = np.float32(1.0)
    for got, lg in ((s1, lg_en), (h1, lg_h)):
        x = -lg.astype(np.float64)
        u = _ulps(got, 1.0 / (1.0 + np.exp(x)))
        with np.errstate(over='ignore'):
            e = np.exp(x).astype(np.float32)
            lo = one / (one + np.nextafter(e, np.float32(np.inf)))
            hi = one / (one + np.nextafter(e, np.float32(0.0)))
        print('%s sigmoid: %.2f ulp from the exact value' % (tag, float(u.max())))
        assert (got >= np.nextafter(lo, np.float32(0.0))).all() and (got <= np.nextafter(hi, np.float32(2.0))).all(), tag


# ---- (d) logits beyond the overflow of expf ----------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', gc.TAGS)
def test_attention_stage_at_gain_20(tag):
    """(d) gain 20: logits beyond 88.7 (tests/test_gat_archs_host.py).  The output is finite, and |gpu - f64| <= max(4 e_ref,
    4e-6 scale) with e_ref the f32 oracle's own distance from the f64 oracle on the same rows: the kernel may differ from torch by
    expf's last bit and by the summation order, each of the size of torch's own rounding."""
    eng = engine(tag, 'edge')
    g = gc.graph(gc.N_KINDS)
    f64 = gc.forward64(tag, gc.N_KINDS, gc.GAIN_EDGE)
    sd, prm = gc.weights(tag, gc.GAIN_EDGE)
    heads = list(prm['heads']) + [1]
    db = batch(eng, gc.N_KINDS)
    for l in range(f64.L):
        ft2 = f64.ft2[l].float()
        got = eng.edge_softmax_aggregate(db, l, ft2.cuda()).cpu().numpy()
        _sync(eng)
        want = gc.aggregate(sd, l, ft2.double(), g.src, g.dst, prm['alpha'], heads[l])[0].numpy()
        ref32 = gc.aggregate(sd, l, ft2, g.src, g.dst, prm['alpha'], heads[l])[0].numpy()
        e_ref = float(np.abs(ref32 - want).max())
        scale = max(1.0, float(np.abs(want).max()))
        assert np.isfinite(got).all(), (tag, l)
        err = float(np.abs(got - want).max())
        print('%s layer %d gain 20 (logits to %.0f): |gpu - f64| %.2e, e_ref %.2e, 4e-6 scale %.2e'
              % (tag, l, float(f64.e[l].max()), err, e_ref, 4e-6 * scale))
        assert err <= max(4 * e_ref, 4e-6 * scale), (tag, l, err, e_ref)


# ---- (e) same bits on every path ---------------------------------------------------------------------------------------------

def _logits(eng, db):
    sc, sh = eng.gat_scores(db, heads=True)
    return sc.cpu().numpy(), sh.cpu().numpy()


@pytest.mark.parametrize('tag', gc.TAGS)
def test_paths_give_identical_bits(tag, monkeypatch):
    """(e) the switch matrix of test_attention_paths_give_identical_bits on an 8-frame batch: fused / general attention kernels,
    coefficients from the fc2 epilogue / from k_attn_coef, in-edge table / arithmetic, the two forms of the fused kernel's
    phase 3.  No comment in csrc documents a difference between two of these paths for any shape (the one-chain coefficient order
    is the same in row_coef, k_attn_coef and k_gat_fused; 40-wide heads follow coef40 everywhere), so logits and head logits are
    array_equal across all twelve combinations.  For `deployed` and lat4 the default combination runs the latency route and the
    others (MPE_NO_COEF_EPILOGUE) the batch route."""
    eng = engine(tag)
    db = batch(eng, 8)
    res = {}

    def switch(name, on):
        if on:
            monkeypatch.setenv(name, '1')
        else:
            monkeypatch.delenv(name, raising=False)

    try:
        eng.set_gat_output(False)
        for fused in (True, False):
            for epi in (True, False):
                for table in (True, False):
                    for overlap in ((True, False) if fused else (True,)):
                        switch('MPE_NO_FUSED_ATTENTION', not fused)
                        switch('MPE_NO_COEF_EPILOGUE', not epi)
                        switch('MPE_NO_HEAD_SRC_TABLE', not table)
                        switch('MPE_FUSED_NO_OVERLAP', not overlap)
                        res[(fused, epi, table, overlap)] = _logits(eng, db)
        _sync(eng)
    finally:
        eng.set_gat_output(True)
    ref = res[(True, True, True, True)]
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for key, (sc, sh) in res.items():
        assert np.array_equal(sc, ref[0]) and np.array_equal(sh, ref[1]), (tag, key)


# ---- (f) batch invariance ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', gc.TAGS)
def test_batch_invariance(tag, monkeypatch):
    """(f) frame k's logits have the same bits when the frame travels alone, in the 8-frame batch and as frame k of the 96-frame
    batch (k = every frame kind).  The GEMMs go to the tile kernels when ceil(rows / 16) * ceil(n / 16) > 1024: the 96-frame batch
    has 12 816 node rows = 801 row tiles, so every fc1 / fc2 with n >= 17 is a tile launch there (all layers of the architectures
    with hd >= 80: deployed, lat4, odd40, wide, h16, deep8's first; the one-column last fc2 stays on the wave-per-tile kernel at
    any size, by `narrow`), while one frame (at most 276 rows = 18 row tiles) is a wave-per-tile launch up to n = 896.  The
    kernel trace confirms it (profiles/gat_arch_reference_noise.txt, part 4): at 96 frames k_linear_sb / k_linear_dma take 9
    (deployed), 7 (lat4), 5 (odd40), 3 (wide), 4 (h16) and 12 (deep8) of the GEMM launches, at 8 frames none or one.  No comment
    in csrc documents a bit difference between the two for any shape.  lat4: MPE_LATENCY_PATH=0 against the default as well."""
    eng = engine(tag)
    try:
        eng.set_gat_output(False)
        big, small = batch(eng, gc.MAX_FRAMES), batch(eng, 8)
        sc96, sh96 = _logits(eng, big)
        sc8, sh8 = _logits(eng, small)
        for k in range(gc.N_KINDS):
            one = eng.to_device(eng.pack([gc.frames(8)[k]]))
            sc1, sh1 = _logits(eng, one)
            for db, sc, sh in ((small, sc8, sh8), (big, sc96, sh96)):
                h0, H, e0, M = db.host.frame_counts(k)
                assert np.array_equal(sc[e0:e0 + M], sc1) and np.array_equal(sh[h0:h0 + H], sh1), (tag, k, db.n_frames)
        if tag == 'lat4':
            monkeypatch.setenv('MPE_LATENCY_PATH', '0')
            sc8b, sh8b = _logits(eng, small)
            assert np.array_equal(sc8b, sc8) and np.array_equal(sh8b, sh8)
            eng.set_gat_output(True)
            _, p_batch, n_batch = eng.match(small)
            monkeypatch.delenv('MPE_LATENCY_PATH')
            _, p_lat, n_lat = eng.match(small)
            assert torch.equal(n_batch, n_lat) and torch.equal(p_batch, p_lat)
        _sync(eng)
    finally:
        eng.set_gat_output(True)


# ---- (g) decisions -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['odd40', 'lat4', 'deployed'])
def test_decisions_follow_the_gpu_scores(tag):
    """(g) mpe_match_batch: the persons equal oracle_np.cluster run on the GPU's own scores (exact integer logic; sigmoid on,
    threshold 0.5), frame by frame."""
    onp = oracle()
    e = env('panoptic')
    eng = engine(tag)
    g = gc.graph(gc.N_KINDS)
    db = batch(eng, gc.N_KINDS)
    scores, persons, n_persons = eng.match(db)
    _sync(eng)
    scores, persons, n_persons = scores.cpu().numpy(), persons.cpu().numpy(), n_persons.cpu().numpy()
    sm = list(e.params.used_cameras_skeleton_matching)
    some = 0
    for f, gr in enumerate(g.per_frame):
        h0, H, e0, M = db.host.frame_counts(f)
        head_cam = [sm.index(c) for c in gr['nodes_camera'][:H]]
        own = onp.cluster(scores[e0:e0 + M], gr['pairs'], H, head_cam, len(sm))
        k = min(len(own), eng.pcap)
        assert int(n_persons[f]) == k, (tag, f)
        assert np.array_equal(persons[f, :k], np.array(own, np.int32).reshape(-1, len(sm))[:k]), (tag, f)
        some += k
    assert some > 0


# ---- (i) limits are errors, not launches -------------------------------------------------------------------------------------

def test_limits_are_errors():
    """(i) 17 attention heads, and a last layer that is not 1 head x 1 output, come back as MPE_ERR_INVALID from the first batch
    call (ensure_gat_workspace checks both before it allocates or launches anything); 1 and 9 layers are refused by
    mpe_set_gat_params.  The context stays usable: the deployed-shape weights load and run afterwards."""
    L = pkg('lib')
    syn = pkg('synthetic')
    e = env('panoptic')
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=2, max_persons_per_camera=gc.PPC)
    try:
        db = eng.to_device(eng.pack(gc.frames(1)))
        for n_layers in (1, 9):
            assert eng.lib.mpe_set_gat_params(eng.ctx, n_layers, 0.15, 0.01) == MPE_ERR_INVALID
        nf = e.meta['num_feats']
        eng.load_gat(syn.gat_state_dict(3, nf, [4], [17]), syn.gat_params(nf, [4], [17]))
        with pytest.raises(L.MpeError) as err:
            eng.gat_scores(db)
        assert err.value.code == MPE_ERR_INVALID and '16 attention heads' in str(err.value)
        sd = dict(syn.gat_state_dict(3, nf, [4], [2]))
        sd['layers.1.fc2.weight'] = np.concatenate([sd['layers.1.fc2.weight']] * 2)
        sd['layers.1.fc2.bias'] = np.concatenate([sd['layers.1.fc2.bias']] * 2)
        sd['layers.1.attn_l'] = np.concatenate([sd['layers.1.attn_l']] * 2, axis=1)
        sd['layers.1.attn_r'] = np.concatenate([sd['layers.1.attn_r']] * 2, axis=1)
        eng.load_gat(sd, syn.gat_params(nf, [4], [2]))
        assert eng.gat_dims[-1][1:] == (1, 2)
        for call in (lambda: eng.gat_scores(db), lambda: eng.match(db)):
            with pytest.raises(L.MpeError) as err:
                call()
            assert err.value.code == MPE_ERR_INVALID and 'last GAT layer' in str(err.value)
        eng.load_gat(*gc.weights('deployed'))
        assert np.isfinite(eng.gat_scores(db).cpu().numpy()).all()
        eng.sync_status()
    finally:
        eng.close()


# ---- (h) fp16 rows -----------------------------------------------------------------------------------------------------------

_h_cases = {}


def _h_case(tag, which):
    """(graph, f64 forward, frames) of the batches of (h): 'six' = one frame of every kind; 'one' = the frame with 5 persons
    per camera alone (276 rows: every GEMM a wave-per-tile launch); 'many' = 24 frames (3204 rows = 201 row tiles: every fc2 of
    n >= 96 a tile launch, ceil(rows / 16) * ceil(n / 16) > 1024)."""
    if (tag, which) not in _h_cases:
        fr = {'six': gc.frames(6), 'one': [gc.frames(6)[5]], 'many': gc.frames(24)}[which]
        g = gc.Graph(fr)
        _h_cases[(tag, which)] = (g, gc.Forward(tag, g), fr)
    return _h_cases[(tag, which)]


@pytest.mark.parametrize('tag,split,which', [('h16', True, 'six'), ('vec2', True, 'six'), ('vec1', True, 'six'),
                                             ('deployed', True, 'one'), ('deployed', True, 'many'),
                                             ('h16', False, 'six'), ('deployed', False, 'many')])
def test_fp16_rows_vs_f64(tag, split, which):
    """(h) set_precision(attn_fp16=True): mpe_gat_layer of the layers >= 1 against the f64 oracle with ft2 rounded to fp16 before
    the weighted sum (gat_arch_cases.fp16_rows_statement), _close(..., 1e-5) -- plus, for the outputs fed by an ft2 element
    whose exact value lies at a tie between two fp16 values, what one fp16 spacing can move (the statement's `slack`: without it
    the f32 oracle itself, given fp16 rows, misses 1e-5 in hundreds of outputs by up to 95 x; tests/test_gat_archs_host.py).
    Which coefficients (api.hip: gat_layer_linear): the fc2 launch leaves a1 | a2 of the fp32 values in a12 only where it has a
    coefficient epilogue -- out_dim == 40 on a tile kernel (gemm.hip:896, gemm_sb16.hip), in both GEMM forms (gat_split or
    not) -- and `a12_ready` is 0 otherwise: the fused kernel then computes them from its image of the fp16 rows, the general
    path by k_attn_coef(ft_half).  So: fp16-row coefficients everywhere, except the 40-wide layers 1 and 2 of `deployed` in the
    24-frame batch.  Restoring the default restores its bits."""
    eng = engine(tag)
    g, f64, fr = _h_case(tag, which)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    db = eng.to_device(eng.pack(fr))
    dims = gc.dims(tag)
    x1 = f64.x[1].float().cuda()
    before = eng.gat_layer(db, 1, x1, activation=0).cpu().numpy()
    try:
        eng.set_precision(False, False, attn_fp16=True, gat_split=split)
        for l in range(1, f64.L):
            x = f64.x[l].float()
            got = eng.gat_layer(db, l, x.cuda(), activation=0).cpu().numpy().astype(np.float64)
            _sync(eng)
            epilogue = dims[l][2] == 40 and which == 'many'
            res = {}
            for coef_fp16 in (True, False):
                want, slack = gc.fp16_rows_statement(sd, l, x, g, prm['alpha'], heads[l], coef_fp16)
                want = np.where(want > 0, want, want * prm['nonlinearity'])
                bound = gc.BOUND_LAYER * np.maximum(1.0, np.abs(want))
                err = np.abs(got - want)
                res[coef_fp16] = (int((err > bound + slack).sum()), float((err / bound).max()), float((slack == 0).mean()),
                                  float((err[slack == 0] / bound[slack == 0]).max()) if (slack == 0).any() else 0.0)
            mine, other = res[not epilogue], res[epilogue]
            print('%s split=%s %s layer %d (%s coefficients): %d outputs beyond bound + slack, worst %.1f x the bound; %.0f %% of the outputs '
                  'carry no slack, worst of them %.2f x; the other statement: %d beyond'
                  % (tag, split, which, l, 'fp32' if epilogue else 'fp16', mine[0], mine[1], 100 * mine[2], mine[3], other[0]))
            assert np.isfinite(got).all()
            assert mine[0] == 0, (tag, l, mine)
    finally:
        eng.set_precision(False, False)
    after = eng.gat_layer(db, 1, x1, activation=0).cpu().numpy()
    _sync(eng)
    assert np.array_equal(after, before)
