"""CPU side of the GAT architecture cases (tests/gat_arch_cases.py): the weights' knobs, the frames, the conditioning of every
comparison that tests/test_gpu_gat_archs.py makes, and what a wrong kernel would cost against those bounds."""
import numpy as np
import pytest
import torch

import gat_arch_cases as gc
from conftest import env, oracle, pkg


@pytest.mark.parametrize('tag', gc.TAGS)
def test_gat_params_count_the_layers(tag):
    syn = pkg('synthetic')
    hidden, heads = gc.ARCHS[tag]
    prm = syn.gat_params(902, hidden, heads)
    want = len(hidden if hidden is not None else syn.GAT_HIDDEN) + 1
    assert prm['gnn_layers'] == want == len(gc.dims(tag))
    assert len(prm['heads']) == len(prm['num_hidden']) == want - 1
    assert 2 <= want <= 8


def test_gat_params_default_is_unchanged():
    syn = pkg('synthetic')
    prm = syn.gat_params(902)
    assert prm['gnn_layers'] == syn.GAT_LAYERS == 5
    assert prm == env('panoptic').gat[1]
    assert syn.gat_params(902, hidden=[8], heads=[2])['gnn_layers'] == 2


def test_attn_gain_default_leaves_every_fixture_bit():
    syn = pkg('synthetic')
    m = env('panoptic').meta
    fixture = env('panoptic').gat[0]
    for gain in (None, 1.0, [1.0] * 5):
        kw = {} if gain is None else {'attn_gain': gain}
        sd = syn.gat_state_dict(m['gat_seed'], m['num_feats'], logit_gain=m['logit_gain'], logit_shift=m['logit_shift'], **kw)
        assert sorted(sd) == sorted(fixture)
        for k in sd:
            assert sd[k].dtype == fixture[k].dtype and np.array_equal(sd[k].view(np.uint32), fixture[k].view(np.uint32)), k
    sd4 = syn.gat_state_dict(m['gat_seed'], m['num_feats'], logit_gain=m['logit_gain'], logit_shift=m['logit_shift'], attn_gain=4.0)
    per_layer = syn.gat_state_dict(m['gat_seed'], m['num_feats'], logit_gain=m['logit_gain'], logit_shift=m['logit_shift'],
                                   attn_gain=[4.0, 1.0, 1.0, 1.0, 4.0])
    for k in sd4:
        if 'attn' in k:
            assert np.array_equal(sd4[k], fixture[k] * np.float32(4.0))
            assert np.array_equal(per_layer[k], sd4[k] if k.split('.')[1] in '04' else fixture[k])
        else:
            assert np.array_equal(sd4[k], fixture[k]) and np.array_equal(per_layer[k], fixture[k])
    with pytest.raises(ValueError):
        syn.gat_state_dict(m['gat_seed'], m['num_feats'], attn_gain=[1.0, 2.0])


def test_frame_kinds():
    """The smallest graph and the in-degree cap are really among the frames, and frame k is the same frame in every batch."""
    g = gc.graph(gc.N_KINDS)
    V = 5
    assert g.H[4] == 2 and g.M[4] == 1                                   # one person in two views
    assert g.H[5] == V * gc.PPC                                          # every camera holds max_persons_per_camera skeletons
    deg = g.in_degree()
    heads_of_cap = deg[g.frame_rows(5)][:g.H[5]]
    assert heads_of_cap.max() == 1 + (V - 1) * gc.PPC == heads_of_cap.min()      # self loop + every head of the other cameras
    assert (deg[g.is_en] == 3).all()
    assert max(g.H) <= V * gc.PPC
    assert g.H[2] < 2 * V and len(g.per_frame[3]['slots']) == 3          # an empty camera; three cameras
    assert gc.frames(8)[:6] == gc.frames(6) and gc.frames(8)[3] is gc.frames(gc.N_KINDS)[3]


@pytest.mark.parametrize('tag', ['deployed', 'vec2', 'h16'])
def test_aggregate_restates_gat_layer(tag):
    """gat_arch_cases.aggregate on the layer's own ft2 gives the bits of oracle_np.gat_layer, in both precisions."""
    onp = oracle()
    g = gc.graph(gc.N_KINDS)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    for dtype in (torch.float32, torch.float64):
        h = g.feats.to(dtype)
        for l in range(prm['gnn_layers']):
            out, aux = onp.gat_layer(sd, l, h, g.src, g.dst, prm['alpha'], heads[l])
            mine = gc.aggregate(sd, l, aux['ft2'].reshape(g.N, -1), g.src, g.dst, prm['alpha'], heads[l])[0]
            assert torch.equal(mine, out.reshape(g.N, -1)), (dtype, l)
            h = torch.nn.functional.leaky_relu(out.flatten(1), prm.get('nonlinearity', 0.01))


_noise = {}


def _noise_of(tag):
    if tag not in _noise:
        _noise[tag] = gc.reference_noise(tag)
    return _noise[tag]


@pytest.mark.parametrize('tag', gc.TAGS)
def test_reference_noise_is_a_quarter_of_every_bound(tag):
    """Conditioning: on identical rows the f32 oracle sits at most a quarter of the GPU test's bound from the f64 oracle, per
    layer in the metrics of (a) and (b) and for the whole network in that of (c).  Where it did not at attention gain 4 /
    logit gain 25, gat_arch_cases lowers the gain (tight_gains, LOGIT_GAIN); no bound is widened.  Layer 0 in (b) and (c) is
    measured on the oracle with f64 running sums in its GEMMs (gat_arch_cases.layer_f64_sums): that is how the library
    computes that layer, and torch's plain fp32 GEMM over K = 902 alone takes 0.1-0.14 of (b)'s bound before any attention --
    with it no gain keeps both this check and a logit spread of one unit (measured: 0.20-0.33 of the bound at spreads of
    1.1-1.4).  The table (both figures) is profiles/gat_arch_reference_noise.txt."""
    rows, net = _noise_of(tag)
    for l, r in enumerate(rows):
        print('%s layer %d: (a) %.2e (b) %.2e (plain f32 %.2e)' % (tag, l, r['e_agg'], r['e_layer'], r['e_layer_f32']))
        assert r['e_agg'] <= gc.BOUND_AGG / 4, (tag, l, r)
        assert r['e_layer'] <= gc.BOUND_LAYER / 4, (tag, l, r)
        if l > 0:
            assert r['e_layer'] == r['e_layer_f32']
    print('%s network: (c) %.2e (plain f32 %.2e)' % (tag, net['e_net'], net['e_net_f32']))
    assert net['e_net'] <= gc.BOUND_NET / 4, (tag, net)


@pytest.mark.parametrize('tag', gc.TAGS)
def test_no_softmax_is_near_uniform(tag):
    """The attention logits of every hidden layer have a standard deviation within [1, 8] at the tight gains."""
    rows, _ = _noise_of(tag)
    for l, r in enumerate(rows[:-1]):
        assert 1.0 <= r['std'] <= 8.0, (tag, l, r['std'])


@pytest.mark.parametrize('tag', gc.TAGS)
def test_edge_gain_crosses_the_overflow_of_expf(tag):
    """Gain 20: some layer's logits pass 88.7, where expf overflows in fp32 unless the maximum is subtracted first; the f64
    oracle stays finite."""
    f = gc.forward64(tag, gc.N_KINDS, gc.GAIN_EDGE)
    top = [float(e.max()) for e in f.e]
    assert max(top) > gc.EXPF_OVERFLOW, (tag, top)
    assert all(bool(torch.isfinite(a).all()) for a in f.agg)
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(np.float32(max(top))))


def _wrong_vs_bounds(tag, l, wrong_fn):
    """metric (a) of a wrong aggregation of layer l against the f64 statement, on the f64 oracle's ft2 rounded to fp32."""
    g = gc.graph(gc.N_KINDS)
    f64 = gc.forward64(tag, gc.N_KINDS)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    ft2 = f64.ft2[l].float().double()
    want, _, a = gc.aggregate(sd, l, ft2, g.src, g.dst, prm['alpha'], heads[l])
    return gc.metric_agg(wrong_fn(sd, prm, heads[l], ft2, a, g), want)


def test_wrong_variants_would_miss_the_bounds():
    """Evidence that the tests bite, computed with the numpy / torch statement (no broken kernel is built):
    vec2   the edge-node kernel's 16-byte column groups straddle the 6- and 10-wide heads; a kernel that took the group's FIRST
           head for all four columns (`hk = hh`) would miss (a)'s bound by four orders of magnitude in both hidden layers;
    odd40  layer 0 has five 40-wide heads, so the last 80-wide tile of the coefficient epilogue holds ONE head; a kernel that took
           the neighbouring head's attention vector there misses the bound by five orders.
    A wrong head PARITY in coef40 is no mistake at all: parity 1 runs the same four chains as parity 0 in the places (2, 3, 0, 1),
    and (s0 + s1) + (s2 + s3) does not care -- the coefficient has the same bits (asserted below), so no test can see it."""
    def first_head_of_group(sd, prm, nh, ft2, a, g):
        hd = ft2.shape[1]
        od = hd // nh
        col_head = torch.tensor([(4 * (c // 4)) // od for c in range(hd)])
        s, d = torch.from_numpy(g.src).long(), torch.from_numpy(g.dst).long()
        return torch.zeros_like(ft2).index_add_(0, d, ft2[s] * a[:, col_head])

    for l in (0, 1):
        err = _wrong_vs_bounds('vec2', l, first_head_of_group)
        print('vec2 layer %d, hk = hh: %.2e = %.0f x the bound of (a)' % (l, err, err / gc.BOUND_AGG))
        assert err > 1e3 * gc.BOUND_AGG

    def neighbour_head_vector(sd, prm, nh, ft2, a, g):
        bad = dict(sd)
        for k in ('layers.0.attn_l', 'layers.0.attn_r'):
            v = np.array(sd[k])
            v[nh - 1] = v[nh - 2]
            bad[k] = v
        return gc.aggregate(bad, 0, ft2, g.src, g.dst, prm['alpha'], nh)[0]

    err = _wrong_vs_bounds('odd40', 0, neighbour_head_vector)
    print('odd40 layer 0, single-head tile with the neighbour\'s vector: %.2e = %.0f x the bound of (a)' % (err, err / gc.BOUND_AGG))
    assert err > 1e3 * gc.BOUND_AGG

    # parity: the two forms of coef40 (csrc/gat.hip) on the same fp32 rows
    sd, prm = gc.weights('odd40')
    ft = gc.forward64('odd40', gc.N_KINDS).ft2[0].float().numpy().reshape(-1, 5, 40)[:, 4]
    al = np.asarray(sd['layers.0.attn_l'], np.float32).reshape(5, 40)[4]

    def chains(parity):
        tot = []
        for q in range(4):
            if parity == 0:
                idx = [16 * t + 4 * q + i for t in range(2) for i in range(4)] + ([32 + 4 * q + i for i in range(4)] if q < 2 else [])
            else:
                idx = ([4 * q - 8 + i for i in range(4)] if q >= 2 else []) + [8 + 4 * q + i for i in range(4)] + [24 + 4 * q + i for i in range(4)]
            x = np.zeros(len(ft), np.float32)
            for d in idx:
                x = (x + ft[:, d] * al[d]).astype(np.float32)
            tot.append(x)
        return (tot[0] + tot[1]) + (tot[2] + tot[3])

    a_even, a_odd = chains(0), chains(1)
    diff = float(np.abs(a_even - a_odd).max())
    print('odd40 layer 0, head 4 with the wrong parity: coefficients move by %.1e (|a1| <= %.1f)' % (diff, float(np.abs(a_even).max())))
    assert diff == 0.0 and np.abs(a_even).max() > 1


@pytest.mark.parametrize('tag', ['h16', 'vec2'])
def test_fp16_rows_statement_holds_for_an_fp32_implementation(tag):
    """The statement of (h), tried on an implementation that is right by construction: the f32 oracle's own ft2, rounded to fp16,
    through the fp32 graph half.  It sits inside 1e-5 + slack everywhere, with either source of the coefficients -- and NOT inside
    1e-5 alone (h16 layer 1: hundreds of outputs, up to 40 x the bound): an ft2 element at a tie between two fp16 values lands on
    either side depending on the last bit of the fp32 GEMM, and one fp16 spacing is 1e-3 of the value."""
    onp = oracle()
    g = gc.graph(gc.N_KINDS)
    sd, prm = gc.weights(tag)
    heads = list(prm['heads']) + [1]
    f64 = gc.forward64(tag, gc.N_KINDS)
    naive = 0
    for l in range(1, f64.L):
        x = f64.x[l].float()
        ft32 = onp.gat_layer(sd, l, x, g.src, g.dst, prm['alpha'], heads[l])[1]['ft2'].reshape(g.N, -1)
        for coef_fp16 in (True, False):
            if coef_fp16:
                got = gc.aggregate(sd, l, ft32.half().float(), g.src, g.dst, prm['alpha'], heads[l])[0].numpy()
            else:
                got = gc.aggregate(sd, l, ft32, g.src, g.dst, prm['alpha'], heads[l], fp16_sum=True)[0].numpy()
            want, slack = gc.fp16_rows_statement(sd, l, x, g, prm['alpha'], heads[l], coef_fp16)
            err, bound = np.abs(got - want), gc.BOUND_LAYER * np.maximum(1.0, np.abs(want))
            assert (err <= bound + slack).all(), (tag, l, coef_fp16)
            naive += int((err > bound).sum())
            if not coef_fp16:
                assert (slack == 0).mean() > 0.5                   # most outputs keep the bound alone
    assert naive > 0
