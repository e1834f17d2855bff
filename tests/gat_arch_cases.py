"""GAT2 architectures other than the deployed one, as test cases (numpy / torch only, importable without a GPU).

include/mpe.h takes any GAT2 of 2..8 layers and up to 16 attention heads; the kernels are specialised for hidden
[40,40,40,30] x heads [10,10,8,5] and send every other shape down a fallback branch.  ARCHS lists networks that reach those
branches (the tag is the test id), all on the PANOPTIC rig (F = 902).  Weights come from synthetic.gat_state_dict with the
fixtures' seed and shift, their logit gain unless LOGIT_GAIN says otherwise, and with `attn_gain`:

  GAIN_TIGHT (4)   attention logits with a standard deviation of a few units: the softmax over a node's in-edges is far from
                   uniform and not one-hot, so a wrong coefficient moves the output by orders of magnitude more than fp32 noise;
  GAIN_EDGE (20)   logits beyond expf's fp32 overflow (88.7): finite only if the maximum is subtracted before the exponential.

The reference of every comparison is oracle_np.gat_layer in float64 (the same network without fp32 rounding); `aggregate`
restates its graph half (a1/a2, edge softmax, weighted sum) for ft2 rows given by the caller, line for line, and
tests/test_gat_archs_host.py pins the restatement to gat_layer bit for bit."""
import numpy as np
import torch

from conftest import env, oracle, pkg

# tag -> (hidden, heads); None = the deployed network (synthetic.GAT_HIDDEN / GAT_HEADS)
ARCHS = {
    'deployed': (None, None),
    'odd40': ([40, 40], [5, 1]),
    'vec1': ([7, 5], [3, 2]),
    'vec2': ([6, 10], [5, 3]),
    'h16': ([8, 12], [16, 16]),
    'wide': ([64], [4]),
    'deep8': ([40, 24, 17, 9, 4, 12, 30], [2, 3, 1, 7, 2, 4, 5]),
    'lat4': ([40, 40, 30], [10, 8, 5]),
}
TAGS = list(ARCHS)
GAIN_TIGHT = 4.0
GAIN_EDGE = 20.0
# Where gain 4 / logit gain 25 left the f32 oracle more than a quarter of a bound from the f64 oracle, the gain is lowered, as far as
# the other check allows (a logit spread of at least one unit in every hidden layer); measured figures: profiles/gat_arch_reference_noise.txt.
#   layer 0: its logits carry a common offset of 10+ units, so one ulp of a logit is 1e-6 -- a quarter of (a)'s bound at gain 4,
#            0.27-0.36 of it even at gain 2 where the spread is 1.4-2.0.  1.5 keeps both checks for six architectures; for vec1 and
#            h16 the worst-case figure jumps between 0.13 and 0.41 from one gain to the next (it is the extreme of 10^5 outputs),
#            and the values below are those of a sweep over 1.0 .. 1.9 that pass both with the widest margin.
#   odd40 layer 1 (one 40-wide head over K = 200): 0.33 of (b)'s bound at gain 4, 0.21 at 2.5.
#   deep8 layer 5 (4 x 12 on rows that have shrunk to 0.7): a spread of 0.2 at gain 4; 24 gives 1.2.  (The one gain that is raised.)
#   logit gain: the last fc2 multiplies the f32 oracle's error with the logits -- 0.69 / 0.83 / 0.43 of (b)'s bound and 1.46 / 0.77 /
#            0.66 of (c)'s at 25 for deployed / odd40 / wide, under 0.25 at the values below.  The other five keep 25.
GAIN_LAYER0 = 1.5
OVERRIDE_GAIN = {('vec1', 0): 1.1, ('h16', 0): 1.75, ('odd40', 1): 2.5, ('deep8', 5): 24.0}      # (tag, layer) -> gain
LOGIT_GAIN = {'deployed': 3.0, 'odd40': 4.0, 'wide': 2.5}                                         # tag -> logit gain
MAX_FRAMES = 96
PPC = 5                     # max_persons_per_camera of the engines
EXPF_OVERFLOW = 88.7        # expf(x) = inf in fp32 beyond this

# the bounds of tests/test_gpu_gat_archs.py, each in its own metric (see the functions below)
BOUND_AGG = 4e-6            # (a) |got - want|max <= BOUND_AGG * max(1, |want|max)           (test_gpu_stages.py: edge_softmax_aggregate)
BOUND_LAYER = 1e-5          # (b) max |got - want| / max(1, |want|) <= BOUND_LAYER            (test_gpu_stages.py: isolated layer)
BOUND_NET = 2e-5            # (c) the same metric on the whole network's logits


def metric_agg(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))


def metric_rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def dims(tag):
    hidden, heads = ARCHS[tag]
    return pkg('synthetic').gat_layer_dims(env('panoptic').meta['num_feats'], hidden, heads)


def logit_gain(tag):
    return float(LOGIT_GAIN.get(tag, env('panoptic').meta['logit_gain']))


def tight_gains(tag):
    """Attention gain per layer of the tight comparisons: GAIN_TIGHT in the hidden layers, GAIN_LAYER0 in layer 0, and
    GAIN_TIGHT / logit_gain in the last layer, whose rows carry the logit gain (its attention logits then spread like a hidden
    layer's instead of 25 times wider); OVERRIDE_GAIN on top.  Why: the comment at GAIN_LAYER0."""
    L = len(dims(tag))
    g = [GAIN_LAYER0] + [GAIN_TIGHT] * (L - 2) + [GAIN_TIGHT / logit_gain(tag)]
    for (t, l), v in OVERRIDE_GAIN.items():
        if t == tag:
            g[l] = v
    return tuple(g)


_weights = {}


def weights(tag, attn_gain=None):
    """(state dict, prm) of architecture `tag`; attn_gain None = the architecture's tight gain."""
    g = tight_gains(tag) if attn_gain is None else attn_gain
    g = float(g) if np.isscalar(g) else tuple(float(x) for x in g)
    if (tag, g) not in _weights:
        syn = pkg('synthetic')
        m = env('panoptic').meta
        hidden, heads = ARCHS[tag]
        sd = syn.gat_state_dict(m['gat_seed'], m['num_feats'], hidden, heads, logit_gain=logit_gain(tag),
                                logit_shift=m['logit_shift'], attn_gain=g)
        _weights[(tag, g)] = (sd, syn.gat_params(m['num_feats'], hidden, heads))
    return _weights[(tag, g)]


def frame_specs(ppc=PPC):
    """The six frame kinds: the four of test_attention_paths_give_identical_bits, the smallest graph (one person in two views:
    two heads, one edge-node) and a frame whose cameras all hold `ppc` skeletons (head in-degree at its cap)."""
    syn = pkg('synthetic')
    return [syn.FrameSpec(persons=4), syn.FrameSpec(persons=5, joint_drop=0.2),
            syn.FrameSpec(persons=2, empty_cameras=('trackerb',)),
            syn.FrameSpec(persons=3, cameras=['trackerd', 'trackera', 'trackere']),
            syn.FrameSpec(persons=1, cameras=['trackerc', 'trackera']),
            syn.FrameSpec(persons=ppc)]


N_KINDS = 6
_frames = {}


def frames(n, ppc=PPC, start=7000):
    """n frames, kind i % 6 at position i (processed_input form); frames(8)[k] is frames(96)[k]."""
    key = (ppc, start)
    have = _frames.setdefault(key, [])
    if len(have) < n:
        onp, syn, calib = oracle(), pkg('synthetic'), env('panoptic').calib
        specs = frame_specs(ppc)
        for i in range(len(have), n):
            have.append(onp.processed_input(syn.make_frame(calib, start + i, specs[i % N_KINDS])[0]))
    return have[:n]


class Graph:
    """The batch graph of a list of frames in the node order of include/mpe.h (frame by frame: heads, then edge-nodes)."""

    def __init__(self, frame_list):
        onp, calib = oracle(), env('panoptic').calib
        feats, src, dst, self.node_off, self.H, self.M, self.per_frame = [], [], [], [0], [], [], []
        for fr in frame_list:
            g = onp.build_graph(fr, calib)
            assert g is not None, 'every case frame has a graph'
            o = self.node_off[-1]
            feats.append(g['feats'])
            src.append(g['src'].astype(np.int64) + o)
            dst.append(g['dst'].astype(np.int64) + o)
            self.H.append(g['H'])
            self.M.append(g['N'] - g['H'])
            self.node_off.append(o + g['N'])
            self.per_frame.append(g)
        self.feats = torch.cat(feats)                              # [N, F] float32
        self.src, self.dst = np.concatenate(src), np.concatenate(dst)
        self.N = self.node_off[-1]
        is_en = np.zeros(self.N, bool)
        for f in range(len(frame_list)):
            is_en[self.node_off[f] + self.H[f]:self.node_off[f + 1]] = True
        self.is_en = is_en

    def frame_rows(self, f):
        return slice(self.node_off[f], self.node_off[f + 1])

    def in_degree(self):
        return np.bincount(self.dst, minlength=self.N)


_graphs = {}


def graph(n, ppc=PPC):
    if (n, ppc) not in _graphs:
        _graphs[(n, ppc)] = Graph(frames(n, ppc))
    return _graphs[(n, ppc)]


def aggregate(sd, l, ft2, src, dst, alpha, num_heads, fp16_sum=False):
    """The graph half of oracle_np.gat_layer on given ft2 rows [N, heads * out_dim], in the dtype of ft2 -> (out [N, hd], e, a):
    the lines of gat_layer after fc2, unchanged; `e` = the attention logits per edge [E, heads], `a` their softmax.
    fp16_sum: the rows that enter the weighted sum are rounded to fp16 first (the coefficients still come from ft2 as given)."""
    N, dt = ft2.shape[0], ft2.dtype
    p = 'layers.%d.' % l
    ft2 = ft2.reshape(N, num_heads, -1)
    head_ft = ft2.transpose(0, 1)
    a1 = torch.bmm(head_ft, torch.from_numpy(np.ascontiguousarray(sd[p + 'attn_l'])).to(dt)).transpose(0, 1)
    a2 = torch.bmm(head_ft, torch.from_numpy(np.ascontiguousarray(sd[p + 'attn_r'])).to(dt)).transpose(0, 1)
    s = torch.from_numpy(np.asarray(src)).long()
    d = torch.from_numpy(np.asarray(dst)).long()
    e = torch.nn.functional.leaky_relu(a1[s] + a2[d], alpha)
    idx = d.view(-1, 1, 1).expand_as(e)
    mx = torch.full((N, num_heads, 1), float('-inf'), dtype=dt).scatter_reduce(0, idx, e, reduce='amax', include_self=True)
    score = torch.exp(e - mx[d])
    ssum = torch.zeros((N, num_heads, 1), dtype=dt).index_add_(0, d, score)
    a = score / ssum[d]
    rows = ft2.half().to(dt) if fp16_sum else ft2
    out = torch.zeros_like(ft2).index_add_(0, d, rows[s] * a)
    return out.reshape(N, -1), e.reshape(len(s), num_heads), a.reshape(len(s), num_heads)


def layer_f64_sums(sd, l, x32, src, dst, alpha, num_heads):
    """A layer as an fp32 implementation WITH f64 RUNNING SUMS in its two GEMMs computes it: fc1 and fc2 in float64 on the fp32
    rows, each rounded once to fp32, the graph half in fp32.  The library runs layer 0 this way (csrc/gemm_form.h: K > 512), and
    the f32 oracle does not: torch's fp32 GEMM over K = 902 alone sits 1e-6 from the f64 network.  -> (out [N, hd], ft2)."""
    p = 'layers.%d.' % l

    def w(name):
        return torch.from_numpy(np.ascontiguousarray(sd[p + name])).double()
    ft1 = torch.nn.functional.linear(x32.double(), w('fc1.weight'), w('fc1.bias')).float()
    h2 = torch.nn.functional.leaky_relu(ft1, alpha)
    ft2 = torch.nn.functional.linear(h2.double(), w('fc2.weight'), w('fc2.bias')).float()
    return aggregate(sd, l, ft2, src, dst, alpha, num_heads)[0], ft2


class Forward:
    """Architecture `tag` on graph `g` through oracle_np.gat_layer in `dtype`, layer by layer: x[l] the input rows of layer l,
    ft2[l], agg[l] (the layer's output before the activation of GAT2.forward), e[l] the attention logits; `logits` = agg[L-1].
    l0_f64_sums (with float32): layer 0 through layer_f64_sums, as the library computes it."""

    def __init__(self, tag, g, attn_gain=None, dtype=torch.float64, l0_f64_sums=False):
        onp = oracle()
        sd, prm = weights(tag, attn_gain)
        heads = list(prm['heads']) + [1]
        self.L = prm['gnn_layers']
        self.x, self.ft2, self.agg, self.e = [], [], [], []
        h = g.feats.to(dtype)
        for l in range(self.L):
            self.x.append(h)
            if l == 0 and l0_f64_sums:
                out, ft2 = layer_f64_sums(sd, l, h, g.src, g.dst, prm['alpha'], heads[l])
                aux = {'ft2': ft2}
            else:
                out, aux = onp.gat_layer(sd, l, h, g.src, g.dst, prm['alpha'], heads[l])
            ft2 = aux['ft2'].reshape(g.N, -1)
            self.ft2.append(ft2)
            self.agg.append(out.reshape(g.N, -1))
            self.e.append(aggregate(sd, l, ft2, g.src, g.dst, prm['alpha'], heads[l])[1])
            h = torch.nn.functional.leaky_relu(out.flatten(1), prm.get('nonlinearity', 0.01))
        self.logits = self.agg[-1].reshape(-1)


_forwards = {}


def forward64(tag, n, attn_gain=None, ppc=PPC):
    """The float64 oracle of `tag` on graph(n), computed once and shared (read-only)."""
    key = (tag, n, attn_gain if attn_gain is None or np.isscalar(attn_gain) else tuple(attn_gain), ppc)
    if key not in _forwards:
        _forwards[key] = Forward(tag, graph(n, ppc), attn_gain)
    return _forwards[key]


N_NOISE = N_KINDS           # frames of the conditioning check: one of every kind


def reference_noise(tag):
    """The f32 oracle's own distance from the f64 oracle, per layer and for the whole network, at the tight gains, in the metrics
    of the GPU tests -> (rows, net).  rows[l] = dict(std, max: the attention logits of layer l; e_agg: metric (a) on the f64
    oracle's ft2 rounded to fp32; e_layer: metric (b) on the f64 oracle's input rows rounded to fp32; e_layer_f32: the same for
    the plain f32 oracle where e_layer is layer_f64_sums (layer 0)); net = dict(e_net, e_net_f32) in metric (c)."""
    onp = oracle()
    g = graph(N_NOISE)
    f64 = forward64(tag, N_NOISE)
    sd, prm = weights(tag)
    heads = list(prm['heads']) + [1]
    rows = []
    for l in range(f64.L):
        x32 = f64.x[l].float()
        want = onp.gat_layer(sd, l, x32.double(), g.src, g.dst, prm['alpha'], heads[l])[0].reshape(g.N, -1)
        plain = onp.gat_layer(sd, l, x32, g.src, g.dst, prm['alpha'], heads[l])[0].reshape(g.N, -1)
        e_f32 = metric_rel(plain, want)
        e_layer = metric_rel(layer_f64_sums(sd, l, x32, g.src, g.dst, prm['alpha'], heads[l])[0], want) if l == 0 else e_f32
        ft32 = f64.ft2[l].float()
        a32 = aggregate(sd, l, ft32, g.src, g.dst, prm['alpha'], heads[l])[0]
        a64 = aggregate(sd, l, ft32.double(), g.src, g.dst, prm['alpha'], heads[l])[0]
        rows.append({'std': float(f64.e[l].std()), 'max': float(f64.e[l].max()), 'e_agg': metric_agg(a32, a64),
                     'e_layer': e_layer, 'e_layer_f32': e_f32})
    net = {'e_net': metric_rel(Forward(tag, g, dtype=torch.float32, l0_f64_sums=True).logits, f64.logits),
           'e_net_f32': metric_rel(Forward(tag, g, dtype=torch.float32).logits, f64.logits),
           'logit_max': float(f64.logits.abs().max())}
    return rows, net


def noise_table():
    """The text of profiles/gat_arch_reference_noise.txt (its CPU part): python tests/gat_arch_cases.py"""
    out = ['f32 oracle against the f64 oracle of the same layer on identical rows, %d frames (one of every kind), as a fraction of the'
           % N_NOISE, 'bound of the GPU test that uses the metric: (a) %.0e * max(1, |want|max), (b) %.0e relative beyond 1, (c) %.0e likewise.'
           % (BOUND_AGG, BOUND_LAYER, BOUND_NET), 'Every figure has to stay <= 0.25 (tests/test_gat_archs_host.py).  Layer 0 of (b) and (c): the oracle with f64 running sums',
           'in its two GEMMs, as the library computes that layer; the plain f32 oracle in brackets.', '']
    for tag in TAGS:
        rows, net = reference_noise(tag)
        out.append('%-9s attn_gain %s  logit_gain %g' % (tag, '/'.join('%g' % round(g, 3) for g in tight_gains(tag)), logit_gain(tag)))
        for l, (r, (din, nh, od)) in enumerate(zip(rows, dims(tag))):
            out.append('   layer %d  %4d -> %2d x %2d   logit std %5.2f max %6.1f   (a) e_ref %.2e = %.2f   (b) e_ref %.2e = %.2f (f32 %.2f)'
                       % (l, din, nh, od, r['std'], r['max'], r['e_agg'], r['e_agg'] / BOUND_AGG, r['e_layer'],
                          r['e_layer'] / BOUND_LAYER, r['e_layer_f32'] / BOUND_LAYER))
        out.append('   network   |logit| <= %5.1f   (c) e_ref %.2e = %.2f (f32 %.2f)'
                   % (net['logit_max'], net['e_net'], net['e_net'] / BOUND_NET, net['e_net_f32'] / BOUND_NET))
    return '\n'.join(out) + '\n'


if __name__ == '__main__':
    print(noise_table(), end='')


def fp16_rows_statement(sd, l, x32, g, alpha, num_heads, coef_fp16, margin=4.0):
    """Layer l with fp16 ft2 rows (the attn_fp16 mode), stated on the f64 oracle -> (want [N, hd] before the activation, slack).
    ft2 = fc2(...) in float64 on the fp32 input rows, rounded to fp32 and then to fp16; the weighted sum takes the fp16 rows; the
    coefficients a1 / a2 come from the fp32 values (coef_fp16 False: the fc2 epilogue) or from the fp16 rows (True: k_attn_coef,
    the fused kernel's own).

    slack: an implementation computes ft2 in fp32 before it rounds to fp16, so an element whose exact value lies within `rho` of
    a tie between two fp16 values may land on either -- one fp16 spacing (1e-3 relative), a hundred times (h)'s bound.  rho =
    margin x the f32 oracle's own error on these ft2 rows (the margin of (d)).  Such elements, and only they, widen the bound
    of the outputs they feed, by what one spacing can do there: through the weighted sum, a_e x spacing; through a coefficient
    (coef_fp16 only), 2.02 Delta sum_e a_e |row_e| with Delta the largest shift of an in-edge's logit (first order in the softmax,
    1 % for the second).  Outputs fed by no such element keep (h)'s bound alone."""
    onp = oracle()
    N = x32.shape[0]
    ft64 = onp.gat_layer(sd, l, x32.double(), g.src, g.dst, alpha, num_heads)[1]['ft2'].reshape(N, -1)
    ft32 = onp.gat_layer(sd, l, x32, g.src, g.dst, alpha, num_heads)[1]['ft2'].reshape(N, -1)
    rho = margin * float((ft32.double() - ft64).abs().max())
    h = ft64.float().half()
    if coef_fp16:
        want, _, a = aggregate(sd, l, h.double(), g.src, g.dst, alpha, num_heads)
    else:
        want, _, a = aggregate(sd, l, ft64.float().double(), g.src, g.dst, alpha, num_heads, fp16_sum=True)
    hn = h.numpy()
    h64, v = hn.astype(np.float64), ft64.numpy()
    nxt = np.nextafter(hn, np.float16(np.inf)).astype(np.float64)
    prv = np.nextafter(hn, np.float16(-np.inf)).astype(np.float64)
    near = (np.abs(v - (h64 + nxt) / 2) <= rho) | (np.abs(v - (h64 + prv) / 2) <= rho)
    fs = torch.from_numpy(near * np.maximum(nxt - h64, h64 - prv))                       # [N, hd] what a flip moves
    hd = fs.shape[1]
    col_head = torch.arange(hd) // (hd // num_heads)
    s, d = torch.from_numpy(g.src).long(), torch.from_numpy(g.dst).long()
    a_col = a[:, col_head]                                                               # [E, hd]
    slack = torch.zeros_like(fs).index_add_(0, d, a_col * fs[s])
    if coef_fp16:
        p = 'layers.%d.' % l
        al = torch.from_numpy(np.abs(np.asarray(sd[p + 'attn_l'], np.float64)).reshape(num_heads, -1))
        ar = torch.from_numpy(np.abs(np.asarray(sd[p + 'attn_r'], np.float64)).reshape(num_heads, -1))
        fs3 = fs.reshape(N, num_heads, -1)
        d1, d2 = (fs3 * al).sum(2), (fs3 * ar).sum(2)                                    # [N, heads] shift of a1, of a2
        idx = d.view(-1, 1).expand(-1, num_heads)
        delta = torch.zeros((N, num_heads), dtype=torch.float64).scatter_reduce(0, idx, d1[s], reduce='amax', include_self=True) + d2
        mass = torch.zeros_like(fs).index_add_(0, d, a_col * h.double()[s].abs())
        slack = slack + 2.02 * delta[:, col_head] * mass
    return want.numpy(), slack.numpy()
