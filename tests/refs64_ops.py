"""The parameter-gradient protocol of robust_e2e_gan_amd/ops.py against float64: references, the table of
Functions and the pure checker of tests/test_ops_protocol_gpu.py.

Plain torch on the CPU, autograd for every gradient, nothing imported from the product or from ``oracle``.  The references that exist are
reused (refs64.decoder_loop_ref, refs64_att, refs64_dlayers, refs64_rnn, refs64_lm, refs64_fsrnn); what has none gets a thin restatement
here, pinned to torch's own modules in double by tests/test_refs64_ops_cpu.py.

DESIGN.md section 5.1, which the tests quote:
    P1 first write.   ``p.grad is None`` gives a fresh ``p.grad`` equal to dL/dp.  Every element is written.
    P2 accumulate.    With ``p.grad = g0``, the result is ``g0 + dL/dp``.  Nothing outside ``p.grad``'s extent is written.
    P3 several uses.  A parameter used by two calls in one graph receives the sum -- also when the second call and the weight-gradient
                      kernels run on other streams under ``ops.routing(wgrad=..., aux=...)``.
    P4 graph-time choice, per parameter.  A gradient only for a parameter that required one when the forward ran and is not in
                      ``FROZEN_PARAMS`` when the backward runs; ``requires_grad`` flipped in between changes nothing; an excluded parameter's
                      ``.grad`` stays ``None`` / bit-identical; the input gradient and the other parameters' gradients are unaffected.
    P5 no input gradient.  The parameter gradients are still right when the data input needs none.
    P6 upstream forms.  ``dy`` non-contiguous: a transposed view, an expanded scalar, a slice of a larger buffer.
    P7 second walk.   On a retained graph an op whose backward destroys its saved state raises ``Re2eError`` naming the op; every other op
                      gives the same gradient again.

``OPS``: one row per Function and shape (section 3 of the issue: the smallest shape that reaches each host-side branch).  A row's case is
``dict(params, inputs, aux, dy)``: fp32 CPU tensors; ``ref(P, X, aux)`` is the differentiable reference of the FIRST output in the dtype of its
arguments; ``row_grads`` differentiates sum(y * dy) (+ the second use of P3: the same parameters on ``second_use``'s inputs).

Bars: no new numbers.  Each gradient is held to the bar its kernel has in its own refs64* module; an op that composes several kernels
takes the loosest of theirs: the dense products BAR_DENSE = the largest entry of refs64_gemm.BARS (5e-6), convolutions refs64_conv.BARS
of the family the plan names for the row, BatchNorm and the filterbank refs64_feat.BAR_*_GRAD, the recurrences refs64_rnn / refs64_lm /
refs64_fsrnn's gradient bars, the decoder refs64.BAR_DEC_GRAD + ATOL_DEC_GRAD with the absolute rule of test_decoder_loop_against_float64
for gvec_b, the embedding refs64.BAR_GRAD.  For P2 and P3 the distance is that of ``got - g0`` from float64."""
import collections

import torch
import torch.nn.functional as F

import refs64 as R
import refs64_att as RA
import refs64_conv as RC
import refs64_dlayers as RD
import refs64_feat as RFE
import refs64_fsrnn as RF
import refs64_gemm as RG
import refs64_lm as RL
import refs64_rnn as RR

from refs64 import margin_ok, rel_err, rnd          # noqa: F401  (re-exported)

BAR_DENSE = max(b for b, _ in RG.BARS.values())
GUARD = 8                       # guard floats before, between and after a row's gradients in the flat buffer
SENTINEL = -7.25e33             # what the guards hold

Bar = collections.namedtuple('Bar', 'bar atol absolute')       # absolute: max |got - want| <= absolute (a gradient whose true value is zero)


def _bar(bar, atol=0.0, absolute=None):
    return Bar(bar, atol, absolute)


# ---------------------------------------------------------------------------------------------
# thin restatements (pinned to torch.nn in double by tests/test_refs64_ops_cpu.py)
# ---------------------------------------------------------------------------------------------
def act_ref(v, act):
    if act is None:
        return v
    return {'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid, 'lrelu': lambda t: torch.where(t > 0, t, 0.2 * t)}[act](v)


def linear_ref(x, W, b=None, act=None, valid=None):
    """act(x W^T + b); ``valid`` ((T,B) bool, x time-major (T,B,K)): the rows of padded frames hold act(b), what the product over a zero row
    leaves there (ops.gemm_rows(fill=True)) -- nothing of x or W."""
    z = x @ W.t()
    if b is not None:
        z = z + b
    y = act_ref(z, act)
    if valid is not None:
        fill = act_ref(b if b is not None else z.new_zeros(W.shape[0]), act)
        y = torch.where(valid.unsqueeze(-1), y, fill.expand_as(y))
    return y


def linear_2bias_ref(x, W, b1, b2):
    return x @ W.t() + b1 + b2


def fbank_dense_ref(x, W, cmvn=None):
    """log(max(x^2 W, 1e-7)) with W (F, NF), then (y + c0) * c1."""
    y = torch.log(torch.clamp((x * x) @ W, min=RFE.CLAMP))
    return y if cmvn is None else (y + cmvn[0].to(y.dtype)) * cmvn[1].to(y.dtype)


def mask_fc_ref(proj, W, mix, lens):
    """sigmoid(proj W^T) . [t < len] . mix for batch-first proj (B,T,K), mix (B,T,N)."""
    T = proj.shape[1]
    valid = (torch.arange(T).unsqueeze(0) < torch.as_tensor(lens).long().unsqueeze(1)).unsqueeze(-1)
    return torch.sigmoid(proj @ W.t()) * valid.to(proj.dtype) * mix.to(proj.dtype)


def conv2d_ref(x, W, b=None, stride=1, pad=1, act=None, pool=False, rows_out=None):
    """NHWC x (N,H,W,Cin), W (Cout,Cin,KH,KW) -> act(conv + b), NHWC; ``pool``: then the 2x2 / stride-2 ceil-mode max pool; ``rows_out`` (one
    height per image): rows at or beyond it are zero (ops.RowLims.out)."""
    N, H, Wd, _ = x.shape
    Cout, _, KH, KW = W.shape
    OH, OW = RC.conv_out(H, KH, stride, pad), RC.conv_out(Wd, KW, stride, pad)
    # written out as patches x weights (one matrix product, whose fp32 run is a plain blocked sum: the library convolution of the CPU may
    # pick a transformed algorithm for 3x3 layers, which says nothing about fp32 arithmetic on the input)
    cols = F.unfold(x.permute(0, 3, 1, 2), (KH, KW), padding=pad, stride=stride)             # (N, Cin KH KW, OH OW)
    y = (W.reshape(Cout, -1) @ cols).view(N, Cout, OH, OW)
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    y = act_ref(y, act)
    if pool:
        y = F.max_pool2d(y, 2, 2, ceil_mode=True)
    y = y.permute(0, 2, 3, 1)
    if rows_out is not None:
        keep = torch.arange(y.shape[1]).unsqueeze(0) < torch.as_tensor(rows_out).long().unsqueeze(1)
        y = y * keep.to(y.dtype).unsqueeze(-1).unsqueeze(-1)
    return y


def conv_transpose2d_ref(x, Wt, b=None, pad=1):
    """NHWC x (N,H,W,C1), Wt (C1,C2,2p+2,2p+2), stride 2 -> (N,2H,2W,C2)."""
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), Wt, None, 2, pad).permute(0, 2, 3, 1)
    return y if b is None else y + b


def bn_lrelu_ref(x, gamma, beta, eps=1e-5, slope=0.2):
    """Train-mode BatchNorm over all but the last axis of NHWC x (biased variance), then LeakyReLU(slope)."""
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    mean = x2.mean(0)
    var = ((x2 - mean) ** 2).mean(0)
    y = (x - mean) / torch.sqrt(var + eps) * gamma + beta
    return torch.where(y > 0, y, slope * y)


BILSTM_KEYS = tuple('%s.%s' % (d, k) for d in 'fr' for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh'))


def bilstm_layer_ref(x, lens, P):
    """x (T,B,I) time-major -> y (T,B,2H), zero beyond each length: both input projections with both biases, then
    refs64_rnn.lstm_seq_forward."""
    xg = [x @ P[d + '.w_ih'].t() + P[d + '.b_ih'] + P[d + '.b_hh'] for d in 'fr']
    return RR.lstm_seq_forward(xg[0], xg[1], P['f.w_hh'], P['r.w_hh'], lens)[0]


def embedding_ref(table, ids):
    return table[ids.long()]


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
Row = collections.namedtuple('Row', 'name fn run build ref bars cells groups destroys zero_dy')
CELLS = ('P1', 'P2', 'P3', 'P3-routed', 'P4', 'P5', 'P6', 'P7')
OPS = []
NO_DICT_GRAPH = 'the parameters arrive in a dict: without a differentiable input the Function has no node in the graph'


def _add(name, fn, run, build, ref, bars, groups=None, cells=None, destroys=False, zero_dy=None):
    """cells: {cell: reason} for the cells that do NOT apply; groups: {P4 case: parameter names} (default: each parameter on its own);
    zero_dy: why the expanded-scalar form of P6 is left out (the op's contract takes dy zero somewhere), or None."""
    OPS.append(Row(name, fn, run, build, ref, bars, dict(cells or {}), groups, destroys, zero_dy))


def _od(**kw):
    return collections.OrderedDict(kw)


def _all(case, bar):
    return {k: bar for k in list(case['params']) + ['d_' + k for k in case['inputs']]}


# ---- LinearFn ---------------------------------------------------------------------------------------------------------------------
def _linear(xshape, N, act, ragged=None, padded=None):
    def build():
        g = torch.Generator().manual_seed(11 + sum(xshape) + N)
        K = xshape[-1]
        x, W, b = rnd(g, *xshape), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
        dy = rnd(g, *xshape[:-1], N, scale=0.3)
        aux = dict(act=act, lens=None, padded=padded)
        if ragged is not None:
            aux['lens'] = list(ragged)
            dy = dy * RR.valid_mask(ragged, xshape[0]).unsqueeze(-1).float()      # the consumers mask the padded frames: their gradient is zero
        return dict(params=_od(W=W, b=b), inputs=_od(x=x), aux=aux, dy=dy)

    def ref(P, X, aux):
        valid = RR.valid_mask(aux['lens'], X['x'].shape[0]) if aux['lens'] is not None else None
        return linear_ref(X['x'], P['W'], P['b'], aux['act'], valid)
    return build, ref


_RAGGED = 'LinearFn over row maps takes dz zero in the padded rows (its consumers mask them)'
for _name, _args, _zd in (('linear-3x5x12-8-tanh', dict(xshape=(3, 5, 12), N=8, act='tanh'), None),
                          ('linear-rows-T5B3-K12', dict(xshape=(5, 3, 12), N=8, act='tanh', ragged=(5, 3, 1)), _RAGGED),
                          ('linear-rows-T5B3-K10', dict(xshape=(5, 3, 10), N=8, act='tanh', ragged=(5, 3, 1)), _RAGGED),
                          ('linear-M2080-K12-N8', dict(xshape=(2080, 12), N=8, act=None), None),
                          ('linear-padded-T6B2-K8-V7', dict(xshape=(6, 2, 8), N=7, act=None, padded=16), None)):
    _b, _r = _linear(**_args)
    _add(_name, 'LinearFn', 'linear', _b, _r, lambda c: _all(c, _bar(BAR_DENSE)), zero_dy=_zd)


# The padded-gradient hand-over as the step makes it: the projection in front of CtcFn.  CtcFn.backward pads its gradient rows only from 2048
# rows (T * B) on with V % 4 != 0, so the row 'linear-padded-T6B2-K8-V7' above hands LinearFn.backward a buffer padded and registered the
# way CtcFn does it, and this one goes through CtcFn itself at the smallest batch that makes it pad: 32 x 64 rows.
def _linear_ctc_build():
    g = torch.Generator().manual_seed(17)
    T, B, K, V = 32, 64, 8, 7
    labels = [[int(v) for v in torch.randint(1, V, (2 + i % 5,), generator=g)] for i in range(B)]
    return dict(params=_od(W=rnd(g, V, K, scale=K ** -0.5), b=rnd(g, V, scale=0.1)), inputs=_od(x=rnd(g, T, B, K)),
                aux=dict(act=None, lens=None, padded=None, ctc=dict(hlens=[T - i % 12 for i in range(B)], labels=labels)), dy=torch.tensor([1.3]))


def _linear_ctc_ref(P, X, aux):
    logits = linear_ref(X['x'], P['W'], P['b'])
    labels = aux['ctc']['labels']
    nll = F.ctc_loss(logits.log_softmax(2), torch.tensor([v for l in labels for v in l]), torch.tensor(aux['ctc']['hlens']),
                     torch.tensor([len(l) for l in labels]), blank=0, reduction='none', zero_infinity=False)
    return (nll.sum() / logits.shape[1]).view(1)


_add('linear-ctc-T32-B64-K8-V7', 'LinearFn', 'linear_ctc', _linear_ctc_build, _linear_ctc_ref, lambda c: _all(c, _bar(max(R.BAR_GRAD, BAR_DENSE))),
     cells={'P6': 'the upstream gradient of this row is CtcFn\'s own, a scalar\'s: the forms of P6 run on the other LinearFn rows'})


# ---- Linear2BiasFn, FbankDenseFn, MaskFcFn, EmbeddingFn ------------------------------------------------------------------------------
def _linear2_build():
    g = torch.Generator().manual_seed(21)
    return dict(params=_od(W=rnd(g, 8, 10, scale=10 ** -0.5), b1=rnd(g, 8, scale=0.1), b2=rnd(g, 8, scale=0.1)), inputs=_od(x=rnd(g, 4, 3, 10)), aux={},
                dy=rnd(g, 4, 3, 8, scale=0.3))


_add('linear2bias-4x3x10-8', 'Linear2BiasFn', 'linear2', _linear2_build, lambda P, X, aux: linear_2bias_ref(X['x'], P['W'], P['b1'], P['b2']),
     lambda c: _all(c, _bar(BAR_DENSE)))


def _fbank_dense(cmvn):
    def build():
        g = torch.Generator().manual_seed(31)
        W = torch.rand(9, 4, generator=g) * 0.9 + 0.1                # positive: x^2 W stays far from the clamp
        cm = torch.stack([torch.linspace(1.0, 2.0, 4), torch.linspace(0.3, 0.6, 4)]) if cmvn else None
        return dict(params=_od(W=W), inputs=_od(x=rnd(g, 2, 5, 9) + 0.1), aux=dict(cmvn=cm), dy=rnd(g, 2, 5, 4, scale=0.3))
    return build


for _cm in (False, True):
    _add('fbank-dense-2x5x9-4' + ('-cmvn' if _cm else ''), 'FbankDenseFn', 'fbank_dense', _fbank_dense(_cm),
         lambda P, X, aux: fbank_dense_ref(X['x'], P['W'], aux['cmvn']), lambda c: _all(c, _bar(max(RFE.BAR_FBANK_GRAD, BAR_DENSE))))


def _mask_fc(B, T, K, N, lens):
    def build():
        g = torch.Generator().manual_seed(41 + T)
        return dict(params=_od(W=rnd(g, N, K, scale=K ** -0.5)), inputs=_od(proj=rnd(g, B, T, K)), aux=dict(mix=rnd(g, B, T, N).abs(), lens=list(lens), T=T),
                    dy=rnd(g, B, T, N, scale=0.3))
    return build


for _shape in ((3, 11, 16, 257, (11, 7, 4)), (3, 700, 16, 37, (700, 512, 33))):
    _add('maskfc-B%d-T%d-K%d-N%d' % _shape[:4], 'MaskFcFn', 'mask_fc', _mask_fc(*_shape),
         lambda P, X, aux: mask_fc_ref(X['proj'], P['W'], aux['mix'], aux['lens']), lambda c: _all(c, _bar(BAR_DENSE)))


def _embedding_build():
    g = torch.Generator().manual_seed(51)
    return dict(params=_od(table=rnd(g, 9, 6)), inputs=_od(), aux=dict(ids=torch.tensor([3, 0, 3, 8, 5, 3, 0], dtype=torch.int32), block=3),
                dy=rnd(g, 7, 6, scale=0.3))


_add('embedding-V9-D6-n7', 'EmbeddingFn', 'embedding', _embedding_build, lambda P, X, aux: embedding_ref(P['table'], aux['ids']),
     lambda c: _all(c, _bar(R.BAR_GRAD)), cells={'P5': 'EmbeddingFn has no float input'})


# ---- Conv2dFn, ConvTranspose2dFn, BnLreluFn --------------------------------------------------------------------------------------------
def conv_family(row):
    return row.form[0] if row.form[0] in ('wino3x3', 'wino4x4') else 'direct'


def smallest_wgrad_row(family):
    """The smallest weight-gradient row of refs64_conv.CONV_CASES whose declared form belongs to ``family``."""
    rows = [r for r in RC.CONV_CASES if r.direction == RC.WGRAD and conv_family(r) == family and not r.flags]
    return min(rows, key=lambda r: r.N * r.H * r.W * r.Cin * r.Cout)


def _conv(N, H, W, Cin, Cout, k, family, act='relu', pool=False, lims=None):
    def build():
        g = torch.Generator().manual_seed(61 + H + Cin)
        OH = RC.conv_out(H, k, 1, 1)
        OW = RC.conv_out(W, k, 1, 1)
        oshape = (N, (OH + 1) // 2, (OW + 1) // 2, Cout) if pool else (N, OH, OW, Cout)
        # (a mean beside the noise: the bias gradient of a one-channel layer is ONE sum and its own max -- of pure noise it would cancel to a
        #  fortieth of its terms, and the unit 'of the tensor's max' would measure that cancellation, not the kernel)
        dy = rnd(g, *oshape, scale=0.3) + 0.25
        if lims is not None:
            dy = dy * (torch.arange(OH).unsqueeze(0) < torch.tensor(lims[0]).unsqueeze(1)).float().unsqueeze(-1).unsqueeze(-1)
        return dict(params=_od(W=rnd(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5), b=rnd(g, Cout, scale=0.1)), inputs=_od(x=rnd(g, N, H, W, Cin)),
                    aux=dict(stride=1, pad=1, act=act, pool=pool, lims=lims, family=family, shape=(N, H, W, Cin, Cout, k)), dy=dy)

    def ref(P, X, aux):
        return conv2d_ref(X['x'], P['W'], P['b'], 1, 1, aux['act'], aux['pool'], aux['lims'][0] if aux['lims'] is not None else None)

    def bars(case):
        loosest = lambda q: _bar(max(RC.BARS[(q, family)], RC.BARS[('pool', family)]) if pool else RC.BARS[(q, family)])
        return dict(W=loosest('dW'), b=_bar(max(RC.BARS[('db', 'direct')], RC.BARS[('pool', family)]) if pool else RC.BARS[('db', 'direct')]), d_x=loosest('dx'))
    return build, ref, bars


_LIMS = 'Conv2dFn with RowLims takes dz zero in the rows beyond lims.out (the pack that follows never reads them)'
for _fam in ('wino3x3', 'wino4x4', 'direct'):
    _r0 = smallest_wgrad_row(_fam)
    _b, _r, _bars = _conv(_r0.N, _r0.H, _r0.W, _r0.Cin, _r0.Cout, _r0.k, _fam)
    _add('conv-%s-%dx%dx%dx%d-%d-k%d' % (_fam, _r0.N, _r0.H, _r0.W, _r0.Cin, _r0.Cout, _r0.k), 'Conv2dFn', 'conv2d', _b, _r, _bars)
_b, _r, _bars = _conv(1, 5, 3, 4, 36, 3, 'direct')           # (the family's smallest row has one channel each way: one with a channel sum as well)
_add('conv-direct-1x5x3x4-36-k3', 'Conv2dFn', 'conv2d', _b, _r, _bars)
_b, _r, _bars = _conv(2, 30, 7, 64, 64, 3, 'wino3x3', lims=((30, 16), (30, 30)))
_add('conv-wino3x3-rowlims-2x30x7x64-64', 'Conv2dFn', 'conv2d', _b, _r, _bars, zero_dy=_LIMS)
_b, _r, _bars = _conv(2, 9, 17, 64, 64, 3, 'wino3x3', pool=True)
_add('conv-wino3x3-pool-bias-2x9x17x64-64', 'Conv2dFn', 'conv2d', _b, _r, _bars)


def _convt_build():
    g = torch.Generator().manual_seed(71)
    return dict(params=_od(Wt=rnd(g, 6, 4, 4, 4, scale=(6 * 4) ** -0.5), b=rnd(g, 4, scale=0.1)), inputs=_od(x=rnd(g, 2, 4, 3, 6)), aux=dict(pad=1),
                dy=rnd(g, 2, 8, 6, 4, scale=0.3))


_add('convT-2x4x3x6-4-k4s2p1', 'ConvTranspose2dFn', 'conv_transpose2d', _convt_build,
     lambda P, X, aux: conv_transpose2d_ref(X['x'], P['Wt'], P['b'], aux['pad']),
     lambda c: dict(Wt=_bar(RC.BARS[('dW', 'direct')]), b=_bar(RC.BARS[('db', 'direct')]), d_x=_bar(RC.BARS[('dx', 'direct')])))


def _bn(C):
    def build():
        g = torch.Generator().manual_seed(81 + C)
        return dict(params=_od(gamma=1.0 + rnd(g, C, scale=0.2), beta=rnd(g, C, scale=0.1)), inputs=_od(x=rnd(g, 3, 5, 4, C) + 0.3),
                    aux=dict(eps=1e-5, slope=0.2, momentum=0.1), dy=rnd(g, 3, 5, 4, C, scale=0.3))
    return build


for _C in (6, 8):
    _add('bn-lrelu-3x5x4xC%d' % _C, 'BnLreluFn', 'bn_lrelu', _bn(_C),
         lambda P, X, aux: bn_lrelu_ref(X['x'], P['gamma'], P['beta'], aux['eps'], aux['slope']), lambda c: _all(c, _bar(RFE.BAR_BN_GRAD)))


# ---- BiLstmFn -------------------------------------------------------------------------------------------------------------------------
def _bilstm(T, B, I, H, lens, cached):
    """cached: the lengths come from model.e2e_common.lens_dev, so ops.row_maps knows them on the host (the products then run over the valid
    rows where there are enough of them)."""
    def build():
        g = torch.Generator().manual_seed(91 + T + I)
        P = collections.OrderedDict()
        for d in 'fr':
            P[d + '.w_ih'], P[d + '.w_hh'] = rnd(g, 4 * H, I, scale=I ** -0.5), rnd(g, 4 * H, H, scale=H ** -0.5)
            P[d + '.b_ih'], P[d + '.b_hh'] = rnd(g, 4 * H, scale=0.1), rnd(g, 4 * H, scale=0.1)
        return dict(params=P, inputs=_od(x=rnd(g, T, B, I)), aux=dict(lens=list(lens), cached=cached), dy=rnd(g, T, B, 2 * H, scale=0.3))
    return build


_BILSTM_GROUPS = {'lstm-weights': [k for k in BILSTM_KEYS if '.w_' in k], 'lstm-biases': [k for k in BILSTM_KEYS if '.b_' in k],
                  'all-but-f.w_hh': [k for k in BILSTM_KEYS if k != 'f.w_hh']}
# the forward pads its input when the width is no multiple of 4 AND there are at least 1024 rows (T * B): 342 x 3 = 1026
for _name, _args in (('bilstm-T5-B3-I12-H8-ragged', (5, 3, 12, 8, (5, 3, 1), False)), ('bilstm-T5-B3-I12-H8-full', (5, 3, 12, 8, (5, 5, 5), False)),
                     ('bilstm-T342-B3-I5-H8-padded-input', (342, 3, 5, 8, (342, 171, 1), True))):
    _add(_name, 'BiLstmFn', 'bilstm', _bilstm(*_args), lambda P, X, aux: bilstm_layer_ref(X['x'], aux['lens'], P), lambda c: _all(c, _bar(RR.BAR_RNN_GRAD)),
         groups=_BILSTM_GROUPS, destroys=True)


# ---- DecoderLoopFn, DecoderUpperFn -----------------------------------------------------------------------------------------------------
def _upper_params(layers):
    P = collections.OrderedDict()
    for l, lay in enumerate(layers):
        for k in RD.UPPER_KEYS:
            P['l%d.%s' % (l + 1, k)] = lay[k]
    return P


def _layers_of(P):
    n = len([k for k in P if k.endswith('.w_ih') and k.startswith('l')])
    return [{k: P['l%d.%s' % (l + 1, k)] for k in RD.UPPER_KEYS} for l in range(n)]


def _decoder(shape, kind='location', persist=False, upper=0):
    def build():
        c = R.decoder_case(shape) if kind == 'location' else RA.att_case(kind, shape)
        B, T, L1, E, A, D, C, Fh = shape
        P = collections.OrderedDict(c['Pm'])
        if upper:
            P.update(_upper_params(RD.stack_case((B, L1, D, upper + 1))['layers']))
        return dict(params=P, inputs=_od(hmask=c['hmask'], pre=c['pre']), aux=dict(ids=c['ids'], hlens=c['hlens'], L1=L1, kind=kind, persist=persist, B=B),
                    dy=c['gz'])

    def ref(P, X, aux):
        Pm = {k: v for k, v in P.items() if '.' not in k}
        z0 = RD.layer0_ref(aux['kind'], X['hmask'], X['pre'], aux['ids'], aux['hlens'], aux['L1'], Pm)[0]
        lays = _layers_of(P)
        return RD.upper_ref(z0, lays)[-1] if lays else z0

    def bars(case):
        out = _all(case, _bar(R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD))
        if 'gvec_b' in out:      # true gradient zero (a shift of the energies does not move a softmax): test_decoder_loop_against_float64's rule
            out['gvec_b'] = _bar(R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD, absolute=1e-5 * case['aux']['L1'] * case['aux']['B'])
        return out

    def groups(case):
        P = list(case['params'])
        att = [k for k in P if k not in RA.DEC_KEYS and '.' not in k]
        g = {'embed': ['embed'], 'lstm-weights': ['w_ih', 'w_hh'], 'lstm-biases': ['b_ih', 'b_hh'], 'attention': att, 'all-but-w_hh': [k for k in P if k != 'w_hh']}
        if any('.' in k for k in P):
            g['upper'] = [k for k in P if '.' in k]
        return g
    return build, ref, bars, groups


def _dec_rows():
    rows = [((1, 5, 1, 16, 4, 4, 1, 0), 'location', True, 0), ((1, 5, 1, 16, 4, 4, 1, 0), 'location', False, 0),
            ((5, 37, 6, 32, 24, 12, 3, 4), 'location', True, 0), ((5, 37, 6, 32, 24, 12, 3, 4), 'location', False, 0),
            ((2, 33, 3, 68, 65, 20, 5, 8), 'location', False, 0)]          # (A % 4: the persistent form does not take this one)
    rows += [(RA.ATT_SHAPES[0][0], kind, False, 0) for kind in RA.KINDS]
    rows += [((2, 9, 3, 16, 8, 8, 2, 2), 'location', False, 2), ((2, 9, 3, 16, 8, 14, 2, 2), 'location', False, 2)]     # D = 14: the tiny fixtures' width
    for shape, kind, persist, upper in rows:
        b, r, bars, groups = _decoder(shape, kind, persist, upper)
        name = 'decoder-%s-%s-%s%s' % (kind, 'x'.join(str(v) for v in shape), 'persist' if persist else 'step', '-upper%d' % upper if upper else '')
        _add(name, 'DecoderLoopFn', 'decoder_loop', b, r, bars, groups=groups, cells={'P5': NO_DICT_GRAPH}, destroys=True)


_dec_rows()


def _upper(B, L1, D, nl):
    def build():
        c = RD.stack_case((B, L1, D, nl))
        return dict(params=_upper_params(c['layers']), inputs=_od(z0=c['z0']), aux=dict(D=D), dy=c['gz'])
    return build


for _D, _destroys in ((8, False), (14, True)):           # D = 14 runs the general cell kernels, which turn the saved gates into d(gates) in place
    _add('decoder-upper-L3-B2-D%d-two-layers' % _D, 'DecoderUpperFn', 'decoder_upper', _upper(2, 3, _D, 3),
         lambda P, X, aux: RD.upper_ref(X['z0'], _layers_of(P))[-1], lambda c: _all(c, _bar(R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)),
         groups=lambda c: {'layer1': [k for k in c['params'] if k.startswith('l1.')], 'lstm-biases': [k for k in c['params'] if '.b_' in k],
                           'all-but-l2.w_ih': [k for k in c['params'] if k != 'l2.w_ih']},
         cells={'P5': NO_DICT_GRAPH}, destroys=_destroys)


# ---- LmSeqFn, FsrnnSeqFn ---------------------------------------------------------------------------------------------------------------
def _lm_build():
    row = min(RL.LM_CASES, key=lambda r: r[0] * r[1] * r[2])
    c = RL.table_case(row)
    return dict(params=_od(w_hh=c['whh']), inputs=_od(xg=c['xg'], h0=c['h0'], c0=c['c0']), aux={}, dy=c['dy'])


_add('lmseq-' + RL.case_id(min(RL.LM_CASES, key=lambda r: r[0] * r[1] * r[2])), 'LmSeqFn', 'lm_seq', _lm_build,
     lambda P, X, aux: RL.lm_window_forward(X['xg'], P['w_hh'], X['h0'], X['c0'])[0], lambda c: _all(c, _bar(RL.BAR_GRAD)), destroys=True)


def _fs_row():
    return min(RF.FS_CASES, key=lambda r: r[0] * r[1] * r[2] * r[3])


def _fs_build():
    row = _fs_row()
    c = RF.table_case(row)
    L = c['L']
    P = collections.OrderedDict([('c0.w_hh', c['W'][0][1])])
    for k in range(1, L + 1):
        for i, n in enumerate(RD.UPPER_KEYS):
            P['c%d.%s' % (k, n)] = c['W'][k][i]
    st = c['state']
    return dict(params=P, inputs=_od(xg=c['xg'], Fh=st[0], Fc=st[1], Sh=st[2], Sc=st[3]),
                aux=dict(L=L, cell0=(c['W'][0][0], c['W'][0][2], c['W'][0][3]), mh=c['mh'] if row[4] else None, mc=c['mc'] if row[4] else None,
                         dm=c['dm'] if row[5] else None, keep_h=RF.KEEP_H, keep_c=RF.KEEP_C), dy=c['dy'])


def _fs_ref(P, X, aux):
    L, dt = aux['L'], X['xg'].dtype
    cv = lambda t: t if t is None else t.to(dt)
    W = [(cv(aux['cell0'][0]), P['c0.w_hh'], cv(aux['cell0'][1]), cv(aux['cell0'][2]))] + [tuple(P['c%d.%s' % (k, n)] for n in RD.UPPER_KEYS) for k in range(1, L + 1)]
    mh, mc = (cv(aux['mh']), cv(aux['mc'])) if aux['mh'] is not None else (aux['keep_h'], aux['keep_c'])
    h = RF.fs_window_forward(X['xg'], W, (X['Fh'], X['Fc'], X['Sh'], X['Sc']), mh, mc, cv(aux['dm']), L)[0]
    return h[L - 1]


_add('fsrnn-' + RF.case_id(_fs_row()), 'FsrnnSeqFn', 'fsrnn_seq', _fs_build, _fs_ref, lambda c: _all(c, _bar(RF.BAR_GRAD)), destroys=True)

NAMES = [r.name for r in OPS]
BY_NAME = {r.name: r for r in OPS}
assert len(BY_NAME) == len(OPS)

# the torch.autograd.Function subclasses of ops.py that accumulate no parameter gradient (tests/test_refs64_ops_cpu.py: closure)
NO_PARAMETERS = ('Transpose01Fn', 'FbankFn', 'MeanLossFn', 'ActFn', 'MaxPool2Fn', 'VggPackFn', 'InstanceNormLreluFn', 'CtcFn', 'GatherRowsFn', 'CoralFn',
                 'CeFn', 'LabelSmoothFn', 'CmvnPairFn', 'MulConstFn', 'DropoutFn', 'MaskRowsFn')


# ---------------------------------------------------------------------------------------------
# gradients of a row under its upstream gradient
# ---------------------------------------------------------------------------------------------
def groups_of(row, case):
    g = row.groups(case) if callable(row.groups) else row.groups
    return g if g is not None else {k: [k] for k in case['params']}


def second_use(case, seed=1234):
    """The inputs of the second call of P3: the same parameters on half the first call's inputs (zeros, signs and ranges stay what the op's
    contract needs) under a fresh upstream gradient with the zeros of the first."""
    g = torch.Generator().manual_seed(seed)
    dy = case['dy']
    scale = float(dy.std()) if dy.numel() > 1 else float(dy.abs().max())
    dy2 = torch.randn(dy.shape, generator=g) * scale * (dy != 0).float()
    return dict(params=case['params'], inputs=collections.OrderedDict((k, 0.5 * v) for k, v in case['inputs'].items()), aux=case['aux'], dy=dy2)


def row_grads(row, case, dtype=torch.float64, uses=1):
    """-> {parameter: dL/dp, 'd_<input>': dL/dx of the FIRST use, 'd2_<input>': of the second} for L = sum over the uses of sum(y * dy); a
    parameter the loss does not depend on has a zero gradient."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    P = collections.OrderedDict((k, leaf(v)) for k, v in case['params'].items())
    loss, xs = 0.0, []
    for u, c in enumerate([case, second_use(case)][:uses]):
        X = collections.OrderedDict((k, leaf(v)) for k, v in c['inputs'].items())
        y = row.ref(P, X, c['aux'])
        assert y.shape == c['dy'].shape, (row.name, y.shape, c['dy'].shape)
        loss = loss + (y * c['dy'].to(dtype)).sum()
        xs.append(X)
    loss.backward()
    out = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in P.items()}
    for u, X in enumerate(xs):
        out.update({('d_' if u == 0 else 'd2_') + k: v.grad.detach() for k, v in X.items()})
    return out


# ---------------------------------------------------------------------------------------------
# the checker (pure: CPU tensors in, a list of violations out)
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def check_protocol(got, want64, want32, g0, guards, bars, case='', log=None):
    """got: {name: the tested run's gradient after the run, or None}; want64 / want32: {name: the float64 / fp32-CPU dL/dp the run owes (all
    uses and walks summed), or None for a parameter the run must leave alone}; g0: {name: what ``.grad`` held before the run, or None (no
    buffer)}; guards: None or (before, after), the guard floats around the gradients; bars: {name: Bar}.  -> the list of violations; ``log``
    (a list) receives one 'ERR ...' line per quantity, in the format of test_loss_kernels_gpu._held."""
    bad = []
    for name, w64 in want64.items():
        g, before = got.get(name), g0.get(name)
        if w64 is None:                                          # excluded: None stays None, a buffer stays bit-identical
            if before is None:
                if g is not None:
                    bad.append('%s: excluded, but a gradient was produced' % name)
            elif g is None or g.shape != before.shape or not torch.equal(_bits(g), _bits(before)):
                bad.append('%s: excluded, but its gradient buffer changed' % name)
            continue
        if g is None:
            bad.append('%s: no gradient was produced' % name)
            continue
        if tuple(g.shape) != tuple(w64.shape):
            bad.append('%s: gradient of shape %s, parameter of shape %s' % (name, tuple(g.shape), tuple(w64.shape)))
            continue
        b = bars[name]
        d = g.detach().double().cpu() - (before.detach().double().cpu() if before is not None else 0.0)
        w64 = w64.detach().double().cpu()
        if not torch.isfinite(d).all():
            bad.append('%s: %d elements are not finite (left unwritten?)' % (name, int((~torch.isfinite(d)).sum())))
            continue
        scale = w64.abs().max().item() if w64.numel() else 0.0
        if b.absolute is not None:
            err = (d - w64).abs().max().item()
            if log is not None:
                log.append('ERR %-46s %-16s hip %.2e (absolute; bar %.1e)' % (case, name, err, b.absolute))
            if not err <= b.absolute:
                bad.append('%s: %.3e from float64 in absolute terms (bar %.1e)' % (name, err, b.absolute))
            continue
        err = rel_err(d, w64)
        cpu = rel_err(want32[name], w64) if want32 is not None and want32.get(name) is not None else float('nan')
        if log is not None:
            log.append('ERR %-46s %-16s hip %.2e  fp32-cpu %.2e  bar %.0e' % (case, name, err, cpu, b.bar))
        if not err * scale <= b.bar * scale + b.atol:
            bad.append('%s: %.3e of the max from float64 (bar %.1e, fp32 on the CPU %.3e)' % (name, err, b.bar, cpu))
    if guards is not None:
        before, after = guards
        if before.shape != after.shape or not torch.equal(_bits(before), _bits(after)):
            bad.append('guard floats around the gradients were written')
    return bad


def margins(row, case, want64, want32, bars):
    """Precondition of every cell: torch's fp32 CPU run of the same reference is within a quarter of the bar (refs64.margin_ok)."""
    for name, w64 in want64.items():
        if w64 is None or bars[name].absolute is not None:
            continue
        margin_ok('%s %s' % (row.name, name), want32[name], w64, bars[name].bar, bars[name].atol)
