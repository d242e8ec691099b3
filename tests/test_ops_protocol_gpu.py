"""The parameter-gradient protocol of robust_e2e_gan_amd/ops.py (quoted in tests/refs64_ops.py) on the GPU: every
applicable (row, P) cell of refs64_ops.OPS, the fused autograd Functions against the float64 references under the call patterns training
and the direct module tests do not share -- first write, accumulation into a flat buffer between guard floats, two uses on one and on
three streams, parameters excluded at graph time / frozen at backward time / flipped in between, no input gradient, non-contiguous
upstream gradients, a second walk of a retained graph.

Gradient storage for P2 - P4: all of a row's ``.grad``s are views into ONE flat buffer at FlatOptimizer's alignment, every float of the
buffer outside the gradients is a guard (at least 8 before, between and after them) holding a sentinel; the gradients are prefilled with
a random g0 of the gradient's own scale; afterwards the guards must be bit-identical and ``got - g0`` within the bar of float64.

Every cell first asserts that torch's fp32 CPU run of the same reference is within a quarter of the bar (refs64_ops.margins), then prints
``ERR <case> <quantity> hip ... fp32-cpu ... bar ...``.  GPU only.

Measured on an MI355X when the module was written, worst case per Function over all its cells (the one nearest its bar), HIP / fp32 on the
CPU, of the tensor's max:
    LinearFn           5.8e-7 / 3.5e-7 (bar 5e-6; dW of the 2080-row form under dy = 1); behind CtcFn d x 1.2e-5 / 9.1e-6 (1e-4, CTC's)
    Linear2BiasFn      1.6e-7 / 8.4e-8 (5e-6)           FbankDenseFn  2.2e-7 / 5.9e-8 (1e-4)
    MaskFcFn           5.2e-7 / 3.3e-7 (5e-6; d proj)   EmbeddingFn   1.5e-7 / 3.7e-8 (1e-4)
    Conv2dFn           8.8e-6 / 2.1e-7 (3e-5; dW of the F(2x2,4x4) weight gradient, 65 x 65 x 64 -> 64); every other row below 0.2 of its bar
    ConvTranspose2dFn  3.4e-7 / 1.2e-7 (9e-7; db, two uses)
    BnLreluFn          7.3e-7 / 4.3e-7 (1e-4)           BiLstmFn      5.0e-7 / 8.1e-7 (2e-4; T = 342)
    DecoderLoopFn      1.8e-6 / 1.2e-7 (3e-4; d loc_conv, two uses); |d gvec_b| <= 0.006 of its absolute bar 1e-5 L1 B
    DecoderUpperFn     3.2e-7 / 1.2e-7 (3e-4)           LmSeqFn 5.4e-7 / 3.5e-7, FsrnnSeqFn 5.9e-7 / 3.5e-7 (2e-4)
Guards and excluded buffers bit-identical in every cell.  Before the protocol fixes that came with this module the P4 cells of MaskFcFn,
BnLreluFn, BiLstmFn, DecoderLoopFn (all kinds, with and without upper layers) and DecoderUpperFn failed, and the P7 cells of BiLstmFn,
DecoderLoopFn, DecoderUpperFn (D = 14), LmSeqFn and FsrnnSeqFn returned wrong gradients without an error."""
import contextlib
import functools

import pytest
import torch

import refs64_ops as O

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALIGN = 64                      # floats: FlatOptimizer's alignment of a parameter's slice


def _ops():
    from robust_e2e_gan_amd import ops, lib
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    return ops, lib


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


# ---------------------------------------------------------------------------------------------
# references (computed once per row and shared; never modified)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    return O.BY_NAME[name].build()


@functools.lru_cache(maxsize=None)
def _want(name, uses=1, ones=False):
    """(float64, fp32-CPU) gradients of the row under its upstream gradient (``ones``: under dy = 1, what y.sum().backward() hands down)."""
    row, case = O.BY_NAME[name], _case(name)
    if ones:
        case = dict(case, dy=torch.ones_like(case['dy']))
    return O.row_grads(row, case, torch.float64, uses), O.row_grads(row, case, torch.float32, uses)


def _bars(row, case):
    b = row.bars(case)
    return dict(b, **{'d2_' + k: b['d_' + k] for k in case['inputs']})


# ---------------------------------------------------------------------------------------------
# the Functions under test
# ---------------------------------------------------------------------------------------------
def _row_maps(ops, lens, T, B):
    """ops.RowMaps of a (T, B, .) batch, built by hand: ops.row_maps declines batches this small."""
    valid = [t * B + b for t in range(T) for b in range(B) if t < lens[b]]
    invalid = [r for r in range(T * B) if r not in set(valid)]
    ident = next((i for i, r in enumerate(valid) if r != i), len(valid))
    return ops.RowMaps(_i32(valid), _i32(invalid), len(valid), len(invalid), T * B, ident)


def _run_linear(ops, P, X, aux):
    x = X['x']
    maps = _row_maps(ops, aux['lens'], x.shape[0], x.shape[1]) if aux['lens'] is not None else None
    return ops.linear(x, P['W'], P['b'], aux['act'], maps)


def _run_linear_ctc(ops, P, X, aux):
    """The projection in front of ops.ctc_loss: CtcFn.backward pads its gradient rows and LinearFn.backward must recognise the buffer."""
    labels = aux['ctc']['labels']
    ll = [len(l) for l in labels]
    off = [sum(ll[:i]) for i in range(len(ll))]
    logits = ops.linear(X['x'], P['W'], P['b'], None)
    return ops.ctc_loss(logits, _i32(aux['ctc']['hlens']), _i32([v for l in labels for v in l]), _i32(off), _i32(ll), max(ll))


def _run_conv2d(ops, P, X, aux):
    from robust_e2e_gan_amd import lib
    N, H, W, Cin, Cout, k = aux['shape']
    fam = ops.conv_plan(lib.CONV_WGRAD, N, H, W, Cin, Cout, k, k, 1, 1, 0, 0, lib.ACT_NONE, 0)[0]
    assert fam == aux['family'], 'the plan names %s for this weight gradient, the row says %s' % (fam, aux['family'])
    lims = None
    if aux['lims'] is not None:
        out, inp = aux['lims']
        assert ops.conv_plan(lib.CONV_FWD, N, H, W, Cin, Cout, k, k, 1, 1, 0, 0, ops.ACT[aux['act']], lib.CONV_BIAS)[0] == 'wino3x3'
        lims = ops.RowLims(_i32(out), _i32(inp), H - min(out), H - min(inp))
    return ops.conv2d(X['x'], P['W'], P['b'], 1, 1, aux['act'], pool=aux['pool'], lims=lims)


def _run_bilstm(ops, P, X, aux):
    from robust_e2e_gan_amd.model import e2e_common as ec
    lens = ec.lens_dev(aux['lens'], DEV) if aux['cached'] else _i32(aux['lens'])
    y = ops.bilstm(X['x'], lens, [P[k] for k in O.BILSTM_KEYS])
    if 'padded-input' in aux.get('name', ''):
        assert y.grad_fn is None or y.grad_fn.saved_tensors[0].shape[1] != X['x'].shape[2], 'the forward did not pad its input'
    return y


def _run_decoder(ops, P, X, aux):
    Pm = {k: v for k, v in P.items() if '.' not in k}
    upper = O._layers_of(P) or None
    zs, w = ops.DecoderLoopFn.apply(X['hmask'], X['pre'], aux['ids'].to(DEV), _i32(aux['hlens']), aux['L1'], Pm, None, False, aux['kind'], upper)
    assert not w.requires_grad
    if zs.grad_fn is not None:
        assert getattr(zs.grad_fn, 'persist', aux['persist']) == aux['persist'], 'the loop did not take the form the row names'
    return zs


def _run_fsrnn(ops, P, X, aux):
    L = aux['L']
    dv = lambda t: None if t is None else t.to(DEV)
    c0 = aux['cell0']
    W = [(dv(c0[0]), P['c0.w_hh'], dv(c0[1]), dv(c0[2]))] + [tuple(P['c%d.%s' % (k, n)] for n in O.RD.UPPER_KEYS) for k in range(1, L + 1)]
    return ops.fsrnn_seq(X['xg'], (X['Fh'], X['Fc'], X['Sh'], X['Sc']), W, L, dv(aux['mh']), dv(aux['mc']), dv(aux['dm']), aux['keep_h'], aux['keep_c'])[0]


def _run_bn(ops, P, X, aux):
    C = P['gamma'].shape[0]
    return ops.bn_lrelu(X['x'], P['gamma'], P['beta'], torch.zeros(C, device=DEV), torch.ones(C, device=DEV), True, aux['momentum'], aux['eps'], aux['slope'])


RUN = {
    'linear': _run_linear,
    'linear_ctc': _run_linear_ctc,
    'linear2': lambda ops, P, X, aux: ops.linear_2bias(X['x'], P['W'], P['b1'], P['b2']),
    'fbank_dense': lambda ops, P, X, aux: ops.fbank_dense(X['x'], P['W'], None if aux['cmvn'] is None else aux['cmvn'].to(DEV)),
    'mask_fc': lambda ops, P, X, aux: ops.mask_fc(X['proj'], P['W'], aux['mix'].to(DEV), _i32(aux['lens']), aux['T'])[0],
    'embedding': lambda ops, P, X, aux: ops.embedding(P['table'], aux['ids'].to(DEV)),
    'conv2d': _run_conv2d,
    'conv_transpose2d': lambda ops, P, X, aux: ops.conv_transpose2d(X['x'], P['Wt'], P['b'], 2, aux['pad']),
    'bn_lrelu': _run_bn,
    'bilstm': _run_bilstm,
    'decoder_loop': _run_decoder,
    'decoder_upper': lambda ops, P, X, aux: ops.DecoderUpperFn.apply(X['z0'], O._layers_of(P)),
    'lm_seq': lambda ops, P, X, aux: ops.lm_lstm_seq(X['xg'], P['w_hh'], X['h0'], X['c0'])[0],
    'fsrnn_seq': _run_fsrnn,
}


# ---------------------------------------------------------------------------------------------
# gradient storage
# ---------------------------------------------------------------------------------------------
class Flat(object):
    """One flat gradient buffer for a row's parameters, laid out as FlatOptimizer lays its own (every slice at a multiple of ALIGN floats),
    every float outside the slices a guard: at least O.GUARD of them before, between and after the gradients."""

    def __init__(self, P, scales):
        self.slices, n = {}, ALIGN
        for k, p in P.items():
            self.slices[k] = (n, p.numel())
            n += (p.numel() + O.GUARD + ALIGN - 1) // ALIGN * ALIGN
        g = torch.Generator().manual_seed(77)
        host = torch.full((n,), O.SENTINEL)
        self.is_guard = torch.ones(n, dtype=torch.bool)
        self.g0 = {}
        for k, p in P.items():
            off, m = self.slices[k]
            self.g0[k] = (torch.randn(m, generator=g) * scales[k]).view(p.shape)
            host[off:off + m] = self.g0[k].reshape(-1)
            self.is_guard[off:off + m] = False
        self.before = host[self.is_guard].clone()
        self.buf = host.to(DEV)
        for k, p in P.items():
            off, m = self.slices[k]
            p.grad = self.buf[off:off + m].view(p.shape)

    def guards(self):
        return self.before, self.buf.cpu()[self.is_guard]


def _scales(case, w64):
    """A prefill of about the gradient's own scale (1e-3 where the true gradient is zero)."""
    return {k: (float(w64[k].abs().max()) or 1e-3) for k in case['params']}


# ---------------------------------------------------------------------------------------------
# one run
# ---------------------------------------------------------------------------------------------
def _upstream(dy, form):
    """The upstream gradient as autograd hands it to the Function: a transposed view / a slice of a larger buffer with the values of dy."""
    if form == 'transposed':
        return dy.transpose(0, -1).contiguous().transpose(0, -1)
    if form == 'slice':
        big = torch.zeros(dy.shape[:-1] + (dy.shape[-1] + 5,), device=dy.device)
        big[..., 2:2 + dy.shape[-1]] = dy
        return big[..., 2:2 + dy.shape[-1]]
    return dy


def _params(case, off=()):
    return {k: torch.nn.Parameter(v.to(DEV), requires_grad=k not in off) for k, v in case['params'].items()}


def _go(row, case, P, uses=1, routed=False, frozen=(), flip=None, input_grad=True, form='plain', walks=1, expect_raise=False):
    """Forward(s) and backward(s) of the row on the device -> {parameter: .grad or None, 'd_<input>' / 'd2_<input>': input gradients}.
    routed: both uses under ops.routing(wgrad=Stream(), aux=Stream()), the second one on the aux stream, joined the way e2e_model.py joins
    its CTC branch.  frozen: parameter names under ops.frozen_params around the backward.  flip: {name: requires_grad} set between forward
    and backward.  form: the upstream gradient's form (P6).  walks: backward passes over the retained graph (P7)."""
    ops, lib = _ops()
    run = RUN[row.run]
    cases = [case, O.second_use(case)][:uses]
    aborts = lib.query('re2e_lstm_abort_count')
    padded_calls = []
    was_padded = ops._linear_backward_padded

    def counted(*a, **k):
        padded_calls.append(1)
        return was_padded(*a, **k)
    wgrad, aux_s = (torch.cuda.Stream(), torch.cuda.Stream()) if routed else (None, None)
    ys, dys, Xs = [], [], []
    with contextlib.ExitStack() as stack:
        if routed:
            stack.enter_context(ops.routing(wgrad=wgrad, aux=aux_s))
        for u, c in enumerate(cases):
            X = {k: v.to(DEV).requires_grad_(input_grad) for k, v in c['inputs'].items()}
            aux = dict(c['aux'], name=row.name)
            dy = c['dy'].to(DEV)
            if routed and u == 1:
                cur = torch.cuda.current_stream()
                aux_s.wait_stream(cur)
                with torch.cuda.stream(aux_s):
                    for t in list(X.values()) + [dy]:
                        t.record_stream(aux_s)
                    y = run(ops, P, X, aux)
                cur.wait_stream(aux_s)
                y.record_stream(cur)
            else:
                y = run(ops, P, X, aux)
            assert tuple(y.shape) == tuple(dy.shape), (row.name, y.shape, dy.shape)
            ys.append(y)
            dys.append(dy)
            Xs.append(X)
        for k, v in (flip or {}).items():
            P[k].requires_grad_(v)
        ops._linear_backward_padded = counted
        try:
            with ops.frozen_params([P[k] for k in frozen]):
                for walk in range(walks):
                    keep = walk + 1 < walks
                    if form == 'expanded':
                        assert uses == 1
                        ys[0].sum().backward(retain_graph=keep)
                        continue
                    grads = []
                    for y, dy, c in zip(ys, dys, cases):
                        pad = c['aux'].get('padded')
                        if pad and form == 'plain' and walk == 0:
                            # the gradient as CtcFn.backward hands it down: rows zero-padded to ``pad`` floats, the buffer registered
                            buf = torch.zeros(dy.shape[:-1] + (pad,), device=DEV)
                            buf[..., :dy.shape[-1]] = dy
                            ops._PADDED_GRADS[buf.data_ptr()] = (dy.numel() // dy.shape[-1], dy.shape[-1], pad)
                            grads.append(buf[..., :dy.shape[-1]])
                        else:
                            grads.append(_upstream(dy, form))
                    if expect_raise and walk == 1:
                        with pytest.raises(lib.Re2eError, match=row.fn):
                            torch.autograd.backward(ys, grads, retain_graph=keep)
                        break
                    torch.autograd.backward(ys, grads, retain_graph=keep)
        finally:
            ops._linear_backward_padded = was_padded
        if routed:
            torch.cuda.current_stream().wait_stream(wgrad)
    torch.cuda.synchronize()
    assert lib.query('re2e_lstm_abort_count') == aborts, 'a persistent kernel gave up'
    if (case['aux'].get('padded') or case['aux'].get('ctc')) and form == 'plain':
        assert len(padded_calls) == uses * (1 if case['aux'].get('padded') else walks), 'the _PADDED_GRADS branch of LinearFn.backward was not taken'
    got = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in P.items()}
    for u, X in enumerate(Xs):
        got.update({('d_' if u == 0 else 'd2_') + k: (v.grad.detach().cpu() if v.grad is not None else None) for k, v in X.items()})
    return got


def _verdict(row, cell, sub, got, want64, want32, g0, guards, bars):
    label = '%s %s %s%s' % (row.fn, row.name, cell, ('/' + sub) if sub else '')
    log = []
    bad = O.check_protocol(got, want64, want32, g0, guards, bars, label, log)
    print('\n'.join(log))
    return ['%s: %s' % (label, b) for b in bad]


def _setup(name, uses=1, ones=False):
    row, case = O.BY_NAME[name], _case(name)
    w64, w32 = _want(name, uses, ones)
    bars = _bars(row, case)
    O.margins(row, case, w64, w32, bars)
    return row, case, w64, w32, bars


@pytest.fixture(autouse=True)
def _switches(request, monkeypatch):
    """Per row: the decoder loop's form as the row names it; the embedding's block loop at 3 tokens a call."""
    name = request.node.callspec.params.get('name') if hasattr(request.node, 'callspec') else None
    if name is not None:
        ops, _ = _ops()
        row, case = O.BY_NAME[name], _case(name)
        if row.run == 'decoder_loop':
            monkeypatch.setattr(ops, 'DECODER_PERSIST', bool(case['aux']['persist']))
        if row.run == 'embedding':
            monkeypatch.setattr(ops, 'EMBEDDING_BWD_MAX_TOKENS', case['aux']['block'])


def _applies(cell):
    return [n for n in O.NAMES if cell not in O.BY_NAME[n].cells]


def test_every_cell_is_run_or_carries_a_reason():
    here = {'P1': test_p1_first_write, 'P2': test_p2_accumulate, 'P3': test_p3_two_uses, 'P3-routed': test_p3_two_uses_routed, 'P4': test_p4_choice_per_parameter,
            'P5': test_p5_no_input_gradient, 'P6': test_p6_upstream_forms, 'P7': test_p7_second_walk}
    assert set(here) == set(O.CELLS)
    for row in O.OPS:
        assert all(c in O.CELLS and reason for c, reason in row.cells.items())


# ---------------------------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', _applies('P1'))
def test_p1_first_write(name):
    """P1 first write.  ``p.grad is None`` gives a fresh ``p.grad`` equal to dL/dp.  Every element is written."""
    row, case, w64, w32, bars = _setup(name)
    P = _params(case)
    got = _go(row, case, P)
    assert not _verdict(row, 'P1', '', got, w64, w32, {}, None, bars)


@pytest.mark.parametrize('name', _applies('P2'))
def test_p2_accumulate(name):
    """P2 accumulate.  With ``p.grad = g0``, the result is ``g0 + dL/dp``.  Nothing outside ``p.grad``'s extent is written."""
    row, case, w64, w32, bars = _setup(name)
    P = _params(case)
    flat = Flat(P, _scales(case, w64))
    got = _go(row, case, P)
    assert not _verdict(row, 'P2', '', got, w64, w32, flat.g0, flat.guards(), bars)


@pytest.mark.parametrize('name', _applies('P3'))
def test_p3_two_uses(name):
    """P3 several uses.  A parameter used by two calls in one graph receives the sum."""
    row, case, w64, w32, bars = _setup(name, uses=2)
    P = _params(case)
    flat = Flat(P, _scales(case, w64))
    got = _go(row, case, P, uses=2)
    assert not _verdict(row, 'P3', '', got, w64, w32, flat.g0, flat.guards(), bars)


@pytest.mark.parametrize('name', _applies('P3-routed'))
def test_p3_two_uses_routed(name):
    """P3: the same holds when the second call and the weight-gradient kernels run on other streams under ``ops.routing(wgrad=..., aux=...)``.
    One run: a correctness check of the event ordering, not a stress test."""
    row, case, w64, w32, bars = _setup(name, uses=2)
    P = _params(case)
    flat = Flat(P, _scales(case, w64))
    got = _go(row, case, P, uses=2, routed=True)
    assert not _verdict(row, 'P3-routed', '', got, w64, w32, flat.g0, flat.guards(), bars)


@pytest.mark.parametrize('name', _applies('P4'))
def test_p4_choice_per_parameter(name):
    """P4 graph-time choice, per parameter.  A parameter gets a gradient only if it required one when the forward ran and is not in
    ``FROZEN_PARAMS`` when the backward runs.  A change to ``requires_grad`` between forward and backward changes nothing.  An excluded
    parameter's ``.grad`` stays bit-identical.  The input gradient and the other parameters' gradients are unaffected."""
    row, case, w64, w32, bars = _setup(name)
    bad = []
    for gname, group in O.groups_of(row, case).items():
        out = {k: (None if k in group else v) for k, v in w64.items()}
        forms = (('off-at-build', dict(off=group), {}, out),
                 ('frozen', {}, dict(frozen=group), out),
                 ('off-at-build-flipped-on', dict(off=group), dict(flip={k: True for k in group}), out),
                 ('flipped-off', {}, dict(flip={k: False for k in group}), w64))
        if len(group) == len(case['params']) and not case['inputs']:
            forms = forms[1:2] + forms[3:]          # (nothing left that needs a gradient: no graph to walk)
        for fname, pkw, gkw, want in forms:
            P = _params(case, **pkw)
            flat = Flat(P, _scales(case, w64))
            got = _go(row, case, P, **gkw)
            bad += _verdict(row, 'P4', '%s/%s' % (gname, fname), got, want, w32, flat.g0, flat.guards(), bars)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', _applies('P5'))
def test_p5_no_input_gradient(name):
    """P5 no input gradient.  When the data input needs no gradient, the parameter gradients are still right."""
    row, case, w64, w32, bars = _setup(name)
    P = _params(case)
    flat = Flat(P, _scales(case, w64))
    got = _go(row, case, P, input_grad=False)
    assert all(got['d_' + k] is None for k in case['inputs'])
    want = {k: v for k, v in w64.items() if k in case['params']}
    assert not _verdict(row, 'P5', '', got, want, w32, flat.g0, flat.guards(), bars)


@pytest.mark.parametrize('name', _applies('P6'))
def test_p6_upstream_forms(name):
    """P6 upstream forms.  ``dy`` may be non-contiguous: a transposed view, an expanded scalar (``y.sum().backward()``), a slice of a larger
    buffer."""
    bad = []
    for form in ('transposed', 'slice', 'expanded'):
        if form == 'expanded' and O.BY_NAME[name].zero_dy:
            print('P6/expanded left out for %s: %s' % (name, O.BY_NAME[name].zero_dy))
            continue
        row, case, w64, w32, bars = _setup(name, ones=form == 'expanded')
        P = _params(case)
        flat = Flat(P, _scales(case, w64))
        got = _go(row, case, P, form=form)
        bad += _verdict(row, 'P6', form, got, w64, w32, flat.g0, flat.guards(), bars)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', _applies('P7'))
def test_p7_second_walk(name):
    """P7 second walk.  On a retained graph, an op whose backward destroys its saved state raises ``Re2eError``.  The message names the op.
    Every other op gives the same gradient again, so it accumulates twice."""
    row, case, w64, w32, bars = _setup(name)
    P = _params(case)
    got = _go(row, case, P, walks=2, expect_raise=row.destroys)
    times = 1 if row.destroys else 2
    assert not _verdict(row, 'P7', 'raises' if row.destroys else 'twice', got, {k: times * v for k, v in w64.items()},
                        {k: times * v for k, v in w32.items()}, {}, None, bars)
