"""The loss side of the step -- csrc/ctc.hip, seqloss.hip, attloc.hip, decloop.hip -- against the float64 references of tests/refs64.py,
at the smallest shapes that reach each branch of each kernel (every log-sum-exp kernel of the CTC forward and both sides of its
thresholds, two and three wavefronts of extended-label states, repeats, single-path and empty label sequences, padded gradient rows,
infeasible alignments; the row kernels of seqloss.hip at one lane pass, one full pass, one past it and the production vocabulary; the
decoder loop in both of its forms at widths where every slice / chunk / unroll / channel-group loop takes more than one trip).

The bars are the project's own (refs64.BAR_*).  Each test first asserts that torch's fp32 CPU run of the same reference stays within a
quarter of the bar on its input, then prints, per quantity, the HIP kernel's and that fp32 run's distance from float64.  GPU only.

Measured on an MI355X when the module was written, worst case per quantity, HIP / fp32 on the CPU (of the tensor's max):
    CTC loss, nll 5e-7 / 4e-7 (bar 1e-5); CTC gradient 2.6e-5 / 1.4e-5 (bar 1e-4; three wavefronts, next 1.4e-5 at V = 4608)
    cross-entropy, label smoothing: value 7e-7 / 1e-7 (1e-5), gradient 1.7e-6 / 2e-7 (1e-4); embedding gradient 3e-7 / 3e-7;
    log_softmax rows 6e-8 / 8e-8
    decoder, launch per step: states 9e-7 / 1.8e-6, weights 4e-7 / 4e-7 (2e-4), gradients 2.5e-6 (6.5e-6 with a gradient on w) / 3e-6 (3e-4)
    decoder, persistent:      states 2.7e-6,        weights 8e-7,               gradients 3.7e-6; |d gvec_b| <= 8.4e-6 (bar 1e-5 L1 B = 1.5e-4)"""
import functools

import numpy as np
import pytest
import torch

import refs64 as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ops():
    from robust_e2e_gan_amd import ops, lib
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    return ops, lib


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _held(case, name, got, f64, f32, bar, atol=0.0):
    """Precondition (fp32 CPU within a quarter of the bar), then the HIP result within the bar of float64; prints both distances."""
    cpu = R.margin_ok(name, f32, f64, bar, atol)
    err = R.rel_err(got, f64)
    scale = f64.detach().double().abs().max().item()
    print('ERR %-46s %-16s hip %.2e  fp32-cpu %.2e  bar %.0e' % (case, name, err, cpu, bar))
    assert err * scale <= bar * scale + atol, '%s %s: HIP is %.3e of the max from float64 (bar %.1e, fp32 on the CPU: %.3e)' % (case, name, err, bar, cpu)


# ---------------------------------------------------------------------------------------------
# CTC
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ctc_refs(name):
    c = R.ctc_infeasible_case() if name == 'infeasible' else R.ctc_cases()[name]
    return c, R.ctc_ref(c['logits'], c['hlens'], c['labels']), R.ctc_ref(c['logits'], c['hlens'], c['labels'], torch.float32)


def _ctc_args(c):
    ll = [len(l) for l in c['labels']]
    flat = _i32([v for l in c['labels'] for v in l])
    off = _i32(np.concatenate([[0], np.cumsum(ll)[:-1]]))
    return _i32(c['hlens']), flat, off, _i32(ll), max(ll)


def _ctc_hip(c):
    """-> loss (1,), nll per utterance (B,), d (gscale * loss) / d logits (T,B,V), through ops.ctc_loss."""
    ops, lib = _ops()
    lg = c['logits'].to(DEV).requires_grad_(True)
    loss = ops.ctc_loss(lg, *_ctc_args(c))
    nll = loss.grad_fn.saved_tensors[2]
    (loss * c['gscale']).sum().backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), nll.detach().cpu(), lg.grad.cpu()


def _ctc_hip_ldd(c):
    """The same through the C ABI with gradient rows of ldd > V floats, into a buffer prefilled with NaN."""
    ops, lib = _ops()
    T, B, V, ldd = c['T'], c['B'], c['V'], c['ldd']
    hl, flat, off, ll, Lmax = _ctc_args(c)
    lg = c['logits'].to(DEV)
    wsb = lib.query('re2e_ctc_workspace_bytes', T, B, Lmax)
    ws = torch.empty(wsb // 4 + 4, dtype=torch.float32, device=DEV)
    loss, nll = torch.empty(1, device=DEV), torch.empty(B, device=DEV)
    lib.call('re2e_ctc_fwd', lg.data_ptr(), T, B, V, hl.data_ptr(), flat.data_ptr(), off.data_ptr(), ll.data_ptr(), Lmax, loss.data_ptr(), nll.data_ptr(),
             ws.data_ptr(), wsb)
    g = torch.tensor([c['gscale']], dtype=torch.float32, device=DEV)
    d = torch.full((T, B, ldd), float('nan'), dtype=torch.float32, device=DEV)
    lib.call('re2e_ctc_bwd', lg.data_ptr(), T, B, V, hl.data_ptr(), flat.data_ptr(), off.data_ptr(), ll.data_ptr(), Lmax, nll.data_ptr(), g.data_ptr(),
             d.data_ptr(), ldd, ws.data_ptr())
    torch.cuda.synchronize()
    return loss.cpu(), nll.cpu(), d.cpu()


@pytest.mark.parametrize('name', list(R.ctc_cases()))
def test_ctc_against_float64(name):
    c, (n64, l64, d64), (n32, l32, d32) = _ctc_refs(name)
    loss, nll, d = _ctc_hip_ldd(c) if c['ldd'] else _ctc_hip(c)
    V = c['V']
    if c['ldd']:
        assert torch.isfinite(d).all(), 'NaN left in the padded gradient buffer'
        assert (d[..., V:] == 0).all(), 'padding columns must be written as zeros'
        d = d[..., :V]
    _held(name, 'loss', loss.view(()), l64, l32, R.BAR_LOSS)
    _held(name, 'nll_per_utt', nll, n64, n32, R.BAR_LOSS)
    _held(name, 'dlogits', d, d64 * c['gscale'], d32 * c['gscale'], R.BAR_GRAD)
    for b, h in enumerate(c['hlens']):
        assert (d[h:, b] == 0).all(), 'rows at or beyond hlens[%d] must be exact zeros' % b
        assert d[:h, b].abs().max() > 0


def test_ctc_infeasible_alignment_is_inf_loss_and_nan_rows():
    """hlen < L + repeats: F.ctc_loss answers nll = +inf with NaN gradient rows for that utterance, and so must the kernel -- a finite loss
    with finite, wrong rows passes the finite check on the gradient norm and is applied.  The feasible utterances beside it are unaffected."""
    c, (n64, l64, d64), (n32, l32, d32) = _ctc_refs('infeasible')
    loss, nll, d = _ctc_hip(c)
    assert not torch.isfinite(loss).any() and not torch.isfinite(l64)
    for b, h in enumerate(c['hlens']):
        if b in c['infeasible']:
            assert nll[b] == float('inf'), (b, nll[b])
            assert torch.isnan(d[:h, b]).all(), 'gradient rows of utterance %d must be NaN' % b
        else:
            assert torch.isfinite(d[:h, b]).all()
        assert (d[h:, b] == 0).all()
    ok = [b for b in range(c['B']) if b not in c['infeasible']]
    _held('infeasible', 'nll (others)', nll[ok], n64[ok], n32[ok], R.BAR_LOSS)
    _held('infeasible', 'dlogits (others)', d[:, ok], d64[:, ok] * c['gscale'], d32[:, ok] * c['gscale'], R.BAR_GRAD)


# ---------------------------------------------------------------------------------------------
# seqloss.hip
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R_,V', R.SEQLOSS_SHAPES)
def test_cross_entropy_against_float64(R_, V):
    ops, lib = _ops()
    c = R.seqloss_case(R_, V)
    l64, k64, v64, d64 = R.ce_ref(c['x'], c['targets'], c['scale'])
    l32, k32, v32, d32 = R.ce_ref(c['x'], c['targets'], c['scale'], torch.float32)
    lg = c['x'].to(DEV).requires_grad_(True)
    loss, stats = ops.cross_entropy(lg, c['targets'].to(DEV), c['scale'])
    (loss * c['g']).sum().backward()
    torch.cuda.synchronize()
    case = 'ce-%dx%d' % (R_, V)
    _held(case, 'loss', loss.view(()), l64, l32, R.BAR_LOSS)
    _held(case, 'stats[0]', stats[0], l64, l32, R.BAR_LOSS)
    assert (int(stats[1]), int(stats[2])) == (k64, v64), 'correct / valid rows: %s, float64 counts %s' % (stats.tolist(), (k64, v64))
    _held(case, 'dlogits', lg.grad, d64 * c['g'], d32 * c['g'], R.BAR_GRAD)
    ignored = c['targets'] < 0
    assert ignored.any() and (lg.grad.cpu()[ignored] == 0).all(), 'ignored rows must be exact zeros'


@pytest.mark.parametrize('R_,V', R.SEQLOSS_SHAPES)
def test_label_smoothing_against_float64(R_, V):
    ops, lib = _ops()
    c = R.seqloss_case(R_, V)
    assert (c['dist'] == 0).any() and abs(float(c['dist'].sum()) - 1.0) > 0.05 and c['nutt'] != R_
    r64, e64 = R.lsm_ref(c['x'], c['dist'], c['nutt'])
    r32, e32 = R.lsm_ref(c['x'], c['dist'], c['nutt'], torch.float32)
    lg = c['x'].to(DEV).requires_grad_(True)
    reg = ops.label_smoothing(lg, c['dist'].to(DEV), c['nutt'])
    (reg * c['g']).sum().backward()
    torch.cuda.synchronize()
    case = 'lsm-%dx%d' % (R_, V)
    _held(case, 'value', reg.view(()), r64, r32, R.BAR_LOSS)
    _held(case, 'dlogits', lg.grad, e64 * c['g'], e32 * c['g'], R.BAR_GRAD)


@pytest.mark.parametrize('n,D', R.EMB_CASES)
def test_embedding_gradient_against_float64(n, D):
    ops, lib = _ops()
    c = R.embedding_case(n, D)
    V, ldo = c['V'], c['ldo']
    dout, ids = c['dout'].to(DEV), c['ids'].to(DEV)
    for beta in (0.0, 1.0):
        ref = R.embedding_bwd_ref(c['dout'][:, :D], c['ids'], V, beta, c['prev'])
        r32 = R.embedding_bwd_ref(c['dout'][:, :D], c['ids'], V, beta, c['prev'], torch.float32)
        runs = []
        for _ in range(2):
            out = torch.full((V, D), float('nan'), device=DEV) if beta == 0.0 else c['prev'].to(DEV)
            lib.call('re2e_embedding_bwd', dout.data_ptr(), ldo, ids.data_ptr(), n, D, V, out.data_ptr(), beta)
            torch.cuda.synchronize()
            runs.append(out.cpu())
        _held('emb-n%d-D%d-beta%d' % (n, D, int(beta)), 'dtable', runs[0], ref, r32, R.BAR_GRAD)
        assert torch.equal(runs[0], runs[1]), 'the fixed summation order must give the same bits twice'
        if beta == 0.0:
            assert (runs[0][7:] == 0).all(), 'table rows nobody hits must come out as zeros'


@pytest.mark.parametrize('R_,V', R.SEQLOSS_SHAPES)
def test_log_softmax_and_argmax_rows_against_float64(R_, V):
    """Rows of ldx > V floats whose padding holds values that would win every maximum; R is no multiple of 4 in three of the shapes."""
    ops, lib = _ops()
    c = R.seqloss_case(R_, V)
    ldx = V + 5
    xp = torch.full((R_, ldx), 1.0e9)
    xp[:, :V] = c['x']
    xd = xp.to(DEV)
    out = torch.full((R_ + 1, V), float('nan'), device=DEV)
    am = torch.full((R_ + 1,), -7, dtype=torch.int32, device=DEV)
    lib.call('re2e_log_softmax_rows', xd.data_ptr(), R_, V, ldx, out.data_ptr())
    lib.call('re2e_argmax_rows', xd.data_ptr(), R_, V, ldx, am.data_ptr())
    torch.cuda.synchronize()
    case = 'rows-%dx%d' % (R_, V)
    _held(case, 'log_softmax', out[:R_], c['x'].double().log_softmax(1), c['x'].log_softmax(1), R.BAR_LOSS)
    want = R.argmax_first(c['x'].double())
    assert want[[0, 2, 3]].tolist() == [1, 0, 0]            # the three tie rows of the case
    assert am[:R_].cpu().tolist() == want.tolist()
    assert torch.isnan(out[R_]).all() and int(am[R_]) == -7, 'a row past R was written'


# ---------------------------------------------------------------------------------------------
# decoder loop, both forms
# ---------------------------------------------------------------------------------------------
def _dec_params():
    ps = []
    for shape, takes, _ in R.DEC_SHAPES:
        sid = 'x'.join(str(v) for v in shape)
        if takes == 'none':
            ps.append(pytest.param(shape, takes, False, id=sid + '-stepwise-only-persistent-form-declines'))
            continue
        ps.append(pytest.param(shape, takes, False, id=sid + '-stepwise'))
        ps.append(pytest.param(shape, takes, True, id=sid + ('-persistent' if takes == 'both' else '-persistent-forward-stepwise-backward')))
    return ps


@functools.lru_cache(maxsize=None)
def _dec_case(shape):
    return R.decoder_case(shape)


@functools.lru_cache(maxsize=None)
def _dec_refs(shape, upstream):
    c = _dec_case(shape)
    return R.decoder_ref_run(c, upstream=upstream), R.decoder_ref_run(c, torch.float32, upstream)


@pytest.mark.parametrize('upstream', R.DEC_UPSTREAM)
@pytest.mark.parametrize('shape,takes,persist', _dec_params())
def test_decoder_loop_against_float64(shape, takes, persist, upstream):
    """ops.DecoderLoopFn (launch per step: csrc/attloc.hip + the fused gates / cell kernels; persistent: csrc/decloop.hip) against the
    written-out float64 loop on the same inputs: states, attention weights, and the gradients of the encoder states, of their
    projection and of every entry of Pm under a random upstream gradient on the states ('zs': what the model does; the attention
    weights are then a non-differentiable output) and on the states and the attention weights ('zs+w', ``w_grad=True``: the softmax
    backward of EVERY step then has a ``dw_in``, the last one too, and the recurrence's own is added to it; the persistent reverse
    loop has no input for it, so that backward runs launch per step after either forward)."""
    ops, lib = _ops()
    B, T, L1, E, A, D, C, Fh = shape
    fwd_ws = lib.query('re2e_dec_loop_workspace_bytes', L1, B, T, E, D, A, C, Fh)
    bwd_ws = lib.query('re2e_dec_loop_bwd_workspace_bytes', L1, B, T, E, D, A, C, Fh)
    assert (fwd_ws > 0, fwd_ws > 0 and bwd_ws > 0) == (takes != 'none', takes == 'both'), \
        'the persistent form takes something else of this shape than the test id says: workspaces %d / %d' % (fwd_ws, bwd_ws)
    c, (f64, f32) = _dec_case(shape), _dec_refs(shape, upstream)
    hm, pr = c['hmask'].to(DEV).requires_grad_(True), c['pre'].to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in c['Pm'].items()}
    aborts = lib.query('re2e_lstm_abort_count')           # (per process: tests of the give-up protocol before this one leave it above zero)
    was = ops.DECODER_PERSIST
    ops.DECODER_PERSIST = persist
    try:
        if upstream == 'zs':
            zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm)
            assert not w.requires_grad
            up = (zs * c['gz'].to(DEV)).sum()
        else:
            zs, w = ops.DecoderLoopFn.apply(hm, pr, c['ids'].to(DEV), _i32(c['hlens']), L1, Pm, None, True)
            up = (zs * c['gz'].to(DEV)).sum() + (w * c['gw'].to(DEV)).sum()
        assert getattr(zs.grad_fn, 'persist', persist) == persist
        up.backward()
        torch.cuda.synchronize()
    finally:
        ops.DECODER_PERSIST = was
    assert lib.query('re2e_lstm_abort_count') == aborts, 'the persistent loop gave up'
    case = 'dec-%s-%s-%s' % ('x'.join(str(v) for v in shape), 'persist' if persist else 'step', upstream)
    _held(case, 'zs', zs, f64['zs'], f32['zs'], R.BAR_DEC_OUT)
    _held(case, 'w', w, f64['w'], f32['w'], R.BAR_DEC_OUT)
    got = dict(d_enc=hm.grad, d_pre=pr.grad, **{k: v.grad for k, v in Pm.items()})
    assert all(got[k] is not None for k in R.DEC_KEYS)
    bad = []
    for k in sorted(got):
        if k == 'gvec_b':           # true gradient zero (a shift of the energies does not move a softmax): rounding noise of a sum over all frames
            err = got[k].abs().max().item()
            print('ERR %-46s %-16s hip %.2e (absolute; float64 %.1e)' % (case, k, err, f64[k].abs().max().item()))
            if not err <= 1e-5 * float(L1 * B):
                bad.append(k)
            continue
        try:
            _held(case, k, got[k], f64[k], f32[k], R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
        except AssertionError as e:
            if 'input too hard' in str(e):
                raise
            bad.append(k)
    assert not bad, bad
