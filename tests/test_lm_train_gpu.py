"""Training the language model on the GPU (model/lm.py forward_seq / forward / train / evaluate over csrc/lmseq.hip) against
tests/golden/lm_train_tiny.npz, which the reference wrote on the CPU (make_fixtures_lm_train.py), within the README's 1e-3 parity bar:
one window three ways (forward_seq, the reference's per-step loop, two chained windows), three training iterations with a clipped and
an unclipped step, the validation perplexity, and ``train(args)`` end to end.  Beside the fixture: the fused recurrence against the
composed one within the kernel bars, the chunked output layer against the unchunked one, and live dropout against the float64 model of
tests/refs64_lm.py with the masks of oracle/philox.py.  GPU only."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs64_lm as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

BAR = 1e-3          # README: losses and gradients within 1e-3 of the reference's fp32 CPU path
V, I, H = 11, 6, 10


@pytest.fixture(scope='module')
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'lm_train_tiny.npz')))


def _model(fx, prefix='lm.', dropout=0.0, dims=(V, I, H)):
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    m = ClassifierWithState(RNNLM(*dims, dropout_rate=dropout))
    if fx is not None:
        res = m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix + 'predictor.')}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    m.compute_accuracy = False
    return m.to(DEV).train()


def _close(name, got, want, bar=BAR):
    got, want = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(want).detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    err, scale = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-30)
    print('PARITY %-40s %.2e of max (bar %.0e)' % (name, err / scale, bar))
    assert err <= bar * scale, '%s: %.3e of the max from the reference (bar %.1e)' % (name, err / scale, bar)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _check_window(fx, m, losses, state, tag):
    if losses is not None:
        _close(tag + ' losses', losses, fx['win.losses'])
    for k in R.STATE_KEYS:
        _close('%s state %s' % (tag, k), state[k], fx['win.state.' + k])
    g = _grads(m)
    assert len(g) == 11
    for k, v in g.items():
        _close('%s grad %s' % (tag, k), v, fx['win.grad.' + k])


def test_window_through_forward_seq(fx):
    _ops()
    m = _model(fx)
    xs, ts = fx['win.xs'], fx['win.ts']
    state, logits = m.predictor.forward_seq(None, xs)
    assert tuple(logits.shape) == (4, 3, V)
    ref = R.lm_model_ref({k: torch.from_numpy(fx['lm.predictor.' + k]) for k in R.PARAM_NAMES}, xs, ts)
    _close('forward_seq logits', logits, ref['logits'])
    m2 = _model(fx)
    state, loss = m2.forward_seq(None, xs, ts)
    assert loss.dim() == 0 and m2.loss is loss and tuple(m2.y.shape) == (4, 3, V)
    _close('forward_seq loss', loss, fx['win.losses'].sum())
    loss.backward()
    _check_window(fx, m2, None, state, 'forward_seq')


def test_window_through_the_per_step_loop(fx):
    """The reference's loop: four ``forward`` calls in training mode, losses summed, one backward: chains through the state's gradient."""
    _ops()
    m = _model(fx)
    m.compute_accuracy = True
    state, losses, loss = None, [], 0
    for t in range(4):
        state, l = m(state, torch.from_numpy(fx['win.xs'][t]).long(), torch.from_numpy(fx['win.ts'][t]).long())
        assert l.dim() == 0 and tuple(m.y.shape) == (3, V) and 0.0 <= float(m.accuracy) <= 1.0
        losses.append(float(l.detach()))
        loss = loss + l
    m.zero_grad()
    loss.backward()
    _check_window(fx, m, losses, state, 'per-step')
    ref = R.lm_model_ref({k: torch.from_numpy(fx['lm.predictor.' + k]) for k in R.PARAM_NAMES}, fx['win.xs'], fx['win.ts'])
    assert abs(float(m.accuracy) - float((ref['logits'][3].argmax(1) == torch.from_numpy(fx['win.ts'][3]).long()).float().mean())) < 1e-6


def test_window_through_two_chained_windows(fx):
    """T = 2 + 2 without detaching: the gradient of the second window reaches the first through h0 / c0 of both layers."""
    _ops()
    m = _model(fx)
    xs, ts = fx['win.xs'], fx['win.ts']
    state, l0 = m.forward_seq(None, xs[:2], ts[:2])
    assert all(v.requires_grad for v in state.values())
    state, l1 = m.forward_seq(state, xs[2:], ts[2:])
    _close('chained loss', l0 + l1, fx['win.losses'].sum())
    (l0 + l1).backward()
    _check_window(fx, m, None, state, 'chained')


@pytest.mark.parametrize('dims,T,B', [((V, I, H), 4, 3), ((20, 9, 33), 3, 65)], ids=['fixture', 'V20-I9-H33-T3-B65'])
def test_fused_and_composed_arms_agree(fx, dims, T, B, monkeypatch):
    """The window over csrc/lmseq.hip against the same window over re2e_gemm + re2e_lstm_cell_fwd / _bwd per step, within the kernel bars
    (1e-4 of the max for the loss and the state, 2e-4 for gradients), from a non-zero state and with a gradient through the final state."""
    _ops()
    from robust_e2e_gan_amd.model import lm
    g = torch.Generator().manual_seed(17)
    m = _model(fx if dims == (V, I, H) else None, dims=dims)
    if dims != (V, I, H):
        for p in m.parameters():
            p.data.copy_(torch.rand(p.shape, generator=g) - 0.5)
    xs, ts = torch.randint(0, dims[0], (T, B), generator=g).numpy(), torch.randint(0, dims[0], (T, B), generator=g).numpy()
    st0 = {k: (torch.tanh(torch.randn(B, dims[2], generator=g)) * 0.8).to(DEV) for k in R.STATE_KEYS}
    wout = {k: torch.randn(B, dims[2], generator=g).to(DEV) * 0.3 for k in R.STATE_KEYS}
    runs = []
    for composed in (False, True):
        monkeypatch.setattr(lm, 'COMPOSED_PATH', composed)
        m.zero_grad()
        st = {k: v.clone().requires_grad_(True) for k, v in st0.items()}
        state, loss = m.forward_seq(st, xs, ts)
        (loss + sum((state[k] * wout[k]).sum() for k in R.STATE_KEYS)).backward()
        runs.append((loss.detach(), {k: v.detach() for k, v in state.items()}, _grads(m), {k: v.grad.clone() for k, v in st.items()}))
    (lf, sf, gf, df), (lc, sc, gc, dc) = runs
    _close('fused vs composed loss', lf, lc, 1e-4)
    for k in R.STATE_KEYS:
        _close('fused vs composed state ' + k, sf[k], sc[k], 1e-4)
        _close('fused vs composed d state ' + k, df[k], dc[k], 2e-4)
    for k in gf:
        _close('fused vs composed grad ' + k, gf[k], gc[k], 2e-4)


def test_chunked_output_layer_equals_unchunked(fx, monkeypatch):
    """OUTPUT_MAX_ELEMS lowered to 5 rows' worth of logits: 12 rows run as blocks of 5, 5 and 2.  Same per-row arithmetic, another order of
    the sums into the loss and into lo.weight.grad / lo.bias.grad: a few fp32 roundings, bar 1e-5 of the max.  The embedding's gradient
    runs in blocks of 5 rows in the same pass (ops.EMBEDDING_BWD_MAX_TOKENS: re2e_embedding_bwd takes 15 000 rows a call)."""
    _ops()
    from robust_e2e_gan_amd import ops
    from robust_e2e_gan_amd.model import lm
    xs, ts = fx['win.xs'], fx['win.ts']
    calls = []
    real = ops.cross_entropy
    monkeypatch.setattr(ops, 'cross_entropy', lambda logits, *a, **kw: (calls.append(logits.shape[0]), real(logits, *a, **kw))[1])
    runs = []
    for limit, emb_rows in ((lm.OUTPUT_MAX_ELEMS, ops.EMBEDDING_BWD_MAX_TOKENS), (5 * V, 5)):
        monkeypatch.setattr(lm, 'OUTPUT_MAX_ELEMS', limit)
        monkeypatch.setattr(ops, 'EMBEDDING_BWD_MAX_TOKENS', emb_rows)          # the embedding's gradient in blocks of rows as well
        del calls[:]
        m = _model(fx)
        m.compute_accuracy = True
        state, loss = m.forward_seq(None, xs, ts)
        loss.backward()
        runs.append((loss.detach(), state, _grads(m), float(m.accuracy), list(calls)))
    assert runs[0][4] == [12] and runs[1][4] == [5, 5, 2]
    _close('chunked loss', runs[1][0], runs[0][0], 1e-5)
    _close('chunked loss vs fixture', runs[1][0], fx['win.losses'].sum())
    assert abs(runs[0][3] - runs[1][3]) < 1e-6
    for k in runs[0][2]:
        _close('chunked grad ' + k, runs[1][2][k], runs[0][2][k], 1e-5)
    for k in R.STATE_KEYS:
        assert torch.equal(runs[0][1][k], runs[1][1][k])


def test_dropout_window_against_float64_with_philox_masks(fx):
    """p = 0.5: three masks per window, drawn in the order d0, d1, d2 at (seed, call), (seed, call + 1), (seed, call + 2), each over its
    whole (T, B, .) tensor.  The float64 model with those masks is the yardstick; torch's fp32 CPU run of it must stay within a quarter
    of the bar."""
    ops, _ = _ops()
    from oracle.philox import dropout_mask
    xs, ts = fx['win.xs'], fx['win.ts']
    T, B = xs.shape
    seed, call = 0xC0FFEE1234, 7
    ops.dropout_seed(seed, call)
    m = _model(fx, dropout=0.5)
    state, loss = m.forward_seq(None, xs, ts)
    loss.backward()
    assert ops.dropout_state() == (seed, call + 3)
    masks = [torch.from_numpy(dropout_mask(T * B * w, 0.5, seed, call + i)).view(T, B, w) for i, w in enumerate((I, H, H))]
    assert all(0.2 < float((mk == 0).float().mean()) < 0.8 for mk in masks)
    params = {k: torch.from_numpy(fx['lm.predictor.' + k]) for k in R.PARAM_NAMES}
    r64, r32 = R.lm_model_ref(params, xs, ts, masks=masks), R.lm_model_ref(params, xs, ts, masks=masks, dtype=torch.float32)
    plain = R.lm_model_ref(params, xs, ts)
    assert abs(float(r64['loss']) - float(plain['loss'])) > 100 * BAR          # the masks matter at this size
    R.margin_ok('loss', r32['loss'], r64['loss'], BAR)
    _close('dropout loss', loss, r64['loss'])
    for k in R.STATE_KEYS:
        R.margin_ok(k, r32[k], r64[k], BAR)
        _close('dropout state ' + k, state[k], r64[k])
    for k, v in _grads(m).items():
        name = k[len('predictor.'):]
        R.margin_ok(name, r32['grad.' + name], r64['grad.' + name], BAR)
        _close('dropout grad ' + name, v, r64['grad.' + name])
    # evaluation mode draws nothing
    m.eval()
    with torch.no_grad():
        m.predictor.forward_seq(None, xs)
    assert ops.dropout_state() == (seed, call + 3)


def test_three_training_iterations_follow_the_fixture(fx):
    """The trainer's loop body -- next_window, forward_seq, zero_grad, backward, detach, clip at gradclip, SGD lr 1.0 -- from the
    fixture's parameters: loss, gradient norm and all parameters after each iteration; iteration 0 and 1 are clipped, iteration 2 is not."""
    _ops()
    from robust_e2e_gan_amd.data.lm_data_loader import ParallelSequentialIterator
    from robust_e2e_gan_amd.model.lm import evaluate
    from robust_e2e_gan_amd.optim import FlatOptimizer
    m = _model(fx)
    opt = FlatOptimizer(m.parameters(), kind='sgd', lr=1.0)
    it = ParallelSequentialIterator(fx['train.corpus'], 4)
    clip, state, coefs = float(fx['train.gradclip']), None, []
    for k in range(3):
        xs, ts = it.next_window(3)
        state, loss = m.forward_seq(state, xs, ts)
        opt.zero_grad()
        loss.backward()
        state = {n: v.detach() for n, v in state.items()}
        norm = opt.clip_grad_norm(clip)
        opt.step()
        coefs.append(float(opt.stats[1]))
        _close('it%d loss' % k, loss, fx['train.it%d.loss' % k])
        _close('it%d norm' % k, norm, fx['train.it%d.norm' % k])
        for n, p in m.state_dict().items():
            _close('it%d %s' % (k, n), p, fx['train.it%d.%s' % (k, n)])
    assert coefs[0] < 1.0 and coefs[2] == 1.0, coefs
    moved = max(float(np.abs(fx['train.it2.' + n] - fx['lm.' + n]).max()) for n in m.state_dict())
    assert moved > 100 * BAR                     # a trainer that did not update would not pass
    ppl = evaluate(m, ParallelSequentialIterator(fx['train.valid'], 4, repeat=False))
    print('PARITY validation perplexity %.6f vs %.6f' % (ppl, float(fx['train.valid_ppl'])))
    assert abs(ppl - float(fx['train.valid_ppl'])) <= BAR * float(fx['train.valid_ppl'])
    assert m.predictor.training                  # evaluate leaves the predictor in training mode, as the reference does


def test_train_writes_checkpoints_that_decode(fx, tmp_path, monkeypatch):
    """train(args) on the tiny corpus for one epoch: rnnlm.model.0, rnnlm.state.0 and the rnnlm.model.best link; the state dict loads
    strictly into a fresh ClassifierWithState(RNNLM); in evaluation mode its ``predict`` over the few-row kernels of csrc/rnnlm.hip equals
    the composed path on the trained weights; a second call resumes from rnnlm.model.best."""
    _ops()
    from robust_e2e_gan_amd.model import lm
    chars = [str(i) for i in range(V)]
    (tmp_path / 'train.txt').write_text(' '.join(chars[i] for i in fx['train.corpus']) + '\n')
    (tmp_path / 'valid.txt').write_text(' '.join(chars[i] for i in fx['train.valid']) + '\n')
    args = argparse.Namespace(ngpu=1, outdir=str(tmp_path), seed=1, train_label=str(tmp_path / 'train.txt'), valid_label=str(tmp_path / 'valid.txt'),
                              lm_type='rnnlm', batchsize=4, bproplen=3, epoch=1, gradclip=5.0, input_unit=I, unit=H, dropout_rate=0.2,
                              embed_init_file='', n_vocab=V, char_list_dict={c: i for i, c in enumerate(chars)})
    ppl = lm.train(args)
    assert ppl is not None and np.isfinite(ppl) and 1.0 < ppl < 1e4
    assert (tmp_path / 'rnnlm.model.0').is_file() and (tmp_path / 'rnnlm.state.0').is_file()
    best = tmp_path / 'rnnlm.model.best'
    assert best.is_symlink() and os.readlink(str(best)) == 'rnnlm.model.0'
    sd = torch.load(str(best), map_location='cpu')
    assert set(sd) == {'predictor.' + k for k in R.PARAM_NAMES}
    init = lm.ClassifierWithState(lm.RNNLM(V, I, H)).state_dict()
    assert all(tuple(sd[k].shape) == tuple(init[k].shape) and sd[k].device.type == 'cpu' and sd[k].untyped_storage().nbytes() == sd[k].numel() * 4 for k in sd)
    fresh = lm.ClassifierWithState(lm.RNNLM(V, I, H))
    res = fresh.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    ids = np.array([1, 5, 9], np.int32)
    out = []
    for composed in (False, True):
        monkeypatch.setattr(lm, 'COMPOSED_PATH', composed)
        state, lp = fresh.predict(None, ids)
        state, lp2 = fresh.predict(state, ids[::-1].copy())
        out.append((lp, lp2))
    monkeypatch.setattr(lm, 'COMPOSED_PATH', False)
    for a, b in zip(*out):
        _close('predict fused vs composed', a, b, 1e-4)
    assert abs(float(torch.logsumexp(out[0][1], 1)[0])) < 1e-4
    # resume: the second run loads rnnlm.model.best, evaluates it first, and trains on
    ppl2 = lm.train(args)
    assert ppl2 is not None and np.isfinite(ppl2)
