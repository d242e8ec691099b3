"""The FS-RNN language model on the GPU (model/fsrnn.py over csrc/fsrnn.hip and the few-row kernels of csrc/rnnlm.hip) against the reference's
own model (tests/golden/fsrnn_tiny.npz, make_fixtures_fsrnn.py: within 1e-3), against the float64 restatement of tests/refs64_fsrnn.py with
the training masks rebuilt from the counter-based stream, and the fused arm against the composed one (1e-4 of the max for the loss and the
state, 2e-4 for gradients).  GPU only."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs64_fsrnn as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

BAR = 1e-3          # README: losses and gradients within 1e-3 of the reference's fp32 CPU path
V, E, H = 12, 6, 10
LAYERS = (2, 3)


@pytest.fixture(scope='module')
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'fsrnn_tiny.npz')))


def _model(fx, L, keeps=(0.9, 0.5), dropout=0.0, dims=(V, E, H), train=True):
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    m = ClassifierWithState(FSRNNLM(dims[0], dims[1], L, dims[2], dims[2], keeps[0], keeps[1], dropout_rate=dropout))
    if fx is not None:
        pre = 'L%d.lm.' % L
        res = m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    m.compute_accuracy = False
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _close(name, got, want, bar=BAR):
    got, want = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(want).detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    err, scale = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-30)
    print('PARITY %-44s %.2e of max (bar %.0e)' % (name, err / scale, bar))
    assert err <= bar * scale, '%s: %.3e of the max from the reference (bar %.1e)' % (name, err / scale, bar)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _check_window(fx, L, m, losses, state, tag):
    pre = 'L%d.win.' % L
    if losses is not None:
        _close(tag + ' losses', losses, fx[pre + 'losses'])
    for k in R.STATE_KEYS:
        _close('%s state %s' % (tag, k), state[k], fx[pre + 'state.' + k])
    g = _grads(m)
    assert len(g) == len(R.param_names(L))
    for k, v in g.items():
        want = fx[pre + 'grad.' + k]
        if np.abs(want).max() == 0.0:
            assert float(v.abs().max()) == 0.0, k
        else:
            _close('%s grad %s' % (tag, k), v, want)


@pytest.mark.parametrize('L', LAYERS)
def test_window_through_forward_seq(fx, L):
    """Evaluation mode with gradients enabled: the blend, deterministic."""
    _ops()
    m = _model(fx, L, train=False)
    xs, ts = fx['L%d.win.xs' % L], fx['L%d.win.ts' % L]
    state, logits = m.predictor.forward_seq(None, xs)
    assert tuple(logits.shape) == (4, 3, V)
    ref = R.fs_model_ref({k: torch.from_numpy(fx['L%d.lm.predictor.%s' % (L, k)]) for k in R.param_names(L)}, xs, ts, L, 0.9, 0.5)
    _close('forward_seq logits', logits, ref['logits'])
    state, loss = m.forward_seq(None, xs, ts)
    assert loss.dim() == 0 and m.loss is loss and tuple(m.y.shape) == (4, 3, V)
    _close('forward_seq loss', loss, fx['L%d.win.losses' % L].sum())
    loss.backward()
    _check_window(fx, L, m, None, state, 'forward_seq')


@pytest.mark.parametrize('L', LAYERS)
def test_window_through_the_per_step_loop(fx, L):
    """The reference's per-step loop on the fixture's window.  The window is the evaluation-mode blend, and ``forward`` in evaluation mode
    runs without gradients, so the differentiable loop goes over windows of T = 1 (what ``forward`` in training mode is), chained through
    the state's gradient; ``forward`` itself (the few-row kernels) is then checked on the losses and the final state."""
    _ops()
    m = _model(fx, L, train=False)
    pre = 'L%d.win.' % L
    state, losses, loss = None, [], 0
    for t in range(4):
        state, l = m.forward_seq(state, fx[pre + 'xs'][t:t + 1], fx[pre + 'ts'][t:t + 1])
        losses.append(float(l.detach()))
        loss = loss + l
    m.zero_grad()
    loss.backward()
    _check_window(fx, L, m, losses, state, 'per-step')
    # ``forward`` in evaluation mode (no gradients, the few-row kernels) gives the same per-step losses
    state, ev = None, []
    for t in range(4):
        state, l = m(state, torch.from_numpy(fx[pre + 'xs'][t]).long(), torch.from_numpy(fx[pre + 'ts'][t]).long())
        assert not l.requires_grad
        ev.append(float(l))
    _close('per-step eval losses', ev, fx[pre + 'losses'])
    for k in R.STATE_KEYS:
        _close('per-step eval state ' + k, state[k], fx[pre + 'state.' + k])


@pytest.mark.parametrize('L', LAYERS)
def test_window_through_two_chained_windows(fx, L):
    _ops()
    m = _model(fx, L, train=False)
    xs, ts = fx['L%d.win.xs' % L], fx['L%d.win.ts' % L]
    state, l0 = m.forward_seq(None, xs[:2], ts[:2])
    assert all(v.requires_grad for v in state.values())
    state, l1 = m.forward_seq(state, xs[2:], ts[2:])
    _close('chained loss', l0 + l1, fx['L%d.win.losses' % L].sum())
    (l0 + l1).backward()
    _check_window(fx, L, m, None, state, 'chained')


@pytest.mark.parametrize('L,dims,T,B,train', [(2, (V, E, H), 4, 3, False), (3, (20, 9, 33), 3, 65, True), (4, (20, 9, 33), 2, 5, False)],
                         ids=['fixture-L2-eval', 'L3-H33-T3-B65-train', 'L4-H33-T2-B5-eval'])
def test_fused_and_composed_arms_agree(fx, L, dims, T, B, train, monkeypatch):
    """The window over csrc/fsrnn.hip against the same window over re2e_gemm + re2e_lstm_cell_fwd / _bwd + element-wise ops, from a non-zero
    state and with weights on the final state; in training mode both arms draw the same masks (the stream is reset between them)."""
    ops, _ = _ops()
    from robust_e2e_gan_amd.model import lm
    g = torch.Generator().manual_seed(17 + L)
    m = _model(fx if dims == (V, E, H) else None, L, keeps=(0.75, 0.5), dropout=0.5 if train else 0.0, dims=dims, train=train)
    if dims != (V, E, H):
        for p in m.parameters():
            p.data.copy_(torch.rand(p.shape, generator=g) - 0.5)
    xs, ts = torch.randint(0, dims[0], (T, B), generator=g).numpy(), torch.randint(0, dims[0], (T, B), generator=g).numpy()
    st0 = {k: (torch.tanh(torch.randn(B, dims[2], generator=g)) * 0.8).to(DEV) for k in R.STATE_KEYS}
    wout = {k: torch.randn(B, dims[2], generator=g).to(DEV) * 0.3 for k in R.STATE_KEYS}
    runs = []
    for composed in (False, True):
        monkeypatch.setattr(lm, 'COMPOSED_PATH', composed)
        ops.dropout_seed(99, 3)
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
        if k.endswith('weight_ih') and k.startswith('predictor.fast_cells.') and int(k.split('.')[2]) >= 2:
            assert float(gf[k].abs().max()) == 0.0 and float(gc[k].abs().max()) == 0.0, k
        else:
            _close('fused vs composed grad ' + k, gf[k], gc[k], 2e-4)


@pytest.mark.parametrize('L', LAYERS)
def test_training_window_against_float64_with_philox_masks(fx, L):
    """p = 0.5, keeps 0.75 / 0.5: the masks are drawn in the reference's order of use -- d0, then per cell F0, S, F1, F2 .. its zoneout mask of
    c, of h and (F0, S) the dropout behind it, then d3 -- each over its whole (T, B, .) tensor.  The float64 model with those masks is the
    yardstick; torch's fp32 CPU run of it must stay within a quarter of the bar."""
    ops, _ = _ops()
    from oracle.philox import dropout_mask
    xs, ts = fx['L%d.win.xs' % L], fx['L%d.win.ts' % L]
    T, B = xs.shape
    seed, call = 0xC0FFEE1234, 7
    ops.dropout_seed(seed, call)
    m = _model(fx, L, keeps=(0.75, 0.5), dropout=0.5)
    state, loss = m.forward_seq(None, xs, ts)
    loss.backward()
    n_masks = 1 + 2 * (L + 1) + 2 + 1
    assert ops.dropout_state() == (seed, call + n_masks)
    idx = [call]

    def draw(w, p):
        mk = torch.from_numpy(dropout_mask(T * B * w, p, seed, idx[0])).view(T, B, w)
        idx[0] += 1
        return mk
    masks = dict(d0=draw(E, 0.5), mh=torch.empty(L + 1, T, B, H), mc=torch.empty(L + 1, T, B, H))
    for c in [0, L] + list(range(1, L)):
        masks['mc'][c] = (draw(H, 0.5) != 0).float()
        masks['mh'][c] = (draw(H, 0.25) != 0).float()
        if c == 0:
            masks['d1'] = draw(H, 0.5)
        if c == L:
            masks['d2'] = draw(H, 0.5)
    masks['d3'] = draw(H, 0.5)
    assert idx[0] == call + n_masks
    assert 0.6 < float(masks['mh'].mean()) < 0.9 and 0.3 < float(masks['mc'].mean()) < 0.7
    params = {k: torch.from_numpy(fx['L%d.lm.predictor.%s' % (L, k)]) for k in R.param_names(L)}
    r64 = R.fs_model_ref(params, xs, ts, L, 0.75, 0.5, masks=masks)
    r32 = R.fs_model_ref(params, xs, ts, L, 0.75, 0.5, masks=masks, dtype=torch.float32)
    plain = R.fs_model_ref(params, xs, ts, L, 0.75, 0.5)
    assert abs(float(r64['loss']) - float(plain['loss'])) > 100 * BAR          # the masks matter at this size
    R.margin_ok('loss', r32['loss'], r64['loss'], BAR)
    _close('training loss', loss, r64['loss'])
    for k in R.STATE_KEYS:
        R.margin_ok(k, r32[k], r64[k], BAR)
        _close('training state ' + k, state[k], r64[k])
    for k, v in _grads(m).items():
        name = k[len('predictor.'):]
        if float(r64['grad.' + name].abs().max()) == 0.0:
            assert float(v.abs().max()) == 0.0, name
            continue
        R.margin_ok(name, r32['grad.' + name], r64['grad.' + name], BAR)
        _close('training grad ' + name, v, r64['grad.' + name])
    # evaluation mode draws nothing
    m.eval()
    with torch.no_grad():
        m.predictor.forward_seq(None, xs)
        m.predictor(None, xs[0])
    assert ops.dropout_state() == (seed, call + n_masks)


@pytest.mark.parametrize('L', LAYERS)
def test_three_training_iterations_follow_the_fixture(fx, L):
    """The trainer's loop body with dropout 0 and both keeps 1.0 (the reference's training mode is deterministic then): loss, gradient norm
    and all parameters after each iteration; one iteration is clipped and one is not.  Then the validation perplexity of the evaluation loop
    with keeps 0.9 / 0.5 on the fixture's own parameters."""
    ops, _ = _ops()
    from robust_e2e_gan_amd.data.lm_data_loader import ParallelSequentialIterator
    from robust_e2e_gan_amd.model.lm import evaluate
    from robust_e2e_gan_amd.optim import FlatOptimizer
    pre = 'L%d.train.' % L
    m = _model(fx, L, keeps=(1.0, 1.0))
    call0 = ops.dropout_state()
    opt = FlatOptimizer(m.parameters(), kind='sgd', lr=1.0)
    it = ParallelSequentialIterator(fx[pre + 'corpus'], 4)
    clip, state, coefs = float(fx[pre + 'gradclip']), None, []
    for k in range(3):
        xs, ts = it.next_window(3)
        state, loss = m.forward_seq(state, xs, ts)
        opt.zero_grad()
        loss.backward()
        state = {n: v.detach() for n, v in state.items()}
        norm = opt.clip_grad_norm(clip)
        opt.step()
        coefs.append(float(opt.stats[1]))
        _close('it%d loss' % k, loss, fx[pre + 'it%d.loss' % k])
        _close('it%d norm' % k, norm, fx[pre + 'it%d.norm' % k])
        for n, p in m.state_dict().items():
            _close('it%d %s' % (k, n), p, fx[pre + 'it%d.%s' % (k, n)])
    assert ops.dropout_state() == call0          # p = 0 and keep = 1 draw nothing
    assert min(coefs) < 1.0 and max(coefs) == 1.0, coefs
    moved = max(float(np.abs(fx[pre + 'it2.' + n] - fx['L%d.lm.%s' % (L, n)]).max()) for n in m.state_dict())
    assert moved > 100 * BAR                     # a trainer that did not update would not pass
    m = _model(fx, L)
    ppl = evaluate(m, ParallelSequentialIterator(fx[pre + 'valid'], 4, repeat=False))
    print('PARITY validation perplexity %.6f vs %.6f' % (ppl, float(fx[pre + 'valid_ppl'])))
    assert abs(ppl - float(fx[pre + 'valid_ppl'])) <= BAR * float(fx[pre + 'valid_ppl'])
    assert m.predictor.training                  # evaluate leaves the predictor in training mode, as the reference does


@pytest.mark.parametrize('path', ['fused', 'composed'])
@pytest.mark.parametrize('L', LAYERS)
def test_predict_chain_matches_reference(fx, L, path, monkeypatch):
    """8 positions x 3 rows of ClassifierWithState.predict with the state rows permuted (one repeated) between positions, over the few-row
    kernels and over the composed path; every output buffer of the few-row step starts as NaN."""
    _ops()
    from robust_e2e_gan_amd.model import lm as lm_mod
    m = _model(fx, L, train=False)
    monkeypatch.setattr(lm_mod, '_empty', lambda *shape, **kw: torch.full(shape, float('nan'), **kw))
    monkeypatch.setattr(lm_mod, 'COMPOSED_PATH', path == 'composed')
    pre = 'L%d.chain.' % L
    ids, parents = fx[pre + 'ids'], fx[pre + 'parents']
    state = None
    for i in range(ids.shape[0]):
        if state is not None:
            par = torch.from_numpy(parents[i]).to(DEV)
            state = {k: v.index_select(0, par) for k, v in state.items()}
        state, lp = m.predict(state, torch.from_numpy(ids[i]))
        _close('%s logp[%d]' % (path, i), lp, fx[pre + 'logp'][i])
    for k in R.STATE_KEYS:
        _close('%s final %s' % (path, k), state[k], fx[pre + k])


def test_more_rows_than_the_few_row_kernels_take(fx):
    """65 rows in evaluation mode take the window path with T = 1: the first 64 rows equal what the few-row kernels give for them."""
    _ops()
    m = _model(fx, 3, train=False)
    g = torch.Generator().manual_seed(65)
    ids = torch.randint(0, V, (65,), generator=g)
    st = {k: (torch.tanh(torch.randn(65, H, generator=g)) * 0.8).to(DEV) for k in R.STATE_KEYS}
    big_state, big = m.predict(st, ids)
    few_state, few = m.predict({k: v[:64].contiguous() for k, v in st.items()}, ids[:64])
    assert tuple(big.shape) == (65, V) and not big.requires_grad
    _close('65 rows vs 64 rows logp', big[:64], few, 1e-4)
    for k in R.STATE_KEYS:
        _close('65 rows vs 64 rows ' + k, big_state[k][:64], few_state[k], 1e-4)


@pytest.mark.parametrize('how', ['recognize', 'recognize_batch'])
def test_recognize_with_the_fsrnnlm_matches_reference_nbest(golden_dir, fx, how):
    """E2E.recognize / recognize_batch (..., rnnlm=ClassifierWithState(FSRNNLM)) reproduce the reference's n-best lists for the search
    configurations of recog_tiny.npz plus ctc_weight = 1.0, at lm_weight 0.2 and 1.0, three utterances each.  (The generator asserts that
    every list differs from its LM-free counterpart.)"""
    from test_modules_gpu import _fx, _load, _opt
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from test_recog_lm_gpu import LM_CONFIGS_EXTRA, LM_WEIGHTS, _args
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base = _fx(golden_dir, 'recog_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    m = _model(fx, 2, train=False)
    feats = torch.from_numpy(base['feats'])
    lens = base['lens'].tolist()
    chars = [str(i) for i in range(12)]
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS + LM_CONFIGS_EXTRA:
        for w in LM_WEIGHTS:
            args = _args(beam, penalty, ctcw, maxr, minr, nbest, w)
            if how == 'recognize':
                lists = [asr.recognize(feats[u:u + 1, :T], args, chars, rnnlm=m) for u, T in enumerate(lens)]
            else:
                lists = asr.recognize_batch(feats, lens, args, chars, rnnlm=m)
            for u, got in enumerate(lists):
                check_nbest(got, fx, '%s.w%03d' % (name, int(round(w * 100))), u)


def test_lm_train_end_to_end(fx, tmp_path):
    """lm_train.main([... '--lm-type', 'fsrnnlm', ...]) on the tiny corpus for one epoch: rnnlm.model.0, rnnlm.state.0 and the rnnlm.model.best
    link are written, the state dict loads strictly into a fresh ClassifierWithState(FSRNNLM), and a second call resumes."""
    _ops()
    from robust_e2e_gan_amd import lm_train
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    L = 3
    chars = [str(i) for i in range(1, 11)]          # + <blank> and <eos>: 12 labels
    (tmp_path / 'dict.txt').write_text(''.join('%s %d\n' % (c, i + 1) for i, c in enumerate(chars)))
    text = lambda ids: ' '.join(chars[int(i) % 10] for i in ids) + '\n'
    (tmp_path / 'train.txt').write_text(text(fx['L3.train.corpus']))
    (tmp_path / 'valid.txt').write_text(text(fx['L3.train.valid']))
    argv = ['--ngpu', '1', '--outdir', str(tmp_path), '--dict', str(tmp_path / 'dict.txt'), '--train-label', str(tmp_path / 'train.txt'),
            '--valid-label', str(tmp_path / 'valid.txt'), '--lm-type', 'fsrnnlm', '--batchsize', '4', '--bproplen', '3', '--epoch', '1',
            '--input-unit', str(E), '--fast_layers', str(L), '--fast_cell_size', str(H), '--slow_cell_size', str(H), '--zoneout_keep_h', '0.75',
            '--zoneout_keep_c', '0.5', '--dropout-rate', '0.5']
    ppl = lm_train.main(argv)
    assert ppl is not None and np.isfinite(ppl) and 1.0 < ppl < 1e4
    assert (tmp_path / 'rnnlm.model.0').is_file() and (tmp_path / 'rnnlm.state.0').is_file()
    best = tmp_path / 'rnnlm.model.best'
    assert best.is_symlink() and os.readlink(str(best)) == 'rnnlm.model.0'
    sd = torch.load(str(best), map_location='cpu')
    assert set(sd) == {'predictor.' + k for k in R.param_names(L)}
    fresh = ClassifierWithState(FSRNNLM(12, E, L, H, H, 0.75, 0.5))
    res = fresh.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = fresh.to(DEV).eval()
    state, lp = fresh.predict(None, np.array([1, 5, 9], np.int32))
    assert abs(float(torch.logsumexp(lp, 1)[0])) < 1e-4
    ppl2 = lm_train.main(argv)                      # resume: loads rnnlm.model.best, evaluates it first, and trains on
    assert ppl2 is not None and np.isfinite(ppl2)


def test_what_the_reference_cannot_run_is_refused():
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.fsrnn import FSRNNLM
    with pytest.raises(Re2eError, match='fsrnn.py:118'):
        FSRNNLM(12, 6, 2, 10, 8, 0.9, 0.5)
    with pytest.raises(Re2eError, match='fsrnn.py:118'):
        FSRNNLM(12, 6, 1, 10, 10, 0.9, 0.5)


def test_inputless_cells_get_a_zero_gradient_tensor(fx):
    """fast_cells.2.weight_ih.grad is an all-zero tensor, not None, after a backward without an optimizer's pre-allocated gradients."""
    _ops()
    m = _model(fx, 3)
    assert m.predictor.fast_cells[2].weight_ih.grad is None
    state, loss = m.forward_seq(None, fx['L3.win.xs'], fx['L3.win.ts'])
    loss.backward()
    g = m.predictor.fast_cells[2].weight_ih.grad
    assert g is not None and tuple(g.shape) == (4 * H, H) and float(g.abs().max()) == 0.0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert float(m.predictor.fast_cells[2].weight_hh.grad.abs().max()) > 0.0
