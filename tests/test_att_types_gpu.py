"""E2E with ``atype`` dot, add, coverage and coverage_location on the GPU against the golden vectors the reference's own modules
produced (tests/golden/att_types_tiny.npz, make_fixtures_att.py): losses, accuracy, every parameter gradient and the input gradient,
the attention dump, the n-best lists of ``recognize`` and of ``recognize_batch``; and a scheduled-sampling loop for coverage against
the float64 loop fed the tokens the device sampled.  Comparisons and tolerances are those tests/test_modules_gpu.py applies to
e2e_tiny.npz and tests/test_recog_batch_gpu.py to recog_tiny.npz."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs64 as R
import refs64_att as RA
from test_refs64_att_cpu import dump_key, fixture_params, loop_inputs, split_targets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CHARS = [str(i) for i in range(12)]
BIG, NS = 4096, 2048            # make_fixtures_att.py: gradients of more than BIG elements are kept as NS samples plus [l2 norm, sum]


def _opt(kind):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), 'atype': kind})


def _model(golden_dir, kind):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    p, fx = fixture_params(golden_dir, kind)
    sd = dict(p)
    sd.update({'dec.' + k: v for k, v in p.items() if k.startswith('att.')})
    m = E2E(_opt(kind))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(), fx


def rel(name, got, ref, tol=1e-3, atol=1e-7):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref).max()
    print('ERR %-60s %.3e of %.3e' % (name, err, np.abs(ref).max()))
    assert np.isfinite(err) and err <= tol * np.abs(ref).max() + atol, '%s: err %.3e scale %.3e' % (name, err, np.abs(ref).max())


@pytest.mark.parametrize('kind', RA.KINDS)
def test_e2e_forward_backward(golden_dir, kind):
    m, fx = _model(golden_dir, kind)
    feat = torch.from_numpy(fx['feats']).to(DEV).requires_grad_(True)
    lens, tl = torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens'])
    hpad, hl = m.enc(feat, lens)
    rel('hpad', hpad, fx[kind + '.hpad'])
    assert list(hl) == fx[kind + '.hlens'].tolist()
    lc, la, acc = m(feat, torch.from_numpy(fx['targets']), lens, tl, 0.0)
    rel('loss_ctc', lc.view(1), fx[kind + '.loss_ctc'].reshape(1))
    rel('loss_att', la.view(()), fx[kind + '.loss_att'].reshape(()))
    assert abs(float(acc) - float(fx[kind + '.acc'])) < 1e-6
    (0.5 * lc.view(()) + 0.5 * la).backward()
    rel('dfeat', feat.grad, fx[kind + '.dfeat'], tol=1.5e-3)
    seen = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if kind + '.g.' + k in fx:
            rel('g.' + k, p.grad, fx[kind + '.g.' + k], tol=1.5e-3)
        else:
            flat = p.grad.detach().float().cpu().numpy().reshape(-1)
            assert flat.size > BIG
            rel('gs.' + k, flat[np.linspace(0, flat.size - 1, NS).astype(np.int64)], fx[kind + '.gs.' + k], tol=1.5e-3)
            norm, total = fx[kind + '.gn.' + k]
            assert abs(np.sqrt((flat.astype(np.float64) ** 2).sum()) - norm) <= 1.5e-3 * norm, k
            assert abs(flat.astype(np.float64).sum() - total) <= 1.5e-3 * norm, k
        seen += 1
    assert seen == len([k for k in fx if k.startswith((kind + '.g.', kind + '.gs.'))])


@pytest.mark.parametrize('kind', RA.KINDS)
def test_attention_dump(golden_dir, kind):
    """calculate_all_attentions: the weights of every (greedy) step.  For the coverage types that is the fixture's ``att_steps``: upstream's
    own dump repeats their last step (the attention grows ONE list in place), which is not reproduced."""
    m, fx = _model(golden_dir, kind)
    att = m.calculate_all_attentions(torch.from_numpy(fx['feats']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']),
                                     torch.IntTensor(fx['tlens']))
    rel('att', att, fx[dump_key(kind)])
    if kind.startswith('coverage'):
        assert np.abs(att - att[:, -1:]).max() > 1e-3          # one row per step, not the last one repeated


def _args(beam, penalty, ctcw, maxr, minr, nbest, lm_weight=0.0):
    return argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=lm_weight)


def _same(a, b, tol):
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert x['yseq'] == y['yseq'], (x['yseq'], y['yseq'])
        assert abs(x['score'] - y['score']) <= tol * max(1.0, abs(y['score'])), (x['score'], y['score'])


@pytest.mark.parametrize('name', ['att_b3', 'joint_b4'])
@pytest.mark.parametrize('kind', RA.KINDS)
def test_recognize_and_recognize_batch(golden_dir, kind, name):
    """The reference's n-best lists from ``recognize`` utterance by utterance and from ``recognize_batch`` on the three as one padded batch;
    a row of the batch gets what the utterance alone gets (scores to 1e-5, as test_recognize_batch_utterances_are_independent)."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    m, fx = _model(golden_dir, kind)
    feats, lens = torch.from_numpy(fx['feats']), fx['lens'].tolist()
    cfg = [c for c in RECOG_CONFIGS if c[0] == name][0]
    args = _args(*cfg[1:])
    batch = m.recognize_batch(feats, lens, args, CHARS)
    assert len(batch) == 3 and m.training
    for u, T in enumerate(lens):
        one = m.recognize(feats[u:u + 1, :T], args, CHARS)
        check_nbest(one, fx, '%s.%s' % (kind, name), u)
        check_nbest(batch[u], fx, '%s.%s' % (kind, name), u)
        _same(batch[u], one, 1e-5)
    each = m.recognize_batch(feats, lens, args, CHARS, encode='each')
    for u in range(3):
        check_nbest(each[u], fx, '%s.%s' % (kind, name), u)


def test_recognize_with_an_rnnlm_runs_on_every_kind(golden_dir):
    """Shallow fusion does not touch the attention: with the RNNLM of recog_lm_tiny.npz the batched search still equals the single one."""
    from test_recog_lm_gpu import _tiny_lm
    lm = _tiny_lm(dict(np.load(os.path.join(golden_dir, 'recog_lm_tiny.npz'))))
    for kind in RA.KINDS:
        m, fx = _model(golden_dir, kind)
        feats, lens = torch.from_numpy(fx['feats']), fx['lens'].tolist()
        args = _args(4, 0.1, 0.3, 0.0, 0.0, 4, 0.5)
        batch = m.recognize_batch(feats, lens, args, CHARS, rnnlm=lm)
        for u, T in enumerate(lens):
            _same(batch[u], m.recognize(feats[u:u + 1, :T], args, CHARS, rnnlm=lm), 1e-5)


def test_coverage_scheduled_sampling_against_float64_on_the_sampled_tokens(golden_dir):
    """ss_rate = 1.0: every step i > 0 feeds the arg-max of the previous output.  The float64 loop is teacher-forced on the tokens the device
    fed (they are integers: no gradient through the choice), then states, weights and gradients are held to the decoder-loop bars."""
    from robust_e2e_gan_amd import ops
    kind = 'coverage'
    p, fx = fixture_params(golden_dir, kind)
    hlens, ys = fx[kind + '.hlens'].tolist(), split_targets(fx)
    hmask, pre, ids, _, L1, Pm32 = loop_inputs(kind, p, torch.from_numpy(fx[kind + '.hpad']), hlens, ys, 11, torch.float32)
    B = len(hlens)
    g = torch.Generator().manual_seed(9)
    gz = torch.randn(L1, B, Pm32['w_hh'].shape[1], generator=g)
    hm, pr = hmask.to(DEV).requires_grad_(True), pre.to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in Pm32.items()}
    Pm.update(out_w=p['dec.output.weight'].to(DEV), out_b=p['dec.output.bias'].to(DEV))
    steps = tuple(i > 0 for i in range(L1))
    zs, w = ops.DecoderLoopFn.apply(hm, pr, ids.reshape(-1).to(torch.int32).to(DEV), torch.tensor(hlens, dtype=torch.int32).to(DEV), L1, Pm, steps,
                                    False, kind)
    fed = zs.grad_fn.ids.view(L1, B).cpu().long()
    assert torch.equal(fed[0], ids[0]) and not torch.equal(fed, ids)                 # sampled tokens were fed
    (zs * gz.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    case = dict(kind=kind, hmask=hmask, pre=pre, Pm=Pm32, ids=fed, hlens=hlens, L1=L1, gz=gz)
    f64, f32 = RA.att_ref_run(case), RA.att_ref_run(case, torch.float32)
    # the float64 loop, sampling for itself, picks the same tokens: the comparison is not one of two different label sequences
    _, _, own = RA.att_loop_ref(kind, hmask.double(), pre.double(), ids, hlens, L1, {k: v.double() for k, v in Pm32.items()},
                                p['dec.output.weight'].double(), p['dec.output.bias'].double(), steps)
    assert torch.equal(own, fed)
    got = dict(zs=zs, w=w, d_enc=hm.grad, d_pre=pr.grad, **{k: Pm[k].grad for k in Pm32})
    for k in sorted(got):
        if k == 'gvec_b':
            assert got[k].abs().max().item() <= 1e-5 * float(L1 * B)
            continue
        bar, atol = (R.BAR_DEC_OUT, 0.0) if k in ('zs', 'w') else (R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
        R.margin_ok(k, f32[k], f64[k], bar, atol)
        err, scale = R.rel_err(got[k], f64[k]), f64[k].abs().max().item()
        print('ERR ss-coverage %-12s hip %.2e bar %.0e' % (k, err, bar))
        assert err * scale <= bar * scale + atol, (k, err)


@pytest.mark.parametrize('kind', RA.KINDS)
def test_joint_trainer_steps_with_the_kind(golden_dir, kind):
    """ShareE2E / JointTrainer need nothing beyond what E2E gives them: two joint steps on joint_tiny.npz's batch with the attention swapped
    for ``kind`` run, give finite losses, and move every attention parameter."""
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    fx = dict(np.load(os.path.join(golden_dir, 'joint_tiny.npz')))
    opt = _opt(kind)
    torch.manual_seed(7)
    enh, fb, asr, gan = EnhanceModel(opt), FbankModel(opt), ShareE2E(opt), GANModel(opt)
    own = asr.state_dict()
    own.update({k[4:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('asr.') and k[4:] in own and 'att.' not in k})
    asr.load_state_dict(own)
    for m, pre in ((enh, 'enh.'), (gan, 'gan.')):
        m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)})
    enh, fb, asr, gan = enh.to(DEV).train(), fb.to(DEV).train(), asr.to(DEV).train(), gan.to(DEV).train()
    before = {k: v.detach().clone() for k, v in asr.att.named_parameters()}
    tr = JointTrainer(opt, enh, fb, asr, gan)
    t = lambda k: torch.from_numpy(fx[k])
    data = (None, None, t('clean'), None, t('mix'), t('mix_log'), None, t('targets'), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']))
    for _ in range(2):
        out = JointTrainer.to_floats(tr.step(data, 0.0, t('cmvn')))
        assert all(np.isfinite(v) for v in out.values()), out
    torch.cuda.synchronize()
    for k, v in asr.att.named_parameters():
        if k != 'gvec.bias':                      # its gradient is analytically zero
            assert not torch.equal(v.detach(), before[k]), k
