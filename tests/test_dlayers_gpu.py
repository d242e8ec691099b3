"""E2E with ``dlayers`` 2 and 3 on the GPU against the golden vectors the reference's own modules produced (tests/golden/dlayers_tiny.npz,
make_fixtures_dlayers.py): losses, accuracy, every parameter gradient and the input gradient, the attention dump, the n-best lists of
``recognize`` and of ``recognize_batch`` without and with an RNNLM; a scheduled-sampling loop of the 2-layer coverage model against the
float64 loop fed the tokens the device sampled; the persistent layer-0 loop under a 2-layer location model; one JointTrainer step.
Comparisons and tolerances are those of tests/test_att_types_gpu.py."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs64 as R
import refs64_dlayers as RD
from test_att_types_gpu import BIG, CHARS, DEV, NS, _args, _same, rel
from test_refs64_att_cpu import split_targets
from test_refs64_dlayers_cpu import MODELS, fixture_model, stacked_inputs

pytestmark = pytest.mark.gpu
TAGS = [t for t, _, _ in MODELS]
KIND = {t: (k, n) for t, k, n in MODELS}


def _opt(kind, dlayers):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), 'atype': kind, 'dlayers': dlayers})


def _model(golden_dir, tag):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    p, sd, fx, att = fixture_model(golden_dir, tag)
    m = E2E(_opt(*KIND[tag]))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).train(), fx, att, p


@pytest.mark.parametrize('tag', TAGS)
def test_e2e_forward_backward(golden_dir, tag):
    m, fx, att, _ = _model(golden_dir, tag)
    feat = torch.from_numpy(att['feats']).to(DEV).requires_grad_(True)
    lens, tl = torch.IntTensor(att['lens']), torch.IntTensor(att['tlens'])
    lc, la, acc = m(feat, torch.from_numpy(att['targets']), lens, tl, 0.0)
    rel('loss_ctc', lc.view(1), fx[tag + '.loss_ctc'].reshape(1))
    rel('loss_att', la.view(()), fx[tag + '.loss_att'].reshape(()))
    assert abs(float(acc) - float(fx[tag + '.acc'])) < 1e-6
    (0.5 * lc.view(()) + 0.5 * la).backward()
    rel('dfeat', feat.grad, fx[tag + '.dfeat'], tol=1.5e-3)
    seen = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if tag + '.g.' + k in fx:
            rel('g.' + k, p.grad, fx[tag + '.g.' + k], tol=1.5e-3)
        else:
            flat = p.grad.detach().float().cpu().numpy().reshape(-1)
            assert flat.size > BIG
            rel('gs.' + k, flat[np.linspace(0, flat.size - 1, NS).astype(np.int64)], fx[tag + '.gs.' + k], tol=1.5e-3)
            norm, total = fx[tag + '.gn.' + k]
            assert abs(np.sqrt((flat.astype(np.float64) ** 2).sum()) - norm) <= 1.5e-3 * norm, k
            assert abs(flat.astype(np.float64).sum() - total) <= 1.5e-3 * norm, k
        seen += 1
    assert seen == len([k for k in fx if k.startswith((tag + '.g.', tag + '.gs.'))])
    assert any(k.startswith('dec.decoder.%d.' % (KIND[tag][1] - 1)) for k, _ in m.named_parameters())


@pytest.mark.parametrize('tag', TAGS)
def test_attention_dump(golden_dir, tag):
    """calculate_all_attentions: the weights of every (greedy) step; the fed token is the arg-max on the top layer's output."""
    m, fx, att, _ = _model(golden_dir, tag)
    got = m.calculate_all_attentions(torch.from_numpy(att['feats']), torch.from_numpy(att['targets']), torch.IntTensor(att['lens']),
                                     torch.IntTensor(att['tlens']))
    rel('att', got, fx[tag + '.att'])


@pytest.mark.parametrize('name', ['att_b3', 'joint_b4', 'lm_joint_b4'])
@pytest.mark.parametrize('tag', TAGS)
def test_recognize_and_recognize_batch(golden_dir, tag, name):
    """The reference's n-best lists from ``recognize`` utterance by utterance and from ``recognize_batch`` on the three as one padded batch;
    a row of the batch gets what the utterance alone gets (scores to 1e-5).  ``lm_joint_b4``: with the RNNLM of recog_lm_tiny.npz."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    m, fx, att, _ = _model(golden_dir, tag)
    feats, lens = torch.from_numpy(att['feats']), att['lens'].tolist()
    cfg = [c for c in RECOG_CONFIGS if c[0] == name.replace('lm_', '')][0]
    lm = None
    args = _args(*cfg[1:])
    if name.startswith('lm_'):
        from test_recog_lm_gpu import _tiny_lm
        lm = _tiny_lm(dict(np.load(os.path.join(golden_dir, 'recog_lm_tiny.npz'))))
        args = _args(*cfg[1:], lm_weight=float(fx['lm_weight']))
    batch = m.recognize_batch(feats, lens, args, CHARS, rnnlm=lm)
    assert len(batch) == 3 and m.training
    for u, T in enumerate(lens):
        one = m.recognize(feats[u:u + 1, :T], args, CHARS, rnnlm=lm)
        check_nbest(one, fx, '%s.%s' % (tag, name), u)
        check_nbest(batch[u], fx, '%s.%s' % (tag, name), u)
        _same(batch[u], one, 1e-5)


def test_coverage_scheduled_sampling_against_float64_on_the_sampled_tokens(golden_dir):
    """ss_rate = 1.0 on the 2-layer coverage model: every step i > 0 feeds the arg-max of the output layer on the TOP layer's previous state.
    The float64 stacked loop is teacher-forced on the tokens the device fed, then states, weights and gradients are held to the decoder-loop bars."""
    from robust_e2e_gan_amd import ops
    tag, kind = 'cov2', 'coverage'
    p, _, fx, att = fixture_model(golden_dir, tag)
    hlens, ys = att['add.hlens'].tolist(), split_targets(att)
    hmask, pre, ids, _, L1, Pm32, lay32 = stacked_inputs(kind, p, torch.from_numpy(att['add.hpad']), hlens, ys, 11, torch.float32)
    B, D = len(hlens), Pm32['w_hh'].shape[1]
    g = torch.Generator().manual_seed(9)
    gz = torch.randn(L1, B, D, generator=g)
    hm, pr = hmask.to(DEV).requires_grad_(True), pre.to(DEV).requires_grad_(True)
    Pm = {k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in Pm32.items()}
    out_w, out_b = p['dec.output.weight'], p['dec.output.bias']
    Pm.update(out_w=out_w.to(DEV), out_b=out_b.to(DEV))
    lays = [{k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in lay.items()} for lay in lay32]
    steps = tuple(i > 0 for i in range(L1))
    top, w = ops.DecoderLoopFn.apply(hm, pr, ids.reshape(-1).to(torch.int32).to(DEV), torch.tensor(hlens, dtype=torch.int32).to(DEV), L1, Pm, steps,
                                     False, kind, lays)
    fed = top.grad_fn.ids.view(L1, B).cpu().long()
    assert torch.equal(fed[0], ids[0]) and not torch.equal(fed, ids)                 # sampled tokens were fed
    (top * gz.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    case = dict(kind=kind, hmask=hmask, pre=pre, Pm=Pm32, layers=lay32, ids=fed, hlens=hlens, L1=L1, gz=gz)
    f64, f32 = RD.loop_ref_run(case), RD.loop_ref_run(case, torch.float32)
    # the float64 loop's own top states choose the same tokens: the comparison is not one of two different label sequences
    own, _ = RD.sampled_tokens(f64['z_top'], ids, out_w.double(), out_b.double(), steps)
    assert torch.equal(own, fed)
    got = dict(z_top=top, w=w, d_enc=hm.grad, d_pre=pr.grad, **{k: Pm[k].grad for k in Pm32},
               **{'l%d.%s' % (l + 1, k): lay[k].grad for l, lay in enumerate(lays) for k in RD.UPPER_KEYS})
    assert set(got) == set(f64)
    for k in sorted(got):
        if k == 'gvec_b':
            assert got[k].abs().max().item() <= 1e-5 * float(L1 * B)
            continue
        bar, atol = (R.BAR_DEC_OUT, 0.0) if k in ('z_top', 'w') else (R.BAR_DEC_GRAD, R.ATOL_DEC_GRAD)
        R.margin_ok(k, f32[k], f64[k], bar, atol)
        err, scale = R.rel_err(got[k], f64[k]), f64[k].abs().max().item()
        print('ERR ss-cov2 %-12s hip %.2e bar %.0e' % (k, err, bar))
        assert err * scale <= bar * scale + atol, (k, err)


def test_location_keeps_the_persistent_loop_under_two_layers(golden_dir, monkeypatch):
    """With dlayers = 2 the teacher-forced pass still runs layer 0 as ops.DecoderLoopFn alone, called as a single-layer model calls it and in
    its persistent form where that model has it, and the upper layer as ops.DecoderUpperFn on its states.  (The fixtures' dunits = 14 and
    adim = 18 are outside the persistent form for any dlayers: the model here has dunits = 16, adim = 20.)"""
    from robust_e2e_gan_amd import ops
    from robust_e2e_gan_amd.model.e2e_model import E2E
    import __graft_entry__ as g
    att = dict(np.load(os.path.join(golden_dir, 'att_types_tiny.npz')))
    seen = []
    loop, upper = ops.decoder_loop, ops.decoder_upper

    def spy_loop(*a):
        out = loop(*a)
        seen.append(('loop', out[0].grad_fn.persist, len(a)))
        return out

    def spy_upper(z0, lays):
        seen.append(('upper', len(lays)))
        return upper(z0, lays)
    monkeypatch.setattr(ops, 'decoder_loop', spy_loop)
    monkeypatch.setattr(ops, 'decoder_upper', spy_upper)
    feat = torch.from_numpy(att['feats']).to(DEV)
    for nl in (1, 2):
        torch.manual_seed(3)
        m = E2E(argparse.Namespace(**{**vars(g._tiny_opt()), 'dunits': 16, 'adim': 20, 'dlayers': nl})).to(DEV).train()
        _, la, _ = m(feat, torch.from_numpy(att['targets']), torch.IntTensor(att['lens']), torch.IntTensor(att['tlens']), 0.0)
        assert np.isfinite(float(la.detach()))
    assert ops.DECODER_PERSIST is True
    assert seen == [('loop', True, 9), ('loop', True, 9), ('upper', 1)], seen


def test_joint_trainer_steps_with_two_layers(golden_dir):
    """One JointTrainer.step with dlayers = 2 on joint_tiny.npz's batch: a finite loss and a gradient on every parameter of the new layer."""
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    fx = dict(np.load(os.path.join(golden_dir, 'joint_tiny.npz')))
    opt = _opt('location', 2)
    torch.manual_seed(7)
    enh, fb, asr, gan = EnhanceModel(opt), FbankModel(opt), ShareE2E(opt), GANModel(opt)
    own = asr.state_dict()
    own.update({k[4:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('asr.') and k[4:] in own})
    asr.load_state_dict(own)
    for m, pre in ((enh, 'enh.'), (gan, 'gan.')):
        m.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)})
    enh, fb, asr, gan = enh.to(DEV).train(), fb.to(DEV).train(), asr.to(DEV).train(), gan.to(DEV).train()
    new = {k: v for k, v in asr.named_parameters() if k.startswith('dec.decoder.1.')}
    assert len(new) == 4
    before = {k: v.detach().clone() for k, v in new.items()}
    tr = JointTrainer(opt, enh, fb, asr, gan)
    t = lambda k: torch.from_numpy(fx[k])
    data = (None, None, t('clean'), None, t('mix'), t('mix_log'), None, t('targets'), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']))
    out = JointTrainer.to_floats(tr.step(data, 0.0, t('cmvn')))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in out.values()), out
    for k, v in new.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max().item() > 0, k
        assert not torch.equal(v.detach(), before[k]), k
