#!/usr/bin/env python3
"""Golden vectors for the multi-layer attention decoder (``--dlayers`` > 1, model/e2e_decoder.py:37-39, 121-152, 229-258, 399-422): the
reference's own E2E on ``make_fixtures.tiny_opt()`` with dlayers 2 and 3 for ``atype='location'`` and dlayers 2 for ``atype='coverage'``:
forward / backward, attention dump and beam search (without and with the RNNLM of recog_lm_tiny.npz).  Runs only where the reference is
importable (make_fixtures.REF, with its shims); no test imports it.  Writes dlayers_tiny.npz.  Keys of a model are prefixed ``<tag>.`` with
tag = loc2, loc3, cov2:

  p.dec.decoder.{1,2}.*     the new layers' parameters (drawn under the seed).  Every OTHER parameter is e2e_tiny.npz's ``p.*`` and, for
                            coverage, att_types_tiny.npz's ``coverage.p.att.*`` (loaded before the forward), so that this file stays data of
                            a committable size
  loss_ctc, loss_att, acc   E2E.forward on lens [37, 29, 20], labels [5, 4, 3]
  g.*, gs.*, gn.*, dfeat    gradients of 0.5 ctc + 0.5 att, packed as make_fixtures_att.py packs them (BIG / NS)
  att                       the weights of every greedy step (B, Lmax + 1, T'): calculate_all_attentions, for coverage the attention's own list
                            (make_fixtures_att.py run_type says why)
  <config>.u<k>.yseq/score  n-best lists of recognize: att_b3 and joint_b4 of make_fixtures_recog.py, and ``lm_joint_b4`` = joint_b4 with the
                            RNNLM of recog_lm_tiny.npz at lm_weight LM_WEIGHT

``feats``, ``targets``, ``lens``, ``tlens`` are those of att_types_tiny.npz (asserted).  The seed of a model (``<tag>.seed``) is the first from
202 at which adjacent n-best scores of every configuration and utterance are >= 1e-3 apart."""
import argparse
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402
from make_fixtures_att import LENS, TLENS, MIN_GAP, RECOG, pack_grads   # noqa: E402

MODELS = (('loc2', 'location', 2), ('loc3', 'location', 3), ('cov2', 'coverage', 2))
LM_WEIGHT = 0.5


def nbest_arrays(hyps):
    L = max(len(h['yseq']) for h in hyps)
    seqs = np.full((len(hyps), L), -1, np.int64)
    for i, h in enumerate(hyps):
        seqs[i, :len(h['yseq'])] = h['yseq']
    return seqs, np.array([float(h['score']) for h in hyps], np.float64)


def tiny_lm():
    from model.lm import ClassifierWithState, RNNLM
    fx = dict(np.load(os.path.join(HERE, 'recog_lm_tiny.npz')))
    lm = ClassifierWithState(RNNLM(mf.tiny_opt().odim, 6, 10))
    lm.load_state_dict({k[len('lm.'):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('lm.')})
    return lm.eval()


def run_model(atype, dlayers, seed, feats, targets, lm):
    from model.e2e_model import E2E
    opt = mf.tiny_opt()
    opt.atype, opt.dlayers = atype, dlayers
    torch.manual_seed(seed)
    random.seed(0)
    asr = E2E(opt)
    base = dict(np.load(os.path.join(HERE, 'e2e_tiny.npz')))
    own = asr.state_dict()
    new = [k for k in own if k.startswith('dec.decoder.') and not k.startswith('dec.decoder.0.')]
    assert len(new) == 4 * (dlayers - 1), new
    shared = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.')}
    if atype != 'location':
        att = dict(np.load(os.path.join(HERE, 'att_types_tiny.npz')))
        shared = {k: v for k, v in shared.items() if not k.startswith(('att.', 'dec.att.'))}
        for k, v in att.items():
            if k.startswith(atype + '.p.att.'):
                shared[k[len(atype) + 3:]] = shared['dec.' + k[len(atype) + 3:]] = torch.from_numpy(v)
    assert set(shared) == set(own) - set(new), set(shared) ^ (set(own) - set(new))
    own.update(shared)
    asr.load_state_dict(own)
    asr.train()
    input_sizes, target_sizes = torch.IntTensor(LENS), torch.IntTensor(TLENS)
    feat = feats.clone().requires_grad_(True)
    loss_ctc, loss_att, acc = asr(feat, targets, input_sizes, target_sizes, 0.0)
    asr.zero_grad()
    (0.5 * loss_ctc + 0.5 * loss_att).backward()
    fx = dict(loss_ctc=loss_ctc.detach().numpy(), loss_att=loss_att.detach().numpy(), acc=np.float64(acc), dfeat=feat.grad.numpy().copy())
    fx.update({k: v for k, v in mf.sd_np('p.', asr).items() if k[2:] in new})
    fx.update(pack_grads(asr))
    asr.eval()
    seen = []
    hook = asr.att.register_forward_hook(lambda mod, args, out: seen.append(out[1]))
    att_dump = np.asarray(asr.calculate_all_attentions(feats, targets, input_sizes, target_sizes)).copy()
    hook.remove()
    if isinstance(seen[-1], list):
        att_dump = torch.stack(seen[-1][1:], dim=1).detach().numpy().copy()
    fx['att'] = att_dump
    torch.set_grad_enabled(True)
    char_list = [str(i) for i in range(opt.odim)]
    gap = float('inf')
    configs = [(c[0], c[1:], 0.0, None) for c in RECOG] + [('lm_' + c[0], c[1:], LM_WEIGHT, lm) for c in RECOG if c[0] == 'joint_b4']
    for name, (beam, penalty, ctcw, maxr, minr, nbest), lmw, rnnlm in configs:
        args = argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=lmw)
        for u, T in enumerate(LENS):
            with torch.no_grad():
                seqs, scores = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, char_list, rnnlm=rnnlm))
            if len(scores) > 1:
                gap = min(gap, float(np.min(np.abs(np.diff(scores)))))
            fx['%s.u%d.yseq' % (name, u)] = seqs
            fx['%s.u%d.score' % (name, u)] = scores
    return fx, gap


def main():
    mf.install_shims()
    base = dict(np.load(os.path.join(HERE, 'att_types_tiny.npz')))
    feats, targets = torch.from_numpy(base['feats']), torch.from_numpy(base['targets'])
    assert base['lens'].tolist() == LENS and base['tlens'].tolist() == TLENS
    lm = tiny_lm()
    fx = dict(lm_weight=np.float64(LM_WEIGHT))
    for tag, atype, dlayers in MODELS:
        for seed in range(202, 302):
            run, gap = run_model(atype, dlayers, seed, feats, targets, lm)
            if gap >= MIN_GAP:
                break
        else:
            raise SystemExit('%s: no seed with n-best scores >= %g apart' % (tag, MIN_GAP))
        print(tag, 'seed', seed, 'smallest gap between adjacent n-best scores: %.5f' % gap)
        fx.update({'%s.%s' % (tag, k): v for k, v in run.items()})
        fx[tag + '.seed'] = np.int64(seed)
    np.savez_compressed(os.path.join(HERE, 'dlayers_tiny.npz'), **fx)
    for tag, _, _ in MODELS:
        print(tag, 'loss_ctc %.5f loss_att %.5f acc %.4f' % (float(fx[tag + '.loss_ctc']), float(fx[tag + '.loss_att']), float(fx[tag + '.acc'])))
        for k in sorted(fx):
            if k.startswith(tag + '.') and k.endswith('yseq'):
                print(' ', k, fx[k].tolist(), fx[k.replace('yseq', 'score')].round(4).tolist())


if __name__ == '__main__':
    main()
