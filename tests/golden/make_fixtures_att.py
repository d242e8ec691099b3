#!/usr/bin/env python3
"""Golden vectors for the attention types dot, add, coverage and coverage_location (AttDot, AttAdd, AttCov, AttCovLoc,
model/e2e_attention.py:63-196, 302-389, 602-698), and for location as the arm the coverage dumps are compared with: per type, on
``make_fixtures.tiny_opt()`` with ``atype`` set, the reference's own E2E forward / backward, attention dump and beam search.
Runs only where the reference is importable (make_fixtures.REF, with its shims); no test imports it.  Writes att_types_tiny.npz.  Keys of a type are prefixed ``<atype>.``:

  p.att.*                   the attention's parameters (drawn under the seed).  Every OTHER parameter of the four models is e2e_tiny.npz's
                            ``p.*`` (same tiny_opt, loaded before the forward), so that this file stays data of a committable size
  hpad, hlens               the encoder's output on ``feats`` (the same for the four types: they share the encoder)
  loss_ctc, loss_att, acc   E2E.forward on lens [37, 29, 20], labels [5, 4, 3]
  g.*, dfeat                gradients of 0.5 ctc + 0.5 att, every parameter: whole where the tensor has <= BIG elements; of the five larger
                            ones (VGG conv1_2 / conv2_*, bilstm0.weight_ih*) ``gs.*`` = the NS entries at ``sample_index(n)`` and
                            ``gn.*`` = [l2 norm, sum] in float64
  att                       calculate_all_attentions (B, Lmax + 1, T')
  att_steps                 coverage types: the weights of every step (B, Lmax + 1, T'), from the attention's own list -- ``att`` is the
                            last of them repeated there (see run_type)
  <config>.u<k>.yseq/score  n-best lists of recognize, configurations att_b3 and joint_b4 of make_fixtures_recog.py

The seed of a type (``<atype>.seed``) is the first from 202 at which adjacent n-best scores of every configuration and utterance are
>= 1e-3 apart."""
import argparse
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402
from make_fixtures_recog import CONFIGS   # noqa: E402

ATYPES = ('dot', 'add', 'coverage', 'coverage_location')
RECOG = [c for c in CONFIGS if c[0] in ('att_b3', 'joint_b4')]
LENS, TLENS = [37, 29, 20], [5, 4, 3]
MIN_GAP = 1e-3
BIG, NS = 4096, 2048


def sample_index(n):
    """The entries of a flattened gradient of n > BIG elements that the fixture keeps (tests recompute it)."""
    return np.linspace(0, n - 1, NS).astype(np.int64)


def pack_grads(module):
    out = {}
    for k, v in mf.grads_np('', module).items():
        if v.size <= BIG:
            out['g.' + k] = v
        else:
            flat = v.reshape(-1)
            out['gs.' + k] = flat[sample_index(flat.size)].copy()
            out['gn.' + k] = np.array([np.sqrt((flat.astype(np.float64) ** 2).sum()), flat.astype(np.float64).sum()])
    return out


def run_type(atype, seed, feats, targets):
    from model.e2e_model import E2E
    opt = mf.tiny_opt()
    opt.atype = atype
    torch.manual_seed(seed)
    random.seed(0)
    asr = E2E(opt)
    base = dict(np.load(os.path.join(HERE, 'e2e_tiny.npz')))
    own = asr.state_dict()
    shared = {k[2:]: torch.from_numpy(v) for k, v in base.items() if k.startswith('p.') and not k.startswith(('p.att.', 'p.dec.att.'))}
    assert set(shared) == {k for k in own if not k.startswith(('att.', 'dec.att.'))}
    own.update(shared)
    asr.load_state_dict(own)
    asr.train()
    input_sizes, target_sizes = torch.IntTensor(LENS), torch.IntTensor(TLENS)
    feat = feats.clone().requires_grad_(True)
    loss_ctc, loss_att, acc = asr(feat, targets, input_sizes, target_sizes, 0.0)
    asr.zero_grad()
    (0.5 * loss_ctc + 0.5 * loss_att).backward()
    fx = dict(loss_ctc=loss_ctc.detach().numpy(), loss_att=loss_att.detach().numpy(), acc=np.float64(acc), dfeat=feat.grad.numpy().copy())
    hpad, hlens = asr.enc(feats, input_sizes)
    fx.update(hpad=hpad.detach().numpy().copy(), hlens=np.array(list(hlens), np.int32))
    fx.update({k: v for k, v in mf.sd_np('p.', asr).items() if k.startswith('p.att.')})
    fx.update(pack_grads(asr))
    asr.eval()
    seen = []
    hook = asr.att.register_forward_hook(lambda mod, args, out: seen.append(out[1]))
    fx['att'] = np.asarray(asr.calculate_all_attentions(feats, targets, input_sizes, target_sizes)).copy()
    hook.remove()
    if isinstance(seen[-1], list):
        # AttCov / AttCovLoc return the att_prev_list they were given, grown in place, so every entry the decoder collected is the SAME list and
        # its dump (aw[-1] of each, e2e_decoder.py:445-447) repeats the last step's row L times.  The list itself holds the uniform first row and
        # then the weights of every step: those are recorded as ``att_steps``, the dump a caller means
        assert len(seen[-1]) == fx['att'].shape[1] + 1 and all(s is seen[-1] for s in seen)
        fx['att_steps'] = torch.stack(seen[-1][1:], dim=1).detach().numpy().copy()
        assert np.array_equal(fx['att'], np.repeat(fx['att_steps'][:, -1:], fx['att'].shape[1], 1))
    torch.set_grad_enabled(True)
    char_list = [str(i) for i in range(opt.odim)]
    gap = float('inf')
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG:
        args = argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=0.0)
        for u, T in enumerate(LENS):
            with torch.no_grad():
                hyps = asr.recognize(feats[u:u + 1, :T], args, char_list)
            L = max(len(h['yseq']) for h in hyps)
            seqs = np.full((len(hyps), L), -1, np.int64)
            for i, h in enumerate(hyps):
                seqs[i, :len(h['yseq'])] = h['yseq']
            scores = np.array([float(h['score']) for h in hyps], np.float64)
            if len(scores) > 1:
                gap = min(gap, float(np.min(np.abs(np.diff(scores)))))
            fx['%s.u%d.yseq' % (name, u)] = seqs
            fx['%s.u%d.score' % (name, u)] = scores
    return fx, gap, {k: v.clone() for k, v in asr.state_dict().items()}


def main():
    mf.install_shims()
    from model.feat_model import FbankModel
    fb = FbankModel(mf.tiny_opt())
    clean, mix, mix_log, cos = mf.synth_batch(3, LENS, seed=11)
    cm = torch.stack([torch.linspace(10, 14, 80), torch.linspace(0.3, 0.6, 80)])
    feats = fb(clean, cm).detach()
    g = torch.Generator().manual_seed(5)
    targets = torch.randint(1, mf.tiny_opt().odim - 1, (sum(TLENS),), generator=g)
    runs, seeds = {}, {}
    for a in ATYPES:
        for seed in range(202, 302):
            runs[a] = run_type(a, seed, feats, targets)
            if runs[a][1] >= MIN_GAP:
                break
        else:
            raise SystemExit('%s: no seed with n-best scores >= %g apart' % (a, MIN_GAP))
        seeds[a] = seed
        print(a, 'seed', seed, 'smallest gap between adjacent n-best scores: %.5f' % runs[a][1])
    # the state must matter: the same parameters in the type without the coverage state (add has coverage's names but wvec, location
    # exactly coverage_location's) give another attention dump
    from model.e2e_model import E2E
    for cov, base in (('coverage', 'add'), ('coverage_location', 'location')):
        opt = mf.tiny_opt()
        opt.atype = base
        m = E2E(opt)
        m.load_state_dict({k: v for k, v in runs[cov][2].items() if k in m.state_dict()})
        m.eval()
        att = np.asarray(m.calculate_all_attentions(feats, targets, torch.IntTensor(LENS), torch.IntTensor(TLENS)))
        torch.set_grad_enabled(True)
        d = float(np.abs(runs[cov][0]['att_steps'] - att).max())
        print('max |att(%s) - att(%s on the same parameters)| = %.4f' % (cov, base, d))
        assert d > 1e-3, (cov, base, d)
    fx = dict(feats=feats.numpy(), targets=targets.numpy(), lens=np.array(LENS, np.int32), tlens=np.array(TLENS, np.int32))
    for a in ATYPES:
        fx.update({'%s.%s' % (a, k): v for k, v in runs[a][0].items()})
        fx[a + '.seed'] = np.int64(seeds[a])
    np.savez_compressed(os.path.join(HERE, 'att_types_tiny.npz'), **fx)
    for a in ATYPES:
        print(a, 'loss_ctc %.5f loss_att %.5f acc %.4f' % (float(fx[a + '.loss_ctc']), float(fx[a + '.loss_att']), float(fx[a + '.acc'])))
        for k in sorted(fx):
            if k.startswith(a + '.') and k.endswith('yseq'):
                print(' ', k, fx[k].tolist(), fx[k.replace('yseq', 'score')].round(4).tolist())


if __name__ == '__main__':
    main()
