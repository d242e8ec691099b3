#!/usr/bin/env python3
"""Golden vectors for decoding with RNNLM shallow fusion: n-best lists of the reference's own beam
search (E2E.recognize(..., rnnlm=...), model/e2e_decoder.py:270-272,284-285) on the tiny model of make_fixtures_recog.py
plus ClassifierWithState(RNNLM(12, 6, 10)) (model/lm.py:26-146), for five search configurations at two LM weights, and
a ``predict`` chain with permuted / repeated state rows.  Runs only where the reference can be imported; writes
recog_lm_tiny.npz.  No test imports this file."""
import argparse
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402
from make_fixtures_recog import CONFIGS as BASE_CONFIGS   # noqa: E402

CONFIGS = BASE_CONFIGS + [('ctc_only', 2, 0.0, 1.0, 0.0, 0.0, 2)]       # ctc_weight == 1.0: ctc_beam = V (e2e_decoder.py:233-234)
LM_WEIGHTS = [0.2, 1.0]
LENS = [37, 29, 20]
MIN_GAP = 1e-3            # adjacent n-best scores at least the project's fp32 parity bar apart
# predict chain: 8 positions x 3 rows; before each position the state rows are gathered with CHAIN_PARENTS (one repeat each)
CHAIN_IDS = [[2, 2, 2], [5, 1, 7], [3, 3, 9], [11, 0, 4], [6, 8, 2], [1, 10, 5], [7, 7, 3], [4, 9, 11]]
CHAIN_PARENTS = [None, [1, 0, 0], [2, 2, 1], [0, 1, 1], [1, 2, 0], [2, 0, 2], [0, 0, 1], [1, 2, 2]]


def wtag(w):
    return 'w%03d' % int(round(w * 100))


def nbest_arrays(hyps):
    L = max(len(h['yseq']) for h in hyps)
    seqs = np.full((len(hyps), L), -1, np.int64)
    for i, h in enumerate(hyps):
        seqs[i, :len(h['yseq'])] = h['yseq']
    return seqs, np.array([float(h['score']) for h in hyps], np.float64)


def main():
    mf.install_shims()
    from model.e2e_model import E2E
    from model.feat_model import FbankModel
    from model.lm import ClassifierWithState, RNNLM
    opt = mf.tiny_opt()
    torch.manual_seed(606)
    random.seed(0)
    asr = E2E(opt)
    fb = FbankModel(opt)
    clean, mix, mix_log, cos = mf.synth_batch(3, LENS, seed=11)
    cm = torch.stack([torch.linspace(10, 14, 80), torch.linspace(0.3, 0.6, 80)])
    feats = fb(clean, cm).detach()
    base = dict(np.load(os.path.join(HERE, 'recog_tiny.npz')))
    assert np.array_equal(base['feats'], feats.numpy()), 'not the model / utterances of recog_tiny.npz'
    torch.manual_seed(707)
    lm = ClassifierWithState(RNNLM(opt.odim, 6, 10))
    for prm in lm.parameters():
        prm.data.uniform_(-1.0, 1.0)
    lm.eval()
    fx = dict(lens=np.array(LENS, np.int32), lm_weights=np.array(LM_WEIGHTS, np.float64))
    fx.update(mf.sd_np('lm.', lm))
    char_list = [str(i) for i in range(opt.odim)]
    gap = {w: np.inf for w in LM_WEIGHTS}
    for name, beam, penalty, ctcw, maxr, minr, nbest in CONFIGS:
        for u, T in enumerate(LENS):
            args = argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=0.0)
            with torch.no_grad():
                free = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, char_list))
            if '%s.u%d.yseq' % (name, u) in base:
                assert np.array_equal(free[0], base['%s.u%d.yseq' % (name, u)])
            for w in LM_WEIGHTS:
                args.lm_weight = w
                with torch.no_grad():
                    seqs, scores = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, char_list, rnnlm=lm))
                # 1. the LM must change the answer, or a search that ignored it would pass
                assert seqs.shape != free[0].shape or not np.array_equal(seqs, free[0]), (name, u, w, 'n-best unchanged by the LM')
                # 2. the expected order must not hang on rounding
                if len(scores) > 1:
                    g = float(np.min(np.abs(np.diff(scores))))
                    assert g >= MIN_GAP, (name, u, w, g)
                    gap[w] = min(gap[w], g)
                fx['%s.%s.u%d.yseq' % (name, wtag(w), u)] = seqs
                fx['%s.%s.u%d.score' % (name, wtag(w), u)] = scores
    ids = np.asarray(CHAIN_IDS, np.int64)
    state, lps = None, []
    with torch.no_grad():
        for i in range(len(CHAIN_IDS)):
            if CHAIN_PARENTS[i] is not None:
                par = torch.tensor(CHAIN_PARENTS[i])
                state = {k: v.index_select(0, par) for k, v in state.items()}
            state, lp = lm.predict(state, torch.from_numpy(ids[i]))
            lps.append(lp.numpy().copy())
    fx['chain.ids'] = ids
    fx['chain.parents'] = np.asarray([p if p is not None else [0, 1, 2] for p in CHAIN_PARENTS], np.int64)
    fx['chain.logp'] = np.stack(lps)
    for k, v in state.items():
        fx['chain.' + k] = v.numpy().copy()
    np.savez_compressed(os.path.join(HERE, 'recog_lm_tiny.npz'), **fx)
    print('smallest adjacent-score gap:', {w: float('%.3g' % g) for w, g in gap.items()})
    for k in sorted(fx):
        if k.endswith('yseq'):
            print(k, fx[k].tolist(), fx[k.replace('yseq', 'score')].round(4).tolist())


if __name__ == '__main__':
    main()
