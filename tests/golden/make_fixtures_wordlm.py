#!/usr/bin/env python3
"""Golden vectors for decoding with the word-level LMs (model/extlm.py:75-216: LookAheadWordLM, MultiLevelLM): n-best lists of the
reference's own beam search (E2E.recognize(..., rnnlm=ClassifierWithState(LookAheadWordLM / MultiLevelLM))) on the tiny model and utterances
of recog_tiny.npz for the search configurations of make_fixtures_recog_lm.py at two LM weights, and a ``predict`` chain per model with
permuted / repeated state rows.  The 12 labels are named so that 0 is <blank>, 1 <space>, 2 .. 10 the letters a .. i and 11 <eos>; the word
dictionary has 32 entries.  Runs only where the reference can be imported (kenlm is stubbed); writes wordlm_tiny.npz.  No test imports this
file.

One shim: upstream's MultiLevelLM accumulates ``clm_logprob`` with ``+=``, which from the second letter of a word on adds IN PLACE to the
0-dim tensor held by the parent's state tuple -- hypotheses that extend the same parent then see each other's letters.  The states here are
per hypothesis by definition, so the subclass below hands upstream's forward a private copy of that accumulator; nothing else differs."""
import argparse
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402
from make_fixtures_recog_lm import CONFIGS, LENS, LM_WEIGHTS, MIN_GAP, nbest_arrays, wtag   # noqa: E402

CHARS = ['<blank>', '<space>'] + list('abcdefghi') + ['<eos>']
WORDS = ['<blank>', '<unk>', '<eos>', 'a', 'ab', 'abc', 'abd', 'b', 'ba', 'bad', 'bag', 'cab', 'dab', 'dig', 'e', 'ed', 'egg', 'fad', 'fig',
         'gab', 'had', 'hid', 'i', 'ice', 'id', 'if', 'bead', 'face', 'high', 'xyz', 'deaf', 'chef']      # 'xyz': symbols outside the character set
SP, EOS = 1, 11
# predict chains: 10 positions x 3 rows (position 0 starts from no state); before each position the state rows are gathered with CHAIN_PARENTS
CHAIN_IDS = [[11, 11, 11], [2, 3, 9], [3, 1, 1], [4, 2, 7], [1, 8, 8], [5, 1, 2], [10, 6, 1], [8, 1, 2], [11, 3, 3], [1, 0, 1]]
CHAIN_PARENTS = [None, [0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2], [1, 1, 2], [0, 1, 2], [0, 1, 1], [2, 0, 1], [0, 1, 2]]


def main():
    mf.install_shims()
    from model.e2e_model import E2E
    from model.extlm import LookAheadWordLM, MultiLevelLM
    from model.feat_model import FbankModel
    from model.lm import ClassifierWithState, RNNLM

    class PerHypothesisMultiLevelLM(MultiLevelLM):
        def forward(self, state, x):
            if state is not None and torch.is_tensor(state[5]):
                state = tuple(state[:5]) + (state[5].clone(),)
            return super(PerHypothesisMultiLevelLM, self).forward(state, x)

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
    word_dict = {w: i for i, w in enumerate(WORDS)}
    char_dict = {c: i for i, c in enumerate(CHARS)}
    torch.manual_seed(808)
    wordlm, charlm = RNNLM(len(WORDS), 5, 8), RNNLM(len(CHARS), 6, 10)
    for m in (wordlm, charlm):
        for prm in m.parameters():
            prm.data.uniform_(-1.0, 1.0)
    models = {'la': ClassifierWithState(LookAheadWordLM(wordlm, word_dict, char_dict)),
              'ml': ClassifierWithState(PerHypothesisMultiLevelLM(wordlm, charlm, word_dict, char_dict))}
    for m in models.values():
        m.eval()
    fx = dict(lens=np.array(LENS, np.int32), lm_weights=np.array(LM_WEIGHTS, np.float64), words=np.array(WORDS), chars=np.array(CHARS))
    fx.update(mf.sd_np('la.', models['la']))
    fx.update(mf.sd_np('ml.', models['ml']))
    gap = {(tag, w): np.inf for tag in models for w in LM_WEIGHTS}
    for name, beam, penalty, ctcw, maxr, minr, nbest in CONFIGS:
        for u, T in enumerate(LENS):
            args = argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=0.0)
            with torch.no_grad():
                free = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, CHARS))
            if '%s.u%d.yseq' % (name, u) in base:
                assert np.array_equal(free[0], base['%s.u%d.yseq' % (name, u)])
            for tag, lm in models.items():
                for w in LM_WEIGHTS:
                    args.lm_weight = w
                    with torch.no_grad():
                        seqs, scores = nbest_arrays(asr.recognize(feats[u:u + 1, :T], args, CHARS, rnnlm=lm))
                    # 1. the LM must change the answer, or a search that ignored it would pass
                    assert seqs.shape != free[0].shape or not np.array_equal(seqs, free[0]), (tag, name, u, w, 'n-best unchanged by the LM')
                    # 2. the expected order must not hang on rounding
                    if len(scores) > 1:
                        g = float(np.min(np.abs(np.diff(scores))))
                        assert g >= MIN_GAP, (tag, name, u, w, g)
                        gap[tag, w] = min(gap[tag, w], g)
                    fx['%s.%s.%s.u%d.yseq' % (tag, name, wtag(w), u)] = seqs
                    fx['%s.%s.%s.u%d.score' % (tag, name, wtag(w), u)] = scores
    ids = np.asarray(CHAIN_IDS, np.int64)
    for tag, lm in models.items():
        node_at = 2 if tag == 'la' else 3
        seen = set()
        states, lps = [None] * 3, []
        with torch.no_grad():
            for i in range(len(CHAIN_IDS)):
                if CHAIN_PARENTS[i] is not None:
                    states = [states[p] for p in CHAIN_PARENTS[i]]
                row = []
                for r in range(3):
                    if states[r] is not None:
                        node, x = states[r][node_at], int(ids[i, r])
                        if x == SP:
                            seen.add('space from None' if node is None else 'space at word end' if node[1] >= 0 else 'space at non-end')
                        elif node is not None and x not in node[0]:
                            seen.add('off-tree label')
                    states[r], lp = lm.predict(states[r], torch.from_numpy(ids[i, r:r + 1]))
                    row.append(lp.numpy()[0].copy())
                lps.append(np.stack(row))
        assert seen == {'space from None', 'space at word end', 'space at non-end', 'off-tree label'}, (tag, seen)
        fx[tag + '.chain.logp'] = np.stack(lps)
        final = [st[0] if tag == 'la' else st[1] for st in states]                 # the word LM's state
        for k in ('c1', 'h1', 'c2', 'h2'):
            fx['%s.chain.%s' % (tag, k)] = np.concatenate([st[k].numpy() for st in final])
        if tag == 'la':
            fx['la.chain.cumsum'] = np.concatenate([st[1].numpy() for st in states])
        else:
            for k in ('c1', 'h1', 'c2', 'h2'):
                fx['ml.chain.sub_' + k] = np.concatenate([st[0][k].numpy() for st in states])
            fx['ml.chain.wlm_logprobs'] = np.concatenate([st[2].numpy() for st in states])
            fx['ml.chain.clm_logprob'] = np.asarray([float(st[5]) for st in states], np.float32)
    fx['chain.ids'] = ids
    fx['chain.parents'] = np.asarray([p if p is not None else [0, 1, 2] for p in CHAIN_PARENTS], np.int64)
    np.savez_compressed(os.path.join(HERE, 'wordlm_tiny.npz'), **fx)
    print('smallest adjacent-score gap:', {k: float('%.3g' % g) for k, g in gap.items()})
    for k in sorted(fx):
        if k.endswith('yseq'):
            print(k, fx[k].tolist(), fx[k.replace('yseq', 'score')].round(4).tolist())


if __name__ == '__main__':
    main()
