#!/usr/bin/env python3
"""Word-level LMs in the beam search (model/extlm.py): what LookAheadWordLM and MultiLevelLM cost per output position on the kernels of
csrc/wordlm.hip and on the arbiter path (extlm.ARBITER_PATH: torch softmax / cumsum / log_softmax on the device plus a per-row Python
walk of the flat tree).

Workload: a 65000-word dictionary over 26 letters, word RNNLM with 650 hidden units, 52 labels, ``beam`` rows per position (12 and 30),
``--positions`` positions per chain; the state rows are gathered with a fixed permutation between positions, as the search gathers the
survivors.  Labels: one position in six is a <space>, either for all rows at once (``aligned``: the hypotheses of a beam share most of
their prefix) or drawn per row (``independent``: then nearly every position has SOME row at a space, the word LM's worst case).  A chain
is timed with device events after one warm-up chain per arm; the arms alternate ``--rounds`` times.  Also: the ``index_select`` of the
(n, Vw) cumsum state alone, and the bytes that cross to the host per position inside Decoder.recognize_beam_batch with and without the
word LM (counted at torch.Tensor.cpu).

    python tools/bench_recog_wordlm.py"""
import argparse
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VW, LM_I, LM_H, VC = 65000, 256, 650, 52


def dictionaries(seed=3):
    rng = random.Random(seed)
    letters = [chr(ord('a') + i) for i in range(26)]
    chars = ['<blank>', '<space>'] + letters + [chr(ord('A') + i) for i in range(VC - 29)] + ['<eos>']
    words, seen = ['<blank>', '<unk>', '<eos>'], set()
    while len(words) < VW:
        w = ''.join(rng.choice(letters[:14]) for _ in range(rng.randint(1, 7)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return {w: i for i, w in enumerate(words)}, {c: i for i, c in enumerate(chars)}, chars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--beams', type=int, nargs='+', default=[12, 30])
    ap.add_argument('--positions', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--spaces', nargs='+', default=['aligned', 'independent'], choices=['aligned', 'independent'])
    a = ap.parse_args()

    import numpy as np
    import torch
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import extlm
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    dev = 'cuda:0'
    word_dict, char_dict, chars = dictionaries()
    torch.manual_seed(22)
    wordlm, sublm = RNNLM(VW, LM_I, LM_H), RNNLM(VC, LM_I, LM_H)
    for m in (wordlm, sublm):
        m.lo.weight.data.uniform_(-0.5, 0.5)
    models = {'look-ahead': ClassifierWithState(extlm.LookAheadWordLM(wordlm, word_dict, char_dict)).to(dev).eval(),
              'multi-level': ClassifierWithState(extlm.MultiLevelLM(wordlm, sublm, word_dict, char_dict)).to(dev).eval()}
    tree = models['look-ahead'].predictor.tree
    print('dictionary: %d words, %d tree nodes; word LM %d x %d output layer (%.0f MB of fp32 weights per step)'
          % (VW, tree.n_nodes, VW, LM_H, (VW * LM_H + 4 * LM_H * (LM_I + 3 * LM_H)) * 4 / 1e6))

    def labels_for(n, mode, seed):
        rng = np.random.RandomState(seed)
        lab = rng.randint(2, 16, size=(a.positions, n)).astype(np.int32)           # letters a .. n: the dictionary's alphabet
        if mode == 'aligned':
            lab[5::6] = 1
        else:
            lab[rng.rand(a.positions, n) < 1.0 / 6] = 1
        lab[0] = VC - 1                                                             # the search starts from <eos>
        return lab

    def chain(lm, lab, parents, arbiter):
        extlm.ARBITER_PATH = arbiter
        try:
            ids = torch.from_numpy(lab).to(dev)
            state = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(lab.shape[0]):
                if state is not None:
                    state = {k: v.index_select(0, parents) for k, v in state.items()}
                state, lp = lm.predict(state, ids[i], labels=lab[i])
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3 / lab.shape[0]
        finally:
            extlm.ARBITER_PATH = False

    for beam in a.beams:
        parents = torch.from_numpy(np.random.RandomState(beam).randint(0, beam, size=beam).astype(np.int64)).to(dev)
        for mode in a.spaces:
            lab = labels_for(beam, mode, beam)
            frac = float((lab[1:] == 1).any(1).mean())
            print('beam %d, spaces %s: %d positions, %.0f %% of them with a row at a space, %d alternations'
                  % (beam, mode, a.positions, 100 * frac, a.rounds))
            print('  %-12s %-8s %14s %10s %10s %14s' % ('model', 'path', 'median us/pos', 'min', 'max', 'quartiles'))
            for name, lm in models.items():
                per = {False: [], True: []}
                for arb in (False, True):
                    chain(lm, lab, parents, arb)                                    # warm-up
                for _ in range(max(5, a.rounds)):
                    for arb in (False, True):
                        per[arb].append(chain(lm, lab, parents, arb))
                med, iqr = {}, {}
                for arb in (False, True):
                    v = per[arb]
                    q = statistics.quantiles(v, n=4)
                    med[arb], iqr[arb] = statistics.median(v), q[2] - q[0]
                    print('  %-12s %-8s %14.1f %10.1f %10.1f %6.1f-%-7.1f' % (name, 'arbiter' if arb else 'kernels', med[arb], min(v), max(v), q[0], q[2]))
                diff, spread = med[True] - med[False], max(iqr.values())
                print('  %s: kernels %.1f us, arbiter %.1f us per position; difference %.1f us against a spread of %.1f us -> %s'
                      % (name, med[False], med[True], diff, spread, 'the kernels are faster beyond the spread' if diff > spread
                         else 'the kernels are NOT faster than the arbiter beyond the spread'))
        # the survivors' gather of the (n, Vw) cumsum state, alone
        cs = torch.rand(beam, VW, device=dev)
        for _ in range(5):
            cs.index_select(0, parents)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(200):
            cs.index_select(0, parents)
        t1.record()
        t1.synchronize()
        print('beam %d: index_select of the (%d, %d) cumsum state: %.1f us per call (%.1f MB read + written)'
              % (beam, beam, VW, t0.elapsed_time(t1) * 1e3 / 200, 2 * beam * VW * 4 / 1e6))

    # bytes to the host per position inside the batched search
    opt = config4_opt(odim=VC, char_list=chars)
    torch.manual_seed(31)
    asr = E2E(opt).to(dev).eval()
    feats = torch.randn(3, 800, 80, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        hs = [asr.enc(feats[u:u + 1, :T], [T])[0][0] for u, T in enumerate((800, 640, 480))]
    from robust_e2e_gan_amd.model import beam_search
    moved, positions = [0], [0]
    real_cpu, real_call = torch.Tensor.cpu, beam_search.call

    def counting_cpu(t, *args, **kw):
        if t.is_cuda:
            moved[0] += t.numel() * t.element_size()
        return real_cpu(t, *args, **kw)

    def counting_call(name, *args):
        positions[0] += name == 're2e_attloc_fwd_rows'
        return real_call(name, *args)

    for beam in a.beams:
        args = argparse.Namespace(beam_size=beam, penalty=0.0, ctc_weight=0.0, maxlenratio=0.1, minlenratio=0.0, nbest=1, lm_weight=0.5)
        for name, lm in [('no LM', None)] + list(models.items()):
            moved[0], positions[0] = 0, 0
            torch.Tensor.cpu, beam_search.call = counting_cpu, counting_call
            try:
                asr.dec.recognize_beam_batch(hs, None, args, chars, rnnlm=lm)
            finally:
                torch.Tensor.cpu, beam_search.call = real_cpu, real_call
            print('recognize_beam_batch, 3 utterances, beam %d, %-11s: %d positions, %.0f bytes to the host per position'
                  % (beam, name, positions[0], moved[0] / max(1, positions[0])))


if __name__ == '__main__':
    main()
