#!/usr/bin/env python3
"""Beam search over several utterances at once (E2E.recognize_batch) against a loop of E2E.recognize over the same utterances, and the two
ways recognize_batch can encode them: as one padded batch (encode='batch', Encoder.encode_batch) or utterance by utterance (encode='each').

Config-4 widths (V = 4233, T' = 200 encoder frames per utterance), random weights, beam 12, maxlenratio = minlenratio so that every search
runs the same number of output positions.  Three configurations -- attention-only, joint (ctc_weight 0.3), joint + RNNLM (256 / 650 units,
lm_weight 0.2) -- and U in {1, 4, 16}.  The arms are alternated ``--rounds`` times in one process after one warm-up each (the way
tools/bench_recog_lm.py compares its arms); a call is timed on the host clock around a device synchronisation, because the loop's cost is
mostly the host's.  The encoder (with the CTC posteriors) is timed the same way by itself, its two arms alternated as well; each arm's
per-position figure is its call total less its own encoder's time.  Device->host bytes per position are those of the copies the searches
make with a full beam, from the shapes.

    python tools/bench_recog_batch.py [--rounds 7] [--us 1 4 16]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, LM_I, LM_H, BEAM, FRAMES = 4233, 256, 650, 12, 800
CONFIGS = (('attention-only', 0.0, False), ('joint 0.3', 0.3, False), ('joint 0.3 + LM', 0.3, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--us', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--rounds', type=int, default=7, help='alternations of the two arms (>= 3)')
    ap.add_argument('--lenratio', type=float, default=0.1, help='maxlenratio = minlenratio: output positions = lenratio x 200 frames')
    a = ap.parse_args()

    import torch
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import lm as lm_mod
    from robust_e2e_gan_amd.model.e2e_model import E2E
    dev = 'cuda:0'
    opt = config4_opt()
    assert opt.odim == V
    torch.manual_seed(21)
    asr = E2E(opt).to(dev).eval()
    torch.manual_seed(22)
    lm = lm_mod.ClassifierWithState(lm_mod.RNNLM(V, LM_I, LM_H))
    lm.predictor.lo.weight.data.uniform_(-0.5, 0.5)
    lm = lm.to(dev).eval()
    umax = max(a.us)
    feats = torch.randn(umax, FRAMES, 80, generator=torch.Generator().manual_seed(4)).to(dev)
    positions = max(1, int(a.lenratio * (FRAMES // 4)))
    ctc_beam = int(BEAM * 1.5)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def encode_each(U):
        with torch.no_grad():
            for u in range(U):
                hpad, _ = asr.enc(feats[u:u + 1], [FRAMES])
                asr.ctc.log_softmax(hpad)

    def encode_batch(U):
        with torch.no_grad():
            if U == 1:                                                       # recognize_batch takes the single-utterance path there
                return encode_each(1)
            hpad, _ = asr.enc.encode_batch(feats[:U], [FRAMES] * U)
            asr.ctc.log_softmax(hpad)

    def alternate(arms, rounds):
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                t[k].append(timed(f)[0])
        med = {k: statistics.median(v) for k, v in t.items()}
        iqr = {k: (lambda q: q[2] - q[0])(statistics.quantiles(v, n=4)) for k, v in t.items()}
        return med, iqr

    rounds = max(3, a.rounds)
    print('beam %d, %d positions per search, %d frames (T\' = %d) per utterance, %d alternations; times in ms (median, interquartile range)'
          % (BEAM, positions, FRAMES, FRAMES // 4, rounds))
    for name, ctcw, with_lm in CONFIGS:
        args = argparse.Namespace(beam_size=BEAM, penalty=0.0, ctc_weight=ctcw, maxlenratio=a.lenratio, minlenratio=a.lenratio, nbest=1, lm_weight=0.2)
        rn = lm if with_lm else None
        for U in a.us:
            lens = [FRAMES] * U
            arms = {'batch': lambda: asr.recognize_batch(feats[:U], lens, args, opt.char_list, rnnlm=rn, encode='batch'),
                    'each': lambda: asr.recognize_batch(feats[:U], lens, args, opt.char_list, rnnlm=rn, encode='each'),
                    'loop': lambda: [asr.recognize(feats[u:u + 1], args, opt.char_list, rnnlm=rn) for u in range(U)]}
            res = {k: timed(f)[1] for k, f in arms.items()}                  # warm-up; the three must agree
            same = all(x['yseq'] == y['yseq'] for k in ('batch', 'each') for b, l in zip(res[k], res['loop']) for x, y in zip(b, l))
            enc_arms = {'batch': lambda: encode_batch(U), 'each': lambda: encode_each(U)}
            for f in enc_arms.values():
                f()
            emed, eiqr = alternate(enc_arms, rounds)
            med, iqr = alternate(arms, rounds)
            enc_of = {'batch': emed['batch'], 'each': emed['each'], 'loop': emed['each']}
            d2h = {'batch': (5 * U * BEAM + U) * 4, 'each': (5 * U * BEAM + U) * 4, 'loop': U * (3 * BEAM * ctc_beam * 4 if ctcw > 0 else BEAM * V * 4)}
            print('%-15s U %2d  same n-best %s' % (name, U, same))
            print('    encoder: batch %.1f ms (+-%.1f), each %.1f ms (+-%.1f); each / batch = %.2f (difference %.1f ms against a spread of %.1f ms)'
                  % (emed['batch'], eiqr['batch'], emed['each'], eiqr['each'], emed['each'] / emed['batch'], emed['each'] - emed['batch'], max(eiqr.values())))
            for k in ('batch', 'each', 'loop'):
                print('    %-6s %8.1f ms (+-%.1f)  %7.1f utt/s  %7.3f ms/position (search only)  %8d D2H bytes/position'
                      % (k, med[k], iqr[k], U / med[k] * 1e3, max(med[k] - enc_of[k], 0.0) / positions, d2h[k]))
            print('    each / batch = %.2f (difference %.1f ms against a spread of %.1f ms); loop / batch = %.2f'
                  % (med['each'] / med['batch'], med['each'] - med['batch'], max(iqr['batch'], iqr['each']), med['loop'] / med['batch']))


if __name__ == '__main__':
    main()
