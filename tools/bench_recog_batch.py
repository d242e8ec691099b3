#!/usr/bin/env python3
"""Beam search over several utterances at once (E2E.recognize_batch) against a loop of E2E.recognize over the same utterances.

Config-4 widths (V = 4233, T' = 200 encoder frames per utterance), random weights, beam 12, maxlenratio = minlenratio so that every search
runs the same number of output positions.  Three configurations -- attention-only, joint (ctc_weight 0.3), joint + RNNLM (256 / 650 units,
lm_weight 0.2) -- and U in {1, 4, 16}.  The two arms are alternated ``--rounds`` times in one process after one warm-up each (the way
tools/bench_recog_lm.py compares its arms); a call is timed on the host clock around a device synchronisation, because the loop's cost is
mostly the host's.  Both arms encode every utterance on its own, so the encoder's time is in both; it is measured once and taken out of the
per-position figure.  Device->host bytes per position are those of the copies the two searches make with a full beam, from the shapes.

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

    def encode(U):
        with torch.no_grad():
            for u in range(U):
                hpad, _ = asr.enc(feats[u:u + 1], [FRAMES])
                asr.ctc.log_softmax(hpad)

    print('beam %d, %d positions per search, %d frames (T\' = %d) per utterance, %d alternations; times in ms (median, interquartile range)'
          % (BEAM, positions, FRAMES, FRAMES // 4, max(3, a.rounds)))
    for name, ctcw, with_lm in CONFIGS:
        args = argparse.Namespace(beam_size=BEAM, penalty=0.0, ctc_weight=ctcw, maxlenratio=a.lenratio, minlenratio=a.lenratio, nbest=1, lm_weight=0.2)
        rn = lm if with_lm else None
        for U in a.us:
            lens = [FRAMES] * U
            arms = {'batch': lambda: asr.recognize_batch(feats[:U], lens, args, opt.char_list, rnnlm=rn),
                    'loop': lambda: [asr.recognize(feats[u:u + 1], args, opt.char_list, rnnlm=rn) for u in range(U)]}
            res = {k: timed(f)[1] for k, f in arms.items()}                  # warm-up; the two must agree
            same = all(x['yseq'] == y['yseq'] for b, l in zip(res['batch'], res['loop']) for x, y in zip(b, l))
            enc_ms = statistics.median(timed(lambda: encode(U))[0] for _ in range(3))
            t = {k: [] for k in arms}
            for _ in range(max(3, a.rounds)):
                for k, f in arms.items():
                    t[k].append(timed(f)[0])
            med = {k: statistics.median(v) for k, v in t.items()}
            iqr = {k: (lambda q: q[2] - q[0])(statistics.quantiles(v, n=4)) for k, v in t.items()}
            d2h = {'batch': (5 * U * BEAM + U) * 4, 'loop': U * (3 * BEAM * ctc_beam * 4 if ctcw > 0 else BEAM * V * 4)}
            print('%-15s U %2d  same n-best %s  encoder %.1f' % (name, U, same, enc_ms))
            for k in ('batch', 'loop'):
                print('    %-6s %8.1f ms (+-%.1f)  %7.1f utt/s  %7.3f ms/position (search only)  %8d D2H bytes/position'
                      % (k, med[k], iqr[k], U / med[k] * 1e3, max(med[k] - enc_ms, 0.0) / positions, d2h[k]))
            print('    loop / batch = %.2f (difference %.1f ms against a spread of %.1f ms)' % (med['loop'] / med['batch'], med['loop'] - med['batch'],
                                                                                             max(iqr.values())))


if __name__ == '__main__':
    main()
