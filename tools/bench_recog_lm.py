#!/usr/bin/env python3
"""Beam search with RNNLM shallow fusion: what the language model costs per output position, on the few-row kernels
(csrc/rnnlm.hip) and on the composed path over the general entry points (model/lm.py COMPOSED_PATH -- the same arithmetic
through re2e_embedding_fwd, re2e_gemm x 5, re2e_lstm_cell_fwd x 2, re2e_log_softmax_rows).

One utterance of 200 encoder frames at the config-4 widths (V = 4233), LM with 256 input / 650 hidden units, ctc_weight 0.3,
beams 12 and 30.  Three arms -- (a) no LM, (b) LM composed, (c) LM fused -- alternated ``--rounds`` times in one process after one
warm-up search each; a search is timed with device events around Decoder.recognize_beam (the encoder runs once, outside) and
divided by its output positions.  Launches per position are counted on the host side of lib.call (library entry points only: the
searches' few torch launches -- index_select of the survivors' states, the host copies -- are the same in every arm).

    python tools/bench_recog_lm.py                          # the three-arm table
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_recog_lm.py --arm fused --beam 12
    python tools/bench_recog_lm.py --kernel-stats DIR/.../*_kernel_stats.csv      # kernel times -> achieved bytes/s"""
import argparse
import collections
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, LM_I, LM_H = 4233, 256, 650
ARMS = ('none', 'composed', 'fused')


def weight_bytes():
    """fp32 bytes of weights each kernel streams per launch, from the shapes."""
    l1 = 4 * LM_H * (LM_I + LM_H) * 4
    l2 = 4 * LM_H * (LM_H + LM_H) * 4
    lo = V * LM_H * 4
    return {'l1': l1, 'l2': l2, 'lo': lo, 'all': l1 + l2 + lo}


def kernel_stats(path):
    wb = weight_bytes()
    rows = {}
    for r in csv.DictReader(open(path)):
        if 'lm_' in r['Name']:
            rows[r['Name']] = (int(r['Calls']), float(r['AverageNs']), float(r['TotalDurationNs']))
    cell = [(k, v) for k, v in rows.items() if 'lm_cell_kernel' in k]
    out = [(k, v) for k, v in rows.items() if 'lm_out_kernel' in k]
    for k, (calls, avg, tot) in sorted(rows.items()):
        print('%-70s calls %6d  average %8.2f us' % (k[:70], calls, avg / 1e3))
    if cell:
        # both layers run the same instantiation when their alignments agree: l1 + l2 bytes over the time of one call of each
        calls = sum(v[0] for _, v in cell)
        tot = sum(v[2] for _, v in cell)
        print('LSTM cells: %.2f us per layer on average, %.2f TB/s of weights (l1 %.1f MB + l2 %.1f MB per position)'
              % (tot / calls / 1e3, (wb['l1'] + wb['l2']) / 2 / (tot / calls) / 1e3, wb['l1'] / 1e6, wb['l2'] / 1e6))
    if out:
        calls = sum(v[0] for _, v in out)
        tot = sum(v[2] for _, v in out)
        print('output layer: %.2f us, %.2f TB/s of weights (%.1f MB)' % (tot / calls / 1e3, wb['lo'] / (tot / calls) / 1e3, wb['lo'] / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--beams', type=int, nargs='+', default=[12, 30])
    ap.add_argument('--beam', type=int, default=None, help='with --arm: the one beam to run')
    ap.add_argument('--rounds', type=int, default=11, help='alternations of the three arms (>= 5)')
    ap.add_argument('--maxlenratio', type=float, default=0.25, help='output positions = maxlenratio x 200 frames')
    ap.add_argument('--arm', choices=ARMS, default=None, help='run only this arm, three searches (for a kernel trace)')
    ap.add_argument('--kernel-stats', default=None, help="rocprofv3's kernel_stats.csv of an --arm fused run: achieved bytes/s")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)

    import torch
    from robust_e2e_gan_amd import lib, ops
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import beam_search, lm as lm_mod
    from robust_e2e_gan_amd.model.e2e_model import E2E
    dev = 'cuda:0'
    opt = config4_opt()
    assert opt.odim == V
    torch.manual_seed(21)
    asr = E2E(opt).to(dev).eval()
    torch.manual_seed(22)
    lm = lm_mod.ClassifierWithState(lm_mod.RNNLM(V, LM_I, LM_H))
    lm.predictor.lo.weight.data.uniform_(-0.5, 0.5)          # a fresh LM (+-0.1) is nearly flat: give it an opinion
    lm = lm.to(dev).eval()
    feats = torch.randn(1, 800, 80, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        hpad, _ = asr.enc(feats, [800])
        lpz = asr.ctc.log_softmax(hpad)[0]
    h = hpad[0]
    assert h.shape[0] == 200

    counts = collections.Counter()
    real_call = lib.call

    def counting_call(name, *args):
        counts[name] += 1
        return real_call(name, *args)

    def search(arm, beam, count=False):
        args = argparse.Namespace(beam_size=beam, penalty=0.0, ctc_weight=0.3, maxlenratio=a.maxlenratio, minlenratio=0.0, nbest=1, lm_weight=0.2)
        lm_mod.COMPOSED_PATH = arm == 'composed'
        if count:
            counts.clear()
            for m in (ops, beam_search, lm_mod):
                m.call = counting_call
        try:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            asr.dec.recognize_beam(h, lpz, args, opt.char_list, rnnlm=None if arm == 'none' else lm)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3
        finally:
            lm_mod.COMPOSED_PATH = False
            for m in (ops, beam_search, lm_mod):
                m.call = real_call

    if a.arm:
        for _ in range(3):
            search(a.arm, a.beam or a.beams[0])
        return
    wb = weight_bytes()
    print('LM weights streamed per position: %.1f MB (l1 %.1f, l2 %.1f, output %.1f)' % (wb['all'] / 1e6, wb['l1'] / 1e6, wb['l2'] / 1e6, wb['lo'] / 1e6))
    for beam in a.beams:
        launches, positions = {}, {}
        for arm in ARMS:                                     # warm-up search of every arm; it also counts the launches
            search(arm, beam, count=True)
            positions[arm] = counts['re2e_attloc_fwd']
            setup = counts['re2e_transpose01'] + 1           # per search, not per position: w_decT and the mlp_enc product
            launches[arm] = (sum(counts.values()) - setup) / positions[arm]
        per_pos = {arm: [] for arm in ARMS}
        for _ in range(max(5, a.rounds)):
            for arm in ARMS:
                per_pos[arm].append(search(arm, beam) / positions[arm])
        med = {arm: statistics.median(v) for arm, v in per_pos.items()}
        print('beam %d, %s positions per search, %d alternations' % (beam, '/'.join(str(positions[x]) for x in ARMS), max(5, a.rounds)))
        print('  %-12s %14s %10s %10s %12s %18s' % ('arm', 'median us/pos', 'min', 'max', 'quartiles', 'lib launches/pos'))
        iqr = {}
        for arm in ARMS:
            v = per_pos[arm]
            q = statistics.quantiles(v, n=4)
            iqr[arm] = q[2] - q[0]
            print('  %-12s %14.1f %10.1f %10.1f %5.1f-%-6.1f %18.1f' % (arm, med[arm], min(v), max(v), q[0], q[2], launches[arm]))
        # spread: the widest interquartile range of an arm (the boxes are shared: single searches land far out, the quartiles do not)
        spread, full = max(iqr.values()), max(max(v) - min(v) for v in per_pos.values())
        cb, cf = med['composed'] - med['none'], med['fused'] - med['none']
        print('  LM cost per position: composed %.1f us, fused %.1f us; difference %.1f us against a spread of %.1f us (widest interquartile '
              'range; widest min-max %.1f us) -> %s' % (cb, cf, cb - cf, spread, full, 'fused is faster beyond the spread' if cb - cf > spread
                                                        else 'NOT separated from the spread'))


if __name__ == '__main__':
    main()
