"""Numbers for profiles/recog_cli.md, one MI355X, one process:

(a) the aligner (re2e_align_counts) on 7176 x 12 pairs -- a test set's n-best -- with lengths 5 .. 40 over 4233 labels, every hypothesis a
    noisy copy of its reference (about 15 % of the labels substituted, deleted or inserted): time per call, counts only and with paths, by
    device events around the call (table upload + kernel) and on the host clock around the call and a synchronise; next to it the
    plain-Python restatement of tests/refs_align.py on every 50th pair, after checking that both give the same counts on that sample.
(b) joint_recog end to end (recog.run: data set, device decode, enhancer, filterbank, search, result JSON; scoring off) on 64 synthetic
    utterances of 800 frames at the config-4 sizes, random weights, beam 12, ctc-weight 0.3, maxlenratio = minlenratio = 0.1 (20 output
    positions per search, as tools/bench_recog_batch.py): utterances/s at --recog-batch 16 and at --recog-batch 1, alternated three times
    after one warm-up each, host clock around a device synchronise.

    python tools/bench_recog_cli.py [--out profiles/recog_cli_raw.txt]"""
import argparse
import importlib.util
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'
V = 4233


def noisy_pairs(n_ref, nbest, rng):
    refs, hyps, pair_ref = [], [], []
    for r in range(n_ref):
        ref = rng.integers(1, V - 1, int(rng.integers(5, 41))).tolist()
        refs.append(ref)
        for _ in range(nbest):
            h = []
            for t in ref:
                u = rng.random()
                if u < 0.05:
                    continue
                h.append(int(rng.integers(1, V - 1)) if u < 0.10 else t)
                if u > 0.95:
                    h.append(int(rng.integers(1, V - 1)))
            while len(h) < 5:
                h.append(int(rng.integers(1, V - 1)))
            hyps.append(h[:40])
            pair_ref.append(r)
    return refs, hyps, pair_ref


def bench_align(say, calls=20):
    from robust_e2e_gan_amd.utils import score
    spec = importlib.util.spec_from_file_location('refs_align', os.path.join(ROOT, 'tests', 'refs_align.py'))
    refs_align = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refs_align)
    refs, hyps, pair_ref = noisy_pairs(7176, 12, np.random.default_rng(1))
    n = len(hyps)
    ref_flat, ref_off = score.flat_table(refs)
    hyp_flat, hyp_off = score.flat_table(hyps)
    pair_ref = np.asarray(pair_ref, np.int32)
    cap = np.array([len(refs[r]) + len(h) for r, h in zip(pair_ref.tolist(), hyps)], np.int64)
    path_off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    ref_d, hyp_d = torch.from_numpy(ref_flat).to(DEV), torch.from_numpy(hyp_flat).to(DEV)
    counts = torch.empty(n, 6, dtype=torch.int32, device=DEV)
    path = torch.empty(int(path_off[-1]), dtype=torch.uint8, device=DEV)
    say('(a) aligner: %d pairs (%d references x 12), %d + %d labels, costs 4/3/3, %d timed calls after 3 warm-up calls' % (
        n, len(refs), len(ref_flat), len(hyp_flat), calls))
    for name, p, po in (('counts only', None, None), ('with paths', path, path_off)):
        run = lambda: score.align_counts(ref_d, ref_off, hyp_d, hyp_off, pair_ref, (4, 3, 3), counts, p, po)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ev, host = [], []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        q = lambda v: (statistics.median(v), min(v), max(v))
        say('    %-12s device events %.3f ms (min %.3f, max %.3f)   host clock %.3f ms (min %.3f, max %.3f)   %.1f M pairs/s by events' % (
            (name,) + q(ev) + q(host) + (n / statistics.median(ev) / 1e3,)))
    got = counts.cpu().numpy()
    sample = list(range(0, n, 50))
    t0 = time.perf_counter()
    want = [refs_align.align(refs[pair_ref[k]], hyps[k], (4, 3, 3))[0] for k in sample]
    dt = time.perf_counter() - t0
    same = all(got[k].tolist() == w for k, w in zip(sample, want))
    say('    plain Python (tests/refs_align.py) on every 50th pair (%d pairs): %.2f s = %.3f ms/pair, i.e. %.1f s for all pairs; counts equal '
        'the device\'s on the sample: %s' % (len(sample), dt, dt / len(sample) * 1e3, dt / len(sample) * n, same))
    if not same:
        raise SystemExit('the device and the restatement disagree')


def bench_cli(say, rounds=3):
    from robust_e2e_gan_amd import recog
    from robust_e2e_gan_amd.data import kaldi_io
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.options.test_options import TestOptions
    U, T = 64, 800
    rng = np.random.default_rng(2)
    torch.manual_seed(2)
    with tempfile.TemporaryDirectory() as root:
        exp, data = os.path.join(root, 'exp', 'bench'), os.path.join(root, 'data')
        os.makedirs(exp)
        os.makedirs(data)
        opt = config4_opt()
        torch.save({'opt': opt, 'enhance_state_dict': EnhanceModel(opt).state_dict(), 'asr_state_dict': E2E(opt).state_dict(), 'fbank_state_dict': None},
                   os.path.join(exp, 'model.pth'))
        w = kaldi_io.ArkScpWriter(os.path.join(data, 'feats.ark'), False)
        with open(os.path.join(data, 'utt2spk'), 'w') as f, open(os.path.join(data, 'text_char'), 'w', encoding='utf-8') as t:
            for u in range(U):
                w.add('spk%d-utt%02d' % (u % 4, u), (rng.random((T, 257)) * 2.0 + 0.01).astype(np.float32))
                f.write('spk%d-utt%02d spk%d\n' % (u % 4, u, u % 4))
                t.write('spk%d-utt%02d %s\n' % (u % 4, u, ''.join(chr(0x4e00 + int(c)) for c in rng.integers(0, V - 2, 20))))
        w.close(os.path.join(data, 'feats.scp'))
        with open(os.path.join(root, 'train_units.txt'), 'w', encoding='utf-8') as f:
            for k in range(V - 2):
                f.write('%s %d\n' % (chr(0x4e00 + k), k + 1))
        np.save(os.path.join(exp, 'cmvn.npy'), np.stack([np.zeros(257), np.ones(257)]).astype(np.float32))
        np.save(os.path.join(exp, 'fbank_cmvn.npy'), np.stack([np.zeros(80), np.ones(80)]).astype(np.float32))
        argv = ['--recog-dir', data, '--dict_dir', os.path.join(root, 'train_units.txt'), '--checkpoints_dir', os.path.join(root, 'exp'), '--name', 'bench',
                '--works_dir', exp, '--resume', 'model.pth', '--beam-size', '12', '--nbest', '12', '--ctc-weight', '0.3', '--maxlenratio', '0.1',
                '--minlenratio', '0.1', '--verbose', '0', '--no-score']

        def once(batch):
            o = TestOptions().parse(argv + ['--recog-batch', str(batch), '--result-label', os.path.join(root, 'b%d.json' % batch)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            utts = recog.run(o, 'joint')
            torch.cuda.synchronize()
            return time.perf_counter() - t0, utts

        say('(b) joint_recog end to end (checkpoint load, data set, decode, enhancer, filterbank, search, JSON), %d utterances of %d frames, config-4 '
            'sizes, random weights, beam 12, nbest 12, ctc-weight 0.3, 20 positions per search; %d alternations after one warm-up each' % (U, T, rounds))
        res = {16: [], 1: []}
        lists = {}
        for b in (16, 1):
            lists[b] = once(b)[1]
        for _ in range(rounds):
            for b in (16, 1):
                res[b].append(once(b)[0])
        same = all(lists[16][u]['output'][0]['rec_tokenid'] == lists[1][u]['output'][0]['rec_tokenid'] for u in lists[1])
        for b in (16, 1):
            v = res[b]
            say('    --recog-batch %-2d  %.2f s (min %.2f, max %.2f)  %.1f utterances/s (min %.1f, max %.1f)' % (
                b, statistics.median(v), min(v), max(v), U / statistics.median(v), U / max(v), U / min(v)))
        ratios = [x / y for x, y in zip(res[1], res[16])]
        say('    --recog-batch 1 / --recog-batch 16, per alternation: %s; median %.2f (min %.2f, max %.2f); same 1-best: %s' % (
            ', '.join('%.2f' % r for r in ratios), statistics.median(ratios), min(ratios), max(ratios), same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also append the lines to this file')
    ap.add_argument('--only', choices=('align', 'cli'), default=None)
    a = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')

    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is reported without one')
    say('device: %s' % torch.cuda.get_device_name(0))
    if a.only != 'cli':
        bench_align(say)
    if a.only != 'align':
        bench_cli(say)


if __name__ == '__main__':
    main()
