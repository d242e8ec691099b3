#!/usr/bin/env python3
"""Speed perturbation (csrc/resample.hip re2e_wav_resample through data/mix_data_loader.collate_wav_device) measured on one MI355X, at
B = 32 utterances of 12.8 s (204 800 samples):

  1  the resample kernel alone: the 32 speech jobs of one batch at 10/9 (speed 0.9) and at 10/11 (speed 1.1), event timing on one stream,
     and the bytes per second it moves (int16 read once, int16 written once).  Its yardstick is MEASURED in the same process: the forward
     STFT kernel on the same 32 utterances (clean stream only: int16 read, one fp32 spectrum written) and the bytes per second IT moves
  2  the same 32 resamplings on the host: scipy.signal.resample_poly in float64 on 1 and on 16 threads (utterances over a thread pool)
  3  the whole front end as collate_wav_device runs it (host staging, upload and every launch) with the speeds 0.9 / 1.0 / 1.1 in turn
     over the batch, with 0.9 for all, and without speeds
  4  the joint step (config 4 networks) fed through DevicePrefetcher with the speeds of section 3; the comparison arm is fed wav files
     of the kernel's own resampled output, so both arms step over the same batch shapes and the difference is the resampling itself

All arms of a section run in one process, alternated round by round; the tables give the median over the rounds and the (min .. max)
spread.  The result goes between the markers of profiles/wav_speed.md; what stands outside them is kept.
    python tools/bench_wav_speed.py [--rounds 5] [--steps 6] [--no-step] [--out profiles/wav_speed.md]"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_wav_frontend import B, DEV, LABELS, WANT, event_ms, make_corpus, spread
from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.data import wav_io
from robust_e2e_gan_amd.data.mix_data_loader import WAV_BINS, collate_wav_device, resample_jobs, resampled_len, wav_frames_of
from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher

RATIOS = ((10, 9), (10, 11))
CYCLE = ((10, 9), None, (10, 11))
BEGIN, END = '<!-- bench_wav_speed: begin -->', '<!-- bench_wav_speed: end -->'


def write_between_markers(path, body):
    old = open(path).read() if os.path.exists(path) else ''
    if BEGIN in old and END in old:
        head, tail = old.split(BEGIN)[0], old.split(END)[1]
    else:
        head, tail = old, ''
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'w').write(head + BEGIN + '\n' + body + '\n' + END + tail)


def host_resample(speech, ratio, threads, fn):
    t0 = time.perf_counter()
    one = lambda s: fn(s.astype(np.float64), ratio[0], ratio[1])
    if threads == 1:
        for s in speech:
            one(s)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, speech))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wav_speed.md'))
    ap.add_argument('--no-step', action='store_true', help='sections 1-3 only')
    a = ap.parse_args()
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    G = lib.query('re2e_wav_resample_geometry', 0)
    lines = ['# Speed perturbation on one MI355X (tools/bench_wav_speed.py)', '',
             'B = %d utterances of 12.8 s (204 800, 202 752, 200 704, 198 656 samples), noise files of 30 s; the kernel gives a workgroup %d outputs.  '
             'Milliseconds, median (min .. max) over %d rounds, arms alternated round by round.' % (B, G, a.rounds), '']
    with tempfile.TemporaryDirectory() as d:
        make_corpus(d)
        ds = MixWavDataset(argparse.Namespace(noise_repeat_num=1, seed=3, normalize_type=0), d, os.path.join(d, 'dict'))
        items = sorted([ds[i] for i in range(B)], key=lambda s: s[2].shape[0], reverse=True)
        speech = [it[2] for it in items]
        lens = [s.shape[0] for s in speech]
        n_speech = sum(lens)

        # ---- 1: the kernel alone, and the forward STFT as its yardstick ------------------------------------------------------------------------
        longs = lambda v: (ctypes.c_long * len(v))(*[int(x) for x in v])
        ints = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
        soff = [int(x) for x in np.concatenate([[0], np.cumsum(lens)[:-1]])]
        room = n_speech + sum(resampled_len(n, (10, 9)) for n in lens)
        blob = torch.empty(room, dtype=torch.int16, device=DEV)
        blob[:n_speech].copy_(torch.from_numpy(np.concatenate(speech)))
        clip = torch.zeros(1, dtype=torch.int32, device=DEV)
        kern, moved = {}, {}
        for ratio in RATIOS:
            jobs, _, end = resample_jobs(list(zip(soff, lens)), [ratio] * B, n_speech)
            cols = [(ints if c in (2, 3) else longs)([j[c] for j in jobs]) for c in range(7)]
            kern[ratio] = lambda cols=cols: lib.call('re2e_wav_resample', blob.data_ptr(), blob.numel(), *cols, B, blob.numel(), None, blob.data_ptr(),
                                                     clip.data_ptr())
            moved[ratio] = 2.0 * (n_speech + sum(j[5] for j in jobs))
        Tmax = max(wav_frames_of(n) for n in lens)
        spec = torch.empty(B, Tmax, WAV_BINS, dtype=torch.float32, device=DEV)
        stft = lambda: lib.call('re2e_wav_stft', blob.data_ptr(), longs(soff), longs(lens), None, None, None, None, B, Tmax, spec.data_ptr(),
                                None, None, None, None, None, None, None)
        stft_bytes = 2.0 * n_speech + 4.0 * WAV_BINS * sum(wav_frames_of(n) for n in lens)
        res = {k: [] for k in list(RATIOS) + ['stft']}
        for _ in range(a.rounds):
            for ratio in RATIOS:
                res[ratio].append(event_ms(kern[ratio]))
            res['stft'].append(event_ms(stft))
        lines += ['## 1: re2e_wav_resample alone, the %d speech jobs of one batch (%.2f M input samples), beside the forward STFT of the same batch' % (B, n_speech / 1e6),
                  '', '| kernel | ms | MB moved (read once + written once) | GB/s |', '|---|---|---|---|']
        for ratio in RATIOS:
            ms = statistics.median(res[ratio])
            lines.append('| re2e_wav_resample %d/%d | %s | %.1f | %.0f |' % (ratio[0], ratio[1], spread(res[ratio]), moved[ratio] / 1e6, moved[ratio] / ms / 1e6))
        ms = statistics.median(res['stft'])
        lines += ['| re2e_wav_stft, clean magnitudes only | %s | %.1f | %.0f |' % (spread(res['stft']), stft_bytes / 1e6, stft_bytes / ms / 1e6), '',
                  'The STFT row is the expectation the resample kernel is read against: a measured rate of this front end on this device, not a derived one.', '']

        # ---- 2: the same resamplings on the host ---------------------------------------------------------------------------------------------
        try:
            from scipy.signal import resample_poly
        except ImportError:
            resample_poly = None
            lines += ['## 2: the host comparison was NOT measured: scipy is not installed here', '']
        if resample_poly is not None:
            host = {}
            for _ in range(2):
                for ratio in RATIOS:
                    for th in (1, 16):
                        host.setdefault((ratio, th), []).append(host_resample(speech, ratio, th, resample_poly))
            lines += ['## 2: the same %d resamplings on the host, scipy.signal.resample_poly in float64 (2 rounds)' % B, '', '| ratio | threads | ms |', '|---|---|---|']
            lines += ['| %d/%d | %d | %s |' % (k[0][0], k[0][1], k[1], spread(v)) for k, v in host.items()]
            lines.append('')

        # ---- 3: the whole front end --------------------------------------------------------------------------------------------------------------
        with_speeds = lambda sp: [it + ((None, None), sp[i % len(sp)]) for i, it in enumerate(items)]
        fed = {'no speeds': items, 'speeds 0.9 / 1.0 / 1.1 in turn': with_speeds(CYCLE), 'speed 0.9 for all': with_speeds(((10, 9),))}
        fe = {k: [] for k in fed}
        for _ in range(a.rounds):
            for k, its in fed.items():
                fe[k].append(event_ms(lambda its=its: collate_wav_device(its, DEV, None, WANT), iters=4))
        lines += ['## 3: collate_wav_device (host staging, upload and every launch)', '', '| batch | ms |', '|---|---|']
        lines += ['| %s | %s |' % (k, spread(v)) for k, v in fe.items()]
        lines.append('')

        # ---- 4: the joint step, fed either way ---------------------------------------------------------------------------------------------------
        if not a.no_step:
            import bench
            from robust_e2e_gan_amd.joint_train import JointTrainer, config4_opt
            opt = config4_opt()
            opt.train_dataset_len = B
            targets = lambda n: list(np.random.RandomState(n).randint(1, opt.odim - 1, LABELS))
            live = [it[:6] + (targets(i),) + it[7:] for i, it in enumerate(with_speeds(CYCLE))]
            # the comparison arm: wav files of the kernel's own resampled output, read back
            pre = []
            for i, it in enumerate(live):
                if it[8] is None:
                    pre.append(it[:7])
                    continue
                n = resampled_len(it[2].shape[0], it[8])
                src = torch.from_numpy(np.array(it[2])).to(DEV)
                out = torch.empty(n, dtype=torch.int16, device=DEV)
                lib.call('re2e_wav_resample', src.data_ptr(), src.numel(), longs([0]), longs([src.numel()]), ints([it[8][0]]), ints([it[8][1]]),
                         longs([0]), longs([n]), longs([0]), 1, n, None, out.data_ptr(), None)
                path = os.path.join(d, 'speed_%02d.wav' % i)
                wav_io.write_wav(path, out.cpu().numpy())
                pre.append(it[:2] + (wav_io.read_wav(path),) + it[3:7])
            arms = {'resampled on the device': live, 'wav files of the resampled output': pre}
            enh, fb, asr, gan = bench.build(opt, torch.device(DEV))
            tr = JointTrainer(opt, enh, fb, asr, gan)
            fcm = torch.stack([torch.zeros(opt.fbank_dim), torch.ones(opt.fbank_dim)]).to(DEV)
            col = lambda b, dv, p: collate_wav_device(b, dv, None, WANT, pool=p)
            step_ms = {k: [] for k in arms}
            warm = 2
            for r in range(a.rounds + 1):
                for k, its in arms.items():
                    n = 0
                    for data in DevicePrefetcher([its] * (warm + a.steps), DEV, collate=col):
                        if n == warm:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        tr.step(data, 0.0, fcm)
                        n += 1
                    torch.cuda.synchronize()
                    if r > 0:                                            # round 0 warms every arm up
                        step_ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            base = statistics.median(step_ms['wav files of the resampled output'])
            lines += ['## 4: the joint step (config 4 networks, B = 32, speeds 0.9 / 1.0 / 1.1 in turn, %d labels) fed through DevicePrefetcher' % LABELS, '',
                      '| speech | ms per step | minus the pre-resampled feed (medians) |', '|---|---|---|']
            for k, v in step_ms.items():
                lines.append('| %s | %s | %+.3f |' % (k, spread(v), statistics.median(v) - base))
            lines += ['', 'Both arms step over the same batch shapes (T = %d frames at speed 0.9); the resampling runs on the prefetcher\'s stream beside '
                      'the step.' % wav_frames_of(resampled_len(lens[0], (10, 9))), '']
        else:
            lines += ['## 4: the joint step was NOT measured in this run (--no-step)', '']
    body = '\n'.join(lines)
    write_between_markers(a.out, body)
    print(body)


if __name__ == '__main__':
    main()
