#!/usr/bin/env python3
"""Reverberant mixtures (csrc/reverb.hip re2e_wav_reverb, re2e_wav_stft_rev through data/mix_data_loader.collate_wav_device) measured on one
MI355X, at B = 32 utterances of 12.8 s (204 800 samples) and impulse responses of K = 2048, 8000 and 16000 taps:

  1  the convolution kernel alone: the 32 speech jobs of one batch (event timing on one stream), the executed FLOP/s -- 2 (K' + 32) per
     output, K' the taps rounded up to the kernel's trips, over the outputs of whole 32 x 32 tiles -- and that as a share of the
     157.3 TFLOP/s fp32 peak
  2  the same 32 convolutions on the host: scipy.signal.fftconvolve in float64 on 1 and on 16 threads (utterances over a thread pool), and
     np.convolve at the smallest K
  3  the whole reverberant front end (upload, re2e_wav_reverb for speech and noise, re2e_wav_mix_scale, re2e_wav_stft_rev) against the plain
     one, as collate_wav_device runs them (host staging included)
  4  the joint step (config 4 networks) fed through DevicePrefetcher by collate_wav_device with and without reverberation

All arms of a section run in one process, alternated round by round; the tables give the median over the rounds and the (min .. max)
spread.  The result goes between the markers of profiles/wav_reverb.md; what stands outside them is kept.
    python tools/bench_wav_reverb.py [--rounds 5] [--steps 6] [--no-step] [--out profiles/wav_reverb.md]"""
import argparse
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
from robust_e2e_gan_amd.data.mix_data_loader import collate_wav_device
from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher

TAPS = (2048, 8000, 16000)
PEAK_TFLOPS = 157.3
BEGIN, END = '<!-- bench_wav_reverb: begin -->', '<!-- bench_wav_reverb: end -->'


def make_rirs(d, K, n=4):
    """n decaying impulse responses of K taps (unit direct path, RT60 near K / 16 kHz) as .npy, and their scp."""
    rng = np.random.RandomState(K)
    paths = []
    for i in range(n):
        h = rng.randn(K) * np.exp(-6.9 * np.arange(K) / K) * 0.02
        h[0] = 1.0
        p = os.path.join(d, 'rir_%d_%d.npy' % (K, i))
        np.save(p, h.astype(np.float32))
        paths.append(p)
    scp = os.path.join(d, 'rir_%d.scp' % K)
    open(scp, 'w').writelines(p + '\n' for p in paths)
    return scp


def executed_flop(lens, K):
    Kt, st = lib.query('re2e_wav_reverb_geometry', 0), lib.query('re2e_wav_reverb_geometry', 4)
    if K <= Kt:
        steps = -(-(K + 32) // st) * st
    else:                                               # every K-tile is rounded up on its own
        full, rest = divmod(K, Kt)
        steps = (Kt + 32) + (full - 1) * Kt + -(-rest // st) * st
    return sum(2.0 * steps * (-(-n // 1024) * 1024) for n in lens)


def host_conv(speech, hs, threads, fn):
    t0 = time.perf_counter()
    one = lambda sh: fn(sh[1].astype(np.float64), sh[0].astype(np.float64))[:sh[0].shape[0]]
    if threads == 1:
        for sh in zip(speech, hs):
            one(sh)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, zip(speech, hs)))
    return (time.perf_counter() - t0) * 1e3


def write_between_markers(path, body):
    old = open(path).read() if os.path.exists(path) else ''
    if BEGIN in old and END in old:
        head, tail = old.split(BEGIN)[0], old.split(END)[1]
    else:
        head, tail = old, ''
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'w').write(head + BEGIN + '\n' + body + '\n' + END + tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wav_reverb.md'))
    ap.add_argument('--no-step', action='store_true', help='sections 1-3 only')
    a = ap.parse_args()
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    from scipy.signal import fftconvolve
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    Kt, Ot = lib.query('re2e_wav_reverb_geometry', 0), lib.query('re2e_wav_reverb_geometry', 1)
    lines = ['# Reverberant mixtures on one MI355X (tools/bench_wav_reverb.py)', '',
             'B = %d utterances of 12.8 s (204 800, 202 752, 200 704, 198 656 samples), noise files of 30 s, impulse responses of K taps; the kernel '
             'stages K-tiles of %d taps and gives a workgroup %d outputs.  Milliseconds, median (min .. max) over %d rounds, arms alternated round '
             'by round.' % (B, Kt, Ot, a.rounds), '']
    with tempfile.TemporaryDirectory() as d:
        make_corpus(d)
        base = dict(noise_repeat_num=1, seed=3, normalize_type=0)
        sets = {0: MixWavDataset(argparse.Namespace(**base), d, os.path.join(d, 'dict'))}
        for K in TAPS:
            sets[K] = MixWavDataset(argparse.Namespace(rir_scp=make_rirs(d, K), rir_max_taps=K, **base), d, os.path.join(d, 'dict'))
        items = {K: sorted([ds[i] for i in range(B)], key=lambda s: s[2].shape[0], reverse=True) for K, ds in sets.items()}
        speech = [it[2] for it in items[0]]
        lens = [s.shape[0] for s in speech]
        n_speech = sum(lens)

        # ---- 1: the kernel alone (the speech jobs of a batch) -----------------------------------------------------------------------------
        longs = lambda v: (lib.ctypes.c_long * B)(*[int(x) for x in v])
        soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
        blob = torch.empty(2 * n_speech, dtype=torch.int16, device=DEV)
        blob[:n_speech].copy_(torch.from_numpy(np.concatenate(speech)))
        clip = torch.zeros(1, dtype=torch.int32, device=DEV)
        kern = {}
        for K in TAPS:
            hs = [it[7][0] for it in items[K]]
            taps = torch.from_numpy(np.concatenate(hs)).to(DEV)
            hoff = np.concatenate([[0], np.cumsum([h.shape[0] for h in hs])[:-1]])
            cols = (longs(soff), longs(lens), longs([0] * B), longs(lens), longs(hoff), longs([h.shape[0] for h in hs]), longs(soff + n_speech))
            kern[K] = (lambda cols=cols, taps=taps: lib.call('re2e_wav_reverb', blob.data_ptr(), blob.numel(), taps.data_ptr(), taps.numel(), *cols, B,
                                                              blob.numel(), None, blob.data_ptr(), clip.data_ptr()), taps)
        res = {K: [] for K in TAPS}
        for _ in range(a.rounds):
            for K in TAPS:
                res[K].append(event_ms(kern[K][0]))
        lines += ['## 1: re2e_wav_reverb alone, the %d speech jobs of one batch (%.2f M outputs)' % (B, n_speech / 1e6), '',
                  '| K | ms | useful GFLOP (2 K per output) | executed TFLOP/s | of the %.1f TFLOP/s fp32 peak |' % PEAK_TFLOPS, '|---|---|---|---|---|']
        for K in TAPS:
            ms = statistics.median(res[K])
            tf = executed_flop(lens, K) / ms / 1e9
            lines.append('| %d | %s | %.1f | %.1f | %.0f %% |' % (K, spread(res[K]), 2.0 * K * n_speech / 1e9, tf, 100.0 * tf / PEAK_TFLOPS))
        lines.append('')

        # ---- 2: the same convolutions on the host -----------------------------------------------------------------------------------------
        host = {}
        for _ in range(2):
            for K in TAPS:
                hs = [it[7][0] for it in items[K]]
                for th in (1, 16):
                    host.setdefault(('scipy.signal.fftconvolve, float64', K, th), []).append(host_conv(speech, hs, th, fftconvolve))
            hs = [it[7][0] for it in items[TAPS[0]]]
            host.setdefault(('np.convolve, float64', TAPS[0], 16), []).append(host_conv(speech, hs, 16, np.convolve))
        lines += ['## 2: the same %d convolutions on the host (2 rounds)' % B, '', '| method | K | threads | ms |', '|---|---|---|---|']
        lines += ['| %s | %d | %d | %s |' % (k[0], k[1], k[2], spread(v)) for k, v in host.items()]
        lines.append('')

        # ---- 3: the whole front end --------------------------------------------------------------------------------------------------------
        arms = {K: (lambda K=K: collate_wav_device(items[K], DEV, None, WANT)) for K in (0,) + TAPS}
        fe = {K: [] for K in arms}
        for _ in range(a.rounds):
            for K, fn in arms.items():
                fe[K].append(event_ms(fn, iters=4))
        lines += ['## 3: collate_wav_device (host staging, upload and every launch; speech AND noise reverberated)', '', '| K | ms |', '|---|---|']
        lines += ['| %s | %s |' % ('no impulse responses' if K == 0 else str(K), spread(v)) for K, v in fe.items()]
        lines.append('')

        # ---- 4: the joint step, fed either way ---------------------------------------------------------------------------------------------
        if not a.no_step:
            import bench
            from robust_e2e_gan_amd.joint_train import JointTrainer, config4_opt
            opt = config4_opt()
            opt.train_dataset_len = B
            targets = lambda n: list(np.random.RandomState(n).randint(1, opt.odim - 1, LABELS))
            fed = {K: [it[:6] + (targets(i),) + it[7:] for i, it in enumerate(items[K])] for K in (0, 8000, 16000)}
            enh, fb, asr, gan = bench.build(opt, torch.device(DEV))
            tr = JointTrainer(opt, enh, fb, asr, gan)
            fcm = torch.stack([torch.zeros(opt.fbank_dim), torch.ones(opt.fbank_dim)]).to(DEV)
            col = lambda b, dv, p: collate_wav_device(b, dv, None, WANT, pool=p)
            step_ms = {K: [] for K in fed}
            warm = 2
            for r in range(a.rounds + 1):
                for K, its in fed.items():
                    n = 0
                    for data in DevicePrefetcher([its] * (warm + a.steps), DEV, collate=col):
                        if n == warm:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        tr.step(data, 0.0, fcm)
                        n += 1
                    torch.cuda.synchronize()
                    if r > 0:                                            # round 0 warms every arm up
                        step_ms[K].append((time.perf_counter() - t0) * 1e3 / a.steps)
            lines += ['## 4: the joint step (config 4 networks, B = 32, T = 801, %d labels) fed through DevicePrefetcher' % LABELS, '',
                      '| impulse responses | ms per step | minus the plain feed (medians) |', '|---|---|---|']
            for K, v in step_ms.items():
                lines.append('| %s | %s | %+.3f |' % ('none' if K == 0 else '%d taps' % K, spread(v),
                                                       statistics.median(v) - statistics.median(step_ms[0])))
            lines += ['', 'The convolutions run on the prefetcher\'s stream beside the step and use the same matrix cores: what they add to the step is '
                      'at most their own time in section 3, and less where the step leaves compute units idle.', '']
    body = '\n'.join(lines)
    write_between_markers(a.out, body)
    print(body)


if __name__ == '__main__':
    main()
