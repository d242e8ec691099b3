#!/usr/bin/env python3
"""The inverse STFT and the signal metrics (csrc/stft.hip: re2e_wav_istft, re2e_wav_sdr_sums) measured on one MI355X at B = 32 utterances of
12.8 s (204 800 samples, T = 801; ragged as in tools/bench_wav_frontend.py):

  1  re2e_wav_istft with the float output and with the int16 output, re2e_wav_sdr_sums, and -- the yardstick, timed in the same process --
     re2e_wav_stft in the form profiles/wav_frontend.md reports (noise mixed in; clean, mix, mix_log), each timed with events on one stream
     and given as achieved GB/s of the bytes the launch must move (the inverse: two (B,T,257) fp32 reads plus the sample writes)
  2  the same inverse in numpy on the host (irfft + window + two-frame gather, float64 and float32), on 1 thread and on 16 threads

All arms of a section run in one process, alternated round by round; the table gives the median over the rounds and the (min .. max) spread.
The launches of an arm run back to back on the same buffers, as in tools/bench_wav_frontend.py: both directions see the same cache state, so
the GB/s figures compare with each other (they are not cold-HBM figures).
    python tools/bench_wav_istft.py [--rounds 5] [--out profiles/wav_istft.md]"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from robust_e2e_gan_amd import lib

DEV = 'cuda:0'
B, SAMPLES, T = 32, 204800, 801


def spread(xs):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(xs), min(xs), max(xs))


def event_ms(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def host_inverse(mags, angs, lens, dtype, threads):
    n = np.arange(512, dtype=np.float64)
    w = (0.54 - 0.46 * np.cos(2 * np.pi * n / 511)).astype(dtype)
    inv = (1.0 / (np.square(w[:256]) + np.square(w[256:]))).astype(dtype)

    def one(k):
        mag, ang, L = mags[k].astype(dtype), angs[k].astype(dtype), lens[k]
        X = mag * np.cos(ang) + 1j * (mag * np.sin(ang))
        x = np.fft.irfft(X, 512, axis=1) * w
        y = np.zeros(L, dtype)
        y[:256 * (x.shape[0] - 1)] = ((x[:-1, 256:] + x[1:, :256]) * inv).reshape(-1)
        return y
    t0 = time.perf_counter()
    if threads == 1:
        for k in range(len(lens)):
            one(k)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(len(lens))))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wav_istft.md'))
    a = ap.parse_args()
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    rng = np.random.RandomState(1)
    lens = [SAMPLES - 256 * (u % 4) * 8 for u in range(B)]          # 801, 793, 785, 777 frames
    speech = [np.clip(np.round(rng.randn(n) * 4000 * (0.3 + np.abs(np.sin(np.arange(n) / 3000.0)))), -32768, 32767).astype(np.int16) for n in lens]
    noise = np.clip(np.round(rng.randn(16000 * 30) * 1200), -32768, 32767).astype(np.int16)
    n_speech = sum(lens)
    longs = lambda v: (lib.ctypes.c_long * B)(*[int(x) for x in v])
    blob = torch.from_numpy(np.concatenate(speech + [noise])).to(DEV)
    soff = np.concatenate([[0], np.cumsum(lens)[:-1]])
    idx = (longs(soff), longs(lens), longs([n_speech] * B), longs([noise.shape[0]] * B), longs([1000 * u for u in range(B)]))
    db = (lib.ctypes.c_float * B)(*[5.0 + (u % 10) for u in range(B)])
    scale = torch.empty(B, device=DEV)
    zeros = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.call('re2e_wav_mix_scale', blob.data_ptr(), *idx, db, B, scale.data_ptr(), zeros.data_ptr())
    fwd = [torch.empty(B, T, 257, device=DEV) for _ in range(3)]
    mag, ang = torch.empty(B, T, 257, device=DEV), torch.empty(B, T, 257, device=DEV)
    lib.call('re2e_wav_stft', blob.data_ptr(), idx[0], idx[1], None, None, None, None, B, T, mag.data_ptr(), None, None, None, None, ang.data_ptr(), None, None)
    wav = torch.empty(n_speech, device=DEV)
    pcm = torch.empty(n_speech, dtype=torch.int16, device=DEV)
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    sums = torch.empty(B, 3, dtype=torch.float64, device=DEV)
    f_stft = lambda: lib.call('re2e_wav_stft', blob.data_ptr(), *idx, scale.data_ptr(), B, T, fwd[0].data_ptr(), None, fwd[1].data_ptr(), fwd[2].data_ptr(),
                              None, None, None, None)
    f_f32 = lambda: lib.call('re2e_wav_istft', mag.data_ptr(), ang.data_ptr(), longs(soff), longs(lens), B, T, n_speech, wav.data_ptr(), None, None)
    f_i16 = lambda: lib.call('re2e_wav_istft', mag.data_ptr(), ang.data_ptr(), longs(soff), longs(lens), B, T, n_speech, None, pcm.data_ptr(), clip.data_ptr())
    f_sdr = lambda: lib.call('re2e_wav_sdr_sums', blob.data_ptr(), longs(soff), wav.data_ptr(), longs(soff), longs(lens), B, sums.data_ptr())
    f_f32()
    f_i16()
    torch.cuda.synchronize()
    back = pcm.cpu().numpy().astype(np.int64)
    worst, pos = 0, 0
    for n, s in zip(lens, speech):
        worst = max(worst, int(np.abs(back[pos:pos + 256 * (n // 256)] - s[:256 * (n // 256)]).max()))
        pos += n
    frames = sum(1 + n // 256 for n in lens)
    rd = 2.0 * frames * 257 * 4
    moved = {'re2e_wav_stft (noise mixed in; clean, mix, mix_log: the form of profiles/wav_frontend.md)': 2.0 * n_speech * 2 + 3.0 * B * T * 257 * 4,
             're2e_wav_istft, float output': rd + 4.0 * n_speech, 're2e_wav_istft, int16 output + clip count': rd + 2.0 * n_speech,
             're2e_wav_sdr_sums': 6.0 * n_speech}
    arms = dict(zip(moved, (f_stft, f_f32, f_i16, f_sdr)))
    res = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            res[k].append(event_ms(fn))
    lines = ['# Inverse STFT and signal metrics on one MI355X (tools/bench_wav_istft.py)', '',
             'B = %d utterances of 12.8 s (T = 801, 793, 785, 777 frames: %d frames, %.1f M samples).  Milliseconds, median (min .. max) over %d rounds, arms '
             'alternated round by round; every arm is 10 launches back to back on the same buffers.' % (B, frames, n_speech / 1e6, a.rounds), '',
             '## 1: device launches alone', '', '| launch | ms | bytes it must move | achieved |', '|---|---|---|---|']
    rate = {}
    for k in arms:
        rate[k] = moved[k] / statistics.median(res[k]) / 1e6
        lines.append('| %s | %s | %.1f MB | %.0f GB/s |' % (k, spread(res[k]), moved[k] / 1e6, rate[k]))
    ks = list(arms)
    ratio = rate[ks[1]] / rate[ks[0]]
    lines += ['', 'The inverse with the float output reaches %.2f of the forward\'s rate in the same process (int16 output: %.2f).  Round trip of the '
              'batch through both kernels to int16: largest difference from the PCM %d LSB.' % (ratio, rate[ks[2]] / rate[ks[0]], worst), '']
    mags, angs = mag.cpu().numpy(), ang.cpu().numpy()
    mags, angs = [mags[b, :1 + n // 256] for b, n in enumerate(lens)], [angs[b, :1 + n // 256] for b, n in enumerate(lens)]
    host = {(dt.__name__, th): [] for dt in (np.float64, np.float32) for th in (1, 16)}
    for _ in range(max(2, a.rounds // 2)):
        for dt in (np.float64, np.float32):
            for th in (1, 16):
                host[dt.__name__, th].append(host_inverse(mags, angs, lens, dt, th))
    lines += ['## 2: the same inverse in numpy on the host', '', '| restatement | threads | ms |', '|---|---|---|']
    lines += ['| %s | %d | %s |' % (k[0], k[1], spread(v)) for k, v in host.items()]
    lines.append('')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
