#!/usr/bin/env python3
"""The waveform front end (csrc/stft.hip through data/mix_data_loader.collate_wav_device) measured on one MI355X:

  1  the front end alone at B = 32 utterances of 12.8 s (204 800 samples, T = 801): the upload, re2e_wav_mix_scale and re2e_wav_stft
     (clean, mix, mix_log) timed with events on one stream, and the achieved GB/s against the bytes the launches must move
  2  the float64 and float32 numpy restatements of the same batch on the host (pad + frame + window + rfft + abs + log, clean and mixture),
     on 1 thread and on 16 threads (utterances over a thread pool; numpy's FFT releases the GIL)
  3  torch.stft on the device for the same batch (clean and mixture, abs and log), as a yardstick only
  4  the joint step (config 4 networks) fed through DevicePrefetcher by collate_wav_device, against the same step fed by
     collate_kaldi_device from 8-bit records that tools/prepare_feats.py wrote from the same audio (clean and mix records; the angle
     records are left out, so both arms produce the streams the joint step reads)

All arms of a section run in one process, alternated round by round; the table gives the median over the rounds and the (min .. max)
spread.  Acceptance for 4: the wav-fed step may exceed the Kaldi-fed step by no more than that arm's own min-to-max spread.
    python tools/bench_wav_frontend.py [--rounds 5] [--steps 6] [--out profiles/wav_frontend.md]"""
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

from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.data import wav_io
from robust_e2e_gan_amd.data.mix_data_loader import collate_kaldi_device, collate_wav_device
from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher

DEV = 'cuda:0'
B, SAMPLES, T, LABELS = 32, 204800, 801, 40
WANT = ('clean', 'mix', 'mix_log')


def spread(xs):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(xs), min(xs), max(xs))


def make_corpus(d):
    rng = np.random.RandomState(1)
    os.makedirs(d, exist_ok=True)
    lines = []
    for u in range(B):
        n = SAMPLES - 256 * (u % 4) * 8           # ragged: 801, 793, 785, 777 frames
        x = np.clip(np.round(rng.randn(n) * 4000 * (0.3 + np.abs(np.sin(np.arange(n) / 3000.0)))), -32768, 32767).astype(np.int16)
        wav_io.write_wav(os.path.join(d, 'utt%02d.wav' % u), x)
        lines.append('utt%02d %s\n' % (u, os.path.join(d, 'utt%02d.wav' % u)))
    open(os.path.join(d, 'clean_wav.scp'), 'w').writelines(lines)
    noise = []
    for k in range(4):
        x = np.clip(np.round(rng.randn(16000 * 30) * 1200), -32768, 32767).astype(np.int16)
        wav_io.write_wav(os.path.join(d, 'noise%d.wav' % k), x)
        noise.append('%s\n' % os.path.join(d, 'noise%d.wav' % k))
    open(os.path.join(d, 'noise.scp'), 'w').writelines(noise)
    open(os.path.join(d, 'utt2spk'), 'w').writelines('utt%02d spk%d\n' % (u, u % 5) for u in range(B))
    chars = 'abcdefghijklmnopqrstuvwxyz'
    open(os.path.join(d, 'text_char'), 'w').writelines('utt%02d %s\n' % (u, ' '.join(chars[(u + i) % 26] for i in range(LABELS))) for u in range(B))
    open(os.path.join(d, 'dict'), 'w').writelines('%s %d\n' % (c, i + 1) for i, c in enumerate(chars))


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


def host_restatement(items, dtype, threads):
    win = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(512) / 511)).astype(dtype)

    def one(it):
        s, nz, s0, db = it[2].astype(dtype), it[3], it[4], it[5]
        seg = nz[(s0 + np.arange(s.shape[0])) % nz.shape[0]].astype(dtype)
        g = np.sqrt(np.sum(np.square(s, dtype=np.float64)) / (np.sum(np.square(seg, dtype=np.float64)) * 10 ** (db / 10.0)))
        outs = []
        for sig in (s, s + dtype(g) * seg):
            y = np.pad(sig, 256, mode='reflect')
            idx = 256 * np.arange(1 + s.shape[0] // 256)[:, None] + np.arange(512)[None, :]
            mag = np.maximum(np.abs(np.fft.rfft(y[idx] * win, axis=1)), dtype(1e-7))
            outs.append((mag, 10 * np.log10(mag)))
        return outs
    t0 = time.perf_counter()
    if threads == 1:
        for it in items:
            one(it)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, items))
    return (time.perf_counter() - t0) * 1e3


def torch_stft_arm(speech_d, mix_d, win_d):
    outs = []
    for x in (speech_d, mix_d):
        mag = torch.stft(x, 512, 256, 512, window=win_d, center=True, pad_mode='reflect', return_complex=True).abs().clamp_min(1e-7).transpose(1, 2)
        outs.append((mag.contiguous(), 10 * torch.log10(mag)))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wav_frontend.md'))
    ap.add_argument('--no-step', action='store_true', help='sections 1-3 only')
    a = ap.parse_args()
    assert lib.query('re2e_device_ok') == 1, 'not a gfx950 device'
    import prepare_feats
    from robust_e2e_gan_amd.data.kaldi_dataset import MixKaldiDataset
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    lines = ['# Waveform front end on one MI355X (tools/bench_wav_frontend.py)', '',
             'B = %d utterances of 12.8 s (T = 801, 793, 785, 777 frames), noise files of 30 s; outputs clean, mix, mix_log.  Milliseconds, median '
             '(min .. max) over %d rounds, arms alternated round by round.' % (B, a.rounds), '']
    with tempfile.TemporaryDirectory() as d:
        make_corpus(d)
        args = argparse.Namespace(noise_repeat_num=1, seed=3, normalize_type=1, exp_path=os.path.join(d, 'exp'), num_utt_cmvn=B)
        t0 = time.perf_counter()
        ds = MixWavDataset(args, d, os.path.join(d, 'dict'))            # computes the (2, 257) cmvn on the device
        cmvn_s = time.perf_counter() - t0
        cmvn = torch.from_numpy(ds.cmvn)
        items = [ds[i] for i in range(B)]
        items.sort(key=lambda s: s[2].shape[0], reverse=True)

        # ---- 1: the front end alone ------------------------------------------------------------------------------
        speech, noise = [it[2] for it in items], [(it[3], it[4], it[5]) for it in items]
        n_speech = sum(s.shape[0] for s in speech)
        longs = lambda v: (lib.ctypes.c_long * B)(*[int(x) for x in v])
        blob_h = torch.from_numpy(np.concatenate(speech + list({id(x[0]): x[0] for x in noise}.values()))).pin_memory()
        blob = blob_h.to(DEV)
        soff = np.concatenate([[0], np.cumsum([s.shape[0] for s in speech])[:-1]])
        where, pos = {}, n_speech
        for x in noise:
            if id(x[0]) not in where:
                where[id(x[0])] = pos
                pos += x[0].shape[0]
        idx = (longs(soff), longs([s.shape[0] for s in speech]), longs([where[id(x[0])] for x in noise]), longs([x[0].shape[0] for x in noise]),
               longs([x[1] for x in noise]))
        db = (lib.ctypes.c_float * B)(*[x[2] for x in noise])
        scale = torch.empty(B, device=DEV)
        zeros = torch.zeros(1, dtype=torch.int32, device=DEV)
        outs = [torch.empty(B, T, 257, device=DEV) for _ in range(3)]
        cm_d = cmvn.to(DEV)
        f_up = lambda: blob.copy_(blob_h, non_blocking=True)
        f_scale = lambda: lib.call('re2e_wav_mix_scale', blob.data_ptr(), *idx, db, B, scale.data_ptr(), zeros.data_ptr())
        f_stft = lambda: lib.call('re2e_wav_stft', blob.data_ptr(), *idx, scale.data_ptr(), B, T, outs[0].data_ptr(), None, outs[1].data_ptr(),
                                  outs[2].data_ptr(), None, None, None, cm_d.data_ptr())
        f_all = lambda: (f_up(), f_scale(), f_stft())
        f_collate = lambda: collate_wav_device(items, DEV, cmvn, WANT)
        win_d = torch.from_numpy((0.54 - 0.46 * np.cos(2 * np.pi * np.arange(512) / 511)).astype(np.float32)).to(DEV)
        minlen = min(s.shape[0] for s in speech)
        sp_d = torch.stack([torch.from_numpy(s[:minlen].astype(np.float32)) for s in speech]).to(DEV)
        mx_d = sp_d * 1.01
        f_torch = lambda: torch_stft_arm(sp_d, mx_d, win_d)
        arms = {'upload (pinned int16 blob, %.1f MB)' % (blob_h.numel() * 2 / 1e6): f_up, 're2e_wav_mix_scale': f_scale, 're2e_wav_stft': f_stft,
                'upload + mix_scale + stft': f_all, 'collate_wav_device (host staging included)': f_collate,
                'torch.stft + abs + log, clean and mixture (yardstick, %d samples each)' % minlen: f_torch}
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                res[k].append(event_ms(fn))
        rd_scale = 2.0 * n_speech * 2                                  # speech and its noise segment, int16
        mv_stft = 2.0 * n_speech * 2 + 3.0 * B * T * 257 * 4            # both streams read once (+ a 1/8 halo from cache), three fp32 tensors written
        lines += ['## 1 and 3: device launches alone', '', '| launch | ms | |', '|---|---|---|']
        for k in arms:
            note = ''
            if k == 're2e_wav_mix_scale':
                note = '%.0f GB/s of %.1f MB read' % (rd_scale / statistics.median(res[k]) / 1e6, rd_scale / 1e6)
            if k == 're2e_wav_stft':
                note = '%.0f GB/s of %.1f MB moved (%.1f MB PCM in, %.1f MB fp32 out)' % (mv_stft / statistics.median(res[k]) / 1e6, mv_stft / 1e6,
                                                                                       4.0 * n_speech / 1e6, 3.0 * B * T * 257 * 4 / 1e6)
            if k.startswith('upload (') :
                note = '%.1f GB/s over PCIe' % (blob_h.numel() * 2 / statistics.median(res[k]) / 1e6)
            lines.append('| %s | %s | %s |' % (k, spread(res[k]), note))
        lines += ['', 'CMVN over the %d mixtures on the device (MixWavDataset.compute_cmvn, wav files read included): %.2f s.' % (B, cmvn_s), '']

        # ---- 2: the numpy restatements on the host ----------------------------------------------------------------
        host = {(dt.__name__, th): [] for dt in (np.float64, np.float32) for th in (1, 16)}
        for _ in range(max(2, a.rounds // 2)):
            for dt in (np.float64, np.float32):
                for th in (1, 16):
                    host[dt.__name__, th].append(host_restatement(items, dt, th))
        lines += ['## 2: the same batch in numpy on the host', '', '| restatement | threads | ms |', '|---|---|---|']
        lines += ['| %s | %d | %s |' % (k[0], k[1], spread(v)) for k, v in host.items()]
        lines.append('')

        # ---- 4: the joint step, fed either way --------------------------------------------------------------------
        if not a.no_step:
            import bench
            from robust_e2e_gan_amd.joint_train import JointTrainer, config4_opt
            prepare_feats.prepare(d, os.path.join(d, 'feats'), 1, compress=True, seed=3, device=DEV, batch=8)
            kd = MixKaldiDataset(argparse.Namespace(feat_type='kaldi_magspec', normalize_type=0), d, os.path.join(d, 'dict'), raw=True)
            kitems = [kd[i] for i in range(len(kd))]
            opt = config4_opt()
            opt.train_dataset_len = B
            targets = lambda n: list(np.random.RandomState(n).randint(1, opt.odim - 1, LABELS))
            items4 = [it[:6] + (targets(i),) for i, it in enumerate(items)]
            kitems = [it[:4] + (None, None, targets(i)) for i, it in enumerate(sorted(kitems, key=lambda s: s[3].rows, reverse=True))]          # no angle records: the same three streams
            enh, fb, asr, gan = bench.build(opt, torch.device(DEV))
            tr = JointTrainer(opt, enh, fb, asr, gan)
            fcm = torch.stack([torch.zeros(opt.fbank_dim), torch.ones(opt.fbank_dim)]).to(DEV)
            feeds = {'kaldi records (8-bit, collate_kaldi_device)': (kitems, lambda b, dv, p: collate_kaldi_device(b, dv, cmvn)),
                     'wav (collate_wav_device)': (items4, lambda b, dv, p: collate_wav_device(b, dv, cmvn, WANT, pool=p))}
            step_ms = {k: [] for k in feeds}
            warm = 2
            for r in range(a.rounds + 1):
                for k, (its, col) in feeds.items():
                    n = 0
                    for data in DevicePrefetcher([its] * (warm + a.steps), DEV, collate=col):
                        if n == warm:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        tr.step(data, 0.0, fcm)
                        n += 1
                    torch.cuda.synchronize()
                    if r > 0:                                            # round 0 warms both arms up
                        step_ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            kk, wk = list(feeds)
            over = statistics.median(step_ms[wk]) - statistics.median(step_ms[kk])
            room = max(step_ms[kk]) - min(step_ms[kk])
            lines += ['## 4: the joint step (config 4 networks, B = 32, T = 801, %d labels) through DevicePrefetcher' % LABELS, '',
                      '| fed by | ms per step |', '|---|---|']
            lines += ['| %s | %s |' % (k, spread(v)) for k, v in step_ms.items()]
            parts = {k: statistics.median(res[k]) for k in res}
            bound = max(('upload', parts[[k for k in parts if k.startswith('upload (')][0]]), ('mix_scale', parts['re2e_wav_mix_scale']),
                        ('stft', parts['re2e_wav_stft']), key=lambda kv: kv[1])
            lines += ['', 'wav-fed minus Kaldi-fed (medians): %+.3f ms; the Kaldi arm\'s own min-to-max spread: %.3f ms -> %s.' % (
                over, room, 'within it' if over <= room else 'EXCEEDS it; of the front end\'s parts the longest is %s (%.3f ms)' % bound), '']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
