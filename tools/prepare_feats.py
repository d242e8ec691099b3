#!/usr/bin/env python3
"""The reference's offline data/prepare_feats.py on the device front end (csrc/stft.hip): from ``<data_dir>/clean_wav.scp`` and
``<data_dir>/noise.scp`` write the Kaldi tables ``MixKaldiDataset`` reads --

    <feat_dir>/clean/{feats,angles}.ark    <data_dir>/clean_feats.scp  clean_angles.scp
    <feat_dir>/mix/{feats,angles}.ark      <data_dir>/mix_feats.scp    mix_angles.scp     db.scp

with mixtures ``<utt>__mix<k>``, k < noise_repeat_num, each at a noise file, segment start and SNR ~ U(0, 20) dB drawn from a generator
seeded by (seed, 0, index) -- the draws ``MixWavDataset`` makes in epoch 0 with the same seed, so the two input paths can be compared.
Records are 8-bit compressed as the reference's ``copy-feats --compress=true`` writes them; ``--no-compress`` writes float32 records.
No librosa, no Kaldi binaries.

    python tools/prepare_feats.py <data_dir> <feat_dir> <noise_repeat_num> [--no-compress] [--seed 0] [--batch 16]
                                  [--rir_scp FILE] [--reverb_prob P] [--rir_max_taps N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robust_e2e_gan_amd.data import kaldi_io, wav_io
from robust_e2e_gan_amd.data.mix_data_loader import wav_frames_of, wav_frontend_device
from robust_e2e_gan_amd.data.wav_dataset import draw_mixture, draw_reverb


_Table = kaldi_io.ArkScpWriter          # one ark file and the scp lines that point into it


def prepare(data_dir, feat_dir, noise_repeat_num=1, compress=True, seed=0, device='cuda', batch=16, rir_scp=None, reverb_prob=None,
            rir_max_taps=16000):
    """Returns the draws ``[(item id, noise file index, segment start, dB)]`` the mixtures were made with.  ``rir_scp``: reverberant
    mixtures, with the impulse responses ``MixWavDataset`` draws in epoch 0 (seed, 0, index, 1); the clean tables stay the dry signal."""
    rir_paths = []
    if rir_scp:
        with open(rir_scp, encoding='utf-8') as f:
            rir_paths = [line.split()[-1] for line in f if line.strip()]
    prob = 1.0 if reverb_prob is None else float(reverb_prob)
    rir_of = lambda ri: None if ri is None else wav_io.read_rir(rir_paths[ri], rir_max_taps)
    with open(os.path.join(data_dir, 'clean_wav.scp'), encoding='utf-8') as f:
        clean = [line.split() for line in f if line.strip()]
    with open(os.path.join(data_dir, 'noise.scp'), encoding='utf-8') as f:
        noise_paths = [line.split()[-1] for line in f if line.strip()]
    noises = [wav_io.read_wav(p) for p in noise_paths]
    noise_lens = [int(n.shape[0]) for n in noises]
    for sub in ('clean', 'mix'):
        os.makedirs(os.path.join(feat_dir, sub), exist_ok=True)
    tabs = {(sub, kind): _Table(os.path.join(feat_dir, sub, kind + '.ark'), compress) for sub in ('clean', 'mix') for kind in ('feats', 'angles')}
    draws = []
    for k in range(int(noise_repeat_num)):
        for i in range(0, len(clean), batch):
            part = clean[i:i + batch]
            speech = [wav_io.read_wav(p) for _, p in part]
            mine = [draw_mixture(seed, 0, k * len(clean) + i + j, noise_lens, s.shape[0]) for j, s in enumerate(speech)]
            want = ('mix', 'mix_ang') + (('clean', 'clean_ang') if k == 0 else ())
            reverb = None
            if rir_paths:
                reverb = [tuple(rir_of(ri) for ri in draw_reverb(seed, 0, k * len(clean) + i + j, len(rir_paths), prob)) for j in range(len(part))]
            out = wav_frontend_device(speech, device, [(noises[ni], start % noise_lens[ni], db) for ni, start, db in mine], None, want,
                                      reverb=reverb)
            out = {name: t.cpu().numpy() for name, t in out.items()}
            for j, ((utt, _), s, (ni, start, db)) in enumerate(zip(part, speech, mine)):
                T = wav_frames_of(s.shape[0])
                item = '%s__mix%d' % (utt, k)
                tabs['mix', 'feats'].add(item, out['mix'][j, :T])
                tabs['mix', 'angles'].add(item, out['mix_ang'][j, :T])
                if k == 0:
                    tabs['clean', 'feats'].add(utt, out['clean'][j, :T])
                    tabs['clean', 'angles'].add(utt, out['clean_ang'][j, :T])
                draws.append((item, ni, start, db))
    for (sub, kind), tab in tabs.items():
        tab.close(os.path.join(data_dir, '%s_%s.scp' % (sub, kind)))
    with open(os.path.join(data_dir, 'db.scp'), 'w') as f:
        f.writelines('%s %s\n' % (item, repr(db)) for item, _, _, db in draws)
    return draws


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('data_dir')
    ap.add_argument('feat_dir')
    ap.add_argument('noise_repeat_num', type=int)
    ap.add_argument('--no-compress', action='store_true')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rir_scp', default=None, help='room impulse responses (one wav or .npy per line): reverberant mixtures')
    ap.add_argument('--reverb_prob', type=float, default=None, help='share of reverberant items (default 1.0 with --rir_scp)')
    ap.add_argument('--rir_max_taps', type=int, default=16000)
    a = ap.parse_args()
    draws = prepare(a.data_dir, a.feat_dir, a.noise_repeat_num, not a.no_compress, a.seed, batch=a.batch, rir_scp=a.rir_scp,
                    reverb_prob=a.reverb_prob, rir_max_taps=a.rir_max_taps)
    print('%d mixtures written under %s' % (len(draws), a.feat_dir))


if __name__ == '__main__':
    main()
