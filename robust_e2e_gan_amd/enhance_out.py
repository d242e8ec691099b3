"""Dump what a trained enhancer makes of a data set (mirror of the reference's enhance_out.py), and with ``--wav`` the enhanced waveforms
and a figure of merit as well.

    python -m robust_e2e_gan_amd.enhance_out --enhance_dir DATA --dict_dir DICT --resume CKPT --exp_path EXP [--enhance_out_dir enhance_out]

loads ``enhance_state_dict`` of the checkpoint (``EnhanceModel.load_model``), runs the masked inference forward over the clean and the mixture
stream of every item of ``MixKaldiDataset(DATA)`` and writes, under ``EXP/<enhance_out_dir>/``,

    clean_enhanced/{feats.ark, feats.scp, utt2spk, text_char}    mix_enhanced/{feats.ark, feats.scp, utt2spk, text_char}

keyed by the mixture's id with rows cut at the utterance's frame count, as the reference does.  The tables are written by
``kaldi_io.ArkScpWriter`` (no ``copy-feats`` pipe): float32 records, or with ``--compress`` the 8-bit records of ``copy-feats --compress=true``.

``--wav`` reads ``MixWavDataset(DATA)`` instead (``clean_wav.scp``, ``noise.scp``; the mixtures of (seed, epoch 0, item)) and additionally writes

    mix_enhanced_wav/<item>.wav      re2e_wav_istft of the enhanced mixture with the mixture's own phase, 16-bit
    metrics.json                     per item and mean: SI-SDR and SNR of the mixture, of the enhanced signal, and the SI-SDR improvement

The mixture's waveform is ``istft(mix, mix_ang)`` and the enhanced one ``istft(enhance(mix), mix_ang)``: both come out of the same kernel and are
scored by re2e_wav_sdr_sums against the clean samples over the 256 * (L // 256) samples an inverse STFT restores (the rest is zero padding).
With ``--rir_scp`` the mixtures are reverberant (csrc/reverb.hip, the draws of (seed, epoch 0, item, 1)); the reference of the scores stays the
dry signal."""
import argparse
import json
import os

import numpy as np
import torch

from .data import kaldi_io, wav_io
from .data.mix_data_loader import (WAV_HOP, collate_kaldi_device, wav_frames_of, wav_frontend_device, wav_istft_device, wav_sdr_device)

STREAMS = ('clean_enhanced', 'mix_enhanced')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m robust_e2e_gan_amd.enhance_out', description='enhanced features (and waveforms) of a data set')
    ap.add_argument('--enhance_dir', required=True, help='data directory (Kaldi tables; with --wav: clean_wav.scp, noise.scp)')
    ap.add_argument('--dict_dir', required=True, help='directory that holds train_units.txt, or the dictionary file itself')
    ap.add_argument('--resume', required=True, help='checkpoint with enhance_state_dict (relative to --works_dir when given)')
    ap.add_argument('--works_dir', default='')
    ap.add_argument('--exp_path', required=True)
    ap.add_argument('--enhance_out_dir', default='enhance_out')
    ap.add_argument('--batch_size', type=int, default=16)
    ap.add_argument('--wav', action='store_true', help='read wav files, write enhanced wavs and metrics.json as well')
    ap.add_argument('--compress', action='store_true', help='8-bit compressed records, as copy-feats --compress=true')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--noise_repeat_num', type=int, default=1)
    ap.add_argument('--rir_scp', default=None, help='with --wav: room impulse responses (one wav or .npy per line): reverberant mixtures')
    ap.add_argument('--reverb_prob', type=float, default=None, help='share of reverberant items (default 1.0 with --rir_scp)')
    ap.add_argument('--rir_max_taps', type=int, default=16000)
    ap.add_argument('--normalize_type', type=int, default=1)
    ap.add_argument('--num_utt_cmvn', type=int, default=20000)
    ap.add_argument('--feat_type', default='kaldi_magspec')
    ap.add_argument('--model_unit', default='char')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args(argv)
    if a.batch_size < 1:
        ap.error('--batch_size must be at least 1')
    return a


def dict_file_of(dict_dir):
    return dict_dir if os.path.isfile(dict_dir) else os.path.join(dict_dir, 'train_units.txt')


class FeatDir(object):
    """One output directory of the reference's script: feats.ark + feats.scp, utt2spk and text_char."""

    def __init__(self, path, compress=False):
        os.makedirs(path, exist_ok=True)
        self.path = path
        self.table = kaldi_io.ArkScpWriter(os.path.join(path, 'feats.ark'), compress)
        self.utt2spk = open(os.path.join(path, 'utt2spk'), 'w', encoding='utf-8')
        self.text = open(os.path.join(path, 'text_char'), 'w', encoding='utf-8')

    def add(self, utt, spk, rows, tokens):
        self.table.add(utt, rows)
        self.utt2spk.write(utt + ' ' + spk + '\n')
        self.text.write(utt + ' ' + ' '.join(tokens) + '\n')

    def close(self):
        self.table.close(os.path.join(self.path, 'feats.scp'))
        self.utt2spk.close()
        self.text.close()


def summarise(per_utt):
    """``{'utterances': per_utt, 'mean': ...}``: the mean of every figure over the utterances where it is finite."""
    keys = sorted({k for m in per_utt.values() for k in m})
    mean = {}
    for k in keys:
        v = [m[k] for m in per_utt.values() if k in m and np.isfinite(m[k])]
        mean[k] = float(np.mean(v)) if v else float('nan')
    return {'utterances': per_utt, 'mean': mean}


def _batches(n, size):
    return [list(range(i, min(i + size, n))) for i in range(0, n, size)]


def run(a, model=None):
    """The whole dump for parsed arguments ``a``; returns the output directory (and has written metrics.json there with ``a.wav``)."""
    from .model.enhance_model import EnhanceModel
    device = torch.device(a.device)
    path = os.path.join(a.works_dir, a.resume) if a.works_dir else a.resume
    if model is None:
        if not os.path.isfile(path):
            raise FileNotFoundError('no checkpoint found at %s' % path)
        model = EnhanceModel.load_model(path, 'enhance_state_dict')
    model = model.to(device).eval()
    if a.wav:
        from .data.wav_dataset import MixWavDataset
        ds = MixWavDataset(a, a.enhance_dir, dict_file_of(a.dict_dir))
        ds.set_epoch(0)
    else:
        from .data.kaldi_dataset import MixKaldiDataset
        ds = MixKaldiDataset(a, a.enhance_dir, dict_file_of(a.dict_dir), raw=True)
    cmvn = torch.from_numpy(np.asarray(ds.cmvn, dtype=np.float32)) if ds.cmvn is not None else None
    out_dir = os.path.join(a.exp_path, a.enhance_out_dir)
    dirs = {s: FeatDir(os.path.join(out_dir, s), a.compress) for s in STREAMS}
    wav_dir = os.path.join(out_dir, 'mix_enhanced_wav')
    if a.wav:
        os.makedirs(wav_dir, exist_ok=True)
    per_utt = {}
    with torch.no_grad():
        for idx in _batches(len(ds), a.batch_size):
            items = [ds[i] for i in idx]
            if a.wav:
                speech = [it[2] for it in items]
                o = wav_frontend_device(speech, device, [(it[3], it[4], it[5]) for it in items], cmvn,
                                        ('clean', 'clean_log', 'mix', 'mix_log', 'mix_ang'), reverb=[it[7] for it in items] if ds.rir_paths else None)
                utts, spks, targets = [it[0] for it in items], [it[1] for it in items], [it[6] for it in items]
                sizes = [wav_frames_of(s.shape[0]) for s in speech]
                clean, clean_log, mix, mix_log = o['clean'], o['clean_log'], o['mix'], o['mix_log']
            else:
                utts, spks, clean, clean_log, mix, mix_log, _, flat, isz, tsz = collate_kaldi_device(items, device, cmvn)
                sizes, targets, pos = isz.tolist(), [], 0
                for n in tsz.tolist():
                    targets.append(flat[pos:pos + n].tolist())
                    pos += n
            st = torch.IntTensor(sizes)
            clean_out = model(clean, clean_log, st)
            mix_out = model(mix, mix_log, st)
            c_host, m_host = clean_out.cpu().numpy(), mix_out.cpu().numpy()
            for x, utt in enumerate(utts):
                tokens = [ds.char_list[int(t)] for t in targets[x]]
                dirs['clean_enhanced'].add(utt, spks[x], c_host[x, :sizes[x]], tokens)
                dirs['mix_enhanced'].add(utt, spks[x], m_host[x, :sizes[x]], tokens)
            if a.wav:
                lens = [int(s.shape[0]) for s in speech]
                kept = [WAV_HOP * (n // WAV_HOP) for n in lens]          # what an inverse STFT restores: the rest is zero padding
                clip = torch.zeros(1, dtype=torch.int32, device=device)
                mix_blob, offs = wav_istft_device(mix, o['mix_ang'], lens, device, int16=False, blob=True)
                enh_blob, _ = wav_istft_device(mix_out, o['mix_ang'], lens, device, int16=False, blob=True)
                enh_pcm = wav_istft_device(mix_out, o['mix_ang'], lens, device, int16=True, clip_count=clip)
                m_mix = wav_sdr_device(speech, mix_blob, offs, kept)
                m_enh = wav_sdr_device(speech, enh_blob, offs, kept)
                for x, utt in enumerate(utts):
                    wav_io.write_wav(os.path.join(wav_dir, utt + '.wav'), enh_pcm[x])
                    per_utt[utt] = {'si_sdr_mix': m_mix[x]['si_sdr'], 'si_sdr_enhanced': m_enh[x]['si_sdr'],
                                    'si_sdr_improvement': m_enh[x]['si_sdr'] - m_mix[x]['si_sdr'],
                                    'snr_mix': m_mix[x]['snr'], 'snr_enhanced': m_enh[x]['snr']}
                if int(clip.item()):
                    print('%d enhanced samples saturated at 16 bits in this batch' % int(clip.item()))
    for d in dirs.values():
        d.close()
    if a.wav:
        report = summarise(per_utt)
        with open(os.path.join(out_dir, 'metrics.json'), 'w') as f:
            json.dump(report, f, indent=1, sort_keys=True)
        print('SI-SDR over %d utterances: mixture %.2f dB, enhanced %.2f dB, improvement %.2f dB' % (
            len(per_utt), report['mean']['si_sdr_mix'], report['mean']['si_sdr_enhanced'], report['mean']['si_sdr_improvement']))
    print('finish')
    return out_dir


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
