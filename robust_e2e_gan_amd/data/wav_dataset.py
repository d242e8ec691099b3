"""Waveform dataset of the joint / enhancement trainers: the inputs of the reference's offline data/prepare_feats.py (``clean_wav.scp``,
``noise.scp``) read directly, with the noise mixed in and the STFT taken on the device by ``mix_data_loader.collate_wav_device``
(csrc/stft.hip) -- no librosa, no Kaldi binaries, no stored spectra.

Directory layout: ``clean_wav.scp`` (``utt path``), ``noise.scp`` (one path per line; a leading id column is accepted), ``utt2spk``,
``text_char`` | ``text_word`` and a dictionary file.  Items are ``<utt>__mix<k>``, k < ``noise_repeat_num``, as prepare_feats names its
mixtures.  Where prepare_feats draws the noise file, the segment start and the SNR ~ U(0, 20) dB ONCE, offline, here they come from a
generator seeded by (seed, epoch, index): ``set_epoch`` gives fresh mixtures every epoch, and the same triple gives the same mixture.
The segment start follows the reference's rule (prepare_feats.py:45-50) on the noise file repeated until it covers the speech.  The
reference draws again when the noise segment has zero power; here such a mixture is the clean signal and is counted on the device
(re2e_wav_mix_scale), which the loader logs one batch late.

``__getitem__`` returns ``(item id, speaker, speech int16, noise int16, s0, dB, target list)``.

Reverberant mixtures (the reference's Make_Noisy_Wave, data/audioparse.py:254-303): with ``args.rir_scp`` (one impulse response per line; a
leading id column is accepted), an item is reverberant with probability ``args.reverb_prob`` (default 1.0), and the speech and the noise
then get one impulse response each, drawn independently from a generator of their own seeded by (seed, epoch, index, 1) -- the mixture
draws above are the numbers they are without it.  ``__getitem__`` then appends an eighth element ``(h_speech | None, h_noise | None)``
(fp32 taps, ``wav_io.read_rir``); the device convolves (csrc/reverb.hip), the clean stream stays the dry signal.

Speed perturbation (Kaldi's 3-way ``sox speed 0.9 / 1.0 / 1.1``; no reference counterpart): with ``args.speed_perturb``, a comma list of
decimal strings such as ``'0.9,1.0,1.1'``, every item draws one of them uniformly from a generator of its own seeded by
(seed, epoch, index, 2) -- the mixture and RIR draws keep their streams -- and the device resamples the speech by the rational ratio
(csrc/resample.hip, ``mix_data_loader.speed_ratio``) BEFORE it is reverberated and mixed; the perturbed dry signal is the enhancer's target,
the noise is never perturbed.  The mixture is drawn for the perturbed length L' = ceil(L up / down): the reference's segment-start rule
applies to the speech that is actually mixed.  ``__getitem__`` then appends a ninth element ``None | (up, down)`` behind the RIR pair, which
is ``(None, None)`` when the data set has no impulse responses; the speech array itself stays the file's samples.  The length buckets of
``BucketingSampler`` stay on the NOMINAL lengths: a speed changes a length by a tenth, a bucket spans more, and the draw changes every epoch."""
import os
from collections import defaultdict

import numpy as np
import torch

from ..lib import call
from . import wav_io
from .kaldi_dataset import _read_table, read_dictionary, read_targets
from .mix_data_loader import WAV_BINS, resampled_len, speed_ratio, wav_frames_of, wav_frontend_device


def segment_start_range(noise_len, speech_len):
    """Exclusive upper end of the reference's draw of the segment start in the tiled noise: ``randint(0, elen - 1)`` when
    ``elen = tiled - speech_len - 1 > 1``, else 0."""
    tiled = noise_len * max(1, -(-speech_len // noise_len))
    elen = tiled - speech_len - 1
    return elen if elen > 1 else 1


def draw_mixture(seed, epoch, index, noise_lens, speech_len):
    """``(noise file index, segment start in the tiled noise, dB ~ U(0, 20))`` from a generator seeded by (seed, epoch, index)."""
    rng = np.random.default_rng([int(seed), int(epoch), int(index)])
    ni = int(rng.integers(len(noise_lens)))
    start = int(rng.integers(segment_start_range(noise_lens[ni], speech_len)))
    return ni, start, float(rng.uniform(0.0, 20.0))


def draw_reverb(seed, epoch, index, n_rirs, prob):
    """``(speech RIR index | None, noise RIR index | None)`` from a generator seeded by (seed, epoch, index, 1), a stream apart from
    ``draw_mixture``'s: with probability ``prob`` the item is reverberant, and both indices are then drawn independently."""
    rng = np.random.default_rng([int(seed), int(epoch), int(index), 1])
    if n_rirs < 1 or not rng.random() < prob:
        return None, None
    return int(rng.integers(n_rirs)), int(rng.integers(n_rirs))


def draw_speed(seed, epoch, index, n):
    """Index of one of ``n`` speeds, uniform, from a generator seeded by (seed, epoch, index, 2), a stream apart from ``draw_mixture``'s and
    ``draw_reverb``'s."""
    rng = np.random.default_rng([int(seed), int(epoch), int(index), 2])
    return int(rng.integers(n))


class MixWavDataset(torch.utils.data.Dataset):
    def __init__(self, args, data_dir, dict_file):
        self.args = args
        self.clean = _read_table(os.path.join(data_dir, 'clean_wav.scp'))
        self.clean = [(u, p.strip()) for u, p in self.clean]
        with open(os.path.join(data_dir, 'noise.scp'), encoding='utf-8') as f:
            self.noise_paths = [line.split()[-1] for line in f if line.strip()]
        if not self.clean or not self.noise_paths:
            raise ValueError('%s: clean_wav.scp and noise.scp must list at least one file each' % data_dir)
        self.repeat = max(1, int(getattr(args, 'noise_repeat_num', 1)))
        self.seed = int(getattr(args, 'seed', 0))
        self.epoch = 0
        self.samples = [wav_io.wav_frames(p) for _, p in self.clean]              # header only
        short = [u for (u, _), n in zip(self.clean, self.samples) if n < WAV_BINS]
        if short:
            raise wav_io.WavError('%s: shorter than %d samples (the STFT pads by reflection)' % (short[0], WAV_BINS))
        self.noise_len = [wav_io.wav_frames(p) for p in self.noise_paths]
        self._noise = {}
        self.rir_paths = []
        rir_scp = getattr(args, 'rir_scp', None)
        if rir_scp:
            with open(rir_scp, encoding='utf-8') as f:
                self.rir_paths = [line.split()[-1] for line in f if line.strip()]
            if not self.rir_paths:
                raise ValueError('%s lists no impulse response' % rir_scp)
        prob = getattr(args, 'reverb_prob', None)
        self.reverb_prob = 1.0 if prob is None else float(prob)
        self.rir_max_taps = int(getattr(args, 'rir_max_taps', None) or 16000)
        self.speeds = []                                                           # None | (up, down) per configured speed
        speed_perturb = getattr(args, 'speed_perturb', None)
        if speed_perturb:
            self.speeds = [speed_ratio(t) for t in str(speed_perturb).split(',') if t.strip()]
            if not self.speeds:
                raise ValueError('speed_perturb %r lists no speed' % (speed_perturb,))
            short = [u for (u, _), n in zip(self.clean, self.samples) if min(resampled_len(n, r) for r in self.speeds) < WAV_BINS]
            if short:
                raise wav_io.WavError('%s: shorter than %d samples at its fastest speed (the STFT pads by reflection)' % (short[0], WAV_BINS))
        self.feat_size = WAV_BINS
        lengths = [wav_frames_of(self.samples[i % len(self.clean)]) for i in range(len(self))]
        _, edges = np.histogram(lengths, bins='auto')                              # length buckets for BucketingSampler, as MixKaldiDataset
        self.bins_to_samples = defaultdict(list)
        for i, b in enumerate(np.digitize(lengths, bins=edges)):
            self.bins_to_samples[int(b)].append(i)
        self.utt2spk = dict(_read_table(os.path.join(data_dir, 'utt2spk')))
        self.char_list = read_dictionary(dict_file)
        self.num_classes = len(self.char_list)
        unit = getattr(args, 'model_unit', 'char')
        self.targets, self.labeldist = read_targets(os.path.join(data_dir, 'text_char' if unit == 'char' else 'text_word'), self.char_list, unit)
        self.num_utt_cmvn = getattr(args, 'num_utt_cmvn', 20000)
        self.cmvn = self._load_cmvn() if getattr(args, 'normalize_type', 1) == 1 else None

    def __len__(self):
        return len(self.clean) * self.repeat

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    # ---- items ----------------------------------------------------------------------------------------------
    def item_id(self, index):
        """``(<utt>__mix<k>, utt index)``: repeat k covers the whole list before k + 1 starts, as prepare_feats writes them."""
        k, u = divmod(index, len(self.clean))
        return '%s__mix%d' % (self.clean[u][0], k), u

    def draw(self, index, epoch=None):
        """``(noise file index, segment start in the tiled noise, dB)`` of item ``index`` in ``epoch`` (default: the current one)."""
        return draw_mixture(self.seed, self.epoch if epoch is None else epoch, index, self.noise_len,
                            resampled_len(self.samples[self.item_id(index)[1]], self.draw_speed(index, epoch)))

    def draw_speed(self, index, epoch=None):
        """``None | (up, down)`` of item ``index`` in ``epoch`` (default: the current one); None without ``speed_perturb`` and at speed 1."""
        if not self.speeds:
            return None
        return self.speeds[draw_speed(self.seed, self.epoch if epoch is None else epoch, index, len(self.speeds))]

    def noise(self, ni):
        """Noise file ``ni``, read once and kept: items that share it hand the SAME array to the collate, which uploads it once per batch."""
        a = self._noise.get(ni)
        if a is None:
            a = self._noise[ni] = wav_io.read_wav(self.noise_paths[ni])
        return a

    def draw_rirs(self, index, epoch=None):
        """``(speech RIR index | None, noise RIR index | None)`` of item ``index`` in ``epoch`` (default: the current one)."""
        return draw_reverb(self.seed, self.epoch if epoch is None else epoch, index, len(self.rir_paths), self.reverb_prob)

    def rir(self, ri):
        return None if ri is None else wav_io.read_rir(self.rir_paths[ri], self.rir_max_taps)

    def __getitem__(self, index):
        item, u = self.item_id(index)
        utt, path = self.clean[u]
        ni, start, db = self.draw(index)
        out = (item, self.utt2spk[utt], wav_io.read_wav(path), self.noise(ni), start % self.noise_len[ni], db, list(self.targets.get(utt)))
        if self.rir_paths:
            rs, rn = self.draw_rirs(index)
            out += ((self.rir(rs), self.rir(rn)),)
        if not self.speeds:
            return out
        return (out if self.rir_paths else out + ((None, None),)) + (self.draw_speed(index),)

    # ---- CMVN -----------------------------------------------------------------------------------------------
    def compute_cmvn(self, device='cuda', batch=16):
        """[-mean; 1/sqrt(var)] of 10*log10(max(|M|, 1e-7)) over ``num_utt_cmvn`` random mixtures, (2, 257) as MixKaldiDataset's -- the
        spectra and their per-bin sums are taken on the device (re2e_wav_stft, re2e_cmvn_stats), accumulated in float64 on the host."""
        n = min(len(self), self.num_utt_cmvn)
        order = np.random.permutation(len(self))[:n]
        s, sq, frames = np.zeros(WAV_BINS), np.zeros(WAV_BINS), 0
        for i in range(0, n, batch):
            items = [self[int(j)] for j in order[i:i + batch]]
            log = wav_frontend_device([it[2] for it in items], device, [(it[3], it[4], it[5]) for it in items], None, ('mix_log',),
                                      reverb=[it[7] for it in items] if self.rir_paths else None,
                                      speed=[it[8] for it in items] if self.speeds else None)['mix_log']
            lens = [wav_frames_of(resampled_len(it[2].shape[0], it[8] if self.speeds else None)) for it in items]
            ld = torch.tensor(lens, dtype=torch.int32, device=device)
            bs, bq = torch.empty(WAV_BINS, device=device), torch.empty(WAV_BINS, device=device)
            call('re2e_cmvn_stats', log.data_ptr(), ld.data_ptr(), len(items), log.shape[1], WAV_BINS, bs.data_ptr(), bq.data_ptr())
            s += bs.double().cpu().numpy()
            sq += bq.double().cpu().numpy()
            frames += sum(lens)
        mean = s / frames
        var = sq / frames - np.square(mean)
        return np.stack([-mean, 1 / np.sqrt(var)], 0).astype(np.float32)

    def _load_cmvn(self):
        exp = getattr(self.args, 'exp_path', None)
        path = os.path.join(exp, 'cmvn.npy') if exp else None
        if path and os.path.exists(path):
            cm = np.load(path)
            if cm.shape[1] == self.feat_size:
                return cm
        cm = self.compute_cmvn()
        if path:
            os.makedirs(exp, exist_ok=True)
            np.save(path, cm)
        return cm
