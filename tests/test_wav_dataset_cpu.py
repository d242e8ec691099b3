"""data/wav_io.py and data/wav_dataset.py on the CPU: wav files round-trip, anything but 16-bit mono 16 kHz PCM is refused by name, item ids
map to their utterance and speaker, the draws are a function of (seed, epoch, index), the segment start stays inside the reference's range
and the length bins follow the header frame counts."""
import argparse
import os
import wave

import numpy as np
import pytest

import refs64_wav as R
from robust_e2e_gan_amd.data import wav_io
from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset, segment_start_range

LENS = {'uttA': 1279, 'uttB': 257, 'uttC': 2303, 'uttD': 40000}
NOISE = {'n1': 100, 'n2': 5000}


def _write(path, data, width=2, channels=1, rate=16000):
    w = wave.open(str(path), 'wb')
    w.setnchannels(channels)
    w.setsampwidth(width)
    w.setframerate(rate)
    w.writeframes(data)
    w.close()


@pytest.fixture
def corpus(tmp_path):
    rng = np.random.RandomState(3)
    sig = {}
    for name, n in list(LENS.items()) + list(NOISE.items()):
        sig[name] = rng.randint(-20000, 20000, n).astype(np.int16)
        wav_io.write_wav(str(tmp_path / (name + '.wav')), sig[name])
    (tmp_path / 'clean_wav.scp').write_text(''.join('%s %s\n' % (u, tmp_path / (u + '.wav')) for u in LENS))
    (tmp_path / 'noise.scp').write_text(''.join('%s\n' % (tmp_path / (n + '.wav')) for n in NOISE))
    (tmp_path / 'utt2spk').write_text(''.join('%s spk%s\n' % (u, u[-1]) for u in LENS))
    (tmp_path / 'text_char').write_text(''.join('%s a b %s\n' % (u, 'c' * (i + 1)) for i, u in enumerate(LENS)))
    (tmp_path / 'dict').write_text('a 1\nb 2\nc 3\n')
    args = argparse.Namespace(noise_repeat_num=3, seed=11, normalize_type=0, model_unit='char')
    return tmp_path, sig, MixWavDataset(args, str(tmp_path), str(tmp_path / 'dict'))


def test_read_wav_round_trips(tmp_path):
    for n in (1, 257, 4001):
        x = np.random.RandomState(n).randint(-32768, 32768, n).astype(np.int16)
        p = str(tmp_path / ('x%d.wav' % n))
        wav_io.write_wav(p, x)
        got = wav_io.read_wav(p)
        assert got.dtype == np.int16 and np.array_equal(got, x) and wav_io.wav_frames(p) == n


def test_read_wav_refuses_other_formats(tmp_path):
    bad = {'eight_bit': dict(width=1), 'stereo': dict(channels=2), 'eight_khz': dict(rate=8000)}
    for name, kw in bad.items():
        p = tmp_path / (name + '.wav')
        _write(p, b'\x00' * 64, **kw)
        for fn in (wav_io.read_wav, wav_io.wav_frames):
            with pytest.raises(wav_io.WavError) as e:
                fn(str(p))
            assert name + '.wav' in str(e.value)
    p = tmp_path / 'text.wav'
    p.write_text('not a wav file at all')
    with pytest.raises(wav_io.WavError) as e:
        wav_io.read_wav(str(p))
    assert 'text.wav' in str(e.value)


def test_items_map_to_utterance_speaker_and_target(corpus):
    _, sig, ds = corpus
    utts = list(LENS)
    assert len(ds) == 3 * len(utts)
    for i in range(len(ds)):
        item, spk, speech, noise, s0, db, target = ds[i]
        k, u = divmod(i, len(utts))
        assert item == '%s__mix%d' % (utts[u], k) and spk == 'spk' + utts[u][-1]
        assert speech.dtype == np.int16 and np.array_equal(speech, sig[utts[u]])
        ni = ds.draw(i)[0]
        assert np.array_equal(noise, sig[list(NOISE)[ni]]) and noise is ds.noise(ni)          # one array per file: uploaded once per batch
        assert 0 <= s0 < noise.shape[0] and 0.0 <= db < 20.0
        assert target == [1, 2] + [3] * (u + 1)                                                 # '<blank>' a b c '<eos>'


def test_draws_are_a_function_of_seed_epoch_and_index(corpus):
    tmp, _, ds = corpus
    first = [ds.draw(i) for i in range(len(ds))]
    assert first == [ds.draw(i) for i in range(len(ds))]
    again = MixWavDataset(argparse.Namespace(noise_repeat_num=3, seed=11, normalize_type=0), str(tmp), str(tmp / 'dict'))
    assert first == [again.draw(i) for i in range(len(again))]
    ds.set_epoch(1)
    second = [ds.draw(i) for i in range(len(ds))]
    assert all(a != b for a, b in zip(first, second))                     # fresh mixtures every epoch (the dB alone is a continuous draw)
    assert second == [ds.draw(i, epoch=1) for i in range(len(ds))]
    ds.set_epoch(0)
    assert first == [ds.draw(i) for i in range(len(ds))]
    other = MixWavDataset(argparse.Namespace(noise_repeat_num=3, seed=12, normalize_type=0), str(tmp), str(tmp / 'dict'))
    assert all(a != b for a, b in zip(first, [other.draw(i) for i in range(len(other))]))
    assert len({d[0] for e in range(8) for d in [ds.draw(0, epoch=e)]}) == 2          # both noise files are drawn


def test_segment_start_stays_inside_the_reference_range(corpus):
    _, sig, ds = corpus
    for N in (100, 700, 5000):
        for L in (257, 1279, 2303, 5000, 40000):
            assert segment_start_range(N, L) == R.s0_range(N, L)
    utts, noises = list(LENS), list(NOISE)
    for e in range(20):
        for i in range(len(ds)):
            ni, start, _ = ds.draw(i, epoch=e)
            L, N = LENS[utts[i % len(utts)]], NOISE[noises[ni]]
            assert 0 <= start < R.s0_range(N, L)
            # the segment the item hands to the kernel is the reference's tile-then-slice
            if e == 0:
                assert np.array_equal(R.noise_segment(sig[noises[ni]], start % N, L), R.noise_segment_tiled(sig[noises[ni]], start, L))


def test_length_bins_follow_the_header_frame_counts(corpus):
    _, _, ds = corpus
    frames = [1 + LENS[u] // 256 for u in LENS] * 3
    _, edges = np.histogram(frames, bins='auto')
    want = {}
    for i, b in enumerate(np.digitize(frames, bins=edges)):
        want.setdefault(int(b), []).append(i)
    assert dict(ds.bins_to_samples) == want
    assert sorted(i for v in ds.bins_to_samples.values() for i in v) == list(range(len(ds)))
    from robust_e2e_gan_amd.data.mix_data_loader import BucketingSampler
    batches = list(BucketingSampler(ds.bins_to_samples, batch_size=4))
    assert sorted(i for b in batches for i in b) == list(range(len(ds)))


def test_short_utterance_is_refused_by_name(tmp_path):
    wav_io.write_wav(str(tmp_path / 'tiny.wav'), np.zeros(256, np.int16))
    wav_io.write_wav(str(tmp_path / 'n.wav'), np.ones(300, np.int16))
    (tmp_path / 'clean_wav.scp').write_text('tiny %s\n' % (tmp_path / 'tiny.wav'))
    (tmp_path / 'noise.scp').write_text('%s\n' % (tmp_path / 'n.wav'))
    with pytest.raises(wav_io.WavError) as e:
        MixWavDataset(argparse.Namespace(normalize_type=0), str(tmp_path), str(tmp_path / 'dict'))
    assert 'tiny' in str(e.value)
