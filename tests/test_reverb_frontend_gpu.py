"""Reverberant mixtures end to end on the GPU (csrc/stft.hip re2e_wav_stft_rev, mix_data_loader.wav_frontend_device(reverb=...),
data/wav_dataset.py with ``rir_scp``, tools/prepare_feats.py --rir_scp, enhance_out --wav --rir_scp):

  * re2e_wav_stft_rev against the float64 restatement (tests/refs64_reverb.py) at refs64_wav's own bars, on its LENGTHS, with impulse
    responses of 1, 33 and 300 taps.  The kernel's inputs are the 16-bit reverberant signals of the restatement (the convolution is held to
    its own bound in tests/test_reverb_kernels_gpu.py: a sample that rounds the other way there moves a bin by up to one unit, which is the
    size of the magnitude bar itself, so the two kernels are not judged through each other)
  * h = [1.0] on both streams agrees with re2e_wav_stft within those bars -- NOT bit for bit: there M = C + gN is put together from two
    spectra taken apart by conjugate symmetry, here M is the spectrum of the imaginary half itself
  * mix_off == NULL is re2e_wav_stft bit for bit
  * the two input paths agree bit for bit with reverberation as they do without it, also through DevicePrefetcher; reverb_prob 0 gives the
    batch of the data set without impulse responses; the front end equals the restatement's 16-bit reverberant signals within one unit
  * enhance_out --wav --rir_scp runs on a tiny set and writes finite figures.
GPU only; every test takes a few seconds."""
import argparse
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import refs64_reverb as R
import refs64_wav as W
from test_wav_frontend_gpu import _corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('clean', 'clean_log', 'mix', 'mix_log', 'cos', 'clean_ang', 'mix_ang')


def _longs(v):
    return (ctypes.c_long * len(v))(*[int(x) for x in v])


def _lib():
    from robust_e2e_gan_amd import lib
    assert lib.query('re2e_device_ok') == 1
    return lib


@functools.lru_cache(maxsize=None)
def _refs(name):
    return R.mix_case_refs(name), R.mix_case_refs(name, np.float32)


def _place(arrays):
    """One int16 device blob, every signal at an odd sample, 0x7FFF fillers between."""
    parts, offs, pos = [], [], 0
    for a in arrays:
        pad = 1 if pos % 2 == 0 else 2
        parts.append(np.full(pad, 0x7FFF, np.int16))
        pos += pad
        offs.append(pos)
        parts.append(a)
        pos += a.shape[0]
    parts.append(np.full(3, 0x7FFF, np.int16))
    return torch.from_numpy(np.concatenate(parts)).to(DEV), offs


def _stft_rev(lib, speech, mix_speech, noises, s0, db, cm, rev=True, plain=False):
    """re2e_wav_mix_scale (on the mixture's speech) + re2e_wav_stft_rev (or re2e_wav_stft with ``plain``) -> {name: CPU tensor}, 'scale'."""
    B = len(speech)
    lens = [s.shape[0] for s in speech]
    Tmax = max(W.n_frames(L) for L in lens) + 1
    blob, offs = _place(list(speech) + list(mix_speech) + list(noises))
    soff, moff, noff = offs[:B], offs[B:2 * B], offs[2 * B:]
    out = {k: torch.full((B, Tmax, W.NBIN), float('nan'), device=DEV) for k in OUTS}
    scale = torch.full((B,), float('nan'), device=DEV)
    cm_d = torch.from_numpy(cm).to(DEV)
    nidx = (_longs(noff), _longs([n.shape[0] for n in noises]), _longs(s0))
    lib.call('re2e_wav_mix_scale', blob.data_ptr(), _longs(moff), _longs(lens), *nidx, (ctypes.c_float * B)(*db), B, scale.data_ptr(), None)
    ptrs = [out[k].data_ptr() for k in OUTS]
    if plain:
        lib.call('re2e_wav_stft', blob.data_ptr(), _longs(soff), _longs(lens), *nidx, scale.data_ptr(), B, Tmax, *ptrs, cm_d.data_ptr())
    else:
        lib.call('re2e_wav_stft_rev', blob.data_ptr(), _longs(soff), _longs(moff) if rev else None, _longs(lens), *nidx, scale.data_ptr(), B, Tmax,
                 *ptrs, cm_d.data_ptr())
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res['scale'] = scale.cpu()
    return res


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize('name', sorted(R.MIX_CASES))
def test_stft_rev_against_float64(name):
    lib = _lib()
    speech, nz, cm, hs, hn = R.mix_case_signals(name)
    lens, N, s0, db, _, _ = R.MIX_CASES[name]
    assert set(lens) <= set(W.LENGTHS)
    r64, r32 = _refs(name)
    run = lambda: _stft_rev(lib, speech, [r['rs'] for r in r64], [r['rn'] for r in r64], s0, db, cm)
    res, again = run(), run()
    assert _same(res, again), 'the second run differs from the first'
    for b, L in enumerate(lens):
        T = W.n_frames(L)
        for k in OUTS:
            assert torch.isfinite(res[k][b]).all() and (res[k][b, T:] == 0).all(), (name, k, b)
        got = {k: res[k][b, :T].numpy() for k in OUTS}
        got['g'] = float(res['scale'][b])
        cpu = {k: r32[b][k] for k in got}
        hd, cd = W.distances(got, r64[b], cm), W.distances(cpu, r64[b], cm)
        print('ERR %-11s utt %d (L %4d)  %s' % (name, b, L, '  '.join('%s hip %.2e fp32-cpu %.2e' % (k, hd[k], cd[k]) for k in sorted(hd))))
        assert W.violations(cpu, r64[b], cm, frac=0.25) == [], (name, b)
        assert W.violations(got, r64[b], cm) == [], (name, b)


def test_unit_impulse_agrees_with_the_plain_front_end_and_null_mix_off_is_it():
    lib = _lib()
    name = 'wrap700'
    speech, nz, cm, _, _ = R.mix_case_signals(name)
    lens, N, s0, db, _, _ = R.MIX_CASES[name]
    B = len(speech)
    plain = _stft_rev(lib, speech, speech, [nz] * B, s0, db, cm, plain=True)
    null = _stft_rev(lib, speech, speech, [nz] * B, s0, db, cm, rev=False)
    assert _same(plain, null), 'mix_off == NULL is not re2e_wav_stft bit for bit'
    rev = _stft_rev(lib, speech, speech, [nz] * B, s0, db, cm)           # the mixture's speech stream IS the dry one: h = [1.0]
    assert not _same(plain, rev)                                       # M is formed differently: equal within the bars, not in every bit
    # (the clean outputs are not bit-equal either: C comes out of the same complex transform, whose two halves leak into each other at
    # fp32 rounding level, and the imaginary half differs; g is the same call on the same samples)
    assert torch.equal(plain['scale'].view(torch.int32), rev['scale'].view(torch.int32))
    for b, L in enumerate(lens):
        T = W.n_frames(L)
        ref = W.features(speech[b], nz, s0[b], db[b], cm)
        for res in (plain, rev):
            got = {k: res[k][b, :T].numpy() for k in OUTS}
            assert W.violations(got, ref, cm) == [], b


# ---- data set, collate, tools -------------------------------------------------------------------------------------------------------------
def _rirs(tmp_path):
    from robust_e2e_gan_amd.data import wav_io
    np.save(str(tmp_path / 'r0.npy'), np.concatenate([np.zeros(5), R.rir(300, 1).astype(np.float64)]))
    np.save(str(tmp_path / 'r1.npy'), R.rir(33, 2))
    w = np.zeros(600, np.int16)
    w[2] = 20000
    w[3:600] = np.round(4000 * np.random.RandomState(4).randn(597) * np.exp(-np.arange(597) / 120.0))
    wav_io.write_wav(str(tmp_path / 'r2.wav'), w)
    (tmp_path / 'rir.scp').write_text('room0 %s\nroom1 %s\n%s\n' % (tmp_path / 'r0.npy', tmp_path / 'r1.npy', tmp_path / 'r2.wav'))
    return str(tmp_path / 'rir.scp')


def _dataset(tmp_path, seed=7, repeat=1, **extra):
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    return MixWavDataset(argparse.Namespace(noise_repeat_num=repeat, seed=seed, normalize_type=0, **extra), str(tmp_path), str(tmp_path / 'dict'))


def _equal_batches(a, b, streams=(2, 3, 4, 5, 6)):
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[7], b[7]) and torch.equal(a[8], b[8]) and torch.equal(a[9], b[9])
    for k in streams:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), 'stream %d differs' % k


def test_kaldi_records_and_wav_input_agree_with_reverberation(tmp_path):
    from robust_e2e_gan_amd.data.kaldi_dataset import MixKaldiDataset
    from robust_e2e_gan_amd.data.mix_data_loader import collate_kaldi_device, collate_wav_device
    from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import prepare_feats
    finally:
        sys.path.pop(0)
    _lib()
    _, cmvn = _corpus(tmp_path)
    scp = _rirs(tmp_path)
    ds = _dataset(tmp_path, rir_scp=scp, rir_max_taps=400)
    items = [ds[i] for i in range(len(ds))]
    assert len(items) == 3 and all(len(it) == 8 and it[7][0] is not None and it[7][1] is not None for it in items)
    assert 2 <= len({id(h) for it in items for h in it[7]}) <= 3                # one array per file, shared by the items that drew it
    # (one mixture per utterance, as tests/test_wav_frontend_gpu.py: the clean table is written from the first mixture's launch, and the
    # dry spectrum of a later mixture of the same utterance differs from it in the last bit -- the transform's two halves leak into each
    # other at rounding level, with or without reverberation)
    prepare_feats.prepare(str(tmp_path), str(tmp_path / 'feats'), 1, compress=False, seed=7, device=DEV, batch=2, rir_scp=scp, rir_max_taps=400)
    want = ('clean', 'mix', 'mix_log')
    wav = collate_wav_device(items, DEV, cmvn, want=want)
    kd = MixKaldiDataset(argparse.Namespace(feat_type='kaldi_magspec', normalize_type=0), str(tmp_path), str(tmp_path / 'dict'), raw=True)
    kal = collate_kaldi_device([kd[i] for i in range(len(kd))], DEV, cmvn)
    torch.cuda.synchronize()
    assert sorted(wav[0]) == sorted(kal[0]) and len(wav[0]) == 3
    order = [kal[0].index(u) for u in wav[0]]                                   # equal lengths may sort differently: compare by item
    for k, name in ((2, 'clean'), (4, 'mix'), (5, 'mix_log')):
        assert torch.equal(wav[k].view(torch.int32), kal[k][order].view(torch.int32)), '%s: the two input paths differ' % name
    # the mixtures are reverberant, the clean stream is dry
    plain = collate_wav_device([it[:7] for it in items], DEV, cmvn, want=want)
    top = plain[2].max().item()          # (each within BAR_MAG of the same float64 spectrum; the mixtures differ by whole reflections)
    assert (plain[2] - wav[2]).abs().max().item() <= 2 * W.BAR_MAG * top and (plain[4] - wav[4]).abs().max().item() >= 1e-2 * top
    # against the restatement (Make_Noisy_Wave's order, the SNR after reverberation).  The device's 16-bit reverberant signals are within
    # one unit of float64's, so in the worst case every sample is one unit off: a bin moves by at most the window's sum (276.5) times
    # (1 + g), and g itself by at most 1e-3 relative (a power sum of L samples of rms r moves by at most 2 / r + 1 / r^2 relative; r is
    # 5000 for the speech and 1500 for the noise, half of each on the root), which moves a bin by at most 1e-3 of the max.  The restatement's
    # own mistakes are told apart at the kernels' bars (tests/test_refs64_reverb_cpu.py); this one guards the plumbing between them.
    for b, utt in enumerate(wav[0]):
        it = items[[x[0] for x in items].index(utt)]
        ref = R.features_rev(it[2], it[3], it[4], it[5], it[7][0], it[7][1])
        T = W.n_frames(it[2].shape[0])
        d = np.abs(wav[4][b, :T].cpu().numpy().astype(np.float64) - ref['mix']).max()
        bar = (W.BAR_MAG + 1e-3) * ref['mix'].max() + 276.5 * (1 + float(ref['g']))
        print('reverberant front end against float64, %s: %.3e of the max (worst-case bar %.3e)' % (utt, d / ref['mix'].max(), bar / ref['mix'].max()))
        assert d <= bar, (utt, d, bar)
    # through the prefetcher: the same tensors
    batches = [items[:2], items[2:]]
    direct = [collate_wav_device(b, DEV, cmvn, want=want) for b in batches]
    torch.cuda.synchronize()
    n = 0
    for got, ref in zip(DevicePrefetcher(batches, DEV, collate=lambda b, d, p: collate_wav_device(b, d, cmvn, want=want, pool=p)), direct):
        torch.cuda.synchronize()
        _equal_batches(got, ref)
        n += 1
    assert n == 2


def test_reverb_prob_zero_is_the_data_set_without_impulse_responses(tmp_path):
    from robust_e2e_gan_amd.data.mix_data_loader import collate_wav_device
    _lib()
    _, cmvn = _corpus(tmp_path)
    scp = _rirs(tmp_path)
    never, none = _dataset(tmp_path, rir_scp=scp, reverb_prob=0.0), _dataset(tmp_path)
    a = collate_wav_device([never[i] for i in range(len(never))], DEV, cmvn, want=('clean', 'clean_log', 'mix', 'mix_log', 'cos'))
    b = collate_wav_device([none[i] for i in range(len(none))], DEV, cmvn, want=('clean', 'clean_log', 'mix', 'mix_log', 'cos'))
    torch.cuda.synchronize()
    assert all(len(never[i]) == 8 and len(none[i]) == 7 for i in range(len(none)))
    _equal_batches(a, b)


def test_enhance_out_wav_with_reverberation(tmp_path):
    from robust_e2e_gan_amd import enhance_out as E
    from robust_e2e_gan_amd.data import wav_io
    from test_enhance_wav_gpu import _args, _checkpoint, _model
    _corpus(tmp_path)
    scp = _rirs(tmp_path)
    model, opt = _model()
    ckpt = _checkpoint(tmp_path, model, opt)
    E.main(_args(tmp_path, ckpt, '--wav', '--rir_scp', scp, '--rir_max_taps', '400'))
    E.main(_args(tmp_path, ckpt, '--wav', '--enhance_out_dir', 'dry'))
    out = tmp_path / 'exp' / 'enhance_out'
    rep, dry = json.loads((out / 'metrics.json').read_text()), json.loads((tmp_path / 'exp' / 'dry' / 'metrics.json').read_text())
    assert sorted(rep['utterances']) == ['uttA__mix0', 'uttB__mix0', 'uttC__mix0']
    for utt, m in rep['utterances'].items():
        assert all(np.isfinite(v) for v in m.values()), (utt, m)
        y = wav_io.read_wav(str(out / 'mix_enhanced_wav' / (utt + '.wav')))
        assert y.shape[0] == wav_io.wav_frames(str(tmp_path / (utt.split('__')[0] + '.wav')))
        # the reference of the scores is the DRY signal: a reverberant mixture at the same draws scores below the plain one
        assert m['si_sdr_mix'] < dry['utterances'][utt]['si_sdr_mix']
    assert all(np.isfinite(v) for v in rep['mean'].values())
