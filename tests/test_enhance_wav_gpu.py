"""Waveforms out of the enhancer, end to end on the GPU (EnhanceModel.enhance_wav, python -m robust_e2e_gan_amd.enhance_out):

  * enhance_wav of three ragged utterances equals the float64 inverse (tests/refs64_istft.py) of the model's own GPU enhance_out with the
    input's phase, within 1 LSB -- the plumbing between re2e_wav_stft, the masked inference forward and re2e_wav_istft; lengths are kept
  * enhance_out --wav on a tmp data directory (three wavs, noise files, a saved checkpoint): wavs readable and of the right lengths, tables
    readable by kaldi_io.read_mat_scp with rows equal to the model's outputs, metrics.json within 0.05 dB of SI-SDR recomputed in float64
    from the written wavs (the slack: the files are rounded to 16 bits, the kernel's sums are taken before that) and, for the mixture, from
    the float64 mixture of the same draws; without --wav the same tables from Kaldi records.
The model is the tiny BLSTM enhancer of tests/golden/enhance_tiny.npz.  GPU only; every test takes a few seconds."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

import refs64_istft as R
import refs64_wav as W
from test_wav_frontend_gpu import UTTS, _corpus, _wav_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _model():
    import __graft_entry__ as g
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    fx = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'enhance_tiny.npz')))
    opt = g._tiny_opt()
    m = EnhanceModel(opt)
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('p.')}, strict=True)
    return m.to(DEV).eval(), opt


def _cmvn():
    rs = np.random.RandomState(9)
    return torch.from_numpy(np.stack([-(40 + 5 * rs.rand(257)), 0.1 + 0.05 * rs.rand(257)]).astype(np.float32))


def test_enhance_wav_is_the_inverse_of_the_models_own_output():
    from robust_e2e_gan_amd.data.mix_data_loader import wav_frontend_device
    model, _ = _model()
    cmvn = _cmvn()
    pcms = [R.speech(L, 31 + i) for i, L in enumerate((4196, 9233, 1600))]          # T = 17, 37, 7: not sorted
    out = model.enhance_wav(pcms, cmvn)
    assert [o.shape[0] for o in out] == [p.shape[0] for p in pcms] and all(o.dtype == np.int16 for o in out)
    assert all(not p.requires_grad or p.grad is None for p in model.parameters())
    with torch.no_grad():
        o = wav_frontend_device(pcms, DEV, None, cmvn, ('clean', 'clean_log', 'clean_ang'))
        sizes = [W.n_frames(p.shape[0]) for p in pcms]
        eo = model(o['clean'], o['clean_log'], torch.IntTensor(sizes)).cpu().numpy()
    ang = o['clean_ang'].cpu().numpy()
    for b, p in enumerate(pcms):
        L, T = p.shape[0], sizes[b]
        want, clipped = R.to_int16(R.istft(eo[b, :T], ang[b, :T], L))
        d = np.abs(out[b].astype(np.int64) - want)
        print('enhance_wav utt %d (L %d): %.4f%% of the samples one LSB from the float64 inverse, largest |sample| %d' % (
            b, L, 100.0 * (d == 1).mean(), np.abs(want.astype(np.int64)).max()))
        assert d.max() <= 1 and clipped == 0
        assert np.abs(want.astype(np.int64)).max() > 1000 and (out[b][R.HOP * (T - 1):] == 0).all()          # a mask in (0, 1) on speech of 6000 rms


def _checkpoint(tmp_path, model, opt):
    path = str(tmp_path / 'enhance.pth')
    torch.save({'opt': opt, 'enhance_state_dict': {k: v.cpu() for k, v in model.state_dict().items()}}, path)
    return path


def _args(tmp_path, ckpt, *more):
    return ['--enhance_dir', str(tmp_path), '--dict_dir', str(tmp_path / 'dict'), '--resume', ckpt, '--exp_path', str(tmp_path / 'exp'),
            '--normalize_type', '0', '--seed', '7', '--batch_size', '2', '--device', DEV] + list(more)


def test_enhance_out_wav(tmp_path):
    from robust_e2e_gan_amd import enhance_out as E
    from robust_e2e_gan_amd.data import kaldi_io, wav_io
    from robust_e2e_gan_amd.data.mix_data_loader import wav_frontend_device
    sig, _ = _corpus(tmp_path)
    model, opt = _model()
    ckpt = _checkpoint(tmp_path, model, opt)
    E.main(_args(tmp_path, ckpt, '--wav'))
    out = tmp_path / 'exp' / 'enhance_out'
    ds = _wav_dataset(tmp_path, seed=7)
    items = [ds[i] for i in range(len(ds))]
    ids = [it[0] for it in items]
    assert ids == ['uttA__mix0', 'uttB__mix0', 'uttC__mix0']
    assert sorted(os.listdir(str(out))) == ['clean_enhanced', 'metrics.json', 'mix_enhanced', 'mix_enhanced_wav']
    # the tables: the model's own outputs, row for row
    sizes = [W.n_frames(it[2].shape[0]) for it in items]
    for sub, a, b in (('clean_enhanced', 'clean', 'clean_log'), ('mix_enhanced', 'mix', 'mix_log')):
        got = dict(kaldi_io.read_mat_scp(str(out / sub / 'feats.scp')))
        assert list(got) == ids
        for x in range(0, 3, 2):          # the script's batches of two: the same launches, so the same bits
            part = items[x:x + 2]
            with torch.no_grad():
                o = wav_frontend_device([it[2] for it in part], DEV, [(it[3], it[4], it[5]) for it in part], None, (a, b))
                want = model(o[a], o[b], torch.IntTensor(sizes[x:x + 2])).cpu().numpy()
            for j, utt in enumerate(ids[x:x + 2]):
                T = sizes[x + j]
                assert got[utt].shape == (T, 257)
                assert (got[utt] == want[j, :T]).all(), (sub, utt, float(np.abs(got[utt] - want[j, :T]).max()))
        assert (out / sub / 'utt2spk').read_text() == ''.join('%s spk%s\n' % (u, u[3]) for u in ids)
        assert (out / sub / 'text_char').read_text().splitlines()[0] == 'uttA__mix0 1 2 3 4'
    # the wavs and the figures
    rep = json.loads((out / 'metrics.json').read_text())
    assert sorted(rep['utterances']) == ids
    for it in items:
        utt, s = it[0], it[2]
        y = wav_io.read_wav(str(out / 'mix_enhanced_wav' / (utt + '.wav')))
        assert y.shape[0] == s.shape[0] == dict(UTTS)[utt.split('__')[0]]
        n = R.HOP * (s.shape[0] // R.HOP)
        m = rep['utterances'][utt]
        assert abs(m['si_sdr_enhanced'] - R.si_sdr_direct(s[:n], y[:n])) <= 0.05, utt
        g = W.mix_scale(s, it[3], it[4], it[5])
        mixture = s.astype(np.float64) + g * W.noise_segment(it[3], it[4], s.shape[0])
        assert abs(m['si_sdr_mix'] - R.si_sdr_direct(s[:n], mixture[:n])) <= 0.05, utt          # istft(stft(m)) is m on the kept samples
        assert abs(m['si_sdr_improvement'] - (m['si_sdr_enhanced'] - m['si_sdr_mix'])) <= 1e-9
        assert -5 < m['si_sdr_mix'] < 25 and np.isfinite(m['snr_enhanced'])
    mean = np.mean([rep['utterances'][u]['si_sdr_improvement'] for u in ids])
    assert abs(rep['mean']['si_sdr_improvement'] - mean) <= 1e-9


def test_enhance_out_from_kaldi_tables(tmp_path):
    from robust_e2e_gan_amd import enhance_out as E
    from robust_e2e_gan_amd.data import kaldi_io
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import prepare_feats
    finally:
        sys.path.pop(0)
    _corpus(tmp_path)
    prepare_feats.prepare(str(tmp_path), str(tmp_path / 'feats'), 1, compress=False, seed=7, device=DEV, batch=3)
    model, opt = _model()
    ckpt = _checkpoint(tmp_path, model, opt)
    E.main(_args(tmp_path, ckpt, '--enhance_out_dir', 'k'))
    E.main(_args(tmp_path, ckpt, '--wav', '--enhance_out_dir', 'w'))
    assert sorted(os.listdir(str(tmp_path / 'exp' / 'k'))) == ['clean_enhanced', 'mix_enhanced']
    for sub in E.STREAMS:
        k = dict(kaldi_io.read_mat_scp(str(tmp_path / 'exp' / 'k' / sub / 'feats.scp')))
        w = dict(kaldi_io.read_mat_scp(str(tmp_path / 'exp' / 'w' / sub / 'feats.scp')))
        assert sorted(k) == sorted(w) == ['uttA__mix0', 'uttB__mix0', 'uttC__mix0']
        for utt in k:          # float32 records of the same spectra: the two input paths give the same enhanced features
            assert k[utt].shape == w[utt].shape and np.abs(k[utt] - w[utt]).max() <= 1e-4 * np.abs(w[utt]).max(), (sub, utt)
        assert (tmp_path / 'exp' / 'k' / sub / 'text_char').read_text() == (tmp_path / 'exp' / 'w' / sub / 'text_char').read_text()
