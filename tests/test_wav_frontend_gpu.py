"""The waveform input path end to end on the GPU (data/wav_dataset.py, mix_data_loader.collate_wav_device / wav_features_device,
tools/prepare_feats.py on csrc/stft.hip):

  * the two input paths agree: tools/prepare_feats.py writes float32 Kaldi records from tiny wavs with fixed draws, and
    ``collate_kaldi_device`` over those records equals ``collate_wav_device`` with the same draws bit for bit in clean, mix, mix_log, the
    sizes and the targets; cos (cos(clean_angle - mix_angle) there, Re(C conj M) / (|C||M|) here) within the 1e-4 bar.  With 8-bit
    compressed records they agree to the compression step only: that distance is printed, not asserted
  * MixWavDataset.compute_cmvn (spectra and per-bin sums on the device) against the float64 restatement over the same mixtures, written as
    (2, 257) to exp_path/cmvn.npy
  * two JointTrainer steps on wav batches through DevicePrefetcher give finite meters and move the parameters
  * wav_features_device -> EnhanceModel -> FbankModel -> E2E.recognize runs from a wav and equals the same call on the features of the
    float64 restatement (tests/refs64_wav.py) cast to fp32: same yseq, scores within 1e-4 * max(1, |score|).
GPU only; every test takes a few seconds."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import refs64_wav as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UTTS = (('uttA', 9233), ('uttB', 8200), ('uttC', 7001))          # T = 37, 33, 28
NOISES = (('n1', 700), ('n2', 12000))


def _corpus(tmp_path):
    from robust_e2e_gan_amd.data import wav_io
    rng = np.random.RandomState(5)
    sig = {}
    for name, n in UTTS + NOISES:
        sig[name] = np.clip(np.round(rng.randn(n) * (5000 if name.startswith('utt') else 1500)), -32768, 32767).astype(np.int16)
        wav_io.write_wav(str(tmp_path / (name + '.wav')), sig[name])
    (tmp_path / 'clean_wav.scp').write_text(''.join('%s %s\n' % (u, tmp_path / (u + '.wav')) for u, _ in UTTS))
    (tmp_path / 'noise.scp').write_text(''.join('%s\n' % (tmp_path / (n + '.wav')) for n, _ in NOISES))
    (tmp_path / 'utt2spk').write_text(''.join('%s spk%s\n' % (u, u[-1]) for u, _ in UTTS))
    (tmp_path / 'text_char').write_text('uttA 1 2 3 4\nuttB 5 6 7\nuttC 8 9 1 2 3\n')
    (tmp_path / 'dict').write_text(''.join('%d %d\n' % (i, i) for i in range(1, 11)))          # odim 12 with <blank> and <eos>
    rs = np.random.RandomState(9)
    cmvn = torch.from_numpy(np.stack([-(40 + 5 * rs.rand(257)), 0.1 + 0.05 * rs.rand(257)]).astype(np.float32))
    return sig, cmvn


def _wav_dataset(tmp_path, seed=7, repeat=1):
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    return MixWavDataset(argparse.Namespace(noise_repeat_num=repeat, seed=seed, normalize_type=0), str(tmp_path), str(tmp_path / 'dict'))


def test_kaldi_records_and_wav_input_agree(tmp_path):
    from robust_e2e_gan_amd import lib
    from robust_e2e_gan_amd.data.kaldi_dataset import MixKaldiDataset
    from robust_e2e_gan_amd.data.mix_data_loader import collate_kaldi_device, collate_wav_device
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import prepare_feats
    finally:
        sys.path.pop(0)
    assert lib.query('re2e_device_ok') == 1
    _, cmvn = _corpus(tmp_path)
    ds = _wav_dataset(tmp_path)
    draws = prepare_feats.prepare(str(tmp_path), str(tmp_path / 'feats'), 1, compress=False, seed=7, device=DEV, batch=2)
    assert [(d[1], d[2], d[3]) for d in draws] == [ds.draw(i) for i in range(len(ds))]
    assert (tmp_path / 'db.scp').read_text().split()[0] == 'uttA__mix0'
    wav = collate_wav_device([ds[i] for i in range(len(ds))], DEV, cmvn, want=('clean', 'clean_log', 'mix', 'mix_log', 'cos'))
    kargs = argparse.Namespace(feat_type='kaldi_magspec', normalize_type=0)
    kd = MixKaldiDataset(kargs, str(tmp_path), str(tmp_path / 'dict'), raw=True)
    kal = collate_kaldi_device([kd[i] for i in range(len(kd))], DEV, cmvn)
    torch.cuda.synchronize()
    assert wav[0] == kal[0] == ['uttA__mix0', 'uttB__mix0', 'uttC__mix0'] and wav[1] == kal[1]
    assert torch.equal(wav[8], kal[8]) and wav[8].tolist() == [37, 33, 28] and torch.equal(wav[9], kal[9]) and torch.equal(wav[7], kal[7])
    for k, name in ((2, 'clean'), (3, 'clean_log'), (4, 'mix'), (5, 'mix_log')):
        assert torch.equal(wav[k].view(torch.int32), kal[k].view(torch.int32)), '%s: the two input paths differ' % name
    both = (wav[2] >= 1e-3 * wav[2].max()) & (wav[4] >= 1e-3 * wav[4].max())
    d = (wav[6] - kal[6]).abs()
    print('cos: wav path against records, kept bins %.2e (bar 1e-4), all bins %.2e' % (d[both].max().item(), d.max().item()))
    assert d[both].max().item() <= 1e-4 and int(both.sum()) >= 0.99 * sum(wav[8].tolist()) * 257          # the bar reaches 99% of the valid bins
    for b, T in enumerate(wav[8].tolist()):
        assert (wav[6][b, T:] == 0).all() and (wav[4][b, T:] == 0).all()
    # 8-bit compressed records (what copy-feats --compress=true stores): agreement to the compression step only -- reported, not asserted
    prepare_feats.prepare(str(tmp_path), str(tmp_path / 'feats_cm'), 1, compress=True, seed=7, device=DEV, batch=3)
    kc = MixKaldiDataset(kargs, str(tmp_path), str(tmp_path / 'dict'), raw=True)
    assert kc[0][3].kind == 'CM'
    cm = collate_kaldi_device([kc[i] for i in range(len(kc))], DEV, cmvn)
    print('compressed records against the wav path, of the max: clean %.2e mix %.2e' % (
        ((cm[2] - wav[2]).abs().max() / wav[2].max()).item(), ((cm[4] - wav[4]).abs().max() / wav[4].max()).item()))


def test_joint_training_from_wav_batches(tmp_path):
    import __graft_entry__ as g
    from robust_e2e_gan_amd.data.mix_data_loader import collate_wav_device
    from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher
    from robust_e2e_gan_amd.joint_train import JointTrainer
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    from robust_e2e_gan_amd.model.gan_model import GANModel
    _, cmvn = _corpus(tmp_path)
    ds = _wav_dataset(tmp_path, repeat=2)
    opt = g._tiny_opt()
    assert opt.idim == 257 and opt.odim == ds.num_classes == 12
    torch.manual_seed(3)
    enh, fb, asr, gan = (m.to(DEV).train() for m in (EnhanceModel(opt), FbankModel(opt), ShareE2E(opt), GANModel(opt)))
    tr = JointTrainer(opt, enh, fb, asr, gan)
    fbank_cmvn = torch.from_numpy(dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'joint_tiny.npz')))['cmvn'])
    before = {k: v.detach().clone() for m in (enh, asr, gan) for k, v in m.state_dict().items() if v.dtype == torch.float32}
    batches = [[ds[i] for i in range(3)], [ds[i] for i in range(3, 6)]]
    steps = 0
    for data in DevicePrefetcher(batches, DEV, collate=lambda b, d, p: collate_wav_device(b, d, cmvn, pool=p)):
        assert data[2].is_cuda and data[2].shape == (3, 37, 257) and data[3] is None and data[6] is None
        out = JointTrainer.to_floats(tr.step(data, 0.0, fbank_cmvn))
        assert out and all(np.isfinite(v) for v in out.values()), out
        steps += 1
    torch.cuda.synchronize()
    assert steps == 2
    after = {k: v for m in (enh, asr, gan) for k, v in m.state_dict().items() if k in before}
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    assert len(moved) >= len(before) // 2 and all(torch.isfinite(v).all() for v in after.values())
    # the second epoch mixes the same utterances anew
    ds.set_epoch(1)
    assert ds.draw(0) != ds.draw(0, epoch=0)


def test_recognition_from_a_wav(tmp_path):
    import __graft_entry__ as g
    from robust_e2e_gan_amd.data import wav_io
    from robust_e2e_gan_amd.data.mix_data_loader import wav_features_device
    from robust_e2e_gan_amd.model.e2e_model import ShareE2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    _, cmvn = _corpus(tmp_path)
    opt = g._tiny_opt()
    torch.manual_seed(4)
    enh, fb, asr = (m.to(DEV).eval() for m in (EnhanceModel(opt), FbankModel(opt), ShareE2E(opt)))
    fbank_cmvn = torch.from_numpy(dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'joint_tiny.npz')))['cmvn']).to(DEV)
    args = argparse.Namespace(beam_size=3, penalty=0.0, ctc_weight=0.3, maxlenratio=0.3, minlenratio=0.0, nbest=2, lm_weight=0.0)
    pcm = wav_io.read_wav(str(tmp_path / 'uttB.wav'))

    def recognise(inputs, log_inputs, sizes):
        with torch.no_grad():
            feats = fb(enh(inputs, log_inputs, sizes), fbank_cmvn)
        return asr.recognize(feats[0:1, :int(sizes[0])], args, opt.char_list)
    inputs, log_inputs, sizes = wav_features_device([pcm], DEV, cmvn)
    assert inputs.shape == (1, 33, 257) and sizes.tolist() == [33]
    got = recognise(inputs, log_inputs, sizes)
    ref = R.features(pcm, cmvn=cmvn.numpy())
    t32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))[None].to(DEV)
    want = recognise(t32(ref['clean']), t32(ref['clean_log']), sizes)
    assert len(got) == len(want) >= 1
    for a, b in zip(got, want):
        assert list(a['yseq']) == list(b['yseq'])
        assert abs(float(a['score']) - float(b['score'])) <= 1e-4 * max(1.0, abs(float(b['score']))), (a['score'], b['score'])


def test_cmvn_over_the_mixtures_on_the_device(tmp_path):
    """[-mean; 1/sqrt(var)] of 10 log10 |M| per bin over every mixture of the tiny corpus (98 frames), against float64.  Bars: -mean 1e-5 of its
    max (the forward bar; the sums are fp32 on the device, float64 across batches); 1/sqrt(var) 1e-4 relative -- var = E[x^2] - mean^2 with both
    terms near 3e3 carried in fp32 (6e-8 each) against a variance near 30: 1e-5 of the variance, half of that on its inverse root, times
    eight for the sums' own rounding."""
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    _corpus(tmp_path)
    args = argparse.Namespace(noise_repeat_num=1, seed=7, normalize_type=1, exp_path=str(tmp_path / 'exp'), num_utt_cmvn=100)
    ds = MixWavDataset(args, str(tmp_path), str(tmp_path / 'dict'))
    assert ds.cmvn.shape == (2, 257) and ds.cmvn.dtype == np.float32
    assert np.array_equal(np.load(str(tmp_path / 'exp' / 'cmvn.npy')), ds.cmvn)
    logs = []
    for i in range(len(ds)):
        it = ds[i]
        logs.append(10 * np.log10(R.features(it[2], it[3], it[4], it[5])['mix']))
    x = np.concatenate(logs, 0)
    assert x.shape == (37 + 33 + 28, 257)
    mean, var = x.mean(0), (x ** 2).mean(0) - x.mean(0) ** 2
    e_mean = np.abs(ds.cmvn[0] + mean).max() / np.abs(mean).max()
    e_istd = np.abs(ds.cmvn[1] * np.sqrt(var) - 1).max()
    print('cmvn on the device against float64: -mean %.2e of the max (bar 1e-5), 1/sqrt(var) %.2e relative (bar 1e-4)' % (e_mean, e_istd))
    assert e_mean <= 1e-5 and e_istd <= 1e-4
    again = MixWavDataset(args, str(tmp_path), str(tmp_path / 'dict'))          # read back from exp_path, not computed again
    assert np.array_equal(again.cmvn, ds.cmvn)
