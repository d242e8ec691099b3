"""tests/refs64_istft.py, the float64 restatement re2e_wav_istft and re2e_wav_sdr_sums are held to (tests/test_istft_kernels_gpu.py), checked on
the CPU: two derivations of the inverse agree; it inverts refs64_wav.stft; every named mistake lands outside the bar of every case; the
fp32 run of the same statements stays within a quarter of the bar; the host side of the metrics and of enhance_out."""
import json
import os

import numpy as np
import pytest

import refs64_istft as R
import refs64_wav as W

CASES = [(L, 100 + i) for i, L in enumerate(R.LENGTHS)] + [(L, 200 + i) for i, L in enumerate(R.RAGGED)]


def test_two_derivations_agree():
    for L, seed in CASES:
        mag, ang = R.random_spectrum(L, seed)
        a, b = R.istft(mag, ang, L), R.istft_ola(mag, ang, L)
        assert a.shape == b.shape == (L,)
        assert R.rel_err(a, b) <= 1e-12, (L, R.rel_err(a, b))
        n = R.HOP * (W.n_frames(L) - 1)
        assert (a[n:] == 0).all() and np.abs(a[:n]).min() > 0


def test_dc_and_nyquist_imaginary_parts_are_ignored():
    L = 1279
    mag, ang = R.random_spectrum(L, 3)
    ang2 = ang.copy()
    ang2[:, 0] = np.where(np.cos(ang[:, 0]) >= 0, 0.0, np.pi)
    mag2 = mag.copy()
    mag2[:, 0] = mag[:, 0] * np.abs(np.cos(ang[:, 0].astype(np.float64)))          # the real part alone
    assert R.rel_err(R.istft(mag2, ang2, L), R.istft(mag, ang, L)) <= 1e-7           # fp32 storage of mag2 and pi
    assert np.abs(np.sin(ang[:, 0])).min() > 0 and np.abs(np.sin(ang[:, 256])).min() > 0


@pytest.mark.parametrize('L', R.LENGTHS)
def test_round_trip_through_the_forward(L):
    x = R.speech(L, L)
    X = W.stft(x)
    y = R.istft(np.abs(X), np.angle(X), L)
    n = R.HOP * (W.n_frames(L) - 1)
    assert np.abs(y[:n] - x[:n]).max() <= 1e-9 * np.abs(x).max()
    pcm, clipped = R.to_int16(y)
    assert clipped == 0 and (pcm[:n] == x[:n]).all() and (pcm[n:] == 0).all()
    # through fp32 storage of the spectrum (what the forward kernel hands over) the restatement is still exact after rounding
    y32 = R.istft(np.abs(X).astype(np.float32), np.angle(X).astype(np.float32), L)
    assert (R.to_int16(y32)[0][:n] == x[:n]).all()


def test_every_mistake_lands_outside_the_bar():
    """For each case of the GPU test, each mistaken reference is further than the bar from the definition: the bar has teeth.  The one
    exemption: 'tail_not_zero' cannot show where there is no tail (L a multiple of 256: the 512-sample case)."""
    for L, seed in CASES:
        mag, ang = R.random_spectrum(L, seed)
        ref = R.istft(mag, ang, L)
        for m in R.MISTAKES:
            if m == 'tail_not_zero' and L % R.HOP == 0:
                assert L == 512
                continue
            e = R.rel_err(R.istft(mag, ang, L, mistake=m), ref)
            assert e > 10 * R.BAR, (L, m, e)


def test_fp32_precondition():
    """The fp32 numpy run of the restatement stays within a quarter of the bar (the bar is not below what fp32 can do)."""
    worst = 0.0
    for L, seed in CASES:
        mag, ang = R.random_spectrum(L, seed)
        worst = max(worst, R.margin_ok(mag, ang, L))
    mag, ang, x, _ = R.saturating_spectrum()
    worst = max(worst, R.margin_ok(mag, ang, x.shape[0]))
    print('fp32 on the CPU against float64: %.2e of the max (bar %.0e)' % (worst, R.BAR))


def test_saturating_case_is_what_it_says():
    mag, ang, x, pos = R.saturating_spectrum()
    y = R.istft(mag, ang, x.shape[0])
    pcm, clipped = R.to_int16(y)
    over = np.abs(y) > 32768
    assert clipped == len(pos) == 7 and sorted(np.nonzero(over)[0]) == sorted(pos)
    assert (np.abs(y[pos]) > 2 * 32767 * 0.999).all() and np.abs(np.delete(y, pos)).max() < 16384
    assert (pcm[pos] == np.where(x[pos] > 0, 32767, -32768)).all()


def test_scipy_agrees_where_it_is_installed():
    sig = pytest.importorskip('scipy.signal')
    L = 2303
    mag, ang = R.random_spectrum(L, 11)
    X = R.spectrum(mag, ang)
    X[:, 0], X[:, 256] = X[:, 0].real, X[:, 256].real
    w = W.window()
    # scipy divides the forward by sum(w) and multiplies the inverse by it: undo the scaling on the way in
    _, y = sig.istft(X.T / w.sum(), window=w, nperseg=512, noverlap=256, nfft=512, input_onesided=True, boundary=True)
    n = R.HOP * (W.n_frames(L) - 1)
    assert R.rel_err(y[:n], R.istft(mag, ang, L)[:n]) <= 1e-10


# ---- host side of the metrics ------------------------------------------------------------------------------------------------------------
def test_sdr_from_sums_against_direct_float64():
    from robust_e2e_gan_amd.data.mix_data_loader import sdr_from_sums
    rng = np.random.RandomState(2)
    for L, noise in ((257, 3000.0), (4097, 300.0), (20000, 30.0), (20000, 0.6)):
        s = R.speech(L, L)
        y = (0.7 * s + noise * rng.randn(L)).astype(np.float32)           # a scaled copy plus noise: SI-SDR ignores the 0.7, SNR does not
        got = sdr_from_sums(*R.sdr_sums(s, y))
        assert abs(got['si_sdr'] - R.si_sdr_direct(s, y)) <= 1e-6, (L, noise)
        assert abs(got['snr'] - R.snr_direct(s, y)) <= 1e-6, (L, noise)
        assert noise > 300 or got['si_sdr'] > got['snr'] + 10          # SNR is capped near 10.5 dB by the missing 0.3 s
    same = sdr_from_sums(*R.sdr_sums(s, s.astype(np.float32)))
    assert same['snr'] == float('inf')
    silent = sdr_from_sums(0.0, 5.0, 0.0)
    assert np.isnan(silent['si_sdr']) and np.isnan(silent['snr'])


# ---- enhance_out: arguments and layout ---------------------------------------------------------------------------------------------------
def test_enhance_out_arguments():
    from robust_e2e_gan_amd import enhance_out as E
    a = E.parse_args(['--enhance_dir', 'd', '--dict_dir', 'dd', '--resume', 'ck.pth', '--exp_path', 'exp'])
    assert (a.enhance_out_dir, a.wav, a.compress, a.batch_size, a.seed, a.noise_repeat_num) == ('enhance_out', False, False, 16, 0, 1)
    a = E.parse_args(['--enhance_dir', 'd', '--dict_dir', 'dd', '--resume', 'ck.pth', '--exp_path', 'exp', '--wav', '--seed', '7', '--enhance_out_dir', 'o',
                      '--batch_size', '3', '--compress'])
    assert (a.enhance_out_dir, a.wav, a.compress, a.batch_size, a.seed) == ('o', True, True, 3, 7)
    for bad in (['--dict_dir', 'dd', '--resume', 'c', '--exp_path', 'e'], ['--enhance_dir', 'd', '--dict_dir', 'dd', '--resume', 'c', '--exp_path', 'e', '--batch_size', '0']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
    assert E.dict_file_of('/nonexistent/dir') == os.path.join('/nonexistent/dir', 'train_units.txt')
    assert E.dict_file_of(__file__) == __file__


def test_enhance_out_layout(tmp_path):
    from robust_e2e_gan_amd import enhance_out as E
    from robust_e2e_gan_amd.data import kaldi_io
    rng = np.random.RandomState(1)
    rows = {'uttB__mix0': rng.rand(5, 257).astype(np.float32), 'uttA__mix0': rng.rand(3, 257).astype(np.float32)}
    d = E.FeatDir(str(tmp_path / 'out' / 'mix_enhanced'))
    for utt, m in rows.items():
        d.add(utt, 'spk' + utt[3], m, ['1', '2', '<eos>'])
    d.close()
    base = tmp_path / 'out' / 'mix_enhanced'
    assert sorted(os.listdir(str(base))) == ['feats.ark', 'feats.scp', 'text_char', 'utt2spk']
    got = list(kaldi_io.read_mat_scp(str(base / 'feats.scp')))
    assert [k for k, _ in got] == list(rows) and all((m == rows[k]).all() for k, m in got)
    assert (base / 'utt2spk').read_text() == 'uttB__mix0 spkB\nuttA__mix0 spkA\n'
    assert (base / 'text_char').read_text() == 'uttB__mix0 1 2 <eos>\nuttA__mix0 1 2 <eos>\n'
    c = E.FeatDir(str(tmp_path / 'cm'), compress=True)
    c.add('u', 's', rows['uttB__mix0'], [])
    c.close()
    (k, m), = kaldi_io.read_mat_scp(str(tmp_path / 'cm' / 'feats.scp'))
    assert k == 'u' and np.abs(m - rows['uttB__mix0']).max() <= 1.0 / 63          # 8 bits: no step is wider than the range (< 1) / 63
    rep = E.summarise({'a': {'si_sdr_mix': 1.0, 'si_sdr_enhanced': 4.0, 'si_sdr_improvement': 3.0},
                       'b': {'si_sdr_mix': 3.0, 'si_sdr_enhanced': float('inf'), 'si_sdr_improvement': float('inf')}})
    assert rep['mean'] == {'si_sdr_mix': 2.0, 'si_sdr_enhanced': 4.0, 'si_sdr_improvement': 3.0}
    assert json.loads(json.dumps(rep))['utterances']['a']['si_sdr_mix'] == 1.0
