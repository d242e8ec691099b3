"""csrc/stft.hip (re2e_wav_istft, re2e_wav_sdr_sums) against the float64 restatement of tests/refs64_istft.py, through the C ABI (lib.call), in
the protocol of tests/test_wav_kernels_gpu.py: every output blob is pre-filled with a sentinel and sits between guards, utterances start at odd
offsets with gaps between them that must come back untouched, rows t >= T_b of the inputs are NaN, each call runs twice on fresh buffers and
the second result must equal the first bit for bit.

Shapes (refs64_istft.LENGTHS): 257, 511, 512, 1279, 2303 samples (T = 2, 2, 3, 5, 9), 1600 (T = 7, odd, below a workgroup's 16 frames), 3917
(T = 16: exactly the frames one workgroup transforms; its zero tail is the first block of the next) and 4196 (T = 17: one frame past it),
each alone and a ragged batch of three with Tmax = 19.  Random spectra that are the STFT of no signal, with imaginary parts at bins 0 and 256.

Bars: the float output within 1e-5 of the tensor's max of float64 (refs64_wav.BAR_MAG; the fp32 CPU run of the restatement is held to a quarter
of it, and every named mistake lies beyond it: tests/test_refs64_istft_cpu.py); tail samples exactly 0; int16 through the real forward within
1 of the PCM; the saturation count exact; the double sums within 1e-10 relative (only the order of the additions differs).  GPU only.

Measured on an MI355X when the module was written, worst case over the cases, HIP / fp32 on the CPU: float output 2.2e-7 / 1.9e-7 of the max (bar
1e-5); through the real forward no sample of any case differs from the PCM (bar 1); the sums 5e-16 relative (bar 1e-10)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import refs64_istft as R
import refs64_wav as W
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu
GUARD = 64
F_SENT, I_SENT = np.float32(-7.25e8), np.int16(-12345)          # what an output blob holds before the call


def _longs(v):
    return (ctypes.c_long * len(v))(*[int(x) for x in v])


def _layout(lens):
    """Offsets of the utterances in a blob: odd starts, gaps of 3 or 4 samples between them.  -> (offsets, blob size)"""
    offs, pos = [], GUARD + 1
    for L in lens:
        pos += 3 if (pos + 3) % 2 else 4
        offs.append(pos)
        pos += L
    return offs, pos + GUARD


def _spectra(lens, seeds, extra_rows=0):
    """(B, Tmax, 257) fp32 mag and ang on the host, rows t >= T_b NaN, and the per-utterance (mag, ang) the references take."""
    Tmax = max(W.n_frames(L) for L in lens) + extra_rows
    mags, angs = [], []
    for L, seed in zip(lens, seeds):
        m, a = R.random_spectrum(L, seed, extra_rows=Tmax - W.n_frames(L))
        mags.append(m)
        angs.append(a)
    return np.stack(mags), np.stack(angs)


def _istft(lib, mag, ang, lens, want_f32=True, want_i16=True, count=True):
    """One re2e_wav_istft -> {'f32': blob, 'i16': blob, 'clip': int} on the host, with the layout."""
    offs, size = _layout(lens)
    B, Tmax = mag.shape[0], mag.shape[1]
    mag_d, ang_d = torch.from_numpy(mag).to(DEV), torch.from_numpy(ang).to(DEV)
    f32 = torch.full((size,), float(F_SENT), dtype=torch.float32, device=DEV) if want_f32 else None
    i16 = torch.full((size,), int(I_SENT), dtype=torch.int16, device=DEV) if want_i16 else None
    clip = torch.zeros(1, dtype=torch.int32, device=DEV) if count else None
    lib.call('re2e_wav_istft', mag_d.data_ptr(), ang_d.data_ptr(), _longs(offs), _longs(lens), B, Tmax, size,
             f32.data_ptr() if want_f32 else None, i16.data_ptr() if want_i16 else None, clip.data_ptr() if count else None)
    torch.cuda.synchronize()
    return {'f32': f32.cpu() if want_f32 else None, 'i16': i16.cpu() if want_i16 else None, 'clip': clip.cpu() if count else None}, offs


def _twice(run):
    (a, offs), (b, _) = run(), run()
    for k in a:
        if a[k] is not None:
            x, y = (a[k].view(torch.int32), b[k].view(torch.int32)) if a[k].dtype == torch.float32 else (a[k], b[k])
            assert torch.equal(x, y), '%s: the second run differs from the first' % k
    return a, offs


def _untouched(blob, offs, lens, sentinel, tag):
    mask = np.ones(blob.shape[0], bool)
    for o, L in zip(offs, lens):
        mask[o:o + L] = False
    assert (blob.numpy()[mask] == sentinel).all(), '%s: written outside the utterances\' ranges' % tag


@functools.lru_cache(maxsize=None)
def _ref(L, seed):
    mag, ang = R.random_spectrum(L, seed)
    ref = R.istft(mag, ang, L)
    return ref, R.margin_ok(mag, ang, L, ref)


def _check_random(lib, lens, seeds, extra_rows):
    mag, ang = _spectra(lens, seeds, extra_rows)
    res, offs = _twice(lambda: _istft(lib, mag, ang, lens))
    _untouched(res['f32'], offs, lens, F_SENT, 'float blob')
    _untouched(res['i16'], offs, lens, I_SENT, 'int16 blob')
    total_clip = 0
    for b, (L, seed) in enumerate(zip(lens, seeds)):
        ref, cpu = _ref(L, seed)
        got = res['f32'][offs[b]:offs[b] + L].numpy()
        n = R.HOP * (W.n_frames(L) - 1)
        assert np.isfinite(got).all(), 'utt %d (L %d): not finite (a padded row was read?)' % (b, L)
        err = R.rel_err(got, ref)
        print('ERR istft L %5d T %2d  hip %.2e  fp32-cpu %.2e  bar %.0e' % (L, W.n_frames(L), err, cpu, R.BAR))
        assert err <= R.BAR, 'utt %d (L %d): %.3e of the max from float64 (bar %.1e, fp32 on the CPU %.3e)' % (b, L, err, R.BAR, cpu)
        assert (got[n:] == 0).all(), 'utt %d (L %d): tail samples are not exactly 0' % (b, L)
        pcm = res['i16'][offs[b]:offs[b] + L].numpy()
        want, clipped = R.to_int16(got)                 # the int16 output is the float output rounded and saturated, bit for bit
        total_clip += clipped
        assert (pcm == want).all(), 'utt %d (L %d): int16 output is not rintf + saturation of the float output' % (b, L)
    assert int(res['clip']) == total_clip


@pytest.mark.parametrize('L', R.LENGTHS)
def test_random_spectra_against_float64(L):
    _, lib = _ops()
    _check_random(lib, (L,), (100 + R.LENGTHS.index(L),), extra_rows=1)


def test_ragged_batch_with_nan_rows():
    _, lib = _ops()
    _check_random(lib, R.RAGGED, (200, 201, 202), extra_rows=2)


def test_either_output_alone_is_the_same_bits():
    _, lib = _ops()
    lens, seeds = (1600, 4196), (7, 8)
    mag, ang = _spectra(lens, seeds)
    both, _ = _istft(lib, mag, ang, lens)
    only_f, _ = _istft(lib, mag, ang, lens, want_i16=False, count=False)
    only_i, _ = _istft(lib, mag, ang, lens, want_f32=False, count=False)
    assert torch.equal(only_f['f32'].view(torch.int32), both['f32'].view(torch.int32)) and torch.equal(only_i['i16'], both['i16'])


@pytest.mark.parametrize('L', R.LENGTHS)
def test_through_the_real_forward(L):
    """PCM -> re2e_wav_stft (clean, clean_ang) -> re2e_wav_istft -> int16: within 1 of the PCM on every restored sample, zero behind them."""
    _, lib = _ops()
    x = R.speech(L, L)
    T = W.n_frames(L)
    blob = torch.from_numpy(np.concatenate([np.full(1, 0x7FFF, np.int16), x])).to(DEV)
    mag = torch.full((1, T + 1, R.NBIN), float('nan'), device=DEV)
    ang = torch.full((1, T + 1, R.NBIN), float('nan'), device=DEV)
    lib.call('re2e_wav_stft', blob.data_ptr(), _longs([1]), _longs([L]), None, None, None, None, 1, T + 1, mag.data_ptr(), None, None, None, None,
             ang.data_ptr(), None, None)
    mag[:, T:], ang[:, T:] = float('nan'), float('nan')          # the forward zeroes the padded row: the inverse must not need it
    res, offs = _twice(lambda: _istft(lib, mag.cpu().numpy(), ang.cpu().numpy(), (L,), want_f32=False))
    pcm = res['i16'][offs[0]:offs[0] + L].numpy().astype(np.int64)
    n = R.HOP * (T - 1)
    d = np.abs(pcm[:n] - x[:n].astype(np.int64))
    print('round trip L %5d: %.4f%% of the samples off by one, none by more' % (L, 100.0 * (d == 1).mean()))
    assert d.max() <= 1, 'L %d: a sample is %d away from the PCM' % (L, d.max())
    assert (pcm[n:] == 0).all() and int(res['clip']) == 0
    _untouched(res['i16'], offs, (L,), I_SENT, 'int16 blob')


def test_saturation_is_clipped_and_counted():
    _, lib = _ops()
    mag, ang, x, pos = R.saturating_spectrum()
    L = x.shape[0]
    want, count = R.to_int16(R.istft(mag, ang, L))
    assert count == len(pos)
    res, offs = _twice(lambda: _istft(lib, mag[None], ang[None], (L,)))
    pcm = res['i16'][offs[0]:offs[0] + L].numpy()
    assert (pcm[pos] == np.where(x[pos] > 0, 32767, -32768)).all(), pcm[pos]
    assert np.abs(np.delete(pcm.astype(np.int64), pos)).max() < 16384
    assert np.abs(pcm.astype(np.int64) - want).max() <= 1
    assert int(res['clip']) == count, 'clip_count %d, float64 says %d' % (int(res['clip']), count)


def test_refusals_write_nothing():
    _, lib = _ops()
    T = 4
    mag = torch.ones(1, T, R.NBIN, device=DEV)
    ang = torch.zeros(1, T, R.NBIN, device=DEV)
    size = 4096
    f32 = torch.full((size,), float(F_SENT), device=DEV)
    i16 = torch.full((size,), int(I_SENT), dtype=torch.int16, device=DEV)
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    one = lambda v: _longs([v])
    m, a, f, i = mag.data_ptr(), ang.data_ptr(), f32.data_ptr(), i16.data_ptr()
    cases = [
        ('shorter than 257', (m, a, one(0), one(256), 1, T, size, f, i)),
        ('Tmax', (m, a, one(0), one(1279), 1, T, size, f, i)),                       # T = 5 frames
        ('mag and ang', (None, a, one(0), one(512), 1, T, size, f, i)),
        ('mag and ang', (m, None, one(0), one(512), 1, T, size, f, i)),
        ('no output', (m, a, one(0), one(512), 1, T, size, None, None)),
        ('offset outside', (m, a, one(-1), one(512), 1, T, size, f, i)),
        ('offset outside', (m, a, one(size - 511), one(512), 1, T, size, f, i)),
    ]
    for word, args in cases:
        with pytest.raises(lib.Re2eError) as e:
            lib.call('re2e_wav_istft', *args, clip.data_ptr())
        assert word in str(e.value), (word, str(e.value))
    # the second of two utterances is the bad one: the first must not have been launched either
    with pytest.raises(lib.Re2eError):
        mag2, ang2 = torch.ones(2, T, R.NBIN, device=DEV), torch.zeros(2, T, R.NBIN, device=DEV)
        lib.call('re2e_wav_istft', mag2.data_ptr(), ang2.data_ptr(), _longs([0, 600]), _longs([512, 100]), 2, T, size, f, i, clip.data_ptr())
    sums = torch.full((1, 3), float('nan'), dtype=torch.float64, device=DEV)
    for word, args in [('null', (None, one(0), f, one(0), one(300), 1, sums.data_ptr())), ('negative offset', (i, one(-1), f, one(0), one(300), 1, sums.data_ptr())),
                       ('length', (i, one(0), f, one(0), one(0), 1, sums.data_ptr()))]:
        with pytest.raises(lib.Re2eError) as e:
            lib.call('re2e_wav_sdr_sums', *args)
        assert word in str(e.value), (word, str(e.value))
    torch.cuda.synchronize()
    assert (f32.cpu().numpy() == F_SENT).all() and (i16.cpu().numpy() == I_SENT).all() and int(clip.cpu()) == 0 and torch.isnan(sums.cpu()).all()


@pytest.mark.parametrize('lens', R.SDR_CASES)
def test_sdr_sums_against_float64(lens):
    _, lib = _ops()
    B = len(lens)
    rng = np.random.RandomState(sum(lens))
    refs = [R.speech(L, L + 1) for L in lens]
    ests = [(0.8 * r + 400 * rng.randn(r.shape[0])).astype(np.float32) for r in refs]
    roffs, rsize = _layout(lens)
    eoffs, esize = _layout([L + 5 for L in lens])          # other offsets than the reference's
    rb, eb = np.full(rsize, 0x7FFF, np.int16), np.full(esize, np.nan, np.float32)
    for o, r in zip(roffs, refs):
        rb[o:o + r.shape[0]] = r
    for o, y in zip(eoffs, ests):
        eb[o:o + y.shape[0]] = y
    rb_d, eb_d = torch.from_numpy(rb).to(DEV), torch.from_numpy(eb).to(DEV)

    def run():
        store = torch.full((GUARD + 3 * B + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
        out = store[GUARD:GUARD + 3 * B]
        lib.call('re2e_wav_sdr_sums', rb_d.data_ptr(), _longs(roffs), eb_d.data_ptr(), _longs(eoffs), _longs(lens), B, out.data_ptr())
        torch.cuda.synchronize()
        s = store.cpu()
        assert torch.isnan(s[:GUARD]).all() and torch.isnan(s[GUARD + 3 * B:]).all(), 'a guard beside the sums was written'
        return s[GUARD:GUARD + 3 * B].view(B, 3).clone()
    first, second = run(), run()
    assert torch.equal(first.view(torch.int64), second.view(torch.int64)), 'the second run differs from the first'
    for b in range(B):
        want = R.sdr_sums(refs[b], ests[b])
        rel = np.abs(first[b].numpy() - want) / np.abs(want)
        print('ERR sdr_sums L %5d  %s (bar 1e-10)' % (lens[b], ' '.join('%.1e' % v for v in rel)))
        assert (rel <= 1e-10).all(), (lens[b], rel)


def test_python_surface():
    """wav_istft_device / wav_sdr_device: lists of arrays, or the blob with its offsets; metrics against float64 of the same signals."""
    _, lib = _ops()
    from robust_e2e_gan_amd.data.mix_data_loader import wav_istft_device, wav_sdr_device
    lens = (2303, 257, 1279)
    xs = [R.speech(L, L + 2) for L in lens]
    Tmax = max(W.n_frames(L) for L in lens)
    mag, ang = np.zeros((3, Tmax, R.NBIN), np.float32), np.zeros((3, Tmax, R.NBIN), np.float32)
    rng = np.random.RandomState(4)
    noisy = [x + 900 * rng.randn(x.shape[0]) for x in xs]
    for b, y in enumerate(noisy):
        X = W.stft(y)
        mag[b, :X.shape[0]], ang[b, :X.shape[0]] = np.abs(X), np.angle(X)
    mag_d, ang_d = torch.from_numpy(mag).to(DEV), torch.from_numpy(ang).to(DEV)
    pcm = wav_istft_device(mag_d, ang_d, lens, DEV)
    flt = wav_istft_device(mag_d, ang_d, lens, DEV, int16=False)
    blob, offs = wav_istft_device(mag_d, ang_d, lens, DEV, int16=False, blob=True)
    assert [p.shape[0] for p in pcm] == list(lens) and all(p.dtype == np.int16 for p in pcm) and all(f.dtype == np.float32 for f in flt)
    assert blob.is_cuda and blob.dtype == torch.float32 and offs == [0, 2303, 2560]
    kept = [R.HOP * (L // R.HOP) for L in lens]
    got = wav_sdr_device(xs, blob, offs, kept)
    for b, L in enumerate(lens):
        assert (pcm[b] == R.to_int16(flt[b])[0]).all() and np.abs(flt[b][:kept[b]] - noisy[b][:kept[b]]).max() <= 1e-5 * np.abs(noisy[b]).max()
        assert abs(got[b]['si_sdr'] - R.si_sdr_direct(xs[b][:kept[b]], flt[b][:kept[b]])) <= 1e-6
        assert abs(got[b]['snr'] - R.snr_direct(xs[b][:kept[b]], flt[b][:kept[b]])) <= 1e-6
        assert 12 < got[b]['snr'] < 22          # 6000 against 900: 16.5 dB
    with pytest.raises(ValueError):
        wav_istft_device(mag_d, ang_d[:2], lens, DEV)
