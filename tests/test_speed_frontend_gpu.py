"""Speed perturbation end to end on the GPU (csrc/resample.hip through mix_data_loader.wav_frontend_device(speed=...), collate_wav_device,
data/wav_dataset.py with ``speed_perturb``), on the three-utterance corpus of tests/test_wav_frontend_gpu.py:

  * composition is exact: every output of the front end with ``speed`` is bit for bit the output of the same call without it, fed the
    kernel's own int16 resampled arrays as speech -- clean only, with noise, with noise and impulse responses on speech and noise; the clean
    stream is the perturbed dry signal and the frame counts follow L' = ceil(L up / down) (the kernel itself is held to float64 in
    tests/test_resample_kernels_gpu.py)
  * a batch that mixes the speeds 0.9 / 1.0 / 1.1 leaves the rows of the 1.0 utterance bit-equal to its rows in a batch without speeds
  * collate_wav_device sorts by the perturbed length and reports its frame counts; through DevicePrefetcher it gives the same tensors
  * ``speed_perturb='1.0'`` and no ``speed_perturb`` give the batches of today's call form; set_epoch changes the speeds drawn; compute_cmvn
    runs with speeds.
GPU only; every test takes a few seconds."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import refs64_resample as R
import refs64_reverb as RV
from test_wav_frontend_gpu import _corpus

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('clean', 'clean_log', 'mix', 'mix_log', 'cos', 'clean_ang', 'mix_ang')
SPEEDS = [(10, 9), (10, 11), (20, 21)]


def _lib():
    from robust_e2e_gan_amd import lib
    assert lib.query('re2e_device_ok') == 1
    return lib


def _resampled(lib, x, ratio):
    """The kernel's own int16 resampled signal of one utterance (numpy)."""
    if ratio is None:
        return x
    up, down = ratio
    n = R.out_len(x.shape[0], up, down)
    pcm = torch.from_numpy(x).to(DEV)
    out = torch.zeros(n, dtype=torch.int16, device=DEV)
    one = lambda t, v: (t * 1)(int(v))
    lib.call('re2e_wav_resample', pcm.data_ptr(), pcm.numel(), one(ctypes.c_long, 0), one(ctypes.c_long, x.shape[0]), one(ctypes.c_int, up),
             one(ctypes.c_int, down), one(ctypes.c_long, 0), one(ctypes.c_long, n), one(ctypes.c_long, 0), 1, n, None, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), '%s differs' % k


def _signals(tmp_path):
    sig, cmvn = _corpus(tmp_path)
    speech = [sig['uttA'], sig['uttB'], sig['uttC']]
    noise = [(sig['n2'], 11000, 5.0), (sig['n1'], 650, 12.5), (sig['n2'], 300, 0.5)]          # wraps, tiles, inside
    return speech, noise, cmvn


@pytest.mark.parametrize('mode', ['clean_only', 'noise', 'noise_rirs'])
def test_composition_is_exact(tmp_path, mode):
    from robust_e2e_gan_amd.data.mix_data_loader import wav_frames_of, wav_frontend_device
    lib = _lib()
    speech, noise, cmvn = _signals(tmp_path)
    pre = [_resampled(lib, s, r) for s, r in zip(speech, SPEEDS)]
    for s, p, (up, down) in zip(speech, pre, SPEEDS):
        assert p.shape[0] == R.out_len(s.shape[0], up, down) != s.shape[0]
        assert np.abs(p.astype(np.int64) - R.to_pcm(R.resample(s, up, down)).astype(np.int64)).max() <= 1          # it IS the resampled signal
    kw = {}
    want = OUTS
    if mode == 'clean_only':
        noise, want = None, ('clean', 'clean_log', 'clean_ang')
    elif mode == 'noise_rirs':
        kw['reverb'] = [(RV.rir(300, 1), RV.rir(33, 2)), (None, RV.rir(300, 3)), (RV.rir(33, 4), None)]
    got = wav_frontend_device(speech, DEV, noise, cmvn, want, speed=SPEEDS, **kw)
    ref = wav_frontend_device(pre, DEV, noise, cmvn, want, **kw)
    torch.cuda.synchronize()
    _same(got, ref)
    T = [wav_frames_of(p.shape[0]) for p in pre]
    assert got['clean'].shape == (3, max(T), 257)                                   # Tmax follows L'
    for b, t in enumerate(T):
        assert (got['clean'][b, t:] == 0).all() and torch.isfinite(got['clean'][b]).all() and (got['clean'][b, t - 1] != 0).any()
    # the clean stream is the PERTURBED dry signal, not the file's
    dry = wav_frontend_device(speech, DEV, None, cmvn, ('clean',))['clean']
    assert dry.shape[1] != got['clean'].shape[1] or not torch.equal(dry, got['clean'])
    with pytest.raises(ValueError):
        wav_frontend_device(speech, DEV, noise, cmvn, want, speed=SPEEDS[:2])


def test_mixed_speeds_leave_the_unit_speed_rows(tmp_path):
    from robust_e2e_gan_amd.data.mix_data_loader import wav_frames_of, wav_frontend_device
    _lib()
    speech, noise, cmvn = _signals(tmp_path)
    Tmax = wav_frames_of(R.out_len(speech[0].shape[0], 10, 9))
    plain = wav_frontend_device(speech, DEV, noise, cmvn, OUTS, Tmax=Tmax)
    for speeds in ([(10, 9), None, (10, 11)], [(10, 9), (1, 1), (10, 11)]):          # a speed of exactly 1 is not a job, however it is given
        mixed = wav_frontend_device(speech, DEV, noise, cmvn, OUTS, Tmax=Tmax, speed=speeds)
        torch.cuda.synchronize()
        for k in OUTS + ('scale',):
            assert torch.equal(mixed[k][1].view(torch.int32), plain[k][1].view(torch.int32)), k
            assert not torch.equal(mixed[k][0], plain[k][0]) and not torch.equal(mixed[k][2], plain[k][2]), k
    none = wav_frontend_device(speech, DEV, noise, cmvn, OUTS, Tmax=Tmax, speed=[None, None, None])
    torch.cuda.synchronize()
    _same(none, plain)


def _dataset(tmp_path, seed=7, repeat=1, **extra):
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    return MixWavDataset(argparse.Namespace(noise_repeat_num=repeat, seed=seed, normalize_type=0, **extra), str(tmp_path), str(tmp_path / 'dict'))


def _equal_batches(a, b, streams=(2, 3, 4, 5, 6)):
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[7], b[7]) and torch.equal(a[8], b[8]) and torch.equal(a[9], b[9])
    for k in streams:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), 'stream %d differs' % k


def test_collate_sorts_by_the_perturbed_length_and_plugs_into_the_prefetcher(tmp_path):
    from robust_e2e_gan_amd.data.mix_data_loader import collate_wav_device, resampled_len, wav_frames_of
    from robust_e2e_gan_amd.data.prefetch import DevicePrefetcher
    lib = _lib()
    speech, noise, cmvn = _signals(tmp_path)
    # uttA 9233 at speed 1.1 -> 8394, uttB 8200 at 0.9 -> 9112, uttC 7001 at 0.9 -> 7779: the perturbed order is B, A, C
    speeds = [(10, 11), (10, 9), (10, 9)]
    items = [('utt%s' % 'ABC'[b], 'spk', speech[b], noise[b][0], noise[b][1], noise[b][2], [1 + b, 2], (None, None), speeds[b]) for b in range(3)]
    want = ('clean', 'mix', 'mix_log')
    out = collate_wav_device(items, DEV, cmvn, want=want)
    torch.cuda.synchronize()
    Lp = [resampled_len(s.shape[0], r) for s, r in zip(speech, speeds)]
    assert Lp == [8394, 9112, 7779] and out[0] == ['uttB', 'uttA', 'uttC']
    assert out[8].tolist() == [wav_frames_of(Lp[1]), wav_frames_of(Lp[0]), wav_frames_of(Lp[2])] == sorted(out[8].tolist(), reverse=True)
    assert out[7].tolist() == [2, 2, 1, 2, 3, 2] and out[2].shape[1] == out[8][0]
    pre = [_resampled(lib, s, r) for s, r in zip(speech, speeds)]
    ref = collate_wav_device([it[:2] + (p,) + it[3:7] for it, p in zip(items, pre)], DEV, cmvn, want=want)
    torch.cuda.synchronize()
    _equal_batches(out, ref)
    batches = [items[:2], items[2:]]
    direct = [collate_wav_device(b, DEV, cmvn, want=want) for b in batches]
    torch.cuda.synchronize()
    n = 0
    for got, exp in zip(DevicePrefetcher(batches, DEV, collate=lambda b, d, p: collate_wav_device(b, d, cmvn, want=want, pool=p)), direct):
        torch.cuda.synchronize()
        _equal_batches(got, exp)
        n += 1
    assert n == 2


def test_dataset_modes(tmp_path):
    from robust_e2e_gan_amd.data.mix_data_loader import collate_wav_device
    _lib()
    _, cmvn = _corpus(tmp_path)
    none, one = _dataset(tmp_path), _dataset(tmp_path, speed_perturb='1.0')
    want = ('clean', 'clean_log', 'mix', 'mix_log', 'cos')
    a = collate_wav_device([none[i] for i in range(len(none))], DEV, cmvn, want=want)
    b = collate_wav_device([one[i] for i in range(len(one))], DEV, cmvn, want=want)
    torch.cuda.synchronize()
    assert all(len(none[i]) == 7 and len(one[i]) == 9 and one[i][8] is None for i in range(len(none)))
    _equal_batches(a, b)
    ds = _dataset(tmp_path, repeat=4, speed_perturb='0.9,1.0,1.1')
    first = [ds[i][8] for i in range(len(ds))]
    assert set(first) == {(10, 9), None, (10, 11)}
    ds.set_epoch(1)
    assert [ds[i][8] for i in range(len(ds))] != first
    c = collate_wav_device([ds[i] for i in range(len(ds))], DEV, cmvn, want=want)
    torch.cuda.synchronize()
    assert c[8].tolist() == sorted(c[8].tolist(), reverse=True) and all(torch.isfinite(c[k]).all() for k in (2, 3, 4, 5, 6))
    cm = ds.compute_cmvn(device=DEV, batch=5)
    assert cm.shape == (2, 257) and np.isfinite(cm).all() and (cm[1] > 0).all()
