"""csrc/stft.hip (re2e_wav_mix_scale, re2e_wav_stft) against the float64 restatement of tests/refs64_wav.py, through the C ABI (lib.call), in
the protocol of tests/test_feat_kernels_gpu.py: every output is NaN before the call and sits between guards inside one allocation, which
must come back untouched; outputs and the PCM blob start off their natural alignment; each call runs twice on fresh buffers and the second
result must equal the first bit for bit; rows t >= T_b are exactly zero (Tmax is one more than the longest utterance needs).

Shapes (tests/refs64_wav.py CASES, B <= 3): speech of 257, 511, 512, 1279 and 2303 samples (T = 2, 2, 3, 5, 9: below, at and above the 8 frames
of a workgroup, ragged inside one batch), noise of 100 samples (wraps many times), 700 with the segment starting at its end, and 5000.

Bars against float64 (refs64_wav.violations), with the fp32 CPU run of the same restatement printed beside the kernel's distance and held
to a quarter of each: magnitudes and g 1e-5 of the max; logs at bins with |X| >= 1e-3 max within (10 / ln 10) * 1e-5 max / |X| * cmvn[1],
elsewhere finite and not below the clamp floor; cos and exp(i angle) 1e-4 absolute where the magnitudes are >= 1e-3 of their max (at least
99% of the bins of every case: tests/test_refs64_wav_cpu.py).  GPU only.

Measured on an MI355X when the module was written, worst case over the cases, HIP / fp32 on the CPU: magnitudes 1.3e-7 / 1.3e-7 of the max and g
5.3e-8 / 5.3e-8 (bar 1e-5); logs 0.16 / 0.14 of their bound; cos 2.3e-5 / 1.6e-5, exp(i angle) 4.1e-5 / 1.6e-5 (bar 1e-4).  Against Kaldi records of
the same spectra (tests/test_wav_frontend_gpu.py): clean, mix, mix_log bit-equal, cos 6.2e-7; 8-bit compressed records 1.2e-2 of the max."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import refs64_wav as R
from test_feat_kernels_gpu import DEV, _Out, _twice
from test_loss_kernels_gpu import _ops

pytestmark = pytest.mark.gpu

OUTS = ('clean', 'clean_log', 'mix', 'mix_log', 'cos', 'clean_ang', 'mix_ang')          # re2e_wav_stft's argument order
CLEAN_OUTS = ('clean', 'clean_log', 'clean_ang')


def _longs(v):
    return (ctypes.c_long * len(v))(*[int(x) for x in v])


@functools.lru_cache(maxsize=None)
def _refs(name, cmvn=True, noise=True):
    return R.case_refs(name, cmvn=cmvn, noise=noise), R.case_refs(name, np.float32, cmvn=cmvn, noise=noise)


def _blob(speech, noise):
    """One int16 device blob: every signal starts at an ODD sample (2 bytes off any 4-byte boundary), with 0x7FFF fillers between them."""
    parts, offs, pos = [], [], 0
    for a in list(speech) + [noise]:
        pad = 1 if pos % 2 == 0 else 2
        parts.append(np.full(pad, 0x7FFF, np.int16))
        pos += pad
        offs.append(pos)
        parts.append(a)
        pos += a.shape[0]
    parts.append(np.full(3, 0x7FFF, np.int16))
    return torch.from_numpy(np.concatenate(parts)).to(DEV), offs[:-1], offs[-1]


def _run(lib, name, outs=OUTS, cmvn=True, noise=True, extra_rows=1, signals=None, s0=None):
    """One re2e_wav_mix_scale + re2e_wav_stft of a case -> {output: (B, Tmax, 257) CPU tensor, 'scale': (B,), 'zeros': int}."""
    speech, nz, cm = signals or R.case_signals(name)
    lens, N, s0_case, db = R.ALL_CASES[name]
    s0 = s0_case if s0 is None else s0
    B = len(speech)
    Tmax = max(R.n_frames(L) for L in lens) + extra_rows
    blob, soff, noff = _blob(speech, nz)
    out = {k: _Out((B, Tmax, R.NBIN), off=1 + i % 3) for i, k in enumerate(outs)}
    cm_d = torch.from_numpy(cm).to(DEV) if cmvn else None
    p = lambda k: out[k].ptr() if k in out else None
    res = {}
    if noise:
        scale = _Out((B,), off=1)
        zeros = torch.zeros(1, dtype=torch.int32, device=DEV)
        idx = (_longs(soff), _longs(lens), _longs([noff] * B), _longs([nz.shape[0]] * B), _longs(s0))
        lib.call('re2e_wav_mix_scale', blob.data_ptr(), *idx, (ctypes.c_float * B)(*db), B, scale.ptr(), zeros.data_ptr())
        lib.call('re2e_wav_stft', blob.data_ptr(), *idx, scale.ptr(), B, Tmax, *[p(k) for k in OUTS], cm_d.data_ptr() if cmvn else None)
        res['scale'] = scale.result(name + ' scale')
        res['zeros'] = zeros.cpu()
    else:
        lib.call('re2e_wav_stft', blob.data_ptr(), _longs(soff), _longs(lens), None, None, None, None, B, Tmax, *[p(k) for k in OUTS],
                 cm_d.data_ptr() if cmvn else None)
    for k in outs:
        res[k] = out[k].result('%s %s' % (name, k))
    return res


def _per_utt(res, b, T):
    got = {k: v[b, :T].numpy() for k, v in res.items() if k in OUTS}
    if 'scale' in res:
        got['g'] = float(res['scale'][b])
    return got


def _check(name, res, cmvn=True, noise=True):
    """Padded rows exactly zero; every utterance within the bars of its float64 reference, the fp32 CPU run within a quarter of them."""
    lens = R.ALL_CASES[name][0]
    cm = R.case_signals(name)[2] if cmvn else None
    r64s, r32s = _refs(name, cmvn, noise)
    for b, L in enumerate(lens):
        T = R.n_frames(L)
        for k in res:
            if k in OUTS:
                assert torch.isfinite(res[k][b]).all(), '%s %s utt %d: not finite' % (name, k, b)
                assert (res[k][b, T:] == 0).all() and res[k].shape[1] > T, '%s %s utt %d: rows beyond its %d frames are not zero' % (name, k, b, T)
        got = _per_utt(res, b, T)
        cpu = {k: v for k, v in r32s[b].items() if k in got}
        hip_d, cpu_d = R.distances(got, r64s[b], cm), R.distances(cpu, r64s[b], cm)
        print('ERR %-12s utt %d (L %4d)  %s' % (name, b, L, '  '.join('%s hip %.2e fp32-cpu %.2e' % (k, hip_d[k], cpu_d[k]) for k in sorted(hip_d))))
        assert R.violations(cpu, r64s[b], cm, frac=0.25) == [], '%s utt %d: the fp32 CPU run is not within a quarter of a bar' % (name, b)
        assert R.violations(got, r64s[b], cm) == [], '%s utt %d' % (name, b)


@pytest.mark.parametrize('name', sorted(R.ALL_CASES))
def test_front_end_against_float64(name):
    """Every output with cmvn, twice.  'silence': all-zero speech -- every bin at the clamp floor, angles 0, cos 1, g 0."""
    _, lib = _ops()
    res = _twice(lambda: _run(lib, name), name)
    assert int(res['zeros']) == 0
    _check(name, res)
    if name in R.FLOOR_CASES:
        assert (res['clean'][:, :2] == np.float32(1e-7)).all() and (res['mix'][:, :2] == np.float32(1e-7)).all()
        assert (res['clean_ang'] == 0).all() and (res['mix_ang'] == 0).all() and (res['cos'][:, :2] == 1).all() and float(res['scale'][0]) == 0.0


def test_each_optional_output_absent_in_turn():
    """Dropping an output changes nothing in the others (bit for bit) and writes nothing in its place; without cmvn the logs are plain
    10 log10; with no output at all the call is still accepted."""
    _, lib = _ops()
    name = 'near_end700'
    full = _run(lib, name)
    for drop in OUTS:
        part = _run(lib, name, outs=tuple(k for k in OUTS if k != drop))
        for k in part:
            assert torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), 'without %s: %s differs' % (drop, k)
    plain = _twice(lambda: _run(lib, name, cmvn=False), name + ' no cmvn')
    _check(name, plain, cmvn=False)
    for k in ('clean', 'mix', 'cos', 'clean_ang', 'mix_ang'):
        assert torch.equal(plain[k].view(torch.int32), full[k].view(torch.int32)), k
    assert set(_run(lib, name, outs=())) == {'scale', 'zeros'}


@pytest.mark.parametrize('name', ['wrap100', 'single'])
def test_clean_only(name):
    """noise_off == NULL (recognition): the clean stream alone, against float64."""
    _, lib = _ops()
    res = _twice(lambda: _run(lib, name, outs=CLEAN_OUTS, noise=False), name + ' clean only')
    _check(name, res, noise=False)


def test_refusals_write_nothing():
    _, lib = _ops()
    blob = torch.zeros(4096, dtype=torch.int16, device=DEV)
    outs = [_Out((1, 4, R.NBIN)) for _ in OUTS]
    scale = _Out((1,))
    ptrs = [o.ptr() for o in outs]
    one = lambda v: _longs([v])
    noise = (one(2000), one(100), one(5))
    cases = [
        ('shorter than 257', (one(0), one(256)) + noise + (scale.ptr(), 1, 4)),
        ('Tmax', (one(0), one(1279)) + noise + (scale.ptr(), 1, 4)),                      # T = 5 frames
        ('scale', (one(0), one(512)) + noise + (None, 1, 4)),
        ('noise_start', (one(0), one(512), one(2000), one(100), one(100), scale.ptr(), 1, 4)),
    ]
    for word, args in cases:
        with pytest.raises(lib.Re2eError) as e:
            lib.call('re2e_wav_stft', blob.data_ptr(), *args, *ptrs, None)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(lib.Re2eError) as e:
        lib.call('re2e_wav_mix_scale', blob.data_ptr(), one(0), one(100), *noise, (ctypes.c_float * 1)(5.0), 1, scale.ptr(), None)
    assert 'shorter than 257' in str(e.value)
    with pytest.raises(lib.Re2eError) as e:          # a mixture output without noise
        lib.call('re2e_wav_stft', blob.data_ptr(), one(0), one(512), None, None, None, None, 1, 4, *ptrs, None)
    assert 'without noise' in str(e.value)
    for o in outs + [scale]:
        assert torch.isnan(o.result('refusal')).all(), 'a refused call wrote an output'


def test_zero_power_noise_segment_is_counted():
    """A segment of digital silence inside a noise file that is not silent elsewhere: g = 0, mix == clean, the device counter goes to 1 (the
    other utterance of the batch, on the live part of the same file, is mixed as usual)."""
    _, lib = _ops()
    name = 'long5000'
    speech, nz, cm = R.case_signals(name)
    speech, nz = speech[:2], nz.copy()
    nz[1000:3000] = 0
    s0 = (1100, 3500)                       # 1279 samples from 1100: all zero; 511 from 3500: live
    blob, soff, noff = _blob(speech, nz)
    B, lens, Tmax = 2, [1279, 511], 6
    out = {k: _Out((B, Tmax, R.NBIN)) for k in ('clean', 'mix', 'mix_log', 'clean_log', 'cos')}
    scale, zeros = _Out((B,)), torch.zeros(1, dtype=torch.int32, device=DEV)
    idx = (_longs(soff), _longs(lens), _longs([noff] * B), _longs([5000] * B), _longs(s0))
    lib.call('re2e_wav_mix_scale', blob.data_ptr(), *idx, (ctypes.c_float * B)(5.0, 5.0), B, scale.ptr(), zeros.data_ptr())
    lib.call('re2e_wav_stft', blob.data_ptr(), *idx, scale.ptr(), B, Tmax, out['clean'].ptr(), out['clean_log'].ptr(), out['mix'].ptr(),
             out['mix_log'].ptr(), out['cos'].ptr(), None, None, None)
    g = scale.result('scale')
    res = {k: o.result(k) for k, o in out.items()}
    assert int(zeros.cpu()) == 1 and float(g[0]) == 0.0
    assert torch.equal(res['mix'][0], res['clean'][0]) and torch.equal(res['mix_log'][0], res['clean_log'][0])
    assert ((res['cos'][0, :5] - 1).abs() <= 1e-6).all()          # a unit vector against itself, in fp32
    ref = R.features(speech[1], nz, s0[1], 5.0)
    assert abs(float(g[1]) - ref['g']) <= 1e-5 * ref['g']
    assert R.violations({'mix': res['mix'][1, :2].numpy(), 'clean': res['clean'][1, :2].numpy()}, ref) == []
