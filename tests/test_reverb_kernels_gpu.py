"""csrc/reverb.hip (re2e_wav_reverb) against the float64 restatement of tests/refs64_reverb.py, through the C ABI (lib.call).  Outputs sit
between guards inside one allocation (NaN for fp32, the sentinel 0x5A5A for int16) and every sample outside the destination ranges must come
back untouched; sources and destinations start at odd and even samples; each call runs twice on fresh buffers and the second result must
equal the first bit for bit.

The bound is derived (refs64_reverb): |y - y64| <= (K + 32) 2^-24 sum_k |h[k] x[.]| per output; the int16 output is saturate(rintf(.)) of
the fp32 output exactly, within 1 of the rounded float64 value, and differs only where that value is within the bound of a half-integer.
The jobs (refs64_reverb.fir_jobs) place their edges at the kernel's own K-tile and outputs per workgroup, asked of the library
(re2e_wav_reverb_geometry); all 34 go in ONE call, which is also more jobs than one launch carries (32).  GPU only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import refs64_reverb as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
GUARD = 64


def _longs(v):
    return (ctypes.c_long * len(v))(*[int(x) for x in v])


def _geometry(lib):
    return lib.query('re2e_wav_reverb_geometry', 0), lib.query('re2e_wav_reverb_geometry', 1)


@functools.lru_cache(maxsize=None)
def _layout(Kt, Ot):
    """The jobs with their signals placed: source blob (0x7FFF fillers between the signals), tap blob, destination offsets."""
    jobs = R.fir_jobs(Kt, Ot)
    src, taps, rows, spos, hpos, dpos = [], [], [], 0, 0, GUARD
    for n, job in enumerate(jobs):
        name, K, count, first, src_len, sp, dp = job
        x, h = R.job_signals(job, n)
        pad = 1 + (spos + 1 + sp) % 2                    # the signal starts at a sample of parity sp
        src.append(np.full(pad, 0x7FFF, np.int16))
        spos += pad
        assert spos % 2 == sp
        dpos += (dpos + dp) % 2 + 2                      # a gap of sentinels before every destination, parity dp
        rows.append((spos, src_len, first, count, hpos, K, dpos))
        src.append(x)
        taps.append(h)
        spos += src_len
        hpos += K
        dpos += count
    src.append(np.full(3, 0x7FFF, np.int16))
    return jobs, np.concatenate(src), np.concatenate(taps), rows, dpos + GUARD


def _call(lib, pcm, taps, rows, out_samples, wav, pcm_out, clip):
    cols = [_longs([r[c] for r in rows] or [0]) for c in range(7)]
    lib.call('re2e_wav_reverb', pcm.data_ptr(), pcm.numel(), taps.data_ptr(), taps.numel(), *cols, len(rows), out_samples,
             wav.data_ptr() if wav is not None else None, pcm_out.data_ptr() if pcm_out is not None else None,
             clip.data_ptr() if clip is not None else None)


def _run(lib, src, taps, rows, total, f32=True, i16=True):
    pcm, tp = torch.from_numpy(src).to(DEV), torch.from_numpy(taps).to(DEV)
    wav = torch.full((total,), float('nan'), device=DEV) if f32 else None
    out = torch.full((total,), SENT, dtype=torch.int16, device=DEV) if i16 else None
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    _call(lib, pcm, tp, rows, total, wav, out, clip)
    torch.cuda.synchronize()
    return {'wav': wav.cpu().numpy() if f32 else None, 'pcm': out.cpu().numpy() if i16 else None, 'clip': int(clip.cpu())}


def _untouched(res, rows, total, tag):
    inside = np.zeros(total, bool)
    for r in rows:
        assert not inside[r[6]:r[6] + r[3]].any()
        inside[r[6]:r[6] + r[3]] = True
    if res['wav'] is not None:
        assert np.isnan(res['wav'][~inside]).all(), '%s: fp32 written outside the destination ranges' % tag
        assert np.isfinite(res['wav'][inside]).all(), '%s: a destination sample was not written' % tag
    if res['pcm'] is not None:
        assert (res['pcm'][~inside] == SENT).all(), '%s: int16 written outside the destination ranges' % tag


@functools.lru_cache(maxsize=None)
def _grid_result():
    _, lib = _ops()
    jobs, src, taps, rows, total = _layout(*_geometry(lib))
    first, second = _run(lib, src, taps, rows, total), _run(lib, src, taps, rows, total)
    return jobs, src, taps, rows, total, first, second


def test_two_runs_bit_equal_and_nothing_else_written():
    jobs, src, taps, rows, total, first, second = _grid_result()
    assert len(rows) > 32 and {r[0] % 2 for r in rows} == {0, 1} and {r[6] % 2 for r in rows} == {0, 1}
    assert np.array_equal(first['wav'].view(np.int32), second['wav'].view(np.int32)) and np.array_equal(first['pcm'], second['pcm'])
    assert first['clip'] == second['clip']
    _untouched(first, rows, total, 'grid')


def test_jobs_against_float64():
    """Every job of the grid: the fp32 output within the derived bound, the fp32 restatement on the CPU within it too, the int16 rules, and
    the clip count of the whole call."""
    jobs, src, taps, rows, total, res, _ = _grid_result()
    clips = 0
    for job, (so, sl, first, count, ho, K, do) in zip(jobs, rows):
        x, h = src[so:so + sl], taps[ho:ho + K]
        got = res['wav'][do:do + count]
        print('ERR %-22s hip %.3f of the bound, fp32-cpu %.3f' % (job[0], R.fir_ratio(got, x, h, first, count),
                                                               R.fir_ratio(R.fir(x, h, first, count, np.float32), x, h, first, count)))
        assert R.fir_violations(R.fir(x, h, first, count, np.float32), x, h, first, count) == [], job[0]
        assert R.fir_violations(got, x, h, first, count) == [], job[0]
        assert R.pcm_violations(res['pcm'][do:do + count], got, x, h, first, count) == [], job[0]
        clips += R.clipped(got)
    assert res['clip'] == clips


def test_unit_impulse_copies_the_source():
    """h = [1.0]: the fp32 and the int16 outputs are the source bit for bit, at every first."""
    _, lib = _ops()
    Kt, Ot = _geometry(lib)
    x = R.signal(Ot + 2100, 7, sigma=9000)
    src = np.concatenate([np.full(1, 0x7FFF, np.int16), x])
    rows = [(1, x.shape[0], 0, x.shape[0], 0, 1, GUARD + 1), (1, x.shape[0], 1023, Ot + 1, 0, 1, GUARD + 2 + x.shape[0])]
    total = rows[1][6] + rows[1][3] + GUARD
    res = _run(lib, src, np.ones(1, np.float32), rows, total)
    for (so, sl, first, count, ho, K, do) in rows:
        assert np.array_equal(res['pcm'][do:do + count], x[first:first + count])
        assert np.array_equal(res['wav'][do:do + count], x[first:first + count].astype(np.float32))
    assert res['clip'] == 0
    _untouched(res, rows, total, 'unit impulse')


def test_saturation_of_both_signs_is_counted():
    _, lib = _ops()
    x = R.signal(3000, 11, sigma=9000)
    x[99:102], x[199:202] = (0, 32767, 32767), (0, -32768, -32768)
    h = np.array([1.0, 1.0, 0.5], np.float32)              # y[101] = 65534, y[201] = -65536; halves: exact in fp32
    rows = [(0, 3000, 0, 3000, 0, 3, GUARD)]
    res = _run(lib, x, h, rows, 3000 + 2 * GUARD)
    y = R.fir(x, h, 0, 3000)
    got = res['pcm'][GUARD:GUARD + 3000]
    assert np.array_equal(res['wav'][GUARD:GUARD + 3000].astype(np.float64), y)          # halves and integers below 2^24: exact
    assert np.array_equal(got, R.to_pcm(y))
    assert (got == 32767).any() and (got == -32768).any() and (y > 32767.5).any() and (y < -32768.5).any()
    assert res['clip'] == R.clipped(y) > 2


def test_each_optional_output_absent_in_turn():
    _, lib = _ops()
    Kt, Ot = _geometry(lib)
    jobs, src, taps, rows, total = _layout(Kt, Ot)
    pick = [i for i, j in enumerate(jobs) if j[2] <= 1024][:6]
    rows = [rows[i] for i in pick]
    both = _run(lib, src, taps, rows, total)
    only_f, only_i = _run(lib, src, taps, rows, total, i16=False), _run(lib, src, taps, rows, total, f32=False)
    assert np.array_equal(only_f['wav'].view(np.int32), both['wav'].view(np.int32)) and only_f['clip'] == 0
    assert np.array_equal(only_i['pcm'], both['pcm']) and only_i['clip'] == both['clip']
    _untouched(only_f, rows, total, 'fp32 only')
    _untouched(only_i, rows, total, 'int16 only')
    pcm, tp = torch.from_numpy(src).to(DEV), torch.from_numpy(taps).to(DEV)              # no counter: accepted
    out = torch.full((total,), SENT, dtype=torch.int16, device=DEV)
    _call(lib, pcm, tp, rows, total, None, out, None)
    assert np.array_equal(out.cpu().numpy(), both['pcm'])


def test_in_place_behind_the_samples():
    """pcm_out == pcm: accepted when the destinations are disjoint from every source range of the call, refused on overlap."""
    _, lib = _ops()
    x0, x1 = R.signal(1500, 21), R.signal(901, 22)
    h = np.concatenate([R.rir(33, 1), R.rir(300, 2)])
    used = 1 + 1500 + 901
    blob = np.full(used + 1500 + 901 + 5, SENT, np.int16)
    blob[1:1501], blob[1501:used] = x0, x1
    rows = [(1, 1500, 0, 1500, 0, 33, used + 1), (1501, 901, 0, 901, 33, 300, used + 1 + 1500 + 1)]
    want = R.run_jobs(blob.copy(), h, rows)
    dev, tp = torch.from_numpy(blob).to(DEV), torch.from_numpy(h).to(DEV)
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    _call(lib, dev, tp, rows, dev.numel(), None, dev, clip)
    got = dev.cpu().numpy()
    d = got.astype(np.int64) - want.astype(np.int64)
    assert np.array_equal(got[:used + 1], blob[:used + 1]) and got[used + 1501] == SENT and (got[-3:] == SENT).all()
    assert np.abs(d).max() <= 1
    for (so, sl, first, count, ho, K, do) in rows:
        assert R.pcm_violations(got[do:do + count], None, blob[so:so + sl], h[ho:ho + K], first, count) == []
    before = dev.clone()
    for bad in ([(1, 1500, 0, 1500, 0, 33, 1400)],                                      # onto its own source
                [rows[0], (1501, 901, 0, 901, 33, 300, 700)],                            # onto the other job's source
                [(1, 1500, 100, 50, 0, 33, 1)]):                                         # onto a part of the source it does not read
        with pytest.raises(lib.Re2eError) as e:
            _call(lib, dev, tp, bad, dev.numel(), None, dev, clip)
        assert 'overlaps' in str(e.value)
    assert torch.equal(dev, before)


def test_refusals_write_nothing():
    """Every refusal of the header comment, each with a word of its message; the outputs keep their NaN / sentinel."""
    _, lib = _ops()
    pcm = torch.zeros(5000, dtype=torch.int16, device=DEV)
    tp = torch.ones(40000, device=DEV)
    wav = torch.full((4000,), float('nan'), device=DEV)
    out = torch.full((4000,), SENT, dtype=torch.int16, device=DEV)
    ok = (0, 1000, 0, 1000, 0, 10, 0)

    def job(**kw):
        names = ('src_off', 'src_len', 'first', 'count', 'rir_off', 'rir_len', 'dst_off')
        return [tuple(kw.get(n, v) for n, v in zip(names, ok))]
    cases = [
        ('beyond src_len', job(first=1, count=1000)),
        ('beyond src_len', job(first=1001, count=1)),
        ('RE2E_WAV_RIR_MAX', job(rir_len=0)),
        ('RE2E_WAV_RIR_MAX', job(rir_len=32769)),
        ('first < 0', job(first=-1)),
        ('count < 1', job(count=0)),
        ('pcm_samples', job(src_off=4001)),
        ('pcm_samples', job(src_off=-1)),
        ('rir_floats', job(rir_off=39991)),
        ('rir_floats', job(rir_off=-1)),
        ('out_samples', job(dst_off=3001)),
        ('out_samples', job(dst_off=-1)),
    ]
    for word, rows in cases:
        with pytest.raises(lib.Re2eError) as e:
            _call(lib, pcm, tp, rows, 4000, wav, out, None)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(lib.Re2eError) as e:
        _call(lib, pcm, tp, job(), 4000, None, None, None)
    assert 'both NULL' in str(e.value)
    with pytest.raises(lib.Re2eError) as e:
        _call(lib, pcm, tp, [], 4000, wav, out, None)
    assert 'n_jobs' in str(e.value)
    with pytest.raises(lib.Re2eError) as e:          # a good job followed by a bad one: nothing of the first is launched either
        _call(lib, pcm, tp, job() + job(rir_len=0), 4000, wav, out, None)
    torch.cuda.synchronize()
    assert torch.isnan(wav).all() and (out == SENT).all(), 'a refused call wrote an output'
    _call(lib, pcm, tp, job(rir_len=32768), 4000, wav, out, None)          # the longest filter is taken
    torch.cuda.synchronize()
    assert (wav[:1000] == 0).all() and torch.isnan(wav[1000:]).all()
