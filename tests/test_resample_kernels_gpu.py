"""csrc/resample.hip (re2e_wav_resample) against the float64 restatement of tests/refs64_resample.py, through the C ABI (lib.call).  Outputs
sit between guards inside one allocation (NaN for fp32, the sentinel 0x5A5A for int16) and every sample outside the destination ranges must
come back untouched; sources and destinations start at odd and even samples (the word-wide and the narrow loads and stores); each call runs
twice on fresh buffers and the second result must equal the first bit for bit.

The bound is derived (refs64_resample): |y - y64| <= (N + 4) 2^-24 sum_j |h[.] x[j]| per output, N = ceil((2 half + 1) / up); the int16 output
is saturate(rintf(.)) of the fp32 output exactly, within 1 of the rounded float64 value, and differs only where that value is within the
bound of a half-integer.  The jobs (refs64_resample.grid_jobs) are the ratios 10/9, 10/11, 20/21, 2/1, 1/2, 3/2, 63/64, 64/63 at resampled
lengths of 1, 2, G - 1, G, G + 1, 2 G + 1 (G: outputs per workgroup, asked of the library) with impulses at the first, a middle and the
last sample, a constant, noise at 0.3 of full scale and full-scale noise; sub-range jobs whose ends fall on tile edges and mid-tile; and
1/64 and 1/16, whose input span a workgroup stages in parts.  They go out as calls of 1, J and J + 1 jobs (J: jobs per launch), ratios mixed
within a call.  GPU only; the float64 references are taken once."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import refs64_resample as R
from test_loss_kernels_gpu import DEV, _ops

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
GUARD = 64


def _arr(ctype, v):
    return (ctype * max(len(v), 1))(*[int(x) for x in v])


def _geometry(lib):
    return lib.query('re2e_wav_resample_geometry', 0), lib.query('re2e_wav_resample_geometry', 1)


@functools.lru_cache(maxsize=None)
def _layout(G):
    """The jobs with their signals placed: source blob (0x7FFF fillers between the signals), rows, destination size, references."""
    jobs = R.grid_jobs(G)
    src, rows, refs, spos, dpos = [], [], [], 0, GUARD
    for n, job in enumerate(jobs):
        name, up, down, L, first, count, kind, sp, dp = job
        x = R.job_signal(job, n)
        pad = 1 + (spos + 1 + sp) % 2                    # the signal starts at a sample of parity sp
        src.append(np.full(pad, 0x7FFF, np.int16))
        spos += pad
        assert spos % 2 == sp
        dpos += (dpos + dp) % 2 + 2                      # a gap of sentinels before every destination, parity dp
        rows.append((spos, L, up, down, first, count, dpos))
        refs.append((R.job(x, up, down, first, count), R.bound(x, up, down, first, count)))
        src.append(x)
        spos += L
        dpos += count
    src.append(np.full(3, 0x7FFF, np.int16))
    return jobs, np.concatenate(src), rows, dpos + GUARD, refs


def _call(lib, pcm, rows, out_samples, wav, pcm_out, clip):
    types = (ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_long)
    cols = [_arr(t, [r[c] for r in rows]) for c, t in enumerate(types)]
    lib.call('re2e_wav_resample', pcm.data_ptr(), pcm.numel(), *cols, len(rows), out_samples,
             wav.data_ptr() if wav is not None else None, pcm_out.data_ptr() if pcm_out is not None else None,
             clip.data_ptr() if clip is not None else None)


def _run(lib, src, calls, total, f32=True, i16=True):
    """``calls``: lists of rows, one re2e_wav_resample call each, into the same outputs."""
    pcm = torch.from_numpy(src).to(DEV)
    wav = torch.full((total,), float('nan'), device=DEV) if f32 else None
    out = torch.full((total,), SENT, dtype=torch.int16, device=DEV) if i16 else None
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    for rows in calls:
        _call(lib, pcm, rows, total, wav, out, clip)
    torch.cuda.synchronize()
    assert np.array_equal(pcm.cpu().numpy(), src), 'the source blob was written'
    return {'wav': wav.cpu().numpy() if f32 else None, 'pcm': out.cpu().numpy() if i16 else None, 'clip': int(clip.cpu())}


def _untouched(res, rows, total, tag):
    inside = np.zeros(total, bool)
    for r in rows:
        assert not inside[r[6]:r[6] + r[5]].any()
        inside[r[6]:r[6] + r[5]] = True
    if res['wav'] is not None:
        assert np.isnan(res['wav'][~inside]).all(), '%s: fp32 written outside the destination ranges' % tag
        assert np.isfinite(res['wav'][inside]).all(), '%s: a destination sample was not written' % tag
    if res['pcm'] is not None:
        assert (res['pcm'][~inside] == SENT).all(), '%s: int16 written outside the destination ranges' % tag


def _split(rows, J):
    """Calls of 1, J and J + 1 jobs."""
    assert len(rows) == 2 * J + 2
    return [rows[:1], rows[1:1 + J], rows[1 + J:]]


@functools.lru_cache(maxsize=None)
def _grid_result():
    _, lib = _ops()
    G, J = _geometry(lib)
    jobs, src, rows, total, refs = _layout(G)
    calls = _split(rows, J)
    first, second = _run(lib, src, calls, total), _run(lib, src, calls, total)
    return jobs, src, rows, total, refs, first, second


def test_two_runs_bit_equal_and_nothing_else_written():
    jobs, src, rows, total, refs, first, second = _grid_result()
    assert {r[0] % 2 for r in rows} == {0, 1} and {r[6] % 2 for r in rows} == {0, 1}
    assert len({(r[2], r[3]) for r in rows[1:34]}) > 4                      # ratios mixed within one call
    assert np.array_equal(first['wav'].view(np.int32), second['wav'].view(np.int32)) and np.array_equal(first['pcm'], second['pcm'])
    assert first['clip'] == second['clip']
    _untouched(first, rows, total, 'grid')


def test_jobs_against_float64():
    """Every job of the grid: the fp32 output within the derived bound, the int16 rules, and the clip count of the three calls together,
    which equals the reference's (tests/test_refs64_resample_cpu.py: no float64 value within the bound of a threshold)."""
    jobs, src, rows, total, refs, res, _ = _grid_result()
    clips = 0
    for job, (so, L, up, down, first, count, do), (ref, bnd) in zip(jobs, rows, refs):
        got = res['wav'][do:do + count]
        print('ERR %-34s hip %.3f of the bound' % (job[0], R.ratio(got, ref, bnd)))
        assert R.violations(got, ref, bnd) == [], job[0]
        assert R.pcm_violations(res['pcm'][do:do + count], got, ref, bnd) == [], job[0]
        if job[6] != 'noise_full':
            assert R.clipped(got) == 0, job[0]
        clips += R.clipped(ref)
    assert res['clip'] == clips > 50


def test_impulses_read_the_table_out():
    """An impulse of 20000 at sample p: y[m] = 20000 h[half + m down - p up] EXACTLY (one product, exact zeros), phase by phase."""
    jobs, src, rows, total, refs, res, _ = _grid_result()
    _, lib = _ops()
    n = 0
    for job, (so, L, up, down, first, count, do) in zip(jobs, rows):
        if not job[6].startswith('impulse'):
            continue
        h, half = lib.resample_taps(up, down)
        p, amp = {'impulse_first': (0, 20000), 'impulse_mid': (L // 2, -20000), 'impulse_last': (L - 1, 20000)}[job[6]]
        idx = half + np.arange(first, first + count) * down - p * up
        ok = (idx >= 0) & (idx <= 2 * half)
        want = np.where(ok, np.float32(amp) * h[np.clip(idx, 0, 2 * half)], np.float32(0)).astype(np.float32)
        assert np.array_equal(res['wav'][do:do + count], want), job[0]
        n += 1
    assert n >= 20


def test_table_call():
    _, lib = _ops()
    for up, down in R.RATIOS + R.WIDE_RATIOS:
        h, half = lib.resample_taps(up, down)
        assert half == R.table(up, down)[1] and R.table_violations(h, up, down) == []


def test_each_optional_output_absent_in_turn():
    _, lib = _ops()
    G, J = _geometry(lib)
    jobs, src, rows, total, refs = _layout(G)
    pick = [i for i, j in enumerate(jobs) if j[6] == 'noise_full' and j[5] > 1][:8]
    rows = [rows[i] for i in pick]
    assert {r[6] % 2 for r in rows} == {0, 1}
    both = _run(lib, src, [rows], total)
    only_f, only_i = _run(lib, src, [rows], total, i16=False), _run(lib, src, [rows], total, f32=False)
    assert np.array_equal(only_f['wav'].view(np.int32), both['wav'].view(np.int32)) and only_f['clip'] == 0
    assert np.array_equal(only_i['pcm'], both['pcm']) and only_i['clip'] == both['clip'] > 0
    _untouched(only_f, rows, total, 'fp32 only')
    _untouched(only_i, rows, total, 'int16 only')
    pcm = torch.from_numpy(src).to(DEV)                                              # no counter: accepted
    out = torch.full((total,), SENT, dtype=torch.int16, device=DEV)
    _call(lib, pcm, rows, total, None, out, None)
    assert np.array_equal(out.cpu().numpy(), both['pcm'])


def test_in_place_behind_the_samples():
    """pcm_out == pcm: accepted when the destinations are disjoint from every source range of the call, refused on overlap."""
    _, lib = _ops()
    x0, x1 = R.signal('noise_0.3', 1500, 21), R.signal('noise_full', 901, 22)
    n0, n1 = R.out_len(1500, 10, 9), R.out_len(901, 10, 11)
    used = 1 + 1500 + 901
    blob = np.full(used + n0 + n1 + 5, SENT, np.int16)
    blob[1:1501], blob[1501:used] = x0, x1
    rows = [(1, 1500, 10, 9, 0, n0, used + 1), (1501, 901, 10, 11, 0, n1, used + 1 + n0 + 1)]
    want = R.run_jobs(blob.copy(), rows)
    dev = torch.from_numpy(blob).to(DEV)
    clip = torch.zeros(1, dtype=torch.int32, device=DEV)
    _call(lib, dev, rows, dev.numel(), None, dev, clip)
    got = dev.cpu().numpy()
    d = got.astype(np.int64) - want.astype(np.int64)
    assert np.array_equal(got[:used + 1], blob[:used + 1]) and got[used + 1 + n0] == SENT and (got[-3:] == SENT).all()
    assert np.abs(d).max() <= 1
    for (so, L, up, down, first, count, do) in rows:
        x = blob[so:so + L]
        assert R.pcm_violations(got[do:do + count], None, R.job(x, up, down, first, count), R.bound(x, up, down, first, count)) == []
    before = dev.clone()
    for bad in ([(1, 1500, 10, 9, 0, n0, 1400)],                                         # onto its own source
                [rows[0], (1501, 901, 10, 11, 0, n1, 700)],                              # onto the other job's source
                [(1, 1500, 10, 9, 100, 50, 1)]):                                         # onto a part of the source it does not read
        with pytest.raises(lib.Re2eError) as e:
            _call(lib, dev, bad, dev.numel(), None, dev, clip)
        assert 'overlaps' in str(e.value)
    assert torch.equal(dev, before)


def test_refusals_write_nothing():
    """Every refusal of the header comment, each with a word of its message; the outputs keep their NaN / sentinel."""
    _, lib = _ops()
    pcm = torch.zeros(5000, dtype=torch.int16, device=DEV)
    wav = torch.full((4000,), float('nan'), device=DEV)
    out = torch.full((4000,), SENT, dtype=torch.int16, device=DEV)
    ok = (0, 900, 10, 9, 0, 1000, 0)                      # 900 samples at 10/9: exactly 1000

    def job(**kw):
        names = ('src_off', 'src_len', 'up', 'down', 'first', 'count', 'dst_off')
        return [tuple(kw.get(n, v) for n, v in zip(names, ok))]
    cases = [
        ('up < 1', job(up=0)),
        ('down < 1', job(down=0)),
        ('down < 1', job(down=-9)),
        ('up == down', job(up=9)),
        ('up == down', job(up=1, down=1)),
        ('gcd', job(up=20, down=18)),
        ('RE2E_WAV_RESAMPLE_MAX_RATE', job(up=65, down=64)),
        ('RE2E_WAV_RESAMPLE_MAX_RATE', job(up=1, down=65)),
        ('first < 0', job(first=-1)),
        ('count < 1', job(count=0)),
        ('beyond the resampled length', job(first=1, count=1000)),
        ('beyond the resampled length', job(first=1001, count=1)),
        ('beyond the resampled length', job(src_len=899)),              # L' = 999
        ('pcm_samples', job(src_off=4101)),
        ('pcm_samples', job(src_off=-1)),
        ('source length', job(src_len=0)),
        ('out_samples', job(dst_off=3001)),
        ('out_samples', job(dst_off=-1)),
    ]
    for word, rows in cases:
        with pytest.raises(lib.Re2eError) as e:
            _call(lib, pcm, rows, 4000, wav, out, None)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(lib.Re2eError) as e:
        _call(lib, pcm, job(), 4000, None, None, None)
    assert 'both NULL' in str(e.value)
    with pytest.raises(lib.Re2eError) as e:
        _call(lib, pcm, [], 4000, wav, out, None)
    assert 'n_jobs' in str(e.value)
    with pytest.raises(lib.Re2eError) as e:          # good jobs followed by a bad one beyond the first launch: nothing is launched either
        _call(lib, pcm, job() * 40 + job(up=0), 4000, wav, out, None)
    torch.cuda.synchronize()
    assert torch.isnan(wav).all() and (out == SENT).all(), 'a refused call wrote an output'
    _call(lib, pcm, job(up=64, down=63, src_len=63, count=64), 4000, wav, out, None)          # the largest ratio is taken
    torch.cuda.synchronize()
    assert (wav[:64] == 0).all() and torch.isnan(wav[64:]).all()
