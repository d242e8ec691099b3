"""tests/refs64_reverb.py on the CPU, and the host side of reverberant mixtures: the fp32 restatement stays inside the bounds the kernels
are held to and every named mistake breaks them on the chosen cases; ``reverb_jobs`` reproduces the reference's order (reverberate the
whole noise file, cut, tile, slice) in the three cases of its table and on their boundaries; ``draw_reverb`` is a function of
(seed, epoch, index) on a stream of its own; ``read_rir`` aligns, normalises, cuts and caches; a data set without ``rir_scp`` hands out
the 7-tuples of the commit before reverberation existed."""
import argparse
import functools
import wave

import numpy as np
import pytest

import refs64_reverb as R
import refs64_wav as W
from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.data import wav_io
from robust_e2e_gan_amd.data.mix_data_loader import reverb_jobs
from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset, draw_mixture, draw_reverb


@functools.lru_cache(maxsize=None)
def _jobs():
    import os
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    Kt, Ot = lib.query('re2e_wav_reverb_geometry', 0), lib.query('re2e_wav_reverb_geometry', 1)
    assert Kt >= 64 and Ot >= 1024 and Ot % 1024 == 0
    jobs = R.fir_jobs(Kt, Ot)
    return Kt, Ot, [(j,) + R.job_signals(j, n) for n, j in enumerate(jobs)]


def test_job_grid_covers_every_edge():
    Kt, Ot, jobs = _jobs()
    Ks, counts = {j[1] for j, _, _ in jobs}, {j[2] for j, _, _ in jobs}
    assert {1, 2, 31, 32, 33, Kt - 1, Kt, Kt + 1, 2 * Kt + 5} <= Ks
    assert {1, 31, 1024, Ot - 1, Ot, Ot + 1, 2 * Ot + 7} <= counts
    firsts = {('0' if j[3] == 0 else '1' if j[3] == 1 else 'K-1' if j[3] == j[1] - 1 else 'K' if j[3] == j[1] else 'far' if j[3] > Ot else '?')
              for j, _, _ in jobs if j[1] > 2}
    assert firsts >= {'0', '1', 'K-1', 'K', 'far'}
    assert any(j[4] < j[1] for j, _, _ in jobs)                               # src_len < K
    assert len(jobs) > lib.query('re2e_wav_reverb_geometry', 2)               # more jobs than one launch
    assert {j[5] for j, _, _ in jobs} == {0, 1} and {j[6] for j, _, _ in jobs} == {0, 1}
    assert lib.query('re2e_wav_reverb_geometry', 3) == 32768


def test_fp32_restatement_is_inside_the_bound_and_convolve_is_the_definition():
    _, _, jobs = _jobs()
    for j, x, h in jobs:
        name, K, count, first = j[:4]
        assert R.fir_violations(R.fir(x, h, first, count, np.float32), x, h, first, count, frac=0.5) == [], name
        got = R.to_pcm(R.fir(x, h, first, count, np.float32))
        assert R.pcm_violations(got, R.fir(x, h, first, count, np.float32), x, h, first, count) == [], name
    # np.convolve against the sum it stands for, on one small job
    j, x, h = [t for t in jobs if t[0][1] == 33 and t[0][2] == 31][0]
    first, count = j[3], j[2]
    xs = x.astype(np.float64)
    direct = [sum(float(h[k]) * xs[first + i - k] for k in range(33) if first + i - k >= 0) for i in range(count)]
    assert np.abs(np.array(direct) - R.fir(x, h, first, count)).max() <= 1e-9 * np.abs(direct).max()


@pytest.mark.parametrize('mistake', R.FIR_MISTAKES)
def test_fir_mistakes_break_the_bound(mistake):
    _, _, jobs = _jobs()
    broken = [j[0] for j, x, h in jobs if R.fir_violations(R.fir(x, h, j[3], j[2], mistake=mistake), x, h, j[3], j[2]) != []]
    assert len(broken) >= 5, (mistake, broken)
    if mistake != 'history_not_zero':                  # (a job that starts at first >= K has no history before sample 0 to get wrong)
        assert len(broken) >= len(jobs) // 2, (mistake, broken)


@functools.lru_cache(maxsize=None)
def _mix_refs(name, dtype=np.float64, mistake=None):
    return R.mix_case_refs(name, dtype, mistake)


@pytest.mark.parametrize('name', sorted(R.MIX_CASES))
def test_mixture_fp32_restatement_and_mistakes(name):
    cm = R.mix_case_signals(name)[2]
    r64 = _mix_refs(name)
    outs = ('clean', 'clean_log', 'clean_ang', 'mix', 'mix_log', 'mix_ang', 'cos', 'g')
    for b, (a, r) in enumerate(zip(_mix_refs(name, np.float32), r64)):
        assert W.violations({k: a[k] for k in outs}, r, cm, frac=0.25) == [], (name, b)
    for mistake in R.MIX_MISTAKES:
        wrong = _mix_refs(name, mistake=mistake)
        assert any(W.violations({k: a[k] for k in outs}, r, cm) != [] for a, r in zip(wrong, r64)), (name, mistake)
    # the clean stream is the DRY signal: the reverberant speech does not reach it
    speech = R.mix_case_signals(name)[0]
    for s, r in zip(speech, r64):
        assert np.array_equal(r['clean'], W.features(s)['clean'])


def test_unit_impulse_is_the_plain_mixture():
    """h = [1.0] on both streams: refs64_wav.features itself."""
    speech, nz, cm, _, _ = R.mix_case_signals('wrap700')
    one = np.ones(1, np.float32)
    for b, s in enumerate(speech):
        a = R.features_rev(s, nz, 5 + b, 7.0, one, one, cm)
        r = W.features(s, nz, 5 + b, 7.0, cm)
        assert W.violations({k: a[k] for k in ('clean', 'mix', 'mix_log', 'cos', 'g')}, r, cm, frac=1e-3) == []


# ---- reverb_jobs ------------------------------------------------------------------------------------------------------------------------
def _noise_case(L, N, s0, with_speech_rir=True):
    """One utterance through reverb_jobs and the host model of the kernel -> the samples the mixture reads, against the restatement."""
    s, n = R.signal(L, 3 * L + N), R.signal(N, 5 * N + s0)
    hs, hn = R.rir(33, 1), R.rir(300, 2)
    taps = np.concatenate([hs, hn])
    pos = 1 + L + 2 + N
    blob = np.full(pos + 2 * L + N + 8, 0x5A5A, np.int16)
    blob[1:1 + L], blob[3 + L:3 + L + N] = s, n
    jobs, moff, nz, end = reverb_jobs([(1, L)], [(3 + L, N, s0)], [((0, 33) if with_speech_rir else None, (33, 300))], pos)
    assert end <= blob.shape[0] and all(j[6] >= pos and j[6] + j[3] <= end for j in jobs)
    R.run_jobs(blob, taps, jobs)
    (noff, nlen, start), = nz
    rn = R.reverberant_pcm(hn, n)
    got = W.noise_segment(blob[noff:noff + nlen], start, L)
    assert np.array_equal(got, W.noise_segment(rn, s0, L)), (L, N, s0)
    if s0 < W.s0_range(N, L):                          # a start the reference can draw: its own statement, tile then slice
        assert np.array_equal(got, W.noise_segment_tiled(rn, s0, L)), (L, N, s0)
    want_rs = R.reverberant_pcm(hs, s) if with_speech_rir else s
    assert np.array_equal(blob[moff[0]:moff[0] + L], want_rs)
    return jobs, nz[0]


def test_reverb_jobs_reproduce_the_reference_order():
    # inside the file: one job, the new file is the segment
    jobs, (noff, nlen, start) = _noise_case(500, 2000, 700)
    assert [(j[2], j[3]) for j in jobs] == [(0, 500), (700, 500)] and (nlen, start) == (500, 0)
    # s0 + L == N: still one job
    jobs, nz = _noise_case(500, 2000, 1500)
    assert [(j[2], j[3]) for j in jobs][1:] == [(1500, 500)] and nz[1:] == (500, 0)
    # wraps once: two jobs to consecutive destinations
    jobs, nz = _noise_case(500, 2000, 1501)
    assert [(j[2], j[3]) for j in jobs][1:] == [(1501, 499), (0, 1)] and jobs[2][6] == jobs[1][6] + 499 and nz[1:] == (500, 0)
    # L == N: start 0 is one job, any other start wraps once
    jobs, nz = _noise_case(600, 600, 0)
    assert [(j[2], j[3]) for j in jobs][1:] == [(0, 600)] and nz[1:] == (600, 0)
    jobs, nz = _noise_case(600, 600, 599)
    assert [(j[2], j[3]) for j in jobs][1:] == [(599, 1), (0, 599)] and nz[1:] == (600, 0)
    # L > N: the whole file once, the start is kept
    jobs, nz = _noise_case(1279, 600, 0)
    assert [(j[2], j[3]) for j in jobs][1:] == [(0, 600)] and nz[1:] == (600, 0)
    jobs, nz = _noise_case(1279, 600, 577)
    assert [(j[2], j[3]) for j in jobs][1:] == [(0, 600)] and nz[1:] == (600, 577)
    jobs, nz = _noise_case(601, 600, 3, with_speech_rir=False)
    assert [(j[2], j[3]) for j in jobs] == [(0, 600)] and nz[1:] == (600, 3)


def test_reverb_jobs_without_impulse_responses_change_nothing():
    jobs, moff, nz, end = reverb_jobs([(0, 300), (300, 400)], [(700, 100, 5), (700, 100, 7)], [(None, None), ((0, 4), None)], 800)
    assert jobs == [(300, 400, 0, 400, 0, 4, 800)] and moff == [0, 800] and nz == [(700, 100, 5), (700, 100, 7)] and end == 1200


# ---- draws ------------------------------------------------------------------------------------------------------------------------------
def test_draw_reverb_is_a_function_of_seed_epoch_and_index():
    first = [draw_reverb(11, 0, i, 5, 1.0) for i in range(40)]
    assert first == [draw_reverb(11, 0, i, 5, 1.0) for i in range(40)]
    assert all(a is not None and b is not None and 0 <= a < 5 and 0 <= b < 5 for a, b in first)
    assert {a for a, _ in first} == set(range(5)) and any(a != b for a, b in first)          # both drawn, independently
    assert first != [draw_reverb(11, 1, i, 5, 1.0) for i in range(40)] and first != [draw_reverb(12, 0, i, 5, 1.0) for i in range(40)]
    assert all(draw_reverb(11, e, i, 5, 0.0) == (None, None) for e in range(3) for i in range(40))
    half = [draw_reverb(11, 0, i, 5, 0.5) for i in range(400)]
    n = sum(a is not None for a, _ in half)
    assert 150 <= n <= 250 and all((a is None) == (b is None) for a, b in half)
    assert draw_reverb(11, 0, 0, 0, 1.0) == (None, None)


# draw_mixture(11, epoch, i, [100, 5000], L_i) of the commit before reverberation existed, L = 1279, 257, 2303, 40000 in turn
_PARENT_DRAWS = [(0, 2, 9.9855572488023), (0, 16, 2.493816229942998), (0, 37, 12.990240578871603), (1, 0, 1.6555899598688062),
                 (0, 13, 4.789144038588069), (1, 2765, 19.376089416379507), (0, 9, 0.9874009139049811), (0, 0, 19.54243416606409),
                 (0, 5, 3.8564645838690814), (1, 1571, 18.793031116398602), (1, 2125, 5.354949765437153), (1, 0, 9.068905724365777)]
_PARENT_DRAWS_E3 = [(0, 19, 16.9797852041011), (0, 29, 18.984673102151312), (1, 1566, 4.3874894415199694), (0, 0, 14.650024146263645)]
_LENS = {'uttA': 1279, 'uttB': 257, 'uttC': 2303, 'uttD': 40000}
_NOISE = {'n1': 100, 'n2': 5000}


def test_draw_mixture_is_what_it_was():
    lens = list(_LENS.values())
    assert [draw_mixture(11, 0, i, [100, 5000], lens[i % 4]) for i in range(12)] == _PARENT_DRAWS
    assert [draw_mixture(11, 3, i, [100, 5000], lens[i % 4]) for i in range(4)] == _PARENT_DRAWS_E3


def _corpus(tmp_path, **extra):
    rng = np.random.RandomState(3)
    sig = {}
    for name, n in list(_LENS.items()) + list(_NOISE.items()):
        sig[name] = rng.randint(-20000, 20000, n).astype(np.int16)
        wav_io.write_wav(str(tmp_path / (name + '.wav')), sig[name])
    (tmp_path / 'clean_wav.scp').write_text(''.join('%s %s\n' % (u, tmp_path / (u + '.wav')) for u in _LENS))
    (tmp_path / 'noise.scp').write_text(''.join('%s\n' % (tmp_path / (n + '.wav')) for n in _NOISE))
    (tmp_path / 'utt2spk').write_text(''.join('%s spk%s\n' % (u, u[-1]) for u in _LENS))
    (tmp_path / 'text_char').write_text(''.join('%s a b %s\n' % (u, 'c' * (i + 1)) for i, u in enumerate(_LENS)))
    (tmp_path / 'dict').write_text('a 1\nb 2\nc 3\n')
    args = argparse.Namespace(noise_repeat_num=3, seed=11, normalize_type=0, model_unit='char', **extra)
    return sig, MixWavDataset(args, str(tmp_path), str(tmp_path / 'dict'))


def _rir_files(tmp_path):
    a = np.zeros(400)
    a[7], a[8:400] = -0.5, 0.1 * np.random.RandomState(1).randn(392) * np.exp(-np.arange(392) / 80.0)
    np.save(str(tmp_path / 'r0.npy'), a)
    b = np.zeros(50, np.int16)
    b[3], b[4], b[20] = 16384, 8192, -4096
    wav_io.write_wav(str(tmp_path / 'r1.wav'), b)
    (tmp_path / 'rir.scp').write_text('room0 %s\n%s\n' % (tmp_path / 'r0.npy', tmp_path / 'r1.wav'))
    return a, b


def test_dataset_without_rir_scp_hands_out_the_parent_tuples(tmp_path):
    sig, ds = _corpus(tmp_path)
    utts, noises = list(_LENS), list(_NOISE)
    for i in range(len(ds)):
        it = ds[i]
        ni, start, db = _PARENT_DRAWS[i]
        k, u = divmod(i, 4)
        assert len(it) == 7 and it[0] == '%s__mix%d' % (utts[u], k) and it[1] == 'spk' + utts[u][-1]
        assert np.array_equal(it[2], sig[utts[u]]) and np.array_equal(it[3], sig[noises[ni]])
        assert it[4] == start % _NOISE[noises[ni]] and it[5] == db and it[6] == [1, 2] + [3] * (u + 1)


def test_dataset_with_rir_scp_appends_the_impulse_responses(tmp_path):
    a, b = _rir_files(tmp_path)
    sig, ds = _corpus(tmp_path, rir_scp=str(tmp_path / 'rir.scp'), rir_max_taps=100)
    assert ds.reverb_prob == 1.0 and len(ds.rir_paths) == 2
    seen = set()
    for i in range(len(ds)):
        it = ds[i]
        assert len(it) == 8 and (it[4], it[5]) == (_PARENT_DRAWS[i][1] % it[3].shape[0], _PARENT_DRAWS[i][2])          # the mixture draws stay
        hs, hn = it[7]
        rs, rn = ds.draw_rirs(i)
        assert hs is ds.rir(rs) and hn is ds.rir(rn) and hs.dtype == np.float32 and hs.shape[0] <= 100 and hs[0] == 1.0
        seen.add((rs, rn))
    assert len(seen) >= 3
    ds.set_epoch(1)
    assert [ds.draw_rirs(i) for i in range(len(ds))] != [ds.draw_rirs(i, epoch=0) for i in range(len(ds))]
    _, never = _corpus(tmp_path, rir_scp=str(tmp_path / 'rir.scp'), reverb_prob=0.0)
    assert all(never[i][7] == (None, None) for i in range(len(never)))


# ---- read_rir ---------------------------------------------------------------------------------------------------------------------------
def test_read_rir_aligns_normalises_cuts_and_caches(tmp_path):
    a, b = _rir_files(tmp_path)
    h = wav_io.read_rir(str(tmp_path / 'r0.npy'))
    assert h.dtype == np.float32 and h.shape == (393,) and h[0] == 1.0                    # starts at the largest tap (index 7, negative)
    assert np.array_equal(h, (a[7:] / a[7]).astype(np.float32))
    assert wav_io.read_rir(str(tmp_path / 'r0.npy')) is h                                 # one object per file
    cut = wav_io.read_rir(str(tmp_path / 'r0.npy'), max_taps=10)
    assert cut.shape == (10,) and np.array_equal(cut, h[:10])
    w = wav_io.read_rir(str(tmp_path / 'r1.wav'))
    assert w.shape == (47,) and w[0] == 1.0 and w[1] == 0.5 and w[17] == -0.25 and wav_io.read_rir(str(tmp_path / 'r1.wav')) is w


def test_read_rir_refuses_by_name(tmp_path):
    def _write(path, data, channels=1, rate=16000):
        f = wave.open(str(path), 'wb')
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(data)
        f.close()
    _write(tmp_path / 'stereo.wav', b'\x01\x00' * 64, channels=2)
    _write(tmp_path / 'eight_khz.wav', b'\x01\x00' * 64, rate=8000)
    np.save(str(tmp_path / 'matrix.npy'), np.ones((4, 2)))
    np.save(str(tmp_path / 'zeros.npy'), np.zeros(9))
    (tmp_path / 'text.npy').write_text('no array')
    for name in ('stereo.wav', 'eight_khz.wav', 'matrix.npy', 'zeros.npy', 'text.npy'):
        with pytest.raises(wav_io.WavError) as e:
            wav_io.read_rir(str(tmp_path / name))
        assert name in str(e.value)
