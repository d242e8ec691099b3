"""tests/refs64_resample.py on the CPU, and the host side of speed perturbation: the written-out sum is scipy.signal.resample_poly; the fp32
restatement stays inside a quarter of the bound the kernel is held to and every named mistake breaks it (``length_floor``: the length
check) on the GPU test's own inputs; the saturating inputs keep clear of the thresholds by more than the bound, so the clip counts can be
compared; the library's table; ``resample_jobs``; ``draw_speed`` is a function of (seed, epoch, index) on a stream of its own and a data
set without ``speed_perturb`` hands out what it handed out."""
import functools
import os

import numpy as np
import pytest

import refs64_resample as R
from robust_e2e_gan_amd import lib
from robust_e2e_gan_amd.data import wav_io
from robust_e2e_gan_amd.data.mix_data_loader import WAV_RESAMPLE_MAX_RATE, resample_jobs, resampled_len, reverb_jobs, speed_ratio
from robust_e2e_gan_amd.data.wav_dataset import draw_mixture, draw_speed
from test_refs64_reverb_cpu import _LENS, _NOISE, _PARENT_DRAWS, _corpus, _rir_files


def _built():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib


@functools.lru_cache(maxsize=None)
def _grid():
    """[(job, x, float64 outputs, bound)] of the GPU test's grid."""
    G = _built().query('re2e_wav_resample_geometry', 0)
    assert G >= 256 and G % 64 == 0
    out = []
    for n, j in enumerate(R.grid_jobs(G)):
        x = R.job_signal(j, n)
        out.append((j, x, R.job(x, j[1], j[2], j[4], j[5]), R.bound(x, j[1], j[2], j[4], j[5])))
    return G, out


def test_geometry_and_grid_cover_every_edge():
    G, grid = _grid()
    J = lib.query('re2e_wav_resample_geometry', 1)
    assert lib.query('re2e_wav_resample_geometry', 2) == WAV_RESAMPLE_MAX_RATE == 64 and lib.query('re2e_wav_resample_geometry', 3) == -1
    jobs = [g[0] for g in grid]
    assert len(jobs) == 1 + J + (J + 1), 'the grid goes out as calls of 1, J and J + 1 jobs'
    assert {(j[1], j[2]) for j in jobs} == set(R.RATIOS) | set(R.WIDE_RATIOS)
    full = [j for j in jobs if j[4] == 0 and j[5] == R.out_len(j[3], j[1], j[2])]
    assert {j[5] for j in full} >= {1, 2, G - 1, G, G + 1, 2 * G + 1} and any(j[3] == 1 for j in full)
    for up, down in R.RATIOS:
        assert {j[6] for j in jobs if (j[1], j[2]) == (up, down)} == set(R.KINDS), 'every ratio meets every kind of input'
    sub = [j for j in jobs if not (j[4] == 0 and j[5] == R.out_len(j[3], j[1], j[2]))]
    assert len(sub) == 16 and any(j[4] % G == 0 and (j[4] + j[5]) % G == 0 for j in sub) and any(j[4] % G and (j[4] + j[5]) % G for j in sub)
    assert {j[7] for j in jobs} == {0, 1} and {j[8] for j in jobs} == {0, 1}


@pytest.mark.parametrize('up,down', [(10, 9), (10, 11), (20, 21), (2, 1), (1, 2), (3, 2)])
def test_written_out_sum_is_resample_poly(up, down):
    signal = pytest.importorskip('scipy.signal')
    rng = np.random.RandomState(up * 100 + down)
    for L in (1, 2, 3, 17, 100, 299, 300):
        x = rng.randn(L)
        want = signal.resample_poly(x, up, down)
        got = R.resample(x, up, down)
        assert got.shape == want.shape, (up, down, L)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (up, down, L)


def test_fp32_restatement_holds_a_quarter_of_the_bound():
    _, grid = _grid()
    for j, x, ref, bnd in grid:
        y32 = R.job(x, j[1], j[2], j[4], j[5], np.float32)
        assert R.violations(y32, ref, bnd, frac=0.25) == [], j[0]
        assert R.pcm_violations(R.to_pcm(y32), y32, ref, bnd) == [], j[0]


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_mistakes_break_the_bound(mistake):
    _, grid = _grid()
    if mistake == 'length_floor':                       # only the length changes: the length check has to catch it
        short = [j[0] for j, x, ref, bnd in grid if R.out_len(j[3], j[1], j[2], mistake) != R.out_len(j[3], j[1], j[2])]
        assert len(short) >= len(grid) // 2, short
        j, x, ref, bnd = [g for g in grid if g[0][0] in short and g[0][4] == 0][0]
        assert R.violations(R.resample(x, j[1], j[2], mistake=mistake), ref, bnd) != []
        return
    broken = [j[0] for j, x, ref, bnd in grid if R.violations(R.job(x, j[1], j[2], j[4], j[5], mistake=mistake), ref, bnd) != []]
    assert len(broken) >= len(grid) // 2, (mistake, len(broken))
    for up, down in R.RATIOS:       # ... at every ratio (time_reversed: with up <= 2 every phase is its own negative; gain_missing: up = 1 is no gain)
        if (mistake == 'time_reversed' and up <= 2) or (mistake == 'gain_missing' and up == 1):
            continue
        assert any(b.startswith('%d_%d_' % (up, down)) for b in broken), (mistake, up, down)


def test_saturating_inputs_keep_clear_of_the_thresholds():
    _, grid = _grid()
    n = 0
    for j, x, ref, bnd in grid:
        if j[6] != 'noise_full':
            assert R.clipped(ref) == 0 and np.abs(ref).max() + bnd.max() < 32767, j[0]
            continue
        assert (np.abs(ref - 32767.5) > bnd).all() and (np.abs(ref + 32768.5) > bnd).all(), j[0]
        n += R.clipped(ref)
    assert n > 50


def test_library_table():
    _built()
    for up, down in R.RATIOS + R.WIDE_RATIOS + ((64, 1), (5, 3)):
        h, half = lib.resample_taps(up, down)
        assert half == 10 * max(up, down) == R.table(up, down)[1]
        assert R.table_violations(h, up, down) == []
        wrong = R.table(up, down, 'hann_window')[0].astype(np.float32)
        assert R.table_violations(wrong, up, down) != []
    for up, down, word in ((0, 3, 'up < 1'), (3, 0, 'down < 1'), (3, 3, 'up == down'), (4, 6, 'gcd'), (65, 64, 'MAX_RATE'), (1, 65, 'MAX_RATE')):
        with pytest.raises(lib.Re2eError) as e:
            lib.resample_taps(up, down)
        assert word in str(e.value)


# ---- resample_jobs ----------------------------------------------------------------------------------------------------------------------------------
def test_speed_ratio():
    assert speed_ratio('0.9') == (10, 9) and speed_ratio('1.1') == (10, 11) and speed_ratio('0.95') == (20, 19) and speed_ratio('1.05') == (20, 21)
    assert speed_ratio('1.0') is None and speed_ratio('1') is None and speed_ratio(' 2 ') == (1, 2) and speed_ratio('0.5') == (2, 1)
    for bad in ('', '-0.9', '0', '0.0', 'fast', '1e-1', '0.9x', '9/10'):
        with pytest.raises(ValueError) as e:
            speed_ratio(bad)
        assert 'positive decimal' in str(e.value)
    for bad in ('0.99', '65', '0.015'):
        with pytest.raises(ValueError) as e:
            speed_ratio(bad)
        assert 'RE2E_WAV_RESAMPLE_MAX_RATE' in str(e.value)


def test_resample_jobs_arithmetic():
    speech = [(0, 1000), (1000, 999), (1999, 257), (2256, 10)]
    jobs, moved, end = resample_jobs(speech, [(10, 9), None, (10, 11), (1, 1)], 3000)
    assert jobs == [(0, 1000, 10, 9, 0, 1112, 3000), (1999, 257, 10, 11, 0, 234, 4112)]          # ceil(10000 / 9), ceil(2570 / 11)
    assert moved == [(3000, 1112), (1000, 999), (4112, 234), (2256, 10)] and end == 4346          # speed 1.0 and None: no job, own samples
    assert [resampled_len(L, r) for (_, L), r in zip(speech, [(10, 9), None, (10, 11), (1, 1)])] == [m[1] for m in moved]
    assert all(R.out_len(L, 10, 9) == resampled_len(L, (10, 9)) and R.out_len(L, 10, 11) == resampled_len(L, (10, 11)) for L in range(1, 200))
    assert resample_jobs(speech, [None] * 4, 3000) == ([], speech, 3000)
    # the speech RIR job reads the RESAMPLED signal, and the noise job is sized by L'
    rj, moff, nz, end2 = reverb_jobs(moved[:1], [(5000, 2000, 100)], [((0, 33), (33, 300))], end)
    assert rj[0] == (3000, 1112, 0, 1112, 0, 33, 4346) and moff == [4346]
    assert rj[1] == (5000, 2000, 100, 1112, 33, 300, 4346 + 1112) and nz == [(5458, 1112, 0)] and end2 == 4346 + 2224
    # the host model of the kernel, in place: the moved speech is the resampled signal
    x = R.signal('noise_0.3', 1000, 1)
    blob = np.full(4346, 0x5A5A, np.int16)
    blob[:1000] = x
    R.run_jobs(blob, jobs[:1])
    assert np.array_equal(blob[3000:4112], R.to_pcm(R.resample(x, 10, 9))) and (blob[4112:] == 0x5A5A).all()


# ---- draws and the data set -------------------------------------------------------------------------------------------------------------------------
def test_draw_speed_is_a_function_of_seed_epoch_and_index():
    first = [draw_speed(11, 0, i, 3) for i in range(60)]
    assert first == [draw_speed(11, 0, i, 3) for i in range(60)] and set(first) == {0, 1, 2}
    assert first != [draw_speed(11, 1, i, 3) for i in range(60)] and first != [draw_speed(12, 0, i, 3) for i in range(60)]
    assert all(draw_speed(11, e, i, 1) == 0 for e in range(3) for i in range(20))
    assert min(first.count(k) for k in range(3)) >= 10                                            # uniform


def test_dataset_without_speed_perturb_is_what_it_was(tmp_path):
    a, b = _rir_files(tmp_path)
    _, plain = _corpus(tmp_path)
    _, rev = _corpus(tmp_path, rir_scp=str(tmp_path / 'rir.scp'), rir_max_taps=100)
    _, one = _corpus(tmp_path, speed_perturb='1.0')
    for i in range(len(plain)):
        assert len(plain[i]) == 7 and len(rev[i]) == 8 and plain.draw_speed(i) is None
        assert (plain[i][4], plain[i][5]) == (_PARENT_DRAWS[i][1] % plain[i][3].shape[0], _PARENT_DRAWS[i][2])
        assert plain.draw(i) == rev.draw(i) == one.draw(i) == _PARENT_DRAWS[i]
        assert len(one[i]) == 9 and one[i][7] == (None, None) and one[i][8] is None and one[i][:2] == plain[i][:2]
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(one[i][:7], plain[i]))


_LENS_S = dict(_LENS, uttB=283)          # 283 samples are 258 at speed 1.1: the shortest utterance every speed of the test leaves long enough


def _corpus_s(tmp_path, **extra):
    import argparse
    from robust_e2e_gan_amd.data.wav_dataset import MixWavDataset
    rng = np.random.RandomState(3)
    sig = {}
    for name, n in list(_LENS_S.items()) + list(_NOISE.items()):
        sig[name] = rng.randint(-20000, 20000, n).astype(np.int16)
        wav_io.write_wav(str(tmp_path / (name + '.wav')), sig[name])
    (tmp_path / 'clean_wav.scp').write_text(''.join('%s %s\n' % (u, tmp_path / (u + '.wav')) for u in _LENS_S))
    (tmp_path / 'noise.scp').write_text(''.join('%s\n' % (tmp_path / (n + '.wav')) for n in _NOISE))
    (tmp_path / 'utt2spk').write_text(''.join('%s spk%s\n' % (u, u[-1]) for u in _LENS_S))
    (tmp_path / 'text_char').write_text(''.join('%s a b %s\n' % (u, 'c' * (i + 1)) for i, u in enumerate(_LENS_S)))
    (tmp_path / 'dict').write_text('a 1\nb 2\nc 3\n')
    args = argparse.Namespace(noise_repeat_num=3, seed=11, normalize_type=0, model_unit='char', **extra)
    return sig, MixWavDataset(args, str(tmp_path), str(tmp_path / 'dict'))


def test_dataset_with_speed_perturb(tmp_path):
    a, b = _rir_files(tmp_path)
    sig, ds = _corpus_s(tmp_path, speed_perturb='0.9,1.0,1.1')
    _, both = _corpus_s(tmp_path, speed_perturb='0.9, 1.0, 1.1', rir_scp=str(tmp_path / 'rir.scp'), rir_max_taps=100)
    _, plain = _corpus_s(tmp_path)
    assert ds.speeds == [(10, 9), None, (10, 11)] == both.speeds
    lens, seen = list(_LENS_S.values()), set()
    noise_lens = list(_NOISE.values())
    for i in range(len(ds)):
        it, sp = ds[i], ds.draw_speed(i)
        assert len(it) == 9 and it[7] == (None, None) and it[8] == sp == ds.speeds[draw_speed(11, 0, i, 3)]
        assert np.array_equal(it[2], sig[list(_LENS_S)[i % 4]])                                     # the file's samples: the device resamples
        Lp = resampled_len(lens[i % 4], sp)
        ni, start, db = draw_mixture(11, 0, i, noise_lens, Lp)                                    # draw_mixture sees L'
        assert ds.draw(i) == (ni, start, db) and (it[4], it[5]) == (start % noise_lens[ni], db)
        full = both[i]
        assert len(full) == 9 and full[8] == sp and full[7][0] is both.rir(both.draw_rirs(i)[0]) and (full[4], full[5]) == (it[4], it[5])
        seen.add(sp)
    assert seen == {(10, 9), None, (10, 11)}
    assert any(ds.draw(i)[1] != plain.draw(i)[1] for i in range(len(ds)) if ds.draw_speed(i) is not None)
    assert all(ds.draw(i) == plain.draw(i) for i in range(len(ds)) if ds.draw_speed(i) is None)
    before = [ds.draw_speed(i) for i in range(len(ds))]
    ds.set_epoch(1)
    assert [ds.draw_speed(i) for i in range(len(ds))] != before and [ds.draw_speed(i, epoch=0) for i in range(len(ds))] == before
    # the length buckets stay on the nominal lengths
    assert dict(ds.bins_to_samples) == dict(plain.bins_to_samples)


def test_constructor_refusals(tmp_path):
    for bad, word in (('0.9,fast', 'positive decimal'), ('-1.1', 'positive decimal'), ('0', 'positive decimal'), ('0.99', 'RE2E_WAV_RESAMPLE_MAX_RATE'),
                      (' , ', 'lists no speed')):
        with pytest.raises(ValueError) as e:
            _corpus(tmp_path, speed_perturb=bad)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(wav_io.WavError) as e:                        # uttB has 257 samples: 234 at speed 1.1
        _corpus(tmp_path, speed_perturb='1.0,1.1')
    assert 'uttB' in str(e.value) and '257' in str(e.value)
