"""tests/refs64_wav.py, the float64 restatement the waveform front end (csrc/stft.hip) is held to, checked on the CPU: against the
definition it restates, the precondition of every bar of tests/test_wav_kernels_gpu.py (the same statements in fp32 within a quarter of
it), the condition on the inputs those bars assume, and that each named mistake moves a case beyond a bar.

Measured when the module was written, fp32 on the CPU against float64 over the cases: magnitudes 5.8e-8 .. 1.2e-7 of the max (bar 1e-5),
logs 0.09 .. 0.14 of their bound at kept bins, cos at most 1.6e-5, exp(i angle) at most 1.6e-5 (bar 1e-4), g at most 5.3e-8 (1e-5); bins
below 1e-3 of the max: at most 0.2% per utterance."""
import numpy as np
import pytest

import refs64_wav as R


def test_rfft_is_the_dft_of_the_definition():
    rng = np.random.RandomState(0)
    sig = np.round(rng.randn(767) * 5000)
    X = R.stft(sig)
    y = np.pad(sig, 256, mode='reflect')
    for t in (0, 1, 2):
        direct = (R.window() * y[256 * t:256 * t + 512]) @ R.dft_matrix()
        assert np.abs(direct - X[t]).max() <= 1e-12 * np.abs(X).max()
    w = R.window()
    assert w[0] == w[511] and abs(w[0] - 0.08) < 1e-15 and np.allclose(w, w[::-1], rtol=0, atol=1e-15)          # symmetric: 511 in the cosine
    assert R.window(np.float32).dtype == np.float32 and np.array_equal(R.window(np.float32), w.astype(np.float32))


@pytest.mark.parametrize('L,T', [(257, 2), (512, 3), (767, 3)])
def test_frame_count_and_reflect_indices(L, T):
    sig = np.arange(L, dtype=np.float64) + 1
    assert R.n_frames(L) == T and R.stft(sig).shape == (T, 257)
    i = np.arange(-256, L + 256)
    r = R.reflect_index(i, L)
    assert r.min() >= 0 and r.max() < L
    assert np.array_equal(sig[r], np.pad(sig, 256, mode='reflect'))
    assert 256 * (T - 1) - 256 + 511 < L + 256                    # the last frame ends inside the padded signal


@pytest.mark.parametrize('N', [100, 700, 5000])
def test_modular_noise_index_is_tile_then_slice(N):
    rng = np.random.RandomState(N)
    noise = rng.randint(-3000, 3000, N).astype(np.int16)
    for L in (257, 1279, 2303):
        top = R.s0_range(N, L)
        for s0 in sorted({0, top // 2, top - 1}):
            assert np.array_equal(R.noise_segment(noise, s0 % N, L), R.noise_segment_tiled(noise, s0, L)), (N, L, s0)


@pytest.mark.parametrize('name', sorted(R.ALL_CASES))
def test_fp32_restatement_is_within_a_quarter_of_every_bar(name):
    _, _, cm = R.case_signals(name)
    for b, (r64, r32) in enumerate(zip(R.case_refs(name), R.case_refs(name, np.float32))):
        got = {k: v for k, v in r32.items() if k not in ('C', 'M')}
        print('ERR %-12s utt %d fp32-cpu %s' % (name, b, ' '.join('%s %.2e' % kv for kv in sorted(R.distances(got, r64, cm).items()))))
        assert R.violations(got, r64, cm, frac=0.25) == [], (name, b)
        assert R.violations({k: v for k, v in r64.items() if k not in ('C', 'M')}, r64, cm, frac=1e-9) == []


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_inputs_leave_at_most_one_percent_of_small_bins(name):
    for r in R.case_refs(name):
        assert R.small_share(r['clean']) <= 0.01 and R.small_share(r['mix']) <= 0.01, name
    lens = R.CASES[name][0]
    assert set(lens) <= set(R.LENGTHS)


def test_cases_cover_what_the_kernels_branch_on():
    lens = {L for c in R.CASES.values() for L in c[0]}
    assert lens == set(R.LENGTHS)
    assert {R.n_frames(L) for L in lens} == {2, 3, 5, 9}                      # below, at and above the 8 frames of a workgroup
    assert {c[1] for c in R.CASES.values()} == {100, 700, 5000}
    assert any(len(set(c[0])) > 1 for c in R.CASES.values())                   # ragged lengths inside one batch
    assert any(s0 + 2 >= c[1] for c in R.CASES.values() for s0 in c[2])        # a segment that starts at the end of its file and wraps
    tone = np.round(8000 * np.sin(2 * np.pi * 440 / 16000 * np.arange(2303)))
    assert R.small_share(np.abs(R.stft(tone))) > 0.5                           # why the cases are not clean tones


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_named_mistakes_move_a_case_beyond_a_bar(mistake):
    moved = []
    for name in sorted(R.ALL_CASES):
        _, _, cm = R.case_signals(name)
        for r64, wrong in zip(R.case_refs(name), R.case_refs(name, mistake=mistake)):
            bad = R.violations({k: v for k, v in wrong.items() if k not in ('C', 'M')}, r64, cm)
            if bad:
                moved.append((name, bad))
    assert moved, '%s stays within every bar of every case' % mistake
