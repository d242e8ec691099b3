"""Reverberant mixtures (csrc/reverb.hip: re2e_wav_reverb; csrc/stft.hip: re2e_wav_stft_rev) restated in numpy, on tests/refs64_wav.py:
the reference's Make_Reverberation ``np.convolve(h, x)[:len(x)]`` and Make_Noisy_Wave (speech and noise reverberated with one impulse
response each, THEN mixed at the drawn SNR; the enhancer's target stays the dry speech).  ``dtype=np.float64`` is the reference,
``dtype=np.float32`` the same statements in fp32 on the CPU.

Definition.  y[i] = sum_{k < K} h[k] x[i - k], x[j] = 0 for j < 0, i < len(x).  A reverberant signal is 16-bit PCM like every signal of
the front end: r = saturate(rint(y)).  For an utterance s of L samples, a noise file n of N samples, start s0, impulse responses h_s, h_n:
    rs = pcm(conv(h_s, s)),  rn = pcm(conv(h_n, n))  (the WHOLE file, cut to N, then tiled and sliced),
    g = sqrt(sum rs^2 / (P 10^(dB/10))),  P = sum_{i<L} rn[(s0 + i) mod N]^2,   m[i] = rs[i] + g rn[(s0 + i) mod N],
    C = STFT(s) (dry),  M = STFT(m);  every output as refs64_wav.features defines it.

The bound of the convolution is derived, not measured: a sum of K + 32 fp32 products (the kernel's contraction has 32 steps of exact zeros),
in ANY order, is within (K + 32) 2^-24 sum_k |h[k] x[i - k]| of the exact value (each partial sum is rounded once, relative 2^-24, and is
bounded by the sum of magnitudes; first order).  The 16-bit value then differs from the rounded float64 value by at most 1, and only where
the float64 value lies within that bound of a half-integer.  The spectra are held to refs64_wav's bars.

``MISTAKES`` names the ways an implementation goes wrong that these bounds have to tell from the definition."""
import numpy as np

import refs64_wav as W

FIR_MISTAKES = ('correlation', 'tap_off_by_one', 'history_not_zero', 'same_mode')
MIX_MISTAKES = ('noise_tiled_before_reverb', 'snr_before_reverb')
MISTAKES = FIR_MISTAKES + MIX_MISTAKES
EPS = 2.0 ** -24


def reverberate(h, x, dtype=np.float64, mistake=None):
    """np.convolve(h, x)[:len(x)] in ``dtype`` (Make_Reverberation)."""
    h, x = np.asarray(h).astype(dtype), np.asarray(x).astype(dtype)
    L, K = x.shape[0], h.shape[0]
    if mistake == 'correlation':                     # y[i] = sum h[k] x[i + k]
        return np.convolve(h[::-1], x)[K - 1:K - 1 + L]
    if mistake == 'tap_off_by_one':                  # y[i] = sum h[k] x[i - k - 1]
        return np.concatenate([np.zeros(1, dtype), np.convolve(h, x)])[:L]
    if mistake == 'history_not_zero':                # x[j] = x[j mod L] before sample 0
        reps = -(-K // L) + 1
        return np.convolve(h, np.tile(x, reps + 1))[reps * L:(reps + 1) * L]
    if mistake == 'same_mode':
        return np.convolve(h, x, mode='same')[:L]
    y = np.convolve(h, x)[:L]
    assert y.dtype == dtype
    return y


def fir(x, h, first, count, dtype=np.float64, mistake=None):
    """What job (x, h, first, count) of re2e_wav_reverb writes: y[first .. first + count)."""
    return reverberate(h, np.asarray(x)[:first + count], dtype, mistake)[first:first + count]


def fir_bound(x, h, first, count):
    """(K + 32) 2^-24 sum_k |h[k] x[i - k]| per output, in float64."""
    mag = np.convolve(np.abs(np.asarray(h, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64)[:first + count]))
    return (len(h) + 32) * EPS * mag[first:first + count]


def to_pcm(y):
    """saturate(rint(y)) as int16 (rint: half to even, as rintf)."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)), -32768, 32767).astype(np.int16)


def clipped(y):
    r = np.rint(np.asarray(y, dtype=np.float64))
    return int(((r > 32767) | (r < -32768)).sum())


def fir_violations(got, x, h, first, count, frac=1.0):
    """What of the fp32 output ``got`` of a job lies beyond ``frac`` of the bound from float64 (a list of strings; empty: held)."""
    ref, bound = fir(x, h, first, count), fir_bound(x, h, first, count)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bad = err > frac * bound
    if not bad.any():
        return []
    i = int(np.argmax(err - frac * bound))
    return ['%d output(s) beyond the bound; worst at %d: |err| %.3e, bound %.3e' % (int(bad.sum()), i, err[i], frac * bound[i])]


def pcm_violations(got_pcm, got_f32, x, h, first, count):
    """The int16 output against its three rules."""
    bad = []
    ref, bound = fir(x, h, first, count), fir_bound(x, h, first, count)
    got_pcm = np.asarray(got_pcm).astype(np.int64)
    if got_f32 is not None and not np.array_equal(got_pcm, to_pcm(got_f32).astype(np.int64)):
        bad.append('int16 is not saturate(rintf(fp32 output))')
    d = got_pcm - to_pcm(ref).astype(np.int64)
    if np.abs(d).max() > 1:
        bad.append('int16 differs from the rounded float64 value by %d' % np.abs(d).max())
    near_half = np.abs(np.abs(ref - np.floor(ref)) - 0.5) <= bound
    if (d != 0)[~near_half].any():
        bad.append('int16 differs where float64 is not within the bound of a half-integer (%d samples)' % int((d != 0)[~near_half].sum()))
    return bad


def fir_ratio(got, x, h, first, count):
    """max |err| / bound (0/0 counts as 0), for the printed lines."""
    ref, bound = fir(x, h, first, count), fir_bound(x, h, first, count)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err > 0, err / bound, 0.0)
    return float(q.max())


def rir(K, seed):
    """A decaying random impulse response of K taps with a unit direct path, fp32; its tail is scaled so that speech seldom saturates."""
    rng = np.random.RandomState(1000 + 7 * seed + K)
    k = np.arange(K, dtype=np.float64)
    h = rng.randn(K) * np.exp(-k / max(K / 5.0, 1.0)) * 0.3 / np.sqrt(max(1.0, K / 50.0))
    h[0] = 1.0
    return h.astype(np.float32)


def signal(n, seed, sigma=3000):
    rng = np.random.RandomState(50000 + seed)
    return np.clip(np.round(rng.randn(n) * sigma), -32768, 32767).astype(np.int16)


def fir_jobs(Kt, Ot):
    """The jobs of tests/test_reverb_kernels_gpu.py, [(name, K, count, first, src_len, src_off parity, dst_off parity)]: every K of
    1, 2, 31, 32, 33, Kt - 1, Kt, Kt + 1, 2 Kt + 5 (Kt: the kernel's K-tile), every count of 1, 31, 1024, Ot - 1, Ot, Ot + 1, 2 Ot + 7 (Ot: its
    outputs per workgroup) and every first of 0, 1, K - 1, K and a value beyond Ot appears, each K with a short and a long count, each
    count under a short and a long filter; src_len < K; offsets of both parities.  Not the full product: a job is independent of its
    neighbours, and the float64 reference of the large ones takes a tenth of a second each."""
    Ks = (1, 2, 31, 32, 33, Kt - 1, Kt, Kt + 1, 2 * Kt + 5)
    counts = (1, 31, 1024, Ot - 1, Ot, Ot + 1, 2 * Ot + 7)
    jobs = []

    def add(K, count, first_kind, tail=0):
        first = {'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'far': Ot + 13}[first_kind]
        n = len(jobs)
        jobs.append(('K%d_c%d_f%s' % (K, count, first_kind), K, count, first, first + count + tail, n % 2, (n // 2) % 2))
    kinds = ('0', '1', 'K-1', 'K', 'far')
    for i, K in enumerate(Ks):
        add(K, counts[i % 3], kinds[i % 5], tail=i % 2)                       # short counts
        add(K, counts[3 + i % 4], kinds[(i + 2) % 5], tail=(i + 1) % 2)       # around and beyond a workgroup
    for i, c in enumerate(counts):
        add(Ks[i % 5], c, kinds[(i + 1) % 5])
        add(Ks[5 + i % 4], c, kinds[(i + 3) % 5], tail=3)
    add(33, 20, '0')                                                          # src_len = 20 < K
    add(Kt + 1, 700, '0')                                                     # src_len = 700 < K, beyond one K-tile
    return jobs


def job_signals(job, index):
    name, K, count, first, src_len, _, _ = job
    return signal(src_len, index), rir(K, index)


# ---- the mixture --------------------------------------------------------------------------------------------------------------------------
def reverberant_pcm(h, x):
    """pcm(conv(h, x)[:len(x)]), the convolution in float64; ``h`` None: x itself."""
    return np.asarray(x) if h is None else to_pcm(reverberate(h, x))


def features_rev(speech, noise, s0, db, h_s=None, h_n=None, cmvn=None, dtype=np.float64, mistake=None):
    """Every output of re2e_wav_stft_rev for one utterance and ``g``, as refs64_wav.features; plus 'rs' and 'rn', the 16-bit reverberant
    speech and noise file (taken in float64 whatever ``dtype``: they are the kernel's INPUT, held to the convolution's own bound)."""
    speech, noise = np.asarray(speech), np.asarray(noise)
    L, N = speech.shape[0], noise.shape[0]
    rs = reverberant_pcm(h_s, speech)
    if mistake == 'noise_tiled_before_reverb':
        seg = reverberant_pcm(h_n, W.noise_segment(noise, s0, L))
    else:
        rn = reverberant_pcm(h_n, noise)
        seg = W.noise_segment(rn, s0, L)
    if mistake == 'snr_before_reverb':
        g = W.mix_scale(speech, noise, s0, db, dtype)
    else:
        g = W.mix_scale(rs, seg, 0, db, dtype)            # seg has L samples: start 0, no wrap
    out = W.features(speech, None, cmvn=cmvn, dtype=dtype)           # the dry stream
    cd = np.float64 if dtype == np.float64 else np.float32
    m = rs.astype(dtype) + g * seg.astype(dtype)
    M = W.stft(m, dtype)
    m0, m1 = (cmvn[0].astype(cd), cmvn[1].astype(cd)) if cmvn is not None else (cd(0), cd(1))
    mag = np.maximum(np.abs(M), cd(W.FLOOR)).astype(cd)
    out['g'], out['M'], out['mix'] = g, M, mag
    out['mix_log'] = ((cd(10) * np.log10(mag) + m0) * m1).astype(cd)
    out['mix_ang'] = np.angle(M).astype(cd)
    out['cos'] = np.real(W._angle_unit(out['C']) * np.conj(W._angle_unit(M))).astype(cd)
    out['rs'] = rs
    if mistake != 'noise_tiled_before_reverb':
        out['rn'] = rn
    return out


# name -> (speech lengths (refs64_wav.LENGTHS, not sorted), noise length, s0, dB, taps of h_s, taps of h_n; 0 taps: no impulse response)
MIX_CASES = {
    'inside5000': ((1279, 257, 2303), 5000, (0, 4100, 2696), (19.0, 0.5, 10.0), (33, 300, 1), (300, 1, 33)),
    'wrap700': ((512, 511, 2303), 700, (698, 650, 5), (3.0, 12.0, 7.5), (300, 0, 33), (33, 300, 0)),
}


def mix_case_signals(name):
    lens, N, s0, db, ks, kn = MIX_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    speech = [np.clip(np.round(rng.randn(L) * 4000), -32768, 32767).astype(np.int16) for L in lens]
    noise = np.clip(np.round(rng.randn(N) * 2500), -32768, 32767).astype(np.int16)
    cmvn = np.stack([-(40 + 5 * rng.rand(W.NBIN)), 0.1 + 0.05 * rng.rand(W.NBIN)]).astype(np.float32)
    hs = [rir(k, 2 * b) if k else None for b, k in enumerate(ks)]
    hn = [rir(k, 2 * b + 1) if k else None for b, k in enumerate(kn)]
    return speech, noise, cmvn, hs, hn


def mix_case_refs(name, dtype=np.float64, mistake=None, cmvn=True):
    speech, nz, cm, hs, hn = mix_case_signals(name)
    _, _, s0, db, _, _ = MIX_CASES[name]
    return [features_rev(s, nz, s0[b], db[b], hs[b], hn[b], cm if cmvn else None, dtype, mistake) for b, s in enumerate(speech)]


def run_jobs(blob, taps, jobs):
    """re2e_wav_reverb's jobs on the host, in place (``blob`` int16, ``taps`` fp32 blob), the convolutions in float64."""
    for src_off, src_len, first, count, rir_off, rir_len, dst_off in jobs:
        assert first + count <= src_len
        blob[dst_off:dst_off + count] = to_pcm(fir(blob[src_off:src_off + src_len], taps[rir_off:rir_off + rir_len], first, count))
    return blob
