"""The inverse STFT and the signal metrics (csrc/stft.hip: re2e_wav_istft, re2e_wav_sdr_sums) restated in numpy on ``np.fft.irfft``.
``dtype=np.float64`` is the reference the kernel is held to, ``dtype=np.float32`` the same statements in fp32 on the CPU (the precondition
of the bar).  The forward it inverts is ``refs64_wav.stft``.

Definition (librosa.istft(hop_length=256, window=scipy.signal.hamming, center=True, length=L)), for (T, 257) ``mag`` and ``ang``, T = 1 + L // 256:
    X_t[k] = mag (cos ang + i sin ang), imaginary parts of bins 0 and 256 ignored;  x_t = irfft(X_t, 512) (with the 1/512)
    w[n] = 0.54 - 0.46 cos(2 pi n / 511);  for i < 256 (T - 1), t = 1 + i // 256, m = i % 256:
    y[i] = (w[m + 256] x_{t-1}[m + 256] + w[m] x_t[m]) / (w[m + 256]^2 + w[m]^2);  y[i] = 0 for 256 (T - 1) <= i < L
``istft`` is that two-frame gather; ``istft_ola`` derives the same samples by a generic overlap-add into a padded buffer, a division by
the accumulated sum of w^2 and a trim of 256 samples at both ends.  ``MISTAKES`` names the ways an implementation goes wrong that the bar
has to tell from the definition."""
import numpy as np

import refs64_wav as W

NFFT, HOP, NBIN = W.NFFT, W.HOP, W.NBIN
BAR = W.BAR_MAG                  # float output against float64: 1e-5 of the tensor's max (the project's forward bar)
MISTAKES = ('no_window_norm', 'periodic_window', 'no_trim', 'conj_phase', 'keep_dc_imag', 'tail_not_zero')
GROUP = 15                       # hop blocks a workgroup of wav_istft_kernel owns (csrc/stft.hip IBLOCKS); it transforms GROUP + 1 frames
SDR_STRIDE = 4096                # samples a workgroup of wav_sdr_sums_kernel takes per trip (SDR_THREADS * SDR_UNROLL)


def spectrum(mag, ang, dtype=np.float64, mistake=None):
    """(T, 257) complex X of the given magnitudes and angles."""
    cd = np.complex128 if dtype == np.float64 else np.complex64
    mag, ang = np.asarray(mag).astype(dtype), np.asarray(ang).astype(dtype)
    sign = dtype(-1) if mistake == 'conj_phase' else dtype(1)
    X = (mag * np.cos(ang) + 1j * (sign * mag * np.sin(ang))).astype(cd)
    return X


def frames(mag, ang, dtype=np.float64, mistake=None):
    """(T, 512) real frames x_t = irfft(X_t).  'keep_dc_imag': frames 2q and 2q + 1 share one complex transform z = X_a + i X_b with the
    imaginary parts of bins 0 and 256 left in, which then land in the partner frame: x_a -= (Im X_b[0] + (-1)^n Im X_b[256]) / 512 and
    x_b += (Im X_a[0] + (-1)^n Im X_a[256]) / 512."""
    X = spectrum(mag, ang, dtype, mistake)
    leak_src = X.copy()
    X[:, 0] = X[:, 0].real
    X[:, NBIN - 1] = X[:, NBIN - 1].real
    x = np.fft.irfft(X, NFFT, axis=1)
    assert x.dtype == dtype
    if mistake == 'keep_dc_imag':
        alt = (1 - 2 * (np.arange(NFFT) % 2)).astype(dtype)
        leak = (leak_src[:, :1].imag + alt[None, :] * leak_src[:, NBIN - 1:].imag) / dtype(NFFT)         # (T, 512): what frame t gives away
        T = x.shape[0]
        for a in range(0, T, 2):
            b = a + 1
            if b < T:
                x[a] -= leak[b]
                x[b] += leak[a]
    return x.astype(dtype)


def istft(mag, ang, L, dtype=np.float64, mistake=None):
    """(L,) samples: the two-frame gather."""
    T = W.n_frames(L)
    mag, ang = np.asarray(mag)[:T], np.asarray(ang)[:T]
    assert mag.shape == (T, NBIN) and ang.shape == (T, NBIN)
    x = frames(mag, ang, dtype, mistake)
    w = W.window(dtype, periodic=mistake == 'periodic_window')
    y = np.zeros(L, dtype)
    n_keep = HOP * (T - 1)
    shift = 0 if mistake == 'no_trim' else HOP           # 'no_trim': the first 256 samples of the padded signal are not dropped
    i = np.arange(n_keep)
    p = i + shift
    t, m = p // HOP, p % HOP
    prev = np.where(t >= 1, t - 1, 0)
    num = w[m] * x[np.minimum(t, T - 1), m] * (t <= T - 1) + w[m + HOP] * x[prev, m + HOP] * (t >= 1)
    den = np.square(w[m]) * (t <= T - 1) + np.square(w[m + HOP]) * (t >= 1)
    y[:n_keep] = num if mistake == 'no_window_norm' else num / den
    if mistake == 'tail_not_zero':                       # the last frame's second half runs on past 256 (T - 1)
        j = np.arange(L - n_keep)
        y[n_keep:] = x[T - 1, HOP + j] / w[HOP + j]
    return y.astype(dtype)


def istft_ola(mag, ang, L):
    """The same samples by the textbook route, float64: overlap-add w x_t at 256 t into a buffer of 256 (T + 1) samples, divide by the
    accumulated w^2, drop 256 samples at both ends, zero-pad to L."""
    T = W.n_frames(L)
    x = frames(np.asarray(mag)[:T], np.asarray(ang)[:T])
    w = W.window()
    buf, wsum = np.zeros(HOP * (T + 1)), np.zeros(HOP * (T + 1))
    for t in range(T):
        buf[HOP * t:HOP * t + NFFT] += w * x[t]
        wsum[HOP * t:HOP * t + NFFT] += np.square(w)
    y = (buf / wsum)[HOP:HOP * T]
    return np.concatenate([y, np.zeros(L - y.shape[0])])


def to_int16(y):
    """(int16 samples, number of samples that saturate): round half to even as rintf, clip to -32768 .. 32767."""
    r = np.rint(np.asarray(y, dtype=np.float64))
    return np.clip(r, -32768, 32767).astype(np.int16), int(((r > 32767) | (r < -32768)).sum())


def rel_err(got, ref):
    return W.rel_err(got, ref)


def margin_ok(mag, ang, L, ref64=None, frac=0.25):
    """The fp32 CPU run of the restatement against float64, as a share of the max; asserts it stays within ``frac`` of the bar."""
    ref64 = istft(mag, ang, L) if ref64 is None else ref64
    e = rel_err(istft(mag, ang, L, np.float32), ref64)
    assert e <= frac * BAR, 'fp32 on the CPU is %.3e of the max from float64: not within %.2f of the bar %.1e' % (e, frac, BAR)
    return e


# ---- signal metrics ----------------------------------------------------------------------------------------------------------------------
def sdr_sums(s, y):
    """(sum s^2, sum y^2, sum s y) in float64 of an int16 reference and an fp32 estimate."""
    s, y = np.asarray(s).astype(np.float64), np.asarray(y).astype(np.float64)
    return np.array([np.dot(s, s), np.dot(y, y), np.dot(s, y)])


def snr_direct(s, y):
    s, y = np.asarray(s).astype(np.float64), np.asarray(y).astype(np.float64)
    return 10 * np.log10(np.sum(np.square(s)) / np.sum(np.square(s - y)))


def si_sdr_direct(s, y):
    """10 log10(|a s|^2 / |a s - y|^2), a = <s, y> / <s, s>, from the signals themselves."""
    s, y = np.asarray(s).astype(np.float64), np.asarray(y).astype(np.float64)
    a = np.dot(s, y) / np.dot(s, s)
    return 10 * np.log10(np.sum(np.square(a * s)) / np.sum(np.square(a * s - y)))


# ---- the cases of tests/test_istft_kernels_gpu.py ----------------------------------------------------------------------------------------
# refs64_wav.LENGTHS (T = 2, 2, 3, 5, 9) and: an odd T below the group (T = 7); GROUP + 1 = 16 frames, exactly what one workgroup transforms
# (its zero tail is the first block of the next); one frame more (T = 17: the second workgroup has a lone frame and one block of samples)
LENGTHS = W.LENGTHS + (1600, HOP * GROUP + 77, HOP * (GROUP + 1) + 100)
RAGGED = (HOP * (GROUP + 1) + 100, 257, 1600)          # B = 3, Tmax = 17 + 2: rows t >= T_b are NaN
SDR_CASES = ((257,), (SDR_STRIDE + 1,), (2303, 257, 1279))


def random_spectrum(L, seed, extra_rows=0, scale=3.0e5):
    """(T + extra_rows, 257) fp32 ``mag`` and ``ang`` that are NOT the STFT of any signal: independent magnitudes and angles, with nonzero
    imaginary parts at bins 0 and 256.  Rows t >= T are NaN."""
    T = W.n_frames(L)
    rng = np.random.RandomState(seed)
    mag = (np.abs(rng.randn(T, NBIN)) * scale).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, (T, NBIN)).astype(np.float32)
    pad = np.full((extra_rows, NBIN), np.nan, np.float32)
    return np.concatenate([mag, pad]), np.concatenate([ang, pad])


def speech(L, seed):
    """Gaussian int16 speech, as refs64_wav.case_signals."""
    rng = np.random.RandomState(seed)
    return np.clip(np.round(rng.randn(L) * 6000), -32768, 32767).astype(np.int16)


def saturating_spectrum(L=1600, seed=5):
    """A consistent spectrum (fp32 mag / ang of the float64 STFT) of a signal that is below half scale everywhere but on 7 known samples
    at twice full scale (four above, three below): its float64 reconstruction exceeds full scale exactly there.  Returns
    ``(mag, ang, signal float64, positions)``."""
    rng = np.random.RandomState(seed)
    x = np.clip(rng.randn(L) * 3000, -12000, 12000)
    pos = np.array([3, 255, 256, 700, 1023, 1024, 1500])
    assert pos.max() < HOP * (W.n_frames(L) - 1)
    x[pos] = np.array([65536.0, -65536.0, 65536.0, -65536.0, 65536.0, -65536.0, 65536.0])
    X = W.stft(x)
    return np.abs(X).astype(np.float32), np.angle(X).astype(np.float32), x, pos
