"""The waveform front end (csrc/stft.hip: re2e_wav_mix_scale, re2e_wav_stft) restated in numpy: reflect padding, framing, the symmetric
Hamming window and ``np.fft.rfft``; mixture and scale as the reference's MakeMixture meant them.  ``dtype=np.float64`` is the reference the
kernels are held to (no intermediate rounding), ``dtype=np.float32`` the same statements in fp32 on the CPU (the precondition of every bar).

Definition, for 16-bit mono PCM s[0..L), 257 <= L < 2^31:
    T = 1 + L // 256;  y[i] = s[-i] (i < 0), s[2(L-1)-i] (i >= L);  x_t[n] = w[n] y[256 t - 256 + n], n < 512;
    w[n] = 0.54 - 0.46 cos(2 pi n / 511);  X_t[k] = sum_n x_t[n] exp(-2 pi i k n / 512), k = 0..256
    m[i] = s[i] + g n[(s0 + i) mod N],  g = sqrt(sum s^2 / (P 10^(dB/10))),  P = the power of the N-periodic noise over i < L
``MISTAKES`` names the ways an implementation goes wrong that the bars have to tell from the definition."""
import numpy as np

NFFT, HOP, NBIN = 512, 256, 257
FLOOR = 1e-7
SMALL = 1e-3                     # bins below SMALL * max are held to finiteness and the clamp floor only
BAR_MAG = 1e-5                   # magnitudes and g: of the tensor's max (the project's forward bar)
BAR_ANG = 1e-4                   # cos and exp(i angle): absolute, where both magnitudes are >= SMALL * max
MISTAKES = ('periodic_window', 'edge_padding', 'hop_255', 'no_clamp', 'g_whole_file')


def window(dtype=np.float64, periodic=False):
    """The table is built in double and rounded: what ``scipy.signal.hamming(512)`` gives librosa."""
    n = np.arange(NFFT, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2 * np.pi * n / (NFFT if periodic else NFFT - 1))).astype(dtype)


def n_frames(L):
    return 1 + L // HOP


def reflect_index(i, L):
    """Index into s of padded sample y[i], i in [-256, L + 256)."""
    i = np.asarray(i, dtype=np.int64)
    return np.where(i < 0, -i, np.where(i >= L, 2 * (L - 1) - i, i))


def stft(sig, dtype=np.float64, mistake=None):
    """(T, 257) complex spectrum of a 1-D signal."""
    sig = np.asarray(sig).astype(dtype)
    L = sig.shape[0]
    assert L >= NBIN
    hop = 255 if mistake == 'hop_255' else HOP
    y = np.pad(sig, NFFT // 2, mode='edge' if mistake == 'edge_padding' else 'reflect')
    T = n_frames(L)
    idx = hop * np.arange(T)[:, None] + np.arange(NFFT)[None, :]
    x = y[idx] * window(dtype, periodic=mistake == 'periodic_window')[None, :]
    X = np.fft.rfft(x, axis=1)
    assert X.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return X


def dft_matrix():
    """(512, 257) float64 DFT matrix, to check ``np.fft.rfft`` against the definition."""
    n, k = np.arange(NFFT)[:, None], np.arange(NBIN)[None, :]
    return np.exp(-2j * np.pi * ((n * k) % NFFT) / NFFT)


def noise_segment(noise, s0, L):
    """n[(s0 + i) mod N], i < L."""
    noise = np.asarray(noise)
    return noise[(s0 + np.arange(L, dtype=np.int64)) % noise.shape[0]]


def noise_segment_tiled(noise, s0, L):
    """The reference's statement (prepare_feats.py MakeMixture): repeat the file until it covers the speech, then slice."""
    ex = np.asarray(noise)
    while ex.shape[0] < L:
        ex = np.concatenate([ex, noise], 0)
    return ex[s0:s0 + L]


def s0_range(N, L):
    """Exclusive upper end of the reference's draw of the segment start (prepare_feats.py:45-50): randint(0, elen - 1) when elen > 1."""
    tiled = N
    while tiled < L:
        tiled += N
    elen = tiled - L - 1
    return elen if elen > 1 else 1


def mix_scale(speech, noise, s0, db, dtype=np.float64, mistake=None):
    s = np.asarray(speech).astype(dtype)
    seg = (np.asarray(noise) if mistake == 'g_whole_file' else noise_segment(noise, s0, s.shape[0])).astype(dtype)
    p = np.sum(np.square(seg))
    if p <= 0:
        return dtype(0)
    return np.sqrt(np.sum(np.square(s)) / (p * dtype(10) ** (dtype(db) / dtype(10)))).astype(dtype)


def _angle_unit(X):
    """exp(i angle X) with angle 0 where X == 0, as np.angle."""
    mag = np.abs(X)
    return np.where(mag > 0, X / np.where(mag > 0, mag, 1), 1)


def features(speech, noise=None, s0=0, db=0.0, cmvn=None, dtype=np.float64, mistake=None):
    """Every output of re2e_wav_stft for one utterance, (T, 257) each, and ``g``.  Clean only when ``noise`` is None."""
    cd = np.float64 if dtype == np.float64 else np.float32
    C = stft(speech, dtype, mistake)
    floor = 0.0 if mistake == 'no_clamp' else FLOOR
    m0, m1 = (cmvn[0].astype(cd), cmvn[1].astype(cd)) if cmvn is not None else (cd(0), cd(1))

    def pair(X):
        mag = np.maximum(np.abs(X), cd(floor)).astype(cd)
        with np.errstate(divide='ignore'):
            return mag, ((cd(10) * np.log10(mag) + m0) * m1).astype(cd)
    out = {'C': C}
    out['clean'], out['clean_log'] = pair(C)
    out['clean_ang'] = np.angle(C).astype(cd)
    if noise is None:
        return out
    g = mix_scale(speech, noise, s0, db, dtype, mistake)
    m = np.asarray(speech).astype(dtype) + g * noise_segment(noise, s0, len(speech)).astype(dtype)
    M = stft(m, dtype, mistake)
    out['g'], out['M'] = g, M
    out['mix'], out['mix_log'] = pair(M)
    out['mix_ang'] = np.angle(M).astype(cd)
    out['cos'] = np.real(_angle_unit(C) * np.conj(_angle_unit(M))).astype(cd)
    return out


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def kept(mag64):
    """Bins the log and angle bars apply to: |X| >= SMALL * max, and above the clamp floor."""
    return (mag64 >= SMALL * mag64.max()) & (mag64 > FLOOR)


def log_bound(mag64, m1=1.0):
    """What the magnitude bar implies for (10 log10 |X| + m0) m1: (10 / ln 10) * BAR_MAG * max / |X| * m1."""
    return (10 / np.log(10)) * BAR_MAG * mag64.max() / mag64 * np.abs(m1)


# ---- the cases of tests/test_wav_kernels_gpu.py ----------------------------------------------------------------------------------------
LENGTHS = (257, 511, 512, 1279, 2303)            # T = 2, 2, 3, 5, 9
# name -> (speech lengths of the batch (not sorted: the kernels take any order), noise length, s0 per utterance, dB per utterance)
CASES = {
    'wrap100': ((2303, 257, 1279), 100, (37, 0, 99), (0.0, 20.0, 7.5)),
    'near_end700': ((512, 1279), 700, (698, 650), (3.0, 12.0)),
    'long5000': ((1279, 511, 2303), 5000, (0, 4100, 2696), (19.0, 0.5, 10.0)),
    'single': ((511,), 700, (188,), (5.0,)),
}
# all-zero speech: |C| = |M| = 0 and g = 0 -> every bin at the clamp floor, angle 0, cos 1.  Apart from CASES: the log and angle bars follow
# from the magnitude bar and do not reach a bin the clamp fired at; such a bin is held to the floor itself, finiteness and the fp32 value of
# the log at the floor (violations() below).
FLOOR_CASES = {'silence': ((257,), 100, (5,), (10.0,))}
ALL_CASES = dict(CASES, **FLOOR_CASES)


def case_signals(name):
    """Gaussian int16-range speech per utterance, ONE noise file and a (2, 257) cmvn for a case.  Gaussian: a flat spectrum, so almost no bin
    is small against the max (a clean tone without a noise floor leaves 69% below SMALL * max)."""
    lens, N, s0, db = ALL_CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    speech = [np.clip(np.round(rng.randn(L) * (0 if name == 'silence' else 6000)), -32768, 32767).astype(np.int16) for L in lens]
    noise = np.clip(np.round(rng.randn(N) * 2500), -32768, 32767).astype(np.int16)
    cmvn = np.stack([-(40 + 5 * rng.rand(NBIN)), 0.1 + 0.05 * rng.rand(NBIN)]).astype(np.float32)
    return speech, noise, cmvn


def case_refs(name, dtype=np.float64, mistake=None, cmvn=True, noise=True):
    """Per utterance of a case: ``features`` (every output and g) -- the reference a kernel run of that case is held to."""
    speech, nz, cm = case_signals(name)
    _, _, s0, db = ALL_CASES[name]
    return [features(s, nz if noise else None, s0[b], db[b], cm if cmvn else None, dtype, mistake) for b, s in enumerate(speech)]


def small_share(mag64):
    """Share of bins the log and angle bars do not reach."""
    return 1.0 - float((mag64 >= SMALL * mag64.max()).mean())


def _unit(angle):
    return np.exp(1j * np.asarray(angle, dtype=np.float64))


def violations(got, ref, cmvn=None, frac=1.0):
    """What of ``got`` (name -> (T, 257) array, 'g' -> scalar; any subset) lies beyond ``frac`` of its bar from the float64 ``ref`` of the
    same utterance, as a list of strings with the measured distance (empty: all bars held).
      magnitudes, g: BAR_MAG of the tensor's max, and never below the clamp floor
      logs: finite everywhere; at bins with |X| >= SMALL * max within (10 / ln 10) * BAR_MAG * max / |X| * cmvn[1]
      cos, exp(i angle): BAR_ANG absolute where the magnitudes involved are >= SMALL * max"""
    bad = []
    m1 = np.abs(cmvn[1].astype(np.float64)) if cmvn is not None else 1.0
    keep = {'clean': kept(ref['clean'])}
    if 'mix' in ref:
        keep['mix'] = kept(ref['mix'])
    for q in ('clean', 'mix'):
        if q in got:
            e = rel_err(got[q], ref[q])
            if not e <= frac * BAR_MAG:
                bad.append('%s %.3e of the max (bar %.1e)' % (q, e, frac * BAR_MAG))
            if not (np.asarray(got[q], dtype=np.float64) >= FLOOR * (1 - 1e-6)).all():          # float32(1e-7) or 1e-7
                bad.append('%s below the clamp floor' % q)
        ql = q + '_log'
        if ql in got:
            g64 = np.asarray(got[ql], dtype=np.float64)
            if not np.isfinite(g64).all():
                bad.append('%s not finite' % ql)
            else:
                e = (np.abs(g64 - ref[ql]) / (log_bound(ref[q]) * m1))[keep[q]].max() if keep[q].any() else 0.0
                at_floor = ref[q] <= FLOOR                                  # the log of the floor itself: fp32 rounding of a value near -70 + m0
                if at_floor.any() and not (np.abs(g64 - ref[ql])[at_floor] <= 1e-5 * np.abs(ref[ql])[at_floor].max()).all():
                    bad.append('%s at the clamp floor is not the log of the floor' % ql)
                if not e <= frac:
                    bad.append('%s %.3f of its bound (bar %.2f)' % (ql, e, frac))
        qa = q + '_ang'
        if qa in got:
            e = np.abs(_unit(got[qa]) - _unit(ref[qa]))[keep[q] | (ref[q] <= FLOOR)].max()          # at the floor X = 0: angle 0
            if not e <= frac * BAR_ANG:
                bad.append('%s %.3e (bar %.1e)' % (qa, e, frac * BAR_ANG))
    if 'cos' in got:
        both = (keep['clean'] | (ref['clean'] <= FLOOR)) & (keep['mix'] | (ref['mix'] <= FLOOR))
        e = np.abs(np.asarray(got['cos'], dtype=np.float64) - ref['cos'])[both].max()
        if not e <= frac * BAR_ANG:
            bad.append('cos %.3e (bar %.1e)' % (e, frac * BAR_ANG))
    if 'g' in got:
        e = abs(float(got['g']) - float(ref['g'])) / max(abs(float(ref['g'])), 1e-300) if float(ref['g']) != 0 else abs(float(got['g']))
        if not e <= frac * BAR_MAG:
            bad.append('g %.3e (bar %.1e)' % (e, frac * BAR_MAG))
    return bad


def distances(got, ref, cmvn=None):
    """The same distances as numbers, for the printed lines: name -> distance in units of what ``violations`` compares with its bar."""
    out = {}
    m1 = np.abs(cmvn[1].astype(np.float64)) if cmvn is not None else 1.0
    keep = {q: kept(ref[q]) for q in ('clean', 'mix') if q in ref}
    for q in keep:
        if q in got:
            out[q] = rel_err(got[q], ref[q])
        if q + '_log' in got:
            out[q + '_log'] = float((np.abs(np.asarray(got[q + '_log'], dtype=np.float64) - ref[q + '_log']) / (log_bound(ref[q]) * m1))[keep[q]].max()) if keep[q].any() else 0.0
        if q + '_ang' in got:
            out[q + '_ang'] = float(np.abs(_unit(got[q + '_ang']) - _unit(ref[q + '_ang']))[keep[q] | (ref[q] <= FLOOR)].max())
    if 'cos' in got:
        both = (keep['clean'] | (ref['clean'] <= FLOOR)) & (keep['mix'] | (ref['mix'] <= FLOOR))
        out['cos'] = float(np.abs(np.asarray(got['cos'], dtype=np.float64) - ref['cos'])[both].max())
    if 'g' in got and float(ref['g']) != 0:
        out['g'] = abs(float(got['g']) - float(ref['g'])) / abs(float(ref['g']))
    return out
