"""16-bit mono 16 kHz PCM wav files through the standard library's ``wave`` module (the reference reads them with scipy.io.wavfile,
data/prepare_feats.py:26-28, and uses the int16 samples as they are)."""
import wave

import numpy as np

SAMPLE_RATE = 16000


class WavError(ValueError):
    pass


def _open(path):
    try:
        w = wave.open(path, 'rb')
    except (wave.Error, EOFError) as e:
        raise WavError('%s: not a PCM wav file (%s)' % (path, e))
    if w.getsampwidth() != 2 or w.getnchannels() != 1 or w.getframerate() != SAMPLE_RATE or w.getcomptype() != 'NONE':
        got = (8 * w.getsampwidth(), w.getnchannels(), w.getframerate())
        w.close()
        raise WavError('%s: %d-bit, %d channel(s), %d Hz; the front end takes 16-bit mono %d Hz PCM' % ((path,) + got + (SAMPLE_RATE,)))
    return w


def read_wav(path):
    """The samples as an int16 ndarray."""
    w = _open(path)
    try:
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.int16, copy=False)
    finally:
        w.close()


def wav_frames(path):
    """Sample count, from the header only."""
    w = _open(path)
    try:
        return w.getnframes()
    finally:
        w.close()


_rirs = {}          # (path, max_taps) -> the one array object of that file


def read_rir(path, max_taps=16000):
    """A room impulse response as fp32 taps: a 16-bit mono 16 kHz wav (divided by 32768) or a 1-D ``.npy``.  The filter starts at its
    largest-magnitude tap (the direct path lands on tap 0, so a reverberant signal stays aligned with its dry source), is divided by that
    tap (unit direct path) and cut to ``max_taps``.  One array object per file, kept: items that share a file hand the SAME array to the
    collate, which uploads it once per batch."""
    key = (str(path), int(max_taps))
    h = _rirs.get(key)
    if h is not None:
        return h
    if int(max_taps) < 1:
        raise WavError('%s: max_taps must be at least 1' % path)
    if str(path).endswith('.npy'):
        try:
            a = np.load(path, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise WavError('%s: not a .npy file (%s)' % (path, e))
        if a.ndim != 1 or a.dtype.kind not in 'fiu':
            raise WavError('%s: shape %s of %s; an impulse response is a 1-D real array' % (path, a.shape, a.dtype))
        a = a.astype(np.float64)
    else:
        a = read_wav(path).astype(np.float64) / 32768.0
    if a.size == 0 or not np.isfinite(a).all():
        raise WavError('%s: an impulse response needs at least one tap, all finite' % path)
    peak = int(np.argmax(np.abs(a)))
    if a[peak] == 0.0:
        raise WavError('%s: an impulse response of zeros' % path)
    h = np.ascontiguousarray((a[peak:peak + int(max_taps)] / a[peak]).astype(np.float32))
    h.setflags(write=False)
    _rirs[key] = h
    return h


def write_wav(path, samples):
    """int16 samples -> a 16-bit mono 16 kHz file (tools and tests)."""
    samples = np.asarray(samples)
    if samples.dtype != np.int16 or samples.ndim != 1:
        raise WavError('write_wav takes a 1-D int16 array')
    w = wave.open(path, 'wb')
    try:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SAMPLE_RATE)
        w.writeframes(samples.astype('<i2').tobytes())
    finally:
        w.close()
