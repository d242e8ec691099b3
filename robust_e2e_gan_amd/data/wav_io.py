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
