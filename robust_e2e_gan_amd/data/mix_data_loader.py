"""Batch collation for the joint trainer (mirror of data/mix_data_loader.py:264-346).

``_collate_fn`` keeps the reference's host-side semantics (sort by length desc, zero padding,
IntTensor sizes, flat LongTensor targets).  ``collate_device`` is the MI355X-first variant (K1):
the ragged utterances are concatenated once on the host, shipped with ONE H2D copy per stream and
zero-padded on the device by re2e_pack_pad -- 3 live tensors instead of 5 (cos_angles and
clean_log_inputs are never read by joint_train.py).

``collate_wav_device`` / ``wav_features_device`` start from 16-bit PCM instead: the samples go over PCIe as ONE pinned int16 blob and
re2e_wav_mix_scale / re2e_wav_stft (csrc/stft.hip) mix the noise in at the drawn SNR and produce the padded spectra on the device.
``wav_istft_device`` goes the other way (re2e_wav_istft: enhanced magnitudes and a phase back to samples) and ``wav_sdr_device`` scores the
result against the clean samples (re2e_wav_sdr_sums: SNR and SI-SDR).  With speeds (``resample_jobs``, ``wav_frontend_device(speed=...)``) the
speech is resampled on the device first (re2e_wav_resample, csrc/resample.hip): speed perturbation."""
import ctypes
import logging
import re
from fractions import Fraction

import numpy as np
import torch

from ..lib import call


def _collate_fn(batch):
    """sample = (utt_id, spk_id, clean, clean_log, mix, mix_log, cos_angle, target)"""
    batch = sorted(batch, key=lambda sample: sample[2].size(0), reverse=True)
    longest = batch[0][2]
    F_, B, T = longest.size(1), len(batch), longest.size(0)
    outs = [torch.zeros(B, T, F_) for _ in range(5)]
    input_sizes = torch.IntTensor(B)
    target_sizes = torch.IntTensor(B)
    targets, utt_ids, spk_ids = [], [], []
    for x, s in enumerate(batch):
        utt_ids.append(s[0])
        spk_ids.append(s[1])
        n = s[2].size(0)
        for k in range(5):
            outs[k][x].narrow(0, 0, n).copy_(s[2 + k])
        input_sizes[x] = n
        target_sizes[x] = len(s[7])
        targets.extend(s[7])
    return (utt_ids, spk_ids, outs[0], outs[1], outs[2], outs[3], outs[4], torch.LongTensor(targets), input_sizes, target_sizes)


def pack_pad_device(flat_dev, lens, Tmax):
    """(sum T_i, F) device rows -> zero padded (B, Tmax, F) on the device (re2e_pack_pad)."""
    B, F_ = len(lens), flat_dev.shape[1]
    dev = flat_dev.device
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    out = torch.empty(B, Tmax, F_, dtype=torch.float32, device=dev)
    off_d = torch.from_numpy(off).to(dev)                 # keep both index tensors alive across the launch
    len_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    call('re2e_pack_pad', flat_dev.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), B, Tmax, F_, out.data_ptr())
    return out


def collate_device(batch, device, streams=(2, 4, 5)):
    """Device-side collate: returns the same 10-tuple as ``_collate_fn`` with the selected streams
    (default clean, mix, mix_log) padded on ``device``; the unused ones are None."""
    batch = sorted(batch, key=lambda sample: sample[2].size(0), reverse=True)
    lens = [int(s[2].size(0)) for s in batch]
    T = lens[0]
    outs = [None] * 5
    for k in streams:
        flat = torch.cat([s[k] for s in batch], 0).pin_memory() if torch.cuda.is_available() else torch.cat([s[k] for s in batch], 0)
        outs[k - 2] = pack_pad_device(flat.to(device, non_blocking=True), lens, T)
    targets = torch.LongTensor([t for s in batch for t in s[7]])
    return ([s[0] for s in batch], [s[1] for s in batch], outs[0], outs[1], outs[2], outs[3], outs[4], targets, torch.IntTensor(lens),
            torch.IntTensor([len(s[7]) for s in batch]))


def decode_pad_device(raws, device, Tmax=None, cmvn=None, want_log=False):
    """List of ``kaldi_io.RawMat`` (one per utterance, equal column counts) -> zero padded (B,Tmax,F) fp32 on ``device``
    (and, with ``want_log``, the normalised ``(10*log10(max(x,1e-7)) + cmvn[0]) * cmvn[1]`` tensor): the record bytes go
    over PCIe as ONE pinned blob and are decoded by re2e_kaldi_decode_pad.  'DM' records are converted to 'FM' first."""
    B, F_ = len(raws), raws[0].cols
    lens = [r.rows for r in raws]
    Tmax = max(lens) if Tmax is None else Tmax
    chunks, offs, kinds, pos = [], [], [], 0
    for r in raws:
        if r.cols != F_:
            raise ValueError('records of one stream must have the same number of columns')
        if r.kind == 'CM':
            body, kind = r.payload, 2
        else:                                    # data part only, as fp32
            data = r.payload if r.kind == 'FM' else np.frombuffer(r.payload.tobytes(), '<f8').astype('<f4').view(np.uint8)
            body, kind = data, 0
        pad = (-pos) % 16
        if pad:
            chunks.append(np.zeros(pad, np.uint8))
            pos += pad
        offs.append(pos)
        kinds.append(kind)
        chunks.append(np.ascontiguousarray(body))
        pos += body.size
    blob = torch.from_numpy(np.concatenate(chunks))
    on_gpu = torch.device(device).type == 'cuda'
    to = (lambda t: t.pin_memory().to(device, non_blocking=True)) if on_gpu else (lambda t: t.to(device))
    blob_d, off_d = to(blob), to(torch.tensor(offs, dtype=torch.int64))
    kind_d, len_d = to(torch.tensor(kinds, dtype=torch.int32)), to(torch.tensor(lens, dtype=torch.int32))
    out = torch.empty(B, Tmax, F_, dtype=torch.float32, device=device)
    out_log = torch.empty_like(out) if want_log else None
    cm = cmvn.to(device).float().contiguous() if cmvn is not None else None
    call('re2e_kaldi_decode_pad', blob_d.data_ptr(), off_d.data_ptr(), kind_d.data_ptr(), len_d.data_ptr(), B, Tmax, F_, out.data_ptr(),
         out_log.data_ptr() if want_log else None, cm.data_ptr() if cm is not None else None)
    for t in (blob_d, off_d, kind_d, len_d):      # uploaded on this stream, read by the kernel just launched
        t.record_stream(torch.cuda.current_stream()) if on_gpu else None
    return (out, out_log) if want_log else out


def collate_kaldi_device(batch, device, cmvn=None):
    """Device-side collate for Kaldi-table datasets.  ``batch`` = list of
    ``(utt_id, spk_id, clean RawMat, mix RawMat, clean_angle RawMat, mix_angle RawMat, target list)`` (angles may be
    None).  Returns the reference's 10-tuple (mix_data_loader.py:264-302) with all five feature streams on ``device``:
    linear spectra clamped at 1e-7, log spectra CMVN-normalised with the dataset ``cmvn`` (2,F) and
    ``cos_angles = cos(clean_angle - mix_angle)`` (:231), everything sorted by length (descending) and zero padded."""
    batch = sorted(batch, key=lambda s: s[3].rows, reverse=True)
    lens = [s[3].rows for s in batch]
    T = lens[0]
    clean, clean_log = decode_pad_device([s[2] for s in batch], device, T, cmvn, want_log=True)
    mix, mix_log = decode_pad_device([s[3] for s in batch], device, T, cmvn, want_log=True)
    cos = None
    if batch[0][4] is not None:
        ca, ma = decode_pad_device([s[4] for s in batch], device, T), decode_pad_device([s[5] for s in batch], device, T)
        cos = torch.cos(ca - ma)          # data-pipeline glue, as numpy in the reference; padded frames give cos(0) = 1 ...
        cos = ops_mask_rows(cos, lens)    # ... which the reference's zero padding does not have
    targets = torch.LongTensor([t for s in batch for t in s[6]])
    return ([s[0] for s in batch], [s[1] for s in batch], clean, clean_log, mix, mix_log, cos, targets, torch.IntTensor(lens),
            torch.IntTensor([len(s[6]) for s in batch]))


def ops_mask_rows(x, lens):
    from .. import ops
    from ..model.e2e_common import lens_dev
    with torch.no_grad():
        return ops.mask_rows(x, lens_dev(lens, x.device))


WAV_OUTPUTS = ('clean', 'clean_log', 'mix', 'mix_log', 'cos', 'clean_ang', 'mix_ang')       # re2e_wav_stft's outputs, in its argument order
WAV_BINS, WAV_HOP = 257, 256
_zero_noise = {}          # device -> [counter (device int32), pinned copy, event behind the copy, count already logged]


def wav_frames_of(n_samples):
    """Frames of an utterance of ``n_samples`` samples: 1 + L // 256 (librosa center=True, hop 256)."""
    return 1 + int(n_samples) // WAV_HOP


def _zero_noise_counter(device):
    """The device counter re2e_wav_mix_scale increments for a noise segment of zero power (the mixture is then the clean signal).  It is read
    one batch LATE -- the copy enqueued behind the previous batch, if it has landed -- so that no collate waits for the device."""
    key = str(device)
    st = _zero_noise.get(key)
    if st is None:
        st = _zero_noise[key] = [torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32).pin_memory(), None, 0]
    counter, host, ev, seen = st
    if ev is not None and ev.query():
        n = int(host[0])
        if n > seen:
            logging.getLogger(__name__).warning('%d noise segment(s) of zero power so far: those mixtures are the clean signal', n)
            st[3] = n
        st[2] = None
    return st


_reverb_clip = {}         # device -> the same four for the samples re2e_wav_reverb saturated


def _reverb_clip_counter(device):
    """The device counter re2e_wav_reverb increments for every reverberant sample it saturated to int16; read one batch late, as the
    zero-power counter."""
    key = str(device)
    st = _reverb_clip.get(key)
    if st is None:
        st = _reverb_clip[key] = [torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32).pin_memory(), None, 0]
    counter, host, ev, seen = st
    if ev is not None and ev.query():
        n = int(host[0])
        if n > seen:
            logging.getLogger(__name__).warning('%d reverberant sample(s) clipped at the 16-bit range so far', n)
            st[3] = n
        st[2] = None
    return st


_resample_clip = {}       # device -> the same four for the samples re2e_wav_resample saturated


def _resample_clip_counter(device):
    """The device counter re2e_wav_resample increments for every resampled sample it saturated to int16; read one batch late, as the
    zero-power counter."""
    key = str(device)
    st = _resample_clip.get(key)
    if st is None:
        st = _resample_clip[key] = [torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32).pin_memory(), None, 0]
    counter, host, ev, seen = st
    if ev is not None and ev.query():
        n = int(host[0])
        if n > seen:
            logging.getLogger(__name__).warning('%d speed-perturbed sample(s) clipped at the 16-bit range so far', n)
            st[3] = n
        st[2] = None
    return st


WAV_RESAMPLE_MAX_RATE = 64        # include/re2e.h RE2E_WAV_RESAMPLE_MAX_RATE


def speed_ratio(speed):
    """A speed factor given as a decimal string ('0.9') -> ``(up, down)`` of re2e_wav_resample, or None for a speed of exactly 1: the
    factor is p/q in lowest terms, up = q, down = p (0.9: 10/9, 1.1: 10/11).  Refuses what is not a positive decimal and a ratio beyond
    RE2E_WAV_RESAMPLE_MAX_RATE."""
    text = str(speed).strip()
    if not re.fullmatch(r'\d+(\.\d*)?|\.\d+', text) or Fraction(text) <= 0:
        raise ValueError('a speed is a positive decimal such as 0.9, got %r' % (speed,))
    f = Fraction(text)
    up, down = f.denominator, f.numerator
    if max(up, down) > WAV_RESAMPLE_MAX_RATE:
        raise ValueError('speed %s is the ratio %d/%d: beyond RE2E_WAV_RESAMPLE_MAX_RATE = %d' % (text, up, down, WAV_RESAMPLE_MAX_RATE))
    return None if up == down else (up, down)


def resampled_len(n_samples, ratio):
    """L' = ceil(L up / down) of an L-sample signal at ``ratio`` = None | (up, down)."""
    n = int(n_samples)
    if ratio is None or ratio[0] == ratio[1]:
        return n
    return -(-n * int(ratio[0]) // int(ratio[1]))


def resample_jobs(speech, speeds, pos):
    """The resamplings of one speed-perturbed batch, as re2e_wav_resample takes them (pure host arithmetic, no device).  ``speech``: one
    ``(offset, L)`` per utterance, ``speeds``: one ``None | (up, down)``, ``pos``: the first free sample behind the uploaded ones.  Returns
    ``(jobs, speech, end)``: ``jobs`` rows of ``(src_off, src_len, up, down, first, count, dst_off)``, the new ``(offset, L')`` of every
    utterance's speech (its own without a speed, and at a speed of exactly 1, which is not a job) and the first free sample behind the
    destinations."""
    jobs, out = [], []
    for (soff, L), ratio in zip(speech, speeds):
        if ratio is None or ratio[0] == ratio[1]:
            out.append((soff, L))
            continue
        n = resampled_len(L, ratio)
        jobs.append((soff, L, int(ratio[0]), int(ratio[1]), 0, n, pos))
        out.append((pos, n))
        pos += n
    return jobs, out, pos


def reverb_jobs(speech, noise, rirs, pos):
    """The convolutions of one reverberant batch, as re2e_wav_reverb takes them (pure host arithmetic, no device).  ``speech``: one
    ``(offset, L)`` per utterance, ``noise``: one ``(offset, N, s0)``, ``rirs``: one ``((offset, taps) | None, (offset, taps) | None)`` for
    speech and noise, ``pos``: the first free sample behind the uploaded ones.  Returns ``(jobs, mix_off, noise, end)``: ``jobs`` rows of
    ``(src_off, src_len, first, count, rir_off, rir_len, dst_off)``, the offset of every utterance's mixture speech (its own offset without
    a speech RIR), the ``(offset, N, s0)`` the mixture reads its noise with, and the first free sample behind the destinations.
    The noise follows the reference's order -- the whole file is reverberated, cut to the file's length, tiled and sliced -- without
    filtering samples nobody reads: a segment inside the file is one job (the new file is the segment, start 0), one that wraps once is
    two jobs to consecutive destinations, and a segment longer than the file takes the whole file and keeps its start."""
    jobs, mix_off, noise_out = [], [], []
    for (soff, L), (noff, N, s0), (hs, hn) in zip(speech, noise, rirs):
        if hs is None:
            mix_off.append(soff)
        else:
            jobs.append((soff, L, 0, L, hs[0], hs[1], pos))
            mix_off.append(pos)
            pos += L
        if hn is None:
            noise_out.append((noff, N, s0))
        elif L > N:
            jobs.append((noff, N, 0, N, hn[0], hn[1], pos))
            noise_out.append((pos, N, s0))
            pos += N
        else:
            head = min(L, N - s0)
            jobs.append((noff, N, s0, head, hn[0], hn[1], pos))
            if head < L:
                jobs.append((noff, N, 0, L - head, hn[0], hn[1], pos + head))
            noise_out.append((pos, L, 0))
            pos += L
    return jobs, mix_off, noise_out, pos


def wav_frontend_device(speech, device, noise=None, cmvn=None, want=('clean', 'mix', 'mix_log'), Tmax=None, pool=None, reverb=None, speed=None):
    """16-bit PCM -> spectra on ``device``, all work enqueued on the CURRENT stream.  ``speech``: int16 arrays, one per utterance, in the
    order of the batch rows; ``noise``: None (clean stream only) or one ``(noise int16 array, s0, dB)`` per utterance -- the mixture is
    ``s[i] + g * n[(s0 + i) % len(n)]`` with ``g = sqrt(sum s^2 / (P * 10^(dB/10)))``, P the power of that noise segment.  Arrays that are the
    same object are uploaded once.  Returns ``{name: (B, Tmax, 257) fp32}`` for the names in ``want`` (WAV_OUTPUTS), plus 'scale' (B,) with
    noise.  A noise segment of zero power gives g = 0 and is counted on the device (the reference draws another file instead).
    ``reverb`` (with ``noise``): None or one ``(h_speech | None, h_noise | None)`` of fp32 taps per utterance (Make_Noisy_Wave): the mixture
    is then ``conv(h_s, s)[:L][i] + g * r[(s0 + i) % len(n)]``, ``r = conv(h_n, n)[:len(n)]``, g from the powers AFTER reverberation, while
    'clean' stays the dry ``s``.  The distinct RIR arrays go up once in a pinned fp32 blob; the reverberant signals are rounded to int16
    behind the uploaded samples of the same allocation (re2e_wav_reverb), the spectra come from re2e_wav_stft_rev.  Reverberant samples
    that saturate are counted on the device and logged one batch late.
    ``speed``: None or one ``None | (up, down)`` per utterance (``speed_ratio``): those utterances are resampled first (re2e_wav_resample,
    int16, behind the uploaded samples), and from then on the resampled signal IS the speech -- the clean stream, the frame counts and Tmax
    (from L' = ceil(L up / down)), the source of the speech RIR, the L the noise segment and the SNR run over.  The order is resample,
    reverberate, mix, as Kaldi's recipes have it; the noise is never perturbed.  Saturated samples are counted on the device and logged one
    batch late.  A batch in which no utterance has a speed launches what it launches without the argument."""
    bad = [w for w in want if w not in WAV_OUTPUTS]
    if bad:
        raise ValueError('unknown front-end output %r (one of %s)' % (bad[0], ', '.join(WAV_OUTPUTS)))
    B = len(speech)
    lens = [int(s.shape[0]) for s in speech]
    arrays, where, pos = [], {}, 0

    def place(a):
        nonlocal pos
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError('the front end takes 1-D int16 sample arrays, got %s %s' % (a.dtype, a.shape))
        if id(a) not in where:
            where[id(a)] = pos
            arrays.append(a)
            pos += a.shape[0]
        return where[id(a)]
    soff = [place(s) for s in speech]
    longs = lambda v: (ctypes.c_long * B)(*[int(x) for x in v])
    on_gpu = torch.device(device).type == 'cuda'
    if noise is not None:
        noff = [place(n[0]) for n in noise]
        nlen = [int(n[0].shape[0]) for n in noise]
        s0 = [int(n[1]) % max(ln, 1) for n, ln in zip(noise, nlen)]
        db = (ctypes.c_float * B)(*[float(n[2]) for n in noise])
    uploaded = total = pos
    rs_jobs = []
    if speed is not None:
        if len(speed) != B:
            raise ValueError('speed: one None | (up, down) per utterance, got %d for %d utterances' % (len(speed), B))
        rs_jobs, moved, total = resample_jobs(list(zip(soff, lens)), speed, pos)
        soff, lens = [m[0] for m in moved], [m[1] for m in moved]
    T = max(wav_frames_of(n) for n in lens)
    Tmax = T if Tmax is None else int(Tmax)
    if reverb is not None and not any(h is not None for pair in reverb for h in pair):
        reverb = None                                # a batch without a reverberant item launches what it launches without RIRs
    if reverb is not None:
        if noise is None:
            raise ValueError('reverb needs noise: the reverberant signal is the mixture\'s speech stream')
        taps, hwhere, hpos = [], {}, 0

        def place_rir(h):
            nonlocal hpos
            if h is None:
                return None
            if h.dtype != np.float32 or h.ndim != 1 or h.shape[0] < 1:
                raise ValueError('an impulse response is a 1-D float32 array, got %s %s' % (h.dtype, h.shape))
            if id(h) not in hwhere:
                hwhere[id(h)] = hpos
                taps.append(h)
                hpos += h.shape[0]
            return hwhere[id(h)], int(h.shape[0])
        rirs = [(place_rir(hs), place_rir(hn)) for hs, hn in reverb]
        jobs, moff, nz, total = reverb_jobs(list(zip(soff, lens)), list(zip(noff, nlen, s0)), rirs, total)
        noff, nlen, s0 = [z[0] for z in nz], [z[1] for z in nz], [z[2] for z in nz]
        hhost = pool.get('rir', 4 * hpos).view(torch.float32) if pool is not None else torch.empty(hpos, dtype=torch.float32)
        if pool is None and on_gpu:
            hhost = hhost.pin_memory()
        np.concatenate(taps, out=hhost.numpy())
        hblob = hhost.to(device, non_blocking=True)
    host = pool.get('wav', 2 * uploaded).view(torch.int16) if pool is not None else torch.empty(uploaded, dtype=torch.int16)
    if pool is None and on_gpu:
        host = host.pin_memory()
    np.concatenate(arrays, out=host.numpy())
    if total == uploaded:
        blob = host.to(device, non_blocking=True)
    else:                                            # room behind the uploaded samples for the resampled and the reverberant signals
        blob = torch.empty(total, dtype=torch.int16, device=device)
        blob[:uploaded].copy_(host, non_blocking=True)
    if rs_jobs:
        rclip = _resample_clip_counter(device)
        rcols = [(ctypes.c_int if c in (2, 3) else ctypes.c_long) * len(rs_jobs) for c in range(7)]
        rcols = [t(*[int(j[c]) for j in rs_jobs]) for c, t in enumerate(rcols)]
        call('re2e_wav_resample', blob.data_ptr(), total, *rcols, len(rs_jobs), total, None, blob.data_ptr(), rclip[0].data_ptr())
        if on_gpu and rclip[2] is None:
            rclip[1].copy_(rclip[0], non_blocking=True)
            rclip[2] = torch.cuda.Event()
            rclip[2].record(torch.cuda.current_stream())
    out = {k: torch.empty(B, Tmax, WAV_BINS, dtype=torch.float32, device=device) for k in want}
    cm = cmvn.to(device).float().contiguous() if cmvn is not None else None
    p = lambda k: out[k].data_ptr() if k in out else None
    if noise is None:
        call('re2e_wav_stft', blob.data_ptr(), longs(soff), longs(lens), None, None, None, None, B, Tmax, *[p(k) for k in WAV_OUTPUTS],
             cm.data_ptr() if cm is not None else None)
    else:
        st = _zero_noise_counter(device)
        scale = torch.empty(B, dtype=torch.float32, device=device)
        idx = (longs(soff), longs(lens), longs(noff), longs(nlen), longs(s0))
        if reverb is None:
            call('re2e_wav_mix_scale', blob.data_ptr(), *idx, db, B, scale.data_ptr(), st[0].data_ptr())
            call('re2e_wav_stft', blob.data_ptr(), *idx, scale.data_ptr(), B, Tmax, *[p(k) for k in WAV_OUTPUTS],
                 cm.data_ptr() if cm is not None else None)
        else:
            clip = _reverb_clip_counter(device)
            cols = [(ctypes.c_long * len(jobs))(*[int(j[c]) for j in jobs]) for c in range(7)]
            call('re2e_wav_reverb', blob.data_ptr(), total, hblob.data_ptr(), hpos, *cols, len(jobs), total, None, blob.data_ptr(),
                 clip[0].data_ptr())
            call('re2e_wav_mix_scale', blob.data_ptr(), longs(moff), *idx[1:], db, B, scale.data_ptr(), st[0].data_ptr())
            call('re2e_wav_stft_rev', blob.data_ptr(), idx[0], longs(moff), *idx[1:], scale.data_ptr(), B, Tmax, *[p(k) for k in WAV_OUTPUTS],
                 cm.data_ptr() if cm is not None else None)
            if on_gpu:
                hblob.record_stream(torch.cuda.current_stream())
                if clip[2] is None:
                    clip[1].copy_(clip[0], non_blocking=True)
                    clip[2] = torch.cuda.Event()
                    clip[2].record(torch.cuda.current_stream())
        out['scale'] = scale
        if st[2] is None and on_gpu:
            st[1].copy_(st[0], non_blocking=True)
            st[2] = torch.cuda.Event()
            st[2].record(torch.cuda.current_stream())
    if on_gpu:
        blob.record_stream(torch.cuda.current_stream())
    return out


def collate_wav_device(batch, device, cmvn=None, want=('clean', 'mix', 'mix_log'), pool=None):
    """Device-side collate for ``MixWavDataset``.  ``batch`` = list of ``(utt_id, spk_id, speech int16, noise int16, s0, dB, target list)``,
    with an eighth element ``(h_speech | None, h_noise | None)`` when the data set has impulse responses (reverberant mixtures) and a
    ninth ``None | (up, down)`` when it perturbs the speed (the eighth is then always there): the batch is sorted by the PERTURBED length
    L' and the frame counts are those of L'.
    Returns the reference's 10-tuple (mix_data_loader.py:264-302), sorted by length (descending) and zero padded, with the streams named
    in ``want`` on ``device`` ('clean_log' and 'cos' for the enhancement trainers) and None for the others.  One pinned int16 upload per
    batch, the distinct noise files of the batch once; everything is enqueued on the current stream, so it plugs into ``DevicePrefetcher`` as
    ``lambda b, d, p: collate_wav_device(b, d, cmvn, pool=p)``."""
    length = lambda s: resampled_len(s[2].shape[0], s[8] if len(s) > 8 else None)
    batch = sorted(batch, key=length, reverse=True)
    o = wav_frontend_device([s[2] for s in batch], device, [(s[3], s[4], s[5]) for s in batch], cmvn, want, pool=pool,
                            reverb=[s[7] for s in batch] if len(batch[0]) > 7 else None,
                            speed=[s[8] for s in batch] if len(batch[0]) > 8 else None)
    lens = [wav_frames_of(length(s)) for s in batch]
    targets = torch.LongTensor([t for s in batch for t in s[6]])
    return ([s[0] for s in batch], [s[1] for s in batch], o.get('clean'), o.get('clean_log'), o.get('mix'), o.get('mix_log'), o.get('cos'), targets,
            torch.IntTensor(lens), torch.IntTensor([len(s[6]) for s in batch]))


def wav_features_device(pcms, device, cmvn=None):
    """Recognition from waveforms: ``(inputs, log_inputs, input_sizes)`` as the reference's SequentialDataset hands them to ``enhance_model``,
    ``feat_model`` and ``recognize`` -- the magnitude spectra (B,T,257), their normalised logs and the frame counts, in the order given."""
    o = wav_frontend_device(list(pcms), device, None, cmvn, ('clean', 'clean_log'))
    return o['clean'], o['clean_log'], torch.IntTensor([wav_frames_of(p.shape[0]) for p in pcms])


def wav_istft_device(mag, ang, lengths, device, int16=True, blob=False, clip_count=None):
    """Spectra back to samples on ``device`` (re2e_wav_istft, csrc/stft.hip): ``mag`` and ``ang`` (B,Tmax,257) fp32, ``lengths`` the sample
    count L_b of every utterance (its frames are the rows t < 1 + L_b // 256; ``wav_frontend_device`` of L_b samples gives exactly those).
    Samples 256 * (L_b // 256) .. L_b are zero (librosa's ``length`` padding).  ``int16``: rounded and saturated 16-bit samples, else fp32.
    Returns one numpy array of L_b samples per utterance, or with ``blob`` the device blob and the offsets of the utterances in it
    (nothing is read back).  ``clip_count``: a device int32 tensor incremented by the number of saturated samples."""
    lens = [int(n) for n in lengths]
    B = len(lens)
    if mag.shape != ang.shape or mag.dim() != 3 or mag.shape[0] != B or mag.shape[2] != WAV_BINS:
        raise ValueError('wav_istft_device takes mag and ang of shape (%d, Tmax, %d), got %s and %s' % (B, WAV_BINS, tuple(mag.shape), tuple(ang.shape)))
    mag = mag.to(device).float().contiguous()
    ang = ang.to(device).float().contiguous()
    offs = [0] * B
    for b in range(1, B):
        offs[b] = offs[b - 1] + lens[b - 1]
    total = offs[-1] + lens[-1]
    out = torch.empty(max(total, 1), dtype=torch.int16 if int16 else torch.float32, device=device)
    longs = lambda v: (ctypes.c_long * B)(*v)
    call('re2e_wav_istft', mag.data_ptr(), ang.data_ptr(), longs(offs), longs(lens), B, int(mag.shape[1]), total,
         None if int16 else out.data_ptr(), out.data_ptr() if int16 else None, clip_count.data_ptr() if clip_count is not None else None)
    if blob:
        return out, offs
    host = out.cpu().numpy()
    return [host[o:o + n] for o, n in zip(offs, lens)]


def sdr_from_sums(ss, yy, sy):
    """``{'snr', 'si_sdr'}`` in dB from sum s^2, sum y^2 and sum s y (re2e_wav_sdr_sums), in float64:
    SNR = 10 log10(sum s^2 / sum (s - y)^2), SI-SDR = 10 log10(|a s|^2 / |a s - y|^2) with a = sum s y / sum s^2, i.e.
    |a s|^2 = (sum s y)^2 / sum s^2 and |a s - y|^2 = sum y^2 - |a s|^2.  A zero denominator gives inf, a silent reference nan."""
    ss, yy, sy = float(ss), float(yy), float(sy)
    if ss <= 0.0:
        return {'snr': float('nan'), 'si_sdr': float('nan')}
    db = lambda num, den: float('inf') if den <= 0.0 else (float('-inf') if num <= 0.0 else 10.0 * float(np.log10(num / den)))
    target = sy * sy / ss
    return {'snr': db(ss, ss - 2.0 * sy + yy), 'si_sdr': db(target, yy - target)}


def wav_sdr_device(ref_pcms, est_blob, offsets, lengths):
    """SNR and SI-SDR of estimates on the device against int16 references: ``ref_pcms`` int16 arrays (uploaded as one blob), ``est_blob``
    the fp32 device blob of ``wav_istft_device(..., int16=False, blob=True)`` with its ``offsets``; utterance b is compared over its
    first ``lengths[b]`` samples.  The three sums per utterance are taken in double on the device (re2e_wav_sdr_sums); returns one
    ``{'snr', 'si_sdr'}`` dict per utterance."""
    B = len(ref_pcms)
    lens = [int(n) for n in lengths]
    device = est_blob.device
    if est_blob.dtype != torch.float32:
        raise ValueError('wav_sdr_device takes the fp32 estimate blob, got %s' % est_blob.dtype)
    roff, pos = [], 0
    for r, n, o in zip(ref_pcms, lens, offsets):
        if r.dtype != np.int16 or r.ndim != 1 or r.shape[0] < n or int(o) + n > est_blob.numel():
            raise ValueError('wav_sdr_device: a reference is not 1-D int16, or a length reaches beyond its reference or the estimate blob')
        roff.append(pos)
        pos += r.shape[0]
    host = torch.from_numpy(np.concatenate(ref_pcms))
    ref = (host.pin_memory() if device.type == 'cuda' else host).to(device, non_blocking=True)
    sums = torch.empty(B, 3, dtype=torch.float64, device=device)
    longs = lambda v: (ctypes.c_long * B)(*[int(x) for x in v])
    call('re2e_wav_sdr_sums', ref.data_ptr(), longs(roff), est_blob.data_ptr(), longs(offsets), longs(lens), B, sums.data_ptr())
    return [sdr_from_sums(*row) for row in sums.cpu().tolist()]


class BucketingSampler(object):
    """data/mix_data_loader.py:314-346: batches of similarly sized utterances from length bins."""

    def __init__(self, bins_to_samples, batch_size=1):
        self.bins_to_samples = bins_to_samples
        self.batch_size = batch_size
        self.bins = self.build_bins()

    def build_bins(self):
        ids = []
        for _, sample_idx in self.bins_to_samples.items():
            sample_idx = list(sample_idx)
            np.random.shuffle(sample_idx)
            ids.extend(sample_idx)
        return [ids[i:i + self.batch_size] for i in range(0, len(ids), self.batch_size)]

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch):
        self.bins = self.build_bins()
        np.random.shuffle(self.bins)
