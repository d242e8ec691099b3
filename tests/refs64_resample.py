"""Speed perturbation (csrc/resample.hip: re2e_wav_resample) restated in numpy, nothing imported from the product: the rational
resampler scipy.signal.resample_poly(x, up, down) with its defaults, written out.  ``dtype=np.float64`` is the reference,
``dtype=np.float32`` the same statements in fp32 on the CPU (table rounded once, fp32 products, fp32 sums).

Definition (include/re2e.h).  A speed s = p/q in lowest terms gives up = q, down = p.  For an L-sample source x, L' = ceil(L up / down):
    half = 10 max(up, down),  fc = 1 / max(up, down)
    g[i] = fc sinc(fc (i - half)) kaiser_{2 half + 1, beta = 5}(i),  0 <= i <= 2 half
    h[i] = up g[i] / sum g
    y[m] = sum_j x[j] h[half + m down - j up],  0 <= j < L,  0 <= half + m down - j up <= 2 half      (x is zero outside 0 .. L - 1)
A resampled signal is 16-bit PCM like every signal of the front end: saturate(rint(y)).

The bound is derived, not measured.  An output is a sum of at most N = ceil((2 half + 1) / up) products.  In fp32 each coefficient is
rounded once, each product once, and there are at most N - 1 additions in any order: to first order the value is within
(1 + 1 + N - 1) 2^-24 sum_j |h[.] x[j]| of float64; (N + 4) 2^-24 sum |h x| covers the second-order term and an accumulation split in
parts.  The 16-bit value then differs from the rounded float64 value by at most 1, and only where the float64 value lies within that bound
of a half-integer.  The library's fp32 table is within 2^-24 |h| + 1e-12 max |h| of ``table``: one rounding, and a cap three orders above
the double-precision differences between two evaluations of I0 and sin.

``MISTAKES`` names the ways an implementation goes wrong that the bound (``length_floor``: the length check) has to tell from the definition:
    time_reversed       the phase of the table taken with the wrong sign: output m walks phase (-(half + m down)) mod up
    gain_missing        h without the factor up
    not_normalised      h without the division by sum g
    centre_off_by_one   half + 1 in the index
    length_floor        L' = floor(L up / down)
    edges_reflected     x mirrored at its ends instead of zero outside 0 .. L - 1
    hann_window         a Hann window in place of the Kaiser window"""
import functools

import numpy as np

MISTAKES = ('time_reversed', 'gain_missing', 'not_normalised', 'centre_off_by_one', 'length_floor', 'edges_reflected', 'hann_window')
EPS = 2.0 ** -24
RATIOS = ((10, 9), (10, 11), (20, 21), (2, 1), (1, 2), (3, 2), (63, 64), (64, 63))
WIDE_RATIOS = ((1, 64), (1, 16))          # down / up so large that a workgroup stages its input in several parts


def out_len(L, up, down, mistake=None):
    return L * up // down if mistake == 'length_floor' else -(-L * up // down)


def source_len(target, up, down):
    """The shortest source whose resampled length is at least ``target``."""
    L = max(1, (target - 1) * down // up)
    while out_len(L, up, down) < target:
        L += 1
    return L


@functools.lru_cache(maxsize=None)
def table(up, down, mistake=None):
    """h[0 .. 2 half] in float64, and half."""
    R = max(up, down)
    half = 10 * R
    n = np.arange(2 * half + 1, dtype=np.float64)
    fc = 1.0 / R
    win = np.hanning(2 * half + 1) if mistake == 'hann_window' else np.kaiser(2 * half + 1, 5.0)
    g = fc * np.sinc(fc * (n - half)) * win
    h = g.copy()
    if mistake != 'not_normalised':
        h = h / g.sum()
    if mistake != 'gain_missing':
        h = h * up
    return h, half


def _terms(x, up, down, first, count, dtype, mistake):
    """(count, N) products h[.] x[j] of the outputs first .. first + count - 1 in ``dtype`` (zero where a tap or a sample is outside)."""
    x = np.asarray(x)
    L = x.shape[0]
    h, half = table(up, down, mistake if mistake in ('gain_missing', 'not_normalised', 'hann_window') else None)
    h = h.astype(dtype)
    N = -(-(2 * half + 1) // up)
    m = np.arange(first, first + count, dtype=np.int64)[:, None]
    t = np.arange(N, dtype=np.int64)[None, :]
    a = half + (1 if mistake == 'centre_off_by_one' else 0) + m * down
    jm = a // up
    phi = (-a) % up if mistake == 'time_reversed' else a - jm * up
    idx = phi + t * up
    j = jm - t
    if mistake == 'edges_reflected':
        inside = np.ones_like(j, dtype=bool)
        period = max(2 * L - 2, 1)
        jr = np.abs(j) % period
        j = np.where(jr >= L, period - jr, jr)
    else:
        inside = (j >= 0) & (j < L)
    ok = inside & (idx <= 2 * half)
    hv = np.where(ok, h[np.minimum(idx, 2 * half)], dtype(0))
    xv = np.where(ok, x[np.clip(j, 0, L - 1)].astype(dtype), dtype(0))
    p = hv * xv
    assert p.dtype == dtype
    return p


def job(x, up, down, first, count, dtype=np.float64, mistake=None):
    """What job (x, up, down, first, count) of re2e_wav_resample writes: y[first .. first + count)."""
    y = _terms(x, up, down, first, count, dtype, mistake).sum(axis=1, dtype=dtype)
    assert y.dtype == dtype
    return y


def resample(x, up, down, dtype=np.float64, mistake=None):
    """The whole resampled signal, L' samples."""
    return job(x, up, down, 0, out_len(len(x), up, down, mistake), dtype, mistake)


def bound(x, up, down, first, count):
    """(N + 4) 2^-24 sum_j |h[.] x[j]| per output, in float64."""
    _, half = table(up, down)
    N = -(-(2 * half + 1) // up)
    return (N + 4) * EPS * np.abs(_terms(x, up, down, first, count, np.float64, None)).sum(axis=1)


def to_pcm(y):
    """saturate(rint(y)) as int16 (rint: half to even, as rintf)."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64)), -32768, 32767).astype(np.int16)


def clipped(y):
    r = np.rint(np.asarray(y, dtype=np.float64))
    return int(((r > 32767) | (r < -32768)).sum())


def violations(got, ref, bnd, frac=1.0):
    """What of an fp32 output ``got`` lies beyond ``frac`` of the bound from float64 (a list of strings; empty: held)."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref.shape:
        return ['%d outputs, the definition has %d' % (got.shape[0], ref.shape[0])]
    err = np.abs(got - ref)
    bad = ~(err <= frac * bnd)
    if not bad.any():
        return []
    i = int(np.argmax(np.where(np.isfinite(err), err - frac * bnd, np.inf)))
    return ['%d output(s) beyond the bound; worst at %d: |err| %.3e, bound %.3e' % (int(bad.sum()), i, err[i], frac * bnd[i])]


def ratio(got, ref, bnd):
    """max |err| / bound (0/0 counts as 0), for the printed lines."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err > 0, err / bnd, 0.0)
    return float(q.max())


def pcm_violations(got_pcm, got_f32, ref, bnd):
    """The int16 output against its three rules."""
    bad = []
    got_pcm = np.asarray(got_pcm).astype(np.int64)
    if got_f32 is not None and not np.array_equal(got_pcm, to_pcm(got_f32).astype(np.int64)):
        bad.append('int16 is not saturate(rintf(fp32 output))')
    d = got_pcm - to_pcm(ref).astype(np.int64)
    if np.abs(d).max() > 1:
        bad.append('int16 differs from the rounded float64 value by %d' % np.abs(d).max())
    near_half = np.abs(np.abs(ref - np.floor(ref)) - 0.5) <= bnd
    if (d != 0)[~near_half].any():
        bad.append('int16 differs where float64 is not within the bound of a half-integer (%d samples)' % int((d != 0)[~near_half].sum()))
    return bad


def table_violations(got, up, down):
    """The library's fp32 table against ``table``."""
    h, half = table(up, down)
    got = np.asarray(got, dtype=np.float64)
    if got.shape != h.shape:
        return ['%d taps, the definition has %d' % (got.shape[0], h.shape[0])]
    bad = np.abs(got - h) > EPS * np.abs(h) + 1e-12 * np.abs(h).max()
    return ['%d tap(s) of %d/%d beyond one fp32 rounding' % (int(bad.sum()), up, down)] if bad.any() else []


# ---- the inputs of tests/test_resample_kernels_gpu.py ---------------------------------------------------------------------------------------------
KINDS = ('impulse_first', 'impulse_mid', 'impulse_last', 'constant', 'noise_0.3', 'noise_full')


def signal(kind, L, seed):
    """int16 source of one job.  The impulses read the table out phase by phase; 0.3 of full scale cannot clip (sum |h| over a phase is
    below 3.3), full-scale noise does."""
    x = np.zeros(L, np.int16)
    if kind == 'impulse_first':
        x[0] = 20000
    elif kind == 'impulse_mid':
        x[L // 2] = -20000
    elif kind == 'impulse_last':
        x[L - 1] = 20000
    elif kind == 'constant':
        x[:] = 12000
    else:
        rng = np.random.RandomState(70000 + seed)
        amp = 32767 if kind == 'noise_full' else int(0.3 * 32767)
        x = rng.randint(-amp - (kind == 'noise_full'), amp + 1, size=L).astype(np.int16)
    return x


def grid_jobs(G):
    """The jobs of the GPU test, [(name, up, down, L, first, count, kind, src parity, dst parity)] (G: the kernel's outputs per
    workgroup): every ratio of RATIOS at a source length for each resampled length of 1, 2, G - 1, G, G + 1, 2 G + 1 (the shortest source that
    reaches it: 2/1 has even lengths only), the six kinds of input rotated so that every ratio meets every kind; the two WIDE_RATIOS at
    G + 1; and sixteen sub-range jobs, two per ratio, on sources of 2 G + 1 outputs, whose ends fall on tile edges and mid-tile.  Offsets of
    both parities."""
    jobs = []

    def add(up, down, L, first, count, kind, tag):
        n = len(jobs)
        jobs.append(('%d_%d_%s_%s' % (up, down, tag, kind), up, down, L, first, count, kind, n % 2, (n // 2) % 2))
    targets = (1, 2, G - 1, G, G + 1, 2 * G + 1)
    for r, (up, down) in enumerate(RATIOS):
        for i, target in enumerate(targets):
            L = source_len(target, up, down)
            add(up, down, L, 0, out_len(L, up, down), KINDS[(i + r) % 6], 'n%d' % target)
    for r, (up, down) in enumerate(WIDE_RATIOS):
        L = source_len(G + 1, up, down)
        add(up, down, L, 0, out_len(L, up, down), KINDS[4 + r], 'wide')
    ranges = ((G, G), (G - 1, 2), (517, G), (G, G + 1), (3, 100), (2 * G, 1), (G + 1, G - 1), (0, G),
              (G // 2, G // 2), (1, 2 * G), (G - 3, 7), (2 * G - 1, 2), (G, 1), (255, 258), (G + 64, 129), (0, 1))
    for r, (up, down) in enumerate(RATIOS):
        L = source_len(2 * G + 1, up, down)
        for k in (2 * r, 2 * r + 1):
            first, count = ranges[k]
            assert first + count <= out_len(L, up, down)
            add(up, down, L, first, count, KINDS[4 + k % 2], 'r%d+%d' % (first, count))
    return jobs


def job_signal(job, index):
    return signal(job[6], job[3], index)


def run_jobs(blob, jobs):
    """re2e_wav_resample's jobs on the host, in place (``blob`` int16), in float64: rows (src_off, src_len, up, down, first, count, dst_off)."""
    for src_off, src_len, up, down, first, count, dst_off in jobs:
        assert first + count <= out_len(src_len, up, down)
        blob[dst_off:dst_off + count] = to_pcm(job(blob[src_off:src_off + src_len].copy(), up, down, first, count))
    return blob
