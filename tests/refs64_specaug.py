"""Float64 references of SpecAugment on the features (csrc/specaug.hip; the contract is in include/re2e.h) and the inputs of
tests/test_specaug_kernels_gpu.py.

Plain torch and numpy on the CPU, nothing imported from the product or from ``oracle``.

* ``specaug_ref``: the yardstick.  Each segment of the time warp is resized by ``torch.nn.functional.interpolate(mode='bicubic',
  align_corners=False)`` ITSELF, the masks are written out, and dx comes from autograd.  ``dtype=torch.float32`` runs the same code in fp32:
  how far fp32 arithmetic alone is from float64 on a given input (``margin_ok``).
* ``specaug_restated``: the integer restatement of the contract -- N = (2t+1) n_in - n_out, D = 2 n_out, i0 = floor(N / D), tau = (N - i0 D) / D,
  taps i0-1 .. i0+2 clamped, cubic-convolution weights with A = -0.75 -- and, for dx, the GATHER the contract asks for: every source frame sums
  the contiguous run of output frames whose clamped taps hit it, the run found by inverting i0(t) in integers (``taps_range``).  A second
  derivation of both directions, pinned to the first by tests/test_refs64_specaug_cpu.py.
* ``clamp_plan``: what the kernels make of a plan whose values lie outside their ranges.
* ``cases``: the shapes and plans, the smallest at which each branch of the kernels can go wrong.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F_

from refs64 import margin_ok, rel_err          # noqa: F401  (re-exported)
from refs64_feat import BAR_FBANK_GRAD, BAR_FBANK_OUT      # noqa: F401  (the bars the issue sets: forward 1e-5, backward 1e-4 of the max)

A = -0.75
SENTINEL = 7.25          # what the padding frames of x and dy hold: it must come through unchanged


def plan_width(nF, nT):
    return 3 + 2 * nF + 2 * nT


def clamp_plan(plan, Tp, F, nF, nT):
    """The plan the kernels act on (include/re2e.h): every value clamped into its range."""
    p = np.array(plan, dtype=np.int64).reshape(-1, plan_width(nF, nT)).copy()
    for r in p:
        T = r[0] = min(max(r[0], 0), Tp)
        if r[1] <= 0 or T < 2:
            r[1] = r[2] = 0
        else:
            r[1] = min(r[1], T - 1)
            r[2] = min(max(r[2], 1), T - 1)
        for k in range(nF):
            f0 = r[3 + 2 * k] = min(max(r[3 + 2 * k], 0), F)
            r[4 + 2 * k] = min(max(r[4 + 2 * k], 0), F - f0)
        for k in range(nT):
            t0 = r[3 + 2 * nF + 2 * k] = min(max(r[3 + 2 * nF + 2 * k], 0), T)
            r[4 + 2 * nF + 2 * k] = min(max(r[4 + 2 * nF + 2 * k], 0), T - t0)
    return p.astype(np.int32)


def _keep_mask(row, T, F, nF, nT):
    """(T, F) bool: True where a valid cell survives the masks."""
    keep = np.ones((T, F), dtype=bool)
    for k in range(nF):
        f0, f = int(row[3 + 2 * k]), int(row[4 + 2 * k])
        keep[:, f0:f0 + f] = False
    for k in range(nT):
        t0, t = int(row[3 + 2 * nF + 2 * k]), int(row[4 + 2 * nF + 2 * k])
        keep[t0:t0 + t, :] = False
    return torch.from_numpy(keep)


def _resize(seg, n_out):
    """(n_in, F) -> (n_out, F) as F.interpolate resizes an image of n_in x F pixels to n_out x F."""
    return F_.interpolate(seg[None, None], size=(n_out, seg.shape[1]), mode='bicubic', align_corners=False)[0, 0]


def specaug_ref(x, plan, nF, nT, dy=None, dtype=torch.float64):
    """x (R, Tp, F), plan (R, P) within its ranges -> (y, dx or None)."""
    R, Tp, F = x.shape
    xx = x.detach().to(dtype).clone().requires_grad_(dy is not None)
    rows = []
    for r in range(R):
        p = [int(v) for v in plan[r]]
        T, c, w = p[0], p[1], p[2]
        v = xx[r, :T]
        if c > 0:
            v = torch.cat([_resize(v[:c], w), _resize(v[c:], T - w)], 0)
        v = torch.where(_keep_mask(p, T, F, nF, nT), v, torch.zeros((), dtype=dtype))
        rows.append(torch.cat([v, xx[r, T:]], 0))
    y = torch.stack(rows, 0)
    if dy is None:
        return y.detach(), None
    y.backward(dy.detach().to(dtype))
    return y.detach(), xx.grad


def taps(n_in, n_out, t, dtype=torch.float64):
    """Output frame t of a segment n_in -> n_out: ([4 clamped source frames], [4 weights]) by the contract's integer formula."""
    N, D = (2 * t + 1) * n_in - n_out, 2 * n_out
    i0 = N // D                                            # Python's // is the floor
    num, den = torch.tensor(N - i0 * D, dtype=dtype), torch.tensor(D, dtype=dtype)
    tau = num / den                                        # ONE division in the working precision
    one = torch.ones((), dtype=dtype)

    def conv1(v):
        return ((A + 2) * v - (A + 3)) * v * v + 1

    def conv2(v):
        return ((A * v - 5 * A) * v + 8 * A) * v - 4 * A
    wts = [conv2(tau + one), conv1(tau), conv1(one - tau), conv2((one - tau) + one)]
    return [min(max(i0 - 1 + k, 0), n_in - 1) for k in range(4)], wts


def first_with_i0_at_least(a, n_in, n_out):
    """Smallest output frame t of a segment with i0(t) >= a, clamped to 0 .. n_out:  (2t+1) n_in >= (2a+1) n_out."""
    q = -((-(2 * a + 1) * n_out) // n_in)                  # ceil((2a+1) n_out / n_in): 2t+1 >= q
    return min(max(q // 2, 0), n_out)


def taps_range(n_in, n_out, j):
    """The output frames [lo, hi) of a segment whose clamped taps hit its source frame j (the taps of t are i0-1 .. i0+2, so
    j-2 <= i0 <= j+1; frame 0 also takes every tap clamped from below, frame n_in-1 every tap clamped from above)."""
    lo = 0 if j == 0 else first_with_i0_at_least(j - 2, n_in, n_out)
    hi = n_out if j == n_in - 1 else first_with_i0_at_least(j + 2, n_in, n_out)
    return lo, hi


def _segments(T, c, w):
    """[(first source frame, n_in, first output frame, n_out)] of a row."""
    return [(0, T, 0, T)] if c == 0 else [(0, c, 0, w), (c, T - c, w, T - w)]


def specaug_restated(x, plan, nF, nT, dy=None, dtype=torch.float64):
    """The contract of include/re2e.h written out: the forward by taps, dx as a gather over ``taps_range`` in ascending (t, k)."""
    R, Tp, F = x.shape
    xx = x.detach().to(dtype)
    y = xx.clone()
    dx = dy.detach().to(dtype).clone() if dy is not None else None
    for r in range(R):
        p = [int(v) for v in plan[r]]
        T, c, w = p[0], p[1], p[2]
        keep = _keep_mask(p, T, F, nF, nT)
        desc = {}
        for base, n_in, obase, n_out in _segments(T, c, w):
            for t in range(n_out):
                if n_in == n_out:
                    y[r, obase + t] = xx[r, base + t]
                    desc[obase + t] = ([base + t], [torch.ones((), dtype=dtype)])
                    continue
                idx, wts = taps(n_in, n_out, t, dtype)
                acc = torch.zeros(F, dtype=dtype)
                for i, wt in zip(idx, wts):
                    acc = acc + wt * xx[r, base + i]
                y[r, obase + t] = acc
                desc[obase + t] = ([base + i for i in idx], wts)
        y[r, :T] = torch.where(keep, y[r, :T], torch.zeros((), dtype=dtype))
        if dy is None:
            continue
        g = torch.where(keep, dx[r, :T], torch.zeros((), dtype=dtype)).clone()      # masked cells contribute nothing
        for base, n_in, obase, n_out in _segments(T, c, w):
            for j in range(n_in):
                lo, hi = (j, j + 1) if n_in == n_out else taps_range(n_in, n_out, j)
                acc = torch.zeros(F, dtype=dtype)
                for t in range(obase + lo, obase + hi):
                    for i, wt in zip(*desc[t]):
                        if i == base + j:
                            acc = acc + wt * g[t]
                dx[r, base + j] = acc
    return y, dx


def full_jacobian_hits(n_in, n_out, j):
    """The output frames whose clamped taps hit source frame j, by enumeration (what ``taps_range`` must equal as a range)."""
    return [t for t in range(n_out) if j in taps(n_in, n_out, t)[0]]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _row(T, c, w, fm=(), tm=()):
    return [T, c, w] + [v for m in fm for v in m] + [v for m in tm for v in m]


def cases(fwd_tile=32, bwd_tile=32):
    """name -> dict(shape=(R, Tp, F), nF, nT, plan (R, P) int32, exact=bool, clamp=bool).  W = 5 throughout.  ``exact``: no row warps, or
    every warped segment keeps its length: y (and dx, where no mask applies) is a copy, bit for bit.  ``clamp``: the plan lies outside its
    ranges; the reference runs on ``clamp_plan`` of it."""
    out = {}

    def add(name, shape, nF, nT, rows, exact=False, clamp=False):
        plan = np.array(rows, dtype=np.int32).reshape(shape[0], plan_width(nF, nT))
        out[name] = dict(shape=shape, nF=nF, nT=nT, plan=plan, exact=exact, clamp=clamp)

    # vector and scalar feature widths: two rows, one ragged, warp + two frequency and two time masks each
    for F in (1, 3, 4, 80, 83):
        fa, fb = max(1, F // 8), max(1, F // 3)
        add('width_F%d' % F, (2, 40, F), 2, 2,
            [_row(40, 17, 21, [(0, fa), (F - fb, fb)], [(3, 4), (30, 6)]), _row(33, 9, 5, [(F // 2, fa), (F // 2, fb // 2)], [(0, 2), (31, 2)])])
    # the warp boundary, W = 5
    add('T_2W_no_warp', (1, 10, 8), 0, 0, [_row(10, 0, 0)], exact=True)
    add('T_2W1_w1', (1, 11, 8), 0, 0, [_row(11, 5, 1)])
    add('T_2W1_w2W', (1, 11, 8), 0, 0, [_row(11, 5, 10)])
    add('T_2W1_identity', (1, 11, 8), 0, 0, [_row(11, 5, 5)], exact=True)
    add('T_1', (2, 3, 5), 1, 1, [_row(1, 0, 0, [(1, 2)], [(0, 0)]), _row(1, 0, 0, [(0, 0)], [(0, 1)])])
    add('Tp_1', (1, 1, 4), 0, 0, [_row(1, 0, 0)], exact=True)
    # ragged rows, sentinel in the padding
    add('ragged', (3, 50, 12), 1, 1, [_row(50, 20, 24, [(2, 3)], [(40, 5)]), _row(37, 6, 2, [(0, 1)], [(10, 10)]), _row(12, 5, 9, [(11, 1)], [(0, 3)])])
    # tiling: one frame past one tile, two full tiles, of each kernel's frame tiling
    for tile in sorted({fwd_tile, bwd_tile}):
        add('tile%d_plus1' % tile, (2, tile + 1, 8), 1, 1,
            [_row(tile + 1, tile - 6, tile - 2, [(1, 2)], [(tile - 1, 2)]), _row(tile, 7, 11, [(6, 2)], [(0, 1)])])
        add('tile%d_x2' % tile, (2, 2 * tile, 8), 1, 1,
            [_row(2 * tile, tile, tile + 4, [(1, 2)], [(tile - 2, 4)]), _row(2 * tile - 1, tile + 3, tile - 1, [(6, 2)], [(2 * tile - 3, 2)])])
    # masks
    add('no_masks', (2, 30, 8), 0, 0, [_row(30, 12, 8), _row(25, 5, 10)])
    add('zero_width', (1, 30, 8), 2, 2, [_row(30, 12, 15, [(3, 0), (8, 0)], [(0, 0), (30, 0)])])
    add('full_F', (2, 30, 8), 1, 0, [_row(30, 12, 15, [(0, 8)]), _row(21, 0, 0, [(0, 8)])])
    add('time_overlap', (1, 30, 8), 0, 2, [_row(30, 12, 15, [], [(10, 8), (14, 9)])])
    add('time_to_T', (2, 30, 8), 0, 1, [_row(30, 12, 15, [], [(25, 5)]), _row(22, 6, 4, [], [(20, 2)])])
    # plans outside their ranges: clamped, and in bounds.  Row 3 (1 -> 199 frames) makes one source frame of the backward sum more output frames
    # than a workgroup stages.
    add('clamped', (4, 200, 8), 1, 1,
        [_row(999, 500, -7, [(-3, 5)], [(150, 400)]), _row(-5, 3, 3, [(9, 9)], [(-1, -1)]), _row(60, 59, 1000, [(6, 50)], [(70, 5)]),
         _row(200, 1, 199, [(2, -4)], [(-20, 30)])], clamp=True)
    return out


def _smooth(R, Tp, F, g):
    """Two slow sinusoids along time per (row, feature), periods of 120 frames and more at random phase and amplitude."""
    t = torch.arange(float(Tp))[None, :, None]
    per, ph, amp = 120 + 400 * torch.rand(R, 1, F, generator=g), 6.28 * torch.rand(R, 1, F, generator=g), 0.5 + torch.rand(R, 1, F, generator=g)
    return amp * torch.sin(2 * math.pi * t / per + ph) + 0.3 * amp * torch.sin(2 * math.pi * t / (0.37 * per) + 2 * ph)


def case_tensors(case, seed=0, want_dy=True, smooth=False):
    """x and dy of a case: standard normal on the valid frames, SENTINEL on the padding (valid by the CLAMPED plan).
    ``smooth``: slowly varying along time instead, as filterbank features are.  The fp32 yardstick is ``F.interpolate`` in fp32, which places
    its taps by (t + 0.5) scale - 0.5 in fp32: at several hundred frames that position is off by 1e-4 of a frame, and on white noise, whose
    neighbouring frames differ by more than its standard deviation, the fp32 run alone then uses up the forward bar (4.1e-5 of the max at
    (32, 800, 80)) and the backward bar's quarter (2.9e-5).  The production-shape case therefore changes its DATA, not its bars."""
    R, Tp, F = case['shape']
    g = torch.Generator().manual_seed(1000 + seed)
    x = _smooth(R, Tp, F, g) if smooth else torch.randn(R, Tp, F, generator=g)
    dy = _smooth(R, Tp, F, g) if smooth else torch.randn(R, Tp, F, generator=g)
    plan = clamp_plan(case['plan'], Tp, F, case['nF'], case['nT'])
    for r in range(R):
        x[r, int(plan[r, 0]):] = SENTINEL
        dy[r, int(plan[r, 0]):] = -SENTINEL
    return x, (dy if want_dy else None), plan
