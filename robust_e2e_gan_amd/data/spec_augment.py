"""SpecAugment on the features (Park et al. 2019, in ESPnet's form): the configuration string and the per-batch plan of
``ops.spec_augment`` (csrc/specaug.hip; the plan's layout and ranges are stated in include/re2e.h).  No reference counterpart.

``parse('W,F,nF,T,nT')``: the time-warp window, the widest frequency mask and how many, the widest time mask and how many;
ESPnet's defaults read ``'5,30,2,40,2'``.  ``draw_plan`` draws one row per utterance from a generator seeded by
(seed, step, rank, 3): a random stream apart from the mixture's (seed, epoch, index), the RIRs' (.., 1) and the speeds' (.., 2), which
therefore draw what they drew without augmentation, bit for bit.
"""
import collections

import numpy as np

MAX_MASKS = 8          # include/re2e.h RE2E_SPECAUG_MAX_MASKS

Config = collections.namedtuple('Config', 'W F nF T nT')
_FIELDS = ('W (time-warp window)', 'F (widest frequency mask)', 'nF (frequency masks)', 'T (widest time mask)', 'nT (time masks)')


def parse(text):
    """``'W,F,nF,T,nT'`` -> Config; None, '' and a Config pass through (None for the first two).  Malformed strings are refused by name."""
    if text is None or isinstance(text, Config):
        return text
    if not str(text).strip():
        return None
    parts = [t.strip() for t in str(text).split(',')]
    if len(parts) != 5:
        raise ValueError("spec_augment %r: expected five integers 'W,F,nF,T,nT', e.g. '5,30,2,40,2'" % (text,))
    vals = []
    for name, t in zip(_FIELDS, parts):
        try:
            v = int(t)
        except ValueError:
            raise ValueError('spec_augment %r: %s is not an integer: %r' % (text, name, t))
        if v < 0:
            raise ValueError('spec_augment %r: %s is negative' % (text, name))
        vals.append(v)
    cfg = Config(*vals)
    if cfg.nF > MAX_MASKS or cfg.nT > MAX_MASKS:
        raise ValueError('spec_augment %r: at most %d masks of a kind (nF, nT)' % (text, MAX_MASKS))
    return cfg


def plan_width(cfg):
    return 3 + 2 * cfg.nF + 2 * cfg.nT


def draw_plan(seed, step, rank, lens, F, cfg):
    """(len(lens), 3 + 2 nF + 2 nT) int32: ``[T_r, c, w, f0_1, f_1, .., t0_1, t_1, ..]`` per utterance, a function of
    (seed, step, rank, lens, F, cfg) alone.  Rows in order; per row c ~ U{W .. T_r-W-1} and w ~ U{c-W+1 .. c+W} when W > 0 and T_r > 2W
    (else c = w = 0: no warp), then per frequency mask f ~ U{0 .. min(Fmax, F)}, f0 ~ U{0 .. F-f}, then per time mask
    t ~ U{0 .. min(Tmax, T_r)}, t0 ~ U{0 .. T_r-t}."""
    cfg = parse(cfg)
    rng = np.random.default_rng([int(seed), int(step), int(rank), 3])
    F = int(F)
    plan = np.zeros((len(lens), plan_width(cfg)), dtype=np.int32)
    for r, T in enumerate(int(v) for v in lens):
        row = [T, 0, 0]
        if cfg.W > 0 and T > 2 * cfg.W:
            c = int(rng.integers(cfg.W, T - cfg.W))
            row[1], row[2] = c, int(rng.integers(c - cfg.W + 1, c + cfg.W + 1))
        for _ in range(cfg.nF):
            f = int(rng.integers(0, min(cfg.F, F) + 1))
            row += [int(rng.integers(0, F - f + 1)), f]
        for _ in range(cfg.nT):
            t = int(rng.integers(0, min(cfg.T, T) + 1))
            row += [int(rng.integers(0, T - t + 1)), t]
        plan[r] = row
    return plan


def identity_plan(lens, cfg):
    """The plan that changes nothing: no warp, every mask of width zero."""
    cfg = parse(cfg)
    plan = np.zeros((len(lens), plan_width(cfg)), dtype=np.int32)
    plan[:, 0] = [int(v) for v in lens]
    return plan


def check_plan(plan):
    """The plan as a C-contiguous (R, 3 + 2 nF + 2 nT) int32 array."""
    p = np.ascontiguousarray(np.asarray(plan), dtype=np.int32)
    if p.ndim != 2 or p.shape[1] < 3 or (p.shape[1] - 3) % 2:
        raise ValueError('spec_augment plan: expected (R, 3 + 2 nF + 2 nT) integers, got shape %r' % (p.shape,))
    return p


def validate_plan(plan, Tp, F, nF):
    """Host validation of a plan against the ranges of include/re2e.h (the kernels clamp as well, but a plan that needs clamping is a bug of
    its maker): ValueError naming the first row and value outside its range.  Returns the plan as contiguous int32, and nT."""
    p = check_plan(plan)
    nM = (p.shape[1] - 3) // 2
    nF = int(nF)
    if not 0 <= nF <= nM:
        raise ValueError('spec_augment plan: nF = %d does not fit a row of %d entries' % (nF, p.shape[1]))
    nT = nM - nF
    if nF > MAX_MASKS or nT > MAX_MASKS:
        raise ValueError('spec_augment plan: at most %d masks of a kind' % MAX_MASKS)
    for r, row in enumerate(p.tolist()):
        T, c, w = row[:3]
        if not 0 <= T <= Tp:
            raise ValueError('spec_augment plan row %d: T_r = %d outside 0 .. %d' % (r, T, Tp))
        if c != 0:
            # some window W has W <= c < T_r - W and c - W + 1 <= w <= c + W
            if not (c > 0 and max(c - w + 1, w - c) <= min(c, T - 1 - c)):
                raise ValueError('spec_augment plan row %d: no warp window admits c = %d, w = %d at T_r = %d' % (r, c, w, T))
        for k in range(nF):
            f0, f = row[3 + 2 * k], row[4 + 2 * k]
            if not (0 <= f <= F and 0 <= f0 <= F - f):
                raise ValueError('spec_augment plan row %d: frequency mask %d (f0 = %d, f = %d) outside 0 .. %d' % (r, k, f0, f, F))
        for k in range(nT):
            t0, t = row[3 + 2 * nF + 2 * k], row[4 + 2 * nF + 2 * k]
            if not (0 <= t <= T and 0 <= t0 <= T - t):
                raise ValueError('spec_augment plan row %d: time mask %d (t0 = %d, t = %d) outside 0 .. %d' % (r, k, t0, t, T))
    return p, nT


class Plan(object):
    """A plan with its mask counts: what ``E2E.forward(..., aug=)`` and ``ShareE2E.forward(..., aug=)`` take."""

    def __init__(self, rows, nF):
        self.rows = check_plan(rows)
        self.nF = int(nF)

    @classmethod
    def draw(cls, seed, step, rank, lens, F, cfg):
        cfg = parse(cfg)
        return cls(draw_plan(seed, step, rank, lens, F, cfg), cfg.nF)

    @classmethod
    def identity(cls, lens, cfg):
        cfg = parse(cfg)
        return cls(identity_plan(lens, cfg), cfg.nF)

    def twice(self):
        """The same rows for the two branches of a 2B batch."""
        return Plan(np.concatenate([self.rows, self.rows], 0), self.nF)
