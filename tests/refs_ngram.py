"""The definition the n-gram LM (robust_e2e_gan_amd/model/ngram.py, csrc/ngram.hip) is checked against: Katz back-off in its dictionary
form, pure Python in float64, and a generator of random prefix-closed, PRUNED models (a suffix of an n-gram need not be an n-gram) that writes
real ARPA text.  Nothing here knows about nodes or flat arrays.

A model is ``grams[k-1] = {(l1, .., lk): (log10 p, log10 back-off)}`` over integer labels, values exactly what the ARPA text holds (six
decimals), so that the scorer and a reader of the file start from the same doubles."""
import math

import numpy as np

LN10 = math.log(10.0)
LOGZERO = -10000000000.0


def score(grams, history, w, unk=None):
    """(ln p(w | history), the |terms| that were added): the longest context first; a context that does not hold ``w`` adds its back-off
    (0 when the context is no n-gram).  ``history``: the labels before ``w``, any length.  A label without a unigram is ``unk`` (everywhere);
    without an ``unk`` it scores LOGZERO."""
    order = len(grams)
    canon = lambda v: v if (v,) in grams[0] else unk
    w = canon(w)
    h = tuple(history)[-(order - 1):] if order > 1 else ()
    cut = max([i + 1 for i, v in enumerate(h) if canon(v) is None] or [0])       # nothing is known behind a label the model cannot name
    h = tuple(canon(v) for v in h[cut:])
    acc, terms = 0.0, []
    for k in range(len(h), -1, -1):
        ctx = h[len(h) - k:]
        g = ctx + (w,)
        if w is None and k == 0:                 # no unigram and no <unk>: the floor stands in for the unigram
            return acc + LOGZERO, terms + [abs(LOGZERO)]
        if g in grams[len(g) - 1]:
            lp = grams[len(g) - 1][g][0] * LN10
            return acc + lp, terms + [abs(lp)]
        if k > 0 and ctx in grams[k - 1]:
            bo = grams[k - 1][ctx][1] * LN10
            acc += bo
            terms.append(abs(bo))
    raise AssertionError('a label with a unigram always ends the loop')


def depth(grams, history, w):
    """How many contexts were backed off from before ``w`` was found, counted from the longest suffix of ``history`` that is an n-gram of at
    most order - 1 labels (the state a decoder holds)."""
    order = len(grams)
    h = tuple(history)[-(order - 1):] if order > 1 else ()
    while h and h not in grams[len(h) - 1]:
        h = h[1:]
    n = 0
    for k in range(len(h), -1, -1):
        ctx = h[len(h) - k:]
        if ctx + (w,) in grams[k]:
            return n
        if k == 0 or ctx in grams[k - 1]:
            n += 1
    raise AssertionError('a label with a unigram always ends the loop')


def longest_suffix(grams, history):
    """The longest suffix of ``history`` of at most order - 1 labels that is an n-gram (a tuple; () for none)."""
    order = len(grams)
    h = tuple(history)[-(order - 1):] if order > 1 else ()
    while h and h not in grams[len(h) - 1]:
        h = h[1:]
    return h


def random_model(V, densities, seed, no_unigram=0.0, suffix_share=0.0):
    """A random prefix-closed model over labels 0 .. V-1: ``densities[k-1]`` = the chance that a (k-1)-gram is extended by a given label (entry 0
    is ignored: every label has a unigram, except a share ``no_unigram`` of them).  Extensions are drawn per PREFIX, so a suffix of an n-gram
    is missing as often as the densities say: the model is pruned.  ``suffix_share``: for that share of the n-grams the suffix is added as well
    (with its own prefixes and suffixes), as in a model that was estimated from counts: back-off chains of every length.  Values carry six
    decimals."""
    rng = np.random.default_rng(seed)
    order = len(densities)
    r6 = lambda v: float('%.6f' % v)
    labels = [v for v in range(V) if v == V - 1 or rng.random() >= no_unigram]          # the last label (eos) always has one
    grams = [{(v,): (r6(-rng.uniform(0.3, 3.0)), r6(-rng.uniform(0.0, 1.5)) if order > 1 else 0.0) for v in labels}]
    for k in range(2, order + 1):
        level = {}
        for ctx in grams[-1]:
            m = int(rng.binomial(len(labels), densities[k - 1]))                         # (the count, then which: the same law as a coin per label)
            for i in (rng.choice(len(labels), size=m, replace=False).tolist() if m else ()):
                level[ctx + (labels[i],)] = (r6(-rng.uniform(0.05, 2.5)), r6(-rng.uniform(0.0, 1.5)) if k < order else 0.0)
        grams.append(level)
    value = lambda k: (r6(-rng.uniform(0.05, 2.5)), r6(-rng.uniform(0.0, 1.5)) if k < order else 0.0)

    def ensure(g):
        if g not in grams[len(g) - 1]:
            ensure(g[:-1]), ensure(g[1:])
            grams[len(g) - 1][g] = value(len(g))

    if suffix_share > 0.0:
        for k in range(3, order + 1):
            for g in sorted(grams[k - 1]):
                if rng.random() < suffix_share:
                    ensure(g[1:])
    return grams


def write_arpa(path, grams, name=str, drop_zero_backoff=True):
    """The model as ARPA text; ``name(label)`` is the token of a label.  A back-off of exactly 0 is left out, as the tools that write ARPA do."""
    order = len(grams)
    lines = ['', '\\data\\'] + ['ngram %d=%d' % (k, len(grams[k - 1])) for k in range(1, order + 1)]
    for k in range(1, order + 1):
        lines += ['', '\\%d-grams:' % k]
        for g in sorted(grams[k - 1]):
            lp, bo = grams[k - 1][g]
            line = '%.6f\t%s' % (lp, ' '.join(name(v) for v in g))
            if k < order and not (drop_zero_backoff and bo == 0.0):
                line += '\t%.6f' % bo
            lines.append(line)
    lines += ['', '\\end\\', '']
    with open(path, 'w', encoding='utf-8') as f:
        f.write('\n'.join(lines))
    return path
