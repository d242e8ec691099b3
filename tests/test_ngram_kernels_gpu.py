"""csrc/ngram.hip (re2e_ngram_step, re2e_ngram_score_seqs) against the host arbiter ``NgramTables.step_host`` -- log-probabilities, shallow-fusion
sums and states bit for bit -- and against the dictionary form of Katz back-off in float64 (tests/refs_ngram.py) within
(order + 1) * 2^-24 * sum |terms|: one rounding of every term to fp32 and at most ``order`` fp32 additions.  Every output buffer starts as NaN.

The kernel cuts a row into tiles of 4096 labels and writes each tile with 16-byte stores over its aligned middle: V = 1, 7, 64, 65 and 1031 sit
in one tile with every head / tail length, V = 4233 (the recipe's) and 8200 span two and three tiles."""
import math
import os

import numpy as np
import pytest
import torch

import refs_ngram as R
from robust_e2e_gan_amd.model.ngram import NgramTables

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24
_MODELS = {}


def _model(order, V, tmp):
    """(grams, tables, device tensors) of a random pruned model, built once per (order, V).  Densities fall with V so that a level holds a few
    thousand n-grams at most; label V - 2 is given every label as a successor (a full list), label V - 1 none (an empty one)."""
    key = (order, V)
    if key not in _MODELS:
        dens = [0.0, min(0.5, 4.0 / V)][:order] + [min(0.4, 1.3 / V)] * max(0, order - 2)
        grams = R.random_model(V, dens, 1000 * order + V, suffix_share=0.7 if order <= 5 else 0.25)
        if order > 1:
            rng = np.random.default_rng(V)
            full, empty = (max(V - 2, 0),), (V - 1,)
            for v in range(V):
                if V > 1:
                    grams[1].pop(empty + (v,), None)
                grams[1].setdefault(full + (v,), (float('%.6f' % -rng.uniform(0.05, 2.5)), float('%.6f' % -rng.uniform(0.0, 1.5)) if order > 2 else 0.0))
            for k in range(2, order):                             # keep the model prefix-closed after the removal
                grams[k] = {g: val for g, val in grams[k].items() if g[:-1] in grams[k - 1]}
        path = R.write_arpa(os.path.join(tmp, 'k%d_%d.arpa' % (order, V)), grams)
        t = NgramTables.from_arpa(path, [str(v) for v in range(V)], 'ids')
        _MODELS[key] = (grams, t, {k: v.to(DEV) for k, v in t.tensors().items()})
    return _MODELS[key]


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp('ngram'))


def _nan(*shape, dtype=torch.float32, offset=0):
    """A NaN-filled (int: -77-filled) buffer whose first element sits ``offset`` elements behind a 256-byte boundary."""
    n = int(np.prod(shape))
    flat = torch.full((n + offset,), float('nan') if dtype.is_floating_point else -77, dtype=dtype, device=DEV)
    return flat[offset:].view(*shape)


def _step(t, dev, state, x, att=None, w=0.0, offset=0):
    from robust_e2e_gan_amd.lib import call
    n, V = len(x), t.n_vocab
    x_d = torch.from_numpy(np.asarray(x, np.int32)).to(DEV)
    s_d = torch.from_numpy(np.asarray(state, np.int32)).to(DEV) if state is not None else None
    new, lp = _nan(n, dtype=torch.int32), _nan(n, V, offset=offset)
    att_d = comb = None
    if att is not None:
        att_d = _nan(n, V, offset=offset)
        att_d.copy_(torch.from_numpy(att))
        comb = _nan(n, V, offset=offset)
    call('re2e_ngram_step', *t.table_args(dev), s_d.data_ptr() if s_d is not None else None, x_d.data_ptr(), n,
         att_d.data_ptr() if att_d is not None else None, float(np.float32(w)), new.data_ptr(), lp.data_ptr(), comb.data_ptr() if comb is not None else None)
    torch.cuda.synchronize()
    return new.cpu().numpy(), lp.cpu().numpy(), (comb.cpu().numpy() if comb is not None else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want) if want.dtype == np.float32 else np.zeros(want.shape, bool)
    assert (np.isnan(got) == nan).all() if want.dtype == np.float32 else True, what
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), '%s: %d of %d elements differ, first at %s' % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())


def _host_comb(att, w, lp):
    return att + np.float32(w) * lp                               # fp32 product, then fp32 sum


SHAPES = [(1, 1, 1), (1, 7, 2), (1, 1031, 65), (2, 1, 2), (2, 7, 64), (2, 64, 65), (2, 65, 200), (3, 7, 65), (3, 64, 1), (3, 65, 64), (3, 1031, 200),
          (5, 7, 200), (5, 64, 2), (5, 65, 65), (5, 1031, 64), (8, 7, 64), (8, 65, 2), (8, 1031, 65), (3, 4233, 12), (3, 8200, 3)]


@pytest.mark.parametrize('order,V,n', SHAPES)
def test_step_chain_is_bitwise_the_host_arbiter_and_katz_backoff(tmp, order, V, n):
    """order + 3 positions from ``state_in`` NULL with a parent gather between positions (rows repeated and dropped); ``att`` is given at the odd
    positions and NULL at the even ones.  lp, comb and the states equal step_host bit for bit; a sample of rows is scored by the dictionary
    scorer and the depth of every sampled label is counted: every depth 0 .. min(order, 5) - 1 must have been seen (V > 1)."""
    grams, t, dev = _model(order, V, tmp)
    rng = np.random.default_rng(order * 100000 + V * 100 + n)
    parents = (np.arange(n) * 2) // 3 if n > 2 else np.arange(n)
    special = [v for v in (V - 2, V - 1) if v >= 0]
    state_d = state_h = None
    hists = [[] for _ in range(n)]
    depths = np.zeros(order, np.int64)
    for pos in range(order + 3):
        if pos:
            state_d, state_h, hists = state_d[parents], state_h[parents], [list(hists[p]) for p in parents]
        x = rng.integers(0, V, size=n)
        for r in range(n if pos else 0):                          # mostly follow an n-gram of the model, so that deep contexts are reached
            a, b = int(t.succ_off[state_h[r]]), int(t.succ_off[state_h[r] + 1])
            if b > a and rng.random() < 0.7:
                x[r] = t.succ_label[rng.integers(a, b)]
        x[rng.random(n) < 0.15] = special[pos % len(special)]     # the full and the empty successor lists are visited often
        att = rng.standard_normal((n, V)).astype(np.float32) if pos % 2 else None
        w = 0.3 + 0.1 * pos
        new_d, lp_d, comb_d = _step(t, dev, state_d, x, att, w)
        new_h, lp_h = t.step_host(state_h, x)
        _same_bits(new_d, new_h, 'state at position %d' % pos)
        _same_bits(lp_d, lp_h, 'lp at position %d' % pos)
        if att is not None:
            _same_bits(comb_d, _host_comb(att, w, lp_h), 'comb at position %d' % pos)
        else:
            assert comb_d is None
        for r in range(n):
            hists[r].append(int(x[r]))
        dense = set(rng.integers(0, n, size=min(n, 4)).tolist())                  # a few rows over many labels, every row over two
        for r in range(n):
            for v in sorted(set(rng.integers(0, V, size=min(V, 24) if r in dense else 2).tolist() + (special if r in dense else []))):
                ref, terms = R.score(grams, hists[r], v)
                assert abs(float(lp_d[r, v]) - ref) <= (order + 1) * EPS * sum(terms), (pos, r, v, float(lp_d[r, v]), ref)
                depths[R.depth(grams, hists[r], v)] += 1
        state_d, state_h = new_d, new_h
    print('order=%d V=%d n=%d: nodes %d, successors %d, sampled depths %s' % (order, V, n, t.n_nodes, t.n_succ, depths.tolist()))
    if V > 1:
        assert (depths[:min(order, 5)] > 0).all(), depths         # (the three deepest of order 8: test_every_backoff_depth_of_an_order_8_model)


def test_every_backoff_depth_of_an_order_8_model(tmp):
    """A model made for it: every substring (up to 8 labels) of the chain 0 1 2 3 4 5 6 0, and for j = 1 .. 6 a label 8 + j that only the context
    of the last j labels holds.  After the first seven labels the state is the 7-label context; label 0 is found at depth 0, label 8 + j at
    depth 7 - j, label 7 only at the root (depth 7): all eight levels of the chain, the longest an order-8 model has."""
    V, chain = 16, [0, 1, 2, 3, 4, 5, 6, 0]
    rng = np.random.default_rng(8)
    val = lambda k: (float('%.6f' % -rng.uniform(0.05, 2.5)), float('%.6f' % -rng.uniform(0.1, 1.5)) if k < 8 else 0.0)
    grams = [{} for _ in range(8)]
    for v in range(V):
        grams[0][(v,)] = val(1)
    for a in range(len(chain)):
        for b in range(a + 2, len(chain) + 1):
            grams[b - a - 1].setdefault(tuple(chain[a:b]), val(b - a))
    ctx = tuple(chain[:7])
    for j in range(1, 7):
        grams[j][ctx[7 - j:] + (8 + j,)] = val(j + 1)
    t = NgramTables.from_arpa(R.write_arpa(os.path.join(tmp, 'deep.arpa'), grams), [str(v) for v in range(V)], 'ids')
    dev = {k: v.to(DEV) for k, v in t.tensors().items()}
    state_d = state_h = None
    for x in chain[:7]:
        state_d, lp_d, _ = _step(t, dev, state_d, [x, x])
        state_h, lp_h = t.step_host(state_h, [x, x])
        _same_bits(state_d, state_h, 'state')
        _same_bits(lp_d, lp_h, 'lp')
    want = {0: 0, 7: 7}
    want.update({8 + j: 7 - j for j in range(1, 7)})
    for v, d in want.items():
        assert R.depth(grams, chain[:7], v) == d, (v, d)
        ref, terms = R.score(grams, chain[:7], v)
        assert len(terms) == d + 1 and abs(float(lp_d[0, v]) - ref) <= 9 * EPS * sum(terms), (v, float(lp_d[0, v]), ref)
    state_d, lp_d, _ = _step(t, dev, state_d, [0, 7])             # row 0 moves on to the context 1 2 3 4 5 6 0, row 1 falls to the unigram 7
    state_h, lp_h = t.step_host(state_h, [0, 7])
    _same_bits(state_d, state_h, 'state')
    _same_bits(lp_d, lp_h, 'lp')
    assert state_h[0] != state_h[1] and state_h[1] == t.uni_next[7]


def test_rows_permuted_give_permuted_outputs_and_two_runs_are_equal(tmp):
    grams, t, dev = _model(5, 1031, tmp)
    rng = np.random.default_rng(5)
    n = 65
    state = None
    for pos in range(4):                                          # reach deep states first
        x = rng.integers(0, 1031, size=n)
        state, _, _ = _step(t, dev, state, x)
    x = rng.integers(0, 1031, size=n)
    att = rng.standard_normal((n, 1031)).astype(np.float32)
    a = _step(t, dev, state, x, att, 0.7)
    b = _step(t, dev, state, x, att, 0.7)
    perm = rng.permutation(n)
    c = _step(t, dev, state[perm], x[perm], att[perm], 0.7)
    one = _step(t, dev, state[3:4], x[3:4], att[3:4], 0.7)       # the same row alone: n does not enter its bits
    for k, what in enumerate(('state', 'lp', 'comb')):
        _same_bits(b[k], a[k], 'second run: ' + what)
        _same_bits(c[k], a[k][perm], 'permuted rows: ' + what)
        _same_bits(one[k], a[k][3:4], 'row alone: ' + what)
    assert len(set(a[0].tolist())) > 8                            # the rows really differ


@pytest.mark.parametrize('V', [7, 65, 4233])
def test_bad_rows_are_nan_and_their_neighbours_untouched(tmp, V):
    """A state outside [0, N) or a label outside [0, V): NaN scores (and sums) and state -1 for that row only."""
    grams, t, dev = _model(3, V, tmp)
    rng = np.random.default_rng(V)
    n = 9
    state, _, _ = _step(t, dev, None, rng.integers(0, V, size=n))
    x = rng.integers(0, V, size=n)
    att = rng.standard_normal((n, V)).astype(np.float32)
    good = _step(t, dev, state, x, att, 0.5)
    bad_state, bad_x = state.copy(), x.copy()
    bad_state[1], bad_state[4], bad_x[6], bad_x[8] = t.n_nodes, -1, V, -3
    got = _step(t, dev, bad_state, bad_x, att, 0.5)
    host_state, host_lp = t.step_host(bad_state, bad_x)
    bad = np.zeros(n, bool)
    bad[[1, 4, 6, 8]] = True
    assert (got[0][bad] == -1).all() and np.isnan(got[1][bad]).all() and np.isnan(got[2][bad]).all()
    assert (host_state[bad] == -1).all() and np.isnan(host_lp[bad]).all()
    for k, what in enumerate(('state', 'lp', 'comb')):
        _same_bits(got[k][~bad], good[k][~bad], 'neighbours: ' + what)


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('V', [1, 7, 65, 4233])
def test_unaligned_outputs(tmp, V, offset):
    """lp, att and comb 4, 8 and 12 bytes off a 16-byte boundary: the scalar ends of the wide-store form; with an odd V every row starts at
    another misalignment anyway."""
    grams, t, dev = _model(2 if V == 1 else 3, V, tmp)
    rng = np.random.default_rng(V + offset)
    n = 5
    x = rng.integers(0, V, size=n)
    att = rng.standard_normal((n, V)).astype(np.float32)
    want = _step(t, dev, None, x, att, 0.25)
    got = _step(t, dev, None, x, att, 0.25, offset=offset)
    for k, what in enumerate(('state', 'lp', 'comb')):
        _same_bits(got[k], want[k], what)
    _same_bits(got[1], t.step_host(None, x)[1], 'lp against the host')


def test_att_and_comb_misaligned_against_each_other(tmp):
    from robust_e2e_gan_amd.lib import call
    grams, t, dev = _model(3, 65, tmp)
    n, V = 4, 65
    x = np.asarray([1, 5, 64, 63], np.int32)
    att = np.random.default_rng(0).standard_normal((n, V)).astype(np.float32)
    att_d = _nan(n, V, offset=1)
    att_d.copy_(torch.from_numpy(att))
    new, lp, comb = _nan(n, dtype=torch.int32), _nan(n, V), _nan(n, V, offset=2)
    call('re2e_ngram_step', *t.table_args(dev), None, torch.from_numpy(x).to(DEV).data_ptr(), n, att_d.data_ptr(), 0.5, new.data_ptr(), lp.data_ptr(),
         comb.data_ptr())
    host = t.step_host(None, x)
    _same_bits(lp.cpu().numpy(), host[1], 'lp')
    _same_bits(comb.cpu().numpy(), _host_comb(att, 0.5, host[1]), 'comb')


def test_arguments_are_checked(tmp):
    from robust_e2e_gan_amd.lib import Re2eError, call
    grams, t, dev = _model(2, 7, tmp)
    x = torch.zeros(2, dtype=torch.int32, device=DEV)
    new, lp = _nan(2, dtype=torch.int32), _nan(2, 7)
    with pytest.raises(Re2eError):                                # att without comb_out
        call('re2e_ngram_step', *t.table_args(dev), None, x.data_ptr(), 2, lp.data_ptr(), 0.5, new.data_ptr(), lp.data_ptr(), None)
    with pytest.raises(Re2eError):
        call('re2e_ngram_step', *t.table_args(dev)[:-1], 9, None, x.data_ptr(), 2, None, 0.5, new.data_ptr(), lp.data_ptr(), None)      # order 9
    with pytest.raises(Re2eError):
        call('re2e_ngram_step', *t.table_args(dev), None, x.data_ptr(), 0, None, 0.5, new.data_ptr(), lp.data_ptr(), None)


@pytest.mark.parametrize('order,V', [(1, 7), (3, 65), (5, 1031)])
def test_score_seqs(tmp, order, V):
    """Lengths 0, 1, order and Lmax (= 2 * order + 3) and a few between, with and without the final eos, against the sum of the dictionary
    scorer's terms within 1e-12 * sum |terms| plus the fp32 bound of the terms themselves; and against the host's fp32 terms added in double,
    exactly."""
    grams, t, dev = _model(order, V, tmp)
    rng = np.random.default_rng(order + V)
    Lmax = 2 * order + 3
    lens = [0, 1, order, Lmax, 2, Lmax - 1, order + 1] + rng.integers(0, Lmax + 1, size=70).tolist()
    seqs = [rng.integers(0, V, size=L).tolist() for L in lens]
    eos = V - 1
    for append in (True, False):
        got = t.score_seqs(seqs, torch.device(DEV), append_eos=append)
        assert got.dtype == np.float64 and got.shape == (len(seqs),)
        for q, seq in enumerate(seqs):
            full = list(seq) + ([eos] if append else [])
            terms32 = t.score_host(seq, append)
            host = 0.0
            for v in terms32:
                host += float(v)
            assert got[q] == host, (q, got[q], host)
            ref, mass, fp32_bound = 0.0, 0.0, 0.0
            for i, v in enumerate(full):
                lp, terms = R.score(grams, [eos] + full[:i], v)
                ref, mass, fp32_bound = ref + lp, mass + sum(terms), fp32_bound + (order + 1) * EPS * sum(terms)
            assert abs(got[q] - ref) <= 1e-12 * mass + fp32_bound, (q, got[q], ref)
            exact = math.fsum(float(v) for v in terms32)         # the same fp32 terms, summed without error
            assert abs(got[q] - exact) <= 1e-12 * sum(abs(float(v)) for v in terms32), (q, got[q], exact)
    bad = [list(s) for s in seqs[:5]]
    bad[3][2] = V                                                 # a label out of range: NaN for that sequence alone
    got = t.score_seqs(bad, torch.device(DEV))
    want = t.score_seqs(seqs[:5], torch.device(DEV))
    assert np.isnan(got[3]) and (np.delete(got, 3) == np.delete(want, 3)).all()
