"""csrc/wordlm.hip (re2e_wlm_transition, re2e_wlm_softmax_cumsum, re2e_wlm_lookahead, re2e_wlm_multilevel_fix) against the float64
restatement tests/refs64_wordlm.py, kernel by kernel.  Every output buffer starts as NaN."""
import random

import numpy as np
import pytest
import torch

import refs64_wordlm as R
from test_modules_gpu import DEV

pytestmark = pytest.mark.gpu

CUMSUM_BOUND = 16 * 2.0 ** -24          # 9.5e-7: a few ulp of relative error per fp32 probability (expf, the sum, the divide) on prefix sums <= 1,
#                                         plus the one rounding of the fp64 running sum at the store (2^-25)


def nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -12345, dtype=dtype, device=DEV)
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def dev_i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


def logits_rows(n, Vw, seed):
    """Rows within +-30 at scales from 30 down to 0.03 (sharp to nearly flat: there the prefix sums grow over the whole row); row 1 is
    dominated by a single entry."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(n, Vw, generator=g) * 2 - 1) * 30
    for r in range(n):
        z[r] *= (1.0, 0.1, 0.01, 0.001)[r % 4]
    if n > 1:
        z[1] = -torch.rand(Vw, generator=g) * 30
        z[1, Vw // 2] = 30.0
    return z


def check_cumsum(got, z, what):
    ref = torch.cumsum(torch.softmax(z.double(), dim=1), dim=1)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), '%s: %d elements not finite (not written?)' % (what, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs().max().item()
    last = (got[:, -1] - 1.0).abs().max().item()
    print('%s: max |cumsum - fp64| %.3e, max |last - 1| %.3e (bound %.3e, a quarter of it %.3e)' % (what, err, last, CUMSUM_BOUND, CUMSUM_BOUND / 4))
    assert err <= CUMSUM_BOUND, (what, err)
    assert last <= CUMSUM_BOUND, (what, last)
    assert bool((got[:, 1:] >= got[:, :-1]).all()), '%s: a row decreases' % what


@pytest.mark.parametrize('Vw', [3, 63, 64, 65, 1000, 4099])
def test_softmax_cumsum_vs_float64(Vw):
    from robust_e2e_gan_amd.lib import call
    n = 64
    z = logits_rows(n, Vw, Vw)
    zd, out = z.to(DEV), nan(n, Vw)
    call('re2e_wlm_softmax_cumsum', zd.data_ptr(), n, Vw, None, n, out.data_ptr())
    check_cumsum(out, z, 'Vw=%d n=%d' % (Vw, n))


def test_softmax_cumsum_production_width_scattered_rows():
    """Vw = 65000 (16 passes of the workgroup, the last one partial): m = 3 rows of logits go to rows 4, 0, 2 of a 5-row buffer; rows 1 and
    3 keep their NaN fill.  A destination outside the buffer is skipped."""
    from robust_e2e_gan_amd.lib import call
    Vw, n, m = 65000, 5, 3
    z = logits_rows(4, Vw, 7)[[0, 1, 3]]                # sharp, dominated, nearly flat
    zd, out = z.to(DEV), nan(n, Vw)
    dst = [4, 0, 2]
    dst_d, off_d = dev_i32(dst), dev_i32([5, -1, 1 << 20])
    call('re2e_wlm_softmax_cumsum', zd.data_ptr(), m, Vw, dst_d.data_ptr(), n, out.data_ptr())
    check_cumsum(out[dst], z, 'Vw=%d m=%d of n=%d' % (Vw, m, n))
    assert bool(torch.isnan(out[[1, 3]]).all()), 'rows that are not a destination were written'
    before = out.clone()
    call('re2e_wlm_softmax_cumsum', zd.data_ptr(), m, Vw, off_d.data_ptr(), n, out.data_ptr())
    assert torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(before, nan=-1.0)), 'a destination outside [0, n) was written'


# ---- trees for the lookups: every label is a single symbol, so that any label can be a child of the root ---------------------------------
def symbols(Vc):
    return [chr(0x4e00 + i) for i in range(Vc)]


def make_dicts(Vc, full_root, seed):
    """space = 1, eos = Vc - 1.  full_root: every label is a one-symbol word (the root has all Vc children), plus longer words over the first
    labels; otherwise a sparse dictionary over labels 2 .. 9 with nested prefixes and one-symbol words for two labels only."""
    rng = random.Random(seed)
    sym = symbols(Vc)
    subword = {s: i for i, s in enumerate(sym)}
    words = ['<blank>', '<unk>', '<eos>']
    pool = sym[2:min(Vc - 1, 10)]
    if full_root:
        words += sym
    else:
        words += [pool[0], pool[1]]
    seen = set(words)
    while len(words) < (len(sym) + 60 if full_root else 40):
        w = ''.join(rng.choice(pool) for _ in range(rng.randint(2, 4)))
        if w not in seen:
            seen.add(w)
            words.append(w)
            if len(w) > 2 and w[:-1] not in seen and rng.random() < 0.5:      # a word end with children
                seen.add(w[:-1])
                words.append(w[:-1])
    order = list(range(3, len(words)))
    rng.shuffle(order)                                   # ids are not in tree order: the word-set ranges overlap other words'
    word_dict = {'<blank>': 0, '<unk>': 1, '<eos>': 2}
    for new, old in enumerate(order):
        word_dict[words[old]] = 3 + new
    return word_dict, subword


def pick_nodes(nested):
    """Flat ids: the root, a word end with children, a word-end leaf, an inner non-end node, the node with most children."""
    out = [0]
    for want in (lambda nd: nd.wid >= 0 and nd.succ, lambda nd: nd.wid >= 0 and not nd.succ, lambda nd: nd.wid < 0 and nd.succ and nd.lo is not None):
        found = [k for k, nd in enumerate(nested) if want(nd)]
        assert found, 'the dictionary lacks a node kind'
        out.extend(found[:2])
    return out


def cumsum_rows(n, Vw, seed):
    """fp32 cumulative word probabilities as a float32 cumsum gives them; rows 2 .. 5 have words of probability exactly 0 (flat stretches)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, Vw, generator=g) * 2
    for r in range(2, min(n, 6)):
        z[r, torch.rand(Vw, generator=g) < 0.5] = -200.0
    return torch.cumsum(torch.softmax(z, dim=1), dim=1).contiguous()


def same(got, ref, what, rel=1e-6):
    """NaN where the reference is NaN, the same infinities, |got - ref| <= rel * max(1, |ref|) elsewhere."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), '%s: NaN at other places than the reference' % what
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and not np.isinf(got[~inf & ~np.isnan(ref)]).any(), '%s: infinities differ' % what
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    worst = float(err.max()) if err.size else 0.0
    print('%s: max |err| / max(1, |ref|) %.3e over %d finite, %d -inf, %d NaN entries' % (what, worst, fin.sum(), inf.sum(), np.isnan(ref).sum()))
    assert worst <= rel, (what, worst)


def lookahead_case(Vc, full_root, open_vocab):
    """The tree, the rows and the float64 answer of one look-ahead case (no device)."""
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    word_dict, subword = make_dicts(Vc, full_root, Vc)
    space, eos, unk, weos, oov = 1, Vc - 1, 1, 2, float(np.float32(0.0001))
    flat = LexicalTree(word_dict, subword, unk)
    nested = R.tree_nodes(R.make_tree(word_dict, subword, unk))
    if full_root:
        assert len(nested[0].succ) == Vc
    nodes, flags = [], []
    for k in pick_nodes(nested):
        nodes += [k, k]
        flags += [1, 0]
    nodes += [-1, -1, 0, flat.n_nodes, -2]
    flags += [0, 1, -1, 0, 1]
    n, Vw = len(nodes), len(word_dict)
    c = cumsum_rows(n, Vw, Vc + full_root)
    ref = np.empty((n, Vc))
    for r in range(n):
        if flags[r] < 0 or not -1 <= nodes[r] < flat.n_nodes:
            ref[r] = np.nan
        else:
            ref[r] = R.lookahead_log_y(c[r].numpy(), nested[nodes[r]] if nodes[r] >= 0 else None, flags[r] == 1, Vc, space, eos, unk, weos, oov, open_vocab)
    return flat, nodes, flags, c, ref, (space, eos, unk, weos, oov)


@pytest.mark.parametrize('Vc,full_root', [(12, False), (12, True), (52, False), (52, True), (4233, True)])
@pytest.mark.parametrize('open_vocab', [True, False])
def test_lookahead_vs_float64(Vc, full_root, open_vocab):
    """Rows: the root, word ends with children, word-end leaves (no children), inner non-end nodes, each right after a space and not; node
    -1; and rows that must come out NaN (flag -1, a node >= N).  Both sides read the same float32 cumsum tensor.  Bound: three fp32
    roundings plus logf -> 1e-6 * max(1, |log_y|); -inf exactly where the reference's y is 0."""
    from robust_e2e_gan_amd.lib import call
    flat, nodes, flags, c, ref, (space, eos, unk, weos, oov) = lookahead_case(Vc, full_root, open_vocab)
    n, Vw = c.shape
    t = flat.dev(DEV)
    cd, out, nodes_d, flags_d = c.to(DEV), nan(n, Vc), dev_i32(nodes), dev_i32(flags)
    call('re2e_wlm_lookahead', cd.data_ptr(), n, Vw, nodes_d.data_ptr(), flags_d.data_ptr(), t['wid'].data_ptr(), t['lo'].data_ptr(),
         t['hi'].data_ptr(), t['child_off'].data_ptr(), t['child_label'].data_ptr(), t['child_node'].data_ptr(), flat.n_nodes, flat.n_children, Vc, space,
         eos, unk, weos, oov, int(open_vocab), out.data_ptr())
    assert np.isinf(ref).any(), 'no -inf in the reference: the zero-probability case is not exercised'
    same(out.cpu().numpy(), ref, 'lookahead Vc=%d full_root=%s open_vocab=%s' % (Vc, full_root, open_vocab))


@pytest.mark.parametrize('Vc,full_root', [(12, False), (52, True), (4233, True)])
def test_transition_exact(Vc, full_root):
    """Every (node, label) pair of interest: the first, a middle and the last child of nodes with several children, labels the node lacks,
    <space> at word ends / non-ends / from node -1, any label from node -1, labels outside [0, Vc) and nodes outside [-1, N)."""
    from robust_e2e_gan_amd.lib import call
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    word_dict, subword = make_dicts(Vc, full_root, Vc)
    space, unk = 1, 1
    flat = LexicalTree(word_dict, subword, unk)
    nested = R.tree_nodes(R.make_tree(word_dict, subword, unk))
    number = {id(nd): k for k, nd in enumerate(nested)}
    N = flat.n_nodes
    cases = []
    for k, nd in enumerate(nested):
        labels = sorted(nd.succ)
        if len(labels) >= 3 and len(cases) < 40:
            cases += [(k, labels[0]), (k, labels[len(labels) // 2]), (k, labels[-1])]
            cases += [(k, lab) for lab in (0, labels[0] + 1, Vc - 1) if lab not in nd.succ and lab != space][:2]
    cases += [(k, space) for k in pick_nodes(nested)] + [(-1, space), (-1, 2), (-1, Vc - 1), (0, 0)]
    bad = [(0, -1), (0, Vc), (0, Vc + 5), (-2, 2), (N, 2), (N + 7, space), (-1, -1)]
    cases += bad
    cases = cases[:64]
    n = len(cases)
    assert n >= 20 and cases[-1] == bad[-1]
    out = nan(3, n, dtype=torch.int32)
    t = flat.dev(DEV)
    nodes_d, labels_d = dev_i32([c[0] for c in cases]), dev_i32([c[1] for c in cases])
    call('re2e_wlm_transition', nodes_d.data_ptr(), labels_d.data_ptr(), n, Vc, space, unk, t['wid'].data_ptr(),
         t['child_off'].data_ptr(), t['child_label'].data_ptr(), t['child_node'].data_ptr(), N, flat.n_children, out[0].data_ptr(), out[1].data_ptr(),
         out[2].data_ptr())
    want = []
    for k, lab in cases:
        if not (0 <= lab < Vc and -1 <= k < N):
            want.append((-1, unk, -1))
        elif lab == space:
            want.append((0, nested[k].wid if k >= 0 and nested[k].wid >= 0 else unk, 1))
        else:
            nd = nested[k].succ.get(lab) if k >= 0 else None
            want.append((number[id(nd)] if nd is not None else -1, unk, 0))
    got = out.cpu().numpy().T.tolist()
    assert [tuple(g) for g in got] == want
    assert any(w[0] > 0 for w in want) and any(w == (-1, unk, 0) for w in want) and any(w[1] != unk for w in want)
    # no previous node: every row at the root
    call('re2e_wlm_transition', None, labels_d.data_ptr(), n, Vc, space, unk, t['wid'].data_ptr(), t['child_off'].data_ptr(),
         t['child_label'].data_ptr(), t['child_node'].data_ptr(), N, flat.n_children, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    first = out[0].cpu().tolist()
    for (k, lab), g in zip(cases, first):
        assert g == (-1 if not 0 <= lab < Vc else 0 if lab == space else flat.step(0, lab))


@pytest.mark.parametrize('Vc', [12, 52, 4233])
@pytest.mark.parametrize('open_vocab', [True, False])
def test_multilevel_fix_vs_float64(Vc, open_vocab):
    """Rows at a word end, at an inner node, at node -1, right after a space, with bad flags / nodes / labels (NaN), and the initial position
    (no previous accumulator).  Bound as for the look-ahead rows: one fp32 product or two fp32 sums -> 1e-6 * max(1, |value|); logzero exact."""
    from robust_e2e_gan_amd.lib import call
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    word_dict, subword = make_dicts(Vc, True, Vc)
    space, eos, unk, weos, weight, log_oov = 1, Vc - 1, 1, 2, 0.8, float(np.log(0.5))
    flat = LexicalTree(word_dict, subword, unk)
    nested = R.tree_nodes(R.make_tree(word_dict, subword, unk))
    N, Vw = flat.n_nodes, len(word_dict)
    picked = pick_nodes(nested)
    nodes = picked + [-1, 0, -1, 0, N, 2, 3]
    flags = [0] * len(picked) + [0, 1, 1, -1, 0, 0, 0]
    n = len(nodes)
    labels = [2 + r % (Vc - 3) for r in range(n)]
    labels[-2], labels[-1] = -1, Vc                     # bad labels
    flags[0] = 1                                        # (the root is only ever reached by a space)
    g = torch.Generator().manual_seed(Vc)
    lsm = torch.log_softmax(torch.randn(n, Vc, generator=g) * 3, dim=1)
    wlp = torch.log_softmax(torch.randn(n, Vw, generator=g) * 3, dim=1)
    y_prev = torch.log_softmax(torch.randn(n, Vc, generator=g), dim=1) * weight
    clm_prev = -torch.rand(n, generator=g) * 2          # |clm| stays below 10, so that its fp32 rounding (2^-24 |clm|) fits the bound at |value| ~ 1
    t = flat.dev(DEV)

    def run(initial):
        out, clm = nan(n, Vc), nan(n)
        cp, yp = (None, None) if initial else (clm_prev.to(DEV), y_prev.to(DEV))
        lsm_d, wlp_d, lab_d, nodes_d, flags_d = lsm.to(DEV), wlp.to(DEV), dev_i32(labels), dev_i32(nodes), dev_i32(flags)
        call('re2e_wlm_multilevel_fix', lsm_d.data_ptr(), wlp_d.data_ptr(), n, Vw, nodes_d.data_ptr(), flags_d.data_ptr(), t['wid'].data_ptr(), N,
             cp.data_ptr() if cp is not None else None, yp.data_ptr() if yp is not None else None, None if initial else lab_d.data_ptr(), Vc, space, eos,
             unk, weos, float(np.float32(weight)), float(np.float32(log_oov)), int(open_vocab), out.data_ptr(), clm.data_ptr())
        return out.cpu().numpy(), clm.cpu().numpy()

    got_y, got_clm = run(False)
    ref_y, ref_clm = np.empty((n, Vc)), np.empty(n)
    for r in range(n):
        if flags[r] < 0 or not -1 <= nodes[r] < N or not 0 <= labels[r] < Vc:
            ref_y[r], ref_clm[r] = np.nan, np.nan
        elif flags[r] == 0 and nodes[r] < 0 and not open_vocab:
            ref_y[r], ref_clm[r] = R.LOGZERO, 0.0
        else:
            ref_clm[r] = 0.0 if flags[r] == 1 else float(clm_prev[r]) + float(y_prev[r, labels[r]])
            ref_y[r] = R.multilevel_fix(lsm[r].numpy(), wlp[r].double().numpy(), nested[nodes[r]] if nodes[r] >= 0 else None, flags[r] == 1, ref_clm[r],
                                        space, eos, unk, weos, float(np.float32(weight)), float(np.float32(log_oov)))
    same(got_y, ref_y, 'multilevel_fix Vc=%d open_vocab=%s' % (Vc, open_vocab))
    same(got_clm, ref_clm, 'clm_logprob Vc=%d open_vocab=%s' % (Vc, open_vocab))
    big = np.abs(ref_y) >= 1e9
    assert big.any() and np.array_equal(got_y[big], ref_y[big])
    # the initial position: every row at the root right after a "space", labels not read
    nodes, flags = [0] * n, [1] * n
    got_y, got_clm = run(True)
    ref_y = np.stack([R.multilevel_fix(lsm[r].numpy(), wlp[r].double().numpy(), nested[0], True, 0.0, space, eos, unk, weos, float(np.float32(weight)),
                                       float(np.float32(log_oov))) for r in range(n)])
    same(got_y, ref_y, 'multilevel_fix initial Vc=%d' % Vc)
    assert (got_clm == 0).all()
