"""Pins tests/refs64_dec.py (CPU only): the float64 prefix recursion against an enumeration of all V^T alignments and, in float32, against the
host scorer that follows upstream (model/beam_search.py CTCPrefixScore); the cell, output-layer and log-softmax references against
torch.nn.LSTMCell, F.linear and torch.log_softmax on doubles; for every row of the tables of tests/test_dec_kernels_gpu.py, that the fp32
CPU run of the reference stays within a quarter of the bar the HIP kernels are held to there; that the tables cover what they say they
cover, and that every kernel form they declare follows from the row's widths and offsets under a restatement of the launcher's rule (the
GPU test asserts the library's own answer, re2e_lm_plan).

tests/golden/recog_tiny.npz holds n-best label sequences and their combined scores only, no prefix scores, so there is nothing in it to
pin ``prefix_ref`` to; the recognitions themselves are held to it by tests/test_recog_batch_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refs64_dec as R


# ---------------------------------------------------------------------------------------------
# prefix scores
# ---------------------------------------------------------------------------------------------
def _neg_inf_is_dead(a):
    """The enumeration has log 0 = -inf where the recursion carries LOGZERO (plus what was added to it)."""
    c = R.classes(a)
    c[c == 2] = 1
    return c


@pytest.mark.parametrize('T,V,seed', [(6, 4, 0), (5, 3, 1), (3, 4, 2), (2, 3, 3), (1, 3, 4)])
def test_prefix_ref_against_enumeration(T, V, seed):
    """Chains of three positions from the empty hypothesis, extended by a repeated label, by a fresh one and by <eos> in turn, on until the
    hypothesis has as many labels as there are frames: prefix probability and both forward variables of every step against brute force
    (1e-12 of the live max; the dead masks equal)."""
    g = torch.Generator().manual_seed(seed)
    lpz = torch.log_softmax(2.0 * R.rnd(g, T, V).double(), 1).numpy()          # normalised in double: the frames' probabilities sum to 1
    eos, blank = V - 1, 0
    lab = [v for v in range(1, V - 1)] or [1]
    chains = [[lab[0], lab[0], lab[-1]], [lab[-1], lab[0], lab[0]], [lab[0], lab[-1], lab[-1]]]
    if T >= 4:
        chains.append([lab[i % len(lab)] for i in range(T + 1)])         # on to n = T: the last position scores a hypothesis of T labels
    for chain in chains:
        y, state = [eos], R.prefix_initial_state(lpz, blank)
        for pos, c in enumerate(chain):
            cs = [c, eos] + [v for v in range(V) if v not in (c, eos)]    # the label taken, <eos>, then every other label (blank included)
            psi, r = R.prefix_ref(lpz, y, cs, state, blank, eos)
            n = len(y) - 1
            start = min(max(n, 1), T)
            for j, cj in enumerate(cs):
                if cj == blank:
                    continue                                              # (blank as a candidate is scored mechanically: no labelling collapses to it)
                bp, br = R.prefix_brute(lpz, y[1:] + [cj], blank)
                if cj == eos:                                             # <eos>: the probability of exactly y, all T frames used
                    want = np.logaddexp(*R.prefix_brute(lpz, y[1:], blank)[1][T - 1])
                    assert abs(psi[j] - want) <= 1e-12 * max(1.0, abs(want)), (chain, pos, psi[j], want)
                    continue
                assert (_neg_inf_is_dead(psi[j]) == _neg_inf_is_dead(bp)).all(), (chain, pos, cj, psi[j], bp)
                if np.isfinite(bp):
                    assert abs(psi[j] - bp) <= 1e-12 * max(1.0, abs(bp)), (chain, pos, cj, psi[j], bp)
                got, ref = r[j][start - 1:], br[start - 1:]
                assert (_neg_inf_is_dead(got) == _neg_inf_is_dead(ref)).all(), (chain, pos, cj, got, ref)
                assert R.live_err(got, np.where(np.isfinite(ref), ref, R.LOGZERO)) <= 1e-12, (chain, pos, cj)
            y, state = y + [c], r[0]
            if len(y) - 1 > T:
                break


@pytest.mark.parametrize('name', R.PREFIX_IDS)
def test_prefix_table_rows_hold_their_margin_and_follow_the_host_scorer(name):
    """Per row and entry point: the fp32 run of the reference is within a quarter of the row's bar on every position (scores, local scores,
    the state rows that are read), its classes are float64's; and, for hypotheses of at most T labels, that fp32 run is within 1e-5 of the
    live max of model/beam_search.py's CTCPrefixScore on the same inputs."""
    from robust_e2e_gan_amd.model.beam_search import CTCPrefixScore
    case = R.PREFIX_CASES[R.PREFIX_IDS.index(name)]
    for entry in case['entries']:
        for pos, L in enumerate(R.prefix_chain(name, entry)):
            where = (name, entry, pos)
            mask = R.read_mask(L['f64']['r'].shape, L['starts'])
            for q in ('psi', 'local', 'r'):
                m = mask if q == 'r' else None
                c64, c32 = R.classes(L['f64'][q]), R.classes(L['f32'][q])
                assert (c64 == c32)[m if m is not None else ...].all(), where + (q,)
                e = R.live_err(L['f32'][q], L['f64'][q], m)
                assert e <= 0.25 * (case['bar_r'] if q == 'r' else case['bar']), 'input too hard for the bar: fp32 CPU reference of %s %s is %.3e from float64' % (where, q, e)
            nan_att = np.isnan(L['att']).any(1)
            for k in range(len(L['olen'])):
                u = int(L['utt'][k])
                T = L['T'][u]
                if L['olen'][k] > T or nan_att[k]:
                    continue
                host = CTCPrefixScore(L['lpz'][u, :T], R.BLANK, L['eos'])
                y = [L['eos']] + [1] * (int(L['olen'][k]) - 1) + ([int(L['last'][k])] if L['olen'][k] else [])
                sc, st = host(y, L['cands'][k], L['r_prev'][k, :T])
                first = max(int(L['olen'][k]), 1) - 1
                assert R.live_err(sc, L['f32']['psi'][k]) <= 1e-5, where + (k,)
                assert (R.classes(sc) == R.classes(L['f32']['psi'][k])).all(), where + (k,)
                assert R.live_err(st[:, first:], L['f32']['r'][k, :, first:T]) <= 1e-5, where + (k,)
                assert (R.classes(st[:, first:]) == R.classes(L['f32']['r'][k, :, first:T])).all(), where + (k,)
            if L['U'] > 1:                                                # state rows beyond an utterance's frames are dead
                for k in range(len(L['olen'])):
                    assert (L['f64']['r'][k, :, L['T'][int(L['utt'][k])]:] == R.LOGZERO).all()


def test_prefix_table_covers_what_it_claims():
    topk = [c for c in R.PREFIX_CASES if 'topk' in c['entries']]
    T = lambda c: max(c['T']) if isinstance(c['T'], list) else c['T']
    lds = lambda c: 4 * (c['V'] + 3 * T(c))
    assert any(2 * T(c) <= 256 and c['V'] <= 256 for c in topk) and any(128 < T(c) <= 256 for c in topk) and any(T(c) > 256 for c in topk)
    assert any(c['V'] > 256 and c['cb'] == 64 for c in topk) and any(c['cb'] == 1 for c in topk) and any(c['cb'] == c['V'] for c in topk)
    assert {1, 2} <= {T(c) for c in topk}
    big = [c for c in topk if lds(c) > 64 * 1024]
    assert big and all(lds(c) <= 150 * 1024 for c in R.PREFIX_CASES)
    ncs = {c['cands'][1] for c in R.PREFIX_CASES if 'cands' in c['entries']}
    assert {1, 255, 256, 257} <= ncs
    assert {'sorted', 'subset', 'dups'} == {c['cands'][0] for c in R.PREFIX_CASES if 'cands' in c['entries']}
    for c in R.PREFIX_CASES:
        if 'batch' in c['entries']:
            assert len(c['T']) == 3 and c['T'][1] == 1 and c['T'][2] % 2 == 1 and c['T'][0] == max(c['T'])
    # what a chain of the main rows carries: the repeated label, <eos> and blank as candidates, out_len 0, 1 and >= 2 in ONE launch, rows of
    # different utterances interleaved, duplicates, a hypothesis of T and of T + 3 labels, degenerate attention rows
    for name, entry in (('one-trip', 'topk'), ('one-trip', 'cands'), ('2T-over-256', 'cands'), ('T-over-256', 'topk'), ('batch', 'batch')):
        Ls = R.prefix_chain(name, entry)
        assert len(Ls) == R.POSITIONS
        assert all(any(L['flags'][k] for L in Ls) for k in ('repeat', 'eos', 'blank')), (name, entry)
        assert any(L['flags']['olens'] == [0, 1, 2] for L in Ls), (name, entry)
    Ls = R.prefix_chain('batch', 'batch')
    assert any(len(set(L['utt'].tolist())) == 3 and (np.diff(L['utt']) != 0).sum() >= 3 for L in Ls)
    assert any(len(set(row.tolist())) < len(row) for L in R.prefix_chain('T-over-256', 'cands') for row in L['cands'])
    L = R.prefix_chain('deep', 'topk')[-1]
    assert 3 in L['olen'].tolist() and 6 in L['olen'].tolist() and (L['starts'] <= 3).all()
    L = R.prefix_chain('weak-rows', 'topk')[-1]
    assert np.isneginf(L['att'][0]).sum() > L['V'] - 5 and np.isnan(L['att'][1]).sum() == 1
    assert L['cands'][0].tolist() == [7, 3, 0, 1, 2] and 4 not in L['cands'][1].tolist()
    assert np.isneginf(L['f64']['local'][0, 2:]).all()


# ---------------------------------------------------------------------------------------------
# the few-row LM kernels
# ---------------------------------------------------------------------------------------------
def test_lm_references_against_torch_modules_on_doubles():
    g = torch.Generator().manual_seed(3)
    n, I, H, V = 5, 7, 9, 11
    cell = torch.nn.LSTMCell(I, H).double()
    for p in cell.parameters():
        p.data = R.rnd(g, *p.shape, scale=0.4).double()
    x, h0, c0 = R.rnd(g, n, I).double(), torch.tanh(R.rnd(g, n, H)).double(), R.rnd(g, n, H).double()
    with torch.no_grad():
        for hp, cp in ((h0, c0), (None, None), (h0, None), (None, c0)):
            zeros = torch.zeros(n, H, dtype=torch.float64)
            want = cell(x, (hp if hp is not None else zeros, cp if cp is not None else zeros))
            got = R.cell_ref(x, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, hp, cp)
            assert R.rel_err(got[0], want[0]) <= 1e-12 and R.rel_err(got[1], want[1]) <= 1e-12
        w, b = R.rnd(g, V, H).double(), R.rnd(g, V).double()
        assert R.rel_err(R.out_ref(h0, w, b), F.linear(h0, w, b)) <= 1e-12
    for V_, n_ in ((1, 1), (1025, 3), (8193, 3)):
        d = R.lsm_inputs(V_, n_)
        assert R.rel_err(R.lsm_ref(d['logits']), torch.log_softmax(d['logits'].double(), 1)) <= 1e-12
    # the fp32 restatements: two roundings, not a fused multiply-add; NaN exactly at the labels out of range
    a, l = torch.tensor([[1.0000001, -3.0]]), torch.tensor([[-2.3456789, -0.1234567]])
    two = R.comb_fp32(a, 0.3, l)
    assert torch.equal(two, (a.double() + (np.float32(0.3) * l).double()).float())
    lm, cand = R.rnd(g, 2, 6), torch.tensor([[0, 6, 5], [-1, 2, 2]], dtype=torch.int32)
    out = R.add_cands_fp32(torch.zeros(2, 3), lm, cand, 0.5)
    assert torch.isnan(out).tolist() == [[False, True, False], [True, False, False]] and out[1, 1] == out[1, 2] == 0.5 * lm[1, 2]


def _vec_width(off_bytes, ld):
    """csrc/rnnlm.hip vec_width restated: the widest load (floats) every row of an operand starts aligned for (None: a NULL operand)."""
    if off_bytes is None:
        return 4
    if ld % 4 == 0 and off_bytes % 16 == 0:
        return 4
    if ld % 2 == 0 and off_bytes % 8 == 0:
        return 2
    return 1


def test_lm_tables_declare_the_forms_their_widths_imply():
    seen = set()
    for row in R.LM_CELL_CASES:
        off = lambda k: row['off'].get(k, 0)
        vi = min(_vec_width(off('w_ih'), row['I']), _vec_width(off('x'), row['ldx']))
        vh = min(_vec_width(off('w_hh'), row['H']), _vec_width(off('h_prev') if row['state'] in ('both', 'h') else None, row['H']))
        pair = (4, 4) if (vi, vh) == (4, 4) else (4, 2) if (vi, vh) == (4, 2) else (2, 2) if vi >= 2 and vh >= 2 else (1, 1)
        assert row['form'] == (R.rows_per_trip(row['n']),) + pair, row['name']
        assert row['ldx'] >= row['I'] and 1 <= row['n'] <= 64
        seen.add(row['form'])
    assert seen == {(r, a, b) for r in (4, 8, 16) for a, b in ((4, 4), (4, 2), (2, 2), (1, 1))}
    assert {row['n'] for row in R.LM_CELL_CASES} >= set(R.LM_NS)
    assert {'both', 'none', 'h', 'c'} == {row['state'] for row in R.LM_CELL_CASES} and {'ids', 'dense'} == {row['x'] for row in R.LM_CELL_CASES}
    assert {(256, 650), (650, 650)} <= {(row['I'], row['H']) for row in R.LM_CELL_CASES}
    assert {127, 128, 129, 254, 256, 258, 508, 512, 516} <= {row['I'] for row in R.LM_CELL_CASES if row['I'] == row['H']}
    seen = set()
    for row in R.LM_OUT_CASES:
        vec = min(_vec_width(row['off'].get('w', 0), row['H']), _vec_width(row['off'].get('h', 0), row['H']))
        assert row['form'] == (R.rows_per_trip(row['n']), vec), row['name']
        seen.add(row['form'])
    assert seen == {(r, v) for r in (4, 8, 16) for v in (4, 2, 1)}
    assert {row['V'] for row in R.LM_OUT_CASES} == {1, 3, 4, 5, 4233} and {row['H'] for row in R.LM_OUT_CASES} == {12, 10, 7, 650, 652}
    assert {row['n'] for row in R.LM_OUT_CASES} >= set(R.LM_NS)
    assert len({r['name'] for r in R.LM_CELL_CASES}) == len(R.LM_CELL_CASES) and len({r['name'] for r in R.LM_OUT_CASES}) == len(R.LM_OUT_CASES)


def test_lm_table_rows_hold_their_margin():
    for row in R.LM_CELL_CASES:
        d = R.cell_inputs(row)
        (h64, c64), (h32, c32) = R.cell_case_ref(d), R.cell_case_ref(d, torch.float32)
        R.margin_ok(row['name'] + ' h', h32, h64, R.BAR_OUT)
        R.margin_ok(row['name'] + ' c', c32, c64, R.BAR_OUT)
    for row in R.LM_OUT_CASES:
        d = R.out_inputs(row)
        R.margin_ok(row['name'], R.out_ref(d['h'], d['w'], d['b'], torch.float32), R.out_ref(d['h'], d['w'], d['b']), R.BAR_LOGITS)
    for V, n in R.LSM_CASES:
        d = R.lsm_inputs(V, n)
        R.margin_ok('lsm V%d n%d' % (V, n), R.lsm_ref(d['logits'], torch.float32), R.lsm_ref(d['logits']), R.BAR_GRAD)
    assert {d['lm_weight'] for d in (R.lsm_inputs(V, n) for V, n in R.LSM_CASES)} == {0.0, 0.3}
