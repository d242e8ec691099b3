"""CPU-only: the ARPA reader, the token mapping and the flat tables of robust_e2e_gan_amd/model/ngram.py against the dictionary form of Katz
back-off (tests/refs_ngram.py, float64), the host arbiter ``step_host`` that the GPU tests compare the kernels with, persistence, and the
places that accept or refuse an n-gram LM."""
import argparse
import os

import numpy as np
import pytest
import torch

import refs_ngram as R
from robust_e2e_gan_amd.model.ngram import ArpaError, LOGZERO, NgramLM, NgramTables, load_tables, read_arpa

EPS = 2.0 ** -24

GOOD = ['', '\\data\\', 'ngram 1=4', 'ngram 2=3', 'ngram 3=1', '', '\\1-grams:', '-1.0\t<s>\t-0.5', '-0.7\t</s>', '-0.4\ta\t-0.3', '-0.6\tb\t-0.2', '',
        '\\2-grams:', '-0.2\t<s> a\t-0.1', '-0.3\ta b', '-0.5\tb </s>', '', '\\3-grams:', '-0.1\t<s> a b', '', '\\end\\']


def _write(tmp_path, lines, name='lm.arpa'):
    p = os.path.join(str(tmp_path), name)
    with open(p, 'w', encoding='utf-8') as f:
        f.write('\n'.join(lines) + '\n')
    return p


def _edit(lines, at, new):
    """``lines`` with 1-based line ``at`` replaced by ``new`` (a list: any number of lines)."""
    return lines[:at - 1] + new + lines[at:]


def test_good_file_reads(tmp_path):
    grams = read_arpa(_write(tmp_path, GOOD))
    assert [len(g) for g in grams] == [4, 3, 1]
    assert grams[0][('<s>',)] == (-1.0, -0.5) and grams[0][('</s>',)] == (-0.7, 0.0) and grams[2][('<s>', 'a', 'b')] == (-0.1, 0.0)


@pytest.mark.parametrize('name,lines,lineno,needle', [
    ('count', _edit(GOOD, 4, ['ngram 2=4']), 13, '2-grams'),                                   # reported at the section's header
    ('prefix', _edit(GOOD, 16, ['-0.5\tc </s>']), 16, 'c </s>'),
    ('duplicate', _edit(_edit(GOOD, 4, ['ngram 2=4']), 16, ['-0.5\tb </s>', '-0.5\ta b']), 17, 'a b'),
    ('backoff_on_highest', _edit(GOOD, 19, ['-0.1\t<s> a b\t-0.2']), 19, 'highest'),
    ('order_in_counts', _edit(GOOD, 5, ['ngram 3=1', 'ngram 9=1']), 6, 'order 9'),
    ('order_in_section', _edit(GOOD, 18, ['\\9-grams:']), 18, 'order 9'),
    ('number', _edit(GOOD, 10, ['-0.4x\ta\t-0.3']), 10, '-0.4x'),
    ('backoff_number', _edit(GOOD, 10, ['-0.4\ta\tabc']), 10, 'abc'),
    ('no_end', GOOD[:-1], 20, 'end'),
])
def test_arpa_errors_carry_the_line(tmp_path, name, lines, lineno, needle):
    with pytest.raises(ArpaError) as e:
        read_arpa(_write(tmp_path, lines))
    assert isinstance(e.value, ValueError)
    assert e.value.lineno == lineno and ('line %d:' % lineno) in str(e.value) and needle in str(e.value), str(e.value)


def test_symbols_mode_sentence_marks_share_eos(tmp_path):
    """char_list = <blank>, a, b, <eos>.  <s> and </s> are both label 3: the unigram of eos has </s>'s log-probability and <s>'s back-off; '<s> a'
    is the bigram (eos, a).  <blank> has no unigram and the file has no <unk>: the floor, and the state stays at the root."""
    chars = ['<blank>', 'a', 'b', '<eos>']
    t = NgramTables.from_arpa(_write(tmp_path, GOOD), chars, 'symbols')
    assert (t.order, t.n_vocab, t.eos, t.dropped, t.has_unk) == (3, 4, 3, 0, False)
    ln = lambda v: np.float32(v * R.LN10)
    assert t.uni_logp[3] == ln(-0.7) and t.uni_logp[1] == ln(-0.4) and t.uni_logp[0] == np.float32(LOGZERO) and t.uni_next[0] == 0
    eos_node = int(t.uni_next[3])
    assert eos_node > 0 and t.bo[eos_node] == ln(-0.5)
    state, lp = t.step_host(None, [3])                           # the search's first position: every hypothesis holds [eos]
    assert state[0] == eos_node
    assert lp[0, 1] == ln(-0.2)                                   # p(a | <s>)
    assert lp[0, 2] == np.float32(ln(-0.5) + ln(-0.6))            # b backs off: bo(<s>) + p(b)
    assert lp[0, 0] == np.float32(ln(-0.5) + np.float32(LOGZERO))
    state, lp = t.step_host(state, [1])                           # context (eos, a)
    assert lp[0, 2] == ln(-0.1)                                   # the trigram <s> a b
    assert lp[0, 3] == np.float32(np.float32(ln(-0.1) + ln(-0.3)) + ln(-0.7))      # bo(<s> a) + bo(a) + p(</s>)
    state, lp = t.step_host(state, [0])                           # a label the model cannot name: back at the root
    assert state[0] == 0 and lp[0, 1] == ln(-0.4)


def test_unk_stands_for_labels_without_a_unigram_and_foreign_tokens_are_dropped(tmp_path):
    lines = ['\\data\\', 'ngram 1=6', 'ngram 2=4', '', '\\1-grams:', '-1.0\t<s>\t-0.5', '-0.7\t</s>', '-0.4\ta\t-0.3', '-0.9\t<unk>\t-0.25',
             '-1.1\tzz\t-0.1', '-1.2\tyy', '', '\\2-grams:', '-0.2\t<unk> a', '-0.3\ta <unk>', '-0.6\ta zz', '-0.15\tzz a', '', '\\end\\']
    chars = ['<blank>', 'a', 'b', 'c', '<eos>']
    t = NgramTables.from_arpa(_write(tmp_path, lines), chars, 'symbols')
    assert t.dropped == 2 and t.has_unk and t.order == 2
    ln = lambda v: np.float32(v * R.LN10)
    for v in (0, 2, 3):                                           # <blank>, b, c have no unigram: they are <unk>, in every position
        assert t.uni_logp[v] == ln(-0.9)
        state, lp = t.step_host(None, [v])
        assert state[0] == t.uni_next[2] > 0 and lp[0, 1] == ln(-0.2), v            # history: p(a | <unk>)
        assert lp[0, 4] == np.float32(ln(-0.25) + ln(-0.7))
    state, lp = t.step_host(None, [1])
    assert lp[0, 0] == lp[0, 2] == lp[0, 3] == ln(-0.3)           # predicted: p(<unk> | a)
    assert lp[0, 1] == np.float32(ln(-0.3) + ln(-0.4))            # 'a zz' went with zz


def test_ids_mode_the_eos_id_plays_both_roles(tmp_path):
    """Tokens are decimal label ids (what the reference feeds kenlm); <s> and </s> of such a file are no labels: dropped."""
    lines = ['\\data\\', 'ngram 1=5', 'ngram 2=2', '', '\\1-grams:', '-99\t<s>\t-0.5', '-0.7\t</s>', '-0.4\t1\t-0.3', '-0.8\t2\t-0.45', '-0.6\t7', '',
             '\\2-grams:', '-0.2\t2 1', '-0.35\t1 2', '', '\\end\\']
    t = NgramTables.from_arpa(_write(tmp_path, lines), ['<blank>', 'a', '<eos>'], 'ids')
    assert t.dropped == 3 and not t.has_unk and t.eos == 2                       # <s>, </s> and 7
    ln = lambda v: np.float32(v * R.LN10)
    state, lp = t.step_host(None, [2])
    assert lp[0, 1] == ln(-0.2) and lp[0, 2] == np.float32(ln(-0.45) + ln(-0.8))
    with pytest.raises(ValueError):
        NgramTables.from_arpa(_write(tmp_path, lines), ['<blank>', 'a', '<eos>'], 'words')


def _node_ids(grams):
    """The numbering of the layout, from the model alone: the n-grams of 1 .. order-1 labels by (length, labels), from 1; the root is 0."""
    order = len(grams)
    ctx = sorted((g for k in range(order - 1) for g in grams[k]), key=lambda g: (len(g), g))
    ids = {g: i + 1 for i, g in enumerate(ctx)}
    ids[()] = 0
    return ids


def _check_model(tmp_path, V, densities, seed, chains, no_unigram=0.0):
    """``chains`` random label chains of order + 3 positions through step_host, every row of every position against the dictionary scorer;
    returns how often each back-off depth was hit and how many floor scores were seen."""
    order = len(densities)
    grams = R.random_model(V, densities, seed, no_unigram)
    path = R.write_arpa(os.path.join(str(tmp_path), 'm%d_%d.arpa' % (V, order)), grams)
    t = NgramTables.from_arpa(path, [str(v) for v in range(V)], 'ids')
    assert t.order == order and t.dropped == 0 and t.n_nodes == 1 + sum(len(grams[k]) for k in range(order - 1))
    ids = _node_ids(grams)
    known = lambda v: (v,) in grams[0]
    rng = np.random.default_rng(seed)
    xs = rng.integers(0, V, size=(order + 3, chains))
    state, depths, floors, worst = None, np.zeros(order, np.int64), 0, 0.0
    for pos in range(order + 3):
        state, lp = t.step_host(state, xs[pos])
        assert lp.dtype == np.float32 and state.dtype == np.int32
        for r in range(chains):
            hist = xs[:pos + 1, r].tolist()
            cut = max([i + 1 for i, v in enumerate(hist) if not known(v)] or [0])
            assert state[r] == ids[R.longest_suffix(grams, hist[cut:])], (pos, r, hist)
            for v in range(V):
                ref, terms = R.score(grams, hist, v)
                bound = (order + 1) * EPS * sum(terms)
                err = abs(float(lp[r, v]) - ref)
                assert err <= bound, (pos, r, v, float(lp[r, v]), ref, bound)
                worst = max(worst, err / bound if bound else 0.0)
                if known(v):
                    depths[R.depth(grams, hist[cut:], v)] += 1
                else:
                    floors += 1
    print('V=%d order=%d: nodes %d, successors %d, depths %s, floors %d, worst error / bound %.3f'
          % (V, order, t.n_nodes, t.n_succ, depths.tolist(), floors, worst))
    return depths, floors


@pytest.mark.parametrize('V,densities,chains', [(9, [0, .5, .4, .4, .4], 150), (12, [0, .4, .3], 60), (7, [0, .5], 20), (5, [0], 8)])
def test_step_host_is_katz_backoff(tmp_path, V, densities, chains):
    """Orders 5, 3, 2 and 1; every back-off depth 0 .. order-1 is hit (asserted: with these densities thousands of times each)."""
    depths, _ = _check_model(tmp_path, V, densities, 100 + V, chains)
    assert (depths > 0).all(), depths


def test_labels_without_a_unigram_floor_and_reset(tmp_path):
    """V = 40, order 4, a tenth of the labels without a unigram and no <unk>: LOGZERO, and the history is cut behind such a label."""
    depths, floors = _check_model(tmp_path, 40, [0, .15, .2, .3], 7, 12, no_unigram=0.1)
    assert floors > 0 and depths[0] > 0, (floors, depths)


def test_save_load_is_bit_equal_and_cache(tmp_path):
    grams = R.random_model(12, [0, .4, .3], 3)
    path = R.write_arpa(os.path.join(str(tmp_path), 'c.arpa'), grams)
    chars = [str(v) for v in range(12)]
    t = NgramTables.from_arpa(path, chars, 'ids')
    npz = os.path.join(str(tmp_path), 'saved.npz')
    t.save(npz)
    u = NgramTables.load(npz)
    assert (u.order, u.n_vocab, u.eos, u.dropped, u.has_unk, u.tokens) == (t.order, t.n_vocab, t.eos, t.dropped, t.has_unk, 'ids')
    for name in NgramTables.ARRAYS:
        a, b = getattr(t, name), getattr(u, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert not os.path.exists(path + '.npz')
    first = load_tables(path, chars, 'ids')
    assert os.path.isfile(path + '.npz')
    stamp = os.path.getmtime(path + '.npz')
    with open(path, 'w') as f:                                    # the cache is newer than the file: the text is not read again
        f.write('not an ARPA file\n')
    os.utime(path, (stamp - 10, stamp - 10))
    again = load_tables(path, chars, 'ids')
    assert all(getattr(first, n).tobytes() == getattr(again, n).tobytes() for n in NgramTables.ARRAYS)
    os.utime(path, (stamp + 10, stamp + 10))                      # the file is newer: parsed again, and it no longer parses
    with pytest.raises(ArpaError):
        load_tables(path, chars, 'ids')


def test_binary_kenlm_files_are_refused(tmp_path):
    from robust_e2e_gan_amd.lib import Re2eError
    p = os.path.join(str(tmp_path), 'lm.bin')
    with open(p, 'wb') as f:
        f.write(b'mmap lm http://kheafield.com/code format version 5\n\x00\x01\x02')
    with pytest.raises(Re2eError) as e:
        load_tables(p, ['a', 'b'], 'symbols')
    assert 'ARPA' in str(e.value)
    with pytest.raises(FileNotFoundError):
        load_tables(os.path.join(str(tmp_path), 'nothing.arpa'), ['a', 'b'])


def _tiny_tables(tmp_path, V=12):
    grams = R.random_model(V, [0, .4, .3], 5)
    return NgramTables.from_arpa(R.write_arpa(os.path.join(str(tmp_path), 't%d.arpa' % V), grams), [str(v) for v in range(V)], 'ids')


def test_decoder_accepts_an_ngram_lm_and_still_refuses_the_rest(tmp_path):
    import __graft_entry__ as g
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    dec = E2E(g._tiny_opt()).dec
    cpu = torch.device('cpu')
    lm = ClassifierWithState(NgramLM(_tiny_tables(tmp_path))).eval()
    assert lm.predictor.normalized and lm.predictor.n_vocab == 12 and lm.predictor.device == cpu
    dec._check_decode_lm(lm, None, cpu)
    dec._check_decode_lm(None, None, cpu)
    with pytest.raises(Re2eError, match='evaluation mode'):
        dec._check_decode_lm(ClassifierWithState(NgramLM(_tiny_tables(tmp_path))).train(), None, cpu)
    with pytest.raises(Re2eError, match='13 labels'):
        dec._check_decode_lm(ClassifierWithState(NgramLM(_tiny_tables(tmp_path, 13))).eval(), None, cpu)
    with pytest.raises(Re2eError, match='is on cpu'):
        dec._check_decode_lm(lm, None, torch.device('cuda:0'))
    with pytest.raises(Re2eError, match='fstlm'):
        dec._check_decode_lm(lm, object(), cpu)
    with pytest.raises(Re2eError, match='out of scope'):
        dec._check_decode_lm(ClassifierWithState(torch.nn.Linear(12, 12)).eval(), None, cpu)
    with pytest.raises(Re2eError):
        dec._check_decode_lm(lm.predictor, None, cpu)            # not wrapped
    dec.fusion = 'cold_fusion'
    with pytest.raises(Re2eError, match='cold_fusion'):
        dec._check_decode_lm(lm, None, cpu)
    with pytest.raises(Re2eError, match='no CPU path'):          # the step itself is a kernel: no quiet host fall-back
        lm.predict(None, np.asarray([11], np.int32))
    with pytest.raises(TypeError):
        NgramLM({'uni_logp': None})


def test_command_line(tmp_path):
    from robust_e2e_gan_amd import recog
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    from robust_e2e_gan_amd.options.test_options import TestOptions
    grams = R.random_model(12, [0, .4, .3], 5)
    path = R.write_arpa(os.path.join(str(tmp_path), 'cli.arpa'), grams)
    chars = [str(v) for v in range(12)]
    base = ['--checkpoints_dir', str(tmp_path), '--lmtype', 'ngram', '--ngram-tokens', 'ids']
    for flag in ('--kenlm', '--ngram-lm'):
        opt = TestOptions().parse(base + [flag, path])
        assert opt.lmtype == 'ngram' and opt.ngram_tokens == 'ids' and opt.kenlm == path
        lm = recog.build_lm(opt, chars, torch.device('cpu'))
        assert isinstance(lm, ClassifierWithState) and isinstance(lm.predictor, NgramLM) and not lm.training and lm.predictor.order == 3
    assert TestOptions().parse([]).ngram_tokens == 'symbols'
    with pytest.raises(Re2eError, match='--kenlm'):
        recog.build_lm(TestOptions().parse(base), chars, torch.device('cpu'))
    binary = os.path.join(str(tmp_path), 'lm.bin')
    with open(binary, 'wb') as f:
        f.write(b'mmap lm \x00')
    with pytest.raises(Re2eError, match='ARPA'):
        recog.build_lm(TestOptions().parse(base + ['--kenlm', binary]), chars, torch.device('cpu'))
    with pytest.raises(Re2eError, match='fstlm'):                 # FST files stay refused
        recog.build_lm(argparse.Namespace(lmtype='fstlm', fstlm_path='x.fst'), chars, torch.device('cpu'))
