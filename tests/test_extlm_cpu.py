"""model/extlm.py on the host: the flat LexicalTree against the nested tree of tests/refs64_wordlm.py, the inclusion rules, the state-dict
names of the two models.  CPU only (the predictors themselves have no CPU path: tests/test_recog_wordlm_gpu.py)."""
import os
import random

import numpy as np
import pytest
import torch

import refs64_wordlm as R


def tiny_dicts(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, 'wordlm_tiny.npz')))
    return fx, {w: i for i, w in enumerate(fx['words'].tolist())}, {c: i for i, c in enumerate(fx['chars'].tolist())}


def generated_dicts(n_words=2000, seed=5):
    """<blank>, <unk>, <eos>, then distinct random words of 1 .. 7 letters over a .. z (many nested prefixes), every 50th with a symbol
    outside the character set; ids in order of generation, so the word-set ranges are not contiguous."""
    rng = random.Random(seed)
    chars = ['<blank>', '<space>'] + [chr(ord('a') + i) for i in range(26)] + ["'", '<eos>']
    words = ['<blank>', '<unk>', '<eos>']
    seen = set(words)
    while len(words) < n_words:
        w = ''.join(rng.choice('abcdefghijklmnopqrstuvwxyz\'') for _ in range(rng.randint(1, 7)))
        if len(words) % 50 == 0:
            w = w + '#'
        if w not in seen:
            seen.add(w)
            words.append(w)
    return {w: i for i, w in enumerate(words)}, {c: i for i, c in enumerate(chars)}


def assert_same_tree(flat, root):
    nested = R.tree_nodes(root)
    assert flat.n_nodes == len(nested)
    number = {id(nd): k for k, nd in enumerate(nested)}
    assert flat.child_off[0] == 0 and flat.child_off[-1] == flat.n_children == len(nested) - 1
    for k, nd in enumerate(nested):
        assert flat.wid[k] == nd.wid, k
        assert (flat.lo[k], flat.hi[k]) == ((-1, -1) if nd.lo is None else (nd.lo, nd.hi)), k
        assert flat.children(k) == {c: number[id(ch)] for c, ch in nd.succ.items()}, k
        a, b = flat.child_off[k], flat.child_off[k + 1]
        assert (np.diff(flat.child_label[a:b]) > 0).all(), k                 # ascending inside a node
        for c, ch in nd.succ.items():
            assert flat.step(k, c) == number[id(ch)]
    for arr in (flat.wid, flat.lo, flat.hi, flat.child_off, flat.child_label, flat.child_node):
        assert arr.dtype == np.int32


def test_flat_tree_is_the_nested_tree_tiny(golden_dir):
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    _, word_dict, char_dict = tiny_dicts(golden_dir)
    flat = LexicalTree(word_dict, char_dict, word_dict['<unk>'])
    assert_same_tree(flat, R.make_tree(word_dict, char_dict, word_dict['<unk>']))
    a, b = char_dict['a'], char_dict['b']
    ab = flat.step(flat.step(0, a), b)
    assert flat.wid[flat.step(0, a)] == word_dict['a'] and flat.wid[ab] == word_dict['ab']          # nested prefixes: a, ab, abc
    assert flat.wid[flat.step(ab, char_dict['c'])] == word_dict['abc']
    assert flat.step(0, char_dict['<space>']) == -1 and flat.step(-1, a) == -1 and flat.step(ab, a) == -1


def test_flat_tree_is_the_nested_tree_2000_words():
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    word_dict, char_dict = generated_dicts()
    flat = LexicalTree(word_dict, char_dict, word_dict['<unk>'])
    assert flat.n_nodes > 2000
    assert_same_tree(flat, R.make_tree(word_dict, char_dict, word_dict['<unk>']))


def test_inclusion_rules():
    """Skipped: ids <= 0, <unk>, words with a symbol outside the subword set; subword symbols are the single characters of the word."""
    from robust_e2e_gan_amd.model.extlm import LexicalTree
    char_dict = {'<blank>': 0, '<space>': 1, 'a': 2, 'b': 3, '<': 4, '<eos>': 5}
    word_dict = {'b': 0, 'ba': -3, '<unk>': 1, 'a': 1, '<eos>': 2, 'ab': 3, 'ax': 4, 'bb': 7}
    flat = LexicalTree(word_dict, char_dict, 1)
    words = sorted(int(w) for w in flat.wid if w >= 0)
    assert words == [3, 7]                      # 'ab', 'bb'; 'b' (id 0), 'ba' (< 0), 'a' (the <unk> id), 'ax' (x), '<eos>' / '<unk>' (e, o, s, u, ...) are out
    assert flat.n_nodes == 5 and flat.max_wid == 7
    na = flat.step(0, 2)
    assert (flat.lo[na], flat.hi[na], flat.wid[na]) == (2, 3, -1)
    empty = LexicalTree({'<unk>': 1, '<eos>': 2}, char_dict, 1)
    assert empty.n_nodes == 1 and empty.n_children == 0 and empty.child_off.tolist() == [0, 0] and empty.max_wid == -1


def test_reference_named_state_dicts_load_strictly(golden_dir):
    from robust_e2e_gan_amd.model.extlm import LookAheadWordLM, MultiLevelLM
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    fx, word_dict, char_dict = tiny_dicts(golden_dir)
    la = ClassifierWithState(LookAheadWordLM(RNNLM(len(word_dict), 5, 8), word_dict, char_dict))
    ml = ClassifierWithState(MultiLevelLM(RNNLM(len(word_dict), 5, 8), RNNLM(len(char_dict), 6, 10), word_dict, char_dict))
    for tag, lm in (('la', la), ('ml', ml)):
        sd = {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag + '.predictor.')}
        assert sd and all(k.startswith(('predictor.wordlm.', 'predictor.subwordlm.')) for k in sd)
        lm.load_state_dict(sd, strict=True)
        assert torch.equal(lm.predictor.wordlm.lo.weight, sd['predictor.wordlm.lo.weight'])
    assert any(k.startswith('predictor.subwordlm.') for k in ml.state_dict()) and not any('subwordlm' in k for k in la.state_dict())
    p = la.predictor
    assert p.normalized and (p.oov_penalty, p.open_vocab, p.subword_dict_size) == (0.0001, True, 12)
    assert (p.space, p.eos, p.word_unk, p.word_eos) == (1, 11, 1, 2) and (p.logzero, p.zero) == (-10000000000.0, 1.0e-10)
    q = ml.predictor
    assert q.normalized and (q.subwordlm_weight, q.log_oov_penalty, q.open_vocab, q.subword_dict_size) == (0.8, 0.0, True, 12)


def test_constructors_refuse_what_cannot_run(golden_dir):
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.extlm import LookAheadWordLM, MultiLevelLM
    from robust_e2e_gan_amd.model.lm import RNNLM
    _, word_dict, char_dict = tiny_dicts(golden_dir)
    with pytest.raises(Re2eError):
        LookAheadWordLM(RNNLM(len(word_dict) - 1, 5, 8), word_dict, char_dict)              # a word id beyond the word LM's vocabulary
    with pytest.raises(Re2eError):
        LookAheadWordLM(torch.nn.Linear(3, 3), word_dict, char_dict)
    with pytest.raises(Re2eError):
        MultiLevelLM(RNNLM(len(word_dict), 5, 8), RNNLM(len(char_dict) + 1, 6, 10), word_dict, char_dict)
    with pytest.raises(KeyError):
        LookAheadWordLM(RNNLM(len(word_dict), 5, 8), {'a': 1}, char_dict)
    la = LookAheadWordLM(RNNLM(len(word_dict), 5, 8), word_dict, char_dict).eval()
    with pytest.raises(Re2eError):
        la(None, np.asarray([11]))                                                           # CPU-resident: there is no CPU path
