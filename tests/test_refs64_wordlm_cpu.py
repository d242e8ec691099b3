"""tests/refs64_wordlm.py (the float64 restatement of LookAheadWordLM / MultiLevelLM that arbitrates model/extlm.py and csrc/wordlm.hip)
against the reference's own ``predict`` chains in tests/golden/wordlm_tiny.npz (make_fixtures_wordlm.py).  CPU only."""
import os

import numpy as np
import pytest

import refs64_wordlm as R

LOGZERO_MAG = 1e9          # entries of this magnitude are upstream's logzero = -1e10: compared exactly


def load(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, 'wordlm_tiny.npz')))
    words, chars = fx['words'].tolist(), fx['chars'].tolist()
    return fx, {w: i for i, w in enumerate(words)}, {c: i for i, c in enumerate(chars)}


def sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def models64(fx, word_dict, char_dict):
    return {'la': R.LookAhead64(sub(fx, 'la.predictor.wordlm.'), word_dict, char_dict),
            'ml': R.MultiLevel64(sub(fx, 'ml.predictor.wordlm.'), sub(fx, 'ml.predictor.subwordlm.'), word_dict, char_dict)}


def run_chain(model, fx):
    """The fixture's chain, one hypothesis per call: (log_y (positions, 3, Vc), final states, every state on the way)."""
    ids, parents = fx['chain.ids'], fx['chain.parents']
    states, out, visited = [None] * 3, [], []
    for i in range(ids.shape[0]):
        if i:
            states = [states[p] for p in parents[i]]
        row = []
        for r in range(3):
            states[r], y = model.forward(states[r], ids[i, r])
            row.append(y)
            visited.append(states[r])
        out.append(np.stack(row))
    return np.stack(out), states, visited


@pytest.mark.parametrize('tag', ['la', 'ml'])
def test_restatement_reproduces_golden_chain(golden_dir, tag):
    """Bound per entry: 2e-5 * max(1, |ref|) (the fixture is the reference's float32 arithmetic) and, for the look-ahead model, the
    cancellation in its float32 cumulative sums: a prefix sum of 32 probabilities carries at most 32 * 2^-25 of rounding, a mass is the
    difference of two, and the log divides that by the mass -- at least the smallest word probability of the chain, which the
    restatement itself provides.  logzero entries must be equal."""
    fx, word_dict, char_dict = load(golden_dir)
    got, states, visited = run_chain(models64(fx, word_dict, char_dict)[tag], fx)
    ref = fx[tag + '.chain.logp'].astype(np.float64)
    assert got.shape == ref.shape
    big = np.abs(ref) >= LOGZERO_MAG
    assert np.array_equal(got[big], ref[big])
    tol = 2e-5 * np.maximum(1.0, np.abs(ref))
    if tag == 'la':
        pmin = min(float(np.diff(np.concatenate([[0.0], st[1]])).min()) for st in visited)
        tol = tol + 2 * 32 * 2.0 ** -25 / pmin
        print('smallest word probability %.3e -> cancellation allowance %.3e' % (pmin, 2 * 32 * 2.0 ** -25 / pmin))
    err = np.abs(got - ref)
    print('%s: max |err| %.3e over %d finite entries (max |ref| %.3f)' % (tag, err[~big].max(), (~big).sum(), np.abs(ref[~big]).max()))
    assert (err[~big] <= tol[~big]).all(), (tag, float((err - tol)[~big].max()))
    key = 0 if tag == 'la' else 1
    for k in ('c1', 'h1', 'c2', 'h2'):
        have = np.stack([st[key][k] for st in states])
        assert np.abs(have - fx['%s.chain.%s' % (tag, k)]).max() <= 2e-5, k
    if tag == 'la':
        assert np.abs(np.stack([st[1] for st in states]) - fx['la.chain.cumsum']).max() <= 32 * 2.0 ** -25 + 2e-6
    else:
        assert np.abs(np.stack([st[2] for st in states]) - fx['ml.chain.wlm_logprobs']).max() <= 2e-5 * np.abs(fx['ml.chain.wlm_logprobs']).max()
        assert np.abs(np.asarray([st[5] for st in states]) - fx['ml.chain.clm_logprob']).max() <= 2e-5 * max(1.0, np.abs(fx['ml.chain.clm_logprob']).max())


def test_chain_visits_every_transition(golden_dir):
    """The chain is only worth its name if it walks every branch: a space at a word end, at a non-end and off the tree, and a label with
    no path."""
    fx, word_dict, char_dict = load(golden_dir)
    la = models64(fx, word_dict, char_dict)['la']
    ids, parents = fx['chain.ids'], fx['chain.parents']
    states, seen = [None] * 3, set()
    for i in range(ids.shape[0]):
        if i:
            states = [states[p] for p in parents[i]]
        for r in range(3):
            if states[r] is not None:
                node, x = states[r][2], int(ids[i, r])
                if x == la.space:
                    seen.add('none' if node is None else 'end' if node.wid >= 0 else 'inner')
                elif node is not None and x not in node.succ:
                    seen.add('off')
            states[r], _ = la.forward(states[r], ids[i, r])
    assert seen == {'none', 'end', 'inner', 'off'}


def test_softmax_cumsum_and_open_vocab_off():
    z = np.array([[0.0, 1.0, -2.0, 30.0], [5.0, 5.0, 5.0, 5.0]])
    c = R.softmax_cumsum(z)
    assert np.allclose(c[:, -1], 1.0, atol=1e-15) and (np.diff(c, axis=1) >= 0).all()
    assert np.allclose(c[1], [0.25, 0.5, 0.75, 1.0])
    word_dict = {'<blank>': 0, '<unk>': 1, '<eos>': 2, 'ab': 3}
    char_dict = {'<blank>': 0, '<space>': 1, 'a': 2, 'b': 3, '<eos>': 4}
    rng = np.random.RandomState(0)
    p = {'embed.weight': rng.randn(4, 3), 'lo.weight': rng.randn(4, 5), 'lo.bias': rng.randn(4)}
    for lay, I in (('l1.', 3), ('l2.', 5)):
        p.update({lay + 'weight_ih': rng.randn(20, I), lay + 'weight_hh': rng.randn(20, 5), lay + 'bias_ih': rng.randn(20), lay + 'bias_hh': rng.randn(20)})
    la = R.LookAhead64(p, word_dict, char_dict, open_vocab=False)
    st, y = la.forward(None, 4)
    st, y = la.forward(st, 3)                                  # 'b' at the root: no path
    assert st[2] is None and (y == R.LOGZERO).all()
    st, y = la.forward(st, 2)                                  # stays dead until a space
    assert st[2] is None and (y == R.LOGZERO).all()
    st, y = la.forward(st, 1)
    assert st[2] is la.root and y[1] == np.log(R.ZERO)
