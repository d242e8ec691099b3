"""Word-level LMs in the beam search on the GPU (robust_e2e_gan_amd/model/extlm.py, csrc/wordlm.hip, model/beam_search.py) against the
reference's own LookAheadWordLM / MultiLevelLM and beam search (tests/golden/wordlm_tiny.npz, make_fixtures_wordlm.py), the kernels against
the arbiter path at production widths, and what the decoder refuses."""
import argparse
import random

import numpy as np
import pytest
import torch

from test_modules_gpu import DEV, _fx, _load, _opt

pytestmark = pytest.mark.gpu

LM_CONFIGS_EXTRA = [('ctc_only', 2, 0.0, 1.0, 0.0, 0.0, 2)]
LM_WEIGHTS = (0.2, 1.0)
LOGZERO_MAG = 1e9


def _dicts(fx):
    return {w: i for i, w in enumerate(fx['words'].tolist())}, {c: i for i, c in enumerate(fx['chars'].tolist())}


def _tiny_lm(fx, tag, **kw):
    from robust_e2e_gan_amd.model.extlm import LookAheadWordLM, MultiLevelLM
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    word_dict, char_dict = _dicts(fx)
    if tag == 'la':
        lm = ClassifierWithState(LookAheadWordLM(RNNLM(len(word_dict), 5, 8), word_dict, char_dict, **kw))
    else:
        lm = ClassifierWithState(MultiLevelLM(RNNLM(len(word_dict), 5, 8), RNNLM(len(char_dict), 6, 10), word_dict, char_dict, **kw))
    lm.load_state_dict({k[len(tag) + 1:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag + '.predictor.')}, strict=True)
    return lm.to(DEV).eval()


def _args(beam, penalty, ctcw, maxr, minr, nbest, lm_weight):
    return argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=lm_weight)


class _arbiter(object):
    """The predictors over torch ops and a host walk of the tree (model/extlm.py ARBITER_PATH) for the duration of a ``with`` block."""

    def __enter__(self):
        from robust_e2e_gan_amd.model import extlm
        extlm.ARBITER_PATH = True

    def __exit__(self, *exc):
        from robust_e2e_gan_amd.model import extlm
        extlm.ARBITER_PATH = False


def _nan_buffers(monkeypatch):
    """Every output buffer of the word-level step and of the RNNLMs under it starts as NaN: a kernel that leaves an element unwritten shows."""
    from robust_e2e_gan_amd.model import extlm, lm
    for mod in (extlm, lm):
        monkeypatch.setattr(mod, '_empty', lambda *shape, **kw: torch.full(shape, float('nan') if kw.get('dtype', torch.float32).is_floating_point
                                                                          else -12345, **kw))


def _chain_close(what, got, ref, tol=2e-5):
    """test_recog_lm_gpu.py's chain bound -- max error <= 2e-5 of the largest magnitude -- over the entries that are not upstream's logzero
    (-1e10, which would make that scale meaningless); those must be equal."""
    got, ref = got.detach().double().cpu().numpy(), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    big = np.abs(ref) >= LOGZERO_MAG
    assert np.array_equal(got[big], ref[big]), what
    assert np.isfinite(got).all(), '%s: %d entries not finite' % (what, int((~np.isfinite(got)).sum()))
    err, scale = np.abs(got - ref)[~big].max(), np.abs(ref[~big]).max()
    print('%s: max err %.3e (scale %.3e)' % (what, err, scale))
    assert err <= tol * scale, '%s: max err %.3e vs scale %.3e' % (what, err, scale)


@pytest.mark.parametrize('path', ['kernels', 'arbiter'])
@pytest.mark.parametrize('tag', ['la', 'ml'])
@pytest.mark.parametrize('host_labels', [True, False])
def test_predict_chain_matches_reference(golden_dir, tag, path, host_labels, monkeypatch):
    """10 positions x 3 rows of ClassifierWithState.predict with the state rows permuted (some repeated) between positions -- a space at a
    word end, at a non-end and from node None, labels off the tree: the reference's log-probabilities at every position and its final
    state.  With the labels handed down on the host and without (one read-back of x).  The input state must come back untouched."""
    fx = _fx(golden_dir, 'wordlm_tiny.npz')
    lm = _tiny_lm(fx, tag)
    _nan_buffers(monkeypatch)
    ids, parents = fx['chain.ids'], fx['chain.parents']
    state = None
    ctx = _arbiter() if path == 'arbiter' else None
    if ctx:
        ctx.__enter__()
    try:
        for i in range(ids.shape[0]):
            if state is not None:
                par = torch.from_numpy(parents[i]).to(DEV)
                state = {k: v.index_select(0, par) for k, v in state.items()}
                keep = {k: v.clone() for k, v in state.items()}
            x = torch.from_numpy(ids[i])
            new, lp = lm.predict(state, x, labels=ids[i]) if host_labels else lm.predict(state, x.to(DEV))
            if state is not None:
                for k, v in keep.items():
                    assert torch.equal(state[k], v), 'position %d: forward modified its input state (%s)' % (i, k)
            for k, v in new.items():
                assert v.shape[0] == 3, (k, v.shape)
            state = new
            _chain_close('%s %s logp[%d]' % (tag, path, i), lp, fx[tag + '.chain.logp'][i])
    finally:
        if ctx:
            ctx.__exit__()
    for k in ('c1', 'h1', 'c2', 'h2') + (('cumsum',) if tag == 'la' else ('sub_c1', 'sub_h1', 'sub_c2', 'sub_h2', 'wlm_logprobs', 'clm_logprob')):
        _chain_close('%s %s final %s' % (tag, path, k), state[k], fx['%s.chain.%s' % (tag, k)])


@pytest.mark.parametrize('tag', ['la', 'ml'])
def test_recognize_with_word_lm_matches_reference_nbest(golden_dir, tag):
    """E2E.recognize(..., rnnlm=lm) reproduces the reference's n-best lists with its word-level LMs for the four search configurations of
    recog_tiny.npz plus ctc_weight = 1.0, at lm_weight 0.2 and 1.0, three utterances each (the generator asserts that every list differs
    from its LM-free counterpart)."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'wordlm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx, tag)
    feats = torch.from_numpy(base['feats'])
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS + LM_CONFIGS_EXTRA:
        for w in LM_WEIGHTS:
            for u, T in enumerate(base['lens'].tolist()):
                got = asr.recognize(feats[u:u + 1, :T], _args(beam, penalty, ctcw, maxr, minr, nbest, w), fx['chars'].tolist(), rnnlm=lm)
                check_nbest(got, fx, '%s.%s.w%03d' % (tag, name, int(round(w * 100))), u)


@pytest.mark.parametrize('tag', ['la', 'ml'])
def test_recognize_batch_with_word_lm_matches_reference_nbest(golden_dir, tag):
    """The same lists through E2E.recognize_batch with all three utterances in one call."""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'wordlm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx, tag)
    feats, lens = torch.from_numpy(base['feats']), base['lens'].tolist()
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS + LM_CONFIGS_EXTRA:
        for w in LM_WEIGHTS:
            got = asr.recognize_batch(feats, lens, _args(beam, penalty, ctcw, maxr, minr, nbest, w), fx['chars'].tolist(), rnnlm=lm)
            assert len(got) == len(lens)
            for u in range(len(lens)):
                check_nbest(got[u], fx, '%s.%s.w%03d' % (tag, name, int(round(w * 100))), u)


@pytest.mark.parametrize('tag', ['la', 'ml'])
def test_zero_lm_weight_reproduces_lm_free_nbest(golden_dir, tag):
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'wordlm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx, tag)
    feats = torch.from_numpy(base['feats'])
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS:
        for u, T in enumerate(base['lens'].tolist()):
            got = asr.recognize(feats[u:u + 1, :T], _args(beam, penalty, ctcw, maxr, minr, nbest, 0.0), fx['chars'].tolist(), rnnlm=lm)
            check_nbest(got, base, name, u)


def _full_width_dicts(n_words=65000, seed=3):
    rng = random.Random(seed)
    letters = [chr(ord('a') + i) for i in range(26)] + [chr(ord('A') + i) for i in range(23)]
    chars = ['<blank>', '<space>'] + letters + ['<eos>']
    assert len(chars) == 52
    words, seen = ['<blank>', '<unk>', '<eos>'], set()
    while len(words) < n_words:
        w = ''.join(rng.choice(letters[:12]) for _ in range(rng.randint(1, 6)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return {w: i for i, w in enumerate(words)}, {c: i for i, c in enumerate(chars)}, chars


@pytest.mark.parametrize('tag', ['la', 'ml'])
def test_recognize_full_width_kernels_vs_arbiter(tag):
    """Attention-only search with 52 labels over 200 encoder frames, at most 20 positions, beam 12, and a 65000-word LM of the recipe's width
    (650 units): the kernels and the arbiter path return the same n-best list.  A fresh LM (+-0.1) has nearly flat rows, so the output
    layers are widened and the test first checks that the LM changes the n-best list at all."""
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.extlm import LookAheadWordLM, MultiLevelLM
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    word_dict, char_dict, chars = _full_width_dicts()
    opt = config4_opt(odim=52, char_list=chars)
    torch.manual_seed(31)
    asr = E2E(opt).to(DEV)
    torch.manual_seed(32)
    wordlm = RNNLM(len(word_dict), 64, 650)
    wordlm.lo.weight.data.uniform_(-0.5, 0.5)
    if tag == 'la':
        pred = LookAheadWordLM(wordlm, word_dict, char_dict)
    else:
        sub = RNNLM(52, 64, 650)
        sub.lo.weight.data.uniform_(-0.5, 0.5)
        pred = MultiLevelLM(wordlm, sub, word_dict, char_dict)
    lm = ClassifierWithState(pred).to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(1, 800, 80, generator=g)
    args = _args(12, 0.0, 0.0, 0.1, 0.0, 5, 0.5)
    free = asr.recognize(feats, args, chars)
    fused = asr.recognize(feats, args, chars, rnnlm=lm)
    assert [h['yseq'] for h in fused] != [h['yseq'] for h in free], 'the LM does not change the n-best list: the comparison below would be vacuous'
    with _arbiter():
        arb = asr.recognize(feats, args, chars, rnnlm=lm)
    assert len(fused) == len(arb) == 5
    for a, b in zip(fused, arb):
        assert a['yseq'] == b['yseq'], (a['yseq'], b['yseq'])
        assert abs(a['score'] - b['score']) <= 2e-3 * max(1.0, abs(b['score'])), (a['score'], b['score'])


def test_word_level_lms_the_decoder_refuses(golden_dir):
    """A subword_dict_size other than the decoder's label count, a CPU-resident word LM and training mode are Re2eErrors."""
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.extlm import LookAheadWordLM, MultiLevelLM
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'wordlm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    word_dict, char_dict = _dicts(fx)
    chars = fx['chars'].tolist()
    x = torch.from_numpy(base['feats'])[2:3, :20]
    args = _args(2, 0.0, 0.0, 0.0, 0.0, 1, 0.2)
    for tag in ('la', 'ml'):
        assert asr.recognize(x, args, chars, rnnlm=_tiny_lm(fx, tag))                 # the supported case, for contrast
        assert asr.recognize_batch(x, [20], args, chars, rnnlm=_tiny_lm(fx, tag))
    wider = dict(char_dict, j=12)
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=ClassifierWithState(LookAheadWordLM(RNNLM(len(word_dict), 5, 8), word_dict, wider)).to(DEV).eval())
    with pytest.raises(Re2eError):
        asr.recognize_batch(x, [20], args, chars, rnnlm=ClassifierWithState(MultiLevelLM(RNNLM(len(word_dict), 5, 8), RNNLM(13, 6, 10), word_dict,
                                                                                         wider)).to(DEV).eval())
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=ClassifierWithState(LookAheadWordLM(RNNLM(len(word_dict), 5, 8), word_dict, char_dict)).eval())     # on the CPU
    ml = _tiny_lm(fx, 'ml')
    ml.predictor.wordlm.cpu()
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=ml)                                       # the word LM alone on the CPU
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=_tiny_lm(fx, 'la').train())
    la = _tiny_lm(fx, 'la')
    la.predictor.wordlm.train()
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=la)
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=_tiny_lm(fx, 'la').predictor)             # not wrapped: no predict()
