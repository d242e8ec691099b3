"""RNNLM shallow fusion on the GPU (robust_e2e_gan_amd/model/lm.py, csrc/rnnlm.hip, model/beam_search.py) against the reference's own
beam search with its own RNNLM (tests/golden/recog_lm_tiny.npz, make_fixtures_recog_lm.py), against float64 recurrences at the recipe's
widths, and the fused few-row kernels against the composed path over the general entry points."""
import argparse
import math

import numpy as np
import pytest
import torch

from test_modules_gpu import DEV, _fx, _load, _opt

pytestmark = pytest.mark.gpu

LM_CONFIGS_EXTRA = [('ctc_only', 2, 0.0, 1.0, 0.0, 0.0, 2)]      # ctc_weight == 1.0: every label is a CTC candidate (ctc_beam = V)
LM_WEIGHTS = (0.2, 1.0)
STATE_KEYS = ('c1', 'h1', 'c2', 'h2')


def _tiny_lm(fx):
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    lm = ClassifierWithState(RNNLM(12, 6, 10))
    lm.load_state_dict({k[len('lm.'):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith('lm.')}, strict=True)
    return lm.to(DEV).eval()


def _args(beam, penalty, ctcw, maxr, minr, nbest, lm_weight):
    return argparse.Namespace(beam_size=beam, penalty=penalty, ctc_weight=ctcw, maxlenratio=maxr, minlenratio=minr, nbest=nbest, lm_weight=lm_weight)


class _composed(object):
    """The LM step over the general entry points (model/lm.py COMPOSED_PATH) for the duration of a ``with`` block."""

    def __enter__(self):
        from robust_e2e_gan_amd.model import lm
        lm.COMPOSED_PATH = True

    def __exit__(self, *exc):
        from robust_e2e_gan_amd.model import lm
        lm.COMPOSED_PATH = False


class _host_ctc(object):
    def __enter__(self):
        from robust_e2e_gan_amd.model import beam_search
        beam_search.HOST_CTC_SCORER = True

    def __exit__(self, *exc):
        from robust_e2e_gan_amd.model import beam_search
        beam_search.HOST_CTC_SCORER = False


def _nan_buffers(monkeypatch):
    """Every output buffer of the LM step starts as NaN: a kernel that leaves an element unwritten shows."""
    from robust_e2e_gan_amd.model import lm
    monkeypatch.setattr(lm, '_empty', lambda *shape, **kw: torch.full(shape, float('nan'), **kw))


@pytest.mark.parametrize('path', ['fused', 'composed'])
def test_predict_chain_matches_reference(golden_dir, path, monkeypatch):
    """8 positions x 3 rows of ClassifierWithState.predict with the state rows permuted (one repeated) between positions: the
    reference's log-probabilities at every position and its final state.  Bound: max error over max magnitude <= 2e-5 (what
    test_kernels_gpu.py holds fp32 products of short K to)."""
    from test_kernels_gpu import close
    fx = _fx(golden_dir, 'recog_lm_tiny.npz')
    lm = _tiny_lm(fx)
    _nan_buffers(monkeypatch)
    ids, parents = fx['chain.ids'], fx['chain.parents']
    state = None
    ctx = _composed() if path == 'composed' else None
    if ctx:
        ctx.__enter__()
    try:
        for i in range(ids.shape[0]):
            if state is not None:
                par = torch.from_numpy(parents[i]).to(DEV)
                state = {k: v.index_select(0, par) for k, v in state.items()}
            state, lp = lm.predict(state, torch.from_numpy(ids[i]))
            err = close('%s logp[%d]' % (path, i), lp, torch.from_numpy(fx['chain.logp'][i]), tol=2e-5, atol=0.0)
            print('%s position %d: log-prob max err %.3e (scale %.3e)' % (path, i, err, np.abs(fx['chain.logp'][i]).max()))
    finally:
        if ctx:
            ctx.__exit__()
    for k in STATE_KEYS:
        err = close('%s final %s' % (path, k), state[k], torch.from_numpy(fx['chain.' + k]), tol=2e-5, atol=0.0)
        print('%s final %s: max err %.3e' % (path, k, err))


@pytest.mark.parametrize('scorer', ['device_ctc', 'host_ctc'])
def test_recognize_with_lm_matches_reference_nbest(golden_dir, scorer):
    """E2E.recognize(..., rnnlm=lm) reproduces the reference's n-best lists with its RNNLM for the four search configurations of
    recog_tiny.npz plus ctc_weight = 1.0, at lm_weight 0.2 and 1.0, three utterances each.  (The generator asserts that every one of
    these lists differs from its LM-free counterpart, so a search that ignored the LM cannot pass.)"""
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'recog_lm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx)
    feats = torch.from_numpy(base['feats'])
    ctx = _host_ctc() if scorer == 'host_ctc' else None
    if ctx:
        ctx.__enter__()
    try:
        for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS + LM_CONFIGS_EXTRA:
            for w in LM_WEIGHTS:
                for u, T in enumerate(base['lens'].tolist()):
                    got = asr.recognize(feats[u:u + 1, :T], _args(beam, penalty, ctcw, maxr, minr, nbest, w), [str(i) for i in range(12)], rnnlm=lm)
                    check_nbest(got, fx, '%s.w%03d' % (name, int(round(w * 100))), u)
    finally:
        if ctx:
            ctx.__exit__()


def test_zero_lm_weight_reproduces_lm_free_nbest(golden_dir):
    from test_oracle_golden import RECOG_CONFIGS, check_nbest
    from robust_e2e_gan_amd.model.e2e_model import E2E
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'recog_lm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx)
    feats = torch.from_numpy(base['feats'])
    for name, beam, penalty, ctcw, maxr, minr, nbest in RECOG_CONFIGS:
        for u, T in enumerate(base['lens'].tolist()):
            got = asr.recognize(feats[u:u + 1, :T], _args(beam, penalty, ctcw, maxr, minr, nbest, 0.0), [str(i) for i in range(12)], rnnlm=lm)
            check_nbest(got, base, name, u)


def _cpu_step(sd, state, ids, dtype):
    """RNNLM.forward + log-softmax (model/lm.py:135-146 upstream) in plain torch on the CPU."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    n, H = len(ids), p['predictor.l1.weight_hh'].shape[1]
    if state is None:
        state = {k: torch.zeros(n, H, dtype=dtype) for k in STATE_KEYS}

    def cell(x, h, c, pre):
        g = x @ p[pre + 'weight_ih'].t() + p[pre + 'bias_ih'] + h @ p[pre + 'weight_hh'].t() + p[pre + 'bias_hh']
        i, f, gg, o = g.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        return torch.sigmoid(o) * torch.tanh(c), c
    h1, c1 = cell(p['predictor.embed.weight'][ids], state['h1'], state['c1'], 'predictor.l1.')
    h2, c2 = cell(h1, state['h2'], state['c2'], 'predictor.l2.')
    y = h2 @ p['predictor.lo.weight'].t() + p['predictor.lo.bias']
    return {'c1': c1, 'h1': h1, 'c2': c2, 'h2': h2}, torch.log_softmax(y, 1)


def _rel_err(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


@pytest.mark.parametrize('V,I,H,n', [(4233, 256, 650, 1), (4233, 256, 650, 5), (4233, 256, 650, 12), (4233, 256, 650, 13), (4233, 256, 650, 33),
                                     (4233, 256, 650, 64), (101, 37, 75, 7)])
def test_few_row_kernels_at_production_widths(V, I, H, n, monkeypatch):
    """The fused step at the recipe's widths (H = 650: rows on 8-byte boundaries only; V = 4233 odd) and at widths where nothing is
    even, for row counts around every tile edge, over three chained positions whose parent gather repeats and drops rows.  Arbiter:
    the same recurrences in float64 on the CPU; bound 2e-4 of the tensor's magnitude (test_kernels_gpu.py's bar for fp32 products with
    K in the hundreds to thousands) on the log-probabilities and the four state tensors.  Buffers start as NaN."""
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    torch.manual_seed(1000 + n + V)
    lm = ClassifierWithState(RNNLM(V, I, H)).eval()
    sd = {k: v.clone() for k, v in lm.state_dict().items()}
    lm = lm.to(DEV)
    _nan_buffers(monkeypatch)
    g = torch.Generator().manual_seed(n)
    parents = (torch.arange(n) * 2) // 3                     # 0, 0, 1, 2, 2, 3, ...: repeats rows and drops the upper third
    st_dev, st64, st32 = None, None, None
    for pos in range(3):
        ids = torch.randint(0, V, (n,), generator=g)
        if pos:
            st_dev = {k: v.index_select(0, parents.to(DEV)) for k, v in st_dev.items()}
            st64 = {k: v.index_select(0, parents) for k, v in st64.items()}
            st32 = {k: v.index_select(0, parents) for k, v in st32.items()}
        st_dev, lp = lm.predict(st_dev, ids)
        st64, lp64 = _cpu_step(sd, st64, ids, torch.float64)
        st32, lp32 = _cpu_step(sd, st32, ids, torch.float32)
        got = dict(st_dev, logp=lp)
        ref64, ref32 = dict(st64, logp=lp64), dict(st32, logp=lp32)
        for k in STATE_KEYS + ('logp',):
            out = got[k].cpu()
            assert out.shape == ref64[k].shape, (k, out.shape, ref64[k].shape)
            assert bool(torch.isfinite(out).all()), 'position %d %s: %d elements not finite (not written?)' % (pos, k, int((~torch.isfinite(out)).sum()))
            err, own = _rel_err(out, ref64[k]), _rel_err(ref32[k], ref64[k])
            print('V=%d I=%d H=%d n=%d position %d %s: err/scale %.3e (float32 torch-CPU vs float64: %.3e)' % (V, I, H, n, pos, k, err, own))
            assert math.isfinite(err) and err <= 2e-4, ('V=%d I=%d H=%d n=%d position %d %s: err/scale %.3e > 2e-4; float32 torch on the CPU is '
                                                        '%.3e from float64' % (V, I, H, n, pos, k, err, own))


def test_recognize_full_width_fused_vs_composed_lm():
    """Joint CTC/attention search at the config-4 width (V = 4233, T' = 200; the set-up of
    test_recognize_full_width_device_ctc_vs_host_ctc) with the recipe's LM (256 / 650 units), beam 12, lm_weight 0.2: the few-row
    kernels and the composed path return the same n-best list.  A fresh LM (+-0.1) has nearly flat rows, so lo.weight is widened and
    the test first checks that the LM changes the n-best list at all."""
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    opt = config4_opt()
    torch.manual_seed(21)
    asr = E2E(opt).to(DEV)
    torch.manual_seed(22)
    lm = ClassifierWithState(RNNLM(opt.odim, 256, 650))
    lm.predictor.lo.weight.data.uniform_(-0.5, 0.5)
    lm = lm.to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(1, 800, 80, generator=g)
    args = _args(12, 0.0, 0.3, 0.08, 0.0, 5, 0.2)
    free = asr.recognize(feats, args, opt.char_list)
    fused = asr.recognize(feats, args, opt.char_list, rnnlm=lm)
    assert [h['yseq'] for h in fused] != [h['yseq'] for h in free], 'the LM does not change the n-best list: the comparison below would be vacuous'
    with _composed():
        composed = asr.recognize(feats, args, opt.char_list, rnnlm=lm)
    assert len(fused) == len(composed) == 5
    for a, b in zip(fused, composed):
        assert a['yseq'] == b['yseq'], (a['yseq'], b['yseq'])
        assert abs(a['score'] - b['score']) <= 2e-3 * max(1.0, abs(b['score'])), (a['score'], b['score'])


def test_unsupported_language_models_are_refused(golden_dir):
    from robust_e2e_gan_amd.lib import Re2eError
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.lm import ClassifierWithState
    base, fx = _fx(golden_dir, 'recog_tiny.npz'), _fx(golden_dir, 'recog_lm_tiny.npz')
    asr = _load(E2E(_opt()), base, 'p.')
    lm = _tiny_lm(fx)
    x = torch.from_numpy(base['feats'])[2:3, :20]
    args = _args(2, 0.0, 0.0, 0.0, 0.0, 1, 0.2)
    chars = [str(i) for i in range(12)]
    assert asr.recognize(x, args, chars, rnnlm=lm)                                   # the supported case, for contrast
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, fstlm=object())                                # n-gram / FST LM
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=lm, fstlm=object())
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=ClassifierWithState(torch.nn.Linear(12, 12)).to(DEV).eval())    # not an RNNLM (word-level LMs, FS-RNN)
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=lm.predictor)                            # not wrapped: no predict()
    with pytest.raises(Re2eError):
        E2E(argparse.Namespace(**{**vars(_opt()), 'fusion': 'cold_fusion'}))
    asr.dec.fusion = 'cold_fusion'
    with pytest.raises(Re2eError):
        asr.recognize(x, args, chars, rnnlm=lm)
