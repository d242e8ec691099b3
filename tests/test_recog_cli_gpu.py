"""The recognisers from the command line (robust_e2e_gan_amd.joint_recog / asr_recog over recog.run) on the fixture of tests/recog_fixture.py:
five utterances of 37 / 29 / 20 / 33 / 20 frames, beam 4, nbest 4, ctc-weight 0.3.  Every n-best list the command line writes is compared with
the module API used utterance by utterance (decode one record -> enhancer -> FbankModel(., cmvn) -> E2E.recognize): token ids and their
order exactly, scores within 1e-5 * max(1, |score|) -- the bar of tests/test_recog_batch_gpu.py, since a batch of another composition may
run its products on another plan.  That this bar cannot hide a reordered list is a precondition asserted here, not assumed: adjacent n-best
scores of every utterance are at least 1e-3 apart (tests/recog_fixture.py chose the feature seed for it on the CPU)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import recog_fixture as RF
import refs_align

gpu = pytest.mark.gpu
DEV = 'cuda:0'
TOL, GAP = 1e-5, 1e-3


@pytest.fixture(scope='module')
def fix(tmp_path_factory, golden_dir):
    return RF.build(str(tmp_path_factory.mktemp('recog')), golden_dir)


def _models(fix):
    from robust_e2e_gan_amd.model.e2e_model import E2E
    from robust_e2e_gan_amd.model.enhance_model import EnhanceModel
    from robust_e2e_gan_amd.model.feat_model import FbankModel
    enh, fb, asr = EnhanceModel(fix['opt']), FbankModel(fix['opt']), E2E(fix['opt'])
    enh.load_state_dict(RF.sub(fix['fx'], 'enh.'), strict=True)
    asr.load_state_dict(RF.sub(fix['fx'], 'asr.'), strict=True)
    return enh.to(DEV).eval(), fb.to(DEV).eval(), asr.to(DEV).eval()


def _api(fix, enhance, lm=None, lm_weight=0.1):
    """utt -> n-best through the module API, one utterance at a time; asserts the gap precondition."""
    from robust_e2e_gan_amd.data import kaldi_io
    from robust_e2e_gan_amd.data.mix_data_loader import decode_pad_device
    enh, fb, asr = _models(fix)
    args = argparse.Namespace(lm_weight=lm_weight, **RF.BEAM)
    cmvn, fcm = torch.from_numpy(fix['cmvn']), torch.from_numpy(fix['fbank_cmvn']).to(DEV)
    out = {}
    with torch.no_grad():
        for line in open(os.path.join(fix['data'], 'feats.scp')):
            utt, path = line.split()
            raw = kaldi_io.read_mat_raw(path)
            x, x_log = decode_pad_device([raw], DEV, None, cmvn, want_log=True)
            if enhance:
                x = enh(x, x_log, torch.IntTensor([raw.rows]))
            nb = asr.recognize(fb(x, fcm), args, fix['opt'].char_list, rnnlm=lm)
            s = [h['score'] for h in nb]
            print('GAP %s enhance=%d lm=%d  %s' % (utt, enhance, lm is not None, ['%.5f' % (a - b) for a, b in zip(s, s[1:])]))
            assert len(nb) == 4 and all(a - b >= GAP for a, b in zip(s, s[1:])), (utt, s)
            out[utt] = nb
    return out


def _cli(fix, mode, name, extra):
    from robust_e2e_gan_amd import asr_recog, joint_recog
    result = os.path.join(fix['root'], name, 'data.json')
    (joint_recog if mode == 'joint' else asr_recog).main(fix['argv'] + ['--result-label', result] + extra)
    with open(result, 'rb') as f:
        return json.loads(f.read().decode('utf_8'))['utts'], os.path.dirname(result)


def _check(utts, want):
    assert sorted(utts) == sorted(RF.UTTS)
    chars = ['<blank>'] + RF.SYMBOLS + ['<eos>']
    for utt, ref_ids, text in zip(RF.UTTS, RF.targets(), RF.TEXTS):
        e, nb = utts[utt], want[utt]
        assert e['utt2spk'] == utt.split('-')[0]
        o = e['output'][0]
        assert set(o) == {'name', 'text', 'token', 'tokenid', 'rec_tokenid', 'rec_token', 'rec_text'} and o['name'] == 'target1'
        assert o['tokenid'] == ' '.join(str(t) for t in ref_ids) and o['text'] == text.replace('<space>', ' ')
        assert o['rec_tokenid'] == ' '.join(str(t) for t in nb[0]['yseq'][1:])
        assert o['rec_token'] == ' '.join(chars[t] for t in nb[0]['yseq'][1:])
        for k, h in enumerate(nb):
            assert e['rec_tokenid[%05d]' % k] == ' '.join(str(t) for t in h['yseq'][1:]), (utt, k)
            got = e['score[%05d]' % k]
            assert abs(got - h['score']) <= TOL * max(1.0, abs(h['score'])), (utt, k, got, h['score'])
            assert e['rec_text[%05d]' % k] == e['rec_token[%05d]' % k].replace(' ', '').replace('<space>', ' ')
        assert 'rec_tokenid[%05d]' % len(nb) not in e


@gpu
@pytest.mark.parametrize('batch', [3, 1])
def test_joint_recog_equals_the_module_api(fix, batch):
    """--recog-batch 3: batches of 3 and 2 with the items re-ordered by length (37, 33, 29 | 20, 20); --recog-batch 1: the reference's loop."""
    utts, _ = _cli(fix, 'joint', 'joint_b%d' % batch, ['--recog-batch', str(batch), '--no-score'])
    _check(utts, _api(fix, True))


@gpu
def test_asr_recog_equals_the_module_api_without_the_enhancer(fix):
    utts, _ = _cli(fix, 'asr', 'asr_b3', ['--recog-batch', '3', '--no-score'])
    _check(utts, _api(fix, False))
    joint = _api(fix, True)
    assert any(joint[u][0]['score'] != float(utts[u]['score[00000]']) for u in RF.UTTS), 'the enhancer made no difference: the two modes ran the same path'


@gpu
def test_joint_recog_with_rnnlm(fix, golden_dir):
    """--lmtype rnnlm --rnnlm FILE: the LM of recog_lm_tiny.npz (12 labels, 6 input and 10 hidden units: widths read from the file)."""
    from robust_e2e_gan_amd.model.lm import RNNLM, ClassifierWithState
    lm = ClassifierWithState(RNNLM(12, 6, 10))
    lm.load_state_dict(RF.sub(RF.golden(golden_dir, 'recog_lm_tiny.npz'), 'lm.'), strict=True)
    utts, _ = _cli(fix, 'joint', 'joint_lm', ['--recog-batch', '3', '--no-score', '--lmtype', 'rnnlm', '--rnnlm', fix['lm'], '--lm-weight', '0.3'])
    want = _api(fix, True, lm.to(DEV).eval(), 0.3)
    _check(utts, want)
    plain = _api(fix, True)
    assert any(want[u][0]['score'] != plain[u][0]['score'] for u in RF.UTTS), 'the LM made no difference'


@gpu
def test_scoring_and_no_score(fix):
    utts, out = _cli(fix, 'joint', 'joint_scored', ['--recog-batch', '3'])
    assert sorted(os.listdir(out)) == ['data.json', 'hyp.trn', 'ref.trn', 'result.txt', 'score.json']
    report = json.load(open(os.path.join(out, 'score.json'), encoding='utf-8'))
    assert report['costs'] == {'substitution': 4, 'insertion': 3, 'deletion': 3}
    ids = lambda s: [t for t in (int(v) for v in s.split()) if t not in (0, 11)]
    chars = ['<blank>'] + RF.SYMBOLS + ['<eos>']

    def words(labels):
        return [w for w in ''.join(chars[t] for t in labels).split('<space>') if w]

    for level, seq in (('token', lambda s: ids(s)), ('word', lambda s: words(ids(s)))):
        rep = report if level == 'token' else report['word']
        for utt in RF.UTTS:
            e = utts[utt]
            ref = seq(e['output'][0]['tokenid'])
            rows = [refs_align.align(ref, seq(e['rec_tokenid[%05d]' % k]), (4, 3, 3))[0] for k in range(4)]
            one, orc = rep['utts'][utt]['1best'], rep['utts'][utt]['oracle']
            assert [one[k] for k in ('cost', 'errors', 'C', 'S', 'D', 'I')] == rows[0], (level, utt)
            best = min(range(4), key=lambda k: (rows[k][1], k))
            assert orc['rank'] == best and [orc[k] for k in ('cost', 'errors', 'C', 'S', 'D', 'I')] == rows[best], (level, utt)
            assert rep['utts'][utt]['ntok'] == len(ref) and rep['utts'][utt]['spk'] == utt.split('-')[0]
        assert sorted(rep['speakers']) == ['spkA', 'spkB']
        for k in ('#snt', '#tok', 'C', 'S', 'D', 'I'):
            assert rep['overall'][k] == sum(s[k] for s in rep['speakers'].values())
            want = len(RF.UTTS) if k == '#snt' else sum(u['ntok'] if k == '#tok' else u['1best'][k] for u in rep['utts'].values())
            assert rep['overall'][k] == want
        o = rep['overall']
        assert o['C'] + o['S'] + o['D'] == o['#tok'] and abs(o['err'] - (o['S'] + o['D'] + o['I']) / o['#tok']) < 1e-12
        assert abs(o['oracle_err'] - sum(u['oracle']['errors'] for u in rep['utts'].values()) / o['#tok']) < 1e-12
    for name, key in (('ref.trn', 'tokenid'), ('hyp.trn', 'rec_tokenid')):
        lines = open(os.path.join(out, name), encoding='utf-8').read().splitlines()
        assert len(lines) == 5
        for line, utt in zip(lines, sorted(RF.UTTS)):
            toks = ' '.join(chars[t] for t in ids(utts[utt]['output'][0][key]))
            assert line == '%s (%s-%s)' % (toks, utt.split('-')[0], utt), line
    text = open(os.path.join(out, 'result.txt'), encoding='utf-8').read()
    assert 'substitution 4, insertion 3, deletion 3' in text and 'NIST' in text and 'Levenshtein' in text and 'Sum/Avg' in text
    _, bare = _cli(fix, 'joint', 'joint_bare', ['--recog-batch', '3', '--no-score'])
    assert os.listdir(bare) == ['data.json']
    _, other = _cli(fix, 'joint', 'joint_lev', ['--recog-batch', '3', '--score-costs', '1,1,1', '--score-dir', os.path.join(fix['root'], 'lev')])
    assert os.listdir(other) == ['data.json'] and 'substitution 1, insertion 1, deletion 1' in open(os.path.join(fix['root'], 'lev', 'result.txt')).read()
