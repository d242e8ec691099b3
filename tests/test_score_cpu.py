"""CPU side of the recognisers and the scorer: the restatement of the alignment (tests/refs_align.py) against its invariants and an independent
Levenshtein distance, TestOptions, the result JSON, trn lines and score.json arithmetic from canned counts, SequentialKaldiDataset, the CMVN
lookup order and the refusals.  Nothing here touches a device."""
import json
import os

import numpy as np
import pytest
import torch

import refs_align


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_invariants_on_random_pairs():
    """Seeded pairs over 3 symbols (many ties): the counts add up to both lengths, the path replays over both sequences with 'C' only on
    equal labels, and with unit costs the error count is the Levenshtein distance."""
    rng = np.random.default_rng(11)
    for case in range(1500):
        ref = rng.integers(1, 4, int(rng.integers(0, 13))).tolist()
        hyp = rng.integers(1, 4, int(rng.integers(0, 13))).tolist()
        for costs in ((4, 3, 3), (1, 1, 1), (2, 3, 1), (7, 3, 3)):
            (cost, err, C, S, D, I), path = refs_align.align(ref, hyp, costs)
            where = (ref, hyp, costs, path)
            assert C + S + D == len(ref) and C + S + I == len(hyp) and err == S + D + I, where
            assert cost == costs[0] * S + costs[1] * I + costs[2] * D, where
            assert [path.count(c) for c in 'CSDI'] == [C, S, D, I] and refs_align.replay(ref, hyp, path), where
            if costs == (1, 1, 1):
                assert err == refs_align.levenshtein(ref, hyp), where
            if costs == (7, 3, 3):
                assert S == 0, where


def test_restatement_on_the_pairs_of_the_issue():
    a, b = ([1, 1, 2, 2, 1], [3, 3, 3, 3, 3, 1, 2]), ([2, 3, 3, 1, 1, 1], [1, 1, 1, 3, 2, 3, 2])
    assert refs_align.align(*a, (4, 3, 3))[0] == [22, 6, 1, 4, 0, 2]          # the same cost is reached with 7 errors too: the second key decides
    assert refs_align.align(*b, (4, 3, 3))[0] == [21, 7, 3, 0, 3, 4]
    assert refs_align.align(*b, (1, 1, 1))[0][1:] == [6, 1, 5, 0, 1]          # the cost vector changes the reported error count
    assert refs_align.levenshtein(*b) == 6


# ---- options -----------------------------------------------------------------------------------------------------------------------------------------
def test_test_options_names_and_defaults(tmp_path):
    from robust_e2e_gan_amd.options.test_options import TestOptions
    opt = TestOptions().parse(['--checkpoints_dir', str(tmp_path), '--name', 'x'])
    want = dict(recog_dir=None, enhance_dir=None, enhance_out_dir=None, recog_label=None, recog_json=None, result_label=None, nj=1, nbest=1,
                beam_size=1, penalty=0.0, maxlenratio=0.0, minlenratio=0.0, ctc_weight=0.0, fstlm_path=None, nn_char_map_file=None,
                recog_batch=16, fbank_cmvn=None, score=True, score_costs='4,3,3', score_dir=None, fast_layers=2, fast_cell_size=650,
                slow_cell_size=650, zoneout_keep_h=0.9, zoneout_keep_c=0.5, lmtype=None, rnnlm=None, lm_weight=0.1, feat_type='kaldi_magspec')
    for k, v in want.items():
        assert getattr(opt, k) == v, (k, getattr(opt, k), v)
    assert opt.exp_path == os.path.join(str(tmp_path), 'x') and not os.path.exists(opt.exp_path), 'parse() wrote opt.txt without being asked'
    opt = TestOptions().parse(['--checkpoints_dir', str(tmp_path), '--name', 'x', '--no-score', '--beam-size', '12', '--ctc-weight', '0.3',
                               '--recog-batch', '4', '--result-label', 'r.json', '--nj', '8'], save=True)
    assert (opt.score, opt.beam_size, opt.ctc_weight, opt.recog_batch, opt.result_label, opt.nj) == (False, 12, 0.3, 4, 'r.json', 8)
    assert os.path.isfile(os.path.join(opt.exp_path, 'opt.txt'))


# ---- the result JSON -----------------------------------------------------------------------------------------------------------------------------
CHARS = ['<blank>', 'a', 'b', '<space>', 'c', '<eos>']


def test_result_json_against_a_hand_written_dict(tmp_path):
    from robust_e2e_gan_amd import recog
    nbest = [{'yseq': [5, 1, 3, 2, 5], 'score': -1.5}, {'yseq': [5, 1, 2, 5], 'score': -2.25}]
    got = recog.result_entry('spk-1', [1, 3, 4], nbest, CHARS, beam_size=4)
    assert got == {
        'utt2spk': 'spk-1',
        'output': [{'name': 'target1', 'text': 'a c', 'token': 'a <space> c', 'tokenid': '1 3 4', 'rec_tokenid': '1 3 2 5',
                    'rec_token': 'a <space> b <eos>', 'rec_text': 'a b<eos>'}],
        'rec_tokenid[00000]': '1 3 2 5', 'rec_token[00000]': 'a <space> b <eos>', 'rec_text[00000]': 'a b<eos>', 'score[00000]': -1.5,
        'rec_tokenid[00001]': '1 2 5', 'rec_token[00001]': 'a b <eos>', 'rec_text[00001]': 'ab<eos>', 'score[00001]': -2.25}
    for one in (recog.result_entry('s', [1], nbest, CHARS, beam_size=1), recog.result_entry('s', [1], nbest[:1], CHARS, beam_size=4)):
        assert sorted(one) == ['output', 'utt2spk'], 'n-best keys at beam 1, or for a single hypothesis'
    path = str(tmp_path / 'd' / 'data.json')
    recog.write_result(path, {'u1': got})
    raw = open(path, 'rb').read().decode('utf_8')
    assert json.loads(raw) == {'utts': {'u1': got}} and raw == json.dumps({'utts': {'u1': got}}, indent=4, sort_keys=True)


# ---- trn lines and the arithmetic of score.json --------------------------------------------------------------------------------------------------
def test_trn_lines_labels_and_words():
    from robust_e2e_gan_amd.utils import score
    assert score.trn_line(['a', '<space>', 'b'], 'spk-1-x', 'spk-1-x-utt7') == 'a <space> b (spk_1_x-spk-1-x-utt7)\n'
    assert score.labels_of([5, 1, 0, 3, 2, 5, 5], len(CHARS)) == [1, 3, 2]
    assert score.words_of([3, 1, 2, 3, 3, 4, 3], CHARS) == ['ab', 'c'] and score.words_of([], CHARS) == []
    entry = {'output': [{'rec_tokenid': '1 2'}], 'rec_tokenid[00000]': '1 2', 'rec_tokenid[00001]': '2'}
    assert score.nbest_ids(entry) == [[1, 2], [2]] and score.nbest_ids({'output': [{'rec_tokenid': '4 5'}]}) == [[4, 5]]
    assert score.parse_costs('2,3,1') == (2, 3, 1)
    for bad in ('4,3', '0,3,3', '4,3,256', 'a,b,c'):
        with pytest.raises(Exception):
            score.parse_costs(bad)
    assert score.aligned_lines(['a', 'bb', 'c'], ['a', 'x', 'c', 'd'], 'CSCI') == ('REF: a bb c *', 'HYP: a x  c d', 'OP:    S    I')


def test_score_json_arithmetic_from_canned_counts():
    from robust_e2e_gan_amd.utils import score
    c = lambda cost, err, C, S, D, I: dict(cost=cost, errors=err, C=C, S=S, D=D, I=I)
    per_utt = {'u1': {'spk': 'A', 'ntok': 5, '1best': c(7, 2, 4, 1, 0, 1), 'oracle': c(3, 1, 5, 0, 0, 1)},
               'u2': {'spk': 'A', 'ntok': 3, '1best': c(0, 0, 3, 0, 0, 0), 'oracle': c(0, 0, 3, 0, 0, 0)},
               'u3': {'spk': 'B', 'ntok': 2, '1best': c(6, 2, 0, 0, 2, 0), 'oracle': c(6, 2, 0, 0, 2, 0)}}
    spk, tot = score.summarise(per_utt)
    assert spk['A'] == {'#snt': 2, '#tok': 8, 'C': 7, 'S': 1, 'D': 0, 'I': 1, 'err': 2 / 8, 'serr': 1 / 2, 'oracle_err': 1 / 8}
    assert spk['B'] == {'#snt': 1, '#tok': 2, 'C': 0, 'S': 0, 'D': 2, 'I': 0, 'err': 1.0, 'serr': 1.0, 'oracle_err': 1.0}
    assert tot == {'#snt': 3, '#tok': 10, 'C': 7, 'S': 1, 'D': 2, 'I': 1, 'err': 4 / 10, 'serr': 2 / 3, 'oracle_err': 3 / 10}
    text = score.format_result('token', (4, 3, 3), spk, tot, [('u1', per_utt['u1']['1best'], ('REF: a', 'HYP: b', 'OP:  S'))])
    assert 'substitution 4, insertion 3, deletion 3 (the NIST weights)' in text and 'Levenshtein' in text and 'not claimed' in text
    rows = [l for l in text.splitlines() if l.startswith(('A ', 'B ', 'Sum/Avg'))]
    assert len(rows) == 3 and rows[2].split()[1:] == ['3', '10', '70.0', '10.0', '20.0', '10.0', '40.0', '66.7', '30.0']
    with pytest.raises(Exception):          # the aligner itself has no CPU path
        score.align([[1]], [[1]], [0], device='cpu')


# ---- the data set ----------------------------------------------------------------------------------------------------------------------------------
def _data_dir(tmp_path, utts=('s1-a', 's2-b__n1', 's1-c'), rows=(7, 4, 9)):
    from robust_e2e_gan_amd.data import kaldi_io
    d = str(tmp_path / 'data')
    os.makedirs(d)
    rng = np.random.default_rng(3)
    mats = [(rng.random((T, 6)) + 0.1).astype(np.float32) for T in rows]
    w = kaldi_io.ArkScpWriter(os.path.join(d, 'feats.ark'), False)
    for u, m in zip(utts, mats):
        w.add(u, m)
    w.close(os.path.join(d, 'feats.scp'))
    with open(os.path.join(d, 'utt2spk'), 'w') as f:
        f.write('s1-a s1\ns2-b s2\ns1-c s1\n')
    with open(os.path.join(d, 'text_char'), 'w') as f:
        f.write('s1-a ab\ns2-b bxa\ns1-c b\n')
    with open(os.path.join(d, 'units.txt'), 'w') as f:
        f.write('a 1\nb 2\n')
    return d, mats


def test_sequential_kaldi_dataset(tmp_path):
    import argparse
    from robust_e2e_gan_amd.data.kaldi_dataset import SequentialKaldiDataset
    d, mats = _data_dir(tmp_path)
    args = argparse.Namespace(feat_type='kaldi_magspec', model_unit='char', normalize_type=1, num_utt_cmvn=100, exp_path=str(tmp_path / 'exp'))
    ds = SequentialKaldiDataset(args, d, os.path.join(d, 'units.txt'))
    assert open(os.path.join(d, 'kaldi_feat_len.scp')).read() == 's1-a 7\ns2-b__n1 4\ns1-c 9\n'
    assert len(ds) == 3 and ds.lengths == [7, 4, 9] and ds.feat_size == 6 and ds.char_list == ['<blank>', 'a', 'b', '<eos>']
    assert os.path.isfile(os.path.join(args.exp_path, 'cmvn.npy')) and ds.cmvn.shape == (2, 6)
    utt, spk, x, x_log, y = ds[1]                                  # speaker and transcript of the part before '__'; 'x' is out of vocabulary
    assert (utt, spk, y.tolist()) == ('s2-b__n1', 's2', [2, 1, 1])
    assert torch.equal(x, torch.from_numpy(mats[1]))
    want = (10 * np.log10(mats[1]) + ds.cmvn[0]) * ds.cmvn[1]
    assert np.allclose(x_log.numpy(), want, rtol=1e-6, atol=1e-6)
    raw = SequentialKaldiDataset(args, d, os.path.join(d, 'units.txt'), raw=True)[2]
    assert raw[:2] == ('s1-c', 's1') and (raw[2].rows, raw[2].cols) == (9, 6) and raw[3] == [2]
    assert np.array_equal(raw[2].decode(), mats[2])
    with open(os.path.join(d, 'feats.scp'), 'a') as f:              # an utterance neither table knows, under either id
        f.write('s9-z__n2 %s\n' % open(os.path.join(d, 'feats.scp')).readline().split()[1])
    os.remove(os.path.join(d, 'kaldi_feat_len.scp'))
    ds = SequentialKaldiDataset(args, d, os.path.join(d, 'units.txt'))
    with pytest.raises(KeyError, match='s9-z__n2.*speaker'):
        ds[3]
    with pytest.raises(ValueError, match='kaldi_magspec / kaldi_fbank'):
        SequentialKaldiDataset(argparse.Namespace(feat_type='fbank'), d, os.path.join(d, 'units.txt'))


# ---- CMVN lookup and refusals --------------------------------------------------------------------------------------------------------------------
def _opt(tmp_path, extra=()):
    from robust_e2e_gan_amd.options.test_options import TestOptions
    return TestOptions().parse(['--checkpoints_dir', str(tmp_path), '--name', 'exp', '--result-label', str(tmp_path / 'r.json')] + list(extra))


def test_fbank_cmvn_lookup_order(tmp_path):
    from robust_e2e_gan_amd import recog
    opt = _opt(tmp_path)
    os.makedirs(opt.exp_path)
    with pytest.raises(FileNotFoundError) as e:
        recog.find_fbank_cmvn(opt)
    assert all(w in str(e.value) for w in ('--fbank_cmvn', 'fbank_cmvn.npy', 'enhance_cmvn.npy'))
    enh, fb, own = os.path.join(opt.exp_path, 'enhance_cmvn.npy'), os.path.join(opt.exp_path, 'fbank_cmvn.npy'), str(tmp_path / 'mine.npy')
    np.save(enh, np.zeros((2, 80), np.float32))
    assert recog.find_fbank_cmvn(opt) == enh
    np.save(fb, np.zeros((2, 80), np.float32))
    assert recog.find_fbank_cmvn(opt) == fb
    np.save(own, np.zeros((2, 80), np.float32))
    assert recog.find_fbank_cmvn(_opt(tmp_path, ['--fbank_cmvn', own])) == own
    with pytest.raises(FileNotFoundError):
        recog.find_fbank_cmvn(_opt(tmp_path, ['--fbank_cmvn', own + '.missing']))


def test_refusals(tmp_path):
    from robust_e2e_gan_amd import recog
    from robust_e2e_gan_amd.lib import Re2eError
    with pytest.raises(Re2eError, match='FST LMs'):
        recog.run(_opt(tmp_path, ['--lmtype', 'fstlm', '--fstlm-path', 'lm.fst']), 'joint')
    with pytest.raises(Re2eError, match='no CPU path'):
        recog.run(_opt(tmp_path, ['--gpu_ids', '-1']), 'asr')
    with pytest.raises(FileNotFoundError, match='no checkpoint found'):
        recog.run(_opt(tmp_path, ['--works_dir', str(tmp_path), '--resume', 'missing.pth']), 'joint')
    with pytest.raises(FileNotFoundError, match='no checkpoint found'):
        recog.run(_opt(tmp_path), 'joint')
    with pytest.raises(Re2eError, match='joint or asr'):
        recog.run(_opt(tmp_path), 'enhance')
