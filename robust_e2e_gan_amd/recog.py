"""Recognise and score a data set (mirror of the reference's joint_recog.py / asr_recog.py; the entry points are
``python -m robust_e2e_gan_amd.joint_recog`` and ``python -m robust_e2e_gan_amd.asr_recog``, both thin wrappers over ``run(opt, mode)``).

    python -m robust_e2e_gan_amd.joint_recog --recog-dir DATA --dict_dir DICT --resume CKPT --checkpoints_dir EXP --name NAME \\
        --result-label EXP/NAME/decode/data.json --beam-size 12 --nbest 12 --ctc-weight 0.3 [--lmtype rnnlm --rnnlm LM --lm-weight 0.2]

``joint`` loads EnhanceModel / FbankModel / E2E from the checkpoint's ``enhance_state_dict`` / ``fbank_state_dict`` / ``asr_state_dict``
(joint_recog.py:60-70), ``asr`` the last two (asr_recog.py:57-67).  The items of ``SequentialKaldiDataset(--recog-dir)`` are sorted by frame
count, longest first, and taken ``--recog-batch`` at a time: the records are decoded, clamped, logged, normalised and padded on the device
(re2e_kaldi_decode_pad), go through the enhancer's inference forward (``joint``) and FbankModel -- for ``kaldi_fbank`` features
``(x + cmvn[0]) * cmvn[1]`` instead (asr_recog.py:144-145) -- and are searched together by ``E2E.recognize_batch``; ``--recog-batch 1`` is the
reference's loop, one ``recognize`` per utterance.  Only the n-best lists come back to the host.  ``--result-label`` gets the reference's JSON
(joint_recog.py:142-195); unless ``--no-score`` is given the result is then aligned and scored on the device (utils/score.py).

The filterbank CMVN is ``--fbank_cmvn`` if given, else ``exp_path/fbank_cmvn.npy`` (what the reference reads), else
``exp_path/enhance_cmvn.npy`` (what joint_train writes).  LM widths are read from the LM checkpoint's tensor shapes (the reference hard-codes
650 / 300, which does not fit the recipe's own LMs).  ``--lmtype ngram --kenlm FILE`` (alias ``--ngram-lm``) decodes with an ARPA back-off
model (model/ngram.py; ``--ngram-tokens symbols|ids`` says what the file's tokens are; the tables are cached beside the file as FILE.npz).
``--nj`` is accepted and ignored; FST LMs (--lmtype fstlm --fstlm-path) and binary KenLM files are refused."""
import json
import os

import numpy as np
import torch

from .lib import Re2eError

MODES = ('joint', 'asr')


# ---- what is needed beside the models ---------------------------------------------------------------------------------------------------------------
def find_fbank_cmvn(opt):
    """The CMVN file of the filterbank features, by the order in the module docstring; an error that names all three otherwise."""
    given = getattr(opt, 'fbank_cmvn', None)
    if given:
        if not os.path.isfile(given):
            raise FileNotFoundError('--fbank_cmvn %s does not exist' % given)
        return given
    tried = [os.path.join(opt.exp_path, 'fbank_cmvn.npy'), os.path.join(opt.exp_path, 'enhance_cmvn.npy')]
    for p in tried:
        if os.path.isfile(p):
            return p
    raise FileNotFoundError('no filterbank CMVN: --fbank_cmvn was not given and neither %s nor %s exists' % (tried[0], tried[1]))


def load_labeldict(dict_file):
    """Word dictionary of the word-level LMs: ``word id`` per line; '<blank>' 0 and '<unk>' 1 as in the reference's recognisers."""
    labeldict = {'<blank>': 0}
    with open(dict_file, 'r', encoding='utf-8') as f:
        for line in f:
            if line.strip():
                word, idx = line.split()
                labeldict[word] = int(idx)
    if '<eos>' not in labeldict:
        labeldict['<eos>'] = len(labeldict)
    return labeldict


def _state_dict(path):
    if not path or not os.path.isfile(path):
        raise FileNotFoundError('no language model found at %s' % path)
    return torch.load(path, map_location='cpu')


def _rnnlm_of(sd, what):
    """ClassifierWithState(RNNLM) of the widths the state dict itself has."""
    from .model.lm import RNNLM, ClassifierWithState
    try:
        V, I = sd['predictor.embed.weight'].shape
        H = sd['predictor.l1.weight_hh'].shape[1]
    except KeyError as e:
        raise Re2eError('%s is not an RNNLM state dict (no %s)' % (what, e))
    m = ClassifierWithState(RNNLM(int(V), int(I), int(H)))
    m.load_state_dict(sd)
    return m


def build_lm(opt, char_list, device):
    """The decode-time LM by --lmtype (joint_recog.py:75-132), on ``device`` in evaluation mode, or None."""
    from .model.lm import ClassifierWithState
    if opt.lmtype == 'fstlm':
        if getattr(opt, 'fstlm_path', None):
            raise Re2eError('decode-time LM: only RNNLM shallow fusion (rnnlm=ClassifierWithState(RNNLM(...))) is supported; '
                            'n-gram / FST LMs (fstlm) are out of scope')
        return None
    lm = None
    if opt.lmtype == 'rnnlm':
        if opt.rnnlm:
            lm = _rnnlm_of(_state_dict(opt.rnnlm), opt.rnnlm)
            if lm.predictor.n_vocab != len(char_list):
                raise Re2eError('%s has %d labels, the dictionary %d' % (opt.rnnlm, lm.predictor.n_vocab, len(char_list)))
        if opt.word_rnnlm:
            from .model.extlm import LookAheadWordLM, MultiLevelLM
            if not opt.word_dict:
                raise Re2eError('word dictionary file is not specified for the word RNNLM (--word-dict)')
            word_dict = load_labeldict(opt.word_dict)
            char_dict = {x: i for i, x in enumerate(char_list)}
            word = _rnnlm_of(_state_dict(opt.word_rnnlm), opt.word_rnnlm)
            lm = ClassifierWithState(MultiLevelLM(word.predictor, lm.predictor, word_dict, char_dict) if lm is not None
                                     else LookAheadWordLM(word.predictor, word_dict, char_dict))
    elif opt.lmtype == 'ngram':
        from .model.ngram import NgramLM, load_tables
        path = opt.kenlm                                    # --kenlm or its alias --ngram-lm
        if not path:
            raise Re2eError('--lmtype ngram needs the ARPA file: --kenlm PATH (the reference\'s flag) or --ngram-lm PATH')
        lm = ClassifierWithState(NgramLM(load_tables(path, char_list, getattr(opt, 'ngram_tokens', 'symbols'))))
    elif opt.lmtype == 'fsrnnlm' and opt.rnnlm:
        from .model.fsrnn import FSRNNLM
        sd = _state_dict(opt.rnnlm)
        try:
            V, E = sd['predictor.embed.weight'].shape
            Fs, Ss = sd['predictor.fast_cells.0.weight_hh'].shape[1], sd['predictor.slow_cell.weight_hh'].shape[1]
        except KeyError as e:
            raise Re2eError('%s is not an FS-RNN LM state dict (no %s)' % (opt.rnnlm, e))
        lm = ClassifierWithState(FSRNNLM(int(V), int(E), opt.fast_layers, int(Fs), int(Ss), opt.zoneout_keep_h, opt.zoneout_keep_c))
        lm.load_state_dict(sd)
    return lm.to(device).eval() if lm is not None else None


def load_models(opt, mode, device):
    """(enhancer or None, FbankModel, E2E) of the checkpoint at works_dir/resume, on ``device`` in evaluation mode."""
    from .model.e2e_model import E2E
    from .model.enhance_model import EnhanceModel
    from .model.feat_model import FbankModel
    path = os.path.join(opt.works_dir, opt.resume) if opt.resume else None
    if not path or not os.path.isfile(path):
        raise FileNotFoundError('no checkpoint found at %s' % (path or '(--resume was not given)'))
    enh = EnhanceModel.load_model(path, 'enhance_state_dict') if mode == 'joint' else None
    fb = FbankModel.load_model(path, 'fbank_state_dict')
    asr = E2E.load_model(path, 'asr_state_dict')
    return tuple(m.to(device).eval() if m is not None else None for m in (enh, fb, asr))


# ---- the result JSON (joint_recog.py:142-195) ------------------------------------------------------------------------------------------------------
def result_entry(spk, y_true, nbest_hyps, char_list, beam_size):
    """One utterance of the reference's JSON: the 1-best under 'output', and the n-best keys when the beam is wider than 1 and more than
    one hypothesis came back."""
    text = lambda toks: ''.join(toks).replace('<space>', ' ')
    y_hat = nbest_hyps[0]['yseq'][1:]
    seq_hat, seq_true = [char_list[int(i)] for i in y_hat], [char_list[int(i)] for i in y_true]
    entry = {'utt2spk': spk,
             'output': [{'name': 'target1', 'text': text(seq_true), 'token': ' '.join(seq_true), 'tokenid': ' '.join(str(int(i)) for i in y_true),
                         'rec_tokenid': ' '.join(str(int(i)) for i in y_hat), 'rec_token': ' '.join(seq_hat), 'rec_text': text(seq_hat)}]}
    if beam_size > 1 and len(nbest_hyps) > 1:
        for k, hyp in enumerate(nbest_hyps):
            y = hyp['yseq'][1:]
            toks = [char_list[int(i)] for i in y]
            entry['rec_tokenid[%05d]' % k] = ' '.join(str(int(i)) for i in y)
            entry['rec_token[%05d]' % k] = ' '.join(toks)
            entry['rec_text[%05d]' % k] = text(toks)
            entry['score[%05d]' % k] = float(hyp['score'])
    return entry


def write_result(path, utts):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:
        f.write(json.dumps({'utts': utts}, indent=4, sort_keys=True).encode('utf_8'))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------
def run(opt, mode):
    """Recognise ``opt.recog_dir`` with the models of ``opt.resume``; writes ``opt.result_label`` (and the scores) and returns the 'utts'
    dictionary."""
    from .data.kaldi_dataset import SequentialKaldiDataset
    from .data.mix_data_loader import decode_pad_device
    if mode not in MODES:
        raise Re2eError('mode is joint or asr, not %r' % (mode,))
    if opt.lmtype == 'fstlm' and getattr(opt, 'fstlm_path', None):
        build_lm(opt, [], None)                   # raises
    if not opt.gpu_ids:
        raise Re2eError('the recognisers run on the GPU (--gpu_ids is empty): there is no CPU path')
    if opt.recog_batch < 1:
        raise Re2eError('--recog-batch must be at least 1')
    if not opt.result_label:
        raise Re2eError('--result-label is needed: the result JSON to write')
    device = torch.device('cuda:%d' % opt.gpu_ids[0])
    costs = None
    if opt.score:
        from .utils import score as scorer
        costs = scorer.parse_costs(opt.score_costs)
    enh, fb, asr = load_models(opt, mode, device)
    dict_file = opt.dict_dir if os.path.isfile(opt.dict_dir) else os.path.join(opt.dict_dir, 'train_units.txt')
    ds = SequentialKaldiDataset(opt, opt.recog_dir, dict_file, raw=True)
    char_list = ds.char_list
    if asr.eos + 1 != len(char_list):
        raise Re2eError('the checkpoint decodes %d labels, the dictionary %s has %d' % (asr.eos + 1, dict_file, len(char_list)))
    opt.idim, opt.odim, opt.char_list = ds.feat_size, ds.num_classes, char_list
    lm = build_lm(opt, char_list, device)
    fbank_cmvn = torch.from_numpy(np.load(find_fbank_cmvn(opt)).astype(np.float32)).to(device)
    cmvn = torch.from_numpy(np.asarray(ds.cmvn, np.float32)) if ds.cmvn is not None else None
    order = sorted(range(len(ds)), key=lambda i: -ds.lengths[i])          # stable: equal lengths keep the table's order
    utts = {}
    with torch.no_grad(), torch.cuda.device(device):
        for at in range(0, len(order), opt.recog_batch):
            items = [ds[i] for i in order[at:at + opt.recog_batch]]
            lens = [it[2].rows for it in items]
            x, x_log = decode_pad_device([it[2] for it in items], device, None, cmvn, want_log=True)
            if enh is not None:
                x = enh(x, x_log, torch.IntTensor(lens))
            feats = (x + fbank_cmvn[0, :]) * fbank_cmvn[1, :] if ds.feat_type == 'kaldi_fbank' else fb(x, fbank_cmvn)
            if opt.recog_batch == 1:
                nbests = [asr.recognize(feats, opt, char_list, rnnlm=lm)]
            else:
                nbests = asr.recognize_batch(feats, lens, opt, char_list, rnnlm=lm)
            for (utt, spk, _, target), nbest in zip(items, nbests):
                utts[utt] = result_entry(spk, target, nbest, char_list, opt.beam_size)
            if opt.verbose > 0:
                print('%d / %d utterances' % (min(at + opt.recog_batch, len(order)), len(order)))
    write_result(opt.result_label, utts)
    if opt.score:
        out_dir = opt.score_dir or os.path.dirname(os.path.abspath(opt.result_label))
        report = scorer.score(utts, char_list, out_dir, costs, device)
        o = report['overall']
        print('%d utterances, %d tokens: error rate %.2f %% (C %d S %d D %d I %d), sentence error rate %.2f %%, oracle %.2f %%   [%s]' % (
            o['#snt'], o['#tok'], 100 * o['err'], o['C'], o['S'], o['D'], o['I'], 100 * o['serr'], 100 * o['oracle_err'],
            os.path.join(out_dir, 'result.txt')))
    return utts


def main(mode, argv=None):
    from .options.test_options import TestOptions
    return run(TestOptions().parse(argv), mode)
