"""Re-rank the n-best lists of a result JSON with an ARPA n-gram LM (mirror of the reference's utils/kenlm_rescore.py, without kenlm):

    python -m robust_e2e_gan_amd.utils.ngram_rescore IN.json LM.arpa RESCORE_WEIGHT OUT.json --dict DICT [--ngram-tokens symbols|ids]

Every ``rec_tokenid[k]`` of every utterance of the file is scored by ``re2e_ngram_score_seqs`` (csrc/ngram.hip) in ONE launch: the sequence
without its final <eos> label, from the context [eos] (``<s>``), with the end of the sentence (``</s>``) appended -- what ``kenlm.Model.score``
adds up for a sentence.  ``kenlm_score[k]`` is that sum per token in log10, the unit upstream writes (the search itself works in natural
logarithms: model/ngram.py); upstream divides by the length of the token STRING, spaces included, which is not a per-token mean: here the
divisor is the number of tokens.  The 1-best under 'output' becomes the hypothesis with the largest ``rescore_weight * kenlm_score + score``
(the first one on a tie, as ``list.index(max(..))`` upstream); utterances without an n-best list are copied unchanged."""
import argparse
import json
import math

import torch

from ..lib import Re2eError

LN10 = math.log(10.0)


def _nbest_keys(entry):
    ks = []
    while 'rec_tokenid[%05d]' % len(ks) in entry and 'score[%05d]' % len(ks) in entry:
        ks.append(len(ks))
    return ks


def rescore(utts, tables, rescore_weight, device='cuda:0'):
    """``utts`` (the 'utts' dictionary of a result JSON) with ``kenlm_score[k]`` added and the 1-best re-ranked, in place; returns it."""
    if not torch.cuda.is_available():
        raise Re2eError('the n-gram scorer runs on the GPU: there is no CPU path')
    jobs, seqs = [], []
    for utt in sorted(utts):
        for k in _nbest_keys(utts[utt]):
            ids = [int(t) for t in utts[utt]['rec_tokenid[%05d]' % k].split()]
            while ids and ids[-1] == tables.eos:
                ids.pop()
            jobs.append((utt, k, max(1, len(ids))))
            seqs.append(ids)
    totals = tables.score_seqs(seqs, torch.device(device), append_eos=True) if seqs else []
    best = {}
    for (utt, k, ntok), total in zip(jobs, totals):
        e = utts[utt]
        lm = float(total) / LN10 / ntok
        e['kenlm_score[%05d]' % k] = lm
        new = float(rescore_weight) * lm + float(e['score[%05d]' % k])
        if utt not in best or new > best[utt][0]:
            best[utt] = (new, k)
    for utt, (_, k) in best.items():
        o = utts[utt]['output'][0]
        for key in ('rec_text', 'rec_token', 'rec_tokenid'):
            if '%s[%05d]' % (key, k) in utts[utt]:
                o[key] = utts[utt]['%s[%05d]' % (key, k)]
    return utts


def main(argv=None):
    from ..data.kaldi_dataset import read_dictionary
    from ..model.ngram import load_tables
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('in_json')
    p.add_argument('lm_path')
    p.add_argument('rescore_weight', type=float)
    p.add_argument('out_json')
    p.add_argument('--dict', required=True, help='the dictionary the result was decoded with (train_units.txt)')
    p.add_argument('--ngram-tokens', default='symbols', choices=['symbols', 'ids'])
    p.add_argument('--device', default='cuda:0')
    a = p.parse_args(argv)
    tables = load_tables(a.lm_path, read_dictionary(a.dict), a.ngram_tokens)
    print('%d-gram model, %d nodes, %d successor entries' % (tables.order, tables.n_nodes, tables.n_succ))
    with open(a.in_json, 'r', encoding='utf-8') as f:
        utts = json.load(f)['utts']
    rescore(utts, tables, a.rescore_weight, a.device)
    with open(a.out_json, 'w', encoding='utf-8') as f:
        f.write(json.dumps({'utts': utts}, indent=4, sort_keys=True, ensure_ascii=False))
    return utts


if __name__ == '__main__':
    main()
