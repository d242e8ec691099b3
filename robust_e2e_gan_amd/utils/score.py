"""Error rates of a recognition result (what the reference gets from ``utils/json2trn.py`` piped into an external scorer binary), with the
alignment on the device: every n-best hypothesis of every utterance of the set goes through ONE call of re2e_align_counts (csrc/align.hip).

    score(utts, char_list, out_dir)         utts = the 'utts' dictionary of the recognisers' result JSON (or of a file: ``load_utts``)

writes, under ``out_dir``,

    ref.trn  hyp.trn   ``tokens (spk-utt)`` lines in json2trn's format ('-' -> '_' in the speaker), so that any external scorer still runs
    score.json         per utterance the 1-best counts and the oracle (fewest errors over the n-best, first on ties); per speaker and overall
                       #snt, #tok, C / S / D / I, error rate (S+D+I) / #tok, sentence error rate, oracle error rate; the cost vector; and,
                       when '<space>' is in the dictionary, the same at word level under 'word'
    result.txt         a fixed-width table (one line per speaker, then Sum/Avg) and the aligned 1-best of every utterance with errors

Labels are token ids with <blank> (0) and <eos> (the last id) dropped.  The alignment is the one include/re2e.h defines: minimal weighted cost,
then fewest errors, then diagonal before deletion before insertion.  The default costs are the NIST weights substitution 4, insertion 3,
deletion 3; ``1,1,1`` gives the Levenshtein distance.  Where several alignments tie, another scorer may break the tie differently and report
other C / S / D / I counts: equality with any particular external scorer is not claimed, and none is run here or in the tests."""
import json
import os

import numpy as np
import torch

from .. import lib

DEFAULT_COSTS = (4, 3, 3)          # substitution, insertion, deletion
MAX_LEN = 1024                     # labels per sequence (re2e_align_counts)
COUNT_KEYS = ('cost', 'errors', 'C', 'S', 'D', 'I')
SPACE = '<space>'


def parse_costs(text):
    """'S,I,D' -> (S, I, D), integers in 1 .. 255."""
    try:
        c = tuple(int(v) for v in str(text).split(','))
    except ValueError:
        c = ()
    if len(c) != 3 or not all(1 <= v <= 255 for v in c):
        raise lib.Re2eError('--score-costs takes three integers S,I,D in 1 .. 255, not %r' % (text,))
    return c


# ---- the device call -----------------------------------------------------------------------------------------------------------------------------
def flat_table(seqs):
    """List of label lists -> (flat int32 array, int32 offsets of len + 1)."""
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise lib.Re2eError('more than 2^31 labels in one alignment call')
    flat = np.fromiter((int(t) for s in seqs for t in s), np.int32, count=int(off[-1]))
    return flat, off.astype(np.int32)


def align_counts(ref_labels, ref_off, hyp_labels, hyp_off, pair_ref, costs, counts, path=None, path_off=None):
    """re2e_align_counts on tables the caller built: ``ref_labels`` / ``hyp_labels`` int32 device tensors, ``ref_off`` / ``hyp_off`` /
    ``pair_ref`` int32 and ``path_off`` int64 numpy arrays (host), ``counts`` (n_pairs, 6) int32 and ``path`` uint8 device tensors, written in
    place.  Raises Re2eError with the library's message when a table fails its checks (nothing is launched then)."""
    ref_off, hyp_off, pair_ref = (np.ascontiguousarray(a, np.int32) for a in (ref_off, hyp_off, pair_ref))
    n_ref, n_pairs = len(ref_off) - 1, len(pair_ref)
    if len(hyp_off) != n_pairs + 1:
        raise lib.Re2eError('align_counts: %d pairs but %d hypothesis offsets' % (n_pairs, len(hyp_off)))
    if counts.dtype != torch.int32 or counts.numel() != 6 * n_pairs or ref_labels.dtype != torch.int32 or hyp_labels.dtype != torch.int32:
        raise lib.Re2eError('align_counts: counts is (n_pairs, 6) int32 and the labels are int32')
    if path is not None:
        path_off = np.ascontiguousarray(path_off, np.int64)
        if len(path_off) != n_pairs + 1 or path.dtype != torch.uint8:
            raise lib.Re2eError('align_counts: path is uint8 with n_pairs + 1 int64 offsets')
    need = lib.query('re2e_align_counts_workspace_bytes', ref_off.ctypes.data, n_ref, hyp_off.ctypes.data, pair_ref.ctypes.data, n_pairs,
                     int(path is not None))
    ws = lib.workspace(need, counts.device, 'align')
    lib.call('re2e_align_counts', lib.ptr(ref_labels) if ref_labels.numel() else None, ref_off.ctypes.data, n_ref, ref_labels.numel(),
             lib.ptr(hyp_labels) if hyp_labels.numel() else None, hyp_off.ctypes.data, pair_ref.ctypes.data, n_pairs, hyp_labels.numel(),
             int(costs[0]), int(costs[1]), int(costs[2]), lib.ptr(counts), lib.ptr(path) if path is not None else None,
             path_off.ctypes.data if path is not None else None, path.numel() if path is not None else 0, ws.data_ptr(), ws.numel() * 4)


def align(refs, hyps, pair_ref, costs=DEFAULT_COSTS, paths=False, device='cuda'):
    """Align hypothesis n (a list of ints) with reference ``pair_ref[n]`` in one launch -> (counts (n_pairs, 6) numpy: cost, errors, C, S, D,
    I; the paths as a list of str over 'CSDI', or None)."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise lib.Re2eError('the aligner runs on the GPU (device %s): there is no CPU path' % device)
    n = len(hyps)
    if n == 0:
        return np.zeros((0, 6), np.int32), ([] if paths else None)
    ref_flat, ref_off = flat_table(refs)
    hyp_flat, hyp_off = flat_table(hyps)
    pair_ref = np.asarray(pair_ref, np.int32)
    counts = torch.empty(n, 6, dtype=torch.int32, device=device)
    path = path_off = None
    if paths:
        cap = np.array([len(refs[r]) + len(h) if 0 <= r < len(refs) else 0 for r, h in zip(pair_ref.tolist(), hyps)], np.int64)
        path_off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
        path = torch.empty(max(int(path_off[-1]), 1), dtype=torch.uint8, device=device)
    align_counts(torch.from_numpy(ref_flat).to(device), ref_off, torch.from_numpy(hyp_flat).to(device), hyp_off, pair_ref, costs, counts, path,
                 path_off)
    got = counts.cpu().numpy()
    if not paths:
        return got, None
    raw = path.cpu().numpy().tobytes()
    return got, [raw[int(path_off[k]):int(path_off[k]) + int(got[k, 2:].sum())].decode('ascii') for k in range(n)]


# ---- from the result JSON to tables ------------------------------------------------------------------------------------------------------------
def load_utts(result_json):
    with open(result_json, 'rb') as f:
        return json.loads(f.read().decode('utf_8'))['utts']


def _ids(text):
    return [int(t) for t in text.split()]


def nbest_ids(entry):
    """The hypotheses of one utterance of the result JSON, best first: the n-best keys when they are there, else the 1-best."""
    out, k = [], 0
    while 'rec_tokenid[%05d]' % k in entry:
        out.append(_ids(entry['rec_tokenid[%05d]' % k]))
        k += 1
    return out or [_ids(entry['output'][0]['rec_tokenid'])]


def labels_of(ids, odim):
    """Token ids without <blank> (0) and <eos> (odim - 1)."""
    return [t for t in ids if t != 0 and t != odim - 1]


def words_of(labels, char_list):
    """The runs of labels between <space>, as strings."""
    words, cur = [], []
    for t in labels:
        if char_list[t] == SPACE:
            if cur:
                words.append(''.join(cur))
            cur = []
        else:
            cur.append(char_list[t])
    if cur:
        words.append(''.join(cur))
    return words


def trn_line(tokens, spk, utt):
    """json2trn's line: the tokens, then ``(speaker-utterance)`` with '-' -> '_' in the speaker."""
    return ' '.join(tokens) + ' (' + spk.replace('-', '_') + '-' + utt + ')\n'


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------------------
def _counts_dict(row):
    return {k: int(v) for k, v in zip(COUNT_KEYS, row)}


def summarise(per_utt):
    """per_utt: utt -> {'spk', 'ntok', '1best': counts, 'oracle': counts} -> (per speaker, overall): #snt, #tok, C, S, D, I, err, serr,
    oracle_err.  Rates are fractions; a speaker without reference tokens has err = oracle_err = 0."""
    def total(items):
        t = {'#snt': len(items), '#tok': sum(u['ntok'] for u in items)}
        for k in 'CSDI':
            t[k] = sum(u['1best'][k] for u in items)
        tok = max(t['#tok'], 1)
        t['err'] = (t['S'] + t['D'] + t['I']) / tok
        t['serr'] = sum(1 for u in items if u['1best']['errors'] > 0) / max(len(items), 1)
        t['oracle_err'] = sum(u['oracle']['errors'] for u in items) / tok
        return t
    spks = sorted({u['spk'] for u in per_utt.values()})
    return {s: total([u for u in per_utt.values() if u['spk'] == s]) for s in spks}, total(list(per_utt.values()))


def aligned_lines(ref_tokens, hyp_tokens, path):
    """Three lines (REF / HYP / OP) with the tokens of an alignment in columns; '*' fills a gap."""
    i = j = 0
    cols = []
    for op in path:
        r = ref_tokens[i] if op != 'I' else '*'
        h = hyp_tokens[j] if op != 'D' else '*'
        i += op != 'I'
        j += op != 'D'
        cols.append((r, h, op))
    w = [max(len(r), len(h), 1) for r, h, _ in cols]
    return ('REF: ' + ' '.join(r.ljust(n) for (r, _, _), n in zip(cols, w)).rstrip(),
            'HYP: ' + ' '.join(h.ljust(n) for (_, h, _), n in zip(cols, w)).rstrip(),
            'OP:  ' + ' '.join((' ' if op == 'C' else op).ljust(n) for (_, _, op), n in zip(cols, w)).rstrip())


def format_result(level, costs, speakers, overall, details):
    """result.txt of one level ('token' / 'word'): the header that says what was computed, the table, the aligned utterances with errors."""
    out = ['%s-level scores.  Alignment costs: substitution %d, insertion %d, deletion %d%s.' % (
               level, costs[0], costs[1], costs[2], ' (the NIST weights)' if tuple(costs) == DEFAULT_COSTS else ''),
           'Minimal cost, then fewest errors, then diagonal before deletion before insertion; costs 1,1,1 give the Levenshtein distance.',
           'Where alignments tie another scorer may count C/S/D/I differently: equality with an external scorer is not claimed, none was run.',
           '',
           '%-20s %6s %8s %7s %7s %7s %7s %7s %7s %7s' % ('SPKR', '#Snt', '#Tok', 'Corr', 'Sub', 'Del', 'Ins', 'Err', 'S.Err', 'Oracle')]
    pct = lambda a, b: 100.0 * a / max(b, 1)
    def line(name, t):
        return '%-20s %6d %8d %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f %7.1f' % (name[:20], t['#snt'], t['#tok'], pct(t['C'], t['#tok']), pct(t['S'], t['#tok']),
                                                                       pct(t['D'], t['#tok']), pct(t['I'], t['#tok']), 100 * t['err'], 100 * t['serr'],
                                                                       100 * t['oracle_err'])
    out += [line(s, t) for s, t in speakers.items()]
    out += ['-' * 92, line('Sum/Avg', overall), '']
    for utt, c, lines in details:
        out += ['%s  C=%d S=%d D=%d I=%d' % (utt, c['C'], c['S'], c['D'], c['I'])] + list(lines) + ['']
    return '\n'.join(out) + '\n'


def _score_level(utts, names, refs, nbests, tokens_of, costs, device):
    """One level: refs[u] / nbests[u] label lists -> (per utterance, speakers, overall, details for result.txt)."""
    hyps = [h for nb in nbests for h in nb]
    pair_ref = [u for u, nb in enumerate(nbests) for _ in nb]
    counts, paths = align(refs, hyps, pair_ref, costs, paths=True, device=device)
    per_utt, details, pos = {}, [], 0
    for u, utt in enumerate(names):
        rows = counts[pos:pos + len(nbests[u])]
        best = int(np.argmin(rows[:, 1]))          # the first of the fewest
        one, orc = _counts_dict(rows[0]), _counts_dict(rows[best])
        orc['rank'] = best
        per_utt[utt] = {'spk': utts[utt]['utt2spk'], 'ntok': len(refs[u]), '1best': one, 'oracle': orc}
        if one['errors'] > 0:
            details.append((utt, one, aligned_lines(tokens_of(refs[u]), tokens_of(nbests[u][0]), paths[pos])))
        pos += len(nbests[u])
    speakers, overall = summarise(per_utt)
    return per_utt, speakers, overall, details


def score(utts, char_list, out_dir, costs=DEFAULT_COSTS, device='cuda'):
    """Score the 'utts' dictionary of a result JSON; writes ref.trn, hyp.trn, score.json and result.txt under ``out_dir`` and returns
    score.json's content."""
    odim = len(char_list)
    names = sorted(utts)
    refs = [labels_of(_ids(utts[u]['output'][0]['tokenid']), odim) for u in names]
    nbests = [[labels_of(h, odim) for h in nbest_ids(utts[u])] for u in names]
    for u, r, nb in zip(names, refs, nbests):
        if max([len(r)] + [len(h) for h in nb]) > MAX_LEN:
            raise lib.Re2eError('utterance %s has a sequence of more than %d labels: the aligner does not take it' % (u, MAX_LEN))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'ref.trn'), 'w', encoding='utf-8') as fr, open(os.path.join(out_dir, 'hyp.trn'), 'w', encoding='utf-8') as fh:
        for u, r, nb in zip(names, refs, nbests):
            fr.write(trn_line([char_list[t] for t in r], utts[u]['utt2spk'], u))
            fh.write(trn_line([char_list[t] for t in nb[0]], utts[u]['utt2spk'], u))
    per_utt, speakers, overall, details = _score_level(utts, names, refs, nbests, lambda ids: [char_list[t] for t in ids], costs, device)
    report = {'costs': {'substitution': costs[0], 'insertion': costs[1], 'deletion': costs[2]}, 'utts': per_utt, 'speakers': speakers,
              'overall': overall}
    text = format_result('token', costs, speakers, overall, details)
    if SPACE in char_list:
        vocab = {}
        ids_of = lambda labels: [vocab.setdefault(w, len(vocab)) for w in words_of(labels, char_list)]
        wrefs, wnb = [ids_of(r) for r in refs], [[ids_of(h) for h in nb] for nb in nbests]
        words = sorted(vocab, key=vocab.get)
        w_utt, w_spk, w_all, w_det = _score_level(utts, names, wrefs, wnb, lambda ids: [words[t] for t in ids], costs, device)
        report['word'] = {'utts': w_utt, 'speakers': w_spk, 'overall': w_all}
        text += '\n' + format_result('word', costs, w_spk, w_all, w_det)
    with open(os.path.join(out_dir, 'score.json'), 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1, sort_keys=True, ensure_ascii=False)
    with open(os.path.join(out_dir, 'result.txt'), 'w', encoding='utf-8') as f:
        f.write(text)
    return report
