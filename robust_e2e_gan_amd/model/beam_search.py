"""Beam-search decoding: Decoder.recognize_beam (model/e2e_decoder.py:171-369, no LM) with
CTCPrefixScore (model/e2e_ctc.py:78-155) and end_detect (model/e2e_common.py:226-252).

The reference advances one hypothesis at a time (B = 1 attention / LSTMCell / output-layer calls, ``beam`` of them
per output position).  Here all live hypotheses of a position form ONE batch on the GPU: a single AttLoc step,
LSTMCell, output layer and row-wise log-softmax for the whole beam, one device->host copy of the (beam, V) local
scores per position; the search bookkeeping (pruning, length penalties, end detection) stays on the host and follows the
reference line by line, so the n-best lists agree.

Joint CTC/attention decoding: the CTC prefix scores of ALL live hypotheses x their ``ctc_beam`` candidate labels are one
launch per position (re2e_ctc_prefix_score: top-k pre-selection, Algorithm 2's recursion with the forward variables in
LDS / registers, the combined local score); the hypotheses' CTC states never leave the GPU and only
3 x nh x ctc_beam numbers (candidate labels, local scores, prefix scores) are copied to the host per position -- instead of
the (nh, V) attention scores plus a numpy recursion per hypothesis.  ``ctc_beam`` > 64 (ctc_weight == 1.0 scores all V
labels upstream, e2e_decoder.py:233-234) takes its candidate list from a device-side stable sort of the attention scores
(re2e_ctc_prefix_score_cands, one thread per candidate).  The host scorer below -- upstream's own numpy algorithm -- is kept as the
tests' arbiter (HOST_CTC_SCORER).

RNNLM shallow fusion (e2e_decoder.py:270-272,284-285; model/lm.py here): the LM is fed the last label of every live hypothesis
in one ``predict`` call per position, its four state tensors (nh, n_units) stay on the device and follow the survivors through the
same ``parents`` gather as the decoder state.  Attention-only search ranks ``att + lm_weight * lm`` over all V labels; with CTC
the candidates are chosen on the attention scores alone and ``lm_weight * lm[cand]`` is added to their local scores -- on the
device-CTC path by re2e_lm_add_cands before the 3 x nh x ctc_beam copy, so the LM's (nh, V) rows never cross to the host there.
The LM may also be a word-level one (model/extlm.py: LookAheadWordLM, MultiLevelLM over a lexical tree on the device): its state is a dict of
per-row tensors like the RNNLM's and takes the same gather; it is handed the labels of the position as the host array they were uploaded from
(``labels=``), so that it knows which rows stand at a <space> -- the only ones its word LM advances for -- without a device->host copy.

Decoders of more than one layer (dlayers > 1): the attention step and the first LSTMCell are layer 0's, as for one layer; the layers above advance
by one launch each per position (ops.dec_upper_step: re2e_dec_upper_step, whose rows do not depend on each other bit for bit), the output layer reads
the top one, and every layer's (z_l, c_l) follows the survivors through the ``parents`` gather.  With one layer nothing is launched that was not.

Several utterances per search (``recognize_beam_batch``, E2E.recognize_batch): one loop over output positions drives all unfinished
utterances.  The rows of a position are their live hypotheses, grouped by utterance; an utterance whose own ``end_detect`` fires, whose
hypotheses run out or that reaches its own ``maxlen`` leaves and its rows are compacted away.  The encoder states and ``mlp_enc`` projections
are held once per utterance in (U, T'max, .) buffers and read through a row -> utterance map (re2e_attloc_fwd_rows) instead of being
replicated per hypothesis; the prefix scorer takes the same map and every utterance's own frame count (re2e_ctc_prefix_score_batch); and
the pruning -- the per-hypothesis top-k plus the repeated ``sorted(kept)[:beam]`` below -- is re2e_beam_prune, which orders the survivors of
an utterance exactly as that host loop does (score descending, then parent row ascending, then local score descending, then column
ascending).  The (nh, V) scores never leave the device: one copy of the (U_live, beam) survivor arrays (parent row, column, label, score,
and on the joint path their prefix scores) crosses per position.  Every score is rounded as on the single-utterance path, so the n-best
lists are those of ``recognize_beam`` utterance by utterance.  ``ctc_beam`` > 64 (ctc_weight == 1.0) and ``beam_size`` > 64 are beyond the
kernels' limits: there the batch is a loop over ``recognize_beam``."""
import numpy as np
import torch

from .. import ops
from ..lib import ATT_KINDS, call
from .e2e_common import host_to_dev, lens_dev

CTC_SCORING_RATIO = 1.5          # e2e_decoder.py:20
LOGZERO = -10000000000.0


class CTCPrefixScore(object):
    """Log prefix probabilities of ``y + [c]`` for the candidate labels ``cs`` given the frame posteriors ``x`` (T, V)
    (Watanabe et al., "Hybrid CTC/attention architecture ...", Algorithm 2, evaluated for all candidates at once)."""

    def __init__(self, x, blank, eos):
        self.x, self.blank, self.eos, self.T = x, blank, eos, len(x)

    def initial_state(self):
        r = np.full((self.T, 2), LOGZERO, dtype=np.float32)
        r[:, 1] = np.cumsum(self.x[:, self.blank], dtype=np.float32)
        return r

    def __call__(self, y, cs, r_prev):
        n = len(y) - 1                                   # output length without <sos>
        xs = self.x[:, cs]
        r = np.empty((self.T, 2, len(cs)), dtype=np.float32)
        if n == 0:
            r[0, 0], r[0, 1] = xs[0], LOGZERO
        else:
            r[n - 1] = LOGZERO
        r_sum = np.logaddexp(r_prev[:, 0], r_prev[:, 1])
        log_phi = np.repeat(r_sum[:, None], len(cs), 1)
        if n > 0:
            log_phi[:, cs == y[-1]] = r_prev[:, 1:2]     # a repeated label needs a blank in between
        start = max(n, 1)
        log_psi = r[start - 1, 0].copy()
        xb = self.x[:, self.blank]
        for t in range(start, self.T):
            r[t, 0] = np.logaddexp(r[t - 1, 0], log_phi[t - 1]) + xs[t]
            r[t, 1] = np.logaddexp(r[t - 1, 0], r[t - 1, 1]) + xb[t]
            log_psi = np.logaddexp(log_psi, log_phi[t - 1] + xs[t])
        log_psi[cs == self.eos] = r_sum[-1]
        return log_psi, np.moveaxis(r, 2, 0)


def end_detect(ended, i, M=3, D_end=np.log(1 * np.exp(-10))):
    if not ended:
        return False
    best = max(h['score'] for h in ended)
    count = 0
    for m in range(M):
        same = [h['score'] for h in ended if len(h['yseq']) == i - m]
        if same and max(same) - best < D_end:
            count += 1
    return count == M


def _topk(row, k):
    idx = np.argsort(-row, kind='stable')[:k]
    return row[idx], idx


DEVICE_CTC_MAX_BEAM = 64        # re2e_ctc_prefix_score: one thread per candidate label, <= 64 candidates per hypothesis (in-kernel top-k);
#                                 more candidates (ctc_weight == 1.0: all V labels): re2e_ctc_prefix_score_cands on a device-sorted list
HOST_CTC_SCORER = False         # tests: upstream's numpy CTCPrefixScore on the host instead (the arbiter of the device scorers)


def _att_setup(p, prefix):
    """The attention type of the parameter dict and its step's parameters (None where the type has none)."""
    from .e2e_decoder import att_kind, att_params
    kind = att_kind(p, prefix)
    ap = att_params(p, prefix, kind)
    return kind, ap


def _att_step(kind, ap, pre, enc, z, state, hl, w_decT, nh, T, E, D, A, utt=None, U=0):
    """One attention step for the ``nh`` live rows -> (context (nh,E), the rows' new attention state).  The state is what the search
    gathers by ``parents`` beside z and c: the attention weights for ``location``, the row's own cov = cov_0 + w_0 + ... for the coverage
    types (None = the uniform first row, made by the kernels), nothing for ``dot`` and ``add``.  ``utt`` (nh) / ``U``: the rows share U
    utterances (re2e_*_fwd_rows) and ``hl`` (U) holds their frame counts; without it row r reads pre[r] / enc[r]."""
    dev = z.device
    w_new, cx = torch.empty(nh, T, device=dev), torch.empty(nh, E, device=dev)
    dpj, e_scr = torch.empty(nh, A, device=dev), torch.empty(nh, T, device=dev)
    st = state.data_ptr() if state is not None else None
    if kind in ('location', 'coverage_location'):
        C, Fh = ap['loc_conv'].shape[0], (ap['loc_conv'].shape[3] - 1) // 2
        conv = torch.empty(nh, T, C, device=dev)
        if utt is None:
            call('re2e_attloc_fwd', pre.data_ptr(), enc.data_ptr(), z.data_ptr(), st, hl.data_ptr(), w_decT.data_ptr(), ap['mlp_att'].data_ptr(),
                 ap['loc_conv'].data_ptr(), ap['gvec_w'].data_ptr(), ap['gvec_b'].data_ptr(), nh, T, E, D, A, C, Fh, w_new.data_ptr(), cx.data_ptr(), E,
                 conv.data_ptr(), dpj.data_ptr(), e_scr.data_ptr())
        else:
            call('re2e_attloc_fwd_rows', pre.data_ptr(), enc.data_ptr(), U, hl.data_ptr(), utt.data_ptr(), z.data_ptr(), st, w_decT.data_ptr(),
                 ap['mlp_att'].data_ptr(), ap['loc_conv'].data_ptr(), ap['gvec_w'].data_ptr(), ap['gvec_b'].data_ptr(), nh, T, E, D, A, C, Fh,
                 w_new.data_ptr(), cx.data_ptr(), E, conv.data_ptr(), dpj.data_ptr(), e_scr.data_ptr())
        if kind == 'location':
            return cx, w_new
        cov = torch.empty(nh, T, device=dev)
        call('re2e_attstep_cov_add', st, w_new.data_ptr(), hl.data_ptr(), utt.data_ptr() if utt is not None else None, U if utt is not None else nh,
             nh, T, cov.data_ptr())
        return cx, cov
    K = ATT_KINDS[kind]
    opt = lambda k: ap[k].data_ptr() if k in ap else None
    cov = torch.empty(nh, T, device=dev) if kind == 'coverage' else None
    if utt is None:
        call('re2e_attstep_fwd', K, pre.data_ptr(), enc.data_ptr(), z.data_ptr(), st, hl.data_ptr(), w_decT.data_ptr(), opt('mlp_dec_b'), opt('wvec_w'),
             opt('wvec_b'), opt('gvec_w'), opt('gvec_b'), nh, T, E, D, A, w_new.data_ptr(), cx.data_ptr(), E, cov.data_ptr() if cov is not None else None,
             dpj.data_ptr(), e_scr.data_ptr())
    else:
        call('re2e_attstep_fwd_rows', K, pre.data_ptr(), enc.data_ptr(), U, hl.data_ptr(), utt.data_ptr(), z.data_ptr(), st, w_decT.data_ptr(),
             opt('mlp_dec_b'), opt('wvec_w'), opt('wvec_b'), opt('gvec_w'), opt('gvec_b'), nh, T, E, D, A, w_new.data_ptr(), cx.data_ptr(), E,
             cov.data_ptr() if cov is not None else None, dpj.data_ptr(), e_scr.data_ptr())
    return cx, cov


def _upper_setup(p, prefix):
    """The decoder layers above layer 0 (dlayers > 1): one dict of w_ih, w_hh, b_ih, b_hh per layer; empty for a single-layer decoder."""
    from .e2e_decoder import upper_layers
    return upper_layers(p, prefix)


def _upper_step(upper, state, z0, nh, D):
    """One position of the upper layers for the ``nh`` live rows, one launch per layer (ops.dec_upper_step: re2e_dec_upper_step): layer l reads
    the new state of the layer below and its own (z_l, c_l) of ``state`` -> the rows' new [(z_l, c_l)], gathered by ``parents`` beside the
    attention state."""
    new, x = [], z0
    for lay, (zl, cl) in zip(upper, state):
        zn, cn = torch.empty(nh, D, device=z0.device), torch.empty(nh, D, device=z0.device)
        ops.dec_upper_step(lay, x, zl, cl, zn, cn, nh, D)
        new.append((zn, cn))
        x = zn
    return new


def recognize_beam(p, h, lpz, recog_args, eos, prefix='', lpz_dev=None, rnnlm=None):
    """``p``: reference-named decoder / attention Parameters; ``h``: (T, eprojs) encoder states of ONE utterance on the
    GPU; ``lpz``: (T, V) CTC log posteriors (numpy) or None; ``rnnlm``: a model.lm.ClassifierWithState on the same device or None
    (``recog_args.lm_weight`` is read only with one).  Returns the n-best list of {'yseq', 'score'}."""
    dev = h.device
    T, E = h.shape
    beam, penalty, ctc_weight = recog_args.beam_size, recog_args.penalty, recog_args.ctc_weight
    embed, w_ih, w_hh = p[prefix + 'dec.embed.weight'], p[prefix + 'dec.decoder.0.weight_ih'], p[prefix + 'dec.decoder.0.weight_hh']
    b_ih, b_hh = p[prefix + 'dec.decoder.0.bias_ih'], p[prefix + 'dec.decoder.0.bias_hh']
    out_w, out_b = p[prefix + 'dec.output.weight'], p[prefix + 'dec.output.bias']
    kind, ap = _att_setup(p, prefix)
    upper = _upper_setup(p, prefix)
    mlp_dec = ap['mlp_dec']
    V, Dd, D, A = out_w.shape[0], embed.shape[1], w_hh.shape[1], mlp_dec.shape[0]
    ldw = Dd + E
    lm_weight = np.float32(recog_args.lm_weight) if rnnlm is not None else None
    lm_state = None
    with torch.no_grad():
        pre1 = ops.linear(h.unsqueeze(0), p[prefix + 'att.mlp_enc.weight'], p[prefix + 'att.mlp_enc.bias'],
                          act='tanh' if kind == 'dot' else None)                                               # (1,T,A)
        h_rep = h.unsqueeze(0).expand(beam, T, E).contiguous()          # every hypothesis attends over the same utterance
        pre_rep = pre1.expand(beam, T, A).contiguous()
        hl = lens_dev([T] * beam, dev)
        w_decT = torch.empty(D, A, device=dev)
        call('re2e_transpose01', mlp_dec.data_ptr(), w_decT.data_ptr(), A, D, 1)
        w_ctx = w_ih.data_ptr() + 4 * Dd
        maxlen = T if recog_args.maxlenratio == 0 else max(1, int(recog_args.maxlenratio * T))
        minlen = int(recog_args.minlenratio * T)
        hyps = [{'score': np.float32(0.0), 'yseq': [eos], 'parent': 0}]
        dev_ctc = False
        if lpz is not None:
            ctc = CTCPrefixScore(lpz, 0, eos)
            hyps[0]['ctc_state'], hyps[0]['ctc_score'] = ctc.initial_state(), np.float32(0.0)
            ctc_beam = min(V, int(beam * CTC_SCORING_RATIO)) if ctc_weight != 1.0 else V
            dev_ctc = not HOST_CTC_SCORER
            if dev_ctc:
                lpz_d = lpz_dev.float().contiguous() if lpz_dev is not None else torch.from_numpy(np.ascontiguousarray(lpz, np.float32)).to(dev)
                r_prev = torch.from_numpy(hyps[0].pop('ctc_state')).to(dev).view(1, T, 2)      # states stay on the device from here on
        z, c, a_prev = torch.zeros(1, D, device=dev), torch.zeros(1, D, device=dev), None
        up_state = [(torch.zeros(1, D, device=dev), torch.zeros(1, D, device=dev)) for _ in upper]
        ended = []
        for i in range(maxlen):
            nh = len(hyps)
            ids_h = np.asarray([hp['yseq'][i] for hp in hyps], np.int32)
            ids = host_to_dev(ids_h, dev)
            emb = torch.empty(nh, Dd, device=dev)
            call('re2e_embedding_fwd', embed.data_ptr(), ids.data_ptr(), nh, Dd, emb.data_ptr(), Dd)
            cx, a_new = _att_step(kind, ap, pre_rep, h_rep, z, a_prev, hl, w_decT, nh, T, E, D, A)
            gates = torch.empty(nh, 4 * D, device=dev)
            ops.gemm(emb, w_ih, gates, nh, 4 * D, Dd, transb=True, ldb=ldw, bias=b_ih, bias2=b_hh)
            ops.gemm(cx, w_ctx, gates, nh, 4 * D, E, transb=True, ldb=ldw, beta=1.0, dev=dev)
            ops.gemm(z, w_hh, gates, nh, 4 * D, D, transb=True, beta=1.0)
            z_new, c_new = torch.empty(nh, D, device=dev), torch.empty(nh, D, device=dev)
            call('re2e_lstm_cell_fwd', gates.data_ptr(), c.data_ptr(), c_new.data_ptr(), z_new.data_ptr(), nh, D)
            up_new = _upper_step(upper, up_state, z_new, nh, D)
            z_top = up_new[-1][0] if upper else z_new
            logits, lsm = torch.empty(nh, V, device=dev), torch.empty(nh, V, device=dev)
            ops.gemm(z_top, out_w, logits, nh, V, D, transb=True, bias=out_b)
            call('re2e_log_softmax_rows', logits.data_ptr(), nh, V, V, lsm.data_ptr())
            if rnnlm is not None:
                # att + lm_weight * lm over all V labels is what an attention-only search ranks (e2e_decoder.py:272,291); with CTC only the
                # candidates' LM scores are used (:284-285)
                lm_state, lm_lp, att_lm = rnnlm.predict_combined(lm_state, ids, lsm if lpz is None else None, lm_weight, labels=ids_h)
            if dev_ctc:
                last = host_to_dev(np.asarray([hp['yseq'][-1] for hp in hyps], np.int32), dev)
                if max(len(hp['yseq']) - 1 for hp in hyps) > T:
                    # CTCPrefixScore indexes r[output_length - 1] over the T frames (e2e_ctc.py:128-133): a hypothesis longer than
                    # the utterance has frames (maxlenratio > 1) is an IndexError upstream
                    raise IndexError('CTC prefix score: hypothesis of %d labels on %d encoder frames (lower maxlenratio)'
                                     % (max(len(hp['yseq']) - 1 for hp in hyps), T))
                olen = host_to_dev(np.asarray([len(hp['yseq']) - 1 for hp in hyps], np.int32), dev)
                prev = host_to_dev(np.asarray([hp['ctc_score'] for hp in hyps], np.float32), dev, torch.float32)
                out_d = torch.empty(2, nh, ctc_beam, device=dev)                  # [0] local scores, [1] prefix scores
                r_new = torch.empty(nh * ctc_beam, 2 * T, device=dev)
                if ctc_beam <= DEVICE_CTC_MAX_BEAM:
                    cand_d = torch.empty(nh, ctc_beam, dtype=torch.int32, device=dev)
                    call('re2e_ctc_prefix_score', lpz_d.data_ptr(), T, V, lsm.data_ptr(), nh, r_prev.data_ptr(), last.data_ptr(), olen.data_ptr(),
                         prev.data_ptr(), ctc_beam, float(np.float32(1.0 - ctc_weight)), float(np.float32(ctc_weight)), 0, eos, cand_d.data_ptr(),
                         out_d[0].data_ptr(), out_d[1].data_ptr(), r_new.data_ptr())
                else:
                    # the candidates in the order torch.topk / _topk give them: attention score descending, ties -> lower label (stable sort;
                    # NaN scores last, as the kernel's own selection ranks them)
                    order = torch.sort(torch.nan_to_num(lsm, nan=float('-inf')), dim=1, descending=True, stable=True)[1]
                    cand_d = order[:, :ctc_beam].to(torch.int32).contiguous()
                    call('re2e_ctc_prefix_score_cands', lpz_d.data_ptr(), T, V, lsm.data_ptr(), nh, r_prev.data_ptr(), last.data_ptr(), olen.data_ptr(),
                         prev.data_ptr(), cand_d.data_ptr(), ctc_beam, float(np.float32(1.0 - ctc_weight)), float(np.float32(ctc_weight)), 0, eos,
                         out_d[0].data_ptr(), out_d[1].data_ptr(), r_new.data_ptr())
                if rnnlm is not None:
                    call('re2e_lm_add_cands', out_d[0].data_ptr(), lm_lp.data_ptr(), cand_d.data_ptr(), nh, ctc_beam, V, float(lm_weight))
                cand_all, out_all = cand_d.cpu().numpy(), out_d.cpu().numpy()      # 3 x nh x ctc_beam numbers: this position's host round trip
            else:
                local_all = (lsm if rnnlm is None or lpz is not None else att_lm).cpu().numpy()   # the (nh, V) local scores cross once per position
                lm_all = lm_lp.cpu().numpy() if rnnlm is not None and lpz is not None else None   # host CTC scorer (the arbiter) only
            kept = []
            for k, hyp in enumerate(hyps):
                if dev_ctc:
                    best_scores, joint = _topk(out_all[0, k], beam)
                    for j in range(len(joint)):
                        kept.append({'score': np.float32(hyp['score'] + best_scores[j]), 'yseq': hyp['yseq'] + [int(cand_all[k, joint[j]])],
                                     'parent': k, 'ctc_row': k * ctc_beam + int(joint[j]), 'ctc_score': out_all[1, k, joint[j]]})
                    kept = sorted(kept, key=lambda x: x['score'], reverse=True)[:beam]
                    continue
                local_att = local_all[k]
                if lpz is not None:
                    _, cand = _topk(local_att, ctc_beam)
                    ctc_scores, ctc_states = ctc(hyp['yseq'], cand, hyp['ctc_state'])
                    local = (np.float32(1.0 - ctc_weight) * local_att[cand] + np.float32(ctc_weight) * (ctc_scores - hyp['ctc_score'])).astype(np.float32)
                    if lm_all is not None:
                        local = (local + lm_weight * lm_all[k][cand]).astype(np.float32)
                    best_scores, joint = _topk(local, beam)
                    best_ids = cand[joint]
                else:
                    best_scores, best_ids = _topk(local_att, beam)
                    joint = None
                for j in range(len(best_ids)):
                    new = {'score': np.float32(hyp['score'] + best_scores[j]), 'yseq': hyp['yseq'] + [int(best_ids[j])], 'parent': k}
                    if lpz is not None:
                        new['ctc_state'], new['ctc_score'] = ctc_states[joint[j]], ctc_scores[joint[j]]
                    kept.append(new)
                kept = sorted(kept, key=lambda x: x['score'], reverse=True)[:beam]
            hyps = kept
            if i == maxlen - 1:
                for hyp in hyps:
                    hyp['yseq'].append(eos)
            remained = []
            for hyp in hyps:
                if hyp['yseq'][-1] == eos:
                    if len(hyp['yseq']) > minlen:
                        hyp['score'] = np.float32(hyp['score'] + (i + 1) * penalty)
                        ended.append(hyp)
                else:
                    remained.append(hyp)
            if end_detect(ended, i) and recog_args.maxlenratio == 0.0:
                break
            hyps = remained
            if not hyps:
                break
            parents = host_to_dev(np.asarray([hp['parent'] for hp in hyps], np.int64), dev, torch.int64)
            z, c = z_new.index_select(0, parents), c_new.index_select(0, parents)
            a_prev = a_new.index_select(0, parents) if a_new is not None else None
            up_state = [(zl.index_select(0, parents), cl.index_select(0, parents)) for zl, cl in up_new]
            if lm_state is not None:
                lm_state = {key: v.index_select(0, parents) for key, v in lm_state.items()}
            if dev_ctc:                                                   # the survivors' CTC states, gathered on the device
                rows = host_to_dev(np.asarray([hp['ctc_row'] for hp in hyps], np.int64), dev, torch.int64)
                r_prev = r_new.index_select(0, rows)
        best = sorted(ended, key=lambda x: x['score'], reverse=True)[:min(len(ended), recog_args.nbest)]
        return [{'yseq': b['yseq'], 'score': float(b['score'])} for b in best]


BATCH_MAX_BEAM = 64             # re2e_beam_prune: beam <= 64, at most `beam` rows per utterance


def _final_nbest(ended, nbest):
    best = sorted(ended, key=lambda x: x['score'], reverse=True)[:min(len(ended), nbest)]
    return [{'yseq': b['yseq'], 'score': float(b['score'])} for b in best]


def recognize_beam_batch(p, hs, lpzs, recog_args, eos, prefix='', rnnlm=None):
    """``hs``: list of U (T'_u, eprojs) encoder-state tensors on the GPU; ``lpzs``: list of U (T'_u, V) CTC log posteriors on the same
    device, or None; the rest as ``recognize_beam``.  Returns U n-best lists, element u being what ``recognize_beam`` returns for
    utterance u alone."""
    U = len(hs)
    if U == 0:
        return []
    dev = hs[0].device
    E = hs[0].shape[1]
    Ts = [int(h.shape[0]) for h in hs]
    Tmax = max(Ts)
    beam, penalty, ctc_weight = recog_args.beam_size, recog_args.penalty, recog_args.ctc_weight
    out_w = p[prefix + 'dec.output.weight']
    V = out_w.shape[0]
    joint = lpzs is not None
    ctc_beam = (min(V, int(beam * CTC_SCORING_RATIO)) if ctc_weight != 1.0 else V) if joint else 0
    if beam > BATCH_MAX_BEAM or ctc_beam > DEVICE_CTC_MAX_BEAM or (joint and HOST_CTC_SCORER):
        # beyond the batched kernels' limits (ctc_weight == 1.0 scores all V labels), or the tests' host scorer: the same result, one utterance
        # at a time
        return [recognize_beam(p, hs[u], lpzs[u].detach().cpu().numpy() if joint else None, recog_args, eos, prefix,
                               lpz_dev=lpzs[u] if joint else None, rnnlm=rnnlm) for u in range(U)]
    embed, w_ih, w_hh = p[prefix + 'dec.embed.weight'], p[prefix + 'dec.decoder.0.weight_ih'], p[prefix + 'dec.decoder.0.weight_hh']
    b_ih, b_hh = p[prefix + 'dec.decoder.0.bias_ih'], p[prefix + 'dec.decoder.0.bias_hh']
    out_b = p[prefix + 'dec.output.bias']
    kind, ap = _att_setup(p, prefix)
    upper = _upper_setup(p, prefix)
    mlp_dec = ap['mlp_dec']
    Dd, D, A = embed.shape[1], w_hh.shape[1], mlp_dec.shape[0]
    ldw = Dd + E
    lm_weight = np.float32(recog_args.lm_weight) if rnnlm is not None else None
    lm_state = None
    kk = min(beam, ctc_beam if joint else V)
    with torch.no_grad():
        # one copy of every utterance's states and projections, zero rows beyond its length; the projection is the single-utterance
        # search's own product, utterance by utterance
        enc, pre = torch.zeros(U, Tmax, E, device=dev), torch.zeros(U, Tmax, A, device=dev)
        for u, h in enumerate(hs):
            enc[u, :Ts[u]] = h
            pre[u, :Ts[u]] = ops.linear(h.unsqueeze(0), p[prefix + 'att.mlp_enc.weight'], p[prefix + 'att.mlp_enc.bias'],
                                        act='tanh' if kind == 'dot' else None)[0]
        tl = lens_dev(Ts, dev)
        w_decT = torch.empty(D, A, device=dev)
        call('re2e_transpose01', mlp_dec.data_ptr(), w_decT.data_ptr(), A, D, 1)
        w_ctx = w_ih.data_ptr() + 4 * Dd
        maxlen = [T if recog_args.maxlenratio == 0 else max(1, int(recog_args.maxlenratio * T)) for T in Ts]
        minlen = [int(recog_args.minlenratio * T) for T in Ts]
        hyps = [[{'score': np.float32(0.0), 'yseq': [eos]}] for _ in range(U)]
        ended = [[] for _ in range(U)]
        if joint:
            lpz_d = torch.zeros(U, Tmax, V, device=dev)
            for u in range(U):
                lpz_d[u, :Ts[u]] = lpzs[u].float()
            blank_col = lpz_d[:, :, 0].cpu().numpy()                        # CTCPrefixScore.initial_state, per utterance (once per search)
            r0 = np.full((U, Tmax, 2), LOGZERO, dtype=np.float32)
            for u in range(U):
                r0[u, :Ts[u], 1] = np.cumsum(blank_col[u, :Ts[u]], dtype=np.float32)
                hyps[u][0]['ctc_score'] = np.float32(0.0)
            r_prev = torch.from_numpy(r0).to(dev)
        live = list(range(U))
        z, c, a_prev = torch.zeros(U, D, device=dev), torch.zeros(U, D, device=dev), None
        up_state = [(torch.zeros(U, D, device=dev), torch.zeros(U, D, device=dev)) for _ in upper]
        i = 0
        while live:
            rows = [(u, hp) for u in live for hp in hyps[u]]
            nh, nl = len(rows), len(live)
            seg = np.zeros(nl + 1, np.int32)
            seg[1:] = np.cumsum([len(hyps[u]) for u in live])
            meta = np.empty((3, nh), np.int32)                              # last label, utterance, output length: one upload
            meta[0] = [hp['yseq'][i] for _, hp in rows]
            meta[1] = [u for u, _ in rows]
            meta[2] = [len(hp['yseq']) - 1 for _, hp in rows]
            meta_d = host_to_dev(meta, dev)
            ids, utt, olen = meta_d[0], meta_d[1], meta_d[2]
            seg_d = host_to_dev(seg, dev)
            hsc = host_to_dev(np.asarray([hp['score'] for _, hp in rows], np.float32), dev, torch.float32)
            emb = torch.empty(nh, Dd, device=dev)
            call('re2e_embedding_fwd', embed.data_ptr(), ids.data_ptr(), nh, Dd, emb.data_ptr(), Dd)
            cx, a_new = _att_step(kind, ap, pre, enc, z, a_prev, tl, w_decT, nh, Tmax, E, D, A, utt=utt, U=U)
            gates = torch.empty(nh, 4 * D, device=dev)
            ops.gemm(emb, w_ih, gates, nh, 4 * D, Dd, transb=True, ldb=ldw, bias=b_ih, bias2=b_hh)
            ops.gemm(cx, w_ctx, gates, nh, 4 * D, E, transb=True, ldb=ldw, beta=1.0, dev=dev)
            ops.gemm(z, w_hh, gates, nh, 4 * D, D, transb=True, beta=1.0)
            z_new, c_new = torch.empty(nh, D, device=dev), torch.empty(nh, D, device=dev)
            call('re2e_lstm_cell_fwd', gates.data_ptr(), c.data_ptr(), c_new.data_ptr(), z_new.data_ptr(), nh, D)
            up_new = _upper_step(upper, up_state, z_new, nh, D)
            z_top = up_new[-1][0] if upper else z_new
            logits, lsm = torch.empty(nh, V, device=dev), torch.empty(nh, V, device=dev)
            ops.gemm(z_top, out_w, logits, nh, V, D, transb=True, bias=out_b)
            call('re2e_log_softmax_rows', logits.data_ptr(), nh, V, V, lsm.data_ptr())
            if rnnlm is not None:
                lm_state, lm_lp, att_lm = rnnlm.predict_combined(lm_state, ids, lsm if not joint else None, lm_weight, labels=meta[0])
            # the survivors: parent row, column, label, score (and their prefix scores), one int32 buffer -> one copy to the host
            surv = torch.empty(5 * nl * beam + nl, dtype=torch.int32, device=dev)
            part = [surv[k * nl * beam:(k + 1) * nl * beam] for k in range(5)]
            count_d = surv[5 * nl * beam:]
            ws = torch.empty(2 * nh * kk, dtype=torch.int32, device=dev)
            if joint:
                for u in live:
                    longest = max(len(hp['yseq']) - 1 for hp in hyps[u])
                    if longest > Ts[u]:
                        # CTCPrefixScore indexes r[output_length - 1] over the utterance's frames (e2e_ctc.py:128-133): IndexError upstream
                        raise IndexError('CTC prefix score: utterance %d: hypothesis of %d labels on %d encoder frames (lower maxlenratio)'
                                         % (u, longest, Ts[u]))
                prev = host_to_dev(np.asarray([hp['ctc_score'] for _, hp in rows], np.float32), dev, torch.float32)
                out_d = torch.empty(2, nh, ctc_beam, device=dev)                  # [0] local scores, [1] prefix scores
                r_new = torch.empty(nh * ctc_beam, 2 * Tmax, device=dev)
                cand_d = torch.empty(nh, ctc_beam, dtype=torch.int32, device=dev)
                call('re2e_ctc_prefix_score_batch', lpz_d.data_ptr(), U, Tmax, V, tl.data_ptr(), utt.data_ptr(), lsm.data_ptr(), nh, r_prev.data_ptr(),
                     ids.data_ptr(), olen.data_ptr(), prev.data_ptr(), ctc_beam, float(np.float32(1.0 - ctc_weight)), float(np.float32(ctc_weight)), 0, eos,
                     cand_d.data_ptr(), out_d[0].data_ptr(), out_d[1].data_ptr(), r_new.data_ptr())
                if rnnlm is not None:
                    call('re2e_lm_add_cands', out_d[0].data_ptr(), lm_lp.data_ptr(), cand_d.data_ptr(), nh, ctc_beam, V, float(lm_weight))
                local, cand_ptr, ncand = out_d[0], cand_d.data_ptr(), ctc_beam
            else:
                local, cand_ptr, ncand = (lsm if rnnlm is None else att_lm), None, V
            call('re2e_beam_prune', seg_d.data_ptr(), nl, int(max(len(hyps[u]) for u in live)), hsc.data_ptr(), local.data_ptr(), cand_ptr, nh, ncand, beam,
                 part[0].data_ptr(), part[1].data_ptr(), part[2].data_ptr(), part[3].data_ptr(), count_d.data_ptr(), ws.data_ptr(), ws.numel() * 4)
            if joint:
                at = part[0].clamp(min=0).long() * ctc_beam + part[1].clamp(min=0).long()          # (parent, column) in the scorer's outputs
                part[4].view(torch.float32).copy_(out_d[1].reshape(-1).index_select(0, at))
            surv_h = surv.cpu().numpy()                                       # this position's host round trip
            sv = surv_h[:5 * nl * beam].reshape(5, nl, beam)
            sv_f = sv.view(np.float32)
            counts = surv_h[5 * nl * beam:]
            keep_rows, keep_ctc, still = [], [], []
            for j, u in enumerate(live):
                base = int(seg[j])
                new = []
                for k in range(int(counts[j])):
                    par = int(sv[0, j, k])
                    hyp = {'score': sv_f[3, j, k], 'yseq': hyps[u][par - base]['yseq'] + [int(sv[2, j, k])], 'parent': par}
                    if joint:
                        hyp['ctc_row'], hyp['ctc_score'] = par * ctc_beam + int(sv[1, j, k]), sv_f[4, j, k]
                    new.append(hyp)
                last = i == maxlen[u] - 1
                if last:
                    for hyp in new:
                        hyp['yseq'].append(eos)
                remained = []
                for hyp in new:
                    if hyp['yseq'][-1] == eos:
                        if len(hyp['yseq']) > minlen[u]:
                            hyp['score'] = np.float32(hyp['score'] + (i + 1) * penalty)
                            ended[u].append(hyp)
                    else:
                        remained.append(hyp)
                if (end_detect(ended[u], i) and recog_args.maxlenratio == 0.0) or not remained or last:
                    hyps[u] = []
                    continue
                hyps[u] = remained
                still.append(u)
                keep_rows.extend(hp['parent'] for hp in remained)
                if joint:
                    keep_ctc.extend(hp['ctc_row'] for hp in remained)
            live = still
            i += 1
            if not live:
                break
            parents = host_to_dev(np.asarray(keep_rows, np.int64), dev, torch.int64)
            z, c = z_new.index_select(0, parents), c_new.index_select(0, parents)
            a_prev = a_new.index_select(0, parents) if a_new is not None else None
            up_state = [(zl.index_select(0, parents), cl.index_select(0, parents)) for zl, cl in up_new]
            if lm_state is not None:
                lm_state = {key: v.index_select(0, parents) for key, v in lm_state.items()}
            if joint:
                r_prev = r_new.index_select(0, host_to_dev(np.asarray(keep_ctc, np.int64), dev, torch.int64))
        return [_final_nbest(ended[u], recog_args.nbest) for u in range(U)]
