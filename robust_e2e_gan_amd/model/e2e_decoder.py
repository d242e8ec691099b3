"""Attention decoder (mirror of Decoder.__init__/forward, model/e2e_decoder.py:27-168)."""
import random

import numpy as np
import torch

from .. import ops
from ..lib import Re2eError
from .e2e_common import LinearParams, host_to_dev, lens_dev, lens_list


class LSTMCellParams(torch.nn.Module):
    """nn.LSTMCell's parameter names: weight_ih (4H, I), weight_hh (4H, H), bias_ih, bias_hh."""

    def __init__(self, idim, hdim):
        super().__init__()
        b = 1.0 / np.sqrt(hdim)
        self.weight_ih = torch.nn.Parameter(torch.empty(4 * hdim, idim).uniform_(-b, b))
        self.weight_hh = torch.nn.Parameter(torch.empty(4 * hdim, hdim).uniform_(-b, b))
        self.bias_ih = torch.nn.Parameter(torch.empty(4 * hdim).uniform_(-b, b))
        self.bias_hh = torch.nn.Parameter(torch.empty(4 * hdim).uniform_(-b, b))


class EmbeddingParams(torch.nn.Module):
    def __init__(self, n, d):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(n, d))


# the decoder loop's names (ops.DecoderLoopFn) of an attention's parameters <- their state_dict names under ``att.``
ATT_PARAMS = {
    'location': dict(mlp_dec='mlp_dec.weight', mlp_att='mlp_att.weight', loc_conv='loc_conv.weight', gvec_w='gvec.weight', gvec_b='gvec.bias'),
    'coverage_location': dict(mlp_dec='mlp_dec.weight', mlp_att='mlp_att.weight', loc_conv='loc_conv.weight', gvec_w='gvec.weight', gvec_b='gvec.bias'),
    'add': dict(mlp_dec='mlp_dec.weight', gvec_w='gvec.weight', gvec_b='gvec.bias'),
    'coverage': dict(mlp_dec='mlp_dec.weight', wvec_w='wvec.weight', wvec_b='wvec.bias', gvec_w='gvec.weight', gvec_b='gvec.bias'),
    'dot': dict(mlp_dec='mlp_dec.weight', mlp_dec_b='mlp_dec.bias'),
}
ATT_KIND = 'att.kind'        # key of the attention type in a parameter dict handed to decoder_forward_hip / the beam search


def att_kind(p, prefix=''):
    """The attention type of a parameter dict: what its owner wrote under ATT_KIND, ``location`` without it (callers from before the
    other types existed)."""
    return p.get(prefix + ATT_KIND, 'location')


def att_params(p, prefix, kind):
    if kind not in ATT_PARAMS:
        raise Re2eError('attention type %r has no decoder step here (location, dot, add, coverage, coverage_location)' % (kind,))
    return {k: p[prefix + 'att.' + name] for k, name in ATT_PARAMS[kind].items()}


def upper_layers(p, prefix=''):
    """The decoder layers above layer 0 of a parameter dict, as ops.DecoderLoopFn / DecoderUpperFn / the beam search take them: one dict
    (w_ih, w_hh, b_ih, b_hh) per ``dec.decoder.{l}``, l = 1, 2, ... as far as the dict has them (none: a single-layer decoder)."""
    lays, l = [], 1
    while prefix + 'dec.decoder.%d.weight_ih' % l in p:
        q = prefix + 'dec.decoder.%d.' % l
        lays.append(dict(w_ih=p[q + 'weight_ih'], w_hh=p[q + 'weight_hh'], b_ih=p[q + 'bias_ih'], b_hh=p[q + 'bias_hh']))
        l += 1
    return lays


def decoder_forward_hip(p, hpad, hlens, ys, eos, ss_rate=0.0, return_att=False, prefix='', greedy=False, labeldist=None, lsm_weight=0.0):
    """Decoder pass on the GPU.  ``p`` maps reference state_dict names (att.* / dec.*) to Parameters; ``ys`` is a
    list of 1-D label tensors (host or device).  Teacher forced, except at the steps where scheduled sampling
    fires (e2e_decoder.py:123: ``random.random() < rate and i > 0`` -- one draw of Python's RNG per step, for the
    whole batch) or, with ``greedy`` (calculate_all_attentions :408-412), at every step i > 0.  With ``dec.decoder.1.*`` ... in ``p`` (dlayers > 1)
    the layers above layer 0 follow the loop (teacher forced: ops.DecoderUpperFn on the loop's states) or run inside it (sampled steps: the fed
    token is the arg-max of the output layer on the TOP layer's state); logits, loss and accuracy read the top layer."""
    dev = hpad.device
    B, T, E = hpad.shape
    hl = lens_list(hlens)
    hl_dev = lens_dev(hl, dev)
    ylist = [[int(v) for v in y.tolist()] for y in ys]
    L1 = max(len(y) for y in ylist) + 1
    ids_in = np.full((B, L1), eos, np.int32)         # pad_list(ys_in, eos)   :97
    ids_out = np.full((B, L1), -1, np.int32)         # pad_list(ys_out, -1)   :98
    for b, y in enumerate(ylist):
        ids_in[b, 1:len(y) + 1] = y
        ids_out[b, :len(y)] = y
        ids_out[b, len(y)] = eos
    ids_tm = host_to_dev(np.ascontiguousarray(ids_in.T).reshape(-1), dev)
    tgt_tm = host_to_dev(np.ascontiguousarray(ids_out.T).reshape(-1), dev)
    hmask = ops.mask_rows(hpad, hl_dev)                                            # :85
    kind = att_kind(p, prefix)
    # dot: the encoder side of the product is tanh(mlp_enc(h)), once per batch (AttDot.forward :111-112)
    pre = ops.linear(hmask, p[prefix + 'att.mlp_enc.weight'], p[prefix + 'att.mlp_enc.bias'], act='tanh' if kind == 'dot' else None)
    Pm = dict(embed=p[prefix + 'dec.embed.weight'], w_ih=p[prefix + 'dec.decoder.0.weight_ih'], w_hh=p[prefix + 'dec.decoder.0.weight_hh'],
              b_ih=p[prefix + 'dec.decoder.0.bias_ih'], b_hh=p[prefix + 'dec.decoder.0.bias_hh'])
    Pm.update(att_params(p, prefix, kind))
    if greedy:
        sample_steps = tuple(i > 0 for i in range(L1))
    else:
        sample_steps = tuple((random.random() < ss_rate) and i > 0 for i in range(L1)) if ss_rate > 0.0 else None
    if sample_steps is not None and any(sample_steps):
        Pm.update(out_w=p[prefix + 'dec.output.weight'], out_b=p[prefix + 'dec.output.bias'])
    else:
        sample_steps = None
    ops.mark_grad(pre, 'pre (decoder loop bwd done)')
    ops.mark('decoder loop starts')
    upper = upper_layers(p, prefix)
    if not upper:
        z_all, w_all = ops.decoder_loop(hmask, pre, ids_tm, hl_dev, L1, Pm, sample_steps, False, kind)   # (L1,B,D), (L1,B,T)
    elif sample_steps is None:
        z0, w_all = ops.decoder_loop(hmask, pre, ids_tm, hl_dev, L1, Pm, None, False, kind)              # layer 0 keeps its loop
        z_all = ops.decoder_upper(z0, upper)
    else:
        z_all, w_all = ops.decoder_loop(hmask, pre, ids_tm, hl_dev, L1, Pm, sample_steps, False, kind, upper)
    ops.mark('decoder loop fwd done')
    ops.mark_grad(z_all, 'decoder states (output layer + CE bwd done: loop bwd starts)')
    D = z_all.shape[2]
    logits = ops.linear(z_all.reshape(L1 * B, D), p[prefix + 'dec.output.weight'], p[prefix + 'dec.output.bias'])
    scale = float(np.mean([len(y) + 1 for y in ylist])) - 1.0                      # :159
    loss, stats = ops.cross_entropy(logits, tgt_tm, scale)
    if labeldist is not None:                                                      # :162-166 label smoothing
        reg = ops.label_smoothing(logits, labeldist, B)
        loss = (1.0 - lsm_weight) * loss + lsm_weight * reg
    acc = stats[1] / stats[2]                                                      # th_accuracy (device scalar)
    if return_att:
        return loss.view(()), acc, w_all.transpose(0, 1)
    return loss.view(()), acc


class Decoder(torch.nn.Module):
    def __init__(self, eprojs, odim, dlayers, dunits, sos, eos, att, verbose=0, char_list=None, labeldist=None, lsm_weight=0.,
                 fusion=None, rnnlm=None, model_unit='char', space_loss_weight=0.1):
        super(Decoder, self).__init__()
        if dlayers < 1:
            raise Re2eError('dlayers = %r: the decoder needs at least one layer' % (dlayers,))
        self.labeldist, self.lsm_weight, self.vlabeldist = labeldist, lsm_weight, None
        self.dunits, self.dlayers = dunits, dlayers
        self.embed = EmbeddingParams(odim, dunits)
        self.decoder = torch.nn.ModuleList([LSTMCellParams(dunits + eprojs, dunits)] + [LSTMCellParams(dunits, dunits) for _ in range(1, dlayers)])
        self.output = LinearParams(dunits, odim)
        self.att = att
        self.sos, self.eos = sos, eos
        self.fusion = fusion
        self.ignore_id = -1
        self.loss = None
        self.return_acc_tensor = False

    def forward(self, hpad, hlen, ys, scheduled_sampling_rate=0.0, att_params=None):
        p = {'dec.' + k: v for k, v in self.named_parameters() if not k.startswith('att.')}
        p.update({'att.' + k: v for k, v in self.att.named_parameters()})
        p[ATT_KIND] = getattr(self.att, 'kind', 'location')
        if self.labeldist is not None and (self.vlabeldist is None or self.vlabeldist.device != hpad.device):
            self.vlabeldist = torch.as_tensor(np.asarray(self.labeldist), dtype=torch.float32).to(hpad.device).contiguous()
        loss, acc = decoder_forward_hip(p, hpad, hlen, ys, self.eos, scheduled_sampling_rate, labeldist=self.vlabeldist,
                                        lsm_weight=self.lsm_weight)
        self.loss = loss
        return loss, (acc if self.return_acc_tensor else float(acc))

    def _check_decode_lm(self, rnnlm, fstlm, device):
        """What recognize_beam and recognize_beam_batch accept as a decode-time LM: a ClassifierWithState over an RNNLM, over an FSRNNLM
        (model/fsrnn.py), over a word-level LM of model/extlm.py (LookAheadWordLM, MultiLevelLM) or over an n-gram LM (model/ngram.py NgramLM),
        shallow fusion only."""
        if fstlm is not None:
            raise Re2eError('decode-time LM: only RNNLM shallow fusion (rnnlm=ClassifierWithState(RNNLM(...))) is supported; '
                            'n-gram / FST LMs (fstlm) are out of scope')
        if rnnlm is not None:
            from .extlm import LookAheadWordLM, MultiLevelLM
            from .fsrnn import FSRNNLM
            from .lm import RNNLM, ClassifierWithState
            from .ngram import NgramLM
            if self.fusion in ('deep_fusion', 'cold_fusion'):
                raise Re2eError("decode-time LM: only shallow fusion is supported; fusion=%r changes the trained decoder and is out of scope"
                                % self.fusion)
            if not isinstance(rnnlm, ClassifierWithState) or not isinstance(rnnlm.predictor, (RNNLM, FSRNNLM, LookAheadWordLM, MultiLevelLM, NgramLM)):
                raise Re2eError('decode-time LM: only a ClassifierWithState over an RNNLM, an FSRNNLM, a LookAheadWordLM or a MultiLevelLM is '
                                'supported (shallow fusion); n-gram LMs and %s are out of scope' % type(rnnlm).__name__)
            pred, V = rnnlm.predictor, self.output.weight.shape[0]
            if isinstance(pred, RNNLM):
                labels, lm_device, what = pred.n_vocab, pred.lo.weight.device, 'RNNLM'
            elif isinstance(pred, FSRNNLM):
                labels, lm_device, what = pred.n_vocab, pred.out.weight.device, 'FSRNNLM'
            elif isinstance(pred, NgramLM):
                labels, lm_device, what = pred.n_vocab, pred.device, 'NgramLM'
            else:
                labels, lm_device, what = pred.subword_dict_size, pred.device, type(pred).__name__
                if any(prm.device != lm_device for prm in pred.parameters()):
                    raise Re2eError('the language models of the %s are on different devices' % what)
            if labels != V:
                raise Re2eError('the %s has %d labels, the decoder %d' % (what, labels, V))
            if lm_device != device:
                raise Re2eError('the %s is on %s, the encoder states on %s' % (what, lm_device, device))
            if rnnlm.training or any(mod.training for mod in pred.modules()):
                raise Re2eError('the %s must be in evaluation mode (rnnlm.eval())' % what)

    def recognize_beam(self, h, lpz, recog_args, char_list=None, rnnlm=None, fstlm=None):
        """e2e_decoder.py:171-369: n-best list of {'yseq', 'score'} for the encoder states ``h`` (T', eprojs) of one
        utterance; ``lpz`` = CTC log posteriors (T', V) or None.  All live hypotheses are advanced as one GPU batch.
        ``rnnlm``: a model.lm.ClassifierWithState over an RNNLM, or over a word-level LM of model/extlm.py, for shallow fusion with weight
        ``recog_args.lm_weight`` (:270-272,284-285); no other LM is supported."""
        self._check_decode_lm(rnnlm, fstlm, h.device)
        from .beam_search import recognize_beam
        p = {'dec.' + k: v for k, v in self.named_parameters() if not k.startswith('att.')}
        p.update({'att.' + k: v for k, v in self.att.named_parameters()})
        p[ATT_KIND] = getattr(self.att, 'kind', 'location')
        lp = lpz.detach().cpu().numpy() if isinstance(lpz, torch.Tensor) else lpz
        return recognize_beam(p, h, lp, recog_args, self.eos, lpz_dev=lpz if isinstance(lpz, torch.Tensor) and lpz.is_cuda else None, rnnlm=rnnlm)

    def recognize_beam_batch(self, hs, lpzs, recog_args, char_list=None, rnnlm=None, fstlm=None):
        """``recognize_beam`` for several utterances in one search: ``hs`` = list of (T'_u, eprojs) encoder states on the GPU, ``lpzs`` = list
        of (T'_u, V) CTC log posteriors on the same device or None.  Returns one n-best list per utterance, each what ``recognize_beam``
        returns for that utterance alone; the live hypotheses of all unfinished utterances advance as one GPU batch and are pruned on the
        device (model/beam_search.py recognize_beam_batch)."""
        if len(hs) == 0:
            return []
        self._check_decode_lm(rnnlm, fstlm, hs[0].device)
        if lpzs is not None and len(lpzs) != len(hs):
            raise Re2eError('recognize_beam_batch: %d utterances but %d CTC posterior matrices' % (len(hs), len(lpzs)))
        from .beam_search import recognize_beam_batch
        p = {'dec.' + k: v for k, v in self.named_parameters() if not k.startswith('att.')}
        p.update({'att.' + k: v for k, v in self.att.named_parameters()})
        p[ATT_KIND] = getattr(self.att, 'kind', 'location')
        return recognize_beam_batch(p, [h.float().contiguous() for h in hs], lpzs, recog_args, self.eos, rnnlm=rnnlm)

    def calculate_all_attentions(self, hpad, hlen, ys):
        """e2e_decoder.py:371-461 -- attention weights (B, Lmax+1, T').  NB the reference's pass is GREEDY: for i > 0 it
        feeds the arg-max of its own previous output (:408-412), the labels only fix the number of steps."""
        p = {'dec.' + k: v for k, v in self.named_parameters() if not k.startswith('att.')}
        p.update({'att.' + k: v for k, v in self.att.named_parameters()})
        p[ATT_KIND] = getattr(self.att, 'kind', 'location')
        with torch.no_grad():
            _, _, att = decoder_forward_hip(p, hpad, hlen, ys, self.eos, 0.0, return_att=True, greedy=True)
        return att.cpu().numpy()
